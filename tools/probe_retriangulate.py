"""Timing probe: the device retriangulation (mg_retriangulate_mesh) against
the route it replaces, same host, same run.

(a) the previous product route: Engine.chunk_mesh (device), Mesh.concatenate
    and meshops.merge_close_vertices (host);
(b) Engine.retriangulate_mesh: one device call.
Also the weld alone, on each row's concatenated mesh:
Engine.merge_close_vertices against meshops.merge_close_vertices.

Meshes and grids are the four rows of tools/probe_chunk_mesh.py: the label
with the most faces of the benchmark chunk (bench.bench_input()) and the
chunk's labels in ascending order concatenated until --big-faces faces are
reached, each on a grid of about 8 cells and on one whose cells are 1.37
voxels wide and anchored off the voxel grid. Whole calls on every side (the
engine's include validation, H2D, D2H and the copy-out), one warm-up then
--reps timed. Reports the median and max-min of each side, the difference
against three times the larger spread, and whether the results are equal.

    python tools/probe_retriangulate.py [--big-faces N] [--reps N]
                                        [--out FILE]
"""
import argparse
import sys
import time

sys.path.insert(0, ".")
import numpy as np
from igneous_amd import meshops
from igneous_amd.engine import Engine
from igneous_amd.meshes import Mesh

ap = argparse.ArgumentParser()
ap.add_argument("--big-faces", type=int, default=40000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--radius", type=float, default=1e-5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


import bench
eng = Engine.get(0)
meshes = eng.mesh_chunk(bench.bench_input(), resolution=bench.RESOLUTION)
label = max(meshes, key=lambda k: meshes[k][1].shape[0])
verts, faces = (np.ascontiguousarray(a) for a in meshes[label])
bv, bf, nv, nf = [], [], 0, 0
for lab in sorted(meshes):
    v, f = meshes[lab]
    bv.append(v)
    bf.append(f + np.uint32(nv))
    nv += v.shape[0]
    nf += f.shape[0]
    if nf >= args.big_faces:
        break
bverts, bfaces, nlab = np.concatenate(bv), np.concatenate(bf), len(bv)
del meshes

res = np.asarray(bench.RESOLUTION, dtype=np.float64)
FINE = ("cells 1.37 voxels wide, off the voxel grid", 1.37 * res,
        np.array([3.1, 5.3, 7.7]))


def coarse(v):
    lo, hi = v.min(axis=0), v.max(axis=0)
    return ("about 8 cells", (hi - lo).astype(np.float64) / 2 + 1.0,
            lo.astype(np.float64) - 0.5)


def timed(fn):
    out = fn()  # warm-up
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, float(np.median(ts)) * 1e3, (max(ts) - min(ts)) * 1e3


def same(a, b):
    return (a[0].shape == b[0].shape and a[1].shape == b[1].shape
            and np.array_equal(np.ascontiguousarray(a[0]).view(np.uint32),
                               np.ascontiguousarray(b[0]).view(np.uint32))
            and np.array_equal(a[1], b[1]))


def verdict(name_a, am, asp, name_b, bm, bsp):
    need = 3 * max(asp, bsp)
    return (f"{name_a}/{name_b} {am / bm:.1f}x; difference {am - bm:.3f} ms "
            f"against 3 x larger spread {need:.3f} ms: "
            f"{'holds' if am - bm > need else 'DOES NOT HOLD'}")


def probe(name, verts, faces, grid):
    gname, scale, offset = grid
    r = args.radius

    def route_a():
        cells = eng.chunk_mesh(verts, faces, scale, offset)
        cat = Mesh.concatenate(*(Mesh(v, f) for v, f in cells.values()))
        m = meshops.merge_close_vertices(cat, radius=r)
        return m.vertices, m.faces

    def route_b():
        return eng.retriangulate_mesh(verts, faces, scale, offset, r)

    a, am, asp = timed(route_a)
    b, bm, bsp = timed(route_b)
    cells = eng.chunk_mesh(verts, faces, scale, offset)
    cat = Mesh.concatenate(*(Mesh(v, f) for v, f in cells.values()))
    say(f"{name}, grid '{gname}' scale {np.asarray(scale).tolist()}: "
        f"{len(cells)} cells, {cat.vertices.shape[0]} concatenated vertices, "
        f"{cat.faces.shape[0]} faces -> {b[0].shape[0]} vertices, "
        f"{b[1].shape[0]} faces; results equal: {same(a, b)}")
    say(f"  (a) Engine.chunk_mesh + concatenate + meshops.merge_close_vertices:"
        f" median {am:.3f} ms, max-min {asp:.3f} ms over {args.reps}")
    say(f"  (b) Engine.retriangulate_mesh: median {bm:.3f} ms, max-min "
        f"{bsp:.3f} ms over {args.reps}")
    say("  " + verdict("(a)", am, asp, "(b)", bm, bsp))
    h, hm, hsp = timed(lambda: (lambda m: (m.vertices, m.faces))(
        meshops.merge_close_vertices(cat, radius=r)))
    d, dm, dsp = timed(
        lambda: eng.merge_close_vertices(cat.vertices, cat.faces, r))
    say(f"  weld alone: host meshops.merge_close_vertices median {hm:.3f} ms,"
        f" max-min {hsp:.3f} ms; Engine.merge_close_vertices median "
        f"{dm:.3f} ms, max-min {dsp:.3f} ms; results equal: {same(h, d)}")
    say("  " + verdict("host", hm, hsp, "device", dm, dsp))


say(f"mesh: label {label}, {verts.shape[0]} vertices, {faces.shape[0]} faces;"
    f" big mesh: the first {nlab} labels concatenated, {bverts.shape[0]} "
    f"vertices, {bfaces.shape[0]} faces; radius {args.radius}")
for name, v, f in (("mesh", verts, faces), ("big mesh", bverts, bfaces)):
    for grid in (coarse(v), FINE):
        probe(name, v, f, grid)

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
