"""Timing probe: one octree level of the multires merge in one device call
(mg_encode_octree_level) against the route it replaces, same host, same run.

(a) the previous product route, tasks.multires.encode_octree_level_host over
    the engine's seams: Engine.retriangulate_mesh and Engine.chunk_mesh
    (device, one upload and one download each, one array pair per cell), the
    cmp_zorder sort, then to_stored_model_space and formats.draco.encode per
    fragment (host);
(b) tasks.multires.engine_level_encoder: Engine.encode_octree_level, one
    device call, only the tables and the blob come back.

Meshes and grids are the four rows of tools/probe_chunk_mesh.py: the label
with the most faces of the benchmark chunk (bench.bench_input()) and the
chunk's labels in ascending order concatenated until --big-faces faces are
reached, each on a grid of about 8 cells and on one whose cells are 1.37
voxels wide and anchored off the voxel grid. Each row is a chunked level at
that grid, retriangulated first at twice the grid's resolution (cells half
as wide: the level below, as process_mesh pairs them). A fifth row is the
big mesh as the unchunked coarsest level, retriangulated at the coarse grid.
Whole calls on both sides, one warm-up each, then --reps timed runs with the
two routes interleaved. Reports the median and max-min of each side, the
difference against three times route (a)'s own spread (the rule of DESIGN.md
§4 "Device encode"), and whether nodes, sizes and bytes are equal.

    python tools/probe_octree_level.py [--big-faces N] [--reps N]
                                       [--bits N] [--out FILE]
"""
import argparse
import sys
import time

sys.path.insert(0, ".")
import numpy as np
from igneous_amd.engine import Engine
from igneous_amd.meshes import Mesh
from igneous_amd.tasks import multires

ap = argparse.ArgumentParser()
ap.add_argument("--big-faces", type=int, default=40000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--bits", type=int, default=16)
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


def probe(name, verts, faces, grid, chunked):
    gname, scale, offset = grid
    mesh = Mesh(verts, faces, id=1)
    # chunked: lod 1 of 3 with chunk_shape = scale / 2, so the level's grid
    # is `scale` and the retriangulation's is scale / 2; unchunked: lod 1 of
    # 2 with chunk_shape = scale, the retriangulation's grid
    chunk, num_lods = (np.asarray(scale) / 2, 3) if chunked \
        else (np.asarray(scale), 2)
    level_args = (mesh, chunk, 1, num_lods, offset, args.bits)
    routes = (multires.encode_octree_level_host,
              multires.engine_level_encoder)
    outs = [fn(*level_args) for fn in routes]  # warm-up
    ts = ([], [])
    for _ in range(args.reps):
        for i, fn in enumerate(routes):
            t0 = time.perf_counter()
            outs[i] = fn(*level_args)
            ts[i].append(time.perf_counter() - t0)
    (am, asp), (bm, bsp) = ((float(np.median(t)) * 1e3,
                             (max(t) - min(t)) * 1e3) for t in ts)
    a, b = outs
    equal = (tuple(a[0]) == tuple(b[0]) and list(a[1]) == list(b[1])
             and a[2] == b[2])
    what = f"chunked at scale {np.asarray(scale).tolist()}" if chunked \
        else "unchunked"
    say(f"{name}, grid '{gname}', {what}, retriangulated at "
        f"{chunk.tolist()}: {len(b[0])} fragments, {len(b[2])} bytes; "
        f"nodes, sizes and bytes equal: {equal}")
    say(f"  (a) retriangulate_mesh + chunk_mesh + sort + per-fragment "
        f"quantise and draco.encode: median {am:.3f} ms, max-min {asp:.3f} "
        f"ms over {args.reps}")
    say(f"  (b) Engine.encode_octree_level: median {bm:.3f} ms, max-min "
        f"{bsp:.3f} ms over {args.reps}")
    need = 3 * asp
    say(f"  (a)/(b) {am / bm:.1f}x; difference {am - bm:.3f} ms against 3 x "
        f"(a)'s spread {need:.3f} ms: "
        f"{'holds' if am - bm > need else 'DOES NOT HOLD'}")
    return equal and am - bm > need


say(f"mesh: label {label}, {verts.shape[0]} vertices, {faces.shape[0]} faces;"
    f" big mesh: the first {nlab} labels concatenated, {bverts.shape[0]} "
    f"vertices, {bfaces.shape[0]} faces; {args.bits} bits")
ok = True
for name, v, f in (("mesh", verts, faces), ("big mesh", bverts, bfaces)):
    for grid in (coarse(v), FINE):
        ok = probe(name, v, f, grid, True) and ok
ok = probe("big mesh", bverts, bfaces, coarse(bverts), False) and ok
say(f"every row equal and beyond the margin: {ok}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
