"""Timing probe: device chunk_mesh (mg_chunk_mesh) against the host
function it replaces (meshops.chunk_mesh), same host, same run.

Mesh: the label with the most faces of the benchmark chunk
(bench.bench_input()), meshed once with the engine. Two grids: one of
about 8 cells (half the mesh's extent per axis) and one whose cells are
1.37 voxels wide and anchored off the voxel grid, so most faces cross a
boundary (marching-cubes faces are at most one voxel across and their
vertices sit on the half-voxel grid: a voxel-aligned grid cuts none of
them). Both sides: whole calls (the engine's include H2D and D2H), one
warm-up then 5 timed. Reports the median and max-min of each side and
checks that the two results are equal. --max-faces N keeps only the first
N faces (said in the output) if the host loop is too slow.

--big-faces N (default 40000, 0 = off) repeats both grids' cell sizes on
a mesh a merge task is more likely to see: the chunk's labels in
ascending order concatenated until N faces are reached, host timed 3
times.

    python tools/probe_chunk_mesh.py [--max-faces N] [--big-faces N]
                                     [--no-host] [--out FILE]
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
ap.add_argument("--max-faces", type=int, default=0)
ap.add_argument("--big-faces", type=int, default=40000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-host", action="store_true",
                help="time the device only (for a profiler run)")
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
verts, faces = meshes[label]
big = None
if args.big_faces:
    bv, bf, nv, nf = [], [], 0, 0
    for lab in sorted(meshes):
        v, f = meshes[lab]
        bv.append(v)
        bf.append(f + np.uint32(nv))
        nv += v.shape[0]
        nf += f.shape[0]
        if nf >= args.big_faces:
            break
    big = (np.concatenate(bv), np.concatenate(bf), len(bv))
del meshes
if args.max_faces and faces.shape[0] > args.max_faces:
    say(f"mesh cut down to its first {args.max_faces} of {faces.shape[0]} "
        f"faces")
    faces = faces[:args.max_faces]
    verts = verts[:int(faces.max()) + 1]
verts = np.ascontiguousarray(verts)
faces = np.ascontiguousarray(faces)
lo, hi = verts.min(axis=0), verts.max(axis=0)
say(f"mesh: label {label}, {verts.shape[0]} vertices, {faces.shape[0]} "
    f"faces, extent {(hi - lo).tolist()} nm")

res = np.asarray(bench.RESOLUTION, dtype=np.float64)
grids = [
    ("about 8 cells", (hi - lo).astype(np.float64) / 2 + 1.0,
     lo.astype(np.float64) - 0.5),
    ("cells 1.37 voxels wide, off the voxel grid", 1.37 * res,
     np.array([3.1, 5.3, 7.7])),
]


def spread(ts):
    return float(np.median(ts)) * 1e3, (max(ts) - min(ts)) * 1e3


def probe(name, verts, faces, scale, offset, host_reps, host_warm=True):
    mesh = Mesh(verts, faces, id=1)
    got = eng.chunk_mesh(verts, faces, scale, offset)  # warm-up
    dev = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        got = eng.chunk_mesh(verts, faces, scale, offset)
        dev.append(time.perf_counter() - t0)
    dm, ds = spread(dev)
    if args.no_host:
        say(f"grid '{name}' scale {np.asarray(scale).tolist()}: "
            f"{len(got)} cells; device whole call median {dm:.3f} ms, "
            f"max-min {ds:.3f} ms over {args.reps} (host not run)")
        return
    if host_warm:
        meshops.chunk_mesh(mesh, scale, offset)  # warm-up
    host = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        want = meshops.chunk_mesh(mesh, scale, offset)
        host.append(time.perf_counter() - t0)
    same = list(got) == list(want) and all(
        np.array_equal(got[k][1], want[k].faces)
        and np.array_equal(got[k][0].view(np.uint32),
                           want[k].vertices.view(np.uint32))
        for k in want)
    hm, hs = spread(host)
    reps = host_reps
    say(f"grid '{name}' scale {np.asarray(scale).tolist()}: {len(want)} "
        f"cells, {sum(len(m.faces) for m in want.values())} output faces, "
        f"results equal: {same}")
    say(f"  device whole call (H2D + kernels + D2H + copy-out): median "
        f"{dm:.3f} ms, max-min {ds:.3f} ms over {args.reps}")
    say(f"  host meshops.chunk_mesh: median {hm:.3f} ms, max-min "
        f"{hs:.3f} ms over {reps}")
    say(f"  host/device {hm / dm:.1f}x; difference {hm - dm:.3f} ms against "
        f"3 x larger spread {3 * max(ds, hs):.3f} ms")

for name, scale, offset in grids:
    probe(name, verts, faces, scale, offset, args.reps)

if big is not None:
    bverts, bfaces, nlab = big
    say(f"big mesh: the first {nlab} labels concatenated, "
        f"{bverts.shape[0]} vertices, {bfaces.shape[0]} faces (host "
        f"without warm-up, 3 timed)")
    blo, bhi = bverts.min(axis=0), bverts.max(axis=0)
    probe("big, about 8 cells", bverts, bfaces,
          (bhi - blo).astype(np.float64) / 2 + 1.0,
          blo.astype(np.float64) - 0.5, 3, host_warm=False)
    probe("big, " + grids[1][0], bverts, bfaces, grids[1][1], grids[1][2], 3,
          host_warm=False)

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
