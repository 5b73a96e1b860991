"""Timing probe: device fill_holes (levels 1-2) at the bench config, against
the same call without fill in the same run (the pipeline as it was).

Volume: the benchmark's 512^3 uint64 chunk with seeded background cavities
and swallowed blobs punched into cells that are wide enough to hold them
(the Voronoi cells themselves enclose nothing). Device: one warm-up call
then 5 timed device_only calls each with fill_holes 0, 1 and 2, each with
a real H2D (fill forbids skip_h2d); reports mean ms_fill, ms_total of the
filled meshing and ms_total of the hole meshing, plus the productive
rounds from one standalone fill_holes call per level.
Host: the numpy/scipy checker (tests/fill_holes_ref.py) on the 128^3
corner of the same volume — a DIFFERENT size, reported as such and not
extrapolated.

    python tools/probe_fill_holes.py [--no-host] [--out FILE]
"""
import argparse
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np
from igneous_amd.engine import Engine

ap = argparse.ArgumentParser()
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


import bench
data = bench.bench_input().copy(order="F")

# punch: a 5^3 probe box that lies inside ONE cell gets its inner 3^3
# turned into background (cavity) or into a fresh label (swallowed blob)
rng = np.random.default_rng(41)
fresh = int(data.max()) + 1
ncav = nblob = 0
for k, (x, y, z) in enumerate(rng.integers(4, 508, size=(40000, 3))):
    box = data[x - 2:x + 3, y - 2:y + 3, z - 2:z + 3]
    L = box[0, 0, 0]
    if L == 0 or not np.all(box == L):
        continue
    if k % 2:
        box[1:4, 1:4, 1:4] = 0
        ncav += 1
    else:
        box[1:4, 1:4, 1:4] = fresh
        fresh += 1
        nblob += 1
say(f"volume {data.shape} {data.dtype}: {ncav} cavities and {nblob} "
    f"swallowed blobs of 27 voxels punched in")

eng = Engine.get(0)
res = (16., 16., 40.)


def timed(level):
    kw = {"fill_holes": level} if level else {}
    eng.mesh_chunk(data, resolution=res, device_only=True, **kw)
    acc = {"ms_fill": 0.0, "ms_total": 0.0, "holes_ms_total": 0.0}
    for _ in range(5):
        eng.mesh_chunk(data, resolution=res, device_only=True, **kw)
        first = eng.last_fill_stats if level else eng.stats()
        acc["ms_fill"] += first["ms_fill"] / 5
        acc["ms_total"] += first["ms_total"] / 5
        if level:
            acc["holes_ms_total"] += eng.stats()["ms_total"] / 5
    return acc, first


for level in (0, 1, 2):
    acc, st = timed(level)
    msg = (f"device fill_holes={level}: ms_fill {acc['ms_fill']:.2f}, "
           f"ms_total {acc['ms_total']:.2f} (labels {st['n_labels']}, "
           f"tris {st['total_tris']})")
    if level:
        filled, holes, rounds = eng.fill_holes(data, level)
        msg += (f", hole meshing ms_total {acc['holes_ms_total']:.2f}, "
                f"productive rounds {rounds} (+1 to see the fixed point), "
                f"{np.count_nonzero(filled != data)} voxels rewritten, "
                f"{np.count_nonzero(holes)} non-zero hole voxels")
        del filled, holes
    say(msg)

if not args.no_host:
    import fill_holes_ref as R
    small = np.asfortranarray(data[:128, :128, :128])
    for level in (1, 2):
        t0 = time.perf_counter()
        f, h, r = R.fill_holes_ref(small, level)
        dt = time.perf_counter() - t0
        say(f"host checker at 128^3 (1/64 of the voxels, not extrapolated) "
            f"fill_holes={level}: {dt:.2f} s, productive rounds {r}, "
            f"{np.count_nonzero(f != small)} voxels rewritten")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
