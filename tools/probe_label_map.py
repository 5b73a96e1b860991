"""Timing probe: device label map (remap_table / object_ids /
exclude_object_ids) at the bench config, against the host numpy sequence
it replaces.

Device: one warm-up call then 5 timed calls per map, device_only, each
with a real H2D (a map forbids skip_h2d); reports mean ms_labelmap and
ms_total. A dust_threshold run is included so that a kernel trace of this
script holds k_dust_zero next to k_label_map (same volume, same run).
Host: the igneous_amd/remap.py sequence at 256^3 (512^3 takes minutes;
multiply by 8 for the voxel count — an extrapolation, not a measurement).

    python tools/probe_label_map.py [--no-host] [--out FILE]
"""
import argparse
import sys
import time

sys.path.insert(0, ".")
import numpy as np
from igneous_amd import remap as R
from igneous_amd.engine import Engine
from igneous_amd.synth import voronoi_labels

ap = argparse.ArgumentParser()
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


import bench
data = bench.bench_input()  # voronoi_labels((512,)*3, 50000, 303, uint64)
# labels seen in a 1/64 subsample: enough to build the maps from
real = [int(x) for x in np.unique(data[::4, ::4, ::4]) if x != 0]
rng = np.random.default_rng(0)
say(f"volume {data.shape} {data.dtype}, {len(real)} labels sampled")

grouped = {r: real[i - i % 10] for i, r in enumerate(real)}
fill = np.unique(rng.integers(1, 1 << 40, size=2_100_000, dtype=np.uint64))
fill = fill[~np.isin(fill, np.asarray(real, dtype=np.uint64))]
fill = rng.permutation(fill)[:2_000_000 - len(real)]
big_keys = np.concatenate([np.asarray(real, dtype=np.uint64), fill])
maps = {
    "object_ids x8": R.fold_label_ops(None, real[:8], [], data.dtype),
    "object_ids x2048": R.fold_label_ops(None, real[:2048], [], data.dtype),
    "exclude x8": R.fold_label_ops(None, None, real[:8], data.dtype),
    f"remap {len(real)}->{len(set(grouped.values()))}":
        R.fold_label_ops(grouped, None, [], data.dtype),
    # identity on the real labels + absent filler keys (arrays built
    # directly: the fold's per-entry Python loop is not what is timed)
    f"remap {len(big_keys)} keys, mostly absent":
        (big_keys, big_keys.copy(), 'zero'),
}

eng = Engine.get(0)
res = (16., 16., 40.)


def timed(**kw):
    eng.mesh_chunk(data, resolution=res, device_only=True, **kw)
    acc = {"ms_labelmap": 0.0, "ms_total": 0.0, "ms_h2d": 0.0}
    for _ in range(5):
        eng.mesh_chunk(data, resolution=res, device_only=True, **kw)
        st = eng.stats()
        for k in acc:
            acc[k] += st[k] / 5
    return acc, st


acc, st = timed()
say(f"device no map: ms_total {acc['ms_total']:.2f} "
    f"(labels {st['n_labels']}, tris {st['total_tris']})")
acc, st = timed(dust_threshold=1000)
say(f"device dust_threshold=1000: ms_total {acc['ms_total']:.2f} "
    f"(labels {st['n_labels']})")
for name, lm in maps.items():
    acc, st = timed(label_map=lm)
    say(f"device {name} [n={len(lm[0])}, miss={lm[2]}]: "
        f"ms_labelmap {acc['ms_labelmap']:.3f}, "
        f"ms_total {acc['ms_total']:.2f} (labels {st['n_labels']})")

if not args.no_host:
    small = voronoi_labels((256, 256, 256), 1000, 202, dtype=np.uint64)
    sreal = [int(x) for x in np.unique(small) if x != 0]
    table = {r: sreal[i - i % 10] for i, r in enumerate(sreal)}
    table[0] = 0

    def host(name, fn):
        vol = small.copy()
        t0 = time.perf_counter()
        fn(vol)
        dt = time.perf_counter() - t0
        say(f"host 256^3 {name}: {dt:.2f} s "
            f"(x8 extrapolated to 512^3: {8 * dt:.1f} s)")

    host("mask_except x8", lambda v: R.mask_except(v, sreal[:8]))
    host("mask x8", lambda v: R.mask(v, sreal[:8]))
    host(f"mask_except + remap {len(sreal)}->{len(set(table.values())) - 1}",
         lambda v: R.remap(R.mask_except(v, list(table)), table))

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
