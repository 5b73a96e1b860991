"""Timing probe: the device encode stage against the host loop it replaces,
on one 256^3 synth chunk (the chunks256 bench's generator).

Two paths, interleaved in one session, one warm-up and five timed runs each:
  (a) mesh_chunk(copy=False) followed by MeshTask's per-label host loop
      (tasks.mesh.encode_fragment: shift, box, encode) — the path before
      the encode stage, still the fallback;
  (b) mesh_chunk_encoded(copy=False) followed by items() into dicts.
for precomputed and draco, simplification_factor 0 and 100. Reports the
median and max-min of each path's wall time and, for (b), the median
ms_encode and ms_d2h. Both paths include the upload of the chunk.

    python tools/probe_encode.py [--out FILE]
"""
import argparse
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
from igneous_amd.engine import Engine
from igneous_amd.meshes import Mesh
from igneous_amd.synth import voronoi_labels
from igneous_amd.tasks.draco import draco_encoding_settings
from igneous_amd.tasks.mesh import encode_fragment

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=5)
args = ap.parse_args()

lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


RES = (16.0, 16.0, 40.0)
data = voronoi_labels((256, 256, 256), 6250, 1000, dtype=np.uint64)
shift = (np.asarray([256, 512, 768], dtype=np.float32)
         * np.asarray(RES, dtype=np.float32))
draco = draco_encoding_settings(
    shape=(257, 257, 257), offset=(256, 512, 768), resolution=RES,
    compression_level=1, create_metadata=False)
draco['quantization_bits'] = int(draco['quantization_bits'])
eng = Engine.get(0)
say(f"volume {data.shape} {data.dtype}; runs {args.runs} after one warm-up; "
    f"times in ms (wall, upload included)")


def host_path(encoding, rf):
    t0 = time.perf_counter()
    raw = eng.mesh_chunk(data, resolution=RES, reduction_factor=rf,
                         max_error=40.0, copy=False)
    t1 = time.perf_counter()
    binaries, boxes = {}, {}
    for label, (v, f) in raw.items():
        binaries[label], boxes[label] = encode_fragment(
            Mesh(v, f, id=label), shift, encoding, draco)
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, (t2 - t1) * 1e3, binaries, boxes


def device_path(encoding, rf):
    t0 = time.perf_counter()
    ch = eng.mesh_chunk_encoded(data, resolution=RES, reduction_factor=rf,
                                max_error=40.0, shift=shift,
                                encoding=encoding, draco=draco, copy=False)
    t1 = time.perf_counter()
    binaries, boxes = {}, {}
    for label, b, box in ch.items():
        binaries[label] = b
        boxes[label] = box
    t2 = time.perf_counter()
    st = eng.stats()
    return ((t2 - t0) * 1e3, (t2 - t1) * 1e3, binaries, boxes,
            st["ms_encode"], st["ms_d2h"],
            (int(ch.nverts.sum()), int(ch.ntris.sum())))


def med(xs):
    return statistics.median(xs)


def spread(xs):
    return max(xs) - min(xs)


for encoding in ("precomputed", "draco"):
    for rf in (0, 100):
        _, _, hb, hx = host_path(encoding, rf)            # warm-up
        *_, db, dx, _, _, (V, T) = device_path(encoding, rf)  # warm-up
        same = (hb == db and hx == dx)
        a, a_loop, b, b_items, enc, d2h = [], [], [], [], [], []
        for _ in range(args.runs):                        # interleaved
            t, tl, _, _ = host_path(encoding, rf)
            a.append(t)
            a_loop.append(tl)
            t, ti, _, _, e, d, _ = device_path(encoding, rf)
            b.append(t)
            b_items.append(ti)
            enc.append(e)
            d2h.append(d)
        nbytes = sum(len(x) for x in db.values())
        wins = med(a) - med(b) > 3 * spread(a)
        say(f"{encoding} simplification_factor={rf}: labels {len(db)}, "
            f"blob {nbytes} B, bytes+boxes equal to the host loop: {same}")
        say(f"  (a) mesh_chunk + host loop : median {med(a):9.2f}  "
            f"max-min {spread(a):7.2f}  (loop alone {med(a_loop):9.2f})")
        say(f"  (b) mesh_chunk_encoded+items: median {med(b):9.2f}  "
            f"max-min {spread(b):7.2f}  (items alone {med(b_items):8.2f}; "
            f"ms_encode {med(enc):.3f}, ms_d2h {med(d2h):.3f})")
        say(f"  (a)-(b) = {med(a) - med(b):.2f} vs 3 x (a)'s max-min = "
            f"{3 * spread(a):.2f}: "
            f"{'device path faster' if wins else 'NOT faster by the rule'}; "
            f"encoded V {V}, T {T}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
