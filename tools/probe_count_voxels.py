"""Timing probe: mg_count_voxels at the bench config (the volume of
tools/probe_dust.py), volume resident (skip_h2d). Reports ms_count of each
run — the fused run-counting pass, kernels k_count_runs<T> (build + count
in one volume pass) and k_count_compact (one thread per hash slot) — next
to ms_total. For kernel times run it under
`rocprofv3 --kernel-trace --stats`; the pair of passes it replaces is
k_dust_build + k_dust_count of tools/probe_dust.py.

--check compares the result with np.unique; --dust-global times a
dust_global chunk call (count + lookup + mapped call on the counted volume)
against the same call on a volume the host masked first, uploaded normally.
"""
import argparse
import sys
import time

sys.path.insert(0, ".")
import numpy as np

from igneous_amd.engine import Engine
from igneous_amd.synth import voronoi_labels

KERNELS = ("k_count_runs", "k_count_compact")
RES = (16., 16., 40.)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--dust-global", action="store_true")
    args = ap.parse_args()

    data = voronoi_labels((512, 512, 512), 50000, 303, dtype=np.uint64)
    eng = Engine.get(0)
    values, counts = eng.count_voxels(data)       # upload + first launch
    print(f"kernels: {', '.join(KERNELS)}")
    print(f"volume {data.shape} {data.dtype}: {len(values)} values, "
          f"{int(counts[0]) if values[0] == 0 else 0} zero voxels")
    ms = []
    for i in range(args.runs):
        eng.count_voxels(data, skip_h2d=True)
        st = eng.stats()
        ms.append(st["ms_count"])
        print(f"run {i}: ms_count {st['ms_count']:.3f}  ms_total "
              f"{st['ms_total']:.3f}  labels {st['n_labels']}")
    print(f"ms_count median {np.median(ms):.3f}  min {min(ms):.3f}  "
          f"max {max(ms):.3f}")

    if args.check:
        t0 = time.perf_counter()
        u, c = np.unique(data, return_counts=True)
        dt = time.perf_counter() - t0
        ok = np.array_equal(values, u) and np.array_equal(counts, c)
        print(f"np.unique: {dt * 1e3:.0f} ms on the host, equal: {ok}")
        if not ok:
            sys.exit(1)

    if args.dust_global:
        thr = 1000
        table_keys = values
        table_vals = counts

        def lookup(labels):
            return table_vals[np.searchsorted(table_keys, labels)]
        nz = values != 0
        dust = values[nz & (counts < thr)]
        masked = data.copy(order="F")
        masked[np.isin(masked, dust)] = 0
        for name, fn in (
                ("dust_global", lambda: eng.mesh_chunk(
                    data, resolution=RES, device_only=True,
                    dust_global=(thr, lookup))),
                ("premasked ", lambda: eng.mesh_chunk(
                    masked, resolution=RES, device_only=True))):
            fn()
            wall, dev = [], []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                fn()
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(eng.stats()["ms_total"])
            st = eng.stats()
            print(f"{name}: call wall {np.median(wall):.2f} ms (min "
                  f"{min(wall):.2f} max {max(wall):.2f}), chunk call "
                  f"ms_total {np.median(dev):.2f}, labels {st['n_labels']}, "
                  f"tris {st['total_tris']}")


if __name__ == "__main__":
    main()
