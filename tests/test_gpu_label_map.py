"""GPU tests (pytest -m gpu) of the device label map: mg_mesh_chunk_mapped
applies remap_table / object_ids / exclude_object_ids, folded into one
{key -> val} table + miss policy, in a HIP volume pass after dust and
before the count pass.

Checker for the preprocessing: the host sequence from igneous_amd/remap.py
(mask_except -> remap). Checker for the geometry: the CPU oracle on that
preprocessed volume. Equality is bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES = (16.0, 16.0, 40.0)


@pytest.fixture(scope="module")
def eng():
    from igneous_amd.engine import Engine
    return Engine.get(0)


def _assert_meshsets_equal(got: dict, want: dict, what=""):
    assert sorted(got.keys()) == sorted(want.keys()), \
        f"{what}: label sets differ ({len(got)} vs {len(want)})"
    for label in want:
        gv, gf = got[label]
        wv, wf = want[label]
        assert gv.shape == wv.shape, \
            f"{what} label {label}: nverts {gv.shape[0]} != {wv.shape[0]}"
        assert gf.shape == wf.shape, \
            f"{what} label {label}: ntris {gf.shape[0]} != {wf.shape[0]}"
        assert np.array_equal(gf, wf), f"{what} label {label}: faces differ"
        assert np.array_equal(gv, wv), f"{what} label {label}: verts differ"


def host_map(data, label_map):
    """(keys, vals, miss) applied with the host helpers MeshTask used
    before: 'zero' is mask_except(keys) -> remap, 'keep' is remap alone
    (remap leaves absent labels unchanged and looks each voxel up once)."""
    from igneous_amd import remap as R
    keys, vals, miss = label_map
    d = data.copy()
    table = dict(zip([int(k) for k in keys], [int(v) for v in vals]))
    if miss == 'zero':
        d = R.mask_except(d, list(table.keys()) + [0])
    return R.remap(d, table)


def _lm(keys, vals, miss):
    return (np.asarray(keys, dtype=np.uint64),
            np.asarray(vals, dtype=np.uint64), miss)


def _noise_volume(shape, dtype, seed):
    """Random per-voxel labels (every pair of labels is face-adjacent
    somewhere) with a zero border; u64 ids are sparse 40-bit values."""
    rng = np.random.default_rng(seed)
    if dtype == np.uint64:
        ids = rng.integers(1 << 33, 1 << 40, size=6).astype(np.uint64)
    else:
        ids = rng.integers(1, 1 << 31, size=6).astype(np.uint32)
    ids = np.concatenate([np.zeros(1, dtype), ids]).astype(dtype)
    assert len(set(ids.tolist())) == 7
    data = np.zeros(shape, dtype=dtype, order="F")
    inner = tuple(s - 2 for s in shape)
    data[1:-1, 1:-1, 1:-1] = ids[rng.integers(0, 7, size=inner)]
    return np.asfortranarray(data), [int(i) for i in ids[1:]]


def _tiny_volume(dtype):
    """3x3x3: smaller than one wave; slabs a|b|c along x, a and b
    face-adjacent, one background voxel."""
    a, b, c = (5, 9, 1 << 31) if dtype == np.uint32 else \
        (5, (1 << 39) + 3, (1 << 40) - 1)
    data = np.zeros((3, 3, 3), dtype=dtype, order="F")
    data[0], data[1], data[2] = a, b, c
    data[1, 1, 1] = 0
    return data, [a, b, c, a + 1, a + 2, a + 3]


VOLUMES = {
    "u64_40x37x29": lambda: _noise_volume((40, 37, 29), np.uint64, 123),
    # nvox = 24679 is odd: the vector pass leaves a scalar tail
    "u32_37x29x23": lambda: _noise_volume((37, 29, 23), np.uint32, 124),
    "u32_3x3x3": lambda: _tiny_volume(np.uint32),
    "u64_3x3x3": lambda: _tiny_volume(np.uint64),
}


@pytest.mark.parametrize("name", list(VOLUMES))
def test_engine_parity_with_host_preprocessing(eng, name):
    import oracle
    data, (a, b, c, d, e, f) = VOLUMES[name]()
    if name == "u32_37x29x23":
        assert data.size == 24679
    raw = data.copy()
    base = 1000 if data.dtype == np.uint32 else (1 << 36) + 1000
    fresh = next(x for x in range(base, base + 8)
                 if x not in (a, b, c, d, e, f))
    cases = {
        "keep_erase_only": _lm([a, c], [0, 0], 'keep'),
        "zero_identity": _lm([a, b], [a, b], 'zero'),
        # two face-adjacent labels become one: no interior faces remain
        "merge": _lm([a, b, c], [fresh, fresh, c], 'zero'),
        "chain": _lm([a, b], [b, c], 'keep'),
        "chain_zero": _lm([a, b], [b, c], 'zero'),
    }
    for what, lm in cases.items():
        want_vol = host_map(data, lm)
        got = eng.mesh_chunk(data, resolution=RES, label_map=lm)
        want = oracle.mesh_chunk(want_vol, resolution=RES)
        _assert_meshsets_equal(got, want, f"{name}/{what}")
        assert np.array_equal(data, raw), "host labels were modified"
    merged = eng.mesh_chunk(data, resolution=RES, label_map=cases["merge"])
    assert sorted(merged) == sorted({fresh, c})

    assert eng.mesh_chunk(data, resolution=RES,
                          label_map=_lm([], [], 'zero')) == {}
    assert eng.stats()['n_labels'] == 0
    plain = oracle.mesh_chunk(data, resolution=RES)
    _assert_meshsets_equal(
        eng.mesh_chunk(data, resolution=RES, label_map=_lm([], [], 'keep')),
        plain, f"{name}/empty_keep")
    _assert_meshsets_equal(
        eng.mesh_chunk(data, resolution=RES), plain, f"{name}/unmapped")
    assert eng.stats()['ms_labelmap'] == 0


# ---------------------------------------------------------------------------
# table sizes

@pytest.fixture(scope="module")
def vor48():
    """48^3 voronoi volume, its real labels, the group map every sized
    table applies to them (groups of three merge) and the oracle's meshes
    of the fully mapped volume — computed once, never modified."""
    import oracle
    from igneous_amd.synth import voronoi_labels
    data = voronoi_labels((48, 48, 48), 30, 77, dtype=np.uint64)
    real = [int(x) for x in np.unique(data) if x != 0]
    assert len(real) >= 20
    group = {r: real[i - i % 3] for i, r in enumerate(real)}
    full = _lm(list(group.keys()), list(group.values()), 'zero')
    want = oracle.mesh_chunk(host_map(data, full), resolution=RES)
    data.setflags(write=False)
    return data, real, group, want


def _sized_table(real, group, n, rng, near=False):
    """n entries: the first min(n, len(real)) real labels (grouped) plus
    filler keys absent from the volume with non-zero values."""
    used = real[:n]
    keys = list(used)
    vals = [group[r] if group[r] in used else r for r in used]
    nfill = n - len(used)
    if nfill:
        taken = set(real) | {0}
        if near:
            cand = [r + dlt for r in real for dlt in (1, -1)]
        else:
            cand = rng.integers(1, 1 << 40, size=nfill + nfill // 8 + 64)
            cand = np.unique(cand)
            cand = rng.permutation(cand).tolist()
        fill = []
        for k in cand:
            if k not in taken:
                taken.add(k)
                fill.append(int(k))
            if len(fill) == nfill:
                break
        assert len(fill) == nfill
        keys += fill
        vals += [k ^ 0x5A5A for k in fill]
    order = rng.permutation(len(keys))
    return _lm(np.asarray(keys, dtype=np.uint64)[order],
               np.asarray(vals, dtype=np.uint64)[order], 'zero')


def _table_sizes():
    from igneous_amd import engine
    sizes = [1, 63, 64, 65, 2048, 200_000]
    lds = getattr(engine, "LABEL_MAP_LDS_MAX", None)
    if lds is not None:
        sizes += [lds - 1, lds, lds + 1]
    return sorted(set(sizes))


@pytest.mark.parametrize("n", _table_sizes())
def test_table_sizes(eng, vor48, n):
    import oracle
    data, real, group, want_full = vor48
    rng = np.random.default_rng(n)
    lm = _sized_table(real, group, n, rng)
    assert len(lm[0]) == n
    if n >= len(real):
        want = want_full
    else:
        want = oracle.mesh_chunk(host_map(data, lm), resolution=RES)
    got = eng.mesh_chunk(data, resolution=RES, label_map=lm)
    _assert_meshsets_equal(got, want, f"n={n}")
    assert eng.stats()['ms_labelmap'] > 0


def test_table_with_near_miss_keys(eng, vor48):
    """Filler keys are real_label +- 1: near-misses next to every hit."""
    data, real, group, want_full = vor48
    n = len(real) + 40
    lm = _sized_table(real, group, n, np.random.default_rng(5), near=True)
    assert len(lm[0]) == n
    got = eng.mesh_chunk(data, resolution=RES, label_map=lm)
    _assert_meshsets_equal(got, want_full, "near-miss")
    # the same keys under 'keep' with erase-only values for the fillers:
    # nothing real is touched except through its own entry
    keys, vals, _ = lm
    isreal = np.isin(keys, np.asarray(real, dtype=np.uint64))
    vals = np.where(isreal, vals, 0).astype(np.uint64)
    got = eng.mesh_chunk(data, resolution=RES, label_map=(keys, vals, 'keep'))
    _assert_meshsets_equal(got, want_full, "near-miss keep")


# ---------------------------------------------------------------------------
# dust -> map order

def test_dust_runs_before_remap(eng):
    import oracle
    from igneous_amd import remap as R
    data = np.zeros((20, 20, 20), dtype=np.uint32, order="F")
    data[2:4, 2:4, 2:4] = 1        # 8 voxels
    data[4:6, 2:4, 2:4] = 2        # 8 voxels, face-adjacent to 1
    data[8:14, 8:14, 8:14] = 3     # 216 voxels
    thr = 12
    table = {1: 9, 2: 9, 3: 3}

    def dust(vol):
        ids, counts = np.unique(vol, return_counts=True)
        small = [int(i) for i, ct in zip(ids, counts) if ct < thr and i != 0]
        return R.mask(vol.copy(), small)

    lm = R.fold_label_ops(table, None, [], data.dtype)
    dust_then_remap = host_map(dust(data), lm)
    remap_then_dust = dust(host_map(data, lm))
    assert set(np.unique(dust_then_remap).tolist()) == {0, 3}
    # the opposite order would have kept the merged label (16 >= 12)
    assert set(np.unique(remap_then_dust).tolist()) == {0, 3, 9}

    got = eng.mesh_chunk(data, resolution=RES, dust_threshold=thr,
                         label_map=lm)
    _assert_meshsets_equal(
        got, oracle.mesh_chunk(dust_then_remap, resolution=RES), "dust->map")
    assert sorted(got) == [3]


# ---------------------------------------------------------------------------
# errors are return codes, never faults

def test_bad_maps_are_errors_and_engine_survives(eng):
    import oracle
    data, (a, b, c, *_rest) = _noise_volume((21, 19, 17), np.uint32, 9)
    want = oracle.mesh_chunk(data, resolution=RES)

    def still_fine(what):
        _assert_meshsets_equal(
            eng.mesh_chunk(data, resolution=RES), want, f"after {what}")

    with pytest.raises(RuntimeError, match="duplicate key"):
        eng.mesh_chunk(data, resolution=RES,
                       label_map=_lm([a, b, a], [1, 2, 3], 'zero'))
    still_fine("duplicate keys")

    with pytest.raises(RuntimeError, match="key 0"):
        eng.mesh_chunk(data, resolution=RES,
                       label_map=_lm([a, 0], [1, 2], 'keep'))
    still_fine("zero key")

    with pytest.raises(RuntimeError, match="does not fit MG_U32"):
        eng.mesh_chunk(data, resolution=RES,
                       label_map=_lm([a], [1 << 32], 'zero'))
    still_fine("u32 overflow")

    with pytest.raises(ValueError, match="skip_h2d"):
        eng.mesh_chunk(data, resolution=RES, skip_h2d=True,
                       label_map=_lm([a], [b], 'zero'))
    still_fine("skip_h2d")

    with pytest.raises(ValueError, match="miss policy"):
        eng.mesh_chunk(data, resolution=RES,
                       label_map=_lm([a], [b], 'drop'))
    still_fine("bad miss policy")


# ---------------------------------------------------------------------------
# end to end through MeshTask

def test_meshtask_end_to_end_matches_host_path(eng, tmp_path, oracle_mesher):
    from igneous_amd import MeshTask, PrecomputedVolume
    from igneous_amd.storage import CloudFiles
    from igneous_amd.synth import voronoi_labels
    from igneous_amd.tasks import mesh as mesh_mod

    data = voronoi_labels((64, 64, 64), 12, 31, dtype=np.uint32, cache=False)
    ids, counts = np.unique(data[data != 0], return_counts=True)
    by_size = [int(i) for i in ids[np.argsort(counts, kind="stable")]]
    assert len(by_size) >= 8
    s = by_size
    thr = int(sorted(counts)[1])           # only the smallest label is dust
    assert sorted(counts)[0] < thr
    remap_table = {s[0]: s[0], s[1]: 100, s[2]: 100, s[3]: 200, s[4]: 300,
                   s[5]: s[5], s[6]: s[6]}     # s[7:] absent: erased
    opts = dict(remap_table=remap_table,
                object_ids=[s[0], 100, 200, 300, s[5]],   # drops s[6]
                exclude_object_ids=[300],
                dust_threshold=thr)

    layers = {}
    for which in ("host", "device"):
        path = f"file://{tmp_path}/{which}"
        PrecomputedVolume.from_numpy(
            data, path, resolution=(16, 16, 40), chunk_size=(64, 64, 64),
            mesh_dir="mesh")
        layers[which] = path

    def run(path):
        MeshTask(shape=(64, 64, 64), offset=(0, 0, 0), layer_path=path,
                 mip=0, simplification_factor=0, spatial_index=True,
                 **opts).execute()

    run(layers["host"])                    # oracle mesher, host numpy path
    mesh_mod.set_mesher(None)              # the product engine
    run(layers["device"])
    assert eng.stats()['ms_labelmap'] > 0

    host, dev = CloudFiles(layers["host"]), CloudFiles(layers["device"])
    names = list(host.list("mesh/"))
    assert names == list(dev.list("mesh/"))
    frags = [n for n in names if ":0:" in n]
    assert sorted(int(n.split("/")[1].split(":")[0]) for n in frags) == \
        sorted([100, 200, s[5]])
    for n in names:
        assert host.get(n) == dev.get(n), n
