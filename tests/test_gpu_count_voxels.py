"""mg_count_voxels (the GPU part runs under pytest -m gpu): every distinct
value of a volume with its voxel count, exactly np.unique(...,
return_counts=True), on the shapes at which the run-counting pass can go
wrong — a single voxel, less than one 64-voxel step, x not a multiple of 64
with runs crossing row ends, one run across every span, no run longer than
one voxel, labels that need 64 bits — and on more labels than the context's
first label table holds, so the grow-and-retry loop runs."""
import ctypes
import functools

import numpy as np
import pytest

DTYPES = [np.uint64, np.uint32]
_ids = lambda d: np.dtype(d).name  # noqa: E731
TOP = (1 << 64) - 1


def _voronoi(dtype):
    from igneous_amd.synth import voronoi_labels
    return voronoi_labels((64, 64, 64), 500, 17, dtype=dtype, cache=False)


def _distinct(shape, dtype, first=1):
    n = int(np.prod(shape))
    return np.asfortranarray(
        np.arange(first, first + n, dtype=dtype).reshape(shape, order="F"))


def _rows(dtype):
    """65 x 3 x 2: runs that cross the row ends, and a row of zeros."""
    v = np.zeros((65, 3, 2), dtype=dtype, order="F")
    v[:, 0, 0] = 5
    v[:10, 1, 0] = 5          # the run goes on into the next row
    v[10:, 1, 0] = 6
    v[:, 2, 0] = 6            # ... and so does this one
    v[3:64, 0, 1] = 9
    v[64, 2, 1] = 9
    return v


def _wide(dtype):
    """u64: labels at and above 2^32 and 2^64 - 1; u32: the top of u32."""
    hi = [1 << 32, (1 << 32) + 1, 1 << 63, TOP] if dtype == np.uint64 \
        else [1 << 31, (1 << 32) - 1, 7, 8]
    v = np.zeros((70, 5, 3), dtype=dtype, order="F")
    v[:, 0, :] = hi[0]
    v[1::2, 1, :] = hi[1]
    v[:, 2, 0] = hi[2]
    v[5:, 3:, 1:] = hi[3]
    return v


CASES = {
    "1x1x1": lambda d: np.full((1, 1, 1), 3, dtype=d, order="F"),
    "1x1x1_zero": lambda d: np.zeros((1, 1, 1), dtype=d, order="F"),
    "63x1x1": lambda d: np.asfortranarray(
        (np.arange(63) // 5).astype(d).reshape(63, 1, 1)),
    "65x3x2_rows": _rows,
    "voronoi64": _voronoi,
    "all_zero": lambda d: np.zeros((40, 9, 7), dtype=d, order="F"),
    # 150 x 100 x 70 = 1 050 000 voxels: every wave walks more than one step
    "uniform": lambda d: np.full((150, 100, 70), 12345, dtype=d, order="F"),
    "wide_labels": _wide,
    "every_voxel_distinct": lambda d: _distinct((33, 17, 9), d),
}


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    vol = CASES[name](dtype)
    assert vol.flags.f_contiguous and vol.dtype == dtype
    u, c = np.unique(vol, return_counts=True)
    return vol, u.astype(np.uint64), c.astype(np.uint64)


def test_inputs_are_not_trivial():
    for dtype in DTYPES:
        _, u, c = _case("65x3x2_rows", dtype)
        assert u.tolist() == [0, 5, 6, 9] and c.tolist() == [133, 75, 120, 62]
        _, u, c = _case("voronoi64", dtype)
        assert 400 < len(u) <= 501 and u[0] == 0
        _, u, c = _case("every_voxel_distinct", dtype)
        assert len(u) == 33 * 17 * 9 and c.max() == 1 and u[0] == 1
        _, u, c = _case("uniform", dtype)
        assert u.tolist() == [12345] and c.tolist() == [1_050_000]
        _, u, _ = _case("all_zero", dtype)
        assert u.tolist() == [0]
    assert _case("wide_labels", np.uint64)[1].tolist()[-2:] == [1 << 63, TOP]


@pytest.fixture(scope="module")
def eng():
    from igneous_amd.engine import Engine
    e = Engine(0)  # private: no other test's call has run on this ctx
    yield e
    e.lib.mg_destroy(e.ctx)
    e.ctx = None


def _fresh(fn):
    from igneous_amd.engine import Engine
    e = Engine(0)
    try:
        return fn(e)
    finally:
        e.lib.mg_destroy(e.ctx)
        e.ctx = None


def _assert_counts(got, u, c, what=""):
    values, counts = got
    assert values.dtype == np.uint64 and counts.dtype == np.uint64, what
    assert values.shape == u.shape and np.array_equal(values, u), what
    assert np.array_equal(counts, c), what


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", list(CASES))
def test_count_voxels_equals_numpy_unique(eng, name, dtype):
    vol, u, c = _case(name, dtype)
    _assert_counts(eng.count_voxels(vol), u, c, name)


@pytest.mark.gpu
def test_more_labels_than_the_first_table_holds():
    """128 x 128 x 65 distinct labels = 1 064 960 > the 2^20 slots a fresh
    context starts with: the pass overflows, grows the table and runs
    again."""
    vol = _distinct((128, 128, 65), np.uint64, first=(1 << 33))
    assert vol.size > (1 << 20)

    def run(e):
        got = e.count_voxels(vol)
        return got, e.stats()
    (values, counts), st = _fresh(run)
    assert values.shape == (vol.size,)
    assert np.array_equal(values, vol.reshape(-1, order="F"))
    assert np.array_equal(counts, np.ones(vol.size, dtype=np.uint64))
    assert st["n_labels"] == vol.size


@pytest.mark.gpu
def test_two_calls_agree_and_a_small_call_follows_a_large_one(eng):
    big, u, c = _case("voronoi64", np.uint64)
    first = eng.count_voxels(big)
    second = eng.count_voxels(big)
    _assert_counts(first, u, c)
    assert np.array_equal(first[0], second[0])
    assert np.array_equal(first[1], second[1])
    small, su, sc = _case("65x3x2_rows", np.uint64)
    _assert_counts(eng.count_voxels(small), su, sc, "small after large")
    # ... and in the other dtype, through the same buffers
    small32, su, sc = _case("63x1x1", np.uint32)
    _assert_counts(eng.count_voxels(small32), su, sc, "u32 after u64")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_first_and_only_call_of_a_context(dtype):
    vol, u, c = _case("65x3x2_rows", dtype)
    _assert_counts(_fresh(lambda e: e.count_voxels(vol)), u, c)


@pytest.mark.gpu
def test_module_level_counter_is_advertised():
    from igneous_amd import engine
    assert engine.mesh_chunk.count_voxels is engine.count_voxels
    vol, u, c = _case("wide_labels", np.uint64)
    _assert_counts(engine.count_voxels(vol), u, c)


MS_FIELDS = ["ms_h2d", "ms_count", "ms_scan", "ms_emit", "ms_partition",
             "ms_weld", "ms_simplify", "ms_d2h", "ms_total", "ms_labelmap",
             "ms_fill", "ms_encode"]


@pytest.mark.gpu
def test_stats_fields(eng):
    vol, u, _ = _case("voronoi64", np.uint64)
    # a meshing call first: every stage field then holds another call's time
    assert len(eng.mesh_chunk(vol)) == len(u) - 1
    assert eng.stats()["ms_weld"] > 0
    eng.count_voxels(vol)
    st = eng.stats()
    print(st)
    assert st["bytes_read_algorithmic"] == vol.size * 8
    assert st["n_labels"] == len(u) - 1           # non-zero labels
    assert st["total_tris"] == 0 and st["total_verts"] == 0
    assert st["ms_count"] > 0 and st["ms_h2d"] > 0
    assert st["ms_total"] >= st["ms_count"] + st["ms_h2d"] - 1e-3
    for name in MS_FIELDS:
        if name not in ("ms_h2d", "ms_count", "ms_total"):
            assert st[name] == 0.0, name
    # the volume is resident: skip_h2d counts it again without the upload
    again = eng.count_voxels(vol, skip_h2d=True)
    _assert_counts(again, *_case("voronoi64", np.uint64)[1:])


# ---------------------------------------------------------------------------
# raw ABI: rejected calls

def _raw(eng, vol, *, ctx=True, labels=True, dims=None, dtype=None, out=True):
    from igneous_amd import engine as E
    dest = ctypes.POINTER(E._MgLabelCounts)()
    rc = eng.lib.mg_count_voxels(
        eng.ctx if ctx else None,
        vol.ctypes.data_as(ctypes.c_void_p) if labels else None,
        *(dims or vol.shape), E._mg_dtype(vol) if dtype is None else dtype,
        0, ctypes.byref(dest) if out else None)
    return rc, dest


REJECTED = [
    ("null ctx", dict(ctx=False), 1),
    ("null labels", dict(labels=False), 1),
    ("null out", dict(out=False), 1),
    ("sx = 0", dict(dims=(0, 3, 2)), 2),
    ("sy = 2048", dict(dims=(65, 2048, 2)), 2),
    ("bad dtype", dict(dtype=5), 3),
    ("null labels, bad dims", dict(labels=False, dims=(0, 3, 2)), 1),
    ("bad dims, bad dtype", dict(dims=(0, 3, 2), dtype=5), 2),
]


@pytest.mark.gpu
def test_rejected_calls_leave_the_context_usable(eng):
    vol, u, c = _case("65x3x2_rows", np.uint64)
    for what, kw, code in REJECTED:
        rc, dest = _raw(eng, vol, **kw)
        err = eng.lib.mg_last_error(eng.ctx if kw.get("ctx", True) else None)
        print(f"{what}: rc={rc} {err!r}")
        assert rc == code, what
        assert err, what
        assert not dest, what
    rc, dest = _raw(eng, vol)
    assert rc == 0
    try:
        n = int(dest.contents.n)
        assert n == len(u)
        assert np.ctypeslib.as_array(dest.contents.labels,
                                     shape=(n,)).tolist() == u.tolist()
        assert np.ctypeslib.as_array(dest.contents.counts,
                                     shape=(n,)).tolist() == c.tolist()
    finally:
        eng.lib.mg_label_counts_free(dest)
    assert not eng.lib.mg_last_error(eng.ctx)
