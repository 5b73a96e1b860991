"""GPU tests (pytest -m gpu) of the weld's table-driven first-occurrence
test: k_weld_first decides from the 8-byte record alone (mask, t, and
which of cx/cy/cz are 0) whether a corner is the first of its slot,
stores first positions with plain stores into a table that is never
cleared, and ballots the flags into three words per wave. Shapes are the
smallest at which that can go wrong — labels on every volume border,
axes one cell thick, rows of several 64-cell segments, a table full of
another call's positions — all BIT-EXACT against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES = (16.0, 16.0, 40.0)
DTYPES = [np.uint32, np.uint64]
_ids = lambda d: np.dtype(d).name  # noqa: E731


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


def _dense(shape, seed, dtype=np.uint64, nlabels=3):
    """Random labels 0..nlabels filling the volume to its border."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(
        rng.integers(0, nlabels + 1, size=shape).astype(dtype))


def _box(dtype=np.uint64):
    data = np.zeros((24, 24, 24), dtype=dtype, order="F")
    data[2:22, 2:22, 2:22] = 7
    return data


def _single_voxel():
    data = np.zeros((3, 3, 3), dtype=np.uint64, order="F")
    data[1, 1, 1] = 5
    return data


_ORACLE = {}


def _want(key, data, **kw):
    """Oracle result, computed once per key and shared read-only."""
    import oracle
    if key not in _ORACLE:
        _ORACLE[key] = oracle.mesh_chunk(data, resolution=RES, **kw)
    return _ORACLE[key]


def _check(eng, key, data, **kw):
    _assert_meshsets_equal(eng.mesh_chunk(data, resolution=RES, **kw),
                           _want(key, data, **kw), key)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", [(4, 4, 4), (9, 7, 6)],
                         ids=lambda s: "x".join(map(str, s)))
def test_unpadded_dense(eng, shape, dtype):
    """Every c_b == 0 combination incl. the volume's corner cell; with 4
    values over 8 corners most cells hold 3+ labels."""
    data = _dense(shape, 11 + sum(shape), dtype)
    assert (data[0] != 0).any() and (data[:, 0] != 0).any() \
        and (data[:, :, 0] != 0).any()
    _check(eng, f"dense{shape}{np.dtype(dtype).name}", data)


@pytest.mark.parametrize("shape", [(2, 5, 6), (5, 2, 6), (5, 6, 2), (2, 2, 2)],
                         ids=lambda s: "x".join(map(str, s)))
def test_single_cell_thick_axes(eng, shape):
    """One cell along an axis: its boundary bit is set in every record."""
    for dtype in DTYPES:
        data = _dense(shape, 23 + shape[0] + 3 * shape[1], dtype)
        _check(eng, f"thin{shape}{np.dtype(dtype).name}", data)


@pytest.mark.parametrize("shape", [(70, 3, 3), (130, 4, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_several_segments_per_row(eng, shape):
    """Rows of 2 and 3 segments: cx == 0 holds only in the first, and the
    cells at lanes 63/0 share edges across a segment boundary."""
    data = _dense(shape, 37 + shape[0])
    _check(eng, f"segs{shape}", data)


def test_stale_table(eng):
    """The first-position table is not cleared between calls: a corner
    wrongly taken for a later occurrence would read a position left by an
    earlier call. Two different volumes of one shape back to back, then a
    box, a single voxel, and the first volume again."""
    a = _dense((20, 19, 18), 101)
    b = _dense((20, 19, 18), 202)
    assert not np.array_equal(a, b)
    for key, data in (("stale_a", a), ("stale_b", b), ("box", _box()),
                      ("single", _single_voxel()), ("stale_a", a)):
        _check(eng, key, data)


def test_permutation_sort_path(eng, monkeypatch):
    """MG_SORT_RECS=0: records are read through the sort's permutation."""
    monkeypatch.setenv("MG_SORT_RECS", "0")
    _check(eng, "stale_a", _dense((20, 19, 18), 101))
    _check(eng, "segs(70, 3, 3)", _dense((70, 3, 3), 37 + 70))


def test_downstream_simplify(eng):
    _check(eng, "box_simplified", _box(), reduction_factor=4, max_error=1e9)
    assert sum(f.shape[0] for _, f in _ORACLE["box_simplified"].values()) > 0


def test_downstream_fill_holes(eng):
    """fill_holes=1 meshes the filled and the hole volume through the same
    weld; the dense shell reaches the volume border."""
    import oracle
    import fill_holes_ref as R
    data = np.full((14, 13, 12), 3, dtype=np.uint64, order="F")
    data[4:9, 4:9, 4:8] = 9       # enclosed: becomes a hole of label 3
    data[5:7, 5:7, 5:7] = 0
    data[11:] = 0                 # open side, so the filled volume has a surface
    want_f, want_h, _ = R.fill_holes_ref(data, 1)
    assert set(np.unique(want_f).tolist()) == {0, 3}
    assert set(np.unique(want_h).tolist()) == {0, 9}
    got_f, got_h = eng.mesh_chunk(data, resolution=RES, fill_holes=1)
    _assert_meshsets_equal(got_f, oracle.mesh_chunk(want_f, resolution=RES),
                           "filled")
    _assert_meshsets_equal(got_h, oracle.mesh_chunk(want_h, resolution=RES),
                           "holes")
