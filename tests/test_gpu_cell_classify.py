"""GPU tests (pytest -m gpu) of the count/emit cell classification: each
cell's 28 corner compares are done once, giving the case mask of every
corner's label and the set of first corners, and both kernels walk that
set. Shapes are the smallest at which this can go wrong — every case
mask, 64-bit labels that differ in one half only, cells with eight labels
and zeros, rows of one and two cells, labels that run along x across
segment boundaries — all BIT-EXACT against the CPU oracle."""
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


def _check(eng, data, what):
    import oracle
    _assert_meshsets_equal(eng.mesh_chunk(data, resolution=RES),
                           oracle.mesh_chunk(data, resolution=RES), what)


def _all_masks(a, b, dtype):
    """All 256 two-value case masks as 2x2x2 blocks, tiled 16 x 16 with no
    padding: block (bx, by) holds mask by*16+bx, corner bit dx + 2*dy +
    4*dz (the kernels' corner order) -> a, else b."""
    data = np.empty((32, 32, 2), dtype=dtype, order="F")
    for m in range(256):
        bx, by = m % 16, m // 16
        for bit in range(8):
            dx, dy, dz = bit & 1, (bit >> 1) & 1, bit >> 2
            data[2 * bx + dx, 2 * by + dy, dz] = a if (m >> bit) & 1 else b
    return data


# value pairs: both non-zero, then one of them 0. The u64 pairs differ in
# one 32-bit half only, and one non-zero value has an all-zero low half: a
# compare or a zero test that drops a half fails here.
MASK_PAIRS = {
    np.uint32: [(7, 9), (7, 0)],
    np.uint64: [((1 << 32) | 5, 5), ((1 << 40) + 1, (1 << 40) + 2),
                ((1 << 32) | 5, 0), (1 << 32, 0), (5, 0)],
}


@pytest.mark.parametrize(
    "dtype,pair",
    [(d, p) for d in DTYPES for p in MASK_PAIRS[d]],
    ids=lambda v: np.dtype(v).name if isinstance(v, type) else
    "-".join(hex(x) for x in v))
def test_every_case_mask(eng, dtype, pair):
    data = _all_masks(pair[0], pair[1], dtype)
    got = eng.mesh_chunk(data, resolution=RES)
    assert sorted(got.keys()) == sorted(v for v in pair if v != 0)
    _check(eng, data, f"masks{pair}")


def _many_labels(shape, seed, dtype):
    """Dense draw from 1000 values incl. 0, an eighth of the voxels zeroed
    on top: nearly every cell holds eight distinct corner values, some of
    them 0. u64 values also differ above bit 32."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1000, size=shape).astype(np.uint64)
    v[rng.random(shape) < 0.125] = 0
    if dtype == np.uint64:
        v = np.where(v != 0, v + ((v % 5) << np.uint64(33)), v)
    data = np.asfortranarray(v.astype(dtype))
    assert (data == 0).any() and len(np.unique(data)) > 8
    return data


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", [(5, 4, 3), (66, 3, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_eight_labels_per_cell(eng, shape, dtype):
    """(66, 3, 3): a 65-cell row, so a second segment with one live lane,
    and segment triangle totals far above the workload's average."""
    data = _many_labels(shape, 5 + shape[0], dtype)
    c = [data[dx:shape[0] - 1 + dx, dy:shape[1] - 1 + dy,
              dz:shape[2] - 1 + dz]
         for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    distinct = np.sort(np.stack(c), axis=0)
    assert ((np.diff(distinct, axis=0) != 0).sum(axis=0) == 7).any(), \
        "no cell with eight distinct corner values"
    _check(eng, data, f"many{shape}{np.dtype(dtype).name}")


def test_labels_across_segments(eng):
    """Three segments per row (129 cells). A fills y < 2 over all x: each
    of its boundary cells has it on the low-x face, through all three
    segments. B is only in the last voxel column: no low-x face holds it.
    C is one voxel at x = 64: on the low-x face of lane 0 of the second
    segment and only on the high-x corners of lane 63 of the first. Every
    label must reach the label hash exactly once: none missing, none
    added."""
    A, B, C = (1 << 35) | 3, 3, (1 << 35) | 4
    data = np.zeros((130, 4, 4), dtype=np.uint64, order="F")
    data[:, :2, :] = A
    data[129, 2:, :] = B
    data[64, 3, 2] = C
    got = eng.mesh_chunk(data, resolution=RES)
    assert sorted(got.keys()) == sorted([A, B, C])
    _check(eng, data, "chains")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("sx", [2, 3])
def test_short_rows(eng, sx, dtype):
    """One and two cells per row: lanes 1.. / 2.. of every wave are idle."""
    rng = np.random.default_rng(40 + sx)
    data = np.asfortranarray(
        rng.integers(0, 4, size=(sx, 5, 4)).astype(dtype))
    _check(eng, data, f"short{sx}{np.dtype(dtype).name}")
