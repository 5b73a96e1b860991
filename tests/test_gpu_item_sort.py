"""GPU tests (pytest -m gpu) of the per-item stream between emit and weld:
k_emit writes one record per (cell, label) pair, the partition sorts those
items and scans their triangle counts, and k_weld_first expands each item
into its 1..5 triangles, 256 triangles per block. Shapes are the smallest
at which that can go wrong — triangle totals on either side of the weld's
block size, items of every size straddling a block boundary, labels of a
single item, rows of several segments — all BIT-EXACT against the CPU
oracle, each once through the sorted records and once through the sort's
permutation (MG_SORT_RECS=0)."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (16.0, 16.0, 40.0)
WELD_BLOCK = 256  # triangles per k_weld_first block


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


def _ntris(meshes: dict) -> int:
    return sum(f.shape[0] for _, f in meshes.values())


# --- inputs ---------------------------------------------------------------

def _rod(x0, length):
    """One-voxel-thick rod of one label along the x edge of a zero volume
    one cell thick in y and z: every cell the rod passes has two corners of
    it (2 triangles), a free end has one (1 triangle). Flush with x = 0 the
    rod has one free end and 2 * length - 1 triangles, inset by one voxel
    it has two and 2 * length."""
    data = np.zeros((x0 + length + 1, 2, 2), dtype=np.uint64, order="F")
    data[x0:x0 + length, 0, 0] = 5
    return data


# (x0, length) -> T = 255, 256, 257, 511, 512, 513
RODS = [(0, 128), (1, 128), (0, 129), (0, 256), (1, 256), (0, 257)]


def _rod2(length, corner):
    """Dense rod of labels 1 and 2 filling the one-cell-thick cross-section,
    capped by zeros: every cell holds two items of 1-4 triangles. All
    lengths are prefixes of one seeded volume, so T grows by a few
    triangles per cell; it is always even, and a single voxel in the far
    corner of the volume adds the one triangle that makes it odd."""
    rng = np.random.default_rng(4243)
    full = rng.integers(1, 3, size=(160, 2, 2)).astype(np.uint64)
    data = np.zeros((length + 3, 2, 2), dtype=np.uint64, order="F")
    data[:length] = full[:length]
    if corner:
        data[length + 2, 1, 1] = 2
    return data


# (length, corner) -> T = 255, 256, 257, 512, 513, 767
RODS2 = [(40, 1), (41, 0), (41, 1), (81, 0), (81, 1), (118, 1)]


def _dense(shape, seed, dtype=np.uint64, nlabels=3):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(
        rng.integers(0, nlabels + 1, size=shape).astype(dtype))


def _single_items_and_one_large(dtype=np.uint64):
    """Isolated single voxels of distinct labels, every other voxel of a
    block that starts in the volume's corner: a voxel inside the volume is
    in 8 cells (8 items of one triangle), one on a face, an edge or the
    corner of the volume in 4, 2 or exactly 1. Next to them one large
    label."""
    data = np.zeros((24, 12, 10), dtype=dtype, order="F")
    lab = 100
    for z in range(0, 9, 2):
        for y in range(0, 11, 2):
            for x in range(0, 11, 2):
                data[x, y, z] = lab
                lab += 1
    data[13:23, 1:11, 1:9] = 7
    return data


def _box(dtype=np.uint64):
    data = np.zeros((24, 24, 24), dtype=dtype, order="F")
    data[2:22, 2:22, 2:22] = 7
    return data


def _single_voxel():
    data = np.zeros((3, 3, 3), dtype=np.uint64, order="F")
    data[1, 1, 1] = 5
    return data


CASES = {
    "dense20x19x18u32": lambda: _dense((20, 19, 18), 101, np.uint32),
    "dense20x19x18u64": lambda: _dense((20, 19, 18), 101, np.uint64),
    "singles+large": _single_items_and_one_large,
    "one_label": _box,
    "uniform": lambda: np.full((6, 5, 4), 9, dtype=np.uint64, order="F"),
    "zeros": lambda: np.zeros((6, 5, 4), dtype=np.uint64, order="F"),
    "single_voxel": _single_voxel,
    "segs70x3x3": lambda: _dense((70, 3, 3), 37 + 70),
    "segs130x4x3": lambda: _dense((130, 4, 3), 37 + 130),
}
for _x0, _len in RODS:
    CASES[f"rod{_x0}+{_len}"] = (lambda a=_x0, b=_len: _rod(a, b))
for _len, _corner in RODS2:
    CASES[f"rod2x{_len}+{_corner}"] = (lambda a=_len, b=_corner: _rod2(a, b))

_DATA = {}
_ORACLE = {}


def _data(name):
    if name not in _DATA:
        d = CASES[name]()
        d.setflags(write=False)
        _DATA[name] = d
    return _DATA[name]


def _want(name, **kw):
    """Oracle result, computed once per case and shared read-only."""
    import oracle
    key = (name, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        _ORACLE[key] = oracle.mesh_chunk(_data(name), resolution=RES, **kw)
    return _ORACLE[key]


def _check(eng, name, **kw):
    _assert_meshsets_equal(eng.mesh_chunk(_data(name), resolution=RES, **kw),
                           _want(name, **kw), name)


@pytest.fixture(params=["sorted_records", "permutation"])
def sort_path(request, monkeypatch):
    if request.param == "permutation":
        monkeypatch.setenv("MG_SORT_RECS", "0")
    else:
        monkeypatch.delenv("MG_SORT_RECS", raising=False)
    return request.param


# --- numpy classification of the cells into items -------------------------

def _tri_count_table():
    with open(os.path.join(REPO, "igneous_amd", "csrc", "mc_table.h")) as f:
        m = re.search(r"MC_TRI_COUNT\[256\] = \{(.*?)\};", f.read(), re.S)
    t = np.array([int(x) for x in re.findall(r"\d+", m.group(1))])
    assert t.shape == (256,)
    return t


def _item_sizes(data):
    """Triangles of every item of the volume: per cell, one item per
    distinct non-zero label, of MC_TRI_COUNT[mask of corners equal to it]
    triangles (corner i = dx + 2 dy + 4 dz)."""
    tc = _tri_count_table()
    sx, sy, sz = data.shape
    c = [data[dx:sx - 1 + dx, dy:sy - 1 + dy, dz:sz - 1 + dz]
         for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    sizes = []
    for j in range(8):
        mask = np.zeros(c[0].shape, dtype=np.int64)
        for i in range(8):
            mask |= (c[i] == c[j]).astype(np.int64) << i
        first = (c[j] != 0) & (mask != 255)  # a uniform cell has no item
        for i in range(j):
            first &= c[i] != c[j]
        sizes.append(tc[mask[first]])
    return np.concatenate(sizes)


# --- block and wave boundaries of the expansion ---------------------------

def test_rod_totals_hit_block_boundaries():
    """The sweep's triangle totals, from the oracle: one below, at and one
    above one and two weld blocks."""
    totals = [_ntris(_want(f"rod{x0}+{n}")) for x0, n in RODS]
    assert {t % WELD_BLOCK for t in totals} >= {0, 1, WELD_BLOCK - 1}
    assert min(totals) < WELD_BLOCK < 2 * WELD_BLOCK < max(totals)
    assert any(WELD_BLOCK < t < 2 * WELD_BLOCK for t in totals)
    for x0, n in RODS:  # every item of a rod has 1 or 2 triangles
        assert set(_item_sizes(_data(f"rod{x0}+{n}")).tolist()) <= {1, 2}


@pytest.mark.parametrize("rod", RODS, ids=lambda r: f"{r[0]}+{r[1]}")
def test_rod(eng, rod, sort_path):
    _check(eng, f"rod{rod[0]}+{rod[1]}")


def test_rod2_totals_hit_block_boundaries():
    totals = [_ntris(_want(f"rod2x{n}+{c}")) for n, c in RODS2]
    assert {t % WELD_BLOCK for t in totals} >= {0, 1, WELD_BLOCK - 1}
    assert min(totals) < WELD_BLOCK < 2 * WELD_BLOCK < max(totals)
    assert any(WELD_BLOCK < t < 2 * WELD_BLOCK for t in totals)
    # items of 1-4 triangles, so that across the sweep a block boundary
    # falls inside items of different sizes
    for n, c in RODS2:
        assert set(_item_sizes(_data(f"rod2x{n}+{c}")).tolist()) >= \
            {1, 2, 3, 4}


@pytest.mark.parametrize("rod", RODS2, ids=lambda r: f"{r[0]}+{r[1]}")
def test_rod2(eng, rod, sort_path):
    _check(eng, f"rod2x{rod[0]}+{rod[1]}")


# --- every item size -------------------------------------------------------

@pytest.mark.parametrize("dtype", ["u32", "u64"])
def test_dense_every_item_size(eng, dtype, sort_path):
    name = f"dense20x19x18{dtype}"
    sizes = _item_sizes(_data(name))
    assert set(sizes.tolist()) == {1, 2, 3, 4, 5}
    assert int(sizes.sum()) == _ntris(_want(name))
    _check(eng, name)


# --- label ranges over items ----------------------------------------------

def test_singles_have_one_item_labels():
    """The case holds labels of exactly one item (the volume's corner
    voxel), of 2, 4 and 8 one-triangle items, and one large label."""
    want = _want("singles+large")
    per_label = sorted(f.shape[0] for _, f in want.values())
    assert per_label[0] == 1 and {2, 4, 8} <= set(per_label)
    assert per_label[-1] > 100 and len(per_label) > 100
    sizes = _item_sizes(_data("singles+large"))
    assert (sizes == 1).sum() >= sum(p for p in per_label[:-1])


@pytest.mark.parametrize("name", ["singles+large", "one_label", "uniform",
                                  "zeros", "single_voxel"])
def test_label_ranges(eng, name, sort_path):
    if name in ("uniform", "zeros"):
        assert _ntris(_want(name)) == 0
    if name == "one_label":
        assert len(_want(name)) == 1
    _check(eng, name)


def test_singles_u32(eng):
    import oracle
    data = _single_items_and_one_large(np.uint32)
    _assert_meshsets_equal(eng.mesh_chunk(data, resolution=RES),
                           oracle.mesh_chunk(data, resolution=RES), "u32")


# --- rows of 2 and 3 segments: item offsets across segment boundaries -----

@pytest.mark.parametrize("name", ["segs70x3x3", "segs130x4x3"])
def test_several_segments_per_row(eng, name, sort_path):
    _check(eng, name)


# --- determinism ------------------------------------------------------------

def test_deterministic(eng, sort_path):
    data = _data("dense20x19x18u64")
    a = eng.mesh_chunk(data, resolution=RES)
    b = eng.mesh_chunk(data, resolution=RES)
    assert sorted(a) == sorted(b)
    for label in a:
        for x, y in zip(a[label], b[label]):
            assert x.dtype == y.dtype and x.shape == y.shape
            assert x.tobytes() == y.tobytes()


# --- consumers of the per-triangle label array ----------------------------

def test_downstream_simplify(eng, sort_path):
    _check(eng, "one_label", reduction_factor=4, max_error=1e9)
    assert _ntris(_want("one_label", reduction_factor=4, max_error=1e9)) > 0


def test_downstream_simplify_many_labels(eng):
    _check(eng, "dense20x19x18u64", reduction_factor=4, max_error=1e9)


def test_downstream_fill_holes(eng, sort_path):
    import oracle
    import fill_holes_ref as R
    data = np.full((14, 13, 12), 3, dtype=np.uint64, order="F")
    data[4:9, 4:9, 4:8] = 9       # enclosed: becomes a hole of label 3
    data[5:7, 5:7, 5:7] = 0
    data[11:] = 0                 # open side, so the filled volume has a surface
    want_f, want_h, _ = R.fill_holes_ref(data, 1)
    got_f, got_h = eng.mesh_chunk(data, resolution=RES, fill_holes=1)
    _assert_meshsets_equal(got_f, oracle.mesh_chunk(want_f, resolution=RES),
                           "filled")
    _assert_meshsets_equal(got_h, oracle.mesh_chunk(want_h, resolution=RES),
                           "holes")
