"""GPU tests of the per-label weld (pytest -m gpu): one workgroup per label
with the (slot -> vertex id) table in LDS, in three vertex-count bands, and
the global direct-addressed table for the labels above the top band's cap.
Everything is BIT-EXACT against the CPU oracle.

Every case asserts which path it takes before the engine runs, from the
oracle's vertex counts and the caps in eng.stats() (weld_lds_cap is the top
band's cap, the bands below end at a half and a quarter of it), and
afterwards from the
path counters, so a case cannot pass by silently taking the other path.

A solid box of side n in background has exactly 6 n^2 vertices and
12 n^2 - 4 triangles, so n = floor(sqrt(cap / 6)) and n + 1 sit on either
side of a band edge.

The engine numbers labels in the order its count pass meets them, which is
not the order of their values, so the order of the labels in the triangle
stream is not the test's to choose. Where a case needs two labels to share
a 256-triangle block of the stream, it asserts a condition under which they
do for every order."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES = (16.0, 16.0, 40.0)
ANISO = (4.0, 16.0, 40.0)
BLK = 256  # triangles per tile of the weld kernels


@pytest.fixture(scope="module")
def eng():
    from igneous_amd.engine import Engine
    return Engine.get(0)


@pytest.fixture(scope="module")
def caps(eng):
    cap = int(eng.stats()["weld_lds_cap"])
    assert cap >= 512 and cap % 4 == 0
    return cap // 4, cap // 2, cap


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


def _nverts(meshes):
    return {k: int(v.shape[0]) for k, (v, _) in meshes.items()}


def _ntris(meshes):
    return {k: int(f.shape[0]) for k, (_, f) in meshes.items()}


def _expect_paths(meshes, cap):
    """(labels on the LDS path, labels on the table path) by the oracle."""
    nv = _nverts(meshes)
    table = sum(1 for n in nv.values() if n > cap)
    return len(nv) - table, table


def _assert_paths(eng, meshes, cap, what):
    st = eng.stats()
    lds, table = _expect_paths(meshes, cap)
    assert (int(st["weld_lds_labels"]), int(st["weld_table_labels"])) == \
        (lds, table), f"{what}: path counters {st}"


def _edge_sides(cap):
    n = math.isqrt(cap // 6)
    assert 6 * n * n <= cap < 6 * (n + 1) * (n + 1)
    return n, n + 1


BASE = 1 << 33  # u64 ids above 2^32


def _band_edges(caps):
    """Boxes of side n and n + 1 for every band edge, stacked along z, and a
    plane of single-voxel labels whose ids interleave with the boxes'."""
    sides = sum((_edge_sides(c) for c in caps), ())
    w = max(sides) + 4
    depth = sum(sides) + len(sides) + 1 + 3
    data = np.zeros((w, w, depth), dtype=np.uint64, order="F")
    z = 1
    for i, n in enumerate(sides):
        data[2:2 + n, 2:2 + n, z:z + n] = BASE + 100 * (i + 1)
        z += n + 1
    k = 0
    for x in range(2, w - 2, 3):
        for y in range(2, w - 2, 3):
            data[x, y, z + 1] = BASE + 100 * (k % 5) + 50 + k // 5
            k += 1
    assert z + 3 == depth
    return data, sides


def _single_voxel():
    data = np.zeros((3, 3, 3), dtype=np.uint32, order="F")
    data[1, 1, 1] = 5
    return data


def _tiny_labels():
    """7x6x5, every interior voxel its own sparse u64 id above 2^32."""
    rng = np.random.default_rng(2718)
    n = 5 * 4 * 3
    ids = np.unique(rng.integers(1 << 32, 1 << 40, size=4 * n,
                                 dtype=np.uint64))
    ids = rng.permutation(ids)[:n]
    data = np.zeros((7, 6, 5), dtype=np.uint64, order="F")
    data[1:-1, 1:-1, 1:-1] = ids.reshape((5, 4, 3))
    return np.asfortranarray(data)


def _near_full():
    """14x13x12 random over 6 ids above 2^32: irregular labels of roughly a
    thousand vertices each, many probe collisions."""
    rng = np.random.default_rng(606)
    ids = np.concatenate(
        [[0], rng.integers(1 << 32, 1 << 40, size=6)]).astype(np.uint64)
    data = np.zeros((14, 13, 12), dtype=np.uint64, order="F")
    data[1:-1, 1:-1, 1:-1] = ids[rng.integers(1, 7, size=(12, 11, 10))]
    return np.asfortranarray(data)


def _dense(shape, nlab, seed):
    """Unpadded: labels touch all six faces."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(
        rng.integers(0, nlab + 1, size=shape).astype(np.uint32))


def _box_ladder():
    """Boxes of side 1..12, one label each."""
    data = np.zeros((16, 16, 92), dtype=np.uint32, order="F")
    z = 1
    for n in range(1, 13):
        data[2:2 + n, 2:2 + n, z:z + n] = 1000 + n
        z += n + 1
    assert z <= 92
    return data


@pytest.fixture(scope="module")
def ref(caps):
    """Inputs and oracle results, computed once and shared read-only."""
    import oracle
    band, sides = _band_edges(caps)
    out = {"sides": sides}
    for key, data in (("band", band), ("single", _single_voxel()),
                      ("tiny", _tiny_labels()), ("full", _near_full()),
                      ("ladder", _box_ladder())):
        out[key] = (data, oracle.mesh_chunk(data, resolution=RES))
    out["band_simplified"] = (band, oracle.mesh_chunk(
        band, resolution=RES, reduction_factor=100, max_error=40.0))
    for key, data in (("dense_small", _dense((12, 11, 10), 4, 11)),
                      ("dense_big", _dense((24, 23, 22), 1, 12))):
        out[key] = (data, oracle.mesh_chunk(data, resolution=ANISO,
                                            voxel_centered=False))
    return out


def _check_band_preconditions(ref, caps):
    cap = caps[-1]
    data, want = ref["band"]
    nv, nt = _nverts(want), _ntris(want)
    sides = ref["sides"]
    box_nv = sorted(n for n in nv.values() if n > 6)
    assert box_nv == [6 * n * n for n in sides] and len(box_nv) == 2 * len(caps)
    # on either side of each band edge
    for i, edge in enumerate(caps):
        assert box_nv[2 * i] <= edge < box_nv[2 * i + 1]
    assert sum(1 for n in nv.values() if n == 6) >= 20  # the sprinkle
    lds, table = _expect_paths(want, cap)
    assert lds > 0 and table == 1
    # the one over-cap label shares a 256-triangle block of the stream with
    # an LDS-path label wherever it lies: its range [a, a + n) has an end
    # off the block grid with a neighbour behind it. First (a = 0): n is off
    # the grid. Last (a = T - n): a is off the grid. In between: a or a + n.
    (big,) = [k for k in nv if nv[k] > cap]
    total = sum(nt.values())
    assert nt[big] % BLK != 0 and (total - nt[big]) % BLK != 0
    assert nt[big] > 4 * BLK  # and blocks of its own in between


def test_single_voxel_and_tiny_labels(eng, ref, caps):
    """Labels much shorter than one tile: table almost empty, many blocks."""
    for key, nlab in (("single", 1), ("tiny", 60)):
        data, want = ref[key]
        assert len(want) == nlab
        assert max(_ntris(want).values()) < BLK
        assert _expect_paths(want, caps[-1]) == (nlab, 0)
        got = eng.mesh_chunk(data, resolution=RES)
        _assert_meshsets_equal(got, want, key)
        _assert_paths(eng, want, caps[-1], key)


def test_band_edges_all_three_paths(eng, ref, caps):
    _check_band_preconditions(ref, caps)
    data, want = ref["band"]
    got = eng.mesh_chunk(data, resolution=RES)
    _assert_meshsets_equal(got, want, "band edges")
    _assert_paths(eng, want, caps[-1], "band edges")
    st = eng.stats()
    assert st["weld_lds_labels"] > 0 and st["weld_table_labels"] > 0


def test_table_near_full_load(eng, ref, caps):
    small, cap = caps[0], caps[-1]
    data, want = ref["full"]
    nv = _nverts(want)
    assert len(nv) == 6 and min(nv) > (1 << 32)
    assert max(nv.values()) <= cap, nv          # all on the LDS path
    assert max(nv.values()) > small // 2, nv    # tables well filled
    got = eng.mesh_chunk(data, resolution=RES)
    _assert_meshsets_equal(got, want, "near full")
    _assert_paths(eng, want, cap, "near full")


@pytest.mark.parametrize("key", ["dense_small", "dense_big"])
def test_unpadded_dense_volume(eng, ref, caps, key):
    """Labels touch all six faces: boundary bits and the interior index."""
    data, want = ref[key]
    for ax in range(3):
        for side in (0, -1):
            assert np.take(data, side, axis=ax).any()
    lds, table = _expect_paths(want, caps[-1])
    if key == "dense_small":
        assert table == 0 and lds == 4
    else:
        assert (lds, table) == (0, 1)
    got = eng.mesh_chunk(data, resolution=ANISO, voxel_centered=False)
    _assert_meshsets_equal(got, want, key)
    _assert_paths(eng, want, caps[-1], key)


def test_permutation_sort_path(eng, ref, caps, monkeypatch):
    """MG_SORT_RECS=0 (permutation-valued sort) feeds the same weld."""
    _check_band_preconditions(ref, caps)
    monkeypatch.setenv("MG_SORT_RECS", "0")
    data, want = ref["band"]
    _assert_meshsets_equal(eng.mesh_chunk(data, resolution=RES), want,
                           "MG_SORT_RECS=0 band edges")
    _assert_paths(eng, want, caps[-1], "MG_SORT_RECS=0")


def test_simplify_downstream(eng, ref, caps):
    """The per-triangle label array is written by every path and the
    simplifier's scratch buffer is there."""
    _check_band_preconditions(ref, caps)
    data, want = ref["band_simplified"]
    assert sum(_ntris(want).values()) > 0
    got = eng.mesh_chunk(data, resolution=RES, reduction_factor=100,
                         max_error=40.0)
    _assert_meshsets_equal(got, want, "band edges simplified")
    _assert_paths(eng, ref["band"][1], caps[-1], "simplified")


def test_buffer_reuse(eng, ref, caps):
    """Band edges, tiny, band edges on one engine: lazily sized buffers and
    a global table that holds an earlier call's entries."""
    _check_band_preconditions(ref, caps)
    for key in ("band", "single", "band"):
        data, want = ref[key]
        _assert_meshsets_equal(eng.mesh_chunk(data, resolution=RES), want,
                               f"reuse {key}")
        _assert_paths(eng, want, caps[-1], f"reuse {key}")


def test_tile_edges(eng, ref, caps):
    data, want = ref["ladder"]
    nt = sorted(_ntris(want).values())
    assert nt == [12 * n * n - 4 for n in range(1, 13)]
    for edge in (BLK, 2 * BLK):
        assert any(edge - 100 < n < edge for n in nt), nt
        assert any(edge < n < edge + 100 for n in nt), nt
    assert _expect_paths(want, caps[-1]) == (12, 0)
    got = eng.mesh_chunk(data, resolution=RES)
    _assert_meshsets_equal(got, want, "box ladder")
    _assert_paths(eng, want, caps[-1], "box ladder")
