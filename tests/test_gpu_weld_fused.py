"""GPU tests of the weld's position-derived vertex ids (pytest -m gpu):
the flag pass stores each later corner's first stream position in place
of its slot, and one fused kernel derives every vertex id from a position
through the flag-bit words and their scan, writing vertices and faces
together. Shapes are the smallest at which that indexing can go wrong —
a single partial 64-corner word, labels starting mid-word, first
positions many words behind their uses, a tail word — all BIT-EXACT
against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES = (16.0, 16.0, 40.0)
ANISO = (4.0, 16.0, 40.0)


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


def _ncorners(meshes: dict) -> int:
    return 3 * sum(int(f.shape[0]) for _, f in meshes.values())


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
    assert ids.size == n and ids.min() > (1 << 32)
    data = np.zeros((7, 6, 5), dtype=np.uint64, order="F")
    data[1:-1, 1:-1, 1:-1] = ids.reshape((5, 4, 3))
    return np.asfortranarray(data)


def _big_box(dtype):
    data = np.zeros((24, 24, 24), dtype=dtype, order="F")
    data[2:22, 2:22, 2:22] = 7 if dtype == np.uint32 else (1 << 36) + 7
    return data


def _random_labels():
    """The 40x37x29 pattern of test_oracle_parity_random_u64, other seed."""
    rng = np.random.default_rng(4321)
    data = np.zeros((40, 37, 29), dtype=np.uint64, order="F")
    data[1:-1, 1:-1, 1:-1] = rng.integers(
        0, 7, size=(38, 35, 27)).astype(np.uint64)
    ids = np.concatenate(
        [[0], rng.integers(1, 1 << 40, size=6)]).astype(np.uint64)
    return np.asfortranarray(ids[data])


@pytest.fixture(scope="module")
def ref():
    """Inputs and oracle results, computed once and shared read-only."""
    import oracle
    single = _single_voxel()
    tiny = _tiny_labels()
    box32 = _big_box(np.uint32)
    box64 = _big_box(np.uint64)
    rnd = _random_labels()
    out = {
        "single": (single, oracle.mesh_chunk(single, resolution=RES)),
        "tiny": (tiny, oracle.mesh_chunk(tiny, resolution=RES)),
        "tiny_simplified": (tiny, oracle.mesh_chunk(
            tiny, resolution=RES, reduction_factor=100, max_error=40.0)),
        "box32": (box32, oracle.mesh_chunk(box32, resolution=RES)),
        "box64": (box64, oracle.mesh_chunk(box64, resolution=RES)),
        "box64_simplified": (box64, oracle.mesh_chunk(
            box64, resolution=RES, reduction_factor=4, max_error=1e9)),
    }
    for vc in (True, False):
        out[f"random_vc{int(vc)}"] = (rnd, oracle.mesh_chunk(
            rnd, resolution=ANISO, voxel_centered=vc))
    return out


def test_single_voxel_one_partial_word(eng, ref):
    data, want = ref["single"]
    got = eng.mesh_chunk(data, resolution=RES)
    _assert_meshsets_equal(got, want, "single voxel")
    nc = _ncorners(got)
    assert 0 < nc < 64, f"{nc} corners: expected one partial word"


def test_many_tiny_labels_start_mid_word(eng, ref):
    data, want = ref["tiny"]
    got = eng.mesh_chunk(data, resolution=RES)
    _assert_meshsets_equal(got, want, "tiny labels")
    assert len(got) == 60
    # several labels per 64-corner word: label streams start mid-word
    assert max(3 * f.shape[0] for _, f in got.values()) < 64
    assert _ncorners(got) > 64


@pytest.mark.parametrize("key", ["box32", "box64"])
def test_one_large_label(eng, ref, key):
    data, want = ref[key]
    got = eng.mesh_chunk(data, resolution=RES)
    _assert_meshsets_equal(got, want, key)
    assert len(got) == 1
    assert _ncorners(got) > 64 * 100  # first positions many words back


@pytest.mark.parametrize("vc", [False, True])
def test_random_labels_aniso(eng, ref, vc):
    data, want = ref[f"random_vc{int(vc)}"]
    got = eng.mesh_chunk(data, resolution=ANISO, voxel_centered=vc)
    _assert_meshsets_equal(got, want, f"random vc={vc}")


def test_tail_word(eng, ref):
    """Total corner count not a multiple of 64: the last flag word is
    partial, and the last triangles' ids come from it."""
    for key in ("single", "tiny", "random_vc1"):
        data, want = ref[key]
        res = ANISO if key.startswith("random") else RES
        got = eng.mesh_chunk(data, resolution=res)
        assert _ncorners(got) % 64 != 0, f"{key}: no tail word"
        _assert_meshsets_equal(got, want, f"tail {key}")


def test_permutation_sort_path(eng, ref, monkeypatch):
    """MG_SORT_RECS=0 (permutation-valued sort) feeds the same weld."""
    monkeypatch.setenv("MG_SORT_RECS", "0")
    for key, res in (("random_vc1", ANISO), ("tiny", RES)):
        data, want = ref[key]
        _assert_meshsets_equal(eng.mesh_chunk(data, resolution=res), want,
                               f"MG_SORT_RECS=0 {key}")


def test_buffer_reuse(eng, ref):
    """Large, tiny, large again on one engine: the entry array is rewritten
    in place by every call and the buffers are grow-only."""
    for key in ("box64", "single", "box64"):
        data, want = ref[key]
        _assert_meshsets_equal(eng.mesh_chunk(data, resolution=RES), want,
                               f"reuse {key}")


def test_simplify_downstream(eng, ref):
    data, want = ref["tiny_simplified"]
    got = eng.mesh_chunk(data, resolution=RES, reduction_factor=100,
                         max_error=40.0)
    _assert_meshsets_equal(got, want, "tiny labels simplified")
    # the 8-triangle labels collapse away entirely at that factor; a mesh
    # that survives simplification checks the hand-over with real output
    data, want = ref["box64_simplified"]
    assert _ncorners(want) > 0
    got = eng.mesh_chunk(data, resolution=RES, reduction_factor=4,
                         max_error=1e9)
    _assert_meshsets_equal(got, want, "large box simplified")
