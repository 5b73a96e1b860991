"""Context lifecycle (the GPU part runs under pytest -m gpu): mg_destroy
releases a context that has used every buffer family — label hash, label
map, fill volumes, the mesher's and the simplifier's buffers with their
swaps, the pinned staging — and a fresh context computes the same results
afterwards. The volume's properties are checked on the CPU without a GPU.
Private Engines are used so the shared Engine.get cache never holds a
destroyed ctx."""
import numpy as np
import pytest

RES = (16.0, 16.0, 40.0)
A, B, C, D, E = (1 << 33) + 7, (1 << 36) + 3, 9, (1 << 40) + 1, (1 << 35) + 2
B2, C2 = (1 << 34) + 5, 11
LABEL_MAP = (np.array([B, C], dtype=np.uint64),
             np.array([B2, C2], dtype=np.uint64), 'keep')


def _volume():
    """12x11x10 u64: A encloses a one-voxel cavity and the 2x2x2 label E
    (the hole mesh); B and C are remapped; D is a single voxel that
    dust_threshold=2 removes."""
    v = np.zeros((12, 11, 10), dtype=np.uint64, order="F")
    v[1:7, 1:10, 1:9] = A
    v[3, 5, 4] = 0
    v[3:5, 2:4, 6:8] = E
    v[7:11, 1:10, 1:5] = B
    v[7:11, 1:10, 5:9] = C
    v[0, 0, 0] = D
    return v


def _single_voxel():
    data = np.zeros((3, 3, 3), dtype=np.uint32, order="F")
    data[1, 1, 1] = 5
    return data


def _sequence(eng):
    vol = _volume()
    filled, holes = eng.mesh_chunk(
        vol, resolution=RES, reduction_factor=2, dust_threshold=2,
        label_map=LABEL_MAP, fill_holes=2)
    fvol, hvol, rounds = eng.fill_holes(vol, level=1)
    big = max(filled, key=lambda lab: filled[lab][1].shape[0])
    sv, sf = eng.simplify_mesh(filled[big][0], filled[big][1], 2)
    return {"filled": filled, "holes": holes, "fvol": fvol, "hvol": hvol,
            "rounds": rounds, "big": big, "sv": sv, "sf": sf}


def _assert_meshsets_equal(got: dict, want: dict, what=""):
    assert sorted(got.keys()) == sorted(want.keys()), \
        f"{what}: label sets differ ({len(got)} vs {len(want)})"
    for label in want:
        for g, w, part in zip(got[label], want[label], ("verts", "faces")):
            assert g.shape == w.shape and np.array_equal(g, w), \
                f"{what} label {label}: {part} differ"


def _assert_sequences_equal(got, want, what):
    _assert_meshsets_equal(got["filled"], want["filled"], f"{what} filled")
    _assert_meshsets_equal(got["holes"], want["holes"], f"{what} holes")
    for key in ("fvol", "hvol", "sv", "sf"):
        assert np.array_equal(got[key], want[key]), f"{what}: {key} differs"
    assert got["rounds"] == want["rounds"] and got["big"] == want["big"]


def _destroy(eng):
    eng.lib.mg_destroy(eng.ctx)
    eng.ctx = None


def test_volume_has_holes_and_simplifies():
    """CPU check of the inputs: the fill changes something, the hole mesh
    is non-empty and the simplifier removes faces."""
    import oracle
    from fill_holes_ref import fill_holes_ref
    vol = _volume()
    vol[vol == D] = 0                      # dust
    vol[vol == B] = B2                     # label map
    vol[vol == C] = C2
    filled, holes, _ = fill_holes_ref(vol, 2)
    assert filled[3, 5, 4] == A            # the cavity
    assert np.count_nonzero(filled != vol) == 1 + 8
    # the hole volume holds the INPUT where the fill changed it: 0 at the
    # background cavity, E at the enclosed label — E is the hole mesh
    assert np.count_nonzero(holes == E) == 8
    hole_meshes = oracle.mesh_chunk(holes, resolution=RES)
    full = oracle.mesh_chunk(filled, resolution=RES)
    simp = oracle.mesh_chunk(filled, resolution=RES, reduction_factor=2)
    assert sum(f.shape[0] for _, f in simp.values()) < \
        sum(f.shape[0] for _, f in full.values())
    assert sorted(hole_meshes) == [E]
    # ... and again in the standalone call on the already simplified mesh
    big = max(simp, key=lambda lab: simp[lab][1].shape[0])
    _, sf = oracle.simplify_mesh(simp[big][0], simp[big][1], 2)
    assert 0 < sf.shape[0] < simp[big][1].shape[0]


@pytest.mark.gpu
def test_destroy_then_fresh_ctx_agrees():
    from igneous_amd.engine import Engine
    shared = Engine.get(0)
    want = _sequence(shared)
    assert sorted(want["holes"]) == [E]
    assert sorted(want["filled"]) == sorted([A, B2, C2])
    assert want["sf"].shape[0] < want["filled"][want["big"]][1].shape[0]
    assert np.count_nonzero(want["fvol"] != _volume()) > 0

    for run in (1, 2):
        eng = Engine(0)
        try:
            got = _sequence(eng)
        finally:
            _destroy(eng)
        _assert_sequences_equal(got, want, f"private ctx {run}")

    # destroying a ctx left the device's other contexts usable
    import oracle
    single = _single_voxel()
    _assert_meshsets_equal(shared.mesh_chunk(single, resolution=RES),
                           oracle.mesh_chunk(single, resolution=RES),
                           "shared ctx after destroy")
    _assert_sequences_equal(_sequence(shared), want, "shared ctx again")
