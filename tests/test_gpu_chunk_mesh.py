"""GPU tests for mg_chunk_mesh: the device grid chunker must return exactly
what the host function meshops.chunk_mesh returns — the same cell keys in
the same dict order, the same uint32 faces and the same float32 vertex
bits per cell."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _gpu_engine():
    from igneous_amd.engine import Engine
    return Engine.get(0)


def _mesh(v, f, id=1):
    from igneous_amd.meshes import Mesh
    return Mesh(np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3),
                np.ascontiguousarray(f, dtype=np.uint32).reshape(-1, 3),
                id=id)


def _assert_same(got, want, what=""):
    """got: {key: (verts, faces)} from the engine; want: {key: Mesh}."""
    assert list(got.keys()) == list(want.keys()), \
        f"{what}: keys/order differ: {list(got)[:6]} vs {list(want)[:6]}"
    for key, m in want.items():
        gv, gf = got[key]
        assert gf.dtype == np.uint32 and gv.dtype == np.float32
        assert gf.shape == m.faces.shape, (what, key, gf.shape, m.faces.shape)
        assert np.array_equal(gf, m.faces), f"{what}: faces differ in {key}"
        assert gv.shape == m.vertices.shape, \
            (what, key, gv.shape, m.vertices.shape)
        assert np.array_equal(
            np.ascontiguousarray(gv).view(np.uint32),
            np.ascontiguousarray(m.vertices).view(np.uint32)), \
            f"{what}: vertex bits differ in {key}"


def _check(v, f, scale, offset, what="", eng=None):
    from igneous_amd import meshops
    eng = eng or _gpu_engine()
    mesh = _mesh(v, f)
    want = meshops.chunk_mesh(mesh, scale, offset)
    got = eng.chunk_mesh(mesh.vertices, mesh.faces, scale, offset)
    _assert_same(got, want, what)
    return want


@pytest.fixture(scope="module")
def box():
    """The roughened 24^3 box of test_simplify_mesh_parity_vs_oracle
    (seed 17, resolution (4, 4, 40)): 8176 faces."""
    import oracle
    rng = np.random.default_rng(17)
    n = 24
    data = np.zeros((n, n, n), dtype=np.uint64, order="F")
    data[1:-1, 1:-1, 1:-1] = 1
    carve = rng.integers(1, n - 1, size=(n * n // 2, 3))
    data[carve[:, 0], carve[:, 1], carve[:, 2]] = 0
    v, f = oracle.mesh_chunk(data, resolution=(4.0, 4.0, 40.0))[1]
    assert f.shape[0] == 8176
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


@pytest.fixture(scope="module")
def box_simplified(box):
    import oracle
    v, f = oracle.simplify_mesh(box[0], box[1], 20, 1e30)
    assert f.shape[0] == 306
    return v, f


def test_box_planes_on_vertex_coordinates(box):
    """Every grid plane coincides with half-grid vertex coordinates:
    nothing crosses, the -1e-12 and on-plane-is-inside rules decide."""
    want = _check(box[0], box[1], (32, 32, 320), (0, 0, 0), "planes")
    assert len(want) == 27
    assert sum(len(m.faces) for m in want.values()) == 8176


def test_box_real_clipping(box):
    want = _check(box[0], box[1], (30, 30, 300), (-3.5, 1.25, 7), "clip")
    assert len(want) == 36
    assert sum(len(m.faces) for m in want.values()) == 11582


def test_box_many_cells(box):
    want = _check(box[0], box[1], (8, 8, 80), (0, 0, 0), "many")
    assert len(want) == 1248


def test_box_negative_cells(box):
    want = _check(box[0], box[1], (30, 30, 300), (50, 50, 500), "negative")
    assert min(k[0] for k in want) < 0


def test_simplified_faces_span_many_cells(box_simplified):
    v, f = box_simplified
    want = _check(v, f, (8, 8, 80), (0, 0, 0), "simplified")
    assert len(want) == 746
    assert sum(len(m.faces) for m in want.values()) == 5048


# hand-made faces, scale 1, offset 0: (name, verts)
_HAND = [
    # a triangle across 3x3 cells (also half of the two-face order case)
    ("span3x3", [[.2, .2, .2], [2.7, .3, .1], [.3, 2.6, .2]]),
    # a vertex exactly on the plane x=1 with its neighbour outside: the
    # t = 0 duplicate -> a degenerate fan face and an unused vertex
    ("on_plane_vertex", [[1.0, .25, .5], [1.75, .5, .5], [.25, .75, .5]]),
    # lies in the grid plane z=1
    ("in_plane", [[.25, .25, 1.0], [1.5, .25, 1.0], [.25, 1.5, 1.0]]),
    # zero-area input face (two corners share a position)
    ("zero_area", [[.25, .25, .25], [.25, .25, .25], [.5, .5, .5]]),
    # -0.0 against +0.0 in one cell
    ("neg_zero_a", [[-0.0, .25, .25], [.5, .25, .25], [.25, .5, .25]]),
    ("neg_zero_b", [[0.0, .25, .25], [.25, .5, .25], [.25, .25, .75]]),
    # two input vertices at one position used by different faces of a cell
    ("dup_pos_a", [[4.25, 4.25, 4.25], [4.5, 4.25, 4.25], [4.25, 4.5, 4.25]]),
    ("dup_pos_b", [[4.25, 4.25, 4.25], [4.25, 4.5, 4.25], [4.25, 4.25, 4.75]]),
    # the tiny triangle of the two-face order case
    ("tiny_at_5", [[5.1, 5.1, 5.1], [5.2, 5.1, 5.1], [5.1, 5.2, 5.1]]),
]


def _hand_mesh(names):
    v, f = [], []
    for name, tri in _HAND:
        if name in names:
            f.append([len(v), len(v) + 1, len(v) + 2])
            v.extend(tri)
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.uint32)


@pytest.mark.parametrize("name", [n for n, _ in _HAND])
def test_hand_made_face_alone(name):
    v, f = _hand_mesh({name})
    _check(v, f, (1, 1, 1), (0, 0, 0), name)


def test_hand_made_faces_together():
    v, f = _hand_mesh({n for n, _ in _HAND})
    want = _check(v, f, (1, 1, 1), (0, 0, 0), "all hand-made")
    assert (0, 0, 0) in want


def test_two_face_dict_order():
    """Cells with an interior face come first, then cells in order of
    their first boundary fragment: [(5,5,5), (0,0,0), (0,1,0), ...]."""
    v, f = _hand_mesh({"span3x3", "tiny_at_5"})
    want = _check(v, f, (1, 1, 1), (0, 0, 0), "order")
    assert list(want)[:3] == [(5, 5, 5), (0, 0, 0), (0, 1, 0)]


def _soup():
    rng = np.random.default_rng(2024)
    tri = rng.uniform(-0.6, 3.6, size=(500, 3, 3))
    tri[::3] = np.round(tri[::3] * 2) / 2
    v = tri.reshape(-1, 3).astype(np.float32)
    f = np.arange(1500, dtype=np.uint32).reshape(-1, 3)
    return v, f


@pytest.mark.parametrize("scale", [(1, 1, 1), (1, 0.75, 1.5)])
def test_triangle_soup(scale):
    v, f = _soup()
    want = _check(v, f, scale, (0.1, -0.2, 0), f"soup {scale}")
    assert len(want) > 27


def test_deterministic_and_no_stale_buffers(box):
    """The same call twice gives equal output, and a small mesh after the
    large one on the same engine still equals the host."""
    eng = _gpu_engine()
    args = (box[0], box[1], (30, 30, 300), (-3.5, 1.25, 7))
    a = eng.chunk_mesh(*args)
    b = eng.chunk_mesh(*args)
    assert list(a) == list(b)
    for key in a:
        assert np.array_equal(a[key][1], b[key][1])
        assert np.array_equal(a[key][0].view(np.uint32),
                              b[key][0].view(np.uint32))
    v, f = _hand_mesh({n for n, _ in _HAND})
    _check(v, f, (1, 1, 1), (0, 0, 0), "small after large", eng)


def test_empty_mesh():
    eng = _gpu_engine()
    assert eng.chunk_mesh(np.zeros((0, 3), np.float32),
                          np.zeros((0, 3), np.uint32), (1, 1, 1),
                          (0, 0, 0)) == {}


@pytest.mark.parametrize("case", ["face_index", "nan_vertex", "zero_scale"])
def test_out_of_contract_is_a_clean_error(case):
    """Input validation rejects before any kernel runs; the engine stays
    usable."""
    eng = _gpu_engine()
    v, f = _hand_mesh({"span3x3", "tiny_at_5"})
    scale = (1, 1, 1)
    if case == "face_index":
        f = f.copy()
        f[1, 2] = v.shape[0]
        match = "references vertex"
    elif case == "nan_vertex":
        v = v.copy()
        v[4, 1] = np.nan
        match = "not finite"
    else:
        scale = (0, 1, 1)
        match = "must be > 0"
    with pytest.raises(RuntimeError, match=match):
        eng.chunk_mesh(v, f, scale, (0, 0, 0))
    v, f = _hand_mesh({"span3x3", "tiny_at_5"})
    _check(v, f, (1, 1, 1), (0, 0, 0), "after error", eng)


@pytest.mark.parametrize("case", ["cell_range", "pairs", "bounding_box"])
def test_capacity_bounds_are_clean_errors(case):
    """The bounds the first device pass checks: a cell coordinate outside
    [-2^20, 2^20), more than 2^31 (face, cell) pairs, a cell bounding box
    of more than 2^31 cells. Each fails the call and leaves the engine
    usable."""
    eng = _gpu_engine()
    v, f = _hand_mesh({"span3x3", "tiny_at_5"})
    v = v.copy()
    scale = (1, 1, 1)
    if case == "cell_range":
        v[3:6] += np.float32(2.0e6)
        match = "cell coordinate"
    elif case == "pairs":
        v[0], v[1], v[2] = (0, 0, 0), (2000, 0, 2000), (0, 2000, 2000)
        match = "pairs"
    else:
        v[3:6] += np.float32(3000.0)
        match = "bounding box"
    with pytest.raises(RuntimeError, match=match):
        eng.chunk_mesh(v, f, scale, (0, 0, 0))
    v, f = _hand_mesh({"span3x3", "tiny_at_5"})
    _check(v, f, (1, 1, 1), (0, 0, 0), "after error", eng)


def test_pipeline_device_chunker_equals_host_chunker(box, oracle_simplifier):
    """process_mesh with the oracle simplifier in both runs: the device
    chunker and the host chunker give the same manifest and fragment
    bytes."""
    from igneous_amd import engine, meshops
    from igneous_amd.tasks import multires as multires_mod

    vol = types.SimpleNamespace(resolution=(4, 4, 40))
    mesh_info = {"vertex_quantization_bits": 16}

    def run(chunker):
        multires_mod.set_chunker(chunker)
        try:
            manifest, frags = multires_mod.process_mesh(
                vol, mesh_info, 1, _mesh(box[0].copy(), box[1].copy()),
                num_lod=2, min_chunk_size=(4, 4, 4))
        finally:
            multires_mod.set_chunker(None)
        assert manifest is not None and manifest.num_lods > 1
        return manifest.to_binary(), frags

    dev = run(engine.chunk_mesh)
    host = run(meshops.chunk_mesh)
    assert dev[0] == host[0], "manifest bytes differ"
    assert dev[1] == host[1], "fragment bytes differ"
    assert len(host[1]) > 0
