"""GPU tests for mg_retriangulate_mesh: one device call must return exactly
what the host composition returns — meshops.chunk_mesh, Mesh.concatenate
of the cells in dict order, meshops.merge_close_vertices —
and tasks/multires.py must route to it when no seam is injected."""
import numpy as np
import pytest

from merge_close_inputs import (BOX_RES, CAT_GRID, assert_no_ties,
                                assert_same_mesh, box, box_simplified,
                                host_chunks)

pytestmark = pytest.mark.gpu

R = 1e-5
# (mesh, scale, offset): real clipping; planes on vertex coordinates; cells
# 1.37 voxels wide off the voxel grid; the simplified box, whose faces span
# many cells; one cell around the whole mesh
GRIDS = {
    "clip": ("box",) + CAT_GRID,
    "planes": ("box", (32, 32, 320), (0, 0, 0)),
    "many": ("box", tuple(1.37 * x for x in BOX_RES), (3.1, 5.3, 7.7)),
    "simplified": ("box_simplified", (8, 8, 80), (0, 0, 0)),
    "one_cell": ("box", (1000, 1000, 10000), (-50, -50, -500)),
}
MESHES = {"box": box, "box_simplified": box_simplified}


def _gpu_engine():
    from igneous_amd.engine import Engine
    return Engine.get(0)


def _host(grid):
    """The host composition for a named grid, computed once."""
    from igneous_amd import meshops
    from igneous_amd.meshes import Mesh
    which, scale, offset = GRIDS[grid]
    cv, cf, ncells = host_chunks(which, scale, offset)
    if grid not in _host.cache:
        assert_no_ties(cv, R)
        m = meshops.merge_close_vertices(Mesh(cv, cf, id=1), radius=R)
        _host.cache[grid] = (m.vertices, m.faces, cv.shape[0], ncells)
    return _host.cache[grid]


_host.cache = {}


def _check(eng, grid):
    which, scale, offset = GRIDS[grid]
    v, f = MESHES[which]()
    wv, wf, ncat, ncells = _host(grid)
    got = eng.retriangulate_mesh(v, f, scale, offset, R)
    assert_same_mesh(got, (wv, wf), grid)
    return got, ncat, ncells


@pytest.mark.parametrize("grid", list(GRIDS))
def test_retriangulate_equals_host_composition(grid):
    got, ncat, ncells = _check(_gpu_engine(), grid)
    if grid == "clip":
        assert ncells == 36 and got[1].shape[0] == 11582
    elif grid == "planes":
        assert ncells == 27 and ncat == 5226
        assert got[0].shape[0] == 4398 and got[1].shape[0] == 8176
    elif grid == "many":
        assert ncells > 1000
    elif grid == "simplified":
        assert MESHES["box_simplified"]()[1].shape[0] == 306
    else:
        assert ncells == 1


def test_larger_radius_merges_through_the_cell_seams():
    from igneous_amd import meshops
    from igneous_amd.meshes import Mesh
    which, scale, offset = GRIDS["clip"]
    cv, cf, _ = host_chunks(which, scale, offset)
    assert_no_ties(cv, 2.3)
    want = meshops.merge_close_vertices(Mesh(cv, cf), radius=2.3)
    got = _gpu_engine().retriangulate_mesh(*box(), scale, offset, 2.3)
    assert_same_mesh(got, (want.vertices, want.faces), "r=2.3")
    assert got[0].shape[0] == 4815 and got[1].shape[0] == 9024


def test_mesh_without_faces_comes_back_unchanged():
    v = np.arange(12, dtype=np.float32).reshape(4, 3)
    none = np.zeros((0, 3), np.uint32)
    gv, gf = _gpu_engine().retriangulate_mesh(v, none, (1, 1, 1), (0, 0, 0))
    assert_same_mesh((gv, gf), (v, none))


def test_mesh_of_degenerate_faces_comes_back_unchanged():
    """Every face has two corners at one position: chunk_mesh keeps no
    cell, and the host function hands the mesh back."""
    from igneous_amd import meshops
    from igneous_amd.meshes import Mesh
    v = np.array([[.25, .25, .25], [.25, .25, .25], [.5, .5, .5]],
                 np.float32)
    f = np.array([[0, 1, 2], [1, 0, 2]], np.uint32)
    assert meshops.chunk_mesh(Mesh(v, f), (1, 1, 1), (0, 0, 0)) == {}
    got = _gpu_engine().retriangulate_mesh(v, f, (1, 1, 1), (0, 0, 0))
    assert_same_mesh(got, (v, f))


def test_invalid_arguments_are_clean_errors():
    eng = _gpu_engine()
    v, f = box_simplified()
    with pytest.raises(RuntimeError, match="must be > 0"):
        eng.retriangulate_mesh(v, f, (8, 0, 80), (0, 0, 0))
    with pytest.raises(ValueError, match="radius"):
        eng.retriangulate_mesh(v, f, (8, 8, 80), (0, 0, 0), radius=0)
    _check(eng, "simplified")


def test_small_call_after_a_larger_one():
    eng = _gpu_engine()
    _check(eng, "many")
    _check(eng, "simplified")
    _check(eng, "one_cell")


def test_first_call_retriangulate_mesh():
    from igneous_amd.engine import Engine
    which, scale, offset = GRIDS["clip"]
    eng = Engine(0)
    try:
        got = eng.retriangulate_mesh(*box(), scale, offset, R)
    finally:
        eng.lib.mg_destroy(eng.ctx)
        eng.ctx = None
    assert_same_mesh(got, _host("clip")[:2], "first call")


def test_multires_routes_to_the_engine(monkeypatch):
    """No seam injected: multires.retriangulate_mesh is the engine call.
    With the host chunker injected it is the host composition, and the
    engine's retriangulate_mesh is not called."""
    from igneous_amd import meshops
    from igneous_amd.engine import Engine
    from igneous_amd.meshes import Mesh
    from igneous_amd.tasks import multires

    calls = []
    real = Engine.retriangulate_mesh

    def counted(self, *a, **kw):
        calls.append(1)
        return real(self, *a, **kw)

    monkeypatch.setattr(Engine, "retriangulate_mesh", counted)
    which, scale, offset = GRIDS["clip"]
    v, f = box()
    want = _host("clip")[:2]
    got = multires.retriangulate_mesh(Mesh(v, f, id=9), offset, scale)
    assert len(calls) == 1 and got.id == 9
    assert_same_mesh((got.vertices, got.faces), want, "product path")
    multires.set_chunker(meshops.chunk_mesh)
    try:
        del calls[:]
        got = multires.retriangulate_mesh(Mesh(v, f, id=9), offset, scale)
    finally:
        multires.set_chunker(None)
    assert calls == [] and got.id == 9
    assert_same_mesh((got.vertices, got.faces), want, "host composition")
