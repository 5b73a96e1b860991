"""CPU tests of what the device weld is held to, and of the
retriangulator seam of tasks/multires.py. No GPU, no engine.

The contract, restated with numpy and scipy alone in
merge_close_inputs.contract_ref, must equal the checker
meshops.merge_close_vertices on every input the GPU tests use; those inputs
must have no pair within a relative 1e-6 of the radius, where cKDTree's own
rounding could decide."""
import numpy as np
import pytest

from merge_close_inputs import (WELD_CASES, assert_no_ties, assert_same_mesh,
                                contract_ref, host_weld, mesh_input,
                                pair_counts)


@pytest.mark.parametrize("case", list(WELD_CASES))
def test_contract_restatement_equals_host_weld(case):
    name, r, nv, nf = WELD_CASES[case]
    v, f = mesh_input(name)
    assert_no_ties(v, r)
    want = host_weld(name, r)
    assert want[0].shape == (nv, 3) and want[1].shape == (nf, 3), \
        (case, want[0].shape, want[1].shape)
    assert_same_mesh(contract_ref(v, f, r), want, case)


def test_tie_condition_sees_the_clip_plane_radii():
    """r = 0.5 on the clipped box is the kind of radius the condition
    exists to keep out: the clip planes sit 0.5 from half-grid vertices."""
    v, _ = mesh_input("cat")
    counts = pair_counts(v, 0.5)
    assert not counts[0] == counts[1] == counts[2]


def test_vertices_without_faces_and_empty_mesh():
    from igneous_amd import meshops
    from igneous_amd.meshes import Mesh
    v = np.arange(12, dtype=np.float32).reshape(4, 3)
    none = np.zeros((0, 3), np.uint32)
    m = meshops.merge_close_vertices(Mesh(v, none), radius=1e-5)
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3)
    assert_same_mesh(contract_ref(v, none, 1e-5), (m.vertices, m.faces))
    e = meshops.merge_close_vertices(
        Mesh(np.zeros((0, 3), np.float32), none), radius=1e-5)
    assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3)


# --- the retriangulator seam, with stub functions --------------------------

@pytest.fixture
def multires_mod():
    from igneous_amd.tasks import multires
    yield multires
    multires.set_retriangulator(None)
    multires.set_chunker(None)
    multires.set_simplifier(None)


def _tiny_mesh():
    from igneous_amd.meshes import Mesh
    v = np.array([[.2, .2, .2], [2.7, .3, .1], [.3, 2.6, .2]], np.float32)
    return Mesh(v, np.array([[0, 1, 2]], np.uint32), id=7)


def test_set_retriangulator_is_exported(multires_mod):
    assert "set_retriangulator" in multires_mod.__all__
    assert callable(multires_mod.set_retriangulator)


def test_injected_retriangulator_gets_mesh_scale_offset(multires_mod):
    mesh = _tiny_mesh()
    calls = []

    def stub(m, scale, offset):
        calls.append((m, scale, offset))
        return "result"

    multires_mod.set_retriangulator(stub)
    # retriangulate_mesh takes (offset, scale), the seam (scale, offset)
    got = multires_mod.retriangulate_mesh(mesh, "the offset", "the scale")
    assert got == "result"
    assert calls == [(mesh, "the scale", "the offset")]


def test_injected_retriangulator_wins_over_an_injected_chunker(multires_mod):
    def chunker(m, scale, offset):
        raise AssertionError("the chunker must not run")

    multires_mod.set_chunker(chunker)
    multires_mod.set_retriangulator(lambda m, s, o: m)
    mesh = _tiny_mesh()
    assert multires_mod.retriangulate_mesh(mesh, (0, 0, 0), (1, 1, 1)) is mesh


def test_injected_chunker_routes_to_the_host_composition(multires_mod):
    from igneous_amd import meshops
    from igneous_amd.meshes import Mesh
    mesh = _tiny_mesh()
    calls = []

    def chunker(m, scale, offset):
        calls.append((scale, offset))
        return meshops.chunk_mesh(m, scale, offset)

    multires_mod.set_chunker(chunker)
    got = multires_mod.retriangulate_mesh(mesh, (0, 0, 0), (1, 1, 1))
    assert calls == [((1, 1, 1), (0, 0, 0))]
    cells = meshops.chunk_mesh(mesh, (1, 1, 1), (0, 0, 0))
    want = meshops.merge_close_vertices(
        Mesh.concatenate(*cells.values(), id=7), radius=1e-5)
    assert got.id == 7
    assert_same_mesh((got.vertices, got.faces), (want.vertices, want.faces))
    # no chunks: the mesh itself comes back
    multires_mod.set_chunker(lambda m, s, o: {})
    assert multires_mod.retriangulate_mesh(mesh, (0, 0, 0), (1, 1, 1)) is mesh


def test_injected_simplifier_keeps_the_host_composition(multires_mod):
    multires_mod.set_simplifier(lambda m, target: m)
    assert multires_mod._get_retriangulator() \
        is multires_mod._host_retriangulate


def test_set_retriangulator_none_restores_the_default(multires_mod):
    stub = lambda m, s, o: m
    multires_mod.set_retriangulator(stub)
    assert multires_mod._get_retriangulator() is stub
    multires_mod.set_retriangulator(None)
    default = multires_mod._get_retriangulator()
    assert default is not stub
    assert default is not multires_mod._host_retriangulate
    assert default.__name__ == "gpu_retriangulate"
