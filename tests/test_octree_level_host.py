"""The level encoder seam of tasks.multires, the shared per-level host
function and the integer-draco size formula. No GPU.
"""
import os
import types

import numpy as np
import pytest

import octree_level_ref as ref
from igneous_amd import meshops
from igneous_amd.formats import draco
from igneous_amd.meshes import Mesh
from igneous_amd.tasks import multires

# in a directory of its own: test_golden_integrity.py takes every .npz
# directly under golden/ for an oracle fixture
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "octree_level", "sheet33.npz")


def _identity_simplifier(mesh, target_count):
    return Mesh(mesh.vertices.copy(), mesh.faces.copy(), id=mesh.id)


@pytest.fixture
def clean_seams():
    yield
    multires.set_simplifier(None)
    multires.set_chunker(None)
    multires.set_retriangulator(None)
    multires.set_level_encoder(None)


def _process_sheet33():
    """process_mesh on the 33 x 33 sheet as the fixture was recorded: three
    LODs of the same mesh (an identity simplifier), 10 bits."""
    vol = types.SimpleNamespace(resolution=(1.0, 1.0, 1.0))
    return multires.process_mesh(
        vol, {"vertex_quantization_bits": 10}, 1, ref.sheet(33), 2,
        min_chunk_size=(4, 4, 4))


def test_seam_selection(clean_seams):
    default = (multires.engine_level_encoder
               if multires.DEVICE_LEVEL_ENCODER_DEFAULT
               else multires.encode_octree_level_host)
    assert multires._get_level_encoder() is default

    def injected(*a, **kw):
        raise AssertionError("not called")
    multires.set_level_encoder(injected)
    assert multires._get_level_encoder() is injected
    # an injected encoder wins over the host-sequence rule too
    multires.set_simplifier(_identity_simplifier)
    assert multires._get_level_encoder() is injected
    multires.set_level_encoder(None)
    assert multires._get_level_encoder() is multires.encode_octree_level_host
    multires.set_simplifier(None)
    assert multires._get_level_encoder() is default

    for setter, fn in ((multires.set_chunker, meshops.chunk_mesh),
                       (multires.set_retriangulator,
                        lambda mesh, scale, offset: mesh)):
        setter(fn)
        assert multires._get_level_encoder() is \
            multires.encode_octree_level_host
        setter(None)
        assert multires._get_level_encoder() is default


def test_process_mesh_matches_recorded_parent(clean_seams):
    """The fixture holds the manifest and fragment bytes process_mesh gave
    on the 33 x 33 sheet BEFORE its per-level body moved into
    encode_octree_level_host (recorded from that commit with the host
    chunker, an identity simplifier, num_lod=2, min_chunk_size=(4, 4, 4),
    10 bits: 31 / 7 / 1 fragments)."""
    gold = np.load(GOLDEN)
    multires.set_simplifier(_identity_simplifier)
    manifest, blob = _process_sheet33()
    assert manifest.num_fragments_per_lod == [31, 7, 1]
    assert manifest.to_binary() == gold["manifest"].tobytes()
    assert blob == gold["blob"].tobytes()


def test_level_function_matches_recorded_parent_and_inline_loop():
    """The shared per-level function, level by level, against the recorded
    bytes and against the loop written out on the formats alone."""
    gold = np.load(GOLDEN)
    mesh = ref.sheet(33)
    origin, chunk = ref.grid_for(mesh, 3)
    levels = [ref.host_level(mesh, chunk, lod, 3, origin, 10)
              for lod in range(3)]
    assert b"".join(b for _, _, b in levels) == gold["blob"].tobytes()
    largest = []
    for lod, (nodes, sizes, blob) in enumerate(levels):
        inline = ref.inline_level(mesh, chunk, lod, 3, origin, 10)
        assert tuple(nodes) == inline[0]
        assert list(sizes) == inline[1]
        assert blob == inline[2]
        largest.append(max(
            draco.decode(b)[0].shape[0] for b in ref.split(sizes, blob)))
    # the u8 band (lod 0) and the u16 band (lods 1 and 2)
    assert largest[0] < 256 <= largest[1] and largest[2] >= 256, largest


def test_injected_level_encoder_equals_host_path(clean_seams):
    multires.set_simplifier(_identity_simplifier)
    want_manifest, want_blob = _process_sheet33()
    calls = []

    def wrapped(*a, **kw):
        calls.append(a[2])
        return multires.encode_octree_level_host(*a, **kw)
    multires.set_level_encoder(wrapped)
    got_manifest, got_blob = _process_sheet33()
    assert calls == [0, 1, 2]
    assert got_manifest.to_binary() == want_manifest.to_binary()
    assert got_blob == want_blob


@pytest.mark.parametrize("nv", [3, 255, 256, 65535, 65536, 70001,
                                (1 << 21) - 1, 1 << 21])
def test_int_draco_size_formula(nv):
    """The size the host wrapper and the device layout compute for an
    integer-position entry equals len(draco.encode(...)), in the four index
    bands and at their edges."""
    rng = np.random.default_rng(nv)
    nf = 37
    verts = rng.integers(0, 1024, size=(nv, 3)).astype(np.uint32)
    faces = rng.integers(0, nv, size=(nf, 3)).astype(np.uint32)
    faces[0] = (0, nv - 1, nv // 2)  # the widest varints of the band
    want = len(draco.encode(verts, faces))
    assert ref.int_draco_size(nv, nf, faces) == want
    v, f = draco.decode(draco.encode(verts, faces))[:2]
    assert np.array_equal(v, verts) and np.array_equal(f, faces)


def test_int_draco_size_of_empty_is_zero():
    assert ref.int_draco_size(0, 0) == 0
    assert ref.int_draco_size(5, 0) == 0
