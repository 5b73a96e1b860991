"""Host-side tests for the device grid chunker's plumbing (no GPU): the
multires `set_chunker` seam's selection rule and the mg_chunk_mesh ABI
entry."""
import ctypes
import os
import re

import numpy as np
import pytest

from igneous_amd import engine, meshops
from igneous_amd.meshes import Mesh
from igneous_amd.tasks import multires as multires_mod

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "igneous_amd", "csrc", "libmeshgine.so")
HDR = os.path.join(REPO, "include", "meshgine.h")


def _two_cell_mesh():
    v = np.array([[.2, .2, .2], [1.7, .3, .1], [.3, .6, .2]],
                 dtype=np.float32)
    f = np.array([[0, 1, 2]], dtype=np.uint32)
    return Mesh(v, f, id=3)


@pytest.fixture
def counting_host_chunker(monkeypatch):
    calls = []
    real = meshops.chunk_mesh

    def counted(mesh, scale, offset):
        calls.append((tuple(scale), tuple(offset)))
        return real(mesh, scale, offset)

    monkeypatch.setattr(meshops, "chunk_mesh", counted)
    yield calls
    multires_mod.set_chunker(None)
    multires_mod.set_simplifier(None)


def _call_both_sites(mesh):
    """retriangulate_mesh and create_octree_level_from_mesh (lod 0 of 2:
    one chunk_mesh call, no retriangulation)."""
    multires_mod.retriangulate_mesh(mesh, (0, 0, 0), (1, 1, 1))
    multires_mod.create_octree_level_from_mesh(
        mesh, (1, 1, 1), 0, 2, (0, 0, 0), (2, 1, 1))


def test_injected_simplifier_keeps_host_chunker(counting_host_chunker):
    multires_mod.set_simplifier(lambda mesh, target: mesh)
    _call_both_sites(_two_cell_mesh())
    assert len(counting_host_chunker) == 2


def test_injected_chunker_wins(counting_host_chunker):
    mine = []

    def fn(mesh, scale, offset):
        mine.append(1)
        return {(0, 0, 0): mesh}

    multires_mod.set_simplifier(lambda mesh, target: mesh)
    multires_mod.set_chunker(fn)
    _call_both_sites(_two_cell_mesh())
    assert len(mine) == 2
    assert counting_host_chunker == []


def test_set_chunker_none_restores_default(counting_host_chunker):
    multires_mod.set_chunker(lambda mesh, scale, offset: {})
    multires_mod.set_chunker(None)
    # product path: the engine's chunker, never the host function
    assert multires_mod._get_chunker() is engine.chunk_mesh
    multires_mod.set_simplifier(lambda mesh, target: mesh)
    assert multires_mod._get_chunker() is meshops.chunk_mesh
    _call_both_sites(_two_cell_mesh())
    assert len(counting_host_chunker) == 2


def test_symbol_declared_and_listed():
    with open(HDR) as f:
        text = f.read()
    assert re.search(r"\bint\s+mg_chunk_mesh\s*\(", text)
    assert "mg_chunk_mesh" in engine._EXPORTED_SYMBOLS


def test_symbol_exported_when_built():
    if not os.path.exists(SO):
        pytest.skip("libmeshgine.so not built")
    assert hasattr(ctypes.CDLL(SO), "mg_chunk_mesh")
