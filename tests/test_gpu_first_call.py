"""First call on a fresh context (the GPU part runs under pytest -m gpu):
each entry point that reads a device scalar of the context — the
simplifier's totals, the label map's error word, the weld's vertex total —
or allocates its buffers on demand is made as the ONLY call of a private
Engine, so nothing an earlier call allocated or cleared can stand in for
what mg_init and the call itself must provide. Every result is bit-exact
against its CPU checker; the inputs' properties are checked on the CPU
without a GPU."""
import functools

import numpy as np
import pytest

from test_gpu_ctx_lifecycle import (B, B2, C, C2, LABEL_MAP, RES,
                                    _assert_meshsets_equal, _destroy,
                                    _volume)

CHUNK_SCALE = (64.0, 64.0, 64.0)
CHUNK_OFFSET = (0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def _big_mesh():
    """(verts, faces) of the volume's largest label, from the oracle."""
    import oracle
    meshes = oracle.mesh_chunk(_volume(), resolution=RES)
    big = max(meshes, key=lambda lab: meshes[lab][1].shape[0])
    return meshes[big]


def _mapped_volume():
    """_volume() with LABEL_MAP ('keep' policy) applied on the host."""
    vol = _volume()
    out = vol.copy()
    for k, v in zip(LABEL_MAP[0], LABEL_MAP[1]):
        out[vol == k] = v
    return out


def _host_chunks():
    from igneous_amd import meshops
    from igneous_amd.meshes import Mesh
    v, f = _big_mesh()
    return meshops.chunk_mesh(Mesh(v, f, id=1), CHUNK_SCALE, CHUNK_OFFSET)


def _first_call(fn):
    """fn(eng) as the one and only call of a private context."""
    from igneous_amd.engine import Engine
    eng = Engine(0)
    try:
        return fn(eng)
    finally:
        _destroy(eng)


def test_inputs_are_not_trivial():
    import oracle
    from fill_holes_ref import fill_holes_ref
    v, f = _big_mesh()
    _, sf = oracle.simplify_mesh(v, f, 2)
    assert 0 < sf.shape[0] < f.shape[0]
    # at least two cells, and clipping made faces
    chunks = _host_chunks()
    assert len(chunks) >= 2
    assert sum(m.faces.shape[0] for m in chunks.values()) > f.shape[0]
    vol = _volume()
    filled, _, _ = fill_holes_ref(vol, 1)
    assert np.count_nonzero(filled != vol) > 0
    # the map renames labels that get meshes
    raw = oracle.mesh_chunk(vol, resolution=RES)
    mapped = oracle.mesh_chunk(_mapped_volume(), resolution=RES)
    assert B in raw and C in raw and B2 not in raw and C2 not in raw
    assert B2 in mapped and C2 in mapped and B not in mapped
    full = sum(m[1].shape[0] for m in raw.values())
    simp = oracle.mesh_chunk(vol, resolution=RES, reduction_factor=2)
    assert sum(m[1].shape[0] for m in simp.values()) < full


@pytest.mark.gpu
def test_first_call_simplify_mesh():
    import oracle
    v, f = _big_mesh()
    gv, gf = _first_call(lambda eng: eng.simplify_mesh(v, f, 2))
    wv, wf = oracle.simplify_mesh(v, f, 2)
    assert gf.shape == wf.shape and np.array_equal(gf, wf)
    assert gv.shape == wv.shape and np.array_equal(gv, wv)


@pytest.mark.gpu
def test_first_call_chunk_mesh():
    from test_gpu_chunk_mesh import _assert_same
    v, f = _big_mesh()
    got = _first_call(
        lambda eng: eng.chunk_mesh(v, f, CHUNK_SCALE, CHUNK_OFFSET))
    _assert_same(got, _host_chunks(), "first call")


@pytest.mark.gpu
def test_first_call_fill_holes():
    from fill_holes_ref import fill_holes_ref
    vol = _volume()
    filled, holes, rounds = _first_call(
        lambda eng: eng.fill_holes(vol, level=1))
    wf, wh, wr = fill_holes_ref(vol, 1)
    assert np.array_equal(filled, wf) and np.array_equal(holes, wh)
    assert rounds == wr


@pytest.mark.gpu
def test_first_call_label_map_without_dust():
    import oracle
    got = _first_call(lambda eng: eng.mesh_chunk(
        _volume(), resolution=RES, label_map=LABEL_MAP))
    _assert_meshsets_equal(
        got, oracle.mesh_chunk(_mapped_volume(), resolution=RES),
        "first call, label map")


@pytest.mark.gpu
def test_first_call_mesh_chunk_simplified():
    import oracle
    got = _first_call(lambda eng: eng.mesh_chunk(
        _volume(), resolution=RES, reduction_factor=2))
    _assert_meshsets_equal(
        got, oracle.mesh_chunk(_volume(), resolution=RES, reduction_factor=2),
        "first call, reduction_factor=2")
