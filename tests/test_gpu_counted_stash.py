"""MG_FLAG_COUNTED (the GPU part runs under pytest -m gpu): a chunk call that
meshes the raw volume the mg_count_voxels call just before it left resident.
Raw ctypes on private contexts. The flag's check has its own return code,
sits behind every older check, and every rejected call is rejected on the
host; the context works afterwards."""
import ctypes

import numpy as np
import pytest

import fill_holes_ref as R
from test_gpu_chunk_request import (A, B, C, _assert_is_oracle, _call, _err,
                                    _good, _holes, _oracle_tables, _tables,
                                    _volume)

COUNTED, SKIP_H2D = 4, 2
NOT_COUNTED = 9   # include/meshgine.h, MG_FLAG_COUNTED
B2 = 400


def test_constants_match_the_engine_module():
    from igneous_amd import engine as E
    assert (E.MG_FLAG_COUNTED, E.MG_FLAG_SKIP_H2D) == (COUNTED, SKIP_H2D)
    assert E.MG_ERR_NOT_COUNTED == NOT_COUNTED


@pytest.fixture
def eng():
    from igneous_amd.engine import Engine
    e = Engine(0)  # fresh: the stash is context state
    yield e
    e.lib.mg_destroy(e.ctx)
    e.ctx = None


def _count(eng, vol):
    from igneous_amd import engine as E
    dest = ctypes.POINTER(E._MgLabelCounts)()
    rc = eng.lib.mg_count_voxels(
        eng.ctx, vol.ctypes.data_as(ctypes.c_void_p), *vol.shape,
        E._mg_dtype(vol), 0, ctypes.byref(dest))
    assert rc == 0, _err(eng)
    n = int(dest.contents.n)
    labels = np.ctypeslib.as_array(dest.contents.labels, shape=(n,)).tolist()
    eng.lib.mg_label_counts_free(dest)
    return labels


def _map(keys, vals, miss):
    """(mg_label_map, the arrays it points into)."""
    from igneous_amd.engine import _MgLabelMap
    k = np.array(keys, dtype=np.uint64)
    v = np.array(vals, dtype=np.uint64)
    return _MgLabelMap(k.ctypes.data, v.ctypes.data, len(keys), miss), (k, v)


def _rejected(eng, name, vol, **kw):
    rc, _ = _call(eng, name, vol, **kw)
    assert rc == NOT_COUNTED, (rc, _err(eng))
    assert b"MG_FLAG_COUNTED" in _err(eng)


def _still_works(eng):
    vol = _volume()
    _assert_is_oracle(_good(eng, "mg_mesh_chunk", vol), _oracle_tables(vol))
    assert _err(eng) == b""


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.uint64, np.uint32],
                         ids=["uint64", "uint32"])
def test_counted_call_equals_the_ordinary_one(eng, dtype):
    vol = _volume(dtype)
    c = int(vol[1, 6, 6])
    cmap, _keep = _map([B, c], [B2, 0], 0)
    want = _good(eng, "mg_mesh_chunk_mapped", vol, cmap=cmap)
    assert want[0] == sorted([A, B2])
    assert _count(eng, vol) == sorted([0, A, B, c])
    # the host volume is not read: hand over one that would give no mesh
    blank = np.zeros_like(vol)
    got = _good(eng, "mg_mesh_chunk_mapped", blank, cmap=cmap, flags=COUNTED)
    assert got == want
    # without a map, through the narrowest entry point
    _count(eng, vol)
    plain = _good(eng, "mg_mesh_chunk", blank, flags=COUNTED)
    _assert_is_oracle(plain, _oracle_tables(vol))


@pytest.mark.gpu
def test_flag_without_a_stash(eng):
    vol = _volume()
    _rejected(eng, "mg_mesh_chunk_mapped", vol, flags=COUNTED)
    _still_works(eng)
    # the stash is the call's just before: one counted call consumes it
    _count(eng, vol)
    _good(eng, "mg_mesh_chunk", vol, flags=COUNTED)
    _rejected(eng, "mg_mesh_chunk", vol, flags=COUNTED)
    _still_works(eng)


@pytest.mark.gpu
def test_dims_and_dtype_must_match(eng):
    vol = _volume()
    _count(eng, vol)
    other = np.zeros((8, 8, 9), dtype=np.uint64, order="F")
    _rejected(eng, "mg_mesh_chunk", other, flags=COUNTED)
    _count(eng, vol)
    _rejected(eng, "mg_mesh_chunk", _volume(np.uint32), flags=COUNTED)
    # a rejected call has dropped the stash
    _rejected(eng, "mg_mesh_chunk", vol, flags=COUNTED)
    _still_works(eng)


@pytest.mark.gpu
def test_any_call_in_between_drops_the_stash(eng):
    import oracle
    vol = _volume()
    meshes = oracle.mesh_chunk(vol, resolution=(16.0, 16.0, 40.0))
    v, f = meshes[A]
    _count(eng, vol)
    sv, sf = eng.simplify_mesh(v, f, 2)
    assert 0 < sf.shape[0] <= f.shape[0]
    _rejected(eng, "mg_mesh_chunk", vol, flags=COUNTED)
    _count(eng, vol)
    _good(eng, "mg_mesh_chunk", vol)
    _rejected(eng, "mg_mesh_chunk", vol, flags=COUNTED)
    _count(eng, vol)
    eng.chunk_mesh(v, f, (64.0, 64.0, 64.0), (0.0, 0.0, 0.0))
    _rejected(eng, "mg_mesh_chunk", vol, flags=COUNTED)
    _count(eng, vol)
    eng.fill_holes(vol, 1)
    _rejected(eng, "mg_mesh_chunk", vol, flags=COUNTED)
    _still_works(eng)


@pytest.mark.gpu
def test_flag_with_skip_h2d(eng):
    vol = _volume()
    _count(eng, vol)
    _rejected(eng, "mg_mesh_chunk", vol, flags=COUNTED | SKIP_H2D)
    _still_works(eng)


@pytest.mark.gpu
def test_the_new_check_comes_after_the_old_ones(eng):
    """No stash, and an older check trips too: the older check's code."""
    from igneous_amd.engine import _MgLabelMap
    vol = _volume()
    for kw, code in ((dict(dtype=5), 3), (dict(dims=(0, 8, 8)), 2),
                     (dict(labels=False), 1),
                     (dict(cmap=_MgLabelMap(None, None, 0, 9)), 5),
                     (dict(fill_level=3), 6)):
        rc, _ = _call(eng, "mg_mesh_chunk_filled", vol, flags=COUNTED, **kw)
        assert rc == code, (kw, rc, _err(eng))
    # map + SKIP_H2D keeps its own code with the flag set as well
    cmap, _keep = _map([B], [B2], 0)
    _count(eng, vol)
    rc, _ = _call(eng, "mg_mesh_chunk_mapped", vol, cmap=cmap,
                  flags=COUNTED | SKIP_H2D)
    assert rc == 5
    _still_works(eng)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.uint64, np.uint32],
                         ids=["uint64", "uint32"])
def test_flag_with_a_label_map_and_a_fill(eng, dtype):
    """Unlike MG_FLAG_SKIP_H2D the flag may come with a map and a fill: the
    resident volume is known to be raw."""
    vol = _volume(dtype)
    c = int(vol[1, 6, 6])
    mapped = vol.copy()
    mapped[vol == c] = 0
    mapped[vol == B] = B2
    want_f, want_h, rounds = R.fill_holes_ref(mapped, 1)
    assert rounds == 1 and np.count_nonzero(want_f != mapped) == 1
    cmap, _keep = _map([B, c], [B2, 0], 0)
    _count(eng, vol)
    got = _good(eng, "mg_mesh_chunk_filled", vol, cmap=cmap, fill_level=1,
                flags=COUNTED)
    _assert_is_oracle(got, _oracle_tables(want_f))
    assert got[0] == sorted([A, B2])
    rc, dest = _holes(eng)
    assert rc == 0, _err(eng)
    _assert_is_oracle(_tables(eng, dest), _oracle_tables(want_h))
