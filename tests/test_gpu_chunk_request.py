"""The four mg_mesh_chunk* entry points and mg_mesh_holes as one request
path (the GPU part runs under pytest -m gpu): the entry points agree with
each other and with the CPU oracle, the argument checks keep their order and
their return codes, and the two empty returns leave in mg_stats exactly what
they measured. Raw ctypes on a private context; every rejected call is
rejected on the host, before the device is touched.

An 8^3 volume with a zero border has a 6^3 interior, where a 5^3 block and
a disjoint 2^3 block do not both fit: B takes the corner voxel of A.

The dense label ids come from an atomic counter, so the ORDER of the labels
inside the flat vertex / face arrays is not a property of an entry point.
voff / foff are therefore checked to tile the flat arrays, and the vertex
and face bytes are compared label by label through them; labels_arr, nv and
nf are compared as they come."""
import ctypes

import numpy as np
import pytest

import fill_holes_ref as R

RES = (16.0, 16.0, 40.0)
A, B, C = 7, 300, 5_000_000_000   # C needs 64 bits; the u32 volume folds it
DTYPES = [np.uint64, np.uint32]
_ids = lambda d: np.dtype(d).name  # noqa: E731


def _volume(dtype=np.uint64):
    v = np.zeros((8, 8, 8), dtype=dtype, order="F")
    v[1:6, 1:6, 1:6] = A
    v[3, 3, 3] = 0                 # the smallest hole level 1 fills
    v[5:7, 5:7, 5:7] = B
    v[1, 6, 6] = C if dtype == np.uint64 else C & 0xFFFFFFFF
    return v


def _uniform():
    return np.full((4, 4, 4), A, dtype=np.uint64, order="F")


def _oracle_tables(vol, **kw):
    """{label: (nv, nf, vertex bytes, face bytes)} from the CPU oracle."""
    import oracle
    return {int(lab): (v.shape[0], f.shape[0], v.tobytes(), f.tobytes())
            for lab, (v, f) in oracle.mesh_chunk(vol, resolution=RES,
                                                 **kw).items()}


def test_inputs_are_not_trivial():
    for dtype in DTYPES:
        vol = _volume(dtype)
        assert not vol[0].any() and not vol[-1].any()
        assert not vol[:, 0].any() and not vol[:, -1].any()
        assert not vol[:, :, 0].any() and not vol[:, :, -1].any()
        c = int(vol[1, 6, 6])
        assert np.count_nonzero(vol == A) == 125 - 2
        assert np.count_nonzero(vol == B) == 8
        assert np.count_nonzero(vol == c) == 1
        want = _oracle_tables(vol)
        assert sorted(want) == sorted([A, B, c])
        assert all(nv > 0 and nf > 0 for nv, nf, _, _ in want.values())
        filled, holes, rounds = R.fill_holes_ref(vol, 1)
        assert rounds == 1 and filled[3, 3, 3] == A
        assert np.count_nonzero(filled != vol) == 1
        assert not holes.any()     # the cavity held label 0: no hole mesh
        assert _oracle_tables(filled) != want
    simp = _oracle_tables(_volume(), reduction_factor=2)
    assert sum(t[1] for t in simp.values()) < \
        sum(t[1] for t in _oracle_tables(_volume()).values())
    assert _oracle_tables(_uniform()) == {}


# ---------------------------------------------------------------------------
# raw calls

@pytest.fixture(scope="module")
def eng():
    from igneous_amd.engine import Engine
    e = Engine(0)  # private: no other test's call has run on this ctx
    yield e
    e.lib.mg_destroy(e.ctx)
    e.ctx = None


def _call(eng, name, vol, *, ctx=True, labels=True, dims=None, dtype=None,
          red=0, flags=0, cmap=None, fill_level=0, params=None, out=True):
    """One mg_mesh_chunk* call through ctypes -> (rc, destination)."""
    from igneous_amd import engine as E
    encoded = name == "mg_mesh_chunk_encoded"
    dest = ctypes.POINTER(E._MgBlobSet if encoded else E._MgMeshSet)()
    common = [eng.ctx if ctx else None,
              vol.ctypes.data_as(ctypes.c_void_p) if labels else None,
              *(dims or vol.shape),
              E._mg_dtype(vol) if dtype is None else dtype,
              *RES, red, 40.0, 1, 0, flags]
    cmap = ctypes.byref(cmap) if cmap is not None else None
    tail = {"mg_mesh_chunk": [],
            "mg_mesh_chunk_mapped": [cmap],
            "mg_mesh_chunk_filled": [cmap, fill_level],
            "mg_mesh_chunk_encoded": [
                cmap, ctypes.byref(params) if params is not None else None],
            }[name]
    rc = getattr(eng.lib, name)(*common, *tail,
                                ctypes.byref(dest) if out else None)
    return rc, dest


def _holes(eng, red=0):
    from igneous_amd.engine import _MgMeshSet
    dest = ctypes.POINTER(_MgMeshSet)()
    rc = eng.lib.mg_mesh_holes(eng.ctx, *RES, red, 40.0, 1, 0,
                               ctypes.byref(dest))
    return rc, dest


def _err(eng, ctx=True):
    return eng.lib.mg_last_error(eng.ctx if ctx else None) or b""


def _tables(eng, dest):
    """The meshset as (labels_arr, nv, nf, {label: (nv, nf, vertex bytes,
    face bytes)}); voff / foff must tile the flat arrays. Frees it."""
    try:
        ms = dest.contents
        n = int(ms.nmeshes)
        cols = [np.ctypeslib.as_array(p, shape=(n,)).tolist() if n else []
                for p in (ms.labels_arr, ms.voff_arr, ms.nv_arr,
                          ms.foff_arr, ms.nf_arr)]
        labels, voff, nv, foff, nf = cols
        for off, cnt, total in ((voff, nv, int(ms.total_verts)),
                                (foff, nf, int(ms.total_tris))):
            at = 0
            for o, k in sorted(zip(off, cnt)):
                assert o == at, "offsets do not tile the flat array"
                at += k
            assert at == (total if n else 0)
        by_label = {}
        for m in range(n):
            mesh = ms.meshes[m]
            assert (mesh.label, mesh.nverts, mesh.ntris) == \
                (labels[m], nv[m], nf[m])
            vb = ctypes.string_at(
                ctypes.addressof(ms.verts_base.contents) + 12 * voff[m],
                12 * nv[m])
            fb = ctypes.string_at(
                ctypes.addressof(ms.faces_base.contents) + 12 * foff[m],
                12 * nf[m])
            assert ctypes.string_at(mesh.verts, 12 * nv[m]) == vb
            assert ctypes.string_at(mesh.faces, 12 * nf[m]) == fb
            by_label[labels[m]] = (nv[m], nf[m], vb, fb)
        return labels, nv, nf, by_label
    finally:
        eng.lib.mg_meshset_free(dest)


def _good(eng, name, vol, **kw):
    rc, dest = _call(eng, name, vol, **kw)
    assert rc == 0, _err(eng)
    return _tables(eng, dest)


def _assert_is_oracle(got, want):
    labels, nv, nf, by_label = got
    assert labels == sorted(want)
    assert nv == [want[lab][0] for lab in labels]
    assert nf == [want[lab][1] for lab in labels]
    assert by_label == want


# ---------------------------------------------------------------------------
# equivalence of the entry points

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_entry_points_agree(eng, dtype):
    vol = _volume(dtype)
    want = _oracle_tables(vol)
    plain = _good(eng, "mg_mesh_chunk", vol)
    mapped = _good(eng, "mg_mesh_chunk_mapped", vol, cmap=None)
    filled = _good(eng, "mg_mesh_chunk_filled", vol, cmap=None, fill_level=0)
    assert plain == mapped == filled
    _assert_is_oracle(plain, want)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_filled_then_holes_equal_the_oracle(eng, dtype):
    vol = _volume(dtype)
    want_f, want_h, _ = R.fill_holes_ref(vol, 1)
    got_f = _good(eng, "mg_mesh_chunk_filled", vol, fill_level=1)
    rc, dest = _holes(eng)
    assert rc == 0, _err(eng)
    got_h = _tables(eng, dest)
    _assert_is_oracle(got_f, _oracle_tables(want_f))
    _assert_is_oracle(got_h, _oracle_tables(want_h))
    assert got_h[0] == []


# ---------------------------------------------------------------------------
# check order and codes

def _bad_map(miss=9):
    from igneous_amd.engine import _MgLabelMap
    return _MgLabelMap(None, None, 0, miss)


def _enc_params(fmt=0):
    from igneous_amd.engine import _MgEncodeParams
    p = _MgEncodeParams()
    p.format = fmt
    return p


# (what, entry point, arguments of _call, the code of the check it trips)
REJECTED = [
    ("null ctx", "mg_mesh_chunk", dict(ctx=False), 1),
    ("fill_level 3", "mg_mesh_chunk_filled", dict(fill_level=3), 6),
    ("fill + SKIP_H2D", "mg_mesh_chunk_filled",
     dict(fill_level=1, flags=2), 6),
    ("null labels", "mg_mesh_chunk", dict(labels=False), 1),
    ("null meshset", "mg_mesh_chunk_mapped", dict(out=False), 1),
    ("null blobset", "mg_mesh_chunk_encoded",
     dict(params=_enc_params, out=False), 1),
    ("null encode params", "mg_mesh_chunk_encoded", dict(params=None), 8),
    ("unknown format", "mg_mesh_chunk_encoded",
     dict(params=lambda: _enc_params(7)), 8),
    ("sx = 0", "mg_mesh_chunk", dict(dims=(0, 8, 8)), 2),
    ("sz = 2048", "mg_mesh_chunk_filled", dict(dims=(8, 8, 2048)), 2),
    ("bad dtype", "mg_mesh_chunk", dict(dtype=5), 3),
    ("bad miss policy", "mg_mesh_chunk_mapped", dict(cmap=_bad_map), 5),
    ("map + SKIP_H2D", "mg_mesh_chunk_filled",
     dict(cmap=lambda: _bad_map(0), flags=2), 5),
    # two checks tripped: the earlier one's code
    ("fill_level 3, null labels", "mg_mesh_chunk_filled",
     dict(fill_level=3, labels=False), 6),
    ("null labels, sx = 0", "mg_mesh_chunk",
     dict(labels=False, dims=(0, 8, 8)), 1),
    ("bad dtype, bad miss policy", "mg_mesh_chunk_mapped",
     dict(dtype=5, cmap=_bad_map), 3),
]


@pytest.mark.gpu
def test_checks_keep_their_order_and_codes(eng):
    vol = _volume()
    for what, name, kw, code in REJECTED:
        kw = {k: v() if callable(v) else v for k, v in kw.items()}
        rc, _ = _call(eng, name, vol, **kw)
        print(f"{what}: rc={rc} {_err(eng, kw.get('ctx', True))!r}")
        assert rc == code, what
        assert len(_err(eng, kw.get('ctx', True))) > 0, what
    # the context is as good as before
    _assert_is_oracle(_good(eng, "mg_mesh_chunk", vol), _oracle_tables(vol))
    assert _err(eng) == b""


@pytest.mark.gpu
def test_hole_stash_is_dropped_between_encode_and_volume_checks(eng):
    """holes_valid = false sits after check_encode_params and before
    check_volume_args: a call rejected earlier leaves the stash of the call
    before it, a call rejected later has dropped it."""
    vol = _volume()
    _good(eng, "mg_mesh_chunk_filled", vol, fill_level=1)
    rc, _ = _call(eng, "mg_mesh_chunk_encoded", vol, params=None)
    assert rc == 8
    rc, dest = _holes(eng)
    assert rc == 0, _err(eng)
    eng.lib.mg_meshset_free(dest)
    _good(eng, "mg_mesh_chunk_filled", vol, fill_level=1)
    rc, _ = _call(eng, "mg_mesh_chunk", vol, dtype=5)
    assert rc == 3
    rc, _ = _holes(eng)
    assert rc == 7 and b"hole volume" in _err(eng)


# ---------------------------------------------------------------------------
# stats on the empty paths

MS_FIELDS = ["ms_h2d", "ms_count", "ms_scan", "ms_emit", "ms_partition",
             "ms_weld", "ms_simplify", "ms_d2h", "ms_total", "ms_labelmap",
             "ms_fill", "ms_encode"]


def _assert_empty_stats(eng, vol, measured=()):
    """mg_stats after an empty return: the fields in `measured` were taken
    from this call's events, every other ms_* field is exactly 0.0."""
    st = eng.stats()
    print(st)
    assert st["bytes_read_algorithmic"] == vol.size * vol.itemsize
    assert st["total_tris"] == 0 and st["total_verts"] == 0
    for name in MS_FIELDS:
        if name in measured:
            assert st[name] >= 0, name
        else:
            assert st[name] == 0.0 and isinstance(st[name], float), name


def _busy(eng):
    """A non-empty simplified call, then a non-empty encoded one: every
    event of the context now holds a time that is not this call's."""
    vol = _volume()
    labels, _, nf, _ = _good(eng, "mg_mesh_chunk", vol, red=2)
    assert labels == sorted([A, B, C]) and sum(nf) > 0
    st = eng.stats()
    assert st["ms_total"] > 0 and st["ms_simplify"] > 0 and st["ms_d2h"] > 0
    rc, dest = _call(eng, "mg_mesh_chunk_encoded", vol, params=_enc_params())
    assert rc == 0, _err(eng)
    assert dest.contents.n == 3
    eng.lib.mg_blobset_free(dest)
    assert eng.stats()["ms_encode"] > 0


@pytest.mark.gpu
def test_stats_on_the_empty_paths(eng):
    _busy(eng)
    # (a) no cells: nothing is queued, nothing is measured
    flat = np.full((1, 5, 5), A, dtype=np.uint64, order="F")
    assert _good(eng, "mg_mesh_chunk", flat)[0] == []
    _assert_empty_stats(eng, flat)
    # (b) cells, no triangles
    _busy(eng)
    vol = _uniform()
    assert _good(eng, "mg_mesh_chunk", vol)[0] == []
    _assert_empty_stats(eng, vol, ("ms_h2d",))
    # (c) the same through the fill and the hole meshing
    _busy(eng)
    assert _good(eng, "mg_mesh_chunk_filled", vol, fill_level=1)[0] == []
    _assert_empty_stats(eng, vol, ("ms_h2d", "ms_fill"))
    rc, dest = _holes(eng)
    assert rc == 0, _err(eng)
    assert _tables(eng, dest)[0] == []
    _assert_empty_stats(eng, vol, ("ms_h2d",))
    # (d) the same through the encoded call
    _busy(eng)
    rc, dest = _call(eng, "mg_mesh_chunk_encoded", vol, params=_enc_params())
    assert rc == 0, _err(eng)
    assert dest.contents.n == 0 and dest.contents.blob_bytes == 0
    eng.lib.mg_blobset_free(dest)
    _assert_empty_stats(eng, vol, ("ms_h2d",))
