"""GPU tests (pytest -m gpu) of fill_holes levels 1-2: mg_fill_holes,
mg_mesh_chunk_filled and mg_mesh_holes against the numpy/scipy checker in
tests/fill_holes_ref.py. Every volume comparison is equality of every voxel
of BOTH output volumes (filled and holes); meshes are bit-exact against the
CPU oracle run on the checker's volumes."""
import ctypes

import numpy as np
import pytest

import fill_holes_ref as R

pytestmark = pytest.mark.gpu

RES = (16.0, 16.0, 40.0)
DTYPES = [np.uint32, np.uint64]
_ids = lambda d: np.dtype(d).name  # noqa: E731


@pytest.fixture(scope="module")
def eng():
    from igneous_amd.engine import Engine
    return Engine.get(0)


_REF = {}


def ref(key, vol, level):
    """checker result, computed once per (volume key, level)."""
    k = (key, level)
    if k not in _REF:
        _REF[k] = R.fill_holes_ref(vol, level)
    return _REF[k]


def check(eng, key, vol, level):
    raw = vol.copy()
    want_f, want_h, want_r = ref(key, vol, level)
    got_f, got_h, got_r = eng.fill_holes(vol, level)
    assert np.array_equal(vol, raw), "host labels were modified"
    assert got_f.dtype == vol.dtype and got_h.dtype == vol.dtype
    bad = np.count_nonzero(got_f != want_f)
    assert bad == 0, f"{key} level {level}: {bad} filled voxels differ"
    bad = np.count_nonzero(got_h != want_h)
    assert bad == 0, f"{key} level {level}: {bad} hole voxels differ"
    assert got_r == want_r, f"{key} level {level}: rounds {got_r} != {want_r}"
    return got_f, got_h, got_r


def _assert_meshsets_equal(got: dict, want: dict, what=""):
    assert sorted(got.keys()) == sorted(want.keys()), \
        f"{what}: label sets differ ({sorted(got)} vs {sorted(want)})"
    for label in want:
        gv, gf = got[label]
        wv, wf = want[label]
        assert gv.shape == wv.shape and gf.shape == wf.shape, \
            f"{what} label {label}: sizes differ"
        assert np.array_equal(gf, wf), f"{what} label {label}: faces differ"
        assert np.array_equal(gv, wv), f"{what} label {label}: verts differ"


# ---------------------------------------------------------------------------
# closed-form cases of the contract

CLOSED = {
    "nested": lambda d: R.case_nested(d),
    "nested_piece": lambda d: R.case_nested(d, inner='A'),
    "two_adjacent": R.case_two_adjacent,
    "island": R.case_island,
    "open_cavity": R.case_open_cavity,
    "edge_diagonal": R.case_edge_diagonal,
    "three_deep": R.case_three_deep,
}


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", list(CLOSED))
def test_closed_form(eng, name, dtype):
    v = CLOSED[name](dtype)
    A, B = R.lift(1, dtype), R.lift(2, dtype)
    f1, h1, r1 = check(eng, (name, _ids(dtype)), v, 1)
    f2, h2, r2 = check(eng, (name, _ids(dtype)), v, 2)
    if name in ("nested", "nested_piece"):
        assert r1 == 2
        assert np.count_nonzero(f1) == 14 ** 3 and np.all(f1[f1 != 0] == A)
        assert np.count_nonzero(h1) == 504
        assert np.array_equal(h1 != 0, v == B) and np.all(h1[h1 != 0] == B)
    elif name in ("two_adjacent", "island"):
        assert r1 == 0 and np.array_equal(f1, v) and not h1.any()
        assert np.array_equal(f2, v)
    elif name == "open_cavity":
        assert np.array_equal(f1, v) and r1 == 0
        assert np.all(f2 == A) and np.count_nonzero(f2 != v) == 96
        assert not h2.any()
    elif name == "edge_diagonal":
        assert f1[3, 3, 8] == A and np.count_nonzero(f1 != v) == 1
    elif name == "three_deep":
        assert r1 == 3
        assert np.all(f1[1:19, 1:19, 1:19] == A)
        assert np.count_nonzero(h1 == B) == 12 ** 3 - 6 ** 3


# ---------------------------------------------------------------------------
# shapes that break indexing

def _shape_volume(shape, dtype, seed):
    """{0, a, b} noise with a zeroed border on every axis that has one;
    3x3x3 is one background voxel inside a solid block."""
    if shape == (3, 3, 3):
        v = np.full(shape, R.lift(1, dtype), dtype=dtype, order="F")
        v[1, 1, 1] = 0
        return v
    rng = np.random.default_rng(seed)
    vals = np.array([0, R.lift(1, dtype), R.lift(2, dtype)], dtype=dtype)
    v = np.asfortranarray(
        vals[rng.choice(3, size=shape, p=(0.1, 0.8, 0.1))])
    for ax, size in enumerate(shape):
        if size > 1:
            idx = [slice(None)] * 3
            for pos in (0, size - 1):
                idx[ax] = pos
                v[tuple(idx)] = 0
    return v


SHAPES = [(3, 3, 3), (33, 17, 9), (65, 31, 20), (40, 40, 1), (1, 1, 50)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes(eng, shape, dtype):
    v = _shape_volume(shape, dtype, 11)
    for level in (1, 2):
        f, h, r = check(eng, ("shape", shape, _ids(dtype)), v, level)
    # none of these passes vacuously: the checker fills something
    want_f, _, _ = ref(("shape", shape, _ids(dtype)), v, 1)
    assert np.count_nonzero(want_f != v) > 0
    if shape == (3, 3, 3):
        assert np.all(f == R.lift(1, dtype))


# ---------------------------------------------------------------------------
# components that span many workgroups

NOISE = [(i, seed) for i in range(len(R.NOISE_CASES)) for seed in range(3)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("case,seed", NOISE)
def test_noise(eng, case, seed, dtype):
    shape, probs = R.NOISE_CASES[case]
    v = R.case_noise(dtype, shape, probs, seed)
    key = ("noise", case, seed, _ids(dtype))
    want_f, want_h, _ = ref(key, v, 1)
    rewritten = np.count_nonzero(want_f != v)
    nholes = np.count_nonzero(want_h)
    print(f"noise {shape} seed {seed}: checker rewrites {rewritten}, "
          f"{nholes} non-zero hole voxels")
    assert rewritten > 1000 and nholes > 0, "checker comparison is vacuous"
    check(eng, key, v, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("case,seed", NOISE)
def test_noise_open_border_level2(eng, case, seed, dtype):
    shape, probs = R.NOISE_CASES[case]
    v = R.case_noise(dtype, shape, probs, seed, copy_border=True)
    key = ("noise_open", case, seed, _ids(dtype))
    f1, _, _ = ref(key, v, 1)
    f2, _, _ = ref(key, v, 2)
    differ = np.count_nonzero(f1 != f2)
    print(f"open noise {shape} seed {seed}: level 1 vs 2 differ in {differ}")
    assert differ > 0, "level 2 must differ from level 1 here"
    check(eng, key, v, 1)
    check(eng, key, v, 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_serpentine_fills_in_one_round(eng, dtype):
    v = R.case_serpentine(dtype)
    f, h, r = check(eng, ("serpentine", _ids(dtype)), v, 1)
    assert r == 1 and np.all(f == R.lift(1, dtype)) and not h.any()


def test_deterministic(eng):
    shape, probs = R.NOISE_CASES[0]
    v = R.case_noise(np.uint64, shape, probs, 0)
    a = eng.fill_holes(v, 1)
    b = eng.fill_holes(v, 1)
    assert a[0].tobytes() == b[0].tobytes()
    assert a[1].tobytes() == b[1].tobytes()
    assert a[2] == b[2]


# ---------------------------------------------------------------------------
# meshing entry points

def _raw_filled(eng, data, fill_level, flags=0, cmap=None):
    """mg_mesh_chunk_filled through ctypes, no wrapper logic."""
    from igneous_amd.engine import _MgMeshSet, MG_U32, MG_U64
    out = ctypes.POINTER(_MgMeshSet)()
    rc = eng.lib.mg_mesh_chunk_filled(
        eng.ctx, data.ctypes.data_as(ctypes.c_void_p), *data.shape,
        MG_U64 if data.dtype == np.uint64 else MG_U32,
        *RES, 0, 40.0, 1, 0, flags,
        ctypes.byref(cmap) if cmap is not None else None,
        fill_level, ctypes.byref(out))
    return rc, out


def _raw_holes(eng):
    from igneous_amd.engine import _MgMeshSet
    out = ctypes.POINTER(_MgMeshSet)()
    rc = eng.lib.mg_mesh_holes(eng.ctx, *RES, 0, 40.0, 1, 0,
                               ctypes.byref(out))
    return rc, out


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_pipeline_order_dust_map_fill(eng, dtype):
    """dust (raw labels) -> label map -> fill -> mesh, all in one call."""
    import oracle
    from igneous_amd import remap as RM
    A, B, C, D, E = (R.lift(k, dtype) for k in (1, 2, 3, 4, 5))
    v = np.zeros((24, 22, 20), dtype=dtype, order="F")
    v[1:23, 1:21, 1:19] = A
    v[4:12, 4:12, 4:12] = B
    v[7:9, 7:9, 7:9] = 0
    v[15:17, 15, 10] = C          # 2 voxels: dust -> a cavity in A -> filled
    v[14:20, 4:10, 4:10] = D      # erased by the map -> cavity -> filled
    thr = 5
    lm = (np.array([B, D], dtype=np.uint64),
          np.array([E, 0], dtype=np.uint64), 'keep')

    ids, counts = np.unique(v, return_counts=True)
    small = [int(i) for i, ct in zip(ids, counts) if ct < thr and i != 0]
    assert small == [C]
    host = RM.mask(v.copy(), small)
    host = RM.remap(host, {B: E, D: 0})
    want_f, want_h, _ = R.fill_holes_ref(np.asfortranarray(host), 1)
    assert set(np.unique(want_f).tolist()) == {0, A}
    assert set(np.unique(want_h).tolist()) == {0, E}

    got_f, got_h = eng.mesh_chunk(v, resolution=RES, dust_threshold=thr,
                                  label_map=lm, fill_holes=1)
    st = eng.last_fill_stats
    assert st['ms_fill'] > 0 and st['ms_total'] >= st['ms_fill']
    _assert_meshsets_equal(got_f, oracle.mesh_chunk(want_f, resolution=RES),
                           "filled")
    _assert_meshsets_equal(got_h, oracle.mesh_chunk(want_h, resolution=RES),
                           "holes")
    assert sorted(got_f) == [A] and sorted(got_h) == [E]
    # plain meshing afterwards: ms_fill is 0 without fill
    eng.mesh_chunk(v, resolution=RES)
    assert eng.stats()['ms_fill'] == 0


def test_fill_level_zero_equals_mapped(eng):
    from igneous_amd.engine import _MgLabelMap, MG_MAP_MISS_ZERO
    v = R.case_noise(np.uint64, (33, 17, 9), (0.2, 0.5, 0.3), 5)
    a, b = R.lift(1, np.uint64), R.lift(2, np.uint64)
    rc, out = _raw_filled(eng, v, 0)
    assert rc == 0, eng.lib.mg_last_error(eng.ctx)
    _assert_meshsets_equal(eng._collect(out, True),
                           eng.mesh_chunk(v, resolution=RES), "no map")
    keys = np.array([a], dtype=np.uint64)
    vals = np.array([b + 1], dtype=np.uint64)
    cmap = _MgLabelMap(keys.ctypes.data, vals.ctypes.data, 1,
                       MG_MAP_MISS_ZERO)
    rc, out = _raw_filled(eng, v, 0, cmap=cmap)
    assert rc == 0, eng.lib.mg_last_error(eng.ctx)
    _assert_meshsets_equal(
        eng._collect(out, True),
        eng.mesh_chunk(v, resolution=RES, label_map=(keys, vals, 'zero')),
        "map")
    # level 0 leaves no hole volume behind
    rc, _ = _raw_holes(eng)
    assert rc != 0


def test_mesh_holes_needs_a_stash():
    from igneous_amd.engine import Engine
    fresh = Engine(0)  # its own ctx: nothing has run on it
    try:
        rc, _ = _raw_holes(fresh)
        assert rc != 0
        assert b"hole volume" in fresh.lib.mg_last_error(fresh.ctx)
        v = R.case_nested(np.uint32)
        rc, out = _raw_filled(fresh, v, 1)
        assert rc == 0, fresh.lib.mg_last_error(fresh.ctx)
        filled = fresh._collect(out, True)
        rc, out = _raw_holes(fresh)
        assert rc == 0, fresh.lib.mg_last_error(fresh.ctx)
        holes = fresh._collect(out, True)
        assert sorted(filled) == [1] and sorted(holes) == [2]
        rc, _ = _raw_holes(fresh)  # the stash was consumed
        assert rc != 0
        assert len(fresh.lib.mg_last_error(fresh.ctx)) > 0
    finally:
        fresh.lib.mg_destroy(fresh.ctx)
        fresh.ctx = None


def test_errors_are_return_codes(eng):
    import oracle
    from igneous_amd.engine import MG_FLAG_SKIP_H2D, MG_U32
    v = R.case_nested(np.uint32)
    f = np.empty_like(v)
    h = np.empty_like(v)
    for level in (0, 3, 104):
        rc = eng.lib.mg_fill_holes(
            eng.ctx, v.ctypes.data_as(ctypes.c_void_p), 16, 16, 16, MG_U32,
            level, f.ctypes.data_as(ctypes.c_void_p),
            h.ctypes.data_as(ctypes.c_void_p), None)
        assert rc != 0
        assert b"level" in eng.lib.mg_last_error(eng.ctx)
    rc, _ = _raw_filled(eng, v, 3)
    assert rc != 0
    eng.mesh_chunk(v, resolution=RES)  # resident volume for SKIP_H2D
    rc, _ = _raw_filled(eng, v, 1, flags=MG_FLAG_SKIP_H2D)
    assert rc != 0
    assert b"SKIP_H2D" in eng.lib.mg_last_error(eng.ctx)
    with pytest.raises(ValueError):
        eng.mesh_chunk(v, resolution=RES, fill_holes=1, skip_h2d=True)
    with pytest.raises(NotImplementedError):
        eng.mesh_chunk(v, resolution=RES, fill_holes=3)
    with pytest.raises(NotImplementedError):
        eng.fill_holes(v, 3)
    # the engine still works
    _assert_meshsets_equal(eng.mesh_chunk(v, resolution=RES),
                           oracle.mesh_chunk(v, resolution=RES), "after")


def test_simplification_applies_to_both_meshings(eng):
    import oracle
    v = R.case_three_deep(np.uint32)
    want_f, want_h, _ = ref(("three_deep", "uint32"), v, 1)
    got_f, got_h = eng.mesh_chunk(v, resolution=RES, reduction_factor=4,
                                  max_error=1e6, fill_holes=1)
    kw = dict(resolution=RES, reduction_factor=4, max_error=1e6)
    _assert_meshsets_equal(got_f, oracle.mesh_chunk(want_f, **kw), "filled")
    _assert_meshsets_equal(got_h, oracle.mesh_chunk(want_h, **kw), "holes")
    plain = oracle.mesh_chunk(want_h, resolution=RES)
    assert got_h[2][1].shape[0] < plain[2][1].shape[0]


# ---------------------------------------------------------------------------
# end to end

def test_meshtask_end_to_end(tmp_layer_path):
    import oracle
    from igneous_amd import MeshTask, PrecomputedVolume, Mesh
    from igneous_amd.storage import CloudFiles
    A, B, D = 1, 2, 4
    data = np.zeros((32, 32, 32), dtype=np.uint32, order="F")
    data[:16, :16, :16] = R.case_nested(np.uint32)   # A > B > cavity
    data[18:30, 18:30, 18:30] = D                     # D swallows a piece
    data[22:25, 22:25, 22:25] = A                     # ... of A
    PrecomputedVolume.from_numpy(
        data, tmp_layer_path, resolution=(16, 16, 40),
        chunk_size=(32, 32, 32), mesh_dir="mesh")
    # no padding and open edges: the mesher sees exactly `data`, and the
    # vertex shift into global coordinates is zero
    MeshTask(shape=(32,) * 3, offset=(0,) * 3, layer_path=tmp_layer_path,
             mip=0, simplification_factor=0, fill_holes=1,
             low_padding=0, high_padding=0, closed_dataset_edges=False,
             spatial_index=False).execute()

    filled, holes, rounds = R.fill_holes_ref(data, 1)
    assert rounds == 2
    fm = oracle.mesh_chunk(filled, resolution=RES)
    hm = oracle.mesh_chunk(holes, resolution=RES)
    assert sorted(fm) == [A, D] and sorted(hm) == [A, B]
    want = {
        A: Mesh.concatenate(Mesh(*fm[A]), Mesh(*hm[A]), id=A),
        B: Mesh(*hm[B], id=B),
        D: Mesh(*fm[D], id=D),
    }
    cf = CloudFiles(tmp_layer_path)
    for segid, mesh in want.items():
        mesh.vertices[:] += np.float32(0)  # the task's (zero) global shift
        got = cf.get(f"mesh/{segid}:0:0-32_0-32_0-32")
        assert got is not None, f"no fragment for {segid}"
        assert got == mesh.to_precomputed(), f"segment {segid} differs"
    got_a = Mesh.from_precomputed(cf.get(f"mesh/{A}:0:0-32_0-32_0-32"))
    assert got_a.vertices.shape[0] == fm[A][0].shape[0] + hm[A][0].shape[0]
    assert hm[A][0].shape[0] > 0
