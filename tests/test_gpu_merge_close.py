"""GPU tests for mg_merge_close_vertices: the device weld must return
exactly what meshops.merge_close_vertices returns — the same float32 vertex
bits, the same uint32 faces, the same dtypes. The inputs,
their expected sizes and the tie condition are checked on the CPU by
tests/test_merge_close_contract.py as well."""
import ctypes

import numpy as np
import pytest

from merge_close_inputs import (WELD_CASES, assert_no_ties, assert_same_mesh,
                                host_weld, mesh_input)

pytestmark = pytest.mark.gpu

NO_V = np.zeros((0, 3), np.float32)
NO_F = np.zeros((0, 3), np.uint32)


def _gpu_engine():
    from igneous_amd.engine import Engine
    return Engine.get(0)


def _private(fn):
    """fn(eng) as the one and only call of a private context."""
    from igneous_amd.engine import Engine
    eng = Engine(0)
    try:
        return fn(eng)
    finally:
        eng.lib.mg_destroy(eng.ctx)
        eng.ctx = None


def _check_case(eng, case):
    name, r, nv, nf = WELD_CASES[case]
    v, f = mesh_input(name)
    want = host_weld(name, r)
    got = eng.merge_close_vertices(v, f, r)
    assert_same_mesh(got, want, case)
    return got


@pytest.mark.parametrize("case", list(WELD_CASES))
def test_weld_equals_host(case):
    name, r, nv, nf = WELD_CASES[case]
    assert_no_ties(mesh_input(name)[0], r)
    got = _check_case(_gpu_engine(), case)
    assert got[0].shape == (nv, 3) and got[1].shape == (nf, 3)


def test_empty_mesh():
    gv, gf = _gpu_engine().merge_close_vertices(NO_V, NO_F, 1e-5)
    assert gv.shape == (0, 3) and gv.dtype == np.float32
    assert gf.shape == (0, 3) and gf.dtype == np.uint32


def test_vertices_without_faces():
    v, _ = mesh_input("chain")
    gv, gf = _gpu_engine().merge_close_vertices(v, NO_F, 1.0)
    assert gv.shape == (0, 3) and gv.dtype == np.float32
    assert gf.shape == (0, 3) and gf.dtype == np.uint32


def test_module_level_wrapper_carries_the_id():
    from igneous_amd import engine
    from igneous_amd.meshes import Mesh
    v, f = mesh_input("chain")
    v = np.concatenate([v, v[:3] + np.float32(100.0)])
    f = np.concatenate([f, np.array([[50, 51, 52]], np.uint32)])
    want = Mesh(v, f, id=42).merge_close_vertices(radius=0.1)
    got = engine.merge_close_vertices(Mesh(v, f, id=42), radius=0.1)
    assert got.id == 42 and len(want.faces) == 49
    assert_same_mesh((got.vertices, got.faces), (want.vertices, want.faces))


def _raw_rc(eng, v, f, r):
    """mg_merge_close_vertices without the wrapper's own radius check."""
    ov = ctypes.POINTER(ctypes.c_float)()
    of = ctypes.POINTER(ctypes.c_uint32)()
    onv, ont = ctypes.c_uint32(), ctypes.c_uint32()
    with eng._lock:
        rc = eng.lib.mg_merge_close_vertices(
            eng.ctx, v.ctypes.data_as(ctypes.c_void_p), v.shape[0],
            f.ctypes.data_as(ctypes.c_void_p), f.shape[0], r,
            ctypes.byref(ov), ctypes.byref(onv),
            ctypes.byref(of), ctypes.byref(ont))
        err = eng.lib.mg_last_error(eng.ctx).decode()
    return rc, err


@pytest.mark.parametrize("case", ["face_index", "nan_vertex", "r_zero",
                                  "r_inf", "cell_range"])
def test_rejected_inputs_are_clean_errors(case):
    eng = _gpu_engine()
    v, f = (a.copy() for a in mesh_input("chain"))
    r = 1.0
    if case == "face_index":
        f[5, 1] = v.shape[0]
        rc, match = 100, "references vertex"
    elif case == "nan_vertex":
        v[7, 2] = np.nan
        rc, match = 100, "not finite"
    elif case == "r_zero":
        r, rc, match = 0.0, 100, "radius"
    elif case == "r_inf":
        r, rc, match = float("inf"), 100, "radius"
    else:
        v[3, 0] = 1e38
        r, rc, match = 1e-5, 103, "2\\^51"
    if case in ("r_zero", "r_inf"):
        with pytest.raises(ValueError, match="radius"):
            eng.merge_close_vertices(v, f, r)
    else:
        with pytest.raises(RuntimeError, match=match):
            eng.merge_close_vertices(v, f, r)
    got_rc, err = _raw_rc(eng, v, f, r)
    assert got_rc == rc and match.replace("\\", "") in err, (got_rc, err)
    _check_case(eng, "chain")


def test_candidate_cap_rejects_before_the_link():
    """70 000 identical vertices share one grid cell: about 4.9e9 candidate
    visits, over the 2^32 cap. The count pass rejects the call."""
    eng = _gpu_engine()
    v = np.full((70000, 3), 1.25, np.float32)
    f = np.array([[0, 1, 2]], np.uint32)
    with pytest.raises(RuntimeError, match="radius too large"):
        eng.merge_close_vertices(v, f, 1e-5)
    _check_case(eng, "chain")


def test_small_call_after_a_larger_one():
    eng = _gpu_engine()
    _check_case(eng, "box_3.1")
    after = _check_case(eng, "chain")
    assert_same_mesh(after, _private(
        lambda e: e.merge_close_vertices(*mesh_input("chain"), 1.0)))
    after = _check_case(eng, "cloud_0.45")
    _check_case(eng, "box_3.1")
    assert_same_mesh(after, host_weld("cloud", 0.45), "cloud after box")


def test_two_runs_give_identical_bytes():
    eng = _gpu_engine()
    v, f = mesh_input("cat")
    a = eng.merge_close_vertices(v, f, 3.1)
    b = eng.merge_close_vertices(v, f, 3.1)
    assert_same_mesh(a, b, "second run")


def test_first_call_merge_close_vertices():
    v, f = mesh_input("cat")
    got = _private(lambda eng: eng.merge_close_vertices(v, f, 2.3))
    assert_same_mesh(got, host_weld("cat", 2.3), "first call")
