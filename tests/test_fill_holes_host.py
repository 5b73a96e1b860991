"""Host tests of fill_holes levels 1-2: the checker (tests/fill_holes_ref.py)
reproduces the closed-form cases of the contract with their
exact counts, and the Python surface (MeshTask refusal of levels >= 3,
create_meshing_tasks' range assertion, the CLI option, the public names)
is in place. No GPU needed."""
import ctypes

import numpy as np
import pytest

import fill_holes_ref as R

DTYPES = [np.uint32, np.uint64]


@pytest.mark.parametrize("dtype", DTYPES)
def test_nested_cavity(dtype):
    v = R.case_nested(dtype)
    A, B = R.lift(1, dtype), R.lift(2, dtype)
    filled, holes, rounds = R.fill_holes_ref(v, 1)
    assert rounds == 2
    assert np.all(filled[1:15, 1:15, 1:15] == A)
    assert np.count_nonzero(filled) == 14 ** 3
    assert np.count_nonzero(holes) == 504
    assert np.all(holes[holes != 0] == B)
    assert np.array_equal(holes != 0, v == B)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nested_piece_of_outer_label(dtype):
    v = R.case_nested(dtype, inner='A')
    A, B = R.lift(1, dtype), R.lift(2, dtype)
    filled, holes, rounds = R.fill_holes_ref(v, 1)
    assert rounds == 2
    assert np.all(filled[1:15, 1:15, 1:15] == A)
    # the inner A piece ends up A again: not a hole
    assert np.count_nonzero(holes) == 504
    assert np.array_equal(holes != 0, v == B)
    assert np.all(holes[holes != 0] == B)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [R.case_two_adjacent, R.case_island])
@pytest.mark.parametrize("level", [1, 2])
def test_unchanged_cases(dtype, case, level):
    v = case(dtype)
    filled, holes, rounds = R.fill_holes_ref(v, level)
    assert rounds == 0
    assert np.array_equal(filled, v)
    assert not holes.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_open_cavity_levels_differ(dtype):
    v = R.case_open_cavity(dtype)
    assert np.count_nonzero(v == 0) == 96
    f1, h1, r1 = R.fill_holes_ref(v, 1)
    assert np.array_equal(f1, v) and not h1.any() and r1 == 0
    f2, h2, r2 = R.fill_holes_ref(v, 2)
    assert np.all(f2 == R.lift(1, dtype))
    assert np.count_nonzero(f2 != v) == 96
    assert not h2.any()   # a background cavity contributes only zeros
    assert r2 == 1        # the slice pass closed it, one 3-D round fills it


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_diagonal_cavity_is_filled(dtype):
    v = R.case_edge_diagonal(dtype)
    filled, holes, rounds = R.fill_holes_ref(v, 1)
    assert rounds == 1
    assert filled[3, 3, 8] == R.lift(1, dtype)
    assert filled[2, 2, 8] == 0
    assert np.count_nonzero(filled != v) == 1


def test_three_deep_and_serpentine():
    v = R.case_three_deep(np.uint32)
    filled, holes, rounds = R.fill_holes_ref(v, 1)
    assert rounds == 3
    assert np.all(filled[1:19, 1:19, 1:19] == 1)
    assert np.count_nonzero(holes == 2) == 12 ** 3 - 6 ** 3
    assert np.count_nonzero(holes == 3) == 6 ** 3 - 2 ** 3
    s = R.case_serpentine(np.uint32)
    assert np.count_nonzero(s == 0) > 1500
    filled, holes, rounds = R.fill_holes_ref(s, 1)
    assert rounds == 1 and np.all(filled == 1) and not holes.any()


def test_size_one_axes_have_no_border():
    # 40x40x1: the z axis has no border, the in-plane perimeter has
    v = np.ones((40, 40, 1), dtype=np.uint32, order="F")
    v[10:20, 10:20, 0] = 0
    v[0, 5, 0] = 0
    filled, _, rounds = R.fill_holes_ref(v, 1)
    assert rounds == 1 and filled[15, 15, 0] == 1 and filled[0, 5, 0] == 0
    # 1x1x50: only the two end voxels are border
    w = np.ones((1, 1, 50), dtype=np.uint32, order="F")
    w[0, 0, 20:25] = 7
    w[0, 0, 0] = 0
    filled, holes, _ = R.fill_holes_ref(w, 1)
    assert np.all(filled[0, 0, 1:] == 1) and filled[0, 0, 0] == 0
    assert np.count_nonzero(holes == 7) == 5


# ----------------------------------------------------------------------
# Python surface

def _make_layer(path):
    from igneous_amd import PrecomputedVolume
    data = np.zeros((32, 32, 32), dtype=np.uint32)
    data[2:30, 2:30, 2:30] = 4
    PrecomputedVolume.from_numpy(
        data, path, resolution=(1, 1, 1), chunk_size=(32, 32, 32),
        mesh_dir="mesh")


def test_level3_raises_naming_dilation(tmp_layer_path):
    from igneous_amd import MeshTask
    _make_layer(tmp_layer_path)
    t = MeshTask(shape=(32,) * 3, offset=(0,) * 3,
                 layer_path=tmp_layer_path, fill_holes=3)
    with pytest.raises(NotImplementedError, match="dilation"):
        t.execute()


def test_level_104_rejected_by_task_creation(tmp_layer_path):
    from igneous_amd import create_meshing_tasks
    _make_layer(tmp_layer_path)
    with pytest.raises(AssertionError):
        create_meshing_tasks(tmp_layer_path, 0, (32, 32, 32), fill_holes=104)


def test_cli_forwards_fill_holes(tmp_layer_path, monkeypatch):
    from click.testing import CliRunner
    from igneous_amd import cli
    _make_layer(tmp_layer_path)
    seen = []
    monkeypatch.setattr(cli, "execute_tasks",
                        lambda tasks: seen.extend(tasks) or len(seen))
    res = CliRunner().invoke(cli.main, [
        "mesh", "forge", tmp_layer_path, "--shape", "32,32,32",
        "--fill-holes", "2"])
    assert res.exit_code == 0, res.output
    assert len(seen) == 1
    assert seen[0].options['fill_holes'] == 2


def test_public_names():
    import igneous_amd
    from igneous_amd import engine
    assert callable(igneous_amd.fill_holes)
    assert engine.mesh_chunk.handles_fill_holes is True
    for sym in ("mg_fill_holes", "mg_mesh_chunk_filled", "mg_mesh_holes"):
        assert sym in engine._EXPORTED_SYMBOLS
    # mg_stats grew at its end: the earlier layout is a prefix
    assert engine.MgStatsFill._fields_[-1][0] == "ms_fill"
    assert engine.MgStatsFill.ms_fill.offset == ctypes.sizeof(engine.MgStats)
    assert list(engine.MgStatsFill().as_dict())[-2:] == ["ms_labelmap",
                                                         "ms_fill"]


def test_mesher_without_fill_support_is_refused(tmp_layer_path,
                                                oracle_mesher):
    from igneous_amd import MeshTask
    _make_layer(tmp_layer_path)
    t = MeshTask(shape=(32,) * 3, offset=(0,) * 3,
                 layer_path=tmp_layer_path, fill_holes=2)
    with pytest.raises(NotImplementedError, match="handles_fill_holes"):
        t.execute()


def test_task_merges_filled_and_hole_meshes(tmp_layer_path):
    """MeshTask host logic with a mesher that advertises fill support:
    checker fill + oracle meshing behind the seam; the fragments are the
    per-segment concatenation of mesh.py:238-242."""
    import oracle
    from igneous_amd import MeshTask, PrecomputedVolume, Mesh
    from igneous_amd.storage import CloudFiles
    from igneous_amd.tasks import mesh as mesh_mod

    data = np.zeros((32, 32, 32), dtype=np.uint32)
    data[:16, :16, :16] = R.case_nested(np.uint32)
    PrecomputedVolume.from_numpy(
        data, tmp_layer_path, resolution=(1, 1, 1), chunk_size=(32, 32, 32),
        mesh_dir="mesh")
    calls = []

    def fn(vol, resolution=(1, 1, 1), reduction_factor=0, max_error=40.0,
           voxel_centered=True, fill_holes=0, **kw):
        calls.append((vol.copy(), fill_holes))
        filled, holes, _ = R.fill_holes_ref(vol, fill_holes)
        return (oracle.mesh_chunk(filled, resolution=resolution),
                oracle.mesh_chunk(holes, resolution=resolution))
    fn.handles_fill_holes = True

    mesh_mod.set_mesher(fn)
    try:
        MeshTask(shape=(32,) * 3, offset=(0,) * 3, layer_path=tmp_layer_path,
                 fill_holes=1, simplification_factor=0,
                 low_padding=0, high_padding=0).execute()
    finally:
        mesh_mod.set_mesher(None)
    assert len(calls) == 1 and calls[0][1] == 1
    vol = calls[0][0]
    filled, holes, _ = R.fill_holes_ref(vol, 1)
    fm = oracle.mesh_chunk(filled, resolution=(1, 1, 1))
    hm = oracle.mesh_chunk(holes, resolution=(1, 1, 1))
    assert sorted(fm) == [1] and sorted(hm) == [2]
    cf = CloudFiles(tmp_layer_path)
    names = sorted(n.split("/")[-1] for n in cf.list("mesh/")
                   if ":0:" in n)
    assert [n.split(":")[0] for n in names] == ["1", "2"]
    got_b = Mesh.from_precomputed(cf.get("mesh/" + names[1]))
    assert got_b.vertices.shape[0] == hm[2][0].shape[0]
    assert np.array_equal(got_b.faces, hm[2][1])
