"""The global dust threshold on the host: remap.fold_dust, and MeshTask's
dust_global with a fake mesher that advertises handles_dust_global (it does
what the engine does — unique, the lookup it is handed, mask — with numpy
and meshes with the CPU oracle; checker role only).

The dataset is two 32^3 chunks. Label A has 30 voxels in each chunk (60 in
all), label B 40 voxels in chunk 0 only. With dust_threshold=50 the global
threshold keeps A (60 >= 50) in both chunks and drops B; the chunk-local one
drops everything."""
import numpy as np
import pytest

from igneous_amd import remap
from igneous_amd.formats.intmap import IntMap
from igneous_amd.queue import LocalTaskQueue
from igneous_amd.storage import CloudFiles
from igneous_amd.task_creation import (accumulate_voxel_counts,
                                       create_meshing_tasks,
                                       create_voxel_counting_tasks)
from igneous_amd.tasks import mesh as mesh_mod
from igneous_amd.volume import PrecomputedVolume

A, B = 7, (1 << 40) + 3
KEY = "1_1_1"
BOXES = ["0-32_0-32_0-32", "32-64_0-32_0-32"]


def two_chunk_volume():
    vol = np.zeros((64, 32, 32), dtype=np.uint64, order="F")
    vol[4:9, 4:7, 4:6] = A        # 30 voxels, chunk 0
    vol[40:45, 4:7, 4:6] = A      # 30 voxels, chunk 1
    vol[16:21, 16:20, 16:18] = B  # 40 voxels, chunk 0
    return vol


def test_the_dataset_is_the_one_described():
    vol = two_chunk_volume()
    for lo in (0, 32):
        assert np.count_nonzero(vol[lo:lo + 32] == A) == 30
    assert np.count_nonzero(vol[:32] == B) == 40
    assert np.count_nonzero(vol[32:] == B) == 0
    # nothing in the voxel a chunk shares with its neighbour
    assert not vol[31:34].any()


# ---------------------------------------------------------------------------
# fold_dust

def _apply(vol, label_map):
    """One lookup per voxel with its raw label (mg_label_map's rule)."""
    if label_map is None:
        return vol.copy()
    keys, vals, miss = label_map
    assert keys.dtype == np.uint64 and vals.dtype == np.uint64
    assert np.all(keys[1:] > keys[:-1]) and 0 not in keys.tolist()
    table = dict(zip(keys.tolist(), vals.tolist()))
    out = [0 if v == 0 else table.get(v, v if miss == 'keep' else 0)
           for v in vol.reshape(-1).tolist()]
    return np.array(out, dtype=vol.dtype).reshape(vol.shape)


def _maps(rng):
    keep = remap.fold_label_ops(None, None, [3, 4, 9, 40], np.uint64)
    zero_ids = remap.fold_label_ops(None, [1, 2, 3, 5, 9], [], np.uint64)
    table = {int(k): int(rng.integers(1, 5)) for k in (1, 2, 3, 6, 9, 11)}
    zero_remap = remap.fold_label_ops(table, None, [2], np.uint64)
    assert keep[2] == 'keep' and zero_ids[2] == 'zero'
    assert zero_remap[2] == 'zero'
    return [None, keep, zero_ids, zero_remap]


@pytest.mark.parametrize("seed", range(4))
def test_fold_dust_equals_mask_then_map(seed):
    rng = np.random.default_rng(seed)
    for label_map in _maps(rng):
        vol = rng.integers(0, 12, size=(16, 16, 16)).astype(np.uint64)
        dust = rng.choice(np.arange(1, 14), size=5, replace=False)
        want = _apply(remap.mask(vol.copy(), dust.tolist()), label_map)
        folded = remap.fold_dust(label_map, dust.astype(np.uint64),
                                 np.uint64)
        got = _apply(vol, folded)
        assert np.array_equal(got, want)
        if label_map is None:
            assert not np.array_equal(want, vol)


def test_fold_dust_edge_cases():
    assert remap.fold_dust(None, [], np.uint64) is None
    assert remap.fold_dust(None, [0], np.uint64) is None
    keys, vals, miss = remap.fold_dust(None, [9, 2, 9, 0], np.uint32)
    assert keys.tolist() == [2, 9] and vals.tolist() == [0, 0]
    assert miss == 'keep' and keys.dtype == np.uint64
    # an id that does not fit the volume's dtype can never match
    keys, _, _ = remap.fold_dust(None, [5, 1 << 40], np.uint32)
    assert keys.tolist() == [5]
    lm = (np.array([2, 5], np.uint64), np.array([7, 0], np.uint64), 'keep')
    keys, vals, miss = remap.fold_dust(lm, [2, 3], np.uint64)
    assert (keys.tolist(), vals.tolist(), miss) == ([2, 3, 5], [0, 0, 0],
                                                     'keep')
    lm = (np.array([2, 5], np.uint64), np.array([7, 8], np.uint64), 'zero')
    keys, vals, miss = remap.fold_dust(lm, [2, 3], np.uint64)
    assert (keys.tolist(), vals.tolist(), miss) == ([5], [8], 'zero')
    assert remap.fold_dust(lm, [], np.uint64)[0].tolist() == [2, 5]
    with pytest.raises(ValueError):
        remap.fold_dust((lm[0], lm[1], 'drop'), [2], np.uint64)


# ---------------------------------------------------------------------------
# MeshTask

def _oracle(data, kw):
    import oracle
    return oracle.mesh_chunk(
        data, resolution=kw['resolution'],
        reduction_factor=kw['reduction_factor'], max_error=kw['max_error'],
        voxel_centered=kw['voxel_centered'])


def _device_like_mesher(calls):
    """What engine.mesh_chunk does with dust_global= / label_map=."""
    def fn(data, copy=True, label_map=None, dust_global=None, **kw):
        calls.append(dust_global)
        assert 'dust_threshold' not in kw
        if dust_global is not None:
            threshold, lookup = dust_global
            values = np.unique(data).astype(np.uint64)
            values = values[values != 0]
            dust = values[lookup(values) < np.uint64(threshold)]
            data = remap.mask(data.copy(), dust.tolist())
        return _oracle(_apply(data, label_map), kw)
    fn.handles_dust_global = True
    fn.handles_label_map = True
    fn.count_voxels = lambda v: np.unique(v, return_counts=True)
    return fn


def _host_map_mesher(calls):
    """A mesher that takes the global counts but no label map: MeshTask
    counts with count_voxels and masks on the host."""
    def fn(data, copy=True, **kw):
        calls.append(sorted(kw))
        return _oracle(data, kw)
    fn.handles_dust_global = True
    fn.count_voxels = lambda v: np.unique(v, return_counts=True)
    return fn


@pytest.fixture(params=[_device_like_mesher, _host_map_mesher],
                ids=["device_map", "host_map"])
def mesher(request):
    calls = []
    fn = request.param(calls)
    fn.calls = calls
    mesh_mod.set_mesher(fn)
    yield fn
    mesh_mod.set_mesher(None)


def _layer(path, vol=None):
    PrecomputedVolume.from_numpy(
        two_chunk_volume() if vol is None else vol, path,
        chunk_size=(32, 32, 32))
    return path


def _count(path):
    with LocalTaskQueue(parallel=1) as tq:
        tq.insert(create_voxel_counting_tasks(path, mip=0))
    accumulate_voxel_counts(path, mip=0, progress=False)


def _mesh(path, **kw):
    tasks = create_meshing_tasks(
        path, mip=0, shape=(32, 32, 32), simplification=False,
        mesh_dir="mesh", compress=None, **kw)
    assert len(tasks) == 2
    with LocalTaskQueue(parallel=1) as tq:
        tq.insert(tasks)
    cf = CloudFiles(path)
    return {name: cf.get(name) for name in cf.list("mesh/")
            if ":0:" in name}


def test_global_threshold_keeps_what_is_large_overall(tmp_layer_path, mesher):
    _layer(tmp_layer_path)
    _count(tmp_layer_path)
    sidecar = IntMap(CloudFiles(tmp_layer_path).get(
        f"{KEY}/stats/voxel_counts.im"))
    assert sidecar[A] == 60 and sidecar[B] == 40
    frags = _mesh(tmp_layer_path, dust_threshold=50, dust_global=True)
    assert sorted(frags) == [f"mesh/{A}:0:{box}" for box in BOXES]
    assert all(len(b) > 4 for b in frags.values())
    assert len(mesher.calls) == 2


def test_global_threshold_with_a_label_selection(tmp_layer_path, mesher,
                                                 tmp_path):
    """Dust first, on the raw labels, then exclude_object_ids."""
    vol = two_chunk_volume()
    vol[50:54, 20:24, 20:24] = 9   # 64 voxels, chunk 1: large, but excluded
    _layer(tmp_layer_path, vol)
    _count(tmp_layer_path)
    frags = _mesh(tmp_layer_path, dust_threshold=50, dust_global=True,
                  exclude_object_ids=[9])
    assert sorted(frags) == [f"mesh/{A}:0:{box}" for box in BOXES]
    other = f"file://{tmp_path}/premasked"
    vol[vol == B] = 0
    vol[vol == 9] = 0
    _layer(other, vol)
    want = _mesh(other)
    assert frags == want


def test_local_threshold_drops_everything(tmp_layer_path, mesher):
    _layer(tmp_layer_path)
    _count(tmp_layer_path)
    assert _mesh(tmp_layer_path, dust_threshold=50, dust_global=False) == {}


def test_no_threshold_ignores_dust_global(tmp_layer_path, mesher):
    _layer(tmp_layer_path)   # no sidecar: it is never asked for
    frags = _mesh(tmp_layer_path, dust_threshold=None, dust_global=True)
    assert sorted(frags) == sorted(
        [f"mesh/{A}:0:{box}" for box in BOXES] + [f"mesh/{B}:0:{BOXES[0]}"])


def test_a_missing_sidecar_is_an_error(tmp_layer_path, mesher):
    _layer(tmp_layer_path)
    with pytest.raises(FileNotFoundError, match="voxel_counts.im"):
        _mesh(tmp_layer_path, dust_threshold=50, dust_global=True)


def test_a_label_absent_from_the_sidecar_is_an_error(tmp_layer_path, mesher):
    _layer(tmp_layer_path)
    CloudFiles(tmp_layer_path).put(
        f"{KEY}/stats/voxel_counts.im", IntMap({0: 1, A: 60}).tobytes())
    with pytest.raises(KeyError) as e:
        _mesh(tmp_layer_path, dust_threshold=50, dust_global=True)
    assert e.value.args == (B,)


def test_the_sidecar_is_parsed_once_per_path(tmp_layer_path, mesher,
                                             monkeypatch):
    from igneous_amd.formats import intmap
    _layer(tmp_layer_path)
    _count(tmp_layer_path)
    parsed = []
    real = intmap.IntMap._parse
    monkeypatch.setattr(intmap.IntMap, "_parse",
                        staticmethod(lambda buf: parsed.append(1) or
                                     real(buf)))
    _mesh(tmp_layer_path, dust_threshold=50, dust_global=True)
    assert parsed == [1]   # two tasks, one parse
