"""Host side of the device label map: remap.fold_label_ops folds
remap_table / object_ids / exclude_object_ids into one {key -> val} table
plus a miss policy; MeshTask hands that table to a mesher advertising
handles_label_map instead of preprocessing on the host; `mesh forge`
exposes --labels / --exclude-labels.

The checker for the fold is the host sequence MeshTask ran before
(mask_except -> remap -> mask_except -> mask from igneous_amd/remap.py);
the checker for geometry is the CPU oracle. Everything here runs without
a GPU; the engine's kernels are covered by tests/test_gpu_label_map.py."""
import itertools

import numpy as np
import pytest
from click.testing import CliRunner

from igneous_amd import MeshTask, PrecomputedVolume
from igneous_amd import remap as R


def host_sequence(data, remap_table, object_ids, exclude_object_ids):
    """The host preprocessing of MeshTask.execute (reference
    mesh.py:200-204, 357-369) on a copy."""
    d = data.copy()
    if remap_table is not None:
        table = {int(k): int(v) for k, v in remap_table.items()}
        table[0] = 0
        d = R.mask_except(d, list(table.keys()))
        d = R.remap(d, table)
    if object_ids:
        d = R.mask_except(d, object_ids)
    if exclude_object_ids:
        d = R.mask(d, exclude_object_ids)
    return d


def apply_label_map(data, label_map):
    """Trivial per-voxel dict lookup of a folded (keys, vals, miss)."""
    if label_map is None:
        return data.copy()
    keys, vals, miss = label_map
    assert miss in ('keep', 'zero')
    assert keys.dtype == np.uint64 and vals.dtype == np.uint64
    table = dict(zip(keys.tolist(), vals.tolist()))
    assert len(table) == len(keys), "duplicate keys"
    assert 0 not in table
    out = data.copy()
    flat_in = data.reshape(-1)
    flat_out = out.reshape(-1)
    for i, lab in enumerate(flat_in.tolist()):
        if lab == 0:
            continue
        if lab in table:
            flat_out[i] = table[lab]
        elif miss == 'zero':
            flat_out[i] = 0
    return out


def _volume(dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint64:
        ids = rng.integers(1 << 33, 1 << 40, size=6).astype(np.uint64)
    else:
        ids = rng.integers(1, 1 << 28, size=6).astype(np.uint32)
    ids = np.concatenate([np.zeros(1, dtype), ids]).astype(dtype)
    assert len(set(ids.tolist())) == 7
    data = ids[rng.integers(0, 7, size=(9, 8, 7))]
    return np.asfortranarray(data), [int(i) for i in ids[1:]]


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_fold_matches_host_sequence(dtype):
    data, (a, b, c, d, e, f) = _volume(dtype, 11)
    absent = a + 1
    assert absent not in (a, b, c, d, e, f)
    tables = [
        None,
        {},
        {0: a, a: b},                 # key 0 is forced to 0 -> 0
        {a: a, absent: c},            # key absent from the volume
        {a: b, b: c},                 # chain: no second lookup
        {a: d, b: d, c: d},           # many-to-one
        {a: 0, b: b},                 # a value of 0 erases
    ]
    id_lists = [None, [], [b, d], [0, b, c]]
    excludes = [[], [d], [0, b, c]]
    n = 0
    for table, ids, excl in itertools.product(tables, id_lists, excludes):
        folded = R.fold_label_ops(table, ids, excl, dtype)
        want = host_sequence(data, table, ids, excl)
        if table is None and not ids and not excl:
            assert folded is None
        else:
            assert folded is not None
        got = apply_label_map(data, folded)
        assert np.array_equal(got, want), (table, ids, excl)
        n += 1
    assert n == 7 * 4 * 3


def test_fold_shapes_and_policies():
    keys, vals, miss = R.fold_label_ops({3: 7, "5": "7"}, None, [], np.uint32)
    assert keys.tolist() == [3, 5] and vals.tolist() == [7, 7]
    assert miss == 'zero'
    keys, vals, miss = R.fold_label_ops({}, None, [], np.uint64)
    assert len(keys) == 0 and len(vals) == 0 and miss == 'zero'
    keys, vals, miss = R.fold_label_ops(None, [4, 2, 2, 0], [4], np.uint32)
    assert keys.tolist() == [2] and vals.tolist() == [2] and miss == 'zero'
    keys, vals, miss = R.fold_label_ops(None, None, [9, 0, 8], np.uint32)
    assert keys.tolist() == [8, 9] and vals.tolist() == [0, 0]
    assert miss == 'keep'
    assert R.fold_label_ops(None, None, [], np.uint32) is None
    assert R.fold_label_ops(None, [], None, np.uint64) is None


def test_fold_validation():
    with pytest.raises(ValueError):
        R.fold_label_ops({1: 1 << 32}, None, [], np.uint32)
    # the same value fits uint64
    keys, vals, _ = R.fold_label_ops({1: 1 << 32}, None, [], np.uint64)
    assert vals.tolist() == [1 << 32]
    with pytest.raises(ValueError):
        R.fold_label_ops({1: -2}, None, [], np.uint64)
    with pytest.raises(ValueError):
        R.fold_label_ops({-1: 2}, None, [], np.uint64)
    with pytest.raises(ValueError):
        R.fold_label_ops(None, [-3], [], np.uint32)
    with pytest.raises(ValueError):
        R.fold_label_ops(None, None, [-3], np.uint32)
    # keys that cannot be a uint32 voxel are dropped, not an error
    keys, vals, _ = R.fold_label_ops({1 << 32: 5, 2: 6}, None, [], np.uint32)
    assert keys.tolist() == [2] and vals.tolist() == [6]
    keys, _, _ = R.fold_label_ops(None, [7, 1 << 40], [], np.uint32)
    assert keys.tolist() == [7]
    keys, _, _ = R.fold_label_ops(None, None, [7, 1 << 40], np.uint32)
    assert keys.tolist() == [7]


# ---------------------------------------------------------------------------
# MeshTask wiring

class RecordingMesher:
    """Stand-in for the engine's module-level mesh_chunk: advertises both
    device preprocessing steps, applies them itself in numpy in the
    engine's order (dust on raw labels, then the label map), then meshes
    with the oracle."""
    handles_label_map = True
    handles_dust = True

    def __init__(self):
        self.calls = []

    def __call__(self, data, resolution=(1, 1, 1), reduction_factor=0,
                 max_error=40.0, voxel_centered=True, copy=True,
                 dust_threshold=0, label_map=None):
        import oracle
        self.calls.append({
            'data': data.copy(), 'dust_threshold': dust_threshold,
            'label_map': label_map})
        d = data.copy()
        if dust_threshold:
            ids, counts = np.unique(d, return_counts=True)
            dust = [int(i) for i, ct in zip(ids, counts)
                    if ct < dust_threshold and i != 0]
            d = R.mask(d, dust)
        d = apply_label_map(d, label_map)
        return oracle.mesh_chunk(
            d, resolution=resolution, reduction_factor=reduction_factor,
            max_error=max_error, voxel_centered=voxel_centered)


def _wiring_volume():
    data = np.zeros((24, 24, 24), dtype=np.uint32)
    data[2:10, 2:10, 2:10] = 1
    data[10:16, 2:10, 2:10] = 2      # face-adjacent to 1, merged with it
    data[2:10, 12:20, 2:10] = 3
    data[12:20, 12:20, 2:10] = 4     # excluded after the remap
    data[2:4, 2:4, 14:16] = 5        # 8 voxels: dust
    data[12:20, 12:20, 14:22] = 6    # remapped to an id not in object_ids
    data[2:8, 2:8, 18:22] = 7        # absent from the remap table
    return data


WIRING_OPTS = dict(
    remap_table={1: 10, 2: 10, 3: 30, 4: 40, 5: 50, 6: 60},
    object_ids=[10, 30, 40, 50],
    exclude_object_ids=[40],
    dust_threshold=20,
)


def test_meshtask_hands_label_map_to_mesher(tmp_layer_path, oracle_mesher):
    from igneous_amd.tasks import mesh as mesh_mod
    raw = _wiring_volume()
    PrecomputedVolume.from_numpy(
        raw, tmp_layer_path, resolution=(4, 4, 40), chunk_size=(24, 24, 24),
        mesh_dir="mesh")

    def run():
        return MeshTask(
            shape=(24, 24, 24), offset=(0, 0, 0), layer_path=tmp_layer_path,
            mip=0, simplification_factor=0, dry_run=True,
            **WIRING_OPTS).execute()

    want_meshes, want_boxes = run()          # host path (plain oracle)
    assert sorted(want_meshes) == [10, 30]

    fake = RecordingMesher()
    mesh_mod.set_mesher(fake)
    got_meshes, got_boxes = run()

    assert len(fake.calls) == 1
    call = fake.calls[0]
    assert call['dust_threshold'] == 20
    keys, vals, miss = call['label_map']
    assert miss == 'zero'
    assert dict(zip(keys.tolist(), vals.tolist())) == {
        1: 10, 2: 10, 3: 30, 4: 0, 5: 50, 6: 0}
    # the mesher received the RAW labels: nothing was preprocessed on host
    assert set(np.unique(call['data']).tolist()) == {0, 1, 2, 3, 4, 5, 6, 7}

    assert sorted(got_meshes) == sorted(want_meshes)
    for label in want_meshes:
        assert np.array_equal(got_meshes[label].vertices,
                              want_meshes[label].vertices)
        assert np.array_equal(got_meshes[label].faces,
                              want_meshes[label].faces)
    assert got_boxes == want_boxes


def test_fold_above_table_cap_takes_host_path(tmp_layer_path, monkeypatch):
    """A fold larger than the engine's table cap is preprocessed on the
    host (dust included: the host remap forces the host dust order)."""
    from igneous_amd import engine
    from igneous_amd.tasks import mesh as mesh_mod
    PrecomputedVolume.from_numpy(
        _wiring_volume(), tmp_layer_path, resolution=(4, 4, 40),
        chunk_size=(24, 24, 24), mesh_dir="mesh")
    monkeypatch.setattr(engine, "LABEL_MAP_MAX_ENTRIES", 2)
    fake = RecordingMesher()
    mesh_mod.set_mesher(fake)
    try:
        meshes, _ = MeshTask(
            shape=(24, 24, 24), offset=(0, 0, 0), layer_path=tmp_layer_path,
            mip=0, simplification_factor=0, dry_run=True,
            **WIRING_OPTS).execute()
    finally:
        mesh_mod.set_mesher(None)
    call = fake.calls[0]
    assert call['label_map'] is None and call['dust_threshold'] == 0
    assert set(np.unique(call['data']).tolist()) == {0, 10, 30}
    assert sorted(meshes) == [10, 30]


def test_meshtask_without_options_passes_no_map(tmp_layer_path):
    from igneous_amd.tasks import mesh as mesh_mod
    PrecomputedVolume.from_numpy(
        _wiring_volume(), tmp_layer_path, resolution=(4, 4, 40),
        chunk_size=(24, 24, 24), mesh_dir="mesh")
    fake = RecordingMesher()
    mesh_mod.set_mesher(fake)
    try:
        MeshTask(shape=(24, 24, 24), offset=(0, 0, 0),
                 layer_path=tmp_layer_path, mip=0, simplification_factor=0,
                 dry_run=True).execute()
    finally:
        mesh_mod.set_mesher(None)
    assert fake.calls[0]['label_map'] is None
    assert fake.calls[0]['dust_threshold'] == 0


def test_engine_mesher_advertises_label_map():
    from igneous_amd import engine
    assert engine.mesh_chunk.handles_label_map is True
    assert engine.mesh_chunk.handles_dust is True
    assert "mg_mesh_chunk_mapped" in engine._EXPORTED_SYMBOLS
    assert engine.MgStats._fields_[-1][0] == "ms_labelmap"


# ---------------------------------------------------------------------------
# CLI

def test_forge_labels_options(tmp_layer_path, monkeypatch):
    from igneous_amd import cli
    data = np.zeros((32, 32, 32), dtype=np.uint32)
    data[2:30, 2:30, 2:30] = 3
    PrecomputedVolume.from_numpy(
        data, tmp_layer_path, resolution=(1, 1, 1), chunk_size=(32, 32, 32))
    created = []
    real = cli.create_meshing_tasks

    def recording(*args, **kwargs):
        tasks = real(*args, **kwargs)
        created.append(tasks)
        return tasks

    monkeypatch.setattr(cli, "create_meshing_tasks", recording)
    res = CliRunner().invoke(cli.main, [
        "mesh", "forge", tmp_layer_path, "--mip", "0", "--shape", "32,32,32",
        "--labels", "1,3", "--exclude-labels", "3", "--no-execute"])
    assert res.exit_code == 0, res.output
    tasks = list(created[0])
    assert len(tasks) == 1
    for t in tasks:
        assert t.options['object_ids'] == [1, 3]
        assert t.options['exclude_object_ids'] == [3]

    # without the options the tasks carry the defaults
    created.clear()
    res = CliRunner().invoke(cli.main, [
        "mesh", "forge", tmp_layer_path, "--mip", "0", "--shape", "32,32,32",
        "--no-execute"])
    assert res.exit_code == 0, res.output
    for t in created[0]:
        assert t.options['object_ids'] is None
        assert t.options['exclude_object_ids'] == []
