"""dust_global on the product engine (pytest -m gpu): the chunk's labels are
counted on the device, looked up in a global table, the labels below the
threshold folded into the label map and the counted volume meshed without a
second upload. Every result is bit-equal to the same call on a volume the
host masked first; the last test runs the whole pipeline, from the counting
tasks to the mesh files."""
import functools

import numpy as np
import pytest

from igneous_amd import remap
from igneous_amd.formats.intmap import IntMap
from test_dust_global_host import A, B, BOXES, two_chunk_volume
from test_gpu_ctx_lifecycle import _assert_meshsets_equal

RES = (16.0, 16.0, 40.0)
SHIFT = (1600.0, 3200.0, 12000.0)


@functools.lru_cache(maxsize=None)
def _vor48():
    from igneous_amd.synth import voronoi_labels
    return voronoi_labels((48, 48, 48), 60, 11, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _setup():
    """(volume, threshold, global table, dust labels): every second label
    is three times as large elsewhere in the 'dataset', so the global
    threshold keeps labels the chunk-local one would drop."""
    vol = _vor48()
    u, c = np.unique(vol, return_counts=True)
    table = {int(k): int(n) * (3 if i % 2 else 1)
             for i, (k, n) in enumerate(zip(u, c))}
    nz = [(k, n) for k, n in zip(u.tolist(), c.tolist()) if k]
    threshold = int(np.median([n for _, n in nz]))
    dust = [k for k, _ in nz if table[k] < threshold]
    local = [k for k, n in nz if n < threshold]
    return vol, threshold, IntMap(IntMap(table).tobytes()), dust, local


def _masked():
    vol, _, _, dust, _ = _setup()
    return remap.mask(vol.copy(order="F"), dust)


def test_inputs_are_not_trivial():
    vol, threshold, table, dust, local = _setup()
    labels = np.unique(vol[vol != 0]).tolist()
    assert 0 < len(dust) < len(local) < len(labels)
    assert set(dust) < set(local)
    assert _masked().any() and not np.array_equal(_masked(), vol)
    results = []
    for which, sel in _selections().items():
        out = _host_selection(_masked(), **sel)
        assert len(np.unique(out)) > 4, which
        assert not any(np.array_equal(out, r) for r in results), which
        results.append(out)


def _selections():
    vol, _, _, dust, _ = _setup()
    labels = np.unique(vol[vol != 0]).tolist()
    kept = [k for k in labels if k not in dust]
    # merge pairs of labels, one dust label among the keys, and drop some
    table = {k: kept[(i // 2) * 2] for i, k in enumerate(kept[:20])}
    table[dust[0]] = kept[0]
    return {
        "plain": {},
        "remap": dict(remap_table=table),
        "object_ids": dict(object_ids=kept[3:15] + dust[:2]),
        "exclude_object_ids": dict(exclude_object_ids=kept[:7] + dust[:2]),
    }


def _host_selection(vol, remap_table=None, object_ids=None,
                    exclude_object_ids=None):
    """MeshTask's host sequence after dust (mesh.py:199-204, 357-369)."""
    if remap_table is not None:
        table = dict(remap_table)
        table[0] = 0
        vol = remap.mask_except(vol, list(table))
        vol = remap.remap(vol, table)
    if object_ids:
        vol = remap.mask_except(vol, object_ids)
    if exclude_object_ids:
        vol = remap.mask(vol, exclude_object_ids)
    return vol


@pytest.fixture(scope="module")
def eng():
    from igneous_amd.engine import Engine
    return Engine.get(0)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["plain", "remap", "object_ids",
                                   "exclude_object_ids"])
def test_mesh_chunk_equals_the_oracle_on_the_masked_volume(eng, which):
    import oracle
    vol, threshold, table, _, _ = _setup()
    sel = _selections()[which]
    label_map = remap.fold_label_ops(
        sel.get("remap_table"), sel.get("object_ids"),
        sel.get("exclude_object_ids"), vol.dtype)
    assert (label_map is None) == (which == "plain")
    before = vol.copy(order="F")
    got = eng.mesh_chunk(vol, resolution=RES, label_map=label_map,
                         dust_global=(threshold, table.lookup))
    assert np.array_equal(vol, before)      # the host array is not touched
    want_vol = _host_selection(_masked(), **sel)
    want = oracle.mesh_chunk(want_vol, resolution=RES)
    assert len(want) > 3
    _assert_meshsets_equal(got, want, which)


@pytest.mark.gpu
@pytest.mark.parametrize("encoding", ["precomputed", "draco"])
def test_mesh_chunk_encoded_equals_the_call_on_the_masked_volume(
        eng, encoding):
    from test_gpu_encode import _draco_settings
    vol, threshold, table, dust, _ = _setup()
    kw = dict(resolution=RES, shift=SHIFT, encoding=encoding,
              draco=_draco_settings((49, 49, 49))
              if encoding == "draco" else None)
    want = eng.mesh_chunk_encoded(_masked(), **kw)
    got = eng.mesh_chunk_encoded(vol, dust_global=(threshold, table.lookup),
                                 **kw)
    assert len(want) > 3 and not set(dust) & set(want.labels.tolist())
    assert np.array_equal(got.labels, want.labels)
    assert np.array_equal(got.nverts, want.nverts)
    assert np.array_equal(got.ntris, want.ntris)
    assert got.bboxes.tobytes() == want.bboxes.tobytes()
    for (gl, gb, _), (wl, wb, _) in zip(got.items(), want.items()):
        assert gl == wl and gb == wb, gl


@pytest.mark.gpu
def test_keyword_rules(eng):
    vol, threshold, table, _, _ = _setup()
    dg = (threshold, table.lookup)
    with pytest.raises(ValueError, match="dust_threshold"):
        eng.mesh_chunk(vol, dust_threshold=5, dust_global=dg)
    with pytest.raises(ValueError, match="skip_h2d"):
        eng.mesh_chunk(vol, skip_h2d=True, dust_global=dg)
    with pytest.raises(ValueError, match="skip_h2d"):
        eng.mesh_chunk_encoded(vol, skip_h2d=True, dust_global=dg)
    # a label the table does not know: the lookup's KeyError comes through,
    # and the engine works afterwards
    short = IntMap({0: 1})
    with pytest.raises(KeyError):
        eng.mesh_chunk(vol, dust_global=(threshold, short.lookup))
    from igneous_amd import engine
    assert engine.mesh_chunk.handles_dust_global is True
    small = two_chunk_volume()[:32]
    got = eng.mesh_chunk(small, dust_global=(50, IntMap(
        {0: 0, A: 60, B: 40}).lookup))
    assert sorted(got) == [A]


def _files(layer_path, prefix):
    from igneous_amd.storage import CloudFiles
    cf = CloudFiles(layer_path)
    return {name: cf.get(name) for name in cf.list(prefix)}


@pytest.mark.gpu
@pytest.mark.parametrize("encoding", ["precomputed", "draco"])
def test_pipeline_count_sum_mesh(tmp_path, encoding):
    """create_voxel_counting_tasks -> accumulate_voxel_counts ->
    create_meshing_tasks(dust_threshold=50, dust_global=True) on the product
    engine: A (30 + 30 voxels) is meshed in both chunks, B (40) in none —
    the files of a run over the pre-masked dataset without dust."""
    from igneous_amd.queue import LocalTaskQueue
    from igneous_amd.task_creation import (accumulate_voxel_counts,
                                           create_meshing_tasks,
                                           create_voxel_counting_tasks)
    from igneous_amd.tasks import mesh as mesh_mod
    from igneous_amd.volume import PrecomputedVolume
    assert mesh_mod._mesher_fn is None       # the product engine

    def run(path, vol, **kw):
        PrecomputedVolume.from_numpy(vol, path, resolution=(16, 16, 40),
                                     chunk_size=(32, 32, 32))
        with LocalTaskQueue(parallel=1) as tq:
            if kw:
                tq.insert(create_voxel_counting_tasks(path, mip=0))
                accumulate_voxel_counts(path, mip=0, progress=False)
            tq.insert(create_meshing_tasks(
                path, mip=0, shape=(32, 32, 32), mesh_dir="mesh",
                simplification=False,   # a 30-voxel mesh collapses to nothing
                encoding=encoding, **kw))
        return _files(path, "mesh/")

    vol = two_chunk_volume()
    got = run(f"file://{tmp_path}/dusted", vol, dust_threshold=50,
              dust_global=True)
    counts = IntMap(_files(f"file://{tmp_path}/dusted",
                           "16_16_40/stats/voxel_counts.im").popitem()[1])
    assert dict(counts.items()) == {0: vol.size - 100, A: 60, B: 40}
    masked = vol.copy(order="F")
    masked[masked == B] = 0
    want = run(f"file://{tmp_path}/premasked", masked)
    assert sorted(n for n in got if ":0:" in n) == [
        f"mesh/{A}:0:{box}" for box in BOXES]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
