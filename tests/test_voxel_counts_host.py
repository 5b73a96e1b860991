"""CountVoxelsTask, create_voxel_counting_tasks, accumulate_voxel_counts and
the `voxels` commands on the host, with an injected mesher whose
count_voxels is np.unique (checker role; the product counter is the HIP
engine's mg_count_voxels).

The volume is 48 x 32 x 32 with 32^3 tasks: the second task is cut to 16
voxels at the volume's upper edge."""
import os

import numpy as np
import pytest

from igneous_amd.formats.intmap import IntMap
from igneous_amd.queue import LocalTaskQueue, RegisteredTask
from igneous_amd.storage import CloudFiles
from igneous_amd.task_creation import (accumulate_voxel_counts,
                                       create_voxel_counting_tasks)
from igneous_amd.tasks import CountVoxelsTask
from igneous_amd.tasks import mesh as mesh_mod
from igneous_amd.volume import PrecomputedVolume

SHAPE = (32, 32, 32)
KEY = "1_1_1"
NAMES = ["0-32_0-32_0-32", "32-48_0-32_0-32"]
BIG = (1 << 63) + 5


def _volume():
    rng = np.random.default_rng(11)
    vol = rng.integers(0, 6, size=(48, 32, 32)).astype(np.uint64)
    vol[40:, :4, :4] = BIG        # only in the second task
    vol[:8, :8, :8] = 77          # only in the first
    return np.asfortranarray(vol)


def _np_counter(labels):
    assert labels.ndim == 3
    return np.unique(labels, return_counts=True)


@pytest.fixture
def counting_mesher():
    def fn(*a, **kw):
        raise AssertionError("the mesher itself is not called")
    fn.count_voxels = _np_counter
    mesh_mod.set_mesher(fn)
    yield fn
    mesh_mod.set_mesher(None)


@pytest.fixture
def layer(tmp_layer_path):
    PrecomputedVolume.from_numpy(_volume(), tmp_layer_path,
                                 chunk_size=(32, 32, 32))
    return tmp_layer_path


def _want(vol):
    u, c = np.unique(vol, return_counts=True)
    return {int(k): int(v) for k, v in zip(u, c)}


def _run(tasks):
    with LocalTaskQueue(parallel=1) as tq:
        tq.insert(tasks)


def test_tasks_write_one_json_per_unpadded_box(layer, counting_mesher):
    vol = _volume()
    tasks = create_voxel_counting_tasks(layer, mip=0, shape=SHAPE)
    assert len(tasks) == 2
    listed = list(tasks)
    assert [list(t.shape) for t in listed] == [[32, 32, 32], [16, 32, 32]]
    assert all(isinstance(t, CountVoxelsTask) for t in listed)
    _run(listed)
    cf = CloudFiles(layer)
    assert sorted(cf.list(f"{KEY}/stats/")) == [
        f"{KEY}/stats/voxel_counts/{n}.json" for n in NAMES]
    got = [cf.get_json(f"{KEY}/stats/voxel_counts/{n}.json") for n in NAMES]
    assert got[0] == {str(k): v for k, v in _want(vol[:32]).items()}
    assert got[1] == {str(k): v for k, v in _want(vol[32:]).items()}
    assert "0" in got[0] and str(BIG) in got[1] and "77" not in got[1]
    # the boxes do not overlap: every voxel is counted once
    assert sum(sum(g.values()) for g in got) == vol.size


def test_an_oversized_task_is_clamped(layer, counting_mesher):
    CountVoxelsTask(layer, (512, 512, 512), (32, 0, 0)).execute()
    got = CloudFiles(layer).get_json(
        f"{KEY}/stats/voxel_counts/{NAMES[1]}.json")
    assert got == {str(k): v for k, v in _want(_volume()[32:]).items()}


def test_payload_round_trip(layer):
    t = CountVoxelsTask(layer, (16, 32, 32), (32, 0, 0), mip=0,
                        fill_missing=True)
    t2 = RegisteredTask.deserialize(t.payload())
    assert isinstance(t2, CountVoxelsTask)
    assert list(t2.shape) == [16, 32, 32] and list(t2.offset) == [32, 0, 0]
    assert t2.fill_missing is True


def test_accumulate_equals_unique_of_the_whole_volume(layer, counting_mesher,
                                                      tmp_path):
    _run(create_voxel_counting_tasks(layer, mip=0, shape=SHAPE))
    extra = str(tmp_path / "copy.im")
    accumulate_voxel_counts(layer, mip=0, progress=False,
                            additional_output=extra, shape=SHAPE)
    buf = CloudFiles(layer).get(f"{KEY}/stats/voxel_counts.im")
    im = IntMap(buf)
    assert dict(im.items()) == _want(_volume())
    assert 0 in im and im[BIG] == 8 * 4 * 4
    with open(extra, "rb") as f:
        assert f.read() == buf
    # compressed: the same map behind the same name
    accumulate_voxel_counts(layer, mip=0, progress=False, compress="gzip",
                            shape=SHAPE)
    assert os.path.exists(
        os.path.join(layer[len("file://"):], KEY, "stats",
                     "voxel_counts.im.gz"))


def test_provenance_entry(layer, counting_mesher):
    _run(create_voxel_counting_tasks(layer, mip=0, fill_missing=True,
                                     shape=SHAPE))
    prov = CloudFiles(layer).get_json("provenance")
    assert len(prov["processing"]) == 1
    method = prov["processing"][0]["method"]
    assert method == {
        "task": "CountVoxelsTask", "cloudpath": layer, "mip": 0,
        "shape": [32, 32, 32], "fill_missing": True, "agglomerate": False,
        "timestamp": None}
    assert "by" in prov["processing"][0] and "date" in prov["processing"][0]


def test_a_missing_task_file_is_named(layer, counting_mesher):
    _run(create_voxel_counting_tasks(layer, mip=0, shape=SHAPE))
    CloudFiles(layer).delete(f"{KEY}/stats/voxel_counts/{NAMES[1]}.json")
    with pytest.raises(FileNotFoundError, match=NAMES[1]):
        accumulate_voxel_counts(layer, mip=0, progress=False, shape=SHAPE)
    assert not CloudFiles(layer).exists(f"{KEY}/stats/voxel_counts.im")


def test_graphene_options_are_refused(layer):
    with pytest.raises(NotImplementedError):
        CountVoxelsTask(layer, SHAPE, (0, 0, 0), agglomerate=True)
    with pytest.raises(NotImplementedError):
        CountVoxelsTask(layer, SHAPE, (0, 0, 0), timestamp=1700000000)


def test_a_mesher_without_a_counter_is_refused(layer, oracle_mesher):
    with pytest.raises(NotImplementedError, match="count_voxels"):
        CountVoxelsTask(layer, SHAPE, (0, 0, 0)).execute()
    assert list(CloudFiles(layer).list(f"{KEY}/stats/")) == []


def test_cli_count_then_sum(layer, counting_mesher, tmp_path):
    from click.testing import CliRunner
    from igneous_amd.cli import main
    runner = CliRunner()
    res = runner.invoke(main, ["voxels", "count", layer, "--mip", "0"])
    assert res.exit_code == 0, res.output
    assert "1 CountVoxelsTasks" in res.output
    out = str(tmp_path / "counts.im")
    res = runner.invoke(main, ["voxels", "sum", layer, "--mip", "0",
                               "--output", out])
    assert res.exit_code == 0, res.output
    buf = CloudFiles(layer).get(f"{KEY}/stats/voxel_counts.im")
    assert dict(IntMap(buf).items()) == _want(_volume())
    with open(out, "rb") as f:
        assert f.read() == buf
    # ... the sidecar the 32^3 tasks give
    CloudFiles(layer).delete([f"{KEY}/stats/voxel_counts.im"] + list(
        CloudFiles(layer).list(f"{KEY}/stats/voxel_counts/")))
    _run(create_voxel_counting_tasks(layer, mip=0, shape=SHAPE))
    accumulate_voxel_counts(layer, mip=0, progress=False, shape=SHAPE)
    assert CloudFiles(layer).get(f"{KEY}/stats/voxel_counts.im") == buf
    res = runner.invoke(main, ["mesh", "forge", "--help"])
    assert "--dust-global" in res.output
