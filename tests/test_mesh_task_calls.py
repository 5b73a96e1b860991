"""What MeshTask.execute() asks of its mesher: one call per execute, the
exact keyword dict (values AND types), and errors raised inside the mesher
reaching the caller. Plus the two manifest tasks on one fabricated layer.
CPU only: the mesher is a recorder."""
import numpy as np
import pytest

from igneous_amd import (
    MeshTask, MeshManifestFilesystemTask, MeshManifestPrefixTask,
    PrecomputedVolume,
)
from igneous_amd.storage import CloudFiles
from igneous_amd.tasks import mesh as mesh_mod

from test_label_map_host import _wiring_volume


class Recorder:
    """A mesher that advertises every device-side capability and records
    its keywords; it meshes nothing."""
    handles_dust = True
    handles_label_map = True
    handles_fill_holes = True

    def __init__(self, raises=None):
        self.calls = []
        self.raises = raises

    def __call__(self, data, **kw):
        self.calls.append(kw)
        if self.raises is not None:
            raise self.raises
        return ({}, {}) if kw.get('fill_holes') else {}


@pytest.fixture
def layer(tmp_layer_path):
    PrecomputedVolume.from_numpy(
        _wiring_volume(), tmp_layer_path, resolution=(4, 4, 40),
        chunk_size=(24, 24, 24), mesh_dir="mesh")
    return tmp_layer_path


def _execute(layer, mesher, **kw):
    mesh_mod.set_mesher(mesher)
    try:
        return MeshTask(shape=(24, 24, 24), offset=(0, 0, 0),
                        layer_path=layer, mip=0, **kw).execute()
    finally:
        mesh_mod.set_mesher(None)


def test_typeerror_from_the_mesher_propagates_after_one_call(layer):
    boom = TypeError("raised inside the mesher")
    fake = Recorder(raises=boom)
    with pytest.raises(TypeError) as info:
        _execute(layer, fake)
    assert info.value is boom
    assert len(fake.calls) == 1


# the keywords every call carries; simplification_factor and
# max_simplification_error are the task's defaults (100, 40)
COMMON = dict(resolution=(4.0, 4.0, 40.0), reduction_factor=100,
              max_error=40.0, voxel_centered=True, copy=False)

KEYWORD_CASES = {
    "plain": ({}, COMMON),
    "dust_remap_object_ids": (
        dict(dust_threshold=20,
             remap_table={1: 10, 2: 10, 3: 30, 4: 40, 5: 50, 6: 60},
             object_ids=[10, 30, 40, 50]),
        dict(COMMON, dust_threshold=20, label_map=(
            np.array([1, 2, 3, 4, 5, 6], dtype=np.uint64),
            np.array([10, 10, 30, 40, 50, 0], dtype=np.uint64), 'zero'))),
    "fill_holes": (dict(fill_holes=1), dict(COMMON, fill_holes=1)),
    "dry_run": (dict(dry_run=True), dict(COMMON, copy=True)),
}


@pytest.mark.parametrize("case", list(KEYWORD_CASES))
def test_keywords_handed_to_the_mesher(layer, case):
    options, want = KEYWORD_CASES[case]
    want = dict(want)
    fake = Recorder()
    _execute(layer, fake, **options)
    assert len(fake.calls) == 1
    got = dict(fake.calls[0])
    print(case, got)
    assert sorted(got) == sorted(want)
    if 'label_map' in want:
        keys, vals, miss = got.pop('label_map')
        wkeys, wvals, wmiss = want.pop('label_map')
        assert keys.dtype == np.uint64 and vals.dtype == np.uint64
        assert np.array_equal(keys, wkeys) and np.array_equal(vals, wvals)
        assert miss == wmiss
    assert got == want
    for name, value in want.items():
        assert type(got[name]) is type(value), name
    assert all(type(r) is float for r in got['resolution'])


def test_manifest_tasks_filter_by_lod_and_prefix(tmp_layer_path):
    """Two segids, two lods: each task writes the manifests of its lod
    (and prefix) only, fragments in listing order."""
    PrecomputedVolume.from_numpy(
        np.zeros((8, 8, 8), np.uint32), tmp_layer_path, mesh_dir="mesh")
    cf = CloudFiles(tmp_layer_path)
    for segid in (7, 81):
        for lod in (0, 1):
            for frag in ("0-8_0-8_0-8", "8-16_0-8_0-8"):
                cf.put(f"mesh/{segid}:{lod}:{frag}", b"")

    def frags(segid, lod):
        return {"fragments": [f"{segid}:{lod}:0-8_0-8_0-8",
                              f"{segid}:{lod}:8-16_0-8_0-8"]}

    MeshManifestFilesystemTask(layer_path=tmp_layer_path, lod=1)
    assert cf.get_json("mesh/7:1") == frags(7, 1)
    assert cf.get_json("mesh/81:1") == frags(81, 1)
    assert cf.get_json("mesh/7:0") is None
    assert cf.get_json("mesh/81:0") is None

    MeshManifestPrefixTask(layer_path=tmp_layer_path, prefix="8")
    assert cf.get_json("mesh/81:0") == frags(81, 0)
    assert cf.get_json("mesh/7:0") is None
    MeshManifestPrefixTask(layer_path=tmp_layer_path, prefix="7", lod=0,
                           mesh_dir="mesh")
    assert cf.get_json("mesh/7:0") == frags(7, 0)
