"""bench.py --dump-outputs: file set, dtypes, determinism and the size cap,
checked on the host with a stand-in engine (the GPU path is the same
dump_outputs call fed by Engine.mesh_chunk)."""
import os

import numpy as np

import bench


class _FakeEngine:
    """Returns a fixed seeded meshset shaped like Engine.mesh_chunk's."""

    def __init__(self, nlabels=600):
        rng = np.random.default_rng(1)
        self.meshes = {}
        for lab in rng.choice(1 << 40, size=nlabels, replace=False).tolist():
            nv = int(rng.integers(3, 40))
            nf = int(rng.integers(1, 60))
            self.meshes[lab + 1] = (
                rng.random((nv, 3), dtype=np.float32),
                rng.integers(0, nv, size=(nf, 3)).astype(np.uint32))
        self.calls = []

    def mesh_chunk(self, data, **kw):
        self.calls.append(kw)
        return dict(self.meshes)


_STATS = {"total_tris": 123, "total_verts": 77, "n_labels": 600}
_NAMES = {"counts", "labels", "nverts", "nfaces", "sample_index",
          "sample_verts", "sample_faces"}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_files(tmp_path):
    eng = _FakeEngine()
    bench.dump_outputs(eng, None, False, _STATS, str(tmp_path / "a"))
    bench.dump_outputs(eng, None, False, _STATS, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == _NAMES
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    # the fetch uses the timed step's arguments, device-resident input
    assert eng.calls[0]["reduction_factor"] == 0
    assert eng.calls[0]["skip_h2d"] is True
    assert "device_only" not in eng.calls[0]

    labels = sorted(eng.meshes)
    assert a["counts"].tolist() == [123.0, 77.0, 600.0]
    assert a["labels"].astype(np.uint64).tolist() == labels
    assert a["nverts"].tolist() == [eng.meshes[l][0].shape[0] for l in labels]
    assert a["nfaces"].tolist() == [eng.meshes[l][1].shape[0] for l in labels]
    pick = a["sample_index"].astype(int)
    assert len(pick) == bench.DUMP_LABELS and np.all(np.diff(pick) > 0)
    want_v = np.concatenate([eng.meshes[labels[i]][0] for i in pick])
    want_f = np.concatenate([eng.meshes[labels[i]][1] for i in pick])
    assert np.array_equal(a["sample_verts"], want_v)
    assert np.array_equal(a["sample_faces"], want_f.astype(np.float64))


def test_dump_outputs_simplify_and_size_cap(tmp_path, monkeypatch):
    eng = _FakeEngine()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 40000)
    bench.dump_outputs(eng, None, True, _STATS, str(tmp_path))
    assert eng.calls[0]["reduction_factor"] == 100
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert total <= 40000
    a = _load(tmp_path)
    assert 0 < len(a["sample_index"]) < bench.DUMP_LABELS
    assert len(a["labels"]) == 600  # sizes of every label are kept
