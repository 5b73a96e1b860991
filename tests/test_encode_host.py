"""MeshTask's encoded path on the CPU: a mesher whose encode_chunk is the
oracle plus encode_ref (the host loop itself) must leave exactly the files
the plain host loop leaves, and the task must take that path only where it
may. The engine's own encode stage is tests/test_gpu_encode.py."""
import gzip
import os

import numpy as np
import pytest

from igneous_amd import MeshTask, PrecomputedVolume
from igneous_amd.engine import EncodedChunk
from igneous_amd.tasks import mesh as mesh_mod

from encode_ref import encoded_chunk_ref


def _make_layer(path):
    """64^3 u32, resolution (16,16,40), voxel offset, three segments (one
    touching the closed dataset edge so left_offset is exercised)."""
    data = np.zeros((64, 64, 64), dtype=np.uint32)
    data[0:20, 5:30, 5:30] = 7
    data[25:50, 10:40, 10:44] = 3
    data[30:40, 45:60, 50:63] = 1000
    PrecomputedVolume.from_numpy(
        data, path, resolution=(16, 16, 40), voxel_offset=(128, 64, 32),
        chunk_size=(64, 64, 64), mesh_dir="mesh")


def _files(layer_path):
    """{relative name: stored bytes} of everything under the layer; gzip
    objects decompressed (their header carries the write time)."""
    root = layer_path[len("file://"):]
    out = {}
    for dirpath, _dirs, names in os.walk(root):
        for name in names:
            full = os.path.join(dirpath, name)
            with open(full, "rb") as f:
                raw = f.read()
            if raw[:2] == b"\x1f\x8b":
                raw = gzip.decompress(raw)
            out[os.path.relpath(full, root)] = raw
    return out


class _EncodingMesher:
    """The oracle as MeshTask's mesher, advertising encode_chunk built
    from the oracle and encode_ref; counts the calls of each."""

    def __init__(self, empty_label=None):
        self.mesh_calls = 0
        self.encode_calls = 0
        self.empty_label = empty_label
        self.encode_chunk = self._encode_chunk

    def _mesh(self, data, resolution, reduction_factor, max_error,
              voxel_centered):
        import oracle
        return oracle.mesh_chunk(
            data, resolution=resolution, reduction_factor=reduction_factor,
            max_error=max_error, voxel_centered=voxel_centered)

    def __call__(self, data, resolution=(1, 1, 1), reduction_factor=0,
                 max_error=40.0, voxel_centered=True, **kw):
        self.mesh_calls += 1
        return self._mesh(data, resolution, reduction_factor, max_error,
                          voxel_centered)

    def _encode_chunk(self, data, resolution=(1, 1, 1), reduction_factor=0,
                      max_error=40.0, voxel_centered=True, shift=(0, 0, 0),
                      encoding='precomputed', draco=None, copy=True):
        self.encode_calls += 1
        if draco is not None:
            assert type(draco['quantization_bits']) is int
        raw = self._mesh(data, resolution, reduction_factor, max_error,
                         voxel_centered)
        chunk = encoded_chunk_ref(raw, shift, encoding, draco)
        if self.empty_label is not None:
            nverts = chunk.nverts.copy()
            nverts[chunk.labels.tolist().index(self.empty_label)] = 0
            chunk = EncodedChunk(chunk.labels, chunk.offsets, chunk.sizes,
                                 nverts, chunk.ntris, chunk.bboxes, chunk.blob)
        return chunk


@pytest.fixture
def encoding_mesher():
    m = _EncodingMesher()
    mesh_mod.set_mesher(m)
    yield m
    mesh_mod.set_mesher(None)


def _run(tmp_path, sub, **kw):
    path = f"file://{tmp_path}/{sub}"
    _make_layer(path)
    out = MeshTask(shape=(64, 64, 64), offset=(128, 64, 32), layer_path=path,
                   mip=0, simplification_factor=0, **kw).execute()
    return out, _files(path)


CASES = {
    "precomputed_manifests": dict(generate_manifests=True),
    "draco": dict(encoding='draco'),
    "sharded_frags": dict(sharded=True),
    "spatial_index": dict(spatial_index=True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_encoded_path_writes_the_host_loops_files(tmp_path, oracle_mesher,
                                                  case):
    kw = CASES[case]
    _out, want = _run(tmp_path, "host", **kw)   # plain oracle_mesher
    m = _EncodingMesher()
    mesh_mod.set_mesher(m)
    _out, got = _run(tmp_path, "encoded", **kw)
    assert m.encode_calls == 1 and m.mesh_calls == 0
    assert sorted(got) == sorted(want)
    frag_like = [n for n in want if n.startswith("mesh/")]
    assert len(frag_like) >= 1
    for name in want:
        assert got[name] == want[name], name
    if case == "spatial_index":
        import json
        name = [n for n in want if ".spatial" in n][0]
        assert json.loads(got[name]) == json.loads(want[name])
        assert sorted(json.loads(got[name])) == ["1000", "3", "7"]


def test_fill_holes_keeps_the_host_loop(tmp_path, encoding_mesher):
    m = encoding_mesher
    m.handles_fill_holes = True
    orig = m._mesh
    m._mesh = lambda *a: (orig(*a), {})    # (filled, holes) pair
    _run(tmp_path, "fill", fill_holes=1)
    assert m.encode_calls == 0 and m.mesh_calls == 1


def test_dry_run_keeps_the_host_loop(tmp_path, encoding_mesher):
    out, files = _run(tmp_path, "dry", dry_run=True)
    assert encoding_mesher.encode_calls == 0
    assert encoding_mesher.mesh_calls == 1
    meshes, boxes = out
    assert sorted(meshes) == [3, 7, 1000] and sorted(boxes) == [3, 7, 1000]
    assert not [n for n in files if n.startswith("mesh/")]


def test_empty_entry_sends_the_chunk_to_the_host_loop(tmp_path,
                                                      oracle_mesher):
    _out, want = _run(tmp_path, "host")
    m = _EncodingMesher(empty_label=7)
    mesh_mod.set_mesher(m)
    _out, got = _run(tmp_path, "encoded")
    assert m.encode_calls == 1 and m.mesh_calls == 1
    assert got == want


def test_formats_attribute_limits_the_default_path(tmp_path, encoding_mesher):
    """encode_chunk.formats names the encodings the task hands over."""
    m = encoding_mesher

    def only_draco(*a, **kw):
        return m._encode_chunk(*a, **kw)
    only_draco.formats = ('draco',)
    m.encode_chunk = only_draco
    _run(tmp_path, "pre")
    assert (m.encode_calls, m.mesh_calls) == (0, 1)
    _run(tmp_path, "dra", encoding='draco')
    assert (m.encode_calls, m.mesh_calls) == (1, 1)


def _hand_built():
    blob = np.arange(40, dtype=np.uint8)
    # entries out of blob order, with a gap, one of size 0
    return blob, EncodedChunk(
        labels=[2, 9, 2 ** 40], offsets=[30, 0, 12], sizes=[10, 12, 0],
        nverts=[1, 2, 0], ntris=[1, 1, 0],
        bboxes=np.arange(18, dtype=np.float32).reshape(3, 6), blob=blob)


def test_encoded_chunk_slices_by_label():
    blob, ch = _hand_built()
    assert len(ch) == 3
    assert ch[2] == bytes(range(30, 40))
    assert ch[9] == bytes(range(0, 12))
    assert ch[2 ** 40] == b""
    assert ch.bbox(9) == [6.0, 7.0, 8.0, 9.0, 10.0, 11.0]
    assert 9 in ch and 3 not in ch
    with pytest.raises(KeyError):
        ch[3]
    with pytest.raises(KeyError):
        ch[-1]
    items = list(ch.items())
    assert [(k, type(k)) for k, _b, _x in items] == [
        (2, int), (9, int), (2 ** 40, int)]
    assert [b for _k, b, _x in items] == [ch[2], ch[9], b""]
    assert all(type(b) is bytes for _k, b, _x in items)
    assert items[0][2] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    assert ch.sizes.tolist() == [10, 12, 0]
    assert ch.bboxes.shape == (3, 6) and ch.bboxes.dtype == np.float32


def test_encoded_chunk_copy_semantics():
    """The blob is held as given (a view stays a view: copy=False); the
    bytes handed out own their storage."""
    blob, ch = _hand_built()
    assert np.shares_memory(ch.blob, blob)
    before = ch[9]
    blob[0] = 99          # the staging is reused by a later call
    assert before == bytes(range(0, 12))
    assert ch[9][0] == 99
    owned = EncodedChunk(ch.labels, ch.offsets, ch.sizes, ch.nverts,
                         ch.ntris, ch.bboxes, blob.copy())
    blob[1] = 98
    assert owned[9][:2] == bytes([99, 1])


def test_encoded_chunk_rejects_bad_tables():
    with pytest.raises(ValueError):
        EncodedChunk([1, 2], [0, 4], [4, 8], [1, 1], [1, 1],
                     np.zeros((2, 6)), np.zeros(8, np.uint8))   # past blob
    with pytest.raises(ValueError):
        EncodedChunk([2, 1], [0, 4], [4, 4], [1, 1], [1, 1],
                     np.zeros((2, 6)), np.zeros(8, np.uint8))   # not sorted
    with pytest.raises(ValueError):
        EncodedChunk([1, 2], [0], [4], [1], [1],
                     np.zeros((1, 6)), np.zeros(8, np.uint8))   # lengths


def test_engine_advertises_the_encoded_path():
    from igneous_amd import engine
    assert engine.mesh_chunk.encode_chunk is engine.mesh_chunk_encoded
    assert engine.MgStatsEncode._fields_[-1][0] == "ms_encode"
    import ctypes
    assert engine.MgStatsEncode.ms_encode.offset == ctypes.sizeof(
        engine.MgStatsFill)
