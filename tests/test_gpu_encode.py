"""The engine's device encode stage (mg_mesh_chunk_encoded) against the host
loop it replaces. The reference in every case is encode_ref — the host
loop's own per-label function — over Engine.mesh_chunk with identical
arguments: label arrays identical, every label's bytes equal, boxes equal
under float ==."""
import ctypes
import functools
import gzip
import os

import numpy as np
import pytest

from encode_ref import assert_encoded_equal, encode_ref

pytestmark = pytest.mark.gpu

RES = (16.0, 16.0, 40.0)
SHIFT = np.array([-1234.5, 0.375, 70000.25], dtype=np.float32)


@pytest.fixture(scope="module")
def eng():
    from igneous_amd.engine import Engine
    return Engine.get(0)


@functools.lru_cache(maxsize=None)
def _vor48():
    from igneous_amd.synth import voronoi_labels
    return voronoi_labels((48, 48, 48), 60, 11, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _odd():
    """33 x 20 x 17 u32: odd dims, a partial last wave per row."""
    rng = np.random.default_rng(5)
    v = np.zeros((33, 20, 17), dtype=np.uint32, order="F")
    v[1:-1, 1:-1, 1:-1] = rng.integers(0, 6, size=(31, 18, 15))
    v[3:20, 3:15, 3:12] = 77
    return v


def _check(eng, vol, shift=SHIFT, encoding='precomputed', draco=None,
           resolution=RES, **kw):
    """One encoded call against encode_ref over mesh_chunk; -> the chunk."""
    raw = eng.mesh_chunk(vol, resolution=resolution, **kw)
    ref = encode_ref(raw, shift, encoding, draco)
    got = eng.mesh_chunk_encoded(vol, resolution=resolution, shift=shift,
                                 encoding=encoding, draco=draco, **kw)
    assert_encoded_equal(got, ref)
    assert got.nverts.tolist() == [raw[k][0].shape[0] for k in ref]
    assert got.ntris.tolist() == [raw[k][1].shape[0] for k in ref]
    assert got.sizes.tolist() == [len(ref[k][0]) for k in ref]
    # entries do not overlap
    order = np.argsort(got.offsets, kind="stable")
    ends = (got.offsets + got.sizes)[order]
    assert np.all(got.offsets[order][1:] >= ends[:-1])
    return got


# ---------------------------------------------------------------- precomputed
@pytest.mark.parametrize("rf", (0, 4))
@pytest.mark.parametrize("vol", ("vor48", "odd"))
def test_precomputed(eng, vol, rf):
    got = _check(eng, {"vor48": _vor48, "odd": _odd}[vol](),
                 reduction_factor=rf, max_error=40.0)
    assert len(got) > 3
    assert np.all(got.offsets % 4 == 0)


def test_precomputed_dust(eng):
    vol = _odd()
    full = eng.mesh_chunk(vol, resolution=RES)
    # 77 has 17*12*9 voxels, the random labels about 1100 each
    got = _check(eng, vol, dust_threshold=1500)
    assert 0 < len(got) < len(full)


def test_precomputed_label_map(eng):
    vol = _vor48()
    labs = [int(x) for x in np.unique(vol) if x != 0]
    keys = np.asarray(labs[:20], dtype=np.uint64)
    vals = np.asarray([labs[i - i % 4] for i in range(20)], dtype=np.uint64)
    got = _check(eng, vol, label_map=(keys, vals, 'zero'),
                 reduction_factor=4)
    assert got.labels.tolist() == sorted(set(vals.tolist()))


def test_zero_shift_and_voxel_edges(eng):
    _check(eng, _odd(), shift=(0, 0, 0), voxel_centered=False)


# ---------------------------------------------------------------- draco bands
def _draco_settings(shape, offset=(100, 200, 300)):
    from igneous_amd.tasks.draco import draco_encoding_settings
    d = draco_encoding_settings(
        shape=shape, offset=offset, resolution=RES, compression_level=1,
        create_metadata=False, uses_new_draco_bin_size=False)
    d['quantization_bits'] = int(d['quantization_bits'])
    return d


@functools.lru_cache(maxsize=None)
def _band_volume(shape):
    """u32, zero border: label 5 on alternating one-voxel z slices (its
    vertex count is the number of its boundary voxel faces), plus small
    labels of other bands in the last four x columns."""
    sx, sy, sz = shape
    v = np.zeros(shape, dtype=np.uint32, order="F")
    v[1:sx - 6, 1:sy - 1, 1:sz - 1:2] = 5
    v[sx - 4:sx - 2, 1:3, 1:3] = 9             # 2x2x2 cube
    v[sx - 4:sx - 1, 4:7, 1] = 4000000000       # 3x3x1 slab
    v[sx - 3, 1:sy - 1, 4] = 12                 # a rod
    return v


BANDS = {
    # name: (shape, lowest nv, nv bound)
    "u8": ((12, 8, 8), 1, 1 << 8),
    "u16": ((30, 24, 24), 1 << 8, 1 << 16),
    "varint": ((70, 64, 40), 1 << 16, 1 << 21),
    "u32": ((166, 160, 130), 1 << 21, 1 << 32),
}


@pytest.mark.parametrize("band", list(BANDS))
def test_draco_index_bands(eng, band):
    import oracle
    shape, lo, hi = BANDS[band]
    vol = _band_volume(shape)
    # the band, from the oracle's vertex count (label 5 alone: the small
    # labels do not touch it)
    nv = oracle.mesh_chunk((vol == 5).astype(np.uint32) * 5,
                           resolution=RES)[5][0].shape[0]
    assert lo <= nv < hi, (band, nv)
    draco = _draco_settings(shape)
    got = _check(eng, vol, shift=(1600.0, 3200.0, 12000.0),
                 encoding='draco', draco=draco)
    assert int(got.nverts[got.labels.tolist().index(5)]) == nv
    assert len(got) == 4
    from igneous_amd.formats import draco as draco_fmt
    v, f = draco_fmt.decode(got[5])
    assert v.shape == (nv, 3) and int(f.max()) == nv - 1


def test_draco_simplified_u64(eng):
    vol = _vor48()
    _check(eng, vol, encoding='draco', draco=_draco_settings((49, 49, 49)),
           shift=(1600.0, 3200.0, 12000.0), reduction_factor=4)


# ----------------------------------------------------------- draco arithmetic
@pytest.mark.parametrize("origin", ((0.0, 0.0, 0.0), (10.25, 3.0, 7.5)))
@pytest.mark.parametrize("bits", (1, 14, 32))
def test_draco_arithmetic(eng, bits, origin):
    """Resolution 1 puts the vertices on the half grid and range = qmax
    makes the scale 1, so .5 ties reach rint (half to even, not round);
    the second origin lies above some vertices, so the clip to 0 runs."""
    vol = _odd()
    qmax = float((1 << bits) - 1)
    draco = dict(quantization_bits=bits, quantization_range=qmax,
                 quantization_origin=np.asarray(origin))
    raw = eng.mesh_chunk(vol, resolution=(1.0, 1.0, 1.0))
    allv = np.concatenate([v for v, _f in raw.values()])
    assert np.any(allv % 1.0 == 0.5)                    # ties exist
    if origin[0] > 0:
        assert np.any(allv[:, 0] < origin[0])           # the clip runs
    got = _check(eng, vol, shift=(0.0, 0.0, 0.0), encoding='draco',
                 draco=draco, resolution=(1.0, 1.0, 1.0))
    if bits == 14 and origin[0] == 0:
        # rint, not round-half-away: 0.5 -> 0, 2.5 -> 2
        from igneous_amd.formats import draco as draco_fmt
        lab = int(got.labels[0])
        q = np.frombuffer(got[lab], dtype="<u4",
                          count=3 * int(got.nverts[0]),
                          offset=len(got[lab]) - 17 - 12 * int(got.nverts[0]))
        v = raw[lab][0].reshape(-1).astype(np.float64)
        assert np.array_equal(q, np.rint(v / qmax * qmax).astype(np.uint32))
        assert draco_fmt.decode(got[lab])[1].shape == raw[lab][1].shape


def test_draco_defaulting_in_the_wrapper(eng):
    """range <= 0 -> 1.0 and a per-axis range -> its max, as encode does."""
    vol = _odd()
    for rng in (0.0, np.asarray([100.0, 4000.0, 250.0])):
        draco = dict(quantization_bits=10, quantization_range=rng,
                     quantization_origin=np.asarray([0.0, 0.0, 0.0]))
        _check(eng, vol, shift=(0.5, 0.5, 0.5), encoding='draco',
               draco=draco)


# ------------------------------------------------------------------ lifecycle
def _blobs(chunk):
    return {k: (b, box) for k, b, box in chunk.items()}


def test_first_and_only_call_of_a_fresh_ctx():
    from igneous_amd.engine import Engine
    fresh = Engine(0)
    vol = _odd()
    got = fresh.mesh_chunk_encoded(vol, resolution=RES, shift=SHIFT)
    ref = encode_ref(Engine.get(0).mesh_chunk(vol, resolution=RES), SHIFT)
    assert_encoded_equal(got, ref)
    fresh.lib.mg_destroy(fresh.ctx)
    fresh.ctx = None


def test_smaller_call_after_a_larger_one(eng):
    """Nothing stale is read: the same bytes as on a fresh ctx."""
    from igneous_amd.engine import Engine
    draco = _draco_settings((49, 49, 49))
    small = _odd()
    for enc, d in (('precomputed', None), ('draco', draco)):
        eng.mesh_chunk_encoded(_vor48(), resolution=RES, shift=SHIFT,
                               encoding=enc, draco=d)
        after = _blobs(eng.mesh_chunk_encoded(
            small, resolution=RES, shift=SHIFT, encoding=enc, draco=d))
        fresh = Engine(0)
        first = _blobs(fresh.mesh_chunk_encoded(
            small, resolution=RES, shift=SHIFT, encoding=enc, draco=d))
        fresh.lib.mg_destroy(fresh.ctx)
        fresh.ctx = None
        assert after == first


def test_mesh_chunk_after_an_encoded_call_is_unaffected(eng):
    vol = _vor48()
    before = eng.mesh_chunk(vol, resolution=RES, reduction_factor=4)
    eng.mesh_chunk_encoded(_odd(), resolution=RES, shift=SHIFT,
                           encoding='draco', draco=_draco_settings((34,) * 3))
    after = eng.mesh_chunk(vol, resolution=RES, reduction_factor=4)
    assert list(before) == list(after)
    for k in before:
        assert np.array_equal(before[k][0], after[k][0])
        assert np.array_equal(before[k][1], after[k][1])
    assert eng.stats()["ms_encode"] == 0.0


def test_two_runs_give_identical_blobs(eng):
    vol = _vor48()
    kw = dict(resolution=RES, shift=SHIFT, reduction_factor=4,
              encoding='draco', draco=_draco_settings((49, 49, 49)))
    a = eng.mesh_chunk_encoded(vol, **kw)
    b = eng.mesh_chunk_encoded(vol, copy=False, **kw)
    assert _blobs(a) == _blobs(b)
    assert a.labels.tolist() == b.labels.tolist()


def test_all_zero_volume_gives_an_empty_set(eng):
    got = eng.mesh_chunk_encoded(np.zeros((9, 8, 7), np.uint32, order="F"),
                                 resolution=RES, shift=SHIFT)
    assert len(got) == 0 and list(got.items()) == []
    assert got.bboxes.shape == (0, 6) and got.blob.shape == (0,)


def test_device_only_runs_the_stage(eng):
    got = eng.mesh_chunk_encoded(_vor48(), resolution=RES, shift=SHIFT,
                                 device_only=True)
    assert len(got) == 0
    st = eng.stats()
    assert st["ms_encode"] > 0 and st["n_labels"] > 3
    assert st["ms_total"] >= st["ms_encode"]


@pytest.mark.parametrize("encoding", ("precomputed", "draco"))
def test_label_simplified_to_nothing_gets_an_empty_entry(eng, encoding):
    """A one-voxel label loses its last face in the simplifier (oracle and
    engine alike); the host loop would raise in np.amin there. The stage
    gives it size 0 and a zero box, the other labels their usual bytes."""
    import oracle
    vol = np.zeros((14, 12, 11), dtype=np.uint32, order="F")
    vol[2, 2, 2] = 7
    vol[5:12, 3:10, 3:9] = 3
    vol[4, 8, 8] = 2 ** 31
    kw = dict(resolution=RES, reduction_factor=100, max_error=40.0)
    assert oracle.mesh_chunk(vol, **kw)[7][0].shape == (0, 3)
    raw = eng.mesh_chunk(vol, **kw)
    assert [k for k in raw if raw[k][0].shape[0] == 0] == [7, 2 ** 31]
    draco = _draco_settings((15, 13, 12)) if encoding == 'draco' else None
    got = eng.mesh_chunk_encoded(vol, shift=SHIFT, encoding=encoding,
                                 draco=draco, **kw)
    assert got.labels.tolist() == [3, 7, 2 ** 31]
    assert got.nverts.tolist()[1:] == [0, 0]
    assert got.sizes.tolist()[1:] == [0, 0]
    assert got[7] == b"" and got.bbox(7) == [0.0] * 6
    ref = encode_ref({3: raw[3]}, SHIFT, encoding, draco)
    assert (got[3], got.bbox(3)) == ref[3]
    assert int(got.sizes[0]) == len(ref[3][0]) == got.blob.shape[0]


# --------------------------------------------------------------------- errors
def _raw_call(eng, vol, params):
    """mg_mesh_chunk_encoded with hand-made params (None = NULL)."""
    from igneous_amd import engine as E
    out = ctypes.POINTER(E._MgBlobSet)()
    rc = eng.lib.mg_mesh_chunk_encoded(
        eng.ctx, vol.ctypes.data_as(ctypes.c_void_p), *vol.shape,
        E._mg_dtype(vol), *RES, 0, 40.0, 1, 0, 0, None,
        ctypes.byref(params) if params is not None else None,
        ctypes.byref(out))
    try:
        eng._check(rc, "mg_mesh_chunk_encoded")
    finally:
        if rc == 0:
            eng.lib.mg_blobset_free(out)


def _params(fmt=1, shift=(0, 0, 0), origin=(0, 0, 0), rng=1.0, bits=14):
    from igneous_amd import engine as E
    p = E._MgEncodeParams()
    p.format = fmt
    p.shift[:] = shift
    p.q_origin[:] = origin
    p.q_range = rng
    p.q_bits = bits
    return p


ERRORS = {
    "null_params": (None, "null mg_encode_params"),
    "format": (dict(fmt=7), "unknown format 7"),
    "shift_inf": (dict(fmt=0, shift=(0, float("inf"), 0)),
                  r"non-finite shift\[1\]"),
    "shift_nan_draco": (dict(shift=(float("nan"), 0, 0)),
                        r"non-finite shift\[0\]"),
    "origin_nan": (dict(origin=(0, 0, float("nan"))),
                   r"non-finite q_origin\[2\]"),
    "range_inf": (dict(rng=float("inf")), "non-finite q_range"),
    "range_zero": (dict(rng=0.0), "q_range 0 must be > 0"),
    "range_negative": (dict(rng=-2.0), "q_range -2 must be > 0"),
    "bits_0": (dict(bits=0), "q_bits 0 outside 1..32"),
    "bits_33": (dict(bits=33), "q_bits 33 outside 1..32"),
}


@pytest.mark.parametrize("name", list(ERRORS))
def test_errors_leave_the_ctx_usable(eng, name):
    kw, msg = ERRORS[name]
    vol = _odd()
    with pytest.raises(RuntimeError, match=msg):
        _raw_call(eng, vol, None if kw is None else _params(**kw))
    _raw_call(eng, vol, _params())          # the same ctx, a valid call
    assert len(eng.mesh_chunk_encoded(vol, resolution=RES)) > 3


def test_wrapper_errors(eng):
    vol = _odd()
    with pytest.raises(ValueError, match="encoding"):
        eng.mesh_chunk_encoded(vol, encoding='obj')
    with pytest.raises(ValueError, match="draco"):
        eng.mesh_chunk_encoded(vol, encoding='draco')
    with pytest.raises(RuntimeError, match="non-finite shift"):
        eng.mesh_chunk_encoded(vol, shift=(0, np.inf, 0))
    with pytest.raises(RuntimeError, match="q_bits 40"):
        eng.mesh_chunk_encoded(vol, encoding='draco', draco=dict(
            quantization_bits=40, quantization_range=10.0,
            quantization_origin=(0, 0, 0)))
    assert len(eng.mesh_chunk_encoded(vol)) > 3


# ----------------------------------------------------------------- end to end
def _files(layer_path):
    root = layer_path[len("file://"):]
    out = {}
    for dirpath, _dirs, names in os.walk(root):
        for name in names:
            full = os.path.join(dirpath, name)
            with open(full, "rb") as f:
                raw = f.read()
            if raw[:2] == b"\x1f\x8b":      # the header carries the time
                raw = gzip.decompress(raw)
            out[os.path.relpath(full, root)] = raw
    return out


E2E = {
    "precomputed_manifests": dict(generate_manifests=True),
    "draco": dict(encoding='draco'),
    "sharded_spatial": dict(sharded=True, spatial_index=True),
}


@pytest.mark.parametrize("case", list(E2E))
def test_mesh_task_end_to_end(tmp_path, case):
    """MeshTask on a 64^3 layer through the real engine, against the same
    task with the engine behind a plain function that has the handles_*
    attributes but no encode_chunk (the host loop)."""
    from igneous_amd import MeshTask, PrecomputedVolume, engine
    from igneous_amd.synth import voronoi_labels
    from igneous_amd.tasks import mesh as mesh_mod

    data = voronoi_labels((64, 64, 64), 40, 21, dtype=np.uint64, cache=False)
    calls = []

    def host_loop_mesher(*a, **kw):
        calls.append("mesh")
        return engine.mesh_chunk(*a, **kw)
    host_loop_mesher.handles_dust = True
    host_loop_mesher.handles_label_map = True
    host_loop_mesher.handles_fill_holes = True

    def counting(*a, **kw):
        calls.append("encoded")
        return engine.mesh_chunk_encoded(*a, **kw)

    def engine_mesher(*a, **kw):
        return engine.mesh_chunk(*a, **kw)
    engine_mesher.handles_dust = True
    engine_mesher.handles_label_map = True
    engine_mesher.handles_fill_holes = True
    engine_mesher.encode_chunk = counting

    results = {}
    try:
        for sub, mesher in (("host", host_loop_mesher),
                            ("device", engine_mesher)):
            path = f"file://{tmp_path}/{sub}"
            PrecomputedVolume.from_numpy(
                data, path, resolution=(16, 16, 40),
                voxel_offset=(128, 64, 32), chunk_size=(64, 64, 64),
                mesh_dir="mesh")
            mesh_mod.set_mesher(mesher)
            MeshTask(shape=(64, 64, 64), offset=(128, 64, 32),
                     layer_path=path, mip=0, simplification_factor=4,
                     dust_threshold=50, **E2E[case]).execute()
            results[sub] = _files(path)
    finally:
        mesh_mod.set_mesher(None)
    assert calls == ["mesh", "encoded"]
    assert sorted(results["device"]) == sorted(results["host"])
    assert len([n for n in results["host"] if n.startswith("mesh/")]) >= 1
    for name, want in results["host"].items():
        assert results["device"][name] == want, name


@pytest.mark.parametrize("encoding", ("precomputed", "draco"))
def test_product_mesher_hands_over_its_listed_formats(tmp_path, monkeypatch,
                                                      encoding):
    """The default mesher (no set_mesher): MeshTask calls its encode_chunk
    exactly for the encodings encode_chunk.formats lists."""
    from igneous_amd import MeshTask, PrecomputedVolume, engine
    assert engine.mesh_chunk.encode_chunk is engine.mesh_chunk_encoded
    calls = []

    def counting(*a, **kw):
        calls.append(kw["encoding"])
        return engine.mesh_chunk_encoded(*a, **kw)
    counting.formats = engine.mesh_chunk_encoded.formats
    monkeypatch.setattr(engine.mesh_chunk, "encode_chunk", counting)
    path = f"file://{tmp_path}/layer"
    PrecomputedVolume.from_numpy(
        np.ascontiguousarray(_odd()), path, resolution=(16, 16, 40),
        chunk_size=(33, 20, 17), mesh_dir="mesh")
    MeshTask(shape=(33, 20, 17), offset=(0, 0, 0), layer_path=path, mip=0,
             simplification_factor=0, encoding=encoding).execute()
    assert calls == ([encoding] if encoding in counting.formats else [])
    assert len([n for n in _files(path) if n.startswith("mesh/")]) == 6
