"""Checker for the device encode stage (a helper, not a test).

encode_ref restates mg_mesh_chunk_encoded's contract with the host code
itself: every label's mesh goes through tasks.mesh.encode_fragment, the one
function MeshTask's host loop runs per label. encoded_chunk_ref packs that
result into an EncodedChunk, which is how the CPU tests build an
encode_chunk out of the oracle."""
import numpy as np

from igneous_amd.engine import EncodedChunk
from igneous_amd.meshes import Mesh
from igneous_amd.tasks.mesh import encode_fragment


def encode_ref(raw, shift, encoding='precomputed', draco=None):
    """{label: (verts, faces)} -> {label: (bytes, bbox)}, labels ascending.
    The input arrays are left unchanged."""
    shift = np.asarray(shift, dtype=np.float32)
    out = {}
    for label in sorted(int(k) for k in raw):
        verts, faces = raw[label]
        mesh = Mesh(np.array(verts, dtype=np.float32, copy=True),
                    np.array(faces, dtype=np.uint32, copy=True), id=label)
        out[label] = encode_fragment(mesh, shift, encoding, draco)
    return out


def encoded_chunk_ref(raw, shift, encoding='precomputed', draco=None):
    """encode_ref's result as an EncodedChunk (entries back to back)."""
    ref = encode_ref(raw, shift, encoding, draco)
    labels = list(ref)
    sizes = [len(ref[k][0]) for k in labels]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]) if labels else []
    blob = np.frombuffer(b"".join(ref[k][0] for k in labels), dtype=np.uint8)
    return EncodedChunk(
        labels, offsets, sizes,
        [raw[k][0].shape[0] for k in labels],
        [raw[k][1].shape[0] for k in labels],
        np.asarray([ref[k][1] for k in labels],
                   dtype=np.float32).reshape(-1, 6),
        blob)


def assert_encoded_equal(got, ref):
    """got: EncodedChunk; ref: encode_ref's dict. Label arrays identical,
    every label's bytes equal, boxes equal under float ==."""
    assert got.labels.tolist() == list(ref)
    assert len(got) == len(ref)
    n = 0
    for label, binary, box in got.items():
        want_bytes, want_box = ref[label]
        assert binary == want_bytes, (
            f"label {label}: {len(binary)} bytes vs {len(want_bytes)}; first "
            f"difference at byte "
            f"{next((i for i, (a, b) in enumerate(zip(binary, want_bytes)) if a != b), None)}")
        assert box == want_box, f"label {label}: box {box} != {want_box}"
        n += 1
    assert n == len(ref)
