"""ctypes host over libmeshgine.so — the MI355X product compute path.

This is the only mesher the product path uses. If the HIP extension is
missing, fails to load, or no GPU is present, every compute call raises
loudly — there is NO CPU fallback (the CPU oracle under oracle/ is test
infrastructure and must never be routed here).

C ABI: include/meshgine.h. Built by __graft_entry__.build() into
igneous_amd/csrc/libmeshgine.so (in-tree so it travels to GPU hosts).
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import NamedTuple, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "csrc", "libmeshgine.so")

MG_U32, MG_U64 = 0, 1
MG_FLAG_DEVICE_ONLY = 1
MG_FLAG_SKIP_H2D = 2
# the volume is the one the mg_count_voxels call just before left resident
MG_FLAG_COUNTED = 4
# mesh_chunk_checked's code for a MG_FLAG_COUNTED call without that volume
MG_ERR_NOT_COUNTED = 9
MG_MAP_MISS_KEEP, MG_MAP_MISS_ZERO = 0, 1
# mg_mesh_chunk_mapped's table cap: larger folds preprocess on the host
LABEL_MAP_MAX_ENTRIES = 1 << 24
# tables up to this many entries are probed from an LDS copy instead of
# L2 (MAP_LDS_MAX_ENTRIES in csrc/meshgine.hip; tests straddle it)
LABEL_MAP_LDS_MAX = 2048

_EXPORTED_SYMBOLS = [
    "mg_init", "mg_destroy", "mg_mesh_chunk", "mg_mesh_chunk_mapped",
    "mg_mesh_chunk_filled", "mg_mesh_holes", "mg_fill_holes",
    "mg_simplify_mesh", "mg_chunk_mesh", "mg_meshset_free",
    "mg_get_stats", "mg_last_error", "mg_device_count", "mg_version",
    "mg_mesh_chunk_encoded", "mg_blobset_free",
    "mg_count_voxels", "mg_label_counts_free",
    "mg_merge_close_vertices", "mg_retriangulate_mesh",
    "mg_encode_octree_level", "mg_fragset_free",
]
MG_ENC_PRECOMPUTED, MG_ENC_DRACO = 0, 1


class _MgMesh(ctypes.Structure):
    _fields_ = [
        ("label", ctypes.c_uint64),
        ("nverts", ctypes.c_uint32),
        ("ntris", ctypes.c_uint32),
        ("verts", ctypes.POINTER(ctypes.c_float)),
        ("faces", ctypes.POINTER(ctypes.c_uint32)),
    ]


class _MgMeshSet(ctypes.Structure):
    _fields_ = [
        ("nmeshes", ctypes.c_uint32),
        ("meshes", ctypes.POINTER(_MgMesh)),
        ("verts_base", ctypes.POINTER(ctypes.c_float)),
        ("faces_base", ctypes.POINTER(ctypes.c_uint32)),
        ("total_verts", ctypes.c_uint64),
        ("total_tris", ctypes.c_uint64),
        ("labels_arr", ctypes.POINTER(ctypes.c_uint64)),
        ("voff_arr", ctypes.POINTER(ctypes.c_uint32)),
        ("nv_arr", ctypes.POINTER(ctypes.c_uint32)),
        ("foff_arr", ctypes.POINTER(ctypes.c_uint32)),
        ("nf_arr", ctypes.POINTER(ctypes.c_uint32)),
    ]


class _MgLabelMap(ctypes.Structure):
    _fields_ = [
        ("keys", ctypes.c_void_p),
        ("vals", ctypes.c_void_p),
        ("n", ctypes.c_uint64),
        ("miss", ctypes.c_uint32),
    ]


class MgStats(ctypes.Structure):
    _fields_ = [
        ("ms_h2d", ctypes.c_double),
        ("ms_count", ctypes.c_double),
        ("ms_scan", ctypes.c_double),
        ("ms_emit", ctypes.c_double),
        ("ms_partition", ctypes.c_double),
        ("ms_weld", ctypes.c_double),
        ("ms_simplify", ctypes.c_double),
        ("ms_d2h", ctypes.c_double),
        ("ms_total", ctypes.c_double),
        ("total_tris", ctypes.c_uint64),
        ("total_verts", ctypes.c_uint64),
        ("n_labels", ctypes.c_uint64),
        ("bytes_read_algorithmic", ctypes.c_uint64),
        ("ms_labelmap", ctypes.c_double),
    ]

    def as_dict(self) -> dict:
        out = {}
        for klass in reversed(type(self).__mro__):
            for name, _t in klass.__dict__.get("_fields_", ()):
                out[name] = getattr(self, name)
        return out


class MgStatsFill(MgStats):
    """mg_stats as the engine writes it now: the MgStats prefix plus the
    fields appended after it (a ctypes subclass lays its own fields out
    behind the base's, which is how the C struct grew)."""
    _fields_ = [
        ("ms_fill", ctypes.c_double),
    ]


class MgStatsEncode(MgStatsFill):
    """... and ms_encode behind ms_fill (mg_mesh_chunk_encoded)."""
    _fields_ = [
        ("ms_encode", ctypes.c_double),
    ]


class MgStatsWeld(MgStatsEncode):
    """... and the weld's path counters behind ms_encode: labels welded
    through a per-label LDS table, labels above weld_lds_cap vertices
    (global table), and that cap."""
    _fields_ = [
        ("weld_lds_labels", ctypes.c_uint64),
        ("weld_table_labels", ctypes.c_uint64),
        ("weld_lds_cap", ctypes.c_uint64),
    ]


class _MgEncodeParams(ctypes.Structure):
    _fields_ = [
        ("format", ctypes.c_uint32),
        ("shift", ctypes.c_float * 3),
        ("q_origin", ctypes.c_double * 3),
        ("q_range", ctypes.c_double),
        ("q_bits", ctypes.c_uint32),
    ]


class _MgBlobSet(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint32),
        ("labels", ctypes.POINTER(ctypes.c_uint64)),
        ("offset", ctypes.POINTER(ctypes.c_uint64)),
        ("size", ctypes.POINTER(ctypes.c_uint64)),
        ("nverts", ctypes.POINTER(ctypes.c_uint32)),
        ("ntris", ctypes.POINTER(ctypes.c_uint32)),
        ("bbox", ctypes.POINTER(ctypes.c_float)),
        ("blob", ctypes.POINTER(ctypes.c_uint8)),
        ("blob_bytes", ctypes.c_uint64),
    ]


# mg_octree_level.order_cells: (nodes[3n] in dict order, n, order[n], arg)
_ORDER_CELLS_FN = ctypes.CFUNCTYPE(
    ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_uint32,
    ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p)


class _MgOctreeLevel(ctypes.Structure):
    _fields_ = [
        ("scale", ctypes.c_double * 3),
        ("offset", ctypes.c_double * 3),
        ("retriangulate", ctypes.c_uint32),
        ("upper_scale", ctypes.c_double * 3),
        ("radius", ctypes.c_double),
        ("chunked", ctypes.c_uint32),
        ("q_origin", ctypes.c_double * 3),
        ("q_voffset", ctypes.c_double * 3),
        ("q_cell", ctypes.c_double * 3),
        ("q_bits", ctypes.c_uint32),
        ("order_cells", _ORDER_CELLS_FN),
        ("order_arg", ctypes.c_void_p),
    ]


class _MgFragSet(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint32),
        ("nodes", ctypes.POINTER(ctypes.c_int32)),
        ("offset", ctypes.POINTER(ctypes.c_uint64)),
        ("size", ctypes.POINTER(ctypes.c_uint64)),
        ("nverts", ctypes.POINTER(ctypes.c_uint32)),
        ("ntris", ctypes.POINTER(ctypes.c_uint32)),
        ("blob", ctypes.POINTER(ctypes.c_uint8)),
        ("blob_bytes", ctypes.c_uint64),
    ]


class EncodedLevel(NamedTuple):
    """The finished fragments of one octree level (mg_fragset), in z-order:
    each fragment's node, its byte size, and the fragments back to back."""
    nodes: tuple
    sizes: list
    blob: bytes


@_ORDER_CELLS_FN
def _order_cells(nodes, n, order, _arg):
    """mg_octree_level.order_cells: the host sequence's own sort, for grids
    with cells of both signs on one axis, where cmp_zorder is no total order
    and only the same sort of the same sequence gives the same result."""
    try:
        import functools
        from .tasks.multires import cmp_zorder
        keys = [tuple(nodes[3 * i:3 * i + 3]) for i in range(n)]
        ranked = sorted(range(n), key=functools.cmp_to_key(
            lambda a, b: cmp_zorder(keys[a], keys[b])))
        for r, i in enumerate(ranked):
            order[r] = i
        return 0
    except Exception:  # an exception cannot cross the C frame
        return 1


class _MgLabelCounts(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("labels", ctypes.POINTER(ctypes.c_uint64)),
        ("counts", ctypes.POINTER(ctypes.c_uint64)),
    ]


class EncodedChunk:
    """Every label's finished fragment of one chunk (mg_blobset): the
    bytes MeshTask uploads and the box its spatial index stores.

    labels (ascending u64), offsets / sizes (u64, into blob), nverts /
    ntris (u32) and bboxes (n x 6 f32: min x, y, z, max x, y, z) are
    parallel arrays; blob is one uint8 array. len() is the number of
    labels, chunk[label] that label's bytes (KeyError if absent),
    chunk.bbox(label) its box, items() yields (label, bytes, box) in
    ascending label order. The bytes objects own their storage; blob
    itself may be a view of the engine's staging (copy=False), valid
    until the next call on that Engine."""

    def __init__(self, labels, offsets, sizes, nverts, ntris, bboxes, blob):
        self.labels = np.asarray(labels, dtype=np.uint64)
        self.offsets = np.asarray(offsets, dtype=np.uint64)
        self.sizes = np.asarray(sizes, dtype=np.uint64)
        self.nverts = np.asarray(nverts, dtype=np.uint32)
        self.ntris = np.asarray(ntris, dtype=np.uint32)
        self.bboxes = np.asarray(bboxes, dtype=np.float32).reshape(-1, 6)
        self.blob = np.asarray(blob, dtype=np.uint8)
        n = self.labels.shape[0]
        for name in ("offsets", "sizes", "nverts", "ntris", "bboxes"):
            if getattr(self, name).shape[0] != n:
                raise ValueError(f"EncodedChunk: {name} does not have one "
                                 f"entry per label")
        if n and np.any(self.labels[1:] <= self.labels[:-1]):
            raise ValueError("EncodedChunk: labels must be ascending")
        if n and int((self.offsets + self.sizes).max()) > self.blob.shape[0]:
            raise ValueError("EncodedChunk: an entry ends past the blob")

    def __len__(self) -> int:
        return int(self.labels.shape[0])

    def _index(self, label) -> int:
        label = int(label)
        if 0 <= label < (1 << 64):
            i = int(np.searchsorted(self.labels, np.uint64(label)))
            if i < len(self) and int(self.labels[i]) == label:
                return i
        raise KeyError(label)

    def __contains__(self, label) -> bool:
        try:
            self._index(label)
        except KeyError:
            return False
        return True

    def _bytes(self, i: int) -> bytes:
        o = int(self.offsets[i])
        return self.blob[o:o + int(self.sizes[i])].tobytes()

    def __getitem__(self, label) -> bytes:
        return self._bytes(self._index(label))

    def bbox(self, label) -> list:
        return self.bboxes[self._index(label)].tolist()

    def items(self):
        boxes = self.bboxes.tolist()
        for i, label in enumerate(self.labels.tolist()):
            yield label, self._bytes(i), boxes[i]


def _draco_numbers(draco):
    """(origin[3], range, bits) as formats.draco.encode's float path ends
    up using them — its own defaulting applied, so the device sees final
    numbers. Per-mesh defaults (origin / range from each mesh's own
    extent) are not a per-chunk setting and are refused."""
    if draco is None:
        raise ValueError("encoding='draco' needs the draco settings "
                         "(quantization_bits / _range / _origin)")
    if draco.get("quantization_origin") is None \
            or draco.get("quantization_range") is None:
        raise ValueError("draco: quantization_origin and quantization_range "
                         "must be given (MeshTask's draco_encoding_settings "
                         "always sets them)")
    origin = np.asarray(draco["quantization_origin"], dtype=np.float64)
    if origin.shape != (3,):
        raise ValueError("draco: quantization_origin must have 3 components")
    rng = float(np.max(draco["quantization_range"]))
    if rng <= 0:
        rng = 1.0
    bits = int(draco.get("quantization_bits", 14))
    return [float(x) for x in origin], rng, bits


# The arguments every mg_mesh_chunk* function starts with (ctx, labels,
# sx, sy, sz, dtype, rx, ry, rz, reduction_factor, max_error,
# voxel_centered, dust_threshold, flags: Engine._chunk_args builds them) ...
_CHUNK_ARGTYPES = [
    ctypes.c_void_p, ctypes.c_void_p,
    ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
    ctypes.c_float, ctypes.c_float, ctypes.c_float,
    ctypes.c_uint32, ctypes.c_float, ctypes.c_int,
    ctypes.c_uint64, ctypes.c_uint32,
]
# ... and what each of the four adds behind them
_P_MAP = ctypes.POINTER(_MgLabelMap)
_PP_MESHSET = ctypes.POINTER(ctypes.POINTER(_MgMeshSet))
_CHUNK_TAIL_ARGTYPES = {
    "mg_mesh_chunk": [_PP_MESHSET],
    "mg_mesh_chunk_mapped": [_P_MAP, _PP_MESHSET],
    "mg_mesh_chunk_filled": [_P_MAP, ctypes.c_uint32, _PP_MESHSET],
    "mg_mesh_chunk_encoded": [_P_MAP, ctypes.POINTER(_MgEncodeParams),
                              ctypes.POINTER(ctypes.POINTER(_MgBlobSet))],
}

_lib = None
_lib_lock = threading.Lock()


def load_library() -> ctypes.CDLL:
    """dlopen the engine; raises with a clear message if absent."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                f"meshgine HIP engine not built: {SO_PATH} missing. "
                f"Run __graft_entry__.build() (hipcc --offload-arch=gfx950). "
                f"There is no CPU fallback.")
        lib = ctypes.CDLL(SO_PATH)
        for sym in _EXPORTED_SYMBOLS:
            if not hasattr(lib, sym):
                raise RuntimeError(f"{SO_PATH} missing symbol {sym}")
        lib.mg_init.restype = ctypes.c_void_p
        lib.mg_init.argtypes = [ctypes.c_int]
        lib.mg_destroy.argtypes = [ctypes.c_void_p]
        for name, tail in _CHUNK_TAIL_ARGTYPES.items():
            fn = getattr(lib, name)
            fn.restype = ctypes.c_int
            fn.argtypes = _CHUNK_ARGTYPES + tail
        lib.mg_blobset_free.argtypes = [ctypes.POINTER(_MgBlobSet)]
        lib.mg_mesh_holes.restype = ctypes.c_int
        lib.mg_mesh_holes.argtypes = [
            ctypes.c_void_p,
            ctypes.c_float, ctypes.c_float, ctypes.c_float,
            ctypes.c_uint32, ctypes.c_float, ctypes.c_int, ctypes.c_uint32,
            ctypes.POINTER(ctypes.POINTER(_MgMeshSet)),
        ]
        lib.mg_fill_holes.restype = ctypes.c_int
        lib.mg_fill_holes.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.POINTER(ctypes.c_uint32),
        ]
        lib.mg_meshset_free.argtypes = [ctypes.POINTER(_MgMeshSet)]
        lib.mg_count_voxels.restype = ctypes.c_int
        lib.mg_count_voxels.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_uint32,
            ctypes.POINTER(ctypes.POINTER(_MgLabelCounts)),
        ]
        lib.mg_label_counts_free.argtypes = [ctypes.POINTER(_MgLabelCounts)]
        lib.mg_get_stats.restype = ctypes.c_int
        lib.mg_get_stats.argtypes = [ctypes.c_void_p,
                                     ctypes.POINTER(MgStatsWeld)]
        lib.mg_last_error.restype = ctypes.c_char_p
        lib.mg_last_error.argtypes = [ctypes.c_void_p]
        lib.mg_device_count.restype = ctypes.c_int
        lib.mg_version.restype = ctypes.c_char_p
        lib.mg_simplify_mesh.restype = ctypes.c_int
        lib.mg_simplify_mesh.argtypes = [
            ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_uint32,
            ctypes.c_void_p, ctypes.c_uint32,
            ctypes.c_uint32, ctypes.c_float,
            ctypes.POINTER(ctypes.POINTER(ctypes.c_float)),
            ctypes.POINTER(ctypes.c_uint32),
            ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32)),
            ctypes.POINTER(ctypes.c_uint32),
        ]
        lib.mg_chunk_mesh.restype = ctypes.c_int
        lib.mg_chunk_mesh.argtypes = [
            ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_uint32,
            ctypes.c_void_p, ctypes.c_uint32,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
            ctypes.POINTER(ctypes.POINTER(_MgMeshSet)),
            ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32)),
        ]
        # the four result arguments of mg_simplify_mesh and the two welds
        mesh_out = [
            ctypes.POINTER(ctypes.POINTER(ctypes.c_float)),
            ctypes.POINTER(ctypes.c_uint32),
            ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32)),
            ctypes.POINTER(ctypes.c_uint32),
        ]
        lib.mg_merge_close_vertices.restype = ctypes.c_int
        lib.mg_merge_close_vertices.argtypes = [
            ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_uint32,
            ctypes.c_void_p, ctypes.c_uint32,
            ctypes.c_double,
        ] + mesh_out
        lib.mg_retriangulate_mesh.restype = ctypes.c_int
        lib.mg_retriangulate_mesh.argtypes = [
            ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_uint32,
            ctypes.c_void_p, ctypes.c_uint32,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
            ctypes.c_double,
        ] + mesh_out
        lib.mg_encode_octree_level.restype = ctypes.c_int
        lib.mg_encode_octree_level.argtypes = [
            ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_uint32,
            ctypes.c_void_p, ctypes.c_uint32,
            ctypes.POINTER(_MgOctreeLevel),
            ctypes.POINTER(ctypes.POINTER(_MgFragSet)),
        ]
        lib.mg_fragset_free.argtypes = [ctypes.POINTER(_MgFragSet)]
        _lib = lib
        return lib


def _mg_dtype(arr: np.ndarray) -> int:
    """MG_U32 / MG_U64 for a label array."""
    if arr.dtype == np.uint32:
        return MG_U32
    if arr.dtype == np.uint64:
        return MG_U64
    raise ValueError(f"unsupported label dtype {arr.dtype}")


def _np_array(ptr, n: int, width=None, copy: bool = False) -> np.ndarray:
    """n elements (n rows of `width`) behind a typed ctypes pointer as a
    numpy array: a view of that memory, or a copy. n == 0 never reads ptr."""
    shape = (n,) if width is None else (n, width)
    if not n:
        return np.zeros(shape, dtype=ptr._type_)
    arr = np.ctypeslib.as_array(ptr, shape=shape)
    return arr.copy() if copy else arr


def _engine(device_id: Optional[int]) -> "Engine":
    """The shared Engine of the module-level calls: on device_id, else on
    MESHGINE_DEVICE, else on LOCAL_RANK."""
    if device_id is None:
        device_id = int(os.environ.get("MESHGINE_DEVICE",
                                       os.environ.get("LOCAL_RANK", "0")))
    return Engine.get(device_id)


def _check_dust_global(dust_global, dust_threshold, skip_h2d) -> None:
    if dust_global is None:
        return
    if dust_threshold:
        raise ValueError(
            "dust_global (the global threshold) cannot be combined with "
            "dust_threshold (the chunk-local one)")
    if skip_h2d:
        raise ValueError(
            "dust_global cannot be combined with skip_h2d: it counts and "
            "meshes the volume it is given")
    threshold, lookup = dust_global
    if int(threshold) < 0 or not callable(lookup):
        raise ValueError("dust_global: expected (threshold >= 0, lookup)")


def _fill_level_unsupported(what: str) -> NotImplementedError:
    return NotImplementedError(
        f"{what}: the engine implements levels "
        f"1-2; level 3 needs a multilabel dilation and levels >= 4 "
        f"a merge threshold")


# When True, Engine.get() returns one context (and HIP stream) per
# (device, thread): concurrent MeshTasks on one GPU overlap their
# H2D / kernels / D2H — the reference's "one HIP stream per in-flight
# chunk" fan-out. Set by igneous_amd.dispatch.
PER_THREAD_CTX = False


class Engine:
    """One mg_ctx on one HIP device."""

    _per_device: dict = {}
    _cls_lock = threading.Lock()

    def __init__(self, device_id: int = 0):
        lib = load_library()
        self.lib = lib
        self.device_id = int(device_id)
        self._lock = threading.Lock()
        # mg_stats of the last fill_holes meshing's FIRST call (the hole
        # meshing that follows overwrites the ctx's stats)
        self.last_fill_stats = None
        self.ctx = lib.mg_init(self.device_id)
        if not self.ctx:
            raise RuntimeError(
                f"mg_init({device_id}) failed — no usable HIP device. "
                f"The meshgine product path requires an MI355X GPU.")

    @classmethod
    def get(cls, device_id: int = 0) -> "Engine":
        key = (device_id, threading.get_ident()) if PER_THREAD_CTX \
            else device_id
        with cls._cls_lock:
            eng = cls._per_device.get(key)
            if eng is None:
                eng = cls(device_id)
                cls._per_device[key] = eng
            return eng

    def _check(self, rc: int, fn: str) -> None:
        """Raise the ctx's last error if the C call `fn` returned non-zero."""
        if rc != 0:
            err = self.lib.mg_last_error(self.ctx)
            raise RuntimeError(
                f"{fn} failed rc={rc}: "
                f"{err.decode() if err else 'unknown'}")

    def mesh_chunk(self, labels: np.ndarray, resolution=(1.0, 1.0, 1.0),
                   reduction_factor: int = 0, max_error: float = 40.0,
                   voxel_centered: bool = True,
                   device_only: bool = False,
                   skip_h2d: bool = False,
                   dust_threshold: int = 0,
                   copy: bool = True,
                   label_map=None,
                   fill_holes: int = 0,
                   dust_global=None):
        """GPU counterpart of oracle.mesh_chunk: F-order (sx,sy,sz)
        uint32/uint64 labels -> {label: (verts (V,3) f32 nm, faces (F,3) u32)},
        labels ascending. Under device_only returns {} (stats still filled).

        label_map=(keys, vals, miss) as produced by remap.fold_label_ops
        (miss 'keep' or 'zero') rewrites the labels ON DEVICE after dust
        and before meshing (mg_mesh_chunk_mapped); the host array is not
        touched. It cannot be combined with skip_h2d: the resident volume
        is already mapped.

        copy=False returns VIEWS into this context's pinned staging
        buffers — zero host copies, but the arrays are only valid until
        the next mesh_chunk on this Engine. Use when results are consumed
        (encoded/written) before the next call, as MeshTask does.

        fill_holes=1|2 fills holes ON DEVICE after dust and the label map
        (mg_mesh_chunk_filled, contract in DESIGN.md §7) and returns the
        PAIR (filled_meshes, hole_meshes): the meshes of the filled volume
        and of the hole volume (mg_mesh_holes, no second upload). Both
        dicts own their storage whatever `copy` says — the second meshing
        reuses the first one's staging. Not combinable with skip_h2d.

        dust_global=(threshold, lookup) erases every label whose GLOBAL
        voxel count lookup(labels_u64) -> counts_u64 (a host callable, e.g.
        formats.intmap.IntMap.lookup of the voxel_counts.im sidecar) is
        below threshold — the reference's apply_dust_global_threshold
        (mesh.py:324-355). The chunk's labels come from count_voxels; the
        dust labels are folded into the label map (dust first, on the raw
        labels, then the map) and the chunk call meshes the volume the
        count left resident. Not combinable with dust_threshold (the local
        threshold) or skip_h2d."""
        fill_holes = int(fill_holes)
        if fill_holes < 0 or fill_holes > 2:
            raise _fill_level_unsupported(f"fill_holes={fill_holes}")
        if fill_holes and skip_h2d:
            raise ValueError(
                "fill_holes cannot be combined with skip_h2d: the "
                "resident volume has already been filled")
        if fill_holes:
            copy = True
        _check_dust_global(dust_global, dust_threshold, skip_h2d)
        labels = np.asfortranarray(labels)
        # one hold of the lock from the count to the chunk call: no other
        # thread of this ctx can drop the counted volume in between
        with self._lock:
            if dust_global is not None:
                label_map = self._fold_global_dust(
                    labels, dust_global, label_map)
            args, cmap, _keep = self._chunk_args(
                labels, resolution, reduction_factor, max_error,
                voxel_centered, dust_threshold, device_only, skip_h2d,
                label_map, counted=dust_global is not None)
            # the narrowest entry point that takes what was asked for
            if fill_holes:
                fn, tail = "mg_mesh_chunk_filled", (cmap, fill_holes)
            elif cmap is not None:
                fn, tail = "mg_mesh_chunk_mapped", (cmap,)
            else:
                fn, tail = "mg_mesh_chunk", ()
            out = ctypes.POINTER(_MgMeshSet)()
            rc = getattr(self.lib, fn)(*args, *tail, ctypes.byref(out))
            self._check(rc, fn)
            result = self._collect(out, copy)
            if not fill_holes:
                return result
            self.last_fill_stats = self.stats()
            out = ctypes.POINTER(_MgMeshSet)()
            rc = self.lib.mg_mesh_holes(  # resolution .. voxel_centered, flags
                self.ctx, *args[6:12],
                MG_FLAG_DEVICE_ONLY if device_only else 0, ctypes.byref(out))
            self._check(rc, "mg_mesh_holes")
            return result, self._collect(out, True)

    def _count_locked(self, labels, skip_h2d: bool = False):
        """mg_count_voxels of an F-order volume -> (values, counts); the
        caller holds self._lock."""
        dtype = _mg_dtype(labels)
        if labels.ndim != 3:
            raise ValueError("count_voxels expects a 3-D volume")
        sx, sy, sz = labels.shape
        out = ctypes.POINTER(_MgLabelCounts)()
        rc = self.lib.mg_count_voxels(
            self.ctx, labels.ctypes.data_as(ctypes.c_void_p),
            sx, sy, sz, dtype, MG_FLAG_SKIP_H2D if skip_h2d else 0,
            ctypes.byref(out))
        self._check(rc, "mg_count_voxels")
        try:
            n = int(out.contents.n)
            return (_np_array(out.contents.labels, n, copy=True),
                    _np_array(out.contents.counts, n, copy=True))
        finally:
            self.lib.mg_label_counts_free(out)

    def count_voxels(self, labels: np.ndarray, skip_h2d: bool = False):
        """Every distinct value of an F-order uint32/uint64 volume and its
        voxel count on the GPU (mg_count_voxels; fastremap.unique(labels,
        return_counts=True) of the reference's CountVoxelsTask)
        -> (values u64[n] ascending, 0 included when present, counts
        u64[n])."""
        labels = np.asfortranarray(labels)
        with self._lock:
            return self._count_locked(labels, skip_h2d)

    def _fold_global_dust(self, labels, dust_global, label_map):
        """Count the chunk (the raw volume stays resident), look its labels
        up in the global table and fold the ones below the threshold into
        label_map. The caller holds self._lock through the chunk call."""
        from .remap import fold_dust
        threshold, lookup = dust_global
        values, _ = self._count_locked(labels)
        values = values[values != 0]
        totals = np.asarray(lookup(values), dtype=np.uint64)
        if totals.shape != values.shape:
            raise ValueError("dust_global: lookup must return one count "
                             "per label")
        return fold_dust(label_map, values[totals < np.uint64(threshold)],
                         labels.dtype)

    def _chunk_args(self, labels, resolution, reduction_factor, max_error,
                    voxel_centered, dust_threshold, device_only, skip_h2d,
                    label_map, counted: bool = False):
        """The one marshalling of a chunk call: (the _CHUNK_ARGTYPES
        arguments, a reference to the mg_label_map or None, the arrays the
        two point into — the caller holds them until the call returns).
        counted: the call follows this volume's mg_count_voxels
        (MG_FLAG_COUNTED)."""
        labels = np.asfortranarray(labels)
        dtype = _mg_dtype(labels)
        sx, sy, sz = labels.shape
        flags = (MG_FLAG_DEVICE_ONLY if device_only else 0) | \
                (MG_FLAG_SKIP_H2D if skip_h2d else 0) | \
                (MG_FLAG_COUNTED if counted else 0)
        args = (
            self.ctx, labels.ctypes.data_as(ctypes.c_void_p),
            sx, sy, sz, dtype,
            float(resolution[0]), float(resolution[1]), float(resolution[2]),
            int(reduction_factor), float(max_error),
            int(bool(voxel_centered)), int(dust_threshold), flags)
        if label_map is None:
            return args, None, (labels,)
        if skip_h2d:
            raise ValueError(
                "label_map cannot be combined with skip_h2d: the "
                "resident volume has already been mapped")
        keys, vals, miss = label_map
        if miss not in ('keep', 'zero'):
            raise ValueError(f"label_map miss policy {miss!r}: "
                             f"expected 'keep' or 'zero'")
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        if keys.ndim != 1 or keys.shape != vals.shape:
            raise ValueError("label_map keys/vals must be 1-D arrays "
                             "of equal length")
        cmap = _MgLabelMap(
            keys.ctypes.data, vals.ctypes.data, keys.shape[0],
            MG_MAP_MISS_ZERO if miss == 'zero' else MG_MAP_MISS_KEEP)
        return args, ctypes.byref(cmap), (labels, keys, vals, cmap)

    def mesh_chunk_encoded(self, labels: np.ndarray,
                           resolution=(1.0, 1.0, 1.0),
                           reduction_factor: int = 0,
                           max_error: float = 40.0,
                           voxel_centered: bool = True,
                           dust_threshold: int = 0,
                           label_map=None,
                           shift=(0.0, 0.0, 0.0),
                           encoding: str = 'precomputed',
                           draco=None,
                           device_only: bool = False,
                           copy: bool = True,
                           skip_h2d: bool = False,
                           dust_global=None) -> EncodedChunk:
        """mesh_chunk, ending in every label's finished fragment instead
        of its mesh (mg_mesh_chunk_encoded): for each label, the bytes and
        box MeshTask's host loop makes from mesh_chunk's result for the
        same arguments — vertices + shift (three f32), their min/max, and
        Mesh.to_precomputed() or formats.draco.encode(**draco) — computed
        on the device, byte for byte.

        encoding='draco' takes draco = the settings dict of
        tasks.draco.draco_encoding_settings (quantization_bits / _range /
        _origin; other keys are ignored, as the encoder ignores them).
        copy=False leaves the blob a view of this context's pinned
        staging, valid until the next call on this Engine. Under
        device_only the set is empty (stats still filled).
        dust_global=(threshold, lookup): as in mesh_chunk."""
        if encoding not in ('precomputed', 'draco'):
            raise ValueError(f"encoding {encoding!r}: expected "
                             f"'precomputed' or 'draco'")
        params = _MgEncodeParams()
        params.format = (MG_ENC_DRACO if encoding == 'draco'
                         else MG_ENC_PRECOMPUTED)
        shift = np.asarray(shift, dtype=np.float32).reshape(3)
        params.shift[:] = [float(x) for x in shift]
        if encoding == 'draco':
            origin, rng, bits = _draco_numbers(draco)
            params.q_origin[:] = origin
            params.q_range = rng
            if not 0 <= bits < (1 << 32):
                raise ValueError(f"draco: quantization_bits {bits}")
            params.q_bits = bits
        _check_dust_global(dust_global, dust_threshold, skip_h2d)
        labels = np.asfortranarray(labels)
        with self._lock:
            if dust_global is not None:
                label_map = self._fold_global_dust(
                    labels, dust_global, label_map)
            args, cmap, _keep = self._chunk_args(
                labels, resolution, reduction_factor, max_error,
                voxel_centered, dust_threshold, device_only, skip_h2d,
                label_map, counted=dust_global is not None)
            out = ctypes.POINTER(_MgBlobSet)()
            rc = self.lib.mg_mesh_chunk_encoded(
                *args, cmap, ctypes.byref(params), ctypes.byref(out))
            self._check(rc, "mg_mesh_chunk_encoded")
            try:
                bs = out.contents
                n = int(bs.n)
                return EncodedChunk(
                    *(_np_array(p, n, copy=True) for p in (
                        bs.labels, bs.offset, bs.size, bs.nverts, bs.ntris)),
                    _np_array(bs.bbox, n, 6, copy=True),
                    _np_array(bs.blob, int(bs.blob_bytes), copy=copy))
            finally:
                self.lib.mg_blobset_free(out)

    def _collect(self, out, copy: bool) -> dict:
        """Meshset descriptor -> {label: (verts, faces)}; frees it."""
        result = {}
        try:
            ms = out.contents
            n = int(ms.nmeshes)
            if n:
                # one GIL-releasing memmove per flat buffer (the flat
                # buffers are ctx-owned pinned staging, valid until
                # the next call on this ctx), then per-label views
                tv, tt = int(ms.total_verts), int(ms.total_tris)
                if copy:
                    all_v = np.empty((tv, 3), dtype=np.float32)
                    all_f = np.empty((tt, 3), dtype=np.uint32)
                    if tv:
                        ctypes.memmove(all_v.ctypes.data, ms.verts_base,
                                       tv * 12)
                    if tt:
                        ctypes.memmove(all_f.ctypes.data, ms.faces_base,
                                       tt * 12)
                else:
                    all_v = np.ctypeslib.as_array(
                        ms.verts_base, shape=(max(tv, 1), 3))[:tv]
                    all_f = np.ctypeslib.as_array(
                        ms.faces_base, shape=(max(tt, 1), 3))[:tt]
                tables = (_np_array(p, n).tolist() for p in (
                    ms.labels_arr, ms.voff_arr, ms.nv_arr, ms.foff_arr,
                    ms.nf_arr))
                result = {
                    lab: (all_v[vo:vo + kv], all_f[fo:fo + kf])
                    for lab, vo, kv, fo, kf in zip(*tables)
                }
        finally:
            self.lib.mg_meshset_free(out)
        return result

    def fill_holes(self, labels: np.ndarray, level: int = 1):
        """Hole filling of one F-order uint32/uint64 volume on the GPU
        (mg_fill_holes; the fastmorph.fill_holes_v2 replacement of
        mesh.py:220 for levels 1-2, contract in DESIGN.md §7).
        -> (filled, holes, rounds): the filled volume, the hole volume
        (labels[v] where filled[v] != labels[v], else 0) and the number
        of productive 3-D rounds."""
        level = int(level)
        if level not in (1, 2):
            raise _fill_level_unsupported(f"fill_holes level {level}")
        labels = np.asfortranarray(labels)
        dtype = _mg_dtype(labels)
        if labels.ndim != 3:
            raise ValueError("fill_holes expects a 3-D volume")
        sx, sy, sz = labels.shape
        filled = np.empty(labels.shape, dtype=labels.dtype, order="F")
        holes = np.empty(labels.shape, dtype=labels.dtype, order="F")
        rounds = ctypes.c_uint32()
        with self._lock:
            rc = self.lib.mg_fill_holes(
                self.ctx, labels.ctypes.data_as(ctypes.c_void_p),
                sx, sy, sz, dtype, level,
                filled.ctypes.data_as(ctypes.c_void_p),
                holes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rounds))
            self._check(rc, "mg_fill_holes")
        return filled, holes, int(rounds.value)

    def simplify_mesh(self, verts: np.ndarray, faces: np.ndarray,
                      reduction_factor: int,
                      max_error: float = 1e30):
        """Standalone quadric simplification of one mesh on the GPU
        (mg_simplify_mesh; the multires LOD chain's simplify_fqmr
        replacement, multires.py:342). Returns owned (verts, faces)."""
        v = np.ascontiguousarray(verts, dtype=np.float32)
        f = np.ascontiguousarray(faces, dtype=np.uint32)
        ov = ctypes.POINTER(ctypes.c_float)()
        of = ctypes.POINTER(ctypes.c_uint32)()
        onv = ctypes.c_uint32()
        ont = ctypes.c_uint32()
        # the results are views of the ctx's pinned staging: hold the lock
        # until they are copied, or another thread's call overwrites them
        with self._lock:
            rc = self.lib.mg_simplify_mesh(
                self.ctx,
                v.ctypes.data_as(ctypes.c_void_p), v.shape[0],
                f.ctypes.data_as(ctypes.c_void_p), f.shape[0],
                int(reduction_factor), float(max_error),
                ctypes.byref(ov), ctypes.byref(onv),
                ctypes.byref(of), ctypes.byref(ont))
            self._check(rc, "mg_simplify_mesh")
            out_v = _np_array(ov, onv.value, 3, copy=True)
            out_f = _np_array(of, ont.value, 3, copy=True)
        return out_v, out_f

    def chunk_mesh(self, verts: np.ndarray, faces: np.ndarray,
                   scale, offset) -> dict:
        """Grid-partition one mesh with clipping at the cell boundaries on
        the GPU (mg_chunk_mesh; the zmesh.chunk_mesh replacement of
        multires.py:550,574, bit-equal to meshops.chunk_mesh).
        -> {(cx, cy, cz): (verts, faces)} with owned arrays, in the host
        function's dict order."""
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
        sc = (ctypes.c_double * 3)(*[float(x) for x in scale])
        off = (ctypes.c_double * 3)(*[float(x) for x in offset])
        out = ctypes.POINTER(_MgMeshSet)()
        order = ctypes.POINTER(ctypes.c_uint32)()
        # the meshset aliases the ctx's pinned staging: hold the lock
        # until it is copied out
        with self._lock:
            rc = self.lib.mg_chunk_mesh(
                self.ctx,
                v.ctypes.data_as(ctypes.c_void_p), v.shape[0],
                f.ctypes.data_as(ctypes.c_void_p), f.shape[0],
                sc, off, ctypes.byref(out), ctypes.byref(order))
            self._check(rc, "mg_chunk_mesh")
            n = int(out.contents.nmeshes)
            # read out_order before _collect frees the descriptor
            idx = _np_array(order, n).tolist()
            by_label = self._collect(out, True)
        labels = list(by_label)  # ascending label = meshes[] order
        mask = (1 << 21) - 1
        bias = 1 << 20
        result = {}
        for i in idx:
            lab = labels[i]
            key = (((lab >> 42) & mask) - bias, ((lab >> 21) & mask) - bias,
                   (lab & mask) - bias)
            result[key] = by_label[lab]
        return result

    def _weld_call(self, fn: str, verts, faces, radius, *grid):
        """mg_merge_close_vertices / mg_retriangulate_mesh (grid = its
        scale and offset) -> owned (verts, faces), copied under the lock."""
        radius = float(radius)
        if not np.isfinite(radius) or radius <= 0:
            raise ValueError(f"radius {radius}: must be finite and > 0")
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
        grid = [(ctypes.c_double * 3)(*[float(x) for x in g]) for g in grid]
        ov = ctypes.POINTER(ctypes.c_float)()
        of = ctypes.POINTER(ctypes.c_uint32)()
        onv = ctypes.c_uint32()
        ont = ctypes.c_uint32()
        # the results are views of the ctx's pinned staging: hold the lock
        # until they are copied, or another thread's call overwrites them
        with self._lock:
            rc = getattr(self.lib, fn)(
                self.ctx,
                v.ctypes.data_as(ctypes.c_void_p), v.shape[0],
                f.ctypes.data_as(ctypes.c_void_p), f.shape[0],
                *grid, radius,
                ctypes.byref(ov), ctypes.byref(onv),
                ctypes.byref(of), ctypes.byref(ont))
            self._check(rc, fn)
            if not ov:  # mg_retriangulate_mesh: no cell, the input stands
                return v.copy(), f.copy()
            return (_np_array(ov, onv.value, 3, copy=True),
                    _np_array(of, ont.value, 3, copy=True))

    def merge_close_vertices(self, verts: np.ndarray, faces: np.ndarray,
                             radius: float = 1e-5):
        """Weld the vertices within `radius` of each other on the GPU
        (mg_merge_close_vertices; the Mesh.merge_close_vertices replacement
        of multires.py:551, bit-equal to meshops.merge_close_vertices).
        Returns owned (verts, faces)."""
        return self._weld_call("mg_merge_close_vertices", verts, faces,
                               radius)

    def retriangulate_mesh(self, verts: np.ndarray, faces: np.ndarray,
                           scale, offset, radius: float = 1e-5):
        """Cut one mesh at the grid's cell boundaries and weld the pieces
        on the GPU (mg_retriangulate_mesh; retriangulate_mesh of
        multires.py:546-553): bit-equal to meshops.merge_close_vertices of
        the concatenated meshops.chunk_mesh cells, which never leave the
        device. A mesh the chunker keeps no cell of comes back unchanged.
        Returns owned (verts, faces)."""
        return self._weld_call("mg_retriangulate_mesh", verts, faces, radius,
                               scale, offset)

    def encode_octree_level(self, verts: np.ndarray, faces: np.ndarray, *,
                            scale, offset, upper_scale=None,
                            radius: float = 1e-5, chunked: bool = True,
                            q_origin, q_voffset, q_cell,
                            q_bits: int) -> EncodedLevel:
        """One level of a mesh's multires octree, from the mesh to the
        finished fragment bytes, in one device call
        (mg_encode_octree_level; create_octree_level_from_mesh of
        multires.py:556-585 and the quantise + draco loop of :152-174,
        byte-equal to tasks.multires.encode_octree_level_host).
          scale, offset   this level's grid (chunk_shape * 2^lod, grid_origin)
          upper_scale     not None (lod > 0): retriangulate at that grid first
          chunked         False for the coarsest level: one fragment at
                          (0, 0, 0)
          q_*             to_stored_model_space's numbers; q_cell is the f64
                          product chunk_shape * lod_scale
        The mesh stays on the device between the stages; only the tables
        and the blob come back."""
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
        vec = ctypes.c_double * 3
        lv = _MgOctreeLevel()
        lv.scale = vec(*[float(x) for x in scale])
        lv.offset = vec(*[float(x) for x in offset])
        lv.retriangulate = 0 if upper_scale is None else 1
        lv.upper_scale = vec(*[float(x) for x in (
            scale if upper_scale is None else upper_scale)])
        lv.radius = float(radius)
        lv.chunked = 1 if chunked else 0
        lv.q_origin = vec(*[float(x) for x in q_origin])
        lv.q_voffset = vec(*[float(x) for x in q_voffset])
        lv.q_cell = vec(*[float(x) for x in q_cell])
        q_bits = int(q_bits)
        # out of c_uint32's range is out of 1..32 all the same
        lv.q_bits = q_bits if 0 <= q_bits < 2 ** 32 else 0
        lv.order_cells = _order_cells
        out = ctypes.POINTER(_MgFragSet)()
        # the blob is a view of the ctx's pinned staging: hold the lock
        # until it is copied
        with self._lock:
            rc = self.lib.mg_encode_octree_level(
                self.ctx,
                v.ctypes.data_as(ctypes.c_void_p), v.shape[0],
                f.ctypes.data_as(ctypes.c_void_p), f.shape[0],
                ctypes.byref(lv), ctypes.byref(out))
            self._check(rc, "mg_encode_octree_level")
            try:
                fs = out.contents
                n = int(fs.n)
                nodes = _np_array(fs.nodes, 3 * n).reshape(n, 3).tolist()
                sizes = _np_array(fs.size, n).tolist()
                nbytes = int(fs.blob_bytes)
                blob = ctypes.string_at(fs.blob, nbytes) if nbytes else b""
            finally:
                self.lib.mg_fragset_free(out)
        return EncodedLevel(tuple(tuple(p) for p in nodes), sizes, blob)

    def stats(self) -> dict:
        s = MgStatsWeld()
        rc = self.lib.mg_get_stats(self.ctx, ctypes.byref(s))
        if rc != 0:
            raise RuntimeError("mg_get_stats failed")
        return s.as_dict()


def mesh_chunk(labels: np.ndarray, resolution=(1.0, 1.0, 1.0),
               reduction_factor: int = 0, max_error: float = 40.0,
               voxel_centered: bool = True, device_id: Optional[int] = None,
               dust_threshold: int = 0,
               copy: bool = True, label_map=None, fill_holes: int = 0,
               dust_global=None):
    """Module-level product mesher (the default MeshTask path). With
    fill_holes=1|2 returns the pair (filled_meshes, hole_meshes)."""
    return _engine(device_id).mesh_chunk(
        labels, resolution, reduction_factor, max_error, voxel_centered,
        dust_threshold=dust_threshold, copy=copy, label_map=label_map,
        fill_holes=fill_holes, dust_global=dust_global)


# MeshTask checks this to delegate dust_threshold preprocessing to the
# device (three HIP volume passes) instead of a host numpy unique/mask
mesh_chunk.handles_dust = True
# ... and to hand it remap_table / object_ids / exclude_object_ids folded
# into one label_map (remap.fold_label_ops) instead of the host numpy
# mask_except/remap/mask sequence
mesh_chunk.handles_label_map = True
# ... and fill_holes levels 1-2 (device volume pass after dust and the
# label map; the call then returns (filled_meshes, hole_meshes))
mesh_chunk.handles_fill_holes = True
# ... and dust_global=(threshold, lookup): the chunk's labels are counted on
# the device, looked up in the global voxel counts and the dust folded into
# the label map
mesh_chunk.handles_dust_global = True


def mesh_chunk_encoded(labels: np.ndarray, resolution=(1.0, 1.0, 1.0),
                       reduction_factor: int = 0, max_error: float = 40.0,
                       voxel_centered: bool = True,
                       device_id: Optional[int] = None,
                       dust_threshold: int = 0, label_map=None,
                       shift=(0.0, 0.0, 0.0), encoding: str = 'precomputed',
                       draco=None, copy: bool = True,
                       dust_global=None) -> EncodedChunk:
    """Module-level encoded mesher: see Engine.mesh_chunk_encoded."""
    return _engine(device_id).mesh_chunk_encoded(
        labels, resolution, reduction_factor, max_error, voxel_centered,
        dust_threshold=dust_threshold, label_map=label_map, shift=shift,
        encoding=encoding, draco=draco, copy=copy, dust_global=dust_global)


# ... and that it can return the finished fragments instead of meshes:
# MeshTask calls encode_chunk for a chunk without fill_holes or dry_run and
# skips its per-label shift / box / encode loop. encode_chunk.formats names
# the encodings for which the task takes that path by default: a format is
# listed when the device path beat the host loop by more than three times
# the host loop's own max-min on EVERY row of tools/probe_encode.py
# (DESIGN.md §4). draco did; precomputed missed the margin on one row
# (simplification_factor=100: 31.4 ms gained, 33.8 ms asked), so it keeps
# the host loop until a probe says otherwise. The call itself serves both:
# assign ('precomputed', 'draco') here to hand both over.
mesh_chunk.encode_chunk = mesh_chunk_encoded
mesh_chunk_encoded.formats = ('draco',)


def count_voxels(labels: np.ndarray, device_id: Optional[int] = None):
    """Module-level voxel counter -> (values, counts); see
    Engine.count_voxels."""
    return _engine(device_id).count_voxels(labels)


# CountVoxelsTask and MeshTask's host dust_global path find the counter here
mesh_chunk.count_voxels = count_voxels


def fill_holes(labels: np.ndarray, level: int = 1,
               device_id: Optional[int] = None):
    """Module-level hole filling -> (filled, holes, rounds); see
    Engine.fill_holes."""
    return _engine(device_id).fill_holes(labels, level)


def chunk_mesh(mesh, scale, offset, device_id: Optional[int] = None):
    """Module-level grid chunker (the default multires path): Mesh ->
    {(cx, cy, cz): Mesh}, the shape and order of meshops.chunk_mesh."""
    from .meshes import Mesh
    cells = _engine(device_id).chunk_mesh(
        mesh.vertices, mesh.faces, scale, offset)
    return {key: Mesh(v, f, id=mesh.id) for key, (v, f) in cells.items()}


def merge_close_vertices(mesh, radius: float = 1e-5,
                         device_id: Optional[int] = None):
    """Module-level vertex weld: Mesh -> Mesh, the result of
    meshops.merge_close_vertices."""
    from .meshes import Mesh
    v, f = _engine(device_id).merge_close_vertices(
        mesh.vertices, mesh.faces, radius)
    return Mesh(v, f, id=mesh.id)


def retriangulate_mesh(mesh, scale, offset, radius: float = 1e-5,
                       device_id: Optional[int] = None):
    """Module-level retriangulation (the default multires path): Mesh ->
    Mesh, chunk_mesh + Mesh.concatenate + merge_close_vertices in one
    device call."""
    from .meshes import Mesh
    v, f = _engine(device_id).retriangulate_mesh(
        mesh.vertices, mesh.faces, scale, offset, radius)
    return Mesh(v, f, id=mesh.id)


def encode_octree_level(mesh, *, scale, offset, upper_scale=None,
                        radius: float = 1e-5, chunked: bool = True,
                        q_origin, q_voffset, q_cell, q_bits: int,
                        device_id: Optional[int] = None) -> EncodedLevel:
    """Module-level octree level encoder: Mesh -> EncodedLevel; see
    Engine.encode_octree_level."""
    return _engine(device_id).encode_octree_level(
        mesh.vertices, mesh.faces, scale=scale, offset=offset,
        upper_scale=upper_scale, radius=radius, chunked=chunked,
        q_origin=q_origin, q_voffset=q_voffset, q_cell=q_cell,
        q_bits=q_bits)


def simplify_mesh(mesh, target_count: int, max_error: float = 1e30,
                  device_id: Optional[int] = None):
    """Module-level LOD simplifier: Mesh -> Mesh at ~target_count faces
    (reduction_factor = ntris // target; <=1 returns the mesh as-is)."""
    from .meshes import Mesh
    nt = int(mesh.faces.shape[0])
    target = max(int(target_count), 1)
    if nt <= target:
        return Mesh(mesh.vertices.copy(), mesh.faces.copy(), id=mesh.id)
    rf = max(nt // target, 2)
    v, f = _engine(device_id).simplify_mesh(
        mesh.vertices, mesh.faces, rf, max_error)
    return Mesh(v, f, id=mesh.id)
