"""IntMap — serializable uint64 -> uint64 map with O(log N) lookup.

Replaces `mapbuffer.IntMap` at the reference call sites:
  - accumulate_voxel_counts writes the global voxel counts as
    `IntMap(final_counts).tobytes()` to $KEY/stats/voxel_counts.im
    (/root/reference/igneous/task_creation/image.py:2015-2030)
  - MeshTask.apply_dust_global_threshold reads them back per label via
    `IntMap(buf)[label]` (/root/reference/igneous/tasks/mesh/mesh.py:345-353)

PARITY NOTE: like MapBuffer (formats/mapbuffer.py), the
mapbuffer package's byte layout cannot be pinned offline. This module is a
documented STAND-IN behind the same API — IntMap(dict), IntMap(bytes),
tobytes(), [], in, len, get, items — plus a vectorised lookup() for the
engine's dust_global. Writer and reader in this repo agree with each other;
swap the real package back in for byte-level interop with external tooling.
Layout (little-endian):

    0   6s     magic  b'intmap'
    6   B      version = 1
    7   B      reserved = 0
    8   Q      N (number of entries)
    16  N x Q  keys, ascending
    ..  N x Q  values
"""
from __future__ import annotations

import struct

import numpy as np

MAGIC = b"intmap"
VERSION = 1
HEADER_FMT = "<6sBBQ"
HEADER_LEN = struct.calcsize(HEADER_FMT)  # 16
_TOP = (1 << 64) - 1


class IntMap:
    """dict-like uint64 -> uint64 container.

    IntMap(dict_of_ints)  -> .tobytes()
    IntMap(bytes)         -> read-only view of a serialized buffer"""

    def __init__(self, data=None):
        if data is None:
            data = {}
        if isinstance(data, (bytes, bytearray, memoryview)):
            self._keys, self._vals = self._parse(bytes(data))
            return
        items = sorted((int(k), int(v)) for k, v in dict(data).items())
        for k, v in items:
            if not (0 <= k <= _TOP and 0 <= v <= _TOP):
                raise ValueError(f"IntMap: {k}: {v} does not fit uint64")
        self._keys = np.fromiter((k for k, _ in items), dtype=np.uint64,
                                 count=len(items))
        self._vals = np.fromiter((v for _, v in items), dtype=np.uint64,
                                 count=len(items))

    @staticmethod
    def _parse(buf: bytes):
        if len(buf) < HEADER_LEN:
            raise ValueError("IntMap: truncated buffer (no header)")
        magic, version, _reserved, n = struct.unpack_from(HEADER_FMT, buf, 0)
        if magic != MAGIC:
            raise ValueError(f"IntMap: bad magic {magic!r}")
        if version != VERSION:
            raise ValueError(f"IntMap: unsupported version {version}")
        if len(buf) < HEADER_LEN + 16 * n:
            raise ValueError(
                f"IntMap: truncated buffer ({len(buf)} bytes, {n} entries "
                f"need {HEADER_LEN + 16 * n})")
        keys = np.frombuffer(buf, dtype="<u8", count=n, offset=HEADER_LEN)
        vals = np.frombuffer(buf, dtype="<u8", count=n,
                             offset=HEADER_LEN + 8 * n)
        return keys.astype(np.uint64), vals.astype(np.uint64)

    def tobytes(self) -> bytes:
        return (struct.pack(HEADER_FMT, MAGIC, VERSION, 0, len(self))
                + self._keys.astype("<u8").tobytes()
                + self._vals.astype("<u8").tobytes())

    def __len__(self) -> int:
        return int(self._keys.shape[0])

    def _index(self, label) -> int:
        label = int(label)
        if 0 <= label <= _TOP:
            i = int(np.searchsorted(self._keys, np.uint64(label)))
            if i < len(self) and int(self._keys[i]) == label:
                return i
        raise KeyError(label)

    def __getitem__(self, label) -> int:
        return int(self._vals[self._index(label)])

    def __contains__(self, label) -> bool:
        try:
            self._index(label)
        except KeyError:
            return False
        return True

    def get(self, label, default=None):
        try:
            return self[label]
        except KeyError:
            return default

    def keys(self):
        return iter(self._keys.tolist())

    def values(self):
        return iter(self._vals.tolist())

    def items(self):
        return zip(self._keys.tolist(), self._vals.tolist())

    def __iter__(self):
        return self.keys()

    def lookup(self, labels: np.ndarray) -> np.ndarray:
        """values of an array of labels, as uint64 of the same shape. Raises
        KeyError naming the first absent label, as mb[label] does in the
        reference's loop (mesh.py:352)."""
        labels = np.asarray(labels, dtype=np.uint64)
        if labels.size == 0:
            return np.zeros(labels.shape, dtype=np.uint64)
        if len(self) == 0:
            raise KeyError(int(labels.reshape(-1)[0]))
        idx = np.searchsorted(self._keys, labels)
        idx[idx >= len(self)] = 0
        miss = self._keys[idx] != labels
        if miss.any():
            raise KeyError(int(labels[miss][0]))
        return self._vals[idx]
