"""numpy equivalents of the fastremap calls on the MeshTask host path
(/root/reference/igneous/tasks/mesh/mesh.py:201-206,318-320,368-369).

The reference also calls fastremap.renumber (mesh.py:206) purely to shrink
the dtype and give the mesher small ids, inverting the map afterwards
(mesh.py:207, 371-383). Our engine hashes raw uint32/uint64 labels directly,
so the renumber+invert round trip is the identity composition and is
intentionally omitted from the product path (documented in DESIGN.md).
"""
from __future__ import annotations

import numpy as np


def mask(data: np.ndarray, labels, in_place: bool = True) -> np.ndarray:
    """Zero out the given labels (fastremap.mask, mesh.py:204,320)."""
    if len(labels) == 0:
        return data
    sel = np.isin(data, np.asarray(list(labels), dtype=data.dtype))
    out = data if in_place else data.copy()
    out[sel] = 0
    return out


def mask_except(data: np.ndarray, labels, in_place: bool = True) -> np.ndarray:
    """Zero out everything except the given labels
    (fastremap.mask_except, mesh.py:201,355,368)."""
    sel = np.isin(data, np.asarray(list(labels), dtype=data.dtype))
    out = data if in_place else data.copy()
    out[~sel] = 0
    return out


def remap(data: np.ndarray, table: dict, in_place: bool = True) -> np.ndarray:
    """Apply {orig: new} label mapping (fastremap.remap, mesh.py:369).
    Labels absent from the table are left unchanged (the reference masks
    them away first, mesh.py:368)."""
    out = data if in_place else data.copy()
    if not table:
        return out
    keys = np.fromiter(table.keys(), dtype=data.dtype, count=len(table))
    vals = np.fromiter(table.values(), dtype=data.dtype, count=len(table))
    order = np.argsort(keys)
    keys, vals = keys[order], vals[order]
    idx = np.searchsorted(keys, out)
    idx[idx >= len(keys)] = 0
    hit = keys[idx] == out
    out[hit] = vals[idx[hit]]
    return out


def _ids(ids, what: str) -> set:
    out = set()
    for i in (ids if ids is not None else ()):
        i = int(i)
        if i < 0:
            raise ValueError(f"{what}: negative id {i}")
        out.add(i)
    return out


def fold_label_ops(remap_table, object_ids, exclude_object_ids, dtype):
    """Fold MeshTask's three label-selection options, in the reference's
    order remap -> object_ids -> exclude_object_ids (mesh.py:193-204), into
    ONE lookup table for the engine's device label map.

    Returns None when no option is set, else (keys u64[n], vals u64[n],
    miss): each voxel is looked up once with its RAW label (no chaining);
    a hit is replaced by its val (0 = erase), a label absent from the
    table is kept (miss == 'keep') or erased (miss == 'zero'). Label 0 is
    never a key. Applying the triple equals the host sequence
    mask_except(keys) -> remap -> mask_except(object_ids) ->
    mask(exclude_object_ids) above.

    Negative ids and remap values that do not fit dtype raise ValueError;
    keys that do not fit dtype can never match a voxel and are dropped."""
    top = int(np.iinfo(np.dtype(dtype)).max)
    only = _ids(object_ids, "object_ids")
    excl = _ids(exclude_object_ids, "exclude_object_ids")

    if remap_table is not None:
        table = {}
        for k, v in remap_table.items():
            k, v = int(k), int(v)
            if k < 0 or v < 0:
                raise ValueError(f"remap_table: negative id in {k}: {v}")
            if v > top:
                raise ValueError(
                    f"remap_table: value {v} does not fit {np.dtype(dtype)}")
            if k == 0 or k > top:
                continue  # the reference forces remap[0] = 0
            if (only and v not in only) or v in excl:
                v = 0
            table[k] = v
        miss = 'zero'
    elif only:
        table = {k: k for k in only - excl if 0 < k <= top}
        miss = 'zero'
    elif excl:
        table = {k: 0 for k in excl if 0 < k <= top}
        miss = 'keep'
    else:
        return None

    keys = np.fromiter(sorted(table), dtype=np.uint64, count=len(table))
    vals = np.fromiter((table[int(k)] for k in keys), dtype=np.uint64,
                       count=len(table))
    return keys, vals, miss


def fold_dust(label_map, dust_ids, dtype):
    """Fold a set of dust labels into a fold_label_ops table, for the
    global dust threshold (mesh.py:324-355): the reference erases dust on
    the RAW labels first and applies remap / object_ids /
    exclude_object_ids afterwards (mesh.py:193-204), so applying the
    returned triple equals mask(dust_ids) followed by label_map.

    label_map is None or (keys, vals, miss); dust_ids are raw labels (0 and
    ids that do not fit dtype can never match a voxel and are dropped).
      - None: (sorted dust, zeros, 'keep'), or None without dust;
      - miss 'keep': the table plus {d: 0}, replacing any entry for d;
      - miss 'zero': the table without the keys in dust (a miss erases)."""
    top = int(np.iinfo(np.dtype(dtype)).max)
    dust = np.unique(np.asarray(dust_ids, dtype=np.uint64).reshape(-1))
    dust = dust[(dust != 0) & (dust <= np.uint64(top))]
    if label_map is None:
        if dust.shape[0] == 0:
            return None
        return dust, np.zeros_like(dust), 'keep'
    keys, vals, miss = label_map
    keys = np.asarray(keys, dtype=np.uint64)
    vals = np.asarray(vals, dtype=np.uint64)
    if miss not in ('keep', 'zero'):
        raise ValueError(f"label_map miss policy {miss!r}: "
                         f"expected 'keep' or 'zero'")
    if dust.shape[0] == 0:
        return keys, vals, miss
    stay = ~np.isin(keys, dust)
    keys, vals = keys[stay], vals[stay]
    if miss == 'keep':
        keys = np.concatenate([keys, dust])
        vals = np.concatenate([vals, np.zeros_like(dust)])
        order = np.argsort(keys, kind='stable')
        keys, vals = keys[order], vals[order]
    return keys, vals, miss


def unique(data: np.ndarray, return_counts: bool = False):
    """fastremap.unique equivalent (mesh.py:318)."""
    return np.unique(data, return_counts=return_counts)
