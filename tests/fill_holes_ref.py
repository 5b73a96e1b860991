"""Checker for the fill_holes contract — a helper, not a
test file. numpy + scipy.ndimage.label restatement, written independently
of the device code: per-value labelling, then a neighbour reduction with
np.minimum.at / np.maximum.at.

Contract: 6-connectivity; a component is a maximal 6-connected set of
equal value (0 included). In one round every component that (1) has no
voxel on the border (coordinate 0 or size-1 on an axis of size > 1),
(2) sees one single value L on all outside face neighbours and (3) L != 0
is rewritten to L, all at once. Rounds repeat to a fixed point. Level 2
first runs the rounds on the six boundary slices, each as a one-voxel-thick
volume, in the order x=0, x=sx-1, y=0, y=sy-1, z=0, z=sz-1. holes[v] is
input[v] where filled[v] != input[v], else 0.

The volume builders below are shared by the host and the GPU tests.
"""
import numpy as np
from scipy import ndimage

MAX_ROUNDS = 64


def _components(vol):
    """comp (same shape, ids 0..n-1) for 6-connected equal-value sets."""
    comp = np.zeros(vol.shape, dtype=np.int64)
    n = 0
    # values renumbered 1..k so that each is labelled inside its own
    # bounding box only (volumes with thousands of labels stay tractable)
    _, inv = np.unique(vol, return_inverse=True)
    inv = inv.reshape(vol.shape).astype(np.int32) + 1
    for k, box in enumerate(ndimage.find_objects(inv)):
        lab, cnt = ndimage.label(inv[box] == k + 1)  # faces only (default)
        m = lab > 0
        view = comp[box]
        view[m] = lab[m] + (n - 1)
        n += cnt
    return comp, n


def one_round(vol):
    """-> (new volume, number of rewritten voxels)."""
    comp, n = _components(vol)
    border = np.zeros(vol.shape, dtype=bool)
    for ax, size in enumerate(vol.shape):
        if size > 1:
            idx = [slice(None)] * 3
            idx[ax] = 0
            border[tuple(idx)] = True
            idx[ax] = size - 1
            border[tuple(idx)] = True
    on_border = np.zeros(n, dtype=bool)
    on_border[comp[border]] = True
    big = np.iinfo(np.uint64).max
    mn = np.full(n, big, dtype=np.uint64)
    mx = np.zeros(n, dtype=np.uint64)
    v64 = vol.astype(np.uint64)
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax] = slice(0, -1)
        hi[ax] = slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        diff = v64[lo] != v64[hi]
        for me, other in ((lo, hi), (hi, lo)):
            ids = comp[me][diff]
            vals = v64[other][diff]
            np.minimum.at(mn, ids, vals)
            np.maximum.at(mx, ids, vals)
    enclosed = (~on_border) & (mn == mx) & (mn != 0)
    hit = enclosed[comp]
    out = vol.copy()
    out[hit] = mn[comp[hit]].astype(vol.dtype)
    return out, int(hit.sum())


def fixed_point(vol):
    """-> (volume at the fixed point, productive rounds)."""
    rounds = 0
    for _ in range(MAX_ROUNDS):
        vol, changed = one_round(vol)
        if changed == 0:
            return vol, rounds
        rounds += 1
    raise RuntimeError(f"did not converge in {MAX_ROUNDS} rounds")


def fill_holes_ref(labels, level):
    """-> (filled, holes, rounds). rounds counts the productive 3-D
    rounds, like mg_fill_holes' rounds_out."""
    assert level in (1, 2)
    vol = np.array(labels, order="F", copy=True)
    assert vol.ndim == 3
    if level == 2:
        for ax in range(3):
            for pos in (0, vol.shape[ax] - 1):
                idx = [slice(None)] * 3
                idx[ax] = slice(pos, pos + 1)  # keeps the axis, size 1
                idx = tuple(idx)
                vol[idx], _ = fixed_point(vol[idx].copy())
    filled, rounds = fixed_point(vol)
    holes = np.where(filled != labels, labels, 0).astype(labels.dtype)
    return np.asfortranarray(filled), np.asfortranarray(holes), rounds


# ----------------------------------------------------------------------
# volume builders. Labels are given as small integers and lifted into the
# dtype: u64 ids sit above 2^33.

def lift(k, dtype):
    if np.dtype(dtype) == np.uint64:
        return (1 << 33) + 1000003 * int(k)
    return int(k)


def _zeros(shape, dtype):
    return np.zeros(shape, dtype=dtype, order="F")


def case_nested(dtype, inner=0):
    """A > B > (cavity | piece of A) in 16^3. B has 8^3 - 2^3 = 504 voxels."""
    A, B = lift(1, dtype), lift(2, dtype)
    v = _zeros((16,) * 3, dtype)
    v[1:15, 1:15, 1:15] = A
    v[4:12, 4:12, 4:12] = B
    v[7:9, 7:9, 7:9] = A if inner == 'A' else 0
    return v


def case_two_adjacent(dtype):
    """two labels touching each other inside a third: neither has a single
    neighbour label, so nothing is filled (known limitation)."""
    A, B, C = lift(1, dtype), lift(2, dtype), lift(3, dtype)
    v = _zeros((16,) * 3, dtype)
    v[1:15, 1:15, 1:15] = A
    v[5:8, 5:10, 5:10] = B
    v[8:11, 5:10, 5:10] = C
    return v


def case_island(dtype):
    """a label surrounded by background."""
    v = _zeros((16,) * 3, dtype)
    v[5:10, 4:9, 6:12] = lift(1, dtype)
    return v


def case_open_cavity(dtype):
    """4x4x6 background cavity open to the x=0 face of a solid volume."""
    v = _zeros((16,) * 3, dtype)
    v[:] = lift(1, dtype)
    v[0:4, 6:10, 5:11] = 0
    return v


def case_edge_diagonal(dtype):
    """one-voxel cavity whose only contact with the outside background is
    across an edge diagonal: not 6-connected to it, so it is filled."""
    v = _zeros((16,) * 3, dtype)
    v[2:14, 2:14, 2:14] = lift(1, dtype)
    v[2, 2, 8] = 0   # outside background reaches into the block's edge
    v[3, 3, 8] = 0   # the cavity, diagonal to it
    return v


def case_three_deep(dtype):
    """A > B > C > cavity in 20^3: three productive rounds."""
    v = _zeros((20,) * 3, dtype)
    v[1:19, 1:19, 1:19] = lift(1, dtype)
    v[4:16, 4:16, 4:16] = lift(2, dtype)
    v[7:13, 7:13, 7:13] = lift(3, dtype)
    v[9:11, 9:11, 9:11] = 0
    return v


def case_serpentine(dtype):
    """one-voxel-wide background corridor snaking through the middle layer
    of a 64x64x3 slab of one label, closed at both ends: ONE component
    that winds across the whole slab and fills in one round."""
    v = _zeros((64, 64, 3), dtype)
    v[:] = lift(1, dtype)
    rows = list(range(2, 62, 2))
    for k, y in enumerate(rows):
        v[2:62, y, 1] = 0
        if k + 1 < len(rows):
            x = 61 if k % 2 == 0 else 2
            v[x, y + 1, 1] = 0
    return v


def case_noise(dtype, shape, probs, seed, copy_border=False):
    """zero border, interior drawn from {0, a, b}: the majority label
    percolates into one winding component enclosing hundreds of small
    ones. copy_border replaces the border layer by its inner neighbour
    (open cavities on every face: level 1 != level 2)."""
    rng = np.random.default_rng(seed)
    vals = np.array([0, lift(1, dtype), lift(2, dtype)], dtype=dtype)
    v = _zeros(shape, dtype)
    inner = tuple(s - 2 for s in shape)
    v[1:-1, 1:-1, 1:-1] = vals[rng.choice(3, size=inner, p=probs)]
    if copy_border:
        v[0, :, :] = v[1, :, :]
        v[-1, :, :] = v[-2, :, :]
        v[:, 0, :] = v[:, 1, :]
        v[:, -1, :] = v[:, -2, :]
        v[:, :, 0] = v[:, :, 1]
        v[:, :, -1] = v[:, :, -2]
    return v


NOISE_CASES = [((48, 48, 48), (0.2, 0.6, 0.2)),
               ((65, 31, 20), (0.08, 0.84, 0.08))]
