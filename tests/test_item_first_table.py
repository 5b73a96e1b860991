"""MC_ITEM_FIRST (mc_table.h): the per-item form of the weld's
first-occurrence predicate. Entry [mask][interior] has bit 3t + v set when
corner v of triangle t is its slot's first occurrence in the label's stream,
so its popcount is the item's vertex count — the input of the item scan that
gives every item its first vertex id.

Checked against a brute-force evaluation of the per-triangle tables it was
folded from (MC_TRI_FIRST, MC_TRI_PACK, MC_EDGE_NEED), and, through a numpy
replay of the emit order on a small unpadded volume, against the oracle's
per-label vertex counts."""
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

import gen_mc_table as g


def _table(text, name, dims):
    pat = re.escape(name) + "".join(r"\[%d\]" % d for d in dims) + \
        r" = \{(.*?)\};"
    body = re.search(pat, text, re.S).group(1)
    vals = [int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", body)]
    return np.array(vals, dtype=np.int64).reshape(dims)


def _header():
    with open(os.path.join(REPO, "igneous_amd", "csrc", "mc_table.h")) as f:
        text = f.read()
    maxt = int(re.search(r"#define MC_MAX_TRIS (\d+)", text).group(1))
    return {
        "maxt": maxt,
        "count": _table(text, "MC_TRI_COUNT", (256,)),
        "pack": _table(text, "MC_TRI_PACK", (256, maxt)),
        "first": _table(text, "MC_TRI_FIRST", (256, maxt)),
        "need": _table(text, "MC_EDGE_NEED", (12,)),
        "item": _table(text, "MC_ITEM_FIRST", (256, 8)),
    }


def test_item_first_is_the_folded_triangle_tables():
    h = _header()
    assert 3 * h["maxt"] <= 16  # the entry is a u16
    for mask in range(256):
        for interior in range(8):
            want = 0
            for t in range(int(h["count"][mask])):
                for v in range(3):
                    e = (int(h["pack"][mask][t]) >> (5 * v)) & 15
                    if (int(h["first"][mask][t]) >> v) & 1 and \
                            (int(h["need"][e]) & interior) == 0:
                        want |= 1 << (3 * t + v)
            got = int(h["item"][mask][interior])
            assert got == want, (mask, interior, hex(got), hex(want))
            # the generator's own function gives the same
            assert g.item_first_bits(
                g.triangulate(g.loops_for_mask(mask)), interior) == want
    # nothing above the mask's triangles, nothing for the empty masks
    assert h["item"][0].max() == 0 and h["item"][255].max() == 0
    assert h["item"].max() < 1 << (3 * h["maxt"])


def _popcount(a):
    a = a.astype(np.uint64)
    n = np.zeros(a.shape, dtype=np.int64)
    for b in range(16):
        n += ((a >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return n


def _label_vertex_counts(vol, item):
    """Replay the emit in numpy: one item per (cell, distinct non-zero corner
    label); its vertices are popcount(MC_ITEM_FIRST[mask][interior])."""
    sx, sy, sz = vol.shape
    corners = np.stack([vol[dx:sx - 1 + dx, dy:sy - 1 + dy, dz:sz - 1 + dz]
                        for (dx, dy, dz) in g.CORNER_POS])  # 8 x cells
    cx, cy, cz = np.meshgrid(np.arange(sx - 1), np.arange(sy - 1),
                             np.arange(sz - 1), indexing="ij")
    interior = ((cx > 0) * 1 + (cy > 0) * 2 + (cz > 0) * 4)
    pop = _popcount(item)
    counts = {}
    for lab in np.unique(vol):
        if lab == 0:
            continue
        mask = np.zeros(cx.shape, dtype=np.int64)
        for i in range(8):
            mask |= (corners[i] == lab).astype(np.int64) << i
        counts[int(lab)] = int(pop[mask, interior].sum())
    return counts


def test_item_vertex_counts_sum_to_the_oracle_vertex_counts():
    import oracle
    h = _header()
    rng = np.random.default_rng(97)
    # unpadded: labels touch all six faces, every interior value occurs
    vol = np.asfortranarray(
        rng.integers(0, 5, size=(11, 9, 10)).astype(np.uint32))
    want = oracle.mesh_chunk(vol, resolution=(1.0, 1.0, 1.0))
    got = _label_vertex_counts(vol, h["item"])
    assert len(want) >= 4
    for lab, (verts, faces) in want.items():
        assert got[int(lab)] == verts.shape[0], lab
        assert verts.shape[0] > 0 and faces.shape[0] > 0
    assert set(got) == {int(k) for k in want}
