"""The weld's first-occurrence predicate (MC_TRI_FIRST / MC_EDGE_NEED in
mc_table.h) against a brute-force replay of the emit order.

A corner of a label's triangle stream is the first occurrence of its
(edge, label) iff its cell is the lowest cell holding the edge and its
(t, v) is the mask's first use of the edge. The replay walks cells in
(z, y, x) order, each label's triangles t ascending, corners v = 0..2,
and remembers which (label, global edge) pairs it has seen."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import gen_mc_table as g

SHAPES = [(2, 2, 2), (2, 9, 2), (5, 2, 9), (3, 8, 2), (9, 7, 6), (12, 11, 10)]


def _tables_from_scratch():
    """first/need rebuilt from the triangulation and the corner geometry,
    without the generator's own first/need code."""
    tris = [g.triangulate(g.loops_for_mask(m)) for m in range(256)]
    first = []
    for m in range(256):
        row = []
        for t, tri in enumerate(tris[m]):
            before = [e for prev in tris[m][:t] for e in prev]
            row.append(sum(1 << v for v in range(3) if tri[v] not in before))
        first.append(row)
    need = []
    for a, b in g.EDGES:
        pa, pb = g.CORNER_POS[a], g.CORNER_POS[b]
        along = [i for i in range(3) if pa[i] != pb[i]]
        assert len(along) == 1
        need.append(sum(1 << i for i in range(3)
                        if i != along[0] and pa[i] == 0))
    return tris, first, need


def _header_tables():
    hdr = os.path.join(REPO, "igneous_amd", "csrc", "mc_table.h")
    with open(hdr) as f:
        text = f.read()
    maxt = int(re.search(r"#define MC_MAX_TRIS (\d+)", text).group(1))
    m = re.search(r"MC_TRI_FIRST\[256\]\[(\d+)\] = \{(.*?)\};", text, re.S)
    assert int(m.group(1)) == maxt
    first = np.array([int(x) for x in re.findall(r"\d+", m.group(2))],
                     dtype=np.int64).reshape(256, maxt)
    m = re.search(r"MC_EDGE_NEED\[12\] = \{(.*?)\};", text, re.S)
    need = [int(x) for x in re.findall(r"\d+", m.group(1))]
    assert len(need) == 12
    return maxt, first, need


def test_header_tables_match_generator_and_scratch():
    tris, first_ref, need_ref = _tables_from_scratch()
    maxt, first_h, need_h = _header_tables()
    assert need_h == need_ref == [g.edge_need(e) for e in range(12)]
    for m in range(256):
        want = first_ref[m] + [0] * (maxt - len(first_ref[m]))
        assert list(first_h[m]) == want, m
        assert g.tri_first_bits(tris[m]) == first_ref[m], m
    assert first_h.max() < 8 and max(need_h) < 8


def _replay(vol, tris, first, need):
    """(corners checked, mismatches) of predicate vs first-seen."""
    sx, sy, sz = vol.shape
    seen = set()
    n = bad = 0
    for cz in range(sz - 1):
        for cy in range(sy - 1):
            for cx in range(sx - 1):
                c = [int(vol[cx + dx, cy + dy, cz + dz])
                     for (dx, dy, dz) in g.CORNER_POS]
                zero = (cx == 0) | ((cy == 0) << 1) | ((cz == 0) << 2)
                for L in dict.fromkeys(c):  # distinct, corner order
                    if L == 0:
                        continue
                    mask = sum(1 << i for i in range(8) if c[i] == L)
                    for t, tri in enumerate(tris[mask]):
                        for v, e in enumerate(tri):
                            off = g.EDGE_DOFF[e]
                            key = (L, 2 * cx + off[0], 2 * cy + off[1],
                                   2 * cz + off[2])
                            brute = key not in seen
                            seen.add(key)
                            pred = bool((first[mask][t] >> v) & 1) and \
                                (need[e] & ~zero & 7) == 0
                            n += 1
                            bad += pred != brute
    return n, bad


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_predicate_equals_first_seen(shape):
    """Dense volumes, labels 0..k touching every border (no padding)."""
    tris, _, _ = _tables_from_scratch()
    _, first_h, need_h = _header_tables()
    total = 0
    for k in range(2, 10):
        rng = np.random.default_rng(1000 * k + sum(shape))
        vol = rng.integers(0, k + 1, size=shape)
        n, bad = _replay(vol, tris, first_h, need_h)
        assert bad == 0, f"{shape} k={k}: {bad} of {n} corners mismatch"
        total += n
    assert total > 0
