"""GPU parity tests that pin every path of the simplifier's per-label
kernel: its three vertex-count bands (nv <= 2048 and 2048 < nv <= 4096
with LDS-resident tables, nv > 4096 on the global arrays), the band
edges themselves, and the 65536-face hand-over to the global-rounds
path. Engine against the CPU oracle, bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES = (16.0, 16.0, 40.0)
BIG_LABEL = (1 << 40) + 5
# label -> (lowest nv excluded, highest nv included) of its band
BALL_BANDS = {11: (0, 2048), 12: (2048, 4096),
              14: (4096, None), BIG_LABEL: (4096, None)}


@pytest.fixture(scope="module")
def eng():
    from igneous_amd.engine import Engine
    return Engine.get(0)


def _assert_meshsets_equal(got: dict, want: dict, what=""):
    assert sorted(got.keys()) == sorted(want.keys()), \
        f"{what}: label sets differ ({len(got)} vs {len(want)})"
    for label in want:
        gv, gf = got[label]
        wv, wf = want[label]
        assert gv.shape == wv.shape, \
            f"{what} label {label}: nverts {gv.shape[0]} != {wv.shape[0]}"
        assert gf.shape == wf.shape, \
            f"{what} label {label}: ntris {gf.shape[0]} != {wf.shape[0]}"
        assert np.array_equal(gf, wf), f"{what} label {label}: faces differ"
        assert np.array_equal(gv, wv), f"{what} label {label}: verts differ"


def _ball_volume():
    data = np.zeros((112, 64, 64), dtype=np.uint64, order="F")
    x, y, z = np.ogrid[0:112, 0:64, 0:64]

    def ball(cx, cy, cz, r):
        return (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r

    data[ball(12, 12, 12, 9.3)] = 11
    data[ball(16, 44, 40, 14.3)] = 12
    big = ball(72, 32, 32, 29.3)
    data[big & (x < 60)] = BIG_LABEL
    data[big & (x >= 60)] = 14
    return data


@pytest.fixture(scope="module")
def balls():
    """The volume and the oracle's unsimplified meshes of it."""
    import oracle
    data = _ball_volume()
    return data, oracle.mesh_chunk(data, resolution=RES)


def test_every_band_in_one_chunk(eng, balls, monkeypatch):
    """One chunk with a label in each nv band, two of them above 4096
    vertices with a label-label interface between them."""
    import oracle
    data, full = balls
    assert sorted(full) == sorted(BALL_BANDS)
    sizes = {label: (m[0].shape[0], m[1].shape[0])
             for label, m in full.items()}
    assert sizes == {11: (1662, 3320), 12: (3846, 7688),
                     14: (13682, 27360), BIG_LABEL: (6926, 13848)}
    for label, (lo, hi) in BALL_BANDS.items():
        nv, nt = sizes[label]
        assert nv > lo and (hi is None or nv <= hi), (label, nv)
        assert nt < 65536, (label, nt)   # all on the per-label kernel

    def check(factor, err, what):
        got = eng.mesh_chunk(data, resolution=RES, reduction_factor=factor,
                             max_error=err)
        want = oracle.mesh_chunk(data, resolution=RES,
                                 reduction_factor=factor, max_error=err)
        _assert_meshsets_equal(got, want, what)

    for factor, err in ((100, 40.0), (10, 1e9), (4, 0.0)):
        check(factor, err, f"bands f={factor} e={err}")
    # sub-rounds per quadric recompute: both sides read it per call
    for subs in ("1", "3"):
        monkeypatch.setenv("MG_SIMP_SUBS", subs)
        check(100, 40.0, f"bands subs={subs}")


def _height_field(w, h, extra=False):
    """Roughened height field on a w x h vertex grid, two triangles per
    cell in cell order; extra=True hangs one more vertex and triangle on
    a boundary edge."""
    rng = np.random.default_rng(1000 * w + h)
    y, x = np.mgrid[0:h, 0:w]
    smooth = np.rint(40.0 * np.sin(0.31 * x) * np.cos(0.23 * y))
    z = 4.0 * (smooth + rng.integers(-2, 3, size=(h, w)))
    verts = np.stack([16.0 * x, 16.0 * y, z], axis=-1).reshape(-1, 3)
    v00 = (y[:-1, :-1] * w + x[:-1, :-1]).ravel()
    faces = np.stack([v00, v00 + 1, v00 + w + 1,
                      v00, v00 + w + 1, v00 + w], axis=-1).reshape(-1, 3)
    if extra:
        verts = np.concatenate([verts, [[-16.0, 8.0, z[0, 0] + 4.0]]])
        faces = np.concatenate([faces, [[0, w, w * h]]])
    return (np.ascontiguousarray(verts, dtype=np.float32),
            np.ascontiguousarray(faces, dtype=np.uint32))


@pytest.mark.parametrize("w,h,extra,nv,nt", [
    (64, 32, False, 2048, None),      # last size of the first band
    (683, 3, False, 2049, None),      # first size of the second band
    (64, 64, False, 4096, None),      # last size with LDS tables
    (17, 241, False, 4097, None),     # first size on the global arrays
    (129, 257, False, 33153, 65536),  # last size on the per-label path
    (129, 257, True, 33154, 65537),   # first size on the global-rounds
])                                    # path (1 sub-round per group)
def test_band_edges_through_simplify_mesh(eng, w, h, extra, nv, nt):
    import oracle
    v, f = _height_field(w, h, extra)
    assert v.shape[0] == nv
    assert nt is None or f.shape[0] == nt
    for factor, err in ((8, 1e30), (100, 40.0)):
        gv, gf = eng.simplify_mesh(v, f, factor, err)
        wv, wf = oracle.simplify_mesh(v, f, factor, err)
        what = f"{w}x{h}{'+1' if extra else ''} f={factor} e={err}"
        assert wf.shape[0] < f.shape[0], f"{what}: oracle reduced nothing"
        assert gf.shape == wf.shape, f"{what}: {gf.shape} != {wf.shape}"
        assert np.array_equal(gf, wf), f"{what}: faces differ"
        assert np.array_equal(gv, wv), f"{what}: verts differ"
