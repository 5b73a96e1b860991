"""Host reference and input builders of the octree level tests (a helper
module, not a conftest).

The reference is tasks.multires.encode_octree_level_host, the per-level body
of process_mesh: create_octree_level_from_mesh, then to_stored_model_space
and formats.draco.encode per fragment. `host_level` runs it with the pure
host chunker and retriangulator (igneous_amd.meshops); `product_level` runs
it over the engine's chunk_mesh and retriangulate_mesh, the route
process_mesh took before the one-call encoder, for inputs the pure host
functions take too long on.
"""
import contextlib

import numpy as np

from igneous_amd import meshops
from igneous_amd.formats import draco
from igneous_amd.meshes import Mesh
from igneous_amd.tasks import multires


def sheet(n: int) -> Mesh:
    """n x n tilted sheet, two triangles per quad."""
    y, x = np.meshgrid(np.arange(n, dtype=np.float64),
                       np.arange(n, dtype=np.float64), indexing="ij")
    x, y = x.reshape(-1), y.reshape(-1)
    verts = np.stack([1.13 * x + 0.4, 0.97 * y + 0.2,
                      0.37 * x + 0.21 * y + 3.3], axis=1).astype(np.float32)
    i = (np.arange(n - 1, dtype=np.uint32)[:, None] * n
         + np.arange(n - 1, dtype=np.uint32)[None, :]).reshape(-1)
    faces = np.concatenate([
        np.stack([i, i + 1, i + n], axis=1),
        np.stack([i + 1, i + n + 1, i + n], axis=1)]).astype(np.uint32)
    return Mesh(verts, faces, id=1)


def box_surface(n: int = 24) -> Mesh:
    """The roughened n^3 box of test_gpu_chunk_mesh.py (seed 17, resolution
    (4, 4, 40)): a closed marching-cubes surface with interior faces, from
    the CPU oracle."""
    import oracle
    rng = np.random.default_rng(17)
    data = np.zeros((n, n, n), dtype=np.uint32, order="F")
    data[1:-1, 1:-1, 1:-1] = 1
    carve = rng.integers(1, n - 1, size=(n * n // 2, 3))
    data[carve[:, 0], carve[:, 1], carve[:, 2]] = 0
    v, f = oracle.mesh_chunk(data, resolution=(4.0, 4.0, 40.0))[1]
    return Mesh(np.ascontiguousarray(v, dtype=np.float32),
                np.ascontiguousarray(f, dtype=np.uint32), id=1)


def grid_for(mesh: Mesh, num_lods: int):
    """(grid_origin, chunk_shape) as process_mesh derives them:
    offset = floor(min), chunk_shape = ceil(shape / 2^(num_lods - 1))."""
    origin, shape = multires.determine_mesh_shape_from_lods([mesh])
    return origin, np.ceil(shape / (2 ** (num_lods - 1)))


@contextlib.contextmanager
def host_seams():
    """The pure host chunker (and with it the host retriangulation)."""
    multires.set_chunker(meshops.chunk_mesh)
    try:
        yield
    finally:
        multires.set_chunker(None)


def host_level(mesh, chunk_shape, lod, num_lods, grid_origin, vqb):
    with host_seams():
        return multires.encode_octree_level_host(
            mesh, chunk_shape, lod, num_lods, grid_origin, vqb)


def product_level(mesh, chunk_shape, lod, num_lods, grid_origin, vqb):
    return multires.encode_octree_level_host(
        mesh, chunk_shape, lod, num_lods, grid_origin, vqb)


def engine_level(mesh, chunk_shape, lod, num_lods, grid_origin, vqb):
    return multires.engine_level_encoder(
        mesh, chunk_shape, lod, num_lods, grid_origin, vqb)


def inline_level(mesh, chunk_shape, lod, num_lods, grid_origin, vqb):
    """The loop process_mesh held inline before the per-level function,
    written out on the formats alone: (nodes, sizes, blob) of one LOD."""
    with host_seams():
        submeshes, nodes = multires.create_octree_level_from_mesh(
            mesh, chunk_shape, lod, num_lods, grid_origin, None)
    qmax = float((1 << vqb) - 1)
    cell = np.asarray(chunk_shape, dtype=np.float64) * float(2 ** lod)
    origin = np.asarray(grid_origin, dtype=np.float64)
    out = []
    for sub, node in zip(submeshes, nodes):
        v = np.asarray(sub.vertices, dtype=np.float64)
        rel = (v - origin - np.zeros(3)) / cell - np.asarray(
            node, dtype=np.float64)
        q = np.clip(np.rint(rel * qmax), 0, qmax).astype(np.uint32)
        out.append(draco.encode(q, sub.faces) if len(sub.faces) else b"")
    return tuple(nodes), [len(b) for b in out], b"".join(out)


def split(sizes, blob):
    """The level's blob cut back into its fragments."""
    at = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    assert at[-1] == len(blob)
    return [blob[at[i]:at[i + 1]] for i in range(len(sizes))]


def int_draco_size(nv: int, nf: int, faces=None) -> int:
    """Size of formats.draco.encode's output for integer positions: the
    formula the device layout (enc_layout, ENC_DRACO_INT) computes. `faces`
    is needed in the varint band only."""
    def vlen(x):
        return 1 if x < 1 << 7 else 2 if x < 1 << 14 else 3 if x < 1 << 21 \
            else 4 if x < 1 << 28 else 5
    if nv == 0 or nf == 0:
        return 0
    if nv < 1 << 8:
        idx = 3 * nf
    elif nv < 1 << 16:
        idx = 6 * nf
    elif nv < 1 << 21:
        idx = sum(vlen(int(i)) for i in np.asarray(faces).reshape(-1))
    else:
        idx = 12 * nf
    return 11 + vlen(nf) + vlen(nv) + 1 + idx + 10 + 12 * nv
