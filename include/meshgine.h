/* meshgine — C ABI of the MI355X-native per-chunk meshing engine.
 *
 * This is the drop-in boundary under igneous's MeshTask hot path: it
 * replaces the work the reference delegates to the zmesh C++/Cython
 * extension, entry point for entry point:
 *
 *   mg_init            — replaces zmesh.Mesher(resolution) construction,
 *                        /root/reference/igneous/tasks/mesh/mesh.py:151
 *                        (device context instead of a CPU mesher object;
 *                        the anisotropic resolution moves to mg_mesh_chunk
 *                        because the engine is stateless per chunk)
 *   mg_mesh_chunk      — replaces the pair
 *                        Mesher.mesh(data, preserve_order=False)
 *                        (mesh.py:245: one pass over the whole F-order
 *                        chunk, label-vs-rest binary surfaces for every
 *                        non-zero label) and the per-label loop
 *                        Mesher.ids() / Mesher.get(id, reduction_factor,
 *                        max_error, voxel_centered=True)
 *                        (mesh.py:374-381: per-label quadric edge-collapse
 *                        simplification + welded vertex/face extraction).
 *                        One call produces every label's mesh.
 *   mg_mesh_chunk_mapped — mg_mesh_chunk plus the label selection the
 *                        reference runs on the host through fastremap
 *                        ahead of the mesher: remap_table
 *                        (mesh.py:357-369: mask_except to the table's keys,
 *                        then remap) and object_ids / exclude_object_ids
 *                        (mesh.py:200-204: mask_except, mask). The three
 *                        fold into one {key -> val} table + a miss policy
 *                        (mg_label_map) applied in one device volume pass.
 *   mg_fill_holes      — replaces fastmorph.fill_holes_v2 (mesh.py:220) for
 *                        fill_holes levels 1-2: host volume in, filled and
 *                        hole volumes out, computed as device volume passes
 *                        (contract: DESIGN.md §7).
 *   mg_mesh_chunk_filled — mg_mesh_chunk_mapped plus that fill between the
 *                        label map and the mesher (mesh.py:211-230); the
 *                        hole volume stays on the device.
 *   mg_mesh_holes      — replaces the second Mesher.mesh(hole_labels) +
 *                        compute_meshes (mesh.py:234-235) on the hole
 *                        volume left resident by mg_mesh_chunk_filled.
 *   mg_chunk_mesh      — replaces zmesh.chunk_mesh in the multires merge
 *                        (multires.py:550,574): grid partition of one mesh
 *                        with clipping at the cell boundaries.
 *   mg_merge_close_vertices — replaces Mesh.merge_close_vertices in the
 *                        multires merge (multires.py:551): weld of the
 *                        vertices within a radius.
 *   mg_retriangulate_mesh — replaces retriangulate_mesh as a whole
 *                        (multires.py:546-553): chunk, concatenate and weld
 *                        without the cells leaving the device.
 *   mg_encode_octree_level — replaces, for one lod of the multires merge,
 *                        create_octree_level_from_mesh (multires.py:556-585)
 *                        and the to_stored_model_space + DracoPy.encode loop
 *                        (multires.py:152-174): the mesh is uploaded once
 *                        and the level's finished fragment bytes come back.
 *   mg_mesh_chunk_encoded — mg_mesh_chunk_mapped plus the per-label loop
 *                        that follows it in MeshTask: the shift into
 *                        global nm (mesh.py:434-435), the spatial-index
 *                        box, and mesh.to_precomputed (mesh.py:448) or
 *                        DracoPy.encode (mesh.py:442-446). Returns every
 *                        label's finished bytes and box.
 *   mg_count_voxels    — replaces fastremap.unique(labels,
 *                        return_counts=True) in CountVoxelsTask
 *                        (/root/reference/igneous/tasks/image/image.py:876)
 *                        and the per-chunk fastremap.unique of
 *                        MeshTask.apply_dust_global_threshold (mesh.py:346):
 *                        every value of the volume with its voxel count,
 *                        from one device pass. The volume stays resident, so
 *                        the chunk call that follows (MG_FLAG_COUNTED) meshes
 *                        it without a second upload.
 *   mg_meshset_free    — replaces Python GC of zmesh.Mesh objects.
 *   mg_last_error      — error text for the last failed call on this ctx.
 *
 * The caller (igneous_amd.tasks.MeshTask, via ctypes) keeps everything the
 * reference keeps in Python: download, padding, folding the
 * remap/object-id options into an mg_label_map, and upload. The shift of
 * vertices into global nm coordinates (mesh.py:434-435) and the
 * precomputed / draco encoding (mesh.py:442-448) stay there too for
 * mg_mesh_chunk*; mg_mesh_chunk_encoded takes them to the device.
 *
 * Vertices returned are CHUNK-LOCAL nm coordinates (float32), exactly as
 * zmesh returns them to MeshTask before the Python-side offset is applied.
 *
 * Threading: one mg_ctx per device (or several per device for
 * overlapping streams); calls on distinct ctxs may run concurrently.
 * Calls on one ctx serialize internally. No global state besides the HIP
 * runtime. Errors: non-zero int return + mg_last_error.
 * Ownership: the meshset's flat vertex/face storage is CTX-OWNED pinned
 * staging, reused by the ctx's next call (see mg_meshset below);
 * mg_meshset_free frees the descriptor. Consume or copy results before
 * the next mg_mesh_chunk on the same ctx.
 */
#ifndef MESHGINE_H
#define MESHGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_ctx mg_ctx;

/* dtype codes for the label volume */
#define MG_U32 0
#define MG_U64 1

/* flags for mg_mesh_chunk */
#define MG_FLAG_NONE        0u
#define MG_FLAG_DEVICE_ONLY 1u  /* run all kernels, skip the D2H extract
                                   (bench: job complete with outputs in
                                   HBM; sizes still reported) */
#define MG_FLAG_SKIP_H2D    2u  /* label volume already resident in the
                                   ctx's device buffer from a previous
                                   call with identical dims/dtype (bench:
                                   timed region starts with inputs in
                                   HBM). Caller's responsibility. */
#define MG_FLAG_COUNTED     4u  /* the four mg_mesh_chunk* calls: the label
                                   volume is the RAW one the mg_count_voxels
                                   call JUST BEFORE on this ctx left
                                   resident; no upload. Unlike
                                   MG_FLAG_SKIP_H2D it may be combined with
                                   a label map and with fill_level > 0 (the
                                   volume is known to be raw). Checked after
                                   every other argument check, return code
                                   9: no counted volume on the ctx (any
                                   other call in between drops it), dims or
                                   dtype differ from the counted volume's,
                                   or combined with MG_FLAG_SKIP_H2D. */

/* One label's mesh. verts = 3*nverts float32 chunk-local nm (x,y,z);
 * faces = 3*ntris uint32 indices into verts. Pointers alias the meshset's
 * internal storage; freed by mg_meshset_free. */
typedef struct {
  uint64_t  label;
  uint32_t  nverts;
  uint32_t  ntris;
  float    *verts;
  uint32_t *faces;
} mg_mesh;

typedef struct {
  uint32_t  nmeshes;
  mg_mesh  *meshes;      /* sorted by ascending label id */
  /* flat storage the per-mesh pointers alias (single-copy extraction):
   * verts_base[3*total_verts], faces_base[3*total_tris]. The storage is
   * OWNED BY THE CTX (pinned, reused): it stays valid until the next
   * mg_mesh_chunk on the same ctx or mg_destroy. mg_meshset_free frees
   * only the descriptor. */
  float    *verts_base;
  uint32_t *faces_base;
  uint64_t  total_verts;
  uint64_t  total_tris;
  /* flat per-mesh metadata (same order as meshes[]; ctx-independent,
   * stored in the descriptor allocation): hosts without struct-walking
   * FFI can slice the flat storage from these. */
  uint64_t *labels_arr;   /* [nmeshes] */
  uint32_t *voff_arr;     /* [nmeshes] vertex offset into verts_base/3 */
  uint32_t *nv_arr;       /* [nmeshes] */
  uint32_t *foff_arr;     /* [nmeshes] face offset into faces_base/3 */
  uint32_t *nf_arr;       /* [nmeshes] */
} mg_meshset;

/* Per-call kernel timing/stats, HIP-event measured on the engine stream.
 * All times in milliseconds for the LAST mg_mesh_chunk on this ctx. */
typedef struct {
  double ms_h2d;        /* label volume upload */
  double ms_count;      /* pass 1: per-segment triangle count */
  double ms_scan;       /* segment offset scan (+ total readback) */
  double ms_emit;       /* pass 2: triangle emit (keys + label ids) */
  double ms_partition;  /* stable partition of triangles by label */
  double ms_weld;       /* vertex weld + index build + vertex writeout */
  double ms_simplify;   /* per-label quadric collapse (0 if disabled) */
  double ms_d2h;        /* result download (0 under MG_FLAG_DEVICE_ONLY) */
  double ms_total;      /* whole call, device-side */
  uint64_t total_tris;  /* before simplification */
  uint64_t total_verts; /* before simplification */
  uint64_t n_labels;
  uint64_t bytes_read_algorithmic; /* sx*sy*sz * sizeof(label) */
  double ms_labelmap;   /* label map: table upload + build + volume pass,
                           after H2D/dust and before pass 1 (0 if no map;
                           also inside ms_total) */
  double ms_fill;       /* fill_holes: label ids + rounds + hole volume,
                           after the label map and before pass 1 (0 without
                           fill; also inside ms_total) */
  double ms_encode;     /* mg_mesh_chunk_encoded: the encode kernels, after
                           the simplifier (0 for every other call; also
                           inside ms_total). ms_d2h is then the download of
                           the blob and the per-label tables. */
  uint64_t weld_lds_labels;   /* labels welded through a per-label LDS table */
  uint64_t weld_table_labels; /* labels above weld_lds_cap vertices, welded
                                 through the global direct-addressed table */
  uint64_t weld_lds_cap;      /* vertex cap of the LDS weld's top band; the two
                                 bands below end at a half and a quarter of it */
} mg_stats;

/* Fragment encoding on the device (mg_mesh_chunk_encoded). The numbers are
 * final: the caller has applied formats/draco.py's own defaulting. */
#define MG_ENC_PRECOMPUTED 0u  /* u32 nv | 3*nv f32 | 3*nf u32 */
#define MG_ENC_DRACO       1u  /* formats/draco.py encode, float path */
typedef struct {
  uint32_t format;       /* MG_ENC_* */
  float    shift[3];     /* added to every vertex, one f32 add each */
  double   q_origin[3];  /* draco only: quantization origin */
  double   q_range;      /* draco only: quantization range, > 0 */
  uint32_t q_bits;       /* draco only: 1..32 */
} mg_encode_params;

/* Every label's finished fragment. Entry i (labels ascending) is the
 * size[i] bytes at blob + offset[i]; entries do not overlap and lie in the
 * blob in an order of the engine's choosing. bbox holds
 * [min x, min y, min z, max x, max y, max z] of the shifted vertices per
 * entry. A label without vertices has size 0 and a zero box. The blob is
 * CTX-OWNED pinned staging under the meshset's lifetime rule (valid until
 * the next call on the ctx); the tables live in the descriptor allocation,
 * which mg_blobset_free frees. */
typedef struct {
  uint32_t  n;
  uint64_t *labels;      /* [n] ascending */
  uint64_t *offset;      /* [n] into blob */
  uint64_t *size;        /* [n] */
  uint32_t *nverts;      /* [n] */
  uint32_t *ntris;       /* [n] */
  float    *bbox;        /* [6n] */
  uint8_t  *blob;
  uint64_t  blob_bytes;
} mg_blobset;

/* Label selection folded into one lookup table (replaces the host
 * fastremap sequence of mesh.py:200-204 and 357-369). Every voxel is
 * looked up ONCE with its raw label — no chaining: {a:b, b:c} sends a->b
 * and b->c. Labels absent from the table follow the miss policy. Label 0
 * is never looked up and stays 0. */
#define MG_MAP_MISS_KEEP 0u   /* absent labels stay (exclude_object_ids) */
#define MG_MAP_MISS_ZERO 1u   /* absent labels are erased (remap_table,
                                 object_ids) */
typedef struct {
  const uint64_t *keys;   /* n distinct non-zero labels (host) */
  const uint64_t *vals;   /* n replacement labels, 0 = erase   */
  uint64_t        n;      /* 0 is valid                        */
  uint32_t        miss;   /* MG_MAP_MISS_*                     */
} mg_label_map;

/* Create a context on HIP device device_id (0-based). Returns NULL on
 * failure (no device, no HIP). */
mg_ctx  *mg_init(int device_id);
void     mg_destroy(mg_ctx *ctx);

/* Mesh every non-zero label of an F-order label volume.
 *   labels        host pointer, sx*sy*sz elements, F-order (x fastest)
 *   sx,sy,sz      dimensions INCLUDING any overlap padding (<= 2047 each)
 *   dtype         MG_U32 | MG_U64
 *   rx,ry,rz      resolution in nm per voxel (anisotropy, mesh.py:151)
 *   reduction_factor  target triangle reduction (0/1 = no simplification;
 *                     mesh.py:376-381 'reduction_factor')
 *   max_error     max simplification error in nm (mesh.py 'max_error')
 *   voxel_centered nonzero: voxel centers at integer coordinates
 *                  (mesh.py:380 voxel_centered=True)
 *   dust_threshold 0 = off; else labels with fewer voxels than this are
 *                  zeroed ON DEVICE before meshing (the reference's
 *                  dust_threshold preprocessing, mesh.py:313-323 via
 *                  fastremap — here three HIP volume passes instead of
 *                  a multi-second host unique/mask)
 *   flags         MG_FLAG_*
 *   out           receives the meshset (caller frees)
 * Returns 0 on success. */
int mg_mesh_chunk(mg_ctx *ctx, const void *labels,
                  int sx, int sy, int sz, int dtype,
                  float rx, float ry, float rz,
                  uint32_t reduction_factor, float max_error,
                  int voxel_centered, uint64_t dust_threshold,
                  uint32_t flags,
                  mg_meshset **out);

/* mg_mesh_chunk with a label map (NULL = none, identical to
 * mg_mesh_chunk). Device order: H2D -> dust passes (counting RAW labels,
 * mesh.py:193-198) -> label map in place -> count/emit pipeline — the
 * reference's dust -> remap -> object_ids -> exclude_object_ids order
 * (mesh.py:193-204).
 * Errors (non-zero return + mg_last_error, never a fault): a zero key, a
 * duplicate key, miss outside MG_MAP_MISS_*, a value >= 2^32 with MG_U32,
 * more than 2^24 entries, or a map combined with MG_FLAG_SKIP_H2D (the
 * map is not idempotent on an already-mapped resident volume). */
int mg_mesh_chunk_mapped(mg_ctx *ctx, const void *labels,
                         int sx, int sy, int sz, int dtype,
                         float rx, float ry, float rz,
                         uint32_t reduction_factor, float max_error,
                         int voxel_centered, uint64_t dust_threshold,
                         uint32_t flags,
                         const mg_label_map *map,
                         mg_meshset **out);

/* mg_mesh_chunk_mapped with hole filling (fill_level 0 = none, identical
 * to mg_mesh_chunk_mapped). Replaces fastmorph.fill_holes_v2 + the mesher
 * call on filled_labels (mesh.py:220-232). Device order: H2D -> dust ->
 * label map -> fill -> count/emit/.../extract on the FILLED volume. The
 * hole volume (input label where the fill changed it, else 0) stays
 * resident on the ctx for one mg_mesh_holes call.
 * fill_level 1: rounds to a fixed point; 2: the six boundary slices are
 * filled in 2-D first (fix_borders). Errors: fill_level > 2, or
 * fill_level > 0 combined with MG_FLAG_SKIP_H2D. */
int mg_mesh_chunk_filled(mg_ctx *ctx, const void *labels,
                         int sx, int sy, int sz, int dtype,
                         float rx, float ry, float rz,
                         uint32_t reduction_factor, float max_error,
                         int voxel_centered, uint64_t dust_threshold,
                         uint32_t flags,
                         const mg_label_map *map,
                         uint32_t fill_level,
                         mg_meshset **out);

/* mg_mesh_chunk_mapped, ending in the encoded fragments instead of the
 * meshes — replaces MeshTask's per-label host loop (mesh.py:434-448: shift
 * into global nm, bounding box, precomputed or draco encoding). The
 * pipeline is the same through the simplifier; the encode stage then writes
 * every label's bytes and box on the device, byte for byte what the host
 * loop gives for the meshes mg_mesh_chunk_mapped would return, and only the
 * blob and the per-label tables are downloaded. MG_FLAG_DEVICE_ONLY runs
 * the stage and returns an empty set; MG_FLAG_SKIP_H2D keeps its meaning.
 * There is no fill_holes variant.
 * Errors besides mg_mesh_chunk_mapped's (non-zero return + mg_last_error,
 * before any kernel, the ctx stays usable): NULL params, an unknown format,
 * a non-finite shift / q_origin / q_range, q_range <= 0, q_bits outside
 * 1..32 (the q_ fields are read for MG_ENC_DRACO only). */
int mg_mesh_chunk_encoded(mg_ctx *ctx, const void *labels,
                          int sx, int sy, int sz, int dtype,
                          float rx, float ry, float rz,
                          uint32_t reduction_factor, float max_error,
                          int voxel_centered, uint64_t dust_threshold,
                          uint32_t flags,
                          const mg_label_map *map,
                          const mg_encode_params *params,
                          mg_blobset **out);

void mg_blobset_free(mg_blobset *bs);

/* Mesh the hole volume left by the last mg_mesh_chunk_filled
 * (fill_level > 0) on this ctx — replaces Mesher.mesh(hole_labels) +
 * compute_meshes at mesh.py:234-235. The volume is already resident: no
 * upload. Consumes the stash (the hole volume becomes the ctx's resident
 * label volume); a call without a stash is an error, and any other
 * mg_mesh_chunk* / mg_fill_holes call on the ctx drops it. flags: only
 * MG_FLAG_DEVICE_ONLY is honoured. The result reuses the ctx's staging
 * like any mg_mesh_chunk: copy the filled meshset first. */
int mg_mesh_holes(mg_ctx *ctx, float rx, float ry, float rz,
                  uint32_t reduction_factor, float max_error,
                  int voxel_centered, uint32_t flags,
                  mg_meshset **out);

/* Standalone hole filling of a host volume — replaces
 * fastmorph.fill_holes_v2 at mesh.py:220 (levels 1-2 only).
 *   labels       host, sx*sy*sz elements, F-order
 *   level        1 | 2 (anything else is an error)
 *   filled_out   caller buffer, same size/dtype: the filled volume
 *   holes_out    caller buffer: labels[v] where filled[v] != labels[v]
 *   rounds_out   optional: productive 3-D rounds (rounds that rewrote)
 * More than 63 productive rounds on one block is a "did not converge"
 * error. Drops any stashed hole volume. Returns 0 on success. */
int mg_fill_holes(mg_ctx *ctx, const void *labels,
                  int sx, int sy, int sz, int dtype, uint32_t level,
                  void *filled_out, void *holes_out, uint32_t *rounds_out);

void mg_meshset_free(mg_meshset *ms);

/* Every distinct value of a label volume with its voxel count. labels[]
 * is ascending and includes 0 when the volume holds a 0 (as
 * fastremap.unique does); counts[i] voxels carry labels[i]. Both tables
 * live in the descriptor allocation, which mg_label_counts_free frees. */
typedef struct {
  uint64_t  n;
  uint64_t *labels;      /* [n] ascending */
  uint64_t *counts;      /* [n] */
} mg_label_counts;

/* Count the voxels of every label of an F-order volume (arguments as
 * mg_mesh_chunk). One device pass over runs of equal values builds the
 * label table and the histogram together; the count of 0 is the remainder.
 * flags: MG_FLAG_SKIP_H2D keeps its meaning, other bits are ignored.
 * Errors, in this order: NULL ctx / labels / out (1), dims outside 1..2047
 * (2), bad dtype (3), 2^32 or more voxels (2: device counts are 32-bit).
 * The ctx stays usable after any of them. On success the RAW volume stays
 * resident for the next call on the ctx, which may be an mg_mesh_chunk*
 * with MG_FLAG_COUNTED; the call drops a stashed hole volume.
 * mg_get_stats afterwards: ms_h2d, ms_count (the histogram pass, or
 * passes when the label table had to grow), ms_total, n_labels (distinct
 * non-zero labels) and bytes_read_algorithmic; every other field is 0. */
int mg_count_voxels(mg_ctx *ctx, const void *labels,
                    int sx, int sy, int sz, int dtype, uint32_t flags,
                    mg_label_counts **out);

void mg_label_counts_free(mg_label_counts *lc);

/* Quadric edge-collapse simplification of ONE standalone mesh on the
 * GPU — the simplifier reused at merge granularity: replaces
 * zmesh.simplify_fqmr at the multires LOD chain call site
 * (/root/reference/igneous/tasks/mesh/multires.py:342 via
 * generate_lods). Same deterministic contract as the per-label chunk
 * simplifier (oracle/simplify.c omc_simplify_mesh is the checker).
 *   verts/faces      host arrays (float32 V*3 / uint32 T*3)
 *   reduction_factor target = ntris/reduction_factor (<=1: no-op)
 *   max_error        cost bound in the verts' own units
 *   out_*            ctx-owned pinned staging, valid until the ctx's
 *                    next mg_mesh_chunk/mg_simplify_mesh call
 * Returns 0 on success. */
int mg_simplify_mesh(mg_ctx *ctx,
                     const float *verts, uint32_t nverts,
                     const uint32_t *faces, uint32_t ntris,
                     uint32_t reduction_factor, float max_error,
                     const float **out_verts, uint32_t *out_nverts,
                     const uint32_t **out_faces, uint32_t *out_ntris);

/* Grid-partition ONE mesh with triangle clipping at the cell boundaries —
 * replaces zmesh.chunk_mesh at the multires merge's two call sites
 * (the reference's igneous/tasks/mesh/multires.py:550 retriangulate_mesh
 * and :574 create_octree_level_from_mesh). Bit-equal to
 * igneous_amd.meshops.chunk_mesh (the CPU checker; contract in DESIGN.md
 * §7a): cell = floor((p - offset) / scale) in f64, Sutherland-Hodgman
 * against each overlapped cell box, fan triangulation, then a per-cell
 * exact-duplicate weld, degenerate-face drop and unused-vertex drop in
 * first-seen order.
 *   verts/faces   host arrays (float32 V*3 / uint32 T*3)
 *   scale/offset  cell size and grid anchor in the verts' units (f64)
 *   out           one mg_mesh per non-empty cell, label =
 *                 ((cx+2^20)<<42) | ((cy+2^20)<<21) | (cz+2^20), so the
 *                 ascending-label order of meshes[] is lexicographic cell
 *                 order. Storage is ctx-owned pinned staging under the
 *                 mg_simplify_mesh lifetime rule; free the descriptor with
 *                 mg_meshset_free.
 *   out_order     [nmeshes] indices into meshes[] in the checker's dict
 *                 order (cells holding an interior face first, ascending;
 *                 then the rest by first emitted fragment). Lives in the
 *                 descriptor allocation: freed by mg_meshset_free.
 * ntris == 0 returns an empty set. Errors (non-zero return +
 * mg_last_error, never a fault, rejected before any kernel runs): a face
 * index >= nverts, a non-finite vertex/scale/offset, a scale component
 * <= 0. Rejected by the first device pass: a cell coordinate outside
 * [-2^20, 2^20), more than 2^31 (face, cell) pairs, a cell bounding box
 * of more than 2^31 cells, 2^31 or more fragment corners, a clipped
 * polygon of more than 16 points. The ctx stays usable after any of them. */
int mg_chunk_mesh(mg_ctx *ctx,
                  const float *verts, uint32_t nverts,
                  const uint32_t *faces, uint32_t ntris,
                  const double scale[3], const double offset[3],
                  mg_meshset **out, const uint32_t **out_order);

/* Weld the vertices of ONE mesh that lie within `radius` of each other —
 * replaces Mesh.merge_close_vertices in the multires merge (the reference's
 * igneous/tasks/mesh/multires.py:551). Bit-equal to
 * igneous_amd.meshops.merge_close_vertices (the CPU checker; contract in
 * DESIGN.md §7a): vertices i and j are close when
 * dx*dx + dy*dy + dz*dz <= radius*radius in f64; every vertex is replaced
 * by the smallest index of its connected component of close pairs; faces
 * with two equal corners are dropped, the rest keep their order; the output
 * vertices are the representatives a surviving face uses, in ascending
 * input index, with their own stored bits.
 *   verts/faces   host arrays (float32 V*3 / uint32 T*3)
 *   radius        > 0, in the verts' units
 *   out_*         ctx-owned pinned staging under the mg_simplify_mesh
 *                 lifetime rule (valid until the next call on the ctx)
 * A mesh without faces gives 0 vertices and 0 faces.
 * Return codes, used by these two entry points only (non-zero return +
 * mg_last_error, never a fault, the ctx stays usable):
 *   100  rejected before any kernel: a face index >= nverts, a non-finite
 *        vertex, a radius that is not finite or not > 0
 *   101  device allocation or upload failed
 *   102  the grid stage (cells, sort, candidate count) failed
 *   103  rejected by the grid stage: a coordinate with |v / (2*radius)| >=
 *        2^51, or more than 2^32 candidate visits ("radius too large for
 *        this mesh": the sum, over all vertices, of the vertices sharing a
 *        grid bucket with one of its 27 neighbour cells of size 2*radius)
 *   104  the link stage failed      105  the face / vertex stage failed
 *   106  the download failed        107  the cell gather failed
 *        (mg_retriangulate_mesh)
 * besides 1 (null argument), 2 (more than 2^31 vertices or 2^31/3 faces)
 * and 4 (no device). */
int mg_merge_close_vertices(mg_ctx *ctx,
                            const float *verts, uint32_t nverts,
                            const uint32_t *faces, uint32_t ntris,
                            double radius,
                            const float **out_verts, uint32_t *out_nverts,
                            const uint32_t **out_faces, uint32_t *out_ntris);

/* Cut ONE mesh at a grid's cell boundaries and weld the pieces back into
 * one mesh — replaces the whole of retriangulate_mesh in the multires merge
 * (the reference's igneous/tasks/mesh/multires.py:546-553: zmesh.chunk_mesh,
 * Mesh.concatenate, merge_close_vertices). Bit-equal to
 * merge_close_vertices(Mesh.concatenate(*chunk_mesh(mesh, scale,
 * offset).values()), radius) of igneous_amd.meshops, the cells taken in the
 * checker's dict order (mg_chunk_mesh's out_order). The cells never leave
 * the device: only the welded mesh is downloaded.
 *   verts/faces, scale/offset   as mg_chunk_mesh
 *   radius, out_*               as mg_merge_close_vertices
 * When the chunker keeps no cell (ntris == 0, or every face degenerate) the
 * input is the result, as in the reference: the call then sets *out_verts
 * and *out_faces to NULL and *out_nverts / *out_ntris to the INPUT counts.
 * A non-NULL *out_verts is always the welded mesh, even an empty one.
 * Errors: mg_chunk_mesh's (60-73) and mg_merge_close_vertices' (100-107). */
int mg_retriangulate_mesh(mg_ctx *ctx,
                          const float *verts, uint32_t nverts,
                          const uint32_t *faces, uint32_t ntris,
                          const double scale[3], const double offset[3],
                          double radius,
                          const float **out_verts, uint32_t *out_nverts,
                          const uint32_t **out_faces, uint32_t *out_ntris);

/* One level of one mesh's multires octree: where it is cut and how its
 * fragments are quantised (the arguments of the reference's
 * igneous/tasks/mesh/multires.py:556-585 create_octree_level_from_mesh and
 * of the to_stored_model_space + DracoPy.encode loop at :152-174). */
typedef struct mg_octree_level {
  double   scale[3];        /* cell size of this level: chunk_shape * 2^lod */
  double   offset[3];       /* grid anchor (the manifest's grid_origin) */
  uint32_t retriangulate;   /* lod > 0: first cut at upper_scale and weld */
  double   upper_scale[3];  /* cell size of the level below: scale / 2 */
  double   radius;          /* the weld's radius (the reference's 1e-5) */
  uint32_t chunked;         /* 0: the coarsest level, one fragment at (0,0,0) */
  double   q_origin[3];     /* grid_origin */
  double   q_voffset[3];    /* the level's vertex_offsets entry */
  double   q_cell[3];       /* chunk_shape * lod_scale, as one f64 product */
  uint32_t q_bits;          /* vertex_quantization_bits, 1..32 */
  /* Optional. cmp_zorder is a total order only while no axis holds cells of
   * both signs; where one does, the result of a comparison sort depends on
   * the sort's algorithm and on the order it is handed the cells in. The
   * engine then calls order_cells with the n cells (3 i32 each) in
   * mg_chunk_mesh's dict order, and it stores in order[r] the index of the
   * cell that comes r-th; a non-zero return fails the call. NULL, and
   * wherever cmp_zorder is a total order: the engine's own sort by the
   * z-order of the coordinates biased by 2^20, which is cmp_zorder's order
   * there. Grids anchored at the mesh's minimum, as the merge anchors them,
   * have no negative cell and never reach the callback. */
  int (*order_cells)(const int32_t *nodes, uint32_t n, uint32_t *order,
                     void *arg);
  void    *order_arg;
} mg_octree_level;

/* The finished fragments of one octree level, in z-order. The tables live in
 * the descriptor allocation (mg_fragset_free); the blob is ctx-owned pinned
 * staging under the mg_simplify_mesh lifetime rule. */
typedef struct mg_fragset {
  uint32_t  n;
  int32_t  *nodes;       /* [3n] fragment_positions of the level */
  uint64_t *offset;      /* [n] start of the fragment in blob */
  uint64_t *size;        /* [n] bytes: the level's fragment_offsets slice */
  uint32_t *nverts;      /* [n] */
  uint32_t *ntris;       /* [n] */
  const uint8_t *blob;   /* b"".join(mesh_binaries) of the level */
  uint64_t  blob_bytes;
} mg_fragset;

/* Encode ONE level of one mesh's multires octree on the device — replaces,
 * for one lod, create_octree_level_from_mesh (the reference's
 * igneous/tasks/mesh/multires.py:556-585: retriangulate_mesh,
 * zmesh.chunk_mesh, the cmp_zorder sort) and the per-fragment
 * to_stored_model_space + DracoPy.encode loop of process_mesh (:152-174).
 * The mesh is uploaded once and stays on the device between the
 * retriangulation, the chunker and the encode; only the tables and the blob
 * come back. Byte-equal to the host sequence (contract in DESIGN.md §7a):
 *   1. lv->retriangulate: M <- mg_retriangulate_mesh(M, upper_scale, offset,
 *      radius); M stays when the chunker keeps no cell
 *   2. lv->chunked == 0: one fragment, M itself, at node (0, 0, 0);
 *      otherwise the cells of mg_chunk_mesh(M, scale, offset) sorted by
 *      cmp_zorder on (cx, cy, cz)
 *   3. per fragment with node p, in f64, one IEEE operation per step:
 *      clip(rint(((((v - q_origin) - q_voffset) / q_cell) - p) * qmax),
 *      0, qmax) as u32, qmax = 2^q_bits - 1
 *   4. per fragment the draco bytes of integer positions: 11-byte header,
 *      varint nf, varint nv, u8 1, indices at u8 / u16 / varint / u32 by
 *      nv < 2^8 / 2^16 / 2^21 / else, the 10-byte attribute header
 *      (DT_UINT32, sequential INTEGER, prediction -2, uncompressed), 3*nv
 *      u32 — no trailer. A fragment without faces (the unchunked fragment of
 *      a mesh without faces) has size 0.
 *   5. the fragments lie in blob in z-order, back to back from offset 0
 * An empty chunked level gives n == 0. Return codes (non-zero return +
 * mg_last_error, never a fault, the ctx stays usable):
 *   110  rejected before any kernel: q_bits outside 1..32, a non-finite
 *        q_origin / q_voffset / q_cell, a q_cell component <= 0
 *   111  device allocation or a table upload failed
 *   112  the order_cells callback failed or returned no permutation
 *   113  the encode kernels or the size scan failed
 *   114  the download failed       115  out of host memory
 * besides 1, 2 and 4 as above, mg_chunk_mesh's (60-73: 60 also rejects, before
 * any kernel, a face index >= nverts and a non-finite vertex, scale,
 * upper_scale or offset) and mg_merge_close_vertices' (100-107). */
int mg_encode_octree_level(mg_ctx *ctx,
                           const float *verts, uint32_t nverts,
                           const uint32_t *faces, uint32_t ntris,
                           const mg_octree_level *lv, mg_fragset **out);

void mg_fragset_free(mg_fragset *fs);

/* Stats of the last mg_mesh_chunk on this ctx. Returns 0 on success. */
int mg_get_stats(mg_ctx *ctx, mg_stats *out);

/* Error text of the last failed call on this ctx (thread-local static
 * lifetime; valid until the next call on the ctx). */
const char *mg_last_error(mg_ctx *ctx);

/* Engine/device identification (for logging + the bench line). */
int mg_device_count(void);
const char *mg_version(void);

#ifdef __cplusplus
}
#endif

#endif /* MESHGINE_H */
