// chunk_mesh.hip — grid-chunk and clip one mesh on the device (the
// multires merge's zmesh.chunk_mesh call sites, reference multires.py:550
// and :574). Included from meshgine.hip after the ctx helpers (mg_ctx.h):
// the kernels first, then their host driver.
//
// Contract: bit-equal to igneous_amd/meshops.py
// chunk_mesh + consolidate — the same cells, the same dict order, the same
// f32 vertex bits, the same u32 faces. Every f64 operation below is one
// IEEE operation written the way the host function writes it
// (-ffp-contract=off keeps a*b+c two roundings).
//
// Units of work:
//   face      one input triangle
//   pair      one (face, overlapped cell) combination, numbered face-major
//             with the cell loop cx, cy, cz (cz innermost) inside a face —
//             ascending pair number IS the host's emit order
//   fragment  a pair's clipped polygon (k points, 0 when fewer than 3)
//   corner    one polygon point; corner j >= 2 of a fragment also stands
//             for the fan triangle (0, j-1, j)
//
// Schedule (kernel boundaries order the phases; no spin flags, no grid
// sync, every loop bounded; atomics are min/max/or/count only):
//   k_cm_face_count   per face: cell range, pair count, mesh cell bbox
//   scan              pair offsets
//   k_cm_pair         per pair: clip in registers/scratch -> point count,
//                     sort key (dense cell id << 1 | is_boundary)
//   sort_pairs        stable by key: per-cell stream order
//   k_cm_frag_gather  point counts in stream order, cell-head flags
//   scan x2           corner offsets, cell ordinals
//   k_cm_emit         re-clip, f32 corners in stream order
//   4 x (k_cm_weld_key + sort_pairs)   LSD sort of corners by
//                     (cell, x, y, z), -0 canonicalised, stable from
//                     stream order: a run's head is its first occurrence
//   k_cm_heads, scan, k_cm_head_pos, k_cm_rep   corner -> first corner
//   k_cm_faces        fan faces, degenerate drop, used-vertex flags
//   scan x2           vertex ids, face slots
//   k_cm_write        per-cell vertex and face slices
//   k_cm_cell_meta    per-cell bases for the host descriptor

#include <cmath>

#define CM_BLK 256
#define CM_MAXPTS 16               // per-thread polygon capacity (points)
#define CM_CELL_LIM 1048576.0      // cell coordinates live in [-2^20, 2^20)
#define CM_MAX_PAIRS (1ull << 31)
#define CM_MAX_DENSE (1ull << 31)  // cells of the mesh's cell bounding box
#define CM_MAX_CORNERS (1ull << 31)

#define CM_ERR_CELL_RANGE 1u
#define CM_ERR_FACE_CELLS 2u
#define CM_ERR_POLY_OVERFLOW 4u

struct CmGrid {
  double scale[3];
  double offset[3];
};

// dense numbering of the cells inside the mesh's cell bounding box,
// lexicographic in (cx, cy, cz)
struct CmDense {
  int lo[3];
  uint32_t ny, nz;
};

// scalars the host reads back; one 64-byte block at cm_misc
struct CmMisc {
  unsigned long long pairs;    // sum of per-face cell counts
  unsigned long long corners;  // sum of fragment point counts
  int bb_lo[3];
  int bb_hi[3];
  uint32_t err;
  uint32_t pad[5];
};

static inline uint32_t cm_blocks(uint64_t n) {
  return (uint32_t)((n + CM_BLK - 1) / CM_BLK);
}

// Cell range of face f (meshops.py:116-121). Returns false when a cell
// coordinate leaves [-2^20, 2^20); lo/hi are then zeroed.
__device__ __forceinline__ bool cm_face_range(
    const float *__restrict__ verts, const uint32_t *__restrict__ faces,
    uint64_t f, const CmGrid &g, double tri[3][3], int lo[3], int hi[3]) {
  for (int v = 0; v < 3; ++v) {
    uint64_t vi = faces[3 * f + v];
    for (int a = 0; a < 3; ++a) tri[v][a] = (double)verts[3 * vi + a];
  }
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    double mn = fmin(fmin(tri[0][a], tri[1][a]), tri[2][a]);
    double mx = fmax(fmax(tri[0][a], tri[1][a]), tri[2][a]);
    double l = floor((mn - g.offset[a]) / g.scale[a]);
    double h = floor((mx - g.offset[a]) / g.scale[a] - 1e-12);
    h = fmax(h, l);
    if (!(l >= -CM_CELL_LIM && h < CM_CELL_LIM)) ok = false;
    lo[a] = ok ? (int)l : 0;
    hi[a] = ok ? (int)h : 0;
  }
  if (!ok)
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = 0;
  return ok;
}

// One Sutherland-Hodgman pass against an axis plane (meshops.py:82-98).
// Never writes past CM_MAXPTS points; *ovf reports a dropped point.
__device__ __forceinline__ int cm_clip_axis(const double (*in)[3], int n,
                                            double (*out)[3], int a,
                                            double bound, bool keep_below,
                                            bool *ovf) {
  int m = 0;
  for (int i = 0; i < n; ++i) {
    const double *cur = in[i];
    const double *nxt = in[i + 1 == n ? 0 : i + 1];
    bool cin = keep_below ? (cur[a] <= bound) : (cur[a] >= bound);
    bool nin = keep_below ? (nxt[a] <= bound) : (nxt[a] >= bound);
    if (cin) {
      if (m < CM_MAXPTS) {
        out[m][0] = cur[0];
        out[m][1] = cur[1];
        out[m][2] = cur[2];
        ++m;
      } else {
        *ovf = true;
      }
    }
    if (cin != nin) {
      double t = (bound - cur[a]) / (nxt[a] - cur[a]);
      if (m < CM_MAXPTS) {
        for (int k = 0; k < 3; ++k) {
          double d = nxt[k] - cur[k];
          double td = t * d;
          out[m][k] = cur[k] + td;
        }
        ++m;
      } else {
        *ovf = true;
      }
    }
  }
  return m;
}

// Clip the triangle in A against cell (cx,cy,cz) (meshops.py:164-172).
// The result is left in A; returns its point count, 0 if fewer than 3.
__device__ __forceinline__ int cm_clip_cell(double (*A)[3], double (*B)[3],
                                            const CmGrid &g, const int cell[3],
                                            bool *ovf) {
  int n = 3;
  for (int a = 0; a < 3; ++a) {
    double cs = (double)cell[a] * g.scale[a];
    double bmin = g.offset[a] + cs;
    double bmax = bmin + g.scale[a];
    int m = cm_clip_axis(A, n, B, a, bmin, false, ovf);
    n = cm_clip_axis(B, m, A, a, bmax, true, ovf);
    if (n < 3) break;
  }
  return n >= 3 ? n : 0;
}

// the face owning pair p: largest f with pair_off[f] <= p (pair_off is
// strictly increasing, pair_off[ntris] = number of pairs)
__device__ __forceinline__ uint32_t cm_face_of_pair(
    const uint32_t *__restrict__ pair_off, uint32_t ntris, uint32_t p) {
  uint32_t lo = 0, hi = ntris;  // answer in [lo, hi)
  for (int it = 0; it < 32 && hi - lo > 1; ++it) {
    uint32_t mid = lo + (hi - lo) / 2;
    if (pair_off[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// cell q of a face's range, in the host's loop order (cx outer, cz inner)
__device__ __forceinline__ void cm_cell_of(const int lo[3], const int hi[3],
                                           uint32_t q, int cell[3]) {
  uint32_t dy = (uint32_t)(hi[1] - lo[1]) + 1u;
  uint32_t dz = (uint32_t)(hi[2] - lo[2]) + 1u;
  cell[2] = lo[2] + (int)(q % dz);
  uint32_t r = q / dz;
  cell[1] = lo[1] + (int)(r % dy);
  cell[0] = lo[0] + (int)(r / dy);
}

__global__ __launch_bounds__(CM_BLK) void k_cm_face_count(
    const float *__restrict__ verts, const uint32_t *__restrict__ faces,
    uint32_t ntris, CmGrid g, uint32_t *__restrict__ ncells, CmMisc *misc) {
  __shared__ int s_lo[3], s_hi[3];
  if (threadIdx.x < 3) {
    s_lo[threadIdx.x] = INT32_MAX;
    s_hi[threadIdx.x] = INT32_MIN;
  }
  __syncthreads();
  uint64_t f = (uint64_t)blockIdx.x * CM_BLK + threadIdx.x;
  if (f < ntris) {
    double tri[3][3];
    int lo[3], hi[3];
    uint32_t nc = 1;
    if (!cm_face_range(verts, faces, f, g, tri, lo, hi)) {
      atomicOr(&misc->err, CM_ERR_CELL_RANGE);
    } else {
      uint64_t n64 = (uint64_t)(hi[0] - lo[0] + 1) *
                     (uint64_t)(hi[1] - lo[1] + 1) *
                     (uint64_t)(hi[2] - lo[2] + 1);
      if (n64 > CM_MAX_PAIRS) {
        atomicOr(&misc->err, CM_ERR_FACE_CELLS);
      } else {
        nc = (uint32_t)n64;
        for (int a = 0; a < 3; ++a) {
          atomicMin(&s_lo[a], lo[a]);
          atomicMax(&s_hi[a], hi[a]);
        }
      }
    }
    ncells[f] = nc;
    atomicAdd(&misc->pairs, (unsigned long long)nc);
  } else if (f == ntris) {
    ncells[f] = 0;  // scan terminator: pair_off[ntris] = total
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_lo[threadIdx.x] <= s_hi[threadIdx.x]) {
    atomicMin(&misc->bb_lo[threadIdx.x], s_lo[threadIdx.x]);
    atomicMax(&misc->bb_hi[threadIdx.x], s_hi[threadIdx.x]);
  }
}

// decode pair p into its face's corners and its cell; returns whether the
// face is interior (one cell on every axis)
__device__ __forceinline__ bool cm_pair_setup(
    const float *__restrict__ verts, const uint32_t *__restrict__ faces,
    const uint32_t *__restrict__ pair_off, uint32_t ntris, const CmGrid &g,
    uint32_t p, double tri[3][3], int cell[3], uint32_t *p_face) {
  uint32_t f = cm_face_of_pair(pair_off, ntris, p);
  int lo[3], hi[3];
  (void)cm_face_range(verts, faces, f, g, tri, lo, hi);
  cm_cell_of(lo, hi, p - pair_off[f], cell);
  *p_face = f;
  return lo[0] == hi[0] && lo[1] == hi[1] && lo[2] == hi[2];
}

__global__ __launch_bounds__(CM_BLK) void k_cm_pair(
    const float *__restrict__ verts, const uint32_t *__restrict__ faces,
    const uint32_t *__restrict__ pair_off, uint32_t ntris, uint32_t npairs,
    CmGrid g, CmDense dn, uint32_t *__restrict__ keys,
    uint32_t *__restrict__ vals, uint32_t *__restrict__ npts, CmMisc *misc) {
  uint64_t p = (uint64_t)blockIdx.x * CM_BLK + threadIdx.x;
  if (p >= npairs) return;
  double A[CM_MAXPTS][3], B[CM_MAXPTS][3];
  int cell[3];
  uint32_t f;
  bool interior = cm_pair_setup(verts, faces, pair_off, ntris, g,
                                (uint32_t)p, A, cell, &f);
  int k = 3;
  if (!interior) {
    bool ovf = false;
    k = cm_clip_cell(A, B, g, cell, &ovf);
    if (ovf) {
      atomicOr(&misc->err, CM_ERR_POLY_OVERFLOW);
      k = 0;
    }
  }
  uint32_t dense = ((uint32_t)(cell[0] - dn.lo[0]) * dn.ny +
                    (uint32_t)(cell[1] - dn.lo[1])) * dn.nz +
                   (uint32_t)(cell[2] - dn.lo[2]);
  keys[p] = (dense << 1) | (interior ? 0u : 1u);
  vals[p] = (uint32_t)p;
  npts[p] = (uint32_t)k;
  atomicAdd(&misc->corners, (unsigned long long)k);
}

// point counts in stream order + cell-head flags (index npairs: scan
// terminators)
__global__ void k_cm_frag_gather(const uint32_t *__restrict__ keys_s,
                                 const uint32_t *__restrict__ order,
                                 const uint32_t *__restrict__ npts,
                                 uint32_t npairs,
                                 uint32_t *__restrict__ npts_s,
                                 uint32_t *__restrict__ head) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < npairs) {
    npts_s[i] = npts[order[i]];
    head[i] = (i == 0 || (keys_s[i] >> 1) != (keys_s[i - 1] >> 1)) ? 1u : 0u;
  } else if (i == npairs) {
    npts_s[i] = 0;
    head[i] = 0;
  }
}

// per-cell table, five sub-arrays of stride (ncellp + 1)
enum { CM_CELL_C0 = 0, CM_CELL_DENSE, CM_CELL_FIRSTP, CM_CELL_VB, CM_CELL_FB,
       CM_CELL_FIELDS };

__global__ __launch_bounds__(CM_BLK) void k_cm_emit(
    const float *__restrict__ verts, const uint32_t *__restrict__ faces,
    const uint32_t *__restrict__ pair_off, uint32_t ntris, uint32_t npairs,
    CmGrid g, const uint32_t *__restrict__ keys_s,
    const uint32_t *__restrict__ order, const uint32_t *__restrict__ coff,
    const uint32_t *__restrict__ head, const uint32_t *__restrict__ cord_x,
    uint32_t ncorners, uint32_t cstride, float *__restrict__ pos,
    uint32_t *__restrict__ cfrag, uint32_t *__restrict__ ccell,
    uint32_t *__restrict__ cells) {
  uint64_t i = (uint64_t)blockIdx.x * CM_BLK + threadIdx.x;
  if (i >= npairs) return;
  uint32_t ord = cord_x[i] + head[i] - 1u;  // cell ordinal of fragment i
  uint32_t c0 = coff[i];
  uint32_t k = coff[i + 1] - c0;
  if (head[i]) {
    cells[(uint64_t)CM_CELL_C0 * cstride + ord] = c0;
    cells[(uint64_t)CM_CELL_DENSE * cstride + ord] = keys_s[i];
  }
  if (k == 0) return;
  double A[CM_MAXPTS][3], B[CM_MAXPTS][3];
  int cell[3];
  uint32_t f;
  bool interior = cm_pair_setup(verts, faces, pair_off, ntris, g, order[i],
                                A, cell, &f);
  int n = 3;
  if (!interior) {
    bool ovf = false;
    n = cm_clip_cell(A, B, g, cell, &ovf);
  }
  // same inputs, same arithmetic as k_cm_pair: n == k. The bound keeps the
  // writes inside the fragment's slice whatever happens.
  for (uint32_t j = 0; j < k && j < (uint32_t)n && j < CM_MAXPTS; ++j) {
    uint64_t c = (uint64_t)c0 + j;
    if (c >= ncorners) break;
    pos[3 * c + 0] = (float)A[j][0];
    pos[3 * c + 1] = (float)A[j][1];
    pos[3 * c + 2] = (float)A[j][2];
    cfrag[c] = (uint32_t)i;
    ccell[c] = ord;
  }
}

__device__ __forceinline__ uint32_t cm_canon(float v) {
  uint32_t b = __float_as_uint(v);
  return b == 0x80000000u ? 0u : b;  // -0.0 equals +0.0
}

// key of weld sort pass `which` (0: z, 1: y, 2: x, 3: cell ordinal) for
// the corners in their current order
__global__ void k_cm_weld_key(const uint32_t *__restrict__ cur,
                              const float *__restrict__ pos,
                              const uint32_t *__restrict__ ccell,
                              uint32_t ncorners, int which,
                              uint32_t *__restrict__ keys) {
  uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncorners) return;
  uint32_t c = cur[j];
  keys[j] = which == 3 ? ccell[c] : cm_canon(pos[3ull * c + (2 - which)]);
}

// run heads of the (cell, x, y, z)-sorted corners (index ncorners: scan
// terminator)
__global__ void k_cm_heads(const uint32_t *__restrict__ sorted,
                           const float *__restrict__ pos,
                           const uint32_t *__restrict__ ccell,
                           uint32_t ncorners, uint32_t *__restrict__ head) {
  uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j > ncorners) return;
  uint32_t h = 0;
  if (j < ncorners) {
    h = 1;
    if (j > 0) {
      uint32_t a = sorted[j], b = sorted[j - 1];
      h = (ccell[a] != ccell[b] ||
           cm_canon(pos[3ull * a + 0]) != cm_canon(pos[3ull * b + 0]) ||
           cm_canon(pos[3ull * a + 1]) != cm_canon(pos[3ull * b + 1]) ||
           cm_canon(pos[3ull * a + 2]) != cm_canon(pos[3ull * b + 2]))
              ? 1u : 0u;
    }
  }
  head[j] = h;
}

__global__ void k_cm_head_pos(const uint32_t *__restrict__ sorted,
                              const uint32_t *__restrict__ head,
                              const uint32_t *__restrict__ run_x,
                              uint32_t ncorners,
                              uint32_t *__restrict__ head_pos) {
  uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < ncorners && head[j]) head_pos[run_x[j]] = sorted[j];
}

// rep[c] = the first corner (stream position) of c's cell with c's position
__global__ void k_cm_rep(const uint32_t *__restrict__ sorted,
                         const uint32_t *__restrict__ head,
                         const uint32_t *__restrict__ run_x,
                         const uint32_t *__restrict__ head_pos,
                         uint32_t ncorners, uint32_t *__restrict__ rep) {
  uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < ncorners) rep[sorted[j]] = head_pos[run_x[j] + head[j] - 1u];
}

// Fan triangle (0, j-1, j) at corner j >= 2 of each fragment: keep flag
// after the weld, used flags on the welded vertices. Also records each
// cell's first emitted pair (the host's dict order). `used` is zeroed by
// the driver; index ncorners of keep is the scan terminator.
__global__ void k_cm_faces(const uint32_t *__restrict__ cfrag,
                           const uint32_t *__restrict__ ccell,
                           const uint32_t *__restrict__ coff,
                           const uint32_t *__restrict__ order,
                           const uint32_t *__restrict__ rep,
                           uint32_t ncorners, uint32_t cstride,
                           uint32_t *__restrict__ keep,
                           uint32_t *__restrict__ used,
                           uint32_t *__restrict__ cells) {
  uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > ncorners) return;
  if (c == ncorners) {
    keep[c] = 0;
    return;
  }
  uint32_t i = cfrag[c];
  uint32_t c0 = coff[i];
  uint32_t ord = ccell[c];
  if (c == cells[(uint64_t)CM_CELL_C0 * cstride + ord])
    cells[(uint64_t)CM_CELL_FIRSTP * cstride + ord] = order[i];
  uint32_t kp = 0;
  if (c - c0 >= 2) {
    uint32_t a = rep[c0], b = rep[c - 1], d = rep[c];
    if (a != b && b != d && a != d) {
      kp = 1;
      used[a] = 1;
      used[b] = 1;
      used[d] = 1;
    }
  }
  keep[c] = kp;
}

__global__ void k_cm_write(const uint32_t *__restrict__ cfrag,
                           const uint32_t *__restrict__ ccell,
                           const uint32_t *__restrict__ coff,
                           const uint32_t *__restrict__ rep,
                           const uint32_t *__restrict__ keep,
                           const uint32_t *__restrict__ used,
                           const uint32_t *__restrict__ vid_x,
                           const uint32_t *__restrict__ fslot_x,
                           const float *__restrict__ pos,
                           const uint32_t *__restrict__ cells,
                           uint32_t ncorners, float *__restrict__ out_v,
                           uint32_t *__restrict__ out_f) {
  uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncorners) return;
  if (used[c]) {
    uint64_t v = vid_x[c];
    out_v[3 * v + 0] = pos[3 * c + 0];
    out_v[3 * v + 1] = pos[3 * c + 1];
    out_v[3 * v + 2] = pos[3 * c + 2];
  }
  if (keep[c]) {
    uint32_t c0 = coff[cfrag[c]];
    uint32_t vb = vid_x[cells[ccell[c]]];  // CM_CELL_C0 sub-array
    uint64_t t = fslot_x[c];
    out_f[3 * t + 0] = vid_x[rep[c0]] - vb;
    out_f[3 * t + 1] = vid_x[rep[c - 1]] - vb;
    out_f[3 * t + 2] = vid_x[rep[c]] - vb;
  }
}

// vertex / face base of every cell; entry ncellp holds the totals
__global__ void k_cm_cell_meta(const uint32_t *__restrict__ vid_x,
                               const uint32_t *__restrict__ fslot_x,
                               uint32_t ncellp, uint32_t ncorners,
                               uint32_t cstride,
                               uint32_t *__restrict__ cells) {
  uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o > ncellp) return;
  uint32_t c0 = o == ncellp ? ncorners
                            : cells[(uint64_t)CM_CELL_C0 * cstride + o];
  cells[(uint64_t)CM_CELL_VB * cstride + o] = vid_x[c0];
  cells[(uint64_t)CM_CELL_FB * cstride + o] = fslot_x[c0];
}

// ---------------------------------------------------------------------------
// host driver

struct CmCall {
  uint32_t nverts, ntris;
  CmGrid g;
  CmDense dn;
  uint64_t ndense;   // cells in the mesh's cell bounding box
  uint32_t P;        // pairs
  uint32_t C;        // corners
  uint32_t ncellp;   // cells that received a fragment
};

static inline unsigned cm_bits(uint64_t nvalues) {  // bits to hold 0..n-1
  unsigned b = 1;
  while (b < 32 && (1ull << b) < nvalues) ++b;
  return b;
}

// Host-side validation: nothing out of contract reaches a kernel.
static int cm_validate(mg_ctx *c, const float *verts, uint32_t nverts,
                       const uint32_t *faces, uint32_t ntris,
                       const double scale[3], const double offset[3]) {
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(scale[a]) || !std::isfinite(offset[a])) {
      SET_ERR(c, "chunk_mesh: non-finite scale/offset on axis %d", a);
      return 60;
    }
    if (!(scale[a] > 0.0)) {
      SET_ERR(c, "chunk_mesh: scale[%d] = %g must be > 0", a, scale[a]);
      return 60;
    }
  }
  for (uint64_t i = 0; i < 3ull * ntris; ++i) {
    if (faces[i] >= nverts) {
      SET_ERR(c, "chunk_mesh: face %llu references vertex %u >= nverts %u",
              (unsigned long long)(i / 3), faces[i], nverts);
      return 60;
    }
  }
  for (uint64_t i = 0; i < 3ull * nverts; ++i) {
    if (!std::isfinite(verts[i])) {
      SET_ERR(c, "chunk_mesh: vertex %llu is not finite",
              (unsigned long long)(i / 3));
      return 60;
    }
  }
  return 0;
}

// room for a mesh of V vertices and T faces in cm_verts / cm_faces
static int cm_ensure_input(mg_ctx *c, uint64_t V, uint64_t T) {
  if (ensure(c, c->cm_verts, 3 * V + 3)) return 61;
  if (ensure(c, c->cm_faces, 3 * T + 3)) return 61;
  return 0;
}

// [0] upload of the caller's mesh into cm_verts / cm_faces
static int cm_upload(mg_ctx *c, const float *verts, uint32_t nverts,
                     const uint32_t *faces, uint32_t ntris) {
  hipStream_t s = c->stream;
  if (int e = cm_ensure_input(c, nverts, ntris)) return e;
  HIP_TRY(c, hipMemcpyAsync(c->cm_verts.get(), verts, (uint64_t)nverts * 12,
                            hipMemcpyHostToDevice, s), 61);
  HIP_TRY(c, hipMemcpyAsync(c->cm_faces.get(), faces, (uint64_t)ntris * 12,
                            hipMemcpyHostToDevice, s), 61);
  return 0;
}

// [1] per-face cell ranges, pair offsets, cell bounding box of the mesh in
// cm_verts / cm_faces
static int cm_count(mg_ctx *c, CmCall &k) {
  hipStream_t s = c->stream;
  const uint64_t T = k.ntris;
  if (ensure(c, c->cm_ncells, T + 1)) return 61;
  if (ensure(c, c->cm_pair_off, T + 1)) return 61;
  if (ensure(c, c->cm_misc, 1)) return 61;
  CmMisc init = {};
  for (int a = 0; a < 3; ++a) {
    init.bb_lo[a] = INT32_MAX;
    init.bb_hi[a] = INT32_MIN;
  }
  HIP_TRY(c, hipMemcpyAsync(c->cm_misc.get(), &init, sizeof(init),
                            hipMemcpyHostToDevice, s), 61);
  hipLaunchKernelGGL(k_cm_face_count, dim3(cm_blocks(T + 1)), dim3(CM_BLK), 0,
                     s, c->cm_verts.get(), c->cm_faces.get(), k.ntris, k.g,
                     c->cm_ncells.get(), c->cm_misc.get());
  CmMisc m;
  HIP_TRY(c, hipMemcpyAsync(&m, c->cm_misc.get(), sizeof(m),
                            hipMemcpyDeviceToHost, s), 61);
  HIP_TRY(c, hipStreamSynchronize(s), 61);
  if (m.err & CM_ERR_CELL_RANGE) {
    SET_ERR(c, "chunk_mesh: a cell coordinate is outside [-2^20, 2^20)");
    return 62;
  }
  if ((m.err & CM_ERR_FACE_CELLS) || m.pairs > CM_MAX_PAIRS) {
    SET_ERR(c, "chunk_mesh: more than 2^31 (face, cell) pairs");
    return 62;
  }
  k.P = (uint32_t)m.pairs;
  uint64_t n[3];
  for (int a = 0; a < 3; ++a) {
    k.dn.lo[a] = m.bb_lo[a];
    n[a] = (uint64_t)((int64_t)m.bb_hi[a] - m.bb_lo[a] + 1);
  }
  k.ndense = n[0] * n[1] * n[2];  // each factor <= 2^21: no overflow
  if (k.ndense > CM_MAX_DENSE) {
    SET_ERR(c, "chunk_mesh: the mesh's bounding box spans %llu cells "
            "(limit 2^31)", (unsigned long long)k.ndense);
    return 62;
  }
  k.dn.ny = (uint32_t)n[1];
  k.dn.nz = (uint32_t)n[2];
  return scan_u32(c, c->cm_ncells.get(), c->cm_pair_off.get(), T + 1, s,
                  "chunk_mesh pair scan size query failed",
                  "chunk_mesh pair scan failed", 63);
}

// [2] per-pair point counts and sort keys; [3] stable sort into the
// per-cell stream order; corner offsets and cell ordinals
static int cm_pairs(mg_ctx *c, CmCall &k,
                    rocprim::double_buffer<uint32_t> &keys,
                    rocprim::double_buffer<uint32_t> &vals) {
  hipStream_t s = c->stream;
  const uint64_t P = k.P;
  for (auto *b : {&c->cm_npts, &c->cm_npts_s, &c->cm_fhead, &c->cm_coff,
                  &c->cm_ford})
    if (ensure(c, *b, P + 1)) return 64;
  hipLaunchKernelGGL(k_cm_pair, dim3(cm_blocks(P)), dim3(CM_BLK), 0, s,
                     c->cm_verts.get(), c->cm_faces.get(),
                     c->cm_pair_off.get(), k.ntris, k.P, k.g, k.dn,
                     keys.current(), vals.current(), c->cm_npts.get(),
                     c->cm_misc.get());
  if (int e = sort_pairs(c, keys, vals, P, 0, cm_bits(2 * k.ndense), s,
                         "chunk_mesh fragment sort size query failed",
                         "chunk_mesh fragment sort failed", 65))
    return e;
  hipLaunchKernelGGL(k_cm_frag_gather, dim3(cm_blocks(P + 1)), dim3(CM_BLK),
                     0, s, keys.current(), vals.current(), c->cm_npts.get(),
                     k.P, c->cm_npts_s.get(), c->cm_fhead.get());
  if (int e = scan_u32(c, c->cm_npts_s.get(), c->cm_coff.get(), P + 1, s,
                       "chunk_mesh corner scan size query failed",
                       "chunk_mesh corner scan failed", 65))
    return e;
  if (int e = scan_u32(c, c->cm_fhead.get(), c->cm_ford.get(), P + 1, s,
                       "chunk_mesh cell scan size query failed",
                       "chunk_mesh cell scan failed", 65))
    return e;
  CmMisc m;
  uint32_t ncellp = 0;
  HIP_TRY(c, hipMemcpyAsync(&m, c->cm_misc.get(), sizeof(m),
                            hipMemcpyDeviceToHost, s), 66);
  HIP_TRY(c, hipMemcpyAsync(&ncellp, c->cm_ford.get() + P, 4,
                            hipMemcpyDeviceToHost, s), 66);
  HIP_TRY(c, hipStreamSynchronize(s), 66);
  if (m.err & CM_ERR_POLY_OVERFLOW) {
    SET_ERR(c, "chunk_mesh: a clipped polygon exceeded %d points",
            CM_MAXPTS);
    return 67;
  }
  if (m.corners >= CM_MAX_CORNERS) {
    SET_ERR(c, "chunk_mesh: %llu fragment corners (limit 2^31)",
            (unsigned long long)m.corners);
    return 67;
  }
  k.C = (uint32_t)m.corners;
  k.ncellp = ncellp;
  return 0;
}

// [4] corners in stream order
static int cm_emit(mg_ctx *c, const CmCall &k, const uint32_t *keys_s,
                   const uint32_t *order) {
  hipStream_t s = c->stream;
  const uint64_t C = k.C, stride = (uint64_t)k.ncellp + 1;
  if (ensure(c, c->cm_pos, 3 * C + 3)) return 68;
  if (ensure(c, c->cm_cfrag, C + 1)) return 68;
  if (ensure(c, c->cm_ccell, C + 1)) return 68;
  if (ensure(c, c->cm_cells, stride * CM_CELL_FIELDS)) return 68;
  // FIRSTP stays 0xFFFFFFFF for a cell whose fragments were all empty
  HIP_TRY(c, hipMemsetAsync(c->cm_cells.get(), 0xFF,
                            stride * CM_CELL_FIELDS * 4, s), 68);
  hipLaunchKernelGGL(k_cm_emit, dim3(cm_blocks(k.P)), dim3(CM_BLK), 0, s,
                     c->cm_verts.get(), c->cm_faces.get(),
                     c->cm_pair_off.get(), k.ntris, k.P, k.g, keys_s, order,
                     c->cm_coff.get(), c->cm_fhead.get(), c->cm_ford.get(),
                     k.C, (uint32_t)stride, c->cm_pos.get(),
                     c->cm_cfrag.get(), c->cm_ccell.get(),
                     c->cm_cells.get());
  HIP_TRY(c, hipGetLastError(), 68);
  return 0;
}

// [5] weld: rep[c] = first corner of c's cell at c's position
static int cm_weld(mg_ctx *c, const CmCall &k) {
  hipStream_t s = c->stream;
  const uint64_t C = k.C;
  for (auto *b : {&c->cm_wkey, &c->cm_wkey_alt, &c->cm_wval, &c->cm_wval_alt,
                  &c->cm_whead, &c->cm_wrun, &c->cm_head_pos, &c->cm_rep})
    if (ensure(c, *b, C + 1)) return 69;
  rocprim::double_buffer<uint32_t> keys(c->cm_wkey.get(),
                                        c->cm_wkey_alt.get());
  rocprim::double_buffer<uint32_t> vals(c->cm_wval.get(),
                                        c->cm_wval_alt.get());
  const float *pos = c->cm_pos.get();
  const uint32_t *ccell = c->cm_ccell.get();
  hipLaunchKernelGGL(k_iota, dim3(cm_blocks(C)), dim3(CM_BLK), 0, s,
                     vals.current(), C);
  for (int which = 0; which < 4; ++which) {
    hipLaunchKernelGGL(k_cm_weld_key, dim3(cm_blocks(C)), dim3(CM_BLK), 0, s,
                       vals.current(), pos, ccell, k.C, which,
                       keys.current());
    unsigned bits = which == 3 ? cm_bits(k.ncellp) : 32u;
    if (int e = sort_pairs(c, keys, vals, C, 0, bits, s,
                           "chunk_mesh weld sort size query failed",
                           "chunk_mesh weld sort failed", 70))
      return e;
  }
  const uint32_t *sorted = vals.current();
  uint32_t *whead = c->cm_whead.get();
  uint32_t *wrun = c->cm_wrun.get();
  hipLaunchKernelGGL(k_cm_heads, dim3(cm_blocks(C + 1)), dim3(CM_BLK), 0, s,
                     sorted, pos, ccell, k.C, whead);
  if (int e = scan_u32(c, whead, wrun, C + 1, s,
                       "chunk_mesh run scan size query failed",
                       "chunk_mesh run scan failed", 70))
    return e;
  hipLaunchKernelGGL(k_cm_head_pos, dim3(cm_blocks(C)), dim3(CM_BLK), 0, s,
                     sorted, whead, wrun, k.C, c->cm_head_pos.get());
  hipLaunchKernelGGL(k_cm_rep, dim3(cm_blocks(C)), dim3(CM_BLK), 0, s,
                     sorted, whead, wrun, c->cm_head_pos.get(), k.C,
                     c->cm_rep.get());
  HIP_TRY(c, hipGetLastError(), 70);
  return 0;
}

// [6] faces, vertex ids, per-cell output slices
static int cm_faces(mg_ctx *c, const CmCall &k, const uint32_t *order) {
  hipStream_t s = c->stream;
  const uint64_t C = k.C, stride = (uint64_t)k.ncellp + 1;
  for (auto *b : {&c->cm_keep, &c->cm_used, &c->cm_vid, &c->cm_fslot})
    if (ensure(c, *b, C + 1)) return 71;
  if (ensure(c, c->cm_out_v, 3 * C + 3)) return 71;
  if (ensure(c, c->cm_out_f, 3 * C + 3)) return 71;
  const uint32_t *cfrag = c->cm_cfrag.get();
  const uint32_t *ccell = c->cm_ccell.get();
  const uint32_t *coff = c->cm_coff.get();
  const uint32_t *rep = c->cm_rep.get();
  uint32_t *keep = c->cm_keep.get();
  uint32_t *used = c->cm_used.get();
  uint32_t *vid = c->cm_vid.get();
  uint32_t *fslot = c->cm_fslot.get();
  uint32_t *cells = c->cm_cells.get();
  HIP_TRY(c, hipMemsetAsync(used, 0, (C + 1) * 4, s), 71);
  hipLaunchKernelGGL(k_cm_faces, dim3(cm_blocks(C + 1)), dim3(CM_BLK), 0, s,
                     cfrag, ccell, coff, order, rep, k.C, (uint32_t)stride,
                     keep, used, cells);
  if (int e = scan_u32(c, used, vid, C + 1, s,
                       "chunk_mesh vertex scan size query failed",
                       "chunk_mesh vertex scan failed", 72))
    return e;
  if (int e = scan_u32(c, keep, fslot, C + 1, s,
                       "chunk_mesh face scan size query failed",
                       "chunk_mesh face scan failed", 72))
    return e;
  if (C > 0)
    hipLaunchKernelGGL(k_cm_write, dim3(cm_blocks(C)), dim3(CM_BLK), 0, s,
                     cfrag, ccell, coff, rep, keep, used, vid, fslot,
                     c->cm_pos.get(), cells, k.C, c->cm_out_v.get(),
                     c->cm_out_f.get());
  hipLaunchKernelGGL(k_cm_cell_meta, dim3(cm_blocks(stride)), dim3(CM_BLK),
                     0, s, vid, fslot, k.ncellp, k.C, (uint32_t)stride,
                     cells);
  HIP_TRY(c, hipGetLastError(), 72);
  return 0;
}

// field f of a copy of c->cm_cells: CM_CELL_FIELDS u32 arrays of `stride`
// (= ncellp + 1) entries each, entry ncellp = the totals
static const uint32_t *cm_cells_view(const uint32_t *cells, int f,
                                     uint64_t stride) {
  return cells + f * stride;
}

// The per-cell table on the host and what both result stages derive from
// it: the cells that hold faces and the host function's dict order.
struct CmCellTable {
  std::vector<uint32_t> cells;  // copy of c->cm_cells
  const uint32_t *dense, *firstp, *vb, *fb;  // views, entry ncellp = totals
  std::vector<uint32_t> live;   // cell ordinals with faces, ascending
  std::vector<uint32_t> order;  // indices into live, dict order
  uint64_t V, F;                // vertex / face totals over all cells
};

// [7a] read the per-cell table (one sync) and derive the dict order: cells
// whose stream starts with an interior face (sort key bit 0 clear) in
// ascending cell order, then the rest by first emitted pair
static int cm_read_cells(mg_ctx *c, const CmCall &k, CmCellTable &t) {
  hipStream_t s = c->stream;
  const uint64_t stride = (uint64_t)k.ncellp + 1;
  t.cells.resize(stride * CM_CELL_FIELDS);
  HIP_TRY(c, hipMemcpyAsync(t.cells.data(), c->cm_cells.get(),
                            t.cells.size() * 4, hipMemcpyDeviceToHost, s), 73);
  HIP_TRY(c, hipStreamSynchronize(s), 73);
  t.dense = cm_cells_view(t.cells.data(), CM_CELL_DENSE, stride);
  t.firstp = cm_cells_view(t.cells.data(), CM_CELL_FIRSTP, stride);
  t.vb = cm_cells_view(t.cells.data(), CM_CELL_VB, stride);
  t.fb = cm_cells_view(t.cells.data(), CM_CELL_FB, stride);
  t.V = t.vb[k.ncellp];
  t.F = t.fb[k.ncellp];
  t.live.clear();
  for (uint32_t o = 0; o < k.ncellp; ++o)
    if (t.fb[o + 1] > t.fb[o]) t.live.push_back(o);
  t.order.resize(t.live.size());
  for (uint32_t m = 0; m < t.order.size(); ++m) t.order[m] = m;
  std::stable_sort(t.order.begin(), t.order.end(),
                   [&](uint32_t a, uint32_t b) {
    uint32_t oa = t.live[a], ob = t.live[b];
    bool ia = !(t.dense[oa] & 1u), ib = !(t.dense[ob] & 1u);
    if (ia != ib) return ia;
    if (ia) return oa < ob;
    return t.firstp[oa] < t.firstp[ob];
  });
  return 0;
}

// [7] D2H into the ctx's pinned staging + the descriptor: one mesh per
// non-empty cell by ascending label (= lexicographic cell order), and the
// host function's dict order in out_order[nmeshes] behind nf_arr.
static int cm_extract(mg_ctx *c, const CmCall &k, mg_meshset **out,
                      const uint32_t **out_order) {
  hipStream_t s = c->stream;
  CmCellTable t;
  if (int e = cm_read_cells(c, k, t)) return e;
  const uint64_t V = t.V, F = t.F;
  if (ensure(c, c->h_verts, 3 * V + 3)) return 73;
  if (ensure(c, c->h_faces, 3 * F + 3)) return 73;
  float *h_verts = c->h_verts.get();
  uint32_t *h_faces = c->h_faces.get();
  if (V > 0)
    HIP_TRY(c, hipMemcpyAsync(h_verts, c->cm_out_v.get(), V * 12,
                              hipMemcpyDeviceToHost, s), 73);
  if (F > 0)
    HIP_TRY(c, hipMemcpyAsync(h_faces, c->cm_out_f.get(), F * 12,
                              hipMemcpyDeviceToHost, s), 73);
  HIP_TRY(c, hipStreamSynchronize(s), 73);

  const uint32_t n = (uint32_t)t.live.size();
  mg_meshset *ms = alloc_meshset(n, 1);
  if (!ms) {
    SET_ERR(c, "chunk_mesh: out of host memory");
    return 73;
  }
  uint32_t *order = ms->nf_arr + n;
  ms->verts_base = h_verts;
  ms->faces_base = h_faces;
  ms->total_verts = V;
  ms->total_tris = F;
  for (uint32_t m = 0; m < n; ++m) {
    uint32_t o = t.live[m];
    uint32_t d = t.dense[o] >> 1;
    int64_t cz = (int64_t)(d % k.dn.nz) + k.dn.lo[2];
    int64_t cy = (int64_t)((d / k.dn.nz) % k.dn.ny) + k.dn.lo[1];
    int64_t cx = (int64_t)(d / k.dn.nz / k.dn.ny) + k.dn.lo[0];
    const uint64_t label = ((uint64_t)(cx + (1 << 20)) << 42) |
                           ((uint64_t)(cy + (1 << 20)) << 21) |
                           (uint64_t)(cz + (1 << 20));
    set_mesh(ms, m, label, t.vb[o], t.vb[o + 1] - t.vb[o], t.fb[o],
             t.fb[o + 1] - t.fb[o]);
    order[m] = t.order[m];
  }
  *out = ms;
  *out_order = order;
  return 0;
}

// [1]..[6] on the mesh in cm_verts / cm_faces (finite vertices, indices <
// nverts): everything up to the per-cell output slices in cm_out_v /
// cm_out_f and the per-cell table in cm_cells, all left on the device
static int cm_run_device(mg_ctx *c, CmCall &k, uint32_t nverts,
                         uint32_t ntris, const double scale[3],
                         const double offset[3]) {
  k = {};
  k.nverts = nverts;
  k.ntris = ntris;
  for (int a = 0; a < 3; ++a) {
    k.g.scale[a] = scale[a];
    k.g.offset[a] = offset[a];
  }
  if (int e = cm_count(c, k)) return e;
  for (auto *b : {&c->cm_fkey, &c->cm_fkey_alt, &c->cm_fval, &c->cm_fval_alt})
    if (ensure(c, *b, (uint64_t)k.P + 1)) return 64;
  rocprim::double_buffer<uint32_t> keys(c->cm_fkey.get(),
                                        c->cm_fkey_alt.get());
  rocprim::double_buffer<uint32_t> vals(c->cm_fval.get(),
                                        c->cm_fval_alt.get());
  if (int e = cm_pairs(c, k, keys, vals)) return e;
  if (int e = cm_emit(c, k, keys.current(), vals.current())) return e;
  if (k.C > 0)
    if (int e = cm_weld(c, k)) return e;
  return cm_faces(c, k, vals.current());
}

// the same for the caller's host arrays: validation, upload, [1]..[6]
static int cm_run_host(mg_ctx *c, CmCall &k, const float *verts,
                       uint32_t nverts, const uint32_t *faces, uint32_t ntris,
                       const double scale[3], const double offset[3]) {
  if (int e = cm_validate(c, verts, nverts, faces, ntris, scale, offset))
    return e;
  if (int e = cm_upload(c, verts, nverts, faces, ntris)) return e;
  return cm_run_device(c, k, nverts, ntris, scale, offset);
}

static int run_chunk_mesh(mg_ctx *c, const float *verts, uint32_t nverts,
                          const uint32_t *faces, uint32_t ntris,
                          const double scale[3], const double offset[3],
                          mg_meshset **out, const uint32_t **out_order) {
  CmCall k;
  if (int e = cm_run_host(c, k, verts, nverts, faces, ntris, scale, offset))
    return e;
  return cm_extract(c, k, out, out_order);
}
