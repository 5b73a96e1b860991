// merge_verts.hip — weld the close vertices of one mesh on the device, and
// the retriangulation built on it (the multires merge's
// Mesh.merge_close_vertices, reference multires.py:551, and the whole of
// retriangulate_mesh, multires.py:546-553). Included from meshgine.hip after
// chunk_mesh.hip: the kernels first, then their host driver.
//
// Contract: bit-equal to igneous_amd/meshops.py
// merge_close_vertices + consolidate. Vertices i and j are close when
// dx*dx + dy*dy + dz*dz <= r*r, on the f32 inputs widened to f64, every
// operation one IEEE operation as written (-ffp-contract=off). rep[i] is the
// minimum index of i's component in the graph of close pairs. Faces take
// their corners' reps, a face with two equal corners is dropped, the
// survivors keep their order; the output vertices are the reps a surviving
// face uses, ascending, each with its own stored bits.
//
// Close pairs are found through a uniform grid of cell size h = 2r: the
// quotients v/h of two close vertices differ by at most 1/2 plus rounding,
// so their cells differ by at most one per axis and the 27-cell
// neighbourhood holds every partner. The grid is a sort, not a table: a
// vertex's key is a 32-bit hash of its cell triple, and a candidate only
// counts when its own cell triple equals the neighbour triple being
// visited, so hash collisions cost time, never a pair, and a pair is seen
// once even when two neighbour triples share a key.
//
// Schedule (kernel boundaries order the phases; no spin flags, no grid
// sync, every loop bounded; atomics are the union-find CAS and integer
// or/add counters only; the result depends on neither the order of the
// links nor the order inside a bucket):
//   k_mv_cell     per vertex: cell triple, sort key
//   sort_pairs    (key, vertex index)
//   k_mv_count    per vertex: candidate visits = the lengths of the 27 key
//                 runs; the total decides the cap before any link runs
//   k_iota        parent[i] = i
//   k_mv_link     per vertex i: walk the 27 runs, union(i, j) for close j < i
//                 (fill_union of fill_holes.hip: a root only ever receives a
//                 smaller index, so the root is the component's minimum)
//   k_fill_flatten  parent[i] = root(i)
//   k_mv_faces    keep flag per face, used[rep] = 1
//   scan x2       vertex ids, face slots
//   k_mv_write    vertices and renumbered faces
//
// MV_MAX_VISITS is a stated condition, not a tuned number: nobody has
// measured how long 2^32 candidate visits take. It exists so that no call
// (a radius far too large for its mesh) can occupy a shared GPU for minutes.

#define MV_BLK 256
#define MV_CELL_LIM 2251799813685248.0  // 2^51: |v / h| stays below it
#define MV_MAX_VISITS (1ull << 32)

#define MV_ERR_CELL_RANGE 1u

// scalars the host reads back; one block at mv_misc
struct MvMisc {
  unsigned long long visits;  // sum of the 27 run lengths over all vertices
  uint32_t err;
  uint32_t pad;
};

static inline uint32_t mv_blocks(uint64_t n) {
  return (uint32_t)((std::max<uint64_t>(n, 1) + MV_BLK - 1) / MV_BLK);
}

__device__ __forceinline__ uint32_t mv_key(long long cx, long long cy,
                                           long long cz) {
  uint64_t h = mix64((uint64_t)cx);
  h = mix64(h ^ (uint64_t)cy);
  h = mix64(h ^ (uint64_t)cz);
  return (uint32_t)(h >> 32);
}

__global__ __launch_bounds__(MV_BLK) void k_mv_cell(
    const float *__restrict__ verts, uint32_t nverts, double h,
    long long *__restrict__ cell, uint32_t *__restrict__ keys,
    uint32_t *__restrict__ vals, MvMisc *misc) {
  uint64_t i = (uint64_t)blockIdx.x * MV_BLK + threadIdx.x;
  if (i >= nverts) return;
  long long q[3];
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    double d = (double)verts[3 * i + a] / h;
    if (!(fabs(d) < MV_CELL_LIM)) ok = false;
    q[a] = ok ? (long long)floor(d) : 0;
  }
  if (!ok) {
    q[0] = q[1] = q[2] = 0;
    atomicOr(&misc->err, MV_ERR_CELL_RANGE);
  }
  for (int a = 0; a < 3; ++a) cell[3 * i + a] = q[a];
  keys[i] = mv_key(q[0], q[1], q[2]);
  vals[i] = (uint32_t)i;
}

// first position of the sorted keys that is >= key (n when there is none)
__device__ __forceinline__ uint32_t mv_lower(const uint32_t *__restrict__ keys,
                                             uint32_t n, uint32_t key) {
  uint32_t lo = 0, hi = n;  // answer in [lo, hi]
  for (int it = 0; it < 32 && lo < hi; ++it) {
    uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// first position of the sorted keys that is > key
__device__ __forceinline__ uint32_t mv_upper(const uint32_t *__restrict__ keys,
                                             uint32_t n, uint32_t key) {
  uint32_t lo = 0, hi = n;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(MV_BLK) void k_mv_count(
    const long long *__restrict__ cell, const uint32_t *__restrict__ keys_s,
    uint32_t nverts, MvMisc *misc) {
  __shared__ unsigned long long s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  uint64_t i = (uint64_t)blockIdx.x * MV_BLK + threadIdx.x;
  if (i < nverts) {
    const long long cx = cell[3 * i], cy = cell[3 * i + 1],
                    cz = cell[3 * i + 2];
    unsigned long long n = 0;
    for (int d = 0; d < 27; ++d) {
      uint32_t key = mv_key(cx + (d / 9 - 1), cy + (d / 3 % 3 - 1),
                            cz + (d % 3 - 1));
      n += mv_upper(keys_s, nverts, key) - mv_lower(keys_s, nverts, key);
    }
    atomicAdd(&s_sum, n);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_sum) atomicAdd(&misc->visits, s_sum);
}

__global__ __launch_bounds__(MV_BLK) void k_mv_link(
    const float *__restrict__ verts, const long long *__restrict__ cell,
    const uint32_t *__restrict__ keys_s, const uint32_t *__restrict__ vals_s,
    uint32_t nverts, double r2, uint32_t *parent) {
  uint64_t i = (uint64_t)blockIdx.x * MV_BLK + threadIdx.x;
  if (i >= nverts) return;
  const long long cx = cell[3 * i], cy = cell[3 * i + 1], cz = cell[3 * i + 2];
  const double x = (double)verts[3 * i], y = (double)verts[3 * i + 1],
               z = (double)verts[3 * i + 2];
  for (int d = 0; d < 27; ++d) {
    const long long nx = cx + (d / 9 - 1), ny = cy + (d / 3 % 3 - 1),
                    nz = cz + (d % 3 - 1);
    const uint32_t key = mv_key(nx, ny, nz);
    for (uint32_t p = mv_lower(keys_s, nverts, key);
         p < nverts && keys_s[p] == key; ++p) {
      const uint64_t j = vals_s[p];
      if (j >= i) continue;
      if (cell[3 * j] != nx || cell[3 * j + 1] != ny || cell[3 * j + 2] != nz)
        continue;
      const double dx = x - (double)verts[3 * j];
      const double dy = y - (double)verts[3 * j + 1];
      const double dz = z - (double)verts[3 * j + 2];
      const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
      const double xy = xx + yy;
      if (xy + zz <= r2) fill_union(parent, (uint32_t)i, (uint32_t)j);
    }
  }
}

// keep flag per face after the weld, used flags on the reps. `used` is
// zeroed by the driver; index ntris of keep is the scan terminator.
__global__ void k_mv_faces(const uint32_t *__restrict__ faces,
                           const uint32_t *__restrict__ rep, uint32_t ntris,
                           uint32_t *__restrict__ keep,
                           uint32_t *__restrict__ used) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > ntris) return;
  uint32_t kp = 0;
  if (t < ntris) {
    uint32_t a = rep[faces[3 * t]], b = rep[faces[3 * t + 1]],
             d = rep[faces[3 * t + 2]];
    if (a != b && b != d && a != d) {
      kp = 1;
      used[a] = 1;
      used[b] = 1;
      used[d] = 1;
    }
  }
  keep[t] = kp;
}

// thread i writes vertex i (if used) and face i (if kept)
__global__ void k_mv_write(const float *__restrict__ verts,
                           const uint32_t *__restrict__ faces,
                           const uint32_t *__restrict__ rep,
                           const uint32_t *__restrict__ keep,
                           const uint32_t *__restrict__ used,
                           const uint32_t *__restrict__ vid_x,
                           const uint32_t *__restrict__ fslot_x,
                           uint32_t nverts, uint32_t ntris,
                           float *__restrict__ out_v,
                           uint32_t *__restrict__ out_f) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nverts && used[i]) {
    uint64_t v = vid_x[i];
    out_v[3 * v + 0] = verts[3 * i + 0];
    out_v[3 * v + 1] = verts[3 * i + 1];
    out_v[3 * v + 2] = verts[3 * i + 2];
  }
  if (i < ntris && keep[i]) {
    uint64_t t = fslot_x[i];
    out_f[3 * t + 0] = vid_x[rep[faces[3 * i + 0]]];
    out_f[3 * t + 1] = vid_x[rep[faces[3 * i + 1]]];
    out_f[3 * t + 2] = vid_x[rep[faces[3 * i + 2]]];
  }
}

// per-cell gather table of the retriangulation, four sub-arrays of stride
// (ncells + 1) in the host function's dict order; entry ncells of the two
// destination arrays holds the totals
enum { MV_TAB_DST_V = 0, MV_TAB_DST_F, MV_TAB_SRC_V, MV_TAB_SRC_F,
       MV_TAB_FIELDS };

// Mesh.concatenate of the chunker's per-cell slices: thread i moves vertex i
// and face i of the concatenated mesh, the face with its cell's vertex base
// added. Both destination arrays are strictly increasing (every cell of the
// table holds a face, and so a vertex).
__global__ void k_mv_gather(const float *__restrict__ src_v,
                            const uint32_t *__restrict__ src_f,
                            const uint32_t *__restrict__ tab, uint32_t ncells,
                            uint32_t nverts, uint32_t ntris,
                            float *__restrict__ dst_v,
                            uint32_t *__restrict__ dst_f) {
  const uint64_t stride = (uint64_t)ncells + 1;
  const uint32_t *dv = tab + MV_TAB_DST_V * stride;
  const uint32_t *df = tab + MV_TAB_DST_F * stride;
  const uint32_t *sv = tab + MV_TAB_SRC_V * stride;
  const uint32_t *sf = tab + MV_TAB_SRC_F * stride;
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nverts) {
    uint32_t m = cm_face_of_pair(dv, ncells, (uint32_t)i);
    uint64_t s = (uint64_t)sv[m] + (i - dv[m]);
    dst_v[3 * i + 0] = src_v[3 * s + 0];
    dst_v[3 * i + 1] = src_v[3 * s + 1];
    dst_v[3 * i + 2] = src_v[3 * s + 2];
  }
  if (i < ntris) {
    uint32_t m = cm_face_of_pair(df, ncells, (uint32_t)i);
    uint64_t s = (uint64_t)sf[m] + (i - df[m]);
    dst_f[3 * i + 0] = src_f[3 * s + 0] + dv[m];
    dst_f[3 * i + 1] = src_f[3 * s + 1] + dv[m];
    dst_f[3 * i + 2] = src_f[3 * s + 2] + dv[m];
  }
}

// ---------------------------------------------------------------------------
// host driver

struct MvCall {
  uint32_t nverts, ntris;
  double radius;
  uint32_t out_nverts, out_ntris;
};

static int mv_check_radius(mg_ctx *c, double radius) {
  if (!std::isfinite(radius) || !(radius > 0.0)) {
    SET_ERR(c, "merge_close_vertices: radius %g must be finite and > 0",
            radius);
    return 100;
  }
  return 0;
}

// Host-side validation: nothing out of contract reaches a kernel.
static int mv_validate(mg_ctx *c, const float *verts, uint32_t nverts,
                       const uint32_t *faces, uint32_t ntris, double radius) {
  if (int e = mv_check_radius(c, radius)) return e;
  for (uint64_t i = 0; i < 3ull * ntris; ++i) {
    if (faces[i] >= nverts) {
      SET_ERR(c, "merge_close_vertices: face %llu references vertex %u >= "
              "nverts %u", (unsigned long long)(i / 3), faces[i], nverts);
      return 100;
    }
  }
  for (uint64_t i = 0; i < 3ull * nverts; ++i) {
    if (!std::isfinite(verts[i])) {
      SET_ERR(c, "merge_close_vertices: vertex %llu is not finite",
              (unsigned long long)(i / 3));
      return 100;
    }
  }
  return 0;
}

// room for a mesh of V vertices and T faces in mv_verts / mv_faces
static int mv_ensure_input(mg_ctx *c, uint64_t V, uint64_t T) {
  if (ensure(c, c->mv_verts, 3 * V + 3)) return 101;
  if (ensure(c, c->mv_faces, 3 * T + 3)) return 101;
  return 0;
}

// [1] cells, sort, candidate count: the range check and the cap
static int mv_grid(mg_ctx *c, const MvCall &k, const float *d_verts,
                   rocprim::double_buffer<uint32_t> &keys,
                   rocprim::double_buffer<uint32_t> &vals) {
  hipStream_t s = c->stream;
  const uint64_t V = k.nverts;
  HIP_TRY(c, hipMemsetAsync(c->mv_misc.get(), 0, sizeof(MvMisc), s), 102);
  hipLaunchKernelGGL(k_mv_cell, dim3(mv_blocks(V)), dim3(MV_BLK), 0, s,
                     d_verts, k.nverts, 2.0 * k.radius, c->mv_cell.get(),
                     keys.current(), vals.current(), c->mv_misc.get());
  if (int e = sort_pairs(c, keys, vals, V, 0, 32, s,
                         "merge_close_vertices sort size query failed",
                         "merge_close_vertices sort failed", 102))
    return e;
  hipLaunchKernelGGL(k_mv_count, dim3(mv_blocks(V)), dim3(MV_BLK), 0, s,
                     c->mv_cell.get(), keys.current(), k.nverts,
                     c->mv_misc.get());
  MvMisc m;
  HIP_TRY(c, hipMemcpyAsync(&m, c->mv_misc.get(), sizeof(m),
                            hipMemcpyDeviceToHost, s), 102);
  HIP_TRY(c, hipStreamSynchronize(s), 102);
  if (m.err & MV_ERR_CELL_RANGE) {
    SET_ERR(c, "merge_close_vertices: a coordinate over 2 * radius is "
            "outside (-2^51, 2^51)");
    return 103;
  }
  if (m.visits > MV_MAX_VISITS) {
    SET_ERR(c, "merge_close_vertices: radius too large for this mesh (%llu "
            "candidate visits, limit 2^32)", (unsigned long long)m.visits);
    return 103;
  }
  return 0;
}

// [2] union-find over the close pairs: parent[i] = component minimum
static int mv_link(mg_ctx *c, const MvCall &k, const float *d_verts,
                   const uint32_t *keys_s, const uint32_t *vals_s) {
  hipStream_t s = c->stream;
  const uint64_t V = k.nverts;
  uint32_t *parent = c->mv_parent.get();
  hipLaunchKernelGGL(k_iota, dim3(mv_blocks(V)), dim3(MV_BLK), 0, s, parent,
                     V);
  hipLaunchKernelGGL(k_mv_link, dim3(mv_blocks(V)), dim3(MV_BLK), 0, s,
                     d_verts, c->mv_cell.get(), keys_s, vals_s, k.nverts,
                     k.radius * k.radius, parent);
  hipLaunchKernelGGL(k_fill_flatten, dim3(fill_blocks(V)), dim3(FILL_BLK), 0,
                     s, parent, k.nverts);
  HIP_TRY(c, hipGetLastError(), 104);
  return 0;
}

// [3] faces, vertex ids, the welded mesh in mv_out_v / mv_out_f
static int mv_faces(mg_ctx *c, MvCall &k, const float *d_verts,
                    const uint32_t *d_faces) {
  hipStream_t s = c->stream;
  const uint64_t V = k.nverts, T = k.ntris;
  const uint32_t *rep = c->mv_parent.get();
  uint32_t *keep = c->mv_keep.get();
  uint32_t *used = c->mv_used.get();
  uint32_t *vid = c->mv_vid.get();
  uint32_t *fslot = c->mv_fslot.get();
  HIP_TRY(c, hipMemsetAsync(used, 0, (V + 1) * 4, s), 105);
  hipLaunchKernelGGL(k_mv_faces, dim3(mv_blocks(T + 1)), dim3(MV_BLK), 0, s,
                     d_faces, rep, k.ntris, keep, used);
  if (int e = scan_u32(c, used, vid, V + 1, s,
                       "merge_close_vertices vertex scan size query failed",
                       "merge_close_vertices vertex scan failed", 105))
    return e;
  if (int e = scan_u32(c, keep, fslot, T + 1, s,
                       "merge_close_vertices face scan size query failed",
                       "merge_close_vertices face scan failed", 105))
    return e;
  hipLaunchKernelGGL(k_mv_write, dim3(mv_blocks(std::max(V, T))),
                     dim3(MV_BLK), 0, s, d_verts, d_faces, rep, keep, used,
                     vid, fslot, k.nverts, k.ntris, c->mv_out_v.get(),
                     c->mv_out_f.get());
  HIP_TRY(c, hipMemcpyAsync(&k.out_nverts, vid + V, 4, hipMemcpyDeviceToHost,
                            s), 105);
  HIP_TRY(c, hipMemcpyAsync(&k.out_ntris, fslot + T, 4, hipMemcpyDeviceToHost,
                            s), 105);
  HIP_TRY(c, hipStreamSynchronize(s), 105);
  return 0;
}

// Weld the mesh in the DEVICE arrays d_verts (V x 3) / d_faces (T x 3,
// every index < V) into mv_out_v / mv_out_f; the result's counts go to
// k.out_nverts / k.out_ntris. The caller has validated the radius;
// non-finite vertices fail the range check.
static int mv_run_device(mg_ctx *c, MvCall &k, const float *d_verts,
                         uint32_t V, const uint32_t *d_faces, uint32_t T,
                         double radius) {
  k = {V, T, radius, 0, 0};
  if (T == 0) return 0;  // a mesh without faces keeps no vertex
  const uint64_t nv = V, nt = T;
  if (ensure(c, c->mv_misc, 1)) return 101;
  if (ensure(c, c->mv_cell, 3 * nv)) return 101;
  for (auto *b : {&c->mv_key, &c->mv_key_alt, &c->mv_val, &c->mv_val_alt,
                  &c->mv_parent, &c->mv_used, &c->mv_vid})
    if (ensure(c, *b, nv + 1)) return 101;
  for (auto *b : {&c->mv_keep, &c->mv_fslot})
    if (ensure(c, *b, nt + 1)) return 101;
  if (ensure(c, c->mv_out_v, 3 * nv + 3)) return 101;
  if (ensure(c, c->mv_out_f, 3 * nt + 3)) return 101;
  rocprim::double_buffer<uint32_t> keys(c->mv_key.get(), c->mv_key_alt.get());
  rocprim::double_buffer<uint32_t> vals(c->mv_val.get(), c->mv_val_alt.get());
  if (int e = mv_grid(c, k, d_verts, keys, vals)) return e;
  if (int e = mv_link(c, k, d_verts, keys.current(), vals.current()))
    return e;
  return mv_faces(c, k, d_verts, d_faces);
}

// the welded mesh of mv_run_device into the ctx's pinned staging
static int mv_download(mg_ctx *c, const MvCall &k, const float **out_verts,
                       uint32_t *out_nverts, const uint32_t **out_faces,
                       uint32_t *out_ntris) {
  hipStream_t s = c->stream;
  const uint64_t OV = k.out_nverts, OT = k.out_ntris;
  if (ensure(c, c->h_verts, 3 * OV + 3)) return 106;
  if (ensure(c, c->h_faces, 3 * OT + 3)) return 106;
  if (OV > 0)
    HIP_TRY(c, hipMemcpyAsync(c->h_verts.get(), c->mv_out_v.get(), OV * 12,
                              hipMemcpyDeviceToHost, s), 106);
  if (OT > 0)
    HIP_TRY(c, hipMemcpyAsync(c->h_faces.get(), c->mv_out_f.get(), OT * 12,
                              hipMemcpyDeviceToHost, s), 106);
  HIP_TRY(c, hipStreamSynchronize(s), 106);
  *out_verts = c->h_verts.get();
  *out_nverts = (uint32_t)OV;
  *out_faces = c->h_faces.get();
  *out_ntris = (uint32_t)OT;
  return 0;
}

static int run_merge_close(mg_ctx *c, const float *d_verts, uint32_t V,
                           const uint32_t *d_faces, uint32_t T, double radius,
                           const float **out_verts, uint32_t *out_nverts,
                           const uint32_t **out_faces, uint32_t *out_ntris) {
  MvCall k;
  if (int e = mv_run_device(c, k, d_verts, V, d_faces, T, radius)) return e;
  return mv_download(c, k, out_verts, out_nverts, out_faces, out_ntris);
}

// mg_merge_close_vertices: host arrays in
static int run_merge_close_host(mg_ctx *c, const float *verts, uint32_t V,
                                const uint32_t *faces, uint32_t T,
                                double radius, const float **out_verts,
                                uint32_t *out_nverts,
                                const uint32_t **out_faces,
                                uint32_t *out_ntris) {
  hipStream_t s = c->stream;
  if (int e = mv_validate(c, verts, V, faces, T, radius)) return e;
  if (T > 0) {
    if (int e = mv_ensure_input(c, V, T)) return e;
    HIP_TRY(c, hipMemcpyAsync(c->mv_verts.get(), verts, (uint64_t)V * 12,
                              hipMemcpyHostToDevice, s), 101);
    HIP_TRY(c, hipMemcpyAsync(c->mv_faces.get(), faces, (uint64_t)T * 12,
                              hipMemcpyHostToDevice, s), 101);
  }
  return run_merge_close(c, c->mv_verts.get(), V, c->mv_faces.get(), T,
                         radius, out_verts, out_nverts, out_faces, out_ntris);
}

// The retriangulation of the mesh in cm_verts / cm_faces, on the device: the
// chunker's stages, the cells gathered in dict order into one mesh, then the
// weld into mv_out_v / mv_out_f (counts in k). *no_cells: the chunker kept
// no cell and nothing else was done (the result is the input, still in
// cm_verts / cm_faces).
static int mv_retriangulate_device(mg_ctx *c, MvCall &k, uint32_t nverts,
                                   uint32_t ntris, const double scale[3],
                                   const double offset[3], double radius,
                                   bool *no_cells) {
  hipStream_t s = c->stream;
  CmCall ck;
  if (int e = cm_run_device(c, ck, nverts, ntris, scale, offset)) return e;
  CmCellTable t;
  if (int e = cm_read_cells(c, ck, t)) return e;
  const uint32_t n = (uint32_t)t.live.size();
  *no_cells = n == 0;
  if (n == 0) return 0;
  // per-cell bases for the dict order (every live cell holds a face, hence a
  // vertex, so live cells alone carry t.V and t.F)
  const uint64_t stride = (uint64_t)n + 1;
  std::vector<uint32_t> tab(stride * MV_TAB_FIELDS, 0u);
  uint32_t dv = 0, df = 0;
  for (uint32_t m = 0; m < n; ++m) {
    const uint32_t o = t.live[t.order[m]];
    tab[MV_TAB_DST_V * stride + m] = dv;
    tab[MV_TAB_DST_F * stride + m] = df;
    tab[MV_TAB_SRC_V * stride + m] = t.vb[o];
    tab[MV_TAB_SRC_F * stride + m] = t.fb[o];
    dv += t.vb[o + 1] - t.vb[o];
    df += t.fb[o + 1] - t.fb[o];
  }
  tab[MV_TAB_DST_V * stride + n] = dv;
  tab[MV_TAB_DST_F * stride + n] = df;
  if (ensure(c, c->mv_tab, tab.size())) return 101;
  if (int e = mv_ensure_input(c, dv, df)) return e;
  HIP_TRY(c, hipMemcpyAsync(c->mv_tab.get(), tab.data(), tab.size() * 4,
                            hipMemcpyHostToDevice, s), 107);
  hipLaunchKernelGGL(k_mv_gather, dim3(mv_blocks(std::max(dv, df))),
                     dim3(MV_BLK), 0, s, c->cm_out_v.get(),
                     c->cm_out_f.get(), c->mv_tab.get(), n, dv, df,
                     c->mv_verts.get(), c->mv_faces.get());
  HIP_TRY(c, hipGetLastError(), 107);
  HIP_TRY(c, hipStreamSynchronize(s), 107);  // tab is read: it may go
  return mv_run_device(c, k, c->mv_verts.get(), dv, c->mv_faces.get(), df,
                       radius);
}

// mg_retriangulate_mesh: host arrays in, the welded mesh downloaded. With
// *no_cells set nothing is downloaded (the caller's result is its input).
static int run_retriangulate(mg_ctx *c, const float *verts, uint32_t nverts,
                             const uint32_t *faces, uint32_t ntris,
                             const double scale[3], const double offset[3],
                             double radius, bool *no_cells,
                             const float **out_verts, uint32_t *out_nverts,
                             const uint32_t **out_faces,
                             uint32_t *out_ntris) {
  if (int e = mv_check_radius(c, radius)) return e;
  if (int e = cm_validate(c, verts, nverts, faces, ntris, scale, offset))
    return e;
  if (int e = cm_upload(c, verts, nverts, faces, ntris)) return e;
  MvCall k;
  if (int e = mv_retriangulate_device(c, k, nverts, ntris, scale, offset,
                                      radius, no_cells))
    return e;
  if (*no_cells) return 0;
  return mv_download(c, k, out_verts, out_nverts, out_faces, out_ntris);
}
