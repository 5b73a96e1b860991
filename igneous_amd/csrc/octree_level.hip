// octree_level.hip — one level of one mesh's multires octree, from the host
// mesh to the finished fragment bytes (mg_encode_octree_level; replaces, per
// lod, create_octree_level_from_mesh and the to_stored_model_space +
// draco encode loop of process_mesh, reference multires.py:556-585 and
// :152-174). Included from meshgine.hip after merge_verts.hip: it joins the
// chunker (chunk_mesh.hip), the weld (merge_verts.hip) and the encode
// kernels (encode.hip).
//
// Contract (restated by tests/octree_level_ref.py): the bytes
// of tasks/multires.py encode_octree_level_host. The mesh M is uploaded
// once into cm_verts / cm_faces and stays on the device:
//   retriangulate   mv_retriangulate_device at the upper level's grid; the
//                   welded mesh is copied d2d from mv_out_v / mv_out_f back
//                   into cm_verts / cm_faces (valid by construction, so the
//                   host validation runs once, on the caller's arrays)
//   chunked         cm_run_device at this level's grid. In lexicographic
//                   cell order the chunker's per-cell prefix arrays (fields
//                   VB and FB of cm_cells) ARE the vbase / tri_off tables
//                   the encode kernels search; a cell without faces is an
//                   entry without vertices and gets no bytes.
//   unchunked       one entry: the two-entry prefix tables {0, V}, {0, T}
//                   over M itself
// Only the entry offsets follow z-order. The host reads the per-cell table
// once (cm_read_cells), sorts the live cells and uploads `order` (the entry
// of each z-rank) and each entry's node.
//
// Launches, visibility from kernel boundaries only (no spin flags, no grid
// sync, every loop bounded, no atomics):
//   k_enc_varint_sum    block per entry of the varint band (encode.hip)
//   k_ol_sizes          thread per z-rank: the entry's size, gathered
//   rocPRIM scan (u64)  sizes -> offsets, both in z-order
//   k_ol_offsets        thread per z-rank: the offset scattered to its entry
//   k_ol_verts          thread per vertex: entry from the block's staged
//                       vbase range, quantised against the entry's node
//   k_enc_faces, k_enc_varint_write, k_enc_headers   (encode.hip, with
//                       ENC_DRACO_INT)
// Entries are odd-sized and stored byte by byte: no blob address is cast to
// a wider pointer.

// to_stored_model_space's numbers
struct OlQuant {
  double o[3], vo[3], cell[3], qmax;
};

__global__ void k_ol_sizes(EncTables t, const uint32_t *__restrict__ order,
                           uint32_t n, uint64_t *__restrict__ zsize) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  zsize[r] = enc_layout(t, ENC_DRACO_INT, order[r]).size;
}

__global__ void k_ol_offsets(const uint32_t *__restrict__ order,
                             const uint64_t *__restrict__ zoff, uint32_t n,
                             uint64_t *__restrict__ off) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  off[order[r]] = zoff[r];
}

__global__ void __launch_bounds__(ENC_BLK)
k_ol_verts(const float *__restrict__ verts, EncTables t, OlQuant q,
           const int32_t *__restrict__ node, uint8_t *__restrict__ blob,
           uint32_t V) {
  __shared__ uint32_t s_off[ENC_BLK];
  __shared__ uint32_t s_rng[2];
  const uint32_t first = blockIdx.x * ENC_BLK;  // < V by the grid's size
  const uint32_t last =
      (uint32_t)min((uint64_t)first + ENC_BLK - 1, (uint64_t)V - 1);
  const bool valid = (uint64_t)first + threadIdx.x < V;
  const uint32_t i = valid ? first + threadIdx.x : last;
  const uint32_t l = enc_block_label(t.vbase, t.nlabels, first, last, i,
                                     valid, s_off, s_rng);
  if (!valid) return;
  const EncLayout e = enc_layout(t, ENC_DRACO_INT, l);
  const uint64_t j = i - t.vbase[l];
  uint8_t *dst = blob + t.off[l] + e.vpos + 12 * j;
  for (int k = 0; k < 3; ++k) {
    // one IEEE f64 operation per step, in to_stored_model_space's order
    double x = (double)verts[3 * (uint64_t)i + k];
    x = x - q.o[k];
    x = x - q.vo[k];
    x = x / q.cell[k];
    x = x - (double)node[3 * (uint64_t)l + k];
    x = x * q.qmax;
    x = rint(x);
    x = x < 0.0 ? 0.0 : x > q.qmax ? q.qmax : x;
    enc_put_u32(dst + 4 * k, (uint32_t)x);
  }
}

// ---------------------------------------------------------------------------
// host driver

// The result descriptor, one calloc: mg_fragset, then offset / size (u64),
// nodes (3 i32), nverts / ntris (u32) per fragment.
static int new_fragset(mg_ctx *c, uint32_t n, mg_fragset **out) {
  mg_fragset *fs = (mg_fragset *)calloc(
      1, sizeof(mg_fragset) + (size_t)n * (2 * 8 + 3 * 4 + 2 * 4) + 8);
  if (!fs) {
    SET_ERR(c, "encode_octree_level: out of host memory");
    return 115;
  }
  fs->n = n;
  fs->offset = (uint64_t *)((char *)fs + sizeof(mg_fragset));
  fs->size = fs->offset + n;
  fs->nodes = (int32_t *)(fs->size + n);
  fs->nverts = (uint32_t *)(fs->nodes + 3 * (size_t)n);
  fs->ntris = fs->nverts + n;
  *out = fs;
  return 0;
}

// q_bits outside 1..32, a non-finite q_* value, q_cell <= 0: rejected
// before any kernel. Fills the vertex kernel's OlQuant.
static int ol_check_params(mg_ctx *c, const mg_octree_level *lv, OlQuant *q) {
  if (lv->q_bits < 1 || lv->q_bits > 32) {
    SET_ERR(c, "encode_octree_level: q_bits %u outside 1..32", lv->q_bits);
    return 110;
  }
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(lv->q_origin[k])) {
      SET_ERR(c, "encode_octree_level: non-finite q_origin[%d]", k);
      return 110;
    }
    if (!std::isfinite(lv->q_voffset[k])) {
      SET_ERR(c, "encode_octree_level: non-finite q_voffset[%d]", k);
      return 110;
    }
    if (!std::isfinite(lv->q_cell[k])) {
      SET_ERR(c, "encode_octree_level: non-finite q_cell[%d]", k);
      return 110;
    }
    if (!(lv->q_cell[k] > 0.0)) {
      SET_ERR(c, "encode_octree_level: q_cell[%d] = %g must be > 0", k,
              lv->q_cell[k]);
      return 110;
    }
    q->o[k] = lv->q_origin[k];
    q->vo[k] = lv->q_voffset[k];
    q->cell[k] = lv->q_cell[k];
  }
  q->qmax = (double)((1ull << lv->q_bits) - 1);
  return 0;
}

// cmp_zorder (tasks/multires.py) on cell coordinates biased by 2^20, which
// are non-negative: the same order wherever cmp_zorder is a total order (no
// axis with cells of both signs; the low 20 bits of a negative coordinate
// are those of its biased value, and all of an axis' biased values share
// bit 20), and a total order everywhere.
static bool ol_z_less(const int32_t *a, const int32_t *b) {
  auto less_msb = [](uint32_t x, uint32_t y) { return x < y && x < (x ^ y); };
  uint32_t ua[3], ub[3];
  for (int k = 0; k < 3; ++k) {
    ua[k] = (uint32_t)(a[k] + (1 << 20));
    ub[k] = (uint32_t)(b[k] + (1 << 20));
  }
  int msd = 2;
  for (int dim : {1, 0})
    if (less_msb(ua[msd] ^ ub[msd], ua[dim] ^ ub[dim])) msd = dim;
  return ua[msd] < ub[msd];
}

// The z-order of n cells given in dict order: perm[r] = index of the cell
// that comes r-th. Cells of both signs on one axis go to the caller's
// order_cells when there is one (meshgine.h).
static int ol_zorder(mg_ctx *c, const mg_octree_level *lv,
                     const std::vector<int32_t> &nodes, uint32_t n,
                     std::vector<uint32_t> &perm) {
  perm.resize(n);
  bool mixed = false;
  for (int k = 0; k < 3; ++k) {
    bool neg = false, pos = false;
    for (uint32_t m = 0; m < n; ++m)
      (nodes[3 * (size_t)m + k] < 0 ? neg : pos) = true;
    mixed = mixed || (neg && pos);
  }
  if (mixed && lv->order_cells) {
    if (lv->order_cells(nodes.data(), n, perm.data(), lv->order_arg)) {
      SET_ERR(c, "encode_octree_level: the order_cells callback failed");
      return 112;
    }
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t r = 0; r < n; ++r) {
      if (perm[r] >= n || seen[perm[r]]) {
        SET_ERR(c, "encode_octree_level: order_cells returned no permutation "
                "of the %u cells", n);
        return 112;
      }
      seen[perm[r]] = 1;
    }
    return 0;
  }
  for (uint32_t m = 0; m < n; ++m) perm[m] = m;
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
    return ol_z_less(&nodes[3 * (size_t)a], &nodes[3 * (size_t)b]);
  });
  return 0;
}

// What the encode stage is handed: the device mesh, its E entries as two
// device prefix tables, and per z-rank the entry, its node and its counts.
struct OlEntries {
  const float *d_verts;
  const uint32_t *d_faces;
  uint64_t V, T;                  // totals over all entries
  const uint32_t *vbase, *tri_off;  // device, E + 1 each
  uint32_t E;
  std::vector<uint32_t> order;    // [n] entry of z-rank r
  std::vector<int32_t> nodes;     // [3n] node of z-rank r
  std::vector<uint32_t> nv, nf;   // [n]
};

// Encode the n >= 1 fragments into c->enc_blob, then D2H of the two z-order
// tables and of the blob into the ctx's pinned staging.
static int ol_encode(mg_ctx *c, const OlEntries &en, const OlQuant &q,
                     mg_fragset **out) {
  hipStream_t s = c->stream;
  const uint32_t n = (uint32_t)en.order.size(), E = en.E;
  const uint64_t V = en.V, NC = 3 * en.T;
  // the blob's size is known only after the scan; this bound lets every
  // kernel queue without a sync (an index takes at most 4 bytes)
  const uint64_t bound =
      12 * V + 4 * NC + (uint64_t)n * ENC_DRACO_FIXED_MAX;
  if (ensure(c, c->enc_ilen, E)) return 111;
  if (ensure(c, c->enc_off, E)) return 111;
  if (ensure(c, c->ol_zsize, n)) return 111;
  if (ensure(c, c->ol_zoff, n)) return 111;
  if (ensure(c, c->ol_order, n)) return 111;
  if (ensure(c, c->ol_node, 3 * (uint64_t)E)) return 111;
  if (ensure(c, c->enc_blob, bound)) return 111;
  // each entry's node; an entry without a fragment keeps (0, 0, 0)
  std::vector<int32_t> node_of(3 * (size_t)E, 0);
  for (uint32_t r = 0; r < n; ++r)
    for (int k = 0; k < 3; ++k)
      node_of[3 * (size_t)en.order[r] + k] = en.nodes[3 * (size_t)r + k];
  HIP_TRY(c, hipMemcpyAsync(c->ol_order.get(), en.order.data(), n * 4ull,
                            hipMemcpyHostToDevice, s), 111);
  HIP_TRY(c, hipMemcpyAsync(c->ol_node.get(), node_of.data(), E * 12ull,
                            hipMemcpyHostToDevice, s), 111);
  HIP_TRY(c, hipMemsetAsync(c->enc_off.get(), 0, E * 8ull, s), 111);
  HIP_TRY(c, hipStreamSynchronize(s), 111);  // the tables are read
  uint8_t *blob = c->enc_blob.get();
  const EncTables t = {en.vbase, en.tri_off, c->enc_ilen.get(),
                       c->enc_off.get(), E};
  EncParams p = {};
  p.draco = ENC_DRACO_INT;
  const dim3 blk(ENC_BLK), nbe((E + ENC_BLK - 1) / ENC_BLK),
      nbn((n + ENC_BLK - 1) / ENC_BLK);
  hipLaunchKernelGGL(k_enc_varint_sum, dim3(E), blk, 0, s, en.d_faces, t,
                     c->enc_ilen.get());
  hipLaunchKernelGGL(k_ol_sizes, nbn, blk, 0, s, t, c->ol_order.get(), n,
                     c->ol_zsize.get());
  if (int e = scan_u64(c, c->ol_zsize.get(), c->ol_zoff.get(), n, s,
                       "encode_octree_level scan size query failed",
                       "encode_octree_level scan failed", 113))
    return e;
  hipLaunchKernelGGL(k_ol_offsets, nbn, blk, 0, s, c->ol_order.get(),
                     c->ol_zoff.get(), n, c->enc_off.get());
  if (V > 0)
    hipLaunchKernelGGL(k_ol_verts,
                       dim3((uint32_t)((V + ENC_BLK - 1) / ENC_BLK)), blk, 0,
                       s, en.d_verts, t, q, c->ol_node.get(), blob,
                       (uint32_t)V);
  if (NC > 0)
    hipLaunchKernelGGL(k_enc_faces,
                       dim3((uint32_t)((NC + ENC_BLK - 1) / ENC_BLK)), blk, 0,
                       s, en.d_faces, t, ENC_DRACO_INT, blob, NC);
  hipLaunchKernelGGL(k_enc_varint_write, dim3(E), blk, 0, s, en.d_faces, t,
                     blob);
  hipLaunchKernelGGL(k_enc_headers, nbe, blk, 0, s, t, p,
                     (const uint32_t *)nullptr, (float *)nullptr, blob);
  HIP_TRY(c, hipGetLastError(), 113);

  mg_fragset *fs = nullptr;
  if (int e = new_fragset(c, n, &fs)) return e;
  auto fail = [&](int rc) {
    free(fs);
    return rc;
  };
  if (hipMemcpyAsync(fs->offset, c->ol_zoff.get(), n * 8ull,
                     hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(fs->size, c->ol_zsize.get(), n * 8ull,
                     hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    SET_ERR(c, "encode_octree_level: table download failed");
    return fail(114);
  }
  const uint64_t total = fs->offset[n - 1] + fs->size[n - 1];
  if (total > bound) {  // cannot happen; never copy past the allocation
    SET_ERR(c, "encode_octree_level: blob of %llu bytes exceeds its bound "
            "%llu", (unsigned long long)total, (unsigned long long)bound);
    return fail(114);
  }
  if (ensure(c, c->h_blob, total + 1)) return fail(114);
  if (total > 0 &&
      (hipMemcpyAsync(c->h_blob.get(), blob, total, hipMemcpyDeviceToHost,
                      s) != hipSuccess ||
       hipStreamSynchronize(s) != hipSuccess)) {
    SET_ERR(c, "encode_octree_level: blob download failed");
    return fail(114);
  }
  memcpy(fs->nodes, en.nodes.data(), n * 12ull);
  memcpy(fs->nverts, en.nv.data(), n * 4ull);
  memcpy(fs->ntris, en.nf.data(), n * 4ull);
  fs->blob = c->h_blob.get();
  fs->blob_bytes = total;
  *out = fs;
  return 0;
}

// a level without bytes: no fragment (chunked), or the one empty fragment
// at (0, 0, 0) of a mesh without faces
static int ol_empty(mg_ctx *c, const mg_octree_level *lv, uint32_t nverts,
                    mg_fragset **out) {
  if (int e = new_fragset(c, lv->chunked ? 0 : 1, out)) return e;
  if (!lv->chunked) (*out)->nverts[0] = nverts;
  if (ensure(c, c->h_blob, 1)) {
    free(*out);
    *out = nullptr;
    return 114;
  }
  (*out)->blob = c->h_blob.get();
  return 0;
}

static int run_octree_level(mg_ctx *c, const float *verts, uint32_t nverts,
                            const uint32_t *faces, uint32_t ntris,
                            const mg_octree_level *lv, mg_fragset **out) {
  hipStream_t s = c->stream;
  OlQuant q;
  if (lv->retriangulate) {
    if (int e = mv_check_radius(c, lv->radius)) return e;
    if (int e = cm_validate(c, verts, nverts, faces, ntris, lv->upper_scale,
                            lv->offset))
      return e;
  }
  if (int e = cm_validate(c, verts, nverts, faces, ntris, lv->scale,
                          lv->offset))
    return e;
  if (int e = ol_check_params(c, lv, &q)) return e;
  if (ntris == 0) return ol_empty(c, lv, nverts, out);

  // M, in cm_verts / cm_faces from here on
  uint32_t V = nverts, T = ntris;
  if (int e = cm_upload(c, verts, nverts, faces, ntris)) return e;
  if (lv->retriangulate) {
    MvCall mk;
    bool no_cells = true;
    if (int e = mv_retriangulate_device(c, mk, V, T, lv->upper_scale,
                                        lv->offset, lv->radius, &no_cells))
      return e;
    if (!no_cells) {
      V = mk.out_nverts;
      T = mk.out_ntris;
      if (T == 0) return ol_empty(c, lv, V, out);
      if (int e = cm_ensure_input(c, V, T)) return e;
      HIP_TRY(c, hipMemcpyAsync(c->cm_verts.get(), c->mv_out_v.get(),
                                (uint64_t)V * 12, hipMemcpyDeviceToDevice, s),
              111);
      HIP_TRY(c, hipMemcpyAsync(c->cm_faces.get(), c->mv_out_f.get(),
                                (uint64_t)T * 12, hipMemcpyDeviceToDevice, s),
              111);
    }
  }

  OlEntries en;
  if (!lv->chunked) {
    const uint32_t pref[4] = {0, V, 0, T};
    if (ensure(c, c->ol_pref, 4)) return 111;
    HIP_TRY(c, hipMemcpyAsync(c->ol_pref.get(), pref, sizeof(pref),
                              hipMemcpyHostToDevice, s), 111);
    HIP_TRY(c, hipStreamSynchronize(s), 111);  // pref is read
    en.d_verts = c->cm_verts.get();
    en.d_faces = c->cm_faces.get();
    en.V = V;
    en.T = T;
    en.vbase = c->ol_pref.get();
    en.tri_off = c->ol_pref.get() + 2;
    en.E = 1;
    en.order = {0};
    en.nodes = {0, 0, 0};
    en.nv = {V};
    en.nf = {T};
    return ol_encode(c, en, q, out);
  }

  CmCall ck;
  if (int e = cm_run_device(c, ck, V, T, lv->scale, lv->offset)) return e;
  CmCellTable t;
  if (int e = cm_read_cells(c, ck, t)) return e;
  const uint32_t n = (uint32_t)t.live.size();
  if (n == 0) return ol_empty(c, lv, 0, out);
  // the live cells in dict order, their z-order, the entry of each z-rank
  std::vector<int32_t> dict_nodes(3 * (size_t)n);
  for (uint32_t m = 0; m < n; ++m) {
    const uint32_t d = t.dense[t.live[t.order[m]]] >> 1;
    dict_nodes[3 * (size_t)m + 2] = (int32_t)(d % ck.dn.nz) + ck.dn.lo[2];
    dict_nodes[3 * (size_t)m + 1] =
        (int32_t)((d / ck.dn.nz) % ck.dn.ny) + ck.dn.lo[1];
    dict_nodes[3 * (size_t)m + 0] =
        (int32_t)(d / ck.dn.nz / ck.dn.ny) + ck.dn.lo[0];
  }
  std::vector<uint32_t> perm;
  if (int e = ol_zorder(c, lv, dict_nodes, n, perm)) return e;
  const uint64_t stride = (uint64_t)ck.ncellp + 1;
  en.d_verts = c->cm_out_v.get();
  en.d_faces = c->cm_out_f.get();
  en.V = t.V;
  en.T = t.F;
  en.vbase = c->cm_cells.get() + CM_CELL_VB * stride;
  en.tri_off = c->cm_cells.get() + CM_CELL_FB * stride;
  en.E = ck.ncellp;
  en.order.resize(n);
  en.nodes.resize(3 * (size_t)n);
  en.nv.resize(n);
  en.nf.resize(n);
  for (uint32_t r = 0; r < n; ++r) {
    const uint32_t o = t.live[t.order[perm[r]]];
    en.order[r] = o;
    for (int k = 0; k < 3; ++k)
      en.nodes[3 * (size_t)r + k] = dict_nodes[3 * (size_t)perm[r] + k];
    en.nv[r] = t.vb[o + 1] - t.vb[o];
    en.nf[r] = t.fb[o + 1] - t.fb[o];
  }
  return ol_encode(c, en, q, out);
}
