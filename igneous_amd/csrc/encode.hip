// encode.hip — stage [7b]: fragment bytes and bounding boxes on the device
// (mg_mesh_chunk_encoded; replaces MeshTask's per-label host loop of shift,
// np.amin/np.amax and Mesh.to_precomputed / formats.draco.encode). Included
// from meshgine.hip after the stage drivers (ChunkCall, scan_u64, ev_ms).
//
// Contract (restated by tests/encode_ref.py):
//   per label, V' = V + shift (one f32 add per component), box = min/max of
//   V', and the entry bytes
//     precomputed  u32 nv | V' 3*nv f32 | F 3*nf u32
//     draco        11-B header | varint nf | varint nv | u8 1 | indices at
//                  u8 / u16 / varint / u32 by nv < 2^8 / 2^16 / 2^21 / else |
//                  10-B attribute header | 3*nv u32
//                  clip(rint(((f64)v' - o) / r * qmax), 0, 2^32-1) |
//                  o as 3 f32 | r as f32 | bits as u8
//   a label without vertices gets an entry of size 0.
//
// Entries lie in the blob in label-ID order (the order verts / faces already
// have), back to back; the host sorts only the table by label value.
//
// Launches, visibility from kernel boundaries only (no spin flags, no grid
// sync, every loop bounded):
//   k_enc_varint_sum    draco: block per label of the varint band, sum of
//                       the per-index lengths (0 for every other label)
//   k_enc_sizes         thread per label: entry size; box words reset
//   rocPRIM scan (u64)  sizes -> entry offsets
//   k_enc_verts         thread per vertex: label from the block's staged
//                       vbase range, shift, segmented wave min/max then
//                       atomicMin/atomicMax on order-preserving u32 words
//                       (order-free atomics), f32 or quantised
//                       u32 out
//   k_enc_faces         thread per corner: index at the entry's width
//   k_enc_varint_write  draco: block per label of the varint band, block
//                       scan of the lengths chunk by chunk, bytes out
//   k_enc_headers       thread per label: header, trailer, box as f32
// The kernels know entries only through an EncTables (two prefix tables and
// an offset table), so octree_level.hip drives k_enc_varint_sum, k_enc_faces,
// k_enc_varint_write and k_enc_headers over the cells of an octree level,
// with the integer draco layout (ENC_DRACO_INT: DT_UINT32 / sequential
// INTEGER attribute, no trailer, no boxes) and a vertex kernel of its own.
// Precomputed entries are multiples of 4 B at 4-aligned offsets and are
// stored as dwords; draco entries are odd-sized and stored byte by byte —
// no blob address is ever cast to a wider pointer there.

#define ENC_BLK 256
#define ENC_BAND_U8 0
#define ENC_BAND_U16 1
#define ENC_BAND_VARINT 2
#define ENC_BAND_U32 3
// draco bytes around the data: header 11, attribute header 10, trailer 17,
// two varints of at most 5, the connectivity byte
#define ENC_DRACO_FIXED_MAX (11 + 5 + 5 + 1 + 10 + 17)
// the `draco` argument of the layout and of the kernels: 0 precomputed,
// ENC_DRACO_FLOAT the quantised f32 attribute with its 17-byte trailer,
// ENC_DRACO_INT the integer attribute of octree_level.hip, no trailer
#define ENC_DRACO_FLOAT 1
#define ENC_DRACO_INT 2

// final numbers of one call (the wrapper's defaulting is already applied)
struct EncParams {
  int draco;
  float shift[3];
  double o[3], r, qmax;
  float of[3], rf;  // trailer: origin and range as f32
  uint32_t bits;
};

// the per-entry arrays every kernel derives an entry's layout from (an
// entry is a label here, a grid cell in octree_level.hip)
struct EncTables {
  const uint32_t *vbase, *tri_off;  // nlabels + 1 each
  const uint64_t *ilen;             // draco: varint index bytes per label
  const uint64_t *off;              // entry offsets (after the scan)
  uint32_t nlabels;
};

struct EncLayout {
  uint32_t nv, nf, band;
  uint64_t ipos, vpos, size;  // ipos/vpos relative to the entry's start
};

__device__ __forceinline__ uint32_t enc_vlen(uint32_t x) {
  return x < (1u << 7) ? 1 : x < (1u << 14) ? 2 : x < (1u << 21) ? 3
       : x < (1u << 28) ? 4 : 5;
}

__device__ __forceinline__ uint32_t enc_put_varint(uint8_t *p, uint32_t x) {
  uint32_t n = 0;
  for (int i = 0; i < 5; ++i) {
    const uint32_t b = x & 0x7Fu;
    x >>= 7;
    p[n++] = (uint8_t)(x ? (b | 0x80u) : b);
    if (!x) break;
  }
  return n;
}

__device__ __forceinline__ void enc_put_u32(uint8_t *p, uint32_t x) {
  p[0] = (uint8_t)x;
  p[1] = (uint8_t)(x >> 8);
  p[2] = (uint8_t)(x >> 16);
  p[3] = (uint8_t)(x >> 24);
}

__device__ __forceinline__ uint32_t enc_band(uint32_t nv) {
  return nv < (1u << 8) ? ENC_BAND_U8 : nv < (1u << 16) ? ENC_BAND_U16
       : nv < (1u << 21) ? ENC_BAND_VARINT : ENC_BAND_U32;
}

__device__ __forceinline__ EncLayout enc_layout(const EncTables &t, int draco,
                                                uint32_t l) {
  EncLayout e;
  e.nv = t.vbase[l + 1] - t.vbase[l];
  e.nf = t.tri_off[l + 1] - t.tri_off[l];
  e.band = enc_band(e.nv);
  if (!draco) {
    e.vpos = 4;
    e.ipos = 4 + 12ull * e.nv;
    e.size = e.ipos + 12ull * e.nf;
  } else {
    e.ipos = 11 + enc_vlen(e.nf) + enc_vlen(e.nv) + 1;
    const uint64_t idx = e.band == ENC_BAND_U8    ? 3ull * e.nf
                         : e.band == ENC_BAND_U16 ? 6ull * e.nf
                         : e.band == ENC_BAND_U32 ? 12ull * e.nf
                                                  : t.ilen[l];
    e.vpos = e.ipos + idx + 10;
    e.size = e.vpos + 12ull * e.nv + (draco == ENC_DRACO_INT ? 0 : 17);
  }
  if (e.nv == 0) e.size = 0;
  return e;
}

// order-preserving u32 image of an f32 (-0.0 sorts just below +0.0)
__device__ __forceinline__ uint32_t enc_ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float enc_unord(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// largest l in [lo, hi] with off[l] <= i; off ascending, off[lo] <= i
__device__ __forceinline__ uint32_t enc_find(const uint32_t *off, uint32_t lo,
                                             uint32_t hi, uint32_t i) {
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Label of item `mine` (a vertex or a triangle) of a block whose threads
// cover the items [first, last] of off[0..n]: thread 0 finds the labels of
// the block's two ends, the block stages that range of off in LDS and each
// thread searches only there (a range wider than the block, which needs
// empty labels in between, is searched in place). Every thread of the block
// calls this; ~0u for an invalid thread.
__device__ __forceinline__ uint32_t enc_block_label(
    const uint32_t *__restrict__ off, uint32_t n, uint32_t first,
    uint32_t last, uint32_t mine, bool valid, uint32_t *s_off,
    uint32_t *s_rng) {
  if (threadIdx.x == 0) {
    const uint32_t lo = enc_find(off, 0, n - 1, first);
    s_rng[0] = lo;
    s_rng[1] = enc_find(off, lo, n - 1, last);
  }
  __syncthreads();
  const uint32_t lo = s_rng[0], span = s_rng[1] - lo;
  const bool staged = span < ENC_BLK;
  if (staged && threadIdx.x <= span) s_off[threadIdx.x] = off[lo + threadIdx.x];
  __syncthreads();
  if (!valid) return ~0u;
  return lo + enc_find(staged ? s_off : off + lo, 0, span, mine);
}

__global__ void __launch_bounds__(ENC_BLK)
k_enc_varint_sum(const uint32_t *__restrict__ faces, EncTables t,
                 uint64_t *__restrict__ ilen) {
  __shared__ uint64_t s_sum[ENC_BLK / WAVE];
  const uint32_t l = blockIdx.x;
  const uint32_t nv = t.vbase[l + 1] - t.vbase[l];
  if (enc_band(nv) != ENC_BAND_VARINT) {  // uniform over the block
    if (threadIdx.x == 0) ilen[l] = 0;
    return;
  }
  const uint64_t c0 = 3ull * t.tri_off[l];
  const uint64_t nc = 3ull * (t.tri_off[l + 1] - t.tri_off[l]);
  uint64_t sum = 0;
  for (uint64_t k = threadIdx.x; k < nc; k += ENC_BLK)
    sum += enc_vlen(faces[c0 + k]);
  for (int d = WAVE / 2; d > 0; d >>= 1) sum += __shfl_down(sum, d, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) s_sum[threadIdx.x / WAVE] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t tot = 0;
    for (int w = 0; w < ENC_BLK / WAVE; ++w) tot += s_sum[w];
    ilen[l] = tot;
  }
}

__global__ void k_enc_sizes(EncTables t, int draco,
                            uint64_t *__restrict__ size,
                            uint32_t *__restrict__ box) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= t.nlabels) return;
  size[l] = enc_layout(t, draco, l).size;
  for (int k = 0; k < 3; ++k) {
    box[6 * (uint64_t)l + k] = 0xFFFFFFFFu;
    box[6 * (uint64_t)l + 3 + k] = 0u;
  }
}

__global__ void __launch_bounds__(ENC_BLK)
k_enc_verts(const float *__restrict__ verts, EncTables t, EncParams p,
            uint32_t *__restrict__ box, uint8_t *__restrict__ blob,
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
  uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  uint32_t hi[3] = {0u, 0u, 0u};
  if (valid) {
    const EncLayout e = enc_layout(t, p.draco, l);
    const uint64_t j = i - t.vbase[l];
    uint8_t *dst = blob + t.off[l] + e.vpos + 12 * j;
    for (int k = 0; k < 3; ++k) {
      const float x = verts[3 * (uint64_t)i + k] + p.shift[k];
      lo[k] = hi[k] = enc_ord(x);
      if (!p.draco) {
        reinterpret_cast<float *>(dst)[k] = x;  // 4-aligned entry
      } else {
        // one IEEE f64 operation per step, in formats/draco.py's order
        double q = (double)x - p.o[k];
        q = q / p.r;
        q = q * p.qmax;
        q = rint(q);
        q = q < 0.0 ? 0.0 : q > 4294967295.0 ? 4294967295.0 : q;
        enc_put_u32(dst + 4 * k, (uint32_t)q);
      }
    }
  }
  // segmented min/max over the wave: labels are contiguous runs of lanes,
  // so after the doubling steps a run's first lane holds the run's box
  const int lane = threadIdx.x & (WAVE - 1);
  for (int d = 1; d < WAVE; d <<= 1) {
    const uint32_t ol = __shfl_down(l, d, WAVE);
    const bool take = lane + d < WAVE && ol == l;
    for (int k = 0; k < 3; ++k) {
      const uint32_t a = __shfl_down(lo[k], d, WAVE);
      const uint32_t b = __shfl_down(hi[k], d, WAVE);
      if (take) {
        lo[k] = min(lo[k], a);
        hi[k] = max(hi[k], b);
      }
    }
  }
  const uint32_t prev = __shfl_up(l, 1, WAVE);
  if (valid && (lane == 0 || prev != l)) {
    for (int k = 0; k < 3; ++k) {
      atomicMin(&box[6 * (uint64_t)l + k], lo[k]);
      atomicMax(&box[6 * (uint64_t)l + 3 + k], hi[k]);
    }
  }
}

__global__ void __launch_bounds__(ENC_BLK)
k_enc_faces(const uint32_t *__restrict__ faces, EncTables t, int draco,
            uint8_t *__restrict__ blob, uint64_t NC) {
  __shared__ uint32_t s_off[ENC_BLK];
  __shared__ uint32_t s_rng[2];
  const uint64_t first = (uint64_t)blockIdx.x * ENC_BLK;
  const uint64_t last = min(first + ENC_BLK - 1, NC - 1);
  const uint64_t i = first + threadIdx.x;
  const bool valid = i < NC;
  const uint32_t l = enc_block_label(
      t.tri_off, t.nlabels, (uint32_t)(first / 3), (uint32_t)(last / 3),
      (uint32_t)(i / 3), valid, s_off, s_rng);
  if (!valid) return;
  const EncLayout e = enc_layout(t, draco, l);
  const uint64_t j = i - 3ull * t.tri_off[l];
  const uint32_t idx = faces[i];
  uint8_t *dst = blob + t.off[l] + e.ipos;
  if (!draco) {
    reinterpret_cast<uint32_t *>(dst)[j] = idx;  // 4-aligned entry
  } else if (e.band == ENC_BAND_U8) {
    dst[j] = (uint8_t)idx;
  } else if (e.band == ENC_BAND_U16) {
    dst[2 * j] = (uint8_t)idx;
    dst[2 * j + 1] = (uint8_t)(idx >> 8);
  } else if (e.band == ENC_BAND_U32) {
    enc_put_u32(dst + 4 * j, idx);
  }  // the varint band is k_enc_varint_write's
}

__global__ void __launch_bounds__(ENC_BLK)
k_enc_varint_write(const uint32_t *__restrict__ faces, EncTables t,
                   uint8_t *__restrict__ blob) {
  __shared__ uint32_t s_wave[ENC_BLK / WAVE];
  const uint32_t l = blockIdx.x;
  const EncLayout e = enc_layout(t, 1, l);
  if (e.band != ENC_BAND_VARINT) return;  // uniform over the block
  const uint64_t c0 = 3ull * t.tri_off[l], nc = 3ull * e.nf;
  uint8_t *dst = blob + t.off[l] + e.ipos;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  uint64_t base = 0;  // bytes written by the chunks before this one
  for (uint64_t k0 = 0; k0 < nc; k0 += ENC_BLK) {
    const uint64_t k = k0 + threadIdx.x;
    const uint32_t idx = k < nc ? faces[c0 + k] : 0u;
    const uint32_t len = k < nc ? enc_vlen(idx) : 0u;
    const uint32_t incl = wave_incl_scan(len, lane);
    if (lane == WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int w = 0; w < ENC_BLK / WAVE; ++w) {
      if (w < wave) before += s_wave[w];
      total += s_wave[w];
    }
    if (len) enc_put_varint(dst + base + before + (incl - len), idx);
    base += total;
    __syncthreads();  // s_wave is rewritten by the next chunk
  }
}

__global__ void k_enc_headers(EncTables t, EncParams p,
                              const uint32_t *__restrict__ box,
                              float *__restrict__ bbox,
                              uint8_t *__restrict__ blob) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= t.nlabels) return;
  const EncLayout e = enc_layout(t, p.draco, l);
  if (bbox) {  // the integer layout has no boxes
    float *bb = bbox + 6 * (uint64_t)l;
    for (int k = 0; k < 6; ++k)
      bb[k] = e.nv == 0 ? 0.0f : enc_unord(box[6 * (uint64_t)l + k]);
  }
  if (e.nv == 0) return;
  uint8_t *dst = blob + t.off[l];
  if (!p.draco) {
    *reinterpret_cast<uint32_t *>(dst) = e.nv;  // 4-aligned entry
    return;
  }
  // "DRACO", version 2.2, TRIANGULAR_MESH, sequential, u16 flags 0
  const uint8_t head[11] = {'D', 'R', 'A', 'C', 'O', 2, 2, 1, 0, 0, 0};
  for (int k = 0; k < 11; ++k) dst[k] = head[k];
  uint32_t at = 11;
  at += enc_put_varint(dst + at, e.nf);
  at += enc_put_varint(dst + at, e.nv);
  dst[at] = 1;  // raw indices
  // one attributes decoder, one attribute, POSITION, DT_FLOAT32, 3
  // components, not normalised, unique id 0, sequential QUANTIZATION,
  // prediction NONE (-2), uncompressed values
  // (ENC_DRACO_INT: DT_UINT32 and sequential INTEGER, and no trailer)
  const bool integer = p.draco == ENC_DRACO_INT;
  const uint8_t attr[10] = {1, 1, 0, (uint8_t)(integer ? 6 : 9), 3, 0, 0,
                            (uint8_t)(integer ? 1 : 2), 0xFE, 0};
  uint8_t *a = dst + e.vpos - 10;
  for (int k = 0; k < 10; ++k) a[k] = attr[k];
  if (integer) return;
  uint8_t *tr = dst + e.vpos + 12ull * e.nv;
  for (int k = 0; k < 3; ++k) enc_put_u32(tr + 4 * k, __float_as_uint(p.of[k]));
  enc_put_u32(tr + 12, __float_as_uint(p.rf));
  tr[16] = (uint8_t)p.bits;
}

// ---------------------------------------------------------------------------
// host driver

// The result descriptor, one calloc: mg_blobset, then labels / offset / size
// (u64), nverts / ntris (u32) and bbox (6 f32) per entry.
static int new_blobset(mg_ctx *c, uint32_t n, mg_blobset **out) {
  mg_blobset *bs = (mg_blobset *)calloc(
      1, sizeof(mg_blobset) + (size_t)n * (3 * 8 + 2 * 4 + 6 * 4) + 8);
  if (!bs) {
    SET_ERR(c, "mesh_chunk_encoded: out of host memory");
    return 24;
  }
  bs->n = n;
  bs->labels = (uint64_t *)((char *)bs + sizeof(mg_blobset));
  bs->offset = bs->labels + n;
  bs->size = bs->offset + n;
  bs->nverts = (uint32_t *)(bs->size + n);
  bs->ntris = bs->nverts + n;
  bs->bbox = (float *)(bs->ntris + n);
  *out = bs;
  return 0;
}

// NULL params, unknown format, non-finite numbers, range <= 0, bits outside
// 1..32: rejected before any kernel. Fills the kernels' EncParams.
static int check_encode_params(mg_ctx *c, const mg_encode_params *ep,
                               EncParams *p) {
  if (!ep) {
    SET_ERR(c, "encode: null mg_encode_params");
    return 8;
  }
  if (ep->format != MG_ENC_PRECOMPUTED && ep->format != MG_ENC_DRACO) {
    SET_ERR(c, "encode: unknown format %u", ep->format);
    return 8;
  }
  *p = EncParams{};
  p->draco = ep->format == MG_ENC_DRACO;
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(ep->shift[k])) {
      SET_ERR(c, "encode: non-finite shift[%d]", k);
      return 8;
    }
    p->shift[k] = ep->shift[k];
  }
  if (!p->draco) return 0;
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(ep->q_origin[k])) {
      SET_ERR(c, "encode: non-finite q_origin[%d]", k);
      return 8;
    }
    p->o[k] = ep->q_origin[k];
    p->of[k] = (float)ep->q_origin[k];
  }
  if (!std::isfinite(ep->q_range)) {
    SET_ERR(c, "encode: non-finite q_range");
    return 8;
  }
  if (ep->q_range <= 0) {
    SET_ERR(c, "encode: q_range %g must be > 0", ep->q_range);
    return 8;
  }
  if (ep->q_bits < 1 || ep->q_bits > 32) {
    SET_ERR(c, "encode: q_bits %u outside 1..32", ep->q_bits);
    return 8;
  }
  p->r = ep->q_range;
  p->rf = (float)ep->q_range;
  p->bits = ep->q_bits;
  p->qmax = (double)((1ull << ep->q_bits) - 1);
  return 0;
}

// [7b] encode every label's fragment into c->enc_blob, then D2H of the
// per-label tables and of the blob into the ctx's pinned staging. Under
// MG_FLAG_DEVICE_ONLY the kernels run, nothing is copied and the set is
// empty. Records EV_ENCODE_END after the last kernel.
static int run_encode(mg_ctx *c, const ChunkCall &k, uint32_t flags,
                      const EncParams &p, mg_blobset **out) {
  hipStream_t s = c->stream;
  const uint32_t n = k.nlabels;
  const uint64_t V = k.V, NC = 3 * k.T;
  // the blob's size is known only after the scan; this bound (exact for
  // precomputed with no empty label) lets every kernel queue without a sync
  const uint64_t bound = 12 * V + 4 * NC +
                         (uint64_t)n * (p.draco ? ENC_DRACO_FIXED_MAX : 4);
  if (ensure(c, c->enc_size, n)) return 26;
  if (ensure(c, c->enc_off, n)) return 26;
  if (ensure(c, c->enc_box, 6 * (uint64_t)n)) return 26;
  if (ensure(c, c->enc_bbox, 6 * (uint64_t)n)) return 26;
  if (ensure(c, c->enc_blob, bound)) return 26;
  if (p.draco && ensure(c, c->enc_ilen, n)) return 26;
  uint8_t *blob = c->enc_blob.get();
  const EncTables t = {c->vbase.get(), c->tri_off.get(),
                       p.draco ? c->enc_ilen.get() : nullptr,
                       c->enc_off.get(), n};
  const dim3 blk(ENC_BLK), nbl((n + ENC_BLK - 1) / ENC_BLK);
  if (p.draco)
    hipLaunchKernelGGL(k_enc_varint_sum, dim3(n), blk, 0, s, c->faces.get(),
                       t, c->enc_ilen.get());
  hipLaunchKernelGGL(k_enc_sizes, nbl, blk, 0, s, t, p.draco,
                     c->enc_size.get(), c->enc_box.get());
  if (int e = scan_u64(c, c->enc_size.get(), c->enc_off.get(), n, s,
                       "encode scan size query failed", "encode scan failed",
                       26))
    return e;
  if (V > 0)
    hipLaunchKernelGGL(k_enc_verts, dim3((uint32_t)((V + ENC_BLK - 1) / ENC_BLK)),
                       blk, 0, s, c->verts.get(), t, p, c->enc_box.get(),
                       blob, (uint32_t)V);
  if (NC > 0)
    hipLaunchKernelGGL(k_enc_faces,
                       dim3((uint32_t)((NC + ENC_BLK - 1) / ENC_BLK)), blk, 0,
                       s, c->faces.get(), t, p.draco, blob, NC);
  if (p.draco)
    hipLaunchKernelGGL(k_enc_varint_write, dim3(n), blk, 0, s,
                       c->faces.get(), t, blob);
  hipLaunchKernelGGL(k_enc_headers, nbl, blk, 0, s, t, p, c->enc_box.get(),
                     c->enc_bbox.get(), blob);
  HIP_TRY(c, hipGetLastError(), 26);
  HIP_TRY(c, hipEventRecord(c->ev[EV_ENCODE_END], s), 26);
  if (flags & MG_FLAG_DEVICE_ONLY) {
    HIP_TRY(c, hipStreamSynchronize(s), 27);
    return new_blobset(c, 0, out);
  }

  std::vector<uint64_t> h_off(n), h_size(n), h_label_values(n);
  std::vector<uint32_t> h_tri_off(n + 1), h_vbase(n + 1);
  std::vector<float> h_bbox(6 * (size_t)n);
  HIP_TRY(c, hipMemcpyAsync(h_off.data(), c->enc_off.get(), n * 8ull,
                            hipMemcpyDeviceToHost, s), 27);
  HIP_TRY(c, hipMemcpyAsync(h_size.data(), c->enc_size.get(), n * 8ull,
                            hipMemcpyDeviceToHost, s), 27);
  HIP_TRY(c, hipMemcpyAsync(h_label_values.data(), c->label_values.get(),
                            n * 8ull, hipMemcpyDeviceToHost, s), 27);
  HIP_TRY(c, hipMemcpyAsync(h_tri_off.data(), c->tri_off.get(),
                            (n + 1) * 4ull, hipMemcpyDeviceToHost, s), 27);
  HIP_TRY(c, hipMemcpyAsync(h_vbase.data(), c->vbase.get(), (n + 1) * 4ull,
                            hipMemcpyDeviceToHost, s), 27);
  HIP_TRY(c, hipMemcpyAsync(h_bbox.data(), c->enc_bbox.get(), n * 24ull,
                            hipMemcpyDeviceToHost, s), 27);
  HIP_TRY(c, hipStreamSynchronize(s), 27);
  const uint64_t total = h_off[n - 1] + h_size[n - 1];
  if (total > bound) {  // cannot happen; never copy past the allocation
    SET_ERR(c, "encode: blob of %llu bytes exceeds its bound %llu",
            (unsigned long long)total, (unsigned long long)bound);
    return 27;
  }
  if (ensure(c, c->h_blob, total + 1)) return 27;
  if (total > 0)
    HIP_TRY(c, hipMemcpyAsync(c->h_blob.get(), blob, total,
                              hipMemcpyDeviceToHost, s), 27);

  // the table by ascending label value, while the blob copy runs
  mg_blobset *bs = nullptr;
  if (int e = new_blobset(c, n, &bs)) return e;
  std::vector<uint32_t> idx(n);
  for (uint32_t i = 0; i < n; ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
    return h_label_values[a] < h_label_values[b];
  });
  for (uint32_t m = 0; m < n; ++m) {
    const uint32_t l = idx[m];
    bs->labels[m] = h_label_values[l];
    bs->offset[m] = h_off[l];
    bs->size[m] = h_size[l];
    bs->nverts[m] = h_vbase[l + 1] - h_vbase[l];
    bs->ntris[m] = h_tri_off[l + 1] - h_tri_off[l];
    memcpy(bs->bbox + 6 * (size_t)m, h_bbox.data() + 6 * (size_t)l, 24);
  }
  bs->blob = c->h_blob.get();
  bs->blob_bytes = total;
  if (hipStreamSynchronize(s) != hipSuccess) {
    free(bs);
    SET_ERR(c, "encode: blob download failed");
    return 27;
  }
  *out = bs;
  return 0;
}
