// fill_holes.hip — hole filling as a device volume pass (MeshTask
// fill_holes levels 1-2; replaces fastmorph.fill_holes_v2 at the
// reference's igneous/tasks/mesh/mesh.py:220). Included from
// meshgine.hip after the ctx helpers (mg_ctx, ensure, SET_ERR, HIP_TRY).
//
// Contract (restated by tests/fill_holes_ref.py):
//   6-connectivity; a component is a maximal 6-connected set of equal
//   value (value 0 included). One round rewrites, simultaneously, every
//   component that touches no border voxel and whose outside face
//   neighbours all carry one value L != 0, to L. Rounds repeat to a fixed
//   point. Level 2 first runs the same rounds on each of the six boundary
//   slices (as one-voxel-thick volumes) in the order x=0, x=sx-1, y=0,
//   y=sy-1, z=0, z=sz-1. holes[v] = input[v] where filled[v] != input[v].
//
// The rounds run on a u32 working volume: the labels themselves for
// MG_U32, dense ids (+1, 0 stays 0) from the engine's label hash for
// MG_U64 — only equality of neighbour values matters, so the ids'
// scheduling-dependent numbering never reaches the output.
//
// One round = five launches; visibility between them comes from kernel
// boundaries only (no spin flags, no grid sync, every loop bounded):
//   k_fill_init     parent[i] = i, cmin = 0xFFFFFFFF, cmax = 0
//   k_fill_link     union-find on voxel indices: link each voxel with its
//                   -x/-y/-z neighbour of equal value, atomicCAS on roots
//                   (a root only ever receives a SMALLER index, so the
//                   final root is the component's minimum linear index)
//   k_fill_flatten  parent[i] = root(i)
//   k_fill_reduce   per root: atomicMin/atomicMax over the differing face
//                   neighbours' values; a border voxel forces min=0,
//                   max=0xFFFFFFFF (order-free atomics only)
//   k_fill_rewrite  enclosed = (min == max && min != 0): voxel <- min,
//                   bump the rewritten-voxel counter the host reads
// A block is addressed through FillGeom strides, so a boundary slice is
// processed in place with dims (a, b, 1).

#define FILL_MAX_ROUNDS 64
#define FILL_BLK 256
#define FILL_MAX_BLOCKS 8192u

struct FillGeom {
  uint32_t nx, ny, nz;     // extent of the addressed block (voxels)
  uint64_t stx, sty, stz;  // element strides into the working volume
  uint64_t base;           // element offset of the block's (0,0,0)
  uint32_t n;              // nx*ny*nz (< 2^32, checked by the driver)
};

__device__ __forceinline__ uint32_t fill_find(uint32_t *parent, uint32_t x) {
  // plain (possibly stale) loads: any value read was once parent[x], so it
  // is a smaller index in the same component; the walk strictly decreases
  // and ends at a node that looked like a root. Path halving only ever
  // rewires a NON-root to another member above it.
  volatile uint32_t *p = parent;
  uint32_t q = p[x];
  while (q != x) {
    uint32_t gp = p[q];
    if (gp != q) p[x] = gp;
    x = q;
    q = gp;
  }
  return x;
}

__device__ __forceinline__ void fill_union(uint32_t *parent, uint32_t a,
                                           uint32_t b) {
  // max(a, b) strictly decreases on every failed CAS: bounded, lock-free
  for (;;) {
    a = fill_find(parent, a);
    b = fill_find(parent, b);
    if (a == b) return;
    if (a < b) { uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicCAS(&parent[a], a, b);  // link only a ROOT
    if (old == a) return;
    a = old;  // a had been linked meanwhile: continue from its parent
  }
}

__global__ void k_fill_init(uint32_t *__restrict__ parent,
                            uint32_t *__restrict__ cmin,
                            uint32_t *__restrict__ cmax, uint32_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    parent[i] = (uint32_t)i;
    cmin[i] = 0xFFFFFFFFu;
    cmax[i] = 0u;
  }
}

__global__ void k_fill_link(const uint32_t *__restrict__ vol, FillGeom g,
                            uint32_t *parent) {
  const uint32_t nxy = g.nx * g.ny;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t x = (uint32_t)(i % g.nx);
    const uint32_t t = (uint32_t)(i / g.nx);
    const uint32_t y = t % g.ny, z = t / g.ny;
    const uint64_t a = g.base + x * g.stx + y * g.sty + z * g.stz;
    const uint32_t v = vol[a];
    if (x && vol[a - g.stx] == v)
      fill_union(parent, (uint32_t)i, (uint32_t)i - 1u);
    if (y && vol[a - g.sty] == v)
      fill_union(parent, (uint32_t)i, (uint32_t)i - g.nx);
    if (z && vol[a - g.stz] == v)
      fill_union(parent, (uint32_t)i, (uint32_t)i - nxy);
  }
}

__global__ void k_fill_flatten(uint32_t *parent, uint32_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    // a concurrent writer stores the root of the same tree: either value
    // read here leads to that root
    volatile uint32_t *p = parent;
    uint32_t x = (uint32_t)i, q = p[x];
    while (q != x) { x = q; q = p[x]; }
    if (x != (uint32_t)i) p[i] = x;
  }
}

__global__ void k_fill_reduce(const uint32_t *__restrict__ vol, FillGeom g,
                              const uint32_t *__restrict__ parent,
                              uint32_t *cmin, uint32_t *cmax) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t x = (uint32_t)(i % g.nx);
    const uint32_t t = (uint32_t)(i / g.nx);
    const uint32_t y = t % g.ny, z = t / g.ny;
    // an axis of size 1 has no border
    const bool border = (g.nx > 1 && (x == 0 || x == g.nx - 1)) ||
                        (g.ny > 1 && (y == 0 || y == g.ny - 1)) ||
                        (g.nz > 1 && (z == 0 || z == g.nz - 1));
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    bool any = false;
    if (border) {
      lo = 0u; hi = 0xFFFFFFFFu; any = true;  // never min == max
    } else {
      // interior on every axis of size > 1: both neighbours exist there
      const uint64_t a = g.base + x * g.stx + y * g.sty + z * g.stz;
      const uint32_t v = vol[a];
      uint32_t w;
#define FILL_NB(cond, off)                                         \
      if (cond) {                                                  \
        w = vol[a - (off)];                                        \
        if (w != v) { lo = min(lo, w); hi = max(hi, w); any = true; } \
        w = vol[a + (off)];                                        \
        if (w != v) { lo = min(lo, w); hi = max(hi, w); any = true; } \
      }
      FILL_NB(g.nx > 1, g.stx)
      FILL_NB(g.ny > 1, g.sty)
      FILL_NB(g.nz > 1, g.stz)
#undef FILL_NB
    }
    if (any) {
      const uint32_t r = parent[i];
      // the plain pre-reads only skip atomics that could not change the
      // word (min only falls, max only rises): a stale read is conservative
      if (((volatile uint32_t *)cmin)[r] > lo) atomicMin(&cmin[r], lo);
      if (((volatile uint32_t *)cmax)[r] < hi) atomicMax(&cmax[r], hi);
    }
  }
}

__global__ void k_fill_rewrite(uint32_t *__restrict__ vol, FillGeom g,
                               const uint32_t *__restrict__ parent,
                               const uint32_t *__restrict__ cmin,
                               const uint32_t *__restrict__ cmax,
                               uint32_t *__restrict__ counter) {
  uint32_t cnt = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = parent[i];
    const uint32_t lo = cmin[r];
    if (lo != 0u && lo == cmax[r]) {
      const uint32_t x = (uint32_t)(i % g.nx);
      const uint32_t t = (uint32_t)(i / g.nx);
      const uint32_t y = t % g.ny, z = t / g.ny;
      vol[g.base + x * g.stx + y * g.sty + z * g.stz] = lo;
      ++cnt;
    }
  }
  if (cnt) atomicAdd(counter, cnt);
}

// u64 labels -> dense ids + 1 (hash built by k_dust_build beforehand)
__global__ void k_fill_to_ids(const uint64_t *__restrict__ labels,
                              uint64_t nvox, LabelHash lh,
                              uint32_t *__restrict__ vol) {
  uint64_t cl = 0;
  uint32_t cr = 0;  // one-entry cache: runs along x share a label
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < nvox; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t L = labels[i];
    if (L != cl) { cl = L; cr = L ? label_lookup(lh, L) + 1u : 0u; }
    vol[i] = cr;
  }
}

// labels <- filled value, holes <- input where it changed (else 0)
template <typename T>
__global__ void k_fill_finish(T *__restrict__ labels, T *__restrict__ holes,
                              const uint32_t *__restrict__ vol,
                              const uint64_t *__restrict__ values,
                              uint64_t nvox) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < nvox; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = vol[i];
    T f;
    if (sizeof(T) == 4) f = (T)w;
    else f = w ? (T)values[w - 1u] : (T)0;
    const T in = labels[i];
    holes[i] = (f != in) ? in : (T)0;
    if (f != in) labels[i] = f;
  }
}

static inline uint32_t fill_blocks(uint64_t n) {
  return (uint32_t)std::min<uint64_t>(
      std::max<uint64_t>((n + FILL_BLK - 1) / FILL_BLK, 1), FILL_MAX_BLOCKS);
}

// Rounds to a fixed point on one block of the working volume. The loop is
// host-driven: one 4-byte counter readback per round, capped.
static int fill_run_rounds(mg_ctx *c, const FillGeom &g, const char *what,
                           uint32_t *rounds_out) {
  hipStream_t s = c->stream;
  uint32_t *vol = c->fill_vol.get();
  uint32_t *parent = c->fill_parent.get();
  uint32_t *cmin = c->fill_cmin.get();
  uint32_t *cmax = c->fill_cmax.get();
  uint32_t *counter = c->fill_misc.get();  // word 0: voxels rewritten
  const dim3 nb(fill_blocks(g.n)), blk(FILL_BLK);
  uint32_t productive = 0;
  for (int round = 0; round < FILL_MAX_ROUNDS; ++round) {
    HIP_TRY(c, hipMemsetAsync(counter, 0, 4, s), 52);
    hipLaunchKernelGGL(k_fill_init, nb, blk, 0, s, parent, cmin, cmax, g.n);
    hipLaunchKernelGGL(k_fill_link, nb, blk, 0, s, vol, g, parent);
    hipLaunchKernelGGL(k_fill_flatten, nb, blk, 0, s, parent, g.n);
    hipLaunchKernelGGL(k_fill_reduce, nb, blk, 0, s, vol, g, parent, cmin,
                       cmax);
    hipLaunchKernelGGL(k_fill_rewrite, nb, blk, 0, s, vol, g, parent, cmin,
                       cmax, counter);
    HIP_TRY(c, hipGetLastError(), 52);
    uint32_t rewritten = 0;
    HIP_TRY(c, hipMemcpyAsync(&rewritten, counter, 4, hipMemcpyDeviceToHost,
                              s), 52);
    HIP_TRY(c, hipStreamSynchronize(s), 52);
    if (rewritten == 0) {
      if (rounds_out) *rounds_out = productive;
      return 0;
    }
    ++productive;
  }
  SET_ERR(c, "fill_holes did not converge on %s after %d rounds "
          "(nesting deeper than the round cap)", what, FILL_MAX_ROUNDS);
  return 53;
}

// Fill the resident c->labels (sx*sy*sz of dtype) in place and leave the
// hole volume in c->holes. rounds_out = productive rounds of the 3-D phase.
static int run_fill_holes(mg_ctx *c, int dtype, int sx, int sy, int sz,
                          uint32_t level, uint32_t *rounds_out) {
  hipStream_t s = c->stream;
  const size_t esize = (dtype == MG_U64) ? 8 : 4;
  const uint64_t nvox = (uint64_t)sx * sy * sz;
  if (nvox >= (1ull << 32) / 6) {  // u32 voxel indices (engine-wide bound)
    SET_ERR(c, "fill_holes: %llu voxels exceed the u32 voxel-index bound; "
            "split the task shape", (unsigned long long)nvox);
    return 50;
  }
  for (auto *b : {&c->fill_vol, &c->fill_parent, &c->fill_cmin, &c->fill_cmax})
    if (ensure(c, *b, nvox)) return 51;
  if (ensure_bytes(c, c->holes, nvox * esize)) return 51;
  if (ensure(c, c->fill_misc, 64)) return 51;
  uint32_t *vol = c->fill_vol.get();
  const dim3 vnb(fill_blocks(nvox)), blk(FILL_BLK);

  // working volume
  if (dtype == MG_U32) {
    HIP_TRY(c, hipMemcpyAsync(vol, c->labels.ptr, nvox * 4,
                              hipMemcpyDeviceToDevice, s), 51);
  } else {
    uint32_t nl = 0;  // label hash, grow-and-retry like the dust passes
    if (int e = hash_volume_labels(c, dtype, nvox, " (fill_holes)", 51, &nl))
      return e;
    const LabelHash lh = label_hash_view(c);
    if (ensure(c, c->label_values, std::max(nl, 1u))) return 51;
    hipLaunchKernelGGL(k_label_values,
                       dim3((uint32_t)((c->lh_slots + 255) / 256)),
                       dim3(256), 0, s, lh, c->label_values.get(),
                       c->lh_slots);
    hipLaunchKernelGGL(k_fill_to_ids, vnb, blk, 0, s,
                       c->labels.as<const uint64_t>(), nvox, lh, vol);
    HIP_TRY(c, hipGetLastError(), 51);
  }

  const uint64_t usx = sx, usy = sy, usz = sz, sxy = usx * usy;
  if (level >= 2) {
    // boundary slices as one-voxel-thick volumes, addressed in place;
    // later slices see earlier ones
    const FillGeom sl[6] = {
        {(uint32_t)sy, (uint32_t)sz, 1, usx, sxy, 0, 0, (uint32_t)(usy * usz)},
        {(uint32_t)sy, (uint32_t)sz, 1, usx, sxy, 0, usx - 1,
         (uint32_t)(usy * usz)},
        {(uint32_t)sx, (uint32_t)sz, 1, 1, sxy, 0, 0, (uint32_t)(usx * usz)},
        {(uint32_t)sx, (uint32_t)sz, 1, 1, sxy, 0, (usy - 1) * usx,
         (uint32_t)(usx * usz)},
        {(uint32_t)sx, (uint32_t)sy, 1, 1, usx, 0, 0, (uint32_t)sxy},
        {(uint32_t)sx, (uint32_t)sy, 1, 1, usx, 0, (usz - 1) * sxy,
         (uint32_t)sxy},
    };
    static const char *const names[6] = {"slice x=0", "slice x=sx-1",
                                         "slice y=0", "slice y=sy-1",
                                         "slice z=0", "slice z=sz-1"};
    for (int k = 0; k < 6; ++k) {
      int rc = fill_run_rounds(c, sl[k], names[k], nullptr);
      if (rc) return rc;
    }
  }
  const FillGeom full = {(uint32_t)sx, (uint32_t)sy, (uint32_t)sz,
                         1, usx, sxy, 0, (uint32_t)nvox};
  int rc = fill_run_rounds(c, full, "the volume", rounds_out);
  if (rc) return rc;

  // ids back to values through label_values (u64 only: u32 ids ARE labels)
  const uint64_t *values =
      dtype == MG_U64 ? c->label_values.get() : nullptr;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_fill_finish<T>, vnb, blk, 0, s, c->labels.as<T>(),
                       c->holes.as<T>(), vol, values, nvox);
  });
  HIP_TRY(c, hipGetLastError(), 54);
  return 0;
}
