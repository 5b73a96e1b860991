// meshgine.hip — MI355X (gfx950/CDNA4) per-chunk meshing engine.
//
// Implements the C ABI of include/meshgine.h: the compute the reference
// delegates to zmesh's CPU C++ (multi-label marching cubes at
// /root/reference/igneous/tasks/mesh/mesh.py:245, per-label welded extract
// + quadric simplify at mesh.py:374-381) as hand-written HIP kernels.
//
// Canonical contract (bit-exact with oracle/mc_oracle.c — see DESIGN.md):
//   cells in global F-order; per cell distinct non-zero labels in
//   first-seen corner order; triangles from mc_table.h in table order;
//   per-label first-seen vertex welding; vertex position
//   (0.5f*k + shift)*res in f32.
//
// Device pipeline (one mg_mesh_chunk call):
//   H2D labels
//   [0] (optional) k_dust_*: zero labels below dust_threshold;
//       (optional, mg_mesh_chunk_mapped) k_map_build + k_label_map:
//       remap_table / object_ids / exclude_object_ids as one table lookup
//       per voxel, in place;
//       (optional, mg_mesh_chunk_filled) fill_holes.hip: hole filling by
//       union-find rounds, hole volume kept resident for mg_mesh_holes
//   [1] k_count        wave-per-64-cell-segment item and triangle counts
//                      (item = one (cell, label) pair): one
//                      classification per cell, one trip per label
//                      (+ label hash build)                    -> segcnt
//   [2] scan           rocPRIM exclusive scan (u64, both counts)
//                                                      -> segoff, NI, T
//   [3] k_emit         classify again, wave prefix, write one 8-B
//                      record + 4-B label id per ITEM in canonical
//                      global order
//   [4] partition      rocPRIM stable radix-sort of the items by label
//                      id; one u64 scan of the sorted items' vertex and
//                      triangle counts -> itscan (every item's first
//                      vertex id and first triangle); per-label triangle,
//                      item and vertex ranges
//   [5] weld           expand items into triangles (t ascending within
//                      an item: the per-triangle stream, label by label
//                      in emit order); first corners take their ids from
//                      itscan and write the vertices, later corners look
//                      their slot up: one workgroup per label with the
//                      (slot -> id) table in LDS, a direct-addressed
//                      global table for labels above WELD_LDS_CAP vertices
//   [6] (optional) per-label quadric simplification (one workgroup per
//                      label; global matched-pair rounds for huge labels)
//   [7] D2H slices + meshset assembly (ctx-owned pinned staging)
//   [7b] (mg_mesh_chunk_encoded, instead of [7]) encode.hip: shift, boxes
//       and the precomputed / draco fragment bytes of every label, then
//       D2H of the blob and the per-label tables
//
// Determinism: every kernel's output is a pure function of its inputs —
// atomics are only used for hash slot claims (value-keyed; the place of an
// entry in a table never reaches the output), the weld's block list (its
// order is free) and the label counter (affects internal ids only;
// triangle partition order is by internal id but per-label content and the
// final label-sorted meshset are invariant).

#include "mg_ctx.h"  // the context, its buffers and the shared host helpers

#include <algorithm>
#include <atomic>
#include <type_traits>
#include <vector>

#define MC_TABLE_QUAL __device__ static const
#include "mc_table.h"

// ---------------------------------------------------------------------------
// small utilities

#define WAVE 64

static inline uint64_t next_pow2_u64(uint64_t x) {
  if (x < 2) return 2;
  return 1ull << (64 - __builtin_clzll(x - 1));
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// wave-wide inclusive prefix sum (64 lanes)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, int lane) {
  for (int d = 1; d < WAVE; d <<= 1) {
    uint32_t y = __shfl_up(x, d, WAVE);
    if (lane >= d) x += y;
  }
  return x;
}

// ---------------------------------------------------------------------------
// label hash: raw label value -> dense internal id (build in count pass)

struct LabelHash {
  uint64_t *keys;   // 0 = empty (label 0 never inserted)
  uint32_t *vals;
  uint32_t *counter;   // next id
  uint32_t *overflow;  // error flag
  uint64_t nslots;     // power of two
};

__device__ __forceinline__ void label_insert(LabelHash h, uint64_t label) {
  uint64_t slot = mix64(label) & (h.nslots - 1);
  for (uint64_t probe = 0; probe < h.nslots; ++probe) {
    uint64_t cur = h.keys[slot];
    if (cur == label) return;
    if (cur == 0) {
      uint64_t prev = atomicCAS((unsigned long long *)&h.keys[slot], 0ull,
                                (unsigned long long)label);
      if (prev == 0) {
        h.vals[slot] = atomicAdd(h.counter, 1u);
        return;
      }
      if (prev == label) return;
    }
    slot = (slot + 1) & (h.nslots - 1);
  }
  atomicExch(h.overflow, 1u);
}

__device__ __forceinline__ uint32_t label_lookup(LabelHash h, uint64_t label) {
  uint64_t slot = mix64(label) & (h.nslots - 1);
  for (uint64_t probe = 0; probe < h.nslots; ++probe) {
    // ids were published by k_count, which completed before any lookup
    if (h.keys[slot] == label) return h.vals[slot];
    slot = (slot + 1) & (h.nslots - 1);
  }
  atomicExch(h.overflow, 1u);  // bug surfaces as error, not a GPU hang
  return 0;
}

// ---------------------------------------------------------------------------
// device dust removal (MeshTask dust_threshold, reference mesh.py:313-323
// via fastremap.unique + mask): three volume passes — build the label
// hash, histogram voxels per label, zero voxels of labels below the
// threshold. Replaces a multi-second host numpy unique/mask at 512^3.

template <typename T>
__global__ void k_dust_build(const T *__restrict__ labels, uint64_t nvox,
                             LabelHash lh) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < nvox; i += (uint64_t)gridDim.x * blockDim.x) {
    T L = labels[i];
    if (L != 0) label_insert(lh, (uint64_t)L);
  }
}

template <typename T>
__global__ void k_dust_count(const T *__restrict__ labels, uint64_t nvox,
                             LabelHash lh, uint32_t *__restrict__ counts) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < nvox; i += (uint64_t)gridDim.x * blockDim.x) {
    T L = labels[i];
    if (L != 0) atomicAdd(&counts[label_lookup(lh, (uint64_t)L)], 1u);
  }
}

template <typename T>
__global__ void k_dust_zero(T *__restrict__ labels, uint64_t nvox,
                            LabelHash lh,
                            const uint32_t *__restrict__ counts,
                            uint64_t thr) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < nvox; i += (uint64_t)gridDim.x * blockDim.x) {
    T L = labels[i];
    if (L != 0 && (uint64_t)counts[label_lookup(lh, (uint64_t)L)] < thr)
      labels[i] = 0;
  }
}

// ---------------------------------------------------------------------------
// device label map (MeshTask remap_table / object_ids / exclude_object_ids,
// reference mesh.py:200-204 and 357-369 via fastremap.mask_except / remap /
// mask): the three options fold on the host into ONE {key -> val} table
// plus a miss policy (igneous_amd/remap.py fold_label_ops); one volume pass
// rewrites the resident labels in place after dust and before the count
// pass. Each voxel is looked up once with its raw label (no chaining).

struct MapTable {
  ulonglong2 *slots;  // .x = key (0 = empty), .y = val
  uint64_t nslots;    // power of two, >= 2n
};

// flag bits written by k_map_build
#define MAP_ERR_DUPLICATE 1u
#define MAP_ERR_FULL      2u

__global__ void k_map_build(const uint64_t *__restrict__ keys,
                            const uint64_t *__restrict__ vals, uint64_t n,
                            MapTable t, uint32_t *__restrict__ err) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  uint64_t slot = mix64(key) & (t.nslots - 1);
  for (uint64_t probe = 0; probe < t.nslots; ++probe) {
    uint64_t prev = atomicCAS((unsigned long long *)&t.slots[slot].x, 0ull,
                              (unsigned long long)key);
    if (prev == 0) {  // claimed: this thread alone writes the value
      t.slots[slot].y = vals[i];
      return;
    }
    if (prev == key) {  // another entry holds the same key
      atomicOr(err, MAP_ERR_DUPLICATE);
      return;
    }
    slot = (slot + 1) & (t.nslots - 1);
  }
  atomicOr(err, MAP_ERR_FULL);
}

// One lookup. cl/cr are the lane's one-entry cache of its last
// (label, result): runs along x share a label. cl starts at 0, which is
// never looked up.
template <typename T>
__device__ __forceinline__ T map_one(T L, const MapTable &t, bool miss_zero,
                                     T &cl, T &cr) {
  if (L == 0) return 0;
  if (L == cl) return cr;
  T r = miss_zero ? (T)0 : L;
  uint64_t slot = mix64((uint64_t)L) & (t.nslots - 1);
  for (uint64_t probe = 0; probe < t.nslots; ++probe) {
    ulonglong2 e = t.slots[slot];
    if (e.x == (uint64_t)L) { r = (T)e.y; break; }
    if (e.x == 0) break;
    slot = (slot + 1) & (t.nslots - 1);
  }
  cl = L;
  cr = r;
  return r;
}

template <typename T> struct MapVec;
template <> struct MapVec<uint64_t> { typedef ulonglong2 type; };
template <> struct MapVec<uint32_t> { typedef uint4 type; };

template <typename T>
__device__ __forceinline__ void map_volume(T *__restrict__ labels,
                                           uint64_t nvox, const MapTable &t,
                                           uint32_t miss_zero) {
  typedef typename MapVec<T>::type V;
  constexpr int NV = 16 / sizeof(T);
  const uint64_t nvec = nvox / NV;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
  const bool mz = miss_zero != 0;
  T cl = 0, cr = 0;
  V *vp = reinterpret_cast<V *>(labels);  // hipMalloc base: 16-B aligned
  for (uint64_t i = tid; i < nvec; i += nthr) {
    union { V v; T e[NV]; } in, o;
    in.v = vp[i];
    bool changed = false;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      o.e[k] = map_one<T>(in.e[k], t, mz, cl, cr);
      changed |= (o.e[k] != in.e[k]);
    }
    if (changed) vp[i] = o.v;
  }
  // scalar tail: nvox not a multiple of the vector width
  const uint64_t i = nvec * NV + tid;
  if (i < nvox) {
    T L = labels[i];
    T r = map_one<T>(L, t, mz, cl, cr);
    if (r != L) labels[i] = r;
  }
}

// table probed in HBM/L2: any size up to the cap
template <typename T>
__global__ void k_label_map(T *__restrict__ labels, uint64_t nvox,
                            MapTable t, uint32_t miss_zero) {
  map_volume<T>(labels, nvox, t, miss_zero);
}

// small tables (n <= MAP_LDS_MAX_ENTRIES, at most 4096 slots = 64 KB):
// every workgroup stages the built table in LDS once and probes it there.
// Under MISS_ZERO most labels MISS, and a miss walks to an empty slot
// (~2.5 probes at load 0.5) — divergent 16-B requests that cost more than
// the volume stream when they go to L2. 1024 threads x 64 KB keeps two
// workgroups (32 waves) per CU.
#define MAP_LDS_MAX_ENTRIES 2048u
#define MAP_LDS_BLOCK 1024

template <typename T>
__global__ __launch_bounds__(MAP_LDS_BLOCK) void k_label_map_lds(
    T *__restrict__ labels, uint64_t nvox, MapTable g, uint32_t miss_zero) {
  extern __shared__ ulonglong2 s_map_tab[];
  for (uint32_t i = threadIdx.x; i < (uint32_t)g.nslots; i += blockDim.x)
    s_map_tab[i] = g.slots[i];
  __syncthreads();
  MapTable t;
  t.slots = s_map_tab;
  t.nslots = g.nslots;
  map_volume<T>(labels, nvox, t, miss_zero);
}

// invert: label id -> label value (fill after count)
__global__ void k_label_values(LabelHash h, uint64_t *values, uint64_t nslots) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nslots) return;
  uint64_t k = h.keys[i];
  if (k != 0) values[h.vals[i]] = k;
}

// ---------------------------------------------------------------------------
// per-cell triangle enumeration, shared by count and emit
//
// Segment = up to 64 consecutive cells of one x-row (aligned to 64 cells).
// One wave per segment; lane = cell index within the segment.

template <typename T>
__device__ __forceinline__ void load_corners(const T *__restrict__ labels,
                                             int64_t sx, int64_t sxy,
                                             int64_t cx, int64_t cy, int64_t cz,
                                             T c[8]) {
  const T *p = labels + cx + cy * sx + cz * sxy;
  c[0] = p[0];            c[1] = p[1];
  c[2] = p[sx];           c[3] = p[sx + 1];
  c[4] = p[sxy];          c[5] = p[sxy + 1];
  c[6] = p[sxy + sx];     c[7] = p[sxy + sx + 1];
}

// One classification per cell. The 28 pairwise corner compares are each
// done once and give
//   rows   byte i = the 8-bit mask of corners equal to c[i], which is the
//          MC case mask of the label at corner i
//   first  bit i set when c[i] != 0 and no lower corner equals it: the
//          cell's distinct non-zero labels, ascending i = first-seen corner
//          order. 0 for a uniform cell. In a non-uniform cell every such
//          label has triangles (only masks 0 and 255 have none,
//          tests/test_mc_table.py).
// Count and emit walk `first` lowest bit first, so a wave makes as many
// trips as its busiest lane has labels, not 8.
struct CellClass {
  uint64_t rows;
  uint32_t first;
  __device__ __forceinline__ uint32_t row(uint32_t i) const {
    return (uint32_t)(rows >> (i * 8u)) & 255u;
  }
};

template <typename T>
__device__ __forceinline__ CellClass classify_cell(const T c[8]) {
  // one byte-wide register per row while the compares run: every select
  // then takes a constant below 256 (packed rows would keep some forty
  // 32-bit literals in registers across the segment loop)
  uint32_t r[8];
  #pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = 1u << i;  // a corner equals itself
  uint32_t seen = 0;
  #pragma unroll
  for (int j = 1; j < 8; ++j) {
    #pragma unroll
    for (int i = 0; i < j; ++i) {
      const bool eq = c[i] == c[j];
      r[i] |= eq ? (1u << j) : 0u;
      r[j] |= eq ? (1u << i) : 0u;
      seen |= eq ? (1u << j) : 0u;
    }
  }
  uint32_t nz = 0;
  #pragma unroll
  for (int i = 0; i < 8; ++i) nz |= (c[i] != 0) ? (1u << i) : 0u;
  const uint32_t lo = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
  const uint32_t hi = r[4] | (r[5] << 8) | (r[6] << 16) | (r[7] << 24);
  CellClass k;
  k.rows = ((uint64_t)hi << 32) | lo;
  k.first = r[0] == 255u ? 0u : (nz & ~seen);
  return k;
}

// c[i] for a per-lane i, by selects (a dynamically indexed array would
// live in scratch)
template <typename T>
__device__ __forceinline__ T pick_corner(const T c[8], uint32_t i) {
  const bool b0 = i & 1u, b1 = i & 2u, b2 = i & 4u;
  const T a0 = b0 ? c[1] : c[0], a1 = b0 ? c[3] : c[2];
  const T a2 = b0 ? c[5] : c[4], a3 = b0 ? c[7] : c[6];
  const T d0 = b1 ? a1 : a0, d1 = b1 ? a3 : a2;
  return b2 ? d1 : d0;
}

struct GridDims {
  int64_t sx, sy, sz;     // voxel dims
  int64_t ncx, ncy, ncz;  // cell dims
  int64_t nsegx;          // segments per row
  int64_t nseg;           // total segments
};

// XCD-aware segment schedule: block b runs on XCD b%8 (observed CDNA4
// dispatch), so give each XCD one CONTIGUOUS 1/8 slab of the segment
// range — adjacent rows (which share a voxel row) then stream through
// the SAME XCD's L2 instead of being split round-robin across all 8
// (measured 2.1x row re-read from HBM with the naive linear stride).
struct SegSched {
  int64_t beg, end, step;
};

__device__ __forceinline__ SegSched xcd_seg_sched(int64_t nseg,
                                                  int waves_per_blk,
                                                  int wave_in_blk) {
  const int64_t xcd = blockIdx.x & 7;
  const int64_t j = blockIdx.x >> 3;
  const int64_t nbx = (gridDim.x + 7) >> 3;  // blocks per XCD class
  const int64_t slab = (nseg + 7) >> 3;
  SegSched ss;
  ss.beg = xcd * slab + j * waves_per_blk + wave_in_blk;
  ss.end = std::min<int64_t>((xcd + 1) * slab, nseg);
  ss.step = nbx * waves_per_blk;
  return ss;
}

// [1] count: one wave per segment; build label hash; write the segment's
// two counts as one u64, (triangles << 32) | items. An item is one
// (cell, label) pair, so a lane has popcount(first) of them. Both totals
// stay below 2^32, so one u64 scan gives both offsets and the halves never
// carry into each other.
template <typename T>
__global__ void k_count(const T *__restrict__ labels, GridDims g,
                        uint64_t *__restrict__ segcnt, LabelHash lh) {
  __shared__ uint8_t s_cnt[256];
  for (int k = threadIdx.x; k < 256; k += blockDim.x)
    s_cnt[k] = MC_TRI_COUNT[k];
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave_in_blk = threadIdx.x / WAVE;
  const int waves_per_blk = blockDim.x / WAVE;
  const int64_t sxy = g.sx * g.sy;
  const SegSched ss = xcd_seg_sched(g.nseg, waves_per_blk, wave_in_blk);
  for (int64_t seg = ss.beg; seg < ss.end; seg += ss.step) {
    const int64_t row = seg / g.nsegx;
    const int64_t segx = seg - row * g.nsegx;
    const int64_t cy = row % g.ncy;
    const int64_t cz = row / g.ncy;
    const int64_t cx = segx * WAVE + lane;
    // a lane has at most 8 items and 8 * MC_MAX_TRIS triangles, a wave
    // 64 times that: both fit 16 bits, so one u32 reduce carries both
    uint32_t cnt = 0;
    if (cx < g.ncx) {
      T c[8];
      load_corners(labels, g.sx, sxy, cx, cy, cz, c);
      const CellClass k = classify_cell(c);
      cnt = (uint32_t)__popc(k.first);
      for (uint32_t f = k.first; f; f &= f - 1) {
        const uint32_t i = (uint32_t)__builtin_ctz(f);
        cnt += (uint32_t)s_cnt[k.row(i)] << 16;
        label_insert(lh, (uint64_t)pick_corner(c, i));
      }
    }
    // wave reduce
    uint32_t incl = wave_incl_scan(cnt, lane);
    if (lane == WAVE - 1)
      segcnt[seg] = ((uint64_t)(incl >> 16) << 32) | (incl & 0xffffu);
  }
}

// Compact 8-B triangle record: {cell_lin, mask | (t<<8) | (zero<<11)},
// t in bits 8-10, zero = {cx==0, cy==0, cz==0} in bits 11-13 (which lower
// neighbour cells do not exist; the weld's first-occurrence test needs
// it). The three weld slots (edge axis, voxel, side) and the doubled
// vertex coordinates are all recomputable from it via the case tables —
// consumers decode instead of re-reading a fat 16-B record (the record
// stream dominated the MC pipeline's HBM traffic at 16 B/tri).
//
// slot = ((cell_lin*3 + comb[e]) << 1) | side, where comb[e] folds the
// edge's voxel offset and axis; side = is the label the edge's UPPER
// endpoint, baked into MC_TRI_PACK at table-gen time. Collision-free: a
// midpoint is a vertex only for its two endpoint labels; 6*nvox < 2^32
// enforced on the host.

// stage the decode tables into LDS (s_pack: 256*MC_MAX_TRIS u16,
// s_comb: 12 u32). Call before __syncthreads().
__device__ __forceinline__ void stage_decode_tables(
    uint16_t *s_pack, uint32_t *s_comb, int64_t sx, int64_t sxy) {
  for (int k = threadIdx.x; k < 256; k += blockDim.x) {
    #pragma unroll
    for (int t = 0; t < MC_MAX_TRIS; ++t)
      s_pack[k * MC_MAX_TRIS + t] = MC_TRI_PACK[k][t];
  }
  if (threadIdx.x < 12) {
    int e = threadIdx.x;
    uint32_t eoff = (uint32_t)(MC_EDGE_DOFF[e][0] >> 1) +
                    (uint32_t)(MC_EDGE_DOFF[e][1] >> 1) * (uint32_t)sx +
                    (uint32_t)(MC_EDGE_DOFF[e][2] >> 1) * (uint32_t)sxy;
    uint32_t axis = (MC_EDGE_DOFF[e][0] & 1)
                        ? 0u
                        : ((MC_EDGE_DOFF[e][1] & 1) ? 1u : 2u);
    s_comb[e] = eoff * 3u + axis;
  }
}

// [3] emit: classify again, wave prefix of the lanes' item counts, write
// one 8-B record (t = 0) + the 4-B label id per ITEM — per (cell, label)
// pair — in canonical global order. All triangles of an item share the
// cell, the mask, the boundary bits and the label; they differ only in
// t = 0 .. MC_TRI_COUNT[mask]-1, which the weld puts back (k_weld_first).
// So the stream that the partition sorts carries every distinct piece of
// information once, about half as many elements as there are triangles.
//
// The order is unchanged: emit writes items in (z, y, x) cell order, and
// within a cell in first-seen corner order; the stable sort by label id
// keeps each label's items in cell order (a label has at most one item
// per cell); expanding each item with t ascending gives, label by label,
// cells in (z, y, x) order and t ascending within the cell — exactly the
// stream a stable sort of per-triangle records gave.
// 8 waves/SIMD (no scratch): the kernel waits on memory.
template <typename T>
__global__ __launch_bounds__(256, 8) void k_emit(
    const T *__restrict__ labels, GridDims g,
    const uint64_t *__restrict__ segoff, LabelHash lh,
    uint32_t *__restrict__ item_label, uint2 *__restrict__ item_recs) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave_in_blk = threadIdx.x / WAVE;
  const int waves_per_blk = blockDim.x / WAVE;
  const int64_t sxy = g.sx * g.sy;
  const SegSched ss = xcd_seg_sched(g.nseg, waves_per_blk, wave_in_blk);
  for (int64_t seg = ss.beg; seg < ss.end; seg += ss.step) {
    const int64_t row = seg / g.nsegx;
    const int64_t segx = seg - row * g.nsegx;
    const int64_t cy = row % g.ncy;
    const int64_t cz = row / g.ncy;
    const int64_t cx = segx * WAVE + lane;
    T c[8];
    CellClass k;
    k.rows = 0;
    k.first = 0;
    if (cx < g.ncx) {
      load_corners(labels, g.sx, sxy, cx, cy, cz, c);
      k = classify_cell(c);
    }
    const uint32_t cnt = (uint32_t)__popc(k.first);  // the lane's items
    uint32_t incl = wave_incl_scan(cnt, lane);
    // low half of the scanned u64 = the segment's item offset
    uint32_t pos = (uint32_t)segoff[seg] + incl - cnt;
    const uint32_t cell_lin = (uint32_t)((cz * g.sy + cy) * g.sx + cx);
    const uint32_t zero = (uint32_t)(cx == 0) | ((uint32_t)(cy == 0) << 1) |
                          ((uint32_t)(cz == 0) << 2);
    for (uint32_t f = k.first; f; f &= f - 1) {
      const uint32_t i = (uint32_t)__builtin_ctz(f);
      const uint32_t lid = label_lookup(lh, (uint64_t)pick_corner(c, i));
      item_label[pos] = lid;
      item_recs[pos] = make_uint2(cell_lin, k.row(i) | (zero << 11));
      ++pos;
    }
  }
}

// [4b] the two counts of one item as one u64, (vertices << 32) | triangles,
// the input of the item scan (the k_count / segcnt pattern: both totals stay
// below 2^32, so the halves never carry into each other). The vertices of an
// item are its first-occurrence corners (MC_ITEM_FIRST, see "welding"
// below). Read through the sorted records themselves, or through the sort's
// permutation.
__device__ __forceinline__ uint32_t item_first_bits(uint2 rec) {
  // interior = the axes on which the cell's coordinate is above 0
  return MC_ITEM_FIRST[rec.y & 255u][~(rec.y >> 11) & 7u];
}
struct ItemCounts {
  __device__ uint64_t operator()(uint2 rec) const {
    return ((uint64_t)__popc(item_first_bits(rec)) << 32) |
           MC_TRI_COUNT[rec.y & 255u];
  }
};
struct ItemCountsVia {
  const uint2 *recs;
  __device__ uint64_t operator()(uint32_t o) const {
    return ItemCounts{}(recs[o]);
  }
};

// [4c] one thread per sorted ITEM i. itscan[1..nitems] is the inclusive scan
// of the items' counts, itscan[0] = 0 is stored here: the low half of
// itscan[i] is item i's first triangle of the stream, the high half its first
// global vertex id.
//  - per label (labels sorted, every id present), where the label changes:
//    tri_off[label] = the item's first triangle, lab_item[label] = the item,
//    vbase[label] = the item's first vertex. Entry nlabels of each holds the
//    total.
//  - blk_item[b] = the item that holds triangle b * WELD_BLK, the first item
//    of k_weld_first's block b. An item has at most MC_MAX_TRIS < WELD_BLK
//    triangles, so it holds at most one such triangle, and every b below
//    ceil(ntris / WELD_BLK) is held by some item.
#define WELD_BLK 256
__global__ void k_label_ranges(const uint32_t *__restrict__ item_lab,
                               uint64_t *__restrict__ itscan,
                               uint32_t *__restrict__ tri_off,
                               uint32_t *__restrict__ lab_item,
                               uint32_t *__restrict__ vbase,
                               uint32_t *__restrict__ blk_item,
                               uint64_t nitems, uint32_t nlabels) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nitems) return;
  uint64_t sa = 0;
  if (i == 0) {
    itscan[0] = 0;
    const uint64_t tot = itscan[nitems];
    tri_off[nlabels] = (uint32_t)tot;
    vbase[nlabels] = (uint32_t)(tot >> 32);
    lab_item[nlabels] = (uint32_t)nitems;
  } else {
    sa = itscan[i];
  }
  const uint32_t a = (uint32_t)sa;
  if (i == 0 || item_lab[i] != item_lab[i - 1]) {
    const uint32_t l = item_lab[i];
    tri_off[l] = a;
    lab_item[l] = (uint32_t)i;
    vbase[l] = (uint32_t)(sa >> 32);
  }
  const uint32_t b = (uint32_t)itscan[i + 1];
  // the first block boundary at or after a
  const uint32_t m = (a + WELD_BLK - 1) / WELD_BLK;
  if (m * WELD_BLK < b) blk_item[m] = (uint32_t)i;
}

// ---------------------------------------------------------------------------
// welding
//
// A weld slot names one possible vertex: an edge midpoint is a vertex only
// for the labels of the edge's two endpoint voxels, so (edge, side) is a
// collision-free name. slot = ((linear_voxel * 3 + axis) << 1) | side, below
// 6 * nvox, which must fit in u32 (checked on the host; matches the
// reference's own 32-bit mesher task bound, igneous_cli/cli.py:1049-1052).
//
// Whether a corner is the first occurrence of its slot in its label's
// stream is a function of its record alone. The partition is stable, so
// a label's stream keeps emit order: cells in (z, y, x) order, then the
// mask's triangles t ascending, then corners v = 0..2. An edge with the
// label at exactly one endpoint crosses that label's mask in EVERY cell
// holding the edge, and every crossing edge is used by the mask's
// triangulation (pinned by tests/test_mc_table.py). So the first
// occurrence sits in the lowest cell holding the edge — on each axis b
// perpendicular to the edge, either the edge is on the cell's upper side
// or c_b == 0 (MC_EDGE_NEED against the record's boundary bits) — at the
// mask's first (t, v) using the edge (MC_TRI_FIRST). MC_ITEM_FIRST holds
// that predicate per item, bit 3t + v.
//
// Vertices are numbered in first-occurrence order of the stream. The item
// scan gives every item its first vertex id, so a first corner's id is
// itscan[item] >> 32 plus its rank among the item's first corners, and a
// label's ids start at vbase[label]. What is left for the weld is the id of
// every LATER corner: the id its slot's first corner got. That first corner
// always lies earlier in the same label's stream, so a table of (slot -> id)
// per label answers it:
//  - k_weld_label keeps the table in LDS, one workgroup per label, for
//    labels of at most WELD_LDS_CAP vertices;
//  - larger labels go through a direct-addressed table in global memory
//    (wminp, one u32 per slot): k_weld_plan lists the 256-triangle blocks of
//    the stream that hold their triangles, k_weld_first and k_weld_faces
//    run over that list alone.

struct WeldGeom {
  uint32_t usx, usxy;  // voxel strides of y and z
  float rx, ry, rz, shift;
};

// the vertex of a slot: doubled coordinates decoded from
// slot = (lin * 3 + axis) * 2 | side
__device__ __forceinline__ void write_slot_vertex(float *__restrict__ verts,
                                                  uint64_t vid, uint32_t slot,
                                                  const WeldGeom &g) {
  const uint32_t eslot = slot >> 1;
  const uint32_t axis = eslot % 3u;
  const uint32_t lin = eslot / 3u;
  const uint32_t vz = lin / g.usxy;
  const uint32_t rem = lin - vz * g.usxy;
  const uint32_t vy = rem / g.usx;
  const uint32_t vx = rem - vy * g.usx;
  const float dx = (float)(2 * vx + (axis == 0));
  const float dy = (float)(2 * vy + (axis == 1));
  const float dz = (float)(2 * vz + (axis == 2));
  verts[3 * vid + 0] = (0.5f * dx + g.shift) * g.rx;
  verts[3 * vid + 1] = (0.5f * dy + g.shift) * g.ry;
  verts[3 * vid + 2] = (0.5f * dz + g.shift) * g.rz;
}

// LDS staging of one tile of WELD_BLK consecutive triangles of the stream,
// which arrives per ITEM (k_emit): the triangles lie in at most WELD_BLK
// consecutive items, since every item has at least one triangle. Thread i
// takes item first + i: it loads the item's scan entry and record
// (load_weld_item; neither address depends on the other, so a kernel can
// have the next tile's pair in flight while it works on this one), stages
// them, and marks the item's triangles of the tile with i. Thread r then
// finds its triangle's item j = item[r]: t - off[j] is the triangle's index
// within the item.
struct WeldTile {
  uint32_t off[WELD_BLK + 1];  // first triangle of items first .. first + 256
  uint32_t voff[WELD_BLK];     // first global vertex id of the item
  uint2 rec[WELD_BLK];
  uint8_t item[WELD_BLK];
  uint32_t next;  // items that end inside the tile (k_weld_label)
};

struct WeldItem {
  uint64_t sc, sc_end;  // itscan of item first + i; of first + 256 (thread 0)
  uint2 rec;
};

// items at or past i_end count as empty
__device__ __forceinline__ WeldItem load_weld_item(
    const uint2 *__restrict__ item_recs, const uint32_t *__restrict__ order,
    const uint64_t *__restrict__ itscan, uint64_t first, uint64_t i_end) {
  const uint64_t it = first + threadIdx.x;
  WeldItem w;
  w.sc = itscan[std::min<uint64_t>(it, i_end)];
  w.sc_end = 0;
  if (threadIdx.x == 0)
    w.sc_end = itscan[std::min<uint64_t>(first + WELD_BLK, i_end)];
  w.rec = make_uint2(0, 0);
  if (it < i_end) w.rec = order ? item_recs[order[it]] : item_recs[it];
  return w;
}

// Fill `w` for triangles [t0, t1), t1 <= t0 + WELD_BLK, from the loaded
// items. Two barriers inside; the caller's next barrier must come before
// the tile is staged again. With NEXT, w.next = how many of the items end at
// or before t1: the item behind them holds triangle t1. It has one writer:
// off[] ascends, so one i has off[i] <= t1 < off[i + 1], or none has and
// thread 255 writes 256. Empty items past the range's end hold the
// range's end in both entries, which is above t1 whenever a next tile exists.
template <bool NEXT>
__device__ __forceinline__ void stage_weld_tile(WeldTile &w,
                                                const WeldItem &li,
                                                uint32_t t0, uint32_t t1) {
  w.off[threadIdx.x] = (uint32_t)li.sc;
  w.voff[threadIdx.x] = (uint32_t)(li.sc >> 32);
  w.rec[threadIdx.x] = li.rec;
  if (threadIdx.x == 0) w.off[WELD_BLK] = (uint32_t)li.sc_end;
  __syncthreads();
  const uint32_t a = w.off[threadIdx.x], b = w.off[threadIdx.x + 1];
  const uint32_t lo = std::max(a, t0), hi = std::min(b, t1);
  for (uint32_t q = lo; q < hi; ++q) w.item[q - t0] = (uint8_t)threadIdx.x;
  if (NEXT && a <= t1) {
    if (b > t1) w.next = threadIdx.x;
    else if (threadIdx.x == WELD_BLK - 1) w.next = WELD_BLK;
  }
  __syncthreads();
}

// the decoded corners of one triangle
struct TriCorners {
  uint32_t slot[3];
  uint32_t first;  // bit v: corner v is its slot's first occurrence
  uint32_t id[3];  // first corners: global vertex id
};

__device__ __forceinline__ TriCorners decode_tri(
    const WeldTile &w, const uint16_t *s_pack, const uint16_t *s_ifirst,
    const uint32_t *s_comb, uint32_t j, uint32_t t) {
  const uint2 rec = w.rec[j];
  const uint32_t tin = t - w.off[j];  // t within the item
  const uint32_t mask = rec.y & 255u;
  const uint32_t pk = s_pack[mask * MC_MAX_TRIS + tin];
  const uint32_t ib = s_ifirst[mask * 8u + (~(rec.y >> 11) & 7u)];
  const uint32_t cl3 = rec.x * 3u;
  TriCorners c;
  c.first = (ib >> (3u * tin)) & 7u;
  #pragma unroll
  for (int v = 0; v < 3; ++v) {
    const uint32_t nib = (pk >> (5 * v)) & 31u;
    c.slot[v] = ((cl3 + s_comb[nib & 15u]) << 1) | (nib >> 4);
    // rank = the item's first corners below bit 3 * tin + v
    c.id[v] = w.voff[j] + (uint32_t)__popc(ib & ((1u << (3u * tin + v)) - 1u));
  }
  return c;
}

__device__ __forceinline__ void stage_item_first(uint16_t *s_ifirst) {
  for (int k = threadIdx.x; k < 256 * 8; k += blockDim.x)
    s_ifirst[k] = MC_ITEM_FIRST[k >> 3][k & 7];
}

// Vertex caps of the LDS weld's three bands, each twice the one below; the
// table holds twice the cap (load <= 0.5). Larger labels take the global
// table.
#define WELD_LDS_CAP 8192u
#define WELD_EMPTY 0xffffffffu  // no slot: slots are below 6 * nvox < 2^32

// [5a] one workgroup per label whose vertex count nv is in (lo_cap, CAP]
// (any other block exits): the whole weld of that label. The 8192 band's
// 107 KB of LDS is one block per CU (gfx950: 160 KB per CU, all of it open
// to one workgroup). The block walks
// the label's triangles in stream order, one tile of WELD_BLK triangles at a
// time, one thread per triangle (coalesced face stores). Per tile:
//   1. stage the tile's items and decode the three slots of each triangle
//   2. a first corner has local id = its global id - vbase[label]; it
//      claims an entry of the open-addressing table with an LDS atomicCAS
//      on the key (each slot has exactly one inserter), stores the id beside
//      it, and writes its vertex
//   3. barrier
//   4. every other corner looks its slot up: its first occurrence sits
//      earlier in the stream, so in this tile or an earlier one
// The next tile's first item is the item that holds the triangle behind
// this tile, found while the tile is staged; its loads are issued before
// this tile's table work, which hides their latency.
// Probe loops are bounded by the table size; a bound reached (a bug: the
// band keeps the load at or below 0.5) raises *err and the call fails.
template <uint32_t CAP>
__global__ __launch_bounds__(WELD_BLK) void k_weld_label(
    const uint2 *__restrict__ item_recs,  // 8-B records, one per item
    const uint32_t *__restrict__ order,   // label partition permutation,
                                          // or null: records already sorted
    const uint64_t *__restrict__ itscan,  // nitems + 1 scan entries
    const uint32_t *__restrict__ lab_item,
    const uint32_t *__restrict__ tri_off,
    const uint32_t *__restrict__ vbase,
    uint32_t *__restrict__ lab_sorted,  // label id per triangle, or null
    float *__restrict__ verts, uint32_t *__restrict__ faces,
    WeldGeom g, uint32_t lo_cap, uint32_t *__restrict__ err) {
  constexpr uint32_t TAB = 2 * CAP;
  static_assert((TAB & (TAB - 1)) == 0 && CAP <= 65536, "");
  constexpr uint32_t SHIFT = 32 - __builtin_ctz(TAB);
  __shared__ uint32_t s_key[TAB];
  __shared__ uint16_t s_val[TAB];
  __shared__ uint16_t s_pack[256 * MC_MAX_TRIS];
  __shared__ uint16_t s_ifirst[256 * 8];
  __shared__ uint32_t s_comb[12];
  __shared__ WeldTile s_tile;
  const uint32_t l = blockIdx.x;
  const uint32_t vb = vbase[l];
  const uint32_t nv = vbase[l + 1] - vb;
  if (nv <= lo_cap || nv > CAP) return;
  const uint32_t t_end = tri_off[l + 1];
  const uint64_t i_end = lab_item[l + 1];
  uint64_t first = lab_item[l];
  WeldItem li = load_weld_item(item_recs, order, itscan, first, i_end);
  stage_decode_tables(s_pack, s_comb, g.usx, g.usxy);
  stage_item_first(s_ifirst);
  for (uint32_t k = threadIdx.x; k < TAB; k += WELD_BLK) s_key[k] = WELD_EMPTY;
  for (uint32_t t0 = tri_off[l]; t0 < t_end; t0 += WELD_BLK) {
    const uint32_t t1 = std::min(t0 + WELD_BLK, t_end);
    stage_weld_tile<true>(s_tile, li, t0, t1);
    // the next tile's items, in flight while this tile is welded (s_tile.next
    // is not written again before the barrier below)
    if (t1 < t_end) {
      first += s_tile.next;
      li = load_weld_item(item_recs, order, itscan, first, i_end);
    }
    const uint32_t t = t0 + threadIdx.x;
    TriCorners c;
    if (t < t1) {
      c = decode_tri(s_tile, s_pack, s_ifirst, s_comb,
                     s_tile.item[threadIdx.x], t);
      #pragma unroll
      for (int v = 0; v < 3; ++v) {
        if (!((c.first >> v) & 1u)) continue;
        uint32_t pos = (c.slot[v] * 2654435761u) >> SHIFT;
        uint32_t n = 0;
        for (; n < TAB; ++n) {
          if (atomicCAS(&s_key[pos], WELD_EMPTY, c.slot[v]) == WELD_EMPTY)
            break;
          pos = (pos + 1) & (TAB - 1);
        }
        if (n == TAB) atomicOr(err, 1u);
        else s_val[pos] = (uint16_t)(c.id[v] - vb);
        write_slot_vertex(verts, c.id[v], c.slot[v], g);
      }
    }
    __syncthreads();
    if (t < t1) {
      #pragma unroll
      for (int v = 0; v < 3; ++v) {
        uint32_t id = c.id[v] - vb;
        if (!((c.first >> v) & 1u)) {
          uint32_t pos = (c.slot[v] * 2654435761u) >> SHIFT;
          uint32_t n = 0, key;
          while ((key = s_key[pos]) != c.slot[v] && key != WELD_EMPTY &&
                 ++n < TAB)
            pos = (pos + 1) & (TAB - 1);
          id = s_val[pos];
          if (key != c.slot[v]) atomicOr(err, 2u);  // absent
        }
        faces[3ull * t + v] = id;
      }
      if (lab_sorted) lab_sorted[t] = l;
    }
  }
}

// [5b] one wave per label: a label above WELD_LDS_CAP vertices appends the
// WELD_BLK-triangle blocks of the stream that hold its triangles to
// blk_list (in no particular order) and counts itself. Its first block is
// left out when an earlier such label, which has listed it, reaches into
// it. The cost follows those labels' triangles, not the stream's.
__global__ void k_weld_plan(const uint32_t *__restrict__ tri_off,
                            const uint32_t *__restrict__ vbase,
                            uint32_t nlabels, uint32_t *__restrict__ blk_list,
                            uint32_t *__restrict__ nlist,
                            uint32_t *__restrict__ ntable) {
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint64_t l = gid / WAVE;
  if (l >= nlabels) return;
  if (vbase[l + 1] - vbase[l] <= WELD_LDS_CAP) return;
  uint32_t b0 = tri_off[l] / WELD_BLK;
  const uint32_t b1 = (tri_off[l + 1] - 1) / WELD_BLK;
  // label m - 1 ends in block b0 or later while tri_off[m] > b0 * WELD_BLK;
  // every label has a triangle, so this looks at fewer than WELD_BLK labels
  for (uint64_t m = l; m > 0 && tri_off[m] > b0 * WELD_BLK; --m)
    if (vbase[m] - vbase[m - 1] > WELD_LDS_CAP) {
      ++b0;  // listed by label m - 1 (b0 <= b1 + 1 now: n may be 0)
      break;
    }
  const uint32_t n = b1 + 1 - b0;
  uint32_t base = 0;
  if (lane == 0) {
    base = atomicAdd(nlist, n);
    atomicAdd(ntable, 1u);
  }
  base = __shfl(base, 0);
  for (uint32_t k = lane; k < n; k += WAVE) blk_list[base + k] = b0 + k;
}

// [5c] the global table, first pass: block i takes the stream's block
// blk_list[i], one thread per triangle. A triangle of a label that the LDS
// weld has done is skipped (label WELD_EMPTY in its slot quad). For the
// others: decode the three slots, write the quad (3 slots + label id), and
// for each first corner store its global vertex id into wminp[slot] with a
// plain store (one writer per slot) and write its vertex. The table is
// never cleared: every slot k_weld_faces reads was stored here, in this
// call, by the first corner of the same label.
__global__ __launch_bounds__(WELD_BLK) void k_weld_first(
    const uint2 *__restrict__ item_recs, const uint32_t *__restrict__ order,
    const uint32_t *__restrict__ item_lab,  // sorted label id per item
    const uint64_t *__restrict__ itscan,
    const uint32_t *__restrict__ blk_item,
    const uint32_t *__restrict__ blk_list,
    const uint32_t *__restrict__ vbase,
    uint4 *__restrict__ quads,  // per listed triangle
    uint32_t *__restrict__ wminp,
    uint32_t *__restrict__ lab_sorted,  // label id per triangle, or null
    float *__restrict__ verts, WeldGeom g, uint64_t nitems, uint32_t ntris) {
  __shared__ uint16_t s_pack[256 * MC_MAX_TRIS];
  __shared__ uint16_t s_ifirst[256 * 8];
  __shared__ uint32_t s_comb[12];
  __shared__ WeldTile s_tile;
  stage_decode_tables(s_pack, s_comb, g.usx, g.usxy);
  stage_item_first(s_ifirst);
  const uint32_t b = blk_list[blockIdx.x];
  const uint32_t t0 = b * WELD_BLK;  // < ntris < 2^32
  const uint32_t t1 = std::min(t0 + WELD_BLK, ntris);
  const uint64_t first = blk_item[b];
  stage_weld_tile<false>(
      s_tile, load_weld_item(item_recs, order, itscan, first, nitems), t0,
                  t1);
  const uint32_t t = t0 + threadIdx.x;
  uint4 quad = make_uint4(0, 0, 0, WELD_EMPTY);
  if (t < t1) {
    const uint32_t j = s_tile.item[threadIdx.x];
    const uint32_t l = item_lab[first + j];
    if (vbase[l + 1] - vbase[l] > WELD_LDS_CAP) {
      const TriCorners c = decode_tri(s_tile, s_pack, s_ifirst, s_comb, j, t);
      #pragma unroll
      for (int v = 0; v < 3; ++v)
        if ((c.first >> v) & 1u) {
          wminp[c.slot[v]] = c.id[v];
          write_slot_vertex(verts, c.id[v], c.slot[v], g);
        }
      quad = make_uint4(c.slot[0], c.slot[1], c.slot[2], l);
      if (lab_sorted) lab_sorted[t] = l;
    }
  }
  quads[(uint64_t)blockIdx.x * WELD_BLK + threadIdx.x] = quad;
}

// [5d] the global table, second pass over the same list: a corner's face
// index is the id its slot's first corner stored, made local to the label
__global__ void k_weld_faces(const uint4 *__restrict__ quads,
                             const uint32_t *__restrict__ blk_list,
                             const uint32_t *__restrict__ wminp,
                             const uint32_t *__restrict__ vbase,
                             uint32_t *__restrict__ faces) {
  const uint4 q = quads[(uint64_t)blockIdx.x * WELD_BLK + threadIdx.x];
  if (q.w == WELD_EMPTY) return;
  const uint64_t t = (uint64_t)blk_list[blockIdx.x] * WELD_BLK + threadIdx.x;
  const uint32_t base = vbase[q.w];
  faces[3 * t + 0] = wminp[q.x] - base;
  faces[3 * t + 1] = wminp[q.y] - base;
  faces[3 * t + 2] = wminp[q.z] - base;
}

__global__ void k_iota(uint32_t *p, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (uint32_t)i;
}

// out = exclusive_scan[n-1] + input[n-1]  (total of a scanned array)
__global__ void k_last_sum(const uint32_t *scan, const uint32_t *input,
                           uint64_t n, uint32_t *out) {
  *out = scan[n - 1] + input[n - 1];
}

__global__ void k_any_active(const uint8_t *active, uint32_t nlabels,
                             uint32_t *any) {
  uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l < nlabels && active[l]) atomicExch(any, 1u);
}

#include "simplify.hip"

// ---------------------------------------------------------------------------
// label hash, host side: lh_keys/lh_vals hold c->lh_slots slots; the id
// counter and the overflow flag are the first two words of c->scalars.

static LabelHash label_hash_view(mg_ctx *c) {
  LabelHash lh;
  lh.keys = c->lh_keys.get();
  lh.vals = c->lh_vals.get();
  lh.counter = &c->scalars->lh_counter;
  lh.overflow = &c->scalars->lh_overflow;
  lh.nslots = c->lh_slots;
  return lh;
}

// size the hash for c->lh_slots and clear it (and the scalar block)
static int label_hash_reset(mg_ctx *c, int rc) {
  if (ensure(c, c->lh_keys, c->lh_slots)) return rc;
  if (ensure(c, c->lh_vals, c->lh_slots)) return rc;
  HIP_TRY(c, hipMemsetAsync(c->lh_keys.get(), 0, c->lh_slots * 8, c->stream),
          rc);
  HIP_TRY(c, hipMemsetAsync(c->scalars.get(), 0, sizeof(CtxScalars),
                            c->stream), rc);
  return 0;
}

// the build overflowed: grow x4 for the retry, or fail at 2^27 slots.
// `where` ("", " (dust)", " (fill_holes)") names the pass in the error.
static int label_hash_grow(mg_ctx *c, const char *where, int rc) {
  if (c->lh_slots >= (1ull << 27)) {
    SET_ERR(c, "label hash overflow%s at %llu slots", where,
            (unsigned long long)c->lh_slots);
    return rc;
  }
  c->lh_slots <<= 2;
  return 0;
}

// Hash every non-zero label of the resident volume (dust and the u64
// fill path), growing until it fits. *p_n = distinct labels.
static int hash_volume_labels(mg_ctx *c, int dtype, uint64_t nvox,
                              const char *where, int rc, uint32_t *p_n) {
  hipStream_t s = c->stream;
  for (;;) {
    if (int e = label_hash_reset(c, rc)) return e;
    const LabelHash lh = label_hash_view(c);
    by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(k_dust_build<T>, dim3(4096), dim3(256), 0, s,
                         c->labels.as<const T>(), nvox, lh);
    });
    uint32_t misc[2] = {0, 0};  // lh_counter, lh_overflow
    HIP_TRY(c, hipMemcpyAsync(misc, &c->scalars->lh_counter, 8,
                              hipMemcpyDeviceToHost, s), rc);
    HIP_TRY(c, hipStreamSynchronize(s), rc);
    if (!misc[1]) {
      *p_n = misc[0];
      return 0;
    }
    if (int e = label_hash_grow(c, where, rc)) return e;
  }
}

#include "fill_holes.hip"

extern "C" {

const char *mg_version(void) { return "meshgine 0.1.0 (gfx950)"; }

int mg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

mg_ctx *mg_init(int device_id) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device_id >= n || n == 0) {
    return nullptr;
  }
  if (hipSetDevice(device_id) != hipSuccess) return nullptr;
  mg_ctx *c = new mg_ctx();
  c->device = device_id;
  c->stats.weld_lds_cap = WELD_LDS_CAP;
  bool ok =
      hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) ==
          hipSuccess &&
      hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) ==
          hipSuccess;
  for (auto &e : c->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  // cleared on the ctx's own stream, ahead of its first call: a memset on
  // the null stream would open one more hardware queue per process and
  // change how the contexts' streams share the queues
  ok = ok && ensure(c, c->scalars, 1) == 0 &&
       hipMemsetAsync(c->scalars.get(), 0, sizeof(CtxScalars), c->stream) ==
           hipSuccess;
  if (!ok) {
    delete c;  // ~mg_ctx destroys whatever was created
    return nullptr;
  }
  return c;
}

void mg_destroy(mg_ctx *c) { delete c; }

const char *mg_last_error(mg_ctx *c) {
  return c ? c->err.c_str() : g_err.c_str();
}

int mg_get_stats(mg_ctx *c, mg_stats *out) {
  if (!c || !out) return 1;
  *out = c->stats;
  return 0;
}

void mg_meshset_free(mg_meshset *ms) {
  // the flat vertex/face storage is ctx-owned (pinned, reused); the
  // meshset is just the descriptor + mesh array
  free(ms);
}

}  // extern "C"

// *out = a meshset of n meshes (the caller frees it like any other)
static int new_meshset(mg_ctx *c, uint32_t n, mg_meshset **out) {
  *out = alloc_meshset(n, 0);
  if (!*out) {
    SET_ERR(c, "mesh_chunk: out of host memory");
    return 24;
  }
  return 0;
}

static double ev_ms(mg_ctx *c, int a, int b) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, c->ev[a], c->ev[b]) != hipSuccess) return 0.0;
  return (double)ms;
}

// ---------------------------------------------------------------------------
// one chunk: the stage functions in pipeline order, then mesh_chunk_impl

// Label map table cap: above this the caller preprocesses on the host.
#define MG_MAP_MAX_ENTRIES (1ull << 24)

// Per-call values of one mesh_chunk_impl, filled in as the stages run.
struct ChunkCall {
  int sx, sy, sz, dtype;
  size_t esize;
  uint64_t nvox;
  GridDims g;
  float rx, ry, rz;
  int voxel_centered;
  uint32_t nlabels;        // run_count_emit
  uint64_t NI;             // items = (cell, label) pairs (run_count_emit)
  uint64_t T;              // triangles (run_count_emit; run_simplify)
  uint64_t V;              // vertices (run_weld; run_simplify)
  // run_partition: label id per item (the sort's key output), the 8-B
  // item records the weld reads and the permutation to read them through
  // (null when the records themselves were sorted)
  const uint32_t *item_lab;
  const uint2 *rec_src;
  const uint32_t *order_sorted;
  bool simplify;           // a simplify follows the weld
  uint32_t *lab_sorted;    // label id per triangle (run_weld writes it when
                           // a simplify follows, else null)
};

static void set_hole_stash(mg_ctx *c, const ChunkCall &k) {
  c->holes_valid = true;
  c->holes_sx = k.sx; c->holes_sy = k.sy; c->holes_sz = k.sz;
  c->holes_dtype = k.dtype;
}

// H2D (skipped when the caller staged the identical volume already, or
// mg_count_voxels left it there: MG_FLAG_COUNTED)
static int upload_labels(mg_ctx *c, const ChunkCall &k,
                         const void *labels_host, uint32_t flags) {
  const size_t bytes = k.nvox * k.esize;
  if ((flags & (MG_FLAG_SKIP_H2D | MG_FLAG_COUNTED)) && c->labels.cap >= bytes)
    return 0;
  if (ensure_bytes(c, c->labels, bytes)) return 11;
  HIP_TRY(c, hipMemcpyAsync(c->labels.ptr, labels_host, bytes,
                            hipMemcpyHostToDevice, c->stream), 11);
  return 0;
}

// device dust removal (three volume passes; see k_dust_* above)
static int run_dust(mg_ctx *c, const ChunkCall &k, uint64_t dust_threshold) {
  hipStream_t s = c->stream;
  uint32_t ndl = 0;
  if (int e = hash_volume_labels(c, k.dtype, k.nvox, " (dust)", 16, &ndl))
    return e;
  if (ndl == 0) return 0;
  const LabelHash lh = label_hash_view(c);
  if (ensure(c, c->order, ndl)) return 16;  // voxel count per label id
  HIP_TRY(c, hipMemsetAsync(c->order.get(), 0, (uint64_t)ndl * 4, s), 16);
  by_dtype(k.dtype, [&](auto t) {
    using T = decltype(t);
    const dim3 nb(4096), blk(256);
    hipLaunchKernelGGL(k_dust_count<T>, nb, blk, 0, s,
                       c->labels.as<const T>(), k.nvox, lh, c->order.get());
    hipLaunchKernelGGL(k_dust_zero<T>, nb, blk, 0, s, c->labels.as<T>(),
                       k.nvox, lh, c->order.get(), dust_threshold);
  });
  HIP_TRY(c, hipGetLastError(), 16);
  return 0;
}

// label map in place on the resident labels (after dust, which counted
// the RAW labels — the reference's order, mesh.py:193-204)
static int run_label_map(mg_ctx *c, const ChunkCall &k,
                         const mg_label_map *map) {
  hipStream_t s = c->stream;
  const uint64_t n = map->n, nvox = k.nvox;
  MapTable mt;
  mt.nslots = next_pow2_u64(std::max<uint64_t>(2 * n, 64));
  if (ensure(c, c->map_tab, mt.nslots)) return 41;
  mt.slots = c->map_tab.get();
  uint32_t *d_err = &c->scalars->map_err;
  HIP_TRY(c, hipEventRecord(c->ev[EV_MAP_START], s), 41);
  HIP_TRY(c, hipMemsetAsync(mt.slots, 0, mt.nslots * 16, s), 41);
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 4, s), 41);
  if (n > 0) {
    if (ensure(c, c->map_keys, n)) return 41;
    if (ensure(c, c->map_vals, n)) return 41;
    HIP_TRY(c, hipMemcpyAsync(c->map_keys.get(), map->keys, n * 8,
                              hipMemcpyHostToDevice, s), 41);
    HIP_TRY(c, hipMemcpyAsync(c->map_vals.get(), map->vals, n * 8,
                              hipMemcpyHostToDevice, s), 41);
    const int bblk = 256;
    hipLaunchKernelGGL(k_map_build, dim3((uint32_t)((n + bblk - 1) / bblk)),
                       dim3(bblk), 0, s, c->map_keys.get(),
                       c->map_vals.get(), n, mt, d_err);
  }
  const uint64_t nvec = nvox / (16 / k.esize);
  const uint32_t miss_zero = map->miss == MG_MAP_MISS_ZERO;
  // MG_MAP_LDS=0 reverts small tables to the L2-probed kernel (A/B)
  static const bool use_lds = []() {
    const char *e = getenv("MG_MAP_LDS");
    return !(e && e[0] == '0');
  }();
  const bool lds = use_lds && n <= MAP_LDS_MAX_ENTRIES;
  const int mblk = lds ? MAP_LDS_BLOCK : 256;
  const uint32_t mnb = (uint32_t)std::min<uint64_t>(
      std::max<uint64_t>((nvec + mblk - 1) / mblk, 1), lds ? 512 : 4096);
  by_dtype(k.dtype, [&](auto t) {
    using T = decltype(t);
    if (lds)  // LDS copy of the table: <= 4096 slots = 64 KB
      hipLaunchKernelGGL(k_label_map_lds<T>, dim3(mnb), dim3(mblk),
                         mt.nslots * 16, s, c->labels.as<T>(), nvox, mt,
                         miss_zero);
    else
      hipLaunchKernelGGL(k_label_map<T>, dim3(mnb), dim3(mblk), 0, s,
                         c->labels.as<T>(), nvox, mt, miss_zero);
  });
  HIP_TRY(c, hipGetLastError(), 41);
  HIP_TRY(c, hipEventRecord(c->ev[EV_MAP_END], s), 41);
  uint32_t map_err = 0;
  HIP_TRY(c, hipMemcpyAsync(&map_err, d_err, 4, hipMemcpyDeviceToHost, s),
          41);
  HIP_TRY(c, hipStreamSynchronize(s), 41);
  if (map_err & MAP_ERR_DUPLICATE) {
    SET_ERR(c, "label map: duplicate key among %llu entries",
            (unsigned long long)n);
    return 42;
  }
  if (map_err) {
    SET_ERR(c, "label map: table build failed (flag %u)", map_err);
    return 42;
  }
  c->stats.ms_labelmap = ev_ms(c, EV_MAP_START, EV_MAP_END);
  return 0;
}

// grid of the wave-per-segment kernels (k_count, k_emit)
static inline uint32_t seg_blocks(const GridDims &g, int blk) {
  const int waves_per_blk = blk / WAVE;
  int64_t nb = std::min<int64_t>(
      (g.nseg + waves_per_blk - 1) / waves_per_blk, 8192);
  return (uint32_t)((nb + 7) & ~7ll);  // multiple of 8: XCD slab schedule
}

// [1] count + label hash build, [2] scan. *p_overflow: the hash was too
// small and the pass must be repeated with a bigger one.
static int count_pass(mg_ctx *c, ChunkCall &k, bool *p_overflow) {
  hipStream_t s = c->stream;
  const LabelHash lh = label_hash_view(c);
  uint64_t *d_segcnt = c->segcnt.get();
  uint64_t *d_segoff = c->segoff.get();
  const int64_t nseg = k.g.nseg;
  HIP_TRY(c, hipEventRecord(c->ev[EV_H2D_END], s), 30);  // see the enum
  by_dtype(k.dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_count<T>, dim3(seg_blocks(k.g, 256)), dim3(256), 0,
                       s, c->labels.as<const T>(), k.g, d_segcnt, lh);
  });
  HIP_TRY(c, hipGetLastError(), 30);
  HIP_TRY(c, hipEventRecord(c->ev[EV_COUNT_END], s), 30);

  // check overflow + read label count
  uint32_t misc[2] = {0, 0};  // lh_counter, lh_overflow
  HIP_TRY(c, hipMemcpyAsync(misc, &c->scalars->lh_counter, 8,
                            hipMemcpyDeviceToHost, s), 30);
  // scan segcnt -> segoff
  if (int e = scan_u64(c, d_segcnt, d_segoff, (size_t)nseg, s,
                       "seg scan size query failed", "seg scan failed", 30))
    return e;
  uint64_t last_off = 0, last_cnt = 0;  // (triangles << 32) | items
  HIP_TRY(c, hipMemcpyAsync(&last_off, d_segoff + (nseg - 1), 8,
                            hipMemcpyDeviceToHost, s), 30);
  HIP_TRY(c, hipMemcpyAsync(&last_cnt, d_segcnt + (nseg - 1), 8,
                            hipMemcpyDeviceToHost, s), 30);
  HIP_TRY(c, hipEventRecord(c->ev[EV_SCAN_END], s), 30);
  HIP_TRY(c, hipStreamSynchronize(s), 30);
  *p_overflow = misc[1] != 0;
  k.nlabels = misc[0];
  // NI <= T, and T is held to the corner-index limit (run_count_emit)
  const uint64_t total = last_off + last_cnt;
  k.NI = total & 0xffffffffull;
  k.T = total >> 32;
  return 0;
}

// [1]-[3]: count (grow-and-retry on label hash overflow), scan, label
// values, emit. Leaves k.nlabels / k.T; emits nothing when either is 0.
static int run_count_emit(mg_ctx *c, ChunkCall &k) {
  hipStream_t s = c->stream;
  if (ensure(c, c->segcnt, k.g.nseg)) return 12;
  if (ensure(c, c->segoff, k.g.nseg)) return 12;
  for (;;) {
    if (int e = label_hash_reset(c, 12)) return e;
    bool overflow = false;
    if (int e = count_pass(c, k, &overflow)) return e;
    if (!overflow) break;
    if (int e = label_hash_grow(c, "", 13)) return e;
  }
  c->stats.total_tris = k.T;
  c->stats.n_labels = k.nlabels;
  if (k.T == 0 || k.nlabels == 0) return 0;
  if (k.T > (1ull << 31) / 3 * 2) {  // 3T must fit u32 stream index
    SET_ERR(c, "chunk produces %llu triangles (> corner-index limit); "
            "split the task shape", (unsigned long long)k.T);
    return 15;
  }
  if (k.nlabels >= (1u << 27)) {  // label id shares the 64-bit weld key
    SET_ERR(c, "%u labels exceed the 2^27 per-chunk label limit", k.nlabels);
    return 15;
  }
  const LabelHash lh = label_hash_view(c);
  // label id -> value
  if (ensure(c, c->label_values, k.nlabels)) return 17;
  hipLaunchKernelGGL(k_label_values,
                     dim3((uint32_t)((c->lh_slots + 255) / 256)), dim3(256),
                     0, s, lh, c->label_values.get(), c->lh_slots);
  // [3] emit, one label id + one record per item
  if (ensure(c, c->tri_label, k.NI)) return 18;
  if (ensure(c, c->tri_keys, k.NI)) return 18;
  by_dtype(k.dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_emit<T>, dim3(seg_blocks(k.g, 256)), dim3(256), 0, s,
                       c->labels.as<const T>(), k.g, c->segoff.get(), lh,
                       c->tri_label.get(), c->tri_keys.get());
  });
  HIP_TRY(c, hipGetLastError(), 18);
  HIP_TRY(c, hipEventRecord(c->ev[EV_EMIT_END], s), 18);
  return 0;
}

// [4] stable partition of the ITEMS by label id, then the item scan.
// Default (MG_SORT_RECS=0 reverts): the 8-B records ride the radix sort as
// its 64-bit VALUES, so the weld reads them back SEQUENTIALLY instead of
// paying a random 8-B gather through the permutation.
static int run_partition(mg_ctx *c, ChunkCall &k) {
  hipStream_t s = c->stream;
  const uint64_t T = k.T, NI = k.NI;
  const char *sre = getenv("MG_SORT_RECS");
  const bool sort_recs = !(sre && sre[0] == '0');
  if (ensure(c, c->tri_label_alt, NI)) return 19;
  const dim3 nb((uint32_t)((NI + 255) / 256)), blk(256);
  unsigned end_bit = 1;
  while ((1u << end_bit) < k.nlabels) ++end_bit;
  rocprim::double_buffer<uint32_t> d_keys(c->tri_label.get(),
                                          c->tri_label_alt.get());
  if (sort_recs) {
    // the 8-B item records as the sort's u64 values
    if (ensure(c, c->keys_sorted, 2 * NI)) return 19;
    rocprim::double_buffer<uint64_t> d_vals(
        reinterpret_cast<uint64_t *>(c->tri_keys.get()),
        reinterpret_cast<uint64_t *>(c->keys_sorted.get()));
    if (int e = sort_pairs(c, d_keys, d_vals, NI, 0u, end_bit, s,
                           "radix_sort size query failed",
                           "radix_sort failed", 19))
      return e;
    k.rec_src = reinterpret_cast<const uint2 *>(d_vals.current());
    k.order_sorted = nullptr;  // records already label-partitioned
  } else {
    if (ensure(c, c->order, NI)) return 19;
    if (ensure(c, c->order_alt, NI)) return 19;
    hipLaunchKernelGGL(k_iota, nb, blk, 0, s, c->order.get(), NI);
    rocprim::double_buffer<uint32_t> d_vals(c->order.get(),
                                            c->order_alt.get());
    if (int e = sort_pairs(c, d_keys, d_vals, NI, 0u, end_bit, s,
                           "radix_sort size query failed",
                           "radix_sort failed", 19))
      return e;
    k.rec_src = c->tri_keys.get();
    k.order_sorted = d_vals.current();
  }
  k.item_lab = d_keys.current();
  // itscan[1..NI] = inclusive scan of the sorted items' (vertices <<
  // 32) | triangles; k_label_ranges stores itscan[0]
  if (ensure(c, c->itscan, NI + 1)) return 19;
  uint64_t *itscan = c->itscan.get();
  if (int e = k.order_sorted
          ? scan_incl_u64(c, rocprim::make_transform_iterator(
                                 k.order_sorted, ItemCountsVia{k.rec_src}),
                          itscan + 1, NI, s, "item scan size query failed",
                          "item scan failed", 19)
          : scan_incl_u64(c, rocprim::make_transform_iterator(
                                 k.rec_src, ItemCounts{}),
                          itscan + 1, NI, s, "item scan size query failed",
                          "item scan failed", 19))
    return e;
  // per-label ranges + the first items of the stream's blocks
  const uint64_t nl1 = (uint64_t)k.nlabels + 1;
  if (ensure(c, c->tri_off, nl1)) return 19;
  if (ensure(c, c->lab_item, nl1)) return 19;
  if (ensure(c, c->vbase, nl1)) return 19;
  if (ensure(c, c->blk_item, (T + WELD_BLK - 1) / WELD_BLK)) return 19;
  hipLaunchKernelGGL(k_label_ranges, nb, blk, 0, s, k.item_lab, itscan,
                     c->tri_off.get(), c->lab_item.get(), c->vbase.get(),
                     c->blk_item.get(), NI, k.nlabels);
  HIP_TRY(c, hipGetLastError(), 19);
  HIP_TRY(c, hipEventRecord(c->ev[EV_PARTITION_END], s), 19);
  return 0;
}

static int check_weld_err(mg_ctx *c) {
  const uint32_t werr = *c->h_weld_err.get();
  if (!werr) return 0;
  SET_ERR(c, "weld: a label table probe reached its bound (flag %u)", werr);
  return 29;
}

// [5] weld: per-label LDS tables in three vertex-count bands, and the global
// direct-addressed table for the labels above WELD_LDS_CAP (see "welding")
static int run_weld(mg_ctx *c, ChunkCall &k) {
  hipStream_t s = c->stream;
  const uint64_t T = k.T, NC = 3 * T;  // corners
  const uint64_t wslots = 6 * k.nvox;  // 3 edges/voxel x 2 sides
  if (wslots >= (1ull << 32)) {
    SET_ERR(c, "chunk too large for the 32-bit weld slots (%d x %d x %d); "
            "split the task shape (the reference's own mesher bound is "
            "1023x1023x511, igneous_cli/cli.py:1049-1052)", k.sx, k.sy, k.sz);
    return 20;
  }
  const uint32_t nblocks = (uint32_t)((T + WELD_BLK - 1) / WELD_BLK);
  if (ensure(c, c->blk_list, nblocks)) return 20;
  if (ensure(c, c->h_weld_err, 1)) return 20;
  *c->h_weld_err.get() = 0;
  hipLaunchKernelGGL(k_weld_plan,
                     dim3((uint32_t)(((uint64_t)k.nlabels * WAVE + 255) / 256)),
                     dim3(256), 0, s, c->tri_off.get(), c->vbase.get(),
                     k.nlabels, c->blk_list.get(), &c->scalars->weld_nlist,
                     &c->scalars->weld_table_labels);
  // the one host sync: vertex total (the scan's last element) and the plan
  uint64_t tot = 0;
  uint32_t plan[2] = {0, 0};  // weld_nlist, weld_table_labels
  HIP_TRY(c, hipMemcpyAsync(&tot, c->itscan.get() + k.NI, 8,
                            hipMemcpyDeviceToHost, s), 21);
  HIP_TRY(c, hipMemcpyAsync(plan, &c->scalars->weld_nlist, 8,
                            hipMemcpyDeviceToHost, s), 21);
  HIP_TRY(c, hipStreamSynchronize(s), 21);
  k.V = tot >> 32;
  const uint64_t nlist = plan[0];
  c->stats.total_verts = k.V;
  c->stats.weld_table_labels = plan[1];
  c->stats.weld_lds_labels = k.nlabels - plan[1];

  if (ensure(c, c->verts, 3 * k.V)) return 22;
  if (ensure(c, c->faces, NC)) return 22;
  k.lab_sorted = nullptr;
  if (k.simplify) {
    if (ensure(c, c->lab_sorted, T)) return 22;
    // simp_finalize's scratch: newid[vbase[l]] is read for every l <= nlabels
    if (ensure(c, c->vtx_scan, k.V + 1)) return 22;
    k.lab_sorted = c->lab_sorted.get();
  }
  const WeldGeom wg = {(uint32_t)k.g.sx, (uint32_t)(k.g.sx * k.g.sy),
                       k.rx, k.ry, k.rz, k.voxel_centered ? 0.0f : 0.5f};
  uint32_t *d_err = &c->scalars->weld_err;
  if (plan[1] < k.nlabels) {
    // bands (lo_cap, CAP] of 1, 2 and 4 blocks per CU, the fewest first
    auto launch_band = [&](auto capc, uint32_t lo_cap) {
      hipLaunchKernelGGL(k_weld_label<decltype(capc)::value>, dim3(k.nlabels),
                         dim3(WELD_BLK), 0, s, k.rec_src, k.order_sorted,
                         c->itscan.get(), c->lab_item.get(), c->tri_off.get(),
                         c->vbase.get(), k.lab_sorted, c->verts.get(),
                         c->faces.get(), wg, lo_cap, d_err);
    };
    launch_band(std::integral_constant<uint32_t, WELD_LDS_CAP>{},
                WELD_LDS_CAP / 2);
    launch_band(std::integral_constant<uint32_t, WELD_LDS_CAP / 2>{},
                WELD_LDS_CAP / 4);
    launch_band(std::integral_constant<uint32_t, WELD_LDS_CAP / 4>{}, 0u);
  }
  if (nlist > 0) {
    // only now: the table is 24 B per voxel
    if (ensure(c, c->wh_keys, wslots)) return 22;
    if (ensure(c, c->weld_quads, nlist * WELD_BLK)) return 22;
    hipLaunchKernelGGL(k_weld_first, dim3((uint32_t)nlist), dim3(WELD_BLK), 0,
                       s, k.rec_src, k.order_sorted, k.item_lab,
                       c->itscan.get(), c->blk_item.get(), c->blk_list.get(),
                       c->vbase.get(), c->weld_quads.get(), c->wh_keys.get(),
                       k.lab_sorted, c->verts.get(), wg, k.NI, (uint32_t)T);
    hipLaunchKernelGGL(k_weld_faces, dim3((uint32_t)nlist), dim3(WELD_BLK), 0,
                       s, c->weld_quads.get(), c->blk_list.get(),
                       c->wh_keys.get(), c->vbase.get(), c->faces.get());
  }
  HIP_TRY(c, hipGetLastError(), 22);
  HIP_TRY(c, hipMemcpyAsync(c->h_weld_err.get(), d_err, 4,
                            hipMemcpyDeviceToHost, s), 22);
  HIP_TRY(c, hipEventRecord(c->ev[EV_WELD_END], s), 22);
  // The simplifier indexes vertices by the face ids, so the probe-bound flag
  // is checked before it runs; every other call copies the faces without
  // following them and checks behind its last sync (mesh_chunk_impl).
  if (k.simplify) {
    HIP_TRY(c, hipStreamSynchronize(s), 22);
    if (int e = check_weld_err(c)) return e;
  }
  return 0;
}

// [7] D2H of the flat vertex/face arrays into the ctx's pinned staging
// and the per-label descriptor, meshes by ascending label value. Under
// MG_FLAG_DEVICE_ONLY nothing is copied and the meshset is empty.
static int extract_meshset(mg_ctx *c, const ChunkCall &k, uint32_t flags,
                           mg_meshset **out) {
  hipStream_t s = c->stream;
  if (flags & MG_FLAG_DEVICE_ONLY) {
    HIP_TRY(c, hipStreamSynchronize(s), 23);
    return new_meshset(c, 0, out);
  }
  const uint32_t nlabels = k.nlabels;
  const uint64_t V = k.V, NC = 3 * k.T;
  if (ensure(c, c->h_verts, 3 * V + 3)) return 24;
  if (ensure(c, c->h_faces, NC + 1)) return 24;
  float *h_verts = c->h_verts.get();
  uint32_t *h_faces = c->h_faces.get();
  std::vector<uint32_t> h_tri_off(nlabels + 1), h_vbase(nlabels + 1);
  std::vector<uint64_t> h_label_values(nlabels);
  if (V > 0)
    HIP_TRY(c, hipMemcpyAsync(h_verts, c->verts.get(), V * 12,
                              hipMemcpyDeviceToHost, s), 24);
  if (NC > 0)
    HIP_TRY(c, hipMemcpyAsync(h_faces, c->faces.get(), NC * 4,
                              hipMemcpyDeviceToHost, s), 24);
  HIP_TRY(c, hipMemcpyAsync(h_tri_off.data(), c->tri_off.get(),
                            (nlabels + 1) * 4, hipMemcpyDeviceToHost, s), 24);
  HIP_TRY(c, hipMemcpyAsync(h_vbase.data(), c->vbase.get(), (nlabels + 1) * 4,
                            hipMemcpyDeviceToHost, s), 24);
  HIP_TRY(c, hipMemcpyAsync(h_label_values.data(), c->label_values.get(),
                            nlabels * 8, hipMemcpyDeviceToHost, s), 24);
  HIP_TRY(c, hipStreamSynchronize(s), 24);

  mg_meshset *ms = nullptr;
  if (int e = new_meshset(c, nlabels, &ms)) return e;
  ms->verts_base = h_verts;
  ms->faces_base = h_faces;
  ms->total_verts = V;
  ms->total_tris = k.T;
  // order meshes by ascending label value
  std::vector<uint32_t> idx(nlabels);
  for (uint32_t i = 0; i < nlabels; ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
    return h_label_values[a] < h_label_values[b];
  });
  for (uint32_t m = 0; m < nlabels; ++m) {
    uint32_t l = idx[m];
    set_mesh(ms, m, h_label_values[l], h_vbase[l], h_vbase[l + 1] - h_vbase[l],
             h_tri_off[l], h_tri_off[l + 1] - h_tri_off[l]);
  }
  *out = ms;
  return 0;
}

#include "encode.hip"

// One chunk call as its caller gave it, in the order of the C signatures; the
// four mg_mesh_chunk* entry points and mg_mesh_holes each fill one. Exactly
// one destination is set, and which one says how the call ends: `out` in
// extract_meshset, `bout` (an encoded call, with `ep`) in run_encode.
struct ChunkRequest {
  const void *labels;  // host volume; not read under MG_FLAG_SKIP_H2D /
                       // MG_FLAG_COUNTED
  int sx, sy, sz, dtype;
  float rx, ry, rz;
  uint32_t reduction_factor;
  float max_error;
  int voxel_centered;
  uint64_t dust_threshold;
  uint32_t flags;
  const mg_label_map *map;     // null: no label map
  uint32_t fill_level;
  const mg_encode_params *ep;  // null for a meshset call
  mg_meshset **out;
  mg_blobset **bout;
  EncParams enc;  // ep as check_encode_params accepted it (mesh_chunk_checked)
};

static int empty_result(mg_ctx *c, const ChunkRequest &r) {
  return r.bout ? new_blobset(c, 0, r.bout) : new_meshset(c, 0, r.out);
}

// The one writer of c->stats' stage times (ms_labelmap aside: run_label_map
// syncs for it), once the call's stream is synchronised. meshed = false: no
// triangles, so the events past the count pass are an earlier call's and
// their fields stay 0.
static void write_stage_times(mg_ctx *c, const ChunkRequest &r, bool meshed) {
  mg_stats &st = c->stats;
  st.ms_h2d = ev_ms(c, EV_START, EV_H2D_END);
  if (r.fill_level) st.ms_fill = ev_ms(c, EV_FILL_START, EV_FILL_END);
  if (!meshed) return;
  st.ms_count = ev_ms(c, EV_H2D_END, EV_COUNT_END);
  st.ms_scan = ev_ms(c, EV_COUNT_END, EV_SCAN_END);
  st.ms_emit = ev_ms(c, EV_SCAN_END, EV_EMIT_END);
  st.ms_partition = ev_ms(c, EV_EMIT_END, EV_PARTITION_END);
  st.ms_weld = ev_ms(c, EV_PARTITION_END, EV_WELD_END);
  st.ms_simplify = ev_ms(c, EV_WELD_END, EV_SIMPLIFY_END);
  st.ms_d2h = ev_ms(c, r.bout ? EV_ENCODE_END : EV_SIMPLIFY_END, EV_END);
  if (r.bout) st.ms_encode = ev_ms(c, EV_SIMPLIFY_END, EV_ENCODE_END);
  st.ms_total = ev_ms(c, EV_START, EV_END);
}

static int mesh_chunk_impl(mg_ctx *c, const ChunkRequest &r) {
  ChunkCall k = {};
  k.sx = r.sx; k.sy = r.sy; k.sz = r.sz; k.dtype = r.dtype;
  k.esize = (r.dtype == MG_U64) ? 8 : 4;
  k.nvox = (uint64_t)r.sx * r.sy * r.sz;
  k.rx = r.rx; k.ry = r.ry; k.rz = r.rz;
  k.voxel_centered = r.voxel_centered;
  GridDims &g = k.g;
  g.sx = r.sx; g.sy = r.sy; g.sz = r.sz;
  g.ncx = r.sx > 1 ? r.sx - 1 : 0;
  g.ncy = r.sy > 1 ? r.sy - 1 : 0;
  g.ncz = r.sz > 1 ? r.sz - 1 : 0;
  g.nsegx = (g.ncx + WAVE - 1) / WAVE;
  g.nseg = g.nsegx * g.ncy * g.ncz;

  memset(&c->stats, 0, sizeof(c->stats));
  c->stats.weld_lds_cap = WELD_LDS_CAP;
  c->stats.bytes_read_algorithmic = k.nvox * k.esize;
  hipStream_t s = c->stream;

  // trivial empty-cell-grid case: nothing is queued, no stage time
  if (g.nseg == 0) {
    if (int e = empty_result(c, r)) return e;
    if (r.fill_level) set_hole_stash(c, k);  // nothing to mesh there either
    return 0;
  }

  HIP_TRY(c, hipEventRecord(c->ev[EV_START], s), 10);
  if (int e = upload_labels(c, k, r.labels, r.flags)) return e;
  HIP_TRY(c, hipEventRecord(c->ev[EV_H2D_END], s), 11);
  if (r.dust_threshold > 0)
    if (int e = run_dust(c, k, r.dust_threshold)) return e;
  if (r.map)
    if (int e = run_label_map(c, k, r.map)) return e;
  // fill_holes on the dusted + mapped labels (mesh.py:211-228): the
  // resident volume becomes the filled one, the hole volume stays in
  // c->holes for mg_mesh_holes
  if (r.fill_level) {
    HIP_TRY(c, hipEventRecord(c->ev[EV_FILL_START], s), 56);
    if (int e = run_fill_holes(c, r.dtype, r.sx, r.sy, r.sz, r.fill_level,
                               nullptr))
      return e;
    HIP_TRY(c, hipEventRecord(c->ev[EV_FILL_END], s), 56);
    set_hole_stash(c, k);
  }

  if (int e = run_count_emit(c, k)) return e;
  if (k.T == 0 || k.nlabels == 0) {
    if (int e = empty_result(c, r)) return e;
    HIP_TRY(c, hipStreamSynchronize(s), 14);
    write_stage_times(c, r, false);
    return 0;
  }
  k.simplify = r.reduction_factor > 1;
  if (int e = run_partition(c, k)) return e;
  if (int e = run_weld(c, k)) return e;
  // [6] per-label quadric simplification (mesh.py:376-381 semantics)
  if (k.simplify)
    if (int e = run_simplify(c, k.nlabels, k.lab_sorted, r.reduction_factor,
                             r.max_error, &k.T, &k.V))
      return e;
  HIP_TRY(c, hipEventRecord(c->ev[EV_SIMPLIFY_END], s), 22);
  if (int e = r.bout ? run_encode(c, k, r.flags, r.enc, r.bout)
                     : extract_meshset(c, k, r.flags, r.out))
    return e;
  HIP_TRY(c, hipEventRecord(c->ev[EV_END], s), 25);
  HIP_TRY(c, hipStreamSynchronize(s), 25);
  if (int e = check_weld_err(c)) {
    if (r.bout) { mg_blobset_free(*r.bout); *r.bout = nullptr; }
    else { mg_meshset_free(*r.out); *r.out = nullptr; }
    return e;
  }
  write_stage_times(c, r, true);
  return 0;
}

// ---------------------------------------------------------------------------
// C ABI entry points

// dims / dtype checks shared by the calls that take a label volume
static int check_volume_args(mg_ctx *c, int sx, int sy, int sz, int dtype) {
  if (sx < 1 || sy < 1 || sz < 1 || sx > 2047 || sy > 2047 || sz > 2047) {
    SET_ERR(c, "dims out of range (1..2047): %d %d %d", sx, sy, sz);
    return 2;
  }
  if (dtype != MG_U32 && dtype != MG_U64) {
    SET_ERR(c, "bad dtype %d", dtype);
    return 3;
  }
  return 0;
}

static int check_label_map(mg_ctx *c, const mg_label_map *map, int dtype,
                           uint32_t flags) {
  if (map->miss != MG_MAP_MISS_KEEP && map->miss != MG_MAP_MISS_ZERO) {
    SET_ERR(c, "label map: bad miss policy %u", map->miss);
    return 5;
  }
  if (flags & MG_FLAG_SKIP_H2D) {
    SET_ERR(c, "label map cannot be combined with MG_FLAG_SKIP_H2D "
            "(the resident volume is already mapped)");
    return 5;
  }
  if (map->n > MG_MAP_MAX_ENTRIES) {
    SET_ERR(c, "label map: %llu entries exceed the %llu-entry cap",
            (unsigned long long)map->n,
            (unsigned long long)MG_MAP_MAX_ENTRIES);
    return 5;
  }
  if (map->n > 0 && (!map->keys || !map->vals)) {
    SET_ERR(c, "label map: null keys/vals with n=%llu",
            (unsigned long long)map->n);
    return 5;
  }
  for (uint64_t i = 0; i < map->n; ++i) {
    if (map->keys[i] == 0) {
      SET_ERR(c, "label map: key 0 at entry %llu (label 0 is never "
              "looked up)", (unsigned long long)i);
      return 5;
    }
    if (dtype == MG_U32 && map->vals[i] > 0xFFFFFFFFull) {
      SET_ERR(c, "label map: value %llu at entry %llu does not fit "
              "MG_U32", (unsigned long long)map->vals[i],
              (unsigned long long)i);
      return 5;
    }
  }
  return 0;
}

#include "chunk_mesh.hip"
#include "merge_verts.hip"
#include "octree_level.hip"
#include "count_voxels.hip"

// MG_FLAG_COUNTED: the resident volume must be the one the mg_count_voxels
// call just before left there (`counted`: the stash as this call found it).
static int check_counted(mg_ctx *c, const ChunkRequest &r, bool counted) {
  if (r.flags & MG_FLAG_SKIP_H2D) {
    SET_ERR(c, "MG_FLAG_COUNTED cannot be combined with MG_FLAG_SKIP_H2D");
    return 9;
  }
  if (!counted) {
    SET_ERR(c, "MG_FLAG_COUNTED: no counted volume on this ctx (it is left "
            "by mg_count_voxels for the call right after it)");
    return 9;
  }
  if (r.sx != c->counted_sx || r.sy != c->counted_sy ||
      r.sz != c->counted_sz || r.dtype != c->counted_dtype) {
    SET_ERR(c, "MG_FLAG_COUNTED: the counted volume is %d x %d x %d dtype %d, "
            "the call asks for %d x %d x %d dtype %d", c->counted_sx,
            c->counted_sy, c->counted_sz, c->counted_dtype, r.sx, r.sy, r.sz,
            r.dtype);
    return 9;
  }
  return 0;
}

// The argument checks of the four mg_mesh_chunk* calls, in the order their
// return codes document (the earlier check wins), then mesh_chunk_impl.
static int mesh_chunk_checked(mg_ctx *c, ChunkRequest r) {
  if (!c) { SET_ERR(c, "null ctx"); return 1; }
  std::lock_guard<std::mutex> g(c->lock);
  c->err.clear();
  if (r.fill_level > 2) {
    SET_ERR(c, "fill_level %u: only levels 0-2 are implemented (level 3 "
            "needs a multilabel dilation, 4+ a merge threshold)",
            r.fill_level);
    return 6;
  }
  if (r.fill_level && (r.flags & MG_FLAG_SKIP_H2D)) {
    SET_ERR(c, "fill_holes cannot be combined with MG_FLAG_SKIP_H2D (the "
            "resident volume is already filled)");
    return 6;
  }
  if (!r.labels || (!r.out && !r.bout)) {
    SET_ERR(c, "null argument");
    return 1;
  }
  if (r.bout)
    if (int e = check_encode_params(c, r.ep, &r.enc)) return e;
  const bool counted = c->counted_valid;
  c->holes_valid = false;  // a stash belongs to the call just before
  c->counted_valid = false;
  if (int e = check_volume_args(c, r.sx, r.sy, r.sz, r.dtype)) return e;
  if (r.map)
    if (int e = check_label_map(c, r.map, r.dtype, r.flags)) return e;
  if (r.flags & MG_FLAG_COUNTED)
    if (int e = check_counted(c, r, counted)) return e;
  HIP_TRY(c, hipSetDevice(c->device), 4);
  return mesh_chunk_impl(c, r);
}

extern "C" {

int mg_mesh_chunk_filled(mg_ctx *c, const void *labels, int sx, int sy,
                         int sz, int dtype, float rx, float ry, float rz,
                         uint32_t reduction_factor, float max_error,
                         int voxel_centered, uint64_t dust_threshold,
                         uint32_t flags, const mg_label_map *map,
                         uint32_t fill_level, mg_meshset **out) {
  return mesh_chunk_checked(
      c, {labels, sx, sy, sz, dtype, rx, ry, rz, reduction_factor, max_error,
          voxel_centered, dust_threshold, flags, map, fill_level, nullptr,
          out, nullptr});
}

int mg_mesh_chunk_encoded(mg_ctx *c, const void *labels, int sx, int sy,
                          int sz, int dtype, float rx, float ry, float rz,
                          uint32_t reduction_factor, float max_error,
                          int voxel_centered, uint64_t dust_threshold,
                          uint32_t flags, const mg_label_map *map,
                          const mg_encode_params *params, mg_blobset **out) {
  return mesh_chunk_checked(
      c, {labels, sx, sy, sz, dtype, rx, ry, rz, reduction_factor, max_error,
          voxel_centered, dust_threshold, flags, map, 0u, params, nullptr,
          out});
}

// the blob is ctx-owned (pinned, reused); this frees the descriptor
void mg_blobset_free(mg_blobset *bs) { free(bs); }

int mg_mesh_chunk_mapped(mg_ctx *c, const void *labels, int sx, int sy,
                         int sz, int dtype, float rx, float ry, float rz,
                         uint32_t reduction_factor, float max_error,
                         int voxel_centered, uint64_t dust_threshold,
                         uint32_t flags, const mg_label_map *map,
                         mg_meshset **out) {
  return mesh_chunk_checked(
      c, {labels, sx, sy, sz, dtype, rx, ry, rz, reduction_factor, max_error,
          voxel_centered, dust_threshold, flags, map, 0u, nullptr, out,
          nullptr});
}

int mg_mesh_chunk(mg_ctx *c, const void *labels, int sx, int sy, int sz,
                  int dtype, float rx, float ry, float rz,
                  uint32_t reduction_factor, float max_error,
                  int voxel_centered, uint64_t dust_threshold,
                  uint32_t flags, mg_meshset **out) {
  return mesh_chunk_checked(
      c, {labels, sx, sy, sz, dtype, rx, ry, rz, reduction_factor, max_error,
          voxel_centered, dust_threshold, flags, nullptr, 0u, nullptr, out,
          nullptr});
}

int mg_mesh_holes(mg_ctx *c, float rx, float ry, float rz,
                  uint32_t reduction_factor, float max_error,
                  int voxel_centered, uint32_t flags, mg_meshset **out) {
  if (!c) { SET_ERR(c, "null ctx"); return 1; }
  std::lock_guard<std::mutex> g(c->lock);
  c->err.clear();
  if (!out) { SET_ERR(c, "null argument"); return 1; }
  if (!c->holes_valid) {
    SET_ERR(c, "mg_mesh_holes: no hole volume on this ctx (it is left by "
            "mg_mesh_chunk_filled with fill_level > 0 and consumed by one "
            "mg_mesh_holes call)");
    return 7;
  }
  c->holes_valid = false;  // consumed, also on failure below
  c->counted_valid = false;
  HIP_TRY(c, hipSetDevice(c->device), 4);
  // the hole volume becomes the resident label volume: no upload
  std::swap(c->labels, c->holes);
  return mesh_chunk_impl(
      c, {nullptr, c->holes_sx, c->holes_sy, c->holes_sz, c->holes_dtype, rx,
          ry, rz, reduction_factor, max_error, voxel_centered, 0,
          (flags & MG_FLAG_DEVICE_ONLY) | MG_FLAG_SKIP_H2D, nullptr, 0u,
          nullptr, out, nullptr});
}

int mg_fill_holes(mg_ctx *c, const void *labels, int sx, int sy, int sz,
                  int dtype, uint32_t level, void *filled_out,
                  void *holes_out, uint32_t *rounds_out) {
  if (!c) { SET_ERR(c, "null ctx"); return 1; }
  std::lock_guard<std::mutex> g(c->lock);
  c->err.clear();
  if (!labels || !filled_out || !holes_out) {
    SET_ERR(c, "null argument");
    return 1;
  }
  if (int e = check_volume_args(c, sx, sy, sz, dtype)) return e;
  if (level < 1 || level > 2) {
    SET_ERR(c, "fill level %u: only levels 1-2 are implemented (level 3 "
            "needs a multilabel dilation, 4+ a merge threshold)", level);
    return 6;
  }
  HIP_TRY(c, hipSetDevice(c->device), 4);
  const size_t bytes = (size_t)sx * sy * sz * (dtype == MG_U64 ? 8 : 4);
  c->holes_valid = false;  // c->holes is overwritten
  c->counted_valid = false;  // ... and so is c->labels
  if (ensure_bytes(c, c->labels, bytes)) return 11;
  HIP_TRY(c, hipMemcpyAsync(c->labels.ptr, labels, bytes,
                            hipMemcpyHostToDevice, c->stream), 11);
  uint32_t rounds = 0;
  int rc = run_fill_holes(c, dtype, sx, sy, sz, level, &rounds);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(filled_out, c->labels.ptr, bytes,
                            hipMemcpyDeviceToHost, c->stream), 55);
  HIP_TRY(c, hipMemcpyAsync(holes_out, c->holes.ptr, bytes,
                            hipMemcpyDeviceToHost, c->stream), 55);
  HIP_TRY(c, hipStreamSynchronize(c->stream), 55);
  if (rounds_out) *rounds_out = rounds;
  return 0;
}

// Standalone mesh simplification (multires LOD chain; see meshgine.h).
// Reuses the per-label simplify machinery with ONE label spanning the
// whole mesh.
int mg_simplify_mesh(mg_ctx *c,
                     const float *verts, uint32_t nverts,
                     const uint32_t *faces, uint32_t ntris,
                     uint32_t reduction_factor, float max_error,
                     const float **out_verts, uint32_t *out_nverts,
                     const uint32_t **out_faces, uint32_t *out_ntris) {
  if (!c) { SET_ERR(c, "null ctx"); return 1; }
  std::lock_guard<std::mutex> g(c->lock);
  c->err.clear();
  if (!verts || !faces || !out_verts || !out_faces) {
    SET_ERR(c, "null argument");
    return 1;
  }
  c->counted_valid = false;  // a stash belongs to the call just before
  if (ntris > (1u << 31) / 3) {
    SET_ERR(c, "mesh too large (%u tris)", ntris);
    return 2;
  }
  HIP_TRY(c, hipSetDevice(c->device), 4);
  hipStream_t s = c->stream;
  uint64_t T = ntris, V = nverts;

  if (reduction_factor > 1 && T > 0 && V > 0) {
    if (ensure(c, c->verts, 3 * V + 3)) return 10;
    if (ensure(c, c->faces, 3 * T + 1)) return 10;
    if (ensure(c, c->tri_off, 2)) return 10;
    if (ensure(c, c->vbase, 2)) return 10;
    if (ensure(c, c->tri_label, T + 1)) return 10;
    // simp_finalize's vertex renumbering
    if (ensure(c, c->vtx_scan, std::max<uint64_t>(V + 1, 3 * T))) return 10;
    HIP_TRY(c, hipMemcpyAsync(c->verts.get(), verts, V * 12,
                              hipMemcpyHostToDevice, s), 11);
    HIP_TRY(c, hipMemcpyAsync(c->faces.get(), faces, 3 * T * 4,
                              hipMemcpyHostToDevice, s), 11);
    uint32_t off_h[2] = {0, (uint32_t)T};
    uint32_t vb_h[2] = {0, (uint32_t)V};
    HIP_TRY(c, hipMemcpyAsync(c->tri_off.get(), off_h, 8,
                              hipMemcpyHostToDevice, s), 11);
    HIP_TRY(c, hipMemcpyAsync(c->vbase.get(), vb_h, 8,
                              hipMemcpyHostToDevice, s), 11);
    HIP_TRY(c, hipMemsetAsync(c->tri_label.get(), 0, T * 4, s), 11);
    int rc = run_simplify(c, 1, c->tri_label.get(), reduction_factor,
                          max_error, &T, &V);
    if (rc) return rc;
    if (ensure(c, c->h_verts, 3 * V + 3)) return 12;
    if (ensure(c, c->h_faces, 3 * T + 1)) return 12;
    if (V > 0)
      HIP_TRY(c, hipMemcpyAsync(c->h_verts.get(), c->verts.get(), V * 12,
                                hipMemcpyDeviceToHost, s), 12);
    if (T > 0)
      HIP_TRY(c, hipMemcpyAsync(c->h_faces.get(), c->faces.get(), 3 * T * 4,
                                hipMemcpyDeviceToHost, s), 12);
    HIP_TRY(c, hipStreamSynchronize(s), 12);
  } else {
    // no-op request: hand back a staged copy (uniform ownership)
    if (ensure(c, c->h_verts, 3 * V + 3)) return 12;
    if (ensure(c, c->h_faces, 3 * T + 1)) return 12;
    memcpy(c->h_verts.get(), verts, V * 12);
    memcpy(c->h_faces.get(), faces, 3 * T * 4);
  }
  *out_verts = c->h_verts.get();
  *out_nverts = (uint32_t)V;
  *out_faces = c->h_faces.get();
  *out_ntris = (uint32_t)T;
  return 0;
}

// Grid-chunk and clip one mesh (multires merge; see meshgine.h). The
// pipeline is in chunk_mesh.hip.
int mg_chunk_mesh(mg_ctx *c,
                  const float *verts, uint32_t nverts,
                  const uint32_t *faces, uint32_t ntris,
                  const double scale[3], const double offset[3],
                  mg_meshset **out, const uint32_t **out_order) {
  if (!c) { SET_ERR(c, "null ctx"); return 1; }
  std::lock_guard<std::mutex> g(c->lock);
  c->err.clear();
  if (!out || !out_order || !scale || !offset ||
      (ntris > 0 && (!verts || !faces))) {
    SET_ERR(c, "null argument");
    return 1;
  }
  *out = nullptr;
  *out_order = nullptr;
  c->counted_valid = false;  // a stash belongs to the call just before
  if (ntris > (1u << 31) / 3) {
    SET_ERR(c, "mesh too large (%u tris)", ntris);
    return 2;
  }
  if (ntris == 0) {
    mg_meshset *ms = alloc_meshset(0, 1);
    if (!ms) { SET_ERR(c, "chunk_mesh: out of host memory"); return 73; }
    *out = ms;
    *out_order = ms->nf_arr + ms->nmeshes;
    return 0;
  }
  HIP_TRY(c, hipSetDevice(c->device), 4);
  return run_chunk_mesh(c, verts, nverts, faces, ntris, scale, offset, out,
                        out_order);
}

// the argument checks the two weld entry points share (the ctx is locked)
static int check_weld_args(mg_ctx *c, const float *verts, uint32_t nverts,
                           const uint32_t *faces, uint32_t ntris,
                           const float **out_verts, uint32_t *out_nverts,
                           const uint32_t **out_faces, uint32_t *out_ntris) {
  if (!out_verts || !out_nverts || !out_faces || !out_ntris ||
      (nverts > 0 && !verts) || (ntris > 0 && !faces)) {
    SET_ERR(c, "null argument");
    return 1;
  }
  *out_verts = nullptr;
  *out_faces = nullptr;
  *out_nverts = 0;
  *out_ntris = 0;
  c->counted_valid = false;  // a stash belongs to the call just before
  if (ntris > (1u << 31) / 3 || nverts > (1u << 31)) {
    SET_ERR(c, "mesh too large (%u vertices, %u tris)", nverts, ntris);
    return 2;
  }
  return 0;
}

// Weld the vertices of one mesh that lie within `radius` of each other
// (multires merge; see meshgine.h). The pipeline is in merge_verts.hip.
int mg_merge_close_vertices(mg_ctx *c,
                            const float *verts, uint32_t nverts,
                            const uint32_t *faces, uint32_t ntris,
                            double radius,
                            const float **out_verts, uint32_t *out_nverts,
                            const uint32_t **out_faces, uint32_t *out_ntris) {
  if (!c) { SET_ERR(c, "null ctx"); return 1; }
  std::lock_guard<std::mutex> g(c->lock);
  c->err.clear();
  if (int e = check_weld_args(c, verts, nverts, faces, ntris, out_verts,
                              out_nverts, out_faces, out_ntris))
    return e;
  HIP_TRY(c, hipSetDevice(c->device), 4);
  return run_merge_close_host(c, verts, nverts, faces, ntris, radius,
                              out_verts, out_nverts, out_faces, out_ntris);
}

// Grid-chunk one mesh, concatenate the cells and weld them, all on the
// device (multires merge; see meshgine.h).
int mg_retriangulate_mesh(mg_ctx *c,
                          const float *verts, uint32_t nverts,
                          const uint32_t *faces, uint32_t ntris,
                          const double scale[3], const double offset[3],
                          double radius,
                          const float **out_verts, uint32_t *out_nverts,
                          const uint32_t **out_faces, uint32_t *out_ntris) {
  if (!c) { SET_ERR(c, "null ctx"); return 1; }
  std::lock_guard<std::mutex> g(c->lock);
  c->err.clear();
  if (!scale || !offset) { SET_ERR(c, "null argument"); return 1; }
  if (int e = check_weld_args(c, verts, nverts, faces, ntris, out_verts,
                              out_nverts, out_faces, out_ntris))
    return e;
  bool no_cells = true;
  if (ntris > 0) {
    HIP_TRY(c, hipSetDevice(c->device), 4);
    if (int e = run_retriangulate(c, verts, nverts, faces, ntris, scale,
                                  offset, radius, &no_cells, out_verts,
                                  out_nverts, out_faces, out_ntris))
      return e;
  } else if (int e = mv_check_radius(c, radius)) {
    return e;
  }
  if (no_cells) {  // the input is the result: NULL arrays, its counts
    *out_verts = nullptr;
    *out_faces = nullptr;
    *out_nverts = nverts;
    *out_ntris = ntris;
  }
  return 0;
}

// Encode one level of one mesh's multires octree (see meshgine.h). The
// pipeline is in octree_level.hip.
int mg_encode_octree_level(mg_ctx *c,
                           const float *verts, uint32_t nverts,
                           const uint32_t *faces, uint32_t ntris,
                           const mg_octree_level *lv, mg_fragset **out) {
  if (!c) { SET_ERR(c, "null ctx"); return 1; }
  std::lock_guard<std::mutex> g(c->lock);
  c->err.clear();
  if (!lv || !out || (nverts > 0 && !verts) || (ntris > 0 && !faces)) {
    SET_ERR(c, "null argument");
    return 1;
  }
  *out = nullptr;
  c->counted_valid = false;  // a stash belongs to the call just before
  if (ntris > (1u << 31) / 3 || nverts > (1u << 31)) {
    SET_ERR(c, "mesh too large (%u vertices, %u tris)", nverts, ntris);
    return 2;
  }
  HIP_TRY(c, hipSetDevice(c->device), 4);
  return run_octree_level(c, verts, nverts, faces, ntris, lv, out);
}

// the blob is ctx-owned (pinned, reused); this frees the descriptor
void mg_fragset_free(mg_fragset *fs) { free(fs); }

}  // extern "C"
