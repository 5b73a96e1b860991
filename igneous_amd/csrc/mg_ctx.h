// mg_ctx.h — the engine context and the host helpers every stage driver
// shares. Included at the top of meshgine.hip (single TU).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/meshgine.h"

// Move-only owner of one hipMalloc'd (DevBuf) or pinned (HostBuf) block.
// Moving nulls the source, so std::swap(c->faces, c->simp_faces_alt)
// exchanges the blocks without a free in the swap's temporary.
template <hipError_t (*FREE)(void *)>
struct OwnedBuf {
  void *ptr = nullptr;
  size_t cap = 0;
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf &) = delete;
  OwnedBuf &operator=(const OwnedBuf &) = delete;
  OwnedBuf(OwnedBuf &&o) noexcept
      : ptr(std::exchange(o.ptr, nullptr)), cap(std::exchange(o.cap, 0)) {}
  OwnedBuf &operator=(OwnedBuf &&o) noexcept {
    if (this != &o) {
      release();
      ptr = std::exchange(o.ptr, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~OwnedBuf() { release(); }
  void release() {
    if (ptr) (void)FREE(ptr);
    ptr = nullptr;
    cap = 0;
  }
};
using DevBuf = OwnedBuf<hipFree>;    // untyped: rocPRIM temp storage
using HostBuf = OwnedBuf<hipHostFree>;

// A DevBuf / HostBuf of T. The element type is named once, at the member's
// declaration: get() hands it to kernels, ensure() sizes it in elements,
// and std::swap only compiles between arrays of one type.
template <typename T, typename Owner>
struct TypedArr : Owner {
  T *get() const { return static_cast<T *>(this->ptr); }
  T *operator->() const { return get(); }
};
template <typename T> using DevArr = TypedArr<T, DevBuf>;
template <typename T> using HostArr = TypedArr<T, HostBuf>;

// The resident label volume: u32 or u64 voxels by the call's dtype, so it
// is sized in bytes and typed where the dtype is known (inside by_dtype).
struct LabelVolume : DevBuf {
  template <typename T> T *as() const { return static_cast<T *>(ptr); }
};

// Device-resident scalars that kernels write and the host reads back.
// Allocated and cleared in mg_init; stages pass &c->scalars->field (address
// arithmetic on the device pointer, never dereferenced on the host). No
// field carries a value between calls — each is memset or stored on the
// device inside the call that reads it: the hash words by label_hash_reset
// (which clears the whole block, so the weld_* words start every chunk call
// at 0), map_err by run_label_map, the simp_* totals by k_last_sum, simp_prof by run_simplify,
// cv_cursor by run_count_voxels' own label_hash_reset.
struct CtxScalars {
  uint32_t lh_counter;       // label hash: next dense id = labels so far
  uint32_t lh_overflow;      // label hash: a probe sequence ran out
  uint32_t map_err;          // run_label_map: MAP_ERR_* bits
  uint32_t weld_nlist;       // k_weld_plan: listed blocks of the table path
  uint32_t weld_table_labels;  // k_weld_plan: labels above WELD_LDS_CAP
  uint32_t weld_err;         // k_weld_label: a probe loop hit its bound
  uint32_t simp_kept;        // park_inactive / simp_global_round: faces kept
  uint32_t simp_new_verts;   // simp_finalize: referenced vertices
  uint32_t simp_final_tris;  // simp_finalize: final triangle total
  uint32_t cv_cursor;        // k_count_compact: next (label, count) pair
  unsigned long long simp_prof[6];  // MG_SIMP_PROF phase counters
};
// the hash's two words are read back with one 8-byte copy
static_assert(offsetof(CtxScalars, lh_overflow) ==
                  offsetof(CtxScalars, lh_counter) + 4, "");
// ... and so are k_weld_plan's two
static_assert(offsetof(CtxScalars, weld_table_labels) ==
                  offsetof(CtxScalars, weld_nlist) + 4, "");

struct SimpPlane;  // simplify.hip
struct CmMisc;     // chunk_mesh.hip
struct MvMisc;     // merge_verts.hip

// Every device buffer of a context (grow-only cache). This is the one
// list: ~mg_ctx releases the struct as a whole.
struct DeviceBuffers {
  DevArr<CtxScalars> scalars;
  LabelVolume labels, holes;  // holes: fill_holes' resident hole volume
  DevBuf scan_tmp, sort_tmp;
  DevArr<uint64_t> lh_keys, label_values,
      segcnt, segoff,  // per segment: (triangles << 32) | items
      itscan;  // NI + 1: item -> (its first vertex << 32) | its first triangle
  // Between emit and weld the stream is per ITEM, one (cell, label) pair:
  // tri_label / tri_label_alt (the sort's keys), tri_keys, order /
  // order_alt and itscan hold NI (+1) elements; lab_sorted and everything
  // from the weld on are per triangle.
  DevArr<uint32_t> lh_vals,
      tri_label, tri_label_alt, order, order_alt, tri_off,
      lab_item,     // nlabels + 1: label -> its first item
      blk_item,     // first item of each 256-triangle block of the stream
      blk_list,     // the blocks the weld's global-table path runs over
      lab_sorted,   // label id per triangle (the weld, when a simplify follows)
      keys_sorted,  // the sort's alternate of tri_keys (2 NI words)
      vtx_scan,     // simp_finalize's newid
      wh_keys,      // the weld's global table (labels above WELD_LDS_CAP only)
      faces, vbase;
  DevArr<uint4> weld_quads;  // 3 slots + label per listed triangle
  DevArr<uint2> tri_keys;  // 8-B item records
  DevArr<float> verts;
  // simplifier
  DevArr<SimpPlane> simp_fq;
  DevArr<uint8_t> simp_valid;
  DevArr<float> simp_Q, simp_verts_alt;
  DevArr<unsigned long long> simp_pick;
  DevArr<uint32_t> simp_pk, simp_pk_alt, simp_pv, simp_pv_alt,
      simp_remap, simp_flab, simp_flab_alt, simp_faces_alt, simp_vbase_alt,
      simp_meta,  // carved: simp_alloc
      simp_ref, simp_keep, simp_keep_scan, simp_park, simp_first,
      simp_troff_final, simp_deg, simp_adj, simp_rh, simp_accept;
  // label map table + staged pairs
  DevArr<ulonglong2> map_tab;
  DevArr<uint64_t> map_keys, map_vals;
  // fill_holes: u32 working volume, union-find parents, per-root
  // neighbour min/max, rewrite counter (word 0 of fill_misc)
  DevArr<uint32_t> fill_vol, fill_parent, fill_cmin, fill_cmax, fill_misc;
  // chunk_mesh (chunk_mesh.hip): inputs, per-face / per-pair /
  // per-corner / per-cell arrays, the two sorts' double buffers, outputs
  DevArr<CmMisc> cm_misc;
  DevArr<float> cm_verts, cm_pos, cm_out_v;
  DevArr<uint32_t> cm_faces, cm_ncells, cm_pair_off,
      cm_fkey, cm_fkey_alt, cm_fval, cm_fval_alt,
      cm_npts, cm_npts_s, cm_fhead, cm_coff, cm_ford,
      cm_cfrag, cm_ccell,
      cm_cells,  // carved: CM_CELL_FIELDS arrays of one stride
      cm_wkey, cm_wkey_alt, cm_wval, cm_wval_alt, cm_whead, cm_wrun,
      cm_head_pos, cm_rep, cm_keep, cm_used, cm_vid, cm_fslot, cm_out_f;
  // merge_close_vertices / retriangulate (merge_verts.hip): the mesh to
  // weld, per-vertex cells and union-find parents, the grid sort's double
  // buffers, flags and scans, outputs, the retriangulation's gather table
  DevArr<MvMisc> mv_misc;
  DevArr<float> mv_verts, mv_out_v;
  DevArr<long long> mv_cell;  // 3 per vertex
  DevArr<uint32_t> mv_faces, mv_key, mv_key_alt, mv_val, mv_val_alt,
      mv_parent, mv_keep, mv_used, mv_vid, mv_fslot, mv_out_f,
      mv_tab;  // carved: MV_TAB_FIELDS arrays of one stride
  // encode (encode.hip): per-label entry sizes / offsets / varint index
  // bytes, box words (order-preserving u32) and boxes (f32), the blob
  DevArr<uint64_t> enc_size, enc_off, enc_ilen;
  DevArr<uint32_t> enc_box;
  DevArr<float> enc_bbox;
  DevArr<uint8_t> enc_blob;
  // octree level (octree_level.hip), beside the enc_* arrays it reuses: the
  // entries in z-order, each entry's node, the z-ordered sizes and offsets,
  // the two-entry prefix tables of the unchunked level
  DevArr<uint32_t> ol_order, ol_pref;
  DevArr<int32_t> ol_node;
  DevArr<uint64_t> ol_zsize, ol_zoff;
};

// Timing / ordering events of one mesh_chunk_impl call. EV_H2D_END is
// recorded TWICE: after the upload, and again at the start of the count
// pass — so ms_h2d (EV_START..EV_H2D_END) spans upload + dust + label map
// + fill, and ms_count starts where it ends. Benchmarks and the stored
// profiles were taken with that meaning; keep it.
enum {
  EV_START = 0,
  EV_H2D_END,
  EV_COUNT_END,
  EV_SCAN_END,
  EV_EMIT_END,
  EV_PARTITION_END,
  EV_WELD_END,
  EV_END,           // after the extract
  EV_SIMPLIFY_END,
  EV_SIMP_FORK,     // stream2 waits for the simplify setup
  EV_SIMP_JOIN,     // stream waits for stream2's bands
  EV_MAP_START,
  EV_MAP_END,
  EV_FILL_START,
  EV_FILL_END,
  EV_ENCODE_END,    // after the encode kernels (mg_mesh_chunk_encoded)
  EV_COUNT_
};

struct mg_ctx : DeviceBuffers {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // concurrent simplify band
  std::mutex lock;
  std::string err;
  mg_stats stats = {};
  // hole volume stashed by the last mg_mesh_chunk_filled (mg_mesh_holes
  // consumes it)
  bool holes_valid = false;
  int holes_sx = 0, holes_sy = 0, holes_sz = 0, holes_dtype = 0;
  // raw volume left resident by the last mg_count_voxels (one chunk call
  // with MG_FLAG_COUNTED meshes it without an upload)
  bool counted_valid = false;
  int counted_sx = 0, counted_sy = 0, counted_sz = 0, counted_dtype = 0;
  uint64_t lh_slots = 1ull << 20;
  // pinned output staging, reused across calls
  HostArr<float> h_verts;
  HostArr<uint32_t> h_faces;
  HostArr<uint8_t> h_blob;  // mg_mesh_chunk_encoded's blob, sized in bytes
  HostArr<uint32_t> h_weld_err;  // CtxScalars::weld_err of the current call
  hipEvent_t ev[EV_COUNT_] = {};

  // release order: device buffers, pinned buffers, events, stream2, stream
  ~mg_ctx() {
    (void)hipSetDevice(device);
    static_cast<DeviceBuffers &>(*this) = DeviceBuffers();  // frees each
    h_verts.release();
    h_faces.release();
    h_blob.release();
    h_weld_err.release();
    for (auto &e : ev) if (e) (void)hipEventDestroy(e);
    if (stream2) (void)hipStreamDestroy(stream2);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

static thread_local std::string g_err;  // for ctx==NULL failures

#define SET_ERR(ctx, ...)                                     \
  do {                                                        \
    char _buf[512];                                           \
    snprintf(_buf, sizeof(_buf), __VA_ARGS__);                \
    if (ctx) (ctx)->err = _buf; else g_err = _buf;            \
  } while (0)

#define HIP_TRY(ctx, call, retcode)                           \
  do {                                                        \
    hipError_t _e = (call);                                   \
    if (_e != hipSuccess) {                                   \
      SET_ERR(ctx, "%s failed: %s (%s:%d)", #call,            \
              hipGetErrorString(_e), __FILE__, __LINE__);     \
      return retcode;                                         \
    }                                                         \
  } while (0)

// allocation: grow-only, 25% headroom to damp re-allocs, retry exact
static int ensure_bytes(mg_ctx *c, HostBuf &b, size_t bytes) {
  if (b.cap >= bytes) return 0;
  b.release();
  size_t want = bytes + bytes / 4;
  if (hipHostMalloc(&b.ptr, want) != hipSuccess &&
      hipHostMalloc(&b.ptr, want = bytes) != hipSuccess) {
    SET_ERR(c, "hipHostMalloc(%zu) failed", bytes);
    return 1;
  }
  b.cap = want;
  return 0;
}

static int ensure_bytes(mg_ctx *c, DevBuf &b, size_t bytes) {
  if (b.cap >= bytes) return 0;
  b.release();
  size_t want = bytes + bytes / 4;
  hipError_t e = hipMalloc(&b.ptr, want);
  if (e != hipSuccess) e = hipMalloc(&b.ptr, want = bytes);
  if (e != hipSuccess) {
    SET_ERR(c, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return 1;
  }
  b.cap = want;
  return 0;
}

// room for n elements; b.get() is valid afterwards
template <typename T, typename Owner>
static int ensure(mg_ctx *c, TypedArr<T, Owner> &b, size_t n) {
  return ensure_bytes(c, static_cast<Owner &>(b), n * sizeof(T));
}

// Call f with a zero of the volume's label type, f(uint32_t{}) or
// f(uint64_t{}), so a templated launch is written once:
//   by_dtype(dtype, [&](auto t) { using T = decltype(t); ...k_x<T>... });
template <typename F>
static auto by_dtype(int dtype, F &&f) {
  if (dtype == MG_U64) return f(uint64_t{});
  return f(uint32_t{});
}

// rocPRIM's two-call pattern: size query, grow the temp buffer, run.
// call(tmp_ptr, tmp_bytes) wraps the primitive; the two texts and rc are
// the caller's error for a failed size query / a failed run.
template <typename F>
static int rocprim_two_call(mg_ctx *c, DevBuf &tmp, const char *err_size,
                            const char *err_run, int rc, F call) {
  size_t bytes = 0;
  if (call(nullptr, bytes) != hipSuccess) {
    SET_ERR(c, "%s", err_size);
    return rc;
  }
  if (ensure_bytes(c, tmp, bytes)) return rc;
  if (call(tmp.ptr, bytes) != hipSuccess) {
    SET_ERR(c, "%s", err_run);
    return rc;
  }
  return 0;
}

// Exclusive plus-scan of n u32 values from `in` into `out` on stream s,
// temp storage in c->scan_tmp. In is a template parameter only so that
// each call site keeps the iterator type it always instantiated rocPRIM
// with.
template <typename In>
static int scan_u32(mg_ctx *c, In in, uint32_t *out, size_t n, hipStream_t s,
                    const char *err_size, const char *err_run, int rc) {
  return rocprim_two_call(
      c, c->scan_tmp, err_size, err_run, rc, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, in, out, 0u, n,
                                       rocprim::plus<uint32_t>(), s);
      });
}

// The same over u64 values (the count pass's packed segment counts).
static int scan_u64(mg_ctx *c, const uint64_t *in, uint64_t *out, size_t n,
                    hipStream_t s, const char *err_size, const char *err_run,
                    int rc) {
  return rocprim_two_call(
      c, c->scan_tmp, err_size, err_run, rc, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, in, out, uint64_t{0}, n,
                                       rocprim::plus<uint64_t>(), s);
      });
}

// Inclusive plus-scan of n u64 values: out[i] = in[0] + ... + in[i].
template <typename In>
static int scan_incl_u64(mg_ctx *c, In in, uint64_t *out, size_t n,
                         hipStream_t s, const char *err_size,
                         const char *err_run, int rc) {
  return rocprim_two_call(
      c, c->scan_tmp, err_size, err_run, rc, [&](void *tmp, size_t &bytes) {
        return rocprim::inclusive_scan(tmp, bytes, in, out, n,
                                       rocprim::plus<uint64_t>(), s);
      });
}

// Stable radix sort of n (u32 key, V value) pairs on bits [begin, end) on
// stream s, temp storage in c->sort_tmp; results in the buffers' current().
template <typename V>
static int sort_pairs(mg_ctx *c, rocprim::double_buffer<uint32_t> &keys,
                      rocprim::double_buffer<V> &vals, size_t n,
                      unsigned begin_bit, unsigned end_bit, hipStream_t s,
                      const char *err_size, const char *err_run, int rc) {
  return rocprim_two_call(
      c, c->sort_tmp, err_size, err_run, rc, [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, keys, vals, n,
                                         begin_bit, end_bit, s);
      });
}

// The result descriptor, one calloc: mg_meshset, meshes[n], the flat
// per-mesh arrays labels_arr (u64) and voff/nv/foff/nf (u32) and, behind
// nf_arr, extra_u32_per_mesh more u32 arrays of n (mg_chunk_mesh's
// out_order). Null when the host is out of memory.
static mg_meshset *alloc_meshset(uint32_t n, uint32_t extra_u32_per_mesh) {
  const size_t meta_off = sizeof(mg_meshset) + sizeof(mg_mesh) * n;
  mg_meshset *ms = (mg_meshset *)calloc(
      1, meta_off + (size_t)n * (24 + 4 * extra_u32_per_mesh) +
             2 * sizeof(void *));
  if (!ms) return nullptr;
  ms->nmeshes = n;
  ms->meshes = (mg_mesh *)((char *)ms + sizeof(mg_meshset));
  ms->labels_arr = (uint64_t *)((char *)ms + meta_off);
  ms->voff_arr = (uint32_t *)(ms->labels_arr + n);
  ms->nv_arr = ms->voff_arr + n;
  ms->foff_arr = ms->nv_arr + n;
  ms->nf_arr = ms->foff_arr + n;
  return ms;
}

// Entry m of a meshset whose verts_base / faces_base are set: mesh `label`
// is nv vertices from vertex voff and nf triangles from triangle foff.
static void set_mesh(mg_meshset *ms, uint32_t m, uint64_t label,
                     uint32_t voff, uint32_t nv, uint32_t foff, uint32_t nf) {
  ms->meshes[m] = {label, nv, nf, ms->verts_base + 3ull * voff,
                   ms->faces_base + 3ull * foff};
  ms->labels_arr[m] = label;
  ms->voff_arr[m] = voff;
  ms->nv_arr[m] = nv;
  ms->foff_arr[m] = foff;
  ms->nf_arr[m] = nf;
}
