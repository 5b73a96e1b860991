// count_voxels.hip — mg_count_voxels: every distinct value of a label volume
// with its voxel count (the reference's CountVoxelsTask,
// igneous/tasks/image/image.py:876 fastremap.unique(labels,
// return_counts=True), and the per-chunk unique of
// MeshTask.apply_dust_global_threshold, igneous/tasks/mesh/mesh.py:346).
// Included by meshgine.hip (single TU) after the chunk stage functions.
//
// One volume pass builds the label hash AND the histogram: a segmentation is
// piecewise constant along x, so the pass counts RUNS of the linear
// (x-fastest) order instead of voxels, and only a run's head touches the
// hash. Runs may cross row ends, since only values matter. Counts sit in a
// u32 array indexed by hash SLOT (the storage of lh_vals, zeroed per
// attempt): the dense ids of LabelHash::vals are stored after the CAS and
// are not visible to the other waves of the same kernel, a slot index is.
// k_count_compact then gathers the occupied slots into (label, count) pairs
// through a cursor; the host sorts them by label, which removes the
// cursor's order, and adds label 0 as nvox minus the rest.

#define COUNT_BLOCK 256
#define COUNT_GRID 2048
#define COUNT_UNROLL 4       // 64-voxel steps loaded ahead per wave
#define COUNT_MAX_PROBE 128  // then the insert gives up and flags overflow
#define COUNT_NO_SLOT 0xFFFFFFFFu

// 1: a wave keeps its last run of a step open in registers and closes it
// when the value changes or its span ends, so a run longer than 64 voxels
// costs one atomic. 0: every 64-voxel step closes its own runs.
#ifndef MG_COUNT_CARRY
#define MG_COUNT_CARRY 1
#endif

// insert-or-find -> the label's slot. The probe sequence is bounded by
// COUNT_MAX_PROBE: a nearly full table is never walked end to end, the
// caller grows it and retries. A non-zero key read is final (slots go 0 ->
// label once), a stale 0 is settled by the CAS.
__device__ __forceinline__ uint32_t count_slot(LabelHash h, uint64_t label) {
  uint64_t slot = mix64(label) & (h.nslots - 1);
  for (int probe = 0; probe < COUNT_MAX_PROBE; ++probe) {
    uint64_t cur = h.keys[slot];
    if (cur == label) return (uint32_t)slot;
    if (cur == 0) {
      uint64_t prev = atomicCAS((unsigned long long *)&h.keys[slot], 0ull,
                                (unsigned long long)label);
      if (prev == 0) {
        atomicAdd(h.counter, 1u);  // distinct labels so far
        return (uint32_t)slot;
      }
      if (prev == label) return (uint32_t)slot;
    }
    slot = (slot + 1) & (h.nslots - 1);
  }
  atomicExch(h.overflow, 1u);
  return COUNT_NO_SLOT;
}

// Wave w walks voxels [w * span, min((w + 1) * span, nvox)), span a multiple
// of 64, in 64-voxel steps. In a step a lane is a run head when its value
// differs from the previous voxel's; one ballot gives the heads, and a
// head's run ends at the next head (or at the step's last valid lane).
template <typename T>
__global__ __launch_bounds__(COUNT_BLOCK) void k_count_runs(
    const T *__restrict__ labels, uint64_t nvox, uint64_t span, LabelHash h,
    uint32_t *__restrict__ cnt) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint64_t wave =
      ((uint64_t)blockIdx.x * COUNT_BLOCK + threadIdx.x) / WAVE;
  const uint64_t begin = wave * span;
  if (begin >= nvox) return;  // wave-uniform
  const uint64_t end = begin + span < nvox ? begin + span : nvox;

  T open_label = 0;       // wave-uniform: the run left open by the last step
  uint32_t open_len = 0;  // 0: none
  for (uint64_t base = begin; base < end; base += COUNT_UNROLL * WAVE) {
    T v[COUNT_UNROLL];
#pragma unroll
    for (int u = 0; u < COUNT_UNROLL; ++u) {
      const uint64_t i = base + (uint64_t)u * WAVE + lane;
      v[u] = i < end ? labels[i] : T(0);
    }
#pragma unroll
    for (int u = 0; u < COUNT_UNROLL; ++u) {
      const uint64_t step = base + (uint64_t)u * WAVE;
      if (step >= end) break;  // wave-uniform
      const uint32_t nvalid = end - step < WAVE ? (uint32_t)(end - step) : WAVE;
      const bool valid = (uint32_t)lane < nvalid;
      const T prev = __shfl_up(v[u], 1, WAVE);
      const bool differs =
          lane == 0 ? (open_len == 0 || v[u] != open_label) : v[u] != prev;
      const unsigned long long heads = __ballot(valid && differs);
      if (heads == 0) {  // the open run goes on through the whole step
        open_len += nvalid;
        continue;
      }
      const int first = __ffsll(heads) - 1;
      const int last = 63 - __clzll(heads);
      const unsigned long long above =
          lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
      // a head closes its own run at the next head; the last head's run
      // stays open, and that lane closes the run open so far instead (its
      // length grown by the lanes ahead of the first head)
      T lab = v[u];
      uint32_t len = above ? (uint32_t)(__ffsll(above) - 1 - lane) : 0u;
      if (lane == last) {
        lab = open_label;
        len = open_len + (uint32_t)first;
      }
      if (valid && differs && lab != 0 && len > 0) {
        const uint32_t slot = count_slot(h, (uint64_t)lab);
        if (slot != COUNT_NO_SLOT) atomicAdd(&cnt[slot], len);
      }
      open_label = __shfl(v[u], last, WAVE);
      open_len = nvalid - (uint32_t)last;
#if !MG_COUNT_CARRY
      if (lane == 0 && open_label != 0) {
        const uint32_t slot = count_slot(h, (uint64_t)open_label);
        if (slot != COUNT_NO_SLOT) atomicAdd(&cnt[slot], open_len);
      }
      open_len = 0;
#endif
    }
  }
  if (lane == 0 && open_len > 0 && open_label != 0) {
    const uint32_t slot = count_slot(h, (uint64_t)open_label);
    if (slot != COUNT_NO_SLOT) atomicAdd(&cnt[slot], open_len);
  }
}

// thread per slot: an occupied slot appends its (label, count) pair
__global__ void k_count_compact(LabelHash h, const uint32_t *__restrict__ cnt,
                                uint32_t *cursor, uint32_t n,
                                uint64_t *__restrict__ out_labels,
                                uint32_t *__restrict__ out_counts) {
  const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= h.nslots) return;
  const uint64_t key = h.keys[slot];
  if (key == 0) return;
  const uint32_t i = atomicAdd(cursor, 1u);
  if (i >= n) return;  // cannot happen: n counted the successful inserts
  out_labels[i] = key;
  out_counts[i] = cnt[slot];
}

// The fused pass on the resident volume, growing the hash until every label
// fits: afterwards c->label_values / c->order hold *p_n (label, count)
// pairs of the non-zero labels, in no order.
static int run_count_voxels(mg_ctx *c, int dtype, uint64_t nvox,
                            uint32_t *p_n) {
  hipStream_t s = c->stream;
  const uint64_t waves = (uint64_t)COUNT_GRID * COUNT_BLOCK / WAVE;
  uint64_t span = (nvox + waves - 1) / waves;
  span = (span + WAVE - 1) / WAVE * WAVE;
  const uint64_t used_waves = (nvox + span - 1) / span;
  const uint32_t grid =
      (uint32_t)((used_waves * WAVE + COUNT_BLOCK - 1) / COUNT_BLOCK);
  uint32_t n = 0;
  for (;;) {
    if (int e = label_hash_reset(c, 91)) return e;
    const LabelHash lh = label_hash_view(c);
    // the counts take the storage of the ids (nobody reads ids here)
    HIP_TRY(c, hipMemsetAsync(lh.vals, 0, lh.nslots * 4, s), 91);
    by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(k_count_runs<T>, dim3(grid), dim3(COUNT_BLOCK), 0, s,
                         c->labels.as<const T>(), nvox, span, lh, lh.vals);
    });
    HIP_TRY(c, hipGetLastError(), 91);
    HIP_TRY(c, hipEventRecord(c->ev[EV_COUNT_END], s), 91);
    uint32_t misc[2] = {0, 0};  // lh_counter, lh_overflow
    HIP_TRY(c, hipMemcpyAsync(misc, &c->scalars->lh_counter, 8,
                              hipMemcpyDeviceToHost, s), 91);
    HIP_TRY(c, hipStreamSynchronize(s), 91);
    if (!misc[1]) {
      n = misc[0];
      break;
    }
    if (int e = label_hash_grow(c, " (count_voxels)", 91)) return e;
  }
  *p_n = n;
  if (n == 0) return 0;
  const LabelHash lh = label_hash_view(c);
  if (ensure(c, c->label_values, n)) return 92;
  if (ensure(c, c->order, n)) return 92;
  hipLaunchKernelGGL(k_count_compact, dim3((uint32_t)((lh.nslots + 255) / 256)),
                     dim3(256), 0, s, lh, lh.vals, &c->scalars->cv_cursor, n,
                     c->label_values.get(), c->order.get());
  HIP_TRY(c, hipGetLastError(), 92);
  return 0;
}

extern "C" {

int mg_count_voxels(mg_ctx *c, const void *labels, int sx, int sy, int sz,
                    int dtype, uint32_t flags, mg_label_counts **out) {
  if (!c) { SET_ERR(c, "null ctx"); return 1; }
  std::lock_guard<std::mutex> g(c->lock);
  c->err.clear();
  if (!labels || !out) { SET_ERR(c, "null argument"); return 1; }
  *out = nullptr;
  c->holes_valid = false;
  c->counted_valid = false;
  if (int e = check_volume_args(c, sx, sy, sz, dtype)) return e;
  ChunkCall k = {};
  k.sx = sx; k.sy = sy; k.sz = sz; k.dtype = dtype;
  k.esize = (dtype == MG_U64) ? 8 : 4;
  k.nvox = (uint64_t)sx * sy * sz;
  if (k.nvox >= (1ull << 32)) {
    SET_ERR(c, "mg_count_voxels: %llu voxels, the device counts are 32-bit "
            "(fewer than 2^32 voxels per call)", (unsigned long long)k.nvox);
    return 2;
  }
  HIP_TRY(c, hipSetDevice(c->device), 4);

  memset(&c->stats, 0, sizeof(c->stats));
  c->stats.bytes_read_algorithmic = k.nvox * k.esize;
  hipStream_t s = c->stream;
  HIP_TRY(c, hipEventRecord(c->ev[EV_START], s), 90);
  if (int e = upload_labels(c, k, labels, flags & MG_FLAG_SKIP_H2D)) return e;
  HIP_TRY(c, hipEventRecord(c->ev[EV_H2D_END], s), 90);
  uint32_t n = 0;
  if (int e = run_count_voxels(c, dtype, k.nvox, &n)) return e;

  std::vector<uint64_t> h_labels(n);
  std::vector<uint32_t> h_counts(n);
  if (n) {
    HIP_TRY(c, hipMemcpyAsync(h_labels.data(), c->label_values.get(),
                              (size_t)n * 8, hipMemcpyDeviceToHost, s), 93);
    HIP_TRY(c, hipMemcpyAsync(h_counts.data(), c->order.get(), (size_t)n * 4,
                              hipMemcpyDeviceToHost, s), 93);
  }
  HIP_TRY(c, hipEventRecord(c->ev[EV_END], s), 93);
  HIP_TRY(c, hipStreamSynchronize(s), 93);

  std::vector<uint32_t> idx(n);
  for (uint32_t i = 0; i < n; ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
    return h_labels[a] < h_labels[b];
  });
  uint64_t nonzero = 0;
  for (uint32_t i = 0; i < n; ++i) nonzero += h_counts[i];
  const uint64_t zeros = k.nvox - nonzero;  // label 0 never enters the hash
  const uint64_t total = (uint64_t)n + (zeros ? 1 : 0);
  // descriptor and both tables in one allocation
  mg_label_counts *lc = (mg_label_counts *)calloc(
      1, sizeof(mg_label_counts) + (size_t)(total ? total : 1) * 16);
  if (!lc) {
    SET_ERR(c, "mg_count_voxels: out of host memory");
    return 94;
  }
  lc->n = total;
  lc->labels = (uint64_t *)(lc + 1);
  lc->counts = lc->labels + total;
  uint64_t at = 0;
  if (zeros) {
    lc->labels[at] = 0;
    lc->counts[at++] = zeros;
  }
  for (uint32_t i = 0; i < n; ++i, ++at) {
    lc->labels[at] = h_labels[idx[i]];
    lc->counts[at] = h_counts[idx[i]];
  }
  *out = lc;

  c->stats.ms_h2d = ev_ms(c, EV_START, EV_H2D_END);
  c->stats.ms_count = ev_ms(c, EV_H2D_END, EV_COUNT_END);
  c->stats.ms_total = ev_ms(c, EV_START, EV_END);
  c->stats.n_labels = n;
  // the raw volume stays resident for one MG_FLAG_COUNTED chunk call
  c->counted_valid = true;
  c->counted_sx = sx; c->counted_sy = sy; c->counted_sz = sz;
  c->counted_dtype = dtype;
  return 0;
}

void mg_label_counts_free(mg_label_counts *lc) { free(lc); }

}  // extern "C"
