// simplify.hip — per-label quadric edge-collapse simplifier on the GPU.
//
// Restates zmesh's Mesher.get(id, reduction_factor, max_error,
// voxel_centered) simplification step
// (/root/reference/igneous/tasks/mesh/mesh.py:376-381) with the SAME
// deterministic matched-pair independent-set schedule as the CPU oracle
// (oracle/simplify.c) — bit-exact: identical f32 expressions (plane from
// cross product + correctly-rounded sqrtf/div, unit-weight quadrics summed
// in ascending face order, midpoint placement, cost = (Qu+Qw)(m) <=
// max_error^2, per-vertex cheapest edge with deterministic per-edge tie
// jitter on the 3 low cost bits + smaller-peer tie-break, matched pairs
// collapse, rounds until a label hits its triangle target or stops
// shrinking).
//
// All labels simplify SIMULTANEOUSLY: faces stay label-partitioned, the
// vertex space is label-disjoint (vbase slices), so per-label rounds are
// independent; a finished label freezes while others continue.
//
// Included by meshgine.hip (single TU) after mg_ctx.h and the shared small
// kernels (k_iota, k_last_sum, k_any_active): the kernels first, then their
// host driver (SimpEnv .. run_simplify).

struct SimpPlane {
  float nx, ny, nz, d;
};

// quadric helpers — textually identical arithmetic to oracle/simplify.c
__device__ __forceinline__ void sq_add_plane(float *q, float a, float b,
                                             float c_, float d, float w) {
  q[0] += w * a * a; q[1] += w * a * b; q[2] += w * a * c_; q[3] += w * a * d;
  q[4] += w * b * b; q[5] += w * b * c_; q[6] += w * b * d;
  q[7] += w * c_ * c_; q[8] += w * c_ * d;
  q[9] += w * d * d;
}

__device__ __forceinline__ float sq_eval(const float *q, float x, float y,
                                         float z) {
  return q[0]*x*x + 2.0f*q[1]*x*y + 2.0f*q[2]*x*z + 2.0f*q[3]*x
       + q[4]*y*y + 2.0f*q[5]*y*z + 2.0f*q[6]*y
       + q[7]*z*z + 2.0f*q[8]*z
       + q[9];
}

// Canonical collapse placement — textually identical arithmetic to
// oracle/simplify.c quad_place (the contract expression): GH optimal
// point via Cramer on the summed quadric, midpoint fallback when the
// 3x3 system is near-singular. Writes the placement, returns its cost.
__device__ __forceinline__ float sq_place(const float *S, float mx,
                                          float my, float mz,
                                          float *px, float *py,
                                          float *pz) {
  float a00 = S[0], a01 = S[1], a02 = S[2], b0 = S[3];
  float a11 = S[4], a12 = S[5], b1 = S[6];
  float a22 = S[7], b2 = S[8];
  float m00 = a11*a22 - a12*a12;
  float m01 = a02*a12 - a01*a22;
  float m02 = a01*a12 - a02*a11;
  float m11 = a00*a22 - a02*a02;
  float m12 = a01*a02 - a00*a12;
  float m22 = a00*a11 - a01*a01;
  float det = a00*m00 + a01*m01 + a02*m02;
  float tr = a00 + a11 + a22;
  float x = mx, y = my, z = mz;
  if (fabsf(det) > 1e-6f * tr * tr * tr) {
    float inv = 1.0f / det;
    x = -(m00*b0 + m01*b1 + m02*b2) * inv;
    y = -(m01*b0 + m11*b1 + m12*b2) * inv;
    z = -(m02*b0 + m12*b1 + m22*b2) * inv;
  }
  *px = x; *py = y; *pz = z;
  float cost = sq_eval(S, x, y, z);
  if (cost < 0.0f) cost = 0.0f;
  return cost;
}

// cost-only form for the pick phase (identical arithmetic; the
// placement registers don't outlive the call). Written out rather than
// calling sq_place: the call form leaves the per-label kernel's
// allocation as it is but takes k_edge_pick from 82 to 78 VGPRs, 5 to 6
// waves per SIMD — an occupancy step that should move only in a change
// that times the global-rounds path (simplifier cleanup).
__device__ __forceinline__ float sq_place_cost(const float *S, float mx,
                                               float my, float mz) {
  float a00 = S[0], a01 = S[1], a02 = S[2], b0 = S[3];
  float a11 = S[4], a12 = S[5], b1 = S[6];
  float a22 = S[7], b2 = S[8];
  float m00 = a11*a22 - a12*a12;
  float m01 = a02*a12 - a01*a22;
  float m02 = a01*a12 - a02*a11;
  float m11 = a00*a22 - a02*a02;
  float m12 = a01*a02 - a00*a12;
  float m22 = a00*a11 - a01*a01;
  float det = a00*m00 + a01*m01 + a02*m02;
  float tr = a00 + a11 + a22;
  float x = mx, y = my, z = mz;
  if (fabsf(det) > 1e-6f * tr * tr * tr) {
    float inv = 1.0f / det;
    x = -(m00*b0 + m01*b1 + m02*b2) * inv;
    y = -(m01*b0 + m11*b1 + m12*b2) * inv;
    z = -(m02*b0 + m12*b1 + m22*b2) * inv;
  }
  float cost = sq_eval(S, x, y, z);
  if (cost < 0.0f) cost = 0.0f;
  return cost;
}

// ---- collapse helpers shared by the global-rounds kernels and the
// per-label kernel. Each is the one device copy of an oracle/simplify.c
// expression; expression and operand order are the contract.

// Unit plane of face (i0, i1, i2), global vertex ids. A degenerate face
// gives the zero plane: accumulating it adds exact +0 products, bitwise
// identical to the oracle's skip (quadric sums are never -0). A valid
// plane has a unit normal, so it is never all zero.
__device__ __forceinline__ SimpPlane
sq_face_plane(const float *__restrict__ verts, uint32_t i0, uint32_t i1,
              uint32_t i2) {
  const float *p0 = verts + 3ull*i0, *p1 = verts + 3ull*i1,
              *p2 = verts + 3ull*i2;
  float ux = p1[0]-p0[0], uy = p1[1]-p0[1], uz = p1[2]-p0[2];
  float vx = p2[0]-p0[0], vy = p2[1]-p0[1], vz = p2[2]-p0[2];
  float nx = uy*vz - uz*vy, ny = uz*vx - ux*vz, nz = ux*vy - uy*vx;
  float len = sqrtf(nx*nx + ny*ny + nz*nz);
  if (len <= 0.0f) return SimpPlane{0.0f, 0.0f, 0.0f, 0.0f};
  float inv = 1.0f / len;
  nx *= inv; ny *= inv; nz *= inv;
  float d = -(nx*p0[0] + ny*p0[1] + nz*p0[2]);
  return SimpPlane{nx, ny, nz, d};
}

// Collapse the matched pair (u, w), global ids, u < w: u moves to the
// placement of the summed quadric and absorbs w's quadric. The caller
// owns the remap and pick stores.
__device__ __forceinline__ void sq_collapse(float *__restrict__ verts,
                                            float *__restrict__ Q,
                                            uint64_t u, uint64_t w) {
  float mx = 0.5f*(verts[3*u]+verts[3*w]);
  float my = 0.5f*(verts[3*u+1]+verts[3*w+1]);
  float mz = 0.5f*(verts[3*u+2]+verts[3*w+2]);
  float S[10];
  #pragma unroll
  for (int k = 0; k < 10; ++k) S[k] = Q[12*u + k] + Q[12*w + k];
  float px, py, pz;
  (void)sq_place(S, mx, my, mz, &px, &py, &pz);
  verts[3*u] = px; verts[3*u+1] = py; verts[3*u+2] = pz;
  #pragma unroll
  for (int k = 0; k < 10; ++k) Q[12*u + k] += Q[12*w + k];
}

// Edge picks of one face, in two steps around caller-owned staging arrays
// (declared in the kernel and passed by reference: behind one helper that
// owns them, the compiler allocates the per-label kernel's keep bitmask
// differently and its scratch rises from 48 to 56 B/lane — DESIGN §4).
//
// Step 1: stage the 3 corner quadrics + positions in registers once per
// face. Q rows are 12 floats (48 B, 16-B aligned), 3 dwordx4 loads each;
// the a<b swap in step 2 defeats CSE of the Q loads otherwise, and
// re-loading both quadrics per edge doubles the phase's traffic.
__device__ __forceinline__ void
sq_stage_corners(const uint32_t (&fc)[3], const float *__restrict__ verts,
                 const float *__restrict__ Q, float (&cq)[3][10],
                 float (&cp)[3][3]) {
  #pragma unroll
  for (int ci = 0; ci < 3; ++ci) {
    const float4 *qp = (const float4 *)(Q + 12ull*fc[ci]);
    float4 a = qp[0], b = qp[1], cc = qp[2];
    cq[ci][0] = a.x; cq[ci][1] = a.y; cq[ci][2] = a.z; cq[ci][3] = a.w;
    cq[ci][4] = b.x; cq[ci][5] = b.y; cq[ci][6] = b.z; cq[ci][7] = b.w;
    cq[ci][8] = cc.x; cq[ci][9] = cc.y;
    #pragma unroll
    for (int k = 0; k < 3; ++k) cp[ci][k] = verts[3ull*fc[ci] + k];
  }
}

// Step 2: every edge of the face (corners fc, global ids) whose collapse
// cost is within max_cost bids (cost-bits<<32 | peer) for both ends'
// cheapest-edge slots. pick is indexed by id - pick_base (0 for the global
// table, the label's vertex base for a label-local one); vb is the label's
// vertex base — the tie jitter works in label-LOCAL ids like
// oracle/simplify.c.
__device__ __forceinline__ void
sq_edge_bids(const uint32_t (&fc)[3], const float (&cq)[3][10],
             const float (&cp)[3][3], unsigned long long *pick,
             uint32_t pick_base, uint32_t vb, float max_cost) {
  #pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int ea = e, eb = (e + 1) % 3;   // compile-time after unroll
    uint32_t a = fc[ea], b = fc[eb];
    if (a == b) continue;
    // canonical u < w; addition is commutative-safe here only because
    // both operand orders are evaluated identically (x+y) — keep the
    // oracle's Q[u]+Q[w] order via selects on compile-time indices
    bool fwd = a < b;
    uint32_t u = fwd ? a : b, w = fwd ? b : a;
    float mx = 0.5f*((fwd ? cp[ea][0] : cp[eb][0]) + (fwd ? cp[eb][0] : cp[ea][0]));
    float my = 0.5f*((fwd ? cp[ea][1] : cp[eb][1]) + (fwd ? cp[eb][1] : cp[ea][1]));
    float mz = 0.5f*((fwd ? cp[ea][2] : cp[eb][2]) + (fwd ? cp[eb][2] : cp[ea][2]));
    float S[10];
    #pragma unroll
    for (int k = 0; k < 10; ++k)
      S[k] = (fwd ? cq[ea][k] : cq[eb][k]) + (fwd ? cq[eb][k] : cq[ea][k]);
    float cost = sq_place_cost(S, mx, my, mz);
    if (cost > max_cost) continue;
    uint32_t cb = __float_as_uint(cost);
    // per-edge tie jitter — identical to oracle/simplify.c
    uint32_t ul = u - vb, wl = w - vb;
    uint32_t hsh = ul ^ (wl * 2654435761u);
    hsh ^= hsh >> 16; hsh *= 2246822519u; hsh ^= hsh >> 13;
    cb ^= (hsh & 7u);
    atomicMin(&pick[u - pick_base], ((unsigned long long)cb << 32) | w);
    atomicMin(&pick[w - pick_base], ((unsigned long long)cb << 32) | u);
  }
}

// Quadric of one vertex of degree d <= W from its incident face ids
// fl_in[0..d): sort them ascending in registers (bitonic network,
// compile-time indices; the sorted order is unique because face ids are
// distinct, so it matches the oracle's insertion sort exactly), then add
// the planes in that order into q.
template <int W>
__device__ __forceinline__ void sq_sort_accum(float *q,
                                              const uint32_t *fl_in,
                                              uint32_t d,
                                              const SimpPlane *pl) {
  uint32_t fl[W];
  #pragma unroll
  for (int k = 0; k < W; ++k)
    fl[k] = (k < (int)d) ? fl_in[k] : 0xFFFFFFFFu;
  #pragma unroll
  for (int ksz = 2; ksz <= W; ksz <<= 1) {
    #pragma unroll
    for (int j = ksz >> 1; j > 0; j >>= 1) {
      #pragma unroll
      for (int i = 0; i < W; ++i) {
        int l = i ^ j;
        if (l > i) {
          bool up = ((i & ksz) == 0);
          uint32_t a = fl[i], b2 = fl[l];
          bool sw = up ? (a > b2) : (a < b2);
          fl[i] = sw ? b2 : a;
          fl[l] = sw ? a : b2;
        }
      }
    }
  }
  // gather planes in 8-batches (8 independent loads in flight each) —
  // staging all 16 at once cost 64 VGPRs and pushed the per-label kernel
  // past the 128-VGPR / 4-waves-per-SIMD occupancy step. Accumulation
  // order (ascending fl) is unchanged.
  #pragma unroll
  for (int h = 0; h < W / 8; ++h) {
    SimpPlane ps[8];
    #pragma unroll
    for (int k = 0; k < 8; ++k)
      // pad with face 0 (the label has >= 1 face); fl[k] is the
      // 0xFFFFFFFF sort sentinel beyond d, must not be indexed
      ps[k] = pl[8*h + k < (int)d ? fl[8*h + k] : 0u];
    #pragma unroll
    for (int k = 0; k < 8; ++k)
      if (8*h + k < (int)d)
        sq_add_plane(q, ps[k].nx, ps[k].ny, ps[k].nz, ps[k].d, 1.0f);
  }
}

// [S1] per-face plane (recomputed each round; verts move)
__global__ void k_face_planes(const uint32_t *__restrict__ faces_g,
                              const float *__restrict__ verts,
                              const uint8_t *__restrict__ active_lab,
                              const uint32_t *__restrict__ flab,
                              SimpPlane *__restrict__ fq,
                              uint8_t *__restrict__ fvalid,
                              uint64_t ntris) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntris) return;
  if (!active_lab[flab[t]]) { fvalid[t] = 0; return; }
  SimpPlane p = sq_face_plane(verts, faces_g[3*t], faces_g[3*t+1],
                              faces_g[3*t+2]);
  fq[t] = p;
  fvalid[t] = (p.nx != 0.0f || p.ny != 0.0f || p.nz != 0.0f) ? 1 : 0;
}

// [S2] emit (vertex, face) pairs for quadric accumulation; inactive
// labels get the sentinel key (sorted to the end, skipped)
__global__ void k_emit_vf_pairs(const uint32_t *__restrict__ faces_g,
                                const uint8_t *__restrict__ active_lab,
                                const uint32_t *__restrict__ flab,
                                uint32_t *__restrict__ pk,
                                uint32_t *__restrict__ pv,
                                uint64_t ntris) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntris) return;
  bool act = active_lab[flab[t]];
  #pragma unroll
  for (int v = 0; v < 3; ++v) {
    pk[3*t + v] = act ? faces_g[3*t + v] : 0xFFFFFFFFu;
    pv[3*t + v] = (uint32_t)t;
  }
}

// [S3] per-vertex quadric: walk the vertex's pair segment in ascending
// face order (stable sort preserves it) — the oracle's summation order
__global__ void k_accum_quadrics(const uint32_t *__restrict__ pk,
                                 const uint32_t *__restrict__ pv,
                                 const SimpPlane *__restrict__ fq,
                                 const uint8_t *__restrict__ fvalid,
                                 float *__restrict__ Q,
                                 uint64_t npairs) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npairs) return;
  uint32_t v = pk[i];
  if (v == 0xFFFFFFFFu) return;
  if (i > 0 && pk[i-1] == v) return;  // not a segment head
  float q[10];
  #pragma unroll
  for (int k = 0; k < 10; ++k) q[k] = 0.0f;
  for (uint64_t j = i; j < npairs && pk[j] == v; ++j) {
    uint32_t f = pv[j];
    if (!fvalid[f]) continue;
    SimpPlane p = fq[f];
    sq_add_plane(q, p.nx, p.ny, p.nz, p.d, 1.0f);
  }
  float4 *qo = (float4 *)(Q + 12ull*v);
  qo[0] = make_float4(q[0], q[1], q[2], q[3]);
  qo[1] = make_float4(q[4], q[5], q[6], q[7]);
  qo[2] = make_float4(q[8], q[9], 0.0f, 0.0f);
}

// [S4] per-vertex cheapest incident edge (cost-bits<<32 | peer, min)
__global__ void k_edge_pick(const uint32_t *__restrict__ faces_g,
                            const uint8_t *__restrict__ active_lab,
                            const uint32_t *__restrict__ flab,
                            const uint32_t *__restrict__ vbase,
                            const float *__restrict__ verts,
                            const float *__restrict__ Q,
                            unsigned long long *__restrict__ pick,
                            float max_cost, uint64_t ntris) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntris) return;
  uint32_t lab = flab[t];
  if (!active_lab[lab]) return;
  uint32_t fc[3] = {faces_g[3*t], faces_g[3*t+1], faces_g[3*t+2]};
  float cq[3][10], cp[3][3];
  sq_stage_corners(fc, verts, Q, cq, cp);
  sq_edge_bids(fc, cq, cp, pick, 0u, vbase[lab], max_cost);
}

// [S5] matched pairs collapse; u (smaller id) survives. Matched
// vertices leave the pick graph (blocked marking for the proposal
// wave; the plain-store races are decision-invariant).
__global__ void k_collapse(unsigned long long *__restrict__ pick,
                           float *__restrict__ verts,
                           uint32_t *__restrict__ remap,
                           float *__restrict__ Q,
                           uint64_t nverts) {
  uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= nverts) return;
  unsigned long long pu = pick[u];
  if (pu == ~0ull) return;
  uint32_t w = (uint32_t)pu;
  if (w <= u) return;
  unsigned long long pw = pick[w];
  if (pw == ~0ull || (uint32_t)pw != u) return;
  sq_collapse(verts, Q, u, w);
  remap[w] = (uint32_t)u;
  pick[u] = ~0ull;
  pick[w] = ~0ull;
}

// [S5b] proposal wave (oracle step 3b), global-rounds path. Vertex ids
// in pick are global; the proposer id in the acceptance key preserves
// the oracle's local tie-break order (ids within one label are
// monotone in the global numbering).
__global__ void k_propose(const unsigned long long *__restrict__ pick,
                          uint32_t *__restrict__ accept,
                          uint64_t nverts) {
  uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nverts) return;
  unsigned long long pu = pick[v];
  if (pu == ~0ull) return;
  uint32_t w = (uint32_t)pu;
  if (w <= v) return;                  // propose-up only
  if (pick[w] == ~0ull) return;        // blocked target
  atomicMin(&accept[w], (uint32_t)(v + 1));
}

__global__ void k_accept(const unsigned long long *__restrict__ pick,
                         const uint32_t *__restrict__ accept,
                         float *__restrict__ verts,
                         uint32_t *__restrict__ remap,
                         float *__restrict__ Q,
                         uint64_t nverts) {
  uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nverts) return;
  uint32_t aw = accept[w];
  if (aw == 0xFFFFFFFFu) return;
  unsigned long long pw = pick[w];
  if (pw == ~0ull) return;             // matched or pickless
  if ((uint32_t)pw > w) return;        // proposers never accept
  uint64_t u = (uint64_t)aw - 1;
  sq_collapse(verts, Q, u, w);
  remap[w] = (uint32_t)u;
}

// [S6] remap face corners in place; keep flag for non-degenerates
__global__ void k_remap_faces(uint32_t *__restrict__ faces_g,
                              const uint32_t *__restrict__ remap,
                              uint32_t *__restrict__ keep,
                              uint64_t ntris) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntris) return;
  uint32_t i0 = remap[faces_g[3*t]], i1 = remap[faces_g[3*t+1]],
           i2 = remap[faces_g[3*t+2]];
  faces_g[3*t] = i0; faces_g[3*t+1] = i1; faces_g[3*t+2] = i2;
  keep[t] = (i0 != i1 && i1 != i2 && i0 != i2) ? 1u : 0u;
}

// [S7] stable compaction of kept faces (+ labels); per-label new counts
__global__ void k_compact_faces(const uint32_t *__restrict__ faces_g,
                                const uint32_t *__restrict__ flab,
                                const uint32_t *__restrict__ keep,
                                const uint32_t *__restrict__ keep_scan,
                                uint32_t *__restrict__ faces_out,
                                uint32_t *__restrict__ flab_out,
                                uint32_t *__restrict__ nt_new,
                                uint64_t ntris) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntris) return;
  if (!keep[t]) return;
  uint64_t o = keep_scan[t];
  faces_out[3*o] = faces_g[3*t];
  faces_out[3*o+1] = faces_g[3*t+1];
  faces_out[3*o+2] = faces_g[3*t+2];
  uint32_t lab = flab[t];
  flab_out[o] = lab;
  atomicAdd(&nt_new[lab], 1u);
}

// [S8] per-label round bookkeeping
__global__ void k_update_active(const uint32_t *__restrict__ nt_new,
                                uint32_t *__restrict__ nt_cur,
                                const uint32_t *__restrict__ target,
                                uint8_t *__restrict__ active_lab,
                                uint32_t *__restrict__ any_active,
                                uint32_t nlabels,
                                uint32_t enforce_progress) {
  // enforce_progress=1 on a group's FIRST sub-round: a label whose
  // fresh-quadric sub collapses nothing is done (oracle termination).
  // Later subs leave no-progress labels active — they recompute next
  // group (their remaining subs this group are deterministic no-ops).
  uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nlabels) return;
  if (!active_lab[l]) return;
  uint32_t nn = nt_new[l];
  bool progress = nn != nt_cur[l];
  nt_cur[l] = nn;
  bool act = nn > target[l] && (progress || !enforce_progress);
  active_lab[l] = act ? 1 : 0;
  if (act) atomicExch(any_active, 1u);
}

__global__ void k_init_simplify(const uint32_t *__restrict__ tri_off,
                                uint32_t *__restrict__ nt_cur,
                                uint32_t *__restrict__ target,
                                uint8_t *__restrict__ active_lab,
                                uint32_t reduction_factor,
                                uint32_t nlabels) {
  uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nlabels) return;
  uint32_t nt = tri_off[l+1] - tri_off[l];
  uint32_t tg = nt / reduction_factor;
  if (tg < 1) tg = 1;
  nt_cur[l] = nt;
  target[l] = tg;
  active_lab[l] = (nt > tg) ? 1 : 0;
}

// faces local -> global vertex ids (vbase offset per label)
__global__ void k_globalize_faces(uint32_t *__restrict__ faces,
                                  const uint32_t *__restrict__ lab_sorted,
                                  const uint32_t *__restrict__ vbase,
                                  uint32_t *__restrict__ flab,
                                  uint64_t ntris) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntris) return;
  uint32_t lab = lab_sorted[t];
  flab[t] = lab;
  uint32_t base = vbase[lab];
  faces[3*t] += base; faces[3*t+1] += base; faces[3*t+2] += base;
}

// ---- final referenced-vertex compaction ------------------------------

__global__ void k_mark_ref(const uint32_t *__restrict__ faces_g,
                           uint32_t *__restrict__ ref, uint64_t ncorners) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncorners) return;
  ref[faces_g[i]] = 1u;  // idempotent store, order-free
}

__global__ void k_scatter_verts(const float *__restrict__ verts,
                                const uint32_t *__restrict__ ref,
                                const uint32_t *__restrict__ newid,
                                float *__restrict__ verts_out,
                                uint64_t nverts) {
  uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nverts) return;
  if (!ref[v]) return;
  uint64_t o = newid[v];
  verts_out[3*o] = verts[3*v];
  verts_out[3*o+1] = verts[3*v+1];
  verts_out[3*o+2] = verts[3*v+2];
}

__global__ void k_new_vbase(const uint32_t *__restrict__ vbase_old,
                            const uint32_t *__restrict__ newid,
                            uint32_t *__restrict__ vbase_new,
                            uint32_t nlabels, uint32_t total_new) {
  uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l > nlabels) return;
  vbase_new[l] = (l == nlabels) ? total_new : newid[vbase_old[l]];
}

__global__ void k_localize_faces(const uint32_t *__restrict__ faces_g,
                                 const uint32_t *__restrict__ newid,
                                 const uint32_t *__restrict__ flab,
                                 const uint32_t *__restrict__ vbase_new,
                                 uint32_t *__restrict__ faces_out,
                                 uint64_t ntris) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntris) return;
  uint32_t base = vbase_new[flab[t]];
  faces_out[3*t] = newid[faces_g[3*t]] - base;
  faces_out[3*t+1] = newid[faces_g[3*t+1]] - base;
  faces_out[3*t+2] = newid[faces_g[3*t+2]] - base;
}

// ---- working-set parking: a label that goes inactive leaves the round
// loop entirely; its faces are stored verbatim (in face order) at the
// label's ORIGINAL tri_off offset in the park store, and the working
// array keeps only active labels' faces. Late rounds then touch only the
// shrinking active tail instead of all 155M faces.

__global__ void k_flag_active_faces(const uint32_t *__restrict__ flab,
                                    const uint8_t *__restrict__ active_lab,
                                    uint32_t *__restrict__ aflag,
                                    uint64_t ntris) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntris) return;
  aflag[t] = active_lab[flab[t]] ? 1u : 0u;
}

__global__ void k_first_label_idx(const uint32_t *__restrict__ flab,
                                  uint32_t *__restrict__ first,
                                  uint64_t ntris) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntris) return;
  if (t == 0 || flab[t] != flab[t - 1]) first[flab[t]] = (uint32_t)t;
}

__global__ void k_park_scatter(const uint32_t *__restrict__ faces_g,
                               const uint32_t *__restrict__ flab,
                               const uint32_t *__restrict__ aflag,
                               const uint32_t *__restrict__ apos,
                               const uint32_t *__restrict__ first,
                               const uint32_t *__restrict__ orig_tri_off,
                               uint32_t *__restrict__ work_faces,
                               uint32_t *__restrict__ work_flab,
                               uint32_t *__restrict__ park_faces,
                               uint32_t skip_cap,  // labels <= this size
                               // were parked by k_simplify_label: drop
                               uint64_t ntris) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntris) return;
  uint32_t lab = flab[t];
  if (!aflag[t] &&
      orig_tri_off[lab + 1] - orig_tri_off[lab] <= skip_cap)
    return;  // small label: its park slice is already final
  if (aflag[t]) {
    uint64_t o = apos[t];
    work_faces[3*o] = faces_g[3*t];
    work_faces[3*o+1] = faces_g[3*t+1];
    work_faces[3*o+2] = faces_g[3*t+2];
    work_flab[o] = lab;
  } else {
    uint64_t o = (uint64_t)orig_tri_off[lab] + ((uint32_t)t - first[lab]);
    park_faces[3*o] = faces_g[3*t];
    park_faces[3*o+1] = faces_g[3*t+1];
    park_faces[3*o+2] = faces_g[3*t+2];
  }
}

// assemble the final compact face array from the park store
__global__ void k_gather_final(const uint32_t *__restrict__ park_faces,
                               const uint32_t *__restrict__ orig_tri_off,
                               const uint32_t *__restrict__ final_tri_off,
                               uint32_t *__restrict__ faces_out,
                               uint32_t *__restrict__ flab_out,
                               uint32_t nlabels, uint64_t final_total) {
  uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= final_total) return;
  // binary search: label whose [final_tri_off[l], final_tri_off[l+1]) holds f
  uint32_t lo = 0, hi = nlabels;
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if ((uint64_t)final_tri_off[mid] <= f) lo = mid; else hi = mid;
  }
  uint32_t l = lo;
  uint64_t src = (uint64_t)orig_tri_off[l] + (f - final_tri_off[l]);
  faces_out[3*f] = park_faces[3*src];
  faces_out[3*f+1] = park_faces[3*src+1];
  faces_out[3*f+2] = park_faces[3*src+2];
  flab_out[f] = l;
}

// ---------------------------------------------------------------------------
// Per-label simplification: one workgroup runs a label's ENTIRE round
// loop over its own slices of the global arrays (faces/verts/Q/pick/
// remap + a per-label CSR). A label's working set (~100-300 KB) stays
// cache-resident and there are no global sorts, no host round trips and
// no device-wide synchronization — all 50k labels simplify concurrently.
// Labels larger than `big_cap` faces are left to the global-rounds path.
//
// Arithmetic and schedule are IDENTICAL to oracle/simplify.c per label
// (same plane/quadric/cost expressions, ascending-face quadric order via
// the sorted CSR, jittered pick encoding on label-local ids, mutual-pick
// matched collapse, stable compaction, same termination conditions).

// labels up to SIMP_BIG_CAP faces simplify entirely inside one workgroup
// each (cache-resident round loop, no global sorts); only bigger labels
// go through the global-rounds machinery.
#define SIMP_BIG_CAP 65536u
// threads per label workgroup: the kernel's launch bounds and strides and
// the host's block dimension (6/256 won the SUBS x BS sweeps)
constexpr int SIMP_LABEL_BS = 256;

// wave-shuffle prefix machinery shared by the block-wide helpers below:
// each thread sums its contiguous chunk, a 64-lane shuffle scan orders
// the per-thread partials within the wave (no LDS), ONE barrier shares
// the NW wave totals, and every thread derives its global offset from
// the (tiny) wave-total array. 2 barriers per helper call instead of the
// 16+ of the old Hillis-Steele block scan — the round loop's barrier
// count was the per-label kernel's dominant WAIT source.
template <int BS>
__device__ __forceinline__ uint32_t blk_prefix(uint32_t sum,
                                               uint32_t *s_wsum /*NW*/,
                                               uint32_t *p_total) {
  constexpr int NW = BS / 64;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  uint32_t incl = sum;
  #pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t y = __shfl_up(incl, d, 64);
    if (lane >= d) incl += y;
  }
  if (lane == 63) s_wsum[wid] = incl;
  __syncthreads();
  uint32_t wbase = 0, total = 0;
  #pragma unroll
  for (int w = 0; w < NW; ++w) {
    uint32_t x = s_wsum[w];
    if (w < wid) wbase += x;
    total += x;
  }
  *p_total = total;
  return wbase + incl - sum;  // exclusive prefix of this thread's sum
}

// block-wide exclusive scan of src[0..n) into dst (+base), returns total
template <int BS>
__device__ uint32_t blk_exscan(const uint32_t *src, uint32_t *dst,
                               uint32_t n, uint32_t base,
                               uint32_t *s_sums /*>= BS/64*/,
                               uint32_t *dst2 = nullptr) {
  const uint32_t tid = threadIdx.x;
  const uint32_t chunk = (n + BS - 1) / BS;
  const uint32_t lo = tid * chunk;
  const uint32_t hi = lo + chunk < n ? lo + chunk : n;
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += src[i];
  uint32_t total;
  uint32_t excl = blk_prefix<BS>(sum, s_sums, &total);
  uint32_t run = base + excl;
  for (uint32_t i = lo; i < hi; ++i) {
    uint32_t t = src[i];
    dst[i] = run;
    if (dst2) dst2[i] = run;  // optional cursor copy (src may alias
    run += t;                 // dst2: t was read first)
  }
  __syncthreads();  // s_sums reusable after this
  return total;
}

// fused face rewrite + stable compaction: remap corners through the
// label-local rm[] (LDS), keep-flag in a register bitmask (no valid[]
// array traffic), scan via blk_prefix, scatter kept remapped faces into
// fb. fa is never written: the second pass re-reads fa and re-applies
// the (cheap, LDS) rm gathers instead of paying a 12 B/face global
// write + re-read. Identical output order to the old rewrite + compact
// pair.
template <int BS>
__device__ uint32_t blk_rewrite_compact(const uint32_t *__restrict__ fa,
                                        uint32_t *__restrict__ fb,
                                        const uint32_t *__restrict__ rm,
                                        uint32_t v0,
                                        uint32_t n, uint32_t *s_sums) {
  const uint32_t tid = threadIdx.x;
  const uint32_t chunk = (n + BS - 1) / BS;
  const uint32_t lo = tid * chunk;
  const uint32_t hi = lo + chunk < n ? lo + chunk : n;
  // bitmask register array sized for the kernel's face-count cap
  constexpr uint32_t MAXW = (SIMP_BIG_CAP / BS + 63) / 64 + 1;
  unsigned long long bm[MAXW] = {};
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) {
    uint32_t i0 = rm[fa[3*i] - v0];
    uint32_t i1 = rm[fa[3*i+1] - v0];
    uint32_t i2 = rm[fa[3*i+2] - v0];
    if (i0 != i1 && i1 != i2 && i0 != i2) {
      bm[(i - lo) >> 6] |= 1ull << ((i - lo) & 63);
      ++sum;
    }
  }
  uint32_t total;
  uint32_t run = blk_prefix<BS>(sum, s_sums, &total);
  for (uint32_t i = lo; i < hi; ++i)
    if (bm[(i - lo) >> 6] & (1ull << ((i - lo) & 63))) {
      fb[3*run] = v0 + rm[fa[3*i] - v0];
      fb[3*run+1] = v0 + rm[fa[3*i+1] - v0];
      fb[3*run+2] = v0 + rm[fa[3*i+2] - v0];
      ++run;
    }
  __syncthreads();  // s_sums reusable after this
  return total;
}

// pick/remap/accept reset of one label-local vertex slot
__device__ __forceinline__ void simp_reset_vertex(unsigned long long *pick_l,
                                                  uint32_t *rm,
                                                  uint32_t *accept_l,
                                                  uint32_t v,
                                                  uint32_t propose) {
  pick_l[v] = ~0ull;
  rm[v] = v;  // remap identity (consumed in collapse)
  if (propose) accept_l[v] = 0xFFFFFFFFu;
}

// CAPV = LDS vertex capacity: a label with nv <= CAPV keeps its degree,
// pick and remap tables in LDS, a bigger one in its global slices.
// amdgpu_waves_per_eu(4) IS applied, as a floor of 4 waves per SIMD. The
// CAPV=2048 instantiation meets it: 128 VGPRs, 48 B/lane of scratch (the
// keep bitmask and a few spills; the 16-wide sort tier is the VGPR peak).
// The floor lost 7% while it spilled 52 B/lane from a 148-VGPR kernel and
// was adopted once the kernel fit (simplifier journey and the
// cleanup's resource table). The CAPV=4096 instantiation cannot meet the
// floor — its 64 KB of LDS allows 2 blocks per CU = 2 waves per SIMD — so
// the compiler warns "desired occupancy was 4, final occupancy is 2" for
// it; that is LDS-bound and expected, and it keeps its natural
// spill-free 151-VGPR allocation.
template <int CAPV>
__global__ __launch_bounds__(SIMP_LABEL_BS)
__attribute__((amdgpu_waves_per_eu(4))) void k_simplify_label(
    uint32_t *__restrict__ faces_g,       // slices at 3*tri_off[b]
    uint32_t *__restrict__ faces_tmp,     // same slicing (scratch)
    const uint32_t *__restrict__ tri_off, // L+1 (original offsets)
    const uint32_t *__restrict__ vbase,   // L+1
    float *__restrict__ verts,
    float *__restrict__ Q,                // 10 per vertex
    unsigned long long *__restrict__ pick,
    uint32_t *__restrict__ remap,
    uint32_t *__restrict__ deg,           // per vertex (doubles as cursor)
    uint32_t *__restrict__ adj_off,       // per vertex
    uint32_t *__restrict__ cols,          // 3 per face slot (CSR payload)
    SimpPlane *__restrict__ fq,           // per face (round scratch)
    uint32_t *__restrict__ nt_cur,
    const uint32_t *__restrict__ target,
    uint8_t *__restrict__ active,
    uint32_t *__restrict__ park_faces,
    unsigned long long *__restrict__ prof,  // 6 phase counters or null
    uint32_t *__restrict__ roundhist,  // 160 u32 or null (see host)
    float max_cost, uint32_t nlabels, uint32_t big_cap,
    uint32_t subs, uint32_t nv_lo, uint32_t nv_hi,
    uint32_t *__restrict__ accept_g,  // per-vertex (wave 2)
    uint32_t propose) {
  constexpr int BS = SIMP_LABEL_BS;
  const uint32_t b = blockIdx.x;  // one workgroup per label
  if (b >= nlabels) return;
  unsigned long long t_start =
      roundhist ? __builtin_amdgcn_s_memtime() : 0;
  const uint32_t f0 = tri_off[b];
  const uint32_t nt0 = tri_off[b + 1] - f0;
  if (nt0 > big_cap) return;  // global-rounds path handles big labels
  const uint32_t v0 = vbase[b];
  const uint32_t nv = vbase[b + 1] - v0;
  // size-class dispatch: each launch owns an (nv_lo, nv_hi] band
  if (nv <= nv_lo || nv > nv_hi) return;
  if (!active[b]) {
    // already at/below target: final faces = original faces; park them
    for (uint32_t i = threadIdx.x; i < 3 * nt0; i += BS)
      park_faces[3ull * f0 + i] = faces_g[3ull * f0 + i];
    return;
  }
  const uint32_t tgt = target[b];
  const uint32_t tid = threadIdx.x;
  uint32_t *faces = faces_g + 3ull * f0;
  uint32_t *ftmp = faces_tmp + 3ull * f0;
  SimpPlane *pl = fq + f0;
  uint32_t *aoff = adj_off + v0;
  uint32_t *cl = cols + 3ull * f0;

  __shared__ uint32_t s_sums[BS / 64];  // wave totals for blk_prefix
  __shared__ uint32_t s_nt, s_collapses;
  // the two ATOMIC-hot per-vertex arrays live in LDS when the label fits:
  // neighboring faces' vertices share cache lines, so the global
  // atomicAdd/atomicMin streams serialize on hot L2 lines — LDS atomics
  // are bank-parallel. (~25 KB -> ~6 blocks/CU.)
  __shared__ uint32_t s_deg[CAPV];
  __shared__ unsigned long long s_pick[CAPV];
  // remap holds label-LOCAL canonical ids; LDS-resident when the label
  // fits (rewrite's 3 gathers/face are the hot readers)
  __shared__ uint32_t s_remap[CAPV];
  const bool lds_mode = (nv <= (uint32_t)CAPV);
  uint32_t *dg = lds_mode ? s_deg : (deg + v0);
  unsigned long long *pick_l =
      lds_mode ? s_pick : (pick + v0);
  uint32_t *rm = lds_mode ? s_remap : (remap + v0);
  // accept table (proposal wave): u32 id-only keys — lives in the
  // degree array's bytes (dead during the collapse phases) when the
  // label is LDS-resident; global fallback otherwise
  uint32_t *accept_l = lds_mode ? s_deg : (accept_g + v0);
  // ping-pong face buffers: rewrite reads fa, compaction scatters into
  // fb, then the buffers swap — no copy-back pass. Parking at the end
  // reads whichever buffer is current.
  uint32_t *fa = faces, *fb = ftmp;
  if (tid == 0) s_nt = nt0;
  __syncthreads();

  // env-gated phase profiling (thread 0 wall cycles per phase)
  unsigned long long ph[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long t_last = prof ? __builtin_amdgcn_s_memtime() : 0;
#define PHASE_MARK(k)                                          \
  if (prof && tid == 0) {                                      \
    unsigned long long now = __builtin_amdgcn_s_memtime();     \
    ph[k] += now - t_last;                                     \
    t_last = now;                                              \
  }

  uint32_t n_groups = 0, n_subs = 0;
  for (int round = 0; round < 65536; ++round) {
    uint32_t nt = s_nt;
    if (nt <= tgt) break;
    ++n_groups;
    const uint32_t nt_group = nt;  // group-progress watermark
    PHASE_MARK(0)  // loop head

    // [1+2] face planes fused with the CSR degree count (one face pass)
    for (uint32_t v = tid; v < nv; v += BS) dg[v] = 0;
    __syncthreads();
    for (uint32_t f = tid; f < nt; f += BS) {
      uint32_t i0 = fa[3*f], i1 = fa[3*f+1], i2 = fa[3*f+2];
      atomicAdd(&dg[i0 - v0], 1u);
      atomicAdd(&dg[i1 - v0], 1u);
      atomicAdd(&dg[i2 - v0], 1u);
      pl[f] = sq_face_plane(verts, i0, i1, i2);
    }
    __syncthreads();
    PHASE_MARK(1)  // planes + degree count
    // [3] offsets; the scan also writes the fill cursors (dst2 = dg)
    blk_exscan<BS>(dg, aoff, nv, 0, s_sums, dg);
    for (uint32_t f = tid; f < nt; f += BS) {
      cl[atomicAdd(&dg[fa[3*f] - v0], 1u)] = f;
      cl[atomicAdd(&dg[fa[3*f+1] - v0], 1u)] = f;
      cl[atomicAdd(&dg[fa[3*f+2] - v0], 1u)] = f;
    }
    __syncthreads();
    PHASE_MARK(2)  // offsets scan + CSR fill
    // [5] per-vertex: sort incident faces ascending (insertion sort),
    // accumulate quadrics in that order (oracle step 1)
    for (uint32_t v = tid; v < nv; v += BS) {
      uint32_t lo = aoff[v];
      uint32_t hi = dg[v];  // cursor ended at one-past-last
      uint32_t d = hi - lo;
      float q[10];
      #pragma unroll
      for (int k = 0; k < 10; ++k) q[k] = 0.0f;
      if (d <= 8) {
        // dominant tier: interior vertices have degree ~6 — the 8-wide
        // network + 8 plane gathers costs ~1/3 of the 16-wide one
        sq_sort_accum<8>(q, cl + lo, d, pl);
      } else if (d <= 16) {
        sq_sort_accum<16>(q, cl + lo, d, pl);
      } else {
        // rare high-degree vertex: the oracle's insertion sort in place
        for (uint32_t i = lo + 1; i < hi; ++i) {
          uint32_t x = cl[i];
          uint32_t j = i;
          while (j > lo && cl[j-1] > x) { cl[j] = cl[j-1]; --j; }
          cl[j] = x;
        }
        for (uint32_t i = lo; i < hi; ++i) {
          SimpPlane p = pl[cl[i]];
          sq_add_plane(q, p.nx, p.ny, p.nz, p.d, 1.0f);
        }
      }
      {  // 12-float row (2 pad zeros), 3 dwordx4 stores
        float4 *qo = (float4 *)(Q + 12ull*(v0+v));
        qo[0] = make_float4(q[0], q[1], q[2], q[3]);
        qo[1] = make_float4(q[4], q[5], q[6], q[7]);
        qo[2] = make_float4(q[8], q[9], 0.0f, 0.0f);
      }
      // fused reset (same-thread slots; dg's last read was above)
      simp_reset_vertex(pick_l, rm, accept_l, v, propose);
    }
    __syncthreads();
    PHASE_MARK(3)  // sort + quadric accumulate
    // sub-rounds: reuse merged quadrics (Q[u] += Q[w] on collapse) for
    // up to `subs` pick/collapse/compact passes per recompute (oracle
    // group structure; a full recompute resets the drift)
    for (uint32_t sub = 0; sub < subs; ++sub) {
    nt = s_nt;
    if (nt <= tgt) break;
    ++n_subs;
    if (sub > 0) {
      for (uint32_t v = tid; v < nv; v += BS)
        simp_reset_vertex(pick_l, rm, accept_l, v, propose);
      __syncthreads();
    }
    // [6] picks (oracle step 2)
    for (uint32_t f = tid; f < nt; f += BS) {
      uint32_t fc[3] = {fa[3*f], fa[3*f+1], fa[3*f+2]};
      float cq[3][10], cp[3][3];
      sq_stage_corners(fc, verts, Q, cq, cp);
      sq_edge_bids(fc, cq, cp, pick_l, v0, v0, max_cost);
    }
    PHASE_MARK(4)  // edge picks
    // [7] matched-pair collapse (oracle step 3); rm was pre-set to the
    // identity in the same pass that reset the pick table
    if (tid == 0) s_collapses = 0;
    __syncthreads();
    for (uint32_t v = tid; v < nv; v += BS) {
      uint32_t u = v0 + v;
      unsigned long long pu = pick_l[v];
      if (pu == ~0ull) continue;
      uint32_t w = (uint32_t)pu;
      if (w <= u) continue;
      unsigned long long pw = pick_l[w - v0];
      if (pw == ~0ull || (uint32_t)pw != u) continue;
      sq_collapse(verts, Q, u, w);
      rm[w - v0] = u - v0;
      // blocked marking: matched vertices leave the pick graph (the
      // races on these plain stores are benign: any reader's decision
      // is identical for the old and the cleared value — DESIGN §2)
      pick_l[v] = ~0ull;
      pick_l[w - v0] = ~0ull;
      atomicAdd(&s_collapses, 1u);
    }
    __syncthreads();
    // [7b] proposal-acceptance second wave (oracle step 3b): mutual
    // picks converge on cost-minima stars, so unmatched vertices whose
    // pick points UP propose to that peer; an unmatched non-proposing
    // peer accepts its minimum (costbits, local proposer+1) proposal.
    if (propose) {
      for (uint32_t v = tid; v < nv; v += BS) {
        unsigned long long pu = pick_l[v];
        if (pu == ~0ull) continue;
        uint32_t w = (uint32_t)pu;
        if (w <= v0 + v) continue;            // propose-up only
        if (pick_l[w - v0] == ~0ull) continue;  // blocked target
        atomicMin(&accept_l[w - v0], v + 1);
      }
      __syncthreads();
      for (uint32_t v = tid; v < nv; v += BS) {
        uint32_t aw = accept_l[v];
        if (aw == 0xFFFFFFFFu) continue;
        unsigned long long pw = pick_l[v];
        if (pw == ~0ull) continue;            // matched or pickless
        uint32_t w = v0 + v;
        if ((uint32_t)pw > w) continue;       // proposers never accept
        uint32_t ul = aw - 1;
        uint32_t u = v0 + ul;
        sq_collapse(verts, Q, u, w);
        rm[v] = ul;
        atomicAdd(&s_collapses, 1u);
      }
      __syncthreads();
    }
    if (s_collapses == 0) break;
    // [8] fused rewrite + stable compact (oracle step 4)
    uint32_t kept = blk_rewrite_compact<BS>(fa, fb, rm, v0, nt, s_sums);
    { uint32_t *t = fa; fa = fb; fb = t; }  // compacted faces now in fa
    if (tid == 0) s_nt = kept;
    __syncthreads();
    PHASE_MARK(5)  // collapse + rewrite + compact
    if (kept == nt) break;  // no face dropped this sub
    }  // sub loop
    if (s_nt == nt_group) break;  // group made no progress: terminate
  }
#undef PHASE_MARK
  if (prof && tid == 0) {
    #pragma unroll
    for (int k = 0; k < 6; ++k)
      if (ph[k]) atomicAdd(&prof[k], ph[k]);
  }
  // park the final faces at the label's original offset
  for (uint32_t i = tid; i < 3 * s_nt; i += BS)
    park_faces[3ull * f0 + i] = fa[i];
  if (tid == 0) {
    nt_cur[b] = s_nt;
    active[b] = 0;  // done: global rounds skip this label
    if (roundhist) {
      // layout: [0..63] group-count hist, [64..127] sub-count hist
      // (capped), [128] sum groups, [129] sum subs, [130] labels seen,
      // [131] sum nt0 (faces entering), [132] max label cycles,
      // [133] nt0 of (a) max-cycle label, [134..159] log2 cycle hist
      unsigned long long cyc = __builtin_amdgcn_s_memtime() - t_start;
      uint32_t ck = (uint32_t)(cyc > 0xFFFFFFFFull ? 0xFFFFFFFFull : cyc);
      uint32_t prev = atomicMax(&roundhist[132], ck);
      if (ck > prev) roundhist[133] = nt0;  // racy but indicative
      int lg = 32 - __clz(ck | 1);          // 1..32
      atomicAdd(&roundhist[134 + (lg < 26 ? lg : 25)], 1u);
      // cycle totals split by LDS vs global-array mode ([160..163] u64x2,
      // [164] lds count, [165] global count — buffer is 176 u32)
      atomicAdd((unsigned long long *)&roundhist[lds_mode ? 160 : 162],
                cyc);
      atomicAdd(&roundhist[164 + (lds_mode ? 0 : 1)], 1u);
      atomicAdd(&roundhist[n_groups < 64 ? n_groups : 63], 1u);
      atomicAdd(&roundhist[64 + (n_subs < 64 ? n_subs : 63)], 1u);
      atomicAdd(&roundhist[128], n_groups);
      atomicAdd(&roundhist[129], n_subs);
      atomicAdd(&roundhist[130], 1u);
      atomicAdd(&roundhist[131], nt0);
    }
  }
}

// ---------------------------------------------------------------------------
// host driver of the kernels above; mirrors oracle/simplify.c round for
// round.

#define SIMP_BLK 256

static inline uint32_t simp_blocks(uint64_t n) {
  return (uint32_t)((n + SIMP_BLK - 1) / SIMP_BLK);
}

// Environment switches of the simplifier, read once per call.
struct SimpEnv {
  uint32_t propose;  // MG_SIMP_PROPOSE=0 disables the proposal-acceptance
                     // second matching wave (contract knob shared with
                     // the oracle, which reads the same variable)
  uint32_t subs;     // MG_SIMP_SUBS: sub-rounds per quadric recompute in
                     // the per-label kernel (contract constant, default 6
                     // on both sides)
  bool prof;         // MG_SIMP_PROF: per-phase cycle counters to stderr
  bool roundhist;    // MG_SIMP_ROUNDHIST: round-count histograms to stderr
};

static SimpEnv read_simp_env() {
  SimpEnv env = {1u, 6u, false, false};
  const char *e = getenv("MG_SIMP_PROPOSE");
  if (e && e[0] == '0') env.propose = 0;
  e = getenv("MG_SIMP_SUBS");
  if (e && e[0]) { int v = atoi(e); env.subs = v < 1 ? 1u : (uint32_t)v; }
  env.prof = getenv("MG_SIMP_PROF") != nullptr;
  env.roundhist = getenv("MG_SIMP_ROUNDHIST") != nullptr;
  return env;
}

// Per-call values of one run_simplify.
struct SimpCall {
  SimpEnv env;
  uint64_t L, V;     // labels, vertices (V is fixed until the final compact)
  float max_cost;
  // c->simp_meta: [0,L) nt_cur | [L,2L) target | [2L,3L) nt_new |
  //               3L..: active u8[L] | any u32 (aligned)
  uint32_t *nt_cur, *target, *nt_new;
  uint8_t *active;
  uint32_t *d_any;
  unsigned long long *d_prof;  // 6 phase counters, or null
  uint32_t *d_rh;              // round histogram (176 u32), or null
};

static int simp_alloc(mg_ctx *c, SimpCall &k, uint64_t T) {
  const uint64_t L = k.L, V = k.V;
  const uint64_t active_words = (L + 3) / 4;  // u8[L], padded to a word
  if (ensure(c, c->simp_meta, 3 * L + active_words + 1)) return 40;
  k.nt_cur = c->simp_meta.get();
  k.target = k.nt_cur + L;
  k.nt_new = k.target + L;
  k.active = reinterpret_cast<uint8_t *>(k.nt_new + L);
  k.d_any = k.nt_new + L + active_words;
  if (ensure(c, c->simp_flab, T)) return 40;
  if (ensure(c, c->simp_flab_alt, T)) return 40;
  if (ensure(c, c->simp_faces_alt, 3 * T)) return 40;
  if (ensure(c, c->simp_fq, T)) return 40;
  if (ensure(c, c->simp_valid, T)) return 40;
  if (ensure(c, c->simp_pk, 3 * T)) return 40;
  if (ensure(c, c->simp_pk_alt, 3 * T)) return 40;
  if (ensure(c, c->simp_pv, 3 * T)) return 40;
  if (ensure(c, c->simp_pv_alt, 3 * T)) return 40;
  if (ensure(c, c->simp_Q, 12 * V)) return 40;  // 12-float rows
  if (ensure(c, c->simp_pick, V)) return 40;
  if (ensure(c, c->simp_remap, V)) return 40;
  if (ensure(c, c->simp_keep, T)) return 40;
  if (ensure(c, c->simp_keep_scan, T)) return 40;
  if (ensure(c, c->simp_park, 3 * T)) return 40;
  if (ensure(c, c->simp_first, L + 1)) return 40;
  if (ensure(c, c->simp_troff_final, L + 1)) return 40;
  if (ensure(c, c->simp_deg, V)) return 40;
  if (ensure(c, c->simp_adj, V)) return 40;
  if (ensure(c, c->simp_accept, V)) return 40;
  return 0;
}

// MG_SIMP_PROF / MG_SIMP_ROUNDHIST printouts of the per-label launch
static int simp_print_diagnostics(mg_ctx *c, const SimpCall &k) {
  hipStream_t s = c->stream;
  if (k.d_prof) {
    unsigned long long hp[6];
    HIP_TRY(c, hipMemcpyAsync(hp, k.d_prof, 48, hipMemcpyDeviceToHost, s),
            40);
    HIP_TRY(c, hipStreamSynchronize(s), 40);
    const char *nm[6] = {"loophead", "planes+deg", "scan+fill",
                         "sortaccum", "picks", "collapse+compact"};
    fprintf(stderr, "[mg simp phases, summed tid0 cycles]");
    for (int i = 0; i < 6; ++i) fprintf(stderr, " %s=%llu", nm[i], hp[i]);
    fprintf(stderr, "\n");
  }
  if (k.d_rh) {
    uint32_t h[176];
    HIP_TRY(c, hipMemcpyAsync(h, k.d_rh, 176 * 4, hipMemcpyDeviceToHost, s),
            40);
    HIP_TRY(c, hipStreamSynchronize(s), 40);
    fprintf(stderr, "[mg simp rounds] labels=%u sum_groups=%u "
            "sum_subs=%u sum_nt0=%u max_cycles=%u (nt0=%u)\n",
            h[130], h[128], h[129], h[131], h[132], h[133]);
    unsigned long long lds_c, glob_c;
    memcpy(&lds_c, &h[160], 8);
    memcpy(&glob_c, &h[162], 8);
    fprintf(stderr, "[mg simp mode split] lds: n=%u cyc=%llu | "
            "global: n=%u cyc=%llu\n", h[164], lds_c, h[165], glob_c);
    fprintf(stderr, "[mg simp log2-cycle hist]");
    for (int i = 0; i < 26; ++i)
      if (h[134 + i]) fprintf(stderr, " %d:%u", i, h[134 + i]);
    fprintf(stderr, "\n[mg simp group hist]");
    for (int i = 0; i < 64; ++i)
      if (h[i]) fprintf(stderr, " %d:%u", i, h[i]);
    fprintf(stderr, "\n[mg simp subs hist]");
    for (int i = 0; i < 64; ++i)
      if (h[64 + i]) fprintf(stderr, " %d:%u", i, h[64 + i]);
    fprintf(stderr, "\n");
  }
  return 0;
}

// The per-label kernel, one workgroup per label, in three nv bands:
//   nv <= 2048          CAPV=2048 on the main stream
//   2048 < nv <= 4096   CAPV=4096 (64 KB LDS, 2 blocks/CU) on stream2 —
//                       these used to fall into the global-array mode
//                       whose hot per-vertex atomics serialize on L2 lines
//   nv > 4096           CAPV=2048 (global-array mode) on stream2
// stream2's bands run concurrently with the main band.
static int simp_launch_labels(mg_ctx *c, const SimpCall &k) {
  hipStream_t s = c->stream;
  auto launch_band = [&](auto fn, hipStream_t st, uint32_t nv_lo,
                         uint32_t nv_hi) {
    hipLaunchKernelGGL(fn, dim3((uint32_t)k.L), dim3(SIMP_LABEL_BS), 0,
                       st, c->faces.get(), c->simp_faces_alt.get(),
                       c->tri_off.get(), c->vbase.get(), c->verts.get(),
                       c->simp_Q.get(), c->simp_pick.get(),
                       c->simp_remap.get(), c->simp_deg.get(),
                       c->simp_adj.get(), c->simp_pk.get(),
                       c->simp_fq.get(), k.nt_cur, k.target, k.active,
                       c->simp_park.get(), k.d_prof, k.d_rh,
                       k.max_cost, (uint32_t)k.L, SIMP_BIG_CAP, k.env.subs,
                       nv_lo, nv_hi, c->simp_accept.get(), k.env.propose);
  };
  // record BEFORE enqueuing the main band: stream2 must wait only for the
  // shared setup, so its bands run CONCURRENT with the main one
  // (recording after it serialized them — 51 ms vs 38 ms overlapped)
  HIP_TRY(c, hipEventRecord(c->ev[EV_SIMP_FORK], s), 40);
  HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev[EV_SIMP_FORK], 0), 40);
  launch_band(k_simplify_label<2048>, s, 0u, 2048u);
  launch_band(k_simplify_label<4096>, c->stream2, 2048u, 4096u);
  launch_band(k_simplify_label<2048>, c->stream2, 4096u, 0xFFFFFFFFu);
  HIP_TRY(c, hipEventRecord(c->ev[EV_SIMP_JOIN], c->stream2), 40);
  HIP_TRY(c, hipStreamWaitEvent(s, c->ev[EV_SIMP_JOIN], 0), 40);
  HIP_TRY(c, hipGetLastError(), 40);
  return simp_print_diagnostics(c, k);
}

// Park the faces of labels that are not active: flag the faces of active
// labels, scan, scatter the others into the park store (simp_park) and
// compact the flagged ones into the alt face/label arrays.
//   p_T != null: read the surviving count back into *p_T and make the alt
//                arrays current (a sync point);
//   p_T == null: the force-park — nothing survives, nothing is swapped.
static int park_inactive(mg_ctx *c, const SimpCall &k, uint64_t T,
                         const char *err_size, const char *err_run, int rc,
                         uint64_t *p_T) {
  hipStream_t s = c->stream;
  const dim3 nb(simp_blocks(T)), blk(SIMP_BLK);
  uint32_t *faces_g = c->faces.get();
  uint32_t *flab = c->simp_flab.get();
  uint32_t *keep = c->simp_keep.get();
  uint32_t *keep_scan = c->simp_keep_scan.get();
  hipLaunchKernelGGL(k_flag_active_faces, nb, blk, 0, s, flab, k.active,
                     keep, T);
  if (int e = scan_u32(c, keep, keep_scan, T, s, err_size, err_run, rc))
    return e;
  hipLaunchKernelGGL(k_first_label_idx, nb, blk, 0, s, flab,
                     c->simp_first.get(), T);
  hipLaunchKernelGGL(k_park_scatter, nb, blk, 0, s, faces_g, flab, keep,
                     keep_scan, c->simp_first.get(), c->tri_off.get(),
                     c->simp_faces_alt.get(), c->simp_flab_alt.get(),
                     c->simp_park.get(), SIMP_BIG_CAP, T);
  if (!p_T) {
    HIP_TRY(c, hipGetLastError(), rc);
    return 0;
  }
  uint32_t *d_total = &c->scalars->simp_kept;
  hipLaunchKernelGGL(k_last_sum, dim3(1), dim3(1), 0, s, keep_scan, keep, T,
                     d_total);
  uint32_t act_total = 0;
  HIP_TRY(c, hipMemcpyAsync(&act_total, d_total, 4, hipMemcpyDeviceToHost,
                            s), rc);
  HIP_TRY(c, hipStreamSynchronize(s), rc);
  std::swap(c->faces, c->simp_faces_alt);
  std::swap(c->simp_flab, c->simp_flab_alt);
  *p_T = act_total;
  return 0;
}

// One round of the global (big-label) path over the T working faces:
// quadrics, matched-pair collapse, compaction, then parking of the labels
// that just went inactive. *p_done is set when no label is active any
// more or no face survives the compaction.
//
// One collapse pass per quadric recompute: the same group structure as
// the per-label kernel and the oracle, but measured on 512^3/200 big
// labels sub-rounds > 1 are ~5% SLOWER here (the T- and V-sized sub
// passes dwarf the recompute they skip, unlike the per-label kernel), so
// the contract pins big labels at 1 sub/group — hence k_update_active's
// constant 1u.
static int simp_global_round(mg_ctx *c, const SimpCall &k, uint64_t *p_T,
                             bool *p_done) {
  hipStream_t s = c->stream;
  const dim3 blk(SIMP_BLK), nbl((uint32_t)((k.L + 255) / 256));
  const uint64_t T = *p_T, V = k.V;
  // any label still active?
  HIP_TRY(c, hipMemsetAsync(k.d_any, 0, 4, s), 41);
  hipLaunchKernelGGL(k_any_active, nbl, dim3(256), 0, s, k.active,
                     (uint32_t)k.L, k.d_any);
  uint32_t any = 0;
  HIP_TRY(c, hipMemcpyAsync(&any, k.d_any, 4, hipMemcpyDeviceToHost, s), 41);
  HIP_TRY(c, hipStreamSynchronize(s), 41);
  if (!any) {
    *p_done = true;
    return 0;
  }

  const dim3 nbt(simp_blocks(T)), nbv(simp_blocks(V));
  const uint64_t NP = 3 * T;
  uint32_t *faces_g = c->faces.get();
  float *verts = c->verts.get();
  uint32_t *flab = c->simp_flab.get();
  unsigned long long *pick = c->simp_pick.get();
  uint32_t *remap = c->simp_remap.get();
  uint32_t *accept = c->simp_accept.get();
  uint32_t *keep = c->simp_keep.get();
  uint32_t *keep_scan = c->simp_keep_scan.get();
  float *Q = c->simp_Q.get();

  hipLaunchKernelGGL(k_face_planes, nbt, blk, 0, s, faces_g, verts, k.active,
                     flab, c->simp_fq.get(), c->simp_valid.get(), T);
  hipLaunchKernelGGL(k_emit_vf_pairs, nbt, blk, 0, s, faces_g, k.active, flab,
                     c->simp_pk.get(), c->simp_pv.get(), T);
  // stable sort pairs by vertex (face order preserved within vertex)
  {
    rocprim::double_buffer<uint32_t> dk(c->simp_pk.get(),
                                        c->simp_pk_alt.get());
    rocprim::double_buffer<uint32_t> dv(c->simp_pv.get(),
                                        c->simp_pv_alt.get());
    if (int e = sort_pairs(c, dk, dv, NP, 0u, 32u, s,
                           "simplify sort size query", "simplify sort", 42))
      return e;
    hipLaunchKernelGGL(k_accum_quadrics, dim3(simp_blocks(NP)), blk, 0, s,
                       dk.current(), dv.current(), c->simp_fq.get(),
                       c->simp_valid.get(), Q, NP);
  }
  HIP_TRY(c, hipMemsetAsync(pick, 0xFF, V * 8, s), 43);
  if (k.env.propose) HIP_TRY(c, hipMemsetAsync(accept, 0xFF, V * 4, s), 43);
  hipLaunchKernelGGL(k_edge_pick, nbt, blk, 0, s, faces_g, k.active, flab,
                     c->vbase.get(), verts, Q, pick, k.max_cost, T);
  hipLaunchKernelGGL(k_iota, nbv, blk, 0, s, remap, V);
  hipLaunchKernelGGL(k_collapse, nbv, blk, 0, s, pick, verts, remap, Q, V);
  if (k.env.propose) {
    hipLaunchKernelGGL(k_propose, nbv, blk, 0, s, pick, accept, V);
    hipLaunchKernelGGL(k_accept, nbv, blk, 0, s, pick, accept, verts, remap,
                       Q, V);
  }
  hipLaunchKernelGGL(k_remap_faces, nbt, blk, 0, s, faces_g, remap, keep, T);
  if (int e = scan_u32(c, keep, keep_scan, T, s, "keep scan size query",
                       "keep scan", 44))
    return e;
  uint32_t *d_kept = &c->scalars->simp_kept;
  hipLaunchKernelGGL(k_last_sum, dim3(1), dim3(1), 0, s, keep_scan, keep, T,
                     d_kept);
  uint32_t kept = 0;
  HIP_TRY(c, hipMemcpyAsync(&kept, d_kept, 4, hipMemcpyDeviceToHost, s), 44);
  HIP_TRY(c, hipMemsetAsync(k.nt_new, 0, k.L * 4, s), 44);
  hipLaunchKernelGGL(k_compact_faces, nbt, blk, 0, s, faces_g, flab, keep,
                     keep_scan, c->simp_faces_alt.get(),
                     c->simp_flab_alt.get(), k.nt_new, T);
  hipLaunchKernelGGL(k_update_active, nbl, dim3(256), 0, s, k.nt_new,
                     k.nt_cur, k.target, k.active, k.d_any, (uint32_t)k.L,
                     1u);
  HIP_TRY(c, hipGetLastError(), 44);
  HIP_TRY(c, hipStreamSynchronize(s), 44);
  std::swap(c->faces, c->simp_faces_alt);
  std::swap(c->simp_flab, c->simp_flab_alt);
  *p_T = kept;
  if (kept == 0) {
    *p_done = true;
    return 0;
  }
  // park faces of labels that just went inactive: working set keeps
  // only active labels (late rounds touch only the active tail)
  return park_inactive(c, k, kept, "park scan size query", "park scan", 47,
                       p_T);
}

// Final face array (per-label slices gathered from the park store in
// label-id order), then drop unreferenced vertices (stable) and
// re-localize the faces. *p_T / *p_V = the final totals.
static int simp_finalize(mg_ctx *c, const SimpCall &k, uint64_t *p_T,
                         uint64_t *p_V) {
  hipStream_t s = c->stream;
  const dim3 blk(SIMP_BLK);
  const uint64_t L = k.L, V = k.V;
  uint32_t *troff_final = c->simp_troff_final.get();
  if (int e = scan_u32(c, k.nt_cur, troff_final, L, s,
                       "final troff scan size", "final troff scan", 49))
    return e;
  uint32_t *d_total = &c->scalars->simp_final_tris;
  hipLaunchKernelGGL(k_last_sum, dim3(1), dim3(1), 0, s, troff_final,
                     k.nt_cur, L, d_total);
  HIP_TRY(c, hipMemcpyAsync(troff_final + L, d_total, 4,
                            hipMemcpyDeviceToDevice, s), 49);
  uint32_t final_total = 0;
  HIP_TRY(c, hipMemcpyAsync(&final_total, d_total, 4, hipMemcpyDeviceToHost,
                            s), 49);
  HIP_TRY(c, hipStreamSynchronize(s), 49);
  const uint64_t T = final_total;
  if (T > 0)
    hipLaunchKernelGGL(k_gather_final, dim3(simp_blocks(T)), blk, 0, s,
                       c->simp_park.get(), c->tri_off.get(), troff_final,
                       c->faces.get(), c->simp_flab.get(), (uint32_t)L, T);
  uint32_t *faces_g = c->faces.get();
  std::swap(c->tri_off, c->simp_troff_final);

  if (ensure(c, c->simp_ref, V + 1)) return 45;
  if (ensure(c, c->simp_verts_alt, 3 * V + 3)) return 45;
  if (ensure(c, c->simp_vbase_alt, L + 1)) return 45;
  uint32_t *ref = c->simp_ref.get();
  // V words, sized by the caller (run_weld, mg_simplify_mesh)
  uint32_t *newid = c->vtx_scan.get();
  HIP_TRY(c, hipMemsetAsync(ref, 0, V * 4, s), 45);
  if (T > 0)
    hipLaunchKernelGGL(k_mark_ref, dim3(simp_blocks(3 * T)), blk, 0, s,
                       faces_g, ref, 3 * T);
  if (int e = scan_u32(c, ref, newid, V, s, "ref scan size query",
                       "ref scan", 45))
    return e;
  uint32_t *d_newV = &c->scalars->simp_new_verts;
  hipLaunchKernelGGL(k_last_sum, dim3(1), dim3(1), 0, s, newid, ref, V,
                     d_newV);
  uint32_t newV = 0;
  HIP_TRY(c, hipMemcpyAsync(&newV, d_newV, 4, hipMemcpyDeviceToHost, s), 45);
  HIP_TRY(c, hipStreamSynchronize(s), 45);
  hipLaunchKernelGGL(k_scatter_verts, dim3(simp_blocks(V)), blk, 0, s,
                     c->verts.get(), ref, newid, c->simp_verts_alt.get(), V);
  hipLaunchKernelGGL(k_new_vbase, dim3((uint32_t)((L + 2 + 255) / 256)),
                     dim3(256), 0, s, c->vbase.get(), newid,
                     c->simp_vbase_alt.get(), (uint32_t)L, newV);
  if (T > 0)
    hipLaunchKernelGGL(k_localize_faces, dim3(simp_blocks(T)), blk, 0, s,
                       faces_g, newid, c->simp_flab.get(),
                       c->simp_vbase_alt.get(), c->simp_faces_alt.get(), T);
  HIP_TRY(c, hipGetLastError(), 46);
  std::swap(c->faces, c->simp_faces_alt);
  std::swap(c->verts, c->simp_verts_alt);
  std::swap(c->vbase, c->simp_vbase_alt);
  *p_T = T;
  *p_V = newV;
  return 0;
}

// Simplify every label of the welded mesh in the ctx (faces / verts /
// vbase / tri_off, label per face in lab_sorted). Updates those buffers;
// p_T/p_V become the post-simplification totals.
static int run_simplify(mg_ctx *c, uint32_t nlabels,
                        const uint32_t *lab_sorted,
                        uint32_t reduction_factor, float max_error,
                        uint64_t *p_T, uint64_t *p_V) {
  hipStream_t s = c->stream;
  uint64_t T = *p_T;
  if (T == 0 || *p_V == 0) return 0;
  SimpCall k = {};
  k.env = read_simp_env();
  k.L = nlabels;
  k.V = *p_V;
  k.max_cost = max_error * max_error;
  if (int e = simp_alloc(c, k, T)) return e;

  // faces -> global vertex ids, label per face
  hipLaunchKernelGGL(k_globalize_faces, dim3(simp_blocks(T)), dim3(SIMP_BLK),
                     0, s, c->faces.get(), lab_sorted, c->vbase.get(),
                     c->simp_flab.get(), T);
  hipLaunchKernelGGL(k_init_simplify, dim3((uint32_t)((k.L + 255) / 256)),
                     dim3(256), 0, s, c->tri_off.get(), k.nt_cur, k.target,
                     k.active, reduction_factor, (uint32_t)k.L);
  HIP_TRY(c, hipGetLastError(), 40);

  if (k.env.prof) {
    k.d_prof = c->scalars->simp_prof;
    HIP_TRY(c, hipMemsetAsync(k.d_prof, 0, 48, s), 40);
  }
  if (k.env.roundhist) {  // groups/subs per label
    if (ensure(c, c->simp_rh, 176)) return 40;
    k.d_rh = c->simp_rh.get();
    HIP_TRY(c, hipMemsetAsync(k.d_rh, 0, 176 * 4, s), 40);
  }
  if (int e = simp_launch_labels(c, k)) return e;

  // drop the per-label-kernel labels from the working set; park big
  // never-active labels (their final faces are their originals)
  if (int e = park_inactive(c, k, T, "prepark scan size", "prepark scan", 50,
                            &T))
    return e;

  bool done = false;
  for (int group = 0; group < 65536 && !done; ++group)
    if (int e = simp_global_round(c, k, &T, &done)) return e;

  // any faces still in the working set (round-cap exit): force-park them
  if (T > 0) {
    HIP_TRY(c, hipMemsetAsync(k.active, 0, k.L, s), 48);
    if (int e = park_inactive(c, k, T, "force-park scan size query",
                              "force-park scan", 48, nullptr))
      return e;
  }
  if (int e = simp_finalize(c, k, &T, p_V)) return e;
  *p_T = T;
  return 0;
}
