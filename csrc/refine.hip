// Safety filter: test-time refinement of the actions on the discrete CBF condition, gfx950.
//
//   h      = h(s_t) on the kNN slots, fixed                       (precomputed, cbf_fwd)
//   s'     = s + dt [v, a + delta]   (agents; obstacle nodes are static)
//   deriv  = h(s') - h + dt alpha h  on the time-t slots
//   loss   = sum_e relu(-deriv_e),   delta <- delta - lr dloss/ddelta
//
// One iteration is two launches on one stream:
//   refine_grad_kernel    per 32-edge tile per wave: gather s_i, s_j, a + delta, form s', the CBF
//     forward chain + fp32 head (the recompute chain of cbf_bwd_kernel), the hinge choice, and
//     the data-path backward only (dH3 -> dH2 -> dH1 -> dF). No weight gradients, no LDS stage
//     images, no barrier after the weight copy. p' = p + dt v does not depend on delta, so only
//     the D velocity components of dL/d(s'_i - s'_j) can reach the action: dEv (B,N,K,D).
//   refine_update_kernel  one 16-lane group per agent: delta_i -= lr dt (sum_out dEv - sum_in dEv)
//     over the reverse CSR, fixed xor butterfly, no float atomics.
// Control words ctl[2 it] (edges with a non-zero hinge gradient) and ctl[2 it + 1] (violation sum,
// fixed point) are integer atomics: order independent, so the loop is reproducible bit for bit.
// Early-out on the device: a zero hinge has a zero gradient, so once an iteration counted no
// active edge every later launch returns at once and delta stays as it is.
// Per-env mask (env_active, optional): the edges of an env with 0 are "not in the tile" (no dEv,
// trace, count or violation term), a tile without a live edge skips the MFMA chain on a ballot
// (wave-uniform: tiles straddle envs whenever N*K is no multiple of 32), and the update leaves the
// env's delta at zero. The control words then count the other envs alone, so a batch stops when
// its live envs are clean, exactly as the filter run on those envs alone would.
// Actuator limit (a_max > 0, optional): `a` arrives clamped to the box [-a_max, a_max]^D and every
// update projects delta onto [-a_max - a, a_max - a] after the gradient step, behind one scalar test
// of the kernel argument (off: the instructions of the unlimited filter). The early-out rule is
// unchanged: a saturated agent can keep an edge active for all the iterations.
// Small envs (at most 64 graph nodes): refine_small_kernel runs the whole loop of an env in one
// workgroup and one launch, with the same per-tile body (refine_tile) and the same update
// (refine_node_grad, refine_step) on LDS copies, and per-env result words instead of atomics.
#pragma clang fp contract(off)
#include "common.h"
#include "args.h"
#include "launch.h"
#include "state.h"
#include "cbf_edge.h"
#include "combine.h"

// waves per workgroup: x3 4 (one per SIMD: the split activations double the register
// footprint), 1-pass 8 (two per SIMD) -- as the CBF backward
constexpr int REFINE_NW = MB_X3 ? 4 : 8;

namespace mb {
namespace MB_PREC {

// W2 | W3 row-major images, w1f (2 fragments) | w1ft (4 fragments), the side vector
constexpr size_t REFINE_W_BYTES = (size_t)RMP * 2 + 6 * FRAG_SZ;
constexpr size_t REFINE_LDS = REFINE_W_BYTES + CBF_VEC * 4;

template <int D>
struct RefIn {
  float rp[D], rv[D];   // s'_i - s'_j
  float hv;             // h(s_t) of the slot
  int i, j;
  bool in;
};

// One edge (i, slot) of an env from the env's own arrays (global memory in refine_grad_kernel, the
// LDS copies in refine_small_kernel): Sb the env's node records, ab / db its a / delta rows, jr the
// neighbour slot, hv = h(s_t). Every load is unconditional on a clamped index (idx holds node ids
// up to Nn - 1, a / delta have N rows: an obstacle neighbour reads row N - 1 and is zeroed). An edge
// that is not in the tile (`in` false: past the end, or of a masked-out env) loads like any other.
// LOCAL (the decentralised filter): a neighbour's next state is its nominal one, s_j + dt [v_j, a_j];
// only the self slot (j == i) carries the agent's own delta, so its relative state stays exactly zero.
template <int D, bool LOCAL = false>
DEV void refine_edge(const float4* Sb, const float* ab, const float* db, int jr, float hv, unsigned i, int N, int Nn,
                     float dt, bool in, RefIn<D>& x) {
  x.in = in;
  const unsigned j = (unsigned)min(max(jr, 0), Nn - 1);
  const bool agent_j = j < (unsigned)N;
  const unsigned ja = agent_j ? j : (unsigned)(N - 1);
  float pi[D], vi[D], pj[D], vj[D];
  load_rec<D>(Sb, i, pi, vi);
  load_rec<D>(Sb, j, pj, vj);
  const float* ai = ab + (size_t)i * D;
  const float* di = db + (size_t)i * D;
  const float* aj = ab + (size_t)ja * D;
  const float* dj = db + (size_t)ja * D;
  x.hv = hv;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    const float ui = ai[q] + di[q];
    float uj;
    if constexpr (LOCAL) uj = agent_j ? (j == i ? aj[q] + dj[q] : aj[q]) : 0.f;
    else uj = agent_j ? aj[q] + dj[q] : 0.f;
    // s' = s + [v, a + delta] * dt (the evaluation's own expression order)
    const float pin = pi[q] + vi[q] * dt, pjn = pj[q] + vj[q] * dt;
    const float vin = vi[q] + ui * dt, vjn = vj[q] + uj * dt;
    x.rp[q] = x.in ? pin - pjn : 0.f;
    x.rv[q] = x.in ? vin - vjn : 0.f;
  }
  x.i = (int)i;
  x.j = (int)j;
}

// Edge e = (b*N + i)*K + k of a batch-wide tile. An edge of a masked-out env is marked as not in the tile.
template <int D, bool LOCAL = false>
DEV void refine_load(const RefineArgs& a, unsigned tile, int r, unsigned E, RefIn<D>& x) {
  const unsigned e = tile * 32u + (unsigned)r;
  const bool inside = e < E;
  const unsigned ec = inside ? e : 0u;
  const unsigned ik = ec / (unsigned)a.K;
  const unsigned b = ik / (unsigned)a.N;
  const bool in = inside && (a.env_active ? a.env_active[b] != 0 : true);
  const unsigned i = ik - b * (unsigned)a.N;
  refine_edge<D, LOCAL>(a.S + (size_t)b * (size_t)a.s_env * REC<D>, a.a + (size_t)b * a.N * D,
                        a.delta + (size_t)b * a.N * D, a.idx[ec], a.h[ec], i, a.N, a.Nn, a.dt, in, x);
}

// The weight images in LDS (the same layout in both kernels), copied by the whole workgroup; the
// caller's barrier follows.
struct RefW {
  h16 *W2, *W3, *wf;                          // row-major W2 | W3, w1f (2 frags) | w1ft (4 frags)
  float* vl;                                  // the side vector
};
DEV RefW refine_weights(unsigned char* smem, const RefineArgs& a) {
  RefW w;
  w.W2 = reinterpret_cast<h16*>(smem);
  w.W3 = w.W2 + RM_W2;
  w.wf = w.W2 + RMP;
  w.vl = reinterpret_cast<float*>(smem + REFINE_W_BYTES);
  block_copy16(w.W2, a.wrm, RMP * 2, false);
  block_copy16(w.wf, a.wpack + (size_t)a.f_bwd * FRAG_ELEMS, 2 * FRAG_SZ, false);
  block_copy16(w.wf + 2 * FRAG_ELEMS, a.wpack + (size_t)(a.f_bwd + 66) * FRAG_ELEMS, 4 * FRAG_SZ, false);
  block_copy16(w.vl, a.wvec, CBF_VEC * 4);
  return w;
}

// What one 32-edge tile gives per edge (lanes h = 0 and h = 1 of an edge hold the same values)
template <int D>
struct RefOut {
  float hnv;            // radius-masked h(s')
  float deriv;          // h(s') - h + dt alpha h
  bool on;              // the hinge gradient is on
  float gv[D];          // velocity rows of dL/d(s'_i - s'_j), before the self-edge / inactive zeroing
};

// violation term relu(-deriv) in fixed point; NaN / Inf / out of range -> FX_SAT
DEV unsigned long long refine_viol_fx(float deriv) {
  const float v = deriv < 0.f ? -deriv : (deriv == deriv ? 0.f : __builtin_inff());
  const double xq = (double)v * FX_VIOL;
  return (xq >= 0.0 && xq < FX_SAT) ? (unsigned long long)__double2ll_rn(xq) : (unsigned long long)FX_SAT;
}

// The per-tile body of both kernels, one wave, every lane: forward chain, fp32 head, hinge choice
// and the data-path backward of the 32 edges in `cur`. Edges that are not in the tile (cur.in
// false) ride along as zeros -- no MFMA here is under a lane-divergent condition.
template <int D>
DEV void refine_tile(const RefIn<D>& cur, const RefW& w, const RefineArgs& a, int lane, int h, RefOut<D>& o) {
  const h16 *W2 = w.W2, *W3 = w.W3, *wf = w.wf;
  const float* vl = w.vl;
  const float eye = (cur.in && cur.j == cur.i) ? 1.f : 0.f;
  const float d = sqrtf(sqsum<D>(cur.rp) + a.dist_eps);
  const float dfeat = cur.in ? d - a.dist_thr : 0.f;
  const bool mask = cur.in && d <= a.obs_r;             // radius mask at s'
  const h16x8 F = cbf_edge_frag<D>(cur.rp, cur.rv, eye, dfeat, cur.in, h);
  const h16* wt = wf + opaque_zero();
  const h16* W2c = W2 + opaque_zero();
  const h16* W3c = W3 + opaque_zero();
  const float* vlc = vl + opaque_zero();
  const float* b2 = vlc;
  const float* b3 = vlc + 128;
  const float* w4 = vlc + 192;
  // ---- forward (the recompute chain of cbf_bwd_kernel / cbf_hfwd_kernel)
  Pk H1b[2], H2b[4];
  f32x16 H3p[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const f32x16 t1 = mma_bx(frag_fr(wt, mt, lane), F, zero16());
    H1b[mt] = to_pk_relu(t1);
  }
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    f32x16 t2 = bias_rows4(b2, 32 * mt, h);
    static_for<4>([&](auto kk_) {
      constexpr int kk = decltype(kk_)::value;
      t2 = mma(wrm_acc_fr(W2c, WS2, 32 * mt, kk, lane, RM_LO), pk_fr<kk & 1>(H1b[kk >> 1]), t2);
    });
    H2b[mt] = to_pk_relu(t2);
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    f32x16 t3 = bias_rows4(b3, 32 * mt, h);
    static_for<8>([&](auto kk_) {
      constexpr int kk = decltype(kk_)::value;
      t3 = mma(wrm_acc_fr(W3c, WS3, 32 * mt, kk, lane, RM_LO), pk_fr<kk & 1>(H2b[kk >> 1]), t3);
    });
    relu_(t3);                                   // relu(H3) in fp32 (the head is fp32)
    H3p[mt] = t3;
  }
  // ---- fp32 head, hinge choice
  f32x2 hs2 = {0.f, 0.f};
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 w = *reinterpret_cast<const float4*>(w4 + 32 * mt + 8 * g + 4 * h);
      hs2 = __builtin_elementwise_fma(f32x2{w.x, w.y}, f32x2{H3p[mt][4 * g], H3p[mt][4 * g + 1]}, hs2);
      hs2 = __builtin_elementwise_fma(f32x2{w.z, w.w}, f32x2{H3p[mt][4 * g + 2], H3p[mt][4 * g + 3]}, hs2);
    }
  float hs = hs2.x + hs2.y;
  hs += shfl_xor32(hs);
  const float hnv = mask ? hs + vlc[256] : 0.f;
  const float hv = cur.hv;
  const float deriv = hnv - hv + a.dt_alpha * hv;          // cbf_fwd_kernel's expression order
  // the hinge gradient is on where the condition is violated and h(s') is inside the radius
  // (outside it h(s') = 0 whatever the action)
  const bool on = mask && deriv < 0.f;
  const float dhv = on ? -1.f : 0.f;                       // d relu(-deriv) / d h(s')
  o.hnv = hnv;
  o.deriv = deriv;
  o.on = on;
  // ---- head backward: dH3pre = w4 * dh . relu'(H3)
  Pk d3b[2], H3b[2];
  const f32x2 dh2 = {dhv, dhv};
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    f32x16 d3;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 w = *reinterpret_cast<const float4*>(w4 + 32 * mt + 8 * g + 4 * h);
      const f32x2 lo = f32x2{w.x, w.y} * dh2, hi = f32x2{w.z, w.w} * dh2;
      d3[4 * g] = lo.x; d3[4 * g + 1] = lo.y; d3[4 * g + 2] = hi.x; d3[4 * g + 3] = hi.y;
    }
    H3b[mt] = to_pk(H3p[mt]);
    d3b[mt] = to_pk(d3);
    mask_pk(d3b[mt], H3b[mt]);
  }
  // ---- dH2pre = (W3^T dH3pre) . relu'(H2)
  Pk d2b[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    f32x16 t = zero16();
    static_for<4>([&](auto kk_) {
      constexpr int kk = decltype(kk_)::value;
      t = mma(wrmT_acc_fr(W3c, WS3, 32 * mt, kk, lane, RM_LO), pk_fr<kk & 1>(d3b[kk >> 1]), t);
    });
    d2b[mt] = to_pk(t);
    mask_pk(d2b[mt], H2b[mt]);
  }
  // ---- dH1pre = (W2^T dH2pre) . relu'(H1)
  Pk d1b[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    f32x16 t = zero16();
    static_for<8>([&](auto kk_) {
      constexpr int kk = decltype(kk_)::value;
      t = mma(wrmT_acc_fr(W2c, WS2, 32 * mt, kk, lane, RM_LO), pk_fr<kk & 1>(d2b[kk >> 1]), t);
    });
    d1b[mt] = to_pk(t);
    mask_pk(d1b[mt], H1b[mt]);
  }
  // ---- dF = W1^T dH1pre (rows: s_i - s_j (0..2D-1), eye, dist) -> velocity rows D..2D-1
  {
    f32x16 t = zero16();
    static_for<4>([&](auto kk_) {
      constexpr int kk = decltype(kk_)::value;
      t = mma(frag_fr(wt, 2 + kk, lane), pk_fr<kk & 1>(d1b[kk >> 1]), t);
    });
    // lane h = 0 holds rows 0..3 in regs 0..3, lane h = 1 rows 4..7
    float g4[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) { g4[q] = t[q]; g4[4 + q] = shfl_xor32(t[q]); }
#pragma unroll
    for (int q = 0; q < D; ++q) o.gv[q] = g4[D + q];
  }
}

// What lane h = 0 of an edge in the tile records: the violation term and the active count (per-lane
// integers), the optional trace at the batch-wide edge index et, and the edge's dEv record at dE.
template <int D>
DEV void refine_record(const RefIn<D>& cur, const RefOut<D>& o, float* hn_out, uint8_t* flag_out, size_t et, float* dE,
                       unsigned long long& nact, unsigned long long& vsum) {
  vsum += refine_viol_fx(o.deriv);
  nact += o.on ? 1ull : 0ull;
  if (hn_out) hn_out[et] = o.hnv;
  if (flag_out) flag_out[et] = o.on ? 1 : 0;
  // self edges: s'_i - s'_i = 0 whatever the action; inactive edges: exact zeros
  const bool wr = o.on && cur.j != cur.i;
#pragma unroll
  for (int q = 0; q < D; ++q) dE[q] = wr ? o.gv[q] : 0.f;
}

template <int NW, int D>
__global__ __launch_bounds__(NW * 64, 1) void refine_grad_kernel(RefineArgs a) {
  // early-out: the previous iteration had no active edge -> nothing can change any more (this
  // iteration's control words stay zero, which stops the next one)
  if (a.it > 0 && a.ctl[2 * (a.it - 1)] == 0ull) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const RefW w = refine_weights(smem, a);
  __syncthreads();
  const int wave = wave_id(), lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const unsigned E = (unsigned)a.B * a.N * a.K;
  const unsigned ntiles = (E + 31u) / 32u;
  const unsigned stride = gridDim.x * NW;
  unsigned long long nact = 0, vsum = 0;
  unsigned tile = (unsigned)blockIdx.x * NW + wave;
  RefIn<D> nx;
  refine_load<D>(a, tile, r, E, nx);
  for (; tile < ntiles; tile += stride) {
    const RefIn<D> cur = nx;
    refine_load<D>(a, tile + stride, r, E, nx);          // prefetch (clamped past the end)
    // no live edge (every env of the tile masked out): nothing to evaluate. One scalar branch on
    // the ballot for the whole wave -- no MFMA below runs under a lane-divergent condition.
    if (__ballot(cur.in) == 0ull) continue;
    RefOut<D> o;
    refine_tile<D>(cur, w, a, lane, h, o);
    if (cur.in && h == 0) {
      const size_t e = tile * 32u + (unsigned)r;
      refine_record<D>(cur, o, a.hn_out, a.flag_out, e, a.dEv + e * D, nact, vsum);
    }
  }
  const unsigned long long n = wave_sum_u64(nact), s = wave_sum_u64(vsum);
  if (lane == 0) {
    if (n) atomicAdd(a.ctl + 2 * a.it, n);
    if (s) atomicAdd(a.ctl + 2 * a.it + 1, s);
  }
}

// The decentralised filter's loop path (a.local): refine_grad_kernel with the LOCAL loads, a kernel of
// its own name -- the joint kernel keeps its own, instruction for instruction.
template <int NW, int D>
__global__ __launch_bounds__(NW * 64, 1) void refine_grad_local_kernel(RefineArgs a) {
  // early-out: the previous iteration had no active edge -> nothing can change any more (this
  // iteration's control words stay zero, which stops the next one)
  if (a.it > 0 && a.ctl[2 * (a.it - 1)] == 0ull) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const RefW w = refine_weights(smem, a);
  __syncthreads();
  const int wave = wave_id(), lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const unsigned E = (unsigned)a.B * a.N * a.K;
  const unsigned ntiles = (E + 31u) / 32u;
  const unsigned stride = gridDim.x * NW;
  unsigned long long nact = 0, vsum = 0;
  unsigned tile = (unsigned)blockIdx.x * NW + wave;
  RefIn<D> nx;
  refine_load<D, true>(a, tile, r, E, nx);
  for (; tile < ntiles; tile += stride) {
    const RefIn<D> cur = nx;
    refine_load<D, true>(a, tile + stride, r, E, nx);   // prefetch (clamped past the end)
    // no live edge (every env of the tile masked out): nothing to evaluate. One scalar branch on
    // the ballot for the whole wave -- no MFMA below runs under a lane-divergent condition.
    if (__ballot(cur.in) == 0ull) continue;
    RefOut<D> o;
    refine_tile<D>(cur, w, a, lane, h, o);
    if (cur.in && h == 0) {
      const size_t e = tile * 32u + (unsigned)r;
      refine_record<D>(cur, o, a.hn_out, a.flag_out, e, a.dEv + e * D, nact, vsum);
    }
  }
  const unsigned long long n = wave_sum_u64(nact), s = wave_sum_u64(vsum);
  if (lane == 0) {
    if (n) atomicAdd(a.ctl + 2 * a.it, n);
    if (s) atomicAdd(a.ctl + 2 * a.it + 1, s);
  }
}

// ---------------------------------------------------------------------------------------------
// Persistent filter for small envs (Nn <= SMALL_MAXN graph nodes, K <= 16: at most 32 tiles): one
// workgroup per env runs the whole loop in one launch. Prologue: the weight images and the env's
// own data (node records, a, delta = 0, h(s_t), idx, reverse CSR) go to LDS; dEv lives in LDS.
// Iteration: the waves split the env's tiles (env-local: edge e of the env is in tile e / 32) and
// run refine_tile on `a + delta` from LDS -> barrier -> the env's active count and violation sum
// (integers, summed over the waves in LDS) go to ew[b, it] as plain stores of one lane -> the
// 16-lane-group update of refine_update on the LDS copies -> barrier. The env stops at its first
// iteration without an active edge (a zero hinge has a zero gradient: delta can never change
// again): the later violation words are filled with that iteration's sum -- exact, the iterate
// stays as it is -- and the later counts stay zero. The stop is read from LDS after a barrier and
// made scalar, so every wave runs the same barriers; no workgroup waits for another. An env with
// env_active[b] == 0 returns at once: ew[b] and its delta stay zero. No atomics.
constexpr int RS_MAXN = 64;                    // SMALL_MAXN (ops/native.py)
constexpr int RS_MAXE = RS_MAXN * 16;          // edges of the largest env
constexpr int RS_PTR = 68;                     // Nn + 1 reverse-CSR offsets, padded to 16 B
template <int D> constexpr size_t RS_S_OFF = REFINE_LDS;                                     // node records
template <int D> constexpr size_t RS_A_OFF = RS_S_OFF<D> + (size_t)RS_MAXN * REC<D> * 16;    // a | delta
template <int D> constexpr size_t RS_H_OFF = RS_A_OFF<D> + (size_t)2 * RS_MAXN * D * 4;      // h(s_t)
template <int D> constexpr size_t RS_I_OFF = RS_H_OFF<D> + (size_t)RS_MAXE * 4;              // idx
template <int D> constexpr size_t RS_E_OFF = RS_I_OFF<D> + (size_t)RS_MAXE * 4;              // reverse-CSR edges
template <int D> constexpr size_t RS_P_OFF = RS_E_OFF<D> + (size_t)RS_MAXE * 4;              // reverse-CSR offsets
template <int D> constexpr size_t RS_G_OFF = RS_P_OFF<D> + (size_t)RS_PTR * 4;               // dEv
template <int D> constexpr size_t RS_R_OFF = RS_G_OFF<D> + (size_t)RS_MAXE * D * 4;          // per-wave sums
template <int NW, int D> constexpr size_t REFINE_SMALL_LDS = RS_R_OFF<D> + (size_t)NW * 2 * 8;
static_assert(REFINE_LDS % 16 == 0 && REFINE_SMALL_LDS<REFINE_NW, 3> <= 128 * 1024, "LDS layout");

// The update of both paths, lane l of agent i's 16-lane group: g = sum_out dEv - sum_in dEv over
// one env's arrays (dE (N*K, D), ptr / edges its reverse CSR), the same value in all 16 lanes.
// Outgoing edges: one coalesced segment of K records; incoming: the reverse CSR over the lanes;
// then the fixed xor butterfly.
// LOCAL (the decentralised filter): the agent's own K slots alone -- no in-edge term, no reverse CSR.
template <int D, bool LOCAL = false>
DEV void refine_node_grad(const float* dE, const int* ptr, const int* edges, int i, int l, int K, int NK, float (&g)[D]) {
#pragma unroll
  for (int q = 0; q < D; ++q) g[q] = 0.f;
  for (int k = l; k < K; k += RG)
#pragma unroll
    for (int q = 0; q < D; ++q) g[q] += dE[((size_t)i * K + k) * D + q];
  if constexpr (!LOCAL) {
    const int q0 = min(max(ptr[i], 0), NK), q1 = min(max(ptr[i + 1], 0), NK);
    for (int x = q0 + l; x < q1; x += RG) {
      const int e = min(max(edges[x], 0), NK - 1);
#pragma unroll
      for (int q = 0; q < D; ++q) g[q] -= dE[(size_t)e * D + q];
    }
  }
#pragma unroll
  for (int q = 0; q < D; ++q) g[q] = grp_sum(g[q]);
}
// the gradient step of one delta component: d s'_v / d delta = dt
DEV float refine_step(float d, float lr, float dt, float g) { return d - lr * (dt * g); }
// the projection of one delta component onto the actuator box: ac + delta in [-a_max, a_max] for the
// clamped action ac. Comparisons, not fminf / fmaxf: a NaN stays a NaN, as in torch.clamp.
DEV float refine_project(float d, float ac, float a_max) {
  const float lo = -a_max - ac, hi = a_max - ac;
  return d < lo ? lo : (d > hi ? hi : d);
}

template <int NW, int D>
__global__ __launch_bounds__(NW * 64, 1) void refine_small_kernel(RefineSmallArgs sa) {
  const RefineArgs& a = sa.r;
  const int b = blockIdx.x;
  if (a.env_active && a.env_active[b] == 0) return;        // masked-out env: nothing is written
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const RefW w = refine_weights(smem, a);
  float4* Sl = reinterpret_cast<float4*>(smem + RS_S_OFF<D>);
  float* al = reinterpret_cast<float*>(smem + RS_A_OFF<D>);
  float* dl = al + RS_MAXN * D;
  float* hl = reinterpret_cast<float*>(smem + RS_H_OFF<D>);
  int* il = reinterpret_cast<int*>(smem + RS_I_OFF<D>);
  int* el = reinterpret_cast<int*>(smem + RS_E_OFF<D>);
  int* pl = reinterpret_cast<int*>(smem + RS_P_OFF<D>);
  float* gl = reinterpret_cast<float*>(smem + RS_G_OFF<D>);
  unsigned long long* red = reinterpret_cast<unsigned long long*>(smem + RS_R_OFF<D>);
  const int N = a.N, Nn = a.Nn, K = a.K, NK = N * K;
  const int tid = threadIdx.x, nthr = NW * 64;
  {
    const float4* Sg = a.S + (size_t)b * (size_t)a.s_env * REC<D>;
    for (int x = tid; x < Nn * REC<D>; x += nthr) Sl[x] = Sg[x];
    const float* ag = a.a + (size_t)b * N * D;
    for (int x = tid; x < N * D; x += nthr) { al[x] = ag[x]; dl[x] = 0.f; }
    const float* hg = a.h + (size_t)b * NK;
    const int* ig = a.idx + (size_t)b * NK;
    const int* eg = a.edges + (size_t)b * NK;
    for (int x = tid; x < NK; x += nthr) { hl[x] = hg[x]; il[x] = ig[x]; el[x] = eg[x]; }
    const int* pg = a.ptr + (size_t)b * (Nn + 1);
    for (int x = tid; x <= Nn; x += nthr) pl[x] = pg[x];
  }
  __syncthreads();
  const int wave = wave_id(), lane = tid & 63, r = lane & 31, h = lane >> 5;
  const unsigned ntiles = ((unsigned)NK + 31u) / 32u;
  unsigned long long* ew = sa.ew + (size_t)b * sa.loops * 2;
  for (int it = 0; it < sa.loops; ++it) {
    // ---- gradient phase: tiles wave, wave + NW, ... (a scalar trip count per wave)
    unsigned long long nact = 0, vsum = 0;
    for (unsigned tile = (unsigned)wave; tile < ntiles; tile += NW) {
      const unsigned e = tile * 32u + (unsigned)r;
      const bool inside = e < (unsigned)NK;
      const unsigned ec = inside ? e : 0u;
      RefIn<D> cur;
      refine_edge<D>(Sl, al, dl, il[ec], hl[ec], ec / (unsigned)K, N, Nn, a.dt, inside, cur);
      RefOut<D> o;
      refine_tile<D>(cur, w, a, lane, h, o);
      if (cur.in && h == 0) {
        const bool tr = it == 0;
        refine_record<D>(cur, o, tr ? a.hn_out : nullptr, tr ? a.flag_out : nullptr, (size_t)b * NK + e,
                         gl + (size_t)e * D, nact, vsum);
      }
    }
    const unsigned long long n = wave_sum_u64(nact), s = wave_sum_u64(vsum);
    if (lane == 0) { red[2 * wave] = n; red[2 * wave + 1] = s; }
    __syncthreads();
    unsigned long long act = 0, vs = 0;
#pragma unroll
    for (int x = 0; x < NW; ++x) { act += red[2 * x]; vs += red[2 * x + 1]; }
    if (tid == 0) { ew[2 * it] = act; ew[2 * it + 1] = vs; }
    // the same value in every lane of the workgroup; made scalar so the loop stays wave-uniform
    const bool more = __builtin_amdgcn_readfirstlane((int)(act != 0ull)) != 0;
    if (!more) {
      if (tid == 0)
        for (int x = it + 1; x < sa.loops; ++x) ew[2 * x + 1] = vs;
      break;
    }
    // ---- update phase: one 16-lane group per agent, agents grp, grp + NW*4, ... (the trip count
    // is the same for every lane; a group past the end redoes agent N - 1 and writes nothing)
    const int l = tid % RG, grp = tid / RG;
    for (int i0 = 0; i0 < N; i0 += nthr / RG) {
      const int i = min(i0 + grp, N - 1);
      float g[D];
      refine_node_grad<D>(gl, pl, el, i, l, K, NK, g);
      if (l == 0 && i0 + grp < N) {
        float* d = dl + (size_t)i * D;
#pragma unroll
        for (int q = 0; q < D; ++q) d[q] = refine_step(d[q], a.lr, a.dt, g[q]);
        if (a.a_max > 0.f) {                              // scalar: a kernel argument
          const float* ac = al + (size_t)i * D;
#pragma unroll
          for (int q = 0; q < D; ++q) d[q] = refine_project(d[q], ac[q], a.a_max);
        }
      }
    }
    __syncthreads();
  }
  float* dg = a.delta + (size_t)b * N * D;
  for (int x = tid; x < N * D; x += nthr) dg[x] = dl[x];
}

// ---------------------------------------------------------------------------------------------
// Decentralised filter (coupling "local"), the whole loop in one launch for any scene. Agent i refines
// its own action against its neighbours' NOMINAL next states s_j + dt [v_j, a_j]: its problem depends
// on its own row alone, so a wave keeps everything in registers. A 32-edge tile is 2 agents x 16 slots
// (slots >= K are not in the tile, like the edges of a masked-out env; tiles straddle envs when N is
// odd). The wave gathers s_i, s_j, a_i, a_j and h(s_t) once per tile -- the next tile's gathers are
// issued before the current tile's loop, unconditionally on clamped indices -- and p'_i - p'_j and v'_j
// are loop invariants. Per iteration: u_i = a_i + delta_i, v'_i and rv in refine_edge's expression
// order (the self slot takes v'_j = v'_i: an exact zero), refine_tile unchanged, gv zeroed for self
// and inactive edges, the 16 slots of an agent summed with refine_node_grad's butterfly (one term per
// lane: the same pairing, the same bits), refine_step and refine_project. delta lives in registers and
// is stored once. The tile stops at its first iteration without an active edge (a ballot, scalar: no
// MFMA under a lane-divergent condition) and then adds the violation sum of its unchanged iterate to
// every later word, as refine_small_kernel repeats its word. ctl is the loop path's array, zero at
// the launch; integer atomics, so the result words do not depend on the order. The only barrier is
// the one after the weight copy. hn_out / flag_out: iteration 0 only.
template <int D>
struct LocIn {
  float pi[D], vi[D], pj[D], vj[D], ai[D], aj[D];
  float hv;
  unsigned g, e;        // the agent b*N + i and the edge g*K + k (clamped to 0 where there is none)
  int i, j;
  bool live, in, agent_j;   // live: the lane's agent exists in a live env; in: and its slot is < K
};

template <int D>
DEV void refine_local_load(const RefineArgs& a, unsigned tile, int r, unsigned BN, LocIn<D>& x) {
  const unsigned g = tile * 2u + (unsigned)(r >> 4);
  const int k = r & 15;
  const bool ag = g < BN;
  const unsigned gc = ag ? g : 0u;
  const unsigned b = gc / (unsigned)a.N;
  const unsigned i = gc - b * (unsigned)a.N;
  x.live = ag && (a.env_active ? a.env_active[b] != 0 : true);
  x.in = x.live && k < a.K;
  x.g = gc;
  x.e = (ag && k < a.K) ? gc * (unsigned)a.K + (unsigned)k : 0u;
  const float4* Sb = a.S + (size_t)b * (size_t)a.s_env * REC<D>;
  const float* ab = a.a + (size_t)b * a.N * D;
  const unsigned j = (unsigned)min(max(a.idx[x.e], 0), a.Nn - 1);
  x.agent_j = j < (unsigned)a.N;
  const unsigned ja = x.agent_j ? j : (unsigned)(a.N - 1);
  load_rec<D>(Sb, i, x.pi, x.vi);
  load_rec<D>(Sb, j, x.pj, x.vj);
#pragma unroll
  for (int q = 0; q < D; ++q) {
    x.ai[q] = ab[(size_t)i * D + q];
    x.aj[q] = ab[(size_t)ja * D + q];
  }
  x.hv = a.h[x.e];
  x.i = (int)i;
  x.j = (int)j;
}

template <int NW, int D>
__global__ __launch_bounds__(NW * 64, 1) void refine_local_kernel(RefineSmallArgs sa) {
  const RefineArgs& a = sa.r;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const RefW w = refine_weights(smem, a);
  __syncthreads();
  const int wave = wave_id(), lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const unsigned BN = (unsigned)a.B * a.N;
  const unsigned ntiles = (BN + 1u) / 2u;
  const unsigned stride = gridDim.x * NW;
  const int loops = sa.loops;
  const float dt = a.dt;
  unsigned tile = (unsigned)blockIdx.x * NW + wave;
  LocIn<D> nx;
  refine_local_load<D>(a, tile, r, BN, nx);
  for (; tile < ntiles; tile += stride) {
    const LocIn<D> x = nx;
    refine_local_load<D>(a, tile + stride, r, BN, nx);   // the next tile's gathers (clamped past the end)
    if (__ballot(x.in) == 0ull) continue;                // every env of the tile masked out (scalar)
    RefIn<D> cur;
    cur.in = x.in;
    cur.i = x.i;
    cur.j = x.j;
    cur.hv = x.hv;
    const bool self = x.j == x.i;
    float vjn[D], d[D];
#pragma unroll
    for (int q = 0; q < D; ++q) {
      const float uj = x.agent_j ? x.aj[q] : 0.f;        // the neighbour's nominal action
      const float pin = x.pi[q] + x.vi[q] * dt, pjn = x.pj[q] + x.vj[q] * dt;
      vjn[q] = x.vj[q] + uj * dt;
      cur.rp[q] = x.in ? pin - pjn : 0.f;
      d[q] = 0.f;
    }
    for (int it = 0; it < loops; ++it) {
#pragma unroll
      for (int q = 0; q < D; ++q) {
        const float ui = x.ai[q] + d[q];
        const float vin = x.vi[q] + ui * dt;
        cur.rv[q] = x.in ? vin - (self ? vin : vjn[q]) : 0.f;
      }
      RefOut<D> o;
      refine_tile<D>(cur, w, a, lane, h, o);
      const bool rec = x.in && h == 0;
      if (rec && it == 0) {
        if (a.hn_out) a.hn_out[x.e] = o.hnv;
        if (a.flag_out) a.flag_out[x.e] = o.on ? 1 : 0;
      }
      const unsigned long long act = __ballot(rec && o.on);
      const unsigned long long s = wave_sum_u64(rec ? refine_viol_fx(o.deriv) : 0ull);
      if (lane == 0) {
        if (act) atomicAdd(a.ctl + 2 * it, (unsigned long long)__popcll(act));
        if (s) atomicAdd(a.ctl + 2 * it + 1, s);
      }
      if (act == 0ull) {                                 // scalar: the tile's iterate never changes again
        if (s)
          for (int y = it + 1 + lane; y < loops; y += 64) atomicAdd(a.ctl + 2 * y + 1, s);
        break;
      }
      const bool wr = o.on && !self;
#pragma unroll
      for (int q = 0; q < D; ++q) {
        // gv is the h = 0 lane's (refine_tile: the h = 1 lane holds the position rows there); both
        // halves must step alike, they build the next iteration's fragment together
        const float gh = wr ? o.gv[q] : 0.f, go = shfl_xor32(gh);
        float g = 0.f;
        g += h ? go : gh;
        g = grp_sum(g);
        d[q] = refine_step(d[q], a.lr, dt, g);
      }
      if (a.a_max > 0.f) {                               // scalar: a kernel argument
#pragma unroll
        for (int q = 0; q < D; ++q) d[q] = refine_project(d[q], x.ai[q], a.a_max);
      }
    }
    if (x.live && lane < 32 && (lane & 15) == 0) {
#pragma unroll
      for (int q = 0; q < D; ++q) a.delta[(size_t)x.g * D + q] = d[q];
    }
  }
}

}  // namespace MB_PREC
}  // namespace mb

// once per loop, before the first refine_grad launch: the kernel's dynamic LDS exceeds the default limit
extern "C" int MB_SYM(refine_prepare)(int dim) {
  using namespace mb;
  using namespace mb::MB_PREC;
  if (dim != 2 && dim != 3) return -1;
  return by_dim(dim, [](auto D) {
    const int e = (int)hipFuncSetAttribute((const void*)refine_grad_kernel<REFINE_NW, D()>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)REFINE_LDS);
    if (e) return e;
    return (int)hipFuncSetAttribute((const void*)refine_grad_local_kernel<REFINE_NW, D()>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)REFINE_LDS);
  });
}

extern "C" int MB_SYM(refine_grad)(const mb::RefineArgs* a, int num_blocks, hipStream_t st) {
  using namespace mb;
  using namespace mb::MB_PREC;
  if (a->K > 16 || a->K < 1 || a->B < 1 || a->N < 1 || a->Nn < a->N || num_blocks < 1 || a->it < 0) return -1;
  if (!a->S || !a->idx || !a->a || !a->delta || !a->h || !a->wpack || !a->wrm || !a->wvec || !a->dEv || !a->ctl) return -2;
  if ((long)a->B * a->N * a->K >= (1l << 31) - 32l * 65536) return -3;     // 32-bit edge indexing
  if (a->dim != 2 && a->dim != 3) return -1;
  return by_dim(a->dim, [&](auto D) {     // (the LDS attribute: refine_prepare, once per loop)
    if (a->local)
      return launch(refine_grad_local_kernel<REFINE_NW, D()>, dim3(num_blocks), dim3(REFINE_NW * 64), REFINE_LDS, st, *a);
    return launch(refine_grad_kernel<REFINE_NW, D()>, dim3(num_blocks), dim3(REFINE_NW * 64), REFINE_LDS, st, *a);
  });
}

// The decentralised filter in one launch (refine_local_kernel): sa->r.ctl (2 * loops words) must be
// zero at the launch; r.dEv, r.ptr, r.edges and r.it are not used. Sets the kernel's dynamic-LDS
// attribute itself.
extern "C" int MB_SYM(refine_local)(const mb::RefineSmallArgs* sa, int num_blocks, hipStream_t st) {
  using namespace mb;
  using namespace mb::MB_PREC;
  const RefineArgs* a = &sa->r;
  if (a->K > 16 || a->K < 1 || a->B < 1 || a->N < 1 || a->Nn < a->N || num_blocks < 1 || sa->loops < 1) return -1;
  if (!a->S || !a->idx || !a->a || !a->delta || !a->h || !a->wpack || !a->wrm || !a->wvec || !a->ctl) return -2;
  if ((long)a->B * a->N * 16 >= (1l << 31) - 32l * 65536) return -3;       // 32-bit indexing of the padded rows
  if (a->s_env < a->Nn) return -1;
  if (a->dim != 2 && a->dim != 3) return -1;
  return by_dim(a->dim, [&](auto D) {
    const auto kern = refine_local_kernel<REFINE_NW, D()>;
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)REFINE_LDS);
    if (e != hipSuccess) return (int)e;     // this launcher reports the attribute's error
    return launch(kern, dim3(num_blocks), dim3(REFINE_NW * 64), REFINE_LDS, st, *sa);
  });
}

// The persistent filter of envs of at most RS_MAXN graph nodes: one launch of B workgroups. Sets
// the kernel's dynamic-LDS attribute itself; ew (B, loops, 2) must be zero at the launch.
extern "C" int MB_SYM(refine_small)(const mb::RefineSmallArgs* sa, hipStream_t st) {
  using namespace mb;
  using namespace mb::MB_PREC;
  const RefineArgs* a = &sa->r;
  if (a->K > 16 || a->K < 1 || a->B < 1 || a->N < 1 || a->Nn < a->N || a->Nn > RS_MAXN || sa->loops < 1) return -1;
  if (!a->S || !a->idx || !a->a || !a->delta || !a->h || !a->wpack || !a->wrm || !a->wvec || !a->ptr || !a->edges ||
      !sa->ew)
    return -2;
  if (a->s_env < a->Nn) return -1;
  if (a->dim != 2 && a->dim != 3) return -1;
  return by_dim(a->dim, [&](auto D) {
    const auto kern = refine_small_kernel<REFINE_NW, D()>;
    const size_t lds = REFINE_SMALL_LDS<REFINE_NW, D()>;
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;     // this launcher reports the attribute's error
    return launch(kern, dim3(a->B), dim3(REFINE_NW * 64), lds, st, *sa);
  });
}

#if !MB_X3 && !MB_FP16
// The update is plain fp32: compiled once (with the default build of this file).
namespace mb {

template <int D>
__global__ __launch_bounds__(256) void refine_update_kernel(RefineArgs a) {
  if (a.ctl[2 * a.it] == 0ull) return;                     // no active edge: dEv is all zeros
  const long node = ((long)blockIdx.x * blockDim.x + threadIdx.x) / RG;
  if (node >= (long)a.B * a.N) return;                     // whole 16-lane groups
  const int l = threadIdx.x % RG;
  const int N = a.N, K = a.K, NK = N * K;
  const int b = (int)(node / N), i = (int)(node % N);
  if (a.env_active && a.env_active[b] == 0) return;        // masked-out env: delta stays zero (whole group)
  float g[D];
  MB_PREC::refine_node_grad<D>(a.dEv + (size_t)b * NK * D, a.ptr + (size_t)b * (a.Nn + 1), a.edges + (size_t)b * NK, i, l,
                               K, NK, g);
  if (l != 0) return;
  float* d = a.delta + ((size_t)b * N + i) * D;
#pragma unroll
  for (int q = 0; q < D; ++q) d[q] = MB_PREC::refine_step(d[q], a.lr, a.dt, g[q]);
  if (a.a_max > 0.f) {                                     // scalar: a kernel argument
    const float* ac = a.a + ((size_t)b * N + i) * D;
#pragma unroll
    for (int q = 0; q < D; ++q) d[q] = MB_PREC::refine_project(d[q], ac[q], a.a_max);
  }
}

// The decentralised filter's loop path (a.local): the agent's own K slots alone, no reverse CSR. A kernel
// of its own name -- the joint kernel keeps its own, instruction for instruction.
template <int D>
__global__ __launch_bounds__(256) void refine_update_local_kernel(RefineArgs a) {
  if (a.ctl[2 * a.it] == 0ull) return;                     // no active edge: dEv is all zeros
  const long node = ((long)blockIdx.x * blockDim.x + threadIdx.x) / RG;
  if (node >= (long)a.B * a.N) return;                     // whole 16-lane groups
  const int l = threadIdx.x % RG;
  const int N = a.N, K = a.K, NK = N * K;
  const int b = (int)(node / N), i = (int)(node % N);
  if (a.env_active && a.env_active[b] == 0) return;        // masked-out env: delta stays zero (whole group)
  float g[D];
  MB_PREC::refine_node_grad<D, true>(a.dEv + (size_t)b * NK * D, nullptr, nullptr, i, l, K, NK, g);
  if (l != 0) return;
  float* d = a.delta + ((size_t)b * N + i) * D;
#pragma unroll
  for (int q = 0; q < D; ++q) d[q] = MB_PREC::refine_step(d[q], a.lr, a.dt, g[q]);
  if (a.a_max > 0.f) {                                     // scalar: a kernel argument
    const float* ac = a.a + ((size_t)b * N + i) * D;
#pragma unroll
    for (int q = 0; q < D; ++q) d[q] = MB_PREC::refine_project(d[q], ac[q], a.a_max);
  }
}

}  // namespace mb

extern "C" int mb_refine_update(const mb::RefineArgs* a, hipStream_t st) {
  using namespace mb;
  if (a->K > 16 || a->K < 1 || a->B < 1 || a->N < 1 || a->Nn < a->N || a->it < 0) return -1;
  if (!a->delta || !a->dEv || !a->ctl || (a->a_max > 0.f && !a->a)) return -2;
  if (!a->local && (!a->ptr || !a->edges)) return -2;      // the joint update walks the reverse CSR
  const long total = (long)a->B * a->N * RG;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (a->dim != 2 && a->dim != 3) return -1;
  return by_dim(a->dim, [&](auto D) {
    if (a->local) return launch(refine_update_local_kernel<D()>, grid, dim3(256), 0, st, *a);
    return launch(refine_update_kernel<D()>, grid, dim3(256), 0, st, *a);
  });
}
#endif
