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
#pragma clang fp contract(off)
#include "common.h"
#include "args.h"
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

// Edge e = (b*N + i)*K + k of a tile: every load is unconditional on a clamped index (idx holds
// node ids up to Nn - 1, a / delta have N rows: an obstacle neighbour reads row N - 1 and is zeroed).
// An edge of a masked-out env loads like any other and is then marked as not in the tile.
template <int D>
DEV void refine_load(const RefineArgs& a, unsigned tile, int r, unsigned E, RefIn<D>& x) {
  const unsigned e = tile * 32u + (unsigned)r;
  const bool inside = e < E;
  const unsigned ec = inside ? e : 0u;
  const unsigned ik = ec / (unsigned)a.K;
  const unsigned b = ik / (unsigned)a.N;
  x.in = inside && (a.env_active ? a.env_active[b] != 0 : true);
  const unsigned i = ik - b * (unsigned)a.N;
  const int jr = a.idx[ec];
  const unsigned j = (unsigned)min(max(jr, 0), a.Nn - 1);
  const bool agent_j = j < (unsigned)a.N;
  const unsigned ja = agent_j ? j : (unsigned)(a.N - 1);
  const float4* Sb = a.S + (size_t)b * (size_t)a.s_env * REC<D>;
  float pi[D], vi[D], pj[D], vj[D];
  load_rec<D>(Sb, i, pi, vi);
  load_rec<D>(Sb, j, pj, vj);
  const float* ai = a.a + ((size_t)b * a.N + i) * D;
  const float* di = a.delta + ((size_t)b * a.N + i) * D;
  const float* aj = a.a + ((size_t)b * a.N + ja) * D;
  const float* dj = a.delta + ((size_t)b * a.N + ja) * D;
  x.hv = a.h[ec];
#pragma unroll
  for (int q = 0; q < D; ++q) {
    const float ui = ai[q] + di[q];
    const float uj = agent_j ? aj[q] + dj[q] : 0.f;
    // s' = s + [v, a + delta] * dt (the evaluation's own expression order)
    const float pin = pi[q] + vi[q] * a.dt, pjn = pj[q] + vj[q] * a.dt;
    const float vin = vi[q] + ui * a.dt, vjn = vj[q] + uj * a.dt;
    x.rp[q] = x.in ? pin - pjn : 0.f;
    x.rv[q] = x.in ? vin - vjn : 0.f;
  }
  x.i = (int)i;
  x.j = (int)j;
}

template <int NW, int D>
__global__ __launch_bounds__(NW * 64, 1) void refine_grad_kernel(RefineArgs a) {
  // early-out: the previous iteration had no active edge -> nothing can change any more (this
  // iteration's control words stay zero, which stops the next one)
  if (a.it > 0 && a.ctl[2 * (a.it - 1)] == 0ull) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  h16* W2 = reinterpret_cast<h16*>(smem);
  h16* W3 = W2 + RM_W2;
  h16* wf = W2 + RMP;                         // w1f (2 frags) | w1ft (4 frags)
  float* vl = reinterpret_cast<float*>(smem + REFINE_W_BYTES);
  block_copy16(W2, a.wrm, RMP * 2, false);
  block_copy16(wf, a.wpack + (size_t)a.f_bwd * FRAG_ELEMS, 2 * FRAG_SZ, false);
  block_copy16(wf + 2 * FRAG_ELEMS, a.wpack + (size_t)(a.f_bwd + 66) * FRAG_ELEMS, 4 * FRAG_SZ, false);
  block_copy16(vl, a.wvec, CBF_VEC * 4);
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
    if (cur.in && h == 0) {
      const unsigned e = tile * 32u + (unsigned)r;
      // violation term relu(-deriv) in fixed point; NaN / Inf / out of range -> FX_SAT
      const float v = deriv < 0.f ? -deriv : (deriv == deriv ? 0.f : __builtin_inff());
      const double xq = (double)v * FX_VIOL;
      vsum += (xq >= 0.0 && xq < FX_SAT) ? (unsigned long long)__double2ll_rn(xq) : (unsigned long long)FX_SAT;
      nact += on ? 1ull : 0ull;
      if (a.hn_out) a.hn_out[e] = hnv;
      if (a.flag_out) a.flag_out[e] = on ? 1 : 0;
    }
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
      if (cur.in && h == 0) {
        const unsigned e = tile * 32u + (unsigned)r;
        // self edges: s'_i - s'_i = 0 whatever the action; inactive edges: exact zeros
        const bool wr = on && cur.j != cur.i;
        float* o = a.dEv + (size_t)e * D;
#pragma unroll
        for (int q = 0; q < D; ++q) o[q] = wr ? g4[D + q] : 0.f;
      }
    }
  }
  const unsigned long long n = wave_sum_u64(nact), s = wave_sum_u64(vsum);
  if (lane == 0) {
    if (n) atomicAdd(a.ctl + 2 * a.it, n);
    if (s) atomicAdd(a.ctl + 2 * a.it + 1, s);
  }
}

template <int D>
static void launch_refine_grad(const RefineArgs& a, int num_blocks, hipStream_t st) {
  hipLaunchKernelGGL((refine_grad_kernel<REFINE_NW, D>), dim3(num_blocks), dim3(REFINE_NW * 64), REFINE_LDS, st, a);
}

}  // namespace MB_PREC
}  // namespace mb

// once per loop, before the first refine_grad launch: the kernel's dynamic LDS exceeds the default limit
extern "C" int MB_SYM(refine_prepare)(int dim) {
  using namespace mb::MB_PREC;
  if (dim != 2 && dim != 3) return -1;
  const void* f = dim == 3 ? (const void*)refine_grad_kernel<REFINE_NW, 3> : (const void*)refine_grad_kernel<REFINE_NW, 2>;
  return (int)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)REFINE_LDS);
}

extern "C" int MB_SYM(refine_grad)(const mb::RefineArgs* a, int num_blocks, hipStream_t st) {
  using namespace mb;
  using namespace mb::MB_PREC;
  if (a->K > 16 || a->K < 1 || a->B < 1 || a->N < 1 || a->Nn < a->N || num_blocks < 1 || a->it < 0) return -1;
  if (!a->S || !a->idx || !a->a || !a->delta || !a->h || !a->wpack || !a->wrm || !a->wvec || !a->dEv || !a->ctl) return -2;
  if ((long)a->B * a->N * a->K >= (1l << 31) - 32l * 65536) return -3;     // 32-bit edge indexing
  if (a->dim == 3) launch_refine_grad<3>(*a, num_blocks, st);
  else if (a->dim == 2) launch_refine_grad<2>(*a, num_blocks, st);
  else return -1;
  return (int)hipGetLastError();
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
  const float* dE = a.dEv + (size_t)b * NK * D;
  float g[D];
#pragma unroll
  for (int q = 0; q < D; ++q) g[q] = 0.f;
  // outgoing edges: one coalesced segment of K records; incoming: the reverse CSR over the lanes
  for (int k = l; k < K; k += RG)
#pragma unroll
    for (int q = 0; q < D; ++q) g[q] += dE[((size_t)i * K + k) * D + q];
  const int* ptr = a.ptr + (size_t)b * (a.Nn + 1);
  const int* edges = a.edges + (size_t)b * NK;
  const int q0 = min(max(ptr[i], 0), NK), q1 = min(max(ptr[i + 1], 0), NK);
  for (int x = q0 + l; x < q1; x += RG) {
    const int e = min(max(edges[x], 0), NK - 1);
#pragma unroll
    for (int q = 0; q < D; ++q) g[q] -= dE[(size_t)e * D + q];
  }
#pragma unroll
  for (int q = 0; q < D; ++q) g[q] = grp_sum(g[q]);
  if (l != 0) return;
  // d s'_v / d delta = dt
  float* d = a.delta + ((size_t)b * N + i) * D;
#pragma unroll
  for (int q = 0; q < D; ++q) d[q] = d[q] - a.lr * (a.dt * g[q]);
}

}  // namespace mb

extern "C" int mb_refine_update(const mb::RefineArgs* a, hipStream_t st) {
  using namespace mb;
  if (a->K > 16 || a->K < 1 || a->B < 1 || a->N < 1 || a->Nn < a->N || a->it < 0) return -1;
  if (!a->delta || !a->dEv || !a->ptr || !a->edges || !a->ctl) return -2;
  const long total = (long)a->B * a->N * RG;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (a->dim == 3) hipLaunchKernelGGL(refine_update_kernel<3>, grid, dim3(256), 0, st, *a);
  else if (a->dim == 2) hipLaunchKernelGGL(refine_update_kernel<2>, grid, dim3(256), 0, st, *a);
  else return -1;
  return (int)hipGetLastError();
}
#endif
