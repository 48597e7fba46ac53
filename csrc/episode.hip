// Closed-loop episodes on the device, gfx950: the per-step glue of a batch of episodes (validation
// during training, evaluation) between the scan, the controller and the safety filter.
//
//   episode_limit_kernel    (with an actuator limit only) one thread per action component: the
//     controller's action clamped to [-a_max, a_max] in place, before the filter reads it.
//   episode_advance_kernel  one thread per agent: u = a + delta (clamped to the box under a limit),
//     s' = s + [v, u] * dt (or s, once every env is done), the record of S_next, the env's
//     goal-distance sum in fixed point and, when asked for, the action statistics of the agents whose
//     env is active at the start of the step.
//   episode_tally_kernel    one workgroup per step: the integer totals, the per-env done mask, the
//     "some env still runs" word, the filter's iteration count; clears the per-step accumulators.
//   episode_final_kernel    one workgroup, after the safety-only scan of the final state: the result
//     vector in the order of validate.COUNTS.
// The kernels are ordered by the stream alone: none waits for another workgroup. The expressions are
// those of the Python episode (evaluate._euler, safety_filter's a32 + delta), in plain fp32 without
// contraction, so the states are the Python path's bit for bit; the decisions are integer sums, so
// they do not depend on the order in which waves arrive.
#pragma clang fp contract(off)
#include "common.h"
#include "args.h"
#include "launch.h"
#include "state.h"

namespace mb {

constexpr int EP_BLOCK = 256;

// |p' - g| in fixed point; NaN / Inf / out of range -> FX_SAT (the controller step's scheme)
DEV unsigned long long episode_dist_fx(float d) {
  const double x = (double)d * FX_DIST;
  return (x >= 0.0 && x < FX_SAT) ? (unsigned long long)__double2ll_rn(x) : (unsigned long long)FX_SAT;
}

template <int D>
DEV float episode_goal_dist(const float (&p)[D], const float* g) {
  float e[D];
#pragma unroll
  for (int q = 0; q < D; ++q) e[q] = p[q] - g[q];
  return sqrtf(sqsum<D>(e));
}

// |delta| in 2^-20 fixed point, rounded half-even per component; NaN / Inf / out of range -> FX_SAT
DEV unsigned long long episode_delta_fx(float d) {
  const double x = (double)fabsf(d) * FX_DELTA;
  return (x >= 0.0 && x < FX_SAT) ? (unsigned long long)__double2ll_rn(x) : (unsigned long long)FX_SAT;
}

// torch.clamp(v, -m, m): comparisons, so a NaN stays a NaN
DEV float episode_clamp(float v, float m) { return v < -m ? -m : (v > m ? m : v); }

DEV unsigned wave_max_u32(unsigned v) {
  static_for<6>([&](auto o_) {
    constexpr int O = 32 >> decltype(o_)::value;
    const unsigned w = lane_xor<O>(v);
    v = w > v ? w : v;
  });
  return v;
}

template <int D>
__global__ __launch_bounds__(EP_BLOCK) void episode_limit_kernel(EpisodeArgs a) {
  const long total = (long)a.B * a.N * D;
  const long x = (long)blockIdx.x * EP_BLOCK + threadIdx.x;
  if (x < total) a.A[x] = episode_clamp(a.A[x], a.a_max);
}

template <int D>
__global__ __launch_bounds__(EP_BLOCK) void episode_advance_kernel(EpisodeArgs a) {
  const long total = (long)a.B * a.N;
  const long gid = (long)blockIdx.x * EP_BLOCK + threadIdx.x;
  const bool ok = gid < total;
  const long gc = ok ? gid : total - 1;                 // clamped: every lane stays for the wave sum
  const int b = (int)(gc / a.N), i = (int)(gc % a.N);   // per lane: a wave can straddle two envs
  const bool alive = a.st[EP_ALIVE] != 0;
  const bool limit = a.a_max > 0.f;                     // scalar: a kernel argument
  float p[D], v[D], u[D], dl[D];
  load_rec<D>(a.S_cur + (size_t)b * a.s_env * REC<D>, (unsigned)i, p, v);
#pragma unroll
  for (int q = 0; q < D; ++q) { u[q] = a.A[gc * D + q]; dl[q] = 0.f; }
  if (a.delta) {
#pragma unroll
    for (int q = 0; q < D; ++q) {
      dl[q] = a.delta[gc * D + q];
      u[q] = u[q] + dl[q];
      if (ok) a.delta[gc * D + q] = 0.f;                // the next step's filter starts from zero
    }
  }
  if (limit) {                                          // removes the one rounding by which a + hi can pass a_max
#pragma unroll
    for (int q = 0; q < D; ++q) u[q] = episode_clamp(u[q], a.a_max);
  }
  if (a.act_st) {
    // the agents of the envs that are active at the start of the step (the tally has not run yet);
    // per-wave integer sums / max, then one integer atomic each: order independent
    const bool on = ok && a.active[b] != 0;
    bool at = false, iv = false;
    unsigned long long dsum = 0ull;
    unsigned mx = 0u;
#pragma unroll
    for (int q = 0; q < D; ++q) {
      const float au = fabsf(u[q]);
      at |= limit && au == a.a_max;
      iv |= dl[q] != 0.f;
      dsum += episode_delta_fx(dl[q]);
      const unsigned bits = __float_as_uint(au);
      mx = bits > mx ? bits : mx;
    }
    const unsigned long long n_at = wave_sum_u64(on && at ? 1ull : 0ull), n_iv = wave_sum_u64(on && iv ? 1ull : 0ull);
    const unsigned long long d_all = wave_sum_u64(on ? dsum : 0ull);
    const unsigned m_all = wave_max_u32(on ? mx : 0u);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
      unsigned long long* w = reinterpret_cast<unsigned long long*>(a.act_st);
      if (n_at) atomicAdd(w + EP_ACT_LIMITED, n_at);
      if (n_iv) atomicAdd(w + EP_ACT_INTERVENED, n_iv);
      if (d_all) atomicAdd(w + EP_ACT_DELTA, d_all);
      if (m_all) atomicMax(w + EP_ACT_MAX, (unsigned long long)m_all);
    }
  }
  if (alive) {
#pragma unroll
    for (int q = 0; q < D; ++q) {
      const float pn = p[q] + v[q] * a.dt, vn = v[q] + u[q] * a.dt;
      p[q] = pn;
      v[q] = vn;
    }
  }
  if (ok) store_rec<D>(a.S_next + (size_t)b * a.s_env * REC<D>, (unsigned)i, p, v);
  unsigned long long dq = ok ? episode_dist_fx(episode_goal_dist<D>(p, a.G + gc * D)) : 0ull;
  const long w0 = gid - (threadIdx.x & (WAVE - 1));
  const long w1 = (w0 + WAVE - 1 < total ? w0 + WAVE - 1 : total - 1);
  if (w0 / a.N == w1 / a.N) {                           // the wave's agents share an env: one atomic
    dq = wave_sum_u64(dq);
    if ((threadIdx.x & (WAVE - 1)) == 0) atomicAdd(a.dist_fx + w0 / a.N, dq);
  } else if (ok) {
    atomicAdd(a.dist_fx + b, dq);
  }
}

__global__ __launch_bounds__(EP_BLOCK) void episode_tally_kernel(EpisodeArgs a) {
  __shared__ unsigned long long s_safe, s_env;
  __shared__ int s_any, s_used;
  const int tid = threadIdx.x;
  if (tid == 0) { s_safe = 0ull; s_env = 0ull; s_any = 0; s_used = 0; }
  const long long alive = a.st[EP_ALIVE];
  __syncthreads();
  unsigned long long sf = 0ull, es = 0ull;
  int any = 0, used = 0;
  for (int b = tid; b < a.B; b += EP_BLOCK) {
    const int act = a.active[b] != 0, pa = a.prev_active[b] != 0;
    // safe[b] counts S_cur = s_t: the safety of the step before, of the envs that ran it
    if (pa) sf += (unsigned long long)__float2ll_rn(a.safe[b]);
    es += (unsigned long long)act;
    a.prev_active[b] = (uint8_t)act;
    const int na = act && a.dist_fx[b] >= a.thr_fx;
    a.active[b] = (uint8_t)na;
    any |= na;
    a.dist_fx[b] = 0ull;
    a.safe[b] = 0.f;
    if (a.mode == 2) {                                  // iterations this env's filter worked in
      int n = 0;
      for (int it = 0; it < a.loops; ++it) {
        unsigned long long* w = a.ew + ((size_t)b * a.loops + it) * 2;
        n += w[0] != 0ull;
        w[0] = 0ull;
        w[1] = 0ull;
      }
      used = n > used ? n : used;
    }
  }
  if (a.mode == 1)
    for (int it = tid; it < a.loops; it += EP_BLOCK) used += a.ctl[2 * it] != 0ull;
  if (sf) atomicAdd(&s_safe, sf);
  if (es) atomicAdd(&s_env, es);
  if (any) atomicOr(&s_any, 1);
  if (used) { if (a.mode == 1) atomicAdd(&s_used, used); else atomicMax(&s_used, used); }
  __syncthreads();
  if (tid == 0) {
    a.st[EP_SAFE] += (long long)s_safe;
    a.st[EP_ENV_STEPS] += (long long)s_env;
    a.st[EP_STEPS] += alive != 0;
    if (alive != 0) a.st[EP_ITERS] += s_used;           // a step after the last env finished counts nothing
    a.st[EP_ALIVE] = s_any;
  }
}

template <int D>
__global__ __launch_bounds__(EP_BLOCK) void episode_final_kernel(EpisodeArgs a) {
  __shared__ unsigned long long s_safe, s_dist, s_reach;
  const int tid = threadIdx.x;
  if (tid == 0) { s_safe = 0ull; s_dist = 0ull; s_reach = 0ull; }
  __syncthreads();
  unsigned long long sf = 0ull, ds = 0ull, rc = 0ull;
  for (int b = tid; b < a.B; b += EP_BLOCK)
    if (a.prev_active[b] != 0) sf += (unsigned long long)__float2ll_rn(a.safe[b]);
  const long total = (long)a.B * a.N;
  for (long g = tid; g < total; g += EP_BLOCK) {
    const int b = (int)(g / a.N), i = (int)(g % a.N);
    float p[D], v[D];
    load_rec<D>(a.S_cur + (size_t)b * a.s_env * REC<D>, (unsigned)i, p, v);
    const float d = episode_goal_dist<D>(p, a.G + g * D);
    rc += d < a.thr;
    ds += episode_dist_fx(d);
  }
  if (sf) atomicAdd(&s_safe, sf);
  if (ds) atomicAdd(&s_dist, ds);
  if (rc) atomicAdd(&s_reach, rc);
  __syncthreads();
  if (tid == 0) {
    const long long env_steps = a.st[EP_ENV_STEPS];
    a.out[0] = a.st[EP_SAFE] + (long long)s_safe;
    a.out[1] = env_steps * a.N;
    a.out[2] = (long long)s_reach;
    a.out[3] = total;
    a.out[4] = env_steps;
    a.out[5] = a.st[EP_ITERS];
    a.out[6] = a.st[EP_STEPS];
    a.out[7] = (long long)((s_dist + (1ull << 11)) >> 12);   // 2^-32 -> the 2^-20 of validate.DIST_FX
    if (a.act_st && a.act_out)
      for (int w = 0; w < EP_ACT_WORDS; ++w) a.act_out[w] = a.act_st[w];
  }
}

static int episode_check(const EpisodeArgs* a) {
  if (a->B < 1 || a->N < 1 || a->s_env < a->N || (a->dim != 2 && a->dim != 3)) return -1;
  if ((long)a->B * a->N >= (1l << 31) - 65536) return -3;
  if (!a->S_cur || !a->G || !a->st || !a->safe || !a->prev_active) return -2;
  return 0;
}

}  // namespace mb

// the controller's actions clamped to the actuator box, in place (a_max > 0)
extern "C" int mb_episode_limit(const mb::EpisodeArgs* a, hipStream_t st) {
  using namespace mb;
  if (a->B < 1 || a->N < 1 || (a->dim != 2 && a->dim != 3) || !(a->a_max > 0.f)) return -1;
  if ((long)a->B * a->N >= (1l << 31) - 65536) return -3;
  if (!a->A) return -2;
  const dim3 grid((unsigned)(((long)a->B * a->N * a->dim + EP_BLOCK - 1) / EP_BLOCK));
  return by_dim(a->dim, [&](auto D) { return launch(episode_limit_kernel<D()>, grid, dim3(EP_BLOCK), 0, st, *a); });
}

extern "C" int mb_episode_advance(const mb::EpisodeArgs* a, hipStream_t st) {
  using namespace mb;
  if (const int rc = episode_check(a)) return rc;
  if (!a->S_next || !a->A || !a->dist_fx || a->S_next == a->S_cur || (a->act_st && !a->active)) return -2;
  if (a->a_max < 0.f || a->a_max != a->a_max) return -1;
  const dim3 grid((unsigned)(((long)a->B * a->N + EP_BLOCK - 1) / EP_BLOCK));
  return by_dim(a->dim, [&](auto D) { return launch(episode_advance_kernel<D()>, grid, dim3(EP_BLOCK), 0, st, *a); });
}

extern "C" int mb_episode_tally(const mb::EpisodeArgs* a, hipStream_t st) {
  using namespace mb;
  if (const int rc = episode_check(a)) return rc;
  if (!a->dist_fx || !a->active || a->loops < 0 || a->mode < 0 || a->mode > 2) return -2;
  if ((a->mode == 1 && !a->ctl) || (a->mode == 2 && !a->ew)) return -2;
  return launch(episode_tally_kernel, dim3(1), dim3(EP_BLOCK), 0, st, *a);
}

extern "C" int mb_episode_final(const mb::EpisodeArgs* a, hipStream_t st) {
  using namespace mb;
  if (const int rc = episode_check(a)) return rc;
  if (!a->out) return -2;
  return by_dim(a->dim, [&](auto D) { return launch(episode_final_kernel<D()>, dim3(1), dim3(EP_BLOCK), 0, st, *a); });
}
