// Native rollout driver: the per-step launch loop of the training rollout in C++.
//
// Reference: the inner loop of train.py:58-81 (controller step, Euler step, early break when
// mean |p - g| < DIST_MIN_CHECK) with the kNN/TTC scan of every step. The Python loop paid
// ~10 wrapper calls per step on the host while the GPU finishes a step in ~0.13 ms at
// 1024 agents x 64 envs, so the host fell behind and the GPU idled between steps. Here the
// argument structs of every step are pointer offsets of persistent buffers validated once on
// the Python side (engine/hip_engine.py), and the loop issues per step:
//   [side stream] CBF h of the previous step's main slots (overlapped with this step)
//   cell_sort (every resort_every steps) + scan, ctrl_fwd
//   [copy stream] per-env goal-distance sums -> pinned host memory
// and checks the early-stop criterion one step late (never stalls the queue on the step just
// issued). Per-env done masks are applied on the device afterwards (rollout_stats).
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <tuple>
#include <vector>

#include "args.h"
#include "pyargs.h"

namespace {

hipStream_t ST(u64 s) { return reinterpret_cast<hipStream_t>(static_cast<uintptr_t>(s)); }

class RolloutDriver {
 public:
  // (no Args::done() here or in BpttDriver: the engine passes diagnostic keys that not every build reads)
  explicit RolloutDriver(py::dict cfg) {
    Args c("RolloutDriver", cfg);
    c("B", B_); c("N", N_); c("Nn", Nn_); c("K", K_); c("D", D_);
    W_ = D_ == 2 ? 4 : 8;
    c("Tmax", Tmax_); c("num_cu", num_cu_); c("prec", prec_); prow_ = prec_ == 2 ? 256 : 128;
    c("resort_every", resort_); c("compute_safety", safety_); c("overlap_hfwd", overlap_);
    c("hfwd_blocks", hfwd_blocks_);
    c("L", L_);
    c("S", S_); c("G", G_); c("A", A_); c("idx", idx_); c("dang", dang_); c("cnt", cnt_);
    c("safe", safe_); c("dist", dist_); c("act", act_); c("pooled", pooled_); c("argmax", argmax_);
    c("perm", perm_); c("host_dist", host_dist_);
    c("ctrl_w", ctrl_w_); c("f_edge", f_edge_); c("f_node", f_node_); c("ctrl_v", ctrl_v_);
    c("cbf_w", cbf_w_); c("f_fwd", f_fwd_); c("cbf_rm", cbf_rm_); c("cbf_v", cbf_v_);
    c("hbuf", hbuf_); c("hmask", hmask_); c("src", src_); c("nev", nev_);
    c("r2_train", r2_train_); c("ttc_train", ttc_train_); c("r2_check", r2_check_); c("ttc_check", ttc_check_);
    c("dt", dt_); c("obs_r", obs_r_); c("sqrt3", sqrt3_); c("dist_thr", dist_thr_); c("dist_eps", dist_eps_);
    c("done_thr", done_thr_);
    c("check_every", check_);
    c("noise_key", noise_key_); c("noise_prob", noise_prob_); c("noise_scale", noise_scale_);
    c("scan_ws", scan_ws_); c("scan_ws_env", scan_ws_env_);
    c("apw", apw_);
    c("small_ctl", small_ctl_); c("small_apw", small_apw_); c("knn_tail", knn_tail_);
    c.opt("small_stamps", small_stamps_);
    // the node MLP's activations per step (T, B*N, node_act_bytes), kept for the cooperative node
    // backward (0 = not kept)
    c.opt("node_acts", acts_);
    c.opt("node_act_bytes", act_bytes_);
    if (small_ctl_) {
      chk(hipHostMalloc((void**)&small_res_, 2 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc");
      small_res_[0] = small_res_[1] = 0;
      chk(hipHostGetDevicePointer((void**)&small_res_dev_, small_res_, 0), "hipHostGetDevicePointer");
    }
    // early-stop publication (ctrl.hip publish_step): per-step workgroup counters on the device,
    // the per-env sums and a flag per step in host-coherent memory
    c.opt("publish", publish_);
    c.opt("poll_query_ms", poll_query_ms_);
    if (publish_) {
      const size_t nd = (size_t)Tmax_ * B_, bytes = nd * sizeof(unsigned long long) + (size_t)Tmax_ * sizeof(unsigned);
      chk(hipHostMalloc((void**)&pub_host_, bytes, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc");
      std::memset(pub_host_, 0, bytes);
      chk(hipHostGetDevicePointer((void**)&pub_dev_, pub_host_, 0), "hipHostGetDevicePointer");
      chk(hipMalloc((void**)&pub_ctr_, (size_t)Tmax_ * sizeof(unsigned)), "hipMalloc");
      chk(hipMemset(pub_ctr_, 0, (size_t)Tmax_ * sizeof(unsigned)), "hipMemset");   // once: kernels re-arm them
    }
    if (check_ < 1) check_ = 1;
    if (B_ < 1|| N_ < 1 || Nn_ < N_ || K_ < 1 || K_ > 16 || (D_ != 2 && D_ != 3) || Tmax_ < 1 || resort_ < 1)
      throw std::invalid_argument("RolloutDriver: bad dimensions");
    ev_copy_.resize(Tmax_);
    for (auto& e : ev_copy_) chk(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    // stream -> stream dependencies on one device: a device-scope release is enough (the default
    // system-scope fence writes back / invalidates caches for host visibility and stalls the
    // queue behind it); the copy-completion events the host waits on keep the system fence
    const unsigned fork_flags = hipEventDisableTiming | (c.i("fork_device_scope") ? hipEventReleaseToDevice : 0u);
    chk(hipEventCreateWithFlags(&ev_main_, fork_flags), "hipEventCreate");
    chk(hipEventCreateWithFlags(&ev_side_, fork_flags), "hipEventCreate");
  }
  ~RolloutDriver() {
    for (auto e : ev_copy_) (void)hipEventDestroy(e);
    (void)hipEventDestroy(ev_main_);
    (void)hipEventDestroy(ev_side_);
    if (small_res_) (void)hipHostFree(small_res_);
    if (pub_host_) (void)hipHostFree(pub_host_);
    if (pub_ctr_) (void)hipFree(pub_ctr_);
  }
  RolloutDriver(const RolloutDriver&) = delete;
  RolloutDriver& operator=(const RolloutDriver&) = delete;

  // Returns (T, tail_scanned): T valid steps; tail_scanned = the scan of s_T was issued (the
  // early-stopped case, where step T's scan ran before the break).
  std::pair<int, bool> run(u64 stream, u64 hstream, u64 copy_stream, bool early_stop) {
    hipStream_t st = ST(stream), hs = ST(hstream), cs = ST(copy_stream);
    const volatile unsigned long long* hd = P<const volatile unsigned long long>(host_dist_);
    int T = Tmax_;
    bool tail = false;
    // published early stop: the controller kernels hand the per-env sums to the host (no marker)
    const bool pub = publish_ && early_stop;
    if (pub) {
      ++gen_;      // the per-step counters are zero: set at allocation, re-armed by the last workgroup
      hd = pub_host_;
    }
    for (int t = 0; t < Tmax_; ++t) {
      scan_step(t, st);
      ctrl_step(t, st, pub);
      // ONE marker per step on the compute queue (each marker stalls the queue behind it for
      // ~6 us: the next dispatch waits for its completion signal); both side queues wait on it
      if (overlap_ || (early_stop && !pub)) chk(hipEventRecord(ev_main_, st), "hipEventRecord");
      // CBF h of the previous step's main slots on the side stream (one step late: the slice
      // of a step beyond the early stop is never issued)
      if (overlap_ && t >= 1) {
        chk(hipStreamWaitEvent(hs, ev_main_, 0), "hipStreamWaitEvent");
        hfwd_slice(t - 1, hs);
      }
      if (early_stop) {
        if (!pub) {
          chk(hipStreamWaitEvent(cs, ev_main_, 0), "hipStreamWaitEvent");
          chk(hipMemcpyAsync(P<unsigned long long>(host_dist_) + (long)t * B_, P<const unsigned long long>(dist_) + (long)t * B_,
                             sizeof(unsigned long long) * B_, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync");
          chk(hipEventRecord(ev_copy_[t], cs), "hipEventRecord");
        }
        // host check every check_every steps (small scenes: a step's kernels take less than
        // the host round trip, so checking every step would leave the GPU idle)
        if (t >= 1 && (t % check_ == 0)) {
          if (pub) wait_published(t - 1, st);
          else chk(hipEventSynchronize(ev_copy_[t - 1]), "hipEventSynchronize");
          const int Tf = first_done(hd, t - 1);
          if (Tf > 0) {
            // every env was done after step Tf-1: the trajectory is steps 0..Tf-1; step Tf's
            // scan already gave the kNN graph / safety of s_Tf; later steps are unused
            T = Tf;
            tail = true;
            break;
          }
        }
      }
    }
    if (early_stop && !tail && check_ > 1 && Tmax_ >= 2) {
      // steps after the last strided check: same horizon as a check after every step
      if (pub) wait_published(Tmax_ - 2, st);
      else chk(hipEventSynchronize(ev_copy_[Tmax_ - 2]), "hipEventSynchronize");
      const int Tf = first_done(hd, Tmax_ - 2);
      if (Tf > 0) {
        T = Tf;
        tail = true;
      }
    }
    if (overlap_) {
      if (!tail) {
        // the side stream already waits on the marker after ctrl_fwd(T-1) unless T == 1
        if (T == 1) chk(hipStreamWaitEvent(hs, ev_main_, 0), "hipStreamWaitEvent");
        hfwd_slice(T - 1, hs);
      }
      chk(hipEventRecord(ev_side_, hs), "hipEventRecord");     // join the side stream
      chk(hipStreamWaitEvent(st, ev_side_, 0), "hipStreamWaitEvent");
    }
    return {T, tail};     // converted to a tuple after the GIL is re-acquired
  }

  // Executable graphs of the post-rollout work per horizon (index T; 0: none), captured by the
  // engine (hip_engine.py _capture_bwd): run_small(..., launch_graph) launches graph T as soon as
  // the horizon arrives, without a return to Python in between.
  void set_bwd_graphs(std::vector<u64> execs) { bwd_execs_ = std::move(execs); }

  // Persistent small-scene rollout (ctrl.hip rollout_small_kernel): the whole rollout in one
  // launch, early stop decided on the device; returns (T, true, launched) -- the kernel also scanned
  // s_T; launched: the registered graph of horizon T was launched on `stream`.
  // s0 / g0 (optional): the scenario's start states (B, N, 2D) and goals (B, N, D), loaded by the
  // kernel itself.
  std::tuple<int, bool, bool> run_small(u64 stream, bool early_stop, bool launch_graph, u64 s0, u64 g0) {
    if (!small_ctl_) throw std::runtime_error("RolloutDriver: no small-scene control buffer");
    hipStream_t st = ST(stream);
    int* ctl = P<int>(small_ctl_);
    mb::RolloutSmallArgs a{};
    mb::CtrlArgs& c = a.c;
    c.dim = D_;
    c.S = S_at(0); c.s_env = Nn_;
    c.G = P<const float>(G_);
    c.B = B_; c.N = N_; c.K = K_;
    c.wpack = P<const h16>(ctrl_w_); c.f_edge = f_edge_; c.f_node = f_node_; c.wvec = P<const float>(ctrl_v_);
    c.A = P<float>(A_);
    c.dist_sum = P<unsigned long long>(dist_); c.act_sum = P<unsigned long long>(act_);
    c.noise_key = P<const unsigned long long>(noise_key_); c.noise_prob = noise_prob_; c.noise_scale = noise_scale_;
    c.dt = dt_; c.obs_r = obs_r_; c.sqrt3 = sqrt3_;
    c.pooled = P<h16>(pooled_); c.argmax = P<uint8_t>(argmax_);
    c.apw = small_apw_;
    c.stamps = reinterpret_cast<unsigned long long*>(small_stamps_);   // diagnostics builds only (else 0)
    c.acts = P<unsigned char>(acts_); c.na_env = N_;     // per-step views offset in the kernel
    a.idx = P<int>(idx_); a.dang = P<uint8_t>(dang_); a.cnt = P<float>(cnt_);
    a.safe = safety_ ? P<float>(safe_) : nullptr;
    a.Nn = Nn_; a.Tmax = Tmax_; a.knn_tail = knn_tail_;
    a.r2_train = r2_train_; a.ttc_train = ttc_train_; a.r2_check = r2_check_; a.ttc_check = ttc_check_;
    a.done_thr = early_stop ? done_thr_ : -INFINITY;
    a.ctl = ctl;      // zero at allocation; the kernel's last workgroup re-arms it
    a.res = small_res_dev_;
    a.res_gen = (int)++small_gen_;
    a.s0 = P<const float>(s0); a.g0 = P<const float>(g0);
    if ((s0 == 0) != (g0 == 0)) throw std::invalid_argument("run_small: s0 and g0 go together");
    chk(by_prec(prec_, mb_rollout_small, mb_rollout_small_f16, mb_rollout_small_x3)(&a, st), "rollout_small");
    // the horizon arrives in host-coherent memory when the last workgroup finishes: poll it (a
    // stream synchronisation added a memset, a read-back copy and the blocking wake-up to every
    // iteration of the small configurations)
    const volatile int* res = small_res_;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned long n = 0; __atomic_load_n(&res[1], __ATOMIC_ACQUIRE) != a.res_gen; ++n) {
      if ((n & 4095) == 4095) {
        const auto dt = std::chrono::steady_clock::now() - t0;
        if (dt >= std::chrono::milliseconds(poll_query_ms_)) {
          const hipError_t e = hipStreamQuery(st);
          if (e != hipSuccess && e != hipErrorNotReady) chk(e, "rollout_small stream");
          // the stream drained without the flag: the launch did not run (never spin forever)
          if (e == hipSuccess && __atomic_load_n(&res[1], __ATOMIC_ACQUIRE) != a.res_gen)
            throw std::runtime_error("RolloutDriver: rollout_small finished without publishing its horizon");
        }
        if (dt > std::chrono::seconds(60)) throw std::runtime_error("RolloutDriver: rollout_small horizon not published");
      }
#if defined(__x86_64__)
      __builtin_ia32_pause();
#endif
    }
    const int T = res[0];
    bool launched = false;
    if (launch_graph && T >= 1 && T < (int)bwd_execs_.size() && bwd_execs_[T]) {
      chk(hipGraphLaunch(reinterpret_cast<hipGraphExec_t>(static_cast<uintptr_t>(bwd_execs_[T])), st), "hipGraphLaunch");
      launched = true;
    }
    return {T, true, launched};
  }

 private:
  // Smallest T' (1 <= T' <= t+1) such that every env was done after step T'-1 (env b is done
  // from the first step q_b whose mean goal distance is below the threshold: T' = max_b q_b + 1),
  // or 0 if some env is not done by step t. Checking after every step and breaking at the first
  // hit gives the same T'.
  int first_done(const volatile unsigned long long* hd, int t) const {
    int last = -1;
    for (int b = 0; b < B_; ++b) {
      int q = 0;      // same float arithmetic as rollout_stats_kernel
      while (q <= t && !((float)((double)hd[(long)q * B_ + b] / mb::FX_DIST) / (float)N_ < done_thr_)) ++q;
      if (q > t) return 0;
      if (q > last) last = q;
    }
    return last + 1;
  }

  const float4* S_at(int t) const { return P<const float4>(S_) + (long)t * B_ * Nn_ * (W_ / 4); }

  // Waits until the controller kernel of step t has published its per-env sums (flag == this
  // rollout's generation). Polls host-coherent memory; a stream error or a minute without the
  // flag raises instead of spinning forever.
  void wait_published(int t, hipStream_t st) const {
    const unsigned* flag = reinterpret_cast<const unsigned*>(pub_host_ + (size_t)Tmax_ * B_) + t;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned long n = 0; __atomic_load_n(flag, __ATOMIC_ACQUIRE) != gen_; ++n) {
      if ((n & 4095) == 4095) {
        // the stream-error probe only after poll_query_ms_ of waiting (a step publishes within a
        // millisecond): hipStreamQuery on a busy stream enqueues a marker, and the marker stalled
        // the queue behind it -- the ~6 us gap after every controller step (trace median 5.66 ->
        // 0 us, headline -0.05 ms, profiles/r5_b8/; MACBF_POLL_QUERY_MS=0: probe every 4096 polls)
        const auto dt = std::chrono::steady_clock::now() - t0;
        if (dt >= std::chrono::milliseconds(poll_query_ms_)) {
          const hipError_t e = hipStreamQuery(st);
          if (e != hipSuccess && e != hipErrorNotReady) chk(e, "rollout stream");
        }
        if (dt > std::chrono::seconds(60))
          throw std::runtime_error("RolloutDriver: early-stop flag of step " + std::to_string(t) + " not published");
      }
#if defined(__x86_64__)
      __builtin_ia32_pause();
#endif
    }
  }

  void scan_step(int t, hipStream_t st) {
    if (t % resort_ == 0) {
      mb::CellSortArgs c{};
      c.S = S_at(t); c.s_env = Nn_; c.B = B_; c.N = Nn_; c.L = L_; c.perm = P<int>(perm_); c.rec = W_ / 4;
      chk(mb_cell_sort(&c, st), "cell_sort");
    }
    mb::ScanArgs a{};
    a.S = S_at(t); a.s_env = Nn_; a.perm = P<const int>(perm_);
    a.B = B_; a.N = N_; a.K = K_; a.Nn = Nn_; a.dim = D_;
    const long nk = (long)N_ * K_;
    a.idx = P<int>(idx_) + (long)t * B_ * nk; a.i_env = nk;
    a.dang = P<uint8_t>(dang_) + (long)t * B_ * nk;
    a.cnt = P<float>(cnt_) + (long)t * B_ * 2; a.c_env = 2;
    a.safe = safety_ ? P<float>(safe_) + (long)t * B_ : nullptr; a.sf_env = 1;
    a.r2_train = r2_train_; a.ttc_train = ttc_train_; a.r2_check = r2_check_; a.ttc_check = ttc_check_;
    a.do_knn = 1; a.do_safety = safety_;
    a.prev_idx = t > 0 ? P<const int>(idx_) + (long)(t - 1) * B_ * nk : nullptr; a.pi_env = nk;
    a.ws = P<float4>(scan_ws_); a.ws_env = scan_ws_env_;
    chk(mb_scan(&a, st), "scan");
  }

  void ctrl_step(int t, hipStream_t st, bool pub = false) {
    mb::CtrlArgs a{};
    if (pub) {
      a.pub_ctr = pub_ctr_ + t;
      a.pub_dist = pub_dev_ + (long)t * B_;
      a.pub_flag = reinterpret_cast<unsigned*>(pub_dev_ + (size_t)Tmax_ * B_) + t;
      a.pub_gen = gen_;
    }
    a.dim = D_;
    a.S = S_at(t); a.s_env = Nn_;
    a.G = P<const float>(G_);
    const long nk = (long)N_ * K_;
    a.idx = P<const int>(idx_) + (long)t * B_ * nk; a.i_env = nk;
    a.acts = acts_ ? P<unsigned char>(acts_) + (long)t * B_ * N_ * act_bytes_ : nullptr; a.na_env = N_;
    a.B = B_; a.N = N_; a.K = K_;
    a.wpack = P<const h16>(ctrl_w_); a.f_edge = f_edge_; a.f_node = f_node_; a.wvec = P<const float>(ctrl_v_);
    a.A = P<float>(A_) + (long)t * B_ * N_ * D_; a.a_env = N_;
    a.Snext = const_cast<float4*>(S_at(t + 1)); a.sn_env = Nn_;
    a.dist_sum = P<unsigned long long>(dist_) + (long)t * B_; a.d_env = 1;
    a.act_sum = P<unsigned long long>(act_) + (long)t * B_; a.ac_env = 1;
    a.noise = nullptr; a.n_env = 0;
    a.noise_key = P<const unsigned long long>(noise_key_); a.noise_prob = noise_prob_; a.noise_scale = noise_scale_;
    a.noise_t = t;
    a.dt = dt_; a.obs_r = obs_r_; a.sqrt3 = sqrt3_;
    a.pooled = P<h16>(pooled_) + (long)t * B_ * N_ * prow_; a.p_env = (long)N_ * prow_;
    a.argmax = P<uint8_t>(argmax_) + (long)t * B_ * N_ * 128; a.am_env = (long)N_ * 128;
    a.apw = apw_;
    chk(by_prec(prec_, mb_ctrl_fwd, mb_ctrl_fwd_f16, mb_ctrl_fwd_x3)(&a, num_cu_, st), "ctrl_fwd");
  }

  // CBF h of the main slots of step t, evaluations [t*BNK, (t+1)*BNK), on the side stream
  void hfwd_slice(int t, hipStream_t hs) {
    mb::CbfFwdArgs a{};
    a.dim = D_;
    const long bnk = (long)B_ * N_ * K_;
    a.S = P<const float4>(S_); a.s_env = Nn_; a.s_step = (long)B_ * Nn_;
    a.idx = P<const int>(idx_); a.idx1 = a.idx; a.src = P<const int>(src_); a.nev = P<const int>(nev_);
    a.B = B_; a.T = t + 1; a.N = N_; a.K = K_; a.two = 1;
    a.wpack = P<const h16>(cbf_w_); a.f_fwd = f_fwd_; a.wrm = P<const h16>(cbf_rm_);
    a.wvec = P<const float>(cbf_v_);
    a.h_out = P<float>(hbuf_); a.mask_out = P<uint8_t>(hmask_);
    a.obs_r = obs_r_; a.dist_thr = dist_thr_; a.dist_eps = dist_eps_;
    a.u_begin = (unsigned)(t * bnk); a.u_end = (unsigned)((t + 1) * bnk);
    chk(by_prec(prec_, mb_cbf_hfwd, mb_cbf_hfwd_f16, mb_cbf_hfwd_x3)(&a, hfwd_blocks_, hs), "cbf_hfwd");
  }

  int B_, N_, Nn_, K_, D_, W_, Tmax_, num_cu_, prec_, prow_, resort_, safety_, overlap_, hfwd_blocks_, check_, apw_;
  int publish_ = 0;
  unsigned gen_ = 0;
  int poll_query_ms_ = 100;
  unsigned long long* pub_host_ = nullptr;   // host view: [Tmax][B] sums, then [Tmax] flags
  unsigned long long* pub_dev_ = nullptr;    // the same memory, device view
  unsigned* pub_ctr_ = nullptr;              // [Tmax] per-step workgroup counters (device)
  float L_;
  u64 S_, G_, A_, idx_, dang_, cnt_, safe_, dist_, act_, pooled_, argmax_, perm_, host_dist_;
  u64 ctrl_w_, ctrl_v_, cbf_w_, cbf_rm_, cbf_v_, hbuf_, hmask_, src_, nev_, noise_key_;
  float noise_prob_, noise_scale_;
  u64 scan_ws_;
  long scan_ws_env_;
  u64 small_ctl_ = 0, small_stamps_ = 0, acts_ = 0;
  long act_bytes_ = 0;
  int small_apw_ = 0, knn_tail_ = 0;
  std::vector<u64> bwd_execs_;
  int* small_res_ = nullptr;                 // host-coherent [T, flag] of the persistent rollout
  int* small_res_dev_ = nullptr;             // its device view
  unsigned small_gen_ = 0;
  int f_edge_, f_node_, f_fwd_;
  float r2_train_, ttc_train_, r2_check_, ttc_check_, dt_, obs_r_, sqrt3_, dist_thr_, dist_eps_, done_thr_;
  std::vector<hipEvent_t> ev_copy_;
  hipEvent_t ev_main_ = nullptr, ev_side_ = nullptr;
};

// Native BPTT driver: the reverse-time loop of the controller backward (hand-derived adjoints
// of train.py:58-103's autograd through the rollout). Per step t = T-1..0:
//   ctrl_node_bwd(t)  <- G_{t+1} (dS_T for the last step)
//   ctrl_edge_bwd(t)
//   node_combine(t)   -> G_t
// over the engine's persistent time-major buffers (pointer offsets validated once in Python).
// Three dependent launches per step: the loop is GPU-bound at 1024 x 64 agents but host-bound
// for small scenes (BASELINE config #2: 32 agents), where Python paid ~15 us per launch.
class BpttDriver {
 public:
  explicit BpttDriver(py::dict cfg) {
    Args c("BpttDriver", cfg);
    c("B", B_); c("N", N_); c("Nn", Nn_); c("K", K_); c("D", D_);
    R_ = D_ == 2 ? 1 : 2;
    c("Tmax", Tmax_); c("prec", prec_); prow_ = prec_ == 2 ? 256 : 128; c("nb_node", nb_node_); c("nb_edge", nb_edge_);
    c("qsplit", qsplit_);
    c("pooled", pooled_); c("S", S_); c("G", G_); c("A", A_); c("dS", dS_); c("Gb", Gb_); c("valid", valid_);
    c("idx", idx_); c("argmax", argmax_); c("rptr", rptr_); c("redges", redges_);
    c("ctrl_rm", wrm_); c("o_w1", o1_); c("o_w2", o2_); c("o_w3", o3_); c("o_w4", o4_);
    c("ctrl_v", wvec_); c("act_scale", act_scale_); c("dP", dP_); c("ego", ego_); c("dEc", dEc_);
    c("part_node", part_node_); c("part_edge", part_edge_);
    c("ctrl_w", wpack_); c("f_ew1f", f_ew1f_); c("f_ew2tn", f_ew2tn_);
    c("dt", dt_); c("sqrt3", sqrt3_);
    c("node_chunk", node_chunk_);
    // per-step slab rows (small grids): step t's node / edge workgroups write rows (T-1-t) x grid
    // of the slabs instead of accumulating into one row per workgroup
    c.opt("step_rows", step_rows_);
    c.opt("node_acts", acts_);
    c.opt("node_act_bytes", act_bytes_);
    c.opt("node_part", node_part_);
    c.opt("edge_part", edge_part_);
    if (step_rows_ && (node_part_ <= 0 || edge_part_ <= 0))
      throw std::invalid_argument("BpttDriver: step_rows needs the slab row sizes");
    c.opt("fused_step", fused_);
    if (fused_ && (node_chunk_ != 32 || nb_node_ != nb_edge_))
      throw std::invalid_argument("BpttDriver: the fused step needs 32-agent chunks and one grid");
    c.opt("gscale", gscale_);       // fp16: device loss scale (or 0)
    c.opt("ctrl_w16", ew16_);       // K = 12: 16x16x32 edge backward fragments
    c.opt("node_rm16", nw16_);      // 128-agent chunks: 16x16x32 node backward images
    if (nw16_ && (node_chunk_ != 128 || fused_))
      throw std::invalid_argument("BpttDriver: the 16x16x32 node backward needs 128-agent chunks");
    if (B_ < 1 || N_ < 1 || Nn_ < N_ || K_ < 1 || K_ > 16 || (D_ != 2 && D_ != 3) || Tmax_ < 1 || nb_node_ < 1 ||
        nb_edge_ < 1)
      throw std::invalid_argument("BpttDriver: bad dimensions");
  }

  // use_acts: this iteration's rollout kept the node activations (RolloutDriver with node_acts)
  void run(int T, float act_coef, u64 stream, bool use_acts) {
    if (T < 1 || T > Tmax_) throw std::invalid_argument("BpttDriver: T out of range");
    hipStream_t st = ST(stream);
    const long BN = (long)B_ * N_;
    const long nk = (long)N_ * K_;
    for (int t = T - 1; t >= 0; --t) {
      const float4* Gn = P<const float4>(dS_) + (long)T * BN * R_;       // t = T-1: the direct terms dS_T
      const float4* St = P<const float4>(S_) + (long)t * B_ * Nn_ * R_;
      mb::CtrlNodeBwdArgs na{};
      mb::CtrlEdgeBwdArgs ea{};
      {
        mb::CtrlNodeBwdArgs& a = na;
        a.dim = D_;
        a.pooled = P<const h16>(pooled_) + (long)t * BN * prow_; a.p_env = (long)N_ * prow_;
        a.S = St; a.s_env = Nn_;
        a.G = P<const float>(G_); a.A = P<const float>(A_) + (long)t * BN * D_; a.a_env = N_;
        a.Gn = Gn; a.gn_env = N_;
        a.valid = P<const uint8_t>(valid_) + (long)t * B_; a.v_env = 1;
        a.B = B_; a.N = N_;
        a.wrm = P<const h16>(wrm_); a.o_w1 = o1_; a.o_w2 = o2_; a.o_w3 = o3_; a.o_w4 = o4_;
        a.wvec = P<const float>(wvec_); a.act_coef = act_coef; a.act_scale = P<const float>(act_scale_);
        a.gscale = P<const float>(gscale_);
        a.dt = dt_; a.sqrt3 = sqrt3_;
        a.dP = P<h16>(dP_); a.dp_env = (long)N_ * prow_; a.ego = P<float4>(ego_); a.partial = P<float>(part_node_);
        a.init = t == T - 1;     // the first step of the reverse loop writes the slabs
        if (step_rows_) {
          a.partial += (long)(T - 1 - t) * nb_node_ * node_part_;
          a.init = 1;
        }
        a.chunk = node_chunk_;
        a.acts = (use_acts && acts_) ? P<const unsigned char>(acts_) + (long)t * BN * act_bytes_ : nullptr;
        a.na_env = N_;
        a.wrm16 = P<const h16>(nw16_);
        a.K = K_;
        if (t < T - 1) {
          // fused BPTT combine: G_{t+1} from step t+1's records (dS, ego, dEc, graph t+1, G_{t+2})
          const long t1 = t + 1;
          a.cdS = P<const float4>(dS_) + t1 * BN * R_; a.cds_env = N_;
          // dEc is double-buffered by step parity: step t+1's edge records sit in buffer (t+1)&1
          // while step t's edge phase writes buffer t&1 (the fused launch overlaps the two)
          a.cego = P<const float4>(ego_); a.cdEc = P<const float4>(dEc_) + (t1 & 1) * BN * K_ * R_;
          a.cptr = P<const int>(rptr_) + t1 * B_ * (Nn_ + 1); a.cptr_env = Nn_ + 1;
          a.cedges = P<const int>(redges_) + t1 * B_ * nk; a.cedges_env = nk;
          a.cGn = (t1 == T - 1 ? P<const float4>(dS_) + (long)T * BN * R_ : P<const float4>(Gb_) + (t1 + 1) * BN * R_);
          a.cgn_env = N_;
          a.cGout = P<float4>(Gb_) + t1 * BN * R_; a.cgo_env = N_;
        }
      }
      {
        mb::CtrlEdgeBwdArgs& a = ea;
        a.dim = D_;
        a.S = St; a.s_env = Nn_;
        a.idx = P<const int>(idx_) + (long)t * B_ * nk; a.i_env = nk;
        a.argmax = P<const uint8_t>(argmax_) + (long)t * BN * 128; a.am_env = (long)N_ * 128;
        a.dP = P<const h16>(dP_); a.dp_env = (long)N_ * prow_;
        a.B = B_; a.N = N_; a.K = K_;
        a.wpack = P<const h16>(wpack_); a.f_ew1f = f_ew1f_; a.f_ew2tn = f_ew2tn_;
        a.dEc = P<float4>(dEc_) + (long)(t & 1) * BN * K_ * R_; a.de_env = nk; a.partial = P<float>(part_edge_);
        a.qsplit = qsplit_;
        a.init = t == T - 1;
        if (step_rows_) {
          a.partial += (long)(T - 1 - t) * nb_edge_ * edge_part_;
          a.init = 1;
        }
        a.w16 = fused_ ? nullptr : P<const h16>(ew16_);   // (the fused step keeps its own edge phase)
      }
      if (fused_) {      // node + edge backward of the same 32-agent chunks in one launch
        chk(by_prec(prec_, mb_ctrl_bwd_step, mb_ctrl_bwd_step_f16, mb_ctrl_bwd_step_x3)(&na, &ea, nb_node_, st),
            "ctrl_bwd_step");
      } else {
        chk(by_prec(prec_, mb_ctrl_node_bwd, mb_ctrl_node_bwd_f16, mb_ctrl_node_bwd_x3)(&na, nb_node_, st),
            "ctrl_node_bwd");
        chk(by_prec(prec_, mb_ctrl_edge_bwd, mb_ctrl_edge_bwd_f16, mb_ctrl_edge_bwd_x3)(&ea, nb_edge_, st),
            "ctrl_edge_bwd");
      }
      // (no combine launch: the next step's node backward forms G_t in its prologue; G_0 = dL/ds_0
      // is not needed -- s_0 is sampled, not a function of the weights)
    }
  }

 private:
  int B_, N_, Nn_, K_, D_, R_, Tmax_, prec_, prow_, nb_node_, nb_edge_, qsplit_, node_chunk_ = 0, fused_ = 0;
  int step_rows_ = 0;
  long node_part_ = 0, edge_part_ = 0, act_bytes_ = 0;
  u64 acts_ = 0;
  u64 pooled_, S_, G_, A_, dS_, Gb_, valid_, idx_, argmax_, rptr_, redges_, wrm_, wvec_, act_scale_, dP_, ego_, dEc_;
  u64 part_node_, part_edge_, wpack_, gscale_ = 0, ew16_ = 0, nw16_ = 0;
  int o1_, o2_, o3_, o4_, f_ew1f_, f_ew2tn_;
  float dt_, sqrt3_;
};

// One call of the safety filter: the kernels' arguments (all but r.it) and how they are launched
struct RefineCall {
  mb::RefineSmallArgs sa;       // sa.r: both filters; sa.ew: the persistent filter's result words
  int num_blocks, prec;         // num_blocks: refine_grad's grid (the loop filter's alone, as r.dEv and r.ctl)
};

RefineCall refine_call(Args& x) {
  RefineCall c{};
  mb::RefineArgs& r = c.sa.r;
  x("S", r.S); x("s_env", r.s_env); x("dim", r.dim); x("idx", r.idx); x("a", r.a); x("delta", r.delta);
  x("h", r.h); x("B", r.B); x("N", r.N); x("Nn", r.Nn); x("K", r.K); x("wpack", r.wpack);
  x("f_bwd", r.f_bwd); x("wrm", r.wrm); x("wvec", r.wvec); x("ptr", r.ptr); x("edges", r.edges);
  x.opt("dEv", r.dEv); x.opt("ctl", r.ctl); x("dt", r.dt); x("dt_alpha", r.dt_alpha); x("lr", r.lr);
  x("obs_r", r.obs_r); x("dist_thr", r.dist_thr); x("dist_eps", r.dist_eps); x("hn_out", r.hn_out);
  x("flag_out", r.flag_out); x("env_active", r.env_active); x("loops", c.sa.loops); x.opt("ew", c.sa.ew);
  x.opt("num_blocks", c.num_blocks); x("prec", c.prec);
  return c;
}

// Safety-filter loop (csrc/refine.hip): `loops` x (refine_grad, refine_update) on the caller's
// stream. The pointers and sizes are validated once; the control words (2 per iteration) are
// cleared here; nothing is allocated or built; no host synchronisation -- the early-out lives in the
// kernels. r.hn_out / r.flag_out (optional) receive the first iteration's h(s') and hinge flags.
// r.env_active (optional, (B,) bytes on the device) is handed to the kernels as it is: never read here.
int refine_loop(const RefineCall* c, hipStream_t st) {
  mb::RefineArgs r = c->sa.r;
  const int loops = c->sa.loops;
  if ((r.dim != 2 && r.dim != 3) || r.B < 1 || r.N < 1 || r.Nn < r.N || r.K < 1 || r.K > 16 || loops < 0 ||
      c->num_blocks < 1 || r.f_bwd < 0 || r.s_env < r.Nn || c->prec < 0 || c->prec > 2)
    return -1;
  if (!r.S || !r.idx || !r.a || !r.delta || !r.h || !r.wpack || !r.wrm || !r.wvec || !r.dEv || !r.ptr || !r.edges || !r.ctl)
    return -2;
  if (loops == 0) return 0;
  const hipError_t e = hipMemsetAsync(r.ctl, 0, (size_t)loops * 2 * sizeof(unsigned long long), st);
  if (e != hipSuccess) return (int)e;
  const auto grad = by_prec(c->prec, mb_refine_grad, mb_refine_grad_f16, mb_refine_grad_x3);
  const int pr = by_prec(c->prec, mb_refine_prepare, mb_refine_prepare_f16, mb_refine_prepare_x3)(r.dim);
  if (pr) return pr;
  for (r.it = 0; r.it < loops; ++r.it) {
    int rc = grad(&r, c->num_blocks, st);
    if (rc) return rc;
    rc = mb_refine_update(&r, st);
    if (rc) return rc;
    r.hn_out = nullptr;
    r.flag_out = nullptr;
  }
  return 0;
}

// Persistent safety filter for small envs (csrc/refine.hip refine_small_kernel): the whole loop of
// every env in ONE launch on the caller's stream, one workgroup per env. The pointers and sizes are
// validated once; the kernel's dynamic-LDS attribute is set by its launcher; nothing is allocated
// or cleared here (delta and ew (B, loops, 2) arrive zeroed); no host synchronisation. The kernel
// writes r.hn_out / r.flag_out at iteration 0 only.
int refine_small(const RefineCall* c, hipStream_t st) {
  const mb::RefineArgs& r = c->sa.r;
  if (r.dim != 2 && r.dim != 3) return -1;
  if (r.B < 1 || r.N < 1 || r.Nn < r.N || r.K < 1 || r.K > 16 || c->sa.loops < 0 || r.f_bwd < 0 || r.s_env < r.Nn) return -1;
  if (r.Nn > 64) return -4;                                    // SMALL_MAXN: the env must fit one workgroup's LDS
  if (c->prec < 0 || c->prec > 2) return -1;
  if (!r.S || !r.idx || !r.a || !r.delta || !r.h || !r.wpack || !r.wrm || !r.wvec || !r.ptr || !r.edges || !c->sa.ew) return -2;
  if (c->sa.loops == 0) return 0;
  return by_prec(c->prec, mb_refine_small, mb_refine_small_f16, mb_refine_small_x3)(&c->sa, st);
}

// The arguments of the three launches of csrc/episode.hip (the driver sets S_cur / S_next per step)
mb::EpisodeArgs episode_args(Args& x) {
  mb::EpisodeArgs e{};
  x.opt("S_cur", e.S_cur); x.opt("S_next", e.S_next); x("s_env", e.s_env); x("dim", e.dim); x("B", e.B);
  x("N", e.N); x("A", e.A); x("delta", e.delta); x("G", e.G); x("dt", e.dt); x("st", e.st);
  x("dist_fx", e.dist_fx); x("safe", e.safe); x("active", e.active); x("prev_active", e.prev_active);
  x("ctl", e.ctl); x("ew", e.ew); x("loops", e.loops); x("mode", e.mode); x("thr", e.thr); x("out", e.out);
  e.thr_fx = (unsigned long long)std::llrint((double)e.thr * (double)e.N * mb::FX_DIST);
  return e;
}

// Closed-loop episode driver (csrc/episode.hip): a whole batch of episodes -- validation during
// training, evaluation -- with or without the safety filter, as one call. Per step, on the caller's
// stream: cell_sort + ONE scan of s_t (kNN and the safety count of the step before), the controller
// forward, the filter (cbf_fwd for h(s_t), rev_csr, refine_loop or refine_small), episode_advance,
// episode_tally, and a swap of the two record buffers. The buffers come from Python
// (ops/episode.py), validated there once per call; nothing is allocated and the host does not wait
// inside a step. Every check_every steps the "some env still runs" word is copied to pinned memory
// and the stream is waited for; a step issued after every env finished changes nothing, so the
// result does not depend on that period. After the loop: the safety-only scan of the final state
// and episode_final.
class EpisodeDriver {
 public:
  EpisodeDriver() {
    chk(hipHostMalloc((void**)&alive_host_, sizeof(long long), hipHostMallocDefault), "hipHostMalloc");
    *alive_host_ = 1;
  }
  ~EpisodeDriver() {
    if (alive_host_) (void)hipHostFree(alive_host_);
  }
  EpisodeDriver(const EpisodeDriver&) = delete;
  EpisodeDriver& operator=(const EpisodeDriver&) = delete;

  struct Cfg {
    mb::EpisodeArgs e;          // all but S_cur / S_next (per step); e.mode != 0: the filter runs
    RefineCall r;               // the filter's, all but S (per step)
    int Nn, K, num_cu, prec_ctrl, apw, max_steps, check_every, mask_done, cbf_blocks, f_edge, f_node;
    float L, r2_train, ttc_train, r2_check, ttc_check, obs_r, sqrt3;
    u64 S0, S1, idx, pooled, argmax, perm, ctrl_w, ctrl_v, csr_ws, scan_ws;
    long scan_ws_env;
    mb::LossConsts lc;
    hipStream_t stream;
  };

  // Returns (steps issued, 0 or 1: the buffer that holds the final state).
  std::pair<int, int> run(py::dict c) {
    Cfg g = parse(c);
    py::gil_scoped_release nogil;       // the loop waits for the stream every check_every steps
    return loop(g);
  }

 private:
  // cfg: the driver's own keys, "episode": the EpisodeArgs fields, "refine": the RefineArgs fields or None
  static Cfg parse(const py::dict& c) {
    Args x("EpisodeDriver", c);
    Cfg g{};
    bool none = false;
    Args ex = x.sub("episode"), rx = x.sub("refine", &none);
    g.e = episode_args(ex);
    ex.done();
    if (!none) g.r = refine_call(rx);
    rx.done();
    const mb::EpisodeArgs& e = g.e;
    const bool filter = e.mode != 0;
    x("Nn", g.Nn); x("K", g.K); x("num_cu", g.num_cu); x("prec_ctrl", g.prec_ctrl); x("apw", g.apw);
    x("max_steps", g.max_steps); x("check_every", g.check_every); x("mask_done", g.mask_done);
    x("cbf_blocks", g.cbf_blocks); x("f_edge", g.f_edge); x("f_node", g.f_node); x("L", g.L);
    x("r2_train", g.r2_train); x("ttc_train", g.ttc_train); x("r2_check", g.r2_check); x("ttc_check", g.ttc_check);
    x("obs_r", g.obs_r); x("sqrt3", g.sqrt3); x("S0", g.S0); x("S1", g.S1); x("idx", g.idx); x("pooled", g.pooled);
    x("argmax", g.argmax); x("perm", g.perm); x("ctrl_w", g.ctrl_w); x("ctrl_v", g.ctrl_v); x("csr_ws", g.csr_ws);
    x("scan_ws", g.scan_ws); x("scan_ws_env", g.scan_ws_env);
    g.lc = x.loss_consts<mb::LossConsts>("loss_consts"); g.stream = ST(x.u("stream"));
    x.done();
    if (e.B < 1 || e.N < 1 || g.Nn < e.N || e.s_env != g.Nn || g.K < 1 || g.K > 16 || g.K > g.Nn || (e.dim != 2 && e.dim != 3) ||
        g.max_steps < 0 || e.loops < 0 || e.mode < 0 || e.mode > 2 || g.prec_ctrl < 0 || g.prec_ctrl > 2 || filter == none)
      throw std::invalid_argument("EpisodeDriver: bad dimensions");
    if (g.check_every < 1) g.check_every = 1;
    if (!g.S0 || !g.S1 || g.S0 == g.S1 || !e.G || !g.idx || !e.A || !g.argmax || !g.perm || !e.safe || !e.st ||
        !e.dist_fx || !e.active || !e.prev_active || !e.out || !g.ctrl_w || !g.ctrl_v || (g.prec_ctrl == 2 && !g.pooled))
      throw std::invalid_argument("EpisodeDriver: a required buffer is missing");
    if (filter) {
      const mb::RefineArgs& r = g.r.sa.r;
      if (g.r.prec == 1) throw std::invalid_argument("EpisodeDriver: the safety filter has no fp16 build");
      if (r.B != e.B || r.N != e.N || r.Nn != g.Nn || r.K != g.K || r.dim != e.dim || e.loops < 1 ||
          g.r.sa.loops != e.loops || g.r.sa.ew != e.ew || g.r.prec < 0 || g.r.prec > 2 || r.idx != P<const int>(g.idx))
        throw std::invalid_argument("EpisodeDriver: bad dimensions");
      if (!r.wpack || !r.wrm || !r.wvec || !r.delta || r.delta != e.delta || !r.h || !r.ptr || !r.edges || g.cbf_blocks < 1)
        throw std::invalid_argument("EpisodeDriver: a filter buffer is missing");
      if (e.mode == 2 ? (!e.ew || g.Nn > 64) : (!r.dEv || !r.ctl || g.r.num_blocks < 1))
        throw std::invalid_argument("EpisodeDriver: the filter's result words / workspace are missing");
    }
    return g;
  }

  std::pair<int, int> loop(const Cfg& g) {
    hipStream_t st = g.stream;
    u64 S[2] = {g.S0, g.S1};
    int cur = 0, t = 0;
    mb::EpisodeArgs e = g.e;
    for (; t < g.max_steps;) {
      scan(g, S[cur], true, st);
      ctrl(g, S[cur], st);
      if (e.mode) refine(g, S[cur], st);
      e.S_cur = P<const float4>(S[cur]); e.S_next = P<float4>(S[cur ^ 1]);
      chk(mb_episode_advance(&e, st), "episode_advance");
      chk(mb_episode_tally(&e, st), "episode_tally");
      cur ^= 1;
      ++t;
      if (t % g.check_every == 0 && t < g.max_steps) {
        chk(hipMemcpyAsync(alive_host_, e.st + mb::EP_ALIVE, sizeof(long long), hipMemcpyDeviceToHost, st),
            "hipMemcpyAsync");
        chk(hipStreamSynchronize(st), "hipStreamSynchronize");
        if (*alive_host_ == 0) break;
      }
    }
    scan(g, S[cur], false, st);           // the safety count of the final state
    e.S_cur = P<const float4>(S[cur]); e.S_next = nullptr;
    chk(mb_episode_final(&e, st), "episode_final");
    return {t, cur};
  }

  void scan(const Cfg& g, u64 S, bool knn, hipStream_t st) {
    const mb::EpisodeArgs& e = g.e;
    const int R = e.dim == 2 ? 1 : 2;
    mb::CellSortArgs c{};
    c.S = P<const float4>(S); c.s_env = g.Nn; c.B = e.B; c.N = g.Nn; c.L = g.L; c.perm = P<int>(g.perm); c.rec = R;
    chk(mb_cell_sort(&c, st), "cell_sort");
    mb::ScanArgs a{};
    a.S = P<const float4>(S); a.s_env = g.Nn; a.perm = P<const int>(g.perm);
    a.B = e.B; a.N = e.N; a.K = knn ? g.K : 1; a.Nn = g.Nn; a.dim = e.dim;
    a.idx = knn ? P<int>(g.idx) : nullptr; a.i_env = knn ? (long)e.N * g.K : 0;
    a.safe = e.safe; a.sf_env = 1;
    a.r2_train = g.r2_train; a.ttc_train = g.ttc_train; a.r2_check = g.r2_check; a.ttc_check = g.ttc_check;
    a.do_knn = knn ? 1 : 0; a.do_safety = 1;
    a.ws = P<float4>(g.scan_ws); a.ws_env = g.scan_ws_env;
    chk(mb_scan(&a, st), "scan");
  }

  void ctrl(const Cfg& g, u64 S, hipStream_t st) {
    const mb::EpisodeArgs& e = g.e;
    const int prow = g.prec_ctrl == 2 ? 256 : 128;
    mb::CtrlArgs a{};
    a.dim = e.dim; a.apw = g.apw;
    a.S = P<const float4>(S); a.s_env = g.Nn; a.G = e.G;
    a.idx = P<const int>(g.idx); a.i_env = (long)e.N * g.K;
    a.B = e.B; a.N = e.N; a.K = g.K;
    a.wpack = P<const h16>(g.ctrl_w); a.f_edge = g.f_edge; a.f_node = g.f_node; a.wvec = P<const float>(g.ctrl_v);
    a.A = const_cast<float*>(e.A); a.a_env = e.N;
    a.dt = e.dt; a.obs_r = g.obs_r; a.sqrt3 = g.sqrt3;
    a.pooled = P<h16>(g.pooled); a.p_env = (long)e.N * prow;
    a.argmax = P<uint8_t>(g.argmax); a.am_env = (long)e.N * 128;
    chk(by_prec(g.prec_ctrl, mb_ctrl_fwd, mb_ctrl_fwd_f16, mb_ctrl_fwd_x3)(&a, g.num_cu, st), "ctrl_fwd");
  }

  void refine(const Cfg& g, u64 S, hipStream_t st) {
    const mb::EpisodeArgs& e = g.e;
    RefineCall c = g.r;
    mb::RefineArgs& r = c.sa.r;
    r.S = P<const float4>(S);
    mb::CbfFwdArgs a{};
    a.S = r.S; a.s_env = g.Nn; a.s_step = (long)e.B * g.Nn; a.idx = P<const int>(g.idx);
    a.B = e.B; a.T = 1; a.N = e.N; a.K = g.K; a.two = 0;
    a.wpack = r.wpack; a.f_fwd = r.f_bwd; a.wvec = r.wvec;
    a.h_out = const_cast<float*>(r.h);       // the step's h(s_t) and reverse CSR are written here, read by the filter
    a.dim = e.dim; a.lc = g.lc;
    a.obs_r = r.obs_r; a.dist_thr = r.dist_thr; a.dist_eps = r.dist_eps;
    chk(by_prec(c.prec, mb_cbf_fwd, mb_cbf_fwd_f16, mb_cbf_fwd_x3)(&a, g.cbf_blocks, st), "cbf_fwd");
    mb::CsrArgs v{};
    v.idx = P<const int>(g.idx); v.G = e.B; v.N = e.N; v.K = g.K; v.Nn = g.Nn;
    v.ptr = const_cast<int*>(r.ptr); v.edges = const_cast<int*>(r.edges); v.ws = P<int>(g.csr_ws);
    chk(mb_rev_csr(&v, st), "rev_csr");
    if (!g.mask_done) r.env_active = nullptr;        // validate.py's rule: a finished env is not refined
    if (e.mode == 2) chk(refine_small(&c, st), "refine_small");
    else chk(refine_loop(&c, st), "refine_loop");
  }

  long long* alive_host_ = nullptr;
};

}  // namespace

void register_runtime(py::module& m) {
  def_launch(m, "refine_loop", refine_call, refine_loop);
  def_launch(m, "refine_small", refine_call, refine_small);
  // the three launches of csrc/episode.hip on their own, as EpisodeDriver issues them per step
  def_launch(m, "episode_advance", episode_args, mb_episode_advance);
  def_launch(m, "episode_tally", episode_args, mb_episode_tally);
  def_launch(m, "episode_final", episode_args, mb_episode_final);
  py::class_<EpisodeDriver>(m, "EpisodeDriver")
      .def(py::init<>())
      .def("run", &EpisodeDriver::run, py::arg("cfg"));
  py::class_<BpttDriver>(m, "BpttDriver")
      .def(py::init<py::dict>())
      .def("run", &BpttDriver::run, py::arg("T"), py::arg("act_coef"), py::arg("stream"), py::arg("use_acts") = false);
  py::class_<RolloutDriver>(m, "RolloutDriver")
      .def(py::init<py::dict>())
      .def("set_bwd_graphs", &RolloutDriver::set_bwd_graphs, py::arg("execs"))
      .def("run_small", &RolloutDriver::run_small, py::arg("stream"), py::arg("early_stop"),
           py::arg("launch_graph") = false, py::arg("s0") = 0, py::arg("g0") = 0,
           py::call_guard<py::gil_scoped_release>())
      .def("run", &RolloutDriver::run, py::arg("stream"), py::arg("hstream"), py::arg("copy_stream"),
           py::arg("early_stop"),
           // the loop blocks on hipEventSynchronize: let other Python threads run meanwhile
           py::call_guard<py::gil_scoped_release>());
}
