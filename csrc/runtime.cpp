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
// issued). From the step at which the previous rollout ended, the check moves in front of the
// controller step instead (run(): the zero-lag check), so the step past the horizon is not issued.
// Per-env done masks are applied on the device afterwards (rollout_stats).
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

#include "fill.h"

namespace {

hipStream_t ST(u64 s) { return reinterpret_cast<hipStream_t>(static_cast<uintptr_t>(s)); }

class RolloutDriver {
 public:
  // cfg: the driver's own keys and, as dicts, the arguments of its launches at step 0 -- what the
  // builders of ops/native.py make of the engine's step-0 views (hfwd: of the whole time-major buffers,
  // None without the overlapped CBF slices). Every key is read before the first HIP call.
  explicit RolloutDriver(py::dict cfg) {
    Args c("RolloutDriver", cfg);
    c("Tmax", Tmax_); c("resort_every", resort_); c("check_every", check_); c("hfwd_blocks", hfwd_blocks_);
    c("num_cu", num_cu_); c("prec", prec_); c("host_dist", host_dist_); c("done_thr", done_thr_);
    // early-stop publication (ctrl.hip publish_step): per-step workgroup counters on the device,
    // the per-env sums and a flag per step in host-coherent memory
    c("publish", publish_); c("poll_query_ms", poll_query_ms_);
    c("small_ctl", small_ctl_); c("small_apw", small_apw_); c("knn_tail", knn_tail_);
    c("small_stamps", small_stamps_);      // diagnostics builds only (else 0)
    // the node MLP's activations per step (T, B*N, node_act_bytes), kept for the cooperative node
    // backward (0 = not kept)
    c("node_acts", acts_); c("node_act_bytes", act_bytes_);
    bool none = false;
    hfwd_ = c.sub("hfwd", "RolloutDriver hfwd", cbf_hfwd_args, &none);
    overlap_ = !none;
    sort_ = c.sub("cell_sort", "RolloutDriver cell_sort", cell_sort_args);
    scan_ = c.sub("scan", "RolloutDriver scan", scan_args);
    ctrl_ = c.sub("ctrl", "RolloutDriver ctrl", ctrl_args);
    c.done();
    const mb::ScanArgs& s = scan_;
    const mb::CtrlArgs& a = ctrl_;
    if (check_ < 1) check_ = 1;
    if (s.B < 1 || s.N < 1 || s.Nn < s.N || s.K < 1 || s.K > 16 || (s.dim != 2 && s.dim != 3) || Tmax_ < 1 || resort_ < 1 ||
        a.B != s.B || a.N != s.N || a.K != s.K || a.dim != s.dim || sort_.B != s.B || sort_.N != s.Nn ||
        (overlap_ && (hfwd_.B != s.B || hfwd_.N != s.N || hfwd_.K != s.K || hfwd_.dim != s.dim)))
      throw std::invalid_argument("RolloutDriver: bad dimensions");
    // what the steps offset: all present, on the same records and lists
    if (!s.S || a.S != s.S || sort_.S != s.S || !s.idx || a.idx != s.idx || !s.dang || !s.cnt || !a.A || !a.Snext ||
        !a.dist_sum || !a.act_sum || !a.pooled || !a.argmax || !host_dist_)
      throw std::invalid_argument("RolloutDriver: a required buffer is missing");
    if (!(a.a_max >= 0.f) || std::isinf(a.a_max))
      throw std::invalid_argument("RolloutDriver: a_max is 0 (off) or a positive finite limit");
    if (small_ctl_) {
      chk(hipHostMalloc((void**)&small_res_, 2 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc");
      small_res_[0] = small_res_[1] = 0;
      chk(hipHostGetDevicePointer((void**)&small_res_dev_, small_res_, 0), "hipHostGetDevicePointer");
    }
    if (publish_) {
      const size_t nd = (size_t)Tmax_ * s.B, bytes = nd * sizeof(unsigned long long) + (size_t)Tmax_ * sizeof(unsigned);
      chk(hipHostMalloc((void**)&pub_host_, bytes, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc");
      std::memset(pub_host_, 0, bytes);
      chk(hipHostGetDevicePointer((void**)&pub_dev_, pub_host_, 0), "hipHostGetDevicePointer");
      chk(hipMalloc((void**)&pub_ctr_, (size_t)Tmax_ * sizeof(unsigned)), "hipMalloc");
      chk(hipMemset(pub_ctr_, 0, (size_t)Tmax_ * sizeof(unsigned)), "hipMemset");   // once: kernels re-arm them
    }
    ev_copy_.resize(Tmax_);
    for (auto& e : ev_copy_) chk(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    // stream -> stream dependencies on one device: a device-scope release is enough (the default
    // system-scope fence writes back / invalidates caches for host visibility and stalls the
    // queue behind it); the copy-completion events the host waits on keep the system fence
    const unsigned fork_flags = hipEventDisableTiming | hipEventReleaseToDevice;
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
    const volatile unsigned long long* hd = host_dist_;
    const long B = ctrl_.B;
    int T = Tmax_;
    bool tail = false;
    // published early stop: the controller kernels hand the per-env sums to the host (no marker)
    const bool pub = publish_ && early_stop;
    if (pub) {
      ++gen_;      // the per-step counters are zero: set at allocation, re-armed by the last workgroup
      hd = pub_host_;
    }
    // Zero-lag check from the expected horizon (exp_T_: where the previous rollout ended; a hint --
    // T, tail and every buffer are the same with any value): from step exp_T_ on the publication of
    // step t-1 is awaited after scan(t) -- the tail scan if the rollout ends here -- and BEFORE
    // ctrl(t), so the controller step past the horizon, which nothing reads, is not issued. The
    // sums of step t-1 arrive while the GPU runs scan(t). Earlier steps keep the lagged check.
    const bool zero_lag = pub && zero_lag_ && check_ == 1 && !overlap_ && exp_T_ > 0;
    ctrl_issued_ = 0;
    for (int t = 0; t < Tmax_; ++t) {
      scan_step(t, st);
      // zero-lag: the check of step t-1 comes here, before ctrl(t), instead of after it below
      const bool early = zero_lag && t >= 1 && t >= exp_T_;
      if (early) {
        wait_published(t - 1, st);
        const int Tf = first_done(hd, t - 1);
        if (Tf > 0) {      // scan(t) was the tail scan; ctrl(t) is not issued
          T = Tf;
          tail = true;
          break;
        }
      }
      ctrl_step(t, st, pub);
      ++ctrl_issued_;
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
          chk(hipMemcpyAsync(host_dist_ + t * B, ctrl_.dist_sum + t * B * ctrl_.d_env, sizeof(unsigned long long) * B,
                             hipMemcpyDeviceToHost, cs), "hipMemcpyAsync");
          chk(hipEventRecord(ev_copy_[t], cs), "hipEventRecord");
        }
        // host check every check_every steps (small scenes: a step's kernels take less than
        // the host round trip, so checking every step would leave the GPU idle)
        if (!early && t >= 1 && (t % check_ == 0)) {
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
    if (pub) exp_T_ = T;  // the next rollout's expected horizon
    return {T, tail};     // converted to a tuple after the GIL is re-acquired
  }

  // The zero-lag check (run()): the expected horizon (0: none; run() sets it to the horizon it found),
  // the switch, and the controller steps the last run() issued.
  void set_expected_horizon(int T) { exp_T_ = T < 0 ? 0 : T; }
  int expected_horizon() const { return exp_T_; }
  void set_zero_lag(bool on) { zero_lag_ = on; }
  int ctrl_issued() const { return ctrl_issued_; }

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
    mb::RolloutSmallArgs a{};
    mb::CtrlArgs& c = a.c;
    c = ctrl_;          // the time-major bases: the kernel forms each step's views itself
    c.apw = small_apw_;
    c.stamps = small_stamps_;
    c.acts = acts_; c.na_env = c.N;
    a.idx = scan_.idx; a.dang = scan_.dang; a.cnt = scan_.cnt; a.safe = scan_.safe;
    a.Nn = scan_.Nn; a.Tmax = Tmax_; a.knn_tail = knn_tail_;
    a.r2_train = scan_.r2_train; a.ttc_train = scan_.ttc_train; a.r2_check = scan_.r2_check; a.ttc_check = scan_.ttc_check;
    a.done_thr = early_stop ? done_thr_ : -INFINITY;
    a.ctl = small_ctl_;      // zero at allocation; the kernel's last workgroup re-arms it
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
    const int B = ctrl_.B;
    for (int b = 0; b < B; ++b) {
      int q = 0;      // same float arithmetic as rollout_stats_kernel
      while (q <= t && !((float)((double)hd[(long)q * B + b] / mb::FX_DIST) / (float)ctrl_.N < done_thr_)) ++q;
      if (q > t) return 0;
      if (q > last) last = q;
    }
    return last + 1;
  }

  // the per-step views: the step-0 struct with its pointers moved t steps on, each by its own env stride
  const float4* S_at(int t) const { return sort_.S + (long)t * sort_.B * sort_.s_env * sort_.rec; }

  // Waits until the controller kernel of step t has published its per-env sums (flag == this
  // rollout's generation). Polls host-coherent memory; a stream error or a minute without the
  // flag raises instead of spinning forever.
  void wait_published(int t, hipStream_t st) const {
    const unsigned* flag = reinterpret_cast<const unsigned*>(pub_host_ + (size_t)Tmax_ * ctrl_.B) + t;
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
      mb::CellSortArgs c = sort_;
      c.S = S_at(t);
      chk(mb_cell_sort(&c, st), "cell_sort");
    }
    mb::ScanArgs a = scan_;
    const long tb = (long)t * a.B;
    a.S = S_at(t);
    a.idx += tb * a.i_env; a.dang += tb * a.i_env; a.cnt += tb * a.c_env;
    if (a.safe) a.safe += tb * a.sf_env;
    a.prev_idx = t > 0 ? a.idx - a.B * a.i_env : nullptr; a.pi_env = a.i_env;
    chk(mb_scan(&a, st), "scan");
  }

  void ctrl_step(int t, hipStream_t st, bool pub = false) {
    mb::CtrlArgs a = ctrl_;
    const long tb = (long)t * a.B;
    if (pub) {
      a.pub_ctr = pub_ctr_ + t;
      a.pub_dist = pub_dev_ + tb;
      a.pub_flag = reinterpret_cast<unsigned*>(pub_dev_ + (size_t)Tmax_ * a.B) + t;
      a.pub_gen = gen_;
    }
    a.S = S_at(t); a.Snext += tb * a.sn_env * sort_.rec;
    a.idx += tb * a.i_env; a.A += tb * a.a_env * a.dim;
    a.dist_sum += tb * a.d_env; a.act_sum += tb * a.ac_env;
    a.pooled += tb * a.p_env; a.argmax += tb * a.am_env;
    a.acts = acts_ ? acts_ + tb * a.N * act_bytes_ : nullptr; a.na_env = a.N;
    a.noise_t = t;
    chk(by_prec(prec_, mb_ctrl_fwd, mb_ctrl_fwd_f16, mb_ctrl_fwd_x3)(&a, num_cu_, st), "ctrl_fwd");
  }

  // CBF h of the main slots of step t, evaluations [t*BNK, (t+1)*BNK), on the side stream
  void hfwd_slice(int t, hipStream_t hs) {
    mb::CbfFwdArgs a = hfwd_;
    const long bnk = (long)a.B * a.N * a.K;
    a.T = t + 1; a.u_begin = (unsigned)(t * bnk); a.u_end = (unsigned)((t + 1) * bnk);
    chk(by_prec(prec_, mb_cbf_hfwd, mb_cbf_hfwd_f16, mb_cbf_hfwd_x3)(&a, hfwd_blocks_, hs), "cbf_hfwd");
  }

  mb::CellSortArgs sort_;     // the launches' arguments at step 0
  mb::ScanArgs scan_;
  mb::CtrlArgs ctrl_;
  mb::CbfFwdArgs hfwd_;       // over the whole buffers (overlap_ only)
  int Tmax_, num_cu_, prec_, resort_, hfwd_blocks_, check_, publish_, poll_query_ms_, small_apw_, knn_tail_;
  bool overlap_ = false;
  bool zero_lag_ = true;      // the zero-lag early-stop check from the expected horizon (run())
  int exp_T_ = 0;             // horizon of the previous published early-stop run() (0: none yet)
  int ctrl_issued_ = 0;       // controller steps issued by the last run()
  float done_thr_;
  unsigned gen_ = 0;
  unsigned long long* host_dist_;            // pinned [Tmax][B]: the copied per-env sums
  unsigned long long* pub_host_ = nullptr;   // host view: [Tmax][B] sums, then [Tmax] flags
  unsigned long long* pub_dev_ = nullptr;    // the same memory, device view
  unsigned* pub_ctr_ = nullptr;              // [Tmax] per-step workgroup counters (device)
  int* small_ctl_;
  unsigned long long* small_stamps_;
  unsigned char* acts_;
  long act_bytes_;
  std::vector<u64> bwd_execs_;
  int* small_res_ = nullptr;                 // host-coherent [T, flag] of the persistent rollout
  int* small_res_dev_ = nullptr;             // its device view
  unsigned small_gen_ = 0;
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
  // cfg: the driver's own keys and, as the dicts `node` / `edge`, the arguments of ctrl_node_bwd /
  // ctrl_edge_bwd at step 0 (ops/native.py _node_bwd_kw / _edge_bwd_kw on the engine's step-0 views,
  // without the fused combine). dS, Gb, rptr, redges: the time-major bases of what the combine reads of
  // step t+1, which no field of a step-0 struct holds; so Tmax == 1, where no step has a combine, is no
  // special case. No HIP call here.
  explicit BpttDriver(py::dict cfg) {
    Args c("BpttDriver", cfg);
    c("Tmax", Tmax_); c("prec", prec_); c("nb_node", nb_node_); c("nb_edge", nb_edge_);
    // per-step slab rows (small grids): step t's node / edge workgroups write rows (T-1-t) x grid
    // of the slabs instead of accumulating into one row per workgroup
    c("step_rows", step_rows_); c("node_part", node_part_); c("edge_part", edge_part_);
    c("fused_step", fused_); c("node_acts", acts_); c("node_act_bytes", act_bytes_);
    c("dS", dS_); c("Gb", Gb_); c("rptr", rptr_); c("redges", redges_);
    node_ = c.sub("node", "BpttDriver node", node_bwd_args);
    edge_ = c.sub("edge", "BpttDriver edge", edge_bwd_args);
    c.done();
    const mb::CtrlNodeBwdArgs& n = node_;
    const mb::CtrlEdgeBwdArgs& e = edge_;
    if (step_rows_ && (node_part_ <= 0 || edge_part_ <= 0))
      throw std::invalid_argument("BpttDriver: step_rows needs the slab row sizes");
    if (fused_ && (n.chunk != 32 || nb_node_ != nb_edge_ || e.w16))      // (the fused step keeps its own edge phase)
      throw std::invalid_argument("BpttDriver: the fused step needs 32-agent chunks and one grid");
    if (n.wrm16 && (n.chunk != 128 || fused_))
      throw std::invalid_argument("BpttDriver: the 16x16x32 node backward needs 128-agent chunks");
    if (n.B < 1 || n.N < 1 || n.s_env < n.N || e.K < 1 || e.K > 16 || (n.dim != 2 && n.dim != 3) || Tmax_ < 1 ||
        nb_node_ < 1 || nb_edge_ < 1 || e.B != n.B || e.N != n.N || e.dim != n.dim || e.S != n.S || e.s_env != n.s_env)
      throw std::invalid_argument("BpttDriver: bad dimensions");
    if (!n.S || !n.pooled || !n.A || !n.valid || !n.ego || !n.partial || !e.idx || !e.argmax || !e.dEc || !e.partial ||
        !dS_ || !Gb_ || !rptr_ || !redges_)
      throw std::invalid_argument("BpttDriver: a required buffer is missing");
    if (!(n.a_max >= 0.f) || std::isinf(n.a_max))
      throw std::invalid_argument("BpttDriver: a_max is 0 (off) or a positive finite limit");
  }

  // use_acts: this iteration's rollout kept the node activations (RolloutDriver with node_acts)
  void run(int T, float act_coef, u64 stream, bool use_acts) {
    if (T < 1 || T > Tmax_) throw std::invalid_argument("BpttDriver: T out of range");
    hipStream_t st = ST(stream);
    // strides of the time-major buffers, from the step-0 views: S is contiguous (s_env = Nn nodes)
    const long B = node_.B, N = node_.N, K = edge_.K, Nn = node_.s_env, R = node_.dim == 2 ? 1 : 2;
    const long BN = B * N, nk = N * K;
    for (int t = T - 1; t >= 0; --t) {
      const long tb = t * B;
      mb::CtrlNodeBwdArgs na = node_;
      mb::CtrlEdgeBwdArgs ea = edge_;
      {
        mb::CtrlNodeBwdArgs& a = na;
        a.pooled += tb * a.p_env; a.S += tb * a.s_env * R; a.A += tb * a.a_env * a.dim; a.valid += tb * a.v_env;
        a.Gn = dS_ + T * BN * R;       // t = T-1: the direct terms dS_T
        a.act_coef = act_coef;
        a.init = t == T - 1;     // the first step of the reverse loop writes the slabs
        if (step_rows_) {
          a.partial += (long)(T - 1 - t) * nb_node_ * node_part_;
          a.init = 1;
        }
        a.acts = (use_acts && acts_) ? acts_ + tb * N * act_bytes_ : nullptr;
        a.na_env = N;
        a.K = K;
        if (t < T - 1) {
          // fused BPTT combine: G_{t+1} from step t+1's records (dS, ego, dEc, graph t+1, G_{t+2})
          const long t1 = t + 1;
          a.cdS = dS_ + t1 * BN * R; a.cds_env = N;
          // dEc is double-buffered by step parity: step t+1's edge records sit in buffer (t+1)&1
          // while step t's edge phase writes buffer t&1 (the fused launch overlaps the two)
          a.cego = a.ego; a.cdEc = ea.dEc + (t1 & 1) * B * ea.de_env * R;
          a.cptr = rptr_ + t1 * B * (Nn + 1); a.cptr_env = Nn + 1;
          a.cedges = redges_ + t1 * B * nk; a.cedges_env = nk;
          a.cGn = (t1 == T - 1 ? a.Gn : Gb_ + (t1 + 1) * BN * R);
          a.cgn_env = N;
          a.cGout = Gb_ + t1 * BN * R; a.cgo_env = N;
        }
      }
      {
        mb::CtrlEdgeBwdArgs& a = ea;
        a.S = na.S;
        a.idx += tb * a.i_env; a.argmax += tb * a.am_env;
        a.dEc += (t & 1) * B * a.de_env * R;
        a.init = t == T - 1;
        if (step_rows_) {
          a.partial += (long)(T - 1 - t) * nb_edge_ * edge_part_;
          a.init = 1;
        }
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
  mb::CtrlNodeBwdArgs node_;      // the launches' arguments at step 0
  mb::CtrlEdgeBwdArgs edge_;
  int Tmax_, prec_, nb_node_, nb_edge_, step_rows_, fused_;
  long node_part_, edge_part_, act_bytes_;
  const unsigned char* acts_;
  const float4* dS_;              // (Tmax+1, B, N) direct terms; row T seeds the loop
  float4* Gb_;                    // (Tmax+1, B, N) G_t out
  const int* rptr_;               // reverse CSR of every step's graph: (., B, Nn+1) / (., B, N*K)
  const int* redges_;
};

// One call of the safety filter: the kernels' arguments (all but r.it) and how they are launched
struct RefineCall {
  mb::RefineSmallArgs sa;       // sa.r: both filters; sa.ew: the persistent filter's result words
  int num_blocks, prec;         // num_blocks: refine_grad's grid (the loop filter's alone, as r.dEv and r.ctl)
  int fused, fused_blocks;      // decentralised filter (r.local): one refine_local launch of fused_blocks workgroups
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
  x.opt("a_max", r.a_max);                // the actuator limit: off (0) without the key
  x.opt("local", r.local);                // the decentralised filter: the joint one (0) without the key
  x.opt("fused", c.fused); x.opt("fused_blocks", c.fused_blocks);
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
      c->num_blocks < 1 || r.f_bwd < 0 || r.s_env < r.Nn || c->prec < 0 || c->prec > 2 || !(r.a_max >= 0.f))
    return -1;
  if (!r.S || !r.idx || !r.a || !r.delta || !r.h || !r.wpack || !r.wrm || !r.wvec || !r.dEv || !r.ctl) return -2;
  if (!r.local && (!r.ptr || !r.edges)) return -2;             // the joint update walks the reverse CSR
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
  if (c->prec < 0 || c->prec > 2 || !(r.a_max >= 0.f)) return -1;
  if (!r.S || !r.idx || !r.a || !r.delta || !r.h || !r.wpack || !r.wrm || !r.wvec || !r.ptr || !r.edges || !c->sa.ew) return -2;
  if (c->sa.loops == 0) return 0;
  return by_prec(c->prec, mb_refine_small, mb_refine_small_f16, mb_refine_small_x3)(&c->sa, st);
}

// Decentralised safety filter (csrc/refine.hip refine_local_kernel): the whole loop of every agent in
// ONE launch on the caller's stream. The pointers and sizes are validated once; the control words (2
// per iteration, the loop path's array) are cleared here; delta arrives zeroed; no reverse CSR, no
// dEv; no host synchronisation. The kernel writes r.hn_out / r.flag_out at iteration 0 only.
int refine_local(const RefineCall* c, hipStream_t st) {
  const mb::RefineArgs& r = c->sa.r;
  const int loops = c->sa.loops;
  if ((r.dim != 2 && r.dim != 3) || r.B < 1 || r.N < 1 || r.Nn < r.N || r.K < 1 || r.K > 16 || loops < 0 ||
      c->fused_blocks < 1 || r.f_bwd < 0 || r.s_env < r.Nn || c->prec < 0 || c->prec > 2 || !(r.a_max >= 0.f) || !r.local)
    return -1;
  if (!r.S || !r.idx || !r.a || !r.delta || !r.h || !r.wpack || !r.wrm || !r.wvec || !r.ctl) return -2;
  if (loops == 0) return 0;
  const hipError_t e = hipMemsetAsync(r.ctl, 0, (size_t)loops * 2 * sizeof(unsigned long long), st);
  if (e != hipSuccess) return (int)e;
  return by_prec(c->prec, mb_refine_local, mb_refine_local_f16, mb_refine_local_x3)(&c->sa, c->fused_blocks, st);
}

// The arguments of the three launches of csrc/episode.hip (the driver sets S_cur / S_next per step)
mb::EpisodeArgs episode_args(Args& x) {
  mb::EpisodeArgs e{};
  x.opt("S_cur", e.S_cur); x.opt("S_next", e.S_next); x("s_env", e.s_env); x("dim", e.dim); x("B", e.B);
  x("N", e.N); x("A", e.A); x("delta", e.delta); x("G", e.G); x("dt", e.dt); x("st", e.st);
  x("dist_fx", e.dist_fx); x("safe", e.safe); x("active", e.active); x("prev_active", e.prev_active);
  x("ctl", e.ctl); x("ew", e.ew); x("loops", e.loops); x("mode", e.mode); x("thr", e.thr); x("out", e.out);
  // the actuator limit and the action statistics: off without the keys
  x.opt("a_max", e.a_max); x.opt("act_st", e.act_st); x.opt("act_out", e.act_out);
  e.thr_fx = (unsigned long long)std::llrint((double)e.thr * (double)e.N * mb::FX_DIST);
  return e;
}

// Closed-loop episode driver (csrc/episode.hip): a whole batch of episodes -- validation during
// training, evaluation -- with or without the safety filter, as one call. Per step, on the caller's
// stream: cell_sort + ONE scan of s_t (kNN and the safety count of the step before), the controller
// forward, with an actuator limit episode_limit, the filter (cbf_fwd for h(s_t), rev_csr, refine_loop
// or refine_small; the decentralised filter: cbf_fwd, then refine_local -- the ctl memset and one
// launch -- or its loop path, and no rev_csr), episode_advance,
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
    // the launches' arguments on the first record buffer (S: per step), ops/native.py's builders
    mb::CellSortArgs sort;
    mb::ScanArgs scan, scan_final;      // every step's (kNN + safety); the safety-only scan of the final state
    mb::CtrlArgs ctrl;
    mb::CbfFwdArgs cbf;         // filter: h(s_t) into r.h
    mb::CsrArgs csr;            // filter: the reverse CSR into r.ptr / r.edges
    float4* S1;                 // the second record buffer (the first: scan.S)
    int num_cu, prec_ctrl, cbf_blocks, max_steps, check_every, mask_done;
    hipStream_t stream;
  };

  // Returns (steps issued, 0 or 1: the buffer that holds the final state).
  std::pair<int, int> run(py::dict c) {
    Cfg g = parse(c);
    py::gil_scoped_release nogil;       // the loop waits for the stream every check_every steps
    return loop(g);
  }

 private:
  // cfg: the driver's own keys and one dict per argument struct (refine, cbf, csr: None without the filter)
  static Cfg parse(const py::dict& c) {
    Args x("EpisodeDriver", c);
    Cfg g{};
    bool none = false, no_cbf = false, no_csr = false;
    g.e = x.sub("episode", "EpisodeDriver episode", episode_args);
    g.r = x.sub("refine", "EpisodeDriver refine", refine_call, &none);
    g.sort = x.sub("cell_sort", "EpisodeDriver cell_sort", cell_sort_args);
    g.scan = x.sub("scan", "EpisodeDriver scan", scan_args);
    g.scan_final = x.sub("scan_final", "EpisodeDriver scan_final", scan_args);
    g.ctrl = x.sub("ctrl", "EpisodeDriver ctrl", ctrl_args);
    g.cbf = x.sub("cbf", "EpisodeDriver cbf", cbf_fwd_args, &no_cbf);
    g.csr = x.sub("csr", "EpisodeDriver csr", rev_csr_args, &no_csr);
    x("S1", g.S1); x("num_cu", g.num_cu); x("prec_ctrl", g.prec_ctrl); x("cbf_blocks", g.cbf_blocks);
    x("max_steps", g.max_steps); x("check_every", g.check_every); x("mask_done", g.mask_done);
    g.stream = ST(x.u("stream"));
    x.done();
    const mb::EpisodeArgs& e = g.e;
    const mb::ScanArgs &s = g.scan, &f = g.scan_final;
    const mb::CtrlArgs& a = g.ctrl;
    const bool filter = e.mode != 0;
    const bool local = filter && g.r.sa.r.local != 0;         // the decentralised filter needs no reverse CSR
    if (e.B < 1 || e.N < 1 || s.Nn < e.N || e.s_env != s.Nn || s.K < 1 || s.K > 16 || s.K > s.Nn || (e.dim != 2 && e.dim != 3) ||
        g.max_steps < 0 || e.loops < 0 || e.mode < 0 || e.mode > 2 || g.prec_ctrl < 0 || g.prec_ctrl > 2 || filter == none ||
        no_cbf != none || (local ? !no_csr : no_csr != none) || s.B != e.B || s.N != e.N || s.dim != e.dim || s.s_env != s.Nn || f.B != e.B ||
        f.N != e.N || f.Nn != s.Nn || f.dim != e.dim || f.s_env != s.Nn || a.B != e.B || a.N != e.N || a.K != s.K ||
        a.dim != e.dim || a.s_env != s.Nn || g.sort.B != e.B || g.sort.N != s.Nn || g.sort.s_env != s.Nn)
      throw std::invalid_argument("EpisodeDriver: bad dimensions");
    if (g.check_every < 1) g.check_every = 1;
    if (!s.S || !g.S1 || s.S == g.S1 || !e.G || !s.idx || a.idx != s.idx || !e.A || a.A != e.A || !a.argmax || !s.perm ||
        f.perm != s.perm || g.sort.perm != s.perm || !e.safe || s.safe != e.safe || f.safe != e.safe || !e.st || !e.dist_fx ||
        !e.active || !e.prev_active || !e.out || !a.wpack || !a.wvec || (g.prec_ctrl == 2 && !a.pooled))
      throw std::invalid_argument("EpisodeDriver: a required buffer is missing");
    if (!(e.a_max >= 0.f) || (e.act_st != nullptr) != (e.act_out != nullptr) || (filter && g.r.sa.r.a_max != e.a_max))
      throw std::invalid_argument("EpisodeDriver: bad actuator limit or action-statistics words");
    if (filter) {
      const mb::RefineArgs& r = g.r.sa.r;
      if (g.r.prec == 1) throw std::invalid_argument("EpisodeDriver: the safety filter has no fp16 build");
      if (r.B != e.B || r.N != e.N || r.Nn != s.Nn || r.K != s.K || r.dim != e.dim || e.loops < 1 ||
          g.r.sa.loops != e.loops || g.r.sa.ew != e.ew || g.r.prec < 0 || g.r.prec > 2 || r.idx != s.idx ||
          g.cbf.B != e.B || g.cbf.T != 1 || g.cbf.N != e.N || g.cbf.K != s.K || g.cbf.dim != e.dim || g.cbf.idx != s.idx ||
          (!local && (g.csr.G != e.B || g.csr.N != e.N || g.csr.K != s.K || g.csr.Nn != s.Nn || g.csr.idx != s.idx)) ||
          (local && e.mode != 1) || (g.r.fused && !local))
        throw std::invalid_argument("EpisodeDriver: bad dimensions");
      if (!r.wpack || !r.wrm || !r.wvec || !r.delta || r.delta != e.delta || !r.h || g.cbf.h_out != r.h ||
          (!local && (!r.ptr || g.csr.ptr != r.ptr || !r.edges || g.csr.edges != r.edges)) || !g.cbf.wpack || !g.cbf.wvec ||
          g.cbf_blocks < 1)
        throw std::invalid_argument("EpisodeDriver: a filter buffer is missing");
      if (e.mode == 2 ? (!e.ew || s.Nn > 64)
                      : (!r.ctl || (g.r.fused ? g.r.fused_blocks < 1 : (!r.dEv || g.r.num_blocks < 1))))
        throw std::invalid_argument("EpisodeDriver: the filter's result words / workspace are missing");
    }
    return g;
  }

  std::pair<int, int> loop(const Cfg& g) {
    hipStream_t st = g.stream;
    float4* S[2] = {const_cast<float4*>(g.scan.S), g.S1};
    int cur = 0, t = 0;
    mb::EpisodeArgs e = g.e;
    for (; t < g.max_steps;) {
      scan(g, g.scan, S[cur], st);
      mb::CtrlArgs a = g.ctrl;
      a.S = S[cur];
      chk(by_prec(g.prec_ctrl, mb_ctrl_fwd, mb_ctrl_fwd_f16, mb_ctrl_fwd_x3)(&a, g.num_cu, st), "ctrl_fwd");
      if (e.a_max > 0.f) chk(mb_episode_limit(&e, st), "episode_limit");     // before the filter reads A
      if (e.mode) refine(g, S[cur], st);
      e.S_cur = S[cur]; e.S_next = S[cur ^ 1];
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
    scan(g, g.scan_final, S[cur], st);           // the safety count of the final state
    e.S_cur = S[cur]; e.S_next = nullptr;
    chk(mb_episode_final(&e, st), "episode_final");
    return {t, cur};
  }

  void scan(const Cfg& g, mb::ScanArgs a, const float4* S, hipStream_t st) {
    mb::CellSortArgs c = g.sort;
    c.S = a.S = S;
    chk(mb_cell_sort(&c, st), "cell_sort");
    chk(mb_scan(&a, st), "scan");
  }

  void refine(const Cfg& g, const float4* S, hipStream_t st) {
    RefineCall c = g.r;
    mb::RefineArgs& r = c.sa.r;
    mb::CbfFwdArgs a = g.cbf;
    r.S = a.S = S;         // the step's h(s_t) and reverse CSR are written where the filter reads them
    chk(by_prec(c.prec, mb_cbf_fwd, mb_cbf_fwd_f16, mb_cbf_fwd_x3)(&a, g.cbf_blocks, st), "cbf_fwd");
    if (!r.local) chk(mb_rev_csr(&g.csr, st), "rev_csr");
    if (!g.mask_done) r.env_active = nullptr;        // validate.py's rule: a finished env is not refined
    if (c.fused) chk(refine_local(&c, st), "refine_local");
    else if (g.e.mode == 2) chk(refine_small(&c, st), "refine_small");
    else chk(refine_loop(&c, st), "refine_loop");
  }

  long long* alive_host_ = nullptr;
};

}  // namespace

void register_runtime(py::module& m) {
  def_launch(m, "refine_loop", refine_call, refine_loop);
  def_launch(m, "refine_small", refine_call, refine_small);
  def_launch(m, "refine_local", refine_call, refine_local);
  // the three launches of csrc/episode.hip on their own, as EpisodeDriver issues them per step
  def_launch(m, "episode_limit", episode_args, mb_episode_limit);
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
      .def("set_expected_horizon", &RolloutDriver::set_expected_horizon, py::arg("T"))
      .def("set_zero_lag", &RolloutDriver::set_zero_lag, py::arg("on"))
      .def_property_readonly("expected_horizon", &RolloutDriver::expected_horizon)
      .def_property_readonly("ctrl_issued", &RolloutDriver::ctrl_issued)
      .def("run_small", &RolloutDriver::run_small, py::arg("stream"), py::arg("early_stop"),
           py::arg("launch_graph") = false, py::arg("s0") = 0, py::arg("g0") = 0,
           py::call_guard<py::gil_scoped_release>())
      .def("run", &RolloutDriver::run, py::arg("stream"), py::arg("hstream"), py::arg("copy_stream"),
           py::arg("early_stop"),
           // the loop blocks on hipEventSynchronize: let other Python threads run meanwhile
           py::call_guard<py::gil_scoped_release>());
}
