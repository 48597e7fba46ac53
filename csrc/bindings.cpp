// pybind11 layer: raw-pointer launchers for the gfx950 kernels.
//
// Tensors are validated (device, dtype, contiguity, shape) on the Python side in
// macbf_gnn_amd/ops/native.py and passed here as integer device addresses together with the
// current HIP stream handle of PyTorch, so this module needs no libtorch headers and builds
// in seconds. Every launcher returns the hipError_t of the launch; native.py raises on != 0.
//
// Calling convention: launchers take keyword arguments, read through Args (csrc/pyargs.h). One *_args
// function per struct of csrc/args.h fills it, the keys being the field names (csrc/fill.h: the ones the
// drivers of runtime.cpp read too); launch parameters are num_blocks / num_cu, prec and stream. A missing, misspelt or mistyped argument is a TypeError.
#include <pybind11/pybind11.h>
#include <hip/hip_runtime.h>

#include "fill.h"

static hipStream_t ST(u64 s) { return reinterpret_cast<hipStream_t>(static_cast<uintptr_t>(s)); }

// the launch plan mb_scan picks for a call of this shape (tests assert the instantiation they hit)
static py::tuple scan_plan(int B, int N, int K, int Nn, int dim, int has_prev, int do_knn, int do_safety, int lanes) {
  mb::ScanArgs a{};
  a.B = B; a.N = N; a.K = K; a.Nn = Nn; a.dim = dim; a.lanes = lanes;
  a.do_knn = do_knn; a.do_safety = do_safety;
  static const int dummy = 0;
  a.prev_idx = has_prev ? &dummy : nullptr;
  long out[9] = {};
  const int rc = mb_scan_plan(&a, out);
  if (rc) throw std::runtime_error("scan_plan: bad arguments");
  return py::make_tuple(out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7], out[8]);
}

static mb::ScenArgs scenario_args(Args& x) {
  mb::ScenArgs a{};
  x("S", a.S); x("s_env", a.s_env); x("G", a.G); x("obs", a.obs); x("M", a.M); x("dim", a.dim);
  x("B", a.B); x("N", a.N); x("L", a.L); x("r", a.r); x("spread", a.spread); x("seed", a.seed);
  x("max_rounds", a.max_rounds); x("status", a.status); x("ws", a.ws); x("ws_env", a.ws_env);
  return a;
}

static mb::CbfBwdArgs cbf_bwd_args(Args& x) {
  mb::CbfBwdArgs a{};
  x("S", a.S); x("s_env", a.s_env); x("s_step", a.s_step); x("dim", a.dim); x("idx", a.idx); x("idx1", a.idx1);
  x("B", a.B); x("T", a.T); x("N", a.N); x("K", a.K); x("passes", a.passes); x("dh", a.dh);
  x("wpack", a.wpack); x("f_bwd", a.f_bwd); x("wrm", a.wrm); x("wvec", a.wvec); x("dE", a.dE);
  x("partial", a.partial); x("obs_r", a.obs_r); x("dist_thr", a.dist_thr); x("dist_eps", a.dist_eps);
  x("fused", a.fused); x("dang", a.dang); x("valid", a.valid);
  x("counts", a.counts); a.lc = x.loss_consts<mb::LossConsts>("lc");
  x("src", a.src); x("nev", a.nev); x("act", a.act); x("nact", a.nact); x("rec", a.rec); x("wrm16", a.wrm16);
  x("w16", a.w16); x("dbg", a.dbg); x("stamps", a.stamps);
  return a;
}

static mb::NodeRedArgs node_reduce_args(Args& x) {
  mb::NodeRedArgs a{};
  x("dE", a.dE); x("ptr", a.ptr); x("edges", a.edges); x("B", a.B); x("T", a.T); x("N", a.N);
  x("K", a.K); x("passes", a.passes); x("accumulate", a.accumulate); x("out", a.out); x("pass_mask", a.pass_mask);
  x("Nn", a.Nn); x("dim", a.dim); x("shift1", a.shift1); x("map1", a.map1); x("gate", a.gate); x("t_lo", a.t_lo);
  x("t_hi", a.t_hi);
  return a;
}

static mb::CbfMatchArgs cbf_match_args(Args& x) {
  mb::CbfMatchArgs a{};
  x("idx", a.idx); x("T", a.T); x("B", a.B); x("N", a.N); x("K", a.K); x("mode", a.mode);
  x("phase", a.phase); x("cnt", a.cnt); x("off", a.off); x("bsum", a.bsum); x("nev", a.nev); x("map1", a.map1);
  x("src", a.src);
  return a;
}

static mb::CbfDhArgs cbf_dh_args(Args& x) {
  mb::CbfDhArgs a{};
  x("h", a.h); x("hmask", a.hmask); x("map1", a.map1); x("src", a.src); x("nev", a.nev); x("dang", a.dang);
  x("valid", a.valid); x("B", a.B); x("T", a.T); x("N", a.N); x("K", a.K);
  x("counts", a.counts); a.lc = x.loss_consts<mb::LossConsts>("lc");
  x("dh", a.dh); x("partial", a.partial); x("blk_active", a.blk_active);
  return a;
}

static int cbf_compact(py::kwargs kw) {
  Args x("cbf_compact", kw);
  return x.then(mb_cbf_compact, x.ptr<const float>("dh"), x.ptr<const int>("nev"), x.ptr<const int>("blk_off"),
                x.ptr<int>("act"), x.i("num_blocks"), x.ptr<const int>("blk_active"), x.ptr<int>("nact"),
                x.ptr<const int>("src"), x.ptr<const int>("idx"), x.ptr<const int>("idx1"), (unsigned)x.u("E"),
                x.ptr<void>("rec"), ST(x.u("stream")));
}

static mb::CombineArgs node_combine_args(Args& x) {
  mb::CombineArgs a{};
  x("dim", a.dim); x("dS", a.dS); x("ds_env", a.ds_env); x("ego", a.ego); x("dEc", a.dEc); x("ptr", a.ptr);
  x("ptr_env", a.ptr_env); x("edges", a.edges); x("edges_env", a.edges_env); x("Gn", a.Gn); x("gn_env", a.gn_env);
  x("Gout", a.Gout); x("go_env", a.go_env); x("B", a.B); x("N", a.N); x("K", a.K); x("dt", a.dt);
  return a;
}

static int reduce_rows(py::kwargs kw) {
  Args x("reduce_rows", kw);
  return x.then(mb_reduce_rows, x.ptr<const float>("partial"), x.i("rows"), x.i("cols"), x.ptr<float>("out"),
                x.i("accumulate"), ST(x.u("stream")));
}

static mb::StepCommitArgs commit_args(Args& x) {
  mb::StepCommitArgs a{};
  x("ok", a.ok); x("steps", a.steps); x("mask", a.mask); x("ngroups", a.ngroups); x("skipped", a.skipped);
  x("gscale", a.gscale); x("good", a.good); x("growth", a.growth); x("max_scale", a.max_scale);
  x("stats_row", a.stats_row); x.opt("stats_src", a.stats_src);
  return a;
}

// commit: None, or step_commit's arguments as a dict -- that commit then runs inside the gather launch
static int pack_gather(py::kwargs kw) {
  Args x("pack_gather", kw);
  bool none = false;
  const mb::StepCommitArgs c = x.sub("commit", "pack_gather", commit_args, &none);
  return x.then(mb_pack_gather, x.ptr<const float>("src"), x.i("n"), x.ptr<const int>("idx16"), x.i("m16"),
                x.ptr<unsigned short>("out16"), x.i("f16"), x.ptr<const int>("idx32"), x.i("m32"),
                x.ptr<float>("out32"), none ? nullptr : &c, ST(x.u("stream")));
}

static mb::GradAssembleArgs grad_assemble_args(Args& x) {
  mb::GradAssembleArgs a{};
  x("red", a.red); x("ptr", a.ptr); x("src", a.src); x("n", a.n); x("scale", a.scale); x("gscale", a.gscale);
  x("grad", a.grad); x("ok", a.ok); x("sums", a.sums); x("counts", a.counts); x("local", a.local); x("row", a.row);
  return a;
}

// jobs: [(partial, rows, cols, out, accumulate)] (at most mb::RM_JOBS), one launch
static int reduce_multi(py::list jobs, u64 stream) {
  mb::ReduceMultiArgs a{};
  a.njobs = (int)py::len(jobs);
  if (a.njobs < 1 || a.njobs > mb::RM_JOBS) return -1;
  for (int j = 0; j < a.njobs; ++j) {
    const py::tuple t = jobs[j].cast<py::tuple>();
    a.partial[j] = P<const float>(t[0].cast<u64>()); a.rows[j] = t[1].cast<int>(); a.cols[j] = t[2].cast<int>();
    a.out[j] = P<float>(t[3].cast<u64>()); a.accumulate[j] = t[4].cast<int>();
  }
  return mb_reduce_multi(&a, ST(stream));
}

// groups: [(lo, hi, step_ptr)] (at most mb::AM_GROUPS); the rest as adam()
static int adam_multi(py::list groups, py::kwargs kw) {
  Args x("adam_multi", kw);
  mb::AdamArgs c{};
  x("param", c.param); x("grad", c.grad); x("m", c.m); x("v", c.v); x("b1", c.b1); x("b2", c.b2);
  x("eps", c.eps); x("wd", c.wd); x("ok", c.ok); x("lr", c.lr);
  hipStream_t st = x.then(ST, x.u("stream"));      // argument errors first, then the groups
  mb::AdamMultiArgs a{};
  a.ngroups = (int)py::len(groups);
  if (a.ngroups < 1 || a.ngroups > mb::AM_GROUPS) return -1;
  for (int g = 0; g < a.ngroups; ++g) {
    const py::tuple t = groups[g].cast<py::tuple>();
    mb::AdamArgs& y = a.g[g];
    y = c;
    y.lo = t[0].cast<int>(); y.hi = t[1].cast<int>(); y.step = P<const int>(t[2].cast<u64>());
    if (!y.step) return -2;          // device step counters only (bias corrections on the device)
  }
  return mb_adam_multi(&a, st);
}

static int grad_check(u64 g, int n, u64 ok, u64 stream) {
  return mb_grad_check(P<const float>(g), n, P<int>(ok), ST(stream));
}

static int stats_pack(u64 sums, u64 counts, u64 local, u64 row, u64 stream) {
  return mb_stats_pack(P<const float>(sums), P<const float>(counts), P<const float>(local), P<float>(row),
                       ST(stream));
}

static mb::RolloutStatsArgs rollout_stats_args(Args& x) {
  mb::RolloutStatsArgs a{};
  x("dist", a.dist); x("cnt", a.cnt); x("safe", a.safe); x("act", a.act); x("T", a.T); x("B", a.B);
  x("N", a.N); x("reset_T", a.reset_T); x("thr", a.thr); x("valid", a.valid); x("counts", a.counts);
  x("local", a.local);
  return a;
}

static mb::AdamArgs adam_args(Args& x) {
  mb::AdamArgs a{};
  x("param", a.param); x("grad", a.grad); x("m", a.m); x("v", a.v); x("lo", a.lo); x("hi", a.hi);
  x("b1", a.b1); x("b2", a.b2); x("eps", a.eps); x("wd", a.wd); x("step_size", a.step_size);
  x("bc2_sqrt", a.bc2_sqrt); x("ok", a.ok); x("step", a.step); x("lr", a.lr);
  return a;
}

// One fused BPTT step (ctrl.hip ctrl_bwd_step_kernel): `node` and `edge` are the struct arguments
// of ctrl_node_bwd / ctrl_edge_bwd; one launch of num_blocks workgroups.
static int ctrl_bwd_step(py::dict node, py::dict edge, int num_blocks, int prec, u64 stream) {
  const auto launch = by_prec(prec, mb_ctrl_bwd_step, mb_ctrl_bwd_step_f16, mb_ctrl_bwd_step_x3);
  Args n("ctrl_bwd_step node", node), e("ctrl_bwd_step edge", edge);
  const mb::CtrlNodeBwdArgs na = node_bwd_args(n);
  n.done();
  const mb::CtrlEdgeBwdArgs ea = edge_bwd_args(e);
  e.done();
  return launch(&na, &ea, num_blocks, ST(stream));
}

static py::dict device_info(int dev) {
  hipDeviceProp_t p;
  py::dict d;
  if (hipGetDeviceProperties(&p, dev) != hipSuccess) return d;
  d["name"] = std::string(p.name);
  d["gcn_arch"] = std::string(p.gcnArchName);
  d["cu"] = p.multiProcessorCount;
  d["lds_per_block"] = (long)p.sharedMemPerBlock;
  d["warp"] = p.warpSize;
  return d;
}

static std::string err_str(int e) { return hipGetErrorString((hipError_t)e); }

// workgroups per CU of the 16x16x32 backward kernels of build `prec` (kernel 0 CBF, 1 edge, 2 node)
static int node_act_bytes(int prec) {
  return by_prec(prec, mb_node_act_bytes, mb_node_act_bytes_f16, mb_node_act_bytes_x3)();
}

static int k16_wg_per_cu(int prec, int kernel) {
  return by_prec(prec, mb_k16_wg_per_cu, mb_k16_wg_per_cu_f16, mb_k16_wg_per_cu_x3)(kernel);
}

void register_runtime(py::module& m);   // runtime.cpp: native rollout driver

PYBIND11_MODULE(_C, m) {
  m.doc() = "macbf_gnn_amd native gfx950 kernels";
  register_runtime(m);
  def_launch(m, "scan", scan_args, mb_scan);
  m.def("scan_plan", &scan_plan);
  def_launch(m, "cell_sort", cell_sort_args, mb_cell_sort);
  def_launch(m, "scenario", scenario_args, mb_scenario);
  def_launch(m, "ctrl_fwd", ctrl_args, "num_cu", mb_ctrl_fwd, mb_ctrl_fwd_f16, mb_ctrl_fwd_x3);
  def_launch(m, "cbf_fwd", cbf_fwd_args, "num_blocks", mb_cbf_fwd, mb_cbf_fwd_f16, mb_cbf_fwd_x3);
  def_launch(m, "cbf_bwd", cbf_bwd_args, "num_blocks", mb_cbf_bwd, mb_cbf_bwd_f16, mb_cbf_bwd_x3);
  def_launch(m, "cbf_hfwd", cbf_hfwd_args, "num_blocks", mb_cbf_hfwd, mb_cbf_hfwd_f16, mb_cbf_hfwd_x3);
  def_launch(m, "ctrl_node_bwd", node_bwd_args, "num_blocks", mb_ctrl_node_bwd, mb_ctrl_node_bwd_f16, mb_ctrl_node_bwd_x3);
  def_launch(m, "ctrl_edge_bwd", edge_bwd_args, "num_blocks", mb_ctrl_edge_bwd, mb_ctrl_edge_bwd_f16, mb_ctrl_edge_bwd_x3);
  def_launch(m, "rev_csr", rev_csr_args, mb_rev_csr);
  def_launch(m, "node_reduce", node_reduce_args, mb_node_reduce);
  def_launch(m, "node_combine", node_combine_args, mb_node_combine);
  def_launch(m, "cbf_match", cbf_match_args, mb_cbf_match);
  def_launch(m, "cbf_dh", cbf_dh_args, "num_blocks", mb_cbf_dh);
  m.def("cbf_compact", &cbf_compact);
  m.def("reduce_rows", &reduce_rows);
  def_launch(m, "adam", adam_args, mb_adam);
  def_launch(m, "rollout_stats", rollout_stats_args, mb_rollout_stats);
  m.def("grad_check", &grad_check, py::arg("g"), py::arg("n"), py::arg("ok"), py::arg("stream"));
  def_launch(m, "grad_assemble", grad_assemble_args, mb_grad_assemble);
  m.def("reduce_multi", &reduce_multi, py::arg("jobs"), py::arg("stream"));
  m.def("adam_multi", &adam_multi, py::arg("groups"));
  m.def("pack_gather", &pack_gather);
  def_launch(m, "step_commit", commit_args, mb_step_commit);
  m.def("stats_pack", &stats_pack, py::arg("sums"), py::arg("counts"), py::arg("local"), py::arg("row"),
        py::arg("stream"));
  m.def("ctrl_bwd_step", &ctrl_bwd_step, py::arg("node"), py::arg("edge"), py::arg("num_blocks"), py::arg("prec"),
        py::arg("stream"));
  m.def("device_info", &device_info);
  m.def("err_str", &err_str);
  m.def("k16_wg_per_cu", &k16_wg_per_cu);
  m.def("node_act_bytes", &node_act_bytes);
  m.attr("ARCH") = "gfx950";
}
