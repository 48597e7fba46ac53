// The fill functions of the kernel argument structs that more than one entry point reads: the
// single launches of bindings.cpp and the drivers of runtime.cpp. One function per struct of
// csrc/args.h, the keys being the field names (csrc/pyargs.h). Host-only.
#pragma once
#include "args.h"
#include "pyargs.h"

inline mb::CellSortArgs cell_sort_args(Args& x) {
  mb::CellSortArgs a{};
  x("S", a.S); x("s_env", a.s_env); x("B", a.B); x("N", a.N); x("rec", a.rec); x("L", a.L);
  x("perm", a.perm);
  return a;
}

inline mb::ScanArgs scan_args(Args& x) {
  mb::ScanArgs a{};
  x("S", a.S); x("s_env", a.s_env); x("perm", a.perm); x("B", a.B); x("N", a.N); x("K", a.K);
  x("Nn", a.Nn); x("dim", a.dim); x("idx", a.idx); x("i_env", a.i_env); x("dang", a.dang); x("cnt", a.cnt);
  x("c_env", a.c_env); x("safe", a.safe); x("sf_env", a.sf_env); x("r2_train", a.r2_train);
  x("ttc_train", a.ttc_train); x("r2_check", a.r2_check); x("ttc_check", a.ttc_check); x("do_knn", a.do_knn);
  x("do_safety", a.do_safety); x("prev_idx", a.prev_idx); x("pi_env", a.pi_env); x("ws", a.ws);
  x("ws_env", a.ws_env); x("lanes", a.lanes); x("stamps", a.stamps);
  return a;
}

inline mb::CtrlArgs ctrl_args(Args& x) {
  mb::CtrlArgs a{};
  x("S", a.S); x("s_env", a.s_env); x("dim", a.dim); x("G", a.G); x("idx", a.idx); x("i_env", a.i_env);
  x("B", a.B); x("N", a.N); x("K", a.K); x("wpack", a.wpack); x("f_edge", a.f_edge); x("f_node", a.f_node);
  x("wvec", a.wvec); x("A", a.A); x("a_env", a.a_env); x("Snext", a.Snext); x("sn_env", a.sn_env);
  x("dist_sum", a.dist_sum); x("d_env", a.d_env); x("act_sum", a.act_sum); x("ac_env", a.ac_env);
  x("noise", a.noise); x("n_env", a.n_env); x("noise_key", a.noise_key); x("noise_prob", a.noise_prob);
  x("noise_scale", a.noise_scale); x("noise_t", a.noise_t); x("dt", a.dt); x("obs_r", a.obs_r); x("sqrt3", a.sqrt3);
  x("pooled", a.pooled); x("p_env", a.p_env); x("argmax", a.argmax); x("am_env", a.am_env); x("apw", a.apw);
  x("stamps", a.stamps); x.opt("a_max", a.a_max);      // the actuator limit: off (0) without the key
  x.opt("res", a.res);                                  // the residual head: off (0) without the key
  return a;
}

// what cbf_fwd and cbf_hfwd (the forward over the deduplicated list) share
inline mb::CbfFwdArgs cbf_eval_args(Args& x) {
  mb::CbfFwdArgs a{};
  x("S", a.S); x("s_env", a.s_env); x("s_step", a.s_step); x("dim", a.dim); x("idx", a.idx); x("B", a.B);
  x("T", a.T); x("N", a.N); x("K", a.K); x("wpack", a.wpack); x("f_fwd", a.f_fwd); x("wvec", a.wvec);
  x("h_out", a.h_out); x("obs_r", a.obs_r); x("dist_thr", a.dist_thr); x("dist_eps", a.dist_eps);
  return a;
}

inline mb::CbfFwdArgs cbf_fwd_args(Args& x) {
  mb::CbfFwdArgs a = cbf_eval_args(x);
  x("two", a.two); x("dang", a.dang); x("valid", a.valid); x("hn_out", a.hn_out); x("dh_out", a.dh_out);
  x("counts", a.counts); x("partial", a.partial);
  a.lc = x.loss_consts<mb::LossConsts>("lc");
  return a;
}

inline mb::CbfFwdArgs cbf_hfwd_args(Args& x) {
  mb::CbfFwdArgs a = cbf_eval_args(x);
  a.two = 1;
  x("src", a.src); x("nev", a.nev); x("idx1", a.idx1); x("mask_out", a.mask_out); x("wrm", a.wrm);
  x("u_begin", a.u_begin); x("u_end", a.u_end);
  return a;
}

inline mb::CsrArgs rev_csr_args(Args& x) {
  mb::CsrArgs a{};
  x("idx", a.idx); x("G", a.G); x("N", a.N); x("K", a.K); x("Nn", a.Nn); x("ptr", a.ptr);
  x("edges", a.edges); x("ws", a.ws);
  return a;
}

// the fused BPTT combine (cdS .. cGout, K) is optional: without it the kernel reads Gn as given
inline mb::CtrlNodeBwdArgs node_bwd_args(Args& x) {
  mb::CtrlNodeBwdArgs a{};
  x("pooled", a.pooled); x("p_env", a.p_env); x("S", a.S); x("s_env", a.s_env); x("dim", a.dim); x("G", a.G);
  x("A", a.A); x("a_env", a.a_env); x("Gn", a.Gn); x("gn_env", a.gn_env); x("valid", a.valid); x("v_env", a.v_env);
  x("B", a.B); x("N", a.N); x("wrm", a.wrm); x.opt("wrm16", a.wrm16); x("o_w1", a.o_w1); x("o_w2", a.o_w2);
  x("o_w3", a.o_w3); x("o_w4", a.o_w4); x("wvec", a.wvec); x("act_coef", a.act_coef); x("dt", a.dt);
  x("sqrt3", a.sqrt3); x("act_scale", a.act_scale); x("gscale", a.gscale); x("dP", a.dP); x("dp_env", a.dp_env);
  x("ego", a.ego); x("partial", a.partial); x("init", a.init); x("chunk", a.chunk); x.opt("cdS", a.cdS);
  x.opt("cds_env", a.cds_env); x.opt("cego", a.cego); x.opt("cdEc", a.cdEc); x.opt("cptr", a.cptr);
  x.opt("cptr_env", a.cptr_env); x.opt("cedges", a.cedges); x.opt("cedges_env", a.cedges_env); x.opt("cGn", a.cGn);
  x.opt("cgn_env", a.cgn_env); x.opt("cGout", a.cGout); x.opt("cgo_env", a.cgo_env); x.opt("K", a.K);
  x("stamps", a.stamps); x.opt("a_max", a.a_max); x.opt("res", a.res);
  return a;
}

inline mb::CtrlEdgeBwdArgs edge_bwd_args(Args& x) {
  mb::CtrlEdgeBwdArgs a{};
  x("S", a.S); x("s_env", a.s_env); x("dim", a.dim); x("idx", a.idx); x("i_env", a.i_env); x("argmax", a.argmax);
  x("am_env", a.am_env); x("dP", a.dP); x("dp_env", a.dp_env); x("B", a.B); x("N", a.N); x("K", a.K);
  x("wpack", a.wpack); x("f_ew1f", a.f_ew1f); x("f_ew2tn", a.f_ew2tn); x("dEc", a.dEc); x("de_env", a.de_env);
  x("partial", a.partial); x("init", a.init); x("qsplit", a.qsplit); x.opt("w16", a.w16); x.opt("stamps", a.stamps);
  return a;
}
