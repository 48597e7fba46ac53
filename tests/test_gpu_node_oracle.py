"""The controller node backward pinned, row by row, to a float64 oracle of the SAME inputs
(ops.selfcheck.node_oracle; tests/test_node_oracle_ref.py pins that oracle to autograd on the CPU).

Four bodies run in production -- csrc/node16.h (128-agent chunks), the per-wave node_bwd_body of
csrc/ctrl.hip (chunks of 128 and 64), the cooperative node_bwd_coop (32) and the fused ctrl_bwd_step.
The other node tests compare whole training steps per tensor, or the bodies with each other; neither
sees a defect in what the bodies share (the gain-law / action-loss prologue, node_state_frag, the
valid / act_scale / gscale handling, the env strides), nor one that moves a few rows out of thousands.

* x3 (prec="fp32"): every shared case (tests/node_cases.py) on every body; no dP row and no ego row
  outside ROW_TOL |ref| + ABS_TOL |row scale| unless it is a flagged relu tie (<= 8 % of a case's
  rows, asserted on the reference alone in test_node_oracle_ref.py); weight gradients by the rule
  of test_gpu_oracle16._check_grads. Inputs have NaN-padded env strides, outputs sentinel rows.
* every precision, tolerance-free: an env with Gn = 0 and valid = 0 gives exactly zero rows and no
  other env does; rolling the agents by 37 positions leaves every agent's dP / ego bits unchanged.
* 16-bit builds against the oracle under oracle.emulate_bf16 (bf16-rounded weights) at
  test_gpu_backward.TOL_KERNEL per tensor; fp16 by test_gpu_fp16._cmp.
* node_combine and the node kernels' fused combine on the planted graphs of test_gpu_node_reduce.py,
  per component against a dense float64 sum within n_terms 2^-24 sum |terms| (n_terms - 1 fp32
  additions plus the dt G_p product); the three fused bodies' Gout bit-equal.

Reference ops: controller.py:47-61 and core.py:174-184 of the reference, differentiated by its
train.py:103."""
import types

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.models import CBF
from macbf_gnn_amd.ops import layout as L
from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.selfcheck import _knn, bad_rows, node_oracle
from macbf_gnn_amd.ops.weights import PackedWeights
from macbf_gnn_amd.utils.params import FlatParams
from numerics import rel_cmp

import node_cases as NC
from test_gpu_backward import TOL_KERNEL
from test_gpu_fp16 import _cmp as fp16_cmp
from test_gpu_node_reduce import U24, planted_graphs
from test_gpu_oracle16 import _check_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = 7.0              # rows of dP / ego past the agents keep it
PAD_ROWS = 5
BODY_IDS = [b[0] for b in NC.BODIES]
_NETS, _REFS = {}, {}


def _nets(D, prec):
    """Default-initialised controller (bf16 build: weights rounded to bf16, so the emulating oracle
    evaluates the kernel's function) -> (flat parameters, packed images, float64 parameters)."""
    if (D, prec) not in _NETS:
        ctrl = NC.controller(D).to(DEV)
        fp = FlatParams({"controller": ctrl, "cbf": CBF(2 * D).to(DEV)}, device=DEV)
        if prec == "bf16":
            with torch.no_grad():
                fp.flat.copy_(fp.flat.bfloat16().float())
        pw = PackedWeights(fp, D, DTYPES[prec])
        p64 = {pn: fp.flat[o:o + n].view(shape).detach().double().cpu() for m, pn, shape, o, n in fp.specs
               if m == "controller"}
        _NETS[(D, prec)] = (fp, pw, p64)
    return _NETS[(D, prec)]


def _reference(case, prec, key=None, Gn=None):
    """node_oracle of a built case in the arithmetic `prec` is compared with: float64 on the hi + lo
    pooled rows (fp32), under emulate_bf16 (bf16), float64 on the fp16 pooled rows (fp16). Computed
    once per (case, precision) and shared."""
    key = (case["name"], prec) if key is None else key
    if key not in _REFS:
        fp, pw, p64 = _nets(case["D"], prec)
        hi, lo = NC.split_pooled(case["pv"], pw.dtype, pw.x3)
        args = list(NC.oracle_inputs(case, hi, lo))
        if Gn is not None:
            args[5] = Gn
        with O.emulate_bf16(prec == "bf16"):
            _REFS[key] = node_oracle(p64, *args)
    return _REFS[key]


def _padded(t):
    """(B, R, C) CPU -> the same rows on the device inside a (B, R + 3, C) allocation whose other
    rows are NaN: a kernel that took the env stride for R reads them."""
    B, R, Cc = t.shape
    buf = torch.full((B, R + 3, Cc), float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :R] = t.to(DEV)
    return buf[:, :R]


def _launch(case, prec, chunk, k16, combine=None, step_edge=None):
    """One node-backward call of a built case -> raw dP / ego rows, float64 dP (hi + lo) / ego /
    flat weight gradient. step_edge: run it as the fused ctrl_bwd_step with these edge arguments."""
    fp, pw, _ = _nets(case["D"], prec)
    B, N, D = case["B"], case["N"], case["D"]
    n, W, prow = B * N, native.rec_width(D), L.pooled_row(prec)
    hi, lo = NC.split_pooled(case["pv"], pw.dtype, pw.x3)
    pooled = _padded(torch.cat([hi, lo], -1) if pw.x3 else hi)
    S = _padded(native.to_records(case["s"]))
    A = _padded(case["A"])
    Gn = _padded(native.to_records(case["Gn"]))
    if combine is not None:
        Gn = torch.full_like(Gn, float("nan"))             # the fused combine replaces it
    G = case["G"].to(DEV).contiguous()
    valid = None if case["valid"] is None else case["valid"].to(DEV)
    dev1 = lambda x: None if x is None else torch.full((1,), x, dtype=torch.float32, device=DEV)
    dPb = torch.full((n + PAD_ROWS, prow), SENTINEL, dtype=pw.dtype, device=DEV)
    egb = torch.full((n + PAD_ROWS, W), SENTINEL, dtype=torch.float32, device=DEV)
    nb = NC.blocks(case, chunk)
    if case["init"]:
        fill, part = None, torch.full((nb, native.CTRL_NODE_PARTIAL), float("nan"), device=DEV)
    else:
        fill = NC.slab_fill(nb, native.CTRL_NODE_PARTIAL).to(DEV)
        part = fill.clone()
    kw = dict(pooled=pooled, S=S, G=G, A=A, Gn=Gn, valid_t=valid, wrm=pw.ctrl_rm, offs=pw.node_rm_off, wvec=pw.ctrl_v,
              act_coef=case["act_coef"], dP=dPb[:n].view(B, N, prow), ego=egb[:n].view(B, N, W), partial=part,
              act_cnt=dev1(case["act_cnt"]), prec=prec, init=case["init"], gscale=dev1(case["gscale"]), combine=combine,
              a_max=case["a_max"])
    if step_edge is not None:
        assert chunk == 32 and not k16
        native.ctrl_bwd_step(kw, dict(step_edge, dP=kw["dP"]), nb)
    else:
        native.ctrl_node_bwd(**kw, num_blocks=nb, chunk=chunk, wrm16=pw.node_rm16 if k16 else None)
    torch.cuda.synchronize()
    assert bool((dPb[n:].float() == SENTINEL).all()) and bool((egb[n:] == SENTINEL).all()), "rows past the agents written"
    offs = {pn: o for (m, pn, shape, o, nn) in fp.specs}
    sm, dm = (L.ctrl_node16_grad_map if k16 else L.ctrl_node_grad_map)(offs, D)
    if case["init"]:
        # every workgroup's row overwritten: the whole row of the row-major slab; of node16's tile-major
        # row every element its grad map reads (its tail and unowned dW1f tile slots are never touched)
        used = part[:, torch.as_tensor(sm, device=DEV)] if k16 else part
        assert bool(torch.isfinite(used).all()), "init=True must overwrite every slab row"
    red = (part.double() if fill is None else part.double() - fill.double()).sum(0)
    g = torch.zeros(fp.numel, dtype=torch.float64, device=DEV)
    g.index_add_(0, torch.as_tensor(dm, device=DEV), red[torch.as_tensor(sm, device=DEV)])
    dPr, egr = dPb[:n].clone(), egb[:n].clone()
    dPf = dPr[:, :128].double() + (dPr[:, 128:].double() if pw.x3 else 0.0)
    return types.SimpleNamespace(dP_raw=dPr, ego_raw=egr, dP=dPf.cpu(), ego=native.from_records(egr).double().cpu(),
                                 grad=g.cpu(), fp=fp)


def _check_x3(out, ref, what):
    dP, ego, dw, tie, scales, psc, esc = ref
    for got, want, sc, nm in ((out.dP, dP, psc, "dP"), (out.ego, ego, esc, "ego")):
        bad, worst = bad_rows(got, want, tie, sc)
        print(f"ROWS {what} {nm}: worst err/tol {worst:.3f}, ties {int(tie.sum())}/{tie.numel()}")
        assert bool(torch.isfinite(got).all()), (what, nm)
        assert int(bad.sum()) == 0, (what, nm, int(bad.sum()), bad.nonzero().flatten().tolist()[:8], worst)
    _check_grads(out, out.grad, dw, scales, what + " dW")


# ------------------------------------------------------------------- x3: every case, every body
@pytest.mark.parametrize("body,chunk,k16", NC.BODIES, ids=BODY_IDS)
@pytest.mark.parametrize("name", NC.TABLE)
def test_x3_node_bwd_matches_fp64_oracle(name, body, chunk, k16):
    case = NC.build(name)
    out = _launch(case, "fp32", chunk, k16)
    _check_x3(out, _reference(case, "fp32"), f"{name} {body}")


def _scene_edge(case, prec, K=None):
    """Edge-backward arguments of the case's scene: kNN graph of its states (K neighbours, default
    min(N, TOP_K)), argmax slots of a ctrl_fwd on them."""
    fp, pw, _ = _nets(case["D"], prec)
    B, N, D = case["B"], case["N"], case["D"]
    K, W = min(N, C.TOP_K) if K is None else K, native.rec_width(D)
    s = case["s"].to(DEV)
    S = native.to_records(s).contiguous()
    idx = _knn(s, K, D)
    A = torch.zeros(B, N, D, device=DEV)
    Sn = torch.zeros_like(S)
    pooled = torch.zeros(B, N, L.pooled_row(prec), dtype=pw.dtype, device=DEV)
    am = torch.zeros(B, N, 128, dtype=torch.uint8, device=DEV)
    native.ctrl_fwd(S, case["G"].to(DEV).contiguous(), idx, pw.ctrl_w, pw.ctrl_off["ew1f"], pw.ctrl_off["nw1f"], pw.ctrl_v,
                    A, Sn, None, None, pooled=pooled, argmax=am, prec=prec)
    torch.cuda.synchronize()
    assert bool(((am < K) | (am == 255)).all())
    nb = NC.blocks(case, 32)
    return dict(S=S, idx=idx, argmax=am, wpack=pw.ctrl_w, f_ew1f=pw.ctrl_off["ew1f"], f_ew2tn=pw.ctrl_off["ew2tn"],
                dEc=torch.zeros(B, N, K, W, device=DEV), partial=torch.zeros(nb, native.CTRL_EDGE_PARTIAL, device=DEV),
                prec=prec, init=True)


@pytest.mark.parametrize("name", ["5x13", "3x43"])
def test_fused_step_equals_the_cooperative_body(name):
    """ctrl_bwd_step's node phase is node_bwd_coop: on the same inputs its dP / ego rows and slab sums
    equal ctrl_node_bwd(chunk=32) bit for bit (65 and 129 agents), which the oracle pins above."""
    case = NC.build(name)
    coop = _launch(case, "fp32", 32, False)
    step = _launch(case, "fp32", 32, False, step_edge=_scene_edge(case, "fp32"))
    assert torch.equal(step.dP_raw, coop.dP_raw) and torch.equal(step.ego_raw, coop.ego_raw)
    _check_x3(step, _reference(case, "fp32"), f"{name} ctrl_bwd_step")


# --------------------------------------------------------------- every precision, tolerance-free
@pytest.mark.parametrize("body,chunk,k16", NC.BODIES, ids=BODY_IDS)
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_zero_env_gives_exactly_zero_rows(prec, body, chunk, k16):
    """Gn = 0 and valid = 0: neither the Euler term nor the action loss reaches the env's agents."""
    zero = NC.CASES["5x13"]["valid"]
    case = NC.build("5x13", zero_env=zero)
    out = _launch(case, prec, chunk, k16)
    B, N = case["B"], case["N"]
    dP0 = (out.dP_raw.float().view(B, N, -1) == 0).all(-1)          # (B, N): rows exactly zero
    eg0 = (out.ego_raw.view(B, N, -1) == 0).all(-1)
    other = [b for b in range(B) if b != zero]
    assert bool(dP0[zero].all()) and bool(eg0[zero].all())
    assert not bool(dP0[other].any()) and not bool(eg0[other].any())


@pytest.mark.parametrize("body,chunk,k16", NC.BODIES, ids=BODY_IDS)
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_position_independence(prec, body, chunk, k16):
    """An agent's dP / ego rows are functions of its own MFMA column and lane only: rolling every
    per-agent input by 37 positions (another wave, lane, chunk and stage turn for each agent) and
    rolling the outputs back gives identical bits."""
    base = _launch(NC.build("1x225"), prec, chunk, k16)
    rolled = _launch(NC.build("1x225", roll=37), prec, chunk, k16)
    assert not torch.equal(rolled.dP_raw, base.dP_raw)
    ddp = rolled.dP_raw.roll(-37, 0) != base.dP_raw
    deg = rolled.ego_raw.roll(-37, 0) != base.ego_raw
    assert not bool(ddp.any()) and not bool(deg.any()), (int(ddp.any(-1).sum()), int(deg.any(-1).sum()),
                                                        ddp.any(-1).nonzero().flatten().tolist()[:8])


# ------------------------------------------------------- 16-bit builds vs the emulating oracle
@pytest.mark.parametrize("body,chunk,k16", NC.BODIES, ids=BODY_IDS)
@pytest.mark.parametrize("name", ["5x13", "1x300"])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_16bit_node_bwd_matches_emulated_oracle(prec, name, body, chunk, k16):
    """bf16: the oracle under emulate_bf16 with bf16-rounded weights, per tensor by relative norm at
    test_gpu_backward.TOL_KERNEL. fp16: the float64 oracle, by test_gpu_fp16's comparison (dP, ego
    and the dec-net gradient)."""
    case = NC.build(name)
    out = _launch(case, prec, chunk, k16)
    dP, ego, dw = _reference(case, prec)[:3]
    assert bool(torch.isfinite(out.dP).all()) and bool(torch.isfinite(out.ego).all())
    dec = [(pn, o, n) for m, pn, shape, o, n in out.fp.specs if pn in dw]
    if prec == "bf16":
        rel_cmp(out.dP, dP, "dP", TOL_KERNEL)
        rel_cmp(out.ego, ego, "ego", TOL_KERNEL)
        for pn, o, n in dec:
            rel_cmp(out.grad[o:o + n], dw[pn], pn, TOL_KERNEL)
    else:
        fp16_cmp(out.dP, dP, "dP")
        fp16_cmp(out.ego, ego, "ego")
        fp16_cmp(torch.cat([out.grad[o:o + n] for pn, o, n in dec]), torch.cat([dw[pn].reshape(-1) for pn, o, n in dec]),
                 "controller_dec_net")


# ------------------------------------------------------------------------------------- combine
# (K, node case, Gn given, a non-zero self record)
COMBINE = [(1, "3x24", True, False), (12, "3x24o", False, True), (16, "3x24d3", True, False),
           (12, "3x24d3", False, False), (16, "3x24", True, True)]
_CMB = {}


def _dense_combine(idx, dE, dS, eg, gn, D):
    """Dense float64 G = dS + ego + sum_k dEc[i, k] - sum over the non-self in-edges of i (+ the Euler
    adjoint [Gn_p, Gn_v + dt Gn_p]) -> (G, bound) (B, N, 2D); bound = n_terms 2^-24 sum |terms| per
    component, n_terms the non-zero terms (zeros are exact in any sum)."""
    B, N, K = idx.shape
    out = torch.zeros(B, N, 2 * D, dtype=torch.float64)
    asum, cnt = torch.zeros_like(out), torch.zeros_like(out)

    def add(t, ix=None):
        for acc, v in ((out, t), (asum, t.abs()), (cnt, (t != 0).double())):
            if ix is None:
                acc += v
            else:
                acc.scatter_add_(1, ix, v)

    add(dS.double())
    add(eg.double())
    into = (idx < N) & (idx != torch.arange(N).view(1, N, 1))
    for k in range(K):
        r = dE[:, :, k].double()
        add(r)
        add(torch.where(into[:, :, k, None], -r, torch.zeros((), dtype=torch.float64)),
            idx[:, :, k].clamp(max=N - 1)[..., None].expand(-1, -1, 2 * D))
    if gn is not None:
        g64 = gn.double()
        add(g64)
        add(torch.cat([torch.zeros(B, N, D, dtype=torch.float64), C.TIME_STEP * g64[..., :D]], -1))
    return out, cnt * U24 * asum


def _combine_inputs(K, name, with_gn, self_rec):
    """Step t+1's records on a planted graph (hub of in-degree N - 1, a node nobody lists, self edges
    in slot 0 with zero records) and their dense float64 combination G_{t+1} with its error bound."""
    key = (K, name, with_gn, self_rec)
    if key in _CMB:
        return _CMB[key]
    case = NC.build(name)
    B, N, D, Nn = case["B"], case["N"], case["D"], case["Nn"]
    nn = Nn if Nn > N else None
    idx = planted_graphs(B, N, max(K, 2), n_nodes=nn, seed=20 + K)[..., -K:] if K == 1 else \
        planted_graphs(B, N, K, n_nodes=nn, seed=20 + K)
    gen = torch.Generator().manual_seed(300 + K)
    me = torch.arange(N).view(1, N, 1)
    dE = torch.randn(B, N, K, 2 * D, generator=gen)
    selfm = idx == me
    dE[selfm] = 0.0                                   # the producers' contract: zero self records
    if self_rec:
        b0, i0, k0 = selfm.nonzero()[5].tolist()
        dE[b0, i0, k0] = torch.randn(2 * D, generator=gen)           # added once, never subtracted
    dS, eg = torch.randn(B, N, 2 * D, generator=gen), torch.randn(B, N, 2 * D, generator=gen)
    gn = torch.randn(B, N, 2 * D, generator=gen) if with_gn else None
    out, bound = _dense_combine(idx, dE, dS, eg, gn, D)
    i32 = idx.to(torch.int32).to(DEV).contiguous()
    rptr = torch.zeros(B, (nn or N) + 1, dtype=torch.int32, device=DEV)
    redges = torch.zeros(B, N * K, dtype=torch.int32, device=DEV)
    native.rev_csr(i32, rptr, redges, n_nodes=nn)
    hub_deg = (idx[0] == 1).sum()
    assert int(hub_deg) >= N - 1 and not bool(((idx[0] == 2) & ~selfm[0]).any())       # graph 0: hub 1, orphan 2
    rec = lambda x: None if x is None else native.to_records(x).to(DEV).contiguous()
    _CMB[key] = dict(case=case, K=K, out=out, bound=bound, dS=_padded(native.to_records(dS)), ego=rec(eg), dEc=rec(dE),
                     Gn=None if gn is None else _padded(native.to_records(gn)), rptr=rptr, redges=redges)
    return _CMB[key]


def _check_combine(Gout, c, what):
    got = native.from_records(Gout).double().cpu()
    err = (got - c["out"]).abs()
    pos = c["bound"] > 0
    print(f"RATIO {what} {float((err[pos] / c['bound'][pos]).max()):.4f}")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= c["bound"]).all()), (what, float((err - c["bound"]).max()))


@pytest.mark.parametrize("K,name,with_gn,self_rec", COMBINE)
def test_node_combine_matches_dense_sum(K, name, with_gn, self_rec):
    c = _combine_inputs(K, name, with_gn, self_rec)
    B, N, W = c["ego"].shape
    Gout = torch.full((B, N, W), float("nan"), device=DEV)
    native.node_combine(c["dS"], c["ego"], c["dEc"], c["rptr"], c["redges"], c["Gn"], Gout, K=K)
    torch.cuda.synchronize()
    _check_combine(Gout, c, "node_combine")


@pytest.mark.parametrize("K,name,with_gn,self_rec", COMBINE)
def test_fused_combine_matches_dense_sum_and_feeds_the_step(K, name, with_gn, self_rec):
    """The node kernels' prologue forms G_{t+1} from the same records (csrc/ctrl.hip fused_combine):
    Gout within the fp32 bound of the dense sum, the three bodies' Gout bit-equal ("same terms and
    order", docs/ARCHITECTURE.md), and the step's dP / ego the oracle's for Gn = the kernel's Gout."""
    c = _combine_inputs(K, name, with_gn, self_rec)
    case = c["case"]
    B, N, W = c["ego"].shape
    gouts = {}
    for body, chunk, k16 in NC.BODIES:
        if body == "wave64":
            continue
        Gout = torch.full((B, N, W), float("nan"), device=DEV)
        cmb = dict(dS=c["dS"], ego=c["ego"], dEc=c["dEc"], rptr=c["rptr"], redges=c["redges"], Gn=c["Gn"], Gout=Gout, K=K)
        out = _launch(case, "fp32", chunk, k16, combine=cmb)
        _check_combine(Gout, c, f"fused_combine {body}")
        gouts[body] = Gout
        ref = _reference(case, "fp32", key=("combine", K, name, with_gn, self_rec, body), Gn=Gout.cpu())
        _check_x3(out, ref, f"combine K={K} {name} {body}")
    assert torch.equal(gouts["wave128"], gouts["coop32"]) and torch.equal(gouts["wave128"], gouts["node16"])
