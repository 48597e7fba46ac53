"""The residual head in the controller node backward (macbf_gnn_amd/oracle.py, "Residual head":
dL/dy4[2D + q] = da_q), every body at the sizes that reach it: csrc/node16.h (16 and 300 agents in 2-D,
33 in 3-D), the per-wave node_bwd_body (chunks of 128 and 64, 200 agents), the cooperative
node_bwd_coop (40 agents in 2-D, 33 in 3-D) and the fused ctrl_bwd_step, bit-equal to the cooperative
call. In 3-D row 8 of dY4 is register 4 of the h == 0 lane (32x32 layout) and register 0 of the g == 2 lane
(16x16 layout, one more lane exchange).

Compared as tests/test_gpu_node_oracle.py compares the plain law, with its helpers: dP and ego row by
row against the float64 ops.selfcheck.node_oracle (which reads the residual from the parameter shape;
tests/test_ctrl_residual.py pins it to autograd), the slab sums per parameter within 1e-4 of the sum of
|terms| plus the relu-tie rows' contribution -- and the same rule on the residual rows of dW4 / db4 alone,
which must be non-zero. The options (init, one env off, a_max, act_coef = 0, act_scale, gscale) vary over
the cases (tests/ctrl_residual_cases.py). 16-bit builds: per tensor against the emulating oracle at 2e-2.
An env with Gn = 0 and valid = 0 gives exactly zero rows; with every env off the whole slab sum is zero."""
import copy
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

import ctrl_residual_cases as RC
import node_cases as NC
from test_gpu_oracle16 import _check_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = 7.0
PAD_ROWS = 5
TOL16 = 2e-2
W4, B4 = "controller_dec_net.6.weight", "controller_dec_net.6.bias"
RUN_IDS = [f"{c}-{b}" for c, b, _, _ in RC.NODE_RUNS]
_NETS, _REFS = {}, {}


def _nets(D, prec):
    """The residual controller with random residual rows (16-bit builds: weights rounded to the build's
    16-bit type, so the emulating oracle evaluates the kernel's function) -> (flat parameters, packed
    images, float64 parameters)."""
    if (D, prec) not in _NETS:
        ctrl = copy.deepcopy(RC.controller(D)).to(DEV)
        fp = FlatParams({"controller": ctrl, "cbf": CBF(2 * D).to(DEV)}, device=DEV)
        if prec != "fp32":
            with torch.no_grad():
                fp.flat.copy_(fp.flat.to(DTYPES[prec]).float())
        pw = PackedWeights(fp, D, DTYPES[prec])
        assert pw.residual and pw.n4 == 3 * D
        p64 = {pn: fp.flat[o:o + n].view(shape).detach().double().cpu() for m, pn, shape, o, n in fp.specs
               if m == "controller"}
        _NETS[(D, prec)] = (fp, pw, p64)
    return _NETS[(D, prec)]


def _reference(case, prec):
    key = (case["name"], prec)
    if key not in _REFS:
        fp, pw, p64 = _nets(case["D"], prec)
        hi, lo = NC.split_pooled(case["pv"], pw.dtype, pw.x3)
        # float64 on the hi + lo pooled rows (fp32); rounding where the 16-bit builds round, to their type
        with O.emulate_bf16(prec != "fp32", dtype=torch.float16 if prec == "fp16" else torch.bfloat16):
            _REFS[key] = node_oracle(p64, *NC.oracle_inputs(case, hi, lo))
    return _REFS[key]


def _padded(t):
    B, R, Cc = t.shape
    buf = torch.full((B, R + 3, Cc), float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :R] = t.to(DEV)
    return buf[:, :R]


def _launch(case, prec, chunk, k16, step_edge=None):
    """One node-backward call of a built case (NaN-padded env strides, sentinel rows past the agents) ->
    raw dP / ego rows, float64 dP (hi + lo) / ego / flat weight gradient."""
    fp, pw, _ = _nets(case["D"], prec)
    B, N, D = case["B"], case["N"], case["D"]
    n, W, prow = B * N, native.rec_width(D), L.pooled_row(prec)
    hi, lo = NC.split_pooled(case["pv"], pw.dtype, pw.x3)
    pooled = _padded(torch.cat([hi, lo], -1) if pw.x3 else hi)
    S = _padded(native.to_records(case["s"]))
    A = _padded(case["A"])
    Gn = _padded(native.to_records(case["Gn"]))
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
              act_cnt=dev1(case["act_cnt"]), prec=prec, init=case["init"], gscale=dev1(case["gscale"]),
              a_max=case["a_max"], res=True)
    if step_edge is not None:
        assert chunk == 32 and not k16
        native.ctrl_bwd_step(kw, dict(step_edge, dP=kw["dP"]), nb)
    else:
        native.ctrl_node_bwd(**kw, num_blocks=nb, chunk=chunk, wrm16=pw.node_rm16 if k16 else None)
    torch.cuda.synchronize()
    assert bool((dPb[n:].float() == SENTINEL).all()) and bool((egb[n:] == SENTINEL).all()), "rows past the agents written"
    offs = {pn: o for (m, pn, shape, o, nn) in fp.specs}
    sm, dm = (L.ctrl_node16_grad_map if k16 else L.ctrl_node_grad_map)(offs, D, pw.n4)
    if case["init"]:
        used = part[:, torch.as_tensor(sm, device=DEV)] if k16 else part
        assert bool(torch.isfinite(used).all()), "init=True must overwrite every slab row"
    red = (part.double() if fill is None else part.double() - fill.double()).sum(0)
    g = torch.zeros(fp.numel, dtype=torch.float64, device=DEV)
    g.index_add_(0, torch.as_tensor(dm, device=DEV), red[torch.as_tensor(sm, device=DEV)])
    dPr, egr = dPb[:n].clone(), egb[:n].clone()
    dPf = dPr[:, :128].double() + (dPr[:, 128:].double() if pw.x3 else 0.0)
    return types.SimpleNamespace(dP_raw=dPr, ego_raw=egr, dP=dPf.cpu(), ego=native.from_records(egr).double().cpu(),
                                 grad=g.cpu(), fp=fp, part=part)


def _residual(out, name, D):
    """The residual rows of the kernel's dW4 / db4."""
    o, shape = {pn: (o, shape) for m, pn, shape, o, n in out.fp.specs}[name]
    cols = 64 if len(shape) == 2 else 1
    return out.grad[o + 2 * D * cols:o + 3 * D * cols]


def _check_x3(out, ref, what, D):
    dP, ego, dw, tie, scales, psc, esc = ref
    for got, want, sc, nm in ((out.dP, dP, psc, "dP"), (out.ego, ego, esc, "ego")):
        bad, worst = bad_rows(got, want, tie, sc)
        print(f"ROWS {what} {nm}: worst err/tol {worst:.3f}, ties {int(tie.sum())}/{tie.numel()}")
        assert bool(torch.isfinite(got).all()), (what, nm)
        assert int(bad.sum()) == 0, (what, nm, int(bad.sum()), bad.nonzero().flatten().tolist()[:8], worst)
    _check_grads(out, out.grad, dw, scales, what + " dW")
    # the residual rows alone, by the same rule: 1e-4 of their sum of |terms| + the tie rows' contribution
    for pn in (W4, B4):
        got, want = _residual(out, pn, D), dw[pn][2 * D:].reshape(-1)
        sc, st = float(scales[pn][2 * D:].norm()), float(scales[pn + "@tie"][2 * D:].norm())
        err = float((got - want).norm())
        print(f"RES {what} {pn}: err / sum|terms| {err / sc:.3e}, |rows| {float(want.norm()):.3e}")
        assert float(want.norm()) > 0 and float(got.norm()) > 0, (what, pn, "residual rows are zero")
        assert err <= 1e-4 * sc + 2 * st, (what, pn, err / sc, st / sc)


# --------------------------------------------------------------------------- x3: the issue's table
@pytest.mark.parametrize("name,body,chunk,k16", RC.NODE_RUNS, ids=RUN_IDS)
def test_x3_node_bwd_matches_fp64_oracle(name, body, chunk, k16):
    case = RC.node_case(name)
    out = _launch(case, "fp32", chunk, k16)
    _check_x3(out, _reference(case, "fp32"), f"{name} {body}", case["D"])


def _scene_edge(case, prec):
    """Edge-backward arguments of the case's scene (tests/test_gpu_node_oracle.py)."""
    fp, pw, _ = _nets(case["D"], prec)
    B, N, D = case["B"], case["N"], case["D"]
    K, W = min(N, C.TOP_K), native.rec_width(D)
    s = case["s"][:, :N].to(DEV)
    S = native.to_records(s).contiguous()
    idx = _knn(s, K, D)
    A = torch.zeros(B, N, D, device=DEV)
    pooled = torch.zeros(B, N, L.pooled_row(prec), dtype=pw.dtype, device=DEV)
    am = torch.zeros(B, N, 128, dtype=torch.uint8, device=DEV)
    native.ctrl_fwd(S, case["G"].to(DEV).contiguous(), idx, pw.ctrl_w, pw.ctrl_off["ew1f"], pw.ctrl_off["nw1f"], pw.ctrl_v,
                    A, torch.zeros_like(S), None, None, pooled=pooled, argmax=am, prec=prec, res=True)
    torch.cuda.synchronize()
    assert bool(((am < K) | (am == 255)).all())
    nb = NC.blocks(case, 32)
    return dict(S=S, idx=idx, argmax=am, wpack=pw.ctrl_w, f_ew1f=pw.ctrl_off["ew1f"], f_ew2tn=pw.ctrl_off["ew2tn"],
                dEc=torch.zeros(B, N, K, W, device=DEV), partial=torch.zeros(nb, native.CTRL_EDGE_PARTIAL, device=DEV),
                prec=prec, init=True)


@pytest.mark.parametrize("name", ["res2x20", "res1x33d3", "res3x9", "res3x9d3"])
def test_fused_step_equals_the_cooperative_body(name):
    """ctrl_bwd_step's node phase is node_bwd_coop: dP / ego rows and the node slab bit for bit. The 9-agent
    scenes have K = 9: the runtime-K instantiation ctrl_bwd_step_res_kernel<D, 0>; the others K = 12."""
    case = RC.node_case(name)
    if case["Nn"] != case["N"]:                       # the fused step's two phases share one record view
        case = dict(case, s=case["s"][:, :case["N"]].contiguous(), Nn=case["N"], name=name + "-agents")
    coop = _launch(case, "fp32", 32, False)
    step = _launch(case, "fp32", 32, False, step_edge=_scene_edge(case, "fp32"))
    assert torch.equal(step.dP_raw, coop.dP_raw) and torch.equal(step.ego_raw, coop.ego_raw)
    assert torch.equal(step.grad, coop.grad)
    _check_x3(step, _reference(case, "fp32"), f"{name} ctrl_bwd_step", case["D"])


# --------------------------------------------------------------------------------- exactly zero
@pytest.mark.parametrize("body,chunk,k16", NC.BODIES, ids=[b[0] for b in NC.BODIES])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_zero_env_gives_exactly_zero_rows(prec, body, chunk, k16):
    """Gn = 0 and valid = 0: neither the Euler term nor the action loss reaches the env's agents -- its dP
    and ego rows are exactly zero, no other env's are; with the only env off every slab sum is zero, the
    residual rows of dW4 / db4 included (3-D: row 8)."""
    zero = RC.NODE_CASES["res2x20"]["valid"]
    case = RC.node_case("res2x20", zero_env=zero)
    case = dict(case, act_coef=NC.ACT_COEF)          # the action loss on: `valid` is what keeps it out
    out = _launch(case, prec, chunk, k16)
    B, N = case["B"], case["N"]
    dP0 = (out.dP_raw.float().view(B, N, -1) == 0).all(-1)
    eg0 = (out.ego_raw.view(B, N, -1) == 0).all(-1)
    other = [b for b in range(B) if b != zero]
    assert bool(dP0[zero].all()) and bool(eg0[zero].all())
    assert not bool(dP0[other].any()) and not bool(eg0[other].any())
    assert float(_residual(out, W4, 2).abs().max()) > 0
    off = RC.node_case("res1x24d3off", zero_env=0)
    out = _launch(off, prec, chunk, k16)
    assert bool((out.dP_raw.float() == 0).all()) and bool((out.ego_raw == 0).all())
    assert bool((out.grad == 0).all())


# ------------------------------------------------------- 16-bit builds vs the emulating oracle
@pytest.mark.parametrize("name,body,chunk,k16", RC.NODE_RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_16bit_node_bwd_matches_emulated_oracle(prec, name, body, chunk, k16):
    """Per tensor by relative norm at 2e-2: bf16 against the oracle under emulate_bf16 with bf16-rounded
    weights, fp16 the same with fp16 as the 16-bit type (the builds round at the same points); the residual
    rows of dW4 / db4 as tensors of their own. (Against the float64 oracle WITHOUT the fp16 rounding two
    fp16 cases measured 2.1e-2 (dec_net.2.weight, res1x300 on node16) and 8.6e-2 (dP, res2x20 on coop32),
    the same figures with and without a loss scale on Gn: relu decisions of the fp16-rounded activations,
    which only an emulating reference shares -- tests/test_gpu_node_oracle.py allows the plain law 0.12
    there.)"""
    case = RC.node_case(name)
    D = case["D"]
    out = _launch(case, prec, chunk, k16)
    dP, ego, dw = _reference(case, prec)[:3]
    assert bool(torch.isfinite(out.dP).all()) and bool(torch.isfinite(out.ego).all())
    errs = {"dP": rel_cmp(out.dP, dP, "dP", TOL16), "ego": rel_cmp(out.ego, ego, "ego", TOL16)}
    for m, pn, shape, o, n in out.fp.specs:
        if pn in dw:
            errs[pn] = rel_cmp(out.grad[o:o + n], dw[pn], pn, TOL16)
    for pn in (W4, B4):
        assert float(dw[pn][2 * D:].norm()) > 0
        errs[pn + "[res]"] = rel_cmp(_residual(out, pn, D), dw[pn][2 * D:], pn + " residual rows", TOL16)
    print(f"ERR {name} {body} {prec}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
