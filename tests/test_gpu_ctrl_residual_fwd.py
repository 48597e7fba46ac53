"""The residual head's forward kernels (csrc/ctrl.hip node_phase<RES>: ctrl_fwd_res_kernel with and
without the stored activations, rollout_small_res_kernel) on the device; semantics in
macbf_gnn_amd/oracle.py, "Residual head".

* zero residual rows: every output of the residual kernels has the bits of the plain kernels' (both
  evaluate the same fp32 expressions and add an exact zero);
* random residual rows: A against oracle.controller_forward per tensor (README "GPU numerics": 1e-4
  fp32, 1e-2 bf16 / fp16), and per entry A - A_plain = y_res within the layer-4 bound of
  tests/ctrl_fwd_ref.py (u |relu y3| |W4_res|^T + |b4_res| u + the propagated e3) plus one fp32
  rounding of the sum, 2^-24 |A|: the kernel adds r to the plain action in fp32;
* with a_max the residual kernel clamps the full action in the Euler step and stores the raw one;
* the persistent small rollout stores the per-step driver's bits at every step (3-D, Nn = 64).

Cases (tests/ctrl_residual_cases.py): 2-D 40 x 2 (tile tail), 300, 5 (K = 5); 3-D 33 with one obstacle,
40 with two -- rows 6, 7 and 8 of the last layer, row 8 outside acc_rows8. Each under 32 / 8 / 4 agents
per wave and in fp32 / bf16 / fp16."""
import copy

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.models import CBF
from macbf_gnn_amd.ops import layout as L
from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.weights import PackedWeights
from macbf_gnn_amd.utils.params import FlatParams
from numerics import ratio_log, rel_cmp

import ctrl_fwd_ref as R
import ctrl_residual_cases as RC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
TOL = {"fp32": 1e-4, "bf16": 1e-2, "fp16": 1e-2}          # README, "GPU numerics" (forward)
PRECS = ["fp32", "bf16", "fp16"]
APWS = ["32", "8", "4"]
W4, B4 = "controller_dec_net.6.weight", "controller_dec_net.6.bias"
_NETS, _REFS = {}, {}


def _nets(D, prec, randomise, plain):
    """-> (packed weights, the controller's fp32 parameters on the CPU)."""
    key = (D, prec, randomise, plain)
    if key not in _NETS:
        res = RC.controller(D, randomise=randomise)
        ctrl = (RC.plain_twin(res) if plain else copy.deepcopy(res)).to(DEV)
        fp = FlatParams({"controller": ctrl, "cbf": CBF(2 * D).to(DEV)}, device=DEV)
        pw = PackedWeights(fp, D, DTYPES[prec])
        assert pw.residual is (not plain)
        p = {pn: fp.flat[o:o + n].view(shape).detach().cpu().clone() for m, pn, shape, o, n in fp.specs if m == "controller"}
        _NETS[key] = (pw, p)
    return _NETS[key]


def _launch(case, prec, randomise, plain, a_max=None):
    pw, _ = _nets(case["D"], prec, randomise, plain)
    B, N, D, Nn = case["B"], case["N"], case["D"], case["Nn"]
    W, prow = native.rec_width(D), L.pooled_row(prec)
    S = native.to_records(case["s"]).to(DEV).contiguous()
    Sn = torch.full((B, Nn, W), 7.0, device=DEV)
    A = torch.full((B, N, D), 7.0, device=DEV)
    pooled = torch.full((B, N, prow), float("nan"), dtype=pw.dtype, device=DEV)
    am = torch.full((B, N, 128), 77, dtype=torch.uint8, device=DEV)
    dist = torch.zeros(B, dtype=torch.int64, device=DEV)
    act = torch.zeros(B, dtype=torch.int64, device=DEV)
    G = case["G"].to(DEV).contiguous()
    idx = case["idx"].to(DEV).contiguous()
    native.ctrl_fwd(S, G, idx, pw.ctrl_w, pw.ctrl_off["ew1f"], pw.ctrl_off["nw1f"], pw.ctrl_v, A, Sn, dist, act,
                    pooled=pooled, argmax=am, prec=prec, a_max=a_max, res=pw.residual)
    torch.cuda.synchronize()
    return dict(S=S, Sn=Sn, A=A, pooled=pooled, am=am, dist=dist, act=act, G=G, idx=idx)


# ------------------------------------------------------------------------------- zero residual rows
@pytest.mark.parametrize("apw", APWS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", RC.FWD_ALL)
def test_zero_residual_rows_give_the_plain_kernels_bits(name, prec, apw, monkeypatch):
    monkeypatch.setenv("MACBF_CTRL_APW", apw)
    case = RC.fwd_case(name)
    res, plain = _launch(case, prec, False, False), _launch(case, prec, False, True)
    N = case["N"]
    assert bool((res["A"] != 7.0).any()) and bool((res["Sn"][:, :N] != 7.0).any()) and bool((res["dist"] != 0).all())
    for k in ("A", "Sn", "am", "dist", "act"):
        assert torch.equal(res[k], plain[k]), k
    assert torch.equal(res["pooled"].view(torch.int16), plain["pooled"].view(torch.int16))


# ----------------------------------------------------------------------------- random residual rows
def _reference(name, prec):
    """Once per (case, precision): the fp32 oracle's action (bf16: under emulate_bf16) and what the test
    needs of the kernel-parameter float64 reference."""
    if (name, prec) not in _REFS:
        case = RC.fwd_case(name)
        _, p = _nets(case["D"], prec, True, False)
        N = case["N"]
        s = case["s"]
        with torch.no_grad(), O.emulate_bf16(prec == "bf16"):
            a = O.controller_forward(p, s[:, :N], case["G"], case["idx"].long(), nodes=s)
        _REFS[(name, prec)] = (a, R.kernel_params(p, prec))
    return _REFS[(name, prec)]


def _residual_rows(p, pooled, S, G, prec):
    """y_res = W4[2D:] relu(y3) + b4[2D:] in float64 from the kernel's own pooled rows, and its bound by
    the layer rule of ctrl_fwd_ref (``_layer``, ``unit_errors``) propagated from zero input error."""
    B, N, D = G.shape
    s = native.from_records(S.detach().cpu()[:, :N]).double()
    g = G.detach().cpu().double()
    u1, u2 = R.unit_errors(prec)
    z, e = torch.cat([pooled, s[..., :D] - g, s[..., D:]], -1), None
    for li in (0, 2, 4):
        z, e = R._layer(z, e, p[f"controller_dec_net.{li}.weight"], p[f"controller_dec_net.{li}.bias"], u1 if li == 0 else u2)
        z = torch.relu(z)
    return R._layer(z, e, p[W4][2 * D:], p[B4][2 * D:], u2)


@pytest.mark.parametrize("apw", APWS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", RC.FWD_ALL)
def test_random_residual_rows_match_the_oracle(name, prec, apw, monkeypatch):
    monkeypatch.setenv("MACBF_CTRL_APW", apw)
    case = RC.fwd_case(name)
    a_ref, kp = _reference(name, prec)
    res, plain = _launch(case, prec, True, False), _launch(case, prec, True, True)
    what = f"{name} {prec} apw{apw}"
    A, Ap = res["A"].cpu().double(), plain["A"].cpu().double()
    assert bool(torch.isfinite(A).all())
    print(f"ERR {what} A: {rel_cmp(res['A'].cpu(), a_ref, 'A', TOL[prec]):.3e}")
    # the edge phase does not see the residual
    assert torch.equal(res["am"], plain["am"]) and torch.equal(res["pooled"].view(torch.int16), plain["pooled"].view(torch.int16))
    y, ey = _residual_rows(kp, R.pooled_value(res["pooled"], prec), res["S"], res["G"], prec)
    assert float(y.abs().max()) > 1e-3, what
    bound = ey + 2.0 ** -24 * A.abs()
    err = ((A - Ap) - y).abs()
    ratio_log(what, {"y_res": float((err / bound).max())})
    assert bool((err <= bound).all()), (what, "A - A_plain outside the layer-4 bound", int((err > bound).sum()),
                                        (err > bound).nonzero()[:6].tolist(), float((err / bound).max()))
    # the step and the sums follow the full action (ctrl_fwd_ref's own contracts, from the kernel's A)
    N = case["N"]
    snr, snb = R.next_state(res["S"], res["A"], N)
    sn = native.from_records(res["Sn"].cpu()[:, :N]).double()
    assert bool(((sn - snr).abs() <= snb).all()), what
    dref, dbnd, aref, abnd = R.sum_bounds(res["S"], res["G"], res["Sn"], res["A"], N)
    assert bool(((res["dist"].cpu().double() - dref).abs() <= dbnd).all()), what
    assert bool(((res["act"].cpu().double() - aref).abs() <= abnd).all()), what


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["n40", "3d_n33_o1"])
def test_limit_clamps_the_full_action_and_keeps_the_raw_one(name, prec):
    case = RC.fwd_case(name)
    N = case["N"]
    free = _launch(case, prec, True, False)
    a_max = R.F32(float(free["A"].abs().median()))
    sat = free["A"].abs() > a_max
    assert bool(sat.any()) and bool((~sat).any())
    lim = _launch(case, prec, True, False, a_max=a_max)
    for k in ("A", "am", "act"):                       # the raw action: stored, and what the action sum sees
        assert torch.equal(lim[k], free[k]), k
    assert not torch.equal(lim["Sn"], free["Sn"])
    snr, snb = R.next_state(lim["S"], lim["A"].clamp(-a_max, a_max), N)
    sn = native.from_records(lim["Sn"].cpu()[:, :N]).double()
    assert bool(((sn - snr).abs() <= snb).all()), (name, prec)
    # and a residual controller with zero rows under the limit has the plain limit kernel's bits
    z, zp = _launch(case, prec, False, False, a_max=a_max), _launch(case, prec, False, True, a_max=a_max)
    for k in ("A", "Sn", "am", "dist", "act"):
        assert torch.equal(z[k], zp[k]), k


# ------------------------------------------------------------------------------ persistent rollout
def _trainer(small, **kw):
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.engine.hip_engine import HipEngine
    from macbf_gnn_amd.parallel import DP
    cfg = C.TrainConfig(num_agents=40, num_envs=2, inner_loops=10, seed=3, device="hip", dim=3, num_obstacles=2,
                        ctrl_residual=True, **kw)
    old = HipEngine.small_rollout
    HipEngine.small_rollout = small
    try:
        tr = Trainer(cfg, device=DEV, dp=DP(device=DEV))
    finally:
        HipEngine.small_rollout = old
    assert tr.engine.small_rollout == small and tr.engine.Nn == 64 and tr.engine.pw.residual
    RC.randomise_trainer(tr)
    return tr


def _outputs(tr, s0, g, obs):
    eng = tr.engine
    T = eng.rollout(s0, g, obs, early_stop=True)
    torch.cuda.synchronize()
    out = dict(S=eng.S[: T + 1], idx=eng.idx[:T], dang=eng.dang[:T], cnt=eng.cnt[:T], A=eng.A[:T],
               dist=eng.dist[:T], act=eng.act[:T], pooled=eng.pooled[:T], argmax=eng.argmax[:T])
    return T, {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("kw", [dict(dtype="fp32"), dict(dtype="bf16"), dict(dtype="fp32", a_max=0.25)],
                         ids=["fp32", "bf16", "fp32-limit"])
def test_small_rollout_stores_the_per_step_drivers_bits(kw):
    """The property tests/test_gpu_small.py holds for the plain controller, at every stored step."""
    a, b = _trainer(False, **kw), _trainer(True, **kw)
    assert torch.equal(a.fp.flat, b.fp.flat)
    s0, g, obs = a.sample()
    Ta, oa = _outputs(a, s0, g, obs)
    Tb, ob = _outputs(b, s0, g, obs)
    assert Ta == Tb and Ta >= 1
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    # the residual acts: the plain twin's first action differs
    p = {pn: a.fp.flat[o:o + n].view(shape).cpu() for m, pn, shape, o, n in a.fp.specs if m == "controller"}
    st = native.from_records(oa["S"][0]).cpu()
    with torch.no_grad(), O.emulate_bf16(kw["dtype"] == "bf16"):
        full = O.controller_forward(p, st[:, :40], g.cpu(), oa["idx"][0].cpu().long(), nodes=st)
        p[W4], p[B4] = p[W4][:6], p[B4][:6]
        gains = O.controller_forward(p, st[:, :40], g.cpu(), oa["idx"][0].cpu().long(), nodes=st)
    rel_cmp(oa["A"][0].cpu(), full, "A[0]", TOL[kw["dtype"]])
    assert float((full - gains).abs().max()) > 1e-3
