"""The device-resident CBF safety filter (csrc/refine.hip, ops/refine.py) against the oracle: the
forward at s', the hinge choice (tie-aware), the action gradient with the kernel's own choice
forced, the obstacle-index guard, the loop / early-out properties, the evaluation path and the
argument validation. Inputs are built on the host exactly as in tests/test_evaluate_nd.py."""
import copy
import functools

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import env as E
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.evaluate import EvalConfig, evaluate
from macbf_gnn_amd.models import CBF, Controller
from macbf_gnn_amd.ops import graph, native
from macbf_gnn_amd.ops.packing import module_pack
from macbf_gnn_amd.ops.refine import safety_filter
from numerics import edge_ties_to_nodes, rel_cmp, tie_log

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# name -> (dim, obstacles, N, B, seed)
CASES = {
    "2d_tail": (2, 0, 40, 2, 3),            # tile tail, B > 1
    "3d_obs2": (3, 2, 40, 2, 5),            # Nn = 64, 8-float records, obstacle neighbours
    "2d_obs1_n70": (2, 1, 70, 1, 7),        # N*K not a multiple of 32
    "3d_obs1_n33": (3, 1, 33, 3, 11),       # one agent past a 32-row tile
    "2d_n5": (2, 0, 5, 1, 13),              # K = 5
    "2d_n1024": (2, 0, 1024, 2, 17),        # grid-stride loop over many workgroups
}
TOL = {"fp32": (1e-4, 1e-3), "bf16": (1e-2, 2e-2)}       # (forward, gradient): README "GPU numerics"
LR = C.REFINE_LEARNING_RATE
DTA = C.TIME_STEP * C.ALPHA_CBF


@functools.lru_cache(maxsize=None)
def _inputs(name):
    dim, nobs, N, B, seed = CASES[name]
    s, _, obs = E.generate_scenarios(B, N, dim, nobs, seed)
    torch.manual_seed(seed)
    cbf = CBF(2 * dim)
    s = s.clone()
    s[..., dim:] = torch.randn(B, N, dim) * 0.5
    a = torch.randn(B, N, dim) * 2.0
    idx = O.knn_idx(s, min(12, N), O.with_obstacles(s, obs))
    return cbf, s.to(DEV), a.to(DEV), idx.to(DEV), (None if obs is None else obs.to(DEV))


def _module(name, prec, bias=0.0):
    cbf = copy.deepcopy(_inputs(name)[0]).to(DEV)
    with torch.no_grad():
        cbf.cbf_net[6].bias += bias
        if prec == "bf16":
            cbf.mfma_dtype = torch.bfloat16
            for p in cbf.parameters():
                p.copy_(p.bfloat16().float())
    return cbf


def _s_next(s, act):
    D = s.shape[-1] // 2
    return s + torch.cat([s[..., D:], act], -1) * C.TIME_STEP


def _oracle(cbf, prec, s, act, idx, obs):
    """(deriv, radius mask at s', hn) of every slot, differentiable in ``act``."""
    p = cbf.params_dict()
    with O.emulate_bf16(prec == "bf16"):
        with torch.no_grad():
            h = O.cbf_forward(p, s, idx, nodes=O.with_obstacles(s, obs))
        sn = _s_next(s, act)
        nodes = O.with_obstacles(sn, obs)
        hn = O.cbf_forward(p, sn, idx, nodes=nodes)
        mask = O.cbf_features(sn.detach(), idx, nodes.detach())[1].bool()
    return hn - h + DTA * h, mask, hn


@functools.lru_cache(maxsize=None)
def _first_iteration(name, prec):
    """One filter iteration + the oracle at the same point, shared by the checks below."""
    _, s, a, idx, obs = _inputs(name)
    cbf = _module(name, prec)
    ar, used, viol, tr = safety_filter(cbf, s, a, idx, obstacles=obs, loops=1, lr=LR, return_trace=True)
    a_req = a.clone().requires_grad_(True)
    deriv, mask, hn = _oracle(cbf, prec, s, a_req, idx, obs)
    flags = tr["active"]
    g, = torch.autograd.grad((flags.to(hn.dtype) * (-hn)).sum(), a_req)
    torch.cuda.synchronize()
    return dict(ar=ar, used=used, viol=viol, tr=tr, deriv=deriv.detach(), mask=mask, hn=hn.detach(), grad=g)


ALL = [(n, p) for n in CASES for p in ("fp32", "bf16")]


@pytest.mark.parametrize("name,prec", ALL)
def test_forward_at_next_state(name, prec):
    r = _first_iteration(name, prec)
    assert bool(torch.isfinite(r["tr"]["hn"]).all())
    rel_cmp(r["tr"]["hn"], r["hn"], f"hn {name} {prec}", TOL[prec][0])


@pytest.mark.parametrize("name,prec", ALL)
def test_hinge_choice(name, prec):
    r = _first_iteration(name, prec)
    deriv, mask, flags = r["deriv"], r["mask"], r["tr"]["active"]
    assert not bool((flags & ~mask).any())                       # never on outside the radius at s'
    tie = mask & (deriv.abs() < 1e-3 * r["hn"].abs().max())
    firm = mask & ~tie
    assert torch.equal(flags[firm], (deriv < 0)[firm])
    n_mask, n_tie = int(mask.sum()), int(tie.sum())
    tie_log(f"hinge near-ties {name} {prec}", n_tie, n_mask, int(0.05 * n_mask))
    n_kernel = int(r["tr"]["counts"][0])
    assert n_kernel == int(flags.sum())
    assert abs(n_kernel - int((mask & (deriv < 0)).sum())) <= n_tie
    assert int(r["used"]) == int(n_kernel > 0)


@pytest.mark.parametrize("name,prec", ALL)
def test_action_gradient_with_forced_choice(name, prec):
    _, s, a, idx, obs = _inputs(name)
    r = _first_iteration(name, prec)
    ar = r["ar"]
    assert bool(torch.isfinite(ar).all())
    rel_cmp((a - ar) / LR, r["grad"], f"dloss/da {name} {prec}", TOL[prec][1])
    touched = edge_ties_to_nodes(r["tr"]["active"], idx, a.shape[1])
    assert torch.equal(ar[~touched], a[~touched])                # bit-identical where nothing is active


def test_obstacle_neighbours_are_guarded():
    """idx holds node ids up to Nn - 1 while a / delta have N rows."""
    _, s, a, idx, obs = _inputs("3d_obs2")
    N = a.shape[1]
    assert int((idx >= N).sum()) >= 200
    assert graph.node_records(s, obs).shape[1] == 64
    r = _first_iteration("3d_obs2", "fp32")
    assert bool(torch.isfinite(r["ar"]).all()) and bool(torch.isfinite(r["tr"]["hn"]).all())
    on_obs = r["tr"]["active"] & (idx >= N)
    assert int(on_obs.sum()) > 0                                 # obstacle edges do drive the filter


@pytest.mark.parametrize("name,prec", [("2d_tail", "fp32"), ("3d_obs2", "fp32"), ("3d_obs2", "bf16"),
                                       ("2d_obs1_n70", "bf16"), ("2d_n1024", "fp32")])
def test_loop_properties(name, prec):
    _, s, a, idx, obs = _inputs(name)
    cbf = _module(name, prec)
    runs = [safety_filter(cbf, s, a, idx, obstacles=obs, loops=12, lr=LR, return_trace=True) for _ in range(2)]
    (a1, u1, v1, t1), (a2, u2, v2, t2) = runs
    assert torch.equal(a1, a2) and torch.equal(t1["counts"], t2["counts"]) and torch.equal(v1, v2)
    assert int(u1) == int(u2)
    counts = t1["counts"].tolist()
    assert int(u1) == sum(c > 0 for c in counts)
    if 0 in counts:
        assert not any(counts[counts.index(0):])
    with torch.no_grad():
        d0, _, _ = _oracle(cbf, prec, s, a, idx, obs)
        d1, _, _ = _oracle(cbf, prec, s, a1, idx, obs)
    assert float(torch.relu(-d1).sum()) <= float(torch.relu(-d0).sum())
    assert float(v1) >= 0.0


@pytest.mark.parametrize("name,prec", [("2d_tail", "fp32"), ("3d_obs2", "fp32"), ("3d_obs2", "bf16")])
def test_early_out_is_exact(name, prec):
    """A CBF copy whose last bias is raised until under 1 % of the radius-masked edges violate the
    condition (deriv moves by dt alpha bias where both h are inside the radius); a large step
    then clears the rest within a few iterations, and every later launch must leave the actions
    alone: loops = 12 and loops = 50 agree bit for bit."""
    _, s, a, idx, obs = _inputs(name)
    bias = 0.0
    for _ in range(2000):
        cbf = _module(name, prec, bias)
        with torch.no_grad():
            d, m, _ = _oracle(cbf, prec, s, a, idx, obs)
        share = float((m & (d < 0)).sum()) / float(m.sum())
        if share < 0.01:
            break
        bias += 0.002
    assert 0.0 < share < 0.01
    lr = 300.0
    a12, u12, v12, t12 = safety_filter(cbf, s, a, idx, obstacles=obs, loops=12, lr=lr, return_trace=True)
    a50, u50, v50, t50 = safety_filter(cbf, s, a, idx, obstacles=obs, loops=50, lr=lr, return_trace=True)
    c12, c50 = t12["counts"].tolist(), t50["counts"].tolist()
    assert c12[0] > 0 and c12[-1] == 0, c12                      # it did work, and it finished
    assert c50[:12] == c12 and not any(c50[12:])
    assert torch.equal(a12, a50) and int(u12) == int(u50) and torch.equal(v12, v50)
    assert not torch.equal(a12, a)


@pytest.mark.parametrize("dim,nobs", [(2, 0), (3, 1)])
def test_evaluate_native_filter(dim, nobs):
    # an initialisation whose first step already violates the condition on edges inside the radius
    # in both scenes (CPU oracle: 286 / 13 such edges); some seeds give a CBF with nothing to refine
    torch.manual_seed(0)
    ctrl, cbf = Controller(2 * dim).to(DEV), CBF(2 * dim).to(DEV)
    base = dict(num_agents=64, num_envs=2, episodes=1, max_steps=4, dim=dim, num_obstacles=nobs)
    m = evaluate(ctrl, cbf, EvalConfig(refine_loops=3, refine_impl="native", **base), device=DEV)
    assert 0.0 <= m["safety_rate"] <= 1.0 and 0.0 <= m["reaching_rate"] <= 1.0
    assert m["agent_steps"] > 0 and m["mean_goal_dist"] >= 0.0
    assert m["refine_iters"] > 0
    n0 = evaluate(ctrl, cbf, EvalConfig(refine_loops=0, refine_impl="native", **base), device=DEV)
    a0 = evaluate(ctrl, cbf, EvalConfig(refine_loops=0, refine_impl="autograd", **base), device=DEV)
    assert n0 == a0


def _raw_args(name="2d_tail", loops=2):
    _, s, a, idx, obs = _inputs(name)
    cbf = _module(name, "fp32")
    B, N, D = a.shape
    K = idx.shape[-1]
    mp = module_pack("cbf", cbf, DEV)
    w, v, rm = mp.pack(list(cbf.parameters()))
    S = graph.node_records(s, obs)
    Nn = S.shape[1]
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device=DEV)
    pos = dict(S=S, idx=idx.to(torch.int32).contiguous(), a=a.contiguous(), delta=z(B, N, D), h=z(B, N, K), wpack=w,
               f_bwd=mp.off["w1f"], wrm=rm, wvec=v, dEv=z(B, N, K, D), rptr=z(B, Nn + 1, dt=torch.int32),
               redges=z(B, N * K, dt=torch.int32), ctl=z(2 * loops, dt=torch.int64))
    return pos, dict(loops=loops, lr=LR, prec=mp.prec)


@pytest.mark.parametrize("name,prec", [("2d_obs1_n70", "fp32"), ("3d_obs2", "bf16")])
def test_one_workgroup_walks_every_tile(name, prec):
    """num_blocks = 1: every wave runs several trips of the tile loop (27 / 30 tiles over 4 / 8
    waves), so the prefetched next tile is handed over more than once. Same result as the default
    grid, bit for bit, and the gradient check of the first iteration."""
    _, s, a, idx, obs = _inputs(name)
    cbf = _module(name, prec)
    B, N, D = a.shape
    K = idx.shape[-1]
    mp = module_pack("cbf", cbf, DEV)
    w, v, rm = mp.pack(list(cbf.parameters()))
    S = graph.node_records(s, obs)
    Nn = S.shape[1]
    idx32 = idx.to(torch.int32).contiguous()
    h = torch.empty(1, B, N, K, device=DEV)
    native.cbf_fwd(S.view(1, *S.shape), idx32.view(1, B, N, K), w, mp.off["w1f"], v, two=False, h_out=h, prec=mp.prec)
    rptr = torch.empty(B, Nn + 1, dtype=torch.int32, device=DEV)
    redges = torch.empty(B, N * K, dtype=torch.int32, device=DEV)
    native.rev_csr(idx32, rptr, redges, n_nodes=Nn)
    res = []
    for nb in (None, 1):
        delta = torch.zeros(B, N, D, device=DEV)
        ctl = torch.zeros(2, dtype=torch.int64, device=DEV)
        dEv = torch.empty(B, N, K, D, device=DEV)
        used_nb = native.refine(S, idx32, a.contiguous(), delta, h.view(B, N, K), w, mp.off["w1f"], rm, v, dEv, rptr,
                                redges, ctl, loops=1, lr=LR, prec=mp.prec, num_blocks=nb)
        res.append((delta, ctl, used_nb))
    (d0, c0, nb0), (d1, c1, nb1) = res
    assert nb0 > 1 and nb1 == 1
    assert torch.equal(d0, d1) and torch.equal(c0, c1)
    r = _first_iteration(name, prec)
    assert torch.equal(a + d1, r["ar"])
    rel_cmp(-d1 / LR, r["grad"], f"dloss/da one workgroup {name} {prec}", TOL[prec][1])


def test_safety_filter_does_not_synchronise():
    """used / viol stay on the device: no call inside safety_filter may wait for the GPU."""
    _, s, a, idx, obs = _inputs("3d_obs2")
    cbf = _module("3d_obs2", "fp32")
    safety_filter(cbf, s, a, idx, obstacles=obs, loops=2, lr=LR)          # packing tables are built once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ar, used, viol = safety_filter(cbf, s, a, idx, obstacles=obs, loops=4, lr=LR)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert used.is_cuda and viol.is_cuda and used.dim() == 0 and viol.dim() == 0
    assert 0 <= int(used) <= 4 and float(viol) >= 0.0 and bool(torch.isfinite(ar).all())


@pytest.mark.parametrize("what", ["dtype", "strided_a", "big_k", "idx_shape", "h_shape", "small_ctl", "fp16"])
def test_argument_validation(what):
    pos, kw = _raw_args()
    B, N, D = pos["a"].shape
    K = pos["idx"].shape[-1]
    if what == "dtype":
        pos["delta"] = pos["delta"].double()
    elif what == "strided_a":
        pos["a"] = torch.zeros(B, N, 2 * D, device=DEV)[..., ::2]
        assert tuple(pos["a"].shape) == (B, N, D)
    elif what == "big_k":
        pos["idx"] = torch.zeros(B, N, 17, dtype=torch.int32, device=DEV)
        pos["h"] = torch.zeros(B, N, 17, device=DEV)
        pos["dEv"] = torch.zeros(B, N, 17, D, device=DEV)
        pos["redges"] = torch.zeros(B, N * 17, dtype=torch.int32, device=DEV)
    elif what == "idx_shape":
        pos["idx"] = pos["idx"][:, :-1].contiguous()
    elif what == "h_shape":
        pos["h"] = torch.zeros(B, N, K + 1, device=DEV)
    elif what == "small_ctl":
        pos["ctl"] = torch.zeros(2 * kw["loops"] - 1, dtype=torch.int64, device=DEV)
    elif what == "fp16":
        pos["wpack"] = pos["wpack"].to(torch.float16)
        pos["wrm"] = pos["wrm"].to(torch.float16)
        kw["prec"] = "fp16"
    delta0 = pos["delta"].clone()
    with pytest.raises(native.NativeError):
        native.refine(**pos, **kw)
    torch.cuda.synchronize()
    assert torch.equal(pos["delta"], delta0) and int(pos["ctl"].abs().sum()) == 0    # nothing ran
