"""Training under an actuator limit on the device (macbf_gnn_amd/oracle.py, "Actuator limit"): the
rollout's clamp is exact, a limit far away is no limit, every node-backward body masks dL/da like
torch.clamp's autograd along the engine's own trajectory, the mask is exact at the boundary, the per-T
backward graphs carry the limit, and a Trainer trains under it. Scenes and limits:
tests/train_limit_cases.py (the oracle's share condition: tests/test_train_limit.py).
Reference ops: the rollout /root/reference/train.py:58-81, differentiated by train.py:103."""
import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.ops import native

import train_limit_cases as TL
from numerics import rel_cmp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _trainer(name, small=None, **kw):
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.engine.hip_engine import HipEngine
    from macbf_gnn_amd.parallel import DP
    old = HipEngine.small_rollout
    if small is not None:
        HipEngine.small_rollout = small
    try:
        return Trainer(TL.config(name, "hip", **kw), device=DEV, dp=DP(device=DEV))
    finally:
        HipEngine.small_rollout = old


def _round_params(tr):
    with torch.no_grad():
        tr.fp.flat.copy_(tr.fp.flat.bfloat16().float())
    tr.engine.after_update()


def _share(tr, T):
    """Share of the kernels' raw action components outside the limit: inside the cases' band."""
    e = tr.engine
    valid = e.valid_buf[:T] != 0
    got = TL.saturated_share(e.A[:T], valid, e.a_max)
    assert TL.SHARE_BAND[0] <= got <= TL.SHARE_BAND[1], got
    return got


# ----------------------------------------------------------------------------- the forward is exact
@pytest.mark.parametrize("name,kw,small", [
    ("n32", {}, True),                                               # the persistent one-launch rollout
    ("n96_3d", {}, False),                                           # the per-step driver
    ("n32", dict(add_noise_prob=1.0, noise_scale=0.3), True),        # noise, then the clamp
    ("n32", dict(dtype="bf16"), True), ("n32", dict(dtype="fp16"), True),
    # the per-step driver's limit kernels of the 16-bit builds (3-D and 2-D)
    ("n96_3d", dict(dtype="bf16"), False), ("n128", dict(dtype="fp16"), False),
])
def test_forward_applies_the_clamp_exactly(name, kw, small):
    tr = _trainer(name, **kw)
    e = tr.engine
    assert bool(e.small_rollout) == small
    s0, g, obs = tr.sample()
    T = int(float(e.step(s0, g, obs)["T"]))
    torch.cuda.synchronize()
    N, D = e.N, e.D
    S = native.from_records(e.S[: T + 1, :, :N])                     # (T+1, B, N, 2D)
    A = e.A[:T]
    a = torch.tensor(e.a_max, dtype=torch.float32, device=DEV)
    assert torch.isfinite(A).all() and bool((A.abs() > a).any()) and bool((A.abs() < a).any())
    u = torch.where(A < -a, -a, torch.where(A > a, a, A))
    assert torch.equal(u, A.clamp(-e.a_max, e.a_max))
    dt = float(C.TIME_STEP)
    assert torch.equal(S[1:, ..., D:], S[:-1, ..., D:] + u * dt)
    assert torch.equal(S[1:, ..., :D], S[:-1, ..., :D] + S[:-1, ..., D:] * dt)
    _share(tr, T)
    if kw.get("add_noise_prob"):                                    # the noise is in A: it is not the noiseless run's
        tr0 = _trainer(name)
        tr0.engine.step(s0, g, obs)
        assert not torch.equal(tr0.engine.A[0], A[0])


def test_persistent_rollout_matches_per_step_driver_under_limit():
    out = []
    for small in (False, True):
        tr = _trainer("n32", small=small, inner_loops=40, early_stop=True, num_envs=4, seed=3)
        assert bool(tr.engine.small_rollout) == small
        s0, g, obs = tr.sample()
        e = tr.engine
        T = int(e.rollout(s0, g, obs))
        torch.cuda.synchronize()
        out.append((T, e.S[: T + 1].clone(), e.A[:T].clone(), e.idx[:T].clone()))
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert torch.equal(a, b)
    assert bool((out[0][2].abs() > 0.2).any())


# ----------------------------------------------------------------------------- far away = off
@pytest.mark.parametrize("name", ["n32", "n96_3d"])
def test_limit_far_away_equals_limit_off(name):
    res = []
    for a_max in (1e30, 0.0):
        tr = _trainer(name, a_max=a_max)
        s0, g, obs = tr.sample()
        st = tr.engine.step(s0, g, obs)
        T = int(float(st["T"]))
        torch.cuda.synchronize()
        res.append((tr.engine.S[: T + 1].clone(), tr.engine.A[:T].clone(), tr.fp.grad.clone(), st.raw[:16].clone()))
    assert res[0][0].shape == res[1][0].shape
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- gradients vs the oracle
BODIES = {
    # the cooperative 32-agent body on the persistent rollout's stored activations
    "coop": ("n32", {}, {}),
    "node16": ("n128", {}, dict(MACBF_NODE_CHUNK="128", MACBF_NODE16="1", MACBF_BWD_FUSED="0")),
    "wave32": ("n128", {}, dict(MACBF_NODE_CHUNK="128", MACBF_NODE16="0", MACBF_BWD_FUSED="0")),
    "fused": ("n128", {}, dict(MACBF_BWD_FUSED="1")),
    "nobptt": ("n32", dict(bptt=False), {}),
    "3d_obstacles": ("n40_3d", {}, {}),
    "coop_bf16": ("n32", dict(dtype="bf16"), {}),
    "coop_fp16": ("n32", dict(dtype="fp16"), {}),
}


@pytest.mark.parametrize("body", sorted(BODIES))
def test_gradient_matches_oracle_along_engine_trajectory(body, monkeypatch):
    """The engine's flat gradient against autograd through oracle.rollout(forced=engine.trajectory(T),
    a_max=A) (states, graphs, max-pool slots and the saturation decisions are the engine's), per
    parameter tensor: fp32 1e-3, bf16 2e-2 under emulate_bf16 with bf16 weights; fp16 as
    tests/test_gpu_fp16.py bounds an fp16 step (0.12 relative, cosine 0.99 per network). The mask is
    exercised: the controller gradient is further than that from the same trajectory's unlimited one."""
    from macbf_gnn_amd.engine.oracle_engine import OracleEngine
    name, kw, env = BODIES[body]
    for k, v in env.items():                      # before the engine is built
        monkeypatch.setenv(k, v)
    tr = _trainer(name, **kw)
    e = tr.engine
    prec = tr.cfg.dtype
    tot = e.B * e.N
    if body == "coop":
        assert e.small_rollout and e.node_acts is not None and native.node_bwd_chunk(tot, DEV) == 32
    if body == "node16":
        assert e._node16(tot) is not None
    if body == "wave32":
        assert e._node16(tot) is None and native.node_bwd_chunk(tot, DEV) == 128
    if body == "fused":
        assert native.bwd_step_fused(tot, DEV) and e.native_bptt
    if prec == "bf16":
        _round_params(tr)
    s0, g, obs = tr.sample()
    stats = e.step(s0, g, obs)
    T = int(float(stats["T"]))
    g_hip = tr.fp.grad.clone()
    assert torch.isfinite(g_hip).all()
    _share(tr, T)
    forced = e.trajectory(T)
    assert forced["sat"].dtype == torch.int8 and tuple(forced["sat"].shape) == (e.B, T, e.N, e.D)
    assert torch.equal(forced["A"], e.A[:T].transpose(0, 1))
    oe = OracleEngine(tr)
    with O.emulate_bf16(prec == "bf16"):
        oe.step(s0, g, obs, forced=forced)
        g_ref = tr.fp.grad.clone()
        oe.a_max = None                                    # the same trajectory without the mask
        oe.step(s0, g, obs, forced={k: v for k, v in forced.items() if k != "sat"})
        g_off = tr.fp.grad.clone()
    lo, hi = tr.fp.ranges["controller"]
    if prec == "fp16":
        tol = 0.12
        for net in ("controller", "cbf"):
            a_, b_ = tr.fp.ranges[net]
            rel_cmp(g_hip[a_:b_], g_ref[a_:b_], net, tol, cos=0.99)
    else:
        tol = 2e-2 if prec == "bf16" else 1e-3
        for m, pn, shape, o, n in tr.fp.specs:
            rel_cmp(g_hip[o:o + n], g_ref[o:o + n], f"{m}.{pn}", tol)
    diff = float((g_ref[lo:hi] - g_off[lo:hi]).double().norm() / g_ref[lo:hi].double().norm())
    assert diff > tol, diff


# ----------------------------------------------------------------------------- the mask at the boundary
@pytest.mark.parametrize("body,env", [("coop", {}), ("wave32", dict(MACBF_NODE_CHUNK="128", MACBF_NODE16="0")),
                                      ("node16", dict(MACBF_NODE_CHUNK="128", MACBF_NODE16="1"))])
def test_mask_is_exact_at_the_boundary(body, env, monkeypatch):
    """One node-backward launch (N = 32, B = 1, one step, act_coef = 0, dL/dv' = 1 for every agent) on
    planted actions: agent 3 has both components at exactly a_max (the boundary passes), agent 7 at
    nextafter(a_max, inf), agent 11 at NaN. With every component of an agent masked its dL/da is zero,
    so its rows of dL/dpooled and of the ego gradient are exactly zero; agent 3's are not."""
    from macbf_gnn_amd.ops import graph
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tr = _trainer("n32", num_envs=1)
    e, pw = tr.engine, tr.engine.pw
    a_max = e.a_max
    s0, g, _ = tr.sample()
    S = graph.node_records(s0, None)
    idx = graph.knn(s0, e.K)
    B, N, D = 1, 32, 2
    A = torch.zeros(B, N, D, device=DEV)
    pooled = torch.zeros(B, N, e.prow, dtype=e.hdt, device=DEV)
    am = torch.zeros(B, N, 128, dtype=torch.uint8, device=DEV)
    native.ctrl_fwd(S, g, idx, pw.ctrl_w, pw.ctrl_off["ew1f"], pw.ctrl_off["nw1f"], pw.ctrl_v, A, None, None, None,
                    pooled=pooled, argmax=am, prec=e.prec)
    I, J, Kk = 3, 7, 11
    at = torch.tensor(a_max, dtype=torch.float32)
    A[0, I] = at
    A[0, J] = torch.nextafter(at, torch.tensor(float("inf")))
    A[0, Kk] = float("nan")
    A[0, 5] = -at                                                # the lower boundary passes too
    A[0, 9] = torch.nextafter(-at, torch.tensor(float("-inf")))
    Gn = torch.zeros(B, N, 4, device=DEV)
    Gn[..., 2:] = 1.0
    wrm16 = e.node16_w if body == "node16" else None
    assert (wrm16 is not None) == (body == "node16")
    chunk = 128 if body != "coop" else 32
    nbn = native.ctrl_bwd_grids(B * N, DEV, e.prec)[0]
    valid = torch.ones(B, dtype=torch.uint8, device=DEV)

    def run(limit):
        dP = torch.zeros(B, N, e.prow, dtype=e.hdt, device=DEV)
        ego = torch.zeros(B, N, 4, device=DEV)
        pn = torch.zeros(nbn, native.CTRL_NODE_PARTIAL, device=DEV)
        native.ctrl_node_bwd(pooled, S, g, A, Gn, valid, pw.ctrl_rm, pw.node_rm_off, pw.ctrl_v, 0.0, dP, ego, pn, nbn,
                             prec=e.prec, init=True, chunk=chunk, wrm16=wrm16, a_max=limit)
        torch.cuda.synchronize()
        return dP.float(), ego

    dP, ego = run(a_max)
    for i in (I, 5):
        assert bool((ego[0, i] != 0).any()) and bool((dP[0, i] != 0).any()), i
    for j in (J, Kk, 9):
        assert bool((ego[0, j] == 0).all()) and bool((dP[0, j] == 0).all()), j
    dP0, ego0 = run(None)                                        # without the limit those rows are not zero
    assert bool((ego0[0, J] != 0).any()) and bool((dP0[0, 9] != 0).any())
    others = [i for i in range(N) if i not in (J, Kk, 9) and bool((A[0, i].abs() <= at).all())]
    assert torch.equal(ego[0, others], ego0[0, others]) and torch.equal(dP[0, others], dP0[0, others])


# ----------------------------------------------------------------------------- per-T backward graphs
def test_backward_graph_under_limit_matches_eager(monkeypatch):
    monkeypatch.setenv("MACBF_BWD_GRAPH", "0")
    a = _trainer("n32", inner_loops=20, early_stop=True)
    monkeypatch.setenv("MACBF_BWD_GRAPH", "1")
    b = _trainer("n32", inner_loops=20, early_stop=True)
    c = _trainer("n32", inner_loops=20, early_stop=True, a_max=0.5)
    assert b.engine._bwd_graph_on() and not a.engine._bwd_graph_on()
    s0, g, obs = a.sample()
    for it in range(3):
        sa = a.engine.step(s0, g, obs)
        ga = a.fp.grad.clone()
        sb = b.engine.step(s0, g, obs)
        gb = b.fp.grad.clone()
        torch.cuda.synchronize()
        assert torch.isfinite(ga).all() and torch.equal(ga, gb), it
        assert torch.equal(sa.raw[:16], sb.raw[:16]) and float(sa["T"]) == float(sb["T"]), it
    assert len(b.engine._bwd_graphs) == 1
    key = next(iter(b.engine._bwd_graphs))
    assert b.engine.a_max in key                                  # the limit is part of a graph's key
    assert b.engine._graph_suffix() != c.engine._graph_suffix()  # engines of different limits share no graph
    c.engine.step(s0, g, obs)
    assert not torch.equal(c.fp.grad, gb)


# ----------------------------------------------------------------------------- Trainer
def test_trainer_trains_under_limit_deterministically():
    flat = []
    for _ in range(2):
        tr = _trainer("n32", inner_loops=20, early_stop=True)
        for _ in range(3):
            st = tr.train_step()
        torch.cuda.synchronize()
        assert torch.isfinite(torch.tensor(float(st["loss_total"])))
        r = tr.limited_rate()
        assert 0.0 < r < 1.0, r
        flat.append((tr.fp.flat.clone(), r))
    assert torch.equal(flat[0][0], flat[1][0]) and flat[0][1] == flat[1][1]
