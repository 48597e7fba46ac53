"""The decentralised safety filter on the device (csrc/refine.hip refine_local_kernel and the loop
path's LOCAL instantiations, ops/refine.py ``coupling="local"``): the fused kernel against the loop
path bit for bit, the first iteration against the joint filter and the oracle's centre-row gradient,
locality, the planted obstacle-only graph, the exact stop, and the episodes / evaluation / validation
that run through it. Scenes: the cases of tests/test_gpu_refine.py."""
import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd import validate as V
from macbf_gnn_amd.evaluate import EvalConfig, _cbf_local, evaluate, rollout_eval
from macbf_gnn_amd.models import CBF, Controller
from macbf_gnn_amd.ops import episode, native
from macbf_gnn_amd.ops.refine import safety_filter
from numerics import rel_cmp, tie_log
from refine_local_cases import perturbed_action, planted_obstacle_graph, unaffected_rows
from test_gpu_episode import _shape_scene
from test_gpu_refine import LR, TOL, _first_iteration, _inputs, _module, _oracle, _s_next

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PRECS = ("fp32", "bf16")
LOCAL_IMPLS = ("fused", "loop")


def _filter(cbf, s, a, idx, obs, impl, coupling="local", loops=12, lr=LR, **kw):
    return safety_filter(cbf, s, a, idx, obstacles=obs, loops=loops, lr=lr, return_trace=True, impl=impl,
                         coupling=coupling, **kw)


def _assert_same(x, y, what):
    (a1, u1, v1, t1), (a2, u2, v2, t2) = x, y
    assert torch.equal(t1["counts"], t2["counts"]), (what, t1["counts"].tolist(), t2["counts"].tolist())
    assert int(u1) == int(u2) and torch.equal(v1, v2), (what, int(u1), int(u2), float(v1), float(v2))
    assert torch.equal(t1["hn"], t2["hn"]) and torch.equal(t1["active"], t2["active"]), what
    assert torch.equal(t1["delta"], t2["delta"]), (what, float((t1["delta"] - t2["delta"]).abs().max()))
    assert torch.equal(a1, a2), what


# name -> extra arguments of the call
FUSED_CASES = {
    "2d_tail": {},
    "3d_obs2": {},
    "2d_obs1_n70": {},
    "3d_obs1_n33": dict(mask=[1, 0, 1]),      # N odd: the 2-agent tiles straddle envs, one of them masked out
    "2d_n5": {},
    "2d_n1024": dict(num_blocks=16),          # 1024 tiles over 64 / 128 waves: a wave runs 16 / 8 tiles
    "3d_obs2/a_max": dict(a_max=0.5),       # the host test of the projection: the box is reached here
}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", list(FUSED_CASES))
def test_fused_equals_the_local_loop(case, prec):
    name = case.split("/")[0]
    kw = dict(FUSED_CASES[case])
    _, s, a, idx, obs = _inputs(name)
    cbf = _module(name, prec)
    mask = kw.pop("mask", None)
    if mask is not None:
        kw["env_active"] = torch.tensor(mask, dtype=torch.bool, device=DEV)
    fused = _filter(cbf, s, a, idx, obs, "fused", **kw)
    again = _filter(cbf, s, a, idx, obs, "fused", **kw)
    loop = _filter(cbf, s, a, idx, obs, "loop", **kw)
    counts = fused[3]["counts"].tolist()
    print(f"[{case} {prec}] counts {counts} used {int(fused[1])} viol {float(fused[2]):.6g}")
    assert counts[0] > 0 and bool((fused[3]["delta"] != 0).any())              # the filter had work
    _assert_same(fused, again, f"{case} {prec}: two fused runs")
    _assert_same(fused, loop, f"{case} {prec}: fused against the loop path")
    assert torch.equal(_filter(cbf, s, a, idx, obs, None, **kw)[0], fused[0])   # the default is one of the two
    if mask is not None:
        off = ~kw["env_active"]
        assert torch.equal(fused[0][off], a[off]) and not bool(fused[3]["active"][off].any())
        assert bool((fused[0][~off] != a[~off]).any())
    if "a_max" in kw:
        assert float(fused[0].abs().max()) <= kw["a_max"]
        assert bool((fused[0].abs() == kw["a_max"]).any())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["2d_tail", "3d_obs2", "2d_obs1_n70", "3d_obs1_n33", "2d_n5", "2d_n1024"])
@pytest.mark.parametrize("impl", LOCAL_IMPLS)
def test_first_iteration_against_the_joint_filter_and_the_oracle(name, prec, impl):
    """delta = 0 gives the joint filter's s': the same hn / active trace bit for bit. The step is then
    the gradient of sum(active * -hn) w.r.t. the CENTRE action alone (the neighbour nodes are the
    nominal next states, detached; the self slot is zero), at the README's gradient bounds."""
    _, s, a, idx, obs = _inputs(name)
    cbf = _module(name, prec)
    joint = _first_iteration(name, prec)
    ar, used, viol, tr = _filter(cbf, s, a, idx, obs, impl, loops=1)
    assert torch.equal(tr["hn"], joint["tr"]["hn"]) and torch.equal(tr["active"], joint["tr"]["active"])
    assert torch.equal(tr["counts"], joint["tr"]["counts"]) and torch.equal(viol, joint["viol"])
    assert int(used) == int(joint["used"])
    # the near-tie cap of test_hinge_choice, on the same hn
    tie = joint["mask"] & (joint["deriv"].abs() < 1e-3 * joint["hn"].abs().max())
    tie_log(f"local hinge near-ties {name} {prec}", int(tie.sum()), int(joint["mask"].sum()),
            int(0.05 * int(joint["mask"].sum())))
    p = {k: v.detach() for k, v in cbf.params_dict().items()}
    a_req = a.clone().requires_grad_(True)
    with O.emulate_bf16(prec == "bf16"):
        nominal = O.with_obstacles(_s_next(s, a), obs)
        hn = _cbf_local(p, _s_next(s, a_req), idx, nominal)
    g, = torch.autograd.grad((tr["active"].to(hn.dtype) * (-hn)).sum(), a_req)
    assert bool(torch.isfinite(ar).all()) and float(g.abs().max()) > 0.0
    rel_cmp((a - ar) / LR, g, f"local dloss/da {name} {prec} {impl}", TOL[prec][1])
    idle = ~tr["active"].any(-1)
    assert torch.equal(ar[idle], a[idle])                          # bit-identical where no own edge is active


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("impl", LOCAL_IMPLS)
def test_locality_on_the_device(impl, prec):
    _, s, a, idx, obs = _inputs("2d_obs1_n70")
    cbf = _module("2d_obs1_n70", prec)
    keep = unaffected_rows(idx)
    assert 0 < int(keep[0].sum()) < keep.shape[1] - 1
    d1, d2 = (_filter(cbf, s, x, idx, obs, impl, loops=6)[3]["delta"] for x in (a, perturbed_action(a)))
    assert bool((d1 != 0).any())
    assert torch.equal(d1[keep], d2[keep])
    assert not torch.equal(d1[~keep], d2[~keep])


@pytest.mark.parametrize("prec", PRECS)
def test_obstacle_only_graph_is_the_joint_filter(prec):
    """No agent lists another agent: the joint loop, the local loop and the fused kernel agree bit for bit."""
    import copy
    cbf, s, a, idx, obs = planted_obstacle_graph()
    cbf = copy.deepcopy(cbf).to(DEV)
    if prec == "bf16":
        cbf.mfma_dtype = torch.bfloat16
        with torch.no_grad():
            for q in cbf.parameters():
                q.copy_(q.bfloat16().float())
    s, a, idx, obs = s.to(DEV), a.to(DEV), idx.to(DEV), obs.to(DEV)
    joint = _filter(cbf, s, a, idx, obs, "loop", coupling="joint")
    counts = joint[3]["counts"].tolist()
    print(f"[planted {prec}] counts {counts}")
    assert counts[0] > 0 and bool((joint[3]["delta"] != 0).any())
    for impl in LOCAL_IMPLS:
        _assert_same(_filter(cbf, s, a, idx, obs, impl), joint, f"planted {prec}: local {impl} against the joint loop")


@pytest.mark.parametrize("impl", LOCAL_IMPLS)
@pytest.mark.parametrize("name,prec", [("2d_tail", "fp32"), ("3d_obs2", "fp32"), ("3d_obs2", "bf16")])
def test_stop_is_exact(name, prec, impl):
    """The recipe of test_gpu_refine.test_early_out_is_exact: under 1 % of the edges violate the condition,
    a large step clears them, and every later iteration must leave everything alone. With u the first
    iteration that counts no active edge (of the 50-loop run; 0 < u < 49 is asserted): counts[u:] is zero,
    a run of 12 loops gives the 50-loop run's counts[:12], and every run that evaluates iterate u --
    loops = u + 1, and loops = 12 where u < 12 -- equals the 50-loop run bit for bit in the actions,
    ``used``, ``viol`` and the trace.

    The local filter is slower than the joint one on the same scene: an agent clears its edge alone, its
    neighbour does not move away. Measured u: 2d_tail fp32 3 (counts 8 4 1 0 ...), 3d_obs2 fp32 12
    (9 3 2 3 1 1 1 1 1 1 1 1 0 ...), 3d_obs2 bf16 14. Where u >= 12 the 12-loop run ends before the last
    active edge is cleared, so it can only be compared in what it did evaluate."""
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
    r50 = _filter(cbf, s, a, idx, obs, impl, loops=50, lr=lr)
    r12 = _filter(cbf, s, a, idx, obs, impl, loops=12, lr=lr)
    c12, c50 = r12[3]["counts"].tolist(), r50[3]["counts"].tolist()
    u = int(r50[1])
    print(f"[{name} {prec} {impl}] u {u} counts {c50[:u + 1]}")
    assert c50[0] > 0 and 0 < u < 49 and all(c50[:u]), c50        # it did work, and it finished
    assert not any(c50[u:]), c50                                  # nothing is active after the first zero
    assert c12 == c50[:12] and int(r12[1]) == min(u, 12)
    if name == "2d_tail":
        assert u < 12, u                                          # this scene runs the 12-against-50 comparison below
    assert not torch.equal(r50[0], a)
    if u < 12:
        _assert_same(r12, r50_as(r50, 12), f"{name} {prec} {impl}: loops 12 against 50")
    _assert_same(_filter(cbf, s, a, idx, obs, impl, loops=u + 1, lr=lr), r50_as(r50, u + 1),
                 f"{name} {prec} {impl}: loops {u + 1} against 50")


def r50_as(r, loops):
    """A longer run's result with its counts cut to `loops` words, for ``_assert_same``."""
    a, used, viol, tr = r
    return a, used, viol, dict(tr, counts=tr["counts"][:loops])


# ------------------------------------------------------------------------------------- episodes
T, LOOPS = 6, 4
_EP = {}


def _episode_setup(a_max, coupling="local"):
    key = (a_max, coupling)
    if key not in _EP:
        cfg = C.TrainConfig(num_agents=32, val_envs=3, num_envs=2, inner_loops=T, seed=3, device="hip", val_every=1,
                            val_refine_loops=LOOPS, dtype="fp32", val_a_max=a_max or 0.0, val_refine_coupling=coupling)
        torch.manual_seed(3)
        ctrl, cbf = Controller(4).to(DEV), CBF(4).to(DEV)
        for m in (ctrl, cbf):
            m.eval()
            m.mfma_dtype = V.val_dtype(cfg)
        v = V.Validator(cfg, DEV)
        _shape_scene(v)
        _EP[key] = (cfg, ctrl, cbf, v)
    return _EP[key]


@pytest.mark.parametrize("a_max", [None, 0.5])
def test_validation_episodes_equal_the_python_rollout(a_max):
    """mask_done=True (validate.py's rule): the native call against ``Validator.rollout`` as torch ops with
    the same local filter -- the states bit for bit, the counts exactly."""
    cfg, ctrl, cbf, v = _episode_setup(a_max)
    seen = []
    orig = V._safe_count
    V._safe_count = lambda s, obs=None: (seen.append(s.clone()), orig(s, obs))[1]
    try:
        want = v.rollout(ctrl, cbf, refine=True)
    finally:
        V._safe_count = orig
    c = dict(zip(V.COUNTS, want.tolist()))
    print("reference", c)
    assert c["refine_iters"] > 0
    kw = dict(refine=True, loops=LOOPS, lr=C.REFINE_LEARNING_RATE, max_steps=T, top_k=cfg.top_k, coupling="local",
              return_state=True)
    if a_max is not None:
        kw.update(a_max=a_max, action_stats=True)
    for impl in (None, "fused", "loop"):
        got = episode.run_episodes(ctrl, cbf, v.s0, v.g, v.obs, impl=impl, **kw)
        vec = got[0] if a_max is None else torch.cat([got[0], got[3][:len(V.ACTION_SUMS)]])
        g, w = vec.tolist(), want.tolist()
        k = V.COUNTS.index("goal_dist_fx")
        assert abs(g[k] - w[k]) <= 1 and g[:k] + g[k + 1:] == w[:k] + w[k + 1:], (impl, g, w)
        assert torch.equal(got[1], seen[-1]), (impl, float((got[1] - seen[-1]).abs().max()))
    joint = episode.run_episodes(ctrl, cbf, v.s0, v.g, v.obs, **dict(kw, coupling="joint"))
    assert not torch.equal(joint[1], seen[-1])                     # the coupling is not a no-op on this scene


@pytest.mark.parametrize("a_max", [None, 0.5])
def test_evaluation_episodes_equal_the_python_loop(a_max):
    """mask_done=False (evaluate.py's rule) through ``rollout_eval``: the native rollout against the Python
    loop with the device-resident local filter."""
    cfg, ctrl, cbf, v = _episode_setup(a_max)
    ec = dict(num_agents=cfg.num_agents, num_envs=v.s0.shape[0], max_steps=T, refine=True, refine_loops=LOOPS,
              top_k=cfg.top_k, dim=cfg.dim, refine_impl="native", refine_coupling="local", a_max=a_max)
    want = rollout_eval(ctrl, cbf, v.s0, v.g, EvalConfig(**ec), obstacles=v.obs)
    got = rollout_eval(ctrl, cbf, v.s0, v.g, EvalConfig(rollout_impl="native", **ec), obstacles=v.obs)
    print("native", got, "reference", want)
    assert set(got) == set(want) and want["refine_iters"] > 0
    for k in want:
        if k == "mean_goal_dist":
            assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k])
        else:
            assert got[k] == want[k], (k, got[k], want[k])


def test_evaluate_and_validate_with_local_coupling():
    torch.manual_seed(0)                      # the initialisation of test_gpu_refine.test_evaluate_native_filter
    ctrl, cbf = Controller(4).to(DEV), CBF(4).to(DEV)
    base = dict(num_agents=64, num_envs=2, episodes=1, max_steps=4, refine_loops=3, refine_impl="native")
    for rollout_impl in ("python", "native"):
        m = evaluate(ctrl, cbf, EvalConfig(refine_coupling="local", rollout_impl=rollout_impl, **base), device=DEV)
        assert 0.0 <= m["safety_rate"] <= 1.0 and 0.0 <= m["reaching_rate"] <= 1.0 and m["agent_steps"] > 0
        assert m["refine_iters"] > 0
    keys = {}
    for coupling in ("joint", "local"):
        for impl in V.IMPLS:
            cfg, ctrl, cbf, _ = _episode_setup(None, coupling)
            out = V.Validator(cfg, DEV, impl=impl).validate(ctrl, cbf)
            keys[coupling, impl] = set(out)
            assert 0.0 <= out["val_refined_safety_rate"] <= 1.0
    assert len({frozenset(k) for k in keys.values()}) == 1, keys


def test_local_filter_launches_no_reverse_csr(monkeypatch):
    _, s, a, idx, obs = _inputs("2d_tail")
    cbf = _module("2d_tail", "fp32")

    def boom(*args, **kw):
        raise AssertionError("rev_csr was launched")
    monkeypatch.setattr(native, "rev_csr", boom)
    for impl in LOCAL_IMPLS:
        _filter(cbf, s, a, idx, obs, impl, loops=2)
    with pytest.raises(AssertionError, match="rev_csr"):
        _filter(cbf, s, a, idx, obs, "loop", coupling="joint", loops=2)
