"""The actuator limit on the HIP device: the projected safety filter (csrc/refine.hip, both
implementations), the limited closed-loop episodes with their action statistics (csrc/episode.hip,
``run_episodes(a_max=, action_stats=True)``) and validation under ``val_a_max``.

The projection is pinned without a tolerance: an iteration of the limited filter is an iteration of
the unlimited one at the actions fl(a_c + d_k) followed by a clamp (the kernel forms s' from the
single add a + delta, and d - lr (dt g) equals d + (0 - lr (dt g)) in fp32), so a host emulation
from ``loops=1`` calls of the unlimited filter gives the limited filter's ``delta`` bit for bit. The
unlimited filter itself is compared with outputs recorded from the commit before the limit existed
(tests/golden/action_limit_parent.pt: weights, inputs and results). The episodes are compared with
the unchanged Python rollouts (``Validator.rollout``, ``evaluate.rollout_eval``), whose per-step
values are recorded through their own ``_safe_count`` / ``action_stats`` calls. The episodes' shapes
fit one wave, so the limit kernel and the Euler step's statistics are also launched on their own at 300
agents (two workgroups, a part-filled last wave, waves that straddle envs, a masked-out env).

Filter inputs follow tests/test_gpu_refine.py (actions randn * 2, a_max = 1); the episodes start from
a random-initialised controller whose actions stay below 1, so their limit is the median of |a| of
the longest-running env at step 0. Every test first asserts that some but not all action components exceed the limit."""
import copy
import functools
import io
import json
import os

import pytest
import torch

import test_gpu_episode as EP
import test_gpu_refine as R
from macbf_gnn_amd import config as C
from macbf_gnn_amd import evaluate as EV
from macbf_gnn_amd import validate as V
from macbf_gnn_amd.evaluate import ACTION_STATS, EvalConfig, rollout_eval
from macbf_gnn_amd.models import CBF, Controller
from macbf_gnn_amd.ops import episode, graph, native
from macbf_gnn_amd.ops.refine import choose_impl, safety_filter

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
A_MAX = 1.0
LR = C.REFINE_LEARNING_RATE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "action_limit_parent.pt")


def _saturates(a, a_max):
    """The precondition of every test: some but not all components exceed the limit."""
    assert bool((a.abs() > a_max).any()) and bool((a.abs() < a_max).any())


def _box(a, a_max=A_MAX):
    a_c = a.clamp(-a_max, a_max)
    return a_c, -a_max - a_c, a_max - a_c


# ----------------------------------------------------------------------------- the filter
@functools.lru_cache(maxsize=None)
def _emulation(name, prec, loops):
    """d_0 = 0, d_{k+1} = clamp(d_k + e_k, lo, hi) with e_k the unlimited filter's one-iteration delta
    at the actions a_c + d_k -> (d_loops, per-iteration active counts, whether a clamp changed a value)."""
    _, s, a, idx, obs = R._inputs(name)
    cbf = R._module(name, prec)
    a_c, lo, hi = _box(a)
    d = torch.zeros_like(a)
    counts, projected = [], False
    for _ in range(loops):
        _, _, _, tr = safety_filter(cbf, s, a_c + d, idx, obstacles=obs, loops=1, lr=LR, return_trace=True, impl="loop")
        raw = d + tr["delta"]
        d = torch.min(torch.max(raw, lo), hi)
        projected |= bool((raw != d).any())
        counts.append(int(tr["counts"][0]))
    return d, counts, projected


@pytest.mark.parametrize("impl", ["loop", "persistent"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["2d_n5", "3d_obs1_n33"])
def test_limited_filter_is_the_clamped_chain(name, prec, impl):
    loops = 4
    _, s, a, idx, obs = R._inputs(name)
    _saturates(a, A_MAX)
    cbf = R._module(name, prec)
    want, counts, projected = _emulation(name, prec, loops)
    out, used, viol, tr = safety_filter(cbf, s, a, idx, obstacles=obs, loops=loops, lr=LR, return_trace=True, impl=impl,
                                        a_max=A_MAX)
    a_c, lo, hi = _box(a)
    d = tr["delta"]
    print(f"[{name} {prec} {impl}] counts {counts} non-zero {int((d != 0).sum())} of {d.numel()} at a bound "
          f"{int(((d == lo) | (d == hi)).sum())} projected {projected}")
    assert torch.equal(d, want), float((d - want).abs().max())
    assert tr["counts"].tolist() == counts and int(used) == sum(c > 0 for c in counts)
    assert counts[0] > 0 and float(viol) >= 0.0
    # the projection did work, and not everywhere
    assert projected
    assert bool(((d == lo) | (d == hi)).any())
    assert bool(((d != 0) & (d > lo) & (d < hi)).any())
    # the applied action: inside the box exactly, on its boundary somewhere
    assert torch.equal(out, (a_c + d).clamp(-A_MAX, A_MAX))
    assert float(out.abs().max()) == A_MAX


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name,masked", [("2d_n5", False), ("3d_obs1_n33", False), ("3d_obs1_n33", True)])
def test_persistent_equals_loop_under_a_limit(name, masked, prec):
    """45 graph nodes in the 3-D case (33 agents + 12 obstacle points); with ``masked`` env 1 of its
    three is left out (the 2-D case has one env)."""
    _, s, a, idx, obs = R._inputs(name)
    _saturates(a, A_MAX)
    cbf = R._module(name, prec)
    Nn = s.shape[1] + (0 if obs is None else obs.shape[1])
    assert native.refine_small_eligible(Nn, idx.shape[-1])
    m = None
    if masked:
        m = torch.ones(s.shape[0], dtype=torch.bool, device=DEV)
        m[1] = False
    runs = [safety_filter(cbf, s, a, idx, obstacles=obs, loops=6, lr=LR, return_trace=True, impl=impl, a_max=A_MAX,
                          env_active=m) for impl in ("loop", "persistent")]
    (o1, u1, v1, t1), (o2, u2, v2, t2) = runs
    assert torch.equal(t1["delta"], t2["delta"]) and torch.equal(o1, o2)
    assert int(u1) == int(u2) and torch.equal(v1, v2) and torch.equal(t1["counts"], t2["counts"])
    assert int(u1) > 0 and bool((t1["delta"] != 0).any())
    assert float(o1.abs().max()) == A_MAX
    if masked:
        a_c = a.clamp(-A_MAX, A_MAX)
        assert not bool(t1["delta"][1].any()) and torch.equal(o1[1], a_c[1])        # the masked env: the clamped action


@functools.lru_cache(maxsize=None)
def _golden():
    return torch.load(GOLDEN, map_location="cpu", weights_only=True)


@pytest.mark.parametrize("impl", ["loop", "persistent"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["2d_tail", "3d_obs1_n33"])
def test_without_a_limit_the_filter_is_the_parents(name, prec, impl):
    """The recorded inputs are those of tests/test_gpu_refine.py's cases; the outputs are what the filter
    gave before it had a limit (12 iterations, unmasked and with env 0 masked out)."""
    gold = _golden()
    rec = gold["cases"][name]
    s, a, idx = rec["s"].to(DEV), rec["a"].to(DEV), rec["idx"].to(DEV)
    obs = None if rec["obs"] is None else rec["obs"].to(DEV)
    assert tuple(a.shape) == (R.CASES[name][3], R.CASES[name][2], R.CASES[name][0])
    _saturates(a, A_MAX)
    cbf = CBF(2 * rec["dim"]).to(DEV)
    cbf.load_state_dict(rec["weights"])
    if prec == "bf16":
        cbf.mfma_dtype = torch.bfloat16
        with torch.no_grad():
            for p in cbf.parameters():
                p.copy_(p.bfloat16().float())
    for masked in (False, True):
        want = rec["runs"][f"{prec}/{impl}/{int(masked)}"]
        m = None
        if masked:
            m = torch.ones(s.shape[0], dtype=torch.bool, device=DEV)
            m[0] = False
        for kw in ({}, {"a_max": None}):
            out, used, viol, tr = safety_filter(cbf, s, a, idx, obstacles=obs, loops=gold["loops"], lr=gold["lr"],
                                                return_trace=True, impl=impl, env_active=m, **kw)
            assert torch.equal(out.cpu(), want["out"]), (masked, kw)
            assert int(used) == want["used"] and float(viol) == want["viol"]
            assert torch.equal(tr["counts"].cpu(), want["counts"]) and torch.equal(tr["hn"].cpu(), want["hn"])
            assert torch.equal(tr["active"].cpu(), want["active"])
            assert torch.equal(out, a + tr["delta"])
        assert want["used"] > 0


def test_filter_refuses_a_bad_limit():
    _, s, a, idx, obs = R._inputs("2d_n5")
    cbf = R._module("2d_n5", "fp32")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="a_max"):
            safety_filter(cbf, s, a, idx, obstacles=obs, loops=1, a_max=bad)


# ----------------------------------------------------------------------------- episodes
T = EP.T
LOOPS = EP.LOOPS
EP_CASES = {
    "n12x3_2d_fp32": dict(num_agents=12, val_envs=3, dtype="fp32"),
    "n12x3_2d_bf16": dict(num_agents=12, val_envs=3, dtype="bf16"),
    "n20x3_3d_obs_fp32": dict(num_agents=20, val_envs=3, dim=3, num_obstacles=1, dtype="fp32"),     # 32 graph nodes
    "n20x3_3d_obs_bf16": dict(num_agents=20, val_envs=3, dim=3, num_obstacles=1, dtype="bf16"),
}
_EP_SETUPS = {}
_EP_REFS = {}


def _ep_setup(case):
    """Networks, the shaped scenes of tests/test_gpu_episode.py (env 0 done at once, env 1 part-way, env 2
    to the horizon) and the limit: the median of the last env's |a| at step 0."""
    if case not in _EP_SETUPS:
        cfg = C.TrainConfig(num_envs=2, inner_loops=T, seed=3, device="hip", val_every=1, val_refine_loops=LOOPS,
                            **EP_CASES[case])
        torch.manual_seed(3)
        ctrl, cbf = Controller(2 * cfg.dim).to(DEV), CBF(2 * cfg.dim).to(DEV)
        for m in (ctrl, cbf):
            m.eval()
            m.mfma_dtype = V.val_dtype(cfg)
        v = V.Validator(cfg, DEV)
        EP._shape_scene(v)
        with torch.no_grad():
            a0 = ctrl(v.s0, v.g, idx=graph.knn(v.s0, min(cfg.top_k, cfg.num_agents), v.obs).long(), obstacles=v.obs)
        a_max = float(a0[-1].abs().median())             # of the env that runs to the horizon (env 0 sits on its goals)
        _saturates(a0, a_max)
        _saturates(a0[-1], a_max)
        cfg.val_a_max = a_max
        v.a_max = EV.check_a_max(a_max)
        assert v.a_max == a_max and v.impl == "python"
        _EP_SETUPS[case] = (cfg, ctrl, cbf, v, a_max)
    return _EP_SETUPS[case]


def _recorded(module, run):
    """``run()`` with the states the rollout hands to its safety count and its per-step action statistics
    recorded -> (result, states s_1 .. s_T', summed ACTION_STATS)."""
    seen, stats = [], []
    safe, acts = module._safe_count, module.action_stats
    module._safe_count = lambda s, obs=None: (seen.append(s.clone()), safe(s, obs))[1]
    module.action_stats = lambda *a: (lambda r: (stats.append(r.clone()), r)[1])(acts(*a))
    try:
        res = run()
    finally:
        module._safe_count, module.action_stats = safe, acts
    tot = torch.zeros(len(ACTION_STATS), dtype=torch.int64, device=DEV)
    for r in stats:
        tot = EV.merge_action_stats(tot, r)
    return res, seen, tot


def _ep_reference(case, refine, mask_done, impl):
    """The Python rollout, computed once per key and never changed: ``Validator.rollout`` (mask_done) or
    ``evaluate.rollout_eval`` with the device-resident filter, the filter's implementation forced."""
    key = (case, refine, mask_done, impl)
    if key not in _EP_REFS:
        cfg, ctrl, cbf, v, a_max = _ep_setup(case)
        os.environ["MACBF_REFINE_SMALL"] = "1" if impl == "persistent" else "0"
        try:
            if mask_done:
                res, seen, tot = _recorded(V, lambda: v.rollout(ctrl, cbf, refine=refine))
            else:
                ec = _eval_cfg(case, refine, a_max)
                res, seen, tot = _recorded(EV, lambda: rollout_eval(ctrl, cbf, v.s0, v.g, ec, obstacles=v.obs))
        finally:
            os.environ.pop("MACBF_REFINE_SMALL", None)
        D = cfg.dim
        dist = torch.stack([torch.linalg.vector_norm(s[..., :D] - v.g, dim=-1).mean(-1) for s in seen])
        gap = float((dist.double() - C.DIST_MIN_CHECK).abs().min())
        done = [bool((dist[:, b] < C.DIST_MIN_CHECK).any()) for b in range(dist.shape[1])]
        print(f"[{case} refine={refine} mask_done={mask_done} {impl}] steps {len(seen)} done {done} gap {gap:.3e} "
              f"stats {dict(zip(ACTION_STATS, tot.tolist()))}")
        assert gap > EP.MARGIN and done[0] and not done[-1]      # no mean distance near the threshold; the envs differ
        _EP_REFS[key] = (res, seen[-1], tot)
    return _EP_REFS[key]


def _eval_cfg(case, refine, a_max, **kw):
    cfg, _, _, v, _ = _ep_setup(case)
    return EvalConfig(num_agents=cfg.num_agents, num_envs=v.s0.shape[0], max_steps=T, refine=refine, refine_loops=LOOPS,
                      top_k=cfg.top_k, dim=cfg.dim, refine_impl="native", a_max=a_max, **kw)


def _assert_vectors(got, want, names):
    g, w = dict(zip(names, got.tolist())), dict(zip(names, want.tolist()))
    print("native", g, "reference", w)
    for k in names:
        if k == "goal_dist_fx":       # per-agent rounding at 2^-32 against one rounding of the float64 sum
            assert abs(g[k] - w[k]) <= 1, (k, g[k], w[k])
        else:
            assert g[k] == w[k], (k, g, w)


@pytest.mark.parametrize("impl", ["loop", "persistent"])
@pytest.mark.parametrize("mask_done", [True, False])
@pytest.mark.parametrize("case", list(EP_CASES))
def test_limited_episodes_equal_the_python_rollout(case, mask_done, impl):
    cfg, ctrl, cbf, v, a_max = _ep_setup(case)
    Nn = v.s0.shape[1] + (0 if v.obs is None else v.obs.shape[1])
    assert choose_impl(impl, cfg.dtype, Nn, min(cfg.top_k, cfg.num_agents)) == impl          # both are eligible here
    for refine in (False, True):
        res, s_ref, tot = _ep_reference(case, refine, mask_done, impl)
        vec, s_fin, _, acts = episode.run_episodes(ctrl, cbf, v.s0, v.g, v.obs, refine=refine, loops=LOOPS, lr=LR,
                                                   max_steps=T, top_k=cfg.top_k, mask_done=mask_done, impl=impl,
                                                   a_max=a_max, action_stats=True, return_state=True)
        assert acts.is_cuda and acts.dtype == torch.int64 and acts.shape == (len(ACTION_STATS),)
        assert torch.equal(s_fin, s_ref), float((s_fin - s_ref).abs().max())
        _assert_vectors(acts, tot, ACTION_STATS)
        st = dict(zip(ACTION_STATS, acts.tolist()))
        assert st["limited_agent_steps"] > 0
        assert st["action_abs_max"] == torch.tensor(a_max, dtype=torch.float32).view(torch.int32).item()
        if refine:
            assert st["intervened_agent_steps"] > 0 and st["delta_abs_fx"] > 0
        else:
            assert st["intervened_agent_steps"] == 0 and st["delta_abs_fx"] == 0
        if mask_done:                  # Validator.rollout's vector: COUNTS, then the three sums
            n = len(V.COUNTS)
            _assert_vectors(vec, res[:n], V.COUNTS)
            assert torch.equal(acts[:len(V.ACTION_SUMS)], res[n:])
        else:                          # rollout_eval's dict, through rollout_impl="native"
            got = rollout_eval(ctrl, cbf, v.s0, v.g, _eval_cfg(case, refine, a_max, rollout_impl="native"), obstacles=v.obs)
            print("native", got, "reference", res)
            assert set(got) == set(res) and {"limited_rate", "intervention_rate", "mean_abs_delta", "max_abs_action"} <= set(got)
            for k in got:
                if k == "mean_goal_dist":
                    assert abs(got[k] - res[k]) <= 1e-6 * abs(res[k])
                else:
                    assert got[k] == res[k], (k, got[k], res[k])
            assert got["max_abs_action"] == a_max


def test_statistics_alone_change_nothing():
    """``action_stats`` without a limit: the counts and states of the plain call, no limited agent, and a
    largest action above the limit of the limited runs."""
    case = "n12x3_2d_fp32"
    cfg, ctrl, cbf, v, a_max = _ep_setup(case)
    kw = dict(refine=True, loops=LOOPS, lr=LR, max_steps=T, top_k=cfg.top_k, return_state=True)
    vec0, s0, act0 = episode.run_episodes(ctrl, cbf, v.s0, v.g, v.obs, **kw)
    vec1, s1, act1, acts = episode.run_episodes(ctrl, cbf, v.s0, v.g, v.obs, action_stats=True, **kw)
    assert torch.equal(vec0, vec1) and torch.equal(s0, s1) and torch.equal(act0, act1)
    st = dict(zip(ACTION_STATS, acts.tolist()))
    assert st["limited_agent_steps"] == 0 and st["intervened_agent_steps"] > 0
    assert st["action_abs_max"] > torch.tensor(a_max, dtype=torch.float32).view(torch.int32).item()


# ----------------------------------------------------------------------------- the two launches alone
def _launch_inputs(D, B=3, N=100, M=4):
    """300 agents: two workgroups of the Euler step's kernel, five waves, the last one part-filled, waves
    that straddle envs; actions in +-0.5 against a limit of 0.25, a third of the corrections zero."""
    g = torch.Generator(device="cpu").manual_seed(23 + D)
    r = lambda *s: (torch.rand(*s, generator=g) - 0.5).to(DEV)
    s = r(B, N + M, 2 * D)
    A = r(B, N, D).contiguous()
    delta = (r(B, N, D) * 0.3).contiguous()
    delta[:, ::3] = 0.0
    i64 = dict(dtype=torch.int64, device=DEV)
    st = dict(S_cur=native.to_records(s), G=r(B, N, D).contiguous(), st=torch.tensor([1, 0, 0, 0, 0], **i64),
              dist_fx=torch.zeros(B, **i64), safe=torch.zeros(B, device=DEV),
              active=torch.tensor([1, 0, 1], dtype=torch.uint8, device=DEV),
              prev_active=torch.zeros(B, dtype=torch.uint8, device=DEV))
    return st, s, A, delta


@pytest.mark.parametrize("D", [2, 3])
def test_limit_kernel_is_clamp(D):
    _, _, A, _ = _launch_inputs(D)
    a_max = 0.25
    _saturates(A, a_max)
    want = A.clamp(-a_max, a_max)
    native.episode_limit(A, a_max)
    assert torch.equal(A, want) and float(A.abs().max()) == a_max
    with pytest.raises(native.NativeError, match="a_max"):
        native.episode_limit(A, None)


@pytest.mark.parametrize("with_delta", [True, False])
@pytest.mark.parametrize("a_max", [0.25, None])
@pytest.mark.parametrize("D", [2, 3])
def test_advance_statistics_alone(D, a_max, with_delta):
    st, s, A, delta = _launch_inputs(D)
    B, N = A.shape[:2]
    if a_max is not None:
        _saturates(A, a_max)
        A = A.clamp(-a_max, a_max)
    d0 = delta.clone() if with_delta else None
    u = A if d0 is None else A + d0
    if a_max is not None:
        u = u.clamp(-a_max, a_max)
    active = st["active"].bool()
    step = EV.action_stats(u, d0, active, a_max)
    acts = torch.zeros(native.EP_ACT_WORDS, dtype=torch.int64, device=DEV)
    for n in (1, 2):                                 # the words accumulate: sums add, the maximum stays
        S_next = torch.full_like(st["S_cur"], 7.0)
        dl = None if d0 is None else d0.clone()
        native.episode_advance(S_next=S_next, A=A, delta=dl, a_max=a_max, act_st=acts, **st)
        sa = s[:, :N]
        assert torch.equal(native.from_records(S_next[:, :N]), sa + torch.cat([sa[..., D:], u], -1) * C.TIME_STEP)
        assert acts.tolist() == [n * int(step[0]), n * int(step[1]), n * int(step[2]), int(step[3])], (acts, step)
        st["dist_fx"].zero_()
    c = dict(zip(ACTION_STATS, step.tolist()))
    print(D, a_max, with_delta, c)
    assert (c["limited_agent_steps"] > 0) == (a_max is not None) and c["limited_agent_steps"] < 2 * N
    assert (c["intervened_agent_steps"] > 0) == with_delta and c["intervened_agent_steps"] < 2 * N
    assert c["action_abs_max"] == int(u[active].abs().max().view(torch.int32))


# ----------------------------------------------------------------------------- validation
VAL_A_MAX = 0.25
VAL_NEW = {"val_limited_rate", "val_refined_limited_rate", "val_refined_intervention_rate", "val_refined_mean_abs_delta"}
TRAIN_CASES = {"n32_bf16": dict(num_agents=32, dtype="bf16"), "n32_fp32": dict(num_agents=32, dtype="fp32")}


def _trainer(case, **kw):
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    cfg = C.TrainConfig(num_envs=2, inner_loops=T, seed=3, device="hip", display_steps=1, val_envs=2,
                        val_refine_loops=LOOPS, **TRAIN_CASES[case], **kw)
    tr = Trainer(cfg, device=DEV, dp=DP(device=DEV))
    tr.logger.stream = io.StringIO()
    return tr


def _val_saturates(tr):
    v = V.Validator(tr.cfg, DEV)
    with torch.no_grad():
        a0 = tr.controller(v.s0, v.g, idx=graph.knn(v.s0, min(tr.cfg.top_k, tr.cfg.num_agents), v.obs).long(),
                           obstacles=v.obs)
    _saturates(a0, VAL_A_MAX)


@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_validate_native_returns_the_python_dict_under_a_limit(case):
    tr = _trainer(case, val_every=2, val_impl="native", val_a_max=VAL_A_MAX)
    tr.fit(1)                                       # one real update: not the initial weights
    _val_saturates(tr)
    nat = tr.validate()
    v = tr.validator
    assert v.impl == "native" and v.a_max == VAL_A_MAX
    nat_counts = copy.deepcopy(v.last_counts)
    v.impl = "python"
    py = tr.validate()
    print("native", nat, nat_counts, "python", py, v.last_counts)
    nat.pop("val_ms"), py.pop("val_ms")
    assert nat == py and VAL_NEW <= set(nat)
    for r in ("nominal", "refined"):
        assert set(nat_counts[r]) == set(V.COUNTS) | set(V.ACTION_SUMS)
        for k in nat_counts[r]:
            assert abs(nat_counts[r][k] - v.last_counts[r][k]) <= (1 if k == "goal_dist_fx" else 0), (r, k)
    assert nat_counts["nominal"]["limited_agent_steps"] > 0 and nat_counts["nominal"]["intervened_agent_steps"] == 0
    assert nat_counts["refined"]["intervened_agent_steps"] > 0
    for m in (tr.controller, tr.cbf):
        assert "mfma_dtype" not in m.__dict__ and m.training


@pytest.mark.parametrize("impl", ["python", "native"])
def test_training_is_bit_identical_with_limited_validation(impl):
    case = "n32_fp32"
    ref, tr = _trainer(case), _trainer(case, val_every=2, val_impl=impl, val_a_max=VAL_A_MAX)
    ref.fit(4)
    tr.fit(4)
    torch.cuda.synchronize()
    _val_saturates(tr)
    assert ref.validator is None and tr.validator is not None and tr.validator.impl == impl
    assert torch.equal(tr.fp.flat, ref.fp.flat)
    assert torch.equal(tr.opt.exp_avg, ref.opt.exp_avg) and torch.equal(tr.opt.exp_avg_sq, ref.opt.exp_avg_sq)
    assert tr.opt.steps == ref.opt.steps and tr.skipped_steps == ref.skipped_steps
    recs = [json.loads(l) for l in tr.logger.stream.getvalue().splitlines()]
    ref_recs = [json.loads(l) for l in ref.logger.stream.getvalue().splitlines()]
    vals = [r for r in recs if "val_safety_rate" in r]
    train = [r for r in recs if "loss_total" in r]
    assert [x["step"] for x in vals] == [2, 4] and len(train) == len(ref_recs) == 4
    for r, q in zip(train, ref_recs):
        r.pop("agent_steps_per_s"), q.pop("agent_steps_per_s")
        assert r == q
    for x in vals:
        assert VAL_NEW <= set(x)
        assert 0.0 < x["val_limited_rate"] <= 1.0 and 0.0 <= x["val_refined_intervention_rate"] <= 1.0
        assert x["val_refined_mean_abs_delta"] >= 0.0
