"""The actuator limit and the action statistics on the CPU path (macbf_gnn_amd/evaluate.py
``refine_actions(a_max=)``, ``rollout_eval`` with ``EvalConfig.a_max`` / ``action_stats``, the
validation's ``val_a_max``, the refusals and the CLI flags). The Python path is the yardstick of the
native one (tests/test_gpu_action_limit.py), so its own rule is pinned here: the box holds exactly,
no limit and a limit nothing reaches are the unlimited filter bit for bit, and the statistics are
those of a step-by-step recomputation."""
import io
import json

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import env as E
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd import validate as V
from macbf_gnn_amd.evaluate import (ACTION_STATS, EvalConfig, _euler, _knn, action_metrics, action_stats, evaluate,
                                    refine_actions, rollout_eval)
from macbf_gnn_amd.models import CBF, Controller

CPU = torch.device("cpu")
KEYS = {"safety_rate", "reaching_rate", "mean_goal_dist", "steps", "agent_steps", "refine_iters"}
STAT_KEYS = {"limited_rate", "intervention_rate", "mean_abs_delta", "max_abs_action"}
LOOPS = 5


def _scene(dim=2, N=8, B=2, seed=5, bias=0.0):
    """8 agents per env with random velocities and actions, and a CBF whose head bias is shifted."""
    s, _, _ = E.generate_scenarios(B, N, dim, 0, seed)
    torch.manual_seed(seed)
    cbf = CBF(2 * dim)
    with torch.no_grad():
        cbf.cbf_net[6].bias += bias
    s = s.clone()
    s[..., dim:] = torch.randn(B, N, dim) * 0.5
    a = torch.randn(B, N, dim) * 2.0
    return cbf, s, a, O.knn_idx(s, min(12, N))


def _violation(cbf, s, a, idx):
    with torch.no_grad():
        h = cbf(s, idx=idx)
        hn = cbf(_euler(s, a), idx=idx)
    return float(torch.relu(-(hn - h + C.TIME_STEP * C.ALPHA_CBF * h)).sum())


def _violating_scene():
    """The head bias is lowered until the nominal actions violate the condition: h - h' shrinks with
    the bias (dt alpha h is the only term it does not cancel in), so a negative enough bias does it."""
    for bias in (0.0, -0.5, -1.0, -2.0, -4.0, -8.0):
        cbf, s, a, idx = _scene(bias=bias)
        if _violation(cbf, s, a, idx) > 0.0:
            return cbf, s, a, idx
    raise AssertionError("no head bias gave a violation")


def _parent_refine(cbf, s, a, idx, loops, lr=C.REFINE_LEARNING_RATE, check_every=10):
    """``refine_actions`` as it was before it knew a limit, statement for statement."""
    with torch.no_grad():
        h = cbf(s, idx=idx)
    delta = torch.zeros_like(a, requires_grad=True)
    viol = torch.zeros(())
    used = torch.zeros((), dtype=torch.int64)
    for it in range(1, loops + 1):
        s_next = _euler(s, a + delta)
        hn = cbf(s_next, idx=idx)
        viol = torch.relu(-(hn - h + C.TIME_STEP * C.ALPHA_CBF * h)).sum()
        pending = viol.detach() > 0
        used += pending.long()
        if it % check_every == 0 and not bool(pending):
            break
        g, = torch.autograd.grad(viol, delta)
        with torch.no_grad():
            delta -= lr * g
    return (a + delta).detach(), int(used), float(viol.detach())


def test_refine_actions_keeps_the_box_and_the_off_path():
    cbf, s, a, idx = _violating_scene()
    assert _violation(cbf, s, a, idx) > 0.0                       # precondition: there is something to refine
    a_max = 1.0
    assert bool((a.abs() > a_max).any()) and bool((a.abs() < a_max).any())
    out, used, _, delta = refine_actions(cbf, s, a, idx, loops=LOOPS, a_max=a_max, return_delta=True)
    assert used > 0 and bool((delta != 0).any())
    assert bool((out <= a_max).all()) and bool((out >= -a_max).all())
    a_c = a.clamp(-a_max, a_max)
    assert bool((delta >= -a_max - a_c).all()) and bool((delta <= a_max - a_c).all())
    assert torch.equal(out, (a_c + delta).clamp(-a_max, a_max))
    # off, and a limit that nothing reaches: the parent's result bit for bit
    want = _parent_refine(cbf, s, a, idx, LOOPS)
    for kw in ({}, {"a_max": None}, {"a_max": 1e30}):
        got = refine_actions(cbf, s, a, idx, loops=LOOPS, **kw)
        assert len(got) == 3 and torch.equal(got[0], want[0]) and got[1:] == want[1:], kw
    assert not torch.equal(want[0], a)


def _nets(dim=2, seed=0):
    torch.manual_seed(seed)
    return Controller(2 * dim), CBF(2 * dim)


def _eval_scene(dim=2, N=8, B=2, seed=3):
    s0, g, _ = E.generate_scenarios(B, N, dim, 0, seed)
    return s0, g


def test_rollout_eval_under_the_median_limit():
    ctrl, cbf = _nets()
    s0, g = _eval_scene()
    with torch.no_grad():
        a0 = ctrl(s0, g, idx=_knn(s0, min(C.TOP_K, s0.shape[1])))
    a_max = float(a0.abs().median())
    assert bool((a0.abs() > a_max).any()) and bool((a0.abs() < a_max).any())     # some, not all, saturate
    base = dict(num_agents=8, num_envs=2, max_steps=4, refine_loops=3)
    out = rollout_eval(ctrl, cbf, s0, g, EvalConfig(a_max=a_max, **base))
    assert set(out) == KEYS | STAT_KEYS
    assert out["limited_rate"] > 0.0 and out["max_abs_action"] == a_max
    assert 0.0 <= out["intervention_rate"] <= 1.0 and out["mean_abs_delta"] >= 0.0
    # the statistics alone change no other number, and the default dict is today's
    plain = rollout_eval(ctrl, cbf, s0, g, EvalConfig(**base))
    assert set(plain) == KEYS
    stats = rollout_eval(ctrl, cbf, s0, g, EvalConfig(action_stats=True, **base))
    assert set(stats) == KEYS | STAT_KEYS and {k: stats[k] for k in KEYS} == plain
    assert stats["limited_rate"] == 0.0 and stats["max_abs_action"] > 0.0
    # a limit nothing reaches is the unlimited run
    wide = rollout_eval(ctrl, cbf, s0, g, EvalConfig(a_max=1e30, **base))
    assert {k: wide[k] for k in KEYS} == plain and wide["limited_rate"] == 0.0
    assert wide["max_abs_action"] == stats["max_abs_action"] and wide["mean_abs_delta"] == stats["mean_abs_delta"]


def test_action_statistics_of_hand_written_actions():
    a_max = 1.0
    u = torch.tensor([[[1.0, 0.25], [-1.0, 0.5], [0.5, -0.75]],          # env 0: agents 0 and 1 at the limit
                      [[1.0, 1.0], [0.0, 0.0], [0.0, 0.0]]])             # env 1 is not counted
    delta = torch.tensor([[[0.0, 0.0], [0.5, 0.0], [-2.0 ** -21, 3.0 * 2.0 ** -21]],
                          [[9.0, 9.0], [0.0, 0.0], [0.0, 0.0]]])
    active = torch.tensor([True, False])
    st = dict(zip(ACTION_STATS, action_stats(u, delta, active, a_max).tolist()))
    # 2^-21 * 2^20 = 0.5 rounds to 0 and 1.5 to 2 (half-even, per component), 0.5 * 2^20 exactly
    assert st == {"limited_agent_steps": 2, "intervened_agent_steps": 2, "delta_abs_fx": (1 << 19) + 0 + 2,
                  "action_abs_max": torch.tensor(1.0).view(torch.int32).item()}
    m = action_metrics(st, 3, 2)
    assert m["limited_rate"] == 2 / 3 and m["max_abs_action"] == 1.0
    none = dict(zip(ACTION_STATS, action_stats(u, None, active, None).tolist()))
    assert none["limited_agent_steps"] == 0 and none["intervened_agent_steps"] == 0 and none["delta_abs_fx"] == 0


@pytest.mark.parametrize("kw,name", [(dict(a_max=0.0), "a_max"), (dict(a_max=-1.0), "a_max"),
                                     (dict(a_max=float("inf")), "a_max"), (dict(a_max=float("nan")), "a_max"),
                                     (dict(a_max=1.0, refine_space="gains"), "refine_space"),
                                     (dict(a_max=1.0, diagnose=True), "diagnose")])
def test_refusals_name_the_option(kw, name):
    ctrl, cbf = _nets()
    s0, g = _eval_scene()
    cfg = EvalConfig(num_agents=8, num_envs=2, episodes=1, max_steps=2, refine_loops=2, **kw)
    with pytest.raises(ValueError, match=name) as e:
        rollout_eval(ctrl, cbf, s0, g, cfg)
    assert "a_max" in str(e.value)
    with pytest.raises(ValueError, match=name):
        evaluate(ctrl, cbf, cfg, device=CPU)
    if set(kw) == {"a_max"}:
        cbf2, s, a, idx = _scene()
        with pytest.raises(ValueError, match="a_max"):
            refine_actions(cbf2, s, a, idx, loops=1, **kw)
        with pytest.raises(ValueError, match="val_a_max"):
            V.check_config(C.TrainConfig(num_agents=4, device="cpu", val_every=1, val_a_max=kw["a_max"] or -1.0))


def test_cli_flags(capsys):
    import evaluate as evaluate_cli
    import train
    assert train.build_config(train.parse_args(["--num_agents", "4"])).val_a_max == 0.0
    assert train.build_config(train.parse_args(["--num_agents", "4", "--val_a_max", "1.5"])).val_a_max == 1.5
    common = ["--num_agents", "6", "--episodes", "1", "--max_steps", "2", "--refine_loops", "2", "--device", "cpu"]
    out = evaluate_cli.main(common + ["--a_max", "0.5"])
    assert STAT_KEYS <= set(out) and out["a_max"] == 0.5 and out["max_abs_action"] <= 0.5
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["a_max"] == 0.5
    out = evaluate_cli.main(common + ["--action_stats"])
    assert STAT_KEYS <= set(out) and "a_max" not in out and out["limited_rate"] == 0.0
    assert not STAT_KEYS & set(evaluate_cli.main(common))
    with pytest.raises(SystemExit):
        evaluate_cli.main(common + ["--a_max", "1.0", "--diagnose"])


VAL_NEW = {"val_limited_rate", "val_refined_limited_rate", "val_refined_intervention_rate", "val_refined_mean_abs_delta"}


def _trainer(**kw):
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    cfg = C.TrainConfig(num_agents=8, num_envs=1, inner_loops=4, device="cpu", seed=5, train_steps=2, display_steps=1,
                        val_envs=2, val_refine_loops=2, **kw)
    tr = Trainer(cfg, device=CPU, dp=DP(device=CPU))
    tr.logger.stream = io.StringIO()
    return tr


def test_validation_under_a_limit():
    assert C.TrainConfig().val_a_max == 0.0
    assert V.COUNTS == ("safe_agent_steps", "agent_steps", "reached_agents", "agents", "env_steps", "refine_iters", "steps",
                        "goal_dist_fx")
    ref, off, tr = _trainer(), _trainer(val_every=1), _trainer(val_every=1, val_a_max=0.05)
    for t in (ref, off, tr):
        t.fit(2)
    assert torch.equal(tr.fp.flat, ref.fp.flat) and torch.equal(off.fp.flat, ref.fp.flat)    # training is not touched
    vals = [json.loads(l) for l in tr.logger.stream.getvalue().splitlines() if "val_safety_rate" in l]
    vals_off = [json.loads(l) for l in off.logger.stream.getvalue().splitlines() if "val_safety_rate" in l]
    assert len(vals) == len(vals_off) == 2
    for r, q in zip(vals, vals_off):
        assert set(r) == set(q) | VAL_NEW and not VAL_NEW & set(q)
        assert 0.0 < r["val_limited_rate"] <= 1.0 and 0.0 <= r["val_refined_intervention_rate"] <= 1.0
        assert r["val_refined_mean_abs_delta"] >= 0.0
    c = tr.validator.last_counts
    assert set(c["nominal"]) == set(V.COUNTS) | set(V.ACTION_SUMS) == set(c["refined"])
    assert c["nominal"]["intervened_agent_steps"] == 0 and c["nominal"]["delta_abs_fx"] == 0
    assert set(off.validator.last_counts["nominal"]) == set(V.COUNTS)
    # the rollout's vector: COUNTS, then the sums
    vec = tr.validator.rollout(tr.controller, tr.cbf, refine=False)
    assert vec.shape == (len(V.COUNTS) + len(V.ACTION_SUMS),)
    assert off.validator.rollout(off.controller, off.cbf, refine=False).shape == (len(V.COUNTS),)
