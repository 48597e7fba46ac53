"""Evaluation of every scene family the trainer supports (3-D, static obstacles) on the CPU oracle
path, the 2-D regression pin of the unchanged default path, the CLI switches, and the static
hazard scan of the safety-filter objects."""
import glob
import json
import os
import subprocess
import sys

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import env as E
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.evaluate import EvalConfig, _knn, _safe_count, evaluate, refine_actions
from macbf_gnn_amd.models import CBF, Controller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(dim=3, nobs=2, N=40, B=2, seed=5):
    """The inputs of the GPU filter tests (tests/test_gpu_refine.py), on the CPU."""
    s, _, obs = E.generate_scenarios(B, N, dim, nobs, seed)
    torch.manual_seed(seed)
    cbf = CBF(2 * dim)
    s = s.clone()
    s[..., dim:] = torch.randn(B, N, dim) * 0.5
    a = torch.randn(B, N, dim) * 2.0
    nodes = O.with_obstacles(s, obs)
    idx = O.knn_idx(s, min(12, N), nodes)
    return cbf, s, a, idx, obs


def _deriv(cbf, s, a, idx, obs):
    """deriv of every slot through the oracle, independently of evaluate.py's own arithmetic."""
    p = cbf.params_dict()
    D = s.shape[-1] // 2
    with torch.no_grad():
        h = O.cbf_forward(p, s, idx, nodes=O.with_obstacles(s, obs))
        sn = s + torch.cat([s[..., D:], a], -1) * C.TIME_STEP
        hn = O.cbf_forward(p, sn, idx, nodes=O.with_obstacles(sn, obs))
    return hn - h + C.TIME_STEP * C.ALPHA_CBF * h


def _touched(deriv, idx, N):
    """(B, N) agents with at least one violating incident edge, as centre or as neighbour."""
    bad = deriv < 0
    out = bad.any(-1).clone()
    for b in range(bad.shape[0]):
        j = idx[b][bad[b]]
        out[b, j[j < N]] = True
    return out


@pytest.mark.parametrize("dim", [3, 2])
def test_evaluate_with_obstacles_metrics_ranges(dim):
    torch.manual_seed(1)
    m = evaluate(Controller(2 * dim), CBF(2 * dim),
                 EvalConfig(num_agents=10, num_envs=2, episodes=1, max_steps=4, refine_loops=3, dim=dim,
                            num_obstacles=1))
    assert 0.0 <= m["safety_rate"] <= 1.0 and 0.0 <= m["reaching_rate"] <= 1.0
    assert m["agent_steps"] > 0 and m["mean_goal_dist"] >= 0.0


def test_refine_actions_with_obstacles_reduces_violation():
    cbf, s, a, idx, obs = _case()
    N = s.shape[1]
    assert int((idx >= N).sum()) > 0                 # obstacle neighbours take part
    d0 = _deriv(cbf, s, a, idx, obs)
    v0 = float(torch.relu(-d0).sum())
    # one iteration: exactly the agents of the violating edges move
    a1, _, _ = refine_actions(cbf, s, a, idx, loops=1, obstacles=obs)
    moved = (a1 != a).any(-1)
    assert not bool((moved & ~_touched(d0, idx, N)).any())
    # five iterations: the violation does not increase; agents that never had a violating incident
    # edge along the way keep their action
    ar, it, vend = refine_actions(cbf, s, a, idx, loops=5, obstacles=obs)
    assert ar.shape == a.shape and 0 <= it <= 5
    v5 = float(torch.relu(-_deriv(cbf, s, ar, idx, obs)).sum())
    assert v5 <= v0
    if v0 > 0:
        assert v5 < v0
    ever = torch.zeros_like(moved)
    cur = a
    for _ in range(5):
        ever |= _touched(_deriv(cbf, s, cur, idx, obs), idx, N)
        cur, _, _ = refine_actions(cbf, s, cur, idx, loops=1, obstacles=obs)
    assert not bool(((ar != a).any(-1) & ~ever).any())


def test_obstacles_are_seen_by_knn_and_safety_count():
    N = 10
    s, _, obs = E.generate_scenarios(1, N, 2, 1, seed=2)
    s = s.clone()
    s[0, 0, :2] = obs[0, 0] + torch.tensor([0.5 * C.DIST_MIN_CHECK, 0.0])
    s[0, 0, 2:] = 0.0
    # the moved agent stays clear of every other agent, so only the obstacle can flag it
    d = torch.linalg.vector_norm(s[0, 1:, :2] - s[0, 0, :2], dim=-1)
    assert float(d.min()) > C.DIST_MIN_CHECK
    free = _safe_count(s)
    seen = _safe_count(s, obs)
    assert float(free[0]) - float(seen[0]) == 1.0
    idx = _knn(s, min(C.TOP_K, N), obs)
    assert bool((idx[0, 0] >= N).any())
    assert int(_knn(s, min(C.TOP_K, N)).max()) < N


def _cli(*args):
    return subprocess.run([sys.executable, "evaluate.py", *args], cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_cli_3d_obstacles():
    r = _cli("--num_agents", "8", "--dim", "3", "--num_obstacles", "1", "--episodes", "1", "--max_steps", "3",
             "--refine_loops", "2", "--device", "cpu")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["dim"] == 3 and out["num_obstacles"] == 1 and out["refine_impl"] == "autograd" and out["dtype"] == "fp32"


def test_cli_checkpoint_dimension_mismatch(tmp_path):
    ck = tmp_path / "ck2d.pt"
    torch.manual_seed(2)
    torch.save({"controller": Controller(4).state_dict(), "cbf": CBF(4).state_dict()}, ck)
    r = _cli("--num_agents", "8", "--dim", "3", "--model_path", str(ck), "--episodes", "1", "--max_steps", "2",
             "--device", "cpu")
    assert r.returncode != 0
    assert "2-D networks" in r.stderr and "--dim" in r.stderr


def test_cli_native_filter_needs_hip():
    r = _cli("--num_agents", "8", "--refine_impl", "native", "--episodes", "1", "--max_steps", "2", "--device", "cpu")
    assert r.returncode != 0
    assert "HIP" in r.stderr and "native" in r.stderr


def test_rollout_native_filter_on_cpu_raises():
    with pytest.raises(ValueError, match="HIP"):
        evaluate(Controller(4), CBF(4), EvalConfig(num_agents=6, episodes=1, max_steps=2, refine_impl="native"))


# ---- 2-D regression: the evaluation arithmetic as it stood before the D-aware rewrite ----------
def _old_refine_actions(cbf, s, a, idx, loops, lr, check_every=10):
    with torch.no_grad():
        h = cbf(s, idx=idx)
    delta = torch.zeros_like(a, requires_grad=True)
    viol = torch.zeros((), device=s.device)
    used = torch.zeros((), dtype=torch.int64, device=s.device)
    for it in range(1, loops + 1):
        ar = a + delta
        s_next = s + torch.cat([s[..., 2:], ar], -1) * C.TIME_STEP
        hn = cbf(s_next, idx=idx)
        deriv = hn - h + C.TIME_STEP * C.ALPHA_CBF * h
        viol = torch.relu(-deriv).sum()
        pending = viol.detach() > 0
        used += pending.long()
        if it % check_every == 0 and not bool(pending):
            break
        g, = torch.autograd.grad(viol, delta)
        with torch.no_grad():
            delta -= lr * g
    return (a + delta).detach(), int(used), float(viol.detach())


def _old_evaluate(controller, cbf, cfg):
    controller.eval()
    cbf.eval()
    agg = {}
    for ep in range(cfg.episodes):
        s0, g = E.generate_batch(cfg.num_envs, cfg.num_agents, C.DIST_MIN_THRES, seed=cfg.seed * 7919 + ep)
        s = s0
        B, N, _ = s.shape
        k = min(cfg.top_k, N)
        safe_sum, steps, refine_iters = 0.0, 0, 0
        active = torch.ones(B, dtype=torch.bool)
        for t in range(cfg.max_steps):
            idx = O.knn_idx(s, k)
            with torch.no_grad():
                a = controller(s, g, idx=idx)
            a, it, _ = _old_refine_actions(cbf, s, a, idx, cfg.refine_loops, cfg.refine_lr)
            refine_iters += it
            with torch.no_grad():
                s = s + torch.cat([s[..., 2:], a], -1) * C.TIME_STEP
                safe = O.safe_agent_count(s).float()
                safe_sum += float((safe * active.float()).sum())
                steps += int(active.sum()) * N
                dist = torch.linalg.vector_norm(s[..., :2] - g, dim=-1).mean(-1)
                active = active & (dist >= C.DIST_MIN_CHECK)
            if cfg.early_stop and not bool(active.any()):
                break
        with torch.no_grad():
            d = torch.linalg.vector_norm(s[..., :2] - g, dim=-1)
            reach = float((d < C.DIST_MIN_CHECK).float().mean())
            mean_dist = float(d.mean())
        r = {"safety_rate": safe_sum / max(steps, 1), "reaching_rate": reach, "mean_goal_dist": mean_dist,
             "steps": t + 1, "agent_steps": steps, "refine_iters": refine_iters}
        for kk, v in r.items():
            agg[kk] = agg.get(kk, 0.0) + float(v)
    return {kk: v / cfg.episodes for kk, v in agg.items()}


@pytest.mark.parametrize("seed", [0, 1])
def test_2d_obstacle_free_path_is_bit_identical(seed):
    torch.manual_seed(seed)
    ctrl, cbf = Controller(4), CBF(4)
    cfg = EvalConfig(num_agents=10, num_envs=2, episodes=2, max_steps=5, refine_loops=3, seed=seed)
    assert (cfg.dim, cfg.num_obstacles, cfg.refine_impl, cfg.dtype) == (2, 0, "autograd", "fp32")
    new = evaluate(ctrl, cbf, cfg)
    old = _old_evaluate(ctrl, cbf, cfg)
    assert new == old, (new, old)


def test_safety_filter_objects_have_no_mfma_hazard():
    """scripts/check_mfma_exec.py over the safety filter's objects (all three precisions)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_mfma_exec as c
    objs = sorted(glob.glob(os.path.join(ROOT, "build", "csrc", "refine*.o")))
    if not objs:
        pytest.skip("extension not built (python csrc/build.py)")
    assert c.main(objs) == 0
