"""Validation during training on CPU (macbf_gnn_amd/validate.py, Trainer.validate / fit, train.py):
off by default, the val records of fit, no effect on the training trajectory, the counts against
evaluate.rollout_eval, the DP reduction over gloo, the best checkpoint and its resume, the CLI,
and the throughput window of the logger."""
import io
import json
import os
import socket
import subprocess
import sys
import time
import types

import pytest
import torch
import torch.multiprocessing as mp

from macbf_gnn_amd import config as C
from macbf_gnn_amd import validate as V
from macbf_gnn_amd.evaluate import EvalConfig, rollout_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
KEYS = {"val_safety_rate", "val_reaching_rate", "val_mean_goal_dist", "val_mean_T", "val_refined_safety_rate",
        "val_refined_reaching_rate", "val_refined_mean_T", "val_refine_iters", "val_ms"}


def _cfg(**kw):
    base = dict(num_agents=8, num_envs=1, inner_loops=4, device="cpu", seed=5, train_steps=4, display_steps=1,
                val_envs=2, val_refine_loops=2)
    base.update(kw)
    return C.TrainConfig(**base)


def _trainer(**kw):
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    return Trainer(_cfg(**kw), device=CPU, dp=DP(device=CPU))


def _fit(tr, steps=None):
    buf = io.StringIO()
    tr.logger.stream = buf            # the training records and the val lines go to one stream
    tr.fit(steps)
    return [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith("{")]


def _val(recs):
    return [r for r in recs if "val_safety_rate" in r]


def test_off_by_default_builds_nothing():
    tr = _trainer(train_steps=2)
    recs = _fit(tr)
    assert len(recs) == 2 and not _val(recs)
    assert tr.validator is None
    assert not any(k.startswith("val_") for r in recs for k in r)


def test_fit_emits_val_records_and_leaves_training_alone(tmp_path):
    log = tmp_path / "log.jsonl"
    ref = _trainer()
    ref_recs = _fit(ref)
    tr = _trainer(val_every=2, log_path=str(log))
    recs = _fit(tr)
    vals = _val(recs)
    assert [r["step"] for r in vals] == [2, 4]
    for r in vals:
        assert set(r) == KEYS | {"step"}
        for k in V.RATE_KEYS:
            assert 0.0 <= r[k] <= 1.0
        assert 0.0 < r["val_mean_T"] <= 4 and 0.0 < r["val_refined_mean_T"] <= 4 and r["val_ms"] > 0.0
    assert torch.equal(tr.fp.flat, ref.fp.flat)
    for g in ("controller", "cbf"):
        a, b = tr.opt.torch_state_dict(g), ref.opt.torch_state_dict(g)
        for k in a["state"]:
            for name, v in a["state"][k].items():
                w = b["state"][k][name]
                assert torch.equal(torch.as_tensor(v), torch.as_tensor(w)), (g, k, name)
    train = [r for r in recs if "loss_total" in r]
    assert len(train) == len(ref_recs) == 4
    for r, q in zip(train, ref_recs):
        assert {k: v for k, v in r.items() if k != "agent_steps_per_s"} == \
               {k: v for k, v in q.items() if k != "agent_steps_per_s"}
    logged = [json.loads(l) for l in log.read_text().splitlines()]
    assert _val(logged) == vals and len(logged) == 6
    # modules are left as found
    assert tr.controller.training and tr.cbf.training
    assert "mfma_dtype" not in tr.controller.__dict__ and "mfma_dtype" not in tr.cbf.__dict__


def test_validate_is_repeatable_and_public():
    tr = _trainer(val_every=2)
    g0 = torch.random.get_rng_state()
    a = tr.validate()
    b = tr.validate()
    assert torch.equal(g0, torch.random.get_rng_state())          # no torch global RNG
    a.pop("val_ms"), b.pop("val_ms")
    assert a == b and set(a) == KEYS - {"val_ms"}
    nr = _trainer(val_every=2, val_refine=False).validate()
    assert set(nr) == {"val_safety_rate", "val_reaching_rate", "val_mean_goal_dist", "val_mean_T", "val_ms"}
    for k in ("val_safety_rate", "val_reaching_rate", "val_mean_goal_dist", "val_mean_T"):
        assert nr[k] == a[k]


@pytest.mark.parametrize("dim,nobs", [(2, 0), (3, 1)])
def test_counts_equal_rollout_eval_while_no_env_finishes(dim, nobs):
    """3 steps: no env reaches its goal, so every env is refined at every step and the one
    difference from rollout_eval (done envs are not refined) cannot show."""
    T = 3
    tr = _trainer(val_every=1, inner_loops=T, dim=dim, num_obstacles=nobs, val_refine_loops=3)
    out = tr.validate()
    v = tr.validator
    N, B = 8, 2
    for name, refine in (("nominal", False), ("refined", True)):
        ec = EvalConfig(num_agents=N, num_envs=B, max_steps=T, refine=refine, refine_loops=3, top_k=tr.cfg.top_k,
                        dim=dim, num_obstacles=nobs)
        tr.controller.eval(), tr.cbf.eval()
        r = rollout_eval(tr.controller, tr.cbf, v.s0, v.g, ec, obstacles=v.obs)
        tr.controller.train(), tr.cbf.train()
        c = v.last_counts[name]
        assert r["agent_steps"] == B * N * T == c["agent_steps"]              # nobody finished
        assert c["env_steps"] == B * T and c["steps"] == T and c["agents"] == B * N
        assert c["safe_agent_steps"] == round(r["safety_rate"] * r["agent_steps"])
        assert c["reached_agents"] == round(r["reaching_rate"] * B * N)
        assert c["refine_iters"] == r["refine_iters"]
        assert abs(c["goal_dist_fx"] / V.DIST_FX / (B * N) - r["mean_goal_dist"]) < 1e-5
    assert out["val_safety_rate"] == v.last_counts["nominal"]["safe_agent_steps"] / (B * N * T)
    assert v.last_counts["nominal"]["refine_iters"] == 0


def test_result_does_not_depend_on_the_read_period(monkeypatch):
    """Steps that run after every env is done add nothing: reading the flag every step or never
    (within the episode) gives the same totals. With the goals moved onto the starts every env is
    done after its first step, and steps 2.. of the longer periods are such steps."""
    tr = _trainer(val_every=1, inner_loops=7)
    tr.validate()
    v = tr.validator
    v.g = v.s0[..., :2].clone()
    res = []
    for period in (1, 5, 100):
        monkeypatch.setattr(V, "CHECK_EVERY", period)
        tr.validate()
        res.append(v.last_counts)
    assert res[0] == res[1] == res[2]
    for name in ("nominal", "refined"):
        assert res[0][name]["env_steps"] == 2 and res[0][name]["steps"] == 1
        assert res[0][name]["reached_agents"] == res[0][name]["agents"] == 16


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, outdir):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                       "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank)})
    torch.set_num_threads(1)
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    dp = DP(device=CPU)
    tr = Trainer(_cfg(val_every=1), device=CPU, dp=dp)
    out = tr.validate()
    with open(os.path.join(outdir, f"val{rank}.json"), "w") as f:
        json.dump({"out": out, "counts": tr.validator.last_counts}, f)
    dp.shutdown()


@pytest.mark.timeout(600)
def test_dp_ranks_agree_and_equal_the_weighted_combination(tmp_path):
    mp.start_processes(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    r0, r1 = (json.loads((tmp_path / f"val{r}.json").read_text()) for r in range(2))
    r0["out"].pop("val_ms"), r1["out"].pop("val_ms")
    assert r0 == r1
    # each rank's scenes alone, in one process: the networks are the same (same seed, broadcast)
    tr = _trainer(val_every=1)
    per_rank = []
    for rank in range(2):
        v = V.Validator(tr.cfg, CPU, types.SimpleNamespace(rank=rank, enabled=False))
        v.validate(tr.controller, tr.cbf)
        per_rank.append(v.last_counts)
    assert per_rank[0] != per_rank[1]                               # different scenes per rank
    tot = {name: {k: per_rank[0][name][k] + per_rank[1][name][k] for k in V.COUNTS} for name in ("nominal", "refined")}
    assert tot == r0["counts"]
    assert V.metrics_from_counts(tot["nominal"], tot["refined"], 8) == r0["out"]
    n = tot["nominal"]
    assert r0["out"]["val_safety_rate"] == n["safe_agent_steps"] / n["agent_steps"]
    assert r0["out"]["val_reaching_rate"] == n["reached_agents"] / (2 * 2 * 8)
    assert r0["out"]["val_mean_T"] == n["env_steps"] / 4


def test_save_best_strict_improvement_sidecar_and_resume(tmp_path, monkeypatch):
    from macbf_gnn_amd.models import CBF, Controller
    from macbf_gnn_amd.utils import ckpt
    path = str(tmp_path / "m.pt")
    best, side = path + ".best", path + ".best.json"
    values = iter([0.5, 0.5, 0.7, 0.6])
    tr = _trainer(val_every=1, save_best=True, model_path=path, save_steps=100)
    real = tr.validate

    def fake():
        out = real()
        out["val_refined_safety_rate"] = next(values)
        return out
    monkeypatch.setattr(tr, "validate", fake)
    _fit(tr, 1)
    assert json.loads(open(side).read()) == {"step": 1, "metric": "val_refined_safety_rate", "value": 0.5}
    first = torch.load(best, weights_only=True)
    assert first["step"] == 1 and first["format"] == ckpt.FORMAT
    _fit(tr, 1)                                                  # equal: not strict, kept
    assert json.loads(open(side).read())["step"] == 1
    assert torch.load(best, weights_only=True)["step"] == 1
    _fit(tr, 1)                                                  # 0.7: replaced
    assert json.loads(open(side).read()) == {"step": 3, "metric": "val_refined_safety_rate", "value": 0.7}
    at3 = {k: v.detach().clone() for m in (tr.controller, tr.cbf) for k, v in m.state_dict().items()}
    _fit(tr, 1)                                                  # 0.6: kept
    assert json.loads(open(side).read())["step"] == 3
    ctrl, cbf = Controller(4), CBF(4)
    ckpt.load_models(best, ctrl, cbf)
    loaded = {k: v for m in (ctrl, cbf) for k, v in m.state_dict().items()}
    assert loaded.keys() == at3.keys() and all(torch.equal(loaded[k], at3[k]) for k in at3)   # step 3's networks
    assert not all(torch.equal(v, at3[k]) for m in (tr.controller, tr.cbf) for k, v in m.state_dict().items())
    # resume: model_path holds step 4; the sidecar's 0.7 stands against a worse 0.65, a better 0.8 replaces it
    tr2 = _trainer(val_every=1, save_best=True, model_path=path, save_steps=100, train_steps=6)
    assert tr2.step_count == 4
    values2 = iter([0.65, 0.8])
    real2 = tr2.validate

    def fake2():
        out = real2()
        out["val_refined_safety_rate"] = next(values2)
        return out
    monkeypatch.setattr(tr2, "validate", fake2)
    _fit(tr2, 1)
    assert json.loads(open(side).read()) == {"step": 3, "metric": "val_refined_safety_rate", "value": 0.7}
    _fit(tr2, 1)
    assert json.loads(open(side).read()) == {"step": 6, "metric": "val_refined_safety_rate", "value": 0.8}
    assert torch.load(best, weights_only=True)["step"] == 6


def test_best_metric_choice_and_config_errors(tmp_path):
    assert V.default_best_metric(_cfg()) == "val_refined_safety_rate"
    assert V.default_best_metric(_cfg(val_refine=False)) == "val_safety_rate"
    assert V.default_best_metric(_cfg(best_metric="val_reaching_rate")) == "val_reaching_rate"
    for bad in (dict(val_every=1, best_metric="val_mean_T"),
                dict(val_every=1, val_refine=False, best_metric="val_refined_safety_rate"),
                dict(val_every=1, save_best=True),
                dict(val_every=0, save_best=True, model_path=str(tmp_path / "x.pt"))):
        with pytest.raises(ValueError):
            _trainer(**bad)


def test_cli_writes_val_lines(tmp_path):
    log = tmp_path / "log.jsonl"
    r = subprocess.run([sys.executable, "train.py", "--num_agents", "8", "--train_steps", "4", "--inner_loops", "4",
                        "--display_steps", "2", "--device", "cpu", "--val_every", "2", "--val_envs", "2",
                        "--val_refine_loops", "2", "--log_path", str(log)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(l) for l in log.read_text().splitlines()]
    vals = _val(recs)
    assert [v["step"] for v in vals] == [2, 4]
    assert all(set(v) == KEYS | {"step"} for v in vals)
    assert len(recs) == 4
    r = subprocess.run([sys.executable, "train.py", "--num_agents", "8", "--train_steps", "2", "--inner_loops", "4",
                        "--device", "cpu", "--val_every", "2", "--val_envs", "2", "--no_val_refine",
                        "--best_metric", "val_reaching_rate", "--save_best", "--model_path", str(tmp_path / "m.pt"),
                        "--log_path", str(log)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    side = json.loads((tmp_path / "m.pt.best.json").read_text())
    assert side["metric"] == "val_reaching_rate" and side["step"] == 2
    last = json.loads(log.read_text().splitlines()[-1])
    assert "val_refined_safety_rate" not in last and last["val_reaching_rate"] == side["value"]


def test_throughput_excludes_validation_time(monkeypatch):
    """A clock that advances 1 s per reading, and a validation that takes 1000 s of it: the
    agent-steps/s of the record that follows is that of the training iterations alone."""
    now = [0.0]

    def clock():
        now[0] += 1.0
        return now[0]
    monkeypatch.setattr(time, "perf_counter", clock)
    tr = _trainer(val_every=1, display_steps=2, phase_timing=False)
    real = tr.validate

    def slow():
        now[0] += 1000.0
        return real()
    monkeypatch.setattr(tr, "validate", slow)
    recs = _fit(tr, 4)
    train = [r for r in recs if "agent_steps_per_s" in r]
    assert len(train) == 2 and len(_val(recs)) == 4
    for r in train:
        # at most 2 iterations x 4 steps x 8 agents in a window: under 0.064 / s with a validation's
        # 1000 s in it, and at least 16 agent-steps over the few dozen clock readings without
        assert r["agent_steps_per_s"] > 2 * 64 / 1000.0, r
