"""Validation during training on the HIP device (macbf_gnn_amd/validate.py): it leaves the training
trajectory bit-identical on every engine path, its integer counts equal a loop written here from
the public ops (the filter on the active sub-batch instead of the per-env mask), it is repeatable,
and an fp16 run validates in bf16 and gets its modules back as they were."""
import io
import json

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd.ops import graph
from macbf_gnn_amd.ops.refine import safety_filter
from macbf_gnn_amd.validate import COUNTS, DIST_FX, val_dtype

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T = 10
LOOPS = 4

CASES = {
    "n32_bf16": dict(num_agents=32, dtype="bf16"),                     # persistent rollout + backward graph
    "n32_fp32": dict(num_agents=32, dtype="fp32"),
    "n96_3d_obs": dict(num_agents=96, dim=3, num_obstacles=1),         # 108 nodes: the per-step driver
    "n32_fp16": dict(num_agents=32, dtype="fp16"),                     # loss scaling; validation in bf16
}


def _trainer(case, **kw):
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    cfg = C.TrainConfig(num_envs=2, inner_loops=T, seed=3, device="hip", display_steps=1, val_envs=2,
                        val_refine_loops=LOOPS, **CASES[case], **kw)
    tr = Trainer(cfg, device=DEV, dp=DP(device=DEV))
    tr.logger.stream = io.StringIO()
    return tr


def _records(tr):
    return [json.loads(l) for l in tr.logger.stream.getvalue().splitlines()]


@pytest.mark.parametrize("case", list(CASES))
def test_training_is_bit_identical_with_validation(case):
    ref, tr = _trainer(case), _trainer(case, val_every=2)
    ref.fit(4)
    tr.fit(4)
    torch.cuda.synchronize()
    assert ref.validator is None and tr.validator is not None
    assert torch.equal(tr.fp.flat, ref.fp.flat)
    assert torch.equal(tr.opt.exp_avg, ref.opt.exp_avg) and torch.equal(tr.opt.exp_avg_sq, ref.opt.exp_avg_sq)
    assert tr.opt.steps == ref.opt.steps and tr.skipped_steps == ref.skipped_steps
    recs, ref_recs = _records(tr), _records(ref)
    vals = [r for r in recs if "val_safety_rate" in r]
    train = [r for r in recs if "loss_total" in r]
    assert [v["step"] for v in vals] == [2, 4] and len(train) == len(ref_recs) == 4
    for r, q in zip(train, ref_recs):
        r.pop("agent_steps_per_s"), q.pop("agent_steps_per_s")
        assert r == q
    for v in vals:
        assert 0.0 <= v["val_safety_rate"] <= 1.0 and 0.0 <= v["val_refined_safety_rate"] <= 1.0
        assert 0.0 < v["val_mean_T"] <= T and 0.0 < v["val_refined_mean_T"] <= T and v["val_ms"] > 0.0
    for m in (tr.controller, tr.cbf):
        assert "mfma_dtype" not in m.__dict__ and m.training
    if case == "n32_fp16":
        assert tr.fp16 and val_dtype(tr.cfg) == torch.bfloat16
        assert torch.equal(tr.gscale_dev, ref.gscale_dev) and torch.equal(tr._good_dev, ref._good_dev)


def _loop(tr, refine):
    """The validation rollout from the public ops, one host decision per step: kNN, the modules, the
    unmasked filter on the active sub-batch scattered back, the safety count."""
    v = tr.validator
    s, g, obs = v.s0, v.g, v.obs
    B, N, _ = s.shape
    D = s.shape[-1] // 2
    c = dict.fromkeys(COUNTS, 0)
    active = torch.ones(B, dtype=torch.bool, device=DEV)
    with torch.no_grad():
        for _ in range(T):
            if not bool(active.any()):
                break
            idx = graph.knn(s, min(tr.cfg.top_k, N), obs).long()
            a = tr.controller(s, g, idx=idx, obstacles=obs)
            if refine:
                ar, used, _ = safety_filter(tr.cbf, s[active], a[active], idx[active],
                                            obstacles=None if obs is None else obs[active], loops=LOOPS)
                a = a.clone()
                a[active] = ar
                c["refine_iters"] += int(used)
            s = s + torch.cat([s[..., D:], a], -1) * C.TIME_STEP
            c["safe_agent_steps"] += int((graph.safe_agent_count(s, obs).long() * active.long()).sum())
            c["env_steps"] += int(active.sum())
            c["steps"] += 1
            active = active & (torch.linalg.vector_norm(s[..., :D] - g, dim=-1).mean(-1) >= C.DIST_MIN_CHECK)
        d = torch.linalg.vector_norm(s[..., :D] - g, dim=-1)
        c["reached_agents"] = int((d < C.DIST_MIN_CHECK).sum())
        c["goal_dist_fx"] = int((d.double().sum() * DIST_FX).round())
    c["agent_steps"] = c["env_steps"] * N
    c["agents"] = B * N
    return c


@pytest.mark.parametrize("case", ["n32_fp32", "n96_3d_obs", "n32_fp16"])
def test_counts_equal_a_loop_from_the_public_ops(case):
    """Env 0's goals are moved onto its starts, so its episode is over after the first step and the
    filter runs with a masked-out env from then on; env 1 runs the whole horizon."""
    tr = _trainer(case, val_every=2)
    tr.fit(1)                                       # one real update: not the initial weights
    first = tr.validate()
    v = tr.validator
    D = tr.cfg.dim
    v.g[0] = v.s0[0, :, :D]
    a, b = tr.validate(), tr.validate()
    counts = v.last_counts
    a.pop("val_ms"), b.pop("val_ms"), first.pop("val_ms")
    assert a == b and a != first                    # repeatable; and the scenes are what it runs on
    for m in (tr.controller, tr.cbf):
        m.mfma_dtype = val_dtype(tr.cfg)
        m.eval()
    for name, refine in (("nominal", False), ("refined", True)):
        want = _loop(tr, refine)
        assert counts[name] == want, (name, counts[name], want)
        assert T < want["env_steps"] < 2 * T        # env 0 finished early, env 1 did not
    assert counts["refined"]["refine_iters"] > 0    # the filter had work on the live env
    N = tr.cfg.num_agents
    assert a["val_safety_rate"] == counts["nominal"]["safe_agent_steps"] / counts["nominal"]["agent_steps"]
    assert a["val_refined_reaching_rate"] == counts["refined"]["reached_agents"] / (2 * N)
    assert a["val_refined_mean_T"] == counts["refined"]["env_steps"] / 2


def test_rollout_synchronises_for_the_done_flag_only(monkeypatch):
    """With the period of the "all done" read beyond the horizon a rollout, filter and mask
    included, never waits for the GPU: the flag is the only host read, every CHECK_EVERY steps."""
    from macbf_gnn_amd import validate as V
    assert V.CHECK_EVERY >= 5
    tr = _trainer("n32_fp32", val_every=2)
    tr.validate()                                   # scenes, packing tables
    v = tr.validator
    for m in (tr.controller, tr.cbf):
        m.eval()
    monkeypatch.setattr(V, "CHECK_EVERY", T + 1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        vec = v.rollout(tr.controller, tr.cbf, refine=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert vec.is_cuda and vec.numel() == len(COUNTS)
    want = tr.validator.last_counts["refined"]
    assert dict(zip(COUNTS, vec.tolist())) == want  # and the same totals as with the reads
