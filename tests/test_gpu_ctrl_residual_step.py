"""One full training step (rollout, losses, BPTT backward) of the HIP engine with the residual head
(``TrainConfig.ctrl_residual``; macbf_gnn_amd/oracle.py, "Residual head") against autograd through the
oracle engine, as tests/test_gpu_fp32.py test_full_step_grad_fp32 does for the plain controller: the same
shape of config, every parameter tensor <= 1e-3 relative norm, the loss within that test's bound. The
residual rows are drawn before the step (tests/ctrl_residual_cases.py randomise_trainer), so the residual
acts in the rollout; their gradient is a tensor of its own in the comparison.

Shapes: 32 agents x 2 (persistent rollout, per-T backward graph), 13 x 3 (forced trajectory, as that
test does below 32 agents), 256, 40 in 3-D with two obstacles, 32 under a_max = 0.25, 32 without BPTT (the
batched backward). bf16 and fp16: one finite step each; the fp16 loss scale stays on a finite step."""
import pytest
import torch

from macbf_gnn_amd import config as C

import ctrl_residual_cases as RC
from test_gpu_fp32 import _rel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
W4, B4 = "controller_dec_net.6.weight", "controller_dec_net.6.bias"


def _trainer(dtype="fp32", **kw):
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    cfg = C.TrainConfig(num_agents=kw.pop("N", 32), num_envs=kw.pop("B", 2), inner_loops=kw.pop("T", 5),
                        early_stop=False, seed=0, device="hip", dtype=dtype, ctrl_residual=True, **kw)
    tr = Trainer(cfg, device=DEV, dp=DP(device=DEV))
    assert tr.controller.residual and tr.engine.pw.residual
    RC.randomise_trainer(tr)
    return tr


SHAPES = [("n32", dict(N=32, B=2), False), ("n13-forced", dict(N=13, B=3), True), ("n256", dict(N=256), False),
          ("n40-3d-obs", dict(N=40, dim=3, num_obstacles=2), False), ("n32-limit", dict(N=32, a_max=0.25), False),
          ("n32-nobptt", dict(N=32, bptt=False), False)]


@pytest.mark.parametrize("name,kw,forced", SHAPES, ids=[s[0] for s in SHAPES])
def test_full_step_grad_fp32(name, kw, forced):
    from macbf_gnn_amd.engine.oracle_engine import OracleEngine
    tr = _trainer(**dict(kw))
    D = tr.cfg.dim
    s0, g, obs = tr.sample()
    stats = tr.engine.step(s0, g, obs)
    g_hip = tr.fp.grad.clone()
    T = int(float(stats["T"]))
    if "a_max" in kw:                                  # some, not all, agent-steps saturate
        lim, tot = (float(x) for x in tr.engine.limited_counts())
        assert 0 < lim < tot, (lim, tot)

    def compare(force):
        stats_o = OracleEngine(tr).step(s0, g, obs, forced=tr.engine.trajectory(T) if force else None)
        g_ref = tr.fp.grad.clone()
        worst = [(_rel(g_hip[o:o + n], g_ref[o:o + n]), pn) for m, pn, shape, o, n in tr.fp.specs]
        for m, pn, shape, o, n in tr.fp.specs:         # the residual rows as tensors of their own
            if pn in (W4, B4):
                cols = n // (3 * D)
                a, b = g_hip[o + 2 * D * cols:o + n], g_ref[o + 2 * D * cols:o + n]
                assert float(b.norm()) > 0 and float(a.norm()) > 0, (pn, "residual rows without a gradient")
                worst.append((_rel(a, b), pn + "[res]"))
        worst.sort(reverse=True)
        return worst, stats_o

    worst, stats_o = compare(forced)
    print(f"STEP {name}: worst {worst[:3]}")
    if worst[0][0] > 1e-3 and not forced:
        # a max-pool near-tie (two neighbours' features within the x3 rounding) routes a feature's gradient
        # to another edge: replay the engine's trajectory, graphs and argmax slots, as below 32 agents
        worst, stats_o = compare(True)
        print(f"STEP {name} (forced trajectory): worst {worst[:3]}")
    assert worst[0][0] <= 1e-3, worst[:4]
    assert abs(float(stats["loss_total"]) - stats_o["loss_total"]) <= 1e-4 * abs(stats_o["loss_total"]) + 1e-6


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16bit_step_is_finite(dtype):
    tr = _trainer(dtype=dtype, N=32, B=2)
    scale = tr.grad_scale if dtype == "fp16" else None
    before = tr.fp.flat.clone()
    st = tr.train_step()
    torch.cuda.synchronize()
    assert not st.get("skipped")
    assert bool(torch.isfinite(tr.fp.grad).all()) and bool(torch.isfinite(tr.fp.flat).all())
    assert not torch.equal(before, tr.fp.flat)
    o, n = {pn: (o, n) for m, pn, shape, o, n in tr.fp.specs}[W4]
    assert float(tr.fp.grad[o + 4 * 64:o + n].abs().max()) > 0
    if dtype == "fp16":
        assert tr.fp16 and tr.grad_scale == scale
