"""Training under an actuator limit (macbf_gnn_amd/oracle.py, "Actuator limit"), CPU side: the oracle's
clamp and its gradient, the off paths, the replayed saturation decisions, the oracle engine behind
``train.py --a_max``, and the share condition of the GPU cases (tests/train_limit_cases.py).
Reference ops: the rollout /root/reference/train.py:58-81, differentiated by train.py:103."""
import json
import math

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import oracle as O

import train_limit_cases as TL


def _scene(N=8, B=2, T=4, a_max=0.0, dtype=torch.float64, **kw):
    from macbf_gnn_amd.engine import Trainer
    cfg = C.TrainConfig(num_agents=N, num_envs=B, inner_loops=T, early_stop=False, device="cpu", seed=0, a_max=a_max, **kw)
    tr = Trainer(cfg)
    s0, g, obs = tr.sample()
    cp = {k: v.detach().to(dtype).clone() for k, v in tr.controller.params_dict().items()}
    bp = {k: v.detach().to(dtype).clone() for k, v in tr.cbf.params_dict().items()}
    return tr, s0.to(dtype), g.to(dtype), cp, bp


def _loss(cp, bp, s0, g, T, a_max, forced=None):
    traj = O.rollout(cp, s0, g, inner_loops=T, early_stop=False, a_max=a_max, forced=forced)
    losses, _, _ = O.train_losses(cp, bp, traj, g)
    return losses["total"], traj


A64 = 0.3      # the float64 scene's limit: components on both sides, none within 1e-3 (asserted)


def test_oracle_gradient_matches_finite_differences():
    """float64, B = 2, N = 8, T = 4: autograd of train_losses through rollout(a_max=A) against central
    differences on the controller parameters -- along one random direction per parameter tensor and
    at the largest-gradient coordinate of each. eps = 1e-6: truncation ~1e-12 |f'''|, rounding
    ~1e-16 |f| / eps = 1e-10; bound 1e-6 relative to the tensor's gradient norm (+ 1e-9 absolute)."""
    T = 4
    _, s0, g, cp, bp = _scene(T=T)
    a_max = float(torch.tensor(A64, dtype=torch.float32))
    for v in cp.values():
        v.requires_grad_(True)
    total, traj = _loss(cp, bp, s0, g, T, A64)
    A = traj["A"].detach()
    assert float(((A.abs() - a_max).abs()).min()) > 1e-3          # no component near the kink
    assert bool((A.abs() > a_max).any()) and bool((A.abs() < a_max).any())
    grads = dict(zip(cp, torch.autograd.grad(total, list(cp.values()))))
    eps = 1e-6
    gen = torch.Generator().manual_seed(1)

    def fd(name, d):
        out = []
        for sgn in (1.0, -1.0):
            p = {k: v.detach().clone() for k, v in cp.items()}
            p[name] = p[name] + sgn * eps * d
            out.append(float(_loss(p, bp, s0, g, T, A64)[0]))
        return (out[0] - out[1]) / (2 * eps)

    for name, gr in grads.items():
        d = torch.randn(gr.shape, generator=gen, dtype=gr.dtype)
        d = d / d.norm()
        tol = 1e-6 * float(gr.norm()) + 1e-9
        assert abs(fd(name, d) - float((gr * d).sum())) <= tol, name
        e = torch.zeros_like(gr)
        e.view(-1)[gr.abs().argmax()] = 1.0
        assert abs(fd(name, e) - float(gr.abs().max() * torch.sign(gr.view(-1)[gr.abs().argmax()]))) <= tol, name
    # the mask is in that gradient: it is not the unlimited rollout's
    g_off = torch.autograd.grad(_loss(cp, bp, s0, g, T, None)[0], list(cp.values()))
    assert any(not torch.allclose(a, b, rtol=1e-3, atol=0) for a, b in zip(grads.values(), g_off))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_off_paths_are_bitwise(dtype):
    """a_max=None is the rollout as it was -- s' = s + dt [v, a] on the raw action, recomputed here
    with the same torch expression -- and a limit far away (1e30) returns the same tensors."""
    T = 4
    _, s0, g, cp, _ = _scene(T=T, dtype=dtype)
    off = O.rollout(cp, s0, g, inner_loops=T, early_stop=False)
    none = O.rollout(cp, s0, g, inner_loops=T, early_stop=False, a_max=None)
    far = O.rollout(cp, s0, g, inner_loops=T, early_stop=False, a_max=1e30)
    D = O.sdim(s0)
    for t in range(T):
        s = off["S"][:, t]
        assert torch.equal(off["S"][:, t + 1], s + torch.cat([s[..., D:], off["A"][:, t]], -1) * C.TIME_STEP)
    for k in off:
        assert torch.equal(off[k], none[k]) and torch.equal(off[k], far[k]), k


def test_forced_sat_reproduces_own_gradient():
    """forced["sat"] taken from the oracle's own run: the same values and the same gradient, exactly."""
    T = 4
    _, s0, g, cp, bp = _scene(T=T, dtype=torch.float32)
    a_max = float(torch.tensor(A64, dtype=torch.float32))
    for v in cp.values():
        v.requires_grad_(True)
    total, traj = _loss(cp, bp, s0, g, T, A64)
    g1 = torch.autograd.grad(total, list(cp.values()))
    A = traj["A"].detach()
    sat = (A > a_max).to(torch.int8) - (A < -a_max).to(torch.int8)
    assert bool((sat != 0).any()) and bool((sat == 0).any())
    forced = {"S": traj["S"].detach(), "idx": traj["idx"], "sat": sat}
    total2, traj2 = _loss(cp, bp, s0, g, T, A64, forced=forced)
    g2 = torch.autograd.grad(total2, list(cp.values()))
    assert torch.equal(traj2["S"], traj["S"]) and torch.equal(traj2["A"], traj["A"])
    assert float(total2.detach()) == float(total.detach())
    for a, b, k in zip(g1, g2, cp):
        assert torch.equal(a, b), k
    # and the decisions are what is replayed: all-zero sat is the unlimited gradient along that trajectory
    forced0 = dict(forced, sat=torch.zeros_like(sat))
    g3 = torch.autograd.grad(_loss(cp, bp, s0, g, T, A64, forced=forced0)[0], list(cp.values()))
    assert any(not torch.equal(a, b) for a, b in zip(g1, g3))


def test_train_cli_cpu_under_limit(tmp_path, capsys):
    """One ``train.py --device cpu --a_max A`` iteration at 8 agents: limited_rate in the log line, the
    limit in the saved config; the oracle engine's velocities move by at most A * dt per step."""
    import train
    log, ck = tmp_path / "log.jsonl", tmp_path / "ck.pt"
    train.main(["--num_agents", "8", "--device", "cpu", "--a_max", "0.2", "--train_steps", "1", "--display_steps", "1",
                "--inner_loops", "6", "--log_path", str(log), "--model_path", str(ck)])
    rec = json.loads(log.read_text().splitlines()[0])
    assert 0.0 <= rec["limited_rate"] <= 1.0
    a32 = float(torch.tensor(0.2, dtype=torch.float32))
    assert torch.load(ck, weights_only=True)["config"]["a_max"] == 0.2
    from macbf_gnn_amd.engine import Trainer
    tr = Trainer(C.TrainConfig(num_agents=8, num_envs=2, inner_loops=6, device="cpu", seed=0, a_max=0.2))
    assert tr.engine.a_max == a32
    tr.train_step()
    A, valid, S = tr.engine._last
    D = tr.cfg.dim
    dv = (S[:, 1:, :, D:] - S[:, :-1, :, D:]).abs()
    bound = torch.tensor(a32, dtype=torch.float32) * C.TIME_STEP
    # v' = fl(v + fl(u dt)) in fp32: per element, v' - v exceeds A dt by at most one ulp of the larger of the two
    ulp = torch.finfo(torch.float32).eps * torch.maximum(S[:, 1:, :, D:].abs(), S[:, :-1, :, D:].abs())
    assert bool((dv <= bound + ulp).all())
    assert bool((A.abs() > a32).any())                 # and the limit did bind: A stays raw
    r = tr.limited_rate()
    assert r == float(((A.abs() > a32).any(-1) & valid[..., None]).sum()) / float(valid.sum() * 8) and 0 < r < 1
    # without the option: no key, no limit
    off = Trainer(C.TrainConfig(num_agents=8, num_envs=1, inner_loops=3, device="cpu", seed=0))
    assert off.engine.a_max is None and off.limited_rate() is None


@pytest.mark.parametrize("bad", ["-1", "inf", "nan"])
def test_train_cli_rejects_bad_limit(bad):
    import train
    with pytest.raises(ValueError, match="a_max"):
        train.main(["--num_agents", "8", "--device", "cpu", "--a_max", bad, "--train_steps", "0"])


@pytest.mark.parametrize("name", sorted(TL.CASES))
def test_share_condition(name):
    """The GPU cases' limits bind, but not everywhere: the float32 oracle's own rollout of each scene
    under its limit has between 10 % and 90 % of its valid action components saturated -- the share
    recorded in the table."""
    from macbf_gnn_amd.engine import Trainer
    _, a_max, share = TL.CASES[name]
    tr = Trainer(TL.config(name, "cpu"))
    s0, g, obs = tr.sample()
    tr.engine.step(s0, g, obs)
    A, valid, _ = tr.engine._last
    got = TL.saturated_share(A, valid, tr.engine.a_max)
    assert TL.SHARE_BAND[0] <= got <= TL.SHARE_BAND[1]
    assert math.isclose(got, share, abs_tol=2e-3), got


def test_forced_sat_nan_marker():
    """sat = 2 (a NaN action in the replayed engine): applied as it is, with no gradient -- what
    torch.clamp does with a NaN; the other components are untouched."""
    a = torch.tensor([0.1, 0.5, -0.5, 0.3], requires_grad=True)
    st = torch.tensor([0, 1, -1, 2], dtype=torch.int8)
    u = torch.where(st == 0, a, torch.where(st == 2, a.detach(), st.to(a.dtype) * 0.25))
    u.sum().backward()
    assert u.tolist() == [0.10000000149011612, 0.25, -0.25, 0.30000001192092896]
    assert a.grad.tolist() == [1.0, 0.0, 0.0, 0.0]
    # through the rollout: a trajectory whose sat marks every component NaN has no gradient through the Euler step
    T = 2
    _, s0, g, cp, bp = _scene(T=T, dtype=torch.float32)
    for v in cp.values():
        v.requires_grad_(True)
    traj = O.rollout(cp, s0, g, inner_loops=T, early_stop=False, a_max=A64)
    forced = {"S": traj["S"].detach(), "idx": traj["idx"], "sat": torch.full(traj["A"].shape, 2, dtype=torch.int8)}
    out = O.rollout(cp, s0, g, inner_loops=T, early_stop=False, a_max=A64, forced=forced)
    gr = torch.autograd.grad(out["S"][:, 1:, :, 2:].sum(), list(cp.values()), allow_unused=True)
    assert all(x is None or not bool(x.any()) for x in gr)
