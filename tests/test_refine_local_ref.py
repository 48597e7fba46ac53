"""The decentralised safety filter's Python reference (``evaluate.refine_actions(coupling="local")``,
the rule of ``evaluate.py``'s module docstring) on the host: it is exactly local, it is the joint filter
where no agent lists another agent, an agent without neighbours never moves, and the actuator limit is
the step-then-projection chain."""
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.evaluate import _cbf_local, _euler, refine_actions
from refine_local_cases import (first_iteration, host_inputs, perturbed_action, planted_obstacle_graph,
                                unaffected_rows)

LR = C.REFINE_LEARNING_RATE


def _delta(cbf, s, a, idx, obs, coupling, loops=6, **kw):
    return refine_actions(cbf, s, a, idx, loops, LR, obstacles=obs, return_delta=True, coupling=coupling, **kw)[3]


def test_local_filter_is_exactly_local():
    """Changing agent 19's action leaves delta bit-identical on every agent that neither is 19 nor lists
    it; the joint filter does move such a row (the in-edge term and the neighbours' deltas couple them)."""
    cbf, s, a, idx, obs = host_inputs("2d_obs1_n70")
    a2 = perturbed_action(a)
    keep = unaffected_rows(idx)
    assert 0 < int(keep[0].sum()) < keep.shape[1] - 1            # some rows list agent 19, some do not
    d1, d2 = (_delta(cbf, s, x, idx, obs, "local") for x in (a, a2))
    assert bool((d1 != 0).any())
    assert torch.equal(d1[keep], d2[keep])
    assert not torch.equal(d1[~keep], d2[~keep])
    j1, j2 = (_delta(cbf, s, x, idx, obs, "joint") for x in (a, a2))
    moved = int(((j1 != j2).any(-1) & keep).sum())
    print(f"joint rows outside agent 19's neighbourhood that moved: {moved}")
    assert moved >= 1


def test_obstacle_only_graph_is_the_joint_filter():
    cbf, s, a, idx, obs = planted_obstacle_graph()
    N = s.shape[1]
    assert bool((idx[..., 0] == torch.arange(N)).all()) and bool((idx[..., 1:] >= N).all())
    deriv, active = first_iteration(cbf, s, a, idx, obs)
    assert int(active.sum()) > 0                                  # counts[0] > 0: the filter has work
    assert not bool(active[..., 0].any())                         # the self slot is never active
    out = {c: refine_actions(cbf, s, a, idx, 6, LR, obstacles=obs, return_delta=True, coupling=c)
           for c in ("joint", "local")}
    assert bool((out["local"][3] != 0).any())
    assert torch.equal(out["local"][3], out["joint"][3]) and torch.equal(out["local"][0], out["joint"][0])
    assert out["local"][1] == out["joint"][1] and out["local"][2] == out["joint"][2]


def test_isolated_agent_never_moves():
    """K = 1: the self slot only. Its relative state is exactly zero whatever the action."""
    cbf, s, a, idx, obs = host_inputs("2d_tail")
    N = s.shape[1]
    self_idx = torch.arange(N).view(1, N, 1).expand(s.shape[0], N, 1).contiguous()
    with torch.no_grad():                                         # a CBF whose self slot violates the condition
        import copy
        cbf = copy.deepcopy(cbf)
        p = cbf.params_dict()
        h_self = float(O.cbf_forward({k: v.detach() for k, v in p.items()}, s, self_idx)[0, 0, 0])
        cbf.cbf_net[6].bias -= abs(h_self) + 0.05
    ar, used, viol, delta = refine_actions(cbf, s, a, self_idx, 6, LR, return_delta=True, coupling="local")
    assert viol > 0.0 and used == 6                               # violated all the way, and still
    assert torch.equal(delta, torch.zeros_like(delta)) and torch.equal(ar, a)


def test_projection_is_the_hand_chained_step():
    """With a_max, `loops` iterations are: gradient of the hinge sum at a_c + delta w.r.t. the centre rows
    alone, the step, the projection onto [-a_max - a_c, a_max - a_c]; then the final clamp."""
    cbf, s, a, idx, obs = host_inputs("3d_obs2")
    a_max, loops = 0.5, 4
    ar, used, viol, delta = refine_actions(cbf, s, a, idx, loops, LR, obstacles=obs, a_max=a_max, return_delta=True,
                                           coupling="local")
    p = {k: v.detach() for k, v in cbf.params_dict().items()}
    ac = a.clamp(-a_max, a_max)
    lo, hi = -a_max - ac, a_max - ac
    with torch.no_grad():
        h = O.cbf_forward(p, s, idx, nodes=O.with_obstacles(s, obs))
        nominal = O.with_obstacles(_euler(s, ac), obs)
    d = torch.zeros_like(a)
    n_used = 0
    for _ in range(loops):
        dr = d.clone().requires_grad_(True)
        hn = _cbf_local(p, _euler(s, ac + dr), idx, nominal)
        v = torch.relu(-(hn - h + C.TIME_STEP * C.ALPHA_CBF * h)).sum()
        n_used += int(v > 0)
        g, = torch.autograd.grad(v, dr)
        d = torch.min(torch.max(d - LR * g, lo), hi)
    assert torch.equal(delta, d) and used == n_used
    assert torch.equal(ar, (ac + d).clamp(-a_max, a_max))
    assert float(ar.abs().max()) <= a_max and bool((delta != 0).any())
    assert bool(((ac + d).abs() == a_max).any())                  # the box is reached: the projection did work
