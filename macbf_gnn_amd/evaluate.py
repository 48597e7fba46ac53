"""Evaluation with test-time action refinement (the reference defines
``EVALUATE_STEPS``, ``REFINE_LOOPS``, ``REFINE_LEARNING_RATE`` at ``config.py:17,19-20`` but never
uses them).

Scenes are D-dimensional (D = 2 or 3) double integrators, optionally with static obstacle points
that join the graph as non-controlled nodes (``oracle.with_obstacles``): kNN, the CBF and the
safety check see agents + obstacle points, actions exist for the agents only.

Per rollout step:
    idx     = kNN(s_t)                                   (K1, native on the HIP device)
    a       = pi(s_t, g)                                 (controller)
    refine  : a_r = a + delta, delta <- delta - lr * d/d delta  sum_e relu(-(h(s') - h(s) + dt*alpha*h(s)))
              with s' = s + dt * [v, a_r], h on the time-t neighbour slots, until the discrete CBF
              condition holds on every radius-masked edge or REFINE_LOOPS steps are spent
    s_{t+1} = s_t + dt * [v, a_r]
Metrics: safety rate (all-pairs TTC check with DIST_MIN_CHECK / TIME_TO_COLLISION_CHECK, the
``core.py:212-231`` formula), reaching rate (agents within DIST_MIN_CHECK of their goal at the
end), mean final goal distance and refinement statistics.

On a HIP device the CBF and controller run through the native autograd Functions
(``ops/cbf.py``, ``ops/ctrl.py``); on CPU through the fp32 oracle. ``refine_impl="native"`` (HIP
only, opt-in) runs the action refinement as the device-resident safety filter of
``ops/refine.py`` (``csrc/refine.hip``) instead of the autograd loop.

Actuator limit (``a_max``, opt-in; all of it in fp32). A per-axis box: every component of the applied
action lies in [-a_max, a_max]. A box and not a norm ball because ``clamp`` is exact, so the Python
and native paths agree bit for bit.
    a_c   = clamp(a, -a_max, a_max)                      (nominal action)
    lo    = -a_max - a_c,  hi = a_max - a_c              (one subtraction each)
    delta <- min(max(delta - lr * (dt * g), lo), hi)     (the refinement step, then the projection;
                                                          s' is formed from a_c + delta)
    u     = clamp(a_c + delta, -a_max, a_max)            (applied action: the final clamp removes the
                                                          one rounding by which a_c + hi can pass a_max)
The early-out rule does not change: an iteration without an active edge ends the work, and a
saturated agent can keep an edge active for all ``loops`` iterations.

Coupling (``refine_coupling``, opt-in). ``"joint"`` (the default) is the filter above: one optimisation
over the whole scene, s'_j is formed from a_j + delta_j, so agent i's barrier also pushes its
neighbours' actions and every iteration is a round of neighbour-to-neighbour communication.
``"local"`` is the decentralised filter: every agent refines its own action alone.
    own state    s'_i = s_i + dt [v_i, a_i + delta_i]
    neighbours   s'_j = s_j + dt [v_j, a_j] for every slot with j != i: the neighbour's NOMINAL next state
                 (with a limit a_j is the clamped a_c; an obstacle node has a zero action)
    self slot    (idx == i) the agent's own refined state: its relative state is exactly zero and it
                 carries no gradient, as in the joint filter
    update       delta_i <- delta_i - lr * dt * sum_k dEv[i, k] over the agent's own K slots; no in-edge term
The hinge, the radius mask at s', h(s_t), the expression order of deriv, the projection onto the actuator
box and the final clamp are the joint filter's, and so are the result words: ``counts[it]`` the edges with
a non-zero hinge gradient in iteration it, ``viol`` the hinge sum over all edges at the last evaluated
iterate. An agent whose K edges are all inactive never moves again (its neighbours' terms are fixed), so
the stop rule -- an iteration that counts no active edge ends the work -- stays exact.

Action statistics (``ACTION_STATS``, with ``action_stats`` or a limit), over the agents of the envs
that are active at the start of a step (the mask that weights ``agent_steps``): agents with some
|u_q| == a_max, agents with some delta_q != 0, the sum over agents and components of
round(|delta_q| * 2^20) (float64, half-even, per component: an integer sum, so it does not depend on
the order) and the largest |u_q| (carried as the int bit pattern of the non-negative float and
reduced by an integer max).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import config as C
from . import oracle


@dataclass
class EvalConfig:
    num_agents: int = 32
    num_envs: int = 1
    episodes: int = C.EVALUATE_STEPS
    max_steps: int = C.INNER_LOOPS
    refine: bool = True
    refine_loops: int = C.REFINE_LOOPS
    refine_lr: float = C.REFINE_LEARNING_RATE
    top_k: int = C.TOP_K
    seed: int = 0
    early_stop: bool = True
    diagnose: bool = False      # dense all-pairs check: are the flagged pairs top-K neighbours?
    refine_space: str = "actions"   # "actions" (upstream MACBF) or "gains": refine only the PD gains
                                    # of the reference controller law (controller.py:53-61) -- what
                                    # the trained policy class itself can express
    dim: int = 2                # spatial dimension of the scenes (2 or 3)
    num_obstacles: int = 0      # static point-set obstacles per scene
    obstacle_points: int = 12   # points per obstacle (HIP sampler; the host sampler uses its default)
    dtype: str = "fp32"         # MFMA operand precision on HIP: evaluate() sets the networks' mfma_dtype
                                # (fp32 | bf16 | fp16); no effect on CPU (fp32 oracle)
    refine_impl: str = "autograd"   # "autograd" or "native" (HIP only): the device-resident filter
    rollout_impl: str = "python"    # "python" or "native" (HIP only, opt-in): the whole batch of episodes as one
                                    # native call (ops/episode.py); needs refine off or refine_impl="native",
                                    # refine_space="actions", diagnose off and early_stop on
    a_max: Optional[float] = None   # per-axis actuator limit on the applied action (module docstring); None: off.
                                    # Not with refine_space="gains" or diagnose. Implies action_stats
    action_stats: bool = False      # add limited_rate, intervention_rate, mean_abs_delta, max_abs_action
    refine_coupling: str = "joint"  # "joint": the centralised filter | "local": every agent refines its own action
                                    # against its neighbours' nominal next states (module docstring). Not with
                                    # refine_space="gains"


MFMA_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# the action statistics of a batch of episodes, an int64 vector: three sums, then a maximum
ACTION_STATS = ("limited_agent_steps", "intervened_agent_steps", "delta_abs_fx", "action_abs_max")
DELTA_FX = float(1 << 20)           # fixed-point scale of delta_abs_fx
_FX_SAT = float(1 << 46)            # a non-finite or absurd |delta| term (csrc/args.h FX_SAT)


def check_a_max(a_max) -> Optional[float]:
    """None (off), or the limit as the fp32 value every path compares with."""
    if a_max is None:
        return None
    a_max = float(a_max)
    if not math.isfinite(a_max) or a_max <= 0.0:
        raise ValueError(f"a_max must be a positive finite number (or None for no limit), got {a_max!r}")
    m = float(torch.tensor(a_max, dtype=torch.float32))
    if not math.isfinite(m) or m <= 0.0:
        raise ValueError(f"a_max = {a_max!r} is not a positive finite fp32 number")
    return m


COUPLINGS = ("joint", "local")


def check_coupling(coupling) -> str:
    if coupling not in COUPLINGS:
        raise ValueError(f"unknown coupling {coupling!r} (joint or local)")
    return coupling


def check_refine_coupling(cfg: "EvalConfig") -> str:
    """``cfg.refine_coupling`` checked; the option it cannot be combined with is an error that names it."""
    c = check_coupling(cfg.refine_coupling)
    if c == "local" and cfg.refine and cfg.refine_space == "gains":
        raise ValueError("refine_coupling='local' refines free actions: refine_space='gains' has no local variant; use "
                         "refine_space='actions' or refine_coupling='joint'")
    return c


def check_residual(controller, cfg: "EvalConfig") -> bool:
    """Whether ``controller`` has the residual head (``oracle.py``, "Residual head"); the option it cannot be
    combined with is an error that names it: the gain refinement moves the gain pre-activations alone and
    would drop the residual from the action."""
    res = bool(getattr(controller, "residual", False))
    if res and cfg.refine and cfg.refine_space == "gains":
        raise ValueError("a residual controller (ctrl_residual) commands more than the gain law: refine_space='gains' "
                         "refines the gains alone; use refine_space='actions'")
    return res


def check_action_limit(cfg: "EvalConfig") -> Optional[float]:
    """``cfg.a_max`` checked (``check_a_max``); the options a limit cannot be combined with are errors
    that name them."""
    m = check_a_max(cfg.a_max)
    if m is not None and cfg.refine and cfg.refine_space == "gains":
        raise ValueError("a_max limits free actions: refine_space='gains' has the gain law's own bounds; use "
                         "refine_space='actions' or a_max=None")
    if m is not None and cfg.diagnose:
        raise ValueError("a_max has no diagnose mode: use diagnose=False or a_max=None")
    return m


def action_stats(u, delta, active, a_max) -> torch.Tensor:
    """``ACTION_STATS`` of one step: u (B, N, D) applied actions, delta (B, N, D) the filter's correction
    or None (no filter), active (B,) bool the envs counted, a_max the fp32 limit or None -> int64 (4,)
    on u's device. Nothing is read on the host."""
    act = active.view(-1, 1)
    au = u.detach().float().abs()
    zero = torch.zeros((), dtype=torch.int64, device=u.device)
    limited = ((au == a_max).any(-1) & act).sum() if a_max is not None else zero
    amax = (au.contiguous().view(torch.int32).amax(-1).long() * act).max()
    if delta is None:
        return torch.stack([limited, zero, zero, amax])
    d = delta.detach().float()
    x = d.abs().double() * DELTA_FX
    fx = torch.where((x >= 0) & (x < _FX_SAT), x.round(), torch.full_like(x, _FX_SAT)).long()
    return torch.stack([limited, ((d != 0).any(-1) & act).sum(), (fx.sum(-1) * act).sum(), amax])


def merge_action_stats(total, step):
    """Running ``ACTION_STATS``: the sums add, the bit pattern of the largest |u| is an integer max."""
    return torch.cat([total[:3] + step[:3], torch.maximum(total[3:], step[3:])])


def action_metrics(c: Dict[str, int], agent_steps: int, D: int) -> Dict[str, float]:
    """The four result keys from the integer statistics (a dict over ``ACTION_STATS``)."""
    n = max(agent_steps, 1)
    bits = torch.tensor(c["action_abs_max"], dtype=torch.int64).to(torch.int32)
    return {"limited_rate": c["limited_agent_steps"] / n, "intervention_rate": c["intervened_agent_steps"] / n,
            "mean_abs_delta": c["delta_abs_fx"] / DELTA_FX / (n * D), "max_abs_action": float(bits.view(torch.float32))}


def _knn(s, k, obstacles=None):
    if s.is_cuda:
        from .ops import graph
        return graph.knn(s, k, obstacles).long()
    if obstacles is None:
        return oracle.knn_idx(s, k)
    return oracle.knn_idx(s, k, oracle.with_obstacles(s, obstacles))


def _safe_count(s, obstacles=None):
    if s.is_cuda:
        from .ops import graph
        return graph.safe_agent_count(s, obstacles)
    if obstacles is None:
        return oracle.safe_agent_count(s).float()
    return oracle.safe_agent_count(s, oracle.with_obstacles(s, obstacles)).float()


def _euler(s, a):
    """s_{t+1} = s_t + dt [v, a] of the D-dimensional double integrator."""
    D = s.shape[-1] // 2
    return s + torch.cat([s[..., D:], a], -1) * C.TIME_STEP


def refine_actions(cbf, s, a, idx, loops: int = C.REFINE_LOOPS, lr: float = C.REFINE_LEARNING_RATE,
                   check_every: int = 10, obstacles=None, a_max=None, return_delta: bool = False,
                   coupling: str = "joint"):
    """Gradient refinement of the actions on the discrete CBF condition. Returns
    (refined actions, iterations used, remaining violation sum).

    ``coupling``: "joint" (the loop below, through ``cbf``) or "local" (the decentralised rule of the
    module docstring). The local filter is built from the oracle's functions -- ``oracle.edge_rel`` of
    the refined states against the nominal next nodes, the self rows zeroed, then the layers of
    ``oracle.cbf_forward`` on ``cbf.params_dict()`` -- in fp32 torch ops on whatever device the tensors
    are on. It does not go through the native autograd Functions: on a HIP device it is the slow
    reference of ``ops.refine.safety_filter(coupling="local")``, not a production path.

    ``a_max``: the actuator limit of the module docstring -- the action is clamped first, every step is
    projected onto [lo, hi] and the result is clamp(a_c + delta). ``return_delta`` appends ``delta``.

    The violation is a hinge: once it is exactly zero its gradient is exactly zero, so further
    iterations leave the actions unchanged. The loop therefore only looks at the violation on
    the host every ``check_every`` iterations (one sync instead of one per iteration); the
    iteration count (iterations that still had a violation) is kept on the device.

    ``obstacles`` (B, M, D): static points among the neighbour slots of ``idx``; they have no action
    and do not move, so ``delta`` stays (B, N, D)."""
    a_max = check_a_max(a_max)
    local = check_coupling(coupling) == "local"
    with torch.no_grad():
        if a_max is not None:
            a = a.clamp(-a_max, a_max)
            lo, hi = -a_max - a, a_max - a
        if local:
            p = {k: v.detach() for k, v in cbf.params_dict().items()}
            h = oracle.cbf_forward(p, s, idx, nodes=oracle.with_obstacles(s, obstacles))
            nominal = oracle.with_obstacles(_euler(s, a), obstacles)      # s'_j of every node, fixed over the loop
        else:
            h = cbf(s, idx=idx, obstacles=obstacles)
    delta = torch.zeros_like(a, requires_grad=True)
    viol = torch.zeros((), device=s.device)
    used = torch.zeros((), dtype=torch.int64, device=s.device)
    for it in range(1, loops + 1):
        ar = a + delta
        s_next = _euler(s, ar)
        hn = _cbf_local(p, s_next, idx, nominal) if local else cbf(s_next, idx=idx, obstacles=obstacles)
        deriv = hn - h + C.TIME_STEP * C.ALPHA_CBF * h
        viol = torch.relu(-deriv).sum()
        pending = viol.detach() > 0
        used += pending.long()
        if it % check_every == 0 and not bool(pending):
            break
        g, = torch.autograd.grad(viol, delta)
        with torch.no_grad():
            delta -= lr * g
            if a_max is not None:
                delta.copy_(torch.min(torch.max(delta, lo), hi))
    out = (a + delta).detach()
    if a_max is not None:
        out = out.clamp(-a_max, a_max)
    if return_delta:
        return out, int(used), float(viol.detach()), delta.detach()
    return out, int(used), float(viol.detach())


def _cbf_local(p, s_next, idx, nominal):
    """h(s') of the local coupling: centre rows from ``s_next`` (the refined states), neighbour rows from
    ``nominal`` (the nominal next nodes), the self slots exactly zero; then ``oracle.cbf_forward``'s layers."""
    D = s_next.shape[-1] // 2
    rel, eye = oracle.edge_rel(s_next, idx, nodes=nominal)
    rel = torch.where(eye.bool().unsqueeze(-1), torch.zeros_like(rel), rel)
    d = torch.sqrt(oracle.sq_dist(rel, D) + C.CBF_DIST_EPS_COORD * D)
    z = torch.cat([rel, eye.unsqueeze(-1), (d - C.DIST_MIN_THRES).unsqueeze(-1)], dim=-1)
    mask = (d <= C.OBS_RADIUS).to(s_next.dtype)
    for i, act in ((0, True), (2, True), (4, True), (6, False)):
        z = oracle._lin(z, p[f"cbf_net.{i}.weight"], p[f"cbf_net.{i}.bias"], first=i == 0, head=i == 6)
        if act:
            z = torch.relu(z)
    return z[..., 0] * mask


def _pd_action(s, g, y):
    """The reference PD law a_d = -(k_2d (p_d - g_d) + k_2d+1 v_d), k = 2 sigmoid(y) + 0.2."""
    D = s.shape[-1] // 2
    k = 2.0 * torch.sigmoid(y) + 0.2
    return torch.stack([-(k[..., 2 * q] * (s[..., q] - g[..., q]) + k[..., 2 * q + 1] * s[..., D + q])
                        for q in range(D)], dim=-1)


def refine_gains(cbf, s, g, k0, idx, loops: int = C.REFINE_LOOPS, lr: float = C.REFINE_LEARNING_RATE,
                 check_every: int = 10, obstacles=None):
    """refine_actions restricted to the controller's action space: gradient steps on the gain
    pre-activations y (k = 2 sigmoid(y) + 0.2, started at the network's gains k0) instead of free
    actions."""
    with torch.no_grad():
        h = cbf(s, idx=idx, obstacles=obstacles)
        u = ((k0 - 0.2) / 2.0).clamp(1e-6, 1 - 1e-6)
        y = torch.log(u / (1 - u))
    y = y.clone().requires_grad_(True)
    viol = torch.zeros((), device=s.device)
    used = torch.zeros((), dtype=torch.int64, device=s.device)
    for it in range(1, loops + 1):
        a = _pd_action(s, g, y)
        s_next = _euler(s, a)
        hn = cbf(s_next, idx=idx, obstacles=obstacles)
        viol = torch.relu(-(hn - h + C.TIME_STEP * C.ALPHA_CBF * h)).sum()
        pending = viol.detach() > 0
        used += pending.long()
        if it % check_every == 0 and not bool(pending):
            break
        gy, = torch.autograd.grad(viol, y)
        with torch.no_grad():
            y -= lr * gy
    with torch.no_grad():
        return _pd_action(s, g, y), int(used), float(viol.detach())


def _unsafe_diag(s_next, idx, obstacles=None):
    """(unsafe agents, unsafe agents whose every flagged pair is one of their top-K neighbours at
    the step's graph) -- do the controller / CBF see the pairs that the safety check flags?"""
    nodes = None if obstacles is None else oracle.with_obstacles(s_next, obstacles)
    dang = oracle.ttc_mask_all_pairs(s_next, nodes)           # (B, N, Nn) check mask
    unsafe = dang.any(-1)
    in_k = torch.zeros_like(dang)
    in_k.scatter_(-1, idx.long(), True)
    seen = unsafe & ~(dang & ~in_k).any(-1)
    return unsafe.sum(), seen.sum()


def check_rollout_impl(cfg: EvalConfig, device) -> None:
    """``rollout_impl="native"`` runs the episodes of ``rollout_eval`` as one native call: every option
    it cannot honour is an error that names the option, never a silent change of what is measured."""
    if cfg.rollout_impl not in ("python", "native"):
        raise ValueError(f"unknown rollout_impl {cfg.rollout_impl!r} (python or native)")
    if cfg.rollout_impl != "native":
        return
    if cfg.diagnose:
        raise ValueError("rollout_impl='native' has no diagnose mode: use diagnose=False or rollout_impl='python'")
    if cfg.refine and cfg.refine_space != "actions":
        raise ValueError(f"rollout_impl='native' refines actions only: refine_space={cfg.refine_space!r} needs "
                         "rollout_impl='python'")
    if cfg.refine and cfg.refine_impl != "native":
        raise ValueError(f"rollout_impl='native' runs the device-resident filter: refine_impl={cfg.refine_impl!r} "
                         "needs rollout_impl='python' (or set refine_impl='native' or refine=False)")
    if not cfg.early_stop:
        raise ValueError("rollout_impl='native' stops moving a finished scene: early_stop=False needs "
                         "rollout_impl='python'")
    if torch.device(device).type != "cuda":
        raise ValueError("rollout_impl='native' runs the episodes as native HIP kernels (ops/episode.py): it needs a "
                         "HIP device; use rollout_impl='python' on CPU")


def _rollout_native(controller, cbf, s0, g, cfg: EvalConfig, obstacles) -> Dict[str, float]:
    """``rollout_eval``'s result dict from the count vector of ``ops.episode.run_episodes`` with the
    evaluation's rule (``mask_done=False``: a finished env is still refined until the batch stops)."""
    from . import validate as V
    from .ops import episode
    B, N, _ = s0.shape
    a_max = check_action_limit(cfg)
    stats = cfg.action_stats or a_max is not None
    vec = episode.run_episodes(controller, cbf, s0, g, obstacles, refine=cfg.refine, loops=cfg.refine_loops,
                               lr=cfg.refine_lr, max_steps=cfg.max_steps, top_k=cfg.top_k, mask_done=False,
                               check_every=V.CHECK_EVERY, a_max=a_max, action_stats=stats,
                               coupling=check_refine_coupling(cfg))
    if stats:
        vec = torch.cat(vec)
    tot = [int(x) for x in vec.tolist()]                             # the one host read
    c = dict(zip(V.COUNTS, tot))
    # the Python loop's fp32 mean over a (B, N) 0 / 1 tensor, formed the same way from the count
    hit = torch.arange(B * N, device=s0.device).view(B, N) < c["reached_agents"]
    out = {"safety_rate": float(c["safe_agent_steps"]) / max(c["agent_steps"], 1),
           "reaching_rate": float(hit.float().mean()),
           "mean_goal_dist": c["goal_dist_fx"] / V.DIST_FX / max(c["agents"], 1),
           "steps": c["steps"], "agent_steps": c["agent_steps"],
           "refine_iters": c["refine_iters"]}
    if stats:
        out.update(action_metrics(dict(zip(ACTION_STATS, tot[len(V.COUNTS):])), c["agent_steps"], s0.shape[-1] // 2))
    return out


def rollout_eval(controller, cbf, s0, g, cfg: EvalConfig, obstacles=None) -> Dict[str, float]:
    """One batch of episodes from ``s0`` (B, N, 2D) towards ``g`` (B, N, D); ``obstacles`` (B, M, D)
    are static graph nodes seen by kNN, the controller, the CBF and the safety check."""
    if cfg.refine_impl not in ("autograd", "native"):
        raise ValueError(f"unknown refine_impl {cfg.refine_impl!r} (autograd or native)")
    check_rollout_impl(cfg, s0.device)
    check_residual(controller, cfg)
    a_max = check_action_limit(cfg)
    coupling = check_refine_coupling(cfg)
    stats = cfg.action_stats or a_max is not None
    if cfg.rollout_impl == "native":
        return _rollout_native(controller, cbf, s0, g, cfg, obstacles)
    native_filter = cfg.refine and cfg.refine_impl == "native" and cfg.refine_space != "gains"
    if cfg.refine_impl == "native" and not s0.is_cuda:
        raise ValueError("refine_impl='native' is the HIP safety filter (csrc/refine.hip): it needs a HIP device; "
                         "use refine_impl='autograd' on CPU")
    s = s0
    B, N, _ = s.shape
    D = s.shape[-1] // 2
    obs = obstacles
    k = min(cfg.top_k, N)
    safe_sum = 0.0
    steps = 0
    refine_iters = 0
    iters_dev = torch.zeros((), dtype=torch.int64, device=s.device)   # native filter: read once per episode
    unsafe_n = torch.zeros((), device=s.device)
    seen_n = torch.zeros((), device=s.device)
    active = torch.ones(B, dtype=torch.bool, device=s.device)
    acts = torch.zeros(len(ACTION_STATS), dtype=torch.int64, device=s.device)     # read once per episode
    for t in range(cfg.max_steps):
        idx = _knn(s, k, obs)
        with torch.no_grad():
            a = controller(s, g, idx=idx, obstacles=obs)
            if a_max is not None:
                a = a.clamp(-a_max, a_max)
        a_nom, delta = a, None
        if cfg.refine and cfg.refine_space == "gains":
            with torch.no_grad():
                nodes = None if obs is None else oracle.with_obstacles(s, obs)
                _, aux = oracle.controller_forward(controller.params_dict(), s, g, idx, return_aux=True, nodes=nodes)
            a, it, _ = refine_gains(cbf, s, g, aux["gains"], idx, cfg.refine_loops, cfg.refine_lr, obstacles=obs)
            refine_iters += it
            delta = a - a_nom                       # the gain law has no delta of its own: what it changed
        elif native_filter:
            from .ops import refine as refine_ops
            a, used, _, delta = refine_ops.safety_filter(cbf, s, a, idx, obstacles=obs, loops=cfg.refine_loops,
                                                         lr=cfg.refine_lr, a_max=a_max, return_delta=True,
                                                         coupling=coupling)
            iters_dev += used
        elif cfg.refine:
            a, it, _, delta = refine_actions(cbf, s, a, idx, cfg.refine_loops, cfg.refine_lr, obstacles=obs, a_max=a_max,
                                             return_delta=True, coupling=coupling)
            refine_iters += it
        with torch.no_grad():
            if stats:
                acts = merge_action_stats(acts, action_stats(a, delta, active, a_max))
            s = _euler(s, a)
            safe = _safe_count(s, obs)
            safe_sum += float((safe * active.float()).sum())
            if cfg.diagnose:
                u, sn = _unsafe_diag(s[active], idx[active], None if obs is None else obs[active])
                unsafe_n += u
                seen_n += sn
            steps += int(active.sum()) * N
            dist = torch.linalg.vector_norm(s[..., :D] - g, dim=-1).mean(-1)
            active = active & (dist >= C.DIST_MIN_CHECK)
        if cfg.early_stop and not bool(active.any()):
            break
    if native_filter:
        refine_iters += int(iters_dev)
    with torch.no_grad():
        d = torch.linalg.vector_norm(s[..., :D] - g, dim=-1)
        reach = float((d < C.DIST_MIN_CHECK).float().mean())
        mean_dist = float(d.mean())
    out = {"safety_rate": safe_sum / max(steps, 1), "reaching_rate": reach, "mean_goal_dist": mean_dist,
           "steps": t + 1, "agent_steps": steps, "refine_iters": refine_iters}
    if stats:
        out.update(action_metrics(dict(zip(ACTION_STATS, (int(x) for x in acts.tolist()))), steps, D))
    if cfg.diagnose:
        out["unsafe_agent_steps"] = float(unsafe_n)
        out["unsafe_pairs_in_topk_share"] = float(seen_n) / max(float(unsafe_n), 1.0)
    return out


def sample_scenarios(cfg: EvalConfig, episode: int, device):
    """(s0, g, obstacles or None) of one evaluation episode. HIP: the on-device sampler. CPU: the
    2-D obstacle-free case keeps ``env.generate_batch`` and its seed formula (published numbers do
    not move); every other scene comes from ``env.generate_scenarios`` with the same seed."""
    from . import env as E
    if device.type == "cuda":
        from .ops import scenario
        return scenario.generate(cfg.num_envs, cfg.num_agents, seed=cfg.seed + 7919, iteration=episode, rank=0,
                                 device=device, dim=cfg.dim, num_obstacles=cfg.num_obstacles,
                                 obstacle_points=cfg.obstacle_points)
    if cfg.dim == 2 and cfg.num_obstacles == 0:
        s0, g = E.generate_batch(cfg.num_envs, cfg.num_agents, C.DIST_MIN_THRES, seed=cfg.seed * 7919 + episode)
        return s0, g, None
    return E.generate_scenarios(cfg.num_envs, cfg.num_agents, cfg.dim, cfg.num_obstacles,
                                seed=cfg.seed * 7919 + episode)


_MAX_KEYS = ("max_abs_action",)     # over the episodes: the maximum; every other key: the mean


def evaluate(controller, cbf, cfg: EvalConfig, device: Optional[torch.device] = None) -> Dict[str, float]:
    """Run ``cfg.episodes`` fresh scenarios; returns metrics averaged over episodes."""
    device = device or next(controller.parameters()).device
    if cfg.dim not in (2, 3):
        raise ValueError(f"dim must be 2 or 3, got {cfg.dim}")
    for name, net in (("controller", controller), ("cbf", cbf)):
        if getattr(net, "in_dim", 2 * cfg.dim) != 2 * cfg.dim:
            raise ValueError(f"{name} was built for {net.in_dim // 2}-D states, the evaluation runs dim={cfg.dim}")
    if cfg.dtype not in MFMA_DTYPES:
        raise ValueError(f"dtype must be one of {sorted(MFMA_DTYPES)}, got {cfg.dtype!r}")
    check_rollout_impl(cfg, device)
    check_action_limit(cfg)
    check_refine_coupling(cfg)
    check_residual(controller, cfg)
    if device.type == "cuda":
        controller.mfma_dtype = cbf.mfma_dtype = MFMA_DTYPES[cfg.dtype]
    controller.eval()
    cbf.eval()
    agg: Dict[str, float] = {}
    for ep in range(cfg.episodes):
        s0, g, obs = sample_scenarios(cfg, ep, device)
        r = rollout_eval(controller, cbf, s0.to(device), g.to(device), cfg,
                         obstacles=None if obs is None else obs.to(device))
        for kk, v in r.items():
            agg[kk] = max(agg.get(kk, 0.0), float(v)) if kk in _MAX_KEYS else agg.get(kk, 0.0) + float(v)
    return {kk: v if kk in _MAX_KEYS else v / cfg.episodes for kk, v in agg.items()}
