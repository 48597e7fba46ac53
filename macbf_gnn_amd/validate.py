"""Validation during training: closed-loop episodes on held-out scenes, with and without the CBF
safety filter.

The training log shows the open-loop statistics of the training rollouts. What a user picks a
checkpoint by is the closed-loop behaviour: how safe the controller is on its own, and how safe
and how far-reaching it is with the trained CBF as a test-time filter. ``Validator`` measures both
on ``val_envs`` scenes per rank that are sampled once, from a seed stream of their own, and kept on
the device for the whole run, so successive validations are comparable.

Per ``validate(controller, cbf)`` two rollouts run from those scenes: nominal (controller only) and
filtered (skipped with ``val_refine=False``). The metric definitions are those of
``evaluate.rollout_eval`` (safety on s_{t+1} of the envs active at step t, reaching at the episode's
end, ``max_steps = inner_loops``, stop when every env is done), with one deliberate difference: an
env whose episode is over is no longer refined, it takes the controller's action. On a HIP device
that is the per-env mask of the device-resident filter (``ops.refine.safety_filter(...,
env_active=active)``); on CPU ``evaluate.refine_actions`` runs on the active sub-batch.

Everything is counted on the device in integers. The host looks at the "all done" flag every
``CHECK_EVERY`` steps and reads the totals once; a step that runs after every env is done changes
neither the counts nor the states, so the result does not depend on that period. The count vectors
are summed over the DP ranks before any ratio is taken: every rank returns the same dict.

``Validator(impl="native")`` (``TrainConfig.val_impl``, ``train.py --val_impl native``; HIP only,
opt-in) runs each rollout as one native call, ``ops.episode.run_episodes(..., mask_done=True)``:
the same count vector, so everything after ``rollout()`` is shared. ``"python"`` stays the default
and the reference.

``val_a_max > 0`` (``TrainConfig.val_a_max``, ``train.py --val_a_max``; 0: off) puts the per-axis
actuator limit of ``evaluate.py``'s module docstring on both rollouts: the nominal action is clamped,
the filter projects, and the dict gains ``val_limited_rate``, ``val_refined_limited_rate``,
``val_refined_intervention_rate`` and ``val_refined_mean_abs_delta``. Their three integer sums
(``ACTION_SUMS``) travel in the same all-reduce, after the existing counts; the largest |u| is left
out (it would need a second reduction of another kind). Training rollouts are not touched.

``val_refine_coupling="local"`` (``train.py --val_refine_coupling local``; default ``"joint"``) filters
with the decentralised rule of ``evaluate.py``'s module docstring, with both ``val_impl``s; ``COUNTS``
and the keys of the dict do not change.

Precision (HIP): the networks run at the training ``dtype``. The filter has no fp16 build (its -1
upstream gradient has no loss scaling), so a run that trains in fp16 validates both networks in
bf16. ``validate`` puts ``mfma_dtype`` and the train / eval mode of both modules back, draws from
no torch RNG, and uses none of the training engine's buffers, graphs or prefetched samples.
"""
from __future__ import annotations

import time
from typing import Dict, Optional

import torch

from . import config as C
from .evaluate import (ACTION_STATS, DELTA_FX, MFMA_DTYPES, _euler, _knn, _safe_count, action_stats, check_a_max,
                       check_coupling,
                       refine_actions)

VAL_SALT = 0x56414C5345454453          # the validation scenes' seed stream: _mix(cfg.seed, VAL_SALT)
CHECK_EVERY = 5                        # rollout steps between host reads of the "all done" flag
DIST_FX = float(1 << 20)               # fixed-point scale of the goal-distance sum
COUNTS = ("safe_agent_steps", "agent_steps", "reached_agents", "agents", "env_steps", "refine_iters", "steps",
          "goal_dist_fx")
ACTION_SUMS = ACTION_STATS[:3]         # with val_a_max: the integer sums that follow COUNTS in a rollout's vector
RATE_KEYS = ("val_safety_rate", "val_reaching_rate", "val_refined_safety_rate", "val_refined_reaching_rate")
_UNSET = object()


def default_best_metric(cfg) -> str:
    return cfg.best_metric or ("val_refined_safety_rate" if cfg.val_refine else "val_safety_rate")


IMPLS = ("python", "native")


def _check_val_coupling(cfg) -> str:
    try:
        return check_coupling(getattr(cfg, "val_refine_coupling", "joint"))
    except ValueError as e:
        raise ValueError(f"val_refine_coupling: {e}") from None


def check_config(cfg, device=None):
    """The validation entries of a TrainConfig that cannot work, reported before the run starts.
    ``device``: the device the run resolved to (``cfg.device`` may be "auto")."""
    impl = getattr(cfg, "val_impl", "python")
    if impl not in IMPLS:
        raise ValueError(f"val_impl must be one of {IMPLS}, got {impl!r}")
    on_cpu = cfg.device == "cpu" or (device is not None and torch.device(device).type == "cpu")
    if impl == "native" and on_cpu:
        raise ValueError("val_impl='native' runs the validation rollouts as native HIP episodes (ops/episode.py): it "
                         "needs a HIP device; use val_impl='python' on CPU")
    a_max = getattr(cfg, "val_a_max", 0.0)
    if a_max != 0.0:
        try:
            check_a_max(a_max)
        except ValueError as e:
            raise ValueError(f"val_a_max must be a positive finite number, or 0 for no limit: {e}") from None
    _check_val_coupling(cfg)
    if cfg.val_every < 0 or cfg.val_envs < 1 or cfg.val_refine_loops < 0:
        raise ValueError("val_every must be >= 0, val_envs >= 1 and val_refine_loops >= 0")
    m = default_best_metric(cfg)
    if m not in RATE_KEYS:
        raise ValueError(f"best_metric must be one of {RATE_KEYS}, got {m!r}")
    if not cfg.val_refine and "refined" in m:
        raise ValueError(f"best_metric {m!r} needs the filtered rollout, which val_refine=False turns off")
    if cfg.save_best and not cfg.model_path:
        raise ValueError("save_best writes <model_path>.best: it needs model_path")
    if cfg.save_best and cfg.val_every <= 0:
        raise ValueError("save_best needs validation: set val_every > 0")


def val_dtype(cfg) -> torch.dtype:
    """MFMA operand precision of the validation rollouts on a HIP device: the training dtype, bf16
    when that is fp16 (the filter refuses fp16, and both rollouts use one precision)."""
    return torch.bfloat16 if cfg.dtype == "fp16" else MFMA_DTYPES[cfg.dtype]


def metrics_from_counts(nom: Dict[str, int], ref: Optional[Dict[str, int]], num_agents: int,
                        dim: int = 2) -> Dict[str, float]:
    """The ``val_*`` ratios of the summed integer totals (``COUNTS``, with an actuator limit also
    ``ACTION_SUMS``) of the nominal and, if it ran, the filtered rollout."""
    envs = max(nom["agents"] // max(num_agents, 1), 1)
    out = {"val_safety_rate": nom["safe_agent_steps"] / max(nom["agent_steps"], 1),
           "val_reaching_rate": nom["reached_agents"] / max(nom["agents"], 1),
           "val_mean_goal_dist": nom["goal_dist_fx"] / DIST_FX / max(nom["agents"], 1),
           "val_mean_T": nom["env_steps"] / envs}
    if ref is not None:
        out.update({"val_refined_safety_rate": ref["safe_agent_steps"] / max(ref["agent_steps"], 1),
                    "val_refined_reaching_rate": ref["reached_agents"] / max(ref["agents"], 1),
                    "val_refined_mean_T": ref["env_steps"] / envs,
                    # filter iterations per rollout step of a rank's batch
                    "val_refine_iters": ref["refine_iters"] / max(ref["steps"], 1)})
    if "limited_agent_steps" in nom:
        out["val_limited_rate"] = nom["limited_agent_steps"] / max(nom["agent_steps"], 1)
        if ref is not None:
            n = max(ref["agent_steps"], 1)
            out.update({"val_refined_limited_rate": ref["limited_agent_steps"] / n,
                        "val_refined_intervention_rate": ref["intervened_agent_steps"] / n,
                        "val_refined_mean_abs_delta": ref["delta_abs_fx"] / DELTA_FX / (n * dim)})
    return out


class Validator:
    def __init__(self, cfg: C.TrainConfig, device: torch.device, dp=None, impl: Optional[str] = None):
        from .ops import scenario
        self.cfg = cfg
        self.device = device
        self.dp = dp
        self.impl = impl or getattr(cfg, "val_impl", "python")     # "native": rollout() is one native call
        if self.impl not in IMPLS:
            raise ValueError(f"impl must be one of {IMPLS}, got {self.impl!r}")
        if self.impl == "native" and torch.device(device).type != "cuda":
            raise ValueError("impl='native' needs a HIP device; use impl='python' on CPU")
        rank = dp.rank if dp is not None else 0
        s0, g, obs = scenario.generate(cfg.val_envs, cfg.num_agents, seed=scenario._mix(cfg.seed, VAL_SALT),
                                       iteration=0, rank=rank, device=device, dim=cfg.dim,
                                       num_obstacles=cfg.num_obstacles, obstacle_points=cfg.obstacle_points)
        self.s0 = s0.to(device).clone()
        self.g = g.to(device).clone()
        self.obs = None if obs is None else obs.to(device).clone()
        self.max_steps = int(cfg.inner_loops)
        self.a_max = check_a_max(getattr(cfg, "val_a_max", 0.0) or None)    # the fp32 limit, or None
        self.coupling = _check_val_coupling(cfg)           # the filter's coupling (evaluate.py)
        self.last_counts: Dict[str, Dict[str, int]] = {}      # the summed integer totals behind the last dict

    # ------------------------------------------------------------------ one rollout
    def _filter(self, cbf, s, a, idx, active):
        cfg = self.cfg
        if s.is_cuda:
            from .ops import refine as refine_ops
            a, used, _, delta = refine_ops.safety_filter(cbf, s, a, idx, obstacles=self.obs, loops=cfg.val_refine_loops,
                                                         lr=C.REFINE_LEARNING_RATE, env_active=active, a_max=self.a_max,
                                                         return_delta=True, coupling=self.coupling)
            return a, used, delta
        delta = torch.zeros_like(a)
        if not bool(active.any()):
            return a, 0, delta
        ar, it, _, dr = refine_actions(cbf, s[active], a[active], idx[active], cfg.val_refine_loops,
                                       C.REFINE_LEARNING_RATE, obstacles=None if self.obs is None else self.obs[active],
                                       a_max=self.a_max, return_delta=True, coupling=self.coupling)
        a = a.clone()
        a[active] = ar
        delta[active] = dr
        return a, it, delta

    def rollout(self, controller, cbf, refine: bool) -> torch.Tensor:
        """One batch of episodes from the fixed scenes -> this rank's totals, an int64 device vector
        in the order of ``COUNTS``, with an actuator limit followed by ``ACTION_SUMS``. No host read
        except the "all done" flag every CHECK_EVERY steps."""
        s, g, obs = self.s0, self.g, self.obs
        a_max = self.a_max
        if self.impl == "native":
            from .ops import episode
            kw = dict(refine=refine, loops=self.cfg.val_refine_loops, lr=C.REFINE_LEARNING_RATE, max_steps=self.max_steps,
                      top_k=self.cfg.top_k, mask_done=True, check_every=CHECK_EVERY, coupling=self.coupling)
            if a_max is None:
                return episode.run_episodes(controller, cbf, s, g, obs, **kw)
            vec, acts = episode.run_episodes(controller, cbf, s, g, obs, a_max=a_max, action_stats=True, **kw)
            return torch.cat([vec, acts[:len(ACTION_SUMS)]])
        B, N, _ = s.shape
        D = s.shape[-1] // 2
        k = min(self.cfg.top_k, N)
        dev = s.device
        zero = lambda: torch.zeros((), dtype=torch.int64, device=dev)
        safe_n, env_steps, iters, steps = zero(), zero(), zero(), zero()
        active = torch.ones(B, dtype=torch.bool, device=dev)
        acts = None if a_max is None else torch.zeros(len(ACTION_SUMS), dtype=torch.int64, device=dev)
        for t in range(self.max_steps):
            alive = active.any()                     # device flag: false -> this step changes nothing
            idx = _knn(s, k, obs)
            with torch.no_grad():
                a = controller(s, g, idx=idx, obstacles=obs)
                if a_max is not None:
                    a = a.clamp(-a_max, a_max)
            delta = None
            if refine:
                a, used, delta = self._filter(cbf, s, a, idx, active)
                iters += used
            with torch.no_grad():
                if a_max is not None:
                    acts += action_stats(a, delta, active, a_max)[:len(ACTION_SUMS)]
                s = torch.where(alive, _euler(s, a), s)
                act = active.long()
                safe_n += (_safe_count(s, obs).long() * act).sum()
                env_steps += act.sum()
                steps += alive.long()
                dist = torch.linalg.vector_norm(s[..., :D] - g, dim=-1).mean(-1)
                active = active & (dist >= C.DIST_MIN_CHECK)
            if (t + 1) % CHECK_EVERY == 0 and not bool(active.any()):
                break
        with torch.no_grad():
            d = torch.linalg.vector_norm(s[..., :D] - g, dim=-1)
            reached = (d < C.DIST_MIN_CHECK).sum()
            dist_fx = (d.double().sum() * DIST_FX).round().long()
            agents = torch.full((), B * N, dtype=torch.int64, device=dev)
            vec = torch.stack([safe_n, env_steps * N, reached, agents, env_steps, iters, steps, dist_fx])
            return vec if a_max is None else torch.cat([vec, acts])

    # ------------------------------------------------------------------ both rollouts, all ranks
    def _reduce(self, vec: torch.Tensor):
        dp = self.dp
        if dp is not None and dp.enabled:
            on_dev = dp.backend == "nccl" and self.device.type == "cuda"
            vec = vec.to(self.device if on_dev else "cpu")
            dp.all_reduce_(vec)
        return vec.cpu().tolist()

    def validate(self, controller, cbf) -> Dict[str, float]:
        cfg = self.cfg
        cuda = self.device.type == "cuda"
        if cuda:
            torch.cuda.synchronize(self.device)      # the pending training work is not validation time
        t0 = time.perf_counter()
        mods = (controller, cbf)
        modes = [m.training for m in mods]
        dtypes = [m.__dict__.get("mfma_dtype", _UNSET) for m in mods]
        try:
            for m in mods:
                m.eval()
                if cuda:
                    m.mfma_dtype = val_dtype(cfg)
            vecs = [self.rollout(controller, cbf, refine=False)]
            if cfg.val_refine:
                vecs.append(self.rollout(controller, cbf, refine=True))
        finally:
            for m, mode, dt in zip(mods, modes, dtypes):
                m.train(mode)
                if dt is _UNSET:
                    m.__dict__.pop("mfma_dtype", None)
                else:
                    m.mfma_dtype = dt
        n = len(COUNTS)
        # the existing counts of every rollout first, in their places; the action sums after them
        if self.a_max is not None:
            vecs = [v[:n] for v in vecs] + [v[n:] for v in vecs]
        tot = self._reduce(torch.cat(vecs))          # one collective, one host read
        nom = dict(zip(COUNTS, (int(x) for x in tot[:n])))
        ref = dict(zip(COUNTS, (int(x) for x in tot[n:2 * n]))) if cfg.val_refine else None
        if self.a_max is not None:
            m, base = len(ACTION_SUMS), n * (len(vecs) // 2)
            nom.update(zip(ACTION_SUMS, (int(x) for x in tot[base:base + m])))
            if ref is not None:
                ref.update(zip(ACTION_SUMS, (int(x) for x in tot[base + m:base + 2 * m])))
        self.last_counts = {"nominal": nom} if ref is None else {"nominal": nom, "refined": ref}
        out = metrics_from_counts(nom, ref, cfg.num_agents, cfg.dim)
        out["val_ms"] = (time.perf_counter() - t0) * 1e3
        return out


def better(value: float, best: Optional[float]) -> bool:
    """Strict improvement (higher is better)."""
    return best is None or value > best
