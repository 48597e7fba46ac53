"""Cost of the validation during training (macbf_gnn_amd/validate.py) on one device.

    python scripts/bench_validate.py validate [--num_agents 1024] [--val_envs 4] [--dtype fp32]
                                              [--model_path checkpoints/headline_4k.pt] [--rounds 5]
    python scripts/bench_validate.py mask     [--num_agents 1024] [--val_envs 4] [--dtype fp32]
                                              [--model_path checkpoints/headline_4k.pt] [--rounds 5]
                                              [--refine_loops 50]
    python scripts/bench_validate.py impl     [--num_agents 32] [--val_envs 8] [--dtype bf16]
                                              [--model_path checkpoints/cfg2_6k.pt] [--rounds 5]
    python scripts/bench_validate.py episode  [--num_agents 1024] [--val_envs 4] [--dtype fp32]
                                              [--model_path checkpoints/headline_4k.pt] [--rounds 5]

``validate``: wall time of ``Validator.validate`` (both rollouts, the totals' read included), one
warm-up call (scenes, packing tables) and ``--rounds`` timed ones.

``mask``: the effect of the filter's per-env mask. One filtered validation episode is recorded
(states, controller actions, kNN slots and the active mask of every step); then the filter alone
is run on those recorded steps with ``env_active=mask`` and with ``env_active=None``, interleaved
round by round, each episode timed between device synchronisations. The first recorded step is
then timed with B, B-1, .. 0 live envs (10 calls per reading, the minimum over the rounds).

``impl``: the two implementations of the filter (``safety_filter(impl="loop" / "persistent")``) on
a scene the persistent kernel takes (at most 64 graph nodes per env), interleaved round by round in
one process: the filter alone on the recorded steps of one filtered episode (as ``mask`` does, with
the recorded masks), and a whole ``validate()`` with ``MACBF_REFINE_SMALL`` forcing each path.
Reports the minimum, the mean and the spread (max - min) over the rounds, and checks that both
paths gave the same iteration count and the same validation counts.

``episode``: the two implementations of the validation rollouts, ``Validator(impl="python")`` (the
rollout as torch ops) and ``impl="native"`` (one native call per rollout, ops/episode.py), as whole
``validate()`` calls on the same scenes, interleaved round by round in one process: one warm-up
round, ``--rounds`` timed ones. Reports the minimum, the mean and the spread (max - min) of each, the
difference of the minima, whether it exceeds the Python path's spread, and whether both gave the
same counts.

``--val_a_max A`` puts the actuator limit |u| <= A on the validation rollouts of every mode that
runs ``validate()``.

Prints one JSON line. Without ``--model_path`` the networks are random-initialised."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from macbf_gnn_amd import config as C                                           # noqa: E402
from macbf_gnn_amd import validate as V                                         # noqa: E402
from macbf_gnn_amd.evaluate import _euler, _knn                                 # noqa: E402
from macbf_gnn_amd.models import CBF, Controller                               # noqa: E402
from macbf_gnn_amd.ops.refine import safety_filter                             # noqa: E402
from macbf_gnn_amd.utils import ckpt                                            # noqa: E402


def record_episode(v, ctrl, cbf, loops):
    """The filtered validation rollout, keeping every step's filter inputs."""
    s, g, obs = v.s0, v.g, v.obs
    B, N, _ = s.shape
    D = s.shape[-1] // 2
    active = torch.ones(B, dtype=torch.bool, device=s.device)
    rec = []
    for _ in range(v.max_steps):
        if not bool(active.any()):
            break
        idx = _knn(s, min(v.cfg.top_k, N), obs)
        with torch.no_grad():
            a = ctrl(s, g, idx=idx, obstacles=obs)
        rec.append((s, a, idx, active))
        a, _, _ = safety_filter(cbf, s, a, idx, obstacles=obs, loops=loops, env_active=active)
        with torch.no_grad():
            s = _euler(s, a)
            dist = torch.linalg.vector_norm(s[..., :D] - g, dim=-1).mean(-1)
            active = active & (dist >= C.DIST_MIN_CHECK)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["validate", "mask", "impl", "episode"])
    ap.add_argument("--num_agents", type=int, default=1024)
    ap.add_argument("--val_envs", type=int, default=4)
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--num_obstacles", type=int, default=0)
    ap.add_argument("--dtype", choices=["fp32", "bf16", "fp16"], default="fp32")
    ap.add_argument("--refine_loops", type=int, default=C.REFINE_LOOPS)
    ap.add_argument("--model_path", type=str, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--val_a_max", type=float, default=0.0, help="actuator limit of the validation rollouts (0: off)")
    a = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(a.seed)
    ctrl, cbf = Controller(2 * a.dim).to(dev), CBF(2 * a.dim).to(dev)
    if a.model_path:
        ckpt.load_models(a.model_path, ctrl, cbf)
    cfg = C.TrainConfig(num_agents=a.num_agents, val_every=1, val_envs=a.val_envs, dim=a.dim, seed=a.seed,
                        num_obstacles=a.num_obstacles, dtype=a.dtype, val_refine_loops=a.refine_loops, device="hip")
    if a.val_a_max:
        cfg.val_a_max = a.val_a_max
    v = V.Validator(cfg, dev)
    out = {"mode": a.mode, "num_agents": a.num_agents, "val_envs": a.val_envs, "dim": a.dim,
           "num_obstacles": a.num_obstacles, "dtype": a.dtype, "refine_loops": a.refine_loops,
           "model_path": a.model_path, "rounds": a.rounds, "val_a_max": a.val_a_max}
    if a.mode == "validate":
        res = v.validate(ctrl, cbf)                      # warm-up
        ms = [v.validate(ctrl, cbf)["val_ms"] for _ in range(a.rounds)]
        out.update({k: x for k, x in res.items() if k != "val_ms"})
        out.update({"val_ms": ms, "val_ms_min": min(ms), "val_ms_mean": sum(ms) / len(ms),
                    "counts": v.last_counts})
    elif a.mode == "episode":
        impls = ("python", "native")
        val, counts = {n: [] for n in impls}, {}
        for rnd in range(a.rounds + 1):                  # round 0 warms up
            for name in impls:
                v.impl = name
                ms = v.validate(ctrl, cbf)["val_ms"]
                if rnd:
                    val[name].append(ms)
                counts[name] = v.last_counts
        for name in impls:
            out[f"{name}_val_ms"] = val[name]
            out[f"{name}_val_ms_min"] = min(val[name])
            out[f"{name}_val_ms_mean"] = sum(val[name]) / len(val[name])
            out[f"{name}_val_ms_spread"] = max(val[name]) - min(val[name])
        gain = out["python_val_ms_min"] - out["native_val_ms_min"]
        fx = lambda c: {r: {k: x for k, x in d.items() if k != "goal_dist_fx"} for r, d in c.items()}
        out.update({"min_gain_ms": gain, "gain_exceeds_python_spread": gain > out["python_val_ms_spread"],
                    "same_val_counts": fx(counts["python"]) == fx(counts["native"]),
                    "goal_dist_fx": {n: {r: d["goal_dist_fx"] for r, d in counts[n].items()} for n in impls},
                    "counts": counts["native"]})
    elif a.mode == "impl":
        impls = ("loop", "persistent")
        knob = {"loop": "0", "persistent": "1"}
        val, counts = {n: [] for n in impls}, {}
        for rnd in range(a.rounds + 1):                  # round 0 warms up
            for name in impls:
                os.environ["MACBF_REFINE_SMALL"] = knob[name]
                ms = v.validate(ctrl, cbf)["val_ms"]
                if rnd:
                    val[name].append(ms)
                counts[name] = v.last_counts
        os.environ.pop("MACBF_REFINE_SMALL", None)
        ctrl.eval(), cbf.eval()
        ctrl.mfma_dtype = cbf.mfma_dtype = V.val_dtype(cfg)
        rec = record_episode(v, ctrl, cbf, a.refine_loops)
        times, iters = {n: [] for n in impls}, {}
        for rnd in range(a.rounds + 1):
            for name in impls:
                used_sum = torch.zeros((), dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s, act, idx, m in rec:
                    _, used, _ = safety_filter(cbf, s, act, idx, obstacles=v.obs, loops=a.refine_loops, env_active=m,
                                               impl=name)
                    used_sum += used
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(1e3 * (time.perf_counter() - t0))
                iters[name] = int(used_sum)
        out.update({"steps": len(rec), "same_refine_iters": iters["loop"] == iters["persistent"],
                    "same_val_counts": counts["loop"] == counts["persistent"], "refine_iters": iters["loop"]})
        for name in impls:
            for key, d in (("val_ms", val[name]), ("filter_episode_ms", times[name])):
                out[f"{name}_{key}_min"] = min(d)
                out[f"{name}_{key}_mean"] = sum(d) / len(d)
                out[f"{name}_{key}_spread"] = max(d) - min(d)
            out[f"{name}_filter_ms_per_step_min"] = min(times[name]) / max(len(rec), 1)
    else:
        ctrl.eval(), cbf.eval()
        ctrl.mfma_dtype = cbf.mfma_dtype = V.val_dtype(cfg)
        rec = record_episode(v, ctrl, cbf, a.refine_loops)
        live = [int(m.sum()) for _, _, _, m in rec]
        times = {"masked": [], "unmasked": []}
        iters = {}
        for rnd in range(a.rounds + 1):                  # round 0 warms up
            for name in ("masked", "unmasked"):
                used_sum = torch.zeros((), dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s, act, idx, m in rec:
                    _, used, _ = safety_filter(cbf, s, act, idx, obstacles=v.obs, loops=a.refine_loops,
                                               env_active=m if name == "masked" else None)
                    used_sum += used
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(1e3 * (time.perf_counter() - t0))
                iters[name] = int(used_sum)
        out.update({"steps": len(rec), "live_envs_per_step": live})
        # the first recorded step with B, B-1, .. 1, 0 live envs: what a masked-out env saves
        s, act, idx, _ = rec[0]
        sweep = {}
        for rnd in range(a.rounds + 1):
            for n_live in range(s.shape[0], -1, -1):
                m = torch.arange(s.shape[0], device=dev) < n_live
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    safety_filter(cbf, s, act, idx, obstacles=v.obs, loops=a.refine_loops, env_active=m)
                torch.cuda.synchronize()
                if rnd:
                    sweep.setdefault(n_live, []).append(1e2 * (time.perf_counter() - t0))
        out["first_step_ms_by_live_envs"] = {str(k): min(x) for k, x in sweep.items()}
        for name, d in times.items():
            out[f"{name}_episode_ms"] = d
            out[f"{name}_episode_ms_min"] = min(d)
            out[f"{name}_ms_per_step_min"] = min(d) / max(len(rec), 1)
            out[f"{name}_refine_iters"] = iters[name]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
