"""Wall time per rollout step of the evaluation with the two refinement implementations
(``refine_impl`` autograd / native), interleaved on one device.

    python scripts/bench_safety_filter.py [--num_agents 1024] [--num_envs 4] [--dim 2] [--num_obstacles 0]
                                          [--refine_loops 50] [--steps 10] [--warmup 2] [--rounds 3]
                                          [--dtype fp32] [--impl loop|persistent]

Every round runs warmup + steps fixed rollout steps (no early stop) per implementation on the
same scenario and random-init networks. A step is the evaluation's own (``evaluate.rollout_eval``:
kNN, controller, refinement, Euler step, safety count; the native path keeps its iteration count
on the device), timed between device synchronisations. Prints one JSON line with the mean / min
per-step milliseconds of both. ``--impl`` picks the native filter's implementation
(``safety_filter(impl=...)``; default: its automatic choice); the two native implementations are
compared in one process by ``scripts/bench_validate.py impl``."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from macbf_gnn_amd import evaluate as EV                                        # noqa: E402
from macbf_gnn_amd.models import CBF, Controller                               # noqa: E402
from macbf_gnn_amd.ops.refine import safety_filter                             # noqa: E402


def rollout(ctrl, cbf, s, g, obs, cfg, steps, impl=None):
    """-> (per-step wall ms, refinement iterations)"""
    k = min(cfg.top_k, s.shape[1])
    iters = 0
    iters_dev = torch.zeros((), dtype=torch.int64, device=s.device)
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx = EV._knn(s, k, obs)
        with torch.no_grad():
            a = ctrl(s, g, idx=idx, obstacles=obs)
        if cfg.refine_impl == "native":
            a, used, _ = safety_filter(cbf, s, a, idx, obstacles=obs, loops=cfg.refine_loops, lr=cfg.refine_lr,
                                       impl=impl)
            iters_dev += used
        else:
            a, it, _ = EV.refine_actions(cbf, s, a, idx, cfg.refine_loops, cfg.refine_lr, obstacles=obs)
            iters += it
        with torch.no_grad():
            s = EV._euler(s, a)
            EV._safe_count(s, obs)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms, iters + int(iters_dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_agents", type=int, default=1024)
    ap.add_argument("--num_envs", type=int, default=4)
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--num_obstacles", type=int, default=0)
    ap.add_argument("--refine_loops", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--impl", choices=["loop", "persistent"], default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(a.seed)
    ctrl, cbf = Controller(2 * a.dim).to(dev).eval(), CBF(2 * a.dim).to(dev).eval()
    ctrl.mfma_dtype = cbf.mfma_dtype = EV.MFMA_DTYPES[a.dtype]
    times = {"autograd": [], "native": []}
    iters = {}
    for _ in range(a.rounds):
        for impl in ("autograd", "native"):
            cfg = EV.EvalConfig(num_agents=a.num_agents, num_envs=a.num_envs, refine_loops=a.refine_loops, dim=a.dim,
                                num_obstacles=a.num_obstacles, dtype=a.dtype, refine_impl=impl, seed=a.seed)
            s0, g, obs = EV.sample_scenarios(cfg, 0, dev)
            ms, n = rollout(ctrl, cbf, s0, g, obs, cfg, a.warmup + a.steps, a.impl)
            times[impl] += ms[a.warmup:]
            iters[impl] = n
    out = {"num_agents": a.num_agents, "num_envs": a.num_envs, "dim": a.dim, "num_obstacles": a.num_obstacles,
           "refine_loops": a.refine_loops, "dtype": a.dtype, "impl": a.impl, "steps_timed": a.steps * a.rounds}
    for impl, d in times.items():
        out[f"{impl}_ms_per_step_mean"] = sum(d) / len(d)
        out[f"{impl}_ms_per_step_min"] = min(d)
        out[f"{impl}_refine_iters"] = iters[impl]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
