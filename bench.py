"""Headline benchmark: agent-steps/s of the full MACBF training loop (+ safety rate).

BASELINE.json metric "agent-steps/sec (train loop) + safety-rate, 1024 agents at 1/2/4/8 MI355X",
config "1024 agents, 64 batched envs, DP over xGMI (RCCL grad all-reduce)".

One timed step = a full training iteration on every rank: on-device scenario sampling,
rollout (kNN scan + fused controller, until every env is done or INNER_LOOPS), CBF losses,
hand-written backward through the CBF and BPTT through the rollout, RCCL all-reduce of the
flat gradient, fused Adam. agent-steps = sum over envs of N x valid rollout steps.
Default: BASELINE config #3 as stated -- 64 batched envs of 1024 agents over ALL ranks (strong
scaling: every rank trains 64 / world of them; --global_envs G changes the total). Weak scaling
(every rank trains its own --envs environments, 64 unless given) with --weak or an explicit
--envs. The JSON carries "scaling" and "global_batch" either way. Random-init weights, synthetic
scenarios from the on-device sampler (keyed by seed, iteration and rank).

Precision (--dtype): fp32 (default) is the reference precision (/root/reference is fp32 end to
end): the near-fp32 3-term split-bf16 MFMA kernels (each operand hi + lo, ~16 significant bits;
hi*hi + hi*lo + lo*hi, fp32 accumulation: ~2^-16 relative per product, tighter than the TF32 path
cuDNN uses for the reference's Conv1d layers). bf16 / fp16 are the faster 16-bit-input modes (fp16
with dynamic loss scaling). Default window: 20 timed steps after 5 warm-up steps.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dtype fp32|bf16|fp16] [--global_envs G | --weak | --envs E]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N

A plain run does only what the headline figure needs: set up, warm up, time the steps, print the
result line. --dump-outputs DIR also writes what the last timed step computed (dump_outputs
below). --full adds everything else the benchmark can measure, after the timed steps (today the
per-phase timings of --phases).

`python bench.py --gpus N` without a launcher starts the N ranks itself (parallel/launch.py): one
process per GPU, rank r on device r, over RCCL; it fails before any work if fewer than N devices
are visible (MACBF_DP_BACKEND=gloo rehearses N ranks on one device) or if a launcher's
WORLD_SIZE disagrees with --gpus.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# the reference publishes no numbers ("published": {}) and its train loop does not run
# at N=1024 (O((T*N)^2) scene): vs_baseline is null. The only N=1024 reference
# measurement is its rollout-only loop on CPU (autograd on, 93,009 agent-steps/s), reported as a
# non-comparable proxy (different workload, CPU).
CPU_ROLLOUT_PROXY = 93009.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks (one per GPU, RCCL). Standalone (WORLD_SIZE unset) N > 1 starts N rank "
                         "processes through torch.distributed.run; under a launcher it must equal WORLD_SIZE")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--envs", type=int, default=None,
                    help="environments per rank: weak scaling (default 64 with --weak)")
    ap.add_argument("--weak", action="store_true", help="weak scaling: --envs (default 64) environments per rank")
    ap.add_argument("--global_envs", type=int, default=64,
                    help="strong scaling (the default; BASELINE config #3: 64): environments over all ranks, "
                         "sharded per rank")
    ap.add_argument("--inner_loops", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no_early_stop", action="store_true", help="fixed-T (=inner_loops) throughput")
    ap.add_argument("--dim", type=int, default=2, choices=[2, 3], help="3: BASELINE config #5 (3-D)")
    ap.add_argument("--num_obstacles", type=int, default=0, help="static point-set obstacles per env")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16", "fp16"],
                    help="kernel precision: fp32 (reference precision, split-bf16 MFMA), bf16, fp16 "
                         "(dynamic loss scaling; BASELINE config #5)")
    ap.add_argument("--graph", action="store_true",
                    help="replay each iteration as captured HIP graphs (launch-bound small configs)")
    ap.add_argument("--phases", action="store_true",
                    help="after the timed loop, 2 extra steps with per-phase device-event timings")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: today the per-phase timings of --phases. A plain "
                         "run sets up, warms up, times --steps steps and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy "
                         "(see dump_outputs)")
    ap.add_argument("--device", default="hip", choices=["hip", "cpu"],
                    help="cpu: the pure-torch oracle engine over gloo (launch-path rehearsal and CPU tests; "
                         "not a benchmark)")
    args = ap.parse_args()

    import torch
    from macbf_gnn_amd.parallel import launch

    # the parent decides before any GPU call: device_count() does not initialise the device
    ndev = torch.cuda.device_count() if args.device == "hip" else 0
    plan = launch.plan(args.gpus, device_count=ndev, device=args.device)
    if plan.action == "spawn":
        sys.exit(launch.spawn(os.path.abspath(__file__), sys.argv[1:], plan.ranks))

    from macbf_gnn_amd import config as C
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP

    cpu = args.device == "cpu"
    if cpu:
        dev = torch.device("cpu")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a HIP device (--device cpu rehearses the launch path)")
        dev = torch.device("cuda", launch.device_index(plan, ndev))
        torch.cuda.set_device(dev)
    dp = DP(device=dev)
    world, rank = dp.world, dp.rank
    if world != plan.ranks:
        raise SystemExit(f"launch error: process group has {world} ranks, expected {plan.ranks}")
    # every rank reports its device; an RCCL run must hold one distinct device per rank
    dev_ids = dp.gather_ints([-1 if cpu else dev.index, _device_uid(torch, dev)])
    if not cpu and not plan.share_devices and len({u for _, u in dev_ids}) != world:
        raise SystemExit(f"launch error: ranks share devices {dev_ids}; RCCL needs one device per rank")
    sync = (lambda: None) if cpu else torch.cuda.synchronize
    strong = not args.weak and args.envs is None
    if strong and (args.global_envs < world or args.global_envs % world):
        raise SystemExit(f"--global_envs {args.global_envs} must be a positive multiple of the world size {world}")
    envs = args.global_envs // world if strong else (args.envs or 64)
    cfg = C.TrainConfig(num_agents=args.agents, num_envs=envs, inner_loops=args.inner_loops,
                        seed=args.seed, device="cpu" if cpu else "hip", early_stop=not args.no_early_stop,
                        display_steps=10 ** 9, save_steps=10 ** 9, dim=args.dim, num_obstacles=args.num_obstacles,
                        dtype=args.dtype if not cpu else "fp32", graph=args.graph and not cpu)
    tr = Trainer(cfg, device=dev, dp=dp)

    for _ in range(args.warmup):
        tr.train_step()
    dp.barrier()
    sync()
    t0 = time.perf_counter()
    stats = [tr.train_step() for _ in range(args.steps)]   # device-resident until read
    dp.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    elapsed = dp.max_scalar(elapsed)
    acc = torch.tensor([[float(st["agent_steps"]), float(st["safe_agents"]), float(st["T"])] for st in stats],
                       dtype=torch.float64, device=dev).sum(0)    # agent_steps, safe_agents, T
    dp.all_reduce_(acc)
    agent_steps, safe_agents, t_sum = acc.tolist()
    if args.dump_outputs and rank == 0:      # before any extra step moves the parameters on
        dump_outputs(args.dump_outputs, tr, stats[-1] if stats else None)
    phases = None
    if args.phases or args.full:          # outside the timed region
        tr.timer.enabled = True
        tot = {}
        for _ in range(2):
            for k, v in tr.train_step().get("phases_ms", {}).items():
                tot[k] = tot.get(k, 0.0) + v / 2
        tr.timer.enabled = False
        phases = {k: round(v, 3) for k, v in tot.items()}
    value = agent_steps / elapsed
    backend = dp.backend
    out = {
        "metric": f"agent-steps/sec (train loop) + safety-rate, {args.agents} agents",
        "value": value,
        "unit": "agent-steps/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1000.0 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": "strong" if strong else "weak",
        "vs_baseline": None,
        "dtype": cfg.dtype,
        "data": "synthetic (on-device scenario sampler, random-init weights)",
        "config": {"model": f"MACBF-GNN controller+CBF ({args.dim}-D double integrator, top-K=12"
                            + (f", {args.num_obstacles} obstacles x 12 points" if args.num_obstacles else "") + ")",
                   "agents": args.agents, "global_batch": envs * world, "envs_per_gpu": envs,
                   "seq_len": args.inner_loops, "parallelism": f"dp{world}"},
        "safety_rate": safe_agents / agent_steps if agent_steps > 0 else None,
        "mean_T": t_sum / (args.steps * world),
        "early_stop": not args.no_early_stop,
        "skipped_steps": tr.skipped_steps,
        "graph": cfg.graph,
        "world": world,
        "dp_backend": backend,
        "rccl_ranks": world if backend == "nccl" else 0,
        "device_ids": [d for d, _ in dev_ids],
        "shared_devices": plan.share_devices,
        "precision": {"fp32": "near-fp32: 3-term split-bf16 MFMA (hi*hi + hi*lo + lo*hi, ~2^-16 relative per "
                              "product), fp32 accumulate; fp32 distances, TTC, losses, Adam",
                      "bf16": "bf16 MFMA inputs, fp32 accumulate", "fp16": "fp16 MFMA inputs, fp32 accumulate, "
                      "dynamic loss scaling"}[cfg.dtype] if not cpu else "fp32 (CPU oracle engine)",
        "cpu_rollout_proxy": {"value": CPU_ROLLOUT_PROXY, "comparable": False,
                              "source": "BASELINE.md: reference rollout-only loop (no losses / backward) @ N=1024, "
                                        "CPU x8; the reference publishes no numbers"},
    }
    if cpu:
        out["device"] = "cpu"
    if phases is not None:
        out["phases_ms"] = phases
    if rank == 0:
        print(json.dumps(out), flush=True)
    dp.shutdown()


DUMP_STATS = ["loss_total", "loss_dang", "loss_safe", "loss_dang_deriv", "loss_safe_deriv", "loss_action",
              "acc_dang_sum", "acc_safe_sum", "acc_dang_deriv_sum", "acc_safe_deriv_sum",
              "n_dang", "n_safe", "agent_steps", "safe_agents", "T"]


def dump_outputs(path, tr, stats):
    """--dump-outputs: what a caller of ``train_step`` holds after the last timed step (rank 0's),
    one .npy each. The inputs depend only on the arguments (seeded weights, scenarios keyed by
    seed, iteration and rank), so two builds run with the same arguments compare file for file.

    params.npy  float32 (P,)   the flat parameters after the step's Adam update (P = 51141 at --dim 2)
    grad.npy    float32 (P,)   the step's flat gradient (all-reduced over the ranks)
    stats.npy   float64 (15,)  the step's statistics, in the order of DUMP_STATS
    """
    import numpy as np
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "params.npy"), tr.fp.flat.detach().float().cpu().numpy())
    np.save(os.path.join(path, "grad.npy"), tr.fp.grad.detach().float().cpu().numpy())
    if stats is not None:
        np.save(os.path.join(path, "stats.npy"),
                np.array([float(stats.get(k, float("nan"))) for k in DUMP_STATS], dtype=np.float64))


def _device_uid(torch, dev) -> int:
    """A 62-bit id of the physical device (its UUID, else bus id) for the distinct-device check."""
    if dev.type != "cuda":
        return -1
    import hashlib
    p = torch.cuda.get_device_properties(dev)
    uuid = str(getattr(p, "uuid", "") or "")
    if set(uuid) <= set("GPU-0"):
        uuid = ""        # unreported / all-zero UUID: every rank would hash alike
    key = uuid or (f"pci {getattr(p, 'pci_domain_id', 0)}:{getattr(p, 'pci_bus_id', dev.index)}:"
                   f"{getattr(p, 'pci_device_id', 0)}")
    return int.from_bytes(hashlib.sha1(key.encode()).digest()[:8], "little") >> 2


if __name__ == "__main__":
    main()
