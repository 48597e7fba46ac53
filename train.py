"""Training entry point, reference-compatible CLI (``/root/reference/train.py:17-23``).

    python train.py --num_agents N [--model_path P] [--gpu G]

plus the knobs of SURVEY 5.6. Data parallel: launch one process per GPU with
``python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py ...``;
each rank trains ``--num_envs`` environments and gradients are all-reduced over RCCL.
``--val_every K`` adds a closed-loop validation on held-out scenes every K iterations (one extra
JSON line, with and without the CBF safety filter); ``--save_best`` keeps ``<model_path>.best``;
``--val_a_max A`` validates under the actuator limit |u| <= A per axis; ``--a_max A`` trains under it
(the rollout applies the clamped action, the backward masks the saturated components; the log lines
gain ``limited_rate``). Neither option follows the other. ``--ctrl_residual`` gives the controller the
residual head: an additive acceleration beside the gain law, which starts at zero (an architecture
choice: a resumed checkpoint must agree; not with ``--graph``). ``--val_refine_coupling local`` validates with
the decentralised filter (every agent refines its own action alone).
"""
from __future__ import annotations

import argparse
import os


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="MACBF-GNN trainer (MI355X-native)")
    p.add_argument("--num_agents", type=int, required=True)
    p.add_argument("--model_path", type=str, default=None,
                   help="checkpoint path: resumed from if it exists, saved every SAVE_STEPS")
    p.add_argument("--gpu", type=str, default=None,
                   help="device index (sets HIP_VISIBLE_DEVICES before torch initialises HIP)")
    p.add_argument("--num_envs", type=int, default=1, help="batched environments per rank")
    p.add_argument("--train_steps", type=int, default=None)
    p.add_argument("--inner_loops", type=int, default=None)
    p.add_argument("--top_k", type=int, default=None)
    p.add_argument("--lr", type=float, default=None)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=str, default="auto", choices=["auto", "cpu", "hip"])
    p.add_argument("--dtype", type=str, default="fp32", choices=["fp32", "bf16", "fp16"],
                   help="HIP kernel precision: fp32 (default; fp32-accurate split-bf16 MFMA, the reference's "
                        "precision), bf16 or fp16 (faster; fp16 with dynamic loss scaling); the CPU path is fp32")
    p.add_argument("--no_bptt", action="store_true", help="detach states between rollout steps")
    p.add_argument("--no_reuse_nbr_idx", action="store_true", help="recompute kNN for h(s')")
    p.add_argument("--alternate_every", type=int, default=0)
    p.add_argument("--no_early_stop", action="store_true")
    p.add_argument("--display_steps", type=int, default=None)
    p.add_argument("--save_steps", type=int, default=None)
    p.add_argument("--log_path", type=str, default=None)
    p.add_argument("--noise_prob", type=float, default=None)
    p.add_argument("--dim", type=int, default=2, choices=[2, 3], help="spatial dimension of the double integrator")
    p.add_argument("--num_obstacles", type=int, default=0, help="static point-set obstacles per env")
    p.add_argument("--graph", action="store_true",
                   help="HIP: replay each iteration as captured graphs (launch-bound small configs)")
    p.add_argument("--val_every", type=int, default=0,
                   help="closed-loop validation on held-out scenes every this many iterations (0: off)")
    p.add_argument("--val_envs", type=int, default=None, help="validation scenes per rank")
    p.add_argument("--no_val_refine", action="store_true", help="validate the controller only (no safety filter)")
    p.add_argument("--val_refine_loops", type=int, default=None)
    p.add_argument("--val_impl", type=str, default="python", choices=["python", "native"],
                   help="validation rollouts as torch ops (python) or as one native call each (native, HIP only)")
    p.add_argument("--val_a_max", type=float, default=0.0,
                   help="per-axis actuator limit |u| <= this on the validation rollouts (0: off); adds the limited / "
                        "intervention rates to the validation line")
    p.add_argument("--val_refine_coupling", type=str, default="joint", choices=["joint", "local"],
                   help="the validation filter: joint (centralised) or local (every agent refines its own action "
                        "against its neighbours' nominal next states)")
    p.add_argument("--a_max", type=float, default=0.0,
                   help="per-axis actuator limit |u| <= this on the TRAINING rollouts (0: off): clamp in the rollout, "
                        "mask in the backward; adds limited_rate to the log lines. --val_a_max is set separately")
    p.add_argument("--ctrl_residual", action="store_true",
                   help="controller with the residual head: the last node layer has 3D rows, a_d = -(kp e + kv v) + r_d "
                        "(zero at the start); combines with --a_max, not with --graph")
    p.add_argument("--save_best", action="store_true",
                   help="keep <model_path>.best at the best validation value of --best_metric")
    p.add_argument("--best_metric", type=str, default="",
                   help="val_*_rate key to keep the best checkpoint by (default: val_refined_safety_rate)")
    return p.parse_args(argv)


def build_config(args):
    from macbf_gnn_amd import config as C
    if args.ctrl_residual and args.graph:
        raise SystemExit("train.py: --ctrl_residual has no graph mode; drop --graph or --ctrl_residual")
    cfg = C.TrainConfig(num_agents=args.num_agents, num_envs=args.num_envs, seed=args.seed,
                        device=args.device, dtype=args.dtype, bptt=not args.no_bptt,
                        reuse_nbr_idx=not args.no_reuse_nbr_idx,
                        alternate_every=args.alternate_every, early_stop=not args.no_early_stop,
                        model_path=args.model_path, log_path=args.log_path, dim=args.dim,
                        num_obstacles=args.num_obstacles, graph=args.graph, val_every=args.val_every,
                        val_refine=not args.no_val_refine, save_best=args.save_best, best_metric=args.best_metric,
                        val_impl=args.val_impl, val_a_max=args.val_a_max, a_max=args.a_max,
                        val_refine_coupling=args.val_refine_coupling, ctrl_residual=args.ctrl_residual)
    for name in ("train_steps", "inner_loops", "top_k", "lr", "display_steps", "save_steps", "val_envs",
                 "val_refine_loops"):
        v = getattr(args, name)
        if v is not None:
            setattr(cfg, name, v)
    if args.noise_prob is not None:
        cfg.add_noise_prob = args.noise_prob
    return cfg


def main(argv=None):
    args = parse_args(argv)
    if args.gpu is not None and "LOCAL_RANK" not in os.environ:
        # must happen before HIP initialises (the reference sets it after import torch, train.py:28)
        os.environ["HIP_VISIBLE_DEVICES"] = args.gpu
    from macbf_gnn_amd.engine import Trainer
    cfg = build_config(args)
    tr = Trainer(cfg)
    tr.fit(progress=True)
    if cfg.model_path:
        tr.save(cfg.model_path)
    tr.dp.shutdown()


if __name__ == "__main__":
    main()
