"""Evaluate a trained controller + CBF with test-time action refinement.

    python evaluate.py --num_agents 32 [--model_path ckpt.pt] [--num_envs 4] [--episodes 10]
                       [--max_steps 50] [--no_refine] [--refine_space actions|gains] [--diagnose]
                       [--dim 2|3] [--num_obstacles M] [--dtype fp32|bf16|fp16]
                       [--refine_impl autograd|native] [--rollout_impl python|native]
                       [--a_max A] [--action_stats] [--refine_coupling joint|local] [--ctrl_residual]
                       [--device auto|cpu|hip] [--gpu 0]

Prints one JSON line: safety rate, reaching rate, mean final goal distance, refinement
iterations. Without --model_path the networks are random-initialised (plumbing check).
--refine_space gains refines only the PD gains of the controller law (what the trained policy
class can express); --diagnose adds the share of unsafe pairs that are top-K neighbours.
--dim / --num_obstacles select the scene family (a checkpoint's dimension is read from its CBF
input layer and must agree with --dim); --dtype is the MFMA operand precision on a HIP device;
--refine_impl native runs the refinement as the device-resident safety filter (HIP only);
--rollout_impl native runs each batch of episodes as one native call (HIP only; with --no_refine
or --refine_impl native, not with --diagnose or --refine_space gains).
--a_max A limits every component of the applied action to [-A, A] (the nominal action is clamped,
the filter projects onto the box; not with --diagnose or --refine_space gains) and, like
--action_stats alone, adds limited_rate, intervention_rate, mean_abs_delta and max_abs_action.
--refine_coupling local runs the decentralised filter: every agent refines its own action against its
neighbours' nominal next states (not with --refine_space gains).
The controller is built as the checkpoint holds it: with the residual head where its last node layer
has 3D rows. --ctrl_residual asks for that head in a random-init evaluation; with a checkpoint that
holds a plain controller it is an error (not with --refine_space gains either).
"""
from __future__ import annotations

import argparse
import json
import os


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_agents", type=int, required=True)
    ap.add_argument("--model_path", type=str, default=None)
    ap.add_argument("--gpu", type=str, default=None)
    ap.add_argument("--num_envs", type=int, default=1)
    ap.add_argument("--episodes", type=int, default=None)
    ap.add_argument("--max_steps", type=int, default=None)
    ap.add_argument("--no_refine", action="store_true")
    ap.add_argument("--refine_loops", type=int, default=None)
    ap.add_argument("--refine_lr", type=float, default=None)
    ap.add_argument("--refine_space", choices=["actions", "gains"], default="actions")
    ap.add_argument("--diagnose", action="store_true")
    ap.add_argument("--device", type=str, default="auto")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dim", type=int, choices=[2, 3], default=2)
    ap.add_argument("--num_obstacles", type=int, default=0)
    ap.add_argument("--dtype", choices=["fp32", "bf16", "fp16"], default="fp32")
    ap.add_argument("--refine_impl", choices=["autograd", "native"], default="autograd")
    ap.add_argument("--rollout_impl", choices=["python", "native"], default="python")
    ap.add_argument("--a_max", type=float, default=None,
                    help="per-axis actuator limit |u| <= A on the applied action (default: none)")
    ap.add_argument("--action_stats", action="store_true",
                    help="report limited_rate, intervention_rate, mean_abs_delta and max_abs_action")
    ap.add_argument("--refine_coupling", choices=["joint", "local"], default="joint",
                    help="joint: the centralised filter; local: every agent refines its own action alone")
    ap.add_argument("--ctrl_residual", action="store_true",
                    help="random-init evaluation of a controller with the residual head (a checkpoint says it itself)")
    args = ap.parse_args(argv)
    if args.gpu is not None:
        os.environ.setdefault("HIP_VISIBLE_DEVICES", args.gpu)
    import torch
    from macbf_gnn_amd import config as C
    from macbf_gnn_amd.engine.trainer import resolve_device
    from macbf_gnn_amd.evaluate import EvalConfig, evaluate
    from macbf_gnn_amd.models import CBF, Controller
    from macbf_gnn_amd.utils import ckpt

    dev = resolve_device(args.device)
    torch.manual_seed(args.seed)
    if args.refine_impl == "native" and dev.type != "cuda":
        ap.error("--refine_impl native is the HIP safety filter and needs a HIP device; "
                 "use --refine_impl autograd with --device cpu")
    if args.model_path:
        ck_dim = ckpt.model_dim(args.model_path)
        if ck_dim is not None and ck_dim != args.dim:
            ap.error(f"checkpoint {args.model_path} holds {ck_dim}-D networks (CBF input width {2 * ck_dim + 2}) "
                     f"but --dim is {args.dim}; pass --dim {ck_dim}")
    residual = args.ctrl_residual
    if args.model_path:
        ck_res = ckpt.model_residual(args.model_path)
        if ck_res is not None:
            if args.ctrl_residual and not ck_res:
                ap.error(f"--ctrl_residual contradicts checkpoint {args.model_path}, whose controller has no residual "
                         f"head (controller_dec_net.6.weight has {2 * args.dim} rows); drop --ctrl_residual")
            residual = ck_res
    ctrl, cbf = Controller(2 * args.dim, residual=residual).to(dev), CBF(2 * args.dim).to(dev)
    if args.model_path:
        ckpt.load_models(args.model_path, ctrl, cbf)
    cfg = EvalConfig(num_agents=args.num_agents, num_envs=args.num_envs, seed=args.seed, refine=not args.no_refine,
                     refine_space=args.refine_space, diagnose=args.diagnose, dim=args.dim,
                     num_obstacles=args.num_obstacles, dtype=args.dtype, refine_impl=args.refine_impl,
                     rollout_impl=args.rollout_impl, a_max=args.a_max, action_stats=args.action_stats,
                     refine_coupling=args.refine_coupling)
    if args.episodes is not None:
        cfg.episodes = args.episodes
    if args.max_steps is not None:
        cfg.max_steps = args.max_steps
    if args.refine_loops is not None:
        cfg.refine_loops = args.refine_loops
    if args.refine_lr is not None:
        cfg.refine_lr = args.refine_lr
    try:
        out = evaluate(ctrl, cbf, cfg, device=dev)
    except ValueError as e:
        if not ((cfg.rollout_impl == "native" and "rollout_impl" in str(e)) or (cfg.a_max is not None and "a_max" in str(e)) or
                (residual and "ctrl_residual" in str(e)) or
                (cfg.refine_coupling != "joint" and "refine_coupling" in str(e))):
            raise
        ap.error(str(e))
    out.update({"num_agents": args.num_agents, "num_envs": args.num_envs, "episodes": cfg.episodes,
                "refine": cfg.refine, "device": str(dev), "dim": cfg.dim, "num_obstacles": cfg.num_obstacles,
                "refine_impl": cfg.refine_impl, "dtype": cfg.dtype})
    if cfg.rollout_impl != "python":
        out["rollout_impl"] = cfg.rollout_impl
    if cfg.a_max is not None:
        out["a_max"] = cfg.a_max
    if cfg.refine_coupling != "joint":
        out["refine_coupling"] = cfg.refine_coupling
    if residual:
        out["ctrl_residual"] = True
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
