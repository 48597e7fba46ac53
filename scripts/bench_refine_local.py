"""Time of one safety-filter call, joint against decentralised (docs/PERF.md, "Decentralised filter").

    python scripts/bench_refine_local.py [--model_path checkpoints/headline_4k.pt] [--rounds 7] [--calls 20]
                                         [--out FILE.json]

Shapes: 1024 agents x 4 envs in fp32 and 32 agents x 8 envs in bf16, 2-D, K = 12, the evaluation's
scenes (``ops.scenario.generate``) with the controller's actions, ``REFINE_LOOPS`` iterations at the
evaluation's step. Variants: the joint loop, the local loop and the local fused kernel, each a whole
``ops.refine.safety_filter`` call (``cbf_fwd`` for h(s_t), the reverse CSR where there is one, the
launches, and the torch glue around them). The variants are interleaved: every round times ``--calls``
back-to-back calls of each variant between two device events; reported are the minimum and the median
over the rounds of the time per call. One JSON line per shape.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {"joint_loop": dict(coupling="joint", impl="loop"), "local_loop": dict(coupling="local", impl="loop"),
            "local_fused": dict(coupling="local", impl="fused")}
SHAPES = [dict(num_agents=1024, num_envs=4, dtype="fp32"), dict(num_agents=32, num_envs=8, dtype="bf16")]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model_path", type=str, default="checkpoints/headline_4k.pt")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args(argv)
    import torch
    from macbf_gnn_amd import config as C
    from macbf_gnn_amd.evaluate import MFMA_DTYPES
    from macbf_gnn_amd.models import CBF, Controller
    from macbf_gnn_amd.ops import graph, scenario
    from macbf_gnn_amd.ops.refine import safety_filter
    from macbf_gnn_amd.utils import ckpt
    dev = torch.device("cuda")
    lines = []
    for shape in SHAPES:
        torch.manual_seed(0)
        ctrl, cbf = Controller(4).to(dev), CBF(4).to(dev)
        if a.model_path:
            ckpt.load_models(a.model_path, ctrl, cbf)
        ctrl.eval(), cbf.eval()
        ctrl.mfma_dtype = cbf.mfma_dtype = MFMA_DTYPES[shape["dtype"]]
        s, g, _ = scenario.generate(shape["num_envs"], shape["num_agents"], seed=7919, iteration=0, rank=0, device=dev)
        # a few controller steps in, where agents have met: the filter has work, as in an episode
        with torch.no_grad():
            for _ in range(8):
                idx = graph.knn(s, min(C.TOP_K, shape["num_agents"])).long()
                act = ctrl(s, g, idx=idx)
                s = s + torch.cat([s[..., 2:], act], -1) * C.TIME_STEP
            idx = graph.knn(s, min(C.TOP_K, shape["num_agents"])).long()
            act = ctrl(s, g, idx=idx)
        call = lambda kw: safety_filter(cbf, s, act, idx, **kw)
        used = {}
        for name, kw in VARIANTS.items():                  # warm-up: code objects, packing tables
            for _ in range(3):
                r = call(kw)
            used[name] = int(r[1])
        torch.cuda.synchronize()
        ms = {name: [] for name in VARIANTS}
        for _ in range(a.rounds):
            for name, kw in VARIANTS.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    call(kw)
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.calls)
        out = dict(shape, loops=C.REFINE_LOOPS, rounds=a.rounds, calls=a.calls, model_path=a.model_path, used=used,
                   ms_min={k: round(min(v), 4) for k, v in ms.items()},
                   ms_median={k: round(statistics.median(v), 4) for k, v in ms.items()},
                   ms_max={k: round(max(v), 4) for k, v in ms.items()})
        print(json.dumps(out), flush=True)
        lines.append(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
