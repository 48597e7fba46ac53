"""Multi-rank RCCL data parallelism: one rank per device (VERDICT r3 missing #2).

Runs `world = min(8, device_count)` (rounded down to a power of two) ranks over the `nccl`
backend (RCCL on ROCm, xGMI inside the node), rank r on device r, and checks:

* every rank is on a distinct physical device;
* the reduced gradient is bit-identical on every rank and equals the single-process gradient
  on the concatenated env batch (the joint update of /root/reference/train.py:101-105 over the
  global batch; slab partitions differ, so fp32 summation order only: rtol 2e-3);
* after 3 full training steps (own sampling per rank, all-reduce, Adam) the parameters are
  bit-identical across ranks.

Skips on a one-GPU box; it runs on the first 8-GPU node. The bench launcher's fail-fast and
gloo-rehearsal paths on one GPU are checked below as well.
"""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

from macbf_gnn_amd import config as C
from macbf_gnn_amd import env as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BTOT, N, T = 8, 64, 8


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _world():
    n = min(8, torch.cuda.device_count())
    w = 1
    while w * 2 <= n:
        w *= 2
    return w


def _cfg(B):
    return C.TrainConfig(num_agents=N, num_envs=B, inner_loops=T, device="hip", seed=7, early_stop=True)


def _worker(rank, world, port, outdir):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                       "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank)})
    import torch.distributed as dist
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    dev = torch.device("cuda", rank)
    torch.cuda.set_device(dev)
    dp = DP(device=dev)
    assert dist.get_backend() == "nccl" and dp.world == world
    props = torch.cuda.get_device_properties(dev)
    uid = str(getattr(props, "uuid", "") or "") or str(getattr(props, "pci_bus_id", rank))
    s_all, g_all = E.generate_batch(BTOT, N, seed=31)
    B = BTOT // world
    tr = Trainer(_cfg(B), device=dev, dp=dp)
    sl = slice(rank * B, (rank + 1) * B)
    tr.engine.step(s_all[sl].to(dev), g_all[sl].to(dev))
    tr.reduce_grad()
    grad = tr.fp.grad.cpu()
    for _ in range(3):
        tr.train_step()
    dp.barrier()
    torch.cuda.synchronize()
    torch.save({"grad": grad, "flat": tr.fp.flat.cpu(), "uid": uid, "dev": dev.index},
               os.path.join(outdir, f"r{rank}.pt"))
    dp.shutdown()


@pytest.mark.timeout(600)
def test_rccl_multirank_grad_and_params():
    world = _world()
    if world < 2:
        pytest.skip("needs >= 2 HIP devices (one RCCL rank per device)")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        mp.start_processes(_worker, args=(world, _free_port(), d), nprocs=world, join=True, start_method="spawn")
        outs = [torch.load(os.path.join(d, f"r{r}.pt"), weights_only=True) for r in range(world)]
    assert len({o["uid"] for o in outs}) == world, [o["uid"] for o in outs]
    assert [o["dev"] for o in outs] == list(range(world))
    for o in outs[1:]:
        assert torch.equal(o["grad"], outs[0]["grad"])
        assert torch.equal(o["flat"], outs[0]["flat"])
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    dev = torch.device("cuda", 0)
    s_all, g_all = E.generate_batch(BTOT, N, seed=31)
    tr = Trainer(_cfg(BTOT), device=dev, dp=DP(device=dev))
    tr.engine.step(s_all.to(dev), g_all.to(dev))
    ref = tr.fp.grad.cpu()
    assert torch.isfinite(ref).all() and ref.abs().sum() > 0
    torch.testing.assert_close(outs[0]["grad"], ref, rtol=2e-3, atol=1e-6)


def _bench(args, env_extra):
    env = dict(os.environ, **env_extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=240)


@pytest.mark.timeout(300)
def test_bench_gpus_beyond_devices_fails_fast():
    n = torch.cuda.device_count() + 1
    r = _bench(["--gpus", str(n), "--steps", "1", "--warmup", "0"], {"MACBF_DP_BACKEND": ""})
    assert r.returncode != 0 and f"needs {n} HIP devices" in r.stderr, r.stderr[-1500:]


@pytest.mark.timeout(300)
def test_bench_gpus2_gloo_rehearsal_on_one_device():
    r = _bench(["--gpus", "2", "--agents", "64", "--envs", "2", "--steps", "2", "--warmup", "1",
                "--inner_loops", "8"], {"MACBF_DP_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["world"] == 2 and out["dp_backend"] == "gloo"
    assert out["shared_devices"] and len(out["device_ids"]) == 2


@pytest.mark.timeout(300)
def test_bench_dump_outputs_is_the_last_timed_step(tmp_path):
    """--dump-outputs writes what train_step left after warmup + steps iterations. The same
    iterations run here on one trainer (one code path, one seed: only the order of float
    accumulation may differ) give the same gradient within the bound of the fp32 gradient tests,
    and parameters at least 10x closer to the dump than those one Adam step earlier."""
    import numpy as np
    from macbf_gnn_amd.engine import Trainer
    r = _bench(["--gpus", "1", "--agents", "64", "--envs", "2", "--steps", "2", "--warmup", "1", "--inner_loops", "8",
                "--dump-outputs", str(tmp_path)], {})
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["grad", "params", "stats"]
    assert got["params"].dtype == got["grad"].dtype == np.float32 and got["stats"].dtype == np.float64
    tr = Trainer(C.TrainConfig(num_agents=64, num_envs=2, inner_loops=8, seed=0, device="hip",
                               display_steps=10 ** 9, save_steps=10 ** 9))
    for _ in range(2):
        tr.train_step()
    before = tr.fp.flat.double().cpu().numpy()
    st = tr.train_step()
    torch.cuda.synchronize()
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))
    e_p = rel(got["params"], tr.fp.flat.double().cpu().numpy())
    e_b = rel(got["params"], before)
    e_g = rel(got["grad"], tr.fp.grad.double().cpu().numpy())
    print(f"dump vs in-process: params {e_p:.3g} (one step earlier {e_b:.3g}) grad {e_g:.3g}")
    assert np.isfinite(got["grad"]).all() and np.abs(got["grad"]).max() > 0
    assert e_g <= 1e-3
    assert e_b > 0 and e_p <= 0.1 * e_b
    assert got["stats"][12] == st["agent_steps"] and got["stats"][14] == st["T"]
