"""Shared inputs of the controller node-backward oracle tests (tests/test_node_oracle_ref.py on the
CPU, tests/test_gpu_node_oracle.py on the device), built on the CPU from a seeded generator the way
ops.selfcheck._node_check builds its inputs: states from _synthetic_states, goals within +-0.5 of
the positions, pooled = rand * (rand > 0.3), A uniform in (-1, 1) -- deliberately NOT the recomputed
action --, Gn uniform in (-0.5, 0.5); default-initialised Controller weights.

The shapes are the smallest at which each indexing path of the four node bodies exists; the options
vary over the shapes so that every option meets every body (each case runs on every body)."""
import torch

from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.selfcheck import _synthetic_states

ACT_COEF = 0.37
A_MAX = 0.6
SLAB_FILL_MOD = 17          # init=False: slab pre-filled with ((index % 17) - 8) / 1024 (exact in fp32)

# B x N (x dim, Nn): what it reaches                                  | options
CASES = {
    # one 16-agent wave of node16, half a 32-row turn
    "1x16": dict(B=1, N=16, seed=3, init=True, act_cnt=None, gscale=None, valid=None, a_max=None, act_coef=ACT_COEF),
    # several env wraps inside one 16- / 32-agent group; a last group of 1
    "5x13": dict(B=5, N=13, seed=1, init=False, act_cnt=7.0, gscale=None, valid=2, a_max=None, act_coef=ACT_COEF),
    # second 128-chunk with one agent (one stage turn)
    "3x43": dict(B=3, N=43, seed=2, init=True, act_cnt=0.0, gscale=0.5, valid="ones", a_max=A_MAX, act_coef=ACT_COEF),
    # chunk remainder 97: four turns, the last with one agent
    "5x45": dict(B=5, N=45, seed=3, init=False, act_cnt=7.0, gscale=None, valid=1, a_max=A_MAX, act_coef=0.0),
    # three 128-chunks on two workgroups (one runs two chunks, the slab accumulates over them);
    # ten 32-chunks on three
    "1x300": dict(B=1, N=300, seed=4, init=True, act_cnt=7.0, gscale=0.5, valid=None, a_max=None, act_coef=ACT_COEF,
                  blocks={128: 2, 64: 2, 32: 3}),
    # 3-D records, s_env != N
    "2x40d3": dict(B=2, N=40, dim=3, Nn=48, seed=5, init=False, act_cnt=None, gscale=None, valid=0, a_max=A_MAX,
                   act_coef=ACT_COEF),
    # position independence: run as is and with the agents rolled by 37 positions
    "1x225": dict(B=1, N=225, seed=6, init=True, act_cnt=7.0, gscale=None, valid=None, a_max=A_MAX, act_coef=ACT_COEF),
    # the combine tests' node inputs (planted graphs of 24 agents; obstacle nodes: Nn = 29)
    "3x24": dict(B=3, N=24, seed=7, init=True, act_cnt=7.0, gscale=None, valid=None, a_max=None, act_coef=ACT_COEF),
    "3x24o": dict(B=3, N=24, Nn=29, seed=8, init=True, act_cnt=None, gscale=None, valid=1, a_max=A_MAX, act_coef=ACT_COEF),
    "3x24d3": dict(B=3, N=24, dim=3, Nn=29, seed=9, init=True, act_cnt=7.0, gscale=None, valid=None, a_max=None,
                   act_coef=ACT_COEF),
}
TABLE = ["1x16", "5x13", "3x43", "5x45", "1x300", "2x40d3"]
ALL = TABLE + ["1x225", "3x24", "3x24o", "3x24d3"]

# (id, chunk, 16x16x32 kernel)
BODIES = [("wave128", 128, False), ("wave64", 64, False), ("coop32", 32, False), ("node16", 128, True)]


def effective_coef(case) -> float:
    c = case["act_coef"]
    if case["act_cnt"] is not None:
        c = c / max(case["act_cnt"], 1.0)
    if case["gscale"] is not None:
        c = c * case["gscale"]
    return c


def blocks(case, chunk) -> int:
    """Workgroups of the launch: one per chunk unless the case pins fewer."""
    n = (case["B"] * case["N"] + chunk - 1) // chunk
    return case.get("blocks", {}).get(chunk, n)


def build(name, roll=0, zero_env=None):
    """CPU float32 inputs of case `name`: s (B, Nn, 2D) node states (agents first), G (B, N, D),
    A (B, N, D), Gn (B, N, 2D), pv (B, N, 128) pooled values, valid (B,) uint8 | None, and the case's
    options. roll: every per-agent input rolled by that many positions along the agents. zero_env:
    that env gets Gn = 0 (and must be the case's invalid env)."""
    case = dict(CASES[name])
    B, N, D = case["B"], case["N"], case.get("dim", 2)
    Nn = case.get("Nn", N)
    gen = torch.Generator().manual_seed(1000 + case["seed"])
    s = _synthetic_states(B, Nn, D, 1, gen, torch.device("cpu"))[0]
    G = s[:, :N, :D] + (torch.rand(B, N, D, generator=gen) - 0.5)
    A = (torch.rand(B, N, D, generator=gen) - 0.5) * 2.0
    Gn = torch.rand(B, N, 2 * D, generator=gen) - 0.5
    pv = torch.rand(B, N, 128, generator=gen) * (torch.rand(B, N, 128, generator=gen) > 0.3)
    valid = case["valid"]
    if valid == "ones":
        valid = torch.ones(B, dtype=torch.uint8)
    elif valid is not None:
        v = torch.ones(B, dtype=torch.uint8)
        v[valid] = 0
        valid = v
    if zero_env is not None:
        assert valid is not None and int(valid[zero_env]) == 0
        Gn[zero_env] = 0.0
    if roll:
        s = torch.cat([s[:, :N].roll(roll, 1), s[:, N:]], 1)
        G, A, Gn, pv = G.roll(roll, 1), A.roll(roll, 1), Gn.roll(roll, 1), pv.roll(roll, 1)
    case.update(name=name, D=D, Nn=Nn, s=s.contiguous(), G=G.contiguous(), A=A.contiguous(), Gn=Gn.contiguous(),
                pv=pv.contiguous(), valid=valid, c=effective_coef(case))
    return case


def split_pooled(pv, hdt, x3):
    """pooled values -> (hi, lo | None) in the kernels' 16-bit type (x3: hi + lo planes)."""
    hi = pv.to(hdt)
    return hi, ((pv - hi.float()).to(hdt) if x3 else None)


def controller(dim, seed=0):
    from macbf_gnn_amd.models import Controller
    torch.manual_seed(seed)
    return Controller(2 * dim)


def oracle_inputs(case, hi, lo):
    """The arguments of selfcheck.node_oracle after the parameters, from a built case."""
    return (hi, lo, native.to_records(case["s"]), case["G"], case["A"], native.to_records(case["Gn"]), case["valid"],
            case["c"], case["a_max"])


def slab_fill(rows, cols):
    i = torch.arange(rows * cols, dtype=torch.int64)
    return (((i % SLAB_FILL_MOD) - 8).float() / 1024.0).view(rows, cols)

