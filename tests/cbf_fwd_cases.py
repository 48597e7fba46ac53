"""Small shared cases of the CBF-forward oracle tests (tests/test_cbf_fwd_ref.py on the CPU,
tests/test_gpu_cbf_fwd_oracle.py on the device): CPU float32 trajectories S (T + 1, B, Nn, 2D), the kNN
lists of every step and three evaluation lists per case.

Step 0 is ctrl_fwd_cases._from_spec's scene (coordinates on the 2^-6 grid, random agents in a box that
starts at x = 5, a five-agent cluster left of it); every later step moves each random agent's position
and velocity by a seeded grid-rounded displacement of at most 2^-3 per coordinate, so the states stay on
the grid, differences of coordinates are exact and consecutive kNN lists differ in a few slots. The
cluster is re-planted for the CBF's own radius rule, d = sqrt(|dp|^2 + eps D) <= 1, which no pair on the
grid can meet with equality; P, Q and T keep their positions in every step (velocities still move):

    P = (0, 1, ..)            the hub; its planted-axis coordinate is 0, so p_P - p_j is exact
    Q = (x_in, 1, ..)         x_in the largest fp32 x whose fp32 d is <= 1.0f (bisection on the bit pattern)
    T = (-x_out, 1, ..)       x_out = nextafter(x_in, inf): d > 1.0f, the adjacent bit pattern
    R1 = R2 = (0, 1.5, ..)    two nodes with bit-identical records: the hub's two slots have identical
                              features and must have identical h bits; the pair swings to x = -+2^-4 on
                              odd / even later steps, which flips the order of Q and T in its lists

Evaluation lists (``lists``), as cbf_hfwd receives them -- idx the kNN lists of steps 0 .. T - 1:

    "match"   cbf_match's own reference (ops/dedup.py match_reference), reuse mode: idx1 is idx
    "recomp"  the recomputed mode: idx1 = kNN of s_{t+1}, the extras are the last step's slots
    "plant"   extras at a seeded subset of slots in non-monotone slot order, U - E no multiple of 32,
              idx1 = kNN of s_{t+1}

In all three src[:E] and src[U:] hold wrong but valid slot numbers (a kernel that reads them computes a
wrong value, never an out-of-range address)."""
import functools
import struct

import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.ops.dedup import match_reference

import ctrl_fwd_cases as CC

GRID = CC.GRID
PAD = 3                     # NaN records after every env, NaN records after every step, of the padded S
STEP_MOVE = 2.0 ** -3
MODES = ("match", "recomp", "plant")

# name: D, B, N, K, obstacle sets (12 points each), dens, seed, T
CASES = {
    "k1": dict(D=2, B=3, N=9, K=1, nobs=0, dens=1.5, seed=4, T=2),
    "k5": dict(D=2, B=2, N=5, K=5, nobs=0, dens=1.5, seed=5, T=3),          # N = K: the cluster alone
    "k8": dict(D=2, B=3, N=13, K=8, nobs=0, dens=1.5, seed=3, T=2),
    "k12": dict(D=2, B=2, N=40, K=12, nobs=0, dens=1.75, seed=1, T=3),
    "k16": dict(D=2, B=2, N=37, K=16, nobs=0, dens=1.75, seed=2, T=2),
    "3d_obs": dict(D=3, B=2, N=33, K=12, nobs=2, dens=1.5, seed=6, T=2),    # idx >= N: obstacle neighbours
    "n300": dict(D=2, B=1, N=300, K=12, nobs=0, dens=2.0, seed=7, T=2),
}
ALL = list(CASES)


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def _from_bits(n):
    return struct.unpack("<f", struct.pack("<i", n))[0]


def d32(x, D):
    """The kernels' fp32 d of a pair whose relative position is (x, 0, ..) -> python float."""
    t = torch.tensor(x, dtype=torch.float32)
    sq = t * t
    for _ in range(1, D):
        sq = sq + torch.zeros((), dtype=torch.float32)
    return float(torch.sqrt(sq + torch.tensor(C.CBF_DIST_EPS_COORD * D, dtype=torch.float32)))


@functools.lru_cache(maxsize=None)
def radius_edge(D):
    """(x_in, x_out): adjacent positive fp32 values with d32(x_in) <= 1.0 < d32(x_out); d32 is monotone
    in the bit pattern, found by bisection."""
    lo, hi = _bits(0.5), _bits(1.0)
    assert d32(0.5, D) <= 1.0 < d32(1.0, D)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if d32(_from_bits(mid), D) <= 1.0:
            lo = mid
        else:
            hi = mid
    return _from_bits(lo), _from_bits(hi)


@functools.lru_cache(maxsize=None)
def cbf(D, seed=0):
    """Default-initialised CBF of a D-dimensional scene (shared: treat as read-only)."""
    from macbf_gnn_amd.models import CBF
    torch.manual_seed(200 + seed)
    return CBF(2 * D)


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict of CPU tensors (shared: treat as read-only): S (T + 1, B, Nn, 2D) fp32, idx (T, B, N, K)
    int32 = kNN of steps 0 .. T - 1, idx_next (T, B, N, K) = kNN of steps 1 .. T, the plants P, Q, Tt,
    R1 < R2 (B,) or None, and the spec's fields."""
    c = dict(CASES[name])
    D, B, N, K, T = c["D"], c["B"], c["N"], c["K"], c["T"]
    base = CC._from_spec(name, {k: v for k, v in c.items() if k != "T"})
    s0 = base["s"].clone()
    Nn = base["Nn"]
    plants = base["plants"]
    fixed = torch.zeros(B, Nn, dtype=torch.bool)
    fixed[:, N:] = True                                            # obstacle points are static
    if plants:
        x_in, x_out = radius_edge(D)
        for b in range(B):
            P, Q, Tt, R1, R2 = (int(base[k][b]) for k in ("P", "Q", "T", "R1", "R2"))
            pos = torch.ones(5, D)
            pos[0, 0] = 0.0
            pos[1, 0] = x_in
            pos[2, 0] = -x_out
            pos[3, 0] = pos[4, 0] = 0.0
            pos[3, 1] = pos[4, 1] = 1.5
            for n, a in enumerate((P, Q, Tt, R1, R2)):
                s0[b, a, :D] = pos[n]
                fixed[b, a] = True
            s0[b, R2] = s0[b, R1]
    gen = torch.Generator().manual_seed(9000 + c["seed"])
    steps = [s0]
    for t in range(1, T + 1):
        mv = torch.round((torch.rand(B, Nn, 2 * D, generator=gen) * 2 - 1) * STEP_MOVE * GRID) / GRID
        mv[..., :D][fixed] = 0.0                                   # the cluster keeps its positions,
        mv[:, N:] = 0.0                                            # obstacle points their zero velocity too
        nxt = steps[-1] + mv
        if plants:
            # the duplicate pair swings across the hub's axis (x = -+2^-4 on odd / even steps), so the
            # order of Q and T in its lists flips from step to step: idx_next != idx even with N = K
            for b in range(B):
                R1, R2 = int(base["R1"][b]), int(base["R2"][b])
                nxt[b, R1, 0] = -2.0 ** -4 if t % 2 else 2.0 ** -4
                nxt[b, R2] = nxt[b, R1]
        steps.append(nxt)
    S = torch.stack(steps)
    knn = torch.stack([O.knn_idx(S[t, :, :N], K, S[t]) for t in range(T + 1)]).to(torch.int32)
    out = dict(c, name=name, Nn=Nn, M=base["M"], S=S, idx=knn[:T].contiguous(), idx_next=knn[1:].contiguous(), plants=plants)
    if plants:
        out.update(P=base["P"], Q=base["Q"], Tt=base["T"], R1=base["R1"], R2=base["R2"])
    return out


def _wrong_slots(n, E, gen):
    return torch.randint(0, E, (n,), generator=gen)


@functools.lru_cache(maxsize=None)
def lists(name, mode):
    """-> dict: idx1 (T, B, N, K) int32 (the SAME tensor as idx in "match"), src (2E,) int32, U, E, and
    the clean extras `extras` (U - E,) int64 (the slots the extras name)."""
    case = build(name)
    idx = case["idx"]
    T, B, N, K = idx.shape
    E = idx.numel()
    BNK = B * N * K
    gen = torch.Generator().manual_seed(500 + case["seed"] + 17 * MODES.index(mode))
    if mode == "match":
        _, src_ref, U = match_reference(idx, T, recomputed=False)
        extras = src_ref[E:U].clone()
        idx1 = idx
    elif mode == "recomp":
        extras = torch.arange((T - 1) * BNK, E)
        idx1 = case["idx_next"]
    else:
        n = max(1, E // 3)
        if n % 32 == 0:
            n += 5
        extras = torch.randperm(E, generator=gen)[:n]               # non-monotone slot order
        idx1 = case["idx_next"]
    U = E + extras.numel()
    assert int(extras.min()) >= 0 and int(extras.max()) < E
    src = torch.empty(2 * E, dtype=torch.long)
    src[:E] = (torch.arange(E) + 1 + _wrong_slots(E, max(E - 1, 1), gen)) % E        # never the slot itself (E > 1)
    src[E:U] = extras
    src[U:] = _wrong_slots(2 * E - U, E, gen)
    return dict(idx1=idx1, src=src.to(torch.int32), U=U, E=E, extras=extras, mode=mode)


def rolled(case, r):
    """The case with the agents of every env rolled by r positions in every step (agent i -> i + r mod
    N), the kNN lists renumbered: every slot keeps its pair and lands on another lane / tile."""
    N = case["N"]

    def ridx(ix):
        j = ix.long()
        return torch.where(j < N, (j + r) % N, j).roll(r, 2).to(torch.int32).contiguous()

    S = case["S"]
    S2 = torch.cat([S[:, :, :N].roll(r, 2), S[:, :, N:]], 2)
    return dict(case, S=S2, idx=ridx(case["idx"]), idx_next=ridx(case["idx_next"]))


def roll_slot_map(case, r):
    """(E,) int64: main slot e of the case -> the slot of the same (t, b, agent, k) in rolled(case, r)."""
    T, B, N, K = case["idx"].shape
    e = torch.arange(T * B * N * K)
    k, i, tb = e % K, (e // K) % N, e // (K * N)
    return (tb * N + (i + r) % N) * K + k


# the safety-filter cases of tests/test_gpu_refine.py whose forward at s' the oracle test checks:
# name -> (dim, obstacle sets, N, B, seed), the same tuples and the same construction as its _inputs
FILTER_CASES = {"2d_tail": (2, 0, 40, 2, 3), "3d_obs2": (3, 2, 40, 2, 5), "3d_obs1_n33": (3, 1, 33, 3, 11)}


@functools.lru_cache(maxsize=None)
def filter_inputs(name):
    """-> (cbf module, s (B, N, 2D), a (B, N, D), idx (B, N, K) int64, obs (B, M, D) or None), CPU."""
    from macbf_gnn_amd import env as E
    from macbf_gnn_amd.models import CBF
    dim, nobs, N, B, seed = FILTER_CASES[name]
    s, _, obs = E.generate_scenarios(B, N, dim, nobs, seed)
    torch.manual_seed(seed)
    net = CBF(2 * dim)
    s = s.clone()
    s[..., dim:] = torch.randn(B, N, dim) * 0.5
    a = torch.randn(B, N, dim) * 2.0
    idx = O.knn_idx(s, min(12, N), O.with_obstacles(s, obs))
    return net, s, a, idx, obs
