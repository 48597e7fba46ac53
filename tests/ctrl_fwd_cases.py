"""Small shared cases of the controller-forward oracle tests (tests/test_ctrl_fwd_ref.py on the CPU,
tests/test_gpu_ctrl_fwd_oracle.py on the device): CPU float32 inputs from seeded generators, every
coordinate on a 2^-6 grid (so differences of coordinates, the radius plants and the duplicate
records are exact in fp32 and in float64 alike).

A case is a random scene -- positions uniform in a box of side L = (N_random / 8)^(1/D) * dens next
to the plants, so that a good part of the listed neighbours is in radius -- plus, with N >= 5, a
five-agent plant cluster per env, more than one radius away from every random agent:

    P              the hub
    Q = P + (1, 0, ..)                 a pair EXACTLY at the radius: masked (strict <), asserted exactly
    T = P - (1 + 2^-19, 0, ..)         beside the radius, outside: masked
    R1 = R2 = P + (0, 1 - 2^-20, ..)   beside the radius, inside; two nodes j1 < j2 with bit-identical records:
                                       the first occurrence wins every feature, j2's slot never appears
    Q and T                            isolated agents: every other listed neighbour is out of radius, their
                                       pooled rows come from the self row alone

and one agent at rest on its goal (p == g, v == 0: its action is exactly +-0). The cluster's agents
sit at seeded random indices of the env, so they fall on different waves, lanes and dense-row phases.
idx is oracle.knn_idx of the planted fp32 state (stable: ties by the lower node index)."""
import functools

import torch

from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.models import Controller

GRID = 64.0                 # coordinates are multiples of 2^-6
NEAR_IN = 1.0 - 2.0 ** -20
NEAR_OUT = 1.0 + 2.0 ** -19
PAD = 3                     # NaN records / sentinel rows after every env of the padded buffers

# name: D, B, N, K, obstacles (12 points each), dens, seed
CASES = {
    # env stride padded by 3 NaN records; second 32-agent group partial; waves straddle envs
    "k12": dict(D=2, B=2, N=40, K=12, nobs=0, dens=1.75, seed=1),
    # every slot of the 16-slot tile live
    "k16": dict(D=2, B=2, N=37, K=16, nobs=0, dens=1.75, seed=2),
    # N > K, K < 12
    "k8": dict(D=2, B=3, N=13, K=8, nobs=0, dens=1.5, seed=3),
    # self edge only
    "k1": dict(D=2, B=3, N=9, K=1, nobs=0, dens=1.5, seed=4),
    # N = K: the plant cluster alone
    "k5": dict(D=2, B=2, N=5, K=5, nobs=0, dens=1.5, seed=5),
    # 3-D records, obstacle neighbours j >= N
    "3d_obs": dict(D=3, B=2, N=33, K=12, nobs=2, dens=1.5, seed=6),
    # ten 32-agent groups
    "n300": dict(D=2, B=1, N=300, K=12, nobs=0, dens=2.0, seed=7),
}
ALL = list(CASES)


def _grid(x):
    return torch.round(x * GRID) / GRID


@functools.lru_cache(maxsize=None)
def controller(D, seed=0):
    """Default-initialised controller of a D-dimensional scene (shared: treat as read-only)."""
    torch.manual_seed(100 + seed)
    return Controller(2 * D)


@functools.lru_cache(maxsize=None)
def build(name):
    """The shared case `name` of CASES, built once (see _from_spec)."""
    return _from_spec(name, CASES[name])


_SPEC_BUILT = {}


def build_spec(name, spec):
    """A case from a spec dict in the form of CASES' entries, built once per (name, spec); a name of
    CASES with that entry's spec is build(name) itself."""
    if CASES.get(name) == spec:
        return build(name)
    key = (name, tuple(sorted(spec.items())))
    if key not in _SPEC_BUILT:
        _SPEC_BUILT[key] = _from_spec(name, spec)
    return _SPEC_BUILT[key]


def _from_spec(name, spec):
    """spec: dict(D, B, N, K, nobs, dens, seed) -> dict of CPU tensors (shared between tests: treat
    as read-only): s (B, Nn, 2D) node states (agents first, obstacle points after with zero
    velocity), G (B, N, D), idx (B, N, K) int32, and the plants: per env the agent indices P, Q, T,
    R1 < R2 and `rest`; planted (B, N, K) bool = the edges whose radius mask is planted and exact."""
    c = dict(spec)
    D, B, N, K, nobs = c["D"], c["B"], c["N"], c["K"], c["nobs"]
    gen = torch.Generator().manual_seed(7000 + c["seed"])
    plants = N >= 5 and K >= 2                 # (K = 1 lists the self edge only: nothing to plant)
    Nr = N - 5 if plants else N
    M = 12 * nobs
    L = max(1.0, Nr / 8.0) ** (1.0 / D) * c["dens"]
    p = torch.zeros(B, N, D)
    v = _grid((torch.rand(B, N, D, generator=gen) - 0.5) * 1.2)
    cl = torch.zeros(B, 5, dtype=torch.long)
    rnd = torch.zeros(B, max(Nr, 0), dtype=torch.long)
    for b in range(B):
        perm = torch.randperm(N, generator=gen)
        if plants:
            five = perm[:5].clone()
            five[3:] = five[3:].sort().values                    # R1 < R2
            cl[b] = five
        rnd[b] = perm[5:] if plants else perm
    # random agents: the box [5, 5 + L] x [0, L]^(D-1); the cluster around P = (2, 1, ..): every random
    # agent is >= 2 away from Q = (3, 1, ..), farther from the others
    if Nr:
        pr = _grid(torch.rand(B, Nr, D, generator=gen) * L)
        pr[..., 0] += 5.0
        p.scatter_(1, rnd.unsqueeze(-1).expand(-1, -1, D), pr)
    out = dict(c, name=name, Nn=N + M, M=M, L=L)
    if plants:
        base = torch.full((D,), 1.0)
        base[0] = 2.0
        off = torch.zeros(5, D)
        off[1, 0] = 1.0
        off[2, 0] = -NEAR_OUT
        off[3, 1] = NEAR_IN
        off[4, 1] = NEAR_IN
        for b in range(B):
            p[b, cl[b]] = base + off
            v[b, cl[b, 4]] = v[b, cl[b, 3]]                      # bit-identical records
        out.update(P=cl[:, 0], Q=cl[:, 1], T=cl[:, 2], R1=cl[:, 3], R2=cl[:, 4])
    G = _grid(p + (torch.rand(B, N, D, generator=gen) - 0.5))
    rest = rnd[:, 0] if Nr else (cl[:, 1] if plants else torch.zeros(B, dtype=torch.long))
    for b in range(B):
        v[b, rest[b]] = 0.0
        G[b, rest[b]] = p[b, rest[b]]
    s = torch.cat([p, v], -1)
    if M:
        # obstacles: 12 grid points within +-0.25 of a centre inside the random box
        ctr = torch.rand(B, nobs, 1, D, generator=gen) * L
        ctr[..., 0] += 5.0
        pts = _grid(ctr + (torch.rand(B, nobs, 12, D, generator=gen) - 0.5) * 0.5).reshape(B, M, D)
        s = torch.cat([s, torch.cat([pts, torch.zeros(B, M, D)], -1)], 1)
    idx = O.knn_idx(s[:, :N], K, s).to(torch.int32)
    planted = torch.zeros(B, N, K, dtype=torch.bool)
    if plants:
        il = idx.long()
        for b in range(B):
            P, Q, T, R1, R2 = cl[b].tolist()
            for i, js in ((P, (Q, T, R1, R2)), (Q, (P,)), (T, (P,)), (R1, (P,)), (R2, (P,))):
                for j in js:
                    planted[b, i] |= il[b, i] == j
    out.update(s=s, G=G, idx=idx, rest=rest, planted=planted, plants=plants)
    return out


def rolled(case, r):
    """The case with the agents of every env rolled by r positions (agent i -> i + r mod N), idx
    remapped: every agent keeps its inputs and its list order and lands on another lane / row phase."""
    B, N, K = case["idx"].shape
    s, idx = case["s"], case["idx"].long()
    s2 = torch.cat([s[:, :N].roll(r, 1), s[:, N:]], 1)
    j2 = torch.where(idx < N, (idx + r) % N, idx)
    return dict(case, s=s2, G=case["G"].roll(r, 1), idx=j2.roll(r, 1).to(torch.int32), planted=case["planted"].roll(r, 1),
                rest=(case["rest"] + r) % N)
