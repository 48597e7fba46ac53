"""Shared cases of the controller edge-backward oracle tests (tests/test_edge_bwd_ref.py on the CPU,
tests/test_gpu_edge_bwd_oracle.py on the device): the scenes of tests/ctrl_fwd_cases.py (2^-6 grid
coordinates, the five-agent radius plant cluster) at the neighbour counts where the 32x32x16 edge
backward (csrc/ctrl.hip edge_bwd_body) takes another path, plus a seeded upstream gradient
dP ~ N(0, 1) of shape (B, N, 128) per case.

The dense edge rows put row 32q + r of a 32-agent group on agent (32q + r) / K: a tile holds
ceil(32 / K) (+1 when straddling) agents, of which two lane-half passes (four agents) are prefetched
and the others loaded inside the tile (in effect K <= 9 except 8: agents per tile are 32, 16, 12, 8, 8,
6, 6, 4, 5, 4, 4, 4, .. for K = 1, 2, ..). The fused step (SPLIT) spreads the K tiles of a
group over four waves."""
import torch

import ctrl_fwd_cases as CC

# name: D, B, N, K, obstacles (12 points each), dens, seed. The scenes that tests/ctrl_fwd_cases.py
# already has are taken from there unchanged (same tensors, built once for both suites).
NEW = {
    # largest K whose tile fits the two prefetched passes (a tile spans at most 4 agents)
    "k11": dict(D=2, B=1, N=35, K=11, nobs=0, dens=1.75, seed=11),
    # the `K <= 10` branch without a trip: 32 q mod 10 is even, so no tile starts on an agent's last slot
    # and every tile spans 4 agents (the seeded defect that skips the loop leaves k10 green)
    "k10": dict(D=2, B=2, N=45, K=10, nobs=0, dens=1.75, seed=12),
    # the largest K whose tile spans 5 agents (tile 7 = rows 224..255 = agents 24..28): first trip of
    # the non-prefetched loop
    "k9": dict(D=2, B=2, N=41, K=9, nobs=0, dens=1.75, seed=16),
    # 3-D records, obstacle neighbours, odd K
    "k7d3": dict(D=3, B=2, N=20, K=7, nobs=1, dens=1.5, seed=13),
    # K < 4: SPLIT waves without any tile
    "k3": dict(D=2, B=4, N=11, K=3, nobs=0, dens=1.5, seed=14),
    # 16 agents per tile
    "k2": dict(D=2, B=2, N=33, K=2, nobs=0, dens=1.5, seed=15),
}
# k12: constant-K instantiation, env wrap inside a 32-agent group; k16: 2 agents per tile, aligned;
# k8: N < 32 (the division path of agent_bi), 4 agents per tile; k1: self edge only; k5: N = K;
# n300: three 128-agent chunks
SHARED = ("k12", "k16", "k8", "k1", "k5", "n300")
ALL = ["k12", "k16", "k11", "k10", "k9", "k8", "k7d3", "k3", "k2", "k1", "k5", "n300"]
SPECS = {n: (CC.CASES[n] if n in SHARED else NEW[n]) for n in ALL}
_CASES = {}


def build(name):
    """The scene of ctrl_fwd_cases.build_spec plus dP (B, N, 128) float32 (shared: read-only)."""
    if name not in _CASES:
        c = dict(CC.build_spec(name, SPECS[name]))
        gen = torch.Generator().manual_seed(9000 + c["seed"])
        c["dP"] = torch.randn(c["B"], c["N"], 128, generator=gen)
        _CASES[name] = c
    return _CASES[name]


def rolled(case, r):
    """ctrl_fwd_cases.rolled with the upstream gradient rolled along."""
    return dict(CC.rolled(case, r), dP=case["dP"].roll(r, 1))


def split_dP(dP, hdt, x3):
    """The upstream rows as the `hdt` build stores them: [hi | lo] planes (x3, 256 wide) or one
    rounding to the 16-bit type (128 wide)."""
    hi = dP.to(hdt)
    return torch.cat([hi, (dP - hi.float()).to(hdt)], -1) if x3 else hi
