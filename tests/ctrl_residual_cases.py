"""Shared inputs of the residual-head tests (tests/test_ctrl_residual.py on the CPU,
tests/test_gpu_ctrl_residual_{fwd,bwd}.py on the device).

The controllers: a default-initialised ``Controller(2D, residual=True)`` whose residual rows (zero at
construction) are drawn the way ``nn.Linear`` initialises the gain rows -- uniform in +-1/sqrt(fan_in),
weight and bias alike --, and its plain twin: a ``Controller(2D)`` holding the same other parameters.

The scenes are built by the shared builders of the plain tests (tests/ctrl_fwd_cases.py,
tests/node_cases.py) from entries of this module's own tables; an entry is in the builder's table only for
the duration of its build, so what the plain tests see does not depend on this module."""
import copy
import functools
from unittest import mock

import torch

import ctrl_fwd_cases as CC
import node_cases as NC
from macbf_gnn_amd.models import Controller

# ---- forward scenes (the issue's cases). The 2-D ones are the plain tests' own cases; the 3-D ones are
#      entries of this module, built by ctrl_fwd_cases.build while they sit in its table and taken out again
FWD_CASES = {
    # 3-D, one obstacle (12 points): rows 6, 7 and 8 of the last layer; 33 agents: a second group of 1
    "res_3d_n33_o1": dict(D=3, B=2, N=33, K=12, nobs=1, dens=1.5, seed=11),
    # 3-D, two obstacles, 40 agents
    "res_3d_n40_o2": dict(D=3, B=2, N=40, K=12, nobs=2, dens=1.5, seed=12),
}
FWD = {"n40": "k12", "n300": "n300", "n5": "k5", "3d_n33_o1": "res_3d_n33_o1", "3d_n40_o2": "res_3d_n40_o2"}
FWD_ALL = list(FWD)


@functools.lru_cache(maxsize=None)
def fwd_case(name):
    """The built case (shared: treat as read-only). ctrl_fwd_cases' table is what it was when this returns."""
    key = FWD[name]
    if key not in FWD_CASES:
        return CC.build(key)
    with mock.patch.dict(CC.CASES, {key: FWD_CASES[key]}):
        return CC.build.__wrapped__(key)          # (not through their cache: nothing of ours stays behind)


# ---- node-backward inputs: the options vary over the shapes of the issue's table
A, M = NC.ACT_COEF, NC.A_MAX
NODE_CASES = {
    # node16: one 16-agent wave
    "res1x16": dict(B=1, N=16, seed=21, init=True, act_cnt=None, gscale=None, valid=None, a_max=None, act_coef=A),
    # node16: three 128-chunks on two workgroups
    "res1x300": dict(B=1, N=300, seed=22, init=True, act_cnt=7.0, gscale=0.5, valid=None, a_max=M, act_coef=A,
                     blocks={128: 2}),
    # 3-D (row 8), s_env != N: node16 and the cooperative body
    "res1x33d3": dict(B=1, N=33, dim=3, Nn=45, seed=23, init=False, act_cnt=None, gscale=None, valid=None, a_max=M,
                      act_coef=A),
    # per-wave chunks of 128 and 64: 200 agents, one env off, the slab accumulated over two chunks
    "res2x100": dict(B=2, N=100, seed=24, init=False, act_cnt=7.0, gscale=None, valid=1, a_max=None, act_coef=A,
                     blocks={64: 2}),
    # cooperative 32: 40 agents, one env off, no action loss
    "res2x20": dict(B=2, N=20, seed=25, init=True, act_cnt=7.0, gscale=None, valid=0, a_max=M, act_coef=0.0),
    # 9 agents per env: K = 9, the fused step's runtime-K instantiation (ctrl_bwd_step_res_kernel<D, 0>)
    "res3x9": dict(B=3, N=9, seed=27, init=True, act_cnt=None, gscale=None, valid=None, a_max=M, act_coef=A),
    "res3x9d3": dict(B=3, N=9, dim=3, seed=28, init=False, act_cnt=7.0, gscale=None, valid=None, a_max=None,
                     act_coef=A),
    # the only env off (with Gn = 0: everything exactly zero), 3-D
    "res1x24d3off": dict(B=1, N=24, dim=3, seed=26, init=True, act_cnt=None, gscale=None, valid=0, a_max=None,
                         act_coef=A),
}
NODE_ALL = ["res1x16", "res1x300", "res1x33d3", "res2x100", "res2x20", "res3x9", "res3x9d3"]
# (case, body id, chunk, 16x16x32 kernel): the issue's table, and the K = 9 scenes on the cooperative body
NODE_RUNS = [("res1x16", "node16", 128, True), ("res1x300", "node16", 128, True), ("res1x33d3", "node16", 128, True),
             ("res2x100", "wave128", 128, False), ("res2x100", "wave64", 64, False),
             ("res2x20", "coop32", 32, False), ("res1x33d3", "coop32", 32, False),
             ("res3x9", "coop32", 32, False), ("res3x9d3", "coop32", 32, False)]
# every option is in the table
_cs = [NODE_CASES[n] for n in NODE_ALL]
assert {c["init"] for c in _cs} == {True, False}
assert any(isinstance(c["valid"], int) for c in _cs) and any(c["valid"] is None for c in _cs)
assert {M, None} <= {c["a_max"] for c in _cs}
assert any(c["act_coef"] == 0.0 for c in _cs) and any(c["act_coef"] != 0.0 for c in _cs)


def node_case(name, **kw):
    """node_cases.build on an entry of this module; node_cases' table is what it was when this returns."""
    with mock.patch.dict(NC.CASES, {name: NODE_CASES[name]}):
        return NC.build(name, **kw)


# ---- controllers (shared: treat as read-only)
@functools.lru_cache(maxsize=None)
def controller(D, randomise=True, seed=0):
    torch.manual_seed(100 + seed)
    c = Controller(2 * D, residual=True)
    if randomise:
        gen = torch.Generator().manual_seed(4000 + 10 * D + seed)
        lin = c.controller_dec_net[6]
        bound = 1.0 / lin.in_features ** 0.5
        with torch.no_grad():
            lin.weight[2 * D:] = (torch.rand(D, lin.in_features, generator=gen) * 2.0 - 1.0) * bound
            lin.bias[2 * D:] = (torch.rand(D, generator=gen) * 2.0 - 1.0) * bound
    return c


def plain_twin(res):
    """Controller(2D) with the residual controller's other parameters (its gain rows included)."""
    D = res.in_dim // 2
    c = Controller(2 * D)
    sd = copy.deepcopy(res.state_dict())
    sd["controller_dec_net.6.weight"] = sd["controller_dec_net.6.weight"][:2 * D].clone()
    sd["controller_dec_net.6.bias"] = sd["controller_dec_net.6.bias"][:2 * D].clone()
    c.load_state_dict(sd)
    return c


def randomise_trainer(tr, seed=0):
    """Draw the residual rows of a trainer's (zero-initialised) residual head as ``controller`` does, in the
    flat master parameters, and repack: the step under test then has a residual that acts."""
    D = tr.cfg.dim
    gen = torch.Generator().manual_seed(5000 + seed)
    spec = {pn: (o, shape) for m, pn, shape, o, n in tr.fp.specs if m == "controller"}
    with torch.no_grad():
        for pn in ("controller_dec_net.6.weight", "controller_dec_net.6.bias"):
            o, shape = spec[pn]
            assert shape[0] == 3 * D, "the trainer's controller has no residual head"
            cols = 64 if len(shape) == 2 else 1
            rows = (torch.rand(D * cols, generator=gen) * 2.0 - 1.0) / 8.0
            tr.fp.flat[o + 2 * D * cols:o + 3 * D * cols] = rows.to(tr.fp.flat.device)
    tr.engine.after_update()
