"""The per-env active mask of the safety filter (csrc/refine.hip, ``env_active``): a masked batch
equals, bit for bit, the filter run on the active sub-batch alone; masked-out envs keep their
actions; all ones equals no mask, control words included; all zeros changes nothing.

Shapes: the smallest at which 32-edge tiles straddle envs -- 100 edges per env in 2-D (N = K = 10)
and 144 in 3-D with obstacle points (N = K = 12), B = 3. Inputs are built on the host as in
tests/test_gpu_refine.py; the seeds give every env some dozens of edges with a non-zero hinge
gradient at the first iteration (CPU oracle: 72 / 82 / 69 and 41 / 42 / 32), which the tests assert
from the unmasked filter on each env alone."""
import copy
import functools

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import env as E
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.models import CBF
from macbf_gnn_amd.ops import graph, native
from macbf_gnn_amd.ops.packing import module_pack
from macbf_gnn_amd.ops.refine import safety_filter

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# name -> (dim, obstacles, N, seed); B = 3, K = N
CASES = {"2d": (2, 0, 10, 5), "3d_obs": (3, 1, 12, 5)}
B = 3
LOOPS = 4
LR = C.REFINE_LEARNING_RATE
MASKS = {"101": (1, 0, 1), "010": (0, 1, 0), "111": (1, 1, 1), "000": (0, 0, 0)}
ALL = [(n, p) for n in CASES for p in ("fp32", "bf16")]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    dim, nobs, N, seed = CASES[name]
    s, _, obs = E.generate_scenarios(B, N, dim, nobs, seed)
    torch.manual_seed(seed)
    cbf = CBF(2 * dim)
    s = s.clone()
    s[..., dim:] = torch.randn(B, N, dim) * 0.5
    a = torch.randn(B, N, dim) * 2.0
    idx = O.knn_idx(s, min(12, N), O.with_obstacles(s, obs))
    assert idx.shape[-1] == N and (N * N) % 32 != 0              # tiles straddle envs
    return cbf, s.to(DEV), a.to(DEV), idx.to(DEV), (None if obs is None else obs.to(DEV))


@functools.lru_cache(maxsize=None)
def _module(name, prec):
    cbf = copy.deepcopy(_inputs(name)[0]).to(DEV)
    with torch.no_grad():
        if prec == "bf16":
            cbf.mfma_dtype = torch.bfloat16
            for p in cbf.parameters():
                p.copy_(p.bfloat16().float())
    return cbf


def _mask(bits, dtype=torch.bool):
    return torch.tensor(bits, dtype=dtype, device=DEV)


def _run(name, prec, env_active=None, sel=None, **kw):
    """safety_filter on the batch (``sel`` None) or on the envs ``sel`` of it alone -> (a, used, viol, trace)."""
    _, s, a, idx, obs = _inputs(name)
    if sel is not None:
        s, a, idx = s[sel], a[sel], idx[sel]
        obs = None if obs is None else obs[sel]
    return safety_filter(_module(name, prec), s, a, idx, obstacles=obs, loops=LOOPS, lr=LR, return_trace=True,
                         env_active=env_active, **kw)


@functools.lru_cache(maxsize=None)
def _alone(name, prec, bits):
    """The unmasked filter on the envs with a 1 in ``bits`` alone: the reference, computed once."""
    sel = torch.tensor([i for i, b in enumerate(bits) if b], device=DEV)
    out = _run(name, prec, sel=sel)
    torch.cuda.synchronize()
    return sel, out


def _assert_precondition(name, prec):
    """Every env, kept or masked out, has work at the first iteration: otherwise a mask shows nothing."""
    for e in range(B):
        bits = tuple(int(i == e) for i in range(B))
        _, (_, used, _, tr) = _alone(name, prec, bits)
        assert int(tr["counts"][0]) > 0 and int(used) > 0, (name, prec, e, tr["counts"].tolist())


def _assert_equals_sub_batch(name, prec, bits, got):
    a = _inputs(name)[2]
    ar, used, viol, tr = got
    sel, (ar_ref, used_ref, viol_ref, tr_ref) = _alone(name, prec, bits)
    off = torch.tensor([i for i, b in enumerate(bits) if not b], device=DEV)
    assert torch.equal(ar[sel], ar_ref)
    assert not torch.equal(ar_ref, a[sel])                        # the filter did move the kept envs
    assert int(used) == int(used_ref) and torch.equal(viol, viol_ref)
    assert torch.equal(tr["counts"], tr_ref["counts"]), (tr["counts"].tolist(), tr_ref["counts"].tolist())
    assert torch.equal(tr["hn"][sel], tr_ref["hn"]) and torch.equal(tr["active"][sel], tr_ref["active"])
    assert torch.equal(ar[off], a[off])                           # masked-out envs: the inputs, bit for bit
    assert not bool(tr["active"][off].any()) and not bool(tr["hn"][off].any())   # and no trace written


@pytest.mark.parametrize("bits", ["101", "010"])
@pytest.mark.parametrize("name,prec", ALL)
def test_masked_batch_equals_the_active_sub_batch(name, prec, bits):
    _assert_precondition(name, prec)
    m = MASKS[bits]
    _assert_equals_sub_batch(name, prec, m, _run(name, prec, env_active=_mask(m)))


@pytest.mark.parametrize("name,prec", [("2d", "fp32"), ("3d_obs", "bf16")])
def test_uint8_mask_and_one_workgroup(name, prec):
    """num_blocks = 1: one workgroup walks live and skipped tiles alike (10 / 14 tiles over 4 / 8
    waves, so a wave meets a skipped tile and hands its prefetch on); the mask given as uint8."""
    _assert_precondition(name, prec)
    for bits in ("101", "010"):
        m = MASKS[bits]
        got = _run(name, prec, env_active=_mask(m, torch.uint8), num_blocks=1)
        _assert_equals_sub_batch(name, prec, m, got)


def _raw(name, prec, env_active, loops=LOOPS):
    """native.refine itself -> (delta, ctl, dEv): every control word, not only what safety_filter reads."""
    _, s, a, idx, obs = _inputs(name)
    cbf = _module(name, prec)
    _, N, D = a.shape
    K = idx.shape[-1]
    mp = module_pack("cbf", cbf, DEV)
    w, v, rm = mp.pack(list(cbf.parameters()))
    S = graph.node_records(s, obs)
    Nn = S.shape[1]
    idx32 = idx.to(torch.int32).contiguous()
    h = torch.empty(1, B, N, K, device=DEV)
    native.cbf_fwd(S.view(1, *S.shape), idx32.view(1, B, N, K), w, mp.off["w1f"], v, two=False, h_out=h, prec=mp.prec)
    rptr = torch.empty(B, Nn + 1, dtype=torch.int32, device=DEV)
    redges = torch.empty(B, N * K, dtype=torch.int32, device=DEV)
    native.rev_csr(idx32, rptr, redges, n_nodes=Nn)
    delta = torch.zeros(B, N, D, device=DEV)
    ctl = torch.full((2 * loops,), -1, dtype=torch.int64, device=DEV)        # the driver clears it
    dEv = torch.full((B, N, K, D), 7.0, device=DEV)
    native.refine(S, idx32, a.contiguous(), delta, h.view(B, N, K), w, mp.off["w1f"], rm, v, dEv, rptr, redges, ctl,
                  loops=loops, lr=LR, prec=mp.prec, env_active=env_active)
    return delta, ctl, dEv


@pytest.mark.parametrize("name,prec", ALL)
def test_all_ones_equals_no_mask(name, prec):
    a0, u0, v0, t0 = _run(name, prec)
    a1, u1, v1, t1 = _run(name, prec, env_active=_mask(MASKS["111"]))
    assert torch.equal(a0, a1) and int(u0) == int(u1) and torch.equal(v0, v1)
    assert torch.equal(t0["counts"], t1["counts"]) and int(t0["counts"][0]) > 0
    assert torch.equal(t0["hn"], t1["hn"]) and torch.equal(t0["active"], t1["active"])
    d0, c0, e0 = _raw(name, prec, None)
    d1, c1, e1 = _raw(name, prec, _mask(MASKS["111"]))
    assert torch.equal(c0, c1) and int(c0[0]) > 0 and int(c0[1]) > 0          # ctl, every word
    assert torch.equal(d0, d1) and torch.equal(e0, e1)


@pytest.mark.parametrize("name,prec", ALL)
def test_all_zeros_leaves_everything_unchanged(name, prec):
    a = _inputs(name)[2]
    ar, used, viol, tr = _run(name, prec, env_active=_mask(MASKS["000"]))
    assert torch.equal(ar, a) and int(used) == 0 and float(viol) == 0.0
    assert not bool(tr["counts"].any()) and not bool(tr["active"].any()) and not bool(tr["hn"].any())
    delta, ctl, dEv = _raw(name, prec, _mask(MASKS["000"]))
    assert not bool(delta.any()) and not bool(ctl.any())
    assert bool((dEv == 7.0).all())                                           # no edge record written


def test_masked_filter_does_not_synchronise():
    """The mask is read by the kernels: with one given, safety_filter still never waits for the GPU."""
    name, prec = "3d_obs", "fp32"
    _, s, a, idx, obs = _inputs(name)
    cbf = _module(name, prec)
    m = _mask(MASKS["101"])
    safety_filter(cbf, s, a, idx, obstacles=obs, loops=2, lr=LR, env_active=m)   # packing tables are built once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ar, used, viol = safety_filter(cbf, s, a, idx, obstacles=obs, loops=LOOPS, lr=LR, env_active=m)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert used.is_cuda and viol.is_cuda
    assert 0 < int(used) <= LOOPS and torch.equal(ar[1], a[1])


@pytest.mark.parametrize("what", ["dtype", "shape", "host"])
def test_mask_argument_validation(what):
    name, prec = "2d", "fp32"
    bad = {"dtype": torch.ones(B, dtype=torch.int32, device=DEV),
           "shape": torch.ones(B + 1, dtype=torch.bool, device=DEV),
           "host": torch.ones(B, dtype=torch.bool)}[what]
    with pytest.raises(native.NativeError):
        _run(name, prec, env_active=bad)
