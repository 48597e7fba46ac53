"""The 32x32x16 controller edge backward (csrc/ctrl.hip edge_bwd_body: the production edge backward
of the bf16 / fp16 builds at every K and of the fp32 build at every K != 12, and the edge phase of the
fused ctrl_bwd_step) pinned, row by row, to the float64 oracle of the SAME inputs
(ops.selfcheck.edge_oracle; tests/test_edge_bwd_ref.py pins that oracle to autograd on the CPU).

The other backward tests reach this body through whole training steps at K = min(N, 12), per tensor.
Here native.ctrl_edge_bwd runs without the 16x16x32 images on the shared cases
(tests/edge_bwd_cases.py: K = 1, 2, 3, 5, 7, 8, 9, 10, 11, 12, 16; N < 32, N = K, 3-D records with obstacle
neighbours, 300 agents), with the tile split (qsplit) and the grid chosen by the test:

* inputs: the argmax slots of one native.ctrl_fwd call on the scene; S, idx, argmax, dP and dEc in
  allocations padded by 3 rows per env (five different env strides) -- S and dP NaN there, idx an id
  whose record is NaN, argmax slot 0, dEc a sentinel; the slab NaN (init) or pre-filled (accumulate).
  The launcher's shape check wants dense dP / dEc tensors, so ``_edge_call`` fills the argument
  struct through native._edge_bwd_kw and replaces those two pointers and strides.
* x3: no dEc row outside ROW_TOL |ref| + ABS_TOL |row scale| unless it is a flagged relu / radius tie
  (<= 3 % of a case's rows); weight gradients by test_gpu_oracle16._check_grads.
* 1-pass builds: the same with ABS_TOL + u on the row scale and 1e-4 + u on the weight gradients,
  u = 2^-8 (bf16) / 2^-11 (fp16): layer 1 is the hi / lo split (fp32-accurate), dZ is a copy of the
  stored dP, and d1 = W2^T dZ is rounded once to 16 bits (to_pk) before W1^T; H1 and d1 are each
  rounded once before the weight-gradient stages. One term the first device run added: the backward
  routes by the stored argmax and never looks at the sign of that slot's z2, the oracle applies its
  own float64 relu'(z2); the 1-pass forward resolves z2 only to ctrl_fwd_ref's e2, so a feature with
  |z2| <= e2 at its named slot may contribute wholly on one side only (``_forward_ambiguous``: that
  contribution is added to the row's bound; without it 1 row each of k10 / k7d3 / n300 bf16 was outside,
  at 1.34 - 3.44 of the bound). The weight-gradient rule gets the same features' share (their sum of |terms|,
  once: they are on one side only); without it k7d3-bf16 was at 5.88e-3 of the sum of |terms| of
  controller_centr_net.2.weight against 1e-4 + 2^-8 = 4.01e-3 (51 such features on 49 of 280 rows).
* tolerance-free: dEc bit-equal over qsplit 1 / 2 / 4 / 8 / 16 and over grids smaller and larger than
  the work; exact-zero slab rows of workgroups and parts without work; self rows exactly zero;
  rolling the agents leaves every agent's bits unchanged; the fused step's dEc bit-equal to the
  separate launch.

Measured err / bound ratios and tie counts: docs/PERF.md ("Edge backward oracle"). Reference ops:
controller.py:16-20,43-46 of the reference, differentiated by its train.py:103."""
import copy
import types

import pytest
import torch

from macbf_gnn_amd.models import CBF
from macbf_gnn_amd.ops import layout as L
from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.selfcheck import ABS_TOL, ROW_TOL, bad_rows, edge_oracle
from macbf_gnn_amd.ops.weights import PackedWeights
from macbf_gnn_amd.utils.params import FlatParams
from numerics import ratio_log, tie_log

import ctrl_fwd_cases as CC
import ctrl_fwd_ref as R
import edge_bwd_cases as EC
import node_cases as NC
import test_gpu_node_oracle as TN
from test_gpu_oracle16 import _check_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
PAD = CC.PAD
SENTINEL = 7.0
TIE_CAP = 0.03              # tests/test_edge_bwd_ref.py asserts it on the reference's own argmax
U = {"fp32": 0.0, **R.U16}
U24 = 2.0 ** -24
_NETS, _INPUTS, _REFS = {}, {}, {}

# rows that are flagged AND outside the row tolerance, counted on the first device run of each
# (case, precision) (profiles/edge_bwd_oracle/num.jsonl); the allowance is max(1, 2 x measured).
# Measured: 0 for every case, precision and fused-step case, so every allowance is 1.
EXEMPT = {}


def _nets(D, prec):
    """The shared default-initialised controller packed for `prec` -> (flat parameters, packed
    images, the parameters as that build's kernels receive them: float64 on the CPU, weight matrices
    and the layer-1 biases rounded to the 16-bit type in the 1-pass builds)."""
    if (D, prec) not in _NETS:
        ctrl = copy.deepcopy(CC.controller(D)).to(DEV)
        fp = FlatParams({"controller": ctrl, "cbf": CBF(2 * D).to(DEV)}, device=DEV)
        pw = PackedWeights(fp, D, DTYPES[prec])
        p = R.kernel_params({pn: fp.flat[o:o + n].view(shape) for m, pn, shape, o, n in fp.specs if m == "controller"}, prec)
        _NETS[(D, prec)] = (fp, pw, p)
    return _NETS[(D, prec)]


def _padded(t, fill, dtype=None):
    """(B, R, ...) CPU rows -> a (B, R + PAD, ...) device allocation filled with `fill`, rows copied;
    returns the (B, R, ...) view (env stride R + PAD rows)."""
    buf = torch.full((t.shape[0], t.shape[1] + PAD, *t.shape[2:]), fill, dtype=dtype or t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


def _inputs(case, prec, key):
    """Padded device inputs of a built case and the argmax slots of one ctrl_fwd call on it."""
    key = (key, prec)
    if key in _INPUTS:
        return _INPUTS[key]
    fp, pw, _ = _nets(case["D"], prec)
    B, N, D, Nn, K = case["B"], case["N"], case["D"], case["Nn"], case["K"]
    W, prow = native.rec_width(D), L.pooled_row(prec)
    S = _padded(native.to_records(case["s"]), float("nan"))
    idx = _padded(case["idx"], Nn + 1)                      # the padding names a NaN record of S
    am = _padded(torch.zeros(B, N, 128, dtype=torch.uint8), 0)
    hdt = torch.bfloat16 if prec == "fp32" else DTYPES[prec]
    dP = _padded(EC.split_dP(case["dP"], hdt, prec == "fp32"), float("nan"))
    native.ctrl_fwd(S, case["G"].to(DEV).contiguous(), case["idx"].to(DEV).contiguous(), pw.ctrl_w, pw.ctrl_off["ew1f"],
                    pw.ctrl_off["nw1f"], pw.ctrl_v, torch.zeros(B, N, D, device=DEV), torch.zeros(B, Nn, W, device=DEV), None, None,
                    pooled=torch.zeros(B, N, prow, dtype=pw.dtype, device=DEV), argmax=am, prec=prec)
    torch.cuda.synchronize()
    assert bool(((am < K) | (am == R.NONE)).all())
    _INPUTS[key] = dict(S=S, idx=idx, am=am, dP=dP, K=K, B=B, N=N, D=D, W=W, prow=prow)
    return _INPUTS[key]


def _reference(case, prec, key):
    """edge_oracle of the case on the kernel's argmax slots and stored dP rows, once per (case, precision)."""
    key = (key, prec)
    if key not in _REFS:
        _, _, p = _nets(case["D"], prec)
        inp = _inputs(case, prec, key[0])
        _REFS[key] = edge_oracle(p, native.to_records(case["s"]), case["idx"], inp["am"].cpu(), inp["dP"].cpu(), case["N"],
                                 case["D"], exact=case["planted"])
    return _REFS[key]


def chunks(total):
    return (total + 32 * native.CTRL_EDGE_WAVES - 1) // (32 * native.CTRL_EDGE_WAVES)


def _edge_call(inp, pw, prec, dEc, partial, num_blocks, init):
    """native.ctrl_edge_bwd's launch with dP / dEc views of padded allocations: the arguments are
    validated and filled by the launcher's own reader on dense stand-ins of the same shape, then the
    two pointers and env strides are replaced."""
    B, N, K, W, prow = inp["B"], inp["N"], inp["K"], inp["W"], inp["prow"]
    dP = inp["dP"]
    assert dP.stride(1) == prow and dP.stride(2) == 1 and dEc.stride(1) == K * W and dEc.stride(2) == W and dEc.stride(3) == 1
    kw, f16 = native._edge_bwd_kw(inp["S"], inp["idx"], inp["am"], torch.empty(B, N, prow, dtype=dP.dtype, device=DEV), pw.ctrl_w,
                                  pw.ctrl_off["ew1f"], pw.ctrl_off["ew2tn"], torch.empty(B, N, K, W, device=DEV), partial,
                                  num_blocks, prec=prec, init=init)
    kw.update(dP=native.ptr(dP), dp_env=dP.stride(0), dEc=native.ptr(dEc), de_env=dEc.stride(0) // W)
    native._ok(native.lib().ctrl_edge_bwd(num_blocks=int(num_blocks), prec=f16, stream=native.stream_handle(), **kw),
               "ctrl_edge_bwd")


def _run(case, prec, qsplit, monkeypatch, num_blocks=None, fill=None, key=None):
    """One 32x32x16 edge-backward launch -> raw dEc (B, N, K, W), the slab, the flat float64 weight
    gradient (slab minus fill, summed over the rows), the work count."""
    fp, pw, _ = _nets(case["D"], prec)
    inp = _inputs(case, prec, key or case["name"])
    B, N, K, W, D = inp["B"], inp["N"], inp["K"], inp["W"], inp["D"]
    monkeypatch.setattr(native, "ctrl_edge_qsplit", lambda total, device: qsplit)
    work = chunks(B * N) * qsplit
    nb = work if num_blocks is None else num_blocks
    dEb = torch.full((B, N + PAD, K, W), SENTINEL, device=DEV)
    slab = torch.full((nb, native.CTRL_EDGE_PARTIAL), float("nan"), device=DEV) if fill is None else fill.to(DEV).clone()
    _edge_call(inp, pw, prec, dEb[:, :N], slab, nb, init=fill is None)
    torch.cuda.synchronize()
    assert bool((dEb[:, N:] == SENTINEL).all()), "sentinel rows past an env's agents written"
    assert bool(torch.isfinite(slab).all()), "every slab row must be finite (init=True overwrites every row)"
    red = (slab.double() if fill is None else slab.double() - fill.to(DEV).double()).sum(0)
    return types.SimpleNamespace(dEc=dEb[:, :N].clone(), slab=slab, grad=_unpack(fp, D, red), work=work, nb=nb)


def _unpack(fp, D, red):
    offs = {pn: o for (m, pn, shape, o, n) in fp.specs}
    sm, dm = L.ctrl_edge_grad_map(offs, D)
    g = torch.zeros(fp.numel, dtype=torch.float64, device=red.device)
    g.index_add_(0, torch.as_tensor(dm, device=red.device), red[torch.as_tensor(sm, device=red.device)])
    return g.cpu()


def _forward_ambiguous(case, prec, key):
    """1-pass builds: the backward routes dP[f] to the stored argmax slot without looking at the sign
    of that slot's layer-2 pre-activation; the oracle multiplies by relu'(z2) of its own float64 z2.
    The 1-pass forward resolves z2 only to e2 (ctrl_fwd_ref.edge_phase: 2^-8 / 2^-11 of the layer's
    sum of |terms|, far wider than the TAU band of the tie flags), so where |z2| <= e2 at the named
    slot the feature's whole contribution |dP_f| |W2[f, :]| |W1| may be on either side. -> that sum
    per row (B N K, 2D), the number of such features, and their share of every weight gradient
    (dict): with dz2 = |dP_f| on the row of each such feature and dz1 = dz2 |W2| relu'(z1), the sums
    dz2^T |h1|, dz2, dz1^T |x|, dz1 over the rows, as selfcheck.abs_scales forms them."""
    _, _, p = _nets(case["D"], prec)
    inp = _inputs(case, prec, key)
    B, N, K, D = inp["B"], inp["N"], inp["K"], inp["D"]
    ed = R.edge_phase(p, native.to_records(case["s"]), case["idx"], N, prec)
    am = inp["am"].cpu().long()
    slot = am.clamp(max=K - 1)
    z2s = ed["z2"].gather(2, slot.unsqueeze(2)).squeeze(2)
    e2s = ed["e2"].gather(2, slot.unsqueeze(2)).squeeze(2)
    amb = (am < K) & (z2s.abs() <= e2s)
    w1 = p["controller_centr_net.0.weight"].reshape(64, -1)[:, :2 * D].abs()
    w2 = p["controller_centr_net.2.weight"].reshape(128, 64).abs()
    contrib = (inp["dP"].cpu().double()[..., :128].abs() * amb).unsqueeze(-1) * (w2 @ w1)          # (B, N, 128, 2D)
    out = torch.zeros(B, N, K, 2 * D, dtype=torch.float64)
    out.scatter_add_(2, slot.unsqueeze(-1).expand(-1, -1, -1, 2 * D), contrib)
    # the same features' share of the weight gradients
    s64 = case["s"].double()
    il = case["idx"].long()
    sj = torch.gather(s64, 1, il.reshape(B, -1, 1).expand(-1, -1, 2 * D)).reshape(B, N, K, 2 * D)
    eye = (il == torch.arange(N).view(1, N, 1)).double().unsqueeze(-1)
    x = torch.cat([s64[:, :N].unsqueeze(2) - sj, eye], -1).reshape(B * N * K, -1)
    W1 = p["controller_centr_net.0.weight"].reshape(64, -1)
    z1 = x @ W1.t() + p["controller_centr_net.0.bias"]
    dz2 = torch.zeros(B, N, K, 128, dtype=torch.float64)
    dz2.scatter_add_(2, slot.unsqueeze(2), (inp["dP"].cpu().double()[..., :128].abs() * amb).unsqueeze(2))
    dz2 = dz2.reshape(B * N * K, 128)
    dz1 = (dz2 @ w2) * (z1 > 0).double()
    share = {"controller_centr_net.2.weight": dz2.t() @ torch.relu(z1), "controller_centr_net.2.bias": dz2.sum(0),
             "controller_centr_net.0.weight": dz1.t() @ x.abs(), "controller_centr_net.0.bias": dz1.sum(0)}
    return out.reshape(-1, 2 * D), int(amb.sum()), share


def _contract(dEc, grad, ref, idx, fp, prec, what, key, extra=None, share=None):
    """The row and weight-gradient contract of one call (module docstring): dEc (B, N, K, W) raw
    records, grad the flat float64 slab sum, ref = edge_oracle's outputs, idx (B, N, K) CPU."""
    drel, tie, dws, scales, rscale = ref
    B, N, K = idx.shape
    u = U[prec]
    D2 = drel.shape[-1]
    got = native.from_records(dEc.cpu()).double().reshape(-1, D2)
    want, sc, t = drel.reshape(-1, D2), rscale.reshape(-1, D2), tie.reshape(-1)
    assert bool(torch.isfinite(got).all()), what
    err = (got - want).norm(dim=1)
    tol = ROW_TOL * want.norm(dim=1) + (ABS_TOL + u) * sc.norm(dim=1) + 1e-30
    if extra is not None:
        tol = tol + extra.norm(dim=1)
    over = err > tol
    if u == 0.0:
        bad, _ = bad_rows(got, want, t, sc)
        assert torch.equal(bad, over & ~t)
    ratio = float((err / tol)[~t].max()) if bool((~t).any()) else 0.0
    ratio_log(what, {"rows": ratio})
    assert int((over & ~t).sum()) == 0, (what, int((over & ~t).sum()), (over & ~t).nonzero().flatten().tolist()[:8], ratio)
    tie_log(what + " tie rows", int(t.sum()), t.numel(), int(TIE_CAP * t.numel()))
    assert int(t.sum()) <= TIE_CAP * t.numel(), (what, "tie rows", int(t.sum()), t.numel())
    tie_log(what + " exempt rows", int((over & t).sum()), t.numel(), max(1, 2 * EXEMPT.get(key, 0)))
    # self rows exactly zero (the whole record)
    selfm = idx.long() == torch.arange(N).view(1, N, 1)
    assert not bool(dEc.cpu()[selfm].ne(0).any()), (what, "a self row is not exactly zero")
    if u == 0.0:
        _check_grads(types.SimpleNamespace(fp=fp), grad, dws, scales, what + " dW")
    worst = 0.0
    for m, pn, shape, o, n in fp.specs:          # the same rule with 1e-4 + u (H1 and d1 are rounded once before the stages)
        if pn in dws and float(dws[pn].norm()) > 0:
            e = float((grad[o:o + n] - dws[pn].reshape(-1)).norm())
            sc_, st = float(scales[pn].norm()), float(scales[pn + "@tie"].norm())
            sa = float(share[pn].norm()) if share is not None else 0.0      # _forward_ambiguous: on one side only
            worst = max(worst, e / ((1e-4 + u) * sc_ + 2 * st + sa))
            assert e <= (1e-4 + u) * sc_ + 2 * st + sa, (what, pn, e / sc_, st / sc_, sa / sc_)
    ratio_log(what + " dW", {"dW": worst})


def no_tile_parts(K, qsplit):
    """Parts of a chunk whose tile range [part K / qsplit, (part + 1) K / qsplit) is empty."""
    return [p for p in range(qsplit) if (p + 1) * K // qsplit == p * K // qsplit]


def _zero_rows_expected(run, K, qsplit):
    """Slab rows that must be exactly zero after an init=True launch: workgroups beyond the work and,
    with one work item per workgroup, the parts without a tile."""
    rows = list(range(run.work, run.nb))
    if run.nb >= run.work:
        rows += [c * qsplit + p for c in range(run.work // qsplit) for p in no_tile_parts(K, qsplit)]
    return rows


# ----------------------------------------------------------------------------- a. x3 rows and slabs
@pytest.mark.parametrize("qsplit", [1, 16])
@pytest.mark.parametrize("name", EC.ALL)
def test_x3_edge_bwd_matches_fp64_oracle(name, qsplit, monkeypatch):
    case = EC.build(name)
    fp, _, _ = _nets(case["D"], "fp32")
    run = _run(case, "fp32", qsplit, monkeypatch)
    _contract(run.dEc, run.grad, _reference(case, "fp32", name), case["idx"], fp, "fp32", f"{name} fp32 q{qsplit}", (name, "fp32"))
    zr = _zero_rows_expected(run, case["K"], qsplit)
    assert not bool(run.slab[zr].ne(0).any()), "a part without a tile must write a zero slab row"
    if name == "k1":
        assert not bool(run.dEc.ne(0).any()), "K = 1: self edges only, every row exactly zero"
        assert float(run.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------ b. 1-pass rows
# rows whose bound _forward_ambiguous widens, counted on the first device run of each case
# (profiles/edge_bwd_oracle/num.jsonl); the allowance is the project's 2 x measured (numerics.tie_log)
WIDENED = {("k12", "bf16"): 38, ("k16", "bf16"): 38, ("k10", "bf16"): 52, ("k8", "bf16"): 17, ("k7d3", "bf16"): 49,
           ("n300", "bf16"): 156, ("k12", "fp16"): 4, ("k10", "fp16"): 5}
ONEPASS = [(n, "bf16") for n in ("k12", "k16", "k10", "k8", "k7d3", "n300")] + [(n, "fp16") for n in ("k12", "k10")]


@pytest.mark.parametrize("name,prec", ONEPASS, ids=[f"{n}-{p}" for n, p in ONEPASS])
def test_1pass_edge_bwd_matches_fp64_oracle(name, prec, monkeypatch):
    case = EC.build(name)
    fp, _, _ = _nets(case["D"], prec)
    run = _run(case, prec, 16, monkeypatch)
    extra, namb, share = _forward_ambiguous(case, prec, name)
    print(f"AMBIGUOUS {name} {prec}: {namb} features, {int(extra.ne(0).any(-1).sum())} rows of {extra.shape[0]}")
    tie_log(f"{name} {prec} q16 widened rows", int(extra.ne(0).any(-1).sum()), extra.shape[0], 2 * WIDENED[(name, prec)])
    _contract(run.dEc, run.grad, _reference(case, prec, name), case["idx"], fp, prec, f"{name} {prec} q16", (name, prec),
              extra=extra, share=share)


# ------------------------------------------------------------------ c. partition independence
@pytest.mark.parametrize("name", ["k12", "k10", "k3", "k1"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_partition_independence(prec, name, monkeypatch):
    """The tile split and the grid change which workgroup contracts which tile, never a row: the raw
    dEc buffers are identical; the slab sums differ by the fp32 summation order only, within
    n_rows 2^-24 sum |terms| per element (the 16-bit builds' terms carry two roundings: 1 + 4u)."""
    case = EC.build(name)
    fp, _, _ = _nets(case["D"], prec)
    K, n_rows = case["K"], case["idx"].numel()
    scales = _reference(case, prec, name)[3]
    base = _run(case, prec, 1, monkeypatch)
    assert bool(base.dEc.ne(SENTINEL).all())
    variants = [(q, None) for q in (2, 4, 8, 16)] + [(4, 1), (4, chunks(case["B"] * case["N"]) * 4 + 3), (1, 4)]
    for q, nb in variants:
        run = _run(case, prec, q, monkeypatch, num_blocks=nb)
        assert torch.equal(run.dEc.view(torch.int32), base.dEc.view(torch.int32)), (q, nb)
        for m, pn, shape, o, n in fp.specs:
            if pn in scales:
                # 1 + 4u: a kernel term is a product of two values each rounded once to 16 bits (H1 / d1 and
                # dZ / F), |term| <= (1 + u)^2 of the oracle's unrounded |term| that `scales` sums
                bound = n_rows * U24 * (1 + 4 * U[prec]) * scales[pn].reshape(-1)
                d = (run.grad[o:o + n] - base.grad[o:o + n]).abs()
                assert bool((d <= bound).all()), (q, nb, pn, float((d - bound).max()))
        zr = _zero_rows_expected(run, K, q)
        assert not bool(run.slab[zr].ne(0).any()), (q, nb, "a workgroup or part without work must write zeros")
        if q > K and nb is None:
            assert len(zr) == chunks(case["B"] * case["N"]) * (q - K)


def test_partition_independence_over_chunks(monkeypatch):
    """Three 128-agent chunks: one workgroup looping over all work items with live accumulators, and
    a grid larger than the work, give the bits of one workgroup per work item."""
    case = EC.build("n300")
    base = _run(case, "fp32", 2, monkeypatch)
    assert base.work == 6
    for nb in (1, 4, 9):
        run = _run(case, "fp32", 2, monkeypatch, num_blocks=nb)
        assert torch.equal(run.dEc.view(torch.int32), base.dEc.view(torch.int32)), nb
        assert not bool(run.slab[base.work:].ne(0).any())


# --------------------------------------------------------------------------------- d. accumulate
def test_accumulate_into_a_filled_slab(monkeypatch):
    case = EC.build("k10")
    fp, _, _ = _nets(2, "fp32")
    work = chunks(case["B"] * case["N"]) * 4
    fill = NC.slab_fill(work + 3, native.CTRL_EDGE_PARTIAL)
    run = _run(case, "fp32", 4, monkeypatch, num_blocks=work + 3, fill=fill)
    assert torch.equal(run.slab[work:].cpu(), fill[work:]), "workgroups without work must leave their rows"
    assert not torch.equal(run.slab[:work].cpu(), fill[:work])
    _contract(run.dEc, run.grad, _reference(case, "fp32", "k10"), case["idx"], fp, "fp32", "k10 fp32 q4 accumulate", ("k10", "fp32"))


# ------------------------------------------------------------------------ e. position independence
@pytest.mark.parametrize("name", ["k12", "k10", "k7d3"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_position_independence(prec, name, monkeypatch):
    """Rolling the agents of every env by 37 % N (idx remapped) puts every agent on another tile, lane
    half and dense-row phase and leaves its dEc bits unchanged."""
    case = EC.build(name)
    r = 37 % case["N"]
    base = _run(case, prec, 16, monkeypatch)
    roll = _run(EC.rolled(case, r), prec, 16, monkeypatch, key=name + "-rolled")
    assert not torch.equal(roll.dEc, base.dEc)
    same = roll.dEc.roll(-r, 1).view(torch.int32) == base.dEc.view(torch.int32)
    assert bool(same.all()), (~same).flatten(1).any(-1).nonzero().tolist()[:8]


# ---------------------------------------------------------------- f. the fused step's edge phase
FUSED = [("5x13", 1, "fp32"), ("5x13", 3, "fp32"), ("5x13", 8, "fp32"), ("5x13", 12, "fp32"), ("3x43", 10, "fp32"),
         ("3x43", 16, "fp32"), ("5x13", 3, "bf16"), ("5x13", 12, "bf16")]


@pytest.mark.parametrize("name,K,prec", FUSED, ids=[f"{n}-k{k}-{p}" for n, k, p in FUSED])
def test_fused_step_edge_phase(name, K, prec):
    """ctrl_bwd_step (SPLIT: the K tiles of a 32-agent group over four waves; waves without a tile in
    the last round, or in any with K < 4): its dEc and edge slab meet the contract above with the
    oracle fed the dP rows that this launch's node phase wrote, and its dEc is bit-equal to a separate
    ctrl_edge_bwd launch on those rows."""
    case = NC.build(name)
    fp, pw, p64 = TN._nets(case["D"], prec)
    B, N, D = case["B"], case["N"], case["D"]
    edge = TN._scene_edge(case, prec, K=K)
    nb = NC.blocks(case, 32)
    edge["partial"] = torch.full((nb, native.CTRL_EDGE_PARTIAL), float("nan"), device=DEV)
    edge["dEc"] = torch.full_like(edge["dEc"], SENTINEL)
    step = TN._launch(case, prec, 32, False, step_edge=edge)
    prow = L.pooled_row(prec)
    dP = step.dP_raw.view(B, N, prow)
    idx = edge["idx"].cpu()
    ref = edge_oracle(p64, edge["S"].cpu(), idx, edge["argmax"].cpu(), dP.cpu(), N, D)
    assert bool(torch.isfinite(edge["partial"]).all())
    grad = _unpack(fp, D, edge["partial"].double().sum(0))
    _contract(edge["dEc"], grad, ref, idx, fp, prec, f"fused {name} k{K} {prec}", ("fused", name, K, prec))
    if K == 1:
        assert not bool(edge["dEc"].ne(0).any())
    sep = torch.full_like(edge["dEc"], SENTINEL)
    nb2 = chunks(B * N) * native.ctrl_edge_qsplit(B * N, DEV)
    native.ctrl_edge_bwd(edge["S"], edge["idx"], edge["argmax"], dP.contiguous(), pw.ctrl_w, pw.ctrl_off["ew1f"],
                         pw.ctrl_off["ew2tn"], sep, torch.zeros(nb2, native.CTRL_EDGE_PARTIAL, device=DEV), nb2, prec=prec,
                         init=True)
    torch.cuda.synchronize()
    assert torch.equal(sep.view(torch.int32), edge["dEc"].view(torch.int32))
