"""CPU: the float64 references of tests/dedup_ref.py that pin cbf_dh / cbf_compact on the GPU
(tests/test_gpu_dedup_loss.py). The margin condition of every shared case is checked here, so a
seed that puts a hinge argument within fp32 rounding of zero is found without a GPU; the mapped
reference is checked against the oracle's loss on plain (h, h') tensors."""
import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.ops import native

import dedup_ref as R

CASES = [(s, rc, vp) for s in R.SHAPES for rc in (False, True) for vp in R.VALID_PATTERNS]


def _id(c):
    return "x".join(map(str, c[0])) + ("-rc" if c[1] else "-reuse") + "-" + c[2]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_case_margin_and_structure(case):
    shape, rc, vp = case
    c = R.make_case(*shape, R.case_seed(shape), rc, vp)            # asserts the margin condition
    T, B, N, K = shape
    E, U = c["E"], c["U"]
    bad, ties = R.margin_violations(c["h"], c["map1"], U)
    assert bad == 0
    assert ties[0] >= 1 and ties[1] >= 8 and ties[3] >= 1, ties
    args, hm, hn = R.hinge_args(c["h"], c["map1"], U)
    for a in args:
        assert bool(((a == 0) | (a.abs() >= R.MARGIN)).all())
    BNK = B * N * K
    if rc or T == 1:
        assert U == E + BNK                                        # only the last step has extras
    else:
        assert E + BNK < U < 2 * E                                 # some neighbour sets change
    assert bool((c["h"][c["hmask"] == 0] == 0).all())
    frac0 = 1.0 - float(c["hmask"][:U].float().mean())
    assert 0.03 < frac0 < 0.2
    assert 0.15 < float(c["dang"].float().mean()) < 0.45
    v = c["valid"]
    if vp == "none":
        assert v is None
    elif vp == "ones":
        assert bool(v.all())
    elif vp == "drop" and T > 1:
        t0 = max(1, T // 2)
        assert bool(v[:t0, 0].all()) and not bool(v[t0:, 0].any()) and bool(v[:, 1:].all())
    elif vp == "dead":
        assert not bool(v[:, B - 1].any()) and bool(v[:, :B - 1].all())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_mapped_reference_equals_oracle_loss_gradient(case, monkeypatch):
    """h and h' as independent tensors through oracle.cbf_loss_sums + finalize_losses (with the
    constants rounded to fp32 as the kernel receives them), gradients scattered through map1."""
    shape, rc, vp = case
    c = R.make_case(*shape, R.case_seed(shape), rc, vp)
    T, B, N, K = shape
    E, U = c["E"], c["U"]
    eps, dta = R.loss_consts64()[:2]
    monkeypatch.setattr(C, "LOSS_EPS_DANG", float(eps))
    monkeypatch.setattr(C, "TIME_STEP", float(dta))
    monkeypatch.setattr(C, "ALPHA_CBF", 1.0)
    m = c["map1"].reshape(-1)
    h64 = c["h"][:U].double()
    h = h64[:E].view(T, B, N, K).clone().requires_grad_(True)
    hn = h64[m].view(T, B, N, K).clone().requires_grad_(True)
    valid = torch.ones(T, B, dtype=torch.bool) if c["valid"] is None else c["valid"].bool()
    sums = O.cbf_loss_sums(h, hn, c["dang"], valid)
    fin = O.finalize_losses(sums, torch.zeros((), dtype=torch.float64), 1)
    fin["total"].backward()
    want = torch.zeros(U, dtype=torch.float64)
    want[:E] += h.grad.reshape(-1)
    want.index_add_(0, m, hn.grad.reshape(-1))
    counts = torch.stack([sums["n_dang"], sums["n_safe"]]).detach()
    ones = torch.ones_like(c["hmask"])
    dh, abs_terms, s8 = R.dh_reference(c["h"], ones, c["map1"], c["src"], U, c["dang"], c["valid"], counts)
    scale = float(want.abs().max()) if float(want.abs().max()) > 0 else 1.0
    assert float((dh - want).abs().max()) <= 1e-12 * scale
    for q, name in enumerate(R.SUM_NAMES):
        ref = sums[name].detach()
        assert float((s8[q] - ref).abs()) <= 1e-12 * max(1.0, float(ref.abs())), name
    # the mask, the scales and abs_terms
    dh2, abs2, _ = R.dh_reference(c["h"], c["hmask"], c["map1"], c["src"], U, c["dang"], c["valid"], counts,
                                  grad_scale=0.5, gscale=1024.0)
    assert float((dh2 - 512.0 * want * c["hmask"][:U].double()).abs().max()) <= 1e-12 * 512.0 * scale
    assert bool((abs_terms >= dh.abs() * (1 - 1e-12)).all())
    assert torch.allclose(abs2, 512.0 * abs_terms, rtol=1e-12, atol=0)


def test_drop_case_has_source_only_gradients():
    """The "drop" pattern does what it is for: evaluations whose own step is invalid but whose
    source slot's step is valid, with a nonzero h'-role gradient."""
    shape = R.SHAPES[0]
    c = R.make_case(*shape, R.case_seed(shape), False, "drop")
    T, B, N, K = shape
    E, U = c["E"], c["U"]
    ones = torch.ones_like(c["hmask"])
    dh, _, _ = R.dh_reference(c["h"], ones, c["map1"], c["src"], U, c["dang"], c["valid"], c["counts"])
    t0 = max(1, T // 2)
    own = torch.arange(E).view(T, B, N, K)[t0, 0].reshape(-1)      # main slots of the first invalid step
    assert bool((c["src"][own] >= 0).any())
    assert int((dh[own] != 0).sum()) > 0
    later = torch.arange(E).view(T, B, N, K)[t0 + 1:, 0].reshape(-1)
    assert bool((dh[later] == 0).all())


def test_compact_reference_by_hand():
    E, U = 4, 7
    dh = torch.tensor([0.0, 1.5, -0.0, -2.0, 0.25, 0.0, 3.0, 9.0])          # dh[7] lies beyond U
    src = torch.tensor([-1, -1, -1, -1, 2, 0, 3, 1])
    idx = torch.tensor([10, 11, 12, 13])
    idx1 = torch.tensor([20, 21, 22, 23])
    act, rec = R.compact_reference(dh, U, E, src, idx, idx1)
    assert act.tolist() == [1, 3, 4, 6]
    bits = dh.view(torch.int32)
    sign = -(1 << 31)
    assert rec.dtype == torch.int32 and rec.tolist() == [
        [1, 1, 11, int(bits[1])], [3, 3, 13, int(bits[3])], [4, 2 + sign, 22, int(bits[4])],
        [6, 3 + sign, 23, int(bits[6])]]
    _, rec0 = R.compact_reference(dh, U, E, src, idx, idx)
    assert rec0[:, 2].tolist() == [11, 13, 12, 13]
    assert (rec[:, 1] < 0).tolist() == [False, False, True, True]


def test_loss_consts_are_fp32_values():
    for c64, c in zip(R.loss_consts64(), native.LOSS_CONSTS):
        assert float(c64) == float(torch.tensor(c, dtype=torch.float32))
    assert R.span_of(1, 1) == 256 and R.span_of(257, 1) == 512 and R.span_of(2049, 7) == 512
