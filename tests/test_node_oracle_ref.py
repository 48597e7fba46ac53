"""CPU: ops.selfcheck.node_oracle (the float64 contract of one controller node-backward call) against
autograd through oracle.controller_forward, and the conditions the device test
(tests/test_gpu_node_oracle.py) relies on, checked on the reference alone for every shared case.

The comparison graph is idx = self (K = 1) with pool_values= a leaf and A = a: the only edge is
s_i - s_i = 0, so the edge path has zero derivative in s and dP / ego / the dec-net gradients of the
node contract must equal dL/dpool_values, dL/ds and the parameter gradients of
dt Gn_v . (m a) + c valid action_loss_terms. Reference op: controller.py:47-61 and
core.py:174-184 of the reference."""
import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.selfcheck import node_oracle

import node_cases as NC

TIE_CAP = 0.08              # tie rows per case (the device test exempts flagged rows; measured 0-6.2 %)
SIGN_MARGIN = 1e-4          # | |A|^2 - |a_ref|^2 | >= SIGN_MARGIN (|A|^2 + |a_ref|^2): the sign is unambiguous in fp32
LIMIT_MARGIN = 1e-6         # every |A_q| at least this far from a_max


def _dec_params(ctrl):
    return {k: v.detach().double() for k, v in ctrl.params_dict().items()}


@pytest.mark.parametrize("name", NC.ALL)
def test_node_oracle_matches_controller_autograd(name):
    case = NC.build(name)
    B, N, D = case["B"], case["N"], case["D"]
    p64 = _dec_params(NC.controller(D))
    p = {k: v.clone().requires_grad_(True) for k, v in p64.items()}
    s = case["s"][:, :N].double().requires_grad_(True)
    g = case["G"].double()
    pool = case["pv"].double().requires_grad_(True)
    idx = torch.arange(N).view(1, N, 1).expand(B, N, 1)
    a = O.controller_forward(p, s, g, idx, pool_values=pool)
    A = a.detach()
    m = torch.ones_like(A) if not case["a_max"] else ((A >= -case["a_max"]) & (A <= case["a_max"])).double()
    vb = torch.ones(B, dtype=torch.float64) if case["valid"] is None else case["valid"].double()
    gnv = case["Gn"].double()[..., D:]
    loss = (C.TIME_STEP * gnv * m * a).sum() + (case["c"] * vb.view(B, 1) * O.action_loss_terms(s, g, a)).sum()
    names = [k for k in p if k.startswith("controller_dec_net")]
    ref = torch.autograd.grad(loss, [pool, s] + [p[k] for k in names])
    dP, ego, dw, tie, scales, psc, esc = node_oracle(p64, case["pv"], None, native.to_records(case["s"]), case["G"], A,
                                                      native.to_records(case["Gn"]), case["valid"], case["c"],
                                                      case["a_max"])
    n = B * N

    def close(got, want, what):
        bound = 1e-6 * float(want.abs().max())
        assert float((got - want).abs().max()) <= bound, (what, float((got - want).abs().max()), bound)

    close(dP, ref[0].reshape(n, 128), "dP")
    close(ego, ref[1].reshape(n, 2 * D), "ego")
    for k, r in zip(names, ref[2:]):
        close(dw[k], r, k)
        assert scales[k].shape == r.shape and bool((scales[k] + 1e-300 >= r.abs()).all()), k   # sum |terms| >= |sum terms|
        assert bool((scales[k + "@tie"] <= scales[k]).all())
    assert dP.shape == psc.shape and ego.shape == esc.shape and tie.shape == (n,)
    assert bool((psc + 1e-300 >= dP.abs()).all()) and bool((esc * (1 + 1e-12) + 1e-300 >= ego.abs()).all())


@pytest.mark.parametrize("name", NC.ALL)
def test_case_conditions(name):
    """What the device test takes for granted, on the float64 reference: few tie rows, an unambiguous
    action-loss sign, and raw actions clear of the actuator limit with both sides populated."""
    case = NC.build(name)
    D = case["D"]
    hi, lo = NC.split_pooled(case["pv"], torch.bfloat16, True)
    p64 = _dec_params(NC.controller(D))
    tie = node_oracle(p64, *NC.oracle_inputs(case, hi, lo))[3]
    frac = float(tie.double().mean())
    print(f"CASE {name}: tie rows {int(tie.sum())}/{tie.numel()}")
    assert frac <= TIE_CAP, (name, int(tie.sum()), tie.numel())
    s, A = case["s"][:, :case["N"]].double(), case["A"].double()
    ar = O.action_ref(s, case["G"].double())
    a2, r2 = (A * A).sum(-1), (ar * ar).sum(-1)
    margin = float(((a2 - r2).abs() / (a2 + r2)).min())
    print(f"CASE {name}: min sign margin {margin:.3e}")
    assert margin >= SIGN_MARGIN, (name, margin)
    if case["a_max"]:
        gap = float((A.abs() - case["a_max"]).abs().min())
        masked = float((A.abs() > case["a_max"]).double().mean())
        print(f"CASE {name}: limit gap {gap:.3e}, masked {masked:.3f}")
        assert gap >= LIMIT_MARGIN and 0.1 <= masked <= 0.9, (name, gap, masked)


def test_every_option_is_in_the_table():
    cs = [NC.CASES[n] for n in NC.TABLE]
    assert {c["init"] for c in cs} == {True, False}
    assert {7.0, 0.0, None} <= {c["act_cnt"] for c in cs}
    assert {0.5, None} <= {c["gscale"] for c in cs}
    assert any(isinstance(c["valid"], int) for c in cs) and any(c["valid"] is None for c in cs)
    assert {NC.A_MAX, None} <= {c["a_max"] for c in cs}
    assert any(c["act_coef"] == 0.0 for c in cs) and any(c["act_coef"] != 0.0 for c in cs)


def test_rolled_case_is_a_permutation():
    a, b = NC.build("1x225"), NC.build("1x225", roll=37)
    for k in ("G", "A", "Gn", "pv"):
        assert torch.equal(a[k].roll(37, 1), b[k])
    assert torch.equal(a["s"][:, :225].roll(37, 1), b["s"][:, :225])
