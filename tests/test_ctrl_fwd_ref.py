"""The float64 reference of the controller forward (tests/ctrl_fwd_ref.py) pinned to
oracle.controller_forward, and the conditions the shared cases (tests/ctrl_fwd_cases.py) must meet
for the device tests' per-entry assertions to be decidable -- all from the reference alone, on the
CPU: every planted feature present, pool near-ties and zero-ambiguous entries rare, no radius tie
that is not planted."""
import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.ops import native

import ctrl_fwd_cases as CC
import ctrl_fwd_ref as R

NEAR_TIE_CAP = 0.02          # pool entries whose top two values are within 2 bnd (u = TAU)
ZERO_AMB_CAP = 0.01          # entries whose masked maximum pre-activation is within +-bnd of zero


def _ref(name, prec="fp32"):
    case = CC.build(name)
    p = R.kernel_params(CC.controller(case["D"]).params_dict(), prec)
    S = native.to_records(case["s"])
    ed = R.edge_phase(p, S, case["idx"], case["N"], prec)
    return case, p, S, ed, R.pooled_bound(ed, prec)


@pytest.mark.parametrize("name", CC.ALL)
def test_reference_equals_the_oracle_in_float64(name):
    case, p, S, ed, pb = _ref(name)
    N, D = case["N"], case["D"]
    s64, g64 = case["s"].double(), case["G"].double()
    a, aux = O.controller_forward(p, s64[:, :N], g64, case["idx"].long(), return_aux=True, nodes=s64)
    nd = R.node_phase(p, pb["top"], S, case["G"], "fp32")
    for got, want, nm in ((ed["hm"], aux["hm"], "hm"), (pb["top"], aux["pooled"], "pooled"), (nd["gains"], aux["gains"], "gains"),
                          (nd["a"], a, "a"), (ed["mask"], aux["mask"], "mask")):
        assert float((got - want).abs().max()) <= 1e-12, nm
    # the action bound at random initialisation: ~1e-3 of the row's sum of |terms| with u = TAU
    pos = nd["terms"] > 0
    worst = float((nd["da"][pos] / nd["terms"][pos]).max())
    print(f"BOUND {name}: da / terms <= {worst:.2e}")
    assert worst <= 5e-3


@pytest.mark.parametrize("name", CC.ALL)
def test_case_conditions(name):
    case, p, S, ed, pb = _ref(name)
    B, N, K = case["idx"].shape
    il = case["idx"].long()
    inr, rtie = ed["inr"], ed["rtie"]
    assert int(il.max()) < case["Nn"] and int(il.min()) >= 0
    assert case["B"] == B and case["N"] == N and case["K"] == K
    if case["M"]:
        assert int((il >= N).sum()) >= 50                       # obstacle neighbours j >= N
    # the agent at rest on its goal
    for b in range(B):
        r = int(case["rest"][b])
        assert torch.equal(case["s"][b, r, :case["D"]], case["G"][b, r]) and not bool(case["s"][b, r, case["D"]:].any())
    assert not bool((rtie & ~case["planted"]).any()), "a radius tie that is not planted"
    if case["plants"]:
        for b in range(B):
            P, Q, T, R1, R2 = (int(case[k][b]) for k in ("P", "Q", "T", "R1", "R2"))
            slot = lambda i, j: int((il[b, i] == j).nonzero()[0, 0]) if bool((il[b, i] == j).any()) else None
            for j in (Q, T, R1, R2):
                assert slot(P, j) is not None, (name, b, "planted neighbour not in the hub's list")
            # exactly at the radius and beside it: masks exact, d exact
            assert float(ed["d"][b, P, slot(P, Q)]) == 1.0 and not bool(inr[b, P, slot(P, Q)])
            assert float(ed["d"][b, P, slot(P, T)]) == CC.NEAR_OUT and not bool(inr[b, P, slot(P, T)])
            assert float(ed["d"][b, P, slot(P, R1)]) == CC.NEAR_IN and bool(inr[b, P, slot(P, R1)])
            for i in (Q, T):
                assert slot(i, P) is not None and not bool(inr[b, i, slot(i, P)])
                # isolated: only the self row is in radius
                assert int(inr[b, i].sum()) == 1 and int(il[b, i][inr[b, i]][0]) == i
            # duplicate neighbours: bit-identical records, j1 < j2, j2's slot flagged and later
            assert R1 < R2 and torch.equal(case["s"][b, R1], case["s"][b, R2])
            s1, s2 = slot(P, R1), slot(P, R2)
            assert s1 < s2 and bool(ed["dup"][b, P, s2]) and not bool(ed["dup"][b, P, s1])
            assert torch.equal(ed["hm"][b, P, s1], ed["hm"][b, P, s2]) and bool((ed["hm"][b, P, s1] > 0).any())
    elif K >= 2:
        raise AssertionError("every case with K >= 2 carries the plants")
    # only the planted duplicates are flagged
    want_dup = torch.zeros_like(ed["dup"])
    if case["plants"]:
        for b in range(B):
            P, R1, R2 = int(case["P"][b]), int(case["R1"][b]), int(case["R2"][b])
            want_dup[b, P] = il[b, P] == R2
    assert torch.equal(ed["dup"] & inr, want_dup & inr)
    near, amb = R.near_tie_fractions(ed, pb)
    frac_in = float(inr.double().mean())
    print(f"CASE {name}: in radius {frac_in:.2f}, pool near-ties {near:.4f}, zero-ambiguous {amb:.4f}, "
          f"255 entries {float((pb['top'] <= 0).double().mean()):.3f}")
    assert near <= NEAR_TIE_CAP and amb <= ZERO_AMB_CAP


def test_rolled_case_keeps_every_agent():
    case = CC.build("k12")
    rc = CC.rolled(case, 5)
    N = case["N"]
    assert torch.equal(rc["s"][:, :N].roll(-5, 1), case["s"][:, :N]) and torch.equal(rc["G"].roll(-5, 1), case["G"])
    a = O.edge_rel(case["s"][:, :N], case["idx"].long(), case["s"])
    b = O.edge_rel(rc["s"][:, :N], rc["idx"].long(), rc["s"])
    assert torch.equal(b[0].roll(-5, 1), a[0]) and torch.equal(b[1].roll(-5, 1), a[1])
