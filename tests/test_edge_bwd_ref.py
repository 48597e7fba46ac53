"""CPU: ops.selfcheck.edge_oracle (the float64 contract of one controller edge-backward call) against
autograd through oracle.controller_forward's edge MLP and max-pool, and the conditions the device
test (tests/test_gpu_edge_bwd_oracle.py) relies on, checked on the reference alone for every shared
case (tests/edge_bwd_cases.py): few tie rows, non-zero rows to compare.

The argmax slots here are the float64 forward's own (first slot of the maximum, 255 without a
positive in-radius row); on the device they are the kernel's saved ones. Reference op:
controller.py:16-20,43-46 of the reference, differentiated by its train.py:103."""
import pytest
import torch

from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.selfcheck import edge_oracle

import ctrl_fwd_cases as CC
import ctrl_fwd_ref as R
import edge_bwd_cases as EC

# non-zero reference dEc rows per case on the float64 forward's own argmax (a silent change of the case
# builder or of a seed moves them)
NONZERO = {"k12": 422, "k16": 393, "k11": 182, "k10": 472, "k9": 403, "k8": 131, "k7d3": 134, "k3": 67, "k2": 62, "k1": 0, "k5": 10,
           "n300": 1601}
TIE_CAP = 0.03              # tie rows per case: a condition on the cases, not a measurement (0 - 1.9 % here)
_REFS = {}


def _reference(name):
    """(case, float64 parameters, argmax (B, N, 128) uint8, edge_oracle's outputs), once per case."""
    if name not in _REFS:
        case = EC.build(name)
        p = R.kernel_params(CC.controller(case["D"]).params_dict(), "fp32")
        S = native.to_records(case["s"])
        pb = R.pooled_bound(R.edge_phase(p, S, case["idx"], case["N"], "fp32"), "fp32")
        am = torch.where(pb["top"] > 0, pb["arg"], torch.full_like(pb["arg"], R.NONE)).to(torch.uint8)
        dP = EC.split_dP(case["dP"], torch.bfloat16, True)
        _REFS[name] = (case, p, am, edge_oracle(p, S, case["idx"], am, dP, case["N"], case["D"], exact=case["planted"]))
    return _REFS[name]


@pytest.mark.parametrize("name", ["k12", "k7d3", "k3"])
def test_edge_oracle_matches_controller_autograd(name, monkeypatch):
    """drel and the edge-net gradients equal autograd of sum(dP * pooled) through
    oracle.controller_forward with pool_slots pinned, to 1e-12 relative; self rows are zero in the
    contract (+i - i cancels) whatever autograd gives for the relative state of a self pair."""
    case, p, am, (drel, tie, dws, scales, rscale) = _reference(name)
    N, D = case["N"], case["D"]
    dP = EC.split_dP(case["dP"], torch.bfloat16, True).double()
    dPf = dP[..., :128] + dP[..., 128:]
    kept = {}
    orig = O.edge_rel

    def spy(*a, **k):
        rel, eye = orig(*a, **k)
        rel.retain_grad()
        kept["rel"] = rel
        return rel, eye

    monkeypatch.setattr(O, "edge_rel", spy)
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    s64 = case["s"].double().requires_grad_(True)
    _, aux = O.controller_forward(pr, s64[:, :N], case["G"].double(), case["idx"].long(), return_aux=True, nodes=s64,
                                  pool_slots=am)
    names = [k for k in pr if k.startswith("controller_centr_net")]
    gw = torch.autograd.grad((dPf * aux["pooled"]).sum(), [pr[k] for k in names], retain_graph=True)
    (dPf * aux["pooled"]).sum().backward()
    want = kept["rel"].grad
    notself = (case["idx"].long() != torch.arange(N).view(1, N, 1)).unsqueeze(-1)

    def close(got, ref, what):
        bound = 1e-12 * float(ref.abs().max())
        assert float((got - ref).abs().max()) <= bound, (what, float((got - ref).abs().max()), bound)

    assert float(want.abs().max()) > 0
    close(drel, want * notself, "drel")
    assert not bool(drel[~notself.expand_as(drel)].any())
    for k, g in zip(names, gw):
        close(dws[k], g, k)
        assert float(g.abs().max()) > 0, k
        assert bool((scales[k] + 1e-300 >= g.abs()).all()), k                 # sum |terms| >= |sum terms|
    assert bool((rscale * (1 + 1e-12) + 1e-300 >= drel.abs()).all())


@pytest.mark.parametrize("name", EC.ALL)
def test_case_conditions(name):
    """Tie rows (relu ties on z1 / z2, radius ties on unplanted edges) <= 3 % of the case's rows; every
    case but k1 has non-zero reference rows; k1 (self edges only) has none and non-zero weight
    gradients."""
    case, p, am, (drel, tie, dws, scales, rscale) = _reference(name)
    B, N, K = case["idx"].shape
    assert (case["B"], case["N"], case["K"]) == (B, N, K) and (K == N or N > K)
    rows = drel.reshape(-1, drel.shape[-1])
    nz = int(rows.ne(0).any(-1).sum())
    print(f"CASE {name}: tie rows {int(tie.sum())}/{tie.numel()}, non-zero rows {nz}")
    assert int(tie.sum()) <= TIE_CAP * tie.numel(), (name, int(tie.sum()), tie.numel())
    assert bool(torch.isfinite(rows).all())
    assert nz == NONZERO[name] and (nz > 0) == (name != "k1"), (name, nz)
    for k, g in dws.items():
        assert float(g.abs().max()) > 0, (name, k)
    # the 255 entries carry a finite non-zero dP that must reach nothing
    none = am == R.NONE
    assert bool(none.any()) or name in ("k5",)
    assert bool((case["dP"][none] != 0).all()) and bool(torch.isfinite(case["dP"]).all())


def test_shared_scenes_are_the_forward_suite_s():
    for n in EC.SHARED:
        a, b = EC.build(n), CC.build(n)
        for k in ("s", "G", "idx", "planted"):
            assert a[k] is b[k], (n, k)


def test_rolled_case_keeps_every_agent():
    case = EC.build("k10")
    N = case["N"]
    r = 37 % N
    rc = EC.rolled(case, r)
    assert torch.equal(rc["dP"].roll(-r, 1), case["dP"]) and torch.equal(rc["s"][:, :N].roll(-r, 1), case["s"][:, :N])
    a = O.edge_rel(case["s"][:, :N], case["idx"].long(), case["s"])
    b = O.edge_rel(rc["s"][:, :N], rc["idx"].long(), rc["s"])
    assert torch.equal(b[0].roll(-r, 1), a[0]) and torch.equal(b[1].roll(-r, 1), a[1])
