"""The float64 reference of the CBF h forward (tests/cbf_fwd_ref.py) pinned to oracle.cbf_forward, and
the conditions the shared cases (tests/cbf_fwd_cases.py) must meet for the device tests' per-evaluation
assertions to be decidable -- all from the reference alone, on the CPU: the planted pair brackets the
radius on adjacent bit patterns, no other edge comes near it, every list has extras and both mask
values, and the bound is finite, positive and far below the old per-tensor tolerance."""
import math

import pytest
import torch

from macbf_gnn_amd import oracle as O

import cbf_fwd_cases as FC
import cbf_fwd_ref as R

CASE_MODES = [(n, m) for n in FC.ALL for m in FC.MODES]


def _params(case, prec="fp32"):
    return R.kernel_params(FC.cbf(case["D"]).params_dict(), prec)


def _main_list(case):
    """The main slots alone as an evaluation list (U = E)."""
    E = case["idx"].numel()
    return case["idx"], case["idx"], torch.zeros(2 * E, dtype=torch.int32), E


@pytest.mark.parametrize("name", FC.ALL)
def test_reference_equals_the_oracle_in_float64(name):
    """Features formed in float64 (the oracle's arithmetic): h of the main slots on s_t and of the slots
    on s_{t+1} with the next step's lists equals oracle.cbf_forward to 1e-12, obstacle neighbours
    through nodes=; with bf16-rounded parameters and activations the emulating oracle likewise."""
    case = FC.build(name)
    T, N = case["T"], case["N"]
    S, idx = case["S"], case["idx"]
    E = idx.numel()
    S64 = S.double()
    for prec, emu in (("fp32", None), ("bf16", torch.bfloat16)):
        p = _params(case, prec)
        with O.emulate_bf16(emu is not None):
            want0 = O.cbf_forward(p, S64[:T, :, :N], idx.long(), nodes=S64[:T]).reshape(-1)
            want1 = O.cbf_forward(p, S64[1:, :, :N], case["idx_next"].long(), nodes=S64[1:]).reshape(-1)
        got0 = R.list_reference(p, prec, S, *_main_list(case), emulate=emu, dtype=torch.float64)["h"]
        # every slot as an extra: evaluation E + e is slot e on s_{t+1} with idx1 = the next step's list
        src = torch.cat([torch.zeros(E, dtype=torch.int32), torch.arange(E, dtype=torch.int32)])
        got1 = R.list_reference(p, prec, S, idx, case["idx_next"], src, 2 * E, emulate=emu, dtype=torch.float64)["h"][E:]
        assert float((got0 - want0).abs().max()) <= 1e-12, (name, prec, "h(s_t)")
        assert float((got1 - want1).abs().max()) <= 1e-12, (name, prec, "h(s_t+1)")
        assert bool((want0 != 0).any()) and bool((want1 != 0).any())


@pytest.mark.parametrize("name", FC.ALL)
def test_fp32_mask_equals_the_oracles_fp32_mask(name):
    case = FC.build(name)
    T, N = case["T"], case["N"]
    S, idx = case["S"], case["idx"]
    ref = R.list_reference(_params(case), "fp32", S, *_main_list(case))
    x, m = O.cbf_features(S[:T, :, :N], idx.long(), nodes=S[:T])
    assert m.dtype == torch.float32
    assert torch.equal(ref["mask"], m.reshape(-1).bool())
    assert torch.equal(ref["x"].float(), x.reshape(-1, x.shape[-1]))          # the features too, bit for bit


@pytest.mark.parametrize("D", [2, 3])
def test_planted_pair_brackets_the_radius(D):
    x_in, x_out = FC.radius_edge(D)
    assert FC._bits(x_out) == FC._bits(x_in) + 1                               # adjacent bit patterns
    assert FC.d32(x_in, D) <= 1.0 < FC.d32(x_out, D)
    assert FC.d32(x_in, D) == 1.0          # exactly at the radius: `<` in place of `<=` flips this mask
    assert x_out == float(torch.nextafter(torch.tensor(x_in), torch.tensor(math.inf)))


@pytest.mark.parametrize("name,mode", CASE_MODES, ids=[f"{n}-{m}" for n, m in CASE_MODES])
def test_case_conditions(name, mode):
    case, ls = FC.build(name), FC.lists(name, mode)
    T, B, N, K = case["idx"].shape
    E, U, src, idx1 = ls["E"], ls["U"], ls["src"], ls["idx1"]
    Nn = case["Nn"]
    for ix in (case["idx"], case["idx_next"]):
        assert int(ix.min()) >= 0 and int(ix.max()) < Nn
    assert src.numel() == 2 * E and int(src.min()) >= 0 and int(src.max()) < E       # every entry a valid slot
    assert E < U <= 2 * E, "no extras"
    assert not bool((src[:E].long() == torch.arange(E)).any())                        # wrong in the main part
    assert (idx1 is case["idx"]) == (mode == "match")
    if mode == "plant":
        assert (U - E) % 32 != 0 and bool((ls["extras"][1:] < ls["extras"][:-1]).any())
    if case["M"]:
        assert int((case["idx"].long() >= N).sum()) >= 50                              # obstacle neighbours
    assert torch.isfinite(case["S"]).all()
    assert torch.equal(case["S"][..., : case["D"]] * FC.GRID, torch.round(case["S"][..., : case["D"]] * FC.GRID)) or case["plants"]
    ref = R.list_reference(_params(case), "fp32", case["S"], case["idx"], idx1, src, U)
    le, d, mask = ref["le"], ref["d"].double(), ref["mask"]
    assert bool(torch.isfinite(ref["e_h"]).all()) and bool((ref["e_h"] > 0).all())
    # self edges: one per agent and step, in slot 0 unless a duplicate record with a lower index sits on it
    self_e = le["i"] == le["j"]
    assert int(self_e[:E].sum()) == T * B * N
    if K > 1:
        # (K = 1 lists the self edge alone: always in radius, idx_next == idx)
        assert bool(mask.any()) and bool((~mask).any())
        assert bool(mask[E:].any()) and bool((~mask[E:]).any()), "the extras carry one mask value only"
        if mode == "recomp":
            e = le["e"][E:]
            assert bool((idx1.reshape(-1)[e] != case["idx"].reshape(-1)[e]).any()), "idx1 == idx on every extra"
    planted = torch.zeros(U, dtype=torch.bool)
    if case["plants"]:
        x_in, x_out = FC.radius_edge(case["D"])
        for b in range(B):
            P, Q, Tt, R1, R2 = (int(case[k][b]) for k in ("P", "Q", "Tt", "R1", "R2"))
            eb = le["b"] == b
            for i, j, inside in ((P, Q, True), (Q, P, True), (P, Tt, False), (Tt, P, False)):
                sel = eb & (le["i"] == i) & (le["j"] == j)
                assert int(sel[:E].sum()) == T, (name, b, i, j, "the planted edge is not in every step's list")
                assert bool((mask[sel] == inside).all())
                assert bool((ref["x"][sel, 0].abs() == (x_in if inside else x_out)).all())
                planted |= sel
            # the duplicate pair: two slots of the hub with identical features and identical reference h
            for t in range(T):
                s1 = (eb & (le["t"] == t) & (le["pas"] == 0) & (le["i"] == P) & (le["j"] == R1)).nonzero().reshape(-1)
                s2 = (eb & (le["t"] == t) & (le["pas"] == 0) & (le["i"] == P) & (le["j"] == R2)).nonzero().reshape(-1)
                assert s1.numel() == 1 and s2.numel() == 1
                assert torch.equal(ref["x"][s1], ref["x"][s2]) and bool(mask[s1]) and float(ref["h"][s1]) == float(ref["h"][s2])
    elif K >= 2:
        raise AssertionError("every case with K >= 2 carries the plants")
    # every other edge is at least 2^-16 from the radius (on the grid the margin is ~2e-5)
    near = ((d - 1.0).abs() < 2.0 ** -16) & ~planted
    assert not bool(near.any()), (name, mode, "an unplanted edge near the radius", d[near][:6].tolist())
    print(f"CASE {name} {mode}: E {E} U {U} in radius {float(mask.double().mean()):.2f} "
          f"(extras {float(mask[E:].double().mean()):.2f})")


# The bound's size, read off the reference on the CPU over the in-radius evaluations of every case's
# "plant" list (this test prints the figures; max |h| is 0.211 at the default initialisation):
#
#              largest e_h    largest e_h / max(|h|, 1e-3)    largest e_h / head scale
#     fp32     4.21e-3        7.2e-2                          1.7e-2
#     fp16     1.77e-2        3.1e-1                          6.1e-2
#     bf16     1.19e-1        2.1                             4.0e-1
#
# (head scale = |relu z3| . |w4| + |b4|, the sum of absolute terms h is the signed sum of.) The worst-case
# propagation through |W2| and |W3| costs a factor of ~4 per layer, so the x3 bound is NOT below the old
# per-tensor scale of 1e-4 max |h| = 2.1e-5: it is 200 times that -- but it holds for every single
# evaluation, where the old checks let one entry be wrong by the whole tensor's budget (1e-4 |h|_2 ~ 2e-3 at
# these sizes, 2e-2 max |h| + 2e-3 ~ 6e-3 in test_gpu_forward). In bf16 the bound is half of max |h|: on its
# own it would catch gross errors only, which is why the 1-pass builds are held to the rounded-activation
# reference as well (CAPS16 below) next to the exact parts of the contract (mask bytes, +0.0, bit
# equalities); docs/PERF.md, "CBF forward oracle", has the measured err / bound ratios and what each seeded
# defect trips. The caps below are these figures rounded up (not fitted to any kernel
# output: the reference alone gives them); a change of the bound that loosens it shows here.
CAPS = {"fp32": (5e-3, 8e-2), "fp16": (2e-2, 3.5e-1), "bf16": (1.3e-1, 2.3)}     # (e_h, e_h / max(|h|, 1e-3))
# largest e16 of the rounded-activation reference (cbf_fwd_ref.forward_rounded), read off the same way:
# bf16 1.02e-2 (median 1.9e-4 on k12: 350 times below the median e_h), fp16 1.59e-3 (median 1.6e-4)
CAPS16 = {"bf16": 1.1e-2, "fp16": 1.7e-3}


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_bound_is_not_vacuous(prec):
    worst, worst_abs, hmax, worst_head, worst16, gap16 = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
    for name in FC.ALL:
        case, ls = FC.build(name), FC.lists(name, "plant")
        p = _params(case, prec)
        ref = R.list_reference(p, prec, case["S"], case["idx"], ls["idx1"], ls["src"], ls["U"])
        m = ref["mask"]
        rel = ref["e_h"][m] / ref["h"][m].abs().clamp_min(1e-3)
        worst = max(worst, float(rel.max()))
        worst_abs = max(worst_abs, float(ref["e_h"][m].max()))
        hmax = max(hmax, float(ref["h"][m].abs().max()))
        worst_head = max(worst_head, float((ref["e_h"][m] / ref["head_scale"][m]).max()))
        if prec != "fp32":
            # the rounded-activation reference: a tighter bound, and itself inside the plain bound of the
            # unrounded reference (the two references bound the same kernel)
            worst16 = max(worst16, float(ref["e16"][m].max()))
            gap16 = max(gap16, float(((ref["h16"][m] - ref["h"][m]).abs() / ref["e_h"][m]).max()))
            assert bool((ref["e16"][m] > 0).all()) and bool((ref["e16"][m] < ref["e_h"][m]).all())
    if prec != "fp32":
        print(f"BOUND {prec}: rounded-activation e16 <= {worst16:.3e}, |h16 - h| / e_h <= {gap16:.3e}")
        assert worst16 <= CAPS16[prec] and gap16 < 1.0
    print(f"BOUND {prec}: e_h <= {worst_abs:.3e}, e_h / max(|h|, 1e-3) <= {worst:.3e}, e_h / head scale <= {worst_head:.3e}, "
          f"max |h| {hmax:.3e}")
    assert worst_abs <= CAPS[prec][0] and worst <= CAPS[prec][1]
    if prec == "fp32":
        assert worst_abs < 2e-2 * hmax          # every x3 evaluation within 2 % of the largest |h|


@pytest.mark.parametrize("name", ["k12", "3d_obs"])
def test_rolled_case_keeps_every_evaluation(name):
    """rolled(case, 5) with the extras renamed through roll_slot_map: every evaluation keeps its features."""
    case, ls = FC.build(name), FC.lists(name, "plant")
    E, U = ls["E"], ls["U"]
    rc, mp = FC.rolled(case, 5), FC.roll_slot_map(case, 5)
    src = ls["src"].clone()
    src[E:U] = mp[ls["extras"]].to(torch.int32)
    p = _params(case)
    a = R.list_reference(p, "fp32", case["S"], case["idx"], ls["idx1"], ls["src"], U)
    b = R.list_reference(p, "fp32", rc["S"], rc["idx"], rc["idx_next"], src, U)
    assert torch.equal(a["x"][:E], b["x"][:E][mp]) and torch.equal(a["x"][E:], b["x"][E:])
    assert torch.equal(a["h"][:E], b["h"][:E][mp]) and not torch.equal(a["x"][:E], b["x"][:E])
    assert sorted(mp.tolist()) == list(range(E))


@pytest.mark.parametrize("name", list(FC.FILTER_CASES))
def test_filter_cases_have_no_edge_at_the_radius(name):
    """s' = s + dt [v, a] is off the grid: for exactly these seeds no edge has |d' - 1| <= 1e-6 (then the
    fp32 mask at s' is decidable and the device test asserts it exactly). If one turns up, change the seed."""
    _, s, a, idx, obs = FC.filter_inputs(name)
    f = R.filter_features(s, a, idx, obs)
    d = f["d"].double()
    assert not bool(((d - 1.0).abs() <= 1e-6).any())
    assert bool(f["mask"].any()) and bool((~f["mask"]).any())
    assert bool((f["ex"] >= 0).all()) and bool((f["ex"][..., -1] > 0).all())
