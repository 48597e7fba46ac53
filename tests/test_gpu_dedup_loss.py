"""GPU: cbf_dh_kernel and cbf_compact_kernel (csrc/dedup.hip) on their own, against the float64
references of tests/dedup_ref.py.

cbf_dh: the inputs keep every hinge argument either exactly zero (ties, which test the strict
`> 0`) or further from zero than fp32 rounding reaches (checked on the CPU by
tests/test_dedup_loss_ref.py), so the kernel's eight indicators must equal the reference's and the
gradient differs by the rounding of its few fp32 operations only. cbf_compact: integers, exact."""
import math

import pytest
import torch

from macbf_gnn_amd.ops import native

import dedup_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENT = 1234.5
U24 = 2.0 ** -24


def _note(group, ratio):
    print(f"RATIO {group} {ratio:.4f}")


def _dev_case(c):
    i32 = torch.int32
    return dict(h=c["h"].to(DEV), hmask=c["hmask"].to(DEV), map1=c["map1"].to(i32).to(DEV).contiguous(),
                src=c["src"].to(i32).to(DEV), nev=torch.tensor([c["U"]], dtype=i32, device=DEV),
                dang=c["dang"].to(DEV), valid=None if c["valid"] is None else c["valid"].to(DEV))


def _run_dh(c, nb, counts, grad_scale=1.0, gscale=None):
    d = _dev_case(c)
    dh = torch.full((2 * c["E"],), SENT, device=DEV)
    partial = torch.full((nb, native.DH_PARTIAL), 7.0, device=DEV)
    blk = torch.full((nb,), -5, dtype=torch.int32, device=DEV)
    gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device=DEV)
    native.cbf_dh(d["h"], d["hmask"], d["map1"], d["src"], d["nev"], d["dang"], d["valid"], counts.to(DEV), dh, partial,
                  grad_scale=grad_scale, blk_active=blk, gscale=gs)
    torch.cuda.synchronize()
    return d, dh, partial.cpu(), blk.cpu()


def _check_dh(c, nb, counts=None, grad_scale=1.0, gscale=None):
    E, U = c["E"], c["U"]
    counts = c["counts"] if counts is None else counts
    ref, abs_terms, sums = R.dh_reference(c["h"], c["hmask"], c["map1"], c["src"], U, c["dang"], c["valid"], counts,
                                          grad_scale=grad_scale, gscale=gscale)
    _, dh_dev, partial, blk = _run_dh(c, nb, counts, grad_scale, gscale)
    dh = dh_dev.cpu()
    assert bool((dh[U:] == SENT).all())
    got = dh[:U].double()
    bound = 2e-6 * (abs_terms + float(ref.abs().max()))
    err = (got - ref).abs()
    if float(bound.max()) > 0:
        _note("cbf_dh.dh", float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all()), float((err - bound).max())
    zero = (abs_terms == 0) | (c["hmask"][:U] == 0)
    assert bool((got[zero] == 0).all())
    assert bool((got[ref.abs() > bound] != 0).all())
    # loss partials: [0, 0, acc[0..7], 0, 0]
    col = partial.double().sum(0)
    assert col[0] == 0 and col[1] == 0 and col[10] == 0 and col[11] == 0
    assert bool((partial[:, [0, 1, 10, 11]] == 0).all())
    for q in (2, 3, 6, 7):
        assert float(col[2 + q]) == float(sums[q]), (R.SUM_NAMES[q], float(col[2 + q]), float(sums[q]))
    for q in (0, 1, 4, 5):
        lb = (math.ceil(U / 256) + 16) * U24 * float(sums[q].abs())
        e = abs(float(col[2 + q]) - float(sums[q]))
        if lb > 0:
            _note("cbf_dh.loss", e / lb)
        assert e <= lb, (R.SUM_NAMES[q], float(col[2 + q]), float(sums[q]), lb)
    # per-block active counts: the kernel's own dh and the reference's zero pattern
    span = R.span_of(U, nb)
    for b in range(nb):
        lo, hi = min(U, b * span), min(U, (b + 1) * span)
        assert int(blk[b]) == int((dh[lo:hi] != 0).sum()), b
        assert int(blk[b]) == int((ref[lo:hi] != 0).sum()), b
    return dh_dev, blk


def _nbs(U):
    return (1, 3, 7, math.ceil(U / 256) + 3)       # the last: span 256, trailing blocks own nothing


@pytest.mark.parametrize("nbi", [0, 1, 2, 3], ids=["nb1", "nb3", "nb7", "nbtail"])
@pytest.mark.parametrize("vp", R.VALID_PATTERNS)
@pytest.mark.parametrize("recomputed", [False, True], ids=["reuse", "rc"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cbf_dh_equals_reference(shape, recomputed, vp, nbi):
    c = R.make_case(*shape, R.case_seed(shape), recomputed, vp)
    _check_dh(c, _nbs(c["U"])[nbi])


def test_cbf_dh_scales():
    """Host grad_scale and the device loss scale multiply every term."""
    shape = R.SHAPES[0]
    c = R.make_case(*shape, R.case_seed(shape), False, "drop")
    _check_dh(c, 3, grad_scale=0.5, gscale=1024.0)


def test_cbf_dh_counts_are_the_argument():
    """The normalisers come from `counts` (the global pooled counts), not from this call's masks."""
    shape = R.SHAPES[3]
    c = R.make_case(*shape, R.case_seed(shape), False, "dead")
    _check_dh(c, 3, counts=torch.tensor([c["counts"][0] * 3 + 17, c["counts"][1] * 2 + 5]))


# ---------------------------------------------------------------------------- cbf_compact
# (U, E, nb): U < E, E < U < 2E; spans 256 / 1280 / 2560 (rounds of 1024 evaluations); trailing empty blocks
COMPACT = [(1, 8, 1), (1, 8, 3), (255, 200, 1), (256, 200, 2), (257, 200, 2), (257, 300, 1), (2500, 1500, 2),
           (2500, 1500, 1), (2500, 1500, 12), (2500, 3000, 3)]


def _synthetic(U, E, density, seed):
    g = torch.Generator().manual_seed(seed)
    dh = torch.randn(2 * E, generator=g)
    dh[dh == 0] = 1.0
    keep = torch.rand(2 * E, generator=g) < density
    if density >= 1.0:
        keep[:] = True
    neg0 = torch.rand(2 * E, generator=g) < 0.3
    dh = torch.where(keep, dh, torch.where(neg0, torch.tensor(-0.0), torch.tensor(0.0)))
    dh[U:] = 7.0                                               # garbage beyond U
    src = torch.full((2 * E,), -1, dtype=torch.int32)
    src[E:] = torch.randint(0, E, (E,), generator=g, dtype=torch.int32)
    idx = torch.randint(0, 1000, (E,), generator=g, dtype=torch.int32)
    idx1 = torch.randint(1000, 2000, (E,), generator=g, dtype=torch.int32)
    return dh, src, idx, idx1


def _blk_active(dh, U, nb):
    span = R.span_of(U, nb)
    return torch.tensor([int((dh[min(U, b * span):min(U, (b + 1) * span)] != 0).sum()) for b in range(nb)],
                        dtype=torch.int32)


def _check_compact(dh_dev, U, E, blk_dev, src_dev, idx_dev, idx1_dev):
    """act list and records (idx1 = idx and a different idx1) of one dh buffer, exact."""
    nev = torch.tensor([U], dtype=torch.int32, device=DEV)
    n2 = dh_dev.numel()
    act_ref, _ = R.compact_reference(dh_dev, U, E, src_dev, idx_dev, idx1_dev)
    n = act_ref.numel()
    act = torch.full((n2,), -9, dtype=torch.int32, device=DEV)
    nact = native.cbf_active(dh_dev, nev, blk_dev, act)
    torch.cuda.synchronize()
    assert int(nact) == n
    assert torch.equal(act[:n].cpu().long(), act_ref)
    assert bool((act[n:] == -9).all())
    for other in (idx_dev, idx1_dev):
        _, rec_ref = R.compact_reference(dh_dev, U, E, src_dev, idx_dev, other)
        rec = torch.full((n2, 4), -9, dtype=torch.int32, device=DEV)
        nact = native.cbf_active(dh_dev, nev, blk_dev, None, rec=rec, src=src_dev, idx=idx_dev, idx1=other)
        torch.cuda.synchronize()
        assert int(nact) == n
        assert torch.equal(rec[:n].cpu(), rec_ref)
        assert bool((rec[n:] == -9).all())
        assert torch.equal(rec[:n, 1].cpu() < 0, act_ref >= E)          # the pass bit is the sign bit
        assert torch.equal(rec[:n, 1].cpu().long() & 0x7FFFFFFF,
                           torch.where(act_ref >= E, src_dev.cpu().long()[act_ref], act_ref))
    return n


@pytest.mark.parametrize("density", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("U,E,nb", COMPACT)
def test_cbf_active_equals_reference(U, E, nb, density):
    dh, src, idx, idx1 = _synthetic(U, E, density, seed=U + E + nb)
    blk = _blk_active(dh, U, nb)
    n = _check_compact(dh.to(DEV), U, E, blk.to(DEV), src.to(DEV), idx.to(DEV), idx1.to(DEV))
    if density == 0.0:
        assert n == 0
    elif density == 1.0:
        assert n == U
    if density < 1.0 and U >= 255:
        assert bool(((dh[:U] == 0) & torch.signbit(dh[:U])).any())      # -0.0 entries are present


def test_compact_spans_cover_the_listed_block_shapes():
    spans = {R.span_of(U, nb) for U, _, nb in COMPACT}
    assert {256, 1280, 2560} <= spans
    assert any(R.span_of(U, nb) * (nb - 1) >= U for U, _, nb in COMPACT if nb > 1)    # a trailing empty block
    assert any(U < E for U, E, _ in COMPACT) and any(E < U < 2 * E for U, E, _ in COMPACT)


@pytest.mark.parametrize("recomputed", [False, True], ids=["reuse", "rc"])
def test_cbf_dh_then_cbf_active(recomputed):
    """cbf_dh -> cbf_active on the same buffers, as the engine chains them."""
    shape = R.SHAPES[2]
    c = R.make_case(*shape, R.case_seed(shape), recomputed, "drop")
    dh_dev, blk = _check_dh(c, 3)
    T = c["T"]
    idx = c["idx"][:T].contiguous().to(DEV)
    idx1 = c["idx"][1:T + 1].contiguous().to(DEV) if recomputed else idx
    src = c["src"].to(torch.int32).to(DEV)
    n = _check_compact(dh_dev, c["U"], c["E"], blk.to(DEV), src, idx, idx1)
    assert 0 < n < c["U"]
