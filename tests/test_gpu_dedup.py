"""GPU: the deduplicated CBF path (csrc/dedup.hip + cbf_hfwd + non-fused cbf_bwd on the
evaluation list + node_reduce with map1) against its pure-torch index reference and against
the fused two-evaluation kernel."""
import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.dedup import match_reference

import dedup_ref as DR
from test_gpu_backward import _cmp, _states, _trainer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("recomputed", [False, True])
def test_cbf_match_equals_reference(recomputed):
    T, B, N, K = 4, 2, 50, C.TOP_K
    S = _states((T + 1, B), N, seed=4, vscale=1.5).contiguous()
    Tg = T + int(recomputed)
    idx = torch.stack([O.knn_idx(S[t], K) for t in range(Tg)]).to(torch.int32).contiguous()
    E = T * B * N * K
    map1 = torch.full((T, B, N, K), -7, dtype=torch.int32, device=DEV)
    src = torch.full((2 * E,), -7, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(T * B * N, dtype=torch.int32, device=DEV)
    nev = native.cbf_match(idx, T, map1, src, cnt, recomputed=recomputed)
    m_ref, s_ref, n_ref = match_reference(idx, T, recomputed=recomputed)
    torch.cuda.synchronize()
    assert int(nev) == n_ref
    assert torch.equal(map1.cpu().long(), m_ref)
    assert torch.equal(src[:n_ref].cpu().long(), s_ref[:n_ref])
    if not recomputed:
        assert n_ref > E            # the states move: some neighbour sets change


@pytest.mark.parametrize("recomputed", [False, True])
@pytest.mark.parametrize("case", DR.MATCH_CASES + [DR.MATCH_BIG], ids=DR.match_case_id)
def test_cbf_match_on_planted_lists(case, recomputed):
    """cbf_match on synthetic lists (tests/dedup_ref.planted_lists: self in slot 0, distinct ids, 0.9
    of the neighbours kept per step in shuffled slots) at every K, at row counts around a 256-row
    block, without a next step, with the step boundaries inside blocks, and above 2,048 blocks (the
    second trip of block_sum_prefix's unrolled loop): nev, map1 and src[:nev] exact, src[nev:]
    untouched."""
    T, B, N, K = case[:4]
    idx, m_ref, s_ref, n_ref = DR.match_case(case, recomputed)
    E = T * B * N * K
    map1 = torch.full((T, B, N, K), -7, dtype=torch.int32, device=DEV)
    src = torch.full((2 * E,), -7, dtype=torch.int32, device=DEV)
    cnt = torch.zeros((T * B * N + native.MATCH_BLOCK - 1) // native.MATCH_BLOCK, dtype=torch.int32, device=DEV)
    nev = native.cbf_match(idx.to(DEV), T, map1, src, cnt, recomputed=recomputed)
    torch.cuda.synchronize()
    assert int(nev) == n_ref
    assert torch.equal(map1.cpu().long(), m_ref)
    assert torch.equal(src[:n_ref].cpu().long(), s_ref[:n_ref])
    assert bool((src[n_ref:] == -7).all())
    if case == DR.MATCH_BIG:
        assert cnt.numel() > 2048
    if K >= 2 and T >= 2 and not recomputed:      # (recomputed lists match slot k with slot k: the last step's slots alone)
        assert n_ref > E + B * N * K, "the extras are all in the last step"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("reuse", [True, False])
def test_dedup_step_matches_fused_kernel(reuse, prec):
    """One training step: deduplicated evaluation list vs the fused h/h' kernel (same
    semantics, different evaluation order; bf16: the summed upstream grads dh + dh' of a
    shared evaluation are rounded once instead of twice -> a looser bound)."""
    a = _trainer(DEV, N=96, B=3, T=6, reuse_nbr_idx=reuse, cbf_dedup=True, dtype=prec)
    b = _trainer(DEV, N=96, B=3, T=6, reuse_nbr_idx=reuse, cbf_dedup=False, dtype=prec)
    rel = 1e-4 if prec == "fp32" else 2e-2
    assert a.engine.dedup and not b.engine.dedup
    s0, g, _ = a.sample()
    sa = a.engine.step(s0, g)
    ga = a.fp.grad.clone()
    sb = b.engine.step(s0, g)
    gb = b.fp.grad.clone()
    for name in ("controller", "cbf"):
        lo, hi = a.fp.ranges[name]
        _cmp(ga[lo:hi], gb[lo:hi], name, rel=rel)
    for k in ("loss_dang", "loss_safe", "loss_dang_deriv", "loss_safe_deriv", "loss_action",
              "acc_dang_sum", "acc_safe_sum", "acc_dang_deriv_sum", "acc_safe_deriv_sum"):
        x, y = float(sa[k]), float(sb[k])
        assert abs(x - y) <= 2e-3 * abs(y) + 1e-5, (k, x, y)
    # the per-step state gradients (CBF -> dS) agree too
    _cmp(a.engine.dS, b.engine.dS, "dS", rel=rel)


def test_dedup_deterministic():
    tr = _trainer(DEV, N=64, B=3, T=5)
    assert tr.engine.dedup
    s0, g, _ = tr.sample()
    tr.engine.step(s0, g)
    g1 = tr.fp.grad.clone()
    tr.engine.step(s0, g)
    assert torch.equal(g1, tr.fp.grad)
