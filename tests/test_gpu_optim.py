"""The fused optimizer tail of round 6 (csrc/optim.hip) against the single-purpose launches it
replaced and plain torch: one slab-reduction launch for several slabs (wide and narrow), the
gradient assembly with its finite check and statistics row, both Adam groups in one launch, and the
optimizer commit inside the weight repack. Reference: the two optimizers of /root/reference
train.py:36-37 (torch.optim.Adam, L2 weight decay) and their step at train.py:101-105."""
import pytest
import torch

from macbf_gnn_amd.ops import native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def test_reduce_multi_equals_reduce_rows_and_torch():
    """Wide slabs: bitwise the per-slab reduce_rows sums (same fixed order); the narrow loss-partial
    slab (12 columns x 4,096 rows, 64 row slices) and every slab within fp32 rounding of a float64
    torch sum."""
    jobs = [(_rand(256, 28896, seed=1), 28896), (_rand(256, 10368, seed=2), 10368), (_rand(4096, 12, seed=3), 12),
            (_rand(40, 8, seed=4), 8)]
    outs = [torch.zeros(c, device=DEV) for _, c in jobs]
    native.reduce_multi([(p, o, False) for (p, _), o in zip(jobs, outs)])
    torch.cuda.synchronize()
    for (p, c), o in zip(jobs, outs):
        ref = torch.zeros(c, device=DEV)
        native.reduce_rows(p, ref)
        torch.cuda.synchronize()
        assert torch.equal(o, ref), c
        want = p.double().sum(0).float()
        torch.testing.assert_close(o, want, rtol=1e-5, atol=1e-4 * p.shape[0] ** 0.5)


def test_reduce_multi_accumulates():
    p, o = _rand(64, 32, seed=5), _rand(32, seed=6)
    ref = o.clone() + p.double().sum(0).float()
    native.reduce_multi([(p, o, True)])
    torch.cuda.synchronize()
    torch.testing.assert_close(o, ref, rtol=1e-5, atol=1e-5)


def test_adam_multi_is_bitwise_two_adam_launches():
    n = 51141
    ranges = [(0, 30000), (30000, n)]
    base = [_rand(n, seed=s) for s in (7, 8)] + [_rand(n, seed=9).abs()]
    grad = _rand(n, seed=10)
    outs = []
    for fused in (False, True):
        p, m, v = (t.clone() for t in base)
        steps = torch.tensor([3, 5], dtype=torch.int32, device=DEV)
        ok = torch.ones(1, dtype=torch.int32, device=DEV)
        if fused:
            native.adam_multi(p, grad, m, v, [(a, b, steps[i:i + 1]) for i, (a, b) in enumerate(ranges)],
                              1e-3, 0.9, 0.999, 1e-8, 1e-2, ok=ok)
        else:
            for i, (a, b) in enumerate(ranges):
                native.adam(p, grad, m, v, a, b, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, ok=ok, step_dev=steps[i:i + 1])
        torch.cuda.synchronize()
        outs.append((p, m, v))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    # a cleared guard flag leaves everything untouched
    p, m, v = (t.clone() for t in base)
    native.adam_multi(p, grad, m, v, [(0, n, torch.zeros(1, dtype=torch.int32, device=DEV))], 1e-3, 0.9, 0.999, 1e-8,
                      0.0, ok=torch.zeros(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(p, base[0]) and torch.equal(m, base[1]) and torch.equal(v, base[2])


@pytest.mark.parametrize("ok_in,fp16", [(1, False), (0, False), (1, True), (0, True)])
def test_commit_in_pack_gather_equals_step_commit(ok_in, fp16):
    """The optimizer commit run by the weight-repack launch == the step_commit kernel: step counts
    of the masked groups, skip count, fp16 loss scale / good-step count, the statistics row's two
    fields, the re-armed flag."""
    res = []
    for via_pack in (False, True):
        ok = torch.full((1,), ok_in, dtype=torch.int32, device=DEV)
        steps = torch.tensor([4, 9], dtype=torch.int32, device=DEV)
        skipped = torch.tensor([2], dtype=torch.int32, device=DEV)
        gscale = torch.tensor([1024.0], device=DEV) if fp16 else None
        good = torch.tensor([999], dtype=torch.int32, device=DEV) if fp16 else None
        row = torch.zeros(18, device=DEV)
        kw = dict(gscale=gscale, good=good, growth=1000, stats_row=row)
        if via_pack:
            src = _rand(100, seed=11)
            idx16 = torch.arange(64, dtype=torch.int32, device=DEV)
            idx32 = torch.arange(32, dtype=torch.int32, device=DEV)
            out16 = torch.empty(64, dtype=torch.bfloat16, device=DEV)
            out32 = torch.empty(32, device=DEV)
            native.pack_gather(src, idx16, out16, idx32, out32, commit=native.step_commit_args(ok, steps, 0b10, skipped,
                                                                                               **kw))
            torch.cuda.synchronize()
            assert torch.equal(out32, src[:32]) and torch.equal(out16, src[:64].bfloat16())
        else:
            native.step_commit(ok, steps, 0b10, skipped, **kw)
        torch.cuda.synchronize()
        res.append([ok, steps, skipped, row] + ([gscale, good] if fp16 else []))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert int(res[1][0]) == 1                                   # re-armed


def test_grad_assemble_check_and_stats_row():
    """grad_assemble with ok: clears it on a non-finite assembled element only; with stats: the row
    stats_pack writes."""
    n = 5000
    red = _rand(3 * n, seed=12)
    ptr = torch.arange(0, 3 * n + 1, 3, dtype=torch.int32, device=DEV)
    src = torch.arange(3 * n, dtype=torch.int32, device=DEV)
    sums, counts, local = _rand(10, seed=13), _rand(3, seed=14), _rand(3, seed=15)
    for poison in (False, True):
        r = red.clone()
        if poison:
            r[4711] = float("inf")
        grad = torch.empty(n, device=DEV)
        ok = torch.ones(1, dtype=torch.int32, device=DEV)
        row, ref_row = torch.zeros(18, device=DEV), torch.zeros(18, device=DEV)
        native.grad_assemble(r, ptr, src, grad, scale=0.5, ok=ok, stats=(sums, counts, local, row))
        native.stats_pack(sums, counts, local, ref_row)
        g0 = torch.empty(n, device=DEV)
        native.grad_assemble(r, ptr, src, g0, scale=0.5)
        torch.cuda.synchronize()
        assert torch.equal(grad, g0)
        assert int(ok) == (0 if poison else 1)
        assert torch.equal(row, ref_row)


@pytest.mark.parametrize("with_gscale", [False, True])
def test_grad_assemble_ragged_csr_equals_float64_sum(with_gscale):
    """Segments of length 0 / 1 / 2 / 7 / 300 over a source list with repeats, against a float64 sum.
    The kernel adds a segment's len terms one after the other in fp32 (the first addition, to 0, is
    exact: len - 1 roundings) and multiplies by the scale (one more):
    |err| <= (max(len - 1, 1) + 1) * 2**-24 * scale * sum|terms|; an empty segment gives exactly 0.
    The device loss scale is a power of two, so scale / gscale is exact."""
    g = torch.Generator().manual_seed(21)
    n, nred = 601, 5000
    lens = torch.tensor([0, 1, 2, 7, 300])[torch.randint(0, 5, (n,), generator=g)]
    lens[:5] = torch.tensor([0, 1, 2, 7, 300])
    ptr = torch.zeros(n + 1, dtype=torch.int64)
    ptr[1:] = lens.cumsum(0)
    src = torch.randint(0, nred, (int(ptr[-1]),), generator=g)
    assert src.unique().numel() < src.numel()                   # repeats
    red = torch.randn(nred, generator=g)
    scale = 0.3
    gs = torch.tensor([1024.0], device=DEV) if with_gscale else None
    grad = torch.full((n,), 99.0, device=DEV)
    native.grad_assemble(red.to(DEV), ptr.to(torch.int32).to(DEV), src.to(torch.int32).to(DEV), grad, scale=scale,
                         gscale=gs)
    torch.cuda.synchronize()
    s64 = float(torch.tensor(scale, dtype=torch.float32)) / (1024.0 if with_gscale else 1.0)
    terms = red.double()[src]
    seg = torch.repeat_interleave(torch.arange(n), lens)
    want = torch.zeros(n, dtype=torch.float64).index_add_(0, seg, terms) * s64
    asum = torch.zeros(n, dtype=torch.float64).index_add_(0, seg, terms.abs())
    bound = ((lens - 1).clamp_min(1) + 1).double() * 2.0 ** -24 * s64 * asum
    err = (grad.cpu().double() - want).abs()
    print(f"RATIO grad_assemble {float((err[bound > 0] / bound[bound > 0]).max()):.4f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    assert bool((grad.cpu()[lens == 0] == 0).all()) and int((lens == 0).sum()) > 0


@pytest.mark.parametrize("f16", [False, True])
def test_pack_gather_real_index_maps(f16):
    """Random maps with repeats, the constant entries n (0) and n + 1 (1), and bit 30 on some 16-bit
    indices (bf16: the residual bf16(v - float(bf16(v))); fp16 ignores the bit): exact against torch
    casts. m16 + m32 is no multiple of the block size."""
    g = torch.Generator().manual_seed(22)
    n, m16, m32 = 1000, 300, 213
    assert (m16 + m32) % 256 != 0
    src = torch.randn(n, generator=g)
    ext = torch.cat([src, torch.tensor([0.0, 1.0])])
    k16 = torch.randint(0, n + 2, (m16,), generator=g)
    k16[:4] = torch.tensor([n, n + 1, n, n + 1])
    lo = torch.rand(m16, generator=g) < 0.3
    lo[:2], lo[2:4] = False, True
    k32 = torch.randint(0, n + 2, (m32,), generator=g)
    k32[-2:] = torch.tensor([n, n + 1])
    idx16 = (k16 + lo.long() * (1 << 30)).to(torch.int32).to(DEV)
    out16 = torch.zeros(m16, dtype=torch.float16 if f16 else torch.bfloat16, device=DEV)
    out32 = torch.full((m32,), 99.0, device=DEV)
    native.pack_gather(src.to(DEV), idx16, out16, k32.to(torch.int32).to(DEV), out32)
    torch.cuda.synchronize()
    v = ext[k16]
    if f16:
        want16 = v.half()
    else:
        hi = v.bfloat16()
        want16 = torch.where(lo, (v - hi.float()).bfloat16(), hi)
        assert bool((want16[lo] != hi[lo]).any())
    assert torch.equal(out16.cpu().view(torch.int16), want16.view(torch.int16))
    assert torch.equal(out32.cpu(), ext[k32])
