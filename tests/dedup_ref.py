"""Float64 references of the deduplicated CBF loss path (csrc/dedup.hip: cbf_dh_kernel,
cbf_compact_kernel) and the small cases the CPU and GPU tests share.

``dh_reference`` is autograd on the oracle's loss over the evaluation list; ``compact_reference``
the active list and its 16-byte records; ``make_case`` one deterministic input set whose hinge
arguments are, apart from exact ties, further from zero than fp32 rounding can move them, so that
the kernel's fp32 indicators must equal the reference's."""
import functools
import math

import torch
import torch.nn.functional as F

from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.dedup import match_reference

MARGIN = 4e-6               # see margin_violations
H_MAX = 4.0
VALID_PATTERNS = ("none", "ones", "drop", "dead")
SHAPES = ((3, 2, 13, 12), (1, 2, 20, 12), (4, 1, 33, 16), (3, 3, 9, 3))
SUM_NAMES = ("loss_dang", "loss_safe", "acc_dang", "acc_safe", "loss_dang_deriv", "loss_safe_deriv",
             "acc_dang_deriv", "acc_safe_deriv")       # acc[0..7] of cbf_dh_kernel


def loss_consts64():
    """native.LOSS_CONSTS as the kernel receives them: rounded to fp32, held in float64."""
    return [torch.tensor(c, dtype=torch.float32).double() for c in native.LOSS_CONSTS]


def _scale64(grad_scale, gscale):
    # the launcher passes float(LOSS_SCALE * grad_scale) as one fp32; the device scale multiplies it
    s = torch.tensor(native.LOSS_CONSTS[6] * float(grad_scale), dtype=torch.float32).double()
    return s * (1.0 if gscale is None else float(gscale))


def _valid_w(valid, T, B):
    if valid is None:
        return torch.ones(T, B, 1, 1, dtype=torch.float64)
    return valid.reshape(T, B).double()[..., None, None]


def span_of(U, nb):
    """Evaluations per cbf_dh / cbf_compact block (dh_span in csrc/dedup.hip)."""
    per = (U + nb - 1) // nb
    return (per + 255) // 256 * 256


def loss_terms(h_bar, h_main, h_next, dang, valid):
    """The four hinge terms per slot (T,B,N,K), masked by flag and validity, and the accuracy
    indicators, like oracle.cbf_loss_sums; h_bar feeds the barrier terms, h_main / h_next the
    derivative terms (one tensor for both in the plain loss)."""
    eps, dta = loss_consts64()[:2]
    T, B = dang.shape[:2]
    w = _valid_w(valid, T, B)
    dm = dang.double() * w
    sm = (1.0 - dang.double()) * w
    deriv = h_next - h_main + dta * h_main
    return {
        "loss_dang": F.relu(h_bar + eps) * dm, "loss_safe": F.relu(-h_bar) * sm,
        "acc_dang": (h_bar <= 0).double() * dm, "acc_safe": (h_bar > 0).double() * sm,
        "loss_dang_deriv": F.relu(-deriv + eps) * dm, "loss_safe_deriv": F.relu(-deriv) * sm,
        "acc_dang_deriv": (deriv >= 0).double() * dm, "acc_safe_deriv": (deriv > 0).double() * sm,
    }


def _weighted(terms, counts, scale):
    """oracle.finalize_losses' total without the action term, normalised by the given counts."""
    _, _, w_dang, w_safe, w_dang_d, w_safe_d, _ = loss_consts64()
    nd = 1e-5 + float(counts[0])
    ns = 1e-5 + float(counts[1])
    return scale * (w_dang * terms["loss_dang"].sum() / nd + w_safe * terms["loss_safe"].sum() / ns
                    + w_dang_d * terms["loss_dang_deriv"].sum() / nd + w_safe_d * terms["loss_safe_deriv"].sum() / ns)


def dh_reference(h, hmask, map1, src, U, dang, valid, counts, grad_scale=1.0, gscale=None):
    """-> (dh_ref (U,), abs_terms (U,), sums (8,)), float64.

    dh_ref: d loss / d h of every evaluation (h-role + h'-role through map1) times hmask.
    abs_terms: the sum of the absolute values of an evaluation's role terms (barrier, own
    derivative, source slot's derivative), unmasked: the scale of the kernel's rounding error.
    sums: the eight raw sums in the order of cbf_dh_kernel's acc[0..7]. `src` is not needed (map1
    carries the structure); it is accepted so that the call mirrors native.cbf_dh."""
    T, B, N, K = map1.shape
    E = T * B * N * K
    m = map1.reshape(-1).long()
    scale = _scale64(grad_scale, gscale)
    h64 = h[:U].detach().cpu().double()
    dang = dang.cpu().reshape(T, B, N, K)
    valid = None if valid is None else valid.cpu()

    h_eval = h64.clone().requires_grad_(True)
    h_main = h_eval[:E].view(T, B, N, K)
    h_next = h_eval[m].view(T, B, N, K)
    terms = loss_terms(h_main, h_main, h_next, dang, valid)
    _weighted(terms, counts, scale).backward()
    dh_ref = h_eval.grad * hmask[:U].cpu().double()

    # the three roles through separate leaves: their absolute values add up to abs_terms
    leaves = [h64.clone().requires_grad_(True) for _ in range(3)]
    t3 = loss_terms(leaves[0][:E].view(T, B, N, K), leaves[1][:E].view(T, B, N, K), leaves[2][m].view(T, B, N, K),
                    dang, valid)
    _weighted(t3, counts, scale).backward()
    roles = [torch.zeros(U, dtype=torch.float64) if x.grad is None else x.grad for x in leaves]
    assert torch.allclose(roles[0] + roles[1] + roles[2], h_eval.grad, rtol=1e-13, atol=0)
    abs_terms = roles[0].abs() + roles[1].abs() + roles[2].abs()
    sums = torch.stack([terms[k].detach().sum() for k in SUM_NAMES])
    return dh_ref.detach(), abs_terms, sums


def compact_reference(dh, U, E, src, idx, idx1):
    """-> (act (nact,) int64, rec (nact, 4) int32): the evaluations u < U with dh[u] != 0 in index
    order (-0.0 is inactive) and their records {u, e | pass << 31, j, dh bits}: e = u (pass 0,
    u < E) or src[u] (pass 1), j = idx.flat[e] or idx1.flat[e]."""
    dh = dh.detach().cpu()
    act = (dh[:U] != 0).nonzero().reshape(-1)
    pas = act >= E
    e = torch.where(pas, src.cpu().long()[act], act)
    j0 = idx.cpu().reshape(-1).long()[e]
    j1 = idx1.cpu().reshape(-1).long()[e]
    word1 = e - pas.long() * (1 << 31)                       # the pass bit is the int32 sign bit
    bits = dh[:U].float().contiguous().view(torch.int32)[act].long()
    rec = torch.stack([act, word1, torch.where(pas, j1, j0), bits], 1).to(torch.int32)
    return act, rec


def hinge_args(h, map1, U):
    """The four hinge arguments (h + eps, -h, -deriv + eps, -deriv) of every main slot in float64,
    with the (h, h') they come from."""
    eps, dta = loss_consts64()[:2]
    E = map1.numel()
    h64 = h[:U].double()
    hm, hn = h64[:E], h64[map1.reshape(-1).long()]
    deriv = hn - hm + dta * hm
    return (hm + eps, -hm, -deriv + eps, -deriv), hm, hn


def margin_violations(h, map1, U):
    """Number of hinge arguments closer to zero than MARGIN that are not exact ties.

    An exact tie is an argument that is zero in fp32 and float64 alike: h + eps at h = fp32(-eps),
    -h at h = 0, and the derivative arguments at h = h' = 0. Everywhere else |argument| >= MARGIN:
    the kernel forms an argument with at most three fp32 roundings of values |.| <= 2 * H_MAX + 1,
    each at most half an ulp (<= 2**-21), below 1.3e-6 in total, so the fp32 argument has the sign
    of the float64 one. Also returns the number of exact ties per argument."""
    eps = loss_consts64()[0]
    args, hm, hn = hinge_args(h, map1, U)
    both0 = (hm == 0) & (hn == 0)
    tie_ok = (hm == -eps, hm == 0, torch.zeros_like(both0), both0)
    bad, ties = 0, []
    for a, ok in zip(args, tie_ok):
        near = a.abs() < MARGIN
        bad += int((near & ~(ok & (a == 0))).sum())
        ties.append(int((a == 0).sum()))
    return bad, ties


@functools.lru_cache(maxsize=None)
def _graph(T, B, N, K, seed, recomputed):
    """idx (T + recomputed, B, N, K) of moving random states and its dedup maps."""
    g = torch.Generator().manual_seed(seed)
    L_ = math.sqrt(max(1.0, N / 8.0))
    p = torch.rand(B, N, 2, generator=g) * L_
    v = (torch.rand(B, N, 2, generator=g) - 0.5) * 3.0
    Tg = T + int(recomputed)
    S = torch.stack([torch.cat([p + 0.25 * t * v, v], -1) for t in range(Tg)])
    idx = torch.stack([O.knn_idx(S[t], K) for t in range(Tg)]).to(torch.int32).contiguous()
    map1, src, U = match_reference(idx, T, recomputed=recomputed)
    return idx, map1, src, U


def make_valid(T, B, pattern):
    """(T,B) uint8 or None. "drop": env 0 is valid up to step t0 - 1 and invalid from t0 =
    max(1, T // 2) on (T = 1 has no such step: all valid); "dead": the last env is invalid from
    step 0."""
    if pattern == "none":
        return None
    valid = torch.ones(T, B, dtype=torch.uint8)
    if pattern == "drop":
        valid[max(1, T // 2):, 0] = 0
    elif pattern == "dead":
        valid[:, B - 1] = 0
    elif pattern != "ones":
        raise ValueError(pattern)
    return valid


@functools.lru_cache(maxsize=None)
def make_case(T, B, N, K, seed, recomputed, valid_pattern):
    """One input set of cbf_dh (CPU tensors; shared between tests: treat as read-only).

    h is N(0,1) clipped to |h| <= H_MAX, 0 where hmask == 0 (about 10 %); dang about 30 % ones.
    Planted exact ties: slots with h = h' = 0 (safe and dangerous), dangerous slots with
    h = fp32(-eps_dang). Asserts the margin condition."""
    idx, map1, src, U = _graph(T, B, N, K, seed, recomputed)
    E = T * B * N * K
    g = torch.Generator().manual_seed(seed + 1000)
    h = torch.zeros(2 * E)
    h[:U] = torch.randn(U, generator=g).clamp_(-H_MAX, H_MAX)
    hmask = torch.zeros(2 * E, dtype=torch.uint8)
    hmask[:U] = (torch.rand(U, generator=g) >= 0.1).to(torch.uint8)
    h[hmask == 0] = 0.0                          # masked evaluations hold h = 0
    dang =(torch.rand(T, B, N, K, generator=g) < 0.3).to(torch.uint8)
    m = map1.reshape(-1)
    pick = torch.randperm(E, generator=g)[:12].tolist()
    eps32 = torch.tensor(native.LOSS_CONSTS[0], dtype=torch.float32)
    for q, e in enumerate(pick[:8]):             # h = h' = 0, flags mixed (hmask stays as drawn)
        h[e] = 0.0
        h[m[e]] = 0.0
        dang.view(-1)[e] = q % 2
    for e in pick[8:]:                           # h + eps == 0 on dangerous slots
        h[e] = -eps32
        hmask[e] = 1
        dang.view(-1)[e] = 1
    valid =make_valid(T, B, valid_pattern)
    w = _valid_w(valid, T, B)
    counts = torch.stack([(dang.double() * w).sum(), ((1.0 - dang.double()) * w).sum()]).float()
    bad, ties = margin_violations(h, map1, U)
    assert bad == 0, f"seed {seed}: {bad} hinge arguments within {MARGIN} of zero"
    assert ties[0] > 0 and ties[1] > 0 and ties[3] > 0, ties
    assert float(h.abs().max()) <= H_MAX
    return dict(T=T, B=B, N=N, K=K, E=E, U=U, idx=idx, map1=map1, src=src, h=h, hmask=hmask, dang=dang, valid=valid,
                counts=counts, recomputed=recomputed)


def case_seed(shape):
    return 11 + SHAPES.index(tuple(shape))


# ------------------------------------------------------------------------- cbf_match on planted lists
def match_reference_fast(idx, T, recomputed=False):
    """ops.dedup.match_reference without a Python loop over slots (broadcast compares, one cumulative
    sum for the extras' ranks): the same (map1 (T, B, N, K), src (2E,), nev) as int64 tensors.
    tests/test_dedup.py pins it to the loop reference on every small case."""
    _, B, N, K = idx.shape
    BNK = B * N * K
    E = T * BNK
    idx = idx.long().cpu()
    m = torch.full((T, B, N, K), -1, dtype=torch.long)
    if T > 1:
        if recomputed:
            m[:T - 1] = torch.arange(K)
        else:
            eq = idx[:T - 1].unsqueeze(-1) == idx[1:T].unsqueeze(-2)              # (T-1, B, N, K, K'): slot k vs next slot q
            m[:T - 1] = (eq.long() * torch.arange(1, K + 1)).max(-1).values - 1     # the last matching slot, -1 without one
    m = m.reshape(-1)
    e = torch.arange(E)
    un = m < 0
    rank = torch.cumsum(un.long(), 0) - un.long()                                  # extras are ordered by (t, b, i, k)
    u = torch.where(un, E + rank, e - e % K + BNK + m)
    src = torch.full((2 * E,), -1, dtype=torch.long)
    src[u] = e
    return u.view(T, B, N, K), src, E + int(un.sum())


def planted_lists(T, B, N, K, n_nodes=None, seed=0, recomputed=False, keep=0.9, dup=False):
    """Synthetic neighbour lists (T + recomputed, B, N, K) int32: slot 0 is the agent itself, the
    other slots distinct ids below the node count (agent i's candidates are i + 1 .. i + P mod n_nodes,
    P = min(n_nodes - 1, 64)); each step keeps each non-self slot's neighbour with probability `keep`
    -- in a shuffled slot -- and otherwise replaces it by an id the row did not hold. dup (K >= 3): in
    the last step every third agent's last slot repeats its slot 1, so a neighbour kept from the step
    before matches two slots of the next list and the LAST one must win (only the last step, which
    is nobody's current list but its own all-extras one, so the maps stay injective)."""
    Nn = N if n_nodes is None else n_nodes
    P = min(Nn - 1, 64)
    assert Nn >= N and (K == 1 or P >= 2 * (K - 1)), "not enough candidates to replace every slot"
    g = torch.Generator().manual_seed(seed)
    Tg = T + int(recomputed)
    me = torch.arange(N).view(1, N, 1).expand(B, N, 1)
    out = torch.empty(Tg, B, N, K, dtype=torch.int32)
    held = None                                                     # (B, N, P) bool: offsets in the row
    for t in range(Tg):
        score = torch.rand(B, N, P, generator=g)
        if held is not None:
            drop = held & (torch.rand(B, N, P, generator=g) >= keep)
            score = torch.where(held & ~drop, score - 2.0, score)   # kept neighbours stay
            score = torch.where(drop, score + 2.0, score)           # replaced ones leave the row
        off = score.argsort(-1)[..., :K - 1]                        # K - 1 distinct offsets, in random order
        held = torch.zeros(B, N, P, dtype=torch.bool).scatter_(-1, off, True)
        out[t] = torch.cat([me, (me + 1 + off) % Nn], -1).to(torch.int32)
    if dup:
        assert K >= 3 and T >= 2 and not recomputed
        out[T - 1, :, 0::3, K - 1] = out[T - 1, :, 0::3, 1]
    return out.contiguous()


# (T, B, N, K, node count): every K at (3, 2, 50); rows T B N around a 256-row block; no next step;
# the (T-1) B N = 400 and B N K boundaries inside blocks
MATCH_CASES = [(3, 2, 50, K, 50, False) for K in (1, 2, 5, 8, 12, 16)] + \
              [(1, 1, 1, 12, 64, False), (1, 3, 85, 12, 85, False), (2, 1, 128, 5, 128, False), (1, 1, 257, 3, 257, False),
               (1, 2, 40, 12, 40, False), (3, 1, 200, 12, 200, False),
               # duplicate ids in the last list: first match and last match differ (reuse mode only)
               (3, 2, 50, 6, 50, True)]
MATCH_BIG = (3, 1, 174850, 2, 174850, False)         # 2,050 blocks: block_sum_prefix's second trip; 1.05 M slots


def match_case_id(c):
    return "T{}-B{}-N{}-K{}".format(*c[:4]) + ("-dup" if c[5] else "")


@functools.lru_cache(maxsize=None)
def match_case(case, recomputed):
    """(idx, the reference's map1, src, nev) of a planted-list case; the loop-free reference (the big
    case could not afford the loop)."""
    T, B, N, K, Nn, dup = case
    idx = planted_lists(T, B, N, K, n_nodes=Nn, seed=31 + K + N, recomputed=recomputed, dup=dup and not recomputed)
    return (idx,) + tuple(match_reference_fast(idx, T, recomputed=recomputed))
