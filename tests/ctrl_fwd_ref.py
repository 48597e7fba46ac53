"""Float64 reference of ONE controller forward call (csrc/ctrl.hip ctrl_fwd_kernel and its siblings,
the persistent rollout's edge / node phases) with a propagated, not fitted, error bound per entry.

Inputs are what the kernel receives: the node records S (agents first, obstacle nodes after), G, idx
and the controller parameters through ``kernel_params`` -- unrounded fp32 for the x3 build; for the
1-pass builds every weight matrix and the two layer-1 biases (they are folded into the layer-1 MFMA
fragments, ops/layout.py) rounded to bf16 / fp16, the other biases fp32 (the side vector).

Edge phase (``edge_phase``), per edge row x = [s_i - s_j, eye]::

    z1 = x W1^T + b1              e1 = u1 (|x| |W1|^T + |b1|)
    z2 = relu(z1) W2^T + b2       e2 = u2 (|relu z1| |W2|^T + |b2|) + e1 |W2|^T
    hm = relu(z2) * [d < OBS_RADIUS]        (strict; rtie: |d - R| <= 1e-6, selfcheck.edge_oracle's rule)

u is the unit error of one layer's products (``unit_errors``): selfcheck.TAU for every x3 layer and
for layer 1 of the 1-pass builds (its input is split hi / lo), 2^-8 (bf16) / 2^-11 (fp16) for the
other 1-pass layers (one rounded operand pair). relu and max are 1-Lipschitz, so a pooled entry
max_k hm is off by at most the largest e2 of its in-radius rows, plus the storage of the value:
2^-16 |value| for the x3 [hi | lo] row (the 16-ulp truncation by the slot code, 2^-19, is far inside
it), one ulp of the 16-bit type for the single h16 row (``pooled_bound``).

Node phase (``node_phase``), from a GIVEN pooled row (the tests pass the kernel's own hi + lo, so an
edge-phase near-tie cannot leak into the node check): x = [pooled, p - g, v], four layers with the
bound propagated the same way from zero input error, k = 2 sigmoid(y) + 0.2 (|dk / dy| <= 1/2),
a_q = -(k_2q ex_q + k_2q+1 v_q)::

    |da_q| <= 0.5 (e_y[2q] |ex_q| + e_y[2q+1] |v_q|) + 2^-21 (|k_2q ex_q| + |k_2q+1 v_q|)

the last term for __expf, the fp32 ex = p - g and the final fp32 operations.

Forward values get no relu-tie exemption (relu and max are continuous); only rows touching a radius
tie are exempt, and the shared cases (tests/ctrl_fwd_cases.py) contain none but planted, exactly
representable ones, which are asserted exactly instead.

``step_contract`` is the per-row / per-entry check of one call's outputs against all of the above; the
GPU tests (tests/test_gpu_ctrl_fwd_oracle.py) apply it to direct calls and to every stored step of the
engine's rollouts. Reference ops: controller.py:31-63 and the Euler step of train.py:70 of the
reference.

Every bound here is derived, none fitted: a non-tie row outside its bound means a term is missing
from the derivation (add it here with its reason) or the kernel is wrong. Measured err / bound
ratios: docs/PERF.md, "Controller forward oracle"."""
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.selfcheck import TAU

U16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
DT16 = {"bf16": torch.bfloat16, "fp16": torch.float16}
FOLDED_BIASES = ("controller_centr_net.0.bias", "controller_dec_net.0.bias")
NONE = 255                                  # argmax: no positive in-radius row
F32 = lambda x: float(torch.tensor(x, dtype=torch.float32))      # a launch constant as the kernel gets it


def unit_errors(prec):
    """(u of a layer-1 product sum, u of the later layers)."""
    return (TAU, TAU) if prec == "fp32" else (TAU, U16[prec])


def kernel_params(p, prec):
    """The controller parameters as the `prec` build's kernels receive them, float64 on the CPU."""
    out = {}
    for k, v in p.items():
        v = v.detach().float().cpu()
        if prec != "fp32" and (k.endswith("weight") or k in FOLDED_BIASES):
            v = v.to(DT16[prec]).float()
        out[k] = v.double()
    return out


def _layer(x, ex, w, b, u):
    """x W^T + b and its bound u (|x| |W|^T + |b|) + ex |W|^T."""
    w = w.reshape(w.shape[0], -1)
    z = x @ w.t() + b
    e = u * (x.abs() @ w.abs().t() + b.abs())
    if ex is not None:
        e = e + ex @ w.abs().t()
    return z, e


def edge_phase(p, S, idx, N, prec):
    """S (B, Nn, W) records, idx (B, N, K) -> dict: z2 (B, N, K, 128) layer-2 pre-activations, e2 their
    bound, hm = relu(z2) * mask, mask (B, N, K) float64, inr / rtie (B, N, K) bool, d."""
    s = native.from_records(S.detach().cpu()).double()
    B, _, K = idx.shape
    D = s.shape[-1] // 2
    il = idx.detach().cpu().long()
    sj = torch.gather(s, 1, il.reshape(B, -1, 1).expand(-1, -1, 2 * D)).reshape(B, N, K, 2 * D)
    rel = s[:, :N].unsqueeze(2) - sj
    eye = (il == torch.arange(N).view(1, N, 1)).double().unsqueeze(-1)
    x = torch.cat([rel, eye], -1)
    d = torch.sqrt((rel[..., :D] ** 2).sum(-1))
    inr = d < C.OBS_RADIUS
    u1, u2 = unit_errors(prec)
    z1, e1 = _layer(x, None, p["controller_centr_net.0.weight"], p["controller_centr_net.0.bias"], u1)
    z2, e2 = _layer(torch.relu(z1), e1, p["controller_centr_net.2.weight"], p["controller_centr_net.2.bias"], u2)
    mask = inr.double()
    # slots whose edge row is bit-identical to an earlier slot's (duplicate neighbours): the same
    # MFMA inputs give the same row, and the first occurrence wins -- never a near-tie
    same = (x.unsqueeze(3) == x.unsqueeze(2)).all(-1)                          # (B, N, K, K)
    dup = (same & torch.ones(K, K, dtype=torch.bool).tril(-1)).any(-1)
    return dict(z2=z2, e2=e2, hm=torch.relu(z2) * mask.unsqueeze(-1), mask=mask, inr=inr,
                rtie=(d - C.OBS_RADIUS).abs() <= 1e-6, d=d, K=K, D=D, dup=dup)


def ulp16(v, prec):
    """One ulp of the 16-bit type at |v| (fp16: the subnormal spacing 2^-24 below 2^-14)."""
    _, e = torch.frexp(v.abs().clamp_min(1e-300))               # |v| = m 2^e, 0.5 <= m < 1
    if prec == "bf16":
        return torch.ldexp(torch.ones_like(v), e - 8)
    return torch.ldexp(torch.ones_like(v), (e - 11).clamp_min(-24))


def pooled_bound(ed, prec):
    """-> dict over the (B, N, 128) pooled entries: top = max_k hm and its first slot arg, second (the
    second largest hm over the slots that are no exact duplicate of an earlier one, 0 with one slot), zmax = the masked maximum PRE-activation (-inf with no
    in-radius row), bnd = max over the in-radius slots of e2 + the storage term."""
    hm, inr = ed["hm"], ed["inr"].unsqueeze(-1)
    top, arg = hm.max(dim=2)
    first = torch.where(ed["dup"].unsqueeze(-1), torch.zeros((), dtype=torch.float64), hm)      # exact duplicates dropped
    second = first.topk(2, dim=2).values[:, :, 1] if hm.shape[2] >= 2 else torch.zeros_like(top)
    ninf = torch.full((), float("-inf"), dtype=torch.float64)
    zmax = torch.where(inr, ed["z2"], ninf).max(dim=2).values
    emax = torch.where(inr, ed["e2"], torch.zeros((), dtype=torch.float64)).max(dim=2).values
    store = 2.0 ** -16 * top if prec == "fp32" else torch.where(top > 0, ulp16(top, prec), torch.zeros_like(top))
    return dict(top=top, arg=arg, second=second, zmax=zmax, bnd=emax + store, any_in=ed["inr"].any(-1))


def node_phase(p, pooled, S, G, prec):
    """pooled (B, N, 128) float64 (a given row), S records, G (B, N, D) -> dict: y (B, N, 2D) gain
    pre-activations, e_y, gains, a (B, N, D), da, terms = |k_p ex| + |k_v v| per axis, ex, v."""
    B, N, D = G.shape
    s = native.from_records(S.detach().cpu()[:, :N]).double()
    g = G.detach().cpu().double()
    ex, v = s[..., :D] - g, s[..., D:]
    u1, u2 = unit_errors(prec)
    z, e = torch.cat([pooled.double(), ex, v], -1), None
    for li in (0, 2, 4, 6):
        z, e = _layer(z, e, p[f"controller_dec_net.{li}.weight"], p[f"controller_dec_net.{li}.bias"], u1 if li == 0 else u2)
        if li != 6:
            z = torch.relu(z)
    k = 2.0 * torch.sigmoid(z) + 0.2
    kp, kv, ep, ev = k[..., 0::2], k[..., 1::2], e[..., 0::2], e[..., 1::2]
    a = -(kp * ex + kv * v)
    terms = (kp * ex).abs() + (kv * v).abs()
    da = 0.5 * (ep * ex.abs() + ev * v.abs()) + 2.0 ** -21 * terms
    return dict(y=z, e_y=e, gains=k, a=a, da=da, terms=terms, ex=ex, v=v)


def next_state(S, A, N):
    """s + dt [v, A] in float64 from the kernel's own A (dt as the launch passes it, an fp32) and the
    bound 2^-23 (|s| + dt |u|) of its two fp32 roundings -> (Sn_ref (B, N, 2D), bound)."""
    s = native.from_records(S.detach().cpu()[:, :N]).double()
    D = s.shape[-1] // 2
    u = torch.cat([s[..., D:], A.detach().cpu().double()], -1)
    dt = F32(C.TIME_STEP)
    return s + dt * u, 2.0 ** -23 * (s.abs() + dt * u.abs())


def sum_bounds(S, G, Sn, A, N):
    """Per-env fixed-point sums from the kernel's own Sn / A in float64 -> (dist_ref, dist_bound,
    act_ref, act_bound), (B,) float64 in fixed-point units.

    dist: sum_i rint(d_i 2^32), d_i = |p'_i - g_i|; bound sum_i (D + 2) 2^-24 d_i 2^32 + N (the D + 2
    fp32 operations of the norm after an exact-or-rounded difference, one unit per agent for the
    rounding to an integer).
    act: sum_i rint(t_i 2^24), t_i = | |a|^2 - |a_ref|^2 |, a_ref = -(ex + sqrt3 v); bound
    sum_i (2D + 3) 2^-24 (|a|^2 + |a_ref|^2) 2^24 + N: the term is a difference, so its error scales
    with the two squares, not with t_i."""
    s = native.from_records(S.detach().cpu()[:, :N]).double()
    sn = native.from_records(Sn.detach().cpu()[:, :N]).double()
    g = G.detach().cpu().double()
    a = A.detach().cpu().double()
    D = g.shape[-1]
    d = torch.sqrt(((sn[..., :D] - g) ** 2).sum(-1))
    dref = torch.round(d * native.FX_DIST).sum(-1)
    dbnd = ((D + 2) * 2.0 ** -24 * d * native.FX_DIST).sum(-1) + N
    ar = -((s[..., :D] - g) + F32(C.SQRT3) * s[..., D:])
    a2, r2 = (a * a).sum(-1), (ar * ar).sum(-1)
    aref = torch.round((a2 - r2).abs() * native.FX_ACT).sum(-1)
    abnd = ((2 * D + 3) * 2.0 ** -24 * (a2 + r2) * native.FX_ACT).sum(-1) + N
    return dref, dbnd, aref, abnd


def pooled_value(pooled, prec):
    """The kernel's pooled rows (B, N, prow) -> float64 (B, N, 128): hi + lo for x3."""
    pv = pooled[..., :128].detach().cpu().double()
    return pv + pooled[..., 128:256].detach().cpu().double() if prec == "fp32" else pv


def step_contract(p, prec, S, G, idx, pooled, argmax, A, Sn, dist=None, act=None, exact_edges=None, what=""):
    """Every per-row / per-entry assertion of one controller forward call (module docstring and
    tests/test_gpu_ctrl_fwd_oracle.py). p = kernel_params(.., prec); S (B, Nn, W), Sn (B, >= N, W)
    records, G (B, N, D), idx (B, N, K), pooled (B, N, prow) 16-bit, argmax (B, N, 128) uint8, A
    (B, N, D), dist / act (B,) int64 or None. exact_edges (B, N, K) bool: radius-tie edges whose mask is
    exactly representable (planted) and therefore not exempt. -> dict of the worst err / bound ratios."""
    B, N, K = idx.shape
    ed = edge_phase(p, S, idx, N, prec)
    pb = pooled_bound(ed, prec)
    tie = ed["rtie"] if exact_edges is None else ed["rtie"] & ~exact_edges
    free = ~tie.any(-1)                                            # agents with no unplanted radius tie
    pv = pooled_value(pooled, prec)
    am = argmax.detach().cpu().long()
    bnd, top, hm = pb["bnd"], pb["top"], ed["hm"]
    out = {}
    # ---- pooled values
    assert bool(torch.isfinite(pv).all()), what
    perr = (pv - top).abs()
    badp = (perr > bnd) & free.unsqueeze(-1)
    out["pooled"] = float((perr / bnd.clamp_min(1e-300))[free.unsqueeze(-1).expand_as(perr) & (bnd > 0)].max()) if bool((bnd > 0).any()) else 0.0
    assert not bool(badp.any()), (what, "pooled entries outside the bound", int(badp.sum()), badp.nonzero()[:6].tolist(),
                                  float((perr - bnd).max()))
    # ---- argmax slots
    has = am < K
    assert bool((has | (am == NONE)).all()), (what, "argmax neither a slot below K nor 255")
    slot = am.clamp(max=K - 1)
    in_at = torch.gather(ed["inr"], 2, slot) | ~has                # (B, N, 128): the named slot is in radius
    assert bool(in_at.all()), (what, "argmax names an out-of-radius slot", (~in_at).nonzero()[:6].tolist())
    dup_at = torch.gather(ed["dup"], 2, slot) & has
    assert not bool(dup_at.any()), (what, "argmax names the later of two bit-identical rows", dup_at.nonzero()[:6].tolist())
    val = hm.gather(2, slot.unsqueeze(2)).squeeze(2)              # hm_ref at the kernel's slot
    fr = free.unsqueeze(-1)
    far = has & fr & ((top - val) > 2 * bnd)
    assert not bool(far.any()), (what, "argmax value farther than 2 bnd from the maximum", far.nonzero()[:6].tolist())
    clear = fr & (top > bnd) & ((top - pb["second"]) > 2 * bnd)
    wrong = clear & (am != pb["arg"])
    assert not bool(wrong.any()), (what, "argmax differs from a clear reference argmax", int(wrong.sum()),
                                   wrong.nonzero()[:6].tolist())
    must_none = fr & (~pb["any_in"].unsqueeze(-1) | (pb["zmax"] < -bnd))
    must_slot = fr & (pb["zmax"] > bnd)
    assert not bool((must_none & has).any()), (what, "a slot where 255 is required", (must_none & has).nonzero()[:6].tolist())
    assert not bool((must_slot & ~has).any()), (what, "255 where a slot is required", (must_slot & ~has).nonzero()[:6].tolist())
    raw = pooled.detach().cpu().float()
    planes = raw.reshape(B, N, -1, 128)                            # (B, N, 1 | 2, 128)
    nz = (planes != 0).any(2)
    assert not bool((nz & ~has).any()), (what, "255 with a non-zero pooled entry")
    # ---- actions from the kernel's own pooled rows
    nd = node_phase(p, pv, S, G, prec)
    a = A.detach().cpu().double()
    assert bool(torch.isfinite(a).all()), what
    aerr = (a - nd["a"]).abs()
    bada = aerr > nd["da"]
    pos = nd["da"] > 0
    out["A"] = float((aerr[pos] / nd["da"][pos]).max()) if bool(pos.any()) else 0.0
    assert not bool(bada.any()), (what, "actions outside the bound", int(bada.sum()), bada.nonzero()[:6].tolist(), out["A"])
    # ---- next state from the kernel's own A
    snr, snb = next_state(S, A, N)
    sn = native.from_records(Sn.detach().cpu()[:, :N]).double()
    serr = (sn - snr).abs()
    pos = snb > 0
    out["Sn"] = float((serr[pos] / snb[pos]).max()) if bool(pos.any()) else 0.0
    assert not bool((serr > snb).any()), (what, "next state outside the bound", (serr > snb).nonzero()[:6].tolist(), out["Sn"])
    # ---- per-env sums from the kernel's own Sn / A
    if dist is not None:
        dref, dbnd, aref, abnd = sum_bounds(S, G, Sn, A, N)
        derr = (dist.detach().cpu().double() - dref).abs()
        cerr = (act.detach().cpu().double() - aref).abs()
        out["dist"], out["act"] = float((derr / dbnd).max()), float((cerr / abnd).max())
        assert bool((derr <= dbnd).all()), (what, "dist_sum outside the bound", out["dist"])
        assert bool((cerr <= abnd).all()), (what, "act_sum outside the bound", out["act"])
    return out


def near_tie_fractions(ed, pb):
    """Case conditions from the reference alone -> (pool near-tie fraction: top two within 2 bnd and
    top > bnd; zero-ambiguous fraction: the masked maximum pre-activation within +- bnd of zero)."""
    top, bnd = pb["top"], pb["bnd"]
    near = ((top - pb["second"]) <= 2 * bnd) & (top > bnd)
    amb = pb["zmax"].abs() <= bnd
    n = top.numel()
    return int(near.sum()) / n, int(amb.sum()) / n
