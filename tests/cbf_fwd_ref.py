"""Float64 reference of ONE CBF h forward call (csrc/cbf.hip: cbf_hfwd_kernel over a deduplicated
evaluation list, cbf_fwd_kernel over the main slots; csrc/refine.hip: the safety filter's forward at
s') with a propagated, not fitted, error bound per evaluation.

Parameters as the kernel receives them (``kernel_params``), each read from the packing code:

* ``cbf_net.{0,2,4}.weight``: ops/layout.py ``cbf_packer`` (w1f / w2 / w3 fragments) and ``cbf_rm`` (the
  row-major W2 | W3 images) gather them into the 16-bit buffers of ops/weights.py ``PackedWeights``
  (``_buf16``): rounded to bf16 / fp16 in the 1-pass builds; the x3 build stores [hi | lo] planes
  (``x3_frags`` / ``x3_planes``), i.e. the fp32 value to 2^-17 relative, which TAU covers: unrounded.
* ``cbf_net.0.bias``: ``cbf_packer``'s ``w1f`` returns ``b1 + o`` for the slot ``cbf_w1_slot`` marks
  ``('b',)`` -- the bias is a column of the layer-1 fragment, multiplied by the constant-1 feature lane
  of ``cbf_edge_frag`` (csrc/cbf_edge.h: f[6] / f[7] = 1): rounded like a weight.
* ``cbf_net.2.bias``, ``cbf_net.4.bias``, ``cbf_net.6.weight``, ``cbf_net.6.bias``: ``cbf_vec_index``
  (b2 | b3 | w4 | b4), gathered into the fp32 side vector ``_buf32`` (``cbf_v``): fp32 in every build.

Features (``features``), formed in fp32 in the order of ``cbf_edge`` (contraction is off in cbf.hip and
refine.hip, so each line is one IEEE operation and the fp32 tensors here are the kernel's bits):
rp = p_i - p_j, rv = v_i - v_j, eye = [j == i], sq = rp_0^2 + rp_1^2 (+ rp_2^2) in coordinate order,
d = sqrt(sq + eps) with eps = fp32(CBF_DIST_EPS_COORD * D) as the launcher passes it, dfeat = d -
fp32(DIST_MIN_THRES), mask = d <= fp32(OBS_RADIUS). Then cast to float64. The mask is the fp32
decision and is asserted exactly.

Layers (``forward``), float64, x = [rp, rv, eye, dfeat] (oracle.cbf_features' column order), through
``ctrl_fwd_ref._layer``::

    z1 = x W1^T + b1            e1 = u1 (|x| |W1|^T + |b1|) + ex |W1|^T
    z2 = relu(z1) W2^T + b2     e2 = u2 (|relu z1| |W2|^T + |b2|) + e1 |W2|^T
    z3 = relu(z2) W3^T + b3     e3 = u2 (|relu z2| |W3|^T + |b3|) + e2 |W3|^T
    h  = relu(z3) . w4 + b4     e_h = e3 . |w4| + 66 * 2^-24 (|relu z3| . |w4| + |b4|)

Derivation of each term:

* u1 (|x| |W1|^T + |b1|): layer 1 is one MFMA chain of products x_c W1[o, c] and 1 * b1[o] summed in
  fp32. The input is split into a 16-bit hi and its residual lo (``split_h16``), so x is represented to
  2^-16 (bf16) / 2^-22 (fp16) relative; in x3 the weights carry a lo plane too and the product is
  hi hi + hi lo + lo hi, dropping lo lo <= 2^-16 relative. Every product therefore carries at most
  ~2^-16 relative error, the fp32 accumulation of <= 16 terms another 16 * 2^-24 = 2^-20 of the sum of
  absolute terms: together inside TAU = 3e-5 ~ 2^-15 (ops/selfcheck.py), the unit ``unit_errors`` gives.
* ex |W1|^T: an input off by ex_c moves z1[o] by at most ex_c |W1[o, c]|.
* u2 (|relu z| |W|^T + |b|): x3 -- activations and weights both [hi | lo], three products, as above:
  TAU. 1-pass -- ``to_pk_relu`` rounds the activation to the 16-bit type (half an ulp: 2^-9 / 2^-12
  relative; the unit 2^-8 / 2^-11 of ``unit_errors`` is one full ulp and also covers the rounding of
  an activation that itself is off by e), the weights are exact 16-bit values, the fp32 accumulation
  of 64 / 128 terms adds at most 128 * 2^-24 = 2^-17 of the absolute sum, inside the slack between
  half and full ulp. The bias is the fp32 accumulator's initial value.
* e |W|^T: relu is 1-Lipschitz, so an error e of the pre-activations reaches the next layer through
  |W| at most.
* e3 . |w4|: the same through the head's weights.
* 66 * 2^-24 (|relu z3| . |w4| + |b4|): the head is fp32 -- 32 multiply-adds per lane (fused in
  cbf_hfwd / refine, a product and a sum rounding each in cbf_fwd's cbf_mlp), two lanes, so at most
  64 roundings of half an ulp (2^-24 relative to a partial sum no larger than the sum of absolute
  terms) on any path to the result, one more for the half-wave add, one for the bias add: 66.
* ex: zero on the relative coordinates of a direct call (each is one IEEE subtraction of the kernel's
  own inputs, reproduced here bit for bit), two fp32 ulp of d on the dfeat channel (sqrtf and the
  reference's sqrt may each be one ulp off the correctly rounded value). The safety filter's s' adds
  two fp32 ulp of each relative coordinate (``filter_features``).

``contract`` is the per-evaluation check of one call: the mask byte exactly, h bit-equal to +0.0 where
the mask is 0, |h - ref| <= e_h where it is 1. No evaluation is exempt: h is continuous in every
pre-activation, so there is no relu tie list and no trimmed share.

The bound above is a worst case (it charges every 1-pass activation a full 16-bit ulp: e_h reaches half
of max |h| in bf16 at the default initialisation). The 1-pass builds are therefore held to a second
reference as well, ``forward_rounded``: the same layers with relu(z1), relu(z2) rounded to the 16-bit type
as the kernel rounds them, and a bound made of the input split, the fp32 accumulation and only those
activations whose rounding can actually differ (its docstring has the derivation): |h - h16| <= e16,
a few 1e-4 for most evaluations. Both must hold; x3 has the first alone.

Every bound here is derived, none fitted: an evaluation outside its bound means a term is missing
from the derivation (add it here with its reason) or the kernel is wrong. Measured err / bound
ratios: docs/PERF.md, "CBF forward oracle"."""
import torch

from macbf_gnn_amd import config as C

from ctrl_fwd_ref import DT16, F32, U16, _layer, ulp16, unit_errors  # noqa: F401  (shared, not copied)

ROUNDED = ("cbf_net.0.weight", "cbf_net.2.weight", "cbf_net.4.weight", "cbf_net.0.bias")
HEAD_OPS = 66                       # fp32 roundings on any path through the head (module docstring)
U32 = 2.0 ** -24


def kernel_params(p, prec):
    """The CBF parameters as the `prec` build's kernels receive them (module docstring), float64, CPU."""
    out = {}
    for k, v in p.items():
        v = v.detach().float().cpu()
        if prec != "fp32" and k in ROUNDED:
            v = v.to(DT16[prec]).float()
        out[k] = v.double()
    return out


def ulp32(v):
    """One fp32 ulp at |v| (float64 tensor)."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))          # |v| = m 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(v), e - 24)


def features(si, sj, eye, dtype=torch.float32):
    """si, sj (..., 2D) node states, eye (...) bool -> dict: x (..., 2D + 2) float64 = [rp, rv, eye,
    dfeat], d (...), mask (...) bool, ex (..., 2D + 2) float64 input error. Formed in `dtype`: fp32 is
    the kernels' arithmetic (the mask is then the fp32 decision); float64 is oracle.cbf_features'
    (the CPU test's comparison with the oracle)."""
    si, sj = si.to(dtype), sj.to(dtype)
    D = si.shape[-1] // 2
    rel = si - sj
    sq = rel[..., 0] * rel[..., 0]
    for q in range(1, D):
        sq = sq + rel[..., q] * rel[..., q]
    d = torch.sqrt(sq + torch.tensor(C.CBF_DIST_EPS_COORD * D, dtype=dtype))
    dfeat = d - torch.tensor(C.DIST_MIN_THRES, dtype=dtype)
    mask = d <= torch.tensor(C.OBS_RADIUS, dtype=dtype)
    x = torch.cat([rel, eye.to(dtype).unsqueeze(-1), dfeat.unsqueeze(-1)], -1).double()
    ex = torch.zeros_like(x)
    ex[..., -1] = 2.0 * ulp32(d.double())
    return dict(x=x, d=d, mask=mask, ex=ex)


def filter_features(s, a, idx, nodes_static=None):
    """The safety filter's first-iteration features at s' = s + dt [v, a] (delta = 0), formed in fp32 in
    refine_edge's expression order: p' = p + v * dt, v' = v + u * dt per node (u = a for agents, 0 for
    obstacle nodes), then the differences. s (B, N, 2D), a (B, N, D), idx (B, N, K) into the nodes
    (agents, then nodes_static (B, M, D) obstacle points) -> features' dict, ex extended by two fp32 ulp
    of each relative coordinate (the two roundings of each s' coordinate are reproduced here, the ulps
    cover a reference that takes s' as given) and their sum on the dfeat channel (|dd / drp_q| <= 1)."""
    s, a = s.detach().float().cpu(), a.detach().float().cpu()
    B, N, D2 = s.shape
    D = D2 // 2
    dt = torch.tensor(C.TIME_STEP, dtype=torch.float32)
    u = a
    nodes = s
    if nodes_static is not None:
        o = nodes_static.detach().float().cpu()
        nodes = torch.cat([s, torch.cat([o, torch.zeros_like(o)], -1)], 1)
        u = torch.cat([a, torch.zeros(B, o.shape[1], D)], 1)
    pn = nodes[..., :D] + nodes[..., D:] * dt
    vn = nodes[..., D:] + u * dt
    sn = torch.cat([pn, vn], -1)
    il = idx.detach().cpu().long()
    K = il.shape[-1]
    sj = torch.gather(sn, 1, il.reshape(B, -1, 1).expand(-1, -1, D2)).reshape(B, N, K, D2)
    si = sn[:, :N].unsqueeze(2).expand(-1, -1, K, -1)
    f = features(si.contiguous(), sj, il == torch.arange(N).view(1, N, 1))
    er = 2.0 * ulp32(f["x"][..., :D2])
    f["ex"][..., :D2] = er
    f["ex"][..., -1] += er[..., :D].sum(-1)
    return f


def forward(p, x, ex, prec, emulate=None):
    """-> (h (...) float64 UNMASKED, e_h, the head's sum of absolute terms). emulate: a 16-bit dtype --
    round relu(z1), relu(z2) to it as oracle.emulate_bf16 does (the CPU test's comparison with the
    emulating oracle; not a bound)."""
    u1, u2 = unit_errors(prec)
    rnd = (lambda t: t) if emulate is None else (lambda t: t.to(emulate).double())
    z1, e1 = _layer(x, ex, p["cbf_net.0.weight"], p["cbf_net.0.bias"], u1)
    z2, e2 = _layer(rnd(torch.relu(z1)), e1, p["cbf_net.2.weight"], p["cbf_net.2.bias"], u2)
    z3, e3 = _layer(rnd(torch.relu(z2)), e2, p["cbf_net.4.weight"], p["cbf_net.4.bias"], u2)
    w4 = p["cbf_net.6.weight"].reshape(-1)
    b4 = p["cbf_net.6.bias"].reshape(())
    r3 = torch.relu(z3)
    h = r3 @ w4 + b4
    scale = r3 @ w4.abs() + b4.abs()
    e_h = e3 @ w4.abs() + HEAD_OPS * U32 * scale
    return h, e_h, scale


U_SPLIT = {"bf16": 2.0 ** -18, "fp16": 2.0 ** -24}      # |x - hi - lo| / |x| of split_h16 (forward_rounded)


def _round_act(z, dz, dt):
    """relu and the kernel's 16-bit rounding of a pre-activation known to within dz -> (value, bound).
    relu and round-to-nearest are monotone, so the kernel's rounded activation lies between the rounded
    relu(z - dz) and relu(z + dz): the bound is the distance to the farther of the two -- the plain
    propagated dz where no rounding boundary is in reach, one more 16-bit step where one is."""
    r = torch.relu(z).to(dt).double()
    lo = torch.relu(z - dz).to(dt).double()
    hi = torch.relu(z + dz).to(dt).double()
    return r, torch.maximum(r - lo, hi - r)


def forward_rounded(p, x, ex, prec):
    """The 1-pass builds' own arithmetic in float64 -> (h UNMASKED, bound): a second, tighter reference
    next to ``forward``, whose bound charges every activation a full 16-bit ulp whether or not its
    rounding can differ. Here relu(z1) and relu(z2) are rounded to the 16-bit type as ``to_pk_relu``
    rounds them (round to nearest even, csrc/common.h ``to_h16x16``), so what is left between the kernel
    and this reference is

    * the layer-1 input split (``split_h16``): hi = RN16(x), the residual x - hi is exact in fp32, lo =
      RN16(x - hi), so |x - hi - lo| <= 2^-9 * 2^-9 |x| = 2^-18 |x| in bf16 and 2^-12 * 2^-12 |x| = 2^-24 |x| in
      fp16, plus 2^-25 absolute where the fp16 lo is subnormal: added to ex;
    * the fp32 accumulation of an MFMA chain: the products of two 16-bit values are exact in fp32, each of
      the n additions (n = 16 slots, 64 or 128 inputs, + the initial value) is off by at most one fp32
      ulp (2^-23) of a partial sum no larger than the sum of absolute terms: u = (n + 1) 2^-23;
    * the activations whose rounding can differ because the kernel's fp32 pre-activation is off by the
      above (``_round_act``), propagated through |W| like any other error;
    * the fp32 head, as in ``forward``."""
    dt = DT16[prec]
    w1, w2, w3 = (p[f"cbf_net.{i}.weight"] for i in (0, 2, 4))
    ex = ex + U_SPLIT[prec] * x.abs() + (2.0 ** -25 if prec == "fp16" else 0.0)
    ex[..., -2] = 0.0                                           # eye: 0 or 1, exact
    z1, d1 = _layer(x, ex, w1, p["cbf_net.0.bias"], 17 * 2.0 ** -23)
    a1, da1 = _round_act(z1, d1, dt)
    z2, d2 = _layer(a1, da1, w2, p["cbf_net.2.bias"], (w2.shape[1] + 1) * 2.0 ** -23)
    a2, da2 = _round_act(z2, d2, dt)
    z3, d3 = _layer(a2, da2, w3, p["cbf_net.4.bias"], (w3.shape[1] + 1) * 2.0 ** -23)
    w4 = p["cbf_net.6.weight"].reshape(-1)
    b4 = p["cbf_net.6.bias"].reshape(())
    r3 = torch.relu(z3)
    return r3 @ w4 + b4, d3 @ w4.abs() + HEAD_OPS * U32 * (r3 @ w4.abs() + b4.abs())


def reference(p, prec, f, emulate=None):
    """features' dict -> dict: h float64 masked, e_h, mask, d, x, head_scale; in the 1-pass builds also
    h16 / e16, the rounded-activation reference and its bound (``forward_rounded``)."""
    h, e_h, scale = forward(p, f["x"], f["ex"], prec, emulate)
    m = f["mask"].double()
    out = dict(h=h * m, e_h=e_h, mask=f["mask"], d=f["d"], x=f["x"], head_scale=scale)
    if prec != "fp32" and emulate is None:
        h16, e16 = forward_rounded(p, f["x"], f["ex"], prec)
        out.update(h16=h16 * m, e16=e16)
    return out


def list_edges(idx, idx1, src, U):
    """The evaluation list's first U entries -> dict of (U,) int64: pas (1 = extra), e (main slot),
    t, b, i, k, j (the neighbour: idx1.flat[e] for extras, idx.flat[e] otherwise), step (t + pas)."""
    T, B, N, K = idx.shape
    E = T * B * N * K
    u = torch.arange(U)
    pas = (u >= E).long()
    e = torch.where(pas.bool(), src.detach().cpu().long()[:U], u)
    assert int(e.min()) >= 0 and int(e.max()) < E, "evaluation list names a slot outside [0, E)"
    k = e % K
    i = (e // K) % N
    b = (e // (K * N)) % B
    t = e // (K * N * B)
    j = torch.where(pas.bool(), idx1.detach().cpu().reshape(-1).long()[e], idx.detach().cpu().reshape(-1).long()[e])
    return dict(pas=pas, e=e, t=t, b=b, i=i, k=k, j=j, step=t + pas)


def list_reference(p, prec, S, idx, idx1, src, U, emulate=None, dtype=torch.float32):
    """S (T + 1, B, Nn, 2D) fp32 states -> dict: h (U,) float64 masked, e_h, mask (U,) bool, d, le."""
    S = S.detach().float().cpu()
    le = list_edges(idx, idx1, src, U)
    si = S[le["step"], le["b"], le["i"]]
    sj = S[le["step"], le["b"], le["j"]]
    f = features(si, sj, le["i"] == le["j"], dtype)
    return dict(reference(p, prec, f, emulate), le=le)


def check_values(ref, h, mask, what="", rows=None, lo=0, hi=None):
    """The three per-evaluation assertions on entries [lo, hi) of flat outputs h (float32) and mask
    (uint8 or None: a kernel without a mask output) against ref = dict(h, e_h, mask) (flat, float64 /
    bool). rows: callable n -> tuple describing flat entry n, for the failure report.
    In the 1-pass builds (ref carries h16 / e16) the in-radius entries are held to the rounded-activation
    reference as well: |h - h16| <= e16. -> dict of the worst err / bound over the in-radius entries:
    h, and h16 where checked."""
    hi = ref["h"].numel() if hi is None else hi
    sl = slice(lo, hi)
    hk = h.detach().cpu().reshape(-1)[sl]
    rm = ref["mask"].reshape(-1)[sl]
    assert hk.dtype == torch.float32 and hk.numel() == hi - lo, what
    desc = (lambda n: (n,)) if rows is None else rows
    if mask is not None:
        mk = mask.detach().cpu().reshape(-1)[sl]
        badm = mk != rm.to(mk.dtype)
        assert not bool(badm.any()), (what, "mask bytes differ from the fp32 decision", int(badm.sum()),
                                      [desc(lo + int(n)) + (int(mk[n]), int(rm[n])) for n in badm.nonzero().reshape(-1)[:6]])
    bits = hk.view(torch.int32)
    badz = ~rm & (bits != 0)
    assert not bool(badz.any()), (what, "h outside the radius is not +0.0", int(badz.sum()),
                                  [desc(lo + int(n)) + (float(hk[n]),) for n in badz.nonzero().reshape(-1)[:6]])
    out = {}
    for key, kh, ke, msg in (("h", "h", "e_h", "h outside the bound"),
                             ("h16", "h16", "e16", "h outside the rounded-activation bound")):
        if kh not in ref:
            continue
        rh, re = ref[kh].reshape(-1)[sl], ref[ke].reshape(-1)[sl]
        assert bool(torch.isfinite(re).all()) and bool((re > 0).all()), (what, key, "reference bound not finite and positive")
        err = (hk.double() - rh).abs()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
        ratio = torch.where(rm, err / re, torch.zeros_like(err))
        bad = ratio > 1.0
        if bool(bad.any()):
            worst = ratio.argsort(descending=True)[:6]
            raise AssertionError((what, msg, int(bad.sum()),
                                  [desc(lo + int(n)) + (float(hk[n]), float(rh[n]), float(re[n])) for n in worst if bool(bad[n])]))
        out[key] = float(ratio.max()) if ratio.numel() else 0.0
    return out


def contract(p, prec, S, idx, idx1, src, U, h, mask, u_begin=0, u_end=None, what=""):
    """Every evaluation u_begin <= u < (u_end or U) of one cbf_hfwd call (module docstring): p =
    kernel_params(.., prec), S (T + 1, B, Nn, 2D) fp32 states, idx / idx1 (T, B, N, K), src (>= U,),
    h (>= U,) float32, mask (>= U,) uint8. A failure reports up to 6 worst entries
    (u, t, b, i, k, j, got, ref, bound). -> check_values' dict of worst err / bound."""
    ref = list_reference(p, prec, S, idx, idx1, src, U)
    le = ref["le"]
    rows = lambda u: (u,) + tuple(int(le[c][u]) for c in ("t", "b", "i", "k", "j"))
    hi = U if u_end is None else u_end
    return check_values(ref, h.reshape(-1)[:U], None if mask is None else mask.reshape(-1)[:U], what, rows, u_begin, hi)
