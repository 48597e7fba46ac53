"""The CBF h forward (csrc/cbf.hip: cbf_hfwd_kernel, cbf_fwd_kernel; csrc/refine.hip: the safety filter's
forward at s') pinned to a float64 oracle of the SAME inputs, evaluation by evaluation
(tests/cbf_fwd_ref.py: the reference, its propagated error bound and the contract;
tests/test_cbf_fwd_ref.py pins that reference to oracle.cbf_forward on the CPU and asserts the shared
cases' conditions).

The other h tests bound whole tensors (one wrong evaluation hides behind a few thousand right ones) and
launch cbf_hfwd directly at one shape only. Here:

* direct native.cbf_hfwd calls on the shared cases (tests/cbf_fwd_cases.py: K = 1, 5, 8, 12, 16, 3-D with
  obstacle neighbours, 300 agents; a pair on adjacent bit patterns either side of the radius, duplicate
  records) x three evaluation lists (cbf_match's reference, the recomputed mode, a planted non-monotone
  list): every case in fp32, k8 / k12 / k16 / 3d_obs in bf16, k12 / k16 in fp16; grids of 1, 3, 9 and the
  default number of workgroups; host ranges step by step as the rollout driver launches them. S sits in a
  NaN-padded allocation whose env and step strides both differ from the dense ones, src holds wrong but
  valid slots wherever the kernel must not read it, h / mask carry sentinels wherever it must not write.
* every evaluation: the mask byte exactly the fp32 decision, h bit-equal to +0.0 outside the radius,
  |h - ref| <= e_h inside; in the 1-pass builds also |h - h16| <= e16 against the reference that rounds the
  activations as the kernel does (cbf_fwd_ref.forward_rounded: a few 1e-4 where e_h is a few 1e-2). No
  evaluation is exempt.
* tolerance-free: bit-equal across the grids, across host ranges and shifted range starts, between the
  two duplicate slots, and under a roll of the agents by 5.
* direct native.cbf_fwd calls (the safety filter's h(s_t), the two-kernel training path), the safety
  filter's own forward at s', and the engine's stored evaluation list after one training step.

Measured err / bound ratios: docs/PERF.md ("CBF forward oracle")."""
import copy
import functools

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd.models import Controller
from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.refine import safety_filter
from macbf_gnn_amd.ops.weights import PackedWeights
from macbf_gnn_amd.utils.params import FlatParams
from numerics import ratio_log

import cbf_fwd_cases as FC
import cbf_fwd_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
PAD = FC.PAD
H_SENT, M_SENT = 7.0, 77
_NETS = {}

# every case in fp32; k8, k12, k16, 3d_obs also in bf16; k12, k16 also in fp16
PRECS = [(n, "fp32") for n in FC.ALL] + [(n, "bf16") for n in ("k8", "k12", "k16", "3d_obs")] + \
        [(n, "fp16") for n in ("k12", "k16")]
DIRECT = [(n, m, p) for n, p in PRECS for m in FC.MODES]
GRIDS = (1, 3, 9, None)


def _cbf_params(fp, prec):
    return R.kernel_params({pn: fp.flat[o:o + n].view(shape) for m, pn, shape, o, n in fp.specs if m == "cbf"}, prec)


def _nets(D, prec):
    """The shared default-initialised CBF packed for `prec` -> (packed images, the parameters as that
    build's kernels receive them, float64)."""
    if (D, prec) not in _NETS:
        fp = FlatParams({"controller": Controller(2 * D).to(DEV), "cbf": copy.deepcopy(FC.cbf(D)).to(DEV)}, device=DEV)
        _NETS[(D, prec)] = (PackedWeights(fp, D, DTYPES[prec]), _cbf_params(fp, prec))
    return _NETS[(D, prec)]


def _padded_S(S):
    """(T + 1, B, Nn, 2D) CPU states -> a device view of records (T + 1, B, Nn, W) inside a NaN-filled
    allocation: PAD NaN records after every env, PAD more after every step (env and step stride both
    differ from the dense ones) -> (view, the whole allocation)."""
    rec = native.to_records(S)
    T1, B, Nn, W = rec.shape
    env = Nn + PAD
    step = B * env + PAD
    flat = torch.full((T1 * step * W,), float("nan"), device=DEV)
    view = flat.as_strided((T1, B, Nn, W), (step * W, env * W, W, 1))
    view.copy_(rec.to(DEV))
    return view, flat


@functools.lru_cache(maxsize=None)
def _inputs(name, mode, roll=0):
    """Device inputs of one case x list (shared: read-only) -> dict."""
    case, ls = FC.build(name), FC.lists(name, mode)
    src = ls["src"]
    if roll:
        m = FC.roll_slot_map(case, roll)
        src = src.clone()
        src[ls["E"]:ls["U"]] = m[ls["extras"]].to(torch.int32)
        case = FC.rolled(case, roll)
    S, flat = _padded_S(case["S"])
    idx = case["idx"].to(DEV).contiguous()
    idx1 = idx if mode == "match" else case["idx_next"].to(DEV).contiguous()
    return dict(case=case, S=S, flat=flat, flat0=flat.clone(), idx=idx, idx1=idx1, src=src.to(DEV), U=ls["U"], E=ls["E"],
                nev=torch.tensor([ls["U"]], dtype=torch.int32, device=DEV))


@functools.lru_cache(maxsize=None)
def _ref(name, mode, prec):
    """The reference of one case x list x precision, computed once."""
    case, ls = FC.build(name), FC.lists(name, mode)
    _, p = _nets(case["D"], prec)
    return R.list_reference(p, prec, case["S"], case["idx"], ls["idx1"], ls["src"], ls["U"])


def _rows(ref):
    le = ref["le"]
    return lambda u: (u,) + tuple(int(le[c][u]) for c in ("t", "b", "i", "k", "j"))


def _hfwd(inp, prec, num_blocks=None, u_begin=0, u_end=None, out=None, nev=None):
    """One native.cbf_hfwd call into sentinel-filled (or the given) outputs -> (h, mask, workgroups)."""
    pw, _ = _nets(inp["case"]["D"], prec)
    E = inp["E"]
    h, m = out if out is not None else (torch.full((2 * E,), H_SENT, device=DEV),
                                        torch.full((2 * E,), M_SENT, dtype=torch.uint8, device=DEV))
    nb = native.cbf_hfwd(inp["S"], inp["idx"], inp["idx1"], inp["src"], inp["nev"] if nev is None else nev, pw.cbf_w,
                         pw.cbf_off["w1f"], pw.cbf_rm, pw.cbf_v, h, m, num_blocks=num_blocks, u_begin=u_begin, u_end=u_end,
                         prec=prec)
    torch.cuda.synchronize()
    return h, m, nb


def _sentinels(h, m, lo, hi, what):
    """Entries outside [lo, hi) still hold the sentinels."""
    for a, b in ((0, lo), (hi, h.numel())):
        assert bool((h[a:b] == H_SENT).all()) and bool((m[a:b] == M_SENT).all()), (what, f"written outside [{lo}, {hi})")


def _bits_equal(a, b, what):
    (ha, ma), (hb, mb) = a, b
    same = (ha.view(torch.int32) == hb.view(torch.int32)) & (ma == mb)
    assert bool(same.all()), (what, int((~same).sum()), (~same).nonzero().reshape(-1)[:8].tolist())


def _duplicates(name, mode, h, what):
    """The hub's two slots on the duplicate records hold the same h bits (main slots of every step)."""
    case, ref = FC.build(name), _ref(name, mode, "fp32")
    if not case["plants"]:
        return
    le = ref["le"]
    E = case["idx"].numel()
    hb = h.cpu().view(torch.int32)
    n = 0
    for b in range(case["B"]):
        P, R1, R2 = (int(case[k][b]) for k in ("P", "R1", "R2"))
        for t in range(case["T"]):
            sel = (le["pas"] == 0) & (le["b"] == b) & (le["t"] == t) & (le["i"] == P)
            s1 = int((sel & (le["j"] == R1)).nonzero()[0, 0])
            s2 = int((sel & (le["j"] == R2)).nonzero()[0, 0])
            assert s1 < E and s2 < E and int(hb[s1]) == int(hb[s2]) and int(hb[s1]) != 0, (what, "duplicate slots differ", b, t)
            n += 1
    assert n


# --------------------------------------------------------------------------- direct cbf_hfwd calls
@pytest.mark.parametrize("name,mode,prec", DIRECT, ids=[f"{n}-{m}-{p}" for n, m, p in DIRECT])
def test_hfwd_matches_fp64_oracle_per_evaluation(name, mode, prec):
    inp, ref = _inputs(name, mode), _ref(name, mode, prec)
    what = f"hfwd {name} {mode} {prec}"
    h, m, _ = _hfwd(inp, prec)
    U = inp["U"]
    _sentinels(h, m, 0, U, what)
    assert torch.equal(inp["flat"].view(torch.int32), inp["flat0"].view(torch.int32)), (what, "S written")
    ratio_log(what, R.check_values(ref, h[:U], m[:U], what, _rows(ref)))
    _duplicates(name, mode, h, what)


@pytest.mark.parametrize("name,prec", PRECS, ids=[f"{n}-{p}" for n, p in PRECS])
def test_hfwd_grids(name, prec):
    """The planted list at 1 workgroup (one workgroup walks every tile: 0- to 4-tile prologues of the gather
    pipeline, waves without a tile where there are fewer than 8), 3 and 9 (no multiple of the 8 XCDs) and
    the default: the contract at each, and h / mask bit-equal across all four."""
    inp, ref = _inputs(name, "plant"), _ref(name, "plant", prec)
    U = inp["U"]
    outs = []
    for nb in GRIDS:
        what = f"hfwd {name} plant {prec} grid {nb}"
        h, m, used = _hfwd(inp, prec, num_blocks=nb)
        assert nb is None or used == nb
        _sentinels(h, m, 0, U, what)
        r = R.check_values(ref, h[:U], m[:U], what, _rows(ref))
        outs.append((h, m))
    ratio_log(f"hfwd {name} plant {prec} grids", r)
    for o, nb in zip(outs[:-1], GRIDS[:-1]):
        _bits_equal(o, outs[-1], f"hfwd {name} {prec}: grid {nb} differs from the default grid")


@pytest.mark.parametrize("name,prec", PRECS, ids=[f"{n}-{p}" for n, p in PRECS])
def test_hfwd_host_ranges(name, prec):
    """The rollout driver's launches: the main slots step by step over [t BNK, (t + 1) BNK) with a zeroed
    nev and the wrong-but-valid src (BNK is no multiple of 32 in k5, k8, k16, 3d_obs), then the extras
    with u_begin = E. Every entry equals the single whole-list launch bit for bit, nothing outside a
    range is written by its launch, an empty range launches nothing."""
    inp, ref = _inputs(name, "match"), _ref(name, "match", prec)
    case = inp["case"]
    E, U, T = inp["E"], inp["U"], case["T"]
    BNK = E // T
    whole = _hfwd(inp, prec)[:2]
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    h = torch.full((2 * E,), H_SENT, device=DEV)
    m = torch.full((2 * E,), M_SENT, dtype=torch.uint8, device=DEV)
    assert _hfwd(inp, prec, u_begin=BNK, u_end=BNK, out=(h, m), nev=zero)[2] == 0
    _sentinels(h, m, 0, 0, "empty range")
    for t in range(T):
        what = f"hfwd {name} {prec} range step {t}"
        assert _hfwd(inp, prec, u_begin=t * BNK, u_end=(t + 1) * BNK, out=(h, m), nev=zero)[2] > 0
        _sentinels(h, m, 0, (t + 1) * BNK, what)
        assert int(zero) == 0
    _hfwd(inp, prec, u_begin=E, out=(h, m))
    _sentinels(h, m, 0, U, f"hfwd {name} {prec} extras")
    _bits_equal((h, m), whole, f"hfwd {name} {prec}: ranges differ from the whole-list launch")
    R.check_values(ref, h[:U], m[:U], f"hfwd {name} {prec} ranges", _rows(ref))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["k12", "k5"])
def test_hfwd_shifted_range_starts(name, prec):
    """A host range starting 1 .. 31 slots later (every lane phase of the first tile), and the extras
    starting 1 .. 31 evaluations later: every entry still covered keeps its bits, nothing else is written."""
    inp = _inputs(name, "plant")
    E, U = inp["E"], inp["U"]
    BNK = E // inp["case"]["T"]
    whole = _hfwd(inp, prec)[:2]
    for s in range(1, 32):
        for lo, hi, kw in ((BNK + s, 2 * BNK, dict(u_begin=BNK + s, u_end=2 * BNK)), (E + s, U, dict(u_begin=E + s))):
            if lo >= hi:
                continue
            h, m, _ = _hfwd(inp, prec, **kw)
            _sentinels(h, m, lo, hi, f"shift {s}")
            _bits_equal((h[lo:hi], m[lo:hi]), (whole[0][lo:hi], whole[1][lo:hi]), f"hfwd {name} {prec}: start shifted by {s}")


ROLLS = [("k12", "fp32"), ("k12", "bf16"), ("k12", "fp16"), ("3d_obs", "fp32"), ("3d_obs", "bf16")]


@pytest.mark.parametrize("name,prec", ROLLS, ids=[f"{n}-{p}" for n, p in ROLLS])
def test_hfwd_position_independence(name, prec):
    """Rolling the agents of every env by 5 (records moved, idx / idx1 renumbered, the extras naming the
    moved slots) puts every evaluation on another lane and tile and leaves its bits unchanged."""
    base, roll = _inputs(name, "plant"), _inputs(name, "plant", 5)
    E, U = base["E"], base["U"]
    hb, mb, _ = _hfwd(base, prec)
    hr, mr, _ = _hfwd(roll, prec)
    mp = FC.roll_slot_map(base["case"], 5).to(DEV)
    _bits_equal((hb[:E], mb[:E]), (hr[:E][mp], mr[:E][mp]), f"{name} {prec}: main slots change under a roll")
    _bits_equal((hb[E:U], mb[E:U]), (hr[E:U], mr[E:U]), f"{name} {prec}: extras change under a roll")
    assert not torch.equal(hb[:E], hr[:E])


# ---------------------------------------------------------------------------- direct cbf_fwd calls
@functools.lru_cache(maxsize=None)
def _ref_two(name, prec):
    """cbf_fwd's pair of outputs as one list: u < E is h of slot u on s_t, E + e is hn of slot e -- the
    same neighbour idx[e] on s_{t+1}, masked at s_{t+1}."""
    case = FC.build(name)
    _, p = _nets(case["D"], prec)
    E = case["idx"].numel()
    src = torch.cat([torch.zeros(E, dtype=torch.int32), torch.arange(E, dtype=torch.int32)])
    return R.list_reference(p, prec, case["S"], case["idx"], case["idx"], src, 2 * E)


@pytest.mark.parametrize("name,prec", PRECS, ids=[f"{n}-{p}" for n, p in PRECS])
def test_cbf_fwd_matches_fp64_oracle_per_evaluation(name, prec):
    """two=False with h_out alone (the safety filter's h(s_t)) and two=True with h_out and hn_out (the
    two-kernel training path), at 1 workgroup and the default grid: the contract on every entry (no mask
    byte here: +0.0 outside the radius, the bound inside) and bit-equality over the grids and the modes."""
    inp, ref = _inputs(name, "match"), _ref_two(name, prec)
    case = inp["case"]
    pw, _ = _nets(case["D"], prec)
    T, B, N, K = case["idx"].shape
    E = inp["E"]
    outs = []
    for two in (False, True):
        for nb in (1, None):
            what = f"cbf_fwd {name} {prec} two={two} grid {nb}"
            h = torch.full((T, B, N, K), H_SENT, device=DEV)
            hn = torch.full((T, B, N, K), H_SENT, device=DEV) if two else None
            native.cbf_fwd(inp["S"], inp["idx"], pw.cbf_w, pw.cbf_off["w1f"], pw.cbf_v, two=two, h_out=h, hn_out=hn,
                           num_blocks=nb, prec=prec)
            torch.cuda.synchronize()
            r = R.check_values(ref, h, None, what + " h", _rows(ref), 0, E)
            if two:
                full = torch.cat([h.reshape(-1), hn.reshape(-1)])
                rn = R.check_values(ref, full, None, what + " hn", _rows(ref), E, 2 * E)
                r.update({k.replace("h", "hn", 1): v for k, v in rn.items()})
            outs.append((h, hn))
    ratio_log(f"cbf_fwd {name} {prec}", r)
    for h, hn in outs[1:]:
        assert torch.equal(h.view(torch.int32), outs[0][0].view(torch.int32)), "h differs between grids / modes"
    assert torch.equal(outs[2][1].view(torch.int32), outs[3][1].view(torch.int32)), "hn differs between grids"
    assert torch.equal(inp["flat"].view(torch.int32), inp["flat0"].view(torch.int32)), "S written"


# ---------------------------------------------------------------- the safety filter's forward at s'
FILTER = [(n, p) for n in FC.FILTER_CASES for p in ("fp32", "bf16")]


@pytest.mark.parametrize("name,prec", FILTER, ids=[f"{n}-{p}" for n, p in FILTER])
def test_filter_forward_at_next_state(name, prec):
    """safety_filter(loops=1, impl="loop"): the trace's hn against the reference at s' = s + dt [v, a]
    formed in fp32 in refine_edge's order (cbf_fwd_ref.filter_features), every slot."""
    net, s, a, idx, obs = FC.filter_inputs(name)
    cbf = copy.deepcopy(net).to(DEV)
    if prec == "bf16":
        cbf.mfma_dtype = torch.bfloat16
        with torch.no_grad():
            for q in cbf.parameters():
                q.copy_(q.bfloat16().float())
    dev = lambda t: None if t is None else t.to(DEV)
    _, _, _, tr = safety_filter(cbf, dev(s), dev(a), dev(idx), obstacles=dev(obs), loops=1, lr=C.REFINE_LEARNING_RATE,
                                return_trace=True, impl="loop")
    torch.cuda.synchronize()
    p = R.kernel_params(cbf.params_dict(), prec)
    f = R.filter_features(s, a, idx, obs)
    B, N, K = idx.shape
    ref = R.reference(p, prec, f)
    il = idx.reshape(-1)
    rows = lambda n: (n, 0, n // (N * K), (n // K) % N, n % K, int(il[n]))
    r = R.check_values(ref, tr["hn"], None, f"filter {name} {prec}", rows)
    ratio_log(f"filter hn {name} {prec}", {k.replace("h", "hn", 1): v for k, v in r.items()})


# ------------------------------------------------------------------------------ through the engine
def _trainer(**kw):
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.engine.hip_engine import HipEngine
    from macbf_gnn_amd.parallel import DP
    cfg = C.TrainConfig(num_agents=40, num_envs=2, inner_loops=4, seed=5, device="hip", early_stop=False, **kw)
    old = HipEngine.small_rollout
    HipEngine.small_rollout = False
    try:
        tr = Trainer(cfg, device=DEV, dp=DP(device=DEV))
    finally:
        HipEngine.small_rollout = old
    return tr


def _engine_step(monkeypatch, overlap, **kw):
    """One training step -> (the engine, the stored list's ratios): every stored evaluation u < nev of
    the engine's own S / idx / src / hbuf / hmask checked with the contract."""
    monkeypatch.setenv("MACBF_OVERLAP_HFWD", "1" if overlap else "0")
    tr = _trainer(**kw)
    eng = tr.engine
    assert eng.overlap_hfwd == overlap and eng.dedup and eng.reuse
    s0, g, obs = tr.sample()
    eng.step(s0, g, obs)
    torch.cuda.synchronize()
    T = eng.Tmax
    assert eng._last_T in (None, T)
    U = int(eng.nev_dev)
    idx = eng.idx[:T]
    E = idx.numel()
    assert E < U <= 2 * E and eng.K == kw.get("top_k", C.TOP_K)
    S = native.from_records(eng.S[: T + 1]).cpu()
    what = f"engine top_k {eng.K} {eng.prec} overlap {int(overlap)}"
    r = R.contract(_cbf_params(tr.fp, eng.prec), eng.prec, S, idx.cpu(), idx.cpu(), eng.src.cpu(), U, eng.hbuf, eng.hmask,
                   what=what)
    ratio_log(what, r)
    return eng, U


ENGINE = [("k8", dict(top_k=8)), ("k12", dict(top_k=12)), ("k16", dict(top_k=16)), ("k12-bf16", dict(top_k=12, dtype="bf16"))]


@pytest.mark.parametrize("name,kw", ENGINE, ids=[e[0] for e in ENGINE])
def test_engine_step_evaluations_match_the_oracle(name, kw, monkeypatch):
    _engine_step(monkeypatch, False, **dict(kw))


def test_engine_overlapped_hfwd_is_bit_equal(monkeypatch):
    """overlap_hfwd (the main slots evaluated step by step on a side stream during the rollout, the
    extras after the match): the contract, and hbuf / hmask bit-equal to the non-overlapped run of the
    same sample."""
    a, Ua = _engine_step(monkeypatch, False, top_k=12)
    ha, ma = a.hbuf[:Ua].clone(), a.hmask[:Ua].clone()
    b, Ub = _engine_step(monkeypatch, True, top_k=12)
    assert Ua == Ub
    _bits_equal((ha, ma), (b.hbuf[:Ub], b.hmask[:Ub]), "overlapped hbuf differs")
