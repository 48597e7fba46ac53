"""The controller forward (csrc/ctrl.hip: ctrl_fwd_kernel and its siblings, the persistent small
rollout's edge / node phases) pinned to a float64 oracle of the SAME inputs, per row and per entry
(tests/ctrl_fwd_ref.py: the reference, its propagated error bounds and the step contract;
tests/test_ctrl_fwd_ref.py pins that reference to oracle.controller_forward on the CPU and asserts
the shared cases' conditions).

The other forward tests bound whole tensors (one wrong agent hides behind a few hundred right ones),
compare one kernel path with another bit for bit (a defect both share passes), and never launch a
native kernel with K != 12 while N > K. Here:

* direct native.ctrl_fwd calls on the shared cases (tests/ctrl_fwd_cases.py: K = 1, 5, 8, 12, 16, 3-D
  with obstacle neighbours, 300 agents; planted isolated agents, pairs exactly at and beside the
  radius, duplicate neighbours, an agent at rest): every case in fp32, k12 / k16 / k8 / 3d_obs in bf16, k12 / k16 in fp16; the K = 12 cases
  under 32 / 8 agents per wave (dense rows) and 4 (16-slot tiles). Inputs sit in NaN-padded env
  strides, outputs in sentinel-filled buffers (A = 7, argmax = 77, pooled NaN).
* pooled entries, argmax slots, actions (from the kernel's own pooled rows), next states (from the
  kernel's own actions) and the per-env fixed-point sums (from the kernel's own next states) each
  within its derived bound; the planted features exactly.
* tolerance-free: rolling the agents by 5 leaves every agent's bits unchanged; the 1-pass builds
  without the optional outputs give the same A / Sn / sums.
* through the engine (rollout only, T = 4): the per-step driver at top_k 8 / 12 / 16 and the
  persistent small rollout, every stored step checked from the kernel's own inputs; the scan's
  K = 8 / 16 instantiations with N > K against oracle.knn_idx.

Measured err / bound ratios: docs/PERF.md ("Controller forward oracle")."""
import copy

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.models import CBF
from macbf_gnn_amd.ops import layout as L
from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.weights import PackedWeights
from macbf_gnn_amd.utils.params import FlatParams
from numerics import ratio_log

import ctrl_fwd_cases as CC
import ctrl_fwd_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
PAD = CC.PAD
_NETS = {}

# every case in fp32; k12, k16, k8, 3d_obs also in bf16; k12, k16 also in fp16
DIRECT = [(n, "fp32") for n in CC.ALL] + [(n, "bf16") for n in ("k12", "k16", "k8", "3d_obs")] + \
         [(n, "fp16") for n in ("k12", "k16")]


def _nets(D, prec):
    """The shared default-initialised controller packed for `prec` -> (packed images, the parameters
    as that build's kernels receive them, float64)."""
    if (D, prec) not in _NETS:
        ctrl = copy.deepcopy(CC.controller(D)).to(DEV)
        fp = FlatParams({"controller": ctrl, "cbf": CBF(2 * D).to(DEV)}, device=DEV)
        pw = PackedWeights(fp, D, DTYPES[prec])
        _NETS[(D, prec)] = (pw, _kernel_params(fp, prec))
    return _NETS[(D, prec)]


def _kernel_params(fp, prec):
    return R.kernel_params({pn: fp.flat[o:o + n].view(shape) for m, pn, shape, o, n in fp.specs if m == "controller"}, prec)


def _padded(t, fill, dtype=None):
    """(B, R, C) CPU rows -> a (B, R + PAD, C) device allocation filled with `fill`, rows copied."""
    B, Rr, Cc = t.shape
    buf = torch.full((B, Rr + PAD, Cc), fill, dtype=dtype or t.dtype, device=DEV)
    buf[:, :Rr] = t.to(DEV)
    return buf


def _launch(case, prec, outputs=True):
    """One native.ctrl_fwd call of a built case: NaN-padded records, sentinel-filled outputs ->
    dict of the full (padded) buffers."""
    pw, _ = _nets(case["D"], prec)
    B, N, D, Nn = case["B"], case["N"], case["D"], case["Nn"]
    W, prow = native.rec_width(D), L.pooled_row(prec)
    S = _padded(native.to_records(case["s"]), float("nan"))
    Sn = torch.full((B, Nn + PAD, W), 7.0, device=DEV)
    A = torch.full((B, N + PAD, D), 7.0, device=DEV)
    pooled = torch.full((B, N + PAD, prow), float("nan"), dtype=pw.dtype, device=DEV) if outputs else None
    am = torch.full((B, N + PAD, 128), 77, dtype=torch.uint8, device=DEV) if outputs else None
    dist = torch.zeros(B, dtype=torch.int64, device=DEV)
    act = torch.zeros(B, dtype=torch.int64, device=DEV)
    G = case["G"].to(DEV).contiguous()
    idx = case["idx"].to(DEV).contiguous()
    native.ctrl_fwd(S[:, :Nn], G, idx, pw.ctrl_w, pw.ctrl_off["ew1f"], pw.ctrl_off["nw1f"], pw.ctrl_v, A[:, :N], Sn[:, :Nn],
                    dist, act, pooled=None if pooled is None else pooled[:, :N], argmax=None if am is None else am[:, :N],
                    prec=prec)
    torch.cuda.synchronize()
    return dict(S=S, Sn=Sn, A=A, pooled=pooled, am=am, dist=dist, act=act, G=G, idx=idx)


def _check(case, prec, o, what):
    """Sentinels, the step contract and the planted features of one direct call."""
    _, p = _nets(case["D"], prec)
    B, N, Nn = case["B"], case["N"], case["Nn"]
    # padding records and sentinel rows beyond the agents stay untouched (Sn: obstacle rows too)
    assert bool(torch.isnan(o["S"][:, Nn:]).all()) and torch.equal(o["S"][:, :Nn].cpu(), native.to_records(case["s"])), \
        (what, "input records written")
    for k, keep in (("Sn", o["Sn"][:, N:] == 7.0), ("A", o["A"][:, N:] == 7.0), ("argmax", o["am"][:, N:] == 77),
                    ("pooled", torch.isnan(o["pooled"][:, N:].float()))):
        assert bool(keep.all()), (what, f"{k}: sentinel rows past the agents written", (~keep).any(-1).nonzero()[:6].tolist())
    r = R.step_contract(p, prec, o["S"][:, :Nn], o["G"], o["idx"], o["pooled"][:, :N], o["am"][:, :N], o["A"][:, :N],
                        o["Sn"][:, :N], o["dist"], o["act"], exact_edges=case["planted"], what=what)
    ratio_log(what, r)
    A, am, K = o["A"].cpu(), o["am"].cpu().long(), case["K"]
    il = case["idx"].long()
    for b in range(B):
        assert bool((A[b, int(case["rest"][b])] == 0).all()), (what, "the resting agent's action is not +-0")
        if not case["plants"]:
            continue
        P, Q, T, R1, R2 = (int(case[k][b]) for k in ("P", "Q", "T", "R1", "R2"))
        slot = lambda i, j: int((il[b, i] == j).nonzero()[0, 0])
        row = am[b, P]
        assert not bool((row == slot(P, R2)).any()), (what, "a feature routed to the later duplicate")
        assert not bool((row == slot(P, Q)).any()) and not bool((row == slot(P, T)).any()), (what, "a masked plant's slot")
        assert bool((row == slot(P, R1)).any()), (what, "the in-radius plant wins no feature")
        for i in (Q, T):                                    # isolated: the self row or none
            assert bool(((am[b, i] == slot(i, i)) | (am[b, i] == R.NONE)).all()), what
    return r


# ------------------------------------------------------------------------------- direct calls
@pytest.mark.parametrize("name,prec", DIRECT, ids=[f"{n}-{p}" for n, p in DIRECT])
def test_ctrl_fwd_matches_fp64_oracle_per_row(name, prec):
    case = CC.build(name)
    _check(case, prec, _launch(case, prec), f"{name} {prec}")


APW = [("k12", "32"), ("k12", "8"), ("k12", "4"), ("n300", "32"), ("3d_obs", "32")]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name,apw", APW, ids=[f"{n}-apw{a}" for n, a in APW])
def test_ctrl_fwd_agents_per_wave(name, apw, prec, monkeypatch):
    """K = 12 under 32 / 8 agents per wave (the dense-row edge phase: agents straddle tiles, the
    32-agent groups of k12 straddle the two envs) and 4 (the 2-agent x 16-slot tiles), each against
    the oracle -- not against each other."""
    monkeypatch.setenv("MACBF_CTRL_APW", apw)
    case = CC.build(name)
    _check(case, prec, _launch(case, prec), f"{name} {prec} apw{apw}")


@pytest.mark.parametrize("apw", ["32", "8", ""])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_position_independence(prec, apw, monkeypatch):
    """Rolling the agents of k12 by 5 within each env (idx remapped) puts every agent on another lane,
    tile and dense-row phase and leaves its A / pooled / argmax bits unchanged."""
    if apw:
        monkeypatch.setenv("MACBF_CTRL_APW", apw)
    case = CC.build("k12")
    N = case["N"]
    base, roll = _launch(case, prec), _launch(CC.rolled(case, 5), prec)
    for k in ("A", "pooled", "am"):
        x, y = base[k][:, :N], roll[k][:, :N].roll(-5, 1)
        same = x.view(torch.int32 if k == "A" else (torch.uint8 if k == "am" else torch.int16)) == \
            y.view(torch.int32 if k == "A" else (torch.uint8 if k == "am" else torch.int16))
        assert bool(same.all()), (k, (~same).any(-1).nonzero()[:8].tolist())
    assert not torch.equal(base["am"], roll["am"])


@pytest.mark.parametrize("apw", ["32", ""])
@pytest.mark.parametrize("name", ["k12", "k16"])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_optional_outputs_change_nothing(prec, name, apw, monkeypatch):
    """1-pass builds: pooled = argmax = None (the episode driver's arm) gives A, Sn and the per-env
    sums bit-equal to the call that stores them."""
    if apw:
        monkeypatch.setenv("MACBF_CTRL_APW", apw)
    case = CC.build(name)
    full, bare = _launch(case, prec), _launch(case, prec, outputs=False)
    for k in ("A", "Sn", "dist", "act"):
        assert torch.equal(full[k], bare[k]), k
    assert bool((full["A"][:, :case["N"]] != 7.0).any())


# ------------------------------------------------------------------------------ through the engine
def _trainer(small, **kw):
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.engine.hip_engine import HipEngine
    from macbf_gnn_amd.parallel import DP
    cfg = C.TrainConfig(num_agents=kw.pop("N"), num_envs=kw.pop("B", 2), inner_loops=4, seed=kw.pop("seed", 5), device="hip",
                        early_stop=False, **kw)
    old = HipEngine.small_rollout
    HipEngine.small_rollout = small
    try:
        tr = Trainer(cfg, device=DEV, dp=DP(device=DEV))
    finally:
        HipEngine.small_rollout = old
    assert tr.engine.small_rollout == small
    return tr


ENGINE = [("step-k8", False, dict(N=40, top_k=8)), ("step-k12", False, dict(N=40, top_k=12)),
          ("step-k16", False, dict(N=40, top_k=16)), ("step-k16-bf16", False, dict(N=40, top_k=16, dtype="bf16")),
          ("small-10x5", True, dict(N=10, B=5)), ("small-3d-obs", True, dict(dim=3, num_obstacles=2, N=24))]


@pytest.mark.parametrize("name,small,kw", ENGINE, ids=[e[0] for e in ENGINE])
def test_engine_rollout_steps_match_the_oracle(name, small, kw):
    """engine.rollout, T = 4, no early stop: every stored step's kNN graph equals oracle.knn_idx of the
    stored state (the scan at K = 8 / 16 with N > K) and its (S[t], idx[t]) -> (pooled, argmax, A,
    S[t+1], dist, act) meets the step contract -- each step from the kernel's own inputs."""
    tr = _trainer(small, **dict(kw))
    eng = tr.engine
    s0, g, obs = tr.sample()
    T = eng.rollout(s0, g, obs, early_stop=False)
    torch.cuda.synchronize()
    assert T == 4
    N, K, prec = eng.N, eng.K, eng.prec
    assert K == min(eng.Nn, kw.get("top_k", C.TOP_K))
    p = _kernel_params(tr.fp, prec)
    worst = {}
    for t in range(T):
        st = native.from_records(eng.S[t])
        assert torch.equal(eng.idx[t].long(), O.knn_idx(st[:, :N], K, st)), (name, t, "kNN graph")
        r = R.step_contract(p, prec, eng.S[t], eng.G, eng.idx[t], eng.pooled[t], eng.argmax[t], eng.A[t], eng.S[t + 1][:, :N],
                            eng.dist[t], eng.act[t], what=f"{name} t={t}")
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
        if eng.M:                                           # obstacle nodes: static, never written
            assert torch.equal(eng.S[t + 1][:, N:], eng.S[0][:, N:])
    ratio_log(f"engine {name}", worst)


@pytest.mark.parametrize("lanes", [4, 8])
@pytest.mark.parametrize("K", [8, 16])
def test_scan_at_other_k(K, lanes):
    """native.scan at (B, N) = (2, 40) with K = 8 / 16 (N > K, K != 12): lists, danger bits, counts
    and safety equal the oracle's, as test_gpu_forward._scan_vs_oracle checks them at K = 12."""
    B, N = 2, 40
    s = CC.build("k12")["s"].to(DEV).contiguous()
    idx = torch.empty(B, N, K, dtype=torch.int32, device=DEV)
    dang = torch.empty(B, N, K, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(B, 2, dtype=torch.float32, device=DEV)
    safe = torch.zeros(B, dtype=torch.float32, device=DEV)
    native.scan(s, idx, dang, cnt, safe, K=K, lanes=lanes)
    torch.cuda.synchronize()
    ref = O.knn_idx(s, K)
    assert torch.equal(idx.long(), ref)
    dref = O.ttc_mask_knn(s, ref)
    assert torch.equal(dang.bool(), dref)
    assert torch.equal(cnt[:, 0], dref.sum((1, 2)).float())
    assert torch.equal(cnt[:, 1], (~dref).sum((1, 2)).float())
    assert torch.equal(safe, O.safe_agent_count(s).float())
