"""Device-resident closed-loop episodes (macbf_gnn_amd/ops/episode.py, csrc/episode.hip): the native
call gives the integer totals, the final states and the done masks of the unchanged Python episodes
(``Validator.rollout`` with impl="python", ``evaluate.rollout_eval``), for any period of the host's
flag read, repeatably, and validation through it leaves training bit-identical. The three launches
are also checked on their own against torch expressions and hand-written words.

Scenes: env 0's goals sit on its starts (its episode is over after the first step); with three envs,
env 1 starts 0.2 from its goals at speed 0.3 towards them and finishes part-way; the last env runs
the whole horizon. The reference's own per-step values are checked first (``_check_reference``), so
no case passes vacuously: the done steps differ, and every mean goal distance is more than 1e-3 from
DIST_MIN_CHECK -- over ten times the worst fp32 summation error of N <= 96 distances of a few units
(N * 2^-24 * mean, about 5e-5), so the native fixed-point sum and the torch mean decide alike."""
import io
import json

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import validate as V
from macbf_gnn_amd.evaluate import EvalConfig, rollout_eval
from macbf_gnn_amd.models import CBF, Controller
from macbf_gnn_amd.ops import episode, native
from macbf_gnn_amd.ops import refine as refine_ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T = 10
LOOPS = 4
MARGIN = 1e-3

CASES = {
    "a_n32x3_2d_fp32": dict(num_agents=32, val_envs=3, dtype="fp32"),                                    # loop filter
    "b_n20x2_3d_obs_bf16": dict(num_agents=20, val_envs=2, dim=3, num_obstacles=1, dtype="bf16"),     # 32 nodes: persistent
    "c_n96x2_3d_obs_fp32": dict(num_agents=96, val_envs=2, dim=3, num_obstacles=1, dtype="fp32"),     # 108 nodes: per-step scan plan
    "d_n33x3_2d_fp32": dict(num_agents=33, val_envs=3, dtype="fp32"),                                    # waves / tiles straddle envs
}
NODES = {"a_n32x3_2d_fp32": 32, "b_n20x2_3d_obs_bf16": 32, "c_n96x2_3d_obs_fp32": 108, "d_n33x3_2d_fp32": 33}
_SETUPS = {}
_REFS = {}


def _shape_scene(v, all_done=False):
    """The module docstring's scene: env 0 done at once, env 1 of three (every later env with
    ``all_done``) part-way, the last env untouched."""
    D = v.cfg.dim
    B = v.s0.shape[0]
    v.g[0] = v.s0[0, :, :D]
    part = range(1, B) if all_done else range(1, B - 1)
    for b in part:
        e = torch.zeros(D, device=DEV)
        e[b % D] = 1.0
        v.g[b] = v.s0[b, :, :D] + 0.2 * e
        v.s0[b, :, D:] = 0.3 * e


def _setup(case, all_done=False):
    key = (case, all_done)
    if key not in _SETUPS:
        cfg = C.TrainConfig(num_envs=2, inner_loops=T, seed=3, device="hip", val_every=1, val_refine_loops=LOOPS,
                            **CASES[case])
        torch.manual_seed(3)
        ctrl, cbf = Controller(2 * cfg.dim).to(DEV), CBF(2 * cfg.dim).to(DEV)
        for m in (ctrl, cbf):
            m.eval()
            m.mfma_dtype = V.val_dtype(cfg)
        v = V.Validator(cfg, DEV)
        assert v.impl == "python"
        _shape_scene(v, all_done)
        Nn = v.s0.shape[1] + (0 if v.obs is None else v.obs.shape[1])
        assert Nn == NODES[case]
        _SETUPS[key] = (cfg, ctrl, cbf, v)
    return _SETUPS[key]


def _reference(case, refine, all_done=False):
    """``Validator.rollout`` as it is, with the states it hands to the safety count recorded: s_1 ..
    s_T' (the last one is the final state) -> (count vector, final states, final active, per-step
    per-env mean goal distances). Computed once per (case, refine) and never changed."""
    key = (case, refine, all_done)
    if key not in _REFS:
        cfg, ctrl, cbf, v = _setup(case, all_done)
        seen = []
        orig = V._safe_count
        V._safe_count = lambda s, obs=None: (seen.append(s.clone()), orig(s, obs))[1]
        try:
            vec = v.rollout(ctrl, cbf, refine=refine)
        finally:
            V._safe_count = orig
        D = cfg.dim
        dist = torch.stack([torch.linalg.vector_norm(s[..., :D] - v.g, dim=-1).mean(-1) for s in seen])   # (T', B)
        active = (dist >= C.DIST_MIN_CHECK).all(0)
        _REFS[key] = (vec.clone(), seen[-1], active, dist.cpu())
    return _REFS[key]


def _check_reference(case, refine, all_done=False):
    """The preconditions, on the reference's own values."""
    vec, _, active, dist = _reference(case, refine, all_done)
    c = dict(zip(V.COUNTS, vec.tolist()))
    done = [int((dist[:, b] < C.DIST_MIN_CHECK).float().argmax()) + 1 if bool((dist[:, b] < C.DIST_MIN_CHECK).any())
            else T + 1 for b in range(dist.shape[1])]
    gap = float((dist.double() - C.DIST_MIN_CHECK).abs().min())
    print(f"[{case} refine={refine} all_done={all_done}] done steps {done} min |mean dist - thr| {gap:.3e} counts {c}")
    assert len(set(done)) > 1, done                                   # the done steps are not all equal
    assert done[0] == 1
    assert gap > MARGIN, (gap, dist)
    if all_done:
        assert max(done) < T - 1, done                                # steps run after every env finished
    else:
        assert done[-1] == T + 1 and not bool(active[0]) and bool(active[-1])
        if len(done) == 3:
            assert 1 < done[1] <= T, done                             # part-way
    if refine and case[0] in "ac":
        assert c["refine_iters"] > 0, c
    return c


def _native(case, refine, all_done=False, **kw):
    cfg, ctrl, cbf, v = _setup(case, all_done)
    return episode.run_episodes(ctrl, cbf, v.s0, v.g, v.obs, refine=refine, loops=LOOPS, lr=C.REFINE_LEARNING_RATE,
                                max_steps=T, top_k=cfg.top_k, **kw)


def _assert_counts(got, want):
    g, w = dict(zip(V.COUNTS, got.tolist())), dict(zip(V.COUNTS, want.tolist()))
    print("native", g, "reference", w)
    for k in V.COUNTS:
        if k == "goal_dist_fx":
            # per-agent rounding at 2^-32 over <= 192 agents is under 2^-25, plus the final rounding
            assert abs(g[k] - w[k]) <= 1, (k, g[k], w[k])
        else:
            assert g[k] == w[k], (k, g, w)


@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_counts_and_states_equal_the_python_rollout(case, refine):
    _check_reference(case, refine)
    want, s_ref, act_ref, _ = _reference(case, refine)
    s0 = _setup(case)[3].s0.clone()
    got, s_fin, active = _native(case, refine, return_state=True)
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == (len(V.COUNTS),)
    _assert_counts(got, want)
    assert torch.equal(_setup(case)[3].s0, s0)                         # the caller's scenes are not written
    assert s_fin.shape == s_ref.shape and active.dtype == torch.bool
    assert torch.equal(active, act_ref), (active, act_ref)
    assert torch.equal(s_fin, s_ref), float((s_fin - s_ref).abs().max())


def test_the_filter_path_is_the_one_the_case_is_for(monkeypatch):
    monkeypatch.delenv("MACBF_REFINE_SMALL", raising=False)
    K = {c: min(C.TOP_K, CASES[c]["num_agents"]) for c in CASES}
    want = {"a_n32x3_2d_fp32": "loop", "b_n20x2_3d_obs_bf16": "persistent", "c_n96x2_3d_obs_fp32": "loop",
            "d_n33x3_2d_fp32": "loop"}
    for c in CASES:
        assert refine_ops.choose_impl(None, CASES[c]["dtype"], NODES[c], K[c]) == want[c]
    assert (33 * 3) % 64 and 33 % 64 and (33 * K["d_n33x3_2d_fp32"]) % 32    # (d): waves and 32-edge tiles straddle envs
    # (c) runs the scan's per-step plan with both outputs from one launch
    plan = native.scan_plan(2, 96, K["c_n96x2_3d_obs_fp32"], Nn=108, dim=3, prev=False, do_knn=True, do_safety=True)
    assert plan["blocks"] >= 1 and plan["glb"] == 0


@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_evaluation_rule_matches_rollout_eval(case, refine):
    """mask_done=False through ``rollout_eval(rollout_impl="native")`` against the Python loop with
    the device-resident filter: a finished env is still refined until the batch stops."""
    cfg, ctrl, cbf, v = _setup(case)
    _check_reference(case, refine)
    ec = dict(num_agents=cfg.num_agents, num_envs=v.s0.shape[0], max_steps=T, refine=refine, refine_loops=LOOPS,
              top_k=cfg.top_k, dim=cfg.dim, refine_impl="native")
    want = rollout_eval(ctrl, cbf, v.s0, v.g, EvalConfig(**ec), obstacles=v.obs)
    got = rollout_eval(ctrl, cbf, v.s0, v.g, EvalConfig(rollout_impl="native", **ec), obstacles=v.obs)
    print("native", got, "reference", want)
    assert set(got) == set(want)
    for k in ("agent_steps", "steps", "refine_iters"):
        assert isinstance(got[k], int) and got[k] == int(want[k]), (k, got[k], want[k])
    assert got["safety_rate"] == want["safety_rate"] and got["reaching_rate"] == want["reaching_rate"]
    assert abs(got["mean_goal_dist"] - want["mean_goal_dist"]) <= 1e-6 * abs(want["mean_goal_dist"])
    if refine and case[0] in "ac":
        assert want["refine_iters"] > 0


@pytest.mark.parametrize("case,all_done", [("a_n32x3_2d_fp32", False), ("a_n32x3_2d_fp32", True),
                                           ("b_n20x2_3d_obs_bf16", False), ("d_n33x3_2d_fp32", True)])
def test_result_does_not_depend_on_the_check_period(case, all_done):
    """check_every 1, 3 and 10: with 10 the driver never looks and runs every step; with ``all_done``
    every env finishes before the horizon, so the later steps run on a finished batch."""
    want_c = _check_reference(case, True, all_done)
    outs = [_native(case, True, all_done, check_every=p, return_state=True) for p in (1, 3, 10)]
    _assert_counts(outs[0][0], _reference(case, True, all_done)[0])
    if all_done:
        assert want_c["steps"] < T - 1 and not bool(outs[0][2].any())
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]), (o[0], outs[0][0])
        assert torch.equal(o[1], outs[0][1]) and torch.equal(o[2], outs[0][2])
    for mask_done in (True, False):
        a = _native(case, True, all_done, check_every=1, mask_done=mask_done)
        b = _native(case, True, all_done, check_every=10, mask_done=mask_done)
        assert torch.equal(a, b), (mask_done, a, b)


@pytest.mark.parametrize("case", list(CASES))
def test_two_calls_give_identical_outputs(case):
    for refine in (False, True):
        a = _native(case, refine, return_state=True)
        b = _native(case, refine, return_state=True)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_refusals_on_the_device():
    cfg, ctrl, cbf, v = _setup("a_n32x3_2d_fp32")
    with pytest.raises(native.NativeError, match="HIP device"):
        episode.run_episodes(ctrl, cbf, v.s0.cpu(), v.g.cpu(), None, refine=False)
    with pytest.raises(native.NativeError, match="MAX_TOP_K"):
        episode.run_episodes(ctrl, cbf, v.s0, v.g, None, refine=False, top_k=17)
    half = CBF(4).to(DEV)
    half.mfma_dtype = torch.float16
    with pytest.raises(native.NativeError, match="fp16 is not supported"):
        episode.run_episodes(ctrl, half, v.s0, v.g, None, refine=True)


# ----------------------------------------------------------------------------- the three launches alone
FX = 2 ** 32


def _norm(x):
    """|x| over the last axis in fp32, squares added in coordinate order (the kernels' order)."""
    sq = x * x
    s = sq[..., 0]
    for q in range(1, x.shape[-1]):
        s = s + sq[..., q]
    return s.sqrt()


def _launch_state(D, B=3, N=33, M=7, alive=1):
    g = torch.Generator(device="cpu").manual_seed(11 + D)
    r = lambda *s: (torch.rand(*s, generator=g) - 0.5).to(DEV)
    s = r(B, N + M, 2 * D)
    i64 = dict(dtype=torch.int64, device=DEV)
    return dict(S_cur=native.to_records(s), G=r(B, N, D).contiguous(), st=torch.tensor([alive, 0, 0, 0, 0], **i64),
                dist_fx=torch.zeros(B, **i64), safe=torch.zeros(B, device=DEV),
                active=torch.ones(B, dtype=torch.uint8, device=DEV),
                prev_active=torch.zeros(B, dtype=torch.uint8, device=DEV)), s, r


@pytest.mark.parametrize("alive", [1, 0])
@pytest.mark.parametrize("with_delta", [True, False])
@pytest.mark.parametrize("D", [2, 3])
def test_advance_is_the_python_euler_step(D, with_delta, alive):
    """33 agents x 3 envs + 7 obstacle rows: two of the advance kernel's waves straddle envs."""
    st, s, r = _launch_state(D, alive=alive)
    B, N = st["G"].shape[:2]
    A = r(B, N, D).contiguous()
    delta = r(B, N, D).contiguous() if with_delta else None
    d0 = None if delta is None else delta.clone()
    S_next = torch.full_like(st["S_cur"], 7.0)
    native.episode_advance(S_next=S_next, A=A, delta=delta, **st)
    u = A if delta is None else A + d0
    sa = s[:, :N]
    want = sa + torch.cat([sa[..., D:], u], -1) * C.TIME_STEP if alive else sa
    assert torch.equal(native.from_records(S_next[:, :N]), want)
    assert bool((S_next[:, N:] == 7.0).all())                         # obstacle rows are not touched
    if delta is not None:
        assert not bool(delta.any())                                  # zeroed for the next step
    d = _norm(want[..., :D] - st["G"])
    assert st["dist_fx"].tolist() == (d.double() * FX).round().long().sum(-1).tolist()
    assert st["st"].tolist() == [alive, 0, 0, 0, 0] and torch.equal(native.to_records(s), st["S_cur"])


@pytest.mark.parametrize("mode", ["none", "loop", "persistent"])
def test_tally_of_hand_written_words(mode):
    st, _, _ = _launch_state(2)
    N = st["G"].shape[1]
    thr = int(round(float(torch.tensor(C.DIST_MIN_CHECK, dtype=torch.float32).double()) * N * FX))
    st["st"].copy_(torch.tensor([1, 100, 200, 300, 400]))
    st["safe"].copy_(torch.tensor([5.0, 6.0, 7.0]))
    st["prev_active"].copy_(torch.tensor([1, 0, 1], dtype=torch.uint8))
    st["active"].copy_(torch.tensor([1, 1, 0], dtype=torch.uint8))
    st["dist_fx"].copy_(torch.tensor([thr - 1, thr, 1 << 40]))
    kw, used = {}, 0
    if mode == "loop":          # iterations 0 and 2 had an active edge
        kw, used = dict(ctl=torch.tensor([3, 9, 0, 9, 2, 9, 0, 9], dtype=torch.int64, device=DEV), loops=4), 2
    elif mode == "persistent":  # env 0 worked in 1 iteration, env 1 in 3, env 2 in none: the slowest env counts
        ew = torch.tensor([[[4, 9], [0, 9], [0, 9], [0, 9]], [[4, 9], [2, 9], [1, 9], [0, 9]],
                           [[0, 0], [0, 0], [0, 0], [0, 0]]], dtype=torch.int64, device=DEV)
        kw, used = dict(ew=ew, loops=4), 3
    native.episode_tally(**st, **kw)
    assert st["st"].tolist() == [1, 100 + 5 + 7, 200 + 2, 300 + 1, 400 + used]
    assert st["active"].tolist() == [0, 1, 0] and st["prev_active"].tolist() == [1, 1, 0]
    assert not bool(st["dist_fx"].any()) and not bool(st["safe"].any())
    if mode == "persistent":
        assert not bool(kw["ew"].any())                               # zero again for the next launch
    # a step after the last env finished: nothing counts, and alive stays 0
    st["st"][0] = 0
    st["active"].zero_()
    st["prev_active"].zero_()
    st["safe"].fill_(9.0)
    if mode == "persistent":
        kw["ew"][:, 0, 0] = 5
    before = st["st"].tolist()
    native.episode_tally(**st, **kw)
    assert st["st"].tolist() == before


@pytest.mark.parametrize("D", [2, 3])
def test_final_vector(D):
    st, s, _ = _launch_state(D)
    B, N = st["G"].shape[:2]
    st["G"][0] = s[0, :N, :D]                                         # env 0 sits on its goals
    st["G"][1, :5] = s[1, :5, :D] + 0.01
    st["st"].copy_(torch.tensor([0, 1000, 17, 9, 36]))
    st["safe"].copy_(torch.tensor([30.0, 31.0, 32.0]))
    st["prev_active"].copy_(torch.tensor([0, 1, 1], dtype=torch.uint8))
    out = torch.zeros(native.EP_OUT, dtype=torch.int64, device=DEV)
    native.episode_final(out=out, **st)
    d = _norm(s[:, :N, :D] - st["G"])
    fx32 = int((d.double() * FX).round().long().sum())
    want = [1000 + 31 + 32, 17 * N, int((d < C.DIST_MIN_CHECK).sum()), B * N, 17, 36, 9, (fx32 + (1 << 11)) >> 12]
    assert out.tolist() == want
    assert want[2] >= N + 5


# ----------------------------------------------------------------------------- Validator integration
TRAIN_CASES = {
    "n32_bf16": dict(num_agents=32, dtype="bf16"),
    "n96_3d_obs": dict(num_agents=96, dim=3, num_obstacles=1),
}


def _trainer(case, **kw):
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    cfg = C.TrainConfig(num_envs=2, inner_loops=T, seed=3, device="hip", display_steps=1, val_envs=2,
                        val_refine_loops=LOOPS, **TRAIN_CASES[case], **kw)
    tr = Trainer(cfg, device=DEV, dp=DP(device=DEV))
    tr.logger.stream = io.StringIO()
    return tr


def _records(tr):
    return [json.loads(l) for l in tr.logger.stream.getvalue().splitlines()]


@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_validate_native_returns_the_python_dict(case):
    tr = _trainer(case, val_every=2, val_impl="native")
    tr.fit(1)                                       # one real update: not the initial weights
    nat = tr.validate()
    v = tr.validator
    assert v.impl == "native"
    nat_counts = dict(v.last_counts)
    v.impl = "python"
    py = tr.validate()
    print("native", nat, nat_counts, "python", py, v.last_counts)
    nat.pop("val_ms"), py.pop("val_ms")
    assert nat == py
    assert nat_counts == v.last_counts
    assert nat_counts["refined"]["steps"] > 0 and nat_counts["nominal"]["agent_steps"] > 0
    for m in (tr.controller, tr.cbf):
        assert "mfma_dtype" not in m.__dict__ and m.training


@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_training_is_bit_identical_with_native_validation(case):
    ref, tr = _trainer(case), _trainer(case, val_every=2, val_impl="native")
    ref.fit(4)
    tr.fit(4)
    torch.cuda.synchronize()
    assert ref.validator is None and tr.validator is not None and tr.validator.impl == "native"
    assert torch.equal(tr.fp.flat, ref.fp.flat)
    assert torch.equal(tr.opt.exp_avg, ref.opt.exp_avg) and torch.equal(tr.opt.exp_avg_sq, ref.opt.exp_avg_sq)
    assert tr.opt.steps == ref.opt.steps and tr.skipped_steps == ref.skipped_steps
    recs, ref_recs = _records(tr), _records(ref)
    vals = [r for r in recs if "val_safety_rate" in r]
    train = [r for r in recs if "loss_total" in r]
    assert [x["step"] for x in vals] == [2, 4] and len(train) == len(ref_recs) == 4
    for r, q in zip(train, ref_recs):
        r.pop("agent_steps_per_s"), q.pop("agent_steps_per_s")
        assert r == q
    for x in vals:
        assert 0.0 <= x["val_safety_rate"] <= 1.0 and 0.0 <= x["val_refined_safety_rate"] <= 1.0
        assert 0.0 < x["val_mean_T"] <= T and 0.0 < x["val_refined_mean_T"] <= T and x["val_ms"] > 0.0
    for m in (tr.controller, tr.cbf):
        assert "mfma_dtype" not in m.__dict__ and m.training
