"""The persistent one-launch safety filter of small envs (csrc/refine.hip refine_small_kernel,
``safety_filter(impl="persistent")``) against the launch loop (``impl="loop"``, pinned to the CPU
oracle by tests/test_gpu_refine.py): the refined actions bit for bit, ``used`` and the per-iteration
counts as integers, ``viol`` as float64 (the same integer over 2^32 on both paths).

Cases (B envs of N agents, Nn graph nodes, K slots, fp32 and bf16 each, loops 6 / 1 / 0):
  a  2-D  B 3  N 10            Nn 10  K 10  100 edges per env: 3 full tiles and a tail
  b  3-D  B 3  N 12 + 12 obs   Nn 24  K 12  144 edges, obstacle neighbours (clamped a / delta rows)
  c  3-D  B 2  N 52 + 12 obs   Nn 64  K 12  624 edges, a tail tile, the boundary Nn = 64
  d  2-D  B 2  N 64            Nn 64  K 16  1024 edges: the largest env, 32 full tiles
Inputs are built on the host as in tests/test_gpu_refine_mask.py. The seeds give every env edges
with a non-zero hinge gradient at the first iteration; the fp32 CPU model (the loop of
``evaluate.refine_actions`` with the active edges counted per env and iteration) gives
  a  seed 5: 72 / 82 / 69      b  seed 5: 41 / 42 / 32      c  seed 1: 589 / 561      d  seed 1: 524 / 467
which the tests assert (> 0) from the loop path on each env alone.

Per-env stop: the case a shape with env 1's positions scaled by 100, so every pair of it is outside
the radius. The self edges stay inside it (distance 0), and h of a self edge depends on the weights
alone: with the weights of seed 5 it is negative, every self edge violates the condition for ever
(its gradient does not reach the action) and no env ever counts zero. Seed 1 has a non-negative
self-edge h: there the spread-out env counts zero at iteration 0 and the others keep working (CPU
model: 47 / 0 / 44). A scan of seeds 0..299 of the case a shape on the CPU model (loops 6) found
no env that clears strictly between iteration 1 and loops - 1 while another works to the end --
with random-init weights an env's active count hardly moves within 6 steps -- so the scaled-env case
is the only one."""
import copy
import functools

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import env as E
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.models import CBF
from macbf_gnn_amd.ops import graph, native
from macbf_gnn_amd.ops.packing import module_pack
from macbf_gnn_amd.ops.refine import safety_filter

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# name -> (dim, obstacles, B, N, K, seed)
CASES = {"a": (2, 0, 3, 10, 10, 5), "b": (3, 1, 3, 12, 12, 5), "c": (3, 1, 2, 52, 12, 1), "d": (2, 0, 2, 64, 16, 1),
         "a_far": (2, 0, 3, 10, 10, 1),            # the case a shape, env 1 spread out: it stops at iteration 0
         "n65": (3, 1, 1, 53, 12, 1)}              # 65 graph nodes: not eligible
NODES = {"a": 10, "b": 24, "c": 64, "d": 64, "a_far": 10, "n65": 65}
LOOPS = 6
LR = C.REFINE_LEARNING_RATE
PRECS = ("fp32", "bf16")
MASKS = {"101": (1, 0, 1), "010": (0, 1, 0), "000": (0, 0, 0), "111": (1, 1, 1)}


def host_inputs(name):
    """(cbf, s, a, idx, obs) on the host."""
    dim, nobs, B, N, K, seed = CASES[name]
    s, _, obs = E.generate_scenarios(B, N, dim, nobs, seed)
    torch.manual_seed(seed)
    cbf = CBF(2 * dim)
    s = s.clone()
    s[..., dim:] = torch.randn(B, N, dim) * 0.5
    a = torch.randn(B, N, dim) * 2.0
    if name == "a_far":
        s[1, :, :dim] *= 100.0
    idx = O.knn_idx(s, K, O.with_obstacles(s, obs))
    assert idx.shape == (B, N, K) and O.with_obstacles(s, obs).shape[1] == NODES[name]
    return cbf, s, a, idx, obs


@functools.lru_cache(maxsize=None)
def _inputs(name):
    cbf, s, a, idx, obs = host_inputs(name)
    return cbf, s.to(DEV), a.to(DEV), idx.to(DEV), (None if obs is None else obs.to(DEV))


@functools.lru_cache(maxsize=None)
def _module(name, prec):
    cbf = copy.deepcopy(_inputs(name)[0]).to(DEV)
    with torch.no_grad():
        if prec == "bf16":
            cbf.mfma_dtype = torch.bfloat16
            for p in cbf.parameters():
                p.copy_(p.bfloat16().float())
    return cbf


def _run(name, prec, impl, loops=LOOPS, env_active=None, sel=None):
    _, s, a, idx, obs = _inputs(name)
    if sel is not None:
        s, a, idx = s[sel], a[sel], idx[sel]
        obs = None if obs is None else obs[sel]
    return safety_filter(_module(name, prec), s, a, idx, obstacles=obs, loops=loops, lr=LR, return_trace=True,
                         env_active=env_active, impl=impl)


@functools.lru_cache(maxsize=None)
def _loop(name, prec, loops=LOOPS, bits=None):
    """The reference: the launch loop on the batch (optionally masked), computed once."""
    m = None if bits is None else torch.tensor(bits, dtype=torch.bool, device=DEV)
    out = _run(name, prec, "loop", loops, env_active=m)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _loop_alone(name, prec, e):
    """The launch loop on env e alone -> (used, counts)."""
    _, used, _, tr = _run(name, prec, "loop", sel=torch.tensor([e], device=DEV))
    return int(used), tr["counts"].tolist()


def _assert_every_env_works(name, prec):
    for e in range(CASES[name][2]):
        used, counts = _loop_alone(name, prec, e)
        assert counts[0] > 0 and used > 0, (name, prec, e, counts)


def _assert_same(got, want, trace=True):
    ar, used, viol, tr = got
    ar_ref, used_ref, viol_ref, tr_ref = want
    assert torch.equal(ar, ar_ref)
    assert used.dtype == used_ref.dtype and int(used) == int(used_ref), (int(used), int(used_ref))
    assert viol.dtype == torch.float64 and torch.equal(viol, viol_ref), (float(viol), float(viol_ref))
    assert tr["counts"].shape == tr_ref["counts"].shape
    assert torch.equal(tr["counts"], tr_ref["counts"]), (tr["counts"].tolist(), tr_ref["counts"].tolist())
    if trace:
        assert torch.equal(tr["hn"], tr_ref["hn"]) and torch.equal(tr["active"], tr_ref["active"])


@pytest.mark.parametrize("loops", [LOOPS, 1, 0])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_persistent_equals_the_loop_bit_for_bit(name, prec, loops):
    _assert_every_env_works(name, prec)
    want = _loop(name, prec, loops)
    got = _run(name, prec, "persistent", loops)
    _assert_same(got, want, trace=False)
    if loops:
        assert int(want[1]) > 0 and not torch.equal(want[0], _inputs(name)[2])     # the filter did move the actions
    else:
        assert int(got[1]) == 0 and float(got[2]) == 0.0 and torch.equal(got[0], _inputs(name)[2])


@pytest.mark.parametrize("prec", PRECS)
def test_an_env_that_stops_early_leaves_the_others_working(prec):
    name = "a_far"
    useds = [_loop_alone(name, prec, e) for e in range(3)]
    assert useds[1][0] == 0 and useds[1][1][0] == 0, useds             # the spread-out env: nothing to do
    assert useds[0][0] > 0 and useds[2][0] > 0, useds                  # the others work
    assert len({u for u, _ in useds}) > 1
    want = _loop(name, prec)
    _assert_same(_run(name, prec, "persistent"), want)
    a = _inputs(name)[2]
    assert torch.equal(want[0][1], a[1]) and not torch.equal(want[0][0], a[0])


@pytest.mark.parametrize("bits", list(MASKS))
@pytest.mark.parametrize("prec", PRECS)
def test_mask(prec, bits):
    name = "b"
    _assert_every_env_works(name, prec)
    m = MASKS[bits]
    want = _loop(name, prec, LOOPS, m)
    got = _run(name, prec, "persistent", env_active=torch.tensor(m, dtype=torch.bool, device=DEV))
    _assert_same(got, want)
    a = _inputs(name)[2]
    off = torch.tensor([i for i, b in enumerate(m) if not b], dtype=torch.long, device=DEV)
    assert torch.equal(got[0][off], a[off])                            # masked-out envs: the inputs, bit for bit
    assert not bool(got[3]["active"][off].any()) and not bool(got[3]["hn"][off].any())
    if bits == "000":
        assert int(got[1]) == 0 and float(got[2]) == 0.0 and not bool(got[3]["counts"].any())
    else:
        assert int(got[1]) > 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_first_iteration_trace(name, prec):
    want, got = _loop(name, prec), _run(name, prec, "persistent")
    assert torch.equal(got[3]["hn"], want[3]["hn"]) and torch.equal(got[3]["active"], want[3]["active"])
    assert bool(got[3]["active"].any()) and int(got[3]["active"].sum()) == int(want[3]["counts"][0])


@pytest.mark.parametrize("prec", PRECS)
def test_a_scene_of_65_nodes_is_not_eligible(prec):
    name = "n65"
    with pytest.raises(native.NativeError):
        _run(name, prec, "persistent")
    want = _loop(name, prec)
    assert int(want[3]["counts"][0]) > 0
    _assert_same(_run(name, prec, None), want)                         # automatic: the loop path


def test_unknown_impl_and_fp16_raise():
    with pytest.raises(native.NativeError):
        _run("a", "fp32", "fused")
    _, s, a, idx, obs = _inputs("a")
    cbf = copy.deepcopy(_inputs("a")[0]).to(DEV)
    cbf.mfma_dtype = torch.float16
    for impl in (None, "loop", "persistent"):
        with pytest.raises(native.NativeError):
            safety_filter(cbf, s, a, idx, obstacles=obs, loops=2, impl=impl)


def _raw(name, prec, **over):
    """The arguments of native.refine_small, ready to launch."""
    cbf, s, a, idx, obs = _inputs(name)
    cbf = _module(name, prec)
    B, N, D = a.shape
    K = idx.shape[-1]
    mp = module_pack("cbf", cbf, DEV)
    w, v, rm = mp.pack(list(cbf.parameters()))
    S = graph.node_records(s, obs)
    Nn = S.shape[1]
    idx32 = idx.to(torch.int32).contiguous()
    h = torch.empty(1, B, N, K, device=DEV)
    native.cbf_fwd(S.view(1, *S.shape), idx32.view(1, B, N, K), w, mp.off["w1f"], v, two=False, h_out=h, prec=mp.prec)
    rptr = torch.empty(B, Nn + 1, dtype=torch.int32, device=DEV)
    redges = torch.empty(B, N * K, dtype=torch.int32, device=DEV)
    native.rev_csr(idx32, rptr, redges, n_nodes=Nn)
    args = dict(S=S, idx=idx32, a=a.contiguous(), delta=torch.zeros(B, N, D, device=DEV), h=h.view(B, N, K), wpack=w,
                f_bwd=mp.off["w1f"], wrm=rm, wvec=v, rptr=rptr, redges=redges,
                ew=torch.zeros(B, LOOPS, 2, dtype=torch.int64, device=DEV))
    args.update(over)
    return args, dict(loops=LOOPS, lr=LR, prec=mp.prec)


@pytest.mark.parametrize("prec", PRECS)
def test_result_words_of_the_kernel(prec):
    """native.refine_small itself: every word of ew. The spread-out env of a_far has all-zero counts
    and one violation value in every iteration; a working env's counts sum to the loop's."""
    args, kw = _raw("a_far", prec)
    native.refine_small(**args, **kw)
    ew = args["ew"]
    want = _loop("a_far", prec)
    assert torch.equal(ew[:, :, 0].sum(0), want[3]["counts"])
    assert not bool(ew[1, :, 0].any()) and bool((ew[1, :, 1] == ew[1, 0, 1]).all())
    assert not bool(args["delta"][1].any()) and bool(args["delta"][0].any())
    used, viol, counts = native.refine_reduce(ew)
    assert int(used) == int(want[1]) and torch.equal(viol, want[2]) and torch.equal(counts, want[3]["counts"])


@pytest.mark.parametrize("what", ["ew_shape", "ew_dtype", "delta_dtype", "idx_shape", "no_ew"])
def test_refine_small_argument_validation(what):
    B = CASES["a"][2]
    bad = {"ew_shape": dict(ew=torch.zeros(B, LOOPS + 1, 2, dtype=torch.int64, device=DEV)),
           "ew_dtype": dict(ew=torch.zeros(B, LOOPS, 2, dtype=torch.int32, device=DEV)),
           "delta_dtype": dict(delta=torch.zeros(B, 10, 2, dtype=torch.float64, device=DEV)),
           "idx_shape": dict(idx=torch.zeros(B + 1, 10, 10, dtype=torch.int32, device=DEV)),
           "no_ew": dict(ew=None)}[what]
    args, kw = _raw("a", "fp32", **bad)
    with pytest.raises(native.NativeError):
        native.refine_small(**args, **kw)


@pytest.mark.parametrize("prec", PRECS)
def test_two_calls_give_equal_bits(prec):
    x, y = _run("d", prec, "persistent"), _run("d", prec, "persistent")
    _assert_same(x, y)
    assert int(x[1]) > 0


def test_persistent_filter_does_not_synchronise():
    name, prec = "b", "bf16"
    _, s, a, idx, obs = _inputs(name)
    cbf = _module(name, prec)
    m = torch.tensor(MASKS["101"], dtype=torch.bool, device=DEV)
    safety_filter(cbf, s, a, idx, obstacles=obs, loops=2, lr=LR, env_active=m, impl="persistent")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ar, used, viol = safety_filter(cbf, s, a, idx, obstacles=obs, loops=LOOPS, lr=LR, env_active=m,
                                       impl="persistent")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert used.is_cuda and viol.is_cuda and 0 < int(used) <= LOOPS and torch.equal(ar[1], a[1])


def test_the_knob_forces_the_choice(monkeypatch):
    """impl=None: MACBF_REFINE_SMALL = 1 / 0 picks the path -- seen by which native entry is called --
    and an explicit impl wins over the knob."""
    calls = []
    small, loop = native.refine_small, native.refine
    monkeypatch.setattr(native, "refine_small", lambda *a, **k: (calls.append("persistent"), small(*a, **k))[1])
    monkeypatch.setattr(native, "refine", lambda *a, **k: (calls.append("loop"), loop(*a, **k))[1])
    want = _loop("a", "fp32")
    for knob, impl, path in (("1", None, "persistent"), ("0", None, "loop"), ("0", "persistent", "persistent"),
                             ("1", "loop", "loop")):
        monkeypatch.setenv("MACBF_REFINE_SMALL", knob)
        del calls[:]
        _assert_same(_run("a", "fp32", impl), want)
        assert calls == [path], (knob, impl, calls)
    monkeypatch.setenv("MACBF_REFINE_SMALL", "1")                      # forced on, scene not eligible: the loop
    del calls[:]
    _run("n65", "fp32", None)
    assert calls == ["loop"]


def test_validation_is_the_same_on_both_paths(monkeypatch):
    """A Validator at 32 agents x 2 envs in bf16 (random-init networks, weights rounded to bf16),
    val_refine_loops 6 over 8 steps, with the knob forcing each path: equal integer totals, and an
    equal result dict apart from the wall time."""
    from macbf_gnn_amd import validate as V
    from macbf_gnn_amd.models import Controller
    cfg = C.TrainConfig(num_agents=32, num_envs=2, inner_loops=8, seed=3, device="hip", val_every=1, val_envs=2,
                        val_refine_loops=LOOPS, dtype="bf16")
    torch.manual_seed(3)
    ctrl, cbf = Controller(2 * cfg.dim).to(DEV), CBF(2 * cfg.dim).to(DEV)
    with torch.no_grad():
        for p in list(ctrl.parameters()) + list(cbf.parameters()):
            p.copy_(p.bfloat16().float())
    v = V.Validator(cfg, DEV)
    calls = []
    small, loop = native.refine_small, native.refine
    monkeypatch.setattr(native, "refine_small", lambda *a, **k: (calls.append("persistent"), small(*a, **k))[1])
    monkeypatch.setattr(native, "refine", lambda *a, **k: (calls.append("loop"), loop(*a, **k))[1])
    res = {}
    for knob, path in (("0", "loop"), ("1", "persistent")):
        monkeypatch.setenv("MACBF_REFINE_SMALL", knob)
        del calls[:]
        out = v.validate(ctrl, cbf)
        out.pop("val_ms")
        assert calls and set(calls) == {path}
        res[path] = (out, copy.deepcopy(v.last_counts))
    assert res["loop"][1] == res["persistent"][1]
    assert res["loop"][0] == res["persistent"][0]
    assert res["loop"][1]["refined"]["refine_iters"] > 0               # the filter had work
