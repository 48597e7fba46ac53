"""CPU: the controller's residual head (macbf_gnn_amd/oracle.py, "Residual head") through the Python
layers -- the model's shapes and initialisation, oracle.controller_forward, ops.selfcheck.node_oracle,
the packing tables (fragments, row-major images, side vector, gradient maps) with the lane-level
emulator of ops/layout.py, checkpoints, the evaluation's refusals, one oracle-engine training step and a
world-2 gloo step. The device tests are tests/test_gpu_ctrl_residual_{fwd,bwd,step}.py.

Reference op: controller.py:47-61 of the reference (the gain law the residual adds to)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from macbf_gnn_amd import config as C
from macbf_gnn_amd import env as E
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.models import CBF, Controller
from macbf_gnn_amd.ops import layout as L
from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.selfcheck import node_oracle
from macbf_gnn_amd.utils import ckpt
from macbf_gnn_amd.utils.params import FlatParams

import ctrl_residual_cases as RC
import node_cases as NC
from test_layout import acc_to_mat

CPU = torch.device("cpu")
W4, B4 = "controller_dec_net.6.weight", "controller_dec_net.6.bias"


# ----------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("D", [2, 3])
def test_state_dict_shapes_and_zero_rows(D):
    plain, res = Controller(2 * D), Controller(2 * D, residual=True)
    sp, sr = plain.state_dict(), res.state_dict()
    assert list(sp) == list(sr)                                     # the same parameter names
    assert tuple(sp[W4].shape) == (2 * D, 64) and tuple(sp[B4].shape) == (2 * D,)
    assert tuple(sr[W4].shape) == (3 * D, 64) and tuple(sr[B4].shape) == (3 * D,)
    for k in sp:
        if k not in (W4, B4):
            assert sp[k].shape == sr[k].shape, k
    assert bool((sr[W4][2 * D:] == 0).all()) and bool((sr[B4][2 * D:] == 0).all())
    assert bool((sr[W4][:2 * D] != 0).any()) and bool((sr[B4][:2 * D] != 0).any())
    assert plain.residual is False and res.residual is True


def _scene(D, B=2, N=9, K=5, seed=0):
    gen = torch.Generator().manual_seed(seed)
    s = torch.cat([torch.rand(B, N, D, generator=gen) * 2.0, (torch.rand(B, N, D, generator=gen) - 0.5)], -1)
    g = s[..., :D] + (torch.rand(B, N, D, generator=gen) - 0.5)
    return s, g, O.knn_idx(s, K)


@pytest.mark.parametrize("D", [2, 3])
def test_oracle_forward_zero_rows_equal_plain_and_random_rows_add_y(D):
    s, g, idx = _scene(D)
    res = RC.controller(D, randomise=False)
    plain = RC.plain_twin(res)
    a_res = O.controller_forward(res.params_dict(), s, g, idx)
    a_plain = O.controller_forward(plain.params_dict(), s, g, idx)
    assert torch.equal(a_res, a_plain)
    # random residual rows: plain + y[..., 2D:], y recomputed here in float64
    res = RC.controller(D)
    p64 = {k: v.detach().double() for k, v in res.params_dict().items()}
    pp64 = {k: v.detach().double() for k, v in RC.plain_twin(res).params_dict().items()}
    s64, g64 = s.double(), g.double()
    a = O.controller_forward(p64, s64, g64, idx)
    a_pl, aux = O.controller_forward(pp64, s64, g64, idx, return_aux=True)
    z = torch.cat([aux["pooled"], s64[..., :D] - g64, s64[..., D:]], -1)
    for li in (0, 2, 4):
        z = torch.relu(z @ p64[f"controller_dec_net.{li}.weight"].t() + p64[f"controller_dec_net.{li}.bias"])
    y_res = z @ p64[W4][2 * D:].t() + p64[B4][2 * D:]
    assert float(y_res.abs().max()) > 1e-3
    assert float((a - (a_pl + y_res)).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------ the node oracle
@pytest.mark.parametrize("name", RC.NODE_ALL)
def test_node_oracle_matches_controller_autograd(name):
    """As tests/test_node_oracle_ref.py for the plain law (its graph, its tolerance): idx = self, the
    pooled values a leaf, A = a."""
    case = RC.node_case(name)
    B, N, D = case["B"], case["N"], case["D"]
    p64 = {k: v.detach().double() for k, v in RC.controller(D).params_dict().items()}
    assert p64[W4].shape[0] == 3 * D
    p = {k: v.clone().requires_grad_(True) for k, v in p64.items()}
    s = case["s"][:, :N].double().requires_grad_(True)
    g = case["G"].double()
    pool = case["pv"].double().requires_grad_(True)
    idx = torch.arange(N).view(1, N, 1).expand(B, N, 1)
    a = O.controller_forward(p, s, g, idx, pool_values=pool)
    A = a.detach()
    m = torch.ones_like(A) if not case["a_max"] else ((A >= -case["a_max"]) & (A <= case["a_max"])).double()
    vb = torch.ones(B, dtype=torch.float64) if case["valid"] is None else case["valid"].double()
    gnv = case["Gn"].double()[..., D:]
    loss = (C.TIME_STEP * gnv * m * a).sum() + (case["c"] * vb.view(B, 1) * O.action_loss_terms(s, g, a)).sum()
    names = [k for k in p if k.startswith("controller_dec_net")]
    ref = torch.autograd.grad(loss, [pool, s] + [p[k] for k in names])
    dP, ego, dw, tie, scales, psc, esc = node_oracle(p64, case["pv"], None, native.to_records(case["s"]), case["G"], A,
                                                      native.to_records(case["Gn"]), case["valid"], case["c"],
                                                      case["a_max"])
    n = B * N

    def close(got, want, what):
        bound = 1e-6 * float(want.abs().max())
        assert float((got - want).abs().max()) <= bound, (what, float((got - want).abs().max()), bound)

    close(dP, ref[0].reshape(n, 128), "dP")
    close(ego, ref[1].reshape(n, 2 * D), "ego")
    for k, r in zip(names, ref[2:]):
        close(dw[k], r, k)
        assert scales[k].shape == r.shape and bool((scales[k] + 1e-300 >= r.abs()).all()), k
    assert float(dw[W4][2 * D:].abs().max()) > 0 and float(dw[B4][2 * D:].abs().max()) > 0


@pytest.mark.parametrize("name", RC.NODE_ALL)
def test_node_case_conditions(name):
    """What the device test takes for granted (tests/test_node_oracle_ref.py's conditions): few tie rows,
    an unambiguous action-loss sign, raw actions clear of the limit with both sides populated."""
    from test_node_oracle_ref import LIMIT_MARGIN, SIGN_MARGIN, TIE_CAP
    case = RC.node_case(name)
    D = case["D"]
    hi, lo = NC.split_pooled(case["pv"], torch.bfloat16, True)
    p64 = {k: v.detach().double() for k, v in RC.controller(D).params_dict().items()}
    tie = node_oracle(p64, *NC.oracle_inputs(case, hi, lo))[3]
    assert float(tie.double().mean()) <= TIE_CAP, (name, int(tie.sum()), tie.numel())
    s, A = case["s"][:, :case["N"]].double(), case["A"].double()
    ar = O.action_ref(s, case["G"].double())
    a2, r2 = (A * A).sum(-1), (ar * ar).sum(-1)
    assert float(((a2 - r2).abs() / (a2 + r2)).min()) >= SIGN_MARGIN
    if case["a_max"]:
        assert float((A.abs() - case["a_max"]).abs().min()) >= LIMIT_MARGIN
        assert 0.1 <= float((A.abs() > case["a_max"]).double().mean()) <= 0.9


# ------------------------------------------------------------------------------------- packing
def _setup(D, residual):
    res = RC.controller(D)
    ctrl = res if residual else RC.plain_twin(res)
    fp = FlatParams({"controller": ctrl, "cbf": CBF(2 * D)})
    offs = {pn: o for (m, pn, shape, o, n) in fp.specs}
    src = np.concatenate([fp.flat.numpy().astype(np.float64), [0.0, 1.0]])
    return ctrl, fp, offs, src


def _owner(fp):
    """flat index -> (parameter name, row-major index inside it); the two constants -> themselves."""
    own = {}
    for m, pn, shape, o, n in fp.specs:
        for i in range(n):
            own[o + i] = (pn, i)
    own[fp.numel], own[fp.numel + 1] = "ZERO", "ONE"
    return own


def _tables(fp, offs, D, n4):
    r = lambda a: L.resolve(np.asarray(a), fp.numel)
    return {"frags": r(L.ctrl_packer(offs, D, n4).index()), "vec": r(L.ctrl_vec_index(offs, D, n4)[0]),
            "rm": r(L.ctrl_node_rm(offs, D, n4).index()), "rm16": r(L.node_rm16(offs, D, n4).index())}


@pytest.mark.parametrize("D", [2, 3])
def test_grad_maps_cover_every_last_layer_element_once(D):
    ctrl, fp, offs, _ = _setup(D, True)
    mp_ = __import__("macbf_gnn_amd.ops.packing", fromlist=["ModulePack"]).ModulePack("ctrl", ctrl, CPU)
    moffs = {n: o for n, _, o, _ in mp_.shapes}
    maps = {"node": (L.ctrl_node_grad_map(offs, D, 3 * D), offs, native.CTRL_NODE_PARTIAL),
            "node16": (L.ctrl_node16_grad_map(offs, D, 3 * D), offs, native.CTRL_NODE_PARTIAL),
            "module": (tuple(x.numpy() for x in mp_.maps["node"]), moffs, native.CTRL_NODE_PARTIAL)}
    for name, ((sm, dm), of, width) in maps.items():
        assert len(set(sm.tolist())) == len(sm) and sm.min() >= 0 and sm.max() < width, name
        for pn, n in ((W4, 3 * D * 64), (B4, 3 * D)):
            hits = np.bincount(dm[(dm >= of[pn]) & (dm < of[pn] + n)] - of[pn], minlength=n)
            assert (hits == 1).all(), (name, pn, np.nonzero(hits != 1)[0][:8].tolist())
    # the plain maps: what they were (the default n4 is the plain 2D; no residual-row destination)
    _, fpp, offp, _ = _setup(D, False)
    for fn in (L.ctrl_node_grad_map, L.ctrl_node16_grad_map):
        a, b = fn(offp, D), fn(offp, D, 2 * D)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        sr, dr = fn(offs, D, 3 * D)
        own_p, own_r = _owner(fpp), _owner(fp)
        plain_pairs = {(int(s_), own_p[int(d_)]) for s_, d_ in zip(*a)}
        res_pairs = {(int(s_), own_r[int(d_)]) for s_, d_ in zip(sr, dr)}
        assert plain_pairs <= res_pairs
        extra = res_pairs - plain_pairs
        assert len(extra) == D * 64 + D
        assert all((pn == W4 and i >= 2 * D * 64) or (pn == B4 and i >= 2 * D) for _, (pn, i) in extra)
    with pytest.raises(ValueError, match="residual"):
        L.ctrl_node_grad_map(offs, D, 2 * D + 1)


@pytest.mark.parametrize("D", [2, 3])
def test_plain_tables_unchanged_and_residual_tables_add_only_residual_rows(D):
    """Every packed position holds the same parameter element as in the tables built at residual=False;
    the positions that are zero there and not here hold residual rows, each residual element somewhere."""
    _, fpp, offp, _ = _setup(D, False)
    _, fpr, offr, _ = _setup(D, True)
    plain, plain_dflt, res = _tables(fpp, offp, D, 2 * D), _tables(fpp, offp, D, None), _tables(fpr, offr, D, 3 * D)
    own_p, own_r = _owner(fpp), _owner(fpr)
    for k in plain:
        assert np.array_equal(plain[k], plain_dflt[k]), k
        assert plain[k].shape == res[k].shape, k                    # no slab, fragment count or image size changes
        a = [own_p[int(i)] for i in plain[k]]
        b = [own_r[int(i)] for i in res[k]]
        new = set()
        for x, y in zip(a, b):
            if x != y:
                assert x == "ZERO" and y[0] in (W4, B4), (k, x, y)
                assert y[1] >= (2 * D * 64 if y[0] == W4 else 2 * D), (k, y)
                new.add(y)
        want = {(B4, 2 * D + q) for q in range(D)} if k == "vec" else {(W4, i) for i in range(2 * D * 64, 3 * D * 64)}
        assert new == want, (k, len(new))


@pytest.mark.parametrize("D", [2, 3])
def test_packed_images_hold_the_residual_rows_where_the_fragments_read_them(D):
    ctrl, fp, offs, src = _setup(D, True)
    n4 = 3 * D
    Wm = ctrl.controller_dec_net[6].weight.detach().numpy().astype(np.float64)      # (3D, 64)
    bm = ctrl.controller_dec_net[6].bias.detach().numpy().astype(np.float64)
    assert np.abs(Wm[2 * D:]).min() > 0
    rng = np.random.default_rng(5)
    Y3 = [rng.normal(size=(64, 16)) for _ in range(2)]                              # accumulator tiles (64 x 32 agents)
    Y3m = np.concatenate([acc_to_mat(y) for y in Y3], 0)
    d4 = np.zeros((64, 16))
    d4m = np.zeros((32, 32))
    d4m[:n4] = rng.normal(size=(n4, 32))
    for l in range(64):
        for reg in range(16):
            d4[l, reg] = d4m[L.acc_row(reg, l >> 5), l & 31]
    pk = L.ctrl_packer(offs, D, n4)
    vals = src[L.resolve(pk.index(), fp.numel)]
    fo = pk.offsets()
    # forward fragments nw4: y4 = W4 Y3 (rows past 3D zero)
    c = np.zeros((64, 16))
    for kk in range(4):
        c = L.emu_mfma(L.emu_frag(vals, fo["nw4"] + kk), L.emu_acc_frag(Y3[kk >> 1], kk & 1), c)
    y4 = acc_to_mat(c)
    np.testing.assert_allclose(y4[:n4], Wm @ Y3m, rtol=1e-12, atol=1e-12)
    assert not y4[n4:].any()
    # row 8 (D = 3) is register 4 of the h == 0 lane, rows 4..7 registers 0..3 of the h == 1 lane
    assert L.acc_row(4, 0) == 8 and [L.acc_row(q, 1) for q in range(4)] == [4, 5, 6, 7]
    # transposed fragments nw4t: dY3 = W4^T d4
    for mt in range(2):
        c = np.zeros((64, 16))
        for kk in range(2):
            c = L.emu_mfma(L.emu_frag(vals, fo["nw4t"] + mt * 2 + kk), L.emu_acc_frag(d4, kk), c)
        np.testing.assert_allclose(acc_to_mat(c), (Wm.T @ d4m[:n4])[32 * mt:32 * mt + 32], rtol=1e-12, atol=1e-12)
    # the row-major image of the 32x32x16 backward bodies: W fragments (wrm_acc) and W^T (wrmT_acc)
    rm = L.ctrl_node_rm(offs, D, n4)
    img = src[L.resolve(rm.index(), fp.numel)][rm.offsets()["w4"]:].reshape(32, L.NODE_STRIDES["w4"])
    c = np.zeros((64, 16))
    for kk in range(4):
        c = L.emu_mfma(L.emu_wrm_acc(img, 0, kk), L.emu_acc_frag(Y3[kk >> 1], kk & 1), c)
    np.testing.assert_allclose(acc_to_mat(c)[:n4], Wm @ Y3m, rtol=1e-12, atol=1e-12)
    for mt in range(2):
        c = np.zeros((64, 16))
        for kk in range(2):
            c = L.emu_mfma(L.emu_wrmT_acc(img, 32 * mt, kk), L.emu_acc_frag(d4, kk), c)
        np.testing.assert_allclose(acc_to_mat(c), (Wm.T @ d4m[:n4])[32 * mt:32 * mt + 32], rtol=1e-12, atol=1e-12)
    # the 16x16x32 body's image: 16 rows, columns permuted by perm32_logical, rows past 3D zero
    rm16 = L.node_rm16(offs, D, n4)
    img16 = src[L.resolve(rm16.index(), fp.numel)][rm16.offsets()["w4"]:].reshape(16, L.NODE16_STRIDES["w4"])
    for r in range(16):
        for c_ in range(64):
            assert img16[r, c_] == (Wm[r, L.perm32_logical(c_)] if r < n4 else 0.0), (r, c_)
    # side vector: nb4 holds all 3D biases, zero up to its 32 slots
    vec, voff = L.ctrl_vec_index(offs, D, n4)
    v = src[L.resolve(vec, fp.numel)]
    assert np.array_equal(v[voff["nb4"]:voff["nb4"] + n4], bm) and not v[voff["nb4"] + n4:voff["nb4"] + 32].any()


def test_packed_weights_and_module_pack_read_the_shape():
    from macbf_gnn_amd.ops.packing import module_pack
    from macbf_gnn_amd.ops.weights import PackedWeights
    for D in (2, 3):
        for residual in (False, True):
            ctrl, fp, _, _ = _setup(D, residual)
            pw = PackedWeights(fp, D, torch.float32)
            assert pw.residual is residual and pw.n4 == (3 if residual else 2) * D
            assert module_pack("ctrl", ctrl, CPU).residual is residual
    assert module_pack("cbf", CBF(4), CPU).residual is False


# --------------------------------------------------------------------------------- checkpoints
def _tr(**kw):
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    cfg = C.TrainConfig(num_agents=kw.pop("N", 8), num_envs=kw.pop("B", 2), inner_loops=kw.pop("T", 4), device="cpu",
                        seed=kw.pop("seed", 0), **kw)
    return Trainer(cfg, device=CPU, dp=DP(device=CPU))


def test_checkpoint_round_trip_and_model_residual(tmp_path):
    assert C.TrainConfig().ctrl_residual is False and "ctrl_residual" in ckpt.ARCH_KEYS
    tr = _tr(ctrl_residual=True)
    assert tr.controller.residual and tuple(tr.controller.state_dict()[W4].shape) == (6, 64)
    with torch.no_grad():
        tr.controller.controller_dec_net[6].weight[4:].normal_()      # (the modules' parameters are views of fp.flat)
    pr, pp = str(tmp_path / "res.pt"), str(tmp_path / "plain.pt")
    tr.save(pr)
    _tr().save(pp)
    assert ckpt.model_residual(pr) is True and ckpt.model_residual(pp) is False
    torch.save({"cbf": CBF(4).state_dict()}, tmp_path / "cbf.pt")
    assert ckpt.model_residual(str(tmp_path / "cbf.pt")) is None
    back = _tr(ctrl_residual=True, seed=5)
    ckpt.load(back, pr)
    for k, v in tr.controller.state_dict().items():
        assert torch.equal(v, back.controller.state_dict()[k]), k
    with pytest.raises(ValueError, match="ctrl_residual=True.*ctrl_residual=False"):
        ckpt.load(_tr(), pr)
    with pytest.raises(ValueError, match="ctrl_residual=False.*ctrl_residual=True"):
        ckpt.load(_tr(ctrl_residual=True), pp)
    # a checkpoint from before the option existed holds a plain controller
    ck = torch.load(pp, weights_only=True)
    ck["config"].pop("ctrl_residual")
    torch.save(ck, pp)
    ckpt.load(_tr(), pp)
    with pytest.raises(ValueError, match="ctrl_residual"):
        ckpt.load(_tr(ctrl_residual=True), pp)


def test_train_cli_flag():
    import train
    assert train.build_config(train.parse_args(["--num_agents", "4"])).ctrl_residual is False
    cfg = train.build_config(train.parse_args(["--num_agents", "4", "--ctrl_residual", "--a_max", "0.5"]))
    assert cfg.ctrl_residual is True and cfg.a_max == 0.5


def test_graph_mode_is_refused_by_name():
    import train
    with pytest.raises(ValueError) as e:
        _tr(ctrl_residual=True, graph=True)
    assert "ctrl_residual" in str(e.value) and "graph" in str(e.value)
    with pytest.raises(SystemExit) as e:
        train.build_config(train.parse_args(["--num_agents", "4", "--ctrl_residual", "--graph"]))
    assert "--ctrl_residual" in str(e.value) and "--graph" in str(e.value)
    assert train.build_config(train.parse_args(["--num_agents", "4", "--graph"])).graph is True


# ---------------------------------------------------------------------------------- evaluation
def test_evaluate_refuses_gain_refinement_and_a_contradicting_flag(tmp_path, capsys):
    import evaluate as evaluate_cli
    from macbf_gnn_amd.evaluate import EvalConfig, evaluate
    base = dict(num_agents=6, episodes=1, max_steps=2)
    with pytest.raises(ValueError) as e:
        evaluate(Controller(4, residual=True), CBF(4), EvalConfig(refine_space="gains", **base))
    assert "ctrl_residual" in str(e.value) and "refine_space='gains'" in str(e.value)
    evaluate(Controller(4), CBF(4), EvalConfig(refine_space="gains", **base))                 # the plain law: as before
    out = evaluate(Controller(4, residual=True), CBF(4), EvalConfig(**base))
    assert 0.0 <= out["safety_rate"] <= 1.0
    # the CLI builds what the checkpoint holds; a flag that contradicts it names both
    pr, pp = tmp_path / "res.pt", tmp_path / "plain.pt"
    torch.save({"controller": Controller(4, residual=True).state_dict(), "cbf": CBF(4).state_dict()}, pr)
    torch.save({"controller": Controller(4).state_dict(), "cbf": CBF(4).state_dict()}, pp)
    common = ["--num_agents", "6", "--episodes", "1", "--max_steps", "2", "--device", "cpu", "--no_refine"]
    assert evaluate_cli.main(common + ["--model_path", str(pr)])["ctrl_residual"] is True
    assert "ctrl_residual" not in evaluate_cli.main(common + ["--model_path", str(pp)])
    assert evaluate_cli.main(common + ["--ctrl_residual"])["ctrl_residual"] is True          # random init
    assert evaluate_cli.main(common + ["--ctrl_residual", "--model_path", str(pr)])["ctrl_residual"] is True
    capsys.readouterr()
    with pytest.raises(SystemExit):
        evaluate_cli.main(common + ["--ctrl_residual", "--model_path", str(pp)])
    err = capsys.readouterr().err
    assert "--ctrl_residual" in err and str(pp) in err and "controller_dec_net.6.weight" in err
    with pytest.raises(SystemExit):
        evaluate_cli.main(common[:-1] + ["--ctrl_residual", "--refine_space", "gains"])
    err = capsys.readouterr().err
    assert "ctrl_residual" in err and "refine_space" in err


# ------------------------------------------------------------------------------- training steps
def test_oracle_engine_step_reaches_the_residual_rows():
    tr = _tr(N=10, B=2, T=6, ctrl_residual=True)
    assert tr.engine.name == "oracle"
    s, g = E.generate_batch(2, 10, seed=3)
    tr.engine.step(s, g)
    gW, gb = tr.controller.controller_dec_net[6].weight.grad, tr.controller.controller_dec_net[6].bias.grad
    assert tuple(gW.shape) == (6, 64)
    for x in (gW[4:], gb[4:]):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0
    plain = _tr(N=10, B=2, T=6)
    assert tr.fp.numel == plain.fp.numel + 2 * 64 + 2
    before = tr.fp.flat.clone()
    tr.train_step(s, g)
    assert not torch.equal(tr.controller.controller_dec_net[6].weight[4:], torch.zeros(2, 64))
    assert not torch.equal(before, tr.fp.flat)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


NE = 4


def _dp_cfg(B):
    return C.TrainConfig(num_agents=10, num_envs=B, inner_loops=6, device="cpu", seed=3, early_stop=True, train_steps=1,
                         ctrl_residual=True)


def _worker(rank, world, port, outdir):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                       "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank)})
    torch.set_num_threads(1)
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    dp = DP(device=torch.device("cpu"))
    s_all, g_all = E.generate_batch(NE, 10, seed=11)
    B = NE // world
    tr = Trainer(_dp_cfg(B), device=torch.device("cpu"), dp=dp)
    sl = slice(rank * B, (rank + 1) * B)
    tr.engine.step(s_all[sl], g_all[sl])
    tr.reduce_grad()
    torch.save(tr.fp.grad.clone(), os.path.join(outdir, f"grad{rank}.pt"))
    dp.shutdown()


@pytest.mark.timeout(600)
def test_dp2_reduces_the_longer_flat_gradient(tmp_path):
    """In the manner of tests/test_dp.py: the all-reduced gradient of a world-2 gloo step equals the
    single-process gradient on the concatenated env batch, residual rows included."""
    mp.start_processes(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    g0 = torch.load(tmp_path / "grad0.pt", weights_only=True)
    assert torch.equal(g0, torch.load(tmp_path / "grad1.pt", weights_only=True))
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    s_all, g_all = E.generate_batch(NE, 10, seed=11)
    tr = Trainer(_dp_cfg(NE), device=CPU, dp=DP(device=CPU))
    tr.engine.step(s_all, g_all)
    assert g0.numel() == tr.fp.numel == _tr(N=10).fp.numel + 2 * 64 + 2
    torch.testing.assert_close(g0, tr.fp.grad, rtol=2e-4, atol=1e-7)
    o = {pn: (o_, n) for m, pn, shape, o_, n in tr.fp.specs}[W4]
    assert float(g0[o[0] + 4 * 64:o[0] + o[1]].abs().max()) > 0
