"""The device-free parts of the native closed-loop episodes (ops/native.py ``episode_advance``,
``episode_tally``, ``episode_final``, ``episode_run``; ops/episode.py; the ``rollout_impl`` /
``val_impl`` options): every argument check comes before any launch, so it can be exercised with
host tensors, and an option the native path cannot honour is an error that names it."""
import types

import pytest
import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import validate as V
from macbf_gnn_amd.evaluate import EvalConfig, check_rollout_impl, evaluate, rollout_eval
from macbf_gnn_amd.models import CBF, Controller
from macbf_gnn_amd.ops import episode, native


def _state(B=2, N=5, Nn=7, D=2):
    W = 4 if D == 2 else 8
    return dict(S_cur=torch.zeros(B, Nn, W), G=torch.zeros(B, N, D), st=torch.zeros(native.EP_WORDS, dtype=torch.int64),
                dist_fx=torch.zeros(B, dtype=torch.int64), safe=torch.zeros(B), active=torch.ones(B, dtype=torch.uint8),
                prev_active=torch.zeros(B, dtype=torch.uint8))


def _advance(B=2, N=5, Nn=7, D=2):
    W = 4 if D == 2 else 8
    return dict(_state(B, N, Nn, D), S_next=torch.zeros(B, Nn, W), A=torch.zeros(B, N, D), delta=torch.zeros(B, N, D))


BAD = {
    "dtype": ("A", lambda t: t.double(), "A must be a torch.float32 tensor"),
    "dtype_words": ("st", lambda t: t.int(), "st must be a torch.int64 tensor"),
    "dtype_mask": ("active", lambda t: t.bool(), "active must be a torch.uint8 tensor"),
    "shape": ("delta", lambda t: t[:, :4], r"delta shape \(2, 4, 2\) != \(2, 5, 2\)"),
    "shape_dist": ("dist_fx", lambda t: torch.zeros(3, dtype=torch.int64), r"dist_fx shape \(3,\) != \(2,\)"),
    "contiguous": ("A", lambda t: torch.zeros(2, 2, 5).transpose(1, 2), "A must be contiguous"),
    "records": ("S_cur", lambda t: torch.zeros(2, 7, 5), "4 .2-D. or 8 .3-D. floats wide"),
    "agents": ("G", lambda t: torch.zeros(2, 9, 2), "N = 9 agents but the records hold 7 nodes"),
    "host": (None, None, "must be on the HIP device"),       # everything in order: host tensors are refused
}


@pytest.mark.parametrize("what", list(BAD))
def test_advance_argument_checks(what):
    args = _advance()
    name, f, msg = BAD[what]
    if name is not None:
        args[name] = f(args[name])
    with pytest.raises(native.NativeError, match=msg):
        native.episode_advance(**args)


def test_advance_refuses_one_buffer_for_both_states():
    args = _advance()
    args["S_next"] = None
    with pytest.raises(native.NativeError, match="S_next is required"):
        native.episode_advance(**args)


@pytest.mark.parametrize("what", ["dtype_words", "shape_dist", "dtype_mask", "records", "host"])
def test_tally_and_final_share_the_state_checks(what):
    name, f, msg = BAD[what]
    for fn, extra in ((native.episode_tally, {}), (native.episode_final, {"out": torch.zeros(8, dtype=torch.int64)})):
        args = _state()
        if name is not None:
            args[name] = f(args[name])
        with pytest.raises(native.NativeError, match=msg):
            fn(**args, **extra)


def test_tally_result_word_checks():
    i64 = torch.int64
    with pytest.raises(native.NativeError, match="loops must be >= 0"):
        native.episode_tally(**_state(), loops=-1)
    with pytest.raises(native.NativeError, match="exclude each other"):
        native.episode_tally(**_state(), ctl=torch.zeros(8, dtype=i64), ew=torch.zeros(2, 4, 2, dtype=i64), loops=4)
    with pytest.raises(native.NativeError, match=r"at least 2\*loops = 8 words"):
        native.episode_tally(**_state(), ctl=torch.zeros(6, dtype=i64), loops=4)
    with pytest.raises(native.NativeError, match="ctl must be a torch.int64 tensor"):
        native.episode_tally(**_state(), ctl=torch.zeros(8, dtype=torch.int32), loops=4)
    with pytest.raises(native.NativeError, match=r"ew shape \(2, 3, 2\) != \(2, 4, 2\)"):
        native.episode_tally(**_state(), ew=torch.zeros(2, 3, 2, dtype=i64), loops=4)
    with pytest.raises(native.NativeError, match=r"out shape \(7,\) != \(8,\)"):
        native.episode_final(**_state(), out=torch.zeros(7, dtype=i64))
    with pytest.raises(native.NativeError, match="out must be a torch.int64 tensor"):
        native.episode_final(**_state(), out=torch.zeros(8))


def _packs(half=torch.bfloat16, prec="bf16"):
    cmp_ = types.SimpleNamespace(prec=prec, off={"ew1f": 0, "nw1f": 18})
    bmp = types.SimpleNamespace(prec=prec, off={"w1f": 0})
    ctrl = (torch.zeros(80 * 512, dtype=half), torch.zeros(352), None, cmp_)
    cbf = (torch.zeros(80 * 512, dtype=half), torch.zeros(260), torch.zeros(128 * 68 + 64 * 148, dtype=half), bmp)
    return ctrl, cbf


def _buffers():
    buf = _state()
    buf["S0"] = buf.pop("S_cur")
    return buf


def _run(buf=None, K=4, half=torch.bfloat16, prec="bf16", **kw):
    ctrl, cbf = _packs(half, prec)
    args = dict(K=K, max_steps=3, check_every=5, refine=True, loops=4, lr=0.3, mask_done=True, persistent=False,
                ctrl=ctrl, cbf=cbf)
    args.update(kw)
    return native.episode_run(_buffers() if buf is None else buf, **args)


def test_driver_checks_before_any_launch():
    with pytest.raises(native.NativeError, match="K = 17 outside 1..16"):
        _run(K=17)
    with pytest.raises(native.NativeError, match="fp16 is not supported"):
        _run(half=torch.float16, prec="fp16")
    with pytest.raises(native.NativeError, match="max_steps >= 0, check_every >= 1"):
        _run(check_every=0)
    with pytest.raises(native.NativeError, match="refine needs the packed CBF"):
        _run(cbf=None)
    with pytest.raises(native.NativeError, match="bad K=8 for Nn=7"):
        _run(K=8)
    with pytest.raises(native.NativeError, match="node records"):
        _run({})
    buf = _buffers()
    with pytest.raises(native.NativeError, match="S1 is required"):
        _run(buf)
    buf["S1"] = torch.zeros(2, 7, 4, dtype=torch.float64)
    with pytest.raises(native.NativeError, match="S1 must be a torch.float32 tensor"):
        _run(buf)
    buf["S1"] = torch.zeros(2, 7, 4)
    buf["idx"] = torch.zeros(2, 5, 3, dtype=torch.int32)
    with pytest.raises(native.NativeError, match=r"idx shape \(2, 5, 3\) != \(2, 5, 4\)"):
        _run(buf)
    buf["idx"] = torch.zeros(2, 5, 4, dtype=torch.int32)
    buf["A"] = torch.zeros(2, 2, 5).transpose(1, 2)
    with pytest.raises(native.NativeError, match="A must be contiguous"):
        _run(buf)
    buf["A"] = torch.zeros(2, 5, 2)
    with pytest.raises(native.NativeError, match="perm is required"):
        _run(buf)                                   # and with everything present: host tensors are refused
    buf.update(perm=torch.zeros(2, 7, dtype=torch.int32), out=torch.zeros(8, dtype=torch.int64),
               pooled=torch.zeros(2, 5, 128, dtype=torch.bfloat16), argmax=torch.zeros(2, 5, 128, dtype=torch.uint8),
               delta=torch.zeros(2, 5, 2), h=torch.zeros(2, 5, 4), rptr=torch.zeros(2, 8, dtype=torch.int32),
               redges=torch.zeros(2, 20, dtype=torch.int32), dEv=torch.zeros(2, 5, 4, 2))
    with pytest.raises(native.NativeError, match="ctl is required"):
        _run(buf)
    buf["ctl"] = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(native.NativeError, match=r"ew shape \(2, 3, 2\) != \(2, 4, 2\)"):
        _run(dict(buf, ew=torch.zeros(2, 3, 2, dtype=torch.int64)), persistent=True)
    with pytest.raises(native.NativeError, match="must be on the HIP device"):
        _run(buf)


def test_run_episodes_refuses_what_it_cannot_run():
    ctrl, cbf = Controller(4), CBF(4)
    s0, g = torch.zeros(2, 5, 4), torch.zeros(2, 5, 2)
    with pytest.raises(native.NativeError, match="runs on the HIP device"):
        episode.run_episodes(ctrl, cbf, s0, g, None, refine=True)
    with pytest.raises(native.NativeError, match="runs on the HIP device"):
        episode.run_episodes(ctrl, cbf, s0, g, None, refine=False, top_k=17)


def _eval_cfg(**kw):
    return EvalConfig(num_agents=4, num_envs=1, episodes=1, max_steps=2, rollout_impl="native", **kw)


@pytest.mark.parametrize("kw,name", [(dict(refine_impl="native", diagnose=True), "diagnose"),
                                     (dict(refine_impl="native", refine_space="gains"), "refine_space"),
                                     (dict(refine_impl="native", early_stop=False), "early_stop"),
                                     (dict(refine_impl="autograd"), "refine_impl"),
                                     (dict(refine_impl="native"), "HIP device"),
                                     (dict(refine=False), "HIP device")])
def test_native_rollout_names_the_option_it_cannot_honour(kw, name):
    cfg = _eval_cfg(**kw)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="rollout_impl='native'") as e:
        check_rollout_impl(cfg, cpu)
    assert name in str(e.value)
    with pytest.raises(ValueError, match=name):
        rollout_eval(Controller(4), CBF(4), torch.zeros(1, 4, 4), torch.zeros(1, 4, 2), cfg)
    with pytest.raises(ValueError, match=name):
        evaluate(Controller(4), CBF(4), cfg, device=cpu)


def test_rollout_impl_defaults_and_unknown_values():
    assert EvalConfig().rollout_impl == "python" and C.TrainConfig().val_impl == "python"
    check_rollout_impl(EvalConfig(diagnose=True, early_stop=False, refine_space="gains"), torch.device("cpu"))
    with pytest.raises(ValueError, match="unknown rollout_impl 'fast'"):
        check_rollout_impl(EvalConfig(rollout_impl="fast"), torch.device("cpu"))
    # the option checks do not depend on the device: on a HIP device they are the same errors
    with pytest.raises(ValueError, match="diagnose"):
        check_rollout_impl(_eval_cfg(refine_impl="native", diagnose=True), torch.device("cuda"))
    check_rollout_impl(_eval_cfg(refine_impl="native"), torch.device("cuda"))
    check_rollout_impl(_eval_cfg(refine=False, refine_impl="autograd", refine_space="gains"), torch.device("cuda"))


def test_check_config_rejects_native_validation_on_cpu():
    with pytest.raises(ValueError, match="val_impl='native'.*HIP device"):
        V.check_config(C.TrainConfig(num_agents=4, device="cpu", val_every=1, val_impl="native"))
    with pytest.raises(ValueError, match="val_impl='native'.*HIP device"):
        V.check_config(C.TrainConfig(num_agents=4, val_every=1, val_impl="native"), torch.device("cpu"))
    with pytest.raises(ValueError, match="val_impl must be one of"):
        V.check_config(C.TrainConfig(num_agents=4, device="cpu", val_every=1, val_impl="fast"))
    V.check_config(C.TrainConfig(num_agents=4, device="hip", val_every=1, val_impl="native"))
    V.check_config(C.TrainConfig(num_agents=4, device="cpu", val_every=1))
    with pytest.raises(ValueError, match="needs a HIP device"):
        V.Validator(C.TrainConfig(num_agents=4, device="cpu", val_every=1, val_envs=1), torch.device("cpu"), impl="native")
    from macbf_gnn_amd.engine import Trainer
    with pytest.raises(ValueError, match="val_impl='native'"):
        Trainer(C.TrainConfig(num_agents=4, device="cpu", val_every=1, val_impl="native"), device=torch.device("cpu"))


def test_train_cli_flag():
    import train
    assert train.build_config(train.parse_args(["--num_agents", "4"])).val_impl == "python"
    assert train.build_config(train.parse_args(["--num_agents", "4", "--val_impl", "native"])).val_impl == "native"
    with pytest.raises(SystemExit):
        train.parse_args(["--num_agents", "4", "--val_impl", "fast"])
