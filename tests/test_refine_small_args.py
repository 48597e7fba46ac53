"""The device-free parts of the persistent safety filter (ops/native.py ``refine_small``,
``refine_reduce``; ops/refine.py ``choose_impl``): the argument checks that come before any launch,
the reduction of the per-env result words to the loop path's ``used`` / ``viol`` / ``counts`` on a
hand-written tensor, and the choice of the implementation."""
import pytest
import torch

from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops import refine as R

FX = 2 ** 32


def _host_args(B=2, N=10, Nn=10, K=10, D=2, loops=4, half=torch.bfloat16):
    return dict(S=torch.zeros(B, Nn, 4 if D == 2 else 8), idx=torch.zeros(B, N, K, dtype=torch.int32),
                a=torch.zeros(B, N, D), delta=torch.zeros(B, N, D), h=torch.zeros(B, N, K),
                wpack=torch.zeros(80 * 512, dtype=half), f_bwd=0, wrm=torch.zeros(128 * 68 + 64 * 148, dtype=half),
                wvec=torch.zeros(260), rptr=torch.zeros(B, Nn + 1, dtype=torch.int32),
                redges=torch.zeros(B, N * K, dtype=torch.int32), ew=torch.zeros(B, loops, 2, dtype=torch.int64))


def test_refine_small_refuses_more_than_small_maxn_nodes():
    assert native.SMALL_MAXN == 64
    with pytest.raises(native.NativeError, match="at most SMALL_MAXN = 64 graph nodes, got 65"):
        native.refine_small(**_host_args(N=53, Nn=65, K=12), loops=4, lr=0.1)
    assert native.refine_small_eligible(64, 16) and native.refine_small_eligible(1, 1)
    assert not native.refine_small_eligible(65, 12) and not native.refine_small_eligible(64, 17)
    assert not native.refine_small_eligible(0, 1) and not native.refine_small_eligible(10, 0)


def test_refine_small_refuses_fp16():
    with pytest.raises(native.NativeError, match="fp16 is not supported"):
        native.refine_small(**_host_args(half=torch.float16), loops=4, lr=0.1)
    with pytest.raises(native.NativeError, match="fp16 is not supported"):
        native.refine_small(**_host_args(half=torch.float16), loops=4, lr=0.1, prec="fp16")
    with pytest.raises(native.NativeError, match="bf16 or fp16"):
        native.refine_small(**_host_args(half=torch.float32), loops=4, lr=0.1)


@pytest.mark.parametrize("what", ["no_S", "S_dim", "loops", "no_ew", "host"])
def test_refine_small_argument_checks(what):
    args, loops = _host_args(), 4
    if what == "no_S":
        args["S"], msg = None, "node records"
    elif what == "S_dim":
        args["S"], msg = torch.zeros(10, 4), "node records"
    elif what == "loops":
        loops, msg = -1, "loops must be >= 0"
    elif what == "no_ew":
        args["ew"], msg = None, "ew is required"
    else:
        msg = "must be on the HIP device"          # everything else in order: host tensors are refused
    with pytest.raises(native.NativeError, match=msg):
        native.refine_small(**args, loops=loops, lr=0.1)


def test_reduce_of_hand_written_words():
    """Three envs, 5 iterations. Env 0 works in iterations 0..2 and stops at 3; env 1 never has work
    (stops at 0: one violation value throughout); env 2 is masked out (all zero)."""
    ew = torch.tensor([[[7, 90 * FX], [4, 50 * FX], [1, 20 * FX], [0, 6 * FX], [0, 6 * FX]],
                       [[0, 3 * FX], [0, 3 * FX], [0, 3 * FX], [0, 3 * FX], [0, 3 * FX]],
                       [[0, 0], [0, 0], [0, 0], [0, 0], [0, 0]]], dtype=torch.int64)
    used, viol, counts = native.refine_reduce(ew)
    assert used.dtype == torch.int64 and used.dim() == 0 and int(used) == 3           # the slowest env
    assert viol.dtype == torch.float64 and viol.dim() == 0 and float(viol) == 9.0     # iteration 3: 6 + 3 + 0
    assert counts.dtype == torch.int64 and counts.tolist() == [7, 4, 1, 0, 0]


def test_reduce_when_the_last_iteration_still_works():
    """Env 0 has work in every iteration: the violation is the last iteration's (index loops - 1),
    where env 1, stopped at iteration 1, contributes its stopping value."""
    ew = torch.tensor([[[5, 40 * FX + 1], [5, 30 * FX], [5, 20 * FX + 2]],
                       [[2, 8 * FX], [0, 1 * FX], [0, 1 * FX]]], dtype=torch.int64)
    used, viol, counts = native.refine_reduce(ew)
    assert int(used) == 3 and counts.tolist() == [7, 5, 5]
    assert float(viol) == (21 * FX + 2) / FX                                          # an integer sum, then / 2^32


def test_reduce_of_nothing():
    used, viol, counts = native.refine_reduce(torch.zeros(3, 4, 2, dtype=torch.int64))
    assert int(used) == 0 and float(viol) == 0.0 and counts.tolist() == [0, 0, 0, 0]
    used, viol, counts = native.refine_reduce(torch.zeros(3, 0, 2, dtype=torch.int64))    # loops = 0
    assert int(used) == 0 and float(viol) == 0.0 and viol.dtype == torch.float64 and counts.shape == (0,)
    for bad in (torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, 4, 2, dtype=torch.int32)):
        with pytest.raises(native.NativeError):
            native.refine_reduce(bad)


def test_choice_of_the_implementation(monkeypatch):
    monkeypatch.delenv("MACBF_REFINE_SMALL", raising=False)
    assert R.choose_impl("loop", "bf16", 10, 10) == "loop"
    assert R.choose_impl("persistent", "fp32", 64, 16) == "persistent"
    assert R.choose_impl("loop", "bf16", 1024, 12) == "loop"
    with pytest.raises(native.NativeError, match="at most 64 graph nodes"):
        R.choose_impl("persistent", "bf16", 65, 12)
    with pytest.raises(native.NativeError, match="unknown safety-filter impl"):
        R.choose_impl("fused", "bf16", 10, 10)
    # automatic: never the persistent kernel on a scene it does not take, whatever the knob says
    assert R.choose_impl(None, "bf16", 65, 12) == "loop"
    for prec in ("bf16", "fp32", "fp16"):
        top = R.AUTO_PERSISTENT.get(prec, 0)
        assert top <= native.SMALL_MAXN
        for Nn in (1, 32, 33, 64):
            assert R.choose_impl(None, prec, Nn, 12) == ("persistent" if Nn <= top else "loop")
    monkeypatch.setenv("MACBF_REFINE_SMALL", "1")
    assert R.choose_impl(None, "fp32", 64, 12) == "persistent" and R.choose_impl(None, "fp32", 65, 12) == "loop"
    assert R.choose_impl("loop", "fp32", 64, 12) == "loop"
    monkeypatch.setenv("MACBF_REFINE_SMALL", "0")
    assert R.choose_impl(None, "bf16", 32, 12) == "loop" and R.choose_impl("persistent", "bf16", 32, 12) == "persistent"
