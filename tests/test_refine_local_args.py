"""What the decentralised filter's entry points refuse before any device work, on host tensors: the
pairs of coupling and implementation that do not exist, an unknown coupling, fp16, and the gain
refinement."""
import pytest
import torch

from macbf_gnn_amd.evaluate import EvalConfig, evaluate, refine_actions
from macbf_gnn_amd.models import CBF, Controller
from macbf_gnn_amd.ops import native
from macbf_gnn_amd.ops.refine import choose_impl, safety_filter
from macbf_gnn_amd.validate import check_config
from macbf_gnn_amd import config as C


def _host():
    torch.manual_seed(0)
    B, N, D, K = 1, 6, 2, 3
    return CBF(2 * D), torch.randn(B, N, 2 * D), torch.randn(B, N, D), torch.zeros(B, N, K, dtype=torch.long)


def test_persistent_has_no_local_coupling():
    cbf, s, a, idx = _host()
    with pytest.raises(native.NativeError, match="impl='persistent'.*local"):
        safety_filter(cbf, s, a, idx, impl="persistent", coupling="local")
    with pytest.raises(native.NativeError, match="persistent"):
        choose_impl("persistent", "bf16", 32, 12, "local")


def test_unknown_coupling():
    cbf, s, a, idx = _host()
    with pytest.raises(native.NativeError, match="unknown coupling 'both'"):
        safety_filter(cbf, s, a, idx, coupling="both")
    with pytest.raises(ValueError, match="unknown coupling 'both'"):
        refine_actions(cbf, s, a, idx, 1, coupling="both")
    with pytest.raises(ValueError, match="unknown coupling"):
        evaluate(Controller(4), cbf, EvalConfig(num_agents=6, refine_coupling="both"), device=torch.device("cpu"))


def test_fused_has_no_joint_coupling():
    cbf, s, a, idx = _host()
    with pytest.raises(native.NativeError, match="impl='fused'.*joint"):
        safety_filter(cbf, s, a, idx, impl="fused")
    with pytest.raises(native.NativeError, match="impl='fused'"):
        safety_filter(cbf, s, a, idx, impl="fused", coupling="joint")


def test_the_choice_of_implementation():
    assert choose_impl(None, "fp32", 1024, 12, "local", 4096) in ("fused", "loop")
    assert choose_impl("fused", "bf16", 32, 12, "local") == "fused"
    assert choose_impl("loop", "bf16", 32, 12, "local") == "loop"
    assert choose_impl(None, "fp32", 1024, 12) == "loop"          # the joint choice is what it was
    with pytest.raises(native.NativeError, match="unknown safety-filter impl"):
        choose_impl("small", "fp32", 32, 12, "local")


def test_fp16_is_refused():
    B, N, Nn, K, D = 1, 4, 4, 3, 2
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt)
    with pytest.raises(native.NativeError, match="fp16 is not supported"):
        native.refine_local(z(B, Nn, 4), z(B, N, K, dt=torch.int32), z(B, N, D), z(B, N, D), z(B, N, K),
                            z(80 * 512, dt=torch.float16), 0, z(128 * 68 + 64 * 148, dt=torch.float16), z(260),
                            z(4, dt=torch.int64), loops=2, lr=0.3, prec="fp16")


def test_gain_refinement_has_no_local_coupling():
    cfg = EvalConfig(num_agents=6, refine_space="gains", refine_coupling="local")
    with pytest.raises(ValueError, match="refine_coupling='local'.*refine_space='gains'"):
        evaluate(Controller(4), CBF(4), cfg, device=torch.device("cpu"))
    # without the filter the pair means nothing and is let through
    evaluate(Controller(4), CBF(4), EvalConfig(num_agents=6, refine=False, refine_space="gains", refine_coupling="local",
                                               episodes=1, max_steps=1), device=torch.device("cpu"))


def test_validation_coupling_is_checked():
    cfg = C.TrainConfig(num_agents=8, device="cpu", val_refine_coupling="both")
    with pytest.raises(ValueError, match="val_refine_coupling"):
        check_config(cfg)
    assert C.TrainConfig(num_agents=8).val_refine_coupling == "joint"


def test_host_evaluation_with_local_coupling():
    """The reference path end to end on the host: the same result keys as the joint filter."""
    torch.manual_seed(0)
    ctrl, cbf = Controller(4), CBF(4)
    base = dict(num_agents=16, num_envs=2, episodes=1, max_steps=3, refine_loops=2)
    j = evaluate(ctrl, cbf, EvalConfig(**base), device=torch.device("cpu"))
    l = evaluate(ctrl, cbf, EvalConfig(refine_coupling="local", **base), device=torch.device("cpu"))
    assert set(j) == set(l) and 0.0 <= l["safety_rate"] <= 1.0
