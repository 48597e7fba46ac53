"""GPU: the zero-lag early-stop check of the native rollout driver (csrc/runtime.cpp
RolloutDriver::run). From the expected horizon on, the driver waits for the publication of step
t-1 after scan(t) and before ctrl(t), so the controller step past the horizon is not issued. The
expectation is a hint: with any value the horizon, the tail flag, the trajectory, the graphs and the
step's statistics are those of the lagged check, bit for bit; only the number of controller steps
issued changes -- T0 where the zero-lag check was on at the stop, T0 + 1 (the lagged check's) otherwise."""
import pytest
import torch

from macbf_gnn_amd import config as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TMAX = 30


def _trainer():
    from macbf_gnn_amd.engine import Trainer
    from macbf_gnn_amd.parallel import DP
    cfg = C.TrainConfig(num_agents=96, num_envs=2, inner_loops=TMAX, seed=1, device="hip")
    tr = Trainer(cfg, device=DEV, dp=DP(device=DEV))
    eng = tr.engine
    assert eng.Nn > 64 and not eng.small_rollout       # the per-step driver
    eng.check_every = 1                                # before the driver is built: a check after every step
    return tr


def _run(tr, s0, g, early_stop=True):
    eng = tr.engine
    seen = {}
    tail_scan = eng._tail_scan
    eng._tail_scan = lambda T, scanned: (seen.update(tail=bool(scanned)), tail_scan(T, scanned))[1]
    try:
        T = eng.rollout(s0, g, None, early_stop=early_stop)
    finally:
        eng._tail_scan = tail_scan
    safe, dist = eng.safe[: T + 1].clone(), eng.dist[:T].clone()       # (_counts zeroes the sums after reading them)
    valid = eng._counts(T)                                              # the step's statistics: validity, pooled counts
    torch.cuda.synchronize()
    out = dict(T=T, tail=seen["tail"], S=eng.S[: T + 1].clone(), A=eng.A[:T].clone(), idx=eng.idx[:T].clone(),
               safe=safe, dist=dist, valid=valid.clone(), counts=eng.counts.clone(), local=eng.local.clone())
    return out, eng._driver().ctrl_issued


def _same(a, b):
    assert a["T"] == b["T"] and a["tail"] == b["tail"]
    for k in ("S", "A", "idx", "safe", "dist", "valid", "counts", "local"):
        assert torch.equal(a[k], b[k]), k


def test_expected_horizon_is_a_hint():
    tr = _trainer()
    drv = tr.engine._driver()
    s0, g, _ = tr.sample()
    tr.engine.expect_horizon = False                  # the engine hands the switch to the driver at every rollout
    base, issued = _run(tr, s0, g)
    T0 = base["T"]
    assert 3 <= T0 < TMAX and base["tail"]            # the early stop triggered
    assert issued == T0 + 1                           # the lagged check: one controller step past the horizon
    assert drv.expected_horizon == T0                 # every published early-stop run leaves its horizon
    again, issued = _run(tr, s0, g)                   # the switch is off: the expectation is not used
    _same(again, base)
    assert issued == T0 + 1
    tr.engine.expect_horizon = True                   # on a live engine: read at the next rollout
    for exp, want in ((T0, T0), (T0 - 2, T0), (1, T0), (T0 + 1, T0 + 1), (TMAX, T0 + 1), (0, T0 + 1)):
        drv.set_expected_horizon(exp)
        assert drv.expected_horizon == exp
        got, issued = _run(tr, s0, g)
        _same(got, base)
        assert issued == want, (exp, issued, want)
        assert drv.expected_horizon == T0
    # without a setter: the second of two consecutive rollouts expects the first one's horizon
    got, issued = _run(tr, s0, g)
    _same(got, base)
    assert issued == T0


def test_no_early_stop_issues_every_step():
    tr = _trainer()
    drv = tr.engine._driver()
    s0, g, _ = tr.sample()
    drv.set_expected_horizon(2)
    got, issued = _run(tr, s0, g, early_stop=False)
    assert got["T"] == TMAX and not got["tail"] and issued == TMAX
    assert drv.expected_horizon == 2                  # nothing was awaited, nothing learnt
    # and the trajectory's first steps are those of the early-stopped rollout
    base, _ = _run(tr, s0, g)
    T0 = base["T"]
    assert T0 < TMAX
    assert torch.equal(got["S"][: T0 + 1], base["S"]) and torch.equal(got["A"][:T0], base["A"])
