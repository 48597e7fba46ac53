"""The scenes of the training-limit tests (tests/test_train_limit.py, tests/test_gpu_train_limit.py).

Each case: the TrainConfig entries of a scene (seed 0, 5 steps, no early stop), the actuator limit A
and the share of the valid raw action components with |a_q| > A that the float32 oracle's own rollout
under that limit has. A is the median |a_q| of the oracle's unlimited rollout of the scene (n32 0.2166,
n96_3d 0.2172, n128 0.2324, n40_3d 0.2200), to two digits -- for n32 to one digit: under 0.22 that scene's trajectory
puts ONE first-layer relu pre-activation of the node MLP (unit 47, one agent-step) within the fp32
kernels' product rounding of zero, the kernels and the fp32 oracle take different sides of it, and
that unit alone moves the gradient of controller_dec_net.0 by 1.7e-3 (its bias gradient differs in
entry 47 by 1.15e-6, in every other entry by <= 1.3e-9; the unlimited step and the limits 0.2 and 0.3
agree to 1e-5). A relu tie of the comparison, as tests/test_gpu_fp32.py documents for its own seeds,
not the mask. The share was measured once (tests/test_train_limit.py test_share_condition re-measures it on
the CPU and fails on a drift). The GPU tests assert the same [0.1, 0.9] band on the kernels' actions.
"""
SHARE_BAND = (0.1, 0.9)
T = 5

CASES = {
    "n32": (dict(num_agents=32, num_envs=2), 0.2, 0.5813),
    "n96_3d": (dict(num_agents=96, num_envs=2, dim=3, num_obstacles=2), 0.22, 0.5316),
    "n128": (dict(num_agents=128, num_envs=2), 0.23, 0.5395),
    "n40_3d": (dict(num_agents=40, num_envs=2, dim=3, num_obstacles=2), 0.22, 0.5425),
}


def config(name, device, **kw):
    from macbf_gnn_amd import config as C
    scene, a_max, _ = CASES[name]
    base = dict(inner_loops=T, early_stop=False, seed=0, device=device, a_max=a_max, **scene)
    base.update(kw)
    return C.TrainConfig(**base)


def saturated_share(A, valid, a_max):
    """A (..., N, D) raw actions with `valid` broadcastable over the leading dims -> share of the valid
    components with |a_q| > a_max."""
    m = valid[..., None, None].expand_as(A)
    return float((A[m].abs() > a_max).float().mean())
