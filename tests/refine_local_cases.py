"""Inputs shared by the decentralised-filter tests (tests/test_refine_local_ref.py on the host,
tests/test_gpu_refine_local.py on the device): the scenes of tests/test_gpu_refine.py built on the
host with that file's recipe, the perturbation of the locality check, and a planted graph whose
neighbour slots are obstacle nodes only."""
import functools

import torch

from macbf_gnn_amd import config as C
from macbf_gnn_amd import env as E
from macbf_gnn_amd import oracle as O
from macbf_gnn_amd.models import CBF
from test_gpu_refine import CASES

DTA = C.TIME_STEP * C.ALPHA_CBF
PERTURBED = 19                  # the agent of env 0 whose action the locality check changes
PERTURBATION = 1.5


@functools.lru_cache(maxsize=None)
def host_inputs(name):
    """(cbf, s, a, idx, obs) of a case on the host -- tests/test_gpu_refine._inputs without the copy."""
    dim, nobs, N, B, seed = CASES[name]
    s, _, obs = E.generate_scenarios(B, N, dim, nobs, seed)
    torch.manual_seed(seed)
    cbf = CBF(2 * dim)
    s = s.clone()
    s[..., dim:] = torch.randn(B, N, dim) * 0.5
    a = torch.randn(B, N, dim) * 2.0
    idx = O.knn_idx(s, min(12, N), O.with_obstacles(s, obs))
    return cbf, s, a, idx, obs


def perturbed_action(a):
    a2 = a.clone()
    a2[0, PERTURBED] += PERTURBATION
    return a2


def unaffected_rows(idx):
    """(B, N) bool: the agents that neither are the perturbed one nor list it among their slots."""
    keep = torch.ones(idx.shape[:2], dtype=torch.bool, device=idx.device)
    keep[0] = ~(idx[0] == PERTURBED).any(-1)
    keep[0, PERTURBED] = False
    return keep


def first_iteration(cbf, s, a, idx, obs):
    """(deriv, active) of every slot at delta = 0 from the fp32 oracle: the joint and the local filter
    see the same s' there."""
    p = {k: v.detach() for k, v in cbf.params_dict().items()}
    with torch.no_grad():
        h = O.cbf_forward(p, s, idx, nodes=O.with_obstacles(s, obs))
        D = s.shape[-1] // 2
        sn = s + torch.cat([s[..., D:], a], -1) * C.TIME_STEP
        nodes = O.with_obstacles(sn, obs)
        hn = O.cbf_forward(p, sn, idx, nodes=nodes)
        mask = O.cbf_features(sn, idx, nodes)[1].bool()
    deriv = hn - h + DTA * h
    return deriv, mask & (deriv < 0)


@functools.lru_cache(maxsize=None)
def planted_obstacle_graph():
    """(cbf, s, a, idx, obs): the agents of case 3d_obs2 moved next to obstacle points, slot 0 the agent
    itself and every other slot one of its 11 nearest OBSTACLE nodes -- no agent lists another agent, so
    the joint filter has no in-edge term and no neighbour delta: it is the local filter.

    The last bias is raised until h of the self slot is positive. The self slot's features are the
    same constants at s and s' ([0, 1, sqrt(eps) - r]), so its deriv is dt alpha h_self for every agent:
    with h_self > 0 it is never active. (An active self slot changes nothing in the kernels, which
    zero its record, but the autograd reference adds +g and -g of that slot to the row's sum in
    separate roundings.) The raise moves deriv of the other slots by dt alpha bias only."""
    cbf0, s, a, _, obs = host_inputs("3d_obs2")
    B, N, SD = s.shape
    D = SD // 2
    M = obs.shape[1]
    g = torch.Generator().manual_seed(23)
    s = s.clone()
    s[..., :D] = obs[:, torch.arange(N) % M] + 0.25 * torch.randn(B, N, D, generator=g)
    d = s[..., :D].unsqueeze(-2) - obs.unsqueeze(-3)                     # (B, N, M, D)
    near = torch.sort(O.sq_dist(d, D), dim=-1, stable=True).indices[..., :11] + N
    idx = torch.cat([torch.arange(N).view(1, N, 1).expand(B, N, 1), near], -1)
    import copy
    cbf = copy.deepcopy(cbf0)
    p = {k: v.detach() for k, v in cbf.params_dict().items()}
    with torch.no_grad():
        h_self = float(O.cbf_forward(p, s, idx, nodes=O.with_obstacles(s, obs))[0, 0, 0])
        if h_self <= 0.0:
            cbf.cbf_net[6].bias += 0.05 - h_self
    return cbf, s, a, idx, obs
