"""Device-resident CBF safety filter (``csrc/refine.hip``): the action refinement of
``evaluate.refine_actions`` without autograd and without a host synchronisation.

    h      = h(s_t) on the kNN slots (one ``cbf_fwd`` launch), fixed over the loop
    s'     = s + dt [v, a + delta]        (agents; obstacle nodes are static)
    loss   = sum_e relu(-(h(s') - h + dt alpha h))
    delta <- delta - lr dloss/ddelta      for at most ``loops`` iterations

``used`` counts the iterations that still had an edge with a non-zero hinge gradient (violated,
and inside the radius at s' -- outside it h(s') is 0 whatever the action); once an iteration has
none, the remaining launches return at once and the actions stay as they are. ``viol`` is the
hinge sum at the last evaluated iterate, as ``refine_actions`` reports it.

``env_active`` (B,) bool / uint8 on the device masks whole envs out of a batch (episodes that are
already over): their actions come back unchanged, and ``used`` / ``viol`` / the counts are those
of the remaining envs, bit for bit what the filter gives on that sub-batch alone. The mask is read
by the kernels; the host never looks at it.

Two implementations, bit for bit the same results. ``"loop"``: ``loops`` x (refine_grad,
refine_update) launches, any scene. ``"persistent"``: envs of at most ``native.SMALL_MAXN`` graph
nodes run the whole loop in one launch, one workgroup per env (``refine_small_kernel``); each env
stops on its own and reports per-env result words, which ``native.refine_reduce`` turns into the
loop path's ``used`` / ``viol`` / counts on the device. ``impl=None`` chooses: ``MACBF_REFINE_SMALL``
(0 / 1) if set, else the persistent kernel where it measured faster (``AUTO_PERSISTENT``: bf16 envs
of at most 32 graph nodes; docs/PERF.md, "Persistent filter") and the loop everywhere else.

``a_max`` (opt-in): the per-axis actuator limit of ``evaluate.py``'s module docstring. The action is
clamped with a torch op before the launches, both update kernels project ``delta`` onto
[-a_max - a_c, a_max - a_c] after every step (behind one scalar test: without a limit they run the
instructions they always ran), and the result is clamp(a_c + delta, -a_max, a_max).

``coupling`` (opt-in; ``evaluate.py``'s module docstring states the rule): ``"joint"`` is the filter
above. ``"local"`` is the decentralised filter -- every agent refines its own action against its
neighbours' nominal next states -- with two implementations of its own, bit for bit the same results:
``"fused"`` (``refine_local_kernel``: a 2-agent x 16-slot tile runs its whole loop in one wave, delta in
registers, one launch for any scene; the default) and ``"loop"`` (``refine_grad_local_kernel`` /
``refine_update_local_kernel``: the loop path's instantiations without the neighbour's delta and the
in-edge sum). Neither builds a reverse CSR. The persistent filter has no local variant, and the fused
kernel no joint one: both pairs are errors that name the option.
"""
from __future__ import annotations

import torch

from .. import config as C
from .. import knobs
from ..evaluate import COUPLINGS, check_a_max
from . import graph, native
from .packing import module_pack


IMPLS = (None, "loop", "persistent")
LOCAL_IMPLS = (None, "fused", "loop")
# coupling="local", impl=None: precision -> the smallest scene (agents in the batch) from which the loop
# path is the default. Empty: the fused kernel measured 2.2x (1024 x 4 fp32: 0.78 against 1.73 ms per
# call) and 2.5x (32 x 8 bf16: 0.28 against 0.68 ms) faster than the loop path (docs/PERF.md,
# "Decentralised filter").
AUTO_LOCAL_LOOP = {}
# impl=None: precision -> the largest env (graph nodes) for which the persistent kernel is the
# default, i.e. where its minimum beat the loop path's by more than that path's spread
# (docs/PERF.md, "Persistent filter"): bf16 at 32 nodes (0.50 against 0.71 ms per call); at 64 nodes
# it is 5 % behind, and in fp32 (x3, 4 waves, three MFMAs per product) it is behind at every size.
AUTO_PERSISTENT = {"bf16": 32}


def choose_impl(impl, prec: str, Nn: int, K: int, coupling: str = "joint", agents: int = 0) -> str:
    """"loop" or "persistent" for a scene of Nn graph nodes per env and K slots (module docstring).
    An explicit "persistent" on a scene that is not eligible is an error, never a fall-back.
    coupling="local": "fused" or "loop" (``agents``: B * N, for ``AUTO_LOCAL_LOOP``)."""
    if coupling not in COUPLINGS:
        raise native.NativeError(f"unknown coupling {coupling!r} ('joint' or 'local')")
    if coupling == "local":
        if impl == "persistent":
            raise native.NativeError("impl='persistent' has no local coupling: with coupling='local' use impl='fused', "
                                     "'loop' or None")
        if impl not in LOCAL_IMPLS:
            raise native.NativeError(f"unknown safety-filter impl {impl!r} for coupling='local' (None, 'fused' or 'loop')")
        if impl is not None:
            return impl
        return "loop" if agents >= AUTO_LOCAL_LOOP.get(prec, float("inf")) else "fused"
    if impl == "fused":
        raise native.NativeError("unknown safety-filter impl 'fused' for coupling='joint': impl='fused' is the local "
                                 "coupling's kernel; use impl='loop', 'persistent' or None with coupling='joint'")
    if impl not in IMPLS:
        raise native.NativeError(f"unknown safety-filter impl {impl!r} (None, 'loop' or 'persistent')")
    ok = native.refine_small_eligible(Nn, K)
    if impl == "persistent" and not ok:
        raise native.NativeError(f"the persistent filter takes envs of at most {native.SMALL_MAXN} graph nodes and "
                                 f"K <= {C.MAX_TOP_K} (got Nn = {Nn}, K = {K}); use impl='loop' or None")
    if impl is not None:
        return impl
    forced = knobs.get_int("MACBF_REFINE_SMALL", -1)
    if forced >= 0:
        return "persistent" if forced and ok else "loop"
    return "persistent" if ok and Nn <= AUTO_PERSISTENT.get(prec, 0) else "loop"


def safety_filter(cbf_module, s, a, idx, obstacles=None, loops: int = C.REFINE_LOOPS,
                  lr: float = C.REFINE_LEARNING_RATE, return_trace: bool = False, *, env_active=None,
                  num_blocks=None, impl=None, a_max=None, return_delta: bool = False, coupling: str = "joint"):
    """s (B, N, 2D), a (B, N, D), idx (B, N, K) on the HIP device, obstacles (B, M, D) or None ->
    (a_refined (B, N, D), used, viol); ``used`` (int64) and ``viol`` (float64) are 0-d device
    tensors -- the caller decides when to read them. ``return_trace=True`` appends a dict with the
    per-iteration active-edge counts ``counts`` (loops,), and ``hn`` (B, N, K) / ``active`` (B, N, K)
    bool of the first iteration (tests). ``env_active`` (B,): envs with False / 0 are not refined
    (module docstring); ``num_blocks`` overrides the workgroup count of the loop path's gradient
    kernel (and of the fused local kernel); ``impl`` None / "loop" / "persistent", with ``coupling="local"``
    None / "fused" / "loop" (module docstring). ``a_max``: the actuator limit
    (module docstring); the trace dict also holds the raw ``delta`` (B, N, D), and ``return_delta=True``
    appends it as a last element of its own."""
    a_max = check_a_max(a_max)
    choose_impl(impl, "fp32", 1, 1, coupling)       # an unknown coupling / impl pair: refused before any work
    if not s.is_cuda:
        raise native.NativeError("the safety filter runs on the HIP device")
    if s.dim() != 3 or a.dim() != 3 or idx.dim() != 3:
        raise native.NativeError("s (B, N, 2D), a (B, N, D) and idx (B, N, K) are required")
    B, N, SD = s.shape
    D = SD // 2
    K = idx.shape[-1]
    loops = int(loops)
    dev = s.device
    mp = module_pack("cbf", cbf_module, dev)
    if mp.prec == "fp16":
        raise native.NativeError("safety filter: fp16 is not supported (the -1 upstream gradient has no loss "
                                 "scaling); use fp32 or bf16")
    if mp.dim != D:
        raise native.NativeError(f"the CBF was built for {mp.dim}-D states, s is {D}-D")
    obs = None
    if obstacles is not None:
        obs = obstacles if obstacles.dim() == 3 else obstacles.unsqueeze(0)
        obs = obs.expand(B, *obs.shape[-2:]).float()
    with torch.no_grad():
        w, v, rm = mp.pack(list(cbf_module.parameters()))
        S = graph.node_records(s, obs)                           # (B, Nn, W)
        Nn = S.shape[1]
        idx32 = idx.to(torch.int32).contiguous()
        a32 = a.detach().float().contiguous()
        if a_max is not None:
            a32 = a32.clamp(-a_max, a_max)
        delta = torch.zeros_like(a32)
        h = torch.empty(1, B, N, K, dtype=torch.float32, device=dev)
        which = choose_impl(impl, mp.prec, Nn, K, coupling, B * N)
        persistent, local = which == "persistent", coupling == "local"
        hn = flags = None
        if return_trace:
            hn = torch.zeros(B, N, K, dtype=torch.float32, device=dev)
            flags = torch.zeros(B, N, K, dtype=torch.uint8, device=dev)
        ctl = ew = None
        if persistent:
            ew = torch.zeros(B, loops, 2, dtype=torch.int64, device=dev)
        else:
            ctl = torch.zeros(max(2 * loops, 2), dtype=torch.int64, device=dev)
        if loops > 0:
            native.cbf_fwd(S.view(1, *S.shape), idx32.view(1, B, N, K), w, mp.off["w1f"], v, two=False, h_out=h,
                           prec=mp.prec)
            rptr = redges = None
            if not local:
                rptr = torch.empty(B, Nn + 1, dtype=torch.int32, device=dev)
                redges = torch.empty(B, N * K, dtype=torch.int32, device=dev)
                native.rev_csr(idx32, rptr, redges, n_nodes=Nn)
            if which == "fused":
                native.refine_local(S, idx32, a32, delta, h.view(B, N, K), w, mp.off["w1f"], rm, v, ctl, loops=loops,
                                    lr=lr, prec=mp.prec, hn_out=hn, flag_out=flags, env_active=env_active,
                                    num_blocks=num_blocks, a_max=a_max)
            elif persistent:
                native.refine_small(S, idx32, a32, delta, h.view(B, N, K), w, mp.off["w1f"], rm, v, rptr, redges, ew,
                                    loops=loops, lr=lr, prec=mp.prec, hn_out=hn, flag_out=flags,
                                    env_active=env_active, a_max=a_max)
            else:
                dEv = torch.empty(B, N, K, D, dtype=torch.float32, device=dev)
                native.refine(S, idx32, a32, delta, h.view(B, N, K), w, mp.off["w1f"], rm, v, dEv, rptr, redges, ctl,
                              loops=loops, lr=lr, prec=mp.prec, hn_out=hn, flag_out=flags, env_active=env_active,
                              num_blocks=num_blocks, a_max=a_max, local=local)
        if persistent:
            used, viol, counts = native.refine_reduce(ew)
        else:
            counts = ctl[0:2 * loops:2]
            used = (counts > 0).sum()
            if loops > 0:
                # the violation of the last evaluated iterate: iteration `used` if it ran (it then counted
                # no active edge), else the last one; selected on the device (no host read)
                last = torch.clamp(used, max=loops - 1).view(1)
                viol = ctl[1:2 * loops:2].index_select(0, last).view(()).double() / native.FX_VIOL
            else:
                viol = torch.zeros((), dtype=torch.float64, device=dev)
        out = a32 + delta
        if a_max is not None:
            out = out.clamp(-a_max, a_max)
        out = out.to(a.dtype)
    res = (out, used, viol)
    if return_trace:
        res += ({"counts": counts.clone(), "hn": hn, "active": flags.bool() if flags is not None else None,
                 "delta": delta},)
    return res + (delta,) if return_delta else res
