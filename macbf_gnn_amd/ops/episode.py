"""Device-resident closed-loop episodes (``csrc/episode.hip`` + ``EpisodeDriver`` in
``csrc/runtime.cpp``): what ``Validator.rollout`` and ``evaluate.rollout_eval`` do step by step in
torch ops, as one native call.

Per step the driver enqueues, on the current stream: one scan of s_t (the kNN lists and, from the
same launch, the safety count that belongs to the step before), the controller forward, with
``refine`` the safety filter (``cbf_fwd`` for h(s_t), ``rev_csr``, then the loop or the persistent
filter, as ``ops.refine.choose_impl`` picks; with ``coupling="local"``, the decentralised filter of
``evaluate.py``'s module docstring: ``cbf_fwd``, the control words' memset and one ``refine_local``
launch -- no ``rev_csr``, no loop of launches), the Euler step and the step's bookkeeping. Both
networks are packed once per call. The host reads the "some env still runs" word every
``check_every`` steps and nothing else; a step issued after every env finished changes neither the
states nor a count, so the result does not depend on that period.

``mask_done`` chooses the one rule in which the two Python episodes differ: True (``validate.py``)
an env whose episode is over is no longer refined, False (``evaluate.py``) the filter keeps running
on every env until the batch stops.

The integer results equal the Python path's; the states are the same bit for bit (the kernels use
its expressions, ``a32 + delta`` and ``s + [v, u] * dt``, in fp32 without contraction). The done
decision compares an integer sum of per-agent distances (2^-32 fixed point) with the threshold
instead of an fp32 mean: the two can differ only for a mean within summation error (about
N * 2^-24 of its value) of ``DIST_MIN_CHECK``.

``a_max`` (opt-in) is the per-axis actuator limit of ``evaluate.py``'s module docstring: after the
controller forward ``episode_limit_kernel`` clamps the actions in place, the filter projects its
correction, and the Euler step applies clamp(a_c + delta). ``action_stats`` adds the integer action
statistics (``evaluate.ACTION_STATS``), accumulated by the Euler step's kernel over the agents of the
envs that are active at the start of each step.
"""
from __future__ import annotations

import torch

from .. import config as C
from . import graph, native
from . import layout as L
from .packing import module_pack
from .refine import choose_impl


def run_episodes(controller, cbf, s0, g, obstacles=None, *, refine, loops=C.REFINE_LOOPS,
                 lr=C.REFINE_LEARNING_RATE, max_steps=C.INNER_LOOPS, top_k=C.TOP_K, mask_done=True, check_every=5,
                 impl=None, return_state=False, a_max=None, action_stats=False, coupling="joint"):
    """s0 (B, N, 2D), g (B, N, D) on the HIP device, obstacles (B, M, D) or None -> the batch's totals,
    an int64 device vector in the order of ``validate.COUNTS``; with ``return_state`` also the final
    states (B, N, 2D) and the final ``active`` (B,) bool. ``impl``: the filter's implementation
    (None / "loop" / "persistent", ``ops.refine``); ``coupling`` "joint" / "local" (with "local" ``impl`` is
    None / "fused" / "loop"). Nothing is read on the host except the driver's
    flag; the caller decides when to read the vector. ``a_max``: the actuator limit (module docstring);
    ``action_stats=True`` appends one more element to the result, the int64 device vector of
    ``evaluate.ACTION_STATS``."""
    if not isinstance(s0, torch.Tensor) or not s0.is_cuda:
        raise native.NativeError("run_episodes runs on the HIP device")
    if s0.dim() != 3 or g.dim() != 3 or s0.shape[-1] not in (4, 6) or g.shape != (*s0.shape[:2], s0.shape[-1] // 2):
        raise native.NativeError("s0 (B, N, 2D) and g (B, N, D) with D = 2 or 3 are required")
    B, N, SD = s0.shape
    D = SD // 2
    K = min(int(top_k), N)
    if K > C.MAX_TOP_K:
        raise native.NativeError(f"K = {K} neighbour slots, the kernels take at most MAX_TOP_K = {C.MAX_TOP_K}")
    loops, max_steps = int(loops), int(max_steps)
    if refine:
        choose_impl(impl, "fp32", 1, 1, coupling)       # an unknown coupling / impl pair: refused before any work
    if a_max is not None:                       # the fp32 value the kernels compare with
        a_max = float(torch.tensor(native._a_max(a_max), dtype=torch.float32))
    dev = s0.device
    cmp_ = module_pack("ctrl", controller, dev)
    bmp = None
    if refine:
        bmp = module_pack("cbf", cbf, dev)
        if bmp.prec == "fp16":
            raise native.NativeError("safety filter: fp16 is not supported (the -1 upstream gradient has no loss "
                                     "scaling); use fp32 or bf16")
        if bmp.dim != D:
            raise native.NativeError(f"the CBF was built for {bmp.dim}-D states, s is {D}-D")
    if cmp_.dim != D:
        raise native.NativeError(f"the controller was built for {cmp_.dim}-D states, s is {D}-D")
    obs = None
    if obstacles is not None:
        obs = obstacles if obstacles.dim() == 3 else obstacles.unsqueeze(0)
        obs = obs.expand(B, *obs.shape[-2:]).float()
    with torch.no_grad():
        cw, cv, crm = cmp_.pack(list(controller.parameters()))          # once per call
        bw = bv = brm = None
        if refine:
            bw, bv, brm = bmp.pack(list(cbf.parameters()))
        S0 = graph.node_records(s0, obs)                                # (B, Nn, W); obstacle rows stay as they are
        if S0.data_ptr() == s0.data_ptr():
            S0 = S0.clone()                                             # never write into the caller's states
        Nn = S0.shape[1]
        filt = bool(refine) and loops > 0
        which = choose_impl(impl, bmp.prec, Nn, K, coupling, B * N) if filt else None
        persistent, local, fused = which == "persistent", filt and coupling == "local", which == "fused"
        i64 = dict(dtype=torch.int64, device=dev)
        st = torch.zeros(native.EP_WORDS, **i64)
        st[0] = 1
        buf = dict(S0=S0, S1=S0.clone(), G=g.detach().float().contiguous(),
                   idx=torch.empty(B, N, K, dtype=torch.int32, device=dev),
                   A=torch.empty(B, N, D, dtype=torch.float32, device=dev),
                   pooled=torch.empty(B, N, L.pooled_row(cmp_.prec), dtype=cw.dtype, device=dev),
                   argmax=torch.empty(B, N, 128, dtype=torch.uint8, device=dev),
                   perm=torch.empty(B, Nn, dtype=torch.int32, device=dev), st=st,
                   dist_fx=torch.zeros(B, **i64), safe=torch.zeros(B, dtype=torch.float32, device=dev),
                   active=torch.ones(B, dtype=torch.uint8, device=dev),
                   prev_active=torch.zeros(B, dtype=torch.uint8, device=dev), out=torch.empty(native.EP_OUT, **i64))
        if action_stats:
            buf.update(act_st=torch.zeros(native.EP_ACT_WORDS, **i64), act_out=torch.empty(native.EP_ACT_WORDS, **i64))
        if filt:
            buf.update(delta=torch.zeros(B, N, D, dtype=torch.float32, device=dev),
                       h=torch.empty(B, N, K, dtype=torch.float32, device=dev))
            if not local:
                buf.update(rptr=torch.empty(B, Nn + 1, dtype=torch.int32, device=dev),
                           redges=torch.empty(B, N * K, dtype=torch.int32, device=dev))
            if persistent:
                buf["ew"] = torch.zeros(B, loops, 2, **i64)
            else:
                buf["ctl"] = torch.zeros(2 * loops, **i64)
                if not fused:
                    buf["dEv"] = torch.empty(B, N, K, D, dtype=torch.float32, device=dev)
        _, cur = native.episode_run(buf, K=K, max_steps=max_steps, check_every=check_every, refine=refine, loops=loops,
                                    lr=lr, mask_done=mask_done, persistent=persistent, ctrl=(cw, cv, crm, cmp_),
                                    cbf=(bw, bv, brm, bmp) if refine else None, a_max=a_max, local=local, fused=fused)
        res = (buf["out"],)
        if return_state:
            s_fin = native.from_records(buf["S1" if cur else "S0"][:, :N]).to(s0.dtype).contiguous()
            res += (s_fin, buf["active"].bool())
        if action_stats:
            res += (buf["act_out"],)
        return res if len(res) > 1 else res[0]
