"""Loader and validated launch wrappers for the gfx950 extension ``macbf_gnn_amd._C``.

The extension is built in-tree by ``csrc/build.py`` (``__graft_entry__.build()``). On a HIP
device there is no fallback: if the extension is missing or was built for another arch,
``lib()`` raises. Every wrapper checks device/dtype/contiguity/shape on the host before
passing raw device addresses to the kernels (an out-of-bounds kernel can take the GPU down,
so shapes are never trusted implicitly).
"""
from __future__ import annotations

import functools
import math
import os

import torch

from .. import config as C
from . import layout as L

_LIB = None


class NativeError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        alt = os.environ.get("MACBF_EXT")
        if alt:   # experiment builds (scripts/build_variants.sh) loaded in place of the in-tree .so
            import importlib.util
            import sys
            spec = importlib.util.spec_from_file_location("macbf_gnn_amd._C", alt)
            mod = importlib.util.module_from_spec(spec)
            sys.modules["macbf_gnn_amd._C"] = mod
            spec.loader.exec_module(mod)
        try:
            from .. import _C  # noqa: F401  (in-tree .so)
        except ImportError as e:  # pragma: no cover - exercised on GPU boxes only
            raise NativeError(
                "native extension macbf_gnn_amd._C is not built; run `python csrc/build.py` "
                f"(or __graft_entry__.build()) first: {e}") from e
        _LIB = _C
    return _LIB


_PROBE = None


def probe_lib():
    """The layout-probe extension (csrc/probe.hip, tests only; not part of _C)."""
    global _PROBE
    if _PROBE is None:
        lib()       # HIP runtime + the main extension first
        try:
            from .. import _probe  # noqa: F401
        except ImportError as e:  # pragma: no cover
            raise NativeError(f"probe extension macbf_gnn_amd._probe is not built: {e}") from e
        _PROBE = _probe
    return _PROBE


def available() -> bool:
    try:
        lib()
        return True
    except NativeError:
        return False


def stream_handle(device=None) -> int:
    """Raw hipStream_t of the current stream. Direct C calls (no torch.cuda device-index
    resolution): this runs once per kernel launch and the host issues ~10 launches per rollout
    step, ahead of a GPU that finishes a step in ~0.13 ms."""
    if device is None:
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    return int(torch.cuda.current_stream(device).cuda_stream)


@functools.lru_cache(maxsize=None)
def device_info(index: int = 0) -> dict:
    return dict(lib().device_info(index))


def num_cu(device=None) -> int:
    idx = device.index if isinstance(device, torch.device) and device.index is not None else torch.cuda.current_device()
    return int(device_info(idx).get("cu", 256))


def ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


def check(t, dtype, shape=None, name="tensor"):
    if t is None:
        return
    if not t.is_cuda:
        raise NativeError(f"{name} must be on the HIP device")
    if t.dtype != dtype:
        raise NativeError(f"{name} dtype {t.dtype} != {dtype}")
    if not t.is_contiguous():
        raise NativeError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise NativeError(f"{name} shape {tuple(t.shape)} != {tuple(shape)}")


HALF_DTYPES = (torch.bfloat16, torch.float16)


def _half(t, name, prec=None):
    """Kernel precision variant of a packed-weight tensor (csrc/prec.h): 0 bf16, 1 fp16, 2 the
    fp32-accurate 3-term split ("fp32", bf16 hi/lo planes). prec=None: from the dtype."""
    if t is None or t.dtype not in HALF_DTYPES:
        raise NativeError(f"{name} must be bf16 or fp16")
    if prec is None:
        return int(t.dtype == torch.float16)
    if prec not in L.PREC_CODE:
        raise NativeError(f"unknown precision {prec!r}")
    code = L.PREC_CODE[prec]
    if (code == 1) != (t.dtype == torch.float16):
        raise NativeError(f"{name}: dtype {t.dtype} does not match precision {prec}")
    return code


def _planes(code):
    return 2 if code == 2 else 1


def _prow(code):
    return 256 if code == 2 else 128


def _same_half(t, ref, name):
    if t is not None and t.dtype != ref.dtype:
        raise NativeError(f"{name} dtype {t.dtype} != weight dtype {ref.dtype}")


def _ok(rc, what):
    if rc != 0:
        raise NativeError(f"{what} launch failed: {rc} ({lib().err_str(rc) if rc > 0 else 'bad args'})")


# ----------------------------------------------------------------------------- node records
def rec_width(dim: int) -> int:
    """Floats per node record: D = 2 -> (x, y, vx, vy); D = 3 -> (x, y, z, 0, vx, vy, vz, 0)."""
    return 4 if dim == 2 else 8


def dim_of(S) -> int:
    w = S.shape[-1]
    if w == 4:
        return 2
    if w == 8:
        return 3
    raise NativeError(f"node records must be 4 (2-D) or 8 (3-D) floats wide, got {w}")


def to_records(s: torch.Tensor) -> torch.Tensor:
    """(..., 2D) states -> (..., rec_width(D)) kernel records (identity for D = 2)."""
    D = s.shape[-1] // 2
    if D == 2:
        return s.contiguous()
    z = torch.zeros(*s.shape[:-1], 1, dtype=s.dtype, device=s.device)
    return torch.cat([s[..., :3], z, s[..., 3:6], z], -1).contiguous()


def from_records(r: torch.Tensor) -> torch.Tensor:
    """Inverse of ``to_records``."""
    if r.shape[-1] == 4:
        return r
    return torch.cat([r[..., 0:3], r[..., 4:7]], -1)


# ----------------------------------------------------------------------------- kernels
SMALL_MAXN = 64             # envs up to this many graph nodes: persistent one-launch rollout (ctrl.hip)
SMALL_WAVES = 8


def small_apw(N: int) -> int:
    """Agents per wave of the persistent rollout's edge phase: the env's agents over its 8 waves."""
    a = -(-N // SMALL_WAVES)
    return max(2, min(32, a + (a & 1)))


SCAN_CONSTS = dict(r2_train=float(C.DIST_MIN_THRES * C.DIST_MIN_THRES), ttc_train=float(C.TIME_TO_COLLISION),
                   r2_check=float(C.DIST_MIN_CHECK * C.DIST_MIN_CHECK), ttc_check=float(C.TIME_TO_COLLISION_CHECK))
SCAN_MAX_N = 4096           # envs up to this many graph nodes are staged whole in LDS
SCAN_MAX_NODES = 262144     # beyond SCAN_MAX_N: global staging (csrc/scan.hip scan_stage_kernel); the
                            # culling boxes in LDS up to ~36 K nodes, read from the workspace above


def scan_ws_f4(Nn: int) -> int:
    """float4s of global scan staging per env (0 when the env fits LDS)."""
    if Nn <= SCAN_MAX_N:
        return 0
    Np = (Nn + 7) // 8 * 8
    nch = Np // 8
    nsc = (nch + 7) // 8
    return 2 * Np + 2 * (nch + nsc)


def scan_ws(B: int, Nn: int, device):
    """(workspace tensor or None, float4s per env) for scans of B envs of Nn graph nodes."""
    f4 = scan_ws_f4(Nn)
    if not f4:
        return None, 0
    return _workspace("scan", B * f4 * 16, device), f4
_perm_cache = {}
_perm_sorted = set()      # cached permutation buffers that hold a curve order


def _perm_buf(B, N, device):
    key = (B, N, str(device))
    t = _perm_cache.get(key)
    if t is None:
        t = torch.empty(B, N, dtype=torch.int32, device=device)
        _perm_cache[key] = t
    return t


def _scan_kw(S, idx, dang, cnt, safe, *, K, do_knn=True, do_safety=True, perm=None, n_agents=None, prev_idx=None,
             sort=True, lanes=0, stamps=None, ws=None):
    """scan's checks -> (the CellSortArgs fields (csrc/args.h) as a dict, or None when the curve order of
    the previous call is reused; the ScanArgs fields). ws: the caller's own (tensor or None, float4s per
    env) global staging instead of the cached per-stream one (the rollout driver keeps the pointer)."""
    if lanes not in (0, 4, 8):
        raise NativeError("lanes must be 0 (auto), 4 or 8")
    B, Nn = S.shape[0], S.shape[1]
    if stamps is not None:   # diagnostics (scripts/stamps_scan.py): [block][wave][16] int64, <= 512 waves per env
        if K != 12 or stamps.dtype != torch.int64 or stamps.numel() < B * 8192 or not stamps.is_contiguous():
            raise NativeError("scan stamps: K = 12 and a contiguous int64 buffer of B * 8192")
    D = dim_of(S)
    W = rec_width(D)
    N = Nn if n_agents is None else int(n_agents)     # centres = the first N nodes
    if Nn > SCAN_MAX_NODES or N > Nn:
        raise NativeError(f"scan: N <= Nn <= {SCAN_MAX_NODES} graph nodes per env (got {N}, {Nn})")
    if S.dtype != torch.float32 or S.stride(2) != 1 or S.stride(1) != W:
        raise NativeError(f"S must be float32 with contiguous (Nn,{W}) rows")
    if K < 1 or K > C.MAX_TOP_K or K > Nn:
        raise NativeError(f"bad K={K} for Nn={Nn}")
    if do_knn:
        if idx.dtype != torch.int32 or tuple(idx.shape) != (B, N, K) or idx.stride(2) != 1 or idx.stride(1) != K:
            raise NativeError("idx must be int32 (B,N,K) with contiguous (N,K)")
        if dang is not None and (dang.dtype != torch.uint8 or tuple(dang.shape) != (B, N, K)
                                 or dang.stride() != idx.stride()):
            raise NativeError("dang must be uint8 (B,N,K) with idx's strides")
        if cnt is not None and (cnt.dtype != torch.float32 or tuple(cnt.shape) != (B, 2) or cnt.stride(1) != 1):
            raise NativeError("cnt must be float32 (B,2)")
    if do_safety and safe is not None and (safe.dtype != torch.float32 or tuple(safe.shape) != (B,)):
        raise NativeError("safe must be float32 (B,)")
    if prev_idx is not None and (not do_knn or prev_idx.dtype != torch.int32 or tuple(prev_idx.shape) != (B, N, K)
                                 or prev_idx.stride(2) != 1 or prev_idx.stride(1) != K):
        raise NativeError("prev_idx must be int32 (B,N,K) with contiguous (N,K)")
    if perm is None:
        perm = _perm_buf(B, Nn, S.device)
        # never scan through a never-sorted (uninitialised) cached permutation: it indexes nodes
        key = (B, Nn, str(S.device))
        if not sort and key not in _perm_sorted:
            sort = True
        _perm_sorted.add(key)
    ws, ws_f4 = ws or scan_ws(B, Nn, S.device)
    if ws_f4 != scan_ws_f4(Nn) or (ws_f4 and ws.numel() < B * ws_f4 * 16):
        raise NativeError("scan workspace too small")
    cs = dict(S=ptr(S), s_env=S.stride(0) // W, B=B, N=Nn, L=float(max(1.0, N / C.AGENT_DENSITY) ** (1.0 / D)),
              perm=ptr(perm), rec=W // 4) if sort else None
    return cs, dict(S=ptr(S), s_env=S.stride(0) // W, perm=ptr(perm), B=B, N=N, K=K, idx=ptr(idx) if do_knn else 0,
                    i_env=idx.stride(0) if do_knn else 0, dang=ptr(dang) if do_knn else 0,
                    cnt=ptr(cnt) if do_knn else 0, c_env=cnt.stride(0) if (do_knn and cnt is not None) else 0,
                    safe=ptr(safe) if do_safety else 0, sf_env=safe.stride(0) if (do_safety and safe is not None) else 0,
                    do_knn=int(do_knn), do_safety=int(do_safety), Nn=Nn, dim=D, prev_idx=ptr(prev_idx),
                    pi_env=prev_idx.stride(0) if prev_idx is not None else 0, ws=ptr(ws), ws_env=int(ws_f4),
                    lanes=int(lanes), stamps=ptr(stamps), **SCAN_CONSTS)


def scan(S, idx, dang, cnt, safe, *, K, do_knn=True, do_safety=True, perm=None, n_agents=None, prev_idx=None,
         sort=True, lanes=0, stamps=None):
    """K1 over one timestep. S: (B, N, 4) view with env stride (may be a slice of a (B,T+1,N,4)
    buffer); idx/dang: (B, N, K) views; cnt: (B, 2) view; safe: (B,) view.

    Two launches: cell_sort orders each env's agents along a Hilbert curve, then the scan walks
    candidates outward along it (results are order independent; the order only keeps the
    wave-divergent top-K insertion rare). prev_idx (B, N, K): the previous step's kNN of the same
    agents; their current distances bound the K-th distance (tighter culling, same result).
    sort=False reuses the curve order of the previous call on the same perm buffer (the agents
    moved one step: slightly looser culling, identical results). lanes: lanes per agent (0: by
    grid size -- 8 when 4-lane 256-thread blocks leave CUs idle; 4 or 8 forces the layout; the
    lists, bits and counts are identical for either)."""
    cs, kw = _scan_kw(S, idx, dang, cnt, safe, K=K, do_knn=do_knn, do_safety=do_safety, perm=perm, n_agents=n_agents,
                      prev_idx=prev_idx, sort=sort, lanes=lanes, stamps=stamps)
    if cs:
        _ok(lib().cell_sort(stream=stream_handle(), **cs), "cell_sort")
    _ok(lib().scan(stream=stream_handle(), **kw), "scan")


def scan_plan(B: int, N: int, K: int, *, Nn: int | None = None, dim: int = 2, prev: bool = True, do_knn: bool = True,
              do_safety: bool = True, lanes: int = 0) -> dict:
    """The launch plan ``scan`` picks for a call of this shape, without launching (csrc/scan.hip
    mb_scan_plan): block size ``bs``, lanes per agent ``lpa``, staging mode ``glb`` (0 LDS, 1 global
    records, 2 global boxes), cell-grid LDS allocated ``cells`` / searched ``use_cells``, grid side
    ``cell_g``, per-wave count atomics ``wave_atomic``, ``blocks`` and dynamic ``lds`` bytes. Tests
    use it to assert the instantiation they exercise."""
    Nn = N if Nn is None else int(Nn)
    v = lib().scan_plan(int(B), int(N), int(K), Nn, int(dim), int(bool(prev)), int(bool(do_knn)),
                        int(bool(do_safety)), int(lanes))
    return dict(zip(("bs", "lpa", "glb", "cells", "use_cells", "cell_g", "wave_atomic", "blocks", "lds"), v))


def scenario(S, G, *, seed, L, r=C.DIST_MIN_THRES, spread=C.GOAL_SPREAD, max_rounds=256, status=None, obs=None,
             lds_free=False):
    """S (B, >=N, W) agent records out (velocity 0), G (B, N, D) goals out; obs (B, M, D) static
    obstacle points kept > r from every start and goal. lds_free: the per-env arrays and cell grid
    in a global workspace even when they fit LDS (the large-env path; same results)."""
    B, N, D = G.shape
    W = rec_width(D)
    _records(S, "S", (B, N), W)
    check(G, torch.float32, (B, N, D), "G")
    check(status, torch.int32, (B,), "status")
    M = 0
    if obs is not None:
        M = obs.shape[1]
        check(obs, torch.float32, (B, M, D), "obs")
    base = (3 * N + M) * D * 4 + 5 * N + 16
    ws, ws_env = None, 0
    if lds_free or base + 4 * 2 ** D > 160 * 1024 - 64:
        # env too large for LDS: the sampler's arrays live in a per-env global workspace with a
        # full-resolution cell grid (same results: acceptance does not depend on the grid)
        span = float(L) + 2.0 * (float(spread) + float(r))
        import numpy as _np
        G1 = max(1, int(_np.floor(_np.float32(span) / _np.float32(r))))
        ws_env = (base + 4 * (G1 + 2) ** D + 255) // 256 * 256      # (+2: float rounding slack)
        ws = _workspace("scenario", B * ws_env, S.device)
    rc = lib().scenario(S=ptr(S), s_env=S.stride(0) // W, G=ptr(G), obs=ptr(obs), M=M, dim=D, B=B, N=N, L=float(L),
                        r=float(r), spread=float(spread), seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                        max_rounds=int(max_rounds), status=ptr(status), ws=ptr(ws), ws_env=int(ws_env),
                        stream=stream_handle())
    _ok(rc, "scenario")


_WS = {}


def _workspace(name, nbytes, device):
    """Cached uint8 device scratch, one per (name, device, current stream): grown on demand,
    reused in stream order. Per stream, because launches on different streams may run
    concurrently (the trainer samples the next iteration's scenarios on a side stream while
    the current one is still being sampled / simulated) and must not share scratch."""
    key = (name, str(device), stream_handle(device))
    t = _WS.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
        _WS[key] = t
    return t


def _rows(t, last, name, lead):
    """t is a float/bf16 view whose trailing dims are contiguous rows of width `last`."""
    if t is None:
        return
    if tuple(t.shape[:len(lead)]) != tuple(lead) or t.shape[-1] != last or t.stride(-1) != 1 \
            or t.stride(-2) != last:
        raise NativeError(f"{name}: expected {lead}x{last} with contiguous rows, got {tuple(t.shape)} {t.stride()}")


def _records(t, name, lead, W, min_rows=None):
    """(lead..., rows, W) float32 view with contiguous records; rows may exceed lead[-1] (nodes)."""
    if t is None:
        return
    if t.dtype != torch.float32 or t.dim() != len(lead) + 1 or tuple(t.shape[:len(lead) - 1]) != tuple(lead[:-1]) \
            or t.shape[-2] < lead[-1] or t.shape[-1] != W or t.stride(-1) != 1 or t.stride(-2) != W:
        raise NativeError(f"{name}: expected {lead}x{W} float32 records, got {tuple(t.shape)} {t.stride()}")


def _ctrl_fwd_kw(S, G, idx, wpack, f_edge, f_node, wvec, A, Sn, dist_sum, act_sum, noise=None, pooled=None, argmax=None,
                 prec=None, noise_key=None, noise_prob=0.0, noise_scale=0.0, noise_t=0, stamps=None, a_max=None, res=False):
    """ctrl_fwd's checks -> (the CtrlArgs fields (csrc/args.h) as a dict, precision code, num_cu).
    a_max (optional): the training rollout's per-axis actuator limit (oracle.py, "Actuator limit"); the
    key is only there with a limit, so a call without one passes what it always passed. res: the packed
    controller has the residual head (oracle.py, "Residual head": 3D rows in the last node layer, what
    ``PackedWeights.residual`` / ``ModulePack.residual`` say); the key is only there with it."""
    B, N, K = idx.shape
    D = dim_of(S)
    W = rec_width(D)
    if K < 1 or K > C.MAX_TOP_K:
        raise NativeError("K out of range")
    _records(S, "S", (B, N), W)
    _records(Sn, "Sn", (B, N), W)
    _rows(A, D, "A", (B, N))
    check(G, torch.float32, (B, N, D), "G")
    if idx.dtype != torch.int32 or idx.stride(2) != 1 or idx.stride(1) != K:
        raise NativeError("idx must be int32 (B,N,K)")
    f16 = _half(wpack, "wpack", prec)
    check(wpack, wpack.dtype, None, "wpack")
    check(wvec, torch.float32, None, "wvec")
    if wvec.numel() < 352 or wpack.numel() < (f_node + 54) * 512 * _planes(f16):
        raise NativeError("packed controller weights too small")
    if f16 == 2 and pooled is None:
        raise NativeError("the fp32 (x3) controller step needs the pooled buffer")
    for t, n in ((dist_sum, "dist_sum"), (act_sum, "act_sum")):
        if t is not None and (t.dtype != torch.int64 or tuple(t.shape) != (B,)):
            raise NativeError(f"{n} must be int64 (B,) fixed point")
    _rows(noise, D, "noise", (B, N))
    check(noise_key, torch.int64, (1,), "noise_key")
    if pooled is not None:
        _rows(pooled, _prow(f16), "pooled", (B, N))
        _same_half(pooled, wpack, "pooled")
    if argmax is not None:
        _rows(argmax, 128, "argmax", (B, N))
        if argmax.dtype != torch.uint8:
            raise NativeError("argmax must be uint8")
    if stamps is not None:   # diagnostics (scripts/stamps_ctrl.py): x3 step only, [blocks, 8 waves, 16]
        if f16 != 2 or stamps.dtype != torch.int64 or not stamps.is_contiguous():
            raise NativeError("ctrl_fwd stamps: int64 buffer of the x3 step")
        if stamps.numel() < 16 * 8 * 2 * num_cu(S.device):       # the grid is at most 2 blocks per CU
            raise NativeError("ctrl_fwd stamps buffer too small")
    kw = dict(S=ptr(S), s_env=S.stride(0) // W, G=ptr(G), idx=ptr(idx), i_env=idx.stride(0), B=B, N=N, K=K,
              wpack=ptr(wpack), f_edge=int(f_edge), f_node=int(f_node), wvec=ptr(wvec),
              A=ptr(A), a_env=A.stride(0) // D if A is not None else 0,
              Snext=ptr(Sn), sn_env=Sn.stride(0) // W if Sn is not None else 0,
              dist_sum=ptr(dist_sum), d_env=dist_sum.stride(0) if dist_sum is not None else 0,
              act_sum=ptr(act_sum), ac_env=act_sum.stride(0) if act_sum is not None else 0,
              noise=ptr(noise), n_env=noise.stride(0) // D if noise is not None else 0,
              dt=float(C.TIME_STEP), obs_r=float(C.OBS_RADIUS), sqrt3=float(C.SQRT3),
              pooled=ptr(pooled), p_env=pooled.stride(0) if pooled is not None else 0,
              argmax=ptr(argmax), am_env=argmax.stride(0) if argmax is not None else 0,
              dim=D, apw=ctrl_fwd_apw(B * N, S.device, N),
              noise_key=ptr(noise_key), noise_prob=float(noise_prob), noise_scale=float(noise_scale),
              noise_t=int(noise_t), stamps=ptr(stamps))
    if _a_max(a_max) > 0.0:
        kw["a_max"] = _a_max(a_max)
    if res:
        if stamps is not None:
            raise NativeError("ctrl_fwd stamps: the residual kernels have no phase clocks")
        kw["res"] = 1
    return kw, f16, num_cu(S.device)


def ctrl_fwd(S, G, idx, wpack, f_edge, f_node, wvec, A, Sn, dist_sum, act_sum, noise=None, pooled=None, argmax=None,
             prec=None, noise_key=None, noise_prob=0.0, noise_scale=0.0, noise_t=0, stamps=None, a_max=None, res=False):
    """Fused controller step on per-step views: S/Sn (B,Nn,W) node records (agents first),
    G (B,N,D), idx (B,N,K), A (B,N,D), dist_sum/act_sum (B,) int64 fixed point (x FX_DIST /
    x FX_ACT: order-independent integer atomics), pooled (B,N,128) bf16
    ((B,N,256) [hi | lo] rows for prec="fp32", required there), argmax (B,N,128) uint8.
    a_max (optional): Sn applies clamp(a, -a_max, a_max); A and act_sum keep the raw action.
    res: the packed controller has the residual head (a_q += y4[2D + q])."""
    kw, f16, ncu = _ctrl_fwd_kw(S, G, idx, wpack, f_edge, f_node, wvec, A, Sn, dist_sum, act_sum, noise, pooled, argmax,
                                prec, noise_key, noise_prob, noise_scale, noise_t, stamps, a_max, res)
    _ok(lib().ctrl_fwd(num_cu=ncu, prec=f16, stream=stream_handle(), **kw), "ctrl_fwd")


def ctrl_fwd_apw(total_agents: int, device, n_agents: int | None = None) -> int:
    """Agents per wave of the controller step's edge phase: 32, halved (down to 4) while the
    scene has fewer groups than eight per CU, so smaller scenes spread the edge phase over more
    waves; scenes of >= 8,192 agents stop at 8. Measured per-rank work of config #3 (fp32,
    interleaved, profiles/r6_runs/r6au/, r6av/, r6ap/): 65,536 agents 32 / 16 / 8 -> 10.08-10.27 /
    10.41-10.43 / 11.02 ms; 32,768: 16 -> 5.79 vs 6.17-6.24 (32) and 6.19 (8); 16,384: 8 -> 3.88-3.90
    vs 3.97-4.27 (16) and 4.17 (4); 8,192: 8 -> 2.80-2.82 vs 2.91-2.98 (4) and 2.91-2.96 (16). Any
    grouping gives the same results (the per-env sums are per-agent fixed-point integers).
    MACBF_CTRL_APW overrides (A/B runs)."""
    env = os.environ.get("MACBF_CTRL_APW")
    if env:
        return int(env)
    apw, cap = 32, 8 * num_cu(device)
    for cand in (16, 8, 4):
        if (total_agents + apw - 1) // apw >= cap or (cand == 4 and total_agents >= 8192):
            break
        apw = cand
    return apw


LOSS_CONSTS = (C.LOSS_EPS_DANG, C.TIME_STEP * C.ALPHA_CBF, C.LOSS_WEIGHTS[0], C.LOSS_WEIGHTS[1],
               C.LOSS_WEIGHTS[2], C.LOSS_WEIGHTS[3], C.LOSS_SCALE)
CBF_CONSTS = dict(obs_r=float(C.OBS_RADIUS), dist_thr=float(C.DIST_MIN_THRES))      # + dist_eps: per dimension


def _loss_consts(grad_scale=1.0, gscale=None):
    """LOSS_CONSTS with the upstream-gradient scale: a host factor and/or a device loss scale
    (fp16 dynamic scaling: 1-element float32 tensor read by the kernel, no host round trip)."""
    check(gscale, torch.float32, (1,), "gscale")
    return LOSS_CONSTS[:6] + (LOSS_CONSTS[6] * float(grad_scale), ptr(gscale))
CBF_FWD_WAVES = 4
CBF_PARTIAL = 18704
CBF_P_LOSS = 18692          # 10 loss partial sums in the CBF slab (fused mode)
CTRL_NODE_PARTIAL = 28896
CTRL_EDGE_PARTIAL = 10368
NODE_RM_ELEMS = 64 * 168 + 128 * 68 + 64 * 132 + 32 * 68     # csrc/ctrl.hip row-major node images


def cbf_fwd_grid(E: int, device) -> int:
    tiles = (E + 31) // 32
    return max(1, min((tiles + CBF_FWD_WAVES - 1) // CBF_FWD_WAVES, num_cu(device) * 4))


def _time_major_S(S, T, B, N, need):
    """S (>= T+need, B, Nn >= N, W) node records (agents first, then obstacle points)."""
    W = S.shape[-1] if S.dim() == 4 else 0
    if S.dtype != torch.float32 or S.dim() != 4 or S.shape[0] < T + need or S.shape[1] != B \
            or S.shape[2] < N or W not in (4, 8) or S.stride(3) != 1 or S.stride(2) != W:
        raise NativeError(f"S must be float32 (>=T+{need}, B, >=N, 4|8) with contiguous rows")
    return dim_of(S), W


def _cbf_fwd_kw(S, idx, wpack, f_fwd, wvec, *, dang=None, valid=None, two=True, h_out=None, hn_out=None,
                dh_out=None, counts=None, partial=None, num_blocks=None, prec=None):
    """cbf_fwd's checks -> (the CbfFwdArgs fields (csrc/args.h) as a dict, precision code, num_blocks)."""
    T, B, N, K = idx.shape
    check(idx, torch.int32, None, "idx")
    D, W = _time_major_S(S, T, B, N, 1 if two else 0)
    E = B * T * N * K
    check(dang, torch.uint8, (T, B, N, K), "dang")
    check(valid, torch.uint8, (T, B), "valid")
    check(h_out, torch.float32, (T, B, N, K), "h_out")
    check(hn_out, torch.float32, (T, B, N, K), "hn_out")
    check(dh_out, torch.float32, (2, T, B, N, K), "dh_out")
    if dh_out is not None:
        check(counts, torch.float32, None, "counts")
    f16 = _half(wpack, "wpack", prec)
    check(wpack, wpack.dtype, None, "wpack")
    check(wvec, torch.float32, None, "wvec")
    if wpack.numel() < (f_fwd + 34) * 512 * _planes(f16):
        raise NativeError("packed CBF weights too small")
    nb = num_blocks or cbf_fwd_grid(E, S.device)
    check(partial, torch.float32, (nb, 10), "partial")
    kw = dict(S=ptr(S), s_env=S.stride(1) // W, s_step=S.stride(0) // W, idx=ptr(idx), dang=ptr(dang),
              valid=ptr(valid), B=B, T=T, N=N, K=K, two=int(two), wpack=ptr(wpack), f_fwd=int(f_fwd),
              wvec=ptr(wvec), h_out=ptr(h_out), hn_out=ptr(hn_out), dh_out=ptr(dh_out), counts=ptr(counts),
              partial=ptr(partial), lc=LOSS_CONSTS, dim=D, dist_eps=float(C.CBF_DIST_EPS_COORD * D), **CBF_CONSTS)
    return kw, f16, nb


def cbf_fwd(S, idx, wpack, f_fwd, wvec, *, dang=None, valid=None, two=True, h_out=None, hn_out=None,
            dh_out=None, counts=None, partial=None, num_blocks=None, prec=None):
    """Time-major: S (>=T+two, B, N, 4); idx/dang/h (T, B, N, K); valid (T, B); dh (2, T, B, N, K)."""
    kw, f16, nb = _cbf_fwd_kw(S, idx, wpack, f_fwd, wvec, dang=dang, valid=valid, two=two, h_out=h_out, hn_out=hn_out,
                              dh_out=dh_out, counts=counts, partial=partial, num_blocks=num_blocks, prec=prec)
    _ok(lib().cbf_fwd(num_blocks=nb, prec=f16, stream=stream_handle(), **kw), "cbf_fwd")
    return nb


# ----------------------------------------------------------------------------- deduplicated h / h'
MATCH_BLOCK = 256


def cbf_match(idx, T, map1, src, cnt, *, recomputed=False, nev=None):
    """Deduplicate the h / h' evaluations of a rollout (csrc/dedup.hip).

    idx (>= T + recomputed, B, N, K) int32 neighbour slots. Writes map1 (T, B, N, K): the
    evaluation index of each slot's h' partner (< E: the next step's main slot with the same
    neighbour; >= E: an extra evaluation) and src (2E): the slot whose h' evaluation u is, or
    -1. cnt: int32 scratch (>= one entry per 256-row block). Returns the device int32 tensor
    [U] (evaluations; written into `nev` when given). Two launches, the exclusive scan of the
    per-row extras counts runs inside the kernels; stream-ordered, no host synchronisation."""
    _, B, N, K = idx.shape
    if idx.shape[0] < T + int(recomputed):
        raise NativeError("idx has too few steps")
    check(idx, torch.int32, None, "idx")
    E = T * B * N * K
    if 2 * E >= 2 ** 31:
        raise NativeError("too many edge evaluations for 32-bit indexing")
    check(map1, torch.int32, (T, B, N, K), "map1")
    check(src, torch.int32, (2 * E,), "src")
    rows = T * B * N
    nblk = (rows + MATCH_BLOCK - 1) // MATCH_BLOCK
    check(cnt, torch.int32, None, "cnt")
    if cnt.numel() < nblk:
        raise NativeError("cnt too small")
    if nev is None:
        nev = torch.empty(1, dtype=torch.int32, device=idx.device)
    check(nev, torch.int32, (1,), "nev")
    mode = 1 if recomputed else 0
    rowcnt = _workspace("match_rows", rows * 4, idx.device).view(torch.int32)
    # phase 0: match + everything but the extras' offsets; phase 1: the offsets (rows with extras)
    kw = dict(idx=ptr(idx), T=T, B=B, N=N, K=K, mode=mode, cnt=ptr(rowcnt), off=0, map1=ptr(map1), src=ptr(src),
              bsum=ptr(cnt))
    _ok(lib().cbf_match(phase=0, nev=0, stream=stream_handle(), **kw), "cbf_match/match")
    _ok(lib().cbf_match(phase=1, nev=ptr(nev), stream=stream_handle(), **kw), "cbf_match/extras")
    return nev


HFWD_WAVES = 8


def cbf_hfwd_grid(EV: int, device, per_cu: int | None = None) -> int:
    """Workgroups of an h evaluation launch: up to per_cu per CU (default 4)."""
    tiles = (EV + 31) // 32
    if per_cu is None:
        per_cu = 4
    return max(1, min((tiles + HFWD_WAVES - 1) // HFWD_WAVES, num_cu(device) * per_cu))


def _cbf_hfwd_kw(S, idx, idx1, src, nev, wpack, f_fwd, wrm, wvec, h_out, mask_out, num_blocks=None,
                 u_begin=0, u_end=None, prec=None):
    """cbf_hfwd's checks -> (the CbfFwdArgs fields (csrc/args.h) as a dict, precision code, num_blocks: 0
    for an empty host range, which launches nothing)."""
    T, B, N, K = idx.shape
    check(idx, torch.int32, None, "idx")
    check(idx1, torch.int32, (T, B, N, K), "idx1")
    D, W = _time_major_S(S, T, B, N, 1)
    E = B * T * N * K
    if 2 * E >= 2 ** 31:
        raise NativeError("too many edge evaluations for 32-bit indexing")
    cap = src.numel() if src is not None else 0
    if u_end is not None and not (0 <= u_begin <= u_end <= E):
        raise NativeError(f"host range [{u_begin}, {u_end}) must lie in the main slots [0, {E})")
    if cap < 2 * E or h_out is None or h_out.numel() < 2 * E or mask_out is None or mask_out.numel() < 2 * E:
        raise NativeError("src / h_out / mask_out must hold >= 2E evaluations")
    check(src, torch.int32, None, "src")
    check(nev, torch.int32, (1,), "nev")
    check(h_out, torch.float32, None, "h_out")
    check(mask_out, torch.uint8, None, "mask_out")
    f16 = _half(wpack, "wpack", prec)
    check(wpack, wpack.dtype, None, "wpack")
    check(wrm, wpack.dtype, (_planes(f16) * (128 * 68 + 64 * 148),), "wrm")
    check(wvec, torch.float32, None, "wvec")
    if wpack.numel() < (f_fwd + 2) * 512 * _planes(f16):
        raise NativeError("packed CBF weights too small")
    nb = num_blocks or cbf_hfwd_grid((u_end if u_end is not None else 2 * E) - u_begin, S.device)
    kw = dict(S=ptr(S), s_env=S.stride(1) // W, s_step=S.stride(0) // W, idx=ptr(idx), idx1=ptr(idx1),
              src=ptr(src), nev=ptr(nev), B=B, T=T, N=N, K=K, wpack=ptr(wpack), f_fwd=int(f_fwd), wrm=ptr(wrm),
              wvec=ptr(wvec), h_out=ptr(h_out), mask_out=ptr(mask_out), dim=D, u_begin=int(u_begin),
              u_end=int(u_end or 0), dist_eps=float(C.CBF_DIST_EPS_COORD * D), **CBF_CONSTS)
    return kw, f16, 0 if u_end is not None and u_end == u_begin else nb


def cbf_hfwd(S, idx, idx1, src, nev, wpack, f_fwd, wrm, wvec, h_out, mask_out, num_blocks=None,
             u_begin=0, u_end=None, prec=None):
    """h (masked) and the radius mask of every evaluation u_begin <= u < (u_end or nev) of the
    deduplicated list: S (>= T+1, B, N, W); idx / idx1 (T, B, N, K) (idx1 = idx for
    reuse_nbr_idx); src, h_out, mask_out (>= 2E,). Weights: w1f fragments at f_fwd of wpack + the
    row-major W2|W3 image. A host range [u_begin, u_end) within the main slots (u_end <= E) needs
    neither src nor nev contents: the rollout evaluates step t's main slots (idx[:t+1]) while
    later steps are still being simulated."""
    kw, f16, nb = _cbf_hfwd_kw(S, idx, idx1, src, nev, wpack, f_fwd, wrm, wvec, h_out, mask_out, num_blocks, u_begin,
                               u_end, prec)
    if nb:
        _ok(lib().cbf_hfwd(num_blocks=nb, prec=f16, stream=stream_handle(), **kw), "cbf_hfwd")
    return nb


DH_BLOCK = 256
DH_PARTIAL = 12


def cbf_dh_grid(EV: int, device) -> int:
    # >= ~8 evaluations per thread (the loop body is a chain of dependent gathers, map1 -> h),
    # 16 blocks per CU: enough loads in flight, a small partial-sum slab
    return max(1, min((EV + 8 * DH_BLOCK - 1) // (8 * DH_BLOCK), num_cu(device) * 16))


def cbf_dh(h, hmask, map1, src, nev, dang, valid, counts, dh, partial, *, grad_scale=1.0, blk_active=None,
           gscale=None):
    """Upstream dL/dh of every deduplicated evaluation (h-role + h'-role) and the 10 loss
    partial sums per block (slots as CBF_P_LOSS: [0, 0, 8 sums], padded) -> partial (nb, DH_PARTIAL)."""
    T, B, N, K = map1.shape
    E = T * B * N * K
    check(h, torch.float32, (2 * E,), "h")
    check(hmask, torch.uint8, (2 * E,), "hmask")
    check(map1, torch.int32, (T, B, N, K), "map1")
    check(src, torch.int32, (2 * E,), "src")
    check(nev, torch.int32, (1,), "nev")
    check(dang, torch.uint8, (T, B, N, K), "dang")
    check(valid, torch.uint8, (T, B), "valid")
    check(counts, torch.float32, None, "counts")
    check(dh, torch.float32, (2 * E,), "dh")
    if partial is None or partial.dim() != 2 or partial.shape[1] != DH_PARTIAL:
        raise NativeError(f"partial must be (nb, {DH_PARTIAL})")
    check(partial, torch.float32, None, "partial")
    nb = partial.shape[0]
    check(blk_active, torch.int32, (nb,), "blk_active")
    _ok(lib().cbf_dh(h=ptr(h), hmask=ptr(hmask), map1=ptr(map1), src=ptr(src), nev=ptr(nev), dang=ptr(dang),
                     valid=ptr(valid), B=B, T=T, N=N, K=K, counts=ptr(counts), lc=_loss_consts(grad_scale, gscale),
                     dh=ptr(dh), partial=ptr(partial), blk_active=ptr(blk_active), num_blocks=nb,
                     stream=stream_handle()), "cbf_dh")


def cbf_active(dh, nev, blk_active, act, nact=None, *, rec=None, src=None, idx=None, idx1=None):
    """Stable list of the evaluations with dh != 0 (cbf_dh's per-block counts blk_active, same
    grid): act[:nact] in index order. Returns the device int32 tensor [nact] (written into
    `nact` when given; block offsets are scanned in-kernel, one launch). The backward skips the
    rest: their upstream gradient, hence every contribution, is exactly zero.

    rec (int32 (2E, 4), the 16x16x32 x3 backward's input) replaces act: one record per active
    evaluation {u, e | pass << 31, neighbour j, dh bits}, resolved through src (deduplicated
    list) and idx (T,B,N,K) / idx1 (pass-1 neighbours, None = idx)."""
    check(dh, torch.float32, None, "dh")
    check(nev, torch.int32, (1,), "nev")
    check(blk_active, torch.int32, None, "blk_active")
    if rec is None:
        check(act, torch.int32, (dh.numel(),), "act")
    else:
        check(rec, torch.int32, (dh.numel(), 4), "rec")
        check(src, torch.int32, (dh.numel(),), "src")
        check(idx, torch.int32, None, "idx")
        check(idx1, torch.int32, tuple(idx.shape), "idx1")
        if 2 * idx.numel() != dh.numel():
            raise NativeError("rec: dh must cover the two passes of idx")
    if nact is None:
        nact = torch.empty(1, dtype=torch.int32, device=dh.device)
    check(nact, torch.int32, (1,), "nact")
    E = idx.numel() if idx is not None else 0
    _ok(lib().cbf_compact(dh=ptr(dh), nev=ptr(nev), blk_off=0, act=ptr(act) if rec is None else 0,
                          num_blocks=blk_active.numel(), blk_active=ptr(blk_active), nact=ptr(nact), src=ptr(src),
                          idx=ptr(idx), idx1=ptr(idx1), E=int(E), rec=ptr(rec), stream=stream_handle()), "cbf_compact")
    return nact


def node_act_bytes(prec) -> int:
    """Bytes per agent and step of the node activations the rollout keeps for the cooperative node
    backward (csrc/ctrl.hip NODE_ACT_BYTES: 1152 x3, 640 in the 16-bit builds)."""
    return int(lib().node_act_bytes(L.PREC_CODE[prec]))


def k16_wg_per_cu(prec, kernel: int) -> int:
    """Workgroups per CU of the 16x16x32 backward kernel `kernel` (0 CBF, 1 edge, 2 node) of the
    build of `prec` (csrc/mfma16.h: x3 one, the 1-pass builds two)."""
    return int(lib().k16_wg_per_cu(L.PREC_CODE[prec], kernel))


def cbf_bwd_grid(EV: int, device, prec=None) -> int:
    """Workgroups of the CBF backward over EV evaluations (128 per chunk): one per CU, or as many
    as the 16x16x32 kernel of `prec` keeps resident per CU when prec is given."""
    per_cu = k16_wg_per_cu(prec, 0) if prec is not None else 1
    return max(1, min((EV + 127) // 128, per_cu * num_cu(device)))


CBF_RM16 = 128 * 80 + 64 * 144     # elements per plane of the 16x16x32 W2 | W3 images (layout.cbf_rm16)


def cbf_bwd(S, idx, dh, wpack, f_bwd, wrm, wvec, *, passes=2, dE=None, partial=None, num_blocks=None,
            fused=False, dang=None, valid=None, counts=None, idx1=None, grad_scale=1.0, src=None, nev=None,
            act=None, nact=None, prec=None, gscale=None, stamps=None, rec=None, wrm16=None, w16=None, dbg=None):
    """dh (passes, T, B, N, K) -> dE (passes, T, B, N, K, 4), per-WG dW slabs (nb, CBF_PARTIAL).

    fused=True (training, passes=2): dh is not read; the kernel evaluates h and h' of every
    edge, forms the hinge-loss upstream gradients from dang (T,B,N,K), valid (T,B) and the
    global counts [n_dang, n_safe], and writes the 10 loss partial sums at CBF_P_LOSS.
    grad_scale multiplies the in-kernel upstream gradients (fp16 loss scaling); the loss sums
    are unscaled.

    src/nev (deduplicated list, non-fused, passes=2): evaluation u < nev is main slot u (u < E)
    or the extra evaluation of slot src[u] on s_{t+1}; dh / dE are indexed by u (sizes 2E)."""
    T, B, N, K = idx.shape
    check(idx, torch.int32, None, "idx")
    D, W = _time_major_S(S, T, B, N, passes - 1)
    if fused:
        if passes != 2:
            raise NativeError("fused CBF backward needs passes=2")
        check(dang, torch.uint8, (T, B, N, K), "dang")
        check(valid, torch.uint8, (T, B), "valid")
        check(counts, torch.float32, None, "counts")
        if dang is None or counts is None or counts.numel() < 2:
            raise NativeError("fused CBF backward needs dang and counts")
    else:
        check(dh, torch.float32, (passes, T, B, N, K), "dh")
    check(dE, torch.float32, (passes, T, B, N, K, W), "dE")
    if src is not None:
        if fused or passes != 2:
            raise NativeError("deduplicated CBF backward is non-fused with passes=2")
        check(src, torch.int32, (2 * B * T * N * K,), "src")
        check(nev, torch.int32, (1,), "nev")
    if act is not None:
        if src is None:
            raise NativeError("the active list needs the deduplicated evaluation list")
        check(act, torch.int32, (2 * B * T * N * K,), "act")
        check(nact, torch.int32, (1,), "nact")
    f16 = _half(wpack, "wpack", prec)
    if rec is not None:
        # 16x16x32 backward over cbf_compact's records (csrc/cbf16.h)
        if fused or src is None:
            raise NativeError("record backward: deduplicated non-fused path only")
        check(rec, torch.int32, (2 * B * T * N * K, 4), "rec")
        check(nact, torch.int32, (1,), "nact")
        check(wrm16, wpack.dtype, (_planes(f16) * CBF_RM16,), "wrm16")
        check(w16, wpack.dtype, (6 * 512 * _planes(f16),), "w16")
    check(wpack, wpack.dtype, None, "wpack")
    check(wvec, torch.float32, None, "wvec")
    if wpack.numel() < (f_bwd + 70) * 512 * _planes(f16):
        raise NativeError("packed CBF weights too small")
    check(wrm, wpack.dtype, (_planes(f16) * (128 * 68 + 64 * 148),), "wrm")
    if idx1 is not None:
        check(idx1, torch.int32, (T, B, N, K), "idx1")
    E = B * T * N * K
    if E * passes >= 2 ** 31:
        raise NativeError("too many edge evaluations for 32-bit indexing")
    nb = num_blocks or cbf_bwd_grid(E * passes, S.device)
    check(partial, torch.float32, (nb, CBF_PARTIAL), "partial")
    check(stamps, torch.int64, (nb, 8 if (rec is not None or f16 != 2) else 4, 8), "stamps")   # phase cycles
    rc = lib().cbf_bwd(S=ptr(S), s_env=S.stride(1) // W, s_step=S.stride(0) // W, idx=ptr(idx), B=B, T=T, N=N, K=K,
                       passes=int(passes), dh=0 if fused else ptr(dh), wpack=ptr(wpack), f_bwd=int(f_bwd), wrm=ptr(wrm),
                       wvec=ptr(wvec), dE=ptr(dE), partial=ptr(partial), fused=int(fused), dang=ptr(dang) if fused else 0,
                       valid=ptr(valid) if fused else 0, counts=ptr(counts) if fused else 0,
                       lc=_loss_consts(grad_scale, gscale), idx1=ptr(idx1), dim=D, num_blocks=nb, prec=f16, src=ptr(src),
                       nev=ptr(nev) if src is not None else 0, act=ptr(act),
                       nact=ptr(nact) if (act is not None or rec is not None) else 0, rec=ptr(rec), wrm16=ptr(wrm16),
                       w16=ptr(w16), dbg=ptr(dbg), stamps=ptr(stamps), dist_eps=float(C.CBF_DIST_EPS_COORD * D),
                       stream=stream_handle(), **CBF_CONSTS)
    _ok(rc, "cbf_bwd")
    return nb


def _rev_csr_kw(idx, rptr, redges, n_nodes=None):
    """rev_csr's checks -> the CsrArgs fields (csrc/args.h) as a dict."""
    Gn, N, K = idx.shape
    Nn = N if n_nodes is None else int(n_nodes)
    check(idx, torch.int32, (Gn, N, K), "idx")
    check(rptr, torch.int32, (Gn, Nn + 1), "rptr")
    check(redges, torch.int32, (Gn, N * K), "redges")
    ws = None
    if (2 * Nn + 1) * 4 > 150 * 1024:         # counters beyond LDS: csrc/graph.hip global path
        ws = _workspace("csr", Gn * Nn * 4, idx.device)
    return dict(idx=ptr(idx), G=Gn, N=N, K=K, ptr=ptr(rptr), edges=ptr(redges), Nn=Nn, ws=ptr(ws))


def rev_csr(idx, rptr, redges, n_nodes=None):
    """idx (G, N, K) int32 contiguous -> rptr (G, Nn+1), redges (G, N*K); Nn = n_nodes (agents +
    obstacle points, default N)."""
    _ok(lib().rev_csr(stream=stream_handle(), **_rev_csr_kw(idx, rptr, redges, n_nodes)), "rev_csr")


def node_reduce(dE, rptr, redges, out, *, T, B, N, K, passes=2, accumulate=False, pass_mask=0, shift1=0,
                n_nodes=None, map1=None, gate=None, t_range=None):
    """dE (passes, T, B, N, K, W) -> out[t'] (+)= sum over passes p of the edge->node reduction of
    step t' - p, for the N agents. pass_mask selects passes (0 = all); shift1=1: pass-1 edges live
    in graph t+1 (h' on the recomputed kNN of s_{t+1}), so the CSR arrays must hold T+1 graphs.
    map1 (T, B, N, K): deduplicated evaluations (cbf_match) -- dE is then indexed by evaluation
    and pass 1 reads only the extras map1[e] >= E. t_range=(lo, hi): only output steps
    lo <= t' < hi (the BPTT consumes dS from the last step down: the early steps can be reduced
    on a side stream while it runs)."""
    Nn = N if n_nodes is None else int(n_nodes)
    W = dE.shape[-1]
    D = 2 if W == 4 else 3
    check(dE, torch.float32, (passes, T, B, N, K, W), "dE")
    check(rptr, torch.int32, None, "rptr")
    check(redges, torch.int32, None, "redges")
    if rptr.shape[0] < (T + shift1) * B or redges.shape[0] < (T + shift1) * B or rptr.shape[1] != Nn + 1:
        raise NativeError("reverse CSR too small")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.shape[0] < T + 1 or \
            tuple(out.shape[1:]) != (B, N, W):
        raise NativeError(f"out must be float32 (>=T+1, B, N, {W})")
    if map1 is not None:
        check(map1, torch.int32, (T, B, N, K), "map1")
        if passes != 2:
            raise NativeError("map1 needs passes=2")
    if gate is not None:
        check(gate, torch.float32, (passes * T * B * N * K,), "gate")
    lo, hi = (0, 0) if t_range is None else (int(t_range[0]), int(t_range[1]))
    if t_range is not None and not (0 <= lo < hi <= T + 1):
        raise NativeError(f"t_range must satisfy 0 <= lo < hi <= T+1 (got {t_range}, T={T})")
    _ok(lib().node_reduce(dE=ptr(dE), ptr=ptr(rptr), edges=ptr(redges), B=B, T=T, N=N, K=K, passes=passes,
                          accumulate=int(accumulate), out=ptr(out), pass_mask=int(pass_mask), shift1=int(shift1), Nn=Nn,
                          dim=D, map1=ptr(map1), gate=ptr(gate), t_lo=int(lo), t_hi=int(hi), stream=stream_handle()),
        "node_reduce")


def node_combine(dS_t, ego, dEc, rptr_t, redges_t, Gn, Gout, *, K, dt=C.TIME_STEP):
    """All (B,N,W) record views; dEc (B,N,K,W); rptr_t (B, Nn+1) / redges_t (B, N*K) of graph t."""
    B, N, W = dS_t.shape
    D = 2 if W == 4 else 3
    _records(dS_t, "dS_t", (B, N), W)
    _records(Gout, "Gout", (B, N), W)
    _records(Gn, "Gn", (B, N), W)
    check(ego, torch.float32, (B, N, W), "ego")
    check(dEc, torch.float32, (B, N, K, W), "dEc")
    if dEc is not None:
        if rptr_t.dtype != torch.int32 or rptr_t.shape[0] != B or rptr_t.shape[1] < N + 1 or rptr_t.stride(1) != 1:
            raise NativeError("rptr_t must be int32 (B, Nn+1)")
        if redges_t.dtype != torch.int32 or tuple(redges_t.shape) != (B, N * K) or redges_t.stride(1) != 1:
            raise NativeError("redges_t must be int32 (B, N*K)")
    _ok(lib().node_combine(dS=ptr(dS_t), ds_env=dS_t.stride(0) // W, ego=ptr(ego), dEc=ptr(dEc),
                           ptr=ptr(rptr_t), ptr_env=rptr_t.stride(0) if dEc is not None else 0,
                           edges=ptr(redges_t), edges_env=redges_t.stride(0) if dEc is not None else 0,
                           Gn=ptr(Gn), gn_env=Gn.stride(0) // W if Gn is not None else 0, Gout=ptr(Gout),
                           go_env=Gout.stride(0) // W, B=B, N=N, K=K, dt=float(dt), dim=D, stream=stream_handle()),
        "node_combine")


# ----------------------------------------------------------------------------- safety filter
FX_VIOL = 2.0 ** 32           # csrc/args.h: fixed-point scale of the violation sums


def refine_grid(E: int, device, prec_code: int) -> int:
    """Workgroups of refine_grad over E edges: one per CU (csrc/refine.hip REFINE_NW waves each,
    a 32-edge tile per wave per trip)."""
    waves = 4 if prec_code == 2 else 8
    tiles = (E + 31) // 32
    return max(1, min((tiles + waves - 1) // waves, num_cu(device)))


def _a_max(a_max) -> float:
    """The actuator limit as the kernels take it: 0.0 is off."""
    if a_max is None:
        return 0.0
    a_max = float(a_max)
    if not (0.0 < a_max < float("inf")):
        raise NativeError(f"a_max must be a positive finite number or None, got {a_max!r}")
    return a_max


def _refine_args(S, idx, a, delta, h, wpack, f_bwd, wrm, wvec, rptr, redges, loops, prec, hn_out, flag_out,
                 env_active, lr, a_max=None, local=False):
    """The argument validation shared by ``refine``, ``refine_small`` and ``refine_local`` ->
    (B, N, Nn, K, D, loops, precision code, the RefineArgs fields of ``_refine_kw``). ``local``: the
    decentralised filter, which has no reverse CSR (rptr / redges must be None)."""
    if S is None or S.dim() != 3:
        raise NativeError("S must be (B, Nn, 4|8) node records")
    B, Nn, W = S.shape
    D = dim_of(S)
    check(S, torch.float32, (B, Nn, W), "S")
    if idx is None or idx.dim() != 3 or idx.shape[0] != B:
        raise NativeError(f"idx must be int32 (B={B}, N, K)")
    _, N, K = idx.shape
    check(idx, torch.int32, (B, N, K), "idx")
    if K < 1 or K > C.MAX_TOP_K:
        raise NativeError(f"K = {K} outside 1..{C.MAX_TOP_K}")
    if N < 1 or N > Nn:
        raise NativeError(f"idx has N = {N} agents but S holds {Nn} nodes")
    for t, name in ((a, "a"), (delta, "delta")):
        if t is None:
            raise NativeError(f"{name} is required")
        check(t, torch.float32, (B, N, D), name)
    if h is None:
        raise NativeError("h is required")
    check(h, torch.float32, (B, N, K), "h")
    if local:
        if rptr is not None or redges is not None:
            raise NativeError("the decentralised filter takes no reverse CSR (rptr / redges)")
    else:
        if rptr is None or redges is None:
            raise NativeError("h, rptr and redges are required")
        check(rptr, torch.int32, (B, Nn + 1), "rptr")
        check(redges, torch.int32, (B, N * K), "redges")
    loops = int(loops)
    if loops < 0:
        raise NativeError("loops must be >= 0")
    code = _half(wpack, "wpack", prec)
    if code == 1:
        raise NativeError("safety filter: fp16 is not supported (the -1 upstream gradient has no loss scaling); "
                          "use fp32 or bf16")
    check(wpack, wpack.dtype, None, "wpack")
    check(wvec, torch.float32, None, "wvec")
    if wvec is None or wvec.numel() < 260:
        raise NativeError("CBF side vector too small")
    if f_bwd < 0 or wpack.numel() < (f_bwd + 70) * 512 * _planes(code):
        raise NativeError("packed CBF weights too small")
    check(wrm, wpack.dtype, (_planes(code) * (128 * 68 + 64 * 148),), "wrm")
    check(hn_out, torch.float32, (B, N, K), "hn_out")
    check(flag_out, torch.uint8, (B, N, K), "flag_out")
    if env_active is not None:
        if not isinstance(env_active, torch.Tensor) or env_active.dtype not in (torch.bool, torch.uint8):
            raise NativeError("env_active must be a bool or uint8 tensor")
        check(env_active, env_active.dtype, (B,), "env_active")
        if env_active.dtype == torch.bool:
            env_active = env_active.view(torch.uint8)         # same bytes, 0 / 1
    extra = dict(local=1) if local else {}
    return B, N, Nn, K, D, loops, code, _refine_kw(B, N, Nn, K, D, S, idx, a, delta, h, wpack, f_bwd, wrm, wvec, rptr,
                                                   redges, lr, hn_out, flag_out, env_active, a_max=a_max, **extra)


def _refine_kw(B, N, Nn, K, D, S, idx, a, delta, h, wpack, f_bwd, wrm, wvec, rptr, redges, lr, hn_out=None,
               flag_out=None, env_active=None, a_max=None, **loop):
    """The RefineArgs fields (csrc/args.h) both filters take; `loop`: what the caller adds (dEv, ctl, launch
    parameters, local=1 for the decentralised filter). The actuator limit is an optional key of the native
    layer: passed only when one is set."""
    if _a_max(a_max) > 0.0:
        loop["a_max"] = _a_max(a_max)
    return dict(S=ptr(S), s_env=Nn, dim=D, idx=ptr(idx), a=ptr(a), delta=ptr(delta), h=ptr(h), B=B, N=N, Nn=Nn, K=K,
                wpack=ptr(wpack), f_bwd=int(f_bwd), wrm=ptr(wrm), wvec=ptr(wvec), ptr=ptr(rptr), edges=ptr(redges),
                dt=float(C.TIME_STEP), dt_alpha=float(C.TIME_STEP * C.ALPHA_CBF), lr=float(lr), hn_out=ptr(hn_out),
                flag_out=ptr(flag_out), env_active=ptr(env_active), dist_eps=float(C.CBF_DIST_EPS_COORD * D), **CBF_CONSTS,
                **loop)


def refine(S, idx, a, delta, h, wpack, f_bwd, wrm, wvec, dEv, rptr, redges, ctl, *, loops, lr,
           prec=None, hn_out=None, flag_out=None, num_blocks=None, env_active=None, a_max=None, local=False):
    """The safety-filter loop (csrc/refine.hip + the driver in csrc/runtime.cpp): ``loops`` gradient
    steps of ``delta`` (B, N, D), in place, on sum_e relu(-(h(s') - h + dt alpha h)) with
    s' = s + dt [v, a + delta].

    S (B, Nn, 4|8) node records of s_t (agents first); idx (B, N, K) int32 into the Nn nodes;
    a / delta (B, N, D) fp32 contiguous; h (B, N, K) the radius-masked h(s_t); wpack / wrm / wvec the
    packed CBF weights (``module_pack``); dEv (B, N, K, D) workspace; rptr (B, Nn+1) / redges
    (B, N*K) the reverse CSR of idx (``rev_csr``); ctl int64, >= 2*loops words, cleared by the
    driver: ctl[2 it] = edges with a non-zero hinge gradient in iteration it, ctl[2 it + 1] = the
    violation sum of iteration it times FX_VIOL. hn_out (B, N, K) fp32 / flag_out (B, N, K) uint8
    (optional): h(s') and the hinge flags of the first iteration. env_active (B,) bool / uint8 on the
    device (optional): envs with 0 are left out -- their delta stays zero, they write no dEv / trace
    and ctl counts the other envs alone; None is every env. The mask is read by the kernels only.
    a_max (optional): the per-axis actuator limit -- ``a`` must already be clamped to [-a_max, a_max];
    every update then projects delta onto [-a_max - a, a_max - a]. No host synchronisation.
    local=True: the decentralised filter's loop path (refine_grad_local_kernel, refine_update_local_kernel;
    ``evaluate.py``'s module docstring) -- rptr and redges must be None.
    fp32 (x3) and bf16 builds; fp16 is not supported (the -1 upstream gradient has no loss scaling)."""
    if dEv is None or ctl is None:
        raise NativeError("dEv and ctl are required")
    B, N, Nn, K, D, loops, code, kw = _refine_args(S, idx, a, delta, h, wpack, f_bwd, wrm, wvec, rptr, redges, loops, prec,
                                                   hn_out, flag_out, env_active, lr, a_max, local=local)
    check(dEv, torch.float32, (B, N, K, D), "dEv")
    check(ctl, torch.int64, None, "ctl")
    if ctl.dim() != 1 or ctl.numel() < 2 * loops:
        raise NativeError(f"ctl must be int64 with at least 2*loops = {2 * loops} words, got {tuple(ctl.shape)}")
    E = B * N * K
    if E >= 2 ** 31 - 2 ** 21:
        raise NativeError("too many edges for 32-bit indexing")
    nb = int(num_blocks) if num_blocks else refine_grid(E, S.device, code)
    if nb < 1 or nb > 4096:
        raise NativeError("num_blocks outside 1..4096")
    _ok(lib().refine_loop(loops=loops, num_blocks=nb, prec=code, stream=stream_handle(), dEv=ptr(dEv), ctl=ptr(ctl), **kw),
        "refine")
    return nb


def refine_local_grid(BN: int, device, prec_code: int) -> int:
    """Workgroups of refine_local over BN agents: a tile is 2 agents x 16 slots and runs its whole loop in
    one wave (csrc/refine.hip REFINE_NW waves per workgroup). One workgroup per REFINE_NW tiles, capped at
    4 * CUs: beyond that a wave walks several tiles (grid stride). The LDS footprint lets 3 (bf16) or 1
    (fp32) workgroups reside per CU, so the rest of the grid queues behind them and is handed out as
    tiles stop early; the factor 4 is an unmeasured tuning constant, not a residency figure."""
    waves = 4 if prec_code == 2 else 8
    tiles = (BN + 1) // 2
    return max(1, min((tiles + waves - 1) // waves, 4 * num_cu(device)))


def refine_local(S, idx, a, delta, h, wpack, f_bwd, wrm, wvec, ctl, *, loops, lr,
                 prec=None, hn_out=None, flag_out=None, num_blocks=None, env_active=None, a_max=None):
    """The decentralised safety filter (csrc/refine.hip refine_local_kernel, ``evaluate.py``'s module
    docstring): every agent refines its own action against its neighbours' nominal next states, the whole
    loop in ONE launch for any scene. Arguments as for ``refine`` without dEv and the reverse CSR; delta
    (B, N, D) must be ZERO on entry; ctl int64, >= 2*loops words, cleared by the driver, holds the loop
    path's control words afterwards (ctl[2 it] exactly; ctl[2 it + 1] is the violation sum of iteration it
    for every it, also after the stop). Bit for bit the results of ``refine(..., local=True)``. Returns the
    workgroup count. No host synchronisation. fp32 (x3) and bf16 builds; fp16 is not supported."""
    # what needs no device first: the precision, the loop count
    if _half(wpack, "wpack", prec) == 1:
        raise NativeError("safety filter: fp16 is not supported (the -1 upstream gradient has no loss scaling); "
                          "use fp32 or bf16")
    if int(loops) < 0:
        raise NativeError("loops must be >= 0")
    if ctl is None:
        raise NativeError("ctl is required")
    B, N, Nn, K, D, loops, code, kw = _refine_args(S, idx, a, delta, h, wpack, f_bwd, wrm, wvec, None, None, loops, prec,
                                                   hn_out, flag_out, env_active, lr, a_max, local=True)
    check(ctl, torch.int64, None, "ctl")
    if ctl.dim() != 1 or ctl.numel() < 2 * loops:
        raise NativeError(f"ctl must be int64 with at least 2*loops = {2 * loops} words, got {tuple(ctl.shape)}")
    if B * N * 16 >= 2 ** 31 - 2 ** 21:
        raise NativeError("too many agents for 32-bit indexing")
    nb = int(num_blocks) if num_blocks else refine_local_grid(B * N, S.device, code)
    if nb < 1 or nb > 4096:
        raise NativeError("num_blocks outside 1..4096")
    _ok(lib().refine_local(loops=loops, fused=1, fused_blocks=nb, prec=code, stream=stream_handle(), ctl=ptr(ctl), **kw),
        "refine_local")
    return nb


def refine_small_eligible(Nn: int, K: int) -> bool:
    """Envs the persistent filter takes: at most SMALL_MAXN graph nodes (agents + obstacle points)
    and K <= 16, so at most 32 tiles of 32 edges per env."""
    return 1 <= Nn <= SMALL_MAXN and 1 <= K <= C.MAX_TOP_K


def refine_small(S, idx, a, delta, h, wpack, f_bwd, wrm, wvec, rptr, redges, ew, *, loops, lr,
                 prec=None, hn_out=None, flag_out=None, env_active=None, a_max=None):
    """The persistent safety filter of small envs (csrc/refine.hip refine_small_kernel): the whole
    loop of ``refine`` in ONE launch, one workgroup per env, for envs of at most SMALL_MAXN graph
    nodes. Arguments as for ``refine`` (no dEv: it lives in LDS), except the result words: ew
    (B, loops, 2) int64, ZERO on entry (as is delta), ew[b, it, 0] = env b's edges with a non-zero
    hinge gradient in iteration it, ew[b, it, 1] = its violation sum times FX_VIOL. An env stops at
    its first iteration u without an active edge: its later counts stay zero and its later violation
    words repeat the one of u (the iterate no longer changes). Envs with env_active 0 write nothing.
    ``refine_reduce`` turns ew into the loop path's ``used`` / ``viol`` / ``counts``. No host
    synchronisation. fp32 (x3) and bf16 builds; fp16 is not supported."""
    # what needs no device first: the size limit, the precision, the loop count
    if S is None or S.dim() != 3:
        raise NativeError("S must be (B, Nn, 4|8) node records")
    if S.shape[1] > SMALL_MAXN:
        raise NativeError(f"the persistent filter takes envs of at most SMALL_MAXN = {SMALL_MAXN} graph nodes, "
                          f"got {S.shape[1]}")
    if _half(wpack, "wpack", prec) == 1:
        raise NativeError("safety filter: fp16 is not supported (the -1 upstream gradient has no loss scaling); "
                          "use fp32 or bf16")
    if int(loops) < 0:
        raise NativeError("loops must be >= 0")
    if ew is None:
        raise NativeError("ew is required")
    B, N, Nn, K, D, loops, code, kw = _refine_args(S, idx, a, delta, h, wpack, f_bwd, wrm, wvec, rptr, redges, loops, prec,
                                                   hn_out, flag_out, env_active, lr, a_max)
    check(ew, torch.int64, (B, loops, 2), "ew")
    _ok(lib().refine_small(ew=ptr(ew), loops=loops, prec=code, stream=stream_handle(), **kw), "refine_small")


def refine_reduce(ew):
    """ew (B, loops, 2) int64 per-env result words of ``refine_small`` -> (used, viol, counts) as the
    loop path's control words give them, with tensor ops alone (nothing is read on the host):
    counts[it] = sum_b ew[b, it, 0]; used = max_b #{it: ew[b, it, 0] != 0} -- the batch runs as long
    as its slowest env; viol = sum_b ew[b, min(used, loops - 1), 1] / FX_VIOL, where an env that
    stopped earlier contributes the (unchanged) violation of its stopping iteration. Integer sums:
    exactly the loop path's values. loops = 0: (0, 0.0, empty)."""
    if ew.dim() != 3 or ew.shape[-1] != 2 or ew.dtype != torch.int64:
        raise NativeError("ew must be int64 (B, loops, 2)")
    B, loops, _ = ew.shape
    counts = ew[:, :, 0].sum(0)
    if loops == 0 or B == 0:
        return (torch.zeros((), dtype=torch.int64, device=ew.device),
                torch.zeros((), dtype=torch.float64, device=ew.device), counts)
    used = (ew[:, :, 0] != 0).sum(1).max()
    last = torch.clamp(used, max=loops - 1).view(1)
    viol = ew[:, :, 1].index_select(1, last).sum().double() / FX_VIOL
    return used, viol, counts


CTRL_EDGE_WAVES = 4          # csrc/ctrl.hip EB_WAVES


def ctrl_edge_qsplit(total_agents: int, device) -> int:
    """Workgroups per 128-agent chunk of the edge backward: small scenes split a chunk's tile
    rounds (K of them with the dense edge rows, csrc/ctrl.hip) over up to 16 workgroups (the tiles
    are independent; a single wave would otherwise run all of them back to back; a part with no
    tile writes a zero slab row); 1 once the chunks alone fill the GPU."""
    che = (total_agents + 32 * CTRL_EDGE_WAVES - 1) // (32 * CTRL_EDGE_WAVES)
    cap = (8 // CTRL_EDGE_WAVES) * num_cu(device)
    p = 1
    while p < 16 and che * p * 2 <= cap:
        p *= 2
    return p


def node_bwd_chunk(total_agents: int, device) -> int:
    """Agents per node-backward workgroup chunk: 128 while the chunks fill half the CUs, else 64
    while they fill the CUs, else 32 (small scenes and strong-scaling slices: more, shorter
    workgroups; a chunk's empty stage turns are skipped). At 16,384 agents (config #3 per rank at
    DP 4) 128 over 64: 3.815-3.853 vs 3.873-3.888 ms interleaved (profiles/r6_runs/r6ax/, r6ay/).
    MACBF_NODE_CHUNK overrides."""
    env = os.environ.get("MACBF_NODE_CHUNK")
    if env:
        return int(env)
    cu = num_cu(device)
    if (total_agents + 127) // 128 >= cu // 2:
        return 128
    if (total_agents + 63) // 64 >= cu:
        return 64
    return 32


def ctrl_bwd_grids(total_agents: int, device, prec=None, eb16=False):
    """(node, edge) backward grids: the node kernel takes node_bwd_chunk-agent chunks, one
    workgroup per CU; the edge kernel 32*CTRL_EDGE_WAVES-agent chunks x ctrl_edge_qsplit tile
    ranges, at most as many workgroups as fit the CUs at once (4 waves: two per CU in the 16-bit
    builds; one in the fp32 (x3) build -- 322 registers, 118 KB of LDS: a grid of one per CU
    loops over two chunks instead of running a second round of workgroups, 142 -> 137 us per
    call at 1024 x 64, profiles/r2_egrid/); eb16: the 8-wave 16x16x32 kernel (same 128-agent
    chunks, k16_wg_per_cu per CU). MACBF_EDGE_WG_PER_CU overrides the cap."""
    ca = node_bwd_chunk(total_agents, device)
    ch = (total_agents + ca - 1) // ca
    che = (total_agents + 32 * CTRL_EDGE_WAVES - 1) // (32 * CTRL_EDGE_WAVES)
    cu = num_cu(device)
    if bwd_step_fused(total_agents, device):      # one fused launch per step: one grid for both
        n = max(1, min(ch, cu))
        return n, n
    if eb16:
        per_cu = k16_wg_per_cu(prec or "bf16", 1)
    else:
        per_cu = 1 if prec == "fp32" else 8 // CTRL_EDGE_WAVES
    per_cu = int(os.environ.get("MACBF_EDGE_WG_PER_CU", per_cu))
    return max(1, min(ch, cu)), max(1, min(che * ctrl_edge_qsplit(total_agents, device), per_cu * cu))


NODE16_RM = 64 * 176 + 128 * 80 + 64 * 144 + 16 * 80    # csrc/node16.h: elements per plane (layout.node_rm16)


def _node_bwd_kw(pooled, S, G, A, Gn, valid_t, wrm, offs, wvec, act_coef, dP, ego, partial, num_blocks,
                 act_cnt=None, prec=None, init=False, chunk=None, gscale=None, combine=None, stamps=None, wrm16=None,
                 a_max=None, res=False):
    """ctrl_node_bwd's checks -> (the CtrlNodeBwdArgs fields (csrc/args.h) as a dict, precision code).
    a_max (optional): the rollout's actuator limit -- the key is only there with a limit. res: the packed
    controller has the residual head -- the key is only there with it."""
    B, N = G.shape[:2]
    D = dim_of(S)
    W = rec_width(D)
    f16 = _half(wrm, "wrm", prec)
    _rows(pooled, _prow(f16), "pooled", (B, N))
    _records(S, "S", (B, N), W)
    check(G, torch.float32, (B, N, D), "G")
    _rows(A, D, "A", (B, N))
    _records(Gn, "Gn", (B, N), W)
    if valid_t is not None and (valid_t.dtype != torch.uint8 or tuple(valid_t.shape) != (B,)):
        raise NativeError("valid_t must be uint8 (B,)")
    check(wrm, wrm.dtype, None, "wrm")
    if wrm.numel() < _planes(f16) * NODE_RM_ELEMS:
        raise NativeError("node weight images too small")
    check(dP, wrm.dtype, (B, N, _prow(f16)), "dP")
    _same_half(pooled, wrm, "pooled")
    check(ego, torch.float32, (B, N, W), "ego")
    check(partial, torch.float32, (num_blocks, CTRL_NODE_PARTIAL), "partial")
    check(act_cnt, torch.float32, (1,), "act_cnt")
    check(gscale, torch.float32, (1,), "gscale")
    check(stamps, torch.int64, (num_blocks, 8 if wrm16 is not None else 4, 16), "stamps")
    kw = dict(pooled=ptr(pooled), p_env=pooled.stride(0), S=ptr(S), s_env=S.stride(0) // W, G=ptr(G), A=ptr(A),
              a_env=A.stride(0) // D, Gn=ptr(Gn), gn_env=Gn.stride(0) // W if Gn is not None else 0,
              valid=ptr(valid_t), v_env=valid_t.stride(0) if valid_t is not None else 0, B=B, N=N,
              wrm=ptr(wrm), o_w1=offs["w1"], o_w2=offs["w2"], o_w3=offs["w3"], o_w4=offs["w4"], wvec=ptr(wvec),
              act_coef=float(act_coef), act_scale=ptr(act_cnt), dt=float(C.TIME_STEP), sqrt3=float(C.SQRT3), dP=ptr(dP),
              dp_env=dP.stride(0), ego=ptr(ego), partial=ptr(partial), dim=D, init=int(bool(init)),
              chunk=int(chunk or node_bwd_chunk(B * N, S.device)), gscale=ptr(gscale), stamps=ptr(stamps))
    if combine is not None:
        # fused BPTT combine: Gn is formed in the kernel from step t+1's records (node_combine's terms)
        c = combine
        K = int(c["K"])
        _records(c["dS"], "combine dS", (B, N), W)
        check(c["ego"], torch.float32, (B, N, W), "combine ego")
        check(c["dEc"], torch.float32, (B, N, K, W), "combine dEc")
        _rows(c["rptr"], c["rptr"].shape[1], "combine rptr", (B,))
        _rows(c["redges"], N * K, "combine redges", (B,))
        _records(c["Gn"], "combine Gn", (B, N), W)
        _records(c["Gout"], "combine Gout", (B, N), W)
        if c["rptr"].dtype != torch.int32 or c["redges"].dtype != torch.int32 or c["rptr"].shape[1] < N + 1:
            raise NativeError("combine rptr / redges must be int32 CSR rows")
        Gn_c = c["Gn"]
        kw.update(cdS=ptr(c["dS"]), cds_env=c["dS"].stride(0) // W, cego=ptr(c["ego"]), cdEc=ptr(c["dEc"]),
                  cptr=ptr(c["rptr"]), cptr_env=c["rptr"].stride(0), cedges=ptr(c["redges"]),
                  cedges_env=c["redges"].stride(0), cGn=ptr(Gn_c), cgn_env=Gn_c.stride(0) // W if Gn_c is not None else 0,
                  cGout=ptr(c["Gout"]), cgo_env=c["Gout"].stride(0) // W, K=K)
    if wrm16 is not None:
        # 16x16x32 kernel (csrc/node16.h): 128-agent chunks (eight 16-agent waves)
        if kw["chunk"] != 128:
            raise NativeError("16x16x32 node backward: 128-agent chunks only")
        check(wrm16, wrm.dtype, (_planes(f16) * NODE16_RM,), "wrm16")
        kw["wrm16"] = ptr(wrm16)
    if _a_max(a_max) > 0.0:
        kw["a_max"] = _a_max(a_max)
    if res:
        if stamps is not None:
            raise NativeError("ctrl_node_bwd stamps: the residual kernels have no phase clocks")
        kw["res"] = 1
    return kw, f16


def ctrl_node_bwd(pooled, S, G, A, Gn, valid_t, wrm, offs, wvec, act_coef, dP, ego, partial, num_blocks,
                  act_cnt=None, prec=None, init=False, chunk=None, gscale=None, combine=None, stamps=None, wrm16=None,
                  a_max=None, res=False):
    """act_cnt: optional 1-element device tensor holding the (all-reduced) action-loss count
    n_act; the action-loss coefficient is then act_coef / max(n_act, 1), read by the kernel (no
    host round trip, no extra launch). init: write the weight-gradient slabs instead of
    accumulating into them (no zero fill needed). stamps: diagnostics only, int64
    (num_blocks, 4, 16) phase clocks of the cooperative 32-agent path (scripts/stamps_node.py).
    a_max (optional): the rollout's actuator limit -- dL/da through the Euler step is zero where the
    raw action A lies outside [-a_max, a_max] or is NaN (the action-loss term is kept).
    res: the packed controller has the residual head (dL/dy4[2D + q] = da_q)."""
    kw, f16 = _node_bwd_kw(pooled, S, G, A, Gn, valid_t, wrm, offs, wvec, act_coef, dP, ego, partial, num_blocks,
                           act_cnt, prec, init, chunk, gscale, combine, stamps, wrm16, a_max, res)
    _ok(lib().ctrl_node_bwd(num_blocks=int(num_blocks), prec=f16, stream=stream_handle(), **kw), "ctrl_node_bwd")


def _edge_bwd_kw(S, idx, argmax, dP, wpack, f_ew1f, f_ew2tn, dEc, partial, num_blocks, prec=None, init=False,
                 w16=None, stamps=None):
    """ctrl_edge_bwd's checks -> (the CtrlEdgeBwdArgs fields (csrc/args.h) as a dict, precision code)."""
    B, N, K = idx.shape
    D = dim_of(S)
    W = rec_width(D)
    _records(S, "S", (B, N), W)
    if idx.dtype != torch.int32 or idx.stride(2) != 1 or idx.stride(1) != K:
        raise NativeError("idx must be int32 (B,N,K)")
    _rows(argmax, 128, "argmax", (B, N))
    f16 = _half(wpack, "wpack", prec)
    check(dP, wpack.dtype, (B, N, _prow(f16)), "dP")
    if wpack.numel() < (f_ew2tn + 20) * 512 * _planes(f16) or wpack.numel() < (f_ew1f + 2) * 512 * _planes(f16):
        raise NativeError("packed controller weights too small")
    check(dEc, torch.float32, (B, N, K, W), "dEc")
    check(partial, torch.float32, (num_blocks, CTRL_EDGE_PARTIAL), "partial")
    kw = dict(S=ptr(S), s_env=S.stride(0) // W, idx=ptr(idx), i_env=idx.stride(0), argmax=ptr(argmax),
              am_env=argmax.stride(0), dP=ptr(dP), dp_env=dP.stride(0), B=B, N=N, K=K, wpack=ptr(wpack),
              f_ew1f=int(f_ew1f), f_ew2tn=int(f_ew2tn), dEc=ptr(dEc), de_env=dEc.stride(0) // W if dEc is not None else 0,
              partial=ptr(partial), dim=D, qsplit=ctrl_edge_qsplit(B * N, S.device), init=int(bool(init)))
    if w16 is not None:
        if K != 12:
            raise NativeError("16x16x32 edge backward: K = 12 only")
        check(w16, wpack.dtype, (22 * 512 * _planes(f16),), "w16")
        kw["w16"] = ptr(w16)
    if stamps is not None:
        if w16 is None:
            raise NativeError("edge backward stamps: 16x16x32 kernel only")
        check(stamps, torch.int64, (num_blocks, 8, 16), "stamps")
        kw["stamps"] = ptr(stamps)
    return kw, f16


def ctrl_edge_bwd(S, idx, argmax, dP, wpack, f_ew1f, f_ew2tn, dEc, partial, num_blocks, prec=None, init=False,
                  w16=None, stamps=None):
    """w16 (K = 12): the 16x16x32 fragments (layout.ctrl_edge_packer16) -> the 8-wave 16x16x32 kernel
    (csrc/ctrl16.h); same slabs, same dEc records. stamps (num_blocks, 8, 16) int64 (diagnostics,
    16x16x32 kernel): per wave the shader-clock cycles of each loop phase summed over its tiles
    (slot 15: tiles), scripts/stamps_edge16.py."""
    kw, f16 = _edge_bwd_kw(S, idx, argmax, dP, wpack, f_ew1f, f_ew2tn, dEc, partial, num_blocks, prec, init, w16, stamps)
    _ok(lib().ctrl_edge_bwd(num_blocks=int(num_blocks), prec=f16, stream=stream_handle(), **kw), "ctrl_edge_bwd")


def ctrl_bwd_step(node: dict, edge: dict, num_blocks: int):
    """One fused BPTT step (csrc/ctrl.hip ctrl_bwd_step_kernel): the node backward of each
    workgroup's 32-agent chunks, then the edge backward of the same agents, in one launch.
    `node` / `edge` are the keyword arguments of ctrl_node_bwd / ctrl_edge_bwd (validated the same
    way); both run on num_blocks workgroups (their slabs need num_blocks rows each)."""
    if node.get("wrm16") is not None or edge.get("w16") is not None or edge.get("stamps") is not None:
        raise NativeError("ctrl_bwd_step: the fused kernel takes no 16x16x32 images and no edge stamps")
    na, prec = _node_bwd_kw(**node, num_blocks=num_blocks, chunk=32)
    ea, _ = _edge_bwd_kw(**edge, num_blocks=num_blocks)
    _ok(lib().ctrl_bwd_step(node=na, edge=ea, num_blocks=int(num_blocks), prec=prec, stream=stream_handle()),
        "ctrl_bwd_step")


BWD_FUSED_DEFAULT = True


def bwd_step_fused(total_agents: int, device) -> bool:
    """Whether the BPTT runs as fused node+edge launches (ctrl_bwd_step): in the cooperative regime
    (32-agent node chunks) with at least half a chunk per CU -- strong-scaling slices. Small scenes
    keep the separate launches: their edge backward splits a chunk over up to 16 workgroups
    (qsplit), which one fused workgroup cannot. MACBF_BWD_FUSED=0/1 forces the choice."""
    env = os.environ.get("MACBF_BWD_FUSED")
    if env is not None:
        return env == "1" and node_bwd_chunk(total_agents, device) == 32
    return BWD_FUSED_DEFAULT and node_bwd_chunk(total_agents, device) == 32 and (total_agents + 31) // 32 >= num_cu(device) // 2


def reduce_multi(jobs):
    """Several reduce_rows in ONE launch: jobs = [(partial (rows, cols), out (cols,), accumulate)]
    (at most 4; the same fixed-order sums as reduce_rows)."""
    if not 1 <= len(jobs) <= 4:
        raise NativeError("reduce_multi takes 1..4 jobs")
    _ok(lib().reduce_multi(jobs=[_reduce_job(*j) for j in jobs], stream=stream_handle()), "reduce_multi")


def _reduce_job(partial, out, accumulate):
    rows, cols = partial.shape
    check(partial, torch.float32, None, "partial")
    check(out, torch.float32, (cols,), "out")
    if cols % 4:
        raise NativeError("cols must be a multiple of 4")
    return ptr(partial), rows, cols, ptr(out), int(bool(accumulate))


def reduce_rows(partial, out, accumulate=False):
    p, rows, cols, o, acc = _reduce_job(partial, out, accumulate)
    _ok(lib().reduce_rows(partial=p, rows=rows, cols=cols, out=o, accumulate=acc, stream=stream_handle()), "reduce_rows")


FX_DIST = 2.0 ** 32           # csrc/args.h: fixed-point scales of the per-env rollout sums
FX_ACT = 2.0 ** 24


def rollout_stats(dist, cnt, safe, act, valid, counts, local, *, N, reset=None):
    """dist/act (T,B), cnt (T,B,2), safe (T+1,B) or None -> valid (T,B) u8, counts[:3] =
    [n_dang, n_safe, n_act] of this rank, local[:3] = [agent-steps, safe agents of s_{t+1},
    action-loss sum]. One launch, deterministic. reset = (dist, cnt, safe, act) full (Tmax, ...)
    buffers whose leading views are the inputs: zeroed after they are read, so the next
    rollout's atomics start from zero without fill kernels."""
    T, B = dist.shape
    reset_T = 0
    if reset is not None:
        zd, zc, zs, za = reset
        reset_T = zd.shape[0]
        check(zd, torch.int64, (reset_T, B), "reset dist")
        check(zc, torch.float32, (reset_T, B, 2), "reset cnt")
        check(zs, torch.float32, (reset_T + 1, B), "reset safe")
        check(za, torch.int64, (reset_T, B), "reset act")
        if (ptr(zd), ptr(zc), ptr(zs), ptr(za)) != (ptr(dist), ptr(cnt), ptr(safe), ptr(act)) or T > reset_T:
            raise NativeError("reset buffers must start at the inputs")
    check(dist, torch.int64, (T, B), "dist")
    check(cnt, torch.float32, (T, B, 2), "cnt")
    check(safe, torch.float32, (T + 1, B), "safe")
    check(act, torch.int64, (T, B), "act")
    check(valid, torch.uint8, (T, B), "valid")
    check(counts, torch.float32, None, "counts")
    check(local, torch.float32, None, "local")
    if counts.numel() < 3 or local.numel() < 3:
        raise NativeError("counts / local need 3 slots")
    _ok(lib().rollout_stats(dist=ptr(dist), cnt=ptr(cnt), safe=ptr(safe), act=ptr(act), T=T, B=B, N=int(N),
                            thr=float(C.DIST_MIN_CHECK), valid=ptr(valid), counts=ptr(counts), local=ptr(local),
                            reset_T=int(reset_T), stream=stream_handle()), "rollout_stats")


def adam_multi(param, grad, m, v, groups, lr, b1, b2, eps, wd, ok=None):
    """Fused Adam over several ranges in ONE launch: groups = [(lo, hi, step_dev)] (at most 4; each
    step_dev a 1-element device int32 counter, step = *step_dev + 1); ok as in adam."""
    for t, n in ((param, "param"), (grad, "grad"), (m, "m"), (v, "v")):
        check(t, torch.float32, (param.numel(),), n)
    check(ok, torch.int32, None, "ok")
    if not 1 <= len(groups) <= 4:
        raise NativeError("adam_multi takes 1..4 groups")
    spec = []
    for lo, hi, sd in groups:
        if not (0 <= lo <= hi <= param.numel()):
            raise NativeError("bad Adam range")
        check(sd, torch.int32, (1,), "step_dev")
        spec.append((int(lo), int(hi), ptr(sd)))
    _ok(lib().adam_multi(groups=spec, param=ptr(param), grad=ptr(grad), m=ptr(m), v=ptr(v), b1=float(b1), b2=float(b2),
                         eps=float(eps), wd=float(wd), ok=ptr(ok), lr=float(lr), stream=stream_handle()), "adam_multi")


def adam(param, grad, m, v, lo, hi, lr, b1, b2, eps, wd, step, ok=None, step_dev=None):
    """Fused Adam over param[lo:hi]. step: host step count (bias corrections), or step_dev: a
    1-element device int32 counter (step = *step_dev + 1, read by the kernel); ok: optional
    device int32 guard flag (0 -> the kernel leaves everything untouched)."""
    for t, n in ((param, "param"), (grad, "grad"), (m, "m"), (v, "v")):
        check(t, torch.float32, (param.numel(),), n)
    if not (0 <= lo <= hi <= param.numel()):
        raise NativeError("bad Adam range")
    check(ok, torch.int32, None, "ok")
    check(step_dev, torch.int32, None, "step_dev")
    bc1 = 1.0 - b1 ** max(step, 1)
    bc2 = 1.0 - b2 ** max(step, 1)
    _ok(lib().adam(param=ptr(param), grad=ptr(grad), m=ptr(m), v=ptr(v), lo=int(lo), hi=int(hi), b1=float(b1),
                   b2=float(b2), eps=float(eps), wd=float(wd), step_size=float(lr / bc1), bc2_sqrt=float(bc2 ** 0.5),
                   ok=ptr(ok), step=ptr(step_dev), lr=float(lr), stream=stream_handle()), "adam")


def pack_gather(src, idx16, out16, idx32, out32, commit=None):
    """out16[i] = h16(src'[idx16[i]]), out32[j] = src'[idx32[j]] with src' = [src, 0, 1]: all
    packed weight buffers of both networks in one launch. commit: step_commit_args(...) of the
    optimizer step just enqueued -- its commit then runs in this launch (one launch fewer)."""
    check(src, torch.float32, None, "src")
    check(idx16, torch.int32, None, "idx16")
    check(idx32, torch.int32, None, "idx32")
    check(out32, torch.float32, (idx32.numel(),), "out32")
    if out16.dtype not in HALF_DTYPES or not out16.is_contiguous() or out16.numel() != idx16.numel():
        raise NativeError("out16 must be a contiguous bf16/fp16 buffer matching idx16")
    n = src.numel()    # index range (<= n + 1) is validated once by ops.weights.PackedWeights
    _ok(lib().pack_gather(src=ptr(src), n=n, idx16=ptr(idx16), m16=idx16.numel(), out16=ptr(out16),
                          f16=int(out16.dtype == torch.float16), idx32=ptr(idx32), m32=idx32.numel(), out32=ptr(out32),
                          commit=commit, stream=stream_handle()), "pack_gather")


def grad_assemble(red, ptr_, src, grad, scale=1.0, gscale=None, ok=None, stats=None):
    """grad[p] = scale * sum(red[src[ptr[p]:ptr[p+1]]]) (/ *gscale: the device loss scale) for
    every flat parameter p (one launch, fixed order). ptr (n+1,) / src int32 from a host-built CSR
    (validated by the caller). In the same launch (single-process runs): ok (int32 flag) <- 0 if an
    assembled element is not finite (grad_check's test); stats = (sums, counts, local, row): the
    iteration's statistics row (stats_pack's work)."""
    n = grad.numel()
    check(red, torch.float32, None, "red")
    check(ptr_, torch.int32, (n + 1,), "ptr")
    check(src, torch.int32, None, "src")
    check(grad, torch.float32, None, "grad")
    check(gscale, torch.float32, (1,), "gscale")
    check(ok, torch.int32, (1,), "ok")
    sums = counts = local = row = None
    if stats is not None:
        sums, counts, local, row = stats
        _stats_args(sums, counts, local, row)
    _ok(lib().grad_assemble(red=ptr(red), ptr=ptr(ptr_), src=ptr(src), n=n, scale=float(scale), gscale=ptr(gscale),
                            grad=ptr(grad), ok=ptr(ok), sums=ptr(sums), counts=ptr(counts), local=ptr(local), row=ptr(row),
                            stream=stream_handle()), "grad_assemble")


def _stats_args(sums, counts, local, row):
    check(sums, torch.float32, None, "sums")
    check(counts, torch.float32, None, "counts")
    check(local, torch.float32, None, "local")
    if sums.numel() < 10 or counts.numel() < 3 or local.numel() < 3:
        raise NativeError("stats_pack needs 10 sums, 3 counts, 3 local values")
    if row.dtype != torch.float32 or row.numel() < 18 or not row.is_contiguous():
        raise NativeError("row must be a contiguous float32 row of >= 18")


def grad_check(g, ok):
    """ok (int32, 1 between steps: step_commit resets it) <- 0 if any element of g is not finite.
    No host sync."""
    check(g, torch.float32, None, "g")
    check(ok, torch.int32, None, "ok")
    _ok(lib().grad_check(g=ptr(g), n=g.numel(), ok=ptr(ok), stream=stream_handle()), "grad_check")


def _check_stats_src(stats_src, stats_row):
    if stats_src is None:
        return
    if stats_row is None:
        raise NativeError("stats_src needs stats_row")
    if stats_src.dtype != torch.float32 or stats_src.numel() < 16 or not stats_src.is_contiguous():
        raise NativeError("stats_src must be a contiguous float32 row of >= 16")


def step_commit_args(ok, steps, mask, skipped, *, gscale=None, good=None, growth=1000, max_scale=2.0 ** 24,
                     stats_row=None, stats_src=None):
    """Validated step_commit arguments as the dict pack_gather(commit=...) takes; stats_src: the
    commit first copies stats_row[0:16] from it (the graph-replayed backward's fixed row)."""
    check(ok, torch.int32, (1,), "ok")
    check(steps, torch.int32, None, "steps")
    check(skipped, torch.int32, (1,), "skipped")
    check(gscale, torch.float32, (1,), "gscale")
    check(good, torch.int32, (1,), "good")
    if (gscale is None) != (good is None):
        raise NativeError("gscale and good go together")
    if stats_row is not None and (stats_row.dtype != torch.float32 or stats_row.numel() < 18
                                  or not stats_row.is_contiguous()):
        raise NativeError("stats_row must be a contiguous float32 row of >= 18")
    _check_stats_src(stats_src, stats_row)
    return dict(ok=ptr(ok), steps=ptr(steps), mask=int(mask), ngroups=steps.numel(), skipped=ptr(skipped),
                gscale=ptr(gscale), good=ptr(good), growth=int(growth), max_scale=float(max_scale),
                stats_row=ptr(stats_row), stats_src=ptr(stats_src))


def step_commit_raw(args):
    """step_commit from a step_commit_args dict (its own launch)."""
    _ok(lib().step_commit(**args, stream=stream_handle()), "step_commit")


def step_commit(ok, steps, mask, skipped, *, gscale=None, good=None, growth=1000, max_scale=2.0 ** 24,
                stats_row=None, stats_src=None):
    """End of an optimizer step on the device: steps[g] += 1 for the groups in mask if *ok, else
    skipped += 1; fp16 (gscale, good): the dynamic loss scale halves on a skipped step and doubles
    after `growth` finite ones; stats_row[16:18] = [skipped, loss scale]; *ok reset to 1."""
    step_commit_raw(step_commit_args(ok, steps, mask, skipped, gscale=gscale, good=good, growth=growth,
                                     max_scale=max_scale, stats_row=stats_row, stats_src=stats_src))


def stats_pack(sums, counts, local, row):
    """row[:18] = [sums (10) | counts (3) | local (3) | 0 | 1] (one launch; utils.metrics.StepStats)."""
    _stats_args(sums, counts, local, row)
    _ok(lib().stats_pack(sums=ptr(sums), counts=ptr(counts), local=ptr(local), row=ptr(row), stream=stream_handle()),
        "stats_pack")


# ----------------------------------------------------------------------------- closed-loop episodes
EP_WORDS = 5                  # csrc/args.h: [alive, safe agent-steps, env steps, steps, filter iterations]
EP_OUT = 8                    # result words, the order of validate.COUNTS
EP_ACT_WORDS = 4              # action-statistic words, the order of evaluate.ACTION_STATS
EP_MODES = {None: 0, "loop": 1, "persistent": 2}
_EPISODE_DRIVER = None


def _ep(t, dtype, shape, name, required=True):
    """Dtype, shape and contiguity of one tensor; the device is checked for all of a call's tensors
    together, last (``_ep_device``), so every other mistake is reported without one."""
    if t is None:
        if required:
            raise NativeError(f"{name} is required")
        return
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise NativeError(f"{name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
    if tuple(t.shape) != tuple(shape):
        raise NativeError(f"{name} shape {tuple(t.shape)} != {tuple(shape)}")
    if not t.is_contiguous():
        raise NativeError(f"{name} must be contiguous")


def _ep_device(**tensors):
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise NativeError(f"{name} must be on the HIP device")


def _episode_state(S_cur, G, st, dist_fx, safe, active, prev_active):
    """The checks shared by the three episode launches -> (B, N, Nn, D, the EpisodeArgs fields (csrc/args.h) of the state)."""
    if S_cur is None or not isinstance(S_cur, torch.Tensor) or S_cur.dim() != 3:
        raise NativeError("S_cur must be (B, Nn, 4|8) node records")
    B, Nn, W = S_cur.shape
    D = dim_of(S_cur)
    if G is None or not isinstance(G, torch.Tensor) or G.dim() != 3 or G.shape[0] != B:
        raise NativeError(f"G must be float32 (B={B}, N, D)")
    N = G.shape[1]
    if N < 1 or N > Nn:
        raise NativeError(f"G has N = {N} agents but the records hold {Nn} nodes")
    if B * N >= 2 ** 31 - 65536:
        raise NativeError("too many agents for 32-bit indexing")
    _ep(S_cur, torch.float32, (B, Nn, W), "S_cur")
    _ep(G, torch.float32, (B, N, D), "G")
    _ep(st, torch.int64, (EP_WORDS,), "st")
    _ep(dist_fx, torch.int64, (B,), "dist_fx")
    _ep(safe, torch.float32, (B,), "safe")
    _ep(active, torch.uint8, (B,), "active")
    _ep(prev_active, torch.uint8, (B,), "prev_active")
    return B, N, Nn, D, dict(s_env=Nn, dim=D, B=B, N=N, A=0, delta=0, G=ptr(G), dt=float(C.TIME_STEP), st=ptr(st),
                             dist_fx=ptr(dist_fx), safe=ptr(safe), active=ptr(active), prev_active=ptr(prev_active),
                             ctl=0, ew=0, loops=0, mode=0, thr=float(C.DIST_MIN_CHECK), out=0)


def _episode_limit_kw(a_max, act_st=None, act_out=None) -> dict:
    """The optional EpisodeArgs keys: passed only when a limit is set / the statistics are asked for."""
    kw = {}
    if _a_max(a_max) > 0.0:
        kw["a_max"] = _a_max(a_max)
    if act_st is not None:
        kw["act_st"] = ptr(act_st)
    if act_out is not None:
        kw["act_out"] = ptr(act_out)
    return kw


def episode_limit(A, a_max):
    """The controller's actions clamped to the actuator box, in place (csrc/episode.hip
    episode_limit_kernel, one thread per component): A (B, N, D) float32 <- clamp(A, -a_max, a_max)."""
    if not isinstance(A, torch.Tensor) or A.dim() != 3 or A.shape[-1] not in (2, 3):
        raise NativeError("A must be float32 (B, N, D) with D = 2 or 3")
    B, N, D = A.shape
    _ep(A, torch.float32, (B, N, D), "A")
    if _a_max(a_max) <= 0.0:
        raise NativeError("episode_limit needs a limit: a_max must be a positive finite number")
    _ep_device(A=A)
    _ok(lib().episode_limit(S_cur=0, S_next=0, s_env=N, dim=D, B=B, N=N, A=ptr(A), delta=0, G=0, dt=0.0, st=0, dist_fx=0,
                            safe=0, active=0, prev_active=0, ctl=0, ew=0, loops=0, mode=0, thr=0.0, out=0,
                            a_max=_a_max(a_max), stream=stream_handle()), "episode_limit")


def episode_advance(S_cur, S_next, A, delta, G, st, dist_fx, safe, active, prev_active, *, a_max=None, act_st=None):
    """One Euler step of every agent (csrc/episode.hip episode_advance_kernel): S_next's agent records
    = s + [v, u] * dt of S_cur's with u = A + delta (unchanged when st[0], the "some env still runs" word,
    is 0), dist_fx[b] += sum_i |p'_i - g_i| * FX_DIST. S_cur / S_next (B, Nn, 4|8) distinct record buffers
    (obstacle rows are not touched); A (B, N, D); delta (B, N, D) or None, zeroed once it is read.
    a_max (optional): u is clamped to [-a_max, a_max]. act_st (EP_ACT_WORDS,) int64 (optional): the
    running action statistics (evaluate.ACTION_STATS) gain this step's, over the agents of the envs
    with active != 0."""
    B, N, Nn, D, kw = _episode_state(S_cur, G, st, dist_fx, safe, active, prev_active)
    _ep(S_next, torch.float32, tuple(S_cur.shape), "S_next")
    _ep(A, torch.float32, (B, N, D), "A")
    _ep(delta, torch.float32, (B, N, D), "delta", required=False)
    _ep(act_st, torch.int64, (EP_ACT_WORDS,), "act_st", required=False)
    if S_next.data_ptr() == S_cur.data_ptr():
        raise NativeError("S_next must not be S_cur")
    _ep_device(S_cur=S_cur, S_next=S_next, A=A, delta=delta, G=G, st=st, dist_fx=dist_fx, safe=safe, active=active,
               prev_active=prev_active, act_st=act_st)
    _ok(lib().episode_advance(S_cur=ptr(S_cur), S_next=ptr(S_next), stream=stream_handle(),
                              **dict(kw, A=ptr(A), delta=ptr(delta)), **_episode_limit_kw(a_max, act_st)),
        "episode_advance")


def _episode_words(B, ctl, ew, loops):
    loops = int(loops)
    if loops < 0:
        raise NativeError("loops must be >= 0")
    if ctl is not None and ew is not None:
        raise NativeError("ctl (loop filter) and ew (persistent filter) exclude each other")
    if ctl is not None:
        if not isinstance(ctl, torch.Tensor) or ctl.dim() != 1 or ctl.numel() < 2 * loops:
            raise NativeError(f"ctl must be int64 with at least 2*loops = {2 * loops} words")
        _ep(ctl, torch.int64, tuple(ctl.shape), "ctl")
        return loops, 1
    if ew is not None:
        _ep(ew, torch.int64, (B, loops, 2), "ew")
        return loops, 2
    return loops, 0


def episode_tally(S_cur, G, st, dist_fx, safe, active, prev_active, *, ctl=None, ew=None, loops=0):
    """The step's bookkeeping (episode_tally_kernel, one workgroup), run after episode_advance:
    st += [safe agents of S_cur of the envs that ran the step before, envs running, alive, the
    filter's iterations], prev_active <- active, active &= dist_fx >= DIST_MIN_CHECK * N, st[0] =
    any(active); dist_fx, safe (and ew) are cleared. ctl: the loop filter's control words; ew
    (B, loops, 2): the persistent filter's; neither: no filter."""
    B, N, Nn, D, kw = _episode_state(S_cur, G, st, dist_fx, safe, active, prev_active)
    loops, mode = _episode_words(B, ctl, ew, loops)
    _ep_device(S_cur=S_cur, G=G, st=st, dist_fx=dist_fx, safe=safe, active=active, prev_active=prev_active, ctl=ctl, ew=ew)
    _ok(lib().episode_tally(S_cur=ptr(S_cur), S_next=0, stream=stream_handle(),
                            **dict(kw, ctl=ptr(ctl), ew=ptr(ew), loops=loops, mode=mode)), "episode_tally")


def episode_final(S_cur, G, st, dist_fx, safe, active, prev_active, out):
    """The result vector (episode_final_kernel), after the safety-only scan of the final state S_cur:
    out (EP_OUT,) int64 in the order of validate.COUNTS."""
    B, N, Nn, D, kw = _episode_state(S_cur, G, st, dist_fx, safe, active, prev_active)
    _ep(out, torch.int64, (EP_OUT,), "out")
    _ep_device(S_cur=S_cur, G=G, st=st, dist_fx=dist_fx, safe=safe, active=active, prev_active=prev_active, out=out)
    _ok(lib().episode_final(S_cur=ptr(S_cur), S_next=0, stream=stream_handle(), **dict(kw, out=ptr(out))), "episode_final")


def episode_run(buf: dict, *, K, max_steps, check_every, refine, loops, lr, mask_done, persistent, ctrl, cbf,
                a_max=None, local=False, fused=False):
    """A whole batch of closed-loop episodes as one native call (csrc/runtime.cpp EpisodeDriver).

    buf: the call's device buffers (ops/episode.py allocates them): S0 / S1 (B, Nn, 4|8) record
    buffers, both holding s_0 and the obstacle rows; G (B, N, D); idx (B, N, K) int32; A (B, N, D);
    pooled (B, N, 128|256) 16-bit, argmax (B, N, 128) uint8; perm (B, Nn) int32; st (EP_WORDS,) int64 =
    [1, 0, 0, 0, 0]; dist_fx (B,) int64 zero; safe (B,) float32 zero; active (B,) uint8 ones;
    prev_active (B,) uint8 zero; out (EP_OUT,) int64; with refine and loops > 0 also delta (B, N, D)
    zero, h (B, N, K), rptr (B, Nn+1) / redges (B, N*K) int32 and ctl (2*loops,) int64 + dEv
    (B, N, K, D) (loop filter) or ew (B, loops, 2) int64 zero (persistent). ctrl / cbf: (wpack, wvec,
    wrm, ModulePack) of the packed networks (cbf may be None without refine). a_max (optional): the
    per-axis actuator limit (the controller's actions are clamped in place, the filter projects, the
    applied action is clamped). buf may hold act_st (EP_ACT_WORDS,) int64 zero and act_out
    (EP_ACT_WORDS,) int64, both or neither: the action statistics (evaluate.ACTION_STATS).
    local: the decentralised filter (``evaluate.py``'s module docstring) -- no rptr / redges, never
    persistent, the loop filter's ctl; fused (local only): one refine_local launch per step, no dEv.
    Returns (steps issued, index of the record buffer that holds the final state)."""
    K, max_steps, check_every, loops = int(K), int(max_steps), int(check_every), int(loops)
    if K < 1 or K > C.MAX_TOP_K:
        raise NativeError(f"K = {K} outside 1..{C.MAX_TOP_K}")
    if max_steps < 0 or check_every < 1 or loops < 0:
        raise NativeError("max_steps >= 0, check_every >= 1 and loops >= 0 are required")
    local, fused = bool(local), bool(fused)
    if local and persistent:
        raise NativeError("the persistent filter has no local coupling")
    if fused and not local:
        raise NativeError("the fused filter is the local coupling's")
    # what needs no device first: K, the loop counts, the filter's precision
    qc = 0
    bw = bv = brm = bmp = None
    if refine:
        if cbf is None:
            raise NativeError("refine needs the packed CBF")
        bw, bv, brm, bmp = cbf
        qc = _half(bw, "CBF wpack", bmp.prec)
        if qc == 1:
            raise NativeError("safety filter: fp16 is not supported (the -1 upstream gradient has no loss scaling); "
                              "use fp32 or bf16")
    S0 = buf.get("S0")
    B, N, Nn, D, ep = _episode_state(S0, buf.get("G"), buf.get("st"), buf.get("dist_fx"), buf.get("safe"),
                                     buf.get("active"), buf.get("prev_active"))
    W = rec_width(D)
    if K > Nn:
        raise NativeError(f"bad K={K} for Nn={Nn}")
    if Nn > SCAN_MAX_NODES:
        raise NativeError(f"at most {SCAN_MAX_NODES} graph nodes per env (got {Nn})")
    _ep(buf.get("S1"), torch.float32, (B, Nn, W), "S1")
    if buf["S1"].data_ptr() == S0.data_ptr():
        raise NativeError("S1 must not be S0")
    _ep(buf.get("idx"), torch.int32, (B, N, K), "idx")
    _ep(buf.get("A"), torch.float32, (B, N, D), "A")
    _ep(buf.get("perm"), torch.int32, (B, Nn), "perm")
    _ep(buf.get("out"), torch.int64, (EP_OUT,), "out")
    if (buf.get("act_st") is None) != (buf.get("act_out") is None):
        raise NativeError("act_st and act_out come together")
    _ep(buf.get("act_st"), torch.int64, (EP_ACT_WORDS,), "act_st", required=False)
    _ep(buf.get("act_out"), torch.int64, (EP_ACT_WORDS,), "act_out", required=False)
    limit_kw = _episode_limit_kw(a_max, buf.get("act_st"), buf.get("act_out"))
    cw, cv, _, cmp_ = ctrl
    pc = _half(cw, "controller wpack", cmp_.prec)
    _ep(cw, cw.dtype, tuple(cw.shape), "controller wpack")
    _ep(cv, torch.float32, tuple(cv.shape) if isinstance(cv, torch.Tensor) else (), "controller wvec")
    _ep(buf.get("pooled"), cw.dtype, (B, N, _prow(pc)), "pooled")
    _ep(buf.get("argmax"), torch.uint8, (B, N, 128), "argmax")
    filt = bool(refine) and loops > 0
    if filt:
        _ep(bw, bw.dtype, tuple(bw.shape), "CBF wpack")
        _ep(bv, torch.float32, tuple(bv.shape) if isinstance(bv, torch.Tensor) else (), "CBF wvec")
        if bv.numel() < 260 or bw.numel() < (bmp.off["w1f"] + 70) * 512 * _planes(qc):
            raise NativeError("packed CBF weights too small")
        _ep(brm, bw.dtype, (_planes(qc) * (128 * 68 + 64 * 148),), "CBF wrm")
        _ep(buf.get("delta"), torch.float32, (B, N, D), "delta")
        _ep(buf.get("h"), torch.float32, (B, N, K), "h")
        if not local:
            _ep(buf.get("rptr"), torch.int32, (B, Nn + 1), "rptr")
            _ep(buf.get("redges"), torch.int32, (B, N * K), "redges")
        if B * N * (16 if fused else K) >= 2 ** 31 - 2 ** 21:
            raise NativeError("too many edges for 32-bit indexing")
        if persistent:
            if not refine_small_eligible(Nn, K):
                raise NativeError(f"the persistent filter takes envs of at most {SMALL_MAXN} graph nodes")
            _ep(buf.get("ew"), torch.int64, (B, loops, 2), "ew")
        else:
            _ep(buf.get("ctl"), torch.int64, (2 * loops,), "ctl")
            if not fused:
                _ep(buf.get("dEv"), torch.float32, (B, N, K, D), "dEv")
    _ep_device(**{k: t for k, t in buf.items() if isinstance(t, torch.Tensor)}, ctrl_wpack=cw, ctrl_wvec=cv,
               cbf_wpack=bw, cbf_wvec=bv, cbf_wrm=brm)
    dev = S0.device
    E = B * N * K
    global _EPISODE_DRIVER
    if _EPISODE_DRIVER is None:
        _EPISODE_DRIVER = lib().EpisodeDriver()
    g = buf.get
    mode = EP_MODES[None if not filt else "persistent" if persistent else "loop"]
    ep.update(A=ptr(g("A")), delta=ptr(g("delta") if filt else None), ctl=ptr(g("ctl") if mode == 1 else None),
              ew=ptr(g("ew") if mode == 2 else None), loops=loops, mode=mode, out=ptr(g("out")), **limit_kw)
    # the filter's arguments (S: per step; the mask is dropped by the driver unless mask_done)
    loc = {}
    if local:
        loc = dict(local=1, fused=int(fused), fused_blocks=refine_local_grid(B * N, dev, qc))
    flt = _refine_kw(B, N, Nn, K, D, None, g("idx"), g("A"), g("delta"), g("h"), bw, bmp.off["w1f"], brm, bv,
                     None if local else g("rptr"), None if local else g("redges"), lr, env_active=g("active"), a_max=a_max,
                     dEv=ptr(g("dEv") if mode == 1 and not fused else None), ctl=ep["ctl"],
                     ew=ep["ew"], loops=loops, num_blocks=refine_grid(E, dev, qc), prec=qc, **loc) if filt else None
    # the step's launches on S0 (the driver swaps the record buffers): one scan with the kNN lists and the
    # safety count, the safety-only scan of the final state, the controller, and the filter's h(s_t) and CSR
    cs, sc = _scan_kw(S0, g("idx"), None, None, g("safe"), K=K, perm=g("perm"), n_agents=N)
    _, fin = _scan_kw(S0, None, None, None, g("safe"), K=1, do_knn=False, perm=g("perm"), n_agents=N)
    ck, pc, ncu = _ctrl_fwd_kw(S0, g("G"), g("idx"), cw, cmp_.off["ew1f"], cmp_.off["nw1f"], cv, g("A"), None, None, None,
                               pooled=g("pooled"), argmax=g("argmax"), prec=cmp_.prec, res=cmp_.residual)
    cbf_kw, nb = None, 0
    if filt:
        cbf_kw, _, nb = _cbf_fwd_kw(S0[None], g("idx")[None], bw, bmp.off["w1f"], bv, two=False, h_out=g("h")[None],
                                    prec=bmp.prec)
    cfg = dict(episode=ep, refine=flt, cell_sort=cs, scan=sc, scan_final=fin, ctrl=ck, cbf=cbf_kw,
               csr=_rev_csr_kw(g("idx"), g("rptr"), g("redges"), Nn) if filt and not local else None, S1=ptr(g("S1")), num_cu=ncu,
               prec_ctrl=pc, cbf_blocks=nb, max_steps=max_steps, check_every=check_every,
               mask_done=int(bool(mask_done)), stream=stream_handle())
    try:
        steps, cur = _EPISODE_DRIVER.run(cfg)
    except (RuntimeError, ValueError) as e:
        raise NativeError(f"episode driver: {e}") from e
    return int(steps), int(cur)
