"""GPU: node_reduce_kernel (csrc/graph.hip) in the modes the engine runs it in -- map1 + gate,
shift1, n_nodes, t_range, pass_mask, passes=1, accumulate, 3-D records -- against a dense float64
reference.

Reference: record r of slot (t,b,i,k) in pass p is added to out[t+p, b, i] and, if its neighbour
j = idx[t + p*shift1, b, i, k] is an agent (j < N), subtracted from out[t+p, b, j]. With map1 the
records are indexed by evaluation: pass 0 reads record e, pass 1 reads record map1[e] and only
where that is an extra (>= E). A zero gate removes the record; such records are NaN in the input,
so a kernel that loaded one would show it.

Self edges (j == i) cancel in the reference: +r - r. The kernels rely on a contract instead: the
reverse CSR leaves self edges out (csrc/args.h CsrArgs) and every producer of edge records writes
zeros for self pairs (csrc/cbf.hip), so node_reduce adds the self record to its node and never
subtracts it. The inputs here follow that contract (zero_self_records); the zero terms are exact
in any sum and are not counted in n_terms.

Tolerance per node and component:
(n_terms - 1) * 2**-24 * sum|terms| -- the kernel adds the n_terms records in fp32 in a fixed tree
(any order of n_terms values has at most n_terms - 1 inexact additions, each below half an ulp of
a partial sum that is at most sum|terms|)."""
import pytest
import torch

from macbf_gnn_amd.ops import native

import dedup_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
U24 = 2.0 ** -24
SHAPES = [(3, 3, 37, 12), (2, 1, 8, 5)]          # 7 blocks with a ragged tail; one partial block


def _note(group, ratio):
    print(f"RATIO {group} {ratio:.4f}")


def planted_graphs(G, N, K, n_nodes=None, seed=0):
    """(G, N, K) int64 lists: slot 0 is a self edge, slot 1 the hub (in-degree N - 1 + its self edge
    > 16: more than one round of in-edge slots), nobody lists the orphan (its own slot 0 points
    elsewhere), the other slots are distinct random nodes; hub and orphan move with the graph.
    n_nodes > N: about a fifth of the free slots point at obstacle nodes."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.zeros(G, N, K, dtype=torch.long)
    for q in range(G):
        hub, orphan = (1 + q) % N, (2 + q) % N
        for i in range(N):
            free = [j for j in range(N) if j not in (i, hub, orphan)]
            perm = torch.randperm(len(free), generator=g).tolist()
            row = [free[p] for p in perm[:K]]
            row[0] = i if i != orphan else row[0]
            if i != hub:
                row[1] = hub
            idx[q, i] = torch.tensor(row)
    if n_nodes is not None and n_nodes > N:
        obst = torch.randint(N, n_nodes, (G, N, K), generator=g)
        swap = torch.rand(G, N, K, generator=g) < 0.2
        swap[..., :2] = False
        idx = torch.where(swap, obst, idx)
    return idx


def zero_self_records(dE, idx, *, T, B, N, K, shift1=0, map1=None):
    """Zero the records of self pairs in place (the producers' contract, see the module docstring):
    slot e of pass p is a self pair if idx[t + p*shift1, b, i, k] == i."""
    E = T * B * N * K
    flat = dE.view(-1, dE.shape[-1])
    e = torch.arange(E).view(T, B, N, K)
    me = torch.arange(N).view(1, 1, N, 1)
    for p in range(dE.shape[0]):
        selfm = idx[p * shift1:p * shift1 + T].long() == me
        x = p * E + e
        if map1 is not None and p == 1:
            x = map1.long()
            selfm = selfm & (x >= E)
        flat[x[selfm]] = 0.0
    return dE


def reference(dE, idx, *, T, B, N, K, passes=2, pass_mask=0, shift1=0, map1=None, gate=None, out0=None,
              contract=True):
    """-> (out, bound) float64 (T+1, B, N, W). dE (passes,T,B,N,K,W), idx (>= T + shift1, B, N, K),
    map1 (T,B,N,K), gate (passes*E,), out0: the accumulate=True input. contract: assert that the
    records of self pairs are zero."""
    W = dE.shape[-1]
    E = T * B * N * K
    flat = dE.reshape(-1, W).double().cpu()
    idx = idx.long().cpu()
    out = torch.zeros(T + 1, B, N, W, dtype=torch.float64)
    asum = torch.zeros_like(out)
    nterm = torch.zeros(T + 1, B, N, dtype=torch.float64)
    if out0 is not None:
        out += out0.double().cpu()
        asum += out0.double().cpu().abs()
        nterm += 1
    e = torch.arange(E).view(T, B, N, K)
    for p in range(passes):
        if pass_mask and not (pass_mask >> p) & 1:
            continue
        if map1 is not None and p == 1:
            x = map1.long().cpu()
            on = x >= E
        else:
            x = p * E + e
            on = torch.ones(T, B, N, K, dtype=torch.bool)
        if gate is not None:
            on = on & (gate.cpu()[x] != 0)
        r = torch.where(on[..., None], flat[x], torch.zeros((), dtype=torch.float64))       # (T,B,N,K,W)
        j = idx[p * shift1:p * shift1 + T]
        notself = j != torch.arange(N).view(1, 1, N, 1)
        assert not contract or bool((r[on & ~notself] == 0).all())
        out[p:p + T] += r.sum(3)
        asum[p:p + T] += r.abs().sum(3)
        nterm[p:p + T] += (on & notself).sum(3)
        into = on & (j < N)
        jj = j.clamp(max=N - 1).reshape(T * B, N * K)
        rr = torch.where(into[..., None], r, torch.zeros((), dtype=torch.float64)).reshape(T * B, N * K, W)
        out[p:p + T].view(T * B, N, W).scatter_add_(1, jj[..., None].expand(-1, -1, W), -rr)
        asum[p:p + T].view(T * B, N, W).scatter_add_(1, jj[..., None].expand(-1, -1, W), rr.abs())
        nterm[p:p + T].view(T * B, N).scatter_add_(1, jj, (into & notself).reshape(T * B, N * K).double())
    bound = (nterm - 1).clamp_min(0)[..., None] * U24 * asum
    return out, bound


def _csr(idx, n_nodes=None):
    G, B, N, K = idx.shape
    Nn = N if n_nodes is None else n_nodes
    i32 = idx.to(torch.int32).to(DEV).contiguous()
    rptr = torch.zeros(G * B, Nn + 1, dtype=torch.int32, device=DEV)
    redges = torch.zeros(G * B, N * K, dtype=torch.int32, device=DEV)
    native.rev_csr(i32.view(G * B, N, K), rptr, redges, n_nodes=n_nodes)
    return rptr, redges


def _records(passes, T, B, N, K, W, seed, idx=None, shift1=0, map1=None):
    """Random records; with idx: self pairs zeroed."""
    g = torch.Generator().manual_seed(seed)
    dE = torch.randn(passes, T, B, N, K, W, generator=g)
    if idx is not None:
        zero_self_records(dE, idx, T=T, B=B, N=N, K=K, shift1=shift1, map1=map1)
    return dE


def _run(dE, idx, *, T, B, N, K, out=None, n_nodes=None, **kw):
    W = dE.shape[-1]
    rptr, redges = _csr(idx, n_nodes)
    if out is None:
        out = torch.full((T + 1, B, N, W), 4321.0, device=DEV)       # every row is written: no zero-fill needed
    native.node_reduce(dE.to(DEV).contiguous(), rptr, redges, out, T=T, B=B, N=N, K=K, n_nodes=n_nodes,
                       passes=dE.shape[0], **kw)
    torch.cuda.synchronize()
    return out


def _check(got, ref, bound, group):
    err = (got.cpu().double() - ref).abs()
    assert not bool(torch.isnan(got).any())
    pos = bound > 0
    if bool(pos.any()):
        _note(group, float((err[pos] / bound[pos]).max()))
    assert bool((err <= bound).all()), float((err - bound).max())


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


@pytest.mark.parametrize("W", [4, 8])
@pytest.mark.parametrize("T,B,N,K", SHAPES)
def test_defaults_two_passes(T, B, N, K, W):
    idx = planted_graphs(T * B, N, K, seed=1).view(T, B, N, K)
    dE = _records(2, T, B, N, K, W, seed=2, idx=idx)
    # the planted structure is there
    deg = torch.zeros(N, dtype=torch.long).scatter_add_(0, idx[0, 0].reshape(-1), torch.ones(N * K, dtype=torch.long))
    assert int(deg[1]) == N and int(deg[2]) == 0                    # graph 0: hub 1 (+ its self edge), orphan 2
    assert bool((idx[0, 0, 3:, 0] == torch.arange(3, N)).all())     # self edges in slot 0
    ref, bound = reference(dE, idx, T=T, B=B, N=N, K=K)
    got = _run(dE, idx, T=T, B=B, N=N, K=K)
    _check(got, ref, bound, "node_reduce.default")
    again = _run(dE, idx, T=T, B=B, N=N, K=K)
    assert torch.equal(got, again)                                   # deterministic: identical bits


@pytest.mark.parametrize("T,B,N,K", SHAPES)
def test_one_pass(T, B, N, K):
    idx = planted_graphs(T * B, N, K, seed=3).view(T, B, N, K)
    dE = _records(1, T, B, N, K, 4, seed=4, idx=idx)
    ref, bound = reference(dE, idx, T=T, B=B, N=N, K=K, passes=1)
    got = _run(dE, idx, T=T, B=B, N=N, K=K)
    _check(got, ref, bound, "node_reduce.passes1")
    assert bool((got[T] == 0).all())                                 # no pass reaches the last row


@pytest.mark.parametrize("T,B,N,K", SHAPES)
def test_shift1_reads_pass1_edges_from_the_next_graph(T, B, N, K):
    idx = planted_graphs((T + 1) * B, N, K, seed=5).view(T + 1, B, N, K)
    assert not torch.equal(idx[:T], idx[1:])
    dE = _records(2, T, B, N, K, 4, seed=6, idx=idx, shift1=1)
    ref, bound = reference(dE, idx, T=T, B=B, N=N, K=K, shift1=1)
    got = _run(dE, idx, T=T, B=B, N=N, K=K, shift1=1)
    _check(got, ref, bound, "node_reduce.shift1")
    wrong, _ = reference(dE, idx, T=T, B=B, N=N, K=K, shift1=0, contract=False)
    assert bool(((ref - wrong).abs() > 10 * bound).any())            # the two readings are told apart


@pytest.mark.parametrize("shift1", [0, 1])
@pytest.mark.parametrize("T,B,N,K", SHAPES)
def test_obstacle_nodes_receive_nothing(T, B, N, K, shift1):
    Nn = N + 5
    idx = planted_graphs((T + shift1) * B, N, K, n_nodes=Nn, seed=7).view(T + shift1, B, N, K)
    assert bool((idx >= N).any())
    dE = _records(2, T, B, N, K, 4, seed=8, idx=idx, shift1=shift1)
    ref, bound = reference(dE, idx, T=T, B=B, N=N, K=K, shift1=shift1)
    got = _run(dE, idx, T=T, B=B, N=N, K=K, n_nodes=Nn, shift1=shift1)
    _check(got, ref, bound, "node_reduce.n_nodes")


@pytest.mark.parametrize("T,B,N,K", SHAPES)
def test_pass_mask_keeps_pass_1_only(T, B, N, K):
    idx = planted_graphs(T * B, N, K, seed=9).view(T, B, N, K)
    dE = _records(2, T, B, N, K, 4, seed=10, idx=idx)
    dE[0] = float("nan")                                             # the masked pass is never loaded
    ref, bound = reference(dE, idx, T=T, B=B, N=N, K=K, pass_mask=2)
    got = _run(dE, idx, T=T, B=B, N=N, K=K, pass_mask=2)
    _check(got, ref, bound, "node_reduce.pass_mask")
    assert bool((got[0] == 0).all())


@pytest.mark.parametrize("T,B,N,K", SHAPES)
def test_accumulate(T, B, N, K):
    idx = planted_graphs(T * B, N, K, seed=11).view(T, B, N, K)
    dE = _records(2, T, B, N, K, 4, seed=12, idx=idx)
    out0 = torch.randn(T + 1, B, N, 4, generator=torch.Generator().manual_seed(13))
    ref, bound = reference(dE, idx, T=T, B=B, N=N, K=K, out0=out0)
    got = _run(dE, idx, T=T, B=B, N=N, K=K, out=out0.to(DEV).clone(), accumulate=True)
    _check(got, ref, bound, "node_reduce.accumulate")


def _engine_case(shape, recomputed, W, seed, by_slot=False):
    """map1 + gate as HipEngine._backward passes them: records by evaluation, gate = dL/dh, NaN
    records wherever the gate is zero (the active-list backward never writes those). by_slot: the
    same gate over records indexed by (pass, slot), for the calls without map1."""
    c = R.make_case(*shape, R.case_seed(shape), recomputed, "drop")
    T, B, N, K = shape
    E, U = c["E"], c["U"]
    dh, _, _ = R.dh_reference(c["h"], c["hmask"], c["map1"], c["src"], U, c["dang"], c["valid"], c["counts"])
    gate = torch.zeros(2 * E)
    gate[:U] = dh.float()
    assert 0 < int((gate != 0).sum()) < U
    dE = _records(2, T, B, N, K, W, seed=seed, idx=c["idx"], shift1=int(recomputed),
                  map1=None if by_slot else c["map1"])
    dE.view(2 * E, W)[gate == 0] = float("nan")
    return c, gate, dE


@pytest.mark.parametrize("W", [4, 8])
@pytest.mark.parametrize("recomputed", [False, True], ids=["reuse", "rc"])
@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]], ids=lambda s: "x".join(map(str, s)))
def test_map1_and_gate(shape, recomputed, W):
    T, B, N, K = shape
    c, gate, dE = _engine_case(shape, recomputed, W, seed=14)
    s1 = int(recomputed)
    kw = dict(T=T, B=B, N=N, K=K, shift1=s1)
    ref, bound = reference(dE, c["idx"], map1=c["map1"], gate=gate, **kw)
    m32 = c["map1"].to(torch.int32)
    got = _run(dE, c["idx"], map1=_dev(m32), gate=_dev(gate), **kw)
    _check(got, ref, bound, "node_reduce.map1_gate")
    assert torch.equal(got, _run(dE, c["idx"], map1=_dev(m32), gate=_dev(gate), **kw))     # identical bits
    # pass 1 carries the extras only: reading every map1 entry would differ
    assert bool((c["map1"] < c["E"]).any()) or T == 1
    # map1 with pass 1 only
    ref, bound = reference(dE, c["idx"], map1=c["map1"], gate=gate, pass_mask=2, **kw)
    got = _run(dE, c["idx"], map1=_dev(m32), gate=_dev(gate), pass_mask=2, **kw)
    _check(got, ref, bound, "node_reduce.map1_gate")
    # gate alone: records by (pass, slot) under a mask
    c, gate, dE = _engine_case(shape, recomputed, W, seed=14, by_slot=True)
    ref, bound = reference(dE, c["idx"], gate=gate, **kw)
    got = _run(dE, c["idx"], gate=_dev(gate), **kw)
    _check(got, ref, bound, "node_reduce.gate")


@pytest.mark.parametrize("engine", [False, True], ids=["plain", "map1_gate"])
def test_t_range_halves_equal_the_full_call(engine):
    if engine:
        shape = R.SHAPES[2]
        T, B, N, K = shape
        c, gate, dE = _engine_case(shape, True, 4, seed=15)
        idx = c["idx"]
        kw = dict(T=T, B=B, N=N, K=K, shift1=1, map1=_dev(c["map1"].to(torch.int32)), gate=_dev(gate))
    else:
        T, B, N, K = SHAPES[0]
        idx = planted_graphs(T * B, N, K, seed=16).view(T, B, N, K)
        dE = _records(2, T, B, N, K, 4, seed=17, idx=idx)
        kw = dict(T=T, B=B, N=N, K=K)
    full = _run(dE, idx, **kw)
    for ts in range(1, T + 1):
        out = torch.full((T + 1, B, N, 4), -77.0, device=DEV)
        _run(dE, idx, out=out, t_range=(ts, T + 1), **kw)
        assert bool((out[:ts] == -77.0).all())                       # rows outside the range are untouched
        assert torch.equal(out[ts:], full[ts:])
        _run(dE, idx, out=out, t_range=(0, ts), **kw)
        assert torch.equal(out, full)
    out = torch.full((T + 1, B, N, 4), -77.0, device=DEV)
    _run(dE, idx, out=out, t_range=(1, 2), **kw)
    assert bool((out[:1] == -77.0).all()) and bool((out[2:] == -77.0).all()) and torch.equal(out[1], full[1])
