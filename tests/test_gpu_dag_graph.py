"""Graph queries of the DAG conditioner on the device (-m gpu): gnf_dag_levels / ops.dag_levels against a Kahn walk in numpy on
the host, the C ABI at its minimum alignment, and DAGConditioner / NormalizingFlowStep with `device_graph` set against the
same objects without it.  Every expected value comes from ref_levels() below, from networkx or from the host statements of
the conditioner, never from the kernel."""
import ctypes

import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 2, 63, 64, 65, 127, 129, 200, 1030)         # the word boundaries, and more rows than the 1024 threads of the peel


# ------------------------------------------------------------------------------------------------ reference and graphs
def ref_levels(adj):
    """Kahn walk.  adj[i, j]: j is a parent of i.  -> (level with -1 on or behind a cycle, n_levelled, n_levels)"""
    adj = np.asarray(adj, dtype=bool)
    d = adj.shape[0]
    rows, cols = np.nonzero(adj)                           # edge cols -> rows
    by_parent = np.argsort(cols, kind="stable")
    kids, start = rows[by_parent], np.searchsorted(cols[by_parent], np.arange(d + 1))
    indeg = adj.sum(1).astype(np.int64)                    # a self loop keeps its node above zero for ever
    level = np.full(d, -1, dtype=np.int64)
    frontier, k, done = np.nonzero(indeg == 0)[0], 0, 0
    while frontier.size:
        level[frontier] = k
        done += frontier.size
        ch = np.concatenate([kids[start[j]:start[j + 1]] for j in frontier]) if frontier.size else kids[:0]
        np.subtract.at(indeg, ch, 1)
        frontier = np.unique(ch[indeg[ch] == 0])
        k += 1
    return level, done, k


def test_reference_walk_is_networkx():
    """the yardstick itself, once, against nx.topological_generations and nx.dag_longest_path_length"""
    adj = graphs(40, 3)[0]
    level, done, k = ref_levels(adj)
    G = nx.from_numpy_array(adj.T.astype(np.float32), create_using=nx.DiGraph)      # nx: entry [u, v] is the edge u -> v
    gens = list(nx.topological_generations(G))
    assert done == 40 and k == len(gens) == nx.dag_longest_path_length(G) + 1
    for g, nodes in enumerate(gens):
        assert sorted(nodes) == np.nonzero(level == g)[0].tolist()
    cyc = graphs(40, 3)[3]
    level, done, _ = ref_levels(cyc)
    assert done < 40 and not nx.is_directed_acyclic_graph(nx.from_numpy_array(cyc.T.astype(np.float32), create_using=nx.DiGraph))


def perm_dag(d, seed, density=.1):
    """a seeded lower-triangular graph under a random permutation, with the edge perm[0] -> perm[1] (d > 1)"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(d)
    low = np.tril(rng.random((d, d)) < density, -1)
    if d > 1:
        low[1, 0] = True
    adj = np.zeros((d, d), dtype=bool)
    adj[np.ix_(perm, perm)] = low
    return adj, perm


def graphs(d, seed):
    """[permuted DAG, empty, chain (d rounds), DAG + one 2-cycle, DAG + a self loop].  d == 1 has no 2-cycle: its fourth
    graph is the self loop too."""
    dag, perm = perm_dag(d, seed)
    chain = np.zeros((d, d), dtype=bool)
    chain[perm[1:], perm[:-1]] = True
    two = dag.copy()
    if d > 1:
        two[perm[0], perm[1]] = True                       # perm[0] -> perm[1] is an edge of the DAG: now a 2-cycle
    else:
        two[0, 0] = True
    loop = dag.copy()
    loop[perm[d // 2], perm[d // 2]] = True
    return [dag, np.zeros((d, d), dtype=bool), chain, two, loop]


def check(level, info, adjs):
    level, info = level.cpu().numpy(), info.cpu().numpy()
    assert level.dtype == np.int32 and info.dtype == np.int32
    for g, adj in enumerate(adjs):
        want, done, k = ref_levels(adj)
        assert info[g].tolist() == [done, k], (g, info[g], done, k)
        assert np.array_equal(level[g], want), (g, np.nonzero(level[g] != want)[0][:8])


# ------------------------------------------------------------------------------------------------ raw op
@pytest.mark.parametrize("d", SIZES)
def test_levels_against_the_host_walk(d):
    from gnf_hip import ops
    adjs = graphs(d, 100 + d)
    level, info = ops.dag_levels(torch.from_numpy(np.stack(adjs)).float().to(DEV))
    assert level.shape == (5, d) and info.shape == (5, 2)
    check(level, info, adjs)
    lv = level.cpu().numpy()
    assert info[1].tolist() == [d, 1] and info[2].tolist() == [d, d]               # empty graph, chain
    if d > 2:
        two = adjs[3]
        behind = np.nonzero(two[:, np.nonzero(lv[3] == -1)[0]].any(1))[0]              # children of an unlevelled node
        assert (lv[3][behind] == -1).all() and (lv[3] == -1).sum() >= 2


def test_longest_peel_at_the_edge_of_the_domain():
    from gnf_hip import ops
    d = 4096
    perm = torch.from_numpy(np.random.default_rng(5).permutation(d)).to(DEV)
    M = torch.zeros(d, d, dtype=torch.bool, device=DEV)
    M[perm[1:], perm[:-1]] = True
    level, info = ops.dag_levels(M)
    assert level.shape == (d,) and info.tolist() == [d, d]
    assert torch.equal(level[perm].cpu(), torch.arange(d, dtype=torch.int32))       # node perm[t] sits behind t parents
    with pytest.raises(Exception, match="GNF_ESHAPE"):
        ops.dag_levels(torch.zeros(4097, 4097, dtype=torch.bool, device=DEV))
    assert not ops.dag_levels_supported(4097) and ops.dag_levels_supported(4096)


def test_element_types_strides_and_batches():
    from gnf_hip import ops
    d = 129
    adjs = graphs(d, 7)[:1] + [perm_dag(d, 8, .3)[0], graphs(d, 9)[3]]
    f = torch.from_numpy(np.stack(adjs)).float().to(DEV) * 2.5
    want = ops.dag_levels(f)
    check(*want, adjs)                                                             # G = 3 distinct matrices
    for other in (ops.dag_levels(f != 0), ops.dag_levels((f != 0).to(torch.uint8))):   # bool and uint8 storage
        assert torch.equal(other[0], want[0]) and torch.equal(other[1], want[1])
    big = torch.full((3, d + 2, d + 7), 9., device=DEV)                             # ld > d, graph stride > d * ld: edges all around
    view = big[:, 1:d + 1, 3:d + 3]
    view.copy_(f)
    got = ops.dag_levels(view)
    assert view.stride() == ((d + 2) * (d + 7), d + 7, 1)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    bview = (big != 0)[:, 1:d + 1, 3:d + 3]
    got = ops.dag_levels(bview)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    one = ops.dag_levels(view[1])                                                  # [d, d]: no batch dimension in the result
    assert one[0].shape == (d,) and torch.equal(one[0], want[0][1]) and torch.equal(one[1], want[1][1])
    again = ops.dag_levels(f)                                                      # the same call, the same bytes
    assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])
    empty = ops.dag_levels(torch.zeros(0, d, d, device=DEV))                       # G == 0
    assert empty[0].shape == (0, d) and empty[1].shape == (0, 2)


def test_thresholds_over_one_shared_matrix():
    from gnf_hip import ops
    d = 200
    rng = np.random.default_rng(11)
    dag, perm = perm_dag(d, 12, .2)
    w = rng.random((d, d)).astype(np.float32)
    M = np.where(dag, w, 0.).astype(np.float32)
    back = dag.T & (rng.random((d, d)) < .3)                                       # weak back edges: cycles at low thresholds
    M = np.where(back, .45 * w, M).astype(np.float32)
    ths = [.05, .2, .4, .6, .95]
    level, info = ops.dag_levels(torch.from_numpy(M).to(DEV), ths)
    assert level.shape == (5, d) and info.shape == (5, 2)
    check(level, info, [M > np.float32(t) for t in ths])
    lv, nf = level.cpu().numpy(), info.cpu().numpy()
    assert nf[0, 0] < d and nf[-1, 0] == d                                         # cyclic at first, acyclic in the end
    for g in range(4):                                                             # fewer edges: nothing gets worse
        assert nf[g + 1, 0] >= nf[g, 0]
        both = lv[g] >= 0
        assert (lv[g + 1][both] >= 0).all() and (lv[g + 1][both] <= lv[g][both]).all()
    tens = ops.dag_levels(torch.from_numpy(M).to(DEV), torch.tensor(ths, device=DEV))
    assert torch.equal(tens[0], level) and torch.equal(tens[1], info)
    per_graph = ops.dag_levels(torch.from_numpy(M).to(DEV).expand(5, d, d).contiguous(), ths)
    assert torch.equal(per_graph[0], level) and torch.equal(per_graph[1], info)


def test_predicate_edges_are_torchs():
    """entries at float32(th), one ulp around it, -0.0, NaN, +-inf: node i has the ONE candidate parent i - 1, so the levels show
    every decision.  The expectation is torch's own `M > th` (th a Python float, compared in fp32) and `M != 0` on the device."""
    from gnf_hip import ops
    th = .15                                                                       # float32(.15) > .15
    t32 = np.float32(th)
    vals = np.array([t32, np.nextafter(t32, np.float32(0)), np.nextafter(t32, np.float32(1)), -0., 0., np.nan, np.inf, -np.inf,
                     1., np.float32(1e-45), -1.], dtype=np.float32)
    d = vals.size + 1
    M = np.zeros((d, d), dtype=np.float32)
    M[np.arange(1, d), np.arange(d - 1)] = vals
    Md = torch.from_numpy(M).to(DEV)
    above, nonzero = (Md > th).cpu().numpy(), (Md != 0).cpu().numpy()
    assert np.array_equal(above, M > t32)                                          # pinned: the scalar is rounded to fp32 first
    assert float(t32) > th and float(M[1, 0]) > th and not above[1, 0]             # an edge in double, none in fp32
    assert above[3, 2] and not above[2, 1] and not above[6, 5] and above[7, 6] and not above[8, 7]
    assert not nonzero[4, 3] and not nonzero[5, 4] and nonzero[6, 5]               # -0.0, 0.0, NaN
    level, info = ops.dag_levels(Md, [th])
    check(level, info, [above])
    level, info = ops.dag_levels(Md)
    check(level[None], info[None], [nonzero])
    level, info = ops.dag_levels(torch.stack((Md, Md.abs())), [th, 2.])
    check(level, info, [above, np.abs(M) > 2.])


# ------------------------------------------------------------------------------------------------ C ABI
def raw(M, et, stride_g, ld, th, level, info, ws_ptr, ws_bytes, G, d):
    from gnf_hip import abi
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return abi.load().gnf_dag_levels(p(M), et, stride_g, ld, p(th), p(level), p(info), ctypes.c_void_p(ws_ptr), ws_bytes, G, d,
                                     abi.stream())


def test_abi_at_minimum_alignment_and_every_entry_written():
    from gnf_hip import abi
    lib = abi.load()
    d = 65
    adjs = graphs(d, 21)[:1] + [graphs(d, 22)[3]]
    fbuf = torch.zeros(2 * d * d + 1, device=DEV)
    Mf = fbuf[1:].view(2, d, d)                                                    # fp32 M one float off
    Mf.copy_(torch.from_numpy(np.stack(adjs)).float())
    bbuf = torch.zeros(2 * d * d + 1, dtype=torch.uint8, device=DEV)
    Mb = bbuf[1:].view(2, d, d)                                                    # uint8 M one byte off
    Mb.copy_(torch.from_numpy(np.stack(adjs)).to(torch.uint8))
    thr = torch.full((3,), -7., device=DEV)[1:]                                    # thresholds one float off: m > -7 keeps 0 too
    assert Mf.data_ptr() % 8 == 4 and Mb.data_ptr() % 2 == 1 and thr.data_ptr() % 8 == 4
    nws = lib.gnf_dag_levels_ws_bytes(2, d)
    assert nws == 2 * (2 + 1) * d * 8
    ws = torch.zeros(nws // 4 + 4, dtype=torch.int32, device=DEV)
    base = ws.data_ptr() + (-ws.data_ptr()) % 8
    for M, et in ((Mf, abi.DAG_ELEM_F32), (Mb, abi.DAG_ELEM_U8)):
        lbuf = torch.full((2 * d + 1,), -99, dtype=torch.int32, device=DEV)
        ibuf = torch.full((4 + 1,), -99, dtype=torch.int32, device=DEV)
        level, info = lbuf[1:].view(2, d), ibuf[1:].view(2, 2)                     # outputs one int off, filled with a sentinel
        assert level.data_ptr() % 8 == 4 and info.data_ptr() % 8 == 4
        assert raw(M, et, d * d, d, None, level, info, base, nws, 2, d) == 0
        check(level, info, adjs)                                                   # -1 and levels only: every entry was written
        assert int(lbuf[0]) == -99 and int(ibuf[0]) == -99 and int((level == -99).sum()) == 0
    # a complete graph with self loops under the offset thresholds: nothing is levelled
    lbuf = torch.full((2 * d,), -99, dtype=torch.int32, device=DEV)
    ibuf = torch.full((4,), -99, dtype=torch.int32, device=DEV)
    assert raw(Mf, abi.DAG_ELEM_F32, d * d, d, thr, lbuf, ibuf, base, nws, 2, d) == 0
    assert ibuf.tolist() == [0, 0, 0, 0] and int((lbuf != -1).sum()) == 0
    # refused before any launch: ws at a dword that is no 8-byte address, ws too small, uint8 with thresholds, ld < d
    lbuf.fill_(-99)
    ibuf.fill_(-99)
    assert raw(Mf, abi.DAG_ELEM_F32, d * d, d, None, lbuf, ibuf, base + 4, nws, 2, d) == -1
    assert raw(Mf, abi.DAG_ELEM_F32, d * d, d, None, lbuf, ibuf, base, nws - 1, 2, d) == -3
    assert raw(Mb, abi.DAG_ELEM_U8, d * d, d, thr, lbuf, ibuf, base, nws, 2, d) == -1
    assert raw(Mf, abi.DAG_ELEM_F32, d * d, d - 1, None, lbuf, ibuf, base, nws, 2, d) == -1
    assert raw(Mf, abi.DAG_ELEM_F32, 0, 4097, None, lbuf, ibuf, base, nws, 2, 4097) == -2
    torch.cuda.synchronize()
    assert int((lbuf != -99).sum()) == 0 and int((ibuf != -99).sum()) == 0         # nothing was touched
    assert raw(Mf, abi.DAG_ELEM_F32, d * d, d, None, lbuf, ibuf, base, nws, 2, d) == 0   # and the device is as usable as before
    check(lbuf.view(2, d), ibuf.view(2, 2), adjs)
    assert raw(None, abi.DAG_ELEM_F32, 0, d, None, None, None, 0, 0, 0, d) == 0    # G == 0: NULL everywhere


# ------------------------------------------------------------------------------------------------ conditioner
def weighted(adj, seed, weak_back=None):
    """A for a conditioner: weights in [1, 2) on the edges (the 2-cycles of `weak_back` edges at that weight)"""
    g = torch.Generator().manual_seed(seed)
    A = torch.from_numpy(adj).float() * (1. + torch.rand(adj.shape, generator=g))
    if weak_back is not None:
        r, c = np.nonzero(adj)
        A[torch.from_numpy(c[:weak_back[0]]), torch.from_numpy(r[:weak_back[0]])] = weak_back[1]
    return A


def mnist_prior():
    from models.NormalizingFlowFactories import MNIST_A_prior
    return MNIST_A_prior(28, 2)                            # the 5x5 windows, both directions: full of 2-cycles


def mnist_dag():
    return (mnist_prior() * torch.tril(torch.ones(784, 784), -1)).numpy() > 0


CONDS = {"d12": lambda: weighted(perm_dag(12, 31, .4)[0], 1),
         "d12-cyclic": lambda: weighted(graphs(12, 32)[3], 2),
         "d200": lambda: weighted(perm_dag(200, 33, .05)[0], 3),
         "d200-weak-cycles": lambda: weighted(perm_dag(200, 34, .05)[0], 4, weak_back=(5, .45)),
         "mnist-prior-lower": lambda: weighted(mnist_dag(), 5),
         "mnist-prior": mnist_prior}


def conditioner(A):
    from models import DAGConditioner
    torch.manual_seed(0)
    cond = DAGConditioner(A.shape[0], [8, 8], 2, A_prior=A.clone()).to(DEV)
    return cond


def counted(monkeypatch):
    from gnf_hip import ops
    calls, real = [], ops.dag_levels
    monkeypatch.setattr(ops, "dag_levels", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def as_lists(lv, with_host):
    if lv is None:
        return None
    for item in lv:
        rows = item[0] if with_host else item
        assert rows.dtype == torch.long and rows.device.type == "cuda" and rows.dim() == 1
        if with_host:
            assert isinstance(item[1], tuple) and all(type(r) is int for r in item[1]) and list(item[1]) == rows.tolist()
    return [(item[0] if with_host else item).tolist() for item in lv]


@pytest.mark.parametrize("name", list(CONDS))
def test_conditioner_queries_equal_the_host_statements(name, monkeypatch):
    A = CONDS[name]()
    d = A.shape[0]
    calls = counted(monkeypatch)
    want_level, done, k = ref_levels(A.numpy() > 0)
    out = []
    for on in (True, False):
        cond = conditioner(A)
        cond.device_graph = on
        assert cond._device_graph() == on
        n0 = len(calls)
        P = cond.soft_thresholded_A()
        res = [as_lists(cond.levels(with_host=True), True), as_lists(cond.levels(), False), as_lists(cond.levels(P=P), False),
               as_lists(cond.levels(P=P, with_host=True), True), cond.depth()]
        assert (len(calls) - n0 == 5) == on and (len(calls) == n0) != on
        cond.post_process()
        assert (len(calls) - n0 == 6) == on
        res += [cond.A.detach().cpu().clone(), cond.A.requires_grad, cond.depth(), as_lists(cond.levels(), False)]
        out.append(res)
    for a, b in zip(*out):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    lv = out[0][0]
    if done == d:                                                                  # and both equal the reference
        assert out[0][4] == k - 1 and [sorted(l) for l in lv] == lv
        assert lv == [np.nonzero(want_level == g)[0].tolist() for g in range(k)]
    else:
        assert lv is None and out[0][4] == 0


@pytest.mark.parametrize("name", ["d200-weak-cycles", "d12"])
def test_post_process_threshold_is_the_first_acyclic_candidate(name):
    from models.Conditionners.DAGConditioner import threshold_candidates
    A = CONDS[name]()
    d = A.shape[0]
    cond = conditioner(A)
    cond.device_graph = True
    S = cond.soft_thresholded_A().detach().abs().cpu().numpy()
    th = next(t for t in threshold_candidates() if ref_levels(S > np.float32(t))[1] == d)
    assert (th > .1) == (name == "d200-weak-cycles")                               # cyclic at .1, acyclic at a later candidate
    cond.post_process()
    assert np.array_equal(cond.A.detach().cpu().numpy(), ((S > np.float32(th)) & ~np.eye(d, dtype=bool)).astype(np.float32))
    assert not cond.A.requires_grad and cond.levels() is not None
    explicit = conditioner(A)
    explicit.device_graph = True
    explicit.post_process(zero_threshold=.01)                                      # an explicit threshold: no search
    assert np.array_equal(explicit.A.detach().cpu().numpy(), ((S > np.float32(.01)) & ~np.eye(d, dtype=bool)).astype(np.float32))


@pytest.mark.parametrize("name", ["d12", "d12-cyclic", "d200", "mnist-prior"])
def test_last_branch_of_the_dual_update(name, monkeypatch):
    A = CONDS[name]()
    calls = counted(monkeypatch)
    acyclic = ref_levels((A * A).numpy() != 0)[1] == A.shape[0]
    states = []
    for on in (True, False):
        cond = conditioner(A)
        cond.device_graph = on
        cond._set("dag_const", 0.)                                                 # the constraint is off: the last branch
        n0 = len(calls)
        cond.update_dual_param()
        assert (len(calls) - n0 == 1) == on
        states.append((cond.is_invertible, float(cond.dag_const), cond.stoch_gate, cond.A.requires_grad,
                       cond.A.detach().cpu().clone()))
    assert states[0][:4] == states[1][:4] and torch.equal(states[0][4], states[1][4])
    assert states[0][0] == acyclic and states[0][1] == (0. if acyclic else 1.)


# ------------------------------------------------------------------------------------------------ whole flows
def freeze(cond, A):
    cond.stoch_gate = cond.noise_gate = cond.s_thresh = False
    cond.h_thresh = 0.
    with torch.no_grad():
        cond.A.copy_(A.to(DEV))
    cond.A.requires_grad = False
    cond.is_invertible = True
    cond.invalidate_caches()


def test_inversion_of_a_small_flow_is_bit_identical(monkeypatch):
    """eager pass, capture and hipGraph replay under both settings"""
    from models import AffineNormalizer, DAGConditioner
    from models.NormalizingFlow import NormalizingFlowStep, _INV_GRAPHS
    d = 12
    adj = perm_dag(d, 41, .5)[0]
    assert ref_levels(adj)[2] > 5                                                  # more than 4 levels: the pass is graphed
    torch.manual_seed(42)
    cond = DAGConditioner(d, [16, 16], 2).to(DEV)
    freeze(cond, torch.from_numpy(adj).float())
    step = NormalizingFlowStep(cond, AffineNormalizer()).to(DEV)
    z = torch.randn(5, d, generator=torch.Generator().manual_seed(43)).to(DEV)
    calls = counted(monkeypatch)
    xs = {}
    for on in (False, True):
        cond.device_graph = on
        cond.invalidate_caches()                                                   # a new schedule request, new graphs
        _INV_GRAPHS.pop(step, None)
        xs[on] = [step.invert(z) for _ in range(3)]
        assert any(isinstance(v, tuple) for v in _INV_GRAPHS[step].values())       # the second call captured, the third replayed
        assert len(calls) == (1 if on else 0)                                      # one query per gate state
    for x in xs[False] + xs[True]:
        assert torch.equal(x, xs[False][0])
    with torch.no_grad():
        back, _ = step(xs[True][2])
    assert torch.allclose(back, z, atol=1e-4)
    cond.is_invertible = False
    step.level_schedule = False                                                    # the fixed-point passes: depth() + 1 of them
    fixed = {}
    for on in (False, True):
        cond.device_graph = on
        fixed[on] = step.invert(z)
    assert torch.equal(fixed[True], fixed[False]) and len(calls) == 2


def test_cifar_sized_flow():
    """d = 3072, B = 2: the schedule of a seeded sparse DAG from the device equals the host walk, and so do the samples"""
    from models import AffineNormalizer
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow
    d = 3072
    torch.manual_seed(50)
    flow = buildCIFAR10NormalizingFlow([1], AffineNormalizer, {}).to(DEV)
    cond = flow.getConditioners()[0]
    gen = torch.Generator().manual_seed(51)
    order = torch.randperm(d, generator=gen)
    A = torch.zeros(d, d)
    A[order[1:8], order[0:7]] = 1.
    for t in range(1, d):
        A[order[t], order[torch.randint(0, t, (2,), generator=gen)]] = 1.
    freeze(cond, A)
    want, done, k = ref_levels(A.numpy() > 0)
    assert done == d and k > 4
    cond.device_graph = True
    assert cond._device_graph()
    lv = cond.levels(with_host=True)
    assert [list(h) for _, h in lv] == [np.nonzero(want == g)[0].tolist() for g in range(k)]
    assert all(r.tolist() == list(h) for r, h in lv) and cond.depth() == k - 1
    z = torch.randn(2, d, generator=torch.Generator().manual_seed(52)).to(DEV) * .5
    flow.steps[0].graph_invert = False
    x_dev = flow.invert(z)
    cond.device_graph = False
    cond.invalidate_caches()
    assert torch.equal(flow.invert(z), x_dev)
