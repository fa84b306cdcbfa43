"""The first layer of a DAGMLP with the DAG gate and the one-hot fused in (csrc/gnf_dagmlp.hip, gnf_hip.ops.DagMlpFrontFn /
dag_mlp_rows, DAGMLP.gated_front): against fp64 (the oracle's masked copies followed by the linear chain in fp64 torch) and
against the composed path (DagGateFn + MLPFn, `gated_front = False`).

Ties: the fused first layer sums in another order than the GEMM on e, so a hidden ReLU within fp32 roundoff of zero may
legitimately flip.  Tied samples (dagmlp_ref.tied_samples, the criterion of conftest.integrand_knife_elements) are redrawn with
knife_units.resample_off_ties; every remaining case is compared at the normal tolerance, none is excluded."""
import ctypes

import pytest
import torch

from conftest import assert_fwd
from dagmlp_ref import (CASES, DEV, INJECTED, SHAPES, assert_grad, chain64, copies64, cu, draw_inputs, graph_nodes,
                        hidden_of, layers64, make_cond, set_noise, tied_samples)
from knife_units import resample_off_ties

pytestmark = pytest.mark.gpu

FUSED, GATE = "DagMlpFrontFnBackward", "DagGateFnBackward"


def sid(shape):
    return "x".join(str(v) for v in shape)


def run(cond, x, on, cot=None, want_x=False):
    """(h, autograd nodes, gradients by name) of one conditioner call with the switch set to `on`, same Philox offset"""
    cond.embedding_net.gated_front = on
    cond._gate_calls = 40
    cond.zero_grad(set_to_none=True)
    xd = cu(x).clone().requires_grad_(want_x)
    h = cond(xd)
    nodes = graph_nodes(h)
    grads = None
    if cot is not None:
        (h * cot).sum().backward()
        grads = {n: p.grad.clone() for n, p in cond.named_parameters() if p.grad is not None}
        if want_x:
            grads["x"] = xd.grad.clone()
    return h.detach(), nodes, grads


def philox_copies(cond, x):
    """e as cond.masked_inputs returns it for the (gate_seed, _gate_calls) of run()"""
    cond._gate_calls = 40
    with torch.no_grad():
        return cond.masked_inputs(cu(x)).detach().cpu().double()


# ------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_forward_against_fp64_and_the_composed_path(shape, case):
    B, d, H = shape
    for hot in (True, False):
        cond = make_cond(d, hidden_of(d, H), 30, hot, case, 100 + B + d, DEV)
        gen = torch.Generator().manual_seed(1000 + B * d + H)
        x, u1, u2 = draw_inputs(B, d, case, gen)
        set_noise(cond, case, u1, u2)
        h1, nodes1, _ = run(cond, x, True)
        h0, nodes0, _ = run(cond, x, False)
        assert FUSED in nodes1 and GATE not in nodes1, nodes1
        assert GATE in nodes0 and FUSED not in nodes0, nodes0
        e = copies64(cond, case, x.double(), u1, u2) if CASES[case][4] or case == "det" else philox_copies(cond, x)
        ref = chain64(e, layers64(cond)).view(B, d, -1)
        assert_fwd(h1, ref, what="fused against fp64 (hot %s)" % hot)
        assert_fwd(h1, h0, what="fused against composed (hot %s)" % hot)


# ------------------------------------------------------------------------------------------- 2. gradients
def clean_draw(cond, case, B, d, gen, copies=None):
    """inputs without a tied sample: (x, u1, u2), rounds"""
    L = layers64(cond)
    copies = copies or (lambda x, u1, u2: copies64(cond, case, x.double(), u1, u2))
    return resample_off_ties(lambda: draw_inputs(B, d, case, gen),
                             lambda x, u1, u2: tied_samples(copies(x, u1, u2), L, B, d))


def reference_grads(cond, case, x, u1, u2, cot):
    """fp64: (h, {name: gradient}, cotangent of the first layer's pre-activation)"""
    L = layers64(cond)
    x64 = x.double().requires_grad_(True)
    A64 = cond.A.detach().cpu().double().requires_grad_(True)
    P = [p.clone().requires_grad_(True) for Wb in L for p in Wb]
    keep = []
    h = chain64(copies64(cond, case, x64, u1, u2, A=A64), list(zip(P[0::2], P[1::2])), keep)
    keep[0].retain_grad()
    (h * cot.double().view(h.shape)).sum().backward()
    g = {"x": x64.grad, "A": A64.grad}
    for l in range(len(L)):
        g["embedding_net.net.%d.weight" % (2 * l)] = P[2 * l].grad
        g["embedding_net.net.%d.bias" % (2 * l)] = P[2 * l + 1].grad
    return h.detach(), g, keep[0].grad


def check_grads(got, ref, d, hot, names=None):
    for n in (names or ref):
        assert n in got, (n, sorted(got))
        assert_grad(got[n], ref[n], n)
    w1 = "embedding_net.net.0.weight"
    if w1 in (names or ref):
        assert_grad(got[w1][:, :d], ref[w1][:, :d], "gW1[:, :d]")
        if hot:
            assert_grad(got[w1][:, d:], ref[w1][:, d:], "gW1[:, d:2d]")


GRAD_CASES = [(s, True) for s in SHAPES] + [((7, 6, 60), False), ((100, 21, 210), False)]


@pytest.mark.parametrize("case", INJECTED)
@pytest.mark.parametrize("shape,hot", GRAD_CASES, ids=lambda v: sid(v) if isinstance(v, tuple) else ("hot" if v else "plain"))
def test_gradients_against_fp64(shape, hot, case):
    B, d, H = shape
    cond = make_cond(d, hidden_of(d, H), 30, hot, case, 200 + B + d, DEV)
    gen = torch.Generator().manual_seed(2000 + B * d + H)
    (x, u1, u2), rounds = clean_draw(cond, case, B, d, gen)
    set_noise(cond, case, u1, u2)
    cot = torch.randn(B, d, 30, generator=gen)
    h64, ref, gpre = reference_grads(cond, case, x, u1, u2, cot)
    h1, nodes, got = run(cond, x, True, cu(cot), want_x=True)
    assert FUSED in nodes and GATE not in nodes
    assert_fwd(h1, h64.view(B, d, -1), what="forward")
    check_grads(got, ref, d, hot)
    if hot:                                                     # the one-hot half of gW1 is a sum over the samples alone
        assert_grad(got["embedding_net.net.0.weight"][:, d:], gpre.view(B, d, -1).sum(0).t(), "gW1[:, d:2d] against sum_b")
    if case == "h_thresh":
        from oracle import gnf_oracle as O
        off = O.dag_soft_thresholded_A(cond.A.detach().cpu().double()) <= CASES[case][3]
        if d > 1:
            assert bool(off.any()) and bool((~off).any())
        assert bool((got["A"].cpu()[off] == 0).all()), "gA where dP/dA = 0"
    # the same call, the same bits
    _, _, again = run(cond, x, True, cu(cot), want_x=True)
    assert set(again) == set(got)
    for n in got:
        assert torch.equal(got[n], again[n]), n
    # a frozen A: no gradient for it, the others unchanged
    cond.A.requires_grad = False
    _, nodes, frozen = run(cond, x, True, cu(cot), want_x=True)
    assert FUSED in nodes and cond.A.grad is None and "A" not in frozen
    check_grads(frozen, ref, d, hot, names=[n for n in ref if n != "A"])


@pytest.mark.parametrize("shape", [(7, 6, 60), (300, 8, 80), (100, 21, 210), (64, 63, 630)], ids=sid)
def test_philox_gradients(shape):
    """Philox noise at T = .5 (the UCI driver's setting): the parameter gradients against fp64 on e as masked_inputs returns
    it, gA and gx against the composed path, which regenerates the same noise"""
    B, d, H = shape
    case = "philox-T.5"
    cond = make_cond(d, hidden_of(d, H), 30, True, case, 300 + B + d, DEV)
    gen = torch.Generator().manual_seed(3000 + B * d + H)
    (x, u1, u2), _ = clean_draw(cond, case, B, d, gen, copies=lambda x, u1, u2: philox_copies(cond, x))
    set_noise(cond, case, u1, u2)
    cot = torch.randn(B, d, 30, generator=gen)
    L = layers64(cond)
    P = [p.clone().requires_grad_(True) for Wb in L for p in Wb]
    h64 = chain64(philox_copies(cond, x), list(zip(P[0::2], P[1::2])))
    (h64 * cot.double().view(h64.shape)).sum().backward()
    h1, nodes1, g1 = run(cond, x, True, cu(cot), want_x=True)
    h0, nodes0, g0 = run(cond, x, False, cu(cot), want_x=True)
    assert FUSED in nodes1 and GATE not in nodes1 and GATE in nodes0
    assert_fwd(h1, h64.detach().view(B, d, -1), what="forward")
    for l in range(len(L)):
        assert_grad(g1["embedding_net.net.%d.weight" % (2 * l)], P[2 * l].grad, "gW%d" % (l + 1))
        assert_grad(g1["embedding_net.net.%d.bias" % (2 * l)], P[2 * l + 1].grad, "gb%d" % (l + 1))
    assert_grad(g1["A"], g0["A"].cpu(), "gA against the composed path")
    assert_grad(g1["x"], g0["x"].cpu(), "gx against the composed path")


# ------------------------------------------------------------------------------------------- 3. one-layer DAGMLP
@pytest.mark.parametrize("case", ["det", "gumbel-injected", "noise-gate"])
@pytest.mark.parametrize("shape", [(5, 3, 2), (7, 6, 30), (33, 43, 30)], ids=sid)
def test_one_layer_dagmlp(shape, case):
    """hidden = []: the first layer is the whole net, identity activation"""
    B, d, out = shape
    for hot in (True, False):
        cond = make_cond(d, [], out, hot, case, 400 + B + d, DEV)
        gen = torch.Generator().manual_seed(4000 + B * d)
        x, u1, u2 = draw_inputs(B, d, case, gen)
        set_noise(cond, case, u1, u2)
        cot = torch.randn(B, d, out, generator=gen)
        L = layers64(cond)
        assert len(L) == 1
        x64 = x.double().requires_grad_(True)
        A64 = cond.A.detach().cpu().double().requires_grad_(True)
        W, b = (p.clone().requires_grad_(True) for p in L[0])
        h64 = chain64(copies64(cond, case, x64, u1, u2, A=A64), [(W, b)])
        (h64 * cot.double().view(h64.shape)).sum().backward()
        ref = {"x": x64.grad, "A": A64.grad, "embedding_net.net.0.weight": W.grad, "embedding_net.net.0.bias": b.grad}
        h1, nodes, got = run(cond, x, True, cu(cot), want_x=True)
        assert FUSED in nodes and GATE not in nodes and "MLPFnBackward" not in nodes
        assert_fwd(h1, h64.detach().view(B, d, -1), what="forward")
        check_grads(got, ref, d, hot)


# ------------------------------------------------------------------------------------------- 4. rows form
def rows_reference(cond, x, P, rows, vm):
    """fp64 of the parent's torch statements (DAGConditioner.forward_rows)"""
    B, d, R = x.shape[0], x.shape[1], len(rows)
    idx = torch.tensor(rows, dtype=torch.long)
    e = (x.double().unsqueeze(1) * P.double()[idx].unsqueeze(0))
    if cond.hot_encoding:
        hot = torch.zeros(R, d, dtype=torch.float64)
        hot[torch.arange(R), idx] = 1.
        e = torch.cat((e, hot.unsqueeze(0).expand(B, -1, -1)), 2)
    h = chain64(e.reshape(B * R, -1), layers64(cond)).view(B, R, -1)
    return h.permute(1, 0, 2) if vm else h


@pytest.mark.parametrize("hot", [True, False], ids=["hot", "plain"])
@pytest.mark.parametrize("B,d,H", [(9, 6, 60), (5, 21, 210), (3, 63, 630), (70, 8, 80)])
def test_forward_rows(B, d, H, hot, monkeypatch):
    from gnf_hip import ops
    cond = make_cond(d, hidden_of(d, H), 30, hot, "det", 500 + d, DEV)
    net = cond.embedding_net
    calls = []
    real = ops.dag_mlp_rows
    monkeypatch.setattr(ops, "dag_mlp_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    gen = torch.Generator().manual_seed(5000 + d)
    x = torch.randn(B, d, generator=gen)
    with torch.no_grad():
        P = cond.deterministic_importance().detach()
        perm = torch.randperm(d, generator=gen).tolist()
        subsets = [[], [d - 1], perm[:max(d // 3, 1)], list(range(d)), perm]
        for rows in subsets:
            rt = torch.tensor(rows, dtype=torch.long, device=DEV)
            for vm in (False, True):
                net.gated_front = True
                n0 = len(calls)
                h1 = cond.forward_rows(cu(x), rt, P, variable_major=vm)
                assert len(calls) == n0 + 1
                assert tuple(h1.shape) == ((len(rows), B, 30) if vm else (B, len(rows), 30))
                if not rows:
                    continue
                net.gated_front = False
                h0 = cond.forward_rows(cu(x), rt, P, variable_major=vm)
                assert len(calls) == n0 + 1
                ref = rows_reference(cond, x, P.cpu(), rows, vm)
                assert_fwd(h1, ref, what="rows %d vm %s against fp64" % (len(rows), vm))
                assert_fwd(h1, h0, what="rows %d vm %s against the torch statements" % (len(rows), vm))
        # a level loop, twice: the same bits
        net.gated_front = True
        with torch.no_grad():
            cond.A.copy_(torch.tril(torch.ones(d, d), -1).to(DEV) * cond.A)
        cond.invalidate_caches()
        P = cond.deterministic_importance().detach()
        levels = cond.levels(P)
        assert levels is not None and sum(r.numel() for r in levels) == d
        passes = [[cond.forward_rows(cu(x), r, P, variable_major=True).clone() for r in levels] for _ in range(2)]
        for a, b, r in zip(passes[0], passes[1], levels):
            assert torch.equal(a, b)
            assert_fwd(a, rows_reference(cond, x, P.cpu(), r.tolist(), True), what="level")


def dag_flow(d, hidden, seed, band=None):
    """one Affine + DAG step with hot encoding behind a post-processed (frozen 0/1) lower-triangular A"""
    from models import AffineNormalizer, DAGConditioner, buildFCNormalizingFlow
    torch.manual_seed(seed)
    A = torch.tril(torch.ones(d, d), -1)
    if band:
        A = A * (torch.triu(torch.ones(d, d), -band))
    flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": hidden, "out_size": 2, "hot_encoding": True,
                                                      "A_prior": A * 1.5}, AffineNormalizer, {}).to(DEV)
    cond = flow.getConditioners()[0]
    cond.post_process()
    cond.is_invertible = True
    assert cond.deterministic_importance() is not None and not cond.A.requires_grad
    return flow, cond


@pytest.mark.parametrize("d,hidden,band", [(8, [80, 80, 80], None), (21, [210], 3)], ids=["d8", "d21"])
def test_invert_round_trip(d, hidden, band, monkeypatch):
    from gnf_hip import ops
    flow, cond = dag_flow(d, hidden, 600 + d, band)
    calls = []
    real = ops.dag_mlp_rows
    monkeypatch.setattr(ops, "dag_mlp_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    x = cu(torch.randn(32, d, generator=torch.Generator().manual_seed(6000 + d)))
    out = {}
    with torch.no_grad():
        for on in (True, False):
            cond.embedding_net.gated_front = on
            n0 = len(calls)
            z, _ = flow(x)
            assert len(calls) == n0 + (1 if on else 0)          # the no-grad forward behind post_process(): the rows kernel
            xs = [flow.invert(z) for _ in range(3)]             # eager, captured, replayed
            assert (len(calls) > n0 + 1) == on
            for xr in xs[1:]:
                assert torch.equal(xr, xs[0])
            out[on] = (z, xs[0])
    from conftest import rel_err
    assert rel_err(out[True][1].cpu(), x.cpu()) < 1e-4
    assert_fwd(out[True][0], out[False][0], what="z")
    assert_fwd(out[True][1], out[False][1], what="inverted x")


# ------------------------------------------------------------------------------------------- 5. fall-backs
def both_switches(cond, x, cot):
    on, off = run(cond, x, True, cot), run(cond, x, False, cot)
    assert FUSED not in on[1] and on[1] == off[1], (on[1], off[1])
    assert torch.equal(on[0], off[0])
    assert set(on[2]) == set(off[2])
    for n in on[2]:
        assert torch.equal(on[2][n], off[2][n]), n
    return on


def test_fallbacks_keep_the_parents_statements():
    gen = torch.Generator().manual_seed(70)
    # d = 65: outside the kernels' domain
    cond = make_cond(65, [32], 4, True, "philox-T.5", 700, DEV)
    assert not cond.embedding_net.supports_gated(cu(torch.zeros(2, 65)), True)
    on = both_switches(cond, torch.randn(3, 65, generator=gen), cu(torch.randn(3, 65, 4, generator=gen)))
    assert GATE in on[1]
    # gumble = False: the clipped-normal gate of torch ops
    cond = make_cond(6, [16], 4, True, "gumbel-injected", 701, DEV)
    cond.gumble = False
    cond.gate_noise = (cu(torch.randn(3, 6, 6, generator=gen)),)
    on = both_switches(cond, torch.randn(3, 6, generator=gen), cu(torch.randn(3, 6, 4, generator=gen)))
    assert GATE not in on[1]
    # a CPU conditioner: neither path exists without the GPU, the fused one is not tried
    from gnf_hip import abi
    cond = make_cond(6, [16], 4, True, "det", 702, "cpu")
    cond.embedding_net.gated_front = True
    assert not cond.embedding_net.supports_gated(torch.zeros(2, 6), True)
    with pytest.raises(abi.GnfError):
        cond(torch.zeros(2, 6))


def test_image_nets_take_the_nodes_they_took():
    from models import DAGConditioner
    from models.MLP import CIFAR10CNN, MNISTCNN
    torch.manual_seed(71)
    cond = DAGConditioner(784, MNISTCNN(out_d=2), 2).to(DEV)
    h = cond(cu(torch.randn(1, 784)))
    assert "DagConvFrontFnBackward" in graph_nodes(h) and FUSED not in graph_nodes(h)
    net = CIFAR10CNN(out_d=2, fc_l=[16, 32, 32], size_img=[1, 8, 8], k_size=2)
    net.gated_front = True
    cond = DAGConditioner(64, net, 2).to(DEV)
    h = cond(cu(torch.randn(2, 64)))
    assert "DagLenetFrontFnBackward" in graph_nodes(h) and FUSED not in graph_nodes(h)
    assert not getattr(net, "accepts_hot", False) and not getattr(MNISTCNN, "accepts_hot", False)
    cond.hot_encoding = True                                    # they keep refusing the one-hot columns
    seen = []
    net.forward = lambda e, context=None: (seen.append(tuple(e.shape)), e[:, :2] * net.fc3.bias)[1]
    h = cond(cu(torch.randn(2, 64)))
    assert seen == [(128, 128)] and GATE in graph_nodes(h)


# ------------------------------------------------------------------------------------------- 6. raw C ABI
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("B,d,H,hot", [(7, 6, 60, 1), (4, 21, 30, 1), (3, 63, 17, 0)])
def test_raw_abi_at_dword_alignment(B, d, H, hot):
    """every new entry point on operands 4, 8 and 12 bytes past a 16-byte boundary and W1 rows of pitch > 2 d: the bits of
    the aligned call (the summation order does not depend on the alignment), guard bands intact"""
    from gnf_hip import abi, ops
    from misaligned import guards_intact, place
    gen = torch.Generator().manual_seed(80 + d)
    kw = 2 * d if hot else d
    ld = kw + 3
    x, A = cu(torch.randn(B, d, generator=gen)), cu(.8 + .4 * torch.randn(d, d, generator=gen))
    Wbig, b1 = cu(torch.randn(H, ld, generator=gen) * .3), cu(torch.randn(H, generator=gen) * .1)
    g = cu(torch.randn(B * d, H, generator=gen))
    rows = torch.randperm(d, generator=gen)[:max(d // 2, 1)].to(torch.int32).to(DEV)
    R = rows.numel()
    lib, st = abi.load(), abi.stream
    ntab = int(lib.gnf_dag_gate_fwd_ws_bytes(d)) // 4
    nws = int(lib.gnf_dagmlp_gated_bwd_ws_bytes(B, d, H))
    assert int(lib.gnf_dagmlp_supported(d, H)) == 1
    res = {}
    for k in (0, 1, 2, 3):
        xk, Ak, bk, gk = place(x, k), place(A, k), place(b1, k), place(g, k)
        Wk = place(Wbig[:, :kw], k)
        assert Wk.stride(0) == ld
        tab = place(torch.zeros(ntab, device=DEV), k)
        a1 = place(torch.zeros(B * d, H, device=DEV), k)
        abi.call("gnf_dagmlp_gated_fwd", _p(xk), _p(Ak), _p(tab), ops.IMP_SOFT, ops.GATE_GUMBEL, 0., .5, None, None, 77, 5,
                 _p(Wk), ld, _p(bk), hot, 1, _p(a1), B, d, H, st())
        gx, gA, gb = (place(torch.zeros(s, device=DEV), k) for s in ((B, d), (d, d), (H,)))
        gW = place(torch.full((H, ld), 7., device=DEV)[:, :kw], k)
        ws = place(torch.zeros(nws // 4 + 4, device=DEV), k)
        abi.call("gnf_dagmlp_gated_bwd", _p(xk), _p(tab), ops.IMP_SOFT, ops.GATE_GUMBEL, .5, None, None, 77, 5, _p(Wk), ld,
                 hot, _p(gk), _p(gx), _p(gA), 0, _p(gW), ld, _p(gb), _p(ws), nws, B, d, H, st())
        Pk = place(torch.sigmoid(A), k)
        r1 = place(torch.zeros(B * R, H, device=DEV), k)
        r2 = place(torch.zeros(R * B, H, device=DEV), k)
        for out, vm in ((r1, 0), (r2, 1)):
            abi.call("gnf_dagmlp_rows_fwd", _p(xk), _p(Pk), d, _p(rows), R, _p(Wk), ld, _p(bk), hot, 1, _p(out), vm, B, d, H,
                     st())
        torch.cuda.synchronize()
        for t in (xk, Ak, bk, gk, Wk, tab, a1, gx, gA, gb, gW, ws, Pk, r1, r2):
            assert guards_intact(t)
        res[k] = [t.clone() for t in (a1, gx, gA, gW, gb, r1, r2)]
    for k in (1, 2, 3):
        for a, b, name in zip(res[k], res[0], ("a1", "gx", "gA", "gW1", "gb1", "rows", "rows variable-major")):
            assert torch.equal(a, b), (name, k)
    # the raw calls against the autograd node on contiguous operands
    xr, Ar = x.clone().requires_grad_(True), A.clone().requires_grad_(True)
    W, b = Wbig[:, :kw].contiguous().requires_grad_(True), b1.clone().requires_grad_(True)
    a1 = ops.dag_mlp_front(xr, Ar, ops.IMP_SOFT, ops.GATE_GUMBEL, 0., .5, None, None, 77, 5, W, b, bool(hot), True)
    a1.backward(g)
    for a, b_, name in zip(res[0][:5], (a1.detach(), xr.grad, Ar.grad, W.grad, b.grad), ("a1", "gx", "gA", "gW1", "gb1")):
        assert torch.equal(a, b_), name
    assert torch.equal(res[0][5].view(B, R, H).permute(1, 0, 2), res[0][6].view(R, B, H))
    assert_fwd(res[0][5], ops.dag_mlp_rows(x, torch.sigmoid(A), rows, W.detach(), b.detach(), bool(hot), True), what="rows")


def test_raw_abi_empty_batch_and_unsupported_shapes():
    from gnf_hip import abi, ops
    lib, st = abi.load(), abi.stream
    d, H = 6, 20
    A, W, b = cu(torch.rand(d, d)), cu(torch.randn(H, 2 * d)), cu(torch.randn(H))
    tab = torch.zeros(int(lib.gnf_dag_gate_fwd_ws_bytes(d)) // 4, device=DEV)
    assert lib.gnf_dagmlp_gated_fwd(None, _p(A), _p(tab), 1, 1, 0., .5, None, None, 1, 1, _p(W), 2 * d, _p(b), 1, 1, None, 0, d,
                                    H, st()) == 0
    nws = int(lib.gnf_dagmlp_gated_bwd_ws_bytes(0, d, H))
    assert nws > 0
    ws = torch.zeros(nws // 4 + 1, device=DEV)
    gA, gW, gb = (torch.full(s, float("nan"), device=DEV) for s in ((d, d), (H, 2 * d), (H,)))
    assert lib.gnf_dagmlp_gated_bwd(None, _p(tab), 1, 1, .5, None, None, 1, 1, _p(W), 2 * d, 1, None, None, _p(gA), 0, _p(gW),
                                    2 * d, _p(gb), _p(ws), nws, 0, d, H, st()) == 0
    assert lib.gnf_dagmlp_rows_fwd(None, _p(A), d, None, d, _p(W), 2 * d, _p(b), 1, 1, None, 0, 0, d, H, st()) == 0
    torch.cuda.synchronize()
    for t in (gA, gW, gb):
        assert bool((t == 0).all())
    # through autograd: an empty batch gives zero parameter gradients
    # (the conditioner itself stops at its `.view(0, d, -1)` like the reference: tests/test_gpu_empty.py)
    Ar, Wr, br = (t.clone().requires_grad_(True) for t in (A, W, b))
    a1 = ops.dag_mlp_front(torch.zeros(0, d, device=DEV), Ar, 1, 1, 0., .5, None, None, 1, 1, Wr, br, True, True)
    assert tuple(a1.shape) == (0, H) and FUSED in graph_nodes(a1)
    a1.sum().backward()
    for t in (Ar, Wr, br):
        assert tuple(t.grad.shape) == tuple(t.shape) and bool((t.grad == 0).all())
    # unsupported shapes: a code, no launch
    d = 65
    x, A, W, b = cu(torch.zeros(2, d)), cu(torch.zeros(d, d)), cu(torch.zeros(H, 2 * d)), cu(torch.zeros(H))
    tab, a1 = torch.zeros(4 * d * d, device=DEV), torch.zeros(2 * d, H, device=DEV)
    assert int(lib.gnf_dagmlp_supported(d, H)) == 0
    assert lib.gnf_dagmlp_gated_fwd(_p(x), _p(A), _p(tab), 1, 1, 0., .5, None, None, 1, 1, _p(W), 2 * d, _p(b), 1, 1, _p(a1),
                                    2, d, H, st()) != 0
    assert lib.gnf_dagmlp_rows_fwd(_p(x), _p(A), d, None, d, _p(W), 2 * d, _p(b), 1, 1, _p(a1), 0, 2, d, H, st()) != 0
    assert lib.gnf_dagmlp_gated_bwd_ws_bytes(2, d, H) < 0
    assert lib.gnf_dagmlp_gated_bwd(_p(x), _p(tab), 1, 1, .5, None, None, 1, 1, _p(W), 2 * d, 1, _p(a1), None, _p(A), 0,
                                    _p(W), 2 * d, _p(b), _p(tab), 4 * d * d * 4, 2, d, H, st()) != 0
    assert lib.gnf_dagmlp_gated_fwd(_p(x), _p(A), _p(tab), 1, 1, 0., .5, None, None, 1, 1, _p(W), 2 * d, _p(b), 1, 1, _p(a1),
                                    2, 6, 0, st()) != 0
    torch.cuda.synchronize()
    assert bool((a1 == 0).all())


# ------------------------------------------------------------------------------------------- 7. memory
def test_peak_memory_drops_by_one_copy_of_e():
    """(256, 63, 630), one hidden layer, stochastic gate: the peak of forward + backward with the fused path lies below the
    composed path's by at least the bytes of one e [B d, 2 d] (the design removes e and its cotangent)"""
    B, d, H = 256, 63, 630
    cond = make_cond(d, [H], 30, True, "philox-T.5", 1000, DEV)
    gen = torch.Generator().manual_seed(10000)
    x, cot = cu(torch.randn(B, d, generator=gen)), cu(torch.randn(B, d, 30, generator=gen))
    one_e, peak = B * d * 2 * d * 4, {}
    for on in (True, False):
        cond.embedding_net.gated_front = on
        cond.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        (cond(x) * cot).sum().backward()
        torch.cuda.synchronize()
        peak[on] = torch.cuda.max_memory_allocated() - base
    print("peak bytes above the operands: fused %d, composed %d; one e: %d" % (peak[True], peak[False], one_e))
    assert peak[True] <= peak[False] - one_e, (peak, one_e)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- 8. whole flows
def uci_flow(d, monotonic, on, seed, hidden):
    from gnf_hip import dp
    from models import AffineNormalizer, DAGConditioner, MonotonicNormalizer, buildFCNormalizingFlow
    torch.manual_seed(seed)
    out = 10 if monotonic else 2
    cargs = {"in_size": d, "hidden": hidden, "out_size": out, "hot_encoding": True, "gumble_T": .5, "l1": .2}
    nargs = {"integrand_net": [16, 16], "cond_size": out, "nb_steps": 10} if monotonic else {}
    flow = buildFCNormalizingFlow(2, DAGConditioner, cargs, MonotonicNormalizer if monotonic else AffineNormalizer,
                                  nargs).to(DEV)
    for c in flow.getConditioners():
        c.embedding_net.gated_front = on
    dp.seed_gates(flow, 0)
    return flow


@pytest.mark.parametrize("monotonic", [False, True], ids=["affine", "monotonic"])
@pytest.mark.parametrize("d,hidden", [(6, [20, 20]), (21, [32])], ids=["d6", "d21"])
def test_training_step_of_whole_flows(d, hidden, monotonic, monkeypatch):
    """one dp.train_step with the stochastic gate: loss and updated parameters with the fused front against the composed path"""
    from gnf_hip import dp, ops
    calls = []
    real = ops.dag_mlp_front
    monkeypatch.setattr(ops, "dag_mlp_front", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    x = cu(torch.randn(8, d, generator=torch.Generator().manual_seed(1100 + d)))
    res = {}
    for on in (True, False):
        flow = uci_flow(d, monotonic, on, 1100 + d, hidden)
        state = dp.FlatState(flow)
        n0 = len(calls)
        loss = dp.train_step(flow, state, x, lr=1e-3)
        assert len(calls) - n0 == (2 if on else 0)
        res[on] = (loss.detach().clone(), state.flat.clone())
    assert bool(torch.isfinite(res[False][0]))
    assert_fwd(res[True][0], res[False][0], what="loss")
    assert_grad(res[True][1], res[False][1].cpu(), "parameters after the step")


@pytest.mark.parametrize("monotonic", [False, True], ids=["affine", "monotonic"])
def test_graphed_steps_behind_post_process(monotonic, monkeypatch):
    """after post_process() the step is graphable: three replayed steps of dp.GraphedStep match three eager steps, with the
    fused front in both (autograd on, frozen deterministic gate: the gated node with GATE_DET)"""
    from gnf_hip import dp, ops
    d = 6

    def make():
        flow = uci_flow(d, monotonic, True, 1200, [20, 20])
        for c in flow.getConditioners():
            with torch.no_grad():
                c.A.copy_(torch.tril(torch.ones(d, d), -1).to(DEV) * 1.5)
            c.post_process()
        return flow
    xs = [cu(torch.randn(8, d, generator=torch.Generator().manual_seed(1210 + i))) for i in range(4)]
    fa = make()
    assert dp.GraphedStep.graphable(fa)
    calls = []
    real = ops.dag_mlp_front
    monkeypatch.setattr(ops, "dag_mlp_front", lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1])
    sa = dp.FlatState(fa)
    for x in xs:
        la = dp.train_step(fa, sa, x, lr=1e-3, graph=False)
    assert len(calls) == 8 and all(g == ops.GATE_DET for g in calls)
    fb = make()
    sb = dp.FlatState(fb)
    gs = dp.GraphedStep(fb, sb, xs[0], lr=1e-3, warmup=1)
    for x in xs[1:]:
        lb = gs(x)
    torch.cuda.synchronize()
    assert gs.captures == 1 and sb.t == sa.t == 4
    assert_fwd(lb, la.detach(), what="loss of the third replayed step")
    assert_grad(sb.flat, sa.flat.cpu(), "parameters after three replayed steps")
