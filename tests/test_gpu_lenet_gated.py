"""GPU: the DAG gate fused into the LeNet front of CIFAR10CNN (gnf_lenet_gated_*, gnf_hip.ops.DagLenetFrontFn,
CIFAR10CNN.forward_gated): the masked copies are built in LDS, neither they nor their cotangent exist in memory.

The yardstick is the composed path (`gated_front = False`: DagGateFn + LenetConvFn), which tests/test_gpu_lenet.py holds to
the fp64 oracle.  Both paths get the same Philox stream (`gate_seed`, `_gate_calls` set before every call).  The forward
must agree BIT FOR BIT, so every ReLU and pool decision is the same on both sides and the gradient comparisons need no
knife-edge handling.  Gradient tolerance: rel_err < 1e-4 of the tensor maximum and
|a - b| <= 1e-6 max|b| + 1e-4 |b| per entry.  One test compares against the fp64 restatement directly, with the knife-edge
condition of tests/test_gpu_lenet.py."""
import ctypes
import os

import pytest
import torch

from conftest import assert_close, assert_fwd, rel_err
import lenet_ref
from lenet_ref import DEV, assert_grad, cu, geo_args, graph_nodes
import misaligned

pytestmark = pytest.mark.gpu
GEOS = lenet_ref.GEOMETRIES
FEAT = (400, 576, 64, 16)
DIMS = tuple(s[0] * s[1] * s[2] for s, _, _ in GEOS)          # 3072, 1024, 256, 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def open_uniforms(shape, gen):
    """injected gate noise in the OPEN interval (0, 1) (tests/test_gpu_lenet.py: at an exact 0 the injected-noise form of
    the gate does not return the reference's limit; the endpoint is left to the gate's own tests)"""
    return torch.rand(shape, generator=gen).clamp_(min=2. ** -24)


def conv_params(gi, seed):
    size_img, k, _ = GEOS[gi]
    torch.manual_seed(seed)
    c1, c2 = torch.nn.Conv2d(size_img[0], 6, k), torch.nn.Conv2d(6, 16, k)
    return [t.detach().clone() for t in (c1.weight, c1.bias, c2.weight, c2.bias)]


# gate cases: (stoch_gate, noise_gate, gumble_T, h_thresh, injected noise)
GATES = {"deterministic": (False, False, 1., 0., False),
         "gumbel_injected": (True, False, 1., 0., True),
         "gumbel_T1": (True, False, 1., 0., False),
         "gumbel_T05": (True, False, .5, 0., False),
         "gumbel_T07": (True, False, .7, 0., False),
         "noise_gate": (False, True, 1., 0., False),
         "h_thresh": (True, False, 1., .3, False)}
# each geometry at B = 1 and at one B whose last group of IPB samples is partial (IPB = 28 / 5 / 1 / 1); d = 1024 and 3072
# have more (row, chunk) units than the backward's 512 workgroups: the row loop
CASES = [(gi, B, gate) for gi, Bs in ((3, (1, 30)), (2, (1, 7))) for B in Bs for gate in GATES]
CASES += [(gi, B, "gumbel_T1") for gi in (1, 0) for B in (1, 2)]
IDS = ["d%d-B%d-%s" % (DIMS[gi], B, gate) for gi, B, gate in CASES]


def make_conditioner(gi, gate):
    from models import DAGConditioner
    from models.MLP import CIFAR10CNN
    size_img, k, fc_l = GEOS[gi]
    stoch, noise, T, h_thresh, _ = GATES[gate]
    torch.manual_seed(70 + gi)
    net = CIFAR10CNN(out_d=2, fc_l=list(fc_l), size_img=list(size_img), k_size=k)
    cond = DAGConditioner(DIMS[gi], net, 2)
    cond.stoch_gate, cond.noise_gate, cond.gumble_T, cond.h_thresh = stoch, noise, T, h_thresh
    if h_thresh > 0:
        # about half of the entries below the hard threshold: importance and dP/dA exactly 0 there
        small = torch.rand(DIMS[gi], DIMS[gi], generator=torch.Generator().manual_seed(77)) < .5
        with torch.no_grad():
            cond.A.mul_(torch.where(small, torch.tensor(.2), torch.tensor(1.)))
        cond.invalidate_caches()
    return cond.to(DEV)


def run(cond, x, cot, fused, noise=None, x_grad=False, backward=True):
    """one forward (+ backward) of the conditioner through the fused or the composed front on the same Philox stream ->
    (h, A.grad, {parameter gradients}, x.grad, autograd node names)"""
    net = cond.embedding_net
    net.gated_front = fused
    cond.zero_grad(set_to_none=True)
    cond.gate_seed, cond._gate_calls, cond.gate_noise = 1234567, 40, noise
    xd = x.clone().requires_grad_(x_grad)
    assert net.supports_gated(xd) == fused
    h = cond(xd)
    nodes = graph_nodes(h)
    if backward and h.requires_grad:
        (h * cot).sum().backward()
    return (h.detach(), None if cond.A.grad is None else cond.A.grad.clone(),
            {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, xd.grad, nodes)


_pairs = {}


def both_paths(gi, B, gate):
    """composed reference and two fused runs of one case, computed once and shared by the tests below"""
    key = (gi, B, gate)
    if key not in _pairs:
        d = DIMS[gi]
        cond = make_conditioner(gi, gate)
        gen = torch.Generator().manual_seed(9000 + 10 * gi + B)
        x, cot = cu(torch.randn(B, d, generator=gen)), cu(torch.randn(B, d, 2, generator=gen))
        noise = None
        if GATES[gate][4]:
            noise = (cu(open_uniforms((B, d, d), gen)), cu(open_uniforms((B, d, d), gen)))
        _pairs[key] = (run(cond, x, cot, False, noise), run(cond, x, cot, True, noise), run(cond, x, cot, True, noise))
    return _pairs[key]


# ------------------------------------------------------------------------------------------- 1. forward bits
@pytest.mark.parametrize("gi,B,gate", CASES, ids=IDS)
def test_forward_bits_equal_the_composed_path(gi, B, gate):
    ref, got, _ = both_paths(gi, B, gate)
    assert "DagLenetFrontFnBackward" in got[4] and "DagLenetFrontFnBackward" not in ref[4]
    assert "DagGateFnBackward" in ref[4] and "DagGateFnBackward" not in got[4]
    assert got[0].shape == (B, DIMS[gi], 2)
    assert bool(torch.isfinite(ref[0]).all())
    assert torch.equal(got[0], ref[0])


# ------------------------------------------------------------------------------------------- 2. backward
@pytest.mark.parametrize("gi,B,gate", CASES, ids=IDS)
def test_backward_against_the_composed_path(gi, B, gate):
    ref, got, again = both_paths(gi, B, gate)
    assert float(ref[1].abs().max()) > 0
    assert_grad(got[1], ref[1], "gA")
    assert set(got[2]) == set(ref[2]) and len(ref[2]) == 10
    for n in ref[2]:
        assert_grad(got[2][n], ref[2][n], n)
    if gate == "h_thresh":
        zero = ref[1] == 0
        assert .25 < float(zero.float().mean()) < .75
        assert bool((got[1][zero] == 0).all())
    assert torch.equal(got[1], again[1])                       # the same call, the same bits
    for n in ref[2]:
        assert torch.equal(got[2][n], again[2][n]), n


# ------------------------------------------------------------------------------------------- 3. fp64, without the composed path
@pytest.mark.parametrize("stoch", [False, True], ids=["deterministic", "gumbel"])
@pytest.mark.parametrize("gi", [3, 2], ids=["d64", "d256"])
def test_against_fp64(gi, stoch):
    from models import DAGConditioner
    from models.MLP import CIFAR10CNN
    from oracle import gnf_oracle as O
    size_img, k, fc_l = GEOS[gi]
    d, B = DIMS[gi], 3
    torch.manual_seed(70 + gi)
    net = CIFAR10CNN(out_d=2, fc_l=list(fc_l), size_img=list(size_img), k_size=k)
    cond = DAGConditioner(d, net, 2)
    cond.stoch_gate = stoch
    p = {n: q.detach().cpu().clone() for n, q in net.named_parameters()}
    A = cond.A.detach().clone()
    gen = torch.Generator().manual_seed(700 + gi)
    u1 = u2 = None
    if stoch:
        u1, u2 = open_uniforms((B, d, d), gen), open_uniforms((B, d, d), gen)
    conv = [p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"]]
    for _ in range(6):                                        # x redrawn until at most 15 % of its copies hold a knife edge
        x = torch.randn(B, d, generator=gen)
        with torch.no_grad():
            e = O.dag_masked_inputs(x, A, True, 0., stoch, False, 1., u1, u2, None, False)
        knife = lenet_ref.knife_images(e, *conv, size_img)
        if float(knife.float().mean()) <= .15:
            break
    assert float(knife.float().mean()) <= .15, float(knife.float().mean())      # a condition, not a tolerance
    cot = torch.randn(B * d, 2, generator=gen) * (~knife).float().unsqueeze(1)  # knife copies: zero cotangent
    # the gate in fp32 as the reference evaluates it, the network in fp64 (tests/test_gpu_lenet.py::_cpu_conditioner)
    A64 = A.clone().requires_grad_(True)
    p64 = {n: v.double().requires_grad_(True) for n, v in p.items()}
    h0 = lenet_ref.cifar10cnn(O.dag_masked_inputs(x, A64, True, 0., stoch, False, 1., u1, u2, None, False).double(), p64,
                              size_img)
    names = list(p64)
    grads = torch.autograd.grad((h0 * cot.double()).sum(), [A64] + [p64[n] for n in names])
    cond = cond.to(DEV)
    h, gA, gp, _, nodes = run(cond, cu(x), cu(cot).view(B, d, 2), True, (cu(u1), cu(u2)) if stoch else None)
    assert "DagLenetFrontFnBackward" in nodes
    assert_fwd(h.reshape(B * d, 2), h0.detach(), what="h")
    assert_grad(gA, grads[0], "gA")
    for n, g0 in zip(names, grads[1:]):
        assert_grad(gp[n], g0, n)


# ------------------------------------------------------------------------------------------- 4. frozen operands
def _frozen_setup(gi=2, B=7):
    cond = make_conditioner(gi, "gumbel_T1")
    gen = torch.Generator().manual_seed(4100 + gi)
    return cond, cu(torch.randn(B, DIMS[gi], generator=gen)), cu(torch.randn(B, DIMS[gi], 2, generator=gen))


def test_frozen_A_still_gives_the_parameter_gradients():
    cond, x, cot = _frozen_setup()
    cond.A.requires_grad_(False)
    ref, got = run(cond, x, cot, False), run(cond, x, cot, True)
    assert "DagLenetFrontFnBackward" in got[4]
    assert torch.equal(got[0], ref[0])
    assert got[1] is None and ref[1] is None and len(got[2]) == 10
    for n in ref[2]:
        assert_grad(got[2][n], ref[2][n], n)


def test_x_requiring_grad_runs_the_composed_nodes():
    cond, x, cot = _frozen_setup()
    ref, got = run(cond, x, cot, False, x_grad=True), run(cond, x, cot, True, x_grad=True)
    assert "DagLenetFrontFnBackward" not in got[4] and "DagGateFnBackward" in got[4]
    assert torch.equal(got[0], ref[0]) and torch.equal(got[3], ref[3]) and torch.equal(got[1], ref[1])
    assert float(got[3].abs().max()) > 0


def test_no_grad_forward_bits():
    cond, x, cot = _frozen_setup()
    with torch.no_grad():
        ref, got = run(cond, x, cot, False, backward=False), run(cond, x, cot, True, backward=False)
        grad_x = run(cond, x, cot, True, x_grad=True, backward=False)      # no graph: the fused kernels, whatever x asks
    assert not ref[4] - {"NoneType"} and not got[4] - {"NoneType"}
    assert torch.equal(got[0], ref[0]) and torch.equal(grad_x[0], ref[0])


# ------------------------------------------------------------------------------------------- raw entry points
def raw_fwd(x, A, P, gi, B, feat=None, arg=True, tab=None, gate_mode=1, seed=11, offset=3):
    from gnf_hip import abi
    d = DIMS[gi]
    feat = torch.empty(B * d, FEAT[gi], device=DEV) if feat is None else feat
    arg = torch.empty(B * d, FEAT[gi], dtype=torch.uint8, device=DEV) if arg is True else arg
    tab = torch.empty(4 * d * d, device=DEV) if tab is None else tab
    abi.call("gnf_lenet_gated_fwd", abi.ptr(x), abi.ptr(A), abi.ptr(tab), *geo_args(gi), 1, gate_mode, 0., 1., None, None,
             seed, offset, *(abi.ptr(p) for p in P), abi.ptr(feat), abi.rawptr(arg) if arg is not None else None, B,
             abi.stream())
    return feat, arg, tab


def raw_bwd(x, tab, P, arg, gf, gi, B, gA=None, outs=None, accumulate=0, gate_mode=1, seed=11, offset=3):
    from gnf_hip import abi
    d = DIMS[gi]
    gA = torch.empty(d, d, device=DEV) if gA is None else gA
    outs = [torch.empty_like(p) for p in P] if outs is None else outs
    nws = abi.load().gnf_lenet_gated_bwd_ws_bytes(*geo_args(gi), B)
    ws = torch.empty(max(nws // 4, 1), device=DEV)
    abi.call("gnf_lenet_gated_bwd", abi.ptr(x), abi.ptr(tab), *geo_args(gi), 1, gate_mode, 1., None, None, seed, offset,
             *(abi.ptr(p) for p in P), abi.rawptr(arg) if arg is not None else None, abi.ptr(gf), abi.ptr(gA), accumulate,
             *(abi.ptr(o) for o in outs), abi.rawptr(ws), nws, B, abi.stream())
    return [gA] + outs


def _raw_operands(gi, B, seed):
    d = DIMS[gi]
    gen = torch.Generator().manual_seed(seed)
    P = [cu(p) for p in conv_params(gi, seed)]
    x = cu(torch.randn(B, d, generator=gen))
    A = cu(1.5 + .02 * torch.randn(d, d, generator=gen))
    gf = cu(torch.randn(B * d, FEAT[gi], generator=gen))
    return P, x, A, gf


# ------------------------------------------------------------------------------------------- 5. alignment
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("gi", [3, 2], ids=["d64", "d256"])
def test_dword_aligned_operands(gi, k):
    """x, A, g_feat, the conv parameters and every output 4 k bytes past a 16-byte boundary, between guard bands: the same
    bits as the aligned call"""
    B = 3
    P, x, A, gf = _raw_operands(gi, B, 500 + gi)
    feat0, arg0, tab0 = raw_fwd(x, A, P, gi, B)
    res0 = raw_bwd(x, tab0, P, arg0, gf, gi, B)
    recomputed = raw_bwd(x, tab0, P, None, gf, gi, B)          # argmax2 = NULL: conv2 recomputed, the same bits
    xm, Am, gfm, Pm = misaligned.place(x, k), misaligned.place(A, k), misaligned.place(gf, k), [misaligned.place(p, k) for p in P]
    featm = misaligned.place(torch.zeros_like(feat0), k)
    _, argm, tabm = raw_fwd(xm, Am, Pm, gi, B, feat=featm)
    assert torch.equal(featm, feat0) and torch.equal(argm, arg0) and torch.equal(tabm, tab0)
    outs = [misaligned.place(torch.zeros_like(p), k) for p in P]
    gAm = misaligned.place(torch.zeros_like(A), k)
    res = raw_bwd(xm, tabm, Pm, argm, gfm, gi, B, gA=gAm, outs=outs)
    for a, b, c in zip(res, res0, recomputed):
        assert torch.equal(a, b) and torch.equal(b, c)
    for t in [xm, Am, gfm, featm, gAm] + Pm + outs:
        assert misaligned.guards_intact(t)


# ------------------------------------------------------------------------------------------- 6. the C ABI
def test_symbols_declared_and_bound():
    from gnf_hip import abi
    header = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    for name in ("gnf_lenet_gated_fwd", "gnf_lenet_gated_bwd_ws_bytes", "gnf_lenet_gated_bwd"):
        assert name + "(" in header and name in abi.SIGNATURES
        assert hasattr(abi.load(), name)


def test_empty_batch_and_argument_errors():
    from gnf_hip import abi
    lib = abi.load()
    gi, d = 2, 256
    P, x, A, gf = _raw_operands(gi, 2, 600)
    p, s = abi.ptr, abi.stream()
    # B = 0: nothing is launched forward (the table stays as it was); backward: zero gradients, an accumulated gA untouched
    tab = torch.full((4 * d * d,), 7., device=DEV)
    feat, _, _ = raw_fwd(None, A, P, gi, 0, tab=tab)
    assert feat.shape == (0, 64) and bool((tab == 7.).all())
    outs = [torch.full_like(q, 7.) for q in P]
    gA = torch.full((d, d), 7., device=DEV)
    raw_bwd(None, None, P, None, None, gi, 0, gA=gA, outs=outs)
    assert all(float(o.abs().max()) == 0. for o in outs) and float(gA.abs().max()) == 0.
    gA.fill_(7.)
    raw_bwd(None, None, P, None, None, gi, 0, gA=gA, outs=outs, accumulate=1)
    assert bool((gA == 7.).all())
    # accumulate adds to what gA holds
    feat, arg, tab = raw_fwd(x, A, P, gi, 2)
    g0 = raw_bwd(x, tab, P, arg, gf, gi, 2)[0]
    g1 = raw_bwd(x, tab, P, arg, gf, gi, 2, gA=torch.full((d, d), .5, device=DEV), accumulate=1)[0]
    assert_close(g1, g0 + .5, rtol=1e-6, atol=1e-6 * float(g0.abs().max() + .5), what="accumulated gA")   # one rounding
    # return codes
    grads = [torch.empty_like(q) for q in P]
    gA = torch.empty(d, d, device=DEV)
    need = lib.gnf_lenet_gated_bwd_ws_bytes(1, 16, 16, 3, 2)
    ws = torch.empty(need // 4, device=DEV)

    def fwd(C, H, W, k, x_=x, A_=A, tab_=tab, W1=P[0], feat_=feat, gate=1, imp=1):
        return lib.gnf_lenet_gated_fwd(p(x_), p(A_), p(tab_), C, H, W, k, imp, gate, 0., 1., None, None, 1, 1, p(W1), p(P[1]),
                                       p(P[2]), p(P[3]), p(feat_), None, 2, s)

    def bwd(C, H, W, k, x_=x, tab_=tab, gf_=gf, gW1=grads[0], ws_=ws, ws_bytes=need, gA_=gA):
        return lib.gnf_lenet_gated_bwd(p(x_), p(tab_), C, H, W, k, 1, 1, 1., None, None, 1, 1, p(P[0]), p(P[1]), p(P[2]),
                                       p(P[3]), None, p(gf_), p(gA_), 0, p(gW1), p(grads[1]), p(grads[2]), p(grads[3]),
                                       abi.rawptr(ws_) if ws_ is not None else None, ws_bytes, 2, s)
    assert fwd(1, 16, 16, 3) == 0 and bwd(1, 16, 16, 3) == 0 and bwd(1, 16, 16, 3, gA_=None) == 0
    for bad in ((3, 28, 28, 5), (1, 32, 32, 4)):
        assert fwd(*bad) == -2 and bwd(*bad) == -2 and lib.gnf_lenet_gated_bwd_ws_bytes(*bad, 2) == -2     # GNF_ESHAPE
    for kw in ({"x_": None}, {"A_": None}, {"tab_": None}, {"W1": None}, {"feat_": None}, {"gate": 3}, {"imp": 4}):
        assert fwd(1, 16, 16, 3, **kw) == -1, kw                                                           # GNF_EINVAL
    for kw in ({"x_": None}, {"tab_": None}, {"gf_": None}, {"gW1": None}, {"ws_": None}):
        assert bwd(1, 16, 16, 3, **kw) == -1, kw
    assert need > 0 and bwd(1, 16, 16, 3, ws_bytes=need - 4) == -3                                          # GNF_EWS
    assert lib.gnf_lenet_gated_bwd_ws_bytes(1, 16, 16, 3, -1) == -1
    byte_off = ctypes.c_void_p(x.data_ptr() + 2)                                                           # below dword alignment
    assert lib.gnf_lenet_gated_fwd(byte_off, p(A), p(tab), 1, 16, 16, 3, 1, 1, 0., 1., None, None, 1, 1, p(P[0]), p(P[1]),
                                   p(P[2]), p(P[3]), p(feat), None, 2, s) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 7. memory
def test_peak_memory_without_the_masked_copies():
    """d = 3072, B = 8, forward + backward of the op: the fused node must peak at least 1.5 B d^2 floats below the composed
    nodes -- e and its cotangent are 2 B d^2, half of one is room for the per-chunk dL/dP rows of the fused backward"""
    from gnf_hip import ops
    gi, B, d = 0, 8, 3072
    P = [cu(p).requires_grad_(True) for p in conv_params(gi, 700)]
    gen = torch.Generator().manual_seed(701)
    x = cu(torch.randn(B, d, generator=gen))
    A = cu(1.5 + .02 * torch.randn(d, d, generator=gen)).requires_grad_(True)
    gf = cu(torch.randn(B * d, 400, generator=gen))

    def composed():
        e = ops.DagGateFn.apply(x, A, ops.IMP_SOFT, ops.GATE_GUMBEL, 0., 1., False, None, None, 5, 9)
        return ops.lenet_conv(e, *P, GEOS[gi][0], GEOS[gi][1])

    def fused():
        return ops.dag_lenet_front(x, A, ops.IMP_SOFT, ops.GATE_GUMBEL, 0., 1., None, None, 5, 9, *P, GEOS[gi][0], GEOS[gi][1])
    peak, grads = {}, {}
    for name, fn in (("composed", composed), ("fused", fused)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        g = torch.autograd.grad((fn() * gf).sum(), [A] + P)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        grads[name] = g[0]
        del g
    print("peak bytes above the operands:", peak, "B d^2 floats = %d bytes" % (B * d * d * 4))
    assert_grad(grads["fused"], grads["composed"], "gA")
    assert peak["composed"] - peak["fused"] >= 1.5 * B * d * d * 4, peak
    del grads
    torch.cuda.empty_cache()
