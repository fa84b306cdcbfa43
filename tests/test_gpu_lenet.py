"""GPU: the LeNet convolutional front of CIFAR10CNN (csrc/gnf_lenetcnn.hip) and everything built on it -- the C-ABI calls
against the reference fixture and an fp64 restatement (tests/lenet_ref.py), torch's tie rules, 64-bit row offsets, operand
alignment and argument checking, the module switch `fused_front`, the DAG conditioner at the four CIFAR sizes, the flows
buildCIFAR10NormalizingFlow builds, and the inverse of the multi-scale flow for the shapes that factory creates.

Tolerances are the project's: forward |a - b| <= 1e-6 max|b| + 1e-5 |b| per entry (assert_fwd);
gradients rel_err < 1e-4 of the tensor maximum and |a - b| <= 1e-6 max|g| + 1e-4 |b| per entry.  Knife-edge decisions
(lenet_ref.knife_images): independent images are redrawn until none is left; masked copies of one x get a zero cotangent
and their share is asserted to be at most 15 %."""
import ctypes

import pytest
import torch

from conftest import assert_fwd, load_golden, rel_err
import lenet_ref
from lenet_ref import DEV, assert_grad, cu, geo_args
import misaligned

pytestmark = pytest.mark.gpu
GEOS = lenet_ref.GEOMETRIES
FEAT = (400, 576, 64, 16)


def conv_params(gi, seed):
    """default-initialised convolutions of geometry gi (what CIFAR10CNN constructs), as CPU tensors"""
    size_img, k, _ = GEOS[gi]
    torch.manual_seed(seed)
    c1, c2 = torch.nn.Conv2d(size_img[0], 6, k), torch.nn.Conv2d(6, 16, k)
    return [t.detach().clone() for t in (c1.weight, c1.bias, c2.weight, c2.bias)]


def raw_fwd(e, P, gi, save=True):
    """gnf_lenet_conv_fwd on device tensors -> (feat, argmax2 or None)"""
    from gnf_hip import abi
    n = e.shape[0]
    feat = torch.empty(n, FEAT[gi], device=DEV)
    arg = torch.empty(n, FEAT[gi], dtype=torch.uint8, device=DEV) if save else None
    abi.call("gnf_lenet_conv_fwd", abi.ptr(e), e.stride(0), *geo_args(gi), *(abi.ptr(p) for p in P), abi.ptr(feat),
             abi.rawptr(arg) if save else None, n, abi.stream())
    return feat, arg


def raw_bwd(e, P, arg, gf, gi, want_ge=True, outs=None, ge=None):
    """gnf_lenet_conv_bwd -> (ge or None, gW1, gb1, gW2, gb2)"""
    from gnf_hip import abi
    n = e.shape[0]
    d = e.shape[1]
    if want_ge and ge is None:
        ge = torch.empty(n, d, device=DEV)
    outs = outs if outs is not None else [torch.empty_like(p) for p in P]
    nws = abi.load().gnf_lenet_conv_bwd_ws_bytes(*geo_args(gi), n)
    ws = torch.empty(max(nws // 4, 1), device=DEV)
    abi.call("gnf_lenet_conv_bwd", abi.ptr(e), e.stride(0), *geo_args(gi), *(abi.ptr(p) for p in P),
             abi.rawptr(arg) if arg is not None else None, abi.ptr(gf), abi.ptr(ge) if want_ge else None,
             ge.stride(0) if want_ge else d, *(abi.ptr(o) for o in outs), abi.rawptr(ws), nws, n, abi.stream())
    return (ge if want_ge else None, *outs)


def ref64(e, P, gf, gi):
    """fp64 front on the CPU: feat and the gradients of (feat * gf).sum() w.r.t. e and the four parameters"""
    e64 = e.double().requires_grad_(True)
    P64 = [p.double().requires_grad_(True) for p in P]
    feat = lenet_ref.front(e64, *P64, GEOS[gi][0])
    grads = torch.autograd.grad((feat * gf.double()).sum(), [e64] + P64)
    return feat.detach(), grads


# ------------------------------------------------------------------------------------------- 1. the reference fixture
@pytest.mark.parametrize("gi", range(4))
def test_module_against_reference_fixture(gi):
    from models.MLP import CIFAR10CNN
    g = load_golden("cifar10cnn")
    size_img, k, fc_l = GEOS[gi]
    tag = "g%d." % gi
    net = CIFAR10CNN(out_d=2, fc_l=list(fc_l), size_img=list(size_img), k_size=k)
    net.load_state_dict({n[len(tag) + 2:]: v for n, v in g.items() if n.startswith(tag + "p.")})
    net = net.to(DEV)
    x = cu(g[tag + "x"]).requires_grad_(True)
    assert net._fused_front(x)
    out = net(x)
    (out * cu(g[tag + "g"])).sum().backward()
    assert_fwd(out, g[tag + "out"], what="out")
    assert_grad(x.grad, g[tag + "gx"], "gx")
    for n, p in net.named_parameters():
        assert_grad(p.grad, g[tag + "g." + n], n)


# ------------------------------------------------------------------------------------------- 2. fp64 restatement
@pytest.mark.parametrize("n", [1, 2, 65, 257])
@pytest.mark.parametrize("gi", range(4))
def test_kernels_against_fp64(gi, n):
    P = conv_params(gi, 10 + gi)
    gen = torch.Generator().manual_seed(1000 * gi + n)
    e, left = lenet_ref.draw_clean_images(n, GEOS[gi][0], *P, gen)
    assert left == 0                                   # redrawn, not excluded: none may be left after 6 rounds
    gf = torch.randn(n, FEAT[gi], generator=gen)
    feat0, (ge0, *gP0) = ref64(e, P, gf, gi)
    ed, Pd, gfd = cu(e), [cu(p) for p in P], cu(gf)
    feat, arg = raw_fwd(ed, Pd, gi)
    assert_fwd(feat, feat0, what="feat")
    feat_b, _ = raw_fwd(ed, Pd, gi, save=False)
    assert torch.equal(feat, feat_b)
    res = raw_bwd(ed, Pd, arg, gfd, gi)
    for got, want, what in zip(res, [ge0] + gP0, ("ge", "gW1", "gb1", "gW2", "gb2")):
        assert_grad(got, want, what)
    again = raw_bwd(ed, Pd, arg, gfd, gi)                         # same operands, same bits
    no_ge = raw_bwd(ed, Pd, arg, gfd, gi, want_ge=False)          # ge = NULL: parameter gradients unchanged bit for bit
    recomputed = raw_bwd(ed, Pd, None, gfd, gi)                   # argmax2 = NULL: conv2 recomputed, the same bits
    for k in range(5):
        assert torch.equal(res[k], again[k]) and torch.equal(res[k], recomputed[k])
        if k:
            assert torch.equal(res[k], no_ge[k])


# ------------------------------------------------------------------------------------------- 3. exact ties
@pytest.mark.parametrize("gi", range(4))
def test_exact_ties_follow_torch(gi):
    """an all-zero image, an all-equal image, an image that is zero outside one 5 x 5 patch: every pool window of the
    constant regions is an exact tie, and a wrong tie rule moves O(1) of the gradient.  Reference: torch CPU fp32 autograd."""
    size_img, k, _ = GEOS[gi]
    c, h, w = size_img
    P = conv_params(gi, 20 + gi)
    gen = torch.Generator().manual_seed(300 + gi)
    e = torch.zeros(3, c, h, w)
    e[1] = .75
    e[2, :, 1:6, 2:7] = torch.randn(c, 5, 5, generator=gen)
    e = e.reshape(3, -1)
    gf = torch.randn(3, FEAT[gi], generator=gen)
    e32 = e.clone().requires_grad_(True)
    P32 = [p.clone().requires_grad_(True) for p in P]
    feat0 = lenet_ref.front(e32, *P32, size_img)
    want = torch.autograd.grad((feat0 * gf).sum(), [e32] + P32)
    ed, Pd = cu(e), [cu(p) for p in P]
    feat, arg = raw_fwd(ed, Pd, gi)
    assert_fwd(feat, feat0.detach(), what="feat")
    res = raw_bwd(ed, Pd, arg, cu(gf), gi)
    for got, ref, what in zip(res, want, ("ge", "gW1", "gb1", "gW2", "gb2")):
        assert_grad(got, ref, what)


# ------------------------------------------------------------------------------------------- 4. offsets beyond 2^32 bytes
def test_row_offsets_beyond_4gb():
    gi, n, blk = 0, 349600, 64                          # 349 600 rows of 3072 floats: 4.3 GB
    P = [cu(p) for p in conv_params(gi, 30)]
    gen = torch.Generator().manual_seed(31)
    e = cu(torch.randn(blk, 3072, generator=gen)).repeat((n + blk - 1) // blk, 1)[:n].contiguous()
    gf = cu(torch.randn(blk, 400, generator=gen)).repeat((n + blk - 1) // blk, 1)[:n].contiguous()
    assert e.numel() * 4 > 2 ** 32
    feat, arg = raw_fwd(e, P, gi)
    full = n // blk
    assert bool((feat[:full * blk].view(full, blk, 400) == feat[:blk]).all())
    assert torch.equal(feat[full * blk:], feat[:n - full * blk])
    ge = raw_bwd(e, P, arg, gf, gi)[0]
    rows = torch.arange(n - blk, n, device=DEV)        # the last 64 rows: every one of them starts beyond 2^32 bytes
    assert (n - blk) * 3072 * 4 > 2 ** 32
    assert torch.equal(ge[rows], ge[rows % blk])
    del e, ge, gf, feat
    torch.cuda.empty_cache()


def test_grid_stride_over_groups_of_several_images():
    """(1,8,8,2) holds 28 images per group; n = 28 * 1024 + 5 is more groups than either grid has workgroups (1024
    forward, 512 backward), the last of them partly filled, so every workgroup strides on to a second or third group.
    feat, the pool decisions and ge are per-image quantities: the bits of the same entry points on consecutive slices of
    at most 28 * 512 images, which no workgroup strides over.  The parameter gradients are sums over the images in another
    order: the fp64 sum of the slices' gradients, under assert_grad."""
    gi, ipb = 3, 28
    n, step = ipb * 1024 + 5, ipb * 512
    P = [cu(p) for p in conv_params(gi, 35)]
    gen = torch.Generator().manual_seed(36)
    e, gf = cu(torch.randn(n, 64, generator=gen)), cu(torch.randn(n, FEAT[gi], generator=gen))
    feat, arg = raw_fwd(e, P, gi)
    res = raw_bwd(e, P, arg, gf, gi)
    feat_b, arg_b = raw_fwd(e, P, gi)                               # same operands, same bits
    assert torch.equal(feat, feat_b) and torch.equal(arg, arg_b)
    for a, b in zip(res, raw_bwd(e, P, arg, gf, gi)):
        assert torch.equal(a, b)
    sums = [torch.zeros_like(p, dtype=torch.float64) for p in P]
    for i0 in range(0, n, step):
        sl = slice(i0, min(i0 + step, n))
        feat_s, arg_s = raw_fwd(e[sl], P, gi)
        assert torch.equal(feat[sl], feat_s) and torch.equal(arg[sl], arg_s)
        ge_s, *gP_s = raw_bwd(e[sl], P, arg_s, gf[sl], gi)
        assert torch.equal(res[0][sl], ge_s)
        for acc, g in zip(sums, gP_s):
            acc += g.double()
    for got, want, what in zip(res[1:], sums, ("gW1", "gb1", "gW2", "gb2")):
        assert_grad(got, want, what)


# ------------------------------------------------------------------------------------------- 5. edge cases
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("gi", range(4))
def test_dword_aligned_operands(gi, k):
    """every operand 4 k bytes past a 16-byte boundary, between guard bands: the same bits as the aligned call"""
    n = 3
    P = [cu(p) for p in conv_params(gi, 40 + gi)]
    gen = torch.Generator().manual_seed(400 + gi)
    d = GEOS[gi][0][0] * GEOS[gi][0][1] * GEOS[gi][0][2]
    e, gf = cu(torch.randn(n, d, generator=gen)), cu(torch.randn(n, FEAT[gi], generator=gen))
    feat0, arg0 = raw_fwd(e, P, gi)
    res0 = raw_bwd(e, P, arg0, gf, gi)
    from gnf_hip import abi
    em, gfm, Pm = misaligned.place(e, k), misaligned.place(gf, k), [misaligned.place(p, k) for p in P]
    featm = misaligned.place(torch.zeros_like(feat0), k)
    abi.call("gnf_lenet_conv_fwd", abi.ptr(em), em.stride(0), *geo_args(gi), *(abi.ptr(p) for p in Pm), abi.ptr(featm),
             abi.rawptr(arg0), n, abi.stream())
    assert torch.equal(featm, feat0)
    outs = [misaligned.place(torch.zeros_like(p), k) for p in P]
    gem = misaligned.place(torch.zeros_like(e), k)
    res = raw_bwd(em, Pm, arg0, gfm, gi, outs=outs, ge=gem)
    for a, b in zip(res, res0):
        assert torch.equal(a, b)
    for t in [em, gfm, featm, gem] + Pm + outs:
        assert misaligned.guards_intact(t)


def test_empty_batch_shape_and_argument_errors():
    from gnf_hip import abi
    lib = abi.load()
    gi = 2
    P = [cu(p) for p in conv_params(gi, 50)]
    # n = 0: forward returns 0 without touching anything, backward writes zero parameter gradients
    e0, gf0 = torch.empty(0, 256, device=DEV), torch.empty(0, 64, device=DEV)
    feat, _ = raw_fwd(e0, P, gi)
    assert feat.shape == (0, 64)
    outs = [torch.full_like(p, 7.) for p in P]
    raw_bwd(e0, P, None, gf0, gi, outs=outs)
    assert all(float(o.abs().max()) == 0. for o in outs)
    # the rest through the raw entry points: return codes
    e, gf = torch.randn(2, 256, device=DEV), torch.randn(2, 64, device=DEV)
    feat, ge = torch.empty(2, 64, device=DEV), torch.empty(2, 256, device=DEV)
    grads = [torch.empty_like(p) for p in P]
    ws = torch.empty(1 << 16, device=DEV)
    p = abi.ptr
    s = abi.stream()

    def fwd(C, H, W, k, e_=e, W1=P[0], feat_=feat):
        return lib.gnf_lenet_conv_fwd(p(e_), 256, C, H, W, k, p(W1), p(P[1]), p(P[2]), p(P[3]), p(feat_), None, 2, s)

    def bwd(C, H, W, k, gf_=gf, gW1=grads[0], ws_=ws, ws_bytes=ws.numel() * 4):
        return lib.gnf_lenet_conv_bwd(p(e), 256, C, H, W, k, p(P[0]), p(P[1]), p(P[2]), p(P[3]), None, p(gf_), p(ge), 256,
                                      p(gW1), p(grads[1]), p(grads[2]), p(grads[3]), abi.rawptr(ws_) if ws_ is not None else None,
                                      ws_bytes, 2, s)
    assert fwd(1, 16, 16, 3) == 0 and bwd(1, 16, 16, 3) == 0
    for bad in ((3, 28, 28, 5), (1, 32, 32, 4)):
        assert fwd(*bad) == -2 and bwd(*bad) == -2                          # GNF_ESHAPE
        assert lib.gnf_lenet_conv_bwd_ws_bytes(*bad, 2) == -2
    assert fwd(1, 16, 16, 3, e_=None) == -1 and fwd(1, 16, 16, 3, W1=None) == -1 and fwd(1, 16, 16, 3, feat_=None) == -1
    assert bwd(1, 16, 16, 3, gf_=None) == -1 and bwd(1, 16, 16, 3, gW1=None) == -1 and bwd(1, 16, 16, 3, ws_=None) == -1
    need = lib.gnf_lenet_conv_bwd_ws_bytes(1, 16, 16, 3, 2)
    assert need > 0 and bwd(1, 16, 16, 3, ws_bytes=need - 4) == -3          # GNF_EWS
    assert bwd(1, 16, 16, 3, ws_bytes=need) == 0
    byte_off = ctypes.c_void_p(e.data_ptr() + 2)                            # below dword alignment
    assert lib.gnf_lenet_conv_fwd(byte_off, 256, 1, 16, 16, 3, p(P[0]), p(P[1]), p(P[2]), p(P[3]), p(feat), None, 1, s) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 6. the module switch
@pytest.mark.parametrize("gi", range(4))
def test_module_fused_front_against_torch_path(gi):
    from models.MLP import CIFAR10CNN
    size_img, k, fc_l = GEOS[gi]
    torch.manual_seed(60 + gi)
    net = CIFAR10CNN(out_d=2, fc_l=list(fc_l), size_img=list(size_img), k_size=k)
    P = [t.detach() for t in (net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv2.bias)]
    x, left = lenet_ref.draw_clean_images(5, size_img, *P, torch.Generator().manual_seed(600 + gi))
    assert left == 0
    net = net.to(DEV)
    g = torch.randn(5, 2, generator=torch.Generator().manual_seed(6)).to(DEV)
    got = {}
    for fused in (False, True):
        net.fused_front = fused
        net.zero_grad()
        xd = cu(x).requires_grad_(True)
        assert net._fused_front(xd) == fused
        out = net(xd)
        (out * g).sum().backward()
        got[fused] = (out.detach(), xd.grad, {n: p.grad.clone() for n, p in net.named_parameters()})
    assert_fwd(got[True][0], got[False][0].cpu(), what="out")
    assert_grad(got[True][1], got[False][1].cpu(), "gx")
    for n in got[True][2]:
        assert_grad(got[True][2][n], got[False][2][n].cpu(), n)


def test_saved_and_recomputed_pool_decisions_agree(monkeypatch):
    """GNF_LENET_SAVE_ARGMAX=0 (the A/B switch of tools/bench_lenet_front.py): the autograd node keeps no decision plane and
    the backward recomputes conv2 -- the same bits"""
    from gnf_hip import ops
    gi = 1
    P = [cu(p).requires_grad_(True) for p in conv_params(gi, 65)]
    x = cu(torch.randn(9, 1024, generator=torch.Generator().manual_seed(650))).requires_grad_(True)
    g = cu(torch.randn(9, 576, generator=torch.Generator().manual_seed(651)))
    got = []
    for save in ("1", "0"):
        monkeypatch.setenv("GNF_LENET_SAVE_ARGMAX", save)
        feat = ops.lenet_conv(x, *P, GEOS[gi][0], GEOS[gi][1])
        assert (feat.grad_fn.arg is not None) == (save == "1")
        got.append(torch.autograd.grad((feat * g).sum(), [x] + P))
    for a, b in zip(*got):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------- 7. the conditioner
def open_uniforms(shape, gen):
    """injected gate noise in the OPEN interval (0, 1).  torch.rand returns an exact 0 with probability 2^-24 per element
    -- about one per 9.4 M-element tensor at d = 3072 -- and at u2 == 0 exactly the injected-noise form of the gate kernel
    (gnf_dag_gate.hip, a test hook; untouched here) does not return the reference's limit gate = 1: measured on the first
    version of these tests, every masked copy that missed the tolerance (h off by 5e-2 relative) held such an element and
    no other copy missed.  The kernels under test here never see the difference; the endpoint is left to the gate's own
    tests."""
    return torch.rand(shape, generator=gen).clamp_(min=2. ** -24)


def _net_params(net):
    return {n: p.detach().cpu().clone() for n, p in net.named_parameters()}


def _cpu_conditioner(x, A, p, size_img, stoch, u1, u2, cot):
    """h = CIFAR10CNN(e), e = the oracle's masked copies of x; gradients of (h * cot).sum() w.r.t. A, x and p"""
    from oracle import gnf_oracle as O
    x = x.clone().requires_grad_(True)
    A = A.clone().requires_grad_(True)
    p = {n: v.double().requires_grad_(True) for n, v in p.items()}
    # the gate in fp32, as the reference evaluates it: log(u + 1e-6) of a uniform within 1e-6 of 1 is decided by the fp32
    # rounding of that sum, and an fp64 gate differs by O(1) on a handful of the 9.4 M elements; the network in fp64
    e = O.dag_masked_inputs(x, A, True, 0., stoch, False, 1., u1, u2, None, False)
    h = lenet_ref.cifar10cnn(e.double(), p, size_img)
    names = list(p)
    grads = torch.autograd.grad((h * cot.double()).sum(), [A, x] + [p[n] for n in names])
    return h.detach(), grads[0], grads[1], dict(zip(names, grads[2:]))


@pytest.mark.parametrize("stoch", [False, True], ids=["deterministic", "gumbel"])
@pytest.mark.parametrize("gi", [3, 2, 1, 0], ids=["d64", "d256", "d1024", "d3072"])
def test_conditioner_at_the_cifar_sizes(gi, stoch):
    from models import DAGConditioner
    from models.MLP import CIFAR10CNN
    from oracle import gnf_oracle as O
    size_img, k, fc_l = GEOS[gi]
    d = size_img[0] * size_img[1] * size_img[2]
    torch.manual_seed(70 + gi)
    net = CIFAR10CNN(out_d=2, fc_l=list(fc_l), size_img=list(size_img), k_size=k)
    cond = DAGConditioner(d, net, 2)
    cond.stoch_gate = stoch
    p, A = _net_params(net), cond.A.detach().clone()
    gen = torch.Generator().manual_seed(700 + gi)
    u1 = u2 = None
    if stoch:
        u1, u2 = open_uniforms((1, d, d), gen), open_uniforms((1, d, d), gen)
    conv = [p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"]]
    # x is drawn on the CPU, before any GPU work, until at most 15 % of its masked copies hold a knife-edge decision
    for _ in range(6):
        x = torch.randn(1, d, generator=gen)
        with torch.no_grad():
            e = O.dag_masked_inputs(x, A, True, 0., stoch, False, 1., u1, u2, None, False)
        knife = lenet_ref.knife_images(e, *conv, size_img)
        if float(knife.float().mean()) <= .15:
            break
    assert float(knife.float().mean()) <= .15, float(knife.float().mean())      # a condition, not a tolerance
    cot = torch.randn(d, 2, generator=gen) * (~knife).float().unsqueeze(1)       # knife copies: zero cotangent
    h0, gA0, gx0, gp0 = _cpu_conditioner(x, A, p, size_img, stoch, u1, u2, cot)
    cond = cond.to(DEV)
    if stoch:
        cond.gate_noise = (cu(u1), cu(u2))
    xd = cu(x).requires_grad_(True)
    h = cond(xd)
    assert h.shape == (1, d, 2)
    assert_fwd(h.reshape(d, 2), h0, what="h")
    (h.reshape(d, 2) * cu(cot)).sum().backward()
    assert_grad(cond.A.grad, gA0, "gA")
    assert_grad(xd.grad, gx0, "gx")
    for n, q in cond.embedding_net.named_parameters():
        assert_grad(q.grad, gp0[n], n)


# ------------------------------------------------------------------------------------------- 8. the flows
def test_affine_one_scale_flow():
    from models import AffineNormalizer
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow
    from oracle import gnf_oracle as O
    torch.manual_seed(80)
    flow = buildCIFAR10NormalizingFlow([1], AffineNormalizer, {})
    cond = flow.steps[0].conditioner
    p, A = _net_params(cond.embedding_net), cond.A.detach().clone()
    gen = torch.Generator().manual_seed(800)
    B, d = 2, 3072
    x = torch.randn(B, d, generator=gen)
    u1, u2 = open_uniforms((B, d, d), gen), open_uniforms((B, d, d), gen)
    with torch.no_grad():                                    # the CPU composition: fp32 gate (see _cpu_conditioner), the rest fp64
        e = O.dag_masked_inputs(x, A, True, 0., True, False, 1., u1, u2, None, False).double()
        h0 = lenet_ref.cifar10cnn(e, {n: v.double() for n, v in p.items()}, (3, 32, 32)).view(B, d, 2)
        z0, jac0 = O.affine_forward(x.double(), h0)
        ld0 = torch.log(jac0).sum(1)
        nll0 = -(ld0 + O.normal_log_density(z0)).mean()
    flow = flow.to(DEV)
    cond.gate_noise = (cu(u1), cu(u2))
    with torch.no_grad():
        z, ld = flow(cu(x))
        nll = -(ld + flow.z_log_density(z)).mean()
    assert z.shape == (B, d) and ld.shape == (B,)
    assert_fwd(z, z0, what="z")
    assert_fwd(ld, ld0, what="logdet")
    assert_fwd(nll.reshape(1), nll0.reshape(1), what="nll")


def test_monotonic_one_scale_flow():
    from models import MonotonicNormalizer
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow
    from oracle import gnf_oracle as O
    torch.manual_seed(81)
    S = 20
    flow = buildCIFAR10NormalizingFlow([1], MonotonicNormalizer, {"integrand_net": [50, 50, 50], "cond_size": 30,
                                                                 "nb_steps": S, "solver": "CC"})
    step = flow.steps[0]
    cond = step.conditioner
    assert cond.embedding_net.out_d == 30
    p, A = _net_params(cond.embedding_net), cond.A.detach().clone()
    sd = step.normalizer.state_dict()
    layers = [(sd["integrand_net.net.%d.weight" % i].detach().double().cpu(),
               sd["integrand_net.net.%d.bias" % i].detach().double().cpu()) for i in (0, 2, 4, 6)]
    gen = torch.Generator().manual_seed(810)
    d = 3072
    x = torch.randn(1, d, generator=gen)
    u1, u2 = open_uniforms((1, d, d), gen), open_uniforms((1, d, d), gen)
    with torch.no_grad():                                    # the CPU composition: fp32 gate (see _cpu_conditioner), the rest fp64
        e = O.dag_masked_inputs(x, A, True, 0., True, False, 1., u1, u2, None, False).double()
        h0 = lenet_ref.cifar10cnn(e, {n: v.double() for n, v in p.items()}, (3, 32, 32)).view(1, d, 30)
    z0, jac0 = O.monotonic_forward(x.double(), h0, layers, S)
    flow = flow.to(DEV)
    cond.gate_noise = (cu(u1), cu(u2))
    xd = cu(x)
    h = cond(xd)
    z, jac = step.normalizer(xd, h)
    assert_fwd(h, h0, what="h")
    assert_fwd(z, z0.detach(), what="z")
    assert_fwd(jac, jac0.detach(), what="jac")
    zz, ld = flow(xd)
    loss = flow.loss(zz, ld)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for n, q in flow.named_parameters():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), n


def test_four_scale_flow_forward():
    from models import AffineNormalizer
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow
    torch.manual_seed(82)
    flow = buildCIFAR10NormalizingFlow([1, 1, 1, 1], AffineNormalizer, {}).to(DEV)
    for c in flow.getConditioners():
        c.stoch_gate = False                           # deterministic gates: the scales can be re-run one by one
    x = cu(torch.randn(1, 3072, generator=torch.Generator().manual_seed(820)))
    z, ld = flow(x)
    assert z.shape == (1, 3072) and ld.shape == (1,) and bool(torch.isfinite(z).all())
    # the log-det is the sum over the THREE active scales, each fed the kept block of the one before
    total, xk = 0., x
    with torch.no_grad():
        for scale, drop in zip(flow.steps[:3], flow.dropping_factors):
            zk, ldk = scale(xk)
            total = total + ldk
            xk = flow._blocks(zk, scale.img_sizes, drop)[..., 0].reshape(1, -1)
    assert_fwd(ld, total.cpu(), what="logdet")
    assert xk.shape == (1, 64) and torch.equal(z[:, -64:], xk)
    (ld.sum() + (z ** 2).sum()).backward()
    assert all(q.grad is None for q in flow.steps[3].parameters())          # the fourth flow is never used
    assert all(q.grad is not None for k in range(3) for q in flow.steps[k].parameters())


# ------------------------------------------------------------------------------------------- 9. CNNormalizingFlow.invert
def _scale(img_size, seed):
    """two Affine + Autoregressive steps on one image scale"""
    from models import AffineNormalizer, AutoregressiveConditioner
    from models.NormalizingFlow import FCNormalizingFlow, NormalizingFlowStep
    torch.manual_seed(seed)
    d = img_size[0] * img_size[1] * img_size[2]
    steps = [NormalizingFlowStep(AutoregressiveConditioner(d, [24, 24], 2), AffineNormalizer()) for _ in range(2)]
    flow = FCNormalizingFlow(steps, None)
    flow.img_sizes = img_size
    return flow


@pytest.mark.parametrize("case", ["three_flows_two_factors", "two_flows_last_factor_drops"])
def test_cnn_flow_invert_round_trip(case):
    from models.NormalizingFlow import CNNormalizingFlow
    from models.NormalizingFlowFactories import NormalLogDensity
    if case == "three_flows_two_factors":                  # the third flow is never used, the second scale still drops
        scales = [_scale([1, 4, 4], 90), _scale([1, 2, 2], 91), _scale([1, 1, 1], 92)]
        drops = [[1, 2, 2], [1, 2, 2]]
    else:
        scales = [_scale([1, 4, 4], 93), _scale([1, 2, 2], 94)]
        drops = [[1, 2, 2], [1, 2, 2]]
    flow = CNNormalizingFlow(scales, NormalLogDensity(), drops).to(DEV)
    x = cu(torch.randn(7, 16, generator=torch.Generator().manual_seed(95)))
    with torch.no_grad():
        z, _ = flow(x)
        back = flow.invert(z)
    assert z.shape == (7, 16)
    assert rel_err(back.cpu(), x.cpu()) < 1e-4             # the tolerance of test_multi_step_inverse_round_trip
