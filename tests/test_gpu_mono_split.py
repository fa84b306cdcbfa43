"""GPU: the Monotonic forward and backward of WIDE integrand nets on the bf16 matrix pipe (mono_fwd_wide_split_k, the chain
wavefronts of mono_bwd_wide_k<split>: exact 3 x bf16 operand splits, six cross terms, fp32 accumulate) against an fp64 evaluation of the reference's arithmetic
(models/Normalizers/MonotonicNormalizer.py:21-66; the Clenshaw-Curtis rule as the kernels receive it) and against the fp32-MFMA
kernel it replaces (gnf_monotonic_fwd_f32 = what GNF_TRUE_F32=1 runs).  Adoption criterion, as for the fc1 products
(tests/test_gpu_split.py): the split kernel's error against fp64 is not larger than the fp32-MFMA kernel's."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _params(hidden, c, seed, scale=1.):
    g = torch.Generator().manual_seed(seed)
    dims = [1 + c] + list(hidden) + [1]
    ps = []
    for i in range(len(dims) - 1):
        bound = scale / dims[i] ** .5
        ps.append(((torch.rand(dims[i + 1], dims[i], generator=g) * 2 - 1) * bound * 1.7).to(DEV))
        ps.append(((torch.rand(dims[i + 1], generator=g) * 2 - 1) * bound).to(DEV))
    return ps


def _fwd(entry, params, x, h, S):
    from gnf_hip import abi, ops
    from gnf_hip.abi import call, ptr, stream
    net = ops._mono_net(params)
    pack = ops._mono_pack(net, x)
    w, t = ops.cc_rule(S, x.device)
    z, jac = torch.empty_like(x), torch.empty_like(x)
    call(entry, ptr(pack), ctypes.byref(net), ptr(x), ptr(h), h.stride(0), h.stride(1), h.stride(2), ptr(w), ptr(t), int(S),
         ptr(z), ptr(jac), x.shape[0], x.shape[1], stream())
    return z, jac, abi.load().gnf_monotonic_fwd_kernel().decode()


def _fp64(params, x, h, S):
    """the same quadrature in fp64 (weights / nodes = the fp32 rule the kernels receive, promoted)"""
    from gnf_hip import ops
    w, t = ops.cc_rule(S, x.device)
    w, t = w.double(), t.double()
    P = [p.double() for p in params]
    xd, hd = x.double(), h.double()
    fS = torch.tensor(float(S), dtype=torch.float32, device=x.device)
    xT = (fS * (x / fS)).double()                      # xT is formed in fp32 by the reference (x0 + nb_steps * step)

    def f(tt):                                         # tt [B, d, K]
        a = torch.cat([tt.unsqueeze(-1), hd.unsqueeze(2).expand(-1, -1, tt.shape[2], -1)], -1)
        for k in range(0, len(P), 2):
            a = a @ P[k].t() + P[k + 1]
            if k + 2 < len(P):
                a = torch.relu(a)
        a = a[..., 0]
        return torch.where(a > 0, a, torch.expm1(torch.clamp(a, max=0.))) + 1.05
    nodes = xT.unsqueeze(-1) * (t + 1.) / 2.
    z = (f(nodes) * w).sum(-1) * xT / 2. + hd[..., 0]
    jac = f(xd.unsqueeze(-1))[..., 0]
    return z, jac


CASES = [([100, 100, 100], 30, 6, 700, 20), ([150, 150, 150], 30, 9, 300, 20), ([160, 160], 8, 5, 333, 9), ([112] * 4, 30, 3, 257, 20),
         ([97, 105, 112], 17, 4, 129, 15), ([145, 160, 150], 30, 7, 64, 150), ([150, 150, 150], 30, 63, 50, 250)]


@pytest.mark.parametrize("hidden,c,d,B,S", CASES)
def test_split_forward_vs_fp64_and_fp32_mfma(hidden, c, d, B, S):
    from gnf_hip import abi
    if not abi.load().gnf_gemm_split_enabled():
        pytest.skip("GNF_TRUE_F32=1")
    params = _params(hidden, c, seed=sum(hidden) + S, scale=1.3)
    g = torch.Generator().manual_seed(B)
    x = (torch.randn(B, d, generator=g) * 2.).to(DEV)
    h = torch.randn(B, d, c, generator=g).to(DEV)
    zs, js, ks = _fwd("gnf_monotonic_fwd", params, x, h, S)
    zf, jf, kf = _fwd("gnf_monotonic_fwd_f32", params, x, h, S)
    assert ks == "mono_fwd_wide_split_k" and kf == "mono_fwd_wide_k", (ks, kf)
    z64, j64 = _fp64(params, x, h, S)

    def errs(a, ref):
        e = (a.double() - ref).abs()
        return float(e.max() / ref.abs().max()), float((e.pow(2).mean() / ref.pow(2).mean()).sqrt())
    ez_s, ez_f, ej_s, ej_f = errs(zs, z64), errs(zf, z64), errs(js, j64), errs(jf, j64)
    print("\n[mono split %s S=%d] z: split max %.2e rms %.2e | fp32-MFMA max %.2e rms %.2e;  jac: split max %.2e rms %.2e | fp32-MFMA max %.2e rms %.2e"
          % (hidden, S, *ez_s, *ez_f, *ej_s, *ej_f))
    # the split kernel is as close to fp64 as the kernel it replaces.  Both sit at the roundoff of the fp32 parts they share
    # (layer 1, the last layer's dot product, the quadrature sum: ~1e-7 of the result), so "not larger" is asked up to a quarter
    # of the fp32 kernel's own error plus a fraction of one fp32 epsilon (1.2e-7)
    assert ez_s[1] <= 1.25 * ez_f[1] + 2e-8 and ej_s[1] <= 1.25 * ej_f[1] + 2e-8, (ez_s, ez_f, ej_s, ej_f)
    assert ez_s[0] <= 1.5 * ez_f[0] + 1.2e-7 and ej_s[0] <= 1.5 * ej_f[0] + 1.2e-7, (ez_s, ez_f, ej_s, ej_f)
    assert ez_s[0] < 2e-6 and ej_s[0] < 2e-6, (ez_s, ej_s)
    # deterministic
    zs2, js2, _ = _fwd("gnf_monotonic_fwd", params, x, h, S)
    assert torch.equal(zs, zs2) and torch.equal(js, js2)


NCASES = [([50, 50, 50], 30, 784, 12, 20), ([50, 50, 50], 30, 784, 3, 150), ([49, 49], 8, 5, 333, 9), ([51] * 3, 30, 3, 257, 20),
          ([50, 50, 50], 30, 1, 1, 20), ([50, 50, 50], 5, 7, 19, 21)]


@pytest.mark.parametrize("hidden,c,d,B,S", NCASES)
def test_narrow_split_forward_vs_fp64_and_fp32_mfma(hidden, c, d, B, S):
    """the peeled narrow nets (H = 49..51: the reference's default integrand net, cfg4): mono_fwd_x_k<split>"""
    from gnf_hip import abi
    if not abi.load().gnf_gemm_split_enabled():
        pytest.skip("GNF_TRUE_F32=1")
    params = _params(hidden, c, seed=sum(hidden) + S + 3, scale=1.3)
    g = torch.Generator().manual_seed(B + 5)
    x = (torch.randn(B, d, generator=g) * 2.).to(DEV)
    h = torch.randn(B, d, c, generator=g).to(DEV)
    zs, js, ks = _fwd("gnf_monotonic_fwd", params, x, h, S)
    zf, jf, kf = _fwd("gnf_monotonic_fwd_f32", params, x, h, S)
    assert ks == "mono_fwd_x_k<split>" and kf == "mono_fwd_k", (ks, kf)
    z64, j64 = _fp64(params, x, h, S)

    def errs(a, ref):
        e = (a.double() - ref).abs()
        return float(e.max() / ref.abs().max()), float((e.pow(2).mean() / ref.pow(2).mean()).sqrt())
    ez_s, ez_f, ej_s, ej_f = errs(zs, z64), errs(zf, z64), errs(js, j64), errs(jf, j64)
    print("\n[mono narrow split %s S=%d] z: split max %.2e rms %.2e | fp32-MFMA max %.2e rms %.2e;  jac: split max %.2e rms %.2e | fp32-MFMA max %.2e rms %.2e"
          % (hidden, S, *ez_s, *ez_f, *ej_s, *ej_f))
    assert ez_s[1] <= 1.25 * ez_f[1] + 2e-8 and ej_s[1] <= 1.25 * ej_f[1] + 2e-8, (ez_s, ez_f, ej_s, ej_f)
    assert ez_s[0] <= 1.5 * ez_f[0] + 1.2e-7 and ej_s[0] <= 1.5 * ej_f[0] + 1.2e-7, (ez_s, ez_f, ej_s, ej_f)
    assert ez_s[0] < 2e-6 and ej_s[0] < 2e-6, (ez_s, ej_s)
    zs2, js2, _ = _fwd("gnf_monotonic_fwd", params, x, h, S)
    assert torch.equal(zs, zs2) and torch.equal(js, js2)


def test_narrow_split_declines_what_does_not_fit_two_workgroups_per_cu():
    """four hidden layers: the fp32 image + three matrices' planes exceed half the LDS -- the fp32 kernel runs"""
    params = _params([51] * 4, 30, seed=2)
    x, h = torch.randn(9, 5, device=DEV), torch.randn(9, 5, 30, device=DEV)
    zs, js, ks = _fwd("gnf_monotonic_fwd", params, x, h, 20)
    zf, jf, kf = _fwd("gnf_monotonic_fwd_f32", params, x, h, 20)
    assert ks == "mono_fwd_k" and kf == "mono_fwd_k" and torch.equal(zs, zf) and torch.equal(js, jf)


def test_split_forward_ragged_sizes_and_strided_h():
    """element counts around the group / half-group boundaries of the persistent schedule, h as a permuted view (MADE's output)"""
    from gnf_hip import abi
    if not abi.load().gnf_gemm_split_enabled():
        pytest.skip("GNF_TRUE_F32=1")
    params = _params([150, 150, 150], 30, seed=11)
    for B, d in [(1, 1), (1, 31), (3, 11), (5, 13), (16385, 1), (513, 33)]:
        g = torch.Generator().manual_seed(B + d)
        x = (torch.randn(B, d, generator=g) * 2.).to(DEV)
        hT = torch.randn(B, 30, d, generator=g).to(DEV)
        h = hT.permute(0, 2, 1)                          # [B, d, c] view with strides (30 d, 1, d)
        zs, js, ks = _fwd("gnf_monotonic_fwd", params, x, h, 20)
        zf, jf, _ = _fwd("gnf_monotonic_fwd_f32", params, x, h, 20)
        assert ks == "mono_fwd_wide_split_k"
        assert torch.allclose(zs, zf, rtol=2e-6, atol=2e-6) and torch.allclose(js, jf, rtol=2e-6, atol=2e-6), (B, d)


def _bwd(entry, params, x, h, S, gz, gjac, ws_bytes=None):
    """ws_bytes: the workspace handed to the entry point (default: what gnf_monotonic_bwd_ws_bytes asks for this problem)"""
    from gnf_hip import abi, ops
    from gnf_hip.abi import call, ptr, stream
    net = ops._mono_net(params)
    pack = ops._mono_pack(net, x)
    w, t = ops.cc_rule(S, x.device)
    B, d = x.shape
    gx, gh = torch.empty_like(x), torch.empty_like(h)
    gp = [torch.empty_like(p) for p in params]
    nl = net.nl
    gW = (ctypes.c_void_p * nl)(*[gp[2 * l].data_ptr() for l in range(nl)])
    gb = (ctypes.c_void_p * nl)(*[gp[2 * l + 1].data_ptr() for l in range(nl)])
    nbytes = abi.load().gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), S, B, d) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nbytes // 4, 1), device=x.device)
    call(entry, ptr(pack), ctypes.byref(net), ptr(x), ptr(h), h.stride(0), h.stride(1), h.stride(2), ptr(w), ptr(t), S, ptr(gz), ptr(gjac),
         ptr(gx), ptr(gh), gh.stride(0), gh.stride(1), gh.stride(2), gW, gb, ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4, B, d, stream())
    return [gx, gh] + gp, abi.load().gnf_monotonic_bwd_kernel().decode()


def _bwd64(params, x, h, S, gz, gjac):
    """fp64 autograd of the fp64 quadrature, with UMNN's Leibniz rule for x (dz/dx = f(x; h)): the z-path treats the nodes as
    constants in x, the jac path differentiates f at x"""
    P = [p.double().requires_grad_(True) for p in params]
    hd = h.double().requires_grad_(True)
    xd = x.double().requires_grad_(True)
    from gnf_hip import ops
    w, t = ops.cc_rule(S, x.device)
    w, t = w.double(), t.double()
    fS = torch.tensor(float(S), dtype=torch.float32, device=x.device)
    xT = (fS * (x / fS)).double()

    def f(tt):
        a = torch.cat([tt.unsqueeze(-1), hd.unsqueeze(2).expand(-1, -1, tt.shape[2], -1)], -1)
        for k in range(0, len(P), 2):
            a = a @ P[k].t() + P[k + 1]
            if k + 2 < len(P):
                a = torch.relu(a)
        a = a[..., 0]
        return torch.where(a > 0, a, torch.expm1(torch.clamp(a, max=0.))) + 1.05
    nodes = xT.unsqueeze(-1) * (t + 1.) / 2.
    z = (f(nodes) * w).sum(-1) * xT / 2. + hd[..., 0]
    jac = f(xd.unsqueeze(-1))[..., 0]
    obj = (z * gz.double()).sum() + (jac * gjac.double()).sum()
    g = torch.autograd.grad(obj, [xd, hd] + P)
    gx = g[0] + gz.double() * jac.detach()             # Leibniz: + gz f(x; h)
    return [gx, g[1]] + list(g[2:])


BCASES = [([100, 100, 100], 30, 6, 700, 20), ([150, 150, 150], 30, 9, 300, 20), ([160, 160], 8, 5, 333, 9), ([112] * 4, 30, 3, 257, 20),
          ([97, 105, 112], 17, 4, 129, 15), ([145, 160, 150], 30, 63, 50, 25)]


@pytest.mark.parametrize("hidden,c,d,B,S", BCASES)
def test_split_backward_vs_fp64_and_fp32_mfma(hidden, c, d, B, S):
    from gnf_hip import abi
    if not abi.load().gnf_gemm_split_enabled():
        pytest.skip("GNF_TRUE_F32=1")
    params = _params(hidden, c, seed=sum(hidden) + S + 1, scale=1.3)
    g = torch.Generator().manual_seed(B + 7)
    x = (torch.randn(B, d, generator=g) * 2.).to(DEV)
    h = torch.randn(B, d, c, generator=g).to(DEV)
    gz, gjac = torch.randn(B, d, generator=g).to(DEV), torch.randn(B, d, generator=g).to(DEV)
    gs, ks = _bwd("gnf_monotonic_bwd", params, x, h, S, gz, gjac)
    gf, kf = _bwd("gnf_monotonic_bwd_f32", params, x, h, S, gz, gjac)
    # (the backward's split form is adopted for H = 145..160 only: at H <= 112 it measured slower than the fp32 chain)
    assert ks == ("mono_bwd_wide_k<split>" if max(hidden) > 112 else "mono_bwd_wide_k<f32>") and kf == "mono_bwd_wide_k<f32>", (ks, kf)
    g64 = _bwd64(params, x, h, S, gz, gjac)
    names = ["gx", "gh"] + ["gW%d" % (i // 2) if i % 2 == 0 else "gb%d" % (i // 2) for i in range(len(params))]
    worst = []
    for nm, a, b, r in zip(names, gs, gf, g64):
        scale = float(r.abs().max()) + 1e-30
        es, ef = float((a.double() - r).abs().max()) / scale, float((b.double() - r).abs().max()) / scale
        rs = float(((a.double() - r).pow(2).mean() / (r.pow(2).mean() + 1e-60)).sqrt())
        rf = float(((b.double() - r).pow(2).mean() / (r.pow(2).mean() + 1e-60)).sqrt())
        worst.append((nm, es, ef, rs, rf))
        # The backward's chain products use ONE accumulator class (registers): 30 roundings per output instead of the fp32
        # MFMA's 40 -- the same error level, not a better one.  Per tensor: within 2x of the fp32 kernel's error + one epsilon;
        # over the tensors of a case: not worse on (geometric) average.  (Errors of 1e-4 against fp64 are common to both
        # kernels: ReLU gates of pre-activations within roundoff of zero.)
        assert rs <= 2. * rf + 1.2e-7, (nm, es, ef, rs, rf)
        assert es <= 2. * ef + 2.4e-7, (nm, es, ef, rs, rf)
        assert es < 5e-3, (nm, es)
    ratio = float(np.exp(np.mean([np.log((w_[3] + 1e-9) / (w_[4] + 1e-9)) for w_ in worst])))
    assert ratio <= 1.15, (ratio, worst)
    print("\n[mono split bwd %s S=%d] geometric mean of rms(split) / rms(fp32-MFMA) over the tensors: %.2f; max rel. error split | fp32-MFMA (rms split | fp32): " % (hidden, S, ratio)
          + ", ".join("%s %.1e|%.1e (%.1e|%.1e)" % w_ for w_ in worst))
    gs2, _ = _bwd("gnf_monotonic_bwd", params, x, h, S, gz, gjac)
    for a, b in zip(gs, gs2):
        assert torch.equal(a, b)


NBCASES = [([50, 50, 50], 30, 784, 6, 20), ([50, 50, 50], 30, 13, 40, 21), ([49, 49], 8, 5, 333, 9), ([51] * 3, 30, 3, 257, 20),
           ([50, 50, 50], 30, 1, 1, 20)]


@pytest.mark.parametrize("hidden,c,d,B,S", NBCASES)
def test_narrow_split_backward_vs_fp64_and_fp32_mfma(hidden, c, d, B, S):
    """the peeled narrow nets (cfg4): mono_bwd_pair_x_k<split> -- recompute and data gradient of the 48 x 48 main blocks on the
    bf16 matrix pipe (two accumulator classes), weight gradients fp32"""
    from gnf_hip import abi
    if not abi.load().gnf_gemm_split_enabled():
        pytest.skip("GNF_TRUE_F32=1")
    params = _params(hidden, c, seed=sum(hidden) + S + 5, scale=1.3)
    g = torch.Generator().manual_seed(B + 9)
    x = (torch.randn(B, d, generator=g) * 2.).to(DEV)
    h = torch.randn(B, d, c, generator=g).to(DEV)
    gz, gjac = torch.randn(B, d, generator=g).to(DEV), torch.randn(B, d, generator=g).to(DEV)
    gs, ks = _bwd("gnf_monotonic_bwd", params, x, h, S, gz, gjac)
    gf, kf = _bwd("gnf_monotonic_bwd_f32", params, x, h, S, gz, gjac)
    assert ks == "mono_bwd_pair_x_k<split>" and kf == "mono_bwd_k", (ks, kf)
    g64 = _bwd64(params, x, h, S, gz, gjac)
    names = ["gx", "gh"] + ["gW%d" % (i // 2) if i % 2 == 0 else "gb%d" % (i // 2) for i in range(len(params))]
    worst = []
    for nm, a, b, r in zip(names, gs, gf, g64):
        scale = float(r.abs().max()) + 1e-30
        es, ef = float((a.double() - r).abs().max()) / scale, float((b.double() - r).abs().max()) / scale
        rs = float(((a.double() - r).pow(2).mean() / (r.pow(2).mean() + 1e-60)).sqrt())
        rf = float(((b.double() - r).pow(2).mean() / (r.pow(2).mean() + 1e-60)).sqrt())
        worst.append((nm, es, ef, rs, rf))
        assert rs <= 2. * rf + 2.4e-7 and es <= 2. * ef + 4.8e-7, (nm, es, ef, rs, rf)
    ratio = float(np.exp(np.mean([np.log((w_[3] + 1e-9) / (w_[4] + 1e-9)) for w_ in worst])))
    assert ratio <= 1.15, (ratio, worst)
    print("\n[mono narrow split bwd %s S=%d] geometric mean of rms(split) / rms(fp32-MFMA): %.2f; " % (hidden, S, ratio)
          + ", ".join("%s %.1e|%.1e" % (w_[0], w_[3], w_[4]) for w_ in worst))
    gs2, _ = _bwd("gnf_monotonic_bwd", params, x, h, S, gz, gjac)
    for a, b in zip(gs, gs2):
        assert torch.equal(a, b)


def test_split_backward_ragged_sizes():
    """element counts around the group / half-group boundaries of the persistent schedule (h contiguous: the backward entry
    asks for a collapsible element stride, ops.MonotonicFn.backward makes the copy)"""
    from gnf_hip import abi
    if not abi.load().gnf_gemm_split_enabled():
        pytest.skip("GNF_TRUE_F32=1")
    params = _params([150, 150, 150], 30, seed=12)
    for B, d in [(1, 1), (1, 31), (3, 11), (5, 13), (8193, 1), (513, 33)]:
        g = torch.Generator().manual_seed(B + d)
        x = (torch.randn(B, d, generator=g) * 2.).to(DEV)
        h = torch.randn(B, d, 30, generator=g).to(DEV)
        gz, gjac = torch.randn(B, d, generator=g).to(DEV), torch.randn(B, d, generator=g).to(DEV)
        gs, ks = _bwd("gnf_monotonic_bwd", params, x, h, 20, gz, gjac)
        gf, _ = _bwd("gnf_monotonic_bwd_f32", params, x, h, 20, gz, gjac)
        assert ks == "mono_bwd_wide_k<split>"
        # an indexing mistake at a group boundary is an O(1) error.  The bound is not roundoff-tight: the parameter gradients are
        # sums of 10^5..10^6 signed terms (|sum| ~ 1e-2 .. 1e-3 of the sum of magnitudes), so two correct fp32 evaluations in
        # different orders differ by ~1e-4 of the result (as either does from fp64, test_split_backward_vs_fp64_and_fp32_mfma)
        for nm, (a, b) in enumerate(zip(gs, gf)):
            num, den = float((a - b).double().pow(2).sum().sqrt()), float(b.double().pow(2).sum().sqrt())
            mx = float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)
            assert num <= 2e-3 * den + 1e-7 and mx <= 2e-2, (B, d, nm, num / (den + 1e-30), mx)


# one net per backward family, each the smallest that reaches it: peeled pair kernel (in-kernel dW), pair kernel, ones column
# (staged dW through the split-K GEMM, GNF_GEMM_ACCUM across chunks), whole image, wide, HT 7 outside the wide kernel
# (mono_dw_k with acc), HT 16 (tall row-sums of staged rows)
CHUNKED = [([50, 50, 50], 30, "gnf_monotonic_bwd"), ([20, 20], 5, "gnf_monotonic_bwd"), ([48, 50, 50, 50], 5, "gnf_monotonic_bwd"),
           ([40, 64, 24], 5, "gnf_monotonic_bwd"), ([150, 150, 150], 30, "gnf_monotonic_bwd"),
           ([150, 150, 150], 30, "gnf_monotonic_bwd_f32"), ([100, 100], 33, "gnf_monotonic_bwd"), ([200, 200], 8, "gnf_monotonic_bwd")]


@pytest.mark.parametrize("hidden,c,entry", CHUNKED)
def test_chunked_backward_vs_fp64_and_full_workspace(hidden, c, entry):
    """a workspace that holds one 16-element chunk: n = 40 runs as chunks of 16, 16 and 8 (the last one ragged), every staged
    product and partial row accumulated across them.  Against fp64 the chunked evaluation is held to what
    test_split_backward_vs_fp64_and_fp32_mfma asks of two evaluation orders: per tensor within 2x of the one-chunk run's
    error plus one epsilon.  The same kernel family runs either way."""
    from gnf_hip import abi, ops
    B, d, S = 5, 8, 20
    params = _params(hidden, c, seed=sum(hidden) + c, scale=1.3)
    g = torch.Generator().manual_seed(len(hidden) + c)
    x = (torch.randn(B, d, generator=g) * 2.).to(DEV)
    h = torch.randn(B, d, c, generator=g).to(DEV)
    gz, gjac = torch.randn(B, d, generator=g).to(DEV), torch.randn(B, d, generator=g).to(DEV)
    net = ops._mono_net(params)
    one_chunk = abi.load().gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), S, 1, 1)
    assert 0 < one_chunk < abi.load().gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), S, B, d)
    gf, kf = _bwd(entry, params, x, h, S, gz, gjac)
    gc, kc = _bwd(entry, params, x, h, S, gz, gjac, ws_bytes=one_chunk)
    assert kc == kf, (kc, kf)
    g64 = _bwd64(params, x, h, S, gz, gjac)
    names = ["gx", "gh"] + ["gW%d" % (i // 2) if i % 2 == 0 else "gb%d" % (i // 2) for i in range(len(params))]
    rows = []
    for nm, a, b, r in zip(names, gc, gf, g64):
        scale = float(r.abs().max()) + 1e-30
        es, ef = float((a.double() - r).abs().max()) / scale, float((b.double() - r).abs().max()) / scale
        rs = float(((a.double() - r).pow(2).mean() / (r.pow(2).mean() + 1e-60)).sqrt())
        rf = float(((b.double() - r).pow(2).mean() / (r.pow(2).mean() + 1e-60)).sqrt())
        rows.append((nm, es, ef, rs, rf))
    print("\n[mono chunked bwd %s c=%d %s] %s; max rel. error chunked | full (rms chunked | full): " % (hidden, c, entry, kc)
          + ", ".join("%s %.1e|%.1e (%.1e|%.1e)" % r_ for r_ in rows))
    for nm, es, ef, rs, rf in rows:
        assert rs <= 2. * rf + 1.2e-7, (nm, es, ef, rs, rf)
        assert es <= 2. * ef + 2.4e-7, (nm, es, ef, rs, rf)


def test_true_f32_switch_selects_the_fp32_kernel():
    import subprocess
    import sys
    code = ("import sys, torch; sys.path[:0] = [%r, %r]\n"
            "from tests.test_gpu_mono_split import _params, _fwd\n"
            "p = _params([150, 150, 150], 30, 1)\n"
            "x = torch.randn(40, 7, device='cuda:0'); h = torch.randn(40, 7, 30, device='cuda:0')\n"
            "print(_fwd('gnf_monotonic_fwd', p, x, h, 20)[2])\n"
            "from tests.test_gpu_mono_split import _bwd\n"
            "print(_bwd('gnf_monotonic_bwd', p, x, h, 20, torch.ones_like(x), torch.ones_like(x))[1])\n") % (ROOT, ROOT + "/graphical-normalizing-flows_amd")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GNF_TRUE_F32="1"), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-2:] == ["mono_fwd_wide_k", "mono_bwd_wide_k<f32>"], out.stdout


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
