"""GPU parity tests proper (-m gpu): the HIP path, called through the mirrored plug-in API
and the C ABI, against (a) the golden vectors generated from the reference and (b) the CPU
oracle on the same seeded inputs.  Tolerance: north_star's 1e-5 relative fp32 for
transformed x, log|det J| and NLL; gradients 1e-4 relative to the tensor's max (sums of
many fp32 products in a different order than torch's addmm)."""
import numpy as np
import pytest
import torch

from conftest import (load_golden, params_of, linear_layers, rel_err, assert_close, assert_fwd, conv_front_knife_images,
                      integrand_knife_elements)
from oracle import gnf_oracle as O
import knife_units

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
GTOL = 1e-4


def cu(t):
    return t.to(DEV)


def req(t):
    return t.clone().to(DEV).requires_grad_(True)


def load_into(module, g, prefix="p."):
    sd = {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}
    missing, unexpected = module.load_state_dict(sd, strict=True), None
    return module.to(DEV)


def grads_match(module, g, tol=GTOL, prefix="g."):
    named = dict(module.named_parameters())
    n = 0
    for k, v in g.items():
        if k.startswith(prefix):
            p = named[k[len(prefix):]]
            assert p.grad is not None, k
            assert rel_err(p.grad.cpu(), v) < tol, (k, rel_err(p.grad.cpu(), v))
            n += 1
    assert n > 0


# --------------------------------------------------------------------------------- normalizers
def test_affine_golden():
    from models import AffineNormalizer
    g = load_golden("affine")
    x, h = req(g["x"]), req(g["h"])
    norm = AffineNormalizer()
    z, jac = norm(x, h)
    assert rel_err(z.cpu(), g["z"]) < TOL and rel_err(jac.cpu(), g["jac"]) < TOL
    assert_fwd(z, g["z"], what='z')
    assert_fwd(jac, g["jac"], what='jac')
    gx, gh = torch.autograd.grad((z * cu(g["gz"])).sum(), (x, h), retain_graph=True)
    assert rel_err(gx.cpu(), g["gx_from_z"]) < TOL and rel_err(gh.cpu(), g["gh_from_z"]) < TOL
    assert_fwd(gx, g["gx_from_z"], what='gx')
    assert_fwd(gh, g["gh_from_z"], what='gh')
    z2, ld = norm.forward_logdet(x, h)
    gh2, = torch.autograd.grad((ld * cu(g["gld"])).sum(), h)
    assert rel_err(gh2.cpu(), g["gh_from_logdet"]) < TOL
    assert_fwd(gh2, g["gh_from_logdet"], what='gh2')
    assert rel_err(ld.detach().cpu(), torch.log(g["jac"]).sum(1)) < TOL
    assert_fwd(ld, torch.log(g["jac"]).sum(1), what='ld')
    assert rel_err(norm.inverse_transform(cu(g["z"]), cu(g["h"])).cpu(), g["x_inverse"]) < TOL
    # in-place clamp option reproduces the reference's mutation of h
    norm.inplace_clamp = True
    hc = cu(g["h"]).clone()
    norm(cu(g["x"]), hc)
    ref = g["h"].clone()
    ref[:, :, 0].clamp_(-5., 5.)
    ref[:, :, 1].clamp_(-5., 2.)
    assert torch.equal(hc.cpu(), ref)


def test_affine_strided_h_and_large():
    from gnf_hip import ops
    torch.manual_seed(0)
    B, d = 3000, 63
    x = torch.randn(B, d)
    hraw = torch.randn(B, 2 * d) * 3
    h = hraw.view(B, 2, d).permute(0, 2, 1)          # MADE layout: strides (2d, 1, d)
    z0, j0 = O.affine_forward(x, h)
    xg, hg = req(x), cu(hraw).requires_grad_(True)
    z, jac, ld, _ = ops.AffineFn.apply(xg, hg.view(B, 2, d).permute(0, 2, 1))
    assert rel_err(z.cpu(), z0) < TOL and rel_err(jac.cpu(), j0) < TOL
    assert_fwd(z, z0, what='z')
    assert_fwd(jac, j0, what='jac')
    assert rel_err(ld.cpu(), torch.log(j0).sum(1)) < TOL
    assert_fwd(ld, torch.log(j0).sum(1), what='ld')
    (z.sum() + ld.sum()).backward()
    xr, hr = x.clone().requires_grad_(True), hraw.clone().requires_grad_(True)
    zr, jr = O.affine_forward(xr, hr.view(B, 2, d).permute(0, 2, 1))
    (zr.sum() + torch.log(jr).sum()).backward()
    assert rel_err(xg.grad.cpu(), xr.grad) < TOL and rel_err(hg.grad.cpu(), hr.grad) < TOL
    assert_fwd(xg.grad, xr.grad, what='xg.grad')
    assert_fwd(hg.grad, hr.grad, what='hg.grad')


@pytest.mark.parametrize("B,d", [(4163, 63), (20001, 63), (4500, 62), (4100, 64), (50003, 6), (70001, 5), (300001, 1)])
def test_affine_flat_vectorised_path_vs_oracle(B, d):
    """short rows in the contiguous [B,d,2] layout (tabular configurations, cfg5: d = 63) take the span-per-wavefront
    kernels with 16-B accesses: every row count modulo the span, odd / even / multiple-of-4 widths, ragged last span"""
    from gnf_hip import ops
    assert B * d >= 1 << 18
    torch.manual_seed(B + d)
    x, h = torch.randn(B, d), torch.randn(B, d, 2) * 3
    z0, j0 = O.affine_forward(x, h)
    xg, hg = req(x), req(h)
    z, jac, ld, _ = ops.AffineFn.apply(xg, hg)
    assert rel_err(z.cpu(), z0) < TOL and rel_err(jac.cpu(), j0) < TOL
    assert_fwd(z, z0, what='z')
    assert_fwd(jac, j0, what='jac')
    assert rel_err(ld.cpu(), torch.log(j0).sum(1)) < TOL
    assert_fwd(ld, torch.log(j0).sum(1), what='ld')
    assert_close(ld, torch.log(j0).sum(1), atol=2e-6 * d ** .5, what="logdet")
    gz, gj, gl = torch.randn(B, d), torch.randn(B, d), torch.randn(B)
    ((z * cu(gz)).sum() + (jac * cu(gj)).sum() + (ld * cu(gl)).sum()).backward()
    xr, hr = x.clone().requires_grad_(True), h.clone().requires_grad_(True)
    zr, jr = O.affine_forward(xr, hr)
    ((zr * gz).sum() + (jr * gj).sum() + (torch.log(jr).sum(1) * gl).sum()).backward()
    assert rel_err(xg.grad.cpu(), xr.grad) < TOL and rel_err(hg.grad.cpu(), hr.grad) < TOL
    assert_fwd(xg.grad, xr.grad, what='xg.grad')
    assert_fwd(hg.grad, hr.grad, what='hg.grad')
    # the fused step's variant (no jac output) and determinism
    with torch.no_grad():
        z2, _, ld2, _ = ops.AffineFn.apply(cu(x), cu(h), False, False)
        z3, _, ld3, _ = ops.AffineFn.apply(cu(x), cu(h), False, False)
    assert torch.equal(z2, z.detach()) and torch.equal(ld2, ld3) and rel_err(ld2.cpu(), ld.detach().cpu()) < 1e-6


def test_normal_log_density_and_logsum():
    from models.NormalizingFlowFactories import NormalLogDensity
    from gnf_hip import ops
    g = load_golden("normal_log_density")
    z = req(g["z"])
    out = NormalLogDensity().to(DEV)(z)
    assert rel_err(out.cpu(), g["out"]) < TOL
    assert_fwd(out, g["out"], what='out')
    out.sum().backward()
    assert rel_err(z.grad.cpu(), -g["z"]) < TOL
    assert_fwd(z.grad, -g["z"], what='z.grad')
    for B, d in [(5, 1), (7, 2), (33, 6), (100, 784), (1000, 63)]:
        jac = torch.rand(B, d) + .1
        j = req(jac)
        o = ops.LogSumRowsFn.apply(j)
        assert rel_err(o.cpu(), torch.log(jac).sum(1)) < TOL
        assert_fwd(o, torch.log(jac).sum(1), what='o')
        w = torch.randn(B)
        (o * cu(w)).sum().backward()
        assert rel_err(j.grad.cpu(), w[:, None] / jac) < TOL
        assert_fwd(j.grad, w[:, None] / jac, what='j.grad')


# --------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (7, 5, 3), (100, 1024, 784), (64, 64, 16), (130, 70, 33),
                                   (2500, 60, 12), (300, 300, 300), (1568, 128, 2304)])
def test_gemm_shapes(M, N, K):
    from gnf_hip import ops
    torch.manual_seed(M + N + K)
    A, W = torch.randn(M, K), torch.randn(N, K)
    mask = (torch.rand(N, K) < .6).float()
    bias = torch.randn(N)
    ref = torch.relu(A.double() @ (W * mask).double().t() + bias.double())
    C = torch.empty(M, N, device=DEV)
    ops.gemm(cu(A), (K, 1), cu(W), (1, K), C, (N, 1), M, N, K, Bmask=cu(mask), bias=cu(bias), relu=True)
    assert rel_err(C.cpu(), ref) < 2e-6
    # transposed-A form used for weight gradients, with output mask
    G = torch.randn(M, N)
    ref2 = (G.double().t() @ A.double()) * mask.double()
    C2 = torch.empty(N, K, device=DEV)
    ops.gemm(cu(G), (1, N), cu(A), (K, 1), C2, (K, 1), N, K, M, Cmask=cu(mask), cm_strides=(K, 1))
    assert rel_err(C2.cpu(), ref2) < 2e-6
    # data-gradient form with ReLU gate
    gate = torch.randn(M, K)
    ref3 = (G.double() @ (W * mask).double()) * (gate > 0).double()
    C3 = torch.empty(M, K, device=DEV)
    ops.gemm(cu(G), (N, 1), cu(W), (K, 1), C3, (K, 1), M, K, N, Bmask=cu(mask), gate=cu(gate), g_strides=(K, 1))
    assert rel_err(C3.cpu(), ref3) < 2e-6


def _last_gemm_kernel():
    from gnf_hip import abi
    return abi.load().gnf_gemm_last_kernel().decode()


@pytest.mark.parametrize("M,N,K", [(78400, 128, 2304), (65536, 128, 256), (65000, 100, 288), (49152, 128, 256),
                                   (48500, 127, 320), (40000, 128, 256)])
def test_gemm_tall_long_k_path(M, N, K):
    """C = relu(A[M x K] W[N x K]^T + b), both k-contiguous, 96 < N <= 128, K % 32 == 0, tall M (the fc1 forward of the
    MNISTCNN): the persistent gemm_tall_k with 320- / 256- / 192-row blocks (78 400 -> 5, 65 536 -> 4, 49 152 -> 3 tiles per
    wavefront row), ragged last blocks and N < 128 included; 40 000 rows fill no block height and stay on gemm_vec_k.
    Strided rows of A / C and a plain (no bias, no ReLU) call too; every entry of C is written exactly where it belongs."""
    from gnf_hip import ops
    torch.manual_seed(M + N + K)
    A, W, bias = torch.randn(M, K, device=DEV), torch.randn(N, K, device=DEV), torch.randn(N, device=DEV)
    C = torch.full((M, N), float("nan"), device=DEV)
    from gnf_hip import abi
    from gnf_hip.abi import ptr, call, stream
    rows = torch.cat([torch.arange(0, 700), torch.randint(0, M, (3000,)), torch.arange(M - 700, M)]).to(DEV)
    ref = torch.relu(A[rows].double() @ W.double().t() + bias.double())
    # the fp32-MFMA kernel of the shape (no workspace: the split-bf16 dispatch of round 6 needs one; this is also what
    # GNF_TRUE_F32=1 runs)
    call("gnf_gemm", ptr(A), K, 1, ptr(W), None, 1, K, ptr(C), N, 1, ptr(bias), None, 0, 0, None, 0, 0, 1, M, N, K, None, 0, stream())
    ran = _last_gemm_kernel()
    assert ran == ("gemm_tall_k" if M != 40000 else "gemm_vec_k<64,64>"), ran     # the shape reaches the kernel it is written for
    assert not torch.isnan(C).any()
    assert rel_err(C[rows].cpu(), ref.cpu()) < 2e-6
    # the product's dispatch (ops.gemm hands gnf_gemm its workspace): K % 128 == 0 goes to the split-bf16 tall kernel
    C.fill_(float("nan"))
    ops.gemm(A, (K, 1), W, (1, K), C, (N, 1), M, N, K, bias=bias, relu=True)
    ran = _last_gemm_kernel()
    if abi.load().gnf_gemm_split_enabled() and K % 128 == 0:
        assert ran == "gemm_split_tall_k", ran
    else:
        assert ran == ("gemm_tall_k" if M != 40000 else "gemm_vec_k<64,64>"), ran
    assert not torch.isnan(C).any()
    assert rel_err(C[rows].cpu(), ref.cpu()) < 2e-6
    if M <= 50000:
        Aw, Cw = torch.randn(M, K + 8, device=DEV), torch.zeros(M, N + 4, device=DEV)
        ops.gemm(Aw, (K + 8, 1), W, (1, K), Cw, (N + 4, 1), M, N, K)
        assert rel_err(Cw[rows, :N].cpu(), (Aw[rows, :K].double() @ W.double().t()).cpu()) < 2e-6
        assert float(Cw[:, N:].abs().max()) == 0.


@pytest.mark.parametrize("M,N,K", [(128, 2304, 78400), (64, 516, 40001), (128, 640, 20000), (100, 1024, 33000)])
def test_gemm_kmajor_split_k_path(M, N, K):
    """C[M x N] = dY[K x M]^T X[K x N], both operands k-major, M <= 128, K >= 16 384 (the fc1 weight gradient of the
    MNISTCNN): gemm_kmajor_k over 256 / ntile K ranges + the split-K reduction; ragged K ranges (K not a multiple of 64 or
    of the split count), ragged N tiles, M < 128, and strided rows of both operands (views into wider buffers)"""
    from gnf_hip import ops
    torch.manual_seed(M + N + K)
    dY, X = torch.randn(K, M, device=DEV), torch.randn(K, N, device=DEV)
    from gnf_hip import abi
    from gnf_hip.abi import ptr, call, stream
    lib = abi.load()
    ref = dY.double().t() @ X.double()
    C = torch.full((M, N), float("nan"), device=DEV)
    # the fp32-MFMA kernel: a workspace of exactly its split-K partials (too small for the split-bf16 dispatch of round 6;
    # what GNF_TRUE_F32=1 runs), then the product's dispatch through ops.gemm
    nws = int(lib.gnf_gemm_f32_ws_bytes(M, N, K))
    w = torch.empty(nws // 4, device=DEV)
    call("gnf_gemm", ptr(dY), 1, M, ptr(X), None, N, 1, ptr(C), N, 1, None, None, 0, 0, None, 0, 0, 0, M, N, K, ptr(w), nws, stream())
    assert _last_gemm_kernel() == "gemm_kmajor_k", _last_gemm_kernel()
    assert rel_err(C.cpu(), ref.cpu()) < 2e-6
    C.fill_(float("nan"))
    ops.gemm(dY, (1, M), X, (N, 1), C, (N, 1), M, N, K)
    split = lib.gnf_gemm_split_enabled() and N % 128 == 0 and M >= 16
    assert _last_gemm_kernel() == ("gemm_split_kmajor_k" if split else "gemm_kmajor_k"), _last_gemm_kernel()
    assert rel_err(C.cpu(), ref.cpu()) < 2e-6
    dYw, Xw = torch.randn(K, M + 4, device=DEV), torch.randn(K, N + 8, device=DEV)
    C2 = torch.full((M, N), float("nan"), device=DEV)
    ops.gemm(dYw, (1, M + 4), Xw, (N + 8, 1), C2, (N, 1), M, N, K)
    assert rel_err(C2.cpu(), (dYw[:, :M].double().t() @ Xw[:, :N].double()).cpu()) < 2e-6


@pytest.mark.parametrize("M,N", [(4096, 512), (5003, 644), (78400, 2304)])
def test_gemm_wide_short_k_path(M, N):
    """C = A[M x 128] * B[128 x N], A k-contiguous, B n-contiguous, no epilogue options (the fc1 data gradient of the
    MNISTCNN): the persistent unit-range kernel (gemm_wide_k), ragged row blocks and N tiles included"""
    from gnf_hip import ops
    torch.manual_seed(M + N)
    K = 128
    A, B = torch.randn(M, K, device=DEV), torch.randn(K, N, device=DEV)
    C = torch.full((M, N), float("nan"), device=DEV)
    from gnf_hip import abi
    from gnf_hip.abi import ptr, call, stream
    ref = (A.double() @ B.double())
    # the fp32-MFMA kernel (no workspace -> no split-bf16 dispatch; what GNF_TRUE_F32=1 runs), then the product's dispatch
    call("gnf_gemm", ptr(A), K, 1, ptr(B), None, N, 1, ptr(C), N, 1, None, None, 0, 0, None, 0, 0, 0, M, N, K, None, 0, stream())
    assert _last_gemm_kernel() == "gemm_wide_k", _last_gemm_kernel()
    assert rel_err(C.cpu(), ref.cpu()) < 2e-6
    assert not torch.isnan(C).any()
    C.fill_(float("nan"))
    ops.gemm(A, (K, 1), B, (N, 1), C, (N, 1), M, N, K)
    split = abi.load().gnf_gemm_split_enabled() and M >= 10240 and N % 128 == 0
    assert _last_gemm_kernel() == ("gemm_split_wide_k" if split else "gemm_wide_k"), _last_gemm_kernel()
    assert rel_err(C.cpu(), ref.cpu()) < 2e-6
    assert not torch.isnan(C).any()
    # strided rows of A and C (views into wider buffers)
    Aw, Cw = torch.randn(M, K + 8, device=DEV), torch.zeros(M, N + 12, device=DEV)
    ops.gemm(Aw, (K + 8, 1), B, (N, 1), Cw, (N + 12, 1), M, N, K)
    assert rel_err(Cw[:, :N].cpu(), (Aw[:, :K].double() @ B.double()).cpu()) < 2e-6 and float(Cw[:, N:].abs().max()) == 0.


def test_gemm_operand_beyond_4_GiB_on_the_generic_kernels():
    """byte offsets past 2^32 on the kernels that have no dedicated guard (verdict r04 #2): a 4.9 GB A operand through
    gemm_vec_k (N = 48 keeps it off the tall kernel), last rows against torch; the dedicated fc1 kernels see such extents in
    test_cfg4_strong_scaling_n1_point_B800 (pooled features 5.8 GB)"""
    from gnf_hip import ops
    M, N, K = 600_000, 48, 2048
    torch.manual_seed(1)
    A = torch.empty(M, K, device=DEV).normal_()
    W, bias = torch.randn(N, K, device=DEV), torch.randn(N, device=DEV)
    assert A.numel() * 4 > (1 << 32)
    C = torch.full((M, N), float("nan"), device=DEV)
    ops.gemm(A, (K, 1), W, (1, K), C, (N, 1), M, N, K, bias=bias, relu=True)
    assert _last_gemm_kernel().startswith("gemm_vec_k"), _last_gemm_kernel()
    rows = torch.cat([torch.arange(0, 200), torch.randint(0, M, (1000,)), torch.arange(M - 200, M)]).to(DEV)
    ref = torch.relu(A[rows].double() @ W.double().t() + bias.double())
    assert not torch.isnan(C).any()
    assert rel_err(C[rows].cpu(), ref.cpu()) < 2e-6
    # ... and as the contraction of a weight-gradient product (K = 600 000 rows of the same 4.9 GB operand)
    G = torch.randn(M, 16, device=DEV)
    D = torch.full((16, K), float("nan"), device=DEV)
    ops.gemm(G, (1, 16), A, (K, 1), D, (K, 1), 16, K, M)
    assert _last_gemm_kernel() in ("gemm_kmajor_k", "gemm_split_kmajor_k")
    assert rel_err(D.cpu(), (G.double().t() @ A.double()).cpu()) < 1e-5      # 600 000 fp32 terms per entry: 3.7e-6 measured


def test_colsum():
    from gnf_hip import ops
    for M, N in [(1, 1), (513, 7), (5000, 300)]:
        a = torch.randn(M, N)
        assert rel_err(ops.colsum(cu(a)).cpu(), a.double().sum(0)) < 2e-6


# --------------------------------------------------------------------------------- conditioners
def test_coupling_golden():
    from models import CouplingConditioner
    g = load_golden("coupling")
    c = load_into(CouplingConditioner(5, [16, 16], 3), g)
    x = req(g["x"])
    h = c(x)
    assert rel_err(h.cpu(), g["h"]) < TOL
    assert_fwd(h, g["h"], what='h')
    (h * cu(g["gh"])).sum().backward()
    assert rel_err(x.grad.cpu(), g["gx"]) < GTOL
    grads_match(c, g)


def test_autoregressive_golden():
    from models import AutoregressiveConditioner
    g = load_golden("autoregressive")
    c = AutoregressiveConditioner(7, [16, 12, 16], 3)
    for k, v in c.state_dict().items():          # masks built by the mirror == reference masks
        if k.endswith("mask"):
            assert torch.equal(v, g["p." + k])
    c = load_into(c, g)
    x = req(g["x"])
    h = c(x)
    assert h.shape == g["h"].shape and rel_err(h.cpu(), g["h"]) < TOL
    (h * cu(g["gh"])).sum().backward()
    assert rel_err(x.grad.cpu(), g["gx"]) < GTOL
    grads_match(c, g)
    assert c.depth() == 6


@pytest.mark.parametrize("tag", ["det", "gumbel", "gumbel_hot_T05", "hard", "hard_gumbel"])
def test_dag_golden(tag):
    from models import DAGConditioner
    g = load_golden("dag_" + tag)
    hot, stoch, hth, T = g["flags"].tolist()
    c = DAGConditioner(6, [12, 10], 4, hot_encoding=bool(hot), gumble_T=T, l1=.1)
    c = load_into(c, g)
    c.stoch_gate = bool(stoch)
    c.h_thresh = hth
    c.gate_noise = (cu(g["u1"]), cu(g["u2"]))
    x = req(g["x"])
    h = c(x)
    assert rel_err(h.cpu(), g["h"]) < TOL
    assert_fwd(h, g["h"], what='h')
    loss = c.loss()
    assert rel_err(loss.detach().cpu(), g["loss"]) < TOL
    assert_fwd(loss, g["loss"], what='loss')
    assert rel_err(c.get_power_trace().detach().cpu(), g["trace"]) < TOL
    assert_fwd(c.get_power_trace(), g["trace"], what='c.get_power_trace()')
    ((h * cu(g["gh"])).sum() + loss).backward()
    assert rel_err(x.grad.cpu(), g["gx"]) < GTOL
    grads_match(c, g)


def test_dag_gate_philox_statistics_and_determinism():
    from gnf_hip import ops
    torch.manual_seed(0)
    B, d = 64, 48
    x = torch.ones(B, d, device=DEV)
    A = (torch.rand(d, d, device=DEV) * 1.5).requires_grad_(True)
    args = (ops.IMP_SOFT, ops.GATE_GUMBEL, 0., 1., False, None, None, 1234, 7)
    e1 = ops.DagGateFn.apply(x, A, *args)
    e2 = ops.DagGateFn.apply(x, A, *args)
    assert torch.equal(e1, e2)                                        # counter-based: reproducible
    e3 = ops.DagGateFn.apply(x, A, ops.IMP_SOFT, ops.GATE_GUMBEL, 0., 1., False, None, None, 1234, 8)
    assert not torch.equal(e1, e3)
    # Gumbel-max identity: P(gate > 1/2) = P(log(p+eps)+g1 > log(1-p+eps)+g2) = (p+eps)/(1+2eps), any T
    p = (2 * (torch.sigmoid(2 * A.detach() ** 2) - .5))
    frac = torch.stack([(ops.DagGateFn.apply(x, A, ops.IMP_SOFT, ops.GATE_GUMBEL, 0., .5, False, None, None, 99, k)
                         .detach().view(B, d, d) > .5).float() for k in range(40)]).mean((0, 1))
    assert (frac - p).abs().max() < .05          # 2560 draws per entry: sigma <= 0.01
    # backward regenerates the same noise: finite-difference check of d(sum e)/dA on one entry
    e1.sum().backward()
    gA = A.grad.clone()
    with torch.no_grad():
        Ap = A.detach().clone(); Ap[3, 5] += 1e-2
        Am = A.detach().clone(); Am[3, 5] -= 1e-2
        fd = (ops.DagGateFn.apply(x, Ap, *args).double().sum() - ops.DagGateFn.apply(x, Am, *args).double().sum()) / 2e-2
    assert abs(fd.item() - gA[3, 5].item()) < 2e-2 * max(1., abs(fd.item()))


def test_dag_gate_single_uniform_sampler_has_the_reference_law():
    """The Philox path draws ONE uniform V per element and uses exp(g2 - g1) = V / (1 - V): E1 / (E1 + E2) of two
    independent Exp(1) variates is exactly uniform, so this is the law of the reference's two-uniform Gumbel ratio
    (DAGConditioner.py:99-103).  Checked empirically against the kernel fed with torch.rand u1, u2 (the parity path)
    at several importances and temperatures: the empirical CDFs of the gate agree within sampling error."""
    from gnf_hip import ops
    torch.manual_seed(3)
    B, d = 512, 16
    x = torch.ones(B, d, device=DEV)
    A = torch.linspace(.05, 1.6, d * d, device=DEV).view(d, d).contiguous()
    for T in (1., .5, .7):
        fast = torch.cat([ops.DagGateFn.apply(x, A, ops.IMP_SOFT, ops.GATE_GUMBEL, 0., T, False, None, None, 4242, k)
                          .view(B, d, d) for k in range(8)])                       # 4096 draws per entry
        ref = torch.cat([ops.DagGateFn.apply(x, A, ops.IMP_SOFT, ops.GATE_GUMBEL, 0., T, False,
                                             torch.rand(B, d, d, device=DEV), torch.rand(B, d, d, device=DEV), 0, 0)
                         .view(B, d, d) for _ in range(8)])
        for thr in (.05, .25, .5, .75, .95):
            cf, cr = (fast < thr).float().mean(0), (ref < thr).float().mean(0)
            # two binomial proportions of 4096 draws each: sigma of the difference <= sqrt(2 * .25 / 4096) = .011
            assert (cf - cr).abs().max() < .055, (T, thr, (cf - cr).abs().max().item())
        assert (fast.mean(0) - ref.mean(0)).abs().max() < .03


def test_mnistcnn_golden():
    from models.MLP import MNISTCNN
    g = load_golden("mnistcnn")
    net = load_into(MNISTCNN(out_d=30), g)
    e = req(g["e"])
    out = net(e)
    assert rel_err(out.cpu(), g["out"]) < TOL
    assert_fwd(out, g["out"], what='out')
    # element-wise too (review of round 5, item 7: the infinity norm leaves the small entries unconstrained)
    assert_close(out, g["out"], rtol=1e-5, atol=1e-6 * g["out"].abs().max().item(), what="out")
    (out * cu(g["gout"])).sum().backward()
    assert rel_err(e.grad.cpu(), g["ge"]) < GTOL
    grads_match(net, g)
    # element-wise against the REFERENCE's gradients (verdict r04 item 5)
    assert_close(e.grad, g["ge"], rtol=1e-4, atol=1e-6 * g["ge"].abs().max().item(), what="de")
    for k, p in net.named_parameters():
        assert_close(p.grad, g["g." + k], rtol=1e-4, atol=1e-6 * g["g." + k].abs().max().item(), what="d" + k)


@pytest.mark.parametrize("n,kind", [(1, "dense"), (3, "sparse"), (700, "dense"), (1300, "sparse"),
                                    # the software-pipelined kernels of round 4 (next image's conv1 under this image's MFMA
                                    # work, two input / a1 buffers): workgroups with exactly one image, one workgroup with
                                    # two and the others with one, exactly two each, an odd tail
                                    (2, "dense"), (257, "dense"), (512, "dense"), (515, "sparse")])
def test_mnist_conv_front_vs_torch_cpu(n, kind):
    """fused conv1+ReLU+conv2+maxpool kernel (fwd, bwd) vs the same torch-CPU ops the oracle uses;
    'sparse' images have large exactly-constant regions -> exact pool ties (first max must win)."""
    import torch.nn.functional as F
    from gnf_hip import ops
    # Knife edges: a ReLU / max-pool decision taken on a quantity within fp32 roundoff of the tie can flip between two correct
    # fp32 evaluations (different summation order).  An fp64 evaluation finds the images that hold one (5.7-8.5 % of the images of
    # these seeds at 16 ulps); they are REDRAWN from the same generator until none is left -- images are independent, a redraw
    # touches no other image's decisions -- so every image carries a live cotangent here.  The tied images of the raw draw are
    # judged against the fp64 gradient of one admissible decision in tests/test_gpu_knife.py.  (Until round 4: a blanket 5e-3;
    # rounds 5-6: a zero cotangent for up to 10 % of the images.)
    (e, W1, b1, W2, b2), redraw = knife_units.draw_conv_front(n, kind)
    (e,), _ = knife_units.resample_off_ties(redraw, lambda e_: conv_front_knife_images(e_, W1, b1, W2, b2)[0], first=(e,))
    ps = [t.clone().requires_grad_(True) for t in (e, W1, b1, W2, b2)]
    ref = torch.flatten(F.max_pool2d(F.conv2d(torch.relu(F.conv2d(ps[0].view(-1, 1, 28, 28), ps[1], ps[2])),
                                              ps[3], ps[4]), 2), 1)
    gp = torch.randn(n, 2304)
    assert bool((gp.abs().amax(1) > 0).all())
    (ref * gp).sum().backward()
    pg = [req(t) for t in (e, W1, b1, W2, b2)]
    out = ops.MnistConvFn.apply(*pg, kind == "sparse")        # exactly tied windows -> the tie-exact forward
    assert rel_err(out.cpu(), ref.detach()) < TOL
    assert_fwd(out, ref.detach(), what='out')
    assert_close(out, ref, rtol=1e-5, atol=1e-6 * ref.detach().abs().max().item(), what="pooled (every image)")
    (out * cu(gp)).sum().backward()
    ge, gr = pg[0].grad.cpu(), ps[0].grad
    per_img = (ge - gr).abs().amax(1) / gr.abs().amax(1).clamp_min(1e-30)
    assert float(per_img.max()) < GTOL, (per_img.max().item(), int(per_img.argmax()))
    for a, b, name in zip(pg[1:], ps[1:], ("W1", "b1", "W2", "b2")):
        assert rel_err(a.grad.cpu(), b.grad) < GTOL, (name, rel_err(a.grad.cpu(), b.grad))
        assert_close(a.grad, b.grad, rtol=1e-4, atol=2e-6 * b.grad.abs().max().item(), what="d" + name)
    assert int(conv_front_knife_images(e, W1, b1, W2, b2)[0].sum()) == 0            # no tied image is left


# --------------------------------------------------------------------------------- flows (golden)
def _build(name):
    from models import (buildFCNormalizingFlow, CouplingConditioner, AutoregressiveConditioner, DAGConditioner,
                        AffineNormalizer)
    if name == "flow_affine_coupling_1":
        return buildFCNormalizingFlow(1, CouplingConditioner, {"in_size": 2, "hidden": [32, 32], "out_size": 2},
                                      AffineNormalizer, {})
    if name == "flow_affine_coupling_3":
        return buildFCNormalizingFlow(3, CouplingConditioner, {"in_size": 5, "hidden": [16, 16], "out_size": 2},
                                      AffineNormalizer, {})
    if name == "flow_affine_made_1":
        return buildFCNormalizingFlow(1, AutoregressiveConditioner,
                                      {"in_size": 8, "hidden": [24, 24, 24], "out_size": 2}, AffineNormalizer, {})
    if name == "flow_affine_dag_2":
        return buildFCNormalizingFlow(2, DAGConditioner, {"in_size": 6, "hidden": [16, 16], "out_size": 2,
                                                          "l1": .05, "gumble_T": .5, "hot_encoding": True},
                                      AffineNormalizer, {})
    raise KeyError(name)


@pytest.mark.parametrize("name", ["flow_affine_coupling_1", "flow_affine_coupling_3", "flow_affine_made_1",
                                  "flow_affine_dag_2"])
def test_flow_golden(name):
    g = load_golden(name)
    flow = _build(name)
    assert list(flow.state_dict().keys()) == list(g["state_keys"])       # checkpoint-compatible keys
    flow = load_into(flow, g)
    for s, step in enumerate(flow.steps):
        if "u1_%d" % s in g:
            step.conditioner.gate_noise = (cu(g["u1_%d" % s]), cu(g["u2_%d" % s]))
    x = req(g["x"])
    z, ld = flow(x)
    assert rel_err(z.cpu(), g["z"]) < TOL and rel_err(ld.cpu(), g["logdet"]) < TOL
    assert_fwd(z, g["z"], what='z')
    assert_fwd(ld, g["logdet"], what='ld')
    assert_close(z, g["z"], what="z")                      # element-wise: |a-b| <= 1e-6 + 1e-5 |b|
    assert_close(ld, g["logdet"], what="logdet")
    loss = flow.loss(z, ld)
    assert rel_err(loss.detach().cpu(), g["loss"]) < TOL
    assert_fwd(loss, g["loss"], what='loss')
    assert_close(loss, g["loss"], what="loss")
    loss.backward()
    assert rel_err(x.grad.cpu(), g["gx"]) < GTOL
    grads_match(flow, g)


@pytest.mark.parametrize("name", ["flow_affine_coupling_1", "flow_affine_made_1"])
def test_flow_inverse_golden(name):
    g, gi = load_golden(name), load_golden(name + "_inv")
    flow = load_into(_build(name), g)
    x = flow.invert(cu(gi["z"]))
    assert rel_err(x.cpu(), gi["x"]) < TOL
    assert_fwd(x, gi["x"], what='x')
    assert rel_err(x.cpu(), g["x"]) < 1e-4


def test_multi_step_inverse_round_trip():
    g = load_golden("flow_affine_coupling_3")
    flow = load_into(_build("flow_affine_coupling_3"), g)
    with torch.no_grad():
        z, _ = flow(cu(g["x"]))
        x = flow.invert(z)
    assert rel_err(x.cpu(), g["x"]) < 1e-4


def test_mnist_affine_dag_flow_golden():
    from models import AffineNormalizer
    from models.NormalizingFlowFactories import buildMNISTNormalizingFlow
    g = load_golden("flow_mnist_affine_dag")
    flow = buildMNISTNormalizingFlow([1], AffineNormalizer, {}, l1=0., nb_epoch_update=10, hot_encoding=False,
                                     prior_kernel=2)
    assert list(flow.state_dict().keys()) == list(g["state_keys"])
    sd = {k[2:]: v for k, v in g.items() if k.startswith("p.")}
    sd["steps.0.conditioner.A"] = flow.steps[0].conditioner.A.detach().clone()   # the kernel-2 prior itself
    flow.load_state_dict(sd)
    flow = flow.to(DEV)
    torch.manual_seed(int(g["gate_seed"]))
    u1 = torch.rand(2, 784, 784)
    u2 = torch.rand(2, 784, 784)
    cond = flow.steps[0].conditioner
    cond.gate_noise = (cu(u1), cu(u2))
    z, ld = flow(cu(g["x"]))
    assert rel_err(z.cpu(), g["z"]) < TOL and rel_err(ld.cpu(), g["logdet"]) < TOL
    assert_fwd(z, g["z"], what='z')
    assert_fwd(ld, g["logdet"], what='ld')
    assert_close(z, g["z"], atol=2e-6, what="z")
    assert_close(ld, g["logdet"], what="logdet")
    loss = flow.loss(z, ld)
    assert rel_err(loss.detach().cpu(), g["loss"]) < TOL
    assert_fwd(loss, g["loss"], what='loss')
    loss.backward()
    gA = cond.A.grad.cpu()
    idx = g["gA_idx"].long()
    assert rel_err(gA[idx[:, 0], idx[:, 1]], g["gA_val"]) < GTOL
    assert int((gA != 0).sum()) == idx.shape[0]        # zero entries of A keep an exactly-zero gradient
    named = dict(flow.named_parameters())
    for k, v in g.items():
        if k.startswith("g."):
            assert rel_err(named[k[2:]].grad.cpu(), v) < GTOL, k


def test_mnist_three_scale_flow_golden():
    """CNNormalizingFlow of the 3-scale MNIST factory (reference Factories.py:51-78, NormalizingFlow.py:172-194),
    deterministic gates: z, log-det, loss and gradients against the reference."""
    from models import AffineNormalizer
    from models.NormalizingFlowFactories import buildMNISTNormalizingFlow
    g = load_golden("flow_mnist3_affine")
    flow = buildMNISTNormalizingFlow([1, 1, 1], AffineNormalizer, {}, l1=0., nb_epoch_update=10, hot_encoding=False,
                                     prior_kernel=2)
    assert list(flow.state_dict().keys()) == list(g["state_keys"])
    sd = {k[2:]: v for k, v in g.items() if k.startswith("p.")}
    for k, v in flow.state_dict().items():
        if k.endswith("conditioner.A"):
            sd[k] = v.detach().clone()                   # the kernel-2 priors themselves
    flow.load_state_dict(sd)
    flow = flow.to(DEV)
    for c in flow.getConditioners():
        c.stoch_gate = False
    z, ld = flow(cu(g["x"]))
    assert rel_err(z.cpu(), g["z"]) < TOL and rel_err(ld.cpu(), g["logdet"]) < TOL
    assert_fwd(z, g["z"], what='z')
    assert_fwd(ld, g["logdet"], what='ld')
    loss = flow.loss(z, ld)
    assert rel_err(loss.detach().cpu(), g["loss"]) < TOL
    assert_fwd(loss, g["loss"], what='loss')
    loss.backward()
    named = dict(flow.named_parameters())
    for k, v in g.items():
        if k.startswith("g."):
            assert rel_err(named[k[2:]].grad.cpu(), v) < GTOL, k
        elif k.startswith("g8."):
            assert rel_err(named[k[3:]].grad.cpu()[:8], v) < GTOL, k
        elif k.startswith("gAidx."):
            gA = named[k[6:]].grad.cpu()
            idx = v.long()
            assert rel_err(gA[idx[:, 0], idx[:, 1]], g["gAval." + k[6:]]) < GTOL, k
            assert int((gA != 0).sum()) == idx.shape[0]


def test_mnist_three_scale_invert_round_trip():
    from models import AffineNormalizer
    from models.NormalizingFlowFactories import buildMNISTNormalizingFlow
    torch.manual_seed(3)
    flow = buildMNISTNormalizingFlow([1, 1, 1], AffineNormalizer, {}, prior_kernel=1).to(DEV)
    for c in flow.getConditioners():
        c.stoch_gate = False
        n = int(round(c.in_size ** .5))          # the window prior is symmetric (not a DAG): keep "pixel above" only
        A = torch.zeros(c.in_size, c.in_size)
        A[torch.arange(n, c.in_size), torch.arange(0, c.in_size - n)] = 1.
        c.A.data.copy_(A)
    x = cu(torch.randn(2, 784))
    with torch.no_grad():
        z, _ = flow(x)
        xr = flow.invert(z)
    assert rel_err(xr.cpu(), x.cpu()) < 1e-4


_INV_SNIPPET = """
import sys, torch
sys.path[:0] = %r
from gnf_hip import ops
from models import MonotonicNormalizer
torch.manual_seed(3)
n, d, c, S, H = %d, 1, 30, %d, %d
norm = MonotonicNormalizer([H, H, H], c, nb_steps=S).to("cuda:0")
g = torch.Generator().manual_seed(4)
z = (torch.randn(n, d, generator=g) * 3).to("cuda:0")
h = torch.randn(n, d, c, generator=g).to("cuda:0")
x = ops.monotonic_inverse(z, h, S, [p.detach() for p in norm.integrand_net.flat_params()])
torch.save(x.cpu(), %r)
"""


@pytest.mark.parametrize("n,S,H", [(700, 20, 50), (37, 20, 50), (3, 27, 50), (1000, 30, 50), (700, 7, 50), (512, 20, 50),
                                   (513, 20, 50), (301, 31, 50),
                                   # more nodes than the two-steps-per-round kernel has slots for (32 per point): both runs take
                                   # the one-step kernel -- a two-element workgroup would otherwise still fit its wavefront budget
                                   (100, 40, 50), (300, 32, 50),
                                   # the other peeled widths: 51 = three tiles + THREE units on the VALU, 49 = + one
                                   (700, 20, 51), (200, 20, 51), (700, 20, 49), (64, 9, 49)])
def test_split_inverse_two_steps_per_round_is_bit_identical(n, S, H, tmp_path):
    """the level kernels of a sampling pass take TWO bisection steps per round (midpoint + both quarter points evaluated at
    once, mono_inv_ks_x_k; workgroups of two elements up to 512 elements per call, of four above): same midpoints, same sums,
    so the same bits as the 20 sequential steps (GNF_MONO_INV_PTS=1, run in a second process: the switch is read once) --
    reference MonotonicNormalizer.py:69-83"""
    import os, subprocess, sys
    from conftest import ROOT, PKG
    outs = []
    for tag, env in (("pts3", {}), ("pts1", {"GNF_MONO_INV_PTS": "1"})):
        f = str(tmp_path / (tag + ".pt"))
        code = _INV_SNIPPET % ([ROOT, PKG], n, S, H, f)
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(torch.load(f))
    assert torch.equal(outs[0], outs[1])
    assert torch.isfinite(outs[0]).all() and float(outs[0].abs().max()) <= 20.


@pytest.mark.parametrize("normalizer", ["affine", "monotonic"])
def test_dag_level_schedule_inversion_equals_fixed_point(normalizer):
    """inverting each variable once, in topological order, gives the values of the reference's
    depth()+1 full passes (NormalizingFlow.py:98-107)."""
    from models import DAGConditioner, AffineNormalizer, MonotonicNormalizer, buildFCNormalizingFlow
    torch.manual_seed(21)
    d = 9
    if normalizer == "affine":
        flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [24, 24], "out_size": 2,
                                                          "hot_encoding": True}, AffineNormalizer, {})
    else:
        flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [24, 24], "out_size": 6,
                                                          "hot_encoding": True},
                                      MonotonicNormalizer, {"integrand_net": [16, 16], "cond_size": 6,
                                                            "nb_steps": 20, "solver": "CC"})
    cond = flow.steps[0].conditioner
    # non-negative entries: depth() of the reference counts A > 0 edges only (post-processed A is 0/1)
    cond.A.data.copy_(torch.tril(torch.rand(d, d) + .1, -1) * (torch.rand(d, d) < .5).float())
    cond.stoch_gate = False
    flow = flow.to(DEV)
    z = cu(torch.randn(16, d) * .7)
    step = flow.steps[0]
    step.level_schedule = True
    x_lvl = step.invert(z)
    step.level_schedule = False
    x_it = step.invert(z)
    # Affine: identical up to fp32 rounding of the importance table.  Monotonic: every variable is a 20-step bisection
    # (resolution 1.9e-5) whose quantisation error is amplified from level to level, in both schedules alike.
    assert rel_err(x_lvl.cpu(), x_it.cpu()) < (1e-6 if normalizer == "affine" else 5e-3)
    with torch.no_grad():
        zz, _ = flow(x_lvl)
    assert rel_err(zz.cpu(), z.cpu()) < (1e-4 if normalizer == "affine" else 2e-3)   # bisection resolution 1.9e-5 abs


# --------------------------------------------------------------------------------- small-batch Linear kernels
@pytest.mark.parametrize("M,N,K", [(1, 16, 16), (7, 40, 48), (100, 1024, 784), (100, 1568, 1024), (128, 96, 160),
                                   (37, 150, 2), (129, 64, 64), (100, 30, 50)])
@pytest.mark.parametrize("mask_kind", ["none", "full", "deg", "deg_strict"])
def test_linear_layer_kernels_vs_torch(M, N, K, mask_kind):
    """gnf_linear_fwd / _bwd_x / _bwd_w (gnf_linear.hip: weight-streaming kernels for M <= 128 with the MADE mask as a
    degree rule or as a tensor; the tiled GEMM otherwise, e.g. M = 129 or K = 50) against F.linear(x, mask * W, b) and its
    autograd on the CPU (AutoregressiveConditioner.py:24-25)."""
    from gnf_hip import ops
    g = torch.Generator().manual_seed(M * 1000 + N + K)
    x = torch.randn(M, K, generator=g)
    W, b = torch.randn(N, K, generator=g) / K ** .5, torch.randn(N, generator=g) * .1
    W2, b2 = torch.randn(N, N, generator=g) / N ** .5, torch.randn(N, generator=g) * .1
    gy = torch.randn(M, N, generator=g)
    masks = degs = None
    m1 = m2 = None
    if mask_kind != "none":
        strict = mask_kind == "deg_strict"
        do1, di1 = torch.randint(0, 9, (N,), generator=g).float(), torch.randint(0, 9, (K,), generator=g).float()
        do2, di2 = torch.randint(0, 9, (N,), generator=g).float(), do1
        cmp = torch.lt if strict else torch.le
        m1, m2 = cmp(di1[None, :], do1[:, None]).float(), cmp(di2[None, :], do2[:, None]).float()
        if mask_kind == "full":                            # an arbitrary 0/1 pattern: no degree structure
            m1 = (torch.rand(N, K, generator=g) < .6).float()
            m2 = (torch.rand(N, N, generator=g) < .6).float()
        else:
            degs = [(cu(do1), cu(di1), strict), (cu(do2), cu(di2), strict)]
        masks = [cu(m1), cu(m2)]
    # two layers: the first one's backward exercises the gated data gradient of the second
    xr, Wr, br, W2r, b2r = (t.clone().requires_grad_(True) for t in (x, W, b, W2, b2))
    h = torch.relu(torch.nn.functional.linear(xr, Wr * m1 if m1 is not None else Wr, br))
    y0 = torch.nn.functional.linear(h, W2r * m2 if m2 is not None else W2r, b2r)
    (y0 * gy).sum().backward()
    xg, Wg, bg, W2g, b2g = (req(t) for t in (x, W, b, W2, b2))
    y = ops.mlp(xg, [(Wg, bg), (W2g, b2g)], masks, degs=degs)
    assert_close(y, y0, rtol=1e-5, atol=2e-5, what="y")
    (y * cu(gy)).sum().backward()
    for name, a, r in (("gx", xg, xr), ("gW1", Wg, Wr), ("gb1", bg, br), ("gW2", W2g, W2r), ("gb2", b2g, b2r)):
        assert rel_err(a.grad.cpu(), r.grad) < GTOL, (name, rel_err(a.grad.cpu(), r.grad))
        if name.startswith("gW") and m1 is not None:       # masked-out weights get an exactly-zero gradient
            mk = m1 if name == "gW1" else m2
            assert int(((a.grad.cpu() != 0) & (mk == 0)).sum()) == 0


@pytest.mark.parametrize("M,N,K", [(100, 1024, 784), (9, 48, 32), (130, 64, 64)])
@pytest.mark.parametrize("frozen", ["input", "weights"])
def test_linear_layer_single_gradient_launches(M, N, K, frozen):
    """gnf_linear_bwd runs both gradients of a layer in one launch; a layer whose input (the first MADE layer: x carries
    no gradient) or whose weights (a frozen conditioner) need none goes through gnf_linear_bwd_w / _bwd_x alone."""
    from gnf_hip import ops
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g)
    W, b = torch.randn(N, K, generator=g) / K ** .5, torch.randn(N, generator=g) * .1
    do, di = torch.randint(0, 5, (N,), generator=g).float(), torch.randint(0, 5, (K,), generator=g).float()
    m = (di[None, :] <= do[:, None]).float()
    gy = torch.randn(M, N, generator=g)
    xr, Wr, br = (t.clone().requires_grad_(True) for t in (x, W, b))
    (torch.nn.functional.linear(xr, Wr * m, br) * gy).sum().backward()
    xg = cu(x).requires_grad_(frozen != "input")
    Wg, bg = (cu(t).requires_grad_(frozen != "weights") for t in (W, b))
    y = ops.mlp(xg, [(Wg, bg)], [cu(m)], degs=[(cu(do), cu(di), False)])
    (y * cu(gy)).sum().backward()
    if frozen == "input":
        assert xg.grad is None
        assert rel_err(Wg.grad.cpu(), Wr.grad) < GTOL and rel_err(bg.grad.cpu(), br.grad) < GTOL
    else:
        assert Wg.grad is None and bg.grad is None
        assert rel_err(xg.grad.cpu(), xr.grad) < GTOL


@pytest.mark.parametrize("M,H,N", [(4099, 128, 30), (2048, 64, 32), (78400, 128, 30), (3000, 128, 1), (2500, 64, 17),
                                   (60000, 60, 60), (5003, 60, 30), (2100, 12, 30), (2500, 64, 64), (3000, 128, 64),
                                   (2049, 4, 33), (2600, 100, 50),
                                   # below 2048 rows only the FORWARD takes the tall kernel (a level of a sampling pass: a
                                   # few hundred rows through fc2), the gradients stay on the tiled GEMM
                                   (129, 128, 30), (700, 128, 30), (1999, 64, 17), (333, 12, 60)])
def test_linear_tall_narrow_layers(M, H, N):
    """gnf_linear_tall.hip: the fc2 shape of the headline model (78 400 x 128 -> 30), the DAGMLP layers of cfg2
    (60 000 x 12 -> 60 -> 60 -> 60 -> 30, DAGConditioner.py:7-20) and their relatives (N <= 64, K <= 128 a multiple of
    4) -- forward with the weight resident in registers, both gradients + the ReLU gate of the layer's input in one
    launch -- against F.linear and its autograd in fp64 on the CPU, as both layers of a chain (the second gated) and
    alone."""
    from gnf_hip import ops
    g = torch.Generator().manual_seed(M + H + N)
    x = torch.randn(M, 24, generator=g)
    W1, b1 = torch.randn(H, 24, generator=g) / 24 ** .5, torch.randn(H, generator=g) * .1
    W2, b2 = torch.randn(N, H, generator=g) / H ** .5, torch.randn(N, generator=g) * .1
    gy = torch.randn(M, N, generator=g)
    ref = [t.double().requires_grad_(True) for t in (x, W1, b1, W2, b2)]
    h = torch.relu(torch.nn.functional.linear(ref[0], ref[1], ref[2]))
    y0 = torch.nn.functional.linear(h, ref[3], ref[4])
    (y0 * gy.double()).sum().backward()
    dev = [req(t) for t in (x, W1, b1, W2, b2)]
    y = ops.mlp(dev[0], [(dev[1], dev[2]), (dev[3], dev[4])])
    assert_close(y, y0.float(), rtol=1e-5, atol=2e-5, what="y")
    (y * cu(gy)).sum().backward()
    for name, a, r in zip(("gx", "gW1", "gb1", "gW2", "gb2"), dev, ref):
        assert rel_err(a.grad.cpu(), r.grad.float()) < GTOL, (name, rel_err(a.grad.cpu(), r.grad.float()))
    # alone (no gate), input and weights needing gradients
    hd = h.detach().float()
    hr = hd.double().requires_grad_(True)
    W2r, b2r = ref[3].detach().clone().requires_grad_(True), ref[4].detach().clone().requires_grad_(True)
    (torch.nn.functional.linear(hr, W2r, b2r) * gy.double()).sum().backward()
    hg, W2g, b2g = req(hd), req(W2), req(b2)
    (ops.mlp(hg, [(W2g, b2g)]) * cu(gy)).sum().backward()
    for name, a, r in (("gx", hg, hr), ("gW", W2g, W2r), ("gb", b2g, b2r)):
        assert rel_err(a.grad.cpu(), r.grad.float()) < GTOL, (name, rel_err(a.grad.cpu(), r.grad.float()))


@pytest.mark.parametrize("M,N,K", [(100, 64, 48), (300, 40, 24), (4099, 30, 128)])
def test_linear_bwd_entry_with_column_sums(M, N, K):
    """gnf_linear_bwd through the C ABI with `gxsum` (the column sums of the data gradient = the bias gradient of the
    layer below): produced by the same launch on the tall-batch path (gnf_linear_gxsum_fused == 1), by a column-sum pass
    behind the small-batch / tiled paths -- against torch on the CPU; and the entry point's argument checks."""
    import ctypes
    from gnf_hip import abi
    lib = abi.load()
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.relu(torch.randn(M, K, generator=g))
    W, gy = torch.randn(N, K, generator=g) / K ** .5, torch.randn(M, N, generator=g)
    gx0 = (gy.double() @ W.double()) * (a > 0)
    gW0, gb0 = gy.double().t() @ a.double(), gy.double().sum(0)
    ad, Wd, gd = cu(a), cu(W), cu(gy)
    gx, gW, gb, gxs = (torch.empty(s, device=DEV) for s in ((M, K), (N, K), (N,), (K,)))
    nws = lib.gnf_linear_ws_bytes(M, N, K)
    ws = torch.empty(max(nws // 4, 1), device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = abi.stream()
    args = lambda **o: [P(gd), P(Wd), P(ad), None, None, None, 0, P(ad), o.get("gx", P(gx)), o.get("gW", P(gW)), P(gb), P(gxs), M, N, K,
                        P(ws), o.get("nws", nws), st]
    assert lib.gnf_linear_bwd(*args()) == 0
    fused = lib.gnf_linear_gxsum_fused(M, N, K, 0)
    assert fused == (1 if (M >= 2048 and N <= 64 and K <= 128 and K % 4 == 0) else 0)
    for name, t, r in (("gx", gx, gx0), ("gW", gW, gW0), ("gb", gb, gb0), ("gxsum", gxs, gx0.sum(0))):
        assert rel_err(t.cpu(), r.float()) < GTOL, (name, rel_err(t.cpu(), r.float()))
    assert lib.gnf_linear_bwd(*args(gW=None)) == -1                      # GNF_EINVAL
    assert lib.gnf_linear_bwd(*args(gx=None)) == -1
    if fused:
        assert lib.gnf_linear_bwd(*args(nws=16)) == -3                   # GNF_EWS: the partials do not fit


def test_made_degree_rule_is_verified_against_the_mask_buffer():
    """MaskedLinear hands the kernels its degree vectors only while the mask buffer equals the degree rule; a mask that
    was overwritten (a checkpoint, a user's own pattern) is read as a tensor again, and the result follows it."""
    from models import AutoregressiveConditioner
    torch.manual_seed(3)
    cond = AutoregressiveConditioner(12, [32, 32], 2).to(DEV)
    layers = cond.masked_autoregressive_net.masked_layers()
    assert all(l.degree_spec() is not None for l in layers)
    sd = cond.state_dict()
    assert not any("deg_" in k for k in sd)                   # the reference's checkpoint keys, nothing more
    x = torch.randn(9, 12, device=DEV)
    h0 = cond(x)
    with torch.no_grad():
        layers[1].mask.copy_((torch.rand_like(layers[1].mask) < .5).float())
    assert layers[1].degree_spec() is None and layers[0].degree_spec() is not None
    h1 = cond(x)
    ref = x
    for k, l in enumerate(layers):
        ref = torch.nn.functional.linear(ref, l.weight * l.mask, l.bias)
        if k < len(layers) - 1:
            ref = torch.relu(ref)
    ref = ref.view(9, -1, 12).permute(0, 2, 1)
    assert_close(h1, ref, rtol=1e-5, atol=1e-5, what="h with an arbitrary mask")
    assert (h1 - h0).abs().max() > 1e-3


# --------------------------------------------------------------------------------- fused tail of a flow step
@pytest.mark.parametrize("B,d", [(7, 5), (33, 63), (5000, 63), (4200, 64), (9000, 30), (400, 784), (3, 1)])
def test_nll_reduce_vs_torch(B, d):
    """gnf_nll_reduce (log(jac).sum(1) and the Normal log-density in one pass; models/NormalizingFlow.py:70,
    NormalizingFlowFactories.py:15-16) and its one-launch backward, on the row-group and the span-per-wavefront kernels
    (B d >= 2^18, d <= 64: d = 63 -> 4 rows per span, 30 -> 2, 64 -> 1)."""
    from gnf_hip import ops
    g = torch.Generator().manual_seed(B + d)
    z = torch.randn(B, d, generator=g)
    jac = torch.rand(B, d, generator=g) * 3 + .05
    gl, gn = torch.randn(B, generator=g), torch.randn(B, generator=g)
    zr, jr = z.clone().double().requires_grad_(True), jac.clone().double().requires_grad_(True)
    ld0 = torch.log(jr).sum(1)
    ln0 = O.normal_log_density(zr)
    ((ld0 * gl.double()).sum() + (ln0 * gn.double()).sum()).backward()
    zg, jg = req(z), req(jac)
    ld, ln = ops.NllReduceFn.apply(zg, jg)
    assert_close(ld, ld0.detach().float(), rtol=2e-6, atol=1e-5 * d ** .5, what="logdet")
    assert_close(ln, ln0.detach().float(), rtol=2e-6, atol=1e-5 * d ** .5, what="logN")
    ((ld * cu(gl)).sum() + (ln * cu(gn)).sum()).backward()
    assert_close(zg.grad, zr.grad.float(), rtol=1e-6, atol=1e-7, what="gz")
    assert_close(jg.grad, jr.grad.float(), rtol=2e-6, atol=1e-7, what="gjac")
    # the stand-alone entry points run on the same kernels
    assert torch.equal(ops.NormalLogDensityFn.apply(cu(z)), ln.detach())
    assert torch.equal(ops.LogSumRowsFn.apply(cu(jac)), ld.detach())


@pytest.mark.parametrize("B,d,layout", [(9, 7, "contig"), (6000, 63, "contig"), (64, 40, "made")])
def test_affine_fused_normal_log_density(B, d, layout):
    """AffineFn with the Normal log-density of z reduced in the same pass (want_logn) and its cotangent folded into
    the backward (z recomputed): against plain torch on the CPU."""
    from gnf_hip import ops
    g = torch.Generator().manual_seed(17 * B + d)
    x = torch.randn(B, d, generator=g)
    hraw = torch.randn(B, 2 * d, generator=g) * 2.5 if layout == "made" else torch.randn(B, d, 2, generator=g) * 2.5
    gzv, gl, gn = torch.randn(B, d, generator=g), torch.randn(B, generator=g), torch.randn(B, generator=g)
    xr, hr = x.clone().requires_grad_(True), hraw.clone().requires_grad_(True)
    hv = hr.view(B, 2, d).permute(0, 2, 1) if layout == "made" else hr
    mu, ls = torch.clamp(hv[:, :, 0], -5., 5.), torch.clamp(hv[:, :, 1], -5., 2.)
    z0 = xr * torch.exp(ls) + mu
    ld0, ln0 = ls.sum(1), O.normal_log_density(z0)
    ((z0 * gzv).sum() + (ld0 * gl).sum() + (ln0 * gn).sum()).backward()
    xg, hg = req(x), req(hraw)
    hgv = hg.view(B, 2, d).permute(0, 2, 1) if layout == "made" else hg
    z, _, ld, ln = ops.AffineFn.apply(xg, hgv, False, False, True)
    assert_close(z, z0, what="z")
    assert_close(ld, ld0, atol=1e-5, what="logdet")
    assert_close(ln, ln0, rtol=2e-6, atol=1e-4, what="logN")
    ((z * cu(gzv)).sum() + (ld * cu(gl)).sum() + (ln * cu(gn)).sum()).backward()
    assert rel_err(xg.grad.cpu(), xr.grad) < GTOL and rel_err(hg.grad.cpu(), hr.grad) < GTOL


def test_flow_loss_in_one_launch_equals_the_separate_evaluation():
    """flow.loss(z, logdet) -- the Normal log-density of z, the batch mean and the constraints term in ONE launch that reads
    z itself (gnf_hip.ops.NllLossFn) -- gives the value and the gradients of the separate evaluation
    constraints - (logdet + z_log_density(z)).mean() (reference NormalizingFlow.py:144-146)."""
    from models import buildFCNormalizingFlow, AutoregressiveConditioner, AffineNormalizer, MonotonicNormalizer
    from gnf_hip import ops
    for norm_t, args in ((AffineNormalizer, {}), (MonotonicNormalizer, {"integrand_net": [16, 16], "cond_size": 6})):
        torch.manual_seed(5)
        hs = 2 if norm_t is AffineNormalizer else 6
        flow = buildFCNormalizingFlow(2, AutoregressiveConditioner, {"in_size": 9, "hidden": [32, 32], "out_size": hs},
                                      norm_t, args).to(DEV)
        x = torch.randn(21, 9, device=DEV)
        z, ld = flow(x)
        loss = flow.loss(z, ld)
        assert type(loss.grad_fn).__name__ == "NllLossFnBackward"
        fresh = flow.constraintsLoss() - (ld + ops.NormalLogDensityFn.apply(z.detach())).mean()
        assert abs(loss.item() - fresh.item()) <= 1e-6 * max(1., abs(fresh.item()))
        ref = -(ld.detach().cpu().double() + O.normal_log_density(z.detach().cpu().double())).mean()
        assert abs(loss.item() - ref.item()) <= 1e-6 * max(1., abs(ref.item()))
        loss.backward()
        g1 = [p.grad.clone() for p in flow.parameters()]
        for p in flow.parameters():
            p.grad = None
        z2, ld2 = flow(x)
        (flow.constraintsLoss() - (ld2 + ops.NormalLogDensityFn.apply(z2)).mean()).backward()
        for a, b in zip(g1, (p.grad for p in flow.parameters())):
            assert rel_err(a.cpu(), b.cpu()) < 1e-5


@pytest.mark.parametrize("B,d", [(1, 1), (5, 3), (100, 784), (2, 784), (1000, 63), (16644, 63)])
def test_nll_loss_entry_points_vs_torch(B, d):
    """gnf_nll_loss_fwd / _bwd (the flat one-workgroup form) against torch on the CPU in fp64, with and without the
    addend; above gnf_nll_loss_max_elems() the entry point refuses and the flow takes the row kernels"""
    from gnf_hip import ops, abi
    g = torch.Generator().manual_seed(B + d)
    z, ld, c = torch.randn(B, d, generator=g) * 1.3, torch.randn(B, generator=g) * 5, torch.randn((), generator=g)
    for addend in (None, c):
        zr, lr = z.double().requires_grad_(True), ld.double().requires_grad_(True)
        ref = (0. if addend is None else addend.double()) - (lr + O.normal_log_density(zr)).mean()
        ref.backward()
        zg, lg = req(z), req(ld)
        out = ops.NllLossFn.apply(zg, lg, None if addend is None else cu(addend))
        assert abs(out.item() - ref.item()) <= 2e-6 * max(1., abs(ref.item())), (out.item(), ref.item())
        out.backward()
        assert_close(zg.grad, zr.grad, rtol=1e-6, atol=1e-9, what="gz")
        assert_close(lg.grad, lr.grad, rtol=1e-6, atol=1e-12, what="glogdet")
    assert ops.nll_loss_fits(cu(z))
    big = torch.empty(1 << 11, (1 << 9) + 1, device=DEV)
    assert not ops.nll_loss_fits(big)
    assert abi.load().gnf_nll_loss_fwd(big.data_ptr(), big.data_ptr(), None, big.data_ptr(), big.shape[0], big.shape[1], None) == -2


@pytest.mark.parametrize("norm_kind", ["affine", "monotonic"])
def test_loss_and_density_read_the_z_they_are_handed(norm_kind):
    """No density is remembered from the forward pass: after ANY rewrite of z -- an in-place op, or a write through `.data`
    that moves neither the version counter nor the address (the idiom of the reference's own DAGConditioner.py:89 and of
    torch-1.5-era callers; until round 4 such a z was scored with the density of its old contents) -- z_log_density(z) and
    flow.loss(z, logdet) are those of the new contents, as in the reference (NormalizingFlowFactories.py:15-16)."""
    from models import buildFCNormalizingFlow, AutoregressiveConditioner, AffineNormalizer, MonotonicNormalizer
    torch.manual_seed(5)
    norm_t, args, hs = ((AffineNormalizer, {}, 2) if norm_kind == "affine" else
                        (MonotonicNormalizer, {"integrand_net": [16, 16], "cond_size": 6, "nb_steps": 15, "solver": "CC"}, 6))
    flow = buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": 9, "hidden": [32, 32], "out_size": hs},
                                  norm_t, args).to(DEV)
    x = torch.randn(33, 9, device=DEV)
    with torch.no_grad():
        z, ld = flow(x)
        fresh = O.normal_log_density(z.cpu())
        assert_close(flow.z_log_density(z), fresh, what="density")
        for k, write in enumerate((lambda t: t.add_(1.), lambda t: t.data.add_(1.), lambda t: t.data.mul_(.5))):
            version = z._version
            write(z)
            assert (z._version == version) == (k > 0)         # the .data writes are invisible to autograd's counter
            moved = O.normal_log_density(z.cpu())
            assert (moved - fresh).abs().max() > .1            # the test would be blind otherwise
            assert_close(flow.z_log_density(z), moved, what="density after write %d" % k)
            want = (-(ld.cpu() + moved).mean()).item()
            assert abs(flow.loss(z, ld).item() - want) < 1e-5 * max(1., abs(want)), k
            fresh = moved


def test_made_sampled_ordering_golden():
    """MADE(random=True, num_masks=3) under its second mask set: h and every gradient against the reference's
    (tests/golden/made_random.npz); the masks are degree rules, so the small-batch kernels evaluate them from the degrees."""
    from models.Conditionners.AutoregressiveConditioner import MADE
    g = load_golden("made_random")
    cfg = [int(v) for v in g["perm.cfg"].tolist()]
    net = MADE(cfg[0], cfg[4:], cfg[1], num_masks=cfg[2], natural_ordering=bool(cfg[3]), random=True)
    net.load_state_dict({k[len("perm.p."):]: v for k, v in g.items() if k.startswith("perm.p.")}, strict=False)
    net.update_masks()                                           # -> the second of the three orderings
    net = net.to(DEV)
    for k, layer in enumerate(net.masked_layers()):
        assert torch.equal(layer.mask.cpu().to(torch.uint8), g["perm.mask1.%d" % k].to(torch.uint8))
    x = req(g["perm.x"])
    h = net(x)
    assert_close(h, g["perm.h"], what="h")
    (h * cu(g["perm.gh"])).sum().backward()
    assert rel_err(x.grad.cpu(), g["perm.gx"]) < GTOL
    for name, p in net.named_parameters():
        assert rel_err(p.grad.cpu(), g["perm.g." + name]) < GTOL, name


def test_dag_hutchinson_trace_estimator():
    """DAGConditioner.get_power_trace with `hutchinson = h_iter` (reference DAGConditioner.py:179-190): with injected probe
    vectors the estimate equals the reference expression evaluated in fp64; with its own draws it scatters around the exact
    tr((I + alpha A o A)^d) - d; gradients reach A."""
    from models import DAGConditioner
    torch.manual_seed(4)
    d = 6
    c = DAGConditioner(d, [8, 8], 2).to(DEV)
    with torch.no_grad():
        c.A.copy_((torch.rand(d, d) * .9 * (1 - torch.eye(d))).to(DEV))
    alpha = min(1., float(c.alpha)) * c.alpha_factor
    Bm = torch.eye(d, dtype=torch.float64) + alpha * c.A.detach().cpu().double() ** 2
    exact = torch.linalg.matrix_power(Bm, d).diagonal().sum().item() - d
    c.hutchinson = 4
    noise = torch.randn(4, d)
    c.hutchinson_noise = noise
    tr = c.get_power_trace()
    e0 = noise.double().t()
    ref = ((e0 * (torch.linalg.matrix_power(Bm, d) @ e0)).sum() / 4 - d).item()
    assert abs(tr.item() - ref) < 1e-5 * max(1., abs(ref)), (tr.item(), ref)
    tr.backward()
    assert c.A.grad is not None and torch.isfinite(c.A.grad).all() and float(c.A.grad.abs().max()) > 0
    c.hutchinson_noise = None
    c.hutchinson = 4000
    with torch.no_grad():
        est = c.get_power_trace().item()
    assert abs(est - exact) < .15 * max(1., abs(exact) + d), (est, exact)
    c.hutchinson = 0
    with torch.no_grad():
        assert abs(c.get_power_trace().item() - (torch.linalg.matrix_power(Bm, c.exponent).diagonal().sum().item() - d)) < 1e-4


def test_loss_calls_a_subclassed_base_density():
    """FCNormalizingFlow.loss folds the base density into its own launch only for the factories' NormalLogDensity itself: a
    subclass that overrides forward (a tempered density here) inherits the class attribute but must be CALLED, as the
    reference calls whatever z_log_density is (NormalizingFlow.py:144-146) -- round-5 advisor finding."""
    from models import buildFCNormalizingFlow, CouplingConditioner, AffineNormalizer
    from models.NormalizingFlowFactories import NormalLogDensity

    class Tempered(NormalLogDensity):
        def forward(self, z):
            return super().forward(z) * .5 - 3.

    torch.manual_seed(2)
    flow = buildFCNormalizingFlow(1, CouplingConditioner, {"in_size": 6, "hidden": [16, 16], "out_size": 2},
                                  AffineNormalizer, {}).to(DEV)
    x = torch.randn(40, 6, device=DEV)
    z, ld = flow(x)
    plain = flow.loss(z, ld).item()
    want_plain = (-(ld.detach().cpu() + O.normal_log_density(z.detach().cpu())).mean()).item()
    assert abs(plain - want_plain) < 1e-5 * max(1., abs(want_plain))
    flow.z_log_density = Tempered().to(DEV)
    got = flow.loss(z, ld).item()
    want = (-(ld.detach().cpu() + O.normal_log_density(z.detach().cpu()) * .5 - 3.).mean()).item()
    assert abs(want - want_plain) > .1 and abs(got - want) < 1e-5 * max(1., abs(want)), (got, want, plain)


# --------------------------------------------------------------------------------- Monotonic vs oracle
def _mono_case(B, d, c, hidden, S, seed, h_layout="contig"):
    from models import MonotonicNormalizer
    torch.manual_seed(seed)
    norm = MonotonicNormalizer(hidden, c, nb_steps=S, solver="CC")
    x = torch.randn(B, d) * 1.5
    if h_layout == "made":
        hraw = torch.randn(B, c * d)
        h = hraw.view(B, c, d).permute(0, 2, 1)
    else:
        hraw = torch.randn(B, d, c)
        h = hraw
    return norm, x, hraw, h


def _layers_cpu(norm):
    ps = [p.detach().cpu().clone() for p in norm.integrand_net.flat_params()]
    return [(ps[i], ps[i + 1]) for i in range(0, len(ps), 2)]


@pytest.mark.parametrize("hidden,S,layout", [([10], 20, "contig"), ([16, 16], 21, "made"), ([50, 50, 50], 20, "contig"),
                                              ([50, 50, 50], 29, "made"), ([100, 100, 100], 20, "contig"),
                                              ([150, 150, 150], 20, "made"), ([40, 64, 24], 15, "contig"),
                                              ([200, 200], 22, "contig"),
                                              # wide nets whose layers end in DIFFERENT k-steps of their last unit tile (the
                                              # pack's K order and the truncated contractions, MonoLayout::perm): 97 -> 1 of
                                              # 4 k-steps of tile 6, 110 -> all 4 minus 2 units, 101 -> 2;  145 / 158 / 147
                                              ([97, 110, 101], 20, "contig"), ([145, 158, 147], 20, "made"),
                                              # layers whose last real tile is not the padded image's last tile (HP = 160)
                                              ([100, 150, 100], 20, "contig"),
                                              # four hidden layers: narrow -> bias gradients through the ones column of the
                                              # staged activations (image + tiles exceed the LDS); wide (the reference's
                                              # default integrand) -> one hidden matrix swapped through LDS at a time
                                              ([48, 50, 50, 50], 20, "contig"), ([100, 100, 100, 100], 20, "made")])
def test_monotonic_forward_backward_vs_oracle(hidden, S, layout):
    B, d, c = 9, 7, 30 if len(hidden) == 3 else 5
    norm, x, hraw, h = _mono_case(B, d, c, hidden, S, seed=len(hidden) * 100 + S, h_layout=layout)
    layers = _layers_cpu(norm)
    # oracle (fp32) and an fp64 oracle to measure what fp32 roundoff alone allows
    xr, hr = x.clone().requires_grad_(True), hraw.clone().requires_grad_(True)
    lr = [(W.clone().requires_grad_(True), b.clone().requires_grad_(True)) for W, b in layers]
    hview = hr.view(B, c, d).permute(0, 2, 1) if layout == "made" else hr
    z0, j0 = O.monotonic_forward(xr, hview, lr, S)
    gz, gj = torch.randn(B, d), torch.randn(B, d)
    ((z0 * gz).sum() + (torch.log(j0) * gj).sum()).backward()

    norm = norm.to(DEV)
    xg, hg = req(x), cu(hraw).requires_grad_(True)
    hgv = hg.view(B, c, d).permute(0, 2, 1) if layout == "made" else hg
    z, jac = norm(xg, hgv)
    assert rel_err(z.cpu(), z0.detach()) < TOL, rel_err(z.cpu(), z0.detach())
    assert_fwd(z, z0.detach(), what='z')
    assert rel_err(jac.cpu(), j0.detach()) < TOL
    assert_fwd(jac, j0.detach(), what='jac')
    assert_close(z, z0, atol=2e-6, what="z")               # element-wise (the integral sums ~20 terms of O(1))
    assert_close(jac, j0, what="jac")
    assert_close(torch.log(jac).sum(1), torch.log(j0.detach()).sum(1), what="logdet")
    ((z * cu(gz)).sum() + (torch.log(jac) * cu(gj)).sum()).backward()
    assert rel_err(xg.grad.cpu(), xr.grad) < GTOL
    assert rel_err(hg.grad.cpu(), hr.grad) < GTOL
    for (W, b), p_w, p_b in zip(lr, norm.integrand_net.flat_params()[0::2], norm.integrand_net.flat_params()[1::2]):
        assert rel_err(p_w.grad.cpu(), W.grad) < GTOL, ("W", tuple(W.shape), rel_err(p_w.grad.cpu(), W.grad))
        assert rel_err(p_b.grad.cpu(), b.grad) < GTOL, ("b", tuple(b.shape))
        # element-wise (verdict r04 item 5): |a - b| <= 1e-6 max|g| + 1e-4 |b| for every entry of every parameter gradient
        assert_close(p_w.grad, W.grad, rtol=1e-4, atol=1e-6 * W.grad.abs().max().item(), what="dW %s" % (tuple(W.shape),))
        assert_close(p_b.grad, b.grad, rtol=1e-4, atol=1e-6 * b.grad.abs().max().item(), what="db %s" % (tuple(b.shape),))
    assert_close(xg.grad, xr.grad, rtol=1e-4, atol=1e-6 * xr.grad.abs().max().item(), what="dx")
    assert_close(hg.grad, hr.grad, rtol=1e-4, atol=1e-6 * hr.grad.abs().max().item(), what="dh")


def test_monotonic_golden_jacobian():
    """Jacobian / log|det J| of a Monotonic flow: pinned by the reference itself."""
    from models import buildFCNormalizingFlow, AutoregressiveConditioner, MonotonicNormalizer
    g = load_golden("flow_mono_made_1")
    flow = buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": 4, "hidden": [12, 12], "out_size": 6},
                                  MonotonicNormalizer, {"integrand_net": [10, 10], "cond_size": 6, "nb_steps": 20,
                                                        "solver": "CC"})
    assert list(flow.state_dict().keys()) == list(g["state_keys"])
    flow = load_into(flow, g)
    x = cu(g["x"])
    h = flow.steps[0].conditioner(x)
    assert rel_err(h.cpu(), g["h"]) < TOL
    assert_fwd(h, g["h"], what='h')
    z, jac = flow.steps[0].normalizer(x, h)
    assert rel_err(jac.cpu(), g["jac"]) < TOL
    assert_fwd(jac, g["jac"], what='jac')
    _, ld = flow(x)
    assert rel_err(ld.cpu(), g["logdet"]) < TOL
    assert_fwd(ld, g["logdet"], what='ld')


def test_monotonic_golden_integrand_grads():
    from models import MonotonicNormalizer
    g = load_golden("integrand")
    norm = MonotonicNormalizer([16, 16, 16], 5, nb_steps=20)
    norm.integrand_net.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("p.")})
    norm = norm.to(DEV)
    x, h = req(g["x"]), req(g["h"])
    _, jac = norm(x, h)
    assert rel_err(jac.cpu(), g["jac"]) < TOL
    assert_fwd(jac, g["jac"], what='jac')
    (torch.log(jac) * cu(g["gj"])).sum().backward()
    assert rel_err(x.grad.cpu(), g["gx"]) < GTOL and rel_err(h.grad.cpu(), g["gh"]) < GTOL
    grads_match(norm.integrand_net, g)


def test_monotonic_inverse_vs_oracle_and_round_trip():
    norm, x, hraw, h = _mono_case(11, 5, 30, [50, 50, 50], 30, seed=5)
    layers = _layers_cpu(norm)
    z0, _ = O.monotonic_forward(x, h, layers, 30)
    x0 = O.monotonic_inverse(z0.detach(), h, layers, 30)
    norm = norm.to(DEV)
    xi = norm.inverse_transform(cu(z0.detach()), cu(h))
    # same bisection on nearly identical z(x): decisions can differ only by one last-step interval
    assert (xi.cpu() - x0).abs().max() <= 40. / 2 ** 20 + 1e-6
    assert (xi.cpu() - x).abs().max() < 1e-3


# --------------------------------------------------------------------------------- size-independent properties at full size
def test_full_size_cfg4_properties():
    """MNIST d=784, B=100, Monotonic [50,50,50] c=30: z strictly increasing in x, z(0) = h0,
    fixed-S determinism, and dz/dx ~ jac by central differences."""
    from models import MonotonicNormalizer
    torch.manual_seed(1)
    B, d, c = 100, 784, 30
    norm = MonotonicNormalizer([50, 50, 50], c, nb_steps=20).to(DEV)
    x = torch.randn(B, d, device=DEV)
    h = torch.randn(B, d, c, device=DEV)
    with torch.no_grad():
        z1, j1 = norm(x, h)
        z1b, _ = norm(x, h)
        assert torch.equal(z1, z1b)
        z2, _ = norm(x + .25, h)
        assert (z2 > z1).all() and (j1 > .05).all()
        z0, _ = norm(torch.zeros_like(x), h)
        assert torch.equal(z0, h[:, :, 0])
        norm.nb_steps = 150
        zp, _ = norm(x + 1e-2, h)
        zm, _ = norm(x - 1e-2, h)
        _, j = norm(x, h)
        assert (((zp - zm) / 2e-2 - j).abs() / j).max() < 5e-2


def test_full_size_cfg5_affine_roundtrip():
    from models import AffineNormalizer
    torch.manual_seed(2)
    B, d = 50000, 63
    x = torch.randn(B, d, device=DEV)
    h = torch.randn(B, d, 2, device=DEV) * 2
    n = AffineNormalizer()
    with torch.no_grad():
        z, jac = n(x, h)
        xr = n.inverse_transform(z, h)
    assert ((xr - x).abs() / (1 + x.abs())).max() < 1e-4


# --------------------------------------------------------------------------------- more coverage
def test_dag_noise_gate_vs_oracle():
    """noise gate branch (DAG:114-116) with explicit N(0,1) samples."""
    from gnf_hip import ops
    torch.manual_seed(3)
    B, d = 7, 9
    x, A, nz = torch.randn(B, d), torch.rand(d, d) * 1.2, torch.randn(B, d, d)
    xr, Ar = x.clone().requires_grad_(True), A.clone().requires_grad_(True)
    e0 = O.dag_masked_inputs(xr, Ar, True, 0., False, True, 1., None, None, nz, False)
    w = torch.randn_like(e0)
    (e0 * w).sum().backward()
    xg, Ag = req(x), req(A)
    e = ops.DagGateFn.apply(xg, Ag, ops.IMP_SOFT, ops.GATE_NOISE, 0., 1., False, cu(nz), None, 0, 0)
    assert rel_err(e.cpu(), e0.detach()) < TOL
    assert_fwd(e, e0.detach(), what='e')
    (e * cu(w)).sum().backward()
    assert rel_err(xg.grad.cpu(), xr.grad) < GTOL and rel_err(Ag.grad.cpu(), Ar.grad) < GTOL


def test_dag_flow_invert_round_trip():
    """A DAG conditioner whose A is a (post-processed) strictly lower-triangular 0/1 matrix is invertible:
    depth()+1 fixed-point passes recover x (NormalizingFlow.py:98-107, DAG:262-266)."""
    from models import buildFCNormalizingFlow, DAGConditioner, AffineNormalizer
    torch.manual_seed(5)
    d = 6
    flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [16, 16], "out_size": 2,
                                                      "A_prior": torch.tril(torch.ones(d, d), -1)},
                                  AffineNormalizer, {})
    cond = flow.steps[0].conditioner
    cond.stoch_gate, cond.noise_gate, cond.s_thresh, cond.h_thresh = False, False, False, 0.
    cond.is_invertible = True
    flow = flow.to(DEV)
    assert cond.depth() == d - 1
    x = torch.randn(32, d, device=DEV)
    with torch.no_grad():
        z, _ = flow(x)
        xr = flow.invert(z)
    assert rel_err(xr.cpu(), x.cpu()) < 1e-4


def test_abi_error_codes():
    import ctypes
    from gnf_hip import abi
    lib = abi.load()
    st = abi.stream()
    x = torch.zeros(4, 4, device=DEV)
    P = ctypes.c_void_p
    assert lib.gnf_affine_fwd(None, P(x.data_ptr()), 8, 2, 1, P(x.data_ptr()), None, None, None, 0, 2, 2, st) == -1
    # a degree rule needs both vectors; the small-batch Linear entry points validate like the others
    assert lib.gnf_linear_fwd(P(x.data_ptr()), P(x.data_ptr()), None, None, P(x.data_ptr()), None, 0, 0,
                              P(x.data_ptr()), 4, 4, 4, None, 0, st) == -1
    assert lib.gnf_gemm(P(x.data_ptr()), 4, 1, None, None, 1, 4, P(x.data_ptr()), 4, 1, None, None, 0, 0, None, 0, 0, 0,
                        4, 4, 4, None, 0, st) == -1
    net = abi.MonoNet()
    net.nl = 1                                  # needs >= 2 Linear layers
    assert lib.gnf_monotonic_pack_floats(ctypes.byref(net)) == -2
    net.nl = 2
    net.dims[0], net.dims[1], net.dims[2] = 4, 300, 1      # hidden wider than any compiled instantiation (256)
    assert lib.gnf_monotonic_pack_floats(ctypes.byref(net)) == -2
    with pytest.raises(abi.GnfError):
        abi.ptr(torch.zeros(2, dtype=torch.float64, device=DEV))
    # graph-capturable Adam and the ceiling probes validate their arguments the same way
    assert lib.gnf_adam_step_dev(P(x.data_ptr()), P(x.data_ptr()), P(x.data_ptr()), P(x.data_ptr()), 16, 1e-3, .9, .999,
                                 1e-8, 0., 1., None, 1, st) == -1
    assert lib.gnf_probe_copy(P(x.data_ptr()), P(x.data_ptr()), 6, st) == -1          # n must be a multiple of 4
    assert lib.gnf_probe_mfma_f32(None, 1, 1, st) == -1
    # the device-side step counter advances by one per call and the update equals the by-value entry point
    from gnf_hip import ops
    torch.manual_seed(2)
    p0, g0 = torch.randn(1000, device=DEV), torch.randn(1000, device=DEV)
    pa, ma, va = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    pb, mb, vb = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    step = torch.zeros(2, dtype=torch.int32, device=DEV)             # {steps taken, ticket counter of the last launch}
    for t in (1, 2, 3):
        ops.adam_step(pa, g0, ma, va, t, lr=1e-2, weight_decay=1e-4)
        ops.adam_step_dev(pb, g0, mb, vb, step, lr=1e-2, weight_decay=1e-4)
    assert step.tolist() == [3, 0] and rel_err(pb.cpu(), pa.cpu()) < 1e-6
    ops.adam_step_dev(pb, g0, mb, vb, step, lr=1e-2, weight_decay=1e-4, advance=False)
    assert step.tolist() == [3, 0]
    big = torch.randn(3_000_001, device=DEV)                          # many workgroups, scalar tail
    pc, mc, vc = big.clone(), torch.zeros_like(big), torch.zeros_like(big)
    pd, md, vd = big.clone(), torch.zeros_like(big), torch.zeros_like(big)
    for t in (4, 5):
        ops.adam_step(pc, big, mc, vc, t, lr=1e-2)
        ops.adam_step_dev(pd, big, md, vd, step, lr=1e-2)
    assert step.tolist() == [5, 0] and torch.equal(pc, pd)


@pytest.mark.parametrize("name,B", [("cfg1", 512), ("cfg2", 10000), ("cfg3", 100), ("cfg5", 2000)])
def test_baseline_configs_train_step(name, B):
    """every BASELINE.json configuration (cfg4 is the bench itself; cfg5 at a reduced batch to bound the test time):
    a full fwd + log|det J| + NLL + bwd step runs, the loss is finite, every parameter gets a finite gradient,
    and the log-likelihood decomposition loss = constraints - mean(logdet + logN(z)) holds."""
    from gnf_hip.configs import baseline_config
    flow, x = baseline_config(name)
    x = x[:B]
    for nrm in flow.getNormalizers():
        if hasattr(nrm, "nb_steps"):
            nrm.nb_steps = 20
    z, ld = flow(x)
    loss = flow.loss(z, ld)
    loss.backward()
    assert torch.isfinite(loss).item() and z.shape == x.shape and ld.shape == (x.shape[0],)
    ref = flow.constraintsLoss() - (ld + O.normal_log_density(z.detach().cpu()).to(DEV)).mean()
    assert abs(ref.item() - loss.item()) < 1e-4 * max(1., abs(loss.item()))
    for k, p in flow.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


@pytest.mark.parametrize("B,d,hidden", [(1, 1, [50, 50, 50]), (3, 7, [50, 50, 50]), (5, 13, [100, 100, 100]),
                                        (2, 9, [150, 150]), (70, 3, [100, 100, 100]),
                                        # more than one round of the 256 persistent workgroups with a ragged last round:
                                        # 8238 elements = 256 full groups of 32 + three HALF groups (16 elements x 4 nodes
                                        # per batch, the last one with 14 elements); 8220 = 256 + two half groups
                                        (1373, 6, [100, 100, 100]), (1370, 6, [150, 150]),
                                        # narrow nets above 2048 elements: d W1h = Dsum^T h and d b1 on the tall
                                        # weight-gradient kernel (gnf_linear_tall_wgrad) instead of GEMM + reductions
                                        (300, 7, [50, 50, 50]), (131, 17, [40, 64, 24]), (2049, 1, [16, 16]),
                                        # widest nets (H = 161..256, the UCI configs' [200,200,200]) on the same tall
                                        # first-layer path: the hidden-layer BIAS gradients are column sums of the staged
                                        # dpre rows and were skipped there (zero db_l) -- round-3 advisor finding
                                        (300, 7, [200, 200]), (420, 5, [200, 200, 200])])
def test_monotonic_ragged_sizes(B, d, hidden):
    """element counts that leave wavefronts of the last workgroup without a group of their own (and the wide-net
    weight-swapping mode, whose workgroups iterate in lockstep) -- regression for a staging clobber by tail waves; the
    wide nets' backward deals the elements of an unfilled last round as half groups (gnf_monotonic_wide.hip, WideSched)."""
    c, S = 30, 20
    # ReLU gates on the knife edge: with 2 100 elements x 22 nodes x 200 units x 3 layers a handful of pre-activations lie
    # within fp32 roundoff of zero and the gate differs between two correct fp32 evaluations; one flipped gate moves a row of
    # dW by ~1e-4 of the tensor's max (tests/dbg_mono_wide_grads.py: sometimes the torch fp32 oracle is the side that is
    # off).  An fp64 evaluation of the integrand net finds the elements that hold such a gate (0-4.4 % at these seeds for
    # H <= 150, 7.0 / 8.9 % for the [200]-wide nets); those elements (x[b,i], h[b,i,:]) are REDRAWN from the same generator until
    # none is left -- elements are independent -- so gz, gj are live everywhere and every gradient is compared at GTOL,
    # element-wise too.  The tied elements of the raw draw are judged against the fp64 gradient of one admissible gate
    # combination in tests/test_gpu_knife.py.  (Until round 4: 2e-3 for the widest nets; rounds 5-6: a zero cotangent for up to
    # 10 % of the elements.)
    (norm, x, h), redraw = knife_units.draw_monotonic(B, d, hidden, c, S)
    frozen = _layers_cpu(norm)
    (x, h), _ = knife_units.resample_off_ties(redraw, lambda x_, h_: integrand_knife_elements(x_, h_, frozen, S), first=(x, h))
    layers = [(W.clone().requires_grad_(True), b.clone().requires_grad_(True)) for W, b in frozen]
    xr, hr = x.clone().requires_grad_(True), h.clone().requires_grad_(True)
    z0, j0 = O.monotonic_forward(xr, hr, layers, S)
    assert int(integrand_knife_elements(x, h, frozen, S).sum()) == 0                # no tied element is left
    gz, gj = torch.randn(B, d), torch.randn(B, d)
    ((z0 * gz).sum() + (j0 * gj).sum()).backward()
    norm = norm.to(DEV)
    xg, hg = req(x), req(h)
    z, jac = norm(xg, hg)
    assert rel_err(z.cpu(), z0.detach()) < TOL and rel_err(jac.cpu(), j0.detach()) < TOL
    assert_fwd(z, z0.detach(), what='z')
    assert_fwd(jac, j0.detach(), what='jac')
    ((z * cu(gz)).sum() + (jac * cu(gj)).sum()).backward()
    assert rel_err(xg.grad.cpu(), xr.grad) < GTOL and rel_err(hg.grad.cpu(), hr.grad) < GTOL
    ps = norm.integrand_net.flat_params()
    for (W, b), pw, pb in zip(layers, ps[0::2], ps[1::2]):
        assert rel_err(pw.grad.cpu(), W.grad) < GTOL, ("W", tuple(W.shape), rel_err(pw.grad.cpu(), W.grad))
        assert rel_err(pb.grad.cpu(), b.grad) < GTOL, ("b", tuple(b.shape), rel_err(pb.grad.cpu(), b.grad))
        assert_close(pw.grad, W.grad, rtol=1e-4, atol=2e-6 * W.grad.abs().max().item(), what="dW %s" % (tuple(W.shape),))
        assert_close(pb.grad, b.grad, rtol=1e-4, atol=2e-6 * b.grad.abs().max().item(), what="db %s" % (tuple(b.shape),))


@pytest.mark.parametrize("B,d,hidden", [(4100, 6, [100, 100, 100]), (4099, 4, [150, 150])])
def test_monotonic_forward_half_groups(B, d, hidden):
    """the wide nets' forward kernel runs up to three persistent workgroups per CU; element counts just above a whole
    number of rounds (24 600 = 768 groups of 32 + two half groups; 16 396 = 512 + two, the second with 12 elements) take
    the half-group path (16 elements x 4 nodes per batch, the two node halves of an element summed in LDS)."""
    from models import MonotonicNormalizer
    torch.manual_seed(B + d)
    c, S = 30, 20
    norm = MonotonicNormalizer(hidden, c, nb_steps=S)
    x, h = torch.randn(B, d) * 1.5, torch.randn(B, d, c)
    with torch.no_grad():
        z0, j0 = O.monotonic_forward(x, h, _layers_cpu(norm), S)
        z, jac = norm.to(DEV)(cu(x), cu(h))
    assert rel_err(z.cpu(), z0) < TOL and rel_err(jac.cpu(), j0) < TOL
    assert_fwd(z, z0, what='z')
    assert_fwd(jac, j0, what='jac')
    assert_close(z, z0, atol=3e-6, what="z")
    assert_close(jac, j0, what="jac")


def test_train_uci_driver_and_checkpoint_formats(tmp_path):
    """train_uci.py (UCIExperiments.py's role): two epochs on synthetic POWER-shaped data; model.pt carries the
    reference's state_dict keys and ADAM.pt loads into torch.optim.Adam(model.parameters())."""
    import train_uci
    args = train_uci.parse(["-dataset", "power", "-data", "synthetic", "-folder", str(tmp_path), "-nb_epoch", "2",
                            "-b_size", "2000", "-conditioner", "DAG", "-emb_net", "20", "20", "6", "-normalizer",
                            "monotonic", "-int_net", "16", "16", "-nb_steps_dual", "30", "-l1", "0."])
    model = train_uci.train(args)
    lines = [l for l in open(tmp_path / "logs") if l.startswith("epoch")]
    assert len(lines) == 2
    losses = [float(l.split("Train loss:")[1].split()[0]) for l in lines]
    assert losses[1] < losses[0]                               # N(0,1) data: the NLL goes down from the random init
    sd = torch.load(tmp_path / "model.pt", map_location="cpu")
    assert list(sd.keys()) == list(model.state_dict().keys())
    fresh, _, _ = train_uci.build(args, 6)
    fresh.load_state_dict(sd)
    opt = torch.optim.Adam(fresh.parameters(), lr=1e-3, weight_decay=1e-5)
    opt.load_state_dict(torch.load(tmp_path / "ADAM.pt", map_location="cpu"))
    assert all("exp_avg" in st for st in opt.state_dict()["state"].values())
    # resuming restores the fused-Adam moments
    args2 = train_uci.parse(["-dataset", "power", "-data", "synthetic", "-folder", str(tmp_path), "-nb_epoch", "1",
                             "-b_size", "2000", "-conditioner", "DAG", "-emb_net", "20", "20", "6", "-normalizer",
                             "monotonic", "-int_net", "16", "16", "-nb_steps_dual", "30", "-l1", "0.", "-load"])
    train_uci.train(args2)
    lines = [l for l in open(tmp_path / "logs") if l.startswith("epoch")]
    assert float(lines[2].split("Train loss:")[1].split()[0]) < losses[0]


@pytest.mark.parametrize("kind", ["coupling", "made"])
def test_graphed_step_equals_eager_steps(kind):
    """gnf_hip.dp.GraphedStep (one hipGraph per optimisation step, Adam step count in device memory) follows the same
    parameter trajectory as dp.train_step issued launch by launch."""
    from gnf_hip import dp
    from models import (buildFCNormalizingFlow, CouplingConditioner, AutoregressiveConditioner, AffineNormalizer)

    def make():
        torch.manual_seed(5)
        if kind == "coupling":
            f = buildFCNormalizingFlow(2, CouplingConditioner, {"in_size": 4, "hidden": [32, 32], "out_size": 2},
                                       AffineNormalizer, {})
        else:
            f = buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": 12, "hidden": [64, 64], "out_size": 2},
                                       AffineNormalizer, {})
        return f.to(DEV)
    d = 4 if kind == "coupling" else 12
    xs = [cu(torch.randn(64, d, generator=torch.Generator().manual_seed(100 + i))) for i in range(4)]
    fa = make()
    sa = dp.FlatState(fa)
    for _ in range(3):
        dp.train_step(fa, sa, xs[0], lr=1e-2, graph=False)
    for x in xs:
        la = dp.train_step(fa, sa, x, lr=1e-2, graph=False)
    fb = make()
    sb = dp.FlatState(fb)
    gs = dp.GraphedStep(fb, sb, xs[0], lr=1e-2, warmup=3)
    for x in xs:
        lb = gs(x)
    torch.cuda.synchronize()
    assert sb.t == sa.t == 7 and int(gs.step_dev.item()) == 7
    # an eager graph of the same flow that is still referenced must not disturb the capture (its gradient accumulators
    # are bound to the default stream; GraphedStep differentiates w.r.t. fresh leaves instead)
    fc = make()
    z, ld = fc(xs[0])
    keep = fc.loss(z, ld)
    keep.backward()
    gc = dp.GraphedStep(fc, dp.FlatState(fc), xs[0])
    assert torch.isfinite(gc(xs[1])).item() and keep.requires_grad
    assert rel_err(lb.cpu(), la.detach().cpu()) < 1e-5
    assert rel_err(sb.flat.cpu(), sa.flat.cpu()) < 1e-5



# --------------------------------------------------------------------------------- sparse masked-image front (8(f)1)
def _windowed_conditioner(seed, post_processed):
    """DAGConditioner(MNISTCNN) on 28x28 with the kernel-2 prior; deterministic gate"""
    from models import DAGConditioner
    from models.MLP import MNISTCNN
    from models.NormalizingFlowFactories import MNIST_A_prior
    torch.manual_seed(seed)
    prior = MNIST_A_prior(28, 2)
    A = prior * (torch.rand(784, 784) < .7).float() * (.5 + torch.rand(784, 784))
    cond = DAGConditioner(784, MNISTCNN(out_d=30), 30, A_prior=A.clone()).to(DEV)
    cond.stoch_gate = False                        # deterministic soft-thresholded importance
    if post_processed:                             # what post_process() leaves: binary A, raw product
        cond.s_thresh, cond.h_thresh = False, 0.
        cond.A.data = (cond.A.data != 0).float()
        cond.A.requires_grad = False
    with torch.no_grad():
        for p in cond.embedding_net.parameters():  # biases of both signs: background relu(b) partly 0, partly > 0
            if p.dim() == 1:
                p.copy_(torch.randn_like(p) * .3)
    return cond


def _knife_edge_windows(cond, x, with_images=False):
    """Pool windows of the dense (tie-exact) forward whose recorded argmax differs from torch-CPU's on the same masked
    copies.  Exact ties are decided identically (first maximum); what remains are windows whose two largest values are
    EQUAL IN EXACT ARITHMETIC but come from different patches, so that each fp32 evaluation order rounds them apart by
    an ulp its own way -- no implementation can follow another's choice there.  Returns their number after checking IN FP64
    that every one of them is such a near-tie (top two values within 16 fp32 ulps of their terms' magnitude); with_images:
    also the indices (b * 784 + i) of the masked copies that hold one -- the parity tests give those a zero cotangent
    instead of loosening the tolerance of the gradients."""
    import torch.nn.functional as F
    from gnf_hip import abi
    from conftest import EPS32
    net = cond.embedding_net
    B = x.shape[0]
    e = (x.cpu().unsqueeze(1) * cond.deterministic_importance().detach().cpu().unsqueeze(0)).reshape(B * 784, 784)
    W1, b1, W2, b2 = [t.detach().cpu() for t in (net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv2.bias)]
    c2 = F.conv2d(torch.relu(F.conv2d(e.view(-1, 1, 28, 28), W1, b1)), W2, b2)
    _, idx = F.max_pool2d(c2, 2, return_indices=True)
    ref = (((idx // 24) % 2) * 2 + (idx % 24) % 2).flatten(1)
    dev = [t.to(DEV).contiguous() for t in (e, W1, b1, W2, b2)]
    pooled = torch.empty(B * 784, 2304, device=DEV)
    arg = torch.empty(B * 784, 2304, dtype=torch.uint8, device=DEV)
    abi.call("gnf_mnistcnn_conv_fwd", *[abi.ptr(t) for t in dev], abi.ptr(pooled), abi.rawptr(arg), B * 784, 1,
             abi.stream())
    flips = (arg.cpu().long() != ref).nonzero()
    if flips.shape[0]:
        imgs = flips[:, 0].unique()
        a1 = torch.relu(F.conv2d(e[imgs].double().view(-1, 1, 28, 28), W1.double(), b1.double()))
        c64 = F.conv2d(a1, W2.double(), b2.double())
        mag = F.conv2d(a1, W2.double().abs(), b2.double().abs())
        win = c64.view(-1, 16, 12, 2, 12, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 2304, 4)
        wmag = mag.view(-1, 16, 12, 2, 12, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 2304, 4).amax(2)
        pos = {int(v): k for k, v in enumerate(imgs.tolist())}
        for i, p in flips.tolist():
            top = win[pos[i], p].sort(descending=True).values
            assert (top[0] - top[1]).abs() <= 16 * EPS32 * wmag[pos[i], p], (i, p, top.tolist())
    if with_images:
        return flips.shape[0], flips[:, 0].unique()
    return flips.shape[0]


@pytest.mark.parametrize("post_processed", [False, True])
def test_sparse_front_matches_oracle_and_dense(post_processed):
    """forward of the conditioner under a deterministic gate: sparse crop path == CPU oracle on the explicit
    78 400-wide masked copies == the dense HIP kernels"""
    cond = _windowed_conditioner(3, post_processed)
    B = 3
    x = torch.rand(B, 784)
    with torch.no_grad():
        P = cond.deterministic_importance()
        assert cond._sparse_plan(cu(x), None, P) is not None
        h_sparse = cond(cu(x))
        cond.sparse_front = False
        h_dense = cond(cu(x))
        cond.sparse_front = True
        e = (x.unsqueeze(1) * P.cpu().unsqueeze(0)).reshape(B * 784, 784)
        ref = O.mnistcnn_forward(e, {k: v.detach().cpu() for k, v in cond.embedding_net.state_dict().items()})
    ref = ref.view(B, 784, 30)
    assert h_sparse.shape == (B, 784, 30)
    assert rel_err(h_sparse.cpu(), ref) < TOL, rel_err(h_sparse.cpu(), ref)
    assert_fwd(h_sparse, ref, what='h_sparse')
    assert rel_err(h_dense.cpu(), ref) < TOL
    assert_fwd(h_dense, ref, what='h_dense')
    # per-row check as well (a wrong row permutation of a few copies would hide in a global norm)
    err = (h_sparse.cpu() - ref).abs().amax(2) / ref.abs().amax(2).clamp_min(1e-6)
    assert err.max() < 1e-4, err.max()


def test_sparse_front_row_subsets_and_fallbacks():
    cond = _windowed_conditioner(5, True)
    B = 5
    x = cu(torch.rand(B, 784))
    rows = torch.tensor([783, 0, 27, 28, 400, 401, 13 * 28 + 13, 6 * 28 + 7, 21 * 28 + 20, 755], device=DEV)
    with torch.no_grad():
        P = cond.deterministic_importance()
        got = cond.forward_rows(x, rows, P)
        cond.sparse_front = False
        want = cond.forward_rows(x, rows, P)
        cond.sparse_front = True
        assert got.shape == want.shape == (B, rows.numel(), 30)
        assert rel_err(got.cpu(), want.cpu()) < TOL
        assert_fwd(got, want.cpu(), what='got')
        # an entry outside the 5x5 window: the sparse front must step aside (dense result unchanged)
        cond.A[0, 300] = 1.
        assert cond._sparse_plan(x, None, cond.deterministic_importance()) is None
        cond.A[0, 300] = 0.
        assert cond._sparse_plan(x, None, cond.deterministic_importance()) is not None
    # a gradient wanted for x (or for A) -> dense path
    assert cond._sparse_plan(x.clone().requires_grad_(True), None, cond.deterministic_importance()) is None
    cond.A.requires_grad = True
    assert cond._sparse_plan(x, None, cond.deterministic_importance()) is None
    cond.A.requires_grad = False
    # stochastic gate -> never sparse
    cond.stoch_gate, cond.s_thresh = True, True
    assert cond.deterministic_importance() is None


@pytest.mark.parametrize("B", [2, 7])
def test_sparse_front_parameter_gradients(B):
    """training with a frozen deterministic gate: parameter gradients of the sparse pair == CPU oracle autograd on the
    explicit masked copies == the dense HIP kernels"""
    cond = _windowed_conditioner(7 + B, True)
    net = cond.embedding_net
    x = torch.rand(B, 784)
    gh = torch.randn(B, 784, 30)
    # masked copies with a knife-edge pool window (fp64-verified near-ties, see _knife_edge_windows) get a ZERO cotangent:
    # what is left is compared at GTOL on every path (until round 4: 5e-3 on the conv gradients whenever one was counted)
    flips, knife = _knife_edge_windows(cond, x, with_images=True)
    assert flips <= 1 + B                              # a handful per million windows
    gh.view(B * 784, 30)[knife] = 0.
    assert cond._sparse_plan(cu(x), None, cond.deterministic_importance()) is not None
    h = cond(cu(x))
    assert h.requires_grad
    (h * cu(gh)).sum().backward()
    got = {k: p.grad.clone() for k, p in net.named_parameters()}
    for p in net.parameters():
        p.grad = None
    cond.sparse_front = False
    (cond(cu(x)) * cu(gh)).sum().backward()
    dense = {k: p.grad.clone() for k, p in net.named_parameters()}
    # CPU oracle
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in net.named_parameters()}
    e = (x.unsqueeze(1) * cond.A.detach().cpu().unsqueeze(0)).reshape(B * 784, 784)
    (O.mnistcnn_forward(e, params).view(B, 784, 30) * gh).sum().backward()
    for k in got:
        assert rel_err(got[k].cpu(), params[k].grad) < GTOL, (k, rel_err(got[k].cpu(), params[k].grad))
        # dense path under a deterministic gate = the tie-exact direct forward (DAGConditioner sets exact_pool_ties): the
        # exact max-pool ties of the constant background follow torch's first-maximum rule there too
        assert rel_err(dense[k].cpu(), params[k].grad) < GTOL, (k, flips, rel_err(dense[k].cpu(), params[k].grad))


@pytest.mark.parametrize("B,rows", [(1, [391]), (1, None), (33, [0, 783]), (130, [5, 6, 7, 300])])
def test_sparse_front_edge_sizes(B, rows):
    """single sample / single masked copy / batch sizes that are no multiple of anything"""
    cond = _windowed_conditioner(21, True)
    x = cu(torch.rand(B, 784))
    with torch.no_grad():
        P = cond.deterministic_importance()
        r = torch.arange(784, device=DEV) if rows is None else torch.tensor(rows, device=DEV)
        got = cond.forward_rows(x, r, P)
        cond.sparse_front = False
        want = cond.forward_rows(x, r, P)
    assert got.shape == want.shape == (B, r.numel(), 30)
    assert rel_err(got.cpu(), want.cpu()) < TOL
    assert_fwd(got, want.cpu(), what='got')
    # and the parameter gradients on the same subset (masked copies holding a knife-edge pool window: zero cotangent)
    cond.sparse_front = True
    gh = cu(torch.randn(B, r.numel(), 30))
    flips = 0
    if rows is None:                                   # counted on the full set of masked copies
        flips, knife = _knife_edge_windows(cond, x.cpu(), with_images=True)
        gh.view(B * 784, 30)[knife.to(DEV)] = 0.
    grads = []
    for sparse in (True, False):
        cond.sparse_front = sparse
        for p in cond.embedding_net.parameters():
            p.grad = None
        (cond.forward_rows(x, r, P) * gh).sum().backward()
        grads.append([p.grad.clone() for p in cond.embedding_net.parameters()])
    for a, b, (k, _) in zip(grads[0], grads[1], cond.embedding_net.named_parameters()):
        assert rel_err(a.cpu(), b.cpu()) < GTOL, (k, flips, rel_err(a.cpu(), b.cpu()))


def test_sparse_front_reference_golden():
    """MNIST DAG flow after the DAG phase against the REFERENCE's own numbers (tests/golden/make_golden_frozen.py):
    z, log-det, loss (sparse forward) and the embedding-net gradients (sparse backward)"""
    from models import AffineNormalizer
    from models.NormalizingFlowFactories import buildMNISTNormalizingFlow
    g0, g = load_golden("flow_mnist_affine_dag"), load_golden("flow_mnist_affine_dag_frozen")
    flow = buildMNISTNormalizingFlow([1], AffineNormalizer, {}, l1=0., nb_epoch_update=10, hot_encoding=False,
                                     prior_kernel=2)
    sd = {k[2:]: v for k, v in g0.items() if k.startswith("p.")}
    sd["steps.0.conditioner.A"] = flow.steps[0].conditioner.A.detach().clone()
    flow.load_state_dict(sd)
    flow = flow.to(DEV)
    cond = flow.steps[0].conditioner
    with torch.no_grad():
        cond.post_process(zero_threshold=.1)
    x = cu(g0["x"])
    assert cond._sparse_plan(x, None, cond.deterministic_importance()) is not None
    z, ld = flow(x)
    assert rel_err(z.cpu(), g["z"]) < TOL and rel_err(ld.cpu(), g["logdet"]) < TOL
    assert_fwd(z, g["z"], what='z')
    assert_fwd(ld, g["logdet"], what='ld')
    loss = flow.loss(z, ld)
    assert rel_err(loss.detach().cpu(), g["loss"]) < TOL
    assert_fwd(loss, g["loss"], what='loss')
    loss.backward()
    named = dict(flow.named_parameters())
    n = 0
    for k, v in g.items():
        if k.startswith("g.") or k.startswith("g8."):
            got = named[k.split(".", 1)[1]].grad.cpu()
            assert rel_err(got[:8] if k.startswith("g8.") else got, v) < GTOL, (k, rel_err(got[:8] if k.startswith("g8.") else got, v))
            n += 1
    assert n == 8
    with torch.no_grad():                              # evaluation path (no saved tensors)
        z2, ld2 = flow(x)
    assert rel_err(z2.cpu(), g["z"]) < TOL and rel_err(ld2.cpu(), g["logdet"]) < TOL
    assert_fwd(z2, g["z"], what='z2')
    assert_fwd(ld2, g["logdet"], what='ld2')


def test_sparse_front_prepared_tables_give_the_same_bits(monkeypatch):
    """gnf_mnistcnn_sparse_prepare + _fwd_prepared (the parameter-only tables built once for the 109 levels of a sampling
    pass) == gnf_mnistcnn_sparse_fwd, bit for bit; the holder is only consulted without autograd.  (GNF_SPARSE_FC12=0: the
    one-launch fc1 + fc2 kernel of the held-table path sums in another order, test_sparse_front_fc12_* compares that one.)"""
    monkeypatch.setenv("GNF_SPARSE_FC12", "0")
    from models import DAGConditioner
    from models.MLP import MNISTCNN
    from gnf_hip import ops
    torch.manual_seed(21)
    net = MNISTCNN(out_d=30).to(DEV)
    A = torch.zeros(784, 784)
    for i in range(784):
        for dr in (-2, -1, 0, 1, 2):
            for dc in (-2, -1, 0, 1, 2):
                r, c = i // 28 + dr, i % 28 + dc
                if (dr or dc) and 0 <= r < 28 and 0 <= c < 28:
                    A[i, r * 28 + c] = float(torch.rand(()) < .5)
    P = cu(A)
    x = cu(torch.randn(5, 784))
    rows = [0, 27, 300, 391, 392, 783, 29]
    sr = ops.SparseRows(rows, 5, torch.device(DEV))
    with torch.no_grad():
        ref = net.sparse_rows(x, P, sr)
        assert net._held_prep is None
        with net.hold_prepared():
            assert net._held_prep is not None
            got = net.sparse_rows(x, P, sr)
            got2 = net.sparse_rows(x * 2., P, sr)           # the tables do not depend on the inputs
        assert net._held_prep is None
        ref2 = net.sparse_rows(x * 2., P, sr)
    assert torch.equal(got, ref) and torch.equal(got2, ref2)
    with net.hold_prepared():                               # with autograd on, the holder is ignored (the backward needs pd / argmax)
        out = net.sparse_rows(x, P, sr)
        out.sum().backward()
    assert net.fc1.weight.grad is not None and torch.equal(out.detach(), ref)
    # ABI validation of the new entry points
    from gnf_hip import abi
    lib = abi.load()
    F = 128
    nb = lib.gnf_mnistcnn_sparse_prep_bytes(F)
    assert nb == (64 * 400 * F + 16 + F + 64) * 4
    prep = torch.empty(nb // 4, device=DEV)
    ps = [net.conv1.bias, net.conv2.weight, net.conv2.bias, net.fc1.weight, net.fc1.bias]
    st = abi.stream()
    assert lib.gnf_mnistcnn_sparse_prepare(*[abi.ptr(t) for t in ps], F, abi.rawptr(prep), nb - 4, st) == -3
    assert lib.gnf_mnistcnn_sparse_prepare(*[abi.ptr(t) for t in ps], 130, abi.rawptr(prep), nb, st) == -2
    assert lib.gnf_mnistcnn_sparse_prepare(*[abi.ptr(t) for t in ps], F, None, nb, st) == -1


def _random_window_gate(seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.zeros(784, 784)
    for i in range(784):
        for dr in (-2, -1, 0, 1, 2):
            for dc in (-2, -1, 0, 1, 2):
                r, c = i // 28 + dr, i % 28 + dc
                if (dr or dc) and 0 <= r < 28 and 0 <= c < 28:
                    A[i, r * 28 + c] = float(torch.rand((), generator=g) < .5) * float(torch.rand((), generator=g) + .2)
    return A


@pytest.mark.parametrize("B,rows,out_d", [(5, [0, 27, 300, 391, 392, 783, 29], 30), (1, [391], 30), (100, [3, 59, 115, 171], 30),
                                          (37, list(range(0, 784, 5)), 30), (16, [400, 401], 1), (17, [10, 700], 32)])
def test_sparse_front_fc12_one_launch_vs_oracle(B, rows, out_d, monkeypatch):
    """gnf_mnistcnn_sparse_fwd_prepared_fc2 (crop kernel + ONE launch for fc1 + ReLU + fc2, MLP.py:43-47): element-wise
    against the oracle's dense MNISTCNN on the masked copies, and against the grouped-GEMM + tall-layer pair it replaces.
    Row counts per crop origin that are no multiple of the kernel's 16-row tiles, one masked copy, 157 of them, out_d = 1
    and the widest fc2 the kernel takes."""
    from models.MLP import MNISTCNN
    from gnf_hip import ops
    from conftest import assert_close
    torch.manual_seed(5)
    net = MNISTCNN(out_d=out_d).to(DEV)
    P = cu(_random_window_gate(3))
    x = cu(torch.randn(B, 784))
    sr = ops.SparseRows(rows, B, torch.device(DEV))
    with torch.no_grad(), net.hold_prepared():
        got = net.sparse_rows(x, P, sr)                      # [B, R, out_d] through the one-launch kernel
        monkeypatch.setenv("GNF_SPARSE_FC12", "0")
        pair = net.sparse_rows(x, P, sr)
        monkeypatch.delenv("GNF_SPARSE_FC12")
        got_vm = net.sparse_rows(x, P, sr, variable_major=True)
    assert got.shape == pair.shape == (B, len(rows), out_d) and torch.equal(got_vm.permute(1, 0, 2), got)
    assert_close(got, pair, what="one launch vs GEMM pair")
    ps = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    e = (x.cpu().unsqueeze(1) * P.cpu()[rows].unsqueeze(0)).reshape(B * len(rows), 784)
    want = O.mnistcnn_forward(e, ps).view(B, len(rows), out_d)
    assert_close(got, want, what="one launch vs oracle")


def test_sparse_front_fc12_abi_validation():
    import ctypes
    from gnf_hip import abi
    lib = abi.load()
    N = None
    t = torch.zeros(64 * 400 * 128 + 4096, device=DEV)
    i32 = torch.zeros(128, dtype=torch.int32, device=DEV)
    p, ip = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(i32.data_ptr())
    nb = 400 * 4
    f = lib.gnf_mnistcnn_sparse_fwd_prepared_fc2
    assert f(p, 1, p, ip, 1, ip, 1, p, p, p, p, 128, p, p, p, 30, p, p, nb, N) == 0          # (one masked copy, zero tables)
    assert f(p, 1, p, ip, 1, ip, 1, p, p, p, p, 64, p, p, p, 30, p, p, nb, N) == -2           # fc1 width it is not built for
    assert f(p, 1, p, ip, 1, ip, 1, p, p, p, p, 128, p, p, p, 33, p, p, nb, N) == -2          # fc2 wider than two MFMA tiles
    assert f(p, 1, p, ip, 1, ip, 1, p, p, p, p, 128, p, p, p, 0, p, p, nb, N) == -1
    assert f(p, 1, p, ip, 1, ip, 1, p, p, p, p, 128, p, N, p, 30, p, p, nb, N) == -1          # no fc2 weight
    assert f(p, 1, p, ip, 1, ip, 1, p, p, p, p, 128, p, p, p, 30, p, p, nb - 4, N) == -1      # workspace short
    assert f(p, 1, p, ip, 1, ip, 2, p, p, p, p, 128, p, p, p, 30, p, p, nb, N) == -1          # group larger than the call
    assert f(p, 0, p, ip, 1, ip, 1, p, p, p, p, 128, p, p, p, 30, N, N, 0, N) == 0            # empty batch: nothing to do
    torch.cuda.synchronize()


@pytest.mark.parametrize("hidden,R,B", [([50, 50, 50], 7, 100), ([50, 50, 50], 1, 3), ([20, 20], 5, 33), ([100, 100, 100], 4, 40),
                                        ([150, 150, 150], 3, 20)])
def test_monotonic_inverse_scattered_result(hidden, R, B):
    """gnf_monotonic_inv_scatter == gnf_monotonic_inv followed by x[:, rows] = result.t(), bit for bit, for the level kernels
    (two steps per round and one), the register-chained and the wide nets; columns outside `rows` are not touched."""
    from models import MonotonicNormalizer
    torch.manual_seed(4)
    nrm = MonotonicNormalizer(hidden, 30, nb_steps=20).to(DEV)
    z = cu(torch.randn(R, B))
    h = cu(torch.randn(R, B, 30))
    rows = torch.randperm(784)[:R].to(torch.int32).to(DEV)
    with torch.no_grad():
        want = torch.full((B, 784), 7.5, device=DEV)
        want[:, rows.long()] = nrm.inverse_transform(z, h).t()
        got = torch.full((B, 784), 7.5, device=DEV)
        assert nrm.inverse_transform_into(z, h, got, rows)
    assert torch.equal(got, want)


def test_sparse_front_backward_reuses_the_forwards_tables():
    """gnf_mnistcnn_sparse_bwd_tables against the tables the forward built == gnf_mnistcnn_sparse_bwd building them again,
    bit for bit (same parameters, same kernels: only two launches fewer)"""
    from gnf_hip import ops
    cond = _windowed_conditioner(5, True)
    x = cu(torch.rand(3, 784))
    gh = cu(torch.randn(3, 784, 30))
    out = []
    for reuse in (True, False):
        ops.SPARSE_REUSE_TABLES = reuse
        try:
            for p in cond.embedding_net.parameters():
                p.grad = None
            (cond(x) * gh).sum().backward()
        finally:
            ops.SPARSE_REUSE_TABLES = True
        out.append([p.grad.clone() for p in cond.embedding_net.parameters()])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_sparse_front_abi_validation():
    import ctypes
    from gnf_hip import abi
    lib = abi.load()
    assert lib.gnf_mnistcnn_sparse_ws_bytes(10, 128) == (10 * 400 + 64 * 400 * 128 + 16 + 128 + 64) * 4
    assert lib.gnf_mnistcnn_sparse_bwd_ws_bytes(10, 128, 3) > lib.gnf_mnistcnn_sparse_ws_bytes(10, 128)
    N = None
    assert lib.gnf_mnistcnn_sparse_fwd(N, 1, N, N, 1, N, 1, N, N, N, N, N, N, 128, N, N, N, N, 0, N) == -1
    t = torch.zeros(64 * 400 * 8 * 2 + (1 << 22), device=DEV)
    i32 = torch.zeros(128, dtype=torch.int32, device=DEV)
    p, ip = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(i32.data_ptr())
    nb = t.numel() * 4
    # F not a multiple of 4 -> shape error; zero rows -> no-op success
    assert lib.gnf_mnistcnn_sparse_fwd(p, 1, p, ip, 1, ip, 1, p, p, p, p, p, p, 6, p, N, N, p, nb, N) == -2
    assert lib.gnf_mnistcnn_sparse_fwd(p, 0, p, ip, 1, ip, 1, p, p, p, p, p, p, 8, p, N, N, p, 0, N) == 0
    # workspace too small; pd_save without argmax_save
    assert lib.gnf_mnistcnn_sparse_fwd(p, 1, p, ip, 1, ip, 1, p, p, p, p, p, p, 8, p, N, N, p, 16, N) == -1
    assert lib.gnf_mnistcnn_sparse_fwd(p, 1, p, ip, 1, ip, 1, p, p, p, p, p, p, 8, p, p, N, p, nb, N) == -1
    # backward: null gradient output, bad F, zero rows (gradients zeroed)
    assert lib.gnf_mnistcnn_sparse_bwd(p, 1, p, ip, 1, ip, 1, ip, 1, ip, p, p, p, p, p, 8, p, p, p, N, p, p, p, p, p, p, nb, N) == -1
    assert lib.gnf_mnistcnn_sparse_bwd(p, 1, p, ip, 1, ip, 1, ip, 1, ip, p, p, p, p, p, 6, p, p, p, p, p, p, p, p, p, p, nb, N) == -2
    g = torch.ones(8 * 2304, device=DEV)
    gp = ctypes.c_void_p(g.data_ptr())
    assert lib.gnf_mnistcnn_sparse_bwd(p, 0, p, ip, 1, ip, 1, ip, 1, ip, p, p, p, p, p, 8, p, p, p, p, p, p, p, gp, p, p, nb, N) == 0
    torch.cuda.synchronize()
    assert float(g.abs().sum()) == 0.


def test_mnist_level_inversion_uses_sparse_front():
    """DAG 'pixel above and left-above': level-scheduled inversion with the sparse front == with the dense kernels"""
    from models import DAGConditioner, AffineNormalizer
    from models.NormalizingFlow import NormalizingFlowStep
    from models.MLP import MNISTCNN
    torch.manual_seed(11)
    A = torch.zeros(784, 784)
    for i in range(28, 784):
        A[i, i - 28] = 1.
        if i % 28:
            A[i, i - 29] = 1.
    cond = DAGConditioner(784, MNISTCNN(out_d=2), 2, A_prior=A).to(DEV)
    cond.stoch_gate, cond.s_thresh, cond.h_thresh = False, False, 0.
    cond.A.requires_grad = False
    step = NormalizingFlowStep(cond, AffineNormalizer()).to(DEV)
    z = cu(torch.randn(4, 784) * .5)
    x_sparse = step.invert(z)
    assert len(cond._sparse_plans) >= 28
    cond.sparse_front = False
    x_dense = step.invert(z)
    assert rel_err(x_sparse.cpu(), x_dense.cpu()) < 1e-4
    with torch.no_grad():
        z_back, _ = step(x_sparse)
    assert rel_err(z_back.cpu(), z.cpu()) < 1e-4


@pytest.mark.parametrize("normalizer", ["affine", "monotonic"])
def test_level_inversion_replayed_as_a_graph(normalizer):
    """sampling with a frozen gate (reference ImageExperiments.py:341-350 samples after post_process()): the first pass of a
    shape runs eagerly, the second is captured into a hipGraph, later ones replay it.  All three give the SAME bits as the
    eager pass; a replay reads the CURRENT parameters (the normalizer's weight image is packed inside the graph) and a
    changed gate drops the graphs."""
    from models import DAGConditioner, AffineNormalizer, MonotonicNormalizer
    from models.NormalizingFlow import NormalizingFlowStep, _INV_GRAPHS
    from models.MLP import MNISTCNN
    torch.manual_seed(13)
    A = torch.zeros(784, 784)
    for i in range(28, 784):
        A[i, i - 28] = 1.
        if i % 28:
            A[i, i - 29] = 1.
    mono = normalizer == "monotonic"
    cond = DAGConditioner(784, MNISTCNN(out_d=30 if mono else 2), 30 if mono else 2, A_prior=A).to(DEV)
    cond.stoch_gate, cond.s_thresh, cond.h_thresh = False, False, 0.
    cond.A.requires_grad = False
    norm = MonotonicNormalizer([50, 50, 50], 30, nb_steps=20, solver="CC") if mono else AffineNormalizer()
    step = NormalizingFlowStep(cond, norm).to(DEV)
    z = cu(torch.randn(3, 784) * .5)
    step.graph_invert = False
    x_eager = step.invert(z)
    step.graph_invert = True
    x1 = step.invert(z)                       # eager, marks the shape
    x2 = step.invert(z)                       # captured + replayed
    x3 = step.invert(z)                       # replayed
    graphs = _INV_GRAPHS[step]
    assert len(graphs) == 1 and isinstance(next(iter(graphs.values())), tuple)
    for x in (x1, x2, x3):
        assert torch.equal(x, x_eager)
    z2 = cu(torch.randn(3, 784) * .5)         # other inputs through the same graph
    step.graph_invert = False
    ref2 = step.invert(z2)
    step.graph_invert = True
    assert torch.equal(step.invert(z2), ref2)
    with torch.no_grad():                     # parameters move (a training step between two sampling passes)
        for p in step.parameters():
            if p.requires_grad:
                p.mul_(1.01)
    step.graph_invert = False
    ref3 = step.invert(z)
    step.graph_invert = True
    got3 = step.invert(z)
    assert torch.equal(got3, ref3) and not torch.equal(ref3, x_eager)
    with torch.no_grad():                     # another gate: new schedule, the graphs are dropped
        cond.A[100, 72] = 0.
    x4 = step.invert(z)
    assert step not in _INV_GRAPHS or all(v == "warm" for v in _INV_GRAPHS[step].values())
    with torch.no_grad():
        zb, _ = step(x4)
    assert rel_err(zb.cpu(), z.cpu()) < 1e-4
    assert not any("graph" in k.lower() and k != "graph_invert" for k in step.__dict__)    # graphs live outside the module


@pytest.mark.parametrize("d,l1", [(84, .3), (6, 0.), (50, .5), (784, .1)])
def test_dag_loss_fused_vs_reference_expression(d, l1):
    """DAGConditioner.loss() through the fused kernels == the reference's expression (:176-194, :268-271) evaluated with
    plain torch ops, value and gradient; d = 50 -> exponent 0 (the trace term is identically 0, Appendix B)"""
    from models import DAGConditioner
    torch.manual_seed(d)
    cond = DAGConditioner(d, [8], 2, l1=l1).to(DEV)
    with torch.no_grad():
        cond.A.mul_(.2)
        cond.lambd.fill_(.7)
        cond.c.fill_(.05)
    assert cond.exponent == d % 50
    loss = cond.loss()
    loss.backward()
    got_g = cond.A.grad.clone()
    cond.A.grad = None
    lag = cond.get_power_trace()
    ref = cond.dag_const * (cond.lambd * lag + cond.c / 2 * lag ** 2) + cond.l1_weight * cond.A.abs().mean()
    ref.backward()
    assert rel_err(loss.detach().cpu(), ref.detach().cpu()) < TOL, (loss.item(), ref.item())
    assert_fwd(loss, ref.detach().cpu(), what='loss')
    assert rel_err(got_g.cpu(), cond.A.grad.cpu()) < GTOL


def test_dag_loss_of_a_frozen_gate_is_evaluated_once_per_state():
    """post_process() froze A but the constraint is still on: the term has no gradient left, so loss() evaluates its matrix
    power once per state of (A, dual buffers, exponent) and returns the same value until one of them changes"""
    from gnf_hip import ops
    from models import DAGConditioner
    torch.manual_seed(2)
    cond = DAGConditioner(56, [8], 2, l1=.2).to(DEV)
    with torch.no_grad():
        cond.A.mul_(.4)
        cond.post_process(zero_threshold=.1)
        cond.lambd.fill_(.3)
    calls = []
    real = ops.DagLossFn.apply
    try:
        ops.DagLossFn.apply = lambda *a: (calls.append(1), real(*a))[1]
        v1 = cond.loss()
        v2 = cond.loss()
        assert len(calls) == 1 and v1 is v2 and not v1.requires_grad
        lag = cond.get_power_trace()
        ref = cond.dag_const * (cond.lambd * lag + cond.c / 2 * lag ** 2) + cond.l1_weight * cond.A.abs().mean()
        assert rel_err(v1.cpu(), ref.cpu()) < TOL
        assert_fwd(v1, ref.cpu(), what='v1')
        with torch.no_grad():
            cond.lambd.add_(1.)                    # in-place change of a dual buffer: new state
        v3 = cond.loss()
        assert len(calls) == 2
        ref3 = cond.dag_const * (cond.lambd * lag + cond.c / 2 * lag ** 2) + cond.l1_weight * cond.A.abs().mean()
        assert rel_err(v3.cpu(), ref3.cpu()) < TOL
        assert_fwd(v3, ref3.cpu(), what='v3')
        cond.exponent += 50                        # what update_dual_param() does when the trace vanishes
        cond.loss()
        assert len(calls) == 3
        cond.A.requires_grad = True                # re-opened: the term has a gradient again, nothing is cached
        cond.loss(); cond.loss()
        assert len(calls) == 5
    finally:
        ops.DagLossFn.apply = real


def test_dag_loss_switched_off_after_dag_phase():
    """dag_const = l1_weight = 0 with a frozen A (what update_dual_param() leaves): loss() is exactly 0 without touching
    the matrix power, and comes back when the buffers change"""
    from models import DAGConditioner
    cond = DAGConditioner(12, [8], 2, l1=.2).to(DEV)
    with torch.no_grad():
        cond.post_process(zero_threshold=.1)
    assert cond.loss().item() != 0.
    cond.dag_const = torch.tensor(0., device=DEV)
    cond.l1_weight = torch.tensor(0., device=DEV)
    assert cond._constraints_off() and cond.loss().item() == 0.
    cond.l1_weight = torch.tensor(.5, device=DEV)
    assert not cond._constraints_off() and cond.loss().item() > 0.
    with torch.no_grad():
        cond.l1_weight.zero_()                       # in-place change is seen too (version counter)
    assert cond._constraints_off()


@pytest.mark.parametrize("size_img,fc_in", [([1, 14, 14], 400), ([1, 7, 7], 16), ([1, 9, 12], 16 * 2 * 4), ([2, 10, 10], 144)])
def test_mnistcnn_other_geometries(size_img, fc_in):
    """single-channel images up to 28x28 run zero-embedded on the fused 28x28 kernels, anything else on the batched
    im2col + MFMA GEMM: both against the oracle's torch-CPU convolution, forward and gradients"""
    from models.MLP import MNISTCNN
    torch.manual_seed(sum(size_img))
    net = MNISTCNN(out_d=5, fc_l=[fc_in, 12], size_img=size_img).to(DEV)
    n, d = 37, size_img[0] * size_img[1] * size_img[2]
    e = torch.randn(n, d)
    gout = torch.randn(n, 5)
    eg = req(e)
    out = net(eg)
    (out * cu(gout)).sum().backward()
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in net.named_parameters()}
    ec = e.clone().requires_grad_(True)
    ref = O.mnistcnn_forward(ec, params, tuple(size_img))
    (ref * gout).sum().backward()
    assert rel_err(out.detach().cpu(), ref.detach()) < TOL
    assert_fwd(out, ref.detach(), what='out')
    assert rel_err(eg.grad.cpu(), ec.grad) < GTOL
    for k, p in net.named_parameters():
        assert rel_err(p.grad.cpu(), params[k].grad) < GTOL, k


@pytest.mark.parametrize("variant", ["0", "1"])
def test_monotonic_backward_ab_variants(variant):
    """the A/B switch of the narrow-net backward (GNF_MONO_INDW=0: HBM-staged weight gradients, =1: in-kernel, one node per
    pass; default: two nodes per pass) is read once per process: run the gradient parity tests in a child process"""
    import os
    import subprocess
    import sys
    env = dict(os.environ, GNF_MONO_INDW=variant)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), "-q", "-m", "gpu",
                        "-k", "test_monotonic_forward_backward_vs_oracle or test_monotonic_golden_integrand_grads or test_monotonic_ragged_sizes", "-x"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
