"""GPU: every uninitialised buffer poisoned; the results must not change.

The library allocates nothing itself: every output, saved activation and workspace of a kernel is a `torch.empty` made in
gnf_hip/ops.py, models/ or gnf_hip/dp.py, and whether every word a kernel reads was written first is decided case by case in
csrc/.  tests/poison.py fills those allocations with a chosen bit pattern; each case below runs one path through the public
route (the ops.* autograd Functions and helpers, the flow objects; the C ABI only where ops.py has no route: the fp32-only and
the split-bf16 GEMM workspaces, the Monotonic backward's GNF_TRUE_F32 twin and its bounded workspace, the prefix kernel's read
set) under three patterns -- zeros, NaN, 3.4e38 -- and demands the same bits of every returned tensor and every gradient
(poison.three_arms).  No tolerance appears: correctness against fp64 stays with the tests of each op; a few cheap fp64 judges
run on the ZERO arm so that a case cannot pass by being consistently wrong.  Where the dispatcher exposes its choice, the
kernel's name is one of the compared results AND asserted: a case that falls onto another family proves nothing.

Integer, bool and uint8 buffers (pool decisions, plans, keys) are zero in every arm: out of scope (tests/poison.py).  The
words a kernel reads from a float workspace AS INTEGERS were checked in the code instead: the only such workspace is
gnf_dag_levels' (64-bit edge masks; dag_pack_k stores every word and every nonzero-word mask of every row before dag_peel_k
reads them, padding bits zero); every counter or flag a kernel waits on lives in LDS and is zeroed by that kernel, and Adam's
ticket lives in a torch.zeros buffer.

Exclusions from the bit comparison (a region of a returned tensor the header or ops.py documents as undefined): none.  The
tensors image_prep, toy_sample and tab_batch return with out=None are contiguous -- no row pitch, no padding -- and are
compared whole.  The GNF_GEMM_ACCUM path (partials added from the second chunk on) is an internal flag of the Monotonic
backward's staged weight gradients: the chunked cases reach it."""
import ctypes

import pytest
import torch

import poison
from poison import three_arms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the coverage pin (tests/test_poison_helper.py): every gnf_*_ws_bytes of include/gnf_hip.h -> the cases that reach it
WORKSPACES = {
    "gnf_colsum_ws_bytes": ["test_colsum"],
    "gnf_linear_ws_bytes": ["test_mlp_chains"],
    "gnf_gemm_ws_bytes": ["test_gemm_through_ops"],
    "gnf_gemm_f32_ws_bytes": ["test_gemm_fp32_split_k_partials"],
    "gnf_gemm_split_ws_bytes": ["test_gemm_split_bf16_families"],
    "gnf_dag_gate_fwd_ws_bytes": ["test_dag_gate", "test_dag_mlp_front_and_rows", "test_lenet_gated_front"],
    "gnf_dag_gate_bwd_ws_bytes": ["test_dag_gate"],
    "gnf_dag_gate_bwd_cols_ws_bytes": ["test_dag_conv_front_on_its_plan"],
    "gnf_monotonic_bwd_ws_bytes": ["test_monotonic_through_ops", "test_monotonic_backward_in_chunks",
                                   "test_monotonic_narrow_backward_true_f32"],
    # (ops.py asks gnf_made_prefix_ctx_ws_bytes with cond_in = 0, which this one forwards to: the same workspace)
    "gnf_made_prefix_ws_bytes": ["test_made_inversion", "test_made_whole_inversion_in_the_workspace_form",
                                 "test_made_prefix_reads_only_lower_degrees", "test_made_monotonic_step_inverts_by_columns"],
    "gnf_made_prefix_ctx_ws_bytes": ["test_made_inversion"],
    "gnf_made_adjoint_ws_bytes": ["test_made_adjoint_both_forms", "test_rsample_backward"],
    "gnf_mnistcnn_conv_bwd_ws_bytes": ["test_mnist_conv", "test_dag_conv_front_on_its_plan"],
    "gnf_lenet_conv_bwd_ws_bytes": ["test_lenet_front"],
    "gnf_lenet_gated_bwd_ws_bytes": ["test_lenet_gated_front"],
    "gnf_lenet_rows_bwd_ws_bytes": ["test_lenet_rows_front"],
    "gnf_dagmlp_gated_bwd_ws_bytes": ["test_dag_mlp_front_and_rows", "test_shared_gradient_slot_of_A"],
    "gnf_mnistcnn_sparse_ws_bytes": ["test_sparse_front_inference"],
    "gnf_mnistcnn_sparse_bwd_ws_bytes": ["test_sparse_front_backward"],
    "gnf_dag_levels_ws_bytes": ["test_dag_levels"],
}


def cu(t):
    return None if t is None else t.to(DEV)


def req(t):
    return t.to(DEV).requires_grad_(True)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def lib():
    from gnf_hip import abi
    return abi.load()


def gemm_kernel():
    return lib().gnf_gemm_last_kernel().decode()


def grads_of(out, leaves, cot, names):
    """{g<name>: gradient} of (out * cot).sum() for the named leaves"""
    gs = torch.autograd.grad(out, leaves, grad_outputs=cot, allow_unused=True)
    return {"g" + n: g for n, g in zip(names, gs) if g is not None}


def near(a, ref, tol, what):
    err = float((a.double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)
    assert err < tol, (what, err)


# ================================================================================================== GEMM
def _dev_randn(seed, *shape):
    torch.manual_seed(seed)
    return torch.randn(*shape, device=DEV)


def _gemm_operands(M, N, K, la, lb):
    """A [M, K] row-major ('r': strides (K, 1)) or k-major ('c': (1, M)); B [K, N] row-major ('r': (N, 1)) or the Linear
    layout ('c': (1, K)); values from a fixed seed"""
    sc = K ** -.25
    A = _dev_randn(M + 3 * N + 7 * K, *((M, K) if la == "r" else (K, M))) * sc
    B = _dev_randn(M + 3 * N + 7 * K + 1, *((K, N) if lb == "r" else (N, K))) * sc
    return A, ((K, 1) if la == "r" else (1, M)), B, ((N, 1) if lb == "r" else (1, K))


def _gemm_ref(A, sa, B, sb, M, N, K, rows):
    A2 = A if sa[1] == 1 else A.t()
    B2 = B if sb[1] == 1 else B.t()
    return A2[rows].double() @ B2.double()


# split-K with a ragged last K-range (k-major, M <= 128, N >= 512, K >= 16384, K % 64 != 0); the persistent tall kernel with a
# ragged last block and N < 128 (K % 128 != 0 keeps it on the fp32 kernel also with the workspace)
OPS_GEMM = [("kmajor_ragged_K", 28, 516, 16400, "c", "r", "gemm_kmajor_k", "gemm_kmajor_k"),
            ("kmajor_existing", 64, 516, 40001, "c", "r", "gemm_kmajor_k", "gemm_kmajor_k"),
            ("split_kmajor", 64, 512, 20001, "c", "r", "gemm_split_kmajor_k", "gemm_kmajor_k"),
            ("tall_ragged_block", 48500, 127, 320, "r", "c", "gemm_tall_k", "gemm_tall_k")]


@pytest.mark.parametrize("name,M,N,K,la,lb,k_split,k_f32", OPS_GEMM, ids=[c[0] for c in OPS_GEMM])
def test_gemm_through_ops(name, M, N, K, la, lb, k_split, k_f32):
    """ops.gemm: the workspace of gnf_gemm_ws_bytes (fp32 split-K partials, or the split-bf16 kernels' operand planes and
    partials) and C itself are poisoned"""
    from gnf_hip import ops
    want = k_split if lib().gnf_gemm_split_enabled() else k_f32
    rows = torch.arange(0, M, max(M // 64, 1), device=DEV)

    def fn():
        A, sa, B, sb = _gemm_operands(M, N, K, la, lb)
        C = torch.empty(M, N, device=DEV)
        ops.gemm(A, sa, B, sb, C, (N, 1), M, N, K)
        return {"C": C, "kernel": gemm_kernel()}

    def judge(r):
        assert r["kernel"] == want, r["kernel"]
        A, sa, B, sb = _gemm_operands(M, N, K, la, lb)
        near(r["C"][rows], _gemm_ref(A, sa, B, sb, M, N, K, rows), 1e-5, name)
    three_arms(fn, judge)


@pytest.mark.parametrize("M,N,K", [(28, 516, 16400), (60, 70, 2052)], ids=["kmajor", "vec_split_k"])
def test_gemm_fp32_split_k_partials(M, N, K):
    """gnf_gemm with a workspace of exactly gnf_gemm_f32_ws_bytes (what GNF_TRUE_F32=1 runs): the fp32-MFMA kernels' split-K
    partials (k_per_split, c_split_stride) with a short last K-range, and the reduction that sums them"""
    from gnf_hip.abi import call, ptr, stream
    la = "c" if M == 28 else "r"

    def fn():
        A, sa, B, sb = _gemm_operands(M, N, K, la, "r")
        bias = _dev_randn(5, N)
        C = torch.empty(M, N, device=DEV)
        nws = int(lib().gnf_gemm_f32_ws_bytes(M, N, K))
        assert nws > 0
        w = torch.empty(nws // 4, device=DEV)
        call("gnf_gemm", ptr(A), sa[0], sa[1], ptr(B), None, sb[0], sb[1], ptr(C), N, 1, ptr(bias), None, 0, 0, None, 0, 0, 1,
             M, N, K, ptr(w), nws, stream())
        return {"C": C, "kernel": gemm_kernel()}

    def judge(r):
        assert r["kernel"] == ("gemm_kmajor_k" if M == 28 else "gemm_vec_k<64,64>"), r["kernel"]
        A, sa, B, sb = _gemm_operands(M, N, K, la, "r")
        rows = torch.arange(M, device=DEV)
        near(r["C"], torch.relu(_gemm_ref(A, sa, B, sb, M, N, K, rows) + _dev_randn(5, N).double()), 1e-5, "C")
    three_arms(fn, judge)


# the smallest shapes of tests/test_gpu_split.py with a ragged edge: last block short and N < 128 (zero-padded planes); last
# block short; M < 128 and K neither a multiple of 64 nor of the ranges
SPLIT_BF16 = [("tall", 10301, 100, 1024, "r", "c", "gemm_split_tall_k"), ("wide", 10333, 1280, 128, "r", "r", "gemm_split_wide_k"),
              ("kmajor", 64, 512, 20001, "c", "r", "gemm_split_kmajor_k"), ("general", 70, 65, 100, "r", "c", "gemm_split_k")]


@pytest.mark.parametrize("name,M,N,K,la,lb,expect", SPLIT_BF16, ids=[c[0] for c in SPLIT_BF16])
def test_gemm_split_bf16_families(name, M, N, K, la, lb, expect):
    """gnf_gemm_split_bf16 with gnf_gemm_split_ws_bytes: pre-split fragment-major operand planes and split-K partials"""
    from gnf_hip import abi
    from gnf_hip.abi import call, ptr, stream
    rows = torch.cat([torch.arange(0, M, max(M // 64, 1)), torch.arange(max(M - 40, 0), M)]).to(DEV)

    def fn():
        A, sa, B, sb = _gemm_operands(M, N, K, la, lb)
        C = torch.empty(M, N, device=DEV)
        nws = int(lib().gnf_gemm_split_ws_bytes(M, N, K))
        w = torch.empty(max(nws // 4, 4), device=DEV)
        call("gnf_gemm_split_bf16", ptr(A), sa[0], sa[1], ptr(B), sb[0], sb[1], ptr(C), N, 1, None, 0, M, N, K, 0, 1, 0,
             abi.rawptr(w), nws, stream())
        return {"C": C, "kernel": lib().gnf_gemm_split_last_kernel().decode()}

    def judge(r):
        assert r["kernel"] == expect, r["kernel"]
        A, sa, B, sb = _gemm_operands(M, N, K, la, lb)
        near(r["C"][rows], _gemm_ref(A, sa, B, sb, M, N, K, rows), 1e-5, name)
    three_arms(fn, judge)


def test_colsum():
    from gnf_hip import ops
    three_arms(lambda: {"out": ops.colsum(cu(torch.randn(513, 7, generator=gen(1))))},
               lambda r: near(r["out"], cu(torch.randn(513, 7, generator=gen(1))).double().sum(0), 1e-5, "colsum"))


# (M, widths): (300, .., 40 <- 24) and (4099, .., 30 <- 128): gnf_linear_bwd with the column sums of its data gradient (fused
# into the launch on the tall path, a column-sum pass behind the small-batch one); (2500, 64, 17): the tall-narrow layers of
# test_linear_tall_narrow_layers; (100, ..): the weight-streaming small-batch kernels
MLP_CHAINS = [(300, [16, 24, 40]), (4099, [24, 128, 30]), (2500, [24, 64, 17]), (100, [20, 33, 30])]


@pytest.mark.parametrize("M,dims", MLP_CHAINS, ids=["M%d" % c[0] for c in MLP_CHAINS])
def test_mlp_chains(M, dims):
    from gnf_hip import ops
    # the last layer's launch hands the bias gradient of the layer below out of the same launch exactly on the tall path
    # (M >= 2048, N <= 64, K <= 128, K % 4 == 0: include/gnf_hip.h); behind the small-batch kernels it is a column-sum pass
    assert bool(lib().gnf_linear_gxsum_fused(M, dims[2], dims[1], 0)) == (M >= 2048), (M, dims)
    assert lib().gnf_linear_ws_bytes(M, dims[2], dims[1]) > 0
    names = ["x"] + ["%s%d" % (s, l) for l in range(len(dims) - 1) for s in "Wb"]

    def operands():
        g = gen(M)
        x = torch.randn(M, dims[0], generator=g)
        ps = [p for k, n in zip(dims, dims[1:]) for p in (torch.randn(n, k, generator=g) / k ** .5, torch.randn(n, generator=g) * .1)]
        return [x] + ps, torch.randn(M, dims[-1], generator=g)

    def fn():
        ts, gy = operands()
        leaves = [req(t) for t in ts]
        y = ops.mlp(leaves[0], [(leaves[1 + 2 * l], leaves[2 + 2 * l]) for l in range(len(dims) - 1)])
        return dict(grads_of(y, leaves, cu(gy), names), y=y.detach())

    def judge(r):
        ts, gy = operands()
        leaves = [t.double().requires_grad_(True) for t in ts]
        a = leaves[0]
        for l in range(len(dims) - 1):
            a = torch.nn.functional.linear(a, leaves[1 + 2 * l], leaves[2 + 2 * l])
            a = torch.relu(a) if l < len(dims) - 2 else a
        ref = torch.autograd.grad((a * gy.double()).sum(), leaves)
        assert set(r) == {"g" + n for n in names} | {"y"}
        near(r["y"].cpu(), a.detach(), 2e-5, "y")
        for n, g0 in zip(names, ref):
            near(r["g" + n].cpu(), g0, 1e-4, "g" + n)
    three_arms(fn, judge)


# ================================================================================================== Monotonic normalizer
def _mono_operands(hidden, c, B, d, seed, layout="contig"):
    from test_gpu_mono_split import _params
    params = _params(hidden, c, seed=seed, scale=1.3)
    g = gen(B + 7 * d)
    x = (torch.randn(B, d, generator=g) * 2.).to(DEV)
    if layout == "made":                                   # MADE's [B, c d] output viewed as [B, d, c]: strides (c d, 1, d)
        h = torch.randn(B, c, d, generator=g).to(DEV).permute(0, 2, 1)
    else:
        h = torch.randn(B, d, c, generator=g).to(DEV)
    gz, gjac = torch.randn(B, d, generator=g).to(DEV), torch.randn(B, d, generator=g).to(DEV)
    return params, x, h, gz, gjac


NARROW, WIDE7, WIDE10 = [50, 50, 50], [100, 100, 100], [150, 150, 150]
# the ragged sizes of test_monotonic_ragged_sizes (B d % 16 != 0), more than one 16-element group, the strided h
MONO_OPS = [(NARROW, 1, 1, "contig"), (NARROW, 3, 7, "contig"), (NARROW, 5, 13, "made"), (NARROW, 40, 13, "contig"),
            (WIDE7, 3, 7, "contig"), (WIDE7, 5, 13, "made"), (WIDE10, 1, 1, "contig"), (WIDE10, 3, 7, "made"),
            (WIDE10, 5, 13, "contig"), (WIDE10, 50, 9, "contig")]


@pytest.mark.parametrize("hidden,B,d,layout", MONO_OPS, ids=["H%d-%dx%d-%s" % (c[0][0], c[1], c[2], c[3]) for c in MONO_OPS])
def test_monotonic_through_ops(hidden, B, d, layout):
    """ops.MonotonicFn forward + backward: z, jac, the weight image, gx, gh, every parameter gradient and the workspace
    (staged rows / accumulator rows / partial rows) poisoned.  The peeled pair kernel with in-kernel weight gradients (H = 50),
    the wide kernel at HT 7 (fp32 chain) and HT 10 (split-bf16 chain, the library memsets the partial rows)."""
    from gnf_hip import ops
    c = 30
    split = bool(lib().gnf_gemm_split_enabled())
    want = {50: "mono_bwd_pair_x_k<split>" if split else "mono_bwd_k", 100: "mono_bwd_wide_k<f32>",
            150: "mono_bwd_wide_k<split>" if split else "mono_bwd_wide_k<f32>"}[hidden[0]]

    def fn():
        params, x, h, gz, gjac = _mono_operands(hidden, c, B, d, seed=sum(hidden))
        leaves = [x.requires_grad_(True), h.requires_grad_(True)] + [p.requires_grad_(True) for p in params]
        z, jac = ops.MonotonicFn.apply(leaves[0], leaves[1], 20, *leaves[2:])
        fk = lib().gnf_monotonic_fwd_kernel().decode()
        gs = torch.autograd.grad([z, jac], leaves, grad_outputs=[gz, gjac])
        out = {"g%d" % i: g for i, g in enumerate(gs)}
        out.update(z=z.detach(), jac=jac.detach(), fwd_kernel=fk, bwd_kernel=lib().gnf_monotonic_bwd_kernel().decode())
        return out

    def judge(r):
        assert r["bwd_kernel"] == want, r["bwd_kernel"]
        assert r["g1"].shape == (B, d, c) and len(r) == 2 + 2 * (len(hidden) + 1) + 4
    three_arms(fn, judge)


def _chunked_cases():
    from test_gpu_mono_split import CHUNKED
    return CHUNKED


@pytest.mark.parametrize("which", range(8))
@pytest.mark.parametrize("ws", ["one_chunk", "full"])
def test_monotonic_backward_in_chunks(which, ws):
    """the backward families of tests/test_gpu_mono_split.py CHUNKED (bwd_route: PairXSplit, Pair, Ones with the staged rows
    through the split-K GEMM, Image, Wide split and its GNF_TRUE_F32 twin, Resident = HT 7 outside the wide kernel, Streamed =
    HT 16; PairX, the GNF_TRUE_F32 twin of the peeled pair kernel, is test_monotonic_narrow_backward_true_f32's).  NOT reached
    by any case of this file: OneMatrix (HT 7 / 10 nets whose hidden matrices do not fit the LDS together and that the wide
    kernel declines) and the one-node InDw route (GNF_MONO_INDW=1, read once per process: a measurement switch).
    At n = 40 elements, with the full workspace and with one that holds a single 16-element chunk: chunks of 16, 16 and 8,
    every staged product and partial row accumulated across them (GNF_GEMM_ACCUM), the last chunk short"""
    from gnf_hip import ops
    from test_gpu_mono_split import _bwd
    hidden, c, entry = _chunked_cases()[which]
    B, d, S = 5, 8, 20

    def fn():
        params, x, h, gz, gjac = _mono_operands(hidden, c, B, d, seed=sum(hidden) + c)
        net = ops._mono_net(params)
        full = lib().gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), S, B, d)
        one = lib().gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), S, 1, 1)
        assert 0 < one < full
        gs, k = _bwd(entry, params, x, h, S, gz, gjac, ws_bytes=one if ws == "one_chunk" else None)
        return dict({"g%d" % i: g for i, g in enumerate(gs)}, kernel=k)
    r = three_arms(fn)
    if max(hidden) == 150:
        split = entry == "gnf_monotonic_bwd" and lib().gnf_gemm_split_enabled()
        assert r["kernel"] == ("mono_bwd_wide_k<split>" if split else "mono_bwd_wide_k<f32>"), r["kernel"]
    elif hidden == [50, 50, 50] and lib().gnf_gemm_split_enabled():
        assert r["kernel"] == "mono_bwd_pair_x_k<split>", r["kernel"]
    else:
        assert r["kernel"] == "mono_bwd_k", r["kernel"]


@pytest.mark.parametrize("B,d,ws", [(1, 1, "full"), (5, 8, "full"), (5, 8, "one_chunk")], ids=["1x1", "5x8", "5x8-one_chunk"])
def test_monotonic_narrow_backward_true_f32(B, d, ws):
    """the GNF_TRUE_F32 arm of the peeled narrow net [50, 50, 50], c = 30 (gnf_monotonic_bwd_f32): bwd_route takes PairX where the
    default takes PairXSplit -- another kernel, another LDS plan, its own decision (wcomb) about who owns the accumulator rows.
    The smallest case of NBCASES (one element) and n = 40 with the full and the one-chunk workspace (chunks of 16, 16 and 8)"""
    from gnf_hip import ops
    from test_gpu_mono_split import _bwd
    hidden, c, S = [50, 50, 50], 30, 20

    def fn():
        params, x, h, gz, gjac = _mono_operands(hidden, c, B, d, seed=sum(hidden) + c)
        net = ops._mono_net(params)
        one = lib().gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), S, 1, 1)
        assert 0 < one and (B * d <= 16 or one < lib().gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), S, B, d))
        gs, k = _bwd("gnf_monotonic_bwd_f32", params, x, h, S, gz, gjac, ws_bytes=one if ws == "one_chunk" else None)
        return dict({"g%d" % i: g for i, g in enumerate(gs)}, kernel=k)
    r = three_arms(fn)
    assert r["kernel"] == "mono_bwd_k", r["kernel"]


@pytest.mark.parametrize("hidden,R,n", [([20, 20], 5, 33), ([50, 50, 50], 1, 3), ([150, 150, 150], 3, 20)])
def test_monotonic_inverse(hidden, R, n):
    """ops.monotonic_inverse: the plain result (a fresh tensor) and the scattered one -- the caller's `out` is initialised by the
    test, and the columns not named in out_cols come back untouched"""
    from gnf_hip import ops
    from test_gpu_mono_split import _params
    width = 40

    def fn():
        params = _params(hidden, 30, seed=4)
        g = gen(R + n)
        z, h = cu(torch.randn(R, n, generator=g)), cu(torch.randn(R, n, 30, generator=g))
        cols = torch.randperm(width, generator=g)[:R].to(torch.int32).to(DEV)
        x = ops.monotonic_inverse(z, h, 20, params)
        out = torch.full((n, width), 7.5, device=DEV)
        ops.monotonic_inverse(z, h, 20, params, out=out, out_cols=cols)
        assert torch.equal(out[:, cols.long()], x.t())
        rest = torch.ones(width, dtype=torch.bool, device=DEV)
        rest[cols.long()] = False
        assert bool((out[:, rest] == 7.5).all())
        return {"x": x, "out": out}
    three_arms(fn)


# ================================================================================================== MADE inversion, adjoint
def _made(d, c, hidden, seed=3):
    from test_gpu_rsample import _flow
    return _flow("made", d, c, hidden, seed=seed)


MADE_CASES = [(17, 0, [40, 33, 19], 70), (3, 0, [40, 33], 70), (17, 3, [40, 33, 19], 37), (3, 1, [40, 33], 37), (5, 2, [19], 3)]


@pytest.mark.parametrize("d,c,hidden,B", MADE_CASES, ids=["d%d-c%d-B%d" % (k[0], k[1], k[3]) for k in MADE_CASES])
def test_made_inversion(d, c, hidden, B):
    """the column-by-column inversion: the whole sweep in one launch (activations in LDS; in the workspace:
    test_made_whole_inversion_in_the_workspace_form), the sweep in two ranges and step by
    step through the carried workspace (the lane-group dot path, d = 17; the MFMA path, d = 3; B leaves the last tile of rows
    ragged), without and with a context; the weight image, the workspace and the fresh x poisoned"""
    from gnf_hip import ops

    def fn():
        flow = _made(d, c, hidden)
        cond = flow.steps[0].conditioner
        g = gen(B + d)
        z = cu(.7 * torch.randn(B, d, generator=g))
        ctx = cu(torch.randn(B, c, generator=g)) if c else None
        plan, params = cond.prefix_plan(with_context=bool(c)), cond._prefix_params()
        assert plan is not None
        pack = ops.made_prefix_pack(params, plan)
        kw = {"context": ctx} if c else {}
        with torch.no_grad():
            whole = flow.steps[0].invert(z, ctx) if c else flow.steps[0].invert(z)
        lds = ops.made_prefix_steps(params, plan, pack, z, torch.empty_like(z), 0, d, ops.MADE_NORM_AFFINE, **kw)
        k = max(d // 2, 1)
        ws = ops.made_prefix_workspace(params, plan, B)
        two = torch.empty_like(z)
        ops.made_prefix_steps(params, plan, pack, z, two, 0, k, ops.MADE_NORM_AFFINE, ws=ws, **kw)
        ops.made_prefix_steps(params, plan, pack, z, two, k, d, ops.MADE_NORM_AFFINE, ws=ws, **kw)
        ws = ops.made_prefix_workspace(params, plan, B)
        steps = torch.empty_like(z)
        for t in range(d):
            ops.made_prefix_steps(params, plan, pack, z, steps, t, t + 1, ops.MADE_NORM_AFFINE, ws=ws, **kw)
        assert torch.equal(lds, whole) and torch.equal(two, whole) and torch.equal(steps, whole)       # same code, same order
        return {"whole": whole, "lds": lds, "two": two, "steps": steps, "pack": pack}
    three_arms(fn)


@pytest.mark.parametrize("c", [0, 2])
def test_made_whole_inversion_in_the_workspace_form(c, monkeypatch):
    """a tile's activation rows that do not fit the LDS (16 rows of c + 3 + 1024 + 1024 + 512 floats > 160 KB): the library
    declines the (0, d) call without a workspace (GNF_EWS), ops.made_prefix_steps allocates one and the whole sweep runs on
    made_prefix_k<16, false>; B = 20 leaves the second tile ragged"""
    from gnf_hip import ops
    d, hidden, B = 3, [1024, 1024, 512], 20
    made = []
    real = ops.made_prefix_workspace
    monkeypatch.setattr(ops, "made_prefix_workspace", lambda *a, **k: (made.append(1), real(*a, **k))[1])

    def fn():
        flow = _made(d, c, hidden)
        cond = flow.steps[0].conditioner
        g = gen(B + d)
        z = cu(.7 * torch.randn(B, d, generator=g))
        ctx = cu(torch.randn(B, c, generator=g)) if c else None
        plan, params = cond.prefix_plan(with_context=bool(c)), cond._prefix_params()
        assert plan is not None and 16 * 4 * (c + d + sum(hidden)) > 160 * 1024
        pack = ops.made_prefix_pack(params, plan)
        n0 = len(made)
        x = ops.made_prefix_steps(params, plan, pack, z, torch.empty_like(z), 0, d, ops.MADE_NORM_AFFINE,
                                  **({"context": ctx} if c else {}))
        assert len(made) == n0 + 1, "the whole sweep ran in LDS"
        with torch.no_grad():
            zz, _ = flow(x, ctx) if c else flow(x)
        near(zz, z.double(), 1e-4, "forward(invert(z)) = z")
        return {"x": x}
    three_arms(fn)


def test_made_monotonic_step_inverts_by_columns():
    """flow.steps[0].invert of a MADE + Monotonic step (NormalizingFlowStep._invert_by_columns): the [B, out] buffer the
    GNF_MADE_NORM_NONE prefix step writes and the fused Monotonic inverse reads, the carried workspace and the weight images
    are the allocations of models/; the conditioner module is never called"""
    from test_gpu_rsample import _flow

    def fn():
        flow = _flow("made", 5, 0, [19], seed=3, out=6, integrand=[16, 16])
        step = flow.steps[0]
        z = cu(.7 * torch.randn(9, 5, generator=gen(14)))
        calls = []
        hook = step.conditioner.register_forward_hook(lambda *a: calls.append(1))
        try:
            x = step.invert(z)
        finally:
            hook.remove()
        assert not calls, "the passes ran, not the column schedule"
        with torch.no_grad():
            zz, _ = flow(x)
        near(zz, z.double(), 2e-3, "forward(invert(z)) = z")       # 20-step bisection: tests/test_gpu_made_invert.py
        return {"x": x}
    three_arms(fn)


@pytest.mark.parametrize("d,c,hidden,B", [(17, 0, [40, 33, 19], 37), (3, 1, [40, 33], 37)], ids=["dot", "mfma-ctx"])
def test_made_prefix_reads_only_lower_degrees(d, c, hidden, B):
    """include/gnf_hip.h: a call with t0 > 0 reads only the columns of x of degree < t0.  GNF_MADE_NORM_NONE, one step per call
    through the carried workspace: the columns of degree >= t0 hold the arm's pattern when the call is made and come back
    bit-intact; the conditioner outputs h_out are those of the true sample in every arm"""
    from gnf_hip import ops

    def fn():
        flow = _made(d, c, hidden)
        cond = flow.steps[0].conditioner
        g = gen(B + d)
        z = cu(.7 * torch.randn(B, d, generator=g))
        ctx = cu(torch.randn(B, c, generator=g)) if c else None
        plan, params = cond.prefix_plan(with_context=bool(c)), cond._prefix_params()
        pack = ops.made_prefix_pack(params, plan)
        kw = {"context": ctx} if c else {}
        truth = ops.made_prefix_steps(params, plan, pack, z, torch.zeros_like(z), 0, d, ops.MADE_NORM_AFFINE, **kw)
        var = plan["var_host"]
        x = torch.empty_like(z)                            # every column: the arm's pattern
        ws = ops.made_prefix_workspace(params, plan, B)
        hs = []
        for t in range(d):
            h_out = torch.empty(B, plan["out"], device=DEV)
            ops.made_prefix_steps(params, plan, pack, None, x, t, t + 1, ops.MADE_NORM_NONE, h_out=h_out, ws=ws, **kw)
            assert poison.holds_pattern(x[:, var[t:]]), "step %d wrote a column of x in GNF_MADE_NORM_NONE" % t
            hs.append(h_out)
            x[:, var[t]] = truth[:, var[t]]                # the caller inverts the column
        h = torch.stack(hs, 1)                             # [B, d (degree order), out]
        with torch.no_grad():
            href = cond(truth, ctx) if c else cond(truth)  # [B, d, out] by variable
        near(h, href[:, var].double(), 1e-5, "h_out against the conditioner's forward")
        return {"h": h, "x": x}
    three_arms(fn)


@pytest.mark.parametrize("case", [(17, 3, [40, 33, 19]), (3, 1, [40, 33]), (5, 0, [19])], ids=["dot", "mfma", "c0"])
@pytest.mark.parametrize("force_ws", [False, True], ids=["lds", "ws"])
def test_made_adjoint_both_forms(case, force_ws):
    """ops.made_adjoint with the tile's rows in LDS and in the workspace (force_ws): lambda, the weight image and the workspace
    poisoned; B = 37 leaves the last tile ragged"""
    from gnf_hip import ops
    from test_gpu_rsample import _kernel_operands
    d, c, hidden = case

    def fn():
        cond, x, ctx, g, jac, dzdh = _kernel_operands(d, c, hidden, 37, seed=3)
        plan, params = cond.prefix_plan(with_context=bool(c)), cond._prefix_params()
        pack = ops.made_adjoint_pack(params, plan)
        return {"lam": ops.made_adjoint(params, plan, pack, x, g, jac, dzdh, context=ctx, force_ws=force_ws), "pack": pack}
    three_arms(fn)


@pytest.mark.parametrize("force_ws", [False, True], ids=["lds", "ws"])
@pytest.mark.parametrize("c", [0, 2])
def test_rsample_backward(c, force_ws, monkeypatch):
    """flow.rsample and its backward (ops.InvertFn: the adjoint sweep, one vjp of the step): x and the gradients for z, the
    context and every parameter, the adjoint kernel in both forms"""
    from gnf_hip import ops
    from test_gpu_rsample import _flow, _inputs
    real = ops.made_adjoint
    seen = []

    def adjoint(*a, **k):
        seen.append(1)
        return real(*a, **dict(k, force_ws=force_ws))
    monkeypatch.setattr(ops, "made_adjoint", adjoint)

    def fn():
        flow = _flow("made", 5, c, [19], seed=3, nb_flow=2)
        z, ctx, w = _inputs(9, 5, c, 3)
        z.requires_grad_(True)
        if ctx is not None:
            ctx.requires_grad_(True)
        x = flow.rsample(z, ctx)
        leaves = [z] + ([ctx] if c else []) + list(flow.parameters())
        names = ["z"] + (["ctx"] if c else []) + [n for n, _ in flow.named_parameters()]
        return dict(grads_of(x, leaves, w, names), x=x.detach())
    n0 = len(seen)
    r = three_arms(fn)
    assert len(seen) - n0 == 4 * 2                          # one adjoint sweep per step and run
    assert "gz" in r and (not c or "gctx" in r)


# ================================================================================================== conv fronts
def _mnist_conv_params(g):
    return [torch.randn(16, 1, 3, 3, generator=g) * .3, torch.randn(16, generator=g) * .1,
            torch.randn(16, 16, 3, 3, generator=g) * .1, torch.randn(16, generator=g) * .1]


@pytest.mark.parametrize("path", ["saved_a1", "recompute", "exact_ties"])
@pytest.mark.parametrize("n", [1, 3])
def test_mnist_conv(n, path):
    """ops.mnist_conv / MnistConvFn forward + backward: pooled, the saved conv1 activations (with them and without), ge, the four
    parameter gradients and the per-workgroup partials of the workspace; n = 1 and 3: one partial tile of images"""
    from gnf_hip import ops
    names = ["e", "W1", "b1", "W2", "b2"]

    def fn():
        g = gen(n)
        leaves = [req(t) for t in [torch.randn(n, 784, generator=g)] + _mnist_conv_params(g)]
        gp = cu(torch.randn(n, 2304, generator=g))
        if path == "saved_a1":
            out = ops.mnist_conv(*leaves)                  # grad mode on: the Winograd forward keeps conv1's activations
        else:
            out = ops.MnistConvFn.apply(*leaves, path == "exact_ties")      # no grad_mode: nothing kept, conv1 recomputed
        return dict(grads_of(out, leaves, gp, names), out=out.detach())
    r = three_arms(fn)
    assert set(r) == {"out"} | {"g" + k for k in names}


@pytest.mark.parametrize("gate", ["det", "gumbel"])
def test_dag_conv_front_on_its_plan(gate):
    """ops.dag_conv_front without a gradient for x (B = 1: 784 masked copies): the backward runs on the forward's column plan --
    gnf_mnistcnn_conv_bwd_cols (det: tie-exact forward, conv1 recomputed) / _cols_a1 (gumbel: Winograd forward, saved a1) and
    gnf_dag_gate_bwd_cols; e, the gate table, gec and both workspaces poisoned"""
    from gnf_hip import ops
    from test_gpu_alignment import _window_gate
    names = ["A", "W1", "b1", "W2", "b2"]

    def fn():
        g = gen(4)
        A, x = _window_gate(g, .5), torch.randn(1, 784, generator=g)
        ps = _mnist_conv_params(g)
        gp = cu(torch.randn(784, 2304, generator=g))
        leaves = [req(A)] + [req(p) for p in ps]
        out = ops.dag_conv_front(cu(x), leaves[0], ops.IMP_SOFT, ops.GATE_GUMBEL if gate == "gumbel" else ops.GATE_DET, 0., 1.,
                                 None, None, 11, 3, *leaves[1:], exact_ties=gate == "det")
        return dict(grads_of(out, leaves, gp, names), out=out.detach())
    r = three_arms(fn)
    assert set(r) == {"out"} | {"g" + k for k in names}


def _lenet_params(gi):
    from test_gpu_lenet import conv_params
    return conv_params(gi, 7)


GI = 3                                                     # the smallest supported geometry: (1, 8, 8), k = 2, 16 features


def _geo():
    import lenet_ref
    return lenet_ref.GEOMETRIES[GI][0], lenet_ref.GEOMETRIES[GI][1]


@pytest.mark.parametrize("n", [1, 3, 65])
def test_lenet_front(n):
    """ops.lenet_conv forward + backward at the smallest supported geometry"""
    from gnf_hip import ops
    size_img, k = _geo()
    names = ["e", "W1", "b1", "W2", "b2"]

    def fn():
        g = gen(n)
        leaves = [req(torch.randn(n, 64, generator=g))] + [req(p) for p in _lenet_params(GI)]
        feat = ops.lenet_conv(*leaves, size_img, k)
        return dict(grads_of(feat, leaves, cu(torch.randn(n, 16, generator=g)), names), feat=feat.detach())
    r = three_arms(fn)
    assert set(r) == {"feat"} | {"g" + k_ for k_ in names}


@pytest.mark.parametrize("vm", [False, True], ids=["sample-major", "variable-major"])
@pytest.mark.parametrize("want_gx", [False, True], ids=["params", "params+gx"])
def test_lenet_rows_front(want_gx, vm):
    """ops.lenet_rows_train on a row subset (five of the 64 rows), with and without a gradient for x: the backward's workspace
    differs by want_gx"""
    from gnf_hip import ops
    size_img, k = _geo()
    B, rows = 3, [63, 0, 17, 18, 40]

    def fn():
        g = gen(5)
        x = torch.randn(B, 64, generator=g)
        P = torch.rand(64, 64, generator=g) * (torch.rand(64, 64, generator=g) < .5).float()
        ps = [req(p) for p in _lenet_params(GI)]
        xd = req(x) if want_gx else cu(x)
        feat = ops.lenet_rows_train(xd, cu(P), torch.tensor(rows, dtype=torch.int32, device=DEV), *ps, size_img, k,
                                    variable_major=vm)
        cot = cu(torch.randn(*feat.shape, generator=g))
        leaves, names = ([xd] if want_gx else []) + ps, (["x"] if want_gx else []) + ["W1", "b1", "W2", "b2"]
        with torch.no_grad():
            plain = ops.lenet_rows(cu(x), cu(P), torch.tensor(rows, dtype=torch.int32, device=DEV), *[p.detach() for p in ps],
                                   size_img, k, variable_major=vm)
        return dict(grads_of(feat, leaves, cot, names), feat=feat.detach(), plain=plain)
    r = three_arms(fn)
    assert ("gx" in r) == want_gx and tuple(r["feat"].shape) == ((5, B, 16) if vm else (B, 5, 16))


@pytest.mark.parametrize("gate", ["det", "gumbel"])
def test_lenet_gated_front(gate):
    """ops.dag_lenet_front (the gate fused into the LeNet front) forward + backward for A and the conv parameters: the gate
    table the forward writes and the backward reads, the per-workgroup partials"""
    from gnf_hip import ops
    size_img, k = _geo()
    names = ["A", "W1", "b1", "W2", "b2"]

    def fn():
        g = gen(6)
        x = cu(torch.randn(2, 64, generator=g))
        A = req((torch.rand(64, 64, generator=g) * 1.2 + .2) * (torch.rand(64, 64, generator=g) < .7).float())
        ps = [req(p) for p in _lenet_params(GI)]
        feat = ops.dag_lenet_front(x, A, ops.IMP_SOFT, ops.GATE_GUMBEL if gate == "gumbel" else ops.GATE_DET, 0., 1., None,
                                   None, 11, 3, *ps, size_img, k)
        return dict(grads_of(feat, [A] + ps, cu(torch.randn(2 * 64, 16, generator=g)), names), feat=feat.detach())
    r = three_arms(fn)
    assert set(r) == {"feat"} | {"g" + k_ for k_ in names}


@pytest.mark.parametrize("mode", ["plain", "prepared", "fc12"])
def test_sparse_front_inference(mode):
    """the sparse masked-image front without a backward: tables built per call (gnf_mnistcnn_sparse_ws_bytes), held tables, and
    held tables with the one-launch fc1 + ReLU + fc2 kernel.  The held tables are a tensor ops.mnistcnn_sparse_prepare returns:
    compared whole.  (This case found their last 64 floats -- slack behind the background response that no kernel reads --
    unwritten; sparse_bg_k now stores zeros there.)"""
    from gnf_hip import ops
    from test_gpu_alignment import _sparse_setup

    def fn():
        sr, _, _, vals = _sparse_setup(2)
        t = {k: v.to(DEV) for k, v in vals.items()}
        with torch.no_grad():
            prep = None if mode == "plain" else ops.mnistcnn_sparse_prepare(t["b1"], t["W2"], t["b2"], t["Wfc1"], t["bfc1"])
            if mode == "fc12":
                out = ops.mnistcnn_sparse_fwd_fc2(t["x"], t["P"], sr, t["W1"], t["b1"], t["W2"], t["b2"], prep, t["Wfc2"], t["bfc2"])
            else:
                out = ops.mnistcnn_sparse_fwd(t["x"], t["P"], sr, t["W1"], t["b1"], t["W2"], t["b2"], t["Wfc1"], t["bfc1"],
                                              pre_gated=True, prep=prep)
        return {"out": out} if prep is None else {"out": out, "prep": prep}
    three_arms(fn)


@pytest.mark.parametrize("reuse_tables", [True, False], ids=["bwd_tables", "bwd"])
def test_sparse_front_backward(reuse_tables, monkeypatch):
    """the training path at B = 2 with ten rows: h1, the pooled blocks, the tables, the six parameter gradients and the
    backward's workspace"""
    from gnf_hip import ops
    from test_gpu_alignment import SPARSE_NAMES, _sparse_setup
    monkeypatch.setattr(ops, "SPARSE_REUSE_TABLES", reuse_tables)
    pn = SPARSE_NAMES[2:]

    def fn():
        sr, _, _, vals = _sparse_setup(2)
        t = {k: v.to(DEV) for k, v in vals.items()}
        leaves = [t[k].requires_grad_(True) for k in pn]
        h1 = ops.mnistcnn_sparse_fwd(t["x"], t["P"], sr, *leaves[:6], pre_gated=True)
        out = ops.mlp(h1, [(leaves[6], leaves[7])], relu_in=True)
        return dict(grads_of(out, leaves, cu(torch.randn(*out.shape, generator=gen(1))), pn), out=out.detach())
    r = three_arms(fn)
    assert set(r) == {"out"} | {"g" + k for k in pn}


# ================================================================================================== DAG pieces
def _A(d, g):
    return (torch.rand(d, d, generator=g) * 1.2 + .2) * (torch.rand(d, d, generator=g) < .7).float()


@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hot"])
@pytest.mark.parametrize("gate", ["det", "gumbel", "noise", "gumbel-injected"])
def test_dag_gate(gate, hot):
    """ops.DagGateFn forward + backward in each gate mode at d = 6: e, the (i, j) table the forward writes and the backward
    reads, gx, gA and the backward's per-sample partials"""
    from gnf_hip import ops
    d, B = 6, 5
    gm = {"det": ops.GATE_DET, "gumbel": ops.GATE_GUMBEL, "noise": ops.GATE_NOISE, "gumbel-injected": ops.GATE_GUMBEL}[gate]

    def fn():
        g = gen(d)
        x, A = req(torch.randn(B, d, generator=g)), req(_A(d, g))
        u1 = u2 = None
        if gate == "gumbel-injected":
            u1, u2 = (cu(torch.rand(B, d, d, generator=g).clamp(.02, .98)) for _ in range(2))
        e = ops.DagGateFn.apply(x, A, ops.IMP_SOFT, gm, 0., .5, hot, u1, u2, 11, 3)
        return dict(grads_of(e, [x, A], cu(torch.randn(B * d, 2 * d if hot else d, generator=g)), ["x", "A"]), e=e.detach())
    r = three_arms(fn)
    assert set(r) == {"e", "gx", "gA"}


@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hot"])
@pytest.mark.parametrize("gate", ["det", "gumbel"])
def test_dag_mlp_front_and_rows(gate, hot):
    """ops.dag_mlp_front (gate + first DAGMLP layer, forward + backward) and ops.dag_mlp_rows at d = 6"""
    from gnf_hip import ops
    d, B, H = 6, 7, 20
    gm = ops.GATE_GUMBEL if gate == "gumbel" else ops.GATE_DET

    def fn():
        g = gen(d + H)
        x, A = req(torch.randn(B, d, generator=g)), req(_A(d, g))
        W1 = req(torch.randn(H, 2 * d if hot else d, generator=g) / d ** .5)
        b1 = req(torch.randn(H, generator=g) * .1)
        a1 = ops.dag_mlp_front(x, A, ops.IMP_SOFT, gm, 0., .5, None, None, 11, 3, W1, b1, hot, True)
        out = dict(grads_of(a1, [x, A, W1, b1], cu(torch.randn(B * d, H, generator=g)), ["x", "A", "W1", "b1"]), a1=a1.detach())
        with torch.no_grad():
            rows = torch.tensor([5, 0, 3], dtype=torch.int32, device=DEV)
            P = cu(torch.rand(d, d, generator=g))
            out["rows"] = ops.dag_mlp_rows(x.detach(), P, rows, W1.detach(), b1.detach(), hot, True)
            out["rows_all_vm"] = ops.dag_mlp_rows(x.detach(), P, None, W1.detach(), b1.detach(), hot, False, variable_major=True)
        return out
    r = three_arms(fn)
    assert set(r) == {"a1", "gx", "gA", "gW1", "gb1", "rows", "rows_all_vm"}


class _GateNet(torch.nn.Module):
    def __init__(self, d, H, g):
        super().__init__()
        self.A = torch.nn.Parameter(_A(d, g) * .3)
        self.W1 = torch.nn.Parameter(torch.randn(H, 2 * d, generator=g) / d ** .5)
        self.b1 = torch.nn.Parameter(torch.randn(H, generator=g) * .1)


@pytest.mark.parametrize("order", ["front-first", "loss-first"])
def test_shared_gradient_slot_of_A(order):
    """the DAG matrix receives two contributions per backward (the gate behind the fused front, the acyclicity term) into ONE
    slot of a FlatState's gradient buffer: whichever backward runs first takes the slot, the other adds into it -- the front's
    kernel accumulates itself (acc = 1), the loss goes through a scratch tensor.  Both orders; the packed gradient buffer is the
    result"""
    from gnf_hip import dp, ops
    d, B, H = 6, 7, 20

    def fn():
        g = gen(9)
        net = _GateNet(d, H, g).to(DEV)
        state = dp.FlatState(net)
        x = cu(torch.randn(B, d, generator=g))
        cot = cu(torch.randn(B * d, H, generator=g))

        def front():
            return (ops.dag_mlp_front(x, net.A, ops.IMP_SOFT, ops.GATE_GUMBEL, 0., .5, None, None, 11, 3, net.W1, net.b1, True,
                                      True) * cot).sum()

        def loss():
            return ops.DagLossFn.apply(net.A, 1. / d, 1., .7, .05, 1., .3, d)
        # autograd runs the node created LAST first
        total = (loss() + front()) if order == "front-first" else (front() + loss())
        total.backward()
        state.pack_grads()
        assert state.pack_stats["in_place"] == 3, state.pack_stats
        return {"total": total.detach(), "grad": state.grad.clone()}
    three_arms(fn)


@pytest.mark.parametrize("d", [6, 50])
def test_dag_loss(d):
    """ops.DagLossFn forward + backward: B = I + alpha A o A, the four scalars and the 512 partials of the value kernel"""
    from gnf_hip import ops
    from models import DAGConditioner

    def fn():
        torch.manual_seed(d)
        cond = DAGConditioner(d, [8], 2, l1=.3).to(DEV)
        with torch.no_grad():
            cond.A.mul_(.2)
            cond.lambd.fill_(.7)
            cond.c.fill_(.05)
        A = cond.A.detach().clone().requires_grad_(True)
        loss = ops.DagLossFn.apply(A, cond.alpha, cond.alpha_factor, cond.lambd, cond.c, cond.dag_const, cond.l1_weight,
                                   cond.exponent)
        gA, = torch.autograd.grad(loss, A)
        return {"loss": loss.detach().reshape(1), "gA": gA}
    three_arms(fn)


@pytest.mark.parametrize("d", [6, 84])
def test_dag_levels(d):
    """ops.dag_levels: the workspace is allocated as fp32 and read as 64-bit edge masks -- written whole by dag_pack_k before
    dag_peel_k reads it (module docstring); d = 84: two words per row, the second partly padding"""
    from gnf_hip import ops

    def fn():
        g = gen(d)
        perm = torch.randperm(d, generator=g)
        low = torch.tril(torch.rand(d, d, generator=g), -1) * (torch.rand(d, d, generator=g) < .3).float()
        low[d - 1, 0] = .8                                 # the first node of the hidden order is a parent of the last
        M = torch.zeros(d, d)
        M[perm[:, None], perm[None, :]] = low              # a DAG under a hidden order
        cyc = M.clone()
        cyc[perm[0], perm[d - 1]] = .9                     # one back edge: a cycle
        both = cu(torch.stack([M, cyc]))
        level, info = ops.dag_levels(both)
        l1, i1 = ops.dag_levels(cu(M))
        lt, it = ops.dag_levels(cu(M), thresholds=[0., .5, 2.])
        assert info[0].tolist()[0] == d and info[1].tolist()[0] < d and torch.equal(l1, level[0]) and it[2].tolist() == [d, 1]
        return {"level": level, "info": info, "l1": l1, "i1": i1, "lt": lt, "it": it}
    three_arms(fn)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "identity"])
@pytest.mark.parametrize("H", [8, 7], ids=["quads", "dwords"])
def test_group_bias(H, relu):
    """ops.group_bias forward + backward in the 16-byte form (H % 4 == 0) and the dword form"""
    from gnf_hip import ops
    B, G = 5, 6

    def fn():
        g = gen(H)
        y, cb = req(torch.randn(B * G, H, generator=g)), req(torch.randn(B, H, generator=g))
        out = ops.group_bias(y, cb, G, relu)
        return dict(grads_of(out, [y, cb], cu(torch.randn(B * G, H, generator=g)), ["y", "cb"]), out=out.detach())

    def judge(r):
        g = gen(H)
        y, cb = torch.randn(B * G, H, generator=g), torch.randn(B, H, generator=g)
        want = y + cb.repeat_interleave(G, 0)
        assert torch.equal(r["out"].cpu(), torch.relu(want) if relu else want)
    three_arms(fn, judge)


# ================================================================================================== row-wise kernels
# the four kernel families of ROW_SHAPES (tests/test_gpu_alignment.py): generic lane groups; a workgroup per row; 16-lane
# groups; the flat span kernels
ROW_SHAPES = [(7, 5), (3, 257), (1041, 63), (4162, 63)]


@pytest.mark.parametrize("layout", ["contig", "made"])
@pytest.mark.parametrize("B,d", ROW_SHAPES)
def test_affine(B, d, layout):
    """ops.AffineFn forward (with and without jac / logN) + backward, ops.affine_inverse"""
    from gnf_hip import ops
    from test_gpu_alignment import _h

    def fn():
        g = gen(B + d)
        x, h = req(torch.randn(B, d, generator=g)), _h(B, d, layout, g).to(DEV).requires_grad_(True)
        gz, gj, gl, gn = (cu(torch.randn(s, generator=g)) for s in ((B, d), (B, d), (B,), (B,)))
        z, jac, logdet, logn = ops.AffineFn.apply(x, h, False, True, True)
        out = {"z": z.detach(), "jac": jac.detach(), "logdet": logdet.detach(), "logn": logn.detach()}
        gs = torch.autograd.grad([z, jac, logdet, logn], [x, h], grad_outputs=[gz, gj, gl, gn])
        out.update(gx=gs[0], gh=gs[1])
        z2, _, ld2, _ = ops.AffineFn.apply(x, h, False, False, False)       # the fused step's form: no jac, no logN
        gs2 = torch.autograd.grad([z2, ld2], [x, h], grad_outputs=[gz, gl])
        out.update(gx2=gs2[0], gh2=gs2[1], inv=ops.affine_inverse(z.detach(), h.detach()))
        assert gs[1].stride() == h.stride()
        return out

    def judge(r):
        near(r["inv"].cpu(), torch.randn(B, d, generator=gen(B + d)), 1e-4, "inverse(forward(x)) = x")
    three_arms(fn, judge)


@pytest.mark.parametrize("B,d", ROW_SHAPES)
def test_row_reductions_and_losses(B, d):
    """the NLL reduce, the stand-alone row reductions, the batch mean and the one-launch loss, each forward + backward"""
    from gnf_hip import ops

    def fn():
        g = gen(B + d)
        z, jac = req(torch.randn(B, d, generator=g)), req(torch.rand(B, d, generator=g) * 3 + .05)
        gl, gn = cu(torch.randn(B, generator=g)), cu(torch.randn(B, generator=g))
        addend = cu(torch.randn((), generator=g))
        out = {}
        logdet, logn = ops.NllReduceFn.apply(z, jac)
        out["r_gz"], out["r_gjac"] = torch.autograd.grad([logdet, logn], [z, jac], grad_outputs=[gl, gn])
        ls, nd = ops.LogSumRowsFn.apply(jac), ops.NormalLogDensityFn.apply(z)
        out["ls_gjac"], = torch.autograd.grad(ls, jac, gl)
        out["nd_gz"], = torch.autograd.grad(nd, z, gn)
        ld, ln = logdet.detach().requires_grad_(True), logn.detach().requires_grad_(True)
        mean = ops.NllMeanFn.apply(ld, ln, addend)
        out["m_gld"], out["m_gln"] = torch.autograd.grad(mean, [ld, ln])
        assert ops.nll_loss_fits(z)
        loss = ops.NllLossFn.apply(z, ld, addend)
        out["l_gz"], out["l_gld"] = torch.autograd.grad(loss, [z, ld])
        out.update(logdet=logdet.detach(), logn=logn.detach(), ls=ls.detach(), nd=nd.detach(), mean=mean.detach().reshape(1),
                   loss=loss.detach().reshape(1))
        return out

    def judge(r):
        assert torch.equal(r["ls"], r["logdet"]) and torch.equal(r["nd"], r["logn"])
        near(r["loss"], r["mean"].double(), 1e-5, "the loss from z = the mean of the reductions")
    three_arms(fn, judge)


def test_image_prep_toy_sample_tab_batch():
    """the batch makers with out=None: the tensors they return are contiguous -- no row pitch, no padding -- and compared whole"""
    from gnf_hip import ops

    def fn():
        g = gen(2)
        data = cu(torch.randint(0, 256, (9, 64), generator=g, dtype=torch.uint8))
        rows = torch.tensor([8, 0, 3, 3, 5], dtype=torch.int32, device=DEV)
        x, term = ops.image_prep(data, rows, True, None, 7, 2, .05, (1, 8, 8), True)
        x3, term3 = ops.image_prep(cu(torch.randint(0, 256, (3, 3 * 32 * 32), generator=g, dtype=torch.uint8)), None, None,
                                   None, 7, 3, .05, (3, 32, 32), True)
        toy = ops.toy_sample("8-MIX", 37, 5, 1, DEV)
        toy1 = ops.toy_sample(["moons"], 1, 5, 2, DEV)
        X = cu(torch.randn(50, 21, generator=g))
        perm = torch.randperm(50, generator=g).to(torch.int32).to(DEV)
        tb = ops.tab_batch(X[:, 2:19], perm, 3, 2, 13)
        tb1 = ops.tab_batch(X, None, 0, 1, 7, cursor=torch.tensor([4], dtype=torch.int32, device=DEV))
        keys = ops.shuffle_keys(3, 1, 50, device=DEV)
        assert all(t.is_contiguous() for t in (x, term, x3, toy, toy1, tb, tb1))
        return {"x": x, "term": term, "x3": x3, "term3": term3, "toy": toy, "toy1": toy1, "tb": tb, "tb1": tb1, "keys": keys}
    three_arms(fn)


# ================================================================================================== whole training steps
def _affine_made():
    from models import AffineNormalizer, AutoregressiveConditioner, buildFCNormalizingFlow
    torch.manual_seed(31)
    return buildFCNormalizingFlow(2, AutoregressiveConditioner, {"in_size": 7, "hidden": [24, 24], "out_size": 2}, AffineNormalizer,
                                  {}).to(DEV), 7, 0


def _monotonic_dag():
    from gnf_hip import dp
    from models import DAGConditioner, MonotonicNormalizer, buildFCNormalizingFlow
    torch.manual_seed(32)
    flow = buildFCNormalizingFlow(2, DAGConditioner, {"in_size": 6, "hidden": [20, 20], "out_size": 10, "hot_encoding": True,
                                                      "gumble_T": .5, "l1": .2},
                                  MonotonicNormalizer, {"integrand_net": [16, 16], "cond_size": 10, "nb_steps": 10}).to(DEV)
    dp.seed_gates(flow, 0)
    return flow, 6, 0


def _conditional():
    from gnf_hip import dp
    from models import AffineNormalizer, DAGConditioner, buildFCNormalizingFlow
    torch.manual_seed(11)
    flow = buildFCNormalizingFlow(2, DAGConditioner, {"in_size": 5, "hidden": [16, 16], "out_size": 2, "cond_in": 2},
                                  AffineNormalizer, {}).to(DEV)
    dp.seed_gates(flow, 0)
    return flow, 5, 2


@pytest.mark.parametrize("build", [_affine_made, _monotonic_dag, _conditional], ids=["affine-made", "monotonic-dag", "conditional-dag"])
def test_two_eager_training_steps(build):
    """two dp.train_step(graph=False) on a FlatState: here the gradient slots (ops.grad_out, grad_out_shared), pack_grads' zeroing
    of the slots nobody took and the Adam kernel meet -- a slot one backward leaves partly unwritten shows in state.grad and,
    one step later, in the parameters and moments"""
    from gnf_hip import dp

    def fn():
        flow, d, c = build()
        state = dp.FlatState(flow)
        g = gen(12)
        losses = []
        for _ in range(2):
            x = cu(torch.randn(20, d, generator=g))
            ctx = cu(torch.randn(20, c, generator=g)) if c else None
            losses.append(dp.train_step(flow, state, x, graph=False, context=ctx).detach().reshape(1).clone())
        assert state.t == 2 and getattr(state, "_graphed", None) is None
        return {"loss1": losses[0], "loss2": losses[1], "flat": state.flat.clone(), "grad": state.grad.clone(),
                "m": state.m.clone(), "v": state.v.clone()}
    r = three_arms(fn)
    assert bool(r["m"].abs().sum() > 0)
