"""GPU: the training form of the row-subset LeNet front of CIFAR10CNN behind a FROZEN deterministic DAG gate
(gnf_lenet_rows_fwd_arg / gnf_lenet_rows_bwd, gnf_hip.ops.LenetRowsFn / lenet_rows_train, CIFAR10CNN.rows_train_front): the
masked copies x[b] * P[rows[r]] are built in LDS forward and backward, neither the [B, R, d] product nor its cotangent exists
in memory, and dL/dx is summed over the rows in registers.

The yardstick is the composed path (`rows_train_front = False`: DagGateFn or the broadcast product, then LenetConvFn), which
tests/test_gpu_lenet.py holds to the fp64 oracle.  A copy is ONE fp32 product on both sides, so the forward agrees BIT FOR
BIT, every ReLU and pool decision is the same on both sides and the gradient comparisons need no knife-edge handling.
Gradient tolerance: rel_err < 1e-4 of the tensor maximum and |a - b| <= 1e-6 max|b| + 1e-4 |b| per
entry.  One test compares against the fp64 restatement directly, with the knife-edge condition of tests/test_gpu_lenet.py.
Every test sets `rows_train_front` itself: none depends on ROWS_TRAIN_FRONT_DEFAULT."""
import ctypes
import os

import pytest
import torch

from conftest import assert_fwd, rel_err
import lenet_ref
from lenet_ref import DEV, assert_grad, cu, geo_args, graph_nodes
import misaligned

pytestmark = pytest.mark.gpu
GEOS = lenet_ref.GEOMETRIES
FEAT = (400, 576, 64, 16)
DIMS = tuple(s[0] * s[1] * s[2] for s, _, _ in GEOS)          # 3072, 1024, 256, 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPOSED = {"DagGateFnBackward", "LenetConvFnBackward"}


def row_sets(d):
    """one row; five unsorted rows, one of them twice; None = all d rows in order"""
    return {"one": [d // 3], "five": [d - 1, 2, d // 2, 2, 5], "all": None}


def importance(kind, d, gen):
    """what post_process() leaves -- 0/1 at density 0.1, zero diagonal -- or uniform [0, 1)"""
    if kind == "uniform":
        return torch.rand(d, d, generator=gen)
    return (torch.rand(d, d, generator=gen) < .1).float() * (1. - torch.eye(d))


def make_conditioner(gi, P=None, seed=70):
    """DAGConditioner over CIFAR10CNN with a deterministic gate on the raw A; P given: A = P, frozen"""
    from models import DAGConditioner
    from models.MLP import CIFAR10CNN
    size_img, k, fc_l = GEOS[gi]
    torch.manual_seed(seed + gi)
    net = CIFAR10CNN(out_d=2, fc_l=list(fc_l), size_img=list(size_img), k_size=k)
    cond = DAGConditioner(DIMS[gi], net, 2)
    cond.stoch_gate = cond.noise_gate = cond.s_thresh = False
    cond.h_thresh = 0.
    if P is not None:
        with torch.no_grad():
            cond.A.copy_(P)
        cond.A.requires_grad = False
    cond.invalidate_caches()
    return cond.to(DEV)


def run(cond, x, cot, on, x_grad, rows=None, vm=False):
    """one forward + backward of the conditioner with `rows_train_front = on` ->
    (h, {parameter gradients}, x.grad, A.grad, autograd node names)"""
    net = cond.embedding_net
    net.rows_train_front = on
    cond.zero_grad(set_to_none=True)
    cond.gate_seed, cond._gate_calls = 1234567, 40
    xd = x.clone().requires_grad_(x_grad)
    with torch.enable_grad():
        if rows is None:
            h = cond(xd)
        else:
            h = cond.forward_rows(xd, torch.tensor(rows, device=DEV), cond.deterministic_importance(), tuple(rows),
                                  variable_major=vm)
        nodes = graph_nodes(h)
        (h * cot).sum().backward()
    return (h.detach(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, xd.grad,
            None if cond.A.grad is None else cond.A.grad.clone(), nodes)


# each geometry at B = 1 and at one more B: 30 and 7 leave the last group of IPB = 28 / 5 samples partial (two groups);
# d = 1024 and 3072 (IPB = 1) over all rows have more units than the backward's 512 workgroups: the grid-stride loop
CASES = [(gi, B, rs, kind) for gi, Bs in ((3, (1, 30)), (2, (1, 7))) for B in Bs for rs in ("one", "five", "all")
         for kind in ("01", "uniform")]
CASES += [(gi, B, "all", kind) for gi in (1, 0) for B in (1, 2) for kind in ("01", "uniform")]
IDS = ["d%d-B%d-%s-P%s" % (DIMS[gi], B, rs, kind) for gi, B, rs, kind in CASES]
_runs = {}


def both_paths(gi, B, rs, kind):
    """per x_grad in (False, True): the composed reference and two runs of the rows front of one case, computed once and
    shared by the tests below -> (x, P, rows, {x_grad: (ref, got, again)})"""
    key = (gi, B, rs, kind)
    if key not in _runs:
        d = DIMS[gi]
        gen = torch.Generator().manual_seed(5000 + 100 * gi + B)
        x, P = cu(torch.randn(B, d, generator=gen)), importance(kind, d, gen)
        rows = row_sets(d)[rs]
        R = d if rows is None else len(rows)
        cot = cu(torch.randn(B, R, 2, generator=gen))
        cond = make_conditioner(gi, P)
        _runs[key] = (x, cu(P), rows, cond,
                      {xg: (run(cond, x, cot, False, xg, rows), run(cond, x, cot, True, xg, rows),
                            run(cond, x, cot, True, xg, rows)) for xg in (False, True)})
    return _runs[key]


# ------------------------------------------------------------------------------------------- 1. forward bits
@pytest.mark.parametrize("gi,B,rs,kind", CASES, ids=IDS)
def test_forward_bits_equal_the_composed_path(gi, B, rs, kind):
    from gnf_hip import ops
    x, P, rows, cond, runs = both_paths(gi, B, rs, kind)
    d = DIMS[gi]
    R = d if rows is None else len(rows)
    for xg in (False, True):
        ref, got, _ = runs[xg]
        assert got[0].shape == (B, R, 2) and bool(torch.isfinite(ref[0]).all()) and float(ref[0].abs().max()) > 0
        assert torch.equal(got[0], ref[0]), xg                  # the conditioner output, autograd on
    # the features of the node against the conv front on the materialised product, both layouts, autograd on
    net = cond.embedding_net
    W = [net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv2.bias]
    rows32 = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=DEV)
    Pr = P if rows is None else P[torch.tensor(rows, device=DEV)]
    with torch.enable_grad():
        e = (x[:, None, :] * Pr[None]).reshape(B * R, d)
        feat0 = ops.lenet_conv(e, *W, GEOS[gi][0], GEOS[gi][1]).detach().view(B, R, -1)
        for vm in (False, True):
            feat = ops.lenet_rows_train(x.clone().requires_grad_(True), P, rows32, *W, GEOS[gi][0], GEOS[gi][1], vm)
            assert feat.requires_grad and type(feat.grad_fn).__name__ == "LenetRowsFnBackward"
            assert feat.shape == ((R, B, FEAT[gi]) if vm else (B, R, FEAT[gi])) and feat.is_contiguous()
            assert torch.equal(feat.detach(), feat0.permute(1, 0, 2) if vm else feat0), vm
    if rows is not None:                                        # [R, B, out] through the conditioner: the fc chain sees the
        cot = torch.ones(R, B, 2, device=DEV)                   # rows in another order, hence the forward tolerance
        off, on = run(cond, x, cot, False, True, rows, True), run(cond, x, cot, True, True, rows, True)
        assert on[0].shape == (R, B, 2) and "LenetRowsFnBackward" in on[4]
        assert_fwd(on[0], off[0], what="h, variable-major")
        assert_grad(on[2], off[2], "x.grad, variable-major")


# ------------------------------------------------------------------------------------------- 2. backward
@pytest.mark.parametrize("gi,B,rs,kind", CASES, ids=IDS)
def test_backward_against_the_composed_path(gi, B, rs, kind):
    x, P, rows, cond, runs = both_paths(gi, B, rs, kind)
    for xg in (False, True):
        ref, got, again = runs[xg]
        assert "LenetRowsFnBackward" in got[4] and not (got[4] & COMPOSED)
        assert "LenetRowsFnBackward" not in ref[4] and "LenetConvFnBackward" in ref[4]
        if rows is None and xg:                                 # forward(): the gate node; forward_rows: a torch product
            assert "DagGateFnBackward" in ref[4]
        assert set(got[1]) == set(ref[1]) and len(ref[1]) == 10
        for n in ref[1]:
            assert float(ref[1][n].abs().max()) > 0, n
            assert_grad(got[1][n], ref[1][n], n)
            assert torch.equal(got[1][n], again[1][n]), n       # the same call, the same bits
        assert got[3] is None and ref[3] is None                # A is frozen
        if xg:
            assert got[2].shape == x.shape
            assert_grad(got[2], ref[2], "x.grad")
            assert torch.equal(got[2], again[2])
        else:
            assert got[2] is None and ref[2] is None


# ------------------------------------------------------------------------------------------- 3. fp64, without the composed path
def fp64_case(gi, kind):
    """operands of test_against_fp64 (CPU tensors): conditioner, x, P, knife flags of the B*d copies"""
    d, B = DIMS[gi], 3
    gen = torch.Generator().manual_seed(5200 + gi)
    x, P = torch.randn(B, d, generator=gen), importance(kind, d, gen)
    cond = make_conditioner(gi, P)
    p = {n: q.detach().cpu().clone() for n, q in cond.embedding_net.named_parameters()}
    e = (x[:, None, :] * P[None]).reshape(B * d, d)
    knife = lenet_ref.knife_images(e, p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"], GEOS[gi][0])
    cot = torch.randn(B * d, 2, generator=gen) * (~knife).float().unsqueeze(1)      # knife copies: zero cotangent
    return cond, p, x, P, knife, cot


@pytest.mark.parametrize("kind", ["01", "uniform"])
@pytest.mark.parametrize("gi", [3, 2], ids=["d64", "d256"])
def test_against_fp64(gi, kind):
    """d = 64 / 256, B = 3, all rows, x.requires_grad: lenet_ref.cifar10cnn in fp64 on the fp32 products x.unsqueeze(1) * P.
    Copies holding a knife-edge decision get a zero cotangent; at most 5 % of the copies may be left out (a condition,
    not a tolerance).  Flagged share of exactly these inputs, computed on the CPU with lenet_ref.knife_images:
    d64-01 0 of 192, d64-uniform 0 of 192, d256-01 3 of 768 (0.39 %), d256-uniform 4 of 768 (0.52 %)."""
    d, B, size_img = DIMS[gi], 3, GEOS[gi][0]
    cond, p, x, P, knife, cot = fp64_case(gi, kind)
    share = float(knife.float().mean())
    print("knife-edge copies: %d of %d (%.2f %%)" % (int(knife.sum()), knife.numel(), 100 * share))
    assert share <= .05, share
    x0 = x.clone().requires_grad_(True)
    p64 = {n: v.double().requires_grad_(True) for n, v in p.items()}
    h0 = lenet_ref.cifar10cnn((x0[:, None, :] * P[None]).reshape(B * d, d).double(), p64, size_img)
    names = list(p64)
    grads = torch.autograd.grad((h0 * cot.double()).sum(), [x0] + [p64[n] for n in names])
    h, gp, gx, _, nodes = run(cond, cu(x), cu(cot).view(B, d, 2), True, True)
    assert "LenetRowsFnBackward" in nodes and not (nodes & COMPOSED)
    assert_fwd(h.reshape(B * d, 2), h0.detach(), what="h")
    assert_grad(gx, grads[0], "x.grad")
    for n, g0 in zip(names, grads[1:]):
        assert_grad(gp[n], g0, n)


# ------------------------------------------------------------------------------------------- 4. fallbacks
def _fallback_setup(gi=2, B=3):
    d = DIMS[gi]
    gen = torch.Generator().manual_seed(5400 + gi)
    x, P = cu(torch.randn(B, d, generator=gen)), importance("01", d, gen)
    return make_conditioner(gi, P), x, cu(torch.randn(B, d, 2, generator=gen))


def _same_as_switched_off(cond, x, cot, x_grad, same=torch.equal):
    """the switch changes nothing: the same nodes, the same output bits, the same gradients (`same`: bit for bit where the
    backward is this package's kernels, which sum in a fixed order)"""
    off, on = run(cond, x, cot, False, x_grad), run(cond, x, cot, True, x_grad)
    assert "DagGateFnBackward" in on[4] and "LenetRowsFnBackward" not in on[4], on[4]
    assert on[4] == off[4]
    assert torch.equal(on[0], off[0])
    assert set(on[1]) == set(off[1]) and len(off[1]) == 10
    for n in off[1]:
        assert same(on[1][n], off[1][n]), n
    for a, b in ((on[2], off[2]), (on[3], off[3])):
        assert (a is None and b is None) or same(a, b)
    return on


def test_trainable_A_keeps_the_composed_nodes():
    cond, x, cot = _fallback_setup()
    with torch.no_grad():
        cond.A.copy_(cu(1.5 + .02 * torch.randn(256, 256, generator=torch.Generator().manual_seed(1))))
    cond.A.requires_grad = True
    on = _same_as_switched_off(cond, x, cot, False)
    assert on[3] is not None and float(on[3].abs().max()) > 0      # the gate's gradient still arrives


def test_gumbel_gate_keeps_the_composed_nodes():
    cond, x, cot = _fallback_setup()
    with torch.no_grad():
        cond.A.copy_(cu(1.5 + .02 * torch.randn(256, 256, generator=torch.Generator().manual_seed(2))))
    cond.stoch_gate = cond.s_thresh = True
    cond.invalidate_caches()
    assert cond.deterministic_importance() is None
    _same_as_switched_off(cond, x, cot, True)


def test_hot_encoding_keeps_the_composed_nodes():
    cond, x, cot = _fallback_setup()
    net = cond.embedding_net
    cond.hot_encoding = True
    seen = []

    def no_rows(*a, **k):
        raise AssertionError("the rows front has no one-hot columns")

    def record(e, context=None):                                # CIFAR10CNN itself takes no one-hot columns
        seen.append(tuple(e.shape))
        return e[:, :2] * net.fc3.bias

    net.forward_rows, net.forward = no_rows, record
    off, on = run(cond, x, cot, False, True), run(cond, x, cot, True, True)
    assert seen == [(3 * 256, 512)] * 2
    assert "DagGateFnBackward" in on[4] and on[4] == off[4]
    assert torch.equal(on[0], off[0]) and torch.equal(on[2], off[2])


def test_torch_convolutions_keep_the_composed_nodes():
    cond, x, cot = _fallback_setup()
    cond.embedding_net.fused_front = False
    assert not cond.embedding_net.supports_rows_train(x)

    def same(a, b):                                             # the library's convolution backward sums with atomics: two
        assert_grad(a, b, "torch convolutions")                 # runs of the SAME statements differ in the last bits
        return True
    on = _same_as_switched_off(cond, x, cot, True, same)
    assert "LenetConvFnBackward" not in on[4]


def test_an_importance_matrix_that_requires_grad_is_refused():
    from gnf_hip import abi, ops
    cond, x, _ = _fallback_setup()
    net = cond.embedding_net
    W = [net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv2.bias]
    P = cond.A.detach().clone().requires_grad_(True)
    with pytest.raises(abi.GnfError):
        ops.lenet_rows_train(x, P, None, *W, GEOS[2][0], GEOS[2][1])
    assert ops.lenet_rows_train(x, P.detach(), None, *W, GEOS[2][0], GEOS[2][1]).requires_grad


# ------------------------------------------------------------------------------------------- raw entry points
def conv_params(gi, seed):
    size_img, k, _ = GEOS[gi]
    torch.manual_seed(seed)
    c1, c2 = torch.nn.Conv2d(size_img[0], 6, k), torch.nn.Conv2d(6, 16, k)
    return [cu(t.detach().clone()) for t in (c1.weight, c1.bias, c2.weight, c2.bias)]


def raw_fwd(x, P, rows, R, W, gi, B, vm=0, feat=None, arg=True):
    from gnf_hip import abi
    feat = torch.zeros(B * R, FEAT[gi], device=DEV) if feat is None else feat
    arg = torch.zeros(B * R, FEAT[gi], dtype=torch.uint8, device=DEV) if arg is True else arg
    abi.call("gnf_lenet_rows_fwd_arg", abi.ptr(x), abi.ptr(P), P.stride(0), abi.rawptr(rows) if rows is not None else None, R,
             *geo_args(gi), *(abi.ptr(w) for w in W), abi.ptr(feat), abi.rawptr(arg) if arg is not None else None, vm, B,
             abi.stream())
    return feat, arg


def raw_bwd(x, P, rows, R, W, arg, gf, gi, B, vm=0, gx=True, outs=None):
    """-> [gx (or None), gW1, gb1, gW2, gb2]"""
    from gnf_hip import abi
    gx = torch.full((B, DIMS[gi]), 7., device=DEV) if gx is True else gx
    outs = [torch.full_like(w, 7.) for w in W] if outs is None else outs
    nws = abi.load().gnf_lenet_rows_bwd_ws_bytes(*geo_args(gi), R, B, int(gx is not None))
    ws = torch.empty(max(nws // 4, 1), device=DEV)
    abi.call("gnf_lenet_rows_bwd", abi.ptr(x), abi.ptr(P), P.stride(0), abi.rawptr(rows) if rows is not None else None, R,
             *geo_args(gi), *(abi.ptr(w) for w in W), abi.rawptr(arg) if arg is not None else None, abi.ptr(gf), vm,
             abi.ptr(gx), *(abi.ptr(o) for o in outs), abi.rawptr(ws), nws, B, abi.stream())
    return [gx] + outs


# ------------------------------------------------------------------------------------------- 5. pitch, alignment, NULL planes
@pytest.mark.parametrize("gi", [3, 2], ids=["d64", "d256"])
def test_pitched_importance_dword_aligned_operands_and_null_planes(gi):
    """P as the [:, :d] view of a [d, d + 4] matrix; every fp32 operand 4 k bytes past a 16-byte boundary between guard
    bands; argmax2 = NULL (conv2 recomputed); gx = NULL; the [R, B] layout: the bits of the aligned, contiguous call"""
    d, B, R = DIMS[gi], 3, 5
    gen = torch.Generator().manual_seed(5500 + gi)
    W = conv_params(gi, 550 + gi)
    x = cu(torch.randn(B, d, generator=gen))
    wide = cu(torch.rand(d, d + 4, generator=gen))
    Pv = wide[:, :d]
    assert Pv.stride(0) == d + 4
    rows = torch.tensor(row_sets(d)["five"], dtype=torch.int32, device=DEV)
    gf = cu(torch.randn(B * R, FEAT[gi], generator=gen))
    feat0, arg0 = raw_fwd(x, Pv.contiguous(), rows, R, W, gi, B)
    plain, _ = raw_fwd(x, Pv.contiguous(), rows, R, W, gi, B, arg=None)
    assert float(feat0.abs().max()) > 0 and int(arg0.max()) <= 4 and torch.equal(plain, feat0)
    res0 = raw_bwd(x, Pv.contiguous(), rows, R, W, arg0, gf, gi, B)
    assert all(float(t.abs().max()) > 0 and bool(torch.isfinite(t).all()) for t in res0)

    def same(res, what, skip_gx=False):
        for a, b in list(zip(res, res0))[1 if skip_gx else 0:]:
            assert torch.equal(a, b), what
    feat1, arg1 = raw_fwd(x, Pv, rows, R, W, gi, B)
    assert torch.equal(feat1, feat0) and torch.equal(arg1, arg0)
    same(raw_bwd(x, Pv, rows, R, W, arg0, gf, gi, B), "pitched P")
    same(raw_bwd(x, Pv, rows, R, W, None, gf, gi, B), "argmax2 = NULL")
    no_gx = raw_bwd(x, Pv, rows, R, W, arg0, gf, gi, B, gx=None)
    assert no_gx[0] is None
    same(no_gx, "gx = NULL", skip_gx=True)
    same(raw_bwd(x, Pv, rows, R, W, None, gf, gi, B, gx=None), "argmax2 = NULL, gx = NULL", skip_gx=True)
    # [R, B] layout: the same images, the feature rows in another order
    gf_vm = gf.view(B, R, -1).permute(1, 0, 2).contiguous().view(B * R, -1)
    feat_vm, arg_vm = raw_fwd(x, Pv, rows, R, W, gi, B, vm=1)
    assert torch.equal(feat_vm.view(R, B, -1), feat0.view(B, R, -1).permute(1, 0, 2))
    assert torch.equal(arg_vm.view(R, B, -1), arg0.view(B, R, -1).permute(1, 0, 2))
    same(raw_bwd(x, Pv, rows, R, W, arg_vm, gf_vm, gi, B, vm=1), "variable-major")
    for k in (1, 2, 3):
        xm, Pm, gfm = misaligned.place(x, k), misaligned.place(Pv, k), misaligned.place(gf, k)
        Wm = [misaligned.place(w, k) for w in W]
        assert Pm.stride(0) == d + 4
        featm = misaligned.place(torch.zeros_like(feat0), k)
        _, argm = raw_fwd(xm, Pm, rows, R, Wm, gi, B, feat=featm)
        assert torch.equal(featm, feat0) and torch.equal(argm, arg0)
        outs = [misaligned.place(torch.zeros_like(w), k) for w in W]
        gxm = misaligned.place(torch.zeros_like(x), k)
        same(raw_bwd(xm, Pm, rows, R, Wm, argm, gfm, gi, B, gx=gxm, outs=outs), "misaligned by %d floats" % k)
        for t in [xm, Pm, gfm, featm, gxm] + Wm + outs:
            assert misaligned.guards_intact(t)


# ------------------------------------------------------------------------------------------- 6. empty calls, argument errors
def test_empty_calls_and_argument_errors():
    from gnf_hip import abi
    lib = abi.load()
    gi, d, B, R = 2, 256, 2, 5
    W = conv_params(gi, 560)
    x, P = cu(torch.randn(B, d)), cu(torch.rand(d, d))
    rows = torch.tensor(row_sets(d)["five"], dtype=torch.int32, device=DEV)
    gf = cu(torch.randn(B * R, FEAT[gi]))
    # B = 0 or R = 0: zero parameter gradients over a pre-filled buffer, zero gx
    for B_, R_ in ((0, R), (B, 0), (0, 0)):
        res = raw_bwd(x[:B_], P, rows[:R_], R_, W, None, gf[:B_ * R_], gi, B_)
        torch.cuda.synchronize()
        assert all(float(o.abs().max()) == 0. for o in res[1:]), (B_, R_)
        assert res[0].shape == (B_, d) and (B_ == 0 or float(res[0].abs().max()) == 0.)
    res = raw_bwd(None, P, None, 0, W, None, None, gi, B, gx=None)                  # x and g_feat may be NULL then
    assert all(float(o.abs().max()) == 0. for o in res[1:])
    feat = torch.full((B * R, FEAT[gi]), 7., device=DEV)
    raw_fwd(x, P, rows, 0, W, gi, B, feat=feat)
    raw_fwd(x, P, rows, R, W, gi, 0, feat=feat)
    torch.cuda.synchronize()
    assert bool((feat == 7.).all())
    # return codes
    p, s = abi.ptr, abi.stream()
    grads = [torch.empty_like(w) for w in W]
    gx = torch.empty(B, d, device=DEV)
    need = lib.gnf_lenet_rows_bwd_ws_bytes(1, 16, 16, 3, R, B, 1)
    assert need > lib.gnf_lenet_rows_bwd_ws_bytes(1, 16, 16, 3, R, B, 0) > 0
    ws = torch.empty(need // 4, device=DEV)

    def bwd(C=1, H=16, Wd=16, k=3, x_=x, P_=P, ld=d, rows_=rows, R_=R, W1=W[0], gf_=gf, gx_=gx, gW1=grads[0], ws_=ws,
            ws_bytes=need, B_=B):
        return lib.gnf_lenet_rows_bwd(p(x_), p(P_), ld, abi.rawptr(rows_) if rows_ is not None else None, R_, C, H, Wd, k,
                                      p(W1), p(W[1]), p(W[2]), p(W[3]), None, p(gf_), 0, p(gx_), p(gW1), p(grads[1]),
                                      p(grads[2]), p(grads[3]), abi.rawptr(ws_) if ws_ is not None else None, ws_bytes, B_, s)

    def fwd(C=1, H=16, Wd=16, k=3, x_=x, P_=P, ld=d, rows_=rows, R_=R, feat_=feat):
        return lib.gnf_lenet_rows_fwd_arg(p(x_), p(P_), ld, abi.rawptr(rows_) if rows_ is not None else None, R_, C, H, Wd, k,
                                          p(W[0]), p(W[1]), p(W[2]), p(W[3]), p(feat_), None, 0, B, s)
    assert bwd() == 0 and bwd(gx_=None) == 0 and fwd() == 0
    for bad in ((3, 28, 28, 5), (1, 32, 32, 4)):
        assert bwd(*bad) == -2 and fwd(*bad) == -2 and lib.gnf_lenet_rows_bwd_ws_bytes(*bad, R, B, 1) == -2   # GNF_ESHAPE
    for kw in ({"x_": None}, {"P_": None}, {"W1": None}, {"gf_": None}, {"gW1": None}, {"ws_": None}, {"ld": d - 1},
               {"rows_": None, "R_": d + 1}, {"B_": -1}, {"R_": -1}):
        assert bwd(**kw) == -1, kw                                                                           # GNF_EINVAL
    for kw in ({"x_": None}, {"P_": None}, {"feat_": None}, {"ld": d - 1}, {"rows_": None, "R_": d + 1}):
        assert fwd(**kw) == -1, kw
    assert bwd(ws_bytes=need - 4) == -3                                                                      # GNF_EWS
    assert bwd(gx_=None, ws_bytes=lib.gnf_lenet_rows_bwd_ws_bytes(1, 16, 16, 3, R, B, 0)) == 0
    assert lib.gnf_lenet_rows_bwd_ws_bytes(1, 16, 16, 3, -1, B, 1) == -1
    byte_off = ctypes.c_void_p(x.data_ptr() + 2)                                                             # below dword alignment
    assert lib.gnf_lenet_rows_bwd(byte_off, p(P), d, abi.rawptr(rows), R, 1, 16, 16, 3, p(W[0]), p(W[1]), p(W[2]), p(W[3]),
                                  None, p(gf), 0, p(gx), p(grads[0]), p(grads[1]), p(grads[2]), p(grads[3]),
                                  abi.rawptr(ws), need, B, s) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 7. the C ABI
def test_symbols_declared_and_bound():
    from gnf_hip import abi
    header = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    for name in ("gnf_lenet_rows_fwd_arg", "gnf_lenet_rows_bwd_ws_bytes", "gnf_lenet_rows_bwd"):
        assert name + "(" in header and name in abi.SIGNATURES
        assert hasattr(abi.load(), name)
    assert abi.ABI_VERSION == 11 and abi.load().gnf_abi_version() == 11


# ------------------------------------------------------------------------------------------- 8. memory
def test_peak_memory_below_one_copy_of_the_product():
    """(3,32,32,5), B = 2, A frozen, forward + backward of the conditioner with x.requires_grad: with the rows front the peak
    above the level before the call stays below B d d 4 bytes -- ONE copy of the product, 75.5 MB; the composed path holds
    e (and its cotangent), so its peak is at least that, which checks the measuring method"""
    gi, B, d = 0, 2, 3072
    gen = torch.Generator().manual_seed(5800)
    cond = make_conditioner(gi, importance("01", d, gen))
    x, cot = cu(torch.randn(B, d, generator=gen)), cu(torch.randn(B, d, 2, generator=gen))
    product, peak = B * d * d * 4, {}
    for on in (True, False):
        cond.embedding_net.rows_train_front = on
        cond.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        (cond(xd) * cot).sum().backward()
        torch.cuda.synchronize()
        peak[on] = torch.cuda.max_memory_allocated() - base
        assert xd.grad is not None and bool(torch.isfinite(xd.grad).all())
        del xd
    print("peak bytes above the operands: rows front %d, composed %d; the product: %d" % (peak[True], peak[False], product))
    assert peak[True] < product, (peak, product)
    assert peak[False] >= product, (peak, product)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- 9. end to end
def freeze_to_dag(flow, seed):
    """every conditioner's A <- a fixed 0/1 DAG, frozen (tests/test_gpu_lenet_rows.py::frozen_dag_flow): a random order of the
    variables, a chain through its first 8, about 2 random earlier parents per variable"""
    for n, cond in enumerate(flow.getConditioners()):
        d = cond.in_size
        gen = torch.Generator().manual_seed(seed + n)
        order = torch.randperm(d, generator=gen)
        A = torch.zeros(d, d)
        A[order[1:8], order[0:7]] = 1.
        for t in range(1, d):
            A[order[t], order[torch.randint(0, t, (2,), generator=gen)]] = 1.
        cond.stoch_gate = cond.noise_gate = cond.s_thresh = False
        cond.h_thresh = 0.
        with torch.no_grad():
            cond.A.copy_(A.to(cond.A.device))
        cond.A.requires_grad = False
        cond.invalidate_caches()
        cond.is_invertible = True


def set_switch(flow, on):
    for cond in flow.getConditioners():
        cond.embedding_net.rows_train_front = on


def step_of(flow, x, on):
    set_switch(flow, on)
    flow.zero_grad(set_to_none=True)
    z, ld = flow(x)
    loss = flow.loss(z, ld)
    nodes = graph_nodes(loss)
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in flow.named_parameters() if p.grad is not None}, nodes


@pytest.mark.parametrize("inner", [[2], [1, 1, 1, 1]], ids=["one-scale-two-steps", "four-scales"])
def test_training_step_of_the_frozen_cifar_flows(inner):
    """B = 2; two steps at d = 3072 (the second step's x needs a gradient) and the multi-scale flow (every scale but the
    first gets an x that needs one): loss and every parameter gradient with the rows front against the composed path"""
    from models import AffineNormalizer
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow
    torch.manual_seed(590 + len(inner))
    flow = buildCIFAR10NormalizingFlow(inner, AffineNormalizer, {}).to(DEV)
    freeze_to_dag(flow, 5900)
    x = cu(torch.randn(2, 3072, generator=torch.Generator().manual_seed(5901)))
    loss0, g0, nodes0 = step_of(flow, x, False)
    loss1, g1, nodes1 = step_of(flow, x, True)
    assert "LenetRowsFnBackward" in nodes1 and not (nodes1 & COMPOSED)
    assert "LenetRowsFnBackward" not in nodes0 and COMPOSED <= nodes0
    assert bool(torch.isfinite(loss0))
    assert_fwd(loss1, loss0, what="loss")
    # (the factory's fourth scale never runs -- three dropping factors -- and receives no gradient on either path)
    reached = [n for n, p in flow.named_parameters() if p.requires_grad and not n.startswith("steps.3.")]
    assert set(g1) == set(g0) == set(reached) and len(reached) >= 10 and all(not n.endswith(".A") for n in reached)
    for n in reached:
        assert_grad(g1[n], g0[n], n)


def test_graphed_training_steps_of_the_frozen_flow():
    """dp.GraphedStep.graphable() accepts the frozen one-scale flow (it refuses stochastic gates only, with or without this
    front), so it must still accept it with the rows front, and three replayed steps must match three eager steps: the loss
    at the forward tolerance, the parameters at the gradient tolerance"""
    from gnf_hip import dp
    from models import AffineNormalizer
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow

    def make():
        torch.manual_seed(595)
        flow = buildCIFAR10NormalizingFlow([1], AffineNormalizer, {}).to(DEV)
        freeze_to_dag(flow, 5950)
        set_switch(flow, True)
        return flow
    xs = [cu(torch.randn(2, 3072, generator=torch.Generator().manual_seed(5960 + i))) for i in range(4)]
    fa = make()
    assert dp.GraphedStep.graphable(fa)
    sa = dp.FlatState(fa)
    for x in [xs[0]] + xs[1:]:                                  # the warm-up step of GraphedStep, then three more
        la = dp.train_step(fa, sa, x, lr=1e-3, graph=False)
    fb = make()
    sb = dp.FlatState(fb)
    gs = dp.GraphedStep(fb, sb, xs[0], lr=1e-3, warmup=1)
    for x in xs[1:]:
        lb = gs(x)
    torch.cuda.synchronize()
    assert gs.captures == 1 and sb.t == sa.t == 4
    assert_fwd(lb, la.detach(), what="loss of the third replayed step")
    assert_grad(sb.flat, sa.flat, "parameters after three replayed steps")
