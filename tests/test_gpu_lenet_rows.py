"""GPU: the row-subset LeNet front of CIFAR10CNN for a deterministic DAG gate (gnf_lenet_rows_fwd, gnf_hip.ops.lenet_rows,
CIFAR10CNN.forward_rows, `rows_front`): the masked copies x[b] * P[rows[r]] of a level of the inversion, or of all d rows,
are built in LDS; the [B, R, d] tensor of the broadcast product does not exist.

The yardstick of the features is gnf_hip.ops.lenet_conv on that product (tests/test_gpu_lenet.py holds it to the fp64
oracle): a copy is ONE fp32 product on both sides, so the features must agree BIT FOR BIT.  Through the conditioner the two
settings of `rows_front` differ in the fc chain's row order only; they are compared at the forward tolerance of
tests/conftest.py (assert_fwd), and one test goes to the fp64 restatement directly."""
import ctypes
import os

import pytest
import torch

from conftest import assert_fwd, rel_err
import lenet_ref
from lenet_ref import DEV, cu, geo_args
import misaligned

pytestmark = pytest.mark.gpu
GEOS = lenet_ref.GEOMETRIES
FEAT = (400, 576, 64, 16)
DIMS = tuple(s[0] * s[1] * s[2] for s, _, _ in GEOS)          # 3072, 1024, 256, 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# each geometry at B = 1 and at one more B: 30 and 7 leave the last group of IPB = 28 / 5 samples partial; IPB = 1 at d = 1024, 3072
BATCHES = {3: (1, 30), 2: (1, 7), 1: (1, 2), 0: (1, 2)}


def conv_params(gi, seed):
    size_img, k, _ = GEOS[gi]
    torch.manual_seed(seed)
    c1, c2 = torch.nn.Conv2d(size_img[0], 6, k), torch.nn.Conv2d(6, 16, k)
    return [cu(t.detach().clone()) for t in (c1.weight, c1.bias, c2.weight, c2.bias)]


def row_sets(d):
    """one row; five unsorted rows with one duplicate; None = all d rows in order"""
    return {"one": [d // 3], "five": [d - 1, 2, d // 2, 2, 5], "all": None}


def importance(kind, d, gen):
    if kind == "A":
        return 1.5 + .02 * torch.randn(d, d, generator=gen)
    P = torch.zeros(d, d)                                       # 0/1, about 3 ones per row
    P[torch.arange(d).repeat_interleave(3), torch.randint(0, d, (3 * d,), generator=gen)] = 1.
    return P


def rows_tensor(rows):
    return None if rows is None else torch.tensor(rows, dtype=torch.int32, device=DEV)


def composed(x, P, rows, W, gi, variable_major):
    """the parent's statements: the broadcast product in memory, then the conv front on its B*R rows"""
    from gnf_hip import ops
    B, d = x.shape
    Pr = P if rows is None else P[torch.tensor(rows, device=DEV)]
    e = (x[:, None, :] * Pr[None]).reshape(B * Pr.shape[0], d)
    ref = ops.lenet_conv(e, *W, GEOS[gi][0], GEOS[gi][1]).view(B, Pr.shape[0], -1)
    return ref.permute(1, 0, 2) if variable_major else ref


# ------------------------------------------------------------------------------------------- 1. feature bits
BIT_CASES = [(gi, B, rs, kind) for gi in (3, 2, 1, 0) for B in BATCHES[gi] for rs in ("one", "five", "all")
             for kind in ("A", "01")]


@pytest.mark.parametrize("gi,B,rs,kind", BIT_CASES, ids=["d%d-B%d-%s-P%s" % (DIMS[c[0]], c[1], c[2], c[3]) for c in BIT_CASES])
def test_feature_bits_equal_the_conv_front_on_the_product(gi, B, rs, kind):
    from gnf_hip import ops
    d = DIMS[gi]
    gen = torch.Generator().manual_seed(100 * gi + B)
    W = conv_params(gi, 300 + gi)
    x, P = cu(torch.randn(B, d, generator=gen)), cu(importance(kind, d, gen))
    rows = row_sets(d)[rs]
    R = d if rows is None else len(rows)
    with torch.no_grad():
        for vm in (False, True):
            got = ops.lenet_rows(x, P, rows_tensor(rows), *W, GEOS[gi][0], GEOS[gi][1], vm)
            ref = composed(x, P, rows, W, gi, vm)
            assert got.shape == ((R, B, FEAT[gi]) if vm else (B, R, FEAT[gi])) and got.is_contiguous()
            assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
            assert torch.equal(got, ref), (vm, rel_err(got.cpu(), ref.cpu()))


def test_operands_that_require_grad_are_refused():
    from gnf_hip import abi, ops
    gi, d = 3, 64
    W = conv_params(gi, 1)
    x, P = cu(torch.randn(2, d)), cu(torch.rand(d, d))
    W[0].requires_grad_(True)
    with pytest.raises(abi.GnfError):
        ops.lenet_rows(x, P, None, *W, GEOS[gi][0], GEOS[gi][1], False)
    with torch.no_grad():
        assert ops.lenet_rows(x, P, None, *W, GEOS[gi][0], GEOS[gi][1], False).shape == (2, d, FEAT[gi])


# ------------------------------------------------------------------------------------------- 2. pitch and alignment
def raw_rows(x, P, rows, R, W, gi, B, feat, variable_major=0):
    from gnf_hip import abi
    abi.call("gnf_lenet_rows_fwd", abi.ptr(x), abi.ptr(P), P.stride(0), abi.rawptr(rows) if rows is not None else None, R,
             *geo_args(gi), *(abi.ptr(w) for w in W), abi.ptr(feat), variable_major, B, abi.stream())
    return feat


@pytest.mark.parametrize("gi", [3, 2], ids=["d64", "d256"])
def test_pitched_importance_and_dword_aligned_operands(gi):
    """P as the [:, :d] view of a [d, d + 4] matrix, then every fp32 operand 4 k bytes past a 16-byte boundary between
    guard bands: the bits of the aligned, contiguous call"""
    d, B = DIMS[gi], 3
    gen = torch.Generator().manual_seed(510 + gi)
    W = conv_params(gi, 500 + gi)
    x = cu(torch.randn(B, d, generator=gen))
    wide = cu(1.5 + .02 * torch.randn(d, d + 4, generator=gen))
    Pv = wide[:, :d]
    assert Pv.stride(0) == d + 4
    rows = rows_tensor(row_sets(d)["five"])
    for vm in (0, 1):
        feat0 = raw_rows(x, Pv.contiguous(), rows, 5, W, gi, B, torch.zeros(B * 5, FEAT[gi], device=DEV), vm)
        assert float(feat0.abs().max()) > 0
        feat1 = raw_rows(x, Pv, rows, 5, W, gi, B, torch.zeros(B * 5, FEAT[gi], device=DEV), vm)
        assert torch.equal(feat1, feat0)
        for k in (1, 2, 3):
            xm, Pm, Wm = misaligned.place(x, k), misaligned.place(Pv, k), [misaligned.place(w, k) for w in W]
            assert Pm.stride(0) == d + 4
            featm = raw_rows(xm, Pm, rows, 5, Wm, gi, B, misaligned.place(torch.zeros_like(feat0), k), vm)
            assert torch.equal(featm, feat0), (vm, k)
            for t in [xm, Pm, featm] + Wm:
                assert misaligned.guards_intact(t)


# ------------------------------------------------------------------------------------------- conditioners
def make_conditioner(gi, seed=70):
    from models import DAGConditioner
    from models.MLP import CIFAR10CNN
    size_img, k, fc_l = GEOS[gi]
    torch.manual_seed(seed + gi)
    net = CIFAR10CNN(out_d=2, fc_l=list(fc_l), size_img=list(size_img), k_size=k)
    cond = DAGConditioner(DIMS[gi], net, 2)
    cond.stoch_gate = False                                    # deterministic gate on the soft-thresholded A
    return cond.to(DEV)


def rows_of(cond, x, rows, P, on, variable_major=False, **kw):
    cond.embedding_net.rows_front = on
    return cond.forward_rows(x, torch.tensor(rows, device=DEV), P, tuple(rows), variable_major=variable_major, **kw)


# ------------------------------------------------------------------------------------------- 3. fp64
def test_conditioner_rows_against_fp64():
    """d = 256, B = 7, 9 rows through DAGConditioner.forward_rows with the row-subset front against the fp64 restatement of
    CIFAR10CNN on the same masked copies"""
    gi, B = 2, 7
    d, size_img = DIMS[gi], GEOS[gi][0]
    cond = make_conditioner(gi)
    gen = torch.Generator().manual_seed(3300)
    x = torch.randn(B, d, generator=gen)
    rows = [int(r) for r in torch.randperm(d, generator=gen)[:9]]
    with torch.no_grad():
        P = cond.deterministic_importance()
        h = rows_of(cond, cu(x), rows, P, True)
        e = (x[:, None, :] * P.cpu()[rows][None]).reshape(B * 9, d)                 # the same fp32 products
        p64 = {n: q.detach().cpu().double() for n, q in cond.embedding_net.named_parameters()}
        h0 = lenet_ref.cifar10cnn(e.double(), p64, size_img).view(B, 9, 2)
    assert h.shape == (B, 9, 2)
    assert_fwd(h, h0, what="h")


# ------------------------------------------------------------------------------------------- 4. conditioner parity
@pytest.mark.parametrize("gi", [3, 2, 1, 0], ids=["d64", "d256", "d1024", "d3072"])
def test_forward_rows_parity_with_the_broadcast_product(gi):
    d, B = DIMS[gi], BATCHES[gi][1]
    cond = make_conditioner(gi)
    gen = torch.Generator().manual_seed(4400 + gi)
    x = cu(torch.randn(B, d, generator=gen))
    rows = [int(r) for r in torch.randperm(d, generator=gen)[:9]] + [3, 3]
    R = len(rows)
    with torch.no_grad():
        for P in (cond.A, cond.soft_thresholded_A()):
            for vm in (False, True):
                off, on = rows_of(cond, x, rows, P, False, vm), rows_of(cond, x, rows, P, True, vm)
                assert on.shape == off.shape == ((R, B, 2) if vm else (B, R, 2))
                assert_fwd(on, off, what="h")
        cached = rows_of(cond, x, rows, P, True, True, rows32=torch.tensor(rows, dtype=torch.int32, device=DEV))
        assert torch.equal(cached, on)                         # the caller's int32 table or the conversion: the same call
    # autograd on, trainable weights: the statements of the parent run under either setting
    with torch.enable_grad():
        assert cond.embedding_net.conv1.weight.requires_grad
        off, on = rows_of(cond, x, rows, cond.A.detach(), False), rows_of(cond, x, rows, cond.A.detach(), True)
        assert on.requires_grad and off.requires_grad and torch.equal(on, off)


def test_hot_encoding_takes_the_broadcast_product():
    gi, B = 2, 3
    d = DIMS[gi]
    cond = make_conditioner(gi)
    net = cond.embedding_net
    cond.hot_encoding = True
    seen = []

    def no_rows(*a, **k):
        raise AssertionError("the row-subset front has no one-hot columns")

    def record(e, context=None):
        seen.append(tuple(e.shape))
        return e[:, :2].clone()
    net.forward_rows, net.forward, net.rows_front = no_rows, record, True
    with torch.no_grad():
        x = cu(torch.randn(B, d))
        h = cond.forward_rows(x, torch.tensor([4, 9, 1], device=DEV), cond.A, (4, 9, 1))
        assert seen == [(B * 3, 2 * d)] and h.shape == (B, 3, 2)
        assert torch.equal(h[:, :, 0], x[:, :1] * cond.A[torch.tensor([4, 9, 1], device=DEV), 0][None])


# ------------------------------------------------------------------------------------------- 5. deterministic forward
def test_deterministic_forward_and_untouched_gumbel_gate():
    gi, B = 2, 7
    d = DIMS[gi]
    cond = make_conditioner(gi)
    net = cond.embedding_net
    x = cu(torch.randn(B, d, generator=torch.Generator().manual_seed(5500)))

    def run(on):
        net.rows_front = on
        cond.gate_seed, cond._gate_calls = 1234567, 40
        return cond(x)
    with torch.no_grad():
        off, on = run(False), run(True)
        assert on.shape == off.shape == (B, d, 2)
        assert_fwd(on, off, what="h")
        cond.stoch_gate = True                                 # Gumbel gate: the path is not taken, the same Philox stream
        off, on = run(False), run(True)
        assert torch.equal(on, off)
    cond.stoch_gate = False
    with torch.enable_grad():                                  # autograd on: the parent's nodes
        off, on = run(False), run(True)
        assert on.requires_grad and torch.equal(on, off)


# ------------------------------------------------------------------------------------------- 6. inversion
def frozen_dag_flow(gi, seed):
    """one Affine step on a CIFAR10CNN conditioner whose A is frozen to a 0/1 DAG: a random order of the variables, a chain
    through its first 8 (more than 4 levels), and about 2 random earlier parents per variable"""
    from models import AffineNormalizer
    from models.NormalizingFlow import FCNormalizingFlow, NormalizingFlowStep
    from models.NormalizingFlowFactories import NormalLogDensity
    d = DIMS[gi]
    cond = make_conditioner(gi, seed)
    gen = torch.Generator().manual_seed(seed)
    order = torch.randperm(d, generator=gen)
    A = torch.zeros(d, d)
    A[order[1:8], order[0:7]] = 1.
    for t in range(1, d):
        A[order[t], order[torch.randint(0, t, (2,), generator=gen)]] = 1.
    cond.stoch_gate = cond.noise_gate = cond.s_thresh = False
    cond.h_thresh = 0.
    with torch.no_grad():
        cond.A.copy_(cu(A))
    cond.A.requires_grad = False
    cond.invalidate_caches()
    cond.is_invertible = True
    flow = FCNormalizingFlow([NormalizingFlowStep(cond, AffineNormalizer())], NormalLogDensity()).to(DEV)
    assert len(cond.levels()) > 4
    return flow, cond


@pytest.mark.parametrize("gi,B,graphed", [(2, 7, True), (0, 2, False)], ids=["d256-graphed", "d3072-eager"])
def test_inversion_on_the_row_subset_front(gi, B, graphed):
    flow, cond = frozen_dag_flow(gi, 6600 + gi)
    net = cond.embedding_net
    flow.steps[0].graph_invert = graphed
    z = cu(torch.randn(B, DIMS[gi], generator=torch.Generator().manual_seed(6601)))
    net.rows_front = False
    x_off = flow.invert(z)
    net.rows_front = True
    xs = [flow.invert(z) for _ in range(3 if graphed else 1)]          # eager warm-up, capture, replay
    torch.cuda.synchronize()
    if graphed:
        from models.NormalizingFlow import _INV_GRAPHS
        assert any(isinstance(v, tuple) for v in _INV_GRAPHS[flow.steps[0]].values())     # the pass was captured
    for x_on in xs[1:]:
        assert torch.equal(x_on, xs[0])
    x_on = xs[-1]
    assert bool(torch.isfinite(x_on).all())
    e_off = rel_err(x_on.cpu(), x_off.cpu())
    with torch.no_grad():
        e_rt = rel_err(flow(x_on)[0].cpu(), z.cpu())
    print("inversion d = %d: rel_err(x_on, x_off) = %.3g, rel_err(flow(x_on), z) = %.3g" % (DIMS[gi], e_off, e_rt))
    assert e_off < 1e-4 and e_rt < 1e-4


# ------------------------------------------------------------------------------------------- 7. memory
def test_peak_memory_without_the_broadcast_product():
    """d = 3072, B = 4, all d rows under no_grad: the peak above the level before the call stays below half of the
    [B, d, d] product alone (151 MB); the features and the fc activations are about 30 MB"""
    gi, B, d = 0, 4, 3072
    cond = make_conditioner(gi)
    cond.embedding_net.rows_front = True
    x = cu(torch.randn(B, d, generator=torch.Generator().manual_seed(7700)))
    rows = torch.arange(d, device=DEV)
    host_rows, rows32 = tuple(range(d)), rows.to(torch.int32)
    with torch.no_grad():
        P = cond.deterministic_importance()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        h = cond.forward_rows(x, rows, P, host_rows, rows32=rows32)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    product = B * d * d * 4
    print("peak bytes above the operands: %d; the [B, d, d] product: %d bytes" % (peak, product))
    assert h.shape == (B, d, 2) and bool(torch.isfinite(h).all())
    assert peak < .5 * product, (peak, product)
    del h, P
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- 8. the C ABI
def test_symbol_declared_and_bound():
    from gnf_hip import abi
    header = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    assert "gnf_lenet_rows_fwd(" in header and "gnf_lenet_rows_fwd" in abi.SIGNATURES
    assert hasattr(abi.load(), "gnf_lenet_rows_fwd")


def test_empty_calls_and_argument_errors():
    from gnf_hip import abi
    lib = abi.load()
    gi, d, B, R = 2, 256, 2, 5
    W = conv_params(gi, 800)
    x, P = cu(torch.randn(B, d)), cu(torch.rand(d, d))
    rows = rows_tensor(row_sets(d)["five"])
    feat = torch.full((B * R, FEAT[gi]), 7., device=DEV)
    p, s = abi.ptr, abi.stream()

    def fwd(C=1, H=16, Wd=16, k=3, x_=x, P_=P, ld=d, rows_=rows, R_=R, W1=W[0], b1=W[1], W2=W[2], b2=W[3], feat_=feat, B_=B):
        return lib.gnf_lenet_rows_fwd(p(x_), p(P_), ld, abi.rawptr(rows_) if rows_ is not None else None, R_, C, H, Wd, k,
                                      p(W1), p(b1), p(W2), p(b2), p(feat_), 0, B_, s)
    # B = 0, R = 0: nothing is launched
    assert fwd(B_=0) == 0 and fwd(R_=0) == 0 and fwd(B_=0, x_=None, feat_=None) == 0
    torch.cuda.synchronize()
    assert bool((feat == 7.).all())
    assert fwd(3, 28, 28, 5) == -2 and fwd(1, 32, 32, 4) == -2                                  # GNF_ESHAPE
    for kw in ({"x_": None}, {"P_": None}, {"W1": None}, {"b1": None}, {"W2": None}, {"b2": None}, {"feat_": None},
               {"ld": d - 1}, {"rows_": None, "R_": d + 1}, {"B_": -1}, {"R_": -1}):
        assert fwd(**kw) == -1, kw                                                              # GNF_EINVAL
    byte_off = ctypes.c_void_p(x.data_ptr() + 2)                                                # below dword alignment
    assert lib.gnf_lenet_rows_fwd(byte_off, p(P), d, abi.rawptr(rows), R, 1, 16, 16, 3, p(W[0]), p(W[1]), p(W[2]), p(W[3]),
                                  p(feat), 0, B, s) == -1
    assert lib.gnf_lenet_rows_fwd(p(x), p(P), d, ctypes.c_void_p(rows.data_ptr() + 2), R, 1, 16, 16, 3, p(W[0]), p(W[1]),
                                  p(W[2]), p(W[3]), p(feat), 0, B, s) == -1
    torch.cuda.synchronize()
    assert bool((feat == 7.).all())                            # no refused call wrote anything
    assert fwd() == 0 and fwd(rows_=None, R_=R) == 0           # rows == NULL: rows 0 .. R - 1
    torch.cuda.synchronize()
    assert bool(torch.isfinite(feat).all()) and not bool((feat == 7.).all())
