"""The Spline kernels (csrc/gnf_spline.hip, ops.SplineFn / ops.spline_inverse) on long rows and on every staging route,
against tests/spline_ref.py in fp64: the table of tests/spline_cases.py, whose routes tests/test_spline_routes_host.py
asserts through gnf_spline_route.  The sibling of tests/test_gpu_spline.py, with that file's yardstick unchanged: the
reference in fp64 on the same fp32 inputs is the truth, the reference in fp32 on the CPU the comparator, and the kernel's
largest error at most 2 err_comparator + 1e-6 max|truth| per output tensor (its _rule / _judge, TRUTH_FLOOR included).  Set
GNF_SPLINE_PROFILE=<file> to have the worst measured ratio of every group of this file appended there."""
import os

import pytest
import torch

import misaligned
import poison
import spline_cases as SC
import spline_ref as S
import test_gpu_spline as G
from test_gpu_spline import cu, c64, _judge, _rule, _draw, _specials, _layout, COTANGENTS

pytestmark = pytest.mark.gpu
DEV = G.DEV
T = SC.T
PRE = "long rows, "                          # the groups of this file in G._RATIOS


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GNF_SPLINE_PROFILE")
    mine = {g: rows for g, rows in G._RATIOS.items() if g.startswith(PRE)}
    if path and mine:
        ratio = lambda r: r[1] / max(2. * r[2] + 1e-6 * r[3], 1e-300)
        with open(path, "a") as f:
            for group, rows in mine.items():
                worst = max(rows, key=ratio)
                f.write("%s (tests/test_gpu_spline_long.py), %d cases\n" % (group, len(rows)))
                f.write("worst err / (2 err_comparator + 1e-6 scale) = %.4f at %s: err %.3e, err_comparator %.3e, scale %.3e\n"
                        % (ratio(worst), worst[0], worst[1], worst[2], worst[3]))


class Placed:
    """the fp32 [B, d, C] conditioner output `h` (CPU) in a layout of spline_cases.LAYOUTS on the device.  The allocation
    behind a view that does not cover it is filled with the sentinel bits first; intact() says that not one bit of it
    outside the view has changed since, and that the view still holds h"""

    def __init__(self, h, layout):
        B, d, C = h.shape
        self.h = h
        if layout in SC.OLD_LAYOUTS:
            self.big = self.mark = None
            self.view = _layout(h, layout)
            self.before = self.view.clone()
            return
        shape, view = SC.geometry(layout, B, d, C)
        self.big = torch.empty(shape, device=DEV)
        self.big.view(torch.int32).fill_(misaligned.SENTINEL)
        self.mark = torch.zeros(shape, dtype=torch.bool, device=DEV)
        view(self.mark)[...] = True
        self.view = view(self.big)
        self.view.copy_(cu(h))
        self.before = self.view.clone()

    def intact(self):
        torch.cuda.synchronize()
        if poison.differing(self.view, self.before) != 0:
            return False
        return self.big is None or bool((self.big.view(torch.int32)[~self.mark] == misaligned.SENTINEL).all())


def _plant(x, h, K):
    """the specials of _specials (x = T, -T, 0, a knot, +inf, -inf, NaN; the knot that of the element it lands on) at the
    front, in the first lanes of a middle chunk of row 0, in the last chunk of the last row and over the last elements"""
    B, d = x.shape
    C = h.shape[-1]
    flat, hf = x.view(-1), h.reshape(-1, C)
    nchunk = -(-d // SC.KTILE)
    starts = [0, flat.numel() - 7]
    if nchunk >= 3:
        starts.append(nchunk // 2 * SC.KTILE)
    if nchunk >= 2:
        starts.append((B - 1) * d + (nchunk - 1) * SC.KTILE)
    for p in starts:
        sp = _specials(hf[min(p + 3, flat.numel() - 1)][None], K, T)
        n = min(len(sp), flat.numel() - p)
        flat[p:p + n] = torch.tensor(sp[:n])
    return x


# ------------------------------------------------------------------------------------------------------- 1. values
def _values(x, h, K, layout, case):
    from gnf_hip import ops
    P = Placed(h, layout)
    z, jac, logdet, logn = ops.SplineFn.apply(cu(x), P.view, K, T, True, True)
    z64, j64 = S.forward(x.double(), h.double(), K, T)
    z32, j32 = S.forward(x, h, K, T)
    ld64, ln64 = S.logdet_logn(z64, j64)
    ld32, ln32 = S.logdet_logn(z32, j32)
    for name, got, want, cmp in (("z", z, z64, z32), ("jac", jac, j64, j32), ("logdet", logdet, ld64, ld32),
                                 ("logn", logn, ln64, ln32)):
        _judge(PRE + "values: " + name, case, got, want, cmp)
    # the fused step's form: no jac, no density -- the same z and log-determinant, bit for bit
    z2, jac2, ld2, ln2 = ops.SplineFn.apply(cu(x), P.view, K, T, False, False)
    assert jac2.numel() == 0 and ln2.numel() == 0
    assert poison.differing(z2, z) == 0 and poison.differing(ld2, logdet) == 0
    assert P.intact()
    return z, jac


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_values(case):
    B, d, K, layout = case
    x, h = _draw(B, d, K, T, SC.SCALE)
    # the draw as it is: every row's log|det J| and density finite, so that each is judged by the rule ...
    z, jac = _values(x, h, K, layout, SC.case_id(case))
    out = ~((x >= -T) & (x <= T))
    assert 0 < int(out.sum()) < x.numel()
    assert poison.differing(z[cu(out)], cu(x)[cu(out)]) == 0 and bool((jac[cu(out)] == 1.).all())
    # ... and with the specials planted (a NaN or an infinity makes its row's density one)
    x = _plant(x.clone(), h, K)
    z, jac = _values(x, h, K, layout, SC.case_id(case) + "-specials")
    out = ~((x >= -T) & (x <= T))
    assert 0 < int(out.sum()) < x.numel()
    assert poison.differing(z[cu(out)], cu(x)[cu(out)]) == 0 and bool((jac[cu(out)] == 1.).all())


# ------------------------------------------------------------------------------------------------------- 2. inverse
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_inverse_residual(case):
    """the [B, d] problem of the scatter form is B variables of d samples: at the long shapes the level schedule's own
    geometry, few variables and many samples"""
    from gnf_hip import ops
    B, d, K, layout = case
    z, h = _draw(B, d, K, T, SC.SCALE, seed=1)
    P = Placed(h, layout)
    x = ops.spline_inverse(cu(z), P.view, K, T)
    out = ~((z >= -T) & (z <= T))
    assert poison.differing(x[cu(out)], cu(z)[cu(out)]) == 0
    _rule(PRE + "inverse residual in z", SC.case_id(case), G._residual(x, h, z, K, T),
          G._residual(S.inverse(z, h, K, T), h, z, K, T), z.abs().max().item())
    width = B + 3
    cols = torch.randperm(width, generator=torch.Generator().manual_seed(B))[:B].to(torch.int32)
    target = torch.empty(d, width)
    target.view(torch.int32).fill_(misaligned.SENTINEL)
    target = cu(target)
    ops.spline_inverse(cu(z), P.view, K, T, out=target, out_cols=cu(cols))
    assert poison.differing(target[:, cu(cols).long()].t().contiguous(), x) == 0
    rest = torch.ones(width, dtype=torch.bool)
    rest[cols.long()] = False
    assert bool((target[:, cu(rest)].contiguous().view(torch.int32) == misaligned.SENTINEL).all())
    assert P.intact()


# ------------------------------------------------------------------------------------------------------- 3. gradients
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_gradients(case):
    from gnf_hip import ops
    B, d, K, layout = case
    x, h = _draw(B, d, K, T, SC.SCALE, seed=2)
    x = S.to_bin_middles(x, h, K, T)
    assert int((S.knot_distance(x.double(), h.double(), K, T) < 1e-4).sum()) == 0
    g = torch.Generator().manual_seed(7)
    cot = {"z": torch.randn(B, d, generator=g), "jac": torch.randn(B, d, generator=g),
           "logdet": torch.randn(B, generator=g), "logn": torch.randn(B, generator=g)}

    def loss(outs, which, to):
        return sum((outs[n] * to(cot[n])).sum() for n in which)

    def reference(dtype, which):
        xl, hl = x.to(dtype).clone().requires_grad_(True), h.to(dtype).clone().requires_grad_(True)
        z, jac = S.forward(xl, hl, K, T)
        ld, ln = S.logdet_logn(z, jac)
        return torch.autograd.grad(loss({"z": z, "jac": jac, "logdet": ld, "logn": ln}, which, lambda t: t.to(dtype)), (xl, hl))

    C = 3 * K - 1
    P = Placed(h, layout)
    for which in COTANGENTS:
        (gx64, gh64), (gx32, gh32) = reference(torch.float64, which), reference(torch.float32, which)
        for with_gx in (True, False):
            xd = cu(x).requires_grad_(with_gx)
            hd = P.view.detach().requires_grad_(True)
            assert hd.stride() == P.view.stride() and hd.data_ptr() == P.view.data_ptr()
            z, jac, ld, ln = ops.SplineFn.apply(xd, hd, K, T, "jac" in which, "logn" in which)
            loss({"z": z, "jac": jac, "logdet": ld, "logn": ln}, which, cu).backward()
            tag = "%s-%s%s" % (SC.case_id(case), "+".join(which), "" if with_gx else "-nogx")
            if with_gx:
                _judge(PRE + "gradients: gx", tag, xd.grad, gx64, gx32)
            else:
                assert xd.grad is None
            assert hd.grad.shape == hd.shape
            _judge(PRE + "gradients: gh", tag, hd.grad[:, :, :C], gh64, gh32)
            assert bool((hd.grad[:, :, C:] == 0).all())
            assert P.intact()


# ------------------------------------------------------------------------------------------------------- 4. the image path
def _oracle_mnist_spline(sd, x, u1, u2, K, T_):
    """the oracle chain of tests/test_gpu_configs.py::_oracle_cfg4 with spline_ref.forward where O.monotonic_forward stands"""
    from oracle import gnf_oracle as O
    pre = "steps.0.conditioner."
    sd = {k: v.detach().cpu().clone() for k, v in sd.items()}
    cnn = {k[len(pre + "embedding_net."):]: v.requires_grad_(True) for k, v in sd.items() if "embedding_net." in k}
    A = sd[pre + "A"].requires_grad_(True)
    B, d = x.shape
    e = O.dag_masked_inputs(x, A, True, 0., True, False, 1., u1, u2, None, False)
    h = O.mnistcnn_forward(e, cnn).view(B, d, -1)
    z, jac = S.forward(x, h, K, T_)
    closs = O.dag_loss(A, sd[pre + "alpha"], d % 50, sd[pre + "lambd"], sd[pre + "c"], sd[pre + "dag_const"],
                       sd[pre + "l1_weight"])
    ld = torch.log(jac).sum(1)
    loss = O.flow_loss(z, ld, closs)
    loss.backward()
    grads = {pre + "A": A.grad}
    for name, v in cnn.items():
        grads[pre + "embedding_net." + name] = v.grad
    return z.detach(), ld.detach(), loss.detach(), grads


def test_mnist_spline_flow_vs_oracle():
    """buildMNISTNormalizingFlow([1], SplineNormalizer K = 8, T = 3, prior kernel 2) at B = 2, Gumbel gate with injected u1,
    u2: z, log|det J|, loss, dA and every parameter gradient against the oracle chain, by the tolerances of
    tests/test_gpu_configs.py::test_cfg4_composite_vs_oracle.  The one place where a d = 784 Spline step meets its real
    conditioner output, the [B, d, 23] view of the embedding net's [B d, 23]."""
    from conftest import rel_err, assert_close, assert_fwd
    from test_gpu_configs import TOL, GTOL
    from gnf_hip import configs
    from models import SplineNormalizer
    from models.NormalizingFlowFactories import buildMNISTNormalizingFlow
    B, K = 2, 8
    torch.manual_seed(0)
    flow = buildMNISTNormalizingFlow([1], SplineNormalizer, {"nb_bins": K, "tail_bound": T}, prior_kernel=2)
    x = configs.pseudo_mnist(torch.Generator().manual_seed(77), B, 784)
    g = torch.Generator().manual_seed(78)
    u1, u2 = torch.rand(B, 784, 784, generator=g), torch.rand(B, 784, 784, generator=g)
    z0, ld0, loss0, grads0 = _oracle_mnist_spline(flow.state_dict(), x, u1, u2, K, T)
    inside = (x >= -T) & (x <= T)
    assert int(inside.sum()) > 0                                  # the spline itself, not the identity tails alone

    flow = flow.to(DEV)
    cond = flow.steps[0].conditioner
    cond.gate_noise = (u1.to(DEV), u2.to(DEV))
    z, ld = flow(x.to(DEV))
    loss = flow.loss(z, ld)
    loss.backward()
    assert rel_err(z.cpu(), z0) < TOL and rel_err(ld.cpu(), ld0) < TOL and rel_err(loss.detach().cpu(), loss0) < TOL
    assert_fwd(z, z0, what='z')
    assert_fwd(ld, ld0, what='ld')
    assert_fwd(loss, loss0, what='loss')
    assert_close(z, z0, what="z")
    assert_close(ld, ld0, what="logdet")
    assert_close(loss, loss0, what="loss")
    named = dict(flow.named_parameters())
    assert set(named) == set(grads0)
    for k, g0 in grads0.items():
        assert named[k].grad is not None, k
        assert rel_err(named[k].grad.cpu(), g0) < GTOL, (k, rel_err(named[k].grad.cpu(), g0))
        assert_close(named[k].grad, g0, rtol=1e-4, atol=1e-6 * g0.abs().max().item(), what="d " + k)
    assert int(((cond.A.grad != 0) & (cond.A.detach() == 0)).sum()) == 0
