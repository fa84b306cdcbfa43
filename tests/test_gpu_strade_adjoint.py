"""GPU: the adjoint level sweep of a StrADE step (csrc/gnf_strade_adjoint.hip) and the rsample arm it serves
(StrADEConditioner.adjoint_levels, opt-in).

Criterion, that of tests/test_gpu_rsample.py: the kernel and a comparator -- at most depth() vjps of the existing kernels --
are two fp32 evaluations of one function in different summation orders, so each is measured against the fp64 law
(tests/strade_adjoint_ref.py:law_levels, itself checked against torch.linalg.solve on the host) and
err_kernel <= 2 err_passes + 1e-6 max|law| is required.  The operands of the grid keep every hidden pre-activation away
from a ReLU tie (tests/test_strade_adjoint_host.py asserts that margin in fp64 for every case).
Set GNF_STRADE_ADJOINT_PROFILE=<file> to have the worst measured ratios appended there."""
import ctypes
import os

import numpy as np
import pytest
import torch

import misaligned
import poison
import spline_ref as S
import strade_adjoint_ref as R
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS, TS = 8, 3.
_RATIOS = {}            # group -> [(case, err_test, err_comparator, scale)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GNF_STRADE_ADJOINT_PROFILE")
    if path and _RATIOS:
        with open(path, "a") as f:
            for group, rows in _RATIOS.items():
                worst = max(rows, key=lambda r: r[1] / max(2. * r[2] + 1e-6 * r[3], 1e-300))
                f.write("%s (tests/test_gpu_strade_adjoint.py), %d cases\n" % (group, len(rows)))
                f.write("worst err / (2 err_comparator + 1e-6 scale) = %.3f at %s: err %.3e, err_comparator %.3e, scale %.3e\n"
                        % (worst[1] / max(2. * worst[2] + 1e-6 * worst[3], 1e-300), worst[0], worst[1], worst[2], worst[3]))


def _rule(group, case, e_test, e_cmp, scale):
    print("%s | %s: err %.3e comparator %.3e scale %.3e" % (group, case, e_test, e_cmp, scale))
    _RATIOS.setdefault(group, []).append((case, e_test, e_cmp, scale))
    assert e_test <= 2. * e_cmp + 1e-6 * scale, (group, case, e_test, e_cmp, scale)


def cu(t):
    return None if t is None else t.to(DEV)


def c64(t):
    return t.detach().cpu().double()


def _device_operands(case, B):
    cond, *ts = R.operands(case, B)
    return (cond.to(DEV), *[cu(t) for t in ts])


def _passes(cond, x, ctx, g, jac, dzdh):
    """the same system by vjps of the existing kernels: lambda <- (g - N^T lambda) / jac, exact after depth() of them"""
    xa = x.detach().requires_grad_(True)
    h = cond(xa, ctx)
    lam = g / jac
    for _ in range(cond.depth()):
        nl, = torch.autograd.grad(h, xa, lam.unsqueeze(2) * dzdh, retain_graph=True, allow_unused=True)
        lam = g / jac if nl is None else (g - nl) / jac
    return lam


def _solve(cond, pack, x, g, jac, dzdh, ctx, **kw):
    from gnf_hip import ops
    return ops.strade_adjoint(cond._params(), cond._masks(), cond.level_plan(), pack, x, g, jac, dzdh, context=ctx, **kw)


def _pack(cond):
    from gnf_hip import ops
    return ops.strade_adjoint_pack(cond._params(), cond._masks(), cond.level_plan())


# --------------------------------------------------------------------------------------------- 1. kernel against the law
def test_the_grid_reaches_every_branch_of_the_kernel():
    """from the plans alone: the MFMA product, the dot product at TB = 4, a level of several chunks with a partial last one,
    nlev = 1, one variable per level"""
    from models.Conditionners.StrADEConditioner import strade_level_plan
    reached = set()
    for name, kind, c, out in R.GRID:
        plan = strade_level_plan(R.GRAPHS[name], R.hidden_of(name, kind, c), out, c)
        widths = np.diff(plan["var_off"])
        for B in R.BATCHES:
            TB, ns = R.tile_rows_of(plan, B), R.sweep_products(plan)
            if TB == 16 and (plan["max_new"] >= 8 or out >= 8) and max(ns) >= 8:
                reached.add("mfma")
            if TB == 16 and min(ns) < 8:
                reached.add("dot at TB = 16")
            if TB == 4:
                reached.add("dot at TB = 4")
        if (widths > R.CHUNK).any() and (widths[widths > R.CHUNK] % R.CHUNK != 0).any():
            reached.add("a partial last chunk")
        if plan["nlev"] == 1:
            reached.add("nlev = 1")
        if plan["nlev"] > 1 and (widths == 1).all():
            reached.add("one variable per level")
    assert reached == {"mfma", "dot at TB = 16", "dot at TB = 4", "a partial last chunk", "nlev = 1", "one variable per level"}


@pytest.mark.parametrize("case", R.GRID, ids=R.case_id)
def test_kernel_against_the_law(case):
    for B in R.BATCHES:
        cond, x, ctx, g, jac, dzdh = _device_operands(case, B)
        assert cond.level_plan() is not None
        lam = cond.adjoint_solve(x, g, jac, dzdh, context=ctx)
        assert torch.isfinite(lam).all()
        assert poison.differing(lam, _solve(cond, _pack(cond), x, g, jac, dzdh, ctx)) == 0
        with cond.hold_adjoint_pack():
            assert cond._held_adjoint is not None
            assert poison.differing(lam, cond.adjoint_solve(x, g, jac, dzdh, context=ctx)) == 0
        assert cond._held_adjoint is None
        law = R.law64(cond, x, ctx, g, jac, dzdh)
        lam_p = _passes(cond, x, ctx, g, jac, dzdh)
        print("%d of %d entries differ between the arms" % (int((lam != lam_p).sum()), lam.numel()))
        _rule("adjoint level kernel vs passes, both against the fp64 law", "%s B=%d" % (R.case_id(case), B),
              (c64(lam) - law).abs().max().item(), (c64(lam_p) - law).abs().max().item(), law.abs().max().item())


def test_the_pack_leads_with_the_level_image_and_transposes_it():
    from gnf_hip import ops
    cond = R.build_cond("d17", "40-24", 3, 2, 4).to(DEV)
    with torch.no_grad():                                            # whatever the weight holds where the mask forbids
        for l in cond._layers():
            l.weight.copy_(torch.where(l.mask == 0, torch.full_like(l.weight, float("nan")), l.weight))
    plan = cond.level_plan()
    fwd, pack = ops.strade_pack(cond._params(), cond._masks(), plan), _pack(cond)
    assert pack.data_ptr() % 16 == 0 and torch.isfinite(pack).all()
    assert poison.differing(pack[:fwd.numel()].contiguous(), fwd) == 0
    layers, masks = R.layers_of(cond, torch.float32)
    layers = [(torch.nan_to_num(W), b) for W, b in layers]
    off = fwd.numel()
    for P, _ in R.level_images(layers, masks, R.numpy_plan(cond), 3):
        rows, K = P.shape
        ldt = (rows + 15) // 16 * 16
        got = pack[off:off + K * ldt].view(K, ldt).cpu()
        assert poison.differing(got[:, :rows].contiguous(), P.t().contiguous()) == 0
        assert float(got[:, rows:].abs().max()) == 0 if ldt > rows else True
        off += K * ldt
    assert off == pack.numel()


# ------------------------------------------------------------------------------------ 2. LDS form = workspace form
BITS = [("chain5", "R", 3, 2), ("d17", "40-24", 3, 2), ("wide", "40-24", 0, 23)]      # TB = 4 dot; MFMA; chunks


@pytest.mark.parametrize("case", BITS, ids=R.case_id)
def test_lds_form_equals_workspace_form(case):
    cond, x, ctx, g, jac, dzdh = _device_operands(case, 37)
    pack = _pack(cond)
    lds = _solve(cond, pack, x, g, jac, dzdh, ctx)
    wsf = _solve(cond, pack, x, g, jac, dzdh, ctx, force_ws=True)
    assert torch.isfinite(lds).all() and poison.differing(lds, wsf) == 0


def _beyond_lds():
    torch.manual_seed(1)
    from models import StrADEConditioner
    cond = StrADEConditioner(5, [12000], 2, adjacency=R.GRAPHS["chain5"]).to(DEV)
    gen = torch.Generator().manual_seed(2)
    x, g = cu(.7 * torch.randn(6, 5, generator=gen)), cu(torch.randn(6, 5, generator=gen))
    jac, dzdh = cu(.5 + torch.rand(6, 5, generator=gen)), cu(.5 + torch.rand(6, 5, 2, generator=gen))
    return cond, x, g, jac, dzdh


def test_a_net_beyond_the_lds_tile_goes_to_the_workspace():
    from gnf_hip import abi, ops
    cond, x, g, jac, dzdh = _beyond_lds()
    params, masks, plan = cond._params(), cond._masks(), cond.level_plan()
    pack = _pack(cond)
    # the forward sweep declines the net; the adjoint asks for a workspace instead
    assert ops.strade_levels(params, masks, plan, ops.strade_pack(params, masks, plan), x, torch.zeros_like(x), 1) is None
    net = ops._strade_net([p.detach() for p in params], masks, plan)
    lam = torch.full_like(x, 7.)
    p = abi.ptr
    rc = abi.load().gnf_strade_adjoint(ctypes.byref(net), 0, None, p(pack), p(x), p(g), p(jac), p(dzdh), p(lam), 6, 0, None, 0,
                                       abi.stream())
    torch.cuda.synchronize()
    assert rc == -3 and bool((lam == 7.).all())                       # GNF_EWS, nothing launched
    a = _solve(cond, pack, x, g, jac, dzdh, None)
    b = _solve(cond, pack, x, g, jac, dzdh, None, force_ws=True)
    assert torch.isfinite(a).all() and poison.differing(a, b) == 0
    law = R.law64(cond, x, None, g, jac, dzdh)
    # 60 000 hidden units: a ReLU margin cannot be arranged here, so not the rule but the backward tolerance of the MADE tests
    # of tests/test_gpu_parity.py (1e-4): fp32 sums of 12 000 terms, and a unit decided the other way moves lambda by ~1 / width
    assert (c64(a) - law).abs().max().item() <= 1e-4 * law.abs().max().item()


@pytest.mark.parametrize("case", BITS, ids=R.case_id)
@pytest.mark.parametrize("force_ws", [False, True], ids=["lds", "ws"])
def test_poisoned_buffers_change_no_bit(case, force_ws):
    """ops.strade_adjoint with the tile's rows in LDS and in the workspace (force_ws): lambda, the weight image and the
    workspace are torch.empty of the wrappers -- zeros, NaNs and huge values in them, the same bits (tests/poison.py).  This is
    the poison case of gnf_strade_adjoint_workspace_bytes, which the name-based coverage pin of tests/test_poison_helper.py
    does not see."""
    def run():
        cond, x, ctx, g, jac, dzdh = _device_operands(case, 37)
        pack = _pack(cond)
        return {"lam": _solve(cond, pack, x, g, jac, dzdh, ctx, force_ws=force_ws), "pack": pack}
    poison.three_arms(run)


def test_a_poisoned_workspace_beyond_lds_changes_no_bit():
    """the same for a net whose rows do not fit in LDS: the workspace is not a choice there"""
    def run():
        big, x, g, jac, dzdh = _beyond_lds()
        pack = _pack(big)
        return {"pack": pack, "beyond": _solve(big, pack, x, g, jac, dzdh, None)}
    poison.three_arms(run)


# ------------------------------------------------------------------------------------------- 3. dword-aligned operands
@pytest.mark.parametrize("case", BITS, ids=R.case_id)
def test_dword_aligned_operands(case):
    cond, x, ctx, g, jac, dzdh = _device_operands(case, 37)
    pack = _pack(cond)
    want = _solve(cond, pack, x, g, jac, dzdh, ctx)
    for k in (1, 2, 3):
        moved = [misaligned.place(t, k) for t in (x, g, jac, dzdh) + ((ctx,) if ctx is not None else ())]
        assert all(t.data_ptr() % 16 == 4 * k for t in moved)
        for force in (False, True):
            got = _solve(cond, pack, *moved[:4], moved[4] if ctx is not None else None, force_ws=force)
            assert poison.differing(got, want) == 0, (k, force)
        torch.cuda.synchronize()
        assert all(misaligned.guards_intact(t) for t in moved), k
    from gnf_hip import abi
    off = torch.empty(pack.numel() + 4, device=DEV)[1:1 + pack.numel()].copy_(pack)
    with pytest.raises(abi.GnfError, match="GNF_EINVAL"):
        _solve(cond, off, x, g, jac, dzdh, ctx)


# ------------------------------------------------------------------------------------------------------ 4. path taken
class _Count:
    """calls of ops.strade_adjoint and of the conditioner module while it is entered"""

    def __init__(self, step):
        self.step, self.adjoint, self.module = step, 0, 0

    def __enter__(self):
        from gnf_hip import ops
        self._ops, self._orig = ops, ops.strade_adjoint

        def counted(*a, **k):
            self.adjoint += 1
            return self._orig(*a, **k)
        ops.strade_adjoint = counted
        self._hook = self.step.conditioner.register_forward_hook(lambda *a: setattr(self, "module", self.module + 1))
        return self

    def __exit__(self, *exc):
        self._ops.strade_adjoint = self._orig
        self._hook.remove()


def _flow(name, kind, norm, c, seed=0, out=None, integrand=None):
    from models import AffineNormalizer, MonotonicNormalizer, SplineNormalizer, buildFCNormalizingFlow
    a = R.GRAPHS[name]
    torch.manual_seed(seed)
    out = out or (2 if norm == "affine" else 3 * KS - 1)
    args = {"in_size": a.shape[0], "hidden": R.hidden_of(name, kind, c), "out_size": out, "cond_in": c, "adjacency": a}
    if norm == "monotonic":
        nargs = {"integrand_net": list(integrand), "cond_size": out, "nb_steps": 20, "solver": "CC"}
        return buildFCNormalizingFlow(1, "StrADE", args, MonotonicNormalizer, nargs).to(DEV)
    if norm == "affine":
        return buildFCNormalizingFlow(1, "StrADE", args, AffineNormalizer, {}).to(DEV)
    return buildFCNormalizingFlow(1, "StrADE", args, SplineNormalizer, {"nb_bins": KS, "tail_bound": TS}).to(DEV)


def _inputs(B, d, c, seed):
    gen = torch.Generator().manual_seed(seed)
    return .9 * torch.randn(B, d, generator=gen), (torch.randn(B, c, generator=gen) if c else None), torch.randn(B, d, generator=gen)


@pytest.mark.parametrize("c", [0, 3])
def test_the_adjoint_kernel_is_the_path_taken_when_switched_on(c):
    step = _flow("d17", "40-24", "affine", c, seed=3).steps[0]
    cond = step.conditioner
    z, ctx, w = [cu(t) for t in _inputs(4, 17, c, 1)]
    z.requires_grad_(True)
    assert step.adjoint_schedule is True and cond.adjoint_levels is False
    with _Count(step) as n:                                          # the default: the passes, as before
        (w * step.rsample(z, ctx)).sum().backward()
    assert n.adjoint == 0 and step._rsample_arm[0] == "passes" and 1 <= step._rsample_arm[1] <= cond.depth()
    lam_p = z.grad.clone()
    z.grad = None
    cond.adjoint_levels = True
    with _Count(step) as n:
        x = step.rsample(z, ctx)
        assert (n.adjoint, n.module) == (0, 0)                       # the forward is the level sweep: no module call
        (w * x).sum().backward()
    assert (n.adjoint, n.module) == (1, 1) and step._rsample_arm == ("adjoint", 0)
    assert (z.grad - lam_p).abs().max().item() <= 1e-4 * lam_p.abs().max().item()      # (the arms agree: GTOL of test_gpu_parity.py)
    step.adjoint_schedule = False
    with _Count(step) as n:
        (w * step.rsample(z, ctx)).sum().backward()
    assert (n.adjoint, n.module) == (0, 1) and step._rsample_arm[0] == "passes"


# --------------------------------------------------------------------------------------- 5. whole gradients against fp64
def _cfn(cond, dtype, ctx, P):
    ls = cond._layers()
    layers = [(P[id(l.weight)], P[id(l.bias)]) for l in ls]
    masks = [l.mask.detach().cpu().to(dtype) for l in ls]
    return lambda x: R.masked_forward(layers, masks, x, ctx if ctx is not None else x.new_zeros(x.shape[0], 0))[0]


def _unrolled(z, cfn, inv, depth):
    x = torch.zeros_like(z)
    for _ in range(depth + 1):
        x = inv(z, cfn(x))
    return x


@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("norm", ["affine", "spline"])
def test_whole_gradients_against_fp64_with_the_arm_on(norm, c):
    """L = sum w x + loss(forward(x, c)), x = rsample(z, c), with adjoint_levels on: gradients for z, c and every parameter
    against fp64 autograd through the unrolled passes; the comparator is the same restatement in fp32 on plain torch, the
    references and floors those of tests/test_gpu_strade.py::test_rsample_gradients_against_fp64"""
    B = 6
    flow = _flow("d17", "40-24", norm, c, seed=8)
    step = flow.steps[0]
    cond = step.conditioner
    cond.adjoint_levels = True
    d = cond.in_size
    gen = torch.Generator().manual_seed(44)
    z = .9 * torch.randn(B, d, generator=gen)
    ctx = torch.randn(B, c, generator=gen) if c else None
    w = torch.randn(B, d, generator=torch.Generator().manual_seed(1))
    zd, cd = cu(z).requires_grad_(True), (cu(ctx).requires_grad_(True) if c else None)
    x = flow.rsample(zd, cd)
    assert poison.differing(x.detach(), flow.invert(zd.detach(), None if cd is None else cd.detach())) == 0
    zz, ld = flow(x, cd)
    ((cu(w) * x).sum() + flow.loss(zz, ld)).backward()
    assert step._rsample_arm == ("adjoint", 0)
    names = [n for n, _ in cond.named_parameters()]
    got = {"z": zd.grad, **({"c": cd.grad} if c else {}), **{n: p.grad for n, p in cond.named_parameters()}}
    fwd, inv = ((O.affine_forward, O.affine_inverse) if norm == "affine" else
                ((lambda xx, h: S.forward(xx, h, KS, TS)), (lambda zz_, h: S.inverse(zz_, h, KS, TS))))

    def reference(dtype):
        P = {id(p): p.detach().cpu().to(dtype).requires_grad_(True) for p in cond.parameters()}
        zl = z.to(dtype).requires_grad_(True)
        cl = ctx.to(dtype).requires_grad_(True) if c else None
        cfn = _cfn(cond, dtype, cl, P)
        xx = _unrolled(zl, cfn, inv, cond.depth())
        z2, jac = fwd(xx, cfn(xx))
        L = (w.to(dtype) * xx).sum() + O.flow_loss(z2, torch.log(jac).sum(1))
        wrt = [zl] + ([cl] if c else []) + [P[id(p)] for p in cond.parameters()]
        grads = torch.autograd.grad(L, wrt, allow_unused=True)
        grads = [torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, wrt)]
        return dict(zip(["z"] + (["c"] if c else []) + names, grads))

    r64, r32 = reference(torch.float64), reference(torch.float32)
    scale_p = max(r64[n].abs().max().item() for n in names)
    for n, want in r64.items():
        assert got[n] is not None, n
        _rule("whole gradients with the adjoint arm vs plain-torch fp32, both against fp64", "%s c=%d %s" % (norm, c, n),
              (c64(got[n]) - want).abs().max().item(), (r32[n].double() - want).abs().max().item(),
              want.abs().max().item() if n in ("z", "c") else scale_p)


# ------------------------------------------------------------------------------------------------ 6. Monotonic + StrADE
def test_monotonic_strade_adjoint_arm_against_the_passes_arm():
    B, d = 5, 17
    step = _flow("d17", "40-24", "monotonic", 0, seed=21, out=4, integrand=[16, 16]).steps[0]
    cond, norm = step.conditioner, step.normalizer
    z, _, w = [cu(t) for t in _inputs(B, d, 0, 9)]
    assert step._fast_arm(z, None) is None                           # inverted by passes ...
    x = step.invert(z)
    # dL/dz of L = sum w x is lambda with J^T lambda = w; the operands both arms share, from the device
    with torch.enable_grad():
        h = cond(x.detach().requires_grad_(True), None)
        zz, jac = norm(x, h, None)
        dzdh, = torch.autograd.grad(zz, h, torch.ones_like(zz))
    law = R.law64(cond, x, None, w, jac.detach(), dzdh)
    grads = {}
    for on in (True, False):
        cond.adjoint_levels = on
        zl = z.clone().requires_grad_(True)
        xs = step.rsample(zl)
        assert poison.differing(xs.detach(), x) == 0
        (w * xs).sum().backward()
        assert step._rsample_arm[0] == ("adjoint" if on else "passes")      # ... and still solved by the kernel
        grads[on] = zl.grad
    _rule("adjoint level kernel vs passes, both against the fp64 law", "monotonic d17 out=4",
          (c64(grads[True]) - law).abs().max().item(), (c64(grads[False]) - law).abs().max().item(), law.abs().max().item())


# ------------------------------------------------------------------------------------- 7. empty batch, hand-edited mask
def test_empty_batch_launches_nothing():
    from gnf_hip import ops
    flow = _flow("d17", "40-24", "affine", 3, seed=5)
    step = flow.steps[0]
    cond = step.conditioner
    cond.adjoint_levels = True
    z = torch.zeros(0, 17, device=DEV, requires_grad=True)
    with _Count(step) as n:
        x = flow.rsample(z, torch.zeros(0, 3, device=DEV))
        assert tuple(x.shape) == (0, 17)
        x.sum().backward()
    assert n.adjoint == 0 and tuple(z.grad.shape) == (0, 17)
    assert all(p.grad is None or float(p.grad.abs().max()) == 0 for p in flow.parameters())
    e = torch.zeros(0, 17, device=DEV)
    lam = ops.strade_adjoint(cond._params(), cond._masks(), cond.level_plan(), _pack(cond), e, e, e,
                             torch.zeros(0, 17, 2, device=DEV), context=torch.zeros(0, 3, device=DEV))
    assert tuple(lam.shape) == (0, 17)


def test_a_hand_edited_mask_takes_the_passes_with_the_switch_on():
    step = _flow("d17", "40-24", "affine", 0, seed=6).steps[0]
    cond = step.conditioner
    cond.adjoint_levels = True
    z, _, w = [cu(t) for t in _inputs(4, 17, 0, 2)]
    z.requires_grad_(True)
    with torch.no_grad():
        m = cond._layers()[1].mask
        i, j = [int(v) for v in torch.nonzero(m)[0]]
        m[i, j] = 0.                                                  # one edge fewer: still a DAG, no longer the rule's masks
    assert cond.level_plan() is None
    assert cond.adjoint_solve(z.detach(), w, torch.ones_like(w), torch.ones(4, 17, 2, device=DEV)) is None
    with _Count(step) as n:
        (w * step.rsample(z)).sum().backward()
    assert n.adjoint == 0 and step._rsample_arm[0] == "passes" and torch.isfinite(z.grad).all()


def test_argument_errors_surface_as_gnf_error():
    from gnf_hip import abi, ops
    cond, x, ctx, g, jac, dzdh = _device_operands(BITS[1], 5)
    params, masks, plan, pack = cond._params(), cond._masks(), cond.level_plan(), _pack(cond)
    bad = [dict(x=x[:, :5].contiguous()), dict(g=g.t().contiguous().t()), dict(jac=jac.double()), dict(dzdh=dzdh[:, :, :1].contiguous()),
           dict(ctx=None), dict(ctx=ctx[:, :2].contiguous()), dict(g=g.cpu())]
    for kw in bad:
        a = dict(x=x, g=g, jac=jac, dzdh=dzdh, ctx=ctx)
        a.update(kw)
        with pytest.raises(abi.GnfError):
            ops.strade_adjoint(params, masks, plan, pack, a["x"], a["g"], a["jac"], a["dzdh"], context=a["ctx"])
    with pytest.raises(abi.GnfError):
        ops.strade_adjoint_pack(params, masks[:-1], plan)
