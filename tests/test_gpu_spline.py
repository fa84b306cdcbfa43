"""The Spline normalizer on the GPU (csrc/gnf_spline.hip, the spline epilogue of csrc/gnf_made_prefix.hip, ops.SplineFn /
ops.spline_inverse, models.SplineNormalizer) against tests/spline_ref.py, the law in plain torch.

Yardstick of every comparison: the reference evaluated in fp64 on the same fp32 inputs is the truth, the same reference in
fp32 on the CPU is the comparator, and the kernel's largest absolute error must be at most 2 err_comparator + 1e-6 max|truth|
per output tensor (the form of tests/test_gpu_rsample.py and tests/test_gpu_context_invert.py).  The inverse is judged by
its residual in z, because the direct inverse is ill-conditioned where jac is small.  Set GNF_SPLINE_PROFILE=<file> to have
the worst measured ratio of every group written there."""
import functools
import os

import pytest
import torch

import misaligned
import poison
import spline_cases
import spline_ref as S
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_RATIOS = {}            # group -> [(case, err, err_comparator, scale)]

SHAPES = [(1, 1), (37, 5), (300, 63)]
BINS = [2, 5, 8, 32]
LAYOUTS = ["contig", "made", "wide"]       # [B, d, C] contiguous; MADE's permuted view of [B, C, d]; 3K + 1 components
TAILS = [3., .5]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GNF_SPLINE_PROFILE")
    if path and _RATIOS:
        with open(path, "a") as f:
            for group, rows in _RATIOS.items():
                worst = max(rows, key=lambda r: r[1] / max(2. * r[2] + 1e-6 * r[3], 1e-300))
                f.write("%s (tests/test_gpu_spline.py), %d cases\n" % (group, len(rows)))
                f.write("worst err / (2 err_comparator + 1e-6 scale) = %.4f at %s: err %.3e, err_comparator %.3e, scale %.3e\n"
                        % (worst[1] / max(2. * worst[2] + 1e-6 * worst[3], 1e-300), worst[0], worst[1], worst[2], worst[3]))


TRUTH_FLOOR = 4. * 2.220446049250313e-16     # the fp64 truth's OWN roundoff, relative to quantities of size >= 1 (a lone
#                                               element at x = T has log jac = 0 exactly and -1.1e-16 in the fp64 evaluation)


def _rule(group, case, e_test, e_cmp, scale):
    print("%s | %s: err %.3e comparator %.3e scale %.3e" % (group, case, e_test, e_cmp, scale))
    _RATIOS.setdefault(group, []).append((case, e_test, e_cmp, scale))
    assert e_test <= 2. * e_cmp + 1e-6 * scale + TRUTH_FLOOR * max(1., scale), (group, case, e_test, e_cmp, scale)


def cu(t):
    return t.to(DEV)


def c64(t):
    return t.detach().cpu().double()


def _judge(group, case, got, want64, cmp32):
    """non-finite entries of the truth must come out the same (NaN where NaN, the same infinity); the finite ones by the rule"""
    got, cmp32 = c64(got), c64(cmp32)
    assert got.shape == want64.shape, (case, got.shape, want64.shape)
    nan = torch.isnan(want64)
    assert torch.equal(torch.isnan(got), nan), case
    inf = torch.isinf(want64)
    assert torch.equal(got[inf], want64[inf]), case
    fin = torch.isfinite(want64)
    if fin.any():
        both = fin & torch.isfinite(cmp32)
        _rule(group, case, (got[fin] - want64[fin]).abs().max().item(),
              (cmp32[both] - want64[both]).abs().max().item() if both.any() else 0., want64[fin].abs().max().item())


def _layout(h, layout):
    """the fp32 [B, d, C] conditioner output `h` (CPU) in one of the memory layouts, on the device"""
    B, d, C = h.shape
    if layout == "contig":
        return cu(h).contiguous()
    if layout == "made":                                         # MADE: [B, C d] viewed [B, C, d], permuted
        return cu(h.permute(0, 2, 1).contiguous()).permute(0, 2, 1)
    wide = torch.cat((h, torch.randn(B, d, 2, generator=torch.Generator().manual_seed(1))), 2)
    return cu(wide).contiguous()


@functools.lru_cache(maxsize=None)
def _draw(B, d, K, T, s, seed=0):
    """(x, h) fp32 on the CPU: x ~ 2.2 N(0, 1) T / 3 (15-22 % outside the tails), h ~ s N(0, 1)"""
    g = torch.Generator().manual_seed(1000 * B + 10 * K + int(10 * s) + seed)
    return 2.2 * T / 3. * torch.randn(B, d, generator=g), s * torch.randn(B, d, 3 * K - 1, generator=g)


def _specials(h, K, T):
    """x = T, -T, 0, an fp32 knot of element 0's own spline, +inf, -inf, NaN"""
    X, _, _ = S.knots(h.double().reshape(-1, h.shape[-1])[0], K, T)
    return [T, -T, 0., float(X[max(1, K // 2)].float()), float("inf"), float("-inf"), float("nan")]


CASES = [(sh, K, lay, T, s) for sh in SHAPES for K in BINS for lay in LAYOUTS for T in TAILS for s in (1., 4.)]


def _id(c):
    (B, d), K, lay, T, s = c
    return "%dx%d-K%d-%s-T%g-s%g" % (B, d, K, lay, T, s)


# ------------------------------------------------------------------------------------------------------- 1. values
def _values(x, h, K, T, layout, case, names=("z", "jac", "logdet", "logn")):
    from gnf_hip import ops
    hd = _layout(h, layout)
    z, jac, logdet, logn = ops.SplineFn.apply(cu(x), hd, K, T, True, True)
    z64, j64 = S.forward(x.double(), h.double(), K, T)
    z32, j32 = S.forward(x, h, K, T)
    ld64, ln64 = S.logdet_logn(z64, j64)
    ld32, ln32 = S.logdet_logn(z32, j32)
    for name, got, want, cmp in (("z", z, z64, z32), ("jac", jac, j64, j32), ("logdet", logdet, ld64, ld32),
                                 ("logn", logn, ln64, ln32)):
        if name in names:
            _judge("values: " + name, case, got, want, cmp)
    # the fused step's form: no jac, no density -- the same z and log-determinant, bit for bit
    z2, jac2, ld2, ln2 = ops.SplineFn.apply(cu(x), hd, K, T, False, False)
    assert jac2.numel() == 0 and ln2.numel() == 0
    assert poison.differing(z2, z) == 0 and poison.differing(ld2, logdet) == 0
    return z, jac


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_values(case):
    (B, d), K, layout, T, s = case
    x, h = _draw(B, d, K, T, s)
    x = x.clone()
    sp = _specials(h, K, T)
    if x.numel() >= len(sp):
        x.view(-1)[:len(sp)] = torch.tensor(sp)
        z, jac = _values(x, h, K, T, layout, _id(case))
        out = ~((x >= -T) & (x <= T))
        assert 0 < int(out.sum()) < x.numel()
        assert poison.differing(z[cu(out)], cu(x)[cu(out)]) == 0 and bool((jac[cu(out)] == 1.).all())
    else:
        _values(x, h, K, T, layout, _id(case))
        for v in sp:                                             # a lone element: every special in turn, judged by z and jac
            _values(torch.full_like(x, v), h, K, T, layout, _id(case) + "-x=%g" % v, names=("z", "jac"))


# ------------------------------------------------------------------------------------------------------- 2. inverse
def _residual(xx, h, z, K, T):
    return (S.forward(c64(xx), h.double(), K, T)[0] - z.double()).abs().max().item()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_inverse_residual(case):
    from gnf_hip import ops
    (B, d), K, layout, T, s = case
    z, h = _draw(B, d, K, T, s, seed=1)
    hd = _layout(h, layout)
    x = ops.spline_inverse(cu(z), hd, K, T)
    out = ~((z >= -T) & (z <= T))
    assert poison.differing(x[cu(out)], cu(z)[cu(out)]) == 0
    _rule("inverse residual in z", _id(case), _residual(x, h, z, K, T), _residual(S.inverse(z, h, K, T), h, z, K, T),
          z.abs().max().item())
    # the variable-major scatter form: the [B, d] problem read as B variables of d samples, written into columns of a
    # [d, width] tensor -- the same bits where it writes, and not a bit anywhere else
    width = B + 3
    cols = torch.randperm(width, generator=torch.Generator().manual_seed(B))[:B].to(torch.int32)
    target = torch.empty(d, width)
    target.view(torch.int32).fill_(misaligned.SENTINEL)
    target = cu(target)
    ops.spline_inverse(cu(z), hd, K, T, out=target, out_cols=cu(cols))
    assert poison.differing(target[:, cu(cols).long()].t().contiguous(), x) == 0
    rest = torch.ones(width, dtype=torch.bool)
    rest[cols.long()] = False
    assert bool((target[:, cu(rest)].contiguous().view(torch.int32) == misaligned.SENTINEL).all())


# ------------------------------------------------------------------------------------------------------- 3. gradients
COTANGENTS = [("z", "jac"), ("z", "logdet"), ("logdet", "logn")]
GRAD_CASES = [(sh, K, lay, T, s) for sh in SHAPES for K in BINS for lay in LAYOUTS for T in TAILS for s in (1., 2.)]


@pytest.mark.parametrize("case", GRAD_CASES, ids=_id)
def test_gradients(case):
    from gnf_hip import ops
    (B, d), K, layout, T, s = case
    x, h = _draw(B, d, K, T, s, seed=2)
    # the knife edge by construction: dz/dh and djac/dh of an element ON a knot are those of either bin
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
    for which in COTANGENTS:
        (gx64, gh64), (gx32, gh32) = reference(torch.float64, which), reference(torch.float32, which)
        for with_gx in (True, False):
            xd = cu(x).requires_grad_(with_gx)
            hd = _layout(h, layout).detach().requires_grad_(True)
            z, jac, ld, ln = ops.SplineFn.apply(xd, hd, K, T, "jac" in which, "logn" in which)
            loss({"z": z, "jac": jac, "logdet": ld, "logn": ln}, which, cu).backward()
            tag = "%s-%s%s" % (_id(case), "+".join(which), "" if with_gx else "-nogx")
            if with_gx:
                _judge("gradients: gx", tag, xd.grad, gx64, gx32)
            else:
                assert xd.grad is None
            assert hd.grad.shape == hd.shape
            _judge("gradients: gh", tag, hd.grad[:, :, :C], gh64, gh32)
            assert bool((hd.grad[:, :, C:] == 0).all())


# ------------------------------------------------------------------------------------------------------- 4. steps and flows
KS, TS = 5, 3.


def _made_flow(d, c=0, hidden=(19,), seed=0, K=KS, T=TS):
    from models import AutoregressiveConditioner, SplineNormalizer, buildFCNormalizingFlow
    torch.manual_seed(seed)
    flow = buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": d, "hidden": list(hidden), "out_size": 3 * K - 1,
                                                                 "cond_in": c}, SplineNormalizer,
                                  {"nb_bins": K, "tail_bound": T})
    return flow.to(DEV)


def _made_fn(cond, dtype, ctx):
    """h [B, d, C] of the conditioner from its own parameters and mask buffers, in `dtype` on the CPU"""
    from adjoint_ref import made_t
    P = {"masked_autoregressive_net." + n: p.detach().cpu().to(dtype)
         for n, p in cond.masked_autoregressive_net.named_parameters()}
    return lambda v: made_t(cond, P, v, ctx.to(dtype))


class _Spy:
    """the (t0, t1, mode) of every ops.made_prefix_steps call and the conditioner module calls while entered"""

    def __init__(self, step):
        self.step, self.calls, self.module = step, [], 0

    def __enter__(self):
        from gnf_hip import ops
        self._ops, self._orig = ops, ops.made_prefix_steps

        def spied(params, plan, pack, z, x, t0, t1, mode, **kw):
            self.calls.append((t0, t1, mode))
            return self._orig(params, plan, pack, z, x, t0, t1, mode, **kw)
        ops.made_prefix_steps = spied
        self._hook = self.step.conditioner.register_forward_hook(lambda *a: setattr(self, "module", self.module + 1))
        return self

    def __exit__(self, *exc):
        self._ops.made_prefix_steps = self._orig
        self._hook.remove()


@pytest.mark.parametrize("c", [0, 2])
@pytest.mark.parametrize("d", [1, 2, 5, 17])
def test_made_invert_one_launch(d, c):
    from gnf_hip import ops
    B = 9
    flow = _made_flow(d, c, seed=10 * d + c)
    step = flow.steps[0]
    cond = step.conditioner
    g = torch.Generator().manual_seed(d)
    z = 2.2 * torch.randn(B, d, generator=g)
    ctx = torch.randn(B, c, generator=g)
    kw = {"context": cu(ctx)} if c else {}
    with _Spy(step) as spy:
        x_col = step.invert(cu(z), *([cu(ctx)] if c else []))
    assert spy.calls == [(0, d, ops.MADE_NORM_SPLINE)] and spy.module == 0
    step.column_schedule = False
    with _Spy(step) as spy:
        x_pass = step.invert(cu(z), *([cu(ctx)] if c else []))
    step.column_schedule = True
    assert spy.calls == [] and 1 <= spy.module <= d
    inv = lambda dtype: (lambda zz, h: S.inverse(zz, h, KS, TS))
    x64 = O.step_invert(z.double(), _made_fn(cond, torch.float64, ctx), inv(torch.float64), d - 1)
    case = "d=%d c=%d" % (d, c)
    _rule("Spline + MADE invert, columns vs passes, both against fp64", case, (c64(x_col) - x64).abs().max().item(),
          (c64(x_pass) - x64).abs().max().item(), x64.abs().max().item())
    # forward(invert(z)) = z, by the residual of an fp64 forward; the comparator is the plain-torch fp32 inversion
    x32 = O.step_invert(z, _made_fn(cond, torch.float32, ctx), inv(torch.float32), d - 1)
    fwd64 = lambda xx: S.forward(c64(xx), _made_fn(cond, torch.float64, ctx)(c64(xx)), KS, TS)[0]
    _rule("Spline + MADE forward(invert(z)) residual", case, (fwd64(x_col) - z.double()).abs().max().item(),
          (fwd64(x32) - z.double()).abs().max().item(), z.abs().max().item())
    with torch.no_grad():
        zz, _ = flow(x_col, *([cu(ctx)] if c else []))
    assert (c64(zz) - z.double()).abs().max().item() <= 1e-4 * max(1., z.abs().max().item())
    # partial calls through the workspace: (0, t) then (t, d) give the bits of (0, d)
    plan, params = cond.prefix_plan(with_context=bool(c)), cond._prefix_params()
    pack = ops.made_prefix_pack(params, plan)
    zd = cu(z).contiguous()
    one = ops.made_prefix_steps(params, plan, pack, zd, torch.zeros_like(zd), 0, d, ops.MADE_NORM_SPLINE, spline=(KS, TS), **kw)
    assert poison.differing(one, x_col) == 0
    for t in sorted({1, d // 2, d - 1} - {0, d}):
        ws = ops.made_prefix_workspace(params, plan, B)
        two = torch.zeros_like(zd)
        ops.made_prefix_steps(params, plan, pack, zd, two, 0, t, ops.MADE_NORM_SPLINE, ws=ws, spline=(KS, TS), **kw)
        ops.made_prefix_steps(params, plan, pack, zd, two, t, d, ops.MADE_NORM_SPLINE, ws=ws, spline=(KS, TS), **kw)
        assert poison.differing(two, one) == 0, t


def _dag_step(d=6, K=KS, T=TS):
    from models import DAGConditioner, SplineNormalizer, buildFCNormalizingFlow
    torch.manual_seed(21)
    flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [16, 16], "out_size": 3 * K - 1,
                                                      "hot_encoding": True}, SplineNormalizer, {"nb_bins": K, "tail_bound": T})
    cond = flow.steps[0].conditioner
    cond.A.data.copy_(torch.tril(torch.rand(d, d) + .1, -1) * (torch.rand(d, d) < .6).float())
    cond.stoch_gate = cond.noise_gate = False
    cond.invalidate_caches()
    return flow.to(DEV)


def test_dag_step_inverts_by_levels():
    flow = _dag_step()
    step = flow.steps[0]
    z = cu(2.2 * torch.randn(9, 6, generator=torch.Generator().manual_seed(3)))
    calls = []
    hook = step.conditioner.register_forward_hook(lambda *a: calls.append(1))
    into = []
    orig = step.normalizer.inverse_transform_into
    step.normalizer.inverse_transform_into = lambda *a, **k: (into.append(1), orig(*a, **k))[1]
    try:
        x_lev = step.invert(z)
        assert not calls and into                                # the level schedule, through the scatter form
        step.level_schedule = False
        x_pass = step.invert(z)
        assert calls
    finally:
        hook.remove()
        step.level_schedule = True
        del step.normalizer.inverse_transform_into
    # non-parents are masked by exact zeros in both schedules: the same function, other summation orders at most
    assert (c64(x_lev) - c64(x_pass)).abs().max().item() <= 1e-5 * max(1., c64(x_pass).abs().max().item())
    with torch.no_grad():
        zz, _ = flow(x_lev)
    assert (c64(zz) - c64(z)).abs().max().item() <= 1e-4 * max(1., c64(z).abs().max().item())


# ------------------------------------------------------------------------------------------------------- 5. rsample
def _unrolled(cfn, depth, z, K, T):
    x = torch.zeros_like(z)
    for _ in range(depth + 1):
        x = S.inverse(z, cfn(x), K, T)
    return x


@pytest.mark.parametrize("kind", ["made", "coupling"])
def test_rsample_gradients_against_fp64(kind):
    """L = sum w x, x = rsample(z, c): gradients for z, the context and every parameter against fp64 autograd through the
    unrolled passes (exact: the step's Jacobian is nilpotent off the diagonal); the comparator is the same in fp32"""
    from adjoint_ref import leaves, made_t
    from context_ref import coupling64
    from models import AutoregressiveConditioner, CouplingConditioner, SplineNormalizer, buildFCNormalizingFlow
    d, c, B = 5, 2, 6
    torch.manual_seed(31)
    T_ = {"made": AutoregressiveConditioner, "coupling": CouplingConditioner}[kind]
    flow = buildFCNormalizingFlow(1, T_, {"in_size": d, "hidden": [19], "out_size": 3 * KS - 1, "cond_in": c},
                                  SplineNormalizer, {"nb_bins": KS, "tail_bound": TS}).to(DEV)
    step, cond = flow.steps[0], flow.steps[0].conditioner
    g = torch.Generator().manual_seed(5)
    z, ctx, w = 1.5 * torch.randn(B, d, generator=g), torch.randn(B, c, generator=g), torch.randn(B, d, generator=g)
    zd, cd = cu(z).requires_grad_(True), cu(ctx).requires_grad_(True)
    x = flow.rsample(zd, cd)
    assert poison.differing(x.detach(), flow.invert(zd.detach(), cd.detach())) == 0
    (cu(w) * x).sum().backward()
    assert step._rsample_arm[0] == ("adjoint" if kind == "made" else "passes")
    names = [n for n, _ in flow.named_parameters()]
    got = {"z": zd.grad, "c": cd.grad, **{n: p.grad for n, p in flow.named_parameters()}}

    def reference(dtype):
        P = leaves(flow, dtype)
        zl, cl = z.to(dtype).clone().requires_grad_(True), ctx.to(dtype).clone().requires_grad_(True)
        pre = "steps.0.conditioner."
        if kind == "made":
            cfn, depth = (lambda v: made_t(cond, P, v, cl, pre)), d - 1
        else:
            cfn, depth = (lambda v: coupling64(cond, P, v, cl, pre)), 1
        L = (w.to(dtype) * _unrolled(cfn, depth, zl, KS, TS)).sum()
        wrt = [zl, cl] + [P[n] for n in names]
        grads = torch.autograd.grad(L, wrt, allow_unused=True)
        return dict(zip(["z", "c"] + names, [torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, wrt)]))

    r64, r32 = reference(torch.float64), reference(torch.float32)
    scale_p = max(r64[n].abs().max().item() for n in names)
    for name, want in r64.items():
        assert got[name] is not None, name
        scale = want.abs().max().item() if name in ("z", "c") else scale_p
        _rule("rsample gradients vs plain-torch fp32, both against fp64", "%s %s" % (kind, name),
              (c64(got[name]) - want).abs().max().item(), (r32[name].double() - want).abs().max().item(), scale)


# ------------------------------------------------------------------------------------------------------- 6. hygiene
def _ops_case(K=8, T=3., B=37, d=5, layout="contig"):
    x, h = _draw(B, d, K, T, 1., seed=4)
    return S.to_bin_middles(x, h, K, T), h, _layout(h, layout)


def _ops_shapes(layout):
    """(B, d) of the hygiene cases: the short rows, and a chunked row (two chunks, the second of one lane) for the layouts
    spline_cases.ALIGN names"""
    return [(37, 5)] + [(B, d) for B, d, K, lay in spline_cases.ALIGN if lay == layout and K == 8]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_three_arms_normalizer_entry_points(layout):
    for B, d in _ops_shapes(layout):
        _three_arms_normalizer_entry_points(layout, B, d)


def _three_arms_normalizer_entry_points(layout, B, d):
    from gnf_hip import ops
    K, T = 8, 3.

    def run():
        x, h, hd = _ops_case(K, T, B, d, layout=layout)
        xd, hd = cu(x).requires_grad_(True), hd.detach().requires_grad_(True)
        z, jac, ld, ln = ops.SplineFn.apply(xd, hd, K, T, True, True)
        ((z * z).sum() + jac.sum() + ld.sum() + ln.sum()).backward()
        xi = ops.spline_inverse(z.detach(), hd.detach(), K, T)
        tgt = torch.zeros(x.shape[1], x.shape[0] + 2, device=DEV)
        ops.spline_inverse(z.detach(), hd.detach(), K, T, out=tgt,
                           out_cols=torch.arange(x.shape[0], dtype=torch.int32, device=DEV))
        return {"z": z.detach(), "jac": jac.detach(), "logdet": ld.detach(), "logn": ln.detach(), "gx": xd.grad,
                "gh": hd.grad, "inv": xi, "scatter": tgt}
    poison.three_arms(run)


@pytest.mark.parametrize("c", [0, 2])
def test_three_arms_prefix_entry_points(c):
    def run():
        flow = _made_flow(5, c, seed=77)
        g = torch.Generator().manual_seed(8)
        z, ctx = cu(2.2 * torch.randn(9, 5, generator=g)), cu(torch.randn(9, c, generator=g))
        return {"x": flow.steps[0].invert(z, *([ctx] if c else []))}
    poison.three_arms(run)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_dword_aligned_operands(layout, k):
    """every fp32 array of the three entry points 4 k bytes past a 16-byte boundary: the same bits as the aligned call, and
    not a bit outside the arrays.  On the chunked row the span then starts off the 16-byte grid in every tile, which all go
    by dwords (tests/test_spline_routes_host.py asserts the route)"""
    for B, d in _ops_shapes(layout):
        _dword_aligned_operands(layout, k, B, d)


def _dword_aligned_operands(layout, k, B, d):
    from gnf_hip import ops
    K, T = 8, 3.
    x, h, hd = _ops_case(K, T, B, d, layout=layout)
    g = torch.Generator().manual_seed(9)
    cot = [cu(torch.randn(B, d, generator=g)), cu(torch.randn(B, d, generator=g)), cu(torch.randn(B, generator=g)),
           cu(torch.randn(B, generator=g))]

    def run(k):
        P = lambda t: misaligned.place(t, k)
        xs, hs = P(cu(x)), P(hd)
        outs = [P(torch.zeros(B, d, device=DEV)), P(torch.zeros(B, d, device=DEV)), P(torch.zeros(B, device=DEV)),
                P(torch.zeros(B, device=DEV))]
        st = lambda t: (t.stride(0), t.stride(1), t.stride(2), t.shape[2])
        ops.call("gnf_spline_fwd", ops.ptr(xs), ops.ptr(hs), *st(hs), K, T, *[ops.ptr(o) for o in outs], B, d, ops.stream())
        cs = [P(t) for t in cot]
        gx, gh = P(torch.zeros(B, d, device=DEV)), P(torch.zeros_like(hd))
        ops.call("gnf_spline_bwd", ops.ptr(xs), ops.ptr(hs), *st(hs), K, T, *[ops.ptr(t) for t in cs], ops.ptr(gx), ops.ptr(gh),
                 gh.stride(0), gh.stride(1), gh.stride(2), B, d, ops.stream())
        xi = P(torch.zeros(B, d, device=DEV))
        ops.call("gnf_spline_inv", ops.ptr(outs[0]), ops.ptr(hs), *st(hs), K, T, ops.ptr(xi), None, 0, B, d, ops.stream())
        tgt = P(torch.zeros(d, B + 2, device=DEV))
        colsd = torch.arange(B, dtype=torch.int32, device=DEV)
        ops.call("gnf_spline_inv", ops.ptr(outs[0]), ops.ptr(hs), *st(hs), K, T, ops.ptr(tgt), ops.abi.rawptr(colsd), B + 2, B, d,
                 ops.stream())
        torch.cuda.synchronize()
        every = [xs, hs] + outs + cs + [gx, gh, xi, tgt]
        assert all(misaligned.guards_intact(t) for t in every)
        return [t.clone() for t in outs + [gx, gh, xi, tgt]]
    base, moved = run(0), run(k)
    for a, b in zip(base, moved):
        assert poison.differing(a, b) == 0


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("c", [0, 2])
def test_dword_aligned_prefix_operands(c, k):
    """gnf_made_prefix_spline / gnf_made_prefix_ctx_spline with z, x and the context 4 k bytes past a 16-byte boundary"""
    from gnf_hip import ops
    d, B = 5, 9
    cond = _made_flow(d, c, seed=78).steps[0].conditioner
    plan, params = cond.prefix_plan(with_context=bool(c)), cond._prefix_params()
    pack = ops.made_prefix_pack(params, plan)
    g = torch.Generator().manual_seed(8)
    z, ctx = cu(2.2 * torch.randn(B, d, generator=g)), cu(torch.randn(B, c, generator=g))

    def run(k):
        zs, xs = misaligned.place(z, k), misaligned.place(torch.zeros_like(z), k)
        kw = {"context": misaligned.place(ctx, k)} if c else {}
        ops.made_prefix_steps(params, plan, pack, zs, xs, 0, d, ops.MADE_NORM_SPLINE, spline=(KS, TS), **kw)
        torch.cuda.synchronize()
        assert all(misaligned.guards_intact(t) for t in [zs, xs] + list(kw.values()))
        return xs.clone()
    assert poison.differing(run(0), run(k)) == 0


def test_empty_batch():
    from gnf_hip import ops
    from models import SplineNormalizer
    norm = SplineNormalizer()
    x, h = torch.zeros(0, 5, device=DEV, requires_grad=True), torch.zeros(0, 5, 23, device=DEV, requires_grad=True)
    z, jac = norm(x, h)
    zz, ld = norm.forward_logdet(x, h)
    assert tuple(z.shape) == tuple(jac.shape) == tuple(zz.shape) == (0, 5) and tuple(ld.shape) == (0,)
    (z.sum() + jac.sum() + ld.sum()).backward()
    assert tuple(x.grad.shape) == (0, 5) and tuple(h.grad.shape) == (0, 5, 23)
    assert tuple(norm.inverse_transform(x.detach(), h.detach()).shape) == (0, 5)
    assert tuple(ops.spline_inverse(torch.zeros(3, 0, device=DEV), torch.zeros(3, 0, 23, device=DEV)).shape) == (3, 0)
    tgt = torch.full((0, 7), 2., device=DEV)                     # the level schedule's form of an empty batch
    ops.spline_inverse(torch.zeros(3, 0, device=DEV), torch.zeros(3, 0, 23, device=DEV), out=tgt,
                       out_cols=torch.arange(3, dtype=torch.int32, device=DEV))
    assert tuple(_made_flow(5).steps[0].invert(torch.zeros(0, 5, device=DEV)).shape) == (0, 5)


def test_graphed_training_step():
    """GraphedStep.graphable accepts a Spline + Coupling flow, and replayed steps give the eager steps' loss and parameters
    to the bit (the same kernels on the same operands in the same order)"""
    from gnf_hip import dp
    from models import CouplingConditioner, SplineNormalizer, buildFCNormalizingFlow

    def make():
        torch.manual_seed(41)
        return buildFCNormalizingFlow(2, CouplingConditioner, {"in_size": 6, "hidden": [32, 32], "out_size": 23},
                                      SplineNormalizer, {}).to(DEV)
    xs = [cu(1.5 * torch.randn(100, 6, generator=torch.Generator().manual_seed(50 + i))) for i in range(4)]
    fa = make()
    assert dp.GraphedStep.graphable(fa)
    sa = dp.FlatState(fa)
    for x in xs:
        la = dp.train_step(fa, sa, x, lr=1e-3, graph=False)
    fb = make()
    sb = dp.FlatState(fb)
    gs = dp.GraphedStep(fb, sb, xs[0], lr=1e-3, warmup=1)
    for x in xs[1:]:
        lb = gs(x)
    torch.cuda.synchronize()
    assert gs.captures == 1 and sb.t == sa.t == 4
    assert poison.differing(lb.detach().reshape(()), la.detach().reshape(())) == 0
    assert poison.differing(sb.flat, sa.flat) == 0
