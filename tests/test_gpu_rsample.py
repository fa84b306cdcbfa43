"""Differentiable sampling: NormalizingFlowStep.rsample / FCNormalizingFlow.rsample and the adjoint MADE column sweep
(csrc/gnf_made_adjoint.hip) behind its backward.

The forward is invert, bit for bit.  The backward solves J^T lambda = g at the sample -- by the adjoint kernel (MADE, one
launch) or by at most depth() vjps of the existing kernels (any conditioner) -- and makes one vjp of the step with -lambda.

Criterion, that of tests/test_gpu_context_invert.py: the thing under test and a comparator are two fp32 evaluations of one
function in different summation orders, so each is measured against fp64 (tests/adjoint_ref.py) and
err_test <= 2 err_comparator + 1e-6 max|reference| is required (margin 2, element-wise floor of DESIGN.md section 2).
Set GNF_RSAMPLE_PROFILE=<file> to have the worst measured ratios appended there."""
import os

import pytest
import torch

from adjoint_ref import _pairs, elbo_like, law_sweep, leaves, made_layers, made_t, plan_of
from misaligned import guards_intact, place
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_RATIOS = {}            # group -> [(case, err_test, err_comparator, scale)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GNF_RSAMPLE_PROFILE")
    if path and _RATIOS:
        with open(path, "a") as f:
            for group, rows in _RATIOS.items():
                worst = max(rows, key=lambda r: r[1] / max(2. * r[2] + 1e-6 * r[3], 1e-300))
                f.write("%s (tests/test_gpu_rsample.py), %d cases\n" % (group, len(rows)))
                f.write("worst err / (2 err_comparator + 1e-6 scale) = %.3f at %s: err %.3e, err_comparator %.3e, scale %.3e\n"
                        % (worst[1] / max(2. * worst[2] + 1e-6 * worst[3], 1e-300), worst[0], worst[1], worst[2], worst[3]))


def _rule(group, case, e_test, e_cmp, scale):
    print("%s | %s: err %.3e comparator %.3e scale %.3e" % (group, case, e_test, e_cmp, scale))
    _RATIOS.setdefault(group, []).append((case, e_test, e_cmp, scale))
    assert e_test <= 2. * e_cmp + 1e-6 * scale, (group, case, e_test, e_cmp, scale)


def cu(t):
    return t.to(DEV)


def c64(t):
    return t.detach().cpu().double()


def _flow(kind, d, c, hidden, seed=0, nb_flow=1, out=2, integrand=None):
    from models import (AffineNormalizer, AutoregressiveConditioner, CouplingConditioner, MonotonicNormalizer,
                        buildFCNormalizingFlow)
    T = {"made": AutoregressiveConditioner, "coupling": CouplingConditioner}[kind]
    torch.manual_seed(seed)
    cargs = {"in_size": d, "hidden": list(hidden), "out_size": out, "cond_in": c}
    if integrand is None:
        return buildFCNormalizingFlow(nb_flow, T, cargs, AffineNormalizer, {}).to(DEV)
    return buildFCNormalizingFlow(nb_flow, T, cargs, MonotonicNormalizer,
                                  {"integrand_net": list(integrand), "cond_size": out, "nb_steps": 20, "solver": "CC"}).to(DEV)


def _dag_step(d=6):
    from models import AffineNormalizer, DAGConditioner, buildFCNormalizingFlow
    torch.manual_seed(21)
    flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [16, 16], "out_size": 2, "hot_encoding": True},
                                  AffineNormalizer, {})
    cond = flow.steps[0].conditioner
    cond.A.data.copy_(torch.tril(torch.rand(d, d) + .1, -1) * (torch.rand(d, d) < .6).float())
    cond.stoch_gate = cond.noise_gate = False
    cond.invalidate_caches()
    return flow.to(DEV).steps[0]


def _inputs(B, d, c, seed):
    gen = torch.Generator().manual_seed(seed)
    z = cu(.7 * torch.randn(B, d, generator=gen))
    ctx = cu(torch.randn(B, c, generator=gen)) if c else None
    w = cu(torch.randn(B, d, generator=gen))
    return z, ctx, w


class _Count:
    """calls of ops.made_adjoint and of a conditioner module while it is entered"""

    def __init__(self, step):
        self.step, self.adjoint, self.module = step, 0, 0

    def __enter__(self):
        from gnf_hip import ops
        self._ops, self._orig = ops, ops.made_adjoint

        def counted(*a, **k):
            self.adjoint += 1
            return self._orig(*a, **k)
        ops.made_adjoint = counted
        self._hook = self.step.conditioner.register_forward_hook(lambda *a: setattr(self, "module", self.module + 1))
        return self

    def __exit__(self, *exc):
        self._ops.made_adjoint = self._orig
        self._hook.remove()


# ------------------------------------------------------------------------------------------------------- path taken
def test_the_adjoint_kernel_is_the_path_taken_for_a_made_step():
    step = _flow("made", 5, 2, [19]).steps[0]
    z, ctx, w = _inputs(3, 5, 2, 1)
    z.requires_grad_(True)
    assert step.adjoint_schedule is True
    with _Count(step) as n:
        x = step.rsample(z, ctx)
        assert (n.adjoint, n.module) == (0, 0)      # the forward is the column sweep: no module call
        (w * x).sum().backward()
    assert (n.adjoint, n.module) == (1, 1) and step._rsample_arm == ("adjoint", 0)
    step.adjoint_schedule = False
    with _Count(step) as n:
        (w * step.rsample(z, ctx)).sum().backward()
    assert (n.adjoint, n.module) == (0, 1)
    assert step._rsample_arm[0] == "passes" and 1 <= step._rsample_arm[1] <= 4


def test_a_coupling_step_runs_one_pass():
    step = _flow("coupling", 6, 2, [16]).steps[0]
    z, ctx, w = _inputs(4, 6, 2, 2)
    z.requires_grad_(True)
    with _Count(step) as n:
        (w * step.rsample(z, ctx)).sum().backward()
    assert n.adjoint == 0 and step._rsample_arm == ("passes", 1)


# ------------------------------------------------------------------------------------------------- forward identity
@pytest.mark.parametrize("kind,c,integrand", [("made", 2, None), ("made", 0, None), ("coupling", 2, None), ("made", 2, [16, 16])],
                         ids=["made-c2", "made-c0", "coupling", "made-monotonic"])
def test_forward_is_invert_bit_for_bit(kind, c, integrand):
    flow = _flow(kind, 5, c, [19], seed=3, nb_flow=2, out=2 if integrand is None else 4, integrand=integrand)
    z, ctx, _ = _inputs(9, 5, c, 3)
    z.requires_grad_(True)
    x = flow.rsample(z, ctx)
    assert x.requires_grad and torch.equal(x.detach(), flow.invert(z.detach(), ctx))
    x1 = flow.steps[1].rsample(z, ctx)
    assert torch.equal(x1.detach(), flow.steps[1].invert(z.detach(), ctx))


# --------------------------------------------------------------------------------------------- kernel against the law
def _kernel_operands(d, c, hidden, B, seed):
    flow = _flow("made", d, c, hidden, seed=seed)
    cond = flow.steps[0].conditioner
    with torch.no_grad():
        # twice the initial weights: the off-diagonal part of J is then large enough for the two arms' summation orders to
        # show in lambda (as initialised they agree bit for bit in most entries)
        for l in cond.masked_autoregressive_net.masked_layers():
            l.weight.mul_(2.)
    gen = torch.Generator().manual_seed(1000 + B + d + c)
    x, g = cu(.7 * torch.randn(B, d, generator=gen)), cu(torch.randn(B, d, generator=gen))
    ctx = cu(torch.randn(B, c, generator=gen)) if c else None
    jac = cu(.5 + torch.rand(B, d, generator=gen))                   # synthetic and positive
    dzdh = cu(.5 + torch.rand(B, d, 2, generator=gen))
    return cond, x, ctx, g, jac, dzdh


def _law64(cond, c, x, ctx, g, jac, dzdh):
    ctx64 = c64(ctx) if ctx is not None else torch.zeros(x.shape[0], 0, dtype=torch.float64)
    return law_sweep(made_layers(cond), plan_of(cond), c, c64(x), ctx64, c64(g), c64(jac), c64(dzdh))


def _passes(cond, x, ctx, g, jac, dzdh):
    """the same system by vjps of the existing kernels: lambda <- (g - N^T lambda) / jac, exact after d - 1 of them"""
    xa = x.detach().requires_grad_(True)
    h = cond(xa, ctx)
    lam = g / jac
    for _ in range(x.shape[1] - 1):
        nl, = torch.autograd.grad(h, xa, lam.unsqueeze(2) * dzdh, retain_graph=True, allow_unused=True)
        lam = g / jac if nl is None else (g - nl) / jac
    return lam


GRID = [(d, c, hidden) for d in (1, 2, 5, 17) for hidden in ([], [8], [24, 24], [40, 33, 19]) for c in (0, 3)]
NAMED = [(17, 3, [40, 33, 19]), (3, 1, [40, 33])]                     # the lane-group dot path; the MFMA path


def _case_id(p):
    d, c, hidden = p
    name = {0: "dot-", 1: "mfma-"}.get(NAMED.index(p), "") if p in NAMED else ""
    return "%sd%d-c%d-%s" % (name, d, c, "x".join(map(str, hidden)) or "none")


@pytest.mark.parametrize("case", GRID + NAMED[1:], ids=_case_id)
def test_kernel_against_the_law(case):
    from gnf_hip import ops
    d, c, hidden = case
    for B in (5, 37):                                                # a ragged tile; several tiles
        cond, x, ctx, g, jac, dzdh = _kernel_operands(d, c, hidden, B, seed=100 * d + 10 * c + len(hidden))
        plan, params = cond.prefix_plan(with_context=bool(c)), cond._prefix_params()
        assert plan is not None
        if case == NAMED[1]:
            assert plan["max_new"] >= 8                              # TB = 16 and n >= 8: the MFMA inner product
        if case == NAMED[0]:
            assert plan["max_new"] < 8
        lam = cond.adjoint_solve(x, g, jac, dzdh, context=ctx)
        assert torch.equal(lam, ops.made_adjoint(params, plan, ops.made_adjoint_pack(params, plan), x, g, jac, dzdh,
                                                 context=ctx))
        law = _law64(cond, c, x, ctx, g, jac, dzdh)
        assert torch.isfinite(lam).all()
        lam_p = _passes(cond, x, ctx, g, jac, dzdh)
        print("%d of %d entries differ between the arms" % (int((lam != lam_p).sum()), lam.numel()))
        _rule("adjoint kernel vs passes, both against the fp64 law", "%s B=%d" % (_case_id(case), B),
              (c64(lam) - law).abs().max().item(), (c64(lam_p) - law).abs().max().item(), law.abs().max().item())


def test_kernel_with_a_sampled_ordering():
    from models.Conditionners.AutoregressiveConditioner import ConditionnalMADE
    d, c, B = 9, 2, 37
    cond, x, ctx, g, jac, dzdh = _kernel_operands(d, c, [20, 20], B, seed=5)
    torch.manual_seed(6)
    cond.masked_autoregressive_net = ConditionnalMADE(nin=d, cond_in=c, hidden_sizes=[20, 20], nout=2 * d, num_masks=3,
                                                      random=True).to(DEV)
    cond.masked_autoregressive_net.update_masks()
    lam = cond.adjoint_solve(x, g, jac, dzdh, context=ctx)
    law = _law64(cond, c, x, ctx, g, jac, dzdh)
    _rule("adjoint kernel vs passes, both against the fp64 law", "sampled ordering d=9 c=2",
          (c64(lam) - law).abs().max().item(), (c64(_passes(cond, x, ctx, g, jac, dzdh)) - law).abs().max().item(),
          law.abs().max().item())


@pytest.mark.parametrize("case", NAMED, ids=["dot", "mfma"])
def test_lds_form_equals_workspace_form(case):
    from gnf_hip import ops
    d, c, hidden = case
    cond, x, ctx, g, jac, dzdh = _kernel_operands(d, c, hidden, 37, seed=3)
    plan, params = cond.prefix_plan(with_context=True), cond._prefix_params()
    pack = ops.made_adjoint_pack(params, plan)
    lds = ops.made_adjoint(params, plan, pack, x, g, jac, dzdh, context=ctx)
    wsf = ops.made_adjoint(params, plan, pack, x, g, jac, dzdh, context=ctx, force_ws=True)
    assert torch.isfinite(lds).all() and torch.equal(lds, wsf)


@pytest.mark.parametrize("case", NAMED, ids=["dot", "mfma"])
def test_dword_aligned_operands(case):
    from gnf_hip import ops
    d, c, hidden = case
    cond, x, ctx, g, jac, dzdh = _kernel_operands(d, c, hidden, 37, seed=3)
    plan, params = cond.prefix_plan(with_context=True), cond._prefix_params()
    pack = ops.made_adjoint_pack(params, plan)
    want = ops.made_adjoint(params, plan, pack, x, g, jac, dzdh, context=ctx)
    for k in (1, 2, 3):
        moved = [place(t, k) for t in (x, g, jac, dzdh, ctx)]
        assert all(t.data_ptr() % 16 == 4 * k for t in moved)
        got = ops.made_adjoint(params, plan, pack, *moved[:4], context=moved[4])
        assert torch.equal(got, want), k
        assert all(guards_intact(t) for t in moved), k


# --------------------------------------------------------------------------------------- whole gradients against fp64
@pytest.mark.parametrize("nb_flow", [1, 2])
@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("kind", ["made", "coupling"])
def test_whole_gradients_against_fp64(kind, c, nb_flow):
    """L = sum w x + loss(forward(x, c)), x = rsample(z, c): the shape of an ELBO.  Gradients for z, c and every parameter
    against fp64 autograd through the unrolled passes; the comparator is the same restatement in fp32 on plain torch.
    Every tensor is held to the rule on its own error; the floor is 1e-6 of the largest entry of its group (z, c, all
    parameters): the roundoff of a backward pass is relative to the cotangents that run through the shared chain, not to
    one bias gradient that happens to cancel over the batch."""
    d, B = 5, 6
    flow = _flow(kind, d, c, [19], seed=7 + c + nb_flow, nb_flow=nb_flow)
    z, ctx, w = _inputs(B, d, c, 40 + c + nb_flow)
    z.requires_grad_(True)
    if ctx is not None:
        ctx.requires_grad_(True)
    x = flow.rsample(z, ctx)
    zz, ld = flow(x, ctx)
    ((w * x).sum() + flow.loss(zz, ld)).backward()
    names = [n for n, _ in flow.named_parameters()]
    got = {"z": z.grad, **({"c": ctx.grad} if c else {}), **{n: p.grad for n, p in flow.named_parameters()}}

    def reference(dtype):
        P = leaves(flow, dtype)
        zl = z.detach().cpu().to(dtype).requires_grad_(True)
        cl = ctx.detach().cpu().to(dtype).requires_grad_(True) if c else torch.zeros(B, 0, dtype=dtype)
        wrt = [zl] + ([cl] if c else []) + [P[n] for n in names]
        L = elbo_like(flow, P, zl, cl, w.detach().cpu().to(dtype))
        grads = torch.autograd.grad(L, wrt, allow_unused=True)
        grads = [torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, wrt)]
        return dict(zip(["z"] + (["c"] if c else []) + names, grads))

    r64, r32 = reference(torch.float64), reference(torch.float32)
    scale_p = max(r64[n].abs().max().item() for n in names)
    for name, want in r64.items():
        assert got[name] is not None, name
        scale = want.abs().max().item() if name in ("z", "c") else scale_p
        _rule("whole gradients, rsample + forward vs plain-torch fp32, both against fp64",
              "%s c=%d nb_flow=%d %s" % (kind, c, nb_flow, name), (c64(got[name]) - want).abs().max().item(),
              (r32[name].double() - want).abs().max().item(), scale)


# --------------------------------------------------------------------- Monotonic + MADE, a deterministic-gate DAG step
def _identity_residuals(step_fn, P, x, ctx, w):
    """plain torch: y = S(x(z)) with x(z) by the implicit function theorem gives dsum(w y)/dz = lambda, J^T lambda = J^T w,
    and d/dtheta = (dS/dtheta)^T w - (dS/dtheta)^T lambda.  -> (max|lambda - w|, max over the leaves of |d/dtheta|)"""
    B = x.shape[0]
    lam = []
    for b in range(B):
        cb = None if ctx is None else ctx[b:b + 1]
        J = torch.autograd.functional.jacobian(lambda v: step_fn(v[None], cb)[0], x[b])
        lam.append(torch.linalg.solve(J.t(), J.t() @ w[b]))
    lam = torch.stack(lam)
    z = step_fn(x, ctx)
    ps = list(P.values())
    ga = torch.autograd.grad(z, ps, w, retain_graph=True, allow_unused=True)
    gb = torch.autograd.grad(z, ps, lam, allow_unused=True)
    res = max([(a - b).abs().max().item() for a, b in zip(ga, gb) if a is not None] or [0.])
    return (lam - w).abs().max().item(), res


def _hip_identity(step, z, ctx, w):
    z = z.detach().requires_grad_(True)
    for p in step.parameters():
        p.grad = None
    y, _ = step(step.rsample(z, ctx), ctx)
    (w * y).sum().backward()
    res = max(p.grad.abs().max().item() for p in step.parameters() if p.grad is not None)
    return (z.grad - w).abs().max().item(), res


def test_monotonic_made_arms_against_the_law_and_the_identity():
    d, c, B = 5, 2, 8
    step = _flow("made", d, c, [19], seed=21, out=4, integrand=[16, 16]).steps[0]
    cond, norm = step.conditioner, step.normalizer
    z, ctx, w = _inputs(B, d, c, 9)
    x = step.invert(z, ctx)
    g = cu(torch.randn(B, d, generator=torch.Generator().manual_seed(4)))
    # the operands both arms share
    with torch.enable_grad():
        h = cond(x.detach().requires_grad_(True), ctx)
        zz, jac = norm(x, h, ctx)
        dzdh, = torch.autograd.grad(zz, h, torch.ones_like(zz))
    jac, dzdh = jac.detach().contiguous(), dzdh.contiguous()
    law = _law64(cond, c, x, ctx, g, jac, dzdh)
    step.adjoint_schedule = True
    lam_a, _, _ = step._rsample_backward(x, ctx, [], g, False)
    assert step._rsample_arm == ("adjoint", 0)
    step.adjoint_schedule = False
    lam_p, _, _ = step._rsample_backward(x, ctx, [], g, False)
    assert step._rsample_arm[0] == "passes"
    _rule("adjoint kernel vs passes, both against the fp64 law", "monotonic d=5 c=2",
          (c64(lam_a) - law).abs().max().item(), (c64(lam_p) - law).abs().max().item(), law.abs().max().item())
    # forward(rsample(z)) = z
    P = leaves(step, torch.float32)
    layers = _pairs(P, "normalizer.integrand_net.")
    S = int(norm.nb_steps)
    fn = lambda v, cb: O.monotonic_forward(v, made_t(cond, P, v, cb, "conditioner."), layers, S)[0]
    tz, tp = _identity_residuals(fn, P, x.detach().cpu(), ctx.cpu(), w.cpu())
    wmax = w.abs().max().item()
    for flag in (True, False):
        step.adjoint_schedule = flag
        hz, hp = _hip_identity(step, z, ctx, w)
        arm = "adjoint" if flag else "passes"
        assert step._rsample_arm[0] == arm
        _rule("identity forward(rsample(z)) = z, residual vs plain-torch fp32", "monotonic %s d/dz" % arm, hz, tz, wmax)
        _rule("identity forward(rsample(z)) = z, residual vs plain-torch fp32", "monotonic %s d/dtheta" % arm, hp, tp, wmax)


def test_deterministic_gate_dag_step_identity():
    d, B = 6, 8
    step = _dag_step(d)
    cond = step.conditioner
    assert cond.deterministic_importance() is not None and cond.depth() >= 2
    z, _, w = _inputs(B, d, 0, 12)
    x = step.invert(z)
    P = leaves(step, torch.float32)
    layers = _pairs(P, "conditioner.embedding_net.")

    def fn(v, cb):
        e = O.dag_masked_inputs(v, P["conditioner.A"], bool(cond.s_thresh), 0., False, False, 1., None, None, None, True)
        return O.affine_forward(v, O.mlp(e, layers).view(v.shape[0], d, -1))[0]

    tz, tp = _identity_residuals(fn, P, x.detach().cpu(), None, w.cpu())
    hz, hp = _hip_identity(step, z, None, w)
    assert step._rsample_arm[0] == "passes" and 1 <= step._rsample_arm[1] <= cond.depth()
    wmax = w.abs().max().item()
    _rule("identity forward(rsample(z)) = z, residual vs plain-torch fp32", "dag passes d/dz", hz, tz, wmax)
    _rule("identity forward(rsample(z)) = z, residual vs plain-torch fp32", "dag passes d/dtheta", hp, tp, wmax)


# ------------------------------------------------------------------------------------------------ refusals and edges
def test_a_stochastic_dag_gate_is_refused():
    step = _dag_step()
    step.conditioner.stoch_gate = True
    step.conditioner.invalidate_caches()
    with pytest.raises(ValueError, match="stochastic"):
        step.rsample(cu(torch.randn(3, 6)))


def test_the_image_flow_refuses():
    from models.NormalizingFlow import CNNormalizingFlow
    with pytest.raises(NotImplementedError):
        CNNormalizingFlow([], None, []).rsample(cu(torch.randn(2, 4)))


@pytest.mark.parametrize("kind", ["made", "coupling"])
def test_a_bad_context_raises_what_invert_raises(kind):
    flow = _flow(kind, 5, 2, [16])
    z, ctx, _ = _inputs(6, 5, 2, 5)
    for bad in ((ctx[:, :1],), (), (ctx[:-1],), (ctx.unsqueeze(2),)):
        with pytest.raises(ValueError):
            flow.invert(z, *bad)
        with pytest.raises(ValueError):
            flow.rsample(z, *bad)
        with pytest.raises(ValueError):
            flow.steps[0].rsample(z, *bad)


def test_empty_batch():
    flow = _flow("made", 5, 2, [19])
    z = torch.zeros(0, 5, device=DEV, requires_grad=True)
    x = flow.rsample(z, torch.zeros(0, 2, device=DEV))
    assert tuple(x.shape) == (0, 5)
    x.sum().backward()
    assert tuple(z.grad.shape) == (0, 5)


def test_only_the_parameters_require_grad():
    flow = _flow("made", 5, 2, [19], seed=8)
    z, ctx, w = _inputs(7, 5, 2, 6)
    grads = []
    for need_z in (False, True):
        for p in flow.parameters():
            p.grad = None
        zl = z.clone().requires_grad_(need_z)
        (w * flow.rsample(zl, ctx)).sum().backward()
        assert (zl.grad is not None) == need_z
        grads.append([p.grad.clone() for p in flow.parameters()])
    assert all(torch.isfinite(a).all() and a.abs().max() > 0 for a in grads[0][-2:])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
