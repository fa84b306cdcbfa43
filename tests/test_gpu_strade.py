"""GPU: StrADEConditioner (a masked net over a given DAG) and its level-sweep kernel gnf_strade_levels.

References are fp64 torch on the CPU, restated from the module's own parameters, mask buffers and adjacency.  Tolerances: the
forward and backward ones of the MADE tests of tests/test_gpu_parity.py (1e-5 / 1e-4); for the inversions the rule of
tests/test_gpu_context_invert.py, err <= 2 err_passes + 1e-6 max|x|, both measured against fp64.  As there, the nets are
as initialised: the rule compares two fp32 summation orders and presumes a well-conditioned inversion.  With every parameter
doubled the Spline steps are not (the fp64 residual of forward(invert(z)) reaches 1e-3 in BOTH arms, bins narrow and steep),
and which arm is closer is then the luck of the draw: in that state one of 279 comparisons stood at 1.18 of the bound (the
residual of chain5 / no hidden layer / Spline / c = 3 / B = 17: 2.33e-5 against 7.92e-6 for the passes), every other below 0.91.

Shapes: the smallest that reach every branch of the kernel -- d = 1; 2; a chain of 5 (one variable per level); 17 with a level
of 9 variables and the others of fewer than 8 (with Affine, out = 2, the output products cross n >= 8 and n < 8, with hidden
[40, 24] the hidden ones do); one graph whose widest level is 2 chunks + 3 variables (the chunk loop with a ragged tail)."""
import ctypes

import numpy as np
import pytest
import torch

import misaligned
import poison
import spline_ref as S
from conftest import assert_close, assert_fwd, rel_err
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, GTOL = 1e-5, 1e-4          # tests/test_gpu_parity.py, MADE forward / backward
KS, TS = 8, 3.
CHUNK = 8                       # GNF_STRADE_CHUNK_VARS (asserted below)
BS = [1, 3, 16, 17, 100]


def cu(t):
    return t.to(DEV)


def c64(t):
    return t.detach().cpu().double()


# ------------------------------------------------------------------------------------------------------------ graphs
def _layered(sizes, seed, max_parents=3):
    """a DAG whose level t holds sizes[t] variables: every variable of level t > 0 has a parent in level t - 1 and parents
    among the first `max_parents` variables of the levels below (few distinct parent sets), under a random relabelling"""
    rng = np.random.RandomState(seed)
    d = sum(sizes)
    a = np.zeros((d, d), dtype=np.uint8)
    start = np.concatenate([[0], np.cumsum(sizes)])
    for t in range(1, len(sizes)):
        prev = np.arange(start[t - 1], start[t])[:max_parents]
        older = np.arange(0, start[t - 1])[:max_parents]
        for i in range(start[t], start[t + 1]):
            a[i, rng.choice(prev)] = 1
            for j in older:
                if rng.rand() < .4:
                    a[i, j] = 1
    perm = rng.permutation(d)
    out = np.zeros_like(a)
    out[np.ix_(perm, perm)] = a
    return out


def _d17():
    """levels of 3, 9 and 5 variables; the 9 take the seven non-empty subsets of the roots as parent sets, the 5 share two
    sets: R = 9, so a layer of 40 units computes >= 8 units at every level and a layer of 24 computes 5 - 6 at the last"""
    a = np.zeros((17, 17), dtype=np.uint8)
    for k in range(9):
        for j in range(3):
            if (k % 7 + 1) >> j & 1:
                a[3 + k, j] = 1
    for k in range(5):
        a[12 + k, [3, 0] if k % 2 == 0 else [4, 5]] = 1
    perm = np.random.RandomState(1).permutation(17)
    out = np.zeros_like(a)
    out[np.ix_(perm, perm)] = a
    return out


GRAPHS = {
    "d1": np.zeros((1, 1), dtype=np.uint8),
    "d2": np.array([[0, 0], [1, 0]], dtype=np.uint8),
    "chain5": np.eye(5, k=-1, dtype=np.uint8),
    "d17": _d17(),
    "wide": _layered([2, 2 * CHUNK + 3, 2], 2),
}


def _hidden(name, kind, c):
    from models.Conditionners.StrADEConditioner import strade_sets
    if kind == "none":
        return []
    return [max(strade_sets(GRAPHS[name], c)[1], 1)] if kind == "R" else [40, 24]


def _flow(name, kind, norm, c, seed=0, scale=1.):
    from models import AffineNormalizer, SplineNormalizer, buildFCNormalizingFlow
    a = GRAPHS[name]
    torch.manual_seed(seed)
    out = 2 if norm == "affine" else 3 * KS - 1
    args = {"in_size": a.shape[0], "hidden": _hidden(name, kind, c), "out_size": out, "cond_in": c, "adjacency": a}
    flow = (buildFCNormalizingFlow(1, "StrADE", args, AffineNormalizer, {}) if norm == "affine" else
            buildFCNormalizingFlow(1, "StrADE", args, SplineNormalizer, {"nb_bins": KS, "tail_bound": TS}))
    if scale != 1.:
        with torch.no_grad():
            for p in flow.parameters():
                p.mul_(scale)
    return flow.to(DEV)


def _inputs(B, d, c, seed):
    g = torch.Generator().manual_seed(seed)
    return 1.5 * torch.randn(B, d, generator=g), (torch.randn(B, c, generator=g) if c else None)


def _cond_fn(cond, dtype, ctx, P=None):
    """h [B, d, out] of the conditioner from its own parameters and mask buffers, in `dtype` on the CPU"""
    ls = cond._layers()
    P = P or {id(p): p.detach().cpu().to(dtype) for l in ls for p in (l.weight, l.bias)}
    masks = [l.mask.detach().cpu().to(dtype) for l in ls]
    d = cond.in_size

    def fn(x):
        a = x if ctx is None else torch.cat((ctx.to(dtype), x), 1)
        for k, (l, m) in enumerate(zip(ls, masks)):
            a = a @ (P[id(l.weight)] * m).t() + P[id(l.bias)]
            if k < len(ls) - 1:
                a = torch.relu(a)
        return a.view(x.shape[0], -1, d).permute(0, 2, 1)
    return fn


def _norm_fns(norm):
    if norm == "affine":
        return O.affine_forward, O.affine_inverse
    return (lambda x, h: S.forward(x, h, KS, TS)), (lambda z, h: S.inverse(z, h, KS, TS))


def _passes(z, cfn, inv, depth, idx=(), vals=None):
    x = torch.zeros_like(z)
    if len(idx):
        x[:, list(idx)] = vals
    for _ in range(depth + 1):
        x = inv(z, cfn(x))
        if len(idx):
            x[:, list(idx)] = vals
    return x


def _rule(case, e_test, e_cmp, scale):
    print("%s: err %.3e err_passes %.3e scale %.3e" % (case, e_test, e_cmp, scale))
    assert e_test <= 2. * e_cmp + 1e-6 * scale, (case, e_test, e_cmp, scale)


class _Spy:
    """calls of ops.strade_levels and of the conditioner module while entered"""

    def __init__(self, step):
        self.step, self.sweeps, self.module = step, 0, 0

    def __enter__(self):
        from gnf_hip import ops
        self._ops, self._orig = ops, ops.strade_levels

        def spied(*a, **k):
            self.sweeps += 1
            return self._orig(*a, **k)
        ops.strade_levels = spied
        self._hook = self.step.conditioner.register_forward_hook(lambda *a: setattr(self, "module", self.module + 1))
        return self

    def __exit__(self, *exc):
        self._ops.strade_levels = self._orig
        self._hook.remove()


def test_the_shape_set_is_what_the_docstring_says():
    from gnf_hip import abi
    from models.Conditionners.StrADEConditioner import strade_level_plan
    assert abi.STRADE_CHUNK_VARS == CHUNK
    sizes = lambda n: list(np.bincount(strade_level_plan(GRAPHS[n], [], 2)["level"]))
    assert sizes("chain5") == [1] * 5 and sizes("d17") == [3, 9, 5] and sizes("wide") == [2, 2 * CHUNK + 3, 2]
    plan = strade_level_plan(GRAPHS["d17"], [40, 24], 2, 0)
    news = [np.diff(np.concatenate([[0], o[:-1]])) for o in plan["off"]]
    assert any((n >= 8).any() for n in news) and any(((n > 0) & (n < 8)).any() for n in news)


# ------------------------------------------------------------------------------------- 1. forward and gradients
@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("out", [2, 23])
@pytest.mark.parametrize("kind", ["none", "R", "40-24"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_forward_and_gradients(name, kind, out, c):
    from models import StrADEConditioner
    a = GRAPHS[name]
    d = a.shape[0]
    torch.manual_seed(3)
    cond = StrADEConditioner(d, _hidden(name, kind, c), out, cond_in=c, adjacency=a).to(DEV)
    names = [n for n, _ in cond.named_parameters()]
    for B in BS:
        x, ctx = _inputs(B, d, c, 10 + B)
        w = torch.randn(B, d, out, generator=torch.Generator().manual_seed(B))
        xd, cd = cu(x).requires_grad_(True), (cu(ctx).requires_grad_(True) if c else None)
        for p in cond.parameters():
            p.grad = None
        h = cond(xd, cd)
        assert tuple(h.shape) == (B, d, out) and h.stride() == (out * d, 1, d)
        (h * cu(w)).sum().backward()
        P = {id(p): p.detach().cpu().double().requires_grad_(True) for p in cond.parameters()}
        x64, ctx64 = x.double().requires_grad_(True), (ctx.double().requires_grad_(True) if c else None)
        h64 = _cond_fn(cond, torch.float64, ctx64, P)(x64)
        (h64 * w.double()).sum().backward()
        assert rel_err(h.detach().cpu(), h64.detach()) < TOL
        assert_fwd(h, h64.detach(), what="h B=%d" % B)
        pairs = [("gx", xd.grad, x64.grad)] + ([("gctx", cd.grad, ctx64.grad)] if c else [])
        pairs += [(n, p.grad, P[id(p)].grad) for n, p in zip(names, cond.parameters())]
        for what, got, want in pairs:
            if want.abs().max() == 0:
                assert got is None or float(got.abs().max()) == 0, what
            else:
                assert rel_err(got.cpu(), want) < GTOL, (what, B, rel_err(got.cpu(), want))
        # structural zeros, both ways: x_j moves no output of a non-child, to the bit; the gradient has them too
        if B == 3:
            assert bool((xd.grad.cpu()[:, torch.from_numpy(a.sum(0) == 0)] == 0).all())
            with torch.no_grad():
                base = cond(cu(x), cd)
                for j in range(d):
                    x2 = x.clone()
                    x2[:, j] += 1.7
                    moved = cond(cu(x2), cd)
                    keep = torch.from_numpy(a[:, j] == 0)
                    assert poison.differing(moved[:, keep], base[:, keep]) == 0, j


# ------------------------------------------------------------------------------------------------------- 2. invert
@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("norm", ["affine", "spline"])
@pytest.mark.parametrize("kind", ["none", "R", "40-24"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_invert_level_arm_against_passes_and_fp64(name, kind, norm, c):
    flow = _flow(name, kind, norm, c, seed=5)
    step = flow.steps[0]
    cond = step.conditioner
    d = cond.in_size
    fwd, inv = _norm_fns(norm)
    for B in BS:
        z, ctx = _inputs(B, d, c, 20 + B)
        args = [cu(z)] + ([cu(ctx)] if c else [])
        with _Spy(step) as spy:
            x_fast = step.invert(*args)
        assert (spy.sweeps, spy.module) == (1, 0) and step._fast_arm(*args, *([] if c else [None]))[0] == "strade"
        step.column_schedule = False
        with _Spy(step) as spy:
            x_pass = step.invert(*args)
        step.column_schedule = True
        assert spy.sweeps == 0 and 1 <= spy.module <= cond.depth() + 1
        assert torch.isfinite(x_fast).all()
        cfn = _cond_fn(cond, torch.float64, ctx)
        x64 = _passes(z.double(), cfn, inv, cond.depth())
        case = "%s %s %s c=%d B=%d" % (name, kind, norm, c, B)
        _rule("invert " + case, (c64(x_fast) - x64).abs().max().item(), (c64(x_pass) - x64).abs().max().item(),
              x64.abs().max().item())
        # forward(invert(z)) = z by the residual of an fp64 forward, the passes arm's residual as the comparator
        res = lambda xx: (fwd(c64(xx), cfn(c64(xx)))[0] - z.double()).abs().max().item()
        _rule("forward(invert(z)) " + case, res(x_fast), res(x_pass), z.abs().max().item())
        # an intervention on nothing is invert, to the bit
        x_do = step.intervene(cu(z), [], 0., *args[1:])
        assert step._intervene_arm == "strade" and poison.differing(x_do, x_fast) == 0


def test_a_net_beyond_the_lds_tile_takes_the_passes():
    from models import AffineNormalizer, buildFCNormalizingFlow
    a = GRAPHS["chain5"]
    torch.manual_seed(1)
    flow = buildFCNormalizingFlow(1, "StrADE", {"in_size": 5, "hidden": [12000], "out_size": 2, "adjacency": a},
                                  AffineNormalizer, {}).to(DEV)
    step = flow.steps[0]
    z, _ = _inputs(6, 5, 0, 3)
    assert step._fast_arm(cu(z), None)[0] == "strade"            # the plan is there: the kernel itself declines
    with _Spy(step) as spy:
        x = step.intervene(cu(z), [], 0.)
    assert spy.sweeps == 1 and spy.module >= 1 and step._intervene_arm == "passes"
    step.column_schedule = False
    assert poison.differing(step.invert(cu(z)), x) == 0
    x64 = _passes(z.double(), _cond_fn(step.conditioner, torch.float64, None), O.affine_inverse, 4)
    assert rel_err(x.cpu(), x64) < 1e-4


@pytest.mark.parametrize("norm", ["monotonic", "off"])
def test_other_normalizers_and_the_switch_take_the_passes(norm):
    from models import AffineNormalizer, MonotonicNormalizer, buildFCNormalizingFlow
    a = GRAPHS["d17"]
    torch.manual_seed(2)
    args = {"in_size": 17, "hidden": [40, 24], "out_size": 4, "adjacency": a}
    flow = (buildFCNormalizingFlow(1, "StrADE", args, MonotonicNormalizer, {"integrand_net": [16, 16], "cond_size": 4,
                                                                           "nb_steps": 20, "solver": "CC"})
            if norm == "monotonic" else buildFCNormalizingFlow(1, "StrADE", args, AffineNormalizer, {})).to(DEV)
    step = flow.steps[0]
    step.column_schedule = norm != "off"
    z, _ = _inputs(5, 17, 0, 4)
    assert step._fast_arm(cu(z), None) is None
    with _Spy(step) as spy:
        x = step.intervene(cu(z), [1], .5)
    assert spy.sweeps == 0 and 1 <= spy.module <= 3 and step._intervene_arm == "passes"
    with torch.no_grad():
        zz, _ = flow(x)
    free = [i for i in range(17) if i != 1]
    assert (zz[:, free].cpu() - z[:, free]).abs().max().item() <= 1e-4 * max(1., z.abs().max().item())


# ------------------------------------------------------------------------------- 3. intervene and counterfactual
def _pin_sets(cond):
    level = cond.level_plan()["level_host"]
    d = len(level)
    top = max(level)
    return {"every second": list(range(0, d, 2)), "a level": [i for i in range(d) if level[i] == min(1, top)],
            "all": list(range(d))}


@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("norm", ["affine", "spline"])
@pytest.mark.parametrize("kind", ["none", "R", "40-24"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_intervene_and_counterfactual(name, kind, norm, c):
    flow = _flow(name, kind, norm, c, seed=6)
    step = flow.steps[0]
    cond = step.conditioner
    d = cond.in_size
    fwd, inv = _norm_fns(norm)
    for B in (3, 17):
        z, ctx = _inputs(B, d, c, 30 + B)
        cargs = [cu(ctx)] if c else []
        cfn = _cond_fn(cond, torch.float64, ctx)
        for what, idx in _pin_sets(cond).items():
            vals = torch.randn(B, len(idx), generator=torch.Generator().manual_seed(len(idx)))
            with _Spy(step) as spy:
                x_fast = flow.intervene(cu(z), idx, cu(vals), *cargs)
            assert step._intervene_arm == "strade" and spy.module == 0 and spy.sweeps == (0 if len(idx) == d else 1)
            step.column_schedule = False
            x_pass = flow.intervene(cu(z), idx, cu(vals), *cargs)
            step.column_schedule = True
            assert step._intervene_arm == "passes"
            assert poison.differing(x_fast[:, idx], cu(vals)) == 0 and poison.differing(x_pass[:, idx], cu(vals)) == 0
            x64 = _passes(z.double(), cfn, inv, cond.depth(), idx, vals.double())
            case = "%s %s %s c=%d B=%d do(%s)" % (name, kind, norm, c, B, what)
            _rule("intervene " + case, (c64(x_fast) - x64).abs().max().item(), (c64(x_pass) - x64).abs().max().item(),
                  x64.abs().max().item())
        # counterfactual: abduction on the device, action on the level arm; fp64 does both in fp64
        idx = _pin_sets(cond)["every second"]
        xo = _passes(z.double(), cfn, inv, cond.depth()).float()
        vals = torch.full((B, len(idx)), .25)
        x_cf = flow.counterfactual(cu(xo), idx, .25, *cargs)
        assert step._intervene_arm == "strade" and poison.differing(x_cf[:, idx], cu(vals)) == 0
        step.column_schedule = False
        x_cp = flow.counterfactual(cu(xo), idx, .25, *cargs)
        step.column_schedule = True
        z64 = fwd(xo.double(), cfn(xo.double()))[0]
        x64 = _passes(z64, cfn, inv, cond.depth(), idx, vals.double())
        _rule("counterfactual %s %s %s c=%d B=%d" % (name, kind, norm, c, B), (c64(x_cf) - x64).abs().max().item(),
              (c64(x_cp) - x64).abs().max().item(), x64.abs().max().item())


# ------------------------------------------------------------------------------------------------------ 4. rsample
@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("norm", ["affine", "spline"])
def test_rsample_gradients_against_fp64(norm, c):
    """L = sum w x + loss(forward(x, c)), x = rsample(z, c): the shape of an ELBO.  Gradients for z, c and every parameter
    against fp64 autograd through the unrolled passes; the comparator is the same restatement in fp32 on plain torch, the
    rule and the floors those of tests/test_gpu_rsample.py (1e-6 of the largest entry of z's, c's, the parameters' group)."""
    name, B = "d17", 6
    flow = _flow(name, "40-24", norm, c, seed=8)
    step = flow.steps[0]
    cond = step.conditioner
    d = cond.in_size
    z, ctx = _inputs(B, d, c, 44)
    z = .6 * z
    w = torch.randn(B, d, generator=torch.Generator().manual_seed(1))
    zd, cd = cu(z).requires_grad_(True), (cu(ctx).requires_grad_(True) if c else None)
    x = flow.rsample(zd, cd)
    zz, ld = flow(x, cd)
    ((cu(w) * x).sum() + flow.loss(zz, ld)).backward()
    assert step._rsample_arm[0] == "passes" and 1 <= step._rsample_arm[1] <= cond.depth()
    names = [n for n, _ in cond.named_parameters()]
    got = {"z": zd.grad, **({"c": cd.grad} if c else {}), **{n: p.grad for n, p in cond.named_parameters()}}
    fwd, inv = _norm_fns(norm)

    def reference(dtype):
        P = {id(p): p.detach().cpu().to(dtype).requires_grad_(True) for p in cond.parameters()}
        zl = z.to(dtype).requires_grad_(True)
        cl = ctx.to(dtype).requires_grad_(True) if c else None
        cfn = _cond_fn(cond, dtype, cl, P)
        xx = _passes(zl, cfn, inv, cond.depth())
        z2, jac = fwd(xx, cfn(xx))
        L = (w.to(dtype) * xx).sum() + O.flow_loss(z2, torch.log(jac).sum(1))
        wrt = [zl] + ([cl] if c else []) + [P[id(p)] for p in cond.parameters()]
        grads = torch.autograd.grad(L, wrt, allow_unused=True)
        grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, wrt)]
        return dict(zip(["z"] + (["c"] if c else []) + names, grads))

    r64, r32 = reference(torch.float64), reference(torch.float32)
    scale_p = max(r64[n].abs().max().item() for n in names)
    for n, want in r64.items():
        assert got[n] is not None, n
        _rule("rsample %s c=%d %s" % (norm, c, n), (c64(got[n]) - want).abs().max().item(),
              (r32[n].double() - want).abs().max().item(), want.abs().max().item() if n in ("z", "c") else scale_p)


# --------------------------------------------------------------------------------------------------- 5. log_prob_do
@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("norm", ["affine", "spline"])
def test_log_prob_do_against_the_truncated_factorisation(norm, c):
    name, B = "d17", 17
    flow = _flow(name, "40-24", norm, c, seed=9)
    cond = flow.steps[0].conditioner
    d = cond.in_size
    x, ctx = _inputs(B, d, c, 51)
    fwd, _ = _norm_fns(norm)
    z64, jac64 = fwd(x.double(), _cond_fn(cond, torch.float64, ctx)(x.double()))
    terms = torch.log(jac64) - .5 * (np.log(2 * np.pi) + z64 ** 2)
    for idx in ([], [0, 5, 16], list(range(d))):
        got = flow.log_prob_do(cu(x), idx, *([None, cu(ctx)] if c else []))
        free = [i for i in range(d) if i not in idx]
        want = terms[:, free].sum(1)
        assert_close(got, want, rtol=TOL, atol=1e-6 * max(1., float(terms.abs().sum(1).max())), what="log_prob_do %s" % idx)


# ---------------------------------------------------------------------------------------------- 6. graphed training
@pytest.mark.parametrize("norm", ["affine", "spline"])
def test_graphed_training_step(norm):
    """one dp.train_step on a StrADE flow through GraphedStep equals the eager step: the tolerance of the graphed-step test
    of tests/test_gpu_configs.py, rel_err < 1e-5 on losses and parameters"""
    from gnf_hip import dp
    xs = [cu(_inputs(40, 17, 0, 60 + i)[0]) for i in range(3)]
    fa, fb = _flow("d17", "40-24", norm, 0, seed=12), _flow("d17", "40-24", norm, 0, seed=12)
    assert dp.GraphedStep.graphable(fa)
    sa, sb = dp.FlatState(fa), dp.FlatState(fb)
    for x in xs:
        la = dp.train_step(fa, sa, x, lr=1e-3, graph=False)
    gs = dp.GraphedStep(fb, sb, xs[0], lr=1e-3, warmup=1)
    for x in xs[1:]:
        lb = gs(x)
    torch.cuda.synchronize()
    assert gs.captures == 1 and sb.t == sa.t == 3
    assert rel_err(lb.detach().cpu().reshape(1), la.detach().cpu().reshape(1)) < 1e-5
    for a, b in zip(fb.parameters(), fa.parameters()):
        assert rel_err(a.detach().cpu(), b.detach().cpu()) < 1e-5
    assert fb.steps[0].conditioner.level_plan() is not None      # training moved no mask


# ----------------------------------------------------------------------------------- 7. alignment and poisoning
def _sweep_case(norm, c, name="d17", kind="40-24"):
    step = _flow(name, kind, norm, c, seed=14).steps[0]
    cond = step.conditioner
    z, ctx = _inputs(17, cond.in_size, c, 70)
    mode = {"affine": 1, "spline": 2}[norm]
    return cond, cu(z), (cu(ctx) if c else None), mode, ((KS, TS) if norm == "spline" else None)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("norm", ["affine", "spline"])
def test_dword_aligned_operands(norm, c, k):
    """z, x, the context and every parameter and mask 4 k bytes past a 16-byte boundary (the pack itself must be 16-byte
    aligned and is refused otherwise): the bits of the aligned call, and not a bit outside the arrays"""
    from gnf_hip import abi, ops
    cond, z, ctx, mode, spline = _sweep_case(norm, c)
    plan = cond.level_plan()
    pin = torch.zeros(cond.in_size, dtype=torch.uint8, device=DEV)
    pin[::3] = 1

    def run(k):
        P = lambda t: misaligned.place(t.detach(), k)
        params, masks = [P(p) for p in cond._params()], [P(m) for m in cond._masks()]
        pack = ops.strade_pack(params, masks, plan)
        outs = []
        for table in (None, pin):
            zs, xs = P(z), P(torch.full_like(z, .5))
            kw = {"context": P(ctx)} if c else {}
            assert ops.strade_levels(params, masks, plan, pack, zs, xs, mode, spline=spline, pin=table, **kw) is xs
            torch.cuda.synchronize()
            assert all(misaligned.guards_intact(t) for t in [zs, xs] + list(kw.values()) + params + masks)
            outs += [xs.clone()]
        return [pack.clone()] + outs
    for a, b in zip(run(0), run(k)):
        assert poison.differing(a, b) == 0
    pack = ops.strade_pack(cond._params(), cond._masks(), plan)
    off = torch.empty(pack.numel() + 4, device=DEV)[1:1 + pack.numel()].copy_(pack)
    with pytest.raises(abi.GnfError, match="GNF_EINVAL"):
        ops.strade_levels(cond._params(), cond._masks(), plan, off, z, torch.zeros_like(z), mode, spline=spline,
                          **({"context": ctx} if c else {}))


@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("norm", ["affine", "spline"])
def test_three_arms(norm, c):
    """the pack buffer and every torch.empty of the wrappers filled with zeros, NaNs and huge values: the same bits"""
    def run():
        flow = _flow("wide", "40-24", norm, c, seed=15)
        step = flow.steps[0]
        z, ctx = _inputs(17, step.conditioner.in_size, c, 71)
        cargs = [cu(ctx)] if c else []
        from gnf_hip import ops
        pack = ops.strade_pack(step.conditioner._params(), step.conditioner._masks(), step.conditioner.level_plan())
        return {"pack": pack, "x": step.invert(cu(z), *cargs), "do": step.intervene(cu(z), [0, 3, 4], 1.5, *cargs)}
    poison.three_arms(run)


def test_the_image_holds_exact_zeros_where_the_mask_forbids():
    from gnf_hip import ops
    cond, _, _, _, _ = _sweep_case("affine", 3)
    plan = cond.level_plan()
    with torch.no_grad():
        for l in cond._layers():
            l.weight.copy_(torch.where(l.mask == 0, torch.full_like(l.weight, float("nan")), l.weight))
    pack = ops.strade_pack(cond._params(), cond._masks(), plan)
    assert torch.isfinite(pack).all()
    # first layer of the image: rows by level order, columns [context | variables by level order], pitch 16-aligned
    W0, m0 = cond._layers()[0].weight.detach(), cond._layers()[0].mask
    rows = plan["order"][0].long()
    cols = torch.cat([torch.arange(3, device=DEV), 3 + plan["var_order"].long()])
    want = torch.where(m0 == 0, torch.zeros_like(W0), W0)[rows][:, cols]
    ldw = (want.shape[1] + 15) // 16 * 16
    got = pack[:want.shape[0] * ldw].view(-1, ldw)
    assert poison.differing(got[:, :want.shape[1]].contiguous(), want.contiguous()) == 0
    assert float(got[:, want.shape[1]:].abs().max()) == 0


# ------------------------------------------------------------------------------------------------- 8. argument errors
def test_argument_errors_surface_as_gnf_error():
    from gnf_hip import abi, ops
    cond, z, ctx, mode, _ = _sweep_case("affine", 3)
    plan, params, masks = cond.level_plan(), cond._params(), cond._masks()
    pack = ops.strade_pack(params, masks, plan)
    x = torch.full_like(z, 7.)
    bad = [dict(z=z[:, :5].contiguous()), dict(z=z.t().contiguous().t()), dict(context=None), dict(context=ctx[:, :2].contiguous()),
           dict(context=ctx.double()), dict(pin=torch.zeros(3, dtype=torch.uint8, device=DEV)),
           dict(pin=torch.zeros(17, dtype=torch.int32, device=DEV)), dict(mode=ops.MADE_NORM_NONE), dict(mode=ops.MADE_NORM_SPLINE),
           dict(mode=ops.MADE_NORM_SPLINE, spline=(1, 3.)), dict(mode=ops.MADE_NORM_SPLINE, spline=(8, -1.))]
    for kw in bad:
        a = dict(z=z, context=ctx, mode=mode, spline=None, pin=None)
        a.update(kw)
        with pytest.raises(abi.GnfError):
            ops.strade_levels(params, masks, plan, pack, a["z"], x, a["mode"], context=a["context"], spline=a["spline"], pin=a["pin"])
    with pytest.raises(abi.GnfError):
        ops.strade_levels(params, masks[:-1], plan, pack, z, x, mode, context=ctx)
    with pytest.raises(abi.GnfError):
        ops.strade_pack(params, [m[:, :-1] for m in masks], plan)
    with pytest.raises(abi.GnfError):
        ops.strade_pack([p.cpu() for p in params], masks, plan)
    # GNF_ESHAPE is the wrapper's None: a spline of 8 bins reads 23 outputs, the net has 2
    assert ops.strade_levels(params, masks, plan, pack, z, x, ops.MADE_NORM_SPLINE, context=ctx, spline=(8, 3.)) is None
    torch.cuda.synchronize()
    assert bool((x == 7.).all())                                 # nothing was launched
    # an empty batch launches nothing and answers its shape
    e = torch.zeros(0, 17, device=DEV)
    assert ops.strade_levels(params, masks, plan, pack, e, e.clone(), mode, context=torch.zeros(0, 3, device=DEV)).shape == (0, 17)
    step = _flow("d17", "40-24", "affine", 3).steps[0]
    assert tuple(step.invert(e, torch.zeros(0, 3, device=DEV)).shape) == (0, 17)
    with pytest.raises(ValueError):
        step.invert(z)                                           # a conditional step without its context
    lib = abi.load()
    assert lib.gnf_strade_levels(None, 0, None, None, None, None, 1, 0, ctypes.c_double(0.), None, 4, None) == -1
