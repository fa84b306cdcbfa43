"""GPU: interventional and counterfactual sampling, NormalizingFlowStep.intervene / counterfactual (interventions).

columns arm: the prefix kernel with a pin table (gnf_made_prefix_do, csrc/gnf_made_prefix.hip); levels arm: the level schedule
of the mutilated DAG.  The yardstick of both is the passes arm (`column_schedule = False` / `level_schedule = False`), whose
law tests/test_intervene.py restates in fp64 (law64).  Exact checks carry no tolerance: the pinned columns are the caller's
bits, an empty pin set is invert, and pinning a column to the value the sweep would have produced changes nothing.  The
numerical check is the project's bound for this kernel (tests/test_gpu_context_invert.py): both arms are fp32 evaluations of
one function in different summation orders, each is measured against fp64, and
err_fast <= 2 err_passes + 1e-6 max|x| is required.  Weights as initialised, z = .7 N(0, 1), as there: the fp64 passes
converge (no case is excluded).

Monotonic + MADE: the normalizer's inverse is a 20-step bisection, so every x lies on a lattice of pitch 40 / 2^20 = 3.8e-5
and a comparison that falls the other way in one fp32 arm moves a sample by whole quanta however accurate the conditioner
outputs are.  The inputs are used as drawn.  A case whose columns arm exceeds the fp64 bound is EXCUSED only if every
element beyond it (a) lies in a row whose fp64 bisection is near a tie (tests/test_intervene.py: TIE, a rule on the fp64
reference alone) in a column of that or a lower degree, and (b) is off by at most two quanta: one for its own comparison,
one carried in from a lower degree (the conditioner's gain is below one at the initialisation scale).  Excused cases are at
most 5 % of the cases of each parametrised test and the elements beyond the bound at most 0.5 % of those compared: both
asserted, both counts printed and written to the profile.  The exact checks of these steps -- the launch count and shapes,
the caller's bits, invert's bits below the first pin and for P = {}, and the arms' agreement to the bound of
tests/test_gpu_made_invert.py -- run over the whole grid of the other normalizers; the fp64 bound, whose reference costs
d passes of 20 fp64 quadratures per case, on B in {5, 17}, and at d = 17 on (no context, natural ordering) and (context,
sampled ordering).
Set GNF_INTERVENE_PROFILE=<file> to have the worst measured ratios appended there."""
import ctypes
import itertools
import os

import pytest
import torch

import spline_ref
from conftest import rel_err
from context_ref import d64
from oracle import gnf_oracle as O
from test_intervene import QUANTUM, TIE, bisection_margins64, law64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_BINS, TAIL = 4, 3.
_RATIOS = {"columns": [], "levels": []}            # (case, err_fast, err_passes, max|x|)
_QUANTA = {"cases": 0, "excused": 0, "elements": 0, "beyond": 0}       # the Monotonic cases held to the fp64 bound


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GNF_INTERVENE_PROFILE")
    if not path:
        return
    with open(path, "a") as f:
        for arm, rows in _RATIOS.items():
            if rows:
                w = max(rows, key=lambda r: r[1] / max(2. * r[2] + 1e-6 * r[3], 1e-300))
                f.write("intervene, %s arm vs passes, both against fp64 (tests/test_gpu_intervene.py), %d cases\n"
                        % (arm, len(rows)))
                f.write("worst err_fast / (2 err_passes + 1e-6 max|x|) = %.3f at %s: err_fast %.3e, err_passes %.3e, "
                        "max|x| %.3e\n" % (w[1] / (2. * w[2] + 1e-6 * w[3]), w[0], w[1], w[2], w[3]))
        if _QUANTA["cases"]:
            f.write("Monotonic + MADE on inputs as drawn: %(excused)d of %(cases)d cases excused (whole bisection quanta behind "
                    "a near-tie of the fp64 reference), %(beyond)d of %(elements)d elements beyond the bound\n" % _QUANTA)


def cu(t):
    return t.to(DEV)


# ------------------------------------------------------------------------------------------------------ the steps
def _normalizer(norm):
    from models import AffineNormalizer, MonotonicNormalizer, SplineNormalizer
    if norm == "affine":
        return AffineNormalizer, {}, 2
    if norm == "spline":
        return SplineNormalizer, {"nb_bins": K_BINS, "tail_bound": TAIL}, 3 * K_BINS - 1
    return MonotonicNormalizer, {"integrand_net": [8, 8], "cond_size": 4, "nb_steps": 8, "solver": "CC"}, 4


def _made_step(d, c, hidden, norm, random=False, seed=0, device=None):
    from models import AutoregressiveConditioner, buildFCNormalizingFlow
    from models.Conditionners.AutoregressiveConditioner import ConditionnalMADE
    N, nkw, out = _normalizer(norm)
    torch.manual_seed(seed)
    flow = buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": d, "hidden": list(hidden), "out_size": out,
                                                                 "cond_in": c}, N, nkw)
    if random:
        flow.steps[0].conditioner.masked_autoregressive_net = ConditionnalMADE(
            nin=d, cond_in=c, hidden_sizes=list(hidden), nout=out * d, num_masks=1, random=True)
    return flow.to(device or DEV).steps[0]


def _inverse64(step, norm):
    if norm == "affine":
        return O.affine_inverse
    if norm == "spline":
        return lambda z, h: spline_ref.inverse(z, h, K_BINS, TAIL)
    from models.Conditionners.Conditioner import linear_pairs
    layers = [(d64(W), d64(b)) for W, b in linear_pairs(step.normalizer.integrand_net.net)]
    return lambda z, h: O.monotonic_inverse(z, h, layers, int(step.normalizer.nb_steps))


def _made64(cond, ctx64, layers=None):
    if layers is None:
        layers = [(d64(l.mask) * d64(l.weight), d64(l.bias)) for l in cond.masked_autoregressive_net.masked_layers()]
    return lambda x: O.mlp(torch.cat((ctx64, x), 1), layers).view(x.shape[0], -1, x.shape[1]).permute(0, 2, 1)


def _dag64(cond, ctx64):
    from models.Conditionners.Conditioner import linear_pairs
    layers = [(d64(W), d64(b)) for W, b in linear_pairs(cond.embedding_net.net)]
    A, d = d64(cond.A), cond.in_size

    def fn(x):                                           # deterministic gate, no threshold: the copies are x * A[i]
        e = x.unsqueeze(1) * A.unsqueeze(0)
        if cond.hot_encoding:
            e = torch.cat((e, torch.eye(d, dtype=x.dtype).unsqueeze(0).expand(x.shape[0], -1, -1)), 2)
        rows = torch.cat((e.reshape(-1, e.shape[2]), ctx64.repeat_interleave(d, 0)), 1)
        return O.mlp(rows, layers).view(x.shape[0], d, -1)
    return fn


def _pin_sets(d):
    """by DEGREE (by variable for a DAG): empty, first, last, two consecutive in the middle, every second, all, all but the
    last -- without repetitions at small d"""
    sets = [(), (0,), (d - 1,), tuple(t for t in (d // 2 - 1, d // 2) if 0 <= t < d), tuple(range(0, d, 2)),
            tuple(range(d)), tuple(range(d - 1))]
    out = []
    for s in sets:
        if s not in out:
            out.append(s)
    return out


def _inputs(B, d, c, seed, device=None):
    gen = torch.Generator().manual_seed(seed)
    z = (.7 * torch.randn(B, d, generator=gen)).to(device or DEV)
    ctx = torch.randn(B, c, generator=gen).to(device or DEV) if c else None
    v = torch.randn(B, d, generator=gen).to(device or DEV)
    return z, ctx, v


def _both_arms(step, flag, arm, z, idx, vals, ctx, case):
    """(x_fast, x_passes) of one intervention, the arm taken and the caller's bits checked on both"""
    setattr(step, flag, True)
    x_fast = step.intervene(z, idx, vals, ctx)
    assert step._intervene_arm == arm, (case, step._intervene_arm)
    setattr(step, flag, False)
    x_pass = step.intervene(z, idx, vals, ctx)
    assert step._intervene_arm == "passes"
    setattr(step, flag, True)
    B, S = z.shape[0], len(idx)
    full = vals.expand(B, S) if torch.is_tensor(vals) else torch.full((B, S), float(vals), device=DEV)
    assert torch.equal(x_fast[:, list(idx)], full) and torch.equal(x_pass[:, list(idx)], full), case     # the caller's bits
    assert torch.isfinite(x_fast).all(), case
    return x_fast, x_pass


def _fast_vs_passes(step, flag, arm, z, idx, vals, ctx, cfn64, inv64, depth, case):
    x_fast, x_pass = _both_arms(step, flag, arm, z, idx, vals, ctx, case)
    x64 = law64(d64(z), cfn64, inv64, depth, idx, d64(x_fast[:, list(idx)]))
    e_fast = (d64(x_fast) - x64).abs().max().item()
    e_pass = (d64(x_pass) - x64).abs().max().item()
    xmax = x64.abs().max().item()
    print("%s: err_%s %.3e err_passes %.3e max|x| %.3e" % (case, arm, e_fast, e_pass, xmax))
    _RATIOS[arm].append((case, e_fast, e_pass, xmax))
    assert e_fast <= 2. * e_pass + 1e-6 * xmax, (case, e_fast, e_pass, xmax)
    return x_fast, x_pass


# ------------------------------------------------------------------------------------------------- columns arm
HIDDEN = [[16], [32, 32], []]


@pytest.mark.parametrize("norm", ["affine", "spline"])
@pytest.mark.parametrize("hidden", HIDDEN, ids=lambda h: "x".join(map(str, h)) or "none")
@pytest.mark.parametrize("d", [1, 6, 17])
def test_columns_arm(d, hidden, norm):
    """checks 1 - 5 of the columns arm on Affine / Spline + MADE, one launch each: every tile boundary of TB = 4 / 8 / 16,
    with and without a context, natural and sampled orderings, the seven pin sets by degree"""
    for c in (0, 2):
        for random in ((False, True) if d > 1 else (False,)):    # (the reference's sampled hidden degrees need d >= 2)
            step = _made_step(d, c, hidden, norm, random, seed=100 * d + 10 * c + len(hidden))
            cond = step.conditioner
            var = cond.prefix_plan(with_context=bool(c))["var_host"]
            assert random or var == list(range(d))
            inv64 = _inverse64(step, norm)
            for B in (1, 5, 16, 17, 33):
                z, ctx, v = _inputs(B, d, c, seed=B + d + c)
                cfn64 = _made64(cond, d64(ctx) if c else torch.zeros(B, 0, dtype=torch.float64))
                x0 = step.invert(z, ctx)
                for degs in _pin_sets(d):
                    idx = [var[t] for t in degs]
                    case = "made %s d=%d c=%d hidden=%s random=%s B=%d pins=%s" % (norm, d, c, hidden, random, B, list(degs))
                    x, _ = _fast_vs_passes(step, "column_schedule", "columns", z, idx, v[:, idx], ctx, cfn64, inv64, d - 1,
                                           case)
                    if not degs:
                        assert torch.equal(x, x0), case                              # P = {} is invert, bit for bit
                        continue
                    # columns of degree below the first pinned degree: invert's bits, whatever v
                    below = [var[t] for t in range(min(degs))]
                    assert torch.equal(x[:, below], x0[:, below]), case
                    # broadcast values: the caller's bits again
                    xb = step.intervene(z, torch.tensor(idx), v[0, idx], ctx)
                    assert torch.equal(xb[:, idx], v[0, idx].expand(B, len(idx))) and step._intervene_arm == "columns"
                    assert torch.equal(xb[:1], x[:1]), case                          # row 0 had these very values
                    # self-consistency: pinned to what the sweep would have produced, nothing changes
                    assert torch.equal(step.intervene(z, idx, x0[:, idx], ctx), x0), case


@pytest.mark.parametrize("c", [0, 2])
def test_columns_arm_whole_inversion_through_the_workspace(c, monkeypatch):
    """a tile whose activation rows do not fit the LDS (tests/test_gpu_poison.py: 16 rows of c + 3 + 1024 + 1024 + 512 floats):
    the (0, d) call with pins runs on the workspace form of the kernel"""
    from gnf_hip import ops
    d, hidden, B = 3, [1024, 1024, 512], 20
    made = []
    real = ops.made_prefix_workspace
    monkeypatch.setattr(ops, "made_prefix_workspace", lambda *a, **k: (made.append(1), real(*a, **k))[1])
    step = _made_step(d, c, hidden, "affine", seed=3)
    cond = step.conditioner
    var = cond.prefix_plan(with_context=bool(c))["var_host"]
    assert 16 * 4 * (c + d + sum(hidden)) > 160 * 1024
    z, ctx, v = _inputs(B, d, c, seed=23)
    cfn64 = _made64(cond, d64(ctx) if c else torch.zeros(B, 0, dtype=torch.float64))
    x0 = step.invert(z, ctx)
    for degs in _pin_sets(d):
        idx = [var[t] for t in degs]
        n0 = len(made)
        x, _ = _fast_vs_passes(step, "column_schedule", "columns", z, idx, v[:, idx], ctx, cfn64, O.affine_inverse, d - 1,
                               "made ws form c=%d pins=%s" % (c, list(degs)))
        assert len(made) == n0 + (0 if len(degs) == d else 1), "the whole sweep ran in LDS"
        if degs:
            assert torch.equal(step.intervene(z, idx, x0[:, idx], ctx), x0)
        else:
            assert torch.equal(x, x0)


MAX_QUANTA = 2


def _monotonic_against_fp64(x_fast, x_pass, z, idx, var, cfn64, inv64, layers, nb_steps, case, tally):
    """the fp64 bound on a Monotonic case as drawn; beyond it only whole quanta behind a near-tie (module docstring)"""
    d = z.shape[1]
    x64 = law64(d64(z), cfn64, inv64, d - 1, idx, d64(x_fast[:, list(idx)]))
    e_fast = (d64(x_fast) - x64).abs()
    e_pass = (d64(x_pass) - x64).abs().max().item()
    xmax = x64.abs().max().item()
    bound = 2. * e_pass + 1e-6 * xmax
    beyond = e_fast > bound
    print("%s: err_columns %.3e err_passes %.3e max|x| %.3e, %d elements beyond the bound"
          % (case, e_fast.max().item(), e_pass, xmax, int(beyond.sum())))
    tally["cases"] += 1
    tally["elements"] += e_fast.numel()
    if not bool(beyond.any()):
        _RATIOS["columns"].append((case, e_fast.max().item(), e_pass, xmax))
        return
    near = bisection_margins64(d64(z), cfn64(x64), layers, nb_steps) < TIE
    near[:, list(idx)] = False                           # (a pinned column has no bisection)
    behind = torch.zeros_like(near)
    behind[:, var] = near[:, var].int().cummax(1).values.bool()          # in degree order: a near-tie at that or a lower degree
    assert bool((behind | ~beyond).all()), (case, "beyond the bound without a near-tie", e_fast[beyond & ~behind].max().item())
    assert e_fast[beyond].max().item() <= bound + MAX_QUANTA * QUANTUM * (1. + 1e-6), (case, e_fast[beyond].max().item(), bound)
    tally["excused"] += 1
    tally["beyond"] += int(beyond.sum())


@pytest.mark.parametrize("hidden", HIDDEN, ids=lambda h: "x".join(map(str, h)) or "none")
@pytest.mark.parametrize("d", [1, 6, 17])
def test_columns_arm_monotonic(d, hidden, monkeypatch):
    """Monotonic + MADE: one GNF_MADE_NORM_NONE launch per FREE column (counted on gnf_hip.ops.made_prefix_steps), each
    walking the pinned run in front of it.  The exact checks over the whole grid, the fp64 bound on the subset the module
    docstring names"""
    from gnf_hip import ops
    from models.Conditionners.Conditioner import linear_pairs
    calls = []
    real = ops.made_prefix_steps
    monkeypatch.setattr(ops, "made_prefix_steps", lambda *a, **k: (calls.append((a[5], a[6])), real(*a, **k))[1])
    tally = {"cases": 0, "excused": 0, "elements": 0, "beyond": 0}
    for c in (0, 2):
        for random in ((False, True) if d > 1 else (False,)):    # (the reference's sampled hidden degrees need d >= 2)
            step = _made_step(d, c, hidden, "monotonic", random, seed=7 * d + c)
            var = step.conditioner.prefix_plan(with_context=bool(c))["var_host"]
            inv64 = _inverse64(step, "monotonic")
            layers = [(d64(W), d64(b)) for W, b in linear_pairs(step.normalizer.integrand_net.net)]
            for B in (1, 5, 16, 17, 33):
                z, ctx, v = _inputs(B, d, c, seed=B + d + c)
                fp64 = B in (5, 17) and (d < 17 or (c, random) in ((0, False), (2, True)))
                cfn64 = _made64(step.conditioner, d64(ctx) if c else torch.zeros(B, 0, dtype=torch.float64)) if fp64 else None
                x0 = step.invert(z, ctx)
                for degs in _pin_sets(d):
                    idx = [var[t] for t in degs]
                    case = "made monotonic d=%d c=%d hidden=%s random=%s B=%d pins=%s" % (d, c, hidden, random, B, list(degs))
                    del calls[:]
                    x = step.intervene(z, idx, v[:, idx], ctx)
                    assert step._intervene_arm == "columns" and len(calls) == d - len(degs), (case, calls)
                    assert all(t1 - 1 not in degs and all(t in degs for t in range(t0, t1 - 1)) for t0, t1 in calls), calls
                    x, x_pass = _both_arms(step, "column_schedule", "columns", z, idx, v[:, idx], ctx, case)
                    err = rel_err(x.cpu(), x_pass.cpu())
                    assert err < 5e-3, (case, err)
                    if not degs:
                        assert torch.equal(x, x0), case
                    else:
                        below = [var[t] for t in range(min(degs))]
                        assert torch.equal(x[:, below], x0[:, below]), case
                    if fp64:
                        _monotonic_against_fp64(x, x_pass, z, idx, var, cfn64, inv64, layers, int(step.normalizer.nb_steps),
                                                case, tally)
    print("monotonic d=%d hidden=%s: %d of %d cases excused, %d of %d elements beyond the bound"
          % (d, hidden, tally["excused"], tally["cases"], tally["beyond"], tally["elements"]))
    for k in tally:
        _QUANTA[k] += tally[k]
    assert tally["excused"] <= .05 * tally["cases"] and tally["beyond"] <= .005 * tally["elements"], tally


# ------------------------------------------------------------------------------- the entry point through abi.py
def _operands(d, c, hidden, B, out=2, seed=3):
    from gnf_hip import ops
    step = _made_step(d, c, hidden, "affine", seed=seed)
    cond = step.conditioner
    plan, params = cond.prefix_plan(with_context=bool(c)), [p.detach() for p in cond._prefix_params()]
    pack = ops.made_prefix_pack(params, plan)
    net = ops._made_net(params, plan)
    z, ctx, v = _inputs(B, d, c, seed=B + d)
    return step, plan, params, pack, net, z, ctx, v


def _place(t, k):
    """a copy of t that starts k elements into a larger buffer"""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = buf[k:k + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _pin_table(d, idx, offset=0):
    buf = torch.zeros(d + 8, dtype=torch.uint8, device=DEV)
    pin = buf[offset:offset + d]
    pin[list(idx)] = 1
    return pin


def _do(net, c, ctx, pack, z, x, h, t0, t1, mode, pin, B, ws, bins=0, tail=0.):
    from gnf_hip import abi
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return abi.load().gnf_made_prefix_do(ctypes.byref(net), c, p(ctx), p(pack), p(z), p(x), p(h), t0, t1, mode, bins, tail,
                                         p(pin), B, p(ws), 0 if ws is None else 4 * ws.numel(), abi.stream())


@pytest.mark.parametrize("d,c,hidden", [(17, 3, [40, 33, 19]), (3, 1, [40, 33]), (5, 0, [19])], ids=["dot", "mfma", "c0"])
def test_null_pin_table_is_the_existing_call(d, c, hidden):
    from gnf_hip import ops
    B = 37
    step, plan, params, pack, net, z, ctx, _ = _operands(d, c, hidden, B)
    kw = {"context": ctx} if c else {}
    want = ops.made_prefix_steps(params, plan, pack, z, torch.zeros_like(z), 0, d, ops.MADE_NORM_AFFINE, **kw)
    x = torch.zeros_like(z)
    ws = ops.made_prefix_workspace(params, plan, B)
    assert _do(net, c, ctx, pack, z, x, None, 0, d, ops.MADE_NORM_AFFINE, None, B, ws) == 0
    assert torch.equal(x, want) and torch.equal(x, step.invert(z, ctx))
    # an all-zero table: the pin kernel, the same bits; step by step through the workspace as well
    pin = _pin_table(d, [])
    x1, x2 = torch.zeros_like(z), torch.zeros_like(z)
    assert _do(net, c, ctx, pack, z, x1, None, 0, d, ops.MADE_NORM_AFFINE, pin, B, ws) == 0
    for t in range(d):
        assert _do(net, c, ctx, pack, z, x2, None, t, t + 1, ops.MADE_NORM_AFFINE, pin, B, ws) == 0
    assert torch.equal(x1, want) and torch.equal(x2, want)
    # NONE, single steps, pin = NULL: the h_out of the existing call
    h1, h2 = torch.zeros(B, plan["out"], device=DEV), torch.zeros(B, plan["out"], device=DEV)
    ws2 = ops.made_prefix_workspace(params, plan, B)
    for t in range(d):
        ops.made_prefix_steps(params, plan, pack, None, want, t, t + 1, ops.MADE_NORM_NONE, h_out=h1, ws=ws, **kw)
        assert _do(net, c, ctx, pack, None, want, h2, t, t + 1, ops.MADE_NORM_NONE, None, B, ws2) == 0
        assert torch.equal(h1, h2), t


def test_none_mode_runs_and_refusals():
    """GNF_MADE_NORM_NONE over several steps: allowed behind pinned steps only; h_out of a pinned final step untouched; the
    outputs of the free step behind a pinned run are those of single steps on the same x"""
    from gnf_hip import ops
    d, c, B = 6, 2, 9
    step, plan, params, pack, net, z, ctx, v = _operands(d, c, [16], B, seed=5)
    var = plan["var_host"]
    NONE = ops.MADE_NORM_NONE
    x = step.invert(z, ctx)                                # any full sample: NONE mode reads x, never writes it
    keep = x.clone()
    ws = ops.made_prefix_workspace(params, plan, B)
    ref_ws = ops.made_prefix_workspace(params, plan, B)
    href = []
    for t in range(d):                                     # single steps, no table
        h = torch.zeros(B, plan["out"], device=DEV)
        ops.made_prefix_steps(params, plan, pack, None, x, t, t + 1, NONE, h_out=h, ws=ref_ws, context=ctx)
        href.append(h)
    pin = _pin_table(d, [var[1], var[2], var[5]], offset=1)             # an odd address
    assert pin.data_ptr() % 2 == 1
    h = torch.full((B, plan["out"]), 7.5, device=DEV)
    assert _do(net, c, ctx, pack, None, x, h, 0, 1, NONE, pin, B, ws) == 0 and torch.equal(h, href[0])
    assert _do(net, c, ctx, pack, None, x, h, 1, 4, NONE, pin, B, ws) == 0 and torch.equal(h, href[3])      # run 1, 2 -> 3
    assert _do(net, c, ctx, pack, None, x, h, 4, 5, NONE, pin, B, ws) == 0 and torch.equal(h, href[4])
    h.fill_(7.5)
    assert _do(net, c, ctx, pack, None, x, h, 5, 6, NONE, pin, B, ws) == 0              # a pinned final step
    assert bool((h == 7.5).all()), "h_out of a pinned final step was written"
    assert _do(net, c, ctx, pack, None, x, h, 1, 3, NONE, pin, B, ws) == 0 and bool((h == 7.5).all())   # a run that ends pinned
    assert torch.equal(x, keep)
    # an un-pinned interior step: 0 in (0, 2), 3 in (2, 5), 4 in (3, 6)
    for t0, t1 in ((0, 2), (2, 5), (3, 6), (0, 6)):
        assert _do(net, c, ctx, pack, None, x, h, t0, t1, NONE, pin, B, ws) == -1, (t0, t1)
    assert _do(net, c, ctx, pack, None, x, h, 1, 3, NONE, None, B, ws) == -1            # a run without a table
    assert bool((h == 7.5).all()) and torch.equal(x, keep)
    # B = 0, and no x with rows to compute
    assert _do(net, c, None, None, None, None, None, 0, d, ops.MADE_NORM_AFFINE, pin, 0, None) == 0
    assert _do(net, c, ctx, pack, z, None, None, 0, d, ops.MADE_NORM_AFFINE, pin, B, ws) == -1
    empty = step.intervene(torch.zeros(0, d, device=DEV), [1], 0., torch.zeros(0, c, device=DEV))
    assert tuple(empty.shape) == (0, d)


@pytest.mark.parametrize("d,c,hidden", [(17, 3, [40, 33, 19]), (3, 1, [40, 33])], ids=["dot", "mfma"])
def test_dword_alignment_and_a_byte_aligned_table(d, c, hidden):
    from gnf_hip import ops
    B = 37
    step, plan, params, pack, net, z, ctx, v = _operands(d, c, hidden, B)
    var = plan["var_host"]
    idx = [var[t] for t in range(0, d, 2)]
    ws = ops.made_prefix_workspace(params, plan, B)

    def run(k):
        zz, cc = _place(z, k), _place(ctx, k)
        x = _place(torch.zeros_like(z), k)
        x[:, idx] = v[:, idx]
        pin = _pin_table(d, idx, offset=k)
        assert k == 0 or (zz.data_ptr() % 16 and cc.data_ptr() % 16 and x.data_ptr() % 16 and pin.data_ptr() % 4)
        assert _do(net, c, cc, pack, zz, x, None, 0, d, ops.MADE_NORM_AFFINE, pin, B, None) == 0        # in LDS
        y = _place(torch.zeros_like(z), k)
        y[:, idx] = v[:, idx]
        for t in range(d):
            assert _do(net, c, cc, pack, zz, y, None, t, t + 1, ops.MADE_NORM_AFFINE, pin, B, ws) == 0  # through ws
        assert torch.equal(x, y)
        return x.clone()

    x0 = run(0)
    assert torch.equal(x0, step.intervene(z, idx, v[:, idx], ctx))
    for k in (1, 2, 3):
        assert torch.equal(run(k), x0), k


# --------------------------------------------------------------------------------------------------- levels arm
def _adjacency(graph, d):
    """A[i, j] = 1: j is a parent of i"""
    A = torch.zeros(d, d)
    if graph == "chain":
        A[torch.arange(1, d), torch.arange(d - 1)] = 1.
    elif graph == "fork":                                  # 0 -> everything
        A[1:, 0] = 1.
    elif graph == "collider":                              # everything -> d - 1
        A[d - 1, :d - 1] = 1.
    else:
        gen = torch.Generator().manual_seed(d)
        perm = torch.randperm(d, generator=gen)
        L = torch.tril((torch.rand(d, d, generator=gen) < .3).float(), -1)
        A[perm[:, None], perm[None, :]] = L                # a random DAG at density .3 in a random topological order
    return A


def _dag_step(graph, d, c, norm, seed=0, hot=True):
    from models import DAGConditioner, buildFCNormalizingFlow
    N, nkw, out = _normalizer(norm)
    torch.manual_seed(seed)
    flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [16], "out_size": out, "cond_in": c,
                                                      "hot_encoding": hot}, N, nkw)
    cond = flow.steps[0].conditioner
    with torch.no_grad():
        cond.A.copy_(_adjacency(graph, d))
    cond.stoch_gate = cond.noise_gate = cond.s_thresh = False           # the post-processed state: a frozen 0 / 1 A
    cond.h_thresh = 0.
    cond.A.requires_grad = False
    cond.invalidate_caches()
    return flow.to(DEV).steps[0]


def _descendants(A, idx):
    d = A.shape[0]
    seen, todo = set(idx), list(idx)
    while todo:
        j = todo.pop()
        for i in range(d):
            if A[i, j] != 0 and i not in seen:
                seen.add(i)
                todo.append(i)
    return seen


GRAPHS = ["chain", "fork", "collider", "random"]


@pytest.mark.parametrize("norm", ["affine", "spline"])
@pytest.mark.parametrize("d", [6, 43])
@pytest.mark.parametrize("graph", GRAPHS)
def test_levels_arm(graph, d, norm):
    for c in (0, 2):
        step = _dag_step(graph, d, c, norm, seed=d + c)
        cond = step.conditioner
        assert cond._device_graph() == (d == 43)
        inv64 = _inverse64(step, norm)
        depth = cond.depth()
        pins = _pin_sets(d) if d == 6 else [(), (0,), (d // 2 - 1, d // 2), tuple(range(0, d, 2)), tuple(range(d - 1))]
        for B in (1, 17):
            z, ctx, v = _inputs(B, d, c, seed=B + d + c)
            cfn64 = _dag64(cond, d64(ctx) if c else torch.zeros(B, 0, dtype=torch.float64))
            x0 = step.invert(z, ctx)
            for idx in pins:
                idx = list(idx)
                case = "dag %s %s d=%d c=%d B=%d pins=%s" % (graph, norm, d, c, B, idx if len(idx) < 8 else len(idx))
                x, _ = _fast_vs_passes(step, "level_schedule", "levels", z, idx, v[:, idx], ctx, cfn64, inv64, depth, case)
                if not idx:
                    assert torch.equal(x, x0), case                      # P = {} is invert, bit for bit


def test_level_counts_of_the_mutilated_chain():
    d = 6
    step = _dag_step("chain", d, 0, "affine")
    cond = step.conditioner
    imp = cond.deterministic_importance()
    own = step._levels(imp)
    assert len(own[0]) == d
    levels, _ = step._levels(imp, (0,))
    assert len(levels) == d - 1 and [h for _, h in levels] == [(t,) for t in range(1, d)]      # the root pinned
    levels, _ = step._levels(imp, (3,))
    assert [h for _, h in levels] == [(0,), (1, 4), (2, 5)]                                    # the middle pinned: two chains
    levels, _ = step._levels(imp, (d - 1,))
    assert len(levels) == d - 1
    levels, tables = step._levels(imp, tuple(range(d)))
    assert levels == [] and tables == (None, None)
    assert step._levels(imp, (3,)) is step._levels(imp, (3,))                                  # cached
    for pair in itertools.combinations(range(d), 2):                                           # ... and bounded
        step._levels(imp, pair)
        assert len(step._levels_do) <= step.DO_LEVELS_MAX
    assert step._levels(imp) is own                                                            # ... beside invert's own, kept


@pytest.mark.parametrize("d", [6, 43])
def test_intervene_leaves_inverts_cache_and_graph_alone(d):
    from models.NormalizingFlow import _INV_GRAPHS
    # (without the one-hot: its host scalar keeps a pass of the composed rows from being captured, here as on the parent)
    step = _dag_step("chain", d, 0, "affine", hot=False)
    z, _, v = _inputs(17, d, 0, seed=3)
    xs = [step.invert(z) for _ in range(3)]                 # eager, captured, replayed
    entry = _INV_GRAPHS.get(step)
    assert entry and any(isinstance(e, tuple) for e in entry.values()), "no graph was captured: the test shows nothing"
    imp = step.conditioner.deterministic_importance()
    key, own = step._levels_own                             # invert's schedule: (levels, (all rows, int32 rows)) and its key
    assert step._levels(imp) is own
    graphs = dict(entry)
    # more pinned sets than DO_LEVELS_MAX (all 15 pairs of the first six variables): the mutilated cache overflows and clears
    pins = [[0], [2, 3], []] + [list(p) for p in itertools.combinations(range(6), 2)]
    assert len(pins) > step.DO_LEVELS_MAX + 3
    for idx in pins:
        step.intervene(z, idx, v[:, idx])
        assert step._intervene_arm == "levels" and len(step._levels_do) <= step.DO_LEVELS_MAX
    assert step._levels_own[0] == key and step._levels_own[1] is own and step._levels(imp) is own
    assert _INV_GRAPHS.get(step) == graphs                  # the same entries, none added: no graph for an intervention
    after = [step.invert(z) for _ in range(2)]
    assert all(torch.equal(x, xs[0]) for x in xs + after)


# ----------------------------------------------------------------------------------------------- counterfactual
def _counterfactual_checks(step, x, ctx, idx, free, case):
    """free: the non-descendants of idx.  counterfactual(x, P, x[:, P]) reproduces x -- exactly in P, to twice the inversion's
    own residual elsewhere; under another v the non-descendants stay within that bound and a descendant moves"""
    with torch.no_grad():
        z, _ = step(x, ctx)
    res = (step.invert(z, ctx) - x).abs().max().item()
    same = step.counterfactual(x, idx, x[:, idx], ctx)
    assert torch.equal(same[:, idx], x[:, idx]), case
    err = (same - x).abs().max().item()
    print("%s: residual %.3e, counterfactual(x, P, x_P) - x %.3e" % (case, res, err))
    assert err <= 2. * res, (case, err, res)
    other = step.counterfactual(x, idx, x[:, idx] + 1.5, ctx)
    assert torch.equal(other[:, idx], x[:, idx] + 1.5), case
    if free:
        assert (other[:, free] - x[:, free]).abs().max().item() <= 2. * res, case
    moved = sorted(set(range(x.shape[1])) - set(free) - set(idx))
    if moved:
        assert (other[:, moved] - x[:, moved]).abs().max().item() > 1e3 * max(res, 1e-7), case
    flow_like = step.counterfactual(x, torch.tensor(idx), 0., ctx)
    assert bool((flow_like[:, idx] == 0.).all())


@pytest.mark.parametrize("norm", ["affine", "spline"])
@pytest.mark.parametrize("c", [0, 2])
def test_counterfactual_made(c, norm):
    d, B = 6, 17
    for random in (False, True):
        step = _made_step(d, c, [32, 32], norm, random, seed=11 + c)
        var = step.conditioner.prefix_plan(with_context=bool(c))["var_host"]
        _, ctx, x = _inputs(B, d, c, seed=5)
        for degs in ((0,), (2, 3), (d - 1,)):
            idx = [var[t] for t in degs]
            free = [var[t] for t in range(min(degs))]       # the lower degrees (between and above: descendants or pinned)
            _counterfactual_checks(step, x, ctx, idx, free, "made %s c=%d random=%s degs=%s" % (norm, c, random, degs))
            assert step._intervene_arm == "columns"


@pytest.mark.parametrize("norm", ["affine", "spline"])
@pytest.mark.parametrize("graph", GRAPHS)
def test_counterfactual_dag(graph, norm):
    d, B = 6, 17
    for c in (0, 2):
        step = _dag_step(graph, d, c, norm, seed=13 + c)
        step.graph_invert = False                           # (the residual's invert calls repeat a shape; nothing to capture here)
        A = step.conditioner.A.cpu()
        _, ctx, x = _inputs(B, d, c, seed=6)
        for idx in ([0], [2, 3], [d - 1]):
            free = sorted(set(range(d)) - _descendants(A, idx))
            _counterfactual_checks(step, x, ctx, idx, free, "dag %s %s c=%d pins=%s" % (graph, norm, c, idx))
            assert step._intervene_arm == "levels"


def test_flow_delegates_and_multi_step_refuses():
    from models import AffineNormalizer, AutoregressiveConditioner, buildFCNormalizingFlow
    torch.manual_seed(1)
    flow = buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": 5, "hidden": [16], "out_size": 2},
                                  AffineNormalizer, {}).to(DEV)
    z, _, v = _inputs(7, 5, 0, seed=2)
    assert torch.equal(flow.intervene(z, [1, 3], v[:, [1, 3]]), flow.steps[0].intervene(z, [1, 3], v[:, [1, 3]]))
    assert torch.equal(flow.counterfactual(v, [1], 0.), flow.steps[0].counterfactual(v, [1], 0.))
    two = buildFCNormalizingFlow(2, AutoregressiveConditioner, {"in_size": 5, "hidden": [16], "out_size": 2},
                                 AffineNormalizer, {}).to(DEV)
    with pytest.raises(ValueError, match="ONE-step"):
        two.intervene(z, [1], 0.)


# ---------------------------------------------------------------------------------------------------------- driver
def test_driver_do_sampling_function(tmp_path):
    import numpy as np
    import train_uci
    args = train_uci.parse(["-dataset", "power", "-context_cols", "2", "-conditioner", "Autoregressive", "-emb_net", "20",
                            "20", "2", "-seed", "5", "-sample", "7", "-do", "1=0.5", "3=-2"])
    torch.manual_seed(2)
    model, _, _ = train_uci.build(args, 4)
    model.to(DEV)
    tst = cu(torch.randn(11, 6, generator=torch.Generator().manual_seed(1)))
    said = []
    err, shift = train_uci.sample_do_rows(model, tst, 7, 2, args.seed, str(tmp_path), args.do, said.append)
    out = np.load(os.path.join(str(tmp_path), "samples_do.npy"))
    assert out.shape == (7, 6) and out.dtype == np.float32
    assert np.array_equal(out[:, 4:], tst[:7, 4:].cpu().numpy())
    assert (out[:, 1] == .5).all() and (out[:, 3] == -2.).all()
    z = torch.randn(7, 4, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        zz, _ = model(cu(torch.from_numpy(out[:, :4])), tst[:7, 4:].contiguous())
        base = model.invert(cu(z), tst[:7, 4:].contiguous())
    assert rel_err(zz.cpu()[:, [0, 2]], z[:, [0, 2]]) < 1e-4                    # the Affine round-trip bound, free columns
    assert err < 1e-4 * z.abs().max().item() and len(said) == 2 and "samples_do.npy" in said[0]
    assert np.allclose(shift, (torch.from_numpy(out[:, :4]) - base.cpu()).mean(0).numpy(), atol=1e-6)
    assert shift[0] == 0.                                                       # degree 0 is upstream of both pins
    # a multi-step flow: the model's ValueError
    args2 = train_uci.parse(["-dataset", "power", "-conditioner", "Autoregressive", "-emb_net", "20", "2", "-nb_flow", "2",
                             "-sample", "3", "-do", "1=0"])
    model2, _, _ = train_uci.build(args2, 6)
    with pytest.raises(ValueError, match="ONE-step"):
        train_uci.sample_do_rows(model2.to(DEV), tst, 3, 0, 0, str(tmp_path), args2.do, said.append)
