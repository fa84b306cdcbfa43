"""Host half of the tests of differentiable interventional sampling (NormalizingFlowStep.rsample_do): the law the pinned
adjoint kernels are held to, their ABI, and the refusals that need no GPU.

The law: tests/adjoint_do_ref.py restates the two adjoint sweeps with the pin rule of do(x_P = v) -- lambda_P = 0,
J_FF^T lambda_F = g_F, gdo_P = g_P - (N^T lambda)_P.  Here, in fp64, (lambda, gdo) of the sweeps are compared with
torch.linalg.solve on the assembled MUTILATED Jacobian and g_P - J_FP^T lambda_F (adjoint_do_ref.mutilated_solve), for a
step z[i] = jac[i] x[i] + sum_k dzdh[i, k] h[i, k](x): a normalizer linear in x and h, so that jac and dzdh are free operands
as they are for the kernels.

Tolerance.  Both sides are backward-stable solves of one triangular system, so each is within a small multiple of
eps * cond(J_FF) * max|lambda| of the truth; the dense side adds the roundoff of assembling J by autograd.  The bound asserted
is 64 * eps_fp64 * max(cond(J_FF), 1) * max|reference| per case, with cond the largest 2-norm condition over the case's
samples (1 when nothing is free); for gdo the reference scale is max(max|gdo|, max|g|).  Measured on the CPU while writing
this (the 316 comparisons below): cond(J_FF) between 1.0 and 29.6, worst err / (eps * cond * scale) = 0.81 for lambda and 1.24
for gdo -- a margin of about 50 under the bound, which is there for another BLAS's summation order, not for slack in the law."""
import ctypes
import os
import re

import pytest
import torch

import adjoint_do_ref as D
import strade_adjoint_ref as R
from adjoint_ref import made_layers, plan_of
from context_ref import d64, made64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = torch.finfo(torch.float64).eps
NEW = {"gnf_made_adjoint_do": 16, "gnf_strade_adjoint_do": 16}


def _check(what, h_fn, sweep, order, d, B, gen, out=2):
    x = torch.randn(B, d, generator=gen, dtype=torch.float64)
    g = torch.randn(B, d, generator=gen, dtype=torch.float64)
    jac = .5 + torch.rand(B, d, generator=gen, dtype=torch.float64)
    dzdh = .5 + torch.rand(B, d, out, generator=gen, dtype=torch.float64)
    ran = 0
    for name in D.PATTERNS:
        pos = D.pattern(name, d)
        if pos is None:
            continue
        ran += 1
        pin = D.pin_of(pos, order, d)
        lam, gdo = sweep(x, g, jac, dzdh, pin)
        wl, wg, conds = D.mutilated_solve(h_fn, x, g, jac, dzdh, pin)
        cond = max(conds + [1.])
        # what is specified exactly
        assert torch.equal(lam[:, pin], torch.zeros(B, int(pin.sum()), dtype=torch.float64)), (what, name)
        assert torch.equal(gdo[:, ~pin], torch.zeros(B, int((~pin).sum()), dtype=torch.float64)), (what, name)
        if name == "all":
            assert torch.equal(gdo, g), (what, name)
        if name == "none":
            assert torch.equal(gdo, torch.zeros_like(g)), (what, name)
        for key, got, want in (("lambda", lam, wl), ("gdo", gdo, wg)):
            scale = max(want.abs().max().item(), g.abs().max().item() if key == "gdo" else 0.)
            err = (got - want).abs().max().item()
            ratio = err / (EPS * cond * scale) if scale else 0.
            print("%s %s %s: err %.3e, cond %.3e, err / (eps cond scale) = %.3f" % (what, name, key, err, cond, ratio))
            assert err <= 64. * EPS * cond * scale, (what, name, key, err, cond, scale)
    return ran


def _made_case(cond, d, c, seed, B=3):
    P = {n: d64(p) for n, p in cond.named_parameters()}
    gen = torch.Generator().manual_seed(seed)
    ctx = torch.randn(B, c, generator=gen, dtype=torch.float64)
    plan, layers = plan_of(cond), made_layers(cond)
    return _check("made d=%d c=%d" % (d, c), lambda v, b: made64(cond, P, v, ctx[b:b + 1]),
                  lambda x, g, jac, dzdh, pin: D.law_sweep_do(layers, plan, c, x, ctx, g, jac, dzdh, pin),
                  plan["var_of_step"], d, B, gen)


@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("d,hidden", [(2, [8]), (5, [24, 24]), (17, [40, 33, 19])], ids=["d2", "d5", "d17"])
def test_made_law_with_pins_equals_the_mutilated_solve(d, hidden, c):
    from models import AutoregressiveConditioner
    torch.manual_seed(100 * d + 10 * c + len(hidden))
    cond = AutoregressiveConditioner(d, list(hidden), 2, cond_in=c)
    with torch.no_grad():
        for l in cond.masked_autoregressive_net.masked_layers():
            l.weight.mul_(2.)
    ran = _made_case(cond, d, c, seed=d + c)
    assert ran == {2: 4, 5: 7, 17: 7}[d]


@pytest.mark.parametrize("c", [0, 3])
def test_made_law_with_pins_and_a_sampled_ordering(c):
    from models import AutoregressiveConditioner
    from models.Conditionners.AutoregressiveConditioner import ConditionnalMADE
    d = 9
    torch.manual_seed(6)
    cond = AutoregressiveConditioner(d, [20, 20], 2, cond_in=c)
    cond.masked_autoregressive_net = ConditionnalMADE(nin=d, cond_in=c, hidden_sizes=[20, 20], nout=2 * d, num_masks=3,
                                                      random=True)
    net = cond.masked_autoregressive_net
    net.update_masks()
    assert tuple(int(v) for v in net.m[-1]) != tuple(range(d))
    assert _made_case(cond, d, c, seed=11) == 7


@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", ["d2", "chain5", "d17"])
def test_strade_law_with_pins_equals_the_mutilated_solve(name, kind, c):
    out, B = 2, 3
    cond = R.build_cond(name, kind, c, out, seed=17 + c + out)
    d = cond.in_size
    layers, masks = R.layers_of(cond)
    plan = R.numpy_plan(cond)
    gen = torch.Generator().manual_seed(5 + d + c)
    ctx = torch.randn(B, c, generator=gen, dtype=torch.float64)
    ran = _check("strade %s %s c=%d" % (name, kind, c),
                 lambda v, b: R.masked_forward(layers, masks, v, ctx[b:b + 1])[0],
                 lambda x, g, jac, dzdh, pin: D.law_levels_do(layers, masks, plan, c, x, ctx, g, jac, dzdh, pin),
                 plan["var_order"], d, B, gen)
    assert ran == {2: 4, 5: 7, 17: 7}[d]


def test_the_pinned_law_without_pins_is_the_law():
    """an empty pin set: the sweeps of adjoint_do_ref are those of adjoint_ref / strade_adjoint_ref, bit for bit in fp64"""
    from adjoint_ref import law_sweep
    from models import AutoregressiveConditioner
    torch.manual_seed(3)
    cond = AutoregressiveConditioner(5, [24, 24], 2, cond_in=3)
    gen = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x, ctx, g, jac, dzdh = r(4, 5), r(4, 3), r(4, 5), .5 + r(4, 5).abs(), r(4, 5, 2)
    none = torch.zeros(5, dtype=torch.bool)
    lam, gdo = D.law_sweep_do(made_layers(cond), plan_of(cond), 3, x, ctx, g, jac, dzdh, none)
    assert torch.equal(lam, law_sweep(made_layers(cond), plan_of(cond), 3, x, ctx, g, jac, dzdh)) and not gdo.any()
    sc = R.build_cond("d17", "40-24", 3, 2, seed=5)
    layers, masks = R.layers_of(sc)
    x, ctx, g, jac, dzdh = r(4, 17), r(4, 3), r(4, 17), .5 + r(4, 17).abs(), r(4, 17, 2)
    lam, gdo = D.law_levels_do(layers, masks, R.numpy_plan(sc), 3, x, ctx, g, jac, dzdh, torch.zeros(17, dtype=torch.bool))
    assert torch.equal(lam, R.law_levels(layers, masks, R.numpy_plan(sc), 3, x, ctx, g, jac, dzdh)) and not gdo.any()


def test_intervene_restatement_pins_and_solves():
    """adjoint_do_ref.intervene_t: pinned columns hold the values exactly, free columns solve their equations"""
    from adjoint_ref import leaves, made_t
    from models import AutoregressiveConditioner
    from oracle import gnf_oracle as O
    d, c, B = 5, 3, 4
    torch.manual_seed(9)
    cond = AutoregressiveConditioner(d, [19], 2, cond_in=c)
    P = leaves(cond, torch.float64)
    gen = torch.Generator().manual_seed(2)
    z, ctx = torch.randn(B, d, generator=gen).double(), torch.randn(B, c, generator=gen).double()
    vals = torch.randn(B, d, generator=gen).double()
    cfn = lambda v: made_t(cond, P, v, ctx)
    for pos in ([], [0, 3], [4], list(range(d))):
        pin = D.pin_of(pos, list(range(d)), d)
        x = D.intervene_t(cfn, d - 1, z, pin, vals)
        assert torch.equal(x[:, pin], vals[:, pin])
        zz, _ = O.affine_forward(x, cfn(x))
        assert (zz - z)[:, ~pin].abs().max().item() <= 1e-12 if len(pos) < d else True


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_symbols_exported_declared_and_bound():
    from gnf_hip import abi
    raw = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = abi.load()                                             # dlopen works without a GPU
    for name, arity in NEW.items():
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES, name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(abi.SIGNATURES[name][1]) == arity, name
    assert abi.ABI_VERSION == 11 and lib.gnf_abi_version() == 11
    assert "#define GNF_ABI_VERSION 11" in raw
    # the workspaces are sized by the existing queries: no new *_ws_bytes / *_workspace_bytes name
    queries = set(re.findall(r"\b(gnf_[a-z0-9_]*(?:_ws_bytes|_workspace_bytes))\s*\(", header))
    assert not [q for q in queries if "_do" in q], queries
    assert {q for q in queries if "adjoint" in q} == {"gnf_made_adjoint_ws_bytes", "gnf_strade_adjoint_workspace_bytes"}


def _made_net():
    from gnf_hip import abi
    net = abi.MadeNet()
    net.nh, net.d, net.out, net.max_new = 1, 5, 2, 1
    net.width[0] = 7
    net.var_of_step, net.off[0] = 64, 64                         # never dereferenced: every call is refused or empty
    return net


def _strade_net():
    from gnf_hip import abi
    net = abi.StradeNet()
    net.made.nh, net.made.d, net.made.out, net.made.max_new = 1, 5, 2, 1
    net.made.width[0] = 7
    net.made.var_of_step, net.made.off[0], net.var_off = 64, 64, 64
    net.nlev, net.widest = 3, 2
    return net


@pytest.mark.parametrize("family", ["made", "strade"])
def test_argument_checks_answer_before_any_launch(family):
    from gnf_hip import abi
    lib = abi.load()
    net = _made_net() if family == "made" else _strade_net()
    fn = getattr(lib, "gnf_%s_adjoint_do" % family)
    ref, p = ctypes.byref(net), ctypes.c_void_p(64)
    EINVAL, EWS = -1, -3
    call = lambda *a: fn(*a, None)
    assert call(ref, 3, None, None, None, None, None, None, None, None, None, 0, 0, None, 0) == 0        # B = 0
    assert call(ref, 3, None, None, None, None, None, None, None, p, p, 0, 0, None, 0) == 0              # B = 0, a table
    assert call(ref, 0, None, p, p, p, p, p, p, None, p, 4, 0, None, 0) == EINVAL                        # gdo without a table
    assert call(ref, 0, None, p, p, p, p, p, p, None, p, 0, 0, None, 0) == EINVAL                        # ... also for B = 0
    assert call(ref, 3, None, p, p, p, p, p, p, p, p, 4, 0, None, 0) == EINVAL                           # no context
    assert call(ref, 0, None, ctypes.c_void_p(68), p, p, p, p, p, p, p, 4, 0, None, 0) == EINVAL         # the pack 4 bytes off
    assert call(ref, 0, None, p, p, p, p, p, p, p, p, -1, 0, None, 0) == EINVAL                          # B < 0
    for k in range(6):                                                                                   # each operand NULL
        ops_ = [p] * 6
        ops_[k] = None
        assert call(ref, 0, None, *ops_, p, None, 4, 0, None, 0) == EINVAL, k
    # the workspace is that of the un-pinned entry point
    assert call(ref, 0, None, p, p, p, p, p, p, p, p, 4, 1, None, 0) == EWS
    need = (lib.gnf_made_adjoint_ws_bytes if family == "made" else lib.gnf_strade_adjoint_workspace_bytes)(ref, 0, 4)
    assert need > 0 and call(ref, 0, None, p, p, p, p, p, p, p, None, 4, 1, p, need - 4) == EWS


# ------------------------------------------------------------------------------------------------------- refusals
def _made_flow(nb_flow=1, d=4):
    from models import AffineNormalizer, AutoregressiveConditioner, buildFCNormalizingFlow
    torch.manual_seed(0)
    return buildFCNormalizingFlow(nb_flow, AutoregressiveConditioner, {"in_size": d, "hidden": [8], "out_size": 2},
                                  AffineNormalizer, {})


def test_a_stochastic_gate_is_refused():
    from models import AffineNormalizer, DAGConditioner, buildFCNormalizingFlow
    flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": 4, "hidden": [8], "out_size": 2}, AffineNormalizer, {})
    assert flow.steps[0].conditioner.deterministic_importance() is None
    for fn in (flow.steps[0].rsample_do, flow.steps[0].rcounterfactual, flow.rsample_do, flow.rcounterfactual):
        with pytest.raises(ValueError, match="stochastic"):
            fn(torch.zeros(2, 4), [1], 0.)


def test_several_steps_and_the_image_flow_are_refused():
    from models.NormalizingFlow import CNNormalizingFlow
    flow = _made_flow(nb_flow=2)
    for fn in (flow.rsample_do, flow.rcounterfactual):
        with pytest.raises(ValueError, match="ONE-step flow.*2 steps"):
            fn(torch.zeros(2, 4), [1], 0.)
    img = CNNormalizingFlow([], None, [])
    for fn, name in ((img.rsample_do, "rsample_do"), (img.rcounterfactual, "rcounterfactual")):
        with pytest.raises(ValueError, match="CNNormalizingFlow.%s.*multi-scale" % name):
            fn(torch.zeros(2, 4), [1], 0.)


@pytest.mark.parametrize("method", ["rsample_do", "rcounterfactual"])
def test_bad_arguments_raise_what_intervene_raises(method):
    flow = _made_flow()
    z = torch.zeros(3, 4)
    bad = [([4], 0.), ([-1], 0.), ([1, 1], 0.), ([1.5], 0.), (torch.tensor([True, False, False, False]), 0.),
           ([1], "x"), ([1, 2], torch.zeros(3)), ([1], torch.zeros(2, 1)), ([1], torch.zeros(3, 1, 1))]
    for target in (flow, flow.steps[0]):
        for idx, val in bad:
            with pytest.raises(ValueError) as e_new:
                getattr(target, method)(z, idx, val)
            with pytest.raises(ValueError) as e_old:
                target.intervene(z, idx, val)
            assert str(e_new.value) == str(e_old.value), (idx, val)
        with pytest.raises(ValueError):
            getattr(target, method)(torch.zeros(3), [0], 0.)
