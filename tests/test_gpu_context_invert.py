"""Conditional sampling x ~ p(x | c) on the fast schedules of NormalizingFlowStep.invert: a conditional MADE (cond_in > 0)
column by column on the prefix kernel's gnf_made_prefix_ctx entry points (csrc/gnf_made_prefix.hip), a conditional DAG step
level by level (DAGConditioner.forward_rows with a context), against the reference's fixed-point passes
(NormalizingFlow.py:98-107, `column_schedule = False` / `level_schedule = False`) and against an fp64 inversion on the CPU
oracle (tests/context_ref.py).

The criterion is that of tests/test_gpu_made_invert.py: both schedules are fp32 evaluations of one function in different
summation orders, so each is measured against fp64 and err_fast <= 2 err_passes + 1e-6 max|x| is required (margin 2; the
second term is the element-wise floor of DESIGN.md section 2).  Set GNF_MADE_PROFILE=<file> to have the worst measured ratio
appended there."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_err
from context_ref import d64, dag64, made64
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_RATIOS = []            # (case, err_fast, err_passes, max|x|)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GNF_MADE_PROFILE")
    if path and _RATIOS:
        worst = max(_RATIOS, key=lambda r: r[1] / max(2. * r[2] + 1e-6 * r[3], 1e-300))
        with open(path, "a") as f:
            f.write("conditional invert, fast schedule vs passes, both against fp64 (tests/test_gpu_context_invert.py), "
                    "%d cases\n" % len(_RATIOS))
            f.write("worst err_fast / (2 err_passes + 1e-6 max|x|) = %.3f at %s: err_fast %.3e, err_passes %.3e, "
                    "max|x| %.3e\n" % (worst[1] / (2. * worst[2] + 1e-6 * worst[3]), worst[0], worst[1], worst[2], worst[3]))
            f.write("largest err_fast / err_passes over cases with err_passes > 0: %.3f\n"
                    % max([r[1] / r[2] for r in _RATIOS if r[2] > 0] or [0.]))


def cu(t):
    return t.to(DEV)


def _made_flow(d, c, hidden, seed=0, nb_flow=1):
    from models import AutoregressiveConditioner, AffineNormalizer, buildFCNormalizingFlow
    torch.manual_seed(seed)
    flow = buildFCNormalizingFlow(nb_flow, AutoregressiveConditioner,
                                  {"in_size": d, "hidden": list(hidden), "out_size": 2, "cond_in": c}, AffineNormalizer, {})
    return flow.to(DEV)


def _count_calls(step, z, ctx):
    calls = []
    hook = step.conditioner.register_forward_hook(lambda *a: calls.append(1))
    try:
        x = step.invert(z, ctx)
    finally:
        hook.remove()
    return x, len(calls)


def _made_fp64(step, z, ctx):
    cond = step.conditioner
    P = {n: d64(p) for n, p in cond.named_parameters()}
    c64 = d64(ctx)
    return O.step_invert(d64(z), lambda v: made64(cond, P, v, c64), O.affine_inverse, z.shape[1] - 1)


def _fast_vs_passes(step, z, ctx, case, x64, flag="column_schedule", n_passes=None):
    setattr(step, flag, True)
    x_fast, n_fast = _count_calls(step, z, ctx)
    setattr(step, flag, False)
    x_pass, n_pass = _count_calls(step, z, ctx)
    setattr(step, flag, True)
    e_fast = (x_fast.cpu().double() - x64).abs().max().item()
    e_pass = (x_pass.cpu().double() - x64).abs().max().item()
    xmax = x64.abs().max().item()
    print("%s: err_fast %.3e err_passes %.3e max|x| %.3e" % (case, e_fast, e_pass, xmax))
    _RATIOS.append((case, e_fast, e_pass, xmax))
    assert n_fast == 0 and 1 <= n_pass <= (n_passes or z.shape[1]), (n_fast, n_pass)
    assert torch.isfinite(x_fast).all()
    assert e_fast <= 2. * e_pass + 1e-6 * xmax, (case, e_fast, e_pass, xmax)
    return x_fast


# ------------------------------------------------------------------------------------------------------- path taken
def test_column_schedule_is_the_path_taken_with_a_context():
    flow = _made_flow(5, 2, [19])
    step = flow.steps[0]
    z, ctx = cu(.7 * torch.randn(3, 5)), cu(torch.randn(3, 2))
    assert step.column_schedule is True
    _, n = _count_calls(step, z, ctx)
    assert n == 0                                   # the conditioner module is never called: the prefix kernel evaluates it
    step.column_schedule = False
    _, n = _count_calls(step, z, ctx)
    assert n == 5                                   # depth() + 1 passes


def test_level_schedule_is_the_path_taken_with_a_context():
    from test_gpu_context import _flow
    flow, d, c = _flow("DAG", "affine", 1)          # post-processed, A strictly lower-triangular: depth d - 1
    step = flow.steps[0]
    z, ctx = cu(.7 * torch.randn(3, d)), cu(torch.randn(3, c))
    assert step.level_schedule is True
    _, n = _count_calls(step, z, ctx)
    assert n == 0
    step.level_schedule = False
    _, n = _count_calls(step, z, ctx)
    assert n == step.conditioner.depth() + 1 == d


# --------------------------------------------------------------------------------------------- MADE, Affine, fp64
@pytest.mark.parametrize("hidden", [[], [8], [24, 24], [40, 33, 19]], ids=lambda h: "x".join(map(str, h)) or "none")
@pytest.mark.parametrize("d", [1, 2, 5, 17])
def test_affine_columns_with_a_context_against_fp64(d, hidden):
    for c in (1, 3):
        flow = _made_flow(d, c, hidden, seed=100 * d + 10 * c + len(hidden))
        step = flow.steps[0]
        for B in (1, 3, 70, 129):
            gen = torch.Generator().manual_seed(B + c)
            z, ctx = cu(.7 * torch.randn(B, d, generator=gen)), cu(torch.randn(B, c, generator=gen))
            x = _fast_vs_passes(step, z, ctx, "made d=%d c=%d hidden=%s B=%d" % (d, c, hidden, B), _made_fp64(step, z, ctx))
            with torch.no_grad():
                zz, _ = flow(x, ctx)
            assert rel_err(zz.cpu(), z.cpu()) < 1e-4


@pytest.mark.parametrize("hidden", [[24, 24], []], ids=["hidden", "none"])
def test_context_sensitivity(hidden):
    d, c, B = 5, 2, 9
    flow = _made_flow(d, c, hidden, seed=4)
    step = flow.steps[0]
    gen = torch.Generator().manual_seed(8)
    z, ctx = cu(.7 * torch.randn(B, d, generator=gen)), cu(torch.randn(B, c, generator=gen))
    x1, x2 = step.invert(z, ctx), step.invert(z, ctx + 1.5)
    v0 = step.conditioner.prefix_plan(with_context=True)["var_host"][0]
    for v in range(d):
        if v == v0 and hidden:
            assert torch.equal(x1[:, v], x2[:, v])  # the degree-0 variable's outputs read no hidden unit: the output bias
        else:
            assert not torch.equal(x1[:, v], x2[:, v]), v


@pytest.mark.parametrize("d,c,hidden", [(17, 3, [40, 33, 19]), (3, 1, [40, 33])], ids=["dot", "mfma"])
def test_whole_inversion_in_one_launch_equals_single_steps_with_a_context(d, c, hidden):
    from gnf_hip import ops
    flow = _made_flow(d, c, hidden, seed=3)
    cond = flow.steps[0].conditioner
    plan, params = cond.prefix_plan(with_context=True), cond._prefix_params()
    assert plan is not None and plan["cond_in"] == c
    pack = ops.made_prefix_pack(params, plan)
    z, ctx = cu(.7 * torch.randn(70, d)), cu(torch.randn(70, c))
    x_one = ops.made_prefix_steps(params, plan, pack, z, torch.zeros_like(z), 0, d, ops.MADE_NORM_AFFINE, context=ctx)
    x_steps = torch.zeros_like(z)
    ws = ops.made_prefix_workspace(params, plan, 70)
    for t in range(d):
        ops.made_prefix_steps(params, plan, pack, z, x_steps, t, t + 1, ops.MADE_NORM_AFFINE, ws=ws, context=ctx)
    assert torch.equal(x_one, x_steps)              # same code, same order
    assert torch.equal(x_one, flow.steps[0].invert(z, ctx))
    with pytest.raises(Exception):
        ops.made_prefix_steps(params, plan, pack, z, x_steps, 0, d, ops.MADE_NORM_AFFINE)               # no context
    with pytest.raises(Exception):
        ops.made_prefix_steps(params, plan, pack, z, x_steps, 0, d, ops.MADE_NORM_AFFINE, context=ctx[:-1])         # rows


@pytest.mark.parametrize("d,hidden", [(17, [40, 33, 19]), (3, [40, 33]), (4, [])], ids=["dot", "mfma", "none"])
def test_cond_in_zero_through_the_new_entry_points(d, hidden):
    """gnf_made_prefix_ctx_*(net, 0, NULL, ...) against the entry points without _ctx: the same bits"""
    import ctypes
    from gnf_hip import abi, ops
    from test_gpu_made_invert import _affine_flow
    flow = _affine_flow(d, hidden, seed=3)
    cond = flow.steps[0].conditioner
    plan, params = cond.prefix_plan(), [p.detach() for p in cond._prefix_params()]
    net, lib, st = ops._made_net(params, plan), abi.load(), abi.stream()
    ref = ctypes.byref(net)
    B = 70
    z = cu(.7 * torch.randn(B, d))
    nfl = lib.gnf_made_prefix_ctx_pack_floats(ref, 0)
    assert nfl == lib.gnf_made_prefix_pack_floats(ref)
    pack_old = ops.made_prefix_pack(params, plan)
    pack_new = torch.empty(nfl, device=DEV)
    abi.call("gnf_made_prefix_ctx_pack", ref, 0, abi.ptr(pack_new), st)
    assert torch.equal(pack_old, pack_new)
    x_old = ops.made_prefix_steps(params, plan, pack_old, z, torch.zeros_like(z), 0, d, ops.MADE_NORM_AFFINE)
    nws = lib.gnf_made_prefix_ctx_ws_bytes(ref, 0, B)
    assert nws == lib.gnf_made_prefix_ws_bytes(ref, B)
    ws = torch.empty(nws // 4, device=DEV)
    x_new = torch.zeros_like(z)
    abi.call("gnf_made_prefix_ctx", ref, 0, None, abi.ptr(pack_new), abi.ptr(z), abi.ptr(x_new), None, 0, d,
             ops.MADE_NORM_AFFINE, B, ctypes.c_void_p(ws.data_ptr()), nws, st)
    assert torch.equal(x_old, x_new)
    x_steps = torch.zeros_like(z)
    for t in range(d):
        abi.call("gnf_made_prefix_ctx", ref, 0, None, abi.ptr(pack_new), abi.ptr(z), abi.ptr(x_steps), None, t, t + 1,
                 ops.MADE_NORM_AFFINE, B, ctypes.c_void_p(ws.data_ptr()), nws, st)
    assert torch.equal(x_old, x_steps)


def test_sampled_orderings_with_a_context():
    from models.Conditionners.AutoregressiveConditioner import ConditionnalMADE
    d, c = 9, 2
    flow = _made_flow(d, c, [20, 20], seed=5)
    step = flow.steps[0]
    torch.manual_seed(6)
    step.conditioner.masked_autoregressive_net = ConditionnalMADE(nin=d, cond_in=c, hidden_sizes=[20, 20], nout=2 * d,
                                                                  num_masks=3, random=True).to(DEV)
    net = step.conditioner.masked_autoregressive_net
    z, ctx = cu(.7 * torch.randn(37, d)), cu(torch.randn(37, c))
    orders = []
    for k in range(3):
        net.update_masks()
        orders.append(tuple(int(v) for v in net.m[-1]))
        _fast_vs_passes(step, z, ctx, "sampled ordering %d, c=%d" % (k, c), _made_fp64(step, z, ctx))
    assert len(set(orders)) > 1


# ------------------------------------------------------------------------------------------------- MADE, Monotonic
def _monotonic_flow(d, c, hidden, out, integrand):
    from models import AutoregressiveConditioner, MonotonicNormalizer, buildFCNormalizingFlow
    torch.manual_seed(21)
    flow = buildFCNormalizingFlow(1, AutoregressiveConditioner,
                                  {"in_size": d, "hidden": hidden, "out_size": out, "cond_in": c},
                                  MonotonicNormalizer, {"integrand_net": integrand, "cond_size": out, "nb_steps": 20,
                                                        "solver": "CC"})
    return flow.to(DEV)


def test_monotonic_columns_equal_passes_with_a_context():
    """every variable is a 20-step bisection (resolution 1.9e-5) whose quantisation error is amplified from column to
    column, in both schedules alike: the bounds of test_gpu_made_invert.test_monotonic_columns_equal_passes"""
    flow = _monotonic_flow(6, 2, [30, 30], 6, [16, 16])
    step = flow.steps[0]
    z, ctx = cu(.7 * torch.randn(16, 6)), cu(torch.randn(16, 2))
    x_col, n_col = _count_calls(step, z, ctx)
    step.column_schedule = False
    x_pass, n_pass = _count_calls(step, z, ctx)
    assert n_col == 0 and 1 <= n_pass <= 6
    print("monotonic columns vs passes with a context: %.3e" % rel_err(x_col.cpu(), x_pass.cpu()))
    assert rel_err(x_col.cpu(), x_pass.cpu()) < 5e-3
    with torch.no_grad():
        zz, _ = flow(x_col, ctx)
    assert rel_err(zz.cpu(), z.cpu()) < 2e-3


def test_monotonic_columns_wide_round_trip_with_a_context():
    """the widths of the UCI Monotonic + MADE configuration (the wide integrand kernels, the MFMA prefix path: 10 new units
    per step, 30 outputs per variable) with four context columns"""
    flow = _monotonic_flow(63, 4, [630], 30, [150, 150, 150])
    step = flow.steps[0]
    z, ctx = cu(.7 * torch.randn(4, 63)), cu(torch.randn(4, 4))
    x, n = _count_calls(step, z, ctx)
    assert n == 0 and torch.isfinite(x).all()
    with torch.no_grad():
        zz, _ = flow(x, ctx)
    print("wide monotonic round trip with a context: %.3e" % rel_err(zz.cpu(), z.cpu()))
    assert rel_err(zz.cpu(), z.cpu()) < 2e-3


# ---------------------------------------------------------------------------------------- DAG levels with a context
def _dag_flow(normalizer, hot, bias):
    from models import DAGConditioner, AffineNormalizer, MonotonicNormalizer, buildFCNormalizingFlow
    torch.manual_seed(21)
    d, c = 9, 2
    if normalizer == "affine":
        flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [24, 24], "out_size": 2, "cond_in": c,
                                                          "hot_encoding": hot}, AffineNormalizer, {})
    else:
        flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [24, 24], "out_size": 6, "cond_in": c,
                                                          "hot_encoding": hot},
                                      MonotonicNormalizer, {"integrand_net": [16, 16], "cond_size": 6, "nb_steps": 20,
                                                            "solver": "CC"})
    cond = flow.steps[0].conditioner
    # strictly lower-triangular, non-negative, density .5 (test_gpu_parity.test_dag_level_schedule_inversion_equals_fixed_point)
    cond.A.data.copy_(torch.tril(torch.rand(d, d) + .1, -1) * (torch.rand(d, d) < .5).float())
    cond.stoch_gate = False
    cond.embedding_net.context_bias = bias
    cond.invalidate_caches()
    return flow.to(DEV), d, c


@pytest.mark.parametrize("bias", [False, True], ids=["concat", "context_bias"])
@pytest.mark.parametrize("hot", [True, False], ids=["hot", "plain"])
def test_dag_levels_with_a_context_affine(hot, bias):
    flow, d, c = _dag_flow("affine", hot, bias)
    step = flow.steps[0]
    cond = step.conditioner
    B = 16
    gen = torch.Generator().manual_seed(31)
    z, ctx = cu(.7 * torch.randn(B, d, generator=gen)), cu(torch.randn(B, c, generator=gen))
    P = {n: d64(p) for n, p in cond.named_parameters()}
    one, c64 = torch.ones(B, d, d), d64(ctx)
    depth = cond.depth()
    assert depth >= 2
    x64 = O.step_invert(d64(z), lambda v: dag64(cond, P, "det", v, c64, one, one), O.affine_inverse, depth)
    x = _fast_vs_passes(step, z, ctx, "dag d=%d c=%d hot=%s context_bias=%s" % (d, c, hot, bias), x64,
                        flag="level_schedule", n_passes=depth + 1)
    with torch.no_grad():
        zz, _ = flow(x, ctx)
    assert rel_err(zz.cpu(), z.cpu()) < 1e-4
    # a second sample with another context: another x (a FROZEN A, where a pass could be captured, is the test below)
    x2 = step.invert(z, ctx + 1.)
    x3 = step.invert(z, ctx + 1.)
    assert not torch.equal(x2, x) and torch.equal(x2, x3)


@pytest.mark.parametrize("bias", [False, True], ids=["concat", "context_bias"])
@pytest.mark.parametrize("hot", [True, False], ids=["hot", "plain"])
def test_frozen_dag_sampled_repeatedly_captures_no_graph(hot, bias):
    """the state train_uci.py -sample meets after post-processing: A frozen and 0/1, the importance matrix IS A, nine levels --
    everything an unconditional pass needs to be captured on its second call and replayed from the third.  A pass with a
    context must not be: a replay would read the context of the call that was captured.  Four calls of one shape with four
    contexts, each held to the fp64 criterion of its own context."""
    from models.NormalizingFlow import _INV_GRAPHS
    flow, d, c = _dag_flow("affine", hot, bias)
    step = flow.steps[0]
    cond = step.conditioner
    with torch.no_grad():
        cond.A.diagonal(-1).fill_(1.)               # a chain through every variable: depth d - 1 whatever the draw
    cond.post_process()
    assert not cond.A.requires_grad and cond.depth() == d - 1
    importance = cond.deterministic_importance()
    assert importance.data_ptr() == cond.A.data_ptr() and step.graph_invert and len(step._levels(importance)[0]) == d > 4
    B = 16
    gen = torch.Generator().manual_seed(33)
    z = cu(.7 * torch.randn(B, d, generator=gen))
    P = {n: d64(p) for n, p in cond.named_parameters()}
    one, xs = torch.ones(B, d, d), []
    for k in range(4):
        ctx = cu(torch.randn(B, c, generator=gen))
        c64 = d64(ctx)
        x64 = O.step_invert(d64(z), lambda v: dag64(cond, P, "det", v, c64, one, one), O.affine_inverse, d - 1)
        xs.append(_fast_vs_passes(step, z, ctx, "frozen dag call %d hot=%s context_bias=%s" % (k, hot, bias), x64,
                                  flag="level_schedule", n_passes=d))
        assert not _INV_GRAPHS.get(step), k
    assert all(not torch.equal(xs[0], x) for x in xs[1:])


def test_dag_levels_empty_batch():
    flow, d, c = _dag_flow("affine", True, False)
    x = flow.steps[0].invert(torch.zeros(0, d, device=DEV), torch.zeros(0, c, device=DEV))
    assert tuple(x.shape) == (0, d)
    with pytest.raises(ValueError):
        flow.steps[0].invert(torch.zeros(0, d, device=DEV), torch.zeros(0, c + 1, device=DEV))


@pytest.mark.parametrize("bias", [False, True], ids=["concat", "context_bias"])
@pytest.mark.parametrize("hot", [True, False], ids=["hot", "plain"])
def test_dag_levels_with_a_context_monotonic(hot, bias):
    flow, d, c = _dag_flow("monotonic", hot, bias)
    step = flow.steps[0]
    z, ctx = cu(.7 * torch.randn(16, d)), cu(torch.randn(16, c))
    x_lvl, n_lvl = _count_calls(step, z, ctx)
    step.level_schedule = False
    x_it, n_it = _count_calls(step, z, ctx)
    # (the passes stop early once one changes nothing: the bisection's results are quantised and may repeat exactly)
    assert n_lvl == 0 and 1 <= n_it <= step.conditioner.depth() + 1
    print("monotonic levels vs passes with a context: %.3e" % rel_err(x_lvl.cpu(), x_it.cpu()))
    assert rel_err(x_lvl.cpu(), x_it.cpu()) < 5e-3
    with torch.no_grad():
        zz, _ = flow(x_lvl, ctx)
    assert rel_err(zz.cpu(), z.cpu()) < 2e-3


# --------------------------------------------------------------------------------------------- fallbacks and errors
def test_hand_set_mask_runs_the_passes():
    d, c = 5, 2
    flow = _made_flow(d, c, [19], seed=9)
    step = flow.steps[0]
    layer = step.conditioner.masked_autoregressive_net.masked_layers()[1]
    mask = layer.mask.cpu().numpy().T.copy()
    i, o = np.argwhere(mask > 0)[0]
    mask[i, o] = 0                                  # autoregressive still, but no degree rule
    layer.set_mask(mask)
    assert step.conditioner.prefix_plan(with_context=True) is None
    z, ctx = cu(.7 * torch.randn(3, d)), cu(torch.randn(3, c))
    x_on, n_on = _count_calls(step, z, ctx)
    step.column_schedule = False
    x_off, n_off = _count_calls(step, z, ctx)
    assert torch.equal(x_on, x_off) and n_on == n_off and 1 <= n_on <= d


@pytest.mark.parametrize("kind", ["DAG", "Coupling", "Autoregressive"])
def test_a_bad_context_raises(kind):
    from test_gpu_context import _flow
    flow, d, c = _flow(kind, "affine", 1)
    z, ctx = cu(.7 * torch.randn(6, d)), cu(torch.randn(6, c))
    for bad in ((ctx[:, :1],), (), (ctx[:-1],), (ctx.unsqueeze(2),)):
        with pytest.raises(ValueError):
            flow.invert(z, *bad)
        with pytest.raises(ValueError):
            flow.steps[0].invert(z, *bad)
    assert tuple(flow.invert(z, ctx).shape) == (6, d)


def test_a_context_for_cond_in_zero_still_raises():
    from test_gpu_made_invert import _affine_flow
    flow = _affine_flow(5, [19])
    with pytest.raises(NotImplementedError):
        flow.invert(cu(torch.randn(3, 5)), cu(torch.randn(3, 2)))


def test_empty_batch():
    flow = _made_flow(5, 2, [19], seed=9)
    x = flow.steps[0].invert(torch.zeros(0, 5, device=DEV), torch.zeros(0, 2, device=DEV))
    assert tuple(x.shape) == (0, 5)


# ------------------------------------------------------------------------------------------------------- alignment
def _place(t, k):
    """a copy of t that starts k floats into a larger buffer: 4 k bytes past the allocator's alignment"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("d,c,hidden", [(17, 3, [40, 33, 19]), (3, 1, [40, 33])], ids=["dot", "mfma"])
def test_dword_alignment(d, c, hidden):
    from gnf_hip import ops
    flow = _made_flow(d, c, hidden, seed=3)
    cond = flow.steps[0].conditioner
    plan, params = cond.prefix_plan(with_context=True), cond._prefix_params()
    pack = ops.made_prefix_pack(params, plan)
    B = 70
    z, ctx = cu(.7 * torch.randn(B, d)), cu(torch.randn(B, c))

    def run(k):
        zz, cc = _place(z, k), _place(ctx, k)
        x, h = _place(torch.zeros_like(z), k), _place(torch.zeros(B, plan["out"], device=DEV), k)
        assert k == 0 or (zz.data_ptr() % 16 and cc.data_ptr() % 16 and x.data_ptr() % 16 and h.data_ptr() % 16)
        ops.made_prefix_steps(params, plan, pack, zz, x, 0, d, ops.MADE_NORM_AFFINE, context=cc)
        ws = ops.made_prefix_workspace(params, plan, B)
        hs = []
        for s in range(d):
            ops.made_prefix_steps(params, plan, pack, None, x, s, s + 1, ops.MADE_NORM_NONE, h_out=h, ws=ws, context=cc)
            hs.append(h.clone())
        return x.clone(), torch.stack(hs, 2)

    x0, h0 = run(0)
    assert torch.equal(x0, flow.steps[0].invert(z, ctx))
    for k in (1, 2, 3):
        x, h = run(k)
        assert torch.equal(x, x0) and torch.equal(h, h0), k


# ------------------------------------------------------------------------------------------------------ multi-step
def test_multi_step_round_trip_with_a_context():
    flow = _made_flow(5, 2, [19], seed=11, nb_flow=3)
    x, ctx = cu(torch.randn(7, 5)), cu(torch.randn(7, 2))
    with torch.no_grad():
        z, _ = flow(x, ctx)
        calls = []
        hooks = [s.conditioner.register_forward_hook(lambda *a: calls.append(1)) for s in flow.steps]
        xx = flow.invert(z, ctx)
        for h in hooks:
            h.remove()
    assert not calls
    assert rel_err(xx.cpu(), x.cpu()) < 1e-4


# ---------------------------------------------------------------------------------------------------------- driver
def test_driver_sampling_function(tmp_path):
    import train_uci
    args = train_uci.parse(["-dataset", "power", "-context_cols", "2", "-conditioner", "Autoregressive", "-emb_net", "20",
                            "20", "2", "-seed", "5"])
    torch.manual_seed(2)
    model, _, _ = train_uci.build(args, 4)
    model.to(DEV)
    tst = cu(torch.randn(11, 6, generator=torch.Generator().manual_seed(1)))
    said = []
    err = train_uci.sample_rows(model, tst, 7, 2, args.seed, str(tmp_path), said.append)
    out = np.load(os.path.join(str(tmp_path), "samples.npy"))
    assert out.shape == (7, 6) and out.dtype == np.float32
    assert np.array_equal(out[:, 4:], tst[:7, 4:].cpu().numpy())
    z = torch.randn(7, 4, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        zz, _ = model(cu(torch.from_numpy(out[:, :4])), tst[:7, 4:].contiguous())
    assert rel_err(zz.cpu(), z) < 1e-4              # the Affine round-trip bound
    assert err < 1e-4 * z.abs().max().item() and len(said) == 1 and "samples.npy" in said[0]
