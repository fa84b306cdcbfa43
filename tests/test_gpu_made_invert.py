"""Column-by-column inversion of flow steps with a MADE conditioner (NormalizingFlowStep._invert_by_columns on the prefix
kernel of gnf_hip/csrc/gnf_made_prefix.hip) against the reference's d fixed-point passes (NormalizingFlow.py:98-107), which
`step.column_schedule = False` still runs, and against an fp64 inversion on the CPU oracle.

Both schedules are fp32 evaluations of one function in different summation orders, so neither is the other's yardstick:
the Affine cases measure each against fp64 and require err_columns <= 2 err_passes + 1e-6 max|x| (margin 2; the second term
is the element-wise floor of DESIGN.md section 2 and keeps a pass that happens to be exact from failing the comparison).
Set GNF_MADE_PROFILE=<file> to have the worst measured ratio written there."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_RATIOS = []            # (case, err_columns, err_passes, max|x|)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GNF_MADE_PROFILE")
    if path and _RATIOS:
        worst = max(_RATIOS, key=lambda r: r[1] / max(2. * r[2] + 1e-6 * r[3], 1e-300))
        with open(path, "a") as f:
            f.write("column schedule vs passes, both against fp64 (tests/test_gpu_made_invert.py), %d cases\n" % len(_RATIOS))
            f.write("worst err_columns / (2 err_passes + 1e-6 max|x|) = %.3f at %s: err_columns %.3e, err_passes %.3e, "
                    "max|x| %.3e\n" % (worst[1] / (2. * worst[2] + 1e-6 * worst[3]), worst[0], worst[1], worst[2], worst[3]))
            f.write("largest err_columns / err_passes over cases with err_passes > 0: %.3f\n"
                    % max([r[1] / r[2] for r in _RATIOS if r[2] > 0] or [0.]))


def _affine_flow(d, hidden, seed=0, nb_flow=1):
    from models import AutoregressiveConditioner, AffineNormalizer, buildFCNormalizingFlow
    torch.manual_seed(seed)
    flow = buildFCNormalizingFlow(nb_flow, AutoregressiveConditioner, {"in_size": d, "hidden": list(hidden), "out_size": 2},
                                  AffineNormalizer, {})
    return flow.to(DEV)


def _count_calls(step, z):
    calls = []
    hook = step.conditioner.register_forward_hook(lambda *a: calls.append(1))
    try:
        x = step.invert(z)
    finally:
        hook.remove()
    return x, len(calls)


def _fp64_invert(step, z):
    """the reference's inversion in double on the CPU oracle, from the module's own parameters and mask buffers"""
    net = step.conditioner.masked_autoregressive_net
    layers = [(l.weight.detach().cpu().double(), l.bias.detach().cpu().double()) for l in net.masked_layers()]
    masks = [l.mask.detach().cpu().double() for l in net.masked_layers()]
    return O.step_invert(z.detach().cpu().double(), lambda x: O.made_forward(x, layers, masks), O.affine_inverse,
                         z.shape[1] - 1)


def _columns_vs_passes(step, z, case):
    step.column_schedule = True
    x_col, n_col = _count_calls(step, z)
    step.column_schedule = False
    x_pass, n_pass = _count_calls(step, z)
    step.column_schedule = True
    x64 = _fp64_invert(step, z)
    e_col = (x_col.cpu().double() - x64).abs().max().item()
    e_pass = (x_pass.cpu().double() - x64).abs().max().item()
    xmax = x64.abs().max().item()
    print("%s: err_columns %.3e err_passes %.3e max|x| %.3e" % (case, e_col, e_pass, xmax))
    _RATIOS.append((case, e_col, e_pass, xmax))
    assert n_col == 0 and 1 <= n_pass <= z.shape[1], (n_col, n_pass)
    assert torch.isfinite(x_col).all()
    assert e_col <= 2. * e_pass + 1e-6 * xmax, (case, e_col, e_pass, xmax)
    return x_col


def test_column_schedule_is_the_path_taken():
    flow = _affine_flow(5, [19])
    step = flow.steps[0]
    z = (.7 * torch.randn(3, 5)).to(DEV)
    assert step.column_schedule is True
    _, n = _count_calls(step, z)
    assert n == 0                                   # the conditioner module is never called: the prefix kernel evaluates it
    step.column_schedule = False
    _, n = _count_calls(step, z)
    assert n == 5                                   # depth() + 1 passes


@pytest.mark.parametrize("hidden", [[8], [24, 24], [40, 33, 19]], ids=lambda h: "x".join(map(str, h)))
@pytest.mark.parametrize("d", [1, 2, 5, 17])
def test_affine_columns_against_fp64(d, hidden):
    flow = _affine_flow(d, hidden, seed=100 * d + len(hidden))
    step = flow.steps[0]
    for B in (1, 3, 70, 129):
        torch.manual_seed(B)
        z = (.7 * torch.randn(B, d)).to(DEV)
        x = _columns_vs_passes(step, z, "affine d=%d hidden=%s B=%d" % (d, hidden, B))
        with torch.no_grad():
            zz, _ = flow(x)
        assert rel_err(zz.cpu(), z.cpu()) < 1e-4


@pytest.mark.parametrize("d,hidden", [(17, [40, 33, 19]), (3, [40, 33])], ids=["dot", "mfma"])
def test_whole_inversion_in_one_launch_equals_single_steps(d, hidden):
    from gnf_hip import ops
    flow = _affine_flow(d, hidden, seed=3)
    cond = flow.steps[0].conditioner
    plan, params = cond.prefix_plan(), cond._prefix_params()
    assert plan is not None
    pack = ops.made_prefix_pack(params, plan)
    z = (.7 * torch.randn(70, d)).to(DEV)
    x_one = ops.made_prefix_steps(params, plan, pack, z, torch.zeros_like(z), 0, d, ops.MADE_NORM_AFFINE)
    x_steps = torch.zeros_like(z)
    ws = ops.made_prefix_workspace(params, plan, 70)
    for t in range(d):
        ops.made_prefix_steps(params, plan, pack, z, x_steps, t, t + 1, ops.MADE_NORM_AFFINE, ws=ws)
    assert torch.equal(x_one, x_steps)              # same code, same order
    assert torch.equal(x_one, flow.steps[0].invert(z))


def _monotonic_flow(d, hidden, out, integrand):
    from models import AutoregressiveConditioner, MonotonicNormalizer, buildFCNormalizingFlow
    torch.manual_seed(21)
    flow = buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": d, "hidden": hidden, "out_size": out},
                                  MonotonicNormalizer, {"integrand_net": integrand, "cond_size": out, "nb_steps": 20,
                                                        "solver": "CC"})
    return flow.to(DEV)


def test_monotonic_columns_equal_passes():
    """every variable is a 20-step bisection (resolution 1.9e-5) whose quantisation error is amplified from column to
    column, in both schedules alike: the numbers of test_dag_level_schedule_inversion_equals_fixed_point"""
    flow = _monotonic_flow(6, [30, 30], 6, [16, 16])
    step = flow.steps[0]
    z = (.7 * torch.randn(16, 6)).to(DEV)
    x_col, n_col = _count_calls(step, z)
    step.column_schedule = False
    x_pass, n_pass = _count_calls(step, z)
    assert n_col == 0 and 1 <= n_pass <= 6
    print("monotonic columns vs passes: %.3e" % rel_err(x_col.cpu(), x_pass.cpu()))
    assert rel_err(x_col.cpu(), x_pass.cpu()) < 5e-3
    with torch.no_grad():
        zz, _ = flow(x_col)
    assert rel_err(zz.cpu(), z.cpu()) < 2e-3


def test_monotonic_columns_wide_round_trip():
    """the widths of the UCI Monotonic + MADE configuration at the smallest size that reaches the wide integrand kernels
    and the MFMA prefix path (10 new units per step, 30 outputs per variable)"""
    flow = _monotonic_flow(63, [630], 30, [150, 150, 150])
    step = flow.steps[0]
    z = (.7 * torch.randn(4, 63)).to(DEV)
    x, n = _count_calls(step, z)
    assert n == 0 and torch.isfinite(x).all()
    with torch.no_grad():
        zz, _ = flow(x)
    print("wide monotonic round trip: %.3e" % rel_err(zz.cpu(), z.cpu()))
    assert rel_err(zz.cpu(), z.cpu()) < 2e-3


def test_sampled_orderings():
    from models.Conditionners.AutoregressiveConditioner import ConditionnalMADE
    flow = _affine_flow(9, [20, 20], seed=5)
    step = flow.steps[0]
    torch.manual_seed(6)
    step.conditioner.masked_autoregressive_net = ConditionnalMADE(nin=9, cond_in=0, hidden_sizes=[20, 20], nout=18,
                                                                  num_masks=3, random=True).to(DEV)
    net = step.conditioner.masked_autoregressive_net
    z = (.7 * torch.randn(37, 9)).to(DEV)
    orders = []
    for k in range(3):
        net.update_masks()
        orders.append(tuple(int(v) for v in net.m[-1]))
        _columns_vs_passes(step, z, "sampled ordering %d" % k)       # asserts the hook count 0 as well
    assert len(set(orders)) > 1


def test_fallbacks_run_the_passes():
    d = 5
    flow = _affine_flow(d, [19], seed=9)
    step = flow.steps[0]
    layer = step.conditioner.masked_autoregressive_net.masked_layers()[1]
    mask = layer.mask.cpu().numpy().T.copy()
    i, o = np.argwhere(mask > 0)[0]
    mask[i, o] = 0                                  # autoregressive still, but no degree rule
    layer.set_mask(mask)
    assert step.conditioner.prefix_plan() is None
    z = (.7 * torch.randn(3, d)).to(DEV)
    x_on, n_on = _count_calls(step, z)
    step.column_schedule = False
    x_off, n_off = _count_calls(step, z)
    assert torch.equal(x_on, x_off) and n_on == n_off and 1 <= n_on <= d
    step.column_schedule = True
    assert tuple(step.invert(torch.zeros(0, d, device=DEV)).shape) == (0, d)
    ok = _affine_flow(d, [19], seed=9).steps[0]
    assert tuple(ok.invert(torch.zeros(0, d, device=DEV)).shape) == (0, d)


def test_multi_step_round_trip():
    flow = _affine_flow(5, [19], seed=11, nb_flow=3)
    x = torch.randn(7, 5).to(DEV)
    with torch.no_grad():
        z, _ = flow(x)
        calls = []
        hooks = [s.conditioner.register_forward_hook(lambda *a: calls.append(1)) for s in flow.steps]
        xx = flow.invert(z)
        for h in hooks:
            h.remove()
    assert not calls
    assert rel_err(xx.cpu(), x.cpu()) < 1e-4
