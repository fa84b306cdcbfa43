"""GPU: NormalizingFlowStep.intervene under poisoned allocations (tests/poison.py, in the manner of tests/test_gpu_poison.py):
every `torch.empty` on its three arms -- the weight image and the workspace of the prefix kernel, the [B, out] buffer the
GNF_MADE_NORM_NONE launches write and the fused Monotonic inverse reads, the level schedule's conditioner rows -- holds zeros,
NaNs and 3.4e38 in turn, and the samples must not change by a bit.  h_out itself is handed over poisoned and must come back
untouched from a pinned final step."""
import pytest
import torch

import poison
from poison import three_arms
from test_gpu_intervene import DEV, _dag_step, _inputs, _made_step, _pin_sets

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("norm", ["affine", "spline", "monotonic"])
@pytest.mark.parametrize("d,c,hidden,B", [(17, 2, [32, 32], 33), (6, 0, [16], 5)], ids=["d17-c2", "d6-c0"])
def test_columns_arm(d, c, hidden, B, norm):
    def fn():
        step = _made_step(d, c, hidden, norm, seed=3)
        var = step.conditioner.prefix_plan(with_context=bool(c))["var_host"]
        z, ctx, v = _inputs(B, d, c, seed=B + d)
        out = {}
        for k, degs in enumerate(_pin_sets(d)):
            idx = [var[t] for t in degs]
            out["x%d" % k] = step.intervene(z, idx, v[:, idx], ctx)
            assert step._intervene_arm == "columns"
        return out
    three_arms(fn)


@pytest.mark.parametrize("c", [0, 2])
def test_columns_arm_in_the_workspace_form(c):
    """16 rows of c + 3 + 1024 + 1024 + 512 floats do not fit the LDS: the (0, d) call with pins reads and writes the
    poisoned workspace"""
    d, hidden, B = 3, [1024, 1024, 512], 20

    def fn():
        step = _made_step(d, c, hidden, "affine", seed=3)
        var = step.conditioner.prefix_plan(with_context=bool(c))["var_host"]
        z, ctx, v = _inputs(B, d, c, seed=23)
        return {"x%d" % k: step.intervene(z, [var[t] for t in degs], v[:, [var[t] for t in degs]], ctx)
                for k, degs in enumerate(_pin_sets(d))}
    three_arms(fn)


@pytest.mark.parametrize("graph,d", [("random", 6), ("chain", 43)])
def test_levels_arm(graph, d):
    def fn():
        step = _dag_step(graph, d, 2, "affine", seed=5)
        z, ctx, v = _inputs(17, d, 2, seed=d)
        out = {}
        for k, idx in enumerate(([], [0], [d // 2 - 1, d // 2], list(range(0, d, 2)))):
            out["x%d" % k] = step.intervene(z, idx, v[:, idx], ctx)
            assert step._intervene_arm == "levels"
        return out
    three_arms(fn)


def test_h_out_of_a_pinned_final_step_keeps_the_pattern():
    """the caller's h_out, a fresh torch.empty holding the arm's pattern, behind launches that end in a pinned step"""
    from gnf_hip import ops
    d, c, B = 6, 2, 9

    def fn():
        step = _made_step(d, c, [16], "affine", seed=5)
        cond = step.conditioner
        plan, params = cond.prefix_plan(with_context=True), cond._prefix_params()
        var = plan["var_host"]
        pack = ops.made_prefix_pack(params, plan)
        z, ctx, v = _inputs(B, d, c, seed=B + d)
        pin = torch.zeros(d, dtype=torch.uint8, device=DEV)
        pin[[var[1], var[2], var[5]]] = 1
        x = v.clone()
        ws = ops.made_prefix_workspace(params, plan, B)
        h = torch.empty(B, plan["out"], device=DEV)
        first = torch.zeros(B, plan["out"], device=DEV)
        ops.made_prefix_steps(params, plan, pack, None, x, 0, 1, ops.MADE_NORM_NONE, h_out=first, ws=ws, context=ctx, pin=pin)
        ops.made_prefix_steps(params, plan, pack, None, x, 1, 3, ops.MADE_NORM_NONE, h_out=h, ws=ws, context=ctx, pin=pin)
        assert poison.holds_pattern(h), "h_out written by a run that ends in a pinned step"
        outs = {"first": first, "x": x}
        for t in (3, 4):                                    # the two free steps behind the run
            outs["h%d" % t] = torch.zeros(B, plan["out"], device=DEV)
            ops.made_prefix_steps(params, plan, pack, None, x, t, t + 1, ops.MADE_NORM_NONE, h_out=outs["h%d" % t], ws=ws,
                                  context=ctx, pin=pin)
        ops.made_prefix_steps(params, plan, pack, None, x, 5, 6, ops.MADE_NORM_NONE, h_out=h, ws=ws, context=ctx, pin=pin)
        assert poison.holds_pattern(h), "h_out written by a pinned final step"
        assert torch.equal(x, v)                            # NONE mode reads x, never writes it
        return outs
    three_arms(fn)
