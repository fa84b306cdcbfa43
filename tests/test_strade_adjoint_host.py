"""Host half of the StrADE adjoint level sweep's tests (csrc/gnf_strade_adjoint.hip): the law the kernel is held to, its ABI
and the precondition on the GPU grid's inputs.

The law: tests/strade_adjoint_ref.py:law_levels restates the transposed level sweep from the tables of strade_level_plan.
Here, in fp64, it is compared with torch.linalg.solve(J^T, g) on the Jacobian of the step
z[i] = jac[i] x[i] + sum_k dzdh[i, k] h[i, k](x) -- a normalizer that is linear in x and h, so that jac and dzdh are free
operands as they are for the kernel -- assembled sample by sample by autograd from the DENSE masked net.  Both are exact
solves of one triangular system: 1e-10 of max|lambda|."""
import ctypes
import os
import re

import pytest
import torch

import strade_adjoint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gnf_strade_adjoint_pack_floats", "gnf_strade_adjoint_pack", "gnf_strade_adjoint_workspace_bytes", "gnf_strade_adjoint"]


def _law_case(name, kind, c, out, B=4):
    cond = R.build_cond(name, kind, c, out, seed=17 + c + out)
    d = cond.in_size
    layers, masks = R.layers_of(cond)
    gen = torch.Generator().manual_seed(5 + d + c)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x, ctx, g = r(B, d), r(B, c), r(B, d)
    jac = .5 + torch.rand(B, d, generator=gen, dtype=torch.float64)
    dzdh = .5 + torch.rand(B, d, out, generator=gen, dtype=torch.float64)

    def step(xr, b):
        h, _ = R.masked_forward(layers, masks, xr[None], ctx[b:b + 1])
        return jac[b] * xr + (dzdh[b] * h[0]).sum(1)

    want = torch.stack([torch.linalg.solve(torch.autograd.functional.jacobian(lambda v: step(v, b), x[b]).t(), g[b])
                        for b in range(B)])
    got = R.law_levels(layers, masks, R.numpy_plan(cond), c, x, ctx, g, jac, dzdh)
    err = (got - want).abs().max().item() / want.abs().max().item()
    print("%s %s c=%d out=%d: law_levels vs solve(J^T, g): %.3e of max|lambda|" % (name, kind, c, out, err))
    assert err <= 1e-10, err


@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", list(R.GRAPHS))
def test_law_levels_equals_the_transposed_solve(name, kind, c):
    _law_case(name, kind, c, 2)


def test_law_levels_with_many_outputs():
    _law_case("d17", "40-24", 3, 23)
    _law_case("wide", "R", 0, 23)


def test_the_graphs_are_those_of_the_forward_tests():
    sizes = lambda n: [int(v) for v in torch.bincount(torch.as_tensor(R.numpy_plan(R.build_cond(n, "none", 0, 2, 0))["level"]))]
    assert sizes("d1") == [1] and sizes("d2") == [1, 1] and sizes("chain5") == [1] * 5
    assert sizes("d17") == [3, 9, 5] and sizes("wide") == [2, 2 * R.CHUNK + 3, 2]
    from gnf_hip import abi
    assert abi.STRADE_CHUNK_VARS == R.CHUNK


def test_symbols_exported_declared_and_bound():
    from gnf_hip import abi, build
    header = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = abi.load()                                             # dlopen works without a GPU
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES, name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(abi.SIGNATURES[name][1]), name
    assert abi.ABI_VERSION == 11 and lib.gnf_abi_version() == 11
    assert "#define GNF_ABI_VERSION 11" in header
    assert "gnf_strade_adjoint.hip" in build.SOURCES


def _net(width, nlev=3, widest=2, d=5, out=2):
    from gnf_hip import abi
    net = abi.StradeNet()
    net.made.nh, net.made.d, net.made.out, net.made.max_new = 1, d, out, 1
    net.made.width[0] = width
    # never dereferenced: every call below is refused, empty, or asks for a size
    net.made.var_of_step, net.made.off[0], net.var_off = 64, 64, 64
    net.nlev, net.widest = nlev, widest
    return net


def test_sizes_against_their_formulas():
    from gnf_hip import abi
    lib = abi.load()
    ref = ctypes.byref(_net(7))
    fwd = lib.gnf_strade_pack_floats(ref, 3)
    # the level image, then every layer transposed at a pitch of its rows rounded up to 16
    assert lib.gnf_strade_adjoint_pack_floats(ref, 3) == fwd + (3 + 5) * 16 + 7 * 16
    A, gos = (3 + 5 + 7) | 1, (5 * 2) | 1
    assert lib.gnf_strade_adjoint_workspace_bytes(ref, 3, 37) == 4 * 48 * (A + gos)
    assert lib.gnf_strade_adjoint_workspace_bytes(ref, 3, 0) == 0
    ref = ctypes.byref(_net(33, out=23))
    fwd = lib.gnf_strade_pack_floats(ref, 0)
    assert lib.gnf_strade_adjoint_pack_floats(ref, 0) == fwd + 5 * 48 + 33 * 128
    assert lib.gnf_strade_adjoint_workspace_bytes(ref, 0, 16) == 4 * 16 * (((5 + 33) | 1) + ((5 * 23) | 1))


def test_argument_checks_answer_before_any_launch():
    from gnf_hip import abi
    lib = abi.load()
    net = _net(7)
    ref, p = ctypes.byref(net), ctypes.c_void_p(64)
    call = lambda *a: lib.gnf_strade_adjoint(*a, None)
    EINVAL, EWS = -1, -3
    assert lib.gnf_strade_adjoint_pack_floats(ref, -1) == EINVAL
    assert lib.gnf_strade_adjoint_pack_floats(None, 0) == EINVAL
    assert lib.gnf_strade_adjoint_workspace_bytes(ref, 0, -1) == EINVAL
    assert lib.gnf_strade_adjoint_workspace_bytes(ctypes.byref(_net(7, nlev=0)), 0, 4) == EINVAL      # nlev outside 1..d
    assert lib.gnf_strade_adjoint_workspace_bytes(ctypes.byref(_net(7, widest=6)), 0, 4) == EINVAL    # widest outside 1..d
    assert call(ref, 3, None, None, None, None, None, None, None, 0, 0, None, 0) == 0          # B = 0: nothing to do
    assert call(ref, 0, None, p, p, p, p, p, p, -1, 0, None, 0) == EINVAL                      # B < 0
    assert call(ref, 3, None, p, p, p, p, p, p, 4, 0, None, 0) == EINVAL                       # no context
    for k in range(6):                                                                         # each operand NULL in turn
        ops_ = [p] * 6
        ops_[k] = None
        assert call(ref, 0, None, *ops_, 4, 0, None, 0) == EINVAL, k
    assert call(ref, 0, None, ctypes.c_void_p(68), p, p, p, p, p, 4, 0, None, 0) == EINVAL     # the pack 4 bytes off
    for field in ("var_off", "var_of_step", "off"):                                            # a NULL table
        bad = _net(7)
        if field == "var_off":
            bad.var_off = None
        elif field == "var_of_step":
            bad.made.var_of_step = None
        else:
            bad.made.off[0] = None
        assert call(ctypes.byref(bad), 0, None, p, p, p, p, p, p, 4, 0, None, 0) == EINVAL, field
    assert lib.gnf_strade_adjoint_pack(ref, 0, None, None) == EINVAL
    assert lib.gnf_strade_adjoint_pack(ref, 0, ctypes.c_void_p(68), None) == EINVAL
    # the workspace: asked for by force_ws, and by a net beyond the LDS tile -- GNF_EWS, never GNF_ESHAPE
    assert call(ref, 0, None, p, p, p, p, p, p, 4, 1, None, 0) == EWS
    need = lib.gnf_strade_adjoint_workspace_bytes(ref, 0, 4)
    assert call(ref, 0, None, p, p, p, p, p, p, 4, 1, p, need - 4) == EWS
    big = ctypes.byref(_net(12000))
    assert lib.gnf_strade_levels(big, 0, None, p, p, p, 1, 0, ctypes.c_double(0.), None, 4, None) == -2
    assert call(big, 0, None, p, p, p, p, p, p, 4, 0, None, 0) == EWS


def test_the_switch_is_off_by_default():
    from models import AffineNormalizer, StrADEConditioner, buildFCNormalizingFlow
    assert StrADEConditioner.adjoint_levels is False
    flow = buildFCNormalizingFlow(1, "StrADE", {"in_size": 5, "hidden": [8], "out_size": 2,
                                                "adjacency": R.GRAPHS["chain5"]}, AffineNormalizer, {})
    step = flow.steps[0]
    assert step.conditioner.adjoint_levels is False and "adjoint_levels" not in step.conditioner.state_dict()
    # a host tensor never takes the kernel arm, switch or no switch
    step.conditioner.adjoint_levels = True
    assert step._adjoint_plan(torch.zeros(2, 5), None) is None


@pytest.mark.parametrize("case", R.GRID, ids=R.case_id)
def test_relu_margin_of_the_gpu_grid(case):
    """the precondition of tests/test_gpu_strade_adjoint.py's rule: no hidden pre-activation of a case within MARGIN of a tie"""
    for B in R.BATCHES:
        cond, x, ctx, g, jac, dzdh = R.operands(case, B)
        layers, masks = R.layers_of(cond)
        ctx64 = ctx.double() if ctx is not None else torch.zeros(B, 0, dtype=torch.float64)
        m = R.relu_margin(layers, masks, x.double(), ctx64)
        assert m >= R.MARGIN, (R.case_id(case), B, m)
