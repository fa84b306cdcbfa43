"""Host half of the differentiable-sampling tests (NormalizingFlowStep.rsample): the law the adjoint kernel is held to, and
its ABI.

The law: tests/adjoint_ref.py:law_sweep restates the transposed column sweep of csrc/gnf_made_adjoint.hip from the plan
tables alone.  Here, in fp64, it is compared with torch.linalg.solve(J^T, g) on the Jacobian of the fp64 step
(tests/context_ref.py:made64 + the oracle's Affine normalizer), assembled sample by sample with
torch.autograd.functional.jacobian.  Both are exact solves of one triangular system: 1e-10 relative."""
import os
import re

import pytest
import torch

from adjoint_ref import law_sweep, made_layers, plan_of
from context_ref import d64, made64
from oracle import gnf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gnf_made_adjoint_pack_floats", "gnf_made_adjoint_pack", "gnf_made_adjoint_ws_bytes", "gnf_made_adjoint"]


def _law_case(cond, d, c, seed, B=4):
    P = {n: d64(p) for n, p in cond.named_parameters()}
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, d, generator=gen, dtype=torch.float64)
    ctx = torch.randn(B, c, generator=gen, dtype=torch.float64)
    g = torch.randn(B, d, generator=gen, dtype=torch.float64)

    def step(xr, cr):
        z, _ = O.affine_forward(xr[None], made64(cond, P, xr[None], cr[None]))
        return z[0]

    want = torch.stack([torch.linalg.solve(torch.autograd.functional.jacobian(lambda v: step(v, ctx[b]), x[b]).t(), g[b])
                        for b in range(B)])
    h = made64(cond, P, x, ctx).detach().requires_grad_(True)
    z, jac = O.affine_forward(x, h)
    dzdh, = torch.autograd.grad(z.sum(), h)                           # element-wise normalizer: dz_bi / dh_bi
    got = law_sweep(made_layers(cond), plan_of(cond), c, x, ctx, g, jac.detach(), dzdh)
    err = (got - want).abs().max().item() / want.abs().max().item()
    print("d=%d c=%d: law sweep vs solve(J^T, g): %.3e relative" % (d, c, err))
    assert err <= 1e-10, err


@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("hidden", [[], [8], [24, 24], [40, 33, 19]], ids=lambda h: "x".join(map(str, h)) or "none")
@pytest.mark.parametrize("d", [1, 2, 5, 17])
def test_law_sweep_equals_the_transposed_solve(d, hidden, c):
    from models import AutoregressiveConditioner
    torch.manual_seed(100 * d + 10 * c + len(hidden))
    cond = AutoregressiveConditioner(d, list(hidden), 2, cond_in=c)
    _law_case(cond, d, c, seed=d + c)


def test_law_sweep_with_a_sampled_ordering():
    from models import AutoregressiveConditioner
    from models.Conditionners.AutoregressiveConditioner import ConditionnalMADE
    d, c = 9, 2
    torch.manual_seed(6)
    cond = AutoregressiveConditioner(d, [20, 20], 2, cond_in=c)
    cond.masked_autoregressive_net = ConditionnalMADE(nin=d, cond_in=c, hidden_sizes=[20, 20], nout=2 * d, num_masks=3,
                                                      random=True)
    net = cond.masked_autoregressive_net
    net.update_masks()
    assert tuple(int(v) for v in net.m[-1]) != tuple(range(d))
    _law_case(cond, d, c, seed=11)


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
    assert "gnf_made_adjoint.hip" in build.SOURCES


def test_argument_checks_answer_before_any_launch():
    import ctypes
    from gnf_hip import abi
    lib = abi.load()
    net = abi.MadeNet()
    net.nh, net.d, net.out, net.max_new = 1, 5, 2, 1
    net.width[0] = 7
    net.var_of_step, net.off[0] = 64, 64
    ref, p = ctypes.byref(net), ctypes.c_void_p(64)              # never dereferenced: every call below is refused or empty
    fwd = lib.gnf_made_prefix_ctx_pack_floats(ref, 3)
    # the prefix image, then every layer transposed at a pitch of its rows rounded up to 16
    assert lib.gnf_made_adjoint_pack_floats(ref, 3) == fwd + (3 + 5) * 16 + 7 * 16
    A, gos = (3 + 5 + 7) | 1, (5 * 2) | 1
    assert lib.gnf_made_adjoint_ws_bytes(ref, 3, 37) == 4 * 48 * (A + gos)
    assert lib.gnf_made_adjoint_pack_floats(ref, -1) == -1
    assert lib.gnf_made_adjoint_ws_bytes(ref, 0, -1) == -1
    assert lib.gnf_made_adjoint(ref, 3, None, None, None, None, None, None, None, 0, 0, None, 0, None) == 0   # B = 0
    assert lib.gnf_made_adjoint(ref, 3, None, p, p, p, p, p, p, 4, 0, None, 0, None) == -1          # no context
    assert lib.gnf_made_adjoint(ref, 0, None, ctypes.c_void_p(68), p, p, p, p, p, 4, 0, None, 0, None) == -1
    assert lib.gnf_made_adjoint(ref, 0, None, p, p, p, p, p, p, -1, 0, None, 0, None) == -1
    assert lib.gnf_made_adjoint_pack(ref, 0, None, None) == -1


def test_rsample_refusals_need_no_gpu():
    from models import AffineNormalizer, DAGConditioner, buildFCNormalizingFlow
    from models.NormalizingFlow import CNNormalizingFlow
    flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": 4, "hidden": [8], "out_size": 2}, AffineNormalizer, {})
    assert flow.steps[0].conditioner.deterministic_importance() is None
    with pytest.raises(ValueError, match="stochastic"):
        flow.steps[0].rsample(torch.zeros(2, 4))
    with pytest.raises(NotImplementedError):
        CNNormalizingFlow([], None, []).rsample(torch.zeros(2, 4))
    assert flow.steps[0].adjoint_schedule is True
