"""CPU (-m "not gpu"): the host half of conditional sampling on the column schedule -- the four gnf_made_prefix_ctx_* symbols
of csrc/gnf_made_prefix.hip exported, declared and bound under the unchanged ABI number, their layout formulas and argument
checks, the conditional plan of the MADE (prefix_plan(with_context=True)), and the LAW of the schedule: a numpy fp64
emulation that walks the plan as the kernel does (context first, K = c + t, the units of degree t - 1 per step, the strict
output rule, the Affine inverse per column) against the fixed-point inversion of the CPU oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import gnf_oracle as O
from test_context_host import MADE_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnf_made_prefix_ctx_pack_floats", "gnf_made_prefix_ctx_pack", "gnf_made_prefix_ctx_ws_bytes", "gnf_made_prefix_ctx")


def test_symbols_exported_declared_and_bound():
    from gnf_hip import abi
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


def _host_net(d, widths, out, max_new=1):
    """a gnf_made_net whose pointers are never dereferenced (the size queries and the refused calls read the integers only)"""
    from gnf_hip import abi
    net = abi.MadeNet()
    net.nh, net.d, net.out, net.max_new = len(widths), d, out, max_new
    for l, w in enumerate(widths):
        net.width[l] = w
        net.order[l] = net.off[l] = 64
    for l in range(len(widths) + 1):
        net.W[l] = net.b[l] = 64
    net.var_of_step = 64
    return net


def _round_up(v, m):
    return (v + m - 1) // m * m


@pytest.mark.parametrize("d,widths,out", [(1, [4], 2), (5, [7, 7], 2), (4, [], 2), (17, [40, 33, 19], 3), (63, [630], 30)],
                         ids=["1-4", "5-7x7", "4-none", "17-40x33x19", "63-630"])
def test_pack_and_workspace_sizes(d, widths, out):
    from gnf_hip import abi
    lib = abi.load()
    net = _host_net(d, widths, out)
    ref = ctypes.byref(net)
    assert lib.gnf_made_prefix_ctx_pack_floats(ref, 0) == lib.gnf_made_prefix_pack_floats(ref)
    for B in (0, 1, 70):
        assert lib.gnf_made_prefix_ctx_ws_bytes(ref, 0, B) == lib.gnf_made_prefix_ws_bytes(ref, B)
    for c in (1, 3, 8, 20):
        fan = [c + d] + widths
        rows = widths + [d * out]
        want = sum(r * _round_up(k, 16) + _round_up(r, 4) for r, k in zip(rows, fan))
        assert lib.gnf_made_prefix_ctx_pack_floats(ref, c) == want, c
        for B in (0, 1, 70, 129):
            assert lib.gnf_made_prefix_ctx_ws_bytes(ref, c, B) == 4 * B * ((c + d + sum(widths)) | 1), (c, B)
    assert lib.gnf_made_prefix_ctx_pack_floats(ref, -1) == -1
    assert lib.gnf_made_prefix_ctx_pack_floats(ref, 1 << 26) > 0                 # the widest context the kernel indexes
    assert lib.gnf_made_prefix_ctx_pack_floats(ref, (1 << 26) + 1) == -2
    assert lib.gnf_made_prefix_ctx(ref, (1 << 26) + 1, None, None, None, None, None, 0, 1, 1, 4, None, 0, None) == -2
    assert lib.gnf_made_prefix_ctx_ws_bytes(ref, -1, 4) == -1
    assert lib.gnf_made_prefix_ctx_ws_bytes(ref, 2, -4) == -1


def test_argument_checks_answer_before_any_launch():
    from gnf_hip import abi
    lib = abi.load()
    p = ctypes.c_void_p(64)                                      # never dereferenced: every call below is refused or empty
    net = _host_net(5, [7, 7], 2)
    ref = ctypes.byref(net)
    NONE, AFFINE = abi.MADE_NORM_NONE, abi.MADE_NORM_AFFINE
    assert lib.gnf_made_prefix_ctx(ref, -1, p, p, p, p, p, 0, 5, AFFINE, 4, p, 1 << 20, None) == -1     # negative cond_in
    assert lib.gnf_made_prefix_ctx_pack(ref, -1, p, None) == -1
    assert lib.gnf_made_prefix_ctx(ref, 2, None, p, p, p, p, 0, 5, AFFINE, 4, p, 1 << 20, None) == -1   # null context, B > 0
    assert lib.gnf_made_prefix_ctx(ref, 2, None, p, p, p, p, 2, 3, NONE, 4, p, 1 << 20, None) == -1
    assert lib.gnf_made_prefix_ctx(ref, 2, p, p, p, p, p, 0, 2, NONE, 4, p, 1 << 20, None) == -1        # NONE with t1 > t0 + 1
    assert lib.gnf_made_prefix_ctx(ref, 2, p, p, p, p, p, 0, 6, AFFINE, 4, p, 1 << 20, None) == -1      # t1 > d
    assert lib.gnf_made_prefix_ctx(ref, 2, p, p, p, p, p, 0, 5, 7, 4, p, 1 << 20, None) == -1           # unknown mode
    assert lib.gnf_made_prefix_ctx(ref, 2, None, None, None, None, None, 0, 5, AFFINE, 0, None, 0, None) == 0   # B == 0
    assert lib.gnf_made_prefix_ctx(ref, 2, None, None, None, None, None, 3, 3, AFFINE, 4, None, 0, None) == 0   # t1 == t0
    assert lib.gnf_made_prefix_ctx(ref, 2, p, ctypes.c_void_p(68), p, p, p, 0, 5, AFFINE, 4, p, 1 << 20, None) == -1  # pack
    assert lib.gnf_made_prefix_ctx(ref, 2, p, p, p, p, p, 1, 2, AFFINE, 4, None, 0, None) == -3         # a step needs ws
    assert lib.gnf_made_prefix_ctx(ref, 2, p, p, p, p, p, 1, 2, AFFINE, 4, p, 4 * 4 * 21 - 4, None) == -3


@pytest.mark.parametrize("nin,c,hidden,random", MADE_CASES,
                         ids=["1-1-4", "5-2-7x7", "4-3-none", "5-2-7x7-random", "4-3-none-random"])
def test_conditional_plan(nin, c, hidden, random):
    from models.Conditionners.AutoregressiveConditioner import MADE, ConditionnalMADE
    kw = {"num_masks": 2, "random": True} if random else {}
    net, ref = ConditionnalMADE(nin, c, hidden, 2 * nin, **kw), MADE(nin, hidden, 2 * nin, **kw)
    plans = []
    for _ in range(3 if random else 1):
        assert net.prefix_plan() is None
        plan, want = net.prefix_plan(with_context=True), ref.prefix_plan()
        assert plan is not None and want is not None
        assert plan is net.prefix_plan(with_context=True)                        # cached
        assert plan["cond_in"] == c and want.get("cond_in", 0) == 0
        for k in ("d", "out", "widths", "max_new", "var_host"):
            assert plan[k] == want[k], k
        assert torch.equal(plan["var_of_step"], want["var_of_step"])
        for k in ("order", "off"):
            assert len(plan[k]) == len(want[k]) and all(torch.equal(a, b) for a, b in zip(plan[k], want[k])), k
        plans.append(tuple(plan["var_host"]))
        net.update_masks()
        ref.update_masks()
    if random and nin > 2:
        assert len(set(plans)) > 1                                               # the plan follows the ordering


def test_plan_of_the_conditioner_and_hand_set_masks():
    from models import AutoregressiveConditioner
    cond = AutoregressiveConditioner(5, [19], 2, cond_in=2)
    assert cond.prefix_plan() is None
    plan = cond.prefix_plan(with_context=True)
    assert plan is not None and plan["cond_in"] == 2 and plan["d"] == 5
    plain = AutoregressiveConditioner(5, [19], 2)
    assert plain.prefix_plan() is not None and plain.prefix_plan(with_context=True) is plain.prefix_plan()
    assert plain.prefix_plan()["cond_in"] == 0
    for which in (0, 1):                                         # the first layer (context columns) and the output layer
        cond = AutoregressiveConditioner(5, [19], 2, cond_in=2)
        layer = cond.masked_autoregressive_net.masked_layers()[which]
        mask = layer.mask.cpu().numpy().T.copy()
        i, o = np.argwhere(mask > 0)[0]
        mask[i, o] = 0                                           # autoregressive still, but no degree rule
        layer.set_mask(mask)
        assert cond.prefix_plan(with_context=True) is None


# ------------------------------------------------------------------------------------------------ the law of the schedule
def _emulate(net, plan, z, ctx):
    """fp64 walk of the plan as made_prefix_k walks it: the activation row is [context | x in degree order | hidden ...],
    weights are taken in degree order, no mask is read -- the prefix length is the mask"""
    layers = [(l.weight.detach().double().numpy(), l.bias.detach().double().numpy()) for l in net.masked_layers()]
    nh, d, out, c = len(plan["widths"]), plan["d"], plan["out"], plan["cond_in"]
    var = [int(v) for v in plan["var_of_step"]]
    order = [o.numpy() for o in plan["order"]]
    off = [o.numpy() for o in plan["off"]]
    B = z.shape[0]
    # the packed image: first-layer column k < c is itself, column c + j is c + var_of_step[j]
    cols0 = np.concatenate([np.arange(c), c + np.asarray(var, dtype=np.int64)]).astype(np.int64)
    packed = []
    for l in range(nh + 1):
        W, b = layers[l]
        rows = order[l] if l < nh else np.asarray([(r % out) * d + var[r // out] for r in range(d * out)])
        cols = cols0 if l == 0 else order[l - 1]
        packed.append((W[rows][:, cols], b[rows]))
    inp = np.zeros((B, c + d))
    inp[:, :c] = ctx                                             # known before step 0
    hid = [np.zeros((B, w)) for w in plan["widths"]]
    x = np.zeros((B, d))
    for t in range(d):
        if t >= 1:
            for l in range(nh):
                n0, n1 = off[l][t - 1], off[l][t]                # the units of degree t - 1
                K = c + t if l == 0 else off[l - 1][t]
                src = inp if l == 0 else hid[l - 1]
                W, b = packed[l]
                hid[l][:, n0:n1] = np.maximum(src[:, :K] @ W[n0:n1, :K].T + b[n0:n1], 0.)
        K = c + t if nh == 0 else off[nh - 1][t]                 # strict rule: degree < t (the context's is -1)
        src = inp if nh == 0 else hid[nh - 1]
        W, b = packed[nh]
        h = src[:, :K] @ W[t * out:(t + 1) * out, :K].T + b[t * out:(t + 1) * out]
        mu, sg = np.clip(h[:, 0], -5., 5.), np.exp(np.clip(h[:, 1], -5., 2.))
        xv = (z[:, var[t]] - mu) / sg
        x[:, var[t]] = xv
        inp[:, c + t] = xv
    return x


LAW_CASES = MADE_CASES + [(17, 3, [40, 33, 19], False)]


@pytest.mark.parametrize("nin,c,hidden,random", LAW_CASES,
                         ids=["1-1-4", "5-2-7x7", "4-3-none", "5-2-7x7-random", "4-3-none-random", "17-3-40x33x19"])
def test_law_of_the_schedule(nin, c, hidden, random):
    from context_ref import d64, made64
    from models import AutoregressiveConditioner
    from models.Conditionners.AutoregressiveConditioner import ConditionnalMADE
    torch.manual_seed(10 * nin + c)
    cond = AutoregressiveConditioner(nin, list(hidden), 2, cond_in=c)
    if random:
        cond.masked_autoregressive_net = ConditionnalMADE(nin, c, list(hidden), 2 * nin, num_masks=2, random=True)
    net = cond.masked_autoregressive_net
    gen = torch.Generator().manual_seed(3)
    z = .7 * torch.randn(9, nin, generator=gen).double()
    for _ in range(2 if random else 1):
        plan = net.prefix_plan(with_context=True)
        assert plan is not None
        P = {"masked_autoregressive_net." + n: d64(p) for n, p in net.named_parameters()}
        ctx = torch.randn(9, c, generator=gen).double()
        want = O.step_invert(z, lambda v: made64(cond, P, v, ctx), O.affine_inverse, nin - 1)
        got = _emulate(net, plan, z.numpy(), ctx.numpy())
        err = np.abs(got - want.numpy()).max() / max(np.abs(want.numpy()).max(), 1e-300)
        assert err < 1e-12, err
        # section 1 of the kernel's header: with hidden layers the degree-0 variable's outputs are the output bias, without
        # they read the context
        other = _emulate(net, plan, z.numpy(), ctx.numpy() + 1.)
        v0 = int(plan["var_of_step"][0])
        assert np.array_equal(other[:, v0], got[:, v0]) == bool(hidden)
        net.update_masks()


def test_train_uci_parse_accepts_sample():
    import train_uci
    assert train_uci.parse(["-dataset", "power"]).sample == 0
    assert train_uci.parse(["-dataset", "power", "-sample", "7", "-context_cols", "2"]).sample == 7
    with pytest.raises(SystemExit):
        train_uci.parse(["-dataset", "power", "-sample", "-1"])
