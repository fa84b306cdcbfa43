"""GPU: differentiable interventional sampling -- NormalizingFlowStep.rsample_do / rcounterfactual, and the pinned adjoint
kernels behind their backward (gnf_made_adjoint_do in csrc/gnf_made_adjoint.hip, gnf_strade_adjoint_do in
csrc/gnf_strade_adjoint.hip).

The forward is intervene, bit for bit.  Under do(x_P = v) the backward solves lambda_P = 0, J_FF^T lambda_F = g_F at the
sample and returns dL/dz = lambda, dL/dv = g_P - (N^T lambda)_P; parameters and context get one vjp with -lambda.

Criterion, that of tests/test_gpu_rsample.py: the thing under test and a comparator are two fp32 evaluations of one function
in different summation orders, so each is measured against fp64 and err_test <= 2 err_comparator + 1e-6 max|reference| is
required.  The comparator of the kernels is the passes solve written below with existing ops; the fp64 references are the
laws of tests/adjoint_do_ref.py (checked against torch.linalg.solve by tests/test_rsample_do_host.py).  For gdo the reference
scale is max(max|gdo|, max|g|): gdo = g - u, and a column whose u vanishes reproduces g.
Set GNF_RSAMPLE_DO_PROFILE=<file> to have the worst measured ratios appended there."""
import ctypes
import os

import pytest
import torch

import adjoint_do_ref as D
import misaligned
import poison
import spline_ref as S
import strade_adjoint_ref as R
from adjoint_ref import _pairs, flow_steps, law_sweep, leaves, made_layers, plan_of
from oracle import gnf_oracle as O
from test_gpu_rsample import GRID, NAMED, _case_id, _dag_step, _flow, _inputs, _kernel_operands

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS, TS = 8, 3.
BITS = [("chain5", "R", 3, 2), ("d17", "40-24", 3, 2), ("wide", "40-24", 0, 23)]      # those of tests/test_gpu_strade_adjoint.py
_RATIOS = {}            # group -> [(case, err_test, err_comparator, scale)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GNF_RSAMPLE_DO_PROFILE")
    if path and _RATIOS:
        with open(path, "a") as f:
            for group, rows in _RATIOS.items():
                worst = max(rows, key=lambda r: r[1] / max(2. * r[2] + 1e-6 * r[3], 1e-300))
                f.write("%s (tests/test_gpu_rsample_do.py), %d cases\n" % (group, len(rows)))
                f.write("worst err / (2 err_comparator + 1e-6 scale) = %.3f at %s: err %.3e, err_comparator %.3e, scale %.3e\n"
                        % (worst[1] / max(2. * worst[2] + 1e-6 * worst[3], 1e-300), worst[0], worst[1], worst[2], worst[3]))


def _rule(group, case, e_test, e_cmp, scale):
    print("%s | %s: err %.3e comparator %.3e scale %.3e" % (group, case, e_test, e_cmp, scale))
    _RATIOS.setdefault(group, []).append((case, e_test, e_cmp, scale))
    assert e_test <= 2. * e_cmp + 1e-6 * scale, (group, case, e_test, e_cmp, scale)


def cu(t):
    return None if t is None else t.to(DEV)


def c64(t):
    return t.detach().cpu().double()


def _err(a, b):
    return (c64(a) - b).abs().max().item() if b.numel() else 0.


def _zeros_exactly(t):
    """every entry is +0, bit for bit"""
    return poison.differing(t.contiguous(), torch.zeros_like(t).contiguous()) == 0


def _table(pin):
    return cu(pin.to(torch.uint8))


def _patterns(order, d):
    """[(name, bool [d] by variable)] of the pin patterns that d allows, by position in the topological order"""
    return [(n, D.pin_of(D.pattern(n, d), order, d)) for n in D.PATTERNS if D.pattern(n, d) is not None]


def _passes_do(cond, x, ctx, g, jac, dzdh, pin, depth):
    """the comparator: the mutilated system by vjps of the existing kernels, lambda <- where(pinned, 0, (g - N^T lambda) / jac),
    exact after `depth` of them; gdo from N^T lambda of the last lambda.  Not the code under test."""
    xa = x.detach().requires_grad_(True)
    h = cond(xa, ctx)
    pd, zero = cu(pin), torch.zeros_like(g)

    def nt(lam):
        nl, = torch.autograd.grad(h, xa, lam.unsqueeze(2) * dzdh, retain_graph=True, allow_unused=True)
        return zero if nl is None else nl

    lam = torch.where(pd, zero, g / jac)
    for _ in range(depth):
        lam = torch.where(pd, zero, (g - nt(lam)) / jac)
    return lam, torch.where(pd, g - nt(lam), zero)


def _check_solve(group, case, lam, gdo, lam_only, pin, g, law, cmp):
    """what every pinned solve owes: the exact zeros, lambda independent of gdo, and the rule for both outputs"""
    pd = cu(pin)
    assert torch.isfinite(lam).all() and torch.isfinite(gdo).all(), case
    assert poison.differing(lam, lam_only) == 0, case                 # lambda is the same bits with and without gdo
    assert _zeros_exactly(lam[:, pd]) and _zeros_exactly(gdo[:, ~pd]), case
    if bool(pin.all()):
        assert poison.differing(gdo, g) == 0, case                    # no contraction: dL/dv = g exactly
    _rule(group + ", lambda", case, _err(lam, law[0]), _err(cmp[0], law[0]), law[0].abs().max().item())
    _rule(group + ", gdo", case, _err(gdo, law[1]), _err(cmp[1], law[1]),
          max(law[1].abs().max().item(), c64(g).abs().max().item()))


# ------------------------------------------------------------------------------------ 1. MADE kernel against the law
def _made_solve(cond, x, g, jac, dzdh, ctx, pin, gdo, pack=None, **kw):
    from gnf_hip import ops
    plan, params = cond.prefix_plan(with_context=ctx is not None), cond._prefix_params()
    pack = ops.made_adjoint_pack(params, plan) if pack is None else pack
    return ops.made_adjoint(params, plan, pack, x, g, jac, dzdh, context=ctx, pin=pin, gdo=gdo, **kw)


@pytest.mark.parametrize("case", GRID + NAMED[1:], ids=_case_id)
def test_made_kernel_against_the_law(case):
    from gnf_hip import ops
    d, c, hidden = case
    for B in (5, 37):                                                # a ragged tile; several tiles
        cond, x, ctx, g, jac, dzdh = _kernel_operands(d, c, hidden, B, seed=100 * d + 10 * c + len(hidden))
        plan, params = cond.prefix_plan(with_context=bool(c)), cond._prefix_params()
        pack = ops.made_adjoint_pack(params, plan)
        ctx64 = c64(ctx) if c else torch.zeros(B, 0, dtype=torch.float64)
        unpinned = ops.made_adjoint(params, plan, pack, x, g, jac, dzdh, context=ctx)
        for name, pin in _patterns(plan_of(cond)["var_of_step"], d):
            tab = _table(pin)
            lam, gdo = _made_solve(cond, x, g, jac, dzdh, ctx, tab, True, pack)
            lam_only = _made_solve(cond, x, g, jac, dzdh, ctx, tab, False, pack)
            got = cond.adjoint_solve(x, g, jac, dzdh, context=ctx, pin=tab, want_gdo=True)
            assert poison.differing(got[0], lam) == 0 and poison.differing(got[1], gdo) == 0
            if name == "none":                                       # an all-zero table: the un-pinned entry point's bits
                assert poison.differing(lam, unpinned) == 0 and _zeros_exactly(gdo)
            law = D.law_sweep_do(made_layers(cond), plan_of(cond), c, c64(x), ctx64, c64(g), c64(jac), c64(dzdh), pin)
            cmp = _passes_do(cond, x, ctx, g, jac, dzdh, pin, d - 1)
            _check_solve("pinned MADE adjoint kernel vs passes, both against the fp64 law", "%s B=%d %s" % (_case_id(case), B, name),
                         lam, gdo, lam_only, pin, g, law, cmp)


def test_made_kernel_with_a_sampled_ordering():
    from models.Conditionners.AutoregressiveConditioner import ConditionnalMADE
    d, c, B = 9, 2, 37
    cond, x, ctx, g, jac, dzdh = _kernel_operands(d, c, [20, 20], B, seed=5)
    torch.manual_seed(6)
    cond.masked_autoregressive_net = ConditionnalMADE(nin=d, cond_in=c, hidden_sizes=[20, 20], nout=2 * d, num_masks=3,
                                                      random=True).to(DEV)
    cond.masked_autoregressive_net.update_masks()
    order = plan_of(cond)["var_of_step"]
    assert tuple(int(v) for v in order) != tuple(range(d))
    for name, pin in _patterns(order, d):
        tab = _table(pin)
        lam, gdo = _made_solve(cond, x, g, jac, dzdh, ctx, tab, True)
        lam_only = _made_solve(cond, x, g, jac, dzdh, ctx, tab, False)
        law = D.law_sweep_do(made_layers(cond), plan_of(cond), c, c64(x), c64(ctx), c64(g), c64(jac), c64(dzdh), pin)
        _check_solve("pinned MADE adjoint kernel vs passes, both against the fp64 law", "sampled ordering d=9 c=2 %s" % name,
                     lam, gdo, lam_only, pin, g, law, _passes_do(cond, x, ctx, g, jac, dzdh, pin, d - 1))


def test_made_without_a_table_is_the_existing_entry_point():
    """pin == NULL through the new entry point: the bits of gnf_made_adjoint; gdo without a table is refused"""
    from gnf_hip import abi, ops
    d, c, hidden = NAMED[0]
    cond, x, ctx, g, jac, dzdh = _kernel_operands(d, c, hidden, 37, seed=3)
    plan, params = cond.prefix_plan(with_context=True), cond._prefix_params()
    pack = ops.made_adjoint_pack(params, plan)
    want = ops.made_adjoint(params, plan, pack, x, g, jac, dzdh, context=ctx)
    net = ops._made_net([p.detach() for p in params], plan)
    p = abi.ptr
    for force in (0, 1):
        lam = torch.full_like(x, 7.)
        nbytes = abi.load().gnf_made_adjoint_ws_bytes(ctypes.byref(net), c, 37)
        ws = torch.zeros(nbytes // 4, device=DEV)
        rc = abi.load().gnf_made_adjoint_do(ctypes.byref(net), c, p(ctx), p(pack), p(x), p(g), p(jac), p(dzdh), p(lam), None, None,
                                            37, force, ctypes.c_void_p(ws.data_ptr()), nbytes, abi.stream())
        torch.cuda.synchronize()
        assert rc == 0 and poison.differing(lam, want) == 0, force
    lam, gd = torch.full_like(x, 7.), torch.full_like(x, 7.)
    rc = abi.load().gnf_made_adjoint_do(ctypes.byref(net), c, p(ctx), p(pack), p(x), p(g), p(jac), p(dzdh), p(lam), None, p(gd),
                                        37, 0, None, 0, abi.stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((lam == 7.).all()) and bool((gd == 7.).all())       # GNF_EINVAL, nothing launched
    with pytest.raises(abi.GnfError):
        ops.made_adjoint(params, plan, pack, x, g, jac, dzdh, context=ctx, gdo=True)


# ---------------------------------------------------------------------------------- 2. StrADE kernel against the law
def _strade_solve(cond, x, g, jac, dzdh, ctx, pin, gdo, pack=None, **kw):
    from gnf_hip import ops
    params, masks, plan = cond._params(), cond._masks(), cond.level_plan()
    pack = ops.strade_adjoint_pack(params, masks, plan) if pack is None else pack
    return ops.strade_adjoint(params, masks, plan, pack, x, g, jac, dzdh, context=ctx, pin=pin, gdo=gdo, **kw)


def _strade_operands(case, B):
    cond, *ts = R.operands(case, B)
    return (cond.to(DEV), *[cu(t) for t in ts])


@pytest.mark.parametrize("case", R.GRID, ids=R.case_id)
def test_strade_kernel_against_the_law(case):
    from gnf_hip import ops
    for B in R.BATCHES:
        cond, x, ctx, g, jac, dzdh = _strade_operands(case, B)
        d = cond.in_size
        pack = ops.strade_adjoint_pack(cond._params(), cond._masks(), cond.level_plan())
        unpinned = ops.strade_adjoint(cond._params(), cond._masks(), cond.level_plan(), pack, x, g, jac, dzdh, context=ctx)
        for name, pin in _patterns(R.numpy_plan(cond)["var_order"], d):
            tab = _table(pin)
            lam, gdo = _strade_solve(cond, x, g, jac, dzdh, ctx, tab, True, pack)
            lam_only = _strade_solve(cond, x, g, jac, dzdh, ctx, tab, False, pack)
            got = cond.adjoint_solve(x, g, jac, dzdh, context=ctx, pin=tab, want_gdo=True)
            assert poison.differing(got[0], lam) == 0 and poison.differing(got[1], gdo) == 0
            if name == "none":
                assert poison.differing(lam, unpinned) == 0 and _zeros_exactly(gdo)
            law = D.law64_do(cond, x, ctx, g, jac, dzdh, pin)
            cmp = _passes_do(cond, x, ctx, g, jac, dzdh, pin, cond.depth())
            _check_solve("pinned StrADE adjoint kernel vs passes, both against the fp64 law",
                         "%s B=%d %s" % (R.case_id(case), B, name), lam, gdo, lam_only, pin, g, law, cmp)


def _level_pins(cond, choose):
    """bool [d] by variable: choose(level index, variables of the level in level order) -> the pinned ones of that level"""
    plan = R.numpy_plan(cond)
    var, off = [int(v) for v in plan["var_order"]], [int(v) for v in plan["var_off"]]
    pin = torch.zeros(plan["d"], dtype=torch.bool)
    for t in range(plan["nlev"]):
        for v in choose(t, var[off[t]:off[t + 1]]):
            pin[v] = True
    return pin


@pytest.mark.parametrize("name", ["d17", "wide"])
@pytest.mark.parametrize("out", [2, 23])
def test_strade_chunks_fully_and_partly_pinned(name, out):
    """the middle level of d17 (9 variables: a chunk of 8 and one of 1) and of wide (19: 8 + 8 + 3): its first chunk pinned
    whole -- no contraction behind it without gdo --, its second pinned in part, the levels around it free; and the same with
    the last level pinned whole, which moves t_last onto the middle level"""
    case = (name, "40-24", 3, out)
    cond, x, ctx, g, jac, dzdh = _strade_operands(case, 37)
    for tail in (False, True):
        pin = _level_pins(cond, lambda t, vs: (vs[:R.CHUNK] + vs[R.CHUNK + 1:R.CHUNK + 2] if t == 1 else vs if t == 2 and tail
                                               else []))
        assert int(pin.sum()) >= R.CHUNK
        tab = _table(pin)
        lam, gdo = _strade_solve(cond, x, g, jac, dzdh, ctx, tab, True)
        lam_only = _strade_solve(cond, x, g, jac, dzdh, ctx, tab, False)
        law = D.law64_do(cond, x, ctx, g, jac, dzdh, pin)
        _check_solve("pinned StrADE adjoint kernel vs passes, both against the fp64 law",
                     "%s chunks tail=%s" % (R.case_id(case), tail), lam, gdo, lam_only, pin, g, law,
                     _passes_do(cond, x, ctx, g, jac, dzdh, pin, cond.depth()))


def test_strade_without_a_table_is_the_existing_entry_point():
    from gnf_hip import abi, ops
    cond, x, ctx, g, jac, dzdh = _strade_operands(BITS[1], 37)
    params, masks, plan = cond._params(), cond._masks(), cond.level_plan()
    pack = ops.strade_adjoint_pack(params, masks, plan)
    want = ops.strade_adjoint(params, masks, plan, pack, x, g, jac, dzdh, context=ctx)
    net = ops._strade_net([q.detach() for q in params], masks, plan)
    p = abi.ptr
    nbytes = abi.load().gnf_strade_adjoint_workspace_bytes(ctypes.byref(net), 3, 37)
    ws = torch.zeros(nbytes // 4, device=DEV)
    for force in (0, 1):
        lam = torch.full_like(x, 7.)
        rc = abi.load().gnf_strade_adjoint_do(ctypes.byref(net), 3, p(ctx), p(pack), p(x), p(g), p(jac), p(dzdh), p(lam), None,
                                              None, 37, force, ctypes.c_void_p(ws.data_ptr()), nbytes, abi.stream())
        torch.cuda.synchronize()
        assert rc == 0 and poison.differing(lam, want) == 0, force
    lam, gd = torch.full_like(x, 7.), torch.full_like(x, 7.)
    rc = abi.load().gnf_strade_adjoint_do(ctypes.byref(net), 3, p(ctx), p(pack), p(x), p(g), p(jac), p(dzdh), p(lam), None, p(gd),
                                          37, 0, None, 0, abi.stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((lam == 7.).all()) and bool((gd == 7.).all())
    with pytest.raises(abi.GnfError):
        ops.strade_adjoint(params, masks, plan, pack, x, g, jac, dzdh, context=ctx, gdo=True)


# ------------------------------------------------------------------------------- 3. memory forms, alignment, poison
def _family_cases():
    """(id, operands(), solve, topological order) of the NAMED MADE cases and the BITS StrADE cases"""
    out = []
    for k, case in enumerate(NAMED):
        def make(case=case):
            d, c, hidden = case
            return _kernel_operands(d, c, hidden, 37, seed=3)
        out.append(("made-" + ("dot", "mfma")[k], make, _made_solve, lambda cond: plan_of(cond)["var_of_step"]))
    for case in BITS:
        out.append(("strade-" + R.case_id(case), lambda case=case: _strade_operands(case, 37), _strade_solve,
                    lambda cond: R.numpy_plan(cond)["var_order"]))
    return out


FAMILY = _family_cases()


def _mixed_pin(order, d):
    """every second position and the last one: pinned and free steps alternate, and the run at the end is skipped"""
    return D.pin_of(sorted(set(range(1, d, 2)) | {d - 1}), order, d)


@pytest.mark.parametrize("fam", FAMILY, ids=[f[0] for f in FAMILY])
def test_lds_form_equals_workspace_form(fam):
    _, make, solve, order_of = fam
    cond, x, ctx, g, jac, dzdh = make()
    d = x.shape[1]
    for name, pin in _patterns(order_of(cond), d) + [("mixed", _mixed_pin(order_of(cond), d))]:
        tab = _table(pin)
        for want_gdo in (True, False):
            lds = solve(cond, x, g, jac, dzdh, ctx, tab, want_gdo)
            wsf = solve(cond, x, g, jac, dzdh, ctx, tab, want_gdo, force_ws=True)
            for a, b in zip(lds if want_gdo else (lds,), wsf if want_gdo else (wsf,)):
                assert torch.isfinite(a).all() and poison.differing(a, b) == 0, (name, want_gdo)


def _place_table(tab, offset):
    """the uint8 table at an address = offset (mod 16), between guard bytes: (view, whole buffer, start of the view)"""
    d = tab.numel()
    raw = torch.full((d + 64,), 0xA5, dtype=torch.uint8, device=tab.device)
    start = 16 + (offset - raw.data_ptr() - 16) % 16
    view = raw[start:start + d]
    view.copy_(tab)
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    return view, raw, start


def _table_guards_intact(raw, start, d):
    return bool((raw[:start] == 0xA5).all()) and bool((raw[start + d:] == 0xA5).all())


@pytest.mark.parametrize("fam", FAMILY, ids=[f[0] for f in FAMILY])
def test_dword_aligned_operands_and_a_table_at_any_byte(fam):
    _, make, solve, order_of = fam
    cond, x, ctx, g, jac, dzdh = make()
    d = x.shape[1]
    pin = _mixed_pin(order_of(cond), d)
    tab = _table(pin)
    want = solve(cond, x, g, jac, dzdh, ctx, tab, True)
    for k in (1, 2, 3):
        moved = [misaligned.place(t, k) for t in (x, g, jac, dzdh) + ((ctx,) if ctx is not None else ())]
        assert all(t.data_ptr() % 16 == 4 * k for t in moved)
        for offset in (4 * k, 2 * k + 1):                             # the table dword-aligned only, and at an odd byte
            view, raw, start = _place_table(tab, offset)
            for force in (False, True):
                got = solve(cond, *moved[:4], moved[4] if ctx is not None else None, view, True, force_ws=force)
                assert poison.differing(got[0], want[0]) == 0 and poison.differing(got[1], want[1]) == 0, (k, offset, force)
            torch.cuda.synchronize()
            assert _table_guards_intact(raw, start, d), (k, offset)
        assert all(misaligned.guards_intact(t) for t in moved), k


@pytest.mark.parametrize("force_ws", [False, True], ids=["lds", "ws"])
@pytest.mark.parametrize("fam", FAMILY, ids=[f[0] for f in FAMILY])
def test_poisoned_buffers_change_no_bit(fam, force_ws):
    """lambda, gdo, the weight image and the workspace are torch.empty of the wrappers: zeros, NaNs and huge values in them,
    the same bits (tests/poison.py) -- every element of lambda and of gdo is written, pinned or free"""
    _, make, solve, order_of = fam

    def run():
        cond, x, ctx, g, jac, dzdh = make()
        tab = _table(_mixed_pin(order_of(cond), x.shape[1]))
        lam, gdo = solve(cond, x, g, jac, dzdh, ctx, tab, True, force_ws=force_ws)
        every = _table(torch.ones(x.shape[1], dtype=torch.bool))
        lam_all, gdo_all = solve(cond, x, g, jac, dzdh, ctx, every, True, force_ws=force_ws)
        return {"lam": lam, "gdo": gdo, "lam_only": solve(cond, x, g, jac, dzdh, ctx, tab, False, force_ws=force_ws),
                "lam_all": lam_all, "gdo_all": gdo_all}
    poison.three_arms(run)


# ------------------------------------------------------------------------------------------------------ 4. selection
@pytest.mark.parametrize("fam", FAMILY, ids=[f[0] for f in FAMILY])
def test_pinned_elements_are_selected_never_multiplied(fam):
    """jac = 0, inf, NaN and dzdh = inf, NaN planted at the pinned elements: every output finite and bit-equal to the run with
    benign values there"""
    _, make, solve, order_of = fam
    cond, x, ctx, g, jac, dzdh = make()
    d = x.shape[1]
    for name, pin in [(n, p) for n, p in _patterns(order_of(cond), d) if n != "none"] + [("mixed", _mixed_pin(order_of(cond), d))]:
        tab, pd = _table(pin), cu(pin)
        want = solve(cond, x, g, jac, dzdh, ctx, tab, True)
        assert torch.isfinite(want[0]).all() and torch.isfinite(want[1]).all()
        for jbad, hbad in ((0., float("inf")), (float("inf"), float("nan")), (float("nan"), float("-inf"))):
            j2, h2 = jac.clone(), dzdh.clone()
            j2[:, pd] = jbad
            h2[:, pd] = hbad
            got = solve(cond, x, g, j2, h2, ctx, tab, True)
            assert poison.differing(got[0], want[0]) == 0 and poison.differing(got[1], want[1]) == 0, (name, jbad, hbad)
            assert poison.differing(solve(cond, x, g, j2, h2, ctx, tab, False), want[0]) == 0, (name, jbad, hbad)


def test_a_bad_table_raises_gnf_error():
    from gnf_hip import abi
    for fam in (FAMILY[0], FAMILY[3]):
        _, make, solve, _ = fam
        cond, x, ctx, g, jac, dzdh = make()
        d = x.shape[1]
        good = torch.zeros(d, dtype=torch.uint8, device=DEV)
        bad = [good.bool(), good.int(), good[:-1], good.cpu(), torch.zeros(2 * d, dtype=torch.uint8, device=DEV)[::2],
               good.view(1, d)]
        for tab in bad:
            with pytest.raises(abi.GnfError, match="pin must be a contiguous uint8"):
                solve(cond, x, g, jac, dzdh, ctx, tab, False)


# ------------------------------------------------------------------------------------------------------ 5. path taken
class _Count:
    """calls of ops.made_adjoint / ops.strade_adjoint (and how many of them carried a pin table, asked for gdo) and of the
    conditioner module while it is entered"""

    def __init__(self, step):
        self.step, self.adjoint, self.pinned, self.gdo, self.module = step, 0, 0, 0, 0

    def __enter__(self):
        from gnf_hip import ops
        self._ops, self._orig = ops, (ops.made_adjoint, ops.strade_adjoint)

        def counted(orig):
            def fn(*a, **k):
                self.adjoint += 1
                self.pinned += k.get("pin") is not None
                self.gdo += bool(k.get("gdo"))
                return orig(*a, **k)
            return fn
        ops.made_adjoint, ops.strade_adjoint = counted(self._orig[0]), counted(self._orig[1])
        self._hook = self.step.conditioner.register_forward_hook(lambda *a: setattr(self, "module", self.module + 1))
        return self

    def __exit__(self, *exc):
        self._ops.made_adjoint, self._ops.strade_adjoint = self._orig
        self._hook.remove()


def test_one_adjoint_launch_and_one_conditioner_call_for_a_made_step():
    step = _flow("made", 5, 2, [19]).steps[0]
    z, ctx, w = _inputs(3, 5, 2, 1)
    z.requires_grad_(True)
    v = torch.tensor([.3, -.2], device=DEV, requires_grad=True)
    with _Count(step) as n:
        x = step.rsample_do(z, [1, 3], v, ctx)
        assert (n.adjoint, n.module) == (0, 0) and step._intervene_arm == "columns"
        (w * x).sum().backward()
    assert (n.adjoint, n.pinned, n.gdo, n.module) == (1, 1, 1, 1) and step._rsample_arm == ("adjoint", 0)
    assert _zeros_exactly(z.grad[:, [1, 3]]) and tuple(v.grad.shape) == (2,)
    with _Count(step) as n:                                           # a float value: no gdo is asked for
        (w * step.rsample_do(z, [1, 3], .3, ctx)).sum().backward()
    assert (n.adjoint, n.pinned, n.gdo, n.module) == (1, 1, 0, 1)
    step.adjoint_schedule = False
    with _Count(step) as n:
        (w * step.rsample_do(z, [1, 3], v, ctx)).sum().backward()
    assert (n.adjoint, n.module) == (0, 1) and step._rsample_arm[0] == "passes" and 1 <= step._rsample_arm[1] <= 4


def _strade_flow(name, kind, norm, c, seed=0):
    from models import AffineNormalizer, SplineNormalizer, buildFCNormalizingFlow
    a = R.GRAPHS[name]
    torch.manual_seed(seed)
    args = {"in_size": a.shape[0], "hidden": R.hidden_of(name, kind, c), "out_size": 2 if norm == "affine" else 3 * KS - 1,
            "cond_in": c, "adjacency": a}
    if norm == "affine":
        return buildFCNormalizingFlow(1, "StrADE", args, AffineNormalizer, {}).to(DEV)
    return buildFCNormalizingFlow(1, "StrADE", args, SplineNormalizer, {"nb_bins": KS, "tail_bound": TS}).to(DEV)


def test_adjoint_levels_on_and_off_for_a_strade_step():
    step = _strade_flow("d17", "40-24", "affine", 3, seed=3).steps[0]
    cond = step.conditioner
    gen = torch.Generator().manual_seed(1)
    z, ctx, w = cu(.9 * torch.randn(4, 17, generator=gen)), cu(torch.randn(4, 3, generator=gen)), cu(torch.randn(4, 17, generator=gen))
    z.requires_grad_(True)
    v = torch.zeros(4, 3, device=DEV, requires_grad=True)
    idx = [2, 9, 11]
    with _Count(step) as n:                                           # the default: the passes
        x = step.rsample_do(z, idx, v, ctx)
        assert step._intervene_arm == "strade"
        (w * x).sum().backward()
    assert n.adjoint == 0 and step._rsample_arm[0] == "passes" and 1 <= step._rsample_arm[1] <= cond.depth()
    lam_p, gv_p = z.grad.clone(), v.grad.clone()
    z.grad = v.grad = None
    cond.adjoint_levels = True
    with _Count(step) as n:
        (w * step.rsample_do(z, idx, v, ctx)).sum().backward()
    assert (n.adjoint, n.pinned, n.gdo, n.module) == (1, 1, 1, 1) and step._rsample_arm == ("adjoint", 0)
    assert (z.grad - lam_p).abs().max().item() <= 1e-4 * lam_p.abs().max().item()      # (the arms agree: GTOL of test_gpu_parity.py)
    assert (v.grad - gv_p).abs().max().item() <= 1e-4 * max(gv_p.abs().max().item(), w.abs().max().item())
    assert _zeros_exactly(z.grad[:, idx])


def test_coupling_and_a_deterministic_dag_step_take_the_passes():
    step = _flow("coupling", 6, 2, [16]).steps[0]
    z, ctx, w = _inputs(4, 6, 2, 2)
    z.requires_grad_(True)
    v = torch.tensor(.25, device=DEV, requires_grad=True)
    with _Count(step) as n:
        x = step.rsample_do(z, [0, 4], v, ctx)
        assert step._intervene_arm == "passes"
        (w * x).sum().backward()
    assert n.adjoint == 0 and step._rsample_arm == ("passes", 1) and v.grad.dim() == 0
    assert _zeros_exactly(z.grad[:, [0, 4]])
    step = _dag_step(6)
    z, _, w = _inputs(5, 6, 0, 3)
    z.requires_grad_(True)
    with _Count(step) as n:
        x = step.rsample_do(z, [2], torch.zeros(1, device=DEV, requires_grad=True))
        assert step._intervene_arm == "levels"
        (w * x).sum().backward()
    assert n.adjoint == 0 and step._rsample_arm[0] == "passes" and 1 <= step._rsample_arm[1] <= step.conditioner.depth()


@pytest.mark.parametrize("kind", ["made", "coupling"])
def test_every_variable_pinned_asks_no_conditioner(kind):
    step = _flow(kind, 5, 2, [19]).steps[0]
    z, ctx, w = _inputs(4, 5, 2, 4)
    z.requires_grad_(True)
    v = cu(torch.randn(4, 5, generator=torch.Generator().manual_seed(1))).requires_grad_(True)
    for p in step.parameters():
        p.grad = None
    with _Count(step) as n:
        x = step.rsample_do(z, [4, 0, 2, 1, 3], v, ctx)
        (w * x).sum().backward()
    assert (n.adjoint, n.module) == (0, 0)
    assert poison.differing(x.detach()[:, [4, 0, 2, 1, 3]].contiguous(), v.detach()) == 0
    assert _zeros_exactly(z.grad) and poison.differing(v.grad, w[:, [4, 0, 2, 1, 3]].contiguous()) == 0
    assert all(p.grad is None or float(p.grad.abs().max()) == 0 for p in step.parameters())


# ------------------------------------------------------------------------------------------------ 6. forward identity
def _arm_steps():
    return [("columns", lambda: _flow("made", 5, 2, [19], seed=3), 2, 5),
            ("columns", lambda: _flow("made", 5, 2, [19], seed=3, out=4, integrand=[16, 16]), 2, 5),
            ("strade", lambda: _strade_flow("d17", "40-24", "affine", 3, seed=4), 3, 17),
            ("strade", lambda: _strade_flow("d17", "40-24", "spline", 0, seed=4), 0, 17),
            ("levels", lambda: _dag_step(6), 0, 6),
            ("passes", lambda: _flow("coupling", 5, 2, [19], seed=3), 2, 5)]


@pytest.mark.parametrize("arm,make,c,d", _arm_steps(),
                         ids=["columns", "columns-monotonic", "strade-affine", "strade-spline", "levels", "passes"])
def test_forward_is_intervene_and_counterfactual_bit_for_bit(arm, make, c, d):
    flow = make()
    step = flow if not hasattr(flow, "steps") else flow.steps[0]
    gen = torch.Generator().manual_seed(7)
    z = cu(.7 * torch.randn(9, d, generator=gen)).requires_grad_(True)
    ctx = cu(torch.randn(9, c, generator=gen)) if c else None
    for idx, val in (([1], .5), ([d - 1, 0], cu(torch.randn(2, generator=gen)).requires_grad_(True)),
                     ([2, 1], cu(torch.randn(9, 2, generator=gen)).requires_grad_(True)), ([], 0.)):
        x = step.rsample_do(z, idx, val, ctx)
        assert step._intervene_arm == arm or not idx
        held = None if not torch.is_tensor(val) else val.detach()
        want = step.intervene(z.detach(), idx, val if held is None else held, ctx)
        assert x.requires_grad and poison.differing(x.detach(), want) == 0, idx
        xc = step.rcounterfactual(x.detach().requires_grad_(True), idx, val, ctx)
        assert xc.requires_grad
        assert poison.differing(xc.detach(), step.counterfactual(x.detach(), idx, val if held is None else held, ctx)) == 0, idx
    if hasattr(flow, "steps"):
        assert poison.differing(flow.rsample_do(z, [1], .5, ctx).detach(), flow.intervene(z.detach(), [1], .5, ctx)) == 0


@pytest.mark.parametrize("kind", ["made", "coupling"])
def test_an_empty_do_index_is_rsample_in_value_and_every_gradient(kind):
    flow = _flow(kind, 5, 2, [19], seed=8)
    step = flow.steps[0]
    z, ctx, w = _inputs(7, 5, 2, 6)
    results = []
    for fn in (lambda zl, cl: step.rsample(zl, cl), lambda zl, cl: step.rsample_do(zl, [], 0., cl),
               lambda zl, cl: flow.rsample_do(zl, torch.zeros(0, dtype=torch.long), torch.zeros(0, device=DEV), cl)):
        for p in flow.parameters():
            p.grad = None
        zl, cl = z.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
        x = fn(zl, cl)
        (w * x).sum().backward()
        results.append([x.detach(), zl.grad, cl.grad] + [p.grad.clone() for p in flow.parameters()])
    for other in results[1:]:
        assert all(poison.differing(a, b) == 0 for a, b in zip(results[0], other))


# ----------------------------------------------------------------------------------- 7. whole gradients against fp64
def _dag_cfn(cond, P, dtype):
    layers = _pairs(P, "steps.0.conditioner.embedding_net.")
    d = cond.in_size

    def cfn(v):
        e = O.dag_masked_inputs(v, P["steps.0.conditioner.A"], bool(cond.s_thresh), 0., False, False, 1., None, None, None, True)
        return O.mlp(e, layers).view(v.shape[0], d, -1)
    return cfn


def _dag_constraints(cond, P, dtype):
    t = lambda b: b.detach().cpu().to(dtype)
    alpha = torch.clamp(t(cond.alpha), max=1.) * float(cond.alpha_factor)
    return O.dag_loss(P["steps.0.conditioner.A"], alpha, int(cond.exponent), t(cond.lambd), t(cond.c), t(cond.dag_const),
                      t(cond.l1_weight))


def _whole_case(kind, c):
    """(flow, d, factory (P, ctx leaf, dtype) -> conditioner fn, depth of the unrolled passes, constraint term (P, dtype) or None)"""
    if kind in ("made", "coupling"):
        flow = _flow(kind, 5, c, [19], seed=7 + c)
        return flow, 5, (lambda P, cl, dt: flow_steps(flow, P, cl)[0][0]), (4 if kind == "made" else 1), None
    if kind in ("strade-affine", "strade-spline"):
        flow = _strade_flow("d17", "40-24", kind.split("-")[1], c, seed=8)
        cond = flow.steps[0].conditioner
        cond.adjoint_levels = True

        def factory(P, cl, dt):
            ls = cond._layers()
            names = {id(p): n for n, p in flow.named_parameters()}
            layers = [(P[names[id(l.weight)]], P[names[id(l.bias)]]) for l in ls]
            masks = [l.mask.detach().cpu().to(dt) for l in ls]
            return lambda x: R.masked_forward(layers, masks, x, cl if c else x.new_zeros(x.shape[0], 0))[0]
        return flow, 17, factory, cond.depth(), None
    flow = _dag_flow()
    cond = flow.steps[0].conditioner
    return flow, 6, (lambda P, cl, dt: _dag_cfn(cond, P, dt)), cond.depth(), (lambda P, dt: _dag_constraints(cond, P, dt))


def _dag_flow(d=6):
    """the flow around test_gpu_rsample._dag_step's step (that helper returns the step alone)"""
    from models import AffineNormalizer, DAGConditioner, buildFCNormalizingFlow
    torch.manual_seed(21)
    flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [16, 16], "out_size": 2, "hot_encoding": True},
                                  AffineNormalizer, {})
    cond = flow.steps[0].conditioner
    cond.A.data.copy_(torch.tril(torch.rand(d, d) + .1, -1) * (torch.rand(d, d) < .6).float())
    cond.stoch_gate = cond.noise_gate = False
    cond.invalidate_caches()
    return flow.to(DEV)


WHOLE = [("made", 0), ("made", 3), ("coupling", 0), ("coupling", 3), ("strade-affine", 0), ("strade-affine", 3),
         ("strade-spline", 0), ("strade-spline", 3), ("dag", 0)]


@pytest.mark.parametrize("method", ["rsample_do", "rcounterfactual"])
@pytest.mark.parametrize("vshape", ["S", "BS"])
@pytest.mark.parametrize("kind,c", WHOLE, ids=["%s-c%d" % w for w in WHOLE])
def test_whole_gradients_against_fp64(kind, c, vshape, method):
    """L = sum w x + loss_do(x, targets = do_index), x = rsample_do(z, idx, v, c) (or rcounterfactual(x0, idx, v, c)): gradients
    for z (x0), v, c and every parameter against fp64 autograd through the unrolled pinned passes of
    adjoint_do_ref.intervene_t; the comparator is the same restatement in fp32 on plain torch.  Every tensor is held to the
    rule on its own error; the floor is 1e-6 of the largest entry of its group (z, v, c, all parameters), as in
    tests/test_gpu_rsample.py."""
    B = 6
    flow, d, factory, depth, constraints = _whole_case(kind, c)
    step = flow.steps[0]
    idx = [1, d - 2] if d > 5 else [1, 3]
    gen = torch.Generator().manual_seed(40 + c + d)
    z0 = .7 * torch.randn(B, d, generator=gen)
    ctx0 = torch.randn(B, c, generator=gen) if c else None
    w = torch.randn(B, d, generator=gen)
    v0 = .5 * torch.randn(*((len(idx),) if vshape == "S" else (B, len(idx))), generator=gen)
    zd, vd = cu(z0).requires_grad_(True), cu(v0).requires_grad_(True)
    cd = cu(ctx0).requires_grad_(True) if c else None
    for p in flow.parameters():
        p.grad = None
    x = getattr(flow, method)(zd, idx, vd, cd)
    ((cu(w) * x).sum() + flow.loss_do(x, idx, context=cd)).backward()
    assert step._rsample_arm[0] == ("adjoint" if kind in ("made", "strade-affine", "strade-spline") else "passes")
    names = [n for n, _ in flow.named_parameters()]
    got = {"z": zd.grad, "v": vd.grad, **({"c": cd.grad} if c else {}), **{n: p.grad for n, p in flow.named_parameters()}}
    assert tuple(vd.grad.shape) == tuple(v0.shape)
    spline = kind == "strade-spline"
    fwd = (lambda xx, h: S.forward(xx, h, KS, TS)) if spline else O.affine_forward
    inv = (lambda zz, h: S.inverse(zz, h, KS, TS)) if spline else O.affine_inverse
    pin = D.pin_of(idx, list(range(d)), d)

    def reference(dtype):
        P = leaves(flow, dtype)
        zl, vl = z0.to(dtype).requires_grad_(True), v0.to(dtype).requires_grad_(True)
        cl = ctx0.to(dtype).requires_grad_(True) if c else torch.zeros(B, 0, dtype=dtype)
        cfn = factory(P, cl, dtype)
        vals = torch.zeros(B, d, dtype=dtype).index_add(1, torch.as_tensor(idx), vl.expand(B, len(idx)))
        zz = fwd(zl, cfn(zl))[0] if method == "rcounterfactual" else zl      # the abduction, differentiable
        xx = D.intervene_t(cfn, depth, zz, pin, vals, inv)
        L = (w.to(dtype) * xx).sum() + D.loss_do_t(cfn, xx, pin, fwd)
        if constraints is not None:
            L = L + constraints(P, dtype)
        wrt = [zl, vl] + ([cl] if c else []) + [P[n] for n in names]
        grads = torch.autograd.grad(L, wrt, allow_unused=True)
        grads = [torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, wrt)]
        return dict(zip(["z", "v"] + (["c"] if c else []) + names, grads))

    r64, r32 = reference(torch.float64), reference(torch.float32)
    scale_p = max(r64[n].abs().max().item() for n in names)
    if method == "rsample_do":
        assert _zeros_exactly(zd.grad[:, idx])                       # dL/dz is exactly +0 at the pinned columns
    for name, want in r64.items():
        g_ = got[name]
        g_ = torch.zeros_like(want) if g_ is None else g_
        scale = want.abs().max().item() if name in ("z", "v", "c") else scale_p
        _rule("whole gradients, %s + loss_do vs plain-torch fp32, both against fp64" % method,
              "%s c=%d v=%s %s" % (kind, c, vshape, name), _err(g_, want), (r32[name].double() - want).abs().max().item(), scale)


# --------------------------------------------------------------------------------------------- 8. Monotonic + MADE
def test_monotonic_made_adjoint_arm_against_the_passes_arm():
    d, c, B = 5, 2, 8
    step = _flow("made", d, c, [19], seed=21, out=4, integrand=[16, 16]).steps[0]
    cond, norm = step.conditioner, step.normalizer
    z, ctx, w = _inputs(B, d, c, 9)
    g = cu(torch.randn(B, d, generator=torch.Generator().manual_seed(4)))
    order = plan_of(cond)["var_of_step"]
    for name, pin in _patterns(order, d):
        idx = [int(i) for i in pin.nonzero().flatten()]
        if not idx or len(idx) == d:
            continue
        x = step.intervene(z, idx, .3, ctx)
        # the operands both arms share, measured on the device at the sample (benign: the values pinned are ordinary)
        with torch.enable_grad():
            h = cond(x.detach().requires_grad_(True), ctx)
            zz, jac = norm(x, h, ctx)
            dzdh, = torch.autograd.grad(zz, h, torch.ones_like(zz))
        law = D.law_sweep_do(made_layers(cond), plan_of(cond), c, c64(x), c64(ctx), c64(g), c64(jac), c64(dzdh), pin)
        out = {}
        for on in (True, False):
            step.adjoint_schedule = on
            lam, gv, _, _ = step._rsample_do_backward(x, ctx, [], g, tuple(idx), False, True)
            assert step._rsample_arm[0] == ("adjoint" if on else "passes")
            assert _zeros_exactly(lam[:, idx])
            out[on] = (lam, gv)
        _rule("pinned MADE adjoint kernel vs passes, both against the fp64 law, lambda", "monotonic d=5 c=2 %s" % name,
              _err(out[True][0], law[0]), _err(out[False][0], law[0]), law[0].abs().max().item())
        _rule("pinned MADE adjoint kernel vs passes, both against the fp64 law, gdo", "monotonic d=5 c=2 %s" % name,
              _err(out[True][1], law[1][:, idx]), _err(out[False][1], law[1][:, idx]),
              max(law[1].abs().max().item(), c64(g).abs().max().item()))


# ---------------------------------------------------------------------------------------------- 9. extremes and edges
@pytest.mark.parametrize("adjoint", [True, False], ids=["adjoint", "passes"])
def test_an_extreme_pinned_value_end_to_end(adjoint):
    """the last-degree variable of an Affine + MADE step pinned at 3e38: nothing reads it, so every gradient is finite and
    dL/dv is g at that column exactly"""
    d, c, B = 5, 2, 6
    flow = _flow("made", d, c, [19], seed=5)
    step = flow.steps[0]
    step.adjoint_schedule = adjoint
    last = int(plan_of(step.conditioner)["var_of_step"][d - 1])
    z, ctx, w = _inputs(B, d, c, 8)
    z.requires_grad_(True)
    ctx.requires_grad_(True)
    v = torch.full((B, 1), 3e38, device=DEV, requires_grad=True)
    for p in flow.parameters():
        p.grad = None
    x = flow.rsample_do(z, [last], v, ctx)
    assert bool((x.detach()[:, last] == 3e38).all())
    (w * x).sum().backward()
    assert step._rsample_arm[0] == ("adjoint" if adjoint else "passes")
    for name, t in [("z", z.grad), ("c", ctx.grad), ("v", v.grad)] + [(n, p.grad) for n, p in flow.named_parameters()]:
        assert t is not None and torch.isfinite(t).all(), name
    assert poison.differing(v.grad, w[:, last:last + 1].contiguous()) == 0
    assert _zeros_exactly(z.grad[:, last])


def test_empty_batch_launches_nothing():
    from gnf_hip import ops
    flow = _flow("made", 5, 2, [19])
    step = flow.steps[0]
    z = torch.zeros(0, 5, device=DEV, requires_grad=True)
    v = torch.zeros(2, device=DEV, requires_grad=True)
    with _Count(step) as n:
        x = flow.rsample_do(z, [1, 2], v, torch.zeros(0, 2, device=DEV))
        assert tuple(x.shape) == (0, 5)
        x.sum().backward()
    assert (n.adjoint, n.module) == (0, 0) and tuple(z.grad.shape) == (0, 5) and tuple(v.grad.shape) == (2,)
    cond = step.conditioner
    e = torch.zeros(0, 5, device=DEV)
    lam, gdo = _made_solve(cond, e, e, e, torch.zeros(0, 5, 2, device=DEV), torch.zeros(0, 2, device=DEV),
                           torch.ones(5, dtype=torch.uint8, device=DEV), True)
    assert tuple(lam.shape) == (0, 5) and tuple(gdo.shape) == (0, 5)
    sflow = _strade_flow("d17", "40-24", "affine", 3, seed=5)
    scond = sflow.steps[0].conditioner
    scond.adjoint_levels = True
    e = torch.zeros(0, 17, device=DEV)
    lam, gdo = _strade_solve(scond, e, e, e, torch.zeros(0, 17, 2, device=DEV), torch.zeros(0, 3, device=DEV),
                             torch.ones(17, dtype=torch.uint8, device=DEV), True)
    assert tuple(lam.shape) == (0, 17) and tuple(gdo.shape) == (0, 17)
