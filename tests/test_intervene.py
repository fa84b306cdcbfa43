"""CPU (-m "not gpu"): the host half of interventional sampling (NormalizingFlowStep.intervene / counterfactual).

The law.  The project's conditioners and normalizers evaluate on the GPU only, so the passes arm -- the yardstick of the two
fast arms -- is run here through `intervene` itself on plain-torch fp32 stand-ins that read the real modules' parameters,
masks and adjacency (Conditioner / Normalizer plug-ins, which the passes arm accepts like any other), and compared with the
same law restated below in a dozen lines of fp64 torch.  The bound: one free column costs an inner product of <= 21 terms per
layer, an exponential or a spline bin and a division, each rounded to eps32 = 6e-8, and a column's error reaches the later
ones with the conditioner's gain, O(1) at the initialisation scale of these nets: d = 5 columns stay below 2e-5 max(1, |x|).

Then: the argument errors, P = {} against invert, P = everything without a conditioner call, the launch plan of the column
sweep under pins against a brute-force enumeration, and the new C-ABI symbol with its host-side argument checks."""
import ctypes
import itertools
import os
import re

import pytest
import torch

import spline_ref
from oracle import gnf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, HID, B = 5, [16], 3
K_BINS, TAIL = 4, 3.


# ----------------------------------------------------------------------------------------------- plain-torch stand-ins
def _conditioner_fn(kind, cond, cast):
    """x -> h [B, d, out] of the real module `cond` in plain torch, every tensor through `cast` (fp32 or fp64)"""
    from models.Conditionners.Conditioner import linear_pairs
    if kind == "MADE":
        layers = [(cast(l.mask) * cast(l.weight), cast(l.bias)) for l in cond.masked_autoregressive_net.masked_layers()]
        return lambda x: O.mlp(x, layers).view(x.shape[0], -1, x.shape[1]).permute(0, 2, 1)
    if kind == "Coupling":
        layers = [(cast(W), cast(b)) for W, b in linear_pairs(cond.embeding_net.net)]
        const = cast(cond.constants)
        return lambda x: torch.cat((const.unsqueeze(0).expand(x.shape[0], -1, -1),
                                    O.mlp(x[:, :cond.indep_size], layers).view(x.shape[0], cond.cond_size, cond.out_size)), 1)
    layers = [(cast(W), cast(b)) for W, b in linear_pairs(cond.embedding_net.net)]
    A = cast(cond.A)

    def dag(x):                                          # deterministic gate, no threshold: the copies are x * A[i]
        e = x.unsqueeze(1) * A.unsqueeze(0)
        if cond.hot_encoding:
            e = torch.cat((e, torch.eye(A.shape[0], dtype=x.dtype).unsqueeze(0).expand(x.shape[0], -1, -1)), 2)
        return O.mlp(e.reshape(-1, e.shape[2]), layers).view(x.shape[0], A.shape[0], -1)
    return dag


def _inverse_fn(norm):
    if norm == "affine":
        return O.affine_inverse
    return lambda z, h: spline_ref.inverse(z, h, K_BINS, TAIL)


def _host_step(kind, norm, seed=0):
    """(a NormalizingFlowStep of fp32 stand-ins, the fp64 conditioner function, the inverse function, depth, the stand-in)"""
    from models import AutoregressiveConditioner, CouplingConditioner, DAGConditioner
    from models.Conditionners.Conditioner import Conditioner
    from models.Normalizers.Normalizer import Normalizer
    from models.NormalizingFlow import NormalizingFlowStep
    out = 2 if norm == "affine" else 3 * K_BINS - 1
    torch.manual_seed(seed)
    if kind == "MADE":
        real = AutoregressiveConditioner(D, list(HID), out)
    elif kind == "Coupling":
        real = CouplingConditioner(D, list(HID), out)
    else:
        real = DAGConditioner(D, list(HID), out)
        real.stoch_gate = False
        with torch.no_grad():
            real.A.copy_(torch.tril(torch.rand(D, D) + .1, -1) * (torch.rand(D, D) < .6).float())
            real.A.diagonal(-1).fill_(.8)                # a chain through every variable: depth d - 1
        real.invalidate_caches()
    depth = real.depth()
    inv = _inverse_fn(norm)

    class HostConditioner(Conditioner):
        calls = 0

        def forward(self, x, context=None):
            assert context is None
            self.calls += 1
            return _conditioner_fn(kind, real, lambda t: t.detach().float())(x)

        def depth(self):
            return depth

    class HostNormalizer(Normalizer):
        def inverse_transform(self, z, h, context=None):
            return inv(z, h)

    cond = HostConditioner()
    return NormalizingFlowStep(cond, HostNormalizer()), _conditioner_fn(kind, real, lambda t: t.detach().double()), inv, depth, cond


def law64(z, cfn, inv, depth, idx, vals):
    """the passes arm in fp64: x <- where(pinned, v, normalizer^-1(z, conditioner(x))) from where(pinned, v, 0)"""
    pin = torch.zeros(z.shape[1], dtype=torch.bool)
    pin[list(idx)] = True
    V = torch.zeros_like(z)
    V[:, list(idx)] = vals
    x = torch.where(pin, V, torch.zeros_like(z))
    for _ in range(depth + 1):
        previous = x
        x = torch.where(pin, V, inv(z, cfn(x)))
        if torch.equal(x, previous):
            break
    return x


# ------------------------------------------------------------------------- the Monotonic inverse is a bisection
# MonotonicNormalizer.inverse_transform: 20 halvings of [-20, 20], so every x it returns lies on a lattice of pitch QUANTUM,
# and a comparison z_mid > z that two evaluations decide differently moves the result by whole quanta, however accurate
# both are.  An element is NEAR A TIE when the fp64 bisection passes within TIE max(1, |z|) of z at any of its steps: 4 eps32,
# eight roundings of half an ulp -- the nine terms of the test nets' quadrature sum and its offset.  The rule reads the
# fp64 reference alone.
QUANTUM = 40. / 2 ** 20
TIE = 4 * 2. ** -24


def bisection_margins64(z, h, layers, nb_steps):
    """[B, d]: min over the 20 steps of the oracle's bisection (monotonic_inverse) of |z_mid - z| / max(1, |z|)"""
    x_max = torch.full_like(z, 20.)
    x_min = -x_max
    margin = torch.full_like(z, float("inf"))
    for _ in range(20):
        x_mid = (x_max + x_min) / 2
        z_mid = O.monotonic_integral(x_mid, h, layers, nb_steps) + h[:, :, 0]
        margin = torch.minimum(margin, (z_mid - z).abs() / z.abs().clamp(min=1.))
        left = z_mid > z
        x_max, x_min = torch.where(left, x_mid, x_max), torch.where(left, x_min, x_mid)
    return margin


def test_tie_rule_on_the_fp64_reference():
    """the rule tests/test_gpu_intervene.py excuses whole quanta by, checked where no GPU is needed: it flags a constructed
    tie, and on the inputs of that test it selects few elements -- under 5 % of the free ones"""
    import test_gpu_intervene as G
    from models.Conditionners.Conditioner import linear_pairs
    near = free = 0
    for d, hidden in ((6, [16]), (17, [])):
        step = G._made_step(d, 0, hidden, "monotonic", seed=7 * d, device="cpu")
        layers = [(W.detach().double(), b.detach().double()) for W, b in linear_pairs(step.normalizer.integrand_net.net)]
        S = int(step.normalizer.nb_steps)
        inv64 = lambda z, h: O.monotonic_inverse(z, h, layers, S)
        z, _, v = G._inputs(17, d, 0, seed=17 + d, device="cpu")
        cfn64 = G._made64(step.conditioner, torch.zeros(17, 0, dtype=torch.float64))
        for idx in ((), (0,), tuple(range(0, d, 2))):
            x64 = law64(z.double(), cfn64, inv64, d - 1, idx, v[:, list(idx)].double())
            m = bisection_margins64(z.double(), cfn64(x64), layers, S)
            cols = [i for i in range(d) if i not in idx]
            near += int((m[:, cols] < TIE).sum())
            free += 17 * len(cols)
        # a tie by construction: the first midpoint is x = 0, where the integral vanishes and z_mid is the offset h0
        h = cfn64(x64)
        tied = z.double().clone()
        tied[:, 0] = h[:, 0, 0]
        assert bool((bisection_margins64(tied, h, layers, S)[:, 0] == 0.).all())
    print("near a tie: %d of %d free elements" % (near, free))
    assert near <= .05 * free, (near, free)


PINS = [(), (0,), (D - 1,), (1, 2), (0, 2, 4), (3, 1)]


@pytest.mark.parametrize("norm", ["affine", "spline"])
@pytest.mark.parametrize("kind", ["Coupling", "MADE", "DAG"])
def test_passes_arm_is_the_law(kind, norm):
    step, cfn64, inv, depth, _ = _host_step(kind, norm)
    gen = torch.Generator().manual_seed(7)
    z = .7 * torch.randn(B, D, generator=gen)
    for idx in PINS:
        for vals in (.5, torch.randn(len(idx), generator=gen), torch.randn(B, len(idx), generator=gen)):
            x = step.intervene(z, list(idx), vals)
            assert step._intervene_arm == "passes" and x.dtype == torch.float32 and not x.requires_grad
            v64 = (torch.as_tensor(vals).float().double().expand(B, len(idx)) if idx else torch.zeros(B, 0).double())
            want = law64(z.double(), cfn64, inv, depth, idx, v64)
            err = (x.double() - want).abs().max().item()
            print("%s %s pins %s: |intervene - law64| %.3e, max|x| %.3e" % (kind, norm, idx, err, want.abs().max().item()))
            assert err <= 2e-5 * max(1., want.abs().max().item()), (kind, norm, idx, err)
            if idx:
                assert torch.equal(x[:, list(idx)], torch.as_tensor(vals).float().expand(B, len(idx)))     # the caller's bits


@pytest.mark.parametrize("kind", ["Coupling", "MADE", "DAG"])
def test_empty_pin_set_is_invert_and_full_pin_set_asks_no_conditioner(kind):
    step, _, _, depth, cond = _host_step(kind, "affine", seed=3)
    z = .7 * torch.randn(B, D, generator=torch.Generator().manual_seed(1))
    assert torch.equal(step.intervene(z, [], 0.), step.invert(z))
    assert torch.equal(step.intervene(z, torch.zeros(0, dtype=torch.long), torch.zeros(0)), step.invert(z))
    cond.calls = 0
    v = torch.randn(B, D, generator=torch.Generator().manual_seed(2))
    perm = [3, 0, 4, 1, 2]
    x = step.intervene(z, perm, v)
    assert cond.calls == 0 and torch.equal(x[:, perm], v)
    # a tensor index, and counterfactual = forward then intervene (the stand-ins have no forward: spy on the two calls)
    x2 = step.intervene(z, torch.tensor(perm), v)
    assert torch.equal(x, x2)
    seen = []
    step.forward = lambda x, context=None: (seen.append("forward") or (z, None))
    got = step.counterfactual(torch.zeros(B, D), [1], 2.)
    assert seen == ["forward"] and torch.equal(got, step.intervene(z, [1], 2.))


def test_argument_errors():
    from models import AffineNormalizer, AutoregressiveConditioner, DAGConditioner, buildFCNormalizingFlow
    from models.NormalizingFlow import CNNormalizingFlow
    step, _, _, _, _ = _host_step("MADE", "affine")
    z = torch.zeros(B, D)
    for bad_index in ([1, 1], [0, 2, 0], [D], [-1], [1.5], [True], torch.tensor([1., 2.]), torch.tensor([[1, 2]])):
        with pytest.raises(ValueError):
            step.intervene(z, bad_index, 0.)
    for bad_value in (torch.zeros(3), torch.zeros(B + 1, 2), torch.zeros(B, 3), torch.zeros(B, 2, 1), "1", None):
        with pytest.raises(ValueError):
            step.intervene(z, [1, 2], bad_value)
    with pytest.raises(ValueError):
        step.intervene(torch.zeros(D), [1], 0.)
    flow = buildFCNormalizingFlow(2, AutoregressiveConditioner, {"in_size": D, "hidden": [8], "out_size": 2}, AffineNormalizer, {})
    for call in (flow.intervene, flow.counterfactual):
        with pytest.raises(ValueError, match="ONE-step"):
            call(z, [1], 0.)
    cn = CNNormalizingFlow([], None, [])
    for call in (cn.intervene, cn.counterfactual):
        with pytest.raises(ValueError, match="ONE-step"):
            call(z, [1], 0.)
    dag = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": 4, "hidden": [8], "out_size": 2}, AffineNormalizer, {})
    assert dag.steps[0].conditioner.deterministic_importance() is None          # the state rsample refuses
    for call in (dag.intervene, dag.counterfactual, dag.steps[0].intervene):
        with pytest.raises(ValueError, match="stochastic"):
            call(torch.zeros(2, 4), [1], 0.)


def test_single_step_flow_delegates():
    from models.NormalizingFlow import FCNormalizingFlow
    step, _, _, _, _ = _host_step("Coupling", "affine")
    flow = FCNormalizingFlow([step], None)
    z = .7 * torch.randn(B, D, generator=torch.Generator().manual_seed(4))
    assert torch.equal(flow.intervene(z, [0, 4], 1.), step.intervene(z, [0, 4], 1.))


# ------------------------------------------------------------------------------------------------- the launch plan
def _brute_force_launches(var_of_step, pinned):
    """step by step: which launch a step belongs to, from the definition -- a launch ends at a free step; the pinned steps
    since the previous launch's end ride along; pinned steps after the last free one belong to none"""
    launches, current = [], []
    for t, v in enumerate(var_of_step):
        current.append(t)
        if v not in pinned:
            launches.append((current[0], current[-1] + 1))
            current = []
    return launches


@pytest.mark.parametrize("d", range(1, 9))
def test_launch_plan_under_every_pin_set(d):
    from models.Conditionners.AutoregressiveConditioner import made_do_launches
    gen = torch.Generator().manual_seed(d)
    for order in (list(range(d)), torch.randperm(d, generator=gen).tolist()):
        for n in range(d + 1):
            for pinned in itertools.combinations(range(d), n):
                plan = made_do_launches(order, pinned)
                assert plan == _brute_force_launches(order, set(pinned))
                free = [t for t, v in enumerate(order) if v not in pinned]
                assert len(plan) == len(free) and [t1 - 1 for _, t1 in plan] == free        # one launch per free column
                covered = [t for t0, t1 in plan for t in range(t0, t1)]
                last = free[-1] + 1 if free else 0
                assert covered == list(range(last))                                          # contiguous, the trailing run dropped
                for t0, t1 in plan:
                    assert all(order[t] in pinned for t in range(t0, t1 - 1)) and order[t1 - 1] not in pinned


# -------------------------------------------------------------------------------------------------------- the ABI
def test_symbol_exported_declared_and_bound():
    from gnf_hip import abi
    header = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = abi.load()                                             # dlopen works without a GPU
    name = "gnf_made_prefix_do"
    assert hasattr(lib, name) and name in abi.SIGNATURES
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
    assert m is not None
    assert len([a for a in m.group(1).split(",") if a.strip()]) == len(abi.SIGNATURES[name][1]) == 17
    assert abi.ABI_VERSION == 11 and lib.gnf_abi_version() == 11
    assert "#define GNF_ABI_VERSION 11" in header


def test_argument_checks_answer_before_any_launch():
    from gnf_hip import abi
    from test_context_invert_host import _host_net
    lib = abi.load()
    p = ctypes.c_void_p(64)                                      # never dereferenced: every call below is refused or empty
    net = _host_net(5, [7, 7], 2)
    ref = ctypes.byref(net)
    NONE, AFFINE, SPLINE = abi.MADE_NORM_NONE, abi.MADE_NORM_AFFINE, abi.MADE_NORM_SPLINE
    do = lib.gnf_made_prefix_do
    for pin in (None, p):
        assert do(ref, -1, p, p, p, p, p, 0, 5, AFFINE, 0, 0., pin, 4, p, 1 << 20, None) == -1          # negative cond_in
        assert do(ref, 2, None, p, p, p, p, 0, 5, AFFINE, 0, 0., pin, 4, p, 1 << 20, None) == -1        # null context, B > 0
        assert do(ref, 0, None, p, p, None, p, 0, 5, AFFINE, 0, 0., pin, 4, p, 1 << 20, None) == -1     # null x, B > 0
        assert do(ref, 0, None, p, p, p, p, 0, 6, AFFINE, 0, 0., pin, 4, p, 1 << 20, None) == -1        # t1 > d
        assert do(ref, 0, None, p, p, p, p, 0, 5, 7, 0, 0., pin, 4, p, 1 << 20, None) == -1             # unknown mode
        assert do(ref, 0, None, p, p, p, p, 0, 5, SPLINE, 1, 3., pin, 4, p, 1 << 20, None) == -1        # bins
        assert do(ref, 0, None, p, p, p, p, 0, 5, SPLINE, 4, 3., pin, 4, p, 1 << 20, None) == -2        # out < 3 K - 1
        assert do(ref, 0, None, p, p, p, None, 2, 3, NONE, 0, 0., pin, 4, p, 1 << 20, None) == -1       # NONE without h_out
        assert do(ref, 0, None, p, None, p, p, 0, 5, AFFINE, 0, 0., pin, 4, p, 1 << 20, None) == -1     # AFFINE without z
        assert do(ref, 2, None, None, None, None, None, 0, 5, AFFINE, 0, 0., pin, 0, None, 0, None) == 0        # B == 0
        assert do(ref, 2, None, None, None, None, None, 0, 5, NONE, 0, 0., pin, 0, None, 0, None) == (0 if pin else -1)
        assert do(ref, 2, None, None, None, None, None, 3, 3, AFFINE, 0, 0., pin, 4, None, 0, None) == 0        # t1 == t0
        assert do(ref, 0, None, p, p, p, p, 1, 2, AFFINE, 0, 0., pin, 4, None, 0, None) == -3           # a step needs ws
    assert do(ref, 0, None, p, p, p, p, 0, 2, NONE, 0, 0., None, 4, p, 1 << 20, None) == -1             # a run without a table


# ------------------------------------------------------------------------------------------------------ the driver
def test_driver_do_option():
    import train_uci
    args = train_uci.parse(["-dataset", "power", "-sample", "4", "-do", "1=0.5", "3=-2"])
    assert args.do == ["1=0.5", "3=-2"] and train_uci.parse_do(args.do, 6) == ([1, 3], [.5, -2.])
    assert train_uci.parse(["-dataset", "power", "-sample", "4"]).do is None
    with pytest.raises(SystemExit):
        train_uci.parse(["-dataset", "power", "-do", "1=2"])                    # -do needs -sample N
    for bad in (["1"], ["x=1"], ["1=y"], ["1.5=2"], ["=2"]):
        with pytest.raises(ValueError, match="COL=VALUE"):
            train_uci.parse_do(bad, 6)


def test_index_dtypes():
    step, _, _, _, _ = _host_step("MADE", "affine")
    z = torch.zeros(B, D)
    for dtype in (torch.float64, torch.float16, torch.complex64, torch.complex128, torch.bool):
        with pytest.raises(ValueError):
            step.intervene(z, torch.zeros(1).to(dtype), 0.)
    for dtype in (torch.int8, torch.uint8, torch.int32, torch.int64):
        assert torch.equal(step.intervene(z, torch.tensor([1], dtype=dtype), 2.)[:, 1], torch.full((B,), 2.))
