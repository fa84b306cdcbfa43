"""Conditional flows on the GPU (cond_in > 0): the group-bias kernels of csrc/gnf_group_bias.hip against the fp32 torch
expression (bit for bit) and fp64, the three conditioners and whole flows against the fp64 references of tests/context_ref.py,
inversion, gnf_hip.dp with a context, and train_uci.py -context_cols.

Ties: a hidden ReLU within fp32 roundoff of zero may legitimately be decided differently by two summation orders; tied samples
(dagmlp_ref.tied_samples on the rows with the context appended) are redrawn with knife_units.resample_off_ties, none is
excluded."""
import pytest
import torch

from conftest import assert_fwd, rel_err
from context_ref import (DAG_GATES, DAG_SHAPES, DEV, coupling64, coupling_tied, d64, dag64, dag_case, flow64, leaves64,
                         made64, made_tied)
from dagmlp_ref import assert_grad, cu, graph_nodes, set_noise
from knife_units import resample_off_ties

pytestmark = pytest.mark.gpu

NODE = "GroupBiasFnBackward"


def sid(shape):
    return "x".join(str(v) for v in shape)


# ------------------------------------------------------------------------------------------- 1. the kernels
def _at(t, off):
    """a copy of t whose first element sits `off` floats behind a 16-byte boundary (off = 0: aligned)"""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
    return v


KERNEL_SHAPES = [(1, 1, 1), (3, 6, 100), (5, 7, 33), (2, 64, 64), (130, 3, 5), (2, 63, 630)]


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=sid)
def test_group_bias_kernels(shape):
    from gnf_hip import ops
    B, G, H = shape
    gen = torch.Generator().manual_seed(B * 1000 + G * 10 + H)
    y, cb, g = (cu(torch.randn(n, H, generator=gen)) for n in (B * G, B, B * G))
    first = {}
    for relu in (True, False):
        pre = y + cb.repeat_interleave(G, 0)
        want = torch.relu(pre) if relu else pre
        want_gpre = torch.where(want > 0, g, torch.zeros_like(g)) if relu else g
        ref_gcb = want_gpre.double().view(B, G, H).sum(1)
        for off in (0, 1, 2, 3):                                  # 0: 16-byte aligned; 1..3: dword-only alignment
            for inplace in (False, True):
                yo, co, go = _at(y, off), _at(cb, off), _at(g, off)
                out = ops.group_bias_fwd(yo, co, G, relu, out=yo if inplace else _at(torch.zeros_like(y), off))
                assert (out.data_ptr() == yo.data_ptr()) == inplace
                assert torch.equal(out, want), ("forward", relu, off, inplace)
                if not inplace:
                    assert torch.equal(yo, y) and torch.equal(co, cb)
                a = _at(want, off) if relu else None
                g_pre, g_cb = ops.group_bias_bwd(go, a, G, g_pre=go if inplace else _at(torch.zeros_like(g), off),
                                                 g_cb=_at(torch.zeros_like(cb), off))
                assert (g_pre.data_ptr() == go.data_ptr()) == inplace
                assert torch.equal(g_pre, want_gpre), ("g_pre", relu, off, inplace)
                assert_grad(g_cb, ref_gcb, "g_cb")
                key = relu
                if key not in first:
                    first[key] = g_cb.clone()
                assert torch.equal(g_cb, first[key]), ("g_cb bits", relu, off, inplace)      # every form, every call
        # the identity without a g_pre array: g itself is the cotangent of y
        g_same, g_cb = ops.group_bias_bwd(g, None, G)
        if not relu:
            assert g_same is g and torch.equal(g_cb, first[False])
    # the autograd node: both gradients from the one backward launch
    for relu in (True, False):
        yl, cl = y.clone().requires_grad_(True), cb.clone().requires_grad_(True)
        out = ops.group_bias(yl, cl, G, relu)
        assert NODE in graph_nodes(out)
        out.backward(g)
        pre = y + cb.repeat_interleave(G, 0)
        assert torch.equal(out.detach(), torch.relu(pre) if relu else pre)
        assert torch.equal(yl.grad, torch.where(pre > 0, g, torch.zeros_like(g)) if relu else g)
        assert torch.equal(cl.grad, first[relu])


def test_group_bias_empty_batch_and_bad_group():
    from gnf_hip import abi, ops
    H, G = 12, 3
    out = ops.group_bias_fwd(torch.zeros(0, H, device=DEV), torch.zeros(0, H, device=DEV), G, True)
    assert tuple(out.shape) == (0, H)
    g_pre, g_cb = ops.group_bias_bwd(torch.zeros(0, H, device=DEV), torch.zeros(0, H, device=DEV), G)
    assert tuple(g_pre.shape) == (0, H) and tuple(g_cb.shape) == (0, H)
    guard = torch.full((4, H), 7., device=DEV)                   # M = 0 launches nothing: the arrays keep their values
    abi.call("gnf_group_bias_fwd", abi.ptr(guard), abi.ptr(guard), abi.ptr(guard), 1, 0, H, G, abi.stream())
    abi.call("gnf_group_bias_bwd", abi.ptr(guard), abi.ptr(guard), abi.ptr(guard), abi.ptr(guard), 0, H, G, abi.stream())
    assert bool((guard == 7.).all())
    y, cb = torch.zeros(7, H, device=DEV), torch.zeros(3, H, device=DEV)
    with pytest.raises(abi.GnfError, match="GNF_ESHAPE"):
        abi.call("gnf_group_bias_fwd", abi.ptr(y), abi.ptr(cb), abi.ptr(y), 1, 7, H, G, abi.stream())
    with pytest.raises(abi.GnfError, match="GNF_ESHAPE"):
        abi.call("gnf_group_bias_bwd", abi.ptr(y), abi.ptr(y), abi.ptr(y), abi.ptr(cb), 7, H, G, abi.stream())
    with pytest.raises(abi.GnfError):
        ops.group_bias(y, cb, G, True)
    with pytest.raises(abi.GnfError):
        ops.group_bias_bwd(y, None, G)
    assert bool((y == 0).all())


# ------------------------------------------------------------------------------------------- 2. DAG conditioner
def run_dag(cond, x, ctx, on, cot):
    """(h, autograd nodes, gradients by name) of one conditioner call with DAGMLP.context_bias = on, same Philox offset"""
    cond.embedding_net.context_bias = on
    cond._gate_calls = 40
    cond.zero_grad(set_to_none=True)
    xd, cd = cu(x).clone().requires_grad_(True), cu(ctx).clone().requires_grad_(True)
    h = cond(xd, cd)
    nodes = graph_nodes(h)
    (h * cu(cot)).sum().backward()
    grads = {n: p.grad.clone() for n, p in cond.named_parameters() if p.grad is not None}
    grads["x"], grads["context"] = xd.grad.clone(), cd.grad.clone()
    return h.detach(), nodes, grads


@pytest.mark.parametrize("case", DAG_GATES)
@pytest.mark.parametrize("hot", [True, False], ids=["hot", "plain"])
@pytest.mark.parametrize("shape", DAG_SHAPES, ids=sid)
def test_dag_conditioner_against_fp64(shape, hot, case):
    B, d, H, c = shape
    cond, (x, ctx, u1, u2), cot, rounds = dag_case(shape, hot, case, DEV)
    in_net = 2 * d if hot else d
    assert tuple(cond.embedding_net.net[0].weight.shape) == (H, in_net + c)
    set_noise(cond, case, u1, u2)
    P = leaves64(cond)
    x64, c64 = x.double().requires_grad_(True), ctx.double().requires_grad_(True)
    h64 = dag64(cond, P, case, x64, c64, u1, u2)
    (h64 * cot.double()).sum().backward()
    ref = {n: p.grad for n, p in P.items()}
    ref["x"], ref["context"] = x64.grad, c64.grad
    assert all(v is not None for v in ref.values())
    h1, nodes1, g1 = run_dag(cond, x, ctx, True, cot)
    h0, nodes0, g0 = run_dag(cond, x, ctx, False, cot)
    assert NODE in nodes1 and NODE not in nodes0, (nodes1, nodes0)
    assert tuple(h1.shape) == (B, d, h64.shape[-1])
    assert_fwd(h1, h64.detach(), what="bias form against fp64")
    assert_fwd(h0, h64.detach(), what="concatenated form against fp64")
    assert_fwd(h1, h0, what="bias form against the concatenated form")
    assert set(g1) == set(ref) and set(g0) == set(ref), (sorted(g1), sorted(ref))
    w1 = "embedding_net.net.0.weight"
    for n in ref:
        assert_grad(g1[n], ref[n], "bias form: " + n)
        assert_grad(g0[n], ref[n], "concatenated form: " + n)
        assert_grad(g1[n], g0[n].cpu(), "bias form against the concatenated form: " + n)
    for got in (g1, g0):                                         # both column blocks of W1 at their own scale
        assert_grad(got[w1][:, :in_net], ref[w1][:, :in_net], "gW1[:, :in_net]")
        assert_grad(got[w1][:, in_net:], ref[w1][:, in_net:], "gW1[:, in_net:]")
    _, _, again = run_dag(cond, x, ctx, True, cot)               # the same call, the same bits
    for n in g1:
        assert torch.equal(g1[n], again[n]), n


# ------------------------------------------------------------------------------------------- 3. Coupling, Autoregressive
PLAIN_SHAPES = [(1, 2, 1), (6, 5, 2), (100, 9, 3)]


def _plain_case(kind, shape, hidden=(24, 24)):
    from models import AutoregressiveConditioner, CouplingConditioner
    B, d, c = shape
    torch.manual_seed(700 + B + d + c)
    T = CouplingConditioner if kind == "Coupling" else AutoregressiveConditioner
    cond = T(d, list(hidden), 3, cond_in=c)
    gen = torch.Generator().manual_seed(7000 + B * d + c)
    (x, ctx), _ = resample_off_ties(lambda: (torch.randn(B, d, generator=gen), torch.randn(B, c, generator=gen)),
                                    coupling_tied(cond) if kind == "Coupling" else made_tied(cond))
    return cond.to(DEV), x, ctx, torch.randn(B, d, 3, generator=gen)


@pytest.mark.parametrize("kind", ["Coupling", "Autoregressive"])
@pytest.mark.parametrize("shape", PLAIN_SHAPES, ids=sid)
def test_coupling_and_made_against_fp64(shape, kind):
    B, d, c = shape
    cond, x, ctx, cot = _plain_case(kind, shape)
    P = leaves64(cond)
    x64, c64 = x.double().requires_grad_(True), ctx.double().requires_grad_(True)
    h64 = (coupling64 if kind == "Coupling" else made64)(cond, P, x64, c64)
    (h64 * cot.double()).sum().backward()
    xd, cd = cu(x).requires_grad_(True), cu(ctx).requires_grad_(True)
    h = cond(xd, cd)
    assert tuple(h.shape) == (B, d, 3)
    (h * cu(cot)).sum().backward()
    assert_fwd(h.detach(), h64.detach(), what=kind)
    for n, p in cond.named_parameters():
        assert p.grad is not None and P[n].grad is not None, n
        assert_grad(p.grad, P[n].grad, n)
    assert_grad(cd.grad, c64.grad, "context")
    if kind == "Coupling":
        assert_grad(xd.grad, x64.grad, "x")
        assert bool((xd.grad[:, cond.indep_size:] == 0).all())
        assert bool((P["constants"].grad != 0).any())
    else:
        assert_grad(xd.grad, x64.grad, "x")


@pytest.mark.parametrize("hidden", [(), (24, 24)], ids=["direct", "24x24"])
@pytest.mark.parametrize("shape", PLAIN_SHAPES, ids=sid)
def test_made_sees_earlier_variables_and_the_context_only(shape, hidden):
    """hidden = (): the strict output rule lets EVERY output read the degree -1 context columns, the first variable's
    included.  With hidden layers the degrees are those of MADE(nin, ...), whose hidden units all have degree >= 0: the
    outputs of the degree-0 variable read no hidden unit (they are the output bias, as in the unconditional MADE) and
    cannot see the context; every other variable does (divergence table)."""
    B, d, c = shape
    cond, x, ctx, _ = _plain_case("Autoregressive", shape, hidden)
    net = cond.masked_autoregressive_net
    order = [int(v) for v in net.m[-1]]                          # order[i]: the position of variable i (natural: i)
    assert all(l.degree_spec() is not None for l in net.masked_layers())
    with torch.no_grad():
        xd, cd = cu(x), cu(ctx)
        h = cond(xd, cd)
        for j in range(d):
            xp = xd.clone()
            xp[:, j] += 1.5
            hp = cond(xp, cd)
            for i in range(d):
                if order[i] <= order[j]:
                    assert torch.equal(hp[:, i], h[:, i]), (i, j)
            later = [i for i in range(d) if order[i] > order[j]]
            if later:
                assert not torch.equal(hp[:, later], h[:, later]), j
        for k in range(c):
            cp = cd.clone()
            cp[:, k] += 1.5
            hp = cond(xd, cp)
            for i in range(d):                                   # direct: the first variable's outputs included
                if not hidden or order[i] > 0:
                    assert not torch.equal(hp[:, i], h[:, i]), (i, k)


# ------------------------------------------------------------------------------------------- 4. flows
def _flow(kind, normalizer, nb_steps):
    from models import (AffineNormalizer, AutoregressiveConditioner, CouplingConditioner, DAGConditioner, MonotonicNormalizer,
                        buildFCNormalizingFlow)
    d, c = 5, 2
    T = {"DAG": DAGConditioner, "Coupling": CouplingConditioner, "Autoregressive": AutoregressiveConditioner}[kind]
    out = 2 if normalizer == "affine" else 4
    cargs = {"in_size": d, "hidden": [16, 16], "out_size": out, "cond_in": c}
    if kind == "DAG":
        cargs["A_prior"] = torch.tril(torch.ones(d, d), -1)
    nargs = {} if normalizer == "affine" else {"integrand_net": [8, 8], "cond_size": out, "nb_steps": 20}
    torch.manual_seed(40 + nb_steps + len(kind))
    flow = buildFCNormalizingFlow(nb_steps, T, cargs, AffineNormalizer if normalizer == "affine" else MonotonicNormalizer,
                                  nargs)
    if kind == "DAG":                                            # every step its own A
        for cnd in flow.getConditioners():
            cnd.A = torch.nn.Parameter(cargs["A_prior"].clone())
    if normalizer == "monotonic":
        # A freshly initialised integrand is ~1 everywhere, so log|det J| is a sum of 5 * nb_steps logs of about +-.05 that
        # cancels to ~.02 while each term carries the rounding of its fp32 Jacobian entry (6e-8 absolute): below what
        # assert_fwd's 1e-6 max|b| + 1e-5 |b| can ask of ANY fp32 evaluation.  A last bias of +1 puts the integrand near 2 and
        # log|det J| at order 1 per variable, as in a trained flow, where the tolerance is the meaningful one.
        with torch.no_grad():
            for nrm in flow.getNormalizers():
                nrm.integrand_net.flat_params()[-1].add_(1.)
    flow = flow.to(DEV)
    if kind == "DAG":
        for cnd in flow.getConditioners():
            cnd.post_process()
            assert cnd.depth() == d - 1
    return flow, d, c


@pytest.mark.parametrize("nb_steps", [1, 2])
@pytest.mark.parametrize("normalizer", ["affine", "monotonic"])
@pytest.mark.parametrize("kind", ["DAG", "Coupling", "Autoregressive"])
def test_flows_against_fp64_and_round_trip(kind, normalizer, nb_steps):
    flow, d, c = _flow(kind, normalizer, nb_steps)
    B = 6
    gen = torch.Generator().manual_seed(90 + nb_steps)
    x, ctx, ctx2 = .7 * torch.randn(B, d, generator=gen), torch.randn(B, c, generator=gen), torch.randn(B, c, generator=gen)
    with torch.no_grad():
        z64, ld64, loss64 = flow64(flow, {n: d64(p) for n, p in flow.named_parameters()}, x.double(), ctx.double())
        z, ld = flow(cu(x), cu(ctx))
        loss = flow.loss(z, ld)
        assert_fwd(z, z64, what="z")
        assert_fwd(ld, ld64, what="logdet")
        assert_fwd(loss, loss64, what="loss")
        z2, _ = flow(cu(x), cu(ctx2))
        assert not torch.equal(z2, z)
        back = flow.invert(z, cu(ctx))
        zz, _ = flow(back, cu(ctx))
    # the tolerances of the round trips of tests/test_gpu_made_invert.py and tests/test_gpu_parity.py: 1e-4 for Affine; for
    # Monotonic every variable is a 20-step bisection (resolution 1.9e-5) amplified from level to level: 5e-3 on x, 2e-3 on z
    assert rel_err(back.cpu(), x) < (1e-4 if normalizer == "affine" else 5e-3)
    assert rel_err(zz.cpu(), z.cpu()) < (1e-4 if normalizer == "affine" else 2e-3)
    with pytest.raises(ValueError):
        flow(cu(x))
    with pytest.raises(ValueError):
        flow.invert(z, cu(ctx)[:, :1])


# ------------------------------------------------------------------------------------------- 5. dp
@pytest.mark.parametrize("kind", ["DAG", "DAG-bias", "Coupling", "Autoregressive"])
def test_dp_train_step_with_a_context(kind):
    from gnf_hip import dp
    from models import (AffineNormalizer, AutoregressiveConditioner, CouplingConditioner, DAGConditioner,
                        buildFCNormalizingFlow)
    T = {"DAG": DAGConditioner, "DAG-bias": DAGConditioner, "Coupling": CouplingConditioner,
         "Autoregressive": AutoregressiveConditioner}[kind]

    def build():                                                 # (a DAG conditioner's prev_trace buffer is no leaf: no deepcopy)
        torch.manual_seed(11)
        f = buildFCNormalizingFlow(2, T, {"in_size": 5, "hidden": [16, 16], "out_size": 2, "cond_in": 2}, AffineNormalizer,
                                   {}).to(DEV)
        dp.seed_gates(f, 0)
        if kind.startswith("DAG"):                               # both forms of the first layer through the flat gradient buffer
            for cnd in f.getConditioners():
                cnd.embedding_net.context_bias = kind == "DAG-bias"
        return f

    flow, twin = build(), build()
    twin.load_state_dict(flow.state_dict())
    s1, s2 = dp.FlatState(flow), dp.FlatState(twin)
    assert torch.equal(s1.flat, s2.flat)
    assert dp.steps_replayable(flow) is False
    gen = torch.Generator().manual_seed(12)
    for _ in range(2):
        x, ctx = cu(torch.randn(20, 5, generator=gen)), cu(torch.randn(20, 2, generator=gen))
        l1 = dp.train_step(flow, s1, x, context=ctx)
        l2 = dp.accumulate(twin, x, context=ctx)
        dp.apply_step(s2)
        assert torch.equal(l1.detach(), l2.detach())
        assert torch.equal(s1.flat, s2.flat) and torch.equal(s1.m, s2.m) and torch.equal(s1.v, s2.v)
        assert getattr(s1, "_graphed", None) is None
    assert s1.t == 2 and bool(s1.m.abs().sum() > 0)


# ------------------------------------------------------------------------------------------- 6. the driver
def _driver_args(tmp, conditioner, k, device_batches, epochs=2):
    import train_uci
    argv = ["-dataset", "power", "-data", "synthetic", "-folder", str(tmp), "-nb_epoch", str(epochs), "-b_size", "4000",
            "-conditioner", conditioner, "-emb_net", "16", "16", "2", "-l1", "0.", "-context_cols", str(k)]
    return train_uci.parse(argv + (["-device_batches"] if device_batches else []))


def _val_ll(model, val, k):
    import train_uci
    for cnd in model.getConditioners():                          # the same Philox stream for both models
        if hasattr(cnd, "_gate_calls"):
            cnd._gate_calls = 1000
    return train_uci.mean_ll(model, val, 4000, None, False, k)


@pytest.mark.parametrize("device_batches", [False, True], ids=["host-batches", "device-batches"])
@pytest.mark.parametrize("conditioner", ["DAG", "Coupling", "Autoregressive"])
def test_train_uci_with_context_cols(tmp_path, conditioner, device_batches):
    import train_uci
    from gnf_hip import dp
    args = _driver_args(tmp_path, conditioner, 2, device_batches)
    model = train_uci.train(args)
    first = {"DAG": "embedding_net", "Coupling": "embeding_net", "Autoregressive": "masked_autoregressive_net"}[conditioner]
    sd = torch.load(tmp_path / "model.pt", map_location="cpu")
    in0 = {"DAG": 8, "Coupling": 2, "Autoregressive": 4}[conditioner]          # 4 modelled columns (DAG: one-hot), 2 of context
    assert tuple(sd["steps.0.conditioner.%s.net.0.weight" % first].shape) == (16, in0 + 2)
    assert "epoch: 1 - Train loss" in open(tmp_path / "logs").read()           # it ran to the end
    fresh, _, _ = train_uci.build(args, 4)
    fresh.load_state_dict(sd)
    fresh.to(DEV)
    dp.seed_gates(fresh, 0)
    val = train_uci.load_split("synthetic", "power")[1].to(DEV)
    # the same parameters through the same kernels; 1e-6 relative leaves room for a kernel chosen by another address
    # alignment (the live parameters are views of the flat buffer), which may sum in another order (include/gnf_hip.h)
    live, again = _val_ll(model, val, 2), _val_ll(fresh, val, 2)
    assert live == live and abs(live - again) <= 1e-6 * max(1., abs(live)), (live, again)


def test_train_uci_without_context_cols_is_unchanged(tmp_path):
    import train_uci
    model = train_uci.train(_driver_args(tmp_path, "Coupling", 0, False, epochs=1))
    sd = torch.load(tmp_path / "model.pt", map_location="cpu")
    from models import AffineNormalizer, CouplingConditioner, buildFCNormalizingFlow
    plain = buildFCNormalizingFlow(1, CouplingConditioner, {"in_size": 6, "hidden": [16, 16], "out_size": 2}, AffineNormalizer,
                                   {}).state_dict()
    assert list(sd) == list(plain)
    assert all(sd[k].shape == plain[k].shape for k in sd)
    assert list(model.state_dict()) == list(plain)
