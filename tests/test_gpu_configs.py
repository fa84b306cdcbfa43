"""BASELINE.json configurations as composites (-m gpu): cfg4 (MNIST d=784, Monotonic + DAG(MNISTCNN), the headline)
against the oracle chain at B=2 and through size-independent properties at B=100; cfg5 at its full B=50 000 with the
Monotonic normalizer; the fused Adam kernel against torch.optim.Adam on the device.  Mirrors the reference's
ImageExperiments.py:146-153,173,199-216.  Monotonic z / NLL: UMNN 1.0 parity unpinned (oracle restates the rule)."""
import os
import sys

import pytest
import torch

from conftest import ROOT, rel_err, assert_close, assert_fwd
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
GTOL = 1e-4


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _oracle_cfg4(sd, x, u1, u2, S):
    """dag_masked_inputs -> mnistcnn_forward -> monotonic_forward -> dag_loss -> flow_loss on the CPU oracle"""
    pre = "steps.0.conditioner."
    sd = {k: v.detach().cpu().clone() for k, v in sd.items()}
    cnn = {k[len(pre + "embedding_net."):]: v.requires_grad_(True) for k, v in sd.items() if "embedding_net." in k}
    A = sd[pre + "A"].requires_grad_(True)
    layers, k = [], 0
    ipre = "steps.0.normalizer.integrand_net.net."
    while ipre + "%d.weight" % k in sd:
        layers.append((sd[ipre + "%d.weight" % k].requires_grad_(True), sd[ipre + "%d.bias" % k].requires_grad_(True)))
        k += 2
    B, d = x.shape
    e = O.dag_masked_inputs(x, A, True, 0., True, False, 1., u1, u2, None, False)
    h = O.mnistcnn_forward(e, cnn).view(B, d, -1)
    z, jac = O.monotonic_forward(x, h, layers, S)
    closs = O.dag_loss(A, sd[pre + "alpha"], d % 50, sd[pre + "lambd"], sd[pre + "c"], sd[pre + "dag_const"],
                       sd[pre + "l1_weight"])
    ld = torch.log(jac).sum(1)
    loss = O.flow_loss(z, ld, closs)
    loss.backward()
    grads = {pre + "A": A.grad}
    for name, v in cnn.items():
        grads[pre + "embedding_net." + name] = v.grad
    for i, (W, b) in enumerate(layers):
        grads[ipre + "%d.weight" % (2 * i)] = W.grad
        grads[ipre + "%d.bias" % (2 * i)] = b.grad
    return z.detach(), ld.detach(), loss.detach(), grads


def test_cfg4_composite_vs_oracle():
    """bench.build_flow() -- buildMNISTNormalizingFlow([1], MonotonicNormalizer [50,50,50], prior kernel 2,
    hot_encoding=False), Gumbel gate with injected u1, u2 -- at B=2: z, log|det J|, loss, dA and every parameter
    gradient against the oracle chain."""
    bench = _bench()
    B, S = 2, 20
    flow = bench.build_flow()
    x = bench.pseudo_mnist(torch.Generator().manual_seed(77), B, 784)
    g = torch.Generator().manual_seed(78)
    u1, u2 = torch.rand(B, 784, 784, generator=g), torch.rand(B, 784, 784, generator=g)
    z0, ld0, loss0, grads0 = _oracle_cfg4(flow.state_dict(), x, u1, u2, S)

    flow = flow.to(DEV)
    for nrm in flow.getNormalizers():
        nrm.nb_steps = S
    cond = flow.steps[0].conditioner
    cond.gate_noise = (u1.to(DEV), u2.to(DEV))
    z, ld = flow(x.to(DEV))
    loss = flow.loss(z, ld)
    loss.backward()
    assert rel_err(z.cpu(), z0) < TOL and rel_err(ld.cpu(), ld0) < TOL and rel_err(loss.detach().cpu(), loss0) < TOL
    assert_fwd(z, z0, what='z')
    assert_fwd(ld, ld0, what='ld')
    assert_fwd(loss, loss0, what='loss')
    assert_close(z, z0, what="z")
    assert_close(ld, ld0, what="logdet")
    assert_close(loss, loss0, what="loss")
    nll0 = -(ld0 + O.normal_log_density(z0))
    nll = -(ld + flow.z_log_density(z))
    assert_close(nll, nll0, what="NLL")
    named = dict(flow.named_parameters())
    assert set(named) == set(grads0)
    for k, g0 in grads0.items():
        assert named[k].grad is not None, k
        assert rel_err(named[k].grad.cpu(), g0) < GTOL, (k, rel_err(named[k].grad.cpu(), g0))
        # element-wise (verdict r04 item 5): every entry of every parameter gradient of the headline model
        assert_close(named[k].grad, g0, rtol=1e-4, atol=1e-6 * g0.abs().max().item(), what="d " + k)
    # zero entries of the prior keep an exactly-zero gradient (grad ∝ A, DAG:118-119)
    assert int(((cond.A.grad != 0) & (cond.A.detach() == 0)).sum()) == 0


def test_cfg4_full_size_step_properties():
    """cfg4 at its per-GPU size (B=100, Philox gate): finite loss, a finite gradient for every parameter, the
    decomposition loss = constraints - mean(logdet + log N(z)), z(x) strictly monotone along each coordinate's own
    input (jac > 0.05), and a full dp.train_step that changes every parameter tensor."""
    from gnf_hip import dp
    bench = _bench()
    flow = bench.build_flow().to(DEV)
    x = bench.pseudo_mnist(torch.Generator().manual_seed(1234), 100, 784).to(DEV)
    for nrm in flow.getNormalizers():
        nrm.nb_steps = 20
    z, ld = flow(x)
    loss = flow.loss(z, ld)
    loss.backward()
    assert z.shape == (100, 784) and ld.shape == (100,)
    assert torch.isfinite(loss).item() and torch.isfinite(z).all() and torch.isfinite(ld).all()
    ref = flow.constraintsLoss() - (ld + O.normal_log_density(z.detach().cpu()).to(DEV)).mean()
    assert abs(ref.item() - loss.item()) <= 1e-5 * max(1., abs(loss.item()))
    for k, p in flow.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        assert p.grad.abs().max() > 0, k
        p.grad = None
    state = dp.FlatState(flow)
    before = state.flat.clone()
    l2 = dp.train_step(flow, state, x)
    assert torch.isfinite(l2).item() and state.t == 1
    moved = (state.flat != before)
    o = 0
    for p in state.params:
        assert moved[o:o + p.numel()].any(), "a parameter tensor did not move"
        o += (p.numel() + 3) // 4 * 4


def test_cfg4_strong_scaling_n1_point_B800():
    """The N = 1 point of north_star's strong-scaling curve: the global batch of 8 x 100 on ONE GPU (627 200 masked images;
    pooled features 5.8 GB, so every kernel on the path addresses past 2^32 bytes).  Rows 0..99 of z and log|det J| equal a
    B = 100 run with the same Philox key bit for bit (the noise counter is the row index), every gradient is finite and
    non-zero, dA keeps its exact zeros, and a full dp.train_step moves every parameter tensor.
    Reference: ImageExperiments.py:168,199-216 (the DataParallel batch of n_gpu x b_size rows)."""
    from gnf_hip import dp
    bench = _bench()
    torch.manual_seed(0)
    flow = bench.build_flow().to(DEV)
    for nrm in flow.getNormalizers():
        nrm.nb_steps = 20
    cond = flow.steps[0].conditioner
    x = bench.pseudo_mnist(torch.Generator().manual_seed(4321), 800, 784).to(DEV)
    with torch.no_grad():
        cond._gate_calls = 0
        z1, ld1 = flow(x[:100])
    cond._gate_calls = 0
    z, ld = flow(x)
    assert z.shape == (800, 784) and torch.equal(z[:100], z1) and torch.equal(ld[:100], ld1)
    assert torch.isfinite(z).all() and torch.isfinite(ld).all()
    loss = flow.loss(z, ld)
    loss.backward()
    assert torch.isfinite(loss).item()
    for k, p in flow.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k
    assert int(((cond.A.grad != 0) & (cond.A.detach() == 0)).sum()) == 0
    # the last rows are computed as the first ones are: the same samples placed at the end of another batch give the same bits
    # up to the gate noise (other row indices), so compare a deterministic-gate pass instead
    cond.stoch_gate = False
    with torch.no_grad():
        za, _ = flow(x)
        zb, _ = flow(torch.cat((x[700:], x[:100])))
    cond.stoch_gate = True
    assert torch.equal(za[700:], zb[:100])
    for p in flow.parameters():
        p.grad = None
    del z, ld, loss, za, zb
    state = dp.FlatState(flow)
    before = state.flat.clone()
    l2 = dp.train_step(flow, state, x)
    assert torch.isfinite(l2).item() and state.t == 1
    moved = (state.flat != before)
    o = 0
    for p in state.params:
        assert moved[o:o + p.numel()].any(), "a parameter tensor did not move"
        o += (p.numel() + 3) // 4 * 4


def test_cfg5_full_size_monotonic_step():
    """cfg5 as BASELINE.json states it: d=63, B=50 000 on one GPU, MADE [630]*3 -> 30, Monotonic [150,150,150],
    S=20.  Properties: finite loss and gradients, loss decomposition, jac > 0.05, z(0) = h0-free check by shifting x
    (strictly increasing in each coordinate given h), and agreement with the CPU oracle on a 64-row slice of the SAME
    batch (rows are independent: the slice of a full-size launch must equal the oracle's small run)."""
    from gnf_hip.configs import baseline_config
    flow, x = baseline_config("cfg5")
    assert x.shape == (50000, 63)
    for nrm in flow.getNormalizers():
        nrm.nb_steps = 20
    z, ld = flow(x)
    loss = flow.loss(z, ld)
    loss.backward()
    assert torch.isfinite(loss).item() and torch.isfinite(z).all() and torch.isfinite(ld).all()
    ref = -(ld + O.normal_log_density(z.detach().cpu()).to(DEV)).mean()
    assert abs(ref.item() - loss.item()) <= 1e-5 * max(1., abs(loss.item()))
    for k, p in flow.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    # oracle on rows 0..63 with the same parameters
    sd = {k: v.detach().cpu() for k, v in flow.state_dict().items()}
    pre = "steps.0.conditioner.masked_autoregressive_net."
    made, masks, k = [], [], 0
    while pre + "net.%d.weight" % k in sd:
        made.append((sd[pre + "net.%d.weight" % k], sd[pre + "net.%d.bias" % k]))
        masks.append(sd[pre + "net.%d.mask" % k])
        k += 2
    ipre = "steps.0.normalizer.integrand_net."
    layers, k = [], 0
    while ipre + "net.%d.weight" % k in sd:
        layers.append((sd[ipre + "net.%d.weight" % k], sd[ipre + "net.%d.bias" % k]))
        k += 2
    xs = x[:64].cpu()
    h0 = O.made_forward(xs, made, masks)                 # [64, 63, 30] view, component-major chunks
    z0, j0 = O.monotonic_forward(xs, h0, layers, 20)
    assert rel_err(z[:64].cpu(), z0) < TOL and rel_err(ld[:64].cpu(), torch.log(j0).sum(1)) < TOL
    assert_fwd(z[:64], z0, what='z[:64]')
    assert_fwd(ld[:64], torch.log(j0).sum(1), what='ld[:64]')
    assert_close(z[:64], z0, what="z")
    assert_close(ld[:64], torch.log(j0).sum(1), what="logdet")
    with torch.no_grad():
        h = flow.steps[0].conditioner(x)
        z1, j1 = flow.steps[0].normalizer(x, h)
        z2, _ = flow.steps[0].normalizer(x + .5, h)
        assert (j1 > .05).all() and (z2 > z1).all()
        assert torch.equal(z1, z.detach())


@pytest.mark.parametrize("n,wd", [(1000, 1e-5), (922797, 1e-5), (4099, 0.), (257, 1e-2)])
def test_hip_adam_vs_torch_adam_on_device(n, wd):
    """gnf_adam_step (the flat fused Adam of dp.train_step) against torch.optim.Adam(lr, weight_decay) on the same
    flat tensor for 5 steps on the device (ImageExperiments.py:173: Adam(lr, weight_decay), L2 form)."""
    from gnf_hip import ops
    torch.manual_seed(n)
    p0 = torch.randn(n, device=DEV)
    grads = [torch.randn(n, device=DEV) * (10. ** (i - 2)) for i in range(5)]
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=1e-3, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for t, g in enumerate(grads, 1):
        ref.grad = g.clone()
        opt.step()
        ops.adam_step(p, g, m, v, t, lr=1e-3, weight_decay=wd)
        assert_close(p, ref.data, rtol=1e-6, atol=1e-6, what="step %d" % t)
    st = opt.state[ref]
    # moments: torch forms exp_avg with lerp (m + (g - m) w), the kernel with fma(b1, m, w g): a few ulp of the largest
    # term apart; the gradients here span 1e-2 .. 1e2, so an ulp of the largest one is ~1e-5 absolute
    assert_close(m, st["exp_avg"], rtol=2e-6, atol=2e-5, what="exp_avg")
    assert_close(v, st["exp_avg_sq"], rtol=2e-6, atol=2e-5, what="exp_avg_sq")
    # the all-reduce scale (1/world) folded into the launch: grad_scale=1/4 on 4x the gradient is the same step
    p2, m2, v2 = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ops.adam_step(p2, grads[0] * 4, m2, v2, 1, lr=1e-3, weight_decay=wd, grad_scale=.25)
    ref2 = torch.nn.Parameter(p0.clone())
    opt2 = torch.optim.Adam([ref2], lr=1e-3, weight_decay=wd)
    ref2.grad = grads[0].clone()
    opt2.step()
    assert_close(p2, ref2.data, rtol=1e-6, atol=1e-6, what="grad_scale")


def test_graphed_step_vs_torch_adam_reference():
    """GraphedStep (hipGraph replay, device-side step counter) against an independent trajectory: autograd of the
    same flow + torch.optim.Adam -- not against the eager HIP step."""
    from gnf_hip import dp
    from models import buildFCNormalizingFlow, AutoregressiveConditioner, AffineNormalizer

    def make():
        torch.manual_seed(11)
        return buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": 12, "hidden": [64, 64], "out_size": 2},
                                      AffineNormalizer, {}).to(DEV)
    xs = [torch.randn(64, 12, generator=torch.Generator().manual_seed(200 + i)).to(DEV) for i in range(4)]
    fa = make()
    opt = torch.optim.Adam(fa.parameters(), lr=1e-2, weight_decay=1e-5)
    for x in [xs[0]] * 3 + xs:
        opt.zero_grad()
        z, ld = fa(x)
        la = fa.loss(z, ld)
        la.backward()
        opt.step()
    fb = make()
    sb = dp.FlatState(fb)
    gs = dp.GraphedStep(fb, sb, xs[0], lr=1e-2, weight_decay=1e-5, warmup=3)
    for x in xs:
        lb = gs(x)
    torch.cuda.synchronize()
    assert rel_err(lb.cpu(), la.detach().cpu()) < 1e-5
    for (k, pa), (_, pb) in zip(fa.named_parameters(), fb.named_parameters()):
        assert rel_err(pb.detach().cpu(), pa.detach().cpu()) < 1e-5, k


def test_graphed_frozen_gate_step_sees_a_rewritten_dual_buffer():
    """a captured step of a flow whose DAG gate is frozen bakes the constraint term in as a constant (DAGConditioner.loss
    evaluates it once per state); an in-place change of a dual buffer (what update_dual_param() does between epochs) must
    lead to a new capture, not to a replay with the stale constant.  Reference: the same trajectory stepped eagerly."""
    from gnf_hip import dp
    from models import buildFCNormalizingFlow, DAGConditioner, AffineNormalizer

    def make():
        torch.manual_seed(17)
        f = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": 10, "hidden": [32, 32], "out_size": 2, "l1": .3},
                                   AffineNormalizer, {}).to(DEV)
        with torch.no_grad():
            for c in f.getConditioners():
                c.A.mul_(.5)
                c.post_process(zero_threshold=.1)
                c.lambd.fill_(.25)
        return f
    xs = [torch.randn(40, 10, generator=torch.Generator().manual_seed(300 + i)).to(DEV) for i in range(6)]

    def run(graph):
        f = make()
        st = dp.FlatState(f)
        out = []
        for i, x in enumerate(xs):
            if i == 3:
                with torch.no_grad():
                    for c in f.getConditioners():
                        c.lambd.add_(2.)                 # in place: same buffer object, new version
            out.append(dp.train_step(f, st, x, lr=1e-2, graph="auto" if graph else False).detach().clone())
        torch.cuda.synchronize()
        return out, [p.detach().clone() for p in f.parameters()]
    lg, pg = run(True)
    le, pe = run(False)
    for a, b in zip(lg, le):
        assert rel_err(a.cpu(), b.cpu()) < 1e-5, (lg, le)
    assert abs(float(le[3] - le[2])) > 1e-3              # the change of lambd is visible in the loss at all
    for a, b in zip(pg, pe):
        assert rel_err(a.cpu(), b.cpu()) < 1e-5


def test_data_writes_to_a_frozen_gate_need_invalidate_caches():
    """A frozen A / a dual buffer rewritten through `.data` (reference DAGConditioner.py:89 writes A that way itself) moves
    neither a version counter nor an address -- the keys of the conditioner's value caches.  The contract:
    such a writer calls cond.invalidate_caches().  After it loss() is the oracle's dag_loss of the NEW values, eagerly and
    through a replayed GraphedStep (new capture, not the stale constant); every writer inside the package (post_process,
    constrainA, the dual update, load_state_dict, step()) invalidates by itself."""
    from gnf_hip import dp
    from models import buildFCNormalizingFlow, DAGConditioner, AffineNormalizer

    def oracle_loss(c):
        return O.dag_loss(c.A.detach().cpu(), c.alpha.cpu(), c.exponent, c.lambd.cpu(), c.c.cpu(), c.dag_const.cpu(),
                          c.l1_weight.cpu())

    torch.manual_seed(17)
    f = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": 10, "hidden": [32, 32], "out_size": 2, "l1": .3},
                               AffineNormalizer, {}).to(DEV)
    c = f.getConditioners()[0]
    with torch.no_grad():
        c.A.mul_(.5)
        c.post_process(zero_threshold=.1)
        c.lambd.fill_(.25)
    v0 = c.loss()
    assert rel_err(v0.cpu(), oracle_loss(c)) < TOL
    assert_fwd(v0, oracle_loss(c), what='v0')
    version, address = c.A._version, c.A.data_ptr()
    c.A.data.mul_(.5)
    assert (c.A._version, c.A.data_ptr()) == (version, address)      # invisible to the cache keys ...
    assert c.loss() is v0                                            # ... hence the documented stale value
    c.invalidate_caches()
    v1 = c.loss()
    assert rel_err(v1.cpu(), oracle_loss(c)) < TOL and abs(float(v1 - v0)) > 1e-4
    c.lambd.data.add_(1.)
    c.invalidate_caches()
    v2 = c.loss()
    assert rel_err(v2.cpu(), oracle_loss(c)) < TOL and abs(float(v2 - v1)) > 1e-4
    # the package's own writers invalidate by themselves
    sd = {k: v.clone() for k, v in f.state_dict().items()}
    sd["steps.0.conditioner.lambd"] = sd["steps.0.conditioner.lambd"] + 2.
    f.load_state_dict(sd)
    v3 = c.loss()
    assert rel_err(v3.cpu(), oracle_loss(c)) < TOL and abs(float(v3 - v2)) > 1e-4

    # through the captured step: the constant is baked into the graph; invalidate_caches() must force a new capture
    xs = [torch.randn(40, 10, generator=torch.Generator().manual_seed(300 + i)).to(DEV) for i in range(6)]

    def run(graph):
        torch.manual_seed(17)
        g = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": 10, "hidden": [32, 32], "out_size": 2, "l1": .3},
                                   AffineNormalizer, {}).to(DEV)
        with torch.no_grad():
            for cc in g.getConditioners():
                cc.A.mul_(.5)
                cc.post_process(zero_threshold=.1)
                cc.lambd.fill_(.25)
        st = dp.FlatState(g)
        out = []
        for i, x in enumerate(xs):
            if i == 3:
                for cc in g.getConditioners():
                    cc.A.data.mul_(.5)
                    cc.lambd.data.add_(2.)
                    cc.invalidate_caches()
            out.append(dp.train_step(g, st, x, lr=1e-2, graph="auto" if graph else False).detach().clone())
        torch.cuda.synchronize()
        return out
    lg, le = run(True), run(False)
    for a, b in zip(lg, le):
        assert rel_err(a.cpu(), b.cpu()) < 1e-5, (lg, le)
    assert abs(float(le[3] - le[2])) > 1e-3


def test_level_schedule_is_not_cached_for_a_trainable_gate():
    """with a trainable A under dp.FlatState the optimiser writes A through a raw pointer (no version bump, same
    address): invert() must recompute the level schedule every time.  Here A changes from one DAG to another between two
    inversions without any torch-visible write."""
    from models import buildFCNormalizingFlow, DAGConditioner, AffineNormalizer
    torch.manual_seed(3)
    d = 8
    f = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [16], "out_size": 2}, AffineNormalizer, {}).to(DEV)
    c = f.getConditioners()[0]
    c.stoch_gate = False
    lower = torch.tril(torch.ones(d, d), -1).to(DEV)
    with torch.no_grad():
        c.A.copy_(lower)
    assert c.A.requires_grad
    x = torch.randn(5, d, device=DEV)
    z, _ = f(x)
    assert rel_err(f.invert(z.detach()).cpu(), x.cpu()) < 1e-4
    c.A.data.copy_(lower.t())                        # the reverse ordering, written behind autograd's back
    z2, _ = f(x)
    assert rel_err(f.invert(z2.detach()).cpu(), x.cpu()) < 1e-4


def test_thresholded_importance_is_not_baked_into_a_sampling_graph():
    """a frozen A with s_thresh on hands the level pass a TEMPORARY importance matrix; a captured pass would
    replay reads of its freed address.  Such a gate must stay on the eager level pass (and still invert exactly)."""
    from models import buildFCNormalizingFlow, DAGConditioner, AffineNormalizer
    from models.NormalizingFlow import _INV_GRAPHS
    torch.manual_seed(4)
    d = 12
    f = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [16], "out_size": 2}, AffineNormalizer, {}).to(DEV)
    c, step = f.getConditioners()[0], f.steps[0]
    with torch.no_grad():
        c.A.copy_(torch.tril(torch.ones(d, d), -1).to(DEV) * 1.2)
    c.stoch_gate = False
    c.A.requires_grad = False
    assert c.s_thresh and c.deterministic_importance().data_ptr() != c.A.data_ptr()
    x = torch.randn(6, d, device=DEV)
    with torch.no_grad():
        z, _ = f(x)
        for _ in range(3):
            torch.empty(1 << 20, device=DEV).normal_()         # churn the allocator between the passes
            assert rel_err(f.invert(z).cpu(), x.cpu()) < 1e-4
    assert not any(isinstance(v, tuple) for v in _INV_GRAPHS.get(step, {}).values())


def test_graph_replay_after_eager_steps_keeps_the_adam_step_count():
    """train_step(graph='auto') interleaved with eager steps (graph=False): the eager ones advance state.t but not the
    device-side counter of the captured Adam launches; a later replay must see the right count (bias corrections).
    Reference trajectory: torch.optim.Adam on the same flow."""
    from gnf_hip import dp
    from models import buildFCNormalizingFlow, AutoregressiveConditioner, AffineNormalizer

    def make():
        torch.manual_seed(13)
        return buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": 10, "hidden": [48, 48], "out_size": 2},
                                      AffineNormalizer, {}).to(DEV)
    xs = [torch.randn(32, 10, generator=torch.Generator().manual_seed(300 + i)).to(DEV) for i in range(9)]
    modes = ["auto", "auto", False, False, False, "auto", False, "auto", "auto"]     # replays behind eager steps
    fa = make()
    opt = torch.optim.Adam(fa.parameters(), lr=1e-2, weight_decay=1e-5)
    for x in xs:
        opt.zero_grad()
        z, ld = fa(x)
        fa.loss(z, ld).backward()
        opt.step()
    fb = make()
    sb = dp.FlatState(fb)
    for x, mode in zip(xs, modes):
        dp.train_step(fb, sb, x, lr=1e-2, weight_decay=1e-5, graph=mode)
    torch.cuda.synchronize()
    assert sb.t == len(xs)
    assert int(sb._graphed.step_dev.item()) == sb.t
    for (k, pa), (_, pb) in zip(fa.named_parameters(), fb.named_parameters()):
        assert rel_err(pb.detach().cpu(), pa.detach().cpu()) < 1e-5, k


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_two_ranks_product_flow():
    """`python bench.py --gpus 2` as the driver invokes it: the launcher spawns two ranks of the PRODUCT flow (cfg4,
    B=100 each, different data and gate noise per rank); on a one-GPU box they share the device and the all-reduce
    travels over gloo (GNF_DIST_BACKEND).  n_gpus == 2, finite loss (bench exits non-zero otherwise), the replicas'
    parameter checksums are identical after the steps (ImageExperiments.py:168,205)."""
    import json
    import subprocess
    env = dict(os.environ, GNF_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--full", "--no-secondary", "--no-cpu-baseline"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 200 and out["config"]["parallelism"] == "dp2"
    assert out["replicas_identical"] is True and out["dist_backend"] == "gloo"
    assert out["value"] > 0 and out["steps"] == 3 and out["scaling"] == "weak"
    assert abs(out["value"] - 200 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]
    # communication time of the step's one collective and the per-rank step times travel in the line
    assert out["allreduce_ms_per_step"] is not None and out["allreduce_ms_per_step"] > 0
    assert len(out["ms_per_step_per_rank"]) == 2 and max(out["ms_per_step_per_rank"]) <= out["ms_per_step"] * 1.0001
    # the line says which device each rank sat on: on this one-GPU box the two (gloo) ranks share it, and it says so
    assert len(out["rank_devices"]) == 2 and out["rank_devices"][0] == out["rank_devices"][1] and out["rccl_world_size"] is None


@pytest.mark.parametrize("gpus", [1, 2])
def test_bench_strong_scaling_holds_the_global_batch(gpus):
    """`bench.py --global-batch G`: G is fixed and every rank takes G / N rows, "scaling": "strong" (north_star asks for
    strong scaling; the default line stays BASELINE's weak point of 100 rows per GPU).  N = 1 runs all 200 rows in one
    step, N = 2 (gloo transport on this one-GPU box) 100 per rank: same global batch, same accounting."""
    import json
    import subprocess
    env = dict(os.environ, GNF_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--global-batch", "200",
                        "--steps", "3", "--warmup", "1", "--no-secondary", "--no-cpu-baseline"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == gpus and out["scaling"] == "strong" and out["config"]["global_batch"] == 200
    assert "b_size=%d per GPU" % (200 // gpus) in out["config"]["workload"]
    assert abs(out["value"] - 200 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]
    assert out["replicas_identical"] is True
    # a global batch that does not divide over the ranks is refused before anything runs
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--global-batch", "201",
                        "--steps", "1", "--warmup", "0"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert (r.returncode != 0) == (gpus == 2)


def test_bench_line_carries_issue_figures():
    """the default N = 1 line: roofline.frac is a FRACTION (review of round 5, item 1) -- the flop the kernel executes in
    the algorithm it implements / time / peak: for the Winograd conv pair the MFMA instructions per image of the counter
    pass (profiles/r06_bench_inputs.json) x 2048, i.e. `mfma_issue_frac`; the direct-convolution rate of SURVEY.md 8(d)
    stays beside it as frac_direct_conv_equivalent.  The Monotonic kernels are priced at the algorithmic count (below what
    they issue).  Every hand-written kernel also carries its shared-ALU ceiling, the effective clock and the fraction of
    the peak at that clock."""
    import json
    import subprocess
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "GNF_DIST_BACKEND", "GNF_FORCE_DIST"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full",
                        "--no-secondary", "--no-cpu-baseline"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["scaling"] == "weak" and out["config"]["global_batch"] == 100
    assert out["mfma_operands"] in ("f32", "3xbf16 split (fc1, Monotonic main blocks), f32 elsewhere") and out["dtype"] == "f32"
    # one rank, one device, no collective: the device is named all the same
    assert len(out["rank_devices"]) == 1 and "name=" in out["rank_devices"][0] and out["rccl_world_size"] is None
    entries = [out["roofline"]] + out["roofline_other"]
    assert len(entries) == 4
    rf = out["roofline"]
    assert rf["bound"] == "mfma" and rf["peak"] == 157.3 and rf["unit"] == "TFLOP/s"
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3                   # frac = A / P on the line itself
    for e in entries:
        for f in ("frac", "frac_basis", "mfma_issue_frac", "issue_frac_ceiling_shared_alu", "valu_per_mfma",
                  "effective_clock_GHz", "frac_of_peak_at_clock"):
            assert f in e, (e["kernel"], f)
        assert 0. < e["frac"] <= 1., (e["kernel"], e["frac"])
        assert 0 < e["mfma_issue_frac"] < e["issue_frac_ceiling_shared_alu"] + .05
        if "frac_direct_conv_equivalent" in e:                # the conv pair: executed basis == the issued MFMAs
            assert e["frac_basis"].startswith("executed") and abs(e["frac"] - e["mfma_issue_frac"]) < 2e-3
            assert e["frac_direct_conv_equivalent"] > e["frac"] * 1.8           # Winograd issues ~2x fewer multiplies
        elif e.get("peak") == 2500.:                          # the split-bf16 Monotonic forward: executed bf16 flop against the bf16 peak
            assert e["frac_basis"].startswith("executed: bf16") and e["bound"].startswith("mfma (bf16")
            assert e["fp32_equivalent_TFLOPs_algorithmic"] > 100.     # ... and above what the fp32 kernel reached (96)
        else:                                                 # Monotonic: the algorithmic flop of SURVEY.md 8(d) (the backward issues
            assert e["frac_basis"].startswith("algorithmic")  # more -- recompute --, the forward runs part of it on the VALU)
        # the clock of the run (cycles of a launch from the counter pass / live launch time) sits within a few per cent of the
        # nominal 2.4 GHz on a warm GPU -- on either side of it (boost) -- and the two fractions differ by exactly that ratio
        assert 2.0 < e["effective_clock_GHz"] < 2.6 and 1.9 < e["effective_clock_GHz_in_pmc_pass"] < 2.6
        assert abs(e["frac_of_peak_at_clock"] * e["effective_clock_GHz"] / 2.4 / e["mfma_issue_frac"] - 1.) < 2e-3
        assert 0 < e["frac_of_peak_at_clock"] < 1.
    assert "frac_direct_conv_equivalent" in rf
    assert out["roofline"]["traffic"] and out["roofline"]["traffic_algorithmic"]
    # only the dominant kernel's entry point is timed (HIP events) inside the region, the others behind it
    src = out["ops_ms_source"]
    assert "timed steps" in src["gnf_mnistcnn_conv_bwd"] and "untimed" in src["others"]
    assert abs(src["gnf_mnistcnn_conv_bwd_in_the_untimed_pass"] / out["ops_ms"]["gnf_mnistcnn_conv_bwd"] - 1.) < .1
    assert all("untimed" in e["measured"] for e in out["roofline_other"])


def test_bench_rccl_branch_at_world_size_one():
    """The RCCL code path itself on the ONE GPU of this box (GNF_FORCE_DIST=1): init_process_group("nccl", device_id=...)
    with world size 1, the in-place device all-reduce of the flat gradient buffer inside every step, the device
    all-gather of the replica checksums and of the per-rank step times, dist.barrier() -- in a child process started
    before anything touches the GPU (the reference's nn.DataParallel call site is ImageExperiments.py:168)."""
    import json
    import subprocess
    env = dict(os.environ, GNF_FORCE_DIST="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "GNF_DIST_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full",
                        "--no-secondary", "--no-cpu-baseline"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["dist_backend"] == "nccl" and out["collective_forced_at_world_1"] is True
    assert out["replicas_identical"] is True
    assert out["allreduce_ms_per_step"] is not None and 0 < out["allreduce_ms_per_step"] < 50
    assert len(out["ms_per_step_per_rank"]) == 1
    assert out["rccl_world_size"] == 1 and len(out["rank_devices"]) == 1 and "name=" in out["rank_devices"][0]


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain `bench.py` run (no --full) prints the headline and none of the figures --full adds; `--dump-outputs DIR`
    writes what the last timed step computed: the loss, and per trainable parameter its value after the step and the
    step's gradient, float32, named after the flow's parameters, well under 64 MB."""
    import json
    import subprocess
    import numpy as np
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "GNF_DIST_BACKEND", "GNF_FORCE_DIST"):
        env.pop(k, None)
    dump = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--dump-outputs",
                        str(dump)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["unit"] == "samples/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and abs(out["value"] - 100 * 2 / (out["ms_per_step"] * 2e-3)) < 1e-6 * out["value"]
    for k in ("roofline", "roofline_other", "ops_ms", "secondary", "measured_peaks", "cpu_baseline"):
        assert k not in out, k
    flow = _bench().build_flow()                          # the seeded initial parameters
    params = [(n, p) for n, p in flow.named_parameters() if p.requires_grad]
    assert sorted(os.listdir(dump)) == sorted(["loss.npy"] + ["%s.%s.npy" % (kind, n) for n, _ in params
                                                              for kind in ("param", "grad")])
    loss = np.load(dump / "loss.npy")
    assert loss.dtype == np.float32 and loss.shape == (1,) and np.isfinite(loss).all()
    total, moved = loss.nbytes, 0
    for n, p in params:
        for kind in ("param", "grad"):
            a = np.load(dump / ("%s.%s.npy" % (kind, n)))
            assert a.dtype == np.float32 and a.shape == tuple(p.shape) and np.isfinite(a).all(), (kind, n)
            total += a.nbytes
        moved += not np.array_equal(np.load(dump / ("param.%s.npy" % n)), p.detach().numpy())
    assert total < 64 << 20
    assert moved == len(params), "%d of %d parameters unchanged by three Adam steps" % (len(params) - moved, len(params))


def test_train_uci_two_ranks_dual_updates_stay_in_lockstep(tmp_path):
    """train_uci.py under torch.distributed.run with two ranks (gloo transport on a one-GPU box): a DAG conditioner
    whose dual update fires every epoch (nb_steps_dual 1); the epoch loss is averaged over ranks before model.step(), so
    both replicas take the same branch; a ragged dataset size must not hang the epoch."""
    import subprocess
    import numpy as np
    g = np.random.default_rng(0)
    data = tmp_path / "toy.npz"
    np.savez(data, trn=g.standard_normal((1003, 6)).astype("float32"), val=g.standard_normal((200, 6)).astype("float32"),
             tst=g.standard_normal((200, 6)).astype("float32"))
    env = dict(os.environ, GNF_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "graphical-normalizing-flows_amd", "train_uci.py"), "-dataset", "power", "-data", str(data),
           "-folder", str(tmp_path / "run"), "-nb_epoch", "4", "-b_size", "250", "-conditioner", "DAG", "-emb_net", "16",
           "16", "4", "-normalizer", "affine", "-nb_steps_dual", "1", "-l1", "0.1"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in open(tmp_path / "run" / "logs") if l.startswith("epoch")]
    assert len(lines) == 4
    sd = torch.load(tmp_path / "run" / "model.pt", map_location="cpu")
    assert float(sd["steps.0.conditioner.lambd"]) > 0          # the dual update ran
    assert os.path.exists(tmp_path / "run" / "ADAM.pt")


def test_dag_clipped_normal_gate_golden():
    """`gumble = False` branch of the reference's stochastic gate (DAGConditioner.py:104-111) with the reference's
    own N(0,1) samples: h and every gradient against fixtures generated from the reference."""
    from conftest import load_golden
    from models import DAGConditioner
    g = load_golden("dag_clipped_normal")
    for tag in ("soft", "hard_hot"):
        h_thresh, hot = g[tag + ".cfg"].tolist()
        c = DAGConditioner(7, [12, 12], 3, hot_encoding=bool(hot))
        c.load_state_dict({k[len(tag) + 3:]: v for k, v in g.items() if k.startswith(tag + ".p.")})
        c = c.to(DEV)
        c.h_thresh, c.gumble = h_thresh, False
        c.gate_noise = (g[tag + ".n"].to(DEV),)
        x = g[tag + ".x"].to(DEV).requires_grad_(True)
        h = c(x)
        assert rel_err(h.cpu(), g[tag + ".h"]) < TOL
        assert_fwd(h, g[tag + ".h"], what='h')
        (h * g[tag + ".gh"].to(DEV)).sum().backward()
        assert rel_err(x.grad.cpu(), g[tag + ".gx"]) < GTOL and rel_err(c.A.grad.cpu(), g[tag + ".gA"]) < GTOL
        for k, p in c.named_parameters():
            if k != "A":
                assert rel_err(p.grad.cpu(), g[tag + ".g." + k]) < GTOL, (tag, k)


def test_custom_integrand_module_matches_fused_kernel():
    """MonotonicNormalizer(integrand_net=<nn.Module>) (reference MonotonicNormalizer.py:44-48): a user module is
    evaluated through PyTorch on the device.  Given a module with the arithmetic of the reference's IntegrandNet, the
    torch-op quadrature and the fused gfx950 kernel are two independent evaluations of the same rule: z, jac, every
    gradient and the bisection inverse agree."""
    from models import MonotonicNormalizer

    class Custom(torch.nn.Module):                     # same function as IntegrandNet, different module type
        def __init__(self, hidden, c):
            super().__init__()
            dims = [1 + c] + hidden + [1]
            self.lin = torch.nn.ModuleList(torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))

        def forward(self, x, h):                       # x [B', d], h [B', c*d] cond-major (reference :33-38)
            B, d = x.shape
            a = torch.cat((x.unsqueeze(2), h.view(B, -1, d).permute(0, 2, 1)), 2).reshape(B * d, -1)
            for k, lin in enumerate(self.lin):
                a = lin(a)
                if k < len(self.lin) - 1:
                    a = torch.relu(a)
            return (torch.nn.functional.elu(a) + 1.05).view(B, d)

    torch.manual_seed(8)
    B, d, c, S = 6, 5, 30, 20
    fused = MonotonicNormalizer([50, 50, 50], c, nb_steps=S).to(DEV)
    mod = Custom([50, 50, 50], c).to(DEV)
    with torch.no_grad():
        for lin, (W, b) in zip(mod.lin, zip(fused.integrand_net.flat_params()[0::2], fused.integrand_net.flat_params()[1::2])):
            lin.weight.copy_(W)
            lin.bias.copy_(b)
    custom = MonotonicNormalizer(mod, c, nb_steps=S)
    assert not custom._fused() and fused._fused()
    x0, h0 = torch.randn(B, d, device=DEV) * 1.5, torch.randn(B, d, c, device=DEV)
    gz, gj = torch.randn(B, d, device=DEV), torch.randn(B, d, device=DEV)
    res = []
    for norm in (fused, custom):
        x, h = x0.clone().requires_grad_(True), h0.clone().requires_grad_(True)
        z, jac = norm(x, h)
        ((z * gz).sum() + (torch.log(jac) * gj).sum()).backward()
        res.append((z.detach(), jac.detach(), x.grad, h.grad))
    for a, b, tol in zip(res[0], res[1], (TOL, TOL, GTOL, GTOL)):
        assert rel_err(a.cpu(), b.cpu()) < tol
    assert_close(res[0][0], res[1][0], what="z")
    for lin, (W, b) in zip(mod.lin, zip(fused.integrand_net.flat_params()[0::2], fused.integrand_net.flat_params()[1::2])):
        assert rel_err(lin.weight.grad.cpu(), W.grad.cpu()) < GTOL and rel_err(lin.bias.grad.cpu(), b.grad.cpu()) < GTOL
    xi_f = fused.inverse_transform(res[0][0], h0)
    xi_c = custom.inverse_transform(res[0][0], h0)
    assert (xi_f - xi_c).abs().max() <= 40. / 2 ** 20 + 1e-6 and (xi_c - x0).abs().max() < 1e-3


def test_train_step_auto_graph_follows_epoch_level_changes():
    """dp.train_step replays gate-free steps from a hipGraph by default.  Host-side state a captured step bakes in by
    value (Monotonic node count, batch shape, a DAG conditioner's exponent / gate flags / frozen A) is fingerprinted:
    changing it captures a new variant instead of replaying stale values.  Trajectory == launch-by-launch steps."""
    from gnf_hip import dp
    from models import buildFCNormalizingFlow, AutoregressiveConditioner, MonotonicNormalizer, DAGConditioner, AffineNormalizer

    def make():
        torch.manual_seed(21)
        return buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": 6, "hidden": [32, 32], "out_size": 8},
                                      MonotonicNormalizer, {"integrand_net": [16, 16], "cond_size": 8, "nb_steps": 20,
                                                            "solver": "CC"}).to(DEV)
    xs = [torch.randn(48 if i != 3 else 40, 6, generator=torch.Generator().manual_seed(300 + i)).to(DEV) for i in range(6)]
    nodes = [20, 20, 23, 23, 20, 27]
    fa, fb = make(), make()
    sa, sb = dp.FlatState(fa), dp.FlatState(fb)
    for x, S in zip(xs, nodes):
        for f in (fa, fb):
            f.getNormalizers()[0].nb_steps = S
        la = dp.train_step(fa, sa, x, lr=1e-2, graph=False)
        lb = dp.train_step(fb, sb, x, lr=1e-2)
        assert rel_err(lb.cpu(), la.detach().cpu()) < 1e-5, S
    gs = sb._graphed
    assert gs.captures == 4 and sb.t == sa.t == 6          # (48,S=20) (48,23) (40,23) (48,27); (48,20) replayed
    assert rel_err(sb.flat.cpu(), sa.flat.cpu()) < 1e-5

    # DAG flow with a deterministic gate: the dual update rewrites lambd / c IN PLACE (replay reads the new values) and
    # changes `exponent`, post_process() freezes A (one fewer live leaf): both must show in the replayed trajectory
    def make_dag():
        torch.manual_seed(22)
        f = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": 8, "hidden": [16], "out_size": 2, "l1": .1},
                                   AffineNormalizer, {}).to(DEV)
        f.getConditioners()[0].stoch_gate = False
        return f
    ga, gb = make_dag(), make_dag()
    ta, tb = dp.FlatState(ga), dp.FlatState(gb)
    x = torch.randn(64, 8, device=DEV)
    for phase in range(3):
        for _ in range(2):
            la = dp.train_step(ga, ta, x, lr=1e-2, graph=False)
            lb = dp.train_step(gb, tb, x, lr=1e-2)
            assert rel_err(lb.cpu(), la.detach().cpu()) < 1e-5, phase
        for f in (ga, gb):
            c = f.getConditioners()[0]
            if phase == 0:
                c.update_dual_param()                        # lambd += c h, maybe c *= eta; exponent may move
                c.exponent = 5
            elif phase == 1:
                with torch.no_grad():
                    c.post_process(.1)
    assert rel_err(tb.flat.cpu(), ta.flat.cpu()) < 1e-5
    assert tb._graphed.captures == 3


def test_gradients_are_written_into_the_flat_buffer():
    """ops.grad_out: the backward kernels of a MADE + Affine step write every parameter gradient into its slot of
    FlatState.grad (no concatenation launch); the parameters after two steps are bit-identical to the run that packs fresh
    gradient tensors.  A weight used twice in one graph, and a second micro-batch accumulating into .grad, get a fresh
    tensor for the second contribution -- the sums are those of plain autograd."""
    from gnf_hip import dp, ops
    from models import buildFCNormalizingFlow, AutoregressiveConditioner, AffineNormalizer
    def make():
        torch.manual_seed(5)
        return buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": 12, "hidden": [32, 32], "out_size": 2},
                                      AffineNormalizer, {}).to(DEV)
    x = torch.randn(10, 12, device=DEV)
    fa, fb = make(), make()
    sa, sb = dp.FlatState(fa), dp.FlatState(fb)
    for graph in (False, "auto", "auto"):
        dp.train_step(fa, sa, x, graph=graph)
        if graph is False:
            assert sa.pack_stats == {"in_place": len(sa.params), "copied": 0, "absent": 0}
    ops.unregister_grad_slots(sb)            # the second state without slots: its backward hands autograd fresh tensors
    for graph in (False, "auto", "auto"):
        dp.train_step(fb, sb, x, graph=graph)
        if graph is False:
            assert sb.pack_stats == {"in_place": 0, "copied": len(sb.params), "absent": 0}
    assert torch.equal(sa.flat, sb.flat) and torch.equal(sa.m, sb.m) and torch.equal(sa.v, sb.v)

    # a shared weight: y = L(relu(L(x))) with the same (W, b) twice
    torch.manual_seed(6)
    lin = torch.nn.Linear(16, 16).to(DEV)
    st = dp.FlatState(lin)
    xs = torch.randn(7, 16, device=DEV)
    h = ops.mlp(xs, [(lin.weight, lin.bias)])
    y = ops.mlp(torch.relu(h), [(lin.weight, lin.bias)])
    y.square().sum().backward()
    Wr, br = lin.weight.detach().cpu().requires_grad_(True), lin.bias.detach().cpu().requires_grad_(True)
    yr = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(xs.cpu(), Wr, br)), Wr, br)
    yr.square().sum().backward()
    st.pack_grads()
    assert_close(st.grad_views[0].view(16, 16), Wr.grad, rtol=1e-5, atol=1e-5, what="shared weight gradient")
    assert_close(st.grad_views[1], br.grad, rtol=1e-5, atol=1e-5, what="shared bias gradient")

    # two micro-batches into .grad, then one pack
    for k in range(2):
        ops.mlp(xs[3 * k:3 * k + 3], [(lin.weight, lin.bias)]).square().sum().backward()
    Wr.grad = br.grad = None
    for k in range(2):
        torch.nn.functional.linear(xs[3 * k:3 * k + 3].cpu(), Wr, br).square().sum().backward()
    st.pack_grads()
    assert_close(st.grad_views[0].view(16, 16), Wr.grad, rtol=1e-5, atol=1e-5, what="accumulated weight gradient")
    assert_close(st.grad_views[1], br.grad, rtol=1e-5, atol=1e-5, what="accumulated bias gradient")


def test_shared_gradient_slot_of_the_dag_matrix():
    """A receives two gradient contributions per backward (gate and acyclicity term): the first is written into the
    flat-buffer slot, the second added into it (ops.grad_out_shared) -- one step and two accumulated micro-batches give
    the parameters of the run that packs fresh tensors (gradient slots off)."""
    from gnf_hip import dp, ops
    from models import buildFCNormalizingFlow, DAGConditioner, AffineNormalizer
    def make():
        torch.manual_seed(11)
        f = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": 6, "hidden": [16, 16], "out_size": 2, "l1": .1},
                                   AffineNormalizer, {}).to(DEV)
        for c in f.getConditioners():
            c.stoch_gate = False
        return f
    x = torch.randn(12, 6, device=DEV)

    def run(flow, slots=True):
        st = dp.FlatState(flow)
        if not slots:
            ops.unregister_grad_slots(st)        # this state's backward hands autograd fresh gradient tensors
        dp.train_step(flow, st, x, graph=False)
        stats = dict(st.pack_stats)
        for i in range(2):
            dp.accumulate(flow, x[6 * i:6 * i + 6], .5)
        dp.apply_step(st)
        return st, stats
    sa, stats = run(make())
    assert stats == {"in_place": len(sa.params), "copied": 0, "absent": 0}
    sb, _ = run(make(), slots=False)
    assert_close(sa.flat, sb.flat, rtol=1e-6, atol=1e-7, what="parameters (slots on / off)")
    assert_close(sa.m, sb.m, rtol=1e-5, atol=1e-8, what="first moments")

    # a backward with NO gradient pack behind it (a user inspecting gradients, bench.py's fwd+bwd-only loop) leaves the
    # slots marked taken: the next backward must still hand A the sum of both contributions
    flow = make()
    st = dp.FlatState(flow)
    A = flow.getConditioners()[0].A
    grads = []
    for _ in range(3):
        for p in flow.parameters():
            p.grad = None
        z, ld = flow(x)
        flow.loss(z, ld).backward()
        assert A.grad is not None
        grads.append(A.grad.clone())
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[1], grads[2])
    dp.train_step(flow, st, x, graph=False)                    # ... and the step behind it sees every gradient
    assert st.pack_stats["absent"] == 0
