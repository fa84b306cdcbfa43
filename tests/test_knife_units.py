"""CPU tests of the knife-edge method itself (tests/knife_units.py): the matcher that judges the tied images / elements on the
GPU (tests/test_gpu_knife.py) is logic that can be wrong.  torch-CPU fp32 autograd stands in for the kernels: a correct
evaluation must be accepted, and defects CONFINED to tied cases must be rejected."""
import pytest
import torch
import torch.nn.functional as F

import knife_units as K
from conftest import conv_front_knife_images, integrand_knife_elements
from oracle import gnf_oracle as O

CONV_SHAPES = [(1, "dense"), (3, "sparse"), (700, "dense"), (1300, "sparse"), (2, "dense"), (257, "dense"), (512, "dense"),
               (515, "sparse")]                                                  # test_mnist_conv_front_vs_torch_cpu
MONO_SHAPES = [(1, 1, [50, 50, 50]), (3, 7, [50, 50, 50]), (5, 13, [100, 100, 100]), (2, 9, [150, 150]), (70, 3, [100, 100, 100]),
               (1373, 6, [100, 100, 100]), (1370, 6, [150, 150]), (300, 7, [50, 50, 50]), (131, 17, [40, 64, 24]),
               (2049, 1, [16, 16]), (300, 7, [200, 200]), (420, 5, [200, 200, 200])]   # test_monotonic_ragged_sizes
S = 20


# ------------------------------------------------------------------------------------------------ consistency
@pytest.mark.parametrize("n,kind", [(257, "dense"), (515, "sparse"), (3, "sparse")])
def test_conv_units_reduce_to_the_image_finder(n, kind):
    (e, *params), _ = K.draw_conv_front(n, kind)
    knife, n_relu, n_pool = conv_front_knife_images(e, *params)
    relu, pool = K.conv_front_tied_units(e, *params)
    assert torch.equal(K.conv_front_tied_images(e, *params), knife)
    assert torch.equal(relu.flatten(1).sum(1), n_relu)
    assert [len(p) for p in pool] == n_pool.tolist()
    for p in pool:
        for w, adm in p.items():
            assert len(adm) >= 2                                # the maximum and at least one entry near it
    if n > 3:
        assert int(knife.sum()) > 0


@pytest.mark.parametrize("B,d,hidden", [(131, 17, [40, 64, 24]), (2049, 1, [16, 16]), (300, 7, [200, 200])])
def test_integrand_units_reduce_to_the_element_finder(B, d, hidden):
    (norm, x, h), _ = K.draw_monotonic(B, d, hidden)
    layers = K.layers_cpu(norm)
    knife = integrand_knife_elements(x, h, layers, S)
    gates = K.integrand_tied_gates(x, h, layers, S)
    assert torch.equal(K.integrand_tied_elements(x, h, layers, S), knife) and int(knife.sum()) > 0
    for units in gates.values():
        for node, l, unit in units:
            assert 0 <= node <= S + 1 and 0 <= l < len(hidden) and 0 <= unit < hidden[l]


def test_forced_evaluations_restate_the_references():
    """without an override the forced fp64 evaluations ARE the references: torch's conv front, the oracle's UMNN gradients"""
    (e, *params), _ = K.draw_conv_front(3, "sparse")
    leaves = [t.double().requires_grad_(True) for t in (e, *params)]
    gp = torch.randn(3, 2304, dtype=torch.float64)
    pooled, _, _ = K.conv_front_forced(*leaves)
    g = torch.autograd.grad((pooled * gp).sum(), leaves)
    ref_leaves = [t.double().requires_grad_(True) for t in (e, *params)]
    ref = torch.flatten(F.max_pool2d(F.conv2d(torch.relu(F.conv2d(ref_leaves[0].view(-1, 1, 28, 28), ref_leaves[1], ref_leaves[2])),
                                              ref_leaves[3], ref_leaves[4]), 2), 1)
    assert torch.equal(pooled.detach(), ref.detach())
    for a, b in zip(g, torch.autograd.grad((ref * gp).sum(), ref_leaves)):
        assert float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())
    (norm, x, h), _ = K.draw_monotonic(3, 7, [50, 50, 50])
    layers = [(W.double().requires_grad_(True), b.double().requires_grad_(True)) for W, b in K.layers_cpu(norm)]
    x64, h64 = x.double().requires_grad_(True), h.double().requires_grad_(True)
    gz, gj = torch.randn(3, 7, dtype=torch.float64), torch.randn(3, 7, dtype=torch.float64)
    z0, j0 = O.monotonic_forward(x64, h64, layers, S)
    flat = [p for Wb in layers for p in Wb]
    ref = torch.autograd.grad((z0 * gz).sum() + (j0 * gj).sum(), [x64, h64] + flat)
    tot = [torch.zeros_like(p) for p in flat]
    for b in range(3):
        for i in range(7):
            xe, he = x[b, i].double().requires_grad_(True), h[b, i].double().requires_grad_(True)
            z, jac = K.monotonic_element_forced(xe, he, layers, S)
            assert abs(float(z - z0[b, i])) < 1e-12 * abs(float(z0[b, i])) and abs(float(jac - j0[b, i])) < 1e-12 * float(j0[b, i])
            g = torch.autograd.grad(z * gz[b, i] + jac * gj[b, i], [xe, he] + flat)
            assert abs(float(g[0] - ref[0][b, i])) <= 1e-12 * float(ref[0].abs().max())
            assert float((g[1] - ref[1][b, i]).abs().max()) <= 1e-12 * float(ref[1].abs().max())
            tot = [a + p for a, p in zip(tot, g[2:])]
    for a, r in zip(tot, ref[2:]):
        assert float((a - r).abs().max()) <= 1e-12 * float(r.abs().max())


# ------------------------------------------------------------------------------------------------ resampling
@pytest.mark.parametrize("n,kind", CONV_SHAPES)
def test_resampling_leaves_no_tied_image(n, kind):
    (e, *params), redraw = K.draw_conv_front(n, kind)
    (e2,), rounds = K.resample_off_ties(redraw, lambda e_: K.conv_front_tied_images(e_, *params), first=(e,))
    assert rounds <= 8 and int(conv_front_knife_images(e2, *params)[0].sum()) == 0
    first = conv_front_knife_images(e, *params)[0]
    assert torch.equal(e2[~first], e[~first])                    # only the tied images were replaced
    if kind == "sparse":
        assert float((e2 == 0).float().mean()) > .9              # redrawn as sparse
    print("conv front n=%d %s: %d tied at first draw, %d rounds" % (n, kind, int(first.sum()), rounds))


@pytest.mark.parametrize("B,d,hidden", MONO_SHAPES)
def test_resampling_leaves_no_tied_element(B, d, hidden):
    (norm, x, h), redraw = K.draw_monotonic(B, d, hidden)
    layers = K.layers_cpu(norm)
    (x2, h2), rounds = K.resample_off_ties(redraw, lambda x_, h_: K.integrand_tied_elements(x_, h_, layers, S), first=(x, h))
    assert rounds <= 8 and int(integrand_knife_elements(x2, h2, layers, S).sum()) == 0
    first = integrand_knife_elements(x, h, layers, S)
    assert torch.equal(x2[~first], x[~first]) and torch.equal(h2[~first], h[~first])
    print("Monotonic %s: %d of %d tied at first draw, %d rounds" % ((B, d, hidden), int(first.sum()), B * d, rounds))


def test_resampling_raises_when_ties_remain():
    with pytest.raises(RuntimeError):
        K.resample_off_ties(lambda: (torch.zeros(4),), lambda t: t == 0, max_rounds=3)


# ------------------------------------------------------------------------------------------------ the fp32 stand-ins
def conv_standin(n, kind):
    """the raw draw of the GPU test, cotangent on the live tied images only, torch-CPU fp32 autograd in the kernels' place"""
    (e, *params), _ = K.draw_conv_front(n, kind)
    tied, live = K.conv_front_live_images(*K.conv_front_tied_units(e, *params))
    gp = torch.randn(n, 2304) * live.float().unsqueeze(1)
    leaves = [t.clone().requires_grad_(True) for t in (e, *params)]
    c2 = F.conv2d(torch.relu(F.conv2d(leaves[0].view(-1, 1, 28, 28), leaves[1], leaves[2])), leaves[3], leaves[4])
    pooled, idx = F.max_pool2d(c2, 2, return_indices=True)
    g = torch.autograd.grad((torch.flatten(pooled, 1) * gp).sum(), leaves)
    return e, params, gp, g[0], list(g[1:]), K.pool_indices_to_entries(idx)


def mono_standin(B, d, hidden):
    (norm, x, h), _ = K.draw_monotonic(B, d, hidden)
    layers = K.layers_cpu(norm)
    tied, live = K.monotonic_live_elements(K.integrand_tied_gates(x, h, layers, S), x.shape)
    gz, gj = torch.randn(B, d) * live.float(), torch.randn(B, d) * live.float()
    lr = [(W.clone().requires_grad_(True), b.clone().requires_grad_(True)) for W, b in layers]
    xr, hr = x.clone().requires_grad_(True), h.clone().requires_grad_(True)
    z0, j0 = O.monotonic_forward(xr, hr, lr, S)
    g = torch.autograd.grad((z0 * gz).sum() + (j0 * gj).sum(), [xr, hr] + [p for Wb in lr for p in Wb])
    return x, h, layers, gz, gj, g[0], g[1], list(g[2:])


_CACHE = {}


def cached(fn, *key):
    k = (fn.__name__,) + tuple(str(v) for v in key)
    if k not in _CACHE:
        _CACHE[k] = fn(*key)
    return _CACHE[k]


@pytest.mark.parametrize("n,kind", [(700, "dense"), (515, "sparse"), (1300, "sparse"), (257, "dense")])
def test_conv_front_accepts_a_correct_evaluation(n, kind):
    e, params, gp, de, pgrads, arg = cached(conv_standin, n, kind)
    st = K.judge_conv_front(e, params, gp, de, pgrads, arg)
    print("conv front n=%d %s (fp32 stand-in): %s" % (n, kind, st))
    assert st["worst_best"] < 1e-5                   # fp32 against fp64: two orders under GTOL


MONO_KNIFE_SHAPES = [(300, 7, [50, 50, 50]), (1373, 6, [100, 100, 100]), (300, 7, [200, 200]), (420, 5, [200, 200, 200]),
                     (131, 17, [40, 64, 24])]                                    # those of tests/test_gpu_knife.py


@pytest.mark.parametrize("B,d,hidden", MONO_KNIFE_SHAPES)
def test_monotonic_accepts_a_correct_evaluation(B, d, hidden):
    x, h, layers, gz, gj, dx, dh, pgrads = cached(mono_standin, B, d, hidden)
    st = K.judge_monotonic(x, h, layers, S, gz, gj, dx, dh, pgrads)
    print("Monotonic %s (fp32 stand-in): %s" % ((B, d, hidden), st))
    assert st["worst_best"] < 1e-5


# ------------------------------------------------------------------------------------------------ defects confined to tied cases
def _most_distinct_conv_image(e, params, gp, de, arg):
    """(image, its Resolution) of the live tied image whose second-best combination is farthest from the chosen one"""
    relu, pool = K.conv_front_tied_units(e, *params)
    _, live = K.conv_front_live_images(relu, pool)
    best = None
    for i in live.nonzero().flatten().tolist():
        r = K.resolve_conv_image(e[i], params, gp[i], relu[i], pool[i], de[i], arg[i])
        if r.runner_up < float("inf") and (best is None or r.runner_up > best[1].runner_up):
            best = (i, r)
    return best


@pytest.mark.parametrize("n,kind", [(700, "dense"), (515, "sparse")])
def test_conv_front_rejects_defects_confined_to_a_tied_image(n, kind):
    e, params, gp, de, pgrads, arg = cached(conv_standin, n, kind)
    i, r = _most_distinct_conv_image(e, params, gp, de, arg)
    other = min((ce for ce in r.errs if ce[0] != r.combo), key=lambda ce: ce[1])[0]
    g_other, p_other = r.evaluate(other)
    # (a) the gradient routed to both entries of a tied window / half through a tied gate: the mean of two combinations
    bad = de.clone()
    bad[i] = ((r.grad[0] + g_other[0]) / 2).float()
    with pytest.raises(AssertionError, match="matches no admissible combination"):
        K.judge_conv_front(e, params, gp, bad, pgrads, arg)
    # (b) one tied image's gradient scaled by 1 + 1e-3
    bad = de.clone()
    bad[i] *= 1 + 1e-3
    with pytest.raises(AssertionError, match="matches no admissible combination"):
        K.judge_conv_front(e, params, gp, bad, pgrads, arg)
    # (c) the parameter gradients take another combination than de does
    badp = [(p.double() - a.view_as(p) + b.view_as(p)).float() for p, a, b in zip(pgrads, r.pgrads, p_other)]
    with pytest.raises(AssertionError, match=r"[Wb][12]"):
        K.judge_conv_front(e, params, gp, de, badp, arg)
    # a recorded argmax outside the admissible entries is refused too
    relu, pool = K.conv_front_tied_units(e, *params)
    for j in range(n):
        if pool[j]:
            w, adm = next(iter(pool[j].items()))
            if len(adm) < 4:
                bad_arg = arg.clone()
                bad_arg[j, w] = next(k for k in range(4) if k not in adm)
                with pytest.raises(AssertionError, match="not an admissible entry"):
                    K.judge_conv_front(e, params, gp, de, pgrads, bad_arg)
                break


@pytest.mark.parametrize("B,d,hidden", [(300, 7, [50, 50, 50]), (300, 7, [200, 200])])
def test_monotonic_rejects_defects_confined_to_a_tied_element(B, d, hidden):
    x, h, layers, gz, gj, dx, dh, pgrads = cached(mono_standin, B, d, hidden)
    gates = K.integrand_tied_gates(x, h, layers, S)
    _, live = K.monotonic_live_elements(gates, x.shape)
    x64, h64 = x.double().requires_grad_(True), h.double().requires_grad_(True)
    z0, j0 = O.monotonic_forward(x64, h64, [(W.double(), b.double()) for W, b in layers], S)
    ((z0 * gz.double()).sum() + (j0 * gj.double()).sum()).backward()
    scales = (float(x64.grad.abs().max()), float(h64.grad.abs().max()))
    best = None
    for b, i in live.nonzero().tolist():
        r = K.resolve_mono_element(x[b, i], h[b, i], layers, S, gz[b, i], gj[b, i], gates[(b, i)], (dx[b, i], dh[b, i]), scales)
        if best is None or r.runner_up > best[1].runner_up:
            best = ((b, i), r)
    (b, i), r = best
    assert r.runner_up > 2 * K.GTOL, "no tied element of this draw separates its combinations: %.2e" % r.runner_up
    other = min((ce for ce in r.errs if ce[0] != r.combo), key=lambda ce: ce[1])[0]
    g_other, p_other = r.evaluate(other)
    # (a) half through a tied gate
    bx, bh = dx.clone(), dh.clone()
    bx[b, i], bh[b, i] = ((r.grad[0] + g_other[0]) / 2).float(), ((r.grad[1] + g_other[1]) / 2).float()
    with pytest.raises(AssertionError, match="matches no admissible combination"):
        K.judge_monotonic(x, h, layers, S, gz, gj, bx, bh, pgrads)
    # (b) the element with the largest gradient, scaled by 1 + 1e-3 (the tolerance is relative to the tensor's maximum)
    k = int(dh.abs().amax(2).argmax())
    bh = dh.clone()
    bh[k // d, k % d] *= 1 + 1e-3
    with pytest.raises(AssertionError, match="matches no admissible combination"):
        K.judge_monotonic(x, h, layers, S, gz, gj, dx, bh, pgrads)
    # (c) the parameter gradients take another combination than (dx, dh) does
    badp = [(p.double() - a + o).float() for p, a, o in zip(pgrads, r.pgrads, p_other)]
    with pytest.raises(AssertionError, match=r"[Wb]\d"):
        K.judge_monotonic(x, h, layers, S, gz, gj, dx, dh, badp)
