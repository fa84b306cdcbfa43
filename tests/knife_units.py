"""Knife-edge decisions by UNIT, and the fp64 gradient of one admissible decision.

A ReLU gate / max-pool argmax decided on a quantity within fp32 roundoff of the tie may legitimately differ between two correct
fp32 evaluations.  tests/conftest.py finds the images / elements that hold such a decision (`conv_front_knife_images`,
`integrand_knife_elements`).  Until round 6 those cases got a zero cotangent; a backward defect confined to them passed.  This
module supports the two things that replace the exclusion:

* the main comparisons (`test_mnist_conv_front_vs_torch_cpu`, `test_monotonic_ragged_sizes`, `fuzz_mono.py`, `fuzz_linear.py`)
  REDRAW the tied cases from the same generator until none is left (`resample_off_ties`) -- images, Monotonic elements and MLP
  rows are independent of one another, so a redraw creates or removes ties in that case alone -- and then compare every case
  with a live cotangent;
* `tests/test_gpu_knife.py` keeps the raw draws, puts the cotangent on the tied cases ONLY and demands of each of them what
  can be demanded: its gradient equals the fp64 gradient under ONE admissible combination of its tied decisions
  (`resolve_branches`), and the parameter gradients equal the sum of the chosen combinations' parameter gradients -- the same
  decision for dx and for dW.

The finders use the criterion of tests/conftest.py (decision within `ulps` fp32 ulps of its terms' magnitude, exact ties are not
ties: the first-maximum rule holds on both sides) and return the units: which conv1 pre-activations, which pool windows with
which admissible entries, which (node, layer, unit) of the integrand net.  The forced evaluations restate the operations in
fp64 with the decisions as arguments: `a1 = pre1 * gate`, the pooled value gathered at a given index, a gate override for the
integrand net; the quadrature and the UMNN gradient conventions are those of oracle/gnf_oracle.py:132-195 (Leibniz rule
dz/dx = f(x; h); d/dh and d/dtheta as the quadrature of the integrand's derivatives at detached nodes).

Out of scope: the masked-copy tests of the sparse front (`_knife_edge_windows` in test_gpu_configs.py, fuzz_sparse_grad.py).
Their 784 copies per sample are functions of ONE x and cannot be redrawn independently; their arbitration stays as it is, and
so do `conv_front_knife_images` / `integrand_knife_elements` in tests/conftest.py, which they use."""
import itertools
import math

import torch
import torch.nn.functional as F

EPS32 = float(torch.finfo(torch.float32).eps)
MAX_COMBOS = 16


def _d(t):
    return t.detach().cpu().double()


# =================================================================================================== resampling
def resample_off_ties(draw, is_tied, max_rounds=8, first=None):
    """Replace the tied cases of a draw with fresh draws from the same generator until none is left.
    draw() -> tuple of tensors whose leading dimensions index the cases (a fresh full-size draw each call; only the tied
    cases' slices of it are used); is_tied(*tensors) -> bool tensor over the cases; first: the draw to start from (draw() if
    None).  -> (tensors, rounds used).  Raises if a tied case is left after `max_rounds` redraws."""
    cur = tuple(t.clone() for t in (draw() if first is None else first))
    for rnd in range(max_rounds + 1):
        tied = is_tied(*cur)
        left = int(tied.sum())
        if left == 0:
            return cur, rnd
        if rnd == max_rounds:
            break
        fresh = draw()
        for t, f in zip(cur, fresh):
            t[tied] = f[tied]
    raise RuntimeError("%d tied cases left after %d redraws" % (left, max_rounds))


# =================================================================================================== conv front
def _windows(t):
    """[n,16,24,24] -> [n,2304,4]: the 2x2 pool windows in pooled ([16,12,12]) order, entries in scan order"""
    n = t.shape[0]
    return t.reshape(n, 16, 12, 2, 12, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, 2304, 4)


def pool_indices_to_entries(idx):
    """max_pool2d(..., return_indices=True) indices (into the 24x24 plane) [n,16,12,12] -> [n,2304] entry 0..3 of the window"""
    return (((idx // 24) % 2) * 2 + (idx % 24) % 2).reshape(idx.shape[0], 2304)


def conv_front_tied_units(e, W1, b1, W2, b2, ulps=16.):
    """-> (relu [n,16,26,26] bool, pool): the tied conv1 pre-activations, and per image a dict {window 0..2303: tuple of the
    admissible entries 0..3} (the maximum and every entry within the bound of it) for the tied pool windows.  fp64, the
    criterion of conftest.conv_front_knife_images."""
    e, W1, b1, W2, b2 = [_d(t) for t in (e, W1, b1, W2, b2)]
    img = e.view(-1, 1, 28, 28)
    n = img.shape[0]
    pre1 = F.conv2d(img, W1.view(16, 1, 3, 3), b1)
    mag1 = F.conv2d(img.abs(), W1.view(16, 1, 3, 3).abs(), b1.abs())
    relu = (pre1.abs() < ulps * EPS32 * mag1) & (pre1 != 0)
    a1 = torch.relu(pre1)
    win = _windows(F.conv2d(a1, W2.view(16, 16, 3, 3), b2))
    wmag = _windows(F.conv2d(a1, W2.view(16, 16, 3, 3).abs(), b2.abs())).amax(2)
    gap = win.amax(2, keepdim=True) - win
    near = gap < ulps * EPS32 * wmag.unsqueeze(2)
    tied = (near & (gap != 0)).any(2)
    pool = [dict() for _ in range(n)]
    for i, w in tied.nonzero().tolist():
        pool[i][w] = tuple(near[i, w].nonzero().flatten().tolist())
    return relu, pool


def conv_front_tied_images(e, W1, b1, W2, b2, ulps=16.):
    """[n] bool: the unit finder reduced to images (== conftest.conv_front_knife_images(...)[0])"""
    relu, pool = conv_front_tied_units(e, W1, b1, W2, b2, ulps)
    return relu.flatten(1).any(1) | torch.tensor([len(p) > 0 for p in pool], dtype=torch.bool)


def conv_front_forced(e, W1, b1, W2, b2, gate=None, entry=None):
    """fp64 conv front with forced decisions: a1 = pre1 * gate (gate [m,16,26,26] 0/1, default pre1 > 0), the pooled value
    gathered at `entry` ([m,2304] in 0..3, default torch's first maximum).  -> (pooled [m,2304], gate, entry)"""
    img = e.view(-1, 1, 28, 28)
    pre1 = F.conv2d(img, W1.view(16, 1, 3, 3), b1)
    if gate is None:
        gate = (pre1.detach() > 0).to(pre1.dtype)
    c2 = F.conv2d(pre1 * gate, W2.view(16, 16, 3, 3), b2)
    if entry is None:
        entry = pool_indices_to_entries(F.max_pool2d(c2.detach(), 2, return_indices=True)[1])
    return _windows(c2).gather(2, entry.unsqueeze(2)).squeeze(2), gate, entry


class Resolution:
    """the outcome of resolve_branches for one case"""

    def __init__(self, combo, err, runner_up, grad, pgrads, n_combos, errs, evaluate, own):
        self.combo, self.err, self.runner_up, self.grad, self.pgrads, self.n_combos, self.errs, self.evaluate = \
            combo, err, runner_up, grad, pgrads, n_combos, errs, evaluate
        self.own = own          # {combo: error of the vector-valued gradients relative to THIS case's own maxima} (reported only)


def grad_err(got, ref, scales=None):
    """max over the tensors of max|got - ref| / scale; scale = max|ref| of that tensor unless given"""
    worst = 0.
    for k, (g, r) in enumerate(zip(got, ref)):
        s = float(r.abs().max()) if scales is None else scales[k]
        worst = max(worst, float((g.double() - r).abs().max()) / max(s, 1e-30))
    return worst


def resolve_branches(options, evaluate, got, scales=None, allowed=None, max_combos=MAX_COMBOS):
    """One tied case.  options: per tied decision the tuple of its admissible values; evaluate(combo) -> (grads, pgrads): the fp64
    gradient of this case alone w.r.t. its own inputs (tuple of tensors) and w.r.t. the parameters under that combination of
    decisions; got: the evaluation under test, same layout as grads.  The error of a combination is grad_err(got, grads, scales).
    allowed(combo) -> bool restricts the choice (a recorded pool argmax); the others still count for the runner-up.
    -> Resolution (chosen combination, its error, the best error of any OTHER combination, its gradients), or None when the
    case has more than `max_combos` combinations."""
    n_combos = math.prod(len(o) for o in options)
    if n_combos > max_combos:
        return None
    best, others, errs, own = None, [], [], {}
    for combo in itertools.product(*options):
        grads, pgrads = evaluate(combo)
        err = grad_err(got, grads, scales)
        errs.append((combo, err))
        vec = [k for k, g in enumerate(grads) if g.numel() > 1]
        own[combo] = grad_err([got[k] for k in vec], [grads[k] for k in vec])
        if (allowed is None or allowed(combo)) and (best is None or err < best[1]):
            if best is not None:
                others.append(best[1])
            best = (combo, err, grads, pgrads)
        else:
            others.append(err)
    assert best is not None, "no admissible combination"
    return Resolution(best[0], best[1], min(others) if others else float("inf"), best[2], best[3], n_combos, errs, evaluate, own)


def conv_front_image_options(relu_i, pool_i):
    """(units, options) of one image: units = [("relu", c, y, x) ...] + [("pool", window) ...]"""
    units = [("relu",) + tuple(u) for u in relu_i.nonzero().tolist()] + [("pool", w) for w in sorted(pool_i)]
    options = [(0., 1.)] * int(relu_i.sum()) + [pool_i[w] for w in sorted(pool_i)]
    return units, options


def resolve_conv_image(e_i, params, gp_i, relu_i, pool_i, de_i, arg_i=None, max_combos=MAX_COMBOS):
    """One tied image: e_i [784], params (W1, b1, W2, b2), its cotangent gp_i [2304], its tied units, the gradient under test de_i
    [784] and (optionally) the recorded pool argmax arg_i [2304].  With arg_i the pool decisions are TAKEN from it (each must be
    an admissible entry -- asserted) and only the ReLU gates are enumerated; the other pool entries are still evaluated for the
    runner-up while the whole image has at most `max_combos` combinations.  -> Resolution or None."""
    units, options = conv_front_image_options(relu_i, pool_i)
    allowed = None
    if arg_i is not None:
        rec = {w: int(arg_i[w]) for w in pool_i}
        for w, adm in pool_i.items():
            assert rec[w] in adm, "window %d: recorded argmax %d is not an admissible entry %s" % (w, rec[w], adm)
        if math.prod(len(o) for o in options) > max_combos:
            options = [o if u[0] == "relu" else (rec[u[1]],) for u, o in zip(units, options)]
        allowed = lambda combo: all(u[0] == "relu" or v == rec[u[1]] for u, v in zip(units, combo))    # noqa: E731
    e64, gp64 = _d(e_i).view(1, 784), _d(gp_i).view(1, 2304)
    p64 = [_d(p) for p in params]
    with torch.no_grad():
        _, gate0, entry0 = conv_front_forced(e64, *p64)

    def evaluate(combo):
        gate, entry = gate0.clone(), entry0.clone()
        for u, v in zip(units, combo):
            if u[0] == "relu":
                gate[0, u[1], u[2], u[3]] = v
            else:
                entry[0, u[1]] = v
        leaves = [t.clone().requires_grad_(True) for t in [e64] + p64]
        pooled, _, _ = conv_front_forced(*leaves, gate=gate, entry=entry)
        g = torch.autograd.grad((pooled * gp64).sum(), leaves)
        return (g[0].view(784),), g[1:]

    return resolve_branches(options, evaluate, (_d(de_i),), allowed=allowed, max_combos=max_combos)


# =================================================================================================== Monotonic normalizer
def _cc(nb_steps):
    from oracle import gnf_oracle as O
    w, t = O.cc_rule(nb_steps)
    return torch.tensor(w, dtype=torch.float64), torch.tensor(t, dtype=torch.float64)


def integrand_tied_gates(x, h, layers, nb_steps, ulps=16.):
    """-> {(b, i): [(node, layer, unit), ...]}: the hidden ReLU pre-activations of the integrand net within the bound of zero, at
    the quadrature nodes 0..nb_steps and at x itself (node nb_steps + 1, the Jacobian path).  fp64, the criterion of
    conftest.integrand_knife_elements."""
    _, t = _cc(nb_steps)
    x, h = _d(x), _d(h)
    layers = [(_d(W), _d(b)) for W, b in layers]
    B, d = x.shape
    out = {}
    nodes = [x * (float(tk) + 1.) / 2. for tk in t] + [x]
    for node, xk in enumerate(nodes):
        a = torch.cat((xk.reshape(B, d, 1), h), 2).reshape(B * d, -1)
        for l, (W, b) in enumerate(layers[:-1]):
            pre = a @ W.t() + b
            mag = a.abs() @ W.abs().t() + b.abs()
            for row, unit in ((pre.abs() < ulps * EPS32 * mag) & (pre != 0)).nonzero().tolist():
                out.setdefault((row // d, row % d), []).append((node, l, unit))
            a = torch.relu(pre)
    return out


def integrand_tied_elements(x, h, layers, nb_steps, ulps=16.):
    """[B, d] bool: the unit finder reduced to elements (== conftest.integrand_knife_elements)"""
    tied = torch.zeros(x.shape, dtype=torch.bool)
    for b, i in integrand_tied_gates(x, h, layers, nb_steps, ulps):
        tied[b, i] = True
    return tied


def monotonic_element_forced(x, h, layers, nb_steps, gates=None):
    """fp64 (z, jac) of ONE element of the Monotonic normalizer -- x: 0-d tensor, h: [c] -- with the gate override
    gates = {(node, layer, unit): 0. or 1.}.  Autograd of the result follows the UMNN conventions of the oracle: the quadrature
    nodes are detached (d/dh, d/dtheta = quadrature of the integrand's derivatives, weighted by (xT - x0)/2), and dz/dx = f(x; h)
    enters as a term of its own."""
    S = int(nb_steps)
    w, t = _cc(S)
    xT = S * (x / S)
    xs = torch.cat(((xT.detach() * (t + 1) / 2), x.reshape(1)))                 # nodes 0..S, then x itself (live)
    a = torch.cat((xs.unsqueeze(1), h.unsqueeze(0).expand(S + 2, -1)), 1)
    for l, (W, b) in enumerate(layers):
        pre = F.linear(a, W, b)
        if l == len(layers) - 1:
            break
        gate = (pre.detach() > 0).to(pre.dtype)
        for (node, gl, unit), v in (gates or {}).items():
            if gl == l:
                gate[node, unit] = v
        a = pre * gate
    f = (F.elu(pre) + 1.05).view(S + 2)
    z = (w * f[:S + 1]).sum() * (xT.detach() / 2) + f[S + 1].detach() * (x - x.detach()) + h[0]
    return z, f[S + 1]


def resolve_mono_element(x_bi, h_bi, layers, nb_steps, gz_bi, gj_bi, tied, got, scales, max_combos=MAX_COMBOS):
    """One tied element: its tied gates [(node, layer, unit)], the gradient under test got = (dx 0-d, dh [c]) for the loss
    z * gz + jac * gj of this element, scales = (max|dx|, max|dh|) of the whole reference tensors.  -> Resolution or None."""
    l64 = [(_d(W), _d(b)) for W, b in layers]

    def evaluate(combo):
        x = _d(x_bi).clone().requires_grad_(True)
        h = _d(h_bi).clone().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for Wb in l64 for p in Wb]
        z, jac = monotonic_element_forced(x, h, list(zip(ps[0::2], ps[1::2])), nb_steps, dict(zip(tied, combo)))
        g = torch.autograd.grad(z * float(gz_bi) + jac * float(gj_bi), [x, h] + ps)
        return (g[0], g[1]), g[2:]

    return resolve_branches([(0., 1.)] * len(tied), evaluate, tuple(_d(g) for g in got), scales=scales, max_combos=max_combos)


def settle_ambiguous(res, got_pgrads, tol):
    """Cases with more than one combination under `tol` in their own gradient: the combinations give the same parameter
    contribution only if the flipped unit's upstream gradient is zero.  Where they differ, the parameter-gradient residual
    breaks the tie (one greedy pass over the cases).  res: {case: Resolution}, updated in place.  -> (sum of the chosen
    combinations' parameter gradients, number of ambiguous cases, number whose choice the residual changed)."""
    total = None
    for r in res.values():
        total = [p.clone() for p in r.pgrads] if total is None else [a + p for a, p in zip(total, r.pgrads)]
    n_amb = n_switched = 0
    got = [_d(g) for g in got_pgrads]

    def resid(cand):
        return max(float((g - c).abs().max()) / max(float(c.abs().max()), 1e-30) for g, c in zip(got, cand))

    for r in res.values():
        under = [c for c, e in r.errs if e < tol]
        if len(under) < 2:
            continue
        n_amb += 1
        base = [a - p for a, p in zip(total, r.pgrads)]
        best = (resid(total), r.combo, r.pgrads, r.grad)
        for c in under:
            if c == r.combo:
                continue
            grads, pg = r.evaluate(c)
            rr = resid([a + p for a, p in zip(base, pg)])
            if rr < best[0]:
                best = (rr, c, pg, grads)
        if best[1] != r.combo:
            n_switched += 1
            r.combo, r.pgrads, r.grad = best[1], best[2], best[3]
            r.err = dict(r.errs)[r.combo]
            total = [a + p for a, p in zip(base, best[2])]
    return total, n_amb, n_switched


# =================================================================================================== the tests' draws
def draw_conv_front(n, kind):
    """the seeded draw of test_mnist_conv_front_vs_torch_cpu: (e, W1, b1, W2, b2) and redraw() -> (fresh e,) from the same
    generator ('sparse' images are redrawn as 'sparse')"""
    def images():
        e = torch.randn(n, 784)
        if kind == "sparse":
            e = e * (torch.rand(n, 784) < .03).float()
        return e
    torch.manual_seed(n)
    e = images()
    W1, b1 = torch.randn(16, 1, 3, 3) * .3, torch.randn(16) * .1
    W2, b2 = torch.randn(16, 16, 3, 3) * .1, torch.randn(16) * .1
    return (e, W1, b1, W2, b2), lambda: (images(),)


def draw_monotonic(B, d, hidden, c=30, S=20):
    """the seeded draw of test_monotonic_ragged_sizes: (norm, x, h) and redraw() -> fresh (x, h) from the same generator"""
    from models import MonotonicNormalizer
    torch.manual_seed(B * 100 + d)
    norm = MonotonicNormalizer(hidden, c, nb_steps=S)
    x, h = torch.randn(B, d), torch.randn(B, d, c)
    return (norm, x, h), lambda: (torch.randn(B, d), torch.randn(B, d, c))


def layers_cpu(norm):
    ps = [p.detach().cpu().clone() for p in norm.integrand_net.flat_params()]
    return [(ps[i], ps[i + 1]) for i in range(0, len(ps), 2)]


# =================================================================================================== the whole check
GTOL = 1e-4
MAX_LEFT_OUT = .05          # share of the tied cases that may have more than MAX_COMBOS combinations (zero cotangent)


def conv_front_live_images(relu, pool):
    """-> (tied [n] bool, live [n] bool): live = tied images that get a cotangent.  With the recorded argmax deciding the pool
    windows, an image has 2 ** (tied ReLU gates) combinations; those above MAX_COMBOS are left out."""
    n_relu = relu.flatten(1).sum(1)
    tied = (n_relu > 0) | torch.tensor([len(p) > 0 for p in pool], dtype=torch.bool)
    return tied, tied & (n_relu <= int(math.log2(MAX_COMBOS)))


def _check_cap(n_tied, n_live, what):
    assert n_live >= 1, "%s: no tied case resolved (%d tied)" % (what, n_tied)
    assert n_tied - n_live <= MAX_LEFT_OUT * n_tied, "%s: %d of %d tied cases left out (cap %d %%)" % (
        what, n_tied - n_live, n_tied, round(100 * MAX_LEFT_OUT))


def _check_params(got, ref, names, bound_last=None):
    from conftest import rel_err, assert_close
    for k, (g, r, name) in enumerate(zip(got, ref, names)):
        g = _d(g)
        if bound_last is not None and k == len(ref) - 1:
            # the output bias is ONE number, a sum of signed terms that can cancel: the fuzz walk's form (tests/fuzz_mono.py)
            err = min(rel_err(g, r), float((g - r).abs().max()) / max(bound_last, 1e-30) * 10.)
            assert err < GTOL, (name, err)
            continue
        assert rel_err(g, r) < GTOL, (name, rel_err(g, r))
        assert_close(g, r, rtol=1e-4, atol=2e-6 * r.abs().max().item(), what="d" + name)


def judge_conv_front(e, params, gp, de, pgrads, arg):
    """The decision-resolved check of the conv front.  gp: the cotangent, non-zero on the live tied images only; de [n,784],
    pgrads (dW1, db1, dW2, db2) and arg [n,2304] (recorded pool argmax): the evaluation under test.  Asserts: every live image
    matches an admissible combination at < GTOL (the per-image measure of test_mnist_conv_front_vs_torch_cpu), the parameter
    gradients equal the sum of the chosen combinations', the cap on the left-out images.  -> statistics"""
    relu, pool = conv_front_tied_units(e, *params)
    tied, live = conv_front_live_images(relu, pool)
    _check_cap(int(tied.sum()), int(live.sum()), "conv front")
    assert float(gp[~live].abs().max() if int((~live).sum()) else 0.) == 0. and bool((gp[live].abs().amax(1) > 0).all())
    total, worst, runner, worst_at = None, 0., float("inf"), None
    for i in live.nonzero().flatten().tolist():
        r = resolve_conv_image(e[i], params, gp[i], relu[i], pool[i], de[i], arg[i])
        assert r is not None
        if r.err > worst:
            worst, worst_at = r.err, (i, r.combo, conv_front_image_options(relu[i], pool[i])[0])
        runner = min(runner, r.runner_up)
        assert r.err < GTOL, "image %d matches no admissible combination: %s (units %s)" % (
            i, ["%s %.2e" % ce for ce in r.errs], conv_front_image_options(relu[i], pool[i])[0])
        total = list(r.pgrads) if total is None else [a + p for a, p in zip(total, r.pgrads)]
    dead = ~live
    assert float(_d(de)[dead].abs().max() if int(dead.sum()) else 0.) == 0., "gradient on an image without cotangent"
    _check_params(pgrads, [t.view_as(p) for t, p in zip(total, params)], ("W1", "b1", "W2", "b2"))
    return {"tied": int(tied.sum()), "resolved": int(live.sum()), "left_out": int((tied & ~live).sum()),
            "worst_best": worst, "min_runner_up": runner, "worst_at": worst_at}


def monotonic_live_elements(gates, shape):
    """-> (tied [B,d] bool, live [B,d] bool): an element with k tied gates has 2 ** k combinations"""
    tied, live = torch.zeros(shape, dtype=torch.bool), torch.zeros(shape, dtype=torch.bool)
    for (b, i), units in gates.items():
        tied[b, i] = True
        live[b, i] = 2 ** len(units) <= MAX_COMBOS
    return tied, live


def judge_monotonic(x, h, layers, nb_steps, gz, gj, dx, dh, pgrads):
    """The decision-resolved check of the Monotonic normalizer for the loss sum(z * gz + jac * gj), gz / gj non-zero on the live
    tied elements only.  dx [B,d], dh [B,d,c], pgrads (dW0, db0, ...): the evaluation under test.  An element's error is
    max(|dx - ref| / max|dx_ref|, max|dh - ref| / max|dh_ref|) with the maxima taken over the WHOLE reference tensors (the
    rel_err form of test_monotonic_ragged_sizes; the scales come from the fp64 oracle with its own gates, so they do not depend
    on the choice).  Elements with several combinations under GTOL are settled by the parameter-gradient residual.  -> statistics"""
    from conftest import rel_err
    from oracle import gnf_oracle as O
    gates = integrand_tied_gates(x, h, layers, nb_steps)
    tied, live = monotonic_live_elements(gates, x.shape)
    _check_cap(int(tied.sum()), int(live.sum()), "Monotonic")
    assert float((gz.abs() + gj.abs())[~live].max() if int((~live).sum()) else 0.) == 0. and bool((gz[live] != 0).all())
    x64, h64 = _d(x).requires_grad_(True), _d(h).requires_grad_(True)
    z0, j0 = O.monotonic_forward(x64, h64, [(_d(W), _d(b)) for W, b in layers], nb_steps)
    ((z0 * gz.double()).sum() + (j0 * gj.double()).sum()).backward()
    scales = (float(x64.grad.abs().max()), float(h64.grad.abs().max()))
    res = {}
    for b, i in live.nonzero().tolist():
        res[(b, i)] = resolve_mono_element(x[b, i], h[b, i], layers, nb_steps, gz[b, i], gj[b, i], gates[(b, i)],
                                           (dx[b, i], dh[b, i]), scales)
    for (b, i), r in res.items():
        assert r.err < GTOL, "element (%d, %d) matches no admissible combination: %s (gates %s)" % (
            b, i, ["%s %.2e" % ce for ce in r.errs], gates[(b, i)])
    total, n_amb, n_switched = settle_ambiguous(res, pgrads, GTOL)
    dx_ref, dh_ref = torch.zeros(x.shape, dtype=torch.float64), torch.zeros(h.shape, dtype=torch.float64)
    for (b, i), r in res.items():
        dx_ref[b, i], dh_ref[b, i] = r.grad[0], r.grad[1]
    assert rel_err(_d(dx), dx_ref) < GTOL and rel_err(_d(dh), dh_ref) < GTOL, (rel_err(_d(dx), dx_ref), rel_err(_d(dh), dh_ref))
    names = [s % k for k in range(len(layers)) for s in ("W%d", "b%d")]
    _check_params(pgrads, total, names, bound_last=float((gz.abs() * x.abs() + gj.abs()).sum()))
    single = [r for r in res.values() if len([1 for _, e_ in r.errs if e_ < GTOL]) < 2]
    return {"tied": int(tied.sum()), "resolved": int(live.sum()), "left_out": int((tied & ~live).sum()),
            "worst_best": max(r.err for r in res.values()), "min_runner_up": min(r.runner_up for r in res.values()),
            "min_runner_up_unambiguous": min([r.runner_up for r in single], default=float("inf")),
            "ambiguous": n_amb, "switched_by_param_residual": n_switched,
            # reported, not asserted: dh[b,i,:] against the element's OWN maximum -- the chosen combination and the best other one
            "worst_best_own_scale": max(r.own[r.combo] for r in res.values()),
            "min_runner_up_own_scale": min([e_ for r in res.values() for c_, e_ in r.own.items() if c_ != r.combo],
                                           default=float("inf"))}
