"""The masked reductions of the interventional likelihood (csrc/gnf_do_terms.hip) against the parent's unmasked kernels and
against the same law composed of torch ops.  Appends to profiles/do_likelihood_ab.txt (or --out).

    python tools/bench_do_likelihood.py [--out FILE] [--quick]

Protocol (tools/bench_spline.py): the C-ABI entry points on preallocated operands -- no autograd bookkeeping, no allocator --,
HIP events around 20 launches back to back, median of 9, the two arms of a row alternating (A B A B) inside one process; the
figure of an arm is the smaller of its two medians.  The yardsticks are the PARENT's kernels and the composed torch arm, never
the new code itself:
  (a) gnf_nll_do_fwd / _bwd        vs  gnf_nll_reduce_fwd / _bwd
  (b) gnf_affine_do_fwd / _bwd     vs  gnf_affine_fwd / _bwd with logdet + logn
  (c) the fused Affine pair        vs  the two-launch composition: gnf_affine_fwd with jac, then gnf_nll_do_fwd (and back)
  (d) all of the above             vs  what a user can write today: AffineFn with jac, then torch.where / log / sum, and
                                       autograd for the backward (events around 10 forward + backward calls, 3 with --quick,
                                       median of 5)
  (e) a full loss_do training step vs  the unmasked step, POWER Affine + DAG, B = 2500 (dp.train_step, graph=False both;
                                       with the per-step range check of the regime ids -- a host synchronisation -- and
                                       without it, check_regime=False).  That is like for like, but NOT the parent's default:
                                       at this size dp.train_step(graph="auto") replays the unmasked step from a hipGraph,
                                       which a step with regimes cannot do; the last row times that default too
Shapes [50 000, 63], [10 000, 6], [2500, 6], [100, 784]; tables R = 1 and R = 8 with a regime vector, half of the variables
pinned in every non-observational row."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graphical-normalizing-flows_amd")]
from gnf_hip import abi, dp, ops  # noqa: E402

DEV = "cuda:0"
P, RP, st = abi.ptr, abi.rawptr, abi.stream
LOG2PI = math.log(2. * math.pi)


def timed(fn, n=20, reps=9):
    """median microseconds per call of n back-to-back calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, c = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        c.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(c) / n * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def ab(new, old, n=20, reps=9):
    """(new, old) microseconds: each arm timed twice, alternating; the smaller median of each"""
    a1, b1 = timed(new, n, reps), timed(old, n, reps)
    a2, b2 = timed(new, n, reps), timed(old, n, reps)
    return min(a1, a2), min(b1, b2), (a1, a2, b1, b2)


def tables(B, d, R, gen):
    """(pin uint8 [R, d], regime int32 [B] or None, pinned bool [B, d]) on the device: half of the variables pinned in every
    non-observational row; R = 1: that one row for every sample; R = 8: row 0 observational, ids uniform"""
    half = lambda: (torch.randperm(d, generator=gen) < d // 2).to(torch.uint8)      # noqa: E731
    if R == 1:
        pin = half().view(1, d)
        return pin.to(DEV), None, pin.bool().expand(B, d).contiguous().to(DEV)
    pin = torch.stack([torch.zeros(d, dtype=torch.uint8)] + [half() for _ in range(R - 1)])
    regime = torch.randint(0, R, (B,), generator=gen)
    return pin.to(DEV), regime.to(torch.int32).to(DEV), pin[regime].bool().to(DEV)


def kernels(B, d, R, out, quick):
    g = torch.Generator().manual_seed(B + d + R)
    dev = lambda *s: torch.randn(*s, generator=g).to(DEV)                             # noqa: E731
    x, h, z = dev(B, d), dev(B, d, 2), dev(B, d)
    jac = (torch.rand(B, d, generator=g) * 3 + .05).to(DEV)
    gz, gl, gn = dev(B, d), dev(B), dev(B)
    pin, regime, pinned = tables(B, d, R, g)
    pr, rr = RP(pin), (None if regime is None else RP(regime))
    e = lambda *s: torch.empty(*s, device=DEV)                                        # noqa: E731
    zo, jo, ld, ln, gx, gh, gzo, gjo = e(B, d), e(B, d), e(B), e(B), e(B, d), e(B, d, 2), e(B, d), e(B, d)
    hs = (2 * d, 2, 1)
    tag = "[%6d x %3d R=%d]" % (B, d, R)

    def row(name, new, old, what_old):
        tn, to, raw = ab(new, old)
        line = ("%s %-30s new %8.2f us (%.2f / %.2f)   %s %8.2f us (%.2f / %.2f)   new / yardstick = %.2f"
                % (tag, name, tn, raw[0], raw[1], what_old, to, raw[2], raw[3], tn / to))
        print(line, flush=True)
        out.write(line + "\n")
        return tn, to

    # ---- (a)
    row("(a) nll_do_fwd", lambda: abi.call("gnf_nll_do_fwd", P(z), P(jac), pr, rr, R, P(ld), P(ln), B, d, st()),
        lambda: abi.call("gnf_nll_reduce_fwd", P(z), P(jac), P(ld), P(ln), B, d, st()), "nll_reduce_fwd")
    row("(a) nll_do_bwd",
        lambda: abi.call("gnf_nll_do_bwd", P(z), P(jac), pr, rr, R, P(gl), P(gn), None, P(gzo), P(gjo), B, d, st()),
        lambda: abi.call("gnf_nll_reduce_bwd", P(z), P(jac), P(gl), P(gn), None, P(gzo), P(gjo), B, d, st()), "nll_reduce_bwd")

    # ---- (b)
    def aff_do_fwd():
        abi.call("gnf_affine_do_fwd", P(x), P(h), *hs, pr, rr, R, P(zo), None, P(ld), P(ln), B, d, st())

    def aff_do_bwd():
        abi.call("gnf_affine_do_bwd", P(x), P(h), *hs, pr, rr, R, P(gz), None, P(gl), P(gn), P(gx), P(gh), *hs, B, d, st())
    row("(b) affine_do_fwd", aff_do_fwd,
        lambda: abi.call("gnf_affine_fwd", P(x), P(h), *hs, P(zo), None, P(ld), P(ln), 0, B, d, st()), "affine_fwd")
    row("(b) affine_do_bwd", aff_do_bwd,
        lambda: abi.call("gnf_affine_bwd", P(x), P(h), *hs, P(gz), None, P(gl), P(gn), P(gx), P(gh), *hs, B, d, st()),
        "affine_bwd")

    # ---- (c): AffineFn with jac, then NllDoFn -- two launches each way
    def comp_fwd():
        abi.call("gnf_affine_fwd", P(x), P(h), *hs, P(zo), P(jo), P(ld), None, 0, B, d, st())
        abi.call("gnf_nll_do_fwd", P(zo), P(jo), pr, rr, R, P(ld), P(ln), B, d, st())

    def comp_bwd():
        abi.call("gnf_nll_do_bwd", P(zo), P(jo), pr, rr, R, P(gl), P(gn), P(gz), P(gzo), P(gjo), B, d, st())
        abi.call("gnf_affine_bwd", P(x), P(h), *hs, P(gzo), P(gjo), None, None, P(gx), P(gh), *hs, B, d, st())
    comp_fwd()
    f_new, f_old = row("(c) fused fwd", aff_do_fwd, comp_fwd, "affine_fwd+jac, nll_do_fwd")
    b_new, b_old = row("(c) fused bwd", aff_do_bwd, comp_bwd, "nll_do_bwd, affine_bwd")

    # ---- (d): what a user can write today
    xt, ht = x.clone().requires_grad_(True), h.clone().requires_grad_(True)
    free = ~pinned
    zero, one = torch.zeros((), device=DEV), torch.ones((), device=DEV)

    def user():
        zz, jj, _, _ = ops.AffineFn.apply(xt, ht, False, True, False)
        a = torch.where(free, torch.log(torch.where(free, jj, one)), zero).sum(1)
        b = -.5 * torch.where(free, LOG2PI + torch.where(free, zz, zero) ** 2, zero).sum(1)
        torch.autograd.grad((zz * gz).sum() + (a * gl).sum() + (b * gn).sum(), (xt, ht))

    def mine():
        zz, _, a, b = ops.AffineDoFn.apply(xt, ht, pin, regime, False)
        torch.autograd.grad((zz * gz).sum() + (a * gl).sum() + (b * gn).sum(), (xt, ht))
    nt = 3 if quick else 10
    tn, to, raw = ab(mine, user, n=nt, reps=5)
    line = ("%s %-30s AffineDoFn fwd + bwd through autograd %8.1f us (%.1f / %.1f)   AffineFn + torch.where/log/sum + autograd "
            "%8.1f us (%.1f / %.1f)   ratio %.2f;   kernels alone: fused %.2f us, composition (c) %.2f us"
            % (tag, "(d) user-composed", tn, raw[0], raw[1], to, raw[2], raw[3], tn / to, f_new + b_new, f_old + b_old))
    print(line, flush=True)
    out.write(line + "\n")


def step(out, quick):
    """(e) POWER Affine + DAG, B = 2500: dp.train_step launch by launch, loss_do against the unmasked loss"""
    from models import AffineNormalizer, DAGConditioner, buildFCNormalizingFlow
    B, d, R = 2500, 6, 7
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, d, generator=g).to(DEV)
    targets = torch.cat((torch.zeros(1, d, dtype=torch.uint8), torch.eye(d, dtype=torch.uint8))).to(DEV)
    regime = (torch.arange(B) % R).to(torch.int32).to(DEV)

    def build():
        torch.manual_seed(0)
        flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [60, 60, 60], "out_size": 2, "l1": .2,
                                                          "gumble_T": .5, "nb_epoch_update": 30, "hot_encoding": True},
                                      AffineNormalizer, {}).to(DEV)
        return flow, dp.FlatState(flow)
    f_do, s_do = build()
    f_un, s_un = build()

    def do_step():
        dp.train_step(f_do, s_do, x, graph=False, targets=targets, regime=regime)

    f_nc, s_nc = build()

    def do_step_unchecked():                             # the regime ids validated once, as train_uci.py -regimes does
        dp.train_step(f_nc, s_nc, x, graph=False, targets=targets, regime=regime, check_regime=False)

    def plain_step():
        dp.train_step(f_un, s_un, x, graph=False)
    launches = {}
    orig = abi.call
    for name, fn in (("loss_do", do_step), ("unmasked", plain_step)):
        fn()
        seen = []

        def counting(nm, *a, **k):
            seen.append(nm)
            return orig(nm, *a, **k)
        abi.call = ops.call = counting
        try:
            fn()
        finally:
            abi.call = ops.call = orig
        launches[name] = len(seen)
    tn, to, raw = ab(do_step, plain_step, n=5 if quick else 20, reps=9)
    line = ("[step POWER Affine + DAG B=%d, launch by launch] loss_do step %8.1f us (%.1f / %.1f), %d entry-point calls   "
            "unmasked step %8.1f us (%.1f / %.1f), %d entry-point calls   ratio %.3f"
            % (B, tn, raw[0], raw[1], launches["loss_do"], to, raw[2], raw[3], launches["unmasked"], tn / to))
    print(line, flush=True)
    out.write(line + "\n")
    tn, to, raw = ab(do_step_unchecked, plain_step, n=5 if quick else 20, reps=9)
    line = ("[step POWER Affine + DAG B=%d, launch by launch] loss_do step, check_regime=False %8.1f us (%.1f / %.1f)   "
            "unmasked step %8.1f us (%.1f / %.1f)   ratio %.3f" % (B, tn, raw[0], raw[1], to, raw[2], raw[3], tn / to))
    print(line, flush=True)
    out.write(line + "\n")
    # what opting into regimes costs against the DEFAULT path of the unmasked step at this size: a GraphedStep replay
    f_gr, s_gr = build()

    def graphed_step():
        dp.train_step(f_gr, s_gr, x)
    for _ in range(3):
        graphed_step()
    replayed = getattr(s_gr, "_graphed", None) is not None
    tn, to, raw = ab(do_step_unchecked, graphed_step, n=5 if quick else 20, reps=9)
    line = ("[step POWER Affine + DAG B=%d] loss_do step, launch by launch, check_regime=False %8.1f us (%.1f / %.1f)   "
            "unmasked step on dp.train_step's default path (%s) %8.1f us (%.1f / %.1f)   ratio %.3f"
            % (B, tn, raw[0], raw[1], "hipGraph replay" if replayed else "NOT replayed: launch by launch", to, raw[2], raw[3],
               tn / to))
    print(line, flush=True)
    out.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "do_likelihood_ab.txt"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    abi.load()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_do_likelihood.py measures on the MI355X: no GPU here, nothing is measured")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        out.write("\n== python tools/bench_do_likelihood.py%s on %s ==\n"
                  % (" --quick" if args.quick else "", torch.cuda.get_device_name(0)))
        for B, d in [(50000, 63), (10000, 6), (2500, 6), (100, 784)]:
            for R in (1, 8):
                kernels(B, d, R, out, args.quick)
        step(out, args.quick)


if __name__ == "__main__":
    main()
