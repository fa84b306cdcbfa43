"""The Spline normalizer's kernels against their floors and against the same law composed of torch ops on the device; a
Spline + MADE step against the Monotonic + MADE step at BSDS300 width.  Appends to profiles/spline_ab.txt (or --out).

    python tools/bench_spline.py [--out FILE] [--quick]

Kernel rows: the C-ABI entry points on preallocated outputs (no autograd bookkeeping, no allocator), HIP events around 20
launches back to back, median of 9, arms alternating inside one process; the floor is gnf_probe_copy (a float4 STREAM copy)
over the bytes the kernel has to move, computed from the shapes here, and the share reported is floor time / kernel time.
The torch arm is tests/spline_ref.py -- the reference of the tests -- on device tensors (forward, autograd backward, inverse).
Step rows: NormalizingFlowStep forward + backward and invert, events around one call, median of 9."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graphical-normalizing-flows_amd"), os.path.join(ROOT, "tests")]
from gnf_hip import abi, ops  # noqa: E402
import spline_ref as S  # noqa: E402

DEV = "cuda:0"
P, st = abi.ptr, abi.stream


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


def kernels(B, d, K, T, layout, out, quick):
    C = 3 * K - 1
    g = torch.Generator(device="cpu").manual_seed(B + d)
    x = (2.2 * T / 3. * torch.randn(B, d, generator=g)).to(DEV)
    hc = torch.randn(B, d, C, generator=g).to(DEV)
    h = hc if layout == "contig" else hc.permute(0, 2, 1).contiguous().permute(0, 2, 1)       # MADE's view of [B, C, d]
    hs = (h.stride(0), h.stride(1), h.stride(2), C)
    z, jac, ld, ln = (torch.empty(B, d, device=DEV), torch.empty(B, d, device=DEV), torch.empty(B, device=DEV),
                      torch.empty(B, device=DEV))
    gz, gl = torch.randn(B, d, device=DEV), torch.randn(B, device=DEV)
    gx, gh, xi = torch.empty(B, d, device=DEV), torch.empty_like(h), torch.empty(B, d, device=DEV)
    n = B * d
    # bytes: fwd reads x, h, writes z (+ two rows sums); bwd reads x, h, gz (+ glogdet), writes gx, gh; inv reads z, h, writes x
    fb, bb, ib = 4. * n * (C + 2) + 8 * B, 4. * n * (2 * C + 3) + 4 * B, 4. * n * (C + 2)

    def fwd():
        abi.call("gnf_spline_fwd", P(x), P(h), *hs, K, T, P(z), None, P(ld), P(ln), B, d, st())

    def bwd():
        abi.call("gnf_spline_bwd", P(x), P(h), *hs, K, T, P(gz), None, P(gl), None, P(gx), P(gh), gh.stride(0), gh.stride(1),
                 gh.stride(2), B, d, st())

    def inv():
        abi.call("gnf_spline_inv", P(z), P(h), *hs, K, T, P(xi), None, 0, B, d, st())

    nmax = int(bb) // 8 // 4 * 4 + 4
    src, dst = torch.empty(nmax, device=DEV), torch.empty(nmax, device=DEV)
    lib = abi.load()

    def floor(nbytes):
        m = int(nbytes) // 8 // 4 * 4
        return lambda: lib.gnf_probe_copy(P(dst), P(src), m, st())

    xt, ht = x.clone().requires_grad_(True), h.detach().clone().requires_grad_(True)

    def t_fwd():
        with torch.no_grad():
            zz, jj = S.forward(x, h, K, T)
            return S.logdet_logn(zz, jj)

    def t_fwdbwd():
        zz, jj = S.forward(xt, ht, K, T)
        a, b = S.logdet_logn(zz, jj)
        torch.autograd.grad((zz * gz).sum() + (a * gl).sum(), (xt, ht))

    def t_inv():
        with torch.no_grad():
            return S.inverse(z, h, K, T)

    fwd()
    nt = 3 if quick else 10
    rows = [("fwd (z, logdet, logn)", fwd, floor(fb), fb, t_fwd), ("bwd (gz, glogdet -> gx, gh)", bwd, floor(bb), bb, None),
            ("inv", inv, floor(ib), ib, t_inv)]
    for name, fn, fl, nbytes, tfn in rows:
        t_k, t_f = timed(fn), timed(fl)
        t_k2, t_f2 = timed(fn), timed(fl)                        # arms alternate: the second pair shows the drift
        line = ("[%6d x %3d K=%d %-6s] %-28s kernel %8.2f / %8.2f us   copy floor %7.2f / %7.2f us   share %.2f   %.2f TB/s"
                % (B, d, K, layout, name, t_k, t_k2, t_f, t_f2, min(t_f, t_f2) / min(t_k, t_k2), nbytes / min(t_k, t_k2) / 1e6))
        if tfn is not None:
            t_t = timed(tfn, n=nt, reps=5)
            line += "   torch ops %9.1f us (x%.0f)" % (t_t, t_t / min(t_k, t_k2))
        print(line, flush=True)
        out.write(line + "\n")
    t_fb = timed(lambda: (fwd(), bwd()))
    t_t = timed(t_fwdbwd, n=nt, reps=5)
    line = ("[%6d x %3d K=%d %-6s] %-28s kernel %8.2f us   torch ops fwd + autograd %9.1f us (x%.0f)"
            % (B, d, K, layout, "fwd + bwd", t_fb, t_t, t_t / t_fb))
    print(line, flush=True)
    out.write(line + "\n")


def steps(out, quick):
    from models import (AutoregressiveConditioner, MonotonicNormalizer, SplineNormalizer, buildFCNormalizingFlow)
    d, hidden, B = 63, [630], 2000
    x = torch.randn(B, d, device=DEV)
    z = (.7 * torch.randn(B, d)).to(DEV)

    def build(kind):
        torch.manual_seed(0)
        if kind == "spline":
            return buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": d, "hidden": hidden, "out_size": 23},
                                          SplineNormalizer, {"nb_bins": 8}).to(DEV)
        return buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": d, "hidden": hidden, "out_size": 30},
                                      MonotonicNormalizer, {"integrand_net": [150, 150, 150], "cond_size": 30, "nb_steps": 20,
                                                            "solver": "CC"}).to(DEV)
    for kind in ("spline", "monotonic"):
        flow = build(kind)
        step = flow.steps[0]

        def fb():
            for p in flow.parameters():
                p.grad = None
            zz, ldet = flow(x)
            flow.loss(zz, ldet).backward()

        def inv():
            return step.invert(z)

        launches = []
        orig = abi.call

        def counting(name, *a, **k):
            launches.append(name)
            return orig(name, *a, **k)
        rows = [("forward + backward", fb, 5), ("invert (column schedule)", inv, 1 if kind == "monotonic" else 5)]
        for name, fn, n in rows:
            t = timed(fn, n=n, reps=3 if (quick or kind == "monotonic") else 9)
            line = "[step %-9s + MADE d=%d %s B=%d] %-26s %10.1f us" % (kind, d, hidden, B, name, t)
            print(line, flush=True)
            out.write(line + "\n")
        if kind == "spline":
            for sched in (True, False):
                step.column_schedule = sched
                del launches[:]
                abi.call = ops.call = counting
                try:
                    inv()
                finally:
                    abi.call = ops.call = orig
                t = timed(inv, n=2, reps=3)
                line = ("[step spline    + MADE] invert, column_schedule = %-5s  %3d entry-point calls  %10.1f us"
                        % (sched, len(launches), t))
                print(line, flush=True)
                out.write(line + "\n")
            step.column_schedule = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spline_ab.txt"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    abi.load()
    with open(args.out, "a") as out:
        out.write("\n== tools/bench_spline.py on %s ==\n" % torch.cuda.get_device_name(0))
        for B, d in [(50000, 63), (10000, 6), (100, 784)]:
            for layout in ("contig", "made"):
                kernels(B, d, 8, 3., layout, out, args.quick)
        steps(out, args.quick)


if __name__ == "__main__":
    main()
