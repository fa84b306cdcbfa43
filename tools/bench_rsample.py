"""Time the backward of NormalizingFlowStep.rsample(z, ctx) with the adjoint arm on and off, in one process and one build:
`adjoint_schedule = True` solves J^T lambda = g with the adjoint MADE column sweep (csrc/gnf_made_adjoint.hip, one launch,
its weight image packed inside the timed window), `adjoint_schedule = False` with at most depth() vjps of the existing
kernels (the passes arm, which is all a code base without the kernel could do, and stops as soon as an iteration changes
nothing).  Both then make the same vjp of the step for the parameter and context gradients.
    made-power     Affine + MADE [60]^3,   d = 6,   c = 2,  B = 2500
    made-bsds      Affine + MADE [630],    d = 63,  c = 8,  B = 2000
    made-784       Affine + MADE [1024]^3, d = 784, c = 10, B = 100
    mono-power     Monotonic [150]^3 + MADE [60]^3 (30 outputs), d = 6,  c = 2, B = 2500
    mono-bsds      Monotonic [150]^3 + MADE [630]  (30 outputs), d = 63, c = 8, B = 2000
(the shapes of tools/bench_context_invert.py; a Monotonic step at d = 784 is left out: its passes arm alone is 783 backward
passes of the integrand over 78 400 elements.)  Every shape as initialised (--gains 1) and with every conditioner weight
matrix multiplied by 4, where the dependence chains are long and the passes arm runs its full length; the number of vjps
it took is on the line.  The forward (the sample) is outside the timed window.  Warm-up, then the median of repeated runs,
the two arms alternating; a host clock around work that ends in a device synchronise.

    python tools/bench_rsample.py [--out profiles/rsample_ab.txt] [--reps 5] [--shapes made-power,mono-bsds] [--gains 1,4]"""
import argparse
import statistics
import time

import torch

from bench_context_invert import DEV, SHAPES as INVERT_SHAPES, make

SHAPES = {k: INVERT_SHAPES[k] for k in ("made-power", "made-bsds", "made-784")}
SHAPES["mono-power"] = ("mono", 6, 2, [60, 60, 60], 2500)
SHAPES["mono-bsds"] = INVERT_SHAPES["mono-bsds"]


def timed(step, z, ctx, g, params, on):
    step.adjoint_schedule = on
    x = step.rsample(z, ctx)
    torch.cuda.synchronize()
    t = time.perf_counter()
    grads = torch.autograd.grad(x, [z, ctx] + params, g)
    torch.cuda.synchronize()
    return time.perf_counter() - t, grads, step._rsample_arm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--gains", default="1,4")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    lines = []
    for name, gain in [(n, float(g)) for n in args.shapes.split(",") for g in args.gains.split(",")]:
        kind, d, c, hidden, B = SHAPES[name]
        step, _ = make(kind, d, c, hidden, gain)
        params = [p for p in step.parameters() if p.requires_grad]
        gen = torch.Generator().manual_seed(1)
        z = (.7 * torch.randn(B, d, generator=gen)).to(DEV).requires_grad_(True)
        ctx = torch.randn(B, c, generator=gen).to(DEV).requires_grad_(True)
        g = torch.randn(B, d, generator=gen).to(DEV)
        for on in (True, False):                      # warm-up of every kernel and shape both arms use
            timed(step, z, ctx, g, params, on)
        t_on, t_off = [], []
        for _ in range(args.reps):
            a, g_on, arm_on = timed(step, z, ctx, g, params, True)
            b, g_off, arm_off = timed(step, z, ctx, g, params, False)
            t_on.append(a)
            t_off.append(b)
        assert arm_on[0] == "adjoint" and arm_off[0] == "passes", (arm_on, arm_off)
        diff = ((g_on[0] - g_off[0]).abs().max() / g_off[0].abs().max()).item()
        m_on, m_off = statistics.median(t_on), statistics.median(t_off)
        lines.append("%s d=%d c=%d B=%d gain=%g: adjoint %.3f ms (min %.3f, max %.3f), passes (%d of %d vjps) %.3f ms "
                     "(min %.3f, max %.3f), passes / adjoint = %.2f, max|dz_adjoint - dz_passes| / max|dz| = %.2e, median of %d"
                     % (name, d, c, B, gain, 1e3 * m_on, 1e3 * min(t_on), 1e3 * max(t_on), arm_off[1], step.conditioner.depth(),
                        1e3 * m_off, 1e3 * min(t_off), 1e3 * max(t_off), m_off / m_on, diff, args.reps))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("rsample(z, ctx) backward wall time, adjoint arm / passes arm in one process (tools/bench_rsample.py)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
