"""Time a conditional NormalizingFlowStep.invert(z, ctx) with each fast schedule on and off, in one process and one build:
`column_schedule = False` / `level_schedule = False` run the reference's depth() + 1 fixed-point passes
(NormalizingFlow.py:98-107), which is all a conditional flow had before the schedules took a context.
    made-power     Affine + MADE [60]^3,  d = 6,  c = 2,  B = 2500
    made-bsds      Affine + MADE [630],   d = 63, c = 8,  B = 2000
    made-784       Affine + MADE [1024]^3, d = 784, c = 10, B = 100
    mono-bsds      Monotonic [150]^3 + MADE [630] (30 outputs), d = 63, c = 8, B = 2000
    dag-power      Affine + post-processed DAG [60]^3 (one-hot), d = 6,  c = 2, B = 2500   (A strictly lower-triangular, density .5)
    dag-miniboone  Affine + post-processed DAG [430] (one-hot),  d = 43, c = 4, B = 1000
The passes stop as soon as one changes nothing (the reference's early exit), and a freshly initialised conditioner couples its
variables so weakly that they do after a few: every shape is therefore timed in two states, as initialised (--gains 1) and with
every conditioner weight matrix multiplied by 4 (the Affine normalizer clamps what comes out), where the dependence chains are
long as in a trained flow.  The number of passes a run actually took is on its line.
That state is also ill-conditioned (sigma is clamped at exp(-5): one column can amplify the error of the columns before it by
148), so the two fp32 arms differ visibly there.  --fp64 names the Affine + MADE shapes for which both arms are then measured
against an fp64 inversion on the CPU (B = 256, the same net and gains): one "fp64" line each.
No graph is captured for a pass with a context, so every run is launch by launch (replay-free).  The timing method is that of
tools/time_made_invert.py: warm-up, then the median of repeated runs, the two arms alternating; a host clock around work that
ends in a device synchronise.  Appends one line per shape to the file given with --out.

    python tools/bench_context_invert.py [--out profiles/context_invert_ab.txt] [--reps 5] [--shapes made-power,dag-power] [--fp64 made-power]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graphical-normalizing-flows_amd")]
from models import (AffineNormalizer, AutoregressiveConditioner, DAGConditioner, MonotonicNormalizer,  # noqa: E402
                    buildFCNormalizingFlow)

DEV = "cuda:0"
# name -> (kind, d, c, hidden, B)
SHAPES = {"made-power": ("made", 6, 2, [60, 60, 60], 2500),
          "made-bsds": ("made", 63, 8, [630], 2000),
          "made-784": ("made", 784, 10, [1024, 1024, 1024], 100),
          "mono-bsds": ("mono", 63, 8, [630], 2000),
          "dag-power": ("dag", 6, 2, [60, 60, 60], 2500),
          "dag-miniboone": ("dag", 43, 4, [430], 1000)}


def make(kind, d, c, hidden, gain=1.):
    torch.manual_seed(0)
    if kind == "made":
        flow = buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": d, "hidden": hidden, "out_size": 2, "cond_in": c},
                                      AffineNormalizer, {})
    elif kind == "mono":
        flow = buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": d, "hidden": hidden, "out_size": 30, "cond_in": c},
                                      MonotonicNormalizer, {"integrand_net": [150, 150, 150], "cond_size": 30, "nb_steps": 20,
                                                            "solver": "CC"})
    else:
        gen = torch.Generator().manual_seed(1)
        prior = torch.tril(torch.ones(d, d), -1) * (torch.rand(d, d, generator=gen) < .5).float()
        flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": hidden, "out_size": 2, "cond_in": c,
                                                          "hot_encoding": True, "A_prior": prior}, AffineNormalizer, {})
    if gain != 1.:
        with torch.no_grad():
            for n, p in flow.steps[0].conditioner.named_parameters():
                if n.endswith("weight"):
                    p.mul_(gain)
    flow = flow.to(DEV)
    if kind == "dag":
        flow.steps[0].conditioner.post_process()
    return flow.steps[0], ("level_schedule" if kind == "dag" else "column_schedule")


def fp64_line(name, gain, B=256):
    """both arms of an Affine + MADE shape against the reference's passes in double on the CPU, from the module's own
    parameters and mask buffers"""
    kind, d, c, hidden, _ = SHAPES[name]
    step, flag = make(kind, d, c, hidden, gain)
    gen = torch.Generator().manual_seed(1)
    z, ctx = .7 * torch.randn(B, d, generator=gen), torch.randn(B, c, generator=gen)
    layers = [(l.weight.detach().cpu().double() * l.mask.detach().cpu().double(), l.bias.detach().cpu().double())
              for l in step.conditioner.masked_autoregressive_net.masked_layers()]
    z64, c64 = z.double(), ctx.double()
    x64 = torch.zeros_like(z64)
    for _ in range(d):                                # d = depth() + 1 passes
        a = torch.cat((c64, x64), 1)
        for li, (W, b) in enumerate(layers):
            a = a @ W.t() + b
            if li < len(layers) - 1:
                a = torch.relu(a)
        h = a.view(B, -1, d).permute(0, 2, 1)
        x64 = (z64 - h[:, :, 0].clamp(-5., 5.)) / torch.exp(h[:, :, 1].clamp(-5., 2.))
    out = {}
    for on in (True, False):
        setattr(step, flag, on)
        out[on] = step.invert(z.to(DEV), ctx.to(DEV)).cpu().double()
    e_on, e_off = (out[True] - x64).abs().max().item(), (out[False] - x64).abs().max().item()
    return ("fp64 %s d=%d c=%d B=%d gain=%g: err_columns %.3e, err_passes %.3e (columns / passes = %.2f), "
            "max|x_columns - x_passes| %.3e, max|x| %.3e"
            % (name, d, c, B, gain, e_on, e_off, e_on / max(e_off, 1e-300), (out[True] - out[False]).abs().max().item(),
               x64.abs().max().item()))


def timed(step, flag, z, ctx, on):
    setattr(step, flag, on)
    torch.cuda.synchronize()
    t = time.perf_counter()
    x = step.invert(z, ctx)
    torch.cuda.synchronize()
    return time.perf_counter() - t, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--gains", default="1,4")
    ap.add_argument("--fp64", default="made-power,made-bsds")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    lines = []
    for name, gain in [(n, float(g)) for n in args.shapes.split(",") for g in args.gains.split(",")]:
        kind, d, c, hidden, B = SHAPES[name]
        step, flag = make(kind, d, c, hidden, gain)
        gen = torch.Generator().manual_seed(1)
        z, ctx = (.7 * torch.randn(B, d, generator=gen)).to(DEV), torch.randn(B, c, generator=gen).to(DEV)
        for on in (True, False):                      # warm-up of every kernel and shape both arms use
            timed(step, flag, z, ctx, on)
        t_on, t_off = [], []
        for _ in range(args.reps):
            a, x_on = timed(step, flag, z, ctx, True)
            b, x_off = timed(step, flag, z, ctx, False)
            t_on.append(a)
            t_off.append(b)
        diff = ((x_on - x_off).abs().max() / x_off.abs().max()).item()
        m_on, m_off = statistics.median(t_on), statistics.median(t_off)
        calls = []
        hook = step.conditioner.register_forward_hook(lambda *a: calls.append(1))
        timed(step, flag, z, ctx, False)              # (not timed: the hook) how many passes the early exit left
        hook.remove()
        passes = "%d of %d" % (len(calls), step.conditioner.depth() + 1)
        lines.append("%s d=%d c=%d B=%d gain=%g: %s %.3f ms (min %.3f, max %.3f), %s passes %.3f ms (min %.3f, max %.3f), "
                     "passes / schedule = %.2f, max|x_schedule - x_passes| / max|x| = %.2e, median of %d"
                     % (name, d, c, B, gain, flag.split("_")[0] + "s", 1e3 * m_on, 1e3 * min(t_on), 1e3 * max(t_on), passes,
                        1e3 * m_off, 1e3 * min(t_off), 1e3 * max(t_off), m_off / m_on, diff, args.reps))
        print(lines[-1], flush=True)
    for name, gain in [(n, float(g)) for n in args.fp64.split(",") if n for g in args.gains.split(",")]:
        lines.append(fp64_line(name, gain))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("conditional invert(z, ctx) wall time, schedule on / off in one process (tools/bench_context_invert.py)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
