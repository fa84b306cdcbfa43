"""Time NormalizingFlowStep.invert of the two MADE baseline configurations with the column schedule on and off, in one
process (`column_schedule = False` runs the reference's d fixed-point passes, NormalizingFlow.py:98-107):
    cfg3   Affine + MADE 1024^3, d = 784, B = 100
    cfg5   Monotonic [150]^3 + MADE 630^3, d = 63, at B = 2000 (the passes at B = 50000 run for tens of seconds)
Warm-up, then the median of repeated runs, the two schedules alternating; a host clock around work that ends in a device
synchronise.  Appends one line per shape to the file given with --out (default: standard output only).

    python tools/time_made_invert.py [--out profiles/made_column_invert.txt] [--reps 5]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graphical-normalizing-flows_amd")]
from gnf_hip.configs import baseline_config  # noqa: E402


def timed(step, z, on):
    step.column_schedule = on
    torch.cuda.synchronize()
    t = time.perf_counter()
    x = step.invert(z)
    torch.cuda.synchronize()
    return time.perf_counter() - t, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="cfg3:100,cfg5:2000")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    lines = []
    for spec in args.shapes.split(","):
        name, B = spec.split(":")
        flow, x = baseline_config(name)
        step = flow.steps[0]
        z = (.7 * torch.randn(int(B), x.shape[1], generator=torch.Generator().manual_seed(1))).to(x.device)
        for on in (True, False):                      # warm-up of every kernel and shape both schedules use
            timed(step, z, on)
        t_on, t_off = [], []
        for _ in range(args.reps):
            a, x_on = timed(step, z, True)
            b, x_off = timed(step, z, False)
            t_on.append(a)
            t_off.append(b)
        diff = ((x_on - x_off).abs().max() / x_off.abs().max()).item()
        m_on, m_off = statistics.median(t_on), statistics.median(t_off)
        lines.append("%s d=%d B=%s: columns %.3f ms (min %.3f, max %.3f), passes %.3f ms (min %.3f, max %.3f), "
                     "passes / columns = %.1f, max|x_columns - x_passes| / max|x| = %.2e, median of %d"
                     % (name, z.shape[1], B, 1e3 * m_on, 1e3 * min(t_on), 1e3 * max(t_on), 1e3 * m_off, 1e3 * min(t_off),
                        1e3 * max(t_off), m_off / m_on, diff, args.reps))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("invert() wall time, column schedule on / off in one process (tools/time_made_invert.py)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
