"""Time NormalizingFlowStep.intervene(z, P, v, ctx) on its fast arm (columns for a MADE, levels for a DAG) against its passes
arm (`column_schedule = False` / `level_schedule = False`: x <- where(pinned, v, normalizer^-1(z, conditioner(x))), up to
depth() + 1 times), and against invert(z, ctx) on the same step, in one process and one build:
    power        Affine + MADE [60]^3,                    d = 6,  c = 2, B = 2500
    bsds-affine  Affine + MADE [630],                     d = 63, c = 8, B = 2000
    bsds-spline  Spline (K = 8) + MADE [630],             d = 63, c = 8, B = 2000
    bsds-mono    Monotonic [150]^3 + MADE [630] (30 out), d = 63, c = 8, B = 2000
    dag          Affine + frozen DAG [430] (one-hot),     d = 43, c = 4, B = 1000   (A strictly lower-triangular, density .5)
with three pin sets -- none, every second degree (50 %), the last half of the degrees (50 %; for the DAG: of the variables,
whose index order is a topological one) -- and in two states of the conditioner, as initialised (--gains 1) and with every
weight matrix multiplied by 4, where the passes need most of their depth() + 1 rounds (tools/bench_context_invert.py says
why).  Method of that tool: warm-up, then the median of repeated runs, the arms alternating; a host clock around work that
ends in a device synchronise.  No graph is captured for an intervention, so every run is launch by launch.

--invert-ab OTHER_ROOT times invert(z, ctx) at the same shapes in child processes that import the package alternately from
this tree and from OTHER_ROOT (a checkout of the parent commit, built): the pin branch of the prefix kernel is compiled out
when no table is passed, and this is the measurement of that.

    python tools/bench_intervene.py [--out profiles/intervene_ab.txt] [--reps 7] [--shapes power,dag] [--invert-ab DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# name -> (kind, normalizer, d, c, hidden, B)
SHAPES = {"power": ("made", "affine", 6, 2, [60, 60, 60], 2500),
          "bsds-affine": ("made", "affine", 63, 8, [630], 2000),
          "bsds-spline": ("made", "spline", 63, 8, [630], 2000),
          "bsds-mono": ("made", "mono", 63, 8, [630], 2000),
          "dag": ("dag", "affine", 43, 4, [430], 1000)}
PINS = {"none": lambda d: [], "every-2nd": lambda d: list(range(0, d, 2)), "last-half": lambda d: list(range(d - d // 2, d))}


def make(root, kind, norm, d, c, hidden, gain=1.):
    import torch
    sys.path[:0] = [p for p in (root, os.path.join(root, "graphical-normalizing-flows_amd")) if p not in sys.path]
    import models
    N, nkw, out = {"affine": (models.AffineNormalizer, {}, 2),
                   "spline": (getattr(models, "SplineNormalizer", None), {"nb_bins": 8, "tail_bound": 3.}, 23),
                   "mono": (models.MonotonicNormalizer, {"integrand_net": [150, 150, 150], "cond_size": 30, "nb_steps": 20,
                                                         "solver": "CC"}, 30)}[norm]
    torch.manual_seed(0)
    if kind == "made":
        flow = models.buildFCNormalizingFlow(1, models.AutoregressiveConditioner,
                                             {"in_size": d, "hidden": hidden, "out_size": out, "cond_in": c}, N, nkw)
    else:
        gen = torch.Generator().manual_seed(1)
        prior = torch.tril(torch.ones(d, d), -1) * (torch.rand(d, d, generator=gen) < .5).float()
        flow = models.buildFCNormalizingFlow(1, models.DAGConditioner, {"in_size": d, "hidden": hidden, "out_size": out,
                                                                        "cond_in": c, "hot_encoding": True, "A_prior": prior},
                                             N, nkw)
    if gain != 1.:
        with torch.no_grad():
            for n, p in flow.steps[0].conditioner.named_parameters():
                if n.endswith("weight"):
                    p.mul_(gain)
    flow = flow.to(DEV)
    if kind == "dag":
        flow.steps[0].conditioner.post_process()
    return flow.steps[0], ("level_schedule" if kind == "dag" else "column_schedule")


def inputs(d, c, B):
    import torch
    gen = torch.Generator().manual_seed(1)
    return ((.7 * torch.randn(B, d, generator=gen)).to(DEV), torch.randn(B, c, generator=gen).to(DEV),
            torch.randn(B, d, generator=gen).to(DEV))


def clock(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def ms(ts):
    return "%.3f ms (min %.3f, max %.3f)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))


def arms(args):
    lines = []
    for name, gain in [(n, float(g)) for n in args.shapes.split(",") for g in args.gains.split(",")]:
        kind, norm, d, c, hidden, B = SHAPES[name]
        step, flag = make(ROOT, kind, norm, d, c, hidden, gain)
        z, ctx, v = inputs(d, c, B)
        order = list(range(d)) if kind == "dag" else step.conditioner.prefix_plan(with_context=True)["var_host"]
        for pins, pick in PINS.items():
            idx = [order[t] for t in pick(d)]

            def run(on):
                setattr(step, flag, on)
                return step.intervene(z, idx, v[:, idx], ctx)

            for on in (True, False, True, False):         # warm-up of every kernel and shape both arms use
                clock(lambda: run(on))
                clock(lambda: step.invert(z, ctx))
            setattr(step, flag, True)
            t_fast, t_pass, t_inv = [], [], []
            for _ in range(args.reps):
                a, x_fast = clock(lambda: run(True))
                arm = step._intervene_arm
                b, x_pass = clock(lambda: run(False))
                setattr(step, flag, True)
                e, _ = clock(lambda: step.invert(z, ctx))
                t_fast.append(a)
                t_pass.append(b)
                t_inv.append(e)
            calls = []
            hook = step.conditioner.register_forward_hook(lambda *a: calls.append(1))
            run(False)                                    # (not timed: the hook) how many passes the early exit left
            hook.remove()
            setattr(step, flag, True)
            diff = ((x_fast - x_pass).abs().max() / x_pass.abs().max()).item()
            lines.append("%s %s d=%d c=%d B=%d gain=%g pins=%s (%d of %d): %s %s, %d of %d passes %s, passes / %s = %.2f, "
                         "invert %s, %s / invert = %.2f, max|x_%s - x_passes| / max|x| = %.2e, median of %d"
                         % (name, norm, d, c, B, gain, pins, len(idx), d, arm, ms(t_fast), len(calls),
                            step.conditioner.depth() + 1, ms(t_pass), arm, statistics.median(t_pass) / statistics.median(t_fast),
                            ms(t_inv), arm, statistics.median(t_fast) / statistics.median(t_inv), arm, diff, args.reps))
            print(lines[-1], flush=True)
    return lines


def invert_child(args):
    """one child of --invert-ab: the medians of invert(z, ctx) at every shape, as JSON on the last line"""
    out = {}
    for name, gain in [(n, float(g)) for n in args.shapes.split(",") for g in args.gains.split(",")]:
        kind, norm, d, c, hidden, B = SHAPES[name]
        step, _ = make(args.child, kind, norm, d, c, hidden, gain)
        z, ctx, _ = inputs(d, c, B)
        for _ in range(3):
            clock(lambda: step.invert(z, ctx))
        out["%s gain=%g" % (name, gain)] = statistics.median(clock(lambda: step.invert(z, ctx))[0] for _ in range(args.reps))
    print(json.dumps(out))


def invert_ab(args):
    roots = {"this": ROOT, "parent": os.path.abspath(args.invert_ab)}
    runs = {k: [] for k in roots}
    for _ in range(args.rounds):
        for k, root in roots.items():                     # alternating: this, parent, this, parent, ...
            cmd = [sys.executable, os.path.abspath(__file__), "--child", root, "--shapes", args.shapes, "--gains", args.gains,
                   "--reps", str(args.reps)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout, check=True)
            runs[k].append(json.loads(res.stdout.strip().splitlines()[-1]))
    lines = []
    for case in runs["this"][0]:
        a, b = [r[case] for r in runs["this"]], [r[case] for r in runs["parent"]]
        lines.append("invert %s: this commit %s, parent %s, this / parent = %.3f, %d alternating processes each, median of %d "
                     "calls per process" % (case, ms(a), ms(b), statistics.median(a) / statistics.median(b), args.rounds,
                                            args.reps))
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--gains", default="1,4")
    ap.add_argument("--invert-ab", default=None, metavar="OTHER_ROOT")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=240.)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "timing needs the MI355X"
    if args.child:
        return invert_child(args)
    if args.invert_ab:
        head, lines = "invert(z, ctx) wall time, this commit against its parent (tools/bench_intervene.py --invert-ab)", invert_ab(args)
    else:
        head, lines = "intervene(z, P, v, ctx) wall time, fast arm / passes arm / invert in one process (tools/bench_intervene.py)", arms(args)
    if args.out:
        with open(args.out, "a") as f:
            f.write(head + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
