"""Time the StrADE conditioner against what it replaces, in one process and one build, the arms alternating back to back:

(a) conditioner forward + backward: StrADE vs a DAGConditioner after post_process() on the SAME graph and hidden widths (the DAG
    conditioner sends B d masked copies through its embedding net, StrADE B rows through masked GEMMs), and vs an
    AutoregressiveConditioner of the same widths (the price of streamed fp32 masks instead of the degree rule)
        power      d = 6,   [60]^3,   B = 2500      graph: strictly lower-triangular, density .5
        miniboone  d = 43,  [430],    B = 1000      likewise
        bsds       d = 63,  [630],    B = 2000      likewise
        mnist      d = 784, [1024]^3, B = 100       graph: the lower triangle of MNIST_A_prior(28, 2) (the prior itself is symmetric)
(b) invert of an Affine + StrADE step: the level kernel vs the fixed-point passes (`column_schedule` on / off), with the weights
    as initialised and multiplied by 4 (tools/bench_context_invert.py says why); for the FULL triangular graph also vs the
    MADE column sweep of an AutoregressiveConditioner of the same widths -- one variable per level is the level kernel's worst
    case, and this line says what it loses there.
(c) --made-dag: invert of the existing MADE and DAG steps alone, one "parent-ab" line per shape; run it from two checkouts in
    alternating processes (--pkg names the package directory to import) to compare a commit with its parent.
(d) the rsample backward of a StrADE step (NormalizingFlowStep._rsample_backward at a sample: conditioner and normalizer
    forward, the solve of J^T lambda = g, one vjp for the parameters): the adjoint level kernel (`adjoint_levels` on) vs at
    most depth() vjps (off), for Affine, Spline (8 bins) and Monotonic ([50, 50, 50], 20 steps, 4 outputs) normalizers
    (--norms), gains 1 and 4, on the tool's graph and on the FULL triangular graph -- one variable per level, the kernel's worst
    case -- there also vs the adjoint column sweep of an AutoregressiveConditioner of the same widths.
(e) parent-ab lines for the two files the adjoint level kernel shares code with: invert of an Affine + StrADE step on the
    level kernel, and the rsample backward of an Affine + MADE step on its adjoint kernel.  As (c): two checkouts, alternating
    processes, --pkg.

The timing method is that of tools/bench_context_invert.py: warm-up, then the median of repeated runs, a host clock around
work that ends in a device synchronise.  Appends its lines to the file given with --out.

    python tools/bench_strade.py [--out profiles/strade_ab.txt] [--reps 7] [--parts a,b] [--shapes power,bsds]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# name -> (d, hidden, B)
SHAPES = {"power": (6, [60, 60, 60], 2500), "miniboone": (43, [430], 1000), "bsds": (63, [630], 2000),
          "mnist": (784, [1024, 1024, 1024], 100)}


def graph(name, d, full=False):
    if full:
        return np.tril(np.ones((d, d), dtype=np.uint8), -1)
    if name == "mnist":
        from models.NormalizingFlowFactories import MNIST_A_prior
        return np.tril(MNIST_A_prior(28, 2).numpy(), -1).astype(np.uint8)
    gen = torch.Generator().manual_seed(1)
    return (torch.tril(torch.ones(d, d), -1) * (torch.rand(d, d, generator=gen) < .5).float()).numpy().astype(np.uint8)


def normalizer(norm):
    """(class, arguments, conditioner outputs) of --norms' names"""
    from models import AffineNormalizer, MonotonicNormalizer, SplineNormalizer
    if norm == "affine":
        return AffineNormalizer, {}, 2
    if norm == "spline":
        return SplineNormalizer, {"nb_bins": 8, "tail_bound": 3.}, 23
    return MonotonicNormalizer, {"integrand_net": [50, 50, 50], "cond_size": 4, "nb_steps": 20, "solver": "CC"}, 4


def make(kind, d, hidden, a, gain=1., out=2, norm="affine"):
    from models import AffineNormalizer, AutoregressiveConditioner, DAGConditioner, buildFCNormalizingFlow
    torch.manual_seed(0)
    if norm != "affine":
        N, nargs, out = normalizer(norm)
    else:
        N, nargs = AffineNormalizer, {}
    if kind == "strade":
        flow = buildFCNormalizingFlow(1, "StrADE", {"in_size": d, "hidden": hidden, "out_size": out, "adjacency": a}, N, nargs)
    elif kind == "made":
        flow = buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": d, "hidden": hidden, "out_size": out}, N, nargs)
    else:
        flow = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": hidden, "out_size": out, "hot_encoding": True,
                                                          "A_prior": torch.from_numpy(a).float()}, AffineNormalizer, {})
    if gain != 1.:
        with torch.no_grad():
            for n, p in flow.steps[0].conditioner.named_parameters():
                if n.endswith("weight"):
                    p.mul_(gain)
    flow = flow.to(DEV)
    if kind == "dag":
        flow.steps[0].conditioner.post_process()
    return flow.steps[0]


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def alternate(fns, reps):
    """{name: (median, min, max) in ms} of the callables, run back to back in turn `reps` times after one warm-up round"""
    for fn in fns.values():
        clock(fn)
        clock(fn)
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(clock(fn)[0])
    return {k: (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v)) for k, v in times.items()}


def fmt(name, t):
    return "%s %.3f ms (min %.3f, max %.3f)" % ((name,) + t)


def part_a(name, reps):
    d, hidden, B = SHAPES[name]
    a = graph(name, d)
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(2)).to(DEV)
    fns = {}
    for kind in ("strade", "dag", "made"):
        if kind == "dag" and name == "mnist":
            continue                                   # B d = 78 400 rows through a [784 + 784, 1024] MLP: the image flows' business
        cond = make(kind, d, hidden, a).conditioner

        def run(cond=cond):
            for p in cond.parameters():
                p.grad = None
            cond(x).square().sum().backward()
        fns[kind] = run
    t = alternate(fns, reps)
    line = "fwd+bwd %s d=%d %s B=%d edges=%d: " % (name, d, hidden, B, int(a.sum())) + ", ".join(fmt(k, v) for k, v in t.items())
    if "dag" in t:
        line += ", dag / strade = %.2f" % (t["dag"][0] / t["strade"][0])
    return line + ", strade / made = %.2f, median of %d" % (t["strade"][0] / t["made"][0], reps)


def part_b(name, gain, full, reps):
    d, hidden, B = SHAPES[name]
    a = graph(name, d, full)
    step = make("strade", d, hidden, a, gain)
    z = (.7 * torch.randn(B, d, generator=torch.Generator().manual_seed(1))).to(DEV)

    def arm(on):
        def run():
            step.column_schedule = on
            return step.invert(z)
        return run
    fns = {"levels": arm(True), "passes": arm(False)}
    if full:
        made = make("made", d, hidden, a, gain)
        fns["made columns"] = lambda: made.invert(z)
    t = alternate(fns, reps)
    step.column_schedule = True
    took = step.intervene(z, [], 0.) is not None and step._intervene_arm
    x_on, x_off = fns["levels"](), fns["passes"]()
    calls = []
    hook = step.conditioner.register_forward_hook(lambda *a: calls.append(1))
    fns["passes"]()
    hook.remove()
    line = ("invert %s%s d=%d B=%d gain=%g depth=%d arm=%s: " % (name, " full-triangular" if full else "", d, B, gain,
                                                                   step.conditioner.depth(), took)
            + ", ".join(fmt(k, v) for k, v in t.items())
            + " (%d of %d passes), passes / levels = %.2f" % (len(calls), step.conditioner.depth() + 1, t["passes"][0] / t["levels"][0]))
    if full:
        line += ", levels / made columns = %.2f" % (t["levels"][0] / t["made columns"][0])
    diff = ((x_on - x_off).abs().max() / x_off.abs().max()).item()
    return line + ", max|x_levels - x_passes| / max|x| = %.2e, median of %d" % (diff, reps)


def part_c(name, reps):
    d, hidden, B = SHAPES[name]
    a = graph(name, d)
    z = (.7 * torch.randn(B, d, generator=torch.Generator().manual_seed(1))).to(DEV)
    steps = {"made": make("made", d, hidden, a), "dag": make("dag", d, hidden, a)}
    t = alternate({k: (lambda s=s: s.invert(z)) for k, s in steps.items()}, reps)
    return "parent-ab invert %s d=%d B=%d: " % (name, d, B) + ", ".join(fmt(k, v) for k, v in t.items()) + ", median of %d" % reps


def _backward_arm(step, x, g, on=None):
    """the rsample backward of `step` at the sample x for the cotangent g; on: the conditioner's `adjoint_levels`"""
    params = [p for p in step.parameters() if p.requires_grad]

    def run():
        if on is not None:
            step.conditioner.adjoint_levels = on
        return step._rsample_backward(x, None, params, g, False)[0]
    return run


def part_d(name, norm, gain, full, reps):
    d, hidden, B = SHAPES[name]
    a = graph(name, d, full)
    step = make("strade", d, hidden, a, gain, norm=norm)
    gen = torch.Generator().manual_seed(1)
    z = (.7 * torch.randn(B, d, generator=gen)).to(DEV)
    g = torch.randn(B, d, generator=gen).to(DEV)
    with torch.no_grad():
        x = step.invert(z)
    fns = {"adjoint-levels": _backward_arm(step, x, g, True), "passes": _backward_arm(step, x, g, False)}
    if full:
        made = make("made", d, hidden, a, gain, norm=norm)
        with torch.no_grad():
            xm = made.invert(z)
        fns["made adjoint"] = _backward_arm(made, xm, g)
    t = alternate(fns, reps)
    lam_on = fns["adjoint-levels"]()
    arm_on = step._rsample_arm
    lam_off = fns["passes"]()
    arm_off = step._rsample_arm
    step.conditioner.adjoint_levels = False
    line = ("rsample-backward %s%s %s d=%d B=%d gain=%g depth=%d nlev=%d arms=%s/%s: "
            % (name, " full-triangular" if full else "", norm, d, B, gain, step.conditioner.depth(), step.conditioner.depth() + 1,
               "%s:%d" % arm_on, "%s:%d" % arm_off)
            + ", ".join(fmt(k, v) for k, v in t.items())
            + ", passes / adjoint-levels = %.2f (yardstick: the passes arm of the same process)" % (t["passes"][0] / t["adjoint-levels"][0]))
    if full:
        line += ", adjoint-levels / made adjoint = %.2f" % (t["adjoint-levels"][0] / t["made adjoint"][0])
    diff = ((lam_on - lam_off).abs().max() / lam_off.abs().max()).item()
    return line + ", max|lam_adjoint - lam_passes| / max|lam| = %.2e, median of %d" % (diff, reps)


def part_e(name, reps):
    d, hidden, B = SHAPES[name]
    a = graph(name, d)
    gen = torch.Generator().manual_seed(1)
    z = (.7 * torch.randn(B, d, generator=gen)).to(DEV)
    g = torch.randn(B, d, generator=gen).to(DEV)
    strade, made = make("strade", d, hidden, a), make("made", d, hidden, a)
    with torch.no_grad():
        xm = made.invert(z)
    t = alternate({"strade invert (level kernel)": lambda: strade.invert(z),
                   "made rsample backward (adjoint kernel)": _backward_arm(made, xm, g)}, reps)
    assert made._rsample_arm == ("adjoint", 0) and strade._fast_arm(z, None)[0] == "strade"
    return "parent-ab %s d=%d B=%d: " % (name, d, B) + ", ".join(fmt(k, v) for k, v in t.items()) + ", median of %d" % reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--gains", default="1,4")
    ap.add_argument("--norms", default="affine,spline,monotonic")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "graphical-normalizing-flows_amd"),
                    help="the package directory to import models and gnf_hip from (another checkout for part c)")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path[:0] = [os.path.dirname(os.path.abspath(args.pkg)), os.path.abspath(args.pkg)]
    assert torch.cuda.is_available(), "timing needs the MI355X"
    parts, shapes = args.parts.split(","), args.shapes.split(",")

    def emit(line):                                    # line by line: a run cut short keeps what it measured
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    for name in shapes:
        if "a" in parts:
            emit(part_a(name, args.reps))
        if "b" in parts:
            for gain in [float(g) for g in args.gains.split(",")]:
                for full in ((False, True) if name != "mnist" else (False,)):
                    emit(part_b(name, gain, full, args.reps))
        if "c" in parts and name != "mnist":
            emit(args.label + part_c(name, args.reps))
        if "d" in parts:
            for norm in args.norms.split(","):
                for gain in [float(g) for g in args.gains.split(",")]:
                    for full in ((False, True) if name != "mnist" else (False,)):
                        emit(part_d(name, norm, gain, full, args.reps))
        if "e" in parts and name != "mnist":
            emit(args.label + part_e(name, args.reps))


if __name__ == "__main__":
    main()
