"""Time the backward of NormalizingFlowStep.rsample_do(z, do_index, do_value, ctx) -- the gradient of an interventional
sample -- in one process and one build, arms alternating:
    adjoint   `adjoint_schedule = True` (StrADE: `adjoint_levels` on): one launch of gnf_made_adjoint_do / gnf_strade_adjoint_do
              with the pin table, its weight image packed inside the timed window;
    passes    `adjoint_schedule = False` (`adjoint_levels` off): lambda <- where(pinned, 0, (g - N^T lambda) / jac), at most
              depth() vjps of the existing kernels with early exit (the number taken is on the line), one more for dL/dv;
    rsample   the un-pinned backward of the same step at its own sample (adjoint arm): what the pins are measured against.
All three then make the same vjp of the step for the parameter and context gradients; the sample is outside the timed window.
    made-power / made-bsds / made-784 / mono-power / mono-bsds    the shapes of tools/bench_rsample.py (with a context)
    strade-miniboone / strade-bsds                                the Affine + StrADE shapes of tools/bench_strade.py, no context
Every shape as initialised (--gains 1) and with every conditioner weight matrix multiplied by 4; pins by position in the
topological order (degrees of a MADE, level order of a StrADE net): none / every second / the last half -- the last half is a
trailing pinned run, which the kernels skip; with gdo (do_value requires grad) and without.

--parent-ab times the un-pinned rsample backward alone, for a comparison against another checkout: run the tool once per
checkout (--pkg names the package directory to import, --label the checkout), alternating processes, and compare the lines.

Warm-up, then the median of repeated runs; a host clock around work that ends in a device synchronise.

    python tools/bench_rsample_do.py [--out profiles/rsample_do_ab.txt] [--reps 7] [--shapes made-power,strade-bsds] [--gains 1,4]
    python tools/bench_rsample_do.py --parent-ab --label "this: " [--pkg DIR] [--out ...]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# name -> (kind, d, c, hidden, B)
SHAPES = {"made-power": ("made", 6, 2, [60, 60, 60], 2500),
          "made-bsds": ("made", 63, 8, [630], 2000),
          "made-784": ("made", 784, 10, [1024, 1024, 1024], 100),
          "mono-power": ("mono", 6, 2, [60, 60, 60], 2500),
          "mono-bsds": ("mono", 63, 8, [630], 2000),
          "strade-miniboone": ("strade", 43, 0, [430], 1000),
          "strade-bsds": ("strade", 63, 0, [630], 2000)}
PINS = ("none", "every-second", "last-half")


def make(kind, d, c, hidden, gain):
    from models import AffineNormalizer, AutoregressiveConditioner, MonotonicNormalizer, buildFCNormalizingFlow
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
        a = (torch.tril(torch.ones(d, d), -1) * (torch.rand(d, d, generator=gen) < .5).float()).numpy().astype("uint8")
        flow = buildFCNormalizingFlow(1, "StrADE", {"in_size": d, "hidden": hidden, "out_size": 2, "adjacency": a},
                                      AffineNormalizer, {})
    if gain != 1.:
        with torch.no_grad():
            for n, p in flow.steps[0].conditioner.named_parameters():
                if n.endswith("weight"):
                    p.mul_(gain)
    return flow.to(DEV).steps[0]


def order_of(step, kind, z, ctx):
    """position in the topological order -> variable"""
    if kind == "strade":
        order = step.conditioner.level_plan()["var_order"]
    else:
        order = step.conditioner.prefix_plan(with_context=ctx is not None)["var_of_step"]
    return [int(v) for v in torch.as_tensor(order).tolist()]


def pinned(name, order):
    d = len(order)
    pos = {"none": [], "every-second": range(1, d, 2), "last-half": range(d - d // 2, d)}[name]
    return tuple(order[p] for p in pos)


def set_arm(step, kind, on):
    if kind == "strade":
        step.conditioner.adjoint_levels = on
    else:
        step.adjoint_schedule = on


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def alternate(fns, reps):
    """{name: (median, min, max) in ms} of the callables, run back to back in turn `reps` times after two warm-up rounds"""
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


def operands(kind, d, c, B):
    gen = torch.Generator().manual_seed(1)
    z = (.7 * torch.randn(B, d, generator=gen)).to(DEV)
    ctx = torch.randn(B, c, generator=gen).to(DEV) if c else None
    g = torch.randn(B, d, generator=gen).to(DEV)
    return z, ctx, g


def rows(name, gain, reps):
    kind, d, c, hidden, B = SHAPES[name]
    step = make(kind, d, c, hidden, gain)
    params = [p for p in step.parameters() if p.requires_grad]
    z, ctx, g = operands(kind, d, c, B)
    order = order_of(step, kind, z, ctx)
    with torch.no_grad():
        x0 = step.invert(z, ctx)
    arms = {}

    def unpinned():
        set_arm(step, kind, True)
        out = step._rsample_backward(x0, ctx, params, g, ctx is not None)
        arms["rsample"] = step._rsample_arm
        return out[0]

    for pins in PINS:
        idx = pinned(pins, order)
        x = step.intervene(z, list(idx), 0., ctx)
        for want_v in (True, False):
            def backward(on, idx=idx, x=x, want_v=want_v):
                def run():
                    set_arm(step, kind, on)
                    out = step._rsample_do_backward(x, ctx, params, g, idx, ctx is not None, want_v)
                    arms[on] = step._rsample_arm
                    return out[0], out[1]
                return run
            fns = {"adjoint": backward(True), "passes": backward(False), "rsample": unpinned}
            t = alternate(fns, reps)
            (lam_on, gv_on), (lam_off, gv_off) = fns["adjoint"](), fns["passes"]()
            assert arms[True] == ("adjoint", 0) and arms[False][0] == "passes" and arms["rsample"] == ("adjoint", 0), arms
            diff = ((lam_on - lam_off).abs().max() / lam_off.abs().max().clamp_min(1e-30)).item()
            line = ("rsample_do-backward %s d=%d c=%d B=%d gain=%g pins=%s (%d of %d) gdo=%s: %s, %s (%d of %d vjps), %s, "
                    "passes / adjoint = %.2f, adjoint / rsample = %.2f, max|lam_adjoint - lam_passes| / max|lam| = %.2e"
                    % (name, d, c, B, gain, pins, len(idx), d, "yes" if want_v else "no", fmt("adjoint", t["adjoint"]),
                       fmt("passes", t["passes"]), arms[False][1], step.conditioner.depth(), fmt("rsample", t["rsample"]),
                       t["passes"][0] / t["adjoint"][0], t["adjoint"][0] / t["rsample"][0], diff))
            if want_v and idx:
                line += ", max|dv_adjoint - dv_passes| / max|g| = %.2e" % ((gv_on - gv_off).abs().max() / g.abs().max()).item()
            yield line + ", median of %d" % reps
    set_arm(step, kind, kind != "strade")


def parent_row(name, reps):
    """the un-pinned rsample backward alone, through the public rsample: what a checkout without rsample_do runs too"""
    kind, d, c, hidden, B = SHAPES[name]
    step = make(kind, d, c, hidden, 1.)
    set_arm(step, kind, True)
    params = [p for p in step.parameters() if p.requires_grad]
    z, ctx, g = operands(kind, d, c, B)
    with torch.no_grad():
        x0 = step.invert(z, ctx)
    t = alternate({"rsample": lambda: step._rsample_backward(x0, ctx, params, g, ctx is not None)[0]}, reps)
    assert step._rsample_arm == ("adjoint", 0)
    return "parent-ab rsample-backward %s d=%d c=%d B=%d: %s, median of %d" % (name, d, c, B, fmt("rsample", t["rsample"]), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--gains", default="1,4")
    ap.add_argument("--parent-ab", action="store_true")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "graphical-normalizing-flows_amd"),
                    help="the package directory to import models and gnf_hip from (another checkout for --parent-ab)")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path[:0] = [os.path.dirname(os.path.abspath(args.pkg)), os.path.abspath(args.pkg)]
    assert torch.cuda.is_available(), "timing needs the MI355X"

    def emit(line):                                    # line by line: a run cut short keeps what it measured
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    for name in args.shapes.split(","):
        if args.parent_ab:
            emit(args.label + parent_row(name, args.reps))
            continue
        for gain in [float(g) for g in args.gains.split(",")]:
            for line in rows(name, gain, args.reps):
                emit(line)


if __name__ == "__main__":
    main()
