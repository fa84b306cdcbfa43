"""A/B of the first DAGMLP layer of a CONDITIONAL DAG conditioner (cond_in > 0): the context half of the layer as one
[B, cond_in] x [cond_in, H] product added to the d rows of each sample by the streaming group-bias kernel
(`DAGMLP.context_bias = True`: csrc/gnf_group_bias.hip, gnf_hip.ops.GroupBiasFn) against the plain formulation
(`context_bias = False`: the context repeated d times, concatenated to the masked copies and contracted with them).

    python tools/bench_context_front.py [--pairs 7] [--reps 50] [--out profiles/context_front_ab.txt]

One process, HIP events around `reps` calls ending in a synchronise, warm-up first, the two arms alternating.  A DAG
conditioner with hot encoding and the stochastic gate at T = .5 (the UCI driver's setting) at the tabular shapes of
uci_configs.yml, conditioner forward + backward with gradients for every parameter (x and the context are data), cond_in 1
and 8.  The rule for the default of `context_bias`: on everywhere if the bias form wins or ties (median within 1 %) at every
shape measured; otherwise on only where it wins; off if it wins nowhere."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "graphical-normalizing-flows_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

# (set, B, d, embedding net)
SHAPES = (("POWER", 2500, 6, [60, 60, 60, 30]),
          ("POWER (bench)", 10000, 6, [60, 60, 60, 30]),
          ("GAS", 10000, 8, [80, 80, 80, 30]),
          ("HEPMASS", 100, 21, [210, 210, 210, 30]),
          ("MINIBOONE", 100, 43, [430, 430, 430, 30]),
          ("BSDS300", 100, 63, [630, 630, 630, 30]))
COND_IN = (1, 8)
TIE = .01


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def peak_of(fn):
    """bytes torch allocated at the peak of fn() above the level before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def variants(cond, x, ctx, cot):
    def step(on):
        def fn():
            cond.embedding_net.context_bias = on
            cond.zero_grad(set_to_none=True)
            (cond(x, ctx) * cot).sum().backward()
        return fn
    return (("bias", step(True)), ("concat", step(False)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_front_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_context_front.py needs an MI355X")
    from models import DAGConditioner
    dev = torch.device("cuda", 0)
    lines = ["DAGMLP first layer with a context: per-sample bias + group-bias kernel (bias) against concatenated rows (concat)",
             "conditioner forward + backward, ms per call (HIP events over %d calls), %d alternating pairs after %d warm-up "
             "calls; peak = bytes allocated above the operands in one call" % (args.reps, args.pairs, args.warmup), ""]
    verdicts = []
    for name, B, d, emb in SHAPES:
        for c in COND_IN:
            torch.manual_seed(d + c)
            cond = DAGConditioner(d, emb[:-1], emb[-1], cond_in=c, l1=.2, gumble_T=.5, hot_encoding=True).to(dev)
            gen = torch.Generator().manual_seed(B + d + c)
            x = torch.randn(B, d, generator=gen).to(dev)
            ctx = torch.randn(B, c, generator=gen).to(dev)
            cot = torch.randn(B, d, emb[-1], generator=gen).to(dev)
            vs = variants(cond, x, ctx, cot)
            for _ in range(args.warmup):
                for _, fn in vs:
                    fn()
            torch.cuda.synchronize()
            times = {n: [] for n, _ in vs}
            for _ in range(args.pairs):
                for n, fn in vs:
                    times[n].append(timed(fn, args.reps))
            peaks = {n: peak_of(fn) for n, fn in vs}
            wins = sum(f < g for f, g in zip(times["bias"], times["concat"]))
            med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
            ratio = med["bias"] / med["concat"]
            verdict = "wins" if ratio < 1. - TIE else ("ties" if ratio <= 1. + TIE else "loses")
            verdicts.append((name, B, d, c, ratio, verdict))
            lines.append("%-14s B %5d d %2d cond_in %d  bias %8.4f concat %8.4f  ratio %.3f (%s)  bias wins %d/%d  peak bias %10d "
                         "concat %10d" % (name, B, d, c, med["bias"], med["concat"], ratio, verdict, wins, args.pairs,
                                          peaks["bias"], peaks["concat"]))
            lines.append("    bias   " + " ".join("%.4f" % t for t in times["bias"]))
            lines.append("    concat " + " ".join("%.4f" % t for t in times["concat"]))
            print(lines[-3], flush=True)
    lost = ["%s B %d cond_in %d (%.3f)" % (n, B, c, r) for n, B, d, c, r, v in verdicts if v == "loses"]
    won = [v for v in verdicts if v[5] == "wins"]
    lines += ["", "tie band: median ratio within %.0f %% of 1" % (100 * TIE),
              "shapes the bias form loses: " + ("; ".join(lost) if lost else "none"),
              "rule: %s" % ("on everywhere (wins or ties at every shape measured)" if not lost
                            else "off (wins nowhere)" if not won else "on only where it wins: a shape rule is needed")]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))


if __name__ == "__main__":
    main()
