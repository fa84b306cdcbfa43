"""A/B of the DAGMLP front with the DAG gate and the one-hot fused into the first layer (`DAGMLP.gated_front`,
gnf_hip.ops.DagMlpFrontFn / dag_mlp_rows: the masked copies are built in LDS) against the composed path
(`gated_front = False`: DagGateFn writes e [B d, 2 d], MLPFn reads it; forward_rows builds the broadcast product with torch).

    python tools/bench_dagmlp_gated.py [--pairs 7] [--reps 100] [--out profiles/dagmlp_gated_ab.txt]

One process, HIP events around `reps` calls ending in a synchronise, warm-up first, alternating pairs.  A DAG conditioner
with hot encoding at the UCI shapes, x as data:
  train   conditioner forward + backward with the stochastic gate at T = .5 (the UCI driver's setting);
  frozen  the same behind the frozen deterministic gate (after post_process());
  eval    a no-grad evaluation of all rows behind that gate.
Each variant also reports torch.cuda.max_memory_allocated above the level before one call.  The rule for the default of
`gated_front` is the one of the previous adoptions: on only if the fused path wins EVERY pair of the training form at EVERY
shape."""
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


def make(d, emb, frozen, dev):
    from models import DAGConditioner
    torch.manual_seed(d)
    cond = DAGConditioner(d, emb[:-1], emb[-1], l1=.2, gumble_T=.5, hot_encoding=True).to(dev)
    if frozen:
        with torch.no_grad():
            cond.A.copy_(torch.tril(torch.ones(d, d), -1).to(dev) * 1.5)
        cond.post_process()
    return cond


def variants(cond, x, cot, mode):
    def step(on):
        def fn():
            cond.embedding_net.gated_front = on
            if mode == "eval":
                with torch.no_grad():
                    cond(x)
                return
            cond.zero_grad(set_to_none=True)
            (cond(x) * cot).sum().backward()
        return fn
    return (("fused", step(True)), ("composed", step(False)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dagmlp_gated_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dagmlp_gated.py needs an MI355X")
    dev = torch.device("cuda", 0)
    lines = ["DAGMLP front, gate + one-hot fused into the first layer (fused) against DagGateFn + MLPFn (composed)",
             "ms per call (HIP events over %d calls), %d alternating pairs after %d warm-up calls; peak = bytes allocated above "
             "the operands in one call" % (args.reps, args.pairs, args.warmup), ""]
    lost = []
    for name, B, d, emb in SHAPES:
        gen = torch.Generator().manual_seed(B + d)
        x = torch.randn(B, d, generator=gen).to(dev)
        cot = torch.randn(B, d, emb[-1], generator=gen).to(dev)
        for mode in ("train", "frozen", "eval"):
            cond = make(d, emb, mode != "train", dev)
            vs = variants(cond, x, cot, mode)
            for _ in range(args.warmup):
                for _, fn in vs:
                    fn()
            torch.cuda.synchronize()
            times = {n: [] for n, _ in vs}
            for _ in range(args.pairs):
                for n, fn in vs:
                    times[n].append(timed(fn, args.reps))
            peaks = {n: peak_of(fn) for n, fn in vs}
            wins = sum(f < c for f, c in zip(times["fused"], times["composed"]))
            med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
            lines.append("%-14s B %5d d %2d %-6s fused %8.4f composed %8.4f  ratio %.3f  fused wins %d/%d  peak fused %10d "
                         "composed %10d" % (name, B, d, mode, med["fused"], med["composed"], med["fused"] / med["composed"],
                                            wins, args.pairs, peaks["fused"], peaks["composed"]))
            lines.append("    fused    " + " ".join("%.4f" % t for t in times["fused"]))
            lines.append("    composed " + " ".join("%.4f" % t for t in times["composed"]))
            if mode == "train" and wins < args.pairs:
                lost.append("%s (B %d): %d of %d pairs" % (name, B, args.pairs - wins, args.pairs))
            print(lines[-3], flush=True)
    lines += ["", "training form, pairs lost by the fused path: " + ("; ".join(lost) if lost else "none"),
              "DAGMLP_GATED_FRONT_DEFAULT = %s by the adoption rule" % (not lost)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
