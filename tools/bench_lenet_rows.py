"""A/B of the row-subset LeNet front of CIFAR10CNN (`rows_front`, gnf_hip.ops.lenet_rows: the masked copies x[b] * P[i] of a
deterministic DAG gate are built in LDS) against the broadcast product (`rows_front = False`: x.unsqueeze(1) * P[rows] in
memory, then gnf_lenet_conv_fwd on its B*R rows).

    python tools/bench_lenet_rows.py [--pairs 7] [--out profiles/lenet_rows_ab.txt]

One process on a quiet device, HIP events, warm-up first, alternating pairs, B = 8, everything under no_grad.  A DAG
conditioner with a deterministic gate over CIFAR10CNN at (3,32,32,5) and (1,32,32,3): DAGConditioner.forward_rows over all d
rows, in the [R, B, out] layout the inversion asks for.  Then one full `invert` of the one-scale Affine CIFAR-10 flow whose A
is frozen to a fixed sparse DAG, launch by launch and as the replayed hipGraph.  Each variant also reports
torch.cuda.max_memory_allocated above the level before the call.  The rule for the default of `rows_front` is the one of the
previous adoptions: on only if forward_rows wins every pair of both geometries."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "graphical-normalizing-flows_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

CASES = (((3, 32, 32), 5, (400, 128, 84)),
         ((1, 32, 32), 3, (576, 128, 32)))
B = 8


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def peak_of(fn):
    """bytes torch allocated at the peak of fn() above the level before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def ab(variants, pairs, warmup=3, peaks=True):
    """{name: [ms]} over alternating rounds, {name: peak bytes}"""
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(pairs):
        for name, fn in variants:
            times[name].append(timed(fn))
    return times, {name: peak_of(fn) if peaks else None for name, fn in variants}


def report(lines, variants, times, peaks):
    for name, _ in variants:
        ts = times[name]
        peak = "" if peaks[name] is None else "   peak %.1f MB" % (peaks[name] / 1e6)
        lines.append("%-24s %s   median %.3f%s" % (name, " ".join("%8.3f" % t for t in ts), sorted(ts)[len(ts) // 2], peak))


def sparse_dag(d, seed=0):
    """0/1 adjacency of a fixed DAG: a random order of the variables, a chain through its first 8, 2 random earlier parents
    per variable"""
    gen = torch.Generator().manual_seed(seed)
    order = torch.randperm(d, generator=gen)
    A = torch.zeros(d, d)
    A[order[1:8], order[0:7]] = 1.
    for t in range(1, d):
        A[order[t], order[torch.randint(0, t, (2,), generator=gen)]] = 1.
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from models import AffineNormalizer, DAGConditioner
    from models.MLP import CIFAR10CNN
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow
    lines = ["Row-subset CIFAR10CNN front (rows_front = True, csrc/gnf_lenetcnn.hip lenet_rows_fwd_k) vs the broadcast product "
             "(rows_front = False: x.unsqueeze(1) * P[rows] in memory + gnf_lenet_conv_fwd)",
             "device: %s, torch %s; HIP events, ms; %d alternating pairs after warm-up; B = %d; no_grad; peak = "
             "torch.cuda.max_memory_allocated above the level before the call" %
             (torch.cuda.get_device_name(0), torch.__version__, args.pairs, B)]
    all_win = True
    with torch.no_grad():
        for size_img, k, fc_l in CASES:
            d = size_img[0] * size_img[1] * size_img[2]
            torch.manual_seed(0)
            net = CIFAR10CNN(out_d=2, fc_l=list(fc_l), size_img=list(size_img), k_size=k)
            cond = DAGConditioner(d, net, 2).cuda()
            cond.stoch_gate = False
            x = torch.randn(B, d, device="cuda")
            P = cond.deterministic_importance()
            rows = torch.arange(d, device="cuda")
            host_rows, rows32 = tuple(range(d)), rows.to(torch.int32)

            def fwd_rows(on):
                net.rows_front = on
                cond.forward_rows(x, rows, P, host_rows, variable_major=True, rows32=rows32)

            variants = (("product forward_rows", lambda: fwd_rows(False)), ("rows forward_rows", lambda: fwd_rows(True)))
            times, peaks = ab(variants, args.pairs)
            lines += ["", "forward_rows over all d rows, geometry (C,H,W,k) = (%d,%d,%d,%d): d = %d, %d masked copies, the "
                      "product = %.1f MB" % (*size_img, k, d, B * d, B * d * d * 4 / 1e6)]
            report(lines, variants, times, peaks)
            wins = sum(f < t for f, t in zip(times["rows forward_rows"], times["product forward_rows"]))
            lines.append("rows forward_rows faster than product forward_rows in %d of %d pairs" % (wins, args.pairs))
            all_win = all_win and wins == args.pairs
            del cond, net, x, P
        # one full inversion of the one-scale Affine flow over a fixed sparse DAG
        torch.manual_seed(0)
        flow = buildCIFAR10NormalizingFlow([1], AffineNormalizer, {}).cuda()
        step = flow.steps[0]
        cond, net = step.conditioner, step.conditioner.embedding_net
        cond.stoch_gate = cond.noise_gate = cond.s_thresh = False
        cond.h_thresh = 0.
        cond.A.copy_(sparse_dag(3072).cuda())
        cond.A.requires_grad = False
        cond.invalidate_caches()
        cond.is_invertible = True
        z = torch.randn(B, 3072, device="cuda")

        def invert(on, graphed):
            net.rows_front, step.graph_invert = on, graphed
            flow.invert(z)
        lines += ["", "one invert of buildCIFAR10NormalizingFlow([1], AffineNormalizer, {}) at B = %d, A frozen to a 0/1 DAG with "
                  "%d levels (%d edges):" % (B, len(cond.levels()), int(cond.A.sum().item()))]
        for graphed, label in ((False, "eager"), (True, "hipGraph")):
            variants = (("product invert %s" % label, lambda: invert(False, graphed)),
                        ("rows invert %s" % label, lambda: invert(True, graphed)))
            times, peaks = ab(variants, args.pairs, warmup=3, peaks=not graphed)   # a replay allocates its result only
            report(lines, variants, times, peaks)
            a, b = variants[1][0], variants[0][0]
            wins = sum(f < t for f, t in zip(times[a], times[b]))
            lines.append("%s faster than %s in %d of %d pairs" % (a, b, wins, args.pairs))
    lines += ["", "rule: rows_front defaults to True only if rows forward_rows is faster in every pair of both geometries: %s" %
              ("met" if all_win else "NOT met"),
              "decision: ROWS_FRONT_DEFAULT = %s (models/MLP.py)%s" %
              (all_win, "" if all_win else "; rows_front stays opt-in, for the batches whose product does not fit")]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
