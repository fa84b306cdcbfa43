"""A/B of the graph queries of a DAG conditioner on the device (`DAGConditioner.device_graph`, gnf_hip.ops.dag_levels: the
predicate packed into bits, zero-in-degree nodes peeled by one workgroup per graph) against the host statements
(`device_graph = False`: a copy of the d x d matrix to the CPU and a networkx / Python walk there).

    python tools/bench_dag_graph.py [--pairs 7] [--out profiles/dag_graph_ab.txt] [--kernels-only]

One process, the arms alternate, a host clock around calls that end in a synchronise (both arms end in a host read), the
median of the pairs; Python's cyclic garbage is collected before every timed call, outside the clock.  Per case
`levels(with_host=True)`, `depth()` and `post_process()` of one conditioner; A is put back outside the clock after every
post_process().  The cases: seeded permuted-triangular DAGs at the five UCI sizes d = 6 .. 63, the 5x5 MNIST
prior at d = 784 (symmetric windows: cyclic, the post-processing search runs to .8) and its lower triangle (a DAG), and at
d = 3072 the same DAGs at densities .01 / .1 / .5 and the chain 0 -> 1 -> ... -> 3071 (the most rounds the peel can run).
Last, the post_process() search on A = 1.5 + .02 randn at d = 3072, the state of a new CIFAR conditioner: every low
threshold is the complete graph, which the host arm turns into a networkx DiGraph of 9.4 M edges per candidate -- that arm
is timed ONCE and for the FIRST candidate only (`--dense-host-candidates`), and the file says so.

Then gnf_dag_levels alone from device events at every d: the empty graph (the pack kernel + one round of the peel), the
density-.1 DAG and the chain (d rounds).  `--kernels-only` runs just that part, for a per-kernel trace
(tools/kstats.sh).

The rule for DEVICE_GRAPH_DEFAULT is the one of the previous adoptions: on only if the device arm wins EVERY pair of EVERY
case; if it loses only at small d, on above a DEVICE_GRAPH_MIN_D read off this table."""
import argparse
import gc
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "graphical-normalizing-flows_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def perm_dag(d, density, seed):
    """weights in [1, 2) on a seeded strictly lower-triangular pattern under a random permutation of the nodes"""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(d, generator=g)
    low = torch.tril((torch.rand(d, d, generator=g) < density).float(), -1) * (1. + torch.rand(d, d, generator=g))
    A = torch.zeros(d, d)
    A[perm.unsqueeze(1), perm.unsqueeze(0)] = low
    return A


def chain(d):
    A = torch.zeros(d, d)
    A[torch.arange(1, d), torch.arange(d - 1)] = 1.5
    return A


def cases():
    from models.NormalizingFlowFactories import MNIST_A_prior
    prior = MNIST_A_prior(28, 2)
    return (("POWER d 6, density .5", lambda: perm_dag(6, .5, 6)),
            ("GAS d 8, density .5", lambda: perm_dag(8, .5, 8)),
            ("HEPMASS d 21, density .5", lambda: perm_dag(21, .5, 21)),
            ("MINIBOONE d 43, density .5", lambda: perm_dag(43, .5, 43)),
            ("BSDS300 d 63, density .5", lambda: perm_dag(63, .5, 63)),
            ("MNIST d 784, 5x5 prior (cyclic)", lambda: prior.clone()),
            ("MNIST d 784, prior, lower triangle", lambda: prior * torch.tril(torch.ones(784, 784), -1)),
            ("d 3072, density .01", lambda: perm_dag(3072, .01, 1)),
            ("d 3072, density .1", lambda: perm_dag(3072, .1, 2)),
            ("d 3072, density .5", lambda: perm_dag(3072, .5, 3)),
            ("d 3072, chain", lambda: chain(3072)))


def conditioner(A, dev):
    from models import DAGConditioner
    torch.manual_seed(0)
    cond = DAGConditioner(A.shape[0], [8], 2, A_prior=A.clone())
    return cond.to(dev)


def reopen(cond, A0):
    """undo post_process() (outside the clock)"""
    cond.stoch_gate, cond.noise_gate, cond.s_thresh, cond.h_thresh = True, False, True, 0.
    with torch.no_grad():
        cond.A.copy_(A0)
    cond.A.requires_grad = True
    cond.invalidate_caches()


def clocked(fn):
    # the host arm leaves networkx graphs behind (millions of dicts in reference cycles at d = 3072): collected here, outside
    # the clock, or Python's collector stops whichever arm runs next for up to seconds
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(out):
    if out is None or isinstance(out, int):
        return out
    return "%d levels" % len(out)


def ab(lines, name, cond, A0, pairs, warm_host):
    queries = (("levels", lambda: cond.levels(with_host=True)), ("depth", cond.depth), ("post_process", cond.post_process))
    for qname, fn in queries:
        times, outs = {True: [], False: []}, {}
        for it in range(-1, pairs):                               # -1: warm-up (the host arm only where it is cheap)
            for on in (True, False):
                if it < 0 and not on and not warm_host:
                    continue
                cond.device_graph = on
                ms, out = clocked(fn)
                if qname == "post_process":
                    out = cond.A.detach().clone()
                    reopen(cond, A0)
                if it >= 0:
                    times[on].append(ms)
                    outs[on] = out
        if qname == "post_process":
            same = torch.equal(outs[True], outs[False])
            what = "%d edges kept" % int(outs[True].sum())
        else:
            key = lambda o: o if o is None or isinstance(o, int) else [h for _, h in o]
            same, what = key(outs[True]) == key(outs[False]), summary(outs[True])
        med = {on: sorted(t)[len(t) // 2] for on, t in times.items()}
        wins = sum(a < b for a, b in zip(times[True], times[False]))
        lines.append("%-36s %-13s device %10.3f host %10.3f ms  ratio %.4f  device wins %d/%d  same answer %s (%s)"
                     % (name, qname, med[True], med[False], med[True] / med[False], wins, pairs, same, what))
        lines.append("    device " + " ".join("%.3f" % t for t in times[True]))
        lines.append("    host   " + " ".join("%.3f" % t for t in times[False]))
        print(lines[-3], flush=True)
        yield qname, wins


def dense_search(lines, dev, host_candidates):
    """post_process() of a new CIFAR conditioner.  The host arm: the parent's statements for the first `host_candidates`
    thresholds of the search, once."""
    import networkx as nx
    from models.Conditionners.DAGConditioner import _digraph, threshold_candidates
    torch.manual_seed(7)
    from models import DAGConditioner
    cond = DAGConditioner(3072, [8], 2).to(dev)
    A0 = cond.A.detach().clone()
    cond.device_graph = True
    times = []
    for it in range(-1, 7):
        ms, _ = clocked(cond.post_process)
        kept = int(cond.A.sum())
        reopen(cond, A0)
        if it >= 0:
            times.append(ms)
    S = cond.soft_thresholded_A().detach().abs()
    n_cand = sum(int((S > t).sum()) == 3072 * 3071 for t in threshold_candidates())
    lines.append("%-36s %-13s device %10.3f ms, median of 7 (the whole search: %d candidates in one call, %d edges kept)"
                 % ("d 3072, A = 1.5 + .02 randn", "post_process", sorted(times)[3], len(threshold_candidates()), kept))
    lines.append("    device " + " ".join("%.3f" % t for t in times))
    print(lines[-2], flush=True)
    host = []
    for th in threshold_candidates()[:host_candidates]:
        def one():
            adj = (cond.soft_thresholded_A().data.clone().abs() > th).float().detach().cpu().numpy()
            return nx.is_directed_acyclic_graph(_digraph(adj))
        ms, acyclic = clocked(one)
        host.append(ms)
        lines.append("    host, candidate %.2f ALONE, timed once: %10.1f ms (acyclic: %s)" % (th, ms, acyclic))
        print(lines[-1], flush=True)
    lines.append("    the graph is complete (all d (d - 1) edges, as at that candidate) at the first %d candidates of the search; "
                 "the host arm was NOT timed beyond the candidates listed and nothing is extrapolated here" % n_cand)
    return sorted(times)[3], host


def kernels(lines, dev, reps):
    """gnf_dag_levels alone: device events around `reps` back-to-back calls on a bool matrix"""
    from gnf_hip import ops
    lines += ["", "ops.dag_levels alone (the pack and the peel kernel), ms per call from device events over %d back-to-back calls, "
              "bool input, G = 1:" % reps,
              "  empty graph = the pack kernel + ONE round of the peel;  a graph with n levels = the pack kernel + n + 1 rounds"]
    for d in (6, 63, 784, 3072, 4096):
        graphs = (("empty", torch.zeros(d, d)), ("density .1", perm_dag(d, .1, d)), ("chain", chain(d)))
        row = []
        for gname, A in graphs:
            M = (A.to(dev) > 0)
            for _ in range(3):
                ops.dag_levels(M)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                _, info = ops.dag_levels(M)
            b.record()
            torch.cuda.synchronize()
            row.append("%s %8.4f (%d levels)" % (gname, a.elapsed_time(b) / reps, int(info[1])))
        lines.append("  d %4d  " % d + "   ".join(row))
        print(lines[-1], flush=True)
    d = 3072
    S = (torch.rand(d, d, generator=torch.Generator().manual_seed(9)) * .999).to(dev)
    ths = [.1 + .05 * k for k in range(19)]
    for _ in range(3):
        ops.dag_levels(S, ths)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        ops.dag_levels(S, ths)
    b.record()
    torch.cuda.synchronize()
    lines.append("  d 3072  19 thresholds over one shared fp32 matrix (the post_process() call, threshold upload included) %8.4f"
                 % (a.elapsed_time(b) / reps))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dense-host-candidates", type=int, default=1)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dag_graph_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dag_graph.py needs an MI355X")
    dev = torch.device("cuda", 0)
    lines = []
    if args.kernels_only:
        kernels(lines, dev, args.reps)
        return
    lines += ["graph queries of a DAG conditioner: device (device_graph = True, gnf_hip.ops.dag_levels) against host "
              "(device_graph = False: copy to the CPU, networkx / Python walk)",
              "ms per call, host clock around a call that ends in a synchronise; %d alternating pairs, median" % args.pairs, ""]
    lost = []
    for name, make in cases():
        A0 = make()
        cond = conditioner(A0, dev)
        A0 = cond.A.detach().clone()
        d = A0.shape[0]
        for qname, wins in ab(lines, name, cond, A0, args.pairs, warm_host=d < 3072):
            if wins < args.pairs:
                lost.append((d, "%s %s: %d of %d pairs" % (name, qname, args.pairs - wins, args.pairs)))
    lines.append("")
    dense_search(lines, dev, args.dense_host_candidates)
    kernels(lines, dev, args.reps)
    lines += ["", "pairs lost by the device arm: " + ("; ".join(t for _, t in lost) if lost else "none")]
    if not lost:
        lines.append("DEVICE_GRAPH_DEFAULT = True by the adoption rule")
    else:
        lines.append("largest d with a lost pair: %d" % max(d for d, _ in lost))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
