"""A/B of the epoch loop of train_uci.py: batches cut on the host (a slice of torch.randperm copied over, `trn[rows]`, one
replayed step per batch -- the loop as it was before -device_batches, restated here) against -device_batches (one
gnf_tab_batch launch per batch, dp.DeviceBatches) with -steps_per_replay K = 1, 4 and 16 (train_uci.train_epoch).

    python tools/bench_uci_epoch.py [--pairs 5] [--epochs 3] [--out profiles/uci_device_batches_ab.txt]
    python tools/bench_uci_epoch.py --pkg OTHER_TREE/graphical-normalizing-flows_amd --arms host     # another checkout's loop

One process; every arm owns a model and its optimiser state, runs two warm-up epochs (they capture every variant: the group,
the single full batch, the tail), then the arms alternate.  A sample is the host clock around `--epochs` epochs of training
steps, ending in a device synchronise, in seconds per epoch.  Configurations on synthetic data:
  power-coupling   POWER (d = 6, 20 000 rows), Affine + Coupling, emb_net 100 100 100 2, B = 100: 200 steps per epoch
  made-784         d = 784 (5 000 rows), Affine + MADE 1024^3, B = 100: 50 steps per epoch (cfg3's shape)
  power-mono-dag   POWER, Monotonic + DAG, B = 2500: 8 steps per epoch; the stochastic gate and the node-count jitter refuse
                   every replay, so all arms run the same eager steps and no gain is expected
Then gnf_tab_batch alone against torch.index_select at [50 000, 63] (and d = 64, the float4 form) from a table of 200 000
rows: HIP events around the replay of a hipGraph of `--reps` calls (no host work inside), bytes = 8 B d + 4 B over the kernel time.  Reported, not a gate: the options stay
opt-in whatever this shows."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    "power-coupling": (["-dataset", "power", "-conditioner", "Coupling", "-normalizer", "affine", "-emb_net", "100", "100",
                        "100", "2", "-b_size", "100"], 6, 20000),
    "made-784": (["-dataset", "digits", "-conditioner", "Autoregressive", "-normalizer", "affine", "-emb_net", "1024", "1024",
                  "1024", "2", "-b_size", "100"], 784, 5000),
    "power-mono-dag": (["-dataset", "power", "-conditioner", "DAG", "-normalizer", "monotonic", "-emb_net", "60", "60", "60",
                        "30", "-int_net", "100", "100", "100", "-nb_steps", "20", "-b_size", "2500", "-l1", "0."], 6, 20000),
}
ARMS = {"host": None, "device K=1": 1, "device K=4": 4, "device K=16": 16}


def median(ts):
    return sorted(ts)[len(ts) // 2]


class Arm:
    def __init__(self, T, dp, torch, argv, d, rows, K):
        extra = [] if K is None else ["-device_batches", "-steps_per_replay", str(K)]
        self.T, self.dp, self.torch = T, dp, torch
        self.args = T.parse(argv + extra)
        self.trn = torch.randn(rows, d, generator=torch.Generator().manual_seed(0)).cuda()
        torch.manual_seed(0)
        self.model, _, self.norm_t = T.build(self.args, d)
        self.model.cuda()
        dp.seed_gates(self.model, 0)
        self.state = dp.FlatState(self.model)
        self.gen = torch.Generator().manual_seed(1234)
        self.src = None if K is None else dp.DeviceBatches(self.trn, self.args.b_size, seed=0)
        self.epoch = 0

    def run_epoch(self):
        T, dp, torch, args = self.T, self.dp, self.torch, self.args
        if self.src is not None:
            T.train_epoch(args, self.model, self.state, self.norm_t, self.trn, self.src, self.epoch, 0, 1, self.gen)
        else:                                   # the statements of the loop before -device_batches
            ll_tot, n = torch.zeros((), device=self.trn.device), 0
            for rows in T.shard_batches(self.trn.shape[0], args.b_size, 0, 1, self.gen):
                if self.norm_t is T.MonotonicNormalizer:
                    k = args.nb_steps + int(torch.randint(0, 10, [1], generator=self.gen))
                    for nrm in self.model.getNormalizers():
                        nrm.nb_steps = k
                loss = dp.train_step(self.model, self.state, self.trn[rows.to(self.trn.device)], lr=args.learning_rate,
                                     weight_decay=args.weight_decay)
                ll_tot += loss.detach()
                n += 1
        self.epoch += 1

    def sample(self, epochs):
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(epochs):
            self.run_epoch()
        self.torch.cuda.synchronize()
        return (time.perf_counter() - t0) / epochs


def kernel_part(torch, ops, abi, pairs, reps):
    lines = ["", "gnf_tab_batch alone against torch.index_select, B = 50 000 rows of a [200 000, d] table through a permutation; "
             "HIP events around one replay of a hipGraph of %d calls, microseconds per call; bytes = 8 B d + 4 B" % reps]
    B, n = 50000, 200000
    for d in (63, 64):
        X = torch.randn(n, d, device="cuda")
        perm = (torch.sort(ops.shuffle_keys(1, 0, n, device="cuda")).values & 0xffffffff).to(torch.int32)
        rows, out, out2 = perm[:B].long(), torch.empty(B, d, device="cuda"), torch.empty(B, d, device="cuda")
        variants = (("index_select", lambda: torch.index_select(X, 0, rows, out=out2)),
                    ("gnf_tab_batch", lambda: ops.tab_batch(X, perm, 0, 1, B, out=out)))
        for _, fn in variants:
            for _ in range(3):
                fn()
        assert torch.equal(out, out2)
        graphs = {}
        for name, fn in variants:               # `reps` calls per graph: the replay holds the kernels and no host work
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(reps):
                    fn()
            graphs[name].replay()
        times = {name: [] for name, _ in variants}
        for _ in range(pairs):
            for name, _ in variants:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                graphs[name].replay()
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b) * 1e3 / reps)
        lines.append("d = %d" % d)
        for name, _ in variants:
            m = median(times[name])
            lines.append("  %-14s %s   median %8.2f us = %.2f TB/s" % (name, " ".join("%8.2f" % t for t in times[name]), m,
                                                                      (8 * B * d + 4 * B) / (m * 1e-6) / 1e12))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", nargs="*", default=list(CONFIGS), choices=list(CONFIGS),
                    help="none: only the kernel part")
    ap.add_argument("--arms", nargs="+", default=list(ARMS), choices=list(ARMS))
    ap.add_argument("--pkg", default=os.path.join(ROOT, "graphical-normalizing-flows_amd"),
                    help="the package directory to import train_uci and gnf_hip from (another checkout: only the host arm)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_uci_epoch.py measures on the MI355X: no GPU here")
    import train_uci as T
    from gnf_hip import abi, dp, ops
    lines = ["Epoch loop of train_uci.py: host batches vs -device_batches with -steps_per_replay K (tools/bench_uci_epoch.py)",
             "device: %s, torch %s; package %s" % (torch.cuda.get_device_name(0), torch.__version__,
                                                   os.path.relpath(os.path.abspath(args.pkg), ROOT)),
             "%d alternating rounds after two warm-up epochs per arm; a sample: host clock around %d epochs of training steps "
             "ending in a synchronise, milliseconds per epoch" % (args.pairs, args.epochs)]
    for name in args.configs:
        argv, d, rows = CONFIGS[name]
        arms = [(a, Arm(T, dp, torch, argv, d, rows, ARMS[a])) for a in args.arms]
        for _, arm in arms:
            arm.sample(2)
        times = {a: [] for a, _ in arms}
        for _ in range(args.pairs):
            for a, arm in arms:
                times[a].append(arm.sample(args.epochs) * 1e3)
        steps = len(dp.batch_slices(rows, arms[0][1].args.b_size, 0, 1)) if hasattr(dp, "batch_slices") else -(-rows // arms[0][1].args.b_size)
        lines += ["", "%s: %d rows, d = %d, B = %d, %d steps per epoch" % (name, rows, d, arms[0][1].args.b_size, steps)]
        for a, arm in arms:
            m = median(times[a])
            gs = getattr(arm.state, "_graphed", None)
            lines.append("  %-12s %s   median %9.3f  (min %9.3f max %9.3f) ms = %.4f ms per step; graphs captured: %s"
                         % (a, " ".join("%9.3f" % t for t in times[a]), m, min(times[a]), max(times[a]), m / steps,
                            "none" if gs is None else gs.captures))
        if "host" in times:
            for a in times:
                if a != "host":
                    wins = sum(x < h for x, h in zip(times[a], times["host"]))
                    lines.append("  %s faster than host in %d of %d rounds, median ratio host / arm %.3f"
                                 % (a, wins, args.pairs, median(times["host"]) / median(times[a])))
        del arms
        torch.cuda.empty_cache()
    if hasattr(ops, "tab_batch"):
        lines += kernel_part(torch, ops, abi, max(args.pairs, 5), args.reps)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
