"""A/B of the batch production of train_toy.py: ONE launch of gnf_toy_sample (gnf_hip.ops.toy_sample, Philox on the device) against
a vectorised host draw of the same arithmetic plus the host-to-device copy (train_toy.HostBatches: numpy uniforms, train_toy.
toy_reference in torch on the CPU -- no Python loop over the batch, unlike the reference's generator -- then `.to(device)`).

    python tools/bench_toy_data.py [--pairs 7] [--out profiles/toy_data_ab.txt]

One process, warm-up first, alternating pairs.  Three parts:
  1. a batch: both arms at B = 100 and B = 1000 for `8gaussians` and `8-MIX`; a sample is the host clock around `--reps` calls that
     end in a device synchronise, per call (the host arm is host work: device events would not see it);
  2. the entry point alone on a preallocated output, HIP events, per call;
  3. the driver: the epoch times train_toy.train reports for `--epochs` epochs (one batch of 100 and one test pass each; the
     first quarter, which holds the graph capture, is dropped), device batches against `-host_data`.
Reported against the 0.149 ms graphed step of configuration cfg1 (README.md).  Reported, not a gate: the device path is the
driver's default whatever this shows."""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "graphical-normalizing-flows_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

GRAPHED_STEP_MS = 0.149      # README.md: cfg1, the full step replayed from one hipGraph


def wall(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps   # microseconds per call


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def ab(variants, pairs, reps, timer, warmup=3):
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(pairs):
        for name, fn in variants:
            times[name].append(timer(fn, reps))
    return times


def median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_toy_data.py measures on the MI355X: no GPU here")
    import train_toy as T
    from gnf_hip import abi, ops
    dev = torch.device("cuda", 0)
    lines = ["Toy batches: one launch of gnf_toy_sample (csrc/gnf_toy_data.hip) vs a vectorised host draw of the same arithmetic + the "
             "host-to-device copy (train_toy.HostBatches)",
             "device: %s, torch %s; %d alternating pairs after warm-up; the graphed cfg1 step it feeds: %.3f ms (README.md)"
             % (torch.cuda.get_device_name(0), torch.__version__, args.pairs, GRAPHED_STEP_MS), "",
             "1. one batch, host clock around %d calls ending in a synchronise, microseconds per call" % args.reps]
    for name in ("8gaussians", "8-MIX"):
        for B in (100, 1000):
            device_arm, host_arm = T.DeviceBatches(name, dev), T.HostBatches(name, dev)
            variants = (("host draw + copy", lambda: host_arm(B)), ("one launch", lambda: device_arm(B)))
            times = ab(variants, args.pairs, args.reps, wall)
            lines.append("%s, B = %d" % (name, B))
            for vname, _ in variants:
                m = median(times[vname])
                lines.append("  %-18s %s   median %8.2f us = %.2f graphed steps"
                             % (vname, " ".join("%8.2f" % t for t in times[vname]), m, m / (GRAPHED_STEP_MS * 1e3)))
            wins = sum(k < c for k, c in zip(times["one launch"], times["host draw + copy"]))
            lines.append("  one launch faster than the host arm in %d of %d pairs" % (wins, args.pairs))
    lines += ["", "2. the entry point alone on a preallocated output, HIP events around %d calls, microseconds per call" % args.reps]
    fn = abi.load().gnf_toy_sample
    import ctypes
    stream = abi.stream()
    for name in ("8gaussians", "8-MIX"):
        blocks, scale = ops.toy_blocks(name)
        karr = (ctypes.c_int32 * len(blocks))(*blocks)
        sptr = None if scale is None else ctypes.c_void_p(scale.ctypes.data)
        variants = []
        keep = []
        for B in (100, 1000, 65536):
            x = torch.empty(B, 2 * len(blocks), device=dev)
            keep.append(x)
            a = (ctypes.cast(karr, ctypes.c_void_p), len(blocks), sptr, None, 12345, 0, x.data_ptr(), 2 * len(blocks), B, stream)
            variants.append(("B = %d" % B, (lambda a=a: abi.check(fn(*a), "gnf_toy_sample"))))
        times = ab(variants, args.pairs, args.reps, events)
        lines.append(name)
        for vname, _ in variants:
            lines.append("  %-18s %s   median %8.2f us" % (vname, " ".join("%8.2f" % t for t in times[vname]), median(times[vname])))
    lines += ["", "3. the driver: median epoch time of train_toy.train over the last three quarters of %d epochs (Coupling, the "
              "reference's defaults: one batch of 100, the test pass on 1000 rows, the log line), milliseconds" % args.epochs]
    for name in ("8gaussians", "8-MIX"):
        res = {"device batches": [], "-host_data": []}
        for _ in range(args.pairs):
            for arm, extra in (("-host_data", ["-host_data"]), ("device batches", [])):
                with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
                    run = T.train(T.parse(["-dataset", name, "-nb_epoch", str(args.epochs), "-plot_every", str(10 ** 9),
                                           "-folder", tmp + os.sep] + extra))
                res[arm].append(median(run.epoch_seconds[args.epochs // 4:]) * 1e3)
        lines.append(name)
        for arm in ("-host_data", "device batches"):
            lines.append("  %-18s %s   median %8.3f ms" % (arm, " ".join("%8.3f" % t for t in res[arm]), median(res[arm])))
        wins = sum(k < c for k, c in zip(res["device batches"], res["-host_data"]))
        lines.append("  device batches faster in %d of %d pairs" % (wins, args.pairs))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
