"""A/B of the batch preparation of train_image.py: ONE launch of gnf_image_prep (gnf_hip.ops.image_prep: gather, Philox noise,
logit, and the data term of the bits per pixel) against the torch chain it stands for on the same rows (the gather,
train_image.dequantise and train_image.compute_bpp: about twenty launches, noise from a torch generator).

    python tools/bench_image_prep.py [--pairs 7] [--out profiles/image_prep_ab.txt]

One process on a quiet device, HIP events, warm-up first, alternating pairs; a sample is the mean of `--reps` back-to-back
calls (one call is a few microseconds of kernel time: an event pair around a single call measures the events).  Shapes
(100, 3072) and (100, 784): a CIFAR-10 and an MNIST batch of the reference's b_size.  Then the kernel alone at (4096, 3072),
with and without the row term, as a fraction of the HBM rate: 1 byte read + 4 bytes written per element.  Reported, not a
gate: CIFAR-10 batches need the kernel (flip, keyed noise), MNIST keeps the torch chain by default whatever this shows."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "graphical-normalizing-flows_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM_PEAK = 8.0e12            # bytes / s, the data sheet's figure (DESIGN.md section 4 prices every HBM-bound kernel against it)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps            # microseconds per call


def ab(variants, pairs, reps, warmup=3):
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(pairs):
        for name, fn in variants:
            times[name].append(timed(fn, reps))
    return times


def median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_prep.py measures on the MI355X: no GPU here")
    import train_image as T
    from gnf_hip import ops
    dev = torch.device("cuda", 0)
    lines = ["Batch preparation in one launch (csrc/gnf_image_prep.hip, with bpp_term) vs the torch chain on the same rows "
             "(gather + train_image.dequantise + train_image.compute_bpp)",
             "device: %s, torch %s; HIP events, microseconds per call (mean of %d back-to-back calls per sample); %d alternating "
             "pairs after warm-up" % (torch.cuda.get_device_name(0), torch.__version__, args.reps, args.pairs), ""]
    g = torch.Generator().manual_seed(0)
    for (B, d), size, alpha in (((100, 3072), (3, 32, 32), .05), ((100, 784), (1, 28, 28), 1e-6)):
        u8 = torch.randint(0, 256, (10000, d), generator=g).to(torch.uint8).to(dev)
        rows = torch.randperm(10000, generator=g)[:B].to(dev)
        rows32 = rows.to(torch.int32)
        ll = torch.randn(B, device=dev) * 50 - 1500
        noise = torch.Generator(device=dev).manual_seed(1)
        calls = [0]

        def kernel():
            calls[0] += 1
            x, term = ops.image_prep(u8, rows32, None, None, 12345, calls[0], alpha, size, True)
            return T.bpp_from_term(ll, term, d, alpha)

        def chain():
            x = T.dequantise(u8[rows], alpha, noise)
            return T.compute_bpp(ll, x, alpha)
        variants = (("torch chain", chain), ("one launch", kernel))
        times = ab(variants, args.pairs, args.reps)
        lines.append("(B, d) = (%d, %d), alpha = %g, rows gathered from a [10000, %d] data set" % (B, d, alpha, d))
        for name, _ in variants:
            lines.append("%-14s %s   median %.2f" % (name, " ".join("%8.2f" % t for t in times[name]), median(times[name])))
        wins = sum(k < c for k, c in zip(times["one launch"], times["torch chain"]))
        lines.append("one launch faster than the torch chain in %d of %d pairs" % (wins, args.pairs))
        lines.append("")
    # the kernel alone: the entry point itself on preallocated outputs (at 20 us a call, ops.image_prep's two allocations and
    # its argument handling are of the order of the kernel)
    from gnf_hip import abi
    fn = abi.load().gnf_image_prep
    B, d, size = 4096, 3072, (3, 32, 32)
    u8 = torch.randint(0, 256, (B, d), generator=g).to(torch.uint8).to(dev)
    x, term = torch.empty(B, d, device=dev), torch.empty(B, device=dev)
    stream = abi.stream()

    def raw(mode, want_term):
        a = (u8.data_ptr(), B, None, mode, None, *size, None, 12345, 0, .05, x.data_ptr(), term.data_ptr() if want_term else None,
             B, stream)
        return lambda: abi.check(fn(*a), "gnf_image_prep")
    variants = (("with bpp_term", raw(0, True)), ("x only", raw(0, False)), ("x only, flip coin", raw(2, False)),
                ("through ops", lambda: ops.image_prep(u8, None, None, None, 12345, 0, .05, size, True)))
    times = ab(variants, args.pairs, args.reps)
    nbytes = B * d * 5
    lines.append("the kernel alone at (B, d) = (%d, %d), the entry point on preallocated outputs: %.1f MB = 1 B read + 4 B written "
                 "per element" % (B, d, nbytes / 1e6))
    for name, _ in variants:
        m = median(times[name])
        lines.append("%-18s %s   median %.2f us = %.2f TB/s = %.2f of %.1f TB/s"
                     % (name, " ".join("%8.2f" % t for t in times[name]), m, nbytes / m / 1e6, nbytes / (m * 1e-6) / HBM_PEAK,
                        HBM_PEAK / 1e12))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
