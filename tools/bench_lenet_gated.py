"""A/B of the DAG gate fused into the LeNet front of CIFAR10CNN (`gated_front`, gnf_hip.ops.DagLenetFrontFn: the masked
copies are built in LDS) against the composed path (DagGateFn + LenetConvFn: the copies and their cotangent go through HBM).

    python tools/bench_lenet_gated.py [--pairs 7] [--out profiles/lenet_gated_ab.txt]

One process on a quiet device, HIP events, warm-up first, alternating pairs.  A DAG conditioner (Gumbel gate from Philox,
trainable A) over CIFAR10CNN at (3,32,32,5) and (1,32,32,3), B = 8: forward under no_grad, and forward + backward with
gradients for A and the ten network parameters; then one eager training step of the one-scale Affine CIFAR-10 flow at
B = 8.  Each variant also reports torch.cuda.max_memory_allocated above the level before the call.  The rule for the default
of `gated_front` is the one of the previous adoptions: on only if forward + backward wins every pair of both geometries."""
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


def ab(variants, pairs, warmup=3):
    """{name: [ms]} over alternating rounds, {name: peak bytes}"""
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(pairs):
        for name, fn in variants:
            times[name].append(timed(fn))
    return times, {name: peak_of(fn) for name, fn in variants}


def report(lines, variants, times, peaks):
    for name, _ in variants:
        ts = times[name]
        lines.append("%-24s %s   median %.3f   peak %.1f MB" % (name, " ".join("%7.3f" % t for t in ts),
                                                               sorted(ts)[len(ts) // 2], peaks[name] / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from models import AffineNormalizer, DAGConditioner
    from models.MLP import CIFAR10CNN
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow
    lines = ["DAG gate fused into the CIFAR10CNN front (gated_front = True, csrc/gnf_lenetcnn.hip lenet_gated_*_k) vs the "
             "composed path (gated_front = False: gnf_dag_gate_* + gnf_lenet_conv_*)",
             "device: %s, torch %s; HIP events, ms; %d alternating pairs after warm-up; B = %d; peak = "
             "torch.cuda.max_memory_allocated above the level before the call" %
             (torch.cuda.get_device_name(0), torch.__version__, args.pairs, B)]
    all_win = True
    for size_img, k, fc_l in CASES:
        d = size_img[0] * size_img[1] * size_img[2]
        torch.manual_seed(0)
        net = CIFAR10CNN(out_d=2, fc_l=list(fc_l), size_img=list(size_img), k_size=k)
        cond = DAGConditioner(d, net, 2).cuda()
        x = torch.randn(B, d, device="cuda")
        g = torch.randn(B, d, 2, device="cuda")
        params = list(cond.parameters())

        def fwd(gated):
            net.gated_front = gated
            with torch.no_grad():
                cond(x)

        def fwd_bwd(gated):
            net.gated_front = gated
            torch.autograd.grad((cond(x) * g).sum(), params)

        variants = (("composed fwd", lambda: fwd(False)), ("gated fwd", lambda: fwd(True)),
                    ("composed fwd+bwd", lambda: fwd_bwd(False)), ("gated fwd+bwd", lambda: fwd_bwd(True)))
        times, peaks = ab(variants, args.pairs)
        lines += ["", "conditioner over geometry (C,H,W,k) = (%d,%d,%d,%d): d = %d, %d masked copies, one copy set = %.1f MB" %
                  (*size_img, k, d, B * d, B * d * d * 4 / 1e6)]
        report(lines, variants, times, peaks)
        for a, b in (("gated fwd", "composed fwd"), ("gated fwd+bwd", "composed fwd+bwd")):
            wins = sum(f < t for f, t in zip(times[a], times[b]))
            lines.append("%s faster than %s in %d of %d pairs" % (a, b, wins, args.pairs))
            if a == "gated fwd+bwd":
                all_win = all_win and wins == args.pairs
        del cond, net, x, g, params
    # one eager training step of the one-scale Affine flow
    torch.manual_seed(0)
    flow = buildCIFAR10NormalizingFlow([1], AffineNormalizer, {}).cuda()
    net = flow.steps[0].conditioner.embedding_net
    opt = torch.optim.Adam(flow.parameters(), lr=1e-3)
    xb = torch.randn(B, 3072, device="cuda")

    def step(gated):
        net.gated_front = gated
        opt.zero_grad(set_to_none=True)
        z, ld = flow(xb)
        flow.loss(z, ld).backward()
        opt.step()
    variants = (("composed step", lambda: step(False)), ("gated step", lambda: step(True)))
    times, peaks = ab(variants, args.pairs, warmup=2)
    lines += ["", "one eager training step (forward, loss, backward, torch Adam) of buildCIFAR10NormalizingFlow([1], "
              "AffineNormalizer, {}) at B = %d:" % B]
    report(lines, variants, times, peaks)
    wins = sum(f < t for f, t in zip(times["gated step"], times["composed step"]))
    lines.append("gated step faster than composed step in %d of %d pairs" % (wins, args.pairs))
    lines += ["", "rule: gated_front defaults to True only if gated fwd+bwd is faster in every pair of both geometries: %s" %
              ("met" if all_win else "NOT met")]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
