"""A/B of the convolutional front of CIFAR10CNN: the fused LDS-resident kernels (gnf_hip.ops.lenet_conv) against the torch
chain pool(relu(conv2(pool(relu(conv1))))) that `fused_front = False` selects (MIOpen convolutions + elementwise kernels).

    python tools/bench_lenet_front.py [--pairs 7] [--out profiles/lenet_front_ab.txt]

One process, HIP events, warm-up first, alternating pairs.  For (3,32,32,5) at n = 8 * 3072 and (1,32,32,3) at
n = 8 * 1024 (a batch of 8 through a DAG conditioner: one masked copy per variable): forward, and forward + backward with
gradients for the input and the four parameters; the fused backward both with the second pool's decisions saved by the
forward and with conv2 recomputed (GNF_LENET_SAVE_ARGMAX=0).  The first call of the torch path (MIOpen's find / kernel
build) is reported separately and is in no pair.  Also one eager training step of the one-scale Affine CIFAR-10 flow at
B = 8, as a starting number for later work."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "graphical-normalizing-flows_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_FP32 = 157.3e12        # vector fp32, MI355X (spec)
PEAK_HBM = 6.29e12          # measured float4 copy

CASES = (((3, 32, 32), 5, (400, 128, 84), 8 * 3072),
         ((1, 32, 32), 3, (576, 128, 32), 8 * 1024))


def counts(size_img, k):
    """(conv1 MACs, conv2 MACs, MACs of the four gradients over the sparse pooled cotangents, bytes in, bytes out) per image"""
    c, h, _ = size_img
    h1 = h - k + 1
    p1 = h1 // 2
    h2 = p1 - k + 1
    p2 = h2 // 2
    conv1 = (2 * p1) ** 2 * 6 * c * k * k
    conv2 = (2 * p2) ** 2 * 16 * 6 * k * k
    feat = 16 * p2 * p2
    bwd = conv1 + feat * 6 * k * k + p1 * p1 * 16 * 6 * k * k + 6 * p1 * p1 * c * k * k + h * h * 6 * c * k * k
    return conv1, conv2, bwd, c * h * h * 4, feat * 4


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gnf_hip import ops
    from models.MLP import CIFAR10CNN
    lines = ["CIFAR10CNN convolutional front: fused kernels (csrc/gnf_lenetcnn.hip) vs the torch chain (fused_front = False)",
             "device: %s, torch %s; HIP events, ms; %d alternating pairs after warm-up" %
             (torch.cuda.get_device_name(0), torch.__version__, args.pairs)]
    for size_img, k, fc_l, n in CASES:
        torch.manual_seed(0)
        net = CIFAR10CNN(out_d=2, fc_l=list(fc_l), size_img=list(size_img), k_size=k).cuda()
        P = [net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv2.bias]
        x = torch.randn(n, size_img[0] * size_img[1] * size_img[2], device="cuda", requires_grad=True)

        def torch_front():
            f = x.view(-1, *size_img)
            for conv in (net.conv1, net.conv2):
                f = net.pool(F.relu(conv(f)))
            return f.reshape(n, -1)

        def fused_front():
            return ops.lenet_conv(x, *P, size_img, k)

        g = torch.randn_like(fused_front().detach())

        def fwd(front):
            with torch.no_grad():
                front()

        def fwd_bwd(front, save="1"):
            os.environ["GNF_LENET_SAVE_ARGMAX"] = save
            torch.autograd.grad((front() * g).sum(), [x] + P)
            os.environ["GNF_LENET_SAVE_ARGMAX"] = "1"

        t0 = time.perf_counter()
        fwd_bwd(torch_front)
        torch.cuda.synchronize()
        first = (time.perf_counter() - t0) * 1e3
        variants = (("torch fwd", lambda: fwd(torch_front)), ("fused fwd", lambda: fwd(fused_front)),
                    ("torch fwd+bwd", lambda: fwd_bwd(torch_front)), ("fused fwd+bwd", lambda: fwd_bwd(fused_front)),
                    ("fused fwd+bwd, conv2 recomputed", lambda: fwd_bwd(fused_front, "0")))
        for _ in range(3):
            for _, fn in variants:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(args.pairs):
            for name, fn in variants:
                times[name].append(timed(fn))
        conv1, conv2, macs_b, b_in, b_out = counts(size_img, k)
        macs_f = conv1 + conv2
        lines += ["", "geometry (C,H,W,k) = (%d,%d,%d,%d), n = %d images" % (*size_img, k, n),
                  "per image: forward %d FMA, fused backward %d FMA (+ the conv1 recompute, %d), %d B read, %d B written "
                  "forward; backward reads the image and the cotangent again and writes %d B" %
                  (macs_f, macs_b, conv1, b_in, b_out, b_in),
                  "first call of the torch path (fwd+bwd, MIOpen find / kernel build; in no pair): %.1f ms" % first]
        for name, _ in variants:
            ts = times[name]
            lines.append("%-34s %s   median %.3f" % (name, " ".join("%7.3f" % t for t in ts), sorted(ts)[len(ts) // 2]))
        tf = sorted(times["fused fwd"])[len(times["fused fwd"]) // 2] * 1e-3
        tb = sorted(times["fused fwd+bwd"])[len(times["fused fwd+bwd"]) // 2] * 1e-3
        lines.append("fused fwd: %.1f %% of the fp32 vector peak (%.1f TFLOP/s), %.1f %% of the HBM copy rate" %
                     (100 * 2 * macs_f * n / tf / PEAK_FP32, 2 * macs_f * n / tf / 1e12,
                      100 * (b_in + b_out) * n / tf / PEAK_HBM))
        lines.append("fused fwd+bwd: %.1f %% of the fp32 vector peak over the FMAs counted above" %
                     (100 * 2 * (macs_f + conv1 + macs_b) * n / tb / PEAK_FP32))
        for a, b in (("fused fwd", "torch fwd"), ("fused fwd+bwd", "torch fwd+bwd")):
            wins = sum(f < t for f, t in zip(times[a], times[b]))
            lines.append("%s faster than %s in %d of %d pairs" % (a, b, wins, args.pairs))
        del net, x
    # one eager training step of the one-scale Affine flow, B = 8
    from models import AffineNormalizer
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow
    torch.manual_seed(0)
    flow = buildCIFAR10NormalizingFlow([1], AffineNormalizer, {}).cuda()
    opt = torch.optim.Adam(flow.parameters(), lr=1e-3)
    xb = torch.randn(8, 3072, device="cuda")

    def step():
        opt.zero_grad(set_to_none=True)
        z, ld = flow(xb)
        loss = flow.loss(z, ld)
        loss.backward()
        opt.step()
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    ts = [timed(step) for _ in range(5)]
    lines += ["", "one eager training step (forward, loss, backward, torch Adam) of buildCIFAR10NormalizingFlow([1], "
              "AffineNormalizer, {}) at B = 8 (24 576 masked images):",
              " ".join("%.2f" % t for t in ts) + "   median %.2f ms" % sorted(ts)[2]]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
