"""A/B of the training form of the row-subset LeNet front of CIFAR10CNN (`rows_train_front`, gnf_hip.ops.lenet_rows_train: the
masked copies x[b] * P[i] of a FROZEN deterministic DAG gate are built in LDS, forward and backward, and dL/dx is summed over
the rows in registers) against the composed path (`rows_train_front = False`: DagGateFn writes the B*d copies, LenetConvFn
keeps them and writes their cotangent, the gate backward reads it).

    python tools/bench_lenet_rows_train.py [--pairs 7] [--out profiles/lenet_rows_train_ab.txt]

One process on a quiet device, HIP events, warm-up first, alternating pairs, B = 8, A frozen to a fixed 0/1 DAG.  A DAG
conditioner over CIFAR10CNN at (3,32,32,5) and (1,32,32,3): (a) forward + backward with x as data, (b) the same with
x.requires_grad.  Then (c) one full training step (forward, loss, backward) of the one-scale Affine CIFAR-10 flow after
freezing.  Each variant also reports torch.cuda.max_memory_allocated above the level before the call.  The rule for the
default of `rows_train_front` is the one of the previous adoptions: on only if (a) AND (b) win every pair of both
geometries."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "graphical-normalizing-flows_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_lenet_rows import B, CASES, ab, report, sparse_dag  # noqa: E402


def freeze(cond, A):
    cond.stoch_gate = cond.noise_gate = cond.s_thresh = False
    cond.h_thresh = 0.
    with torch.no_grad():
        cond.A.copy_(A.to(cond.A.device))
    cond.A.requires_grad = False
    cond.invalidate_caches()
    cond.is_invertible = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from models import AffineNormalizer, DAGConditioner
    from models.MLP import CIFAR10CNN
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow
    lines = ["Training form of the row-subset CIFAR10CNN front (rows_train_front = True, csrc/gnf_lenetcnn.hip lenet_rows_fwd_arg_k "
             "+ lenet_rows_bwd_k) vs the composed path (rows_train_front = False: DagGateFn + LenetConvFn, e and its cotangent "
             "in memory)",
             "device: %s, torch %s; HIP events, ms; %d alternating pairs after warm-up; B = %d; A frozen to a 0/1 DAG; peak = "
             "torch.cuda.max_memory_allocated above the level before the call" %
             (torch.cuda.get_device_name(0), torch.__version__, args.pairs, B)]
    all_win, lost = True, []
    for size_img, k, fc_l in CASES:
        d = size_img[0] * size_img[1] * size_img[2]
        torch.manual_seed(0)
        net = CIFAR10CNN(out_d=2, fc_l=list(fc_l), size_img=list(size_img), k_size=k)
        cond = DAGConditioner(d, net, 2).cuda()
        freeze(cond, sparse_dag(d))
        x = torch.randn(B, d, device="cuda")
        cot = torch.randn(B, d, 2, device="cuda")

        def fwd_bwd(on, x_grad):
            net.rows_train_front = on
            cond.zero_grad(set_to_none=True)
            (cond(x.clone().requires_grad_(x_grad)) * cot).sum().backward()

        lines += ["", "conditioner forward + backward, geometry (C,H,W,k) = (%d,%d,%d,%d): d = %d, %d masked copies, the "
                  "product = %.1f MB" % (*size_img, k, d, B * d, B * d * d * 4 / 1e6)]
        for tag, x_grad in (("(a) x data", False), ("(b) x.requires_grad", True)):
            variants = (("composed %s" % tag, lambda: fwd_bwd(False, x_grad)), ("rows %s" % tag, lambda: fwd_bwd(True, x_grad)))
            times, peaks = ab(variants, args.pairs)
            report(lines, variants, times, peaks)
            wins = sum(f < t for f, t in zip(times[variants[1][0]], times[variants[0][0]]))
            lines.append("rows faster than composed, %s, in %d of %d pairs" % (tag, wins, args.pairs))
            if wins != args.pairs:
                all_win = False
                lost.append("%s at d = %d: %d of %d pairs lost" % (tag, d, args.pairs - wins, args.pairs))
        del cond, net, x, cot
    # (c) one full training step of the one-scale Affine flow over a fixed sparse DAG
    torch.manual_seed(0)
    flow = buildCIFAR10NormalizingFlow([1], AffineNormalizer, {}).cuda()
    cond = flow.steps[0].conditioner
    freeze(cond, sparse_dag(3072))
    x = torch.randn(B, 3072, device="cuda")

    def step(on):
        cond.embedding_net.rows_train_front = on
        flow.zero_grad(set_to_none=True)
        z, ld = flow(x)
        flow.loss(z, ld).backward()

    variants = (("composed (c) step", lambda: step(False)), ("rows (c) step", lambda: step(True)))
    times, peaks = ab(variants, args.pairs)
    lines += ["", "(c) forward + loss + backward of buildCIFAR10NormalizingFlow([1], AffineNormalizer, {}) at B = %d, A frozen to "
              "a 0/1 DAG (%d edges):" % (B, int(cond.A.sum().item()))]
    report(lines, variants, times, peaks)
    wins = sum(f < t for f, t in zip(times["rows (c) step"], times["composed (c) step"]))
    lines.append("rows (c) step faster than composed (c) step in %d of %d pairs" % (wins, args.pairs))
    lines += ["", "rule: rows_train_front defaults to True only if (a) and (b) are faster in every pair of both geometries: %s" %
              ("met" if all_win else "NOT met (%s)" % "; ".join(lost)),
              "decision: ROWS_TRAIN_FRONT_DEFAULT = %s (models/MLP.py)%s" %
              (all_win, "" if all_win else "; rows_train_front stays opt-in, for the batches whose copies do not fit")]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
