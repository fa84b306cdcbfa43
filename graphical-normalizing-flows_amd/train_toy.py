"""Toy density-estimation driver on the MI355X flow path: the 2-D problems and their 4 / 8 / 14 / 16-column composites of
the reference's ToyExperiments.py (:22-155 run, :160-190 arguments and data-set list), among them `8-MIX`, the paper's
structure-discovery setting (sixteen columns made of eight independent 2-D problems).

    python train_toy.py -dataset 8gaussians -folder runs/
    python train_toy.py -dataset 8-MIX -cond_type DAG -emb_net 100 100 100 10 -nb_flow 1 -l1 .5 -folder runs/

What differs, on purpose (DESIGN.md section 1 lists each):
  * Every training batch is drawn on the device by ONE HIP launch (gnf_hip.ops.toy_sample, csrc/gnf_toy_data.hip) keyed by
    Philox -- key dp.gate_seed(rank, TOY_KEY + seed), offset = the call number -- where the reference draws it on the host
    (lib/toy_data.py, a Python loop over the batch for the Gaussian mixtures) and copies it over.  `-host_data` feeds the same
    arithmetic (toy_reference below) from numpy uniforms instead: the host arm of tools/bench_toy_data.py.
  * The loops and constants the reference hard-codes (:22-57) are options with its values as defaults: -cond_type, -nb_flow,
    -emb_net, -batch_size, -nb_samp, -seed, -plot_every.  `norm_type` stays "Affine" as there.
  * The step is dp.train_step: Coupling / Autoregressive runs are replayed from one hipGraph (GraphedStep); a DAG run keeps
    its stochastic gate and stays eager.
  * No plotting library: for 2-D problems the density on the reference's 100 x 100 grid over [-4.5, 4.5]^2
    (lib/visualize_flow.py:9-10, :45-55) is written as a binary PGM plus the two marginal sums as text; composites (d > 2),
    where the reference's plot cannot run, get no plot.  DAG runs also write the soft-thresholded adjacency of every step.
  * Not reproduced: the `pinwheel` job the reference runs at import (:174-179), `set_detect_anomaly`, the dead `and False`
    block (:103-123), and the `model.compute_ll` call on a NaN loss (a method its flows do not have): a non-finite loss stops
    the run with the epoch and the value in the message.
  * `conditionnal8gaussians` is not offered (no context here); it is not in the reference's `datasets` list either.

Checkpoints: `<folder><dataset>/<save_name>model.pt` and `...ADAM.pt`, save_name = "Affine" + str(emb_net) + str(nb_flow) as
in the reference (:39, :154-155), in the formats train_uci.py writes (state_dict with the reference's keys, torch.optim.Adam's
state): either side can resume the other's run."""
import argparse
import os
import sys
import time
from collections import namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from models import (buildFCNormalizingFlow, DAGConditioner, CouplingConditioner, AutoregressiveConditioner,  # noqa: E402
                    AffineNormalizer)
from gnf_hip import dp, ops  # noqa: E402

COND = {"DAG": DAGConditioner, "Coupling": CouplingConditioner, "Autoregressive": AutoregressiveConditioner}
# the reference's list, in its order (:160-162)
DATASETS = ["2igaussians", "2gaussians", "8gaussians", "swissroll", "moons", "pinwheel", "cos", "2spirals", "checkerboard",
            "line", "line-noisy", "circles", "joint_gaussian", "2spirals-8gaussians", "4-2spirals-8gaussians",
            "8-2spirals-8gaussians", "8-MIX", "7-MIX", "4gaussians"]
NORM_TYPE = "Affine"
TOY_KEY = 1 << 21           # dp.gate_seed(rank, TOY_KEY + seed): the Philox key of the batches (conditioners count from 0,
                            # the image preparation uses 1 << 20)
N_TEST = 1000               # reference :33
LOW, HIGH, NPTS = -4.5, 4.5, 100        # lib/visualize_flow.py:9-10, ToyExperiments.py:139

ToyRun = namedtuple("ToyRun", "model state train_losses test_losses epoch_seconds")


# ----------------------------------------------------------------------------- the sampler's arithmetic in torch
def _normal_pair(ua, ub):
    r, th = torch.sqrt(-2. * torch.log(ua)), 6.283185307179586 * ub
    return r * torch.cos(th), r * torch.sin(th)


def _klass(u, K):
    """number of thresholds j / K (rounded to fp32, as the kernel's constants are) that u reaches: comparisons only, so an
    fp32 and an fp64 evaluation of the same uniforms agree on every class"""
    k = torch.zeros(u.shape, dtype=torch.long, device=u.device)
    for j in range(1, K):
        k = k + (u >= float(np.float32(j / K))).long()
    return k


_CENTRES = {0: ((2., 0.), (-2., 0.)), 1: ((2., -2.), (-2., 2.)), 2: ((2., -2.), (-2., 2.), (2., 2.), (-2., -2.)),
            3: tuple((4. * a, 4. * b) for a, b in ((1, 0), (-1, 0), (0, 1), (0, -1), (1. / np.sqrt(2), 1. / np.sqrt(2)),
                                                   (1. / np.sqrt(2), -1. / np.sqrt(2)), (-1. / np.sqrt(2), 1. / np.sqrt(2)),
                                                   (-1. / np.sqrt(2), -1. / np.sqrt(2))))}


def _toy_block(kind, u):
    """the two columns of one base problem from its uniforms u [B, 8] (already in the evaluation dtype): the table at the head
    of csrc/gnf_toy_data.hip, operation by operation"""
    u0, u1, u2, u3, u4, u5 = (u[:, k] for k in range(6))
    if kind <= 3:
        n0, n1 = _normal_pair(u0, u1)
        c = torch.tensor(_CENTRES[kind], dtype=u.dtype, device=u.device)[_klass(u2, len(_CENTRES[kind]))]
        std = .5 if kind == 3 else .75
        a, b = n0 * std + c[:, 0], n1 * std + c[:, 1]
        return (a / 1.414, b / 1.414) if kind == 3 else (a, b)
    if kind == 4:
        t = (1. + 2. * u0) * 4.71238898038469
        n0, n1 = _normal_pair(u1, u2)
        return (t * torch.cos(t) + n0) / 5., (t * torch.sin(t) + n1) / 5.
    if kind == 5:
        f = torch.where(u0 >= .5, .5, 1.).to(u.dtype)
        a = 6.283185307179586 * u1
        n0, n1 = _normal_pair(u2, u3)
        return (f * torch.cos(a) + .08 * n0) * 3., (f * torch.sin(a) + .08 * n1) * 3.
    if kind == 6:
        a = 3.141592653589793 * u1
        c, s = torch.cos(a), torch.sin(a)
        inner = u0 >= .5
        n0, n1 = _normal_pair(u2, u3)
        mx, my = torch.where(inner, 1. - c, c), torch.where(inner, (1. - s) - .5, s)
        return (mx + .1 * n0) * 2. - 1., (my + .1 * n1) * 2. - .2
    if kind == 7:
        n0, n1 = _normal_pair(u0, u1)
        f0, f1 = n0 * .3 + 1., n1 * .1
        a = _klass(u2, 5).to(u.dtype) * 1.2566370614359172 + .25 * torch.exp(f0)
        c, s = torch.cos(a), torch.sin(a)
        return 2. * (f0 * c + f1 * s), 2. * (f1 * c - f0 * s)
    if kind == 8:
        m = torch.sqrt(u0) * 9.42477796076938
        sg = torch.where(u3 >= .5, -1., 1.).to(u.dtype)
        dx, dy = -torch.cos(m) * m + u1 * .5, torch.sin(m) * m + u2 * .5
        n0, n1 = _normal_pair(u4, u5)
        return sg * dx / 3. + .1 * n0, sg * dy / 3. + .1 * n1
    if kind == 9:
        x1 = u0 * 4. - 2.
        par = (((u0 >= .25) & (u0 < .5)) | (u0 >= .75)).to(u.dtype)
        coin = torch.where(u2 >= .5, 2., 0.).to(u.dtype)
        return x1 * 2., ((u1 - coin) + par) * 2.
    if kind == 10:
        x = u0 * 5. - 2.5
        return x, x
    if kind == 11:
        n0, _ = _normal_pair(u1, u2)
        x = u0 * 5. - 2.5
        return x, x + n0
    if kind == 12:
        n0, _ = _normal_pair(u1, u2)
        x = u0 * 6. - 3.
        return x, torch.sin(x * 5.) * 2.5 + n0 * .3
    if kind == 13:
        n0, n1 = _normal_pair(u0, u1)
        x2 = 4. * n0
        return n1 + x2 * x2 / 4., x2
    raise ValueError("toy problem %r is outside 0..13" % (kind,))


def toy_reference(blocks, u, col_scale=None, dtype=torch.float32):
    """The arithmetic of gnf_hip.ops.toy_sample in torch, on any device, fp32 or fp64, with explicit uniforms u [B, P, 8] (a
    tensor or a numpy array): block p is the base problem blocks[p] (an ops.TOY_KINDS index or name) drawn from u[:, p], times
    col_scale[2p], col_scale[2p + 1] (applied in fp32's value: the scale is an fp32 vector).  -> x [B, 2P] of `dtype`.
    What the kernel computes in one launch; the tests' yardstick."""
    u = torch.as_tensor(u).to(dtype)
    cols = []
    for p, kind in enumerate(blocks):
        kind = ops.TOY_KINDS.index(kind) if isinstance(kind, str) else int(kind)
        cols.extend(_toy_block(kind, u[:, p]))
    x = torch.stack(cols, 1) if cols else u.new_zeros((u.shape[0], 0))
    if col_scale is not None:
        x = x * torch.as_tensor(np.asarray(col_scale, dtype=np.float32)).to(device=x.device, dtype=dtype)
    return x


# ----------------------------------------------------------------------------- batches
class DeviceBatches:
    """batches from gnf_hip.ops.toy_sample: the Philox key of this rank and a per-call counter, no generator state"""

    def __init__(self, name, device, rank=0, seed=0):
        self.name, self.device, self.key, self.calls = name, device, dp.gate_seed(rank, TOY_KEY + seed), 0

    def __call__(self, B):
        x = ops.toy_sample(self.name, B, self.key, self.calls, self.device)
        self.calls += 1
        return x


class HostBatches:
    """the host arm (-host_data): numpy uniforms of the kernel's resolution, toy_reference on the CPU, one copy to the device"""

    def __init__(self, name, device, rank=0, seed=0):
        self.blocks, self.scale = ops.toy_blocks(name)
        self.device, self.rng = device, np.random.RandomState(dp.gate_seed(rank, TOY_KEY + seed) % (1 << 32))

    def __call__(self, B):
        u = ((self.rng.randint(0, 1 << 23, size=(B, len(self.blocks), 8)) + .5) * (1. / (1 << 23))).astype(np.float32)
        return toy_reference(self.blocks, u, self.scale).to(self.device)


# ----------------------------------------------------------------------------- model, files
def save_name(args):
    """reference :39"""
    return NORM_TYPE + str(list(args.emb_net)) + str(args.nb_flow)


def build(args, dim):
    cond_t = COND[args.cond_type]
    cargs = {"in_size": dim, "hidden": list(args.emb_net[:-1]), "out_size": args.emb_net[-1]}
    if cond_t is DAGConditioner:                             # reference :45-49
        cargs.update(l1=args.l1, gumble_T=.5, nb_epoch_update=args.nb_steps_dual, hot_encoding=True)
    model = buildFCNormalizingFlow(args.nb_flow, cond_t, cargs, AffineNormalizer, {})
    for c in model.getConditioners():                        # reference :68-72, on every conditioner
        c.stoch_gate, c.noise_gate, c.gumble_T = True, False, .5
    return model, cond_t


@torch.no_grad()
def density_grid(model, device, npts=NPTS):
    """exp(log q) on the npts x npts grid over [LOW, HIGH]^2 in one forward (lib/visualize_flow.py:45-53): qz [npts, npts],
    row = second coordinate, as numpy's meshgrid lays it out"""
    side = np.linspace(LOW, HIGH, npts)
    xx, yy = np.meshgrid(side, side)
    x = torch.tensor(np.hstack([xx.reshape(-1, 1), yy.reshape(-1, 1)])).float().to(device)
    z, jac = model(x)
    return np.exp((model.z_log_density(z) + jac).cpu().numpy()).reshape(npts, npts)


def write_density(path_stem, qz):
    """<stem>.pgm: qz scaled to its maximum, 8-bit binary PGM; <stem>_marginals.txt: qz.sum(1) and qz.sum(0), one row each"""
    top = float(qz.max())
    img = np.zeros(qz.shape, dtype=np.uint8) if not top > 0 else np.round(np.clip(qz / top, 0, 1) * 255).astype(np.uint8)
    with open(path_stem + ".pgm", "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (qz.shape[1], qz.shape[0]))
        f.write(img.tobytes())
    np.savetxt(path_stem + "_marginals.txt", np.stack([qz.sum(1), qz.sum(0)]))


@torch.no_grad()
def test_loss(model, x_test):
    z, jac = model(x_test)
    return -(model.z_log_density(z) + jac).mean()


def train(args):
    if args.dataset not in DATASETS:
        raise SystemExit("unknown toy data set %r (one of %s)" % (args.dataset, ", ".join(DATASETS)))
    if not torch.cuda.is_available():
        raise SystemExit("train_toy.py needs an MI355X (the flow kernels have no CPU fallback)")
    rank = int(os.environ.get("RANK", "0"))
    dev = torch.device("cuda", torch.cuda.current_device())
    toy = args.dataset
    out_dir = os.path.join(args.folder, toy)
    os.makedirs(out_dir, exist_ok=True)
    stem = os.path.join(out_dir, save_name(args))
    batches = (HostBatches if args.host_data else DeviceBatches)(toy, dev, rank, args.seed)
    x_test = batches(N_TEST)                                  # drawn once, at offset 0
    dim = x_test.shape[1]
    torch.manual_seed(args.seed)
    model, cond_t = build(args, dim)
    if args.load:
        model.load_state_dict(torch.load(stem + "model.pt", map_location="cpu"))
    model.to(dev)
    model.train()
    dp.seed_gates(model, rank)
    state = dp.FlatState(model)
    if args.load:
        state.load_optimizer_state_dict(model, torch.load(stem + "ADAM.pt", map_location=dev))
    log = open(os.path.join(out_dir, "logs"), "a")

    def say(msg):
        print(msg, flush=True)
        log.write(msg + "\n")
        log.flush()

    say(str(vars(args)))
    train_losses, test_losses, epoch_seconds = [], [], []
    for epoch in range(args.nb_epoch):
        t0 = time.perf_counter()
        loss_tot = torch.zeros((), device=dev)
        for _ in range(0, args.nb_samp, args.batch_size):
            loss = dp.train_step(model, state, batches(args.batch_size), lr=1e-4, weight_decay=1e-5, graph="auto")
            loss_tot += loss.detach()
        if not torch.isfinite(loss_tot):
            raise SystemExit("non-finite training loss %r in epoch %d" % (float(loss_tot), epoch))
        model.step(epoch, loss_tot)
        elapsed = time.perf_counter() - t0
        ll_test = float(test_loss(model, x_test))
        with torch.no_grad():
            dagness = float(max(model.DAGness()))
        train_losses.append(float(loss_tot))
        test_losses.append(ll_test)
        epoch_seconds.append(elapsed)
        say("epoch: %d - Train loss: %4f - Test loss: %4f - <<DAGness>>: %4f - Elapsed time per epoch %4f (seconds)"
            % (epoch, train_losses[-1], ll_test, dagness, elapsed))
        if epoch % args.plot_every == 0:
            if dim == 2:
                write_density(os.path.join(out_dir, "flow_%s_%d" % (save_name(args), epoch)), density_grid(model, dev))
            if cond_t is DAGConditioner:
                for k, c in enumerate(model.getConditioners()):
                    np.savetxt(os.path.join(out_dir, "A_%d_%d.txt" % (k, epoch)),
                               c.soft_thresholded_A().detach().cpu().numpy())
            torch.save(model.state_dict(), stem + "model.pt")
            torch.save(state.optimizer_state_dict(model, 1e-4, 1e-5), stem + "ADAM.pt")
    log.close()
    return ToyRun(model, state, train_losses, test_losses, epoch_seconds)


def parse(argv=None):
    ap = argparse.ArgumentParser(description="toy density estimation with graphical normalizing flows on MI355X")
    # the reference's arguments (:164-170)
    ap.add_argument("-dataset", default=None, choices=DATASETS, help="Which toy problem ?")
    ap.add_argument("-load", default=False, action="store_true", help="Load a model ?")
    ap.add_argument("-folder", default="", help="Folder")
    ap.add_argument("-nb_steps_dual", default=50, type=int,
                    help="number of step between updating Acyclicity constraint and sparsity constraint")
    ap.add_argument("-l1", default=.0, type=float, help="Maximum weight for l1 regularization")
    ap.add_argument("-nb_epoch", default=20000, type=int, help="Number of epochs")
    # what the reference hard-codes (:22-23, :30-31, :126), with its values
    ap.add_argument("-cond_type", default="Coupling", choices=sorted(COND))
    ap.add_argument("-nb_flow", default=3, type=int)
    ap.add_argument("-emb_net", default=[150, 150, 150], nargs="+", type=int)
    ap.add_argument("-batch_size", default=100, type=int)
    ap.add_argument("-nb_samp", default=100, type=int)
    ap.add_argument("-seed", default=0, type=int, help="model initialisation and the key of the batches")
    ap.add_argument("-plot_every", default=500, type=int, help="epochs between checkpoints / density files")
    ap.add_argument("-host_data", default=False, action="store_true",
                    help="draw the batches on the host (toy_reference on numpy uniforms) instead of the HIP sampler")
    return ap.parse_args(argv)


if __name__ == "__main__":
    a = parse()
    for name in ([a.dataset] if a.dataset is not None else DATASETS):     # reference :181-190: no -dataset runs them all
        train(argparse.Namespace(**dict(vars(a), dataset=name)))
