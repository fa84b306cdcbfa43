"""Tabular density-estimation driver on the MI355X flow path: the run configurations, model construction, epoch
schedule and checkpoint files of the reference's UCIExperiments.py (:58-220, argument names :226-256, yml schema of
UCIExperimentsConfigurations.yml), re-hosted on one process per GPU (`torchrun --nproc-per-node N train_uci.py ...`,
RCCL) with the fused step of gnf_hip.dp.  Datasets are not bundled: pass `-data file.npz` (arrays trn / val / tst,
standardised as in the reference's loaders) or `-data synthetic` for N(0,1) data of the dataset's dimension.

Opt-in: `-device_batches` gathers the training batches on the device through a Philox-keyed permutation per epoch
(gnf_hip.dp.DeviceBatches; `-seed`), `-steps_per_replay K` replays K optimisation steps from one hipGraph, and
`-threshold_sweep` adds the reference's validation at five hard thresholds every 10th epoch (:183-212).
`-context_cols K` trains a CONDITIONAL flow p(first d - K columns | last K columns): the model is built with cond_in = K
and every batch is split into (x, context) -- behind the gather when the batches come from the device.
`-sample N` (after the last evaluation) draws N samples x ~ p(x | context of the first N test rows) through model.invert into
`samples.npy` in -folder and prints the mean |z - forward(x, ctx)| (sample_rows).
`-do COL=VALUE [COL=VALUE ...]` (with -sample N) draws N INTERVENTIONAL samples as well, from the same z and contexts, through
model.intervene into `samples_do.npy`, and prints the mean |z - forward(x, ctx)| over the un-pinned columns and the
per-column mean shift against the un-intervened samples (sample_do_rows).  One-step flows only: -nb_flow > 1 ends with the
model's ValueError, reported.

`-regimes` trains on a MIX of observational and interventional rows with the interventional likelihood
(model.loss_do / log_prob_do): the -data npz then also holds `targets` [R, modelled columns] (non-zero: the variable is an
intervention target in that regime) and `trn_regime` / `val_regime` / `tst_regime` [n]; `-data synthetic -regimes` makes
regime r = row % (d + 1), regime 0 observational, regime r > 0 pinning column r - 1 at 2 + 0.1 randn.  One-step flows, host
batches only: refused with -device_batches, -steps_per_replay > 1 and -nb_flow > 1.

Checkpoints: `model.pt` is `state_dict()` with the reference's keys, `ADAM.pt` is in torch.optim.Adam's format, so
either side can resume the other's run."""
import argparse
import math
import os
import re
import sys
import time

import numpy as np
import torch
import torch.distributed as dist
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from models import (buildFCNormalizingFlow, DAGConditioner, CouplingConditioner, AutoregressiveConditioner,  # noqa: E402
                    StrADEConditioner, AffineNormalizer, MonotonicNormalizer, SplineNormalizer)
from gnf_hip import dp  # noqa: E402

COND = {"DAG": DAGConditioner, "Coupling": CouplingConditioner, "Autoregressive": AutoregressiveConditioner,
        "StrADE": StrADEConditioner}
NORM = {"affine": AffineNormalizer, "monotonic": MonotonicNormalizer, "spline": SplineNormalizer}
DIMS = {"power": 6, "gas": 8, "hepmass": 21, "miniboone": 43, "bsds300": 63, "digits": 64, "proteins": 11}


def load_split(spec, dataset, seed=0):
    if spec == "synthetic":
        g = torch.Generator().manual_seed(seed)
        d = DIMS[dataset]
        return [torch.randn(n, d, generator=g) for n in (20000, 2000, 2000)]
    z = np.load(spec)
    return [torch.from_numpy(np.asarray(z[k], dtype=np.float32)) for k in ("trn", "val", "tst")]


def load_regimes(spec, dataset, splits, context_cols=0, seed=0):
    """-regimes: (splits, targets uint8 [R, d], [trn_regime, val_regime, tst_regime] as int64 [n]) for the d modelled columns.
    synthetic: regime r = row % (d + 1); regime 0 is observational, regime r > 0 targets column r - 1, whose values are
    overwritten by 2 + 0.1 randn (the splits are changed in place).  A file: its arrays `targets` and `*_regime`.
    validate_regimes checks what comes back."""
    if spec == "synthetic":
        d = DIMS[dataset] - context_cols
        g = torch.Generator().manual_seed(seed + 1)
        targets = torch.cat((torch.zeros(1, d, dtype=torch.uint8), torch.eye(d, dtype=torch.uint8)))
        regimes = []
        for X in splits:
            r = torch.arange(X.shape[0]) % (d + 1)
            for col in range(d):
                rows = r == col + 1
                X[rows.to(X.device), col] = (2. + .1 * torch.randn(int(rows.sum()), generator=g)).to(X.device)
            regimes.append(r)
        return splits, targets, regimes
    z = np.load(spec)
    missing = [k for k in ("targets", "trn_regime", "val_regime", "tst_regime") if k not in z.files]
    if missing:
        raise ValueError("-regimes: %s holds no %s (needed: targets [R, d], trn_regime / val_regime / tst_regime [n])"
                         % (spec, ", ".join(missing)))
    targets = torch.from_numpy(np.asarray(z["targets"]))
    return splits, targets, [torch.from_numpy(np.asarray(z[k + "_regime"])) for k in ("trn", "val", "tst")]


def validate_regimes(targets, regimes, splits, d):
    """once, after loading: targets [R, d] (bool / integer, read as non-zero = pinned) and one integer regime id in [0, R) per
    row of every split -> (targets as uint8, regimes as int64).  ValueError otherwise.  The per-batch calls then skip the
    check (check_regime=False)."""
    if targets.dim() != 2 or targets.shape[1] != d or targets.dtype.is_floating_point or targets.dtype.is_complex:
        raise ValueError("-regimes: targets must be an integer or bool [R, %d] table, got %s %s"
                         % (d, targets.dtype, tuple(targets.shape)))
    R = targets.shape[0]
    out = []
    for name, r, X in zip(("trn", "val", "tst"), regimes, splits):
        if r.dim() != 1 or r.shape[0] != X.shape[0] or r.dtype.is_floating_point or r.dtype.is_complex or r.dtype == torch.bool:
            raise ValueError("-regimes: %s_regime must be an integer vector [%d], got %s %s"
                             % (name, X.shape[0], r.dtype, tuple(r.shape)))
        if r.numel() and (int(r.min()) < 0 or int(r.max()) >= R):
            raise ValueError("-regimes: %s_regime spans [%d, %d], targets has R = %d rows"
                             % (name, int(r.min()), int(r.max()), R))
        out.append(r.to(torch.int64))
    return (targets != 0).to(torch.uint8).contiguous(), out


def batches(X, b, shuffle, gen):
    idx = torch.randperm(X.shape[0], generator=gen) if shuffle else torch.arange(X.shape[0])
    for i in range(0, X.shape[0], b):
        yield X[idx[i:i + b].to(X.device)]


def shard_batches(n, b, rank, world, gen):
    """Index tensors of this rank's share of every global minibatch of one epoch.  The permutation is drawn from `gen`,
    which every rank seeds identically, so all ranks cut the SAME global batches; each batch is trimmed to a multiple
    of `world` rows and dealt round-robin, so every rank runs the same number of steps with the same shard size (no rank
    is left waiting in the per-step all-reduce, and the mean of the rank means is the global batch mean)."""
    idx = torch.randperm(n, generator=gen)
    out = []
    for i in range(0, n, b):
        cur = idx[i:i + b]
        keep = cur.numel() // world * world
        if keep:
            out.append(cur[:keep][rank::world])
    return out


def load_adjacency(path, dim):
    """the [dim, dim] 0/1 graph of -adjacency: a .npy array (adjacency[i][j] = 1: x_j is a parent of x_i), or a checkpoint
    (state_dict) of a one-step DAG flow, whose get_dag() is taken after post_process(); None without a path"""
    if path is None:
        return None
    if path.endswith(".npy"):
        return np.load(path)
    sd = torch.load(path, map_location="cpu")
    keys = [k for k in sd if k.endswith("conditioner.A")]
    if len(keys) != 1:
        raise ValueError("-adjacency %s: a checkpoint of a ONE-step DAG flow is needed (found %d DAG conditioners)"
                         % (path, len(keys)))
    cond = DAGConditioner(dim, [8], 2)
    with torch.no_grad():
        cond.A.copy_(sd[keys[0]])
    cond.post_process()                                   # (a no-op on a checkpoint saved after it: A is 0/1 already)
    return (cond.get_dag().A.detach().cpu() != 0).to(torch.uint8).numpy()


def build(args, dim):
    cond_t, norm_t = COND[args.conditioner], NORM[args.normalizer]
    cargs = {"in_size": dim, "hidden": args.emb_net[:-1], "out_size": args.emb_net[-1]}
    if getattr(args, "context_cols", 0):      # `dim` counts the modelled columns only
        cargs["cond_in"] = args.context_cols
    if cond_t is DAGConditioner:          # reference :83-88 (gumble_T is pinned to .5 there)
        cargs.update(l1=args.l1, gumble_T=.5, nb_epoch_update=args.nb_steps_dual, hot_encoding=True)
    if cond_t is StrADEConditioner:       # a masked net over a GIVEN graph; without -adjacency the full triangular one
        if args.nb_flow > 1:
            raise ValueError("-conditioner StrADE with -nb_flow %d: one graph describes the data-side variables of a ONE-step "
                             "flow; the variables between two steps are flipped and are not the data's" % args.nb_flow)
        cargs["adjacency"] = load_adjacency(getattr(args, "adjacency", None), dim)
    nargs = {}
    if norm_t is MonotonicNormalizer:
        nargs = {"integrand_net": args.int_net, "cond_size": args.emb_net[-1], "nb_steps": args.nb_steps,
                 "solver": args.solver}
    if norm_t is SplineNormalizer:
        nargs = {"nb_bins": getattr(args, "spline_bins", 8), "tail_bound": getattr(args, "spline_tail", 3.)}
        need = SplineNormalizer.h_size(**nargs)
        if args.emb_net[-1] < need:              # before any training: the kernel would refuse the first batch
            raise ValueError("-normalizer spline with -spline_bins %d reads 3 K - 1 = %d conditioner outputs per variable: "
                             "the last entry of -emb_net is %d" % (nargs["nb_bins"], need, args.emb_net[-1]))
    model = buildFCNormalizingFlow(args.nb_flow, cond_t, cargs, norm_t, nargs)
    if getattr(args, "gated_front", False):      # DAG gate and one-hot built inside the first DAGMLP layer (csrc/gnf_dagmlp.hip)
        for c in model.getConditioners():
            if hasattr(getattr(c, "embedding_net", None), "gated_front"):
                c.embedding_net.gated_front = True
    return model, cond_t, norm_t


def split_context(rows, k):
    """(x, context) of a batch of data rows: the last k columns are the context (-context_cols), None for k = 0"""
    if not k:
        return rows, None
    return rows[:, :rows.shape[1] - k].contiguous(), rows[:, rows.shape[1] - k:].contiguous()


@torch.no_grad()
def mean_ll(model, X, b, gen, on_device=False, context_cols=0):
    """mean over the batches of the batch means.  on_device (-device_batches): the means add up in a device scalar and
    ONE read-back ends the pass, instead of one per batch"""
    tot, n = torch.zeros((), device=X.device) if on_device else 0., 0
    for cur in batches(X, b, False, gen):
        cur, ctx = split_context(cur, context_cols)
        z, jac = model(cur) if ctx is None else model(cur, ctx)
        ll = (model.z_log_density(z) + jac).mean()
        tot += ll if on_device else ll.item()
        n += 1
    return float(tot) / max(n, 1)


@torch.no_grad()
def mean_ll_do(model, X, regime, targets, b, context_cols=0):
    """-regimes: mean over the batches of the batch means of log p(x | do(x_S(regime))) (model.log_prob_do; the regime ids
    were validated once, after loading)"""
    tot, n = 0., 0
    for i in range(0, X.shape[0], b):
        cur, ctx = split_context(X[i:i + b], context_cols)
        tot += model.log_prob_do(cur, targets, regime[i:i + b], ctx, check_regime=False).mean().item()
        n += 1
    return tot / max(n, 1)


@torch.no_grad()
def sample_rows(model, tst, n, context_cols, seed, folder, say=print):
    """-sample N: x ~ p(x | c) for the contexts of the first N rows of the test split (their last context_cols columns;
    an unconditional flow: x ~ p(x)), z ~ N(0, I) from a torch.Generator seeded by `seed`, through model.invert.  Writes
    samples.npy into `folder`: [N, modelled columns + context columns], in the normalisation of the data.  Returns and
    reports the mean |z - forward(x, ctx)[0]|, as the reference's image script does for its samples
    (ImageExperiments.py:341-350)."""
    import numpy as np
    rows = tst[:n]
    _, ctx = split_context(rows, context_cols)
    d = rows.shape[1] - context_cols
    z = torch.randn(rows.shape[0], d, generator=torch.Generator().manual_seed(int(seed))).to(rows.device)
    x = model.invert(z) if ctx is None else model.invert(z, ctx)
    zz = (model(x) if ctx is None else model(x, ctx))[0]
    err = float((z - zz).abs().mean()) if z.numel() else 0.
    out = x if ctx is None else torch.cat((x, ctx), 1)
    os.makedirs(folder, exist_ok=True)
    np.save(os.path.join(folder, "samples.npy"), out.cpu().numpy())
    say("samples: %d rows -> %s - mean |z - forward(x)|: %.3e" % (out.shape[0], os.path.join(folder, "samples.npy"), err))
    return err


def parse_do(pairs, d):
    """-do COL=VALUE ... -> ([columns], [values]); ValueError for anything else (a column twice or outside 0 .. d - 1 is
    left to model.intervene, which says it better)"""
    cols, vals = [], []
    for item in pairs:
        col, sep, val = str(item).partition("=")
        try:
            if not sep:
                raise ValueError
            cols.append(int(col))
            vals.append(float(val))
        except ValueError:
            raise ValueError("-do %r: expected COL=VALUE with an integer column of the %d modelled ones and a number"
                             % (item, d)) from None
    return cols, vals


@torch.no_grad()
def sample_do_rows(model, tst, n, context_cols, seed, folder, do, say=print):
    """-sample N -do COL=VALUE ...: x ~ p(x | do(x_COL = VALUE), c) for the z and the contexts sample_rows uses, through
    model.intervene.  Writes samples_do.npy ([N, modelled columns + context columns]); reports the mean |z - forward(x, ctx)|
    over the UN-pinned columns (a pinned column's z is not the one drawn) and the per-column mean of x_do - x against the
    un-intervened samples of the same z.  Returns (that mean, the shifts as a list)."""
    import numpy as np
    rows = tst[:n]
    _, ctx = split_context(rows, context_cols)
    d = rows.shape[1] - context_cols
    cols, vals = parse_do(do, d)
    z = torch.randn(rows.shape[0], d, generator=torch.Generator().manual_seed(int(seed))).to(rows.device)
    value = torch.tensor(vals, dtype=z.dtype, device=z.device)
    x = model.intervene(z, cols, value) if ctx is None else model.intervene(z, cols, value, ctx)
    base = model.invert(z) if ctx is None else model.invert(z, ctx)
    zz = (model(x) if ctx is None else model(x, ctx))[0]
    free = [i for i in range(d) if i not in cols]
    err = float((z - zz)[:, free].abs().mean()) if z.shape[0] and free else 0.
    shift = (x - base).mean(0).tolist() if z.shape[0] else [0.] * d
    out = x if ctx is None else torch.cat((x, ctx), 1)
    os.makedirs(folder, exist_ok=True)
    np.save(os.path.join(folder, "samples_do.npy"), out.cpu().numpy())
    say("samples under do(%s): %d rows -> %s - mean |z - forward(x)| over the un-pinned columns: %.3e"
        % (", ".join("x%d = %g" % cv for cv in zip(cols, vals)), out.shape[0], os.path.join(folder, "samples_do.npy"), err))
    say("mean shift per column against the un-intervened samples: " + " ".join("%+.4f" % s for s in shift))
    return err, shift


THRESHOLDS = (.95, .5, .1, .01, .0001)


def threshold_sweep(model, val, b, gen, epoch, say, on_device=False, context_cols=0, do_tab=None):
    """every 10th epoch (UCIExperiments.py:183-212): validation with the deterministic hard-thresholded adjacency at five
    thresholds, the gate settings restored afterwards.  The mean is over the batch count (the reference divides by the
    last batch INDEX, :202), and h_thresh returns to the value it had (the reference leaves the last threshold set).
    do_tab (-regimes): (targets, regime ids of `val`) -- the rows are scored by log_prob_do, as the epoch's validation is"""
    conds = model.getConditioners()
    saved = [(c.stoch_gate, c.noise_gate, c.s_thresh, c.h_thresh) for c in conds]
    for c in conds:
        c.stoch_gate, c.noise_gate, c.s_thresh = False, False, True
    try:
        for th in THRESHOLDS:
            for c in conds:
                c.h_thresh = th
            # (-context_cols 0 makes today's call: a mean_ll installed by a caller keeps its five arguments)
            if do_tab is not None:
                ll = mean_ll_do(model, val, do_tab[1], do_tab[0], b, context_cols)
            else:
                ll = mean_ll(model, val, b, gen, on_device, context_cols) if context_cols else mean_ll(model, val, b, gen, on_device)
            with torch.no_grad():
                dagness = float(max(model.DAGness()))
            say("epoch: %d - Threshold: %4f - Valid log-likelihood: %4f - <<DAGness>>: %4f" % (epoch, th, ll, dagness))
    finally:
        for c, (sg, ng, st, ht) in zip(conds, saved):
            c.stoch_gate, c.noise_gate, c.s_thresh, c.h_thresh = sg, ng, st, ht


def train_epoch(args, model, state, norm_t, trn, src, epoch_no, rank, world, gen, do_tab=None):
    """the optimisation steps of one epoch -> (device sum of the step losses, number of steps).  src = None: the batches
    are slices of a host permutation drawn from `gen`, copied over; a dp.DeviceBatches: gathered on the device from the
    permutation of epoch `epoch_no`.  do_tab (-regimes; src is None then): (targets, regime ids of the training rows) -- every
    step minimises model.loss_do on its batch with that batch's own ids (each rank its shard's), validated once in train()"""
    dev = trn.device
    ll_tot, n = torch.zeros((), device=dev), 0
    ctx_cols = int(getattr(args, "context_cols", 0))
    if src is not None:
        group = 1 if ctx_cols else int(getattr(args, "steps_per_replay", 1))     # a conditional step is never replayed
        src.start_epoch(epoch_no)
        # groups of -steps_per_replay full batches from one hipGraph replay each, while the flow admits it (asked every
        # epoch: model.step() changes the gate flags); what is left over runs step by step below
        while group > 1 and src.full_left() >= group and dp.steps_replayable(model, src):
            ll_tot += dp.train_steps(model, state, src, group, lr=args.learning_rate, weight_decay=args.weight_decay)
            n += group
        feed = ((src.next(), None) for _ in range(src.left()))
    else:
        shards = (rows.to(dev) for rows in shard_batches(trn.shape[0], max(args.b_size, world), rank, world, gen))
        feed = ((trn[rows], None if do_tab is None else do_tab[1][rows]) for rows in shards)
    for x, reg in feed:
        if norm_t is MonotonicNormalizer:                    # node-count jitter of the reference (:131-133)
            k = args.nb_steps + int(torch.randint(0, 10, [1], generator=gen))
            for nrm in model.getNormalizers():
                nrm.nb_steps = k
        kw = {}                                              # (neither option makes exactly today's call)
        if ctx_cols:                                         # (a gathered batch is split behind the gather)
            x, kw["context"] = split_context(x, ctx_cols)
        if reg is not None:
            kw.update(targets=do_tab[0], regime=reg, check_regime=False)
        loss = dp.train_step(model, state, x, lr=args.learning_rate, weight_decay=args.weight_decay, **kw)
        ll_tot += loss.detach()
        n += 1
    return ll_tot, n


def train(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("train_uci.py needs an MI355X (the flow kernels have no CPU fallback)")
    backend = os.environ.get("GNF_DIST_BACKEND", "nccl")     # "nccl" is RCCL; "gloo" only to exercise N>1 on a 1-GPU box
    ndev = torch.cuda.device_count()
    if backend == "nccl" and local >= ndev:
        raise SystemExit("rank %d has no GPU (%d visible)" % (local, ndev))
    local %= max(ndev, 1)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    trn, val, tst = [t.to(dev) for t in load_split(args.data, args.dataset)]
    torch.manual_seed(0)
    ctx_cols = int(getattr(args, "context_cols", 0))
    if not 0 <= ctx_cols < trn.shape[1]:
        raise SystemExit("-context_cols %d: the data has %d columns, at least one must be modelled" % (ctx_cols, trn.shape[1]))
    do_tab = None
    if getattr(args, "regimes", False):
        # validated ONCE, here; every batch then goes to the kernels unchecked (their NaN rule is the backstop)
        splits, targets, regimes = load_regimes(args.data, args.dataset, [trn, val, tst], ctx_cols)
        try:
            targets, regimes = validate_regimes(targets, regimes, splits, trn.shape[1] - ctx_cols)
        except ValueError as exc:
            raise SystemExit(str(exc))
        trn, val, tst = splits
        do_tab = (targets.to(dev), [r.to(dev).to(torch.int32) for r in regimes])   # the kernels' types: no cast per batch
    model, cond_t, norm_t = build(args, trn.shape[1] - ctx_cols)
    os.makedirs(args.folder, exist_ok=True)
    tag = "_" + args.f_number if args.f_number is not None else ""
    if args.load:
        model.load_state_dict(torch.load(os.path.join(args.folder, "model%s.pt" % tag), map_location="cpu"))
    model.to(dev)
    dp.seed_gates(model, rank)                               # independent gate noise per rank and per flow step
    state = dp.FlatState(model)
    state.broadcast(0)
    adam_file = os.path.join(args.folder, "ADAM%s.pt" % tag)
    if args.load and os.path.isfile(adam_file):
        state.load_optimizer_state_dict(model, torch.load(adam_file, map_location=dev))
    gen = torch.Generator().manual_seed(1234)
    on_dev = bool(getattr(args, "device_batches", False))
    src, epoch0 = None, 0
    if on_dev:
        # batches gathered on the device through the sort of Philox keys (dp.DeviceBatches): the permutation of an epoch is a
        # function of (-seed, the number of epochs trained so far, n) -- the count comes from the optimiser's step number, which
        # ADAM.pt carries, so a resumed run goes on with the epochs a single run would have reached
        src = dp.DeviceBatches(trn, max(args.b_size, world), rank, world, seed=args.seed)
        epoch0 = state.t // max(len(src), 1)
    best = math.inf
    log = open(os.path.join(args.folder, "logs"), "a") if rank == 0 else None

    def say(msg):
        if rank == 0:
            print(msg, flush=True)
            log.write(msg + "\n")
            log.flush()

    say(str(vars(args)))
    ctx_arg = (ctx_cols,) if ctx_cols else ()                # -context_cols 0 makes exactly today's calls
    if ctx_cols and getattr(args, "steps_per_replay", 1) > 1:
        say("-steps_per_replay %d is ignored with -context_cols: a step with a context runs launch by launch"
            % args.steps_per_replay)
    for epoch in range(args.nb_epoch):
        t0 = time.perf_counter()
        if cond_t is DAGConditioner:
            with torch.no_grad():
                for c in model.getConditioners():
                    c.constrainA(zero_threshold=0.)
        ll_tot = torch.zeros((), device=dev)
        if not args.test:
            ll_tot, n = train_epoch(args, model, state, norm_t, trn, src, epoch0 + epoch, rank, world, gen,
                                    *(() if do_tab is None else ((do_tab[0], do_tab[1][0]),)))
            ll_tot /= max(n, 1)
            if world > 1:
                # model.step() decides the dual update / post-processing from this value (DAGConditioner.step): every
                # replica must take the same branch, so they all see the mean over ranks
                dp.all_reduce_sum(ll_tot)
                ll_tot /= world
            if not torch.isfinite(ll_tot):
                if rank == 0:
                    torch.save(model.state_dict(), os.path.join(args.folder, "NANmodel.pt"))
                raise SystemExit("non-finite loss")
            model.step(epoch, ll_tot)
            if not dp.replicas_identical(state, model):
                raise SystemExit("data-parallel replicas diverged in epoch %d" % epoch)
        if norm_t is MonotonicNormalizer:
            for nrm in model.getNormalizers():
                nrm.nb_steps = args.nb_steps + 20
        if do_tab is not None:
            ll_val = mean_ll_do(model, val, do_tab[1][1], do_tab[0], args.b_size, ctx_cols)
        else:
            ll_val = mean_ll(model, val, args.b_size, gen, on_dev, *ctx_arg)
        with torch.no_grad():
            dagness = float(max(model.DAGness()))
        say("epoch: %d - Train loss: %4f - Valid log-likelihood: %4f - <<DAGness>>: %4f - Elapsed time per epoch %4f "
            "(seconds)" % (epoch, float(ll_tot), ll_val, dagness, time.perf_counter() - t0))
        if rank == 0:
            if dagness < 1e-20 and -ll_val < best:
                best = -ll_val
                torch.save(model.state_dict(), os.path.join(args.folder, "best_model.pt"))
                ll_tst = (mean_ll_do(model, tst, do_tab[1][2], do_tab[0], args.b_size, ctx_cols) if do_tab is not None else
                          mean_ll(model, tst, args.b_size, gen, on_dev, *ctx_arg))
                say("epoch: %d - Test log-likelihood: %4f - <<DAGness>>: %4f" % (epoch, ll_tst, dagness))
        if getattr(args, "threshold_sweep", False) and epoch % 10 == 0 and cond_t is DAGConditioner:
            # every rank: same work, rank 0 logs
            if do_tab is not None:
                threshold_sweep(model, val, args.b_size, gen, epoch, say, on_dev, ctx_cols, (do_tab[0], do_tab[1][1]))
            else:
                threshold_sweep(model, val, args.b_size, gen, epoch, say, on_dev, *ctx_arg)
        if rank == 0:
            torch.save(model.state_dict(), os.path.join(args.folder, "model.pt"))
            torch.save(state.optimizer_state_dict(model, args.learning_rate, args.weight_decay),
                       os.path.join(args.folder, "ADAM.pt"))
    refused = False
    if getattr(args, "sample", 0) > 0 and rank == 0:
        sample_rows(model, tst, args.sample, ctx_cols, args.seed, args.folder, say)
        if getattr(args, "do", None):
            try:
                sample_do_rows(model, tst, args.sample, ctx_cols, args.seed, args.folder, args.do, say)
            except ValueError as exc:                        # a multi-step flow, a column twice or out of range
                say("-do: %s" % exc)
                refused = True
    if world > 1:
        dist.destroy_process_group()                         # (before the exit below: the other ranks wait in it)
    if refused:
        raise SystemExit(2)
    return model


_SCI = re.compile(r"[-+]?(\d[\d_]*\.?[\d_]*|\.[\d_]+)([eE][-+]?\d+)?")


def _yml_number(v):
    """PyYAML reads `1e-3` and `.5e1` as strings (YAML 1.1 wants a dot AND a signed exponent); the reference installs a
    YAML 1.2 float resolver so that its configuration file's `weight_decay: 1e-3` arrives as a float
    (UCIExperiments.py:258-269, UCIExperimentsConfigurations.yml:84).  Same outcome: plain-number strings -> float."""
    if isinstance(v, str) and _SCI.fullmatch(v.strip()):
        return float(v.replace("_", ""))
    if isinstance(v, list):
        return [_yml_number(e) for e in v]
    return v


def parse(argv=None):
    ap = argparse.ArgumentParser(description="UCI density estimation with graphical normalizing flows on MI355X")
    ap.add_argument("-load_config", default=None, type=str)
    ap.add_argument("-config_file", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "uci_configs.yml"))
    ap.add_argument("-dataset", default=None, choices=sorted(DIMS))
    ap.add_argument("-data", default="synthetic")
    ap.add_argument("-load", default=False, action="store_true")
    ap.add_argument("-folder", default="")
    ap.add_argument("-f_number", default=None, type=str)
    ap.add_argument("-test", default=False, action="store_true")
    ap.add_argument("-nb_flow", type=int, default=1)
    ap.add_argument("-weight_decay", default=1e-5, type=float)
    ap.add_argument("-learning_rate", default=1e-3, type=float)
    ap.add_argument("-nb_epoch", default=10000, type=int)
    ap.add_argument("-b_size", default=100, type=int)
    ap.add_argument("-conditioner", default="DAG", choices=sorted(COND))
    ap.add_argument("-adjacency", default=None, type=str,
                    help="-conditioner StrADE: the graph, a [d, d] .npy array (row i: the parents of x_i) or a checkpoint of a "
                         "one-step DAG flow (its get_dag() after post_process()); default: the full triangular graph")
    ap.add_argument("-emb_net", default=[100, 100, 100, 10], nargs="+", type=int)
    ap.add_argument("-nb_steps_dual", default=100, type=int)
    ap.add_argument("-l1", default=.2, type=float)
    ap.add_argument("-gumble_T", default=1., type=float)
    ap.add_argument("-normalizer", default="affine", choices=sorted(NORM))
    ap.add_argument("-spline_bins", default=8, type=int, help="-normalizer spline: bins K (2 .. 32); -emb_net must end in >= 3 K - 1")
    ap.add_argument("-spline_tail", default=3., type=float, help="-normalizer spline: the spline acts on [-T, T], identity outside")
    ap.add_argument("-int_net", default=[100, 100, 100, 100], nargs="+", type=int)
    ap.add_argument("-nb_steps", default=20, type=int)
    ap.add_argument("-solver", default="CC", type=str, choices=["CC", "CCParallel"])
    ap.add_argument("-gated_front", default=False, action="store_true",
                    help="DAGMLP.gated_front = True on every DAG conditioner: gate and one-hot fused into the first layer")
    ap.add_argument("-device_batches", default=False, action="store_true",
                    help="training batches gathered on the device through a Philox-keyed permutation (gnf_tab_batch)")
    ap.add_argument("-seed", default=0, type=int, help="Philox key of the -device_batches permutations")
    ap.add_argument("-steps_per_replay", default=1, type=int,
                    help="with -device_batches: optimisation steps captured into one hipGraph replay")
    ap.add_argument("-threshold_sweep", default=False, action="store_true",
                    help="DAG conditioners: validation at five hard thresholds every 10th epoch")
    ap.add_argument("-context_cols", default=0, type=int,
                    help="the last K columns of the data are the context of a conditional flow over the others (cond_in = K)")
    ap.add_argument("-sample", default=0, type=int,
                    help="after the last evaluation: N samples x ~ p(x | context of the first N test rows) into samples.npy")
    ap.add_argument("-do", default=None, nargs="+", metavar="COL=VALUE",
                    help="with -sample N: N samples under the intervention do(x_COL = VALUE, ...) into samples_do.npy")
    ap.add_argument("-regimes", default=False, action="store_true",
                    help="train on observational and interventional rows with the interventional likelihood: -data holds "
                         "targets [R, d] and trn_regime / val_regime / tst_regime [n] (synthetic: regime = row %% (d + 1))")
    args = ap.parse_args(argv)
    if args.load_config is not None:                         # a named entry of the yml overrides the command line
        with open(args.config_file) as f:
            cfg = yaml.safe_load(f)[args.load_config]
        for k, v in cfg.items():
            setattr(args, k, _yml_number(v))
    if args.dataset is None:
        ap.error("-dataset (or a -load_config entry naming one) is required")
    if args.steps_per_replay < 1:
        ap.error("-steps_per_replay must be at least 1")
    if args.sample < 0:
        ap.error("-sample must not be negative")
    if args.context_cols < 0:
        ap.error("-context_cols must not be negative")
    if args.conditioner == "StrADE" and args.nb_flow > 1:
        ap.error("-conditioner StrADE with -nb_flow > 1: one graph describes the data-side variables of a ONE-step flow")
    if args.adjacency is not None and args.conditioner != "StrADE":
        ap.error("-adjacency needs -conditioner StrADE")
    if args.do and args.sample <= 0:
        ap.error("-do needs -sample N (the interventional samples are drawn from the z of the plain ones)")
    if args.steps_per_replay > 1 and not args.device_batches:
        ap.error("-steps_per_replay needs -device_batches (a replayed group reads its batches from device memory)")
    if args.regimes:
        if args.device_batches:
            ap.error("-regimes with -device_batches: the device-side epochs gather the data rows only, a batch's regime ids "
                     "are not carried through the gather")
        if args.steps_per_replay > 1:
            ap.error("-regimes with -steps_per_replay > 1: a replayed group has one input buffer per step and none for the "
                     "regime ids; a step with regimes runs launch by launch")
        if args.nb_flow > 1:
            ap.error("-regimes with -nb_flow > 1: the truncated factorisation is defined on the data-side equations of a "
                     "ONE-step flow")
    if not args.folder:
        args.folder = os.path.join("runs", args.load_config or args.dataset)
    return args


if __name__ == "__main__":
    train(parse())
