"""Flow composition on the MI355X path: one (conditioner, normalizer) step, a stack of steps, and the multi-scale
image flow.  Class and method names, constructor arguments and `state_dict` keys are those of the reference's
models/NormalizingFlow.py (the drivers call getConditioners / getNormalizers / DAGness / step / isInvertible / invert
by name); the bodies are written against gnf_hip.ops.

    step:   h = conditioner(x);  z, jac = normalizer(x, h);  log|det J| = sum_i log jac_i      (reference :61-70)
    stack:  steps in sequence, feature order reversed between steps, log-dets added             (reference :110-126)
    loss:   sum of conditioner constraint terms - mean(log|det J| + log N(z))                  (reference :128-146)
"""
import contextlib
import weakref

import torch
import torch.nn as nn

from gnf_hip import ops
from .Conditionners import Conditioner, DAGConditioner
from .Conditionners.AutoregressiveConditioner import made_do_launches
from .Conditionners.Conditioner import checked_context
from .Normalizers import Normalizer, AffineNormalizer, SplineNormalizer


# captured inversion graphs per NormalizingFlowStep, kept OUTSIDE the modules: a hipGraph is neither copyable nor
# picklable, and flows are deep-copied / saved by the drivers
_INV_GRAPHS = weakref.WeakKeyDictionary()


def _crop_order(host_rows):
    """the variables of one level of a 28 x 28 image in the order the sparse embedding kernels work in: crop origin, pixel"""
    return tuple(sorted(host_rows, key=lambda r: (8 * ops.crop_origin(r // 28) + ops.crop_origin(r % 28), r)))


def _is_dag(conditioner):
    # exact type test, as everywhere in the reference (subclasses are deliberately not recognised)
    return type(conditioner) is DAGConditioner


def _is_std_normal(dens):
    """the factories' standard-normal base density itself, nothing that merely inherits from it: a subclass that overrides
    forward (tempered / scaled / conditional density) is called as the reference calls it"""
    return bool(getattr(dens, "standard_normal", False) and getattr(type(dens), "_std_forward", None) is type(dens).forward)


def _is_zero(c):
    return isinstance(c, float) and c == 0.


def _is_device_scalar(c):
    return torch.is_tensor(c) and c.is_cuda and c.dim() == 0 and c.dtype == torch.float32


def _nll_mean(c, logdet, logn):
    """c - mean(logdet + logn) for the constraints term c: one launch where c is plain zero or a device scalar"""
    if _is_zero(c):
        return ops.NllMeanFn.apply(logdet, logn)                                 # -(logdet + logn).mean(), one launch
    if _is_device_scalar(c):
        return ops.NllMeanFn.apply(logdet, logn, c)                              # constraints - mean(...), the same launch
    return c + ops.NllMeanFn.apply(logdet, logn)


_SINGLE_STEP = ("%s: an intervention is defined on the data-side equations x_i = T^-1(z_i; h_i(x_pa(i), context)) of a "
                "ONE-step flow; the intermediate variables of a stacked or multi-scale flow are not the x_i (this flow has "
                "%d steps)")


def _index_tuple(index, d, who, must_be, twice, got):
    """a sequence of ints or an integer tensor [S] (never bool) as a tuple of unique ints in [0, d); ValueError otherwise,
    worded for the caller: `who` names the function and its argument, `must_be` what the argument may be, `twice` is the
    verb of the repeated-variable message, `got` says whether a refusal also names what came (then a non-iterable is a
    ValueError too, not the TypeError of tuple())"""
    def bad(seen=""):
        return ValueError("%s must be %s%s" % (who, must_be, ", got " + seen if got and seen else ""))
    if torch.is_tensor(index):
        if index.dim() != 1 or index.dtype.is_floating_point or index.dtype.is_complex or index.dtype == torch.bool:
            raise bad("%s %s" % (index.dtype, tuple(index.shape)))
        idx = tuple(int(i) for i in index.tolist())
    else:
        try:
            idx = tuple(index)
        except TypeError:
            if not got:
                raise
            raise bad("%r" % (type(index),)) from None
        if any(isinstance(i, bool) or not isinstance(i, int) for i in idx):
            raise bad()
    if any(i < 0 or i >= d for i in idx):
        raise ValueError("%s %s out of range for d = %d" % (who, list(idx), d))
    if len(set(idx)) != len(idx):
        raise ValueError("%s %s %s a variable twice" % (who, list(idx), twice))
    return idx


def do_arguments(do_index, do_value, z):
    """(pinned variables as a tuple of ints, their values as a [B, S] tensor like z) of an intervention on z [B, d]:
    do_index a sequence of ints or an integer tensor [S], unique and in range; do_value a float, [S] or [B, S].
    ValueError otherwise."""
    if z.dim() != 2:
        raise ValueError("intervene: z must be [B, d], got %s" % (tuple(z.shape),))
    B, d = z.shape
    idx = _index_tuple(do_index, d, "intervene: do_index", "a sequence of ints or an integer tensor [S]", "names", False)
    S = len(idx)
    if torch.is_tensor(do_value) and do_value.dim() > 0:
        if tuple(do_value.shape) not in ((S,), (B, S)):
            raise ValueError("intervene: do_value must be a float, [S] or [B, S] = [%d, %d], got %s"
                             % (B, S, tuple(do_value.shape)))
        vals = do_value.detach().to(device=z.device, dtype=z.dtype).expand(B, S).contiguous()
    elif torch.is_tensor(do_value) or isinstance(do_value, (int, float)):
        vals = torch.full((B, S), float(do_value), dtype=z.dtype, device=z.device)
    else:
        raise ValueError("intervene: do_value must be a float, [S] or [B, S], got %r" % (type(do_value),))
    return idx, vals


def _targets_known_empty(targets):
    """True when the HOST can see that nothing is pinned (an empty index list / tensor): no device value is read"""
    if torch.is_tensor(targets):
        return targets.dim() == 1 and targets.numel() == 0 and targets.dtype not in (torch.bool, torch.uint8)
    try:
        return len(targets) == 0
    except TypeError:
        return False


def do_targets(targets, regime, x, check_regime=True):
    """(pin uint8 [R, d] contiguous on x's device, regime int32 [B] on x's device or None): the mask table of the
    interventional likelihood (gnf_hip.ops.NllDoFn / AffineDoFn) for data x [B, d].  `targets`:
      a sequence of ints or an integer tensor [S] -- one target set for the whole batch, unique and in range, as the do_index
        of intervene (a uint8 tensor is always read as a MASK, never as indices);
      a bool / uint8 tensor [d]                   -- the same as a mask;
      a bool / uint8 tensor [R, d] with regime [B] (integer ids in [0, R)) -- a target set per regime;
      a bool / uint8 tensor [B, d] without a regime -- a target set per sample.
    ValueError for any other rank, width or dtype, for a regime without an [R, d] table, and for a regime id outside [0, R).
    That last check reads regime.min() / .max() -- one synchronisation on a device tensor; check_regime=False skips it for a
    caller that validated its data set once (the kernels answer a bad id with NaN rows and never index the table with it).
    A contiguous uint8 table and an int32 regime vector already on x's device are handed on as they are -- the kernels read
    any non-zero byte as pinned -- so an unchecked call costs no launch."""
    if x.dim() != 2:
        raise ValueError("do_targets: x must be [B, d], got %s" % (tuple(x.shape),))
    B, d = x.shape
    table = None
    if torch.is_tensor(targets) and targets.dtype in (torch.bool, torch.uint8):
        if targets.dim() not in (1, 2) or targets.shape[-1] != d:
            raise ValueError("do_targets: a mask of targets must be [d], [R, d] or [B, d] with d = %d, got %s"
                             % (d, tuple(targets.shape)))
        if targets.dim() == 1:
            table = targets.view(1, d)
        else:
            table = targets
            if regime is None and table.shape[0] not in (1, B):
                raise ValueError("do_targets: a [%d, d] mask without a regime vector must have B = %d rows (or one)"
                                 % (table.shape[0], B))
        if regime is not None and targets.dim() != 2:
            raise ValueError("do_targets: a regime vector needs an [R, d] table of targets, got a [d] mask")
        if table.dtype == torch.uint8 and table.device == x.device and table.is_contiguous():
            pin = table                                 # the kernels read any non-zero byte as pinned: no launch, no copy
        else:
            pin = (table != 0).to(device=x.device, dtype=torch.uint8).contiguous()
    else:
        if regime is not None:
            raise ValueError("do_targets: a regime vector needs a bool / uint8 [R, d] table of targets")
        idx = _index_tuple(targets, d, "do_targets: targets",       # (a bool / uint8 tensor is a mask: it never gets here)
                           "a sequence of ints, an integer tensor [S] or a bool / uint8 mask", "name", True)
        host = torch.zeros(1, d, dtype=torch.uint8)
        if idx:
            host[0, list(idx)] = 1
        pin = host.to(x.device)
    if regime is None:
        return pin, None
    if (not torch.is_tensor(regime) or regime.dim() != 1 or regime.shape[0] != B or regime.dtype.is_floating_point
            or regime.dtype.is_complex or regime.dtype == torch.bool):
        raise ValueError("do_targets: regime must be an integer tensor [B] = [%d], got %s"
                         % (B, (regime.dtype, tuple(regime.shape)) if torch.is_tensor(regime) else type(regime)))
    R = pin.shape[0]
    if check_regime and B > 0:
        lo, hi = int(regime.min()), int(regime.max())
        if lo < 0 or hi >= R:
            raise ValueError("do_targets: regime ids span [%d, %d], the table has R = %d rows" % (lo, hi, R))
    return pin, regime.to(device=x.device, dtype=torch.int32).contiguous()


class NormalizingFlow(nn.Module):
    """Protocol shared by all flows.  forward(x, context=None) -> (z, log|det J|).  The aggregate queries have
    default implementations in terms of getConditioners(), which every concrete flow provides."""

    def __init__(self):
        super().__init__()

    def forward(self, x, context=None):
        raise NotImplementedError

    def invert(self, z, context=None):
        raise NotImplementedError

    def rsample(self, z, context=None):
        """invert(z, context) as a differentiable function of z, the context and the parameters"""
        raise NotImplementedError

    def intervene(self, z, do_index, do_value, context=None):
        """x under do(x[:, do_index] = do_value): the pinned equations replaced by constants, every other one kept"""
        raise NotImplementedError

    def counterfactual(self, x, do_index, do_value, context=None):
        """what the observation x would have been under do(x[:, do_index] = do_value): abduct z = forward(x), intervene"""
        raise NotImplementedError

    def rsample_do(self, z, do_index, do_value, context=None):
        """intervene(...) as a differentiable function of z, do_value (a tensor that requires grad), the context and the
        parameters"""
        raise NotImplementedError

    def rcounterfactual(self, x, do_index, do_value, context=None):
        """counterfactual(...) as a differentiable function of x, do_value, the context and the parameters"""
        raise NotImplementedError

    def getConditioners(self):
        raise NotImplementedError

    def getNormalizers(self):
        raise NotImplementedError

    def constraintsLoss(self):
        total = None                                    # (sum(..., 0.) of the reference: 0. + loss is one more launch)
        for c in self.getConditioners():
            if _is_dag(c):
                total = c.loss() if total is None else total + c.loss()
        return 0. if total is None else total

    def DAGness(self):
        return [c.get_power_trace() if _is_dag(c) else 0. for c in self.getConditioners()]

    def step(self, epoch_number, loss_avg):
        for c in self.getConditioners():
            if _is_dag(c):
                c.step(epoch_number, loss_avg)

    def isInvertible(self):
        return all(c.is_invertible for c in self.getConditioners())


class NormalizingFlowStep(NormalizingFlow):
    """One autoregressive-style transformation.  A normalizer that offers `forward_logdet` returns the row-summed
    log-Jacobian itself: the Affine normalizer from the kernel that computes z (log-det and Normal log-density reduced
    in the same pass), the Monotonic one from a single fused reduction pass over its (z, jac) (its integrand kernels
    spread a row over many wavefronts); any other Normalizer plug-in goes through the log + row-sum reduction kernel."""

    def __init__(self, conditioner: Conditioner, normalizer: Normalizer):
        super().__init__()
        self.conditioner = conditioner
        self.normalizer = normalizer
        self.level_schedule = True       # invert(): topological level schedule for DAG conditioners
        self.graph_invert = True         # ... replayed as a hipGraph from the second pass of a shape on (frozen A, GPU)
        self.column_schedule = True      # invert(): one column per step for MADE conditioners, every hidden unit once
        self.adjoint_schedule = True     # rsample() backward: the transposed column sweep for MADE conditioners, one launch

    def getConditioners(self):
        return [self.conditioner]

    def getNormalizers(self):
        return [self.normalizer]

    def forward(self, x, context=None):
        h = self.conditioner(x, context)
        fused = getattr(self.normalizer, "forward_logdet", None)
        if fused is not None:
            return fused(x, h, context)
        z, jac = self.normalizer(x, h, context)
        return z, ops.LogSumRowsFn.apply(jac)

    def forward_do(self, x, targets, regime=None, context=None, check_regime=True):
        """(z, logdet, logn) of x under do(x_S): z = forward's z for every column, logdet[b] = sum over the FREE variables of
        log|dz_i/dx_i| and logn[b] = sum over the free variables of log N(z_i) -- the truncated factorisation
        log p(x | do(x_S)) = logdet + logn (interventional likelihood).  The pinned values still feed their
        children's conditioners; their own terms never enter a sum or a gradient.  targets / regime: do_targets.  All three
        results are differentiable; this is the training path, so a stochastic DAG gate is allowed.

        The Affine normalizer reduces in the kernel that writes z (ops.AffineDoFn); every other normalizer runs as in
        forward and ops.NllDoFn reduces its (z, jac).  Targets the HOST knows to be empty ([] or an empty index tensor)
        take forward itself and the unmasked Normal log-density, bit for bit."""
        if regime is None and _targets_known_empty(targets):
            if x.dim() != 2:
                raise ValueError("do_targets: x must be [B, d], got %s" % (tuple(x.shape),))
            z, logdet = self.forward(x, context)
            return z, logdet, ops.NormalLogDensityFn.apply(z)
        pin, reg = do_targets(targets, regime, x, check_regime)
        h = self.conditioner(x, context)
        fused = getattr(self.normalizer, "forward_logdet_do", None)
        if fused is None:                               # a plug-in that does not derive from Normalizer: the base method on it
            return Normalizer.forward_logdet_do(self.normalizer, x, h, pin, reg, context)
        return fused(x, h, pin, reg, context)

    # -- inversion ----------------------------------------------------------------------------------------------
    DO_LEVELS_MAX = 8                    # mutilated level schedules kept per step (pinned tuples of one gate)

    def _levels(self, importance, idx=()):
        """(levels, (all rows, int32 rows per level)) of the current gate under do(x_idx), or None for a cyclic graph: the
        pinned variables lose their parents (their rows of the importance matrix zeroed) and leave the level lists; levels
        that held only pinned variables vanish.  idx = (): the schedule of invert.

        Recomputed only when A (storage or version counter) or the gate's thresholds changed: DAGConditioner.levels() is a
        host synchronisation in front of every sampling pass otherwise.  With `device_graph` it is two launches
        (gnf_hip.ops.dag_levels), a sort and one copy of 2 d + 3 integers; without it the d x d adjacency goes to the host
        and is walked in Python (5 ms against 0.9 at 784 x 784, 39 .. 427 ms against 1.6 .. 15 at d = 3072:
        profiles/dag_graph_ab.txt).  The un-pinned schedule is held alone in `_levels_own` -- the captured graphs of invert
        replay it, so no intervention may evict it -- and the mutilated ones in `_levels_do`, at most DO_LEVELS_MAX."""
        cond = self.conditioner
        # A trainable A is rewritten by the optimiser through a raw pointer (gnf_hip.dp: fused Adam on the flat buffer, a
        # replayed hipGraph), which moves neither its version counter nor its address: nothing is cached for it.  A frozen
        # one is keyed on (storage, version, thresholds, the conditioner's cache epoch -- see invalidate_caches()).
        key = (None if cond.A.requires_grad else
               (cond.A.data_ptr(), cond.A._version, float(cond.h_thresh), bool(cond.s_thresh), cond.A.device,
                getattr(cond, "_cache_epoch", 0), tuple(sorted(idx))))
        cache, own = self.__dict__.setdefault("_levels_do", {}), self.__dict__.get("_levels_own")
        if key is not None and idx and key in cache:
            return cache[key]
        if key is not None and not idx and own is not None and own[0] == key:
            return own[1]
        cut = importance
        if idx:
            cut = importance.detach().clone()
            cut[list(idx)] = 0
        lv = cond.levels(cut, with_host=True)
        entry = None
        if lv is not None:
            # the order of the variables INSIDE a level is free: for a 28 x 28 image take the one the sparse embedding kernels
            # work in (crop origin, then pixel), so that their output needs no un-sorting gather
            pinned, crop, out = set(idx), cond.A.shape[0] == 784, []
            for rows, host in lv:
                keep = tuple(r for r in host if r not in pinned)
                if crop:
                    keep = _crop_order(keep)
                if keep:
                    out.append((rows if keep == host else torch.as_tensor(keep, dtype=torch.long, device=rows.device), keep))
            # one gather of z per pass, and the scatter tables of the inverse
            entry = (out, (torch.cat([rows for rows, _ in out]), [rows.to(torch.int32) for rows, _ in out]) if out else
                     (None, None))
        if not idx:
            self._levels_own = None if key is None else (key, entry)
            _INV_GRAPHS.pop(self, None)                 # graphs captured for another gate replay another schedule
        elif key is not None:
            if len(cache) >= self.DO_LEVELS_MAX:
                cache.clear()
            cache[key] = entry
        return entry

    def _invert_levels_body(self, z, levels, importance, context, tables, x=None):
        """variable-major inside: z is gathered ONCE into [sum of level sizes, B] (a level is a contiguous slice), the
        conditioner rows come as [R, B, out] -- the layout the sparse kernels write -- and the normalizer's inverse is
        element-wise in whatever two leading dimensions z and h share.  Per level that leaves the embedding front, the
        inverse and one scatter into x (no gather of z, no un-sorting or permuting copy of h).  tables: the second half of
        `_levels`' answer for these levels; x: the start of an intervention, pinned columns filled."""
        cond = self.conditioner
        x = torch.zeros_like(z) if x is None else x
        all_rows, rows32 = tables
        zt = z.t()[all_rows]                                                  # [sum R, B], contiguous
        off = 0
        into = getattr(self.normalizer, "inverse_transform_into", None)       # (the normalizers ignore the context)
        for k, (rows, host_rows) in enumerate(levels):
            R = rows.numel()
            h = cond.forward_rows(x, rows, importance, host_rows, variable_major=True, rows32=rows32[k],
                                  **({} if context is None else {"context": context}))
            # the normalizer writes its [R, B] result into columns `rows` of x itself where it can
            if into is None or not into(zt[off:off + R], h, x, rows32[k]):
                x[:, rows] = self.normalizer.inverse_transform(zt[off:off + R], h, context).t()
            off += R
        return x

    GRAPH_INVERT_MAX = 8                 # captured (batch shape, node count) variants kept per step

    def _holders(self):
        """objects that can build parameter-only images ONCE for a whole inversion (attribute name, context factory):
        the normalizer's packed integrand weights, the embedding net's sparse-front tables"""
        out = []
        if getattr(self.normalizer, "hold_pack", None) is not None:
            out.append((self.normalizer, "_held_pack", self.normalizer.hold_pack))
        net = getattr(self.conditioner, "embedding_net", None)
        if getattr(net, "hold_prepared", None) is not None:
            out.append((net, "_held_prep", net.hold_prepared))
        return out

    def _fast_arm(self, z, context):
        """which schedule inverts (z, context), and with what: ("levels", importance, checked context) for a DAG conditioner
        with a deterministic gate (`level_schedule`), ("columns", plan, checked contiguous context) for a MADE whose masks
        are its degree rule (`column_schedule`; the plan is None for an empty batch, which needs none), ("strade", level plan,
        checked contiguous context) for a StrADE conditioner whose masks are the rule's masks for its adjacency, under an
        Affine or Spline normalizer (the same switch, `column_schedule`: False sends MADE and StrADE alike to the passes), None
        for the fixed-point passes.  A conditioner built with cond_in > 0 has its context checked first -- ValueError: missing, wrong
        width / rank / rows; one with cond_in = 0 that is given a context goes to the passes, which raise what it raises."""
        cond = self.conditioner
        cond_in = int(getattr(cond, "cond_in", 0) or 0)
        if not cond_in and context is not None:
            return None
        if _is_dag(cond) and self.level_schedule:
            ctx = checked_context(context, cond_in, z) if cond_in else context
            if not cond_in or (z.dim() == 2 and ctx.device == z.device and ctx.dtype == z.dtype):
                importance = cond.deterministic_importance()
                if importance is not None:
                    return "levels", importance, ctx
        get_plan, get_levels = getattr(cond, "prefix_plan", None), getattr(cond, "level_plan", None)
        if not (self.column_schedule and (get_plan is not None or get_levels is not None) and z.is_cuda and z.dim() == 2
                and z.dtype == torch.float32):
            return None
        if get_plan is None and type(self.normalizer) not in (AffineNormalizer, SplineNormalizer):
            return None                                 # the level kernel inverts in its epilogue: these two or the passes
        if cond_in:
            context = checked_context(context, cond_in, z)
            if context.device != z.device or context.dtype != torch.float32:
                return None
            context = context.contiguous()
        name = "columns" if get_plan is not None else "strade"
        if z.shape[0] == 0:
            return name, None, context
        if get_plan is None:
            plan = get_levels()
        else:
            plan = get_plan(with_context=True) if cond_in else get_plan()
        return (name, plan, context) if plan is not None and plan["d"] == z.shape[1] else None

    def _invert_by_levels(self, z, importance, context, idx=(), vals=None, capture=False):
        """DAG conditioner with a deterministic gate: every variable is inverted once, after its parents -- d
        conditioner rows in total instead of (depth + 1) * d.  Same values as the fixed-point passes (non-parents are
        masked by exact zeros either way).  Returns None for a cyclic graph.

        Under do(x_idx = vals) it is the schedule of the mutilated graph: x[:, idx] = vals is written before the first
        level, then the remaining rows run -- fewer conditioner rows and no more levels than invert needs.

        A conditioner built with cond_in > 0 takes its (checked) context along: every level's rows are completed with
        context[b] by the DAGMLP, on the composed formulation, launch by launch (no graph is captured for such a pass).

        capture (invert alone, never an intervention): on the GPU the pass of a given (gate, batch shape, node count) is
        captured into a hipGraph the second time it is asked for and replayed from then on (`graph_invert`): with a frozen
        A the schedule, the row tables and the sparse plans are static, and a sampling pass over MNIST is ~650 launches of
        5-100 us (reference ImageExperiments.py:341-350 samples after post_process()).  The weight image of the normalizer
        is packed INSIDE the graph, so a replay reads the current parameters."""
        cond = self.conditioner
        entry = self._levels(importance, idx)
        if entry is None:
            return None
        levels, tables = entry
        if not capture:                                 # launch by launch; invert's graphs are neither read nor added to
            x = torch.zeros_like(z)
            if idx:
                x[:, list(idx)] = vals
            if z.shape[0] == 0 or not levels:
                return x
            return self._invert_levels_body(z, levels, importance, context, tables, x=x)
        if context is not None and z.shape[0] == 0:
            return torch.zeros_like(z)                  # no rows, no launch (as the column schedule answers an empty batch)
        # a captured pass bakes the ADDRESS of the importance matrix in: only A itself qualifies -- the thresholded forms
        # (s_thresh / h_thresh > 0, the state the reference's threshold sweep sets) are temporaries freed after this call
        graphable = (self.graph_invert and context is None and z.is_cuda and not cond.A.requires_grad
                     and z.dtype == torch.float32 and importance.data_ptr() == cond.A.data_ptr()
                     and len(levels) > 4 and not torch.cuda.is_current_stream_capturing())
        if not graphable:
            return self._invert_levels_body(z, levels, importance, context, tables)
        # what a captured pass bakes in: shapes, the node count, the front, and the ADDRESSES of every parameter and buffer
        # (values may change freely; a re-bound or moved tensor must not be read through a stale pointer)
        key = (tuple(z.shape), int(getattr(self.normalizer, "nb_steps", 0)), bool(getattr(cond, "sparse_front", False)),
               bool(getattr(getattr(cond, "embedding_net", None), "rows_front", False)),
               bool(getattr(getattr(cond, "embedding_net", None), "gated_front", False)),
               tuple(t.data_ptr() for t in self.parameters()), tuple(t.data_ptr() for t in self.buffers()))
        graphs = _INV_GRAPHS.setdefault(self, {})
        entry = graphs.get(key)
        if entry is None:                               # first request: eager (workspaces, plans and tables come to exist)
            graphs[key] = "warm"
            return self._invert_levels_body(z, levels, importance, context, tables)
        if entry == "eager":                            # a capture of this variant failed once: launch by launch from then on
            return self._invert_levels_body(z, levels, importance, context, tables)
        if entry == "warm":
            import gc
            zbuf = z.clone()
            import contextlib
            holders = self._holders()
            saved = [(obj, attr, getattr(obj, attr)) for obj, attr, _ in holders]
            for obj, attr, _ in holders:                # the build launches belong INTO the graph (current parameters on replay)
                setattr(obj, attr, None)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):               # once on the capture stream's allocator pool
                with contextlib.ExitStack() as stack:
                    for _, _, make in holders:
                        stack.enter_context(make())
                    self._invert_levels_body(zbuf, levels, importance, context, tables)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            gc_was_on = gc.isenabled()
            gc.collect()
            gc.disable()                                # no finaliser may run inside the capture
            failed = None
            try:
                with torch.cuda.graph(graph), contextlib.ExitStack() as stack:
                    for _, _, make in holders:
                        stack.enter_context(make())
                    xbuf = self._invert_levels_body(zbuf, levels, importance, context, tables)
            except Exception as exc:                    # noqa: BLE001  (e.g. a host synchronisation inside a user-supplied
                failed = exc                            # integrand / embedding module): this variant stays eager
            finally:
                if gc_was_on:
                    gc.enable()
                for obj, attr, val in saved:
                    setattr(obj, attr, val)
            if failed is not None:
                import warnings
                warnings.warn("NormalizingFlowStep.invert: hipGraph capture of the level schedule failed (%r); this variant "
                              "runs eagerly from now on" % (failed,), RuntimeWarning, stacklevel=2)
                graphs[key] = "eager"
                torch.cuda.synchronize()
                return self._invert_levels_body(z, levels, importance, context, tables)
            if len(graphs) > self.GRAPH_INVERT_MAX:
                graphs.clear()
            entry = graphs[key] = (graph, zbuf, xbuf)
        graph, zbuf, xbuf = entry
        zbuf.copy_(z, non_blocking=True)
        graph.replay()
        return xbuf.clone()

    def _invert_by_columns(self, z, plan, context, idx=(), vals=None):
        """MADE conditioner: the variables are inverted in degree order, one per step, and a step evaluates only the hidden
        units that became final with the previous column (AutoregressiveConditioner.prefix_plan) -- about half of ONE masked
        forward and ONE normalizer inverse in total, where the passes below spend depth() + 1 = d of each.  The same function
        in another fp32 summation order.

        A conditional MADE (cond_in > 0) is inverted the same way from its conditional plan (prefix_plan(with_context=True)):
        the checked context heads the kernel's activation rows, the conditioner module is never called.

        Under do(x_idx = vals) the sweep takes a pin table (gnf_made_prefix_do): x[:, idx] = vals is written first, and a
        pinned step reads its column instead of computing it.  Affine / Spline + MADE are ONE launch either way; any other
        normalizer is stepped through made_do_launches: one launch per FREE column, which advances through the run of pinned
        degrees in front of it, and none for a trailing run -- (t, t + 1) for every t when nothing is pinned."""
        cond = self.conditioner
        if z.shape[0] == 0:
            # no rows, no launch: the empty result (the passes would stop at the MADE's `.view(0, -1, d)` as the reference's do)
            return torch.zeros_like(z)
        kw = {} if context is None else {"context": context}
        z = z.contiguous()
        x = torch.zeros_like(z)
        B, d, out = z.shape[0], plan["d"], plan["out"]
        if idx:
            x[:, list(idx)] = vals
            if len(idx) == d:
                return x                                # every degree is a trailing pinned one: no launch
            pin = kw["pin"] = torch.zeros(d, dtype=torch.uint8, device=z.device)
            pin[list(idx)] = 1
        with cond.hold_prefix_pack():
            if type(self.normalizer) is AffineNormalizer:
                # the whole inversion, one launch
                cond.prefix_steps(z, x, 0, d, ops.MADE_NORM_AFFINE, **kw)
                return x
            if type(self.normalizer) is SplineNormalizer:
                # likewise: the spline's closed-form inverse is the kernel's per-row epilogue
                cond.prefix_steps(z, x, 0, d, ops.MADE_NORM_SPLINE, spline=(self.normalizer.nb_bins, self.normalizer.tail_bound),
                                  **kw)
                return x
            h = torch.empty(B, out, dtype=torch.float32, device=z.device)
            ws = cond.prefix_workspace(B)
            zt = z.t().contiguous()                                          # a column of z as a one-row [1, B] problem
            cols = torch.arange(d, dtype=torch.int32, device=z.device)
            into = getattr(self.normalizer, "inverse_transform_into", None)
            for t0, t1 in made_do_launches(plan["var_host"], idx):
                v = plan["var_host"][t1 - 1]            # the launch's one free column, behind t1 - 1 - t0 pinned ones
                cond.prefix_steps(z, x, t0, t1, ops.MADE_NORM_NONE, h_out=h, ws=ws, **kw)
                # the normalizer's own inverse of that one column; the fused Monotonic kernel writes x[:, v] itself
                if into is None or not into(zt[v:v + 1], h.view(1, B, out), x, cols[v:v + 1]):
                    x[:, v:v + 1] = self.normalizer.inverse_transform(z[:, v:v + 1], h.view(B, 1, out), context)
        return x

    def _invert_by_strade(self, z, plan, context, idx=(), vals=None):
        """StrADE conditioner (a masked net over a given DAG) with an Affine or Spline normalizer: the variables are inverted
        level by level in ONE launch (StrADEConditioner.level_sweep, gnf_strade_levels), every hidden unit computed once,
        when the variables of its parent set are known -- where the passes below spend depth() + 1 masked forwards and
        normalizer inverses.  The same function in another fp32 summation order.  The conditioner module is never called;
        a context heads the kernel's activation rows.

        Under do(x_idx = vals) the sweep takes a pin table: x[:, idx] = vals is written first, a pinned variable keeps its
        level and its column is read instead of computed.  Returns None, having launched nothing, when the net's rows do not
        fit the kernel's LDS tile: the passes serve."""
        cond = self.conditioner
        if z.shape[0] == 0:
            return torch.zeros_like(z)                  # no rows, no launch
        kw = {} if context is None else {"context": context}
        z = z.contiguous()
        x = torch.zeros_like(z)
        d = plan["d"]
        if idx:
            x[:, list(idx)] = vals
            if len(idx) == d:
                return x                                # no free equation: no launch
            pin = kw["pin"] = torch.zeros(d, dtype=torch.uint8, device=z.device)
            pin[list(idx)] = 1
        if type(self.normalizer) is SplineNormalizer:
            kw["spline"] = (self.normalizer.nb_bins, self.normalizer.tail_bound)
            mode = ops.MADE_NORM_SPLINE
        else:
            mode = ops.MADE_NORM_AFFINE
        with cond.hold_level_pack():
            return cond.level_sweep(z, x, mode, **kw)

    def _invert_by_passes(self, z, context, idx=(), vals=None):
        """Reference :98-107: fixed point of x <- normalizer^-1(z, conditioner(x)) from x = 0, depth() + 1 passes, early exit
        once a pass changes nothing (its progress print is dropped).  Under do(x_idx = vals):
        x <- where(pinned, vals, normalizer^-1(z, conditioner(x))) from where(pinned, vals, 0), on the un-mutilated graph --
        the mutilated one is never deeper."""
        cols = list(idx)
        x = torch.zeros_like(z)
        if cols:
            x[:, cols] = vals
            if len(cols) == z.shape[1]:
                return x                                # no free equation: the conditioner is never asked
        for _ in range(self.conditioner.depth() + 1):
            previous = x
            x = self.normalizer.inverse_transform(z, self.conditioner(x, context), context)
            if cols:
                x[:, cols] = vals
            if torch.equal(x, previous):
                break
        return x

    def _by_schedule(self, z, context, idx=(), vals=None, capture=False):
        """(x, arm) from the schedule `_fast_arm` names, or (None, "passes") where none applies.  capture: `_invert_by_levels`"""
        arm = self._fast_arm(z, context)
        if arm is not None and arm[0] == "columns":
            return self._invert_by_columns(z, arm[1], arm[2], idx, vals), "columns"
        if arm is not None and arm[0] == "strade":
            x = self._invert_by_strade(z, arm[1], arm[2], idx, vals)
            return x, ("passes" if x is None else "strade")
        x = None if arm is None else self._invert_by_levels(z, arm[1], arm[2], idx, vals, capture)
        return x, ("passes" if x is None else "levels")

    def invert(self, z, context=None):
        """x with forward(x, context) = z: by levels (DAG), by columns (MADE), or by the reference's fixed-point passes"""
        with torch.no_grad(), contextlib.ExitStack() as stack:   # parameters do not change inside: build their images once
            for _, _, make in self._holders():
                stack.enter_context(make())
            x, _ = self._by_schedule(z, context, capture=True)
            return self._invert_by_passes(z, context) if x is None else x

    # -- interventions ------------------------------------------------------------------------------------------
    def _refuse_stochastic_gate(self, what, why):
        cond = self.conditioner
        if _is_dag(cond) and cond.deterministic_importance() is None:
            raise ValueError("NormalizingFlowStep.%s: the DAG conditioner's gate is stochastic (stoch_gate / noise_gate); %s.  "
                             "Use a deterministic gate (stoch_gate = noise_gate = False)" % (what, why))

    _EVERY_DRAW = "every evaluation of the conditioner would draw another graph than the one the intervention cuts"

    def intervene(self, z, do_index, do_value, context=None):
        """x under do(x[:, do_index] = do_value) (interventions):  x[b, i] = do_value[b, i] exactly for a pinned
        i, x[b, i] = normalizer^-1(z[b, i], conditioner(x, context)[b, i]) for every other; z[:, do_index] is ignored.  An
        empty do_index is invert(z, context), bit for bit.  Three arms on invert's conditions (`level_schedule`,
        `column_schedule`), recorded in `_intervene_arm`: "levels" (DAG), "columns" (MADE), "strade" (StrADE, Affine / Spline),
        "passes" (anything, anywhere).
        Launch by launch: no graph is captured, and invert's schedule and its captured graphs are not touched.

        A DAG conditioner with a stochastic or noisy gate is refused as rsample refuses it: every pass and every level
        would draw another graph to mutilate."""
        self._refuse_stochastic_gate("intervene", self._EVERY_DRAW)
        idx, vals = do_arguments(do_index, do_value, z)
        self._intervene_arm = None
        with torch.no_grad(), contextlib.ExitStack() as stack:
            for _, _, make in self._holders():
                stack.enter_context(make())
            x, self._intervene_arm = self._by_schedule(z, context, idx, vals)
            return self._invert_by_passes(z, context, idx, vals) if x is None else x

    def counterfactual(self, x, do_index, do_value, context=None):
        """abduction, then action: z = forward(x, context), then intervene(z, ...).  No column is copied from x: what a
        non-descendant of the pinned variables comes back as is the inversion's own residual."""
        self._refuse_stochastic_gate("intervene", self._EVERY_DRAW)
        do_arguments(do_index, do_value, x)             # (the argument errors before the abduction's launches)
        with torch.no_grad():
            z, _ = self.forward(x, context)
        return self.intervene(z, do_index, do_value, context)

    # -- differentiable sampling --------------------------------------------------------------------------------
    def rsample(self, z, context=None):
        """x = invert(z, context) -- the same kernels, the same bits -- with gradients for z, the context and the step's
        parameters from the implicit function theorem (rsample).  With J = dz/dx of the step at the sample and
        a cotangent g = dL/dx:  J^T lambda = g,  dL/dz = lambda,  dL/dtheta = -(dS/dtheta)^T lambda, dL/dc likewise: one
        transposed triangular solve and one vjp of the forward, instead of a backward through depth() + 1 passes.

        A DAG conditioner with a stochastic or noisy gate is refused: the backward re-evaluates the conditioner at the
        sample, and would draw another gate than the one the sample saw."""
        self._refuse_stochastic_gate("rsample", "the backward would recompute the conditioner under another draw of the gate "
                                     "than the sample saw")
        return ops.InvertFn.apply(self, z, context, *[p for p in self.parameters() if p.requires_grad])

    def _adjoint_plan(self, x, context):
        """the MADE plan of the adjoint arm when `_fast_arm` names the column sweep for this sample (and `adjoint_schedule`,
        and the conditioner can solve), else None: the passes arm.  Never raises: a context that `_fast_arm` would refuse
        answers None as a missing one does.  A StrADE conditioner with `adjoint_levels` on answers its level plan, whatever
        the normalizer and however the sample was inverted: the solve reads jac and dz/dh alone."""
        cond = self.conditioner
        cond_in = int(getattr(cond, "cond_in", 0) or 0)
        if not (self.adjoint_schedule and getattr(cond, "adjoint_solve", None) is not None
                and bool(cond_in) == (context is not None)):
            return None
        if getattr(cond, "prefix_plan", None) is None:
            if not (getattr(cond, "adjoint_levels", False) and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32):
                return None
            if context is not None and (context.device != x.device or context.dtype != torch.float32
                                        or tuple(context.shape) != (x.shape[0], cond_in)):
                return None
            plan = cond.level_plan()
            return plan if plan is not None and plan["d"] == x.shape[1] else None
        try:
            arm = self._fast_arm(x, context)
        except ValueError:
            return None
        return arm[1] if arm is not None and arm[0] == "columns" else None

    def _rsample_backward(self, x, context, params, g, want_context):
        """(lambda, dL/dcontext, [dL/dp for p in params]) of ops.InvertFn for the sample x and the cotangent g = dL/dx"""
        self._rsample_arm = None                        # which arm the last backward took, and its vjps through the step
        if x.shape[0] == 0:
            return torch.zeros_like(x), None, [None] * len(params)
        want_context = bool(want_context and context is not None)
        with torch.enable_grad():
            # two leaves of the same values: grad(z, xa) is N^T lambda alone (the conditioner's path), the diagonal of J is
            # the normalizer's own jac -- no J^T lambda - D lambda cancellation
            xa, xb = x.detach().requires_grad_(True), x.detach()
            ctx = context.detach().requires_grad_(True) if want_context else context
            h = self.conditioner(xa, ctx)
            zz, jac = self.normalizer(xb, h, ctx)
        jac = jac.detach()
        plan = self._adjoint_plan(x, context)
        if plan is not None:
            # the normalizers are element-wise: one backward with a cotangent of ones is dz_bi/dh_bi
            dzdh, = torch.autograd.grad(zz, h, torch.ones_like(zz), retain_graph=True)
            lam = self.conditioner.adjoint_solve(x.contiguous(), g, jac.contiguous(), dzdh.contiguous(),
                                                 **({} if context is None else {"context": context.detach().contiguous()}))
            self._rsample_arm = ("adjoint", 0)
        else:
            # exact by nilpotency: N^(depth + 1) = 0
            lam, n = g / jac, 0
            for _ in range(self.conditioner.depth()):
                nl, = torch.autograd.grad(zz, xa, lam, retain_graph=True, allow_unused=True)
                n += 1
                new = g / jac if nl is None else (g - nl) / jac
                same = torch.equal(new, lam)
                lam = new
                if same:
                    break
            self._rsample_arm = ("passes", n)
        wrt = list(params) + ([ctx] if want_context else [])
        grads = list(torch.autograd.grad(zz, wrt, -lam, allow_unused=True)) if wrt else []
        gctx = grads.pop() if want_context else None
        return lam, gctx, grads

    # -- differentiable interventional sampling -----------------------------------------------------------------
    def rsample_do(self, z, do_index, do_value, context=None):
        """x = intervene(z, do_index, do_value, context) -- the same arm (recorded in `_intervene_arm`), the same bits --
        with gradients for z, do_value, the context and the step's parameters (rsample under an intervention).
        The equations of the free variables F are kept, those of the pinned variables P read x_P = v.  With J = D + N at the
        sample and g = dL/dx:  lambda_P = 0,  J_FF^T lambda_F = g_F,  dL/dz = lambda (exact zeros at the pinned columns),
        dL/dv = g_P - (N^T lambda)_P,  dL/dtheta and dL/dc one vjp of the forward with cotangent -lambda.  Pinned
        quantities are selected, never multiplied away: the normalizer is not evaluated at a pinned element.

        do_value: a float (no gradient), or a tensor -- 0-dim, [S] or [B, S]; when it requires grad, its gradient comes
        back in its own shape.  An empty do_index is rsample(z, context): the same bits, forward and backward.  The
        backward's arm is recorded in `_rsample_arm` as rsample records it.  A stochastic DAG gate is refused."""
        self._refuse_stochastic_gate("rsample_do", "the backward would recompute the conditioner under another draw of the "
                                     "gate than the sample saw")
        idx, vals = do_arguments(do_index, do_value.detach() if torch.is_tensor(do_value) else do_value, z)
        if torch.is_tensor(do_value) and do_value.requires_grad:
            # the value path, not detached: autograd's expand reduces the gradient to do_value's own shape
            vals = do_value.to(device=z.device, dtype=z.dtype).expand(z.shape[0], len(idx))
        return ops.InterveneFn.apply(self, z, idx, vals, context, *[p for p in self.parameters() if p.requires_grad])

    def rcounterfactual(self, x, do_index, do_value, context=None):
        """counterfactual(x, do_index, do_value, context), bit for bit, differentiable: the abduction z = forward(x, context)
        WITH grad, then rsample_do.  Gradients reach x and, through the abduction too, the parameters and the context."""
        self._refuse_stochastic_gate("rsample_do", "the backward would recompute the conditioner under another draw of the "
                                     "gate than the sample saw")
        do_arguments(do_index, do_value, x)             # (the argument errors before the abduction's launches)
        z, _ = self.forward(x, context)
        return self.rsample_do(z, do_index, do_value, context)

    def _rsample_do_backward(self, x, context, params, g, idx, want_context, want_value):
        """(lambda, dL/dvals [B, S] or None, dL/dcontext, [dL/dp for p in params]) of ops.InterveneFn for the sample x under
        do(x[:, idx] = vals) and the cotangent g = dL/dx"""
        cols = list(idx)
        if not cols:
            lam, gctx, grads = self._rsample_backward(x, context, params, g, want_context)
            return lam, (g[:, :0] if want_value else None), gctx, grads
        self._rsample_arm = None
        B, d = x.shape
        if B == 0:
            return torch.zeros_like(x), (g[:, cols] if want_value else None), None, [None] * len(params)
        if len(cols) == d:
            # no free equation: nothing depends on z, the context or a parameter, and x = vals
            self._rsample_arm = ("passes", 0)
            return torch.zeros_like(x), (g[:, cols] if want_value else None), None, [None] * len(params)
        want_context = bool(want_context and context is not None)
        pin = torch.zeros(d, dtype=torch.uint8, device=x.device)
        pin[cols] = 1
        pinned = pin.bool()
        with torch.enable_grad():
            xa, xb = x.detach().requires_grad_(True), x.detach()
            ctx = context.detach().requires_grad_(True) if want_context else context
            h = self.conditioner(xa, ctx)
            # the normalizer never sees a pinned element: benign detached stand-ins there, chosen by selection, so that the
            # pinned columns of h receive an exactly zero cotangent whatever the normalizer's derivatives would be at vals
            hs = torch.where(pinned.view(1, d, 1), torch.zeros_like(h), h)
            zz, jac = self.normalizer(torch.where(pinned, torch.zeros_like(xb), xb), hs, ctx)
        jac = jac.detach()
        zero = torch.zeros_like(g)
        plan = self._adjoint_plan(x, context)
        gdo = None
        if plan is not None:
            dzdh, = torch.autograd.grad(zz, hs, torch.ones_like(zz), retain_graph=True)
            kw = {} if context is None else {"context": context.detach().contiguous()}
            res = self.conditioner.adjoint_solve(x.contiguous(), g, jac.contiguous(), dzdh.contiguous(), pin=pin,
                                                 want_gdo=bool(want_value), **kw)
            lam, gdo = res if want_value else (res, None)
            self._rsample_arm = ("adjoint", 0)
        else:
            # lambda <- where(pinned, 0, (g - N^T lambda) / jac): exact by nilpotency, as in _rsample_backward
            lam, n, nl, confirmed = torch.where(pinned, zero, g / jac), 0, None, False
            for _ in range(self.conditioner.depth()):
                nl, = torch.autograd.grad(zz, xa, lam, retain_graph=True, allow_unused=True)
                n += 1
                new = torch.where(pinned, zero, (g if nl is None else g - nl) / jac)
                confirmed = torch.equal(new, lam)       # then nl is N^T lambda of the lambda returned
                lam = new
                if confirmed:
                    break
            if want_value:
                if not confirmed:
                    nl, = torch.autograd.grad(zz, xa, lam, retain_graph=True, allow_unused=True)
                gdo = g if nl is None else g - nl
            self._rsample_arm = ("passes", n)
        wrt = list(params) + ([ctx] if want_context else [])
        grads = list(torch.autograd.grad(zz, wrt, -lam, allow_unused=True)) if wrt else []
        gctx = grads.pop() if want_context else None
        return lam, (gdo[:, cols] if want_value else None), gctx, grads


class FCNormalizingFlow(NormalizingFlow):
    """Steps applied in sequence on flat [B, d] data."""

    def __init__(self, steps, z_log_density):
        super().__init__()
        self.steps = nn.ModuleList(steps)
        self.z_log_density = z_log_density

    def getConditioners(self):
        return [c for s in self.steps for c in s.getConditioners()]

    def getNormalizers(self):
        return [n for s in self.steps for n in s.getNormalizers()]

    def forward(self, x, context=None):
        logdet = None
        last = len(self.steps) - 1
        for k, flow_step in enumerate(self.steps):
            z, ld = flow_step(x, context)
            logdet = ld if logdet is None else logdet + ld      # (the reference's 0. + ld is one more launch)
            if k < last:
                x = torch.flip(z, dims=[1])      # the reference's z[:, inv_idx] (:120-123)
        return z, logdet                         # the last step's z is returned un-flipped (:126)

    def loss(self, z, jac):
        dens = self.z_log_density
        fused = (z.is_cuda and jac.is_cuda and jac.dim() == 1 and z.dim() == 2 and jac.shape[0] == z.shape[0]
                 and z.dtype == torch.float32 and jac.dtype == torch.float32)
        c = self.constraintsLoss()
        if fused and _is_std_normal(dens) and ops.nll_loss_fits(z) and (_is_zero(c) or _is_device_scalar(c)):
            # constraints - mean(log|det J| + log N(z)) in ONE launch that reads z itself (the standard-normal base density of
            # the factories; any other z_log_density module is called as the reference calls it)
            return ops.NllLossFn.apply(z, jac, None if _is_zero(c) else c)
        logn = dens(z)
        if fused and logn.shape == jac.shape and jac.shape[0] > 0 and logn.dtype == torch.float32:
            return _nll_mean(c, jac, logn)
        return c - (jac + logn).mean()

    def _backwards(self, method, z, context):
        """the steps' `method` (invert / rsample), last step to first, the flip between two steps undone"""
        for k in range(len(self.steps) - 1, -1, -1):
            x = getattr(self.steps[k], method)(z, context)
            z = torch.flip(x, dims=[1]) if k else x
        return z

    def invert(self, z, context=None):
        """Exact inverse of forward for any number of steps.  The reference (:166-169) visits steps[-0] == steps[0]
        first and never undoes the flip, so it only inverts nb_flow = 1 flows; for nb_flow = 1 this is
        identical to it."""
        return self._backwards("invert", z, context)

    def rsample(self, z, context=None):
        """invert(z, context), differentiable in z, the context and the parameters: the steps' rsample, last to first"""
        return self._backwards("rsample", z, context)

    def _single_step(self, what):
        if len(self.steps) != 1:
            raise ValueError(_SINGLE_STEP % (type(self).__name__ + "." + what, len(self.steps)))
        return self.steps[0]

    def intervene(self, z, do_index, do_value, context=None):
        """the single step's intervene; ValueError for a flow of several steps"""
        return self._single_step("intervene").intervene(z, do_index, do_value, context)

    # -- likelihoods --------------------------------------------------------------------------------------------
    def log_prob(self, x, context=None):
        """log p(x) [B]: log|det J| + z_log_density(z) of forward, the observational convenience"""
        z, logdet = self.forward(x, context)
        return logdet + self.z_log_density(z)

    def _do_step(self, what):
        """the single step of a flow whose likelihood can be truncated; ValueError otherwise"""
        step = self._single_step(what)
        dens = self.z_log_density
        if not _is_std_normal(dens):                    # (the test `loss` uses for its fold)
            raise ValueError("%s.%s: the truncated factorisation drops the pinned variables' terms log N(z_i) of a FACTORISED "
                             "base density; z_log_density here is %s, not the factories' standard normal, and a joint density "
                             "has no per-variable terms to truncate" % (type(self).__name__, what, type(dens).__name__))
        return step

    def log_prob_do(self, x, targets, regime=None, context=None, check_regime=True):
        """log p(x | do(x_S)) [B]: the joint's terms with those of the intervention targets left out (targets / regime:
        do_targets).  ValueError for a flow of several steps and for a base density other than the standard normal."""
        _, logdet, logn = self._do_step("log_prob_do").forward_do(x, targets, regime, context, check_regime)
        return logdet + logn

    def loss_do(self, x, targets, regime=None, context=None, check_regime=True):
        """constraintsLoss() - mean_b log p(x_b | do(x_S(b))): the training loss on a mix of observational and interventional
        rows, through the batch-mean launch of `loss` (ops.NllMeanFn)"""
        _, logdet, logn = self._do_step("loss_do").forward_do(x, targets, regime, context, check_regime)
        return _nll_mean(self.constraintsLoss(), logdet, logn)

    def counterfactual(self, x, do_index, do_value, context=None):
        """the single step's counterfactual; ValueError for a flow of several steps"""
        return self._single_step("counterfactual").counterfactual(x, do_index, do_value, context)

    def rsample_do(self, z, do_index, do_value, context=None):
        """the single step's rsample_do (intervene, differentiable); ValueError for a flow of several steps"""
        return self._single_step("rsample_do").rsample_do(z, do_index, do_value, context)

    def rcounterfactual(self, x, do_index, do_value, context=None):
        """the single step's rcounterfactual (counterfactual, differentiable); ValueError for a flow of several steps"""
        return self._single_step("rcounterfactual").rcounterfactual(x, do_index, do_value, context)


class CNNormalizingFlow(FCNormalizingFlow):
    """Multi-scale image flow (reference :172-226): after every scale the image is cut into d_c x d_h x d_w blocks;
    the first element of each block goes on to the next (coarser) flow, the others are emitted as latent variables."""

    def __init__(self, steps, z_log_density, dropping_factors):
        super().__init__(steps, z_log_density)
        self.dropping_factors = dropping_factors

    @staticmethod
    def _kept_shape(img_size, drop):
        return tuple(int(n / f) for n, f in zip(img_size, drop))

    @staticmethod
    def _blocks(z, img_size, drop):
        """[B, C*H*W] -> [B, c, h, w, d_c*d_h*d_w]  (equals the unfold chain of reference :184-185)"""
        c, h, w = CNNormalizingFlow._kept_shape(img_size, drop)
        d_c, d_h, d_w = drop
        return z.view(-1, c, d_c, h, d_h, w, d_w).permute(0, 1, 3, 5, 2, 4, 6).reshape(z.shape[0], c, h, w, -1)

    def forward(self, x, context=None):
        batch = x.shape[0]
        logdet, latents = None, []
        for flow, drop in zip(self.steps, self.dropping_factors):
            z, ld = flow(x, context)
            logdet = ld if logdet is None else logdet + ld
            blocks = self._blocks(z, flow.img_sizes, drop)
            latents.append(blocks[..., 1:].reshape(batch, -1))
            x = blocks[..., 0].reshape(batch, -1)
        latents.append(x)
        return torch.cat(latents, 1), logdet

    def invert(self, z, context=None):
        """Exact inverse of forward.  Only the flows forward's zip reaches take part (the CIFAR-10 factory builds four
        flows for three dropping factors), and when the last of them still drops elements, the tail of z is the block
        forward kept (`latents.append(x)`): the coarse-to-fine pass starts from it.  The reference (:209-226) pairs the
        reversed lists from their ends -- the wrong flow with each factor when the lengths differ, an IndexError for four
        and three -- and starts from `0.`, which it then views (divergence table)."""
        batch = z.shape[0]
        active = min(len(self.steps), len(self.dropping_factors))
        steps, drops = list(self.steps)[:active], list(self.dropping_factors)[:active]
        # slice z back into the per-scale latent blocks, in emission order
        parts, start = [], 0
        for flow, drop in zip(steps, drops):
            full = flow.img_sizes[0] * flow.img_sizes[1] * flow.img_sizes[2]
            c, h, w = self._kept_shape(flow.img_sizes, drop)
            width = full - c * h * w if full != c * h * w else full
            parts.append(z[:, start:start + width])
            start += width
        x = z[:, start:].contiguous() if start < z.shape[1] else None   # the block the last active scale kept, if any
        for flow, drop, zk in zip(reversed(steps), reversed(drops), reversed(parts)):
            c, h, w = self._kept_shape(flow.img_sizes, drop)
            if c * h * w != flow.img_sizes[0] * flow.img_sizes[1] * flow.img_sizes[2]:
                # re-interleave the element kept for the coarser scale with the dropped ones of each block
                blocks = torch.cat((x.view(batch, c, h, w, 1), zk.reshape(batch, c, h, w, -1)), 4)
                zk = blocks.view(batch, c, h, w, *drop).permute(0, 1, 4, 2, 5, 3, 6).reshape(batch, -1)
            x = flow.invert(zk.reshape(batch, -1), context)
        return x

    def rsample(self, z, context=None):
        raise NotImplementedError("CNNormalizingFlow.rsample: differentiable sampling of the multi-scale image flow is not "
                                  "implemented (the flat FCNormalizingFlow.rsample does not apply to it)")

    def intervene(self, z, do_index, do_value, context=None):
        raise ValueError(_SINGLE_STEP % ("CNNormalizingFlow.intervene", len(self.steps)) + "; a multi-scale flow has none "
                         "of one step's equations even with a single scale: its latent is cut and re-interleaved")

    def counterfactual(self, x, do_index, do_value, context=None):
        raise ValueError(_SINGLE_STEP % ("CNNormalizingFlow.counterfactual", len(self.steps)) + "; a multi-scale flow has "
                         "none of one step's equations even with a single scale: its latent is cut and re-interleaved")

    def rsample_do(self, z, do_index, do_value, context=None):
        raise ValueError(_SINGLE_STEP % ("CNNormalizingFlow.rsample_do", len(self.steps)) + "; a multi-scale flow has none "
                         "of one step's equations even with a single scale: its latent is cut and re-interleaved")

    def rcounterfactual(self, x, do_index, do_value, context=None):
        raise ValueError(_SINGLE_STEP % ("CNNormalizingFlow.rcounterfactual", len(self.steps)) + "; a multi-scale flow has "
                         "none of one step's equations even with a single scale: its latent is cut and re-interleaved")

    def _do_step(self, what):
        raise ValueError(_SINGLE_STEP % ("CNNormalizingFlow." + what, len(self.steps)) + "; a multi-scale flow has none "
                         "of one step's equations even with a single scale: its latent is cut and re-interleaved")
