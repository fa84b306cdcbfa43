"""Flow composition on the MI355X path: one (conditioner, normalizer) step, a stack of steps, and the multi-scale
image flow.  Class and method names, constructor arguments and `state_dict` keys are those of the reference's
models/NormalizingFlow.py (the drivers call getConditioners / getNormalizers / DAGness / step / isInvertible / invert
by name); the bodies are written against gnf_hip.ops.

    step:   h = conditioner(x);  z, jac = normalizer(x, h);  log|det J| = sum_i log jac_i      (reference :61-70)
    stack:  steps in sequence, feature order reversed between steps, log-dets added             (reference :110-126)
    loss:   sum of conditioner constraint terms - mean(log|det J| + log N(z))                  (reference :128-146)
"""
import weakref

import torch
import torch.nn as nn

from gnf_hip import ops
from .Conditionners import Conditioner, DAGConditioner
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


_SINGLE_STEP = ("%s: an intervention is defined on the data-side equations x_i = T^-1(z_i; h_i(x_pa(i), context)) of a "
                "ONE-step flow; the intermediate variables of a stacked or multi-scale flow are not the x_i (this flow has "
                "%d steps)")


def do_arguments(do_index, do_value, z):
    """(pinned variables as a tuple of ints, their values as a [B, S] tensor like z) of an intervention on z [B, d]:
    do_index a sequence of ints or an integer tensor [S], unique and in range; do_value a float, [S] or [B, S].
    ValueError otherwise."""
    if z.dim() != 2:
        raise ValueError("intervene: z must be [B, d], got %s" % (tuple(z.shape),))
    B, d = z.shape
    if torch.is_tensor(do_index):
        if (do_index.dim() != 1 or do_index.dtype.is_floating_point or do_index.dtype.is_complex
                or do_index.dtype == torch.bool):
            raise ValueError("intervene: do_index must be a sequence of ints or an integer tensor [S]")
        idx = tuple(int(i) for i in do_index.tolist())
    else:
        idx = tuple(do_index)
        if any(isinstance(i, bool) or not isinstance(i, int) for i in idx):
            raise ValueError("intervene: do_index must be a sequence of ints or an integer tensor [S]")
    if any(i < 0 or i >= d for i in idx):
        raise ValueError("intervene: do_index %s out of range for d = %d" % (list(idx), d))
    if len(set(idx)) != len(idx):
        raise ValueError("intervene: do_index %s names a variable twice" % (list(idx),))
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
        if torch.is_tensor(targets):
            if (targets.dim() != 1 or targets.dtype.is_floating_point or targets.dtype.is_complex):
                raise ValueError("do_targets: targets must be a sequence of ints, an integer tensor [S] or a bool / uint8 "
                                 "mask, got %s %s" % (targets.dtype, tuple(targets.shape)))
            idx = tuple(int(i) for i in targets.tolist())
        else:
            try:
                idx = tuple(targets)
            except TypeError:
                raise ValueError("do_targets: targets must be a sequence of ints, an integer tensor [S] or a bool / uint8 "
                                 "mask, got %r" % (type(targets),)) from None
            if any(isinstance(i, bool) or not isinstance(i, int) for i in idx):
                raise ValueError("do_targets: targets must be a sequence of ints, an integer tensor [S] or a bool / uint8 mask")
        if any(i < 0 or i >= d for i in idx):
            raise ValueError("do_targets: targets %s out of range for d = %d" % (list(idx), d))
        if len(set(idx)) != len(idx):
            raise ValueError("do_targets: targets %s name a variable twice" % (list(idx),))
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
    def _levels(self, importance):
        """the level schedule of the current gate, recomputed only when A (storage or version counter) or the gate's
        thresholds changed: DAGConditioner.levels() is a host synchronisation in front of every sampling pass otherwise.
        With `device_graph` it is two launches (gnf_hip.ops.dag_levels), a sort and one copy of 2 d + 3 integers; without
        it the d x d adjacency goes to the host and is walked in Python (5 ms against 0.9 at 784 x 784, 39 .. 427 ms
        against 1.6 .. 15 at d = 3072: profiles/dag_graph_ab.txt)"""
        cond = self.conditioner
        # A trainable A is rewritten by the optimiser through a raw pointer (gnf_hip.dp: fused Adam on the flat buffer, a
        # replayed hipGraph), which moves neither its version counter nor its address: nothing is cached for it.  A frozen
        # one is keyed on (storage, version, thresholds, the conditioner's cache epoch -- see invalidate_caches()).
        key = (None if cond.A.requires_grad else
               (cond.A.data_ptr(), cond.A._version, float(cond.h_thresh), bool(cond.s_thresh), cond.A.device,
                getattr(cond, "_cache_epoch", 0)))
        if key is None or getattr(self, "_levels_key", None) != key:
            lv = cond.levels(importance, with_host=True)
            if lv is not None and cond.A.shape[0] == 784:
                # the order of the variables INSIDE a level is free: take the one the sparse embedding kernels work in (crop
                # origin, then pixel), so that their output needs no un-sorting gather
                lv = [(torch.as_tensor(_crop_order(hr), dtype=torch.long, device=rows.device), _crop_order(hr))
                      for rows, hr in lv]
            self._levels_val = lv
            self._levels_all = torch.cat([rows for rows, _ in lv]) if lv else None   # one gather of z per pass
            self._levels_rows32 = [rows.to(torch.int32) for rows, _ in lv] if lv else None   # scatter tables of the inverse
            self._levels_key = key
            _INV_GRAPHS.pop(self, None)                 # graphs captured for another gate replay another schedule
        return self._levels_val, key

    def _invert_levels_body(self, z, levels, importance, context, x=None, tables=None):
        """variable-major inside: z is gathered ONCE into [sum of level sizes, B] (a level is a contiguous slice), the
        conditioner rows come as [R, B, out] -- the layout the sparse kernels write -- and the normalizer's inverse is
        element-wise in whatever two leading dimensions z and h share.  Per level that leaves the embedding front, the
        inverse and one scatter into x (no gather of z, no un-sorting or permuting copy of h)."""
        cond = self.conditioner
        # (intervene() brings its own x, pinned columns filled, and the (all rows, int32 rows) tables of its own schedule)
        x = torch.zeros_like(z) if x is None else x
        zt = z.t()[self._levels_all if tables is None else tables[0]]         # [sum R, B], contiguous
        off = 0
        into = getattr(self.normalizer, "inverse_transform_into", None)       # (the normalizers ignore the context)
        rows32 = getattr(self, "_levels_rows32", None) if tables is None else tables[1]
        if into is not None and (rows32 is None or len(rows32) != len(levels)):
            into = None
        for k, (rows, host_rows) in enumerate(levels):
            R = rows.numel()
            h = cond.forward_rows(x, rows, importance, host_rows, variable_major=True,
                                  rows32=rows32[k] if rows32 is not None and len(rows32) == len(levels) else None,
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

    def _invert_by_levels(self, z, context):
        """DAG conditioner with a deterministic gate: every variable is inverted once, after its parents -- d
        conditioner rows in total instead of (depth + 1) * d.  Same values as the fixed-point passes (non-parents are
        masked by exact zeros either way).  Returns None when not applicable.

        A conditioner built with cond_in > 0 takes its (checked) context along: every level's rows are completed with
        context[b] by the DAGMLP, on the composed formulation, launch by launch (no graph is captured for such a pass).

        On the GPU the pass of a given (gate, batch shape, node count) is captured into a hipGraph the second time it is
        asked for and replayed from then on (`graph_invert`): with a frozen A the schedule, the row tables and the sparse
        plans are static, and a sampling pass over MNIST is ~650 launches of 5-100 us (reference ImageExperiments.py:341-350
        samples after post_process()).  The weight image of the normalizer is packed INSIDE the graph, so a replay reads
        the current parameters."""
        cond = self.conditioner
        if not (_is_dag(cond) and self.level_schedule):
            return None
        cond_in = int(getattr(cond, "cond_in", 0) or 0)
        if not cond_in and context is not None:
            return None                                 # the passes raise what a cond_in = 0 conditioner raises
        if cond_in:
            context = checked_context(context, cond_in, z)              # ValueError: missing, wrong width / rank / rows
            if z.dim() != 2 or context.device != z.device or context.dtype != z.dtype:
                return None
        importance = cond.deterministic_importance()
        if importance is None:
            return None
        levels, lkey = self._levels(importance)
        if levels is None:
            return None
        if cond_in and z.shape[0] == 0:
            return torch.zeros_like(z)                  # no rows, no launch (as the column schedule answers an empty batch)
        # a captured pass bakes the ADDRESS of the importance matrix in: only A itself qualifies -- the thresholded forms
        # (s_thresh / h_thresh > 0, the state the reference's threshold sweep sets) are temporaries freed after this call
        graphable = (self.graph_invert and context is None and z.is_cuda and not cond.A.requires_grad
                     and z.dtype == torch.float32 and importance.data_ptr() == cond.A.data_ptr()
                     and len(levels) > 4 and not torch.cuda.is_current_stream_capturing())
        if not graphable:
            return self._invert_levels_body(z, levels, importance, context)
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
            return self._invert_levels_body(z, levels, importance, context)
        if entry == "eager":                            # a capture of this variant failed once: launch by launch from then on
            return self._invert_levels_body(z, levels, importance, context)
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
                    self._invert_levels_body(zbuf, levels, importance, context)
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
                    xbuf = self._invert_levels_body(zbuf, levels, importance, context)
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
                return self._invert_levels_body(z, levels, importance, context)
            if len(graphs) > self.GRAPH_INVERT_MAX:
                graphs.clear()
            entry = graphs[key] = (graph, zbuf, xbuf)
        graph, zbuf, xbuf = entry
        zbuf.copy_(z, non_blocking=True)
        graph.replay()
        return xbuf.clone()

    def _invert_by_columns(self, z, context):
        """MADE conditioner: the variables are inverted in degree order, one per step, and a step evaluates only the hidden
        units that became final with the previous column (AutoregressiveConditioner.prefix_plan) -- about half of ONE masked
        forward and ONE normalizer inverse in total, where the passes below spend depth() + 1 = d of each.  The same function
        in another fp32 summation order.  Returns None when not applicable.

        A conditional MADE (cond_in > 0) is inverted the same way from its conditional plan (prefix_plan(with_context=True)):
        the checked context heads the kernel's activation rows, the conditioner module is never called."""
        cond = self.conditioner
        get_plan = getattr(cond, "prefix_plan", None)
        if not (self.column_schedule and get_plan is not None and z.is_cuda and z.dim() == 2
                and z.dtype == torch.float32):
            return None
        cond_in = int(getattr(cond, "cond_in", 0) or 0)
        if not cond_in and context is not None:
            return None                                 # the passes raise what a cond_in = 0 conditioner raises
        if cond_in:
            context = checked_context(context, cond_in, z)              # ValueError: missing, wrong width / rank / rows
            if context.device != z.device or context.dtype != torch.float32:
                return None
        if z.shape[0] == 0:
            # no rows, no launch: the empty result (the passes would stop at the MADE's `.view(0, -1, d)` as the reference's do)
            return torch.zeros_like(z)
        plan = get_plan(with_context=True) if cond_in else get_plan()
        if plan is None or plan["d"] != z.shape[1]:
            return None
        if cond_in:
            context = context.contiguous()
        z = z.contiguous()
        x = torch.zeros_like(z)
        B, d, out = z.shape[0], plan["d"], plan["out"]
        with cond.hold_prefix_pack():
            if type(self.normalizer) is AffineNormalizer:
                # the whole inversion, one launch
                cond.prefix_steps(z, x, 0, d, ops.MADE_NORM_AFFINE, **({"context": context} if cond_in else {}))
                return x
            if type(self.normalizer) is SplineNormalizer:
                # likewise: the spline's closed-form inverse is the kernel's per-row epilogue
                cond.prefix_steps(z, x, 0, d, ops.MADE_NORM_SPLINE, spline=(self.normalizer.nb_bins, self.normalizer.tail_bound),
                                  **({"context": context} if cond_in else {}))
                return x
            h = torch.empty(B, out, dtype=torch.float32, device=z.device)
            ws = cond.prefix_workspace(B)
            zt = z.t().contiguous()                                          # a column of z as a one-row [1, B] problem
            cols = torch.arange(d, dtype=torch.int32, device=z.device)
            into = getattr(self.normalizer, "inverse_transform_into", None)
            for t in range(d):
                v = plan["var_host"][t]
                cond.prefix_steps(z, x, t, t + 1, ops.MADE_NORM_NONE, h_out=h, ws=ws,
                                  **({"context": context} if cond_in else {}))
                # the normalizer's own inverse of that one column; the fused Monotonic kernel writes x[:, v] itself
                if into is None or not into(zt[v:v + 1], h.view(1, B, out), x, cols[v:v + 1]):
                    x[:, v:v + 1] = self.normalizer.inverse_transform(z[:, v:v + 1], h.view(B, 1, out), context)
        return x

    def invert(self, z, context=None):
        """Reference :98-107: fixed point of x <- normalizer^-1(z, conditioner(x)) from x = 0, depth()+1 passes, early
        exit once a pass changes nothing (its progress print is dropped)."""
        import contextlib
        with torch.no_grad(), contextlib.ExitStack() as stack:   # parameters do not change inside: build their images once
            for _, _, make in self._holders():
                stack.enter_context(make())
            x = self._invert_by_levels(z, context)
            if x is None:
                x = self._invert_by_columns(z, context)
            if x is not None:
                return x
            x = torch.zeros_like(z)
            for _ in range(self.conditioner.depth() + 1):
                previous = x
                x = self.normalizer.inverse_transform(z, self.conditioner(x, context), context)
                if torch.equal(x, previous):
                    break
        return x

    # -- interventions ------------------------------------------------------------------------------------------
    DO_LEVELS_MAX = 8                    # mutilated level schedules kept per step (pinned tuples of one gate)

    def _do_levels(self, importance, idx):
        """(levels, (all rows, int32 rows per level)) of the MUTILATED graph of do(x_idx): the pinned variables lose their
        parents (their rows of the importance matrix zeroed) and leave the level lists; levels that held only pinned
        variables vanish.  None for a cyclic graph.  Cached beside -- never in -- invert's `_levels_*` attributes, on the
        key of `_levels` plus the pinned tuple; a trainable A caches nothing, as there."""
        cond = self.conditioner
        key = (None if cond.A.requires_grad else
               (cond.A.data_ptr(), cond.A._version, float(cond.h_thresh), bool(cond.s_thresh), cond.A.device,
                getattr(cond, "_cache_epoch", 0), tuple(sorted(idx))))
        cache = self.__dict__.setdefault("_do_levels_cache", {})
        if key is not None and key in cache:
            return cache[key]
        cut = importance.detach().clone()
        cut[list(idx)] = 0
        lv = cond.levels(cut, with_host=True)
        entry = None
        if lv is not None:
            pinned, out = set(idx), []
            for rows, host in lv:
                keep = tuple(r for r in host if r not in pinned)
                if cond.A.shape[0] == 784:              # the order inside a level that the sparse embedding kernels work in
                    keep = _crop_order(keep)
                if keep:
                    out.append((rows if len(keep) == len(host) and cond.A.shape[0] != 784 else
                                torch.as_tensor(keep, dtype=torch.long, device=rows.device), keep))
            tables = ((torch.cat([rows for rows, _ in out]), [rows.to(torch.int32) for rows, _ in out]) if out else
                      (None, None))
            entry = (out, tables)
        if key is not None:
            if len(cache) >= self.DO_LEVELS_MAX:
                cache.clear()
            cache[key] = entry
        return entry

    def _intervene_by_levels(self, z, idx, vals, context):
        """DAG conditioner, deterministic gate: the level schedule of the mutilated graph.  x[:, idx] = vals is written
        before the first level, then `_invert_levels_body` runs on the remaining rows -- fewer conditioner rows and no
        more levels than invert needs.  Launch by launch: no graph is captured, and invert's cache and its captured
        graphs are not touched.  Returns None when not applicable (the conditions of `_invert_by_levels`)."""
        cond = self.conditioner
        if not (_is_dag(cond) and self.level_schedule):
            return None
        cond_in = int(getattr(cond, "cond_in", 0) or 0)
        if not cond_in and context is not None:
            return None
        if cond_in:
            context = checked_context(context, cond_in, z)
            if z.dim() != 2 or context.device != z.device or context.dtype != z.dtype:
                return None
        importance = cond.deterministic_importance()
        if importance is None:
            return None
        if idx:
            entry = self._do_levels(importance, idx)
            if entry is None:
                return None
            levels, tables = entry
        else:                                           # P empty: invert's own schedule, read as invert reads it
            levels, _ = self._levels(importance)
            if levels is None:
                return None
            tables = None
        x = torch.zeros_like(z)
        if idx:
            x[:, list(idx)] = vals
        if z.shape[0] == 0 or not levels:
            return x
        return self._invert_levels_body(z, levels, importance, context, x=x, tables=tables)

    def _intervene_by_columns(self, z, idx, vals, context):
        """MADE conditioner: the column sweep with a pin table (gnf_made_prefix_do).  x[:, idx] = vals is written first; a
        pinned step reads its column instead of computing it.  Affine / Spline + MADE stay ONE launch; any other normalizer
        is stepped through AutoregressiveConditioner.made_do_launches: one launch per FREE column, which advances through
        the run of pinned degrees in front of it, and none for a trailing run.  Returns None when not applicable (the
        conditions of `_invert_by_columns`)."""
        from .Conditionners.AutoregressiveConditioner import made_do_launches
        cond = self.conditioner
        get_plan = getattr(cond, "prefix_plan", None)
        if not (self.column_schedule and get_plan is not None and z.is_cuda and z.dim() == 2
                and z.dtype == torch.float32):
            return None
        cond_in = int(getattr(cond, "cond_in", 0) or 0)
        if not cond_in and context is not None:
            return None
        if cond_in:
            context = checked_context(context, cond_in, z)
            if context.device != z.device or context.dtype != torch.float32:
                return None
        if z.shape[0] == 0:
            return torch.zeros_like(z)
        plan = get_plan(with_context=True) if cond_in else get_plan()
        if plan is None or plan["d"] != z.shape[1]:
            return None
        kw = {"context": context.contiguous()} if cond_in else {}
        z = z.contiguous()
        x = torch.zeros_like(z)
        B, d, out = z.shape[0], plan["d"], plan["out"]
        if idx:
            x[:, list(idx)] = vals
            if len(idx) == d:
                return x                                # every degree is a trailing pinned one: no launch
            pin = torch.zeros(d, dtype=torch.uint8, device=z.device)
            pin[list(idx)] = 1
            kw["pin"] = pin
        with cond.hold_prefix_pack():
            if type(self.normalizer) is AffineNormalizer:
                cond.prefix_steps(z, x, 0, d, ops.MADE_NORM_AFFINE, **kw)
                return x
            if type(self.normalizer) is SplineNormalizer:
                cond.prefix_steps(z, x, 0, d, ops.MADE_NORM_SPLINE, spline=(self.normalizer.nb_bins, self.normalizer.tail_bound),
                                  **kw)
                return x
            h = torch.empty(B, out, dtype=torch.float32, device=z.device)
            ws = cond.prefix_workspace(B)
            zt = z.t().contiguous()
            cols = torch.arange(d, dtype=torch.int32, device=z.device)
            into = getattr(self.normalizer, "inverse_transform_into", None)
            for t0, t1 in made_do_launches(plan["var_host"], idx):
                v = plan["var_host"][t1 - 1]            # the launch's one free column, behind t1 - 1 - t0 pinned ones
                cond.prefix_steps(z, x, t0, t1, ops.MADE_NORM_NONE, h_out=h, ws=ws, **kw)
                if into is None or not into(zt[v:v + 1], h.view(1, B, out), x, cols[v:v + 1]):
                    x[:, v:v + 1] = self.normalizer.inverse_transform(z[:, v:v + 1], h.view(B, 1, out), context)
        return x

    def _refuse_stochastic_gate(self):
        cond = self.conditioner
        if _is_dag(cond) and cond.deterministic_importance() is None:
            raise ValueError("NormalizingFlowStep.intervene: the DAG conditioner's gate is stochastic (stoch_gate / noise_gate); "
                             "every evaluation of the conditioner would draw another graph than the one the intervention "
                             "cuts.  Use a deterministic gate (stoch_gate = noise_gate = False)")

    def intervene(self, z, do_index, do_value, context=None):
        """x under do(x[:, do_index] = do_value) (interventions):  x[b, i] = do_value[b, i] exactly for a pinned
        i, x[b, i] = normalizer^-1(z[b, i], conditioner(x, context)[b, i]) for every other; z[:, do_index] is ignored.  An
        empty do_index is invert(z, context), bit for bit.  Three arms on invert's conditions (`level_schedule`,
        `column_schedule`), recorded in `_intervene_arm`: "levels" (DAG), "columns" (MADE), "passes" (anything, anywhere:
        x <- where(pinned, v, normalizer^-1(z, conditioner(x))) from where(pinned, v, 0), depth() + 1 passes of the
        un-mutilated graph -- the mutilated one is never deeper -- with invert's early exit).

        A DAG conditioner with a stochastic or noisy gate is refused as rsample refuses it: every pass and every level
        would draw another graph to mutilate."""
        import contextlib
        cond = self.conditioner
        self._refuse_stochastic_gate()
        idx, vals = do_arguments(do_index, do_value, z)
        self._intervene_arm = None
        with torch.no_grad(), contextlib.ExitStack() as stack:
            for _, _, make in self._holders():
                stack.enter_context(make())
            x = self._intervene_by_levels(z, idx, vals, context)
            if x is not None:
                self._intervene_arm = "levels"
                return x
            x = self._intervene_by_columns(z, idx, vals, context)
            if x is not None:
                self._intervene_arm = "columns"
                return x
            self._intervene_arm = "passes"
            cols = list(idx)
            x = torch.zeros_like(z)
            if cols:
                x[:, cols] = vals
            if len(cols) == z.shape[1]:
                return x                                # no free equation: the conditioner is never asked
            for _ in range(cond.depth() + 1):
                previous = x
                x = self.normalizer.inverse_transform(z, cond(x, context), context)
                if cols:
                    x[:, cols] = vals
                if torch.equal(x, previous):
                    break
        return x

    def counterfactual(self, x, do_index, do_value, context=None):
        """abduction, then action: z = forward(x, context), then intervene(z, ...).  No column is copied from x: what a
        non-descendant of the pinned variables comes back as is the inversion's own residual."""
        self._refuse_stochastic_gate()
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
        cond = self.conditioner
        if _is_dag(cond) and cond.deterministic_importance() is None:
            raise ValueError("NormalizingFlowStep.rsample: the DAG conditioner's gate is stochastic (stoch_gate / noise_gate); "
                             "the backward would recompute the conditioner under another draw of the gate than the sample "
                             "saw.  Use a deterministic gate (stoch_gate = noise_gate = False)")
        return ops.InvertFn.apply(self, z, context, *[p for p in self.parameters() if p.requires_grad])

    def _adjoint_plan(self, x, context):
        """the MADE plan of the adjoint arm when _invert_by_columns would be taken for this sample (and `adjoint_schedule`),
        else None: the passes arm"""
        cond = self.conditioner
        get_plan = getattr(cond, "prefix_plan", None)
        if not (self.adjoint_schedule and self.column_schedule and get_plan is not None
                and getattr(cond, "adjoint_solve", None) is not None and x.is_cuda and x.dim() == 2
                and x.dtype == torch.float32):
            return None
        cond_in = int(getattr(cond, "cond_in", 0) or 0)
        if bool(cond_in) != (context is not None):
            return None
        if cond_in and (context.device != x.device or context.dtype != torch.float32):
            return None
        plan = get_plan(with_context=True) if cond_in else get_plan()
        return plan if plan is not None and plan["d"] == x.shape[1] else None

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
        plain_c = isinstance(c, float) and c == 0.
        dev_c = torch.is_tensor(c) and c.is_cuda and c.dim() == 0 and c.dtype == torch.float32
        # the fold applies to the factories' base density and to nothing that merely inherits from it: a subclass that
        # overrides forward (tempered / scaled / conditional density) is called as the reference calls it
        std_normal = (getattr(dens, "standard_normal", False)
                      and getattr(type(dens), "_std_forward", None) is type(dens).forward)
        if fused and std_normal and ops.nll_loss_fits(z) and (plain_c or dev_c):
            # constraints - mean(log|det J| + log N(z)) in ONE launch that reads z itself (the standard-normal base density of
            # the factories; any other z_log_density module is called as the reference calls it)
            return ops.NllLossFn.apply(z, jac, None if plain_c else c)
        logn = dens(z)
        if fused and logn.shape == jac.shape and jac.shape[0] > 0 and logn.dtype == torch.float32:
            if plain_c:
                return ops.NllMeanFn.apply(jac, logn)                            # -(jac + logn).mean(), one launch
            if dev_c:
                return ops.NllMeanFn.apply(jac, logn, c)                         # constraints - mean(...), the same launch
            return c + ops.NllMeanFn.apply(jac, logn)
        return c - (jac + logn).mean()

    def invert(self, z, context=None):
        """Exact inverse of forward for any number of steps.  The reference (:166-169) visits steps[-0] == steps[0]
        first and never undoes the flip, so it only inverts nb_flow = 1 flows; for nb_flow = 1 this is
        identical to it."""
        for k in range(len(self.steps) - 1, -1, -1):
            x = self.steps[k].invert(z, context)
            z = torch.flip(x, dims=[1]) if k else x
        return z

    def rsample(self, z, context=None):
        """invert(z, context), differentiable in z, the context and the parameters: the steps' rsample, last to first"""
        for k in range(len(self.steps) - 1, -1, -1):
            x = self.steps[k].rsample(z, context)
            z = torch.flip(x, dims=[1]) if k else x
        return z

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
        # the test `loss` uses for its fold: the factories' standard normal itself, nothing that merely inherits from it
        if not (getattr(dens, "standard_normal", False)
                and getattr(type(dens), "_std_forward", None) is type(dens).forward):
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
        c = self.constraintsLoss()
        if isinstance(c, float) and c == 0.:
            return ops.NllMeanFn.apply(logdet, logn)
        if torch.is_tensor(c) and c.is_cuda and c.dim() == 0 and c.dtype == torch.float32:
            return ops.NllMeanFn.apply(logdet, logn, c)
        return c + ops.NllMeanFn.apply(logdet, logn)

    def counterfactual(self, x, do_index, do_value, context=None):
        """the single step's counterfactual; ValueError for a flow of several steps"""
        return self._single_step("counterfactual").counterfactual(x, do_index, do_value, context)


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

    def _do_step(self, what):
        raise ValueError(_SINGLE_STEP % ("CNNormalizingFlow." + what, len(self.steps)) + "; a multi-scale flow has none "
                         "of one step's equations even with a single scale: its latent is cut and re-interleaved")
