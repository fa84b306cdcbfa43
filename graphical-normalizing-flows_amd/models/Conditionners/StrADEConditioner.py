"""StrADE: a masked autoencoder whose masks encode a GIVEN directed acyclic graph, so the d conditioners of a graphical
flow step cost one B-row pass of masked GEMMs (not in the reference: its models/Conditionners/strADEConditioner.py is an
empty file).  The graph may be one a DAG flow learned (DAGConditioner.get_dag() after post_process()), a known causal
graph, or a structural prior such as MNIST_A_prior."""
import contextlib

import numpy as np
import torch
import torch.nn as nn

from gnf_hip import ops
from .AutoregressiveConditioner import MaskedLinear
from .Conditioner import Conditioner, checked_context


def checked_adjacency(adjacency, d=None):
    """`adjacency` ([d, d] 0/1 array or tensor, adjacency[i][j] = 1: x_j is a parent of x_i -- the row convention of
    DAGConditioner; None: the full strictly-lower-triangular graph on d variables) as a uint8 numpy array.  ValueError for a
    non-square shape, entries other than 0/1, a non-zero diagonal or a cycle."""
    if adjacency is None:
        return np.tril(np.ones((d, d), dtype=np.uint8), -1)
    a = adjacency.detach().cpu().numpy() if torch.is_tensor(adjacency) else np.asarray(adjacency)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError("StrADE: the adjacency must be a square [d, d] array, got shape %s" % (tuple(a.shape),))
    if d is not None and a.shape[0] != d:
        raise ValueError("StrADE: the adjacency must be [%d, %d] (in_size), got shape %s" % (d, d, tuple(a.shape)))
    if not np.isin(a, (0, 1)).all():
        i, j = np.argwhere(~np.isin(a, (0, 1)))[0]
        raise ValueError("StrADE: the adjacency holds entries other than 0/1 (adjacency[%d][%d] = %r)" % (i, j, a[i, j]))
    a = a.astype(np.uint8)
    if a.diagonal().any():
        raise ValueError("StrADE: node %d is its own parent (non-zero diagonal)" % int(np.flatnonzero(a.diagonal())[0]))
    strade_var_levels(a)                                # (raises for a cycle)
    return a


def strade_var_levels(a):
    """level[i] = 0 for a root, else 1 + the largest level of a parent; ValueError naming a node for a cyclic graph"""
    d = a.shape[0]
    level, left = np.zeros(d, dtype=np.int64), a.sum(1).astype(np.int64)
    ready, seen = [i for i in range(d) if left[i] == 0], 0
    children = [np.flatnonzero(a[:, j]) for j in range(d)]
    while ready:
        j = ready.pop()
        seen += 1
        for i in children[j]:
            level[i] = max(level[i], level[j] + 1)
            left[i] -= 1
            if left[i] == 0:
                ready.append(int(i))
    if seen != d:
        raise ValueError("StrADE: the adjacency has a cycle through node %d" % int(np.flatnonzero(left > 0)[0]))
    return level


def strade_sets(a, cond_in):
    """[R', d] bool: the distinct non-empty parent sets P_0 .. P_{R-1} in order of first occurrence by variable index --
    with cond_in > 0 the empty set as well, so the root variables see the context.  A graph without any such set (no edge,
    no context) answers the empty set alone, R' = 1: every unit is a constant, as every output must be.  -> (sets, R)"""
    seen, sets = set(), []
    for i in range(a.shape[0]):
        key = a[i].tobytes()
        if key not in seen and (a[i].any() or cond_in > 0):
            seen.add(key)
            sets.append(a[i].astype(bool))
    R = len(sets)
    return (np.stack(sets) if sets else np.zeros((1, a.shape[0]), dtype=bool)), R


def strade_masks(adjacency, hidden, out_size, cond_in=0):
    """The masks of a StrADE net over `adjacency` ([d, d], checked_adjacency), one uint8 [out_features, in_features] array
    per layer (nn.Linear layout).  Pure numpy, deterministic.

    Let P_0 .. P_{R-1} be the sets of strade_sets.  Hidden unit k of EVERY hidden layer is assigned S_k = P_{k mod R}.
        first layer:       [u][c + j] = j in S_u; the cond_in context columns in front are visible to every unit
        hidden to hidden:  [u'][u] = S_u subset of S_u'
        output neuron c * d + i (component-major, as MADE):  [..][u] = S_u subset of pa(i)
        no hidden layer:   the output mask is the adjacency itself, the context visible to all outputs
    ValueError when a hidden width is below R: some variable would silently lose a parent.

    Consequence: output i can depend on exactly pa(i) (and on the context), on nothing else, for any widths >= R.  Nothing
    forbidden: a path input j -> ... -> output i runs through sets S_1 subset ... subset S_n subset pa(i) with j in S_1.
    Nothing lost: pa(i) is one of the P_r, every layer holds a unit with that set, and those units form a path from every
    j in pa(i) to output i."""
    a = checked_adjacency(adjacency)
    d, hidden = a.shape[0], [int(h) for h in hidden]
    ctx = np.ones(int(cond_in), dtype=np.uint8)
    if not hidden:
        row = np.concatenate([np.broadcast_to(ctx, (d, ctx.size)), a], 1)
        return [np.tile(row, (int(out_size), 1)).astype(np.uint8)]
    sets, R = strade_sets(a, cond_in)
    for h in hidden:
        if h < R:
            raise ValueError("StrADE: a hidden width of %d is below the %d distinct parent sets of the graph: some variable "
                             "would lose a parent" % (h, R))
    n = sets.shape[0]
    # P_a is a subset of Q iff no member of P_a lies outside Q: a count, exact in fp32 for d < 2^24
    member = sets.astype(np.float32)
    inside = member @ (~sets).astype(np.float32).T == 0                   # [a][b] = P_a subset of P_b
    below = member @ (a == 0).astype(np.float32).T == 0                   # [a][i] = P_a subset of pa(i)
    idx = [np.arange(h) % n for h in hidden]
    masks = [np.concatenate([np.broadcast_to(ctx, (hidden[0], ctx.size)), sets[idx[0]]], 1).astype(np.uint8)]
    for lo, hi in zip(idx, idx[1:]):
        masks.append(inside[lo][:, hi].T.astype(np.uint8))
    masks.append(np.tile(below[idx[-1]].T, (int(out_size), 1)).astype(np.uint8))
    return masks


def strade_level_plan(adjacency, hidden, out_size, cond_in=0):
    """Host tables for evaluating the StrADE net of strade_masks level by level, in the order in which an inversion learns
    the variables (pure numpy; gnf_strade_levels, include/gnf_hip.h):
        level[i]    0 for roots, else 1 + max over the parents;  nlev = depth + 1
        var_order   the variables in a stable sort by level;  var_off[t] (t = 0..nlev) = number of variables of level < t
        a unit's level: the largest variable level in its set, -1 for the empty set
        order[l]    the units of hidden layer l in a stable sort by level
        off[l][t]   (t = 0..nlev) number of units of level < t (the empty-set units count from t = 0 on)
        max_new     the largest number of units of one level in a layer (the last level excepted: nothing reads its units)
        widest      the largest number of variables of one level
    Level t computes the units of level t - 1 of every layer, order[l][off[l][t-1]:off[l][t]] (t = 0: order[l][:off[l][0]]):
    layer 0 from the context and var_order[:var_off[t]], layer l from order[l-1][:off[l-1][t]]; the outputs of the variables
    var_order[var_off[t]:var_off[t+1]] read order[-1][:off[-1][t]] (context and var_order[:var_off[t]] without a hidden
    layer).  Inside those prefixes the mask still applies."""
    a = checked_adjacency(adjacency)
    d, hidden = a.shape[0], [int(h) for h in hidden]
    level = strade_var_levels(a)
    nlev = int(level.max()) + 1
    var_off = np.searchsorted(np.sort(level), np.arange(nlev + 1), side="left").astype(np.int32)
    plan = {"d": d, "out": int(out_size), "widths": hidden, "cond_in": int(cond_in), "level": level, "nlev": nlev,
            "var_order": np.argsort(level, kind="stable").astype(np.int32), "var_off": var_off, "order": [], "off": [],
            "max_new": 0, "widest": int(np.diff(var_off).max())}
    if hidden:
        sets, R = strade_sets(a, cond_in)
        set_level = np.array([int(level[s].max()) if s.any() else -1 for s in sets], dtype=np.int64)
        for h in hidden:
            if h < R:
                raise ValueError("StrADE: a hidden width of %d is below the %d distinct parent sets of the graph" % (h, R))
            ul = set_level[np.arange(h) % sets.shape[0]]
            off = np.searchsorted(np.sort(ul), np.arange(nlev + 1), side="left").astype(np.int32)
            plan["order"].append(np.argsort(ul, kind="stable").astype(np.int32))
            plan["off"].append(off)
            plan["max_new"] = max(plan["max_new"], int(np.diff(np.concatenate([[0], off[:nlev]])).max()))
    return plan


class StrADENet(nn.Module):
    """the Sequential of MaskedLinear + ReLU under the key `net`, as MADE keeps it"""

    def __init__(self, sizes):
        super().__init__()
        net = []
        for h0, h1 in zip(sizes, sizes[1:]):
            net.extend([MaskedLinear(h0, h1), nn.ReLU()])
        net.pop()
        self.net = nn.Sequential(*net)

    def masked_layers(self):
        return [l for l in self.net if isinstance(l, MaskedLinear)]


class StrADEConditioner(Conditioner):
    """h[b, i, :] depends on x[b, pa(i)] (and the context) only, pa(i) read from a given `adjacency` (checked_adjacency;
    None: the full strictly-lower-triangular graph).  The net is a MADE whose masks are strade_masks(adjacency, ...): output
    i can depend on exactly pa(i), on nothing else, for any hidden widths >= the number of distinct parent sets.  forward is
    one ops.mlp call that streams the masks (degs=None); it returns the permuted [B, d, out] view of
    AutoregressiveConditioner.  The adjacency is kept as the persistent uint8 buffer `adjacency`; masks, depth() and the
    level plan follow the BUFFERS, so a loaded state_dict brings its graph along."""

    def __init__(self, in_size, hidden, out_size, cond_in=0, adjacency=None):
        super().__init__()
        self.in_size, self.hidden = int(in_size), [int(h) for h in hidden]
        self.out_size, self.cond_in = int(out_size), int(cond_in)
        a = checked_adjacency(adjacency, self.in_size)
        masks = strade_masks(a, self.hidden, self.out_size, self.cond_in)
        self.register_buffer("adjacency", torch.from_numpy(a.copy()))
        sizes = [self.in_size + self.cond_in] + self.hidden + [self.out_size * self.in_size]
        self.masked_autoregressive_net = StrADENet(sizes)
        for layer, mk in zip(self.masked_autoregressive_net.masked_layers(), masks):
            layer.mask.data.copy_(torch.from_numpy(mk.astype(np.float32)))
            layer._deg_checked = None

    def _layers(self):
        return self.masked_autoregressive_net.masked_layers()

    def forward(self, x, context=None):
        context = checked_context(context, self.cond_in, x)
        ls = self._layers()
        inp = x if context is None else torch.cat((context, x), 1)
        y = ops.mlp(inp, [(l.weight, l.bias) for l in ls], [l.mask for l in ls], degs=None)
        return y.view(x.shape[0], -1, self.in_size).permute(0, 2, 1)

    # -- what follows the buffers --------------------------------------------------------------------------------------
    _graph_cache = None                  # (key, (adjacency as numpy, depth)): plain attributes, nothing enters the state_dict
    _plan_cache = None                   # (key, plan)

    def _graph(self):
        key = (self.adjacency._version, self.adjacency.data_ptr())
        if self._graph_cache is None or self._graph_cache[0] != key:
            a = self.adjacency.detach().cpu().numpy()
            try:
                depth = int(strade_var_levels(a).max())
            except ValueError:                           # a loaded buffer that is no DAG: as deep as a graph can be
                depth = self.in_size - 1
            self._graph_cache = (key, (a, depth))
        return self._graph_cache[1]

    def depth(self):
        """the longest path of the graph in the `adjacency` buffer"""
        return self._graph()[1]

    def level_plan(self):
        """strade_level_plan of the `adjacency` buffer with its tables on the weights' device (and "var_host", the level
        order as ints), or None when the mask buffers in force are not strade_masks of that adjacency (a hand-edited mask, a
        checkpoint of other masks): the passes serve then.  Cached; re-derived when a buffer changes or moves."""
        layers = self._layers()
        dev = layers[0].weight.device
        key = (self.adjacency._version, self.adjacency.data_ptr(), dev,
               tuple((l.mask._version, l.mask.data_ptr()) for l in layers))
        if self._plan_cache is None or self._plan_cache[0] != key:
            plan = None
            a = self._graph()[0]
            try:
                want = strade_masks(a, self.hidden, self.out_size, self.cond_in)
                if all(tuple(l.mask.shape) == w.shape and np.array_equal(l.mask.detach().cpu().numpy(), w.astype(np.float32))
                       for l, w in zip(layers, want)):
                    plan = strade_level_plan(a, self.hidden, self.out_size, self.cond_in)
            except ValueError:
                plan = None
            if plan is not None:
                plan["var_host"] = [int(v) for v in plan["var_order"]]
                plan["level_host"] = [int(v) for v in plan["level"]]
                for k in ("order", "off"):
                    plan[k] = [torch.from_numpy(t).to(dev) for t in plan[k]]
                for k in ("var_order", "var_off"):
                    plan[k] = torch.from_numpy(plan[k]).to(dev)
            self._plan_cache = (key, plan)
        return self._plan_cache[1]

    # -- level-by-level inversion (NormalizingFlowStep._invert_by_strade) ----------------------------------------------------
    _held_pack = None

    def _params(self):
        return [p for l in self._layers() for p in (l.weight, l.bias)]

    def _masks(self):
        return [l.mask for l in self._layers()]

    def hold_level_pack(self):
        """context manager: the level-ordered image of mask o W, built once for the sweeps inside"""
        @contextlib.contextmanager
        def hold():
            prev = self._held_pack
            plan = self.level_plan()
            if prev is None and plan is not None:
                self._held_pack = ops.strade_pack(self._params(), self._masks(), plan)
            try:
                yield
            finally:
                self._held_pack = prev
        return hold()

    def level_sweep(self, z, x, mode, context=None, spline=None, pin=None):
        """the whole inversion on the HIP level kernel (gnf_hip.ops.strade_levels, one launch): x, or None when the net's
        rows do not fit the kernel's LDS tile (the passes serve).  `context`: the checked contiguous [B, cond_in] context;
        `spline`: (nb_bins, tail_bound) for ops.MADE_NORM_SPLINE; `pin`: the uint8 [d] pin table, by variable"""
        plan, params, masks = self.level_plan(), self._params(), self._masks()
        pack = self._held_pack if self._held_pack is not None else ops.strade_pack(params, masks, plan)
        return ops.strade_levels(params, masks, plan, pack, z, x, mode, context=context, spline=spline, pin=pin)

    # -- the adjoint of that sweep (NormalizingFlowStep.rsample's backward) -------------------------------------------------
    adjoint_levels = False               # opt-in: rsample's backward solves J^T lambda = g on gnf_strade_adjoint (one launch)
    _held_adjoint = None

    def hold_adjoint_pack(self):
        """context manager: the adjoint kernel's weight image (the level image and every layer transposed), built once for
        the adjoint_solve calls inside"""
        @contextlib.contextmanager
        def hold():
            prev = self._held_adjoint
            plan = self.level_plan()
            if prev is None and plan is not None:
                self._held_adjoint = ops.strade_adjoint_pack(self._params(), self._masks(), plan)
            try:
                yield
            finally:
                self._held_adjoint = prev
        return hold()

    def adjoint_solve(self, x, g, jac, dzdh, context=None, pin=None, want_gdo=False):
        """lambda [B, d] with J^T lambda = g for the step whose sample is x, on the HIP adjoint level kernel
        (gnf_hip.ops.strade_adjoint, one launch): jac [B, d] the normalizer's dz_i/dx_i, dzdh [B, d, out] its dz_i/dh_i;
        `context`: the checked [B, cond_in] context.  None when level_plan() is None (a hand-edited mask): the passes serve.
        pin (uint8 [d] on the device, by variable): the solve under do(x_pin = v) -- lambda is 0 at a pinned column;
        want_gdo: (lambda, gdo) with gdo = dL/dv at the pinned columns"""
        plan = self.level_plan()
        if plan is None:
            return None
        params, masks = self._params(), self._masks()
        pack = self._held_adjoint if self._held_adjoint is not None else ops.strade_adjoint_pack(params, masks, plan)
        do = {} if pin is None and not want_gdo else {"pin": pin, "gdo": want_gdo}
        return ops.strade_adjoint(params, masks, plan, pack, x, g, jac, dzdh, context=context, **do)
