import numpy as np
import torch
import torch.nn as nn

from gnf_hip import ops
from .Conditioner import Conditioner, checked_context


class MaskedLinear(nn.Linear):
    """nn.Linear with a fixed 0/1 `mask` buffer on the weights (reference
    AutoregressiveConditioner.py:14-25).  The product mask*weight is never materialised:
    the GEMM multiplies the mask in while it stages the weight tile."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__(in_features, out_features, bias)
        self.register_buffer('mask', torch.ones(out_features, in_features))
        # the degrees the mask was built from (not part of the reference's state_dict): mask[o][i] = deg_in[i] <= deg_out[o]
        # (strict: <).  The small-batch kernels evaluate that rule instead of streaming the fp32 mask next to the weights.
        self.register_buffer('deg_out', torch.zeros(out_features), persistent=False)
        self.register_buffer('deg_in', torch.zeros(in_features), persistent=False)
        self.deg_strict = False
        self._deg_checked = None           # (mask version, deg versions) of the last verification, and its verdict
        self._deg_ok = False

    def set_mask(self, mask, deg_out=None, deg_in=None, strict=False):
        self.mask.data.copy_(torch.from_numpy(mask.astype(np.uint8).T))
        if deg_out is not None:
            self.deg_out.data.copy_(torch.as_tensor(np.asarray(deg_out), dtype=torch.float32))
            self.deg_in.data.copy_(torch.as_tensor(np.asarray(deg_in), dtype=torch.float32))
            self.deg_strict = bool(strict)
        self._deg_checked = None

    def degree_spec(self):
        """(deg_out, deg_in, strict) if the mask buffer IS the degree rule (checked once per change of the buffers -- a
        loaded checkpoint or a user's set_mask may carry any 0/1 pattern), else None: the kernels then read the mask."""
        key = (self.mask._version, self.deg_out._version, self.deg_in._version, self.mask.data_ptr(), self.deg_strict)
        if self._deg_checked != key:
            cmp = torch.lt if self.deg_strict else torch.le
            self._deg_ok = bool(torch.equal(self.mask, cmp(self.deg_in[None, :], self.deg_out[:, None]).to(self.mask.dtype)))
            self._deg_checked = key
        return (self.deg_out, self.deg_in, self.deg_strict) if self._deg_ok else None

    def forward(self, input):
        return ops.mlp(input, [(self.weight, self.bias)], [self.mask], degs=[self.degree_spec()])


def made_degrees(nin, hidden_sizes, random=False, natural_ordering=False, rng=None):
    """Degrees of the reference MADE (:79-87): the natural ordering with degrees nin - 1 - (i mod nin) (`random=False`, the
    only form the reference's AutoregressiveConditioner builds), or a sampled ordering / connectivity drawn from `rng` exactly
    as the reference draws it (input order: a permutation unless natural_ordering; hidden degrees uniform in
    [min of the layer below, nin - 1))."""
    if random:
        m = {-1: np.arange(nin) if natural_ordering else rng.permutation(nin)}
        for l, hsz in enumerate(hidden_sizes):
            m[l] = rng.randint(m[l - 1].min(), nin - 1, size=hsz)
        return m
    m = {-1: np.arange(nin)}
    for l, hsz in enumerate(hidden_sizes):
        m[l] = np.array([nin - 1 - (i % nin) for i in range(hsz)])
    return m


def made_prefix_plan(m, nin, nout):
    """Tables for evaluating a MADE with degrees `m` (MADE.m: {-1: inputs, l: hidden layer l}) prefix by prefix, in the order
    in which an inversion learns the variables: step t inverts the variable of degree t, and by the degree rule a hidden
    unit of degree g is final once the variables of degree <= g are known.  Pure numpy:
        order[l]     the units of hidden layer l in a stable sort by degree
        off[l][t]    (t = 0..nin) number of units of degree < t: those units are order[l][:off[l][t]]
        var_of_step  var_of_step[t] = the variable of degree t
        out          outputs per variable (output neuron of component c of variable v: c * nin + v)
        max_new      the largest number of units of one degree < nin - 1 in a layer (what one step computes)
    Step t >= 1 computes the units of degree t - 1 of every layer, order[l][off[l][t-1]:off[l][t]]: layer 0 from the inputs
    of degree <= t - 1 (var_of_step[:t]), layer l from order[l-1][:off[l-1][t]]; the outputs of var_of_step[t] read the last
    hidden layer's units of degree < t, order[-1][:off[-1][t]] (the inputs of degree < t when there is no hidden layer)."""
    L = len(m) - 1
    deg_in = np.asarray(m[-1]).astype(np.int64)
    if not np.array_equal(np.sort(deg_in), np.arange(nin)):
        raise ValueError("the input degrees must be a permutation of 0..nin-1")
    order, off, widths, max_new = [], [], [], 0
    for l in range(L):
        deg = np.asarray(m[l]).astype(np.int64)
        order.append(np.argsort(deg, kind="stable").astype(np.int32))
        off.append(np.searchsorted(np.sort(deg), np.arange(nin + 1), side="left").astype(np.int32))
        widths.append(int(deg.size))
        if nin > 1:
            max_new = max(max_new, int(np.diff(off[-1][:nin]).max()))
    return {"d": int(nin), "out": int(nout // nin), "widths": widths, "order": order, "off": off,
            "var_of_step": np.argsort(deg_in, kind="stable").astype(np.int32), "max_new": max_new}


def made_do_launches(var_of_step, pinned):
    """The NONE-mode launches (t0, t1) of a column sweep under do(x_pinned): one per FREE variable, in degree order, each
    starting behind the previous one's column -- so the run of pinned degrees in front of a free column is walked inside
    the launch that computes that column's outputs (step t1 - 1 free, every step of [t0, t1 - 1) pinned: what
    gnf_made_prefix_do demands of such a call) -- and nothing for a trailing run of pinned degrees, which no column
    reads.  Pure host logic: var_of_step[t] = the variable of degree t, pinned = the pinned variables."""
    pinned = set(int(v) for v in pinned)
    out, t0 = [], 0
    for t, v in enumerate(var_of_step):
        if int(v) not in pinned:
            out.append((t0, t + 1))
            t0 = t + 1
    return out


class MADE(nn.Module):
    """Masked autoencoder, reference AutoregressiveConditioner.py:28-109: natural ordering (`random=False`, what the
    conditioner builds) or sampled orderings (`random=True`), cycling through `num_masks` seeds on update_masks().  Every
    mask is a degree rule deg_in <= deg_out (< for the output layer), so the small-batch kernels evaluate it from the two
    degree vectors whatever the ordering; output neurons are chunked component-major."""

    def __init__(self, nin, hidden_sizes, nout, num_masks=1, natural_ordering=False, random=False, device="cpu", cond_in=0):
        super().__init__()
        self.random = random
        self.nin = nin
        self.nout = nout
        self.hidden_sizes = hidden_sizes
        self.cond_in = cond_in                           # context columns in FRONT of the nin variables in the first layer
        assert self.nout % self.nin == 0, "nout must be integer multiple of nin"
        net = []
        hs = [nin + cond_in] + hidden_sizes + [nout]
        for h0, h1 in zip(hs, hs[1:]):
            net.extend([MaskedLinear(h0, h1), nn.ReLU()])
        net.pop()
        self.net = nn.Sequential(*net)
        self.natural_ordering = natural_ordering
        self.num_masks = num_masks
        self.seed = 0                                    # cycles through the num_masks orderings (reference :68)
        self.m = {}
        self.update_masks()

    def update_masks(self):
        if self.m and self.num_masks == 1:
            return
        L = len(self.hidden_sizes)
        rng = np.random.RandomState(self.seed)           # (drawn from even when unused, as the reference does)
        self.seed = (self.seed + 1) % self.num_masks
        self.m = made_degrees(self.nin, self.hidden_sizes, self.random, self.natural_ordering, rng)
        # degrees of the columns of each layer: a context column has degree -1, below every variable's, so every unit of the
        # first layer sees it -- under the strict rule of the output layer too (hidden_sizes == [])
        din = {l: self.m[l] for l in range(-1, L)}
        if self.cond_in:
            din[-1] = np.concatenate([np.full(self.cond_in, -1, dtype=self.m[-1].dtype), self.m[-1]])
        masks = [din[l - 1][:, None] <= self.m[l][None, :] for l in range(L)]
        masks.append(din[L - 1][:, None] < self.m[-1][None, :])
        degs = [(self.m[l], din[l - 1], False) for l in range(L)]
        deg_last = self.m[-1]
        if self.nout > self.nin:
            masks[-1] = np.concatenate([masks[-1]] * int(self.nout / self.nin), axis=1)
            deg_last = np.concatenate([deg_last] * int(self.nout / self.nin))
        degs.append((deg_last, din[L - 1], True))
        for layer, mk, (do, di, strict) in zip(self.masked_layers(), masks, degs):
            layer.set_mask(mk, do, di, strict)
        # position of input dimension k in the sampled order (a public attribute of the reference's class, :99-101)
        self.i_map = self.m[-1].copy()
        for k in range(len(self.m[-1])):
            self.i_map[self.m[-1][k]] = k

    def masked_layers(self):
        return [l for l in self.net if isinstance(l, MaskedLinear)]

    _prefix_cache = None                 # (key, plan): plain attributes, nothing enters the state_dict

    def prefix_plan(self, with_context=False):
        """made_prefix_plan(self.m) with its tables on the weights' device, or None when the masks in force are not the
        degree rule of self.m (a loaded checkpoint, a hand-set mask) or the net is conditioned on a context.  Cached;
        rebuilt when update_masks() installs another ordering or a mask buffer changes.
        with_context=True: the plan of a net with cond_in > 0 as well -- the same tables plus plan["cond_in"]; the context
        columns have input degree -1 and sit in front of the variables in the first layer, which is what the prefix
        kernel's gnf_made_prefix_ctx entry points evaluate (a caller of such a plan hands the context over)."""
        cond_in = int(getattr(self, "cond_in", 0))
        if cond_in != 0 and not with_context:
            return None
        with_context = cond_in != 0                      # (cond_in == 0: one plan, one cache entry, whatever the flag)
        layers = self.masked_layers()
        specs = [l.degree_spec() for l in layers]
        if any(s is None for s in specs):
            return None
        key = (tuple(l._deg_checked for l in layers), layers[0].weight.device, bool(with_context))
        cache = self._prefix_cache
        if cache is None or cache[0] is not self.m or cache[1] != key:
            L, dev = len(self.hidden_sizes), layers[0].weight.device
            reps = self.nout // self.nin
            din = {l: self.m[l] for l in range(-1, L)}
            if cond_in:
                din[-1] = np.concatenate([np.full(cond_in, -1, dtype=self.m[-1].dtype), self.m[-1]])
            want = [(self.m[l], din[l - 1], False) for l in range(L)] + [(np.tile(self.m[-1], reps), din[L - 1], True)]
            same = all(strict == ws and np.array_equal(do.cpu().numpy(), np.asarray(wo, dtype=np.float32))
                       and np.array_equal(di.cpu().numpy(), np.asarray(wi, dtype=np.float32))
                       for (do, di, strict), (wo, wi, ws) in zip(specs, want))
            plan = None
            if same:
                plan = made_prefix_plan(self.m, self.nin, self.nout)
                plan["var_host"] = [int(v) for v in plan["var_of_step"]]
                for k in ("order", "off"):
                    plan[k] = [torch.from_numpy(a).to(dev) for a in plan[k]]
                plan["var_of_step"] = torch.from_numpy(plan["var_of_step"]).to(dev)
                plan["cond_in"] = cond_in
            cache = self._prefix_cache = (self.m, key, plan)
        return cache[2]

    def forward(self, x):
        ls = self.masked_layers()
        y = ops.mlp(x, [(l.weight, l.bias) for l in ls], [l.mask for l in ls], degs=[l.degree_spec() for l in ls])
        return y.view(x.shape[0], -1, x.shape[1]).permute(0, 2, 1)


class ConditionnalMADE(MADE):
    """(sic) reference AutoregressiveConditioner.py:115-141, whose cond_in > 0 form cannot be constructed.  Here
    it is a MADE over the nin variables whose first MaskedLinear is [H1, cond_in + nin] -- the context columns first, the
    reference's cat((context, x), 1) -- with input degree -1 for the context columns: every hidden unit and, without hidden
    layers, every output sees the context, the outputs of the first variable in the order included.  Degrees, orderings
    (num_masks, random) and the output layout are those of MADE(nin, ...); cond_in == 0 IS that MADE.  With hidden layers
    the outputs of the degree-0 variable read no hidden unit (all hidden degrees are >= 0, the output rule is strict): they
    stay the output bias, as in the unconditional MADE, and only the other variables' outputs move with the context."""

    def __init__(self, nin, cond_in, hidden_sizes, nout, num_masks=1, natural_ordering=False, random=False,
                 device="cpu"):
        super().__init__(nin, hidden_sizes, nout, num_masks, natural_ordering, random, device, cond_in=cond_in)
        self.nin_non_cond = nin

    def forward(self, x, context=None):
        context = checked_context(context, self.cond_in, x)
        if context is None:
            return super().forward(x)
        ls = self.masked_layers()
        y = ops.mlp(torch.cat((context, x), 1), [(l.weight, l.bias) for l in ls], [l.mask for l in ls],
                    degs=[l.degree_spec() for l in ls])
        return y.view(x.shape[0], -1, self.nin).permute(0, 2, 1)


class AutoregressiveConditioner(Conditioner):
    """reference AutoregressiveConditioner.py:144-154: h[b,i,:] depends on x[b,:i] only.
    Returns a permuted [B,d,hs] view (strides (hs*d, 1, d)) exactly like the reference; the
    normalizer kernels take the strides as they are."""

    def __init__(self, in_size, hidden, out_size, cond_in=0):
        super(AutoregressiveConditioner, self).__init__()
        self.in_size = in_size
        self.cond_in = cond_in
        self.masked_autoregressive_net = ConditionnalMADE(in_size, cond_in=cond_in, hidden_sizes=hidden,
                                                          nout=out_size * in_size)

    def forward(self, x, context=None):
        return self.masked_autoregressive_net(x, context)

    def depth(self):
        return self.in_size - 1

    # -- column-by-column inversion (NormalizingFlowStep._invert_by_columns) ---------------------------------------------
    def prefix_plan(self, with_context=False):
        get = getattr(self.masked_autoregressive_net, "prefix_plan", None)
        if get is None:
            return None
        return get(with_context=True) if with_context else get()

    _held_prefix = None

    def _prefix_params(self):
        return [p for l in self.masked_autoregressive_net.masked_layers() for p in (l.weight, l.bias)]

    def hold_prefix_pack(self):
        """context manager: the degree-ordered weight image of the prefix kernel, built once for the step calls inside"""
        import contextlib

        @contextlib.contextmanager
        def hold():
            prev = self._held_prefix
            plan = self.prefix_plan(with_context=bool(self.cond_in))
            if prev is None and plan is not None:
                self._held_prefix = ops.made_prefix_pack(self._prefix_params(), plan)
            try:
                yield
            finally:
                self._held_prefix = prev
        return hold()

    def prefix_workspace(self, batch):
        return ops.made_prefix_workspace(self._prefix_params(), self.prefix_plan(with_context=bool(self.cond_in)), batch)

    def prefix_steps(self, z, x, t0, t1, mode, h_out=None, ws=None, context=None, spline=None, pin=None):
        """steps t0 <= t < t1 of the plan on the HIP prefix kernel (gnf_hip.ops.made_prefix_steps); `context`: the checked
        [B, cond_in] context of a conditional conditioner (the plan is then prefix_plan(with_context=True)); `spline`:
        (nb_bins, tail_bound) for ops.MADE_NORM_SPLINE; `pin`: the uint8 [d] pin table, by variable, of an intervention
        (a pinned step reads its column of x)"""
        plan, params = self.prefix_plan(with_context=bool(self.cond_in)), self._prefix_params()
        pack = self._held_prefix if self._held_prefix is not None else ops.made_prefix_pack(params, plan)
        return ops.made_prefix_steps(params, plan, pack, z, x, t0, t1, mode, h_out=h_out, ws=ws, context=context,
                                     spline=spline, pin=pin)

    # -- the adjoint of that sweep (NormalizingFlowStep.rsample's backward) -------------------------------------------------
    _held_adjoint = None

    def hold_adjoint_pack(self):
        """context manager: the adjoint kernel's weight image (the prefix image and every layer transposed), built once for
        the adjoint_solve calls inside"""
        import contextlib

        @contextlib.contextmanager
        def hold():
            prev = self._held_adjoint
            plan = self.prefix_plan(with_context=bool(self.cond_in))
            if prev is None and plan is not None:
                self._held_adjoint = ops.made_adjoint_pack(self._prefix_params(), plan)
            try:
                yield
            finally:
                self._held_adjoint = prev
        return hold()

    def adjoint_solve(self, x, g, jac, dzdh, context=None, pin=None, want_gdo=False):
        """lambda [B, d] with J^T lambda = g for the step whose sample is x, on the HIP adjoint kernel (gnf_hip.ops.made_adjoint,
        one launch): jac [B, d] the normalizer's dz_i/dx_i, dzdh [B, d, out] its dz_i/dh_i; `context`: the checked
        [B, cond_in] context of a conditional conditioner.  pin (uint8 [d] on the device, by variable): the solve under
        do(x_pin = v) -- lambda is 0 at a pinned column; want_gdo: (lambda, gdo) with gdo = dL/dv at the pinned columns"""
        plan, params = self.prefix_plan(with_context=bool(self.cond_in)), self._prefix_params()
        pack = self._held_adjoint if self._held_adjoint is not None else ops.made_adjoint_pack(params, plan)
        do = {} if pin is None and not want_gdo else {"pin": pin, "gdo": want_gdo}
        return ops.made_adjoint(params, plan, pack, x, g, jac, dzdh, context=context, **do)
