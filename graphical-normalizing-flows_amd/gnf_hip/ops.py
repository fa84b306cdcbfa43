"""torch.autograd wrappers around the C-ABI kernels (gnf_hip.abi).

PyTorch's role here is plumbing: tensor allocation, autograd graph bookkeeping and the
current HIP stream.  Every numerical step of the flow hot path runs in libgnf_hip.so."""
import ctypes
import math
import os

import weakref

import numpy as np

import torch

from . import abi
from .abi import ptr, stream, call


def _empty(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _ws(nbytes, like):
    return torch.empty(max(int(nbytes) // 4, 1), dtype=torch.float32, device=like.device)


# ----------------------------------------------------------------------------- gradient slots
# A training state that keeps every gradient in ONE flat buffer (dp.FlatState: one all-reduce, one Adam launch) registers
# the slot of each parameter here; a backward that produces a parameter gradient writes it straight into the slot instead
# of a fresh tensor, and the state's gradient pack finds it already in place (no concatenation launch, 12.8 MB less
# traffic per MADE step).  A slot is handed out once per pack: a parameter used twice in a graph, or a second micro-batch
# accumulating into `.grad`, gets a fresh tensor and autograd adds it as usual.
_grad_slots = {}                       # parameter data_ptr -> (weakref to the owning state, index into its params)


def register_grad_slots(owner, params):
    """owner: object with `grad_views` (one tensor per parameter, same numel) and a set `_taken`"""
    ref = weakref.ref(owner)
    for i, p in enumerate(params):
        _grad_slots[p.data_ptr()] = (ref, i)


def unregister_grad_slots(owner):
    """drop the slots of `owner` (dp.FlatState.__del__ / close).  Lookups are safe without it -- a parameter of a live state
    is a view of the state's own flat buffer, so its address cannot be handed to anybody else, and an entry whose owner has
    died is deleted by the lookup that finds it -- but a dead state should not leave entries behind."""
    for k in [k for k, (ref, _) in _grad_slots.items() if ref() is owner or ref() is None]:
        del _grad_slots[k]


def grad_out(p):
    """the tensor a backward writes the gradient of parameter (or saved alias of it) `p` into"""
    ent = _grad_slots.get(p.data_ptr())
    if ent is not None:
        owner = ent[0]()
        if owner is None:
            del _grad_slots[p.data_ptr()]
        else:
            i = ent[1]
            v = owner.grad_views[i]
            if (i not in owner._taken and v.numel() == p.numel() and p.is_contiguous() and v.device == p.device
                    and v.dtype == p.dtype):
                owner._taken.add(i)
                return v.view(p.shape)
    return torch.empty_like(p)


_open_slots = set()                    # (id(owner), index) of shared slots taken in the backward pass that is running NOW


def _close_slots():
    _open_slots.clear()


def grad_out_shared(p, accumulate_ok=False):
    """(tensor, finish, accumulate) for a parameter that receives SEVERAL gradient contributions per backward (the DAG matrix A: gate
    and acyclicity term).  The first contribution takes the flat-buffer slot as grad_out does; a later one OF THE SAME
    BACKWARD PASS is written to a scratch tensor and finish() adds it INTO the slot and returns None, so autograd sees one
    contribution -- the slot -- instead of summing two tensors into a third that the gradient pack then copies (add +
    2.4 MB copy per cfg4 step).  "Same pass" is tracked by a callback the autograd engine runs when the pass ends: a slot
    left taken by an earlier pass (a backward without a gradient pack behind it, a previous micro-batch) is never added
    into -- that contribution gets a fresh tensor and autograd sums as usual.  finish(t) returns what the backward hands
    to autograd.  accumulate_ok: the caller's kernel can add into its output; a later contribution then gets the slot
    itself with accumulate = True (no scratch tensor, no add launch)."""
    ent = _grad_slots.get(p.data_ptr())
    owner = ent[0]() if ent is not None else None
    if owner is not None:
        i = ent[1]
        v = owner.grad_views[i]
        if v.numel() == p.numel() and p.is_contiguous() and v.device == p.device and v.dtype == p.dtype:
            key = (id(owner), i)
            if i not in owner._taken:
                owner._taken.add(i)
                if not _open_slots:
                    torch.autograd.Variable._execution_engine.queue_callback(_close_slots)
                _open_slots.add(key)
                return v.view(p.shape), (lambda t: t), False
            if key in _open_slots:
                if accumulate_ok:                                   # the caller's kernel adds INTO the slot itself
                    return v.view(p.shape), (lambda t: None), True

                def finish(t, v=v):
                    v.add_(t.reshape(-1))
                    return None
                return torch.empty_like(p), finish, False
    return torch.empty_like(p), (lambda t: t), False


# ----------------------------------------------------------------------------- Affine normalizer
class AffineFn(torch.autograd.Function):
    """(z, jac, logdet, logn) of models/Normalizers/AffineNormalizer.py:9-12 fused with the log|det J| row reduction of
    models/NormalizingFlow.py:70 and (want_logn) the Normal log-density of z (NormalizingFlowFactories.py:15-16): the
    pass that produces z also reduces it, and the backward recomputes z instead of reading it."""

    @staticmethod
    def forward(ctx, x, h, clamp_inplace=False, want_jac=True, want_logn=False):
        x = x.contiguous()
        B, d = x.shape
        ctx.set_materialize_grads(False)     # a step that only uses logdet / logn must not get zero tensors for z and jac
        z, logdet = _empty((B, d), x), _empty((B,), x)
        jac = _empty((B, d), x) if want_jac else None       # the fused step only needs log|det J|: 4 B/elem less traffic
        logn = _empty((B,), x) if want_logn else None
        h_bwd = h.detach().clone() if clamp_inplace else h
        call("gnf_affine_fwd", ptr(x), ptr(h), h.stride(0), h.stride(1), h.stride(2), ptr(z), ptr(jac), ptr(logdet),
             ptr(logn), int(bool(clamp_inplace)), B, d, stream())
        ctx.save_for_backward(x, h_bwd)
        ctx.hshape = tuple(h.shape)
        if jac is None:
            jac = z.new_empty(0)
            ctx.mark_non_differentiable(jac)
        if logn is None:
            logn = z.new_empty(0)
            ctx.mark_non_differentiable(logn)
        return z, jac, logdet, logn

    @staticmethod
    def backward(ctx, gz, gjac, glogdet, glogn=None):
        x, h = ctx.saved_tensors
        B, d = x.shape
        hs = ctx.hshape[2]
        # same memory format as h so that e.g. MADE's permuted view flows back without a copy
        gh = torch.empty_like(h) if hs == 2 else torch.zeros_like(h)
        gx = _empty((B, d), x) if ctx.needs_input_grad[0] else None
        call("gnf_affine_bwd", ptr(x), ptr(h), h.stride(0), h.stride(1), h.stride(2),
             ptr(gz.contiguous()) if gz is not None else None,
             ptr(gjac.contiguous()) if (gjac is not None and gjac.numel() > 0) else None,
             ptr(glogdet.contiguous()) if glogdet is not None else None,
             ptr(glogn.contiguous()) if (glogn is not None and glogn.numel() > 0) else None,
             ptr(gx), ptr(gh), gh.stride(0), gh.stride(1), gh.stride(2), B, d, stream())
        return gx, gh, None, None, None


def affine_inverse(z, h):
    """(z - mu)/sigma   (AffineNormalizer.py:14-17)."""
    z = z.contiguous()
    B, d = z.shape
    x = _empty((B, d), z)
    call("gnf_affine_inv", ptr(z), ptr(h), h.stride(0), h.stride(1), h.stride(2), ptr(x), B, d, stream())
    return x


# ----------------------------------------------------------------------------- Spline normalizer
def _spline_args(h, nb_bins, tail_bound):
    """(K, T) checked against the conditioner output h [.., .., C]: ValueError before anything is launched"""
    K, T = int(nb_bins), float(tail_bound)
    if not abi.SPLINE_MIN_BINS <= K <= abi.SPLINE_MAX_BINS:
        raise ValueError("spline: nb_bins = %d, must be %d .. %d" % (K, abi.SPLINE_MIN_BINS, abi.SPLINE_MAX_BINS))
    if not (T > 0. and math.isfinite(T)):
        raise ValueError("spline: tail_bound = %r, must be positive and finite" % (tail_bound,))
    if h.dim() != 3 or h.shape[2] < 3 * K - 1:
        raise ValueError("spline: %d bins read 3 K - 1 = %d conditioner outputs per variable, h is %s"
                         % (K, 3 * K - 1, tuple(h.shape)))
    return K, T


class SplineFn(torch.autograd.Function):
    """(z, jac, logdet, logn) of the monotone rational-quadratic spline with K bins on [-T, T] (include/gnf_hip.h,
    gnf_spline_fwd), the two row reductions fused as in AffineFn; the backward recomputes the forward."""

    @staticmethod
    def forward(ctx, x, h, nb_bins=8, tail_bound=3., want_jac=True, want_logn=False):
        K, T = _spline_args(h, nb_bins, tail_bound)
        x = x.contiguous()
        B, d = x.shape
        ctx.set_materialize_grads(False)     # a step that only uses logdet / logn must not get zero tensors for z and jac
        z, logdet = _empty((B, d), x), _empty((B,), x)
        jac = _empty((B, d), x) if want_jac else None
        logn = _empty((B,), x) if want_logn else None
        call("gnf_spline_fwd", ptr(x), ptr(h), h.stride(0), h.stride(1), h.stride(2), h.shape[2], K, T, ptr(z), ptr(jac),
             ptr(logdet), ptr(logn), B, d, stream())
        ctx.save_for_backward(x, h)
        ctx.KT = (K, T)
        if jac is None:
            jac = z.new_empty(0)
            ctx.mark_non_differentiable(jac)
        if logn is None:
            logn = z.new_empty(0)
            ctx.mark_non_differentiable(logn)
        return z, jac, logdet, logn

    @staticmethod
    def backward(ctx, gz, gjac, glogdet, glogn=None):
        x, h = ctx.saved_tensors
        B, d = x.shape
        K, T = ctx.KT
        # same memory format as h so that e.g. MADE's permuted view flows back without a copy
        gh = torch.empty_like(h) if h.shape[2] == 3 * K - 1 else torch.zeros_like(h)
        gx = _empty((B, d), x) if ctx.needs_input_grad[0] else None
        call("gnf_spline_bwd", ptr(x), ptr(h), h.stride(0), h.stride(1), h.stride(2), h.shape[2], K, T,
             ptr(gz.contiguous()) if gz is not None else None,
             ptr(gjac.contiguous()) if (gjac is not None and gjac.numel() > 0) else None,
             ptr(glogdet.contiguous()) if glogdet is not None else None,
             ptr(glogn.contiguous()) if (glogn is not None and glogn.numel() > 0) else None,
             ptr(gx), ptr(gh), gh.stride(0), gh.stride(1), gh.stride(2), B, d, stream())
        return gx, gh, None, None, None, None


def spline_inverse(z, h, nb_bins=8, tail_bound=3., out=None, out_cols=None):
    """the spline's closed-form inverse (gnf_spline_inv).  out / out_cols: write the TRANSPOSED result into columns out_cols
    of `out`, as monotonic_inverse does for the level and column schedules (z [variables, batch], out [batch, d])."""
    K, T = _spline_args(h, nb_bins, tail_bound)
    z = z.contiguous()
    B, d = z.shape
    if out is not None:
        assert out.is_contiguous() and out.dtype == torch.float32 and out.shape[0] == d and out_cols.dtype == torch.int32
        assert out_cols.numel() == B and out_cols.device == z.device
        if z.numel() == 0:                   # no variable or no sample (an empty batch is the SECOND dimension here)
            return out
        call("gnf_spline_inv", ptr(z), ptr(h), h.stride(0), h.stride(1), h.stride(2), h.shape[2], K, T, ptr(out),
             abi.rawptr(out_cols), out.shape[1], B, d, stream())
        return out
    x = _empty((B, d), z)
    if z.numel():
        call("gnf_spline_inv", ptr(z), ptr(h), h.stride(0), h.stride(1), h.stride(2), h.shape[2], K, T, ptr(x), None, 0, B,
             d, stream())
    return x


# ----------------------------------------------------------------------------- MADE prefix evaluation
MADE_NORM_NONE, MADE_NORM_AFFINE, MADE_NORM_SPLINE = abi.MADE_NORM_NONE, abi.MADE_NORM_AFFINE, abi.MADE_NORM_SPLINE


def _made_net(params, plan):
    """params: [W0, b0, ..., W_out, b_out] (nn.Linear layout) of a MADE; plan: MADE.prefix_plan() -> gnf_made_net.  The
    returned struct holds raw pointers: the caller keeps params and plan alive while it is in use.  A conditional plan
    (prefix_plan(with_context=True), plan["cond_in"] = c > 0) has the c context columns in front of the variables in the
    first layer: W0 is [rows, c + d]."""
    nh = len(plan["widths"])
    if len(params) != 2 * (nh + 1) or nh > abi.MADE_MAX_HIDDEN:
        raise abi.GnfError("MADE prefix kernel: 0..%d hidden layers, one (weight, bias) pair per layer"
                           % abi.MADE_MAX_HIDDEN)
    net = abi.MadeNet()
    net.nh, net.d, net.out, net.max_new = nh, plan["d"], plan["out"], plan["max_new"]
    fan_in = plan["d"] + _plan_cond_in(plan)
    for l in range(nh + 1):
        W, b = params[2 * l], params[2 * l + 1]
        rows = plan["widths"][l] if l < nh else plan["d"] * plan["out"]
        if tuple(W.shape) != (rows, fan_in) or tuple(b.shape) != (rows,) or not (W.is_contiguous() and b.is_contiguous()):
            raise abi.GnfError("MADE prefix kernel: layer %d is not a contiguous [%d, %d] Linear" % (l, rows, fan_in))
        net.W[l], net.b[l] = ptr(W).value, ptr(b).value
        if l < nh:
            net.width[l] = rows
            net.order[l] = abi.rawptr(plan["order"][l]).value
            net.off[l] = abi.rawptr(plan["off"][l]).value
            fan_in = rows
    net.var_of_step = abi.rawptr(plan["var_of_step"]).value
    return net


def _plan_cond_in(plan):
    c = int(plan.get("cond_in", 0))
    if c < 0:
        raise abi.GnfError("MADE prefix kernel: cond_in = %d" % c)
    return c


@torch.no_grad()
def made_prefix_pack(params, plan):
    """the prefix kernel's weight image (weights and biases in degree order): parameter-only, one launch; a caller that
    steps through an inversion builds it once (AutoregressiveConditioner.hold_prefix_pack)"""
    params = [p.detach() for p in params]
    net, c = _made_net(params, plan), _plan_cond_in(plan)
    nfl = abi.load().gnf_made_prefix_ctx_pack_floats(ctypes.byref(net), c)       # (c = 0: the unconditional image)
    if nfl < 0:
        abi.check(int(nfl), "gnf_made_prefix_ctx_pack_floats")
    pack = _empty((int(nfl),), params[0])
    call("gnf_made_prefix_ctx_pack", ctypes.byref(net), c, ptr(pack), stream())
    return pack


@torch.no_grad()
def made_prefix_workspace(params, plan, batch):
    """the activation workspace that carries an inversion of `batch` rows from one made_prefix_steps call to the next"""
    params = [p.detach() for p in params]
    net, c = _made_net(params, plan), _plan_cond_in(plan)
    nbytes = abi.load().gnf_made_prefix_ctx_ws_bytes(ctypes.byref(net), c, int(batch))
    if nbytes < 0:
        abi.check(int(nbytes), "gnf_made_prefix_ctx_ws_bytes")
    return _ws(nbytes, params[0])


@torch.no_grad()
def made_prefix_steps(params, plan, pack, z, x, t0, t1, mode, h_out=None, ws=None, context=None, spline=None, pin=None):
    """Steps t0 <= t < t1 of the column-by-column inversion of a MADE step: z, x [B, d] fp32 contiguous.  Every call runs on
    gnf_made_prefix_do, the entry point whose arguments superset the other four's (NULL context, no bins, NULL table).
    MADE_NORM_AFFINE writes column var_of_step[t] of x per step ((0, d): the whole inversion, one launch);
    MADE_NORM_NONE (t1 == t0 + 1) writes the conditioner outputs of that variable to h_out [B, out] and leaves the column
    to the caller.  ws (made_prefix_workspace): the same buffer for every call of one inversion; allocated here when a call
    that needs one comes without.  context: the contiguous fp32 [B, cond_in] device tensor of a conditional plan, None for
    cond_in == 0.  MADE_NORM_SPLINE takes spline = (nb_bins, tail_bound).  pin: the contiguous uint8 [d] device table of an
    intervention, one byte per VARIABLE, non-zero = pinned: a pinned step reads its column of x, which the caller filled,
    and writes nothing; MADE_NORM_NONE may then span t1 > t0 + 1 steps whose all but the last are pinned (the library
    checks that against the table, at the price of a stream synchronisation)."""
    params = [p.detach() for p in params]
    net, c = _made_net(params, plan), _plan_cond_in(plan)
    B, d = x.shape
    if pin is not None and (pin.dtype != torch.uint8 or pin.device != x.device or tuple(pin.shape) != (plan["d"],)
                            or not pin.is_contiguous()):
        raise abi.GnfError("made_prefix_steps: pin must be a contiguous uint8 [%d] tensor on the device of x" % plan["d"])
    if d != plan["d"] or not x.is_contiguous() or (z is not None and (tuple(z.shape) != (B, d) or not z.is_contiguous())):
        raise abi.GnfError("made_prefix_steps: z and x must be contiguous [B, %d]" % plan["d"])
    if h_out is not None and (tuple(h_out.shape) != (B, plan["out"]) or not h_out.is_contiguous()):
        raise abi.GnfError("made_prefix_steps: h_out must be contiguous [B, %d]" % plan["out"])
    if c == 0 and context is not None:
        raise abi.GnfError("made_prefix_steps: a context for a plan with cond_in = 0")
    if c and (context is None or not context.is_cuda or context.device != x.device or context.dtype != torch.float32
              or tuple(context.shape) != (B, c) or not context.is_contiguous()):
        raise abi.GnfError("made_prefix_steps: context must be a contiguous fp32 [B, %d] tensor on the device of x" % c)
    if ws is None and not (t0 == 0 and t1 == d):
        ws = made_prefix_workspace(params, plan, B)
    bins, tail = 0, 0.
    if int(mode) == MADE_NORM_SPLINE:
        if spline is None:
            raise abi.GnfError("made_prefix_steps: MADE_NORM_SPLINE needs spline = (nb_bins, tail_bound)")
        bins, tail = int(spline[0]), float(spline[1])
    args = lambda w: (ctypes.byref(net), c, ptr(context), ptr(pack), ptr(z), ptr(x), ptr(h_out), int(t0), int(t1), int(mode),
                      bins, tail, None if pin is None else ctypes.c_void_p(pin.data_ptr()), B,
                      None if w is None else ctypes.c_void_p(w.data_ptr()), 0 if w is None else w.numel() * 4, stream())
    if ws is None:
        # a whole inversion whose tile of activations fits in LDS needs no workspace; the library says when it does not
        rc = abi.load().gnf_made_prefix_do(*args(None))
        if rc == 0:
            return x
        if rc != -3:
            abi.check(rc, "gnf_made_prefix_do")
        ws = made_prefix_workspace(params, plan, B)
    call("gnf_made_prefix_do", *args(ws))
    return x


# ----------------------------------------------------------------------------- StrADE level sweep
def _strade_net(params, masks, plan):
    """params [W0, b0, ..., W_out, b_out], masks [M0, ..., M_out] (fp32, the layout of the weights) of a StrADE net; plan:
    StrADEConditioner.level_plan() -> gnf_strade_net: the gnf_made_net of _made_net with the plan's level tables where the
    degree tables stand, the masks and the level offsets.  Raw pointers: the caller keeps all three alive."""
    net = abi.StradeNet()
    net.made = _made_net(params, {"widths": plan["widths"], "d": plan["d"], "out": plan["out"], "max_new": plan["max_new"],
                                  "cond_in": plan["cond_in"], "order": plan["order"], "off": plan["off"],
                                  "var_of_step": plan["var_order"]})
    if len(masks) != len(params) // 2:
        raise abi.GnfError("StrADE level kernel: one mask per layer")
    for l, M in enumerate(masks):
        W = params[2 * l]
        if tuple(M.shape) != tuple(W.shape) or M.device != W.device or not M.is_contiguous():
            raise abi.GnfError("StrADE level kernel: mask %d is not a contiguous fp32 %s tensor on the weights' device"
                               % (l, tuple(W.shape)))
        net.mask[l] = ptr(M).value
    net.var_off = abi.rawptr(plan["var_off"]).value
    net.nlev, net.widest = plan["nlev"], plan["widest"]
    return net


@torch.no_grad()
def strade_pack(params, masks, plan):
    """the level kernel's weight image (mask o W and the biases in level order, a masked entry an exact zero):
    parameter-only, one launch (StrADEConditioner.hold_level_pack builds it once for several sweeps)"""
    params = [p.detach() for p in params]
    net, c = _strade_net(params, masks, plan), _plan_cond_in(plan)
    nfl = abi.load().gnf_strade_pack_floats(ctypes.byref(net), c)
    if nfl < 0:
        abi.check(int(nfl), "gnf_strade_pack_floats")
    pack = _empty((int(nfl),), params[0])
    call("gnf_strade_pack", ctypes.byref(net), c, ptr(pack), stream())
    return pack


@torch.no_grad()
def strade_levels(params, masks, plan, pack, z, x, mode, context=None, spline=None, pin=None):
    """The level-by-level inversion of a StrADE step, one launch of gnf_strade_levels: z, x [B, d] fp32 contiguous, x written
    column by column (MADE_NORM_AFFINE, or MADE_NORM_SPLINE with spline = (nb_bins, tail_bound)).  context: the contiguous
    fp32 [B, cond_in] device tensor of a conditional plan.  pin: the contiguous uint8 [d] device table of an intervention,
    one byte per VARIABLE, non-zero = pinned: such a column of x, which the caller filled, is read and handed on.
    Returns x -- or None, having launched nothing, where the library answers GNF_ESHAPE (the net's rows do not fit the
    kernel's LDS tile, or the normalizer needs more outputs than the net has): the caller inverts by passes.  An empty
    batch launches nothing."""
    params = [p.detach() for p in params]
    net, c = _strade_net(params, masks, plan), _plan_cond_in(plan)
    B, d = x.shape
    if pin is not None and (pin.dtype != torch.uint8 or pin.device != x.device or tuple(pin.shape) != (plan["d"],)
                            or not pin.is_contiguous()):
        raise abi.GnfError("strade_levels: pin must be a contiguous uint8 [%d] tensor on the device of x" % plan["d"])
    if d != plan["d"] or not x.is_contiguous() or tuple(z.shape) != (B, d) or not z.is_contiguous() or z.device != x.device:
        raise abi.GnfError("strade_levels: z and x must be contiguous [B, %d] on one device" % plan["d"])
    if c == 0 and context is not None:
        raise abi.GnfError("strade_levels: a context for a plan with cond_in = 0")
    if c and (context is None or not context.is_cuda or context.device != x.device or context.dtype != torch.float32
              or tuple(context.shape) != (B, c) or not context.is_contiguous()):
        raise abi.GnfError("strade_levels: context must be a contiguous fp32 [B, %d] tensor on the device of x" % c)
    bins, tail = 0, 0.
    if int(mode) == MADE_NORM_SPLINE:
        if spline is None:
            raise abi.GnfError("strade_levels: MADE_NORM_SPLINE needs spline = (nb_bins, tail_bound)")
        bins, tail = int(spline[0]), float(spline[1])
    args = (ctypes.byref(net), c, ptr(context), ptr(pack), ptr(z), ptr(x), int(mode), bins, tail,
            None if pin is None else ctypes.c_void_p(pin.data_ptr()), B, stream())
    rc = int(abi.load().gnf_strade_levels(*args))       # (the shape checks come before any launch, also for B = 0)
    if rc == -2:
        return None
    abi.check(rc, "gnf_strade_levels")
    return x


# ----------------------------------------------------------------------------- MADE adjoint sweep, rsample
@torch.no_grad()
def made_adjoint_pack(params, plan):
    """the adjoint kernel's weight image: the prefix image followed by every layer transposed (gnf_made_adjoint_pack);
    parameter-only, one launch (AutoregressiveConditioner.hold_adjoint_pack builds it once for several solves)"""
    params = [p.detach() for p in params]
    net, c = _made_net(params, plan), _plan_cond_in(plan)
    nfl = abi.load().gnf_made_adjoint_pack_floats(ctypes.byref(net), c)
    if nfl < 0:
        abi.check(int(nfl), "gnf_made_adjoint_pack_floats")
    pack = _empty((int(nfl),), params[0])
    call("gnf_made_adjoint_pack", ctypes.byref(net), c, ptr(pack), stream())
    return pack


@torch.no_grad()
def made_adjoint(params, plan, pack, x, g, jac, dzdh, context=None, force_ws=False, pin=None, gdo=False):
    """lambda [B, d] with J^T lambda = g for the MADE step whose sample is x (gnf_made_adjoint, one launch): x, g, jac
    [B, d] and dzdh [B, d, out] fp32 contiguous, jac the normalizer's own derivative dz_i/dx_i, dzdh[b, i, :] = dz_bi/dh_bi;
    context: the contiguous [B, cond_in] tensor of a conditional plan.  force_ws (tests): keep the tile's rows in the
    workspace even when they fit in LDS -- the same bits.

    pin: the contiguous uint8 [d] device table of an intervention, one byte per VARIABLE, non-zero = pinned
    (gnf_made_adjoint_do): lambda is +0 at a pinned column and jac / dzdh are not read there.  gdo=True (with a table) returns
    (lambda, gdo): gdo = g - u = dL/dv at pinned columns, +0 at free ones.  Without a table the call is the un-pinned entry
    point, the same launch and bits."""
    params = [p.detach() for p in params]
    net, c = _made_net(params, plan), _plan_cond_in(plan)
    B, d = x.shape
    ok = lambda t, shape: (t.is_cuda and t.device == x.device and t.dtype == torch.float32 and tuple(t.shape) == shape
                           and t.is_contiguous())
    if d != plan["d"] or not (ok(x, (B, d)) and ok(g, (B, d)) and ok(jac, (B, d)) and ok(dzdh, (B, d, plan["out"]))):
        raise abi.GnfError("made_adjoint: x, g, jac [B, %d] and dzdh [B, %d, %d] must be contiguous fp32 device tensors"
                           % (plan["d"], plan["d"], plan["out"]))
    if (context is not None) != (c > 0) or (c > 0 and not ok(context, (B, c))):
        raise abi.GnfError("made_adjoint: context must be a contiguous fp32 [B, %d] tensor on the device of x (None for "
                           "cond_in = 0)" % c)
    if pin is not None and (pin.dtype != torch.uint8 or pin.device != x.device or tuple(pin.shape) != (plan["d"],)
                            or not pin.is_contiguous()):
        raise abi.GnfError("made_adjoint: pin must be a contiguous uint8 [%d] tensor on the device of x" % plan["d"])
    if gdo and pin is None:
        raise abi.GnfError("made_adjoint: gdo is the gradient of the pinned values: it needs a pin table")
    lam = torch.empty_like(x)
    gd = torch.empty_like(x) if gdo else None
    # the un-pinned entry point when there is no table: its call sites and counters stay as they are
    entry = "gnf_made_adjoint" if pin is None else "gnf_made_adjoint_do"
    do = () if pin is None else (ctypes.c_void_p(pin.data_ptr()), ptr(gd))
    args = lambda w: (ctypes.byref(net), c, ptr(context), ptr(pack), ptr(x), ptr(g), ptr(jac), ptr(dzdh), ptr(lam), *do, B,
                      int(bool(force_ws)), None if w is None else ctypes.c_void_p(w.data_ptr()),
                      0 if w is None else w.numel() * 4, stream())
    done = lambda: (lam, gd) if gdo else lam
    if not force_ws:
        # a tile whose rows fit in LDS needs no workspace; the library says when it does not
        rc = getattr(abi.load(), entry)(*args(None))
        if rc == 0:
            return done()
        if rc != -3:
            abi.check(rc, entry)
    nbytes = abi.load().gnf_made_adjoint_ws_bytes(ctypes.byref(net), c, B)
    if nbytes < 0:
        abi.check(int(nbytes), "gnf_made_adjoint_ws_bytes")
    call(entry, *args(_ws(nbytes, x)))
    return done()


# ----------------------------------------------------------------------------- StrADE adjoint sweep, rsample
@torch.no_grad()
def strade_adjoint_pack(params, masks, plan):
    """the StrADE adjoint kernel's weight image: the level image of strade_pack followed by every layer of mask o W
    transposed (gnf_strade_adjoint_pack); parameter-only, one launch (StrADEConditioner.hold_adjoint_pack builds it once
    for several solves)"""
    params = [p.detach() for p in params]
    net, c = _strade_net(params, masks, plan), _plan_cond_in(plan)
    nfl = abi.load().gnf_strade_adjoint_pack_floats(ctypes.byref(net), c)
    if nfl < 0:
        abi.check(int(nfl), "gnf_strade_adjoint_pack_floats")
    pack = _empty((int(nfl),), params[0])
    call("gnf_strade_adjoint_pack", ctypes.byref(net), c, ptr(pack), stream())
    return pack


@torch.no_grad()
def strade_adjoint(params, masks, plan, pack, x, g, jac, dzdh, context=None, force_ws=False, pin=None, gdo=False):
    """lambda [B, d] with J^T lambda = g for the StrADE step whose sample is x (gnf_strade_adjoint, one launch): x, g, jac
    [B, d] and dzdh [B, d, out] fp32 contiguous, jac the normalizer's own derivative dz_i/dx_i, dzdh[b, i, :] = dz_bi/dh_bi
    by variable index; context: the contiguous [B, cond_in] tensor of a conditional plan.  force_ws (tests): keep the
    tile's rows in the workspace even when they fit in LDS -- the same bits.  An empty batch launches nothing.

    pin: the contiguous uint8 [d] device table of an intervention, one byte per VARIABLE, non-zero = pinned
    (gnf_strade_adjoint_do): lambda is +0 at a pinned column and jac / dzdh are not read there.  gdo=True (with a table) returns
    (lambda, gdo): gdo = g - u = dL/dv at pinned columns, +0 at free ones.  Without a table the call is the un-pinned entry
    point, the same launch and bits."""
    params = [p.detach() for p in params]
    net, c = _strade_net(params, masks, plan), _plan_cond_in(plan)
    B, d = x.shape
    ok = lambda t, shape: (t.is_cuda and t.device == x.device and t.dtype == torch.float32 and tuple(t.shape) == shape
                           and t.is_contiguous())
    if d != plan["d"] or not (ok(x, (B, d)) and ok(g, (B, d)) and ok(jac, (B, d)) and ok(dzdh, (B, d, plan["out"]))):
        raise abi.GnfError("strade_adjoint: x, g, jac [B, %d] and dzdh [B, %d, %d] must be contiguous fp32 device tensors"
                           % (plan["d"], plan["d"], plan["out"]))
    if (context is not None) != (c > 0) or (c > 0 and not ok(context, (B, c))):
        raise abi.GnfError("strade_adjoint: context must be a contiguous fp32 [B, %d] tensor on the device of x (None for "
                           "cond_in = 0)" % c)
    if pin is not None and (pin.dtype != torch.uint8 or pin.device != x.device or tuple(pin.shape) != (plan["d"],)
                            or not pin.is_contiguous()):
        raise abi.GnfError("strade_adjoint: pin must be a contiguous uint8 [%d] tensor on the device of x" % plan["d"])
    if gdo and pin is None:
        raise abi.GnfError("strade_adjoint: gdo is the gradient of the pinned values: it needs a pin table")
    lam = torch.empty_like(x)
    gd = torch.empty_like(x) if gdo else None
    # the un-pinned entry point when there is no table: its call sites and counters stay as they are
    entry = "gnf_strade_adjoint" if pin is None else "gnf_strade_adjoint_do"
    do = () if pin is None else (ctypes.c_void_p(pin.data_ptr()), ptr(gd))
    args = lambda w: (ctypes.byref(net), c, ptr(context), ptr(pack), ptr(x), ptr(g), ptr(jac), ptr(dzdh), ptr(lam), *do, B,
                      int(bool(force_ws)), None if w is None else ctypes.c_void_p(w.data_ptr()),
                      0 if w is None else w.numel() * 4, stream())
    done = lambda: (lam, gd) if gdo else lam
    if not force_ws:
        # a tile whose rows fit in LDS needs no workspace; the library says when it does not
        rc = getattr(abi.load(), entry)(*args(None))
        if rc == 0:
            return done()
        if rc != -3:
            abi.check(rc, entry)
    nbytes = abi.load().gnf_strade_adjoint_workspace_bytes(ctypes.byref(net), c, B)
    if nbytes < 0:
        abi.check(int(nbytes), "gnf_strade_adjoint_workspace_bytes")
    call(entry, *args(_ws(nbytes, x)))
    return done()


class InvertFn(torch.autograd.Function):
    """x = step^-1(z; theta, context) with the gradient of the implicit function theorem (NormalizingFlowStep.rsample).
    Forward: step.invert, the same kernels and bits.  Backward, for a cotangent g = dL/dx: lambda solves J^T lambda = g
    with J = dz/dx of the step at the sample; dL/dz = lambda, and dL/dtheta, dL/dcontext are ONE vjp of the step's forward
    at x (detached) with cotangent -lambda.  `params` are the step's parameters, passed as inputs so that the gradients
    reach them (as MonotonicFn takes the integrand's)."""

    @staticmethod
    def forward(ctx, step, z, context, *params):
        x = step.invert(z, context)
        ctx.step = step
        ctx.has_context = context is not None
        ctx.save_for_backward(x, *(() if context is None else (context,)), *params)
        return x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, *rest = ctx.saved_tensors                    # (raises when a parameter was modified in place since the sample)
        context = rest.pop(0) if ctx.has_context else None
        lam, gctx, gparams = ctx.step._rsample_backward(x, context, rest, g.contiguous(), ctx.needs_input_grad[2])
        return (None, lam, gctx, *gparams)


class InterveneFn(torch.autograd.Function):
    """x = step.intervene(z, idx, vals, context) -- the same kernels, the same bits -- with the gradient of the implicit
    function theorem on the mutilated system (NormalizingFlowStep.rsample_do; the sibling of InvertFn).  The equations of
    the free variables are kept, those of the pinned ones are x_P = vals.  Backward, for g = dL/dx: lambda_P = 0,
    J_FF^T lambda_F = g_F; dL/dz = lambda (exact zeros at the pinned columns), dL/dvals = g_P - (N^T lambda)_P, and
    dL/dtheta, dL/dcontext are ONE vjp of the step's forward at x with cotangent -lambda.  `idx`: the pinned variables, a
    tuple of ints; `vals` [B, S]: their values (autograd's expand reduces the gradient to the caller's do_value)."""

    @staticmethod
    def forward(ctx, step, z, idx, vals, context, *params):
        x = step.intervene(z, list(idx), vals.detach(), context)
        ctx.step, ctx.idx = step, tuple(idx)
        ctx.has_context = context is not None
        ctx.save_for_backward(x, *(() if context is None else (context,)), *params)
        return x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, *rest = ctx.saved_tensors                    # (raises when a parameter was modified in place since the sample)
        context = rest.pop(0) if ctx.has_context else None
        lam, gvals, gctx, gparams = ctx.step._rsample_do_backward(x, context, rest, g.contiguous(), ctx.idx,
                                                                  ctx.needs_input_grad[4], ctx.needs_input_grad[3])
        return (None, lam, None, gvals, gctx, *gparams)


# ----------------------------------------------------------------------------- row reductions
class LogSumRowsFn(torch.autograd.Function):
    """torch.log(jac).sum(1)   (models/NormalizingFlow.py:70)."""

    @staticmethod
    def forward(ctx, jac):
        jac = jac.contiguous()
        B, d = jac.shape
        out = _empty((B,), jac)
        call("gnf_logsum_rows_fwd", ptr(jac), ptr(out), B, d, stream())
        ctx.save_for_backward(jac)
        return out

    @staticmethod
    def backward(ctx, g):
        jac, = ctx.saved_tensors
        B, d = jac.shape
        gj = _empty((B, d), jac)
        call("gnf_logsum_rows_bwd", ptr(jac), ptr(g.contiguous()), ptr(gj), B, d, stream())
        return gj


class NormalLogDensityFn(torch.autograd.Function):
    """-.5*(log(2 pi) + z**2).sum(1)   (models/NormalizingFlowFactories.py:15-16)."""

    @staticmethod
    def forward(ctx, z):
        z = z.contiguous()
        B, d = z.shape
        out = _empty((B,), z)
        call("gnf_normal_logdensity_fwd", ptr(z), ptr(out), B, d, stream())
        ctx.save_for_backward(z)
        return out

    @staticmethod
    def backward(ctx, g):
        z, = ctx.saved_tensors
        B, d = z.shape
        gz = _empty((B, d), z)
        call("gnf_normal_logdensity_bwd", ptr(z), ptr(g.contiguous()), ptr(gz), B, d, stream())
        return gz


class NllReduceFn(torch.autograd.Function):
    """(log(jac).sum(1), -.5*(log(2 pi) + z**2).sum(1)): the two row reductions of a flow step's tail
    (models/NormalizingFlow.py:70, NormalizingFlowFactories.py:15-16) in one pass over z and jac, and one backward
    launch producing both cotangents (the Monotonic normalizer's kernels cannot reduce over a row themselves)."""

    @staticmethod
    def forward(ctx, z, jac):
        z, jac = z.contiguous(), jac.contiguous()
        B, d = z.shape
        ctx.set_materialize_grads(False)
        logdet, logn = _empty((B,), z), _empty((B,), z)
        call("gnf_nll_reduce_fwd", ptr(z), ptr(jac), ptr(logdet), ptr(logn), B, d, stream())
        ctx.save_for_backward(z, jac)
        return logdet, logn

    @staticmethod
    def backward(ctx, glogdet, glogn):
        z, jac = ctx.saved_tensors
        B, d = z.shape
        gz, gjac = _empty((B, d), z), _empty((B, d), z)
        call("gnf_nll_reduce_bwd", ptr(z), ptr(jac), ptr(glogdet.contiguous()) if glogdet is not None else None,
             ptr(glogn.contiguous()) if glogn is not None else None, None, ptr(gz), ptr(gjac), B, d, stream())
        return gz, gjac


# ----------------------------------------------------------------------------- interventional likelihood
def _do_table(pin, regime, like):
    """(pin pointer, regime pointer or None, R) of a checked mask table for the masked reductions: pin uint8 [R, d] and
    regime int32 [B] or None, contiguous, on the device of `like` (models.NormalizingFlow.do_targets makes them)"""
    B, d = like.shape
    if pin.dtype != torch.uint8 or pin.dim() != 2 or pin.shape[1] != d or not pin.is_contiguous() or pin.device != like.device:
        raise ValueError("pin must be a contiguous uint8 [R, %d] table on %s, got %s %s on %s"
                         % (d, like.device, pin.dtype, tuple(pin.shape), pin.device))
    R = pin.shape[0]
    if regime is None:
        if R != 1 and R != B:
            raise ValueError("pin has %d rows: without a regime vector it must have 1 or B = %d" % (R, B))
        return abi.rawptr(pin), None, R
    if (regime.dtype != torch.int32 or tuple(regime.shape) != (B,) or not regime.is_contiguous()
            or regime.device != like.device):
        raise ValueError("regime must be a contiguous int32 [%d] vector on %s, got %s %s on %s"
                         % (B, like.device, regime.dtype, tuple(regime.shape), regime.device))
    return abi.rawptr(pin), abi.rawptr(regime), R


class NllDoFn(torch.autograd.Function):
    """NllReduceFn over the FREE variables only: (sum_free log jac, -.5 sum_free (log 2 pi + z^2)), the truncated
    factorisation log p(x | do(x_S)) behind any normalizer's (z, jac).  pin [R, d] uint8 (non-zero: pinned), regime int32 [B]
    or None (R = 1: one target set for the batch, R = B: a row per sample).  A pinned element's z and jac never enter a sum or
    a cotangent; a regime id outside [0, R) gives NaN rows.  pin and regime carry no gradient."""

    @staticmethod
    def forward(ctx, z, jac, pin, regime=None):
        z, jac = z.contiguous(), jac.contiguous()
        B, d = z.shape
        ctx.set_materialize_grads(False)
        p, r, R = _do_table(pin, regime, z)
        logdet, logn = _empty((B,), z), _empty((B,), z)
        call("gnf_nll_do_fwd", ptr(z), ptr(jac), p, r, R, ptr(logdet), ptr(logn), B, d, stream())
        ctx.save_for_backward(z, jac, pin, *([] if regime is None else [regime]))
        return logdet, logn

    @staticmethod
    def backward(ctx, glogdet, glogn):
        z, jac, pin, *rest = ctx.saved_tensors
        regime = rest[0] if rest else None
        B, d = z.shape
        p, r, R = _do_table(pin, regime, z)
        gz, gjac = _empty((B, d), z), _empty((B, d), z)
        call("gnf_nll_do_bwd", ptr(z), ptr(jac), p, r, R, ptr(glogdet.contiguous()) if glogdet is not None else None,
             ptr(glogn.contiguous()) if glogn is not None else None, None, ptr(gz), ptr(gjac), B, d, stream())
        return gz, gjac, None, None


class AffineDoFn(torch.autograd.Function):
    """AffineFn (without the in-place clamp) with log|det J| and the Normal log-density reduced over the FREE columns in the
    pass that writes z: (z, jac, logdet, logn) under do(x_S).  z is written for every column -- a pinned column's z is
    defined and unused --, the row cotangents of logdet / logn reach x and h through free elements only, those of z and jac
    act on every element.  Both layouts of h (contiguous [B, d, 2], MADE's permuted view); gh comes back in h's format."""

    @staticmethod
    def forward(ctx, x, h, pin, regime=None, want_jac=False):
        x = x.contiguous()
        B, d = x.shape
        ctx.set_materialize_grads(False)
        if h.dim() != 3 or h.shape[0] != B or h.shape[1] != d or h.shape[2] < 2:
            raise ValueError("AffineDoFn: h must be [%d, %d, >= 2], got %s" % (B, d, tuple(h.shape)))
        p, r, R = _do_table(pin, regime, x)
        z, logdet, logn = _empty((B, d), x), _empty((B,), x), _empty((B,), x)
        jac = _empty((B, d), x) if want_jac else None
        call("gnf_affine_do_fwd", ptr(x), ptr(h), h.stride(0), h.stride(1), h.stride(2), p, r, R, ptr(z), ptr(jac),
             ptr(logdet), ptr(logn), B, d, stream())
        ctx.save_for_backward(x, h, pin, *([] if regime is None else [regime]))
        ctx.hshape = tuple(h.shape)
        if jac is None:
            jac = z.new_empty(0)
            ctx.mark_non_differentiable(jac)
        return z, jac, logdet, logn

    @staticmethod
    def backward(ctx, gz, gjac, glogdet, glogn):
        x, h, pin, *rest = ctx.saved_tensors
        regime = rest[0] if rest else None
        B, d = x.shape
        p, r, R = _do_table(pin, regime, x)
        # same memory format as h so that e.g. MADE's permuted view flows back without a copy
        gh = torch.empty_like(h) if ctx.hshape[2] == 2 else torch.zeros_like(h)
        gx = _empty((B, d), x) if ctx.needs_input_grad[0] else None
        call("gnf_affine_do_bwd", ptr(x), ptr(h), h.stride(0), h.stride(1), h.stride(2), p, r, R,
             ptr(gz.contiguous()) if gz is not None else None,
             ptr(gjac.contiguous()) if (gjac is not None and gjac.numel() > 0) else None,
             ptr(glogdet.contiguous()) if glogdet is not None else None,
             ptr(glogn.contiguous()) if glogn is not None else None,
             ptr(gx), ptr(gh), gh.stride(0), gh.stride(1), gh.stride(2), B, d, stream())
        return gx, gh, None, None, None


class NllMeanFn(torch.autograd.Function):
    """addend - (logdet + logn).mean(): FCNormalizingFlow.loss (models/NormalizingFlow.py:144-146; addend = the constraints
    term as a 0-dim tensor, or None) and its cotangents, one launch each way."""

    @staticmethod
    def forward(ctx, logdet, logn, addend=None):
        logdet, logn = logdet.contiguous(), logn.contiguous()
        out = _empty((), logdet)
        call("gnf_nll_mean_fwd", ptr(logdet), ptr(logn), ptr(addend), ptr(out), logdet.shape[0], stream())
        ctx.B = logdet.shape[0]
        ctx.like = logdet
        return out

    @staticmethod
    def backward(ctx, g):
        gl, gn = _empty((ctx.B,), ctx.like), _empty((ctx.B,), ctx.like)
        call("gnf_nll_mean_bwd", ptr(g.contiguous()), ptr(gl), ptr(gn), ctx.B, stream())
        return gl, gn, (g if len(ctx.needs_input_grad) > 2 and ctx.needs_input_grad[2] else None)


class NllLossFn(torch.autograd.Function):
    """addend - (logdet + logN(z)).mean() with the Normal log-density computed from z ITSELF inside the loss launch
    (FCNormalizingFlow.loss, models/NormalizingFlow.py:144-146 with NormalizingFlowFactories.py:15-16): one launch each
    way.  Until round 4 the density was reduced by the kernel that produced z and remembered on the tensor; a z rewritten
    through `.data` (no version bump) was then scored with the old density.  Now the loss reads the z it is handed."""

    @staticmethod
    def forward(ctx, z, logdet, addend=None):
        z, logdet = z.contiguous(), logdet.contiguous()
        B, d = z.shape
        out = _empty((), z)
        call("gnf_nll_loss_fwd", ptr(z), ptr(logdet), ptr(addend), ptr(out), B, d, stream())
        ctx.save_for_backward(z)
        return out

    @staticmethod
    def backward(ctx, g):
        z, = ctx.saved_tensors
        B, d = z.shape
        gz, gl = _empty((B, d), z), _empty((B,), z)
        call("gnf_nll_loss_bwd", ptr(g.contiguous()), ptr(z), ptr(gz), ptr(gl), B, d, stream())
        return gz, gl, (g if len(ctx.needs_input_grad) > 2 and ctx.needs_input_grad[2] else None)


_LOSS_MAX = None


def nll_loss_fits(z):
    """True when NllLossFn takes this z (one workgroup reads all of it: up to 2^20 elements)"""
    global _LOSS_MAX
    if _LOSS_MAX is None:
        _LOSS_MAX = int(abi.load().gnf_nll_loss_max_elems())
    return z.dim() == 2 and 0 < z.numel() <= _LOSS_MAX


def colsum(a):
    """sum over rows of a contiguous [M,N] tensor (bias gradients)."""
    M, N = a.shape
    out = _empty((N,), a)
    ws = _ws(abi.load().gnf_colsum_ws_bytes(M, N), a)
    call("gnf_colsum", ptr(a), N, ptr(out), M, N, ptr(ws), stream())
    return out


# ----------------------------------------------------------------------------- MFMA GEMM / MLP chains
def gemm(A, a_strides, Bm, b_strides, C, c_strides, M, N, K, Bmask=None, bias=None, Cmask=None, cm_strides=(0, 0),
         gate=None, g_strides=(0, 0), relu=False):
    nws = abi.load().gnf_gemm_ws_bytes(M, N, K)
    ws = _ws(nws, C) if nws > 0 else None
    call("gnf_gemm", ptr(A), a_strides[0], a_strides[1], ptr(Bm), ptr(Bmask), b_strides[0], b_strides[1], ptr(C),
         c_strides[0], c_strides[1], ptr(bias), ptr(Cmask), cm_strides[0], cm_strides[1], ptr(gate), g_strides[0],
         g_strides[1], 1 if relu else 0, M, N, K, ptr(ws), nws, stream())


class MLPFn(torch.autograd.Function):
    """y = L_n(relu(L_{n-1}(... relu(L_1(x))))), L_i(a) = a @ (mask_i * W_i)^T + b_i.

    One Function for every Linear/ReLU chain of the conditioners: CouplingMLP
    (CouplingConditioner.py:6-19), DAGMLP (DAGConditioner.py:7-20), MADE's masked linears
    (AutoregressiveConditioner.py:14-25, mask fused into the weight load instead of a
    mask*weight product per forward), MNISTCNN.fc1/fc2 (MLP.py:44-47).  The backward fuses the
    ReLU gate into the epilogue of the data-gradient kernel, the mask into the weight-gradient
    one and the bias gradient (column sums) into the same launch.  Every layer goes through the
    gnf_linear_* entry points: small batches run on weight-streaming kernels that evaluate a
    degree-structured mask (`degs[i] = (deg_out, deg_in, strict)`) instead of reading it."""

    @staticmethod
    def _spec(ctx, li):
        mk = ctx.masks[li] if ctx.masks is not None else None
        dg = ctx.degs[li] if ctx.degs is not None else None
        if dg is None:
            return ptr(mk), None, None, 0
        return ptr(mk), ptr(dg[0]), ptr(dg[1]), int(dg[2])

    @staticmethod
    def forward(ctx, x, masks, relu_in, degs, *params):
        """relu_in: x is itself the output of a ReLU (e.g. fc1 of the sparse embedding front): its gradient leaves this
        Function already gated by x > 0, fused into the data-gradient kernel's epilogue."""
        x = x.contiguous()
        n = len(params) // 2
        ctx.masks, ctx.degs, ctx.n, ctx.relu_in = masks, degs, n, bool(relu_in)
        acts = [x]
        a = x
        for li in range(n):
            W, b = params[2 * li].contiguous(), params[2 * li + 1]
            out_f, in_f = W.shape
            M = a.shape[0]
            y = _empty((M, out_f), x)
            nws = abi.load().gnf_linear_ws_bytes(M, out_f, in_f)
            ws = _ws(nws, x) if nws > 0 else None
            mk, do, di, st = MLPFn._spec(ctx, li)
            call("gnf_linear_fwd", ptr(a), ptr(W), ptr(b), mk, do, di, st, 1 if li < n - 1 else 0, ptr(y), M, out_f, in_f,
                 ptr(ws), nws, stream())
            a = y
            if li < n - 1:
                acts.append(y)
        ctx.save_for_backward(*acts, *params)
        return a

    @staticmethod
    def backward(ctx, gy):
        n = ctx.n
        saved = ctx.saved_tensors
        acts, params = saved[:n], saved[n:]
        g = gy.contiguous()
        grads = [None] * (2 * n)
        gx = None
        gb_ready = None                     # bias gradient of layer li, already produced by layer li + 1's launch
        for li in range(n - 1, -1, -1):
            W = params[2 * li].contiguous()
            out_f, in_f = W.shape
            a = acts[li]
            M = a.shape[0]
            nws = abi.load().gnf_linear_ws_bytes(M, out_f, in_f)
            ws = _ws(nws, W) if nws > 0 else None
            mk, do, di, st = MLPFn._spec(ctx, li)
            want_w, want_b = ctx.needs_input_grad[4 + 2 * li], ctx.needs_input_grad[5 + 2 * li]
            want_x = li > 0 or ctx.needs_input_grad[0]
            gW = grad_out(W) if want_w else None
            gb = gb_ready
            if gb is None and want_w and want_b:
                gb = grad_out(params[2 * li + 1])
            ga = _empty((M, in_f), W) if want_x else None
            gate = a if (li > 0 or ctx.relu_in) else None
            gb_next = None
            if want_w and want_x:
                # the column sums of this layer's data gradient ARE the bias gradient of the layer below
                if (li > 0 and ctx.needs_input_grad[5 + 2 * (li - 1)] and ctx.needs_input_grad[4 + 2 * (li - 1)]
                        and abi.load().gnf_linear_gxsum_fused(M, out_f, in_f, int(mk is not None or do is not None))):
                    gb_next = grad_out(params[2 * li - 1])
                call("gnf_linear_bwd", ptr(g), ptr(W), ptr(a), mk, do, di, st, ptr(gate), ptr(ga), ptr(gW),
                     None if gb_ready is not None else ptr(gb), ptr(gb_next), M, out_f, in_f, ptr(ws), nws, stream())
            elif want_w:
                call("gnf_linear_bwd_w", ptr(g), ptr(a), mk, do, di, st, ptr(gW), None if gb_ready is not None else ptr(gb), M,
                     out_f, in_f, ptr(ws), nws, stream())
            elif want_x:
                call("gnf_linear_bwd_x", ptr(g), ptr(W), mk, do, di, st, ptr(gate), ptr(ga), M, out_f, in_f, ptr(ws), nws,
                     stream())
            grads[2 * li], grads[2 * li + 1] = gW, gb
            if want_b and not want_w:
                grads[2 * li + 1] = colsum(g)
            gb_ready = gb_next
            if want_x:
                g = ga
                if li == 0:
                    gx = ga
        return (gx, None, None, None, *grads)


def mlp(x, layers, masks=None, relu_in=False, degs=None):
    """layers: list of (weight, bias) parameter pairs; masks: per-layer [out, in] 0/1 tensors (or None); degs: per-layer
    (deg_out [out], deg_in [in], strict) with mask[o][i] = deg_in[i] <= deg_out[o] (strict: <) where the caller has
    verified that the mask tensor has that structure, else None."""
    flat = [p for Wb in layers for p in Wb]
    return MLPFn.apply(x, masks, relu_in, degs, *flat)


# ----------------------------------------------------------------------------- MNISTCNN conv front
A1_SAVE_CAP_DEFAULT = 8 << 30      # bytes; policy, not a measurement: B <= 219 at d = 784 (46 720 B per image)


def _a1_buffer(n, like, will_backward, exact_ties):
    """Buffer for the conv1 activations of n images that the Winograd forward keeps for the backward (which then loads
    them instead of recomputing conv1 on the ALU that bounds it), or None: no backward will come, exact_ties (the direct
    forward keeps nothing), GNF_CONV_SAVE_A1=0 (the A/B switch), or more bytes than the cap GNF_CONV_SAVE_A1_MAX_BYTES
    (default 8 GiB).  None selects the recompute entry points.  The buffer lives and dies with the autograd node.
    will_backward must come from OUTSIDE the Function: inside `forward` grad mode is always off and
    `ctx.needs_input_grad` follows `requires_grad` of the inputs alone, also under `no_grad`."""
    if not will_backward or exact_ties or n <= 0 or os.environ.get("GNF_CONV_SAVE_A1", "1") == "0":
        return None
    nbytes = int(abi.load().gnf_mnistcnn_conv_a1_bytes(n))
    if nbytes > int(os.environ.get("GNF_CONV_SAVE_A1_MAX_BYTES", A1_SAVE_CAP_DEFAULT)):
        return None
    return torch.empty(nbytes // 4, dtype=torch.float32, device=like.device)


def _conv_fwd(e, W1c, b1c, W2c, b2c, pooled, arg, a1, n, exact_ties):
    if a1 is None:
        call("gnf_mnistcnn_conv_fwd", ptr(e), ptr(W1c), ptr(b1c), ptr(W2c), ptr(b2c), ptr(pooled), abi.rawptr(arg), n,
             int(bool(exact_ties)), stream())
    else:
        call("gnf_mnistcnn_conv_fwd_save", ptr(e), ptr(W1c), ptr(b1c), ptr(W2c), ptr(b2c), ptr(pooled), abi.rawptr(arg),
             ptr(a1), n, int(bool(exact_ties)), stream(), profile_as="gnf_mnistcnn_conv_fwd")


class MnistConvFn(torch.autograd.Function):
    """flatten(max_pool2d(conv2(relu(conv1(e))), 2)) for 28x28 single-channel images
    (models/MLP.py:36-43), fused in LDS; the backward loads the conv1 activations the forward kept (_a1_buffer) or
    recomputes conv1 in-kernel."""

    @staticmethod
    def forward(ctx, e, W1, b1, W2, b2, exact_ties=False, grad_mode=None):
        """exact_ties: direct-convolution forward whose pool argmax follows torch's first-maximum rule on exactly tied
        windows (include/gnf_hip.h); the Winograd forward otherwise.  grad_mode: torch.is_grad_enabled() at the call
        (mnist_conv hands it in); a bare .apply without it keeps nothing and recomputes"""
        e = e.contiguous()
        n = e.shape[0]
        W1c, b1c, W2c, b2c = W1.contiguous(), b1.contiguous(), W2.contiguous(), b2.contiguous()
        pooled = _empty((n, 2304), e)
        arg = torch.empty((n, 2304), dtype=torch.uint8, device=e.device)
        a1 = _a1_buffer(n, e, bool(grad_mode) and any(ctx.needs_input_grad), exact_ties)
        _conv_fwd(e, W1c, b1c, W2c, b2c, pooled, arg, a1, n, exact_ties)
        ctx.save_for_backward(e, W1c, b1c, W2c, b2c, arg)
        ctx.a1 = a1                        # an intermediate, not an output: freed with the node
        return pooled

    @staticmethod
    def backward(ctx, gp):
        e, W1, b1, W2, b2, arg = ctx.saved_tensors
        n = e.shape[0]
        gp = gp.contiguous()
        ge = _empty((n, 784), e)
        gW1, gb1, gW2, gb2 = grad_out(W1), grad_out(b1), grad_out(W2), grad_out(b2)
        nws = abi.load().gnf_mnistcnn_conv_bwd_ws_bytes(n)
        ws = _ws(nws, e)
        if ctx.a1 is None:
            call("gnf_mnistcnn_conv_bwd", ptr(e), ptr(W1), ptr(b1), ptr(W2), ptr(gp), abi.rawptr(arg), ptr(ge), ptr(gW1),
                 ptr(gb1), ptr(gW2), ptr(gb2), abi.rawptr(ws), nws, n, stream())
        else:
            call("gnf_mnistcnn_conv_bwd_a1", ptr(e), ptr(ctx.a1), ptr(W1), ptr(b1), ptr(W2), ptr(gp), abi.rawptr(arg),
                 ptr(ge), ptr(gW1), ptr(gb1), ptr(gW2), ptr(gb2), abi.rawptr(ws), nws, n, stream(),
                 profile_as="gnf_mnistcnn_conv_bwd")
        return ge, gW1, gb1, gW2, gb2, None, None


def mnist_conv(e, W1, b1, W2, b2, exact_ties=False):
    return MnistConvFn.apply(e, W1, b1, W2, b2, exact_ties, torch.is_grad_enabled())


# ----------------------------------------------------------------------------- CIFAR10CNN conv front
def lenet_conv_supported(size_img, k):
    """the geometries gnf_lenet_conv_* is instantiated for (the four of buildCIFAR10NormalizingFlow)"""
    c, h, w = size_img
    return bool(abi.load().gnf_lenet_conv_supported(int(c), int(h), int(w), int(k)))


def _keep_argmax(ctx, grad_mode):
    """does the forward of a LeNet front keep the second pool's decisions?  Only when a backward will come (grad mode on,
    an input that needs a gradient), and not with GNF_LENET_SAVE_ARGMAX=0 (the backward then recomputes conv2)"""
    return bool(grad_mode) and any(ctx.needs_input_grad) and os.environ.get("GNF_LENET_SAVE_ARGMAX", "1") != "0"


def _contiguous(*tensors):
    return tuple(t.contiguous() for t in tensors)


class LenetConvFn(torch.autograd.Function):
    """flatten(pool2(relu(conv_k(6->16)(pool2(relu(conv_k(C->6)(e))))))) on rows e [n, C*H*W] (reference models/MLP.py:66-68),
    fused in LDS (csrc/gnf_lenetcnn.hip).  The forward keeps the second pool's decisions (one byte per feature) when a
    backward will come; the backward recomputes conv1 and, without that plane, conv2 as well."""

    @staticmethod
    def forward(ctx, e, W1, b1, W2, b2, size_img, k, grad_mode=None):
        c, h, w = (int(v) for v in size_img)
        k = int(k)
        if e.stride(-1) != 1 or e.stride(0) < c * h * w:
            e = e.contiguous()
        n = e.shape[0]
        W1c, b1c, W2c, b2c = _contiguous(W1, b1, W2, b2)
        F = int(abi.load().gnf_lenet_conv_feat(c, h, w, k))
        feat = _empty((n, F), e)
        keep = _keep_argmax(ctx, grad_mode)
        arg = torch.empty((n, F), dtype=torch.uint8, device=e.device) if keep else None
        call("gnf_lenet_conv_fwd", ptr(e), e.stride(0), c, h, w, k, ptr(W1c), ptr(b1c), ptr(W2c), ptr(b2c), ptr(feat),
             abi.rawptr(arg) if keep else None, n, stream())
        ctx.save_for_backward(e, W1c, b1c, W2c, b2c)
        ctx.arg, ctx.geo = arg, (c, h, w, k)
        return feat

    @staticmethod
    def backward(ctx, gf):
        e, W1, b1, W2, b2 = ctx.saved_tensors
        c, h, w, k = ctx.geo
        n = e.shape[0]
        gf = gf.contiguous()
        ge = _empty((n, c * h * w), e) if ctx.needs_input_grad[0] else None
        outs = [grad_out_shared(p) for p in (W1, b1, W2, b2)]
        nws = abi.load().gnf_lenet_conv_bwd_ws_bytes(c, h, w, k, n)
        ws = _ws(nws, e)
        call("gnf_lenet_conv_bwd", ptr(e), e.stride(0), c, h, w, k, ptr(W1), ptr(b1), ptr(W2), ptr(b2),
             abi.rawptr(ctx.arg) if ctx.arg is not None else None, ptr(gf), ptr(ge), c * h * w,
             *(ptr(t) for t, _, _ in outs), abi.rawptr(ws), nws, n, stream())
        return (ge, *(finish(t) for t, finish, _ in outs), None, None, None)


def lenet_conv(e, W1, b1, W2, b2, size_img, k):
    return LenetConvFn.apply(e, W1, b1, W2, b2, size_img, k, torch.is_grad_enabled())


def lenet_rows(x, P, rows32, W1, b1, W2, b2, size_img, k, variable_major=False):
    """Features of the CIFAR10CNN front on the masked copies x[b] * P[rows32[r]] of a deterministic gate (rows32: int32
    device indices, None = all d rows in order): [B, R, F], or [R, B, F] when variable_major.  The copies are built in LDS
    (csrc/gnf_lenetcnn.hip, gnf_lenet_rows_fwd): the [B, R, d] tensor of the broadcast product never exists.  The bits of
    lenet_conv on that product.  Evaluation only: a plain function, no autograd node."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, P, W1, b1, W2, b2)):
        raise abi.GnfError("lenet_rows has no backward: call it under torch.no_grad() or on operands without requires_grad")
    return _rows_forward(x, P, rows32, W1, b1, W2, b2, size_img, k, variable_major, False,
                         profile_as="gnf_lenet_rows_fwd")[0]


def _rows_operands(x, P, rows32, size_img, k):
    """the operands of gnf_lenet_rows_* as the kernels want them: (x, P, rows32, R, (C, H, W, k), F)"""
    c, h, w = (int(v) for v in size_img)
    k = int(k)
    x = x.contiguous()
    d = x.shape[1]
    if d != c * h * w or tuple(P.shape) != (d, d):
        raise abi.GnfError("the row-subset front needs x [B, %d] and P [%d, %d]" % (c * h * w, d, d))
    if P.stride(1) != 1 or P.stride(0) < d:
        P = P.contiguous()
    if rows32 is None:
        R = d
    else:
        if rows32.dtype != torch.int32 or rows32.device != x.device:
            raise abi.GnfError("lenet_rows: rows32 must be an int32 tensor on the device of x")
        rows32 = rows32.contiguous()
        R = rows32.numel()
    F = int(abi.load().gnf_lenet_conv_feat(c, h, w, k))
    if F < 0:
        abi.check(F, "gnf_lenet_conv_feat")
    return x, P, rows32, R, (c, h, w, k), F


def _rows_forward(x, P, rows32, W1, b1, W2, b2, size_img, k, variable_major, keep, profile_as=None):
    """the gnf_lenet_rows_fwd_arg call of lenet_rows and LenetRowsFn: (feat, the second pool's decisions or None when not
    keep, the operands as the kernel took them, (R, geometry, variable_major))"""
    x, P, rows32, R, geo, F = _rows_operands(x, P, rows32, size_img, k)
    B, vm = x.shape[0], int(bool(variable_major))
    params = _contiguous(W1, b1, W2, b2)
    feat = _empty((R, B, F) if vm else (B, R, F), x)
    arg = torch.empty((B * R, F), dtype=torch.uint8, device=x.device) if keep else None
    call("gnf_lenet_rows_fwd_arg", ptr(x), ptr(P), P.stride(0), abi.rawptr(rows32) if rows32 is not None else None, R, *geo,
         *(ptr(t) for t in params), ptr(feat), abi.rawptr(arg) if keep else None, vm, B, stream(), profile_as=profile_as)
    return feat, arg, (x, P, rows32, *params), (R, geo, vm)


class LenetRowsFn(torch.autograd.Function):
    """lenet_rows with a backward, for training behind a FROZEN deterministic gate (csrc/gnf_lenetcnn.hip,
    gnf_lenet_rows_fwd_arg / gnf_lenet_rows_bwd): differentiable w.r.t. the four conv parameters and, when it asks for one,
    x; never w.r.t. P.  Saved for the backward: x, P, rows32, the parameters and one byte per feature (the second pool's
    decisions) -- never a [B, R, d] tensor, forward or backward.  No host synchronisation: safe under hipGraph capture."""

    @staticmethod
    def forward(ctx, x, P, rows32, W1, b1, W2, b2, size_img, k, variable_major, grad_mode=None):
        feat, ctx.arg, saved, ctx.cfg = _rows_forward(x, P, rows32, W1, b1, W2, b2, size_img, k, variable_major,
                                                      _keep_argmax(ctx, grad_mode))
        ctx.save_for_backward(*saved)
        return feat

    @staticmethod
    def backward(ctx, gf):
        x, P, rows32, W1, b1, W2, b2 = ctx.saved_tensors
        R, geo, vm = ctx.cfg
        B, d = x.shape
        gf = gf.contiguous()
        gx = _empty((B, d), x) if ctx.needs_input_grad[0] else None
        outs = [grad_out_shared(p) for p in (W1, b1, W2, b2)]
        nws = abi.load().gnf_lenet_rows_bwd_ws_bytes(*geo, R, B, int(gx is not None))
        ws = _ws(nws, x)
        call("gnf_lenet_rows_bwd", ptr(x), ptr(P), P.stride(0), abi.rawptr(rows32) if rows32 is not None else None, R, *geo,
             ptr(W1), ptr(b1), ptr(W2), ptr(b2), abi.rawptr(ctx.arg) if ctx.arg is not None else None, ptr(gf), vm,
             ptr(gx), *(ptr(t) for t, _, _ in outs), abi.rawptr(ws), nws, B, stream())
        return (gx, None, None, *(finish(t) for t, finish, _ in outs), None, None, None, None)


def lenet_rows_train(x, P, rows32, W1, b1, W2, b2, size_img, k, variable_major=False):
    """lenet_rows as an autograd node (LenetRowsFn): the features [B, R, F] ([R, B, F] when variable_major) of the copies
    x[b] * P[rows32[r]], with gradients for W1, b1, W2, b2 and for x when x.requires_grad.  P is a constant of the node: a P
    that requires grad (a trainable A) is refused, the caller takes the composed path for it."""
    if P.requires_grad:
        raise abi.GnfError("lenet_rows_train has no gradient for P: freeze A (post_process()) or take the composed path")
    return LenetRowsFn.apply(x, P, rows32, W1, b1, W2, b2, size_img, k, bool(variable_major), torch.is_grad_enabled())


def crop_origin(p):
    """cell origin of the 5x5 pooled block that can deviate from the background for a pixel row / column p"""
    return min(max((p - 6) >> 1, 0), 7)


def mnist_window_mask(device, kernel=2):
    """[784,784] bool: True where pixel j lies in the (2 kernel + 1)^2 window around pixel i (the support
    MNIST_A_prior(28, kernel) allows, diagonal included)"""
    r = torch.arange(28, device=device).repeat_interleave(28)
    c = torch.arange(28, device=device).repeat(28)
    return ((r[:, None] - r[None, :]).abs() <= kernel) & ((c[:, None] - c[None, :]).abs() <= kernel)


class SparseRows:
    """Masked copies to evaluate, in the order the sparse kernels want them: sorted by crop origin, with the
    (first output row, row count) table of the 64 origins for a batch of B samples."""

    def __init__(self, rows, B, device):
        rows = [int(r) for r in rows]
        origin = [8 * crop_origin(r // 28) + crop_origin(r % 28) for r in rows]
        order = sorted(range(len(rows)), key=lambda k: (origin[k], rows[k]))
        self.R, self.B = len(rows), B
        self.identity = order == list(range(len(rows)))         # the caller's rows already are in the kernels' order
        self.pix = torch.tensor([rows[k] for k in order], dtype=torch.int32, device=device)
        inv = [0] * len(rows)
        for pos, k in enumerate(order):
            inv[k] = pos
        self.unsort = torch.tensor(inv, dtype=torch.long, device=device)   # position of rows[k] in the sorted order
        self.order = torch.tensor(order, dtype=torch.long, device=device)  # caller's index of the copy at a sorted position
        counts = [0] * 64
        for g in origin:
            counts[g] += 1
        table, first = [], 0
        for g in range(64):
            table += [first * B, counts[g] * B]
            first += counts[g]
        self.groups = torch.tensor(table, dtype=torch.int32, device=device)
        self.max_group_rows = max(max(counts) * B, 1)
        # chunks of <= 512 output rows inside each origin's range (the backward's per-chunk fc1 weight gradients)
        chunks, per_origin = [], []
        for g in range(64):
            first, rows_g = table[2 * g], table[2 * g + 1]
            per_origin += [len(chunks) // 2, (rows_g + 511) // 512]
            for o in range(0, rows_g, 512):
                chunks += [first + o, min(512, rows_g - o)]
        self.n_kgroups = len(chunks) // 2
        self.kgroups = torch.tensor(chunks or [0, 0], dtype=torch.int32, device=device)
        self.origin_chunks = torch.tensor(per_origin, dtype=torch.int32, device=device)


SPARSE_REUSE_TABLES = True     # the sparse front's backward reads the tables its forward built (False: builds them again; tests)


class MnistSparseFn(torch.autograd.Function):
    """relu(fc1(flatten(maxpool(conv2(relu(conv1(x * P[i]))))))) for the masked copies i of a SparseRows, P zero outside
    the 5x5 pixel windows: [R*B, F] in the SparseRows' sorted order (row = position * B + sample).  Differentiable w.r.t.
    the six network parameters only (x and P are treated as constants: frozen deterministic gate)."""

    @staticmethod
    def forward(ctx, x, P, sr, pre_gated, W1, b1, W2, b2, Wfc1, bfc1, prep=None, grad_mode=True):
        """pre_gated: the consumer returns the cotangent of h1 already multiplied by [h1 > 0] (MLPFn's relu_in);
        prep: the parameter-only tables of mnistcnn_sparse_prepare (inference: they are not rebuilt per call)"""
        x, P = x.contiguous(), P.contiguous()
        ws_ = [t.contiguous() for t in (W1, b1, W2, b2, Wfc1, bfc1)]
        F = Wfc1.shape[0]
        n = sr.R * sr.B
        h1 = _empty((n, F), x)
        # (needs_input_grad reports the parameters' requires_grad even under torch.no_grad(), and inside forward() the
        # grad mode is always off: the caller's mode comes in as an argument -- without it every sampling / evaluation pass
        # saved the pooled blocks and the argmax bytes of a backward that never comes)
        train = bool(grad_mode) and any(ctx.needs_input_grad[4:10])
        if prep is not None and not train:
            nws = n * 400 * 4
            ws = _ws(nws, x)
            call("gnf_mnistcnn_sparse_fwd_prepared", ptr(x), sr.B, ptr(P), abi.rawptr(sr.pix), sr.R, abi.rawptr(sr.groups),
                 sr.max_group_rows, *[ptr(t) for t in ws_[:4]], F, abi.rawptr(prep), ptr(h1), abi.rawptr(ws), nws, stream())
            return h1
        ctx.pre_gated = bool(pre_gated)
        if not train:
            nws = abi.load().gnf_mnistcnn_sparse_ws_bytes(n, F)
            ws = _ws(nws, x)
            call("gnf_mnistcnn_sparse_fwd", ptr(x), sr.B, ptr(P), abi.rawptr(sr.pix), sr.R, abi.rawptr(sr.groups),
                 sr.max_group_rows, *[ptr(t) for t in ws_], F, ptr(h1), None, None, abi.rawptr(ws), nws, stream())
            return h1
        pd = _empty((n, 400), x)
        arg = torch.empty((n, 400), dtype=torch.uint8, device=x.device)
        # training: ONLY the parameter-only tables (fc1 column blocks per crop origin, background response: 13 MB) are this
        # call's own and stay alive for the backward, which reads them instead of building them again; the pooled blocks go
        # straight to pd (round 5 held a whole workspace whose first n * 400 floats nobody touched: 125 MB per in-flight
        # forward at B = 100)
        nt = abi.load().gnf_mnistcnn_sparse_prep_bytes(F)
        tables = torch.empty(max(int(nt) // 4, 1), dtype=torch.float32, device=x.device)
        call("gnf_mnistcnn_sparse_fwd_train", ptr(x), sr.B, ptr(P), abi.rawptr(sr.pix), sr.R, abi.rawptr(sr.groups),
             sr.max_group_rows, *[ptr(t) for t in ws_], F, ptr(h1), ptr(pd), abi.rawptr(arg), abi.rawptr(tables), nt, stream())
        ctx.save_for_backward(x, P, *ws_[:5], pd, arg, h1)
        ctx.sr = sr
        ctx.tables = tables if SPARSE_REUSE_TABLES else None
        return h1

    @staticmethod
    def backward(ctx, gh1):
        x, P, W1, b1, W2, b2, Wfc1, pd, arg, h1 = ctx.saved_tensors
        sr = ctx.sr
        F = Wfc1.shape[0]
        n = sr.R * sr.B
        g = gh1.contiguous() if ctx.pre_gated else (gh1 * (h1 > 0)).contiguous()
        gW1, gb1, gW2, gb2 = grad_out(W1), grad_out(b1), grad_out(W2), grad_out(b2)
        gWf, gbf = grad_out(Wfc1), _empty((F,), x)
        nws = abi.load().gnf_mnistcnn_sparse_bwd_ws_bytes(n, F, sr.n_kgroups)
        ws = _ws(nws, x)
        tables = getattr(ctx, "tables", None)
        call("gnf_mnistcnn_sparse_bwd_tables", ptr(x), sr.B, ptr(P), abi.rawptr(sr.pix), sr.R, abi.rawptr(sr.groups),
             sr.max_group_rows, abi.rawptr(sr.kgroups), sr.n_kgroups, abi.rawptr(sr.origin_chunks), ptr(W1), ptr(b1), ptr(W2),
             ptr(b2), ptr(Wfc1), F, abi.rawptr(tables) if tables is not None else None, ptr(pd), abi.rawptr(arg), ptr(g),
             ptr(gW1), ptr(gb1), ptr(gW2), ptr(gb2), ptr(gWf), ptr(gbf), abi.rawptr(ws), nws, stream())
        ctx.tables = None
        return None, None, None, None, gW1, gb1, gW2, gb2, gWf, gbf, None, None


def mnistcnn_sparse_fwd(x, P, sr, W1, b1, W2, b2, Wfc1, bfc1, pre_gated=False, prep=None):
    return MnistSparseFn.apply(x, P, sr, pre_gated, W1, b1, W2, b2, Wfc1, bfc1, prep, torch.is_grad_enabled())


def sparse_fc12_fits(Wfc1, Wfc2):
    """the widths the one-launch fc1 + ReLU + fc2 kernel is built for (the reference's MNISTCNN: 2304 -> 128 -> <= 32);
    GNF_SPARSE_FC12=0 keeps the grouped GEMM + tall-layer pair (A/B runs)"""
    import os
    return (Wfc1.shape[0] == 128 and Wfc2.shape[1] == 128 and 1 <= Wfc2.shape[0] <= 32
            and os.environ.get("GNF_SPARSE_FC12", "1") != "0")


def mnistcnn_sparse_fwd_fc2(x, P, sr, W1, b1, W2, b2, prep, Wfc2, bfc2):
    """fc2(relu(fc1(conv front))) of the masked copies of `sr` against prepared tables: [R*B, out_d], inference only
    (MLP.py:36-47 on the deterministic-gate copies, crop kernel + ONE launch for both linear layers)"""
    x, P = x.detach().contiguous(), P.detach().contiguous()
    ts = [t.detach().contiguous() for t in (W1, b1, W2, b2, Wfc2, bfc2)]
    n, out_d = sr.R * sr.B, Wfc2.shape[0]
    h2 = _empty((n, out_d), x)
    nws = max(n, 1) * 400 * 4
    ws = _ws(nws, x)
    call("gnf_mnistcnn_sparse_fwd_prepared_fc2", ptr(x), sr.B, ptr(P), abi.rawptr(sr.pix), sr.R, abi.rawptr(sr.groups),
         sr.max_group_rows, *[ptr(t) for t in ts[:4]], 128, abi.rawptr(prep), ptr(ts[4]), ptr(ts[5]), out_d, ptr(h2),
         abi.rawptr(ws), nws, stream())
    return h2


def mnistcnn_sparse_prepare(b1, W2, b2, Wfc1, bfc1):
    """the parameter-only tables of the sparse front (fc1 weight columns per crop origin, background responses), built
    once for a caller that evaluates the front many times with unchanged parameters (the levels of a sampling pass)"""
    ts = [t.detach().contiguous() for t in (b1, W2, b2, Wfc1, bfc1)]
    F = Wfc1.shape[0]
    nb = abi.load().gnf_mnistcnn_sparse_prep_bytes(F)
    prep = _ws(nb, Wfc1)
    call("gnf_mnistcnn_sparse_prepare", *[ptr(t) for t in ts], F, abi.rawptr(prep), nb, stream())
    return prep


class PermuteRowsFn(torch.autograd.Function):
    """y = x[perm] along dim 0 with a gather in both directions (inv = inverse permutation): autograd's own backward
    of an index is a sort + scatter-add"""

    @staticmethod
    def forward(ctx, x, perm, inv):
        ctx.save_for_backward(inv)
        return x.index_select(0, perm)

    @staticmethod
    def backward(ctx, g):
        inv, = ctx.saved_tensors
        return g.index_select(0, inv), None, None


# ----------------------------------------------------------------------------- DAG gate
IMP_RAW, IMP_SOFT, IMP_HARD_SOFT, IMP_HARD_SQ = 0, 1, 2, 3
GATE_DET, GATE_GUMBEL, GATE_NOISE = 0, 1, 2


class DagGateFn(torch.autograd.Function):
    """e[b*d+i, :] = x[b, :] * gate(importance(A[i, :])) (+ one-hot(i))
    (models/Conditionners/DAGConditioner.py:94-166)."""

    @staticmethod
    def forward(ctx, x, A, imp_mode, gate_mode, h_thresh, temperature, hot, u1, u2, seed, offset):
        x = x.contiguous()
        A = A.contiguous()
        B, d = x.shape
        ld = 2 * d if hot else d
        e = _empty((B * d, ld), x)
        u1 = u1.contiguous() if u1 is not None else None
        u2 = u2.contiguous() if u2 is not None else None
        nws = abi.load().gnf_dag_gate_fwd_ws_bytes(d)
        keep = A.requires_grad or x.requires_grad          # a backward will follow: its own buffer keeps the (i, j) table
        ws = torch.empty(max(int(nws) // 4, 1), dtype=torch.float32, device=x.device) if keep else _ws(nws, x)
        call("gnf_dag_gate_fwd", ptr(x), ptr(A), ptr(e), ld, imp_mode, gate_mode, float(h_thresh), float(temperature),
             ptr(u1), ptr(u2), seed, offset, int(hot), ptr(ws), B, d, stream())
        ctx.tab = ws if (keep and B > 0) else None
        ctx.save_for_backward(x, A, u1, u2)
        ctx.cfg = (imp_mode, gate_mode, float(h_thresh), float(temperature), ld, seed, offset)
        return e

    @staticmethod
    def backward(ctx, ge):
        x, A, u1, u2 = ctx.saved_tensors
        imp_mode, gate_mode, h_thresh, temperature, ld, seed, offset = ctx.cfg
        B, d = x.shape
        ge = ge.contiguous()
        gA, finish, _ = grad_out_shared(A) if ctx.needs_input_grad[1] else (None, None, False)
        gx = _empty((B, d), x) if ctx.needs_input_grad[0] else None
        ws = _ws(abi.load().gnf_dag_gate_bwd_ws_bytes(B, d), x)
        call("gnf_dag_gate_bwd", ptr(x), ptr(A), ptr(ge), ld, imp_mode, gate_mode, h_thresh, temperature, ptr(u1),
             ptr(u2), seed, offset, ptr(ctx.tab), ptr(gA), ptr(gx), ptr(ws), B, d, stream())
        return gx, (finish(gA) if gA is not None else None), None, None, None, None, None, None, None, None, None


class DagConvFrontFn(torch.autograd.Function):
    """flatten(max_pool2d(conv2(relu(conv1(e))), 2)) of the masked copies e[b*d+i, :] = x[b, :] * gate(importance(A[i, :]))
    -- DagGateFn and MnistConvFn as ONE autograd node (DAGConditioner.py:94-166,169 -> MLP.py:36-43), which is what lets the
    backward drop the structural zeros: dL/dA[i,j] = dP/dA[i,j] * (...) and dP/dA is exactly 0 wherever A is (97.2 % of
    MNIST_A_prior, DAGConditioner.py:118-119), so when x wants no gradient the conv backward writes the cotangent of e at
    the <= 32 columns per row the forward's plan lists (10 MB instead of 243 MB at B = 100, and it skips the W1^T dpre1
    products nobody reads) and the gate backward visits those (i, j) pairs only.  The plan is rebuilt from A on the device
    in every forward; a row with more columns than the plan holds sends both kernels down their dense code (decided on the
    device); x.requires_grad takes the dense entry points."""

    @staticmethod
    def forward(ctx, x, A, imp_mode, gate_mode, h_thresh, temperature, u1, u2, seed, offset, W1, b1, W2, b2, exact_ties,
                grad_mode):
        x, A = x.contiguous(), A.contiguous()
        B, d = x.shape
        if d != 784:
            raise abi.GnfError("the fused masked-image front is the 28 x 28 MNISTCNN one: d = %d" % d)
        n = B * d
        e = _empty((n, d), x)
        u1 = u1.contiguous() if u1 is not None else None
        u2 = u2.contiguous() if u2 is not None else None
        lib = abi.load()
        tab = torch.empty(max(int(lib.gnf_dag_gate_fwd_ws_bytes(d)) // 4, 1), dtype=torch.float32, device=x.device)
        want_plan = bool(grad_mode) and ctx.needs_input_grad[1] and not ctx.needs_input_grad[0] and B > 0
        plan, nplan = None, 0
        if want_plan:
            nplan = int(lib.gnf_dag_gate_plan_bytes(d))
            plan = torch.empty(nplan // 4, dtype=torch.int32, device=x.device)
        call("gnf_dag_gate_fwd_plan", ptr(x), ptr(A), ptr(e), d, imp_mode, gate_mode, float(h_thresh), float(temperature),
             ptr(u1), ptr(u2), seed, offset, 0, ptr(tab), abi.rawptr(plan) if plan is not None else None, nplan, B, d,
             stream())
        W1c, b1c, W2c, b2c = W1.contiguous(), b1.contiguous(), W2.contiguous(), b2.contiguous()
        pooled = _empty((n, 2304), x)
        arg = torch.empty((n, 2304), dtype=torch.uint8, device=x.device)
        a1 = _a1_buffer(n, x, bool(grad_mode) and any(ctx.needs_input_grad), exact_ties)
        _conv_fwd(e, W1c, b1c, W2c, b2c, pooled, arg, a1, n, exact_ties)
        ctx.save_for_backward(x, A, u1, u2, e, W1c, b1c, W2c, b2c, arg)
        ctx.tab, ctx.plan, ctx.a1 = (tab if B > 0 else None), plan, a1
        ctx.cfg = (imp_mode, gate_mode, float(h_thresh), float(temperature), seed, offset)
        return pooled

    @staticmethod
    def backward(ctx, gp):
        x, A, u1, u2, e, W1, b1, W2, b2, arg = ctx.saved_tensors
        imp_mode, gate_mode, h_thresh, temperature, seed, offset = ctx.cfg
        B, d = x.shape
        n = B * d
        lib = abi.load()
        gp = gp.contiguous()
        ge = _empty((n, d), x)                 # (with a plan: touched only if one of its rows overflows)
        gW1, gb1, gW2, gb2 = grad_out(W1), grad_out(b1), grad_out(W2), grad_out(b2)
        nws = lib.gnf_mnistcnn_conv_bwd_ws_bytes(n)
        ws = _ws(nws, x)
        plan = ctx.plan
        gec = _empty((n, abi.DAG_PLAN_KC), x) if plan is not None else None
        if ctx.a1 is None:
            call("gnf_mnistcnn_conv_bwd_cols", ptr(e), ptr(W1), ptr(b1), ptr(W2), ptr(gp), abi.rawptr(arg), ptr(ge),
                 abi.rawptr(plan) if plan is not None else None, d, ptr(gec), ptr(gW1), ptr(gb1), ptr(gW2), ptr(gb2),
                 abi.rawptr(ws), nws, n, stream())
        else:
            call("gnf_mnistcnn_conv_bwd_cols_a1", ptr(e), ptr(ctx.a1), ptr(W1), ptr(b1), ptr(W2), ptr(gp),
                 abi.rawptr(arg), ptr(ge), abi.rawptr(plan) if plan is not None else None, d, ptr(gec), ptr(gW1),
                 ptr(gb1), ptr(gW2), ptr(gb2), abi.rawptr(ws), nws, n, stream(),
                 profile_as="gnf_mnistcnn_conv_bwd_cols")
        gA, finish, acc = (grad_out_shared(A, accumulate_ok=plan is not None) if ctx.needs_input_grad[1]
                           else (None, None, False))
        gx = _empty((B, d), x) if ctx.needs_input_grad[0] else None
        if plan is not None:
            ws2 = _ws(lib.gnf_dag_gate_bwd_cols_ws_bytes(B, d), x)
            call("gnf_dag_gate_bwd_cols", ptr(x), ptr(ge), ptr(gec), abi.rawptr(plan), imp_mode, gate_mode, temperature,
                 ptr(u1), ptr(u2), seed, offset, ptr(ctx.tab), ptr(gA), int(acc), ptr(ws2), B, d, stream())
        elif gA is not None or gx is not None:
            ws2 = _ws(lib.gnf_dag_gate_bwd_ws_bytes(B, d), x)
            call("gnf_dag_gate_bwd", ptr(x), ptr(A), ptr(ge), d, imp_mode, gate_mode, h_thresh, temperature, ptr(u1),
                 ptr(u2), seed, offset, ptr(ctx.tab), ptr(gA), ptr(gx), ptr(ws2), B, d, stream())
        return (gx, (finish(gA) if gA is not None else None), None, None, None, None, None, None, None, None,
                gW1, gb1, gW2, gb2, None, None)


def dag_conv_front(x, A, imp_mode, gate_mode, h_thresh, temperature, u1, u2, seed, offset, W1, b1, W2, b2,
                   exact_ties=False):
    return DagConvFrontFn.apply(x, A, imp_mode, gate_mode, h_thresh, temperature, u1, u2, seed, offset, W1, b1, W2, b2,
                                exact_ties, torch.is_grad_enabled())


class DagLenetFrontFn(torch.autograd.Function):
    """LenetConvFn on the masked copies e[b*d+i, :] = x[b, :] * gate(importance(A[i, :])) as ONE autograd node whose kernels
    build each copy in LDS (csrc/gnf_lenetcnn.hip, gnf_lenet_gated_*): no [B*d, d] tensor is allocated, forward or
    backward -- at d = 3072 e and its cotangent are 37.7 MB per sample each.  The features are bit-identical to
    DagGateFn + LenetConvFn with the same (seed, offset).  Differentiable w.r.t. A and the conv parameters, not x
    (dag_lenet_front composes the two nodes for that)."""

    @staticmethod
    def forward(ctx, x, A, imp_mode, gate_mode, h_thresh, temperature, u1, u2, seed, offset, W1, b1, W2, b2, size_img, k,
                grad_mode):
        c, h, w = (int(v) for v in size_img)
        k = int(k)
        x, A = x.contiguous(), A.contiguous()
        B, d = x.shape
        if d != c * h * w or tuple(A.shape) != (d, d):
            raise abi.GnfError("the fused masked-image front needs x [B, %d] and A [%d, %d]" % (c * h * w, d, d))
        u1 = u1.contiguous() if u1 is not None else None
        u2 = u2.contiguous() if u2 is not None else None
        lib = abi.load()
        W1c, b1c, W2c, b2c = _contiguous(W1, b1, W2, b2)
        F = int(lib.gnf_lenet_conv_feat(c, h, w, k))
        if F < 0:
            abi.check(F, "gnf_lenet_conv_feat")
        tab = torch.empty(max(int(lib.gnf_dag_gate_fwd_ws_bytes(d)) // 4, 1), dtype=torch.float32, device=x.device)
        feat = _empty((B * d, F), x)
        keep = _keep_argmax(ctx, grad_mode)
        arg = torch.empty((B * d, F), dtype=torch.uint8, device=x.device) if keep else None
        call("gnf_lenet_gated_fwd", ptr(x), ptr(A), ptr(tab), c, h, w, k, imp_mode, gate_mode, float(h_thresh),
             float(temperature), ptr(u1), ptr(u2), seed, offset, ptr(W1c), ptr(b1c), ptr(W2c), ptr(b2c), ptr(feat),
             abi.rawptr(arg) if keep else None, B, stream())
        ctx.save_for_backward(x, A, u1, u2, tab, W1c, b1c, W2c, b2c)
        ctx.arg, ctx.geo = arg, (c, h, w, k)
        ctx.cfg = (imp_mode, gate_mode, float(temperature), seed, offset)
        return feat

    @staticmethod
    def backward(ctx, gf):
        x, A, u1, u2, tab, W1, b1, W2, b2 = ctx.saved_tensors
        c, h, w, k = ctx.geo
        imp_mode, gate_mode, temperature, seed, offset = ctx.cfg
        B = x.shape[0]
        gf = gf.contiguous()
        gA, finish_A, acc = grad_out_shared(A, accumulate_ok=True) if ctx.needs_input_grad[1] else (None, None, False)
        outs = [grad_out_shared(p) for p in (W1, b1, W2, b2)]
        nws = abi.load().gnf_lenet_gated_bwd_ws_bytes(c, h, w, k, B)
        ws = _ws(nws, x)
        call("gnf_lenet_gated_bwd", ptr(x), ptr(tab), c, h, w, k, imp_mode, gate_mode, temperature, ptr(u1), ptr(u2), seed,
             offset, ptr(W1), ptr(b1), ptr(W2), ptr(b2), abi.rawptr(ctx.arg) if ctx.arg is not None else None, ptr(gf),
             ptr(gA), int(acc), *(ptr(t) for t, _, _ in outs), abi.rawptr(ws), nws, B, stream())
        return (None, (finish_A(gA) if gA is not None else None), None, None, None, None, None, None, None, None,
                *(finish(t) for t, finish, _ in outs), None, None, None)


def dag_lenet_front(x, A, imp_mode, gate_mode, h_thresh, temperature, u1, u2, seed, offset, W1, b1, W2, b2, size_img, k):
    """features [B*d, F] of the CIFAR10CNN front on the masked copies of x.  A gradient for x needs a sum over the rows i
    across workgroups, and stacked steps are rare in the CIFAR factory: that case runs the two existing nodes."""
    if torch.is_grad_enabled() and x.requires_grad:
        e = DagGateFn.apply(x, A, imp_mode, gate_mode, h_thresh, temperature, False, u1, u2, seed, offset)
        return lenet_conv(e, W1, b1, W2, b2, size_img, k)
    return DagLenetFrontFn.apply(x, A, imp_mode, gate_mode, h_thresh, temperature, u1, u2, seed, offset, W1, b1, W2, b2,
                                 size_img, k, torch.is_grad_enabled())


# ----------------------------------------------------------------------------- DAGMLP first layer behind the gate
def dagmlp_supported(d, H):
    """the shapes gnf_dagmlp_* takes (1 <= d <= 64, H >= 1)"""
    return bool(abi.load().gnf_dagmlp_supported(int(d), int(H)))


def _first_layer(W1, b1, d, hot):
    """W1, b1 of the first Linear as the kernels want them: rows of unit stride, (2 d | d) columns"""
    if W1.dim() != 2 or W1.shape[1] != (2 * d if hot else d) or tuple(b1.shape) != (W1.shape[0],):
        raise abi.GnfError("the fused DAGMLP front needs W1 [H, %d] and b1 [H]" % (2 * d if hot else d))
    return W1.contiguous(), b1.contiguous()


class DagMlpFrontFn(torch.autograd.Function):
    """act(Linear_1(e)) on the masked copies e[b*d+i, :] = (x[b, :] * gate(importance(A[i, :])) | one-hot(i)) as ONE autograd
    node whose kernels build each copy in LDS (csrc/gnf_dagmlp.hip, gnf_dagmlp_gated_*): DagGateFn and the first layer of
    MLPFn without e [B*d, 2d] or its cotangent in memory; the one-hot half of the layer is column d+i of W1.  act = ReLU
    (relu) -- the consumer (MLPFn with relu_in) then returns the cotangent already multiplied by [a1 > 0] -- or the identity.
    Saved: x, A, (u1, u2), W1, b1 and the gate table; the noise is regenerated.  Differentiable w.r.t. x, A, W1, b1."""

    @staticmethod
    def forward(ctx, x, A, imp_mode, gate_mode, h_thresh, temperature, u1, u2, seed, offset, W1, b1, hot, relu):
        x, A = x.contiguous(), A.contiguous()
        B, d = x.shape
        if tuple(A.shape) != (d, d):
            raise abi.GnfError("the fused DAGMLP front needs x [B, %d] and A [%d, %d]" % (d, d, d))
        W1c, b1c = _first_layer(W1, b1, d, hot)
        H = W1c.shape[0]
        u1 = u1.contiguous() if u1 is not None else None
        u2 = u2.contiguous() if u2 is not None else None
        tab = torch.empty(max(int(abi.load().gnf_dag_gate_fwd_ws_bytes(d)) // 4, 1), dtype=torch.float32, device=x.device)
        a1 = _empty((B * d, H), x)
        call("gnf_dagmlp_gated_fwd", ptr(x), ptr(A), ptr(tab), imp_mode, gate_mode, float(h_thresh), float(temperature),
             ptr(u1), ptr(u2), seed, offset, ptr(W1c), W1c.stride(0), ptr(b1c), int(bool(hot)), int(bool(relu)), ptr(a1), B,
             d, H, stream())
        ctx.save_for_backward(x, A, u1, u2, tab, W1c, b1c)
        ctx.cfg = (imp_mode, gate_mode, float(temperature), seed, offset, bool(hot))
        return a1

    @staticmethod
    def backward(ctx, g):
        x, A, u1, u2, tab, W1, b1 = ctx.saved_tensors
        imp_mode, gate_mode, temperature, seed, offset, hot = ctx.cfg
        B, d = x.shape
        H = W1.shape[0]
        g = g.contiguous()
        gx = _empty((B, d), x) if ctx.needs_input_grad[0] else None
        gA, finish_A, acc = grad_out_shared(A, accumulate_ok=True) if ctx.needs_input_grad[1] else (None, None, False)
        gW1 = grad_out(W1) if ctx.needs_input_grad[10] else None
        gb1 = grad_out(b1) if ctx.needs_input_grad[11] else None
        nws = abi.load().gnf_dagmlp_gated_bwd_ws_bytes(B, d, H)
        ws = _ws(nws, x)
        call("gnf_dagmlp_gated_bwd", ptr(x), ptr(tab), imp_mode, gate_mode, temperature, ptr(u1), ptr(u2), seed, offset,
             ptr(W1), W1.stride(0), int(hot), ptr(g), ptr(gx), ptr(gA), int(acc), ptr(gW1),
             gW1.stride(0) if gW1 is not None else 0, ptr(gb1), abi.rawptr(ws), nws, B, d, H, stream())
        return (gx, (finish_A(gA) if gA is not None else None), None, None, None, None, None, None, None, None, gW1, gb1,
                None, None)


def dag_mlp_front(x, A, imp_mode, gate_mode, h_thresh, temperature, u1, u2, seed, offset, W1, b1, hot, relu):
    """a1 [B*d, H] = act(first DAGMLP layer) of the masked copies of x (DagMlpFrontFn); feed the rest of the chain with
    mlp(a1, layers[1:], relu_in=True)"""
    return DagMlpFrontFn.apply(x, A, imp_mode, gate_mode, h_thresh, temperature, u1, u2, seed, offset, W1, b1, bool(hot),
                               bool(relu))


def dag_mlp_rows(x, P, rows32, W1, b1, hot, relu, variable_major=False):
    """act(first DAGMLP layer) on the copies (x[b] * P[rows32[r]] | one-hot(rows32[r])) of a deterministic gate (rows32: int32
    device indices, None = all d rows in order): [B*R, H] in the row order b*R + r, or r*B + b when variable_major.  The
    copies are built in LDS (gnf_dagmlp_rows_fwd).  Evaluation only: a plain function, no autograd node."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, P, W1, b1)):
        raise abi.GnfError("dag_mlp_rows has no backward: call it under torch.no_grad() or on operands without requires_grad")
    x = x.contiguous()
    B, d = x.shape
    if tuple(P.shape) != (d, d):
        raise abi.GnfError("dag_mlp_rows needs x [B, %d] and P [%d, %d]" % (d, d, d))
    if P.stride(1) != 1 or P.stride(0) < d:
        P = P.contiguous()
    if rows32 is None:
        R = d
    else:
        if rows32.dtype != torch.int32 or rows32.device != x.device:
            raise abi.GnfError("dag_mlp_rows: rows32 must be an int32 tensor on the device of x")
        rows32 = rows32.contiguous()
        R = rows32.numel()
    W1c, b1c = _first_layer(W1.detach(), b1.detach(), d, hot)
    H = W1c.shape[0]
    a1 = _empty((B * R, H), x)
    call("gnf_dagmlp_rows_fwd", ptr(x), ptr(P), P.stride(0), abi.rawptr(rows32) if rows32 is not None and R else None, R,
         ptr(W1c), W1c.stride(0), ptr(b1c), int(bool(hot)), int(bool(relu)), ptr(a1), int(bool(variable_major)), B, d, H,
         stream())
    return a1


# ----------------------------------------------------------------------------- DAGMLP first layer with a context
def _group_rows(t, other, G, what):
    if t.dim() == 2 and G >= 1 and t.shape[0] % G != 0:
        abi.check(-2, what)                                          # GNF_ESHAPE, as the entry point itself answers
    if t.dim() != 2 or other.dim() != 2 or other.shape[1] != t.shape[1] or G < 1 or other.shape[0] * G != t.shape[0]:
        raise abi.GnfError("%s needs [M, H] rows and a [M / G, H] group array: got %s, %s, G = %d"
                           % (what, tuple(t.shape), tuple(other.shape), G))


def group_bias_fwd(y, cb, G, relu, out=None):
    """out[r, :] = act(y[r, :] + cb[r // G, :]) (gnf_group_bias_fwd; act = ReLU or the identity).  y: [M, H], cb: [M / G, H],
    both contiguous; out: None (a new tensor), y itself (in place) or another contiguous [M, H].  No autograd."""
    G = int(G)
    _group_rows(y, cb, G, "gnf_group_bias_fwd")
    if not (y.is_contiguous() and cb.is_contiguous()):
        raise abi.GnfError("gnf_group_bias_fwd needs contiguous operands")
    if out is None:
        out = torch.empty_like(y)
    elif out.shape != y.shape or not out.is_contiguous():
        raise abi.GnfError("gnf_group_bias_fwd: out must be a contiguous tensor of y's shape")
    M, H = y.shape
    call("gnf_group_bias_fwd", ptr(y), ptr(cb), ptr(out), int(bool(relu)), M, H, G, stream())
    return out


def group_bias_bwd(g, a, G, g_pre=None, g_cb=None):
    """(g_pre, g_cb) of gnf_group_bias_bwd: g_pre = g * [a > 0] (a: the saved forward output; None for the identity, and g_pre
    is then g itself unless a tensor is given), g_cb[b] = the sum of the G rows of g_pre of sample b, in ascending order.
    g_pre: None (a new tensor), g (in place) or another contiguous [M, H]."""
    G = int(G)
    if g.dim() != 2 or G < 1 or not g.is_contiguous() or (a is not None and (a.shape != g.shape or not a.is_contiguous())):
        raise abi.GnfError("gnf_group_bias_bwd needs contiguous [M, H] operands and G >= 1")
    M, H = g.shape
    if M % G != 0:
        abi.check(-2, "gnf_group_bias_bwd")
    if g_pre is None and a is not None:
        g_pre = torch.empty_like(g)
    if g_pre is not None and (g_pre.shape != g.shape or not g_pre.is_contiguous()):
        raise abi.GnfError("gnf_group_bias_bwd: g_pre must be a contiguous tensor of g's shape")
    if g_cb is None:
        g_cb = _empty((M // G, H), g)
    elif tuple(g_cb.shape) != (M // G, H) or not g_cb.is_contiguous():
        raise abi.GnfError("gnf_group_bias_bwd: g_cb must be a contiguous [M / G, H] tensor")
    call("gnf_group_bias_bwd", ptr(g), ptr(a), ptr(g_pre), ptr(g_cb), M, H, G, stream())
    return (g if g_pre is None else g_pre), g_cb


class GroupBiasFn(torch.autograd.Function):
    """act(y + cb repeated over groups of G rows) (csrc/gnf_group_bias.hip): the context half of a DAGMLP's first layer
    enters the [B*d, H] pre-activation as one bias row per sample.  act = ReLU (relu) -- the consumer (MLPFn with relu_in)
    returns the cotangent already gated, and gating it again changes nothing -- or the identity.  The backward is ONE launch:
    the cotangent of y (g * [out > 0]) and its sum over each group, the cotangent of cb."""

    @staticmethod
    def forward(ctx, y, cb, G, relu):
        y, cb = y.contiguous(), cb.contiguous()
        out = group_bias_fwd(y, cb, G, relu)
        ctx.G, ctx.relu = int(G), bool(relu)
        if ctx.relu:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        a = ctx.saved_tensors[0] if ctx.relu else None
        g_pre, g_cb = group_bias_bwd(g.contiguous(), a, ctx.G)
        return (g_pre if ctx.needs_input_grad[0] else None), (g_cb if ctx.needs_input_grad[1] else None), None, None


def group_bias(y, cb, G, relu):
    """act(y[r] + cb[r // G]) for y [M, H] and cb [M / G, H] with gradients for both (GroupBiasFn)"""
    return GroupBiasFn.apply(y, cb, int(G), bool(relu))


# ----------------------------------------------------------------------------- Monotonic (UMNN) normalizer
_CC = {}


def cc_rule(nb_steps, device):
    """Clenshaw-Curtis weights / nodes, built on the host in fp64 with the construction of
    UMNN 1.0's compute_cc_weights (third-party, absent from the reference tree; restated
    from its published algorithm -- parity unpinned), cast to fp32."""
    key = (int(nb_steps), str(device))
    if key not in _CC:
        S = int(nb_steps)
        k = np.arange(0, S + 1, dtype=np.float64).reshape(-1, 1)
        lam = np.cos((k @ k.T) * math.pi / S)
        lam[:, 0] = .5
        lam[:, -1] = .5 * lam[:, -1]
        lam = lam * 2 / S
        W = k.copy()
        odd = np.arange(1, S + 1, 2)
        W[odd] = 0
        W = 2 / (1 - W ** 2)
        W[0] = 1
        W[odd] = 0
        w = (lam.T @ W).reshape(-1)
        t = np.cos(np.arange(0, S + 1) * math.pi / S)
        _CC[key] = (torch.tensor(w, dtype=torch.float32, device=device),
                    torch.tensor(t, dtype=torch.float32, device=device))
    return _CC[key]


def _mono_net(params):
    """params: [W0, b0, W1, b1, ...] contiguous fp32 HIP tensors -> gnf_mono_net."""
    nl = len(params) // 2
    if nl < 2 or nl > abi.MONO_MAX_LAYERS:
        raise abi.GnfError("integrand net needs 2..%d Linear layers" % abi.MONO_MAX_LAYERS)
    net = abi.MonoNet()
    net.nl = nl
    net.dims[0] = params[0].shape[1]
    for l in range(nl):
        W, b = params[2 * l], params[2 * l + 1]
        if W.shape[1] != net.dims[l]:
            raise abi.GnfError("integrand net layer %d: in_features mismatch" % l)
        net.dims[l + 1] = W.shape[0]
        net.W[l] = ptr(W).value
        net.b[l] = ptr(b).value
    return net


def _mono_pack(net, like):
    """the kernels' image of the integrand net's parameters (padded, transposed and fragment-major copies)"""
    nfl = abi.load().gnf_monotonic_pack_floats(ctypes.byref(net))
    if nfl < 0:
        abi.check(int(nfl), "gnf_monotonic_pack_floats")
    pack = _empty((int(nfl),), like)
    call("gnf_monotonic_pack", ctypes.byref(net), ptr(pack), stream())
    return pack


def monotonic_pack(params, like):
    """the weight image for `monotonic_inverse(..., pack=...)`: a caller that inverts many times with unchanged parameters
    (the 109 DAG levels of one MNIST sampling pass) packs once.  (Not cached behind the caller's back: the fused Adam
    launch and a replayed hipGraph rewrite the parameters without touching torch's version counters.)"""
    params = [p.detach().contiguous() for p in params]
    return _mono_pack(_mono_net(params), like)


class MonotonicFn(torch.autograd.Function):
    """z = int_0^x f(t;h) dt + h[...,0],  jac = f(x;h)
    (models/Normalizers/MonotonicNormalizer.py:51-66 + UMNN NeuralIntegral, incl. its
    Leibniz-rule x-gradient)."""

    @staticmethod
    def forward(ctx, x, h, nb_steps, *params):
        x = x.contiguous()
        params = [p.contiguous() for p in params]
        B, d = x.shape
        net = _mono_net(params)
        if h.shape[2] != net.dims[0] - 1:
            raise abi.GnfError("cond_size %d != integrand net input %d - 1" % (h.shape[2], net.dims[0]))
        pack = _mono_pack(net, x)
        w, t = cc_rule(nb_steps, x.device)
        z, jac = _empty((B, d), x), _empty((B, d), x)
        call("gnf_monotonic_fwd", ptr(pack), ctypes.byref(net), ptr(x), ptr(h), h.stride(0), h.stride(1), h.stride(2),
             ptr(w), ptr(t), int(nb_steps), ptr(z), ptr(jac), B, d, stream())
        ctx.save_for_backward(x, h, pack, *params)
        ctx.S = int(nb_steps)
        return z, jac

    @staticmethod
    def backward(ctx, gz, gjac):
        x, h, pack, *params = ctx.saved_tensors
        B, d = x.shape
        S = ctx.S
        net = _mono_net(params)
        if h.stride(0) != d * h.stride(1):
            h = h.contiguous()          # element stride must collapse for the d W1 GEMM
        w, t = cc_rule(S, x.device)
        gz = gz.contiguous() if gz is not None else torch.zeros_like(x)
        gjac = gjac.contiguous() if gjac is not None else None
        gx = _empty((B, d), x)
        gh = _empty(tuple(h.shape), x)
        gparams = [grad_out(p) for p in params]
        nl = net.nl
        gW = (ctypes.c_void_p * nl)(*[gparams[2 * l].data_ptr() for l in range(nl)])
        gb = (ctypes.c_void_p * nl)(*[gparams[2 * l + 1].data_ptr() for l in range(nl)])
        nbytes = abi.load().gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), S, B, d)
        if nbytes < 0:
            abi.check(int(nbytes), "gnf_monotonic_bwd_ws_bytes")
        ws = _ws(nbytes, x)
        call("gnf_monotonic_bwd", ptr(pack), ctypes.byref(net), ptr(x), ptr(h), h.stride(0), h.stride(1), h.stride(2),
             ptr(w), ptr(t), S, ptr(gz), ptr(gjac), ptr(gx), ptr(gh), gh.stride(0), gh.stride(1), gh.stride(2),
             gW, gb, ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4, B, d, stream())
        return (gx, gh, None, *gparams)


def monotonic_inverse(z, h, nb_steps, params, pack=None, out=None, out_cols=None):
    """20-step bisection on [-20, 20], the quadrature fused in the kernel
    (MonotonicNormalizer.py:69-83).  out / out_cols: write the TRANSPOSED result into columns out_cols of `out` (the
    level loop of NormalizingFlowStep.invert: z is [level rows, batch], the sample is [batch, d])."""
    z = z.contiguous()
    params = [p.detach().contiguous() for p in params]
    B, d = z.shape
    net = _mono_net(params)
    if pack is None:
        pack = _mono_pack(net, z)
    w, t = cc_rule(nb_steps, z.device)
    if out is not None:
        # element (b, j) of this [B, d] problem -> out[j, out_cols[b]]  (out [d, width] contiguous, out_cols int32 [B])
        assert out.is_contiguous() and out.dtype == torch.float32 and out.shape[0] == d and out_cols.dtype == torch.int32
        assert out_cols.numel() == B and out_cols.device == z.device
        call("gnf_monotonic_inv_scatter", ptr(pack), ctypes.byref(net), ptr(z), ptr(h), h.stride(0), h.stride(1),
             h.stride(2), ptr(w), ptr(t), int(nb_steps), ptr(out), abi.rawptr(out_cols), out.shape[1], B, d, stream())
        return out
    x = _empty((B, d), z)
    call("gnf_monotonic_inv", ptr(pack), ctypes.byref(net), ptr(z), ptr(h), h.stride(0), h.stride(1), h.stride(2),
         ptr(w), ptr(t), int(nb_steps), ptr(x), B, d, stream())
    return x


class ModuleIntegralFn(torch.autograd.Function):
    """z = int_0^x f(t; h) dt for a USER-SUPPLIED integrand module (MonotonicNormalizer(integrand_net=<nn.Module>),
    reference MonotonicNormalizer.py:44-48,51-63): the module is honoured as it is and evaluated through PyTorch-ROCm
    on the device, at all Clenshaw-Curtis nodes in one batch ("CCParallel" form; "CC" gives the same numbers up to
    summation order).  Only the reference's own IntegrandNet architecture is fused into the gfx950 kernel.

    Same conventions as the fused kernel / UMNN's NeuralIntegral (restated, parity unpinned): forward without a graph;
    backward re-evaluates the integrand at the nodes to get d/d(theta) and d/dh by the same quadrature weighted by
    grad * x / 2, and uses the Leibniz rule for the upper limit, dz/dx = f(x; h)."""

    @staticmethod
    def forward(ctx, x, hflat, module, nb_steps, *params):
        w, t = cc_rule(nb_steps, x.device)
        S1 = w.numel()
        B, d = x.shape
        with torch.no_grad():
            nodes = (x.unsqueeze(0) * ((t.view(S1, 1, 1) + 1.) * .5)).reshape(S1 * B, d)
            f = module(nodes, hflat.unsqueeze(0).expand(S1, B, -1).reshape(S1 * B, -1)).view(S1, B, d)
            z = (f * w.view(S1, 1, 1)).sum(0) * x * .5
        ctx.module, ctx.S = module, int(nb_steps)
        ctx.save_for_backward(x, hflat)
        return z

    @staticmethod
    def backward(ctx, gz):
        x, hflat = ctx.saved_tensors
        module = ctx.module
        w, t = cc_rule(ctx.S, x.device)
        S1 = w.numel()
        B, d = x.shape
        params = [p for p in module.parameters() if p.requires_grad]
        with torch.enable_grad():
            hr = hflat.detach().requires_grad_(True)
            nodes = (x.detach().unsqueeze(0) * ((t.view(S1, 1, 1) + 1.) * .5)).reshape(S1 * B, d)
            f = module(nodes, hr.unsqueeze(0).expand(S1, B, -1).reshape(S1 * B, -1)).view(S1, B, d)
            weight = (gz * x.detach() * .5).unsqueeze(0) * w.view(S1, 1, 1)
            grads = torch.autograd.grad((f * weight).sum(), [hr] + params, allow_unused=True)
            fx = module(x.detach(), hflat.detach())
        gx = gz * fx.detach() if ctx.needs_input_grad[0] else None
        return (gx, grads[0], None, None, *grads[1:])


def module_monotonic(x, h, module, nb_steps):
    """(z, jac) of MonotonicNormalizer.forward for a custom integrand module; h: [B, d, c]"""
    B, d = x.shape
    hflat = h.permute(0, 2, 1).contiguous().view(B, -1)          # cond-major, as the reference passes it (:55)
    params = [p for p in module.parameters() if p.requires_grad]
    z = ModuleIntegralFn.apply(x, hflat, module, int(nb_steps), *params) + h[:, :, 0]
    return z, module(x, hflat)


def module_monotonic_inverse(z, h, module, nb_steps):
    """the reference's bisection (MonotonicNormalizer.py:69-83): 20 halvings of [-20, 20], midpoint returned"""
    B, d = z.shape
    hflat = h.permute(0, 2, 1).contiguous().view(B, -1)
    lo = torch.full_like(z, -20.)
    hi = torch.full_like(z, 20.)
    h0 = h[:, :, 0]
    with torch.no_grad():
        for _ in range(20):
            mid = (lo + hi) * .5
            zm = ModuleIntegralFn.apply(mid, hflat, module, int(nb_steps)) + h0
            left = zm > z                                     # (:76-79) solution lies left of the midpoint
            hi = torch.where(left, mid, hi)
            lo = torch.where(left, lo, mid)
    return (lo + hi) * .5


# ----------------------------------------------------------------------------- image batch preparation
def image_prep(data_u8, rows, flip, u, seed, offset, alpha, size_img, want_bpp):
    """One launch of gnf_image_prep (csrc/gnf_image_prep.hip): rows of the uint8 data set [n, d] -> (x [B, d], bpp_term [B] or
    None), x = logit(alpha + (1 - 2 alpha) (pixel + u) / 256) and bpp_term = sum_j log2 y + log2 (1 - y).
    rows: int32 device indices [B] (any order, repeats allowed; clamped into the data set by the kernel), or None for every
    row of data_u8 in order.  flip: None / False (no flip), True (one Philox coin per output row), or a uint8 / bool mask [B].
    u: explicit uniforms [B, d] (parity tests) or None for Philox keyed by (seed, offset); the layout: include/gnf_hip.h.
    size_img = (C, H, W), d = C*H*W.  The inputs are data: no autograd node."""
    c, h, w = (int(v) for v in size_img)
    if data_u8.dtype != torch.uint8 or data_u8.dim() != 2 or data_u8.shape[1] != c * h * w:
        raise abi.GnfError("image_prep needs a uint8 tensor [n, %d]: got %s %s" % (c * h * w, data_u8.dtype, tuple(data_u8.shape)))
    if not data_u8.is_contiguous():
        data_u8 = data_u8.contiguous()
    n, d = data_u8.shape
    if rows is None:
        B = n
    else:
        if rows.dtype != torch.int32 or rows.device != data_u8.device:
            raise abi.GnfError("image_prep: rows must be an int32 tensor on the device of the data")
        rows = rows.contiguous()
        B = rows.numel()
    mode, mask = 0, None
    if flip is True:
        mode = 2
    elif flip is not None and flip is not False:
        if flip.device != data_u8.device or flip.dtype not in (torch.uint8, torch.bool) or flip.numel() != B:
            raise abi.GnfError("image_prep: the flip mask must be %d uint8 / bool entries on the device of the data" % B)
        mode, mask = 1, flip.contiguous().view(torch.uint8) if flip.dtype == torch.bool else flip.contiguous()
    if u is not None:
        if tuple(u.shape) != (B, d):
            raise abi.GnfError("image_prep: explicit uniforms must be [%d, %d]" % (B, d))
        u = u.contiguous()
    x = torch.empty((B, d), dtype=torch.float32, device=data_u8.device)
    term = torch.empty((B,), dtype=torch.float32, device=data_u8.device) if want_bpp else None
    call("gnf_image_prep", abi.rawptr(data_u8) if n else None, n, abi.rawptr(rows) if rows is not None and B else None, mode,
         abi.rawptr(mask) if mask is not None and B else None, c, h, w, ptr(u), int(seed), int(offset), float(alpha), ptr(x),
         ptr(term), B, stream())
    return x, term


# ----------------------------------------------------------------------------- toy-problem batches
# the 2-D base problems of the reference's lib/toy_data.py, in the numbering of gnf_toy_sample (include/gnf_hip.h)
TOY_KINDS = ("2igaussians", "2gaussians", "4gaussians", "8gaussians", "swissroll", "circles", "moons", "pinwheel", "2spirals",
             "checkerboard", "line", "line-noisy", "cos", "joint_gaussian")
TOY_MAX_BLOCKS = 8
# lib/toy_data.py:42-43 (8-MIX; 7-MIX, :55-56, is its first fourteen entries)
_TOY_MIX_STD = (1.604934, 1.584863, 2.0310535, 2.0305095, 1.337718, 1.4043778, 1.6944685, 1.6935346,
                1.7434783, 1.0092416, 1.4860426, 1.485661, 2.3067558, 2.311637, 1.4430547, 1.4430547)
# the composites as block lists (:16-59).  8-MIX in the order the reference concatenates (data1 .. data8, where `line` was
# assigned to data5 and `moons` to data8); the `std` vector is then applied to those columns as it stands
_TOY_COMPOSITES = {
    "2spirals-8gaussians": (("2spirals", "8gaussians"), None),
    "4-2spirals-8gaussians": (("2spirals", "8gaussians") * 2, None),
    "8-2spirals-8gaussians": (("2spirals", "8gaussians") * 4, None),
    "7-MIX": (("2spirals", "8gaussians", "swissroll", "circles", "moons", "pinwheel", "checkerboard"), _TOY_MIX_STD[:14]),
    "8-MIX": (("2spirals", "8gaussians", "swissroll", "circles", "line", "pinwheel", "checkerboard", "moons"), _TOY_MIX_STD),
}
TOY_DATASETS = TOY_KINDS + tuple(_TOY_COMPOSITES)      # the nineteen names of the toy driver's `datasets` list


def toy_blocks(name):
    """(block list as a tuple of TOY_KINDS indices, col_scale as a float32 numpy vector [2P] or None) of a data set of the toy
    driver: a base problem is one block; the MIX sets carry the reciprocals of the reference's `std` vector."""
    if name in _TOY_COMPOSITES:
        names, std = _TOY_COMPOSITES[name]
        scale = None if std is None else (np.float32(1.) / np.asarray(std, dtype=np.float32))
        return tuple(TOY_KINDS.index(n) for n in names), scale
    if name in TOY_KINDS:
        return (TOY_KINDS.index(name),), None
    raise abi.GnfError("unknown toy data set %r (one of %s)" % (name, ", ".join(TOY_DATASETS)))


def toy_sample(names_or_kinds, B, seed, offset, device, u=None, out=None, col_scale=None):
    """One launch of gnf_toy_sample (csrc/gnf_toy_data.hip): x [B, 2P] fp32 on `device`, block p a draw of a 2-D base problem.
    names_or_kinds: a data set name (base or composite: toy_blocks supplies blocks and column scale), or a sequence of base
    names / TOY_KINDS indices, at most eight, with an optional col_scale [2P].  (seed, offset): Philox key and call counter;
    row b of block p depends on (seed, offset, b, p, kind) only.  u: explicit uniforms [B, P, 8] (parity tests) or None.
    out: a [B, 2P] fp32 view to fill (unit column stride; its row stride is the kernel's ldx) -- returned.  No autograd node."""
    if isinstance(names_or_kinds, str):
        kinds, scale = toy_blocks(names_or_kinds)
        if col_scale is not None:
            raise abi.GnfError("toy_sample: a data set name brings its own column scale")
    else:
        kinds, scale = [], col_scale
        for k in names_or_kinds:
            if isinstance(k, str):
                if k not in TOY_KINDS:
                    raise abi.GnfError("toy_sample: %r is not a base problem (%s)" % (k, ", ".join(TOY_KINDS)))
                k = TOY_KINDS.index(k)
            if not isinstance(k, (int, np.integer)) or not 0 <= int(k) < len(TOY_KINDS):
                raise abi.GnfError("toy_sample: block kind %r is outside 0..%d" % (k, len(TOY_KINDS) - 1))
            kinds.append(int(k))
    P = len(kinds)
    if not 1 <= P <= TOY_MAX_BLOCKS:
        raise abi.GnfError("toy_sample takes 1..%d blocks: got %d" % (TOY_MAX_BLOCKS, P))
    B = int(B)
    if not 0 <= B <= 1 << 32:
        raise abi.GnfError("toy_sample: B = %d is outside 0..2^32" % B)
    device = torch.device(device)
    if device.type != "cuda":
        raise abi.GnfError("gnf_hip kernels run on the MI355X only: got device %s (no CPU fallback)" % device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if scale is not None:
        scale = np.ascontiguousarray(np.asarray(scale, dtype=np.float32))
        if scale.shape != (2 * P,):
            raise abi.GnfError("toy_sample: col_scale must have %d entries" % (2 * P))
    if u is not None:
        if u.device != device or u.dtype != torch.float32 or tuple(u.shape) != (B, P, 8):
            raise abi.GnfError("toy_sample: explicit uniforms must be fp32 [%d, %d, 8] on %s: got %s %s on %s"
                               % (B, P, device, u.dtype, tuple(u.shape), u.device))
        u = u.contiguous()
    if out is None:
        out = torch.empty((B, 2 * P), dtype=torch.float32, device=device)
    elif (out.device != device or out.dtype != torch.float32 or tuple(out.shape) != (B, 2 * P)
          or (B > 0 and out.stride(1) != 1) or (B > 1 and out.stride(0) < 2 * P)):
        raise abi.GnfError("toy_sample: out must be fp32 [%d, %d] on %s with unit column stride: got %s %s strides %s on %s"
                           % (B, 2 * P, device, out.dtype, tuple(out.shape), tuple(out.stride()), out.device))
    ldx = out.stride(0) if B > 1 else 2 * P
    karr = (ctypes.c_int32 * P)(*kinds)
    with torch.cuda.device(device):
        call("gnf_toy_sample", ctypes.cast(karr, ctypes.c_void_p), P,
             None if scale is None else ctypes.c_void_p(scale.ctypes.data), ptr(u) if B else None, int(seed), int(offset),
             ptr(out) if B else None, ldx, B, stream())
    return out


# ----------------------------------------------------------------------------- tabular batches from device memory
def shuffle_keys(seed, offset, n, device=None, out=None):
    """One launch of gnf_shuffle_keys (csrc/gnf_tab_batch.hip): int64 keys [n], keys[i] = (31 Philox bits << 32) | i, whose
    ascending sort is the permutation of epoch `offset` under key `seed` (the layout: include/gnf_hip.h).
    out: a contiguous int64 HIP tensor [n] to fill (returned), or None for a new one on `device`.  No autograd node."""
    n = int(n)
    if not 0 <= n < 1 << 31:
        raise abi.GnfError("shuffle_keys: n = %d is outside 0..2^31-1" % n)
    if out is None:
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise abi.GnfError("gnf_hip kernels run on the MI355X only: got device %s (no CPU fallback)" % device)
        out = torch.empty((n,), dtype=torch.int64, device=device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (n,) or not out.is_contiguous():
        raise abi.GnfError("shuffle_keys: out must be a contiguous int64 tensor [%d]: got %s %s" % (n, out.dtype, tuple(out.shape)))
    with torch.cuda.device(out.device):
        call("gnf_shuffle_keys", int(seed) & (1 << 64) - 1, int(offset) & (1 << 64) - 1, n, abi.rawptr(out) if n else None,
             stream())
    return out


def tab_batch(X, perm, first, stride, B, cursor=None, out=None):
    """One launch of gnf_tab_batch (csrc/gnf_tab_batch.hip): x [B, d], row r = X[perm[pos + r*stride]], pos = first
    (+ cursor[0] when `cursor`, a device int32 tensor, is given: the capturable form, nothing step-dependent by value).
    X: fp32 [n, d] on the GPU with unit column stride (any row stride: a column slice of a wider table is not copied).
    perm: int32 device tensor of row indices, or None for the identity.  Position and row index are clamped on the device;
    without a cursor a batch that runs past the permutation is refused.  out: a contiguous [B, d] fp32 tensor to fill
    (returned), or None for a new one.  The inputs are data: no autograd node."""
    if X.dim() != 2 or X.dtype != torch.float32 or not X.is_cuda:
        raise abi.GnfError("tab_batch needs an fp32 HIP tensor [n, d]: got %s %s on %s" % (X.dtype, tuple(X.shape), X.device))
    n, d = X.shape
    if d < 1 or (n > 0 and X.stride(1) != 1) or (n > 1 and X.stride(0) < d):
        X = X.contiguous()
    ldx = X.stride(0) if n > 1 else d
    B = int(B)
    for name, t in (("perm", perm), ("cursor", cursor)):
        if t is not None and (t.dtype != torch.int32 or t.device != X.device or not t.is_contiguous() or t.numel() < 1):
            raise abi.GnfError("tab_batch: %s must be a contiguous, non-empty int32 tensor on the device of the data" % name)
    if out is None:
        out = torch.empty((max(B, 0), d), dtype=torch.float32, device=X.device)
    elif out.dtype != torch.float32 or out.device != X.device or tuple(out.shape) != (B, d) or not out.is_contiguous():
        raise abi.GnfError("tab_batch: out must be a contiguous fp32 tensor [%d, %d] on %s: got %s %s on %s"
                           % (B, d, X.device, out.dtype, tuple(out.shape), out.device))
    call("gnf_tab_batch", ptr(X) if n else None, n, d, ldx, abi.rawptr(perm) if perm is not None else None,
         perm.numel() if perm is not None else 0, int(first), int(stride),
         abi.rawptr(cursor) if cursor is not None else None, ptr(out) if B > 0 else None, B, stream())
    return out


# ----------------------------------------------------------------------------- graph queries of the DAG conditioner
def dag_levels_supported(d):
    """the sizes gnf_dag_levels takes (1 <= d <= 4096)"""
    return bool(abi.load().gnf_dag_levels_supported(int(d)))


def dag_levels(M, thresholds=None):
    """Topological levels of the graphs `j -> i where pred(M[.., i, j])` in two launches (csrc/gnf_dag_graph.hip):
    -> (level int32, info int32).  level[.., i] = length of the longest parent chain of node i, -1 on or behind a cycle;
    info[..] = (n_levelled, n_levels): acyclic iff n_levelled == d, and the depth is then n_levels - 1.
    M: [d, d] or [G, d, d] on the GPU, fp32 or bool / uint8, any row stride (a view of a flat parameter buffer).
    thresholds None: the predicate is M != 0 (a NaN is an edge).  thresholds = G floats (a sequence or an fp32 tensor; fp32 M
    only): M > thresholds[g], compared in fp32 like torch's `tensor > python_float`; with a [d, d] matrix they all share it.
    Shapes: [d] and [2] for a [d, d] matrix without thresholds, else [G, d] and [G, 2].  Integers: no autograd node."""
    if not M.is_cuda:
        raise abi.GnfError("gnf_hip kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % M.device)
    M = M.detach()
    if M.dtype == torch.bool:
        M = M.view(torch.uint8)
    if M.dtype not in (torch.float32, torch.uint8):
        raise abi.GnfError("dag_levels takes fp32 or bool / uint8: got %s" % M.dtype)
    if M.dim() not in (2, 3) or M.shape[-1] != M.shape[-2]:
        raise abi.GnfError("dag_levels needs [d, d] or [G, d, d]: got %s" % (tuple(M.shape),))
    d = M.shape[-1]
    if thresholds is not None:
        if M.dtype != torch.float32:
            raise abi.GnfError("dag_levels: thresholds need an fp32 matrix")
        if not torch.is_tensor(thresholds):
            thresholds = torch.tensor([float(t) for t in thresholds], dtype=torch.float32)     # RNE, as torch rounds a scalar
        thresholds = thresholds.to(device=M.device, dtype=torch.float32).contiguous().view(-1)
    squeeze = M.dim() == 2 and thresholds is None
    G = M.shape[0] if M.dim() == 3 else (1 if thresholds is None else thresholds.numel())
    if thresholds is not None and thresholds.numel() != G:
        raise abi.GnfError("dag_levels: %d thresholds for %d graphs" % (thresholds.numel(), G))
    if d > 1 and (M.stride(-1) != 1 or M.stride(-2) < d):
        M = M.contiguous()
    level = torch.empty((G, d), dtype=torch.int32, device=M.device)
    info = torch.empty((G, 2), dtype=torch.int32, device=M.device)
    nws = abi.load().gnf_dag_levels_ws_bytes(G, d)
    abi.check(min(nws, 0), "gnf_dag_levels_ws_bytes")
    ws = _ws(nws + 8, M)
    off = (-ws.data_ptr()) % 8                                   # the words are 64-bit: 8-byte aligned whatever the allocator gave
    call("gnf_dag_levels", abi.rawptr(M) if G else None, abi.DAG_ELEM_F32 if M.dtype == torch.float32 else abi.DAG_ELEM_U8,
         (M.stride(0) if G > 1 else 0) if M.dim() == 3 else 0, M.stride(-2) if d > 1 else d, ptr(thresholds) if G else None,
         abi.rawptr(level) if G else None, abi.rawptr(info), ctypes.c_void_p(ws.data_ptr() + off), nws, G, d, stream())
    return (level[0], info[0]) if squeeze else (level, info)


# ----------------------------------------------------------------------------- Adam on a flat buffer
def adam_step(p, g, m, v, step, lr=1e-3, betas=(.9, .999), eps=1e-8, weight_decay=0., grad_scale=1.):
    call("gnf_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, betas[0], betas[1], eps, weight_decay,
         grad_scale, int(step), stream())


def adam_step_dev(p, g, m, v, step_dev, lr=1e-3, betas=(.9, .999), eps=1e-8, weight_decay=0., grad_scale=1.,
                  advance=True):
    """Adam with the step counter in device memory (int32 tensor, incremented by the call): graph-capturable."""
    if step_dev.dtype != torch.int32 or not step_dev.is_cuda or step_dev.numel() < 2 or not step_dev.is_contiguous():
        raise abi.GnfError("step_dev must be a contiguous int32 HIP tensor {steps taken, 0}")
    call("gnf_adam_step_dev", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, betas[0], betas[1], eps, weight_decay,
         grad_scale, abi.rawptr(step_dev), int(bool(advance)), stream())


class PowerTraceFn(torch.autograd.Function):
    """tr(B^k) of the DAG acyclicity term (DAGConditioner.py:192-194) with the closed-form gradient
    d tr(B^k) / dB = k (B^(k-1))^T: one power B^(k-1) serves the value (tr(B^k) = sum_ij (B^(k-1))_ij B_ji) and the
    gradient, instead of autograd through every product of torch.matrix_power (6 instead of 18 d x d GEMMs per step
    at d = 784, k = 34).  The GEMMs themselves stay on the library."""

    @staticmethod
    def forward(ctx, B, k):
        k = int(k)
        ctx.k = k
        if k == 0:
            ctx.save_for_backward(None)
            return B.new_tensor(float(B.shape[0]))
        P = torch.matrix_power(B, k - 1)
        ctx.save_for_backward(P)
        return (P * B.t()).sum()

    @staticmethod
    def backward(ctx, g):
        (P,) = ctx.saved_tensors
        if ctx.k == 0:
            return None, None
        return (g * ctx.k) * P.t(), None



class DagLossFn(torch.autograd.Function):
    """dag_const (lambd h + c/2 h^2) + l1 mean|A| with h = tr((I + alpha A o A)^k) - d  (DAGConditioner.py:176-194,
    268-271): three fused launches around the library matrix power instead of ~40 elementwise ones; the conditioner's
    scalar buffers are read on the device (no host synchronisation).  Returns the loss; `.trace` of the ctx-less call is
    available through dag_loss_terms()."""

    @staticmethod
    def forward(ctx, A, alpha, alpha_factor, lambd, c, dag_const, l1_weight, k):
        A = A.contiguous()
        d = A.shape[0]
        k = int(k)
        f32 = lambda t: torch.as_tensor(t, dtype=torch.float32, device=A.device).detach().reshape(1)   # buffers or floats
        al, lm, cc, dc, l1 = f32(alpha), f32(lambd), f32(c), f32(dag_const), f32(l1_weight)
        Bm = _empty((d, d), A)
        call("gnf_dag_loss_prep", ptr(A), ptr(al), float(alpha_factor), ptr(Bm), d, stream())
        P = torch.matrix_power(Bm, k - 1) if k > 0 else None
        out4, ws = _empty((4,), A), _empty((512,), A)
        call("gnf_dag_loss_value", ptr(A), ptr(Bm), ptr(P), ptr(al), float(alpha_factor), ptr(lm), ptr(cc), ptr(dc),
             ptr(l1), k, ptr(out4), ptr(ws), d, stream())
        ctx.save_for_backward(A, P, out4)
        return out4[0]

    @staticmethod
    def backward(ctx, g):
        A, P, out4 = ctx.saved_tensors
        gA, finish, _ = grad_out_shared(A)
        call("gnf_dag_loss_bwd", ptr(A), ptr(P), ptr(out4), ptr(g.contiguous().reshape(1)), ptr(gA), A.shape[0], stream())
        return finish(gA), None, None, None, None, None, None, None
