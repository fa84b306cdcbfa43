"""References of NormalizingFlowStep.rsample_do's backward (tests/test_rsample_do_host.py, tests/test_gpu_rsample_do.py):
plain torch and numpy on the CPU.

The law under do(x_P = v).  One step z = S(x), J = dz/dx = D + N at the sample, D = diag(jac), N strictly triangular in
topological order.  The equations of the free set F are kept, those of P read x_P = v, so for g = dL/dx
    lambda_P = 0,   J_FF^T lambda_F = g_F,   dL/dv = g_P - (N^T lambda)_P.
law_sweep_do (MADE) and law_levels_do (StrADE) are adjoint_ref.law_sweep / strade_adjoint_ref.law_levels with the pin rule:
at a pinned variable u is computed as ever, lambda := 0 and gdo := g - u by SELECTION (jac and dzdh of a pinned element are
never read), and the cotangent row of its outputs is zeros.  They skip nothing: what the kernels skip is exactly zero here.
mutilated_solve assembles the mutilated system densely and solves it with torch.linalg.solve: the check of the law.

intervene_t: a differentiable restatement of NormalizingFlowStep.intervene (an Affine step unless another inverse is handed
in), in the dtype of its inputs: depth + 1 passes of x <- where(pinned, v, T^-1(z, h(x))).  loss_do_t: -mean_b sum_{i free} (log jac_bi + log N(z_bi))."""
import math

import numpy as np
import torch

from adjoint_ref import ordered_layers
from oracle import gnf_oracle as O
from strade_adjoint_ref import _replay, level_images

# the pin patterns of the issue, by position in the topological order the caller hands in (degree order for a MADE, level
# order for a StrADE net): name -> positions pinned, or None where d does not allow the pattern
PATTERNS = ("none", "first", "last", "every-second", "trailing-3", "all-but-one", "all")


def pattern(name, d):
    """positions (in topological order) pinned by pattern `name` for d variables; None when d is too small for it to differ
    from a pattern listed before it"""
    if name == "none":
        return []
    if name == "first":
        return [0]
    if name == "last":
        return [d - 1] if d >= 2 else None
    if name == "every-second":
        return list(range(1, d, 2)) if d >= 3 else None
    if name == "trailing-3":
        return list(range(d - 3, d)) if d >= 5 else None
    if name == "all-but-one":
        return [p for p in range(d) if p != d // 2] if d >= 3 else None
    if name == "all":
        return list(range(d)) if d >= 2 else None
    raise KeyError(name)


def pin_of(positions, order, d):
    """bool [d] by VARIABLE for pinned positions of the topological order `order` (position -> variable)"""
    pin = torch.zeros(d, dtype=torch.bool)
    for p in positions:
        pin[int(order[p])] = True
    return pin


# ------------------------------------------------------------------------------------------------------- MADE
def law_sweep_do(layers, plan, c, x, ctx, g, jac, dzdh, pin):
    """(lambda, gdo) [B, d] of the MADE step at x under do(x_pin = .): adjoint_ref.law_sweep with the pin rule.  pin: bool
    [d] by variable.  All floating tensors in the dtype of x."""
    d, out, off, var = plan["d"], plan["out"], [np.asarray(o) for o in plan["off"]], [int(v) for v in plan["var_of_step"]]
    nh, B = len(plan["widths"]), x.shape[0]
    P = ordered_layers(layers, plan, c)
    a_in = torch.cat((ctx, x[:, var]), 1)
    acts = [x.new_zeros(B, w) for w in plan["widths"]]
    for t in range(1, d):
        for l in range(nh):
            n0, n1 = int(off[l][t - 1]), int(off[l][t])
            K = c + t if l == 0 else int(off[l - 1][t])
            src = a_in if l == 0 else acts[l - 1]
            acts[l][:, n0:n1] = torch.relu(src[:, :K] @ P[l][0][n0:n1, :K].t() + P[l][1][n0:n1])
    dec = [(a > 0).to(x.dtype) for a in acts]
    go = x.new_zeros(B, d * out)
    cot = [torch.zeros_like(a) for a in acts]
    lam, gdo = torch.zeros_like(x), torch.zeros_like(x)
    for t in range(d - 1, -1, -1):
        for l in range(nh - 1, -1, -1):
            n0, n1 = int(off[l][t]), int(off[l][t + 1])
            if l == nh - 1:
                r0 = (t + 1) * out
                val = go[:, r0:] @ P[nh][0][r0:, n0:n1]
            else:
                r0 = int(off[l + 1][t])
                val = cot[l + 1][:, r0:] @ P[l + 1][0][r0:, n0:n1]
            cot[l][:, n0:n1] = val * dec[l][:, n0:n1]
        if nh > 0:
            r0 = int(off[0][t])
            u = cot[0][:, r0:] @ P[0][0][r0:, c + t]
        else:
            r0 = (t + 1) * out
            u = go[:, r0:] @ P[0][0][r0:, c + t]
        v = var[t]
        if bool(pin[v]):
            gdo[:, v] = g[:, v] - u                     # lambda stays 0, the output cotangents stay 0: selection
        else:
            lam[:, v] = (g[:, v] - u) / jac[:, v]
            go[:, t * out:(t + 1) * out] = lam[:, v:v + 1] * dzdh[:, v, :]
    return lam, gdo


# ----------------------------------------------------------------------------------------------------- StrADE
def law_levels_do(layers, masks, plan, c, x, ctx, g, jac, dzdh, pin):
    """(lambda, gdo) [B, d] of the StrADE step at x under do(x_pin = .): strade_adjoint_ref.law_levels with the pin rule"""
    d, out = plan["d"], plan["out"]
    off, var_off = [np.asarray(o) for o in plan["off"]], np.asarray(plan["var_off"])
    var = [int(v) for v in plan["var_order"]]
    nh, nlev, B = len(plan["widths"]), plan["nlev"], x.shape[0]
    P = level_images(layers, masks, plan, c)
    acts, _ = _replay(P, plan, c, x, ctx)
    dec = [(a > 0).to(x.dtype) for a in acts]
    go = x.new_zeros(B, d * out)
    cot = [torch.zeros_like(a) for a in acts]
    lam, gdo = torch.zeros_like(x), torch.zeros_like(x)
    for t in range(nlev - 1, -1, -1):
        p0, p1 = int(var_off[t]), int(var_off[t + 1])
        for l in range(nh - 1, -1, -1):
            n0, n1 = int(off[l][t]), int(off[l][t + 1])
            if l == nh - 1:
                r0 = p1 * out
                val = go[:, r0:] @ P[nh][0][r0:, n0:n1]
            else:
                r0 = int(off[l + 1][t])
                val = cot[l + 1][:, r0:] @ P[l + 1][0][r0:, n0:n1]
            cot[l][:, n0:n1] = val * dec[l][:, n0:n1]
        for p in range(p0, p1):
            if nh > 0:
                r0 = int(off[0][t])
                u = cot[0][:, r0:] @ P[0][0][r0:, c + p]
            else:
                r0 = p1 * out
                u = go[:, r0:] @ P[0][0][r0:, c + p]
            v = var[p]
            if bool(pin[v]):
                gdo[:, v] = g[:, v] - u
            else:
                lam[:, v] = (g[:, v] - u) / jac[:, v]
        for p in range(p0, p1):
            v = var[p]
            if not bool(pin[v]):
                go[:, p * out:(p + 1) * out] = lam[:, v:v + 1] * dzdh[:, v, :]
    return lam, gdo


def law64_do(cond, x, ctx, g, jac, dzdh, pin):
    """the fp64 StrADE law for operands of any device and dtype (strade_adjoint_ref.law64 with the pin table)"""
    from strade_adjoint_ref import layers_of, numpy_plan
    c64 = lambda t: t.detach().cpu().double()
    layers, masks = layers_of(cond)
    ctx64 = c64(ctx) if ctx is not None else torch.zeros(x.shape[0], 0, dtype=torch.float64)
    return law_levels_do(layers, masks, numpy_plan(cond), cond.cond_in, c64(x), ctx64, c64(g), c64(jac), c64(dzdh),
                         pin.cpu().bool())


# ------------------------------------------------------------------------------------- the dense mutilated system
def mutilated_solve(h_fn, x, g, jac, dzdh, pin):
    """(lambda, gdo, condition numbers [B]) from the assembled Jacobian: N[b] = sum_k dzdh[b, i, k] dh[b, i, k] / dx[b, j]
    by autograd on h_fn ((x [1, d], sample index b) -> h [1, d, out]), J = diag(jac) + N; lambda_F = J_FF^-T g_F, lambda_P = 0,
    gdo_P = g_P - J_FP^T lambda_F (= g_P - (N^T lambda)_P: D has no FP entries), gdo_F = 0"""
    B, d = x.shape
    F, Pn = (~pin).nonzero().flatten(), pin.nonzero().flatten()
    lam, gdo, conds = torch.zeros_like(x), torch.zeros_like(x), []
    for b in range(B):
        dh = torch.autograd.functional.jacobian(lambda v: h_fn(v[None], b)[0], x[b])           # [d, out, d]
        J = torch.diag(jac[b]) + torch.einsum("ik,ikj->ij", dzdh[b], dh)
        if len(F):
            JFF = J[F][:, F]
            lam[b, F] = torch.linalg.solve(JFF.t(), g[b, F])
            conds.append(torch.linalg.cond(JFF).item())
        if len(Pn):
            gdo[b, Pn] = g[b, Pn] - (J[F][:, Pn].t() @ lam[b, F] if len(F) else 0.)
    return lam, gdo, conds


# ------------------------------------------------------------------- intervene and loss_do, differentiable, any dtype
def intervene_t(cfn, depth, z, pin, vals, inv=O.affine_inverse):
    """NormalizingFlowStep.intervene unrolled: x <- where(pinned, vals, inv(z, cfn(x))) from where(pinned, vals, 0),
    depth + 1 passes.  pin: bool [d]; vals [B, d], read at the pinned columns only; inv: the normalizer's inverse."""
    x = torch.where(pin, vals, torch.zeros_like(z))
    if bool(pin.all()):
        return x
    for _ in range(depth + 1):
        x = torch.where(pin, vals, inv(z, cfn(x)))
    return x


def loss_do_t(cfn, x, pin, fwd=O.affine_forward):
    """-mean_b sum_{i free} (log jac_bi + log N(z_bi)): FCNormalizingFlow.loss_do of a one-step flow with a standard-normal
    base, without its constraint term; the terms of the pinned variables are left out by selection.  fwd: the normalizer"""
    zz, jac = fwd(x, cfn(x))
    terms = torch.log(jac) - .5 * zz * zz - .5 * math.log(2. * math.pi)
    return -torch.where(pin, torch.zeros_like(terms), terms).sum(1).mean()
