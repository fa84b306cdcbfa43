"""References of NormalizingFlowStep.rsample's backward (tests/test_rsample_host.py, tests/test_gpu_rsample.py): plain torch
on the CPU.

law_sweep: the transposed column sweep of csrc/gnf_made_adjoint.hip restated from the plan tables alone
(made_prefix_plan: order, off, var_of_step) -- no mask is read, the suffix start IS the mask.  In fp64 it is the law the
kernel is held to; tests/test_rsample_host.py checks it against torch.linalg.solve on the assembled Jacobian.

made_t / flow_steps / flow_invert / flow_forward: a MADE or Coupling + Affine flow and its inverse unrolled into depth() + 1
passes, in the dtype of the leaves handed in: fp64 it is the reference of the whole gradients, fp32 the plain-torch
comparator."""
import numpy as np
import torch

from oracle import gnf_oracle as O


def plan_of(cond):
    """the numpy plan of an AutoregressiveConditioner's net in force"""
    from models.Conditionners.AutoregressiveConditioner import made_prefix_plan
    net = cond.masked_autoregressive_net
    return made_prefix_plan(net.m, net.nin, net.nout)


def ordered_layers(layers, plan, c):
    """[(Wp, bp)] in degree order: rows of hidden layer l = order[l], columns = the layer below in its order; the first
    layer's columns are [context | var_of_step]; output row t * out + k is neuron k * d + var_of_step[t]"""
    d, out, order, var = plan["d"], plan["out"], plan["order"], plan["var_of_step"]
    nh = len(plan["widths"])
    cols0 = torch.as_tensor(list(range(c)) + [c + int(v) for v in var], dtype=torch.long)
    res = []
    for l, (W, b) in enumerate(layers):
        rows = (torch.as_tensor(np.asarray(order[l]), dtype=torch.long) if l < nh else
                torch.as_tensor([k * d + int(var[t]) for t in range(d) for k in range(out)], dtype=torch.long))
        cols = cols0 if l == 0 else torch.as_tensor(np.asarray(order[l - 1]), dtype=torch.long)
        res.append((W[rows][:, cols], b[rows]))
    return res


def law_sweep(layers, plan, c, x, ctx, g, jac, dzdh):
    """lambda [B, d] with J^T lambda = g for the MADE step at x.  layers: [(W, b)] in nn.Linear layout, UNMASKED; plan: the
    numpy tables; x, g, jac [B, d]; ctx [B, c]; dzdh [B, d, out].  All in the dtype of x."""
    d, out, off, var = plan["d"], plan["out"], [np.asarray(o) for o in plan["off"]], [int(v) for v in plan["var_of_step"]]
    nh, B = len(plan["widths"]), x.shape[0]
    P = ordered_layers(layers, plan, c)
    # replay: the hidden units of degree t - 1 from the prefixes of step t
    a_in = torch.cat((ctx, x[:, var]), 1)
    acts = [x.new_zeros(B, w) for w in plan["widths"]]
    for t in range(1, d):
        for l in range(nh):
            n0, n1 = int(off[l][t - 1]), int(off[l][t])
            K = c + t if l == 0 else int(off[l - 1][t])
            src = a_in if l == 0 else acts[l - 1]
            acts[l][:, n0:n1] = torch.relu(src[:, :K] @ P[l][0][n0:n1, :K].t() + P[l][1][n0:n1])
    dec = [(a > 0).to(x.dtype) for a in acts]
    # the sweep: suffixes
    go = x.new_zeros(B, d * out)
    cot = [torch.zeros_like(a) for a in acts]
    lam = torch.zeros_like(x)
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
        lam[:, v] = (g[:, v] - u) / jac[:, v]
        go[:, t * out:(t + 1) * out] = lam[:, v:v + 1] * dzdh[:, v, :]
    return lam


def made_layers(cond, dtype=torch.float64):
    return [(l.weight.detach().cpu().to(dtype), l.bias.detach().cpu().to(dtype))
            for l in cond.masked_autoregressive_net.masked_layers()]


# ---------------------------------------------------------------------------------------- flows in the leaves' dtype
def _pairs(P, prefix):
    out, k = [], 0
    while "%snet.%d.weight" % (prefix, k) in P:
        out.append((P["%snet.%d.weight" % (prefix, k)], P["%snet.%d.bias" % (prefix, k)]))
        k += 2
    return out


def made_t(cond, P, x, ctx, prefix=""):
    """context_ref.made64 in the dtype of the leaves P (that one multiplies by fp64 masks, which promotes fp32 leaves)"""
    net = cond.masked_autoregressive_net
    a = torch.cat((ctx, x), 1)
    layers = _pairs(P, prefix + "masked_autoregressive_net.")
    for li, ((W, b), l) in enumerate(zip(layers, net.masked_layers())):
        a = a @ (l.mask.detach().cpu().to(W.dtype) * W).t() + b
        if li < len(layers) - 1:
            a = torch.relu(a)
    return a.view(x.shape[0], -1, x.shape[1]).permute(0, 2, 1)


def leaves(module, dtype):
    return {n: p.detach().cpu().to(dtype).clone().requires_grad_(True) for n, p in module.named_parameters()}


def flow_steps(flow, P, ctx):
    """[(conditioner fn, depth)] of an FCNormalizingFlow of Autoregressive / Coupling steps with Affine normalizers"""
    from context_ref import coupling64
    from models import AffineNormalizer, AutoregressiveConditioner, CouplingConditioner
    steps = []
    for k, step in enumerate(flow.steps):
        cond, pre = step.conditioner, "steps.%d.conditioner." % k
        assert isinstance(step.normalizer, AffineNormalizer)
        if isinstance(cond, CouplingConditioner):
            steps.append((lambda v, cond=cond, pre=pre: coupling64(cond, P, v, ctx, pre), 1))
        else:
            assert isinstance(cond, AutoregressiveConditioner)
            steps.append((lambda v, cond=cond, pre=pre: made_t(cond, P, v, ctx, pre), cond.in_size - 1))
    return steps


def flow_invert(steps, z):
    """FCNormalizingFlow.invert unrolled: every step depth + 1 differentiable passes from x = 0, last step first"""
    for k in range(len(steps) - 1, -1, -1):
        cfn, depth = steps[k]
        x = torch.zeros_like(z)
        for _ in range(depth + 1):
            x = O.affine_inverse(z, cfn(x))
        z = torch.flip(x, dims=[1]) if k else x
    return z


def flow_forward(steps, x):
    return O.fc_flow_forward(x, [(cfn, O.affine_forward) for cfn, _ in steps])


def elbo_like(flow, P, z, ctx, w):
    """L = sum w x + loss(forward(x, c)) with x = invert(z, c), everything differentiable in the leaves' dtype"""
    steps = flow_steps(flow, P, ctx)
    x = flow_invert(steps, z)
    zz, logdet = flow_forward(steps, x)
    return (w * x).sum() + O.flow_loss(zz, logdet)
