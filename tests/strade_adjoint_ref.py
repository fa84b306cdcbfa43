"""References and operands of the StrADE adjoint level sweep (csrc/gnf_strade_adjoint.hip): plain torch on the CPU, shared by
tests/test_strade_adjoint_host.py and tests/test_gpu_strade_adjoint.py.

law_levels: the transposed level sweep restated from the tables of strade_level_plan (var_order, var_off, order, off) and the
level-ordered images of mask o W.  The suffix start is NOT the mask: the images hold exact zeros where the mask forbids.  In
fp64 it is the law the kernel is held to; the host test checks it against torch.linalg.solve on the assembled Jacobian.

The graphs are those of tests/test_gpu_strade.py, restated.  operands() builds a conditioner on the CPU (weights doubled, so
that the off-diagonal part of J is large enough for two summation orders to show in lambda) and synthetic positive jac and
dzdh, as _kernel_operands of tests/test_gpu_rsample.py does.

ReLU margin: a ReLU decision within a rounding of zero makes lambda differ at order one between two correct fp32 evaluations,
which no error rule absorbs.  The seeds are therefore chosen such that in fp64 every hidden pre-activation of a case has
|pre| >= MARGIN * max|pre| of that case (relu_margin; asserted by the host test).  SEED_BUMP lists the cases whose first
seed failed that and how far the seed was moved."""
import numpy as np
import torch

CHUNK = 8                       # GNF_STRADE_CHUNK_VARS
MARGIN = 1e-4


# ------------------------------------------------------------------------------------------------------------ graphs
def _layered(sizes, seed, max_parents=3):
    """a DAG whose level t holds sizes[t] variables: every variable of level t > 0 has a parent in level t - 1 and parents
    among the first `max_parents` variables of the levels below (few distinct parent sets), under a random relabelling"""
    rng = np.random.RandomState(seed)
    d = sum(sizes)
    a = np.zeros((d, d), dtype=np.uint8)
    start = np.concatenate([[0], np.cumsum(sizes)])
    for t in range(1, len(sizes)):
        prev = np.arange(start[t - 1], start[t])[:max_parents]
        older = np.arange(0, start[t - 1])[:max_parents]
        for i in range(start[t], start[t + 1]):
            a[i, rng.choice(prev)] = 1
            for j in older:
                if rng.rand() < .4:
                    a[i, j] = 1
    perm = rng.permutation(d)
    out = np.zeros_like(a)
    out[np.ix_(perm, perm)] = a
    return out


def _d17():
    """levels of 3, 9 and 5 variables; the 9 take the seven non-empty subsets of the roots as parent sets, the 5 share two"""
    a = np.zeros((17, 17), dtype=np.uint8)
    for k in range(9):
        for j in range(3):
            if (k % 7 + 1) >> j & 1:
                a[3 + k, j] = 1
    for k in range(5):
        a[12 + k, [3, 0] if k % 2 == 0 else [4, 5]] = 1
    perm = np.random.RandomState(1).permutation(17)
    out = np.zeros_like(a)
    out[np.ix_(perm, perm)] = a
    return out


GRAPHS = {
    "d1": np.zeros((1, 1), dtype=np.uint8),
    "d2": np.array([[0, 0], [1, 0]], dtype=np.uint8),
    "chain5": np.eye(5, k=-1, dtype=np.uint8),
    "d17": _d17(),
    "wide": _layered([2, 2 * CHUNK + 3, 2], 2),
}
KINDS = ("none", "R", "40-24")
GRID = [(name, kind, c, out) for name in GRAPHS for kind in KINDS for c in (0, 3) for out in (2, 23)]
BATCHES = (5, 37)               # a ragged tile; several tiles


def case_id(case):
    return "%s-%s-c%d-out%d" % case


def hidden_of(name, kind, c):
    from models.Conditionners.StrADEConditioner import strade_sets
    if kind == "none":
        return []
    return [max(strade_sets(GRAPHS[name], c)[1], 1)] if kind == "R" else [40, 24]


# ------------------------------------------------------------------------------------------------------------ the law
def numpy_plan(cond):
    """strade_level_plan of a StrADEConditioner's adjacency buffer, tables on the host"""
    from models.Conditionners.StrADEConditioner import strade_level_plan
    return strade_level_plan(cond.adjacency.detach().cpu().numpy(), cond.hidden, cond.out_size, cond.cond_in)


def layers_of(cond, dtype=torch.float64):
    """([(W, b)], [mask]) of the conditioner's net in `dtype` on the CPU"""
    ls = cond._layers()
    return ([(l.weight.detach().cpu().to(dtype), l.bias.detach().cpu().to(dtype)) for l in ls],
            [l.mask.detach().cpu().to(dtype) for l in ls])


def level_images(layers, masks, plan, c):
    """[(P, b)]: mask o W and the biases in level order, as strade_pack_k builds them: rows of hidden layer l = order[l],
    output row q * out + k = neuron k * d + var_order[q]; the first layer's columns are [context | var_order], a later
    layer's the units below in their order"""
    d, out, order, var = plan["d"], plan["out"], plan["order"], plan["var_order"]
    nh = len(plan["widths"])
    cols0 = torch.as_tensor(list(range(c)) + [c + int(v) for v in var], dtype=torch.long)
    res = []
    for l, ((W, b), M) in enumerate(zip(layers, masks)):
        rows = (torch.as_tensor(np.asarray(order[l]), dtype=torch.long) if l < nh else
                torch.as_tensor([k * d + int(var[q]) for q in range(d) for k in range(out)], dtype=torch.long))
        cols = cols0 if l == 0 else torch.as_tensor(np.asarray(order[l - 1]), dtype=torch.long)
        res.append((torch.where(M != 0, W, torch.zeros_like(W))[rows][:, cols], b[rows]))
    return res


def _replay(P, plan, c, x, ctx):
    """the forward level sweep's hidden units: (activations, pre-activations of the units it evaluates) per layer"""
    off, var_off = [np.asarray(o) for o in plan["off"]], np.asarray(plan["var_off"])
    var = [int(v) for v in plan["var_order"]]
    nh, nlev, B = len(plan["widths"]), plan["nlev"], x.shape[0]
    a_in = torch.cat((ctx, x[:, var]), 1)
    acts = [x.new_zeros(B, w) for w in plan["widths"]]
    pres = []
    for t in range(nlev):
        for l in range(nh):
            n0, n1 = (int(off[l][t - 1]) if t >= 1 else 0), int(off[l][t])
            K = c + int(var_off[t]) if l == 0 else int(off[l - 1][t])
            src = a_in if l == 0 else acts[l - 1]
            pre = src[:, :K] @ P[l][0][n0:n1, :K].t() + P[l][1][n0:n1]
            pres.append(pre)
            acts[l][:, n0:n1] = torch.relu(pre)
    return acts, pres


def law_levels(layers, masks, plan, c, x, ctx, g, jac, dzdh):
    """lambda [B, d] with J^T lambda = g for the StrADE step at x.  layers: [(W, b)] in nn.Linear layout, masks alongside;
    plan: strade_level_plan's numpy tables; x, g, jac [B, d]; ctx [B, c]; dzdh [B, d, out], by variable index.  All in the
    dtype of x."""
    d, out = plan["d"], plan["out"]
    off, var_off = [np.asarray(o) for o in plan["off"]], np.asarray(plan["var_off"])
    var = [int(v) for v in plan["var_order"]]
    nh, nlev, B = len(plan["widths"]), plan["nlev"], x.shape[0]
    P = level_images(layers, masks, plan, c)
    acts, _ = _replay(P, plan, c, x, ctx)
    dec = [(a > 0).to(x.dtype) for a in acts]
    go = x.new_zeros(B, d * out)
    cot = [torch.zeros_like(a) for a in acts]
    lam = torch.zeros_like(x)
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
            lam[:, v] = (g[:, v] - u) / jac[:, v]
        for p in range(p0, p1):                          # after the level's u: variables of one level never read each other
            v = var[p]
            go[:, p * out:(p + 1) * out] = lam[:, v:v + 1] * dzdh[:, v, :]
    return lam


def masked_forward(layers, masks, x, ctx):
    """(h [B, d, out], [pre-activations per hidden layer]) of the masked net, plain and dense, in the dtype of x"""
    a, pres = torch.cat((ctx, x), 1), []
    for k, ((W, b), M) in enumerate(zip(layers, masks)):
        a = a @ (W * M).t() + b
        if k < len(layers) - 1:
            pres.append(a)
            a = torch.relu(a)
    return a.view(x.shape[0], -1, x.shape[1]).permute(0, 2, 1), pres


def relu_margin(layers, masks, x, ctx):
    """min|pre| / max|pre| over every hidden pre-activation of the case (inf without a hidden layer)"""
    _, pres = masked_forward(layers, masks, x, ctx)
    if not pres:
        return float("inf")
    flat = torch.cat([p.reshape(-1) for p in pres]).abs()
    return (flat.min() / flat.max()).item()


# ------------------------------------------------------------------------------------------------------------ operands
# (case_id, B) -> how far the seed of a case was moved for the ReLU margin
SEED_BUMP = {("d1-40-24-c3-out2", 37): 2, ("d2-40-24-c0-out2", 37): 1, ("d2-40-24-c0-out23", 37): 5, ("d2-40-24-c3-out2", 37): 2,
             ("chain5-40-24-c0-out2", 37): 1, ("chain5-40-24-c3-out2", 5): 1, ("d17-40-24-c0-out2", 37): 2,
             ("d17-40-24-c3-out2", 37): 1, ("d17-40-24-c3-out23", 37): 3, ("wide-40-24-c0-out2", 37): 1,
             ("wide-40-24-c0-out23", 37): 2, ("wide-40-24-c3-out2", 37): 1}


def build_cond(name, kind, c, out, seed):
    """a StrADEConditioner on the CPU, twice the initial weights"""
    from models import StrADEConditioner
    a = GRAPHS[name]
    torch.manual_seed(seed)
    cond = StrADEConditioner(a.shape[0], hidden_of(name, kind, c), out, cond_in=c, adjacency=a)
    with torch.no_grad():
        for l in cond._layers():
            l.weight.mul_(2.)
    return cond


def operands(case, B):
    """(cond on the CPU, x, ctx or None, g, jac, dzdh) in fp32 on the CPU for a case of GRID and a batch size"""
    name, kind, c, out = case
    d = GRAPHS[name].shape[0]
    seed = 100 * d + 10 * c + out + B + 7919 * SEED_BUMP.get((case_id(case), B), 0)
    cond = build_cond(name, kind, c, out, seed)
    gen = torch.Generator().manual_seed(1000 + seed)
    x, g = .7 * torch.randn(B, d, generator=gen), torch.randn(B, d, generator=gen)
    ctx = torch.randn(B, c, generator=gen) if c else None
    jac = .5 + torch.rand(B, d, generator=gen)                        # synthetic and positive
    dzdh = .5 + torch.rand(B, d, out, generator=gen)
    return cond, x, ctx, g, jac, dzdh


def law64(cond, x, ctx, g, jac, dzdh):
    """the fp64 law for operands of any device and dtype"""
    c64 = lambda t: t.detach().cpu().double()
    layers, masks = layers_of(cond)
    ctx64 = c64(ctx) if ctx is not None else torch.zeros(x.shape[0], 0, dtype=torch.float64)
    return law_levels(layers, masks, numpy_plan(cond), cond.cond_in, c64(x), ctx64, c64(g), c64(jac), c64(dzdh))


def tile_rows_of(plan, B):
    """the tile height both StrADE kernels choose for a net far below the LDS limit (strade_tile_rows, gnf_strade.h)"""
    hstride = min(plan["widest"], CHUNK) * plan["out"]
    if max(plan["max_new"], hstride) >= 8 or plan["out"] >= 8:
        return 16
    return 4 if (B + 3) // 4 <= 1024 else 8 if (B + 7) // 8 <= 1024 else 16


def sweep_products(plan):
    """the n of every suffix product of the adjoint sweep: units of a level per layer, variables per chunk"""
    ns = []
    var_off = np.asarray(plan["var_off"])
    for t in range(plan["nlev"]):
        ns += [int(o[t + 1] - o[t]) for o in plan["off"]]
        w = int(var_off[t + 1] - var_off[t])
        ns += [min(CHUNK, w - q) for q in range(0, w, CHUNK)]
    return [n for n in ns if n > 0]
