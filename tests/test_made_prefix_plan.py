"""The host plan of the column-by-column MADE inversion (models/Conditionners/AutoregressiveConditioner.py:
made_prefix_plan, MADE.prefix_plan) -- no GPU needed.  The plan is checked by brute force against the degrees and against
the module's own mask buffers, and the schedule it describes is restated in fp64 and compared with the reference's d
fixed-point passes (NormalizingFlow.py:98-107)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from models import AutoregressiveConditioner
from models.Conditionners.AutoregressiveConditioner import ConditionnalMADE, MADE, made_degrees, made_prefix_plan

NATURAL = [(1, [4]), (2, [8]), (5, [19]), (17, [8]), (17, [40, 33, 19]), (5, [])]
SAMPLED = [(6, [30, 30]), (9, [7, 12]), (12, [20, 20, 20])]
OUT = 2


def _made(nin, hidden, seed=None):
    """a MADE with the natural ordering, or with the sampled ordering of `seed`"""
    if seed is None:
        return MADE(nin, hidden, OUT * nin)
    net = MADE(nin, hidden, OUT * nin, num_masks=seed + 1, random=True)
    for _ in range(seed):
        net.update_masks()                         # the constructor installed seed 0
    return net


CASES = [(nin, hidden, None) for nin, hidden in NATURAL] + [(nin, hidden, s) for nin, hidden in SAMPLED for s in range(3)]
IDS = ["%d-%s-%s" % (nin, "x".join(map(str, hidden)) or "none", "nat" if s is None else "seed%d" % s)
       for nin, hidden, s in CASES]


@pytest.mark.parametrize("nin,hidden,seed", CASES, ids=IDS)
def test_plan_against_degrees_and_masks(nin, hidden, seed):
    net = _made(nin, hidden, seed)
    m, L = net.m, len(hidden)
    if seed is None:
        ref = made_degrees(nin, hidden)
        assert all(np.array_equal(m[k], ref[k]) for k in ref)
    plan = made_prefix_plan(m, nin, OUT * nin)
    assert plan["d"] == nin and plan["out"] == OUT and plan["widths"] == list(hidden)
    var = plan["var_of_step"]
    assert sorted(var.tolist()) == list(range(nin))
    assert all(m[-1][var[t]] == t for t in range(nin))                           # the inverse of m[-1]
    masks = [layer.mask.numpy() for layer in net.masked_layers()]               # [out_features, in_features]
    new_in = [np.zeros(h, dtype=int) for h in hidden]
    for l in range(L):
        order, off = plan["order"][l], plan["off"][l]
        assert sorted(order.tolist()) == list(range(hidden[l])) and off.shape == (nin + 1,)
        assert all(m[l][order[i]] <= m[l][order[i + 1]] for i in range(hidden[l] - 1))
        for t in range(nin + 1):
            assert set(order[:off[t]].tolist()) == {k for k in range(hidden[l]) if m[l][k] < t}
    for t in range(nin):
        for l in range(L if t >= 1 else 0):
            new = plan["order"][l][plan["off"][l][t - 1]:plan["off"][l][t]]
            assert all(m[l][u] == t - 1 for u in new)
            new_in[l][new] += 1
            prefix = var[:t] if l == 0 else plan["order"][l - 1][:plan["off"][l - 1][t]]
            outside = np.ones(masks[l].shape[1], dtype=bool)
            outside[prefix] = False
            assert not masks[l][new][:, outside].any()                           # every non-zero lies inside the prefix
            assert masks[l][new][:, prefix].all()                                # ... and the prefix is not wider than the mask
        prefix = var[:t] if L == 0 else plan["order"][L - 1][:plan["off"][L - 1][t]]
        rows = [c * nin + var[t] for c in range(OUT)]
        outside = np.ones(masks[L].shape[1], dtype=bool)
        outside[prefix] = False
        assert not masks[L][rows][:, outside].any() and masks[L][rows][:, prefix].all()
    for l in range(L):                      # new in exactly one step, or in none if its degree is d - 1
        assert np.array_equal(new_in[l], (m[l] < nin - 1).astype(int))
    if L and nin > 1:
        assert plan["max_new"] == max(int(np.bincount(m[l][m[l] < nin - 1], minlength=1).max()) if (m[l] < nin - 1).any()
                                      else 0 for l in range(L))


def test_non_degree_mask_has_no_plan():
    cond = AutoregressiveConditioner(5, [19], OUT)
    net = cond.masked_autoregressive_net
    assert cond.prefix_plan() is not None and cond.prefix_plan() is cond.prefix_plan()      # cached
    layer = net.masked_layers()[1]
    mask = layer.mask.numpy().T.copy()                         # set_mask takes [in, out]
    i, o = np.argwhere(mask > 0)[0]
    mask[i, o] = 0                                             # still autoregressive, no longer a degree rule
    layer.set_mask(mask)
    assert cond.prefix_plan() is None
    assert ConditionnalMADE(4, 0, [8], 8).prefix_plan() is not None


def test_plan_follows_update_masks_and_keeps_state_dict():
    net = ConditionnalMADE(nin=9, cond_in=0, hidden_sizes=[20, 20], nout=18, num_masks=3, random=True)
    keys = list(net.state_dict().keys())
    seen = []
    for _ in range(3):
        plan = net.prefix_plan()
        assert plan is not None and np.array_equal(net.m[-1][plan["var_of_step"].numpy()], np.arange(9))
        seen.append(plan["var_of_step"].clone())
        net.update_masks()
    assert not all(torch.equal(seen[0], s) for s in seen[1:])                    # another ordering, another plan
    assert list(net.state_dict().keys()) == keys and not any("prefix" in k or "plan" in k for k in keys)


def _affine_inverse(z, h0, h1):
    return (z - h0.clamp(-5., 5.)) / torch.exp(h1.clamp(-5., 2.))


def prefix_schedule_f64(plan, layers, z):
    """the prefix schedule on the plan tables in torch double: layers [(W, b)] in nn.Linear layout, Affine inverse"""
    B, d, out, L = z.shape[0], plan["d"], plan["out"], len(layers) - 1
    var = [int(v) for v in plan["var_of_step"]]
    order = [torch.as_tensor(np.asarray(o), dtype=torch.long) for o in plan["order"]]
    off = [np.asarray(o) for o in plan["off"]]
    x = torch.zeros_like(z)
    acts = [torch.zeros(B, W.shape[0], dtype=z.dtype) for W, _ in layers[:-1]]
    for t in range(d):
        for l in range(L if t >= 1 else 0):
            new = order[l][off[l][t - 1]:off[l][t]]
            below, pre = ((x, torch.as_tensor(var[:t], dtype=torch.long)) if l == 0
                          else (acts[l - 1], order[l - 1][:off[l - 1][t]]))
            W, b = layers[l]
            acts[l][:, new] = torch.relu(below[:, pre] @ W[new][:, pre].t() + b[new])
        below, pre = (x, torch.as_tensor(var[:t], dtype=torch.long)) if L == 0 else (acts[L - 1], order[L - 1][:off[L - 1][t]])
        W, b = layers[L]
        rows = torch.as_tensor([c * d + var[t] for c in range(out)])
        h = below[:, pre] @ W[rows][:, pre].t() + b[rows]
        x[:, var[t]] = _affine_inverse(z[:, var[t]], h[:, 0], h[:, 1])
    return x


def passes_f64(layers, masks, z):
    """d fixed-point passes of plain masked linears (NormalizingFlow.py:98-107, no early exit)"""
    B, d = z.shape
    x = torch.zeros_like(z)
    for _ in range(d):
        a = x
        for li, ((W, b), M) in enumerate(zip(layers, masks)):
            a = F.linear(a, M * W, b)
            if li < len(layers) - 1:
                a = torch.relu(a)
        h = a.view(B, -1, d).permute(0, 2, 1)
        x = _affine_inverse(z, h[:, :, 0], h[:, :, 1])
    return x


@pytest.mark.parametrize("nin,hidden,seed", CASES, ids=IDS)
def test_prefix_schedule_equals_the_passes_in_fp64(nin, hidden, seed):
    torch.manual_seed(7 + nin + len(hidden))
    cond = AutoregressiveConditioner(nin, list(hidden), OUT)
    if seed is not None:
        cond.masked_autoregressive_net = ConditionnalMADE(nin, 0, list(hidden), OUT * nin, num_masks=seed + 1, random=True)
        for _ in range(seed):
            cond.masked_autoregressive_net.update_masks()
    net = cond.masked_autoregressive_net
    layers = [(l.weight.detach().double(), l.bias.detach().double()) for l in net.masked_layers()]
    masks = [l.mask.double() for l in net.masked_layers()]
    plan = made_prefix_plan(net.m, nin, OUT * nin)
    z = .7 * torch.randn(6, nin, dtype=torch.float64)
    x_cols, x_pass = prefix_schedule_f64(plan, layers, z), passes_f64(layers, masks, z)
    err = ((x_cols - x_pass).abs().max() / x_pass.abs().max()).item()
    assert err <= 1e-12, err
