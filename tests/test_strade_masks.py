"""CPU: the StrADE mask rule, its level plan and its state_dict, in numpy and on modules that never see a GPU.

The dependency law is checked on the masks themselves (a boolean product, both directions), the level plan by evaluating
the net level by level in fp64 numpy on an image built as the pack kernel builds it, against the dense masked net."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from models import StrADEConditioner
from models.Conditionners.StrADEConditioner import strade_level_plan, strade_masks, strade_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = [1, 2, 5, 17, 64]
DENSITIES = [0., .2, .5, "full"]


def random_dag(d, density, seed):
    """adjacency[i][j] = 1: j is a parent of i.  A strictly lower-triangular Bernoulli pattern ("full": all of it) under a
    random relabelling of the variables, so the topological order is not the index order"""
    rng = np.random.RandomState(seed)
    low = np.tril(np.ones((d, d)) if density == "full" else rng.rand(d, d) < density, -1).astype(np.uint8)
    perm = rng.permutation(d)
    a = np.zeros((d, d), dtype=np.uint8)
    a[np.ix_(perm, perm)] = low
    return a


def hidden_sets(a, cond_in):
    """the hidden layouts of the issue for this graph: [], [R], [2R + 3], [R, R + 5] (a graph without any parent set still
    gets one unit per layer: a zero-width Linear is no net)"""
    R = max(strade_sets(a, cond_in)[1], 1)
    return [[], [R], [2 * R + 3], [R, R + 5]]


# ------------------------------------------------------------------------------------------------ 1. the dependency law
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("d", DS)
def test_outputs_reach_exactly_their_parents(d, density):
    a = random_dag(d, density, 7 * d + 1)
    for cond_in in (0, 3):
        for hidden in hidden_sets(a, cond_in):
            for out in (1, 2, 23):
                masks = strade_masks(a, hidden, out, cond_in)
                sizes = [cond_in + d] + hidden + [out * d]
                assert [m.shape for m in masks] == [(o, i) for i, o in zip(sizes, sizes[1:])]
                assert all(m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1} for m in masks)
                reach = masks[0].astype(np.int64)
                for m in masks[1:]:
                    reach = (m.astype(np.int64) @ reach > 0).astype(np.int64)
                reach = reach if hidden else masks[0]
                # nothing forbidden and nothing lost: the reachable variables ARE the parents, for every component
                assert np.array_equal(reach[:, cond_in:] > 0, np.tile(a, (out, 1)) > 0), (d, density, hidden, out, cond_in)
                # the context reaches every output, the roots' included
                assert (reach[:, :cond_in] > 0).all(), (d, density, hidden, out, cond_in)


def test_the_rule_is_deterministic_and_none_is_the_lower_triangle():
    a = random_dag(17, .2, 3)
    m1, m2 = strade_masks(a, [40, 24], 2, 3), strade_masks(torch.from_numpy(a), [40, 24], 2, 3)
    assert all(np.array_equal(x, y) for x, y in zip(m1, m2))
    c = StrADEConditioner(5, [9], 2)
    assert np.array_equal(c.adjacency.numpy(), np.tril(np.ones((5, 5), dtype=np.uint8), -1))
    assert c.adjacency.dtype == torch.uint8 and "adjacency" in c.state_dict() and c.depth() == 4 and c.is_invertible


# ------------------------------------------------------------------------------------------------ 2. errors
def test_bad_graphs_and_narrow_layers_are_refused():
    two = np.array([[0, 1], [1, 0]])
    with pytest.raises(ValueError, match="cycle through node"):
        strade_masks(two, [4], 2)
    with pytest.raises(ValueError, match="node 1 is its own parent"):
        strade_masks(np.array([[0, 0], [1, 1]]), [4], 2)
    with pytest.raises(ValueError, match=r"\(3, 4\)"):
        strade_masks(np.zeros((3, 4)), [4], 2)
    with pytest.raises(ValueError, match="other than 0/1"):
        strade_masks(np.array([[0, 0], [2, 0]]), [4], 2)
    a = random_dag(17, .5, 5)
    R = strade_sets(a, 0)[1]
    assert R >= 2
    with pytest.raises(ValueError, match="hidden width of %d is below the %d" % (R - 1, R)):
        strade_masks(a, [R, R - 1], 2)
    strade_masks(a, [R, R], 2)
    for bad in (two, np.zeros((3, 4)), np.zeros((4, 4))):
        with pytest.raises(ValueError):
            StrADEConditioner(2, [4], 2, adjacency=bad)
    with pytest.raises(ValueError, match="cycle"):
        strade_masks(np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]]), [], 2)


# ------------------------------------------------------------------------------------------------ 3. the level plan
def _image(Ws, bs, masks, plan, c):
    """mask o W and the biases in level order, as strade_pack_k writes them (without the pitch padding)"""
    nh, d, out = len(plan["widths"]), plan["d"], plan["out"]
    var = plan["var_order"]
    col0 = np.concatenate([np.arange(c), c + var])
    Wp, bp = [], []
    for l in range(nh + 1):
        rows = plan["order"][l] if l < nh else np.array([k * d + var[p] for p in range(d) for k in range(out)])
        cols = col0 if l == 0 else plan["order"][l - 1]
        Wp.append((Ws[l] * masks[l])[np.ix_(rows, cols)])
        bp.append(bs[l][rows])
    return Wp, bp


def _sweep(Wp, bp, plan, c, z, ctx, pin=None, xpin=None):
    """the level sweep of gnf_strade_levels in fp64 (the Affine inverse with its clamps): -> (x, h [B, d, out] as every variable saw it)"""
    nh, d, out, nlev = len(plan["widths"]), plan["d"], plan["out"], plan["nlev"]
    var, voff, off = plan["var_order"], plan["var_off"], plan["off"]
    B = z.shape[0]
    xs = np.zeros((B, d))                    # x in level order
    hid = [np.full((B, w), np.nan) for w in plan["widths"]]
    x, h = np.zeros((B, d)), np.zeros((B, d, out))
    for t in range(nlev):
        p0, p1 = voff[t], voff[t + 1]
        below = np.concatenate([ctx, xs[:, :p0]], 1)
        for l in range(nh):
            n0, n1 = (off[l][t - 1] if t else 0), off[l][t]
            K = c + p0 if l == 0 else off[l - 1][t]
            src = below if l == 0 else hid[l - 1]
            hid[l][:, n0:n1] = np.maximum(src[:, :K] @ Wp[l][n0:n1, :K].T + bp[l][n0:n1], 0.)
        K = c + p0 if nh == 0 else off[nh - 1][t]
        src = below if nh == 0 else hid[nh - 1]
        o = src[:, :K] @ Wp[nh][p0 * out:p1 * out, :K].T + bp[nh][p0 * out:p1 * out]
        assert not np.isnan(o).any()                     # nothing inside a prefix is read before it is written
        for p in range(p0, p1):
            v, hv = var[p], o[:, (p - p0) * out:(p - p0 + 1) * out]
            h[:, v] = hv
            if pin is not None and pin[v]:
                xs[:, p] = xpin[:, v]
            else:
                xs[:, p] = (z[:, v] - np.clip(hv[:, 0], -5., 5.)) / np.exp(np.clip(hv[:, min(1, out - 1)], -5., 2.))
            x[:, v] = xs[:, p]
    return x, h


def _dense(Ws, bs, masks, x, ctx, d):
    a = np.concatenate([ctx, x], 1)
    for l, (W, b, m) in enumerate(zip(Ws, bs, masks)):
        a = a @ (W * m).T + b
        if l < len(Ws) - 1:
            a = np.maximum(a, 0.)
    return a.reshape(x.shape[0], -1, d).transpose(0, 2, 1)


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("d", DS)
def test_level_sweep_equals_the_dense_net_in_fp64(d, density):
    a = random_dag(d, density, 11 * d + 2)
    rng = np.random.RandomState(d)
    B = 3
    for cond_in in (0, 3):
        for hidden in hidden_sets(a, cond_in):
            for out in (1, 2, 23):
                masks = strade_masks(a, hidden, out, cond_in)
                plan = strade_level_plan(a, hidden, out, cond_in)
                Ws = [rng.randn(*m.shape) / np.sqrt(m.shape[1]) for m in masks]
                bs = [rng.randn(m.shape[0]) * .3 for m in masks]
                z, ctx = rng.randn(B, d), rng.randn(B, cond_in)
                Wp, bp = _image(Ws, bs, masks, plan, cond_in)
                for pin in (None, np.arange(d) % 2 == 1):
                    xpin = rng.randn(B, d)
                    x, h = _sweep(Wp, bp, plan, cond_in, z, ctx, pin, xpin)
                    want = _dense(Ws, bs, masks, x, ctx, d)
                    assert np.abs(h - want).max() <= 1e-12 * max(np.abs(want).max(), 1.), (d, density, hidden, out, cond_in)
                    if pin is not None:
                        assert np.array_equal(x[:, pin], xpin[:, pin])


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("d", DS)
def test_plan_tables(d, density):
    a = random_dag(d, density, 5 * d + 3)
    R = max(strade_sets(a, 3)[1], 1)
    plan = strade_level_plan(a, [R, R + 5], 2, 3)
    level = plan["level"]
    for i in range(d):
        pa = np.flatnonzero(a[i])
        assert level[i] == (0 if pa.size == 0 else 1 + level[pa].max())
    assert plan["nlev"] == level.max() + 1 and plan["var_off"][0] == 0 and plan["var_off"][-1] == d
    assert sorted(plan["var_order"]) == list(range(d)) and (np.diff(level[plan["var_order"]]) >= 0).all()
    assert plan["widest"] == np.bincount(level).max()
    for l, w in enumerate(plan["widths"]):
        assert sorted(plan["order"][l]) == list(range(w)) and plan["off"][l][-1] == w and (np.diff(plan["off"][l]) >= 0).all()
        assert plan["max_new"] >= int(np.diff(np.concatenate([[0], plan["off"][l][:-1]])).max())


# ------------------------------------------------------------------------------------------------ 4. the state dict
def test_state_dict_round_trip_and_a_loaded_graph():
    a, b = random_dag(17, .2, 1), random_dag(17, .5, 2)
    hidden = [40, 24]
    src, dst = StrADEConditioner(17, hidden, 2, cond_in=3, adjacency=a), StrADEConditioner(17, hidden, 2, cond_in=3, adjacency=b)
    sd = src.state_dict()
    keys = {"adjacency"} | {"masked_autoregressive_net.net.%d.%s" % (n, k) for n in (0, 2, 4) for k in ("weight", "bias", "mask")}
    assert set(sd) == keys
    assert not np.array_equal(dst.level_plan()["level"], src.level_plan()["level"])
    dst.load_state_dict(sd)
    assert all(torch.equal(v, dst.state_dict()[k]) for k, v in sd.items())
    # masks, depth and plan follow the LOADED adjacency
    want = strade_masks(a, hidden, 2, 3)
    assert all(np.array_equal(l.mask.numpy(), m.astype(np.float32)) for l, m in zip(dst._layers(), want))
    plan, ref = dst.level_plan(), strade_level_plan(a, hidden, 2, 3)
    assert plan is not None and np.array_equal(plan["level"], ref["level"]) and dst.depth() == ref["nlev"] - 1
    assert np.array_equal(plan["var_order"].numpy(), ref["var_order"])
    assert all(np.array_equal(p.numpy(), r) for p, r in zip(plan["off"], ref["off"]))
    assert dst.level_plan() is plan                                         # cached
    # a hand-edited mask: no level plan, the passes serve
    m = dst._layers()[1].mask
    i, j = [int(v) for v in (m == 0).nonzero()[0]]
    m[i, j] = 1.
    assert dst.level_plan() is None
    m[i, j] = 0.
    assert dst.level_plan() is not None


def test_factory_takes_the_name():
    from models import AffineNormalizer, buildFCNormalizingFlow
    a = random_dag(5, .5, 4)
    flow = buildFCNormalizingFlow(1, "StrADE", {"in_size": 5, "hidden": [8], "out_size": 2, "adjacency": a}, AffineNormalizer, {})
    cond = flow.getConditioners()[0]
    assert type(cond) is StrADEConditioner and np.array_equal(cond.adjacency.numpy(), a) and flow.isInvertible()


def test_uci_driver_takes_a_graph_file_and_a_dag_checkpoint(tmp_path, capsys):
    import train_uci
    from models import AffineNormalizer, DAGConditioner, buildFCNormalizingFlow
    d = train_uci.DIMS["power"]
    a = random_dag(d, .5, 9)
    np.save(str(tmp_path / "graph.npy"), a)
    base = ["-dataset", "power", "-conditioner", "StrADE", "-emb_net", "16", "16", "2"]
    model, cond_t, _ = train_uci.build(train_uci.parse(base + ["-adjacency", str(tmp_path / "graph.npy")]), d)
    assert cond_t is StrADEConditioner and np.array_equal(model.getConditioners()[0].adjacency.numpy(), a)
    none, _, _ = train_uci.build(train_uci.parse(base), d)
    assert np.array_equal(none.getConditioners()[0].adjacency.numpy(), np.tril(np.ones((d, d), dtype=np.uint8), -1))
    # a checkpoint of a one-step DAG flow, saved after post_process()
    torch.manual_seed(0)
    dag = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": d, "hidden": [8], "out_size": 2}, AffineNormalizer, {})
    cond = dag.getConditioners()[0]
    with torch.no_grad():
        cond.A.copy_(torch.from_numpy(a).float() * 3.)
    cond.post_process(zero_threshold=.1)
    torch.save(dag.state_dict(), str(tmp_path / "model.pt"))
    model, _, _ = train_uci.build(train_uci.parse(base + ["-adjacency", str(tmp_path / "model.pt")]), d)
    assert np.array_equal(model.getConditioners()[0].adjacency.numpy(), a)
    for bad, why in ((base + ["-nb_flow", "2"], "ONE-step"),
                     (["-dataset", "power", "-adjacency", str(tmp_path / "graph.npy")], "-conditioner StrADE")):
        with pytest.raises(SystemExit):
            train_uci.parse(bad)
        assert why in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ 5. the ABI
NAMES = {"gnf_strade_pack_floats": 2, "gnf_strade_pack": 4, "gnf_strade_levels": 12}


def test_symbols_exported_declared_and_bound():
    from gnf_hip import abi
    header = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    assert "#define GNF_STRADE_CHUNK_VARS %d\n" % abi.STRADE_CHUNK_VARS in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = abi.load()                                             # dlopen works without a GPU
    for name, nargs in NAMES.items():
        assert hasattr(lib, name) and name in abi.SIGNATURES
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m is not None
        assert len([s for s in m.group(1).split(",") if s.strip()]) == len(abi.SIGNATURES[name][1]) == nargs
    assert not re.search(r"\bgnf_strade\w*_ws_bytes\b", header)   # the sweep takes no workspace
    assert ctypes.sizeof(abi.StradeNet) == ctypes.sizeof(abi.MadeNet) + 8 * (abi.MADE_MAX_HIDDEN + 1) + 8 + 8


def _host_net(d, hidden, out, nlev, widest):
    from gnf_hip import abi
    net = abi.StradeNet()
    net.made.nh, net.made.d, net.made.out, net.made.max_new = len(hidden), d, out, 1
    for l, w in enumerate(hidden):
        net.made.width[l] = w
    net.nlev, net.widest = nlev, widest
    return net


def test_argument_checks_answer_before_any_launch():
    from gnf_hip import abi
    lib = abi.load()
    p = ctypes.c_void_p(64)                                      # never dereferenced: every call below is refused or empty
    net = _host_net(5, [7, 7], 2, 3, 2)
    ref = ctypes.byref(net)
    levels = lambda net_ref, c, ctx, mode, bins, tail, B: lib.gnf_strade_levels(net_ref, c, ctx, p, p, p, mode, bins, tail,
                                                                              None, B, None)
    assert lib.gnf_strade_pack_floats(ref, 0) == 7 * 16 + 8 + 7 * 16 + 8 + 10 * 16 + 12
    assert lib.gnf_strade_pack_floats(ref, -1) == -1 and lib.gnf_strade_pack_floats(None, 0) == -1
    assert levels(ref, 0, None, abi.MADE_NORM_AFFINE, 0, 0., 0) == 0                   # an empty batch launches nothing
    assert levels(ref, 0, None, abi.MADE_NORM_NONE, 0, 0., 0) == -1                    # no such mode here
    assert levels(ref, 0, None, abi.MADE_NORM_AFFINE, 0, 0., -1) == -1
    assert levels(ref, 0, None, abi.MADE_NORM_SPLINE, 1, 3., 0) == -1                  # bins
    assert levels(ref, 0, None, abi.MADE_NORM_SPLINE, 8, 3., 0) == -2                  # out < 3 K - 1
    assert levels(ref, 3, None, abi.MADE_NORM_AFFINE, 0, 0., 4) == -1                  # rows, a context width, no context
    assert levels(ref, 0, None, abi.MADE_NORM_AFFINE, 0, 0., 4) == -1                  # NULL tables
    for nlev, widest in ((0, 2), (6, 2), (3, 0), (3, 6)):
        assert levels(ctypes.byref(_host_net(5, [7, 7], 2, nlev, widest)), 0, None, abi.MADE_NORM_AFFINE, 0, 0., 0) == -1
    one = _host_net(1, [], 1, 1, 1)
    assert levels(ctypes.byref(one), 0, None, abi.MADE_NORM_AFFINE, 0, 0., 0) == -2    # Affine reads two outputs
    wide = _host_net(5, [12000], 2, 3, 2)                                              # 4 rows of 12005 floats: beyond LDS
    assert levels(ctypes.byref(wide), 0, None, abi.MADE_NORM_AFFINE, 0, 0., 4) == -2
    assert lib.gnf_strade_pack(ref, 0, None, None) == -1 and lib.gnf_strade_pack(ref, 0, ctypes.c_void_p(68), None) == -1
    assert lib.gnf_strade_pack(ref, 0, p, None) == -1                                  # NULL parameters
