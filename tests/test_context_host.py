"""CPU (-m "not gpu"): the host half of conditional flows (cond_in > 0) -- constructor shapes and state_dict keys of the three
conditioners, the mask of the conditional MADE, the error cases, the two C-ABI symbols of csrc/gnf_group_bias.hip exported,
declared and bound under the unchanged ABI number, their argument checks, and the driver's -context_cols."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnf_group_bias_fwd", "gnf_group_bias_bwd")


def _conds():
    from models import AutoregressiveConditioner, CouplingConditioner, DAGConditioner
    return {"DAG": DAGConditioner, "Coupling": CouplingConditioner, "Autoregressive": AutoregressiveConditioner}


FIRST = {"DAG": "embedding_net.net.0.weight", "Coupling": "embeding_net.net.0.weight",
         "Autoregressive": "masked_autoregressive_net.net.0.weight"}


@pytest.mark.parametrize("kind", ["DAG", "Coupling", "Autoregressive"])
def test_constructor_shapes_and_state_dict_keys(kind):
    T, d, H, out = _conds()[kind], 5, 12, 2
    extra = {"hot_encoding": True} if kind == "DAG" else {}
    torch.manual_seed(0)
    base = T(d, [H, H], out, **extra).state_dict()
    torch.manual_seed(0)
    zero = T(d, [H, H], out, cond_in=0, **extra).state_dict()
    assert list(base) == list(zero)
    for k in base:                                               # cond_in = 0 is today's module, value for value
        assert base[k].shape == zero[k].shape and torch.equal(base[k], zero[k]), k
    in0 = {"DAG": 2 * d, "Coupling": d - d // 2, "Autoregressive": d}[kind]
    assert tuple(base[FIRST[kind]].shape) == (H, in0)
    for c in (1, 3):
        sd = T(d, [H, H], out, cond_in=c, **extra).state_dict()
        assert list(sd) == list(base), (kind, c)
        for k in sd:
            want = (H, in0 + c) if k in (FIRST[kind], FIRST[kind].replace("weight", "mask")) else tuple(base[k].shape)
            assert tuple(sd[k].shape) == want, (kind, c, k)


# (nin, cond_in, hidden, sampled orderings); the reference's sampled hidden degrees need nin >= 2 (randint(0, 0) at nin = 1)
MADE_CASES = [(1, 1, [4], False), (5, 2, [7, 7], False), (4, 3, [], False), (5, 2, [7, 7], True), (4, 3, [], True)]


@pytest.mark.parametrize("nin,c,hidden,random", MADE_CASES,
                         ids=["1-1-4", "5-2-7x7", "4-3-none", "5-2-7x7-random", "4-3-none-random"])
def test_conditional_made_mask(nin, c, hidden, random):
    from models.Conditionners.AutoregressiveConditioner import MADE, ConditionnalMADE
    kw = {"num_masks": 2, "random": True} if random else {}
    net, ref = ConditionnalMADE(nin, c, hidden, 2 * nin, **kw), MADE(nin, hidden, 2 * nin, **kw)
    for _ in range(3 if random else 1):                          # the orderings the two cycle through stay in step
        assert net.nin == nin and net.nout == 2 * nin and net.cond_in == c
        assert all((net.m[k] == ref.m[k]).all() for k in ref.m) and set(net.m) == set(ref.m)
        layers, plain = net.masked_layers(), ref.masked_layers()
        first = layers[0]
        assert tuple(first.weight.shape) == (plain[0].weight.shape[0], c + nin)
        assert bool((first.mask[:, :c] == 1).all())              # every unit (without hidden layers: every output) sees the context
        assert torch.equal(first.mask[:, c:], plain[0].mask)
        assert bool((first.deg_in[:c] == -1).all()) and torch.equal(first.deg_in[c:], plain[0].deg_in)
        assert first.deg_strict == (not hidden)
        for a, b in zip(layers[1:], plain[1:]):
            assert torch.equal(a.mask, b.mask) and torch.equal(a.deg_in, b.deg_in) and torch.equal(a.deg_out, b.deg_out)
        assert all(l.degree_spec() is not None for l in layers)
        assert net.prefix_plan() is None
        net.update_masks()
        ref.update_masks()


def test_error_cases():
    conds = _conds()
    x = torch.zeros(4, 5)
    for kind, T in conds.items():
        cond = T(5, [8], 2, cond_in=2)
        with pytest.raises(ValueError):
            cond(x)
        with pytest.raises(ValueError):
            cond(x, None)
        for bad in (torch.zeros(4, 3), torch.zeros(3, 2), torch.zeros(4, 2, 1), torch.zeros(8)):
            with pytest.raises(ValueError):
                cond(x, bad)
        plain = T(5, [8], 2)
        with pytest.raises(NotImplementedError):                 # cond_in = 0 keeps refusing any context
            plain(x, torch.zeros(4, 2))
    with pytest.raises(NotImplementedError):
        conds["DAG"](5, torch.nn.Linear(5, 2), 2, cond_in=1)
    from models.MLP import MNISTCNN
    with pytest.raises(NotImplementedError):
        conds["DAG"](784, MNISTCNN(), 2, cond_in=3)
    conds["DAG"](5, torch.nn.Linear(5, 2), 2)                    # a module without a context is what it was


def test_symbols_exported_declared_and_bound():
    from gnf_hip import abi, build
    header = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = abi.load()                                             # dlopen works without a GPU
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES, name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(abi.SIGNATURES[name][1]), name
    assert abi.ABI_VERSION == 11 and lib.gnf_abi_version() == 11
    assert "#define GNF_ABI_VERSION 11" in header
    assert "gnf_group_bias.hip" in build.SOURCES


def test_argument_checks_answer_before_any_launch():
    from gnf_hip import abi
    lib = abi.load()
    p = ctypes.c_void_p(64)                                      # never dereferenced: every call below is refused or empty
    assert lib.gnf_group_bias_fwd(p, p, p, 1, 7, 4, 3, None) == -2          # M % G != 0: GNF_ESHAPE
    assert lib.gnf_group_bias_bwd(p, p, p, p, 7, 4, 3, None) == -2
    assert lib.gnf_group_bias_fwd(None, None, None, 1, 0, 4, 3, None) == 0  # M == 0: nothing launched
    assert lib.gnf_group_bias_bwd(None, None, None, None, 0, 4, 3, None) == 0
    for M, H, G in ((-3, 4, 3), (6, 0, 3), (6, 4, 0)):
        assert lib.gnf_group_bias_fwd(p, p, p, 0, M, H, G, None) == -1
        assert lib.gnf_group_bias_bwd(p, p, p, p, M, H, G, None) == -1
    assert lib.gnf_group_bias_fwd(None, p, p, 0, 6, 4, 3, None) == -1
    assert lib.gnf_group_bias_fwd(ctypes.c_void_p(66), p, p, 0, 6, 4, 3, None) == -1     # below dword alignment
    assert lib.gnf_group_bias_bwd(p, p, None, p, 6, 4, 3, None) == -1       # a gate without a g_pre to write
    assert lib.gnf_group_bias_bwd(p, None, None, None, 6, 4, 3, None) == -1


def test_dag_case_draws_are_tie_free_within_the_default_rounds():
    """the fp64 half of tests/test_gpu_context.py's DAG cases alone: every seeded draw is free of tied samples inside
    resample_off_ties' default 8 redraws (it raises otherwise), and the reference sees the context"""
    from context_ref import DAG_GATES, DAG_SHAPES, d64, dag64, dag_case
    for shape in DAG_SHAPES:
        for hot in (True, False):
            for case in DAG_GATES:
                cond, (x, ctx, u1, u2), cot, rounds = dag_case(shape, hot, case)
                assert 0 <= rounds <= 8 and tuple(ctx.shape) == (shape[0], shape[3])
                P = {n: d64(p) for n, p in cond.named_parameters()}
                h = dag64(cond, P, case, x.double(), ctx.double(), u1, u2)
                assert tuple(h.shape) == (shape[0], shape[1], cot.shape[2])
                if shape[2] >= 16:                               # (three hidden layers of TWO units can be dead for every row)
                    assert not torch.equal(h, dag64(cond, P, case, x.double(), ctx.double() + 1., u1, u2))


def test_train_uci_parse_accepts_context_cols():
    import train_uci
    a = train_uci.parse(["-dataset", "power"])
    assert a.context_cols == 0
    a = train_uci.parse(["-dataset", "power", "-context_cols", "2", "-conditioner", "Coupling"])
    assert a.context_cols == 2
    model, _, _ = train_uci.build(a, 4)
    assert tuple(model.state_dict()["steps.0.conditioner.embeding_net.net.0.weight"].shape) == (a.emb_net[0], 2 + 2)
    with pytest.raises(SystemExit):
        train_uci.parse(["-dataset", "power", "-context_cols", "-1"])
    x, ctx = train_uci.split_context(torch.arange(12.).view(2, 6), 2)
    assert torch.equal(x, torch.tensor([[0., 1, 2, 3], [6, 7, 8, 9]])) and torch.equal(ctx, torch.tensor([[4., 5], [10, 11]]))
    rows = torch.zeros(2, 6)
    assert train_uci.split_context(rows, 0) == (rows, None)


def test_steps_are_not_replayable_with_a_context():
    from gnf_hip import dp
    from models import AffineNormalizer, buildFCNormalizingFlow
    for kind, T in _conds().items():
        args = {"in_size": 5, "hidden": [8], "out_size": 2}
        assert dp.steps_replayable(buildFCNormalizingFlow(1, T, dict(args, cond_in=2), AffineNormalizer, {})) is False
    plain = buildFCNormalizingFlow(1, _conds()["Coupling"], {"in_size": 5, "hidden": [8], "out_size": 2}, AffineNormalizer, {})
    assert dp.steps_replayable(plain) is True
