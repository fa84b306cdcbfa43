"""CPU (-m "not gpu"): the host half of the DAGMLP front with the gate fused in -- the new C-ABI symbols are exported,
declared and bound with matching arity under the unchanged ABI number; the planner's answers for the UCI shapes; the
dispatch of DAGMLP / DAGConditioner on CPU tensors; the driver's flag."""
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ("gnf_dagmlp_supported", "gnf_dagmlp_gated_fwd", "gnf_dagmlp_gated_bwd_ws_bytes", "gnf_dagmlp_gated_bwd",
       "gnf_dagmlp_rows_fwd")
# (d, width of the first hidden layer) of POWER, GAS, HEPMASS, MINIBOONE, BSDS300
UCI = ((6, 60), (8, 80), (21, 210), (43, 430), (63, 630))


def test_symbols_exported_declared_and_bound():
    from gnf_hip import abi
    header = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = abi.load()                                            # dlopen works without a GPU
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES, name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(abi.SIGNATURES[name][1]), name
    assert abi.ABI_VERSION == 11 and lib.gnf_abi_version() == 11
    assert "#define GNF_ABI_VERSION 11" in header


def test_planner_domain():
    from gnf_hip import abi, ops
    lib = abi.load()
    for d, H in UCI:
        assert lib.gnf_dagmlp_supported(d, H) == 1 and ops.dagmlp_supported(d, H)
    for d, H in ((1, 1), (64, 1), (3, 2), (64, 1000)):
        assert lib.gnf_dagmlp_supported(d, H) == 1
    for d, H in ((0, 60), (65, 60), (6, 0), (-1, 4), (6, -2)):
        assert lib.gnf_dagmlp_supported(d, H) == 0 and not ops.dagmlp_supported(d, H)


def test_backward_workspace_is_positive_monotone_and_finite():
    from gnf_hip import abi
    lib = abi.load()
    for d, H in UCI + ((1, 16), (3, 2), (64, 7)):
        last = lib.gnf_dagmlp_gated_bwd_ws_bytes(0, d, H)
        assert 0 < last < 1 << 30
        for B in (1, 2, 7, 100, 2500, 10000, 1 << 20):
            cur = lib.gnf_dagmlp_gated_bwd_ws_bytes(B, d, H)
            assert last <= cur < 1 << 30, (B, d, H, last, cur)
            last = cur
    assert lib.gnf_dagmlp_gated_bwd_ws_bytes(4, 65, 10) < 0 and lib.gnf_dagmlp_gated_bwd_ws_bytes(4, 6, 0) < 0


def test_entry_points_refuse_bad_shapes_without_a_device():
    """the argument checks come before any launch: they answer on a machine without a GPU"""
    from gnf_hip import abi
    lib = abi.load()
    args_fwd = lambda d, H: (None, None, None, 1, 1, 0., .5, None, None, 1, 1, None, 2 * d, None, 1, 1, None, 0, d, H, None)
    assert lib.gnf_dagmlp_gated_fwd(*args_fwd(65, 10)) == -2
    assert lib.gnf_dagmlp_gated_fwd(*args_fwd(0, 10)) != 0
    assert lib.gnf_dagmlp_gated_fwd(*args_fwd(6, 0)) != 0
    assert lib.gnf_dagmlp_gated_fwd(*args_fwd(6, 10)) == -1            # NULL A, tab, W1, b1
    assert lib.gnf_dagmlp_rows_fwd(None, None, 65, None, 1, None, 130, None, 1, 1, None, 0, 0, 65, 10, None) == -2
    assert lib.gnf_dagmlp_gated_bwd(None, None, 1, 1, .5, None, None, 1, 1, None, 130, 1, None, None, None, 0, None, 130, None,
                                    None, 0, 0, 65, 10, None) == -2


def test_dispatch_on_cpu_tensors(monkeypatch):
    from gnf_hip import GnfError, ops
    from models import DAGConditioner
    import importlib
    mod = importlib.import_module("models.Conditionners.DAGConditioner")
    from models.Conditionners.DAGConditioner import DAGMLP
    assert mod.DAGMLP_GATED_FRONT_DEFAULT in (True, False)
    torch.manual_seed(0)
    cond = DAGConditioner(6, [60, 60], 30, hot_encoding=True, gumble_T=.5)
    net = cond.embedding_net
    assert isinstance(net, DAGMLP) and net.gated_front == mod.DAGMLP_GATED_FRONT_DEFAULT and net.accepts_hot
    assert "gated_front" not in "".join(cond.state_dict().keys())
    fused = []
    monkeypatch.setattr(ops, "dag_mlp_front", lambda *a, **k: fused.append("front"))
    monkeypatch.setattr(ops, "dag_mlp_rows", lambda *a, **k: fused.append("rows"))
    x = torch.randn(4, 6)
    for on in (True, False):
        net.gated_front = on
        assert not net.supports_gated(x, True) and not net.supports_rows(x, True)
        msgs = []
        for grad in (True, False):                              # stochastic gate, then the deterministic one without autograd
            cond.stoch_gate = grad
            with torch.set_grad_enabled(grad), pytest.raises(GnfError) as err:
                cond(x)                                         # the parent's statements: they need the GPU (no CPU fallback)
            msgs.append(str(err.value))
        assert all("no CPU fallback" in m for m in msgs)
    assert fused == []


def test_driver_accepts_the_flag():
    import train_uci
    args = train_uci.parse(["-dataset", "power", "-gated_front"])
    assert args.gated_front is True
    assert train_uci.parse(["-dataset", "power"]).gated_front is False
    args.conditioner, args.normalizer, args.emb_net, args.nb_flow = "DAG", "affine", [60, 60, 60, 30], 2
    model, _, _ = train_uci.build(args, 6)
    assert all(c.embedding_net.gated_front is True for c in model.getConditioners())
    args.gated_front = False
    model, _, _ = train_uci.build(args, 6)
    from models.Conditionners.DAGConditioner import DAGMLP_GATED_FRONT_DEFAULT
    assert all(c.embedding_net.gated_front == DAGMLP_GATED_FRONT_DEFAULT for c in model.getConditioners())
