"""CPU (-m "not gpu"): the host half of the device graph queries of the DAG conditioner -- the three C-ABI symbols are
exported, declared and bound with matching arity under the unchanged ABI number; the domain of the kernel; the candidate
thresholds of post_process(); and a CPU conditioner answers the same with `device_graph` set as without (its tensors are
not on the GPU, so every call site runs the host statements)."""
import os
import re

import numpy as np
import torch

from conftest import ROOT

NEW = ("gnf_dag_levels_supported", "gnf_dag_levels_ws_bytes", "gnf_dag_levels")


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
    assert "#define GNF_DAG_ELEM_F32 %d" % abi.DAG_ELEM_F32 in header
    assert re.search(r"#define GNF_DAG_ELEM_U8\s+%d" % abi.DAG_ELEM_U8, header)


def test_domain_and_workspace():
    from gnf_hip import abi, ops
    lib = abi.load()
    for d in (1, 64, 4096):
        assert lib.gnf_dag_levels_supported(d) == 1 and ops.dag_levels_supported(d)
    for d in (0, -1, 4097):
        assert lib.gnf_dag_levels_supported(d) == 0 and not ops.dag_levels_supported(d)
        assert lib.gnf_dag_levels_ws_bytes(1, d) == -2
    # the predicate as bits: ceil(d / 64) 64-bit words per row, and one more for the mask of its nonzero words
    assert lib.gnf_dag_levels_ws_bytes(1, 1) == 2 * 8 and lib.gnf_dag_levels_ws_bytes(1, 64) == 2 * 64 * 8
    assert lib.gnf_dag_levels_ws_bytes(3, 65) == 3 * 3 * 65 * 8 and lib.gnf_dag_levels_ws_bytes(19, 3072) == 19 * 49 * 3072 * 8
    assert lib.gnf_dag_levels_ws_bytes(0, 7) == 0 and lib.gnf_dag_levels_ws_bytes(-1, 7) == -1


def test_entry_point_refuses_bad_arguments_without_a_device():
    """the argument checks come before any launch: they answer on a machine without a GPU"""
    from gnf_hip import abi
    lib = abi.load()
    bad = lambda M, et, sg, ld, th, lv, info, ws, nws, G, d: lib.gnf_dag_levels(M, et, sg, ld, th, lv, info, ws, nws, G, d, None)
    assert bad(None, 0, 0, 4097, None, None, None, None, 0, 1, 4097) == -2
    assert bad(None, 0, 0, 0, None, None, None, None, 0, 1, 0) == -2
    assert bad(None, 0, 0, 8, None, None, None, None, 0, 0, 8) == 0                 # G == 0: nothing to do
    assert bad(None, 0, 0, 8, None, None, None, None, 0, -1, 8) == -1
    assert bad(None, 2, 0, 8, None, None, None, None, 0, 0, 8) == -1                # unknown element type
    assert bad(None, 0, 0, 8, None, None, None, None, 0, 1, 8) == -1                # NULL operands
    assert bad(64, 0, 0, 7, None, 64, 64, 64, 1 << 20, 1, 8) == -1                  # ld < d
    assert bad(66, 0, 0, 8, None, 64, 64, 64, 1 << 20, 1, 8) == -1                  # fp32 M below dword alignment
    assert bad(64, 0, 0, 8, 66, 64, 64, 64, 1 << 20, 1, 8) == -1                    # thresholds
    assert bad(64, 0, 0, 8, None, 66, 64, 64, 1 << 20, 1, 8) == -1                  # level
    assert bad(64, 0, 0, 8, None, 64, 66, 64, 1 << 20, 1, 8) == -1                  # info
    assert bad(64, 0, 0, 8, None, 64, 64, 68, 1 << 20, 1, 8) == -1                  # ws at a dword that is no 8-byte address
    assert bad(65, 1, 0, 8, 64, 64, 64, 64, 1 << 20, 1, 8) == -1                    # thresholds with a uint8 matrix
    assert bad(65, 1, 0, 8, None, 64, 64, 64, 127, 1, 8) == -3                      # uint8 M at any byte; ws too small


def test_threshold_candidates_are_the_doubles_of_the_search_loop():
    from models.Conditionners.DAGConditioner import threshold_candidates
    cands = threshold_candidates()
    th, loop = .1, []
    for _ in range(len(cands)):
        loop.append(th)
        th += .05
    assert cands == loop                                        # the same doubles, bit for bit
    assert cands[0] == .1 and cands[1] == .1 + .05 and cands[1] != .15
    assert len(cands) <= 19
    assert all(np.float32(c) < 1 for c in cands[:-1]) and np.float32(cands[-1]) >= 1
    assert threshold_candidates() is not cands                  # a fresh list: a caller may keep it


def _cpu_conditioner(d, seed, cyclic_until=None):
    from models import DAGConditioner
    torch.manual_seed(seed)
    cond = DAGConditioner(d, [8, 8], 4)
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(d, generator=g)
    low = torch.tril(torch.ones(d, d), -1) * (torch.rand(d, d, generator=g) < .3).float()
    A = torch.zeros(d, d)
    A[perm.unsqueeze(1), perm.unsqueeze(0)] = low * (1. + torch.rand(d, d, generator=g))
    if cyclic_until is not None:                                # a weak back edge: cyclic until the threshold passes it
        i, j = (low > 0).nonzero()[0].tolist()
        A[perm[j], perm[i]] = cyclic_until
    with torch.no_grad():
        cond.A.copy_(A)
    return cond


def test_cpu_conditioner_answers_the_same_with_the_switch_set():
    import importlib
    mod = importlib.import_module("models.Conditionners.DAGConditioner")
    assert mod.DEVICE_GRAPH_DEFAULT in (True, False)
    min_d = getattr(mod, "DEVICE_GRAPH_MIN_D", 0)
    for d, weak in ((5, None), (12, None), (12, .3), (40, .45), (70, .45)):
        res = []
        for on in (True, False):
            cond = _cpu_conditioner(d, d, weak)
            assert cond.device_graph == (mod.DEVICE_GRAPH_DEFAULT and d >= min_d)
            assert "device_graph" not in "".join(cond.state_dict().keys())
            cond.device_graph = on
            assert not cond._device_graph()                     # CPU tensors: the host statements
            lv = cond.levels(with_host=True)
            lv = None if lv is None else [(r.tolist(), h) for r, h in lv]
            lp = cond.levels(P=cond.soft_thresholded_A())
            lp = None if lp is None else [r.tolist() for r in lp]
            depth = cond.depth()
            cond.post_process()
            res.append((lv, lp, depth, cond.A.detach().clone(), cond.depth(), [r.tolist() for r in cond.levels()]))
        (lv1, lp1, d1, A1, pd1, pl1), (lv0, lp0, d0, A0, pd0, pl0) = res
        assert lv1 == lv0 and lp1 == lp0 and d1 == d0 and torch.equal(A1, A0) and pd1 == pd0 and pl1 == pl0
        assert (lv0 is None) == (weak is not None)
