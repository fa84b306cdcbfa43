"""CPU (-m "not gpu"): the host half of the device-side epochs of train_uci.py -- the two C-ABI symbols of
csrc/gnf_tab_batch.hip are exported, declared and bound with matching arity under the unchanged ABI number; their argument
checks answer before any launch; dp.batch_slices cuts what train_uci.shard_batches cuts; the key layout of gnf_shuffle_keys,
restated in numpy, sorts into a permutation; the driver's new options."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import uci_ref

NEW = ("gnf_shuffle_keys", "gnf_tab_batch")


def test_symbols_exported_declared_and_bound():
    from gnf_hip import abi, build
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
    assert "gnf_tab_batch.hip" in build.SOURCES


def test_shuffle_keys_refuses_bad_arguments_without_a_device():
    """the argument checks come before any launch: they answer on a machine without a GPU"""
    from gnf_hip import abi
    keys = abi.load().gnf_shuffle_keys
    assert keys(1, 2, 0, None, None) == 0                       # n == 0: nothing to do
    assert keys(1, 2, -1, 64, None) == -1
    assert keys(1, 2, 5, None, None) == -1                      # NULL keys
    assert keys(1, 2, 5, 68, None) == -1                        # a dword that is no 8-byte address
    assert keys(1, 2, 1 << 31, 64, None) == -2                  # the row is the low word's 31 bits


def test_tab_batch_refuses_bad_arguments_without_a_device():
    from gnf_hip import abi
    lib = abi.load()

    def tb(X=64, n_rows=10, d=4, ldx=4, perm=128, n_perm=10, first=0, stride=1, cursor=None, x=256, B=2):
        return lib.gnf_tab_batch(X, n_rows, d, ldx, perm, n_perm, first, stride, cursor, x, B, None)
    assert tb(B=-1) == -1 and tb(d=0) == -1 and tb(ldx=3) == -1 and tb(stride=0) == -1 and tb(first=-1) == -1
    assert tb(X=None, perm=None, x=None, B=0) == 0              # an empty batch: nothing to do, every pointer may be NULL
    assert tb(B=0, d=0) == -1                                   # ... but the shape arguments are still checked
    assert tb(X=None) == -1 and tb(x=None) == -1 and tb(n_rows=0) == -1 and tb(n_perm=0) == -1
    for name in ("X", "x", "perm", "cursor"):                   # below dword alignment
        assert tb(**{name: 66}) == -1, name
    assert tb(B=1 << 29) == -2 and tb(d=1 << 16, ldx=1 << 16, B=1 << 15) == -2      # B*d = 2^31
    # without a cursor the host knows the last position: first + (B-1)*stride < n_perm (n_rows under the identity)
    assert tb(first=9, B=2) == -1 and tb(first=10, B=1) == -1 and tb(first=0, stride=5, B=3) == -1
    assert tb(perm=None, n_perm=0, n_rows=3, first=2, B=2) == -1
    assert tb(stride=1 << 62, B=3) == -1                        # no overflow in the check itself


@pytest.mark.parametrize("world", [1, 2, 3])
def test_batch_slices_cut_what_shard_batches_cuts(world):
    import train_uci
    from gnf_hip import dp
    for n in (1, 7, 40, 44, 1000):
        for b in (1, 8, 100):
            steps = set()
            for rank in range(world):
                want = train_uci.shard_batches(n, b, rank, world, torch.Generator().manual_seed(5))
                p = torch.randperm(n, generator=torch.Generator().manual_seed(5))
                slices = dp.batch_slices(n, b, rank, world)
                got = [p[first::world][:count] for first, count in slices]
                assert len(got) == len(want), (n, b, rank)
                assert all(g.numel() > 0 and torch.equal(g, w) for g, w in zip(got, want)), (n, b, rank)
                steps.add(tuple(c for _, c in slices))
            assert len(steps) == 1, (n, b)                      # every rank: the same number of steps of the same sizes


def test_sorted_keys_are_a_permutation():
    for n in (1, 5, 1000, 4097):
        keys = uci_ref.shuffle_keys(1234, 0, n)
        assert keys.dtype == np.int64 and (keys >= 0).all()
        assert np.array_equal(keys & 0xffffffff, np.arange(n))
        perms = [uci_ref.permutation(1234, e, n) for e in (0, 1)]
        for p in perms:
            assert p.dtype == np.int32 and np.array_equal(np.sort(p), np.arange(n))
        if n > 5:
            assert not np.array_equal(perms[0], perms[1])       # another epoch, another order
            assert not np.array_equal(perms[0], np.arange(n))
            assert not np.array_equal(perms[0], uci_ref.permutation(1235, 0, n))
    assert uci_ref.shuffle_keys(0, 0, 0).shape == (0,)
    # the offset's high word reaches the counter
    assert not np.array_equal(uci_ref.permutation(7, 1, 1000), uci_ref.permutation(7, 1 + (1 << 32), 1000))


def test_groups_of_steps_are_refused_for_monotonic_and_stochastic_gate_flows():
    from gnf_hip import dp
    from models import (buildFCNormalizingFlow, CouplingConditioner, DAGConditioner, AffineNormalizer, MonotonicNormalizer)
    aff = buildFCNormalizingFlow(1, CouplingConditioner, {"in_size": 6, "hidden": [16], "out_size": 2}, AffineNormalizer, {})
    assert dp.steps_replayable(aff)
    mono = buildFCNormalizingFlow(1, CouplingConditioner, {"in_size": 6, "hidden": [16], "out_size": 4}, MonotonicNormalizer,
                                  {"integrand_net": [16, 16], "cond_size": 4, "nb_steps": 10, "solver": "CC"})
    assert dp.GraphedStep.graphable(mono) and not dp.steps_replayable(mono)      # the drivers jitter nb_steps per batch
    dag = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": 6, "hidden": [16], "out_size": 2, "l1": .1}, AffineNormalizer, {})
    assert not dp.GraphedStep.graphable(dag) and not dp.steps_replayable(dag)    # stochastic gate: noise from a host counter
    with torch.no_grad():
        assert not dp.steps_replayable(aff)                                      # nothing to train


def test_driver_options():
    import train_uci
    args = train_uci.parse(["-dataset", "power"])
    assert (args.device_batches, args.seed, args.steps_per_replay, args.threshold_sweep) == (False, 0, 1, False)
    args = train_uci.parse(["-dataset", "power", "-device_batches", "-seed", "9", "-steps_per_replay", "4",
                            "-threshold_sweep"])
    assert (args.device_batches, args.seed, args.steps_per_replay, args.threshold_sweep) == (True, 9, 4, True)
    for bad in (["-steps_per_replay", "4"], ["-device_batches", "-steps_per_replay", "0"]):
        with pytest.raises(SystemExit):
            train_uci.parse(["-dataset", "power"] + bad)
    assert train_uci.THRESHOLDS == (.95, .5, .1, .01, .0001)
