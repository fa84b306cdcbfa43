"""CPU (-m "not gpu"): the host half of the interventional likelihood log p(x | do(x_S)).

The four C-ABI symbols of csrc/gnf_do_terms.hip exported, declared and bound with matching arity under the unchanged ABI number;
their argument checks, which answer before any launch; `do_targets` -- every accepted form of the targets and every ValueError;
the flow-level refusals of log_prob_do / loss_do; the -regimes option of the UCI driver (refusals, the synthetic regimes, the
validation of a data set's table)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gnf_nll_do_fwd": 10, "gnf_nll_do_bwd": 13, "gnf_affine_do_fwd": 15, "gnf_affine_do_bwd": 20}


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_symbols_exported_declared_and_bound():
    from gnf_hip import abi, build
    header = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    assert "gnf_nll_do_* and gnf_affine_do_* were ADDED under this number" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = abi.load()                                             # dlopen works without a GPU
    for name, arity in NAMES.items():
        assert hasattr(lib, name) and name in abi.SIGNATURES, name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(abi.SIGNATURES[name][1]) == arity, name
    assert abi.ABI_VERSION == 11 and lib.gnf_abi_version() == 11
    assert "#define GNF_ABI_VERSION 11" in header
    assert "gnf_do_terms.hip" in build.SOURCES
    assert not re.search(r"\bgnf_(nll|affine)_do\w*_ws_bytes\b", header)         # no workspace: nothing to poison


def test_argument_checks_answer_before_any_launch():
    from gnf_hip import abi
    lib = abi.load()
    p = ctypes.c_void_p(64)                                      # never dereferenced: every call below is refused or empty
    EINVAL = -1

    def nll_fwd(B, d, pin, regime, R, z=p):
        return lib.gnf_nll_do_fwd(z, p, pin, regime, R, p, p, B, d, None)

    def nll_bwd(B, d, pin, regime, R, z=p):
        return lib.gnf_nll_do_bwd(z, p, pin, regime, R, p, p, None, p, p, B, d, None)

    def aff_fwd(B, d, pin, regime, R, x=p):
        return lib.gnf_affine_do_fwd(x, p, 2 * d, 2, 1, pin, regime, R, p, None, p, p, B, d, None)

    def aff_bwd(B, d, pin, regime, R, x=p):
        return lib.gnf_affine_do_bwd(x, p, 2 * d, 2, 1, pin, regime, R, None, None, p, p, p, p, 2 * d, 2, 1, B, d, None)

    for fn in (nll_fwd, nll_bwd, aff_fwd, aff_bwd):
        assert fn(0, 5, p, None, 1) == 0                         # B == 0 ...
        assert fn(0, 5, None, None, 7, None) == 0                # ... before any pointer or the table is looked at
        assert fn(4, 0, p, None, 1) == EINVAL                    # d == 0
        assert fn(-1, 5, p, None, 1) == EINVAL
        assert fn(4, 5, None, None, 1) == EINVAL                 # pin == NULL: the unmasked entry points exist
        assert fn(4, 5, None, p, 3) == EINVAL
        for R in (0, 2, 3, 5, -1):                               # regime == NULL: R is 1 or B
            assert fn(4, 5, p, None, R) == EINVAL, R
        assert fn(4, 5, p, p, 0) == EINVAL                       # an empty table has no row for anybody
        assert fn(4, 5, p, None, 1, None) == EINVAL              # null data array, B > 0
        assert fn(4, 5, p, None, 4, None) == EINVAL
        assert fn(4, 5, p, p, 3, None) == EINVAL


# ------------------------------------------------------------------------------------------------------------- do_targets
def test_do_targets_accepted_forms():
    from models.NormalizingFlow import do_targets
    B, d = 4, 5
    x = torch.zeros(B, d)
    want = torch.tensor([[0, 1, 0, 1, 0]], dtype=torch.uint8)
    for targets in ([1, 3], (3, 1), torch.tensor([1, 3]), torch.tensor([3, 1], dtype=torch.int32), range(1, 4, 2),
                    torch.tensor([False, True, False, True, False]), torch.tensor([0, 7, 0, 1, 0], dtype=torch.uint8)):
        pin, reg = do_targets(targets, None, x)
        # (non-zero = pinned: a uint8 mask already in place is handed on as it is, the kernels read any non-zero byte as 1)
        assert reg is None and pin.dtype == torch.uint8 and pin.is_contiguous() and torch.equal(pin != 0, want != 0), targets
    for empty in ([], (), torch.zeros(0, dtype=torch.long), torch.zeros(d, dtype=torch.bool)):
        pin, reg = do_targets(empty, None, x)
        assert reg is None and torch.equal(pin, torch.zeros(1, d, dtype=torch.uint8))
    # [R, d] with a regime vector: any integer dtype in, int32 out; a non-contiguous table comes back contiguous
    table = torch.tensor([[0, 0, 0, 0, 0], [1, 0, 0, 0, 2], [1, 1, 1, 1, 1]], dtype=torch.uint8)
    for dtype in (torch.int64, torch.int32, torch.int16, torch.uint8):
        regime = torch.tensor([2, 0, 0, 1]).to(dtype)
        pin, reg = do_targets(table, regime, x)
        assert torch.equal(pin != 0, table != 0) and pin.dtype == torch.uint8 and pin.shape == table.shape
        assert reg.dtype == torch.int32 and reg.is_contiguous() and reg.tolist() == [2, 0, 0, 1]
    wide = torch.zeros(3, 2 * d, dtype=torch.bool)
    wide[1, 0] = wide[2, 4] = True
    pin, reg = do_targets(wide[:, ::2], torch.tensor([1, 1, 2, 0]), x)
    assert pin.is_contiguous() and pin.tolist() == [[0] * 5, [1, 0, 0, 0, 0], [0, 0, 1, 0, 0]]
    # [B, d] without a regime: a row per sample
    per_row = torch.rand(B, d, generator=torch.Generator().manual_seed(0)) < .5
    pin, reg = do_targets(per_row, None, x)
    assert reg is None and torch.equal(pin, per_row.to(torch.uint8))
    # an unchecked regime passes through: the kernels' NaN rule is the backstop
    pin, reg = do_targets(table, torch.tensor([3, -1, 0, 1]), x, check_regime=False)
    assert reg.tolist() == [3, -1, 0, 1]
    # an empty batch has nothing to check
    pin, reg = do_targets(table, torch.zeros(0, dtype=torch.long), torch.zeros(0, d))
    assert reg.numel() == 0 and pin.shape == (3, d)


def test_do_targets_errors():
    from models.NormalizingFlow import do_targets
    B, d = 4, 5
    x = torch.zeros(B, d)
    table = torch.zeros(3, d, dtype=torch.bool)
    ok_regime = torch.tensor([0, 1, 2, 0])
    bad_targets = ([1, 1], [d], [-1], [1.5], [True], "ab", 3, None, torch.tensor([1., 2.]), torch.tensor([[1, 2]]),
                   torch.tensor(1), torch.zeros(d + 1, dtype=torch.bool), torch.zeros(d - 1, dtype=torch.uint8),
                   torch.zeros(3, d, dtype=torch.bool),             # [R, d] without a regime, R neither 1 nor B
                   torch.zeros(B, d + 1, dtype=torch.bool), torch.zeros(2, B, d, dtype=torch.bool),
                   torch.zeros(B, d), torch.zeros(B, d, dtype=torch.int64))
    for t in bad_targets:
        with pytest.raises(ValueError):
            do_targets(t, None, x)
    for t in ([1, 3], torch.tensor([1, 3]), torch.zeros(d, dtype=torch.bool)):   # a regime without an [R, d] table
        with pytest.raises(ValueError, match="regime"):
            do_targets(t, ok_regime, x)
    for r in (torch.tensor([0, 1, 3, 0]), torch.tensor([0, -1, 2, 0])):           # an id outside [0, R)
        with pytest.raises(ValueError, match="regime ids span"):
            do_targets(table, r, x)
    for r in (torch.tensor([0, 1, 2]), torch.tensor([[0, 1, 2, 0]]), torch.tensor([0., 1., 2., 0.]),
              torch.tensor([True, False, True, False]), [0, 1, 2, 0]):
        with pytest.raises(ValueError, match="regime must be"):
            do_targets(table, r, x)
    with pytest.raises(ValueError):
        do_targets([1], None, torch.zeros(d))


# ------------------------------------------------------------------------------------------------------------ the refusals
def test_flow_level_refusals():
    from models import AffineNormalizer, AutoregressiveConditioner, buildFCNormalizingFlow
    from models.NormalizingFlow import CNNormalizingFlow
    from models.NormalizingFlowFactories import NormalLogDensity
    x = torch.zeros(3, 5)
    cargs = {"in_size": 5, "hidden": [8], "out_size": 2}
    two = buildFCNormalizingFlow(2, AutoregressiveConditioner, cargs, AffineNormalizer, {})
    for call in (two.log_prob_do, two.loss_do):
        with pytest.raises(ValueError, match="ONE-step"):
            call(x, [1])
    cn = CNNormalizingFlow([], NormalLogDensity(), [])
    for call in (cn.log_prob_do, cn.loss_do):
        with pytest.raises(ValueError, match="ONE-step.*multi-scale"):
            call(x, [1])

    class Tempered(NormalLogDensity):                            # inherits the marker, overrides forward: not the fold's density
        def forward(self, z):
            return super().forward(z) * .5

    class Joint(torch.nn.Module):
        def forward(self, z):
            return -z.pow(2).sum(1)
    one = buildFCNormalizingFlow(1, AutoregressiveConditioner, cargs, AffineNormalizer, {})
    for dens in (Tempered(), Joint()):
        one.z_log_density = dens
        for call in (one.log_prob_do, one.loss_do):
            with pytest.raises(ValueError, match="standard normal"):
                call(x, [1])
    # the argument errors of do_targets come before any kernel is asked (these tensors are on the host: a launch would raise
    # GnfError, not ValueError)
    one.z_log_density = NormalLogDensity()
    for call in (one.log_prob_do, one.loss_do, one.steps[0].forward_do):
        with pytest.raises(ValueError):
            call(x, [5])
        with pytest.raises(ValueError, match="regime"):
            call(x, [1], torch.tensor([0, 0, 0]))


def test_dp_refuses_a_regime_without_a_table():
    from gnf_hip import dp
    with pytest.raises(ValueError, match="table of targets"):
        dp.accumulate(None, torch.zeros(2, 3), regime=torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError, match="table of targets"):
        dp.train_step(None, None, torch.zeros(2, 3), regime=torch.zeros(2, dtype=torch.long))


# -------------------------------------------------------------------------------------------------------------- the driver
def test_driver_regimes_option():
    import train_uci
    assert train_uci.parse(["-dataset", "power", "-regimes"]).regimes is True
    assert train_uci.parse(["-dataset", "power"]).regimes is False
    for extra in (["-device_batches"], ["-device_batches", "-steps_per_replay", "4"], ["-nb_flow", "2"]):
        with pytest.raises(SystemExit):
            train_uci.parse(["-dataset", "power", "-regimes"] + extra)
    train_uci.parse(["-dataset", "power", "-device_batches", "-steps_per_replay", "4", "-nb_flow", "2"])   # fine without


def test_driver_regime_refusals_say_why(capsys):
    import train_uci
    for extra, why in ((["-device_batches"], "gather"), (["-device_batches", "-steps_per_replay", "4"], "gather"),
                       (["-nb_flow", "2"], "ONE-step")):
        with pytest.raises(SystemExit):
            train_uci.parse(["-dataset", "power", "-regimes"] + extra)
        assert why in capsys.readouterr().err


def test_driver_synthetic_regimes_and_validation(tmp_path):
    import numpy as np
    import train_uci
    d = train_uci.DIMS["power"]
    splits = train_uci.load_split("synthetic", "power")
    plain = [s.clone() for s in splits]
    splits, targets, regimes = train_uci.load_regimes("synthetic", "power", splits)
    targets, regimes = train_uci.validate_regimes(targets, regimes, splits, d)
    assert targets.dtype == torch.uint8 and targets.shape == (d + 1, d)
    assert int(targets[0].sum()) == 0 and torch.equal(targets[1:], torch.eye(d, dtype=torch.uint8))
    for X, X0, r in zip(splits, plain, regimes):
        assert r.dtype == torch.int64 and torch.equal(r, torch.arange(X.shape[0]) % (d + 1))
        pinned = targets[r].bool()
        assert torch.equal(X[~pinned], X0[~pinned])                            # only the targets are overwritten ...
        assert float((X[pinned] - 2.).abs().max()) < .6                        # ... by 2 + 0.1 randn
    # a data file: the arrays are demanded and validated once
    arrays = {k: s.numpy() for k, s in zip(("trn", "val", "tst"), plain)}
    path = str(tmp_path / "plain.npz")
    np.savez(path, **arrays)
    with pytest.raises(ValueError, match="targets, trn_regime"):
        train_uci.load_regimes(path, "power", plain)
    full = dict(arrays, targets=targets.numpy(), **{k + "_regime": r.numpy() for k, r in zip(("trn", "val", "tst"), regimes)})
    path = str(tmp_path / "full.npz")
    np.savez(path, **full)
    _, t2, r2 = train_uci.load_regimes(path, "power", plain)
    t2, r2 = train_uci.validate_regimes(t2, r2, plain, d)
    assert torch.equal(t2, targets) and all(torch.equal(a, b) for a, b in zip(r2, regimes))
    for bad_t in (targets[:, :-1], targets.float(), targets[0]):
        with pytest.raises(ValueError, match="targets must be"):
            train_uci.validate_regimes(bad_t, regimes, plain, d)
    short = [regimes[0][:-1], regimes[1], regimes[2]]
    with pytest.raises(ValueError, match="trn_regime must be"):
        train_uci.validate_regimes(targets, short, plain, d)
    with pytest.raises(ValueError, match="val_regime must be"):
        train_uci.validate_regimes(targets, [regimes[0], regimes[1].float(), regimes[2]], plain, d)
    over = regimes[2].clone()
    over[5] = d + 1
    with pytest.raises(ValueError, match=r"tst_regime spans \[0, %d\]" % (d + 1)):
        train_uci.validate_regimes(targets, [regimes[0], regimes[1], over], plain, d)
