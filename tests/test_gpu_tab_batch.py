"""Device-side epochs of train_uci.py (-m gpu): gnf_tab_batch against torch indexing on both of its forms, with a cursor,
at dword-only alignment and with indices outside the arrays; gnf_shuffle_keys against the numpy restatement of its layout
(tests/uci_ref.py); K optimisation steps per hipGraph replay (dp.GraphedStep.steps) against autograd + torch.optim.Adam on
the same batch sequence; the driver with its new options, resumed, and on two ranks."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err
import misaligned
import uci_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ROWS = 37


def _table(d, pad):
    """[N_ROWS, d] view with row stride d + pad of a seeded table"""
    base = torch.randn(N_ROWS, d + pad, generator=torch.Generator().manual_seed(100 + d)).to(DEV)
    return base[:, :d]


def _perm(n_perm=200):
    return torch.randint(0, N_ROWS, (n_perm,), generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV)


@pytest.mark.parametrize("d", [1, 3, 4, 6, 63, 64])
def test_gather_equals_torch_indexing(d):
    from gnf_hip import abi, ops
    perm = _perm()
    for pad in (0, 4):
        X = _table(d, pad)
        assert X.stride(0) == d + pad
        for B in (1, 5, 65):
            for stride in (1, 3):
                for first in (0, 2):
                    what = (d, pad, B, stride, first)
                    got = ops.tab_batch(X, perm, first, stride, B)
                    assert got.shape == (B, d) and torch.equal(got, X[perm.long()[first::stride][:B]]), what
                    if first + (B - 1) * stride < N_ROWS:          # perm NULL: the identity over the rows
                        assert torch.equal(ops.tab_batch(X, None, first, stride, B), X[first::stride][:B]), what
                    else:                                           # ... which the batch must not run past
                        with pytest.raises(abi.GnfError):
                            ops.tab_batch(X, None, first, stride, B)
    with pytest.raises(abi.GnfError):
        ops.tab_batch(X, perm, 198, 1, 3)                           # runs past the permutation


@pytest.mark.parametrize("d", [4, 64])
def test_dword_aligned_operands_take_the_other_form_with_the_same_bits(d):
    from gnf_hip import ops
    perm = _perm()
    X = _table(d, 0).contiguous()
    want = ops.tab_batch(X, perm, 2, 3, 65)                         # 16-byte aligned, d % 4 == 0: the float4 form;
    # X or x at dword-only alignment: the form for any address (dword-aligned quads + single floats)
    assert torch.equal(want, X[perm.long()[2::3][:65]])
    for kx, ko in ((1, 0), (0, 2), (3, 1), (2, 2)):
        Xm, out = misaligned.place(X, kx), misaligned.place(torch.zeros(65, d, device=DEV), ko)
        ops.tab_batch(Xm, perm, 2, 3, 65, out=out)
        assert torch.equal(out, want), (kx, ko)
        assert misaligned.guards_intact(out) and misaligned.guards_intact(Xm)


def test_cursor_form_equals_first_by_value():
    from gnf_hip import ops
    perm = _perm()
    for d in (6, 64):
        X = _table(d, 0)
        for c in (0, 7, 40):
            cur = torch.tensor([c], dtype=torch.int32, device=DEV)
            got = ops.tab_batch(X, perm, 2, 3, 20, cursor=cur)
            assert torch.equal(got, ops.tab_batch(X, perm, 2 + c, 3, 20)), (d, c)
            assert int(cur) == c                                    # the kernel only reads it


def test_indices_outside_the_arrays_are_clamped():
    from gnf_hip import ops
    for d in (6, 64):
        X = _table(d, 0)
        perm = torch.tensor([-5, N_ROWS + 3, 1, 4], dtype=torch.int32, device=DEV)
        out = misaligned.place(torch.zeros(3, d, device=DEV), 0)
        ops.tab_batch(X, perm, 0, 1, 3, out=out)
        assert torch.equal(out, X[[0, N_ROWS - 1, 1]])
        assert misaligned.guards_intact(out)
        for c in (4, 1000, -9):                                     # a cursor outside the permutation: the last / first position
            cur = torch.tensor([c], dtype=torch.int32, device=DEV)
            out = misaligned.place(torch.zeros(5, d, device=DEV), 0)
            ops.tab_batch(X, perm, 0, 1, 5, cursor=cur, out=out)
            row = 4 if c > 0 else 0
            assert torch.equal(out, X[[row] * 5]) and misaligned.guards_intact(out), (d, c)


def test_empty_batch():
    from gnf_hip import abi, ops
    X = _table(6, 0)
    assert ops.tab_batch(X, _perm(), 0, 1, 0).shape == (0, 6)
    assert abi.load().gnf_tab_batch(None, 0, 6, 6, None, 0, 0, 1, None, None, 0, None) == 0
    assert ops.shuffle_keys(1, 2, 0, device=DEV).shape == (0,)


def test_keys_equal_the_numpy_restatement():
    from gnf_hip import dp, ops
    for n in (1, 5, 1000, 4097):
        for seed, offset in ((0, 0), (1234, 1), (0x9E3779B97F4A7C15, (7 << 32) + 5)):
            keys = ops.shuffle_keys(seed, offset, n, device=DEV)
            assert keys.dtype == torch.int64
            assert np.array_equal(keys.cpu().numpy(), uci_ref.shuffle_keys(seed, offset, n)), (n, seed, offset)
            assert torch.equal(ops.shuffle_keys(seed, offset, n, out=torch.empty_like(keys)), keys)      # the same bits again
    X = _table(6, 0)
    src = dp.DeviceBatches(X, 8, seed=77)
    where = src.perm.data_ptr()
    for e in (0, 1, 5):
        src.start_epoch(e)
        assert src.perm.data_ptr() == where and src.perm.dtype == torch.int32
        assert np.array_equal(src.perm.cpu().numpy(), uci_ref.permutation(77, e, N_ROWS)), e
        assert int(src.cursor) == 0
        got = [src.next() for _ in range(src.left())]
        assert [g.shape[0] for g in got] == [8, 8, 8, 8, 5] and src.full_left() == 0
        assert torch.equal(torch.cat(got), X[src.perm.long()])


def test_k_steps_per_replay_against_autograd_and_torch_adam():
    """Affine + MADE, d = 12, hidden [64, 64], B = 8, N = 44: per epoch two replays of K = 2 steps, one single step, one
    tail of 4 rows.  Reference: autograd + torch.optim.Adam over the batches of the restated permutation -- the reference
    and the bound (rel_err < 1e-5) of test_graphed_step_vs_torch_adam_reference."""
    from gnf_hip import dp
    from models import buildFCNormalizingFlow, AutoregressiveConditioner, AffineNormalizer
    N, B, K, seed, lr, wd = 44, 8, 2, 5, 1e-2, 1e-5

    def make():
        torch.manual_seed(11)
        return buildFCNormalizingFlow(1, AutoregressiveConditioner, {"in_size": 12, "hidden": [64, 64], "out_size": 2},
                                      AffineNormalizer, {}).to(DEV)
    X = torch.randn(N, 12, generator=torch.Generator().manual_seed(201)).to(DEV)
    perms = [uci_ref.permutation(seed, e, N) for e in (0, 1)]
    assert not np.array_equal(perms[0][:32], perms[1][:32])            # epoch 2's replays read other rows than epoch 1's
    fa = make()
    opt = torch.optim.Adam(fa.parameters(), lr=lr, weight_decay=wd)
    want, snaps = [], []
    for p in perms:
        losses = []
        for i in range(0, N, B):
            opt.zero_grad()
            z, ld = fa(X[torch.from_numpy(p[i:i + B].astype(np.int64)).to(DEV)])
            la = fa.loss(z, ld)
            la.backward()
            opt.step()
            losses.append(la.detach().double().cpu())
        want.append(losses)
        snaps.append([q.detach().clone() for q in fa.parameters()])

    fb = make()
    sb = dp.FlatState(fb)
    src = dp.DeviceBatches(X, B, seed=seed)
    assert dp.steps_replayable(fb, src) and src.n_full == 5 and len(src) == 6
    where = src.perm.data_ptr()
    for e in (0, 1):
        src.start_epoch(e)
        assert src.perm.data_ptr() == where
        for r in range(2):
            assert src.full_left() >= K
            got = dp.train_steps(fb, sb, src, K, lr=lr, weight_decay=wd)
            ref = want[e][2 * r] + want[e][2 * r + 1]
            print("epoch %d replay %d: loss sum %.7f, reference %.7f" % (e, r, float(got), float(ref)))
            assert rel_err(got.cpu(), ref) < 1e-5, (e, r)
        assert src.full_left() == 1 and src.left() == 2
        with pytest.raises(RuntimeError):
            dp.train_steps(fb, sb, src, K, lr=lr, weight_decay=wd)      # one full batch left: no group of two
        for i in (4, 5):                                                # the single step and the tail of 4 rows
            x = src.next()
            assert x.shape[0] == (B if i == 4 else 4)
            got = dp.train_step(fb, sb, x, lr=lr, weight_decay=wd)
            assert rel_err(got.detach().cpu(), want[e][i]) < 1e-5, (e, i)
        gs = sb._graphed
        assert sb.t == 6 * (e + 1) and int(gs.step_dev) == sb.t and int(src.cursor) == 2 * K * B and src.left() == 0
        for (k, _), pa, pb in zip(fa.named_parameters(), snaps[e], fb.parameters()):
            err = rel_err(pb.detach().cpu(), pa.cpu())
            print("epoch %d %s: rel_err %.3g" % (e, k, err))
            assert err < 1e-5, (e, k)
    assert gs.captures == 3                                             # the group, the single step, the tail: epoch 2 replays all


def test_replay_of_groups_is_refused_where_a_step_is_not_replayable():
    from gnf_hip import dp
    from models import (buildFCNormalizingFlow, CouplingConditioner, DAGConditioner, AffineNormalizer, MonotonicNormalizer)
    X = _table(6, 0)
    src = dp.DeviceBatches(X, 8)
    mono = buildFCNormalizingFlow(1, CouplingConditioner, {"in_size": 6, "hidden": [16], "out_size": 4}, MonotonicNormalizer,
                                  {"integrand_net": [16, 16], "cond_size": 4, "nb_steps": 10, "solver": "CC"}).to(DEV)
    assert not dp.steps_replayable(mono, src)                           # the drivers jitter nb_steps per batch
    dag = buildFCNormalizingFlow(1, DAGConditioner, {"in_size": 6, "hidden": [16], "out_size": 2, "l1": .1}, AffineNormalizer,
                                 {}).to(DEV)
    assert dp.GraphedStep.graphable(dag) == dp.steps_replayable(dag, src)
    for c in dag.getConditioners():
        c.stoch_gate, c.s_thresh = True, True
    assert not dp.steps_replayable(dag, src)
    with pytest.raises(RuntimeError):
        dp.train_steps(dag, dp.FlatState(dag), src, 2)
    two = dp.DeviceBatches(X, 8, rank=1, world=2)                       # a shard of a two-rank run
    aff = buildFCNormalizingFlow(1, CouplingConditioner, {"in_size": 6, "hidden": [16], "out_size": 2}, AffineNormalizer,
                                 {}).to(DEV)
    assert dp.steps_replayable(aff, src) and not dp.steps_replayable(aff, two)


def _npz(tmp_path, n=1030):
    g = np.random.default_rng(0)
    path = tmp_path / "power_like.npz"
    np.savez(path, trn=g.standard_normal((n, 6)).astype("float32"), val=g.standard_normal((200, 6)).astype("float32"),
             tst=g.standard_normal((200, 6)).astype("float32"))
    return str(path)


def _spies(monkeypatch):
    """records of one or more train_uci.train() calls: the FlatStates built, the epochs started with their permutations,
    the groups replayed"""
    from gnf_hip import dp
    rec = {"states": [], "epochs": [], "groups": 0}

    class State(dp.FlatState):
        def __init__(self, module):
            super().__init__(module)
            rec["states"].append(self)

    start, steps = dp.DeviceBatches.start_epoch, dp.train_steps

    def start_epoch(self, e):
        start(self, e)
        rec["epochs"].append((e, self.perm.cpu().numpy().copy()))

    def train_steps(*a, **k):
        rec["groups"] += 1
        return steps(*a, **k)

    monkeypatch.setattr(dp, "FlatState", State)
    monkeypatch.setattr(dp.DeviceBatches, "start_epoch", start_epoch)
    monkeypatch.setattr(dp, "train_steps", train_steps)
    return rec


def _train_losses(folder):
    lines = [l for l in open(os.path.join(folder, "logs")) if l.startswith("epoch") and "Train loss" in l]
    return [float(re.search(r"Train loss: (\S+)", l).group(1)) for l in lines]


def test_driver_dag_run_takes_single_steps_sweeps_and_resumes(tmp_path, monkeypatch):
    import train_uci
    rec = _spies(monkeypatch)
    folder = str(tmp_path / "dag")
    common = ["-dataset", "power", "-data", _npz(tmp_path), "-folder", folder, "-conditioner", "DAG", "-normalizer", "affine",
              "-emb_net", "16", "16", "4", "-device_batches", "-seed", "3", "-steps_per_replay", "4", "-threshold_sweep"]
    model = train_uci.train(train_uci.parse(common + ["-nb_epoch", "2"]))
    losses = _train_losses(folder)
    assert len(losses) == 2 and all(np.isfinite(l) for l in losses)
    assert rec["groups"] == 0                                           # the stochastic gate: no group is replayed
    assert rec["states"][0].t == 2 * 11                                 # ten full batches and the tail of 30, step by step
    log = open(os.path.join(folder, "logs")).read()
    sweep = re.findall(r"^epoch: (\d+) - Threshold: (\S+) - Valid log-likelihood: (\S+) - <<DAGness>>: (\S+)$", log, re.M)
    assert [(int(e), float(t)) for e, t, _, _ in sweep] == [(0, t) for t in train_uci.THRESHOLDS]
    assert all(np.isfinite(float(ll)) for _, _, ll, _ in sweep)
    # the sweep itself: deterministic hard-thresholded gate inside, every setting back afterwards
    conds = model.getConditioners()
    for c in conds:
        c.h_thresh = .25
    before = [(c.stoch_gate, c.noise_gate, c.s_thresh, c.h_thresh) for c in conds]
    seen, said = [], []

    def mean_ll(m, X, b, gen, on_device=False):
        seen.append([(c.stoch_gate, c.noise_gate, c.s_thresh, c.h_thresh) for c in m.getConditioners()])
        return 0.
    monkeypatch.setattr(train_uci, "mean_ll", mean_ll)
    train_uci.threshold_sweep(model, None, 100, None, 10, said.append)
    assert seen == [[(False, False, True, t)] * len(conds) for t in train_uci.THRESHOLDS] and len(said) == 5
    assert [(c.stoch_gate, c.noise_gate, c.s_thresh, c.h_thresh) for c in conds] == before
    monkeypatch.undo()
    # a resumed run goes on with the permutation of the next epoch number: a function of (seed, epoch, n), no generator
    rec = _spies(monkeypatch)
    train_uci.train(train_uci.parse(common + ["-nb_epoch", "1", "-load"]))
    assert [e for e, _ in rec["epochs"]] == [2]
    assert np.array_equal(rec["epochs"][0][1], uci_ref.permutation(3, 2, 1030))
    assert rec["states"][0].t == 3 * 11


def test_driver_coupling_run_replays_groups(tmp_path, monkeypatch):
    import train_uci
    rec = _spies(monkeypatch)
    folder = str(tmp_path / "coupling")
    args = train_uci.parse(["-dataset", "power", "-data", _npz(tmp_path), "-folder", folder, "-conditioner", "Coupling",
                            "-normalizer", "affine", "-emb_net", "16", "16", "2", "-device_batches", "-seed", "3",
                            "-steps_per_replay", "4", "-threshold_sweep", "-nb_epoch", "3"])
    train_uci.train(args)
    losses = _train_losses(folder)
    assert len(losses) == 3 and all(np.isfinite(l) for l in losses)
    assert "Threshold" not in open(os.path.join(folder, "logs")).read()          # the sweep is for DAG conditioners
    state = rec["states"][0]
    assert rec["groups"] == 3 * 2 and state.t == 3 * 11                 # 10 full batches = 2 groups of 4 + 2 single steps; the tail
    assert state._graphed.captures <= 3                                 # the group, the full batch, the tail -- once each
    assert [e for e, _ in rec["epochs"]] == [0, 1, 2]
    for e, perm in rec["epochs"]:
        assert np.array_equal(perm, uci_ref.permutation(3, e, 1030))
    # the same batches step by step: the trajectory of the groups is that of single steps
    rec2 = _spies(monkeypatch)
    args2 = train_uci.parse(["-dataset", "power", "-data", _npz(tmp_path), "-folder", str(tmp_path / "single"), "-conditioner",
                             "Coupling", "-normalizer", "affine", "-emb_net", "16", "16", "2", "-device_batches", "-seed", "3",
                             "-nb_epoch", "3"])
    train_uci.train(args2)
    assert rec2["groups"] == 0
    assert rel_err(rec2["states"][0].flat.cpu(), state.flat.cpu()) < 1e-5
    assert np.allclose(_train_losses(str(tmp_path / "single")), losses, rtol=1e-5, atol=1e-6)


def test_two_ranks_with_device_batches_stay_in_lockstep(tmp_path):
    """train_uci.py -device_batches under torch.distributed.run with two ranks (gloo transport on a one-GPU box): every rank
    sorts the same keys, so the shards are cut from the same permutation without a broadcast; a ragged data set size"""
    import socket
    import subprocess
    env = dict(os.environ, GNF_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "graphical-normalizing-flows_amd", "train_uci.py"), "-dataset", "power", "-data",
           _npz(tmp_path, 1003), "-folder", str(tmp_path / "run"), "-nb_epoch", "2", "-b_size", "250", "-conditioner", "DAG",
           "-emb_net", "16", "16", "4", "-normalizer", "affine", "-nb_steps_dual", "1", "-l1", "0.1", "-device_batches",
           "-steps_per_replay", "4"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "replicas diverged" not in r.stdout + r.stderr
    assert len(_train_losses(str(tmp_path / "run"))) == 2
