"""gnf_toy_sample (csrc/gnf_toy_data.hip, gnf_hip.ops.toy_sample) on the device, and the toy driver that draws from it.
Injected uniforms against train_toy.toy_reference in fp64; the Philox layout of include/gnf_hip.h against the numpy restatement
of tests/toy_ref.py, bit for bit; independence of a value from B, P, ldx and the other blocks; the float2 form against the scalar
form; the law of the Philox path against the reference's own generator (tests/golden/toy_law.npz); the empty batch; the refused
arguments; two short runs of train_toy.train.

Tolerance of the injected-uniform comparison, per output column: the largest error of the fp32 torch evaluation of toy_reference
(CPU, libm) against its own fp64 evaluation on the same uniforms, times 4 -- the kernel is that arithmetic in fp32, operation by
operation, with the device library's log / sin / cos / exp in place of libm's.  Set GNF_WRITE_PROFILES=1 to write both columns to
profiles/toy_data_error.txt."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import toy_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BATCHES = [1, 5, 63, 64, 65, 257, 1003]
SETS = list(toy_ref.KINDS) + ["8-MIX", "2spirals-8gaussians"]
SEED, OFFSET = 0x1234567887654321 & ((1 << 62) - 1), (7 << 32) + 11       # both halves of the key and of the counter in use
KERNEL_FACTOR = 4.


def _mods():
    import train_toy
    from gnf_hip import ops
    return train_toy, ops


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def parity():
    """per data set: uniforms u [1003, P, 8] (a batch of B rows uses the first B), the fp64 reference and the per-column error
    of the fp32 torch evaluation -- computed once, shared by every batch size"""
    T, ops = _mods()
    out = {}
    for k, name in enumerate(SETS):
        blocks, scale = ops.toy_blocks(name)
        u = toy_ref.toy_uniforms(max(BATCHES), len(blocks), 99, 1000 + k)
        ref64 = T.toy_reference(blocks, u, scale, dtype=torch.float64)
        ref32 = T.toy_reference(blocks, u, scale, dtype=torch.float32)
        out[name] = (blocks, scale, torch.from_numpy(u), ref64, (ref32.double() - ref64).abs().amax(0))
    return out


@pytest.fixture(scope="module")
def kernel_errors(parity):
    """{(name, B): per-column largest |kernel - fp64 reference|}, every data set at every batch size, one launch each"""
    T, ops = _mods()
    errs = {}
    for name, (blocks, scale, u, ref64, tol) in parity.items():
        ud = u.to(DEV)
        for B in BATCHES:
            x = ops.toy_sample(name, B, 0, 0, DEV, u=ud[:B].contiguous())
            assert x.shape == (B, 2 * len(blocks)) and x.dtype == torch.float32
            errs[name, B] = (x.cpu().double() - ref64[:B]).abs().amax(0)
    lines = ["gnf_toy_sample with injected uniforms against train_toy.toy_reference in fp64: largest absolute error over the columns "
             "and over B in %s" % BATCHES,
             "fp32 torch = the fp32 evaluation of toy_reference (CPU) against its fp64 evaluation on the same 1003 x P x 8 "
             "uniforms; the kernel may exceed it by %g per column (tests/test_gpu_toy_data.py); worst ratio = largest "
             "kernel error / fp32 torch error over the columns" % KERNEL_FACTOR,
             "%-22s %14s %14s %12s" % ("data set", "fp32 torch", "kernel", "worst ratio")]
    for name in SETS:
        tol = parity[name][4]
        worst = torch.stack([errs[name, B] for B in BATCHES]).amax(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.nan_to_num(worst.numpy() / tol.numpy(), nan=0.).max()                # 0 / 0: an exact column on both sides
        lines.append("%-22s %14.3e %14.3e %12.3f" % (name, tol.max().item(), worst.max().item(), ratio))
    print("\n".join(lines))
    if os.environ.get("GNF_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "toy_data_error.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return errs


# ------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("B", BATCHES)
def test_injected_uniforms_against_the_reference(parity, kernel_errors, B):
    for name in SETS:
        tol, err = parity[name][4], kernel_errors[name, B]
        over = err > KERNEL_FACTOR * tol
        assert not bool(over.any()), (name, B, err.tolist(), tol.tolist())


def test_numpy_philox_is_the_published_one():
    toy_ref.known_answers()


@pytest.mark.parametrize("P", [1, 8])
def test_philox_layout(P):
    """the kernel keyed by (seed, offset) == the kernel fed the numpy-Philox uniforms of that key, in bits"""
    T, ops = _mods()
    toy_ref.known_answers()
    B = 257
    lists = [[k] for k in range(len(toy_ref.KINDS))] if P == 1 else [list(ops.toy_blocks("8-MIX")[0]), [8] * 8,
                                                                      [13, 12, 11, 10, 9, 7, 2, 1]]
    u = torch.from_numpy(toy_ref.toy_uniforms(B, P, SEED, OFFSET)).to(DEV)
    for blocks in lists:
        keyed = ops.toy_sample(blocks, B, SEED, OFFSET, DEV)
        fed = ops.toy_sample(blocks, B, 0, 0, DEV, u=u)
        assert torch.equal(_bits(keyed), _bits(fed)), blocks


def test_a_value_depends_on_its_own_counter_only():
    T, ops = _mods()
    mix, scale = ops.toy_blocks("8-MIX")
    small, large = ops.toy_sample("8-MIX", 7, SEED, OFFSET, DEV), ops.toy_sample("8-MIX", 300, SEED, OFFSET, DEV)
    assert torch.equal(_bits(small), _bits(large[:7]))                                    # not on B
    # block p of another list at the same position, and alone-but-for-fillers: not on P or the other blocks
    for p in (0, 3, 7):
        other = [0] * (p + 1)
        other[p] = mix[p]
        sc = np.ones(2 * (p + 1), dtype=np.float32)
        sc[2 * p:] = scale[2 * p:2 * p + 2]
        alone = ops.toy_sample(other, 300, SEED, OFFSET, DEV, col_scale=sc)
        assert torch.equal(_bits(alone[:, 2 * p:]), _bits(large[:, 2 * p:2 * p + 2])), p
    for seed, offset in ((SEED + 1, OFFSET), (SEED, OFFSET + 1), (SEED + (1 << 32), OFFSET), (SEED, OFFSET + (1 << 32))):
        moved = ops.toy_sample("8-MIX", 300, seed, offset, DEV)
        assert bool((moved != large).any(1).all()), (seed, offset)                        # every row
    again = ops.toy_sample("8-MIX", 300, SEED, OFFSET, DEV)
    assert torch.equal(_bits(again), _bits(large))


def test_layouts_give_the_same_bits():
    """padding left alone; the scalar-store form (dword-only alignment, odd ldx) == the float2 form; out= is filled and returned"""
    T, ops = _mods()
    for name in ("8-MIX", "2spirals", "2spirals-8gaussians"):
        P = len(ops.toy_blocks(name)[0])
        B = 131
        want = ops.toy_sample(name, B, SEED, OFFSET, DEV)
        assert want.data_ptr() % 8 == 0
        # (padding, floats in front of the base): odd ldx; odd ldx off an 8-byte boundary; the float2 form with padding; even
        # ldx off the boundary -- the sentinel around the columns stays, the bits are those of the contiguous aligned call
        for extra, shift in ((3, 0), (3, 1), (2, 0), (2, 1)):
            ldx = 2 * P + extra
            flat = torch.full((2 + B * ldx,), -7.5, device=DEV)
            rows = flat[shift:shift + B * ldx].view(B, ldx)
            view = rows[:, :2 * P]
            assert view.data_ptr() % 8 == 4 * shift
            got = ops.toy_sample(name, B, SEED, OFFSET, DEV, out=view)
            assert got.data_ptr() == view.data_ptr() and torch.equal(_bits(got), _bits(want)), (name, extra, shift)
            assert bool((rows[:, 2 * P:] == -7.5).all()) and bool((flat[:shift] == -7.5).all())
            assert bool((flat[shift + B * ldx:] == -7.5).all())
        u =torch.from_numpy(toy_ref.toy_uniforms(B, P, SEED, OFFSET)).to(DEV)
        pad = torch.zeros(B * P * 8 + 1, device=DEV)
        pad[1:] = u.reshape(-1)                                                           # uniforms at dword-only alignment
        fed = ops.toy_sample(name, B, 0, 0, DEV, u=pad[1:].view(B, P, 8))
        assert torch.equal(_bits(fed), _bits(want))


def test_rows_past_two_to_the_31_elements():
    """B * 16 > 2^31 output elements: the last rows are those of their own counters (element offsets are 64-bit)"""
    T, ops = _mods()
    B, tail = (1 << 27) + 5, 9
    x = ops.toy_sample("8-MIX", B, SEED, OFFSET, DEV)
    last = x[B - tail:].clone()
    first = x[:tail].clone()
    del x
    torch.cuda.empty_cache()
    blocks, scale = ops.toy_blocks("8-MIX")
    u = torch.from_numpy(toy_ref.toy_uniforms(tail, 8, SEED, OFFSET, b0=B - tail)).to(DEV)
    assert torch.equal(_bits(last), _bits(ops.toy_sample("8-MIX", tail, 0, 0, DEV, u=u)))
    assert torch.equal(_bits(first), _bits(ops.toy_sample("8-MIX", tail, SEED, OFFSET, DEV)))


# ------------------------------------------------------------------------------------ the law of the Philox path
def test_law_of_the_kernels_own_draws():
    """the histogram bound of tests/test_toy_host.py on the kernel's own draws: one launch of 65 536 samples per problem"""
    T, ops = _mods()
    with np.load(os.path.join(GOLDEN, "toy_law.npz")) as f:
        law = {k: f[k] for k in f.files}
    bad = []
    for i, name in enumerate(toy_ref.KINDS):
        x = ops.toy_sample(name, toy_ref.N_LAW, SEED, OFFSET + i, DEV).cpu().numpy()
        assert np.isfinite(x).all(), name
        r_tv, r_mom = toy_ref.law_ratios(x, law["hist"][i], law["mean"][i], law["cov"][i])
        print("%-16s tv ratio %.3f (moment ratio %.3f, reported)" % (name, r_tv, r_mom))
        if not r_tv <= 1.:
            bad.append((name, r_tv))
    assert not bad, bad


# ------------------------------------------------------------------------------------ edges and refusals
def test_empty_batch_on_the_device():
    T, ops = _mods()
    x = ops.toy_sample("8-MIX", 0, SEED, OFFSET, DEV)
    assert x.shape == (0, 16) and x.dtype == torch.float32 and x.device == torch.device(DEV)
    x = ops.toy_sample([3], 0, SEED, OFFSET, DEV, u=torch.zeros(0, 1, 8, device=DEV), out=torch.zeros(0, 2, device=DEV))
    assert x.shape == (0, 2)


def test_wrong_operands_are_refused():
    T, ops = _mods()
    from gnf_hip import GnfError
    ok_u = torch.full((4, 2, 8), .5, device=DEV)
    for u in (ok_u.cpu(), ok_u.double(), ok_u[:3], ok_u[:, :1], torch.full((4, 2, 4), .5, device=DEV)):
        with pytest.raises(GnfError, match="uniforms"):
            ops.toy_sample([8, 3], 4, 1, 0, DEV, u=u)
    for out in (torch.zeros(4, 4), torch.zeros(4, 4, device=DEV, dtype=torch.float64), torch.zeros(4, 6, device=DEV),
                torch.zeros(5, 4, device=DEV), torch.zeros(4, 8, device=DEV)[:, ::2], torch.zeros(4, 4, device=DEV).t()):
        with pytest.raises(GnfError, match="out must be"):
            ops.toy_sample([8, 3], 4, 1, 0, DEV, out=out)
    with pytest.raises(GnfError, match="col_scale"):
        ops.toy_sample([8, 3], 4, 1, 0, DEV, col_scale=np.ones(3, dtype=np.float32))
    with pytest.raises(GnfError, match="own column scale"):
        ops.toy_sample("8-MIX", 4, 1, 0, DEV, col_scale=np.ones(16, dtype=np.float32))
    with pytest.raises(GnfError, match="no CPU fallback"):
        ops.toy_sample([8, 3], 4, 1, 0, "cpu")


# ------------------------------------------------------------------------------------ the driver
def _pgm(path):
    raw = open(path, "rb").read()
    magic, dims, top, body = raw.split(b"\n", 3)
    return magic, tuple(int(v) for v in dims.split()), int(top), np.frombuffer(body, dtype=np.uint8)


def test_driver_coupling_run_is_replayed_from_a_graph(tmp_path):
    T, ops = _mods()
    folder = str(tmp_path) + os.sep
    argv = ["-dataset", "8gaussians", "-nb_epoch", "3", "-plot_every", "1", "-folder", folder]
    run = T.train(T.parse(argv))
    assert len(run.train_losses) == 3 and np.isfinite(run.train_losses).all() and np.isfinite(run.test_losses).all()
    gs = getattr(run.state, "_graphed", None)
    assert gs is not None and gs.captures >= 1 and run.state.t == 3                        # the GraphedStep route
    stem = os.path.join(folder, "8gaussians", "Affine[150, 150, 150]3")
    assert os.path.isfile(stem + "model.pt") and os.path.isfile(stem + "ADAM.pt")
    for epoch in range(3):
        plot = os.path.join(folder, "8gaussians", "flow_Affine[150, 150, 150]3_%d" % epoch)
        magic, dims, top, body = _pgm(plot + ".pgm")
        assert (magic, dims, top) == (b"P5", (100, 100), 255) and body.size == 100 * 100 and body.max() == 255
        assert np.loadtxt(plot + "_marginals.txt").shape == (2, 100)
    qz = T.density_grid(run.model, torch.device(DEV))                                      # the model as the last epoch left it
    assert qz.shape == (100, 100) and np.isfinite(qz).all() and (qz >= 0).all()
    marg = np.loadtxt(plot + "_marginals.txt")
    np.testing.assert_allclose(marg[0], qz.sum(1), rtol=1e-6)
    np.testing.assert_allclose(marg[1], qz.sum(0), rtol=1e-6)
    saved = torch.load(stem + "model.pt", map_location="cpu")
    adam = torch.load(stem + "ADAM.pt", map_location="cpu")
    assert set(saved) == set(run.model.state_dict()) and adam["param_groups"][0]["lr"] == 1e-4
    assert adam["param_groups"][0]["weight_decay"] == 1e-5 and all(float(s["step"]) == 3 for s in adam["state"].values())
    resumed = T.train(T.parse(argv[:2] + ["-nb_epoch", "0", "-load"] + argv[4:]))
    for k, v in resumed.model.state_dict().items():
        assert torch.equal(v.cpu(), saved[k]), k
    assert resumed.state.t == 3
    again = resumed.state.optimizer_state_dict(resumed.model, 1e-4, 1e-5)
    for i, s in adam["state"].items():
        assert torch.equal(again["state"][i]["exp_avg"].cpu(), s["exp_avg"])
        assert torch.equal(again["state"][i]["exp_avg_sq"].cpu(), s["exp_avg_sq"])


def test_driver_dag_run_stays_eager(tmp_path):
    T, ops = _mods()
    folder = str(tmp_path) + os.sep
    run = T.train(T.parse(["-dataset", "8-MIX", "-cond_type", "DAG", "-emb_net", "20", "20", "10", "-nb_flow", "1", "-nb_epoch", "2",
                           "-plot_every", "1", "-folder", folder]))
    assert len(run.train_losses) == 2 and np.isfinite(run.train_losses).all() and np.isfinite(run.test_losses).all()
    assert getattr(run.state, "_graphed", None) is None and run.state.t == 2               # the stochastic gate is not replayed
    out = os.path.join(folder, "8-MIX")
    stem = os.path.join(out, "Affine[20, 20, 10]1")
    assert os.path.isfile(stem + "model.pt") and os.path.isfile(stem + "ADAM.pt")
    assert not [f for f in os.listdir(out) if f.endswith(".pgm") or f.endswith("_marginals.txt")]     # d = 16: no plot
    for epoch in range(2):
        assert np.loadtxt(os.path.join(out, "A_0_%d.txt" % epoch)).shape == (16, 16)
    c = run.model.getConditioners()[0]
    assert c.stoch_gate and not c.noise_gate and c.gumble_T == .5 and c.hot_encoding and c.nb_epoch_update == 50
