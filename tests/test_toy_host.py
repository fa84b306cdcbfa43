"""The toy sampler's host half, no GPU needed: the gnf_toy_sample symbol and its argument checks (every refused call returns
before a launch), the block lists of the nineteen data sets, the LAW of the sampler's arithmetic (train_toy.toy_reference on
the numpy-Philox uniforms the kernel would draw) against statistics of the reference's own generator (tests/golden/toy_law.npz),
and the toy driver's arguments.

The law bound comes from the fixture alone: for every base problem the eight reference draws give a pooled histogram, the
largest leave-one-out total-variation distance among them, and centre and spread of the five moment entries (toy_ref.law_bounds).
Set GNF_WRITE_PROFILES=1 to write the measured ratios to profiles/toy_data_law.txt."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import toy_ref

SEED, OFFSET = 0x0123456789abcdef & ((1 << 62) - 1), (3 << 32) + 5


@pytest.fixture(scope="module")
def law():
    with np.load(os.path.join(GOLDEN, "toy_law.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def candidates():
    """toy_reference (fp32) on the Philox uniforms of (SEED, OFFSET): x [N_LAW, 2] per base problem, computed once"""
    import train_toy
    out = {}
    for k, name in enumerate(toy_ref.KINDS):
        u = toy_ref.toy_uniforms(toy_ref.N_LAW, 1, SEED, OFFSET + k)
        out[name] = train_toy.toy_reference([k], u).numpy()
    return out


# ------------------------------------------------------------------------------------ symbol and argument checks
def test_symbol_declared_and_bound():
    from gnf_hip import abi, ops
    header = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    assert "gnf_toy_sample(" in header
    assert "gnf_toy_sample" in abi.SIGNATURES
    assert hasattr(abi.load(), "gnf_toy_sample")
    assert abi.ABI_VERSION == 11 and abi.load().gnf_abi_version() == 11
    assert "#define GNF_ABI_VERSION 11" in header
    assert ops.TOY_KINDS == toy_ref.KINDS


def test_argument_errors_return_before_any_launch():
    """NULL / never-dereferenced device pointers: every call here returns on the host"""
    from gnf_hip import abi
    fn = abi.load().gnf_toy_sample
    p = ctypes.c_void_p(1 << 20)

    def rc(kinds=(8, 3), P=None, scale=None, u=None, x=p, ldx=None, B=4):
        P = len(kinds) if P is None else P
        arr = (ctypes.c_int32 * max(len(kinds), 1))(*kinds)
        return fn(ctypes.cast(arr, ctypes.c_void_p), P, scale, u, 1, 0, x, 2 * P if ldx is None else ldx, B, None)
    assert rc(kinds=(), P=0, x=None) == -1                       # P = 0
    assert rc(kinds=(0,) * 9, x=None) == -1                      # P = 9
    assert rc(kinds=(8, 14), x=None) == -1 and rc(kinds=(-1,), x=None) == -1      # unknown kind
    assert rc(ldx=3, x=None) == -1                               # ldx < 2P
    assert rc(B=(1 << 32) + 1, x=None) == -1                     # the sample index is one counter word
    assert rc(B=-1) == -1
    assert fn(None, 2, None, None, 1, 0, p, 4, 4, None) == -1    # no block list
    assert rc(x=None) == -1                                      # B > 0 needs x
    odd = ctypes.c_void_p((1 << 20) + 2)
    assert rc(x=odd) == -1 and rc(u=odd) == -1
    assert rc(x=None, B=0) == 0                                  # the empty batch: no launch, x may be NULL
    assert rc(kinds=(8, 14), x=None, B=0) == -1                  # ... but its arguments are still checked


def test_ops_refuses_before_the_call():
    from gnf_hip import ops, GnfError
    with pytest.raises(GnfError, match="no CPU fallback"):
        ops.toy_sample("8gaussians", 4, 1, 0, "cpu")
    with pytest.raises(GnfError, match="unknown toy data set"):
        ops.toy_sample("9gaussians", 4, 1, 0, "cuda")
    with pytest.raises(GnfError, match="not a base problem"):
        ops.toy_sample(["8-MIX"], 4, 1, 0, "cuda")
    with pytest.raises(GnfError, match="outside 0"):
        ops.toy_sample([14], 4, 1, 0, "cuda")
    with pytest.raises(GnfError, match="blocks"):
        ops.toy_sample([0] * 9, 4, 1, 0, "cuda")
    with pytest.raises(GnfError, match="blocks"):
        ops.toy_sample([], 4, 1, 0, "cuda")
    with pytest.raises(GnfError, match="2\\^32"):
        ops.toy_sample([0], (1 << 32) + 1, 1, 0, "cuda")


# ------------------------------------------------------------------------------------ block lists
def test_toy_blocks_of_the_nineteen_data_sets():
    import train_toy
    from gnf_hip import ops, GnfError
    assert len(train_toy.DATASETS) == 19 and set(train_toy.DATASETS) == set(ops.TOY_DATASETS)
    K = ops.TOY_KINDS.index
    for name in ops.TOY_KINDS:
        assert ops.toy_blocks(name) == ((K(name),), None)
    sp, g8 = K("2spirals"), K("8gaussians")
    assert ops.toy_blocks("2spirals-8gaussians") == ((sp, g8), None)
    assert ops.toy_blocks("4-2spirals-8gaussians") == ((sp, g8) * 2, None)
    assert ops.toy_blocks("8-2spirals-8gaussians") == ((sp, g8) * 4, None)
    widths = {n: 2 * len(ops.toy_blocks(n)[0]) for n in train_toy.DATASETS}
    assert [widths[n] for n in ("8gaussians", "2spirals-8gaussians", "4-2spirals-8gaussians", "8-2spirals-8gaussians", "7-MIX",
                                "8-MIX")] == [2, 4, 8, 16, 14, 16]
    # lib/toy_data.py:42-43, :55-56 and the concatenation orders of :44 and :57 (data5 = line and data8 = moons in 8-MIX)
    std = np.array([1.604934, 1.584863, 2.0310535, 2.0305095, 1.337718, 1.4043778, 1.6944685, 1.6935346, 1.7434783,
                    1.0092416, 1.4860426, 1.485661, 2.3067558, 2.311637, 1.4430547, 1.4430547], dtype=np.float32)
    b8, s8 = ops.toy_blocks("8-MIX")
    assert [ops.TOY_KINDS[k] for k in b8] == ["2spirals", "8gaussians", "swissroll", "circles", "line", "pinwheel",
                                              "checkerboard", "moons"]
    assert s8.dtype == np.float32 and np.array_equal(s8, np.float32(1.) / std)
    b7, s7 = ops.toy_blocks("7-MIX")
    assert [ops.TOY_KINDS[k] for k in b7] == ["2spirals", "8gaussians", "swissroll", "circles", "moons", "pinwheel",
                                              "checkerboard"]
    assert np.array_equal(s7, np.float32(1.) / std[:14])
    with pytest.raises(GnfError):
        ops.toy_blocks("conditionnal8gaussians")


# ------------------------------------------------------------------------------------ the law
def test_numpy_philox_is_the_published_one():
    toy_ref.known_answers()


def test_uniform_layout_is_per_sample_and_per_block():
    """a (sample, block) reads its own counters: the uniforms do not depend on B or P"""
    u = toy_ref.toy_uniforms(9, 3, SEED, OFFSET)
    assert np.array_equal(u[2:5, :2], toy_ref.toy_uniforms(3, 2, SEED, OFFSET, b0=2))
    assert u.min() > 0 and u.max() < 1 and len(np.unique(u)) > 200


def test_reference_draws_pass_their_own_bound(law):
    """each of the eight reference draws, judged as a candidate would be"""
    for i, name in enumerate(toy_ref.KINDS):
        for k, (r_tv, r_mom) in enumerate(toy_ref.self_ratios(law["hist"][i], law["mean"][i], law["cov"][i])):
            assert r_tv <= 1. and r_mom <= 1., (name, k, r_tv, r_mom)


def test_fixture_is_what_the_generator_describes(law):
    assert [str(n) for n in law["names"]] == list(toy_ref.KINDS)
    assert law["hist"].shape == (14, 8, 32, 32) and law["hist"].dtype == np.int32
    counts = law["hist"].sum((2, 3))
    pin = toy_ref.KINDS.index("pinwheel")
    assert (np.delete(counts, pin, 0) == toy_ref.N_LAW).all() and (counts[pin] == toy_ref.N_LAW - 1).all()
    assert law["mean"].shape == (14, 8, 2) and law["cov"].shape == (14, 8, 3) and law["mix_corr"].shape == (16, 16)


@pytest.fixture(scope="module")
def ratios(law, candidates):
    """(tv ratio, moment ratio) per problem, computed once; the table goes to profiles/toy_data_law.txt on request"""
    out = {}
    lines = ["Law of train_toy.toy_reference (fp32, numpy-Philox uniforms, N = %d) against tests/golden/toy_law.npz" % toy_ref.N_LAW,
             "tv ratio = TV(candidate, pooled reference) / (%.1f x largest leave-one-out TV of the eight reference draws); "
             "moment ratio = largest |entry - centre| / (%g sd of the eight reference values, floor 1e-3 of the scale); "
             "both must be <= 1 (tests/test_toy_host.py)" % (toy_ref.TV_MARGIN, toy_ref.N_SIGMA),
             "%-16s %10s %12s %10s %12s" % ("problem", "TV", "loo TV max", "tv ratio", "moment ratio")]
    for i, name in enumerate(toy_ref.KINDS):
        h, m, c = law["hist"][i], law["mean"][i], law["cov"][i]
        r_tv, r_mom = toy_ref.law_ratios(candidates[name], h, m, c)
        loo = toy_ref.law_bounds(h, m, c)[1]
        lines.append("%-16s %10.5f %12.5f %10.3f %12.3f" % (name, r_tv * toy_ref.TV_MARGIN * loo, loo, r_tv, r_mom))
        out[name] = (r_tv, r_mom)
    print("\n".join(lines))
    if os.environ.get("GNF_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "toy_data_law.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return out


@pytest.mark.parametrize("name", toy_ref.KINDS)
def test_law_of_the_reference_arithmetic(ratios, name):
    """Histogram and moments of toy_reference's draws inside the fixture's own spread (module docstring).

    The moment bound is the tight one for `circles` and `moons` (ratios .72 and .54 at this key; every other problem stays
    below .5): the reference's spread is not that of an i.i.d. sample there.  scikit-learn lays the angles of make_circles /
    make_moons on a linspace and fixes the ring counts, so across its draws a mean of `circles` varies by the noise term only,
    3 * .08 / sqrt(N) = 9e-4 -- the width is the 1e-3 floor, 1.7e-3 -- while the N = 65 536 independent angles the sampler draws
    on purpose move it by 3 * sqrt(.3125) / sqrt(N) = 6.6e-3 (one standard deviation), four widths of the six allowed.
    The key is fixed, so the outcome is too; the bound is the fixture's and is not widened for these two."""
    r_tv, r_mom = ratios[name]
    assert r_tv <= 1., (name, r_tv)
    assert r_mom <= 1., (name, r_mom)


def test_mix_columns(law):
    """8-MIX through toy_reference: the reference's `std` vector leaves every column near unit standard deviation, and
    columns of different blocks are independent.  N = 16 384 rows on both sides.  Bounds, from sampling theory alone:
      * a correlation of two independent columns has standard deviation 1 / sqrt(N): every cross-block entry, the fixture's
        own included, stays within 5 / sqrt(N) (112 pairs: exceeded with probability 6e-5);
      * a mean of a unit-variance column has standard error 1 / sqrt(N), a standard deviation sqrt((kappa - 1) / 4N) with
        kurtosis kappa < 4 for these bounded or mixture-of-Gaussian columns: candidate and fixture, two independent samples,
        differ by at most 6 sqrt(2) of those."""
    import train_toy
    from gnf_hip import ops
    blocks, scale = ops.toy_blocks("8-MIX")
    N = toy_ref.N_MIX
    x = train_toy.toy_reference(blocks, toy_ref.toy_uniforms(N, 8, SEED, OFFSET + 100), scale).numpy()
    assert x.shape == (N, 16)
    mean, std, corr = toy_ref.mix_stats(x)
    cross = np.kron(np.eye(8), np.ones((2, 2))) == 0
    bound = 5. / np.sqrt(N)
    assert np.abs(law["mix_corr"][cross]).max() <= bound
    assert np.abs(corr[cross]).max() <= bound, np.abs(corr[cross]).max()
    assert np.abs(mean - law["mix_mean"]).max() <= 6. * np.sqrt(2. / N)
    assert np.abs(std - law["mix_std"]).max() <= 6. * np.sqrt(2. * 3. / (4. * N))
    # unit standard deviation where the `std` entries were measured on the block they divide: 8-MIX applies the entries of
    # `moons` to its fifth block, which is `line` there, and the entries of `line` to `moons` (lib/toy_data.py:38, :41, :44) --
    # those four columns come out at .83, 1.43, 1.21 and .70 in the reference as well, which the fixture comparison above pins
    own = np.ones(16, dtype=bool)
    own[[8, 9, 14, 15]] = False
    assert np.abs(law["mix_std"][own] - 1.).max() <= .02
    assert np.abs(std[own] - 1.).max() <= .02 + 6. * np.sqrt(2. * 3. / (4. * N))


def test_reference_in_fp64_is_the_same_law(candidates):
    """fp32 and fp64 evaluations of the same uniforms agree to rounding: no class or coin flips between them"""
    import train_toy
    for k, name in enumerate(toy_ref.KINDS):
        u = toy_ref.toy_uniforms(4096, 1, SEED, OFFSET + k)
        x64 = train_toy.toy_reference([k], u, dtype=torch.float64).numpy()
        assert np.abs(candidates[name][:4096] - x64).max() <= 1e-4 * max(1., np.abs(x64).max()), name


# ------------------------------------------------------------------------------------ the driver's arguments
def test_driver_arguments():
    import train_toy
    a = train_toy.parse([])
    assert (a.dataset, a.load, a.folder, a.nb_steps_dual, a.l1, a.nb_epoch) == (None, False, "", 50, 0., 20000)
    assert (a.cond_type, a.nb_flow, a.emb_net, a.batch_size, a.nb_samp, a.seed, a.plot_every, a.host_data) == \
        ("Coupling", 3, [150, 150, 150], 100, 100, 0, 500, False)
    assert train_toy.save_name(a) == "Affine[150, 150, 150]3"
    b = train_toy.parse(["-dataset", "8-MIX", "-cond_type", "DAG", "-emb_net", "20", "20", "10", "-nb_flow", "1"])
    assert train_toy.save_name(b) == "Affine[20, 20, 10]1" and b.dataset == "8-MIX"
    with pytest.raises(SystemExit):
        train_toy.parse(["-dataset", "conditionnal8gaussians"])
    a.dataset = "9gaussians"
    with pytest.raises(SystemExit, match="unknown toy data set"):
        train_toy.train(a)
