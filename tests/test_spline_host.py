"""CPU (-m "not gpu"): the host half of the Spline normalizer -- the law of tests/spline_ref.py in fp64 (round trip, jac =
dz/dx, continuity across knots and tails), the new gnf_spline_* / gnf_made_prefix*_spline symbols declared, bound and exported
under the unchanged ABI number, the argument checks that answer before any launch, no CPU fallback, the factories' conditioner
width and the UCI driver's argument error."""
import ctypes
import os
import re

import pytest
import torch

import spline_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnf_spline_fwd", "gnf_spline_bwd", "gnf_spline_inv", "gnf_made_prefix_spline", "gnf_made_prefix_ctx_spline")
BINS = (2, 5, 8, 32)


def _case(K, T, seed, n=400, scale=1.):
    g = torch.Generator().manual_seed(seed)
    h = scale * torch.randn(n, 3 * K - 1, generator=g, dtype=torch.float64)
    x = 2.2 * T / 3. * torch.randn(n, generator=g, dtype=torch.float64)
    return x, h


# ------------------------------------------------------------------------------------------------------- the law, fp64
@pytest.mark.parametrize("K", BINS)
@pytest.mark.parametrize("T", (3., .5))
def test_round_trip(K, T):
    x, h = _case(K, T, 10 * K)
    z, jac = S.forward(x, h, K, T)
    assert (jac > 0).all()
    outside = (x < -T) | (x > T)
    assert 0 < int(outside.sum()) < x.numel()
    assert torch.equal(z[outside], x[outside]) and bool((jac[outside] == 1).all())
    assert float((S.inverse(z, h, K, T) - x).abs().max()) <= 1e-10
    assert float((S.forward(S.inverse(x, h, K, T), h, K, T)[0] - x).abs().max()) <= 1e-10


@pytest.mark.parametrize("K", BINS)
def test_jac_is_dz_dx(K):
    x, h = _case(K, 3., 7 + K)
    x.requires_grad_(True)
    z, jac = S.forward(x, h, K, 3.)
    dz, = torch.autograd.grad(z.sum(), x)
    jac = jac.detach()
    assert float((dz - jac).abs().max()) <= 1e-10 * float(jac.abs().max())


@pytest.mark.parametrize("K", BINS)
@pytest.mark.parametrize("T", (3., .5))
def test_continuous_across_knots_and_tails(K, T):
    _, h = _case(K, T, 3 * K, n=64)
    X, _, _ = S.knots(h, K, T)
    dl = 1e-9
    for j in (0, max(1, K // 2), K):                             # -T, an interior knot, T
        at = X[:, j]
        side = []
        for sgn in (-1., 1.):
            p = (at + sgn * dl).requires_grad_(True)
            z, jac = S.forward(p, h, K, T)
            dj, = torch.autograd.grad(jac.sum(), p)
            side.append((z.detach(), jac.detach(), dj))
        (zl, jl, dl_), (zr, jr, dr) = side
        # the two points lie 2e-9 apart on a map of slope jac (and jac of slope d jac/dx): each side is carried to the knot
        # along its own branch (first order; the second-order terms are 1e-18 times a curvature), what is left is the JUMP
        assert float((zr - dl * jr - (zl + dl * jl)).abs().max()) <= 1e-9, j
        assert float((jr - dl * dr - (jl + dl * dl_)).abs().max()) <= 1e-9, j


def test_ignores_components_beyond():
    x, h = _case(5, 3., 1)
    wide = torch.cat((h, torch.randn(h.shape[0], 2, dtype=torch.float64)), 1)
    assert torch.equal(S.forward(x, h, 5, 3.)[0], S.forward(x, wide, 5, 3.)[0])
    assert torch.equal(S.inverse(x, h, 5, 3.), S.inverse(x, wide, 5, 3.))


def test_to_bin_middles_removes_the_knife_edge():
    K, T = 8, 3.
    x, h = _case(K, T, 5, n=4000)
    x, h = x.float(), h.float()
    X, _, _ = S.knots(h.double(), K, T)
    x[:50] = X[:50, 3].float()                                   # on a knot, up to fp32 rounding
    x[50] = T
    x[51] = -T
    assert int((S.knot_distance(x.double(), h.double(), K, T) < 1e-4).sum()) >= 52
    moved = S.to_bin_middles(x, h, K, T)
    assert int((S.knot_distance(moved.double(), h.double(), K, T) < 1e-4).sum()) == 0
    far = S.knot_distance(x.double(), h.double(), K, T) >= 1e-4
    assert torch.equal(moved[far], x[far])


# ------------------------------------------------------------------------------------------------------- the C ABI
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
    assert "#define GNF_MADE_NORM_SPLINE 2" in header and abi.MADE_NORM_SPLINE == 2
    assert "gnf_spline.hip" in build.SOURCES


def _fwd(lib, K, T, hc, B, p, d=3):
    return lib.gnf_spline_fwd(p, p, d * hc, hc, 1, hc, K, T, p, p, p, p, B, d, None)


def _bwd(lib, K, T, hc, B, p, d=3):
    return lib.gnf_spline_bwd(p, p, d * hc, hc, 1, hc, K, T, p, p, p, p, p, p, d * hc, hc, 1, B, d, None)


def _inv(lib, K, T, hc, B, p, d=3):
    return lib.gnf_spline_inv(p, p, d * hc, hc, 1, hc, K, T, p, None, 0, B, d, None)


@pytest.mark.parametrize("entry", (_fwd, _bwd, _inv), ids=("fwd", "bwd", "inv"))
def test_argument_checks_answer_before_any_launch(entry):
    from gnf_hip import abi
    lib = abi.load()
    p = ctypes.c_void_p(64)                                      # never dereferenced: every call below is refused or empty
    assert entry(lib, 1, 3., 23, 4, p) == -1                     # K = 1
    assert entry(lib, 33, 3., 98, 4, p) == -1                    # K = 33
    assert entry(lib, 8, 0., 23, 4, p) == -1                     # T <= 0
    assert entry(lib, 8, -1., 23, 4, p) == -1
    assert entry(lib, 8, float("nan"), 23, 4, p) == -1
    assert entry(lib, 8, 3., 22, 4, p) == -2                     # h too narrow: GNF_ESHAPE
    assert entry(lib, 8, 3., 23, -1, p) == -1                    # B < 0
    assert entry(lib, 8, 3., 23, 4, p, d=0) == -1
    assert entry(lib, 8, 3., 23, 4, None) == -1                  # NULL with B > 0
    assert entry(lib, 8, 3., 23, 0, None) == 0                   # B = 0 with NULLs
    assert entry(lib, 32, .5, 95, 0, None) == 0


def test_scatter_form_argument_checks():
    from gnf_hip import abi
    lib = abi.load()
    p = ctypes.c_void_p(64)
    assert lib.gnf_spline_inv(p, p, 69, 23, 1, 23, 8, 3., p, p, 0, 4, 3, None) == -1     # columns without a width
    assert lib.gnf_spline_inv(None, None, 69, 23, 1, 23, 8, 3., None, None, 0, 0, 3, None) == 0


def _host_net(d, widths, out, max_new=1):
    """a gnf_made_net whose pointers are never dereferenced (the refused calls read the integers only)"""
    from gnf_hip import abi
    net = abi.MadeNet()
    net.nh, net.d, net.out, net.max_new = len(widths), d, out, max_new
    for l, w in enumerate(widths):
        net.width[l] = w
        net.order[l] = net.off[l] = 64
    for l in range(len(widths) + 1):
        net.W[l] = net.b[l] = 64
    net.var_of_step = 64
    return net


def test_prefix_entry_points():
    from gnf_hip import abi
    lib = abi.load()
    p = ctypes.c_void_p(64)
    net = _host_net(5, [7, 7], 14)
    ref = ctypes.byref(net)
    SPL = abi.MADE_NORM_SPLINE
    # the entry points from before the spline still refuse the mode
    assert lib.gnf_made_prefix(ref, p, p, p, p, 0, 5, SPL, 4, p, 1 << 20, None) == -1
    assert lib.gnf_made_prefix_ctx(ref, 2, p, p, p, p, p, 0, 5, SPL, 4, p, 1 << 20, None) == -1
    # the new ones check the spline's own arguments
    assert lib.gnf_made_prefix_spline(ref, p, p, p, p, 0, 5, SPL, 1, 3., 4, p, 1 << 20, None) == -1
    assert lib.gnf_made_prefix_spline(ref, p, p, p, p, 0, 5, SPL, 33, 3., 4, p, 1 << 20, None) == -1
    assert lib.gnf_made_prefix_spline(ref, p, p, p, p, 0, 5, SPL, 5, 0., 4, p, 1 << 20, None) == -1
    assert lib.gnf_made_prefix_spline(ref, p, p, p, p, 0, 5, SPL, 6, 3., 4, p, 1 << 20, None) == -2      # out = 14 < 17
    assert lib.gnf_made_prefix_spline(ref, p, p, p, p, 0, 5, 7, 5, 3., 4, p, 1 << 20, None) == -1        # unknown mode
    assert lib.gnf_made_prefix_spline(ref, p, None, p, p, 0, 5, SPL, 5, 3., 4, p, 1 << 20, None) == -1   # no z
    assert lib.gnf_made_prefix_ctx_spline(ref, 2, None, p, p, p, p, 0, 5, SPL, 5, 3., 4, p, 1 << 20, None) == -1  # no context
    assert lib.gnf_made_prefix_spline(ref, None, None, None, None, 0, 5, SPL, 5, 3., 0, None, 0, None) == 0    # B = 0
    assert lib.gnf_made_prefix_ctx_spline(ref, 2, None, None, None, None, None, 2, 2, SPL, 5, 3., 4, None, 0, None) == 0
    assert lib.gnf_made_prefix_spline(ref, p, p, p, p, 1, 2, SPL, 5, 3., 4, None, 0, None) == -3         # a step needs ws


# ------------------------------------------------------------------------------------------------------- Python
def test_no_cpu_fallback():
    from gnf_hip import abi
    from models import SplineNormalizer
    from models.Normalizers import SplineNormalizer as same
    assert same is SplineNormalizer
    norm = SplineNormalizer()
    assert norm.nb_bins == 8 and norm.tail_bound == 3. and len(norm.state_dict()) == 0
    x, h = torch.randn(4, 3), torch.randn(4, 3, 23)
    for call in (lambda: norm(x, h), lambda: norm.forward_logdet(x, h), lambda: norm.inverse_transform(x, h)):
        with pytest.raises(abi.GnfError):
            call()
    with pytest.raises(ValueError):
        norm(x, torch.randn(4, 3, 22))                           # too narrow: answered before the device is asked
    with pytest.raises(ValueError):
        norm.inverse_transform(x, torch.randn(4, 3, 22))
    for bad in ({"nb_bins": 1}, {"nb_bins": 33}, {"tail_bound": 0.}):
        with pytest.raises(ValueError):
            SplineNormalizer(**bad)


def test_h_size_and_factories():
    from models import SplineNormalizer, AffineNormalizer, MonotonicNormalizer
    from models import NormalizingFlowFactories as F
    assert SplineNormalizer.h_size() == 23 and SplineNormalizer.h_size(nb_bins=5, tail_bound=1.) == 14
    assert F._emb_size(SplineNormalizer, {}, 2) == 23
    assert F._emb_size(SplineNormalizer, {"nb_bins": 4}, 2) == 11
    assert F._emb_size(AffineNormalizer, {}, 2) == 2 and F._emb_size(MonotonicNormalizer, {"integrand_net": [8]}, 30) == 30
    steps = F._mnist_dag_steps(1, [1, 7, 7], [16, 16], SplineNormalizer, {"nb_bins": 8}, 0., 10, False, None)
    assert steps[0].conditioner.embedding_net.out_d == 23 and isinstance(steps[0].normalizer, SplineNormalizer)
    steps = F._cifar_dag_steps(1, [1, 8, 8], [16, 32, 32], 2, SplineNormalizer, {}, 0., 5)
    assert steps[0].conditioner.embedding_net.out_d == 23
    for norm_t, nargs, want in ((AffineNormalizer, {}, 2),):
        assert F._mnist_dag_steps(1, [1, 7, 7], [16, 16], norm_t, nargs, 0., 10, False, None)[0] \
            .conditioner.embedding_net.out_d == want
        assert F._cifar_dag_steps(1, [1, 8, 8], [16, 32, 32], 2, norm_t, nargs, 0., 5)[0].conditioner.embedding_net.out_d == want


def test_train_uci_argument_error():
    import train_uci
    args = train_uci.parse(["-dataset", "power", "-conditioner", "Autoregressive", "-normalizer", "spline",
                            "-emb_net", "60", "60", "22"])
    assert args.spline_bins == 8 and args.spline_tail == 3.
    with pytest.raises(ValueError, match="23"):
        train_uci.build(args, 6)
    args = train_uci.parse(["-dataset", "power", "-conditioner", "Autoregressive", "-normalizer", "spline",
                            "-emb_net", "60", "60", "23"])
    model, _, norm_t = train_uci.build(args, 6)
    assert norm_t.__name__ == "SplineNormalizer" and model.getNormalizers()[0].nb_bins == 8
    args = train_uci.parse(["-dataset", "power", "-conditioner", "Coupling", "-normalizer", "spline", "-spline_bins", "5",
                            "-spline_tail", "2.5", "-emb_net", "30", "14"])
    model, _, _ = train_uci.build(args, 6)
    assert model.getNormalizers()[0].nb_bins == 5 and model.getNormalizers()[0].tail_bound == 2.5
