"""CPU (-m "not gpu"): the CIFAR-10 side of the drop-in contract -- the reference image driver's import line resolves,
buildCIFAR10NormalizingFlow builds the reference's layouts from this package's classes, the functional restatement the
GPU tests judge the kernels by (tests/lenet_ref.py) agrees with the reference fixture, and the new C-ABI calls are
declared on both sides of the binding."""
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden
import lenet_ref

IMG_SIZES = [[3, 32, 32], [1, 32, 32], [1, 16, 16], [1, 8, 8]]
FC_L = [[400, 128, 84], [576, 128, 32], [64, 32, 32], [16, 32, 32]]
K_SIZES = [5, 3, 3, 2]
LENET_SYMBOLS = ("gnf_lenet_conv_supported", "gnf_lenet_conv_feat", "gnf_lenet_conv_fwd", "gnf_lenet_conv_bwd_ws_bytes",
                 "gnf_lenet_conv_bwd")


@pytest.fixture(scope="module")
def golden():
    return load_golden("cifar10cnn")


@pytest.fixture(scope="module")
def flows():
    from models import AffineNormalizer
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow
    torch.manual_seed(0)
    return (buildCIFAR10NormalizingFlow([1], AffineNormalizer, {}),
            buildCIFAR10NormalizingFlow([1, 1, 1, 1], AffineNormalizer, {}))


def test_reference_image_driver_import_line():
    """ImageExperiments.py:14 and ImageExperimentsTest.py:10 of the reference, verbatim"""
    from models.NormalizingFlowFactories import buildMNISTNormalizingFlow, buildCIFAR10NormalizingFlow, buildFCNormalizingFlow
    assert callable(buildMNISTNormalizingFlow) and callable(buildCIFAR10NormalizingFlow) and callable(buildFCNormalizingFlow)
    import models
    assert "buildCIFAR10NormalizingFlow" not in models.__all__          # the reference does not export it there either


def test_state_dict_keys_equal_the_reference(golden, flows):
    one, four = flows
    assert list(one.state_dict().keys()) == [str(k) for k in golden["keys1"]]
    assert list(four.state_dict().keys()) == [str(k) for k in golden["keys4"]]


def _check_step(step, size_img, fc_l, k, emb):
    from models import DAGConditioner, AffineNormalizer
    from models.MLP import CIFAR10CNN
    cond = step.conditioner
    d = size_img[0] * size_img[1] * size_img[2]
    assert type(cond) is DAGConditioner and cond.in_size == d and tuple(cond.A.shape) == (d, d)
    assert cond.nb_epoch_update == 5 and float(cond.l1_weight) == 0. and not cond.hot_encoding
    net = cond.embedding_net
    assert type(net) is CIFAR10CNN and list(net.size_img) == size_img and net.out_d == emb
    assert tuple(net.conv1.weight.shape) == (6, size_img[0], k, k) and tuple(net.conv2.weight.shape) == (16, 6, k, k)
    assert [net.fc1.in_features, net.fc1.out_features, net.fc2.out_features, net.fc3.out_features] == fc_l + [emb]
    assert type(step.normalizer) is AffineNormalizer


def test_one_scale_branch(flows):
    from models.NormalizingFlow import FCNormalizingFlow, CNNormalizingFlow
    from models.NormalizingFlowFactories import NormalLogDensity
    one, _ = flows
    assert type(one) is FCNormalizingFlow and not isinstance(one, CNNormalizingFlow) and len(one.steps) == 1
    assert type(one.z_log_density) is NormalLogDensity
    _check_step(one.steps[0], IMG_SIZES[0], FC_L[0], K_SIZES[0], 2)
    # no A_prior: the default initialisation 1.5 + 0.02 randn, every off-diagonal entry present
    A = one.steps[0].conditioner.A.detach()
    assert int((A != 0).sum()) >= 3072 * 3071 and float(A.max()) < 2.


def test_four_scale_branch_four_flows_three_factors(flows):
    from models.NormalizingFlow import FCNormalizingFlow, CNNormalizingFlow
    _, four = flows
    assert type(four) is CNNormalizingFlow and len(four.steps) == 4
    assert [list(f) for f in four.dropping_factors] == [[3, 1, 1], [1, 2, 2], [1, 2, 2]]
    for flow, size_img, fc_l, k in zip(four.steps, IMG_SIZES, FC_L, K_SIZES):
        assert type(flow) is FCNormalizingFlow and flow.z_log_density is None and list(flow.img_sizes) == size_img
        assert len(flow.steps) == 1
        _check_step(flow.steps[0], size_img, fc_l, k, 2)


def test_embedding_width_and_normalizer_arguments():
    """emb_s = 30 for anything but Affine, and the normalizer is built from normalizer_args ALONE: a Monotonic caller passes
    cond_size itself, as it must with the reference (:115, :129)"""
    from models import MonotonicNormalizer
    from models.NormalizingFlowFactories import _cifar_dag_steps
    args = {"integrand_net": [50, 50, 50], "cond_size": 30, "nb_steps": 15, "solver": "CC"}
    step, = _cifar_dag_steps(1, [1, 8, 8], [16, 32, 32], 2, MonotonicNormalizer, args, 0., 5)
    assert step.conditioner.embedding_net.out_d == 30 and type(step.normalizer) is MonotonicNormalizer
    with pytest.raises(TypeError):
        _cifar_dag_steps(1, [1, 8, 8], [16, 32, 32], 2, MonotonicNormalizer, {"integrand_net": [50, 50, 50]}, 0., 5)


def test_other_lengths_give_none():
    from models import AffineNormalizer
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow
    assert buildCIFAR10NormalizingFlow([1, 1], AffineNormalizer, {}) is None
    assert buildCIFAR10NormalizingFlow([1, 1, 1], AffineNormalizer, {}) is None


@pytest.mark.parametrize("gi", range(4))
def test_lenet_ref_equals_the_reference_fixture(golden, gi):
    """the restatement in fp32 against the reference's own CIFAR10CNN: 2e-6, the oracle-vs-golden bound of
    test_oracle_golden.py, on the output and on every gradient; and the fixture inputs hold no knife-edge decision"""
    size_img, k, _ = lenet_ref.GEOMETRIES[gi]
    tag = "g%d." % gi
    p = {n[len(tag) + 2:]: v.clone().requires_grad_(True) for n, v in golden.items() if n.startswith(tag + "p.")}
    x = golden[tag + "x"].clone().requires_grad_(True)
    assert not bool(lenet_ref.knife_images(x, p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"],
                                           size_img).any())
    out = lenet_ref.cifar10cnn(x, p, size_img)
    (out * golden[tag + "g"]).sum().backward()

    def err(a, b):
        return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))
    assert err(out.detach(), golden[tag + "out"]) < 2e-6
    assert err(x.grad, golden[tag + "gx"]) < 2e-6
    for n, v in p.items():
        assert err(v.grad, golden[tag + "g." + n]) < 2e-6, n


def test_knife_finder_flags_constructed_edges():
    """a pre-activation one fp32 ulp above zero is a ReLU knife; an exactly zero one and an exact pool tie are not"""
    size_img = (1, 8, 8)
    W1 = torch.zeros(6, 1, 2, 2)
    W1[:, 0, 0, 0] = 1.
    b1 = torch.full((6,), -1.)
    W2, b2 = torch.zeros(16, 6, 2, 2), torch.zeros(16)
    e = torch.ones(3, 64)                                   # pre1 = 1 - 1 = 0 exactly, everywhere; all windows tied
    e[1, 9] = 1. + 2. ** -22                                # pre1 = 2^-22 at one position: within 16 ulps of |b| + |w a| = 2
    e[2, 9] = 1.5                                           # a decided gate and a decided pool window
    flagged = lenet_ref.knife_images(e, W1, b1, W2, b2, size_img)
    assert flagged.tolist() == [False, True, False]


def test_new_abi_symbols_declared_on_both_sides():
    from gnf_hip import abi
    header = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in LENET_SYMBOLS:
        assert name in abi.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert abi.ABI_VERSION == 11 and "#define GNF_ABI_VERSION 11" in header
    lib = abi.load()                                        # the host side of these calls works without a GPU
    feats = [lib.gnf_lenet_conv_feat(s[0], s[1], s[2], k) for s, k, _ in lenet_ref.GEOMETRIES]
    assert feats == [400, 576, 64, 16]
    assert all(lib.gnf_lenet_conv_supported(s[0], s[1], s[2], k) == 1 for s, k, _ in lenet_ref.GEOMETRIES)
    assert lib.gnf_lenet_conv_supported(3, 28, 28, 5) == 0 and lib.gnf_lenet_conv_supported(1, 32, 32, 4) == 0
    assert lib.gnf_lenet_conv_feat(3, 28, 28, 5) == -2 and lib.gnf_lenet_conv_bwd_ws_bytes(1, 32, 32, 4, 8) == -2


def test_cnn_invert_uses_the_flows_forward_uses():
    """CPU-checkable part of CNNormalizingFlow.invert: with more flows than dropping factors, and a last active factor
    that still drops, the z layout is sliced for the active flows only and the tail is handed on as the coarsest block"""
    from models.NormalizingFlow import CNNormalizingFlow

    class Shift(torch.nn.Module):                           # an invertible stand-in for an FCNormalizingFlow scale
        def __init__(self, img_sizes, c):
            super().__init__()
            self.img_sizes, self.c = img_sizes, c

        def forward(self, x, context=None):
            return x * 2. + self.c, torch.full((x.shape[0],), 0.6931471805599453 * x.shape[1])

        def invert(self, z, context=None):
            return (z - self.c) / 2.

    flow = CNNormalizingFlow([Shift([1, 4, 4], 1.), Shift([1, 2, 2], -3.), Shift([1, 1, 1], 7.)], None,
                             [[1, 2, 2], [1, 2, 2]])
    x = torch.arange(32.).view(2, 16) / 7.
    z, ld = flow(x)
    assert z.shape == (2, 16) and torch.allclose(ld, torch.full((2,), 0.6931471805599453 * 20))
    assert torch.allclose(flow.invert(z), x, atol=1e-6)
    # equal lengths, last factor [1, 1, 1]: the case every existing caller has
    flow3 = CNNormalizingFlow([Shift([1, 4, 4], 1.), Shift([1, 2, 2], -3.)], None, [[1, 2, 2], [1, 1, 1]])
    z3, _ = flow3(x)
    assert torch.allclose(flow3.invert(z3), x, atol=1e-6)
