"""train_image.py on CIFAR-10.  CPU part: the two file readers (on fabricated files), the restricted unpickler, the
synthetic images, the refusal without data, model construction for -dataset CIFAR10, prepare_reference (the torch statement
of the batch preparation) against an independent fp64 numpy evaluation, and the PPM writer.  GPU part (-m gpu): one epoch of
the one-scale and of the four-scale model on synthetic images, sampling behind an installed DAG, resuming, and MNIST through
the preparation kernel."""
import math
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close

PKG = os.path.join(ROOT, "graphical-normalizing-flows_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

NAMES = ["data_batch_%d" % k for k in range(1, 6)] + ["test_batch"]


def _driver():
    import train_image
    return train_image


def _records(seed, n=6):
    g = np.random.default_rng(seed)
    return g.integers(0, 10, n, dtype=np.uint8), g.integers(0, 256, (n, 3072), dtype=np.uint8)


# ----------------------------------------------------------------------------- readers
def test_binary_reader_on_fabricated_files(tmp_path):
    T = _driver()
    d = tmp_path / "cifar-10-batches-bin"
    d.mkdir()
    pix = []
    for k, name in enumerate(NAMES):
        lab, p = _records(k)
        pix.append(p)
        (d / (name + ".bin")).write_bytes(np.concatenate([lab[:, None], p], 1).tobytes())
    trn, val, tst = T.load_cifar10(str(tmp_path), torch.Generator().manual_seed(0))
    assert trn.dtype == val.dtype == tst.dtype == torch.uint8
    assert trn.shape == (30, 3072) and val.shape == tst.shape == (6, 3072)
    assert np.array_equal(trn.numpy(), np.concatenate(pix[:5])) and np.array_equal(tst.numpy(), pix[5])
    assert torch.equal(val, tst)                                   # reference :106-108, "WARNING VALID = TEST"
    raw = (d / "data_batch_3.bin").read_bytes()
    (d / "data_batch_3.bin").write_bytes(raw[:-5])                 # a truncated record
    with pytest.raises(ValueError, match="records"):
        T.load_cifar10(str(tmp_path), torch.Generator())


def test_pickle_reader_admits_arrays_only(tmp_path, monkeypatch):
    T = _driver()
    d = tmp_path / "cifar-10-batches-py"
    d.mkdir()
    pix = []
    for k, name in enumerate(NAMES):
        lab, p = _records(10 + k)
        pix.append(p)
        with open(d / name, "wb") as f:                            # the keys are bytes, as in the files of the data set
            pickle.dump({b"batch_label": b"batch", b"labels": lab.tolist(), b"data": p, b"filenames": [b"a.png"] * 6}, f,
                        protocol=(2, 3, 4, 5, 2, 4)[k])            # every way numpy has pickled an array
    trn, val, tst = T.load_cifar10(str(tmp_path), torch.Generator().manual_seed(0))
    assert trn.shape == (30, 3072) and trn.dtype == torch.uint8
    assert np.array_equal(trn.numpy(), np.concatenate(pix[:5])) and np.array_equal(val.numpy(), pix[5])
    # a batch file that names any other global is refused before the global is looked up, let alone called
    called = []
    monkeypatch.setattr(os, "getcwd", lambda: called.append(1) or "/")
    (d / "data_batch_2").write_bytes(b"cos\ngetcwd\n(tR.")            # GLOBAL os.getcwd, MARK, TUPLE, REDUCE, STOP
    with pytest.raises(pickle.UnpicklingError, match="not allowed"):
        T.load_cifar10(str(tmp_path), torch.Generator())
    assert not called


def test_synthetic_root_and_missing_directory(tmp_path):
    T = _driver()
    trn, val, tst = T.load_cifar10("synthetic", torch.Generator().manual_seed(3))
    assert trn.shape == (24, 3072) and val.shape == tst.shape == (8, 3072)
    assert trn.dtype == val.dtype == tst.dtype == torch.uint8
    img = trn.view(24, 3, 32, 32).float()
    assert (img[..., 1:] - img[..., :-1]).abs().mean() < 20. < img.std()            # smooth, not noise
    one = T.synthetic_cifar(5, torch.Generator().manual_seed(1))
    assert one.shape == (5, 3072) and torch.equal(one, T.synthetic_cifar(5, torch.Generator().manual_seed(1)))
    with pytest.raises(SystemExit, match="CIFAR10"):
        T.load_cifar10(str(tmp_path / "nowhere"), torch.Generator())
    with pytest.raises(SystemExit, match="CIFAR10.*not found under.*synthetic"):     # before the GPU check, on any box
        T.train(T.parse(("-dataset CIFAR10 -data_root %s -folder %s" % (tmp_path, tmp_path / "run")).split()))


# ----------------------------------------------------------------------------- build()
def test_build_for_cifar10():
    T = _driver()
    from models import DAGConditioner, CouplingConditioner, MonotonicNormalizer, AffineNormalizer
    from models.MLP import CIFAR10CNN
    from models.NormalizingFlow import FCNormalizingFlow, CNNormalizingFlow
    model, cond_t, norm_t = T.build(T.parse("-dataset CIFAR10 -nb_flow 1 -nb_steps_dual 7".split()))
    assert type(model) is FCNormalizingFlow and cond_t is DAGConditioner and norm_t is AffineNormalizer
    cond = model.getConditioners()[0]
    assert cond.in_size == 3072 and type(cond.embedding_net) is CIFAR10CNN and cond.nb_epoch_update == 7
    assert T.image_shape(model) == (3, 32, 32)
    nets = [m for m in model.modules() if isinstance(m, CIFAR10CNN)]
    fresh = CIFAR10CNN()
    assert all(n.gated_front == fresh.gated_front and n.rows_train_front == fresh.rows_train_front for n in nets)
    sd = model.state_dict()
    w = T.wrapped_keys(sd)
    assert all(k.startswith("module.") for k in w) and set(T.plain_keys(w)) == set(sd)

    four, _, _ = T.build(T.parse("-dataset CIFAR10 -nb_flow 1 1 1 1 -gated_front -rows_train_front".split()))
    assert type(four) is CNNormalizingFlow and len(four.steps) == 4
    nets = [m for m in four.modules() if isinstance(m, CIFAR10CNN)]
    assert len(nets) == 4 and all(n.gated_front is True and n.rows_train_front is True for n in nets)
    with pytest.raises(SystemExit, match="1 or 4"):
        T.build(T.parse("-dataset CIFAR10 -nb_flow 1 1".split()))

    mono, _, norm_t = T.build(T.parse("-dataset CIFAR10 -normalizer Monotonic -no_hot_encoding".split()))
    assert norm_t is MonotonicNormalizer
    assert mono.getNormalizers()[0].integrand_net.net[0].in_features == 1 + 30       # cond_size the reference omits
    assert mono.getConditioners()[0].embedding_net.out_d == 30

    coup, cond_t, _ = T.build(T.parse("-dataset CIFAR10 -conditioner Coupling -emb_net 16 16 4".split()))
    assert cond_t is CouplingConditioner and coup.getConditioners()[0].in_size == 3072
    mnist, _, _ = T.build(T.parse([]))                                               # the MNIST branch is as it was
    assert mnist.getConditioners()[0].in_size == 784 and T.image_shape(mnist) == (1, 28, 28)


def test_new_switches_default_off():
    T = _driver()
    a = T.parse([])
    assert a.device_prep is False and a.gated_front is False and a.rows_train_front is False and a.data_root == "."
    a = T.parse("-dataset CIFAR10 -device_prep -gated_front".split())
    assert a.device_prep and a.gated_front and not a.rows_train_front


# ----------------------------------------------------------------------------- prepare_reference, write_ppm
def _numpy_prepare(u8, rows, flip, u, alpha, size_img):
    """independent fp64 evaluation: explicit loops over rows, numpy indexing for the flip, 1 - y by subtraction"""
    c, h, w = size_img
    out_x, out_t = [], []
    for b, r in enumerate(rows):
        img = u8[r].reshape(c, h, w).astype(np.float64)
        if flip[b]:
            img = img[:, :, ::-1]
        y = alpha + (1. - 2. * alpha) * (img.reshape(-1) + u[b].astype(np.float64)) / 256.
        out_x.append(np.log(y / (1. - y)))
        out_t.append((np.log2(y) + np.log2(1. - y)).sum())
    return np.stack(out_x), np.array(out_t)


@pytest.mark.parametrize("alpha", [1e-6, .05])
def test_prepare_reference_against_numpy(alpha):
    T = _driver()
    g = torch.Generator().manual_seed(5)
    size = (3, 5, 7)
    u8 = torch.randint(0, 256, (7, 105), generator=g).to(torch.uint8)
    u8[0], u8[1] = 0, 255
    rows = torch.tensor([4, 1, 0, 6, 1])
    flip = torch.tensor([1, 0, 1, 0, 1], dtype=torch.uint8)
    u = torch.rand(5, 105, generator=g)
    want_x, want_t = _numpy_prepare(u8.numpy(), rows.tolist(), flip.tolist(), u.numpy(), alpha, size)
    x, t = T.prepare_reference(u8, rows, flip, u, alpha, size, torch.float64)
    assert x.dtype == torch.float64 and x.shape == (5, 105) and t.shape == (5,)
    # (the subtraction of the numpy form costs 1e-16 / (1 - y) <= 1e-10 relative at alpha = 1e-6)
    assert_close(x, torch.from_numpy(want_x), rtol=1e-9, atol=1e-12, what="x, fp64")
    assert_close(t, torch.from_numpy(want_t), rtol=1e-12, atol=0., what="bpp_term, fp64")
    x32, t32 = T.prepare_reference(u8, rows, flip, u, alpha, size, torch.float32)
    assert x32.dtype == torch.float32
    assert_close(x32, torch.from_numpy(want_x), rtol=1e-5, atol=1e-6, what="x, fp32")        # white pixels included
    assert_close(t32, torch.from_numpy(want_t), rtol=1e-5, atol=0., what="bpp_term, fp32")
    # rows None: every row in order; flip None: nowhere
    x0, t0 = T.prepare_reference(u8[:5], None, None, u, alpha, size, torch.float64)
    x1, t1 = T.prepare_reference(u8, torch.arange(5), torch.zeros(5, dtype=torch.uint8), u, alpha, size, torch.float64)
    assert torch.equal(x0, x1) and torch.equal(t0, t1) and torch.equal(x0[1], x[1]) and not torch.equal(x0[0], x[0])


def test_uniform_data_costs_eight_bits_at_alpha_05():
    """a density that is uniform on the pixel cube has, after the change of variables of the preparation,
    log p(x) = sum_d log(y (1 - y)) - d log(1 - 2 alpha); the formula must give exactly 8 bits per pixel for it (the
    identity tests/test_image_driver.py checks for compute_bpp at alpha = 1e-6)"""
    T = _driver()
    g = torch.Generator().manual_seed(2)
    alpha, size = .05, (3, 32, 32)
    u8 = torch.randint(0, 256, (6, 3072), generator=g).to(torch.uint8)
    u8[0], u8[1] = 0, 255
    x, term = T.prepare_reference(u8, None, None, torch.rand(6, 3072, generator=g), alpha, size, torch.float32)
    ll_uniform = term * math.log(2.) - 3072 * math.log(1. - 2. * alpha)
    assert_close(T.bpp_from_term(ll_uniform, term, 3072, alpha), torch.full((6,), 8.), rtol=1e-6, atol=0., what="8 bpp")
    assert_close(T.compute_bpp(ll_uniform, x, alpha), torch.full((6,), 8.), rtol=1e-5, atol=1e-4, what="8 bpp, from x")


def test_ppm_grid_file(tmp_path):
    T = _driver()
    x = torch.linspace(0, 1, 16 * 3072).view(16, 3072)
    T.write_ppm(str(tmp_path / "g.ppm"), x)
    raw = (tmp_path / "g.ppm").read_bytes()
    head = b"P6\n128 128\n255\n"
    assert raw.startswith(head) and len(raw) == len(head) + 128 * 128 * 3
    # image 5 sits at grid row 1, column 1; its pixel (c, h, w) = (2, 3, 4) is byte ((32 + 3) * 128 + 32 + 4) * 3 + 2
    want = int((x[5, 2 * 1024 + 3 * 32 + 4] * 255).round())
    assert raw[len(head) + ((32 + 3) * 128 + 32 + 4) * 3 + 2] == want


# ----------------------------------------------------------------------------- GPU
DEV = "cuda:0"
SMALL = "-dataset CIFAR10 -data_root synthetic -normalizer Affine -b_size 2 -nb_epoch 1 -nb_steps_dual 1 -l1 0.1"


def _epoch_lines(run):
    lines = open(run / "logs").read().splitlines()
    return lines, [l for l in lines if l.startswith("epoch:") and "Train loss" in l]


@pytest.mark.gpu
def test_one_scale_epoch_sampling_and_resume(tmp_path):
    T = _driver()
    run = tmp_path / "run"
    model = T.train(T.parse((SMALL + " -max_batches 2 -folder %s" % run).split()))
    lines, ep = _epoch_lines(run)
    assert len(ep) == 1 and math.isfinite(float(ep[0].split("Valid BPP ")[1].split(" ")[0])), ep
    assert sum("Threshold:" in l for l in lines) == 5
    sd = torch.load(run / "model.pt", map_location="cpu")
    assert all(k.startswith("module.") for k in sd) and os.path.exists(run / "ADAM.pt")
    for c in model.getConditioners():
        assert c.stoch_gate and c.h_thresh == 0.                   # the sweep restored the gate settings
    # a DAG of 8 levels: block-diagonal, strictly lower-triangular inside blocks of 8
    idx = torch.arange(3072, device=DEV)
    A = ((idx[:, None] // 8 == idx[None, :] // 8) & (idx[:, None] > idx[None, :])).float()
    with torch.no_grad():
        for c in model.getConditioners():
            c.A.copy_(A)
            c.post_process(.1)
            c.is_invertible = True
    assert model.isInvertible() and len(model.getConditioners()[0].levels()) == 8
    said = []
    T.sample_grids(model, torch.device(DEV), .05, 3, str(run), said.append)
    assert len(said) == 5 and all(math.isfinite(float(l.split("| ")[-1])) for l in said), said
    assert os.path.getsize(run / ("images_3_%f.ppm" % .25)) == len(b"P6\n128 128\n255\n") + 128 * 128 * 3
    with torch.no_grad():
        u8 = T.synthetic_cifar(2, torch.Generator().manual_seed(9)).to(DEV)
        x = T.DevicePrep(0, .05, T.CIFAR_IMG)(u8)[0]
        assert (model.invert(model(x)[0]) - x).abs().max().item() < 2e-3
    T.train(T.parse(("-load " + SMALL + " -max_batches 1 -folder %s" % run).split()))
    assert len(_epoch_lines(run)[1]) == 2


@pytest.mark.gpu
def test_four_scale_epoch(tmp_path):
    T = _driver()
    run = tmp_path / "run"
    T.train(T.parse((SMALL + " -nb_flow 1 1 1 1 -max_batches 1 -folder %s" % run).split()))
    lines, ep = _epoch_lines(run)
    assert len(ep) == 1 and math.isfinite(float(ep[0].split("Valid BPP ")[1].split(" ")[0])), ep
    assert not any(l.startswith("epoch:") and " - T " in l for l in lines)           # not invertible yet: no sampling


@pytest.mark.gpu
def test_mnist_through_the_preparation_kernel(tmp_path):
    T = _driver()
    run = tmp_path / "run"
    T.train(T.parse(("-dataset MNIST -data_root synthetic -device_prep -normalizer Affine -no_hot_encoding -prior_A_kernel 2 "
                     "-b_size 4 -nb_epoch 1 -max_batches 2 -nb_steps_dual 1 -l1 0.1 -folder %s" % run).split()))
    _, ep = _epoch_lines(run)
    assert len(ep) == 1 and math.isfinite(float(ep[0].split("Valid BPP ")[1].split(" ")[0])), ep


@pytest.mark.gpu
def test_bpp_of_a_white_row_without_the_cancellation():
    """an all-255 row at alpha = 1e-6: compute_bpp forms 1 - sigmoid(x) in fp32 (7e-5 bpp off, the 2e-4 the existing driver
    test allows); the kernel's bpp_term comes from y and 1 - y themselves and must be closer to the fp64 value"""
    T = _driver()
    alpha = 1e-6
    u8 = torch.full((2, 784), 255, dtype=torch.uint8, device=DEV)
    x, term = T.DevicePrep(0, alpha, T.MNIST_IMG)(u8, want_bpp=True)
    ll = torch.full((2,), -1500., device=DEV)
    s = torch.sigmoid(x.double())
    want = (-ll.double() / (784 * math.log(2.)) - math.log2(1. - 2. * alpha) + 8.
            + (torch.log2(s) + torch.log2(1. - s)).sum(1) / 784)
    err_kernel = (T.bpp_from_term(ll, term, 784, alpha).double() - want).abs().max().item()
    err_torch = (T.compute_bpp(ll, x, alpha).double() - want).abs().max().item()
    print("bpp error of a white row: kernel term %.3e, compute_bpp %.3e" % (err_kernel, err_torch))
    assert err_kernel < err_torch
    assert err_kernel < 2e-5                  # what the existing driver test asks of compute_bpp on UNsaturated rows
