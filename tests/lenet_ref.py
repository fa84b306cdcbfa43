"""Functional torch restatement of CIFAR10CNN (reference models/MLP.py:51-72) and of its convolutional front, in whatever
dtype the operands have (fp32 against the reference fixture, fp64 as the arbiter of the kernels), plus the fp64 finder of
knife-edge decisions: images in which a ReLU gate or a pool argmax of the front is decided within fp32 roundoff of a tie,
where two correct fp32 evaluations may legitimately differ (tests/conftest.py: conv_front_knife_images is the MNISTCNN
counterpart).  Also the helpers the LeNet front's GPU test files share."""
import torch
import torch.nn.functional as F

EPS32 = float(torch.finfo(torch.float32).eps)

# (size_img, k_size, fc_l) of buildCIFAR10NormalizingFlow, feature widths 400 / 576 / 64 / 16
GEOMETRIES = (((3, 32, 32), 5, (400, 128, 84)),
              ((1, 32, 32), 3, (576, 128, 32)),
              ((1, 16, 16), 3, (64, 32, 32)),
              ((1, 8, 8), 2, (16, 32, 32)))
DEV = "cuda:0"


def cu(t):
    return t.to(DEV)


def assert_grad(a, b, what):
    from conftest import assert_close, rel_err      # here, not at the top: golden/make_golden_cifar.py imports this file outside pytest
    b = torch.as_tensor(b)
    assert rel_err(a.detach().cpu(), b.detach().cpu()) < 1e-4, (what, rel_err(a.detach().cpu(), b.detach().cpu()))
    assert_close(a, b, rtol=1e-4, atol=1e-6 * float(b.detach().abs().max()), what=what)


def geo_args(gi):
    size_img, k, _ = GEOMETRIES[gi]
    return size_img[0], size_img[1], size_img[2], k


def graph_nodes(t):
    """names of the autograd nodes behind t"""
    seen, names, stack = set(), set(), [t.grad_fn]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        stack += [n for n, _ in f.next_functions]
    return names


def front(e, W1, b1, W2, b2, size_img):
    """flatten(pool2(relu(conv(6->16)(pool2(relu(conv(C->6)(e))))))): [n, C*H*W] -> [n, F]"""
    a1 = F.max_pool2d(F.relu(F.conv2d(e.reshape(-1, *size_img), W1, b1)), 2)
    return F.max_pool2d(F.relu(F.conv2d(a1, W2, b2)), 2).flatten(1)


def cifar10cnn(e, p, size_img):
    """CIFAR10CNN.forward on the parameters p (`conv1.weight` ... `fc3.bias`)"""
    h = front(e, p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"], size_img)
    h = F.relu(F.linear(h, p["fc1.weight"], p["fc1.bias"]))
    h = F.relu(F.linear(h, p["fc2.weight"], p["fc2.bias"]))
    return F.linear(h, p["fc3.weight"], p["fc3.bias"])


def _windows(t):
    """[n, c, h, w] -> [n, c * (h//2) * (w//2), 4]: the 2 x 2 windows of floor pooling, entries in scan order"""
    n, c, h, w = t.shape
    t = t[:, :, :h // 2 * 2, :w // 2 * 2]
    return t.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, -1, 4)


def _stage_knife(a, W, b, ulps):
    """one conv + ReLU + pool stage in fp64: per-image count of knife decisions, and the stage's output"""
    pre = F.conv2d(a, W, b)
    mag = F.conv2d(a.abs(), W.abs(), b.abs())              # |b| + sum |w a|: the magnitude of the terms
    relu_k = (pre.abs() < ulps * EPS32 * mag) & (pre != 0)
    r = F.relu(pre)
    win, wmag = _windows(r), _windows(mag).amax(2, keepdim=True)
    gap = win.amax(2, keepdim=True) - win
    pool_k = (gap < ulps * EPS32 * wmag) & (gap != 0)
    return relu_k.flatten(1).sum(1) + pool_k.flatten(1).sum(1), F.max_pool2d(r, 2)


def knife_images(e, W1, b1, W2, b2, size_img, ulps=16.):
    """[n] bool: images holding a ReLU pre-activation within `ulps` fp32 ulps of its terms' magnitude of zero without being
    zero, or a pool entry that close to its window's maximum without being equal to it, in an fp64 evaluation of the front"""
    e, W1, b1, W2, b2 = [t.detach().cpu().double() for t in (e, W1, b1, W2, b2)]
    k1, a1 = _stage_knife(e.reshape(-1, *size_img), W1, b1, ulps)
    k2, _ = _stage_knife(a1, W2, b2, ulps)
    return (k1 + k2) > 0


def draw_clean_images(n, size_img, W1, b1, W2, b2, gen, rounds=6):
    """n randn images without a knife-edge decision: flagged images are redrawn from the same generator, at most `rounds`
    times.  Returns (images [n, C*H*W], number still flagged -- the caller asserts 0)."""
    d = size_img[0] * size_img[1] * size_img[2]
    e = torch.randn(n, d, generator=gen)
    bad = knife_images(e, W1, b1, W2, b2, size_img)
    for _ in range(rounds):
        if not bool(bad.any()):
            break
        e[bad] = torch.randn(int(bad.sum()), d, generator=gen)
        bad = knife_images(e, W1, b1, W2, b2, size_img)
    return e, int(bad.sum())
