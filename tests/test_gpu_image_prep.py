"""gnf_image_prep (csrc/gnf_image_prep.hip, gnf_hip.ops.image_prep): the batch preparation of the image driver in one launch.
Injected uniforms against train_image.prepare_reference in fp64; the dword / float4 form against the byte form, bit for bit;
the Philox layout of include/gnf_hip.h against a numpy restatement; determinism and keys; the law of the noise; the flip coin;
the empty batch and the argument errors (host side, no GPU needed)."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close

PKG = os.path.join(ROOT, "graphical-normalizing-flows_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

DEV = "cuda:0"
SHAPES = [(1, 1, 1, 1), (3, 3, 5, 7), (2, 1, 28, 28), (5, 3, 32, 32)]
N_DATA = 7
ROWS = [1, 4, 1, 0, 6]                   # unordered, row 1 twice from B = 3 on; rows 0 / 1 are all 0 / all 255
FLIPS = [1, 0, 1, 1, 0]
SEED, OFFSET = 0x1234567887654321 & ((1 << 62) - 1), (7 << 32) + 11       # both halves of the key and of the counter in use


def _driver():
    import train_image
    return train_image


def _data(d, dev=DEV, n=N_DATA, seed=0, edges=True):
    u8 = torch.randint(0, 256, (n, d), generator=torch.Generator().manual_seed(seed)).to(torch.uint8)
    if edges:
        u8[0], u8[1] = 0, 255
    return u8.to(dev)


def _uniforms(B, d, seed=1):
    return torch.rand(B, d, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------ numpy restatement of the Philox layout
def _constants():
    src = open(os.path.join(PKG, "gnf_hip", "csrc", "gnf_common.h")).read()
    body = src[src.index("void philox4x32_10("):]
    m0 = re.search(r"\(uint64_t\)(0x[0-9A-Fa-f]+)u \* c0", body).group(1)
    m1 = re.search(r"\(uint64_t\)(0x[0-9A-Fa-f]+)u \* c2", body).group(1)
    w0 = re.search(r"k0 \+= (0x[0-9A-Fa-f]+)u", body).group(1)
    w1 = re.search(r"k1 \+= (0x[0-9A-Fa-f]+)u", body).group(1)
    return tuple(np.uint64(int(v, 16)) for v in (m0, m1, w0, w1))


MASK = np.uint64(0xffffffff)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Salmon et al. 2011, ten rounds; every word a uint64 array holding 32 bits"""
    M0, M1, W0, W1 = _constants()
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def u01_open(w):
    return ((w >> np.uint64(9)).astype(np.float32) + np.float32(.5)) * np.float32(1. / 8388608.)


def _split(v):
    return np.uint64(v & 0xffffffff), np.uint64(v >> 32)


def philox_uniforms(B, d, seed, offset):
    """the uniform of output element e = b d + j: word e & 3 of counter (e >> 2, offset), key seed"""
    e = np.arange(B * d, dtype=np.uint64)
    q = e >> np.uint64(2)
    r = philox4x32_10(q & MASK, q >> S32, *_split(offset), *_split(seed))
    w = np.choose((e & np.uint64(3)).astype(np.int64), r)
    return u01_open(w).reshape(B, d)


def philox_coins(B, seed, offset):
    """the flip coin of output row b: counter (b, offset) with bit 31 of the second word set; mirrored when bit 31 of r[0]"""
    b = np.arange(B, dtype=np.uint64)
    r = philox4x32_10(b & MASK, (b >> S32) | np.uint64(0x80000000), *_split(offset), *_split(seed))
    return (r[0] >> np.uint64(31)).astype(np.uint8)


def test_numpy_philox_is_the_published_one():
    """Random123's known-answer vectors for philox4x32-10 (kat_vectors): the constants read from gnf_common.h and the round
    function restated above give them, so the layout test below compares the kernel with Philox and not with a private
    variant of it"""
    out = philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in out] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    out = philox4x32_10(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)
    assert [int(v) for v in out] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    u = u01_open(np.array([0, 0xffffffff], dtype=np.uint64))
    assert u[0] == np.float32(2. ** -24) and u[1] == np.float32(1. - 2. ** -24)        # open on both sides


def _ks_distance(t):
    t = np.sort(np.asarray(t, dtype=np.float64).reshape(-1))
    n = t.size
    i = np.arange(1, n + 1)
    return max((i / n - t).max(), (t - (i - 1) / n).max())


def test_ks_bound_holds_for_numpy_uniforms():
    """the bound of test_noise_law, 2 / sqrt(N) at N = 24 576 (exceeded by a true uniform sample with probability
    2 exp(-2 * 4) = 7e-4), on numpy's own generator"""
    n = 8 * 3072
    for seed in range(5):
        assert _ks_distance(np.random.default_rng(seed).random(n)) <= 2. / math.sqrt(n)


# ------------------------------------------------------------------------------------ host side: no GPU needed
def test_symbol_declared_and_bound():
    from gnf_hip import abi
    header = open(os.path.join(ROOT, "include", "gnf_hip.h")).read()
    assert "gnf_image_prep(" in header and "gnf_image_prep" in abi.SIGNATURES and hasattr(abi.load(), "gnf_image_prep")
    assert abi.ABI_VERSION == 11 and abi.load().gnf_abi_version() == 11


def test_empty_batch_and_argument_errors_return_before_any_launch():
    """every call here returns on the host: B = 0 with NULL pointers is a valid call; the pointers of the refused calls are
    never dereferenced (there is no device behind them)"""
    from gnf_hip import abi, ops, GnfError
    fn = abi.load().gnf_image_prep
    p = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never read

    def rc(data=p, n_rows=7, rows=p, mode=0, flip=None, chw=(3, 5, 7), u=None, alpha=.05, x=p, term=None, B=2):
        return fn(data, n_rows, rows, mode, flip, *chw, u, 1, 0, alpha, x, term, B, None)
    assert rc(data=None, rows=None, x=None, B=0) == 0
    assert rc(B=-1) == -1 and rc(chw=(3, 0, 7)) == -1 and rc(mode=3) == -1 and rc(mode=-1) == -1
    assert rc(alpha=.5) == -1 and rc(alpha=-1e-3) == -1 and rc(alpha=float("nan")) == -1
    assert rc(data=None) == -1 and rc(x=None) == -1 and rc(n_rows=0) == -1
    assert rc(mode=1, flip=None) == -1                # the mask is required in mode 1
    assert rc(rows=None, B=8) == -1                   # rows 0 .. B-1 need B <= n_rows
    odd = ctypes.c_void_p((1 << 20) + 2)
    assert rc(x=odd) == -1 and rc(u=odd) == -1 and rc(term=odd) == -1 and rc(rows=odd) == -1
    assert rc(B=1 << 31) == -2
    with pytest.raises(GnfError, match="no CPU fallback"):
        ops.image_prep(torch.zeros(7, 105, dtype=torch.uint8), None, None, None, 1, 0, .05, (3, 5, 7), True)
    with pytest.raises(GnfError, match="uint8"):
        ops.image_prep(torch.zeros(7, 104, dtype=torch.uint8), None, None, None, 1, 0, .05, (3, 5, 7), True)


# ------------------------------------------------------------------------------------ GPU
def _raw(data, rows, mode, flip, size, u, seed, offset, alpha, x, term):
    """the entry point itself, on operands placed by the test"""
    from gnf_hip import abi
    B = x.shape[0]
    abi.call("gnf_image_prep", abi.rawptr(data), data.shape[0], abi.rawptr(rows) if rows is not None else None, mode,
             abi.rawptr(flip) if flip is not None else None, *size, abi.ptr(u), seed, offset, alpha, abi.ptr(x),
             abi.ptr(term), B, abi.stream())


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [1e-6, .05])
@pytest.mark.parametrize("shape", SHAPES)
def test_injected_uniforms_against_the_reference(shape, alpha):
    from gnf_hip import ops
    T = _driver()
    B, size = shape[0], shape[1:]
    d = size[0] * size[1] * size[2]
    u8, u = _data(d), _uniforms(B, d)
    rows = torch.tensor(ROWS[:B], dtype=torch.int32)
    mask = torch.tensor(FLIPS[:B], dtype=torch.uint8)
    for r, f in ((rows, mask), (rows, None), (None, mask), (None, None)):
        data = u8 if r is not None else u8[:B]
        x, term = ops.image_prep(data, r.to(DEV) if r is not None else None, f.to(DEV) if f is not None else None,
                                 u.to(DEV), 0, 0, alpha, size, True)
        want_x, want_t = T.prepare_reference(data.cpu(), r, f, u, alpha, size, torch.float64)
        assert torch.isfinite(x).all()
        assert_close(x, want_x, rtol=1e-5, atol=1e-6, what="x %s rows %s flip %s" % (shape, r is not None, f is not None))
        assert_close(term, want_t, rtol=1e-5, atol=0., what="bpp_term %s" % (shape,))
        x2, none = ops.image_prep(data, r.to(DEV) if r is not None else None, f.to(DEV) if f is not None else None,
                                  u.to(DEV), 0, 0, alpha, size, False)
        assert none is None and torch.equal(x2, x)                 # asking for the term changes no bit of x


@pytest.mark.gpu
@pytest.mark.parametrize("philox", [False, True])
def test_vector_and_byte_forms_are_bit_identical(philox):
    """(5,3,32,32): aligned operands take the dword / float4 form; data one, two or three bytes into a buffer, x one, two or
    three floats into one (dword-aligned only), u one float into one -- each sends the call to the byte form.  Same bits."""
    from gnf_hip import ops
    B, size = 5, (3, 32, 32)
    d = 3072
    u8 = _data(d)
    rows = torch.tensor(ROWS, dtype=torch.int32, device=DEV)
    mask = torch.tensor(FLIPS, dtype=torch.uint8, device=DEV)
    u = None if philox else _uniforms(B, d).to(DEV)
    for mode, flip in ((1, mask), (2, None), (0, None)):
        x0 = torch.empty(B, d, device=DEV)
        t0 = torch.empty(B, device=DEV)
        assert u8.data_ptr() % 4 == 0 and x0.data_ptr() % 16 == 0 and (u is None or u.data_ptr() % 16 == 0)
        _raw(u8, rows, mode, flip, size, u, SEED, OFFSET, .05, x0, t0)
        via_ops = ops.image_prep(u8, rows, flip if mode == 1 else mode == 2, u, SEED, OFFSET, .05, size, True)
        assert torch.equal(via_ops[0], x0) and torch.equal(via_ops[1], t0)
        for off in (1, 2, 3):
            buf = torch.zeros(N_DATA * d + 8, dtype=torch.uint8, device=DEV)
            shifted = buf[off:off + N_DATA * d].view(N_DATA, d)
            shifted.copy_(u8)
            assert shifted.data_ptr() % 4 == off
            x1, t1 = torch.empty(B, d, device=DEV), torch.empty(B, device=DEV)
            _raw(shifted, rows, mode, flip, size, u, SEED, OFFSET, .05, x1, t1)
            assert torch.equal(x1, x0) and torch.equal(t1, t0), ("data + %d bytes" % off, mode)
            xbuf = torch.full((B * d + 8,), 7.25, device=DEV)
            x2, t2 = xbuf[off:off + B * d].view(B, d), torch.empty(B, device=DEV)
            assert x2.data_ptr() % 16 == 4 * off
            _raw(u8, rows, mode, flip, size, u, SEED, OFFSET, .05, x2, t2)
            assert torch.equal(x2, x0) and torch.equal(t2, t0), ("x + %d floats" % off, mode)
            assert (xbuf[:off] == 7.25).all() and (xbuf[off + B * d:] == 7.25).all()       # nothing outside x is written
        if u is not None:
            ubuf = torch.zeros(B * d + 4, device=DEV)
            u3 = ubuf[1:1 + B * d].view(B, d)
            u3.copy_(u)
            x3, t3 = torch.empty(B, d, device=DEV), torch.empty(B, device=DEV)
            _raw(u8, rows, mode, flip, size, u3, SEED, OFFSET, .05, x3, t3)
            assert torch.equal(x3, x0) and torch.equal(t3, t0), ("u + 1 float", mode)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (2, 1, 28, 28)])
def test_philox_layout(shape):
    """the uniforms and the row coins of (seed, offset), restated in numpy from the layout of include/gnf_hip.h and handed in
    as explicit uniforms / an explicit mask, give the bits of the Philox call"""
    from gnf_hip import ops
    B, size = shape[0], shape[1:]
    d = size[0] * size[1] * size[2]
    u8 = _data(d)
    rows = torch.tensor(ROWS[:B], dtype=torch.int32, device=DEV)
    u = torch.from_numpy(philox_uniforms(B, d, SEED, OFFSET)).to(DEV)
    assert 0. < float(u.min()) and float(u.max()) < 1.
    x, t = ops.image_prep(u8, rows, None, None, SEED, OFFSET, .05, size, True)
    xi, ti = ops.image_prep(u8, rows, None, u, 0, 0, .05, size, True)
    assert torch.equal(x, xi) and torch.equal(t, ti)
    coins = torch.from_numpy(philox_coins(B, SEED, OFFSET)).to(DEV)
    x, t = ops.image_prep(u8, rows, True, None, SEED, OFFSET, .05, size, True)
    xi, ti = ops.image_prep(u8, rows, coins, u, 0, 0, .05, size, True)
    assert torch.equal(x, xi) and torch.equal(t, ti)


@pytest.mark.gpu
def test_determinism_and_keys():
    from gnf_hip import ops
    size, d = (3, 32, 32), 3072
    u8 = _data(d)
    rows = torch.tensor(ROWS, dtype=torch.int32, device=DEV)

    def run(seed, offset, B=5):
        return ops.image_prep(u8, rows[:B], True, None, seed, offset, .05, size, True)
    x, t = run(SEED, OFFSET)
    x2, t2 = run(SEED, OFFSET)
    assert torch.equal(x, x2) and torch.equal(t, t2)
    for other in (run(SEED, OFFSET + 1), run(SEED + 1, OFFSET), run(SEED, OFFSET + (1 << 32)), run(SEED + (1 << 32), OFFSET)):
        assert (other[0] != x).float().mean().item() > .99
    xs, ts = run(SEED, OFFSET, B=2)                                 # row b does not depend on B
    assert torch.equal(xs, x[:2]) and torch.equal(ts, t[:2])


@pytest.mark.gpu
def test_noise_law():
    """(8,3,32,32), alpha = .05, one fixed seed: t = 256 (sigmoid(x) - alpha) / (1 - 2 alpha) - pixel, in fp64, is the noise
    the kernel added.  It lies in (-1e-3, 1 + 1e-3) (the bounds of the MNIST driver test) and its Kolmogorov-Smirnov
    distance from U(0,1) over the N = 24 576 values is at most 2 / sqrt(N): a condition, not a measurement -- a true uniform
    sample exceeds it with probability 7e-4, the seed is fixed, and numpy's generator at that N stays inside it
    (test_ks_bound_holds_for_numpy_uniforms, on the CPU)."""
    from gnf_hip import ops
    alpha, size, d = .05, (3, 32, 32), 3072
    u8 = _data(d, n=8, seed=4)
    x, _ = ops.image_prep(u8, None, None, None, SEED, OFFSET, alpha, size, False)
    t = 256. * (torch.sigmoid(x.double()) - alpha) / (1. - 2. * alpha) - u8.double()
    print("noise: min %.6f max %.6f" % (t.min().item(), t.max().item()))
    assert t.min().item() > -1e-3 and t.max().item() < 1. + 1e-3
    ks = _ks_distance(t.cpu().numpy())
    print("KS distance %.5f, bound %.5f" % (ks, 2. / math.sqrt(t.numel())))
    assert ks <= 2. / math.sqrt(t.numel())


@pytest.mark.gpu
def test_flip_coin():
    from gnf_hip import ops
    alpha, size, B = .05, (3, 2, 4), 256
    u8 = _data(24, n=B, seed=6, edges=False)                       # (a constant row is its own mirror image)

    def flipped_rows(offset):
        x, _ = ops.image_prep(u8, None, True, None, SEED, offset, alpha, size, False)
        t = (256. * (torch.sigmoid(x.double()) - alpha) / (1. - 2. * alpha)).view(B, 3, 2, 4)
        img = u8.double().view(B, 3, 2, 4)

        def is_it(cand):                                           # pixel <= t < pixel + 1 everywhere, to the noise bounds
            n = (t - cand).flatten(1)
            return (n.min(1).values > -1e-3) & (n.max(1).values < 1. + 1e-3)
        plain, mirrored = is_it(img), is_it(img.flip(3))
        assert (plain ^ mirrored).all()                            # exactly one of the two candidates
        return mirrored
    m = flipped_rows(OFFSET)
    print("flipped rows: %d of %d" % (int(m.sum()), B))
    assert abs(int(m.sum()) - 128) <= 32                           # 4 sigma of Binomial(256, 1/2)
    assert torch.equal(flipped_rows(OFFSET), m)
    assert not torch.equal(flipped_rows(OFFSET + 1), m)
    assert torch.equal(m.cpu(), torch.from_numpy(philox_coins(B, SEED, OFFSET)).bool())


@pytest.mark.gpu
def test_empty_batch_on_the_device():
    from gnf_hip import ops
    u8 = _data(105)
    x, t = ops.image_prep(u8, torch.empty(0, dtype=torch.int32, device=DEV), None, None, 1, 0, .05, (3, 5, 7), True)
    assert x.shape == (0, 105) and t.shape == (0,)
    x, t = ops.image_prep(u8[:0], None, True, None, 1, 0, .05, (3, 5, 7), False)
    assert x.shape == (0, 105) and t is None
    torch.cuda.synchronize()
