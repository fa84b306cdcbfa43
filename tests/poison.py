"""Uninitialised memory with a chosen content.

The library never allocates device memory itself: every output, saved activation and workspace of a kernel is a `torch.empty`
made in Python (gnf_hip/ops.py, models/, gnf_hip/dp.py).  What such a buffer holds before the first kernel writes it is an
accident of the allocator -- zeroed pages in a fresh process, finite leftovers of the previous test inside a long pytest run --
so a kernel that READS a word nobody wrote passes every comparison of the suite.  `poisoned(bits)` removes the accident: for
its duration `torch.empty`, `torch.empty_like`, `torch.empty_strided` and `torch.Tensor.new_empty` return tensors whose
memory holds the bit pattern `bits`, and `three_arms(fn)` runs a computation under three patterns and demands the same bits
from each.  (Only the Python names are replaced: the allocations torch's own operators make in C++ do not pass through them.)

Floating tensors are filled with the int32 pattern `bits`: fp32 through an int32 view of the WHOLE storage (the padding an
`empty_strided` leaves between rows included); another floating width gets the nearest equivalent, the fp32 value of `bits`
(NaN stays NaN, a finite value is clamped into the finite range of the type).

Integer, bool and uint8 tensors are filled with ZEROS IN EVERY ARM: a wild index or a counter that never comes up would be a
fault or a hang, not a failed assertion.  Integer scratch is therefore out of scope of this detector; what a kernel reads as
an integer has to be checked by reading its code.

Arms:  ZERO = 0;  NAN = -1 (0xFFFFFFFF, a NaN in any float width);  HUGE = 0x7F7F7F7F (3.3962e38: finite, so that
0 * HUGE == 0 where 0 * NaN is NaN -- a read that a zero mask hides from HUGE still shows under NAN, and a read that is added
into a sum shows under both)."""
import contextlib
import struct

import torch

ZERO, NAN, HUGE = 0, -1, 0x7F7F7F7F
ARMS = (("ZERO", ZERO), ("NAN", NAN), ("HUGE", HUGE))

_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _as_int32(bits):
    """the signed int32 with the 32-bit pattern `bits` (0xFFFFFFFF and -1 are the same pattern)"""
    bits &= 0xFFFFFFFF
    return bits - (1 << 32) if bits >= 1 << 31 else bits


def float_of(bits):
    """the fp32 value whose bit pattern is `bits`"""
    return struct.unpack("<f", struct.pack("<I", bits & 0xFFFFFFFF))[0]


def fill(t, bits):
    """fill the fresh tensor `t` as the module docstring says; returns t"""
    if not torch.is_tensor(t) or t.device.type == "meta" or t.is_sparse:
        return t
    with torch.no_grad():
        if t.dtype == torch.float32:
            n = t.untyped_storage().nbytes() // 4
            if n:
                torch.as_strided(t.detach().view(torch.int32), (n,), (1,), 0).fill_(_as_int32(bits))
        elif t.is_floating_point():
            v = float_of(bits)
            if v == v:                                                  # finite (or inf): into the range of the type
                top = torch.finfo(t.dtype).max
                v = max(-top, min(top, v))
            t.detach().fill_(v)
        else:
            t.detach().zero_()                                          # integers, bool, complex: zeros in every arm
    return t


_ACTIVE = []


def current_bits():
    """the int32 pattern of the innermost poisoned() in force (None outside): what a fresh fp32 tensor holds right now"""
    return _as_int32(_ACTIVE[-1]) if _ACTIVE else None


def holds_pattern(t):
    """True when every word of the fp32 tensor `t` still holds the pattern in force: nobody wrote it"""
    return bool((t.detach().contiguous().view(torch.int32) == current_bits()).all())


@contextlib.contextmanager
def poisoned(bits):
    """for the duration: every tensor the four Python allocation names return is filled first (see fill)"""
    def wrap(orig):
        def alloc(*args, **kwargs):
            return fill(orig(*args, **kwargs), bits)
        alloc.__name__ = getattr(orig, "__name__", "alloc")
        alloc.__wrapped__ = orig
        return alloc

    names = ("empty", "empty_like", "empty_strided")
    saved = {n: getattr(torch, n) for n in names}
    _ACTIVE.append(bits)
    own_new_empty = torch.Tensor.__dict__.get("new_empty")              # (normally inherited from the C base class: None)
    base_new_empty = torch.Tensor.new_empty
    try:
        for n in names:
            setattr(torch, n, wrap(saved[n]))
        torch.Tensor.new_empty = wrap(base_new_empty)
        yield
    finally:
        _ACTIVE.pop()
        for n in names:
            setattr(torch, n, saved[n])
        if own_new_empty is None:
            if "new_empty" in torch.Tensor.__dict__:
                del torch.Tensor.new_empty
        else:
            torch.Tensor.new_empty = own_new_empty


def _bits_of(t):
    """the tensor as integers of its element size, on the host: equality of these is equality of bits"""
    t = t.detach()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    elif t.is_floating_point() or t.is_complex():
        if t.is_complex():
            t = torch.view_as_real(t)
        t = t.contiguous().view(_INT_OF_SIZE[t.element_size()])
    return t.cpu()


def differing(a, b):
    """number of entries of two results that differ in their bits (-1: another shape, type or kind of value)"""
    if torch.is_tensor(a) != torch.is_tensor(b):
        return -1
    if not torch.is_tensor(a):
        return 0 if a == b else 1
    if a.shape != b.shape or a.dtype != b.dtype:
        return -1
    return int((_bits_of(a) != _bits_of(b)).sum())


def _compare(base, out, arm):
    assert set(out) == set(base), "arm %s returned other results: %s vs %s" % (arm, sorted(out), sorted(base))
    for name in base:
        n = differing(base[name], out[name])
        assert n == 0, ("result %r differs from the ZERO arm in the %s arm: %s" % (
            name, arm, "another shape / type / value" if n < 0 else
            "%d of %d entries" % (n, base[name].numel() if torch.is_tensor(base[name]) else 1)))


def three_arms(fn, judge=None):
    """fn() -> {name: tensor (or a string / number: a kernel name, a count)}.  fn builds its operands from a fixed seed out
    of torch.randn / torch.zeros / .clone() -- never torch.empty -- and runs the computation under test; every torch.empty the
    library makes on the way is poisoned.  Runs fn under ZERO twice, then NAN, then HUGE and asserts, in this order:
      the two ZERO runs agree bit for bit (the kernels promise the same bits on every call; nothing below can be judged without);
      NAN agrees with ZERO bit for bit;  HUGE agrees with ZERO bit for bit;  every floating result is finite.
    judge(results), when given, is called on the first ZERO run (the fp64 comparison of the op's own test: a case must not
    pass by being consistently wrong).  Returns the results of the first ZERO run."""
    with poisoned(ZERO):
        base = fn()
    assert isinstance(base, dict) and base, "fn returns a non-empty dict of named results"
    if judge is not None:
        judge(base)
    with poisoned(ZERO):
        again = fn()
    _compare(base, again, "second ZERO")
    for arm, bits in ARMS[1:]:
        with poisoned(bits):
            out = fn()
        _compare(base, out, arm)
    for name, t in base.items():
        if torch.is_tensor(t) and t.is_floating_point():
            bad = int((~torch.isfinite(t)).sum())
            assert bad == 0, "result %r holds %d non-finite entries of %d (the same in every arm)" % (name, bad, t.numel())
    return base
