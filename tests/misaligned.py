"""Operands at dword-only alignment, between guard bands.

Every allocation of torch starts on (at least) a 16-byte boundary, and so does every operand the rest of the suite builds.
`place(t, k)` returns a tensor equal to `t` whose storage starts 4 k bytes past such a boundary (k = 1, 2, 3; k = 0 gives the
aligned twin with the same guards), carved out of a larger buffer `buf` = [guard | the tensor's span | guard] whose guard
floats hold a fixed bit pattern; `guards_intact` checks both bands bit for bit.  The contract of include/gnf_hip.h is that
every fp32 array may sit at any 4-byte-aligned address: tests/test_gpu_alignment.py hands such tensors to every entry point."""
import torch

SENTINEL = 0x7FA5C3E1            # int32 bit pattern of the guards: a NaN whose payload no kernel produces


def _span(t):
    """(lowest, one past the highest) storage element the view addresses, relative to its storage offset"""
    if t.numel() == 0:
        return 0, 0
    lo = hi = 0
    for n, s in zip(t.shape, t.stride()):
        if s >= 0:
            hi += (n - 1) * s
        else:
            lo += (n - 1) * s
    return lo, hi + 1


def place(t, k, guard=16):
    """A tensor equal to `t` (same shape, same strides) whose first addressed element lies 4 k bytes past a 16-byte boundary,
    with `guard` sentinel floats directly before and after the addressed span.  A non-contiguous `t` gives the same view over
    the displaced base (the elements the view skips hold the sentinel too).  `place(t, k).guard_buf` is the buffer
    [guard | span | guard] (a float32 tensor)."""
    assert t.dtype == torch.float32 and 0 <= k < 4 and guard >= 1
    lo, hi = _span(t)
    span = hi - lo
    raw = torch.empty(2 * guard + span + 4, dtype=torch.float32, device=t.device)
    raw.view(torch.int32).fill_(SENTINEL)
    shift = (k - raw.data_ptr() // 4 - guard) % 4          # buf[guard] lands on offset k (in floats) modulo 16 bytes
    buf = raw[shift:shift + 2 * guard + span]
    out = buf.as_strided(tuple(t.shape), tuple(t.stride()), buf.storage_offset() + guard - lo)
    out.copy_(t)
    out.guard_buf, out.guard = buf, guard
    assert buf[guard:].data_ptr() % 16 == 4 * k
    return out


def guard_bands(t):
    """the two guard regions (int32 views) of a tensor returned by place()"""
    bits = t.guard_buf.view(torch.int32)
    return bits[:t.guard], bits[bits.numel() - t.guard:]


def guards_intact(t):
    """True when both guard bands of a tensor returned by place() still hold the sentinel, bit for bit"""
    return all(bool((band == SENTINEL).all()) for band in guard_bands(t))
