"""CPU: the placement helper of tests/misaligned.py does what tests/test_gpu_alignment.py relies on."""
import pytest
import torch

from misaligned import place, guards_intact, guard_bands, SENTINEL


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(7,), (5, 3), (4, 6, 2), ()])
def test_place_contiguous(k, shape):
    t = torch.randn(shape)
    p = place(t, k)
    assert p.data_ptr() % 16 == 4 * k
    assert p.shape == t.shape and p.stride() == t.stride() and p.is_contiguous()
    assert p.contiguous().data_ptr() == p.data_ptr()          # what ops.py hands to a kernel is the displaced address
    assert torch.equal(p, t)
    assert guards_intact(p)
    lo, hi = guard_bands(p)
    assert lo.numel() == hi.numel() == 16 and int(lo[0]) == SENTINEL
    # the bands touch the tensor: its first and last element are the buffer's neighbours of the guards
    assert p.guard_buf[16:].data_ptr() == p.data_ptr() and p.guard_buf.numel() == 32 + t.numel()


@pytest.mark.parametrize("k", [1, 2, 3])
def test_a_write_next_to_the_tensor_breaks_the_guard(k):
    p = place(torch.randn(9, 5), k, guard=16)
    p.guard_buf[16 - 1] = 0.                                   # the float directly in front of the tensor
    assert not guards_intact(p)
    p = place(torch.randn(9, 5), k, guard=16)
    p.guard_buf[16 + 45] = 1.                                  # the float directly behind it
    assert not guards_intact(p)
    p = place(torch.randn(9, 5), k, guard=4)
    assert guards_intact(p)
    p.guard_buf.view(torch.int32)[0] ^= 1                      # one bit of the outermost guard float
    assert not guards_intact(p)
    p = place(torch.randn(9, 5), k)
    p.fill_(3.)                                                # writing the tensor itself leaves them alone
    assert guards_intact(p)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_place_keeps_a_non_contiguous_view(k):
    B, d = 6, 5
    raw = torch.randn(B, 2 * d)
    views = [raw.view(B, 2, d).permute(0, 2, 1),               # MADE layout of h: strides (2 d, 1, d)
             torch.randn(7, 9)[:, :6],                         # padded leading stride
             torch.randn(9, 7)[:, :4].t()]                     # column-major with padding
    for t in views:
        assert not t.is_contiguous()
        p = place(t, k)
        assert p.shape == t.shape and p.stride() == t.stride() and not p.is_contiguous()
        assert p.data_ptr() % 16 == 4 * k and torch.equal(p, t) and guards_intact(p)
        last = sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
        assert p.guard_buf.numel() == 32 + last + 1            # the guards enclose exactly the span the view addresses
