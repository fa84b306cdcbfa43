"""CPU: the allocation hooks of tests/poison.py do what tests/test_gpu_poison.py relies on, the detector is sensitive, and
every workspace the C ABI declares has a poison case (the coverage pin)."""
import os
import re

import pytest
import torch

import poison
from poison import HUGE, NAN, ZERO, poisoned, three_arms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------ the hooks
@pytest.mark.parametrize("bits", [ZERO, NAN, HUGE, 0x3F800000])
def test_the_four_names_fill_fp32_with_the_pattern(bits):
    want = poison._as_int32(bits)
    like = torch.randn(3, 5)
    with poisoned(bits):
        made = [torch.empty(7), torch.empty((2, 3), dtype=torch.float32), torch.empty(4, 2, device="cpu"), torch.empty(()),
                torch.empty_like(like), torch.empty_like(like.t()), torch.empty_strided((3, 4), (6, 1)),
                like.new_empty(6), like.new_empty((2, 2)), torch.empty(0), torch.empty(3, requires_grad=True)]
    for t in made:
        assert t.dtype == torch.float32
        assert bool((_bits(t.detach()) == want).all()), (tuple(t.shape), t)
    # the padding between the rows of a strided allocation is part of the buffer a kernel may read: filled as well
    pad = made[6]
    whole = torch.as_strided(pad, (pad.untyped_storage().nbytes() // 4,), (1,), 0)
    assert whole.numel() == 16 and bool((_bits(whole) == want).all())
    assert made[5].stride() == like.t().stride() and made[10].requires_grad


def test_the_arms_are_what_their_names_say():
    with poisoned(ZERO):
        z = torch.empty(5)
    with poisoned(NAN):
        n = torch.empty(5)
    with poisoned(HUGE):
        h = torch.empty(5)
    assert bool((z == 0).all()) and bool(torch.isnan(n).all())
    assert bool(torch.isfinite(h).all()) and abs(float(h[0]) - 3.3962e38) < 1e34
    assert bool((h * 0. == 0).all()) and bool(torch.isnan(n * 0.).all())
    assert int(_bits(n)[0]) == -1 and int(_bits(h)[0]) == 0x7F7F7F7F


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.bfloat16])
def test_other_floating_widths_get_the_nearest_equivalent(dtype):
    with poisoned(NAN):
        assert bool(torch.isnan(torch.empty(9, dtype=dtype)).all())
    with poisoned(HUGE):
        t = torch.empty(9, dtype=dtype)
        assert bool(torch.isfinite(t).all()) and float(t[0]) == min(poison.float_of(HUGE), torch.finfo(dtype).max)
    with poisoned(ZERO):
        assert bool((torch.empty(9, dtype=dtype) == 0).all())


@pytest.mark.parametrize("bits", [ZERO, NAN, HUGE])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.uint8, torch.bool, torch.int16])
def test_integer_tensors_come_back_zero_in_every_arm(bits, dtype):
    like = torch.ones(4, dtype=dtype)
    with poisoned(bits):
        made = [torch.empty(6, dtype=dtype), torch.empty_like(like), torch.empty_strided((2, 3), (4, 1), dtype=dtype),
                like.new_empty(3), torch.randn(2).new_empty(5, dtype=dtype)]
    for t in made:
        assert t.dtype == dtype and int(t.to(torch.int64).abs().sum()) == 0


def _names():
    return torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty


def test_hooks_are_restored_on_exit_and_after_an_exception():
    before = _names()
    own = "new_empty" in torch.Tensor.__dict__
    with poisoned(NAN):
        inside = _names()
        assert all(a is not b for a, b in zip(inside, before))
    assert all(a is b for a, b in zip(_names(), before))
    with pytest.raises(RuntimeError, match="on purpose"):
        with poisoned(NAN):
            assert bool(torch.isnan(torch.empty(2)).all())
            raise RuntimeError("on purpose")
    assert all(a is b for a, b in zip(_names(), before))
    assert ("new_empty" in torch.Tensor.__dict__) == own
    # nested: the inner arm wins while it lasts, the outer one comes back
    with poisoned(ZERO):
        with poisoned(NAN):
            assert bool(torch.isnan(torch.empty(2)).all())
        assert bool((torch.empty(2) == 0).all())
    assert all(a is b for a, b in zip(_names(), before))


def test_operators_of_torch_keep_working_under_the_hooks():
    """their allocations are made in C++ and do not pass through the Python names"""
    torch.manual_seed(0)
    a, b = torch.randn(8, 8), torch.randn(8, 8)
    want = a @ b + torch.relu(a).sum(0)
    with poisoned(NAN):
        got = a @ b + torch.relu(a).sum(0)
        lin = torch.nn.Linear(4, 3)                       # (torch.empty + an initialiser: every word overwritten)
    assert torch.equal(got, want)
    assert bool(torch.isfinite(lin.weight).all()) and bool(torch.isfinite(lin.bias).all())


# ------------------------------------------------------------------------------------------------ sensitivity
def _operands():
    g = torch.Generator().manual_seed(3)
    return torch.randn(6, 5, generator=g)


def _clean():
    x = _operands()
    out = torch.empty(6)
    torch.sum(x * x, 1, out=out)                          # every word of `out` written before anybody reads it
    return {"out": out, "note": "rows"}


def _sums_over_scratch():
    x = _operands()
    scratch = torch.empty(8, 5)                           # the "partial rows": only six of the eight are written ...
    scratch[:6] = x * x
    return {"out": scratch.sum(0)}                        # ... and all eight are summed


def _masks_scratch():
    x = _operands()
    scratch = torch.empty(8, 5)
    scratch[:6] = x * x
    keep = torch.zeros(8, 1)
    keep[:6] = 1.
    return {"out": (scratch * keep).sum(0)}               # 0 * HUGE == 0 hides it, 0 * NaN does not


def _selects_scratch():
    x = _operands()
    scratch = torch.empty(8, 5)
    scratch[:6] = x * x
    keep = torch.zeros(8, 1, dtype=torch.bool)
    keep[:6] = True
    return {"out": torch.where(keep, scratch, torch.zeros(())).sum(0)}


def test_three_arms_passes_a_clean_function_and_returns_its_results():
    seen = []
    base = three_arms(_clean, judge=lambda r: seen.append(r))
    assert torch.equal(base["out"], (_operands() ** 2).sum(1)) and base["note"] == "rows"
    assert len(seen) == 1 and seen[0] is base
    three_arms(_selects_scratch)                          # the select form of a mask is clean as well


def test_three_arms_catches_a_sum_over_scratch():
    with pytest.raises(AssertionError, match=r"result 'out' differs from the ZERO arm in the NAN arm: 5 of 5 entries"):
        three_arms(_sums_over_scratch)
    # ... and it is the HUGE arm's finding as well
    with poisoned(ZERO):
        z = _sums_over_scratch()
    with poisoned(HUGE):
        h = _sums_over_scratch()
    assert poison.differing(z["out"], h["out"]) == 5


def test_three_arms_catches_a_zero_mask_in_the_nan_arm_only():
    with pytest.raises(AssertionError, match=r"result 'out' differs from the ZERO arm in the NAN arm: 5 of 5 entries"):
        three_arms(_masks_scratch)
    with poisoned(ZERO):
        z = _masks_scratch()
    with poisoned(HUGE):
        h = _masks_scratch()
    assert poison.differing(z["out"], h["out"]) == 0


def test_three_arms_catches_two_zero_runs_that_differ_and_a_result_that_is_not_finite():
    calls = []

    def drifting():
        calls.append(0)
        return {"out": torch.full((3,), float(len(calls)))}
    with pytest.raises(AssertionError, match=r"result 'out' differs from the ZERO arm in the second ZERO arm: 3 of 3"):
        three_arms(drifting)
    with pytest.raises(AssertionError, match=r"result 'out' holds 1 non-finite entries of 3"):
        three_arms(lambda: {"out": torch.tensor([1., float("inf"), 2.])})
    with pytest.raises(AssertionError, match=r"another shape"):
        sizes = iter([3, 3, 4, 3])
        three_arms(lambda: {"out": torch.zeros(next(sizes))})
    # a kernel name that changes with the arm is a difference like any other
    names = iter(["a", "a", "b", "a"])
    with pytest.raises(AssertionError, match=r"result 'kernel' differs from the ZERO arm in the NAN arm"):
        three_arms(lambda: {"kernel": next(names)})
    assert poison.differing(torch.tensor([0.]), torch.tensor([-0.])) == 1          # bits, not values


# ------------------------------------------------------------------------------------------------ the coverage pin
def _declared_workspaces():
    with open(os.path.join(ROOT, "include", "gnf_hip.h")) as f:
        return sorted(set(re.findall(r"\bgnf_\w+_ws_bytes\b", f.read())))


def test_every_workspace_of_the_header_has_a_poison_case():
    """a workspace added to include/gnf_hip.h without a case in tests/test_gpu_poison.py fails here"""
    import test_gpu_poison as G
    declared = _declared_workspaces()
    assert len(declared) >= 20, declared
    missing = [n for n in declared if not G.WORKSPACES.get(n)]
    assert not missing, "workspaces without a poison case in tests/test_gpu_poison.py: %s" % missing
    stale = sorted(set(G.WORKSPACES) - set(declared))
    assert not stale, "WORKSPACES names what include/gnf_hip.h no longer declares: %s" % stale
    for name, tests in G.WORKSPACES.items():
        for t in tests:
            fn = getattr(G, t.split("[")[0], None)
            assert callable(fn) and t.startswith("test_"), "%s lists %r, which tests/test_gpu_poison.py does not define" % (name, t)
            if "[" in t:                                   # a parametrised case: its id is one of the function's
                ids = [i for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"
                       for i in (m.kwargs.get("ids") or [])]
                assert t[t.index("[") + 1:-1] in ids, "%s lists %r: no such case" % (name, t)
