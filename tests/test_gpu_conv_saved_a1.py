"""Conv pair with the conv1 activations kept by the forward (gnf_mnistcnn_conv_fwd_save) and loaded by the backward
(gnf_mnistcnn_conv_bwd_a1 / _cols_a1) instead of recomputed.  The saved values come from the same instruction sequence
on the same inputs as the recompute, so the yardstick is BIT equality with the recompute entry points of the same build
(which the parity tests pin against torch); only the saved image itself is compared with torch (1e-6 absolute, the bound
the conv-front tests use for activations of this size).

Image counts: 1 (prologue only), 2, 255 / 256 / 257 (around the 256-workgroup grid: one workgroup gets a second image),
773 = 3 * 256 + 5 (the buffer parity toggles three times, ragged tail)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KC = 32
D = 784
NS = (1, 2, 255, 256, 257, 773)
NMAX = max(NS)
A1_CH, A1_IMG = 730, 16 * 730


def _window_plan(overflow):
    """the plan gnf_dag_gate_fwd_plan builds for MNIST_A_prior(28, 2), on the host: counts | int16 columns | overflow word"""
    r, c = torch.arange(28).repeat_interleave(28), torch.arange(28).repeat(28)
    win = ((r[:, None] - r[None, :]).abs() <= 2) & ((c[:, None] - c[None, :]).abs() <= 2)
    win.fill_diagonal_(False)
    cols = torch.full((D, KC), -1, dtype=torch.int16)
    for i in range(D):
        jj = win[i].nonzero().flatten()
        cols[i, :len(jj)] = jj.to(torch.int16)
    cnt = win.sum(1).to(torch.int32)
    if overflow:                       # one row with more columns than the plan holds: the device-side dense fallback
        cnt[5] = KC + 1
    return torch.cat([cnt, cols.view(-1).view(torch.int32), torch.full((1,), int(overflow), dtype=torch.int32)])


@pytest.fixture(scope="module")
def data():
    """seeded masked-image-like inputs: the ~1e-6 gate leak times a pseudo-MNIST logit nearly everywhere and a few O(1)
    pixels (|e| <= 1), computed once for the largest n; smaller counts take a prefix (images are independent).  With
    |e| <= 1 the activations stay below sum |W1| + |b1| ~ 4, where an fp32 rounding is <= 2.4e-7: the 1e-6 absolute
    bound on the saved image is a few roundings of the ten-term sum, not a statement about larger values."""
    from gnf_hip.configs import pseudo_mnist
    g = torch.Generator().manual_seed(11)
    x = pseudo_mnist(g, NMAX, D)
    on = torch.rand(NMAX, D, generator=g) < .04
    # the left border carries signal in every image: de at the image columns 0 and 1 is what reads the pad entries
    on[:, 0::28] = True
    on[:, 1::28] = True
    pix = torch.sign(x) * (.05 + .95 * torch.rand(NMAX, D, generator=g))
    e = torch.where(on, pix, 1e-6 * x).contiguous()
    W1, b1 = torch.randn(16, 9, generator=g) * .3, torch.randn(16, generator=g) * .1
    W2, b2 = torch.randn(16, 144, generator=g) * .1, torch.randn(16, generator=g) * .1
    gp = torch.randn(NMAX, 2304, generator=g)
    a1_ref = torch.relu(F.conv2d(e.double().view(-1, 1, 28, 28), W1.double().view(16, 1, 3, 3), b1.double()))
    d = dict(e=e, W1=W1, b1=b1, W2=W2, b2=b2, gp=gp)
    d = {k: v.to(DEV) for k, v in d.items()}
    d["a1_ref"] = a1_ref
    d["plan"] = _window_plan(False).to(DEV)
    d["plan_ovf"] = _window_plan(True).to(DEV)
    return d


def _fwd(d, n, save):
    from gnf_hip import abi
    from gnf_hip.abi import ptr, rawptr, call, stream
    pooled = torch.full((n, 2304), float("nan"), device=DEV)
    arg = torch.full((n, 2304), 255, dtype=torch.uint8, device=DEV)
    a1 = None
    if save:
        nb = abi.load().gnf_mnistcnn_conv_a1_bytes(n)
        assert nb == n * A1_IMG * 4
        # one guard image behind the n the call may write: every thread also issues stores for the chunks past an image's
        # 2 920, which the per-image descriptor must drop -- for the last image they would land here
        buf = torch.full((n + 1, 16, A1_CH), float("nan"), device=DEV)
        call("gnf_mnistcnn_conv_fwd_save", ptr(d["e"]), ptr(d["W1"]), ptr(d["b1"]), ptr(d["W2"]), ptr(d["b2"]), ptr(pooled),
             rawptr(arg), ptr(buf), n, 0, stream())
        assert bool(torch.isnan(buf[n]).all()), "the forward wrote behind the last saved image"
        a1 = buf[:n]
    else:
        call("gnf_mnistcnn_conv_fwd", ptr(d["e"]), ptr(d["W1"]), ptr(d["b1"]), ptr(d["W2"]), ptr(d["b2"]), ptr(pooled),
             rawptr(arg), n, 0, stream())
    return pooled, arg, a1


def _bwd(d, n, arg, a1, plan):
    """-> ge, gec, [gW1, gb1, gW2, gb2]; a1 None: the recompute entry point"""
    from gnf_hip import abi
    from gnf_hip.abi import ptr, rawptr, call, stream
    nws = abi.load().gnf_mnistcnn_conv_bwd_ws_bytes(n)
    ws = torch.empty(nws // 4, device=DEV)
    ge = torch.full((n, D), float("nan"), device=DEV)
    gec = torch.full((n, KC), float("nan"), device=DEV)
    gs = [torch.full_like(d[k], float("nan")) for k in ("W1", "b1", "W2", "b2")]
    head = [ptr(d["e"])] + ([ptr(a1)] if a1 is not None else []) + [ptr(d["W1"]), ptr(d["b1"]), ptr(d["W2"]), ptr(d["gp"]),
                                                                     rawptr(arg), ptr(ge)]
    tail = [ptr(t) for t in gs] + [rawptr(ws), nws, n, stream()]
    sfx = "_a1" if a1 is not None else ""
    if plan is None:
        call("gnf_mnistcnn_conv_bwd" + sfx, *head, *tail)
    else:
        call("gnf_mnistcnn_conv_bwd_cols" + sfx, *head, rawptr(plan), D, ptr(gec), *tail)
    return ge, gec, gs


def _pad_mask():
    m = torch.zeros(16, A1_CH, dtype=torch.bool)
    rows = m[:, :728].view(16, 26, 28)
    rows[:, :, 26:] = True
    m[:, 728:] = True
    return m


@pytest.fixture(scope="module")
def forwards(data):
    """forward with and without a1save, once per n"""
    return {n: (_fwd(data, n, False), _fwd(data, n, True)) for n in NS}


@pytest.mark.parametrize("n", NS)
def test_forward_outputs_unchanged_and_saved_image(data, forwards, n):
    (p0, a0, _), (p1, a1arg, a1) = forwards[n]
    assert torch.equal(p0, p1) and torch.equal(a0, a1arg)
    assert not bool(torch.isnan(a1).any()), "every entry of the saved image is written"
    a1c = a1.cpu()
    valid = a1c[:, :, :728].view(n, 16, 26, 28)[:, :, :, :26]
    err = (valid.double() - data["a1_ref"][:n]).abs().max().item()
    print("n = %d: max |a1 saved - relu(conv1(e))| = %.3g" % (n, err))
    assert err <= 1e-6
    pads = a1c[:, _pad_mask()]
    assert pads.shape == (n, 16 * (26 * 2 + 2))
    assert bool((pads == 0).all()) and not bool(torch.signbit(pads).any()), "pad entries must be exact zeros"


@pytest.mark.parametrize("n", NS)
def test_dense_backward_bit_equal(data, forwards, n):
    (_, arg, _), (_, _, a1) = forwards[n]
    ge0, _, gs0 = _bwd(data, n, arg, None, None)
    ge1, _, gs1 = _bwd(data, n, arg, a1, None)
    assert not bool(torch.isnan(ge0).any())
    assert torch.equal(ge0, ge1)
    for a, b in zip(gs0, gs1):
        assert not bool(torch.isnan(a).any()) and torch.equal(a, b)


@pytest.mark.parametrize("n", NS)
def test_plan_backward_bit_equal(data, forwards, n):
    (_, arg, _), (_, _, a1) = forwards[n]
    ge0, gec0, gs0 = _bwd(data, n, arg, None, data["plan"])
    ge1, gec1, gs1 = _bwd(data, n, arg, a1, data["plan"])
    assert bool(torch.isnan(ge1).all()), "the compact call must not write the dense cotangent"
    cols = data["plan"][D:D + D * KC // 2].view(torch.int16).view(D, KC)
    on = cols[torch.arange(n, device=DEV) % D] >= 0
    assert not bool(torch.isnan(gec0[on]).any())
    assert torch.equal(gec0[on], gec1[on]) and bool(torch.isnan(gec1[~on]).all())
    for a, b in zip(gs0, gs1):
        assert torch.equal(a, b)


def test_plan_overflow_takes_the_dense_fallback(data, forwards):
    n = 257
    (_, arg, _), (_, _, a1) = forwards[n]
    ge0, _, gs0 = _bwd(data, n, arg, None, data["plan_ovf"])
    ge1, _, gs1 = _bwd(data, n, arg, a1, data["plan_ovf"])
    ged, _, _ = _bwd(data, n, arg, a1, None)
    assert not bool(torch.isnan(ge1).any()) and torch.equal(ge0, ge1) and torch.equal(ge1, ged)
    for a, b in zip(gs0, gs1):
        assert torch.equal(a, b)


def test_backward_depends_on_zero_pads(data, forwards):
    """the whole-image copy overwrites the pad entries of the LDS buffer on every image, and the de gather reads them:
    a sentinel there must change ge (so the data reaches the pads and the zero requirement is real), zeros restore it"""
    n = 257
    (_, arg, _), (_, _, a1) = forwards[n]
    ge0, _, gs0 = _bwd(data, n, arg, None, None)
    bad = a1.clone()
    bad[:, _pad_mask().to(DEV)] = 1e6
    geb, _, _ = _bwd(data, n, arg, bad, None)
    assert not torch.equal(geb, ge0)
    diff = (geb != ge0).view(n, 28, 28)
    # a tap that moves left of column 0 lands on the pad columns of the row above; columns 26, 27 read their own row's
    assert bool(diff[:, :, :2].any()) and not bool(diff[:, :, 2:26].any()), "only the border columns read the pads"
    bad[:, _pad_mask().to(DEV)] = 0.
    gez, _, gsz = _bwd(data, n, arg, bad, None)
    assert torch.equal(gez, ge0)
    for a, b in zip(gs0, gsz):
        assert torch.equal(a, b)


def test_entry_points_validate_their_arguments(data):
    """refusals on REAL small buffers (were a check ever lost, the call would run on valid memory), n = 0 where the check
    comes before the empty-batch return"""
    from gnf_hip import abi
    import ctypes
    lib = abi.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())                                    # noqa: E731
    n = 1
    e, W1, b1, W2, b2, gp = [P(data[k]) for k in ("e", "W1", "b1", "W2", "b2", "gp")]
    pooled, arg = torch.empty(n, 2304, device=DEV), torch.empty(n, 2304, dtype=torch.uint8, device=DEV)
    a1 = torch.zeros(n + 1, A1_IMG, device=DEV)
    odd = ctypes.c_void_p(a1.data_ptr() + 4)                                       # dword- but not 16-byte aligned
    ge = torch.empty(n, D, device=DEV)
    gs = [torch.empty_like(data[k]) for k in ("W1", "b1", "W2", "b2")]
    nws = lib.gnf_mnistcnn_conv_bwd_ws_bytes(n)
    ws = torch.empty(nws // 4, device=DEV)
    assert lib.gnf_mnistcnn_conv_a1_bytes(3) == 3 * A1_IMG * 4 and lib.gnf_mnistcnn_conv_a1_bytes(0) == 0
    # exact_ties keeps nothing; misaligned buffer (both refused ahead of the empty-batch return: n = 0)
    assert lib.gnf_mnistcnn_conv_fwd_save(e, W1, b1, W2, b2, P(pooled), P(arg), P(a1), 0, 1, None) == -1
    assert lib.gnf_mnistcnn_conv_fwd_save(e, W1, b1, W2, b2, P(pooled), P(arg), odd, 0, 0, None) == -1
    tail = [P(t) for t in gs] + [P(ws), nws, n, None]
    assert lib.gnf_mnistcnn_conv_bwd_a1(e, None, W1, b1, W2, gp, P(arg), P(ge), *tail) == -1          # images, no buffer
    tail0 = [P(t) for t in gs] + [P(ws), nws, 0, None]
    assert lib.gnf_mnistcnn_conv_bwd_cols_a1(e, odd, W1, b1, W2, gp, P(arg), P(ge), None, 0, None, *tail0) == -1
    torch.cuda.synchronize()


@pytest.fixture
def a1_count(monkeypatch):
    """counts the saved-a1 buffers ops hands out (ops._a1_buffer wrapped; nothing in the product keeps such a count)"""
    from gnf_hip import ops
    made = []
    real = ops._a1_buffer

    def counting(*args, **kw):
        buf = real(*args, **kw)
        if buf is not None:
            made.append(buf.numel() * 4)
        return buf
    monkeypatch.setattr(ops, "_a1_buffer", counting)
    return made


def _front_step(data, B, exact_ties=False, grad=True):
    from gnf_hip import ops
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, D, generator=g).to(DEV)
    r, c = torch.arange(28).repeat_interleave(28), torch.arange(28).repeat(28)
    win = ((r[:, None] - r[None, :]).abs() <= 2) & ((c[:, None] - c[None, :]).abs() <= 2)
    win.fill_diagonal_(False)
    A = (win.float() * (torch.rand(D, D, generator=g) + .3)).to(DEV).requires_grad_(grad)
    ps = [data[k].clone().requires_grad_(grad) for k in ("W1", "b1", "W2", "b2")]
    wgt = torch.randn(B * D, 2304, generator=g).to(DEV)
    pooled = ops.dag_conv_front(x, A, 1, 1, 0., 1., None, None, 1234, 7, *ps, exact_ties=exact_ties)
    loss = (pooled * wgt).sum()
    if grad:
        loss.backward()
    return loss.detach(), [p.grad for p in ps] + [A.grad]


def test_autograd_plumbing_switch_on_and_off(data, monkeypatch, a1_count):
    monkeypatch.setenv("GNF_CONV_SAVE_A1", "1")
    l1, g1 = _front_step(data, 2)
    assert a1_count == [2 * D * A1_IMG * 4]
    monkeypatch.setenv("GNF_CONV_SAVE_A1", "0")
    l0, g0 = _front_step(data, 2)
    assert len(a1_count) == 1
    assert torch.equal(l0, l1)
    for a, b in zip(g0, g1):
        assert a is not None and torch.equal(a, b)
    monkeypatch.setenv("GNF_CONV_SAVE_A1", "1")
    monkeypatch.setenv("GNF_CONV_SAVE_A1_MAX_BYTES", str(2 * D * A1_IMG * 4 - 1))     # one byte under what B = 2 needs
    lc, gc = _front_step(data, 2)
    assert len(a1_count) == 1 and torch.equal(lc, l1)
    for a, b in zip(gc, g1):
        assert torch.equal(a, b)


def test_no_buffer_without_a_backward_or_with_exact_ties(data, monkeypatch, a1_count):
    monkeypatch.setenv("GNF_CONV_SAVE_A1", "1")
    with torch.no_grad():
        _front_step(data, 1, grad=False)
    _front_step(data, 1, grad=False)                     # grad mode on, nothing requires a gradient
    _, ge = _front_step(data, 1, exact_ties=True)
    assert a1_count == [] and ge[0] is not None


def _conv_step(data, n, exact_ties=False, grad=True, bare=False):
    """MnistConvFn the way models.MLP calls it (ops.mnist_conv); bare: a direct .apply, which carries no grad mode"""
    from gnf_hip import ops
    e = data["e"][:n].clone().requires_grad_(grad)
    ps = [data[k].clone().requires_grad_(True) for k in ("W1", "b1", "W2", "b2")]      # trainable also under no_grad
    pooled = ops.MnistConvFn.apply(e, *ps, exact_ties) if bare else ops.mnist_conv(e, *ps, exact_ties=exact_ties)
    if not pooled.requires_grad:
        return pooled.detach(), None
    (pooled * data["gp"][:n]).sum().backward()
    return pooled.detach(), [e.grad] + [p.grad for p in ps]


def test_mnist_conv_plumbing(data, monkeypatch, a1_count):
    n = 257
    monkeypatch.setenv("GNF_CONV_SAVE_A1", "1")
    p1, g1 = _conv_step(data, n)
    assert a1_count == [n * A1_IMG * 4]
    monkeypatch.setenv("GNF_CONV_SAVE_A1", "0")
    p0, g0 = _conv_step(data, n)
    assert len(a1_count) == 1 and torch.equal(p0, p1)
    for a, b in zip(g0, g1):
        assert a is not None and torch.equal(a, b)
    monkeypatch.setenv("GNF_CONV_SAVE_A1", "1")
    with torch.no_grad():                                # trainable parameters, no backward: nothing kept
        pn, gn = _conv_step(data, n)
    assert len(a1_count) == 1 and gn is None and torch.equal(pn, p1)
    _, gx = _conv_step(data, n, exact_ties=True)         # the direct forward keeps nothing
    assert len(a1_count) == 1 and gx[0] is not None
    pb, gb = _conv_step(data, n, bare=True)              # no grad mode handed in: recompute, same bits
    assert len(a1_count) == 1 and torch.equal(pb, p1)
    for a, b in zip(gb, g1):
        assert torch.equal(a, b)
