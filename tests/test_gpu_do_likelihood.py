"""GPU: the interventional likelihood log p(x | do(x_S)) -- csrc/gnf_do_terms.hip, ops.NllDoFn / AffineDoFn,
NormalizingFlowStep.forward_do, FCNormalizingFlow.log_prob_do / loss_do, dp.train_step(targets=, regime=).

The reference is the law itself, written in torch on fp64 CPU tensors with torch.where:
    logdet[b] = sum_{i free} log jac[b, i]        logn[b] = -1/2 sum_{i free} (log 2 pi + z[b, i]^2)
Inputs and tolerances of the kernel-level cases are those of test_nll_reduce_vs_torch and
test_affine_fused_normal_log_density (tests/test_gpu_parity.py): rtol 2e-6, atol 1e-5 sqrt(d) for the row sums -- a masked sum
has no more terms than the sums those bounds were set for -- and their gradient tolerances.

Shapes: (3, 1), (7, 5), (33, 63), (1100, 63), (1030, 64), (2200, 30) the 16-lane-group kernels (d <= 64; in MADE's layout the
strided lane-group kernels with 8, 32 and 64 lanes per row); (9, 784), (5, 300) a workgroup per row forward and a workgroup
per 256-column chunk backward; (5, 100), added here, is the smallest shape on the row-per-wavefront forward (64 < d < 256) --
(65 600, 5), added here, is the smallest batch at which the 16-lane-group kernels, whose grid stops at 4096 workgroups of 16
rows, take a second trip of their grid-stride loop (B > 65 536), with a regime vector looked up again on that trip -- every
dispatch branch of the four entry points is reached."""
import math

import pytest
import torch

from conftest import assert_close, assert_fwd, rel_err
from misaligned import guards_intact, place
from poison import three_arms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5            # tests/test_gpu_parity.py
GTOL = 1e-4
LOG2PI = math.log(2. * math.pi)
SHAPES = [(3, 1), (7, 5), (33, 63), (1100, 63), (1030, 64), (2200, 30), (9, 784), (5, 300), (5, 100), (65600, 5)]
FORMS = ["R1", "R3", "RB"]


def cu(t):
    return t.to(DEV)


def req(t):
    return t.clone().to(DEV).requires_grad_(True)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------- tables and the law
def table(B, d, form, gen):
    """(pin uint8 [R, d], regime int64 [B] or None, pinned bool [B, d]) on the host.
    R1: one random row.  R3: rows (all free, random, all pinned) and a regime vector that never names row 0.
    RB: a row per sample -- row 0 all free, row 1 all pinned, the others random."""
    rnd = lambda n: (torch.rand(n, d, generator=gen) < .5).to(torch.uint8)     # noqa: E731
    if form == "R1":
        pin, regime = rnd(1), None
        rows = pin.expand(B, d)
    elif form == "R3":
        pin = torch.cat((torch.zeros(1, d, dtype=torch.uint8), rnd(1), torch.ones(1, d, dtype=torch.uint8)))
        regime = 1 + torch.randint(0, 2, (B,), generator=gen)
        regime[0], regime[B - 1] = 1, 2
        rows = pin[regime]
    else:
        pin, regime = rnd(B), None
        pin[0] = 0
        pin[1] = 1
        rows = pin
    return pin.contiguous(), regime, rows.bool().clone()


def dev_table(pin, regime):
    return cu(pin), (None if regime is None else cu(regime).to(torch.int32))


def law64(z, jac, pinned):
    """the truncated factorisation in fp64 with torch.where: a pinned element's value is never part of the sum"""
    z, jac = z.double(), jac.double()
    zero = torch.zeros((), dtype=torch.float64)
    ld = torch.where(pinned, zero, torch.log(torch.where(pinned, torch.ones((), dtype=torch.float64), jac))).sum(1)
    ln = -.5 * torch.where(pinned, zero, LOG2PI + torch.where(pinned, zero, z) ** 2).sum(1)
    return ld, ln


def affine64(x, h, pinned):
    """(z, jac, logdet, logn) of the Affine normalizer under the mask, fp64"""
    mu, ls = torch.clamp(h[:, :, 0], -5., 5.), torch.clamp(h[:, :, 1], -5., 2.)
    z = x * torch.exp(ls) + mu
    zero = torch.zeros((), dtype=torch.float64)
    ld = torch.where(pinned, zero, ls).sum(1)
    ln = -.5 * torch.where(pinned, zero, LOG2PI + torch.where(pinned, zero, z) ** 2).sum(1)
    return z, torch.exp(ls), ld, ln


def h_of(hraw, B, d, layout):
    """the [B, d, 2] view of a conditioner output: contiguous, or MADE's [B, 2 d] viewed with strides (2 d, 1, d)"""
    return hraw.view(B, 2, d).permute(0, 2, 1) if layout == "made" else hraw


# ------------------------------------------------------------------------------------- NllDoFn, forward and backward vs fp64
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,d", SHAPES)
def test_nll_do_vs_fp64(B, d, form):
    from gnf_hip import ops
    g = torch.Generator().manual_seed(B + d)
    z = torch.randn(B, d, generator=g)
    jac = torch.rand(B, d, generator=g) * 3 + .05
    gl, gn = torch.randn(B, generator=g), torch.randn(B, generator=g)
    pin, regime, pinned = table(B, d, form, g)
    zr, jr = z.double().requires_grad_(True), jac.double().requires_grad_(True)
    ld0, ln0 = law64(zr, jr, pinned)
    ((ld0 * gl.double()).sum() + (ln0 * gn.double()).sum()).backward()
    zg, jg = req(z), req(jac)
    p, r = dev_table(pin, regime)
    ld, ln = ops.NllDoFn.apply(zg, jg, p, r)
    at = 1e-5 * d ** .5
    assert_close(ld, ld0.detach(), rtol=2e-6, atol=at, what="logdet")
    assert_close(ln, ln0.detach(), rtol=2e-6, atol=at, what="logN")
    ((ld * cu(gl)).sum() + (ln * cu(gn)).sum()).backward()
    assert_close(zg.grad, zr.grad, rtol=1e-6, atol=1e-7, what="gz")
    assert_close(jg.grad, jr.grad, rtol=2e-6, atol=1e-7, what="gjac")
    # an all-pinned row: both sums and the row's cotangents are exactly zero; a pinned element's gjac is +0, its gz 0
    full = cu(pinned.all(1))
    if bool(full.any()):
        assert bool((ld[full] == 0).all()) and bool((ln[full] == 0).all())
        assert bool((zg.grad[full] == 0).all()) and bool((bits(jg.grad)[full] == 0).all())
    assert form == "R1" or bool(full.any())
    assert bool((bits(jg.grad)[cu(pinned)] == 0).all()) and bool((zg.grad[cu(pinned)] == 0).all())
    # the same operands again: the same bits
    ld2, ln2 = ops.NllDoFn.apply(zg.detach(), jg.detach(), p, r)
    assert torch.equal(bits(ld2), bits(ld)) and torch.equal(bits(ln2), bits(ln))


@pytest.mark.parametrize("B,d", [(7, 5), (33, 63), (5, 300)])
def test_nll_do_zero_table_agrees_with_the_unmasked_reduction(B, d):
    """a device table of zeros takes the masked kernels and agrees with gnf_nll_reduce to rounding (another summation order)"""
    from gnf_hip import ops
    g = torch.Generator().manual_seed(B + d)
    z, jac = cu(torch.randn(B, d, generator=g)), cu(torch.rand(B, d, generator=g) * 3 + .05)
    ld, ln = ops.NllDoFn.apply(z, jac, torch.zeros(1, d, dtype=torch.uint8, device=DEV), None)
    ld1, ln1 = ops.NllReduceFn.apply(z, jac)
    assert_close(ld, ld1, rtol=2e-6, atol=1e-5 * d ** .5, what="logdet")
    assert_close(ln, ln1, rtol=2e-6, atol=1e-5 * d ** .5, what="logN")


# ---------------------------------------------------------------------------------- AffineDoFn, forward and backward vs fp64
@pytest.mark.parametrize("layout", ["contig", "made"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,d", SHAPES)
def test_affine_do_vs_fp64(B, d, form, layout):
    from gnf_hip import ops
    g = torch.Generator().manual_seed(17 * B + d)
    x = torch.randn(B, d, generator=g)
    hraw = torch.randn(B, 2 * d, generator=g) * 2.5 if layout == "made" else torch.randn(B, d, 2, generator=g) * 2.5
    gzv, gjv, gl, gn = (torch.randn(s, generator=g) for s in ((B, d), (B, d), (B,), (B,)))
    pin, regime, pinned = table(B, d, form, g)
    xr, hr = x.double().requires_grad_(True), hraw.double().requires_grad_(True)
    z0, j0, ld0, ln0 = affine64(xr, h_of(hr, B, d, layout), pinned)
    ((z0 * gzv).sum() + (j0 * gjv).sum() + (ld0 * gl).sum() + (ln0 * gn).sum()).backward()
    xg, hg = req(x), req(hraw)
    p, r = dev_table(pin, regime)
    z, jac, ld, ln = ops.AffineDoFn.apply(xg, h_of(hg, B, d, layout), p, r, True)
    at = 1e-5 * d ** .5
    assert_close(z, z0, what="z")
    assert_close(jac, j0, what="jac")
    assert_close(ld, ld0, rtol=2e-6, atol=at, what="logdet")
    assert_close(ln, ln0, rtol=2e-6, atol=at, what="logN")
    ((z * cu(gzv)).sum() + (jac * cu(gjv)).sum() + (ld * cu(gl)).sum() + (ln * cu(gn)).sum()).backward()
    assert rel_err(xg.grad.cpu(), xr.grad) < GTOL and rel_err(hg.grad.cpu(), hr.grad) < GTOL
    assert hg.grad.shape == hraw.shape
    # without jac (the step's form) and with the row cotangents alone: a pinned element gets exactly nothing
    xg2, hg2 = req(x), req(hraw)
    z2, none, ld2, ln2 = ops.AffineDoFn.apply(xg2, h_of(hg2, B, d, layout), p, r, False)
    assert none.numel() == 0 and torch.equal(bits(z2), bits(z))
    assert torch.equal(bits(ld2), bits(ld)) and torch.equal(bits(ln2), bits(ln))          # the same operands: the same bits
    ((ld2 * cu(gl)).sum() + (ln2 * cu(gn)).sum()).backward()
    xr.grad, hr.grad = None, None
    _, _, ld1, ln1 = affine64(xr, h_of(hr, B, d, layout), pinned)
    ((ld1 * gl).sum() + (ln1 * gn).sum()).backward()
    assert rel_err(xg2.grad.cpu(), xr.grad) < GTOL and rel_err(hg2.grad.cpu(), hr.grad) < GTOL
    pd = cu(pinned)
    assert bool((xg2.grad[pd] == 0).all()) and bool((h_of(hg2.grad, B, d, layout)[pd] == 0).all())
    full = pd.all(1)
    if bool(full.any()):
        assert bool((ld[full] == 0).all()) and bool((ln[full] == 0).all())
    assert form == "R1" or bool(full.any())


# ----------------------------------------------------------------------------------------------- excluded means unread
@pytest.mark.parametrize("B,d", SHAPES)
def test_nll_do_never_reads_a_pinned_element(B, d):
    from gnf_hip import ops
    g = torch.Generator().manual_seed(B + d)
    z, jac = torch.randn(B, d, generator=g), torch.rand(B, d, generator=g) * 3 + .05
    gl, gn = cu(torch.randn(B, generator=g)), cu(torch.randn(B, generator=g))
    pin, regime, pinned = table(B, d, "R3", g)
    p, r = dev_table(pin, regime)
    n = int(pinned.sum())
    bad_z = torch.tensor([float("nan"), float("inf"), float("-inf")]).repeat(n // 3 + 1)[:n]
    bad_j = torch.tensor([0., -1., float("nan")]).repeat(n // 3 + 1)[:n]
    hostile_z, hostile_j = z.clone(), jac.clone()
    hostile_z[pinned], hostile_j[pinned] = bad_z, bad_j

    def run(zz, jj):
        zg, jg = req(zz), req(jj)
        ld, ln = ops.NllDoFn.apply(zg, jg, p, r)
        ((ld * gl).sum() + (ln * gn).sum()).backward()
        return ld.detach(), ln.detach(), zg.grad, jg.grad
    ld, ln, gz, gj = run(z, jac)
    ld_h, ln_h, gz_h, gj_h = run(hostile_z, hostile_j)
    free = cu(~pinned)
    assert torch.equal(bits(ld_h), bits(ld)) and torch.equal(bits(ln_h), bits(ln))
    assert torch.equal(bits(gz_h)[free], bits(gz)[free]) and torch.equal(bits(gj_h)[free], bits(gj)[free])
    for t in (gz, gz_h, gj, gj_h):
        assert bool((bits(t)[~free] == 0).all())                          # exactly +0, whatever lies there
    assert bool(torch.isfinite(ld_h).all()) and bool(torch.isfinite(ln_h).all())


@pytest.mark.parametrize("layout", ["contig", "made"])
@pytest.mark.parametrize("B,d", SHAPES)
def test_affine_do_never_uses_a_pinned_element(B, d, layout):
    from gnf_hip import ops
    g = torch.Generator().manual_seed(17 * B + d)
    x = torch.randn(B, d, generator=g)
    hraw = torch.randn(B, 2 * d, generator=g) * 2.5 if layout == "made" else torch.randn(B, d, 2, generator=g) * 2.5
    gl, gn = cu(torch.randn(B, generator=g)), cu(torch.randn(B, generator=g))
    pin, regime, pinned = table(B, d, "R3", g)
    p, r = dev_table(pin, regime)
    hostile_x, hostile_h = x.clone(), hraw.clone()
    hostile_x[pinned] = 1e30
    hv = h_of(hostile_h, B, d, layout)
    sign = torch.where(torch.rand(B, d, generator=g) < .5, -1., 1.)
    hv[:, :, 0] = torch.where(pinned, 1e30 * sign, hv[:, :, 0])
    hv[:, :, 1] = torch.where(pinned, -1e30 * sign, hv[:, :, 1])

    def run(xx, hh):
        xg, hg = req(xx), req(hh)
        z, _, ld, ln = ops.AffineDoFn.apply(xg, h_of(hg, B, d, layout), p, r, False)
        ((ld * gl).sum() + (ln * gn).sum()).backward()
        return z.detach(), ld.detach(), ln.detach(), xg.grad, h_of(hg.grad, B, d, layout)
    z, ld, ln, gx, gh = run(x, hraw)
    z_h, ld_h, ln_h, gx_h, gh_h = run(hostile_x, hostile_h)
    free = cu(~pinned)
    assert torch.equal(bits(ld_h), bits(ld)) and torch.equal(bits(ln_h), bits(ln))
    assert bool(torch.isfinite(ld_h).all()) and bool(torch.isfinite(ln_h).all())
    assert torch.equal(bits(z_h)[free], bits(z)[free])
    assert torch.equal(bits(gx_h)[free], bits(gx)[free]) and torch.equal(bits(gh_h)[free], bits(gh)[free])
    for t in (gx, gx_h, gh, gh_h):                                        # the row cotangents never reach a pinned element
        assert bool((t[~free] == 0).all())


# ------------------------------------------------------------------------------ uninitialised buffers (tests/poison.py)
@pytest.mark.parametrize("B,d", [(7, 5), (33, 63), (5, 300), (5, 100)])
def test_poison_nll_do(B, d):
    from gnf_hip import ops

    def fn():
        g = torch.Generator().manual_seed(B + d)
        zg, jg = req(torch.randn(B, d, generator=g)), req(torch.rand(B, d, generator=g) * 3 + .05)
        gl, gn = cu(torch.randn(B, generator=g)), cu(torch.randn(B, generator=g))
        p, r = dev_table(*table(B, d, "R3", g)[:2])
        ld, ln = ops.NllDoFn.apply(zg, jg, p, r)
        ((ld * gl).sum() + (ln * gn).sum()).backward()
        return {"logdet": ld.detach(), "logn": ln.detach(), "gz": zg.grad, "gjac": jg.grad}
    three_arms(fn)


@pytest.mark.parametrize("layout", ["contig", "made"])
@pytest.mark.parametrize("B,d", [(7, 5), (33, 63), (2200, 30), (5, 300), (5, 100)])
def test_poison_affine_do(B, d, layout):
    from gnf_hip import ops

    def fn():
        g = torch.Generator().manual_seed(17 * B + d)
        xg = req(torch.randn(B, d, generator=g))
        hg = req(torch.randn(B, 2 * d, generator=g) * 2.5 if layout == "made" else torch.randn(B, d, 2, generator=g) * 2.5)
        gzv, gl, gn = (cu(torch.randn(s, generator=g)) for s in ((B, d), (B,), (B,)))
        p, r = dev_table(*table(B, d, "R3", g)[:2])
        out = {}
        for want_jac in (False, True):
            xg.grad = hg.grad = None
            z, jac, ld, ln = ops.AffineDoFn.apply(xg, h_of(hg, B, d, layout), p, r, want_jac)
            ((z * gzv).sum() + (ld * gl).sum() + (ln * gn).sum() + (jac.sum() if want_jac else 0.)).backward()
            out.update({"z%d" % want_jac: z.detach(), "ld%d" % want_jac: ld.detach(), "ln%d" % want_jac: ln.detach(),
                        "gx%d" % want_jac: xg.grad.clone(), "gh%d" % want_jac: hg.grad.clone()})
            if want_jac:
                out["jac"] = jac.detach()
        return out
    three_arms(fn)


# ------------------------------------------------------------------------------------------------------------- alignment
ALIGN_SHAPES = [(7, 5), (33, 63), (5, 300), (5, 100)]


def _odd(pin):
    """the table at an odd address, inside a larger allocation"""
    buf = torch.zeros(pin.numel() + 16, dtype=torch.uint8, device=DEV)
    off = 1 if buf.data_ptr() % 2 == 0 else 2
    out = buf[off:off + pin.numel()].view(pin.shape)
    out.copy_(pin)
    assert out.data_ptr() % 2 == 1 and out.is_contiguous()
    return out


@pytest.mark.parametrize("B,d", ALIGN_SHAPES)
def test_nll_do_entry_points_at_dword_alignment(B, d):
    """every fp32 operand 4, 8 and 12 bytes past a 16-byte boundary between guard bands, the table at an odd address: against
    the aligned run with the tolerance tests/test_gpu_alignment.py holds gnf_nll_reduce to (test_row_reductions_and_losses)"""
    from gnf_hip import abi
    g = torch.Generator().manual_seed(B + d)
    ops_ = {"z": cu(torch.randn(B, d, generator=g)), "jac": cu(torch.rand(B, d, generator=g) * 3 + .05),
            "glogdet": cu(torch.randn(B, generator=g)), "glogn": cu(torch.randn(B, generator=g)),
            "gz_in": cu(torch.randn(B, d, generator=g))}
    pin, regime, _ = table(B, d, "R3", g)
    p, r = dev_table(pin, regime)
    at = 1e-5 * d ** .5

    def run(k, pin_t):
        t = {n: place(v, k) for n, v in ops_.items()}
        t.update({n: place(torch.zeros(B, device=DEV), k) for n in ("logdet", "logn")})
        t.update({n: place(torch.zeros(B, d, device=DEV), k) for n in ("gz", "gjac")})
        P = abi.ptr
        abi.call("gnf_nll_do_fwd", P(t["z"]), P(t["jac"]), abi.rawptr(pin_t), abi.rawptr(r), 3, P(t["logdet"]), P(t["logn"]), B, d,
                 abi.stream())
        abi.call("gnf_nll_do_bwd", P(t["z"]), P(t["jac"]), abi.rawptr(pin_t), abi.rawptr(r), 3, P(t["glogdet"]), P(t["glogn"]),
                 P(t["gz_in"]), P(t["gz"]), P(t["gjac"]), B, d, abi.stream())
        torch.cuda.synchronize()
        for n, v in t.items():
            assert guards_intact(v), "guard band of %s overwritten at offset %d" % (n, 4 * k)
        return {n: t[n].clone() for n in ("logdet", "logn", "gz", "gjac")}
    base = run(0, p)
    for k in (1, 2, 3):
        out = run(k, _odd(p))
        assert_close(out["logdet"], base["logdet"], rtol=2e-6, atol=at, what="logdet +%d" % (4 * k))
        assert_close(out["logn"], base["logn"], rtol=2e-6, atol=at, what="logN +%d" % (4 * k))
        assert_close(out["gz"], base["gz"], rtol=1e-6, atol=1e-7, what="gz +%d" % (4 * k))
        assert_close(out["gjac"], base["gjac"], rtol=2e-6, atol=1e-7, what="gjac +%d" % (4 * k))


@pytest.mark.parametrize("layout", ["contig", "made"])
@pytest.mark.parametrize("B,d", ALIGN_SHAPES)
def test_affine_do_entry_points_at_dword_alignment(B, d, layout):
    """the fused pair likewise: row sums to the bound above, z / jac / gx / gh to the forward bound of
    test_affine_forward_backward_inverse (tests/test_gpu_alignment.py)"""
    from gnf_hip import abi
    g = torch.Generator().manual_seed(17 * B + d)
    hraw = torch.randn(B, 2 * d, generator=g) * 2.5 if layout == "made" else torch.randn(B, d, 2, generator=g) * 2.5
    h = h_of(hraw, B, d, layout).to(DEV)                  # (.to keeps the strides of the MADE view)
    assert h.stride() == h_of(hraw, B, d, layout).stride()
    ops_ = {"x": cu(torch.randn(B, d, generator=g)), "h": h, "gz": cu(torch.randn(B, d, generator=g)),
            "gjac": cu(torch.randn(B, d, generator=g)), "glogdet": cu(torch.randn(B, generator=g)),
            "glogn": cu(torch.randn(B, generator=g))}
    pin, regime, _ = table(B, d, "R3", g)
    p, r = dev_table(pin, regime)
    at = 1e-5 * d ** .5

    def run(k, pin_t):
        t = {n: place(v, k) for n, v in ops_.items()}
        t.update({n: place(torch.zeros(B, device=DEV), k) for n in ("logdet", "logn")})
        t.update({n: place(torch.zeros(B, d, device=DEV), k) for n in ("z", "jac", "gx")})
        t["gh"] = place(torch.zeros_like(h), k)
        P, hh, gh = abi.ptr, t["h"], t["gh"]
        assert gh.stride() == h.stride()
        abi.call("gnf_affine_do_fwd", P(t["x"]), P(hh), hh.stride(0), hh.stride(1), hh.stride(2), abi.rawptr(pin_t), abi.rawptr(r),
                 3, P(t["z"]), P(t["jac"]), P(t["logdet"]), P(t["logn"]), B, d, abi.stream())
        abi.call("gnf_affine_do_bwd", P(t["x"]), P(hh), hh.stride(0), hh.stride(1), hh.stride(2), abi.rawptr(pin_t), abi.rawptr(r),
                 3, P(t["gz"]), P(t["gjac"]), P(t["glogdet"]), P(t["glogn"]), P(t["gx"]), P(gh), gh.stride(0), gh.stride(1),
                 gh.stride(2), B, d, abi.stream())
        torch.cuda.synchronize()
        for n, v in t.items():
            assert guards_intact(v), "guard band of %s overwritten at offset %d" % (n, 4 * k)
        return {n: t[n].clone() for n in ("z", "jac", "logdet", "logn", "gx", "gh")}
    base = run(0, p)
    for k in (1, 2, 3):
        out = run(k, _odd(p))
        assert_close(out["logdet"], base["logdet"], rtol=2e-6, atol=at, what="logdet +%d" % (4 * k))
        assert_close(out["logn"], base["logn"], rtol=2e-6, atol=at, what="logN +%d" % (4 * k))
        for n in ("z", "jac", "gx", "gh"):
            assert rel_err(out[n].cpu(), base[n].cpu()) < TOL, (n, k)
            assert_fwd(out[n], base[n].cpu(), what="%s +%d" % (n, 4 * k))


# ------------------------------------------------------------------------------------- the incoming cotangent gz_in
@pytest.mark.parametrize("B,d", [(7, 5), (33, 63), (5, 300), (65600, 5)])
def test_nll_do_bwd_with_gz_in_vs_fp64(B, d):
    """gnf_nll_do_bwd with gz_in (ops.NllDoFn never passes one) against the law in fp64: gz = gz_in - z glogn at free elements,
    gz = gz_in -- exactly, the caller's bits -- at pinned ones, NaN in the row of a regime id out of range.  The bound at free
    elements is that of tests/test_gpu_alignment.py for gnf_nll_reduce_bwd with gz_in: the plain call's rtol 1e-6, atol 1e-7
    plus the two roundings of the sum, each half an ulp (2^-24) of a term's magnitude."""
    from gnf_hip import abi
    g = torch.Generator().manual_seed(B + d)
    z, jac = torch.randn(B, d, generator=g), torch.rand(B, d, generator=g) * 3 + .05
    gl, gn, gin = torch.randn(B, generator=g), torch.randn(B, generator=g), torch.randn(B, d, generator=g)
    pin, regime, pinned = table(B, d, "R3", g)
    regime[2] = 3                                          # R = 3: out of range
    free = ~pinned
    gz0 = torch.where(free, gin.double() - z.double() * gn.double()[:, None], gin.double())
    gj0 = torch.where(free, gl.double()[:, None] / torch.where(free, jac.double(), torch.ones((), dtype=torch.float64)),
                      torch.zeros((), dtype=torch.float64))
    tol = 1e-6 * gz0.abs() + 1e-7 + 2. ** -23 * ((z.double() * gn.double()[:, None]).abs() + gin.double().abs())
    zd, jd, gld, gnd, gind = (cu(t) for t in (z, jac, gl, gn, gin))
    p, r = dev_table(pin, regime)
    gz, gj = torch.zeros(B, d, device=DEV), torch.zeros(B, d, device=DEV)
    P = abi.ptr
    abi.call("gnf_nll_do_bwd", P(zd), P(jd), abi.rawptr(p), abi.rawptr(r), 3, P(gld), P(gnd), P(gind), P(gz), P(gj), B, d,
             abi.stream())
    ok = torch.ones(B, dtype=torch.bool)
    ok[2] = False
    assert bool(torch.isnan(gz[2]).all()) and bool(torch.isnan(gj[2]).all())
    excess = (gz.cpu().double() - gz0).abs() - tol
    assert float(excess[ok].max()) <= 0., float(excess[ok].max())
    assert_close(gj[cu(ok)], gj0[ok], rtol=2e-6, atol=1e-7, what="gjac")
    keep = pinned & ok[:, None]
    assert bool(keep.any()) and torch.equal(bits(gz.cpu()[keep]), bits(gin[keep]))      # the caller's bits
    assert bool((bits(gj.cpu()[keep]) == 0).all())


# --------------------------------------------------------------------------------------------- out-of-range regime ids
@pytest.mark.parametrize("layout", ["contig", "made"])
@pytest.mark.parametrize("B,d", [(7, 5), (33, 63), (5, 300), (5, 100)])
def test_regime_ids_out_of_range_give_nan_rows_and_touch_nothing_else(B, d, layout):
    """ids R and -1 in two rows; the table is a slice from the middle of a larger allocation, so even a broken guard would
    stay inside owned memory.  Those rows come out NaN -- the row sums, and every output cotangent's row --, every other
    row is the valid run's, bit for bit."""
    from gnf_hip import ops
    g = torch.Generator().manual_seed(B + d)
    R = 3
    big = torch.zeros(R + 8, d, dtype=torch.uint8, device=DEV)
    pin = big[4:4 + R]
    pin.copy_(cu(table(B, d, "R3", g)[0]))
    assert pin.is_contiguous()
    good = torch.randint(0, R, (B,), generator=g).to(torch.int32)
    bad = good.clone()
    bad[1], bad[B - 2] = R, -1
    rows_bad = torch.zeros(B, dtype=torch.bool)
    rows_bad[1] = rows_bad[B - 2] = True
    z, jac = torch.randn(B, d, generator=g), torch.rand(B, d, generator=g) * 3 + .05
    x = torch.randn(B, d, generator=g)
    hraw = torch.randn(B, 2 * d, generator=g) * 2.5 if layout == "made" else torch.randn(B, d, 2, generator=g) * 2.5
    gl, gn, gzv = cu(torch.randn(B, generator=g)), cu(torch.randn(B, generator=g)), cu(torch.randn(B, d, generator=g))

    def run(regime):
        zg, jg, xg, hg = req(z), req(jac), req(x), req(hraw)
        ld, ln = ops.NllDoFn.apply(zg, jg, pin, cu(regime))
        # (sum of products with a NaN row would poison nothing else: the cotangents are rows of gl / gn)
        torch.autograd.backward((ld, ln), (gl, gn))
        za, _, lda, lna = ops.AffineDoFn.apply(xg, h_of(hg, B, d, layout), pin, cu(regime), False)
        torch.autograd.backward((za, lda, lna), (gzv, gl, gn))
        return {"ld": ld.detach(), "ln": ln.detach(), "gz": zg.grad, "gjac": jg.grad, "z_affine": za.detach(),
                "ld_affine": lda.detach(), "ln_affine": lna.detach(), "gx": xg.grad, "gh": h_of(hg.grad, B, d, layout)}
    ok, out = run(good), run(bad)
    nb, keep = cu(rows_bad), cu(~rows_bad)
    for name in ok:
        a, b = out[name], ok[name]
        if name == "z_affine":                            # z is written for every column of every row
            assert torch.equal(bits(a), bits(b))
            continue
        assert bool(torch.isnan(a[nb]).all()), name
        assert torch.equal(bits(a[keep]), bits(b[keep])), name
        assert bool(torch.isfinite(b).all()), name


# -------------------------------------------------------------------------------------------------- step and flow level
K_BINS, TAIL = 4, 3.


def _normalizer(norm):
    from models import AffineNormalizer, MonotonicNormalizer, SplineNormalizer
    if norm == "affine":
        return AffineNormalizer, {}, 2
    if norm == "spline":
        return SplineNormalizer, {"nb_bins": K_BINS, "tail_bound": TAIL}, 3 * K_BINS - 1
    return MonotonicNormalizer, {"integrand_net": [8, 8], "cond_size": 4, "nb_steps": 8, "solver": "CC"}, 4


def _flow(cond, norm, d, c, seed=0):
    """a one-step flow on the device; cond in MADE / DAG (deterministic gate) / DAGstoch (stochastic gate) / Coupling"""
    from models import AutoregressiveConditioner, CouplingConditioner, DAGConditioner, buildFCNormalizingFlow
    N, nkw, out = _normalizer(norm)
    torch.manual_seed(seed)
    cargs = {"in_size": d, "hidden": [16], "out_size": out, "cond_in": c}
    if cond.startswith("DAG"):
        flow = buildFCNormalizingFlow(1, DAGConditioner, dict(cargs, hot_encoding=True, l1=.1), N, nkw)
        cnd = flow.steps[0].conditioner
        with torch.no_grad():
            cnd.A.copy_(torch.rand(d, d) * .8 + .1)
            cnd.A.fill_diagonal_(0.)
        cnd.stoch_gate = cond == "DAGstoch"
        cnd.noise_gate = False
        cnd.invalidate_caches()
    else:
        flow = buildFCNormalizingFlow(1, AutoregressiveConditioner if cond == "MADE" else CouplingConditioner, cargs, N, nkw)
    return flow.to(DEV)


def _fix_gate(flow, B, d, seed):
    cnd = flow.steps[0].conditioner
    if getattr(cnd, "stoch_gate", False):
        gen = torch.Generator().manual_seed(seed)
        cnd.gate_noise = (cu(torch.rand(B, d, d, generator=gen)), cu(torch.rand(B, d, d, generator=gen)))


def _case(B, d, c, seed):
    gen = torch.Generator().manual_seed(seed)
    x = cu(torch.randn(B, d, generator=gen))
    ctx = cu(torch.randn(B, c, generator=gen)) if c else None
    pin, regime, pinned = table(B, d, "R3", gen)
    return x, ctx, cu(pin), cu(regime), pinned


@pytest.mark.parametrize("cond", ["MADE", "DAG", "DAGstoch", "Coupling"])
@pytest.mark.parametrize("norm", ["affine", "spline", "monotonic"])
def test_flow_log_prob_do_and_loss_do(norm, cond):
    """log_prob_do against the fp64 law evaluated on the step's own (z, jac); parameter and x gradients of loss_do against
    autograd on the composed fp32 torch law over the same (z, jac) graph (GTOL, the bound of the normalizers' own tests).

    The bound on log_prob_do = logdet + logn: each row sum is held to rtol 2e-6, atol 1e-5 sqrt(d) above, and the addition
    rounds once more (2^-24 of the result)."""
    for d, B in ((6, 40), (63, 33)):
        for c in (0, 2):
            flow = _flow(cond, norm, d, c, seed=d + c)
            step = flow.steps[0]
            _fix_gate(flow, B, d, seed=B + d)
            x, ctx, pin, regime, pinned = _case(B, d, c, seed=B + d + c)
            case = "%s %s d=%d B=%d c=%d" % (norm, cond, d, B, c)
            with torch.no_grad():
                z, jac = step.normalizer(x, step.conditioner(x, ctx), ctx)
                lp = flow.log_prob_do(x, pin, regime, ctx)
                zs, lds, lns = step.forward_do(x, pin, regime, ctx)
            ld0, ln0 = law64(z.cpu(), jac.cpu(), pinned)
            tol = 2e-6 * (ld0.abs() + ln0.abs()) + 2e-5 * d ** .5 + 2. ** -24 * (ld0 + ln0).abs()
            assert float(((lp.cpu().double() - (ld0 + ln0)).abs() - tol).max()) <= 0., case
            assert_close(lds, ld0, rtol=2e-6, atol=1e-5 * d ** .5, what="logdet " + case)
            assert_close(lns, ln0, rtol=2e-6, atol=1e-5 * d ** .5, what="logN " + case)
            assert_close(zs, z, what="z " + case)
            full = pinned.all(1)
            assert bool(full.any()) and bool((lp[cu(full)] == 0).all()), case
            # ---- gradients
            xa = x.clone().requires_grad_(True)
            loss = flow.loss_do(xa, pin, regime, ctx)
            assert type(loss.grad_fn).__name__ == "NllMeanFnBackward", case
            params = [q for q in flow.parameters() if q.requires_grad]
            got = torch.autograd.grad(loss, [xa] + params, allow_unused=True)
            xb = x.clone().requires_grad_(True)
            zz, jj = step.normalizer(xb, step.conditioner(xb, ctx), ctx)
            free = cu(~pinned)
            zero = torch.zeros((), device=DEV)
            ldc = torch.where(free, torch.log(torch.where(free, jj, zero + 1.)), zero).sum(1)
            lnc = -.5 * torch.where(free, LOG2PI + torch.where(free, zz, zero) ** 2, zero).sum(1)
            ref_loss = flow.constraintsLoss() - (ldc + lnc).mean()
            assert abs(loss.item() - ref_loss.item()) <= 1e-5 * max(1., abs(ref_loss.item())), case
            want = torch.autograd.grad(ref_loss, [xb] + params, allow_unused=True)
            names = ["x"] + [n for n, q in flow.named_parameters() if q.requires_grad]
            for n, a, b in zip(names, got, want):
                assert (a is None) == (b is None), (case, n)
                if a is not None:
                    assert rel_err(a.cpu(), b.cpu()) < GTOL, (case, n, rel_err(a.cpu(), b.cpu()))


@pytest.mark.parametrize("norm", ["affine", "spline", "monotonic"])
def test_poison_loss_do_step(norm):
    """a loss_do step of each normalizer under the three poison arms: values, loss and every gradient keep their bits"""
    def fn():
        out = {}
        for cond in ("MADE", "DAG"):
            flow = _flow(cond, norm, 6, 0, seed=3)
            x, ctx, pin, regime, _ = _case(40, 6, 0, seed=5)
            xa = x.clone().requires_grad_(True)
            loss = flow.loss_do(xa, pin, regime)
            loss.backward()
            out.update({cond + " loss": loss.detach(), cond + " gx": xa.grad})
            out.update({cond + " " + n: q.grad for n, q in flow.named_parameters() if q.grad is not None})
        return out
    three_arms(fn)


def test_affine_inplace_clamp_takes_the_composed_form():
    """AffineNormalizer.inplace_clamp rewrites h, which the masked kernel never does: forward_logdet_do then runs the
    normalizer's own forward and ops.NllDoFn.  The same numbers as the fused form to the row sums' bound; h comes back clamped."""
    d, B = 6, 40
    flow = _flow("MADE", "affine", d, 0, seed=1)
    nrm = flow.steps[0].normalizer
    x, _, pin, regime, _ = _case(B, d, 0, seed=9)
    g = torch.Generator().manual_seed(3)
    h = cu(torch.randn(B, d, 2, generator=g) * 4.)
    z0, ld0, ln0 = nrm.forward_logdet_do(x, h.clone(), pin, cu(regime).to(torch.int32))
    nrm.inplace_clamp = True
    hc = h.clone().requires_grad_(True)
    hv = hc * 1.                                           # (a non-leaf: the kernel writes into it)
    z1, ld1, ln1 = nrm.forward_logdet_do(x, hv, pin, cu(regime).to(torch.int32))
    assert_close(z1, z0, what="z")
    assert_close(ld1, ld0, rtol=2e-6, atol=1e-5 * d ** .5, what="logdet")
    assert_close(ln1, ln0, rtol=2e-6, atol=1e-5 * d ** .5, what="logN")
    assert float(hv.detach()[:, :, 0].abs().max()) <= 5. and float(hv.detach()[:, :, 1].max()) <= 2.
    assert float(h[:, :, 0].abs().max()) > 5.              # ... and there was something to clamp
    (ld1.sum() + ln1.sum()).backward()
    assert bool(torch.isfinite(hc.grad).all())
    with torch.no_grad():
        lp = flow.log_prob_do(x, pin, regime)
        nrm.inplace_clamp = False
        assert_close(lp, flow.log_prob_do(x, pin, regime), rtol=4e-6, atol=2e-5 * d ** .5, what="log_prob_do")


# --------------------------------------------------------------------------------------------- truncation is structural
def test_made_output_bias_of_a_pinned_variable_gets_exactly_no_gradient():
    d, B = 6, 40
    flow = _flow("MADE", "affine", d, 0, seed=1)
    x = cu(torch.randn(B, d, generator=torch.Generator().manual_seed(2)))
    pinned_vars = [1, 4]
    flow.loss_do(x, pinned_vars).backward()
    last = flow.steps[0].conditioner.masked_autoregressive_net.masked_layers()[-1]
    gb, gw = last.bias.grad.view(2, d), last.weight.grad.view(2, d, -1)        # output k of variable i is unit k d + i
    assert bool((gb[:, pinned_vars] == 0).all()) and bool((gw[:, pinned_vars] == 0).all())
    others = [i for i in range(d) if i not in pinned_vars]
    assert bool((gb[:, others] != 0).all())
    # a variable pinned in SOME rows only still trains on the others
    table_ = torch.zeros(2, d, dtype=torch.uint8)
    table_[1, 1] = 1
    flow.zero_grad()
    flow.loss_do(x, table_, torch.arange(B) % 2).backward()
    assert bool((last.bias.grad.view(2, d)[:, 1] != 0).all())


def test_dag_row_of_a_pinned_variable_gets_exactly_no_gradient():
    d, B = 6, 40
    for cond in ("DAG", "DAGstoch"):
        flow = _flow(cond, "affine", d, 0, seed=1)
        _fix_gate(flow, B, d, seed=7)
        x = cu(torch.randn(B, d, generator=torch.Generator().manual_seed(2)))
        A = flow.steps[0].conditioner.A
        # (the likelihood alone: the constraints term of loss_do -- l1 and acyclicity -- has a gradient in every row of A)
        (-flow.log_prob_do(x, [2, 5]).mean()).backward()
        assert bool((A.grad[[2, 5]] == 0).all()), cond
        free_rows = A.grad[[0, 1, 3, 4]]
        off_diag = ~torch.eye(d, dtype=torch.bool, device=DEV)[[0, 1, 3, 4]]
        assert bool((free_rows[off_diag] != 0).any()), cond


# ---------------------------------------------------------------------------------------------- consistency with sampling
@pytest.mark.parametrize("kind", ["MADE", "DAG"])
def test_forward_do_recovers_the_noise_of_an_interventional_sample(kind):
    """x = intervene(z, P, v): forward_do(x, P) returns z' with |z' - z| on the free columns within twice the step's own
    invert round-trip residual, and logn is the fp64 sum over the free columns of log N(z')"""
    d, B = 6, 64
    step = _flow(kind, "affine", d, 0, seed=4).steps[0]
    if kind == "DAG":                                      # fixed weights: a frozen 0 / 1 DAG in a random topological order
        cnd = step.conditioner
        gen = torch.Generator().manual_seed(d)
        perm = torch.randperm(d, generator=gen)
        A = torch.zeros(d, d)
        A[perm[:, None], perm[None, :]] = torch.tril((torch.rand(d, d, generator=gen) < .5).float(), -1)
        with torch.no_grad():
            cnd.A.copy_(cu(A))
        cnd.A.requires_grad = False
        cnd.invalidate_caches()
    gen = torch.Generator().manual_seed(11)
    z, v = cu(.7 * torch.randn(B, d, generator=gen)), cu(torch.randn(B, d, generator=gen))
    with torch.no_grad():
        residual = float((step(step.invert(z))[0] - z).abs().max())
        for P in ([0], [2, 3], [d - 1], [0, 2, 4]):
            x = step.intervene(z, P, v[:, P])
            assert torch.equal(x[:, P], v[:, P])
            z2, ld, ln = step.forward_do(x, P)
            free = [i for i in range(d) if i not in P]
            err = float((z2 - z)[:, free].abs().max())
            print("%s P=%s: |z' - z| on the free columns %.3e, invert round-trip residual %.3e" % (kind, P, err, residual))
            assert err <= 2. * residual, (kind, P, err, residual)
            pinned = torch.zeros(B, d, dtype=torch.bool)
            pinned[:, P] = True
            _, ln0 = law64(z2.cpu(), torch.ones(B, d), pinned)
            assert_close(ln, ln0, rtol=2e-6, atol=1e-5 * d ** .5, what="logN %s %s" % (kind, P))


# ------------------------------------------------------------------------------------------------------ training smoke
def _sem(n, seed):
    """x0 -> x1: x0 ~ N(0, 1), x1 = .8 x0 + .3 eps; odd rows are drawn under do(x1 = 2 + .1 eps')"""
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.randn(n, generator=gen)
    x1 = .8 * x0 + .3 * torch.randn(n, generator=gen)
    regime = torch.arange(n) % 2
    x1 = torch.where(regime == 1, 2. + .1 * torch.randn(n, generator=gen), x1)
    return cu(torch.stack((x0, x1), 1)), cu(regime)


def test_training_on_a_mix_of_regimes():
    from gnf_hip import dp
    targets = torch.tensor([[0, 0], [0, 1]], dtype=torch.uint8, device=DEV)
    flow = _flow("MADE", "affine", 2, 0, seed=0)
    state = dp.FlatState(flow)
    x, regime = _sem(512, seed=1)
    with torch.no_grad():
        before = flow.loss_do(x, targets, regime).item()
    for k in range(20):
        rows = torch.arange(k * 25, k * 25 + 128, device=DEV) % 512
        loss = dp.train_step(flow, state, x[rows], lr=1e-2, weight_decay=0., targets=targets, regime=regime[rows])
        assert torch.isfinite(loss).item()
    with torch.no_grad():
        after = flow.loss_do(x, targets, regime).item()
    print("loss_do: %.4f -> %.4f after 20 steps" % (before, after))
    assert after < before
    # a batch whose every row pins x1 leaves the parameters that only produce h_1 unchanged, bit for bit (fresh moments, no
    # weight decay: Adam's update of a zero gradient is zero)
    flow = _flow("MADE", "affine", 2, 0, seed=0)
    state = dp.FlatState(flow)
    last = flow.steps[0].conditioner.masked_autoregressive_net.masked_layers()[-1]
    w0, b0 = last.weight.detach().clone(), last.bias.detach().clone()
    every = x[regime == 1]
    dp.train_step(flow, state, every, lr=1e-2, weight_decay=0., targets=targets, regime=regime[regime == 1])
    torch.cuda.synchronize()
    for k in (0, 1):                                       # unit k d + i produces output k of variable i = 1
        assert torch.equal(bits(last.bias[2 * k + 1]), bits(b0[2 * k + 1]))
        assert torch.equal(bits(last.weight[2 * k + 1]), bits(w0[2 * k + 1]))
    assert not torch.equal(last.bias.detach()[[0, 2]], b0[[0, 2]])             # ... while those of h_0 moved


# --------------------------------------------------------------------------------------------------------------- API
def test_log_prob_is_forward_plus_the_base_density():
    for cond, norm in (("MADE", "affine"), ("DAG", "monotonic"), ("Coupling", "spline")):
        flow = _flow(cond, norm, 6, 2, seed=2)
        x, ctx, _, _, _ = _case(40, 6, 2, seed=3)
        with torch.no_grad():
            z, ld = flow(x, ctx)
            assert torch.equal(flow.log_prob(x, ctx), ld + flow.z_log_density(z))


@pytest.mark.parametrize("norm", ["affine", "spline", "monotonic"])
def test_host_empty_targets_are_the_existing_path_bit_for_bit(norm):
    from gnf_hip import ops
    flow = _flow("MADE", norm, 6, 0, seed=2)
    x, _, _, _, _ = _case(40, 6, 0, seed=3)
    with torch.no_grad():
        z, ld = flow(x)
        for empty in ([], (), torch.zeros(0, dtype=torch.long)):
            z2, ld2, ln2 = flow.steps[0].forward_do(x, empty)
            assert torch.equal(bits(z2), bits(z)) and torch.equal(bits(ld2), bits(ld))
            assert torch.equal(bits(ln2), bits(ops.NormalLogDensityFn.apply(z)))
            assert torch.equal(flow.log_prob_do(x, empty), flow.log_prob(x))
        # a DEVICE table of zeros takes the masked kernels: the same numbers to rounding
        lp = flow.log_prob_do(x, torch.zeros(6, dtype=torch.bool, device=DEV))
        assert_close(lp, flow.log_prob(x), rtol=4e-6, atol=2e-5 * 6 ** .5, what="zero table")
    xa = x.clone().requires_grad_(True)
    flow.loss_do(xa, []).backward()
    g1 = [q.grad.clone() for q in flow.parameters()]
    flow.zero_grad()
    xb = x.clone().requires_grad_(True)
    zb, ldb = flow(xb)
    (flow.constraintsLoss() - (ldb + flow.z_log_density(zb)).mean()).backward()
    assert rel_err(xa.grad.cpu(), xb.grad.cpu()) < 1e-5
    for a, q in zip(g1, flow.parameters()):
        assert rel_err(a.cpu(), q.grad.cpu()) < 1e-5


def test_accumulate_with_regimes_is_loss_do_backward():
    from gnf_hip import dp
    flow = _flow("DAG", "affine", 6, 2, seed=2)
    x, ctx, pin, regime, _ = _case(40, 6, 2, seed=3)
    loss = dp.accumulate(flow, x, context=ctx, targets=pin, regime=regime)
    got = [q.grad.clone() for q in flow.parameters()]
    flow.zero_grad()
    ref = flow.loss_do(x, pin, regime, ctx)
    ref.backward()
    assert torch.equal(bits(loss), bits(ref))
    for a, q in zip(got, flow.parameters()):
        assert torch.equal(bits(a), bits(q.grad))
    # scale = 1 / k, as for the plain loss
    flow.zero_grad()
    dp.accumulate(flow, x, scale=.5, context=ctx, targets=pin, regime=regime)
    for a, q in zip(got, flow.parameters()):
        assert rel_err(q.grad.cpu(), .5 * a.cpu()) < 1e-6
