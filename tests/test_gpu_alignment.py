"""GPU: every entry point on operands at dword-only alignment.

include/gnf_hip.h promises that an fp32 array may sit at any 4-byte-aligned address (a slice of a [n, 21] data set, a view into a
flat parameter buffer); 16-byte alignment only selects faster kernels.  Every other test of the suite hands the kernels fresh
allocations, i.e. 16-byte aligned bases.  Here each call is made on 16-byte aligned operands and again with each operand -- one
at a time, then all together -- placed 4, 8 and 12 bytes past a 16-byte boundary between guard bands (tests/misaligned.py), and
judged three ways:
  (a) against the high-precision reference and the tolerance of the op's existing (aligned) test;
  (b) bit for bit against the aligned call wherever the same kernel runs (a kernel whose arithmetic does not depend on the
      address must not change one bit when the address moves); where the dispatcher takes another family for a displaced
      pointer, that the family whose launch condition tests this pointer is NOT the one reported;
  (c) the guard bands of every placed operand -- inputs and caller-owned outputs -- are intact afterwards."""
import ctypes

import pytest
import torch

from conftest import rel_err, assert_close, assert_fwd
from misaligned import place, guards_intact
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5          # tests/test_gpu_parity.py
GTOL = 1e-4
OFFSETS = (1, 2, 3)


def _abi():
    from gnf_hip import abi
    return abi


def P(t):
    return _abi().ptr(t)


def call(name, *args):
    _abi().call(name, *args)


def stream():
    return _abi().stream()


def bits_equal(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def variants(names, offsets=OFFSETS):
    """{operand: offset}: each operand alone at each offset, then all of them together"""
    for n in names:
        for k in offsets:
            yield {n: k}
    if len(names) > 1:
        for k in offsets:
            yield {n: k for n in names}


class PtrSpy:
    """records the address of every tensor ops.py hands to a kernel, so that a test through an autograd Function can tell that
    the displaced operand really reached the library (and was not copied to a fresh allocation on the way)"""

    def __init__(self, monkeypatch):
        from gnf_hip import ops
        self.seen = set()
        orig = ops.ptr

        def ptr(t):
            if t is not None:
                self.seen.add(t.data_ptr())
            return orig(t)
        monkeypatch.setattr(ops, "ptr", ptr)


def sweep(operands, run, judge, names=None, offsets=OFFSETS, bitwise=True, spy=None, report=None):
    """operands: {name: device tensor or None}.  run(t) -> {key: tensor or str} on the placed operands t; judge(out, tag) checks
    (a).  bitwise: True / False / f(out, base, var) -> the keys to compare bit for bit with the aligned call.  -> aligned out."""
    names = [n for n in (names or operands) if operands[n] is not None]

    def go(var):
        t = {n: (None if v is None else place(v, var.get(n, 0))) for n, v in operands.items()}
        if spy is not None:
            spy.seen.clear()
        out = run(t)
        torch.cuda.synchronize()
        for n, v in t.items():
            if v is not None:
                assert guards_intact(v), "guard band of %s overwritten at offsets %s" % (n, var)            # (c)
                if spy is not None and n in var:
                    assert v.data_ptr() in spy.seen, "%s at offset %d never reached a kernel" % (n, var[n])
        return out

    base = go({})
    judge(base, "aligned")
    if report is not None:
        report("aligned", base)
    for var in variants(names, offsets):
        tag = " ".join("%s+%d" % nk for nk in var.items())
        out = go(var)
        judge(out, tag)                                                                                     # (a)
        if report is not None:
            report(tag, out)
        keys = bitwise(out, base, var) if callable(bitwise) else ([k for k in base if torch.is_tensor(base[k])] if bitwise else [])
        for key in keys:                                                                                    # (b)
            assert bits_equal(out[key], base[key]), "%s differs from the aligned call at %s (%d entries)" % (
                key, tag, int((out[key] != base[key]).sum()))
    return base


def fwd_close(a, ref, what):
    assert rel_err(a.cpu(), ref) < TOL, (what, rel_err(a.cpu(), ref))
    assert_fwd(a, ref, what=what)


# ================================================================================================== row-wise kernels
# (4162, 63), (8192, 32): B d >= 2^18, d <= 64 (the flat span kernels of the NLL backward; the forward reductions and the Affine
# normalizer take the 16-lane-group kernels there); (1041, 63): B d >= 2^16 (16-lane groups); (3, 257): a workgroup per row /
# a thread per element; (7, 5): the generic lane-group kernels
ROW_SHAPES = [(4162, 63), (8192, 32), (1041, 63), (3, 257), (7, 5)]


def _h(B, d, layout, g, scale=3.):
    if layout == "made":                                  # MADE's [B, 2 d] output viewed as [B, d, 2]: strides (2 d, 1, d)
        return (torch.randn(B, 2 * d, generator=g) * scale).view(B, 2, d).permute(0, 2, 1)
    return torch.randn(B, d, 2, generator=g) * scale


@pytest.mark.parametrize("layout", ["contig", "made"])
@pytest.mark.parametrize("B,d", ROW_SHAPES)
def test_affine_forward_backward_inverse(B, d, layout):
    g = torch.Generator().manual_seed(B + d)
    x, h = torch.randn(B, d, generator=g), _h(B, d, layout, g)
    gz, gj, gl, gn = (torch.randn(s, generator=g) for s in ((B, d), (B, d), (B,), (B,)))
    xr, hr = x.double().requires_grad_(True), h.double().requires_grad_(True)
    z0, j0 = O.affine_forward(xr, hr)
    ld0, ln0 = torch.log(j0).sum(1), O.normal_log_density(z0)
    gx0, gh0 = torch.autograd.grad((z0 * gz).sum() + (j0 * gj).sum() + (ld0 * gl).sum(), (xr, hr), retain_graph=True)
    gx1, gh1 = torch.autograd.grad((z0 * gz).sum() + (ld0 * gl).sum() + (ln0 * gn).sum(), (xr, hr), retain_graph=True)
    z0, j0, ld0, ln0 = (t.detach() for t in (z0, j0, ld0, ln0))
    dev = lambda *ts: [t.to(DEV) for t in ts]            # noqa: E731  (.to keeps the strides of the MADE view)
    empty_h = torch.empty_strided(h.shape, h.stride(), device=DEV)

    # ---- forward: x, h in; z, jac, logdet, logn out
    def fwd(t):
        hh = t["h"]
        call("gnf_affine_fwd", P(t["x"]), P(hh), hh.stride(0), hh.stride(1), hh.stride(2), P(t["z"]), P(t["jac"]), P(t["logdet"]),
             P(t["logn"]), 0, B, d, stream())
        return {k: t[k] for k in ("z", "jac", "logdet", "logn")}

    def judge_fwd(o, tag):
        fwd_close(o["z"], z0, "z " + tag)
        fwd_close(o["jac"], j0, "jac " + tag)
        fwd_close(o["logdet"], ld0, "logdet " + tag)
        assert_close(o["logn"], ln0, rtol=2e-6, atol=1e-4, what="logN " + tag)   # test_affine_fused_normal_log_density
    xd, hd = dev(x, h)
    assert hd.stride() == h.stride()
    sweep({"x": xd, "h": hd, "z": torch.empty(B, d, device=DEV), "jac": torch.empty(B, d, device=DEV),
           "logdet": torch.empty(B, device=DEV), "logn": torch.empty(B, device=DEV)}, fwd, judge_fwd,
          bitwise=True)                                  # no launch condition of the forward reads a pointer

    # ---- backward with the cotangents of z, jac, log|det J| (test_affine_flat_vectorised_path_vs_oracle) ...
    def bwd(t):
        hh, gh = t["h"], t["gh"]
        call("gnf_affine_bwd", P(t["x"]), P(hh), hh.stride(0), hh.stride(1), hh.stride(2), P(t["gz"]), P(t["gjac"]), P(t["glogdet"]),
             P(t["glogn"]), P(t["gx"]), P(gh), gh.stride(0), gh.stride(1), gh.stride(2), B, d, stream())
        return {"gx": t["gx"], "gh": t["gh"]}

    def judge_bwd(o, tag):
        fwd_close(o["gx"], gx0, "gx " + tag)
        fwd_close(o["gh"], gh0, "gh " + tag)
    gzd, gjd, gld, gnd = dev(gz, gj, gl, gn)
    sweep({"x": xd, "h": hd, "gz": gzd, "gjac": gjd, "glogdet": gld, "glogn": None, "gx": torch.empty(B, d, device=DEV),
           "gh": empty_h}, bwd, judge_bwd)

    # ---- ... and with that of the fused Normal log-density (test_affine_fused_normal_log_density: GTOL)
    def judge_bwd_n(o, tag):
        assert rel_err(o["gx"].cpu(), gx1) < GTOL and rel_err(o["gh"].cpu(), gh1) < GTOL, tag
    sweep({"x": xd, "h": hd, "gz": gzd, "gjac": None, "glogdet": gld, "glogn": gnd, "gx": torch.empty(B, d, device=DEV),
           "gh": empty_h}, bwd, judge_bwd_n, names=["h", "glogn", "gh"], offsets=(1, 2))

    # ---- inverse
    xi0 = O.affine_inverse(z0.float().double(), h.double())

    def inv(t):
        hh = t["h"]
        call("gnf_affine_inv", P(t["z"]), P(hh), hh.stride(0), hh.stride(1), hh.stride(2), P(t["x"]), B, d, stream())
        return {"x": t["x"]}
    sweep({"z": z0.float().to(DEV), "h": hd, "x": torch.empty(B, d, device=DEV)}, inv,
          lambda o, tag: assert_fwd(o["x"], xi0, what="x " + tag))


@pytest.mark.parametrize("B,d", ROW_SHAPES)
def test_row_reductions_and_losses(B, d):
    g = torch.Generator().manual_seed(B + d)
    z, jac = torch.randn(B, d, generator=g), torch.rand(B, d, generator=g) * 3 + .05
    gl, gn, gzin = torch.randn(B, generator=g), torch.randn(B, generator=g), torch.randn(B, d, generator=g)
    zr, jr = z.double().requires_grad_(True), jac.double().requires_grad_(True)
    ld0, ln0 = torch.log(jr).sum(1), O.normal_log_density(zr)
    gz0, gj0 = torch.autograd.grad((ld0 * gl).sum() + (ln0 * gn).sum(), (zr, jr), retain_graph=True)
    ld0, ln0 = ld0.detach(), ln0.detach()
    zd, jd, gld, gnd, gzind = (t.to(DEV) for t in (z, jac, gl, gn, gzin))
    row, mat = (lambda: torch.empty(B, device=DEV)), (lambda: torch.empty(B, d, device=DEV))
    at = 1e-5 * d ** .5                                   # test_nll_reduce_vs_torch

    def judge_rows(o, tag):
        if "logdet" in o:
            assert_close(o["logdet"], ld0, rtol=2e-6, atol=at, what="logdet " + tag)
        if "logn" in o:
            assert_close(o["logn"], ln0, rtol=2e-6, atol=at, what="logN " + tag)

    def judge_grads(o, tag):
        if "gz" in o:
            assert_close(o["gz"], gz0, rtol=1e-6, atol=1e-7, what="gz " + tag)
        if "gjac" in o:
            assert_close(o["gjac"], gj0, rtol=2e-6, atol=1e-7, what="gjac " + tag)

    def reduce_fwd(t):
        call("gnf_nll_reduce_fwd", P(t["z"]), P(t["jac"]), P(t["logdet"]), P(t["logn"]), B, d, stream())
        return {"logdet": t["logdet"], "logn": t["logn"]}
    base = sweep({"z": zd, "jac": jd, "logdet": row(), "logn": row()}, reduce_fwd, judge_rows)
    # the backward takes the flat span kernels when every pointer is 16-byte aligned and the lane-group ones otherwise: another
    # family, (a) only
    same = not (d <= 64 and B * d >= 1 << 18)

    def reduce_bwd(t):
        call("gnf_nll_reduce_bwd", P(t["z"]), P(t["jac"]), P(t["glogdet"]), P(t["glogn"]), P(t["gz_in"]), P(t["gz"]), P(t["gjac"]), B, d,
             stream())
        return {"gz": t["gz"], "gjac": t["gjac"]}
    sweep({"z": zd, "jac": jd, "glogdet": gld, "glogn": gnd, "gz_in": None, "gz": mat(), "gjac": mat()}, reduce_bwd, judge_grads,
          bitwise=same)
    # gz_in: an incoming cotangent of z the launch adds to its own.  No aligned test passes one; the bound is the sum's own:
    # gz_in + (-z glogn) in fp32 is at most two roundings, each half an ulp (2^-24) of a term's magnitude, on top of the bound
    # of the plain call (where the two nearly cancel the result is far smaller than the terms' roundings)
    gz_in_ref = gz0 + gzin.double()
    gz_in_tol = 1e-6 * gz_in_ref.abs() + 1e-7 + 2. ** -23 * (gz0.abs() + gzin.double().abs())

    def judge_gz_in(o, tag):
        judge_grads({"gjac": o["gjac"]}, tag)
        excess = (o["gz"].cpu().double() - gz_in_ref).abs() - gz_in_tol
        assert float(excess.max()) <= 0., ("gz with gz_in " + tag, float(excess.max()))
    sweep({"z": zd, "jac": jd, "glogdet": gld, "glogn": gnd, "gz_in": gzind, "gz": mat(), "gjac": mat()}, reduce_bwd,
          judge_gz_in, names=["gz_in", "gz"], bitwise=same)

    # the stand-alone entry points (the same kernels with one array absent)
    def logsum_fwd(t):
        call("gnf_logsum_rows_fwd", P(t["jac"]), P(t["out"]), B, d, stream())
        return {"logdet": t["out"]}
    o = sweep({"jac": jd, "out": row()}, logsum_fwd, judge_rows)
    assert bits_equal(o["logdet"], base["logdet"])

    def logsum_bwd(t):
        call("gnf_logsum_rows_bwd", P(t["jac"]), P(t["g"]), P(t["gjac"]), B, d, stream())
        return {"gjac": t["gjac"]}
    sweep({"jac": jd, "g": gld, "gjac": mat()}, logsum_bwd, judge_grads, bitwise=same)

    def logn_fwd(t):
        call("gnf_normal_logdensity_fwd", P(t["z"]), P(t["out"]), B, d, stream())
        return {"logn": t["out"]}
    o = sweep({"z": zd, "out": row()}, logn_fwd, judge_rows)
    assert bits_equal(o["logn"], base["logn"])

    def logn_bwd(t):
        call("gnf_normal_logdensity_bwd", P(t["z"]), P(t["g"]), P(t["gz"]), B, d, stream())
        return {"gz": t["gz"]}
    sweep({"z": zd, "g": gnd, "gz": mat()}, logn_bwd, judge_grads, bitwise=same)

    # ---- batch mean of the two reductions, and its cotangents (-g / B, exact up to the division's rounding)
    c, gout = torch.randn((), generator=g), torch.randn((), generator=g)
    ldf, lnf = ld0.float(), ln0.float()
    mean0 = c.double() - (ldf.double() + lnf.double()).mean()

    def mean_fwd(t):
        call("gnf_nll_mean_fwd", P(t["logdet"]), P(t["logn"]), P(t["addend"]), P(t["out"]), B, stream())
        return {"out": t["out"]}
    # a fixed-order sum of 2 B fp32 terms: the scalar bound of test_nll_loss_entry_points_vs_torch
    sweep({"logdet": ldf.to(DEV), "logn": lnf.to(DEV), "addend": c.to(DEV), "out": torch.empty((), device=DEV)}, mean_fwd,
          lambda o, tag: abs(o["out"].item() - mean0.item()) <= 2e-6 * max(1., abs(mean0.item())) or pytest.fail(
              "nll_mean %s: %r vs %r" % (tag, o["out"].item(), mean0.item())))

    def mean_bwd(t):
        call("gnf_nll_mean_bwd", P(t["g"]), P(t["glogdet"]), P(t["glogn"]), B, stream())
        return {"glogdet": t["glogdet"], "glogn": t["glogn"]}
    want = torch.full((B,), -gout.double().item() / B, dtype=torch.float64)
    sweep({"g": gout.to(DEV), "glogdet": row(), "glogn": row()}, mean_bwd,
          lambda o, tag: (assert_close(o["glogdet"], want, rtol=1e-6, atol=0., what="glogdet " + tag),
                          assert_close(o["glogn"], want, rtol=1e-6, atol=0., what="glogn " + tag)))

    # ---- the one-launch loss: z read as float4 when it is 16-byte aligned, element by element when not
    z13 = z * 1.3
    zr2, lr2 = z13.double().requires_grad_(True), ldf.double().requires_grad_(True)
    loss0 = c.double() - (lr2 + O.normal_log_density(zr2)).mean()
    gz2, gl2 = torch.autograd.grad(loss0 * gout.double(), (zr2, lr2))

    def loss_fwd(t):
        call("gnf_nll_loss_fwd", P(t["z"]), P(t["logdet"]), P(t["addend"]), P(t["out"]), B, d, stream())
        return {"out": t["out"]}
    sweep({"z": z13.to(DEV), "logdet": ldf.to(DEV), "addend": c.to(DEV), "out": torch.empty((), device=DEV)}, loss_fwd,
          lambda o, tag: abs(o["out"].item() - loss0.item()) <= 2e-6 * max(1., abs(loss0.item())) or pytest.fail(
              "nll_loss %s: %r vs %r" % (tag, o["out"].item(), loss0.item())), bitwise=False)

    def loss_bwd(t):
        call("gnf_nll_loss_bwd", P(t["g"]), P(t["z"]), P(t["gz"]), P(t["glogdet"]), B, d, stream())
        return {"gz": t["gz"], "glogdet": t["glogdet"]}
    sweep({"g": gout.to(DEV), "z": z13.to(DEV), "gz": mat(), "glogdet": row()}, loss_bwd,
          lambda o, tag: (assert_close(o["gz"], gz2, rtol=1e-6, atol=1e-9, what="gz " + tag),
                          assert_close(o["glogdet"], gl2, rtol=1e-6, atol=1e-12, what="glogdet " + tag)))


@pytest.mark.parametrize("M,N,lda", [(1000, 37, 37), (9001, 5, 5), (700, 33, 41)])
def test_colsum(M, N, lda):
    """contiguous rows (the row-sum kernels, two-level above 8192 rows) and strided rows (the two-stage kernels)"""
    lib = _abi().load()
    g = torch.Generator().manual_seed(M + N)
    full = torch.randn(M, lda, generator=g)
    a = full[:, :N]
    ref, mag = a.double().sum(0), a.double().abs().sum(0)
    a_dev = full.to(DEV)[:, :N]                           # (sliced on the device: .to() of a padded view would pack its rows)
    assert a_dev.stride() == (lda, 1)
    nws = int(lib.gnf_colsum_ws_bytes(M, N))

    def run(t):
        call("gnf_colsum", P(t["a"]), lda, P(t["out"]), M, N, P(t["ws"]), stream())
        return {"out": t["out"]}

    def judge(o, tag):
        # fp32 sums of M terms in a fixed tree order: the bound of tests/fuzz_gemm.py on a contraction (2e-6 of the summed
        # term magnitudes)
        assert float(((o["out"].double().cpu() - ref).abs() / (2e-6 * mag + 1e-30)).max()) <= 1., tag
    sweep({"a": a_dev, "out": torch.empty(N, device=DEV), "ws": torch.empty(max(nws // 4, 1), device=DEV)}, run, judge)


# ================================================================================================== Adam
def _adam64(p, g, m, v, t, lr, b1, b2, eps, wd):
    gi = g + wd * p
    m = b1 * m + (1 - b1) * gi
    v = b2 * v + (1 - b2) * gi * gi
    p = p - lr / (1 - b1 ** t) * (m / (v.sqrt() / (1 - b2 ** t) ** .5 + eps))
    return p, m, v


@pytest.mark.parametrize("entry", ["gnf_adam_step", "gnf_adam_step_dev"])
@pytest.mark.parametrize("n", [8 * 1024 + 5, 3])
def test_adam_three_steps(n, entry):
    """both Adam entry points, three steps (m and v are read back), each of p, g, m, v displaced alone -- the launcher then
    takes the element-by-element form of the kernel -- against fp64 Adam at the bounds of test_hip_adam_vs_torch_adam_on_device"""
    from gnf_hip import ops
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * 10. ** (i - 2) for i in range(3)]
    wd, lr = 1e-5, 1e-3
    p6, m6, v6 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t, g in enumerate(grads, 1):
        p6, m6, v6 = _adam64(p6, g.double(), m6, v6, t, lr, .9, .999, 1e-8, wd)
    operands = {"p": p0.to(DEV), "m": torch.zeros(n, device=DEV), "v": torch.zeros(n, device=DEV)}
    operands.update({"g%d" % i: g.to(DEV) for i, g in enumerate(grads)})

    def run(t):
        step_dev = torch.zeros(2, dtype=torch.int32, device=DEV)
        for i in range(3):
            if entry == "gnf_adam_step":
                ops.adam_step(t["p"], t["g%d" % i], t["m"], t["v"], i + 1, lr=lr, weight_decay=wd)
            else:
                ops.adam_step_dev(t["p"], t["g%d" % i], t["m"], t["v"], step_dev, lr=lr, weight_decay=wd)
        assert entry == "gnf_adam_step" or step_dev.tolist() == [3, 0]
        return {k: t[k] for k in ("p", "m", "v")}

    def judge(o, tag):
        assert_close(o["p"], p6, rtol=1e-6, atol=1e-6, what="p " + tag)
        assert_close(o["m"], m6, rtol=2e-6, atol=2e-5, what="exp_avg " + tag)
        assert_close(o["v"], v6, rtol=2e-6, atol=2e-5, what="exp_avg_sq " + tag)
    # (the launcher picks the float4 or the element-by-element form from the four pointers: (a) and (c))
    sweep(operands, run, judge, bitwise=False)


# ================================================================================================== GEMM
# the pointers each dedicated family's launch condition tests (gnf_gemm.hip, gnf_gemm_split.hip)
GEMM_CHECKS = {"gemm_tall_k": {"A", "B"}, "gemm_wide_k": {"A", "B"}, "gemm_kmajor_k": {"A", "B"},
               "gemm_split_tall_k": {"A"}, "gemm_split_wide_k": {"A", "C"}, "gemm_split_kmajor_k": {"B", "C"}}
KERNELS_SEEN = {}


def _mat(rows, cols, layout, pad, gen, scale=1.):
    """[rows, cols] device view, row-major ('r') or column-major ('c'), `pad` extra elements in the leading stride"""
    if layout == "r":
        return (torch.randn(rows, cols + pad, generator=gen) * scale).to(DEV)[:, :cols]
    return (torch.randn(cols, rows + pad, generator=gen) * scale).to(DEV)[:, :rows].t()


def _gemm_case(name, M, N, K, la, lb, pads=(0, 0, 0), bias=False, relu=False, bmask=False, cmask=False, gate=False, ws="f32",
               expect=None, offsets=OFFSETS, entry="gnf_gemm"):
    lib = _abi().load()
    gen = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    sc = K ** -.25
    A, B, C = _mat(M, K, la, pads[0], gen, sc), _mat(K, N, lb, pads[1], gen, sc), _mat(M, N, "r", pads[2], gen)
    ops_ = {"A": A, "B": B, "C": C, "bias": torch.randn(N, generator=gen).to(DEV) if bias else None,
            "Bmask": (torch.empty_strided(B.shape, B.stride(), device=DEV).copy_((_mat(K, N, lb, pads[1], gen) > -.5).float())
                      if bmask else None),
            "Cmask": (torch.rand(M, N, generator=gen) < .7).float().to(DEV) if cmask else None,
            "gate": torch.randn(M, N, generator=gen).to(DEV) if gate else None}
    Bm = B.double() * (ops_["Bmask"].double() if bmask else 1.)
    ref, mag = A.double() @ Bm, A.double().abs() @ Bm.abs()
    if bias:
        ref, mag = ref + ops_["bias"].double(), mag + ops_["bias"].double().abs()
    if cmask:
        ref = ref * ops_["Cmask"].double()
    if relu:
        ref = torch.relu(ref)
    if gate:
        ref = ref * (ops_["gate"].double() > 0)
    tol = 2e-6 * mag + 1e-30                               # tests/fuzz_gemm.py
    if entry == "gnf_gemm":
        nws = int(lib.gnf_gemm_f32_ws_bytes(M, N, K) if ws == "f32" else lib.gnf_gemm_ws_bytes(M, N, K))
    else:
        nws = int(lib.gnf_gemm_split_ws_bytes(M, N, K))
    w = torch.empty(max(nws, 16), dtype=torch.uint8, device=DEV)
    st = lambda t: t.stride() if t is not None else (0, 0)         # noqa: E731

    def run(t):
        a, b, c = t["A"], t["B"], t["C"]
        if entry == "gnf_gemm":
            call("gnf_gemm", P(a), *a.stride(), P(b), P(t["Bmask"]), *b.stride(), P(c), *c.stride(), P(t["bias"]), P(t["Cmask"]),
                 *st(t["Cmask"]), P(t["gate"]), *st(t["gate"]), 1 if relu else 0, M, N, K, _abi().rawptr(w) if nws else None, nws,
                 stream())
            kern = lib.gnf_gemm_last_kernel().decode()
        else:
            call("gnf_gemm_split_bf16", P(a), *a.stride(), P(b), *b.stride(), P(c), *c.stride(), P(t["bias"]), 1 if relu else 0,
                 M, N, K, 0, 1, 0, _abi().rawptr(w), nws, stream())
            kern = lib.gnf_gemm_split_last_kernel().decode()
        return {"C": c, "kernel": kern}

    def judge(o, tag):
        worst = float(((o["C"].double() - ref).abs() / tol).max())
        assert worst <= 1., "%s %s (%s): err/tol %.2f" % (name, tag, o["kernel"], worst)

    def same_kernel(o, base, var):
        k0, k1 = base["kernel"], o["kernel"]
        checked = GEMM_CHECKS.get(k0, set()) & set(var)
        if not checked:
            assert k1 == k0, "%s: %s instead of %s although no pointer it tests moved (%s)" % (name, k1, k0, var)
        assert not (GEMM_CHECKS.get(k1, set()) & set(var)), "%s: %s ran on a displaced %s" % (name, k1, sorted(var))
        return ["C"] if k1 == k0 else []
    base = sweep(ops_, run, judge, bitwise=same_kernel, offsets=offsets,
                 report=lambda tag, o: KERNELS_SEEN.setdefault(name, []).append((tag, o["kernel"])))
    if expect is not None:
        assert base["kernel"] == expect, (name, base["kernel"])
    print("ALIGN %s: %s" % (name, "; ".join("%s -> %s" % tk for tk in KERNELS_SEEN[name])))


def test_gemm_tall_family():
    """the smallest shape tests/fuzz_gemm.py draws for gemm_tall_k that reaches it (a tile height must fill the chip)"""
    _gemm_case("tall", 78400, 97, 256, "r", "c", bias=True, relu=True, expect="gemm_tall_k", offsets=(1, 2))


def test_gemm_wide_family():
    _gemm_case("wide", 7777, 1000, 128, "r", "r", expect="gemm_wide_k", offsets=(1, 2))


def test_gemm_kmajor_family():
    _gemm_case("kmajor", 4, 512, 16384, "c", "r", expect="gemm_kmajor_k")


@pytest.mark.parametrize("la,lb", [("r", "r"), ("r", "c"), ("c", "r"), ("c", "c")])
def test_gemm_vector_tiles_with_every_epilogue(la, lb):
    """gemm_vec_k ("only dword alignment is assumed") in each operand order, odd leading strides, every epilogue operand"""
    _gemm_case("vec_%s%s" % (la, lb), 70, 65, 36, la, lb, pads=(1, 3, 1), bias=True, relu=True, bmask=True, cmask=True, gate=True,
               expect="gemm_vec_k<64,64>")


def test_gemm_split_k():
    _gemm_case("split_k", 60, 70, 2052, "r", "c", pads=(1, 0, 0), bias=True, gate=True)


SPLIT_CASES = [("split_tall", 10240, 65, 256, "r", "c", "gemm_split_tall_k"), ("split_wide", 10240, 512, 128, "r", "r", "gemm_split_wide_k"),
               ("split_kmajor", 16, 512, 16384, "c", "r", "gemm_split_kmajor_k")]


@pytest.mark.parametrize("name,M,N,K,la,lb,expect", SPLIT_CASES + [("split_general", 70, 65, 100, "r", "c", "gemm_split_k")])
def test_gemm_split_bf16_entry(name, M, N, K, la, lb, expect):
    """the split-bf16 kernels through their own entry point: the three dedicated families (smallest eligible shapes of
    tests/test_gpu_split.py) and the general kernel"""
    _gemm_case(name + "/gnf_gemm_split_bf16", M, N, K, la, lb, expect=expect, offsets=(1, 2), entry="gnf_gemm_split_bf16")


@pytest.mark.parametrize("name,M,N,K,la,lb,expect", SPLIT_CASES)
def test_gemm_dispatches_to_the_split_families(name, M, N, K, la, lb, expect):
    """gnf_gemm with a workspace of gnf_gemm_ws_bytes, as ops.gemm passes it: the dedicated split-bf16 kernels where the switch
    is on (the default), the fp32-MFMA families where GNF_TRUE_F32=1 turned it off"""
    on = bool(_abi().load().gnf_gemm_split_enabled())
    f32 = {"split_tall": None, "split_wide": "gemm_wide_k", "split_kmajor": "gemm_kmajor_k"}[name]
    _gemm_case(name + "/gnf_gemm", M, N, K, la, lb, ws="full", expect=expect if on else f32, offsets=(1, 2))


def test_gemm_random_walk_with_base_offsets():
    """the walk of test_gemm_random_shapes (same seed: same shapes, layouts, epilogues, values) with a base offset of 0..3 floats
    drawn for every operand"""
    import fuzz_gemm
    res = fuzz_gemm.walk(16, 2, offset_seed=11)
    bad = [(case, desc, worst) for case, desc, worst, b in res if b]
    assert not bad, bad
    for _, desc, _, _ in res:
        print("ALIGN walk:", desc)


# ================================================================================================== linear layers
def _linear_case(M, K, N, mask_kind, spy, offsets, frozen=None):
    """one Linear on a ReLU output (relu_in: the data gradient is gated by x > 0, so `gate` IS the displaced x) through
    ops.mlp, forward and backward, against fp64 at the bounds of tests/fuzz_linear.py"""
    from gnf_hip import ops
    g = torch.Generator().manual_seed(1000 * M + 10 * K + N)
    x = torch.relu(torch.randn(M, K, generator=g)) + (torch.rand(M, K, generator=g) < .5).float() * .01
    W, b = torch.randn(N, K, generator=g) / K ** .5, torch.randn(N, generator=g) * .1
    gy = torch.randn(M, N, generator=g)
    din, dout = torch.randint(0, 9, (K,), generator=g).float(), torch.randint(0, 9, (N,), generator=g).float()
    mask = None
    if mask_kind == "full":
        mask = (torch.rand(N, K, generator=g) < .6).float()
    elif mask_kind == "deg":
        mask = (din[None, :] <= dout[:, None]).float()
    xr, Wr, br = (t.double().requires_grad_(True) for t in (x, W, b))
    y0 = torch.nn.functional.linear(xr, Wr * mask.double() if mask is not None else Wr, br)
    gx0, gW0, gb0 = torch.autograd.grad((y0 * gy.double()).sum(), (xr, Wr, br))
    gx0 = gx0 * (x > 0)
    y0 = y0.detach()
    operands = {"x": x.to(DEV), "W": W.to(DEV), "b": b.to(DEV), "gy": gy.to(DEV), "mask": None if mask is None else mask.to(DEV),
                "deg_out": dout.to(DEV) if mask_kind == "deg" else None, "deg_in": din.to(DEV) if mask_kind == "deg" else None}

    live = [k for k in ("x", "W", "b") if not (frozen == "input" and k == "x") and not (frozen == "weights" and k != "x")]

    def run(t):
        leaves = [t[k].requires_grad_(True) for k in live]              # frozen: gnf_linear_bwd_w / gnf_linear_bwd_x alone
        y = ops.mlp(t["x"], [(t["W"], t["b"])], [t["mask"]] if mask is not None else None, relu_in=True,
                    degs=[(t["deg_out"], t["deg_in"], False)] if mask_kind == "deg" else None)
        grads = torch.autograd.grad(y, leaves, grad_outputs=t["gy"])
        return dict(zip(["g" + k for k in live], grads), y=y.detach())

    def judge(o, tag):
        what = "M %d K %d N %d %s %s: " % (M, K, N, mask_kind, tag)
        e = rel_err(o["y"].cpu(), y0)
        assert e < 2e-5, what + "y %.2e" % e
        for k, r in (("gx", gx0), ("gW", gW0), ("gb", gb0)):
            if k in o:
                e = rel_err(o[k].cpu(), r)
                assert e < 1e-4, what + "%s %.2e" % (k, e)
        if mask is not None and "gW" in o:
            assert int(((o["gW"].cpu() != 0) & (mask == 0)).sum()) == 0, what + "gW non-zero under the mask"
    # no launch condition of the linear entry points reads a pointer; the tall-layer kernels choose their x / a load by it
    # (a 16-byte load or the descriptor's) and nothing else: the same bits at every offset
    sweep(operands, run, judge, offsets=offsets, spy=spy)


LIN_KN = [(K, N) for K in (16, 64, 128, 20, 100) for N in (30, 33, 64)]


@pytest.mark.parametrize("mask_kind", ["none", "full", "deg"])
@pytest.mark.parametrize("M", [100, 129, 2047, 2049])
def test_linear_layers(M, mask_kind, monkeypatch):
    """M = 100: the small-batch kernels; 129, 2047: the tall forward alone; 2049: the tall forward and backward (both without a
    mask; with one the tiled GEMM).  K = 16, 64, 128 are the exact-K instantiations of the tall kernels (16-byte loads of x / a
    rows when the base allows), 20 and 100 the descriptor ones."""
    spy = PtrSpy(monkeypatch)
    for K, N in LIN_KN:
        _linear_case(M, K, N, mask_kind, spy, OFFSETS if (mask_kind == "none" and K in (16, 64, 128)) else (1, 2))


@pytest.mark.parametrize("frozen", ["input", "weights"])
@pytest.mark.parametrize("M", [100, 2049])
def test_linear_single_gradient_entries(M, frozen, monkeypatch):
    """a layer whose input (weights) wants no gradient: the weight-gradient (data-gradient) entry point alone"""
    spy = PtrSpy(monkeypatch)
    for K, N in [(64, 64), (20, 33)]:
        for mask_kind in ("none", "full"):
            _linear_case(M, K, N, mask_kind, spy, (1, 2), frozen=frozen)


def test_linear_chain_with_hidden_layers(monkeypatch):
    """a three-layer chain on the tall kernels with tests/fuzz_linear.py's knife-edge redraw: the displaced x feeds layer 1, the
    displaced cotangent layer 3, every W and b its own layer"""
    import fuzz_linear
    from gnf_hip import ops
    spy = PtrSpy(monkeypatch)
    M, dims = 2049, [64, 128, 64, 30]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, dims[0], generator=g)
    layers = [(torch.randn(n, k, generator=g) / k ** .5, torch.randn(n, generator=g) * .1) for k, n in zip(dims, dims[1:])]
    x, _ = fuzz_linear.redraw_off_ties(x, layers, [], g)
    gy = torch.randn(M, dims[-1], generator=g)
    xr = x.double().requires_grad_(True)
    ps = [p.double().requires_grad_(True) for Wb in layers for p in Wb]
    a = xr
    for l in range(3):
        a = torch.nn.functional.linear(a, ps[2 * l], ps[2 * l + 1])
        a = torch.relu(a) if l < 2 else a
    ref = torch.autograd.grad((a * gy.double()).sum(), [xr] + ps)
    y0 = a.detach()
    names = ["x"] + ["%s%d" % (s, l) for l in range(3) for s in "Wb"]
    operands = dict(zip(names, [x.to(DEV)] + [p.to(DEV) for Wb in layers for p in Wb]), gy=gy.to(DEV))

    def run(t):
        leaves = [t[n].requires_grad_(True) for n in names]
        y = ops.mlp(leaves[0], [(leaves[1 + 2 * l], leaves[2 + 2 * l]) for l in range(3)])
        grads = torch.autograd.grad(y, leaves, grad_outputs=t["gy"])
        return dict(zip(["g" + n for n in names], grads), y=y.detach())

    def judge(o, tag):
        assert rel_err(o["y"].cpu(), y0) < 2e-5, tag
        for n, r in zip(names, ref):
            assert rel_err(o["g" + n].cpu(), r) < 1e-4, (tag, n, rel_err(o["g" + n].cpu(), r))
    sweep(operands, run, judge, offsets=(1, 2), spy=spy)


# ================================================================================================== Monotonic normalizer
MONO_C, MONO_S = 3, 20


def _mono_setup(hidden, B, d):
    """a seeded normalizer and inputs, knife-edge elements redrawn as in tests/fuzz_mono.py -> (params, x, h, layers)"""
    from conftest import integrand_knife_elements
    from knife_units import resample_off_ties
    from models import MonotonicNormalizer
    torch.manual_seed(sum(hidden) + B)
    norm = MonotonicNormalizer(hidden, MONO_C, nb_steps=MONO_S, solver="CC")
    ps = [p.detach().clone() for p in norm.integrand_net.flat_params()]
    layers = [(ps[i], ps[i + 1]) for i in range(0, len(ps), 2)]
    draw = lambda: (torch.randn(B, d) * 1.5, torch.randn(B, d, MONO_C))          # noqa: E731
    (x, h), _ = resample_off_ties(draw, lambda x_, h_: integrand_knife_elements(x_, h_, layers, MONO_S))
    return ps, x, h, layers


def _mono_net(t, nl):
    """gnf_mono_net over the placed parameters W0, b0, ... of t"""
    abi = _abi()
    net = abi.MonoNet()
    net.nl = nl
    net.dims[0] = t["W0"].shape[1]
    for l in range(nl):
        net.dims[l + 1] = t["W%d" % l].shape[0]
        net.W[l], net.b[l] = P(t["W%d" % l]).value, P(t["b%d" % l]).value
    return net


def _mono_pack(net):
    from gnf_hip import ops
    return ops._mono_pack(net, torch.empty(1, device=DEV))          # (an allocation of its own: 16-byte aligned)


MONO_NETS = {"narrow": [50, 50, 50], "wide": [128, 128, 128]}
MONO_SIZES = [(293, 7), (7, 1)]            # B d = 2051 (>= 2048 elements: d W1 on the tall weight-gradient kernels) and 7


@pytest.mark.parametrize("f32", [False, True], ids=["split", "f32"])
@pytest.mark.parametrize("B,d", MONO_SIZES)
@pytest.mark.parametrize("net_kind", ["narrow", "wide"])
def test_monotonic_forward_and_inverse(net_kind, B, d, f32):
    """forward (the split-bf16 kernels and the fp32-MFMA ones, as tests/test_gpu_mono_split.py selects them), inverse and
    scattered inverse; x / z, h in both layouts, every parameter, every output displaced"""
    from gnf_hip import ops
    lib = _abi().load()
    hidden = MONO_NETS[net_kind]
    ps, x, h, layers = _mono_setup(hidden, B, d)
    nl = len(layers)
    l64 = [(W.double(), b.double()) for W, b in layers]
    z0, j0 = O.monotonic_forward(x.double(), h.double(), l64, MONO_S)
    w, tt = ops.cc_rule(MONO_S, DEV)
    pnames = ["%s%d" % (s, l) for l in range(nl) for s in "Wb"]
    pdev = dict(zip(pnames, [p.to(DEV) for p in ps]))
    entry = "gnf_monotonic_fwd_f32" if f32 else "gnf_monotonic_fwd"
    kernels = set()

    for layout in ("contig", "made"):
        hd = h.to(DEV) if layout == "contig" else h.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1)
        kernels.clear()

        def fwd(t):
            net = _mono_net(t, nl)
            pack = _mono_pack(net)
            hh = t["h"]
            call(entry, P(pack), ctypes.byref(net), P(t["x"]), P(hh), hh.stride(0), hh.stride(1), hh.stride(2), P(w), P(tt), MONO_S,
                 P(t["z"]), P(t["jac"]), B, d, stream())
            kernels.add(lib.gnf_monotonic_fwd_kernel().decode())
            return {"z": t["z"], "jac": t["jac"]}

        def judge(o, tag):
            assert rel_err(o["z"].cpu(), z0) < TOL and rel_err(o["jac"].cpu(), j0) < TOL, (tag, rel_err(o["z"].cpu(), z0))
        operands = dict(pdev, x=x.to(DEV), h=hd, z=torch.empty(B, d, device=DEV), jac=torch.empty(B, d, device=DEV))
        sweep(operands, fwd, judge, names=["x", "h", "z", "jac"])
        sweep(operands, fwd, judge, names=pnames, offsets=(1, 2))
        assert len(kernels) == 1, kernels                 # no launch condition reads a pointer: one kernel at every offset

        if f32:
            continue                                      # (the inverse has one form)
        zt = z0.float()
        x0 = O.monotonic_inverse(zt.double(), h.double(), l64, MONO_S)

        def inv(t):
            net = _mono_net(t, nl)
            hh = t["h"]
            call("gnf_monotonic_inv", P(_mono_pack(net)), ctypes.byref(net), P(t["z"]), P(hh), hh.stride(0), hh.stride(1),
                 hh.stride(2), P(w), P(tt), MONO_S, P(t["x"]), B, d, stream())
            return {"x": t["x"]}

        def judge_inv(o, tag):                            # test_monotonic_inverse_vs_oracle_and_round_trip
            assert (o["x"].cpu().double() - x0).abs().max() <= 40. / 2 ** 20 + 1e-6, tag
        operands = dict(pdev, z=zt.to(DEV), h=hd, x=torch.empty(B, d, device=DEV))
        base = sweep(operands, inv, judge_inv, names=["z", "h", "x"])
        sweep(operands, inv, judge_inv, names=pnames, offsets=(1, 2))

        # scattered: element (b, j) -> out[j, cols[b]] of a caller-owned [d, width] array
        width = B + 5
        cols = torch.randperm(width, generator=torch.Generator().manual_seed(B))[:B].to(torch.int32).to(DEV)
        want = torch.full((d, width), 3.25, device=DEV)
        want[:, cols.long()] = base["x"].t()

        def scatter(t):
            ps_t = [t[n] for n in pnames]
            ops.monotonic_inverse(t["z"], t["h"], MONO_S, ps_t, out=t["out"], out_cols=cols)
            return {"out": t["out"]}
        operands = dict(pdev, z=zt.to(DEV), h=hd, out=torch.full((d, width), 3.25, device=DEV))
        sweep(operands, scatter, lambda o, tag: bits_equal(o["out"], want) or pytest.fail("scatter " + tag), names=["z", "h", "out"])


@pytest.mark.parametrize("f32", [False, True], ids=["split", "f32"])
@pytest.mark.parametrize("B,d", MONO_SIZES)
@pytest.mark.parametrize("net_kind", ["narrow", "wide"])
def test_monotonic_backward(net_kind, B, d, f32):
    """every gradient against the fp64 oracle at the bounds of tests/fuzz_mono.py; x, h, gz, gjac, gx, gh at every offset, the
    parameters and their gradient arrays at offsets 1 and 2"""
    from gnf_hip import ops
    lib = _abi().load()
    hidden = MONO_NETS[net_kind]
    ps, x, h, layers = _mono_setup(hidden, B, d)
    nl = len(layers)
    g = torch.Generator().manual_seed(B + d)
    gz, gj = torch.randn(B, d, generator=g), torch.randn(B, d, generator=g)
    xr, hr = x.double().requires_grad_(True), h.double().requires_grad_(True)
    lr = [(W.double().requires_grad_(True), b.double().requires_grad_(True)) for W, b in layers]
    z0, j0 = O.monotonic_forward(xr, hr, lr, MONO_S)
    ref = torch.autograd.grad((z0 * gz.double()).sum() + (j0 * gj.double()).sum(), [xr, hr] + [p for Wb in lr for p in Wb])
    bound = float((gz.abs() * x.abs() + gj.abs()).sum())      # the output bias: one sum of signed terms (tests/fuzz_mono.py)
    w, tt = ops.cc_rule(MONO_S, DEV)
    pnames = ["%s%d" % (s, l) for l in range(nl) for s in "Wb"]
    gnames = ["g" + n for n in pnames]
    entry = "gnf_monotonic_bwd_f32" if f32 else "gnf_monotonic_bwd"
    kernels = set()
    operands = dict(zip(pnames, [p.to(DEV) for p in ps]))
    operands.update({"g" + n: torch.empty_like(operands[n]) for n in pnames})
    operands.update(x=x.to(DEV), h=h.to(DEV), gz=gz.to(DEV), gjac=gj.to(DEV), gx=torch.empty(B, d, device=DEV),
                    gh=torch.empty(B, d, MONO_C, device=DEV))

    def bwd(t):
        net = _mono_net(t, nl)
        pack = _mono_pack(net)
        gW = (ctypes.c_void_p * nl)(*[t["gW%d" % l].data_ptr() for l in range(nl)])
        gb = (ctypes.c_void_p * nl)(*[t["gb%d" % l].data_ptr() for l in range(nl)])
        nbytes = lib.gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), MONO_S, B, d)
        ws = torch.empty(max(nbytes // 4, 1), device=DEV)
        hh, gh = t["h"], t["gh"]
        call(entry, P(pack), ctypes.byref(net), P(t["x"]), P(hh), hh.stride(0), hh.stride(1), hh.stride(2), P(w), P(tt), MONO_S,
             P(t["gz"]), P(t["gjac"]), P(t["gx"]), P(gh), gh.stride(0), gh.stride(1), gh.stride(2), gW, gb,
             ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4, B, d, stream())
        kernels.add(lib.gnf_monotonic_bwd_kernel().decode())
        return {k: t[k] for k in ["gx", "gh"] + gnames}

    def judge(o, tag):
        for k, r in zip(["gx", "gh"] + gnames, ref):
            e = rel_err(o[k].cpu(), r)
            if k == gnames[-1]:
                e = min(e, float((o[k].cpu().double() - r).abs().max()) / max(bound, 1e-30) * 10.)
            assert e < GTOL, "%s %s: %.2e" % (k, tag, e)
    sweep(operands, bwd, judge, names=["x", "h", "gz", "gjac", "gx", "gh"])
    sweep(operands, bwd, judge, names=pnames + gnames, offsets=(1, 2))
    assert len(kernels) == 1, kernels
    print("ALIGN mono bwd %s B %d d %d %s: %s" % (net_kind, B, d, entry, kernels))


def test_monotonic_weight_image_must_be_16_byte_aligned():
    """the kernels read the packed weight image in 16-byte pieces, some of them straight into LDS: the one array besides the
    saved conv1 activations that has to be 16-byte aligned.  The entry points refuse another address before any launch."""
    from gnf_hip import ops
    lib = _abi().load()
    ps = [p.to(DEV) for p in _mono_setup([50, 50, 50], 7, 1)[0]]
    net = ops._mono_net(ps)
    nfl = int(lib.gnf_monotonic_pack_floats(ctypes.byref(net)))
    x, h = torch.randn(7, 1, device=DEV), torch.randn(7, 1, MONO_C, device=DEV)
    z, jac = torch.empty_like(x), torch.empty_like(x)
    w, tt = ops.cc_rule(MONO_S, DEV)
    good = ops._mono_pack(net, x)
    for k in (1, 2, 3):
        bad = place(torch.zeros(nfl, device=DEV), k)
        bad.copy_(good)
        assert lib.gnf_monotonic_pack(ctypes.byref(net), P(bad), None) == -1
        args = (ctypes.byref(net), P(x), P(h), h.stride(0), h.stride(1), h.stride(2), P(w), P(tt), MONO_S)
        assert lib.gnf_monotonic_fwd(P(bad), *args, P(z), P(jac), 7, 1, None) == -1
        assert lib.gnf_monotonic_fwd_f32(P(bad), *args, P(z), P(jac), 7, 1, None) == -1
        assert lib.gnf_monotonic_inv(P(bad), *args, P(z), 7, 1, None) == -1
        gp = [torch.empty_like(p) for p in ps]
        gW = (ctypes.c_void_p * net.nl)(*[gp[2 * l].data_ptr() for l in range(net.nl)])
        gb = (ctypes.c_void_p * net.nl)(*[gp[2 * l + 1].data_ptr() for l in range(net.nl)])
        ws = torch.empty(max(lib.gnf_monotonic_bwd_ws_bytes(ctypes.byref(net), MONO_S, 7, 1) // 4, 1), device=DEV)
        gh = torch.empty_like(h)
        for pk, wsp in ((bad, ws.data_ptr()), (good, ws.data_ptr() + 4 * k)):
            assert lib.gnf_monotonic_bwd(P(pk), *args, P(z), P(jac), P(x.clone()), P(gh), gh.stride(0), gh.stride(1), gh.stride(2),
                                         gW, gb, ctypes.c_void_p(wsp), ws.numel() * 4 - 16, 7, 1, None) == -1
        assert guards_intact(bad)


# ================================================================================================== DAG gate
def _gate_inputs(d, B, imp, gate, seed):
    g = torch.Generator().manual_seed(seed)
    s_thresh = imp in ("soft", "hard_soft")
    h_thresh = .3 if imp.startswith("hard") else 0.
    while True:        # (a hard threshold is a step function of A: no entry within rounding of it, tests/fuzz_gate.py)
        A = (torch.rand(d, d, generator=g) * 1.2 + .2) * (torch.rand(d, d, generator=g) < .7).float()
        if imp == "hard_sq" and gate == "gumbel":
            A = A.clamp(-.95, .95)
        impv = O.dag_soft_thresholded_A(A) if s_thresh else A ** 2
        if not imp.startswith("hard") or not bool(((impv - h_thresh).abs() < 1e-4).any()):
            break
    x = torch.randn(B, d, generator=g)
    u1 = u2 = None
    if gate == "gumbel":
        u1 = torch.rand(B, d, d, generator=g).clamp(.02, .98)            # (ln u is O(1): no digits lost next to u = 1)
        u2 = torch.rand(B, d, d, generator=g).clamp(.02, .98)
    if gate == "noise":
        u1 = torch.randn(B, d, d, generator=g)
    return A, x, u1, u2, s_thresh, h_thresh


GATE_FORMS = [("raw", "det")] + [(i, g) for i in ("soft", "hard_soft", "hard_sq") for g in ("det", "gumbel", "noise")]


@pytest.mark.parametrize("d", [8, 12, 7])
def test_dag_gate_every_form(d, monkeypatch):
    """d = 8, 12: the kernels read x, the cotangent and their table as 16-byte quads when base and row pitch allow (quad_aligned)
    and element by element for a displaced base; d = 7: always element by element.  The arithmetic behind the loads is shared:
    the same bits at every offset.  Reference: the oracle in fp64, bounds of tests/fuzz_gate.py."""
    from gnf_hip import ops
    spy = PtrSpy(monkeypatch)
    B = 5
    for n, (imp, gate) in enumerate(GATE_FORMS):
        hot, T = bool(n & 1), (.5 if n % 3 == 0 else 1.)
        A, x, u1, u2, s_thresh, h_thresh = _gate_inputs(d, B, imp, gate, 100 * d + n)
        d6 = lambda t: t.double() if t is not None else None            # noqa: E731
        xr, Ar = x.double().requires_grad_(True), A.double().requires_grad_(True)
        if imp == "raw":
            e0 = O.dag_masked_inputs(xr, Ar, False, 0., False, False, 1., None, None, None, hot)
        else:
            e0 = O.dag_masked_inputs(xr, Ar, s_thresh, h_thresh, gate == "gumbel", gate == "noise", T,
                                     d6(u1) if gate == "gumbel" else None, d6(u2), d6(u1) if gate == "noise" else None, hot)
        ge = torch.randn(e0.shape, generator=torch.Generator().manual_seed(n))
        gx0, gA0 = torch.autograd.grad((e0 * ge.double()).sum(), (xr, Ar))
        e0 = e0.detach().reshape(B * d, -1)
        im = {"raw": ops.IMP_RAW, "soft": ops.IMP_SOFT, "hard_soft": ops.IMP_HARD_SOFT, "hard_sq": ops.IMP_HARD_SQ}[imp]
        gm = {"det": ops.GATE_DET, "gumbel": ops.GATE_GUMBEL, "noise": ops.GATE_NOISE}[gate]
        dev = lambda t: None if t is None else t.to(DEV)                # noqa: E731

        def run(t):
            xg, Ag = t["x"].requires_grad_(True), t["A"].requires_grad_(True)
            e = ops.DagGateFn.apply(xg, Ag, im, gm, h_thresh, T, hot, t["u1"], t["u2"], 0, 0)
            gx, gA = torch.autograd.grad(e, (xg, Ag), grad_outputs=t["ge"])
            return {"e": e.detach(), "gx": gx, "gA": gA}

        def judge(o, tag):
            what = "d %d %s/%s hot %d %s: " % (d, imp, gate, hot, tag)
            assert rel_err(o["e"].cpu(), e0) < 1e-5, what + "e %.2e" % rel_err(o["e"].cpu(), e0)
            assert rel_err(o["gx"].cpu(), gx0) < 1e-4, what + "gx %.2e" % rel_err(o["gx"].cpu(), gx0)
            if float(gA0.abs().max()) > 0:
                assert rel_err(o["gA"].cpu(), gA0) < 1e-4, what + "gA %.2e" % rel_err(o["gA"].cpu(), gA0)
            else:
                assert float(o["gA"].abs().max()) == 0., what + "gA"
        sweep({"x": dev(x), "A": dev(A), "u1": dev(u1), "u2": dev(u2), "ge": dev(ge.reshape(B * d, -1))}, run, judge, spy=spy)


# ================================================================================================== DAG loss
@pytest.mark.parametrize("d,l1", [(7, 0.), (84, .3)])
def test_dag_loss_forward_backward(d, l1, monkeypatch):
    """the acyclicity + l1 term (three launches around the library's matrix power), A displaced.  Reference and bounds of
    test_dag_loss_fused_vs_reference_expression: the reference's expression (DAGConditioner.py:176-194, 268-271) in plain torch
    ops on the same module -- both sides raise the same fp32 matrix to its power on the library"""
    from gnf_hip import ops
    from models import DAGConditioner
    spy = PtrSpy(monkeypatch)
    torch.manual_seed(d)
    cond = DAGConditioner(d, [8], 2, l1=l1).to(DEV)
    with torch.no_grad():
        cond.A.mul_(.2)
        cond.lambd.fill_(.7)
        cond.c.fill_(.05)
    lag = cond.get_power_trace()
    ref = cond.dag_const * (cond.lambd * lag + cond.c / 2 * lag ** 2) + cond.l1_weight * cond.A.abs().mean()
    gA0, = torch.autograd.grad(ref, cond.A)
    loss0, gA0 = ref.detach().cpu(), gA0.cpu()

    def run(t):
        Ag = t["A"].requires_grad_(True)
        loss = ops.DagLossFn.apply(Ag, cond.alpha, cond.alpha_factor, cond.lambd, cond.c, cond.dag_const, cond.l1_weight,
                                   cond.exponent)
        gA, = torch.autograd.grad(loss, Ag)
        return {"loss": loss.detach().reshape(1), "gA": gA}

    def judge(o, tag):
        assert rel_err(o["loss"].cpu(), loss0.reshape(1)) < TOL, (tag, o["loss"].item(), loss0.item())
        assert rel_err(o["gA"].cpu(), gA0) < GTOL, (tag, rel_err(o["gA"].cpu(), gA0))
    sweep({"A": cond.A.detach().clone()}, run, judge, spy=spy)


# ================================================================================================== conv front
@pytest.mark.parametrize("path", ["recompute", "saved_a1", "exact_ties"])
def test_mnist_conv_front(path, monkeypatch):
    """n = 5 images (one partial tile of the pipelined kernels); the backward that recomputes conv1, the one that loads the
    conv1 activations the Winograd forward saved (the saved buffer is the library's own allocation and stays 16-byte aligned:
    its refusal is tests/test_gpu_conv_saved_a1.py's), and the tie-exact direct forward.  Reference and bounds:
    test_mnist_conv_front_vs_torch_cpu (knife-edge images redrawn)."""
    import torch.nn.functional as F
    import knife_units
    from conftest import conv_front_knife_images
    from gnf_hip import ops
    spy = PtrSpy(monkeypatch)
    n = 5
    (e, W1, b1, W2, b2), redraw = knife_units.draw_conv_front(n, "dense")
    (e,), _ = knife_units.resample_off_ties(redraw, lambda e_: conv_front_knife_images(e_, W1, b1, W2, b2)[0], first=(e,))
    ps = [t.double().requires_grad_(True) for t in (e, W1, b1, W2, b2)]
    ref = torch.flatten(F.max_pool2d(F.conv2d(torch.relu(F.conv2d(ps[0].view(-1, 1, 28, 28), ps[1], ps[2])), ps[3], ps[4]), 2), 1)
    gp = torch.randn(n, 2304, generator=torch.Generator().manual_seed(n))
    gref = torch.autograd.grad((ref * gp.double()).sum(), ps)
    ref = ref.detach()
    names = ["e", "W1", "b1", "W2", "b2"]

    def run(t):
        leaves = [t[k].requires_grad_(True) for k in names]
        if path == "saved_a1":
            out = ops.mnist_conv(*leaves)                          # grad mode on: the forward keeps conv1's activations
        else:
            out = ops.MnistConvFn.apply(*leaves, path == "exact_ties")     # no grad_mode: nothing kept, conv1 recomputed
        grads = torch.autograd.grad(out, leaves, grad_outputs=t["gp"])
        return dict(zip(["g" + k for k in names], grads), out=out.detach())

    def judge(o, tag):
        assert rel_err(o["out"].cpu(), ref) < TOL, tag
        assert_close(o["out"], ref, rtol=1e-5, atol=1e-6 * ref.abs().max().item(), what="pooled " + tag)
        per_img = (o["ge"].cpu().double() - gref[0]).abs().amax(1) / gref[0].abs().amax(1).clamp_min(1e-30)
        assert float(per_img.max()) < GTOL, (tag, per_img.max().item())
        for k, r in zip(names[1:], gref[1:]):
            assert rel_err(o["g" + k].cpu(), r) < GTOL, (tag, k)
            assert_close(o["g" + k], r, rtol=1e-4, atol=2e-6 * r.abs().max().item(), what="d%s %s" % (k, tag))
    sweep(dict(zip(names, [t.to(DEV) for t in (e, W1, b1, W2, b2)]), gp=gp.to(DEV)), run, judge, spy=spy)


# ================================================================================================== sparse front
def _window_gate(gen, density):
    """an importance matrix that is zero outside the 5 x 5 pixel windows (tests/fuzz_sparse.py)"""
    r, c = torch.arange(28).repeat_interleave(28), torch.arange(28).repeat(28)
    win = ((r[:, None] - r[None, :]).abs() <= 2) & ((c[:, None] - c[None, :]).abs() <= 2)
    return (win & (torch.rand(784, 784, generator=gen) < density)).float() * (torch.rand(784, 784, generator=gen) + .2)


SPARSE_ROWS = [783, 0, 27, 28, 400, 401, 13 * 28 + 13, 6 * 28 + 7, 21 * 28 + 20, 755]
SPARSE_NAMES = ["x", "P", "W1", "b1", "W2", "b2", "Wfc1", "bfc1", "Wfc2", "bfc2"]


def _sparse_setup(B):
    from gnf_hip import ops
    from models.MLP import MNISTCNN
    gen = torch.Generator().manual_seed(B)
    torch.manual_seed(B)
    net = MNISTCNN(out_d=30)
    with torch.no_grad():
        for p in net.parameters():                     # biases of both signs: background relu(b) partly 0, partly > 0
            if p.dim() == 1:
                p.copy_(torch.randn_like(p) * .3)
    ps = {k: v.detach().clone() for k, v in net.state_dict().items()}
    P, x = _window_gate(gen, .5), torch.randn(B, 784, generator=gen)
    sr = ops.SparseRows(SPARSE_ROWS, B, torch.device(DEV))
    pix = sr.pix.cpu().long()
    e = (x.unsqueeze(0) * P[pix].unsqueeze(1)).reshape(len(SPARSE_ROWS) * B, 784)      # row = sorted position * B + sample
    vals = [x, P] + [ps[k] for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias",
                                     "fc2.weight", "fc2.bias")]
    return sr, e, ps, dict(zip(SPARSE_NAMES, vals))


@pytest.mark.parametrize("mode", ["plain", "prepared", "fc12"])
def test_sparse_front_inference(mode, monkeypatch):
    """the sparse masked-image front without a backward: tables built per call, held tables, and held tables with the one-launch
    fc1 + ReLU + fc2 kernel; against the oracle's dense MNISTCNN on the explicit masked copies at the bound of
    tests/fuzz_sparse.py"""
    from gnf_hip import ops
    spy = PtrSpy(monkeypatch)
    B = 3
    sr, e, ps, vals = _sparse_setup(B)
    want = O.mnistcnn_forward(e.double(), {k: v.double() for k, v in ps.items()})

    def run(t):
        with torch.no_grad():
            prep = None if mode == "plain" else ops.mnistcnn_sparse_prepare(t["b1"], t["W2"], t["b2"], t["Wfc1"], t["bfc1"])
            if mode == "fc12":
                assert ops.sparse_fc12_fits(t["Wfc1"], t["Wfc2"])
                out = ops.mnistcnn_sparse_fwd_fc2(t["x"], t["P"], sr, t["W1"], t["b1"], t["W2"], t["b2"], prep, t["Wfc2"], t["bfc2"])
            else:
                h1 = ops.mnistcnn_sparse_fwd(t["x"], t["P"], sr, t["W1"], t["b1"], t["W2"], t["b2"], t["Wfc1"], t["bfc1"],
                                             pre_gated=True, prep=prep)
                out = ops.mlp(h1, [(t["Wfc2"], t["bfc2"])], relu_in=True)
        return {"out": out}

    def judge(o, tag):
        excess = (o["out"].cpu().double() - want).abs() - (1e-6 + 1e-5 * want.abs())
        assert float(excess.max()) <= 0., (tag, float(excess.max()))
    sweep({k: v.to(DEV) for k, v in vals.items()}, run, judge, offsets=(1, 2), spy=spy)


@pytest.mark.parametrize("reuse_tables", [True, False], ids=["bwd_tables", "bwd"])
def test_sparse_front_training(reuse_tables, monkeypatch):
    """forward and parameter gradients of the training path (argmax record, grouped fc1 GEMMs -- the displaced cotangent is their
    A / B operand --, crop backward); copies with a decision on a knife edge in fp64 (conv1 ReLU, pool window, fc1 ReLU) get a
    zero cotangent, as in test_sparse_front_parameter_gradients: they cannot be redrawn, all copies come from one x"""
    from conftest import conv_front_knife_images, EPS32
    from gnf_hip import ops
    spy = PtrSpy(monkeypatch)
    monkeypatch.setattr(ops, "SPARSE_REUSE_TABLES", reuse_tables)     # the backward reads the forward's tables / builds its own
    B = 3
    sr, e, ps, vals = _sparse_setup(B)
    p64 = {k: v.double().requires_grad_(True) for k, v in ps.items()}
    want = O.mnistcnn_forward(e.double(), p64)
    gh = torch.randn(want.shape, generator=torch.Generator().manual_seed(1))
    knife = conv_front_knife_images(e, ps["conv1.weight"], ps["conv1.bias"], ps["conv2.weight"], ps["conv2.bias"])[0]
    with torch.no_grad():
        import torch.nn.functional as F
        pooled = F.max_pool2d(F.conv2d(torch.relu(F.conv2d(e.double().view(-1, 1, 28, 28), p64["conv1.weight"], p64["conv1.bias"])),
                                       p64["conv2.weight"], p64["conv2.bias"]), 2).flatten(1)
        pre = pooled @ p64["fc1.weight"].t() + p64["fc1.bias"]
        mag = pooled.abs() @ p64["fc1.weight"].abs().t() + p64["fc1.bias"].abs()
        knife = knife | ((pre.abs() < 64 * EPS32 * mag) & (pre != 0)).any(1)
    assert int(knife.sum()) <= 3
    gh[knife] = 0.
    keys = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
    gref = torch.autograd.grad((want * gh.double()).sum(), [p64[k] for k in keys])
    want = want.detach()
    pn = SPARSE_NAMES[2:]

    def run(t):
        leaves = [t[k].requires_grad_(True) for k in pn]
        h1 = ops.mnistcnn_sparse_fwd(t["x"], t["P"], sr, *leaves[:6], pre_gated=True)
        out = ops.mlp(h1, [(leaves[6], leaves[7])], relu_in=True)
        grads = torch.autograd.grad(out, leaves, grad_outputs=t["gh"])
        return dict(zip(["g" + k for k in pn], grads), out=out.detach())

    def judge(o, tag):
        excess = (o["out"].cpu().double() - want).abs() - (1e-6 + 1e-5 * want.abs())
        assert float(excess.max()) <= 0., (tag, float(excess.max()))
        for k, r in zip(pn, gref):
            assert rel_err(o["g" + k].cpu(), r) < GTOL, (tag, k, rel_err(o["g" + k].cpu(), r))
    sweep(dict({k: v.to(DEV) for k, v in vals.items()}, gh=gh.to(DEV)), run, judge, offsets=(1, 2), spy=spy)


# ================================================================================================== MADE prefix evaluation
@pytest.mark.parametrize("d,hidden", [(17, [40, 33, 19]), (3, [40, 33])], ids=["dot", "mfma"])
def test_made_prefix(d, hidden):
    """the column-by-column inversion kernel on its lane-group branch and its MFMA branch (the shapes of
    test_whole_inversion_in_one_launch_equals_single_steps): z, x, h_out and the parameters handed to made_prefix_pack displaced.
    Bound: the column schedule's error against the fp64 inversion is at most twice the fixed-point passes' + 1e-6 max|x|
    (tests/test_gpu_made_invert.py)."""
    from gnf_hip import ops
    from test_gpu_made_invert import _affine_flow, _fp64_invert
    flow = _affine_flow(d, hidden, seed=3)
    step = flow.steps[0]
    cond = step.conditioner
    plan, params = cond.prefix_plan(), [p.detach() for p in cond._prefix_params()]
    assert plan is not None
    B = 70
    z = (.7 * torch.randn(B, d, generator=torch.Generator().manual_seed(d))).to(DEV)
    x64 = _fp64_invert(step, z)
    step.column_schedule = False
    e_pass = (step.invert(z).cpu().double() - x64).abs().max().item()
    step.column_schedule = True
    bound = 2. * e_pass + 1e-6 * x64.abs().max().item()
    net = cond.masked_autoregressive_net
    layers = [(l.weight.detach().cpu().double(), l.bias.detach().cpu().double()) for l in net.masked_layers()]
    masks = [l.mask.detach().cpu().double() for l in net.masked_layers()]
    var = plan["var_host"]
    pnames = ["p%d" % i for i in range(len(params))]
    operands = dict(zip(pnames, params), z=z, x=torch.zeros(B, d, device=DEV), h_out=torch.empty(B, plan["out"], device=DEV))

    def run(t):
        ps = [t[n] for n in pnames]
        pack = ops.made_prefix_pack(ps, plan)
        ops.made_prefix_steps(ps, plan, pack, t["z"], t["x"], 0, d, ops.MADE_NORM_AFFINE)
        # the conditioner outputs alone (MADE_NORM_NONE), variable by variable over the x just found
        ws = ops.made_prefix_workspace(ps, plan, B)
        hs = []
        for s in range(d):
            ops.made_prefix_steps(ps, plan, pack, None, t["x"], s, s + 1, ops.MADE_NORM_NONE, h_out=t["h_out"], ws=ws)
            hs.append(t["h_out"].clone())
        return {"x": t["x"], "h": torch.stack(hs, 2)}                  # [B, out, step]

    def judge(o, tag):
        assert (o["x"].cpu().double() - x64).abs().max().item() <= bound, (tag, bound)
        # the conditioner outputs at the kernel's own x ([B, d, out] -> the variables in step order): one masked-MLP forward,
        # the bound of tests/fuzz_linear.py on y
        want = O.made_forward(o["x"].cpu().double(), layers, masks)[:, var, :].permute(0, 2, 1)
        assert rel_err(o["h"].cpu(), want) < 2e-5, (tag, rel_err(o["h"].cpu(), want))
    sweep(operands, run, judge, names=["z", "x", "h_out"])
    sweep(operands, run, judge, names=pnames, offsets=(1, 2))
    bad = place(torch.zeros(8, device=DEV), 1)
    net_c = ops._made_net(params, plan)
    assert _abi().load().gnf_made_prefix(ctypes.byref(net_c), P(bad), P(z), P(operands["x"]), None, 0, d, ops.MADE_NORM_AFFINE, B,
                                         None, 0, None) == -1            # the weight image must be 16-byte aligned: refused


# ================================================================================================== gradient slots
class _Slots:
    """the interface ops.register_grad_slots asks of a flat training state"""

    def __init__(self, params, k):
        self.grad_views = [place(torch.zeros(p.numel(), device=DEV), k) for p in params]
        self._taken = set()


@pytest.mark.parametrize("k", [1, 2, 3])
def test_gradients_written_into_displaced_slots(k):
    """backward kernels write parameter gradients straight into the slots a flat training state registers
    (ops.register_grad_slots); dp.FlatState pads its slots to 16 bytes, another owner need not.  Slots at every offset: the
    linear layers (small-batch and tall), the Monotonic normalizer, the DAG gate (d = 8: its dA kernel stores quads when it
    may) and the DAG loss write the bits they write into fresh tensors, and nothing next to them."""
    from gnf_hip import ops
    from models import MonotonicNormalizer
    g = torch.Generator().manual_seed(k)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)               # noqa: E731
    cases = []
    for M in (100, 2049):
        W, b, x, gy = rnd(30, 64) / 8., rnd(30), rnd(M, 64), rnd(M, 30)
        cases.append(("linear M=%d" % M, [W, b], lambda ps, x=x, gy=gy: (ops.mlp(x, [(ps[0], ps[1])]) * gy).sum()))
    torch.manual_seed(k)
    mono = [p.detach().to(DEV) for p in MonotonicNormalizer([50, 50, 50], MONO_C, nb_steps=MONO_S).integrand_net.flat_params()]
    xm, hm = rnd(9, 7), rnd(9, 7, MONO_C)
    cases.append(("monotonic", mono, lambda ps: sum(t.sum() for t in ops.MonotonicFn.apply(xm, hm, MONO_S, *ps))))
    A, xg, ge = (torch.rand(8, 8, generator=g) + .2).to(DEV), rnd(5, 8), rnd(40, 8)
    cases.append(("dag gate", [A], lambda ps: (ops.DagGateFn.apply(xg, ps[0], ops.IMP_SOFT, ops.GATE_DET, 0., 1., False, None, None,
                                                                    0, 0) * ge).sum()))
    cases.append(("dag loss", [A * .2], lambda ps: ops.DagLossFn.apply(ps[0], .7, 1., .7, .05, 1., .3, 8)))
    for name, params, loss in cases:
        fresh = [p.clone().requires_grad_(True) for p in params]
        want = torch.autograd.grad(loss(fresh), fresh)
        slotted = [p.clone().requires_grad_(True) for p in params]
        owner = _Slots(slotted, k)
        ops.register_grad_slots(owner, slotted)
        try:
            got = torch.autograd.grad(loss(slotted), slotted)
        finally:
            ops.unregister_grad_slots(owner)
        torch.cuda.synchronize()
        assert owner._taken == set(range(len(params))), (name, owner._taken)
        for i, (a, b_, v) in enumerate(zip(got, want, owner.grad_views)):
            assert bits_equal(v.view_as(b_), b_), "%s: slot %d does not hold the gradient at offset %d" % (name, i, k)
            assert bits_equal(a, b_), "%s: gradient %d differs at offset %d" % (name, i, k)
            assert guards_intact(v), "%s: guard of slot %d overwritten at offset %d" % (name, i, k)


def test_probe_copy_refuses_unaligned_arrays():
    """the measurement probe is a float4 stream copy by definition: listed among the exceptions of include/gnf_hip.h"""
    lib = _abi().load()
    src, dst = torch.arange(64., device=DEV), torch.zeros(64, device=DEV)
    assert lib.gnf_probe_copy(P(dst), P(src), 64, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst, src)
    for k in (1, 2, 3):
        bad = place(src, k)
        assert lib.gnf_probe_copy(P(dst), P(bad), 64, None) == -1 and lib.gnf_probe_copy(P(bad), P(src), 64, None) == -1
        torch.cuda.synchronize()
        assert guards_intact(bad) and torch.equal(bad, src)


# ================================================================================================== fused gate + conv front
@pytest.mark.parametrize("gate", ["det", "gumbel"])
@pytest.mark.parametrize("want_x", [False, True], ids=["plan", "dense"])
def test_dag_conv_front(want_x, gate, monkeypatch):
    """the DAG gate and the conv front as one autograd node (B = 1: 784 masked copies).  Without a gradient for x the backward
    runs on the forward's column plan (gnf_dag_gate_fwd_plan, gnf_mnistcnn_conv_bwd_cols[_a1], gnf_dag_gate_bwd_cols), with one
    on the dense entry points.
    det: the deterministic gate -- copies exactly zero outside their windows, exact pool ties, the tie-exact forward and the
    backward that recomputes conv1; value and every gradient against fp64, the copies that hold a knife-edge decision in fp64
    with a zero cotangent (functions of one x: they cannot be redrawn).
    gumbel: injected noise, the Winograd forward that saves conv1's activations and the backward that loads them.  Outside
    its <= 32 live pixels a copy is a near-constant image of ~1e-6-sized values: EVERY copy holds pool windows tied within
    roundoff in fp64 (784 of 784 by conftest.conv_front_knife_images), so no fp64 gradient is a reference here; the pooled
    values are judged against fp64, the gradients bit for bit against the aligned call."""
    import torch.nn.functional as F
    from conftest import conv_front_knife_images
    from gnf_hip import ops
    spy = PtrSpy(monkeypatch)
    gen = torch.Generator().manual_seed(4)
    A, x = _window_gate(gen, .5), torch.randn(1, 784, generator=gen)
    u1 = u2 = None
    if gate == "gumbel":
        u1 = torch.rand(1, 784, 784, generator=gen).clamp(.02, .98)
        u2 = torch.rand(1, 784, 784, generator=gen).clamp(.02, .98)
    W1, b1 = torch.randn(16, 1, 3, 3, generator=gen) * .3, torch.randn(16, generator=gen) * .1
    W2, b2 = torch.randn(16, 16, 3, 3, generator=gen) * .1, torch.randn(16, generator=gen) * .1
    names = ["x", "A", "W1", "b1", "W2", "b2"]
    leaves64 = [t.double().requires_grad_(True) for t in (x, A, W1, b1, W2, b2)]
    d6 = lambda t: None if t is None else t.double()                   # noqa: E731
    e0 = O.dag_masked_inputs(leaves64[0], leaves64[1], True, 0., gate == "gumbel", False, 1., d6(u1), d6(u2), None, False)
    e0 = e0.reshape(784, 784)
    ref = torch.flatten(F.max_pool2d(F.conv2d(torch.relu(F.conv2d(e0.view(-1, 1, 28, 28), leaves64[2], leaves64[3])),
                                              leaves64[4], leaves64[5]), 2), 1)
    gp = torch.randn(784, 2304, generator=gen)
    live = [n for n in names if want_x or n != "x"]
    gref = None
    if gate == "det":
        knife = conv_front_knife_images(e0.detach().float(), W1, b1, W2, b2)[0]
        assert int(knife.sum()) <= 784 // 16
        gp[knife] = 0.
        gref = torch.autograd.grad((ref * gp.double()).sum(), [leaves64[names.index(n)] for n in live])
    ref = ref.detach()
    gm = ops.GATE_GUMBEL if gate == "gumbel" else ops.GATE_DET

    def run(t):
        leaves = [t[n].requires_grad_(True) for n in live]
        out = ops.dag_conv_front(t["x"], t["A"], ops.IMP_SOFT, gm, 0., 1., t["u1"], t["u2"], 0, 0, t["W1"], t["b1"], t["W2"], t["b2"],
                                 exact_ties=gate == "det")
        grads = torch.autograd.grad(out, leaves, grad_outputs=t["gp"])
        return dict(zip(["g" + n for n in live], grads), out=out.detach())

    def judge(o, tag):
        assert rel_err(o["out"].cpu(), ref) < TOL, (tag, rel_err(o["out"].cpu(), ref))
        for n, r in zip(live, gref or ()):
            assert rel_err(o["g" + n].cpu(), r) < GTOL, (tag, n, rel_err(o["g" + n].cpu(), r))
    dev = lambda t: None if t is None else t.to(DEV)                    # noqa: E731
    operands = dict(zip(names, [t.to(DEV) for t in (x, A, W1, b1, W2, b2)]), u1=dev(u1), u2=dev(u2), gp=gp.to(DEV))
    sweep(operands, run, judge, offsets=(1, 2), spy=spy)
