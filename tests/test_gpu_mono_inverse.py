"""The Monotonic inverse (gnf_monotonic_inv / _inv_scatter) against fp64 on every route inv_route dispatches: one case per
row of tests/mono_inverse_cases.py, whose claimed route tests/test_mono_inverse_routes_host.py pins without a GPU.  Each
case asserts that the kernel that RAN (gnf_monotonic_inv_kernel) is the one the query names, so a moved threshold cannot
quietly turn a row into a second test of another kernel.

Setup: seeded MonotonicNormalizer(hidden, cond_size, nb_steps=S, solver="CC") as initialised, x = 1.5 randn(B, d),
h = randn(B, d, c), targets zt = float32(z64(x)) with z64 the oracle's forward in fp64; the first two and the last two targets
(the last two sit in the ragged tail group) are overwritten with +-1e4.  h is passed contiguous and in the MADE permutation
([B, c, d] storage).

Checks, every element, none left out:
  * bracket (mimics no bisection): with W = 40 / 2^20, the interval after 20 halvings of [-20, 20], the answer xi is the
    midpoint of the kernel's last interval, and its own fp32 z lies on either side of zt at the two ends, so
        z64(xi - W/2) - tol <= zt <= z64(xi + W/2) + tol,   tol = 4 e_ref + 4e-6,  e_ref = max |z32_oracle(x) - z64(x)|
    (the forward rule of tests/test_gpu_eval_path.py; e_ref is measured per case on the CPU, against the reference, never
    against the kernel);
  * the standing bound |xi - x64| <= W + 1e-6 against the oracle's bisection in fp64
    (test_monotonic_inverse_vs_oracle_and_round_trip);
  * saturated targets give +-float32(20 - 40 / 2^21) bit for bit (every step of the arithmetic is exact there);
  * 64 sentinel floats behind element n - 1 of the output are intact;
  * out= / out_cols= (the scattered form) is bit-equal to the plain result and leaves the other columns alone.

Measured on an MI355X, all 39 rows in both layouts of h (the two layouts gave identical bits on every row): e_ref
2.1e-7 .. 1.9e-6, tol 4.8e-6 .. 1.2e-5.  Worst bracket excess as a share of tol, the largest two:
    0.068   [50, 50, 50] c 30, S 8, n 8195     mono_fwd_x_k<HM=3,EX=2,WM=1,INV=1>
    0.062   [50, 50, 50] c 30, S 8, n 32802    mono_fwd_x_k<HM=3,EX=2,WM=1,INV=1>
(then 0.047 for [20, 20] S 8 n 32802 on mono_fwd_k<HT=2,WM=1,INV=1> and 0.046 for [20, 20] S 20 n 4083 on
mono_inv_split_k<HT=2,WM=1,EPG=16>; 0 on most of the small rows).  Worst |xi - x64| / W: exactly 1 (one last-step interval:
a decision that fp32 and fp64 take differently) on 18 of the 39 rows, 0 on the others -- never between, never above."""
import ctypes

import pytest
import torch

from mono_inverse_cases import ROWS, case_id
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = 40. / 2 ** 20
SAT = float(torch.tensor(20., dtype=torch.float32) - torch.tensor(40. / 2 ** 21, dtype=torch.float32))
SENTINEL = -12345.5


def _reference(hidden, c, S, B, d, seed):
    """everything the CPU computes for a case, once: inputs, targets, e_ref, the fp64 inverse and z64 as a function"""
    from models import MonotonicNormalizer
    torch.manual_seed(seed)
    norm = MonotonicNormalizer(hidden, c, nb_steps=S, solver="CC")
    x = torch.randn(B, d) * 1.5
    h = torch.randn(B, d, c)
    ps = [p.detach().clone() for p in norm.integrand_net.flat_params()]
    layers = [(ps[i], ps[i + 1]) for i in range(0, len(ps), 2)]
    layers64 = [(Wl.double(), b.double()) for Wl, b in layers]
    h64 = h.double()

    def z64(xx):
        with torch.no_grad():
            return O.monotonic_forward(xx, h64, layers64, S)[0]
    with torch.no_grad():
        zx = z64(x.double())
        e_ref = (O.monotonic_forward(x, h, layers, S)[0].double() - zx).abs().max().item()
        zt = zx.float()
        sat = torch.zeros(B * d, dtype=torch.bool)
        flat = zt.view(-1)
        for k, v in ((0, 1e4), (1, -1e4), (B * d - 2, 1e4), (B * d - 1, -1e4)):
            flat[k] = v
            sat[k] = True
        x64 = O.monotonic_inverse(zt.double(), h64, layers64, S)
    return norm, h, zt, sat.view(B, d), x64, e_ref, z64


def _route_line(norm, S, B, d):
    from gnf_hip import abi, ops
    net = ops._mono_net([p.detach().contiguous() for p in norm.integrand_net.flat_params()])
    buf = ctypes.create_string_buffer(256)
    assert abi.load().gnf_monotonic_inv_route(ctypes.byref(net), S, B, d, buf, 256) == 0
    return buf.value


def _inverse_into(norm, z, h, S, x):
    """gnf_monotonic_inv into a buffer of the caller's (ops.monotonic_inverse allocates its own)"""
    from gnf_hip import abi, ops
    params = [p.detach().contiguous() for p in norm.integrand_net.flat_params()]
    net = ops._mono_net(params)
    pack = ops._mono_pack(net, z)
    w, t = ops.cc_rule(S, z.device)
    B, d = z.shape
    abi.call("gnf_monotonic_inv", abi.ptr(pack), ctypes.byref(net), abi.ptr(z), abi.ptr(h), h.stride(0), h.stride(1),
             h.stride(2), abi.ptr(w), abi.ptr(t), int(S), abi.ptr(x), B, d, abi.stream())


@pytest.mark.parametrize("row", ROWS, ids=[case_id(r) for r in ROWS])
def test_inverse_against_fp64_on_its_route(row):
    from gnf_hip import abi, ops
    hidden, c, S, B, d, template, block, grid = row
    n = B * d
    norm, h, zt, sat, x64, e_ref, z64 = _reference(hidden, c, S, B, d, seed=1000 + ROWS.index(row))
    tol = 4 * e_ref + 4e-6
    norm = norm.to(DEV)
    params = norm.integrand_net.flat_params()
    line = _route_line(norm, S, B, d)
    assert line.decode().split(" ")[0] == template and ("block=%d grid=%d " % (block, grid)) in line.decode(), line
    z = zt.to(DEV)
    # (as_strided: permute() rewrites the stride of a size-1 dimension, and c = 1 is a case)
    made = torch.as_strided(h.permute(0, 2, 1).contiguous().to(DEV), (B, d, c), (c * d, 1, d))
    layouts = {"contiguous": h.to(DEV), "made": made}
    assert made.stride() == (c * d, 1, d) and torch.equal(made, layouts["contiguous"])
    lib = abi.load()
    want_sat = torch.where(zt > 0, torch.tensor(SAT), torch.tensor(-SAT))
    results = {}
    for name, hd in layouts.items():
        with torch.no_grad():
            xi = ops.monotonic_inverse(z, hd, S, params)
        assert lib.gnf_monotonic_inv_kernel() == line, (lib.gnf_monotonic_inv_kernel(), line)
        xi = xi.cpu()
        results[name] = xi
        assert torch.isfinite(xi).all()
        # saturated targets: the end of the search interval, bit for bit
        assert torch.equal(xi[sat], want_sat[sat]), (name, xi[sat], want_sat[sat])
        xi64 = xi.double()
        with torch.no_grad():
            lo, hi = z64(xi64 - W / 2), z64(xi64 + W / 2)
        viol = torch.maximum(lo - zt.double(), zt.double() - hi)[~sat]
        share = max(viol.max().item(), 0.) / tol
        dist = ((xi64 - x64).abs()[~sat].max() / W).item()
        print("\n[mono-inverse] %s h=%s %s e_ref=%.3g tol=%.3g bracket_excess/tol=%.3f |xi-x64|/W=%.4f"
              % (case_id(row), name, line.decode(), e_ref, tol, share, dist))
        bad = int((viol > tol).sum())
        assert bad == 0, "%s: %d of %d elements outside the bracket, worst excess %.3g (tol %.3g)" % (
            name, bad, viol.numel(), viol.max().item(), tol)
        assert (xi64 - x64).abs().max().item() <= W + 1e-6, (name, (xi64 - x64).abs().max().item())
    # the result does not depend on how h is laid out (the same values reach the same arithmetic)
    assert torch.equal(results["contiguous"], results["made"])

    # a buffer of the test's own: 64 sentinels behind element n - 1 stay
    buf = torch.full((n + 64,), SENTINEL, device=DEV)
    _inverse_into(norm, z, layouts["made"], S, buf[:n].view(B, d))
    assert lib.gnf_monotonic_inv_kernel() == line
    buf = buf.cpu()
    assert torch.equal(buf[:n].view(B, d), results["contiguous"])
    assert (buf[n:] == SENTINEL).all()

    # the scattered form: element (b, j) -> out[j, cols[b]], nothing else written
    torch.manual_seed(7)
    width = B + 5
    cols = torch.randperm(width)[:B].to(torch.int32).to(DEV)
    want = torch.full((d, width), 7.5)
    want[:, cols.cpu().long()] = results["contiguous"].t()
    got = torch.full((d, width), 7.5, device=DEV)
    with torch.no_grad():
        ops.monotonic_inverse(z, layouts["contiguous"], S, params, out=got, out_cols=cols)
    assert lib.gnf_monotonic_inv_kernel() == line
    assert torch.equal(got.cpu(), want)
