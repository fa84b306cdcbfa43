"""Decision-resolved gradient checks of the knife-edge cases (-m gpu).

The main comparisons (test_gpu_parity.py: test_mnist_conv_front_vs_torch_cpu, test_monotonic_ragged_sizes) redraw the images /
elements that hold a ReLU gate or a pool window within 16 fp32 ulps of a tie.  Here the RAW draws of the same seeds are kept,
the batch is the full one (the kernels' launch geometry is that of the main test), and the cotangent is non-zero ONLY on the
tied cases -- the very ones that carried a zero cotangent until round 6.  Each of them must reproduce the fp64 gradient of one
admissible combination of its tied decisions at GTOL, and the parameter gradients must equal the sum of the chosen combinations'
fp64 parameter gradients (a gate taken one way for dx and another way for dW fails that).  The method and its own tests:
tests/knife_units.py, tests/test_knife_units.py; measured figures: profiles/r07_knife_resolution.txt."""
import pytest
import torch

import knife_units as K
from conftest import rel_err, assert_close, assert_fwd
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


def dev(t):
    return t.clone().to(DEV).requires_grad_(True)


@pytest.mark.parametrize("n,kind", [(700, "dense"), (1300, "sparse"), (515, "sparse"), (257, "dense")])
def test_conv_front_tied_images_match_an_admissible_decision(n, kind):
    """cnn_fwd_wino_k / the tie-exact forward and cnn_bwd_wino_k on the tied images of the raw draw: the recorded argmax of
    every tied window is one of its admissible entries, de of every tied image equals the fp64 gradient under that argmax and
    one combination of its tied ReLU gates at < GTOL (per-image measure of the main test), dW1 / db1 / dW2 / db2 equal the sum
    of the chosen combinations' gradients.
    Measured figures: profiles/r07_knife_resolution.txt."""
    import torch.nn.functional as F
    from gnf_hip import ops, abi
    (e, W1, b1, W2, b2), _ = K.draw_conv_front(n, kind)
    params = (W1, b1, W2, b2)
    tied, live = K.conv_front_live_images(*K.conv_front_tied_units(e, *params))
    gp = torch.randn(n, 2304) * live.float().unsqueeze(1)
    pg = [dev(t) for t in (e, *params)]
    out = ops.MnistConvFn.apply(*pg, kind == "sparse")
    ref = torch.flatten(F.max_pool2d(F.conv2d(torch.relu(F.conv2d(e.view(-1, 1, 28, 28), W1, b1)), W2, b2), 2), 1)
    assert rel_err(out.cpu(), ref) < TOL                      # forward values of the tied images: compared like everyone's
    assert_fwd(out, ref, what="out")
    assert_close(out, ref, rtol=1e-5, atol=1e-6 * ref.abs().max().item(), what="pooled (every image)")
    (out * gp.to(DEV)).sum().backward()
    # the argmax the backward consumed: the same entry point on the same inputs
    pooled = torch.empty_like(out)
    arg = torch.empty((n, 2304), dtype=torch.uint8, device=DEV)
    ops.call("gnf_mnistcnn_conv_fwd", *[ops.ptr(t.detach().contiguous()) for t in pg], ops.ptr(pooled), abi.rawptr(arg), n,
             int(kind == "sparse"), ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(pooled, out.detach()) and int(arg.max()) <= 3
    st = K.judge_conv_front(e, params, gp, pg[0].grad.cpu(), [p.grad.cpu() for p in pg[1:]], arg.cpu().long())
    print("KNIFE conv front n=%d %s (MI355X): %s" % (n, kind, st))


@pytest.mark.parametrize("B,d,hidden", [(300, 7, [50, 50, 50]), (1373, 6, [100, 100, 100]), (300, 7, [200, 200]),
                                        (420, 5, [200, 200, 200]), (131, 17, [40, 64, 24])])
def test_monotonic_tied_elements_match_an_admissible_gate_combination(B, d, hidden):
    """the narrow kernels (mono_bwd_pair_x_k, the tall wgrad path), the wide kernel and its weight-swapping mode on the tied
    elements of the raw draw: (dx, dh[b,i,:]) of every tied element equals the fp64 gradient under one combination of its tied
    gates within GTOL of the reference tensors' maxima, and every dW / db equals the sum of the chosen combinations' gradients.
    Most combinations of an element differ by less than that tolerance in (dx, dh) (one gate at one of 22 nodes); the choice
    among those is settled by the parameter-gradient residual (knife_units.settle_ambiguous) and the count is reported.
    Measured figures: profiles/r07_knife_resolution.txt."""
    c, S = 30, 20
    (norm, x, h), _ = K.draw_monotonic(B, d, hidden, c, S)
    layers = K.layers_cpu(norm)
    tied, live = K.monotonic_live_elements(K.integrand_tied_gates(x, h, layers, S), x.shape)
    gz, gj = torch.randn(B, d) * live.float(), torch.randn(B, d) * live.float()
    with torch.no_grad():
        z0, j0 = O.monotonic_forward(x, h, layers, S)
    norm = norm.to(DEV)
    xg, hg = dev(x), dev(h)
    z, jac = norm(xg, hg)
    assert rel_err(z.cpu(), z0) < TOL and rel_err(jac.cpu(), j0) < TOL
    assert_fwd(z, z0, what="z")
    assert_fwd(jac, j0, what="jac")
    ((z * gz.to(DEV)).sum() + (jac * gj.to(DEV)).sum()).backward()
    st = K.judge_monotonic(x, h, layers, S, gz, gj, xg.grad.cpu(), hg.grad.cpu(),
                           [p.grad.cpu() for p in norm.integrand_net.flat_params()])
    print("KNIFE Monotonic %s (MI355X): %s" % ((B, d, hidden), st))
