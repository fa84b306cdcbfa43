"""Golden vectors of the CIFAR-10 embedding net and factory, from the REFERENCE ITSELF (build container only).

    python tests/golden/make_golden_cifar.py      # writes tests/golden/cifar10cnn.npz

For each of the four geometries buildCIFAR10NormalizingFlow constructs (tests/lenet_ref.py: GEOMETRIES), the reference's own
CIFAR10CNN(out_d=2, ...) with its default initialisation: parameters `gK.p.*`, n = 3 seeded inputs `gK.x`, the output
`gK.out`, the cotangent `gK.g` and the gradients of (out * g).sum() w.r.t. the input (`gK.gx`) and every parameter
(`gK.g.*`).  The inputs are redrawn until an fp64 evaluation finds no knife-edge ReLU / pool decision in them
(lenet_ref.knife_images), so every fp32 evaluation order agrees on the subgradient.  n = 3 and out_d = 2 keep the file under
1 MB (the parameter gradients are as large as the parameters; fc1 alone is 576 x 128).

Also the `state_dict` key lists of buildCIFAR10NormalizingFlow([1], AffineNormalizer, {}) and ([1, 1, 1, 1], ...): names
only (`keys1`, `keys4`)."""
import os
import sys

import numpy as np
import torch

from make_golden import _import_reference, npy, save

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lenet_ref  # noqa: E402


def main():
    _import_reference()
    from models import AffineNormalizer
    from models.MLP import CIFAR10CNN
    from models.NormalizingFlowFactories import buildCIFAR10NormalizingFlow
    values = {}
    for gi, (size_img, k, fc_l) in enumerate(lenet_ref.GEOMETRIES):
        torch.manual_seed(100 + gi)
        net = CIFAR10CNN(out_d=2, fc_l=list(fc_l), size_img=list(size_img), k_size=k)
        p = {n: v.detach() for n, v in net.named_parameters()}
        gen = torch.Generator().manual_seed(200 + gi)
        x, left = lenet_ref.draw_clean_images(3, size_img, p["conv1.weight"], p["conv1.bias"], p["conv2.weight"],
                                              p["conv2.bias"], gen)
        assert left == 0, "knife-edge images left after the redraws"
        x.requires_grad_(True)
        out = net(x)
        g = torch.randn(out.shape, generator=gen)
        (out * g).sum().backward()
        tag = "g%d." % gi
        values.update({tag + "x": npy(x), tag + "out": npy(out), tag + "g": npy(g), tag + "gx": npy(x.grad)})
        for n, v in net.named_parameters():
            values[tag + "p." + n] = npy(v)
            values[tag + "g." + n] = npy(v.grad)
    for name, steps in (("keys1", [1]), ("keys4", [1, 1, 1, 1])):
        flow = buildCIFAR10NormalizingFlow(steps, AffineNormalizer, {})
        values[name] = np.array(list(flow.state_dict().keys()))
    save("cifar10cnn", **values)


if __name__ == "__main__":
    main()
