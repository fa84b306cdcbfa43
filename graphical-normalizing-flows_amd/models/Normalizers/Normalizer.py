import torch.nn as nn


class Normalizer(nn.Module):
    """Plug-in protocol of the reference (models/Normalizers/Normalizer.py:4-28):
    forward(x[B,d], h[B,d,hs], context=None) -> (z[B,d], jac[B,d]) with jac the diagonal
    Jacobian (not its log); inverse_transform(z, h, context=None) -> x[B,d]."""

    def __init__(self):
        super(Normalizer, self).__init__()

    def forward(self, x, h, context=None):
        pass

    def inverse_transform(self, z, h, context=None):
        pass

    def forward_logdet_do(self, x, h, pin, regime=None, context=None):
        """(z, logdet, logn) under do(x_S): forward's (z, jac) with log jac and log N(z) summed over the FREE variables
        only (pin uint8 [R, d], regime int32 [B] or None: models.NormalizingFlow.do_targets) in one masked reduction pass.
        A normalizer whose kernel can reduce over a row itself overrides this (AffineNormalizer)."""
        from gnf_hip import ops
        z, jac = self(x, h, context)
        logdet, logn = ops.NllDoFn.apply(z, jac, pin, regime)
        return z, logdet, logn
