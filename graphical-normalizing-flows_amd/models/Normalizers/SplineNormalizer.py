import torch

from gnf_hip import ops
from .Normalizer import Normalizer


class SplineNormalizer(Normalizer):
    """Monotone rational-quadratic spline transformer (Durkan et al., Neural Spline Flows, 2019) with `nb_bins` bins on
    [-tail_bound, tail_bound] and the identity outside, on the fused gfx950 kernels (include/gnf_hip.h, gnf_spline_*).

    Per variable the conditioner supplies 3 nb_bins - 1 numbers: nb_bins width logits, nb_bins height logits and the
    nb_bins - 1 derivative logits of the interior knots (`h_size` tells a factory that width); components beyond are
    ignored.  Forward, inverse and log-derivative are closed-form and element-wise; the normalizer has no parameters."""

    def __init__(self, nb_bins=8, tail_bound=3.):
        super(SplineNormalizer, self).__init__()
        self.nb_bins = int(nb_bins)
        self.tail_bound = float(tail_bound)
        if not 2 <= self.nb_bins <= 32:
            raise ValueError("SplineNormalizer: nb_bins = %d, must be 2 .. 32" % self.nb_bins)
        if not self.tail_bound > 0.:
            raise ValueError("SplineNormalizer: tail_bound = %r, must be positive" % (tail_bound,))

    @staticmethod
    def h_size(nb_bins=8, **_):
        """conditioner outputs per variable"""
        return 3 * int(nb_bins) - 1

    def forward(self, x, h, context=None):
        z, jac, _, _ = ops.SplineFn.apply(x, h, self.nb_bins, self.tail_bound)
        return z, jac

    def forward_logdet(self, x, h, context=None):
        """(z, log|det J|) with the row reduction fused into the kernel that computes z (used by NormalizingFlowStep)"""
        z, _, logdet, _ = ops.SplineFn.apply(x, h, self.nb_bins, self.tail_bound, False, False)
        return z, logdet

    def inverse_transform(self, z, h, context=None):
        with torch.no_grad():
            return ops.spline_inverse(z, h, self.nb_bins, self.tail_bound)

    def inverse_transform_into(self, z, h, out, cols, context=None):
        """out[:, cols] = inverse_transform(z, h).t() for a variable-major problem (z [R, B], h [R, B, c], out [B, d], cols
        int32 [R]): the kernel writes where the values belong.  Returns False when that form does not apply."""
        if not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32):
            return False
        with torch.no_grad():
            ops.spline_inverse(z, h, self.nb_bins, self.tail_bound, out=out, out_cols=cols)
        return True
