import torch.nn as nn


def linear_pairs(seq):
    """[(weight, bias)] of the nn.Linear members of an nn.Sequential, in order."""
    return [(m.weight, m.bias) for m in seq if isinstance(m, nn.Linear)]


def no_context(context, cond_in=0):
    """The rule of a conditioner built WITHOUT a context input (cond_in == 0): only context=None is accepted.  (`context` is
    dead in the reference, whose three conditioners fail when cond_in > 0; with cond_in > 0 the conditioners
    here take one, see checked_context.)"""
    if context is not None or cond_in:
        raise NotImplementedError("context conditioning (cond_in > 0) is not supported "
                                  "(it raises in the reference as well)")


def checked_context(context, cond_in, x):
    """The context a conditioner built with `cond_in` evaluates x [B, ...] with: None for cond_in == 0 (where any context
    still raises, as no_context does), else the fp32 [B, cond_in] tensor itself -- ValueError when it is missing or has
    another shape.  The same tensor serves every step of a flow; normalizers ignore it (divergence table)."""
    if not cond_in:
        no_context(context, 0)
        return None
    if context is None:
        raise ValueError("this conditioner was built with cond_in = %d: forward needs a [B, %d] context" % (cond_in, cond_in))
    if context.dim() != 2 or context.shape[0] != x.shape[0] or context.shape[1] != cond_in:
        raise ValueError("context must be [%d, %d] (batch of x, cond_in): got %s"
                         % (x.shape[0], cond_in, tuple(context.shape)))
    return context


class Conditioner(nn.Module):
    """Plug-in protocol of the reference (models/Conditionners/Conditioner.py:4-23):
    forward(x[B,d], context=None) -> h[B,d,hs]; depth() -> longest path of the equivalent
    Bayesian network; attribute is_invertible."""

    def __init__(self):
        super(Conditioner, self).__init__()
        self.is_invertible = True

    def forward(self, x, context=None):
        pass

    def depth(self):
        pass


def relu_stack(sizes):
    """nn.Sequential(Linear, ReLU, Linear, ..., Linear) over consecutive `sizes`: the parameter container every
    conditioner MLP of the reference uses (keys net.0, net.2, ...)."""
    mods = []
    for i, (n_in, n_out) in enumerate(zip(sizes[:-1], sizes[1:])):
        if i:
            mods.append(nn.ReLU())
        mods.append(nn.Linear(n_in, n_out))
    return nn.Sequential(*mods)

