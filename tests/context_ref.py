"""fp64 references of the conditional conditioners and flows (cond_in > 0; tests/test_gpu_context.py,
tests/test_context_host.py): plain torch on the CPU, built from a module's own parameters and mask buffers.

Semantics (divergence table): the context is one fp32 [B, cond_in] tensor, the same for every step of a flow;
normalizers ignore it.  Coupling: the MLP reads cat(x[:, :indep], context).  MADE: the first masked layer reads
cat(context, x) and the mask buffer carries the rule.  DAG: row b*d + i of the embedding net's input is (e[b*d+i] | context[b])."""
import torch

from oracle import gnf_oracle as O
from dagmlp_ref import CASES, chain64, copies64, tied_samples

DEV = "cuda:0"


def d64(t):
    return t.detach().cpu().double()


def leaves64(module):
    """{name: fp64 leaf requiring grad} of every parameter of `module`"""
    return {n: d64(p).clone().requires_grad_(True) for n, p in module.named_parameters()}


def _pairs(P, prefix):
    out, k = [], 0
    while "%snet.%d.weight" % (prefix, k) in P:
        out.append((P["%snet.%d.weight" % (prefix, k)], P["%snet.%d.bias" % (prefix, k)]))
        k += 2
    return out


# ------------------------------------------------------------------------------------------------------- conditioners
def coupling64(cond, P, x, ctx, prefix=""):
    """h [B, d, out] of a CouplingConditioner from the fp64 leaves P (names relative to `prefix`)"""
    B = x.shape[0]
    first = torch.cat((x[:, :cond.indep_size], ctx), 1)
    learned = O.mlp(first, _pairs(P, prefix + "embeding_net.")).view(B, cond.cond_size, cond.out_size)
    return torch.cat((P[prefix + "constants"].unsqueeze(0).expand(B, -1, -1), learned), 1)


def made64(cond, P, x, ctx, prefix=""):
    """h [B, d, out] of an AutoregressiveConditioner: masked linears on cat(context, x) with the module's mask buffers"""
    net = cond.masked_autoregressive_net
    masks = [d64(l.mask) for l in net.masked_layers()]
    a = torch.cat((ctx, x), 1)
    layers = _pairs(P, prefix + "masked_autoregressive_net.")
    for li, ((W, b), M) in enumerate(zip(layers, masks)):
        a = a @ (M * W).t() + b
        if li < len(layers) - 1:
            a = torch.relu(a)
    return a.view(x.shape[0], -1, x.shape[1]).permute(0, 2, 1)


def dag_rows64(cond, case, x, ctx, u1, u2, A=None):
    """the rows the embedding net reads: the oracle's masked copies with context[b] appended to the d copies of sample b"""
    e = copies64(cond, case, x, u1, u2, A=A)
    return torch.cat((e, ctx.repeat_interleave(cond.in_size, 0)), 1)


def dag64(cond, P, case, x, ctx, u1, u2, prefix="", keep=None):
    """h [B, d, out] of a DAGConditioner with a DAGMLP; A is the leaf P[prefix + 'A'] when it is one"""
    A = P.get(prefix + "A")
    rows = dag_rows64(cond, case, x, ctx, u1, u2, A=A if A is not None else d64(cond.A))
    return chain64(rows, _pairs(P, prefix + "embedding_net."), keep).view(x.shape[0], cond.in_size, -1)


def dag_tied(cond, case, B, d):
    """is_tied(x, ctx, u1, u2) for knife_units.resample_off_ties: dagmlp_ref.tied_samples on the copies with the context appended"""
    from dagmlp_ref import layers64
    L = layers64(cond)
    return lambda x, ctx, u1, u2: tied_samples(dag_rows64(cond, case, x.double(), ctx.double(), u1, u2), L, B, d)


def coupling_tied(cond):
    """is_tied(x, ctx): dagmlp_ref.tied_samples on the rows a CouplingMLP reads (one row per sample)"""
    from models.Conditionners.Conditioner import linear_pairs
    L = [(d64(W), d64(b)) for W, b in linear_pairs(cond.embeding_net.net)]
    return lambda x, ctx: tied_samples(torch.cat((x[:, :cond.indep_size], ctx), 1).double(), L, x.shape[0], 1)


def made_tied(cond):
    """is_tied(x, ctx): the same criterion on the masked layers of the conditional MADE"""
    L = [(d64(l.mask) * d64(l.weight), d64(l.bias)) for l in cond.masked_autoregressive_net.masked_layers()]
    return lambda x, ctx: tied_samples(torch.cat((ctx, x), 1).double(), L, x.shape[0], 1)


# (B, d, H, cond_in) of the DAG conditioner tests and the gate cases of dagmlp_ref.CASES they run
DAG_SHAPES = [(1, 1, 16, 1), (5, 3, 2, 2), (7, 6, 60, 3), (33, 43, 430, 1)]
DAG_GATES = ("det", "gumbel-injected", "noise-gate")
DAG_OUT = 10


def dag_case(shape, hot, case, device="cpu"):
    """the seeded conditioner and tie-free draw of one DAG case: (cond, (x, ctx, u1, u2), cotangent [B, d, out], redraw rounds).
    The draw and the tie search are fp64 on the CPU and do not depend on `device`."""
    from dagmlp_ref import draw_inputs, hidden_of
    from knife_units import resample_off_ties
    B, d, H, c = shape
    cond = make_dag(d, hidden_of(d, H), DAG_OUT, hot, case, 500 + B + d + (17 if hot else 0), c)
    gen = torch.Generator().manual_seed(5000 + B * d + H + (1 if hot else 0))

    def draw():
        x, u1, u2 = draw_inputs(B, d, case, gen)
        return x, torch.randn(B, c, generator=gen), u1, u2

    inputs, rounds = resample_off_ties(draw, dag_tied(cond, case, B, d))
    cot = torch.randn(B, d, DAG_OUT, generator=gen)
    return cond.to(device), inputs, cot, rounds


def make_dag(d, hidden, out, hot, case, seed, c, device="cpu"):
    """dagmlp_ref.make_cond with cond_in = c: a seeded DAGConditioner in the state of `case`, |A| in [.3, 1.1] with random
    signs (the conditioning argument is in dagmlp_ref.make_cond)"""
    from models import DAGConditioner
    stoch, noise, T, h_thresh, _ = CASES[case]
    torch.manual_seed(seed)
    cond = DAGConditioner(d, list(hidden), out, cond_in=c, hot_encoding=hot, gumble_T=T)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        sign = (torch.rand(d, d, generator=gen) < .5).float() * 2. - 1.
        cond.A.copy_(sign * (.3 + .8 * torch.rand(d, d, generator=gen)))
    cond.stoch_gate, cond.noise_gate, cond.h_thresh = stoch, noise, h_thresh
    cond.gate_seed, cond._gate_calls = 1234567 + seed, 40
    cond.invalidate_caches()
    return cond.to(device)


# ------------------------------------------------------------------------------------------------------------- flows
def flow64(flow, P, x, ctx):
    """(z, logdet, loss) of an FCNormalizingFlow of Coupling / Autoregressive / deterministic-gate DAG steps with Affine or
    Monotonic normalizers, from the fp64 leaves P of flow.named_parameters()"""
    from models import AffineNormalizer, AutoregressiveConditioner, CouplingConditioner, DAGConditioner
    steps, constraints = [], 0.
    for k, step in enumerate(flow.steps):
        cond, norm, pre = step.conditioner, step.normalizer, "steps.%d.conditioner." % k
        if isinstance(cond, CouplingConditioner):
            cfn = lambda v, cond=cond, pre=pre: coupling64(cond, P, v, ctx, pre)
        elif isinstance(cond, AutoregressiveConditioner):
            cfn = lambda v, cond=cond, pre=pre: made64(cond, P, v, ctx, pre)
        else:
            assert isinstance(cond, DAGConditioner) and cond.deterministic_importance() is not None
            one = torch.ones(x.shape[0], cond.in_size, cond.in_size)
            cfn = lambda v, cond=cond, pre=pre: dag64(cond, P, "det", v, ctx, one, one, pre)
            A = P.get(pre + "A", d64(cond.A))
            constraints = constraints + O.dag_loss(A, d64(cond.alpha).clamp(max=1.) * cond.alpha_factor, int(cond.exponent),
                                                   d64(cond.lambd), d64(cond.c), d64(cond.dag_const), d64(cond.l1_weight))
        if isinstance(norm, AffineNormalizer):
            nfn = O.affine_forward
        else:
            layers = _pairs(P, "steps.%d.normalizer.integrand_net." % k)
            nfn = lambda v, h, layers=layers, S=int(norm.nb_steps): O.monotonic_forward(v, h, layers, S)
        steps.append((cfn, nfn))
    z, logdet = O.fc_flow_forward(x, steps)
    return z, logdet, O.flow_loss(z, logdet, constraints)
