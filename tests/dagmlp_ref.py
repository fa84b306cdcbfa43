"""Helpers shared by the tests of the DAGMLP front with the gate fused in (tests/test_gpu_dagmlp_gated.py,
tests/test_dagmlp_gated_host.py): the gate cases, seeded conditioners and draws, the fp64 reference (the oracle's masked
copies followed by the linear chain in fp64 torch) and the fp64 finder of tied samples -- samples one of whose d copies has
a hidden ReLU pre-activation within fp32 roundoff of zero, where the fused first layer (another summation order than the
GEMM on e) may legitimately decide differently."""
import torch

from oracle import gnf_oracle as O

EPS32 = float(torch.finfo(torch.float32).eps)
DEV = "cuda:0"

# (B, d, H): the edges of the issue
SHAPES = [(1, 1, 16), (5, 3, 2), (1, 6, 60), (7, 6, 60), (300, 8, 80), (100, 21, 210), (33, 43, 430), (64, 63, 630),
          (2500, 6, 60)]

# gate case -> (stoch_gate, noise_gate, gumble_T, h_thresh, injected noise)
CASES = {"det": (False, False, 1., 0., False),
         "gumbel-injected": (True, False, 1., 0., True),
         "gumbel-injected-T.5": (True, False, .5, 0., True),
         "philox-T.5": (True, False, .5, 0., False),
         "philox-T.7": (True, False, .7, 0., False),
         "noise-gate": (False, True, 1., 0., True),
         "h_thresh": (True, False, 1., .3, True)}
INJECTED = [k for k, v in CASES.items() if v[4] or k == "det"]


def cu(t):
    return t.to(DEV)


def hidden_of(d, H):
    """the reference's three hidden layers where the tied share lets a redraw terminate (d <= 8), one hidden layer above"""
    return [H, H, H] if d <= 8 else [H]


def make_cond(d, hidden, out, hot, case, seed, device="cpu"):
    """a seeded DAGConditioner in the state of `case`; A is redrawn so that every entry matters, diagonal included (for
    h_thresh: about half of the soft-thresholded importances lie below the threshold).

    The range of |A|: the gate's (i, j) table (csrc/gnf_dag_gate.h, shared by the composed path and the fused kernels) holds
    ((1 - p + eps) / (p + eps))^(1/T) and 1/(1 - p + eps) evaluated in fp32 from the fp32 importance p, so their relative
    error is eps32 / (1 - p): 1e-5 -- the whole forward tolerance -- at 1 - p = 6e-3 (|A| = 1.7), 1e-4 at |A| = 2.  That is the
    fp32 conditioning of the reference's own formula (DAGConditioner.py:95-103), not a property of any kernel, and an fp64
    evaluation from A does not share it.  |A| is therefore drawn from [.3, 1.1], where p lies in [.09, .84] and both p and
    1 - p are well conditioned (relative error < 1e-6), with random signs."""
    from models import DAGConditioner
    stoch, noise, T, h_thresh, _ = CASES[case]
    torch.manual_seed(seed)
    cond = DAGConditioner(d, list(hidden), out, hot_encoding=hot, gumble_T=T)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        sign = (torch.rand(d, d, generator=gen) < .5).float() * 2. - 1.
        if h_thresh > 0:                                       # soft(A) = .3 at |A| = .556
            cond.A.copy_(sign * (.556 + .25 * (2. * torch.rand(d, d, generator=gen) - 1.)))
        else:
            cond.A.copy_(sign * (.3 + .8 * torch.rand(d, d, generator=gen)))
    cond.stoch_gate, cond.noise_gate, cond.h_thresh = stoch, noise, h_thresh
    cond.gate_seed, cond._gate_calls = 1234567 + seed, 40
    cond.invalidate_caches()
    return cond.to(device)


def draw_inputs(B, d, case, gen):
    """(x, u1, u2): x [B, d]; the injected noise of the case as [B, d, d] tensors (uniforms for the Gumbel gate, a normal
    sample in u1 for the noise gate; ones where the case takes none, so that the tuple always has three tensors)"""
    stoch, noise, _, _, injected = CASES[case]
    x = torch.randn(B, d, generator=gen)
    one = torch.ones(B, d, d)
    if not injected:
        return x, one, one
    if stoch:
        return x, torch.rand(B, d, d, generator=gen) * .98 + .01, torch.rand(B, d, d, generator=gen) * .98 + .01
    return x, torch.randn(B, d, d, generator=gen), one


def set_noise(cond, case, u1, u2):
    stoch, noise, _, _, injected = CASES[case]
    if not injected:
        cond.gate_noise = None
    elif stoch:
        cond.gate_noise = (cu(u1), cu(u2))
    else:
        cond.gate_noise = (cu(u1), None)


def layers64(cond):
    from models.Conditionners.Conditioner import linear_pairs
    return [(W.detach().cpu().double(), b.detach().cpu().double()) for W, b in linear_pairs(cond.embedding_net.net)]


def copies64(cond, case, x, u1, u2, A=None):
    """the oracle's masked copies in fp64 (autograd through x and A when they require grad)"""
    stoch, noise, T, h_thresh, _ = CASES[case]
    A = cond.A.detach().cpu().double() if A is None else A
    return O.dag_masked_inputs(x, A, bool(cond.s_thresh), float(h_thresh), stoch, noise, float(T),
                               u1.double() if stoch else None, u2.double() if stoch else None,
                               u1.double() if noise else None, bool(cond.hot_encoding))


def chain64(e, layers, keep=None):
    """the Linear/ReLU chain in fp64; keep: a list that receives the pre-activation of the first layer"""
    a = e
    for l, (W, b) in enumerate(layers):
        a = a @ W.t() + b
        if l == 0 and keep is not None:
            keep.append(a)
        if l < len(layers) - 1:
            a = torch.relu(a)
    return a


def tied_samples(e, layers, B, d, ulps=16.):
    """[B] bool: samples one of whose d copies has a hidden pre-activation within `ulps` fp32 ulps of its terms' magnitude of
    zero without being zero (the criterion of conftest.integrand_knife_elements), fp64"""
    a = e.detach()
    tied = torch.zeros(B, dtype=torch.bool)
    for W, b in layers[:-1]:
        pre = a @ W.t() + b
        mag = a.abs() @ W.abs().t() + b.abs()
        tied |= ((pre.abs() < ulps * EPS32 * mag) & (pre != 0)).any(1).view(B, d).any(1)
        a = torch.relu(pre)
    return tied


def graph_nodes(t):
    """names of the autograd nodes behind t"""
    seen, names, stack = set(), set(), [t.grad_fn]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        stack += [n for n, _ in f.next_functions]
    return names


def assert_grad(a, b, what):
    """rel_err < 1e-4 of the tensor maximum, and per entry 1e-6 max|b| + 1e-4 |b|"""
    from conftest import assert_close, rel_err
    b = torch.as_tensor(b)
    if b.numel() == 0:
        assert a.numel() == 0
        return
    assert rel_err(a.detach().cpu(), b.detach().cpu()) < 1e-4, (what, rel_err(a.detach().cpu(), b.detach().cpu()))
    assert_close(a, b, rtol=1e-4, atol=1e-6 * float(b.detach().abs().max()), what=what)
