"""The monotone rational-quadratic spline (Durkan et al., Neural Spline Flows, 2019) in plain torch, dtype-generic: the only
reference of tests/test_spline_host.py and tests/test_gpu_spline.py.

K bins on [-T, T], identity outside; per element the conditioner outputs h[0 .. 3K-2] (components beyond are ignored):
    w = MIN + (1 - MIN K) softmax(h[0:K]),  X_0 = -T, X_k = -T + 2T sum_{j<k} w_j, X_K = T (forced), W_k = X_{k+1} - X_k
    the same from h[K:2K] for Y_k, H_k;  D_0 = D_K = 1, D_k = MIN + softplus(h[2K + k - 1])
    inside: k = #{j in 1..K-1: x >= X_j}, xi = (x - X_k)/W_k, s = H_k/W_k, e = D_{k+1} + D_k - 2s, den = s + e xi(1-xi)
        z = Y_k + H_k (s xi^2 + D_k xi(1-xi))/den,   jac = s^2 (D_{k+1} xi^2 + 2 s xi(1-xi) + D_k (1-xi)^2)/den^2
    outside (NaN, +-inf included): z = x, jac = 1
    inverse inside: bin by Y, dl = z - Y_k, a = H_k (s - D_k) + dl e, b = H_k D_k - dl e, c = -s dl,
        xi = 2c/(-b - sqrt(max(b^2 - 4ac, 0))), x = xi W_k + X_k
Everything is evaluated in the dtype of the inputs (fp64 for the truth, fp32 on the CPU for the error yardstick)."""
import torch
import torch.nn.functional as F

MIN = 1e-3


def knots(h, K, T):
    """(X [.., K+1], Y [.., K+1], D [.., K+1]) of conditioner outputs h [.., >= 3K-1]"""
    def cum(logits):
        w = MIN + (1. - MIN * K) * torch.softmax(logits, -1)
        c = torch.cumsum(w, -1)
        edge = torch.full_like(c[..., :1], T)
        return torch.cat((-edge, -T + 2. * T * c[..., :K - 1], edge), -1)
    one = torch.ones_like(h[..., :1])
    D = torch.cat((one, MIN + F.softplus(h[..., 2 * K:3 * K - 1]), one), -1)
    return cum(h[..., :K]), cum(h[..., K:2 * K]), D


def _bin(v, knot, K):
    return (v.unsqueeze(-1) >= knot[..., 1:K]).sum(-1)


def _take(t, k):
    return torch.gather(t, -1, k.unsqueeze(-1)).squeeze(-1)


def forward(x, h, K=8, T=3.):
    """(z, jac) of x [..] and h [.., C]"""
    X, Y, D = knots(h, K, T)
    inside = (x >= -T) & (x <= T)
    xs = torch.where(inside, x, torch.zeros_like(x))          # a harmless point inside: the branch is discarded below
    k = _bin(xs, X, K)
    Xk, Yk, D0, D1 = _take(X, k), _take(Y, k), _take(D, k), _take(D, k + 1)
    W, H = _take(X, k + 1) - Xk, _take(Y, k + 1) - Yk
    xi = (xs - Xk) / W
    s = H / W
    e = D1 + D0 - 2. * s
    q = xi * (1. - xi)
    den = s + e * q
    z = Yk + H * (s * xi * xi + D0 * q) / den
    jac = s * s * (D1 * xi * xi + 2. * s * q + D0 * (1. - xi) * (1. - xi)) / (den * den)
    return torch.where(inside, z, x), torch.where(inside, jac, torch.ones_like(x))


def inverse(z, h, K=8, T=3.):
    X, Y, D = knots(h, K, T)
    inside = (z >= -T) & (z <= T)
    zs = torch.where(inside, z, torch.zeros_like(z))
    k = _bin(zs, Y, K)
    Xk, Yk, D0, D1 = _take(X, k), _take(Y, k), _take(D, k), _take(D, k + 1)
    W, H = _take(X, k + 1) - Xk, _take(Y, k + 1) - Yk
    s = H / W
    e = D1 + D0 - 2. * s
    dl = zs - Yk
    a = H * (s - D0) + dl * e
    b = H * D0 - dl * e
    c = -s * dl
    xi = 2. * c / (-b - torch.sqrt(torch.clamp(b * b - 4. * a * c, min=0.)))
    return torch.where(inside, xi * W + Xk, z)


def logdet_logn(z, jac):
    """(sum_i log jac, -1/2 sum_i (log 2 pi + z^2)) of [B, d] tensors"""
    import math
    return torch.log(jac).sum(-1), -0.5 * (math.log(2. * math.pi) + z * z).sum(-1)


def knot_distance(x, h, K, T):
    """distance of x to the nearest X knot of its own spline (the ends -T, T are knots 0 and K), in the dtype of the inputs"""
    X, _, _ = knots(h, K, T)
    return (x.unsqueeze(-1) - X).abs().amin(-1)


def to_bin_middles(x, h, K, T, closer_than=1e-4):
    """x with every element closer than `closer_than` to a knot of its own spline (fp64 law) moved to the middle of its bin
    (of the first or last bin for elements near -T or T); fp32 in, fp32 out"""
    x64, h64 = x.double(), h.double()
    X, _, _ = knots(h64, K, T)
    near = knot_distance(x64, h64, K, T) < closer_than
    k = _bin(torch.clamp(x64, -T, T), X, K)
    mid = 0.5 * (_take(X, k) + _take(X, k + 1))
    return torch.where(near, mid, x64).float()
