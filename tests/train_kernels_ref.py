"""fp64 restatements of the operations the training kernels replace (bn_train.hip): train-mode BatchNorm2d statistics,
the normalise + activation + skip-add pass, its backward, the bias gradient and the gradient of nearest 2x upsampling; and of
the convolution's weight gradient (wgrad_*.hip).

Plain torch, no project code; CPU or device tensors. Every input is taken as stored (already rounded to its dtype) and
promoted to fp64. Channels are the LAST dimension everywhere (NHWC, or (m, c) with the pixels flattened); per-channel
vectors have shape (c,). ``tests/test_train_kernels_ref_host.py`` ties these functions to torch.autograd in fp64.
"""
import numpy as np
import torch

ACT_NONE, ACT_LEAKY, ACT_MISH = 0, 1, 2
LEAKY_SLOPE = 0.1


def _d(t):
    return None if t is None else torch.as_tensor(t).double()


def act_ref(v, act):
    v = _d(v)
    if act == ACT_NONE:
        return v
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, LEAKY_SLOPE * v)
    if act == ACT_MISH:
        return v * torch.tanh(torch.logaddexp(v, torch.zeros_like(v)))      # softplus(v) = log(1 + e^v), no overflow
    raise ValueError(act)


def act_grad_ref(u, act):
    u = _d(u)
    if act == ACT_NONE:
        return torch.ones_like(u)
    if act == ACT_LEAKY:
        return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, LEAKY_SLOPE))
    if act == ACT_MISH:
        t = torch.tanh(torch.logaddexp(u, torch.zeros_like(u)))
        return t + u * (1.0 - t * t) * torch.sigmoid(u)
    raise ValueError(act)


def _chunks(m, rows):
    rows = m if not rows else rows
    return [(a, min(m, a + rows)) for a in range(0, m, rows)]


def bn_stats_ref(z, gamma, beta, eps, momentum, rm=None, rv=None, chunk_rows=None):
    """(mean, invstd, scale, shift, new running mean, new running var) of z (..., c) over all leading dimensions.
    Biased variance for the normalisation; the running variance takes the unbiased one, except that a single value per
    channel (m == 1) leaves it biased. rm / rv None: the running statistics are returned as None.
    chunk_rows: promote that many pixels at a time (the same two-pass fp64 sums without an fp64 copy of a large z)."""
    z = torch.as_tensor(z)
    z = z.reshape(-1, z.shape[-1])
    m = z.shape[0]
    mean = sum(_d(z[a:b]).sum(0) for a, b in _chunks(m, chunk_rows)) / m
    var = sum(((_d(z[a:b]) - mean) ** 2).sum(0) for a, b in _chunks(m, chunk_rows)) / m
    invstd = 1.0 / torch.sqrt(var + eps)
    scale, shift = _d(gamma) * invstd, _d(beta).clone()
    if rm is None:
        return mean, invstd, scale, shift, None, None
    unbiased = var * m / (m - 1) if m > 1 else var
    return mean, invstd, scale, shift, (1.0 - momentum) * _d(rm) + momentum * mean, (1.0 - momentum) * _d(rv) + momentum * unbiased


def bn_act_fwd_ref(z, mean, scale, shift, act, residual=None):
    """act((z - mean) * scale + shift) + residual; mean None means 0, residual None means none."""
    z = _d(z)
    u = (z - _d(mean) if mean is not None else z) * _d(scale) + _d(shift)
    y = act_ref(u, act)
    return y if residual is None else y + _d(residual)


def bn_act_bwd_ref(dy, z, gamma, mean, invstd, scale, shift, act, totals=None):
    """(dgamma, dbeta, dz, u, du, zhat) of y = act(u), u = (z - mean) * scale + shift, zhat = (z - mean) * invstd:
    du = dy * act'(u); dbeta = sum du; dgamma = sum du * zhat; dz = gamma * invstd * (du - dbeta / m - zhat * dgamma / m).
    dy and z are (m, c) (or (..., c): the leading dimensions are the batch). totals = (dgamma, dbeta, m): dy and z are only
    some pixels of a batch whose sums (added up from the u, du, zhat of such calls) and size are given."""
    dy, z = _d(dy), _d(z)
    c = z.shape[-1]
    dy2, z2 = dy.reshape(-1, c), z.reshape(-1, c)
    zc = z2 - _d(mean)
    u = zc * _d(scale) + _d(shift)
    zhat = zc * _d(invstd)
    du = dy2 * act_grad_ref(u, act)
    if totals is None:
        dgamma, dbeta, m = (du * zhat).sum(0), du.sum(0), z2.shape[0]
    else:
        dgamma, dbeta, m = totals
    dz = _d(gamma) * _d(invstd) * (du - dbeta / m - zhat * (dgamma / m))
    return dgamma, dbeta, dz.reshape(z.shape), u.reshape(z.shape), du.reshape(z.shape), zhat.reshape(z.shape)


def bias_grad_ref(dy):
    dy = _d(dy)
    return dy.reshape(-1, dy.shape[-1]).sum(0)


def upsample2x_bwd_ref(dup):
    """Gradient of nearest-neighbour 2x upsampling: dup (n, 2h, 2w, c) -> (n, h, w, c), each source pixel sums its 2x2 copies."""
    dup = _d(dup)
    return (dup[:, 0::2, 0::2] + dup[:, 0::2, 1::2]) + (dup[:, 1::2, 0::2] + dup[:, 1::2, 1::2])


def upsample2x_bwd_abs_ref(dup):
    """Sum of the magnitudes of the four terms (the scale of the rounding bound)."""
    a = _d(dup).abs()
    return a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]


def wgrad_ref(x, dz, k, stride):
    """Weight gradient of conv2d(padding = k // 2): x (n, h, w, cin), dz (n, ho, wo, cout), both NHWC -> dW (cout, cin, k, k):
    dW[co, ci, kh, kw] = sum over n, ho, wo of dz[n, ho, wo, co] * x[n, ho * stride + kh - pad, wo * stride + kw - pad, ci],
    as k * k shifted sums over the pixels both operands have. fp64 whatever the inputs are, on their device."""
    n, h, w, cin = x.shape
    ho, wo, cout = dz.shape[1], dz.shape[2], dz.shape[3]
    pad = k // 2
    x, dz = _d(x), _d(dz)
    dw = torch.zeros((cout, cin, k, k), dtype=torch.float64, device=x.device)
    for kh in range(k):
        for kw in range(k):
            # output rows / columns whose tap (kh, kw) lies inside the image
            a0, a1 = max(0, -((kh - pad) // stride)), min(ho, (h - 1 - kh + pad) // stride + 1)
            b0, b1 = max(0, -((kw - pad) // stride)), min(wo, (w - 1 - kw + pad) // stride + 1)
            if a1 <= a0 or b1 <= b0:
                continue
            xs = x[:, a0 * stride + kh - pad:(a1 - 1) * stride + kh - pad + 1:stride,
                   b0 * stride + kw - pad:(b1 - 1) * stride + kw - pad + 1:stride]
            dw[:, :, kh, kw] = torch.einsum("nhwc,nhwd->dc", xs, dz[:, a0:a1, b0:b1])
    return dw


def mish_fp32_formula_rel_error(lo=-30.0, hi=30.0, n=600001):
    """Largest relative error over [lo, hi] of a PLAIN fp32 evaluation (accurate exp, one rounding per operation) of the
    formula the kernels use for Mish, v * n / (n + 2) with n = e (e + 2), e = exp(min(v, 20)) and v itself above 20,
    against fp64 v * tanh(softplus(v)). The kernels' hardware exp and reciprocal come on top of this figure."""
    v = np.linspace(lo, hi, n).astype(np.float32)
    f = np.float32
    e = np.exp(np.minimum(v, f(20.0)).astype(np.float64)).astype(np.float32)       # correctly rounded fp32 exp
    nn = (e * (e + f(2.0))).astype(np.float32)
    got = np.where(v > f(20.0), v, (v * (nn / (nn + f(2.0))).astype(np.float32)).astype(np.float32)).astype(np.float64)
    v64 = v.astype(np.float64)
    want = v64 * np.tanh(np.logaddexp(v64, 0.0))
    nz = want != 0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz])))


def ulp_of(x, dtype):
    """Unit in the last place of the values x (fp64 tensor) in a torch floating dtype (the spacing of its binade,
    the subnormal spacing below the smallest normal)."""
    p, emin = {torch.float32: (23, -126), torch.float16: (10, -14), torch.bfloat16: (7, -126)}[dtype]
    x = _d(x).abs()
    e = torch.frexp(x)[1].double() - 1.0                 # floor(log2 |x|) for x != 0
    e = torch.where(x == 0, torch.full_like(e, float(emin)), torch.clamp(e, min=float(emin)))
    return torch.exp2(e - p)
