"""Reference of gradient clipping by global norm (`yolo_for_turbines_amd/optim.py`, the `clip_*` kernels of `csrc/optim.hip`):
the contract, nothing else.

    inv_scale  = float32(1 / float64(scale))                               GradScaler.unscale_
    total_norm = sqrt(sum(float64(float32(g * inv_scale)) ** 2))           norm_type 2, in fp64 (the device rounds it to fp32 once)
               = max(|float32(g * inv_scale)|), NaN-propagating            norm_type inf
    coef       = min(fl(fl(1 / fl(total_norm + 1e-6f)) * max_norm), 1)     numpy.float32, every operation rounded on its own:
                                                                           torch.clamp(max_norm / (t + 1e-6), max=1.0)
"""
import numpy as np

BOUND = 2.0 ** -23      # |device norm - fp64 norm| <= BOUND * norm: n * 2^-53 of the fp64 sum, halved by the root, + one fp32 rounding


def inv_scale(scale):
    return np.float32(1.0 / np.float64(scale))


def unscaled(g, scale=None):
    """``g`` (a float32 array) as the step sees it: multiplied by the reciprocal of the scale, rounded to fp32."""
    g = np.asarray(g, dtype=np.float32)
    if scale is None:
        return g
    out = g * inv_scale(scale)
    assert out.dtype == np.float32
    return out


def total_norm(grads, scale=None, norm_type=2.0):
    """fp64 norm over a list of float32 arrays (2.0), or the fp32 maximum of their magnitudes (inf; NaN if any is NaN)."""
    gs = [unscaled(g, scale).reshape(-1) for g in grads]
    if norm_type == float("inf"):
        m = np.float32(0.0)
        for g in gs:
            if g.size:
                m = np.maximum(m, np.max(np.abs(g)))       # numpy's max and maximum propagate NaN
        return m
    assert norm_type == 2.0
    return np.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in gs))


def coef(total, max_norm):
    """The clip coefficient for an fp32 ``total`` as a numpy.float32."""
    with np.errstate(all="ignore"):
        t = np.float32(total) + np.float32(1e-6)
        r = np.float32(1.0) / t
        c = r * np.float32(max_norm)
    assert c.dtype == np.float32
    return c if (np.isnan(c) or c <= np.float32(1.0)) else np.float32(1.0)
