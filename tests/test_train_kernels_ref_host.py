"""The fp64 references of tests/train_kernels_ref.py against torch.autograd in fp64 (CPU): they restate
``batch_norm(training=True) -> leaky_relu(0.1) / mish -> + residual`` and ``interpolate(scale_factor=2, nearest)``,
the operations the kernels of bn_train.hip replace. Agreement is asked to 1e-12 of the largest magnitude involved."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_kernels_ref as R

TOL = 1e-12
EPS, MOM = 1e-5, 0.1


def _rel(got, want, scale=None):
    s = float(want.abs().max()) if scale is None else float(scale)
    return float((got - want).abs().max()) / max(s, 1e-300)


def _chain(z, gamma, beta, rm, rv, act, res):
    # torch.batch_norm is what F.batch_norm calls, without the Python-side refusal of a single value per channel (m == 1)
    y = torch.batch_norm(z, gamma, beta, rm, rv, True, MOM, EPS, False)
    y = F.leaky_relu(y, 0.1) if act == R.ACT_LEAKY else F.mish(y)
    return y + res


@pytest.mark.parametrize("act", [R.ACT_LEAKY, R.ACT_MISH])
@pytest.mark.parametrize("nhw", [(1, 1, 1), (2, 1, 1), (3, 5, 7)])          # m = 1, 2, 105
def test_references_equal_autograd_fp64(nhw, act):
    n, h, w = nhw
    c, m = 6, n * h * w
    g = torch.Generator().manual_seed(1000 * m + act)
    z = (torch.randn((n, c, h, w), generator=g, dtype=torch.float64) * 1.5 + 0.3).requires_grad_(True)
    res = torch.randn((n, c, h, w), generator=g, dtype=torch.float64)
    dy = torch.randn((n, c, h, w), generator=g, dtype=torch.float64)
    gamma = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (torch.randn(c, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    rm0, rv0 = torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    y = _chain(z, gamma, beta, rm, rv, act, res)
    y.backward(dy)

    nhwc = lambda t: t.detach().permute(0, 2, 3, 1)
    mean, invstd, scale, shift, nrm, nrv = R.bn_stats_ref(nhwc(z), gamma.detach(), beta.detach(), EPS, MOM, rm0, rv0)
    assert _rel(nrm, rm) <= TOL
    if m > 1:
        assert _rel(nrv, rv) <= TOL
    else:
        # torch divides by m - 1 = 0 here; the kernels (and the reference) keep the biased variance, which is 0
        assert torch.equal(nrv, (1.0 - MOM) * rv0)
    got = R.bn_act_fwd_ref(nhwc(z), mean, scale, shift, act, nhwc(res))
    assert _rel(got, nhwc(y)) <= TOL
    dgamma, dbeta, dz, u, du, zhat = R.bn_act_bwd_ref(nhwc(dy), nhwc(z), gamma.detach(), mean, invstd, scale, shift, act)
    s_du, s_dz = float(du.abs().max()), float((gamma.detach() * invstd).abs().max() * du.abs().max())
    assert _rel(dbeta, beta.grad, m * s_du) <= TOL
    assert _rel(dgamma, gamma.grad, m * s_du * max(float(zhat.abs().max()), 1.0)) <= TOL
    assert _rel(dz, nhwc(z.grad), s_dz) <= TOL           # dz cancels to ~0 for m = 1, 2: relative to its terms
    assert _rel(R.bias_grad_ref(nhwc(dy)), dy.sum((0, 2, 3))) <= TOL


def test_m1_statistics_by_definition():
    z = torch.tensor([[1.5, -2.0, 0.25]], dtype=torch.float64)
    one, zero = torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    mean, invstd, scale, shift, nrm, nrv = R.bn_stats_ref(z, 2 * one, one, EPS, 0.03, zero, one)
    assert torch.equal(mean, z[0]) and torch.equal(shift, one)
    np.testing.assert_allclose(invstd.numpy(), EPS ** -0.5, rtol=1e-15)
    np.testing.assert_allclose(scale.numpy(), 2 * EPS ** -0.5, rtol=1e-15)
    np.testing.assert_allclose(nrm.numpy(), 0.03 * z[0].numpy(), rtol=1e-15)
    np.testing.assert_allclose(nrv.numpy(), 0.97, rtol=1e-15)
    assert R.bn_stats_ref(z, one, one, EPS, 0.1)[4:] == (None, None)


def test_forward_modes_of_the_apply_pass():
    g = torch.Generator().manual_seed(5)
    z, r = torch.randn((7, 4), generator=g, dtype=torch.float64), torch.randn((7, 4), generator=g, dtype=torch.float64)
    one, zero = torch.ones(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    assert torch.equal(R.bn_act_fwd_ref(z, None, one, zero, R.ACT_NONE, r), z + r)          # the gradient add
    assert torch.equal(R.bn_act_fwd_ref(z, zero, one, zero, R.ACT_NONE), z)
    assert _rel(R.bn_act_fwd_ref(z, None, one, zero, R.ACT_MISH), F.mish(z)) <= TOL
    assert _rel(R.act_grad_ref(z, R.ACT_MISH), torch.autograd.functional.jvp(F.mish, z, torch.ones_like(z))[1]) <= TOL


@pytest.mark.parametrize("shape", [(1, 1, 1, 3), (3, 5, 7, 4)])
def test_upsample_gradient_equals_autograd(shape):
    n, h, w, c = shape
    x = torch.zeros((n, c, h, w), dtype=torch.float64, requires_grad=True)
    dup = torch.randn((n, c, 2 * h, 2 * w), generator=torch.Generator().manual_seed(h), dtype=torch.float64)
    F.interpolate(x, scale_factor=2, mode="nearest").backward(dup)
    got = R.upsample2x_bwd_ref(dup.permute(0, 2, 3, 1))
    assert _rel(got, x.grad.permute(0, 2, 3, 1)) <= TOL
    assert bool((R.upsample2x_bwd_abs_ref(dup.permute(0, 2, 3, 1)) >= got.abs() - 1e-15).all())


def test_fp32_mish_formula_error_is_what_the_gpu_tolerance_assumes():
    """tests/test_gpu_train_kernels.py allows the Mish outputs 4x this figure; 2.7e-7 was measured when it was written."""
    e = R.mish_fp32_formula_rel_error()
    print(f"fp32 evaluation of v n / (n + 2) over [-30, 30]: max rel err {e:.3e}")
    assert 2.0 ** -24 < e < 2e-6


def test_ulp_of():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, 0.0, 2.0 ** -20, 3e-8], dtype=torch.float64)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        xs = x.to(dt)
        nxt = torch.nextafter(xs.float(), torch.full_like(xs.float(), float("inf"))) if dt == torch.float32 else None
        want = (nxt.double() - xs.double()) if nxt is not None else None
        got = R.ulp_of(xs.double(), dt)
        if want is not None:
            assert torch.equal(got, want)
    assert float(R.ulp_of(torch.tensor([1.0]), torch.float16)) == 2.0 ** -10
    assert float(R.ulp_of(torch.tensor([3.0]), torch.bfloat16)) == 2.0 ** -6
    assert float(R.ulp_of(torch.tensor([2.0 ** -20]), torch.float16)) == 2.0 ** -24
    assert float(R.ulp_of(torch.tensor([0.0]), torch.float16)) == 2.0 ** -24
