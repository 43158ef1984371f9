"""tests/conv_h16_ref.py on the CPU: the fp64 restatement of the 16-bit convolution block against torch.nn.functional and
oracle.net.cnn_block, and the two properties of the integer cases that tests/test_gpu_conv_patch_h16.py relies on when it
asks the kernels for bit equality:

  exactness   every partial sum of a case is bounded by K * 8 * 2 + |shift| + |residual| < 2^24, and an evaluation in fp32
              gives the very values of the evaluation in fp64 (with the kernels' two order-independent fp32 roundings stated,
              for LeakyReLU): the fp32 value ahead of the store is the same in any order of accumulation
  sharpness   at least half of the expected outputs of a bf16 case, and all of an fp16 or head case, are representable in
              the output type as they are: a wrong sum cannot hide in the rounding at the store. (LeakyReLU cases: asked of
              the outputs on the identity branch; v * 0.1f is never a 16-bit value, and its rounding is part of the reference.)
"""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_h16_ref as R

TOL = 1e-12
DTYPES = ["bf16", "fp16"]


def _rel(got, want):
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_LEAKY, R.ACT_MISH])
@pytest.mark.parametrize("shape", [(2, 5, 7, 6, 9, 1, 1), (3, 6, 5, 4, 7, 3, 1), (2, 8, 12, 5, 6, 3, 2), (1, 1, 1, 3, 2, 3, 1)])
def test_forward_reference_equals_torch_functional(shape, act):
    b, h, w, cin, cout, k, stride = shape
    g = torch.Generator().manual_seed(sum(shape) * 10 + act)
    x = torch.randn((b, cin, h, w), generator=g, dtype=torch.float64)
    wt = torch.randn((cout, cin, k, k), generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5, torch.randn(cout, generator=g, dtype=torch.float64)
    mean, var = torch.randn(cout, generator=g, dtype=torch.float64), torch.rand(cout, generator=g, dtype=torch.float64) + 0.5
    y = F.batch_norm(F.conv2d(x, wt, stride=stride, padding=k // 2), mean, var, gamma, beta, False, 0.1, 1e-5)
    y = F.leaky_relu(y, 0.1) if act == R.ACT_LEAKY else (F.mish(y) if act == R.ACT_MISH else y)
    res = torch.randn(y.shape, generator=g, dtype=torch.float64)
    scale = gamma / torch.sqrt(var + 1e-5)
    got = R.conv_fwd_ref(x.permute(0, 2, 3, 1), wt, scale, beta - mean * scale, act, stride, res.permute(0, 2, 3, 1))
    assert _rel(got, (y + res).permute(0, 2, 3, 1)) <= TOL
    # the stored layouts: nearest 2x upsampling, and ScalePredictionBlock's reshape + permute
    assert torch.equal(R.upsample2x(got), F.interpolate(got.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1))
    if cout % 3 == 0:
        nchw = got.permute(0, 3, 1, 2)
        ho, wo = nchw.shape[2:]
        assert torch.equal(R.head_layout(got, cout // 3), nchw.reshape(b, 3, cout // 3, ho, wo).permute(0, 1, 3, 4, 2))


@pytest.mark.parametrize("act", ["leaky_relu", "mish"])
@pytest.mark.parametrize("bn", [True, False])
def test_forward_reference_equals_oracle_block(bn, act):
    from oracle import net as onet
    g = torch.Generator().manual_seed(7 + bn)
    cin, cout, k, stride = 5, 6, 3, 2
    d = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    sd = {"b.conv.weight": d(cout, cin, k, k), "b.conv.bias": d(cout), "b.batch_norm.weight": d(cout).abs() + 0.5, "b.batch_norm.bias": d(cout),
          "b.batch_norm.running_mean": d(cout), "b.batch_norm.running_var": d(cout).abs() + 0.5}
    x = d(2, cin, 6, 8)
    want = onet.cnn_block(sd, dict(prefix="b", k=k, stride=stride, bn=bn), x, act)
    if bn:
        scale = sd["b.batch_norm.weight"] / torch.sqrt(sd["b.batch_norm.running_var"] + onet.BN_EPS)
        shift = sd["b.batch_norm.bias"] - sd["b.batch_norm.running_mean"] * scale
        a = R.ACT_LEAKY if act == "leaky_relu" else R.ACT_MISH
    else:                                                          # a bare convolution: scale = 1, shift = bias, no activation
        scale, shift, a = torch.ones(cout, dtype=torch.float64), sd["b.conv.bias"], R.ACT_NONE
    got = R.conv_fwd_ref(x.permute(0, 2, 3, 1), sd["b.conv.weight"], scale, shift, a, stride)
    assert _rel(got, want.permute(0, 2, 3, 1)) <= TOL


@pytest.mark.parametrize("shape", [(2, 3, 5, 4, 6), (1, 1, 1, 3, 2), (2, 4, 4, 5, 3)])
def test_input_gradient_reference_equals_autograd(shape):
    b, ho, wo, cin, cout = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn((b, cin, 2 * ho, 2 * wo), generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.randn((cout, cin, 3, 3), generator=g, dtype=torch.float64)
    dz = torch.randn((b, cout, ho, wo), generator=g, dtype=torch.float64)
    res = torch.randn((b, 2 * ho, 2 * wo, cin), generator=g, dtype=torch.float64)
    F.conv2d(x, wt, stride=2, padding=1).backward(dz)
    got = R.dgrad_s2_ref(dz.permute(0, 2, 3, 1), wt, res)
    assert _rel(got, x.grad.permute(0, 2, 3, 1) + res) <= TOL


def test_leaky_relu_as_the_kernels_round_it():
    """fmaxf(v, v * 0.1f): the fp64 statement with kernel_steps equals the fp32 evaluation, on integers and halves"""
    v = torch.arange(-40000, 40000, dtype=torch.float64) * 0.5
    got = R.act_ref(v, R.ACT_LEAKY, kernel_steps=True)
    want = torch.maximum(v.float(), v.float() * torch.tensor(0.1, dtype=torch.float32))
    assert torch.equal(got, want.double())
    assert float((got - R.act_ref(v, R.ACT_LEAKY)).abs().max()) <= 20000 * 2.0 ** -24      # and is LeakyReLU(0.1) to fp32 rounding


def test_case_tables_reach_what_they_name():
    """block counts 1, 7, 8, 9 of the 1x1 grid (pixel tiles of 128 x channel tiles of 64), every remainder of the two
    three-chunk unrolls, both BN of the gradient launches, every unaligned view really off 16 bytes"""
    blocks = {-(-c.B * c.H * c.W // 128) * -(-c.cout // 64) for c in R.INT_1X1}
    assert {1, 7, 8, 9} <= blocks
    assert {c.cin // 32 for c in R.INT_1X1} >= {1, 2, 3, 4, 5, 7}
    assert sorted(c.cout // 32 for c in R.INT_DGRAD[:5]) == [1, 2, 3, 4, 5]
    assert any(c.H > 52 for c in R.INT_DGRAD) and any(c.H <= 52 and c.cin > 64 for c in R.INT_DGRAD)
    assert all(c.cin not in (32, 64) and c.cout % 32 == 0 for c in R.INT_DGRAD)            # the per-class launches, not the fused GEMM
    for c in R.INT_UNALIGNED + R.INT_DGRAD[-2:]:
        assert R.n_out(c) % 8 == 0 and (c.y_ld % 8 or c.y_off % 8 or (c.res and (c.r_ld % 8 or c.r_off % 8))), c.name
    for c in R.INT_CASES + R.GAUSS_CASES:
        assert c.x_ld % 8 == 0 and c.x_off % 8 == 0 and c.y_off + R.n_out(c) <= c.y_ld and (not c.res or c.r_off + R.n_out(c) <= c.r_ld), c.name
        assert c.out != R.OUT_HEAD or (c.cout % 3 == 0 and not c.res)
    assert len({c.name for c in R.INT_CASES + R.GAUSS_CASES}) == len(R.INT_CASES + R.GAUSS_CASES)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.INT_CASES, ids=lambda c: c.name)
def test_integer_cases_are_exact_and_sharp(case, dtype):
    c, tdt = case, R.TDT[dtype]
    ops = R.operands(c, dtype)
    n = R.n_out(c)
    # operands as specified, and unchanged by the rounding to the 16-bit type
    x, w = ops["x"].float(), ops["w"]
    assert bool(((x.abs() >= 1) & (x.abs() <= 8) & (x == x.round())).all()) and bool((w.abs() <= 1).all()) and bool((w == w.round()).all())
    assert torch.equal(w.to(tdt).float(), w) and bool(torch.isin(ops["scale"], torch.tensor([1.0, 2.0, 0.5])).all())
    assert torch.equal(ops["shift"], ops["shift"].round())
    rmax = 0.0 if ops["r"] is None else float(ops["r"].float().abs().max())
    assert rmax <= 8
    # exactness
    bound = R.k_terms(c) * 8 * 2 + float(ops["shift"].abs().max()) + rmax
    assert bound < 2 ** 24
    v64 = R.value(c, ops, torch.float64, kernel_steps=True)
    v32 = R.value(c, ops, torch.float32, kernel_steps=True)
    assert float(v64.abs().max()) <= bound
    assert v32.dtype == torch.float32 and torch.equal(v32.double(), v64)
    assert torch.equal(v32.view(torch.int32), v64.float().view(torch.int32))
    if c.act == R.ACT_NONE:                                        # and with no rounding at all: the plain fp64 value
        assert torch.equal(R.value(c, ops, torch.float64), v64)
    assert v64.shape[-1] == n
    # sharpness
    if c.out == R.OUT_HEAD:
        share = 1.0                                                # fp32 output: v32 itself
    else:
        keep = torch.ones_like(v32, dtype=torch.bool)
        if c.act == R.ACT_LEAKY:                                   # the identity branch: scale * conv + shift >= 0
            keep = R.conv_fwd_ref(ops["x"][..., c.x_off:c.x_off + c.cin], w, ops["scale"], ops["shift"], R.ACT_NONE, c.stride) >= 0
        share = float((v32.to(tdt).float() == v32)[keep].float().mean())
    print("%s %s: bound %d, max |value| %g, stored without rounding %.3f" % (c.name, dtype, bound, float(v64.abs().max()), share))
    assert share >= (0.5 if dtype == "bf16" else 1.0)
    # a value of every sign and no constant output: a dropped term cannot cancel everywhere
    assert bool((v64 > 0).any()) and bool((v64 < 0).any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_sharpness_at_the_largest_k(dtype):
    """the share of exactly representable sums, for the integer operands of the cases, at K = 1440 and K = 2016"""
    g = torch.Generator().manual_seed(11)
    for k, least in ((1440, {"bf16": 0.5, "fp16": 1.0}), (2016, {"bf16": 0.5, "fp16": 1.0})):
        x = R._ints((4096, k), g)
        w = torch.randint(-1, 2, (k, 64), generator=g).float()
        v = x.double() @ w.double()
        share = float((v.float().to(R.TDT[dtype]).double() == v).float().mean())
        print("K = %d %s: %.3f" % (k, dtype, share))
        assert share >= least[dtype]
