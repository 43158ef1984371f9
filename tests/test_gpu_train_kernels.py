"""GPU tests (``-m gpu``) of the training kernels against fp64 restatements of the operations they replace
(tests/train_kernels_ref.py, tied to torch.autograd by tests/test_train_kernels_ref_host.py), each called through the C ABI
at the smallest shapes that reach every branch of its launch geometry:

  A  yolo_bn_stats          bn_stats_partial / bn_stats_finalize
  B  yolo_bn_act_fwd        bn_act_fwd_kernel (NHWC, residual slice, 2x-upsampled store, in-place gradient add, NaN flag)
  C  yolo_bn_act_bwd        bn_bwd_partial / bn_bwd_finalize / bn_bwd_apply, and the bare-conv bias gradient
  D  yolo_upsample2x_bwd
  E  yolo_conv_wgrad, fp32  six wgrad_f32_kernel instantiations, the K-slice split, wgrad_reduce<1|4|16>
  F  yolo_conv_dgrad_s2, fp32
  G  the fp32 1x1 input gradient (yolo_pack_weights_dgrad(flip = 1, ksize = 1) + the forward kernels)

Every output buffer is pre-filled with a sentinel; channels outside [off, off + c) and the bytes past the stated workspace
size must come back unchanged. All data is seeded from the case tuple. The large cases (block caps of the reductions and of
the apply passes) are generated and referenced on the device, a few thousand pixels at a time. Every measured maximum is
printed (run with -s). The `LONG` variants of the two reduction kernels need > 268 M vectors in one tensor and are not reached.
"""
import zlib

import numpy as np
import pytest
import torch

from tests import train_kernels_ref as R

pytestmark = pytest.mark.gpu

SENT = -12288.0                       # exact in fp32, fp16 and bf16
GUARD = 256                           # bytes behind every workspace that must stay 0xA5
CHUNK = 1 << 16                       # pixels promoted to fp64 at a time
EPS = float(np.float32(1e-5))         # as the kernels receive them (C float arguments)
DTYPES = ["fp32", "bf16", "fp16"]
ACTS = {"none": R.ACT_NONE, "leaky": R.ACT_LEAKY, "mish": R.ACT_MISH}
YOLO_OK, YOLO_ERR_WORKSPACE = 0, -4


@pytest.fixture(scope="module")
def L():
    from yolo_for_turbines_amd import _lib
    _lib.lib()                        # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


@pytest.fixture(scope="module")
def eps_mish():
    """4x the relative error of a plain fp32 evaluation of the kernels' Mish formula (re-measured, see the host test): the
    factor covers the hardware exp and reciprocal (about 1 ulp each, plus |v| 2^-24 from the exponent scaling)."""
    return 4.0 * R.mish_fp32_formula_rel_error()


def _dt(L, dtype):
    return {"fp32": (L.F32, torch.float32, 4), "bf16": (L.BF16, torch.bfloat16, 8), "fp16": (L.F16, torch.float16, 8)}[dtype]


def _gen(*case):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(case).encode()))


def _sync():
    torch.cuda.synchronize()


def _ceil(a, b):
    return (a + b - 1) // b


def _geom(m, c, vn, run, cap):
    """(blocks, pixels per block, pixel lanes, pixels per thread and block) of red_blocks (16, 4096) / ap_blocks (8, 8192)."""
    cv = c // vn
    lanes = 256 // min(cv, 256)
    ppb = run * lanes
    nblk = max(1, min(_ceil(m, ppb), cap))
    ppb = _ceil(m, nblk)
    return _ceil(m, ppb), ppb, lanes, _ceil(ppb, lanes)


def _red(m, c, vn):
    return _geom(m, c, vn, 16, 4096)


def _chunks(m):
    return [(a, min(m, a + CHUNK)) for a in range(0, m, CHUNK)]


def _slice_buf(m, c, ld, off, tdt):
    """(m, ld) buffer of sentinels and its [off, off + c) channel view."""
    buf = torch.full((m, ld), SENT, dtype=tdt, device="cuda")
    return buf, buf[:, off:off + c]


def _fill_normal(view, g, mu=None, sigma=None):
    for a, b in _chunks(view.shape[0]):
        x = torch.randn((b - a, view.shape[1]), generator=g, device="cuda")
        if sigma is not None:
            x = x * sigma + mu
        view[a:b] = x.to(view.dtype)


def _fill_ints(view, g):
    """integers in +-{1..8}: exact in all three dtypes, and so are fp32 sums of a few thousand of them"""
    for a, b in _chunks(view.shape[0]):
        v = torch.randint(-8, 8, (b - a, view.shape[1]), generator=g, device="cuda", dtype=torch.int8)
        view[a:b] = torch.where(v >= 0, v + 1, v).to(view.dtype)


def _outside_untouched(buf, off, c):
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    keep[off:off + c] = False
    return bool((buf[..., keep] == SENT).all())


def _vec(c, fill=SENT, pad=8):
    return torch.full((c + pad,), fill, dtype=torch.float32, device="cuda")


def _ws(need):
    return torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")


def _guard_ok(ws, need):
    return bool((ws[need:] == 0xA5).all())


def _ulps(got, want64):
    """error of fp32 values in units in the last place of the fp64 reference"""
    return float(((got.double() - want64).abs() / R.ulp_of(want64, torch.float32)).max())


def _uniform(c, lo, hi, g):
    return torch.rand(c, generator=g, device="cuda") * (hi - lo) + lo


# =============================================================================================== A. yolo_bn_stats
def _stats_cases(vn):
    return [(1, vn, vn, 0), (255, vn, vn, 0), (257, vn, vn, 0),             # cv = 1: 256 lanes, fewer pixels than lanes, runs of 1-2
            (4097, vn, vn, 0),                                              # two blocks of 2049 pixels: main loop of 8 plus tail
            (161, 24 * vn, 24 * vn, 0), (1000, 24 * vn, 24 * vn, 0),        # vc = 24: 10 lanes, 16 idle threads; 2 and 7 blocks
            (105, 25 * vn, 25 * vn, 0),                                     # vc = 25: 6 idle threads, one block
            (98, 256 * vn, 256 * vn, 0), (17, 256 * vn, 256 * vn, 0),       # lanes = 1
            (33, 257 * vn, 257 * vn, 0),                                    # two passes, the second with one live vector channel
            (338, 128, 384, 256), (338, 256, 768, 0)]                       # a slice of a concat buffer


# block cap of the reductions: 4091 / 4095 blocks of 264 / 517 pixels (no multiples of the 16 / 32 lanes), thread runs of 17
BIG = {"fp32": (3 * 600 * 600, 64, 64, 0), "bf16": (3 * 840 * 840, 64, 64, 0)}
NHW = {1: (1, 1, 1), 255: (1, 15, 17), 257: (1, 1, 257), 4097: (1, 17, 241), 161: (1, 7, 23), 1000: (2, 20, 25), 105: (3, 5, 7),
       98: (2, 7, 7), 17: (1, 17, 1), 33: (1, 3, 11), 338: (2, 13, 13), 3 * 600 * 600: (3, 600, 600), 3 * 840 * 840: (3, 840, 840)}
SHAPE_PARAMS = [(dt, case) for dt, vn in (("fp32", 4), ("bf16", 8), ("fp16", 8)) for case in _stats_cases(vn)]
SHAPE_PARAMS += [(dt, case) for dt, case in BIG.items()]
SHAPE_IDS = ["%s-m%d-c%d-ld%d-off%d" % ((dt,) + case) for dt, case in SHAPE_PARAMS]


def test_geometry_of_the_cases_is_what_the_tables_say():
    """the launch geometry the case tables rely on, from a restatement of red_blocks / ap_blocks"""
    assert _red(3 * 600 * 600, 64, 4) == (4091, 264, 16, 17) and _red(3 * 840 * 840, 64, 8) == (4095, 517, 32, 17)
    assert _geom(3 * 600 * 600, 64, 4, 8, 8192)[:2] == (8182, 132) and _geom(3 * 840 * 840, 64, 8, 8, 8192)[:2] == (8173, 259)
    assert _red(4097, 4, 4)[:2] == (2, 2049) and _red(161, 96, 4)[:3] == (2, 81, 10) and _red(1000, 96, 4)[0] == 7
    assert _red(105, 100, 4)[:3] == (1, 105, 10) and _red(98, 1024, 4)[2] == 1 and _red(33, 1028, 4)[2] == 1


def _call_stats(L, code, zbuf, m, c, ld, off, gamma, beta, mom, rm, rv):
    lib = L.lib()
    out = [_vec(c) for _ in range(4)]
    need = lib.yolo_bn_workspace_bytes(m, c)
    ws = _ws(need)
    rc = lib.yolo_bn_stats(zbuf.data_ptr(), m, c, ld, off, gamma.data_ptr(), beta.data_ptr(), mom, EPS, L.ptr(rm), L.ptr(rv),
                           *[t.data_ptr() for t in out], code, ws.data_ptr(), need, L.current_stream())
    L.check(rc, "yolo_bn_stats")
    _sync()
    assert _guard_ok(ws, need), "bn_stats wrote past its stated workspace"
    assert all(bool((t[c:] == SENT).all()) for t in out), "bn_stats wrote past channel c"
    return [t[:c] for t in out]


# measured on an MI355X (largest over all cases and dtypes), against the bounds asserted below:
#   exact:  mean bitwise; invstd 1.93 ulp, scale 2.22 ulp, running mean 1.61 ulp, running var 1.76 ulp     (bound: 4 ulp)
#   random: mean error / bound 0.29; invstd relative error / bound 0.21; at the block cap (r = 17) 0.02 and 0.05
@pytest.mark.parametrize("dtype,case", SHAPE_PARAMS, ids=SHAPE_IDS)
def test_bn_stats_exact_on_integers(L, dtype, case):
    """z in +-{1..8}: every fp32 run and every fp64 sum of the kernel is exact, so a dropped, repeated or misassigned pixel
    or channel changes an integer sum. mean must be the correctly rounded quotient; invstd, scale and the running statistics
    see one sqrtf, one divide and a (possibly contracted) multiply-add: within 4 ulp of fp64. Momentum 0.1."""
    m, c, ld, off = case
    code, tdt, vn = _dt(L, dtype)
    g = _gen("stats-int", dtype, case)
    zbuf, z = _slice_buf(m, c, ld, off, tdt)
    _fill_ints(z, g)
    S = sum(z[a:b].to(torch.int64).sum(0) for a, b in _chunks(m))
    Q = sum((z[a:b].to(torch.int64) ** 2).sum(0) for a, b in _chunks(m))
    mom = float(np.float32(0.1))
    gamma, beta = _uniform(c, 0.5, 1.5, g), _uniform(c, -1.0, 1.0, g)
    # running mean with the sign of the batch mean: the update then adds two terms of one sign, and "4 ulp of the result" is
    # a statement about the roundings, not about cancellation
    rm0 = _uniform(c, 0.5, 1.5, g) * torch.where(S < 0, -1.0, 1.0).float()
    rv0 = _uniform(c, 0.5, 1.5, g)
    rm, rv = rm0.clone(), rv0.clone()
    mean, invstd, scale, shift = _call_stats(L, code, zbuf, m, c, ld, off, gamma, beta, mom, rm, rv)
    mean64 = S.double() / m
    var64 = (Q * m - S * S).double() / (float(m) * m)                       # exact integers up to the one division
    invstd64 = 1.0 / torch.sqrt(var64 + EPS)
    unb64 = var64 * m / (m - 1) if m > 1 else var64
    assert torch.equal(mean, mean64.float()), "mean is not the correctly rounded integer quotient"
    assert torch.equal(shift, beta)
    u = {"invstd": _ulps(invstd, invstd64), "scale": _ulps(scale, gamma.double() * invstd64),
         "running_mean": _ulps(rm, (1.0 - mom) * rm0.double() + mom * mean64),
         "running_var": _ulps(rv, (1.0 - mom) * rv0.double() + mom * unb64)}
    print(f"bn_stats exact {dtype} {case}: ulps {u}")
    assert max(u.values()) <= 4.0, u


@pytest.mark.parametrize("dtype,case", SHAPE_PARAMS, ids=SHAPE_IDS)
def test_bn_stats_random_vs_fp64(L, dtype, case):
    """z = mu_c + sigma_c N(0, 1), |mu_c| <= 8 sigma_c, rounded to the dtype. With r the pixels a thread adds in fp32 before
    the fp64 tree: |mean - ref| <= (r + 1) 2^-24 max|z|, and the relative error of invstd <= (r + 2) 2^-24 (mu^2 + sigma^2) /
    (sigma^2 + eps) + 2^-22 (the sum of squares carries the run's roundings; sqrt, divide and the fp32 casts the rest).
    Momentum 0.03; the running statistics follow from mean and variance with the same bounds."""
    m, c, ld, off = case
    code, tdt, vn = _dt(L, dtype)
    r = _red(m, c, vn)[3]
    g = _gen("stats-rand", dtype, case)
    sigma = _uniform(c, 0.5, 2.0, g)
    mu = sigma * _uniform(c, -8.0, 8.0, g)
    zbuf, z = _slice_buf(m, c, ld, off, tdt)
    _fill_normal(z, g, mu, sigma)
    mom = float(np.float32(0.03))
    gamma, beta = _uniform(c, 0.5, 1.5, g), _uniform(c, -1.0, 1.0, g)
    rm0, rv0 = _uniform(c, -1.0, 1.0, g), _uniform(c, 0.5, 1.5, g)
    rm, rv = rm0.clone(), rv0.clone()
    mean, invstd, scale, shift = _call_stats(L, code, zbuf, m, c, ld, off, gamma, beta, mom, rm, rv)
    w_mean, w_invstd, w_scale, w_shift, w_rm, w_rv = R.bn_stats_ref(z, gamma, beta, EPS, mom, rm0, rv0, chunk_rows=CHUNK)
    zmax = torch.stack([z[a:b].abs().amax(0) for a, b in _chunks(m)]).amax(0).double()
    var64 = 1.0 / w_invstd ** 2 - EPS
    b_mean = (r + 1) * 2.0 ** -24 * zmax
    b_inv = (r + 2) * 2.0 ** -24 * (w_mean ** 2 + var64) / (var64 + EPS) + 2.0 ** -22
    e_mean = (mean.double() - w_mean).abs()
    e_inv = (invstd.double() - w_invstd).abs() / w_invstd
    print(f"bn_stats random {dtype} {case}: r {r}; mean err/bound {float((e_mean / b_mean).max()):.3f}; "
          f"invstd rel err {float(e_inv.max()):.3e}, err/bound {float((e_inv / b_inv).max()):.3f}")
    assert bool((e_mean <= b_mean).all()) and bool((e_inv <= b_inv).all())
    assert torch.equal(shift, beta)
    assert bool(((scale.double() - w_scale).abs() <= (b_inv + 2.0 ** -23) * w_scale.abs()).all())
    # running statistics: the errors of mean / variance scaled by the momentum, plus the update's own three roundings
    assert bool(((rm.double() - w_rm).abs() <= mom * b_mean + 3 * 2.0 ** -24 * ((1 - mom) * rm0.abs() + mom * w_mean.abs())).all())
    assert bool(((rv.double() - w_rv).abs() <= (2 * b_inv + 3 * 2.0 ** -24) * w_rv).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_stats_constant_channel_and_no_running_statistics(L, dtype):
    """Channels that hold one value (exactly summable: a few mantissa bits): the variance is 0, never negative, and invstd is
    1 / sqrt(eps) to 2 ulp. running_mean = running_var = NULL: accepted, the four outputs are the same."""
    code, tdt, vn = _dt(L, dtype)
    m, c = 161, 24 * vn
    g = _gen("stats-const", dtype)
    zbuf, z = _slice_buf(m, c, c, 0, tdt)
    _fill_normal(z, g)
    consts = {0: 2.75, 5: -0.625, c - 1: 7.0}
    for ch, v in consts.items():
        z[:, ch] = v
    gamma, beta = _uniform(c, 0.5, 1.5, g), _uniform(c, -1.0, 1.0, g)
    rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    a = _call_stats(L, code, zbuf, m, c, c, 0, gamma, beta, 0.1, rm, rv)
    b = _call_stats(L, code, zbuf, m, c, c, 0, gamma, beta, 0.1, None, None)
    for ch, v in consts.items():
        assert float(a[0][ch]) == v
        assert _ulps(a[1][ch:ch + 1], torch.tensor([EPS ** -0.5], dtype=torch.float64, device="cuda")) <= 2.0
        assert float(rv[ch]) == float(np.float32(1.0 - np.float32(0.1)))            # 0.9 * 1 + 0.1 * 0
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# =============================================================================================== B. yolo_bn_act_fwd
def _fwd_params(c, g):
    """arbitrary per-channel fp32 vectors (they need not be anyone's statistics); scales of both signs"""
    mean = torch.randn(c, generator=g, device="cuda")
    scale = _uniform(c, 0.25, 3.0, g) * torch.where(_uniform(c, 0, 1, g) < 0.25, -1.0, 1.0)
    shift = torch.randn(c, generator=g, device="cuda")
    return mean, scale, shift


def _fwd_tol(zc, rc, ref, stored, mean, scale, shift, act, tdt, eps_mish):
    zz = zc.double()
    zz = zz - mean.double() if mean is not None else zz
    du = 2.0 ** -22 * (zz.abs() * scale.double().abs() + shift.double().abs())
    tol = (eps_mish * ref.abs() + 1.1 * du) if act == R.ACT_MISH else du
    if rc is not None:
        tol = tol + 2.0 ** -24 * rc.double().abs()
    if tdt != torch.float32:
        tol = tol + 0.5 * R.ulp_of(stored.double(), tdt)
    return tol


def _check_fwd(zv, rv, yv, mean, scale, shift, act, tdt, eps_mish):
    """largest error / tolerance of y (m, c) against the fp64 reference, a chunk of pixels at a time"""
    worst = 0.0
    for a, b in _chunks(zv.shape[0]):
        rc = rv[a:b] if rv is not None else None
        ref = R.bn_act_fwd_ref(zv[a:b], mean, scale, shift, act, rc)
        tol = _fwd_tol(zv[a:b], rc, ref, yv[a:b], mean, scale, shift, act, tdt, eps_mish)
        worst = max(worst, float(((yv[a:b].double() - ref).abs() / tol.clamp_min(1e-300)).max()))
    return worst


def _call_fwd(L, code, zbuf, z_ld, z_off, mean, scale, shift, rbuf, r_ld, r_off, ybuf, y_ld, y_off, n, h, w, c, act, out_mode, flag=None):
    rc = L.lib().yolo_bn_act_fwd(zbuf.data_ptr(), z_ld, z_off, L.ptr(mean), scale.data_ptr(), shift.data_ptr(), L.ptr(rbuf), r_ld, r_off,
                                 ybuf.data_ptr(), y_ld, y_off, n, h, w, c, act, out_mode, code, L.ptr(flag), L.current_stream())
    L.check(rc, "yolo_bn_act_fwd")
    _sync()


# measured on an MI355X, largest error / tolerance over all cases:
#   fp32:   none 0.86, leaky 0.80, mish 0.50 (block-cap case 0.48, 0.48, 0.20); upsampled store 0.66; in-place add 0.93
#   16-bit: 0.997 .. 1.000 everywhere: the half ulp of the stored value is the whole error
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("dtype,case", SHAPE_PARAMS, ids=SHAPE_IDS)
def test_bn_act_fwd_vs_fp64(L, eps_mish, dtype, case, act):
    """y = act((z - mean) scale + shift) [+ residual] on the shapes of A as (n, h, w): plain NHWC into a channel slice, then
    (small cases) with the residual read from a slice of another buffer (r_ld != z_ld, r_off != 0). Per element, with
    du = 2^-22 (|z - mean| |scale| + |shift|) (three fp32 roundings of u): none / leaky du + 2^-24 |residual|;
    mish eps_m |y| + 1.1 du + 2^-24 |residual| (1.1 > max mish'); 16-bit outputs add half an ulp of the stored value."""
    m, c, z_ld, z_off = case
    n, h, w = NHW[m]
    code, tdt, vn = _dt(L, dtype)
    big = m > 100000
    g = _gen("fwd", dtype, case, act)
    mean, scale, shift = _fwd_params(c, g)
    zbuf, z = _slice_buf(m, c, z_ld, z_off, tdt)
    _fill_normal(z, g, mean, 2.0)
    y_ld, y_off = (c, 0) if big else (c + 2 * vn, vn)
    ybuf, y = _slice_buf(m, c, y_ld, y_off, tdt)
    _call_fwd(L, code, zbuf, z_ld, z_off, mean, scale, shift, None, 0, 0, ybuf, y_ld, y_off, n, h, w, c, ACTS[act], L.OUT_NHWC)
    worst = _check_fwd(z, None, y, mean, scale, shift, ACTS[act], tdt, eps_mish)
    assert _outside_untouched(ybuf, y_off, c)
    print(f"bn_act_fwd {dtype} {act} {case}: plain err/tol {worst:.3f}", end="")
    assert worst <= 1.0
    if big:
        print()
        return
    r_ld, r_off = z_ld + 3 * vn, 2 * vn
    rbuf, r = _slice_buf(m, c, r_ld, r_off, tdt)
    _fill_normal(r, g)
    ybuf.fill_(SENT)
    _call_fwd(L, code, zbuf, z_ld, z_off, mean, scale, shift, rbuf, r_ld, r_off, ybuf, y_ld, y_off, n, h, w, c, ACTS[act], L.OUT_NHWC)
    worst = _check_fwd(z, r, y, mean, scale, shift, ACTS[act], tdt, eps_mish)
    print(f"; residual slice err/tol {worst:.3f}")
    assert _outside_untouched(ybuf, y_off, c) and _outside_untouched(rbuf, r_off, c)
    assert worst <= 1.0


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_act_fwd_upsampled_store(L, eps_mish, dtype, act):
    """YOLO_OUT_UPSAMPLE2X into a slice of a wider buffer (n = 3, Ho = 5, Wo = 7): the four copies of every pixel are equal
    and right, the other channels untouched."""
    code, tdt, vn = _dt(L, dtype)
    n, h, w, c = 3, 5, 7, 24 * vn
    m = n * h * w
    g = _gen("fwd-up", dtype, act)
    mean, scale, shift = _fwd_params(c, g)
    zbuf, z = _slice_buf(m, c, c, 0, tdt)
    _fill_normal(z, g, mean, 2.0)
    rbuf, r = _slice_buf(m, c, c + vn, vn, tdt)
    _fill_normal(r, g)
    y_ld, y_off = 2 * c + 2 * vn, c
    ybuf = torch.full((n, 2 * h, 2 * w, y_ld), SENT, dtype=tdt, device="cuda")
    _call_fwd(L, code, zbuf, c, 0, mean, scale, shift, rbuf, c + vn, vn, ybuf, y_ld, y_off, n, h, w, c, ACTS[act], L.OUT_UPSAMPLE2X)
    assert _outside_untouched(ybuf, y_off, c)
    y = ybuf[..., y_off:y_off + c]
    copies = [y[:, i::2, j::2].reshape(m, c) for i in (0, 1) for j in (0, 1)]
    assert all(torch.equal(copies[0], k) for k in copies[1:]), "the four copies of a pixel differ"
    worst = _check_fwd(z, r, copies[0], mean, scale, shift, ACTS[act], tdt, eps_mish)
    print(f"bn_act_fwd upsample {dtype} {act}: err/tol {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_act_fwd_in_place_gradient_add(L, eps_mish, dtype):
    """The skip-connection gradient add exactly as `_Grads.add_alias` issues it: mean = NULL, scale of ones, shift of zeros,
    y == residual (the accumulated gradient), z a slice of another buffer: own += z."""
    code, tdt, vn = _dt(L, dtype)
    n, h, w, c = 2, 13, 13, 128
    m = n * h * w
    g = _gen("fwd-add", dtype)
    zbuf, z = _slice_buf(m, c, 384, 256, tdt)
    _fill_normal(z, g)
    obuf, own = _slice_buf(m, c, 256, 128, tdt)
    _fill_normal(own, g)
    own0 = own.clone()
    ones, zeros = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
    _call_fwd(L, code, zbuf, 384, 256, None, ones, zeros, obuf, 256, 128, obuf, 256, 128, n, h, w, c, L.ACT_NONE, L.OUT_NHWC)
    worst = _check_fwd(z, own0, own, None, ones, zeros, R.ACT_NONE, tdt, eps_mish)
    print(f"bn_act_fwd in-place add {dtype}: err/tol {worst:.3f}")
    assert _outside_untouched(obuf, 128, c) and worst <= 1.0
    assert torch.equal(own, (z.float() + own0.float()).to(tdt))                 # one correctly rounded addition


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_act_fwd_nan_flag(L, dtype):
    """One NaN in the last pixel of the last block sets bit 2 of the flag and leaves the other bits; without a NaN the flag
    is unchanged; a NULL flag is accepted."""
    code, tdt, vn = _dt(L, dtype)
    n, h, w = NHW[1000]
    m, c = 1000, 24 * vn
    assert _geom(m, c, vn, 8, 8192)[0] == 13
    g = _gen("fwd-nan", dtype)
    mean, scale, shift = _fwd_params(c, g)
    zbuf, z = _slice_buf(m, c, c, 0, tdt)
    _fill_normal(z, g)
    ybuf, y = _slice_buf(m, c, c, 0, tdt)
    flag = torch.tensor([5, 1234567], dtype=torch.int32, device="cuda")
    _call_fwd(L, code, zbuf, c, 0, mean, scale, shift, None, 0, 0, ybuf, c, 0, n, h, w, c, L.ACT_LEAKY, L.OUT_NHWC, flag)
    assert flag.tolist() == [5, 1234567]
    z[m - 1, c - 1] = float("nan")
    _call_fwd(L, code, zbuf, c, 0, mean, scale, shift, None, 0, 0, ybuf, c, 0, n, h, w, c, L.ACT_LEAKY, L.OUT_NHWC, flag)
    assert flag.tolist() == [7, 1234567]
    assert bool(torch.isnan(y[m - 1, c - 1])) and int(torch.isnan(y).sum()) == 1
    _call_fwd(L, code, zbuf, c, 0, mean, scale, shift, None, 0, 0, ybuf, c, 0, n, h, w, c, L.ACT_LEAKY, L.OUT_NHWC, None)


# =============================================================================================== C. yolo_bn_act_bwd
def _call_bwd(L, code, dybuf, dy_ld, dy_off, zbuf, z_ld, z_off, gamma, mean, invstd, scale, shift, m, c, act, dzbuf, dz_ld, dz_off):
    lib = L.lib()
    dgamma, dbeta = _vec(c), _vec(c)
    need = lib.yolo_bn_workspace_bytes(m, c)
    ws = _ws(need)
    rc = lib.yolo_bn_act_bwd(dybuf.data_ptr(), dy_ld, dy_off, L.ptr(zbuf), z_ld, z_off, L.ptr(gamma), L.ptr(mean), L.ptr(invstd), L.ptr(scale),
                             L.ptr(shift), m, c, act, dgamma.data_ptr() if gamma is not None else 0, dbeta.data_ptr(), L.ptr(dzbuf), dz_ld,
                             dz_off, code, ws.data_ptr(), need, L.current_stream())
    assert rc == YOLO_OK, L.lib().yolo_last_error()
    _sync()
    assert _guard_ok(ws, need), "bn_act_bwd wrote past its stated workspace"
    assert bool((dgamma[c:] == SENT).all()) and bool((dbeta[c:] == SENT).all())
    return dgamma[:c], dbeta[:c]


def _bwd_params(c, g):
    gamma, invstd = _uniform(c, 0.5, 1.5, g), _uniform(c, 0.5, 2.0, g)
    mean, shift = _uniform(c, -1.0, 1.0, g), _uniform(c, -0.5, 0.5, g)
    return gamma, mean, invstd, gamma * invstd, shift               # scale = fl(gamma invstd) in [0.25, 3]


# measured on an MI355X, largest error / tolerance over all cases:
#   fp32:   leaky dbeta 0.04, dgamma 0.05, dz 0.04;  mish dbeta 0.09, dgamma 0.09, dz 0.11
#   16-bit: leaky dbeta 0.06, dgamma 0.05;  mish dbeta 0.29, dgamma 0.33 (m = 1; 0.06 / 0.09 otherwise);  dz 0.99 .. 0.999 (the
#           half ulp of the stored value)
#   min |u| of the reference: 0.1250 fp32, 0.1243 fp16, 0.1176 bf16
@pytest.mark.parametrize("act", ["leaky", "mish"])
@pytest.mark.parametrize("dtype,case", SHAPE_PARAMS, ids=SHAPE_IDS)
def test_bn_act_bwd_vs_fp64(L, dtype, case, act):
    """dgamma, dbeta, dz on the shapes of A, dy and dz in channel slices of wider buffers. The inputs keep off the leaky kink,
    so that no rounding-induced sign flip of u decides anything and no element is excluded: u_t = sign(n) (0.125 + |n|),
    z = mean + (u_t - shift) / scale rounded to the dtype, and min |u| >= 0.1 is asserted on the reference alone.
    With r the fp32 run of a thread: dbeta within (r + 2) 2^-24 sum|du| + 2^-19 sum|du|, dgamma the same with |du zhat|,
    dz within 2^-18 |gamma invstd| (|du| + mean|du| + |zhat| mean|du zhat|) (+ half an ulp in 16 bits): about ten roundings,
    the reduction error and the approximations of the Mish derivative; a wrong coefficient is off by 1e4 times as much."""
    m, c, z_ld, z_off = case
    code, tdt, vn = _dt(L, dtype)
    r = _red(m, c, vn)[3]
    big = m > 100000
    g = _gen("bwd", dtype, case, act)
    gamma, mean, invstd, scale, shift = _bwd_params(c, g)
    zbuf, z = _slice_buf(m, c, z_ld, z_off, tdt)
    for a, b in _chunks(m):
        nrm = torch.randn((b - a, c), generator=g, device="cuda").double()
        ut = torch.where(nrm < 0, -1.0, 1.0) * (0.125 + nrm.abs())          # (torch.sign(0) is 0, and 1e8 draws do hit 0)
        z[a:b] = (mean.double() + (ut - shift.double()) / scale.double()).to(tdt)
    dy_ld, dy_off, dz_ld, dz_off = (c, 0, c, 0) if big else (c + 2 * vn, vn, c + vn, vn)
    dybuf, dy = _slice_buf(m, c, dy_ld, dy_off, tdt)
    _fill_normal(dy, g)
    dzbuf, dz = _slice_buf(m, c, dz_ld, dz_off, tdt)
    dgamma, dbeta = _call_bwd(L, code, dybuf, dy_ld, dy_off, zbuf, z_ld, z_off, gamma, mean, invstd, scale, shift, m, c, ACTS[act],
                              dzbuf, dz_ld, dz_off)
    assert _outside_untouched(dzbuf, dz_off, c) and _outside_untouched(dybuf, dy_off, c)
    # pass 1: the sums and the scales of their bounds
    w_db = w_dg = a_du = a_dq = 0.0
    umin = float("inf")
    for a, b in _chunks(m):
        _, _, _, u, du, zhat = R.bn_act_bwd_ref(dy[a:b], z[a:b], gamma, mean, invstd, scale, shift, ACTS[act])
        w_db, w_dg = w_db + du.sum(0), w_dg + (du * zhat).sum(0)
        a_du, a_dq = a_du + du.abs().sum(0), a_dq + (du * zhat).abs().sum(0)
        umin = min(umin, float(u.abs().min()))
    assert umin >= 0.1, umin
    k = (r + 2) * 2.0 ** -24 + 2.0 ** -19
    e_db, e_dg = (dbeta.double() - w_db).abs() / (k * a_du), (dgamma.double() - w_dg).abs() / (k * a_dq)
    # pass 2: dz with the reference's own sums
    worst = 0.0
    k0 = (gamma.double() * invstd.double()).abs()
    for a, b in _chunks(m):
        _, _, w_dz, u, du, zhat = R.bn_act_bwd_ref(dy[a:b], z[a:b], gamma, mean, invstd, scale, shift, ACTS[act], totals=(w_dg, w_db, m))
        tol = 2.0 ** -18 * k0 * (du.abs() + a_du / m + zhat.abs() * (a_dq / m))
        if tdt != torch.float32:
            tol = tol + 0.5 * R.ulp_of(dz[a:b].double(), tdt)
        worst = max(worst, float(((dz[a:b].double() - w_dz).abs() / tol.clamp_min(1e-300)).max()))
    print(f"bn_act_bwd {dtype} {act} {case}: r {r}, min|u| {umin:.4f}; err/tol dbeta {float(e_db.max()):.3f} "
          f"dgamma {float(e_dg.max()):.3f} dz {worst:.3f}")
    assert float(e_db.max()) <= 1.0 and float(e_dg.max()) <= 1.0 and worst <= 1.0


@pytest.mark.parametrize("dtype,case", SHAPE_PARAMS, ids=SHAPE_IDS)
def test_bn_act_bwd_exact_sum_on_integers(L, dtype, case):
    """No activation and integer dy: du = dy, every fp32 run and the fp64 tree are exact, dbeta is the integer sum."""
    m, c, z_ld, z_off = case
    code, tdt, vn = _dt(L, dtype)
    g = _gen("bwd-int", dtype, case)
    gamma, mean, invstd, scale, shift = _bwd_params(c, g)
    dybuf, dy = _slice_buf(m, c, z_ld, z_off, tdt)
    _fill_ints(dy, g)
    dzbuf, dz = _slice_buf(m, c, c, 0, tdt)
    # z = dy (same buffer): only dgamma and dz depend on it
    dgamma, dbeta = _call_bwd(L, code, dybuf, z_ld, z_off, dybuf, z_ld, z_off, gamma, mean, invstd, scale, shift, m, c, L.ACT_NONE,
                              dzbuf, c, 0)
    S = sum(dy[a:b].to(torch.int64).sum(0) for a, b in _chunks(m))
    assert torch.equal(dbeta, S.double().float())
    assert not bool(torch.isnan(dz.float()).any()) and not bool((dz == SENT).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 7, 7, 255, 256), (3, 10, 10, 21, 32)])
def test_bias_gradient_of_the_heads(L, dtype, shape):
    """The bare-conv mode exactly as the detection heads call it: gamma = NULL and every other pointer 0; c is the padded
    channel count, the padding channels hold zeros. dbias is exact on integers; nothing is written through the null pointers."""
    n, h, w, cout, c = shape
    m = n * h * w
    code, tdt, vn = _dt(L, dtype)
    g = _gen("dbias", dtype, shape)
    dybuf, dy = _slice_buf(m, c, c, 0, tdt)
    _fill_ints(dy, g)
    dy[:, cout:] = 0
    _, db = _call_bwd(L, code, dybuf, c, 0, None, 0, 0, None, None, None, None, None, m, c, L.ACT_NONE, None, 0, 0)
    assert torch.equal(db.double(), R.bias_grad_ref(dy)) and bool((db[cout:] == 0).all())
    dy2buf, dy2 = _slice_buf(m, c, c, 0, tdt)
    _fill_normal(dy2, g)
    _, db = _call_bwd(L, code, dy2buf, c, 0, None, 0, 0, None, None, None, None, None, m, c, L.ACT_NONE, None, 0, 0)
    r = _red(m, c, vn)[3]
    assert bool(((db.double() - R.bias_grad_ref(dy2)).abs() <= (r + 2) * 2.0 ** -24 * dy2.double().abs().sum(0)).all())


# =============================================================================================== D. yolo_upsample2x_bwd
def _up_cases(vn):
    return [(1, 1, 1, vn, 2 * vn, vn, 2 * vn, 0), (3, 5, 7, 24 * vn, 24 * vn, 0, 24 * vn, 0),
            (2, 13, 13, 128, 384, 256, 256, 128)]                       # (n, h, w, c, d_ld, d_off, x_ld, x_off)


UP_PARAMS = [(dt, case) for dt, vn in (("fp32", 4), ("bf16", 8), ("fp16", 8)) for case in _up_cases(vn)]
UP_PARAMS.append(("fp32", (3, 128, 128, 256, 256, 0, 256, 0)))          # 3.1 M vectors: above the 8192-block grid, 200 MB


# measured on an MI355X: random data, largest error / bound 0.65 (fp32), 1.00 (16-bit: the half ulp of the result)
@pytest.mark.parametrize("dtype,case", UP_PARAMS, ids=["%s-%s" % (dt, "x".join(map(str, c))) for dt, c in UP_PARAMS])
def test_upsample2x_bwd(L, dtype, case):
    """dx[n, h, w] = the sum of the 2x2 pixels of dup it was copied to: exact on integers; on random data three additions,
    |err| <= 3 2^-24 sum|4 terms| (+ half an ulp of the 16-bit result). dup and dx are slices of wider buffers."""
    n, h, w, c, d_ld, d_off, x_ld, x_off = case
    code, tdt, vn = _dt(L, dtype)
    g = _gen("up", dtype, case)
    for kind in ("ints", "random"):
        dbuf, dup = _slice_buf(n * 2 * h * 2 * w, c, d_ld, d_off, tdt)
        (_fill_ints if kind == "ints" else _fill_normal)(dup, g)
        xbuf, dx = _slice_buf(n * h * w, c, x_ld, x_off, tdt)
        L.check(L.lib().yolo_upsample2x_bwd(dbuf.data_ptr(), d_ld, d_off, xbuf.data_ptr(), x_ld, x_off, n, h, w, c, code, L.current_stream()),
                "yolo_upsample2x_bwd")
        _sync()
        assert _outside_untouched(xbuf, x_off, c)
        worst, per = 0.0, max(1, CHUNK // (4 * h * w))                   # images per chunk
        for a in range(0, n, per):
            d4 = dup.reshape(n, 2 * h, 2 * w, c)[a:a + per]
            got, ref = dx.reshape(n, h, w, c)[a:a + per].double(), R.upsample2x_bwd_ref(d4)
            if kind == "ints":
                assert torch.equal(got, ref)
                continue
            tol = 3 * 2.0 ** -24 * R.upsample2x_bwd_abs_ref(d4)
            if tdt != torch.float32:
                tol = tol + 0.5 * R.ulp_of(got, tdt)
            worst = max(worst, float(((got - ref).abs() / tol.clamp_min(1e-300)).max()))
        if kind == "random":
            print(f"upsample2x_bwd {dtype} {case}: err/bound {worst:.3f}")
            assert worst <= 1.0
        del dbuf, dup, xbuf, dx


# =============================================================================================== E. fp32 yolo_conv_wgrad
WGRAD32_CASES = [  # (N, H, W, cin, cout, k, s, x_ld, x_off, dz_ld), K slices of plan_wgrad        instantiation <BM, BN>, reduce
    ((1, 100, 93, 32, 64, 3, 1, 32, 0, 64), 37),        # <64,64>; last slice 3 steps, last step 20 px; wgrad_reduce<16>, odd slice count
    ((4, 33, 31, 64, 128, 3, 1, 64, 0, 128), 16),       # <128,64>; last step 28 px; <4>
    ((2, 40, 28, 64, 128, 3, 1, 64, 0, 128), 9),        # <128,64>; last slice 6 steps; <4>
    ((1, 48, 48, 128, 64, 1, 1, 128, 0, 64), 9),        # <64,128>; 1x1; <4>
    ((2, 13, 13, 128, 256, 3, 1, 128, 0, 256), 2),      # <128,128>; two M tiles; slices of 6 + 5 steps, last step 18 px; <1>
    ((2, 13, 13, 128, 64, 3, 2, 128, 0, 64), 1),        # <64,128>; stride 2 with odd H; last step 2 px
    ((1, 19, 38, 192, 96, 3, 1, 192, 0, 96), 3),        # <128,128>; two N tiles per tap, the second half empty
    ((3, 9, 9, 40, 72, 3, 1, 40, 0, 72), 1),            # <128,64>; channels no multiples of the tiles
    ((2, 7, 7, 512, 255, 1, 1, 512, 0, 256), 1),        # head: 255 outputs over two M tiles
    ((3, 10, 10, 256, 21, 1, 1, 256, 0, 32), 2),        # head: 21 outputs
    ((1, 20, 36, 3, 32, 3, 1, 4, 0, 32), 3),            # SMALLC <64,64>
    ((2, 9, 11, 3, 96, 3, 1, 4, 0, 96), 1),             # SMALLC <128,64>
    ((1, 1, 5, 64, 64, 3, 1, 64, 0, 64), 1),            # one row: every vertical tap out of range
    ((2, 26, 26, 128, 128, 1, 1, 384, 256, 128), 6),    # input read from a route / concat slice
]


def _wgrad_setup(L, case):
    N, H, W, cin, cout, k, s, x_ld, x_off, dz_ld = case
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(repr(case).encode())))
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    x = torch.from_numpy(rng.standard_normal((N, H, W, cin), dtype=np.float32))
    dz = torch.zeros((N, Ho, Wo, dz_ld))
    dz[..., :cout] = torch.from_numpy(rng.standard_normal((N, Ho, Wo, cout), dtype=np.float32))      # padding channels zero
    xp = torch.from_numpy(rng.standard_normal((N, H, W, x_ld), dtype=np.float32))                    # neighbours of the slice: noise
    if cin < 4:
        xp[..., cin:4] = 0                                                                           # the input buffer's own padding
    xp[..., x_off:x_off + cin] = x
    need = L.lib().yolo_wgrad_workspace_bytes(N, H, W, cin, cout, k, s, L.F32)
    return x, dz, xp.cuda(), dz.cuda(), need


def _wgrad_call(L, case, xd, dzd, need, ws_bytes=None):
    N, H, W, cin, cout, k, s, x_ld, x_off, dz_ld = case
    ws = _ws(need)
    dw = torch.full((cout, cin, k, k), float("nan"), device="cuda")
    rc = L.lib().yolo_conv_wgrad(dzd.data_ptr(), dz_ld, 0, xd.data_ptr(), x_ld, x_off, dw.data_ptr(), N, H, W, cin, cout, k, s, L.F32,
                                 ws.data_ptr(), need if ws_bytes is None else ws_bytes, L.current_stream())
    _sync()
    assert _guard_ok(ws, need), "wgrad wrote past its stated workspace"
    return rc, dw


# measured on an MI355X: largest max|err| / max|want| over the cases 5.9e-7
@pytest.mark.parametrize("case,nslices", WGRAD32_CASES, ids=["x".join(map(str, c)) for c, _ in WGRAD32_CASES])
def test_wgrad_fp32_kernel_vs_fp64(L, case, nslices):
    """yolo_conv_wgrad(fp32) against the fp64 weight gradient of conv2d on the same operands; the bar of
    test_wgrad_16bit_kernel_vs_fp64 (both paths accumulate exact products in fp32 the same way). dw is pre-filled with NaN."""
    N, H, W, cin, cout, k, s, x_ld, x_off, dz_ld = case
    x, dz, xd, dzd, need = _wgrad_setup(L, case)
    bm, cp = (128 if cout > 64 else 64), (cin + 3) // 4 * 4
    assert need == nslices * _ceil(cout, bm) * bm * k * k * cp * 4, "the case no longer has the K slices it was chosen for"
    w = torch.zeros((cout, cin, k, k), dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w, stride=s, padding=k // 2)
    y.backward(dz[..., :cout].double().permute(0, 3, 1, 2))
    want = w.grad
    rc, dw = _wgrad_call(L, case, xd, dzd, need)
    L.check(rc, "yolo_conv_wgrad")
    err = float((dw.cpu().double() - want).abs().max() / want.abs().max())
    print(f"wgrad fp32 {case}: rel err {err:.3e}")
    assert err < 2e-5, f"{case}: rel err {err}"


def test_wgrad_fp32_fixed_order_and_workspace_check(L):
    """Two calls give the same bits (the header promises a fixed order of additions); a workspace one byte short is refused."""
    case = WGRAD32_CASES[0][0]
    x, dz, xd, dzd, need = _wgrad_setup(L, case)
    rc1, a = _wgrad_call(L, case, xd, dzd, need)
    rc2, b = _wgrad_call(L, case, xd, dzd, need)
    assert rc1 == YOLO_OK and rc2 == YOLO_OK and torch.equal(a, b) and not bool(torch.isnan(a).any())
    rc, c = _wgrad_call(L, case, xd, dzd, need, ws_bytes=need - 1)
    assert rc == YOLO_ERR_WORKSPACE and bool(torch.isnan(c).all())


# =============================================================================================== F. fp32 yolo_conv_dgrad_s2
S2_DGRAD32_CASES = [  # (B, Ho, Wo, cin, cout, residual, dz_ld, dx_ld, dx_off)
    (2, 13, 13, 32, 64, False, 64, 32, 0), (1, 26, 26, 64, 128, True, 128, 64, 0), (3, 5, 5, 64, 128, True, 160, 96, 32),
    (2, 8, 8, 32, 96, False, 96, 32, 0), (1, 12, 12, 128, 256, True, 256, 128, 0),      # S2_DGRAD_CASES of test_gpu_parity.py
    (2, 5, 9, 64, 128, True, 128, 64, 0),               # rectangular
    (1, 3, 3, 32, 64, False, 64, 32, 0),                # Mc = 9: one ragged tile per class
    (1, 1, 4, 32, 32, False, 32, 32, 0),                # no row below
    (1, 6, 6, 96, 64, True, 64, 160, 32),               # second channel tile ragged
]


# measured on an MI355X: largest max|err| / max|ref| over the cases 9.8e-7
@pytest.mark.parametrize("case", S2_DGRAD32_CASES, ids=["x".join(map(str, map(int, c))) for c in S2_DGRAD32_CASES])
def test_stride2_input_gradient_fp32(L, case):
    """yolo_conv_dgrad_s2(fp32) (parity-class-major transposed convolution) with yolo_pack_weights_dgrad(flip = 0) against
    fp64 conv_transpose2d(stride 2, padding 1, output_padding 1) [+ residual]; 1e-5 of max |ref|, the bar of
    test_fp32_winograd_input_gradient (the reduction here is shorter). Untouched channels of dx keep their bits."""
    import torch.nn.functional as F
    B, Ho, Wo, cin, cout, residual, dz_ld, dx_ld, dx_off = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    lib, st = L.lib(), L.current_stream()
    dz = torch.randn((B, Ho, Wo, dz_ld), generator=g)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (cout * 2.25)) ** 0.5
    dx0 = torch.randn((B, 2 * Ho, 2 * Wo, dx_ld), generator=g)
    wp = torch.empty(lib.yolo_packed_dgrad_bytes(cout, cin, 3, 0, L.F32), dtype=torch.uint8, device="cuda")
    L.check(lib.yolo_pack_weights_dgrad(w.cuda().data_ptr(), wp.data_ptr(), cout, cin, 3, 0, L.F32, st), "pack")
    ref = F.conv_transpose2d(dz[..., :cout].double().permute(0, 3, 1, 2), w.double(), stride=2, padding=1, output_padding=1)
    ref = ref.permute(0, 2, 3, 1)
    if residual:
        ref = ref + dx0[..., dx_off:dx_off + cin].double()
    dzd, dxd = dz.cuda(), dx0.clone().cuda()
    L.check(lib.yolo_conv_dgrad_s2(dzd.data_ptr(), dz_ld, 0, wp.data_ptr(), dxd.data_ptr() if residual else 0, dx_ld, dx_off, dxd.data_ptr(),
                                   dx_ld, dx_off, B, Ho, Wo, cin, cout, L.F32, st), "yolo_conv_dgrad_s2")
    _sync()
    got = dxd.cpu()
    err = float((got[..., dx_off:dx_off + cin].double() - ref).abs().max() / ref.abs().max())
    print(f"dgrad_s2 fp32 {case}: rel err {err:.3e}")
    assert err <= 1e-5, err
    keep = torch.ones(dx_ld, dtype=torch.bool)
    keep[dx_off:dx_off + cin] = False
    assert torch.equal(got[..., keep], dx0[..., keep])


# =============================================================================================== G. fp32 1x1 input gradient
DGRAD1_CASES = [  # (B, H, W, cin, cout, accumulate, dx_ld, dx_off)
    (2, 10, 10, 256, 255, False, 256, 0),               # head: coutp = 256
    (3, 9, 7, 512, 21, True, 512, 0),                   # head: coutp = 32, accumulate
    (1, 13, 13, 128, 256, True, 384, 256),              # accumulate into a slice of a concat buffer
    (2, 20, 20, 64, 32, False, 64, 0),
]


# measured on an MI355X: largest max|err| / max|ref| over the cases 6.7e-7
@pytest.mark.parametrize("case", DGRAD1_CASES, ids=["x".join(map(str, map(int, c))) for c in DGRAD1_CASES])
def test_fp32_1x1_input_gradient(L, case):
    """The input gradient of a 1x1 convolution as the train step runs it: yolo_pack_weights_dgrad(flip = 1, ksize = 1) and the
    forward kernels (yolo_conv_fwd_ws, the library's own tile choice) over dz with its channels padded to 32 (the heads' 255 ->
    256 and 21 -> 32), identity epilogue, optional accumulate. Reference fp64; 1e-5 of max |ref| as for the 3x3 one."""
    B, H, W, cin, cout, accumulate, dx_ld, dx_off = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    lib, st = L.lib(), L.current_stream()
    coutp = (cout + 31) // 32 * 32
    dz = torch.zeros((B, H, W, coutp))
    dz[..., :cout] = torch.randn((B, H, W, cout), generator=g)
    w = torch.randn((cout, cin, 1, 1), generator=g) * (1.0 / cin) ** 0.5
    dx0 = torch.randn((B, H, W, dx_ld), generator=g)
    ref = torch.einsum("bhwo,oi->bhwi", dz[..., :cout].double(), w[:, :, 0, 0].double())
    if accumulate:
        ref = ref + dx0[..., dx_off:dx_off + cin].double()
    wp = torch.empty(lib.yolo_packed_dgrad_bytes(cout, cin, 1, 1, L.F32), dtype=torch.uint8, device="cuda")
    L.check(lib.yolo_pack_weights_dgrad(w.cuda().data_ptr(), wp.data_ptr(), cout, cin, 1, 1, L.F32, st), "pack")
    ones, zeros = torch.ones(cin, device="cuda"), torch.zeros(cin, device="cuda")
    d = L.ConvDesc(n=B, h=H, w=W, cin=coutp, cout=cin, ksize=1, stride=1, x_ld=coutp, x_off=0, y_ld=dx_ld, y_off=dx_off, r_ld=dx_ld,
                   r_off=dx_off, act=L.ACT_NONE, out_mode=L.OUT_NHWC, dtype=L.F32, flags=L.FLAG_RESIDUAL if accumulate else 0, tile=0)
    need = lib.yolo_conv_workspace_bytes(d)
    ws = _ws(max(need, 16))
    dzd, dxd = dz.cuda(), dx0.clone().cuda()
    L.check(lib.yolo_conv_fwd_ws(d, dzd.data_ptr(), wp.data_ptr(), ones.data_ptr(), zeros.data_ptr(), dxd.data_ptr() if accumulate else 0,
                                 dxd.data_ptr(), ws.data_ptr() if need else 0, need, 0, st), "yolo_conv_fwd_ws(1x1 dgrad)")
    _sync()
    assert _guard_ok(ws, max(need, 16))
    got = dxd.cpu()
    err = float((got[..., dx_off:dx_off + cin].double() - ref).abs().max() / ref.abs().max())
    print(f"1x1 dgrad fp32 {case}: rel err {err:.3e}")
    assert err <= 1e-5, err
    keep = torch.ones(dx_ld, dtype=torch.bool)
    keep[dx_off:dx_off + cin] = False
    assert torch.equal(got[..., keep], dx0[..., keep])
