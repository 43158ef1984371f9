"""GPU tests (``-m gpu``) of the 16-bit weight-gradient kernels, called through the C ABI (yolo_conv_wgrad, bf16 and fp16) at the
edges of their launch geometry:

  wgrad_patch_h16<T, 1, 1 | 3, 2 | 3, 1> + wgrad_reduce<1|4|16>       wgrad_h16.hip
  wgrad3_dma_h16<T, 3 | 5> + wgrad_reduce_acc<1|4|16>                 wgrad_dma_h16.hip
  stem_wgrad_h16 + stem_wgrad_reduce                                  wgrad_stem_h16.hip

The cases and what each is meant to reach are in tests/wgrad_h16_cases.py. Every case first asserts, through yolo_wgrad_plan, that it
still runs on the kernel and with the K slices, reduce fan-in and empty trailing slices it was chosen for. x and dz are channel
slices [off, off + c) of wider buffers whose other channels hold noise of the operands' scale (only a slice's own padding up to the
next multiple of 8 channels is zero, as the kernels ask). dw is pre-filled with NaN; the workspace is exactly
yolo_wgrad_workspace_bytes, followed by 256 guard bytes that must survive. Operands are seeded from the case tuple, generated on the
device and referenced in fp64 on the device (train_kernels_ref.wgrad_ref, tied to autograd by tests/test_wgrad_plan_host.py).
The switch variants (fall-back routes, look-ahead 5, one stem workgroup) run in a child process: tests/workers/wgrad_h16_cases.py.
Every measured maximum is printed (run with -s)."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from tests import train_kernels_ref as R
from tests import wgrad_h16_cases as W

pytestmark = pytest.mark.gpu

GUARD = 256                           # bytes behind the workspace that must stay 0xA5
YOLO_OK, YOLO_ERR_WORKSPACE = 0, -4
DTYPES = ["bf16", "fp16"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM_BAR = 2e-5                     # max|err| / max|want|: the bar of test_wgrad_16bit_kernel_vs_fp64 and of the fp32 kernel's test


@pytest.fixture(scope="module")
def L():
    from yolo_for_turbines_amd import _lib
    _lib.lib()                        # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd as pkg
    from yolo_for_turbines_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return pkg


def _dt(L, dtype):
    return {"bf16": (L.BF16, torch.bfloat16), "fp16": (L.F16, torch.float16)}[dtype]


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(key).encode()))


def _out_hw(case):
    N, H, W_, cin, cout, k, s = case[:7]
    pad = k // 2
    return (H + 2 * pad - k) // s + 1, (W_ + 2 * pad - k) // s + 1


def _ints(shape, amp, g, tdt):
    """integers in +-{1..amp}: exact in both 16-bit types"""
    v = torch.randint(-amp, amp, shape, generator=g, device="cuda", dtype=torch.int8)
    return torch.where(v >= 0, v + 1, v).to(tdt)


def _slice_of(buf, off, c):
    """The channel slice of a buffer, after zeroing the slice's own padding up to the next multiple of 8 channels."""
    buf[..., off + c:min(buf.shape[-1], off + (c + 7) // 8 * 8)] = 0
    return buf[..., off:off + c]


def operands(case, tdt, kind, *key):
    """(x buffer, dz buffer, x slice, dz slice) of a case; kind "exact" (integers whose fp32 sums are exact in any order) or
    "random" (standard normal, rounded to the dtype). The neighbour channels of both slices hold the same kind of values."""
    N, H, W_, cin, cout, k, s, x_ld, x_off, dz_ld, dz_off = case
    Ho, Wo = _out_hw(case)
    g = _gen("wgrad16", kind, str(tdt), case, *key)
    if kind == "exact":
        pixels = N * Ho * Wo
        amp = 8 if pixels * 64 <= 2 ** 24 else 4
        assert pixels * amp * amp <= 2 ** 24, "a sum of this many products is not exact in fp32"
        xbuf, dzbuf = _ints((N, H, W_, x_ld), amp, g, tdt), _ints((N, Ho, Wo, dz_ld), amp, g, tdt)
    else:
        xbuf = torch.randn((N, H, W_, x_ld), generator=g, device="cuda").to(tdt)
        dzbuf = torch.randn((N, Ho, Wo, dz_ld), generator=g, device="cuda").to(tdt)
    return xbuf, dzbuf, _slice_of(xbuf, x_off, cin), _slice_of(dzbuf, dz_off, cout)


def call(L, case, code, xbuf, dzbuf, ws_bytes=None):
    """yolo_conv_wgrad into a NaN-filled dw with a guarded workspace of exactly the stated size; (rc, dw)."""
    N, H, W_, cin, cout, k, s, x_ld, x_off, dz_ld, dz_off = case
    lib = L.lib()
    need = lib.yolo_wgrad_workspace_bytes(N, H, W_, cin, cout, k, s, code)
    assert need > 0
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dw = torch.full((cout, cin, k, k), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.yolo_conv_wgrad(dzbuf.data_ptr(), dz_ld, dz_off, xbuf.data_ptr(), x_ld, x_off, dw.data_ptr(), N, H, W_, cin, cout, k, s, code,
                             ws.data_ptr(), need if ws_bytes is None else ws_bytes, L.current_stream())
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "wgrad wrote past its stated workspace"
    return rc, dw


def library_plan(L, case, code):
    import ctypes as C
    N, H, W_, cin, cout, k, s, x_ld, x_off, dz_ld, dz_off = case
    out = (C.c_int32 * 8)()
    L.check(L.lib().yolo_wgrad_plan(N, H, W_, cin, cout, k, s, code, dz_ld, dz_off, x_ld, x_off, out), "yolo_wgrad_plan")
    return list(out)


def assert_geometry(L, case, code, expect=None, **env):
    """The launch the library plans is the one restated for this environment (and, by default, the table's)."""
    got, want = library_plan(L, case, code), W.plan(case, **env)
    assert got == want, f"{case}: plan {got}, restated {want}"
    if expect is not None:
        assert (got[0], got[3], got[5], got[6]) == tuple(expect), f"{case}: the case no longer has the geometry it was chosen for: {got}"
    return got


def run_exact(L, case, dtype):
    """dw must EQUAL the fp64 reference: every product and every partial sum is an integer below 2^24."""
    code, tdt = _dt(L, dtype)
    xbuf, dzbuf, x, dz = operands(case, tdt, "exact")
    want = R.wgrad_ref(x, dz, case[5], case[6])
    rc, dw = call(L, case, code, xbuf, dzbuf)
    L.check(rc, "yolo_conv_wgrad")
    assert float(want.abs().max()) <= 2 ** 24
    bad = int((dw.double() != want).sum())              # (NaN != x: an element that was never written counts)
    assert bad == 0, f"{case} {dtype}: {bad} of {want.numel()} elements differ, largest difference {float((dw.double() - want).abs().max())}"


def run_random(L, case, dtype):
    code, tdt = _dt(L, dtype)
    xbuf, dzbuf, x, dz = operands(case, tdt, "random")
    want = R.wgrad_ref(x, dz, case[5], case[6])
    rc, dw = call(L, case, code, xbuf, dzbuf)
    L.check(rc, "yolo_conv_wgrad")
    err = float((dw.double() - want).abs().max() / want.abs().max())
    print(f"wgrad {dtype} {case}: rel err {err:.3e}")
    assert err < RANDOM_BAR, f"{case} {dtype}: rel err {err}"          # (a NaN fails the comparison)
    return err


CASE_IDS = [nm for nm, _, _ in W.ALL_CASES]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,case,expect", W.ALL_CASES, ids=CASE_IDS)
def test_wgrad_h16_exact_on_integers(L, name, case, expect, dtype):
    assert_geometry(L, case, _dt(L, dtype)[0], expect)
    run_exact(L, case, dtype)


# measured on an MI355X: largest max|err| / max|want| over the cases and both dtypes 2.3e-7 (patch11, bf16); under the switch
# variants of the child runs 2.7e-7 (stem5 as one workgroup, fp16)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,case,expect", W.ALL_CASES, ids=CASE_IDS)
def test_wgrad_h16_random_vs_fp64(L, name, case, expect, dtype):
    """Standard-normal operands rounded to the dtype, against fp64 on the same rounded operands: only the order of the fp32
    additions differs."""
    assert_geometry(L, case, _dt(L, dtype)[0], expect)
    run_random(L, case, dtype)


ONE_OF_EACH = ["dma3", "patch12", "stem5"]          # an empty trailing slice on each of the split-K kernels; five stem workgroups


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ONE_OF_EACH)
def test_wgrad_h16_fixed_order_and_workspace_check(L, name, dtype):
    """Two calls give the same bits (the header promises a fixed order of additions); a workspace one byte short is refused and
    nothing is written."""
    case, expect = W.by_name(name)
    code, tdt = _dt(L, dtype)
    assert_geometry(L, case, code, expect)
    xbuf, dzbuf, x, dz = operands(case, tdt, "random", "twice")
    rc1, a = call(L, case, code, xbuf, dzbuf)
    rc2, b = call(L, case, code, xbuf, dzbuf)
    assert rc1 == YOLO_OK and rc2 == YOLO_OK and torch.equal(a, b) and not bool(torch.isnan(a).any())
    need = L.lib().yolo_wgrad_workspace_bytes(*case[:7], code)
    rc, c = call(L, case, code, xbuf, dzbuf, ws_bytes=need - 1)
    assert rc == YOLO_ERR_WORKSPACE and bool(torch.isnan(c).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["dma6", "stem4"])         # 5 x 17 and 7 x 48: no multiples of the 4 x 16 K tile / of a batch of 4 K steps
def test_wgrad_h16_image_corners(L, name, dtype):
    """x is zero except for one pixel at each corner of each image, dz is one everywhere: tap (kh, kw) of dW[:, ci] then adds up
    exactly the corner pixels that some output pixel sees through that tap: the top corners for kh >= 1 (bottom: kh <= 1), the
    left ones for kw >= 1 (right: kw <= 1). A halo read from the wrong row, column or image lands in another tap."""
    case, expect = W.by_name(name)
    N, H, W_, cin, cout, k, s, x_ld, x_off, dz_ld, dz_off = case
    code, tdt = _dt(L, dtype)
    assert_geometry(L, case, code, expect)
    assert (k, s) == (3, 1) and H >= 2 and W_ >= 2
    xbuf, dzbuf, x, dz = operands(case, tdt, "exact", "corners")       # the neighbour channels keep their noise
    x.zero_()
    dz.fill_(1)
    want = torch.zeros((cin, 3, 3), dtype=torch.float64)
    ci = torch.arange(cin)
    for n in range(N):
        for r, (hi, wi) in enumerate(((0, 0), (0, W_ - 1), (H - 1, 0), (H - 1, W_ - 1))):
            v = (1 + (ci + 3 * r + 5 * n) % 7).double()
            x[n, hi, wi] = v.to(tdt).cuda()
            for kh in range(3):
                for kw in range(3):
                    if 0 <= hi - kh + 1 < H and 0 <= wi - kw + 1 < W_:
                        want[:, kh, kw] += v
    want = want.cuda().expand(cout, cin, 3, 3)
    assert torch.equal(R.wgrad_ref(x, dz, 3, 1), want)
    rc, dw = call(L, case, code, xbuf, dzbuf)
    L.check(rc, "yolo_conv_wgrad")
    assert torch.equal(dw.double(), want)


# ------------------------------------------------------------------------------------------------- switch variants, in a child
@pytest.mark.parametrize("variant", list(W.VARIANTS))
def test_wgrad_h16_switch_variants(variant):
    """The library reads its switches once, at load: a fresh child per environment (tests/workers/wgrad_h16_cases.py) runs the named
    cases with the exact and the random assertion and reports, per case and dtype, the kernel yolo_wgrad_plan named."""
    env, names, _ = W.VARIANTS[variant]
    clean = {k: v for k, v in os.environ.items() if k not in W.SWITCHES}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "workers", "wgrad_h16_cases.py"), variant], env=dict(clean, **env),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("case ")]
    assert sorted((ln[1], ln[2]) for ln in lines) == sorted((nm, dt) for nm in names for dt in DTYPES)
    assert all(ln[-1] == "ok" for ln in lines)
    kernels = {ln[1]: ln[3] for ln in lines}
    if variant == "fallback":
        assert set(kernels.values()) == {W.KERNEL_NAMES[W.PATCH]}
    else:
        assert all(kernels[nm] == W.KERNEL_NAMES[W.DMA if nm.startswith("dma") else W.STEM] for nm in names)


# ------------------------------------------------------------------------------------------------- the kernels' first unit test
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", W.LEGACY_CASES)
def test_wgrad_16bit_kernel_vs_fp64(yt, case, dtype):
    """yolo_conv_wgrad on 16-bit operands (transposing-read MFMA kernel) against an fp64 CPU convolution
    weight gradient of the SAME rounded operands: only the fp32 accumulation order differs."""
    from yolo_for_turbines_amd import _lib as L
    cin, cout, k, s, H, W_, N, dz_ld = case
    tdt, code = (torch.bfloat16, L.BF16) if dtype == "bf16" else (torch.float16, L.F16)
    rng = np.random.Generator(np.random.PCG64(hash(case) % 1000))
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W_ + 2 * pad - k) // s + 1
    x = torch.from_numpy(rng.standard_normal((N, H, W_, cin), dtype=np.float32)).to(tdt)
    x_ld = 8 if cin <= 3 else cin                                   # the first block reads the 8-channel 16-bit input buffer
    dz = torch.zeros((N, Ho, Wo, dz_ld), dtype=tdt)
    dz[..., :cout] = torch.from_numpy(rng.standard_normal((N, Ho, Wo, cout), dtype=np.float32)).to(tdt)
    xw = x.double().permute(0, 3, 1, 2)
    w = torch.zeros((cout, cin, k, k), dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(xw, w, stride=s, padding=pad)
    y.backward(dz[..., :cout].double().permute(0, 3, 1, 2))
    want = w.grad
    lib = L.lib()
    ws = torch.empty(lib.yolo_wgrad_workspace_bytes(N, H, W_, cin, cout, k, s, code), dtype=torch.uint8, device="cuda")
    dw = torch.full((cout, cin, k, k), float("nan"), dtype=torch.float32, device="cuda")
    xp = torch.zeros((N, H, W_, x_ld), dtype=tdt)
    xp[..., :cin] = x
    xd, dzd = xp.cuda(), dz.cuda()
    L.check(lib.yolo_conv_wgrad(dzd.data_ptr(), dz_ld, 0, xd.data_ptr(), x_ld, 0, dw.data_ptr(), N, H, W_, cin, cout, k, s, code,
                                ws.data_ptr(), ws.numel(), L.current_stream()), "wgrad")
    got = dw.cpu().double()
    err = float((got - want).abs().max() / want.abs().max())
    assert err < 2e-5, f"{case} {dtype}: rel err {err}"
