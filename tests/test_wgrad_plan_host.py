"""The 16-bit weight gradient on the host (nothing is launched): yolo_wgrad_plan against a Python restatement of the launch plans
(tests/wgrad_h16_cases.py) on the case tables of tests/test_gpu_wgrad_h16.py and on the network's own layers, the routing rules of
yolo_conv_wgrad one by one, the return codes of calls that are refused before any launch, and the fp64 reference the GPU tests
compare with (train_kernels_ref.wgrad_ref) against torch.autograd."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import train_kernels_ref as R
from tests import wgrad_h16_cases as W

OK, ERR_ARG, ERR_WORKSPACE = 0, -1, -4
FAKE = 1 << 20          # a non-null, 16-byte aligned "device pointer" for calls that must return before they launch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def _plan(L, case, dtype=None):
    n, h, w, cin, cout, k, s, x_ld, x_off, dz_ld, dz_off = case
    out = (C.c_int32 * 8)(*[-7] * 8)
    rc = L.lib().yolo_wgrad_plan(n, h, w, cin, cout, k, s, L.BF16 if dtype is None else dtype, dz_ld, dz_off, x_ld, x_off, out)
    return rc, list(out)


def _kernel(L, case, dtype=None):
    rc, out = _plan(L, case, dtype)
    assert rc == OK, (case, L.lib().yolo_last_error())
    return out[0]


def _call(L, case, dtype=None, dz=FAKE, x=FAKE, ws=FAKE, ws_bytes=None):
    """yolo_conv_wgrad on fake pointers: it must come back before any launch."""
    n, h, w, cin, cout, k, s, x_ld, x_off, dz_ld, dz_off = case
    lib, dt = L.lib(), L.BF16 if dtype is None else dtype
    need = lib.yolo_wgrad_workspace_bytes(n, h, w, cin, cout, k, s, dt)
    return lib.yolo_conv_wgrad(dz, dz_ld, dz_off, x, x_ld, x_off, FAKE, n, h, w, cin, cout, k, s, dt, ws, need if ws_bytes is None else ws_bytes,
                               None)


# ------------------------------------------------------------------------------------------------- the plans
@pytest.mark.parametrize("name,case,expect", W.ALL_CASES, ids=[nm for nm, _, _ in W.ALL_CASES])
def test_plan_of_the_table_cases(built, name, case, expect):
    """The library's plan equals the restatement, in both 16-bit dtypes, and is what the table says the case was chosen for."""
    L = built
    assert W.accepted(case)
    for dt in (L.BF16, L.F16):
        rc, out = _plan(L, case, dt)
        assert rc == OK and out == W.plan(case)
    assert (out[0], out[3], out[5], out[6]) == expect, "the case no longer has the geometry it was chosen for"
    rc, out = _plan(L, case, L.F32)                         # the same arguments in fp32: the fp32 kernel's plan
    assert rc == OK and out == W.plan(case, sixteen_bit=False) and out[0] == W.F32


def test_what_the_tables_reach():
    """The branches the tables were built for, from the restatement: every fan-in of both reduce kernels, the remainder branch of
    the two-chain loop at G = 16 (slices not a multiple of 32), an empty trailing slice on the dma and on the patch kernel, a slice
    of one K tile, both workgroup maps, the stem's grid cap with a ring that wraps more than once."""
    plans = {nm: W.plan(c) for nm, c, _ in W.ALL_CASES}
    for kern in (W.DMA, W.PATCH):
        assert {p[5] for p in plans.values() if p[0] == kern} == {1, 4, 16}
        assert any(p[6] == 1 for p in plans.values() if p[0] == kern)
        assert {p[3] % 8 == 0 for p in plans.values() if p[0] == kern and p[3] > 1} == {True, False}
    assert plans["dma2"][3:6] == [40, 8, 16] and plans["dma3"][2:5] == [200, 24, 9] and plans["dma4"][2:5] == [1, 1, 1]
    assert plans["dma8"][4] == 13 and plans["dma6"][1] == 6 and plans["dma5"][2:5] == [9, 2, 5]
    assert plans["stem6"][2:5] == [46080, 256, 45] and plans["stem5"][3:5] == [5, 13] and plans["stem1"][2:5] == [1, 1, 1]
    assert W.plan(W.by_name("stem5")[0], stem_cap=1)[3:5] == [1, 65]
    assert W.plan(W.by_name("dma6")[0], no_dma=True)[:2] == [W.PATCH, 6]             # 3 co tiles x 2 ci tiles on wgrad_patch_h16<3, 1>


def test_plan_of_the_network_layers(built):
    """Every convolution of the network at 416 x 416, batch 32, as the 16-bit train step calls it (train_engine.py: x through the
    block's input view, dz dense, the heads' dz padded to 32 channels): the library's plan equals the restatement; the first block
    runs on the stem kernel, every other 3x3 stride-1 block on the dma kernel, the rest on the patch kernel."""
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import engine
    L = built
    prog = engine.build_network_program(yt.YOLOv3(num_classes=80), 32, 416, ch_align=8)
    kernels = []
    for op in prog.ops:
        cv, xv = op["block"].conv, op["x"]
        cout = cv.out_channels
        dz_ld = cout if op["block"].batch_norm_act else (cout + 31) // 32 * 32
        case = (32, xv.H, xv.W, cv.in_channels, cout, op["k"], op["s"], xv.ld, xv.off, dz_ld, 0)
        rc, out = _plan(L, case)
        assert rc == OK and out == W.plan(case), case
        want = W.STEM if cv.in_channels == 3 else W.DMA if (op["k"], op["s"]) == (3, 1) else W.PATCH
        assert out[0] == want, case
        kernels.append(out[0])
    assert len(kernels) == 75 and kernels.count(W.STEM) == 1 and kernels.count(W.DMA) == 32
    assert any(op["x"].off for op in prog.ops), "no layer reads a route / concat slice"


# ------------------------------------------------------------------------------------------------- the routing rules
STEM = (2, 32, 32, 3, 32, 3, 1, 8, 0, 32, 0)        # (N, H, W, cin, cout, k, s, x_ld, x_off, dz_ld, dz_off)
DMA = (2, 13, 13, 64, 128, 3, 1, 64, 0, 128, 0)


def _with(case, **kw):
    names = ("n", "h", "w", "cin", "cout", "k", "s", "x_ld", "x_off", "dz_ld", "dz_off")
    d = dict(zip(names, case))
    d.update(kw)
    return tuple(d[k] for k in names)


def test_stem_rules(built):
    L = built
    assert _kernel(L, STEM) == W.STEM and _kernel(L, _with(STEM, cin=1)) == W.STEM and _kernel(L, _with(STEM, cout=24)) == W.STEM
    assert _kernel(L, _with(STEM, x_ld=16)) == W.PATCH                      # x_ld == 8
    assert _kernel(L, _with(STEM, w=40)) == W.PATCH                         # w % 16 == 0
    assert _kernel(L, _with(STEM, cin=4)) == W.PATCH                        # cin <= 3
    assert _kernel(L, _with(STEM, cout=33, dz_ld=40)) == W.PATCH            # cout <= 32
    assert _kernel(L, _with(STEM, s=2)) == W.PATCH and _kernel(L, _with(STEM, k=1)) == W.PATCH
    # at least 32 dz channels from dz_off to the end of the row, whatever cout is
    assert _kernel(L, _with(STEM, cout=24, dz_ld=64, dz_off=32)) == W.STEM
    assert _kernel(L, _with(STEM, cout=24, dz_ld=24)) == W.PATCH
    assert _kernel(L, _with(STEM, cout=8, dz_ld=56, dz_off=32)) == W.PATCH
    assert _kernel(L, STEM, L.F32) == W.F32


def test_stem_kernel_is_not_given_a_row_it_would_read_past(built):
    """cout = 24, dz_ld = 40, dz_off = 16: the stem kernel moves 32 dz channels per pixel from dz_off, 8 of them the next pixel's
    and, at the last pixel, 16 bytes past the tensor. Nothing of that reaches a result, so only the routing can be checked."""
    L = built
    case = (3, 7, 48, 3, 24, 3, 1, 8, 0, 40, 16)
    assert W.accepted(case) and _plan(L, case) == (OK, W.plan(case)) and _kernel(L, case) == W.PATCH
    assert _kernel(L, _with(case, dz_ld=48)) == W.STEM                      # 32 channels from 16: inside the row


def test_dma_rules(built):
    L = built
    assert _kernel(L, DMA) == W.DMA and _kernel(L, _with(DMA, cin=32, x_ld=32)) == W.DMA
    assert _kernel(L, _with(DMA, cin=40, x_ld=96, x_off=24, cout=72, dz_ld=160, dz_off=80)) == W.DMA
    assert _kernel(L, _with(DMA, cin=24, x_ld=24)) == W.PATCH               # cin >= 32
    assert _kernel(L, _with(DMA, s=2)) == W.PATCH                           # stride 1
    assert _kernel(L, _with(DMA, k=1)) == W.PATCH                           # 3x3
    assert _kernel(L, DMA, L.F32) == W.F32


def test_everything_else_goes_to_patch(built):
    L = built
    for case in ((2, 13, 13, 256, 128, 1, 1, 256, 0, 128, 0), (2, 13, 13, 128, 21, 1, 1, 384, 256, 32, 0), (1, 16, 16, 128, 64, 3, 2, 128, 0, 64, 0),
                 (1, 9, 9, 16, 24, 3, 1, 16, 0, 24, 0), (1, 9, 9, 3, 64, 3, 1, 8, 0, 64, 0)):
        assert _kernel(L, case) == W.PATCH and _kernel(L, case, L.F16) == W.PATCH
    assert _kernel(L, (2, 13, 13, 128, 64, 1, 2, 128, 0, 64, 0)) == W.F32   # the patch kernel has no strided 1x1


@pytest.mark.parametrize("field", ["x_ld", "x_off", "dz_ld", "dz_off"])
def test_ld_or_off_not_a_multiple_of_8_goes_to_the_fp32_layout_kernel(built, field):
    L = built
    wide = {"dma": _with(DMA, x_ld=128, x_off=32, dz_ld=256, dz_off=64), "patch": (2, 13, 13, 64, 128, 1, 1, 128, 32, 256, 64),
            "stem": _with(STEM, dz_ld=64, dz_off=8)}
    for name, case in wide.items():
        assert _kernel(L, case) == {"dma": W.DMA, "patch": W.PATCH, "stem": W.STEM}[name]
        if name == "stem" and field.startswith("x"):
            continue                                                        # x_ld is 8 there
        odd = _with(case, **{field: dict(zip(("x_ld", "x_off", "dz_ld", "dz_off"), case[7:]))[field] + 4})
        assert W.accepted(odd) and _kernel(L, odd) == W.F32, (name, odd)
        assert _plan(L, odd) == (OK, W.plan(odd))


# ------------------------------------------------------------------------------------------------- refusals before a launch
def test_slices_that_do_not_fit_their_buffer_are_refused(built):
    L = built
    lib = L.lib()
    for dt in (L.F32, L.BF16, L.F16):
        assert _call(L, _with(DMA, dz_ld=128, dz_off=8), dt) == ERR_ARG and b"slice" in lib.yolo_last_error()      # 8 + 128 > 128
        assert _call(L, _with(DMA, x_ld=64, x_off=8), dt) == ERR_ARG and b"slice" in lib.yolo_last_error()
        assert _call(L, _with(DMA, cout=72, dz_ld=160, dz_off=96), dt) == ERR_ARG
        assert _call(L, _with(DMA, cin=40, x_ld=96, x_off=64), dt) == ERR_ARG
        assert _plan(L, _with(DMA, dz_ld=128, dz_off=8), dt)[0] == ERR_ARG and _plan(L, _with(DMA, x_ld=64, x_off=8), dt)[0] == ERR_ARG
        assert not W.accepted(_with(DMA, dz_ld=128, dz_off=8)) and not W.accepted(_with(DMA, cin=40, x_ld=96, x_off=64))
    # the slices at the very end of their rows are fine: with a one-byte-short workspace the call gets as far as that check
    for case in (_with(DMA, cout=72, dz_ld=160, dz_off=88), _with(DMA, cin=40, x_ld=96, x_off=56)):
        assert _plan(L, case)[0] == OK


def test_16_bit_operands_must_be_16_byte_aligned(built):
    L = built
    lib = L.lib()
    cases = {"dma": DMA, "patch": (2, 13, 13, 256, 128, 1, 1, 256, 0, 128, 0), "stem": STEM, "fp32 layout": _with(DMA, x_ld=68)}
    for name, case in cases.items():
        for dt in (L.BF16, L.F16):
            for arg in ("dz", "x", "ws"):
                for off in (2, 8):
                    assert _call(L, case, dt, **{arg: FAKE + off}) == ERR_ARG, (name, arg, off)
                    assert b"aligned" in lib.yolo_last_error()


def test_short_workspace_and_bad_arguments_are_refused(built):
    L = built
    lib = L.lib()
    for case in (DMA, STEM, (2, 13, 13, 256, 128, 1, 1, 256, 0, 128, 0)):
        for dt in (L.F32, L.BF16, L.F16):
            need = lib.yolo_wgrad_workspace_bytes(*case[:7], dt)
            assert need > 0
            assert _call(L, case, dt, ws_bytes=need - 1) == ERR_WORKSPACE and b"workspace" in lib.yolo_last_error()
            assert _call(L, case, dt, ws_bytes=0) == ERR_WORKSPACE
            assert _call(L, case, dt, ws=0) == ERR_ARG and _call(L, case, dt, dz=0) == ERR_ARG and _call(L, case, dt, x=0) == ERR_ARG
    assert _call(L, _with(DMA, k=5)) == ERR_ARG and _plan(L, _with(DMA, k=5))[0] == ERR_ARG
    assert _call(L, _with(DMA, x_ld=32)) == ERR_ARG and _plan(L, _with(DMA, x_ld=32))[0] == ERR_ARG            # x_ld < cin
    assert _call(L, _with(DMA, dz_ld=130)) == ERR_ARG and _plan(L, _with(DMA, dz_ld=130))[0] == ERR_ARG        # not a multiple of 4
    assert lib.yolo_wgrad_plan(*DMA[:7], L.BF16, 128, 0, 64, 0, None) == ERR_ARG
    assert lib.yolo_version() >= 102


# ------------------------------------------------------------------------------------------------- the fp64 reference
@pytest.mark.parametrize("shape", [(2, 5, 7, 3, 4, 3, 1), (1, 6, 5, 2, 3, 3, 2), (2, 7, 7, 3, 2, 3, 2), (1, 1, 5, 2, 2, 3, 2), (1, 4, 1, 2, 2, 3, 1),
                                   (3, 4, 4, 5, 6, 1, 1), (1, 1, 1, 1, 1, 3, 1)])
def test_wgrad_ref_equals_autograd_fp64(shape):
    """(n, h, w, cin, cout, k, stride): the nine shifted sums against the weight gradient of conv2d under autograd, to 1e-12 of
    the largest magnitude."""
    n, h, w, cin, cout, k, s = shape
    g = torch.Generator().manual_seed(sum(shape))
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    x = torch.randn((n, h, w, cin), generator=g, dtype=torch.float64)
    dz = torch.randn((n, ho, wo, cout), generator=g, dtype=torch.float64)
    wt = torch.zeros((cout, cin, k, k), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.permute(0, 3, 1, 2), wt, stride=s, padding=pad).backward(dz.permute(0, 3, 1, 2))
    got = R.wgrad_ref(x, dz, k, s)
    assert got.dtype == torch.float64 and got.shape == wt.grad.shape
    assert float((got - wt.grad).abs().max()) <= 1e-12 * float(wt.grad.abs().max())
    # 16-bit operands are promoted, not multiplied in their own precision
    xb, dzb = x.to(torch.bfloat16), dz.to(torch.bfloat16)
    assert torch.equal(R.wgrad_ref(xb, dzb, k, s), R.wgrad_ref(xb.double(), dzb.double(), k, s))
