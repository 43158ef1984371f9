"""What the GPU tests of the 16-bit convolution kernels share (tests/test_gpu_conv_patch_h16.py,
tests/test_gpu_conv_dma_h16.py): guarded output buffers, bit comparison, and the device side of one case of
tests/conv_h16_ref.py launched through the C ABI."""
import ctypes as C
import functools

import torch

from tests import conv_h16_ref as R

SENT = -12288.0                       # exact in fp32, fp16 and bf16
GUARD = 256
ERR_UNSUPPORTED = -2                  # YOLO_ERR_UNSUPPORTED


def code(L, dtype):
    return {"bf16": L.BF16, "fp16": L.F16}[dtype]


class Out:
    """`numel` elements of `tdt` filled with `fill`, with GUARD bytes of 0xA5 in front of and behind them"""

    def __init__(self, numel, tdt, fill=SENT):
        size = torch.empty((), dtype=tdt).element_size()
        self.raw = torch.full((GUARD + numel * size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.end = GUARD + numel * size
        self.t = self.raw[GUARD:self.end].view(tdt)
        self.t.fill_(fill)

    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def guards_ok(self):
        return bool((self.raw[:GUARD] == 0xA5).all()) and bool((self.raw[self.end:] == 0xA5).all())


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def reference(c, dtype, gauss):
    """(operands, fp64 value ahead of the store in the stored layout), computed once per case and type on the CPU"""
    ops = R.operands(c, dtype, gauss)
    return ops, R.stored(c, R.value(c, ops, torch.float64, kernel_steps=not gauss))


@functools.lru_cache(maxsize=None)
def switches(L):
    """the A/B switches the library read when it was loaded, {name: value}"""
    buf = C.create_string_buffer(4096)
    n = L.lib().yolo_switches_describe(buf, len(buf))
    assert 0 < n < len(buf)
    return {k: int(v) for k, v in (ln.split("=") for ln in buf.value.decode().splitlines())}


class Launch:
    """the device side of one case: operands uploaded and weights packed once, then one launch per tile"""

    def __init__(self, L, c, dtype, ops):
        self.L, self.c, self.dtype, self.code, self.tdt = L, c, dtype, code(L, dtype), R.TDT[dtype]
        lib, st = L.lib(), L.current_stream()
        self.x, self.w = ops["x"].cuda(), ops["w"].cuda()
        self.scale, self.shift = ops["scale"].cuda(), ops["shift"].cuda()
        self.r = None if ops["r"] is None else ops["r"].cuda()
        if c.kind == "dgrad":
            self.wp = torch.zeros(lib.yolo_packed_dgrad_bytes(c.cout, c.cin, 3, 0, self.code), dtype=torch.uint8, device="cuda")
            L.check(lib.yolo_pack_weights_dgrad(self.w.data_ptr(), self.wp.data_ptr(), c.cout, c.cin, 3, 0, self.code, st), "pack dgrad")
        else:
            self.wp = torch.zeros(lib.yolo_packed_weight_bytes(c.cout, c.cin, c.k, self.code), dtype=torch.uint8, device="cuda")
            L.check(lib.yolo_pack_weights(self.w.data_ptr(), self.wp.data_ptr(), c.cout, c.cin, c.k, self.code, st), "pack")

    def desc(self, tile, flags):
        c = self.c
        return self.L.ConvDesc(n=c.B, h=c.H, w=c.W, cin=c.cin, cout=c.cout, ksize=c.k, stride=c.stride, x_ld=c.x_ld, x_off=c.x_off, y_ld=c.y_ld,
                               y_off=c.y_off, r_ld=c.r_ld, r_off=c.r_off, act=c.act, out_mode=c.out, dtype=self.code, flags=flags, tile=tile)

    def launch(self, tile=0, x=None, flag=None, nancheck=True):
        """one launch into a fresh output; returns (return code, the output as the host sees it: whole buffer, ld channels wide)"""
        L, c = self.L, self.c
        lib, st = L.lib(), L.current_stream()
        x = self.x if x is None else x
        oh, ow = R.out_hw(c)
        if c.out == R.OUT_HEAD:
            shape, out = (c.B, 3, oh, ow, c.cout // 3), Out(c.B * oh * ow * c.cout, torch.float32, float("nan"))
        else:
            shape, out = (c.B, oh, ow, c.y_ld), Out(c.B * oh * ow * c.y_ld, self.tdt)
        r = self.r
        if c.res == 2:                                              # accumulate in place: the output buffer holds the residual
            out.t.copy_(self.r.view(-1))
            r = out
        rptr = 0 if r is None else (r.ptr() if isinstance(r, Out) else r.data_ptr())
        if c.kind == "dgrad":
            rc = lib.yolo_conv_dgrad_s2(x.data_ptr(), c.x_ld, c.x_off, self.wp.data_ptr(), rptr, c.r_ld, c.r_off, out.ptr(), c.y_ld, c.y_off,
                                        c.B, c.H, c.W, c.cin, c.cout, self.code, st)
        else:
            d = self.desc(tile, (L.FLAG_RESIDUAL if c.res else 0) | (L.FLAG_NANCHECK if nancheck else 0))
            rc = lib.yolo_conv_fwd(d, x.data_ptr(), self.wp.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(), rptr, out.ptr(),
                                   L.ptr(flag), st)
        torch.cuda.synchronize()
        assert out.guards_ok(), "%s tile %d wrote outside its output" % (c.name, tile)
        return rc, out.t.view(shape).cpu()

    def run(self, tile=0, x=None, flag=None, nancheck=True):
        """launch(), which must succeed; returns the output"""
        rc, got = self.launch(tile, x, flag, nancheck)
        self.L.check(rc, "yolo_conv_dgrad_s2" if self.c.kind == "dgrad" else "yolo_conv_fwd")
        return got

    def run_stats(self, tile=0):
        """yolo_conv_fwd_stats into fresh buffers: (z as the host sees it, the partial rows (rows, 2, ld) NaN-filled before)"""
        L, c = self.L, self.c
        lib, st = L.lib(), L.current_stream()
        d = self.desc(tile, 0)
        ld = C.c_int(0)
        rows = lib.yolo_conv_stats_rows(d, C.byref(ld))
        assert rows > 0 and ld.value >= c.cout, (c.name, rows, ld.value)
        oh, ow = R.out_hw(c)
        out = Out(c.B * oh * ow * c.y_ld, self.tdt)
        part = Out(rows * 2 * ld.value, torch.float32, float("nan"))
        L.check(lib.yolo_conv_fwd_stats(d, self.x.data_ptr(), self.wp.data_ptr(), out.ptr(), part.ptr(), part.t.numel() * 4, st), "yolo_conv_fwd_stats")
        torch.cuda.synchronize()
        assert out.guards_ok() and part.guards_ok(), "%s tile %d wrote outside its output" % (c.name, tile)
        return out.t.view(c.B, oh, ow, c.y_ld).cpu(), part.t.view(rows, 2, ld.value).cpu()

    def split(self, got):
        """(the channels the launch owns, whether every other channel of the buffer came back as it was)"""
        c = self.c
        if c.out == R.OUT_HEAD:
            return got, True
        keep = torch.ones(c.y_ld, dtype=torch.bool)
        keep[c.y_off:c.y_off + R.n_out(c)] = False
        before = self.r.cpu()[..., keep] if c.res == 2 else torch.full_like(got[..., keep], SENT)
        return got[..., c.y_off:c.y_off + R.n_out(c)], same_bits(got[..., keep], before)
