"""What the GPU tests of the fp32 convolution kernels share (tests/test_gpu_conv_f32_edges.py,
tests/test_gpu_conv_wino_rs_edges.py): sentinel-filled output buffers with guard bytes, bit comparison, and the reading of an
output buffer back into (n, ho, wo, cout) with the checks that go with it."""
import torch

from tests import conv_f32_cases as K
from tests.conv_h16_launch import GUARD, SENT, bits, same_bits        # one source for both type families


def sentinel_buffer(shape):
    """(raw bytes, fp32 view of `shape`): the view filled with the sentinel, 256 guard bytes of 0xA5 behind it."""
    n = 1
    for s in shape:
        n *= s
    raw = torch.full((4 * n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    view = raw[:4 * n].view(torch.float32).view(shape)
    view.fill_(SENT)
    return raw, view


def y_shape(c):
    ho, wo = K.out_hw(c)
    if c["out"] == K.OUT_HEAD:
        return (c["n"], 3, ho, wo, c["cout"] // 3)
    f = 2 if c["out"] == K.OUT_UP else 1
    return (c["n"], f * ho, f * wo, c["y_ld"])


def values(c, y, tile=None):
    """(n, ho, wo, cout) of an output buffer; everything outside the layer's channels must still be the sentinel, the four pixels of
    a 2x upsampling store equal."""
    if c["out"] == K.OUT_HEAD:
        n, _, ho, wo, nc5 = y.shape
        return y.permute(0, 2, 3, 1, 4).reshape(n, ho, wo, 3 * nc5)
    keep = torch.ones(y.shape[-1], dtype=torch.bool)
    keep[c["y_off"]:c["y_off"] + c["cout"]] = False
    assert bool((y[..., keep] == SENT).all()), (c["name"], tile, "channels outside [y_off, y_off + cout) were written")
    v = y[..., c["y_off"]:c["y_off"] + c["cout"]]
    if c["out"] == K.OUT_UP:
        a = v[:, ::2, ::2]
        assert same_bits(a, v[:, 1::2, ::2]) and same_bits(a, v[:, ::2, 1::2]) and same_bits(a, v[:, 1::2, 1::2]), (c["name"], tile)
        v = a
    return v.contiguous()
