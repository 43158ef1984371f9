"""yolo_split3_weight_bytes on the host (no launch): the size formula of include/yolo_mi355x.h, and 0 where
yolo_conv_split3_supported says no."""
import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def _desc(L, cout, cin, k, s, dtype=None, h=13):
    return L.ConvDesc(n=2, h=h, w=h, cin=cin, cout=cout, ksize=k, stride=s, x_ld=(cin + 3) // 4 * 4, y_ld=cout,
                      dtype=L.F32 if dtype is None else dtype)


@pytest.mark.parametrize("cout,cin,k,s", [(24, 96, 1, 1), (255, 1024, 1, 1), (256, 128, 3, 2)])
def test_weight_bytes_is_the_documented_formula(built, cout, cin, k, s):
    """The packed weights rounded up to 16 bytes, K_pad32 / 32 K steps of three planes of cout_pad128 rows of 64 bytes, then one
    32-bit word per 32 padded output channels; flags, tile and batch of the descriptor do not matter."""
    L = built
    lib = L.lib()
    d = _desc(L, cout, cin, k, s)
    assert lib.yolo_conv_split3_supported(d) == 1
    cp = (cout + 127) // 128 * 128
    kpad = (k * k * cin + 31) // 32 * 32
    front = (lib.yolo_packed_weight_bytes(cout, cin, k, L.F32) + 15) // 16 * 16
    want = front + kpad // 32 * 3 * cp * 64 + cp // 32 * 4
    assert lib.yolo_split3_weight_bytes(d) == want
    assert want - front == 6 * cp * kpad + cp // 8              # the planes: 6 bytes per weight of the padded matrix
    d.flags, d.tile, d.n = L.FLAG_SPLIT_BF16 | L.FLAG_SPLIT_WEIGHTS_READY, 2, 32
    assert lib.yolo_split3_weight_bytes(d) == want


def test_weight_bytes_is_zero_where_the_split_flag_is_not_honoured(built):
    """The stem shape, cin that is no multiple of 32, 16-bit descriptors, and a 3x3 stride-1 layer of the Winograd families
    (a tile-0 launch that brings its workspace does not run on the direct kernels)."""
    L = built
    lib = L.lib()
    for d in (_desc(L, 32, 3, 3, 1), _desc(L, 64, 48, 1, 1), _desc(L, 64, 32, 1, 1, dtype=L.BF16), _desc(L, 64, 32, 1, 1, dtype=L.F16),
              _desc(L, 256, 128, 3, 1, h=52)):
        assert lib.yolo_conv_split3_supported(d) == 0
        assert lib.yolo_split3_weight_bytes(d) == 0
    assert lib.yolo_split3_weight_bytes(None) == 0
