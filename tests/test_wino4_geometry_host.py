"""The size queries of the Winograd F(4x4) family against closed forms written out here (host only: no launch). Every one of them
reads the one launch geometry of conv_wino4_f32.hip (``Wino4Geom``); the workspace layout and the buffers of the engine depend on
these numbers staying what they are."""
import itertools

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def _up(a, b):
    return (a + b - 1) // b * b


def test_size_queries_against_closed_forms(built):
    """T = n ceil(h/4) ceil(w/4), Tpad = T up to 64, C4p = cin/4 up to 2, cp = cout up to 64; a piece of the bf16 planes is 12288
    bytes (3 planes x 64 rows x 64 bytes). One tile, partial tiles on either edge, an odd number of channel quads (the padding plane),
    partial and several tile and channel blocks, cin with and without whole chunks of 32."""
    L = built
    lib = L.lib()
    cases = 0
    for n, h, w, cin, cout in itertools.product((1, 2, 3, 32, 33), (4, 7, 9, 13, 19, 24, 26, 52, 104), (4, 9, 13, 26, 52),
                                                (4, 8, 12, 32, 36, 64, 96, 160, 512), (4, 60, 64, 80, 1024)):
        d = L.ConvDesc(n=n, h=h, w=w, cin=cin, cout=cout, ksize=3, stride=1, x_ld=cin, y_ld=cout, act=L.ACT_LEAKY, out_mode=L.OUT_NHWC,
                       dtype=L.F32, flags=0, tile=15)
        case = (n, h, w, cin, cout)
        T = n * ((h + 3) // 4) * ((w + 3) // 4)
        Tpad, C4p, cp = _up(T, 64), _up(cin // 4, 2), _up(cout, 64)
        fb = 36 * C4p * cp * 16
        f32_ws = 36 * C4p * (Tpad + cp) * 16
        assert lib.yolo_wino4_filter_bytes(d) == fb, case
        assert lib.yolo_conv_workspace_bytes(d) == f32_ws, case
        assert lib.yolo_wino4_appended_bytes(d) - fb == _up(lib.yolo_packed_weight_bytes(cout, cin, 3, L.F32), 16), case
        split = cin % 32 == 0
        assert lib.yolo_wino4_filter_plane_bytes(d) == (36 * (cin // 32) * (cp // 64) * 12288 if split else 0), case
        d.flags = L.FLAG_FILTERS_READY | L.FLAG_WINO_SPLIT_BF16
        assert lib.yolo_conv_workspace_bytes(d) == (36 * (cin // 32) * (Tpad // 64 + cp // 64) * 12288 if split else f32_ws), case
        cases += 1
    assert cases == 5 * 9 * 5 * 9 * 5


@pytest.mark.parametrize("change", [dict(cin=66, x_ld=68), dict(cout=66, y_ld=68), dict(ksize=1), dict(stride=2), dict(dtype="BF16"),
                                    dict(out_mode="OUT_UPSAMPLE2X"), dict(x_ld=130), dict(y_off=2)],
                         ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_filter_size_queries_refuse(built, change):
    """What tile 15 cannot run has no filter buffers: 0 from all three queries."""
    L = built
    lib = L.lib()
    a = dict(n=2, h=24, w=24, cin=128, cout=64, ksize=3, stride=1, x_ld=128, y_ld=64, act=L.ACT_LEAKY, out_mode=L.OUT_NHWC, dtype=L.F32,
             flags=0, tile=15)
    a.update({k: getattr(L, v) if isinstance(v, str) else v for k, v in change.items()})
    d = L.ConvDesc(**a)
    assert (lib.yolo_wino4_filter_bytes(d), lib.yolo_wino4_appended_bytes(d), lib.yolo_wino4_filter_plane_bytes(d)) == (0, 0, 0)


def test_base_descriptor_of_the_refusals_is_accepted(built):
    """... so that each refusal above is the one changed field's."""
    L = built
    lib = L.lib()
    d = L.ConvDesc(n=2, h=24, w=24, cin=128, cout=64, ksize=3, stride=1, x_ld=128, y_ld=64, act=L.ACT_LEAKY, out_mode=L.OUT_NHWC, dtype=L.F32,
                   flags=0, tile=15)
    assert lib.yolo_wino4_filter_bytes(d) == 36 * 32 * 64 * 16
    assert lib.yolo_wino4_filter_plane_bytes(d) == 36 * 4 * 1 * 12288
    assert lib.yolo_wino4_appended_bytes(d) > lib.yolo_wino4_filter_bytes(d)
