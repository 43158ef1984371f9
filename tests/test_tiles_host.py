"""Tiled detection on the host (nothing is launched): the grid rule of yolo_tile_grid against a restatement written here, its error
codes, the workspace size of yolo_tile_collect, the return code of a call whose workspace is too small, and the argument errors of
detect_tiled."""
import ctypes as C

import numpy as np
import pytest

OK, ERR_ARG, ERR_UNSUPPORTED, ERR_LAUNCH, ERR_WORKSPACE = 0, -1, -2, -3, -4
FAKE = 1 << 20          # a non-null "device pointer" for calls that must return before they launch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def axis_rule(L, t, o):
    """The rule of include/yolo_mi355x.h for one axis: length L, tile t, overlap o, stride s = t - o."""
    if L <= t:
        return [0]
    s = t - o
    n = -(-(L - t) // s) + 1
    return [k * s for k in range(n - 1)] + [L - t]


def grid_rule(h, w, th, tw, oh, ow):
    return [[y, x] for y in axis_rule(h, th, oh) for x in axis_rule(w, tw, ow)]


def lib_grid(lib, h, w, th, tw, oh, ow):
    n = lib.yolo_tile_grid(h, w, th, tw, oh, ow, None, 0)
    assert n > 0
    buf = (C.c_int32 * (2 * n))()
    assert lib.yolo_tile_grid(h, w, th, tw, oh, ow, buf, n) == n
    return np.array(list(buf)).reshape(n, 2).tolist()


# (t, o): square and the sides of rectangular tiles, overlap 0, a usual one, and t - 1
AXES = [(96, 24), (64, 0), (64, 16), (32, 31), (416, 83)]


def axis_lengths(t, o):
    """L < t, L == t, L == t + 1, (L - t) an exact multiple of the stride, one more than a multiple."""
    s = t - o
    return [1, t - 1, t, t + 1, t + s, t + 3 * s, t + 3 * s + 1, t + 2 * s - 1]


def test_axis_rule_is_what_the_issue_states():
    assert axis_rule(45, 64, 16) == [0] and axis_rule(64, 64, 16) == [0]
    assert axis_rule(65, 64, 16) == [0, 1]                                   # L == t + 1: the second tile is flush with the edge
    assert axis_rule(64 + 96, 64, 16) == [0, 48, 96]                          # an exact multiple of the stride
    assert axis_rule(64 + 97, 64, 16) == [0, 48, 96, 97]                      # one more
    assert axis_rule(150, 64, 16) == [0, 48, 86] and axis_rule(203, 96, 32) == [0, 64, 107]


@pytest.mark.parametrize("ty,oy", AXES)
@pytest.mark.parametrize("tx,ox", AXES)
def test_tile_grid_equals_the_rule(built, ty, oy, tx, ox):
    """Both axes independently, every pairing of tile sides (so rectangular tiles too) and of the five kinds of length."""
    lib = built.lib()
    for h in axis_lengths(ty, oy):
        for w in axis_lengths(tx, ox):
            want = grid_rule(h, w, ty, tx, oy, ox)
            assert lib_grid(lib, h, w, ty, tx, oy, ox) == want, (h, w)
            ys, xs = {r[0] for r in want}, {r[1] for r in want}
            assert max(ys) + ty >= h and max(xs) + tx >= w                   # the tiles cover the image ...
            assert h <= ty or max(ys) + ty == h                              # ... and an image larger than a tile gets no padding
            assert w <= tx or max(xs) + tx == w


def test_full_frame_count_and_python_wrapper(built):
    import yolo_for_turbines_amd as yt
    lib = built.lib()
    assert lib.yolo_tile_grid(3648, 5472, 416, 416, 83, 83, None, 0) == 11 * 17
    g = yt.tile_grid(3648, 5472)                                             # tile 416, overlap 0.2 -> 83 pixels
    assert tuple(g.shape) == (187, 2) and str(g.dtype) == "torch.int32"
    assert g.tolist() == grid_rule(3648, 5472, 416, 416, 83, 83)
    assert yt.tile_grid(150, 203, (64, 96), (16, 32)).tolist() == grid_rule(150, 203, 64, 96, 16, 32)
    assert yt.tile_grid(150, 203, 96, 0.25).tolist() == grid_rule(150, 203, 96, 96, 24, 24)
    assert yt.tile_grid(150, 203, 100, 0).tolist() == grid_rule(150, 203, 100, 100, 0, 0)      # the grid takes any tile size
    with pytest.raises(ValueError):
        yt.tile_grid(150, 203, 64, 1.0)


def test_tile_grid_return_codes(built):
    lib = built.lib()
    n = lib.yolo_tile_grid(150, 203, 64, 96, 16, 32, None, 0)
    assert n == 9
    assert lib.yolo_tile_grid(150, 203, 64, 96, 16, 32, None, -5) == n       # NULL: the count, whatever cap says
    buf = (C.c_int32 * (2 * n))(*([-7] * (2 * n)))
    assert lib.yolo_tile_grid(150, 203, 64, 96, 16, 32, buf, n - 1) == ERR_ARG
    assert list(buf) == [-7] * (2 * n) and b"tile_grid" in lib.yolo_last_error()
    for bad in ((150, 203, 64, 96, 64, 32), (150, 203, 64, 96, 16, 96), (150, 203, 64, 96, -1, 0), (150, 203, 64, 96, 0, -1),
                (0, 203, 64, 96, 0, 0), (150, -3, 64, 96, 0, 0), (150, 203, 0, 96, 0, 0), (150, 203, 64, 0, 0, 0)):
        assert lib.yolo_tile_grid(*bad, None, 0) == ERR_ARG, bad
        assert lib.yolo_tile_grid(*bad, buf, n) == ERR_ARG, bad


def test_collect_workspace_bytes(built):
    lib = built.lib()
    f = lib.yolo_tile_collect_workspace_bytes
    assert f(1, 1) > 0 and f(32, 10647) > 0
    for n_per in (1, 507, 10647, 22743):
        sizes = [f(t, n_per) for t in (1, 2, 7, 32, 187)]
        assert sizes == sorted(sizes) and sizes[0] > 0
    for t in (1, 6, 32):
        sizes = [f(t, n_per) for n_per in (1, 1023, 1024, 1025, 10647, 22743, 1 << 20)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert f(1 << 16, 1 << 30) > 2 ** 32 and f(1 << 16, 1 << 30) >= 2 * f(1 << 15, 1 << 30)     # a 64-bit value


def test_collect_refuses_a_small_workspace_before_launching(built):
    lib = built.lib()
    need = lib.yolo_tile_collect_workspace_bytes(6, 10647)

    def call(ws, ws_bytes):
        return lib.yolo_tile_collect(FAKE, 6, 10647, FAKE, FAKE, 2, 96, 96, 0.5, FAKE, 1000, FAKE, ws, ws_bytes, None)
    assert call(FAKE, need - 1) == ERR_WORKSPACE
    assert b"tile_collect" in lib.yolo_last_error()
    assert call(None, need) == ERR_WORKSPACE and call(FAKE, 0) == ERR_WORKSPACE
    assert lib.yolo_tile_collect(None, 6, 10647, FAKE, FAKE, 2, 96, 96, 0.5, FAKE, 1000, FAKE, FAKE, need, None) == ERR_ARG
    assert lib.yolo_tile_collect(FAKE, 6, 10647, FAKE, FAKE, 0, 96, 96, 0.5, FAKE, 1000, FAKE, FAKE, need, None) == ERR_ARG
    assert lib.yolo_tile_gather(None, 45, 70, FAKE, 1, 64, 96, FAKE, None) == ERR_ARG
    assert lib.yolo_tile_gather(FAKE, 45, 70, FAKE, 70000, 64, 96, FAKE, None) == ERR_UNSUPPORTED


def test_detect_tiled_argument_errors_need_no_gpu(built):
    """Raised before the model or the device is looked at."""
    import yolo_for_turbines_amd as yt
    img = np.zeros((40, 50, 3), np.uint8)
    with pytest.raises(ValueError, match="multiples of 32"):
        yt.detect_tiled(None, img, None, tile=100)
    with pytest.raises(ValueError, match="multiples of 32"):
        yt.detect_tiled(None, img, None, tile=(96, 100))
    with pytest.raises(ValueError, match="obj_threshold"):
        yt.detect_tiled(None, img, None, tile=96, obj_threshold=-0.1)
    with pytest.raises(ValueError, match="obj_threshold"):
        yt.detect_tiled(None, img, None, tile=96, obj_threshold=float("nan"))
    with pytest.raises(ValueError, match="batch"):
        yt.detect_tiled(None, img, None, tile=96, batch=0)
    with pytest.raises(ValueError, match="overlap"):
        yt.detect_tiled(None, img, None, tile=96, overlap=(96, 0))
    with pytest.raises(ValueError, match="uint8"):
        yt.detect_tiled(None, img.astype(np.float32), None, tile=96)
