"""The drawing contract on the host (no GPU): the numpy restatement (tests/draw_ref.py) against fp64 yardsticks, the font and the
host-only entries of the library, the default palette against matplotlib, the reference's wrappers, and every bad argument of
draw_boxes, which must be refused before a device is touched."""
import numpy as np
import pytest
import torch

from tests import draw_ref as R
from yolo_for_turbines_amd import _lib as L
from yolo_for_turbines_amd import draw as D
from yolo_for_turbines_amd.data import unletterbox_boxes

NEAR = 1e-3              # a box with an edge this close (pixels) to a rounding boundary is left out of the fp64 comparisons
MAX_LEFT_OUT = 0.05


def _font():
    buf = L.C.create_string_buffer(95 * 8)
    L.lib().yolo_draw_font(buf)
    return np.frombuffer(buf.raw, dtype=np.uint8).reshape(95, 8).copy()


def test_blend_formula_is_the_rounded_quotient_for_every_input():
    src = np.arange(256, dtype=np.int64)[:, None]
    col = np.arange(256, dtype=np.int64)[None, :]
    for a in range(256):
        got = R.blend(src, col, a)
        want = np.floor((src * (255 - a) + col * a).astype(np.float64) / 255.0 + 0.5).astype(np.int64)
        assert np.array_equal(got, want), a
    assert np.array_equal(R.blend(src, col, 255), np.broadcast_to(col, (256, 256)))
    assert np.array_equal(R.blend(src, col, 0), np.broadcast_to(src, (256, 256)))


def _rect64(l, t, r, b):
    """fp64 yardstick of the integer box, and how near an edge is to a rounding boundary."""
    es = [min(max(e, -2.0 ** 20), 2.0 ** 20) for e in (l, t, r, b)]
    near = min(abs((e + 0.5) - round(e + 0.5)) for e in es)
    return tuple(int(np.floor(e + 0.5)) for e in es), near


def _compare(rows, h, w, center, to64):
    left_out = 0
    for row in rows:
        want, near = _rect64(*to64(row))
        if near < NEAR:
            left_out += 1
            continue
        assert R.rectangle(row, h, w, center) == want, row
    assert left_out <= MAX_LEFT_OUT * len(rows), left_out
    return left_out


@pytest.mark.parametrize("h,w,seed", [(1080, 1920, 1), (97, 125, 2), (480, 640, 3)])
def test_rectangles_against_fp64(h, w, seed):
    """The fp32 edges carry at most three roundings of 2^-24 relative on values below 1.5 w: under 4e-4 px at w = 1920, inside the
    1e-3 px band that is left out; with uniform edges that band holds 0.8 % of the boxes (four edges x 2e-3)."""
    rng = np.random.default_rng(seed)
    n = 2000
    rows = np.concatenate([rng.uniform(-0.1, 1.1, (n, 2)), rng.uniform(0.0, 0.5, (n, 2)), rng.uniform(0, 1, (n, 2))], 1).astype(np.float32)
    c64 = lambda r: ((float(r[0]) - float(r[2]) / 2) * w, (float(r[1]) - float(r[3]) / 2) * h, (float(r[0]) + float(r[2]) / 2) * w,
                     (float(r[1]) + float(r[3]) / 2) * h)
    _compare(rows, h, w, True, c64)
    corners = rows.copy()
    corners[:, 2:4] = rows[:, :2] + rows[:, 2:4]
    _compare(corners, h, w, False, lambda r: (float(r[0]) * w, float(r[1]) * h, float(r[2]) * w, float(r[3]) * h))


@pytest.mark.parametrize("canvas,meta,seed", [((416, 416), (720, 1280, 234, 416, 91, 0), 4), ((256, 416), (720, 1280, 234, 416, 11, 0), 5),
                                              ((416, 320), (1280, 640, 416, 208, 0, 56), 6)])
def test_unmapping_against_fp64(canvas, meta, seed):
    """fp32 un-mapping then fp32 geometry against unletterbox_boxes(..., meta=) and the geometry in fp64. Three more roundings on
    a normalised coordinate (relative 2^-24 each) reach the frame multiplied by at most 1280: under 8e-4 px together with the
    geometry's own, inside the band that is left out."""
    rng = np.random.default_rng(seed)
    n = 2000
    oh, ow = meta[:2]
    rows = np.concatenate([rng.uniform(0.0, 1.0, (n, 2)), rng.uniform(0.0, 0.4, (n, 2)), rng.uniform(0, 1, (n, 2))], 1).astype(np.float32)

    def to64(row):
        x, y, bw, bh = unletterbox_boxes([[float(v) for v in row]], (oh, ow), canvas, meta=meta)[0][:4]
        return (x - bw / 2) * ow, (y - bh / 2) * oh, (x + bw / 2) * ow, (y + bh / 2) * oh

    left_out = 0
    for row in rows:
        want, near = _rect64(*to64(row))
        if near < NEAR:
            left_out += 1
            continue
        assert R.rectangle(R.unmap(row, meta, canvas, True), oh, ow, True) == want, row
    assert left_out <= MAX_LEFT_OUT * n, left_out


def test_rows_that_draw_nothing():
    for bad in ([np.nan, 0.5, 0.1, 0.1], [0.5, np.inf, 0.1, 0.1], [0.5, 0.5, -0.1, 0.1], [0.5, 0.5, 0.1, -0.2], [0.5, 0.5, np.inf, 0.1]):
        assert R.rectangle(np.array(bad + [1, 0], np.float32), 64, 64) is None, bad
    assert R.rectangle(np.array([1e30, 0.5, 0.1, 0.1, 1, 0], np.float32), 64, 64)[0] == 2 ** 20          # clamped, outside the frame
    assert R.rectangle(np.array([0.5, 0.5, 0.0, 0.0, 1, 0], np.float32), 64, 64) == (32, 32, 32, 32)     # zero-sized: an empty box


def test_ring_is_centred_and_degenerates_to_solid():
    assert R.ring((10, 10, 30, 20), 1) == ((10, 10, 30, 20), (11, 11, 29, 19))
    assert R.ring((10, 10, 30, 20), 4) == ((8, 8, 32, 22), (12, 12, 28, 18))
    assert R.ring((10, 10, 30, 20), 5) == ((8, 8, 32, 22), (13, 13, 27, 17))
    outer, inner = R.ring((10, 10, 30, 20), 10)                        # thicker than half the box: no inner rectangle is left
    assert inner[1] >= inner[3]
    font = _font()
    frame = np.zeros((40, 48, 3), np.uint8)
    box = np.array([[10 / 48, 10 / 40, 30 / 48, 20 / 40, 0.9, 0]], np.float32)
    out = R.draw_frame(frame, box, font, center=False, thickness=10, labels=False, palette=[(9, 8, 7)], fill_alpha=128)
    assert (out[5:25, 5:35] == (9, 8, 7)).all() and out.sum() == 20 * 30 * 24                            # solid, and nothing else
    out = R.draw_frame(frame + 100, box, font, center=False, thickness=2, labels=False, palette=[(200, 0, 50)], fill_alpha=51)
    assert tuple(out[9, 9]) == (200, 0, 50) and tuple(out[10, 10]) == (200, 0, 50) and tuple(out[8, 8]) == (100, 100, 100)
    assert tuple(out[11, 11]) == (120, 80, 90)                         # (100 * 204 + colour * 51 + 127) // 255


def test_plate_placement_and_truncation():
    assert R.plate((20, 30, 60, 50), 4, 1, 100) == (20, 22, 44, 30)    # on the outer rectangle's top-left corner
    assert R.plate((20, 5, 60, 50), 4, 1, 100) == (20, 5, 44, 13)      # would leave the top: moves inside, top at the outer y0
    assert R.plate((20, -3, 60, 50), 4, 1, 100) == (20, -3, 44, 5)     # ... even where that is above the frame (clipped)
    assert R.plate((90, 30, 99, 50), 4, 1, 100) == (76, 22, 100, 30)   # would pass the right edge: shifts left
    assert R.plate((90, 30, 99, 50), 20, 1, 100) == (0, 22, 120, 30)   # ... but never below 0 (then clipped on the right)
    assert R.plate((-7, 30, 40, 50), 4, 2, 100) == (-7, 14, 41, 30)    # a box over the left edge: the plate is clipped there
    cap = L.lib().yolo_draw_text_capacity()
    assert cap == R.TEXT_CAPACITY and cap >= 24
    long = R.label_text("x" * 40, 7, 0.5)
    assert long == "x" * cap
    assert R.label_text("a" * (cap - 4), 123, None) == "a" * (cap - 4) + " #12"
    assert R.label_text("turbine", 12, 0.873) == "turbine #12 87%"
    assert R.label_text("turbine", 0, None) == "turbine" and R.label_text("turbine", -4, None) == "turbine"
    assert R.label_text(None, 3, 1.0) == "#3 100%" and R.label_text(None, None, 0.5) == "50%" and R.label_text("café", None, None) == "caf?"


def test_percent_text():
    got = [R.percent(np.float32(s)) for s in (0, 0.004, 0.005, 0.995, 1, 1.7, -0.1, np.nan)]
    assert got == [0, 0, 1, 100, 100, 100, 0, 0]
    assert [R.label_text(None, None, s) for s in (0.0, 0.07, 0.995)] == ["00%", "07%", "100%"]


def test_font_of_the_library():
    font = _font()
    assert font.shape == (95, 8) and not font[0].any()                 # space is blank
    assert len({bytes(g) for g in font}) == 95                         # all glyphs distinct
    assert not font[:, 7].any() and not (font & 0xE0).any()            # row 7 blank; only bits 4 .. 0 (columns 0 .. 4) are used: column 5 blank
    pixels = np.unpackbits(font, axis=1).reshape(95, -1).sum(1)
    assert (pixels[1:] >= 3).all()


def test_host_only_entries_and_refusals_before_a_launch():
    lib = L.lib()
    tw, th = L.C.c_int(), L.C.c_int()
    lib.yolo_draw_tile(L.C.byref(tw), L.C.byref(th))
    assert tw.value >= 4 and tw.value % 4 == 0 and th.value >= 1 and lib.yolo_draw_chunk() >= 64
    assert lib.yolo_draw_workspace_bytes(3, 10) == 16 + 3 * 10 * 112 and lib.yolo_draw_workspace_bytes(2, 0) == 16
    assert lib.yolo_draw_workspace_bytes(0, 10) == 0 and lib.yolo_draw_workspace_bytes(65536, 1) == 0 and lib.yolo_draw_workspace_bytes(1, -1) == 0
    p = L.DrawParams(1, 1, 255, 0, 1, 1, 0, 0)
    fake = 4096                                                        # never dereferenced: every call below is refused first

    def call(b=1, h=8, w=8, n=1, keep=0, count=0, ids=0, meta=0, canvas=None, params=p, names=0, nc=0, nw=0, pal=fake, k=3, ws=fake, nbytes=1 << 20,
             frames=fake, boxes=fake):
        return lib.yolo_draw_boxes(frames, frames, b, h, w, boxes, n, 1, keep, count, ids, meta, canvas, L.C.byref(params), names, nc, nw, pal, k,
                                   ws, nbytes, None)

    assert call(h=16385) == -2 and call(w=0) == -2 and call(b=0) == -2 and call(b=65536) == -2 and call(n=-1) == -2
    assert call(ws=0) == -2 and call(ws=fake + 4) == -2 and call(nbytes=127) == -2
    assert call(frames=0) == -1 and call(boxes=0) == -1 and call(pal=0) == -1 and call(k=0) == -1
    assert call(keep=fake) == -1 and call(meta=fake) == -1 and call(names=fake, nc=0, nw=4) == -1
    for bad in (L.DrawParams(0, 1, 255, 0, 1, 1, 0, 0), L.DrawParams(65, 1, 255, 0, 1, 1, 0, 0), L.DrawParams(1, 9, 255, 0, 1, 1, 0, 0),
                L.DrawParams(1, 1, 256, 0, 1, 1, 0, 0), L.DrawParams(1, 1, 255, -1, 1, 1, 0, 0), L.DrawParams(1, 1, 255, 0, 1, 1, 1, 0)):
        assert call(params=bad) == -1
    assert call(ws=0) == -2 and b"workspace" in lib.yolo_last_error()


def test_default_palette_is_tab20b():
    import matplotlib
    colours = matplotlib.colormaps["tab20b"].colors
    assert len(colours) == 20
    assert D.TAB20B == tuple(tuple(int(v * 255 + 0.5) for v in c[:3]) for c in colours)
    assert D.default_palette() == D.TAB20B
    cmap = matplotlib.colormaps["tab20b"]
    for n in (1, 2, 3, 7, 20, 21, 80):                                 # the reference: cmap(i) for i in np.linspace(0, 1, n)
        want = tuple(tuple(int(v * 255 + 0.5) for v in cmap(i)[:3]) for i in np.linspace(0, 1, n))
        assert D.default_palette(n) == want, n


def test_default_style_follows_the_reference_inside_the_bounds():
    assert D.default_style(64, 64) == (1, 1) and D.default_style(1080, 1920) == (5, 2) and D.default_style(2160, 3840) == (11, 4)
    assert D.default_style(16384, 16384) == (49, 8)


def test_wrappers_are_exposed_like_soft_nms():
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import utils
    for name in ("plot_original", "plot_image_with_boxes"):
        assert getattr(utils, name) is getattr(D, name) is getattr(yt, name)
        assert name not in utils.__all__ and name not in yt.__all__
    for name in ("draw_boxes", "draw_tracks"):
        assert getattr(yt, name) is getattr(D, name) and name not in yt.__all__ and not hasattr(utils, name)
    image = np.zeros((8, 8, 3), np.uint8)
    assert D.plot_image_with_boxes(image, [], ["a"]) is image           # as the reference: unchanged, before any device is touched
    assert D.plot_original(image, np.zeros((4, 4, 3), np.uint8), [], ["a"]) is image


def test_bad_arguments_raise_before_a_device_is_touched():
    """CPU tensors throughout: a ValueError names the argument; only a call that is otherwise right reaches the device check."""
    fr = torch.zeros((2, 8, 12, 3), dtype=torch.uint8)
    bx = torch.zeros((2, 5, 6))
    keep = torch.zeros((2, 5), dtype=torch.int32)
    count = torch.zeros((2,), dtype=torch.int32)
    ids = torch.zeros((2, 5), dtype=torch.int32)
    ok = dict(frames=fr, boxes=bx)
    bad = [
        (dict(frames=fr.float()), "frames must be a uint8"), (dict(frames=fr[..., :2]), "frames must be a uint8"),
        (dict(frames=fr[0, 0]), "frames must be a uint8"), (dict(frames=np.zeros((8, 8, 3), np.uint8)), "frames must be a uint8"),
        (dict(frames=[]), "a list of frames"), (dict(frames=[fr[0], fr[1]], boxes=bx[:1]), "for a list of 2 frames"),
        (dict(boxes=bx.long()), "boxes must be a floating-point"), (dict(boxes=bx[..., :5]), "boxes must be a floating-point"),
        (dict(boxes=bx[0]), "boxes must be a floating-point"), (dict(boxes=bx[:1]), "boxes of 1 frames, 2 frames"),
        (dict(keep=keep), "keep needs count"), (dict(keep=keep[:, :4], count=count), "keep must be an integer tensor of shape (2, 5)"),
        (dict(keep=keep.float(), count=count), "keep must be an integer tensor"), (dict(count=count[:1]), "count must be an integer tensor of shape (2,)"),
        (dict(count=[1, 2]), "count must be an integer tensor"), (dict(ids=ids[:, :3]), "ids must be an integer tensor of shape (2, 5)"),
        (dict(ids=ids.bool()), "ids must be an integer tensor"),
        (dict(box_format="xyxy"), "box_format must be 'center' or 'corners'"), (dict(color_by="track"), "color_by must be 'class' or 'id'"),
        (dict(color_by="id"), "color_by='id' needs ids"),
        (dict(thickness=0), "thickness must be an integer in [1, 64]"), (dict(thickness=65), "thickness must be an integer in [1, 64]"),
        (dict(thickness=2.0), "thickness must be an integer"), (dict(thickness=True), "thickness must be an integer"),
        (dict(font_scale=0), "font_scale must be an integer in [1, 8]"), (dict(font_scale=9), "font_scale must be an integer in [1, 8]"),
        (dict(fill_alpha=1.5), "fill_alpha must be a number in [0, 1]"), (dict(fill_alpha=-0.1), "fill_alpha must be a number in [0, 1]"),
        (dict(line_alpha=float("nan")), "line_alpha must be a number in [0, 1]"), (dict(line_alpha="x"), "line_alpha must be a number in [0, 1]"),
        (dict(class_names=[]), "class_names must be a non-empty sequence of strings"), (dict(class_names="turbine"), "class_names must be"),
        (dict(class_names=["a", 3]), "class_names must be"),
        (dict(palette=[]), "palette must be a uint8 (K, 3) table"), (dict(palette=[(1, 2)]), "palette must be a uint8 (K, 3) table"),
        (dict(palette=[(1, 2, 256)]), "palette must be a uint8 (K, 3) table"), (dict(palette=torch.zeros((2, 3))), "palette must be a uint8 (K, 3) table"),
        (dict(meta=[(1, 1, 1, 1, 0, 0)] * 2), "meta must be (table, (canvas_h, canvas_w))"),
        (dict(meta=([(1, 1, 1, 1, 0, 0)], (8, 8))), "meta: the table must hold 2 tuples of 6 integers"),
        (dict(meta=([(1, 1, 1, 1, 0)] * 2, (8, 8))), "meta: the table must hold 2 tuples of 6 integers"),
        (dict(meta=([(1, 1, 1, 1, 0, 0)] * 2, (0, 8))), "meta: canvas size (0, 8) must be positive"),
        (dict(meta=(torch.zeros((2, 6)), (8, 8))), "meta: the table must be an int32 tensor of shape (2, 6)"),
        (dict(frames=fr.permute(0, 2, 1, 3), boxes=bx, inplace=True), "inplace needs contiguous frames"),
    ]
    for kw, text in bad:
        args = dict(ok, **kw)
        with pytest.raises(ValueError) as e:
            D.draw_boxes(args.pop("frames"), args.pop("boxes"), args.pop("keep", None), args.pop("count", None), **args)
        assert text in str(e.value), (kw.keys(), str(e.value))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.draw_boxes(fr, bx, keep, count, ids=ids, class_names=["a"], meta=([(8, 12, 8, 12, 0, 0)] * 2, (8, 12)))
    with pytest.raises(ValueError, match="result must be a TrackResult"):
        D.draw_tracks(fr, (bx, ids, count))
