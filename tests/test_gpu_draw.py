"""yolo_draw_boxes / draw_boxes on the GPU, bit for bit against the numpy restatement of its contract (tests/draw_ref.py): frames
and workspaces live in 0xA5-filled buffers with guard bytes before and behind them; the cases are placed from the tile and the chunk
the library reports (yolo_draw_tile, yolo_draw_chunk), so that they cross tile corners, partial tiles, the byte path and the chunk
loop whatever the library chose. Then the Python layer: tracks, lists of frames, letterbox meta, the detector end to end, one
captured replay, and the reference's wrappers."""
import numpy as np
import pytest
import torch

from tests import draw_ref as R
from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu
GUARD = 4096             # guard bytes before and behind every buffer the call writes
NAMES = ["turbine", "blade", "a-name-that-is-longer-than-the-record's-capacity", "x", "Tower 2"]
PALETTE3 = [(255, 0, 0), (0, 200, 40), (10, 20, 250)]


@pytest.fixture(scope="module")
def L():
    import yolo_for_turbines_amd  # noqa: F401
    from yolo_for_turbines_amd import _lib
    _lib.lib()                       # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd
    return yolo_for_turbines_amd


@pytest.fixture(scope="module")
def geo(L):
    tw, th = L.C.c_int(), L.C.c_int()
    L.lib().yolo_draw_tile(L.C.byref(tw), L.C.byref(th))
    return tw.value, th.value, L.lib().yolo_draw_chunk()


@pytest.fixture(scope="module")
def font(L):
    buf = L.C.create_string_buffer(95 * 8)
    L.lib().yolo_draw_font(buf)
    return np.frombuffer(buf.raw, dtype=np.uint8).reshape(95, 8).copy()


def guarded(nbytes, offset=0):
    """A 0xA5-filled device buffer with guards; returns (whole buffer, the view of nbytes at GUARD + offset)."""
    whole = torch.full((GUARD + offset + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD + offset:GUARD + offset + nbytes]


def guards_intact(whole, offset, nbytes):
    return bool((whole[:GUARD + offset] == 0xA5).all()) and bool((whole[GUARD + offset + nbytes:] == 0xA5).all())


def name_table(names):
    width = (max(len(s) for s in names) + 3) // 4 * 4
    return torch.tensor([list(s.encode().ljust(width, b"\0")) for s in names], dtype=torch.uint8).cuda(), width


def run_c(L, frames, boxes, *, keep=None, count=None, ids=None, meta=None, canvas_hw=None, class_names=None, palette=PALETTE3, center=True,
          thickness=1, font_scale=1, line_alpha=255, fill_alpha=0, labels=True, scores=True, color_by_id=False, inplace=False, offset=0):
    """yolo_draw_boxes on numpy inputs (keyword names are draw_ref.draw_batch's); checks every guard; returns the drawn frames."""
    B, H, W, _ = frames.shape
    N = boxes.shape[1]
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    out_whole, out = guarded(frames.size, offset)
    if inplace:
        out.copy_(torch.from_numpy(frames).reshape(-1))
        src_whole, src = out_whole, out
    else:
        src_whole, src = guarded(frames.size, offset)
        src.copy_(torch.from_numpy(frames).reshape(-1))
    nbytes = L.lib().yolo_draw_workspace_bytes(B, N)
    assert nbytes == 16 * ((4 * B + 15) // 16) + 112 * B * N
    ws_whole, ws = guarded(nbytes)
    t_boxes, t_keep, t_count, t_ids, t_meta = dev(boxes, torch.float32), dev(keep, torch.int32), dev(count, torch.int32), dev(ids, torch.int32), \
        dev(meta, torch.int32)
    names_t, width = name_table(class_names) if class_names is not None else (None, 0)
    pal = torch.tensor(palette, dtype=torch.uint8).cuda()
    params = L.DrawParams(thickness, font_scale, line_alpha, fill_alpha, int(labels), int(scores), int(color_by_id), 0)
    chw = (L.C.c_int32 * 2)(*canvas_hw) if canvas_hw is not None else None
    L.check(L.lib().yolo_draw_boxes(src.data_ptr(), out.data_ptr(), B, H, W, L.ptr(t_boxes), N, int(center), L.ptr(t_keep), L.ptr(t_count),
                                    L.ptr(t_ids), L.ptr(t_meta), chw, L.C.byref(params), L.ptr(names_t), len(class_names or ()), width,
                                    pal.data_ptr(), len(palette), ws.data_ptr(), nbytes, L.current_stream()), "yolo_draw_boxes")
    torch.cuda.synchronize()
    assert guards_intact(out_whole, offset, frames.size) and guards_intact(ws_whole, 0, nbytes)
    if not inplace:
        assert guards_intact(src_whole, offset, frames.size) and np.array_equal(src.cpu().numpy().reshape(frames.shape), frames)   # the source is only read
    return out.cpu().numpy().reshape(frames.shape)


def check(L, font, frames, boxes, aligned_twin=False, **kw):
    """Out of place against the restatement; in place equals out of place; untouched pixels keep their bytes."""
    kw.setdefault("palette", PALETTE3)
    want = R.draw_batch(frames, boxes, font, **kw)
    got = run_c(L, frames, boxes, **kw)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(run_c(L, frames, boxes, inplace=True, **kw), want)
    if aligned_twin:                                                   # the same pixels from a base pointer that is not 4-byte aligned: the byte path
        assert frames.shape[2] % 4 == 0
        np.testing.assert_array_equal(run_c(L, frames, boxes, offset=1, **kw), want)
        np.testing.assert_array_equal(run_c(L, frames, boxes, offset=2, inplace=True, **kw), want)
    return want


def rand_frames(seed, b, h, w):
    return np.random.default_rng(seed).integers(0, 256, (b, h, w, 3), dtype=np.uint8)


def px_boxes(rects, h, w, center=True):
    """Rows from pixel rectangles (x0, y0, x1, y1, score, cls)."""
    rows = []
    for x0, y0, x1, y1, score, cls in rects:
        if center:
            rows.append([(x0 + x1) / 2 / w, (y0 + y1) / 2 / h, (x1 - x0) / w, (y1 - y0) / h, score, cls])
        else:
            rows.append([x0 / w, y0 / h, x1 / w, y1 / h, score, cls])
    return np.array(rows, dtype=np.float32)


def hand_rects(h, w, tw, th):
    """The boxes of the issue, placed from the tile: (x0, y0, x1, y1, score, cls) in pixels, and their ids."""
    cx, cy = (tw if w > tw else w // 2), (th if h > th else h // 2)
    rects = [
        (cx - 9, cy - 7, cx + 11, cy + 6, 0.91, 0),                    # straddles a tile corner (or the middle of a one-tile frame)
        (max(tw - 30, 1), 3, min(tw, w), 14, 0.5, 1),                  # ends exactly on a tile edge
        (-12, h // 2 - 5, 9, h // 2 + 6, 0.07, 4),                     # partly outside, over the left edge: its plate is clipped there
        (w - 14, h - 9, w + 20, h + 30, 1.0, 3),                       # partly outside at the bottom right
        (w + 5, 4, w + 40, 20, 0.9, 0),                                # wholly outside
        (-50, -50, -3, -3, 0.9, 1),                                    # wholly outside
        (w // 3, h // 3, w // 3, h // 3, 0.8, 0),                      # zero-sized
        (w // 2, 2, w // 2 + 25, 12, 0.995, 2),                        # plate would leave the top; the name is longer than the capacity
        (w - 16, h // 2, w - 4, h // 2 + 10, 0.004, 4),                # plate would pass the right edge
        (5, h - 12, 11, h - 6, 0.33, 3),                               # small: a thick outline leaves no inner rectangle
        (20, 16, 50, 30, 0.6, 7),                                      # a class outside the name table
        (22, 18, 48, 28, 1.7, -1),                                     # ... and a negative one
        (w // 2 - 20, h // 2 - 4, w // 2 + 2, h // 2 + 9, -0.1, 1),
    ]
    ids = [3, 0, -2, 12345, 1, 1, 7, 41, 2, 1000000007, 5, 6, 0]
    return rects, ids


def hand_case(h, w, tw, th, center=True):
    rects, ids = hand_rects(h, w, tw, th)
    rows = px_boxes(rects, h, w, center)
    bad = np.array([[np.nan, 0.5, 0.2, 0.2, 0.9, 0], [0.5, np.inf, 0.2, 0.2, 0.9, 0], [1e30, 0.5, 0.2, 0.2, 0.9, 1], [0.5, 0.5, 0.2, 0.2, np.nan, np.nan]],
                   dtype=np.float32)
    neg = np.array([[0.5, 0.5, -0.2, 0.2, 0.9, 0]] if center else [[0.6, 0.2, 0.4, 0.5, 0.9, 0]], dtype=np.float32)        # negative width
    rows = np.concatenate([rows[:5], bad, neg, rows[5:]])
    ids = np.array(ids[:5] + [9, 9, 9, 9, 9] + ids[5:], dtype=np.int32)
    return rows, ids


def styles():
    from yolo_for_turbines_amd.draw import default_palette
    return {
        "thin_names_class": dict(thickness=1, font_scale=1, class_names=NAMES, palette=default_palette(len(NAMES))),
        "thick_translucent_by_id": dict(thickness=3, font_scale=2, class_names=NAMES, palette=PALETTE3, color_by_id=True, line_alpha=200, fill_alpha=77),
        "solid_no_labels": dict(thickness=8, labels=False, palette=PALETTE3, fill_alpha=255),
        "ids_and_scores_without_names": dict(thickness=2, font_scale=1, palette=PALETTE3, scores=True),
        "names_only": dict(thickness=2, font_scale=3, class_names=NAMES, palette=PALETTE3, scores=False),
    }


FRAMES = ("one_tile", "byte_path_partial_tiles", "batch_of_three")


def frame_shape(name, tw, th):
    return {"one_tile": (1, th, tw), "byte_path_partial_tiles": (1, th + 5, tw - 3), "batch_of_three": (3, 2 * th + 1, 2 * tw + 2)}[name]


@pytest.mark.parametrize("style", ["thin_names_class", "thick_translucent_by_id", "solid_no_labels", "ids_and_scores_without_names", "names_only"])
@pytest.mark.parametrize("shape", FRAMES)
@pytest.mark.parametrize("center", [True, False])
def test_hand_boxes(L, geo, font, shape, style, center):
    tw, th, _ = geo
    b, h, w = frame_shape(shape, tw, th)
    assert (3 * (tw - 3)) % 4 != 0
    frames = rand_frames(1, b, h, w)
    rows, ids = hand_case(h, w, tw, th, center)
    boxes = np.stack([np.roll(rows, 3 * k, axis=0) for k in range(b)])
    idt = np.stack([np.roll(ids, 3 * k) for k in range(b)])
    kw = dict(styles()[style], center=center)
    with_ids = style != "names_only"
    count = np.array([len(rows), 0, 7], dtype=np.int32)[:b] if b == 3 else None       # different counts per frame, one of them 0
    want = check(L, font, frames, boxes, aligned_twin=(w % 4 == 0), ids=idt if with_ids else None, count=count, **kw)
    assert not np.array_equal(want[0], frames[0])
    if b == 3:
        np.testing.assert_array_equal(want[1], frames[1])
    touched = np.zeros((h, w), dtype=bool)
    R.draw_frame(frames[0], boxes[0], font, ids=idt[0] if with_ids else None, touched=touched, **kw)
    assert touched.any() and (style != "thin_names_class" or not touched.all())
    np.testing.assert_array_equal(want[0][~touched], frames[0][~touched])


def test_three_selection_modes(L, geo, font):
    tw, th, _ = geo
    b, h, w = frame_shape("batch_of_three", tw, th)
    frames = rand_frames(2, b, h, w)
    rows, ids = hand_case(h, w, tw, th)
    n = len(rows)
    boxes = np.stack([rows, rows[::-1], np.roll(rows, 5, axis=0)])
    idt = np.stack([ids, ids[::-1], np.roll(ids, 5)])
    rng = np.random.default_rng(3)
    keep = np.stack([rng.permutation(n) for _ in range(b)]).astype(np.int32)
    keep[0, 1], keep[2, 0] = -1, n                                       # indices outside [0, n) draw nothing
    kw = dict(styles()["thick_translucent_by_id"], ids=idt)
    results = [check(L, font, frames, boxes, keep=keep, count=np.array([n, 4, 0], np.int32), **kw),
               check(L, font, frames, boxes, keep=keep, count=np.array([n + 9, -3, 2], np.int32), **kw),       # clamped to [0, n]
               check(L, font, frames, boxes, count=np.array([5, n, 0], np.int32), **kw),
               check(L, font, frames, boxes, **kw)]
    assert not np.array_equal(results[0], results[2]) and not np.array_equal(results[2], results[3])
    np.testing.assert_array_equal(results[0][2], frames[2])


def test_no_boxes(L, geo, font):
    tw, th, _ = geo
    frames = rand_frames(4, 2, th + 5, tw - 3)
    want = check(L, font, frames, np.zeros((2, 0, 6), np.float32), class_names=NAMES)
    np.testing.assert_array_equal(want, frames)
    np.testing.assert_array_equal(check(L, font, frames, np.zeros((2, 0, 6), np.float32), count=np.array([0, 0], np.int32)), frames)


def test_painters_order_of_two_translucent_boxes(L, geo, font):
    tw, th, _ = geo
    h, w = th, tw
    frames = rand_frames(5, 1, h, w)
    a = px_boxes([(10, 4, 60, 26, 0.9, 0), (30, 10, 90, 30, 0.8, 1)], h, w)
    kw = dict(thickness=3, palette=PALETTE3, line_alpha=160, fill_alpha=90, labels=False)
    ab = check(L, font, frames, a[None], **kw)
    ba = check(L, font, frames, a[None, ::-1], **kw)
    assert not np.array_equal(ab, ba)
    ab_keep = check(L, font, frames, a[None], keep=np.array([[1, 0]], np.int32), count=np.array([2], np.int32), **kw)
    np.testing.assert_array_equal(ab_keep, ba)                         # the order is the selection order, not the row order


@pytest.mark.parametrize("which", ["below", "exact", "above", "two_chunks_and_one"])
def test_chunk_loop(L, geo, font, which):
    tw, th, chunk = geo
    n = {"below": chunk - 1, "exact": chunk, "above": chunk + 1, "two_chunks_and_one": 2 * chunk + 1}[which]
    rng = np.random.default_rng(n)
    x0, y0 = rng.integers(-4, tw, n), rng.integers(-4, th, n)
    rects = [(x0[i], y0[i], x0[i] + rng.integers(0, 24), y0[i] + rng.integers(0, 12), rng.uniform(0, 1), rng.integers(0, 3)) for i in range(n)]
    rects[-1] = (10, 5, 40, 20, 0.5, 1)                                # the last command, alone in the last chunk for chunk + 1 and 2 chunk + 1
    boxes = px_boxes(rects, th, tw)[None]
    frames = rand_frames(6, 1, th, tw)
    kw = dict(thickness=1, palette=PALETTE3, line_alpha=190, fill_alpha=40)
    want = check(L, font, frames, boxes, **kw)
    assert not np.array_equal(want, R.draw_batch(frames, boxes, font, count=np.array([n - 1]), **kw))      # without it the picture differs


@pytest.mark.parametrize("canvas,center", [((416, 416), True), ((256, 416), True), ((416, 320), False)])
def test_meta_unmapping(L, geo, font, canvas, center):
    """Boxes normalised to a letterboxed canvas, drawn on the original frames: two frames with different letterboxes."""
    tw, th, _ = geo
    h, w = th + 9, tw + 6
    ch, cw = canvas
    scale = min(ch / h, cw / w)
    nh, nw = max(int(round(h * scale)), 1), max(int(round(w * scale)), 1)
    meta = np.array([[h, w, nh, nw, (ch - nh) // 2, (cw - nw) // 2], [h, w, nh - 7, nw - 3, 5, 11]], dtype=np.int32)
    rng = np.random.default_rng(7)
    n = 24
    if center:
        rows = np.concatenate([rng.uniform(0, 1, (2, n, 2)), rng.uniform(0, 0.3, (2, n, 2)), rng.uniform(0, 1, (2, n, 1)), rng.integers(0, 5, (2, n, 1))], 2)
    else:
        p = rng.uniform(0, 1, (2, n, 2))
        rows = np.concatenate([p, p + rng.uniform(0, 0.3, (2, n, 2)), rng.uniform(0, 1, (2, n, 1)), rng.integers(0, 5, (2, n, 1))], 2)
    frames = rand_frames(8, 2, h, w)
    want = check(L, font, frames, rows.astype(np.float32), meta=meta, canvas_hw=canvas, center=center, class_names=NAMES, thickness=2)
    assert not np.array_equal(want, R.draw_batch(frames, rows.astype(np.float32), font, center=center, class_names=NAMES, thickness=2, palette=PALETTE3))


# ------------------------------------------------------------------------------------------ the Python layer
def ref_style(h, w):
    from yolo_for_turbines_amd.draw import default_style
    t, s = default_style(h, w)
    return dict(thickness=t, font_scale=s)


def test_draw_tracks_on_a_hand_made_result(yt, geo, font):
    tw, th, _ = geo
    h, w = th + 5, tw + 4
    frames = rand_frames(9, 2, h, w)
    rects = [(4, 20, 40, 36, 0.9, 0), (30, 12, 70, 30, 0.55, 1), (60, 15, 100, 33, 0.7, 4), (0, 0, 0, 0, 0, 0)]
    boxes = np.stack([px_boxes(rects, h, w), px_boxes(rects[::-1], h, w)])
    ids = np.array([[1, 2, 31, 0], [4, 9, 2, 1]], dtype=np.int32)
    count = np.array([3, 4], dtype=np.int32)
    res = yt.TrackResult(torch.from_numpy(boxes).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(count).cuda(), None)
    t = torch.from_numpy(frames).cuda()
    got = yt.draw_tracks(t, res, NAMES, thickness=2, font_scale=1)
    want = R.draw_batch(frames, boxes, font, ids=ids, count=count, class_names=NAMES, thickness=2, font_scale=1, color_by_id=True, palette=yt.draw.TAB20B)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert torch.equal(t.cpu(), torch.from_numpy(frames))              # out of place by default
    same = yt.draw_tracks(t, res, NAMES, thickness=2, font_scale=1, inplace=True)
    assert same.data_ptr() == t.data_ptr() and np.array_equal(t.cpu().numpy(), want)


def test_list_of_frames_of_two_sizes_and_single_frame(yt, geo, font):
    tw, th, _ = geo
    sizes = [(th + 3, tw + 5), (2 * th - 1, tw - 8)]
    frames = [rand_frames(10 + i, 1, h, w)[0] for i, (h, w) in enumerate(sizes)]
    rows = np.stack([px_boxes([(5, 12, 40, 30, 0.8, 1), (50, 14, 90, 28, 0.3, 0)], *sizes[0]), px_boxes([(8, 20, 60, 50, 0.6, 3), (2, 2, 30, 12, 0.2, 4)], *sizes[1])])
    count = np.array([2, 1], dtype=np.int32)
    got = yt.draw_boxes([torch.from_numpy(f).cuda() for f in frames], torch.from_numpy(rows).cuda(), count=torch.from_numpy(count).cuda(), class_names=NAMES)
    assert isinstance(got, list) and len(got) == 2
    pal = yt.draw.default_palette(len(NAMES))
    for i, (h, w) in enumerate(sizes):
        want = R.draw_frame(frames[i], rows[i], font, count=count[i], class_names=NAMES, palette=pal, **ref_style(h, w))
        assert tuple(got[i].shape) == (h, w, 3)
        np.testing.assert_array_equal(got[i].cpu().numpy(), want)
    one = yt.draw_boxes(torch.from_numpy(frames[0]).cuda(), torch.from_numpy(rows[0]).cuda(), class_names=NAMES, fill_alpha=0.25, line_alpha=0.5)
    want = R.draw_frame(frames[0], rows[0], font, class_names=NAMES, palette=pal, fill_alpha=64, line_alpha=128, **ref_style(*sizes[0]))
    np.testing.assert_array_equal(one.cpu().numpy(), want)


def test_python_meta_from_letterbox_tuples(yt, geo, font):
    tw, th, _ = geo
    h, w = th + 9, tw + 6
    frames = rand_frames(12, 2, h, w)
    metas = [(h, w, 50, 64, 7, 0), (h, w, 48, 60, 8, 2)]
    rows = np.random.default_rng(13).uniform(0.1, 0.6, (2, 6, 6)).astype(np.float32)
    rows[..., 5] = [0, 1, 2, 3, 4, 1]
    got = yt.draw_boxes(torch.from_numpy(frames).cuda(), torch.from_numpy(rows).cuda(), class_names=NAMES, meta=(metas, (64, 64)), palette=PALETTE3)
    want = R.draw_batch(frames, rows, font, meta=metas, canvas_hw=(64, 64), class_names=NAMES, palette=PALETTE3, **ref_style(h, w))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    table = torch.tensor(metas, dtype=torch.int32).cuda()
    again = yt.draw_boxes(torch.from_numpy(frames).cuda(), torch.from_numpy(rows).cuda(), class_names=NAMES, meta=(table, (64, 64)), palette=PALETTE3)
    np.testing.assert_array_equal(again.cpu().numpy(), want)


@pytest.fixture(scope="module")
def detections(yt):
    """detect_images of the synthetic 80-class model on two 64 x 64 inputs, at two thresholds: (boxes, keep, count) each."""
    from oracle import net as onet
    m = yt.YOLOv3(num_classes=80)
    m.load_state_dict(onet.synth_state_dict(11, 3, 80, gain=gi.NET_GAIN))
    m = m.cuda().eval()
    anchors = [a.cuda() for a in yt.scaled_anchors(gi.COCO_ANCHORS, 64, 64)]
    x = onet.synth_input(1, 2, 64).cuda()
    with torch.no_grad():
        flat = torch.cat([yt.decode_boxes(p.float().contiguous(), a, mutate=False) for p, a in zip(m(x), anchors)], 1)
    out = []
    for q in (0.9, 0.8):
        thr = float(torch.quantile(flat[..., 4].double().flatten(), q))
        boxes, keep, count = yt.detect_images(m, x, anchors, 0.45, thr)
        assert int(count.min()) >= 1
        out.append((boxes, keep, count))
    return out


def test_detector_end_to_end_and_one_captured_replay(yt, font, detections):
    names = ["c%d" % i for i in range(80)]
    pal = yt.draw.default_palette(80)
    frames = rand_frames(14, 2, 64, 64)
    t = torch.from_numpy(frames).cuda()
    ref = lambda d: R.draw_batch(frames, d[0].cpu().numpy(), font, keep=d[1].cpu().numpy(), count=d[2].cpu().numpy(), class_names=names, palette=pal,
                                 **ref_style(64, 64))
    first, second = detections
    want_first, want_second = ref(first), ref(second)
    assert not np.array_equal(want_first, want_second) and not np.array_equal(want_first, frames)
    static = [v.clone() for v in first]
    eager = yt.draw_boxes(t, *static, class_names=names)              # also makes the device copies of the names and the palette
    np.testing.assert_array_equal(eager.cpu().numpy(), want_first)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = yt.draw_boxes(t, *static, class_names=names)
    for dst, src in zip(static, second):                               # new detections into the captured tensors
        dst.copy_(src)
    out.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want_second)


def test_reference_wrappers(yt, geo, font):
    from yolo_for_turbines_amd import utils
    tw, th, _ = geo
    h, w = th + 20, tw + 30
    image = rand_frames(15, 1, h, w)[0]
    names = ["dirt", "damage"]
    boxes = [[0.3, 0.4, 0.2, 0.3, 0.9, 1], [0.7, 0.6, 0.25, 0.2, 0.8, 0]]
    rows = np.array(boxes, dtype=np.float32)
    pal = yt.draw.default_palette(2)
    got = utils.plot_image_with_boxes(image, boxes, names)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, R.draw_frame(image, rows, font, class_names=names, palette=pal, scores=False, **ref_style(h, w)))
    resized = np.zeros((64, 64, 3), np.uint8)
    mapped = np.array(yt.unletterbox_boxes(boxes, (h, w), (64, 64)), dtype=np.float32)
    got = utils.plot_original(image, resized, boxes, names)
    np.testing.assert_array_equal(got, R.draw_frame(image, mapped, font, class_names=names, palette=pal, scores=False, **ref_style(h, w)))
    assert not np.array_equal(got, image)
