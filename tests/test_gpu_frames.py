"""The frame front end on the GPU (csrc/frames.hip, yolo_for_turbines_amd/frames.py), bit for bit against tests/frames_ref.py: fp32
outputs as raw bits, meta as integers, no pixel, box or case left out. The shapes are a few dozen pixels and are chosen for the
kernel's edges (the tile the library reports is 64 x 16, a lane writes 4 pixels): landscape and portrait, an odd padding difference,
the copy path, an upscale, a non-integer downscale, 1 x 1 / 1 x 7 / 2 x 2 frames, a resized width that is no multiple of 4, canvases
of 32 and 96 columns, pitched rows, one frame, a ragged rect batch, every csc, and a pool offset above 2^31."""
import numpy as np
import pytest
import torch

from tests import frames_ref as R
from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu

# (image_size, [(h, w), ...]); RGB / BGR take them as they are, NV12 needs even sizes
RGB_CASES = {
    "s32": (32, [(1, 1), (1, 7), (20, 48), (48, 20), (32, 17), (10, 12)]),       # (20, 48): 13 rows, padding 9 + 10; (32, 17): the copy path, new_w % 4 = 1
    "s64": (64, [(100, 75), (97, 131)]),                                           # non-integer downscales
    "s96": (96, [(200, 150), (96, 50), (33, 77)]),
    "one": (64, [(41, 23)]),
}
NV12_CASES = {
    "s32": (32, [(2, 2), (20, 48), (48, 20), (32, 18), (10, 12)]),
    "s64": (64, [(100, 76), (98, 130)]),
    "s96": (96, [(200, 150), (96, 50), (34, 78)]),
    "one": (64, [(42, 22)]),
}
RAGGED = [(60, 100), (50, 40), (31, 17), (7, 9), (64, 33)]                       # rect, size 64: (60, 100) sets the width, (50, 40) the height
RAGGED_NV12 = [(60, 100), (50, 40), (30, 18), (8, 10), (64, 34)]


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd
    from yolo_for_turbines_amd import _lib
    _lib.lib()                       # must load: no fallback
    assert torch.cuda.is_available()
    return yolo_for_turbines_amd


def make_frame(rng, fmt, h, w, pitch=None):
    """A random frame as preprocess_frames takes it: an array, or with ``pitch`` a (buffer, h, w, pitch) surface whose padding bytes
    are random too."""
    rows, row = (h * 3 // 2, w) if fmt == "nv12" else (h, 3 * w)
    if pitch is None:
        a = rng.integers(0, 256, (rows, row), dtype=np.uint8)
        return a if fmt == "nv12" else a.reshape(h, w, 3)
    return (rng.integers(0, 256, rows * pitch, dtype=np.uint8), h, w, pitch)


def make_frames(seed, fmt, shapes, extra_pitch=None):
    rng = np.random.default_rng(seed)
    return [make_frame(rng, fmt, h, w, None if extra_pitch is None else (w if fmt == "nv12" else 3 * w) + extra_pitch) for h, w in shapes]


def to_device(frames):
    return [(torch.from_numpy(f[0]).cuda(),) + f[1:] if isinstance(f, tuple) else torch.from_numpy(f).cuda() for f in frames]


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.uint32)


def check(yt, frames, size, fmt, csc="bt601", rect=False, given=None):
    want_x, want_meta = R.preprocess(frames, size, fmt, csc, rect)
    x, meta = yt.preprocess_frames(frames if given is None else given, size, fmt, csc, rect)
    assert x.dtype == torch.float32 and meta.dtype == torch.int32 and x.is_cuda and meta.is_cuda
    assert tuple(x.shape) == want_x.shape
    assert np.array_equal(meta.cpu().numpy(), want_meta)
    assert np.array_equal(bits(x), bits(want_x))
    return x, meta


@pytest.mark.parametrize("fmt", ["rgb", "bgr", "nv12"])
@pytest.mark.parametrize("case", ["s32", "s64", "s96", "one"])
def test_host_frames_against_the_reference(yt, fmt, case):
    size, shapes = (NV12_CASES if fmt == "nv12" else RGB_CASES)[case]
    check(yt, make_frames(1, fmt, shapes), size, fmt)


def test_the_cases_hold_the_edges_they_are_meant_to(yt):
    """The shape list against the kernel's geometry: what the module's docstring promises does occur."""
    from yolo_for_turbines_amd import _lib as L
    tw, th = L.C.c_int(), L.C.c_int()
    L.lib().yolo_frames_tile(L.C.byref(tw), L.C.byref(th))
    assert 32 % tw.value and 96 % tw.value                                         # canvases that are no multiple of the tile width
    metas = np.concatenate([R.preprocess([np.zeros((h, w, 3), np.uint8) for h, w in shapes], size, "rgb")[1] for size, shapes in RGB_CASES.values()])
    oh, ow, nh, nw, top, left = metas.T
    assert (top > 0).any() and (left > 0).any()                                    # landscape and portrait
    assert ((32 - nh[:6]) % 2 == 1).any()                                          # an odd padding difference
    assert ((oh == nh) & (ow == nw)).any() and ((nh > oh) & (nw > ow)).any()        # the copy path, an upscale
    assert (nw % 4 != 0).any() and ((left % 4 != 0) & (left > 0)).any()             # a 4-pixel vector straddles the image edge
    assert R.canvas_hw(RAGGED, 64, True) == (64, 64) and R.resized_hw(*RAGGED[0], 64)[0] < 64 > R.resized_hw(*RAGGED[1], 64)[1]


@pytest.mark.parametrize("csc", R.CSC_KINDS)
def test_every_csc(yt, csc):
    size, shapes = NV12_CASES["s32"]
    check(yt, make_frames(2, "nv12", shapes), size, "nv12", csc)


@pytest.mark.parametrize("fmt", ["rgb", "bgr", "nv12"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_pitched_surfaces(yt, fmt, where):
    size, shapes = (NV12_CASES if fmt == "nv12" else RGB_CASES)["s32"]
    frames = make_frames(3, fmt, shapes, extra_pitch=6 if fmt == "nv12" else 5)
    check(yt, frames, size, fmt, given=to_device(frames) if where == "device" else None)


@pytest.mark.parametrize("fmt,shapes", [("rgb", RAGGED), ("bgr", RAGGED), ("nv12", RAGGED_NV12)])
def test_ragged_rect_batch_whose_canvas_two_frames_set(yt, fmt, shapes):
    frames = make_frames(4, fmt, shapes)
    x, _ = check(yt, frames, 64, fmt, rect=True)
    assert tuple(x.shape[2:]) == (64, 64)
    mixed = [torch.from_numpy(f).cuda() if i % 2 else f for i, f in enumerate(frames)]          # host and device frames in one list
    check(yt, frames, 64, fmt, rect=True, given=mixed)
    low = make_frames(5, fmt, [(30, 100), (40, 90)])                                             # a canvas of 32 x 64
    x, _ = check(yt, low, 64, fmt, rect=True, given=to_device(low))
    assert tuple(x.shape[2:]) == (32, 64)


@pytest.mark.parametrize("fmt", ["rgb", "nv12"])
def test_one_device_batch_tensor_is_read_in_place(yt, fmt):
    frames = make_frames(6, fmt, [(24, 36)] * 3)
    batch = torch.from_numpy(np.stack(frames)).cuda()
    x, meta = check(yt, frames, 32, fmt, given=batch)
    out = torch.full_like(x, -1.0)
    x2, _ = yt.preprocess_frames(batch, 32, fmt, out=out)
    assert x2 is out and torch.equal(out, x)
    with pytest.raises(ValueError, match="contiguous"):
        yt.preprocess_frames(batch.transpose(1, 2), 32, fmt)
    with pytest.raises(ValueError, match="different devices"):
        yt.preprocess_frames(batch, 32, fmt, device="cuda:%d" % (torch.cuda.device_count() + 1))
    with pytest.raises(ValueError, match="out"):
        yt.preprocess_frames(batch, 32, fmt, out=torch.empty((3, 3, 32, 32), dtype=torch.float16, device="cuda"))


def test_rgb_equals_the_existing_letterbox(yt):
    for size, shapes, rect in ((32, RGB_CASES["s32"][1], False), (64, RAGGED, True), (96, RGB_CASES["s96"][1], True)):
        frames = make_frames(7, "rgb", shapes)
        want, want_meta = yt.letterbox(frames, size, rect=rect)
        x, meta = yt.preprocess_frames(frames, size, "rgb", rect=rect)
        assert torch.equal(x.view(torch.int32), want.view(torch.int32))
        assert [tuple(r) for r in meta.tolist()] == [tuple(int(v) for v in m) for m in want_meta]


def test_pool_offset_above_2_31(yt):
    """Two small NV12 frames in one uninitialised 2 GiB + 64 KiB allocation, the second behind 2^31: its table offset needs 64 bits."""
    frames = make_frames(8, "nv12", [(20, 48), (48, 20)], extra_pitch=2)
    big = torch.empty(2 ** 31 + 65536, dtype=torch.uint8, device="cuda")
    at = [0, 2 ** 31 + 4096]
    given = []
    for (buf, h, w, pitch), o in zip(frames, at):
        big[o:o + buf.size].copy_(torch.from_numpy(buf))
        given.append((big[o:o + buf.size], h, w, pitch))
    assert given[1][0].data_ptr() - given[0][0].data_ptr() >= 2 ** 31
    check(yt, frames, 32, "nv12", "bt709", given=given)
    del big, given
    torch.cuda.empty_cache()


def test_full_geometry_1080p_nv12_pitch_2048(yt):
    frames = make_frames(9, "nv12", [(1080, 1920)] * 2, extra_pitch=128)
    assert frames[0][3] == 2048
    check(yt, frames, 416, "nv12", given=to_device(frames))


@pytest.mark.parametrize("fmt,shape,extra", [("rgb", (5, 7), None), ("bgr", (5, 7), 1), ("bgr", (24, 36), None), ("nv12", (6, 10), None),
                                             ("nv12", (24, 36), 3), ("rgb", (1, 1), None)])
def test_frames_to_rgb(yt, fmt, shape, extra):
    frames = make_frames(10, fmt, [shape] * 3, extra_pitch=extra)
    for csc in (("bt601", "bt709-full") if fmt == "nv12" else ("bt601",)):
        want = np.stack([R.to_rgb(f, fmt, csc) for f in frames])
        got = yt.frames_to_rgb(to_device(frames), fmt, csc)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
        out = torch.zeros_like(got)
        assert yt.frames_to_rgb(frames, fmt, csc, out=out) is out and np.array_equal(out.cpu().numpy(), want)


def edge_boxes(meta, canvas, rng):
    """(B, 6, 6) rows on and across each frame's padding edge, plus rows of zeros."""
    B = meta.shape[0]
    rows = np.zeros((B, 6, 6), np.float32)
    for s in range(B):
        _, _, nh, nw, top, left = (int(v) for v in meta[s])
        rows[s, 0] = [left / canvas[1], top / canvas[0], nw / canvas[1], nh / canvas[0], 0.9, 1]               # the image's corner, its size
        rows[s, 1] = [(left + nw) / canvas[1], (top + nh) / canvas[0], 0.5, 0.5, 0.5, 2]                      # the far corner: across the edge
        rows[s, 2] = [(left - 1.5) / canvas[1], (top - 0.25) / canvas[0], 3 / canvas[1], 1 / canvas[0], 0.1, 0]  # in the padding
        rows[s, 3] = rng.random(6).astype(np.float32)
        rows[s, 5] = [1 / 3, 2 / 3, 1e-3, 1.0, 0.7, 79]
    return rows


def test_boxes_to_frames(yt):
    frames = make_frames(11, "rgb", RAGGED)
    _, meta = yt.preprocess_frames(frames, 64, "rgb", rect=True)
    rows = edge_boxes(meta.cpu().numpy(), (64, 64), np.random.default_rng(12))
    want = R.unletterbox(rows, meta.cpu().numpy(), (64, 64))
    t = torch.from_numpy(rows).cuda()
    got = yt.boxes_to_frames(t, meta, (64, 64))
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(t), bits(rows))
    assert (want[:, 4, 2:] == 0).all() and (want[:, 0, :2] == 0).all() and np.array_equal(want[:, 0, 2:4], np.ones((5, 2), np.float32))
    assert yt.boxes_to_frames(t, meta, (64, 64), out=t) is t and np.array_equal(bits(t), bits(want))          # in place
    # ... and row by row it is the package's own host expression
    for s in range(5):
        host = yt.unletterbox_boxes([[float(v) for v in r] for r in rows[s]], None, (64, 64), meta=tuple(meta[s].tolist()))
        assert np.array_equal(bits(np.array(host, np.float64).astype(np.float32)), bits(want[s]))


def test_draw_boxes_takes_the_device_table(yt):
    frames = make_frames(13, "rgb", [(40, 56)] * 3)
    batch = torch.from_numpy(np.stack(frames)).cuda()
    x, meta = yt.preprocess_frames(batch, 64, "rgb", rect=True)
    canvas = tuple(x.shape[2:])
    _, tuples = yt.letterbox(frames, 64, rect=True)
    rows = torch.from_numpy(edge_boxes(meta.cpu().numpy(), canvas, np.random.default_rng(14))).cuda()
    rows[..., 5] = torch.tensor([0, 1, 2, 0, 1, 2], device="cuda")
    names = ["a", "b", "c"]
    with_table = yt.draw_boxes(batch, rows, class_names=names, meta=(meta, canvas))
    with_tuples = yt.draw_boxes(batch, rows, class_names=names, meta=(tuples, canvas))
    assert torch.equal(with_table, with_tuples) and not torch.equal(with_table, batch)


def test_stager_reuses_its_storage_and_replays_in_a_graph(yt):
    n, h, w = 3, 24, 36
    first, second = make_frames(15, "nv12", [(h, w)] * n), make_frames(16, "nv12", [(h, w)] * n)
    want_first, want_meta = R.preprocess(first, 32, "nv12", "bt709")
    want_second, _ = R.preprocess(second, 32, "nv12", "bt709")
    assert not np.array_equal(want_first, want_second)
    st = yt.FrameStager(n, h, w, "nv12", 32, csc="bt709")
    x1, m1 = st.stage(first)                                                       # host frames: the pinned path
    assert np.array_equal(bits(x1), bits(want_first)) and np.array_equal(m1.cpu().numpy(), want_meta)
    x2, m2 = st.stage(np.stack(second))
    assert x2 is x1 and m2 is m1 and x2.data_ptr() == x1.data_ptr() and np.array_equal(bits(x2), bits(want_second))
    x3, _ = st.stage(first)                                                        # the first pinned buffer again
    assert np.array_equal(bits(x3), bits(want_first))
    x4, _ = st.stage([torch.from_numpy(f).cuda() for f in second])                 # a list of device frames: gathered into the pool
    assert np.array_equal(bits(x4), bits(want_second))
    static = torch.from_numpy(np.stack(first)).cuda()
    eager, _ = st.stage(static)
    eager = eager.clone()
    assert np.array_equal(bits(eager), bits(want_first))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, _ = st.stage(static)
    static.copy_(torch.from_numpy(np.stack(second)))                               # new frame contents into the captured tensor
    out.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), bits(want_second))
    with pytest.raises(ValueError, match="frame 0.*shape"):
        st.stage(static[:2])
    with pytest.raises(ValueError, match="frame 1.*shape"):
        st.stage([first[0], first[1][:, :-2], first[2]])


def test_detect_frames_is_letterbox_detect_unletterbox(yt):
    from oracle import net as onet
    m = yt.YOLOv3(num_classes=80)
    m.load_state_dict(onet.synth_state_dict(11, 3, 80, gain=gi.NET_GAIN))
    m = m.cuda().eval()
    anchors = [a.cuda() for a in yt.scaled_anchors(gi.COCO_ANCHORS, 96, 96)]
    frames = make_frames(17, "nv12", [(60, 100), (120, 90)])
    rgb = [R.to_rgb(f, "nv12", "bt709") for f in frames]
    x, tuples = yt.letterbox(rgb, 96)
    with torch.no_grad():
        flat = torch.cat([yt.decode_boxes(p.float().contiguous(), a, mutate=False) for p, a in zip(m(x), anchors)], 1)
    thr = float(torch.quantile(flat[..., 4].double().flatten(), 0.9))
    want_boxes, want_keep, want_count = yt.detect_images(m, x, anchors, 0.45, thr)
    assert int(want_count.min()) >= 1
    boxes, keep, count, meta = yt.detect_frames(m, frames, anchors, 96, "nv12", "bt709", iou_threshold=0.45, obj_threshold=thr)
    assert torch.equal(count, want_count)
    for s in range(2):                                                             # keep is defined up to count
        assert torch.equal(keep[s, :int(count[s])], want_keep[s, :int(count[s])])
    assert [tuple(r) for r in meta.tolist()] == [tuple(int(v) for v in t) for t in tuples]
    wb = want_boxes.cpu().numpy()
    for s in range(2):
        host = yt.unletterbox_boxes([[float(v) for v in r] for r in wb[s]], None, (96, 96), meta=tuples[s])
        assert np.array_equal(bits(boxes[s]), bits(np.array(host, np.float64).astype(np.float32)))
