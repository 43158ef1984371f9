"""Pyramid levels and the seam test of tiled detection on the GPU: yolo_tile_gather_scaled bit for bit against
oracle.preprocess.resize_linear_u8 + slice / pad / scale, yolo_tile_collect_ex bit for bit against a sequential numpy restatement
(float32, one rounding per operation) with hand-placed rows on both sides of every comparison of the seam test, what the two are
for (a fragmented object reported whole by a coarser level), and detect_tiled(scales=..., edge_margin=...) against the composition
of those restatements with model(x), decode_boxes and nms_indices (fp32 and bf16)."""
import numpy as np
import pytest
import torch

from oracle import net as onet
from oracle.preprocess import resize_linear_u8
from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu
SPARE = 4096            # guard bytes behind every output buffer
F32 = np.float32
TH, TW = 64, 96
FRAMES_HW = [(150, 203), (45, 70)]


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


# ------------------------------------------------------------------------------------------ restatements
def np_tiles(img, origins, th, tw):
    """slice, zero-pad, astype(float32) * float32(1 / 255), transpose -> (T, 3, th, tw)"""
    out = np.zeros((len(origins), 3, th, tw), F32)
    for t, (y0, x0) in enumerate(origins):
        part = img[y0:y0 + th, x0:x0 + tw]
        pad = np.zeros((th, tw, 3), np.uint8)
        pad[:part.shape[0], :part.shape[1]] = part
        out[t] = (pad.astype(F32) * F32(1.0 / 255.0)).transpose(2, 0, 1)
    return out


def np_level_tiles(img, lh, lw, origins, th, tw):
    """The level is the whole frame resized (the oracle's uint8 INTER_LINEAR), then cut like a frame."""
    return np_tiles(resize_linear_u8(img, lh, lw), origins, th, tw)


def np_sides(b, th, tw):
    """left, right, top, bottom of the rows of one tile in tile pixels, float32, one rounding per operation."""
    with np.errstate(all="ignore"):
        px, py = b[:, 0] * F32(tw), b[:, 1] * F32(th)
        hx, hy = (b[:, 2] * F32(tw)) * F32(0.5), (b[:, 3] * F32(th)) * F32(0.5)
        out = px - hx, px + hx, py - hy, py + hy
    assert all(v.dtype == F32 for v in out)
    return out


def np_cut(b, y0, x0, H, W, th, tw, margin):
    """Cut by a side of the tile that is not on the level's border. Equality and NaN are not cut; margin < 0 is off."""
    cut = np.zeros(len(b), bool)
    if margin < 0:
        return cut
    m = F32(margin)
    left, right, top, bottom = np_sides(b, th, tw)
    with np.errstate(all="ignore"):
        if x0 > 0:
            cut |= left < m
        if x0 + tw < W:
            cut |= right > F32(tw) - m
        if y0 > 0:
            cut |= top < m
        if y0 + th < H:
            cut |= bottom > F32(th) - m
    return cut


def np_collect_ex(boxes, tiles, level_hw, n_images, th, tw, thr, margin):
    """Per image the candidate rows in (tile, row) order. float32 throughout, every operation rounded once."""
    out = [[np.zeros((0, 6), F32)] for _ in range(n_images)]
    for t, (im, y0, x0, lv) in enumerate(tiles):
        if not (0 <= im < n_images and 0 <= lv < len(level_hw)):
            continue
        H, W = level_hw[lv]
        b = boxes[t]
        with np.errstate(all="ignore"):
            cx = (b[:, 0] * F32(tw) + F32(x0)) / F32(W)
            cy = (b[:, 1] * F32(th) + F32(y0)) / F32(H)
            w = (b[:, 2] * F32(tw)) / F32(W)
            h = (b[:, 3] * F32(th)) / F32(H)
            ok = (b[:, 4].astype(np.float64) > thr) & (cx <= F32(1)) & (cy <= F32(1))
        ok &= ~np_cut(b, y0, x0, H, W, th, tw, margin)
        rows = np.stack([cx, cy, w, h, b[:, 4], b[:, 5]], 1)
        assert rows.dtype == F32
        out[im].append(rows[ok])
    return [np.concatenate(o) for o in out]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def filled(nbytes, value):
    return torch.full((nbytes,), value, dtype=torch.uint8, device="cuda")


def cand_rows(buf, F, cap):
    return buf[:F * cap * 24].view(np.uint32).reshape(F, cap, 6)


def run_collect_ex(L, boxes, tiles, level_hw, n_images, th, tw, thr, margin, cap, fill=0xA5, calls=None):
    """yolo_tile_collect_ex on (a split of) the tiles into a cand buffer pre-filled with `fill`; returns (cand bytes as a uint8 array
    incl. SPARE guard bytes, count)."""
    lib = L.lib()
    T, n_per, F = boxes.shape[0], boxes.shape[1], n_images
    d_boxes = torch.from_numpy(boxes).cuda()
    d_tiles = torch.tensor(tiles, dtype=torch.int32).reshape(T, 4).cuda()
    d_lev = torch.tensor(level_hw, dtype=torch.int32).reshape(len(level_hw), 2).cuda()
    buf = filled(F * cap * 24 + SPARE, fill)
    count = torch.zeros(F, dtype=torch.int32, device="cuda")
    stream = L.current_stream()
    for a, b in calls or [(0, T)]:
        need = lib.yolo_tile_collect_workspace_bytes(b - a, n_per)
        ws = filled(need + SPARE, 0x3C)
        L.check(lib.yolo_tile_collect_ex(d_boxes[a:b].data_ptr(), b - a, n_per, d_tiles[a:b].data_ptr(), d_lev.data_ptr(), len(level_hw), F,
                                         th, tw, thr, margin, buf.data_ptr(), cap, count.data_ptr(), ws.data_ptr(), need, stream),
                "yolo_tile_collect_ex")
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0x3C).all()), "wrote behind the workspace"
    return buf.cpu().numpy(), count.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1. scaled gather
def _gather(L, img, lh, lw, origins, scaled=True):
    h, w = img.shape[:2]
    T = len(origins)
    nbytes = T * 3 * TH * TW * 4
    out = filled(nbytes + SPARE, 0x77)
    d_img = torch.from_numpy(img).cuda()
    d_or = torch.tensor(origins, dtype=torch.int32).reshape(T, 2).cuda()
    lib = L.lib()
    if scaled:
        L.check(lib.yolo_tile_gather_scaled(d_img.data_ptr(), h, w, lh, lw, d_or.data_ptr(), T, TH, TW, out.data_ptr(), L.current_stream()),
                "yolo_tile_gather_scaled")
    else:
        L.check(lib.yolo_tile_gather(d_img.data_ptr(), h, w, d_or.data_ptr(), T, TH, TW, out.data_ptr(), L.current_stream()), "yolo_tile_gather")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[nbytes:] == 0x77).all(), "wrote behind out"
    return got[:nbytes].view(np.uint32)


# frame, level, origins that are appended to the level's grid (anywhere, odd, hanging over the level's edge)
GATHER_CASES = [((150, 203), (75, 102), [(7, 5), (40, 51)]),         # down by 2: 2 x 2 tiles, the last one flush at (11, 6)
                ((45, 70), (68, 105), [(3, 9)]),                      # up by 1.5: 2 x 2 tiles, the last one flush at (4, 9)
                ((45, 70), (22, 35), []),                             # smaller than the tile: rows and columns of padding
                ((150, 203), (150, 203), [(85, 106)])]                # the frame itself


@pytest.mark.parametrize("hw,level,extra", GATHER_CASES)
def test_gather_scaled_bit_for_bit(L, yt, hw, level, extra):
    (h, w), (lh, lw) = hw, level
    rng = np.random.default_rng(h * 1000 + lw)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    grid = yt.tile_grid(lh, lw, (TH, TW), (16, 32)).tolist()
    if level == (75, 102):
        assert grid == [[0, 0], [0, 6], [11, 0], [11, 6]]                       # the last tile is flush with the level, odd y0
    elif level == (68, 105):
        assert grid == [[0, 0], [0, 9], [4, 0], [4, 9]]
    elif level == (22, 35):
        assert grid == [[0, 0]]
    else:
        assert len(grid) == 9 and grid[-1] == [86, 107]
    origins = [tuple(o) for o in grid] + extra
    want = np_level_tiles(img, lh, lw, origins, TH, TW)
    got = _gather(L, img, lh, lw, origins)
    np.testing.assert_array_equal(got, bits(want).reshape(-1))
    assert all(t.max() > 0.9 for t in want)                                      # every tile holds pixels (the means of random ones)
    if level == (22, 35):
        assert (want[:, :, lh:, :] == 0).all() and (want[:, :, :, lw:] == 0).all()
    if level == (75, 102):
        assert (want[-1, :, 75 - 40:, :] == 0).all() and (want[-1, :, :, 102 - 51:] == 0).all() and want[-1].max() > 0.9
    if level == hw:                                                              # the bytes of yolo_tile_gather on the same origins
        np.testing.assert_array_equal(got, _gather(L, img, lh, lw, origins, scaled=False))


# ------------------------------------------------------------------------------------------ 2. collect_ex
N_PER = 10647
THR = 0.98046875                      # 251 / 256: a float32, so a score can sit exactly at the threshold
MARGINS = (-1.0, 0.0, 2.0)
# two images with two levels each: image 0 = levels 0 (the frame) and 1 (x 0.5), image 1 = levels 2 (the frame, smaller than a
# tile) and 3 (x 1.5)
LEVEL_HW = [(150, 203), (75, 102), (45, 70), (68, 105)]
TILES = [(0, 48, 64, 0),              # 0: inside level 0: all four sides interior
         (1, 0, 0, 2),                # 1: the padded single tile of level 2: no interior side
         (0, 0, 0, 1),                # 2: level 1: left and top on the border, right (96 < 102) and bottom (64 < 75) interior
         (-1, 0, 0, 0),               # 3: dead by its image
         (1, 4, 9, 3),                # 4: the flush last tile of level 3: left and top interior, right and bottom on the border
         (0, 0, 0, 7),                # 5: dead by its level
         (0, 86, 107, 0),             # 6: the flush last tile of level 0
         (1, 0, 0, 3)]                # 7: level 3: right and bottom interior
ALL, BORDER_LT, BORDER_RB = 0, 2, 4   # tiles that have every side interior / left and top / right and bottom on the border
W44 = F32(44) / F32(96)               # (W44 * 96) * 0.5 == 22 in float32 (asserted below)


def _hand_rows():
    """name -> (tile, row, [cx, cy, w, h, obj]). The other axis of every row is far from its sides (extent 0.2, centre 0.4 to 0.53)
    and its centre differs from row to row, so a row can be found among the candidates by its coordinates."""
    # two float32 steps up / down: one step of 0.75 is half a step of 64, and 48 + 16 would round back to 64
    up = lambda v: np.nextafter(np.nextafter(F32(v), F32(2)), F32(2))            # noqa: E731
    dn = lambda v: np.nextafter(np.nextafter(F32(v), F32(-1)), F32(-1))          # noqa: E731
    rows = {}
    k = 3000

    def put(name, tile, vals):
        nonlocal k
        rows[name] = (tile, k, vals)
        k += 7

    for side in ("left", "right", "top", "bottom"):
        horizontal = side in ("left", "right")
        low = side in ("left", "top")
        border_tile = BORDER_LT if low else BORDER_RB

        def row(c, e, obj=1.0, horizontal=horizontal):
            other = 0.4 + len(rows) / 256
            return [c, other, e, 0.2, obj] if horizontal else [other, c, 0.2, e, obj]
        cut = row(0.1 if low else 0.9, 0.3)                                    # reaches 4.8 (3.2) pixels beyond the side
        put(f"{side}_cut_interior", ALL, cut)
        put(f"{side}_kept_border", border_tile, cut)
        if horizontal:                                                         # exactly margin 2 away from the side: 24 -+ 22, 72 +- 22
            put(f"{side}_equal_2", ALL, row(0.25 if low else 0.75, W44))
            put(f"{side}_inside_2", ALL, row(dn(0.25) if low else up(0.75), W44))
        else:                                                                  # 16 -+ 14, 48 +- 14
            put(f"{side}_equal_2", ALL, row(0.25 if low else 0.75, 0.4375))
            put(f"{side}_inside_2", ALL, row(dn(0.25) if low else up(0.75), 0.4375))
        put(f"{side}_equal_0", ALL, row(0.25 if low else 0.75, 0.5))            # exactly on the side: margin 0
        put(f"{side}_inside_0", ALL, row(dn(0.25) if low else up(0.75), 0.5))
        put(f"{side}_nan", ALL, row(0.01 if low else 0.99, np.nan))            # NaN extent: every comparison is false
        put(f"{side}_at_threshold", ALL, row(0.5, 0.2, obj=THR))               # cut by nothing, out by its score
    return rows


HAND = _hand_rows()


@pytest.fixture(scope="module")
def collect_case():
    """Decoded rows of 8 tiles (6 live over 2 images and 4 levels), about 2 % above the threshold, the hand-placed rows, and what
    the restatement makes of them per margin (computed once)."""
    rng = np.random.default_rng(17)
    b = np.empty((len(TILES), N_PER, 6), F32)
    b[..., 0:2] = rng.random((len(TILES), N_PER, 2), dtype=F32)
    b[..., 2:4] = rng.random((len(TILES), N_PER, 2), dtype=F32) * F32(0.3)
    b[..., 4] = rng.random((len(TILES), N_PER), dtype=F32)
    b[..., 5] = rng.integers(0, 80, (len(TILES), N_PER)).astype(F32)
    special = [0, 255, 256, 1023, 1024, 1025, 2047, 2048, 10239, 10240, N_PER - 1]      # around every block boundary
    for t in range(len(TILES)):
        for k, r in enumerate(special):
            b[t, r, 4] = [THR, np.nan, np.inf, np.nextafter(F32(THR), F32(1)), 1.0][(k + t) % 5]
            b[t, r, 0:2] = F32(0.25)                                                     # inside every level
    for tile, r, vals in HAND.values():
        b[tile, r, 0:5] = np.array(vals, F32)
    want = {m: np_collect_ex(b, TILES, LEVEL_HW, 2, TH, TW, THR, m) for m in MARGINS}
    return b, want


def _in_output(row, tile, want_f, th=TH, tw=TW):
    """Is the remapped hand row among the candidates of its image? (its class column, a random integer, is not compared)"""
    im, y0, x0, lv = TILES[tile]
    H, W = LEVEL_HW[lv]
    r = np.array(row[:4], F32)
    key = bits(np.array([(r[0] * F32(tw) + F32(x0)) / F32(W), (r[1] * F32(th) + F32(y0)) / F32(H), (r[2] * F32(tw)) / F32(W),
                         (r[3] * F32(th)) / F32(H)], F32))
    return bool((bits(want_f[:, :4]) == key).all(1).any())


def test_collect_case_has_what_it_should(collect_case):
    b, want = collect_case
    live = [t for t, tl in enumerate(TILES) if 0 <= tl[0] < 2 and 0 <= tl[3] < len(LEVEL_HW)]
    assert live == [0, 1, 2, 4, 6, 7]
    above = sum(int((b[t, :, 4].astype(np.float64) > THR).sum()) for t in live)
    assert 0.01 < above / (len(live) * N_PER) < 0.03
    n = {m: sum(len(w) for w in want[m]) for m in MARGINS}
    assert above > n[-1.0] > n[0.0] > n[2.0] > 200                # centres in the padding; then rows cut at margin 0; more at 2
    for t in (3, 5):
        assert (b[t, :, 4] > THR).any()                           # the dead tiles have candidates to ignore
    for m in MARGINS:
        for w in want[m]:
            assert len(w) > 100 and np.isinf(w[:, 4]).any() and not np.isnan(w[:, 4]).any() and (w[:, 4] > F32(THR)).all()
    # the sides of the hand rows are what their names say, in the float32 arithmetic of the contract
    side_of = {"left": 0, "right": 1, "top": 2, "bottom": 3}
    for name, (tile, r, vals) in HAND.items():
        side, kind = name.split("_", 1)
        im = TILES[tile][0]
        v = np_sides(b[tile, r:r + 1], TH, TW)[side_of[side]][0]
        low = side in ("left", "top")
        edge = F32(0) if low else F32(TW if side == "right" else TH)
        dist = v - edge if low else edge - v                      # how far inside the tile the box ends (exact for these values)
        present = {m: _in_output(vals, tile, want[m][im]) for m in MARGINS}
        if kind == "cut_interior":
            assert dist < 0 and present == {-1.0: True, 0.0: False, 2.0: False}, name
        elif kind == "kept_border":
            assert dist < 0 and present == {-1.0: True, 0.0: True, 2.0: True}, name
        elif kind == "equal_2":
            assert dist == F32(2) and present == {-1.0: True, 0.0: True, 2.0: True}, name
        elif kind == "inside_2":
            assert 1.99 < dist < F32(2) and present == {-1.0: True, 0.0: True, 2.0: False}, name
        elif kind == "equal_0":
            assert dist == F32(0) and present == {-1.0: True, 0.0: True, 2.0: False}, name
        elif kind == "inside_0":
            assert -0.01 < dist < F32(0) and present == {-1.0: True, 0.0: False, 2.0: False}, name
        elif kind == "nan":
            assert np.isnan(v) and b[tile, r, 4] > THR and present == {-1.0: True, 0.0: True, 2.0: True}, name
        else:
            assert kind == "at_threshold" and b[tile, r, 4] == F32(THR) and not any(present.values()), name
    assert len(HAND) == 4 * 8


@pytest.mark.parametrize("margin", MARGINS)
def test_collect_ex_equals_restatement(L, collect_case, margin):
    """One call, and the same tiles in three calls (3 + 2 + 3): rows, order, count, and nothing else touched."""
    b, want = collect_case
    cap = 2048
    for calls in (None, [(0, 3), (3, 5), (5, 8)]):
        buf, count = run_collect_ex(L, b, TILES, LEVEL_HW, 2, TH, TW, THR, margin, cap, calls=calls)
        assert count.tolist() == [len(w) for w in want[margin]]
        rows = cand_rows(buf, 2, cap)
        for f, w in enumerate(want[margin]):
            assert len(w) < cap
            np.testing.assert_array_equal(rows[f, :len(w)], bits(w))
            assert (rows[f, len(w):] == 0xA5A5A5A5).all()
        assert (buf[2 * cap * 24:] == 0xA5).all()


def test_collect_ex_without_seam_test_is_collect(L):
    """edge_margin < 0 and a level table equal to the frame sizes: the bytes of yolo_tile_collect (the whole buffer and the counts)."""
    img_hw = [(150, 203), (45, 70)]
    tiles = [(0, 0, 0, 0), (0, 48, 64, 0), (1, 0, 0, 1), (-1, 0, 0, 0), (0, 86, 107, 0), (1, 0, 0, 1)]
    n_per, cap = 2500, 512
    rng = np.random.default_rng(23)
    b = rng.random((len(tiles), n_per, 6), dtype=F32)
    b[..., 2:4] *= F32(0.3)
    b[..., 5] = rng.integers(0, 80, (len(tiles), n_per)).astype(F32)
    buf, count = run_collect_ex(L, b, tiles, img_hw, 2, TH, TW, THR, -1.0, cap)
    lib = L.lib()
    d_boxes = torch.from_numpy(b).cuda()
    d_tiles = torch.tensor([t[:3] + (0,) for t in tiles], dtype=torch.int32).cuda()        # today's table: the fourth field is 0
    d_hw = torch.tensor(img_hw, dtype=torch.int32).cuda()
    old = filled(2 * cap * 24 + SPARE, 0xA5)
    old_count = torch.zeros(2, dtype=torch.int32, device="cuda")
    need = lib.yolo_tile_collect_workspace_bytes(len(tiles), n_per)
    ws = filled(need, 0x3C)
    L.check(lib.yolo_tile_collect(d_boxes.data_ptr(), len(tiles), n_per, d_tiles.data_ptr(), d_hw.data_ptr(), 2, TH, TW, THR, old.data_ptr(),
                                  cap, old_count.data_ptr(), ws.data_ptr(), need, L.current_stream()), "yolo_tile_collect")
    torch.cuda.synchronize()
    assert count.tolist() == old_count.cpu().tolist() and all(20 < c < cap for c in count.tolist())
    np.testing.assert_array_equal(buf, old.cpu().numpy())
    want = np_collect_ex(b, tiles, img_hw, 2, TH, TW, THR, -1.0)
    assert count.tolist() == [len(w) for w in want]


def test_collect_ex_overflow(L, collect_case):
    """cap = half of image 0's candidates: the first cap rows, the true totals, the next image and the guard bytes untouched."""
    b, want = collect_case
    want = want[2.0]
    cap = len(want[0]) // 2
    assert 0 < cap < len(want[0]) and cap < len(want[1])
    for calls in (None, [(0, 3), (3, 5), (5, 8)]):
        buf, count = run_collect_ex(L, b, TILES, LEVEL_HW, 2, TH, TW, THR, 2.0, cap, calls=calls)
        assert count.tolist() == [len(w) for w in want]
        rows = cand_rows(buf, 2, cap)
        for f, w in enumerate(want):
            k = min(cap, len(w))
            np.testing.assert_array_equal(rows[f, :k], bits(w[:k]))
            assert (rows[f, k:] == 0xA5A5A5A5).all()
        assert (buf[2 * cap * 24:] == 0xA5).all()


# ------------------------------------------------------------------------------------------ 3. what it is for
def _iou(a, b):
    """IoU of two [cx, cy, w, h] boxes, float64."""
    ax0, ax1, ay0, ay1 = a[0] - a[2] / 2, a[0] + a[2] / 2, a[1] - a[3] / 2, a[1] + a[3] / 2
    bx0, bx1, by0, by1 = b[0] - b[2] / 2, b[0] + b[2] / 2, b[1] - b[3] / 2, b[1] + b[3] / 2
    inter = max(0.0, min(ax1, bx1) - max(ax0, bx0)) * max(0.0, min(ay1, by1) - max(ay0, by0))
    return inter / (a[2] * a[3] + b[2] * b[3] - inter)


@pytest.mark.parametrize("margin,kept", [(-1.0, 3), (2.0, 1)])
def test_fragments_of_a_large_object_give_way_to_the_coarse_level(L, yt, margin, kept):
    """A diagonal crack in a 96 x 160 frame, bounding box x 50..110, y 28..68: 60 pixels wide, the overlap of the two level-0 tiles
    (tile 96, x0 = 0 and 64) is 32. The left tile sees its upper part up to its right side (x 50..96, y 28..50), the right tile
    its lower part from its left side on (x 64..110, y 46..68); the single tile of the x 0.5 level (48 x 80) sees it whole.
    Both fragments score higher than the whole box and their IoU with it is below the NMS threshold."""
    t, n_per, iou_thr = 96, 4, 0.45
    b = np.zeros((3, n_per, 6), F32)
    b[0, 1] = [73 / 96, 39 / 96, 46 / 96, 22 / 96, 0.9, 3]                  # left tile: ends at 96, its interior right side
    b[1, 2] = [23 / 96, 57 / 96, 46 / 96, 22 / 96, 0.85, 3]                 # right tile: starts at 0, its interior left side
    b[2, 3] = [40 / 96, 24 / 96, 30 / 96, 20 / 96, 0.8, 3]                  # the level of half the size: x 25..55, y 14..34
    tiles, levels, cap = [(0, 0, 0, 0), (0, 0, 64, 0), (0, 0, 0, 1)], [(96, 160), (48, 80)], 8
    whole = [80 / 160, 48 / 96, 60 / 160, 40 / 96]
    frags = [[73 / 160, 39 / 96, 46 / 160, 22 / 96], [(23 + 64) / 160, 57 / 96, 46 / 160, 22 / 96]]
    assert all(0.3 < _iou(f, whole) < iou_thr for f in frags) and _iou(*frags) < iou_thr
    buf, count = run_collect_ex(L, b, tiles, levels, 1, t, t, 0.5, margin, cap, fill=0)
    assert count.tolist() == [kept]
    got = buf[:cap * 24].view(F32).reshape(1, cap, 6).copy()
    np.testing.assert_array_equal(bits(got[0, :kept]), bits(np_collect_ex(b, tiles, levels, 1, t, t, 0.5, margin)[0]))
    np.testing.assert_allclose(got[0, kept - 1, :4], whole, rtol=2 ** -22)     # the coarse level's row is the whole box, in the frame
    keep, n = yt.nms_indices(torch.from_numpy(got).cuda(), iou_thr, 0.5, "center")
    assert int(n[0]) == kept
    order = keep[0, :kept].cpu().tolist()
    assert order == ([0, 1, 2] if kept == 3 else [0])                        # by score: 0.9, 0.85, 0.8 / the whole one alone
    last = got[0, order[-1]]
    assert last[4] == F32(0.8) and last[5] == F32(3)                           # score and class of the coarse level's row


# ------------------------------------------------------------------------------------------ 4.-6. end to end
OVERLAP, BATCH, CAP = (16, 32), 4, 1024


def _model(yt, seed=11):
    m = yt.YOLOv3(num_classes=80)
    m.load_state_dict(onet.synth_state_dict(seed, 3, 80, gain=gi.NET_GAIN))
    return m.cuda().eval()


def _images():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in FRAMES_HW]


def _anchors(yt):
    return [a.cuda() for a in yt.scaled_anchors(gi.COCO_ANCHORS, TH, TW)]


def _composition(yt, m, images, sa, scales):
    """resize_linear_u8 + numpy tiles per (frame, level) -> model(x) at detect_tiled's chunking -> decode_boxes(mutate=False) ->
    per tile decoded boxes (T, N, 6), with the tile table, the level table and the number of tiles per (frame, level)."""
    xs, tiles, levels, per_level = [], [], [], []
    for f, img in enumerate(images):
        for (lh, lw), origins in yt.tile_pyramid(img.shape[0], img.shape[1], (TH, TW), OVERLAP, scales):
            origins = origins.tolist()
            xs.append(np_level_tiles(img, lh, lw, origins, TH, TW))
            tiles += [(f, y0, x0, len(levels)) for y0, x0 in origins]
            levels.append((lh, lw))
            per_level.append(len(origins))
    x = torch.from_numpy(np.concatenate(xs)).cuda()
    decoded = []
    for s in range(0, x.shape[0], BATCH):
        with torch.no_grad():
            preds = m(x[s:s + BATCH].contiguous())
        decoded.append(torch.cat([yt.decode_boxes(p.float(), a, mutate=False) for p, a in zip(preds, sa)], 1))
    return torch.cat(decoded).cpu().numpy(), tiles, levels, per_level


def _pick_threshold(boxes, tiles, n_images):
    """From the composition's own scores: the smaller of the images' 97th percentiles (so every image has candidates), moved to the
    middle between that score and the next one above it: no score of any tile equals the threshold (asserted)."""
    per_image = [np.concatenate([boxes[t, :, 4] for t, tl in enumerate(tiles) if tl[0] == f]) for f in range(n_images)]
    q = min(np.quantile(s.astype(np.float64), 0.97, method="lower") for s in per_image)
    scores = np.unique(boxes[..., 4].astype(np.float64))
    above = scores[scores > q]
    thr = float((q + above[0]) / 2)
    assert q < thr < above[0] and not (scores == thr).any()
    return thr


def _check_end_to_end(yt, m):
    images, sa, scales, margin = _images(), _anchors(yt), (1.0, 0.5), 2.0
    boxes, tiles, levels, per_level = _composition(yt, m, images, sa, scales)
    assert levels == [(150, 203), (75, 102), (45, 70), (22, 35)] and per_level == [9, 4, 1, 1]
    # chunks of 4 tiles: tiles 8..11 span the level boundary of frame 0 (8 | 9), tiles 12..14 the frame boundary (12 | 13) and the
    # level boundary of frame 1 (13 | 14); the last chunk is short
    assert BATCH == 4 and 8 < per_level[0] < 12 and 12 < per_level[0] + per_level[1] < 15 == sum(per_level)
    thr = _pick_threshold(boxes, tiles, 2)
    want = np_collect_ex(boxes, tiles, levels, 2, TH, TW, thr, margin)
    n_want = [len(w) for w in want]
    n_off = [len(w) for w in np_collect_ex(boxes, tiles, levels, 2, TH, TW, thr, -1.0)]
    print("threshold", thr, "candidates", n_want, "without the seam test", n_off)
    assert all(0 < n < CAP for n in n_want) and n_want[0] < n_off[0] and n_want[1] == n_off[1]      # frame 1 has single tiles only
    ref = np.zeros((2, CAP, 6), F32)
    for f, w in enumerate(want):
        ref[f, :len(w)] = w
    keep_ref, count_ref = yt.nms_indices(torch.from_numpy(ref).cuda(), 0.45, thr, "center")
    cand, keep, count, ncand = yt.detect_tiled(m, images, sa, tile=(TH, TW), overlap=OVERLAP, iou_threshold=0.45, obj_threshold=thr,
                                               batch=BATCH, max_candidates=CAP, scales=scales, edge_margin=margin)
    assert tuple(cand.shape) == (2, CAP, 6) and tuple(keep.shape) == (2, CAP) and keep.dtype == torch.int32
    assert ncand.dtype == torch.int32 and ncand.cpu().tolist() == n_want
    assert torch.equal(count.cpu(), count_ref.cpu()) and int(count.min()) > 0
    got = cand.cpu().numpy()
    for f, w in enumerate(want):
        np.testing.assert_array_equal(bits(got[f, :len(w)]), bits(w))
        assert not got[f, len(w):].any()                                     # zero rows behind the candidates
        k = int(count[f])
        assert torch.equal(keep[f, :k].cpu(), keep_ref[f, :k].cpu())
    assert m._engine._defer_nan is False and m._engine._pending_flag is None
    return images, sa, thr, n_want, n_off


def test_detect_tiled_pyramid_equals_composition_fp32(yt):
    m = _model(yt)
    images, sa, thr, n_want, n_off = _check_end_to_end(yt, m)
    # max_candidates counts a frame's candidates over all its levels
    with pytest.raises(ValueError, match=f"image 0 has {n_want[0]} candidates.*{n_want[0] - 1}"):
        yt.detect_tiled(m, images, sa, tile=(TH, TW), overlap=OVERLAP, obj_threshold=thr, batch=BATCH, max_candidates=n_want[0] - 1,
                        scales=(1.0, 0.5), edge_margin=2.0)
    # the pyramid without the seam test: the candidates of the restatement at edge_margin < 0
    off = yt.detect_tiled(m, images, sa, tile=(TH, TW), overlap=OVERLAP, obj_threshold=thr, batch=BATCH, max_candidates=CAP,
                          scales=(1.0, 0.5))
    assert off[3].cpu().tolist() == n_off


def test_detect_tiled_pyramid_equals_composition_bf16(yt):
    """The model's 16-bit compute mode: both sides go through the same model(x), so the equalities stay bit for bit."""
    m = _model(yt)
    m._engine.compute_dtype = "bf16"
    _check_end_to_end(yt, m)


def test_single_tile_level_agrees_with_detect_images(yt):
    """At scale 0.25 the 150 x 203 frame is a 38 x 51 level, one zero-padded tile with no interior side (edge_margin changes
    nothing). detect_tiled's candidates are the rows of detect_images on resize_linear_u8(frame) padded to the tile that are above
    the threshold and whose centre is inside the level, in order; classes and scores equal; coordinates are detect_images' times
    tile / level within 2^-23 relative ((cx 96 + 0) / 51 is two roundings of less than 2^-24 each); the same number kept as by
    nms_indices on those rows."""
    m = _model(yt)
    img = _images()[0]
    sa = _anchors(yt)
    (lh, lw), origins = yt.tile_pyramid(150, 203, (TH, TW), OVERLAP, (0.25,))[0]
    assert (lh, lw) == (38, 51) and origins.tolist() == [[0, 0]]
    x = torch.from_numpy(np_level_tiles(img, lh, lw, [(0, 0)], TH, TW)).cuda()
    scores = yt.detect_images(m, x, sa, 0.45, 0.0, "center")[0][0, :, 4].cpu().numpy()
    thr = float(np.quantile(scores.astype(np.float64), 0.8, method="lower"))
    boxes, _, _ = yt.detect_images(m, x, sa, 0.45, thr, "center")
    rows = boxes[0].cpu().numpy()
    inside = ((rows[:, 0] * F32(TW) + F32(0)) / F32(lw) <= F32(1)) & ((rows[:, 1] * F32(TH) + F32(0)) / F32(lh) <= F32(1))
    above = rows[:, 4].astype(np.float64) > thr
    assert (above & ~inside).any()                                            # some centres are in the padding
    rows = rows[above & inside]
    cand, tkeep, tcount, ncand = yt.detect_tiled(m, img, sa, tile=(TH, TW), overlap=OVERLAP, iou_threshold=0.45, obj_threshold=thr,
                                                 batch=BATCH, max_candidates=CAP, scales=(0.25,), edge_margin=2.0)
    n = int(ncand[0])
    assert 0 < n == len(rows) < CAP
    got = cand[0, :n].cpu().numpy()
    np.testing.assert_array_equal(bits(got[:, 4:6]), bits(rows[:, 4:6]))
    want = rows[:, :4].astype(np.float64) * np.array([TW / lw, TH / lh, TW / lw, TH / lh])
    err = np.abs(got[:, :4].astype(np.float64) - want) / np.abs(want)
    print("largest relative coordinate difference", err.max(), "of", 2.0 ** -23)
    assert err.max() <= 2.0 ** -23
    ref = np.zeros((1, CAP, 6), F32)
    ref[0, :n] = rows
    _, count = yt.nms_indices(torch.from_numpy(ref).cuda(), 0.45, thr, "center")
    assert int(tcount[0]) == int(count[0]) > 0


def test_defaults_are_the_native_resolution_call(yt):
    """scales=(1.0,), edge_margin=None spelled out: the bytes of the call without them."""
    m = _model(yt)
    images, sa = _images(), _anchors(yt)
    kw = dict(tile=(TH, TW), overlap=OVERLAP, iou_threshold=0.45, obj_threshold=0.0, batch=BATCH, max_candidates=4096)
    a = yt.detect_tiled(m, images, sa, **kw)
    b = yt.detect_tiled(m, images, sa, scales=(1.0,), edge_margin=None, **kw)
    n = a[3].cpu().tolist()
    assert n[0] == 9 * 378 and 0 < n[1] < 378               # every sigmoid is above 0; centres in frame 1's padding are out
    for k in (0, 2, 3):                                        # boxes, count, candidates: every byte
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k])
    for f in range(2):                                         # keep is defined up to count
        c = int(a[2][f])
        assert c > 0 and torch.equal(a[1][f, :c], b[1][f, :c])
