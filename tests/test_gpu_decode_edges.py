"""GPU tests (``-m gpu``) of the box decode (decode.hip) against the fp64 restatement of tests/decode_ref.py (tied to the
oracle and to torch.argmax by tests/test_decode_ref_host.py), called through the C ABI at the edges of its geometry:

  entry point                         kernel          cases
  a  yolo_decode_hw                   decode_kernel   19 class counts (empty quarters, the 8-wide score loop once and twice,
                                                      a second trip of the tile staging, the 64 KiB tile) x {45 cells, scalar
                                                      staging; 192 cells, vector staging}; 252 classes refused
  b  yolo_decode_hw                   decode_kernel   planted scores (every maximum position, ties across the quarters, +-inf,
                                                      NaN) staged and unstaged; planted 0, +-20, +-89, NaN in x, y, w, h, obj
  c  yolo_decode_hw                   decode_kernel   1 to 2 x 3 x 19 x 11 cells, tiles across anchors and images; targets
                                                      (is_pred = 0) bit for bit; 1.1 M and 0.2 M cells for the magic division
                                                      and its correction step
  d  yolo_decode_hw                   decode_kernel   aligned, 4 bytes off, the permuted reference view, padded cells, batch
                                                      stride 0
  e  yolo_decode_hw                   decode_kernel   what is_pred = 1 / 2 may write; box_offset and n_total
  f  yolo_decode3_hw / _ex / decode3  decode3_kernel  five forwards against three single launches bit for bit, mixed layouts,
                                                      write_back 0 / 1, the argument errors

Tolerance: box values 0..4 and the write-back against the restatement rounded to fp32 with rtol = 4 x
decode_fp32_rel_error() (the oracle's own fp32 error against the restatement over these inputs, about 1.4e-7; the factor is
the suite's allowance for the hardware exp and reciprocal, as for Mish) and atol = 1e-7 (the suite's value for decode, which
also absorbs results below the normal range); NaNs where the reference has them, infinities equal, classes exact. Every
boxes buffer is pre-filled with a sentinel and every buffer the kernel may write is followed (and, where it starts off its
allocation, preceded) by 0xA5 bytes that must come back unchanged. All data is seeded from the case tuple; every measured
maximum is printed (run with -s). Cell indices near 2^31 are not reached: the box buffer alone would be 48 GB.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests import decode_ref as D

pytestmark = pytest.mark.gpu

SENT = -12288.0
GUARD = 256
ATOL = 1e-7
YOLO_OK, YOLO_ERR_ARG, YOLO_ERR_UNSUPPORTED = 0, -1, -2
LAYOUTS = ["aligned", "off4", "permuted", "padded"]


@pytest.fixture(scope="module")
def L():
    from yolo_for_turbines_amd import _lib
    _lib.lib()                        # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


@pytest.fixture(scope="module")
def rtol():
    """4x the oracle's fp32 error against the restatement (measured, see the host test)"""
    r = 4.0 * D.decode_fp32_rel_error()
    print(f"decode rtol = 4 x {r / 4:.3e}")
    return r


def _sync():
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- buffers
class Buf:
    """`nbytes` of device memory `front` bytes into an allocation, 0xA5 before and behind it"""

    def __init__(self, nbytes, front=0):
        assert front % 4 == 0
        self.raw = torch.full((front + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.front, self.nbytes = front, nbytes
        self.f32 = self.raw[front:front + nbytes].view(torch.float32)

    def guards_ok(self):
        return bool((self.raw[:self.front] == 0xA5).all()) and bool((self.raw[self.front + self.nbytes:] == 0xA5).all())


class Pred:
    """A prediction (B, 3, gh, gw, D) on the device in one of the layouts of part d, with the bytes the kernel must not touch"""

    def __init__(self, pred, layout, B=None):
        p = torch.from_numpy(np.ascontiguousarray(pred))
        b, _, gh, gw, Dk = p.shape
        self.layout, self.host = layout, p
        if layout in ("aligned", "off4"):
            self.buf = Buf(p.numel() * 4, 4 if layout == "off4" else 0)
            self.view = self.buf.f32.view(p.shape)
        elif layout == "permuted":                        # (B, 3, D, gh, gw) memory, like model.py:147-148
            self.buf = Buf(p.numel() * 4)
            self.view = self.buf.f32.view(b, 3, Dk, gh, gw).permute(0, 1, 3, 4, 2)
        elif layout == "padded":                          # unit class stride, three more floats behind every cell
            self.buf = Buf(b * 3 * gh * gw * (Dk + 3) * 4)
            self.store = self.buf.f32.view(b, 3, gh, gw, Dk + 3)
            self.store.fill_(SENT)
            self.view = self.store[..., :Dk]
        elif layout == "bcast":                           # one image for the whole batch: stride 0
            assert b == 1
            self.buf = Buf(p.numel() * 4)
            self.view = self.buf.f32.view(p.shape).expand(B, 3, gh, gw, Dk)
            self.host = p.expand(B, 3, gh, gw, Dk).contiguous()
        else:
            raise ValueError(layout)
        (self.view[:1] if layout == "bcast" else self.view).copy_(p.cuda())
        assert (self.view.data_ptr() % 16 == 4) == (layout == "off4")
        assert self.view.is_contiguous() or layout not in ("aligned", "off4")

    def strides(self):
        return list(self.view.stride())

    def untouched_outside(self):
        ok = self.buf.guards_ok()
        if self.layout == "padded":
            ok = ok and bool((self.store[..., self.view.shape[-1]:] == SENT).all())
        return ok


class Boxes:
    def __init__(self, B, n_total):
        self.buf = Buf(B * n_total * 6 * 4)
        self.t = self.buf.f32.view(B, n_total, 6)
        self.t.fill_(SENT)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _decode(L, P, anchors, is_pred, boxes, box_offset=0, nc=None, expect=YOLO_OK):
    B, _, gh, gw, Dk = P.view.shape
    s = (C.c_int64 * 5)(*P.strides())
    anc = None if anchors is None else torch.as_tensor(anchors, dtype=torch.float32).reshape(3, 2).cuda()
    rc = L.lib().yolo_decode_hw(P.view.data_ptr(), s, L.ptr(anc), B, gh, gw, Dk - 5 if nc is None else nc, is_pred,
                                boxes.t.data_ptr(), boxes.t.shape[1], box_offset, L.current_stream())
    _sync()
    assert rc == expect, (rc, L.lib().yolo_last_error())
    return rc


def _close(got, want64, rtol, what):
    """got (fp32) against the fp64 reference rounded to fp32: NaN where it is NaN, infinities equal, the rest within
    atol + rtol |want|. Returns the largest error in units of that bound."""
    want = want64.float()
    got, want = got.cpu(), want.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaNs differ"
    inf = torch.isinf(got) | torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), f"{what}: infinities differ"
    fin = ~(inf | torch.isnan(want))
    err = (got.double() - want.double()).abs()[fin]
    bound = ATOL + rtol * want.double().abs()[fin]
    worst = float((err / bound).max()) if err.numel() else 0.0
    assert worst <= 1.0, f"{what}: error {worst:.3f} of the bound"
    return worst


def _check(L, rtol, pred, anchors, layout="aligned", is_pred=1, B=None, n_total=None, box_offset=0, tag=""):
    """One launch checked in full: boxes, class column, write-back, and everything that must stay as it was. Returns the boxes."""
    P = Pred(pred, layout, B)
    ref_in = P.host
    b, _, gh, gw, Dk = ref_in.shape
    n = 3 * gh * gw
    boxes = Boxes(b, n if n_total is None else n_total)
    _decode(L, P, anchors, is_pred, boxes, box_offset)
    b64, m64, _ = D.decode_ref64(ref_in, anchors)
    got = boxes.t[:, box_offset:box_offset + n]
    e_box = _close(got[..., :5], b64[..., :5], rtol, "boxes")
    assert torch.equal(got[..., 5].cpu().double(), b64[..., 5]), "class column"
    keep = torch.ones(boxes.t.shape[1], dtype=torch.bool)
    keep[box_offset:box_offset + n] = False
    assert bool((boxes.t[:, keep.cuda()] == SENT).all()), "rows outside [box_offset, box_offset + 3 gh gw) were written"
    assert boxes.buf.guards_ok(), "wrote past the box buffer"
    after = P.view.cpu()
    if is_pred == 1:
        e_wb = _close(after[..., :4], m64[..., :4], rtol, "write-back")
        assert _same_bits(after[..., 4:], ref_in[..., 4:]), "is_pred = 1 changed a channel past the fourth"
    else:
        e_wb = 0.0
        assert _same_bits(after, ref_in), "is_pred = 2 changed the prediction"
    assert P.untouched_outside(), "wrote outside the prediction's cells"
    print(f"decode {tag} {tuple(ref_in.shape)} {layout} is_pred {is_pred}: error / bound boxes {e_box:.3f}, write-back {e_wb:.3f}")
    return boxes.t.clone()


# =============================================================================================== a. class counts
@pytest.mark.parametrize("geom", D.SWEEP_GEOMS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("nc", D.NC_SWEEP)
def test_class_count_sweep(L, rtol, nc, geom):
    """Gaussian scores: every class wins somewhere, so a quarter that is skipped, read twice or cut short changes the class
    column of some of the 45 / 192 cells (45 cells: count != 64 D, scalar staging; 192: three full tiles, 16-byte loads, and a
    second trip of the unrolled-by-6 loop from nc = 92). nc = 251 is the largest tile the host accepts: 64 KiB exactly."""
    pred, anchors = D.gaussian_pred(*geom, nc, "sweep"), D.anchors_of("sweep", geom, nc)
    b1 = _check(L, rtol, pred, anchors, "aligned", 1, tag=f"nc {nc}")
    b2 = _check(L, rtol, pred, anchors, "aligned", 2, tag=f"nc {nc}")
    assert _same_bits(b1, b2)
    seen = torch.unique(b1[..., 5]).numel()
    assert seen >= min(nc, 2), "the inputs do not exercise the class index"


def test_252_classes_are_refused(L):
    """64 x 257 floats exceed the 64 KiB a workgroup can ask for: YOLO_ERR_UNSUPPORTED before any launch"""
    pred = D.gaussian_pred(1, 3, 5, 252, "sweep")
    P, boxes = Pred(pred, "aligned"), Boxes(1, 45)
    for is_pred in (1, 2):
        _decode(L, P, D.anchors_of("refused"), is_pred, boxes, expect=YOLO_ERR_UNSUPPORTED)
        assert L.lib().yolo_last_error()
    assert bool((boxes.t == SENT).all()) and boxes.buf.guards_ok()
    assert _same_bits(P.view.cpu(), P.host) and P.untouched_outside()


# =============================================================================================== b. planted values
@pytest.mark.parametrize("layout", ["aligned", "off4", "permuted"])
@pytest.mark.parametrize("nc", D.PLANTED_NC)
def test_planted_scores(L, rtol, nc, layout):
    """One cell per pattern (tests/decode_ref.score_patterns), through the LDS tile (vector and scalar staging) and unstaged
    from the permuted view (class stride gh gw). The expected classes are those torch.argmax gives (host test)."""
    pred, names = D.planted_scores(nc)
    boxes = _check(L, rtol, pred, D.anchors_of("planted-scores", nc), layout, 1, tag=f"planted scores nc {nc}")
    got = dict(zip(names, boxes[0, :len(names), 5].long().tolist()))
    want = dict(zip(names, torch.argmax(torch.from_numpy(pred)[..., 5:].reshape(-1, nc)[:len(names)], -1).tolist()))
    assert got == want, {k: (got[k], want[k]) for k in names if got[k] != want[k]}


@pytest.mark.parametrize("layout", ["aligned", "permuted"])
def test_planted_box_values(L, rtol, layout):
    """0, +-20, +-89 and NaN in each of x, y, w, h, objectness: e^89 is an infinity in w and h and makes the sigmoid exactly
    0 or 1; e^-89 is below the normal range (within atol of 0 whether or not it is flushed); a NaN stays in its own value."""
    pred, anchors = D.planted_boxes(), D.anchors_of("planted-boxes")
    for is_pred in (1, 2):
        boxes = _check(L, rtol, pred, anchors, layout, is_pred, tag="planted boxes")
        assert int(torch.isinf(boxes).sum()) == 2 and int(torch.isnan(boxes).sum()) == 5


# =============================================================================================== c. geometry
@pytest.mark.parametrize("geom", D.GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_geometry(L, rtol, geom):
    """1, 7, 7, 63, 195, 135 and 1254 cells per image set: tiles that end inside an anchor plane, span anchors and images"""
    pred, anchors = D.gaussian_pred(*geom, D.GEOM_NC, "geometry"), D.anchors_of("geometry", geom)
    for layout in ("aligned", "permuted"):
        _check(L, rtol, pred, anchors, layout, 1, tag="geometry")


@pytest.mark.parametrize("layout", ["aligned", "off4", "permuted", "padded"])
@pytest.mark.parametrize("geom", D.GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_targets_are_bit_exact(L, geom, layout):
    """is_pred = 0 on (B, 3, gh, gw, 6): inv * (v + col) in fp32, one rounding per operation, objectness and class copied"""
    t = D.gaussian_pred(*geom, 1, "targets")
    P = Pred(t, layout)
    boxes = Boxes(geom[0], 3 * geom[1] * geom[2])
    _decode(L, P, None, 0, boxes)
    assert _same_bits(boxes.t.cpu(), torch.from_numpy(D.targets_fp32(t)))
    assert boxes.buf.guards_ok() and _same_bits(P.view.cpu(), P.host) and P.untouched_outside()


def _umulhi_quotient(x, d):
    """pp_fdiv (decode.hip) before its correction: the high word of x * ceil(2^32 / d)"""
    return (x * ((2 ** 32 + d - 1) // d)) >> 32


def test_the_second_index_case_needs_the_correction_of_the_magic_division():
    """(11, 3, 65, 102): 3 gh gw = 19890, and for the last cell, 218789, the multiply-high quotient is 11, one more than
    218789 // 19890 = 10: a kernel without the `q * d > x` correction puts that box into an image that does not exist. Up to
    the 1,108,991 of the other case the three quotients (by 76, 5776, 17328) are exact without it."""
    assert 11 * 3 * 65 * 102 - 1 == 218789 and _umulhi_quotient(218789, 19890) == 11 and 218789 // 19890 == 10
    x = np.arange(64 * 3 * 76 * 76, dtype=np.uint64)
    assert all(np.array_equal((x[:n] * np.uint64((2 ** 32 + d - 1) // d)) >> np.uint64(32), x[:n] // np.uint64(d))
               for d, n in ((17328, x.size), (5776, 17328), (76, 5776)))


@pytest.mark.parametrize("B,gh,gw", [(64, 76, 76), (11, 65, 102)])
def test_index_arithmetic_at_many_cells(L, rtol, B, gh, gw):
    """nc = 1. (64, 3, 76, 76, 6): 1,108,992 cells, the three multiply-high divisions at dividends up to 2^20 with divisors 76,
    5776 and 17328; (11, 3, 65, 102, 6): 218,790 cells, whose last one needs the correction step of the division by
    3 gh gw. A wrong (b, a, row, col) moves a box to another row or adds another cell's column. Generated and referenced
    on the device, eight images at a time."""
    nc = 1
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(("many-cells", B, gh, gw)).encode()))
    anchors = D.anchors_of("many-cells", B, gh, gw)
    pred = torch.randn((B, 3, gh, gw, 5 + nc), generator=g, device="cuda") * 1.5
    before = pred.clone()
    n = 3 * gh * gw
    boxes = torch.full((B * n * 6 + GUARD // 4,), SENT, device="cuda")
    s = (C.c_int64 * 5)(*pred.stride())
    anc = torch.from_numpy(anchors).cuda()
    L.check(L.lib().yolo_decode_hw(pred.data_ptr(), s, anc.data_ptr(), B, gh, gw, nc, 1, boxes.data_ptr(), n, 0, L.current_stream()),
            "yolo_decode_hw")
    _sync()
    assert bool((boxes[B * n * 6:] == SENT).all())
    got = boxes[:B * n * 6].view(B, n, 6)
    worst = 0.0
    for b0 in range(0, B, 8):
        b64, m64, _ = D.decode_ref64(before[b0:b0 + 8], anc)
        for g32, w64 in ((got[b0:b0 + 8, :, :5], b64[..., :5]), (pred[b0:b0 + 8, ..., :4], m64[..., :4])):
            w = w64.float().double()
            worst = max(worst, float(((g32.double() - w).abs() / (ATOL + rtol * w.abs())).max()))
        assert bool((got[b0:b0 + 8, :, 5] == 0).all()) and torch.equal(pred[b0:b0 + 8, ..., 4:], before[b0:b0 + 8, ..., 4:])
    print(f"decode {B * n} cells: error / bound {worst:.3f}")
    assert worst <= 1.0


# =============================================================================================== d. layouts
@pytest.mark.parametrize("layout", LAYOUTS + ["bcast"])
@pytest.mark.parametrize("geom", D.LAYOUT_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_layouts_agree_with_the_reference(L, rtol, geom, layout):
    """The same data through the vector staging (aligned, (1, 4, 16) only: (2, 3, 5) has one ragged tile), the scalar staging
    (4 bytes off), and the unstaged path with class strides gh gw (permuted) and 1 (padded cells, batch stride 0)."""
    pred, anchors = D.gaussian_pred(*geom, D.LAYOUT_NC, "layout"), D.anchors_of("layout", geom)
    if layout == "bcast":
        _check(L, rtol, pred[:1], anchors, "bcast", 2, B=3, tag="layout")
        return
    want = _check(L, rtol, pred, anchors, "aligned", 1, tag="layout")
    for is_pred in (1, 2):
        assert _same_bits(_check(L, rtol, pred, anchors, layout, is_pred, tag="layout"), want)


# =============================================================================================== e. side effects
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom,off,extra", [((2, 3, 5), 7, 5), ((1, 4, 16), 64, 1), ((5, 3, 3), 1, 130)])
def test_box_offset_and_n_total(L, rtol, geom, off, extra, layout):
    """Rows [box_offset, box_offset + 3 gh gw) of every image are written and no other (checked in _check against the sentinel);
    the rows are those of a launch at offset 0, and is_pred = 2 gives the bits of is_pred = 1."""
    pred, anchors = D.gaussian_pred(*geom, D.LAYOUT_NC, "offset"), D.anchors_of("offset", geom)
    n = 3 * geom[1] * geom[2]
    want = _check(L, rtol, pred, anchors, "aligned", 1, tag="offset 0")
    for is_pred in (1, 2):
        got = _check(L, rtol, pred, anchors, layout, is_pred, n_total=off + n + extra, box_offset=off, tag=f"offset {off}")
        assert _same_bits(got[:, off:off + n], want)


# =============================================================================================== f. three scales in one launch
def _scales(name, b, h, w, nc, layouts):
    out = []
    for k, (gh, gw) in enumerate(D.decode3_grids(h, w)):
        out.append((D.gaussian_pred(b, gh, gw, nc, "decode3", name, k), D.anchors_of("decode3", name, k), layouts[k]))
    return out


def _decode3(L, entry, preds, anchors, grids, b, nc, write_back, boxes, n_total, expect=YOLO_OK, null_scale=None, null_anchor=None):
    lib = L.lib()
    ptrs = (C.c_void_p * 3)(*[None if k == null_scale else P.view.data_ptr() for k, P in enumerate(preds)])
    anc = [torch.as_tensor(a, dtype=torch.float32).reshape(3, 2).cuda() for a in anchors]
    aptr = (C.c_void_p * 3)(*[None if k == null_anchor else a.data_ptr() for k, a in enumerate(anc)])
    s15 = (C.c_int64 * 15)(*[v for P in preds for v in P.strides()])
    st = L.current_stream()
    if entry == "hw":
        hw6 = (C.c_int * 6)(*[v for g in grids for v in g])
        rc = lib.yolo_decode3_hw(ptrs, s15, aptr, hw6, b, nc, write_back, boxes.t.data_ptr(), n_total, st)
    else:
        assert all(gh == gw for gh, gw in grids)
        g3 = (C.c_int * 3)(*[g[0] for g in grids])
        if entry == "ex":
            rc = lib.yolo_decode3_ex(ptrs, s15, aptr, g3, b, nc, write_back, boxes.t.data_ptr(), n_total, st)
        else:
            assert write_back == 1
            rc = lib.yolo_decode3(ptrs, s15, aptr, g3, b, nc, boxes.t.data_ptr(), n_total, st)
    _sync()
    assert rc == expect, (rc, lib.yolo_last_error())
    return rc


D3_PARAMS = [(c, ("aligned",) * 3) for c in D.DECODE3_CASES] + [(D.DECODE3_CASES[1], ("permuted", "off4", "padded")),
                                                                (D.DECODE3_CASES[0], ("padded", "permuted", "off4"))]


@pytest.mark.parametrize("write_back", [0, 1])
@pytest.mark.parametrize("case,layouts", D3_PARAMS, ids=[c[0] + "-" + "-".join(l) for c, l in D3_PARAMS])
def test_decode3_equals_three_launches_and_the_reference(L, rtol, case, layouts, write_back):
    """Cells per scale: 32x32 3, 12, 48 (three ragged tiles, one block each); 96x64 (B = 3) 54, 216, 864 (every scale ends
    inside a tile, the block-to-scale map at blocks 1 and 5); 64x64 (B = 4, nc = 80) 48, 192, 768 (the first scale is short of a
    tile, the others are whole tiles); 128x128 (B = 4) 192, 768, 3072: every scale whole tiles. The anchors differ per
    scale, and in the mixed cases so do strides and staging. Bit-equal to three yolo_decode_hw launches at the matching
    box_offset, boxes and write-back; within tolerance of the reference; square grids through all three entry points."""
    name, b, h, w, nc = case
    grids = D.decode3_grids(h, w)
    sc = _scales(name, b, h, w, nc, layouts)
    n_total = sum(3 * gh * gw for gh, gw in grids)
    # three single launches
    one, one_boxes = [Pred(p, lay) for p, _, lay in sc], Boxes(b, n_total)
    off = 0
    for P, (_, a, _), (gh, gw) in zip(one, sc, grids):
        _decode(L, P, a, 1 if write_back else 2, one_boxes, off)
        off += 3 * gh * gw
    entries = ["hw"] + (["ex"] + (["plain"] if write_back else []) if h == w else [])
    for entry in entries:
        three, boxes = [Pred(p, lay) for p, _, lay in sc], Boxes(b, n_total)
        _decode3(L, entry, three, [a for _, a, _ in sc], grids, b, nc, write_back, boxes, n_total)
        assert _same_bits(boxes.t, one_boxes.t), entry
        assert boxes.buf.guards_ok()
        off, worst = 0, 0.0
        for P, Q, (p, a, _), (gh, gw) in zip(three, one, sc, grids):
            assert _same_bits(P.view.cpu(), Q.view.cpu()) and P.untouched_outside()
            b64, m64, _ = D.decode_ref64(P.host, a)
            rows = boxes.t[:, off:off + 3 * gh * gw]
            worst = max(worst, _close(rows[..., :5], b64[..., :5], rtol, "boxes"))
            assert torch.equal(rows[..., 5].cpu().double(), b64[..., 5])
            after = P.view.cpu()
            if write_back:
                worst = max(worst, _close(after[..., :4], m64[..., :4], rtol, "write-back"))
                assert _same_bits(after[..., 4:], P.host[..., 4:])
            else:
                assert _same_bits(after, P.host)
            off += 3 * gh * gw
        print(f"decode3_{entry} {name} {layouts} write_back {write_back}: error / bound {worst:.3f}")


def _untouched(preds, boxes):
    return (bool((boxes.t == SENT).all()) and boxes.buf.guards_ok()
            and all(_same_bits(P.view.cpu(), P.host) and P.untouched_outside() for P in preds))


def test_decode3_argument_errors(L):
    """each: YOLO_ERR_ARG, a message, nothing written"""
    name, b, h, w, nc = D.DECODE3_CASES[0]
    grids = D.decode3_grids(h, w)
    sc = _scales(name, b, h, w, nc, ("aligned",) * 3)
    preds, anchors = [Pred(p, "aligned") for p, _, _ in sc], [a for _, a, _ in sc]
    n_total = sum(3 * gh * gw for gh, gw in grids)
    boxes = Boxes(b, n_total + 1)
    lib = L.lib()
    for entry in ("hw", "ex"):
        for kw, n, ncs in ((dict(), n_total + 1, nc), (dict(), n_total - 1, nc), (dict(null_scale=1), n_total, nc),
                           (dict(null_anchor=2), n_total, nc), (dict(), n_total, 0)):
            for wb in (0, 1):
                _decode3(L, entry, preds, anchors, grids, b, ncs, wb, boxes, n, expect=YOLO_ERR_ARG, **kw)
                assert b"decode3" in lib.yolo_last_error()
    _decode3(L, "plain", preds, anchors, grids, b, nc, 1, boxes, n_total + 1, expect=YOLO_ERR_ARG)
    assert b"decode3" in lib.yolo_last_error()
    assert _untouched(preds, boxes)


def test_decode_argument_errors(L):
    pred = D.gaussian_pred(1, 3, 5, 5, "errors")
    P, boxes = Pred(pred, "aligned"), Boxes(1, 50)
    a = D.anchors_of("errors")
    lib = L.lib()
    for kw in (dict(is_pred=0), dict(is_pred=0, nc=2), dict(is_pred=1, nc=0), dict(is_pred=1, box_offset=6), dict(is_pred=2, box_offset=-1),
               dict(is_pred=1, anchors=None), dict(is_pred=2, anchors=None)):
        kw = dict(dict(anchors=a, box_offset=0), **kw)
        _decode(L, P, kw["anchors"], kw["is_pred"], boxes, kw["box_offset"], nc=kw.get("nc"), expect=YOLO_ERR_ARG)
        assert b"decode" in lib.yolo_last_error()
    assert _untouched([P], boxes)
