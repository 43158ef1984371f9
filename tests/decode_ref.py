"""fp64 restatement of ``cells_to_boxes`` (code/utils.py:86-148) per axis, the inputs of
tests/test_gpu_decode_edges.py, and the fp32-vs-fp64 error its tolerance is built from. Tied to the oracle and to
``torch.argmax`` by tests/test_decode_ref_host.py. Everything here is torch and runs on whatever device its input is on.

What the restatement keeps of the fp32 operation, because it is part of its definition and not of its rounding:
  * ``1 / grid_size`` is a Python float that the multiply casts to fp32: inv_w = fp32(1 / gw), inv_h = fp32(1 / gh);
  * the anchors are the fp32 values the kernel receives;
  * the write-back ``exp(t) * anchor`` is stored in the fp32 prediction before it is scaled: where it overflows fp32 the
    box value is the infinity, whatever inv * (exp(t) * anchor) is in fp64.
"""
import functools
import zlib

import numpy as np
import torch

FLT_MIN = float(np.finfo(np.float32).tiny)
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------- class index
def first_max(scores):
    """Index of the sequential first maximum along the last axis, NaN counting as the maximum: the first NaN if there is
    one, else the first of the largest values (0 when all are -inf)."""
    nan = torch.isnan(scores)
    masked = torch.where(nan, torch.full_like(scores, -INF), scores)
    top = masked.amax(-1, keepdim=True)
    k = torch.arange(scores.shape[-1], device=scores.device).expand(scores.shape)
    big = scores.shape[-1]
    first_top = torch.where(masked == top, k, big).amin(-1)
    first_nan = torch.where(nan, k, big).amin(-1)
    return torch.where(nan.any(-1), first_nan, first_top)


def first_max_loop(row):
    """The same for one list of Python floats, as the loop it describes."""
    best, bv = 0, row[0]
    for k in range(1, len(row)):
        v = row[k]
        if v > bv or (v != v and bv == bv):
            best, bv = k, v
    return best


# ---------------------------------------------------------------------------------------------- the operation
def _grids(p):
    _, _, gh, gw, _ = p.shape
    col = torch.arange(gw, device=p.device, dtype=p.dtype).view(1, 1, 1, gw)
    row = torch.arange(gh, device=p.device, dtype=p.dtype).view(1, 1, gh, 1)
    return gh, gw, col, row


def decode_ref64(pred, anchors):
    """(boxes (B, 3 gh gw, 6), mutated prediction (B, 3, gh, gw, 5 + nc), class index (B, 3, gh, gw)) in fp64 of an fp32
    prediction (B, 3, gh, gw, 5 + nc) and fp32 anchors (3, 2) in grid cells, is_pred = True."""
    p = pred.double()
    B = p.shape[0]
    gh, gw, col, row = _grids(p)
    a = torch.as_tensor(anchors, device=p.device).double().reshape(1, 3, 1, 1, 2)
    inv_w, inv_h = float(np.float32(1.0 / gw)), float(np.float32(1.0 / gh))
    sx, sy = torch.sigmoid(p[..., 0]), torch.sigmoid(p[..., 1])
    w, h = torch.exp(p[..., 2]) * a[..., 0], torch.exp(p[..., 3]) * a[..., 1]
    mutated = p.clone()
    mutated[..., 0], mutated[..., 1], mutated[..., 2], mutated[..., 3] = sx, sy, w, h

    def scaled(inv, v):                                   # the stored fp32 value is what is scaled: its overflow stays
        v32 = v.float().double()
        return torch.where(torch.isinf(v32), v32, inv * v)
    cls = first_max(p[..., 5:])
    boxes = torch.stack([inv_w * (sx + col), inv_h * (sy + row), scaled(inv_w, w), scaled(inv_h, h), torch.sigmoid(p[..., 4]),
                         cls.double()], -1)
    return boxes.reshape(B, 3 * gh * gw, 6), mutated, cls


def decode_fp32(pred, anchors):
    """The oracle's fp32 evaluation (oracle.postprocess.cells_to_boxes: the same torch operations in the same order) with
    per-axis grids; for gh == gw its bits. Returns (boxes, mutated prediction); the argument is left alone."""
    p = pred.clone()
    B = p.shape[0]
    gh, gw, _, _ = _grids(p)
    anchors = torch.as_tensor(anchors, device=p.device, dtype=torch.float32)
    box = p[..., :4]
    box[..., 0:2] = torch.sigmoid(box[..., 0:2])
    box[..., 2:] = torch.exp(box[..., 2:]) * anchors.reshape(1, 3, 1, 1, 2)
    obj = torch.sigmoid(p[..., 4:5])
    cls = torch.argmax(p[..., 5:], dim=-1).unsqueeze(-1)
    col = torch.arange(gw, device=p.device).view(1, 1, 1, gw, 1)
    row = torch.arange(gh, device=p.device).view(1, 1, gh, 1, 1)
    inv_w, inv_h = 1 / gw, 1 / gh
    out = torch.cat((inv_w * (box[..., 0:1] + col), inv_h * (box[..., 1:2] + row), inv_w * box[..., 2:3], inv_h * box[..., 3:4],
                     obj, cls), dim=-1)
    return out.reshape(B, 3 * gh * gw, 6), p


def targets_fp32(t):
    """is_pred = False on (B, 3, gh, gw, 6) targets: plain numpy fp32, one rounding per operation (what the unit, built
    with -ffp-contract=off, must give bit for bit)."""
    t = np.asarray(t, np.float32)
    B, _, gh, gw, _ = t.shape
    inv_w, inv_h = np.float32(1.0 / gw), np.float32(1.0 / gh)
    col = np.arange(gw, dtype=np.float32).reshape(1, 1, 1, gw)
    row = np.arange(gh, dtype=np.float32).reshape(1, 1, gh, 1)
    out = np.stack([inv_w * (t[..., 0] + col), inv_h * (t[..., 1] + row), inv_w * t[..., 2], inv_h * t[..., 3], t[..., 4], t[..., 5]], -1)
    return out.astype(np.float32).reshape(B, 3 * gh * gw, 6)


# ---------------------------------------------------------------------------------------------- inputs, seeded by the case
def _rng(*case):
    return np.random.Generator(np.random.PCG64(zlib.crc32(repr(case).encode())))


def anchors_of(*case):
    """(3, 2) fp32 anchors in grid cells, in [1, 4): at least 1, so that e^89 * anchor overflows fp32 wherever e^89 does and
    the planted +-89 have one answer in fp32 and in fp64."""
    return (1.0 + 3.0 * _rng("anchors", *case).random((3, 2))).astype(np.float32)


def gaussian_pred(B, gh, gw, nc, *case):
    """1.5 N(0, 1), like tests/golden_inputs.decode_input"""
    return _rng("pred", B, gh, gw, nc, *case).standard_normal((B, 3, gh, gw, 5 + nc), dtype=np.float32) * np.float32(1.5)


def quarter_bounds(nc):
    """(last class of quarter q, first class of quarter q + 1) for q = 0, 1, 2 of the kernel's split (per = ceil(nc / 4))"""
    per = (nc + 3) // 4
    return [((q + 1) * per - 1, (q + 1) * per) for q in range(3) if (q + 1) * per < nc]


def score_patterns(nc):
    """[(name, how)], one cell each: `rest` first replaces every Gaussian score of the cell, `set` entries replace the
    score of a class, `add` entries are added to it."""
    pats = [("max@%d" % k, dict(add={k: 20.0})) for k in range(nc)]
    pats += [("tie@%d|%d" % ab, dict(set={ab[0]: 16.0, ab[1]: 16.0})) for ab in quarter_bounds(nc)]
    pats += [("all-equal", dict(rest=0.25)), ("all-neg-inf", dict(rest=-INF)),
             ("one-finite", dict(rest=-INF, set={nc // 2: -3.0})), ("inf-twice", dict(set={nc // 3: INF, nc - 1: INF}))]
    pats += [("nan@%d" % k, dict(set={k: NAN})) for k in range(nc)]
    pats += [("two-nans", dict(set={nc // 2: NAN, nc - 1: NAN})), ("inf-then-nan", dict(set={0: INF, nc - 1: NAN})),
             ("nan-then-inf", dict(set={0: NAN, nc - 1: INF}))]
    return pats


def planted_scores(nc):
    """(prediction (1, 3, gh, 8, 5 + nc), pattern names): cell i of the flattened (a, row, col) order holds pattern i, the
    cells behind the last pattern stay Gaussian."""
    pats = score_patterns(nc)
    gw = 8
    gh = -(-len(pats) // (3 * gw))
    pred = gaussian_pred(1, gh, gw, nc, "planted-scores")
    flat = pred.reshape(-1, 5 + nc)
    for i, (_, p) in enumerate(pats):
        if "rest" in p:
            flat[i, 5:] = p["rest"]
        for k, v in p.get("set", {}).items():
            flat[i, 5 + k] = v
        for k, v in p.get("add", {}).items():
            flat[i, 5 + k] += np.float32(v)
    return pred, [n for n, _ in pats]


BOX_PLANTS = (0.0, 20.0, -20.0, 89.0, -89.0, NAN)


def planted_boxes(nc=3):
    """(1, 3, 2, 5, 5 + nc): cell 6 c + j holds BOX_PLANTS[j] in channel c (x, y, w, h, objectness). e^89 overflows fp32 and
    e^-89 is below its normal range; 20 is where the fp32 sigmoid has lost all but a few bits of 1 - s."""
    pred = gaussian_pred(1, 2, 5, nc, "planted-boxes")
    flat = pred.reshape(-1, 5 + nc)
    for c in range(5):
        for j, v in enumerate(BOX_PLANTS):
            flat[6 * c + j, c] = v
    return pred


NC_SWEEP = (1, 2, 3, 4, 5, 7, 8, 9, 32, 33, 36, 37, 64, 65, 69, 91, 92, 93, 251)
SWEEP_GEOMS = ((1, 3, 5), (1, 4, 16))                      # 45 cells: one ragged tile, scalar staging; 192: three full tiles
PLANTED_NC = (3, 5, 37, 80)
GEOMS = ((1, 1, 1), (1, 1, 7), (1, 7, 1), (1, 3, 7), (1, 5, 13), (5, 3, 3), (2, 19, 11))
GEOM_NC = 5
LAYOUT_GEOMS = ((2, 3, 5), (1, 4, 16))
LAYOUT_NC = 5
# yolo_decode3*: (name, batch, input height, input width, nc); the grids are the input over 32, 16 and 8
DECODE3_CASES = (("32x32", 1, 32, 32, 5), ("96x64", 3, 96, 64, 5), ("64x64", 4, 64, 64, 80), ("128x128", 4, 128, 128, 2))


def decode3_grids(h, w):
    return [(h // s, w // s) for s in (32, 16, 8)]


def host_inputs():
    """Every (prediction, anchors) of test_gpu_decode_edges.py that is generated on the host (all but the 1.1 M-cell index case)"""
    for nc in NC_SWEEP:
        for g in SWEEP_GEOMS:
            yield gaussian_pred(*g, nc, "sweep"), anchors_of("sweep", g, nc)
    for nc in PLANTED_NC:
        yield planted_scores(nc)[0], anchors_of("planted-scores", nc)
    yield planted_boxes(), anchors_of("planted-boxes")
    for g in GEOMS:
        yield gaussian_pred(*g, GEOM_NC, "geometry"), anchors_of("geometry", g)
    for g in LAYOUT_GEOMS:
        yield gaussian_pred(*g, LAYOUT_NC, "layout"), anchors_of("layout", g)
    for name, b, h, w, nc in DECODE3_CASES:
        for k, (gh, gw) in enumerate(decode3_grids(h, w)):
            yield gaussian_pred(b, gh, gw, nc, "decode3", name, k), anchors_of("decode3", name, k)


def rel_error(got, want64):
    """largest |got - want| / |want| over the finite values whose reference is a normal fp32 number"""
    want64 = want64.double()
    ok = torch.isfinite(want64) & (want64.abs() >= FLT_MIN) & torch.isfinite(got)
    if not bool(ok.any()):
        return 0.0
    return float(((got.double() - want64).abs()[ok] / want64.abs()[ok]).max())


@functools.lru_cache(maxsize=None)
def decode_fp32_rel_error():
    """Largest relative error of the oracle's fp32 evaluation (box values 0..4 and the write-back) against the fp64
    restatement over host_inputs(). The kernel's hardware exp and reciprocal come on top of this figure."""
    worst = 0.0
    for pred, anchors in host_inputs():
        p = torch.from_numpy(pred)
        b32, m32 = decode_fp32(p, anchors)
        b64, m64, _ = decode_ref64(p, anchors)
        worst = max(worst, rel_error(b32[..., :5], b64[..., :5]), rel_error(m32[..., :4], m64[..., :4]))
    return worst
