"""(Test infrastructure.) The case tables of tests/test_gpu_wgrad_h16.py and a Python restatement of the launch plans of the 16-bit
weight-gradient kernels (plan_wgrad_h of wgrad_h16.hip, plan_wgrad_d of wgrad_dma_h16.hip, stem_wgrad_blocks of wgrad_stem_h16.hip,
plan_wgrad of wgrad_f32.hip) and of the routing of yolo_conv_wgrad. No project code, no GPU: tests/test_wgrad_plan_host.py compares
the restatement with yolo_wgrad_plan, the GPU test and tests/workers/wgrad_h16_cases.py assert each case's geometry with it.

A case is (N, H, W, cin, cout, k, s, x_ld, x_off, dz_ld, dz_off); its expectation (kernel, slices, G, empty trailing slices)."""
F32, PATCH, DMA, STEM = 0, 1, 2, 3          # YOLO_WGRAD_KERNEL_* of include/yolo_mi355x.h
KERNEL_NAMES = {F32: "wgrad_f32_kernel", PATCH: "wgrad_patch_h16", DMA: "wgrad3_dma_h16", STEM: "stem_wgrad_h16"}


def _ceil(a, b):
    return -(-a // b)


def _up(a, b):
    return _ceil(a, b) * b


def _fan_in(total4, ns, lim16, lim4):
    return 16 if total4 < lim16 and ns >= 32 else 4 if total4 < lim4 and ns >= 8 else 1


def plan_dma(n, h, w, cin, cout, la=3):
    tiles = _ceil(cout, 64) * _ceil(cin, 64)
    total = n * _ceil(h, 4) * _ceil(w, 16)
    ns = max(1, min(256 // tiles, _ceil(total, 8)))
    if ns >= 8:
        ns = ns // 8 * 8
    per = _ceil(total, ns)
    return [DMA, tiles, total, ns, per, _fan_in(tiles * 9 * 64 * 64 // 4, ns, 32768, 131072), ns - _ceil(total, per), la]


def plan_patch(n, h, w, cin, cout, k, s):
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    bm = 64 if k == 3 else 128
    tiles = _ceil(cout, bm) * _ceil(cin, bm)
    th = (4 if s == 1 else 2) if k == 3 else 2
    total = n * _ceil(ho, th) * _ceil(wo, 16) if k == 3 else _ceil(n * ho * wo, th * 16)
    ns = min(512, max(1, min(_ceil(512, tiles), max(1, _ceil(total, 8)))))
    if ns >= 8:
        ns = ns // 8 * 8
    per = _ceil(total, ns)
    return [PATCH, tiles, total, ns, per, _fan_in(cout * k * k * (_up(cin, 4) // 4), ns, 16384, 65536), ns - _ceil(total, per), 0]


def plan_stem(n, h, w, cap=256):
    segs = n * h * (w // 16)
    nblk = max(1, min(_ceil(segs, 64), cap))
    per = _ceil(segs, 4 * nblk)
    return [STEM, 1, segs, nblk, per, 8, nblk - _ceil(segs, 4 * per), 0]


def plan_f32(n, h, w, cin, cout, k, s):
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    cp = _up(cin, 4)
    small = cp == 4
    bm = 128 if cout > 64 else 64
    bn = 64 if small else (128 if cp > 64 else 64)
    tiles = _ceil(cout, bm) * (1 if small else k * k * _ceil(cp, bn))
    steps = _ceil(n * ho * wo, 32)
    ns = min(512, max(1, min(_ceil(1536, tiles), max(1, _ceil(steps, 8)))))
    per = _ceil(steps, ns)
    ns = _ceil(steps, per)
    return [F32, tiles, steps, ns, per, _fan_in(cout * k * k * (cp // 4), ns, 16384, 65536), 0, 0]


def route(case, sixteen_bit=True, no_dma=False, no_stem=False):
    """The kernel yolo_conv_wgrad picks, for arguments it accepts."""
    n, h, w, cin, cout, k, s, x_ld, x_off, dz_ld, dz_off = case
    by8 = not (dz_ld % 8 or dz_off % 8 or x_ld % 8 or x_off % 8)
    if not sixteen_bit or not by8:
        return F32
    if (not no_stem and k == 3 and s == 1 and cin <= 3 and cout <= 32 and x_ld == 8 and w % 16 == 0 and dz_ld - dz_off >= 32
            and n * h * w <= 0x7fffffff):
        return STEM
    covers = dz_ld >= _up(cout, 8) and x_ld >= _up(cin, 8)
    if not no_dma and k == 3 and s == 1 and cin >= 32 and covers:
        return DMA
    if covers and not (k == 1 and s != 1):
        return PATCH
    return F32


def plan(case, sixteen_bit=True, no_dma=False, no_stem=False, la=3, stem_cap=256):
    """What yolo_wgrad_plan fills into out8 for a case the call accepts."""
    n, h, w, cin, cout, k, s = case[:7]
    kern = route(case, sixteen_bit, no_dma, no_stem)
    if kern == STEM:
        return plan_stem(n, h, w, stem_cap)
    if kern == DMA:
        return plan_dma(n, h, w, cin, cout, la)
    if kern == PATCH:
        return plan_patch(n, h, w, cin, cout, k, s)
    return plan_f32(n, h, w, cin, cout, k, s)


def accepted(case):
    """The argument rules of yolo_conv_wgrad that need no pointer."""
    n, h, w, cin, cout, k, s, x_ld, x_off, dz_ld, dz_off = case
    if min(n, h, w, cin, cout) <= 0 or k not in (1, 3) or s not in (1, 2):
        return False
    if dz_ld % 4 or dz_off % 4 or x_ld % 4 or x_off % 4 or x_ld < _up(cin, 4) or dz_ld < _up(cout, 4) or dz_off < 0 or x_off < 0:
        return False
    return dz_off + cout <= dz_ld and x_off + cin <= x_ld


# ---- the case tables: (case, (kernel, slices, G, empty trailing slices)), what each is meant to reach
DMA_CASES = [
    ((1, 128, 128, 64, 64, 3, 1, 64, 0, 64, 0), (DMA, 32, 16, 0)),        # 32 slices of 8, wgrad_reduce_acc<16>, XCD map
    ((1, 128, 160, 64, 64, 3, 1, 64, 0, 64, 0), (DMA, 40, 16, 0)),        # 40 slices: remainder branch of the reduce's two-chain loop
    ((2, 20, 320, 64, 64, 3, 1, 64, 0, 64, 0), (DMA, 24, 4, 1)),          # 200 tiles, 24 slices of 9: one slice of 2, one empty; <4>
    ((1, 4, 16, 32, 32, 3, 1, 32, 0, 32, 0), (DMA, 1, 1, 0)),             # one K tile: K group 1 idle; half-empty 64-wide tile
    ((3, 9, 9, 40, 72, 3, 1, 96, 24, 160, 80), (DMA, 2, 1, 0)),           # both operands from slices; ragged channels; slices of 5 + 4
    ((1, 5, 17, 72, 136, 3, 1, 72, 0, 136, 0), (DMA, 1, 1, 0)),           # 6 dW tiles; H = 4 + 1, W = 16 + 1
    ((1, 52, 52, 128, 128, 3, 1, 128, 0, 128, 0), (DMA, 7, 1, 0)),        # 7 slices: linear map; 4 dW tiles; last slice 4
    ((2, 52, 52, 128, 128, 3, 1, 128, 0, 128, 0), (DMA, 8, 4, 0)),        # 8 slices of 13 (groups get 7 and 6); XCD map with 4 tiles
]
PATCH1_CASES = [
    ((1, 96, 96, 128, 128, 1, 1, 128, 0, 128, 0), (PATCH, 32, 16, 0)),    # 32 slices, wgrad_reduce<16>
    ((1, 80, 80, 256, 128, 1, 1, 256, 0, 128, 0), (PATCH, 24, 4, 1)),     # 24 slices, one empty; 2 dW tiles
    ((2, 26, 26, 128, 128, 1, 1, 384, 256, 128, 0), (PATCH, 6, 1, 0)),    # x from a route slice; 6 slices, linear map
    ((2, 7, 7, 512, 255, 1, 1, 512, 0, 256, 0), (PATCH, 1, 1, 0)),        # head: 255 outputs
    ((3, 10, 10, 256, 21, 1, 1, 256, 0, 64, 32), (PATCH, 2, 1, 0)),       # head: 21 outputs, dz from a slice
]
PATCH32_CASES = [
    ((1, 128, 128, 32, 64, 3, 2, 32, 0, 64, 0), (PATCH, 16, 4, 0)),       # 16 slices, wgrad_reduce<4>
    ((1, 41, 37, 72, 40, 3, 2, 72, 0, 40, 0), (PATCH, 3, 1, 0)),          # odd H and W, ragged channels, two ci tiles
    ((1, 1, 5, 64, 64, 3, 2, 64, 0, 64, 0), (PATCH, 1, 1, 0)),            # one row
]
PATCH31_CASES = [   # wgrad_patch_h16<T, 3, 1>: what the stem and dma kernels decline
    ((1, 128, 128, 16, 24, 3, 1, 16, 0, 24, 0), (PATCH, 32, 16, 0)),      # cin < 32
    ((2, 9, 20, 3, 32, 3, 1, 8, 0, 32, 0), (PATCH, 2, 1, 0)),             # W % 16 != 0; 2 slices of 6
    ((1, 13, 13, 3, 64, 3, 1, 8, 0, 64, 0), (PATCH, 1, 1, 0)),            # cout > 32
    ((3, 7, 48, 3, 24, 3, 1, 8, 0, 40, 16), (PATCH, 3, 1, 0)),            # fewer than 32 dz channels from dz_off to the end of the row
]
STEM_CASES = [
    ((1, 1, 16, 3, 32, 3, 1, 8, 0, 32, 0), (STEM, 1, 8, 0)),              # one K step, three idle waves
    ((1, 3, 16, 1, 32, 3, 1, 8, 0, 32, 0), (STEM, 1, 8, 0)),              # one input channel
    ((2, 32, 32, 3, 32, 3, 1, 8, 0, 32, 0), (STEM, 2, 8, 0)),             # waves that cross an image boundary
    ((3, 7, 48, 3, 24, 3, 1, 8, 0, 64, 32), (STEM, 1, 8, 0)),             # dz_off != 0, 24 outputs
    ((1, 65, 64, 3, 32, 3, 1, 8, 0, 32, 0), (STEM, 5, 8, 0)),             # 5 workgroups, 13 K steps per wave, ragged last batch
    ((3, 512, 480, 3, 32, 3, 1, 8, 0, 32, 0), (STEM, 256, 8, 0)),         # grid cap; 45 steps = 12 batches per wave: the ring wraps 4 times
]
TABLES = {"dma": DMA_CASES, "patch1": PATCH1_CASES, "patch32": PATCH32_CASES, "patch31": PATCH31_CASES, "stem": STEM_CASES}
ALL_CASES = [(f"{t}{i + 1}", c, e) for t, tab in TABLES.items() for i, (c, e) in enumerate(tab)]

# the cases of the kernels' first unit test (cin, cout, k, stride, H, W, N, dz_ld), kept as they were: offsets 0, x_ld = cin (8 for the stem)
LEGACY_CASES = [
    (64, 128, 3, 1, 13, 13, 2, 128), (32, 64, 3, 1, 20, 20, 1, 64), (128, 64, 3, 2, 16, 16, 2, 64), (64, 64, 3, 2, 26, 26, 1, 64),
    (256, 128, 1, 1, 13, 13, 3, 128), (128, 21, 1, 1, 10, 10, 2, 32), (96, 255, 1, 1, 7, 7, 1, 256), (192, 96, 3, 1, 19, 38, 1, 96),
    (64, 32, 1, 1, 52, 52, 1, 32), (512, 64, 3, 1, 5, 5, 4, 64),
    # wgrad3_dma_h16 (3x3 stride 1, cin >= 32): several K slices with the XCD-aware workgroup map and a ragged last
    # slice; one dW tile with 16 slices; channel counts that are not multiples of the 64-wide tile or of 16
    (128, 256, 3, 1, 52, 52, 4, 256), (64, 64, 3, 1, 104, 40, 2, 64), (40, 72, 3, 1, 9, 9, 3, 72), (96, 32, 3, 1, 17, 33, 5, 40),
    # stem_wgrad_h16 (first block: <= 3 input channels in an 8-channel 16-bit buffer, <= 32 output channels, W % 16 == 0):
    # every border, rows shorter than a batch of K steps, waves with ragged last batches, one input channel, 24 output channels
    (3, 32, 3, 1, 32, 32, 2, 32), (3, 32, 3, 1, 7, 48, 3, 32), (1, 32, 3, 1, 16, 16, 1, 32), (3, 24, 3, 1, 20, 64, 2, 40),
    (3, 32, 3, 1, 1, 16, 1, 32), (3, 32, 3, 1, 416, 416, 1, 32)]

# the switch variants run in a child process (tests/workers/wgrad_h16_cases.py): environment, case names, what the plan must say
SWITCHES = ("YOLO_NO_WGRAD_DMA", "YOLO_NO_STEM_WGRAD", "YOLO_WGRAD_LA", "YOLO_WGRAD_PRIO", "YOLO_STEM_WGRAD_BLOCKS")
VARIANTS = {
    "fallback": ({"YOLO_NO_WGRAD_DMA": "1", "YOLO_NO_STEM_WGRAD": "1"}, ["dma1", "dma3", "dma6", "stem3", "stem5"],
                 dict(no_dma=True, no_stem=True)),
    "tuned": ({"YOLO_WGRAD_LA": "5", "YOLO_WGRAD_PRIO": "1", "YOLO_STEM_WGRAD_BLOCKS": "1"}, ["dma3", "dma6", "dma8", "stem5"],
              dict(la=5, stem_cap=1)),
}


def by_name(name):
    return next((c, e) for nm, c, e in ALL_CASES if nm == name)
