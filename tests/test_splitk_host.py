"""YOLO_FLAG_SPLIT_K on the host (nothing is launched): what the library says it supports, the slice count, the workspace formula of
include/yolo_mi355x.h, the return codes of descriptors that are refused before any launch, and ModelState.latency."""
import copy
import ctypes as C
import pickle

import pytest

OK, ERR_ARG, ERR_UNSUPPORTED, ERR_LAUNCH, ERR_WORKSPACE = 0, -1, -2, -3, -4
FAKE = 1 << 20          # a non-null "device pointer" for calls that must return before they launch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def _desc(L, cout, cin, k, s, h=13, w=None, n=2, dtype=None, flags=0, tile=0):
    return L.ConvDesc(n=n, h=h, w=h if w is None else w, cin=cin, cout=cout, ksize=k, stride=s, x_ld=(cin + 3) // 4 * 4, y_ld=cout,
                      dtype=L.F32 if dtype is None else dtype, flags=flags, tile=tile)


def _slices(h, w, cin, cout, k, s):
    """The rule of conv_splitk_f32.hip restated: the smallest S <= 32 that gives a batch-1 launch 512 workgroups of 64 x 64, at least
    4 K steps of 32 per slice, no empty slice."""
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    tiles = -(-ho * wo // 64) * -(-cout // 64)
    kt = k * k * cin // 32
    steps = max(4, -(-kt // min(32, -(-512 // tiles))))
    return -(-kt // steps)


SHAPES = [(384, 32, 1, 1, 5, 5), (24, 96, 1, 1, 13, 13), (255, 256, 1, 1, 13, 13), (64, 512, 3, 1, 13, 13), (256, 32, 3, 1, 1, 40),
          (96, 32, 3, 2, 7, 9), (1024, 512, 3, 1, 13, 13), (512, 1024, 1, 1, 19, 19), (256, 128, 3, 1, 52, 52), (64, 32, 3, 2, 416, 416)]


@pytest.mark.parametrize("cout,cin,k,s,h,w", SHAPES)
def test_supported_eligible_slices_look_at_the_shape_only(built, cout, cin, k, s, h, w):
    L = built
    lib = L.lib()
    d = _desc(L, cout, cin, k, s, h, w)
    assert lib.yolo_conv_splitk_supported(d) == 1
    S = lib.yolo_conv_splitk_slices(d)
    assert S == _slices(h, w, cin, cout, k, s) and 1 <= S <= 32
    el = lib.yolo_conv_splitk_eligible(d)
    assert el in (0, 1)
    for n, flags, tile in ((1, 0, 0), (64, L.FLAG_SPLIT_K, 0), (7, L.FLAG_SPLIT_BF16 | L.FLAG_RESIDUAL, 4), (3, L.FLAG_FILTERS_READY, 15)):
        e = _desc(L, cout, cin, k, s, h, w, n=n, flags=flags, tile=tile)
        assert lib.yolo_conv_splitk_supported(e) == 1
        assert lib.yolo_conv_splitk_slices(e) == S
        assert lib.yolo_conv_splitk_eligible(e) == el


def test_one_k_step_is_one_slice(built):
    L = built
    assert L.lib().yolo_conv_splitk_slices(_desc(L, 384, 32, 1, 1, 5)) == 1
    assert L.lib().yolo_conv_splitk_slices(_desc(L, 24, 96, 1, 1, 13)) == 1          # KT = 3 < 4 steps
    assert L.lib().yolo_conv_splitk_slices(_desc(L, 64, 512, 3, 1, 13)) > 16          # K = 4,608 on 3 tiles: many slices


def test_unsupported_shapes_report_zero(built):
    """A 16-bit dtype, cin of 3 or 4 (the stem), cin that is no multiple of 32."""
    L = built
    lib = L.lib()
    for d in (_desc(L, 64, 32, 1, 1, dtype=L.BF16), _desc(L, 64, 32, 3, 1, dtype=L.F16), _desc(L, 32, 3, 3, 1), _desc(L, 32, 4, 3, 1),
              _desc(L, 64, 48, 1, 1)):
        assert lib.yolo_conv_splitk_supported(d) == 0
        assert lib.yolo_conv_splitk_eligible(d) == 0
        assert lib.yolo_conv_splitk_slices(d) == 0
        d.flags = L.FLAG_SPLIT_K
        assert lib.yolo_conv_workspace_bytes(d) == 0


@pytest.mark.parametrize("cout,cin,k,s,h,w", SHAPES)
def test_workspace_bytes_is_the_documented_formula(built, cout, cin, k, s, h, w):
    """S * n * Ho * Wo * cout_pad4 * 4 with the flag; without it what the descriptor asked for before the flag existed."""
    L = built
    lib = L.lib()
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    for n in (1, 3):
        d = _desc(L, cout, cin, k, s, h, w, n=n)
        before = lib.yolo_conv_workspace_bytes(d)
        d.flags = L.FLAG_SPLIT_K | L.FLAG_NANCHECK
        assert lib.yolo_conv_workspace_bytes(d) == lib.yolo_conv_splitk_slices(d) * n * ho * wo * ((cout + 3) // 4 * 4) * 4
        d.flags = L.FLAG_NANCHECK
        assert lib.yolo_conv_workspace_bytes(d) == before


def test_workspace_bytes_is_a_64_bit_value(built):
    """n = 64 at 608 x 608 (the 19 x 19, 38 x 38 and 76 x 76 maps), and a batch at which the product passes 2^32."""
    L = built
    lib = L.lib()
    for cout, cin, hw in ((1024, 512, 19), (256, 128, 76), (512, 256, 38)):
        d = _desc(L, cout, cin, 3, 1, hw, n=64, flags=L.FLAG_SPLIT_K)
        want = lib.yolo_conv_splitk_slices(d) * 64 * hw * hw * cout * 4
        assert lib.yolo_conv_workspace_bytes(d) == want
    d = _desc(L, 256, 128, 3, 1, 76, n=1024, flags=L.FLAG_SPLIT_K)
    assert lib.yolo_conv_workspace_bytes(d) == lib.yolo_conv_splitk_slices(d) * 1024 * 76 * 76 * 256 * 4 > 2 ** 32


def test_without_the_flag_the_workspace_is_what_it_was(built):
    """The Winograd layers keep their request, the direct ones theirs (none)."""
    L = built
    lib = L.lib()
    assert lib.yolo_conv_workspace_bytes(_desc(L, 256, 128, 3, 1, 52)) > 0
    assert lib.yolo_conv_workspace_bytes(_desc(L, 256, 512, 1, 1, 26)) == 0
    assert lib.yolo_conv_workspace_bytes(_desc(L, 512, 256, 3, 2, 52)) == 0


def _calls(L, d, ws, ws_bytes):
    """Return codes of the three entry points on descriptor d (fake pointers: they must come back before any launch)."""
    lib = L.lib()
    op = (L.ConvOp * 1)()
    C.memmove(C.byref(op[0].d), C.byref(d), C.sizeof(L.ConvDesc))
    op[0].x = op[0].w_packed = op[0].scale = op[0].shift = op[0].y = FAKE
    op[0].workspace, op[0].workspace_bytes = ws, ws_bytes
    return (lib.yolo_conv_fwd(d, FAKE, FAKE, FAKE, FAKE, None, FAKE, None, None),
            lib.yolo_conv_fwd_ws(d, FAKE, FAKE, FAKE, FAKE, None, FAKE, ws or None, ws_bytes, None, None),
            lib.yolo_conv_fwd_batch(op, 1, None, None))


def test_return_codes_without_a_launch(built):
    L = built
    lib = L.lib()
    d = _desc(L, 64, 512, 3, 1, 13, flags=L.FLAG_SPLIT_K)
    need = lib.yolo_conv_workspace_bytes(d)
    assert need > 0
    # no workspace: all three; yolo_conv_fwd has none whatever the caller owns
    assert _calls(L, d, 0, 0) == (ERR_WORKSPACE, ERR_WORKSPACE, ERR_WORKSPACE)
    assert b"SPLIT_K" in lib.yolo_last_error()
    # one byte too small
    assert _calls(L, d, FAKE, need - 1) == (ERR_WORKSPACE, ERR_WORKSPACE, ERR_WORKSPACE)
    # a size without a pointer
    assert _calls(L, d, 0, need)[1:] == (ERR_WORKSPACE, ERR_WORKSPACE)
    # together with each of the other three kernel flags: refused, with or without the workspace
    for other in (L.FLAG_SPLIT_BF16, L.FLAG_SPLIT_WEIGHTS_READY, L.FLAG_FILTERS_READY, L.FLAG_SPLIT_BF16 | L.FLAG_SPLIT_WEIGHTS_READY):
        e = _desc(L, 64, 512, 3, 1, 13, flags=L.FLAG_SPLIT_K | other)
        assert _calls(L, e, FAKE, need) == (ERR_UNSUPPORTED,) * 3, other
        assert _calls(L, e, 0, 0) == (ERR_UNSUPPORTED,) * 3, other
    # a forced tile, a 16-bit dtype, the stem's channels
    for e in (_desc(L, 64, 512, 3, 1, 13, flags=L.FLAG_SPLIT_K, tile=4), _desc(L, 64, 512, 3, 1, 13, flags=L.FLAG_SPLIT_K, tile=15),
              _desc(L, 64, 512, 1, 1, 13, flags=L.FLAG_SPLIT_K, dtype=L.BF16), _desc(L, 32, 3, 3, 1, 16, flags=L.FLAG_SPLIT_K),
              _desc(L, 32, 4, 3, 1, 16, flags=L.FLAG_SPLIT_K)):
        assert _calls(L, e, FAKE, 1 << 30) == (ERR_UNSUPPORTED,) * 3
    assert C.sizeof(L.ConvDesc) == 18 * 4 and L.FLAG_SPLIT_K == 32


def test_workspace_bytes_is_zero_where_the_launch_refuses_the_flag(built):
    """The flag next to another kernel flag, or with a forced tile: the launch returns YOLO_ERR_UNSUPPORTED, so no size is reported."""
    L = built
    lib = L.lib()
    assert lib.yolo_conv_workspace_bytes(_desc(L, 64, 512, 3, 1, 13, flags=L.FLAG_SPLIT_K)) > 0
    for other in (L.FLAG_SPLIT_BF16, L.FLAG_SPLIT_WEIGHTS_READY, L.FLAG_FILTERS_READY):
        assert lib.yolo_conv_workspace_bytes(_desc(L, 64, 512, 3, 1, 13, flags=L.FLAG_SPLIT_K | other)) == 0
    for tile in (4, 7, 15):
        assert lib.yolo_conv_workspace_bytes(_desc(L, 64, 512, 3, 1, 13, flags=L.FLAG_SPLIT_K, tile=tile)) == 0


def test_model_state_carries_latency(built):
    from yolo_for_turbines_amd import engine
    st = engine.ModelState()
    assert st.latency is False
    assert pickle.loads(pickle.dumps(st)).latency is False and copy.deepcopy(st).latency is False
    for mode in (True, "all"):
        st.latency = mode
        assert pickle.loads(pickle.dumps(st)).latency == mode
        assert copy.deepcopy(st).latency == mode
    st.__setstate__({"nan_check": False})                 # a state pickled before the attribute existed
    assert st.latency is False and st.nan_check is False and st.split3 is True
    assert set(engine.ModelState().__getstate__()) == {"nan_check", "autocast_heads", "split3", "latency"}


def test_plan_flags_follow_latency(built):
    """Plans built on the CPU device (no launch), 416 x 416, batch 1: "all" flags every launch behind the stem that the library
    supports, True those it lists as eligible; a flagged op carries none of the other kernel flags and its workspace covers its
    request; off, forced-tile, 16-bit and train plans carry no such flag."""
    import torch
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import engine, train_engine
    L = built
    lib = L.lib()
    m = yt.YOLOv3(num_classes=80).eval()
    dev = torch.device("cpu")
    prog = engine.build_network_program(m, 1, 416)
    others = L.FLAG_FILTERS_READY | L.FLAG_SPLIT_BF16 | L.FLAG_SPLIT_WEIGHTS_READY
    for mode, accepts in ((True, lib.yolo_conv_splitk_eligible), ("all", lib.yolo_conv_splitk_supported)):
        st = engine.ModelState()
        st.latency = mode
        plan = engine.Plan(prog, st, dev)
        flagged = [i for i in range(len(plan.table)) if plan.table[i].d.flags & L.FLAG_SPLIT_K]
        assert flagged == [i for i in range(plan.first, len(plan.table)) if accepts(C.byref(plan.table[i].d))]
        for i in flagged:
            e = plan.table[i]
            assert not e.d.flags & others
            assert e.workspace and e.workspace_bytes >= lib.yolo_conv_workspace_bytes(C.byref(e.d)) > 0
    assert len(flagged) == len(plan.table) - plan.first       # "all": every launch behind the stem has cin % 32 == 0
    assert all(plan.table[i].d.flags & L.FLAG_SPLIT_K for i in range(plan.first, len(plan.table))
               if plan.table[i].d.ksize == 3 and plan.table[i].d.stride == 1)
    off = engine.ModelState()
    for p in (engine.Plan(prog, off, dev), engine.Plan(prog, st, dev, tile_override=4),
              engine.Plan(engine.build_network_program(m, 1, 416, ch_align=8), st, dev, dtype="bf16")):
        assert not any(p.table[i].d.flags & L.FLAG_SPLIT_K for i in range(len(p.table)))
    tprog = engine.build_network_program(m, 2, 96)
    train_engine.TrainPlan(tprog, dev, "fp32")
    assert not any(op["flags"] & L.FLAG_SPLIT_K for op in tprog.ops)
