"""Host side of YOLO_FLAG_WINO_SPLIT_BF16 (Winograd F(4x4) with its GEMMs on bf16 planes): where the library honours the flag, what it
refuses, the workspace it asks for, and which launches of the eval plan carry it (plans built on the CPU device: no launch)."""
import copy
import ctypes as C
import pickle

import pytest
import torch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def _desc(L, n, hw, cin, cout, flags=0, tile=0, ksize=3, stride=1, dtype=None):
    return L.ConvDesc(n=n, h=hw, w=hw, cin=cin, cout=cout, ksize=ksize, stride=stride, x_ld=cin, y_ld=cout, act=L.ACT_LEAKY,
                      out_mode=L.OUT_NHWC, dtype=L.F32 if dtype is None else dtype, flags=flags, tile=tile)


def test_refusals(built):
    """The flag is refused with YOLO_ERR_UNSUPPORTED (-2) before anything is launched (the pointers are never dereferenced) wherever
    it is not honoured; where it is, the launch gets as far as its workspace check (-4 on 16 bytes). Every call brings a 16-byte
    workspace, so none can reach a kernel; the forced tile 15 takes the route without one."""
    L = built
    lib = L.lib()
    S, R, A = L.FLAG_WINO_SPLIT_BF16, L.FLAG_FILTERS_READY, L.FLAG_FILTERS_APPENDED
    assert S == 128

    def launch(d, ws_bytes=16):
        return lib.yolo_conv_fwd_ws(d, 16, 16, 16, 16, 0, 16, 16, ws_bytes, 0, 0)

    for filt in (R, A):                                               # honoured: with either filter flag
        assert launch(_desc(L, 2, 52, 128, 256, flags=S | filt, tile=15)) == -4
        assert b"bf16 planes" in lib.yolo_last_error()
    refused = [
        _desc(L, 2, 52, 128, 256, flags=S, tile=15),                                  # no filter flag
        _desc(L, 2, 52, 128, 256, flags=S | R | L.FLAG_SPLIT_BF16, tile=15),
        _desc(L, 2, 52, 128, 256, flags=S | R | L.FLAG_SPLIT_WEIGHTS_READY, tile=15),
        _desc(L, 2, 52, 68, 84, flags=S | R, tile=15),                                # cin % 32 != 0 (tile 15 itself takes it)
        _desc(L, 2, 52, 128, 256, flags=S, tile=13),                                  # F(2x2)
        _desc(L, 2, 52, 128, 256, flags=S, tile=5),                                   # a direct tile
        _desc(L, 2, 52, 128, 256, flags=S),                                           # tile 0 without the workspace: a direct kernel
        _desc(L, 2, 52, 256, 128, flags=S, ksize=1),
        _desc(L, 2, 52, 128, 256, flags=S, stride=2),
        _desc(L, 2, 52, 128, 256, flags=S | L.FLAG_SPLIT_BF16, stride=2),
        _desc(L, 2, 52, 128, 256, flags=S, dtype=L.BF16),
    ]
    for d in refused:
        assert launch(d) == -2, (d.flags, d.tile, d.ksize, d.stride, d.dtype, lib.yolo_last_error())
        assert b"YOLO_FLAG_" in lib.yolo_last_error()
    # split-K checks its workspace first (an existing refusal: -4 on 16 bytes); with room for its partial sums the new flag is refused
    assert launch(_desc(L, 2, 52, 128, 256, flags=S | L.FLAG_SPLIT_K)) == -4
    assert launch(_desc(L, 2, 52, 128, 256, flags=S | L.FLAG_SPLIT_K), ws_bytes=1 << 40) == -2 and b"WINO_SPLIT_BF16" in lib.yolo_last_error()
    # the refusals that stood before come first: YOLO_FLAG_FILTERS_READY where nothing runs as tile 15 is still the argument error
    assert launch(_desc(L, 2, 52, 256, 128, flags=S | R, ksize=1)) == -1
    assert launch(_desc(L, 2, 52, 128, 256, flags=S | A | R, tile=15)) == -2 and b"FILTERS_APPENDED goes" in lib.yolo_last_error()


def test_workspace_and_queries(built):
    """With the flag yolo_conv_workspace_bytes reports the planes of V4 and U4, 6 bytes per value; without it, and where the flag is
    not honoured, the fp32 workspace as before. The two queries look at the shape only."""
    L = built
    lib = L.lib()
    S, R = L.FLAG_WINO_SPLIT_BF16, L.FLAG_FILTERS_READY
    for n, hw, cin, cout in ((32, 52, 128, 256), (1, 52, 128, 256), (32, 104, 64, 128), (2, 26, 256, 512), (3, 13, 96, 80)):
        tiles = n * ((hw + 3) // 4) ** 2
        rows = (tiles + 63) // 64 * 64 + (cout + 63) // 64 * 64
        assert lib.yolo_conv_workspace_bytes(_desc(L, n, hw, cin, cout, flags=R, tile=15)) == 36 * cin * rows * 4
        assert lib.yolo_conv_workspace_bytes(_desc(L, n, hw, cin, cout, flags=R | S, tile=15)) == 36 * cin * rows * 6
    assert lib.yolo_conv_workspace_bytes(_desc(L, 2, 52, 68, 84, flags=R | S, tile=15)) == 36 * 18 * (384 + 128) * 16       # not honoured
    for n in (1, 32):
        assert lib.yolo_conv_wino4_split_supported(_desc(L, n, 52, 128, 256)) == 1
        assert lib.yolo_conv_wino4_split_supported(_desc(L, n, 13, 512, 1024)) == 1          # (tile 15 once the filters are appended)
        assert lib.yolo_conv_wino4_split_supported(_desc(L, n, 13, 256, 512)) == 0           # F(2x2)
        assert lib.yolo_conv_wino4_split_supported(_desc(L, n, 52, 256, 128, ksize=1)) == 0
        assert lib.yolo_conv_wino4_split_supported(_desc(L, n, 52, 128, 256, stride=2)) == 0
        assert lib.yolo_conv_wino4_split_supported(_desc(L, n, 52, 128, 256, dtype=L.BF16)) == 0
        for d in (_desc(L, n, 52, 128, 256), _desc(L, n, 104, 64, 128), _desc(L, n, 26, 256, 512), _desc(L, n, 13, 512, 1024)):
            assert lib.yolo_conv_wino4_split_eligible(d) in (0, 1)
            assert lib.yolo_conv_wino4_split_eligible(d) == lib.yolo_conv_wino4_split_eligible(_desc(L, 7, d.h, d.cin, d.cout, flags=R | S, tile=15))
        assert lib.yolo_conv_wino4_split_eligible(_desc(L, n, 52, 256, 128, ksize=1)) == 0


def _flagged(L, plan):
    return [i for i in range(len(plan.table)) if plan.table[i].d.flags & L.FLAG_WINO_SPLIT_BF16]


def test_eval_plan_carries_the_flag_where_the_library_names_the_shape(built):
    """At batch 32, 416 x 416, 80 classes: exactly the Winograd F(4x4) launches on finished filters whose shape wino4_split_eligible
    names carry the flag, next to their filter flag, with a workspace that covers the planes; "all" flags every such launch the
    library honours it on (the 24 + 7 of the plan); False, latency mode, a forced tile, a bf16 plan and the train path: none."""
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import engine, train_engine
    L = built
    lib = L.lib()
    S, filt = L.FLAG_WINO_SPLIT_BF16, L.FLAG_FILTERS_READY | L.FLAG_FILTERS_APPENDED
    m = yt.YOLOv3(num_classes=80).eval()
    dev = torch.device("cpu")
    prog = engine.build_network_program(m, 32, 416)
    st = engine.ModelState()
    assert st.wino4_split is True
    plan = engine.Plan(prog, st, dev)
    wino = [i for i in range(len(plan.table)) if plan.table[i].d.flags & filt]
    assert len(wino) == 31
    want = [i for i in wino if lib.yolo_conv_wino4_split_eligible(C.byref(plan.table[i].d))]
    assert _flagged(L, plan) == want
    for i in want:
        e = plan.table[i]
        assert not e.d.flags & (L.FLAG_SPLIT_BF16 | L.FLAG_SPLIT_WEIGHTS_READY | L.FLAG_SPLIT_K)
        assert lib.yolo_conv_pick_tile(C.byref(e.d)) == 15
        tiles = e.d.n * ((e.d.h + 3) // 4) * ((e.d.w + 3) // 4)
        assert e.workspace and e.workspace_bytes >= lib.yolo_conv_workspace_bytes(C.byref(e.d)) == 36 * e.d.cin * ((tiles + 63) // 64 * 64 + (e.d.cout + 63) // 64 * 64) * 6
    st_all = engine.ModelState()
    st_all.wino4_split = "all"
    plan_all = engine.Plan(prog, st_all, dev)
    assert _flagged(L, plan_all) == wino
    assert all(lib.yolo_conv_wino4_split_supported(C.byref(plan_all.table[i].d)) for i in wino)
    st_off = engine.ModelState()
    st_off.wino4_split = False
    st_lat = engine.ModelState()
    st_lat.latency = True
    st_lat.wino4_split = "all"
    plans = [engine.Plan(prog, st_off, dev), engine.Plan(engine.build_network_program(m, 1, 416), st_lat, dev),
             engine.Plan(prog, st_all, dev, tile_override=15), engine.Plan(prog, st_all, dev, tile_override=13),
             engine.Plan(engine.build_network_program(m, 32, 416, ch_align=8), st_all, dev, dtype="bf16")]
    for p in plans:
        assert _flagged(L, p) == []
    # without the flag the plan is today's: the same flags on every launch
    assert [plans[0].table[i].d.flags for i in range(len(plan.table))] == [plan.table[i].d.flags & ~S for i in range(len(plan.table))]
    # the train path builds its descriptors from the program's flags alone (train_engine._desc): the program carries no such flag
    assert not any(op["flags"] & S for op in prog.ops)
    assert "WINO_SPLIT" not in open(train_engine.__file__).read()


def test_model_state_carries_wino4_split(built):
    from yolo_for_turbines_amd import engine
    st = engine.ModelState()
    assert pickle.loads(pickle.dumps(st)).wino4_split is True and copy.deepcopy(st).wino4_split is True
    for v in (False, "all"):
        st.wino4_split = v
        assert pickle.loads(pickle.dumps(st)).wino4_split == v and copy.deepcopy(st).wino4_split == v
    st.__setstate__({"nan_check": False})                 # a state pickled before the attribute existed
    assert st.wino4_split is True
