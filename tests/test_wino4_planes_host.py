"""Host side of YOLO_FLAG_FILTER_PLANES (the bf16 planes of the Winograd F(4x4) filters made once, directly behind their U4): the size
query, what the library refuses, which launches of the eval plan carry the flag, and where the engine keeps the planes (plans and
blocks built on the CPU device: no launch)."""
import ctypes as C

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


def test_filter_plane_bytes(built):
    """36 * cin * cout_pad64 * 6 for the shapes of test_wino4_split_host.py::test_workspace_and_queries (cin and cout only: 1.5 x the
    fp32 U4), and 0 where tile 15 does not honour the split."""
    L = built
    lib = L.lib()
    for n, hw, cin, cout in ((32, 52, 128, 256), (1, 52, 128, 256), (32, 104, 64, 128), (2, 26, 256, 512), (3, 13, 96, 80)):
        d = _desc(L, n, hw, cin, cout)
        assert lib.yolo_wino4_filter_plane_bytes(d) == 36 * cin * ((cout + 63) // 64 * 64) * 6
        assert 2 * lib.yolo_wino4_filter_plane_bytes(d) == 3 * lib.yolo_wino4_filter_bytes(d)
        # the U rows of the workspace formula are these bytes
        tiles = n * ((hw + 3) // 4) ** 2
        ws = lib.yolo_conv_workspace_bytes(_desc(L, n, hw, cin, cout, flags=L.FLAG_FILTERS_READY | L.FLAG_WINO_SPLIT_BF16, tile=15))
        assert ws == 36 * cin * ((tiles + 63) // 64 * 64) * 6 + lib.yolo_wino4_filter_plane_bytes(d)
    assert lib.yolo_wino4_filter_plane_bytes(_desc(L, 32, 13, 512, 1024)) == 113_246_208
    for d in (_desc(L, 2, 52, 68, 84, tile=15), _desc(L, 2, 52, 256, 128, ksize=1), _desc(L, 2, 52, 128, 256, stride=2),
              _desc(L, 2, 52, 128, 256, dtype=L.BF16)):
        assert lib.yolo_wino4_filter_plane_bytes(d) == 0
    assert lib.yolo_wino4_filter_plane_bytes(None) == 0
    assert lib.yolo_wino4_filter_planes(_desc(L, 2, 52, 68, 84, tile=15), 16, 1 << 20, 0) == -2           # refused before any launch
    assert lib.yolo_wino4_filter_planes(_desc(L, 2, 52, 128, 256), 16, 0, 0) == -1
    assert lib.yolo_wino4_filter_planes(_desc(L, 2, 52, 128, 256), 1 << 30, (1 << 30) + 16, 0) == -1      # planes inside their U4


def test_refusals(built):
    """Every call brings a 16-byte workspace, so none can reach a kernel (the pointers are never dereferenced)."""
    L = built
    lib = L.lib()
    P, S, R, A = L.FLAG_FILTER_PLANES, L.FLAG_WINO_SPLIT_BF16, L.FLAG_FILTERS_READY, L.FLAG_FILTERS_APPENDED
    assert P == 256

    def launch(d, ws_bytes=16):
        return lib.yolo_conv_fwd_ws(d, 16, 16, 16, 16, 0, 16, 16, ws_bytes, 0, 0)

    # alone (no filter flag): an argument error, as YOLO_FLAG_FILTERS_READY is where it does not belong
    assert launch(_desc(L, 2, 52, 128, 256, flags=P, tile=15)) == -1 and b"FILTER_PLANES" in lib.yolo_last_error()
    assert launch(_desc(L, 2, 52, 128, 256, flags=P)) == -1
    for d in (_desc(L, 2, 52, 256, 128, flags=P | R, ksize=1), _desc(L, 2, 52, 128, 256, flags=P | R, stride=2),
              _desc(L, 2, 52, 128, 256, flags=P | R, tile=5), _desc(L, 2, 52, 256, 128, flags=P, ksize=1),
              _desc(L, 2, 52, 128, 256, flags=P, stride=2), _desc(L, 2, 52, 128, 256, flags=P, tile=5),
              _desc(L, 2, 52, 68, 84, flags=P | R, tile=15)):                                      # tile 15, but no split: cin % 32
        assert launch(d) == -1, (d.flags, d.tile, d.ksize, d.stride, lib.yolo_last_error())
    for filt in (R, A):
        assert launch(_desc(L, 2, 52, 128, 256, flags=filt | S | P, tile=15)) == -4 and b"bf16 planes" in lib.yolo_last_error()
        # accepted and ignored on the f32 GEMMs: as far as their workspace check
        assert launch(_desc(L, 2, 52, 128, 256, flags=filt | P, tile=15)) == -4 and b"bf16 planes" not in lib.yolo_last_error()
        for f in (filt, filt | S):
            assert (lib.yolo_conv_workspace_bytes(_desc(L, 2, 52, 128, 256, flags=f | P, tile=15))
                    == lib.yolo_conv_workspace_bytes(_desc(L, 2, 52, 128, 256, flags=f, tile=15)) > 0)
    # (the eval plan's route to the small maps: tile 0 with the appended filters)
    assert lib.yolo_conv_workspace_bytes(_desc(L, 32, 13, 512, 1024, flags=A | S | P)) == lib.yolo_conv_workspace_bytes(_desc(L, 32, 13, 512, 1024, flags=A | S))


def _flags(plan):
    return [plan.table[i].d.flags for i in range(len(plan.table))]


def test_eval_plan_carries_the_flag_on_every_launch_with_a_filter_flag(built):
    """At batch 32, 416 x 416, 80 classes: all 31 launches on finished filters carry 256, whatever ``wino4_split`` says, so that the
    plan with ``wino4_split = False`` is the default one with bit 128 cleared; "perlaunch" carries 128 without 256; latency mode, a
    forced tile, a bf16 plan and the train path carry none."""
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import engine, train_engine
    L = built
    lib = L.lib()
    P, S, filt = L.FLAG_FILTER_PLANES, L.FLAG_WINO_SPLIT_BF16, L.FLAG_FILTERS_READY | L.FLAG_FILTERS_APPENDED
    m = yt.YOLOv3(num_classes=80).eval()
    dev = torch.device("cpu")
    prog = engine.build_network_program(m, 32, 416)

    def state(**kw):
        st = engine.ModelState()
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    plan = engine.Plan(prog, state(), dev)
    off = engine.Plan(prog, state(wino4_split=False), dev)
    for p in (plan, off, engine.Plan(prog, state(wino4_split="all"), dev)):
        f = _flags(p)
        assert sum(bool(x & P) for x in f) == 31
        assert [bool(x & P) for x in f] == [bool(x & filt) for x in f]
        assert all(lib.yolo_conv_wino4_split_supported(C.byref(p.table[i].d)) for i, x in enumerate(f) if x & P)
    assert _flags(off) == [x & ~S for x in _flags(plan)]
    per = _flags(engine.Plan(prog, state(wino4_split="perlaunch"), dev))
    assert sum(bool(x & S) for x in per) == 31 and not any(x & P for x in per)
    assert [x & ~P for x in _flags(engine.Plan(prog, state(wino4_split="all"), dev))] == per
    none = [engine.Plan(engine.build_network_program(m, 1, 416), state(latency=True, wino4_split="all"), dev),
            engine.Plan(prog, state(wino4_split="all"), dev, tile_override=15), engine.Plan(prog, state(), dev, tile_override=13),
            engine.Plan(engine.build_network_program(m, 32, 416, ch_align=8), state(wino4_split="all"), dev, dtype="bf16")]
    for p in none:
        assert not any(x & P for x in _flags(p))
    assert not any(op["flags"] & P for op in prog.ops)
    assert "FILTER_PLANES" not in open(train_engine.__file__).read()


def test_planes_live_behind_their_filters_in_one_allocation(built):
    """``prepared["u4"].buf`` and ``PackedBlock.w`` keep their sizes and become the front of a larger allocation: the planes start at
    U4 + yolo_wino4_filter_bytes."""
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import engine
    L = built
    lib = L.lib()
    dev = torch.device("cpu")
    # a 128 -> 256 block at 52 x 52 (U4 in a buffer of its own) and a 512 -> 1024 block at 13 x 13 (U4 behind the packed weights)
    for cin, cout, hw, kind in ((128, 256, 52, "u4"), (512, 1024, 13, "u4a")):
        blk = yt.model.CNNBlock(cin, cout, kernel_size=3, padding=1)
        pk = engine.PackedBlock(blk, dev)
        d = _desc(L, 32, hw, cin, cout)
        nu, npl = lib.yolo_wino4_filter_bytes(d), lib.yolo_wino4_filter_plane_bytes(d)
        assert npl == 36 * cin * cout * 6
        buf = pk.want(kind, d)
        p = pk.prepared[kind]
        assert pk.has_planes(kind) and p.planes.numel() == npl
        assert buf.numel() == nu and p.planes.data_ptr() == buf.data_ptr() + nu
        st = buf.untyped_storage()
        assert p.planes.untyped_storage().data_ptr() == st.data_ptr()
        assert st.nbytes() - (buf.data_ptr() - st.data_ptr()) >= nu + npl
        if kind == "u4a":
            na = lib.yolo_wino4_appended_bytes(d)
            assert pk.w.numel() == na and buf.data_ptr() == pk.w.data_ptr() + na - nu
            assert pk.w.untyped_storage().nbytes() >= na + npl
        else:
            assert pk.w.numel() == lib.yolo_packed_weight_bytes(cout, cin, 3, L.F32) == pk.w.untyped_storage().nbytes()
    # a block the split cannot run (cin % 32) keeps a U4 without planes, and its launches go without the flag
    blk = yt.model.CNNBlock(68, 84, kernel_size=3, padding=1)
    pk = engine.PackedBlock(blk, dev)
    pk.want("u4", _desc(L, 2, 52, 68, 84, tile=15))
    assert not pk.has_planes("u4")
