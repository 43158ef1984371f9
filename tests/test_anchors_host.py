"""Anchor clustering on the host (nothing is launched): the return codes of yolo_anchor_kmeans / yolo_anchor_fitness for arguments
that are refused before any launch, the workspace queries, anchors_layout, anchor_draws and the wrapper's row filter."""
import math

import pytest
import torch

OK, ERR_ARG, ERR_UNSUPPORTED, ERR_LAUNCH, ERR_WORKSPACE = 0, -1, -2, -3, -4
FAKE = 1 << 20          # a non-null, aligned "device pointer" for calls that must return before they launch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def _kmeans(L, n=100, k=9, restarts=4, max_iter=10, wh=FAKE, draws=FAKE, cen=FAKE, fit=FAKE, it=FAKE, conv=FAKE, picks=FAKE, ws=FAKE,
            ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = lib.yolo_anchor_kmeans_workspace_bytes(n, k, restarts)
    return lib.yolo_anchor_kmeans(wh or None, n, k, restarts, draws or None, max_iter, cen or None, fit or None, it or None, conv or None,
                                  picks or None, ws or None, ws_bytes, None)


def _fitness(L, n=100, k=9, thr=0.5, wh=FAKE, anc=FAKE, out=FAKE, counts=FAKE, labels=FAKE, ws=FAKE, ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = lib.yolo_anchor_fitness_workspace_bytes(n, k)
    return lib.yolo_anchor_fitness(wh or None, n, anc or None, k, thr, out or None, counts or None, labels or None, ws or None, ws_bytes, None)


def test_kmeans_argument_errors(built):
    L = built
    for kw in (dict(k=0), dict(k=17), dict(k=-3), dict(n=8, k=9), dict(n=0, k=1), dict(restarts=0), dict(restarts=65), dict(restarts=-1),
               dict(max_iter=0), dict(max_iter=-5), dict(wh=0), dict(draws=0), dict(cen=0), dict(fit=0), dict(it=0), dict(conv=0)):
        assert _kmeans(L, ws_bytes=1 << 30, **kw) == ERR_ARG, kw
        assert L.lib().yolo_last_error().startswith(b"anchor_kmeans")
    # an argument error comes before the workspace is looked at
    assert _kmeans(L, k=17, ws=0, ws_bytes=0) == ERR_ARG
    assert _kmeans(L, wh=0, ws=0, ws_bytes=0) == ERR_ARG


def test_kmeans_workspace_errors(built):
    L = built
    need = L.lib().yolo_anchor_kmeans_workspace_bytes(100, 9, 4)
    assert need > 0
    assert _kmeans(L, ws=0, ws_bytes=0) == ERR_WORKSPACE
    assert _kmeans(L, ws=0, ws_bytes=need) == ERR_WORKSPACE
    assert _kmeans(L, ws_bytes=need - 1) == ERR_WORKSPACE
    assert b"workspace" in L.lib().yolo_last_error()
    for n, k, r in ((1, 1, 1), (9, 9, 2), (70001, 9, 2), (10 ** 6, 16, 64)):
        need = L.lib().yolo_anchor_kmeans_workspace_bytes(n, k, r)
        assert _kmeans(L, n=n, k=k, restarts=r, ws_bytes=need - 1) == ERR_WORKSPACE, (n, k, r)
        assert _kmeans(L, n=n, k=k, restarts=r, ws=0, ws_bytes=need) == ERR_WORKSPACE, (n, k, r)


def test_fitness_argument_and_workspace_errors(built):
    L = built
    for kw in (dict(k=0), dict(k=17), dict(n=0), dict(n=-1), dict(thr=math.nan), dict(wh=0), dict(anc=0), dict(out=0), dict(counts=0)):
        assert _fitness(L, ws_bytes=1 << 30, **kw) == ERR_ARG, kw
        assert L.lib().yolo_last_error().startswith(b"anchor_fitness")
    need = L.lib().yolo_anchor_fitness_workspace_bytes(100, 9)
    assert need > 0
    assert _fitness(L, ws=0, ws_bytes=0) == ERR_WORKSPACE
    assert _fitness(L, ws=0, ws_bytes=need) == ERR_WORKSPACE
    assert _fitness(L, ws_bytes=need - 1) == ERR_WORKSPACE
    assert _fitness(L, n=70001, ws_bytes=L.lib().yolo_anchor_fitness_workspace_bytes(70001, 9) - 1) == ERR_WORKSPACE


def test_workspace_queries(built):
    """Nonzero inside the limits, never smaller for a larger n, 64-bit, 0 outside the limits."""
    lib = built.lib()
    ns = (1, 2, 9, 256, 257, 2048, 2049, 5000, 70001, 10 ** 6, 2 ** 31 - 1)
    for k, r in ((1, 1), (9, 8), (16, 64)):
        sizes = [lib.yolo_anchor_kmeans_workspace_bytes(max(n, k), k, r) for n in ns]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (k, r, sizes)
        assert sizes[-1] > sizes[0]
        fs = [lib.yolo_anchor_fitness_workspace_bytes(n, k) for n in ns]
        assert all(s > 0 for s in fs) and fs == sorted(fs) and fs[-1] > fs[0]
    assert lib.yolo_anchor_kmeans_workspace_bytes(2 ** 31 - 1, 16, 64) > 2 ** 32
    for n, k, r in ((100, 0, 1), (100, 17, 1), (5, 9, 1), (100, 9, 0), (100, 9, 65)):
        assert lib.yolo_anchor_kmeans_workspace_bytes(n, k, r) == 0
    assert lib.yolo_anchor_fitness_workspace_bytes(0, 9) == 0 and lib.yolo_anchor_fitness_workspace_bytes(10, 17) == 0


# nine made-up pairs, areas 1 .. 9 (in units of 1e-2) when sorted
PAIRS = [(0.1, 0.1), (0.1, 0.2), (0.3, 0.1), (0.2, 0.2), (0.1, 0.5), (0.3, 0.2), (0.7, 0.1), (0.2, 0.4), (0.3, 0.3)]


def test_anchors_layout_nine(built):
    import yolo_for_turbines_amd as yt
    order = [4, 8, 0, 6, 2, 7, 1, 5, 3]
    got = yt.anchors_layout(torch.tensor([PAIRS[i] for i in order]))
    want = torch.tensor([PAIRS[6:9], PAIRS[3:6], PAIRS[0:3]])
    assert tuple(got.shape) == (3, 3, 2) and got.dtype == torch.float32 and torch.equal(got, want)
    area = got[..., 0] * got[..., 1]
    assert bool((area[:, 1:] > area[:, :-1]).all())               # ascending inside a group
    assert bool((area[:-1].min(1).values > area[1:].max(1).values).all())  # the largest group first
    # a plain list and a (3, 3, 2) input are taken as nine pairs
    assert torch.equal(yt.anchors_layout([PAIRS[i] for i in order]), want)
    assert torch.equal(yt.anchors_layout(torch.tensor([PAIRS[i] for i in order]).reshape(3, 3, 2)), want)


def test_anchors_layout_equal_areas_keep_input_order(built):
    import yolo_for_turbines_amd as yt
    # 0.5 x 0.25, 0.25 x 0.5 and 0.125 x 1.0 have the same fp32 area exactly (powers of two)
    pairs = [(0.5, 0.5), (0.5, 0.25), (0.25, 0.25), (0.25, 0.5), (1.0, 1.0), (0.125, 1.0)]
    got = yt.anchors_layout(torch.tensor(pairs))
    assert tuple(got.shape) == (3, 2, 2)
    want = torch.tensor([[(0.5, 0.5), (1.0, 1.0)], [(0.25, 0.5), (0.125, 1.0)], [(0.25, 0.25), (0.5, 0.25)]])
    assert torch.equal(got, want)


def test_anchors_layout_other_k(built):
    import yolo_for_turbines_amd as yt
    got = yt.anchors_layout(torch.tensor([(0.4, 0.4), (0.1, 0.1), (0.3, 0.3), (0.2, 0.2)]))
    assert tuple(got.shape) == (4, 2)
    assert torch.equal(got, torch.tensor([(0.1, 0.1), (0.2, 0.2), (0.3, 0.3), (0.4, 0.4)]))
    assert tuple(yt.anchors_layout(torch.tensor([(0.4, 0.4)])).shape) == (1, 2)
    six = yt.anchors_layout(torch.tensor([PAIRS[i] for i in (5, 0, 3, 1, 4, 2)]))
    assert tuple(six.shape) == (3, 2, 2) and torch.equal(six, torch.tensor([PAIRS[4:6], PAIRS[2:4], PAIRS[0:2]]))


def test_anchor_draws(built):
    import yolo_for_turbines_amd as yt
    a = yt.anchor_draws(8, 9, torch.Generator().manual_seed(5))
    b = yt.anchor_draws(8, 9, torch.Generator().manual_seed(5))
    c = yt.anchor_draws(8, 9, torch.Generator().manual_seed(6))
    assert a.dtype == torch.float64 and tuple(a.shape) == (8, 9)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert bool((a >= 0).all()) and bool((a < 1).all())
    g = torch.Generator().manual_seed(5)
    first, second = yt.anchor_draws(2, 3, g), yt.anchor_draws(2, 3, g)
    assert not torch.equal(first, second)                          # the generator moves on


def test_filter_drops_exactly_the_invalid_rows(built):
    from yolo_for_turbines_amd import boxes as utils
    nan = float("nan")
    rows = [[0.5, 0.5, 0.2, 0.3, 1], [0.5, 0.5, 0.0, 0.3, 0], [0.5, 0.5, 0.2, -0.1, 0], [0.5, 0.5, 1.0, 1.0, 2], [0.5, 0.5, 1.0000001, 0.5, 2],
            [0.5, 0.5, nan, 0.5, 0], [0.5, 0.5, 0.5, nan, 0], [0.1, 0.1, 1e-6, 0.999, 0], [9.0, -3.0, 0.4, 0.4, 0], [0.5, 0.5, 0.3, 1.5, 0]]
    keep = [0, 3, 7, 8]                                            # x, y and the class are not looked at
    want = torch.tensor([rows[i][2:4] for i in keep])
    assert torch.equal(utils._anchor_wh(torch.tensor(rows), None), want)
    assert torch.equal(utils._anchor_wh([r[2:4] for r in rows], None), want)                    # (N, 2) sizes
    assert torch.equal(utils._anchor_wh([rows[:4], None, [], rows[4:]], None), want)            # the per-image list of train_batch
    assert torch.equal(utils._anchor_wh([r[:4] for r in rows], None), want)                     # (N, 4)
    # image_size: the factors of build_targets, in fp32
    got = utils._anchor_wh(torch.tensor(rows), (352, 608))
    assert torch.equal(got, want * torch.tensor([1.0, 352 / 608], dtype=torch.float32))
    got = utils._anchor_wh(torch.tensor(rows), (608, 352))
    assert torch.equal(got, want * torch.tensor([352 / 608, 1.0], dtype=torch.float32))
    assert torch.equal(utils._anchor_wh(torch.tensor(rows), 416), want)
    with pytest.raises(ValueError):
        utils._anchor_wh(torch.zeros(4, 3), None)


def test_too_few_valid_rows_is_a_value_error(built):
    import yolo_for_turbines_amd as yt
    rows = [[0.2, 0.3]] * 8 + [[0.0, 0.3], [1.5, 0.2], [float("nan"), 0.1]]
    with pytest.raises(ValueError, match="fewer than k"):
        yt.kmeans_anchors(rows, k=9)
    with pytest.raises(ValueError, match="fewer than k"):
        yt.kmeans_anchors([], k=1)
    with pytest.raises(ValueError):
        yt.kmeans_anchors(rows, k=17)
    with pytest.raises(ValueError):
        yt.kmeans_anchors(rows, k=3, restarts=65)
    with pytest.raises(ValueError):
        yt.kmeans_anchors(rows, k=3, max_iter=0)
    with pytest.raises(ValueError, match="draws"):
        yt.kmeans_anchors(rows, k=3, restarts=2, draws=torch.ones(2, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="no valid box"):
        yt.anchor_fitness([[0.0, 0.3]], [[0.1, 0.1]])
