"""Anchor clustering on the device (yolo_anchor_kmeans / yolo_anchor_fitness, kmeans_anchors / anchor_fitness) against the numpy
restatement of the header's contract (tests/anchors_ref.py). Floats are compared as bits. The contract leaves the association of
the fp64 sums open, so before anything is compared the restatement itself must (a) have kept every seeding draw at least 1e-9 T
away from the nearest running-sum boundary and (b) reach the same bits with two summation orders: equality is only claimed
where the specification is unambiguous."""
import functools

import numpy as np
import pytest
import torch

from tests import anchors_ref as ar

pytestmark = pytest.mark.gpu
SPARE = 4096
MARGIN = 1e-9

# (n, k, restarts) -> (seed of the boxes, seed of the draws)
CASES = {
    (1, 1, 1): (1, 1000),               # smallest input
    (9, 9, 2): (101, 1100),             # n = k
    (257, 9, 3): (201, 1200),           # one box past a 256-lane block
    (5000, 9, 4): (301, 1300),          # typical size
    (5000, 6, 2): (401, 1400),          # k = 6
    (70001, 9, 2): (502, 1501),         # many blocks and a ragged last one
}


@pytest.fixture(scope="module")
def L():
    import yolo_for_turbines_amd  # noqa: F401
    from yolo_for_turbines_amd import _lib
    _lib.lib()                       # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


def _draws(restarts, k, seed):
    import yolo_for_turbines_amd as yt
    return yt.anchor_draws(restarts, k, torch.Generator().manual_seed(seed))


def _checked_reference(wh, draws, max_iter=300):
    """The restatement's result, after its two preconditions have been asserted on it."""
    a = ar.kmeans(wh, draws, max_iter, "pairwise")
    b = ar.kmeans(wh, draws, max_iter, "fsum")
    assert a["margin"] >= MARGIN, f"a seeding draw lies {a['margin']:.1e} T from a running-sum boundary: choose other seeds"
    for key in ("picks", "iterations", "converged"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["centroids"].view(np.uint32), b["centroids"].view(np.uint32)), "the summation orders disagree: choose other seeds"
    assert a["best"] == b["best"]
    return a


@functools.lru_cache(maxsize=None)
def _case(n, k, restarts, max_iter=300):
    bseed, dseed = CASES[(n, k, restarts)]
    wh = ar.make_boxes(n, bseed)
    draws = _draws(restarts, k, dseed)
    return wh, draws, _checked_reference(wh, draws.numpy(), max_iter)


def _bits(t):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32).view(np.uint32)


def _assert_equals_reference(res, ref):
    assert np.array_equal(res.picks.numpy(), ref["picks"])
    assert np.array_equal(res.iterations.numpy(), ref["iterations"])
    assert np.array_equal(res.converged.numpy(), ref["converged"])
    assert np.array_equal(_bits(res.centroids), _bits(ref["centroids"]))
    assert res.best == ref["best"]
    assert tuple(res.anchors.shape) == ref["anchors"].shape and np.array_equal(_bits(res.anchors), _bits(ref["anchors"]))
    got, want = res.fitness.numpy(), ref["fitness"]
    assert got.dtype == np.float64
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (got, want)


@pytest.mark.parametrize("n,k,restarts", list(CASES))
def test_kmeans_equals_the_restatement(L, n, k, restarts):
    import yolo_for_turbines_amd as yt
    wh, draws, ref = _case(n, k, restarts)
    res = yt.kmeans_anchors(wh, k=k, restarts=restarts, draws=draws)
    print(f"n {n} k {k} R {restarts}: iterations {res.iterations.tolist()} fitness {res.fitness.tolist()} best {res.best} "
          f"margin {ref['margin']:.1e}")
    _assert_equals_reference(res, ref)
    assert res.centroids.dtype == torch.float32 and res.picks.dtype == torch.int32 and res.iterations.dtype == torch.int32
    assert tuple(res.anchors.shape) == ((3, k // 3, 2) if k % 3 == 0 else (k, 2))
    if n > k:
        assert int(ref["iterations"].max()) > 1 and int(ref["converged"].min()) == 1        # the case does iterate, and ends by itself


def test_generator_draws_are_the_table(L):
    """``generator`` without ``draws`` draws the table of anchor_draws."""
    import yolo_for_turbines_amd as yt
    wh, draws, ref = _case(257, 9, 3)
    res = yt.kmeans_anchors(wh, k=9, restarts=3, generator=torch.Generator().manual_seed(CASES[(257, 9, 3)][1]))
    _assert_equals_reference(res, ref)


def test_identical_boxes(L):
    """64 copies of one box, k = 3: T == 0 takes the fallback pick min(int(u n), n - 1); clusters 1 and 2 win no box (ties go to the
    lowest index) and keep their seed; step 1 changes nothing."""
    import yolo_for_turbines_amd as yt
    box = np.array([0.3125, 0.171875], dtype=np.float32)
    wh = np.tile(box, (64, 1))
    draws = _draws(2, 3, 77)
    res = yt.kmeans_anchors(wh, k=3, restarts=2, draws=draws)
    want = np.minimum((draws.numpy() * 64).astype(np.int64), 63)
    assert len(set(want.reshape(-1).tolist())) > 1                         # the fallback is not one constant
    assert np.array_equal(res.picks.numpy(), want)
    assert res.iterations.tolist() == [1, 1] and res.converged.tolist() == [1, 1]
    assert np.array_equal(_bits(res.centroids), _bits(np.broadcast_to(box, (2, 3, 2))))
    assert np.array_equal(_bits(res.anchors), _bits(np.broadcast_to(box, (3, 1, 2))))
    assert res.fitness.tolist() == [1.0, 1.0] and res.best == 0
    fit = yt.anchor_fitness(wh, res.centroids[0])
    assert fit.counts.tolist() == [64, 0, 0] and fit.labels.tolist() == [0] * 64 and fit.mean_iou == 1.0 and fit.recall == 1.0
    _assert_equals_reference(res, _checked_reference(wh, draws.numpy()))


def test_two_distinct_boxes(L):
    """Two boxes, 40 copies each, k = 3: the third seed falls back (T == 0 once both boxes are seeds) or doubles a seed."""
    import yolo_for_turbines_amd as yt
    wh = np.concatenate([np.tile(np.array([0.25, 0.5], np.float32), (40, 1)), np.tile(np.array([0.6, 0.2], np.float32), (40, 1))])
    wh = wh[np.random.default_rng(3).permutation(80)]
    draws = _draws(4, 3, 78)
    ref = _checked_reference(wh, draws.numpy())
    res = yt.kmeans_anchors(wh, k=3, restarts=4, draws=draws)
    _assert_equals_reference(res, ref)
    assert res.fitness.tolist() == [1.0] * 4


def test_iteration_cap(L):
    import yolo_for_turbines_amd as yt
    wh, draws, full = _case(5000, 9, 4)
    assert int(full["iterations"].min()) > 2
    ref = _checked_reference(wh, draws.numpy(), max_iter=2)
    res = yt.kmeans_anchors(wh, k=9, restarts=4, max_iter=2, draws=draws)
    assert res.converged.tolist() == [0] * 4 and res.iterations.tolist() == [2] * 4
    _assert_equals_reference(res, ref)
    assert not np.array_equal(_bits(res.centroids), _bits(full["centroids"]))


def test_more_than_256_blocks(L):
    """n = 530,001 is 259 blocks of 2,048 boxes, so every loop over blocks takes a second round: the seeding pick scans the block sums 256
    at a time (the second draw is chosen to land in the last three blocks), the update stages 256 rows of k = 2 per round, and
    anchor_fitness with 16 anchors 85 rows per round. Four Lloyd steps keep the restatement quick."""
    import yolo_for_turbines_amd as yt
    wh = ar.make_boxes(530001, 601)
    draws = torch.tensor([[0.25, 0.9951]], dtype=torch.float64)
    ref = _checked_reference(wh, draws.numpy(), max_iter=4)
    assert int(ref["picks"][0, 1]) >= 256 * 2048
    res = yt.kmeans_anchors(wh, k=2, restarts=1, max_iter=4, draws=draws)
    _assert_equals_reference(res, ref)
    assert res.converged.tolist() == [0] and res.iterations.tolist() == [4]
    anchors = np.random.default_rng(1).uniform(0.02, 0.9, (16, 2)).astype(np.float32)
    _assert_fitness_equals(yt.anchor_fitness(wh, anchors), ar.anchor_fitness(wh, anchors))


def test_largest_k_and_restarts(L):
    """k = 16 and 64 restarts, the limits of the header, on 300 boxes."""
    import yolo_for_turbines_amd as yt
    wh = ar.make_boxes(300, 611)
    draws = _draws(64, 16, 1610)
    ref = _checked_reference(wh, draws.numpy())
    res = yt.kmeans_anchors(wh, k=16, restarts=64, draws=draws)
    _assert_equals_reference(res, ref)
    assert tuple(res.anchors.shape) == (16, 2) and len(set(res.iterations.tolist())) > 1


def _launch(L, wh, draws, k, restarts, max_iter, fill):
    """One yolo_anchor_kmeans with the workspace the library asks for, pre-filled with byte `fill`, and SPARE bytes of 0x5a behind it and
    behind every output: (outputs on the host, the spare bytes after the launch, the input after the launch)."""
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    n = wh.shape[0]
    whd, dd = torch.from_numpy(wh).to(dev), draws.to(dev)
    need = lib.yolo_anchor_kmeans_workspace_bytes(n, k, restarts)
    ws = torch.full((need + SPARE,), fill, dtype=torch.uint8, device=dev)
    ws[need:] = 0x5a
    sizes = dict(centroids=restarts * k * 8, fitness=restarts * 8, iterations=restarts * 4, converged=restarts * 4, picks=restarts * k * 4)
    outs = {name: torch.full((nb + SPARE,), 0x5a, dtype=torch.uint8, device=dev) for name, nb in sizes.items()}
    rc = lib.yolo_anchor_kmeans(whd.data_ptr(), n, k, restarts, dd.data_ptr(), max_iter, outs["centroids"].data_ptr(), outs["fitness"].data_ptr(),
                                outs["iterations"].data_ptr(), outs["converged"].data_ptr(), outs["picks"].data_ptr(), ws.data_ptr(), need, st)
    torch.cuda.synchronize()
    assert rc == 0, lib.yolo_last_error()
    spare = torch.cat([ws[need:].cpu()] + [outs[name][nb:].cpu() for name, nb in sizes.items()])
    return {name: outs[name][:nb].cpu() for name, nb in sizes.items()}, spare, whd.cpu(), dd.cpu()


def test_determinism_and_untouched_memory(L):
    """Two launches are bit-equal, whatever garbage the workspace held (every byte that is read was written by the launch); the
    bytes behind the workspace and behind every output, the boxes and the draws stay as they were."""
    wh, draws, ref = _case(5000, 9, 4)
    clean = torch.full((6 * SPARE,), 0x5a, dtype=torch.uint8)
    runs = []
    for fill in (0xff, 0x00, 0xff):
        out, spare, wh_after, draws_after = _launch(L, wh, draws, 9, 4, 300, fill)
        assert torch.equal(spare, clean)
        assert np.array_equal(wh_after.numpy().view(np.uint32), wh.view(np.uint32)) and torch.equal(draws_after, draws)
        runs.append(out)
    for other in runs[1:]:
        for name in runs[0]:
            assert torch.equal(runs[0][name], other[name]), name
    assert np.array_equal(runs[0]["centroids"].view(torch.float32).numpy().view(np.uint32).reshape(4, 9, 2), _bits(ref["centroids"]))
    assert np.array_equal(runs[0]["picks"].view(torch.int32).numpy().reshape(4, 9), ref["picks"])


def test_picks_may_be_null(L):
    lib, dev = L.lib(), torch.device("cuda:0")
    wh, draws, ref = _case(257, 9, 3)
    whd, dd = torch.from_numpy(wh).to(dev), draws.to(dev)
    cen = torch.empty((3, 9, 2), dtype=torch.float32, device=dev)
    fit = torch.empty(3, dtype=torch.float64, device=dev)
    ic = torch.empty((2, 3), dtype=torch.int32, device=dev)
    ws = torch.empty(lib.yolo_anchor_kmeans_workspace_bytes(257, 9, 3), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_anchor_kmeans(whd.data_ptr(), 257, 9, 3, dd.data_ptr(), 300, cen.data_ptr(), fit.data_ptr(), ic[0].data_ptr(),
                                   ic[1].data_ptr(), None, ws.data_ptr(), ws.numel(), L.current_stream()), "yolo_anchor_kmeans")
    assert np.array_equal(_bits(cen.cpu()), _bits(ref["centroids"])) and np.array_equal(ic[0].cpu().numpy(), ref["iterations"])


# nine arbitrary anchors (made up), scale-major like config.ANCHORS
ARBITRARY = [[(0.31, 0.27), (0.44, 0.62), (0.85, 0.8)], [(0.09, 0.13), (0.17, 0.1), (0.12, 0.33)], [(0.015, 0.02), (0.035, 0.06), (0.07, 0.05)]]


def _assert_fitness_equals(got, want):
    assert np.array_equal(got.counts.numpy(), want["counts"]) and got.counts.dtype == torch.int32
    assert np.array_equal(got.labels.numpy(), want["labels"]) and got.labels.dtype == torch.int32
    assert abs(got.mean_iou - want["mean_iou"]) <= 1e-12 * abs(want["mean_iou"]), (got.mean_iou, want["mean_iou"])
    assert abs(got.recall - want["recall"]) <= 1e-12 * abs(want["recall"]), (got.recall, want["recall"])


@pytest.mark.parametrize("n,k,restarts", [(5000, 9, 4), (70001, 9, 2), (257, 9, 3)])
def test_anchor_fitness_equals_the_restatement(L, n, k, restarts):
    import yolo_for_turbines_amd as yt
    wh, draws, ref = _case(n, k, restarts)
    clustered = ref["centroids"][ref["best"]]
    for anchors, thr in ((clustered, 0.5), (np.array(ARBITRARY, dtype=np.float32), 0.5), (np.array(ARBITRARY, dtype=np.float32), 0.3),
                         (clustered[:4], 0.6)):
        got = yt.anchor_fitness(wh, anchors, iou_threshold=thr)
        want = ar.anchor_fitness(wh, anchors, thr)
        _assert_fitness_equals(got, want)
        assert int(got.counts.sum()) == n and 0.0 < got.recall <= 1.0
    # the clustered anchors' mean_iou is their restart's fitness
    got = yt.anchor_fitness(wh, clustered)
    assert abs(got.mean_iou - ref["fitness"][ref["best"]]) <= 1e-12 * got.mean_iou


def test_clustering_does_not_lower_the_fitness(L):
    """Every restart's final centroids score at least the mean_iou of its own seeds, and the best restart beats the arbitrary anchors."""
    import yolo_for_turbines_amd as yt
    wh, draws, ref = _case(5000, 9, 4)
    res = yt.kmeans_anchors(wh, k=9, restarts=4, draws=draws)
    for r in range(4):
        seeds = wh[res.picks[r].numpy()]
        assert np.array_equal(_bits(seeds), _bits(ref["seeds"][r]))
        before, after = yt.anchor_fitness(wh, seeds).mean_iou, yt.anchor_fitness(wh, res.centroids[r]).mean_iou
        print(f"restart {r}: seeds {before:.4f} -> clustered {after:.4f}")
        assert after >= before
    assert float(res.fitness[res.best]) > yt.anchor_fitness(wh, ARBITRARY).mean_iou


def test_rectangular_canvas(L):
    """image_size=(352, 608) clusters the sizes multiplied in fp32 by (1.0, 352 / 608), the factors build_targets computes; the
    anchors feed scaled_anchors and build_targets on that canvas."""
    import yolo_for_turbines_amd as yt
    wh, draws, _ = _case(5000, 9, 4)
    H, W = 352, 608
    rows = np.concatenate([np.full((len(wh), 2), 0.5, np.float32), wh, np.zeros((len(wh), 1), np.float32)], axis=1)   # [x, y, w, h, class]
    res = yt.kmeans_anchors(rows, k=9, restarts=4, draws=draws, image_size=(H, W))
    rw, rh = np.float32(float(W) / max(H, W)), np.float32(float(H) / max(H, W))
    assert rw == np.float32(1.0)
    pre = wh * np.array([rw, rh], dtype=np.float32)
    want = yt.kmeans_anchors(pre, k=9, restarts=4, draws=draws)
    for name in ("anchors", "centroids"):
        assert np.array_equal(_bits(getattr(res, name)), _bits(getattr(want, name))), name
    assert torch.equal(res.fitness, want.fitness) and torch.equal(res.picks, want.picks) and torch.equal(res.iterations, want.iterations)
    _assert_equals_reference(res, _checked_reference(pre, draws.numpy()))
    fit = yt.anchor_fitness(rows, res.anchors, image_size=(H, W))
    assert abs(fit.mean_iou - float(res.fitness[res.best])) <= 1e-12
    # downstream: grid-cell anchors and targets on the same canvas
    sa = yt.scaled_anchors(res.anchors, H, W)
    assert tuple(sa.shape) == (3, 3, 2) and torch.equal(sa[0], res.anchors[0] * (W // 32))
    per_image = [[[0.5, 0.5, float(w), float(h), 0.0] for w, h in wh[i * 5:i * 5 + 5]] for i in range(4)]
    targets = yt.build_targets(per_image, res.anchors, (H, W))
    assert [tuple(t.shape) for t in targets] == [(4, 3, H // s, W // s, 6) for s in (32, 16, 8)]
    assert all(int((t[..., 4] == 1).sum()) > 0 for t in targets)
    # the per-image list is the same set of boxes
    again = yt.kmeans_anchors([rows[:100].tolist(), None, [], rows[100:].tolist()], k=9, restarts=4, draws=draws, image_size=(H, W))
    assert np.array_equal(_bits(again.centroids), _bits(res.centroids))
