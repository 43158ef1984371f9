"""The layout of the package after utils.py was split by stage (nothing is launched): utils.py re-exports every public name of
before the split, each name is the very object of the module that defines it, every stage module imports on its own, the deferred NaN
guard of ModelState keeps its contract, and the one scale-list validator raises each caller's messages at each caller's bound."""
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = ("boxes", "tiles", "fuse", "metrics", "data", "model")
HOME = {                                                   # the 39 public functions and classes of utils.py -> the module that defines them
    "boxes": ("iou_aligned", "calc_iou", "scaled_anchors", "decode_boxes", "cells_to_boxes", "nms_indices", "non_max_suppression", "detect",
              "detect_images", "AnchorResult", "AnchorFitness", "anchor_draws", "anchors_layout", "kmeans_anchors", "anchor_fitness"),
    "tiles": ("tile_grid", "tile_pyramid", "detect_tiled"),
    "fuse": ("fuse_boxes", "tta_views", "tta_boxes", "detect_tta"),
    "metrics": ("calc_mAP", "EvalResult", "EvalMatches", "evaluate_detections", "evaluate_model", "accuracy_counts", "check_model_accuracy",
                "eval_boxes", "get_eval_boxes"),
    "data": ("build_targets", "letterbox", "unletterbox_boxes", "augment_params", "augment_batch", "train_batch"),
    "model": ("save_checkpoint", "load_checkpoint"),
}
CONSTANTS = {"STRIDES": "boxes", "EVAL_MAX_THRESHOLDS": "metrics", "AUG_NPARAM": "data"}
UTILS_ALL = {"iou_aligned", "calc_iou", "cells_to_boxes", "non_max_suppression", "decode_boxes", "nms_indices", "detect", "detect_tiled",
             "fuse_boxes", "tta_views", "tta_boxes", "detect_tta", "tile_grid", "tile_pyramid", "build_targets", "calc_mAP",
             "evaluate_detections", "evaluate_model", "accuracy_counts", "check_model_accuracy", "eval_boxes", "get_eval_boxes", "letterbox",
             "unletterbox_boxes", "augment_params", "augment_batch", "train_batch", "save_checkpoint", "load_checkpoint", "scaled_anchors",
             "anchor_draws", "kmeans_anchors", "anchor_fitness", "anchors_layout"}
PACKAGE_ALL = ["YOLOLoss", "FusedYOLOLoss", "GraphedTrainStep", "SGD", "Adam", "AdamW", "clip_grad_norm_", "GradScaler", "ModelEMA", "CNNBlock",
               "ResidualBlock", "ScalePredictionBlock", "YOLOv3", "layer_config", "calc_iou", "cells_to_boxes", "decode_boxes", "detect",
               "detect_images", "detect_tiled", "fuse_boxes", "tta_views", "tta_boxes", "detect_tta", "tile_grid", "tile_pyramid", "iou_aligned",
               "nms_indices", "non_max_suppression", "build_targets", "calc_mAP", "evaluate_detections", "evaluate_model", "accuracy_counts",
               "check_model_accuracy", "eval_boxes", "get_eval_boxes", "letterbox", "unletterbox_boxes", "augment_params", "augment_batch",
               "train_batch", "scaled_anchors", "anchor_draws", "kmeans_anchors", "anchor_fitness", "anchors_layout", "Tracker", "TrackResult",
               "track_images"]


def _module(name):
    import importlib
    return importlib.import_module("yolo_for_turbines_amd." + name)


def test_utils_resolves_every_public_name_of_before_the_split():
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import utils
    names = [n for group in HOME.values() for n in group]
    assert len(names) == len(set(names)) == 39 and len(CONSTANTS) == 3 and len(UTILS_ALL) == 34
    for n in names + list(CONSTANTS):
        assert hasattr(utils, n), n
    assert set(utils.__all__) == UTILS_ALL and len(utils.__all__) == 34
    assert yt.__all__ == PACKAGE_ALL
    assert all(getattr(yt, n) is getattr(utils, n) for n in PACKAGE_ALL if n in names)
    assert (utils.STRIDES, utils.EVAL_MAX_THRESHOLDS, utils.AUG_NPARAM) == ((32, 16, 8), 16, 29)
    assert utils.__doc__.startswith("Drop-in mirror of the reference's post-processing functions")


def test_every_name_is_the_object_of_its_stage_module():
    from yolo_for_turbines_amd import utils
    for mod, names in HOME.items():
        m = _module(mod)
        for n in names:
            assert getattr(utils, n) is getattr(m, n), n                               # no wrapper, no second copy
            assert getattr(utils, n).__module__ == "yolo_for_turbines_amd." + mod, n
    for n, mod in CONSTANTS.items():
        assert getattr(utils, n) is getattr(_module(mod), n), n
    # private names are not re-exported: no attribute with a leading underscore (dunders apart) comes from another module
    assert [n for n in vars(utils) if n.startswith("_") and not n.startswith("__")] == []
    # utils.py holds nothing of its own: every attribute that is not a dunder comes from a stage module
    own = [n for n, v in vars(utils).items() if not n.startswith("__") and getattr(v, "__module__", None) == utils.__name__]
    assert own == []


def test_every_stage_module_imports_alone_and_not_through_utils():
    """One fresh interpreter per module (started together): an import cycle cannot hide behind the order the package imports in."""
    code = ("import sys, yolo_for_turbines_amd.{0} as m; "
            "src = open(m.__file__).read(); "
            "sys.exit(1 if 'import utils' in src or 'from .utils' in src or 'from . import utils' in src else 0)")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONDONTWRITEBYTECODE="1")
    procs = {name: subprocess.Popen([sys.executable, "-c", code.format(name)], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                    stderr=subprocess.STDOUT) for name in MODULES}
    for name, p in procs.items():
        out, _ = p.communicate()
        assert p.returncode == 0, (name, out.decode(errors="replace")[-2000:])


def test_deferred_nan_guard_contract():
    from yolo_for_turbines_amd.engine import ModelState
    eng = ModelState()                                                                 # touches no device
    assert eng._defer_nan is False and eng._pending_flag is None
    sentinel = object()
    eng._pending_flag = sentinel                                                       # a stale flag does not survive the entry
    with eng.deferred_nan():
        assert eng._defer_nan is True and eng._pending_flag is None
        assert eng.take_pending_flag() is None                                         # nothing pending: nan_check off, or no forward yet
        eng._pending_flag = sentinel                                                   # what forward() leaves
        assert eng.take_pending_flag() is sentinel and eng._pending_flag is None       # taken and cleared
        assert eng.take_pending_flag() is None
        eng._pending_flag = sentinel                                                   # left untaken: the exit clears it
    assert eng._defer_nan is False and eng._pending_flag is None
    with pytest.raises(KeyError, match="inside"):
        with eng.deferred_nan():
            eng._pending_flag = sentinel
            raise KeyError("inside")
    assert eng._defer_nan is False and eng._pending_flag is None
    with eng.deferred_nan():                                                           # usable again after the raise
        assert eng._defer_nan is True
    assert eng._defer_nan is False and eng._pending_flag is None
    # the host side of the slots: bit 0 is the input guard, bit 1 the layer guard, as one forward's flag
    eng.raise_on_flags([])
    eng.raise_on_flags([0, 0, 0])
    with pytest.raises(AssertionError, match="NaN in the input tensor"):
        eng.raise_on_flags([0, 1, 0])
    with pytest.raises(AssertionError, match="NaN in the input tensor"):
        eng.raise_on_flags([2, 1])                                                     # the input guard comes first, as in a forward
    with pytest.raises(ValueError, match="Nan in layer"):
        eng.raise_on_flags([0, 0, 2])


NUMBERS = "scales must be a non-empty sequence of numbers, got {!r}"
RANGE = "scales must be a non-empty sequence of finite numbers in (0, {}], got {!r}"
REPEAT = "scales must not repeat a level, got {!r}"


def _rejected(fn, message):
    with pytest.raises(ValueError) as e:
        fn()
    assert str(e.value) == message


@pytest.mark.parametrize("top", [8, 4])
def test_scales_validator_at_both_bounds(top):
    from yolo_for_turbines_amd.tiles import _scales
    assert _scales((float(top), 0.5), top) == [float(top), 0.5] and _scales([1], top) == [1.0]
    assert _scales((math.nextafter(0.0, 1.0),), top) == [5e-324]
    for bad in ((top + 0.0001,), (0,), (0.0,), (-1.0,), (math.nan,), (math.inf,), (), [1.0, float(top) * 2]):
        _rejected(lambda: _scales(bad, top), RANGE.format(top, bad))
    for bad in ((True,), (1.0, False), ("1.0",), "1.0", b"1", (b"1",), 1.0, None, (None,), ([1.0],)):
        _rejected(lambda: _scales(bad, top), NUMBERS.format(bad))
    _rejected(lambda: _scales((1.0, 0.5, 1), top), REPEAT.format((1.0, 0.5, 1)))
    assert _scales((1.0, 0.5, 1), top, distinct=False) == [1.0, 0.5, 1.0]


def test_scales_messages_of_the_two_callers():
    """tile_pyramid / detect_tiled validate in (0, 8] and refuse a repeated level; tta_views validates the LIST it made of its argument in
    (0, 4], and a repeated scale is a repeated view there: the texts of the two validators of before the split."""
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd.tiles import _scales
    assert _scales((8.0,)) == [8.0] and yt.tta_views(32, 32, ("none",), (4.0,)) == [(128, 128, 0, 0)]
    _rejected(lambda: _scales((8.0001,)), RANGE.format(8, (8.0001,)))
    _rejected(lambda: _scales((1.0, 1.0)), REPEAT.format((1.0, 1.0)))
    _rejected(lambda: yt.tta_views(32, 32, ("none",), (4.0001,)), RANGE.format(4, [4.0001]))
    _rejected(lambda: yt.tta_views(32, 32, ("none",), (0,)), RANGE.format(4, [0]))
    _rejected(lambda: yt.tta_views(32, 32, ("none",), (math.nan,)), RANGE.format(4, [math.nan]))
    _rejected(lambda: yt.tta_views(32, 32, ("none",), ()), RANGE.format(4, []))
    _rejected(lambda: yt.tta_views(32, 32, ("none",), (True,)), NUMBERS.format([True]))
    _rejected(lambda: yt.tta_views(32, 32, ("none",), ("1.0",)), NUMBERS.format(["1.0"]))
    _rejected(lambda: yt.tta_views(32, 32, ("none",), "1.0"), "flips and scales must be sequences")
    _rejected(lambda: yt.tta_views(32, 32, ("none",), (1.0, 1.0)), "view (32, 32, 0, 0) (scale 1.0, flip 'none') repeats an earlier view")
