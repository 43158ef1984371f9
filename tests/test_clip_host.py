"""CPU-side checks of gradient clipping (`yolo_for_turbines_amd/optim.py`): the header and the ctypes binding agree on the new
entry points and on the state struct, the argument checks of ``SGD`` / ``clip_grad_norm_`` and of the C entry points, and the
coefficient of the reference the GPU tests compare against (`tests/clip_ref.py`) against PyTorch's own on the CPU. No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import clip_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("yolo_clip_norm_partials", "yolo_clip_finalize", "yolo_sgd_step", "yolo_clip_scale_grads")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "yolo_mi355x.h")).read()


def test_header_and_binding_agree_on_the_clip_entry_points(built):
    hdr = _header()
    lib = built.lib()
    for name in NEW:
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr)
        assert decl, f"{name} is not declared in the header"
        n_args = len(decl.group(1).split(","))
        res, args = built._SIGS[name]
        assert res is C.c_int and len(args) == n_args, name
        assert hasattr(lib, name)
    # the state struct: four 32-bit words in the header's order, 16 bytes
    st = re.search(r"typedef struct yolo_clip_state \{([^}]*)\}", hdr).group(1)
    fields = [f.split()[-1] for f in st.split(";") if f.strip()]
    assert fields == [n for n, _ in built.ClipState._fields_] == ["max_norm", "total_norm", "coef", "norm_type"]
    assert C.sizeof(built.ClipState) == 16
    kinds = dict(re.findall(r"(YOLO_NORM_[A-Z0-9]+) = (\d+)", hdr))
    assert built.NORM_KINDS == {2.0: int(kinds["YOLO_NORM_L2"]), math.inf: int(kinds["YOLO_NORM_INF"])}


def test_entry_points_refuse_bad_arguments_before_any_launch(built):
    lib = built.lib()
    ok = 1 << 20                                            # any non-NULL, 16-byte aligned address: nothing is launched
    assert lib.yolo_clip_finalize(0, 0, 0, 0, 0) < 0 and b"clip_finalize" in lib.yolo_last_error()      # NULL state
    assert lib.yolo_clip_finalize(0, 0, 0, ok + 4, 0) < 0                                                # misaligned state
    assert lib.yolo_clip_finalize(ok, -1, 0, ok, 0) < 0                                                  # negative count
    assert lib.yolo_clip_finalize(ok, 1, 3, ok, 0) < 0                                                   # unknown norm type
    assert lib.yolo_clip_norm_partials(ok, ok, -1, 0, 0, ok, 0, 0, 0) < 0
    assert lib.yolo_clip_norm_partials(ok, ok, 1, 0, 2, ok, 0, 0, 0) < 0
    assert lib.yolo_clip_norm_partials(0, ok, 1, 0, 0, ok, 0, 0, 0) < 0 and b"clip_norm_partials" in lib.yolo_last_error()
    # yolo_sgd_step(items, n_items, chunks, n_chunks, hyper4, clip state, grad_scale, found_inf, written, shadows, ema state, ...)
    assert lib.yolo_sgd_step(0, 1, 0, 1, ok, ok, 0, 0, 0, 0, 0, 0, 0, 0) < 0 and b"sgd_step" in lib.yolo_last_error()   # NULL tables
    assert lib.yolo_sgd_step(ok, 1, ok, 1, 0, ok, 0, 0, 0, 0, 0, 0, 0, 0) < 0                            # NULL hyper-parameters
    assert lib.yolo_sgd_step(ok, 1, ok, 1, ok + 4, ok, 0, 0, 0, 0, 0, 0, 0, 0) < 0                       # misaligned hyper-parameters
    assert lib.yolo_sgd_step(ok, 1, ok, 1, ok + 4, 0, 0, 0, 0, 0, 0, 0, 0, 0) < 0                        # the same without a clip state
    assert lib.yolo_sgd_step(ok, 1, ok, 1, ok, ok + 8, 0, 0, 0, 0, 0, 0, 0, 0) < 0                       # misaligned clip state
    assert lib.yolo_sgd_step(ok, -1, ok, 1, ok, ok, 0, 0, 0, 0, 0, 0, 0, 0) < 0                          # negative counts
    assert lib.yolo_sgd_step(ok, 1, ok, -1, ok, ok, 0, 0, 0, 0, 0, 0, 0, 0) < 0
    assert lib.yolo_sgd_step(ok, 1, ok, 1, ok, ok, 0, 0, ok, 0, 0, 0, 0, 0) < 0                          # written without found_inf
    assert lib.yolo_sgd_step(ok, 1, ok, 1, ok, 0, 0, 0, ok, 0, 0, 0, 0, 0) < 0
    assert lib.yolo_sgd_step(ok, 1, ok, 1, ok, ok, 0, 0, 0, ok, 0, 0, 0, 0) < 0                          # shadows without the EMA state
    assert lib.yolo_sgd_step(ok, 1, ok, 1, ok, 0, 0, 0, 0, 0, ok, 0, 0, 0) < 0                           # the EMA state without shadows
    assert lib.yolo_sgd_step(ok, 1, ok, 1, ok, 0, 0, 0, 0, ok, ok + 8, 0, 0, 0) < 0                      # misaligned EMA state
    assert lib.yolo_clip_scale_grads(ok, ok, 1, 0, 0) < 0 and b"clip_scale_grads" in lib.yolo_last_error()
    assert lib.yolo_clip_scale_grads(ok, ok, -1, ok, 0) < 0
    assert lib.yolo_clip_scale_grads(0, 0, 0, ok, 0) == 0 and lib.yolo_sgd_step(0, 0, 0, 0, 0, ok, 0, 0, 0, 0, 0, 0, 0, 0) == 0   # nothing to do
    # a NULL clip state is an option like the others, not an error (no chunks: the argument check is all that runs)
    assert lib.yolo_sgd_step(ok, 1, ok, 0, ok, 0, 0, 0, 0, 0, 0, 0, 0, 0) == 0
    assert lib.yolo_sgd_step(ok, 1, ok, 0, ok, ok + 8, 0, 0, 0, 0, 0, 0, 0, 0) < 0                       # but a misaligned one still is


def test_sgd_and_free_function_argument_checks():
    import yolo_for_turbines_amd as yt
    model = torch.nn.Linear(4, 3)
    for bad in (-1, -0.5, float("nan")):
        with pytest.raises(ValueError, match="norm"):
            yt.SGD(model.parameters(), lr=0.1, max_grad_norm=bad)
    with pytest.raises(ValueError, match="norm_type"):
        yt.SGD(model.parameters(), lr=0.1, max_grad_norm=1.0, grad_norm_type=3)
    opt = yt.SGD(model.parameters(), lr=0.1, max_grad_norm=math.inf, grad_norm_type=math.inf)
    assert opt.max_grad_norm == math.inf and opt.grad_norm_type == math.inf
    opt = yt.SGD(model.parameters(), lr=0.1)
    assert opt.max_grad_norm is None and opt.grad_norm_type == 2.0
    assert "max_grad_norm" not in opt.state_dict()["param_groups"][0]       # not part of the checkpoint
    opt.max_grad_norm = -3.0                                                # a plain attribute: looked at by the next step
    with pytest.raises(ValueError, match="norm"):
        opt.step()
    with pytest.raises(ValueError, match="norm_type"):
        yt.clip_grad_norm_(model.parameters(), 1.0, norm_type=3)
    with pytest.raises(ValueError, match="norm"):
        yt.clip_grad_norm_(model.parameters(), -1.0)
    assert float(yt.clip_grad_norm_(model.parameters(), 1.0)) == 0.0        # no gradients at all: PyTorch's answer
    model.weight.grad = torch.ones(3, 4)
    with pytest.raises(TypeError, match="fp32"):                            # no CPU path
        yt.clip_grad_norm_(model.parameters(), 1.0)
    assert yt.clip_grad_norm_ is yt.optim.clip_grad_norm_ and "clip_grad_norm_" in yt.__all__


def test_clip_ref_coefficient_is_torchs_on_the_cpu():
    """``clip_ref.coef`` against what `torch.nn.utils.clip_grads_with_norm_` multiplies a gradient of 1 by, bit for bit, and
    against the expression it evaluates; random norms over forty binades, the edges, and both sides of max_norm."""
    rng = np.random.default_rng(7)
    norms = np.exp2(rng.uniform(-20, 20, 400)).astype(np.float32) * rng.uniform(1, 2, 400).astype(np.float32)
    maxes = [1.0, 0.37, 1e4, 3.0]
    cases = [(t, m) for t in norms for m in maxes[:2]] + [(t, m) for t in norms[:50] for m in maxes[2:]]
    for m in (1.0, 0.37, 1e4):
        at = np.float32(m)
        cases += [(at, m), (np.nextafter(at, np.float32(0)), m), (np.nextafter(at, np.float32(np.inf)), m)]
    cases += [(np.float32(0), 1.0), (np.float32(np.inf), 1.0), (np.float32(np.nan), 1.0), (np.float32(2), math.inf), (np.float32(np.inf), math.inf)]
    differs_from_division = 0
    for t, m in cases:
        tt = torch.tensor(float(t), dtype=torch.float32)
        want = torch.clamp(m / (tt + 1e-6), max=1.0)
        got = clip_ref.coef(t, m)
        assert want.dtype == torch.float32
        assert np.array_equal(np.float32(want.item()).view(np.int32), got.view(np.int32)) or (math.isnan(want.item()) and np.isnan(got)), (t, m)
        p = torch.nn.Parameter(torch.zeros(1))
        p.grad = torch.ones(1)
        torch.nn.utils.clip_grads_with_norm_([p], m, tt)
        assert float(p.grad) == float(got) or (math.isnan(float(p.grad)) and np.isnan(got)), (t, m)
        with np.errstate(all="ignore"):
            true_div = np.float32(m) / (np.float32(t) + np.float32(1e-6))
        differs_from_division += int(np.isfinite(true_div) and true_div < 1 and true_div != got)
    assert differs_from_division > 0          # reciprocal-then-multiply is NOT a division: the kernel must not "simplify" it


def test_clip_ref_norm_handles_what_fp32_squares_cannot():
    big = np.zeros(10, np.float32)
    big[3] = 3e19
    with np.errstate(over="ignore"):
        assert clip_ref.total_norm([big]) == float(np.float32(3e19)) and np.isinf(np.float32(3e19) * np.float32(3e19))
    tiny = np.full(1000, 1e-30, np.float32)
    want = float(np.float32(1e-30)) * math.sqrt(1000)
    assert abs(clip_ref.total_norm([tiny]) - want) <= 1e-12 * want and np.float32(1e-30) * np.float32(1e-30) == 0
    g = np.array([1.0, -7.0, 3.0], np.float32)
    assert clip_ref.total_norm([g, g[:1]], norm_type=math.inf) == np.float32(7) and clip_ref.total_norm([g], scale=2.0, norm_type=math.inf) == np.float32(3.5)
    assert np.isnan(clip_ref.total_norm([np.array([1.0, np.nan], np.float32), g], norm_type=math.inf))
    assert clip_ref.total_norm([g], scale=3.0) == math.sqrt(sum(float(np.float32(v * clip_ref.inv_scale(3.0))) ** 2 for v in g))
