"""The fp64 restatement of tests/decode_ref.py against what the project already pins (CPU): the oracle's
``cells_to_boxes`` on the three DECODE_CASES, ``torch.argmax`` on every planted score pattern of
tests/test_gpu_decode_edges.py part b, and the fp32-vs-fp64 error that test's tolerance is four times of."""
import numpy as np
import pytest
import torch

from oracle import postprocess as opp
from tests import decode_ref as D
from tests import golden_inputs as gi

ATOL = 1e-7                                    # the suite's value for decode (tests/test_gpu_parity.py)


def decode_fp32_rel_error():
    """Measured once per run (cached): see tests/decode_ref.py."""
    return D.decode_fp32_rel_error()


@pytest.mark.parametrize("name", list(gi.DECODE_CASES))
def test_restatement_equals_the_oracle(name):
    """fp32 oracle within 4 x decode_fp32_rel_error() (+ 1e-7) of the restatement rounded to fp32, as the GPU test asks of
    the kernel; classes exact; and decode_fp32 is the oracle bit for bit on a square grid."""
    pred, anchors = gi.decode_input(name)
    g = gi.DECODE_CASES[name]["g"]
    p = torch.from_numpy(pred.copy())
    want = opp.cells_to_boxes(p, torch.from_numpy(anchors), g)            # mutates p
    b32, m32 = D.decode_fp32(torch.from_numpy(pred), anchors)
    assert torch.equal(b32, want) and torch.equal(m32, p)
    b64, m64, cls = D.decode_ref64(torch.from_numpy(pred), anchors)
    rtol = 4.0 * decode_fp32_rel_error()
    np.testing.assert_allclose(want[..., :5].numpy(), b64[..., :5].float().numpy(), rtol=rtol, atol=ATOL)
    np.testing.assert_allclose(p[..., :4].numpy(), m64[..., :4].float().numpy(), rtol=rtol, atol=ATOL)
    assert torch.equal(m64[..., 4:], torch.from_numpy(pred).double()[..., 4:])
    assert torch.equal(b64[..., 5], want[..., 5].double()) and torch.equal(cls.reshape(want.shape[:2]), want[..., 5].long())
    print(f"{name}: oracle fp32 vs fp64 rel err {D.rel_error(want[..., :5], b64[..., :5]):.3e}")


@pytest.mark.parametrize("nc", D.PLANTED_NC)
def test_class_index_equals_torch_argmax_on_the_planted_scores(nc):
    pred, names = D.planted_scores(nc)
    s = torch.from_numpy(pred)[..., 5:].reshape(-1, nc)
    got = D.first_max(s)
    assert torch.equal(got, torch.argmax(s, dim=-1))
    assert got.tolist() == [D.first_max_loop(r) for r in s.tolist()]
    by = dict(zip(names, got.tolist()))
    # what the patterns are there to show
    assert all(by["max@%d" % k] == k and by["nan@%d" % k] == k for k in range(nc))
    assert all(by["tie@%d|%d" % ab] == ab[0] for ab in D.quarter_bounds(nc))
    assert len(D.quarter_bounds(nc)) == {3: 2, 5: 2, 37: 3, 80: 3}[nc]             # nc = 3 and 5 leave the last quarter empty
    assert by["all-equal"] == 0 and by["all-neg-inf"] == 0 and by["one-finite"] == nc // 2 and by["inf-twice"] == nc // 3
    assert by["two-nans"] == nc // 2 and by["inf-then-nan"] == nc - 1 and by["nan-then-inf"] == 0


def test_torch_argmax_is_the_sequential_first_maximum():
    """first NaN, first of equal maxima, 0 for all -inf"""
    nan, inf = D.NAN, D.INF
    rows = [[1.0, nan, 5.0, nan], [2.0, 7.0, 7.0, 1.0], [-inf] * 4, [inf, 1.0, inf, nan], [nan, inf, 0.0, 0.0]]
    assert torch.argmax(torch.tensor(rows), dim=-1).tolist() == [1, 1, 0, 3, 0] == [D.first_max_loop(r) for r in rows]


def test_planted_boxes_overflow_and_underflow_alike_in_fp32_and_fp64():
    """+-89, +-20, 0 and NaN in x, y, w, h and objectness: the restatement rounded to fp32 has its infinities and NaNs where
    the fp32 evaluation has them; e^-89 is subnormal there and 0 here, which the absolute tolerance is for."""
    pred, anchors = D.planted_boxes(), D.anchors_of("planted-boxes")
    b32, m32 = D.decode_fp32(torch.from_numpy(pred), anchors)
    b64, m64, _ = D.decode_ref64(torch.from_numpy(pred), anchors)
    for got, want in ((b32[..., :5], b64[..., :5].float()), (m32[..., :4], m64[..., :4].float())):
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
        assert int(torch.isnan(got).sum()) >= 5 - (got.shape[-1] == 4)
    assert int(torch.isinf(b32).sum()) == 2 and int(torch.isinf(m32).sum()) == 2          # w and h at +89
    np.testing.assert_allclose(b32[..., :5].numpy(), b64[..., :5].float().numpy(), rtol=4.0 * decode_fp32_rel_error(), atol=ATOL, equal_nan=True)


def test_targets_path_is_the_oracle():
    t = torch.from_numpy(D.gaussian_pred(2, 4, 4, 1, "targets"))
    want = opp.cells_to_boxes(t.clone(), torch.zeros(3, 2), 4, is_pred=False)
    assert np.array_equal(D.targets_fp32(t.numpy()), want.numpy())


def test_fp32_decode_error_is_what_the_gpu_tolerance_assumes():
    """tests/test_gpu_decode_edges.py allows 4x this figure: a few fp32 roundings (exp, 1 + e, the reciprocal, the anchor
    product, the grid scale), so between one and ten units of 2^-24."""
    e = decode_fp32_rel_error()
    print(f"oracle fp32 decode against the fp64 restatement over the inputs of the GPU test: max rel err {e:.3e}")
    assert 2.0 ** -24 < e < 10 * 2.0 ** -24
