"""The ring of conv_wino4s_f32 (six slots, five stages ahead, carried across the six passes) through the C-ABI, on filter planes made
once: at the shapes where the ring can go wrong (tests/gen_golden_wino4s_ring.py: CASES) the kernel gives the bits that the
four-slot ring gave (tests/golden/wino4s_ring.json), the same bits on every launch, and fp32 accuracy against an fp64 convolution."""
import ctypes as C
import json

import pytest
import torch

from tests import gen_golden_wino4s_ring as G


@pytest.fixture(scope="module")
def L():
    from yolo_for_turbines_amd import _lib
    _lib.lib()                       # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


@pytest.fixture(scope="module")
def golden():
    with open(G.OUT) as f:
        return json.load(f)


def _cut(L, d):
    whole, half = C.c_int(-1), C.c_int(-1)
    L.check(L.lib().yolo_conv_wino4_blocks(d, C.byref(whole), C.byref(half)), "yolo_conv_wino4_blocks")
    return whole.value, half.value


def test_the_golden_file_names_the_cases():
    with open(G.OUT) as f:
        assert sorted(json.load(f)) == sorted(G.case_id(c) for c in G.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_ring_bits_race_and_accuracy(L, golden, case, capsys):
    """Five launches into fresh outputs: byte-equal to each other and to the recorded digest, NaN flag 0 (the inputs are randn: a
    stage read from the wrong slot, or before it landed, gives other bits). Then the first 16 images against an fp64 convolution
    with the bound of test_gpu_wino4_planes.py::test_half_workgroups_against_fp64: max|err| / max|y| at most 1e-5 and at most
    twice the f32 GEMMs' on the same operands."""
    import torch.nn.functional as F
    B, H, W, cin, cout, residual = case
    cs = G.Case(L, case)
    whole, half = _cut(L, cs.planes_desc())
    tiles = B * ((H + 3) // 4) * ((W + 3) // 4)
    assert whole + half == (tiles + 63) // 64
    if B > 2000:
        assert half == 0, "the last case is meant to run as whole workgroups"
    runs = [cs.run() for _ in range(5)]
    y32, flag32 = cs.run(cs.desc(L.FLAG_FILTERS_READY))
    torch.cuda.synchronize()
    assert all(int(f.item()) == 0 for _, f in runs) and int(flag32.item()) == 0
    ys = [y.view(torch.int32) for y, _ in runs]
    assert all(torch.equal(ys[0], y) for y in ys[1:])
    assert G.digest(runs[0][0]) == golden[G.case_id(case)]

    n = min(B, 16)
    ref = F.conv2d(cs.x[:n].double().permute(0, 3, 1, 2), cs.w.double(), padding=1) * cs.scale.double().view(1, -1, 1, 1) \
        + cs.shift.double().view(1, -1, 1, 1)
    ref = F.leaky_relu(ref, 0.1).permute(0, 2, 3, 1)
    if residual:
        ref = ref + cs.r[:n].double()
    err = float((runs[0][0][:n].cpu().double() - ref).abs().max() / ref.abs().max())
    err32 = float((y32[:n].cpu().double() - ref).abs().max() / ref.abs().max())
    with capsys.disabled():
        print(f"\nwino4 ring {G.case_id(case)} (whole {whole}, halves {half}): split {err:.3e}  f32 {err32:.3e}  ratio {err / err32:.2f}")
    assert err <= 1e-5, err
    assert err <= 2 * err32, (err, err32)
