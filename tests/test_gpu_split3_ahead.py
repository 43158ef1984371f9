"""conv_split3_f32 after its K step was rewritten (every activation load unconditional, the zero select at the split, B requested
before A, barriers without the fence, the last step written out): at the K-step counts and staging edges where that, or more K
steps of activations in flight, can go wrong (tests/gen_golden_split3_ahead.py: CASES) every tile, on both weight routes, gives the
bits of the kernel before it (tests/golden/split3_ahead.json, written by the library of the commit before), the same bits on every
launch, the NaN flag of that commit, and leaves the output buffer outside the layer's view alone."""
import json

import pytest
import torch

from tests import gen_golden_split3_ahead as G
from tests import test_gpu_split3 as s3
from tests import test_gpu_split3_ready as s3r


@pytest.fixture(scope="module")
def L():
    import yolo_for_turbines_amd  # noqa: F401
    from yolo_for_turbines_amd import _lib
    _lib.lib()                       # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


@pytest.fixture(scope="module")
def golden():
    with open(G.OUT) as f:
        return json.load(f)


def test_the_golden_file_names_the_cases():
    with open(G.OUT) as f:
        assert sorted(json.load(f)) == sorted(G.key(n, t, r) for n in G.NAMES for t in G.TILES for r in G.ROUTES)


def test_the_cases_cover_the_k_step_counts():
    """1, 2, 3, 4, 5 and 9 K steps on the 1x1 cases (32 channels a step), 9 and 18 on the stride-2 ones."""
    steps = {c["k"] * c["k"] * c["cin"] // 32 for c in G.CASES.values()}
    assert {1, 2, 3, 4, 5, 9, 18} <= steps


@pytest.mark.gpu
@pytest.mark.parametrize("name", G.NAMES)
def test_bits_of_one_step_in_flight(L, golden, name):
    c, ops = G.operands(name)
    ready = s3r._prepared(L, c, ops[1])[0]
    for tile in G.TILES:
        for route in G.ROUTES:
            want = golden[G.key(name, tile, route)]
            runs = [G.launch(L, c, ops, tile, route, ready) for _ in range(5)]
            y, flag = runs[0]
            for again, flag_again in runs[1:]:
                assert flag_again == flag and torch.equal(again.view(torch.int32), y.view(torch.int32)), (tile, route, "two launches differ")
            assert G.digest(y) == want["sha256"], (tile, route)
            assert flag == want["nan_flag"], (tile, route, flag)
            if name in G.CASES:
                assert flag == 0
            else:
                assert not torch.isfinite(s3._view(c, y)).all()
            assert s3._outside_untouched(c, y, ops[5]), (tile, route)
