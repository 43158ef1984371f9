"""CPU-side checks of the weight average (`yolo_for_turbines_amd/ema.py`): the decay schedule of the reference the GPU tests
compare against (`tests/ema_ref.py`), the argument checks of ``ModelEMA``, and the checkpoint format with and without an
average. No GPU and no library needed."""
import numpy as np
import pytest
import torch

from tests import ema_ref


def test_ema_ref_decay_schedule():
    decay = 0.9998
    for t in (0, 1, 8):
        d, omd = ema_ref.coeffs(t, decay, True)
        assert d == float(np.float32(1 + t) / np.float32(10 + t))
        assert omd == float(np.float32(1.0) - np.float32(d))
    assert ema_ref.coeffs(0, decay, True)[0] == float(np.float32(0.1))
    # the crossover: the first t whose quotient reaches the decay, found here rather than written down
    dec32 = np.float32(decay)
    cross = next(t for t in range(10 ** 6) if np.float32(1 + t) / np.float32(10 + t) >= dec32)
    assert cross > 8
    assert ema_ref.coeffs(cross - 1, decay, True)[0] < float(dec32)
    for t in (cross, cross + 1, cross + 1000, 10 * cross):
        assert ema_ref.coeffs(t, decay, True) == (float(dec32), float(np.float32(1.0) - dec32))
    ds = [ema_ref.coeffs(t, decay, True)[0] for t in range(cross + 50)]
    assert all(a <= b for a, b in zip(ds, ds[1:])), "the decay never decreases"
    assert ema_ref.coeffs(0, decay, False) == (float(dec32), float(np.float32(1.0) - dec32))
    # a small decay, as the GPU tests use it: the crossover falls inside a dozen updates
    small = [ema_ref.coeffs(t, 0.5, True)[0] for t in range(12)]
    assert small[0] < 0.5 and small[-1] == 0.5 and small[7] < 0.5 <= small[8]


def test_ema_ref_update_is_mul_then_add():
    src = {"w": torch.tensor([1.0, -2.0, 0.5]), "n": torch.tensor(7)}
    ref = ema_ref.EmaRef({"w": torch.zeros(3), "n": torch.tensor(0)}, decay=0.5, warmup=True)
    ref.update(src)
    d, omd = ema_ref.coeffs(0, 0.5, True)
    assert torch.equal(ref.shadow["w"], torch.zeros(3).mul_(d).add_(src["w"], alpha=omd))
    assert int(ref.shadow["n"]) == 7 and ref.updates == 1


def test_model_ema_argument_checks():
    import yolo_for_turbines_amd as yt
    cpu_model = torch.nn.Linear(4, 3)
    with pytest.raises(TypeError):                              # no CPU path
        yt.ModelEMA(cpu_model)
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            yt.ModelEMA(cpu_model, decay=bad)
    with pytest.raises(TypeError):                              # attach is for yt.SGD; everything else calls update()
        yt.ModelEMA.attach(object.__new__(yt.ModelEMA), torch.optim.SGD(cpu_model.parameters(), lr=0.1))
    # update() while attached would average twice. An average cannot be constructed without a GPU, so the attached state is
    # set by hand on a bare instance: the check comes before anything touches the device.
    ema = object.__new__(yt.ModelEMA)
    ema._attached = object()
    with pytest.raises(RuntimeError, match="twice"):
        ema.update()


class _Stub:
    def __init__(self):
        self.loaded = None

    def state_dict(self):
        return {"module": {"w": torch.ones(2)}, "updates": 3, "decay": 0.5, "warmup": True}

    def load_state_dict(self, sd):
        self.loaded = sd


def test_checkpoint_keys_with_and_without_an_average(tmp_path):
    import yolo_for_turbines_amd as yt
    model = torch.nn.Linear(4, 3)
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9)
    plain, with_ema = str(tmp_path / "plain.pth.tar"), str(tmp_path / "ema.pth.tar")
    yt.save_checkpoint(model, opt, filename=plain)
    assert set(torch.load(plain).keys()) == {"state_dict", "optimizer"}
    yt.save_checkpoint(model, opt, filename=with_ema, ema=_Stub())
    ck = torch.load(with_ema)
    assert set(ck.keys()) == {"state_dict", "optimizer", "ema"}
    assert ck["ema"]["updates"] == 3 and torch.equal(ck["ema"]["module"]["w"], torch.ones(2))
    m2 = torch.nn.Linear(4, 3)
    o2 = torch.optim.SGD(m2.parameters(), lr=0.1, momentum=0.9)
    stub = _Stub()
    with pytest.raises(KeyError, match="ema"):
        yt.load_checkpoint(m2, o2, lr=0.01, filename=plain, ema=stub)
    assert stub.loaded is None
    yt.load_checkpoint(m2, o2, lr=0.01, filename=with_ema, ema=stub)
    assert stub.loaded["updates"] == 3 and torch.equal(m2.weight, model.weight)
    yt.load_checkpoint(m2, o2, lr=0.01, filename=with_ema)    # an average in the file is no obligation to load it
