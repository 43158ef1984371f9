"""CPU checks of `guards.SlotGuard`, the one freshness check behind the eval fast path and the training launch tables:
plain ``nn.Conv2d`` / ``nn.BatchNorm2d`` modules, CPU tensors, no device."""
import gc
import weakref

import pytest
import torch
import torch.nn as nn

from yolo_for_turbines_amd.guards import SlotGuard


def _mods():
    torch.manual_seed(0)
    return nn.Conv2d(3, 4, 3, bias=False), nn.BatchNorm2d(4)


def _slots(conv, bn):
    """Every parameter and buffer slot, as the train plan enumerates them (the conv's bias slot holds None)."""
    return ([(m._parameters, k) for m in (conv, bn) for k in m._parameters] +
            [(m._buffers, k) for m in (conv, bn) for k in m._buffers])


def _values(bn):
    return [(vars(bn), k) for k in ("momentum", "eps", "track_running_stats")]


@pytest.mark.parametrize("versions", [False, True])
def test_ok_while_nothing_changed(versions):
    conv, bn = _mods()
    g = SlotGuard(_slots(conv, bn), versions=versions, values=_values(bn))
    assert len(g.tensors) == 1 + 2 + 3                       # conv.weight; gamma, beta; the two statistics and the counter
    assert g.ok() and g.ok()
    conv(torch.zeros(1, 3, 5, 5))                            # reading the tensors changes nothing
    assert g.ok()


@pytest.mark.parametrize("versions", [False, True])
@pytest.mark.parametrize("which", ["weight", "running_mean", "num_batches_tracked"])
def test_another_object_in_the_slot_fails_wherever_it_lives(versions, which):
    conv, bn = _mods()
    g = SlotGuard(_slots(conv, bn), versions=versions, values=_values(bn))
    old = getattr(bn, which)
    if which == "weight":
        bn.weight = nn.Parameter(old.detach().clone())       # new object, new storage
    else:
        setattr(bn, which, old.clone())
    assert not g.ok()
    # a new object over the SAME storage (same address, same values) is still another object
    conv2, bn2 = _mods()
    g2 = SlotGuard(_slots(conv2, bn2), versions=versions, values=_values(bn2))
    old2 = getattr(bn2, which)
    if which == "weight":
        bn2.weight = nn.Parameter(old2.detach())
    else:
        setattr(bn2, which, old2.detach().view_as(old2))
    assert getattr(bn2, which).data_ptr() == old2.data_ptr() and getattr(bn2, which) is not old2
    assert not g2.ok()


@pytest.mark.parametrize("versions", [False, True])
def test_same_object_with_moved_storage_fails(versions):
    conv, bn = _mods()
    g = SlotGuard(_slots(conv, bn), versions=versions, values=_values(bn))
    w = conv.weight
    w.data = w.data.clone()
    assert conv.weight is w and not g.ok()


def test_in_place_write_fails_only_with_versions_on():
    conv, bn = _mods()
    plain = SlotGuard(_slots(conv, bn), values=_values(bn))
    strict = SlotGuard(_slots(conv, bn), versions=True, values=_values(bn))
    with torch.no_grad():
        bn.running_var.mul_(2.0)
    assert plain.ok()                                        # training writes every tensor each step
    assert not strict.ok()


@pytest.mark.parametrize("key,new", [("momentum", 0.2), ("momentum", None), ("eps", 1e-3), ("track_running_stats", False)])
def test_changed_value_fails(key, new):
    conv, bn = _mods()
    g = SlotGuard(_slots(conv, bn), values=_values(bn))
    setattr(bn, key, getattr(bn, key))                       # an equal value, set again, is no change
    bn.momentum = float("0.1")                               # (equal, and another float object)
    assert g.ok()
    setattr(bn, key, new)
    assert not g.ok()


def test_empty_slot_that_gets_a_tensor_fails():
    conv, bn = _mods()
    g = SlotGuard(_slots(conv, bn), values=_values(bn))
    assert any(o is conv._parameters and k == "bias" and v is None for o, k, v in g.values)
    conv.bias = nn.Parameter(torch.zeros(4))
    assert not g.ok()


def test_guard_keeps_only_what_it_was_given():
    """The guard holds the remembered tensors (that is what makes `is` meaningful); dropping the guard frees them."""
    conv, bn = _mods()
    g = SlotGuard(_slots(conv, bn))
    old = weakref.ref(bn.weight)
    bn.weight = nn.Parameter(torch.ones(4))
    gc.collect()
    assert old() is not None and not g.ok()
    del g
    gc.collect()
    assert old() is None
