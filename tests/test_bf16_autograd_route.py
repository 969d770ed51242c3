"""The routing decision of the bf16 autograd path (no GPU needed): which networks bf16_train_supported() takes, and that the
request predicate is off outside bf16 autocast.  The numerics are in test_gpu_autograd_bf16.py."""
import pytest
import torch
from torch import nn

from yogo_amd.engine import Engine, backward_bf16_train, bf16_train_supported, bf16_training_requested
from yogo_amd.model_defns import MODELS


def _net(*blocks):
    return nn.Sequential(*blocks)


def _blk(cin, cout, k=3, s=1, bn=False, act="leaky", drop=0.0, bias=True):
    mods = [nn.Conv2d(cin, cout, k, stride=s, padding=1 if k == 3 else 0, bias=bias)]
    if bn:
        mods.append(nn.BatchNorm2d(cout))
    if act == "leaky":
        mods.append(nn.LeakyReLU())
    elif act == "silu":
        mods.append(nn.SiLU())
    if drop > 0:
        mods.append(nn.Dropout2d(drop))
    return nn.Sequential(*mods)


@pytest.mark.parametrize("name", sorted(n for n in MODELS if n != "convnext_small"))
def test_registered_models_are_supported(name):
    for rgb in (False, True):
        assert bf16_train_supported(Engine(MODELS[name](7, rgb)))


def test_unsupported_networks():
    head = nn.Conv2d(32, 12, 1)
    ok = _net(_blk(1, 16, s=2, bn=True, bias=False), _blk(16, 32, drop=0.1), head)
    assert bf16_train_supported(Engine(ok))
    # first convolution: 1x1, or not 1 / 3 input channels
    assert not bf16_train_supported(Engine(_net(_blk(1, 16, k=1), _blk(16, 32), head)))
    assert not bf16_train_supported(Engine(_net(_blk(4, 16), _blk(16, 32), head)))
    # a first or last SiLU block without BatchNorm (with BatchNorm it is fine)
    assert not bf16_train_supported(Engine(_net(_blk(1, 16, act="silu"), _blk(16, 32), head)))
    assert bf16_train_supported(Engine(_net(_blk(1, 16, bn=True, act="silu"), _blk(16, 32, act="silu"), head)))
    assert not bf16_train_supported(Engine(_net(_blk(1, 16), _blk(16, 32), _blk(32, 12, act="silu"))))
    # BatchNorm or Dropout2d on the last layer
    assert not bf16_train_supported(Engine(_net(_blk(1, 16), _blk(16, 32), _blk(32, 12, k=1, bn=True, act=None))))
    assert not bf16_train_supported(Engine(_net(_blk(1, 16), _blk(16, 32), _blk(32, 12, k=1, act=None, drop=0.1))))
    # BatchNorm2d(momentum=None)
    net = _net(_blk(1, 16, s=2, bn=True), _blk(16, 32), head)
    net[0][1].momentum = None
    assert not bf16_train_supported(Engine(net))
    # a network of one layer, and layers whose channels do not chain
    assert not bf16_train_supported(Engine(_net(_blk(1, 12, act=None))))
    assert not bf16_train_supported(Engine(_net(_blk(1, 16), _blk(8, 32), head)))


def test_training_request_is_off_outside_bf16_autocast():
    assert not bf16_training_requested()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not bf16_training_requested()   # (CPU autocast is not a request for the GPU kernels)


def test_stop_at_outside_the_network_raises():
    eng = Engine(MODELS["base_model"](7, False))
    for bad in (-1, len(eng.layers)):
        with pytest.raises(ValueError, match="stop_at"):
            backward_bf16_train(eng, [], torch.zeros(1, 12, 2, 2), stop_at=bad)
