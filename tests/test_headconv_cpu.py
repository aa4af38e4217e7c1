"""CPU: the flow-head module built by conv(..., isReLU=False) keeps the reference's parameter names, runs on CPU tensors
through F.conv2d, and only a 3x3 / stride 1 / padding 1 / dilation 1 / two-output layer is eligible for the native path."""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F


def test_head_keeps_parameter_names_and_runs_on_cpu():
    from arflow_amd.models import blocks
    head = blocks.conv(8, 2, isReLU=False)
    assert isinstance(head, nn.Sequential) and isinstance(head, blocks.HeadConv)
    assert sorted(head.state_dict()) == ['0.bias', '0.weight']
    plain = nn.Sequential(nn.Conv2d(8, 2, 3, padding=1))
    plain.load_state_dict(head.state_dict())  # a checkpoint of the plain Sequential loads by name, both ways
    head.load_state_dict(plain.state_dict())
    x = torch.randn(2, 8, 9, 11, requires_grad=True)
    y = head(x)
    assert torch.equal(y, plain(x))
    y.sum().backward()
    assert x.grad is not None and head[0].weight.grad is not None and head[0].bias.grad is not None


def test_layers_outside_the_conditions_take_conv2d(monkeypatch):
    from arflow_amd import functional as AF
    from arflow_amd.models import blocks

    def refuse(*a):
        raise AssertionError('native head convolution called')
    monkeypatch.setattr(AF, 'head_conv', refuse)

    class FakeCuda(torch.Tensor):  # a CPU tensor that claims to live on the GPU: only the layer's own conditions are left
        is_cuda = True

    x = torch.randn(1, 8, 12, 12)
    fake = x.as_subclass(FakeCuda)
    assert blocks.conv(8, 2, isReLU=False).native(fake)  # the eligible layer: 3x3, stride 1, padding 1, 2 outputs
    assert not blocks.conv(8, 2, isReLU=False).native(x)  # ... but never on a CPU tensor
    assert not blocks.conv(8, 2, isReLU=False).native(fake.double())
    others = {'dilation 2': blocks.conv(8, 2, dilation=2, isReLU=False), 'stride 2': blocks.conv(8, 2, stride=2, isReLU=False),
              '4 outputs': blocks.conv(8, 4, isReLU=False), '1x1': blocks.conv(8, 2, kernel_size=1, isReLU=False)}
    for what, layer in others.items():
        assert not layer.native(fake), what
        c = layer[0]
        assert torch.equal(layer(x), F.conv2d(x, c.weight, c.bias, c.stride, c.padding, c.dilation)), what
    monkeypatch.setattr(blocks, 'bias_act', lambda t, b, s: t)  # a twin with bias_act swapped out keeps F.conv2d
    assert not blocks.conv(8, 2, isReLU=False).native(fake)


def test_headconv_argument_errors_without_gpu():
    from arflow_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    assert lib.arflow_headconv_fwd(None, one, one, one, 1, 1, 1, 1, None) == -1001
    assert lib.arflow_headconv_fwd(one, one, None, one, 1, 0, 1, 1, None) == -1002
    assert lib.arflow_headconv_bwd_data(one, one, None, 1, 1, 1, 1, None) == -1001
    assert lib.arflow_headconv_bwd_data(one, one, one, 1, 1, -3, 1, None) == -1002
    assert lib.arflow_headconv_bwd_weight(one, one, one, None, None, 1, 1, 1, 1, None) == -1001
    assert lib.arflow_headconv_bwd_weight(one, one, one, None, ctypes.c_void_p(20), 1, 1, 1, 1, None) == -1003  # ws alignment
    assert lib.arflow_headconv_bwd_weight_ws_bytes(16, 595, 96, 160) == 8 * 240 * (595 * 18 + 2)
    assert lib.arflow_headconv_bwd_weight_ws_bytes(1, 1, 0, 1) == -1002
