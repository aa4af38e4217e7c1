"""CPU: the dense flow estimator keeps its parameter names and its tensor expression off the GPU, the fused node
(AF.dense_estimator) is chosen only under the rule of the native flow head plus its own switch, and the two C entry points of
csrc/dense.hip check their arguments before any launch."""
import ctypes

import torch
import torch.nn.functional as F


def _cpu_bias_act(t, b, s):  # what a CPU twin substitutes for the GPU-only epilogue
    return F.leaky_relu(t + b.view(1, -1, 1, 1), s)


def test_estimator_keeps_parameter_names_and_runs_on_cpu(monkeypatch):
    from arflow_amd.models import blocks
    monkeypatch.setattr(blocks, 'bias_act', _cpu_bias_act)
    est = blocks.FlowEstimatorDense(19)
    keys = sorted(est.state_dict())
    assert keys == sorted('%s.0.%s' % (n, p) for n in ('conv1', 'conv2', 'conv3', 'conv4', 'conv5', 'conv_last')
                          for p in ('weight', 'bias'))
    assert isinstance(est.conv_last, blocks.HeadConv) and est.feat_dim == 19 + 448
    x = torch.randn(2, 19, 6, 10, requires_grad=True)
    x6, flow = est(x)
    assert x6.shape == (2, 19 + 448, 6, 10) and flow.shape == (2, 2, 6, 10)
    assert torch.equal(x6[:, 448:], x)  # the input sits at the end of the concatenation
    (x6.sum() + flow.sum()).backward()
    assert x.grad is not None and all(p.grad is not None for p in est.parameters())


def test_only_the_eligible_input_takes_the_fused_node(monkeypatch):
    from arflow_amd import functional as AF
    from arflow_amd.models import blocks

    def refuse(*a):
        raise AssertionError('fused dense estimator called')
    monkeypatch.setattr(AF, 'dense_estimator', refuse)

    class FakeCuda(torch.Tensor):  # a CPU tensor that claims to live on the GPU: only the module's own conditions are left
        is_cuda = True

    est = blocks.FlowEstimatorDense(8)
    x = torch.randn(1, 8, 6, 6)
    fake = x.as_subclass(FakeCuda)
    assert AF.dense_block_enabled() and est.native(fake)
    assert not est.native(x)  # never on a CPU tensor
    assert not est.native(fake.double())
    assert not est.native(fake[0])  # 4-D only
    monkeypatch.setattr(AF, '_DENSE_BLOCK', False)  # ARFLOW_DENSE_BLOCK=0
    assert not est.native(fake)
    monkeypatch.setattr(AF, '_DENSE_BLOCK', True)
    monkeypatch.setattr(AF, '_HEADCONV', False)  # the head belongs inside the node: without the native head, no node
    assert not est.native(fake)
    monkeypatch.setattr(AF, '_HEADCONV', True)
    assert est.native(fake)
    monkeypatch.setattr(blocks, 'bias_act', _cpu_bias_act)  # a twin with bias_act swapped out keeps the tensor expression
    assert not est.native(fake)
    ref = est(x)
    cur = x
    for layer in (est.conv1, est.conv2, est.conv3, est.conv4, est.conv5):
        cur = torch.cat([layer(cur), cur], 1)
    assert torch.equal(ref[0], cur) and torch.equal(ref[1], est.conv_last(cur))


def test_dense_argument_errors_without_gpu():
    from arflow_amd import _lib
    from arflow_amd import functional as AF
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    assert lib.arflow_abi_version() == 10  # the change is additive
    assert lib.arflow_dense_cat_fwd(None, one, one, one, 1, 1, 1, 4, 0.1, None) == -1001
    assert lib.arflow_dense_cat_fwd(one, None, None, one, 1, 1, 1, 4, 0.1, None) == -1001
    assert lib.arflow_dense_cat_fwd(one, None, one, one, 1, 0, 1, 4, 0.1, None) == -1002
    assert lib.arflow_dense_cat_fwd(one, None, one, one, 1, 1, 1, 0, 0.1, None) == -1002
    assert lib.arflow_dense_cat_fwd(one, None, one, ctypes.c_void_p(20), 1, 1, 1, 4, 0.1, None) == -1003  # float4 path: alignment
    assert lib.arflow_dense_gbias_rows(16, 96 * 160) == 16 * 4 and lib.arflow_dense_gbias_rows(1, 5) == 1
    assert lib.arflow_dense_gbias_rows(0, 5) == -1002
    arr = (AF._DenseSrc * 8)()
    for k in range(8):
        arr[k].ptr, arr[k].bstride, arr[k].scale = 16, 8, None
    srcs = ctypes.cast(arr, ctypes.c_void_p)
    assert lib.arflow_dense_grad_gather(None, 1, None, 0, one, None, 1, 2, 4, 0.1, None) == -1001
    assert lib.arflow_dense_grad_gather(srcs, 1, None, 0, None, None, 1, 2, 4, 0.1, None) == -1001
    assert lib.arflow_dense_grad_gather(srcs, 0, None, 0, one, None, 1, 2, 4, 0.1, None) == -1003
    assert lib.arflow_dense_grad_gather(srcs, 9, None, 0, one, None, 1, 2, 4, 0.1, None) == -1003
    assert lib.arflow_dense_grad_gather(srcs, 2, None, 0, one, None, 0, 2, 4, 0.1, None) == -1002
    assert lib.arflow_dense_grad_gather(srcs, 2, one, 7, one, None, 1, 2, 4, 0.1, None) == -1003  # act stride below oc * HW
    arr[1].bstride = 7
    assert lib.arflow_dense_grad_gather(srcs, 2, None, 0, one, None, 1, 2, 4, 0.1, None) == -1003  # source stride below oc * HW
    arr[1].bstride, arr[1].ptr = 8, None
    assert lib.arflow_dense_grad_gather(srcs, 2, None, 0, one, None, 1, 2, 4, 0.1, None) == -1001


def test_fused_node_refuses_cpu_tensors():
    import pytest
    from arflow_amd import _lib
    from arflow_amd import functional as AF
    from arflow_amd.models import blocks
    est = blocks.FlowEstimatorDense(8)
    params = [p for n in ('conv1', 'conv2', 'conv3', 'conv4', 'conv5', 'conv_last') for p in getattr(est, n)[0].parameters()]
    with pytest.raises(_lib.ArflowHipError):
        AF.dense_estimator(torch.zeros(1, 8, 4, 4), 0.1, params)
