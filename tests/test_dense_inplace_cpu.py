"""No GPU: arflow_splitconv_fwd_ex validates its arguments before any launch (include/arflow_hip.h), the ABI version is
unchanged by the additive entry point, and the in-place routing of the dense estimator keeps to its floor and switches."""
import ctypes
import os

import pytest


@pytest.fixture(scope='module')
def lib():
    from arflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_argument_errors_without_gpu(lib):
    one = ctypes.c_void_p(16)
    call = lib.arflow_splitconv_fwd_ex
    dims = (2, 3, 2, 4, 5)  # N, C, K, H, W
    xs, ys = 3 * 4 * 5, 2 * 4 * 5
    assert call(None, xs, one, one, ys, None, 0, 0.0, *dims, None) == -1001
    assert call(one, xs, None, one, ys, None, 0, 0.0, *dims, None) == -1001
    assert call(one, xs, one, None, ys, None, 0, 0.0, *dims, None) == -1001
    for bad in ((0, 3, 2, 4, 5), (2, 0, 2, 4, 5), (2, 3, -1, 4, 5), (2, 3, 2, 0, 5), (2, 3, 2, 4, 0)):
        assert call(one, 1 << 20, one, one, 1 << 20, None, 0, 0.0, *bad, None) == -1002
    # a batch stride below the sample's size, or negative
    assert call(one, xs - 1, one, one, ys, None, 0, 0.0, *dims, None) == -1002
    assert call(one, xs, one, one, ys - 1, None, 0, 0.0, *dims, None) == -1002
    assert call(one, -1, one, one, ys, None, 0, 0.0, *dims, None) == -1002
    assert call(one, xs, one, one, -1, None, 0, 0.0, *dims, None) == -1002
    # N * stride past INT_MAX, for either tensor; the packed sizes past INT_MAX as in arflow_splitconv_fwd
    assert call(one, 1 << 30, one, one, ys, None, 0, 0.0, *dims, None) == -1002
    assert call(one, xs, one, one, 1 << 30, None, 0, 0.0, *dims, None) == -1002
    assert call(one, 1 << 40, one, one, 1 << 40, None, 0, 0.0, 64, 597, 128, 384, 640, None) == -1002
    # the epilogue selector, and a bias without the epilogue
    for act in (-1, 2, 7):
        assert call(one, xs, one, one, ys, None, act, 0.1, *dims, None) == -1003
    assert call(one, xs, one, one, ys, one, 0, 0.1, *dims, None) == -1003
    assert call(one, xs, ctypes.c_void_p(24), one, ys, None, 0, 0.0, *dims, None) == -1003  # packed off a 16-byte boundary
    # the packed entry point is the same checks with packed strides
    assert lib.arflow_splitconv_fwd(None, one, one, *dims, None) == -1001
    assert lib.arflow_splitconv_fwd(one, one, one, 0, 3, 2, 4, 5, None) == -1002
    assert lib.arflow_splitconv_fwd(one, one, one, 64, 597, 128, 384, 640, None) == -1002


def test_abi_version_is_unchanged(lib):
    assert lib.arflow_abi_version() == 10


def test_in_place_weight_gradient_routing(monkeypatch):
    from arflow_amd import functional as AF
    monkeypatch.setattr(AF, '_SPLITCONV', True)
    monkeypatch.setattr(AF, '_SPLITCONV_WGRAD', True)
    # never below the floor of splitconv_wgrad_takes (the shapes of the tests keep MIOpen's dw), whatever the channels
    for N, H, W in ((16, 24, 40), (8, 48, 80), (4, 96, 160), (2, 10, 12), (1, 1, 1)):
        for C, K in ((147, 128), (275, 128), (403, 96), (499, 64), (563, 32)):
            assert not AF._inplace_wgrad_takes(N, C, K, H, W)
    # whatever splitconv_wgrad_takes routes stays routed in place
    for C, K in ((499, 64), (563, 32)):
        assert AF.splitconv_wgrad_takes(16, C, K, 96, 160) and AF._inplace_wgrad_takes(16, C, K, 96, 160)
    # and both switches turn it off
    monkeypatch.setattr(AF, '_SPLITCONV_WGRAD', False)
    assert not any(AF._inplace_wgrad_takes(16, C, K, 96, 160) for C, K in ((147, 128), (275, 128), (403, 96), (499, 64), (563, 32)))
    monkeypatch.setattr(AF, '_SPLITCONV_WGRAD', True)
    monkeypatch.setattr(AF, '_SPLITCONV', False)
    assert not any(AF._inplace_wgrad_takes(16, C, K, 96, 160) for C, K in ((147, 128), (275, 128), (403, 96), (499, 64), (563, 32)))


def test_disjoint_views():
    import torch
    from arflow_amd import functional as AF
    buf = torch.zeros(2, 10, 3, 4)
    bs = 10 * 12
    assert AF._disjoint(buf[:, 6:], bs, buf[:, :6], bs) and AF._disjoint(buf[:, 6:], bs, buf[:, 2:5], bs)
    assert AF._disjoint(buf[:, :4], bs, buf[:, 4:], bs)
    assert not AF._disjoint(buf[:, 6:], bs, buf[:, 1:7], bs) and not AF._disjoint(buf[:, 6:], bs, buf[:, 6:], bs)
    assert not AF._disjoint(buf[:, :5], bs, buf[:, 4:], bs)
    other = torch.zeros(2, 6, 3, 4)
    assert AF._disjoint(buf[:, 6:], bs, other, 6 * 12)
    one = torch.zeros(1, 10, 3, 4)
    assert AF._disjoint(one[:, 6:], 4 * 12, one[:, :6], 6 * 12) and not AF._disjoint(one[:, 6:], 4 * 12, one[:, 3:7], 4 * 12)
