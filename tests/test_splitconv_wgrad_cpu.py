"""CPU: the split-bf16 weight gradient's entry points validate their arguments without a GPU, the workspace size follows the
chunking csrc/splitconv_wgrad.hip documents, the routing predicate has its switches and its floor, and a torch emulation
documents the summation order: per staged row of 64 pixels a fresh accumulator takes the small plane products first and the
(0, 0) products after, rows are added to a running fp32 total per chunk, chunks are added in float64."""
import ctypes
import os

import pytest
import torch

U = 2.0 ** -24


@pytest.fixture(scope='module')
def lib():
    from arflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_argument_errors_without_gpu(lib):
    one = ctypes.c_void_p(16)
    call = lib.arflow_splitconv_wgrad
    ok = (1, 1, 1, 1, 1)
    assert call(None, 1, one, 1, one, one, *ok, None) == -1001
    assert call(one, 1, None, 1, one, one, *ok, None) == -1001
    assert call(one, 1, one, 1, None, one, *ok, None) == -1001
    assert call(one, 1, one, 1, one, None, *ok, None) == -1001
    for bad in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, -1, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0)):
        assert call(one, 1 << 40, one, 1 << 40, one, one, *bad, None) == -1002
        assert lib.arflow_splitconv_wgrad_ws_bytes(*bad) == -1002
    big = 1 << 40
    assert call(one, big, one, big, one, one, 64, 597, 128, 384, 640, None) == -1002  # N C H W overflows int
    assert call(one, big, one, big, one, one, 64, 128, 597, 384, 640, None) == -1002  # N K H W overflows int
    assert call(one, big, one, big, one, one, 1, 1 << 15, 1 << 15, 1, 1, None) == -1002  # 9 K C overflows int
    assert lib.arflow_splitconv_wgrad_ws_bytes(64, 597, 128, 384, 640) == -1002
    assert lib.arflow_splitconv_wgrad_ws_bytes(1, 1 << 15, 1 << 15, 1, 1) == -1002
    # a batch stride below the sample's size (only read where there is a second sample), or negative
    assert call(one, 3 * 4 * 5 - 1, one, big, one, one, 2, 3, 2, 4, 5, None) == -1002
    assert call(one, big, one, 2 * 4 * 5 - 1, one, one, 2, 3, 2, 4, 5, None) == -1002
    assert call(one, -1, one, 1, one, one, *ok, None) == -1002
    for i in range(3):  # x, dy, dw off a float boundary; ws off a 16-byte boundary
        ptrs = [one, one, one, one]
        ptrs[i] = ctypes.c_void_p(18)
        assert call(ptrs[0], 1, ptrs[1], 1, ptrs[2], ptrs[3], *ok, None) == -1003
    assert call(one, 1, one, 1, one, ctypes.c_void_p(20), *ok, None) == -1003


def test_ws_bytes_worked_out_by_hand(lib):
    # 597 -> 128 at 16 x 96 x 160: 20 groups of 8 columns in 3 strips of 8, 8 and 4; 19 C tiles x 2 K chunks x 16 samples x 3
    # strips = 1824 workgroups already fill the chip, so one row block of 96 rows: 16 * 3 * 1 = 48 chunks of [9][128][597] floats
    assert lib.arflow_splitconv_wgrad_ws_bytes(16, 597, 128, 96, 160) == 48 * 9 * 128 * 597 * 4
    # 32 -> 32 at 16 x 48 x 80: 10 groups in 2 strips of 6 and 4; 1 x 1 x 16 x 2 = 32 units want 32 row blocks, i.e. 2 rows, raised
    # to the minimum of 4: 12 row blocks; 16 * 2 * 12 = 384 chunks
    assert lib.arflow_splitconv_wgrad_ws_bytes(16, 32, 32, 48, 80) == 384 * 9 * 32 * 32 * 4
    assert lib.arflow_splitconv_wgrad_ws_bytes(1, 1, 1, 1, 1) == 36


def test_negative_ws_bytes_raises_before_any_allocation(lib, monkeypatch):
    from arflow_amd import _lib, functional as AF
    monkeypatch.setattr(AF, '_need_gpu', lambda *a: None)
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: pytest.fail('torch.empty reached with a negative size'))
    x = torch.zeros(1, 1 << 15, 1, 1)
    gy = torch.zeros(1, 1 << 15, 1, 1)
    with pytest.raises(_lib.ArflowHipError):
        AF.splitconv_wgrad(x, gy)


def test_predicate_switches_and_floor(monkeypatch):
    from arflow_amd import functional as AF
    from arflow_amd.models import blocks
    monkeypatch.setattr(AF, '_SPLITCONV', True)
    monkeypatch.setattr(AF, '_SPLITCONV_WGRAD', True)
    # the unpatched rule refuses every shape below N H W = 16 x 48 x 80, whatever the channels
    for N, H, W in ((16, 24, 40), (8, 48, 80), (16, 48, 79), (4, 96, 160), (1, 1, 1)):
        for C, K in ((147, 128), (597, 128), (563, 32), (64, 32), (128, 128)):
            assert not AF.splitconv_wgrad_takes(N, C, K, H, W)
    asked = []
    monkeypatch.setattr(AF, '_splitconv_wgrad_rule', lambda *a: (asked.append(a), True)[1])

    class OnGpu:  # the predicate reads these four things of its input; no GPU is touched
        is_cuda, dtype, shape = True, torch.float32, (16, 147, 48, 80)

        def dim(self):
            return 4
    layer = blocks.conv(147, 128)
    assert layer.split_wgrad_route(OnGpu()) is True and asked == [(16, 147, 128, 48, 80)]
    assert len(layer.split_route(OnGpu())) == 2
    assert blocks.conv(147, 128, dilation=2).split_wgrad_route(OnGpu()) is False
    assert blocks.conv(147, 128).split_wgrad_route(torch.zeros(1, 147, 4, 4)) is False  # a CPU tensor
    monkeypatch.setattr(AF, '_SPLITCONV_WGRAD', False)  # ARFLOW_SPLITCONV_WGRAD=0
    assert not AF.splitconv_wgrad_takes(16, 147, 128, 96, 160) and layer.split_wgrad_route(OnGpu()) is False
    monkeypatch.setattr(AF, '_SPLITCONV_WGRAD', True)
    monkeypatch.setattr(AF, '_SPLITCONV', False)  # ARFLOW_SPLITCONV=0 switches the weight gradient off as well
    assert not AF.splitconv_wgrad_takes(16, 147, 128, 96, 160) and layer.split_wgrad_route(OnGpu()) is False


def split3(t):
    b0 = t.bfloat16().float()
    r1 = t - b0
    b1 = r1.bfloat16().float()
    return b0, b1, (r1 - b1).bfloat16().float()


def test_bounded_chain_matches_float64_like_plain_fp32():
    """4 chunks of 96 rows of 64 pixels (24 576 terms per output, operands 3 + randn): e = |err| / sum |a b| against float64
    for the kernel's order and for plain fp32 partial sums of 16 in one chain."""
    g = torch.Generator().manual_seed(2)
    outs, chunks, rows, row = 256, 4, 96, 64
    n = chunks * rows * row
    a, b = 3.0 + torch.randn(outs, n, generator=g), 3.0 + torch.randn(outs, n, generator=g)
    ref = (a.double() * b.double()).sum(1)
    S = (a.double() * b.double()).abs().sum(1)
    pa, pb = split3(a), split3(b)
    small, big = ((0, 2), (1, 1), (0, 1), (2, 0), (1, 0)), ((0, 0),)  # (dy plane, x plane), the kernel's order per step
    total = torch.zeros(outs, dtype=torch.float64)
    for ch in range(chunks):
        tot = torch.zeros(outs)
        for r in range(rows):
            acc, base = torch.zeros(outs), (ch * rows + r) * row
            for part in (small, big):
                for k0 in range(base, base + row, 16):
                    for i, j in part:  # one MFMA: 16 exact products added to the accumulator, one rounding
                        acc = (acc.double() + (pa[i][:, k0:k0 + 16].double() * pb[j][:, k0:k0 + 16].double()).sum(1)).float()
            tot = tot + acc
        total += tot.double()
    got = total.float()
    plain = torch.zeros(outs)
    for k0 in range(0, n, 16):
        plain = plain + (a[:, k0:k0 + 16] * b[:, k0:k0 + 16]).sum(1)
    e = lambda t: float(((t.double() - ref).abs() / S).max()) / U
    e6, e32 = e(got), e(plain)
    print('bounded six-product chain %.2f u, plain fp32 partial sums of 16: %.2f u' % (e6, e32))
    assert e6 <= 2.0 * e32  # the criterion of the GPU test
