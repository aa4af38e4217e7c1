"""CPU: the split-bf16 convolution's entry points validate their arguments without a GPU, the routing predicate declines what
the kernel does not compute, and a torch emulation documents the arithmetic csrc/splitconv.hip implements: an fp32 number is
the exact sum of three bf16 numbers, and six of the nine plane products, added smallest first in fp32 per block of 32 channels, are as close to the
float64 result as a plain fp32 product chain (measure and criterion of tests/test_splitconv_gpu.py)."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn

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
    assert lib.arflow_abi_version() == 10  # additive change
    assert lib.arflow_splitconv_pack(None, one, 1, 1, 0, None) == -1001
    assert lib.arflow_splitconv_pack(one, None, 1, 1, 0, None) == -1001
    assert lib.arflow_splitconv_pack(one, one, 0, 1, 0, None) == -1002
    assert lib.arflow_splitconv_pack(one, one, 1, -2, 1, None) == -1002
    assert lib.arflow_splitconv_pack(one, one, 1 << 20, 1 << 20, 0, None) == -1002  # 9 K C overflows int
    assert lib.arflow_splitconv_pack(one, one, 1, 1, 2, None) == -1003
    assert lib.arflow_splitconv_pack(one, ctypes.c_void_p(20), 1, 1, 0, None) == -1003  # packed alignment
    assert lib.arflow_splitconv_fwd(None, one, one, 1, 1, 1, 1, 1, None) == -1001
    assert lib.arflow_splitconv_fwd(one, None, one, 1, 1, 1, 1, 1, None) == -1001
    assert lib.arflow_splitconv_fwd(one, one, None, 1, 1, 1, 1, 1, None) == -1001
    for bad in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, -1, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0)):
        assert lib.arflow_splitconv_fwd(one, one, one, *bad, None) == -1002
    assert lib.arflow_splitconv_fwd(one, one, one, 64, 597, 128, 384, 640, None) == -1002  # N C H W overflows int
    assert lib.arflow_splitconv_fwd(one, one, one, 64, 128, 597, 384, 640, None) == -1002  # N K H W overflows int
    assert lib.arflow_splitconv_fwd(one, ctypes.c_void_p(20), one, 1, 1, 1, 1, 1, None) == -1003
    # three planes x nine taps x K padded to 32 x C padded to 32, two bytes each
    assert lib.arflow_splitconv_pack_bytes(128, 597) == 3 * 9 * 128 * 608 * 2
    assert lib.arflow_splitconv_pack_bytes(1, 1) == 3 * 9 * 32 * 32 * 2
    assert lib.arflow_splitconv_pack_bytes(0, 4) == -1002


def test_routing_declines_what_the_kernel_does_not_compute(monkeypatch):
    from arflow_amd import functional as AF
    from arflow_amd.models import blocks
    monkeypatch.setattr(AF, '_SPLITCONV', True)
    monkeypatch.setattr(AF, '_splitconv_rule', lambda *a: True)  # every SHAPE routed: only the layer's kind can decline

    class OnGpu:  # the predicate reads these four things of its input; no GPU is touched
        is_cuda, dtype, shape = True, torch.float32, (16, 64, 96, 160)

        def dim(self):
            return 4
    x = OnGpu()
    assert blocks.conv(64, 32).split_route(x) == (True, True)
    assert blocks.conv(64, 32, stride=2).split_route(x) == (False, False)
    assert blocks.conv(64, 32, dilation=2).split_route(x) == (False, False)
    assert blocks.conv(64, 32, kernel_size=1).split_route(x) == (False, False)
    assert blocks.conv(64, 32).double().split_route(x) == (False, False)
    half = OnGpu()
    half.dtype = torch.float16
    assert blocks.conv(64, 32).split_route(half) == (False, False)
    assert blocks.conv(64, 32).split_route(torch.zeros(1, 64, 4, 4)) == (False, False)  # a CPU tensor
    grouped = blocks.ConvAct(nn.Conv2d(64, 32, 3, padding=1, groups=2), nn.LeakyReLU(0.1))
    assert grouped.split_route(x) == (False, False)
    monkeypatch.setattr(blocks, 'bias_act', lambda t, bias, s: t)  # a twin that has swapped bias_act out
    assert blocks.conv(64, 32).split_route(x) == (False, False)
    monkeypatch.undo()
    monkeypatch.setattr(AF, '_SPLITCONV', False)  # ARFLOW_SPLITCONV=0
    assert not AF.splitconv_takes(16, 597, 128, 96, 160) and blocks.conv(597, 128).split_route(x) == (False, False)


def test_forward_and_data_gradient_ask_with_swapped_channels(monkeypatch):
    from arflow_amd import functional as AF
    from arflow_amd.models import blocks
    asked = []
    monkeypatch.setattr(AF, '_SPLITCONV', True)
    monkeypatch.setattr(AF, '_splitconv_rule', lambda *a: (asked.append(a), a[1] > a[2])[1])

    class OnGpu:
        is_cuda, dtype, shape = True, torch.float32, (16, 147, 48, 80)

        def dim(self):
            return 4
    assert blocks.conv(147, 128).split_route(OnGpu()) == (True, False)
    assert asked == [(16, 147, 128, 48, 80), (16, 128, 147, 48, 80)]


def split3(t):
    """The three bf16 planes of an fp32 tensor (round to nearest even), as fp32."""
    b0 = t.bfloat16().float()
    r1 = t - b0
    b1 = r1.bfloat16().float()
    b2 = (r1 - b1).bfloat16().float()
    return b0, b1, b2


def pack_emulation(w, transpose_flip):
    """What arflow_splitconv_pack stores, before the fragment ordering: planes of W[k][c][tap], or of w[c][k][8 - tap]."""
    if transpose_flip:
        w = w.transpose(0, 1).flip(2, 3)
    return split3(w.contiguous())


def test_three_planes_reproduce_the_weights_exactly():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(33, 17, 3, 3, generator=g) * torch.exp2(torch.randint(-60, 60, (33, 17, 3, 3), generator=g).float())
    for tf in (False, True):
        p = pack_emulation(w, tf)
        want = w.transpose(0, 1).flip(2, 3) if tf else w
        assert p[0].shape == want.shape
        assert torch.equal((p[2] + p[1]) + p[0], want)  # bit for bit, smallest first
        assert torch.equal(p[0].double() + p[1].double() + p[2].double(), want.double())
        for q in p:  # each plane IS a bf16 number
            assert torch.equal(q.bfloat16().float(), q)
    # the data gradient is the same convolution on the transposed, flipped weights
    x = torch.randn(2, 33, 6, 7, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(2, 33, 6, 7, generator=g, dtype=torch.float64)
    w64 = torch.randn(33, 33, 3, 3, generator=g, dtype=torch.float64)
    dx, = torch.autograd.grad(torch.nn.functional.conv2d(x, w64, None, 1, 1), x, gy)
    assert torch.allclose(dx, torch.nn.functional.conv2d(gy, w64.transpose(0, 1).flip(2, 3), None, 1, 1), rtol=1e-12, atol=1e-12)


def test_six_products_match_float64_like_plain_fp32():
    """A 597 x 9-term dot product per row, operands of mean 3 and std 1: e = |err| / sum |a b| against float64 for the six-product
    sum (each plane product exact in fp32, the small ones first, a fresh accumulator per 32 channels) and for plain fp32."""
    g = torch.Generator().manual_seed(1)
    rows, n = 512, 597 * 9
    a, b = 3.0 + torch.randn(rows, n, generator=g), 3.0 + torch.randn(rows, n, generator=g)
    ref = (a.double() * b.double()).sum(1)
    S = (a.double() * b.double()).abs().sum(1)
    pa, pb = split3(a), split3(b)
    order = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))

    def chain(pairs):
        """The kernel's order: per block of 18 steps (32 channels x 9 taps, 16 terms per MFMA, one rounding each) a fresh
        accumulator takes the small products of every step first, then the (0, 0) products; the blocks are added up."""
        tot, steps = torch.zeros(rows), list(range(0, n, 16))
        for b0 in range(0, len(steps), 18):
            acc = torch.zeros(rows)
            for part in (pairs[:-1], pairs[-1:]):
                for k0 in steps[b0:b0 + 18]:
                    for i, j in part:
                        prod = pa[i][:, k0:k0 + 16].double() * pb[j][:, k0:k0 + 16].double()  # exact: 8 x 8 significand bits
                        assert torch.equal(prod.float().double(), prod)
                        acc = (acc.double() + prod.sum(1)).float()
            tot = tot + acc
        return tot
    e = lambda got: float(((got.double() - ref).abs() / S).max()) / U
    plain = torch.zeros(rows)
    for k0 in range(0, n, 16):
        plain = plain + (a[:, k0:k0 + 16] * b[:, k0:k0 + 16]).sum(1)
    e6, e32 = e(chain(order)), e(plain)
    print('six products %.2f u, plain fp32 %.2f u' % (e6, e32))
    assert e6 <= 2.0 * e32  # the criterion of the GPU test
    # per product: the three dropped terms are below 2.01 * 2^-24 of it; the next three cannot go as well (2^-16 of it)
    exact = a.double() * b.double()
    rel = lambda pairs: float(((sum(pa[i].double() * pb[j].double() for i, j in pairs) - exact).abs() / exact.abs()).max())
    assert rel(order) <= 2.01 * U
    assert rel(order[3:]) > 2.0 ** -18
