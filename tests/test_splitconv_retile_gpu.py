"""The 4 x 1 wave tile of the KT = 2 launches of the split-bf16 convolution kernel.  A workgroup still
owns 8 pixel tiles x 2 channel tiles, but a wave now holds ONE channel tile (waves 0, 1 the first, waves 2, 3 the second) and
FOUR pixel tiles (waves 0, 2 the workgroup's tiles 0..3, waves 1, 3 tiles 4..7).  Only which wave holds which accumulator
changed: no product, no accumulator chain, no summation order.  So

1. indexing is exact, without any golden: a one-hot weight at output channel k in {0, 31, 32, 63} (first and last of either
   channel tile) and full-mantissa inputs give the shifted input plane bit for bit in channel k and exact zeros in every other
   channel, at all nine taps, through the raw forward call and through the transpose_flip call -- at shapes (N, C, K, H, W)
   1x33x64x8x32 (one workgroup: every wave's four pixel tiles and both channel tiles are live, no edge) and 3x64x64x16x64
   (N > 1, 2 x 2 workgroups per sample).  A wave that stored to, or read its pixels from, another wave's tiles cannot pass.
2. every output keeps the bits of the build before the change: tests/golden/splitconv_retile_bits.txt holds the fingerprints
   `tools/splitconv_bits.py --cases retile` printed on that build (K in {40, 65, 160}, C in {64, 70}, N = 2, maps 8x32, 4x33
   and 9x13; y, dx and the in-place slot with and without bias); the list is recomputed and compared, every case runs twice.
"""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'splitconv_retile_bits.txt')


def _tool():
    spec = importlib.util.spec_from_file_location('splitconv_bits', os.path.join(ROOT, 'tools', 'splitconv_bits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


B = _tool()


@pytest.fixture(scope='module')
def run():
    return B.Runner(ROOT)


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        lines = [ln.rstrip('\n') for ln in f if ln.strip()]
    return {ln.split('  ')[0]: ln for ln in lines}


def full_mantissa(*shape, seed):
    """Floats of either sign with all 24 significand bits random, over 14 binades."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(0, 1 << 23, shape, generator=g) + (1 << 23)
    expo = torch.randint(-30, -16, shape, generator=g)
    sign = 1.0 - 2.0 * torch.randint(0, 2, shape, generator=g)
    return sign * torch.ldexp(bits.float(), expo)


def shifted(plane, dr, ds):
    """out[..., h, w] = plane[..., h + dr, w + ds], zero outside."""
    H, W = plane.shape[-2:]
    return F.pad(plane, (1, 1, 1, 1))[..., 1 + dr:1 + dr + H, 1 + ds:1 + ds + W]


ONE_HOT_SHAPES = [(1, 33, 64, 8, 32), (3, 64, 64, 16, 64)]
EDGES = (0, 31, 32, 63)  # first and last channel of either tile of a KT = 2 workgroup


def test_one_hot_shapes_fill_every_tile_of_a_workgroup():
    for N, C, K, H, W in ONE_HOT_SHAPES:
        assert B.pixel_tile(H, W) == 32 and H % 8 == 0 and W % 32 == 0 and K == 64


@pytest.mark.parametrize('shape', ONE_HOT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_one_hot_weight_copies_the_shifted_plane_bit_for_bit(run, shape):
    N, C, K, H, W = shape
    x = full_mantissa(N, C, H, W, seed=11).cuda()
    for k in EDGES:
        for tap in range(9):
            r, s = divmod(tap, 3)
            c = (5 * tap + k) % C
            # forward: y[:, k] = x[:, c] shifted by the tap
            w = torch.zeros(K, C, 3, 3, device='cuda')
            w[k, c, r, s] = 1.0
            y = run.fwd(x, w, 0, torch.full((N, K, H, W), 7.0, device='cuda'))
            want = torch.zeros_like(y)
            want[:, k] = shifted(x[:, c], r - 1, s - 1)
            assert torch.equal(y, want), ('fwd', k, c, r, s)
            # transpose_flip: weights [C, K, 3, 3], taps flipped -- a data gradient's orientation
            wt = torch.zeros(C, K, 3, 3, device='cuda')
            wt[c, k, r, s] = 1.0
            y = run.fwd(x, wt, 1, torch.full((N, K, H, W), 7.0, device='cuda'))
            want = torch.zeros_like(y)
            want[:, k] = shifted(x[:, c], 1 - r, 1 - s)
            assert torch.equal(y, want), ('transpose_flip', k, c, r, s)


def test_retile_maps_take_the_32_and_the_16_wide_pixel_tile():
    assert [B.pixel_tile(H, W) for H, W in B.RETILE_MAPS] == [32, 32, 16]


def test_golden_file_holds_every_case(golden):
    heads = [B.fwd_head(C, K, H, W) for H, W in B.RETILE_MAPS for C in B.RETILE_CS for K in B.RETILE_KS]
    assert sorted(golden) == sorted(heads)


@pytest.mark.parametrize('hw', B.RETILE_MAPS, ids=lambda m: '%dx%d' % m)
def test_bits_match_the_build_before_the_retile_and_repeat(run, golden, hw):
    H, W = hw
    for C in B.RETILE_CS:
        for K in B.RETILE_KS:
            first, second = B.fwd_case(run, C, K, H, W), B.fwd_case(run, C, K, H, W)
            assert first == second, 'two calls differ at C=%d K=%d %dx%d' % (C, K, H, W)
            head = B.fwd_head(C, K, H, W)
            assert B.fmt(head, first) == golden[head]
