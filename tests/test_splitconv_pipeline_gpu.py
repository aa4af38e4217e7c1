"""The operand pipeline of the split-bf16 convolution kernels changes WHEN fragments are requested
and how long the kernel waits for them, never which products are formed or in what order.  So every output must keep the
bits it had before the pipeline: tests/golden/splitconv_bits.txt holds the fingerprints tools/splitconv_bits.py printed on the
build without it.

1. golden bits: the tool's cases are recomputed and compared line by line; a wrong wait count shows as another hash;
2. two calls are bitwise equal: every case runs twice;
3. poisoned neighbours: the packed weights and, separately, x / dy and the weight gradient's workspace stand in the middle of
   a larger allocation filled once with zeros and once with NaN bit patterns; the outputs of the two runs must be equal.  A
   fragment fetched past its buffer that reaches an MFMA poisons the result.  (Reads whose result is dropped -- the prefetch
   behind the last unit, the clamped staging loads -- are not seen by this test; the clamps in the code keep their addresses
   inside the buffers by construction.)

The cases (see the tool) are the smallest that reach every edge of the pipeline; the maps 5x7, 6x20 and 3x40 all take the
32 x 1 pixel tile by the host's rule -- asserted below -- so 9x13 (16 x 2) and 17x7 (8 x 4) run as well.
"""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'splitconv_bits.txt')


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


def test_pixel_tiles_of_the_maps():
    assert [B.pixel_tile(H, W) for H, W in B.MAPS] == [32, 32, 32, 16, 8]


def test_golden_file_holds_every_case(golden):
    heads = [B.fwd_head(C, K, H, W) for H, W in B.MAPS for C in B.CS for K in B.KS] + [B.wgrad_head(*c) for c in B.WGRAD_CASES]
    assert sorted(golden) == sorted(heads)


@pytest.mark.parametrize('hw', B.MAPS, ids=lambda m: '%dx%d' % m)
def test_forward_bits_match_the_golden_file_and_repeat(run, golden, hw):
    H, W = hw
    for C in B.CS:
        for K in B.KS:
            first, second = B.fwd_case(run, C, K, H, W), B.fwd_case(run, C, K, H, W)
            assert first == second, 'two calls differ at C=%d K=%d %dx%d' % (C, K, H, W)
            head = B.fwd_head(C, K, H, W)
            assert B.fmt(head, first) == golden[head]


@pytest.mark.parametrize('case', B.WGRAD_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_weight_gradient_bits_match_the_golden_file_and_repeat(run, golden, case):
    first, second = B.wgrad_case(run, *case), B.wgrad_case(run, *case)
    assert first == second
    head = B.wgrad_head(*case)
    assert B.fmt(head, first) == golden[head]


FILLS = (0, B.NAN_BITS)


@pytest.mark.parametrize('hw', B.MAPS, ids=lambda m: '%dx%d' % m)
@pytest.mark.parametrize('what', ['packed', 'x'])
def test_forward_ignores_what_surrounds_its_buffers(run, what, hw):
    H, W = hw
    for C in B.CS:
        for K in B.KS:
            x, w, wt, bias = B.fwd_inputs(C, K, H, W)
            for tf, wcpu in ((0, w), (1, wt)):
                got = []
                for fill in FILLS:
                    wd = wcpu.cuda()
                    if what == 'packed':
                        xd = x.cuda()
                        packed, _keep = B.embed(torch.zeros(run.pack_bytes(K, C), dtype=torch.uint8), fill, dtype=torch.uint8)
                    else:
                        xd, _keep = B.embed(x, fill)
                        packed = None
                    y = run.fwd(xd, wd, tf, torch.zeros(B.N_FWD, K, H, W, device='cuda'), packed=packed)
                    torch.cuda.synchronize()
                    got.append(y.cpu())
                assert torch.isfinite(got[1]).all(), 'NaN from outside %s reached the output (C=%d K=%d tf=%d)' % (what, C, K, tf)
                assert torch.equal(got[0], got[1]), '%s: C=%d K=%d tf=%d' % (what, C, K, tf)


@pytest.mark.parametrize('case', B.WGRAD_CASES, ids=lambda c: 'x'.join(map(str, c)))
@pytest.mark.parametrize('what', ['x', 'dy', 'ws'])
def test_weight_gradient_ignores_what_surrounds_its_buffers(run, what, case):
    N, C, K, H, W = case
    x, dy = B.wgrad_inputs(*case)
    got = []
    for fill in FILLS:
        xd, dyd, ws = x.cuda(), dy.cuda(), None
        if what == 'x':
            xd, _keep = B.embed(x, fill)
        elif what == 'dy':
            dyd, _keep = B.embed(dy, fill)
        else:
            ws, _keep = B.embed(torch.zeros(run.ws_bytes(*case), dtype=torch.uint8), fill, dtype=torch.uint8)
        dw = run.wgrad(xd, dyd, ws=ws)
        torch.cuda.synchronize()
        got.append(dw.cpu())
    assert torch.isfinite(got[1]).all()
    assert torch.equal(got[0], got[1])
