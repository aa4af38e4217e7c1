"""GPU: the fused warp + mask + L1/SSIM pass (AF.photo_warp_sums, csrc/photo_warp.hip) and the area pyramid against the CPU
oracle, its reproducibility, and the number of C-ABI calls the two pyramid losses issue on top of it.

Tolerances are the project's own for the same quantities: the three sums as tests/test_bench_shapes_gpu.py::
test_photometric_sums_at_bench_shapes (5e-5 / 1e-6, 1e-4 / 5e-6, mask sum 0 / 1e-7), the flow gradient as
test_unflow_loss_end_to_end_at_bench_resolution (atol 2e-7 + 2e-4 max|g|, rtol 2e-3).  The area pyramid is held to the
bound of ANY fp32 summation order: n u mean|x| of the block with n = block size + 1, u = 2^-24 (the rule of
tests/test_headconv_gpu.py).  Every case asserts from the recorded call names that the fused entry points ran."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests.conftest import ROOT, assert_close

pytestmark = pytest.mark.gpu

BENCH_SCALES = [(384, 640), (96, 160), (48, 80), (24, 40), (12, 20)]  # pwclite+unflow_loss at 384x640, non-zero weights
# shapes that miss every tile edge of the 16 x 64 tiling: smallest legal, odd, widths not divisible by 4, one tile
# column with several tile rows, one tile row with several tile columns, one pixel past a tile in both directions
EDGE_SHAPES = [(3, 3), (5, 7), (13, 21), (33, 130), (40, 50), (40, 64), (16, 200), (17, 65)]


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    return functional


@pytest.fixture(scope='module')
def O():
    from oracle import ops
    torch.set_num_threads(16)
    return ops


def _frames(B, frames, H, W, gen):
    """U[0,1) images smoothed by a 5x5 box blur where the size allows it (structure for SSIM)."""
    x = torch.rand(B, 3 * frames, H, W, generator=gen)
    if min(H, W) >= 5:
        x = F.avg_pool2d(F.pad(x, (2, 2, 2, 2), mode='reflect'), 5, 1)
    return x.contiguous()


def _flow(B, C, h, w, gen):
    """A smooth field of about a third of the image extent plus pixel noise: a good share of the samples leave the image."""
    coarse = 0.35 * min(h, w) * torch.randn(B, C, 3, 3, generator=gen)
    return (F.interpolate(coarse, (h, w), mode='bilinear', align_corners=True) + 0.3 * torch.randn(B, C, h, w, generator=gen)).contiguous()


def _share_outside(flow2, h, w):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    cx, cy = xs + flow2[:, 0], ys + flow2[:, 1]
    return float(((cx < 0) | (cx > w - 1) | (cy < 0) | (cy > h - 1)).float().mean())


def _ran(AF, rec):
    return sorted({name for name, _ in rec})


def _case(AF, O, B, h, w, pad, mask_mode, addressing, seed, check=True):
    """One forward + backward of the op next to the oracle composition.  addressing 'flow4': the unFlowLoss pattern (two
    images of one [B,6,h,w] tensor, each the other's source; flow = channels 0:2 / 2:4 of one [B,4,h,w] tensor; mask given
    as 1 - plane); 'shared': the MvLoss pattern (one target for both groups, frames 0 / 2 of a [B,9,h,w] tensor as sources,
    two separate flow tensors)."""
    gen = torch.Generator().manual_seed(seed)
    k = 4 if h <= 96 else 2  # factor of the fine plane in 'nearest' mode
    if addressing == 'flow4':
        im = _frames(B, 2, h, w, gen)
        flow = _flow(B, 4, h, w, gen)
        tgt, src = (im[:, :3], im[:, 3:]), (im[:, 3:], im[:, :3])
        fl = (flow[:, :2], flow[:, 2:])
        invert = True
    else:
        im = _frames(B, 3, h, w, gen)
        fa, fb = _flow(B, 2, h, w, gen), _flow(B, 2, h, w, gen)
        tgt, src = (im[:, 3:6], im[:, 3:6]), (im[:, 0:3], im[:, 6:9])
        fl = (fa, fb)
        invert = False
    mh, mw = (h * k, w * k) if mask_mode == 'nearest' else (h, w)
    plane = None if mask_mode == 'border' else (torch.rand(2 * B, 1, mh, mw, generator=gen) > 0.25).float()
    if min(h, w) >= 12:
        assert _share_outside(torch.cat(fl, 0), h, w) > 0.05, 'the case is meant to push samples out of the image'

    # oracle, fp32 on the CPU
    fr = [f.clone().requires_grad_(True) for f in fl]
    ref, masks, kinks, obj = [], [], [], 0.
    for g in range(2):
        if mask_mode == 'border':
            m = O.border_mask(fr[g].detach())
        else:
            m = plane[g * B:(g + 1) * B]
            if mask_mode == 'nearest':
                m = F.interpolate(m, (h, w), mode='nearest')
        m = 1 - m if invert else m  # (the flag applies to every mode)
        rec = O.flow_warp(src[g], fr[g], pad=pad)
        l1 = ((tgt[g] - rec).abs() * m).sum()
        ss = O.ssim(rec * m, tgt[g] * m).sum()
        ref.append((l1, ss, m.sum()))
        masks.append(m)
        # |tgt - rec| has no derivative at 0.  `rec` is a sum of four fp32 products of values below 1, so two correct
        # evaluations differ by up to ~4 u = 2.4e-7 and may land on opposite sides of the kink (at 384x640 a handful of the
        # 3 M pixel-channels do); the flow gradient is compared everywhere else.
        kinks.append((((tgt[g] - rec.detach()).abs() < 1e-6).any(1, keepdim=True) & (m > 0)).expand(-1, 2, -1, -1))
        obj = obj + (1 + g) * (0.3 * l1 + 0.7 * ss)
    rg = torch.autograd.grad(obj, fr)

    # the op: everything addressed in place inside the uploaded tensors
    imc = im.cuda()
    if addressing == 'flow4':
        flc = flow.cuda().requires_grad_(True)
        tg, sr, leaves = (imc[:, :3], imc[:, 3:]), (imc[:, 3:], imc[:, :3]), [flc]
        arg = flc
    else:
        fac, fbc = fa.cuda().requires_grad_(True), fb.cuda().requires_grad_(True)
        tg, sr, leaves = (imc[:, 3:6], imc[:, 3:6]), (imc[:, 0:3], imc[:, 6:9]), [fac, fbc]
        arg = (fac, fbc)
    mk = None
    if plane is not None:
        pc = plane.cuda()
        mk = (pc[:B], pc[B:])
    AF.start_kernel_timing()
    sums, mout = AF.photo_warp_sums(tg, sr, arg, mk, pad=pad, mask_mode=mask_mode, mask_invert=invert, want_mask=True)
    got = torch.autograd.grad((0.3 * sums[0, 0] + 0.7 * sums[0, 1]) + 2 * (0.3 * sums[1, 0] + 0.7 * sums[1, 1]), leaves)
    ran = _ran(AF, AF.stop_kernel_timing())
    assert ran == ['arflow_photo_warp_bwd', 'arflow_photo_warp_fwd'], 'not the fused entry points: %s' % ran
    gg = (got[0][:, :2], got[0][:, 2:]) if addressing == 'flow4' else got
    if check:
        assert torch.equal(mout.cpu(), torch.cat(masks, 0)), 'mask plane used'
        for g in range(2):
            assert_close(sums[g, 0], ref[g][0], 5e-5, 1e-6, 'group %d sum |tgt - rec| mask' % g)
            assert_close(sums[g, 1], ref[g][1], 0.0001, 5e-6, 'group %d sum SSIM distance' % g)
            assert_close(sums[g, 2], ref[g][2], 0, 1e-7, 'group %d sum mask' % g)
            # (difference of two blurred U[0,1) images: density ~5 at 0, so ~3e-5 of the pixels have a channel inside 1e-6)
            assert int(kinks[g][:, 0].sum()) <= 5 + 2e-4 * kinks[g][:, 0].numel() and bool(torch.isfinite(gg[g]).all())
            assert_close(torch.where(kinks[g], rg[g], gg[g].cpu()), rg[g], 2e-7 + 2e-4 * float(rg[g].abs().max()), 2e-3,
                         'group %d d / d flow' % g)
    return sums, gg


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize('addressing', ['flow4', 'shared'])
@pytest.mark.parametrize('mask_mode', ['plane', 'nearest', 'border'])
@pytest.mark.parametrize('pad', ['zeros', 'border'])
@pytest.mark.parametrize('size', EDGE_SHAPES, ids=_id)
def test_photo_warp_sums_at_tile_edges(AF, O, size, pad, mask_mode, addressing):
    h, w = size
    _case(AF, O, 3, h, w, pad, mask_mode, addressing, seed=h * 131 + w)


@pytest.mark.parametrize('addressing', ['flow4', 'shared'])
@pytest.mark.parametrize('mask_mode', ['plane', 'nearest', 'border'])
@pytest.mark.parametrize('pad', ['zeros', 'border'])
@pytest.mark.parametrize('size', BENCH_SCALES, ids=_id)
def test_photo_warp_sums_at_bench_scales(AF, O, size, pad, mask_mode, addressing):
    """The five scales of pwclite+unflow_loss at 384x640 (batch 8 at the coarse scales; 4 at full resolution, where the
    oracle's autograd pass over 2 x 4 x 3 x 384 x 640 is the cost of the case)."""
    h, w = size
    _case(AF, O, 4 if h == 384 else 8, h, w, pad, mask_mode, addressing, seed=h + w)


@pytest.mark.parametrize('addressing', ['flow4', 'shared'])
def test_photo_warp_sums_are_bitwise_reproducible(AF, O, addressing):
    a = _case(AF, O, 8, 96, 160, 'border', 'plane', addressing, seed=7, check=False)
    b = _case(AF, O, 8, 96, 160, 'border', 'plane', addressing, seed=7, check=False)
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)


def _area_bound_check(AF, frames, sizes):
    H, W = frames.shape[-2:]
    AF.start_kernel_timing()
    got = AF.area_pyramid(frames.cuda(), sizes)
    ran = _ran(AF, AF.stop_kernel_timing())
    assert ran == ['arflow_area_pyramid'], ran
    u = 2.0 ** -24
    for (h, w), g in zip(sizes, got):
        ref = F.interpolate(frames.double(), (h, w), mode='area')
        mean_abs = F.interpolate(frames.double().abs(), (h, w), mode='area')
        n = (H // h) * (W // w) + 1
        err = (g.cpu().double() - ref).abs()
        print('area factor %d: max err / bound = %.3f' % (H // h, float((err / (n * u * mean_abs)).max())))
        assert g.shape == ref.shape
        assert bool((err <= n * u * mean_abs).all()), 'factor %d: worst %.3e' % (H // h, float(err.max()))


def test_area_pyramid_against_float64(AF):
    gen = torch.Generator().manual_seed(11)
    frames = _frames(2, 2, 384, 640, gen)
    _area_bound_check(AF, frames, [(384 // f, 640 // f) for f in (4, 8, 16, 32, 64)])
    same = AF.area_pyramid(frames.cuda(), [(384, 640)])  # factor 1: the frames themselves, nothing launched
    assert same[0].shape == frames.shape and torch.equal(same[0].cpu(), frames)


def test_area_pyramid_other_integer_factors(AF):
    gen = torch.Generator().manual_seed(12)
    _area_bound_check(AF, _frames(2, 3, 30, 45, gen) - 0.5, [(10, 15), (6, 9), (15, 45), (1, 1)])


# ---- launch counts ----------------------------------------------------------------------------------------------------
_COUNT_CHILD = r'''
import json, sys, torch
sys.path.insert(0, %r)
from arflow_amd import functional as AF
from arflow_amd.config import AttrDict
from arflow_amd.losses import get_loss
from arflow_amd.train_step import WORKLOADS
out = {}
for wl in ('pwclite+unflow_loss', 'pwclite3+mv_loss'):
    cfg = AttrDict(WORKLOADS[wl][1])
    B, H, W = 8, 384, 640
    gen = torch.Generator().manual_seed(3)
    sizes = ([(H, W)] + [(H // s, W // s) for s in (4, 8, 16, 32, 64)])[:len(cfg.w_scales)]
    loss = get_loss(cfg)
    if cfg.type == 'mv':
        img = torch.rand(B, 9, H, W, generator=gen).cuda()
        f12 = [(0.02 * h * torch.randn(B, 2, h, w, generator=gen)).cuda().requires_grad_(True) for h, w in sizes]
        f10 = [(0.02 * h * torch.randn(B, 2, h, w, generator=gen)).cuda().requires_grad_(True) for h, w in sizes]
        args, leaves = (f12, f10, img), f12 + f10
    else:
        img = torch.rand(B, 6, H, W, generator=gen).cuda()
        fl = [(0.02 * h * torch.randn(B, 4, h, w, generator=gen)).cuda().requires_grad_(True) for h, w in sizes]
        args, leaves = (fl, img), fl
    for _ in range(2):  # the second pass is the one counted
        AF.start_kernel_timing()
        res = loss(*args)
        res[0].backward()
        rec = AF.stop_kernel_timing()
    names = {}
    for (name, key), v in rec.items():
        names[name] = names.get(name, 0) + len(v)
    out[wl] = names
print('COUNTS ' + json.dumps(out))
'''


def _counts(fused):
    env = dict(os.environ, ARFLOW_PHOTO_WARP='1' if fused else '0')
    r = subprocess.run([sys.executable, '-c', _COUNT_CHILD % ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('COUNTS ')][-1]
    return json.loads(line[len('COUNTS '):])


def test_loss_launch_counts():
    """C-ABI calls of one forward + backward of each pyramid loss at its train_step.WORKLOADS configuration (8 x 384x640,
    flows of the model's shapes).  With S scales of non-zero w_scales and S_sm of non-zero w_sm_scales:
      unFlowLoss  1 (area pyramid) + 1 (occlusion map) + 2 S + 2 S_sm = 14   (S = 5, S_sm = 1)
      MvLoss      1 (area pyramid)                     + 2 S + 2 S_sm = 11   (S = 4, S_sm = 1)
    The composed path (ARFLOW_PHOTO_WARP=0, a child process of its own) is counted the same way and printed: 41 and 30 (measured on MI355X)."""
    fused, composed = _counts(True), _counts(False)
    print('fused', json.dumps(fused, sort_keys=True))
    print('composed', json.dumps(composed, sort_keys=True))
    for wl, most in (('pwclite+unflow_loss', 14), ('pwclite3+mv_loss', 11)):
        n, n0 = sum(fused[wl].values()), sum(composed[wl].values())
        print('%s: %d C-ABI calls fused, %d composed' % (wl, n, n0))
        assert n <= most, (wl, fused[wl])
        assert fused[wl].get('arflow_photo_warp_fwd', 0) >= 4 and fused[wl].get('arflow_photo_warp_bwd', 0) >= 4, fused[wl]
        assert 'arflow_photo_fwd' not in fused[wl] and 'arflow_warp_fwd' not in fused[wl], fused[wl]
        assert 'arflow_photo_warp_fwd' not in composed[wl] and n0 > n, composed[wl]
