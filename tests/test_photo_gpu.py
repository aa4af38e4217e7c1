"""GPU: the photometric family against tests/photo_ref.py -- every output element inside its derived float64 bound.

  stand-alone kernels   arflow_photo_fwd / bwd (the 8 x 32 one-pixel and the 16 x 64 photo4 tiling of csrc/ssim.hip) through
                        AF.PhotoSumsFunction and loss_blocks.SSIM: the three sums, d / d rec under the weights (1, 0), (0, 1)
                        and a mix, the distance map and both map gradients under a random upstream map; noise, blurred,
                        near-equal and low-contrast images, binary / fractional masks and masks with whole windows zero,
                        C = 1, 2, 3, tile counts 1, 7, 9, 17 (padding workgroups) with the sums buffer's block poisoned first
  any-window kernels    arflow_ssim_fwd / bwd at md = 2, 3
  fused pass            AF.photo_warp_sums (csrc/photo_warp.hip): per-pixel forward through one-pixel mask probes, per-pixel
                        d / d flow, the mask planes exactly, over C, G, B, both addressings, the three mask modes with and
                        without inversion, nearest factors with fy != fx; bitwise equality of two identical calls

tests/test_photo_ref_cpu.py shows, for the same inputs, that the bounds hold the fp32 oracle with room and that every listed
mutation of the reference leaves them by 10x.  Every test asserts from the recorded C-ABI calls that its entry points ran;
calls the product does not key for timing are recorded under a key of the test's own.  The worst error / bound of every
site is printed (`MARGIN`), profiles/photo_margins.txt holds one run's figures.
"""
import functools

import pytest
import torch

from tests import photo_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    return functional


@pytest.fixture
def record(AF, monkeypatch):
    """run(fn) -> (fn(), sorted names of the C-ABI calls it made), from AF.start_kernel_timing()'s records"""
    orig = AF._call

    def call(name, *args, key=None):
        return orig(name, *args, key=('test',) if key is None else key)
    monkeypatch.setattr(AF, '_call', call)

    def run(fn):
        AF.start_kernel_timing()
        out = fn()
        return out, sorted({name for name, _ in AF.stop_kernel_timing()})
    return run


def _hold(site, got, ref, keep=None):
    """every element of `got` within its bound of the float64 value; prints the worst ratio"""
    err, bound = (got.detach().cpu().double() - ref.v).abs(), ref.e.expand_as(ref.v)
    assert bool(torch.isfinite(got).all()), site
    if keep is not None:
        err, bound = err[keep], bound[keep]
    w = R.worst(err, bound)
    print('MARGIN %-58s %.3f' % (site, w))
    assert w <= 1.0, '%s: error / bound = %.3f (worst error %.3e)' % (site, w, float(err.max()))
    return w


def _poison(AF, B, H, W):
    """a NaN-filled block of the sums buffer's size goes back to the caching allocator: rows the forward leaves undefined
    would now be NaN if the allocator hands the block out again (extra sensitivity; nothing relies on it)"""
    n = AF._lib.load().arflow_sums_rows(B, H, W) * AF.SUM_COLS
    t = torch.full((n,), float('nan'), device='cuda')
    del t


@functools.lru_cache(maxsize=None)
def _sums_case(c):
    im, rec, mask, up = R.sums_inputs(c)
    return im, rec, mask, up, {w: R.photo_sums_ref(im, rec, mask, w) for w in R.WEIGHTS}


@functools.lru_cache(maxsize=None)
def _map_case(c):
    im, rec, _, up = R.sums_inputs(c)
    return R.photo_sums_ref(im, rec, None, gmap=up), R.photo_sums_ref(rec, im, None, gmap=up)


def _tag(c):
    return '%s %dx%dx%dx%d %s/%s' % (R.kernel_of(c.W), c.B, c.C, c.H, c.W, c.cls, c.mask)


@pytest.mark.parametrize('c', R.SUMS_CASES, ids=str)
def test_photo_sums_and_gradient_per_element(AF, record, c):
    im, rec, mask, _, refs = _sums_case(c)
    rc = rec.cuda().requires_grad_(True)
    imc, mc = im.cuda(), None if mask is None else mask.cuda()

    def fn():
        _poison(AF, c.B, c.H, c.W)
        s = AF.PhotoSumsFunction.apply(imc, rc, mc)
        return s, [torch.autograd.grad(w[0] * s[0] + w[1] * s[1], [rc], retain_graph=True)[0] for w in R.WEIGHTS]
    (s, grads), ran = record(fn)
    assert ran == ['arflow_photo_bwd', 'arflow_photo_fwd'], ran
    ref = refs[R.WEIGHTS[0]]
    for k, what in enumerate(('sum |im - rec| m', 'sum dist', 'sum m')):
        _hold('%s: %s' % (_tag(c), what), s[k], ref.sums[k])
    for w, g in zip(R.WEIGHTS, grads):
        ref = refs[w]
        keep = ~ref.kink.expand_as(ref.grad.v)
        assert float((~keep).double().mean()) <= R.KINK_CAP
        _hold('%s: d / d rec, weights (%.1f, %.1f)' % (_tag(c), w[0], w[1]), g, ref.grad, keep)


@pytest.mark.parametrize('c', R.SUMS_CASES, ids=str)
def test_ssim_map_and_gradients_per_window(AF, record, c):
    from arflow_amd import loss_blocks as LB
    im, rec, _, up, _ = _sums_case(c)
    ra, rb = _map_case(c)
    a, b = rec.cuda().requires_grad_(True), im.cuda().requires_grad_(True)

    def fn():
        _poison(AF, c.B, c.H, c.W)
        y = LB.SSIM(a, b)
        return (y,) + torch.autograd.grad(y, [a, b], up.cuda())
    (y, ga, gb), ran = record(fn)
    assert ran == ['arflow_photo_bwd', 'arflow_photo_fwd'], ran
    tag = '%s %dx%dx%dx%d %s' % (R.kernel_of(c.W), c.B, c.C, c.H, c.W, c.cls)
    _hold(tag + ': map', y, ra.dist)
    for g, r, what in ((ga, ra, 'x'), (gb, rb, 'y')):
        keep = ~r.kink.expand_as(r.grad.v)
        assert float((~keep).double().mean()) <= R.KINK_CAP
        _hold(tag + ': map gradient d / d ' + what, g, r.grad, keep)


@pytest.mark.parametrize('cls', ['blur', 'noise'])
@pytest.mark.parametrize('case', R.ANY_CASES, ids=str)
def test_ssim_any_window_per_element(AF, record, case, cls):
    from arflow_amd import loss_blocks as LB
    md, B, C, H, W = case
    im, rec = R.images(cls, B, C, H, W)
    up = torch.randn(B, C, H - 2 * md, W - 2 * md, generator=R._gen(3, H, W))
    a, b = rec.cuda().requires_grad_(True), im.cuda().requires_grad_(True)

    def fn():
        y = LB.SSIM(a, b, md)
        return (y,) + torch.autograd.grad(y, [a, b], up.cuda())
    (y, ga, gb), ran = record(fn)
    assert md != 1 and ran == ['arflow_ssim_bwd', 'arflow_ssim_fwd'], ran
    tag = 'md=%d %dx%dx%dx%d %s' % (md, B, C, H, W, cls)
    _hold(tag + ': map', y, R.ssim_ref(rec, im, md).dist)
    refs = [R.ssim_any_grad_ref(rec, im, up, md), R.ssim_any_grad_ref(im, rec, up, md)]
    for g, (r, kink), what in ((ga, refs[0], 'x'), (gb, refs[1], 'y')):
        _hold(tag + ': map gradient d / d ' + what, g, r, ~kink.expand_as(r.v))


# ---- the fused pass -------------------------------------------------------------------------------------------------------
def _upload(c, i):
    """the case's tensors on the GPU, addressed as the losses address them -> (tgt, src, flow argument, flow leaves, mask)"""
    C, G, B = c.C, c.G, c.B
    if c.addr == 'flow4':   # unFlowLoss: two images of one tensor, each the other's source; the flows in one tensor
        im = torch.cat([i.tgt[0], i.src[0]], 1).cuda()
        tg, sr = (im[:, :C], im[:, C:])[:G], (im[:, C:], im[:, :C])[:G]
        fl = torch.cat(i.flow, 1).cuda().requires_grad_(True)
        arg, leaves = fl, [fl]
    else:                   # MvLoss: one target, frames 0 / 2 of one tensor as sources, two flow tensors
        im = torch.cat([i.src[0], i.tgt[0], i.src[1]], 1).cuda()
        tg, sr = (im[:, C:2 * C], im[:, C:2 * C]), (im[:, :C], im[:, 2 * C:])
        leaves = [f.cuda().requires_grad_(True) for f in i.flow]
        arg = tuple(leaves)
    mk = None
    if i.mask is not None:
        pc = torch.cat(i.mask, 0).cuda()
        mk = (pc[:B], pc[B:])[:G]
    return tg, sr, arg, leaves, mk


def _run_pw(AF, record, c):
    i = R.pw_inputs(c)
    tg, sr, arg, leaves, mk = _upload(c, i)

    def fn():
        sums, mout = AF.photo_warp_sums(tg, sr, arg, mk, pad=c.pad, mask_mode=c.mode, mask_invert=c.invert, want_mask=True)
        obj = sum(c.coef[g][0] * sums[g, 0] + c.coef[g][1] * sums[g, 1] for g in range(c.G))
        return sums, mout, torch.autograd.grad(obj, leaves)
    (sums, mout, got), ran = record(fn)
    assert ran == ['arflow_photo_warp_bwd', 'arflow_photo_warp_fwd'], ran
    gg = [got[0][:, 2 * g:2 * g + 2] for g in range(c.G)] if c.addr == 'flow4' else list(got)
    return sums, mout, gg


@functools.lru_cache(maxsize=None)
def _pw_ref(c):
    return R.pw_case_ref(c)


@pytest.mark.parametrize('c', R.PW_CASES, ids=lambda c: c.name)
def test_photo_warp_gradient_per_pixel(AF, record, c):
    ref = _pw_ref(c)
    sums, mout, gg = _run_pw(AF, record, c)
    assert torch.equal(mout.cpu(), ref.mask_out), 'the mask plane used'
    for g in range(c.G):
        for k, what in enumerate(('sum |tgt - rec| m', 'sum dist', 'sum m')):
            _hold('fused %s: group %d %s' % (c.name, g, what), sums[g, k], ref.sums[g][k])
        keep = ~ref.kink[g]
        assert float((~keep).double().mean()) <= R.KINK_CAP
        _hold('fused %s: group %d d / d flow' % (c.name, g), gg[g], R.Iv(ref.gflow[g], ref.bound_gflow[g]), keep)


@pytest.mark.parametrize('pad', ['zeros', 'border'])
@pytest.mark.parametrize('shape', R.PROBE_SHAPES, ids=str)
def test_photo_warp_forward_per_pixel_by_probes(AF, record, shape, pad):
    """a plane that is 1 at one pixel per group turns the three sums into that pixel's own terms"""
    H, W = shape
    c, i = R.probe_inputs(H, W, pad)
    rec = [R.probe_warp(i, g, pad) for g in range(2)]
    tg, sr, arg, _, _ = _upload(c, i)
    plane = torch.zeros(2, 1, H, W, device='cuda')
    worst = [0.0, 0.0]
    for (y, x) in R.probe_pixels(H, W):
        plane.zero_()
        plane[:, 0, y, x] = 1.0
        with torch.no_grad():
            sums, ran = record(lambda: AF.photo_warp_sums(tg, sr, arg, (plane[:1], plane[1:]), pad=pad, mask_mode='plane'))
        assert ran == ['arflow_photo_warp_fwd'], ran
        sums = sums.cpu().double()
        for g in range(2):
            ref = R.probe_ref(rec[g], i.tgt[g], y, x)
            assert float(sums[g, 2]) == 1.0, (y, x, g)
            for k in range(2):
                r = R.worst((sums[g, k] - ref[k].v).abs(), ref[k].e)
                worst[k] = max(worst[k], r)
                assert r <= 1.0, 'probe (%d, %d) group %d %s: error / bound = %.3f' % (y, x, g, ('L1', 'SSIM')[k], r)
    print('MARGIN %-58s %.3f' % ('fused probes %dx%d %s: pixel L1' % (H, W, pad), worst[0]))
    print('MARGIN %-58s %.3f' % ('fused probes %dx%d %s: pixel SSIM' % (H, W, pad), worst[1]))


@pytest.mark.parametrize('name', ['33x130 C3 G2 B1 rect', '16x64 C3 G2 B3 plane invert'])
def test_photo_warp_identical_calls_are_bit_equal(AF, record, name):
    c = [c for c in R.PW_CASES if c.name == name][0]
    assert R.n_tiles('pw', c.B * c.G, c.H, c.W) % 8 != 0, 'the case is meant to have padding workgroups'
    a, b = _run_pw(AF, record, c), _run_pw(AF, record, c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)
