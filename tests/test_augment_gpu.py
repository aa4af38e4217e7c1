"""GPU: the batch augmentation kernels (csrc/augment.hip; arflow_amd.augment) per output value against the float64 restatement
of tests/augment_ref.py, and TrainStep's img_pair_ph.  DESIGN.md section 36.

The bound of every output value is derived by tests/augment_ref.py from the inputs alone (every fp32 operation of the kernel
carried as value and absolute error bound, u = 2^-24) and may not exceed 1e-5 (BOUND_CAP) anywhere -- a wrong hue sector or
branch shows as >= 1e-2.  Where nothing is resized img is src / 255 at the mapped pixel BIT FOR BIT.  Each test prints its
largest error / bound ratio.
Shapes: 13 x 22 -> crop 7 x 10 (w % 4 != 0: scalar stores, a ragged last quad), crop 8 x 12 (float4 stores), 40 x 70 (two partial
sums per frame), resizes 13 x 22 -> 16 x 24, -> 9 x 10, 16 x 24 -> 16 x 24 (identity) and crop 7 x 10 -> 16 x 24, F = 1, 2, 3."""
import pytest
import torch

from arflow_amd import augment as A
from tests import augment_ref as R

pytestmark = pytest.mark.gpu
_cache = {}


def reference(key, make):
    """Inputs and float64 references of one case, computed once and left unchanged."""
    if key not in _cache:
        src, p = make()
        img, ph, e, eph = R.augment(src, p, track=True)
        assert float(eph.max()) <= R.BOUND_CAP and float(e.max()) <= R.BOUND_CAP
        _cache[key] = dict(src=src, p=p, img=img, ph=ph, e=e, eph=eph, img32=R.augment(src, p, dtype=torch.float32)[0])
    return _cache[key]


def excess(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
    print('%s: max err %.3e, max bound %.3e, max err / bound %.3f' % (name, float(err.max()), float(bound.max()), ratio))
    return int((err > bound).sum())


def check(name, c, exact_img, src=None):
    img, ph = A.augment_batch(c['src'].cuda() if src is None else src, c['p'])
    assert img.dtype == ph.dtype == torch.float32 and img.shape == ph.shape == c['img'].shape and ph is not img
    assert img.is_contiguous() and ph.is_contiguous()
    if exact_img:
        assert torch.equal(img.cpu(), c['img32']), name + ': img is not src / 255 bit for bit'
    assert excess(name + ' img', img, c['img'], c['e']) == 0
    assert excess(name + ' img_ph', ph, c['ph'], c['eph']) == 0
    return img, ph


@pytest.mark.parametrize('crop', [(7, 10), (8, 12)], ids=['7x10-scalar', '8x12-float4'])
def test_operation_orders(crop):
    """All 4! orders, one per sample, mixed flips, crop origins at 0, the far corner and odd x1, colours planted in every hue
    sector, on the sector boundaries, grey, black and white; then the same geometry with img_ph = NULL."""
    c = reference(('orders', crop), lambda: R.orders_case(crop))
    img, ph = check('orders %dx%d' % crop, c, True)
    assert float((ph - img).abs().max()) > 0.05
    p = c['p']
    geo = A.AugmentParams(p.table, p.src_hw, p.crop_hw, None, False)
    only, same = A.augment_batch(c['src'].cuda(), geo)
    assert same is only and torch.equal(only, img)


def test_partial_sums_of_the_contrast_mean():
    """40 x 70 frames: two partials per frame.  The mean the apply kernel forms (partials in index order, / (h w)) against the
    float64 mean of the fp32 greys' references; the outputs within their bounds; two calls, and a call in deterministic mode,
    bitwise equal."""
    from arflow_amd import _lib, functional as AF
    c = reference('contrast', R.contrast_case)
    src, p = c['src'].cuda(), c['p']
    img, ph = check('contrast 40x70', c, True, src)
    again = A.augment_batch(src, p)[1]
    with AF.deterministic():
        det = A.augment_batch(src, p)[1]
    assert torch.equal(ph, again) and torch.equal(ph, det)
    B, F, (h, w) = p.B, 2, p.out_hw
    parts = _lib.load().arflow_augment_partials(h, w)
    assert parts == 2
    work = torch.full((B * F, parts), float('nan'), device='cuda', dtype=torch.float64)
    AF._call('arflow_augment_stats', src.data_ptr(), 0, p.device_table(src.device).data_ptr(), work.data_ptr(), B, F, h, w, h, w,
             h, w, 0, AF._stream())
    mean = (work[:, 0] + work[:, 1]).cpu().reshape(B, F) / (h * w)
    gray = R.gray(R.geometric(c['src'], p, track=True))
    for b in (0, 3):  # contrast first in the order / contrast alone: the frame in front of contrast is the geometric image
        want, bound = gray.v[b].mean((-1, -2)), gray.e[b].mean((-1, -2)) + 1e-12
        assert ((mean[b] - want).abs() <= bound).all(), (b, mean[b], want, bound)


@pytest.mark.parametrize('shape', [((13, 22), (13, 22), (16, 24)), ((13, 22), (13, 22), (9, 10)), ((16, 24), (16, 24), (16, 24)),
                                   ((13, 22), (7, 10), (16, 24))], ids=['up', 'down', 'identity', 'crop-up'])
def test_scale(shape):
    """Bilinear, align_corners=False, of the cropped and flipped image (half of the samples are flipped), up, down, and the
    identity, which is bitwise."""
    c = reference(('scale', shape), lambda: R.scale_case(*shape))
    assert c['p'].flip.any() and not c['p'].flip.all()
    img, ph = check('scale %s' % (shape,), c, shape[1] == shape[2])
    assert tuple(img.shape[-2:]) == shape[2]
    img2, ph2 = A.augment_batch(c['src'].cuda(), A.AugmentParams(c['p'].table, shape[0], shape[1], None, True), out_hw=shape[2])
    assert torch.equal(img2, img) and torch.equal(ph2, ph)      # out_hw asks for the same resize


@pytest.mark.parametrize('F', [1, 3])
def test_frame_counts_and_input_types(F):
    """F = 1 and F = 3 (every frame of a sample under the sample's row), gamma over its whole range and all six channel
    permutations; a float32 source gives the bits of the uint8 source divided by 255; the [B,3F,H,W] view is the same batch."""
    c = reference(('frames', F), lambda: R.frames_case(F))
    img, ph = check('frames F=%d' % F, c, True)
    assert img.shape[1] == 3 * F
    as_float = c['src'].float() / 255
    img_f, ph_f = A.augment_batch(as_float.cuda(), c['p'])
    assert torch.equal(img_f, img) and torch.equal(ph_f, ph)
    img_v, ph_v = A.augment_batch(c['src'].reshape(6, 3 * F, 13, 22).cuda(), c['p'])
    assert torch.equal(img_v, img) and torch.equal(ph_v, ph)


def test_batch_augment_draws_and_applies():
    geo = dict(crop=True, crop_size=[8, 12], hflip=True)
    pho = dict(hue=0.5, swap_channels=True)
    src = R.orders_case((8, 12))[0].cuda()
    a, b = A.BatchAugment(geo, pho, seed=3), A.BatchAugment(geo, pho, seed=3)
    img, ph = a(src)
    img_b, ph_b = b(src)
    assert torch.equal(img, img_b) and torch.equal(ph, ph_b) and torch.equal(a.last_params.table, b.last_params.table)
    ref_img, ref_ph, e, eph = R.augment(src.cpu(), a.last_params, track=True)
    assert excess('BatchAugment img', img, ref_img, e) == 0 and excess('BatchAugment img_ph', ph, ref_ph, eph) == 0
    img2, _ = a(src)                                            # the generator moves on
    assert not torch.equal(a.last_params.table, b.last_params.table) and img2.shape == img.shape
    none = A.BatchAugment()
    x, y = none(src)
    assert x is y and torch.equal(x.cpu(), (src.cpu().float() / 255).reshape(24, 6, 13, 22))  # the CPU's division is IEEE
    val = A.valid_transform((16, 24))(src)
    whole = R.geometric(src.cpu(), A.make_params((13, 22), (13, 22), [0] * 24, [0] * 24), (16, 24), track=True)
    assert excess('valid_transform', val, whole.v.reshape(24, 6, 16, 24), whole.e.reshape(24, 6, 16, 24)) == 0
    with pytest.raises(ValueError, match='leaves the source'):
        A.augment_batch(src, A.make_params((13, 22), (8, 12), [6] * 24, [0] * 24))
    with pytest.raises(ValueError, match='drawn for'):
        A.augment_batch(src[:3], a.last_params)


def test_train_step_feeds_the_model_the_photometric_pair():
    """img_pair_ph = img_pair is the default step bit for bit; another img_pair_ph changes the loss (the model saw it) while
    the loss still reads img_pair."""
    from arflow_amd import functional as AF
    from arflow_amd.train_step import TrainStep, synthetic_pairs
    dev = torch.device('cuda')
    x = synthetic_pairs(2, 64, 64, device=dev, seed=5)
    other = x.flip(1).contiguous()
    losses = []
    with AF.deterministic():
        for kw in (dict(img_pair_ph=x), dict(), dict(img_pair_ph=other)):
            step = TrainStep('pwclite_uflow+uflow_loss', dev, seed=11)
            step.model.level_dropout = 0.0
            losses.append(step(x, **kw))
    assert all(bool(torch.isfinite(l)) for l in losses), losses
    assert torch.equal(losses[0], losses[1]), (float(losses[0]), float(losses[1]))
    assert not torch.equal(losses[0], losses[2])
    with pytest.raises(ValueError, match='img_pair_ph'):
        step(x, img_pair_ph=x[:, :, :32])
