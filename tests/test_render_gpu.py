"""GPU: the kernels of csrc/render.hip through arflow_amd.render, against the float64 restatement and the bounds of
tests/render_ref.py, the reference's own outputs (tests/golden/render.npz) and, where the arithmetic is the reference's fp32
sequence, the same expression composed of torch ops on the device (bitwise); then arflow_amd.predict.run, the CLI and the
unchanged arflow_amd.inference.infer on top of them.

restore shapes (tests/render_ref.py RESTORE_SHAPES): non-integer upscale (odd W: the float-by-float store), downscale,
identity, a one-pixel axis (both taps clamped onto it), an even W that is no multiple of 4 with a partial last workgroup (the
wide store and its guard), B = 3.  Every shape clamps on both edges (half-pixel centres reach below 0 and beyond n - 1).

Measured on an MI355X: restore error / bound at most 0.26 (flow) and 0.58 (entropy), 0.28 against the reference's golden
restore; mode 0, the statistics and the entropy picture bitwise; mode 1 at the 4 ulp atan2f allowance of render_ref: no
channel outside its range, 0.02 % .. 1.3 % of the channels inside a band, and of 53,274 channel values one differs from
floor(q) of the float64 restatement."""
import os

import numpy as np
import pytest
import torch

from tests import render_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'render.npz'), allow_pickle=False)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _inside(got, want, bound, what):
    err = np.abs(_np(got).astype(np.float64) - want)
    print('%s: max err %.3e, max err / bound %.3f' % (what, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound), what


# ---- restore -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', R.RESTORE_SHAPES)
@pytest.mark.parametrize('variant', ['full', 'slice', 'flow_only'])
def test_restore_against_the_restatement(shape, variant):
    from arflow_amd import render
    B, h, w, H, W = shape
    flow, ent = R.make_flow(R.SEED, B, h, w), R.make_entropy(R.SEED, B, h, w)
    ref = R.restore64(flow, (H, W), ent)
    if variant == 'slice':  # flows_fw[0][:, 0:2] and [:, 2:4] of a [B,4,h,w] tensor, read in place
        wide = _dev(np.concatenate([flow, ent], 1))
        r = render.restore(wide[:, 0:2], (H, W), wide[:, 2:4], stats=True)
    elif variant == 'full':
        r = render.restore(_dev(flow), (H, W), _dev(ent), stats=True)
    else:  # ent == NULL, stats == NULL
        r = render.restore(_dev(flow), (H, W))
        assert r.entropy is None and r.stats is None
    assert tuple(r.flow.shape) == (B, H, W, 2) and r.flow.is_contiguous()
    _inside(r.flow, ref['flow'], ref['flow_bound'], 'restore %s %s flow' % (shape, variant))
    if variant != 'flow_only':
        assert tuple(r.entropy.shape) == (B, H, W, 2)
        _inside(r.entropy, ref['ent'], ref['ent_bound'], 'restore %s %s entropy' % (shape, variant))
        # the statistics: bitwise torch.amax over the kernel's OWN output, and the same bits from a second call
        want = torch.stack([r.flow.abs().amax((1, 2, 3)), r.flow.amax((1, 2, 3))], 1)
        assert torch.equal(r.stats, want)
        again = render.restore(_dev(flow), (H, W), _dev(ent), stats=True)
        assert torch.equal(again.stats, r.stats) and torch.equal(again.flow, r.flow) and torch.equal(again.entropy, r.entropy)
        for layout, t in (('nhwc', r.flow), ('nchw', r.flow.permute(0, 3, 1, 2).contiguous())):
            assert torch.equal(render.flow_stats(t, layout), want), layout


@pytest.mark.parametrize('tag', ['up', 'down'])
def test_restore_against_the_reference(gold, tag):
    from arflow_amd import render
    B, h, w, H, W = (int(v) for v in gold['shape_' + tag])
    flow, ent = gold['flow_' + tag], gold['ent_' + tag]
    ref = R.restore64(flow, (H, W), ent)
    fb, eb = R.golden_extra_bound(flow, (H, W), ent)
    r = render.restore(_dev(flow), (H, W), _dev(ent))
    _inside(r.flow, gold['ref_flow_' + tag].astype(np.float64), ref['flow_bound'] + fb, 'golden %s flow' % tag)
    _inside(r.entropy, gold['ref_ent_' + tag].astype(np.float64), ref['ent_bound'] + eb, 'golden %s entropy' % tag)


def test_restore_detaches_and_refuses():
    from arflow_amd import render
    f = torch.zeros(1, 2, 4, 6, device=DEV, requires_grad=True)
    assert not render.restore(f, (8, 10)).flow.requires_grad
    with pytest.raises(ValueError):
        render.restore(f.double(), (8, 10))
    with pytest.raises(ValueError):
        render.restore(torch.zeros(1, 2, 6, 4, device=DEV).transpose(2, 3), (8, 10))
    with pytest.raises(ValueError):
        render.restore(f, (8, 10), torch.zeros(1, 2, 4, 5, device=DEV))


# ---- mode 0 --------------------------------------------------------------------------------------------------------------------------
def _rgb_torch(flow, scale):
    """np_flow2rgb composed of torch ops on the device: float [B,3,H,W] and its uint8 cast [B,H,W,3]"""
    n = flow / scale.view(-1, 1, 1, 1)
    c = torch.stack([1 + n[:, 0], 1 - 0.5 * (n[:, 0] + n[:, 1]), 1 + n[:, 1]], 1).clamp(0, 1)
    return c, (c * 255.0).permute(0, 2, 3, 1).to(torch.uint8)


@pytest.mark.parametrize('tag', ['s', 'm'])
def test_rgb_equals_the_reference_bitwise(gold, tag):
    from arflow_amd import render
    flow = _dev(gold['rflow_' + tag])
    assert np.array_equal(_np(render.torch_flow2rgb(flow)), gold['t2rgb_' + tag])           # the drop-in
    assert np.array_equal(_np(render.flow_rgb(flow, 'rgb')), gold['t2rgb_u8_' + tag])
    got = render.flow_rgb(flow, 'rgb', max_value=7.5, as_uint8=False)
    assert np.array_equal(_np(got).transpose(0, 2, 3, 1), gold['rgb_val_' + tag])
    nhwc = flow.permute(0, 2, 3, 1).contiguous()
    assert np.array_equal(_np(render.flow_rgb(nhwc, 'rgb', layout='nhwc')), gold['t2rgb_u8_' + tag])
    # the drop-in for one [H,W,2] flow, array in / array out and tensor in / tensor out
    for b in range(flow.shape[0]):
        hw2 = gold['rflow_' + tag][b].transpose(1, 2, 0)
        out = render.flow_to_image(hw2)
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == hw2.shape[:2] + (3,)
        assert np.abs(out.astype(np.int64) - gold['wheel_256_' + tag][b]).max() <= 1
        assert np.array_equal(_np(render.flow_to_image(_dev(hw2))), out)
        out = render.flow_to_image(hw2, max_flow=None)
        assert np.abs(out.astype(np.int64) - gold['wheel_none_' + tag][b]).max() <= 1


@pytest.mark.parametrize('shape', [(2, 33, 67), (2, 32, 68)])
def test_rgb_equals_the_torch_composition_bitwise(shape):
    from arflow_amd import render
    flow = _dev(R.make_flow(R.SEED + 2, *shape))
    absmax = flow.abs().amax((1, 2, 3))
    c, u8 = _rgb_torch(flow, absmax)
    assert torch.equal(render.torch_flow2rgb(flow), c)
    assert torch.equal(render.flow_rgb(flow, 'rgb'), u8)
    assert torch.equal(render.flow_rgb(flow.permute(0, 2, 3, 1).contiguous(), 'rgb', layout='nhwc'), u8)
    wide = torch.zeros(shape[0], 5, *shape[1:], device=DEV)
    wide[:, 1:3] = flow
    assert torch.equal(render.flow_rgb(wide[:, 1:3], 'rgb', stats=render.flow_stats(wide[:, 1:3])), u8)  # a channel slice
    c, u8 = _rgb_torch(flow, torch.full((shape[0],), 3.25, device=DEV))
    assert torch.equal(render.flow_rgb(flow, 'rgb', max_value=3.25), u8)


# ---- mode 1 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', R.RENDER_SHAPES + R.RENDER_SHAPES_WIDE)
@pytest.mark.parametrize('fixed', [True, False])
def test_wheel_band_rule(shape, fixed):
    """Every channel whose float64 level is outside every band equals floor(q); inside a band either neighbour."""
    from arflow_amd import render
    B, H, W = shape
    flow = R.make_wheel_flow(R.SEED, B, H, W)  # a negative-u-axis pixel, and for B = 3 a zero-flow sample
    scale = np.full(B, 256.0) if fixed else flow.reshape(B, -1).max(1).astype(np.float64)  # zero-flow sample: scale 0
    q, d = R.wheel64(flow, scale)
    for layout, t in (('nchw', _dev(flow)), ('nhwc', _dev(flow.transpose(0, 2, 3, 1)))):
        got = _np(render.flow_rgb(t, 'wheel', max_flow=256 if fixed else None, layout=layout))
        bad, share = R.band_check(got, q, d)
        print('wheel %s fixed=%s %s: %d outside, %.4f inside a band, %d differ from floor(q)'
              % (shape, fixed, layout, bad, share, int((got != np.clip(np.floor(q), 0, 255)).sum())))
        assert bad == 0
    if B >= 3:
        assert np.all(got[B - 1] == 255)  # the zero-flow sample renders white under either scale
    y, x = H // 2, W // 2
    assert got[0, y, x, 0] < 250 and min(got[0, y, x, 1:]) >= 254  # the negative u axis: cyan (a sector boundary: in a band)


def test_a_scale_that_is_not_positive_renders_white():
    from arflow_amd import render
    flow = _dev(R.make_flow(R.SEED, 2, 5, 7))
    for s in (0.0, -2.0, float('inf'), float('nan')):
        assert bool((render.flow_rgb(flow, 'rgb', max_value=s) == 255).all())
        assert bool((render.flow_rgb(flow, 'rgb', max_value=s, as_uint8=False) == 1).all())
    zero = torch.zeros(1, 2, 5, 7, device=DEV)
    assert bool((render.flow_rgb(zero, 'rgb') == 255).all()) and bool((render.flow_rgb(zero, 'wheel', max_flow=None) == 255).all())


# ---- the entropy picture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 9, 13), (2, 8, 16)])
def test_entropy_image_equals_the_torch_composition(shape):
    from arflow_amd import render
    B, H, W = shape
    x = _dev(R.make_entropy(R.SEED, B, H, W))
    e = torch.sum(x, dim=1, keepdim=True)  # uflow_elbo_trainer.py:259-261
    e = e - torch.min(e)
    e = e / torch.max(e)
    assert torch.equal(render.entropy_image(x, as_uint8=False), e)
    assert torch.equal(render.entropy_image(x), (e[:, 0] * 255.0).to(torch.uint8))
    wide = torch.zeros(B, 4, H, W, device=DEV)
    wide[:, 2:4] = x
    assert torch.equal(render.entropy_image(wide[:, 2:4], as_uint8=False), e)
    const = torch.full((B, 2, H, W), 0.75, device=DEV)
    assert bool((render.entropy_image(const) == 0).all()) and bool((render.entropy_image(const, as_uint8=False) == 0).all())


# ---- predict ---------------------------------------------------------------------------------------------------------------------------
def _pairs(sizes, test_hw=(64, 64)):
    g = torch.Generator().manual_seed(3)
    keys = ['a/%04d.png' % i for i in range(len(sizes))]
    imgs = [(torch.rand(1, 3, *test_hw, generator=g).to(DEV), torch.rand(1, 3, *test_hw, generator=g).to(DEV)) for _ in sizes]
    return keys, imgs, dict(zip(keys, sizes))


class _Recorded:
    """A model whose last output is kept, so a test compares with THAT call's tensors: two forward passes of the real models
    are not bitwise equal run to run (measured: pwclite differs in the last bits), and no tolerance is chosen for that here."""

    def __init__(self, model):
        self._model, self.outputs = model, []

    def __getattr__(self, name):
        return getattr(self._model, name)

    def __call__(self, *args, **kwargs):
        self.outputs.append(self._model(*args, **kwargs))
        return self.outputs[-1]


# uflow_prob refuses, as the reference does, a cost volume whose feature map is no taller than its max displacement 4; its
# coarsest level is 1/32 of the input, so 160 is the smallest test height it runs at (64 x 64 raises ValueError)
TEST_HW = {'pwclite_uflow': (64, 64), 'uflow_prob': (160, 160), 'pwclite': (64, 64)}


@pytest.mark.parametrize('arch', ['pwclite_uflow', 'uflow_prob'])
def test_predict_run_writes_what_restore_and_flow_rgb_give(arch, tmp_path):
    from arflow_amd import predict, render
    from arflow_amd.flow_io import read_flow
    from arflow_amd.inference import build_model
    model = _Recorded(build_model(arch, 2).to(DEV))
    rule = predict.entropy_rule(arch)
    keys, imgs, size = _pairs([(50, 70), (31, 53)], TEST_HW[arch])
    batches = [([k], a, b) for k, (a, b) in zip(keys, imgs)]
    n = predict.run(model, batches, size.__getitem__, predict.file_sink(str(tmp_path), 'ppm'), rule, 'wheel', rule is not None)
    assert n == 2
    assert len(model.outputs) == 2  # one model call per batch
    for k, res in zip(keys, model.outputs):
        H, W = size[k]
        stem = str(tmp_path / predict.stem_of(k))
        flows = res['flows_fw']
        assert tuple(flows[0].shape[2:]) == TEST_HW[arch]
        r = render.restore(flows[0][:, 0:2], (H, W), flows[0][:, 2:4] if rule else None, stats=True)
        flo = read_flow(stem + '.flo')
        assert flo.shape == (H, W, 2) and np.array_equal(flo, _np(r.flow[0]))
        blob = open(stem + '.ppm', 'rb').read()
        head = b'P6\n%d %d\n255\n' % (W, H)
        assert blob.startswith(head)
        vis = np.frombuffer(blob[len(head):], np.uint8).reshape(H, W, 3)
        assert np.array_equal(vis, _np(render.flow_rgb(r.flow, 'wheel', layout='nhwc')[0]))
        if rule:
            ent = np.load(stem + '.npy')
            assert ent.shape == (H, W, 2) and ent.dtype == np.float32 and np.array_equal(ent, _np(r.entropy[0]))
            assert os.path.getsize(stem + '_entropy.pgm') == len(b'P5\n%d %d\n255\n' % (W, H)) + H * W
        else:
            assert not os.path.exists(stem + '.npy')


class _Stub(torch.nn.Module):
    """Elementwise, so a sample's output does not depend on its batch: the plumbing of run() can be compared bit for bit."""
    upsample_out = True

    def forward(self, a, b, with_bk=False):
        return {'flows_fw': [torch.cat([a[:, :2] - b[:, :2], a[:, 1:3] * b[:, 1:3]], 1) * 5]}


def test_predict_batches_by_size_give_what_single_pairs_give():
    from arflow_amd import predict
    keys, imgs, size = _pairs([(40, 56), (40, 56)], (12, 20))
    one, two = {}, {}
    predict.run(_Stub(), [([k], a, b) for k, (a, b) in zip(keys, imgs)], size.__getitem__,
                lambda k, kind, a: one.__setitem__((k, kind), a), 'channels', 'rgb', True)
    predict.run(_Stub(), [(keys, torch.cat([a for a, _ in imgs]), torch.cat([b for _, b in imgs]))], size.__getitem__,
                lambda k, kind, a: two.__setitem__((k, kind), a), 'channels', 'rgb', True)
    assert sorted(one) == sorted(two) and len(one) == 8
    for key in one:
        assert one[key].shape[:2] == (40, 56) and np.array_equal(one[key], two[key]), key
    with pytest.raises(ValueError):
        predict.run(_Stub(), [(keys, imgs[0][0], imgs[0][1])], size.__getitem__, lambda *a: None)  # two keys, one frame


def test_cli_round_trip(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from arflow_amd import evaluate, inference, predict
    from arflow_amd.flow_io import read_flow, write_flow
    g = np.random.default_rng(5)
    frames = tmp_path / 'frames'
    frames.mkdir()
    sizes = [(72, 96), (72, 96), (72, 96), (48, 80), (48, 80)]
    for i, (H, W) in enumerate(sizes):
        Image.fromarray(g.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(str(frames / ('f%02d.png' % i)))
    out = tmp_path / 'out'
    predict.main(['--arch', 'uflow_prob', '--frames', str(frames), '--out', str(out), '-s', '160', '160', '--batch', '2',
                  '--vis', 'wheel', '--entropy-vis'])
    for i, (H, W) in enumerate(sizes[:-1]):
        stem = str(out / ('f%02d' % i))
        assert read_flow(stem + '.flo').shape == (H, W, 2) and np.load(stem + '.npy').shape == (H, W, 2)
        assert os.path.exists(stem + '.ppm') and os.path.exists(stem + '_entropy.pgm')
    assert not os.path.exists(str(out / 'f04.flo'))  # the last frame starts no pair
    gt = tmp_path / 'gt'
    gt.mkdir()
    for i, (H, W) in enumerate(sizes[:-1]):
        write_flow(str(gt / ('f%02d.flo' % i)), g.standard_normal((H, W, 2)).astype(np.float32))
    evaluate.main(['--pred', str(out), '--gt', str(gt), '--entropy', str(out)])  # accepts the directory unchanged
    # arflow_amd.inference: the additive flags, and the unchanged default
    a, b = str(frames / 'f03.png'), str(frames / 'f04.png')
    inference.main(['-s', '160', '160', '-i', a, b, '--arch', 'uflow_prob', '-o', str(tmp_path / 'o.flo'), '--orig-size',
                    '--entropy-out', str(tmp_path / 'o.npy'), '--vis-out', str(tmp_path / 'o.ppm'), '--entropy-vis',
                    str(tmp_path / 'o.pgm')])
    assert read_flow(str(tmp_path / 'o.flo')).shape == (48, 80, 2) and np.load(str(tmp_path / 'o.npy')).shape == (48, 80, 2)
    assert open(str(tmp_path / 'o.ppm'), 'rb').read().startswith(b'P6\n80 48\n255\n')
    assert os.path.getsize(str(tmp_path / 'o.pgm')) == len(b'P5\n80 48\n255\n') + 48 * 80
    inference.main(['-s', '160', '160', '-i', a, b, '--arch', 'uflow_prob', '-o', str(tmp_path / 'p.flo'), '--entropy-out',
                    str(tmp_path / 'p.npy')])
    assert read_flow(str(tmp_path / 'p.flo')).shape == (160, 160, 2) and np.load(str(tmp_path / 'p.npy')).shape == (160, 160, 2)


@pytest.mark.parametrize('arch', ['pwclite', 'uflow_prob'])
def test_infer_without_the_new_flags_is_the_model_output(arch):
    """infer() is untouched: it returns the NHWC view of what ITS model call returned (kept by _Recorded), bit for bit."""
    from arflow_amd.inference import build_model, infer
    model = _Recorded(build_model(arch, 2).to(DEV))
    g = torch.Generator().manual_seed(11)
    frames = [torch.rand(3, *TEST_HW[arch], generator=g), torch.rand(3, *TEST_HW[arch], generator=g)]
    flow = infer(model, frames, DEV)
    want = model.outputs[-1]['flows_fw'][0][0].permute(1, 2, 0).cpu().numpy()
    assert flow.shape == TEST_HW[arch] + (2,) and np.array_equal(flow, want[..., 0:2])
    if arch == 'uflow_prob':
        flow, ent = infer(model, frames, DEV, want_entropy=True)
        want = model.outputs[-1]['flows_fw'][0][0].permute(1, 2, 0).cpu().numpy()
        assert np.array_equal(flow, want[..., 0:2]) and np.array_equal(ent, want[..., 2:4])
    assert len(model.outputs) == (2 if arch == 'uflow_prob' else 1)  # one model call per infer()
