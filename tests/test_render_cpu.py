"""CPU: the float64 restatement and the fp32 emulation of tests/render_ref.py against the reference's own outputs
(tests/golden/render.npz, tools/make_render_golden.py), the bounds are not vacuous (every named mutation leaves them), the
render entry points are declared, bound and check their arguments before any launch, the PPM / PGM writers, and the pairing,
grouping and refusals of arflow_amd.predict -- none of it needs a GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['arflow_restore_out', 'arflow_flow_stats', 'arflow_flow_render', 'arflow_scalar_stats', 'arflow_scalar_render']
BAND_SHARE_MAX = 0.02


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'render.npz'), allow_pickle=False)


@pytest.fixture(scope='module')
def lib():
    from arflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _within(got, want, bound):
    err = np.abs(np.asarray(got, np.float64) - want)
    return float((err - bound).max()), float(err.max())


# ---- the golden vectors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['s', 'm'])
def test_rgb_emulation_equals_the_reference_bitwise(golden, tag):
    flow = golden['rflow_' + tag]
    absmax = np.abs(flow).reshape(flow.shape[0], -1).max(1)
    assert np.array_equal(R.rgb32(flow, absmax, False), golden['t2rgb_' + tag])          # torch_flow2rgb
    assert np.array_equal(R.rgb32(flow, absmax, True), golden['t2rgb_u8_' + tag])        # its uint8 cast
    val = np.full(flow.shape[0], 7.5, np.float32)
    assert np.array_equal(np.moveaxis(R.rgb32(flow, val, False), 1, -1), golden['rgb_val_' + tag])  # np_flow2rgb(max_value)
    # the float64 restatement: three fp32 roundings of magnitude <= 2 per channel
    assert np.abs(R.rgb64(flow, absmax) - golden['t2rgb_' + tag]).max() <= 6 * R.U1


@pytest.mark.parametrize('tag', ['up', 'down'])
def test_restore_restatement_reproduces_the_reference(golden, tag):
    B, h, w, H, W = (int(v) for v in golden['shape_' + tag])
    flow, ent = golden['flow_' + tag], golden['ent_' + tag]
    r = R.restore64(flow, (H, W), ent)
    fb, eb = R.golden_extra_bound(flow, (H, W), ent)
    over, err = _within(golden['ref_flow_' + tag], r['flow'], r['flow_bound'] + fb)
    print('restore %s: flow max err %.3e, over the bound by %.3e' % (tag, err, over))
    assert over <= 0
    over, err = _within(golden['ref_ent_' + tag], r['ent'], r['ent_bound'] + eb)
    print('restore %s: entropy max err %.3e, over the bound by %.3e' % (tag, err, over))
    assert over <= 0


@pytest.mark.parametrize('tag', ['s', 'm'])
@pytest.mark.parametrize('max_flow', [256, None])
def test_wheel_restatement_reproduces_the_reference(golden, tag, max_flow):
    flow = golden['rflow_' + tag]
    B = flow.shape[0]
    scale = np.full(B, 256.0) if max_flow else flow.reshape(B, -1).max(1).astype(np.float64)
    want = golden['wheel_%s_%s' % ('256' if max_flow else 'none', tag)]
    q, d = R.wheel64(flow, scale)
    bad, share = R.band_check(want, q, d)
    assert bad == 0, (bad, share)
    assert np.abs(want.astype(np.int64) - np.floor(q)).max() <= 1
    assert np.abs(R.wheel32(flow, scale).astype(np.int64) - want.astype(np.int64)).max() <= 1


# ---- the emulation stays inside the bounds, the mutations leave them -------------------------------------------------------------
@pytest.mark.parametrize('shape', R.RESTORE_SHAPES)
def test_restore_emulation_is_inside_the_bound(shape):
    B, h, w, H, W = shape
    flow, ent = R.make_flow(R.SEED, B, h, w), R.make_entropy(R.SEED, B, h, w)
    r64, r32 = R.restore64(flow, (H, W), ent), R.restore32(flow, (H, W), ent)
    assert _within(r32['flow'], r64['flow'], r64['flow_bound'])[0] <= 0
    assert _within(r32['ent'], r64['ent'], r64['ent_bound'])[0] <= 0
    assert r64['flow_bound'].max() < 1e-4 * np.abs(r64['flow']).max()  # the bound is a rounding bound, not a tolerance
    # the maxima of the rounded outputs are the rounded maxima of the exact ones, to the same bound
    assert np.all(np.abs(r32['stats'] - r64['stats']) <= r64['flow_bound'].max())


@pytest.mark.parametrize('mutate', ['align', 'inverse_scale', 'shift_sign', 'swap_uv', 'signed_absmax'])
def test_restore_mutations_leave_the_bound(mutate):
    B, h, w, H, W = R.RESTORE_SHAPES[0]
    flow, ent = R.make_flow(R.SEED, B, h, w), R.make_entropy(R.SEED, B, h, w)
    r64, bad = R.restore64(flow, (H, W), ent), R.restore32(flow, (H, W), ent, mutate)
    assert np.all(r64['stats'][:, 0] > r64['stats'][:, 1])  # the inputs make absmax and the signed max differ
    over = max(_within(bad['flow'], r64['flow'], r64['flow_bound'])[0], _within(bad['ent'], r64['ent'], r64['ent_bound'])[0],
               float((np.abs(bad['stats'] - r64['stats']) - r64['flow_bound'].max()).max()))
    assert over > 0, mutate


@pytest.mark.parametrize('shape', R.RENDER_SHAPES + R.RENDER_SHAPES_WIDE)
@pytest.mark.parametrize('fixed', [True, False])
def test_wheel_emulation_is_inside_the_band_and_the_inputs_are_decisive(shape, fixed):
    B, H, W = shape
    flow = R.make_wheel_flow(R.SEED, B, H, W)
    scale = np.full(B, 256.0) if fixed else flow.reshape(B, -1).max(1).astype(np.float64)
    q, d = R.wheel64(flow, scale)
    bad, share = R.band_check(R.wheel32(flow, scale), q, d)
    print('wheel %s fixed=%s: %.4f of the channel values inside a band' % (shape, fixed, share))
    assert bad == 0
    assert share <= BAND_SHARE_MAX  # on the float64 restatement alone: a GPU test cannot pass by ambiguity
    q_bad, _ = R.wheel64(flow, scale, mutate='sector')
    assert R.band_check(np.floor(q_bad), q, d)[0] > 0


def test_a_scale_that_is_not_positive_renders_white():
    flow = R.make_wheel_flow(R.SEED, 3, 5, 7)
    for s in (0.0, -1.0, np.inf, np.nan):
        scale = np.array([s, 1.0, 1.0])
        assert np.all(R.wheel32(flow, scale)[0] == 255) and np.all(R.rgb32(flow, scale, True)[0] == 255)
        assert np.all(R.wheel64(flow, scale)[0][0] == 255) and np.all(R.rgb64(flow, scale)[0] == 1)
    assert np.all(R.wheel32(flow, np.ones(3))[2] == 255)  # the zero-flow sample: saturation 0


def test_scalar_emulation_is_inside_the_bound():
    x = R.make_entropy(R.SEED, 2, 9, 13)
    r, d = R.scalar64(x)
    assert np.all(np.abs(R.scalar32(x, False) - r) <= d) and d.max() < 1e-5
    lo, hi = R.level_range(255 * r, 255 * d + R.U1 * 255 * r)
    got = R.scalar32(x, True).astype(np.int64)
    assert np.all((lo <= got) & (got <= hi)) and got.min() == 0 and got.max() == 255
    assert np.all(R.scalar32(np.full((1, 2, 3, 4), 0.25, np.float32), True) == 0)  # a constant map


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_render_symbols_are_declared_exported_and_bound(lib):
    from arflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'arflow_hip.h')).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n + '(' in header and n in _lib.PROTOTYPES and hasattr(raw, n), n
    assert lib.arflow_abi_version() == 10
    assert 'render.hip' in open(os.path.join(ROOT, 'arflow_amd', 'csrc', 'Makefile')).read()


def test_render_argument_errors_without_gpu(lib):
    one = ctypes.c_void_p(16)
    h, w, H, W = 4, 6, 8, 10
    ok = dict(flow=one, fbs=2 * h * w, ent=one, ebs=2 * h * w, of=one, oe=one, st=one, B=2)

    def restore(**kw):
        a = dict(ok, **kw)
        return lib.arflow_restore_out(a['flow'], a['fbs'], a['ent'], a['ebs'], a['of'], a['oe'], a['st'], a['B'], h, w, H, W, None)
    assert restore(flow=None) == -1001 and restore(of=None) == -1001
    assert restore(oe=None) == -1001 and restore(ent=None) == -1001  # entropy in and out come together
    assert restore(B=0) == -1002 and restore(fbs=2 * h * w - 1) == -1002 and restore(ebs=2 * h * w - 1) == -1002
    assert lib.arflow_restore_out(one, 48, None, 0, one, None, None, 1, h, w, 0, W, None) == -1002
    hw2 = 2 * H * W
    assert lib.arflow_flow_stats(None, hw2, 0, one, 1, H, W, None) == -1001
    assert lib.arflow_flow_stats(one, hw2, 0, None, 1, H, W, None) == -1001
    assert lib.arflow_flow_stats(one, hw2, 0, one, 0, H, W, None) == -1002
    assert lib.arflow_flow_stats(one, hw2 - 1, 1, one, 2, H, W, None) == -1002
    assert lib.arflow_flow_stats(one, hw2, 2, one, 1, H, W, None) == -1003
    render = lambda **kw: lib.arflow_flow_render(*[dict(dict(f=one, fbs=hw2, lay=0, sc=one, ss=1, out=one, kind=0, mode=0, B=1),  # noqa: E731
                                                        **kw)[k] for k in ('f', 'fbs', 'lay', 'sc', 'ss', 'out', 'kind', 'mode', 'B')],
                                                 H, W, None)
    assert render(f=None) == -1001 and render(sc=None) == -1001 and render(out=None) == -1001
    assert render(B=0) == -1002 and render(fbs=hw2 - 1) == -1002
    assert render(lay=2) == -1003 and render(kind=2) == -1003 and render(mode=2) == -1003 and render(mode=-1) == -1003
    assert lib.arflow_scalar_stats(None, hw2, 2, one, 1, H, W, None) == -1001
    assert lib.arflow_scalar_stats(one, hw2, 2, one, 0, H, W, None) == -1002
    assert lib.arflow_scalar_stats(one, hw2 - 1, 2, one, 1, H, W, None) == -1002
    assert lib.arflow_scalar_stats(one, hw2, 0, one, 1, H, W, None) == -1003
    assert lib.arflow_scalar_render(one, hw2, 2, None, one, 0, 1, H, W, None) == -1001
    assert lib.arflow_scalar_render(one, hw2, 2, one, one, 0, 0, H, W, None) == -1002
    assert lib.arflow_scalar_render(one, hw2, 2, one, one, 5, 1, H, W, None) == -1003
    lib.arflow_take_stale_error()


def test_render_refuses_cpu_tensors_and_wrong_types():
    import torch
    from arflow_amd import _lib, render
    f = torch.zeros(1, 2, 4, 6)
    for call in (lambda: render.restore(f, (8, 10)), lambda: render.flow_rgb(f), lambda: render.torch_flow2rgb(f),
                 lambda: render.flow_to_image(torch.zeros(4, 6, 2)), lambda: render.entropy_image(f),
                 lambda: render.flow_stats(f.permute(0, 2, 3, 1).contiguous(), 'nhwc')):
        with pytest.raises(_lib.ArflowHipError):
            call()
    with pytest.raises(ValueError):
        render.flow_rgb(f, mode='hsv')
    with pytest.raises(ValueError):
        render.restore(torch.zeros(1, 3, 4, 6), (8, 10))
    with pytest.raises(ValueError):
        render.restore(f, (0, 10))


# ---- files -----------------------------------------------------------------------------------------------------------------------
def _read_pnm(path):
    """a plain reader: magic, width, height, maxval as whitespace-separated ASCII, then the raw bytes"""
    blob = open(path, 'rb').read()
    fields, pos = [], 0
    while len(fields) < 4:
        end = pos
        while not blob[end:end + 1].isspace():
            end += 1
        fields.append(blob[pos:end])
        pos = end + 1
    w, h, maxval = (int(v) for v in fields[1:])
    assert maxval == 255
    a = np.frombuffer(blob[pos:], np.uint8)
    return fields[0], a.reshape(h, w, 3) if fields[0] == b'P6' else a.reshape(h, w)


def test_ppm_and_pgm_round_trip(tmp_path):
    from arflow_amd.flow_io import write_image, write_pgm, write_ppm
    g = np.random.default_rng(0)
    rgb, gray = g.integers(0, 256, (5, 7, 3), dtype=np.uint8), g.integers(0, 256, (5, 7), dtype=np.uint8)
    rgb[0, 0] = (10, 32, 13)  # whitespace bytes right behind the header
    write_ppm(tmp_path / 'a.ppm', rgb)
    write_pgm(tmp_path / 'a.pgm', gray)
    write_image(str(tmp_path / 'b.ppm'), rgb[:, ::-1])  # a view that is not contiguous
    write_image(str(tmp_path / 'b.pgm'), gray)
    assert _read_pnm(tmp_path / 'a.ppm')[0] == b'P6' and np.array_equal(_read_pnm(tmp_path / 'a.ppm')[1], rgb)
    assert _read_pnm(tmp_path / 'a.pgm')[0] == b'P5' and np.array_equal(_read_pnm(tmp_path / 'a.pgm')[1], gray)
    assert np.array_equal(_read_pnm(tmp_path / 'b.ppm')[1], rgb[:, ::-1]) and np.array_equal(_read_pnm(tmp_path / 'b.pgm')[1], gray)
    for bad in (lambda: write_ppm(tmp_path / 'c.ppm', gray), lambda: write_pgm(tmp_path / 'c.pgm', rgb),
                lambda: write_ppm(tmp_path / 'c.ppm', rgb.astype(np.float32)), lambda: write_image(str(tmp_path / 'c.pgm'), rgb),
                lambda: write_image(str(tmp_path / 'c.gif'), rgb)):
        with pytest.raises(ValueError):
            bad()


# ---- predict: names only ---------------------------------------------------------------------------------------------------------
def test_predict_pairs_and_groups_by_size():
    from arflow_amd import predict
    names = ['d/f_0003.png', 'd/f_0001.png', 'd/f_0002.png', 'd/f_0005.png', 'd/f_0004.png', 'd/f_0006.png']
    pairs = predict.pairs_from_frames(names)
    assert pairs == [('d/f_000%d.png' % i, 'd/f_000%d.png' % (i + 1)) for i in range(1, 6)]
    size = {'d/f_0001.png': (10, 20), 'd/f_0002.png': (30, 40), 'd/f_0003.png': (10, 20), 'd/f_0004.png': (10, 20),
            'd/f_0005.png': (10, 20)}
    groups = predict.group_by_size(pairs, size.__getitem__, 2)
    assert groups == [((10, 20), [pairs[0], pairs[2]]), ((10, 20), [pairs[3], pairs[4]]), ((30, 40), [pairs[1]])]
    assert sorted(p for _, g in groups for p in g) == sorted(pairs)  # every pair once
    assert all(len(g) <= 2 and len({size[a] for a, _ in g}) == 1 for _, g in groups)
    assert predict.group_by_size(pairs, size.__getitem__, 8)[0][1] == [pairs[0], pairs[2], pairs[3], pairs[4]]
    assert predict.pairs_from_frames(['only.png']) == []
    with pytest.raises(ValueError):
        predict.group_by_size([('a/x.png', 'a/y.png'), ('b/x.png', 'b/y.png')], lambda p: (1, 1), 2)  # both would write x.flo
    with pytest.raises(ValueError):
        predict.group_by_size(pairs, size.__getitem__, 0)
    assert predict.stem_of('/some/dir/frame_0001.final.png') == 'frame_0001.final'


def test_predict_pairs_file(tmp_path):
    from arflow_amd import predict
    p = tmp_path / 'pairs.txt'
    p.write_text('# a comment\na/1.png a/2.png\n\nb/7.png  b/9.png\n')
    assert predict.pairs_from_file(str(p)) == [('a/1.png', 'a/2.png'), ('b/7.png', 'b/9.png')]
    p.write_text('a/1.png\n')
    with pytest.raises(ValueError):
        predict.pairs_from_file(str(p))


def test_predict_entropy_rules_and_refusals():
    from arflow_amd import predict
    from arflow_amd.config import AttrDict
    assert predict.entropy_rule('uflow_prob', 'diag') == 'channels' and predict.entropy_rule('uflow_prob', 'sparse') == 'channels'
    assert predict.entropy_rule('uflow_prob', 'lowrank', columns=4) == 'lowrank' and predict.entropy_rule('uflow_prob', columns=2) == 'lowrank'
    assert predict.entropy_rule('pwclite_prob') == 'half'
    assert predict.entropy_rule('pwclite') is None and predict.entropy_rule('uflow') is None
    with pytest.raises(ValueError, match='weights'):
        predict.entropy_rule('uflow_prob', 'mixture')
    with pytest.raises(ValueError, match='weights'):
        predict.entropy_rule('component')
    with pytest.raises(ValueError, match='inv_cov'):
        predict.entropy_rule('uflow_prob', 'sparse', inv_cov=True)
    # the same refusals through a config, before any model is built
    for cfg in (dict(model=dict(type='component'), loss=dict(approx='mixture')),
                dict(model=dict(type='uflow_prob'), loss=dict(approx='mixture', n_components=3)),
                dict(model=dict(type='uflow_prob'), loss=dict(approx='sparse', inv_cov=True))):
        with pytest.raises(ValueError):
            predict.model_from_config(AttrDict(cfg))
    with pytest.raises(ValueError):
        predict.run(None, [], None, None, rule=None, entropy_vis=True)
