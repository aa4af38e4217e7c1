"""GPU: the uncertainty-metric kernels (csrc/uncert.hip) against the float64 restatement of tests/uncert_ref.py at the smallest
shapes that reach each path, and evaluate_uncertainty / UncertaintyMetrics / CalibrationCurve / validate / the evaluate CLI
on top of them against what the reference returned (tests/golden/uncert.npz).

Bounds (derived, not measured).
ent_map: atol = 32 * 2^-24 * M, M = max|entropy| + 2 max(log max(h, w), |log W/w|, |log H/h|), the larger of a channel's two
  intermediates (entropy - 2 log n, then + 2 log N: not their sum): two roundings in the shift and about six in the blend per channel, one in the channel sum (of magnitude <= 2 M)
  give <= 18 * 2^-24 * M (the `32 * 2^-24 * A` of tests/test_flow_eval_gpu.py, same blend).  min / max: the same bound against
  the restatement, and exactly the extremes of the map the kernel wrote.  sum valid: exact.
sparsify sums, against the restatement on the SAME fp32 maps (the ones the kernels produced) and thresholds:
  sum (1-m) g: absolute 2^-20 sum g.  sum m g, sum err m g: uncert_ref.sums_tol, per term (2 |a| (1 - m) + 12) * 2^-24 of
  itself (13 with err) from the counted roundings of d, a, expf, the division, the products and the 8-pixel fp32 partial
  sum, times a margin of 2 -- derived there, checked on a numpy transliteration in tests/test_uncert_cpu.py.  It holds at
  k = K - 1 too, where the threshold is min - 0.1 and every term is a sigmoid tail of e^-10 and below.
calibration: the kernel bins expf(entropy) (fp32), the restatement exp in float64, so a count may differ by the elements
  within 4 fp32 ulps of an edge (asserted on the restatement to be <= 0.5 % of the elements); sum e and sum e^2 are exact
  double sums of fp32 data in another order: 1e-12 relative on the bins whose counts agree.
end to end: 8 x sens per output, point by point for a curve (tests/test_uncert_cpu.py, module docstring), and the
  fixture's convergence steps."""
import json
import math

import numpy as np
import pytest
import torch

from tests import uncert_ref as U

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
N = 25
# name: (B, h, w, H, W, C)
CASES = {
    'same_c4': (2, 37, 53, 37, 53, 4),    # ratio 1, W % 4 != 0 (scalar path), partial tiles, a mask
    'up_c4': (3, 20, 33, 61, 130, 4),     # non-integer ratio, several rows per sample
    'x4_c2': (2, 24, 80, 96, 320, 2),     # x4, float4 path, several tile rows and columns, no mask
    'one': (1, 1, 1, 5, 7, 2),            # degenerate taps, constant entropy
}


def _raw_prep(ent, epe, gt):
    from arflow_amd import _lib, functional as AF
    B, _, H, W = epe.shape
    n = _lib.load().arflow_uncert_rows(H, W)
    rows = torch.full((B, n, 8), float('nan'), device='cuda', dtype=torch.float64)
    out = torch.full((B, 1, H, W), float('nan'), device='cuda')
    vp, vs = AF._valid_plane(gt, B, H, W)
    off = [float(np.float32(2 * math.log(v))) for v in (ent.shape[3], W, ent.shape[2], H)]
    AF._call('arflow_uncert_prep', AF._p(ent), AF._p(epe), vp, vs, AF._p(out), AF._p(rows), *off, B, ent.shape[2],
             ent.shape[3], H, W, AF._stream())
    return rows, out


def _raw_sums(err, f0, f1, gt, thr):
    from arflow_amd import _lib, functional as AF
    B, _, H, W = err.shape
    F, K = thr.shape[1:]
    n = _lib.load().arflow_uncert_rows(H, W)
    rows = torch.full((B, n, F, K, 3), float('nan'), device='cuda', dtype=torch.float64)
    vp, vs = AF._valid_plane(gt, B, H, W)
    AF._call('arflow_sparsify_sums', AF._p(err), AF._p(f0), AF._p(f1), vp, vs, AF._p(thr), 100.0, AF._p(rows), B, H, W, K,
             AF._stream())
    return rows


def _raw_hist(pred, gt, ent, edges):
    from arflow_amd import _lib, functional as AF
    B, C, H, W = gt.shape
    n = _lib.load().arflow_calib_rows(H, W)
    rows = torch.full((B, n, edges.numel() + 1, 3), float('nan'), device='cuda', dtype=torch.float64)
    AF._call('arflow_calib_hist', AF._p(pred), AF._p(gt), AF._p(ent), AF._p(edges), AF._p(rows), B, C, H, W, edges.numel(),
             AF._stream())
    return rows


@pytest.fixture(scope='module')
def prepared():
    """Per case, once: inputs on the device, the kernels' maps and prep rows, and the float64 restatement of the maps."""
    from arflow_amd import functional as AF
    out = {}
    for name, shape in CASES.items():
        B, h, w, H, W, C = shape
        pred, gt, ent = U.make_case(*shape)
        if name == 'one':
            ent = torch.full_like(ent, 0.75)
        dev = [t.cuda() for t in (pred, gt, ent)]
        _, epe = AF.flow_eval_sums(dev[0], dev[1], want_map=True)
        rows, emap = _raw_prep(dev[2], epe, dev[1])
        M = float(ent.abs().max()) + 2 * max(math.log(max(h, w)), abs(math.log(W / w)), abs(math.log(H / h)))
        out[name] = {'dev': dev, 'epe': epe, 'emap': emap, 'rows': rows, 'ref_map': U.entropy_map(ent, H, W),
                     'valid': gt[:, 2].double() if C == 4 else torch.ones(B, H, W, dtype=torch.float64),
                     'atol': 32 * U24 * M}
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_prep_map_and_rows(prepared, name):
    from arflow_amd import functional as AF
    r = prepared[name]
    emap, rows = r['emap'].cpu()[:, 0].double(), r['rows'].cpu()
    assert not torch.isnan(emap).any() and not torch.isnan(rows).any(), 'a pixel or a row was not written'
    err = float((emap - r['ref_map']).abs().max())
    print(name, 'ent_map max err %.3e atol %.3e' % (err, r['atol']))
    assert err <= r['atol']
    if name == 'one':
        assert float(emap.max() - emap.min()) <= r['atol']
    epe = r['epe'].cpu()[:, 0].double()
    got = torch.stack([rows[:, :, 0].amin(1), rows[:, :, 1].amax(1), rows[:, :, 2].amin(1), rows[:, :, 3].amax(1),
                       rows[:, :, 4].sum(1)], 1)
    want = torch.stack([emap.flatten(1).amin(1), emap.flatten(1).amax(1), epe.flatten(1).amin(1), epe.flatten(1).amax(1),
                        r['valid'].sum((1, 2))], 1)
    assert torch.equal(got, want), (got, want)  # the extremes of the maps as written, and the exact mask count
    assert float((got[:, 0] - r['ref_map'].flatten(1).amin(1)).abs().max()) <= r['atol']
    assert float((got[:, 1] - r['ref_map'].flatten(1).amax(1)).abs().max()) <= r['atol']
    assert torch.equal(rows[:, :, 5:], torch.zeros_like(rows[:, :, 5:]))
    # the wrapper folds the same rows
    wmap, stats = AF.uncert_prep(r['dev'][2], r['epe'], r['dev'][1])
    assert torch.equal(wmap, r['emap']) and torch.equal(stats.cpu(), got) and stats.dtype == torch.float64


def _thresholds(fields, K):
    """[B,F,K] float64: linspace(max + 0.1, min - 0.1, K) of every field of every sample."""
    return torch.from_numpy(np.stack([np.stack([np.linspace(float(f[b].max()) + 0.1, float(f[b].min()) - 0.1, K)
                                                for f in fields]) for b in range(fields[0].shape[0])]))


@pytest.mark.parametrize('F', [1, 2])
@pytest.mark.parametrize('K', [1, 25, 32])
@pytest.mark.parametrize('name', list(CASES))
def test_sparsify_sums_match_float64(prepared, name, K, F):
    from arflow_amd import functional as AF
    r = prepared[name]
    epe, emap = r['epe'].cpu()[:, 0].numpy(), r['emap'].cpu()[:, 0].numpy()
    fields = [emap, epe][:F]
    thr = _thresholds(fields, K)
    rows = _raw_sums(r['epe'], r['emap'], r['epe'] if F == 2 else None, r['dev'][1], thr.cuda())
    assert not torch.isnan(rows).any(), 'a row of the buffer was not written'
    got = rows.sum(1).cpu().numpy()
    # the wrapper folds the same rows (on the device: a host sum adds them in another order)
    assert torch.equal(AF.sparsify_sums(r['epe'], r['emap'], r['epe'] if F == 2 else None, r['dev'][1], thr.cuda(), 100.0),
                       rows.sum(1))
    valid = r['valid'].numpy()
    worst = np.zeros(3)
    for b in range(epe.shape[0]):
        for f in range(F):
            want = U.sums(epe[b], fields[f][b], valid[b], thr[b, f].numpy())
            tol = U.sums_tol(epe[b], fields[f][b], valid[b], thr[b, f].numpy())
            ratio = np.abs(got[b, f] - want) / tol
            worst = np.maximum(worst, ratio.max(0))
            assert np.all(ratio <= 1.0), (name, K, F, b, f, ratio.max(0), int(ratio.max(1).argmax()))
            if K > 1:  # the last threshold leaves only tails, and the bound holds there
                assert want[-1, 1] < 1e-3 * valid[b].sum() and np.all(ratio[-1] <= 1.0)
    print(name, K, F, 'error / bound: frac %.3f, sum m g %.3f, sum err m g %.3f' % tuple(worst))


@pytest.mark.parametrize('name', ['up_c4', 'x4_c2'])
def test_prep_and_sums_are_bitwise_equal_in_either_mode(prepared, name):
    from arflow_amd import functional as AF
    r = prepared[name]
    thr = _thresholds([r['emap'].cpu()[:, 0].numpy(), r['epe'].cpu()[:, 0].numpy()], N).cuda()
    first = None
    for on in (False, True):
        with AF.deterministic(on):
            for _ in range(2):
                rows, emap = _raw_prep(r['dev'][2], r['epe'], r['dev'][1])
                srows = _raw_sums(r['epe'], r['emap'], r['epe'], r['dev'][1], thr)
                if first is None:
                    first = (rows, emap, srows)
                assert torch.equal(rows, first[0]) and torch.equal(emap, first[1]) and torch.equal(srows, first[2])
    assert torch.equal(first[0], r['rows']) and torch.equal(first[1], r['emap'])


def test_unaligned_planes_take_the_scalar_path_to_the_same_bits(prepared):
    r = prepared['x4_c2']

    def off(t):  # same values, base 4 bytes off a 16-byte boundary
        pad = torch.zeros(t.numel() + 1, device='cuda', dtype=t.dtype)
        pad[1:] = t.flatten()
        v = pad[1:].view_as(t)
        assert v.data_ptr() % 16 != 0
        return v
    thr = _thresholds([r['emap'].cpu()[:, 0].numpy(), r['epe'].cpu()[:, 0].numpy()], N).cuda()
    a = _raw_sums(r['epe'], r['emap'], r['epe'], r['dev'][1], thr)
    b = _raw_sums(off(r['epe']), r['emap'], r['epe'], r['dev'][1], thr)
    assert torch.equal(a, b)
    rows, emap = _raw_prep(r['dev'][2], off(r['epe']), r['dev'][1])
    assert torch.equal(rows, r['rows']) and torch.equal(emap, r['emap'])


# ---- calibration ------------------------------------------------------------------------------------------------------
CALIB = {'c4': (2, 36, 60, 4),      # several workgroups per plane, the ground truth's four channels
         'c2_vec': (1, 96, 320, 2),  # float4, many workgroups
         'odd': (1, 37, 53, 2)}      # H * W % 4 != 0: the scalar path, a partial last workgroup
FIELDS = ('constant', 'smooth', 'fast')


@pytest.fixture(scope='module')
def calib():
    out = {}
    edges = np.linspace(0, 3.5, 100)
    for name, (B, H, W, C) in CALIB.items():
        pred, gt, smooth = U.make_case(B, H, W, H, W, C)
        rng = np.random.default_rng(3)
        # fast: i.i.d. sigma over (0.01, 4.5): the 64 lanes of a wave meet well over 32 bins, some past cc_max
        fast = torch.from_numpy(np.log(rng.uniform(0.01, 4.5, tuple(smooth.shape))).astype(np.float32))
        for kind, ent in zip(FIELDS, (torch.full_like(smooth, 0.3), smooth, fast)):
            want, band = U.calib_hist(pred, gt, ent, edges)
            dev = [t.cuda() for t in (pred, gt, ent)]
            rows = _raw_hist(*dev, torch.from_numpy(edges).cuda())
            out[name, kind] = {'dev': dev, 'rows': rows, 'want': want, 'band': band, 'n': ent.numel()}
    return out


@pytest.mark.parametrize('kind', FIELDS)
@pytest.mark.parametrize('name', list(CALIB))
def test_calibration_histogram(calib, name, kind):
    from arflow_amd import functional as AF
    r = calib[name, kind]
    assert r['band'] <= 0.005 * r['n'], 'the inputs put %d of %d elements on a bin edge' % (r['band'], r['n'])
    rows = r['rows']
    assert not torch.isnan(rows).any(), 'a row of the buffer was not written'
    got, want = rows.sum((0, 1)).cpu().numpy(), r['want']
    used = int((want[:, 0] > 0).sum())
    if kind == 'constant':
        assert used == 1
    if kind == 'fast':
        assert used >= 90 and want[-1, 0] > 0, 'a wave must meet many bins, and values past cc_max'
    assert got[:, 0].sum() == r['n'] and np.abs(got[:, 0] - want[:, 0]).max() <= r['band']
    same = got[:, 0] == want[:, 0]
    for q in (1, 2):
        err = np.abs(got[same, q] - want[same, q]) / np.maximum(want[same, q], 1e-300)
        print(name, kind, 'column %d: %d bins in use, max rel err %.2e' % (q, used, err.max()))
        assert err.max() <= 1e-12
    edges = torch.from_numpy(np.linspace(0, 3.5, 100)).cuda()
    assert torch.equal(AF.calib_hist_sums(*r['dev'], edges), rows.sum((0, 1)))
    for on in (False, True):
        with AF.deterministic(on):
            for _ in range(2):
                assert torch.equal(_raw_hist(*r['dev'], edges), r['rows'])


def test_calibration_refuses_unequal_sizes():
    from arflow_amd.metrics import CalibrationCurve
    pred, gt, ent = (t.cuda() for t in U.make_case(1, 12, 16, 24, 32, 2))
    with pytest.raises(ValueError):
        CalibrationCurve().update(pred, gt, ent)


# ---- end to end against the reference's fixture -------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fixture_cases(golden):
    z = golden('uncert')
    return {t: U.load_case(z, t) for t in ('a', 'b', 'c')}


def _steps(c):
    return [[U.steps_of(c['ref_resid'][b, f]) for f in range(2)] for b in range(c['gt'].shape[0])]


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_evaluate_uncertainty_matches_the_reference(fixture_cases, tag):
    from arflow_amd.metrics import UncertaintyMetrics, evaluate_uncertainty
    c = fixture_cases[tag]
    pred, gt, ent = (c[k].cuda() for k in ('pred', 'gt', 'ent'))
    res = evaluate_uncertainty(gt, pred, ent, N)
    assert all(v.is_cuda for v in res.values()) and res['splots'].dtype == torch.float64
    assert res['steps'].tolist() == _steps(c) and bool(res['converged'].all())
    pair = np.array([float(res['AUC'].mean()), float(res['AUC_diff'].mean())])
    print(tag, 'pair', pair, 'reference', c['ref_pair'], 'err / (8 sens)', np.abs(pair - c['ref_pair']) / (8 * c['sens_pair']))
    assert np.all(np.abs(pair - c['ref_pair']) <= 8 * c['sens_pair'])
    for k in ('splots', 'oracle_splots'):
        err, tol = np.abs(res[k].cpu().numpy() - c['ref_' + k]), U.curve_tol(c['sens_' + k], c['ref_' + k])
        print(tag, k, 'max err / tol %.3f' % (err / tol).max())
        assert np.all(err <= tol)
    # the meter: two updates of unequal size give the reference's batch means
    m = UncertaintyMetrics(N)
    m.update(pred[:1], gt[:1], ent[:1])
    if pred.shape[0] > 1:
        m.update(pred[1:], gt[1:], ent[1:])
    out = m.compute()
    assert out['not_converged'] == 0
    assert abs(out['AUC'] - c['ref_pair'][0]) <= 8 * c['sens_pair'][0]
    assert abs(out['AUC_diff'] - c['ref_pair'][1]) <= 8 * c['sens_pair'][1]
    for k in ('splot', 'oracle_splot'):  # the mean curve: within the mean of the points' bounds
        ref, sens = c['ref_' + k + 's'], c['sens_' + k + 's']
        assert np.all(np.abs(np.array(out[k]) - ref.mean(0)) <= U.curve_tol(sens, ref).mean(0)), k
    # a sample without valid pixels is NaN, and only that sample
    if gt.shape[1] == 4:
        gt0 = gt.clone()
        gt0[0, 2:] = 0
        r0 = evaluate_uncertainty(gt0, pred, ent, N)
        assert bool(torch.isnan(r0['AUC'][0])) and torch.equal(r0['AUC'][1:], res['AUC'][1:])


@pytest.mark.parametrize('tag', ['a', 'c'])
def test_public_sp_plot_on_device_tensors(fixture_cases, tag):
    """metrics.sp_plot with its own sums (the F = 1 kernel, a bare [B,1,H,W] mask, the bracket from amin / amax) gives
    the curve evaluate_uncertainty gives (the F = 2 kernel, the mask inside the ground truth, the bracket from the prep
    rows): the same arithmetic per field, so 1e-12 relative.  And with alpha * eps = 0.1 the bracket is widened by the
    host-driven loop over the real K = 1 launch: against the same driver on CPU tensors fed the float64 sums, 1e-5
    relative (alpha = 1: uncert_ref.sums_tol is ~15 * 2^-24 per term there)."""
    from arflow_amd import functional as AF, metrics as M
    c = fixture_cases[tag]
    pred, gt, ent = (c[k].cuda() for k in ('pred', 'gt', 'ent'))
    res = M.evaluate_uncertainty(gt, pred, ent, N)
    _, epe = AF.flow_eval_sums(pred, gt, want_map=True)
    emap, _ = AF.uncert_prep(ent, epe, gt)
    mask = gt[:, 2] if gt.shape[1] == 4 else torch.ones_like(epe[:, 0])
    for field, name in ((emap[:, 0], 'splots'), (epe[:, 0], 'oracle_splots')):
        splot, conv, steps = M.sp_plot(epe[:, 0], field, mask, N, return_steps=True)
        assert splot.is_cuda and bool(conv.all())
        f = 0 if name == 'splots' else 1
        assert steps.tolist() == res['steps'][:, f].tolist()
        assert float((splot / res[name] - 1).abs().max()) <= 1e-12
    one = M.sp_plot(epe[0, 0], emap[0, 0], mask[0], N)[0]  # a 2-D input is a batch of one
    assert one.shape == (1, N) and float((one[0] / res['splots'][0] - 1).abs().max()) <= 1e-12
    # the widening loops
    e, x, g = (t.cpu().numpy() for t in (epe[:, 0], emap[:, 0], mask))

    def ref_sums(thr):
        return torch.from_numpy(np.stack([np.stack([U.sums(e[b], x[b], g[b], thr[b, 0].numpy(), 1.0)]) for b in range(len(e))]))
    calls = []

    def counted(thr):
        calls.append(thr.shape[-1])
        return ref_sums(thr)
    want, wconv = M.sp_plot(*(torch.from_numpy(t) for t in (e, x, g)), 9, alpha=1.0, eps=0.1, sums_fn=counted)
    assert calls.count(1) > 10, 'the bracket must need widening'
    got, gconv = M.sp_plot(epe[:, 0], emap[:, 0], mask, 9, alpha=1.0, eps=0.1)
    assert gconv.tolist() == wconv.tolist()
    assert float((got.cpu() / want - 1).abs().max()) <= 1e-5


def _check_curve(c, vals, means, sigmas, numbers, band):
    assert np.abs(np.array(vals) - c['ref_cc_vals']).max() <= 1e-15
    assert np.abs(np.array(numbers) - c['ref_cc_numbers']).max() <= band and sum(numbers) == c['ent'].numel()
    same = np.array(numbers) == c['ref_cc_numbers']
    for got, name in ((means, 'cc_means'), (sigmas, 'cc_sigmas')):
        got, want = np.array(got), c['ref_' + name]
        assert np.array_equal(np.isnan(got[same]), np.isnan(want[same]))
        ok = same & ~np.isnan(want)
        err, tol = np.abs(got - want)[ok].max(), 8 * c['sens_' + name].max()
        print(name, 'max err %.3e tol %.3e' % (err, tol))
        assert err <= tol


def test_calibration_curve_matches_the_reference(fixture_cases):
    from arflow_amd.metrics import CalibrationCurve
    c = fixture_cases['b']
    _, band = U.calib_hist(c['pred'], c['gt'], c['ent'], np.linspace(0, 3.5, 100))
    assert band <= 0.005 * c['ent'].numel()
    cc = CalibrationCurve()
    for sl in (slice(0, 1), slice(1, None)):
        cc.update(c['pred'][sl].cuda(), c['gt'][sl].cuda(), c['ent'][sl].cuda())
    assert cc.state.is_cuda and tuple(cc.state.shape) == (101, 3)
    _check_curve(c, *cc.calibration_curve(), band)


class _Stub(torch.nn.Module):
    """A model that hands out recorded flows, one batch per call."""

    def __init__(self, flows):
        super().__init__()
        self.flows, self.i = flows, 0

    def forward(self, x):
        self.i += 1
        return {'flows_fw': [self.flows[self.i - 1]], 'entropy': self.i - 1}


def test_validate_with_entropy_returns_the_same_numbers(fixture_cases):
    from arflow_amd.metrics import validate
    c = fixture_cases['a']
    pred, gt, ent = (c[k].cuda() for k in ('pred', 'gt', 'ent'))
    batches = [(torch.zeros(1, 6, 8, 8, device='cuda'), gt[:1]), (torch.zeros(1, 6, 8, 8, device='cuda'), gt[1:])]
    ents = [ent[:1], ent[1:]]
    model = _Stub([pred[:1], pred[1:]])
    model.train()
    out = validate(model, batches, entropy_of=lambda res: ents[res['entropy']])
    assert model.training
    assert list(out) == ['EPE', 'E_noc', 'E_occ', 'F1_all', 'AUC', 'AUC_diff', 'splot', 'oracle_splot', 'not_converged']
    assert abs(out['AUC'] - c['ref_pair'][0]) <= 8 * c['sens_pair'][0] and out['not_converged'] == 0
    assert abs(out['AUC_diff'] - c['ref_pair'][1]) <= 8 * c['sens_pair'][1]
    plain = validate(_Stub([pred[:1], pred[1:]]), batches)
    assert list(plain) == ['EPE', 'E_noc', 'E_occ', 'F1_all'] and all(plain[k] == out[k] for k in plain)


def test_evaluate_cli_with_entropy(fixture_cases, tmp_path, capsys):
    from arflow_amd import evaluate, flow_io
    hwc = lambda t: np.ascontiguousarray(t.permute(1, 2, 0).numpy())  # noqa: E731
    c = fixture_cases['c']  # dense ground truth: what a .flo file holds
    flow_io.write_flow(str(tmp_path / 'pred.flo'), hwc(c['pred'][0]))
    flow_io.write_flow(str(tmp_path / 'gt.flo'), hwc(c['gt'][0]))
    np.save(str(tmp_path / 'ent.npy'), hwc(c['ent'][0]))
    args = ['--pred', str(tmp_path / 'pred.flo'), '--gt', str(tmp_path / 'gt.flo')]
    plain = evaluate.main(args)
    out = evaluate.main(args + ['--entropy', str(tmp_path / 'ent.npy')])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == out and list(out) == ['EPE', 'pairs', 'AUC', 'AUC_diff', 'not_converged'] and list(plain) == ['EPE', 'pairs']
    assert out['EPE'] == plain['EPE'] and out['not_converged'] == 0
    assert abs(out['AUC'] - c['ref_pair'][0]) <= 8 * c['sens_pair'][0]
    assert abs(out['AUC_diff'] - c['ref_pair'][1]) <= 8 * c['sens_pair'][1]
    # two directories matched by stem, with the calibration curve (it ignores the mask: the lists of case b)
    c = fixture_cases['b']
    for d in ('p', 'g', 'e'):
        (tmp_path / d).mkdir()
    for i in range(2):
        flow_io.write_flow(str(tmp_path / 'p' / ('%d.flo' % i)), hwc(c['pred'][i]))
        flow_io.write_flow(str(tmp_path / 'g' / ('%d.flo' % i)), hwc(c['gt'][i, :2]))
        np.save(str(tmp_path / 'e' / ('%d.npy' % i)), hwc(c['ent'][i]))
    out = evaluate.main(['--pred', str(tmp_path / 'p'), '--gt', str(tmp_path / 'g'), '--entropy', str(tmp_path / 'e'),
                         '--calibration'])
    assert out['pairs'] == 2 and 0.0 < out['AUC'] < 1.0
    _, band = U.calib_hist(c['pred'], c['gt'], c['ent'], np.linspace(0, 3.5, 100))
    _check_curve(c, out['cc_vals'], out['cc_means'], out['cc_sigmas'], out['cc_numbers'], band)
