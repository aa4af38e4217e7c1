"""CPU: the uncertainty metrics (csrc/uncert.hip, arflow_amd/metrics.py) -- the float64 restatement
of tests/uncert_ref.py against what the reference returned for the fixture (tests/golden/uncert.npz,
tools/make_uncert_golden.py); the refinement driver and the interpolation of arflow_amd.metrics on CPU tensors, fed the
restatement's sums, against the same fixture down to the step at which every curve converged; the calibration curve from
the restatement's bins; argument validation; and the bound the GPU test holds arflow_sparsify_sums to, checked on a numpy
float32 transliteration of the kernel's arithmetic.  No GPU needed.

Bounds.  `sens` (stored per case by the tool, per point for a curve) is the largest change of an output of the reference over
8 draws of input noise of the size of fp32 rounding; a result that went through another resize (float64 here, fp32 on the
GPU) is held to 8 x sens, point by point, the multiple tests/test_triag_gpu.py grants over its stored gap."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import uncert_ref as U

ENULL, ESHAPE, EPARAM = -1001, -1002, -1003
TAGS = ('a', 'b', 'c')
N = 25
U24 = 2.0 ** -24


@pytest.fixture(scope='module')
def lib():
    from arflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope='module')
def cases(golden):
    z = golden('uncert')
    return {t: U.load_case(z, t) for t in TAGS}


@pytest.mark.parametrize('tag', TAGS)
def test_float64_sp_plot_on_the_stored_fields_matches_the_fixture(cases, tag):
    """Same fields, same float64 arithmetic: only the order of the pixel sums and expit's last bit differ."""
    c = cases[tag]
    for b in range(c['gt'].shape[0]):
        for f, (field, want) in enumerate(((c['ref_ent_map'][b], c['ref_splots'][b]), (c['ref_epe'][b], c['ref_oracle_splots'][b]))):
            got, resid = U.sp_plot(c['ref_epe'][b], field, c['mask'][b], N)
            stored = c['ref_resid'][b, f]
            stored = stored[~np.isnan(stored)]
            err = np.abs(got / want - 1).max()
            print(tag, b, f, 'splot rel err %.2e, checks %s' % (err, resid))
            assert err <= 1e-12
            assert len(resid) == len(stored) and np.abs(np.array(resid) - stored).max() <= 1e-12


@pytest.mark.parametrize('tag', TAGS)
def test_float64_evaluate_uncertainty_is_within_the_noise_floor(cases, tag):
    """The whole restatement from the inputs: its float64 resize and error map differ from the reference's fp32 ones."""
    c = cases[tag]
    got = U.evaluate_uncertainty(c['gt'], c['pred'], c['ent'], N)
    pair = np.array([got['AUC'].mean(), got['AUC_diff'].mean()])
    print(tag, 'pair', pair, 'reference', c['ref_pair'], 'sens', c['sens_pair'])
    assert np.all(np.abs(pair - c['ref_pair']) <= 8 * c['sens_pair'])
    for k in ('splots', 'oracle_splots'):
        err, tol = np.abs(got[k] - c['ref_' + k]), U.curve_tol(c['sens_' + k], c['ref_' + k])
        print(tag, k, 'max err / tol %.3f' % (err / tol).max())
        assert np.all(err <= tol)
    want_steps = [[U.steps_of(c['ref_resid'][b, f]) for f in range(2)] for b in range(c['gt'].shape[0])]
    assert got['steps'].tolist() == want_steps


def _sums_fn(err, fields, mask):
    """The restatement's sums for thr [B,F,K] -> [B,F,K,3] (float64 torch)."""
    def fn(thr):
        t = thr.numpy()
        return torch.from_numpy(np.stack([np.stack([U.sums(err[b], fields[f][b], mask[b], t[b, f]) for f in range(len(fields))])
                                          for b in range(t.shape[0])]))
    return fn


@pytest.mark.parametrize('tag', TAGS)
def test_metrics_sp_plot_on_cpu_tensors_follows_the_reference_break(cases, tag):
    """arflow_amd.metrics.sp_plot / sp_curves with sums_fn = the restatement: the curves of the fixture to 1e-10 and, per
    sample, the step at which the reference left its loop -- the frozen grid IS the reference's `break`."""
    from arflow_amd import metrics as M
    c = cases[tag]
    epe, emap, mask = c['ref_epe'], c['ref_ent_map'], c['mask']
    want_steps = np.array([[U.steps_of(c['ref_resid'][b, f]) for f in range(2)] for b in range(epe.shape[0])])
    assert want_steps.max() >= 1, 'the fixture must hold a curve that needed a refinement'
    te, tm, tg = (torch.from_numpy(np.array(t)) for t in (epe, emap, mask))
    for f, (field, name) in enumerate(((tm, 'splots'), (te, 'oracle_splots'))):
        splot, conv, steps = M.sp_plot(te, field, tg, N, sums_fn=_sums_fn(epe, [field.numpy()], mask), return_steps=True)
        assert splot.shape == (epe.shape[0], N) and splot.dtype == torch.float64 and conv.dtype == torch.bool
        err = (splot.numpy() / c['ref_' + name] - 1).__abs__().max()
        print(tag, name, 'rel err %.2e steps %s' % (err, steps.tolist()))
        assert err <= 1e-10 and bool(conv.all()) and steps.tolist() == want_steps[:, f].tolist()
    # both curves of every sample as one stack, the way evaluate_uncertainty drives it
    lo = torch.stack([tm.flatten(1).amin(1), te.flatten(1).amin(1)], 1)
    hi = torch.stack([tm.flatten(1).amax(1), te.flatten(1).amax(1)], 1)
    tot = tg.double().sum((1, 2))[:, None].expand(-1, 2)
    calls = []

    def counted(thr):
        calls.append(tuple(thr.shape))
        return _sums_fn(epe, [emap, epe], mask)(thr)
    splots, conv, steps = M.sp_curves(lo, hi, tot, counted, N)
    assert calls == [(epe.shape[0], 2, N)] * 11, 'always 1 + 10 evaluations of the whole batch'
    assert steps.tolist() == want_steps.tolist() and bool(conv.all())
    assert np.abs(splots[:, 0].numpy() / c['ref_splots'] - 1).max() <= 1e-10
    assert np.abs(splots[:, 1].numpy() / c['ref_oracle_splots'] - 1).max() <= 1e-10
    auc = M.auc_from_curves(splots)
    pair = np.array([float(auc[:, 0].mean()), float((auc[:, 0] - auc[:, 1]).mean())])
    assert np.abs(pair - c['ref_pair']).max() <= 1e-10
    # a 2-D input is a batch of one
    one = M.sp_plot(te[0], tm[0], tg[0], N, sums_fn=_sums_fn(epe[:1], [emap[:1]], mask[:1]))
    assert one[0].shape == (1, N) and np.abs(one[0][0].numpy() / c['ref_splots'][0] - 1).max() <= 1e-10


def test_sp_curves_reports_a_curve_that_does_not_converge_and_widens_a_soft_bracket():
    """A sums_fn whose fractions never move: 10 refinements, not converged.  And alpha * eps small enough that the end
    fractions miss 0 and 1 by more than eps: the widening loops run (against the restatement of their arithmetic here)."""
    from arflow_amd import metrics as M
    z = torch.zeros(2, 1)
    stuck = lambda thr: torch.stack([torch.full_like(thr, 0.5), torch.full_like(thr, 0.5), torch.full_like(thr, 0.25)], -1)  # noqa: E731
    splot, conv, steps = M.sp_curves(z, z + 1, z + 1, stuck, 5)
    assert not bool(conv.any()) and steps.tolist() == [[10], [10]] and torch.allclose(splot, torch.full_like(splot, 0.5))
    rng = np.random.default_rng(0)
    field = rng.normal(0, 1, (1, 12, 16)).astype(np.float32)
    err = np.abs(rng.normal(0, 1, (1, 12, 16))).astype(np.float32)
    mask = np.ones((1, 12, 16), np.float32)
    alpha, eps = 1.0, 0.1
    fn = lambda thr: torch.from_numpy(np.stack([np.stack([U.sums(err[0], field[0], mask[0], thr.numpy()[0, 0], alpha)])]))  # noqa: E731
    te, tf, tg = (torch.from_numpy(t) for t in (err, field, mask))
    splot, conv = M.sp_plot(te, tf, tg, 9, alpha=alpha, eps=eps, sums_fn=fn)
    # the reference's loops
    least, greatest = float(field.min()) - eps, float(field.max()) + eps
    frac = lambda t: U.sums(err[0], field[0], mask[0], [float(t)], alpha)[0, 0] / mask.sum()  # noqa: E731
    n_lo = n_hi = 0
    while abs(frac(least) - 1.0) > eps:
        least, n_lo = least - 1e-3 * (greatest - least), n_lo + 1
    while abs(frac(greatest)) > eps:
        greatest, n_hi = greatest + 1e-3 * (greatest - least), n_hi + 1
    assert n_lo > 3 and n_hi > 3
    grid = np.linspace(float(greatest), float(least), 9)
    s = U.sums(err[0], field[0], mask[0], grid, alpha)
    assert abs(s[0, 0] / mask.sum()) <= eps and abs(s[-1, 0] / mask.sum() - 1) <= eps
    assert splot.shape == (1, 9) and torch.isfinite(splot).all()
    assert abs(float(splot[0, 0]) - s[0, 2] / s[0, 1]) <= 2e-2 * abs(s[0, 2] / s[0, 1])


def test_torch_interp_equals_numpy_interp():
    from arflow_amd.metrics import interp
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = int(rng.integers(1, 9))
        xp = np.sort(np.round(rng.uniform(0, 1, n) * 4) / 4)        # ties on a grid of quarters
        if trial % 7 == 0:
            xp[:] = 0.5                                             # a constant xp
        fp = rng.normal(size=n)
        x = np.concatenate([np.round(rng.uniform(-0.5, 1.5, 9) * 8) / 8, rng.uniform(-0.5, 1.5, 4), xp[:1], xp[-1:]])
        want = np.interp(x, xp, fp)
        got = interp(torch.from_numpy(x)[None], torch.from_numpy(xp)[None], torch.from_numpy(fp)[None])[0].numpy()
        assert np.array_equal(want, got), (xp, fp, x, want, got)
        assert np.array_equal(want, U.interp(x, xp, fp)), (xp, fp, x)
    # batched: every row on its own xp
    xp = np.sort(rng.uniform(0, 1, (6, 25)), 1)
    fp, x = rng.normal(size=(6, 25)), rng.uniform(-0.1, 1.1, (6, 25))
    got = interp(torch.from_numpy(x), torch.from_numpy(xp), torch.from_numpy(fp)).numpy()
    assert np.array_equal(got, np.stack([np.interp(x[i], xp[i], fp[i]) for i in range(6)]))
    from arflow_amd.metrics import _linspace
    one = torch.ones((), dtype=torch.float64)
    assert np.array_equal(_linspace(0 * one, one, 25).numpy(), np.linspace(0, 1, 25))
    assert np.array_equal(_linspace(0 * one, 3.5 * one, 100).numpy(), np.linspace(0, 3.5, 100))
    assert np.array_equal(_linspace(2.75 * one, -1.3 * one, 25).numpy(), np.linspace(2.75, -1.3, 25))


def test_calibration_curve_from_the_restatement_bins_matches_the_fixture(cases):
    """Counts: equal up to the elements within 4 fp32 ulps of an edge (the reference bins an fp32 exp), asserted to be
    <= 0.5 % of the elements.  Means and standard deviations on the bins whose counts agree: 8 x sens; empty bins are NaN
    on both sides."""
    from arflow_amd.metrics import CalibrationCurve
    c = cases['b']
    cc = CalibrationCurve()
    edges = cc.edges('cpu').numpy()
    assert np.array_equal(edges, np.linspace(0, 3.5, 100))
    sums, band = U.calib_hist(c['pred'], c['gt'], c['ent'], edges)
    assert band <= 0.005 * c['ent'].numel()
    half = c['pred'].shape[0] // 2  # two updates pool into the same bins
    for sl in (slice(0, half), slice(half, None)):
        cc.update_from_sums(torch.from_numpy(U.calib_hist(c['pred'][sl], c['gt'][sl], c['ent'][sl], edges)[0]))
    vals, means, sigmas, numbers = cc.calibration_curve()
    assert len(vals) == len(means) == len(sigmas) == len(numbers) == 101 and isinstance(numbers[0], int)
    assert np.abs(np.array(vals) - c['ref_cc_vals']).max() <= 1e-15
    assert sum(numbers) == c['ent'].numel() and np.abs(np.array(numbers) - c['ref_cc_numbers']).max() <= band
    assert (c['ref_cc_numbers'] == 0).any() and (c['ref_cc_numbers'][-1] > 0), 'empty bins and values past cc_max'
    same = np.array(numbers) == c['ref_cc_numbers']
    for got, name in ((means, 'cc_means'), (sigmas, 'cc_sigmas')):
        got, want = np.array(got), c['ref_' + name]
        assert np.array_equal(np.isnan(got[same]), np.isnan(want[same])) and np.isnan(want).any()
        ok = same & ~np.isnan(want)
        err, tol = np.abs(got - want)[ok].max(), 8 * c['sens_' + name].max()
        print(name, 'max err %.3e tol %.3e' % (err, tol))
        assert err <= tol
    assert CalibrationCurve(2.0, 10).calibration_curve()[3] == [0] * 11
    with pytest.raises(ValueError):
        CalibrationCurve(3.5, 200)


def test_uncertainty_metrics_accumulates_unequal_batches():
    from arflow_amd.metrics import UncertaintyMetrics
    g = torch.Generator().manual_seed(2)
    res = {'AUC': torch.rand(5, generator=g, dtype=torch.float64), 'AUC_diff': torch.rand(5, generator=g, dtype=torch.float64),
           'splots': torch.rand(5, N, generator=g, dtype=torch.float64), 'oracle_splots': torch.rand(5, N, generator=g, dtype=torch.float64),
           'converged': torch.tensor([[1, 1], [1, 0], [1, 1], [0, 0], [1, 1]], dtype=torch.bool)}
    m = UncertaintyMetrics(N)
    assert m.compute() == {}
    for sl in (slice(0, 1), slice(1, 4), slice(4, 5)):
        m.update_from_result({k: v[sl] for k, v in res.items()})
    out = m.compute()
    assert list(out) == ['AUC', 'AUC_diff', 'splot', 'oracle_splot', 'not_converged'] and out['not_converged'] == 2  # samples with a curve that did not converge
    assert abs(out['AUC'] - float(res['AUC'].mean())) <= 1e-14 and abs(out['AUC_diff'] - float(res['AUC_diff'].mean())) <= 1e-14
    assert np.abs(np.array(out['splot']) - res['splots'].mean(0).numpy()).max() <= 1e-14
    assert np.abs(np.array(out['oracle_splot']) - res['oracle_splots'].mean(0).numpy()).max() <= 1e-14


def test_argument_errors_without_gpu(lib):
    # validation happens before any launch, so these are safe on a CPU-only host
    one = ctypes.c_void_p(16)

    def prep(**kw):
        a = dict(ent=one, epe=one, valid=None, vs=0, out=one, rows=one, B=1, h=4, w=4, H=8, W=8)
        a.update(kw)
        return lib.arflow_uncert_prep(a['ent'], a['epe'], a['valid'], a['vs'], a['out'], a['rows'], 1.0, 2.0, 1.0, 2.0, a['B'],
                                      a['h'], a['w'], a['H'], a['W'], None)

    def spars(**kw):
        a = dict(err=one, f0=one, f1=None, valid=None, vs=0, thr=one, rows=one, B=1, H=8, W=8, K=25)
        a.update(kw)
        return lib.arflow_sparsify_sums(a['err'], a['f0'], a['f1'], a['valid'], a['vs'], a['thr'], 100.0, a['rows'], a['B'],
                                        a['H'], a['W'], a['K'], None)

    def hist(**kw):
        a = dict(pred=one, gt=one, ent=one, edges=one, rows=one, B=1, C=4, H=8, W=8, nb=100)
        a.update(kw)
        return lib.arflow_calib_hist(a['pred'], a['gt'], a['ent'], a['edges'], a['rows'], a['B'], a['C'], a['H'], a['W'],
                                     a['nb'], None)
    for k in ('ent', 'epe', 'out', 'rows'):
        assert prep(**{k: None}) == ENULL, k
    for k in ('err', 'f0', 'thr', 'rows'):
        assert spars(**{k: None}) == ENULL, k
    for k in ('pred', 'gt', 'ent', 'edges', 'rows'):
        assert hist(**{k: None}) == ENULL, k
    for fn, keys in ((prep, 'BhwHW'), (spars, 'BHW'), (hist, 'BHW')):
        for k in keys:
            assert fn(**{k: 0}) == ESHAPE and fn(**{k: -2}) == ESHAPE, (fn.__name__, k)
    assert prep(valid=one, vs=63) == ESHAPE and spars(valid=one, vs=63) == ESHAPE  # a mask plane holds H * W floats
    assert spars(K=33) == EPARAM and spars(K=0) == EPARAM and spars(K=33, f1=one) == EPARAM
    assert hist(nb=129) == EPARAM and hist(nb=0) == EPARAM
    assert hist(C=3) == EPARAM and hist(C=1) == EPARAM
    assert spars(err=None, K=33, B=0) == ENULL and spars(K=33, B=0) == ESHAPE  # pointers, then shapes, then parameters
    assert lib.arflow_uncert_rows(0, 8) == ESHAPE and lib.arflow_calib_rows(8, 0) == ESHAPE
    assert lib.arflow_uncert_rows(1, 1) == 1 and lib.arflow_calib_rows(1, 1) == 2
    assert lib.arflow_uncert_rows(436, 1024) == 14 * 16 and lib.arflow_calib_rows(436, 1024) == 2 * 218
    assert lib.arflow_abi_version() == 10  # additive change


def test_wrappers_refuse_cpu_tensors_and_unequal_sizes():
    from arflow_amd import functional as AF, _lib
    from arflow_amd.metrics import CalibrationCurve, UncertaintyMetrics
    pred, gt, ent = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 8, 8), torch.zeros(1, 2, 4, 4)
    with pytest.raises(_lib.ArflowHipError):
        AF.uncert_prep(ent, torch.zeros(1, 1, 8, 8), gt)
    with pytest.raises(_lib.ArflowHipError):
        AF.sparsify_sums(gt[:, :1], gt[:, :1], None, gt, torch.zeros(1, 1, 25, dtype=torch.float64), 100.0)
    with pytest.raises(_lib.ArflowHipError):
        UncertaintyMetrics().update(pred, gt, ent)
    with pytest.raises(_lib.ArflowHipError):
        CalibrationCurve().update(torch.zeros(1, 2, 8, 8), gt, torch.zeros(1, 2, 8, 8))


def test_evaluate_cli_rejects_an_unmatched_entropy_directory(tmp_path):
    from arflow_amd import evaluate, flow_io
    flow = np.zeros((4, 6, 2), np.float32)
    for d in ('p', 'g', 'e'):
        (tmp_path / d).mkdir()
    for i in range(2):
        flow_io.write_flow(str(tmp_path / 'p' / ('%d.flo' % i)), flow)
        flow_io.write_flow(str(tmp_path / 'g' / ('%d.flo' % i)), flow)
    np.save(str(tmp_path / 'e' / '0.npy'), flow)
    args = ['--pred', str(tmp_path / 'p'), '--gt', str(tmp_path / 'g')]
    with pytest.raises(SystemExit, match='no entropy for 1.npy'):
        evaluate.main(args + ['--entropy', str(tmp_path / 'e')])
    with pytest.raises(SystemExit, match='directory'):
        evaluate.main(args + ['--entropy', str(tmp_path / 'e' / '0.npy')])
    with pytest.raises(SystemExit, match='needs --entropy'):
        evaluate.main(args + ['--calibration'])


def sparsify_fp32(err, field, g, thr, alpha):
    """arflow_sparsify_sums in numpy, operation by operation: d = (float)(thr - (double)field), a = alpha * d in fp32,
    m = 1 / (1 + expf(-a)) with a correctly rounded expf, fp32 partial sums over a thread's 8 pixels (2 rows x 4 columns of
    a 32 x 64 tile; here: 8 consecutive pixels of the flattened image, the same count), float64 from there on."""
    f32 = np.float32
    pad = (-err.size) % 8
    e, x, m_ = (np.concatenate([t.ravel().astype(f32), np.zeros(pad, f32)]).reshape(-1, 8) for t in (err, field, g))
    out = np.zeros((len(thr), 3))
    for k, t in enumerate(thr):
        d = (np.float64(t) - x.astype(np.float64)).astype(f32)
        a = f32(alpha) * d
        with np.errstate(over='ignore'):
            ex = np.exp(-a.astype(np.float64)).astype(f32)
            m = f32(1) / (f32(1) + ex)
        mg = m * m_
        terms = ((f32(1) - m) * m_, mg, e * mg)
        for q, v in enumerate(terms):
            s = np.zeros(v.shape[0], f32)
            for j in range(8):
                s = s + v[:, j]
            out[k, q] = s.astype(np.float64).sum()
    return out


def test_fp32_transliteration_of_sparsify_sums_stays_inside_the_derived_bound(cases):
    """The bound is uncert_ref.sums_tol (derived there from the counted roundings); the ratio reached is printed for
    DESIGN.md section 19.  k = K - 1 is the threshold min - 0.1: every term of the two
    relative sums is a sigmoid tail there."""
    worst = {'rel': 0.0, 'tail': 0.0, 'frac': 0.0}
    for tag in TAGS:
        c = cases[tag]
        for b in range(c['gt'].shape[0]):
            for field in (c['ref_ent_map'][b], c['ref_epe'][b]):
                thr = np.linspace(float(field.max()) + 0.1, float(field.min()) - 0.1, N)
                err, g = c['ref_epe'][b], c['mask'][b]
                want, got = U.sums(err, field, g, thr), sparsify_fp32(err, field, g, thr, 100.0)
                ratio = np.abs(got - want) / U.sums_tol(err, field, g, thr)
                assert want[-1, 1] < 1e-3 * g.sum(), 'the last threshold must leave only tails'
                worst['rel'], worst['tail'] = max(worst['rel'], ratio[:, 1:].max()), max(worst['tail'], ratio[-1, 1:].max())
                worst['frac'] = max(worst['frac'], ratio[:, 0].max())
    print('fp32 transliteration: error / bound -- relative sums %.3f (at k = K-1: %.3f), frac sums %.3f' %
          (worst['rel'], worst['tail'], worst['frac']))
    assert worst['rel'] <= 1.0 and worst['frac'] <= 1.0
