"""GPU: the sparse triangular solves (csrc/triag.hip, arflow_amd/triag_solve.py) against what the reference's own code
computed (tests/golden/triag.npz) and, for the grids without a golden entry, against the float64 restatement of
tests/triag_ref.py that the CPU tests pin to that file.

Bounds.  The fixture stores, per output, the gap between the reference's OWN fp32 and float64 runs relative to the
output's largest magnitude (`noise_*`).  An output passes if |got - ref| <= 8 * noise * max|ref|; grids without a golden
entry (and the runs with D = None, which the fixture does not hold) use the largest stored gap of that kind.  The
residual max|J Y - X| / max|X| is held under the same absolute bound times the operator's infinity norm (|J (Y - Yref)|
<= |J|_inf |Y - Yref|_inf, and max|X| >= 1 for these inputs).  Marginal variances: relative error per element <= 8 *
noise_H.  On top of that the kernel states that it keeps the reference's operation order with an IEEE division, so the
solves are also compared bit for bit with the restatement run in fp32.

Grids: the smallest that reach each path of the kernel -- see GRIDS."""
import numpy as np
import pytest
import torch

from tests import triag_ref as R

pytestmark = pytest.mark.gpu

# (K, L, M, N): rows are swept in strips of 64 (one lane per row), columns in chunks of 16 steps
GRIDS = dict(R.SOLVE_CASES)          # strip: crosses a strip boundary; wide: 3 rows, 132 steps, mostly idle lanes;
GRIDS.update(one=(1, 1, 1, 1),       # tall: three strips, narrow; row / col: empty C, D / empty B, D (golden, all five)
             odd=(3, 5, 17, 23))     # a single element; an odd plane count
OUTPUTS = ('Y', 'gX', 'gA', 'gB', 'gC', 'gD')
DIRS = (('lo', 0), ('up', 1))


def _noise(g, key, tag, d, with_d):
    """The stored relative gap of the reference's fp32 run for this output, or the largest one stored for that output."""
    name = 'noise_%s_%s_%s' % (key, d, tag)
    if with_d and name in g:
        return float(g.raw(name))
    return max(float(g.raw(n)) for n in g._z.files if n.startswith('noise_%s_' % key))


def _cuda(case, with_d):
    t = {k: torch.from_numpy(v).cuda() for k, v in case.items()}
    if not with_d:
        t['D'] = None
    return t


def _raw_solve(t, upper):
    """The raw entry point into a NaN-filled output."""
    from arflow_amd import functional as AF
    K, L, M, N = t['A'].shape
    Y = torch.full_like(t['X'], float('nan'))
    AF._call('arflow_triag_solve', AF._p(t['A']), AF._p(t['B']), AF._p(t['C']), AF._p(t['D']), AF._p(t['X']), AF._p(Y), K * L,
             M, N, upper, AF._stream())
    return Y


def _raw_bwd(t, Y, upper):
    from arflow_amd import functional as AF
    K, L, M, N = t['A'].shape
    nan = lambda x: None if x is None else torch.full_like(x, float('nan'))  # noqa: E731
    out = {'gX': nan(Y), 'gA': nan(t['A']), 'gB': nan(t['B']), 'gC': nan(t['C']), 'gD': nan(t['D'])}
    AF._call('arflow_triag_solve_bwd', AF._p(t['A']), AF._p(t['B']), AF._p(t['C']), AF._p(t['D']), AF._p(Y), AF._p(t['gY']),
             *[AF._p(out[k]) for k in ('gX', 'gA', 'gB', 'gC', 'gD')], K * L, M, N, upper, AF._stream())
    return out


@pytest.fixture(scope='module')
def runs(golden):
    """Every grid, direction and D / no D once: the reference (golden where the fixture holds the run, else the float64
    restatement), the fp32 restatement of the solve, and the kernels' outputs through the autograd functions."""
    from arflow_amd import triag_solve as T
    g = golden('triag')
    out = {}
    for tag, shape in GRIDS.items():
        case = R.make_case(*shape)
        for with_d in (True, False):
            D = case['D'] if with_d else None
            for d, upper in DIRS:
                if with_d and tag in R.SOLVE_CASES:
                    ref = {k: g.raw('%s_%s_%s' % (k, d, tag)) for k in OUTPUTS}
                else:
                    Y = R.solve(case['A'], case['B'], case['C'], D, case['X'], bool(upper))
                    ref = dict(R.grads(case['A'], case['B'], case['C'], D, Y, case['gY'], bool(upper)), Y=Y)
                t = _cuda(case, with_d)
                before = {k: v.clone() for k, v in t.items() if v is not None}
                leaves = {k: t[k].requires_grad_(True) for k in 'ABCDX' if t[k] is not None}
                fn = T.BackwardSubst if upper else T.ForwardSubst
                Y = fn.apply(t['A'], t['B'], t['C'], t['D'], t['X'])
                Y.backward(t['gY'])
                got = {'Y': Y.detach().cpu().numpy()}
                got.update({'g' + k: v.grad.cpu().numpy() for k, v in leaves.items()})
                out[tag, d, with_d] = {
                    'ref': ref, 'got': got, 'case': case, 'D': D, 't': {k: (None if v is None else v.detach()) for k, v in t.items()},
                    'before': before, 'Ydev': Y.detach(),
                    'Y32': R.solve(case['A'], case['B'], case['C'], D, case['X'], bool(upper), dtype=np.float32)}
    return out


RUNS = [(tag, d, with_d) for tag in GRIDS for d, _ in DIRS for with_d in (True, False)]


def _ids(v):
    return '%s-%s-%s' % (v[0], v[1], 'D' if v[2] else 'noD')


def _inf_norm(case, D):
    """The largest absolute row sum of J (the same for both forms up to the neighbours' side: take the larger)."""
    a = {k: np.abs(case[k]).astype(np.float64) for k in 'ABC'}
    d = None if D is None else np.abs(D).astype(np.float64)
    ones = np.ones_like(a['A'])
    return max(R.matvec(a['A'], a['B'], a['C'], d, ones, u).max() for u in (False, True))


@pytest.mark.parametrize('run', RUNS, ids=_ids)
def test_solve_against_the_reference(golden, runs, run):
    tag, d, with_d = run
    r = runs[run]
    ref, got = r['ref']['Y'], r['got']['Y']
    assert got.shape == ref.shape and np.isfinite(got).all()
    bound = 8 * _noise(golden('triag'), 'Y', tag, d, with_d) * np.abs(ref).max()
    err = np.abs(got - ref).max()
    case = r['case']
    res = np.abs(R.matvec(case['A'], case['B'], case['C'], r['D'], got, d == 'up') - case['X']).max() / np.abs(case['X']).max()
    print('%s: |Y - ref| %.3e (bound %.3e), residual %.3e (bound %.3e), max|Y| %.2f' %
          (_ids(run), err, bound, res, bound * _inf_norm(case, r['D']), np.abs(ref).max()))
    assert err <= bound
    assert res <= bound * _inf_norm(case, r['D'])


@pytest.mark.parametrize('run', RUNS, ids=_ids)
def test_solve_is_the_fp32_recurrence_bit_for_bit(runs, run):
    """The kernel keeps the reference's order per element (C, B, D products subtracted in turn, IEEE division) and a value
    depends on nothing else, so it equals numpy's fp32 run of the same recurrence."""
    r = runs[run]
    diff = int((r['got']['Y'] != r['Y32']).sum())
    print('%s: %d of %d elements differ from the fp32 recurrence' % (_ids(run), diff, r['Y32'].size))
    assert diff == 0


@pytest.mark.parametrize('run', RUNS, ids=_ids)
def test_backward_against_the_reference(golden, runs, run):
    tag, d, with_d = run
    r = runs[run]
    for k in OUTPUTS[1:]:
        ref = r['ref'][k]
        if ref is None:
            assert k == 'gD' and not with_d and k not in r['got']
            continue
        got = r['got'][k]
        assert got.shape == ref.shape, k
        if ref.size == 0:
            continue
        bound = 8 * _noise(golden('triag'), k, tag, d, with_d) * np.abs(ref).max()
        err = np.abs(got - ref).max()
        print('%s %s: err %.3e bound %.3e' % (_ids(run), k, err, bound))
        assert np.isfinite(got).all() and err <= bound, k


@pytest.mark.parametrize('upper', [0, 1])
def test_gradients_against_finite_differences_of_the_restatement(golden, upper):
    """Central differences in float64 on the restatement's loss sum(gY * J^-1 X) -- not on the kernel -- at every
    parameter of a (1,1,5,6) grid; step 1e-6, so the differences carry ~1e-9 of their own error."""
    from arflow_amd import triag_solve as T
    case = R.make_case(1, 1, 5, 6)
    t = {k: torch.from_numpy(v).cuda().requires_grad_(k != 'gY') for k, v in case.items()}
    fn = T.BackwardSubst if upper else T.ForwardSubst
    fn.apply(t['A'], t['B'], t['C'], t['D'], t['X']).backward(t['gY'])
    p64 = {k: v.astype(np.float64) for k, v in case.items()}

    def loss(p):
        return float((p['gY'] * R.solve(p['A'], p['B'], p['C'], p['D'], p['X'], bool(upper))).sum())
    h = 1e-6
    g = golden('triag')
    for k in 'ABCDX':
        fd = np.zeros_like(p64[k])
        for idx in np.ndindex(*fd.shape):
            hi, lo = dict(p64), dict(p64)
            hi[k], lo[k] = p64[k].copy(), p64[k].copy()
            hi[k][idx] += h
            lo[k][idx] -= h
            fd[idx] = (loss(hi) - loss(lo)) / (2 * h)
        got = t[k].grad.cpu().numpy()
        bound = 8 * _noise(g, 'g' + k, '-', '-', False) * np.abs(fd).max() + 1e-8
        print('upper %d d%s: err %.3e bound %.3e' % (upper, k, np.abs(got - fd).max(), bound))
        assert np.abs(got - fd).max() <= bound, k


@pytest.mark.parametrize('tag', list(R.DIAG_CASES))
def test_inverse_diagonal_against_the_reference(golden, tag):
    from arflow_amd import functional as AF, triag_solve as T
    g = golden('triag')
    A, B, C = [g['%s_diag_%s' % (k, tag)].cuda() for k in 'ABC']
    before = [x.clone() for x in (A, B, C)]
    K, L, M, N = A.shape
    H = torch.full_like(A, float('nan'))
    AF._call('arflow_triag_inverse_diagonal', AF._p(A), AF._p(B), AF._p(C), AF._p(H), K * L, M, N, AF._stream())
    ref = g.raw('H_diag_' + tag)
    rel = np.abs(H.cpu().numpy() - ref) / ref
    bound = 8 * float(g.raw('noise_H_diag_' + tag))
    print('%s: rel err %.3e bound %.3e' % (tag, rel.max(), bound))
    assert np.isfinite(rel).all() and rel.max() <= bound
    H2 = T.inverse_diagonal(A.requires_grad_(True), B, C)
    assert not H2.requires_grad and torch.equal(H2, H)
    with AF.deterministic():
        assert torch.equal(T.inverse_diagonal(A.detach(), B, C), H)
    assert all(torch.equal(x.detach(), y) for x, y in zip((A, B, C), before))


@pytest.mark.parametrize('run', RUNS, ids=_ids)
def test_launch_hygiene(runs, run):
    """Every output element is stored (NaN-filled buffers into the raw calls), two runs agree bit for bit with and without
    deterministic mode, and the inputs are untouched."""
    from arflow_amd import functional as AF
    tag, d, with_d = run
    r = runs[run]
    t, upper = r['t'], int(d == 'up')
    for mode in (False, True):
        with AF.deterministic(mode):
            Y = _raw_solve(t, upper)
            grads = _raw_bwd(t, Y, upper)
        assert torch.equal(Y, r['Ydev']), mode
        assert not torch.isnan(Y).any()
        for k, v in grads.items():
            if v is None:
                assert k == 'gD' and not with_d
                continue
            assert not torch.isnan(v).any(), (k, mode)
            assert np.array_equal(v.cpu().numpy(), r['got'][k]), (k, mode)
    for k, v in r['before'].items():
        assert torch.equal(t[k], v), k


def test_plain_functions_and_layout_checks(runs):
    from arflow_amd import triag_solve as T
    r = runs['odd', 'lo', True]
    t = r['t']
    Y = T.forward_substitution(t['A'], t['B'], t['C'], t['D'], t['X'])
    assert not Y.requires_grad and torch.equal(Y, r['Ydev'])
    up = runs['odd', 'up', False]
    assert torch.equal(T.backward_substitution(t['A'], t['B'], t['C'], None, t['X']), up['Ydev'])
    # J Y = X through the ATen compositions users check residuals with
    res = (T.matrix_vector_product(t['A'], t['B'], t['C'], t['D'], Y) - t['X']).abs().max()
    assert float(res) <= 1e-5
    res = (T.matrix_vector_product_T(t['A'], t['B'], t['C'], None, up['Ydev']) - t['X']).abs().max()
    assert float(res) <= 1e-5
    with pytest.raises(ValueError, match='^X must be contiguous'):
        T.forward_substitution(t['A'], t['B'], t['C'], t['D'], t['X'].transpose(2, 3).contiguous().transpose(2, 3))
    with pytest.raises(ValueError, match='^A must be float32'):
        T.inverse_diagonal(t['A'].double(), t['B'], t['C'])
    with pytest.raises(ValueError, match='^B must be'):
        T.BackwardSubst.apply(t['A'], t['C'], t['C'], t['D'], t['X'])


def test_reparam_triag_inv_repeats_and_sums_over_samples():
    from arflow_amd import triag_solve as T
    case = R.make_case(2, 2, 9, 12)
    mean = torch.from_numpy(case['gY']).cuda().requires_grad_(True)
    co = [torch.from_numpy(case[k]).cuda().requires_grad_(True) for k in 'ABCD']
    eps = torch.randn(4, 2, 9, 12, generator=torch.Generator().manual_seed(3)).cuda()
    w = torch.randn(4, 2, 9, 12, generator=torch.Generator().manual_seed(4)).cuda()
    z = T.reparam_triag_inv(mean, *co, nsamples=2, eps=eps)
    rep = [c.detach().repeat(2, 1, 1, 1).requires_grad_(True) for c in co]
    want = mean.detach().repeat(2, 1, 1, 1) + T.BackwardSubst.apply(*rep, eps)
    assert z.shape == (4, 2, 9, 12) and torch.equal(z, want)
    (z * w).sum().backward()
    (want * w).sum().backward()
    assert torch.equal(mean.grad, w[:2] + w[2:])
    for c, r_, name in zip(co, rep, 'ABCD'):
        # the sum of the two samples' gradients: two terms, so the order of the sum cannot matter
        assert torch.equal(c.grad, r_.grad[:2] + r_.grad[2:]), name
    # eps drawn on the device: right shape, finite, and different between calls
    z1 = T.reparam_triag_inv(mean.detach(), *[c.detach() for c in co], nsamples=3)
    z2 = T.reparam_triag_inv(mean.detach(), *[c.detach() for c in co], nsamples=3)
    assert z1.shape == (6, 2, 9, 12) and z1.is_cuda and bool(torch.isfinite(z1).all()) and not torch.equal(z1, z2)
    z3 = T.reparam_triag_inv(mean.detach(), co[0].detach(), co[1].detach(), co[2].detach(), None, nsamples=1, eps=eps[:2])
    assert torch.equal(z3, mean.detach() + T.backward_substitution(co[0].detach(), co[1].detach(), co[2].detach(), None,
                                                                   eps[:2].contiguous()))
