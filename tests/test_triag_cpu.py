"""CPU: the sparse triangular solves (csrc/triag.hip, arflow_amd/triag_solve.py) -- the float64 restatement of
tests/triag_ref.py reproduces what the reference's own code computed for the fixture (tests/golden/triag.npz,
tools/make_triag_golden.py) and agrees with numpy.linalg on the dense matrix; the entry points are exported and bound and
validate their arguments before any launch; the Python layer rejects what it cannot run.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import triag_ref as R

NEW = ['arflow_triag_solve', 'arflow_triag_solve_bwd', 'arflow_triag_inverse_diagonal']
ENULL, ESHAPE, EPARAM = -1001, -1002, -1003
OUTPUTS = ('Y', 'gX', 'gA', 'gB', 'gC', 'gD')


@pytest.fixture(scope='module')
def lib():
    from arflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _rel(got, want):
    want = np.asarray(want)
    if want.size == 0:
        assert np.shape(got) == want.shape
        return 0.0
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---- the restatement is pinned to the reference ------------------------------------------------------------------
@pytest.mark.parametrize('tag', list(R.SOLVE_CASES))
def test_restatement_reproduces_the_reference_solves(golden, tag):
    g = golden('triag')
    case = R.make_case(*R.SOLVE_CASES[tag])
    for k, v in case.items():
        assert np.array_equal(g.raw('%s_%s' % (k, tag)), v), k  # the seeded inputs are the fixture's
    for d, upper in (('lo', False), ('up', True)):
        Y = R.solve(case['A'], case['B'], case['C'], case['D'], case['X'], upper)
        got = dict(R.grads(case['A'], case['B'], case['C'], case['D'], Y, case['gY'], upper), Y=Y)
        for k in OUTPUTS:
            want = g.raw('%s_%s_%s' % (k, d, tag))
            assert want.dtype == np.float64 and got[k].shape == want.shape, (k, d)
            assert _rel(got[k], want) <= 1e-12, (k, d, _rel(got[k], want))
            noise = float(g.raw('noise_%s_%s_%s' % (k, d, tag)))
            assert 0.0 <= noise <= 2.5e-7, (k, d, noise)  # the reference's own fp32 run against its float64 run


@pytest.mark.parametrize('tag', list(R.DIAG_CASES))
def test_restatement_reproduces_the_reference_marginal_variances(golden, tag):
    g = golden('triag')
    case = R.make_case(*R.DIAG_CASES[tag])
    for k in 'ABC':
        assert np.array_equal(g.raw('%s_diag_%s' % (k, tag)), case[k]), k
    want = g.raw('H_diag_' + tag)
    H = R.inverse_diagonal(case['A'], case['B'], case['C'])
    assert float((np.abs(H - want) / want).max()) <= 1e-12
    assert 0.0 < float(g.raw('noise_H_diag_' + tag)) <= 2.9e-7
    if tag == 'small':  # the golden values are the diagonal of (J J^T)^-1
        dense = R.inverse_diagonal_dense(case['A'], case['B'], case['C'])
        assert float((np.abs(dense - want) / want).max()) <= 1e-13


def test_golden_file_holds_arrays_only(golden):
    z = golden('triag')._z
    assert all(z[k].dtype.kind == 'f' for k in z.files)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', 'triag.npz')) < 1 << 20


# ---- loops against the dense matrix --------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 2, 5, 6), (2, 1, 1, 7), (1, 1, 7, 1), (1, 1, 1, 1)])
@pytest.mark.parametrize('upper', [False, True])
@pytest.mark.parametrize('with_d', [True, False])
def test_dense_path_agrees_with_loop_path(shape, upper, with_d):
    c = R.make_case(*shape)
    D = c['D'] if with_d else None
    Y = R.solve(c['A'], c['B'], c['C'], D, c['X'], upper)
    assert _rel(Y, R.solve_dense(c['A'], c['B'], c['C'], D, c['X'], upper)) <= 1e-13
    assert _rel(R.matvec(c['A'], c['B'], c['C'], D, Y, upper), c['X'].astype(np.float64)) <= 1e-13
    # the gradients against the dense adjoint: gX = J^-T gY, dJ = -gX Y^T read at the stored entries
    g = R.grads(c['A'], c['B'], c['C'], D, Y, c['gY'], upper)
    assert _rel(g['gX'], R.solve_dense(c['A'], c['B'], c['C'], D, c['gY'], not upper)) <= 1e-13
    K, L, M, N = shape
    for (k, l), (a, b, cc, d, y, gx) in R._planes(c['A'], c['B'], c['C'], D, Y, g['gX']):
        dJ = -np.outer(gx.ravel(), y.ravel())
        # d sum(gY * J^-1 X) / d theta = sum(dJ * dJ/dtheta): perturb each coefficient array by ones to pick its entries
        for name, arrs in (('gA', (np.ones_like(a), 0 * b, 0 * cc, None if d is None else 0 * d)),
                           ('gB', (0 * a, np.ones_like(b), 0 * cc, None if d is None else 0 * d)),
                           ('gC', (0 * a, 0 * b, np.ones_like(cc), None if d is None else 0 * d)),
                           ('gD', (0 * a, 0 * b, 0 * cc, None if d is None else np.ones_like(d)))):
            if g[name] is None:
                assert name == 'gD' and D is None
                continue
            mask = R.dense(*arrs, upper=upper) != 0
            picked = np.sort(dJ[mask])
            assert picked.size == g[name][k, l].size
            assert np.allclose(picked, np.sort(g[name][k, l].ravel()), rtol=1e-12, atol=1e-14), name


def test_dense_inverse_diagonal_agrees_with_loop_path():
    c = R.make_case(1, 2, 4, 5)
    H = R.inverse_diagonal(c['A'], c['B'], c['C'])
    assert _rel(H, R.inverse_diagonal_dense(c['A'], c['B'], c['C'])) <= 1e-13


def test_make_case_distributions():
    c = R.make_case(2, 3, 17, 23)
    assert all(v.dtype == np.float32 and v.flags['C_CONTIGUOUS'] for v in c.values())
    assert c['A'].min() > 0 and all(np.abs(c[k]).max() <= 0.3 for k in 'BCD')
    assert np.array_equal(c['A'], R.make_case(2, 3, 17, 23)['A'])  # seeded


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound(lib):
    from arflow_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), '..', '..', 'include', 'arflow_hip.h')).read()
    for n in NEW:
        assert hasattr(raw, n), n
        assert n in _lib.PROTOTYPES, n
        assert n + '(' in header, n
    assert lib.arflow_abi_version() == 10  # additive change


one = ctypes.c_void_p(16)


def _solve(lib, **kw):
    a = dict(A=one, B=one, C=one, D=one, X=one, Y=one, P=1, M=4, N=4, upper=0)
    a.update(kw)
    return lib.arflow_triag_solve(a['A'], a['B'], a['C'], a['D'], a['X'], a['Y'], a['P'], a['M'], a['N'], a['upper'], None)


def _bwd(lib, **kw):
    a = dict(A=one, B=one, C=one, D=one, Y=one, gY=one, gX=one, gA=one, gB=one, gC=one, gD=one, P=1, M=4, N=4, upper=0)
    a.update(kw)
    return lib.arflow_triag_solve_bwd(*[a[k] for k in ('A', 'B', 'C', 'D', 'Y', 'gY', 'gX', 'gA', 'gB', 'gC', 'gD', 'P', 'M',
                                                        'N', 'upper')], None)


def _diag(lib, **kw):
    a = dict(A=one, B=one, C=one, H=one, P=1, M=4, N=4)
    a.update(kw)
    return lib.arflow_triag_inverse_diagonal(a['A'], a['B'], a['C'], a['H'], a['P'], a['M'], a['N'], None)


def test_argument_errors_without_gpu(lib):
    # validation happens before any launch, so these are safe on a CPU-only host
    for fn, required in ((_solve, 'ABCXY'), (_bwd, ('A', 'B', 'C', 'Y', 'gY', 'gX', 'gA', 'gB', 'gC', 'gD')),
                         (_diag, 'ABCH')):
        for k in required:
            assert fn(lib, **{k: None}) == ENULL, (fn.__name__, k)
        for k in 'PMN':
            assert fn(lib, **{k: 0}) == ESHAPE, (fn.__name__, k)
            assert fn(lib, **{k: -2}) == ESHAPE, (fn.__name__, k)
        assert fn(lib, M=16385) == ESHAPE and fn(lib, N=8193) == ESHAPE  # the limits stated in the header
        assert fn(lib, A=None, M=0) == ENULL  # pointers first, then shapes, then parameters
    for fn in (_solve, _bwd):
        for upper in (2, -1):
            assert fn(lib, upper=upper) == EPARAM, (fn.__name__, upper)
        assert fn(lib, M=0, upper=2) == ESHAPE
    assert _bwd(lib, D=None) == EPARAM         # gD without D
    assert _diag(lib, P=1 << 20, M=64, N=64) == ESHAPE  # one workgroup per source pixel: P M N < 2^31


# ---- the Python layer ------------------------------------------------------------------------------------------------
def _tensors(dtype=torch.float32, K=1, L=2, M=4, N=5):
    return (torch.ones(K, L, M, N, dtype=dtype), torch.zeros(K, L, M, N - 1, dtype=dtype),
            torch.zeros(K, L, M - 1, N, dtype=dtype), torch.zeros(K, L, M - 1, N - 1, dtype=dtype),
            torch.ones(K, L, M, N, dtype=dtype))


def test_python_layer_refuses_cpu_tensors_loudly():
    from arflow_amd import _lib, triag_solve as T
    A, B, C, D, X = _tensors()
    for fn in (T.forward_substitution, T.backward_substitution, T.ForwardSubst.apply, T.BackwardSubst.apply):
        with pytest.raises(_lib.ArflowHipError):
            fn(A, B, C, D, X)
        with pytest.raises(_lib.ArflowHipError):
            fn(A, B, C, None, X)
    with pytest.raises(_lib.ArflowHipError):
        T.inverse_diagonal(A, B, C)
    with pytest.raises(_lib.ArflowHipError):
        T.reparam_triag_inv(X, A, B, C, D, nsamples=2)


class _OnGpu(torch.Tensor):
    """A CPU tensor that claims to be on the GPU, so that the checks behind the device check run on a CPU-only host (they
    all raise before anything is launched)."""
    is_cuda = True

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        return super().__torch_function__(func, types, args, kwargs)


def _fake(t):
    return t.as_subclass(_OnGpu)


def test_python_layer_names_the_bad_argument():
    from arflow_amd import triag_solve as T
    A, B, C, D, X = [_fake(t) for t in _tensors()]
    with pytest.raises(ValueError, match=r'^X must be float32'):
        T.forward_substitution(A, B, C, D, _fake(_tensors(torch.float64)[4]))
    with pytest.raises(ValueError, match=r'^A must be float32'):
        T.inverse_diagonal(_fake(_tensors(torch.float64)[0]), B, C)
    with pytest.raises(ValueError, match=r'^B must be \(1, 2, 4, 4\)'):
        T.backward_substitution(A, _fake(torch.zeros(1, 2, 4, 5)), C, D, X)
    with pytest.raises(ValueError, match=r'^C must be \(1, 2, 3, 5\)'):
        T.ForwardSubst.apply(A, B, _fake(torch.zeros(1, 2, 4, 5)), D, X)
    with pytest.raises(ValueError, match=r'^D must be \(1, 2, 3, 4\)'):
        T.BackwardSubst.apply(A, B, C, _fake(torch.zeros(1, 2, 3, 5)), X)
    with pytest.raises(ValueError, match=r'^X must be \(1, 2, 4, 5\)'):
        T.forward_substitution(A, B, C, None, _fake(torch.ones(2, 2, 4, 5)))
    with pytest.raises(ValueError, match=r'^A must be \[K,L,M,N\]'):
        T.inverse_diagonal(_fake(torch.ones(4, 5)), B, C)
    with pytest.raises(ValueError, match=r'^X must be contiguous'):
        T.forward_substitution(A, B, C, D, _fake(torch.ones(1, 2, 5, 4).transpose(2, 3)))


def test_matrix_vector_products_are_the_operator_and_its_transpose():
    from arflow_amd import triag_solve as T
    c = R.make_case(2, 2, 5, 6)
    t = {k: torch.from_numpy(v).double() for k, v in c.items()}
    for D in (t['D'], None):
        Dn = None if D is None else c['D']
        lo = T.matrix_vector_product(t['A'], t['B'], t['C'], D, t['X']).numpy()
        up = T.matrix_vector_product_T(t['A'], t['B'], t['C'], D, t['X']).numpy()
        assert _rel(lo, R.matvec(c['A'], c['B'], c['C'], Dn, c['X'], False)) <= 1e-15
        assert _rel(up, R.matvec(c['A'], c['B'], c['C'], Dn, c['X'], True)) <= 1e-15
        # <J x, g> = <x, J^T g>
        g = t['gY']
        assert abs(float((torch.from_numpy(lo) * g).sum() -
                         (t['X'] * T.matrix_vector_product_T(t['A'], t['B'], t['C'], D, g)).sum())) <= 1e-12
