"""GPU: the banded operator and the fused sampler (csrc/band.hip, arflow_amd/triag_solve.py) against the restatement of
tests/elbo_ref.py, which the CPU tests pin to what the reference's own code computed (tests/golden/elbo.npz).

Forward: EQUAL to the restatement run in fp32 with the reference's operation order (products rounded, added in tap order
onto zero, then added to the mean) -- the kernel states that it keeps that order.
Backward: every element of gX, gA = (gdiag, goff) and gmean against float64 under (terms + 2) 2^-24 sum|term|, the sum of
the absolute terms taken from the restatement on absolute values: one rounding per product, one per addition, and two to
spare; an element with no term on the grid must be exactly 0.  terms = (k + 1)^2 for gX, S for gA and gmean.

Grids (elbo_ref.GRIDS): 1 x 1; 2 x 3, smaller than the band both ways; 17 x 23; 8 x 33 and 9 x 32, one column wider and one
row taller than the kernel's 8 x 32 tile, so the halo crosses a tile edge in each axis -- for every k and both orientations,
B = 2 with S = 1 and 3, and B = 3 with S = 1.  Coefficients and mean are channel slices of wider tensors, Y is written into
channels 2:4 of a 4-channel tensor, and every output is pre-filled with NaN through the raw entry points."""
import numpy as np
import pytest
import torch

from tests import elbo_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BS = ((2, 1), (2, 3), (3, 1))
RUNS = [(tag, k) for tag in R.GRIDS for k in range(4)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _wide(c, k):
    """The case's coefficients and mean as channel slices of wider tensors: batch strides that are not C M N."""
    n2 = 2 * ((k + 1) ** 2 - 1)
    B, _, M, N = c['diag'].shape
    wide = torch.full((B, n2 + 5, M, N), float('nan')).cuda()
    wide[:, 1:3], wide[:, 3:3 + n2] = _dev(c['diag']), _dev(c['off'])
    wm = torch.full((B, 3, M, N), float('nan')).cuda()
    wm[:, 1:3] = _dev(c['mean'])
    return wm[:, 1:3], wide[:, 1:3], (wide[:, 3:3 + n2] if k else None)


def _raw_fwd(mean, diag, off, X, B, S, M, N, k, transpose):
    """-> the [S B,4,M,N] NaN-filled tensor whose channels 2:4 the launch wrote."""
    from arflow_amd import functional as AF
    buf = torch.full((S * B, 4, M, N), float('nan')).cuda()
    Y = buf[:, 2:4]
    AF._call('arflow_band_mv_fwd', AF._p(mean), 0 if mean is None else mean.stride(0), AF._p(diag), diag.stride(0),
             AF._p(off), 0 if off is None else off.stride(0), AF._p(X), X.stride(0), AF._p(Y), Y.stride(0), B, S, M, N, k,
             transpose, AF._stream())
    return buf


def _raw_bwd(diag, off, X, gY, B, S, M, N, k, transpose):
    from arflow_amd import functional as AF
    n2 = 2 * ((k + 1) ** 2 - 1)
    nan = lambda *s: torch.full(s, float('nan')).cuda()  # noqa: E731
    gXb, gA, gmean = nan(S * B, 3, M, N), nan(B, n2 + 3, M, N), nan(B, 2, M, N)
    gX, gdiag, goff = gXb[:, 1:3], gA[:, 0:2], (gA[:, 3:3 + n2] if k else None)
    AF._call('arflow_band_mv_bwd', AF._p(diag), diag.stride(0), AF._p(off), 0 if off is None else off.stride(0), AF._p(X),
             X.stride(0), AF._p(gY), gY.stride(0), AF._p(gX), gX.stride(0), AF._p(gmean), gmean.stride(0), AF._p(gdiag),
             gdiag.stride(0), AF._p(goff), 0 if goff is None else goff.stride(0), B, S, M, N, k, transpose, AF._stream())
    untouched = bool(torch.isnan(gXb[:, 0]).all()) and bool(torch.isnan(gA[:, 2]).all())
    return {'gX': gX, 'gdiag': gdiag, 'goff': goff, 'gmean': gmean}, untouched


def _reference(c, k, S, transpose):
    """fp32 forward in the reference's order; float64 gradients and their sums of absolute terms."""
    y32 = R.sampler(c['mean'], c['diag'], c['off'], c['X'], k, S, transpose, dtype=np.float32)
    names = ('gmean', 'gdiag', 'goff', 'gX')
    g64 = dict(zip(names, R.sampler_grads(c['diag'], c['off'], c['X'], c['gY'], k, S, transpose)))
    ab = {key: np.abs(v) for key, v in c.items()}
    mag = dict(zip(names, R.sampler_grads(ab['diag'], ab['off'], ab['X'], ab['gY'], k, S, transpose)))
    terms = {'gmean': S, 'gdiag': S, 'goff': S, 'gX': (k + 1) ** 2}
    return y32, g64, {key: (terms[key] + 2) * U * mag[key] for key in names}


@pytest.mark.parametrize('tag,k', RUNS, ids=['%s-k%d' % r for r in RUNS])
def test_forward_bits_backward_bounds_and_hygiene(tag, k):
    from arflow_amd import functional as AF
    M, N = R.GRIDS[tag]
    for B, S in BS:
        c = R.make_band_case(B, S, M, N, k)
        mean, diag, off = _wide(c, k)
        X, gY = _dev(c['X']), _dev(c['gY'])
        for transpose in (0, 1):
            y32, g64, bound = _reference(c, k, S, bool(transpose))
            what = '%s k%d B%d S%d T%d' % (tag, k, B, S, transpose)
            buf = _raw_fwd(mean, diag, off, X, B, S, M, N, k, transpose)
            assert bool(torch.isnan(buf[:, 0:2]).all()), what      # nothing outside its channels
            got = buf[:, 2:4].cpu().numpy()
            assert np.array_equal(got, y32), '%s: %d of %d elements differ from the fp32 run' % (
                what, int((got != y32).sum()), y32.size)
            nomean = _raw_fwd(None, diag, off, X, B, S, M, N, k, transpose)[:, 2:4].cpu().numpy()
            assert np.array_equal(nomean, R.sampler(None, c['diag'], c['off'], c['X'], k, S, bool(transpose), np.float32)), what
            grads, untouched = _raw_bwd(diag, off, X, gY, B, S, M, N, k, transpose)
            assert untouched, what
            for key, ref in g64.items():
                if key == 'goff' and not k:
                    assert grads[key] is None
                    continue
                g = grads[key].cpu().numpy().astype(np.float64)
                assert g.shape == ref.shape and np.isfinite(g).all(), (what, key)
                over = np.abs(g - ref) - bound[key]
                print('%s %s: max err %.3e, max err / bound %.3f' % (
                    what, key, np.abs(g - ref).max(), (np.abs(g - ref) / np.maximum(bound[key], 1e-300)).max()))
                assert (over <= 0).all(), (what, key, float(over.max()))
            # two runs agree bit for bit, and so does deterministic mode
            for mode in (False, True):
                with AF.deterministic(mode):
                    again = _raw_fwd(mean, diag, off, X, B, S, M, N, k, transpose)
                    g2, _ = _raw_bwd(diag, off, X, gY, B, S, M, N, k, transpose)
                assert torch.equal(again[:, 2:4], buf[:, 2:4]), (what, mode)
                for key, v in grads.items():
                    assert v is None or torch.equal(v, g2[key]), (what, key, mode)
        # inputs untouched
        assert np.array_equal(diag.cpu().numpy(), c['diag']) and np.array_equal(X.cpu().numpy(), c['X'])


@pytest.mark.parametrize('k', [0, 1, 3])
def test_autograd_operators_against_the_fixture(golden, k):
    """matrix_vector_product[_T]_general on the 5 x 7 grid of the fixture: Y equal to the fp32 run, gA and gX within the
    derived bound of what the reference's own autograd gave in float64."""
    from arflow_amd import triag_solve as T
    g = golden('elbo')
    M, N = R.SMALL
    c = R.make_band_case(2, 1, M, N, k)
    A64 = np.concatenate((c['diag'], c['off']), 1)
    for name, fn, transpose in (('mv', T.matrix_vector_product_general, False), ('mvT', T.matrix_vector_product_T_general, True)):
        A, X = _dev(A64).requires_grad_(True), _dev(c['X']).requires_grad_(True)
        Y = fn(A, X, k=k)
        Y.backward(_dev(c['gY']))
        assert np.array_equal(Y.detach().cpu().numpy(), R.product(A64, c['X'], k, transpose, np.float32))
        magA, magX = R.product_grads(np.abs(A64), np.abs(c['X']), np.abs(c['gY']), k, transpose)
        for key, got, mag, terms in (('gA', A.grad, magA, 1), ('gX', X.grad, magX, (k + 1) ** 2)):
            ref = g.raw('%s_%s_small_k%d' % (key, name, k))
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            assert (err <= (terms + 2) * U * mag).all(), (name, key, float(err.max()))
        assert np.abs(Y.detach().cpu().numpy() - g.raw('Y_%s_small_k%d' % (name, k))).max() <= \
            ((k + 1) ** 2 + 2) * U * R.product(np.abs(A64), np.abs(c['X']), k, transpose).max()


@pytest.mark.parametrize('k', [0, 3])
def test_reparam_triag_equals_the_composition_at_one_sample(k):
    """reparam_triag with S = 2 == mean.repeat + matrix_vector_product_general(A.repeat, eps) composed from the new
    operators at S = 1, bit for bit; its gradients are the two samples' sums (two terms: the order cannot matter)."""
    from arflow_amd import triag_solve as T
    B, S, M, N = 2, 2, 9, 35
    c = R.make_band_case(B, S, M, N, k)
    leaf = lambda a: _dev(a).requires_grad_(True)  # noqa: E731
    mean, diag, off, eps, w = leaf(c['mean']), leaf(c['diag']), leaf(c['off']), _dev(c['X']), _dev(c['gY'])
    z = T.reparam_triag(mean, diag, off if k else None, k, nsamples=S, eps=eps)
    Arep = torch.cat((diag.detach(), off.detach()), 1).repeat(S, 1, 1, 1).requires_grad_(True)
    want = mean.detach().repeat(S, 1, 1, 1) + T.matrix_vector_product_general(Arep, eps, k=k)
    assert z.shape == (S * B, 2, M, N) and torch.equal(z, want)
    (z * w).sum().backward()
    (want * w).sum().backward()
    assert torch.equal(mean.grad, w[:B] + w[B:])
    gA = Arep.grad[:B] + Arep.grad[B:]
    assert torch.equal(diag.grad, gA[:, :2])
    if k:
        assert torch.equal(off.grad, gA[:, 2:])
    # out=: written in place into a channel slice, no graph; eps drawn on the device when not given
    buf = torch.full((S * B, 4, M, N), float('nan')).cuda()
    out = T.reparam_triag(mean, diag, off if k else None, k, nsamples=S, eps=eps, out=buf[:, 0:2])
    assert torch.equal(buf[:, 0:2], z) and bool(torch.isnan(buf[:, 2:4]).all()) and not out.requires_grad
    pair = T.reparam_triag_pair((mean, diag, off, eps), (mean, diag, off, eps), k, S)
    assert pair.shape == (S * B, 4, M, N) and torch.equal(pair[:, 0:2], z) and torch.equal(pair[:, 2:4], z)
    nomean = T.reparam_triag(None, diag, off if k else None, k, nsamples=S, eps=eps, out=buf[:, 2:4])
    assert torch.equal(nomean, T.reparam_triag(None, diag.detach(), off.detach() if k else None, k, nsamples=S, eps=eps))
    # a reduction over the samples sends a gradient expanded along the batch (stride 0) into the backward
    for t in (mean, diag, off):
        t.grad = None
    T.reparam_triag(mean, diag, off if k else None, k, nsamples=S, eps=eps).sum(0).sum().backward()
    ones = np.ones_like(c['X'])
    gm, gd, go, _ = R.sampler_grads(c['diag'], c['off'], c['X'], ones, k, S)
    mg = R.sampler_grads(np.abs(c['diag']), np.abs(c['off']), np.abs(c['X']), ones, k, S)
    assert np.array_equal(mean.grad.cpu().numpy(), gm)
    for got, ref, mag in ((diag.grad, gd, mg[1]),) + (((off.grad, go, mg[2]),) if k else ()):
        assert (np.abs(got.cpu().numpy().astype(np.float64) - ref) <= (S + 2) * U * mag).all()
    z1 = T.reparam_triag(mean.detach(), diag.detach(), off.detach() if k else None, k, nsamples=3)
    z2 = T.reparam_triag(mean.detach(), diag.detach(), off.detach() if k else None, k, nsamples=3)
    assert z1.shape == (3 * B, 2, M, N) and bool(torch.isfinite(z1).all()) and not torch.equal(z1, z2)


def test_layout_checks_name_the_argument():
    from arflow_amd import triag_solve as T
    c = R.make_band_case(2, 1, 5, 7, 1)
    A, X = _dev(np.concatenate((c['diag'], c['off']), 1)), _dev(c['X'])
    with pytest.raises(ValueError, match='^X must be contiguous or a channel slice'):
        T.matrix_vector_product_general(A, X.transpose(2, 3).contiguous().transpose(2, 3), k=1)
    with pytest.raises(ValueError, match='^A must be float32'):
        T.matrix_vector_product_T_general(A.double(), X, k=1)
    with pytest.raises(ValueError, match=r'^X must be \(2, 2, 5, 7\)'):
        T.matrix_vector_product_general(A, X[:, :, :4], k=1)
    with pytest.raises(ValueError, match=r'^offdiag must be \(2, 6, 5, 7\)'):
        T.reparam_triag(X, A[:, :2], A[:, 2:6], 1, eps=X)
    with pytest.raises(ValueError, match=r'^X must be \(4, 2, 5, 7\)'):
        T.reparam_triag(X, A[:, :2], A[:, 2:], 1, nsamples=2, eps=X)
