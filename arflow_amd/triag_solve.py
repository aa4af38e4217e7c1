"""Sparse triangular solves on the pixel grid: the reference's ``utils/triag_solve.py`` on the native kernels of
csrc/triag.hip.  ``from arflow_amd.triag_solve import BackwardSubst`` replaces
``from utils.triag_solve import BackwardSubst``.

The operator J couples a pixel to three neighbours.  Tensors are [K,L,M,N]-shaped as in the reference's docstrings
(utils/triag_solve.py:76-81, :97-102): A [K,L,M,N] centre, B [K,L,M,N-1] left (upper form: right), C [K,L,M-1,N] above
(below), D [K,L,M-1,N-1] above-left (below-right) or None for zero.  Everything is fp32, contiguous and on the GPU: a CPU
tensor raises ArflowHipError, a wrong dtype, layout or shape raises ValueError naming the argument.

The banded operator of the sparse-covariance family (utils/triag_solve.py:29-43, :59-73; csrc/band.hip, DESIGN.md section
21) lives here too: matrix_vector_product_general, matrix_vector_product_T_general and the fused sampler reparam_triag.
Their tensors may be channel slices of wider tensors (rows, planes and channels dense, any batch stride): they are passed to
the kernels in place.
"""
from functools import partial

import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._planes import check_planes, load_optional, plane_dense, save_optional
from .functional import _call, _p, _stream

__all__ = ['forward_substitution', 'backward_substitution', 'ForwardSubst', 'BackwardSubst', 'inverse_diagonal',
           'matrix_vector_product', 'matrix_vector_product_T', 'reparam_triag_inv', 'matrix_vector_product_general',
           'matrix_vector_product_T_general', 'reparam_triag', 'reparam_triag_pair']


def _check(**named):
    """named: A, B, C, then optionally D (may be None) and further [K,L,M,N] tensors -> (K, L, M, N)."""
    A = named['A']
    for name, t in named.items():
        if t is None and name == 'D':
            continue
        if not isinstance(t, torch.Tensor):
            raise ValueError('%s must be a tensor (got %s)' % (name, type(t).__name__))
        if not t.is_cuda:
            raise _lib.ArflowHipError('arflow_amd.triag_solve runs on the GPU only (%s is a %s tensor); there is no CPU '
                                      'fallback' % (name, t.device))
    if A.dim() != 4:
        raise ValueError('A must be [K,L,M,N] (got %s)' % (tuple(A.shape),))
    K, L, M, N = A.shape
    want = {'B': (K, L, M, N - 1), 'C': (K, L, M - 1, N), 'D': (K, L, M - 1, N - 1)}
    for name, t in named.items():
        if t is None and name == 'D':
            continue
        if t.dtype != torch.float32:
            raise ValueError('%s must be float32 (got %s)' % (name, t.dtype))
        if tuple(t.shape) != want.get(name, (K, L, M, N)):
            raise ValueError('%s must be %s for A %s (got %s)' % (name, want.get(name, (K, L, M, N)), tuple(A.shape),
                                                                   tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError('%s must be contiguous' % name)
        if t.device != A.device:
            raise ValueError('%s is on %s, A on %s' % (name, t.device, A.device))
    return K, L, M, N


def _solve(A, B, C, D, X, upper):
    K, L, M, N = _check(A=A, B=B, C=C, D=D, X=X)
    with torch.no_grad():
        Y = torch.empty_like(X)
        with torch.cuda.device_of(A):
            _call('arflow_triag_solve', _p(A), _p(B), _p(C), _p(D), _p(X), _p(Y), K * L, M, N, upper, _stream(),
                  key=(K * L, M, N, upper, D is not None))
    return Y


def _solve_bwd(A, B, C, D, Y, gY, upper):
    """-> gA, gB, gC, gD (None without D), gX: the order of the reference's backward (utils/triag_solve.py:181)."""
    K, L, M, N = A.shape
    gY = gY.contiguous()
    gX, gA, gB, gC = torch.empty_like(Y), torch.empty_like(A), torch.empty_like(B), torch.empty_like(C)
    gD = None if D is None else torch.empty_like(D)
    with torch.cuda.device_of(A):
        _call('arflow_triag_solve_bwd', _p(A), _p(B), _p(C), _p(D), _p(Y), _p(gY), _p(gX), _p(gA), _p(gB), _p(gC), _p(gD),
              K * L, M, N, upper, _stream(), key=(K * L, M, N, upper, D is not None))
    return gA, gB, gC, gD, gX


def forward_substitution(A, B, C, D, X):
    """Solves J y = x for the lower-triangular J (utils/triag_solve.py:76-94).  No autograd."""
    return _solve(A, B, C, D, X, 0)


def backward_substitution(A, B, C, D, X):
    """Solves J y = x for the upper-triangular J (utils/triag_solve.py:97-115).  No autograd."""
    return _solve(A, B, C, D, X, 1)


class ForwardSubst(Function):
    """utils/triag_solve.py:163-181; the backward is one launch of arflow_triag_solve_bwd."""

    @staticmethod
    def forward(ctx, A, B, C, D, X):
        Y = _solve(A, B, C, D, X, 0)
        ctx.save_for_backward(A, B, C, D, Y)
        return Y

    @staticmethod
    @once_differentiable
    def backward(ctx, dY):
        A, B, C, D, Y = ctx.saved_tensors
        return _solve_bwd(A, B, C, D, Y, dY, 0)


class BackwardSubst(Function):
    """utils/triag_solve.py:184-202; the backward is one launch of arflow_triag_solve_bwd."""

    @staticmethod
    def forward(ctx, A, B, C, D, X):
        Y = _solve(A, B, C, D, X, 1)
        ctx.save_for_backward(A, B, C, D, Y)
        return Y

    @staticmethod
    @once_differentiable
    def backward(ctx, dY):
        A, B, C, D, Y = ctx.saved_tensors
        return _solve_bwd(A, B, C, D, Y, dY, 1)


def inverse_diagonal(A, B, C):
    """H[k,l,i,j] = |J^-1 e_(i,j)|^2 for the lower-triangular J without D: the diagonal of (J J^T)^-1, the marginal
    variances when J is the Cholesky factor of a precision (marginal_variances, utils/triag_solve.py:205-218; the kernel
    of utils/triag_solve/triag_solve_cuda.cu:72-139).  The result does not require grad."""
    K, L, M, N = _check(A=A, B=B, C=C)
    with torch.no_grad():
        H = torch.empty_like(A)
        with torch.cuda.device_of(A):
            _call('arflow_triag_inverse_diagonal', _p(A), _p(B), _p(C), _p(H), K * L, M, N, _stream(), key=(K * L, M, N))
    return H


def matrix_vector_product(A, B, C, D, X):
    """J x for the lower-triangular J (utils/triag_solve.py:18-26); plain ATen, differentiable.  D may be None."""
    Y = A * X + F.pad(B * X[:, :, :, :-1], (1, 0)) + F.pad(C * X[:, :, :-1, :], (0, 0, 1, 0))
    return Y if D is None else Y + F.pad(D * X[:, :, :-1, :-1], (1, 0, 1, 0))


def matrix_vector_product_T(A, B, C, D, X):
    """J^T x, the upper-triangular form (utils/triag_solve.py:52-56); plain ATen, differentiable.  D may be None."""
    Y = A * X + F.pad(B * X[:, :, :, 1:], (0, 1)) + F.pad(C * X[:, :, 1:, :], (0, 0, 0, 1))
    return Y if D is None else Y + F.pad(D * X[:, :, 1:, 1:], (0, 1, 0, 1))


def reparam_triag_inv(mean, diag, left, over, leftover, nsamples=1, eps=None):
    """Reparameterised samples with mean `mean` and precision J^T J, J the upper-triangular operator (diag, left, over,
    leftover), as losses/uflow_elbo_loss.py:149-157 draws them: every argument is repeated nsamples times along the batch
    and z = mean + BackwardSubst(diag, left, over, leftover, eps); eps ~ N(0, 1) of the repeated mean's shape, drawn on
    the device when not given."""
    mean = mean.repeat(nsamples, 1, 1, 1)
    diag = diag.repeat(nsamples, 1, 1, 1)
    left = left.repeat(nsamples, 1, 1, 1)
    over = over.repeat(nsamples, 1, 1, 1)
    leftover = None if leftover is None else leftover.repeat(nsamples, 1, 1, 1)
    if eps is None:
        eps = torch.randn(mean.shape, device=mean.device, dtype=mean.dtype)
    return mean + BackwardSubst.apply(diag, left, over, leftover, eps)


# ---- the banded operator (csrc/band.hip) --------------------------------------------------------------------------
_check_band = partial(check_planes, __name__)  # the plane-layout rule (_planes.py) under this module's name


def _band_args(k, nsamples, mean, diag, off, X):
    """Checks one operator's tensors -> (B, S, M, N, strides of mean, diag, off, X)."""
    k, S = int(k), int(nsamples)
    if k not in (0, 1, 2, 3):
        raise ValueError('k must be 0..3 (got %r)' % (k,))
    if S < 1:
        raise ValueError('nsamples must be >= 1 (got %r)' % (nsamples,))
    if not isinstance(diag, torch.Tensor) or diag.dim() != 4:
        raise ValueError('diag must be a [B,2,M,N] tensor')
    B, _, M, N = diag.shape
    d_bs = _check_band('diag', diag, (B, 2, M, N))
    o_bs = _check_band('offdiag', off, (B, 2 * ((k + 1) ** 2 - 1), M, N)) if k > 0 else 0
    m_bs = 0 if mean is None else _check_band('mean', mean, (B, 2, M, N))
    x_bs = _check_band('X', X, (S * B, 2, M, N))
    for name, t in (('offdiag', off if k > 0 else None), ('mean', mean), ('X', X)):
        if t is not None and t.device != diag.device:
            raise ValueError('%s is on %s, diag on %s' % (name, t.device, diag.device))
    return B, S, M, N, m_bs, d_bs, o_bs, x_bs


def _band_fwd(k, S, transpose, mean, diag, off, X, Y):
    B, S, M, N, m_bs, d_bs, o_bs, x_bs = _band_args(k, S, mean, diag, off, X)
    y_bs = _check_band('out', Y, (S * B, 2, M, N))
    off = off if k > 0 else None
    with torch.cuda.device_of(diag):
        _call('arflow_band_mv_fwd', _p(mean), m_bs, _p(diag), d_bs, _p(off), o_bs, _p(X), x_bs, _p(Y), y_bs, B, S, M, N, int(k),
              int(transpose), _stream(), key=(B, S, M, N, int(k), int(transpose)))


def _band_bwd(k, S, transpose, diag, off, X, gY, want_gx, want_gmean, gA=None):
    """-> gmean (or None), gdiag, goff (None for k = 0), gX (or None).  gA: a [B,2(k+1)^2,M,N] tensor to store gdiag and goff
    into (its channels 0:2 and 2:), so that a whole-A gradient needs no cat."""
    B, S, M, N, _, d_bs, o_bs, x_bs = _band_args(k, S, None, diag, off, X)
    gY = plane_dense(gY, (S * B, 2, M, N))
    g_bs = _check_band('gY', gY, (S * B, 2, M, N))
    new = lambda n, c: torch.empty(n, c, M, N, device=diag.device, dtype=torch.float32)  # noqa: E731
    if gA is not None:
        gdiag, goff = gA[:, :2], (gA[:, 2:] if k > 0 else None)
    else:
        gdiag, goff = new(B, 2), (new(B, 2 * ((k + 1) ** 2 - 1)) if k > 0 else None)
    gd_bs = gdiag.stride(0) if B > 1 else 2 * M * N
    go_bs = 0 if goff is None else (goff.stride(0) if B > 1 else goff.shape[1] * M * N)
    gX = new(S * B, 2) if want_gx else None
    gmean = new(B, 2) if want_gmean else None
    off = off if k > 0 else None
    with torch.cuda.device_of(diag):
        _call('arflow_band_mv_bwd', _p(diag), d_bs, _p(off), o_bs, _p(X), x_bs, _p(gY), g_bs, _p(gX), 2 * M * N, _p(gmean),
              2 * M * N, _p(gdiag), gd_bs, _p(goff), go_bs, B, S, M, N, int(k), int(transpose), _stream(),
              key=(B, S, M, N, int(k), int(transpose)))
    return gmean, gdiag, goff, gX


class _BandProduct(Function):
    """Y = L X (transpose 0) or L^T X (1) with L = (A[:, :2], A[:, 2:]); one launch each way."""

    @staticmethod
    def forward(ctx, A, X, k, transpose):
        k = int(k)
        if k not in (0, 1, 2, 3):
            raise ValueError('k must be 0..3 (got %r)' % (k,))
        if not isinstance(A, torch.Tensor) or A.dim() != 4 or A.shape[1] != 2 * (k + 1) ** 2:
            raise ValueError('A must be a [K,%d,M,N] tensor for k = %d (got %s)' % (2 * (k + 1) ** 2, k, tuple(getattr(A, 'shape', ()))))
        _check_band('A', A, A.shape)
        _check_band('X', X, (A.shape[0], 2, A.shape[2], A.shape[3]))
        Y = torch.empty(X.shape, device=X.device, dtype=torch.float32)
        _band_fwd(k, 1, transpose, None, A[:, :2], A[:, 2:], X, Y)
        ctx.save_for_backward(A, X)
        ctx.cfg = (k, int(transpose))
        return Y

    @staticmethod
    @once_differentiable
    def backward(ctx, gY):
        A, X = ctx.saved_tensors
        k, transpose = ctx.cfg
        gA = torch.empty(A.shape, device=A.device, dtype=torch.float32)  # gdiag and goff are stored into its channel slices
        gX = _band_bwd(k, 1, transpose, A[:, :2], A[:, 2:], X, gY, ctx.needs_input_grad[1], False, gA=gA)[3]
        return gA, gX, None, None


def matrix_vector_product_general(A, X, k=1):
    """L x for the banded lower-triangular L of support k (utils/triag_solve.py:29-43): A [K,2(k+1)^2,M,N], X [K,2,M,N].
    Differentiable in A and X; the fp32 bits of the reference's composition."""
    return _BandProduct.apply(A, X, k, 0)


def matrix_vector_product_T_general(A, X, k=1):
    """L^T x (utils/triag_solve.py:59-73); as matrix_vector_product_general."""
    return _BandProduct.apply(A, X, k, 1)


class _Reparam(Function):
    """z = mean + L eps for `ndir` independent operators, S samples each, written side by side into ONE [S B, 2 ndir, M, N]
    tensor (direction d in channels 2d, 2d + 1): apply(k, S, ndir, mean_0, diag_0, off_0, eps_0, mean_1, ...).  One launch
    per direction each way; the coefficients are neither repeated nor concatenated."""

    @staticmethod
    def forward(ctx, k, S, ndir, *t):
        B, S, M, N = _band_args(k, S, *t[0:4])[:4]
        out = torch.empty(S * B, 2 * ndir, M, N, device=t[1].device, dtype=torch.float32)
        for d in range(ndir):
            mean, diag, off, eps = t[4 * d:4 * d + 4]
            _band_fwd(k, S, 0, mean, diag, off, eps, out[:, 2 * d:2 * d + 2])
        save_optional(ctx, t)
        ctx.cfg = (int(k), int(S), int(ndir))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        k, S, ndir = ctx.cfg
        t = load_optional(ctx)[0]
        grads = []
        for d in range(ndir):
            mean, diag, off, eps = t[4 * d:4 * d + 4]
            need = ctx.needs_input_grad[3 + 4 * d:3 + 4 * d + 4]
            gmean, gdiag, goff, geps = _band_bwd(k, S, 0, diag, off, eps, gout[:, 2 * d:2 * d + 2], need[3],
                                                 mean is not None and need[0])
            grads += [gmean, gdiag, goff, geps]
        return (None, None, None) + tuple(grads)


def reparam_triag(mean, diag, offdiag, k, nsamples=1, eps=None, out=None):
    """Reparameterised samples z = mean + L eps of the sparse-covariance family (losses/uflow_elbo_loss.py:142-147) in ONE
    launch: mean, diag [B,2,M,N], offdiag [B,2((k+1)^2-1),M,N] (None for k = 0), eps [nsamples B,2,M,N] ~ N(0,1), drawn on
    the device when not given; sample s of item b is plane s B + b.  k = 0 with diag = exp(log_diag) / exp(-log_diag) is
    reparam_diag / reparam_diag_inv (:118-140).  Gradients to mean, diag, offdiag (and eps).
    out: a [nsamples B,2,M,N] tensor or channel slice to write into; that call records no graph (use it under no_grad, or
    reparam_triag_pair for two directions side by side with gradients)."""
    if isinstance(diag, torch.Tensor) and diag.dim() == 4 and eps is None:
        B, _, M, N = diag.shape
        eps = torch.randn(int(nsamples) * B, 2, M, N, device=diag.device, dtype=diag.dtype)
    if out is not None:
        det = lambda t: t.detach() if isinstance(t, torch.Tensor) else t  # noqa: E731
        _band_fwd(k, nsamples, 0, det(mean), det(diag), det(offdiag), det(eps), out)
        return out
    return _Reparam.apply(k, nsamples, 1, mean, diag, offdiag if int(k) > 0 else None, eps)


def reparam_triag_pair(fw, bw, k, nsamples=1):
    """fw, bw: (mean, diag, offdiag, eps) of the two flow directions -> [nsamples B,4,M,N] with the forward samples in
    channels 0:2 and the backward samples in 2:4 -- the (fw, bw) layout the pair kernels of the losses take, written by the
    two launches directly (no cat)."""
    off = lambda o: o if int(k) > 0 else None  # noqa: E731
    return _Reparam.apply(k, nsamples, 2, fw[0], fw[1], off(fw[2]), fw[3], bw[0], bw[1], off(bw[2]), bw[3])
