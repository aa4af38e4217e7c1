"""Sparse triangular solves on the pixel grid: the reference's ``utils/triag_solve.py`` on the native kernels of
csrc/triag.hip.  ``from arflow_amd.triag_solve import BackwardSubst`` replaces
``from utils.triag_solve import BackwardSubst``.

The operator J couples a pixel to three neighbours.  Tensors are [K,L,M,N]-shaped as in the reference's docstrings
(utils/triag_solve.py:76-81, :97-102): A [K,L,M,N] centre, B [K,L,M,N-1] left (upper form: right), C [K,L,M-1,N] above
(below), D [K,L,M-1,N-1] above-left (below-right) or None for zero.  Everything is fp32, contiguous and on the GPU: a CPU
tensor raises ArflowHipError, a wrong dtype, layout or shape raises ValueError naming the argument.
"""
import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .functional import _call, _p, _stream

__all__ = ['forward_substitution', 'backward_substitution', 'ForwardSubst', 'BackwardSubst', 'inverse_diagonal',
           'matrix_vector_product', 'matrix_vector_product_T', 'reparam_triag_inv']


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
