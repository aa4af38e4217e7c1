"""Shared by the triangular-solve tests and tools/make_triag_golden.py: the seeded input recipe, and a float64
restatement of what arflow_triag_solve, arflow_triag_solve_bwd and arflow_triag_inverse_diagonal compute (include/
arflow_hip.h; utils/triag_solve.py:76-115, 163-218 of the reference), once as substitution loops over the grid and once
through the dense MN x MN matrix and numpy.linalg for grids small enough.  Everything here is numpy on [K,L,M,N] arrays.

The operator, lower form (upper = False):   (J y)[i,j] = A[i,j] y[i,j] + B[i,j-1] y[i,j-1] + C[i-1,j] y[i-1,j]
                                                        + D[i-1,j-1] y[i-1,j-1]
upper form (upper = True), its transpose:   (J y)[i,j] = A[i,j] y[i,j] + B[i,j] y[i,j+1] + C[i,j] y[i+1,j]
                                                        + D[i,j] y[i+1,j+1]
"""
import numpy as np

# the grids of tests/golden/triag.npz: solves with both gradients, and marginal variances
SOLVE_CASES = {'strip': (1, 2, 70, 37), 'wide': (2, 1, 3, 130), 'tall': (1, 3, 130, 5), 'row': (1, 1, 1, 9),
               'col': (1, 1, 9, 1)}
DIAG_CASES = {'small': (1, 2, 9, 11), 'tall': (1, 2, 66, 5), 'wide': (1, 2, 3, 70)}


def make_case(K, L, M, N, seed=11):
    """Diagonally dominant, so the conditioning is bounded: A = exp(0.4 N(0,1)), B, C, D ~ U(-0.3, 0.3); right-hand side X
    and output gradient gY ~ N(0,1).  -> dict of float32 arrays A [K,L,M,N], B [K,L,M,N-1], C [K,L,M-1,N],
    D [K,L,M-1,N-1], X, gY [K,L,M,N]."""
    rng = np.random.default_rng([seed, K, L, M, N])
    out = {'A': np.exp(0.4 * rng.standard_normal((K, L, M, N)))}
    for name, shape in (('B', (K, L, M, N - 1)), ('C', (K, L, M - 1, N)), ('D', (K, L, M - 1, N - 1))):
        out[name] = rng.uniform(-0.3, 0.3, shape)
    out['X'] = rng.standard_normal((K, L, M, N))
    out['gY'] = rng.standard_normal((K, L, M, N))
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def _f64(*arrays, dtype=np.float64):
    return [None if a is None else np.asarray(a, dtype=dtype) for a in arrays]


def _flip(a):
    return None if a is None else a[..., ::-1, ::-1]


def solve(A, B, C, D, X, upper=False, dtype=np.float64):
    """Y = J^-1 X by substitution, float64.  The upper form is the lower form on the grid turned by 180 degrees: every
    array flipped in both axes (a flipped B, C, D then holds each coefficient at its neighbour's index, as the lower form
    reads them).  Per element: subtract the C, the B, then the D product, divide -- with dtype=np.float32 every product,
    difference and quotient is rounded to fp32 in that order, which is the arithmetic csrc/triag.hip states for itself."""
    A, B, C, D, X = _f64(A, B, C, D, X, dtype=dtype)
    if upper:
        return _flip(solve(_flip(A), _flip(B), _flip(C), _flip(D), _flip(X), dtype=dtype))
    M, N = A.shape[-2:]
    Y = np.zeros_like(X)
    for i in range(M):
        for j in range(N):
            acc = X[..., i, j].copy()
            if i:
                acc -= C[..., i - 1, j] * Y[..., i - 1, j]
            if j:
                acc -= B[..., i, j - 1] * Y[..., i, j - 1]
            if i and j and D is not None:
                acc -= D[..., i - 1, j - 1] * Y[..., i - 1, j - 1]
            Y[..., i, j] = acc / A[..., i, j]
    return Y


def matvec(A, B, C, D, X, upper=False):
    """J X, float64."""
    A, B, C, D, X = _f64(A, B, C, D, X)
    if upper:
        return _flip(matvec(_flip(A), _flip(B), _flip(C), _flip(D), _flip(X)))
    Y = A * X
    Y[..., :, 1:] += B * X[..., :, :-1]
    Y[..., 1:, :] += C * X[..., :-1, :]
    if D is not None:
        Y[..., 1:, 1:] += D * X[..., :-1, :-1]
    return Y


def grads(A, B, C, D, Y, gY, upper=False):
    """The gradients of sum(gY * J^-1 X) for the solve of direction `upper` whose result was Y: with gX = J^-T gY,
    d/dJ[a,b] = -gX[a] Y[b] at every stored entry of J.  -> dict gX, gA, gB, gC, gD (None without D), float64."""
    Y, gY = _f64(Y, gY)
    gX = solve(A, B, C, D, gY, upper=not upper)
    if upper:  # entry (a, b) = (pixel, its right / lower / lower-right neighbour), coefficient stored at the pixel
        g = {'gB': -gX[..., :, :-1] * Y[..., :, 1:], 'gC': -gX[..., :-1, :] * Y[..., 1:, :],
             'gD': -gX[..., :-1, :-1] * Y[..., 1:, 1:]}
    else:      # entry (a, b) = (pixel, its left / upper / upper-left neighbour), coefficient stored at the neighbour
        g = {'gB': -gX[..., :, 1:] * Y[..., :, :-1], 'gC': -gX[..., 1:, :] * Y[..., :-1, :],
             'gD': -gX[..., 1:, 1:] * Y[..., :-1, :-1]}
    if D is None:
        g['gD'] = None
    g.update(gX=gX, gA=-gX * Y)
    return g


def inverse_diagonal(A, B, C):
    """H[.., k, l] = |J^-1 e_(k,l)|^2 for the lower form without D, float64: one substitution sweep with all M N unit
    vectors as right-hand sides at once."""
    A, B, C = _f64(A, B, C)
    M, N = A.shape[-2:]
    E = np.eye(M * N).reshape(M * N, M, N)
    lead = A.shape[:-2]
    Y = solve(A[..., None, :, :], B[..., None, :, :], C[..., None, :, :], None, np.broadcast_to(E, lead + E.shape))
    return np.square(Y).sum((-2, -1)).reshape(lead + (M, N))


# ---- through the dense matrix ---------------------------------------------------------------------------------
def dense(A, B, C, D, upper=False):
    """The MN x MN matrix of one plane (A [M,N] ...), rows and columns in row-major pixel order."""
    A, B, C, D = _f64(A, B, C, D)
    M, N = A.shape
    J = np.zeros((M * N, M * N))
    for i in range(M):
        for j in range(N):
            p = i * N + j
            J[p, p] = A[i, j]
            if j:
                J[p, p - 1] = B[i, j - 1]
            if i:
                J[p, p - N] = C[i - 1, j]
            if i and j and D is not None:
                J[p, p - N - 1] = D[i - 1, j - 1]
    return J.T.copy() if upper else J


def _planes(*arrays):
    """[K,L,m,n] arrays -> per plane tuples of [m,n] arrays (None stays None)."""
    K, L = arrays[0].shape[:2]
    for k in range(K):
        for l in range(L):
            yield (k, l), tuple(None if a is None else a[k, l] for a in arrays)


def solve_dense(A, B, C, D, X, upper=False):
    Y = np.zeros(np.shape(X))
    for kl, (a, b, c, d, x) in _planes(*_f64(A, B, C, D, X)):
        Y[kl] = np.linalg.solve(dense(a, b, c, d, upper), x.ravel()).reshape(x.shape)
    return Y


def inverse_diagonal_dense(A, B, C):
    H = np.zeros(np.shape(A))
    for kl, (a, b, c) in _planes(*_f64(A, B, C)):
        J = dense(a, b, c, None)
        H[kl] = np.diag(np.linalg.inv(J @ J.T)).reshape(a.shape)
    return H
