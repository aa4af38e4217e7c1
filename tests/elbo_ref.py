"""Shared by the ELBO tests and tools/make_elbo_golden.py: the seeded input recipes, and a restatement in our own code of
what csrc/band.hip and arflow_amd/losses/uflow_elbo_loss.py compute (utils/triag_solve.py:29-43, :59-73 and losses/
uflow_elbo_loss.py:108-568 of the reference).

The banded operator (numpy, any dtype; A [K,2(k+1)^2,M,N], X [K,2,M,N], tap (i, j) has index ind = i (k + 1) + j and its
coefficient for channel c is channel 2 ind + c of A):
    plain        Y[y,x] = sum_ind A[ind,y-i,x-j] X[y-i,x-j]          transposed   Y[y,x] = sum_ind A[ind,y,x] X[y+i,x+j]
with the terms added in ind order onto zeros, each product rounded first -- with dtype=np.float32 that is the arithmetic
of the reference's fp32 run and of the kernel.  `sampler` adds the repeat over S samples and the mean.
The loss is restated in torch (float64 by default) on the operators of oracle/ops.py, with autograd for its gradients.
"""
import numpy as np
import torch

from oracle import ops as O

# ---- the banded operator ------------------------------------------------------------------------------------------
# grids of the GPU tests: a single pixel; smaller than the band both ways; odd; one column wider / one row taller than the
# kernel's 8 x 32 tile (csrc/band.hip TH, TW), so the halo crosses a tile edge in each axis
TILE_H, TILE_W = 8, 32
GRIDS = {'one': (1, 1), 'tiny': (2, 3), 'odd': (17, 23), 'wider': (TILE_H, TILE_W + 1), 'taller': (TILE_H + 1, TILE_W)}
# grids of tests/golden/elbo.npz: (M, N) -> the k the reference's slicing can run (it needs M, N >= k); all outputs
GOLDEN_GRIDS = {'one': (0, 1), 'tiny': (0, 1, 2), 'small': (0, 1, 2, 3)}
SMALL = (5, 7)
# ... and Y, gX only (a k = 3 coefficient gradient of these grids is 200 kB of float64 each)
GOLDEN_BIG = ('odd', 'wider', 'taller')


def grid_shape(tag):
    return SMALL if tag == 'small' else GRIDS[tag]


def make_band_case(B, S, M, N, k, seed=21):
    """diag = exp(-1 + 0.3 N(0,1)), off-diagonals 0.1 N(0,1), mean 1.5 N(0,1); X and the output gradient gY ~ N(0,1).
    -> dict of float32 arrays mean, diag [B,2,M,N], off [B,2((k+1)^2-1),M,N], X, gY [S B,2,M,N]."""
    rng = np.random.default_rng([seed, B, S, M, N, k])
    n = (k + 1) ** 2 - 1
    out = {'mean': 1.5 * rng.standard_normal((B, 2, M, N)), 'diag': np.exp(-1 + 0.3 * rng.standard_normal((B, 2, M, N))),
           'off': 0.1 * rng.standard_normal((B, 2 * n, M, N)), 'X': rng.standard_normal((S * B, 2, M, N)),
           'gY': rng.standard_normal((S * B, 2, M, N))}
    return {key: np.ascontiguousarray(v, dtype=np.float32) for key, v in out.items()}


def _shift(a, i, j, sign):
    """b[y,x] = a[y - sign i, x - sign j], zero outside (sign +1: from the upper left; -1: from the lower right)."""
    out = np.zeros_like(a)
    M, N = a.shape[-2:]
    if i >= M or j >= N:
        return out
    if sign > 0:
        out[..., i:, j:] = a[..., :M - i, :N - j]
    else:
        out[..., :M - i, :N - j] = a[..., i:, j:]
    return out


def product(A, X, k, transpose=False, dtype=np.float64):
    """L X / L^T X; A [K,2(k+1)^2,M,N], X [K,2,M,N]."""
    A, X = np.asarray(A, dtype=dtype), np.asarray(X, dtype=dtype)
    Y = np.zeros_like(X)
    for i in range(k + 1):
        for j in range(k + 1):
            a = A[:, 2 * (i * (k + 1) + j):2 * (i * (k + 1) + j) + 2]
            if transpose:
                Y = Y + _valid(a * _shift(X, i, j, -1), i, j)
            else:
                Y = Y + _shift(a * X, i, j, +1)
    return Y


def _valid(a, i, j):
    """Zero where (y + i, x + j) leaves the grid (the coefficient there multiplies nothing; keeps a NaN/Inf out)."""
    out = np.zeros_like(a)
    M, N = a.shape[-2:]
    if i < M and j < N:
        out[..., :M - i, :N - j] = a[..., :M - i, :N - j]
    return out


def product_grads(A, X, gY, k, transpose=False, dtype=np.float64):
    """Gradients of sum(gY * product(A, X)): -> gA, gX."""
    A, X, gY = (np.asarray(t, dtype=dtype) for t in (A, X, gY))
    gX = product(A, gY, k, not transpose, dtype)
    gA = np.zeros_like(A)
    for i in range(k + 1):
        for j in range(k + 1):
            ind = i * (k + 1) + j
            if transpose:
                gA[:, 2 * ind:2 * ind + 2] = _valid(gY * _shift(X, i, j, -1), i, j)
            else:
                gA[:, 2 * ind:2 * ind + 2] = _valid(X * _shift(gY, i, j, -1), i, j)
    return gA, gX


def sampler(mean, diag, off, X, k, S, transpose=False, dtype=np.float64):
    """z[s B + b] = mean[b] + (L[b] X[s B + b]): the coefficients tiled S times along the batch, as the reference does."""
    A = np.concatenate((diag, off), 1) if k else np.asarray(diag)
    Y = product(np.tile(A, (S, 1, 1, 1)), X, k, transpose, dtype)
    return Y if mean is None else np.tile(np.asarray(mean, dtype=dtype), (S, 1, 1, 1)) + Y


def sampler_grads(diag, off, X, gY, k, S, transpose=False, dtype=np.float64):
    """-> gmean, gdiag, goff, gX of sum(gY * sampler(...)): the S samples' gradients summed in sample order."""
    A = np.concatenate((diag, off), 1) if k else np.asarray(diag)
    B = A.shape[0]
    gA, gX = product_grads(np.tile(A, (S, 1, 1, 1)), X, gY, k, transpose, dtype)
    fold = lambda g: sum(g[s * B:(s + 1) * B] for s in range(S))  # noqa: E731
    gA = fold(gA)
    return fold(np.asarray(gY, dtype=dtype)), gA[:, :2], gA[:, 2:], gX


# ---- the loss ---------------------------------------------------------------------------------------------------
class Cfg(dict):
    __getattr__ = dict.__getitem__


BASE = dict(type='uflow_elbo', edge_constant=150, edge_asymp=0.0, w_smooth=4.0, order_smooth=1, isotropic_smooth=False,
            penalty_smooth='charbonnier', closed_form_smooth=False, data_loss=['census'], data_weight=[1.0],
            data_penalty=['abs_robust_loss'], w_entropy=0.1, w_oof=0.0, w_occ=0.0, with_bk=True, approx='diag',
            n_components=1, cov_supp=0, inv_cov=False, approx_entropy=False, occ_type='sample', n_samples=1,
            offdiag_reg=0.0, natural_grad=False)
# the cases of tests/golden/elbo.npz: B = 2, 32 x 64 images, an 8 x 16 level 2
CASES = {
    'sparse3': dict(approx='sparse', cov_supp=3, n_samples=2, edge_asymp=0.01, offdiag_reg=0.01),
    'sparse1': dict(approx='sparse', cov_supp=1, n_samples=1),
    'diag': dict(n_samples=2, edge_asymp=0.01),
    'diag_inv': dict(inv_cov=True),
    'diag_approx_entropy': dict(approx_entropy=True),
    'diag_closed1': dict(closed_form_smooth=True, order_smooth=1, isotropic_smooth=True, edge_asymp=0.01),
    'diag_closed2': dict(closed_form_smooth=True, order_smooth=2, edge_asymp=0.01),
    'nobk_oof_occ': dict(with_bk=False, w_oof=0.5, w_occ=0.3, n_samples=2),
}
LOSS_B, LOSS_H, LOSS_W = 2, 32, 64
SCALARS = ('total', 'warp', 'smooth', 'entropy', 'oof')
OUTPUTS = SCALARS + ('flow12_2', 'occu_mask12', 'valid_mask12', 'gnet12', 'gnet21')


def case_cfg(tag):
    return Cfg(dict(BASE, **CASES[tag]))


def make_loss_case(tag, seed=31):
    """mean ~ 1.5 N(0,1), log_diag ~ -1 + 0.3 N(0,1), off-diagonals 0.1 N(0,1), images uniform, noise N(0,1).
    -> dict of float32 arrays net12, net21 [B,C,h,w], im1, im2 [B,3,H,W] (the same pair in every case), eps12, eps21
    [S B,2,h,w]."""
    cfg = case_cfg(tag)
    B, H, W = LOSS_B, LOSS_H, LOSS_W
    h, w = H // 4, W // 4
    k = cfg.cov_supp if cfg.approx == 'sparse' else 0
    n = (k + 1) ** 2 - 1
    rng = np.random.default_rng([seed, sorted(CASES).index(tag)])
    out = {}
    for name in ('net12', 'net21'):
        out[name] = np.concatenate((1.5 * rng.standard_normal((B, 2, h, w)), -1 + 0.3 * rng.standard_normal((B, 2, h, w)),
                                    0.1 * rng.standard_normal((B, 2 * n, h, w))), 1)
    shared = np.random.default_rng(seed)  # one image pair for all cases
    for name in ('im1', 'im2'):
        out[name] = shared.uniform(0, 1, (B, 3, H, W))
    for name in ('eps12', 'eps21'):
        out[name] = rng.standard_normal((cfg.n_samples * B, 2, h, w))
    return {key: np.ascontiguousarray(v, dtype=np.float32) for key, v in out.items()}


def _product_t(A, X, k):
    """product(A, X, k) in torch (differentiable)."""
    Y = torch.zeros_like(X)
    M, N = X.shape[-2:]
    for i in range(k + 1):
        for j in range(k + 1):
            ind = i * (k + 1) + j
            if i < M and j < N:
                p = A[:, 2 * ind:2 * ind + 2, :M - i, :N - j] * X[:, :, :M - i, :N - j]
                Y = Y + torch.nn.functional.pad(p, (j, 0, i, 0))
    return Y


def _charbonnier(x_sq, eps=0.001):
    return torch.sqrt(x_sq + eps ** 2)


def _edge_weights(cfg, im_small, stride):
    gx, gy = O.image_grads(im_small, stride)
    wx = cfg.edge_asymp + (1.0 - cfg.edge_asymp) * torch.exp(-(cfg.edge_constant * gx).abs().mean(1, keepdim=True))
    wy = cfg.edge_asymp + (1.0 - cfg.edge_asymp) * torch.exp(-(cfg.edge_constant * gy).abs().mean(1, keepdim=True))
    return wx, wy


def loss(cfg, case, dtype=torch.float64):
    """The loss of losses/uflow_elbo_loss.py:190-568 for the supported settings.  case: the arrays of make_loss_case.
    -> dict of numpy arrays: OUTPUTS (gnet12, gnet21: the gradients of `total`) and 'occ' (the occlusion penalty)."""
    t = {key: torch.from_numpy(np.asarray(v)).to(dtype) for key, v in case.items()}
    net12, net21 = t['net12'].requires_grad_(True), t['net21'].requires_grad_(True)
    S, B = cfg.n_samples, net12.shape[0]
    k = cfg.cov_supp if cfg.approx == 'sparse' else 0
    n = (k + 1) ** 2 - 1
    rep = lambda x: x.repeat(S, 1, 1, 1)  # noqa: E731

    def sample(net, eps):
        mean, log_diag, off = net[:, 0:2], net[:, 2:4], net[:, 4:4 + 2 * n]
        diag = torch.exp(-log_diag if (cfg.approx == 'diag' and cfg.inv_cov) else log_diag)
        z = rep(mean) + _product_t(rep(torch.cat((diag, off), 1)), eps, k)
        return z, mean, log_diag, diag, off

    f12, mean12, ld12, diag12, off12 = sample(net12, t['eps12'])
    f21, mean21, ld21, diag21, off21 = sample(net21, t['eps21'])
    im1, im2 = rep(t['im1']), rep(t['im2'])
    dirs = [(im1, im2, f12, f21, mean12, ld12, diag12, off12)]
    if cfg.with_bk:
        dirs.append((im2, im1, f21, f12, mean21, ld21, diag21, off21))

    warp = smooth = entropy = oof = occ = offdiag = 0.
    first = None
    for im_a, im_b, f_ab, f_ba, mean, ld, diag, off in dirs:
        # data term
        coords = O.flow_to_warp(O.upsample(f_ab, True, 4.0))
        recons = O.resample(im_b.detach(), coords)
        valid = O.mask_invalid(coords)
        occ_small = torch.clamp(O.compute_range_map(f_ba), 0., 1.)
        mask = (O.upsample(occ_small, False, 4.0) * valid).detach()
        warp = warp + cfg.data_weight[0] * O.census_loss(im_a, recons, mask)
        if first is None:
            first = (occ_small, valid)
        # entropy
        if cfg.approx == 'diag' and not cfg.inv_cov and cfg.approx_entropy:
            q = (f_ab - rep(mean).detach()) / rep(diag).detach()
            entropy = entropy + cfg.w_entropy * (q * q / 2).sum(1).mean()
        else:
            entropy = entropy + (-1. if cfg.inv_cov else 1.) * cfg.w_entropy * ld.sum(1).mean()
        # smoothness
        im_small = O.downsample(im_a[:B], False, 4.0)
        if not cfg.closed_form_smooth:
            wx, wy = _edge_weights(cfg, rep(im_small), 1)
            dx, dy = O.image_grads(f_ab)
            smooth = smooth + (wx / 2 * cfg.w_smooth * _charbonnier(dx ** 2)).mean() \
                + (wy / 2 * cfg.w_smooth * _charbonnier(dy ** 2)).mean()
        else:
            if cfg.order_smooth == 1:
                wx, wy = (v / 2 for v in _edge_weights(cfg, im_small, 1))
                Ex = (mean[..., 1:] - mean[..., :-1]) ** 2 + diag[..., 1:] ** 2 + diag[..., :-1] ** 2
                Ey = (mean[:, :, 1:] - mean[:, :, :-1]) ** 2 + diag[:, :, 1:] ** 2 + diag[:, :, :-1] ** 2
            else:
                wx, wy = _edge_weights(cfg, im_small, 2)
                Ex = (mean[..., :-2] - 2 * mean[..., 1:-1] + mean[..., 2:]) ** 2 \
                    + diag[..., :-2] ** 2 + 4 * diag[..., 1:-1] ** 2 + diag[..., 2:] ** 2
                Ey = (mean[:, :, :-2] - 2 * mean[:, :, 1:-1] + mean[:, :, 2:]) ** 2 \
                    + diag[:, :, :-2] ** 2 + 4 * diag[:, :, 1:-1] ** 2 + diag[:, :, 2:] ** 2
            if cfg.isotropic_smooth:  # [B,h,w'] against [B,1,h,w'] weights: every pair of samples, as the reference
                Ex, Ey = Ex.mean(1), Ey.mean(1)
            smooth = smooth + (wx * cfg.w_smooth * _charbonnier(Ex)).mean() + (wy * cfg.w_smooth * _charbonnier(Ey)).mean()
        # penalties
        if cfg.w_oof > 0:
            c2 = O.flow_to_warp(f_ab)
            hh, ww = f_ab.shape[2:]
            u = torch.clamp(c2[:, 0], max=0) ** 2 + torch.clamp(c2[:, 0] - float(ww - 1), min=0) ** 2
            v = torch.clamp(c2[:, 1], max=0) ** 2 + torch.clamp(c2[:, 1] - float(hh - 1), min=0) ** 2
            oof = oof + cfg.w_oof * (u + v).mean()
        if cfg.w_occ > 0:
            occ = occ + cfg.w_occ * (1 / (100.0 * occ_small + 1) * f_ab ** 2).mean()
        if cfg.approx == 'sparse':
            offdiag = offdiag + (off ** 2).mean()
    total = warp + smooth - entropy + oof + occ
    if cfg.approx == 'sparse':
        total = total + cfg.offdiag_reg * offdiag
    g12, g21 = torch.autograd.grad(total, (net12, net21))
    out = {'total': total, 'warp': warp, 'smooth': smooth, 'entropy': entropy, 'oof': oof, 'occ': occ, 'flow12_2': f12,
           'occu_mask12': first[0], 'valid_mask12': first[1], 'gnet12': g12, 'gnet21': g21}
    return {key: torch.as_tensor(v, dtype=dtype).detach().numpy() for key, v in out.items()}
