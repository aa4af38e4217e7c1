"""Definitions shared by tools/make_mse_golden.py and the tests of MseLoss: the golden cases and their
seeded inputs, and a numpy float64 restatement of resize_flow (utils/flow_utils.py:110-118), of the fused sums and of the whole
loss (losses/mse_loss.py:9-148) with closed-form gradients, together with the per-element error bounds the kernel tests use.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests import triag_ref as T

EPS = 2.0 ** -24  # unit roundoff of fp32
OUTPUTS = ('total', 'mse', 'entropy', 'offdiag')
MODE_COV, MODE_INV, MODE_GIVEN = 0, 1, 2

# ---- golden cases: B = 2, level 6 x 10 -------------------------------------------------------------------------------------
GB, GH, GW = 2, 6, 10
_BASE = dict(type='mse', w_mse=1.0, w_entropy=0.1, diag_dominant=False, approx_entropy=False, offdiag_reg=1000.0)
CASES = {
    'A': dict(_BASE, diag=True, inv_cov=False, n_samples=1, align_corners=False, target=(24, 40)),
    'B': dict(_BASE, diag=True, inv_cov=True, n_samples=3, align_corners=True, target=(23, 37)),
    'C': dict(_BASE, diag=False, inv_cov=False, diag_dominant=True, n_samples=2, align_corners=False, target=(24, 40)),
    'D': dict(_BASE, diag=False, inv_cov=True, n_samples=2, align_corners=False, target=(24, 40)),
    'E': dict(_BASE, diag=False, inv_cov=True, approx_entropy=True, n_samples=1, align_corners=False, target=(24, 40)),
}


def case_cfg(tag):
    return {k: v for k, v in CASES[tag].items() if k != 'target'}


def make_inputs(tag, seed=2800):
    """-> {'net' [2,8,6,10], 'target' [2,2,H,W], 'eps' [S 2,2,6,10]} fp32: a mean of a pixel or so, log-diagonals around -1,
    off-diagonal coefficients within +-0.3 (a well-conditioned factor), a smooth target of a few pixels; multiples of 2^-7."""
    c = CASES[tag]
    rng = np.random.RandomState(seed + ord(tag))
    H, W = c['target']
    net = rng.randn(GB, 8, GH, GW)
    net[:, 2:4] = 0.5 * net[:, 2:4] - 1.0
    net[:, 4:8] = 0.6 * rng.rand(GB, 4, GH, GW) - 0.3
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing='ij')
    target = np.stack([np.stack([4.0 * np.sin(3 * xx + b) + yy, 3.0 * np.cos(2 * yy - b) + 2 * xx]) for b in range(GB)])
    target = target + 0.25 * rng.randn(GB, 2, H, W)
    eps = rng.randn(c['n_samples'] * GB, 2, GH, GW)
    q = lambda a: (np.round(a * 128) / 128).astype(np.float32)  # noqa: E731
    return dict(net=q(net), target=q(target), eps=q(eps))


# ---- resize_flow in float64 ---------------------------------------------------------------------------------------------------
def taps(n_in, n_out, align):
    """-> i0, i1 (int64 [n_out]) and lambda (float64): align False src = max(0, (d + 0.5) (n_in / n_out) - 0.5), align True
    src = d ((n_in - 1) / (n_out - 1)) (0 when n_out == 1); i0 = min(floor(src), n_in - 1), i1 = min(i0 + 1, n_in - 1)."""
    d = np.arange(n_out, dtype=np.float64)
    if align:
        src = d * ((n_in - 1) / (n_out - 1)) if n_out > 1 else np.zeros(n_out)
    else:
        src = np.maximum((d + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def _four(x, size, align):
    """The four taps of every output pixel and their weights: lists of four [..., h, w] arrays."""
    H, W = x.shape[-2:]
    h, w = size
    ya, yb, ly = taps(H, h, align)
    xa, xb, lx = taps(W, w, align)
    ly, lx = ly[:, None], lx[None, :]
    top, bot = x[..., ya, :], x[..., yb, :]
    vals = [top[..., xa], top[..., xb], bot[..., xa], bot[..., xb]]
    wts = [(1 - ly) * (1 - lx), (1 - ly) * lx, ly * (1 - lx), ly * lx]
    return vals, wts


def _reach(n_in, n_out, align, tol):
    """The source rows (columns) an fp32 coordinate within tol of the float64 one can blend: the two taps, and the next one
    outward where lambda lies within tol of 0 or of 1 (the floor may then fall on the other side of the integer)."""
    i0, i1, lam = taps(n_in, n_out, align)
    lo = np.where(lam < tol, np.maximum(i0 - 1, 0), i0)
    hi = np.where(lam > 1 - tol, np.minimum(i1 + 1, n_in - 1), i1)
    return [lo, i0, i1, hi]


def interpolate(x, size, align):
    """ATen's bilinear resize (no antialiasing) of [..., H, W] -> (out, bound), float64.
    bound = 6 u sum_i w_i |tap_i| + 4 u max(H, W) (max tap - min tap): the out_up rule of tests/gauss_pyr_ref.py -- on any
    path a tap passes the rounding of its two weights (1 - lambda), two products and two sums; the second term covers a
    source coordinate formed in fp32: an error of up to 2 u max(H, W) in lambda on each axis moves the blend by at most that
    times the spread of the taps.  Where the float64 coordinate lies within 4 u max(H, W) of an integer the fp32 one may floor
    to the neighbouring cell (ATen's own fp32 resize does, e.g. at the last row of 32 -> 8 with align_corners: 7 (31 / 7) <
    31), so there the spread is taken over that cell's tap as well (_reach); the blend is continuous across the integer, which
    is why the same term covers it."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    vals, wts = _four(x, size, align)
    out = sum(v * k for v, k in zip(vals, wts))
    mag = sum(np.abs(v) * k for v, k in zip(vals, wts))
    tol = 4 * EPS * max(H, W)
    near = [x[..., ys, :][..., xs] for ys in _reach(H, size[0], align, tol) for xs in _reach(W, size[1], align, tol)]
    spread = np.maximum.reduce(near) - np.minimum.reduce(near)
    return out, 6 * EPS * mag + 4 * EPS * max(H, W) * spread


def resize_flow(flow, size, align=False):
    """flow [B,2,H,W] -> (gt [B,2,h,w], bound), float64: the resize above, channel 0 divided by W / w and channel 1 by H / h.
    bound = the resize's bound divided by the scale, plus ONE rounding of the quotient: u (1 + 2^-28) |gt| (the kernel divides
    in float64 and rounds to fp32 once; 2^-28 covers the float64 quotient's own rounding under that final one)."""
    flow = np.asarray(flow, np.float64)
    H, W = flow.shape[-2:]
    h, w = size
    out, bound = interpolate(flow, size, align)
    scale = np.array([W / w, H / h]).reshape(1, 2, 1, 1)
    gt = out / scale
    return gt, bound / scale + EPS * (1 + 2.0 ** -28) * np.abs(gt)


# ---- the fused sums and their adjoint --------------------------------------------------------------------------------------------
def _rep(a, S):
    return np.tile(a, (S, 1, 1, 1))


def sums(net, target, ez, S, mode, align):
    """The four sums of arflow_mse_fwd in float64 and what the per-element bounds need.  ez: the noise (sampling modes) or the
    samples z (MODE_GIVEN).  -> dict: sums [4]; r, gt [S B,2,h,w]; part = std eps (sampling modes); delta = the bound on the
    fp32 residual r; bound0 = the bound on sums[0]:
      delta  = (bound of gt) + (z bound of the sampler: u |z| + 8 u |std eps|, tests/test_gauss_pyr_gpu.py; 0 for a given z,
               which is read, not computed) + u |r| (the rounding of the difference)
      bound0 = sum over the elements of 2 |r| delta + delta^2;  the accumulation itself is float64 (rtol 1e-12)."""
    net, ez = np.asarray(net, np.float64), np.asarray(ez, np.float64)
    h, w = net.shape[-2:]
    gt, gb = resize_flow(target, (h, w), align)
    gt, gb = _rep(gt, S), _rep(gb, S)
    mean, ld = net[:, 0:2], net[:, 2:4]
    if mode == MODE_GIVEN:
        z, part, zb = ez, None, 0.0
        left, over = net[:, 4:6, :, :-1], net[:, 6:8, :-1, :]
        s2, s3 = float((left * left).sum()), float((over * over).sum())
    else:
        std = np.exp(-ld if mode == MODE_INV else ld)
        part = _rep(std, S) * ez
        z = _rep(mean, S) + part
        zb = EPS * np.abs(z) + 8 * EPS * np.abs(part)
        s2 = s3 = 0.0
    r = z - gt
    delta = gb + zb + EPS * np.abs(r)
    return dict(sums=np.array([float((r * r).sum()), float(ld.sum()), s2, s3]), r=r, gt=gt, part=part, delta=delta,
                bound0=float((2 * np.abs(r) * delta + delta * delta).sum()))


def sums_grad(net, target, ez, S, mode, align, gsums):
    """The adjoint arflow_mse_bwd computes for the gradient gsums [4] of the sums, float64, with per-element bounds.
    With c = 2 gsums[0] and gz = c r:
      bound of gz   = |c| delta + 2 u |gz|                  (delta propagated; c rounded to fp32, the product rounded)
      sampling:  gmean = sum_s gz:        sum_s bound(gz) + (S - 1) u sum_s |gz|   (S - 1 fp32 additions)
                 glog_diag = sum_s gz (+- part) + gsums[1]:
                     sum_s (|part| bound(gz) + 8 u |gz part| + u |gz part|) + S u (sum_s |gz part| + |gsums[1]|) + u |gsums[1]|
                     (part carries the sampler's 8 u, each product is rounded, S additions, gsums[1] rounded to fp32)
      given z:   gnet[:, 2:4] = gsums[1] (one rounding), gnet[:, 4:8] = 2 gsums[2 / 3] (left, over): 2 u |.| (the factor and
                 the product rounded); gnet[:, 0:2] = 0 and the left-out column / row exactly."""
    f = sums(net, target, ez, S, mode, align)
    net = np.asarray(net, np.float64)
    B, C, h, w = net.shape
    c = 2.0 * gsums[0]
    gz = c * f['r']
    gzb = abs(c) * f['delta'] + 2 * EPS * np.abs(gz)
    gnet, bound = np.zeros(net.shape), np.zeros(net.shape)
    fold = lambda a: a.reshape(S, B, 2, h, w).sum(0)  # noqa: E731
    if mode == MODE_GIVEN:
        gnet[:, 2:4] = gsums[1]
        bound[:, 2:4] = EPS * abs(gsums[1])
        gnet[:, 4:6, :, :-1] = 2 * gsums[2] * net[:, 4:6, :, :-1]
        gnet[:, 6:8, :-1, :] = 2 * gsums[3] * net[:, 6:8, :-1, :]
        bound[:, 4:8] = 2 * EPS * np.abs(gnet[:, 4:8])
        return dict(gnet=gnet, bound=bound, gz=gz, gz_bound=gzb)
    part = f['part'] if mode == MODE_COV else -f['part']
    prod = gz * part
    gnet[:, 0:2] = fold(gz)
    bound[:, 0:2] = fold(gzb) + (S - 1) * EPS * fold(np.abs(gz))
    gnet[:, 2:4] = fold(prod) + gsums[1]
    bound[:, 2:4] = fold(np.abs(part) * gzb + 9 * EPS * np.abs(prod)) + S * EPS * (fold(np.abs(prod)) + abs(gsums[1])) \
        + EPS * abs(gsums[1])
    return dict(gnet=gnet, bound=bound, gz=None, gz_bound=None)


# ---- the whole loss --------------------------------------------------------------------------------------------------------------
def _pad_left(a):
    return np.pad(a, ((0, 0), (0, 0), (0, 0), (1, 0)))


def _pad_top(a):
    return np.pad(a, ((0, 0), (0, 0), (1, 0), (0, 0)))


def mse_loss(cfg, net, target, eps):
    """losses/mse_loss.py:60-148 in float64 with the given noise, the three names its text leaves unbound taken as the
    4-neighbour operators without D (tests/triag_ref.py) -> dict total, mse, entropy, offdiag (floats) and gnet = d total /
    d net in closed form."""
    net, eps = np.asarray(net, np.float64), np.asarray(eps, np.float64)
    B, C, h, w = net.shape
    S = int(cfg['n_samples'])
    diag, inv = bool(cfg['diag']), bool(cfg['inv_cov'])
    approx = (not diag) and inv and bool(cfg.get('approx_entropy', False))
    gt = _rep(resize_flow(target, (h, w), bool(cfg.get('align_corners', False)))[0], S)
    mean, ld = net[:, 0:2], net[:, 2:4]
    cm = float(cfg['w_mse']) / (S * B * 2 * h * w)
    ce = float(cfg['w_entropy']) / (B * h * w)
    fold = lambda a: a.reshape((S, B) + a.shape[1:]).sum(0)  # noqa: E731
    gnet = np.zeros(net.shape)
    offdiag = 0.0
    if diag:
        std = np.exp(-ld if inv else ld)
        part = _rep(std, S) * eps
        z = _rep(mean, S) + part
        gz = 2 * cm * (z - gt)
        gnet[:, 0:2] = fold(gz)
        gnet[:, 2:4] = fold(gz * (-part if inv else part))
    else:
        left, over = net[:, 4:6, :, :-1], net[:, 6:8, :-1, :]
        A = np.exp(ld)
        if cfg.get('diag_dominant', False):
            A = A + _pad_left(np.abs(left)) + _pad_top(np.abs(over))
        reg = float(cfg['offdiag_reg'])
        offdiag = reg * ((left * left).mean() + (over * over).mean()) / 2.0
        gleft, gover = reg * left / left.size, reg * over / over.size
        Ar, Lr, Or = _rep(A, S), _rep(left, S), _rep(over, S)
        if inv:
            Y = T.solve(Ar, Lr, Or, None, eps, upper=True)
            z = _rep(mean, S) + Y
            gz = 2 * cm * (z - gt)
            if approx:  # :127-130: S == 1; z - mean.detach() carries the gradient to the mean AND through the solve
                tmp = T.matvec(A, left, over, None, z - mean, upper=True)
                gz = gz + T.matvec(A, left, over, None, -ce * tmp, upper=False)
            g = T.grads(Ar, Lr, Or, None, Y, gz, upper=True)
            gA, gB, gC = fold(g['gA']), fold(g['gB']), fold(g['gC'])
        else:
            z = _rep(mean, S) + T.matvec(Ar, Lr, Or, None, eps)
            gz = 2 * cm * (z - gt)
            gA = fold(gz * eps)
            gB = fold(gz[..., :, 1:] * eps[..., :, :-1])
            gC = fold(gz[..., 1:, :] * eps[..., :-1, :])
        gnet[:, 0:2] = fold(gz)
        gnet[:, 2:4] = gA * np.exp(ld)
        gleft, gover = gleft + gB, gover + gC
        if cfg.get('diag_dominant', False):
            gleft = gleft + np.sign(left) * gA[..., :, 1:]
            gover = gover + np.sign(over) * gA[..., 1:, :]
        gnet[:, 4:6, :, :-1] = gleft
        gnet[:, 6:8, :-1, :] = gover
    mse = float(cfg['w_mse']) * float(((z - gt) ** 2).mean())
    if approx:
        entropy = float(cfg['w_entropy']) * float((tmp * tmp / 2).sum(1).mean())
    else:
        entropy = (-1.0 if inv else 1.0) * float(cfg['w_entropy']) * float(ld.sum(1).mean())
        gnet[:, 2:4] -= (-ce if inv else ce)
    return dict(total=mse - entropy + offdiag, mse=mse, entropy=entropy, offdiag=offdiag, gnet=gnet)


# ---- the kernel tests' shapes: (B, S, (h, w), (H, W)) ------------------------------------------------------------------------------
SHAPES = [(1, 1, (1, 1), (1, 1)), (2, 3, (3, 5), (12, 20)), (2, 2, (8, 12), (32, 48)), (2, 3, (5, 7), (23, 31)),
          (1, 2, (6, 9), (4, 5)), (1, 1, (40, 52), (160, 208))]


def kernel_inputs(shape, C=8):
    """Seeded fp32 inputs of one kernel-test shape: net [B,C,h,w] (log-diagonals around -0.5), target [B,2,H,W] of a few pixels,
    noise and given samples [S B,2,h,w], and the gradient of the four sums."""
    B, S, (h, w), (H, W) = shape
    rng = np.random.RandomState(1000 * h + 10 * w + S)
    net = rng.randn(B, C, h, w)
    net[:, 2:4] = 0.75 * net[:, 2:4] - 0.5
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    return dict(net=f32(net), target=f32(3.0 * rng.randn(B, 2, H, W)), eps=f32(rng.randn(S * B, 2, h, w)),
                z=f32(2.0 * rng.randn(S * B, 2, h, w)), gsums=rng.randn(4) / (S * B * 2 * h * w))
