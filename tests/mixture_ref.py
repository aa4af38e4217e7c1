"""Shared by the mixture tests and tools/make_mixture_golden.py: the seeded input recipes, and a restatement in our own code of
what csrc/mixture.hip and the 'mixture' branch of arflow_amd/losses/uflow_elbo_loss.py compute (losses/uflow_elbo_loss.py
:159-178, :224-237, :307-311, :358-361 and utils/misc_utils.py:67-132 of the reference).  TEST INFRASTRUCTURE ONLY.

mean, log_std [B,2K,M,N]: channel 2k + c is flow component c of mixture component k; weights [B,K]; comp [B,S] in 0..K-1; eps
[S B,2,M,N].  Sample s of item b is row n = s B + b, z = comp[b,s], P = M N, std = exp(log_std).  numpy, float64:
    flow[n,c,p] = mean[b,2z+c,p] + std[b,2z+c,p] eps[n,c,p]
    d[n,k,c,p]  = (flow[n,c,p] - mean[b,2k+c,p]) / std[b,2k+c,p]
    A[n,k]      = -sum_p sum_c (log_std[b,2k+c,p] + d^2 / 2)
    logpdf[n]   = (max_k A + log sum_k w[b,k] exp(A[n,k] - max_k A)) / P
    r[n,k]      = w[b,k] e_k / sum_j w[b,j] e_j,   q[n,k] = e_k / sum_j w[b,j] e_j,   e_k = exp(A[n,k] - max_k A)
Gradients of  sum(gZ * flow) + sum(glogpdf * logpdf)  with lambda[n] = glogpdf[n] / P (the samples are not detached inside
logpdf) and G[n,c,p] = gZ[n,c,p] - lambda[n] sum_k r[n,k] d / std:
    gmean[b,2k+c,p]    = sum_s (lambda[n] r[n,k] d / std + [z == k] G[n,c,p])
    glog_std[b,2k+c,p] = sum_s (lambda[n] r[n,k] (d^2 - 1) + [z == k] G[n,c,p] std[b,2k+c,p] eps[n,c,p])
    gweights[b,k]      = sum_s glogpdf[n] q[n,k] / P

Magnitudes for the error bounds of tests/test_mixture_gpu.py (each is a sum of |terms|; the kernels' error is a small multiple
of 2^-24 times it).  The kernels form the sample in fp32 and everything after it in float64, with std and 1 / std from the
fp32 exponential (1 ulp = 2 * 2^-24 relative), and round each output once:
    fmag = |mean_z| + |std_z eps|                   the sample: |error| <= 4 * 2^-24 fmag (exp 2, product 1, sum 1)
    Amag[n,k] = sum_p sum_c (|log_std| + d^2 / 2 + |d| fmag / std)
                the last term is |dA / dflow| fmag: the density is evaluated at the fp32 sample, the restatement at its own
                float64 sample, and the difference (flow - mean_k) cancels: at most 4 * 2^-24 of it.  1 / std is within
                2 * 2^-24 (1 ulp of expf), so d^2 / 2 within 4 * 2^-24 of itself, log_std is exact, and the sums are float64
The gradients' magnitudes list every product that is summed, each with the same sample-rounding term (|d term / d flow| fmag).
The loss is restated in torch (float64) on the operators of oracle/ops.py, with autograd for its gradients.
"""
import numpy as np
import torch

from oracle import ops as O
from tests import elbo_ref as E

# csrc/mixture.hip: pixels one sampler workgroup reduces (CHUNK), and the largest number of components (KMAX)
CHUNK = 1024
KMAX = 4
EPS = 2.0 ** -24


# ---- the operators ------------------------------------------------------------------------------------------------
def make_case(B, S, K, M, N, comp='mixed', weights='uniform', seed=41):
    """Component means within ~std / sqrt(P) of a common base and log-stds within ~0.1 / sqrt(P) of a common one in [-2, 1], so
    that the responsibilities are not one-hot at any size; eps, gZ, glogpdf ~ N(0,1).  comp: 'equal' (one component for all
    samples) or 'mixed'; weights: 'uniform', 'nonuniform' or 'zero' (the last component's weight is exactly 0, and no sample
    is drawn from it -- multinomial would not either).  -> dict of arrays: float32 mean, log_std [B,2K,M,N], weights [B,K],
    eps, gZ [S B,2,M,N], glogpdf [S B]; int64 comp [B,S]."""
    rng = np.random.default_rng([seed, B, S, K, M, N, ['equal', 'mixed'].index(comp),
                                 ['uniform', 'nonuniform', 'zero'].index(weights)])
    P = M * N
    spread = min(1.0, 0.7 / np.sqrt(P))
    base_ls = rng.uniform(-1.9, 0.9, (B, 1, 2, M, N))
    log_std = np.clip(base_ls + spread * 0.1 * rng.standard_normal((B, K, 2, M, N)), -2.0, 1.0)
    base = 1.5 * rng.standard_normal((B, 1, 2, M, N))
    mean = base + spread * np.exp(base_ls) * rng.standard_normal((B, K, 2, M, N))
    if weights == 'uniform':
        w = np.full((B, K), 1.0 / K)
    else:
        w = rng.uniform(0.2, 1.0, (B, K))
        if weights == 'zero' and K > 1:
            w[:, K - 1] = 0.0
        w = w / w.sum(1, keepdims=True)
    top = K - 1 if (weights == 'zero' and K > 1) else K
    if comp == 'equal':
        z = np.full((B, S), min(1, top - 1), dtype=np.int64)
    else:
        z = (np.arange(B)[:, None] + np.arange(S)[None, :] + rng.integers(0, top)) % top
    out = {'mean': mean.reshape(B, 2 * K, M, N), 'log_std': log_std.reshape(B, 2 * K, M, N), 'weights': w,
           'eps': rng.standard_normal((S * B, 2, M, N)), 'gZ': rng.standard_normal((S * B, 2, M, N)),
           'glogpdf': rng.standard_normal(S * B)}
    out = {key: np.ascontiguousarray(v, dtype=np.float32) for key, v in out.items()}
    out['weights'][:, 0] += 1.0 - out['weights'].astype(np.float64).sum(1)  # rows sum to 1 to within one fp32 rounding
    out['comp'] = np.ascontiguousarray(z, dtype=np.int64)
    return out


def _rows(x, comp, S):
    """x [B,K,2,M,N], comp [B,S] -> the drawn component's planes per sample row n = s B + b: [S B,2,M,N]."""
    B = x.shape[0]
    return np.stack([x[b, comp[b, s]] for s in range(S) for b in range(B)])


def sampler(mean, log_std, comp, eps, S):
    """-> (flow [S B,2,M,N], fmag = |mean_z| + |std_z eps|) in float64."""
    mean, log_std, eps = (np.asarray(t, dtype=np.float64) for t in (mean, log_std, eps))
    B, C, M, N = mean.shape
    K = C // 2
    mz = _rows(mean.reshape(B, K, 2, M, N), comp, S)
    sz = np.exp(_rows(log_std.reshape(B, K, 2, M, N), comp, S))
    return mz + sz * eps, np.abs(mz) + np.abs(sz * eps)


def density(mean, log_std, weights, comp, eps, S):
    """-> dict: flow, fmag [S B,2,M,N]; d [S B,K,2,M,N]; A, Amag, resp, q [S B,K]; logpdf [S B]; x, xmag [S B,K,M,N] (the
    per-pixel exponents of the entropy map and their magnitudes)."""
    flow, fmag = sampler(mean, log_std, comp, eps, S)
    mean, log_std, weights = (np.asarray(t, dtype=np.float64) for t in (mean, log_std, weights))
    B, C, M, N = mean.shape
    K = C // 2
    mu = np.tile(mean.reshape(B, K, 2, M, N), (S, 1, 1, 1, 1))
    ls = np.tile(log_std.reshape(B, K, 2, M, N), (S, 1, 1, 1, 1))
    w = np.tile(weights, (S, 1))
    d = (flow[:, None] - mu) * np.exp(-ls)
    x = -(ls + d * d / 2).sum(2)
    xmag = (np.abs(ls) + d * d / 2 + np.abs(d) * fmag[:, None] * np.exp(-ls)).sum(2)
    A, Amag = x.sum((2, 3)), xmag.sum((2, 3))
    top = A.max(1, keepdims=True)
    e = np.exp(A - top)
    tot = (w * e).sum(1, keepdims=True)
    return {'flow': flow, 'fmag': fmag, 'd': d, 'A': A, 'Amag': Amag, 'logpdf': (top + np.log(tot))[:, 0] / (M * N),
            'resp': w * e / tot, 'q': e / tot, 'x': x, 'xmag': xmag, 'w': w}


def logpdf_bound(den, P):
    """8 * 2^-24 sum |terms| / P.  To first order the error of logpdf is sum_k r_k dA_k / P; the kernel's dA_k is at most
    4 * 2^-24 Amag_k (module docstring: 4 on the d^2 / 2 terms, 4 on the sample's rounding), which leaves the same again for
    the one rounding of the result, |logpdf| <= (sum_k r_k |A_k| + log K) / P."""
    return 8 * EPS * ((den['resp'] * den['Amag']).sum(1) + np.log(den['A'].shape[1]) + 1e-30) / P


def resp_bound(den, q=False):
    """The bound on A (8 * 2^-24 Amag) times the softmax sensitivities |dr_k / dA_j| = r_k |delta_kj - r_j|, summed over the
    components, plus 4 * 2^-24 (r <= 1 is rounded once to fp32).  q: the same for q_k = r_k / w_k (dq_k / dA_j = q_k (delta_kj -
    r_j); the rounding relative to q)."""
    r, dA = den['resp'], 8 * EPS * den['Amag']
    K = r.shape[1]
    val = den['q'] if q else r
    out = np.zeros_like(r)
    for k in range(K):
        for j in range(K):
            out[:, k] += val[:, k] * np.abs((1.0 if j == k else 0.0) - r[:, j]) * dA[:, j]
    return out + 4 * EPS * (np.maximum(val, 1.0) if q else 1.0)


def grads(mean, log_std, weights, comp, eps, gZ, glogpdf, S, rb=None):
    """gZ / glogpdf may be None.  -> dict: gmean, glog_std [B,2K,M,N], gweights [B,K] in float64; mag_mean, mag_ls, mag_w: the
    sums of the terms' magnitudes (module docstring); and, when rb [S B,K] (a bound on the responsibilities' error) is given,
    rs_mean, rs_ls = sum |d gradient / d r[n,j]| rb[n,j]."""
    den = density(mean, log_std, weights, comp, eps, S)
    mean, log_std = np.asarray(mean, dtype=np.float64), np.asarray(log_std, dtype=np.float64)
    B, C, M, N = mean.shape
    K, P = C // 2, M * N
    eps = np.asarray(eps, dtype=np.float64)
    gZ = np.zeros((S * B, 2, M, N)) if gZ is None else np.asarray(gZ, dtype=np.float64)
    g = np.zeros(S * B) if glogpdf is None else np.asarray(glogpdf, dtype=np.float64)
    lam = g / P
    inv = np.exp(-log_std.reshape(B, K, 2, M, N))
    std = np.exp(log_std.reshape(B, K, 2, M, N))
    r, d, fmag = den['resp'], den['d'], den['fmag']
    out = {k: np.zeros((B, K, 2, M, N)) for k in ('gmean', 'glog_std', 'mag_mean', 'mag_ls', 'rs_mean', 'rs_ls')}
    rb = np.zeros_like(r) if rb is None else rb
    for s in range(S):
        for b in range(B):
            n, z = s * B + b, int(comp[b, s])
            lr = (lam[n] * r[n])[:, None, None, None]          # [K,1,1,1]
            t1 = lr * d[n] * inv[b]                              # [K,2,M,N]
            t1_flow = np.abs(lr) * inv[b] ** 2 * fmag[n]         # |d t1 / d flow| fmag
            t1_r = np.abs(lam[n] * d[n] * inv[b]) * rb[n][:, None, None, None]
            G = gZ[n] - t1.sum(0)
            Gmag = np.abs(gZ[n]) + (np.abs(t1) + t1_flow).sum(0)
            se = std[b, z] * eps[n]
            out['gmean'][b] += t1
            out['mag_mean'][b] += np.abs(t1) + t1_flow
            out['rs_mean'][b] += t1_r
            out['glog_std'][b] += lr * (d[n] ** 2 - 1)
            out['mag_ls'][b] += np.abs(lr) * (d[n] ** 2 + 1 + 2 * np.abs(d[n]) * inv[b] * fmag[n])
            out['rs_ls'][b] += np.abs(lam[n] * (d[n] ** 2 - 1)) * rb[n][:, None, None, None]
            out['gmean'][b, z] += G
            out['mag_mean'][b, z] += Gmag
            out['rs_mean'][b, z] += t1_r.sum(0)
            out['glog_std'][b, z] += G * se
            out['mag_ls'][b, z] += Gmag * np.abs(se)
            out['rs_ls'][b, z] += t1_r.sum(0) * np.abs(se)
    out = {k: v.reshape(B, 2 * K, M, N) for k, v in out.items()}
    gq = g[:, None] * den['q'] / P
    out['gweights'] = gq.reshape(S, B, K).sum(0)
    out['mag_w'] = np.abs(gq).reshape(S, B, K).sum(0)
    out['den'] = den
    return out


def objective(mean, log_std, weights, comp, eps, gZ, glogpdf, S):
    """sum(gZ * flow) + sum(glogpdf * logpdf): what `grads` differentiates."""
    den = density(mean, log_std, weights, comp, eps, S)
    return (np.asarray(gZ, dtype=np.float64) * den['flow']).sum() + (np.asarray(glogpdf, dtype=np.float64) * den['logpdf']).sum()


def entropy_map(mean, log_std, weights, comp, eps, n):
    """mixture_entropy of utils/misc_utils.py:104-132 on recorded draws comp [B,n], eps [n B,2,M,N] -> (entropy [B,1,M,N], mag
    [B,1,M,N] = (1 / n) sum_i (sum_k r_k xmag_k + log K): to first order the error of one draw's log-sum is sum_k r_k dx_k)."""
    den = density(mean, log_std, weights, comp, eps, n)
    B, K = np.asarray(mean).shape[0], den['x'].shape[1]
    x, w = den['x'], den['w'][:, :, None, None]
    top = x.max(1, keepdims=True)
    e = w * np.exp(x - top)
    lse = (top + np.log(e.sum(1, keepdims=True)))[:, 0]
    rp = e / e.sum(1, keepdims=True)
    mag = (rp * den['xmag']).sum(1) + np.log(K) + 1e-30
    fold = lambda a: a.reshape(n, B, *a.shape[1:]).sum(0)[:, None] / n  # noqa: E731
    return -fold(lse), fold(mag)


# ---- the loss ---------------------------------------------------------------------------------------------------
BASE = dict(E.BASE, approx='mixture', n_components=2, w_entropy=0.3)
# the cases of tests/golden/elbo_mixture.npz: B = 2, 32 x 64 images, an 8 x 16 level 2
CASES = {
    'mix2': dict(n_components=2, n_samples=3),
    'mix3w': dict(n_components=3, n_samples=2, edge_asymp=0.01),
    'mix2_nobk': dict(n_components=2, n_samples=2, with_bk=False, w_oof=0.5, w_occ=0.3),
    'mix2_tie': dict(n_components=2, n_samples=2),
}
WEIGHTED = ('mix3w',)  # explicit weights_fw / weights_bw that require grad
LOSS_B, LOSS_H, LOSS_W = E.LOSS_B, E.LOSS_H, E.LOSS_W
SCALARS, OUTPUTS = E.SCALARS, E.OUTPUTS
TIE_FRACTION = 0.5  # mix2_tie: the second component's mean is the first's plus this times std / sqrt(P) times N(0,1)
ENTROPY_N = 5


def case_cfg(tag):
    return E.Cfg(dict(BASE, **CASES[tag]))


def case_outputs(tag):
    return OUTPUTS + (('gweights12', 'gweights21') if tag in WEIGHTED else ())


def make_loss_case(tag, seed=43):
    """means ~ 1.5 N(0,1) per component, log-stds -1 + 0.3 N(0,1) (mix2_tie: equal log-stds, means TIE_FRACTION std / sqrt(P)
    N(0,1) apart), images uniform, noise N(0,1), component draws mixed within every item.  -> dict of arrays: float32 net12,
    net21 [B,4K,h,w], im1, im2 [B,3,H,W] (the same pair in every case), eps12, eps21 [S B,2,h,w]; int64 comp12, comp21 [B,S];
    for the WEIGHTED cases float32 weights12, weights21 [B,K]."""
    cfg = case_cfg(tag)
    B, H, W = LOSS_B, LOSS_H, LOSS_W
    h, w = H // 4, W // 4
    K, S = cfg.n_components, cfg.n_samples
    rng = np.random.default_rng([seed, sorted(CASES).index(tag)])
    out = {}
    for name in ('net12', 'net21'):
        mean = 1.5 * rng.standard_normal((B, K, 2, h, w))
        ls = -1 + 0.3 * rng.standard_normal((B, K, 2, h, w))
        if tag == 'mix2_tie':
            ls[:, 1:] = ls[:, :1]
            mean[:, 1:] = mean[:, :1] + TIE_FRACTION * np.exp(ls[:, :1]) / np.sqrt(h * w) * rng.standard_normal((B, K - 1, 2, h, w))
        out[name] = np.concatenate((mean.reshape(B, 2 * K, h, w), ls.reshape(B, 2 * K, h, w)), 1)
    shared = np.random.default_rng(seed)  # one image pair for all cases
    for name in ('im1', 'im2'):
        out[name] = shared.uniform(0, 1, (B, 3, H, W))
    for name in ('eps12', 'eps21'):
        out[name] = rng.standard_normal((S * B, 2, h, w))
    if tag in WEIGHTED:
        for name in ('weights12', 'weights21'):
            wts = rng.uniform(0.2, 1.0, (B, K))
            out[name] = wts / wts.sum(1, keepdims=True)
    out = {key: np.ascontiguousarray(v, dtype=np.float32) for key, v in out.items()}
    for d, name in enumerate(('comp12', 'comp21')):
        out[name] = np.ascontiguousarray((np.arange(B)[:, None] + np.arange(S)[None, :] + d) % K, dtype=np.int64)
    return out


def make_entropy_case(seed=47):
    """The `entropy_map` case: mean, log_std [2,4,8,16] (K = 2), non-uniform weights, ENTROPY_N recorded draws."""
    c = make_case(2, ENTROPY_N, 2, 8, 16, comp='mixed', weights='nonuniform', seed=seed)
    return {k: c[k] for k in ('mean', 'log_std', 'weights', 'comp', 'eps')}


def log_pdf_t(flow, mean, log_std, weights):
    """gaussian_mixture_log_pdf (utils/misc_utils.py:72-101, per_pixel=False) in torch: flow [S B,2,h,w], mean, log_std
    [B,2K,h,w], weights [B,K] -> [S B]."""
    S = flow.shape[0] // mean.shape[0]
    B, C, h, w = mean.shape
    mu = mean.view(B, C // 2, 2, h, w).repeat(S, 1, 1, 1, 1)
    ls = log_std.view(B, C // 2, 2, h, w).repeat(S, 1, 1, 1, 1)
    d = (flow[:, None] - mu) * torch.exp(-ls)
    A = -(ls + d * d / 2).sum((2, 3, 4))
    top = A.max(1, keepdim=True)[0]
    return (top + torch.log((weights.repeat(S, 1) * torch.exp(A - top)).sum(1, keepdim=True)))[:, 0] / (h * w)


def sample_t(mean, log_std, comp, eps):
    """reparam_gmm (:159-178) in torch on recorded draws: comp [B,S] -> [S B,2,h,w]."""
    B, C, h, w = mean.shape
    S = comp.shape[1]
    mu, ls = mean.view(B, C // 2, 2, h, w), log_std.view(B, C // 2, 2, h, w)
    mz = torch.stack([mu[b, int(comp[b, s])] for s in range(S) for b in range(B)])
    lz = torch.stack([ls[b, int(comp[b, s])] for s in range(S) for b in range(B)])
    return mz + torch.exp(lz) * eps


def loss(cfg, case, dtype=torch.float64):
    """The 'mixture' loss of losses/uflow_elbo_loss.py:190-568.  case: the arrays of make_loss_case.  -> dict of numpy arrays:
    OUTPUTS (gnet12, gnet21: the gradients of `total`), 'occ' (the occlusion penalty), and gweights12, gweights21 when the case
    has weights."""
    t = {key: torch.from_numpy(np.asarray(v)) for key, v in case.items()}
    t = {key: (v if key.startswith('comp') else v.to(dtype)) for key, v in t.items()}
    net12, net21 = t['net12'].requires_grad_(True), t['net21'].requires_grad_(True)
    S, B, K = cfg.n_samples, net12.shape[0], cfg.n_components
    rep = lambda x: x.repeat(S, 1, 1, 1)  # noqa: E731
    has_w = 'weights12' in t
    if has_w:
        w12, w21 = t['weights12'].requires_grad_(True), t['weights21'].requires_grad_(True)
    else:
        w12 = w21 = torch.full((B, K), 1.0 / K, dtype=dtype)
    f12 = sample_t(net12[:, :2 * K], net12[:, 2 * K:], t['comp12'], t['eps12'])
    f21 = sample_t(net21[:, :2 * K], net21[:, 2 * K:], t['comp21'], t['eps21'])
    im1, im2 = rep(t['im1']), rep(t['im2'])
    dirs = [(im1, im2, f12, f21, net12, w12)]
    if cfg.with_bk:
        dirs.append((im2, im1, f21, f12, net21, w21))
    warp = smooth = entropy = oof = occ = 0.
    first = None
    for im_a, im_b, f_ab, f_ba, net, wts in dirs:
        coords = O.flow_to_warp(O.upsample(f_ab, True, 4.0))
        recons = O.resample(im_b.detach(), coords)
        valid = O.mask_invalid(coords)
        occ_small = torch.clamp(O.compute_range_map(f_ba), 0., 1.)
        mask = (O.upsample(occ_small, False, 4.0) * valid).detach()
        warp = warp + cfg.data_weight[0] * O.census_loss(im_a, recons, mask)
        if first is None:
            first = (occ_small, valid)
        entropy = entropy - cfg.w_entropy * log_pdf_t(f_ab, net[:, :2 * K], net[:, 2 * K:], wts).mean()
        hh, ww = f_ab.shape[2:]
        im_small = O.downsample(im_a[:B], False, 4.0)
        wx, wy = E._edge_weights(cfg, rep(im_small), 1)
        dx, dy = O.image_grads(f_ab)
        smooth = smooth + (wx / 2 * cfg.w_smooth * E._charbonnier(dx ** 2)).mean() \
            + (wy / 2 * cfg.w_smooth * E._charbonnier(dy ** 2)).mean()
        if cfg.w_oof > 0:
            c2 = O.flow_to_warp(f_ab)
            u = torch.clamp(c2[:, 0], max=0) ** 2 + torch.clamp(c2[:, 0] - float(ww - 1), min=0) ** 2
            v = torch.clamp(c2[:, 1], max=0) ** 2 + torch.clamp(c2[:, 1] - float(hh - 1), min=0) ** 2
            oof = oof + cfg.w_oof * (u + v).mean()
        if cfg.w_occ > 0:
            occ = occ + cfg.w_occ * (1 / (100.0 * occ_small + 1) * f_ab ** 2).mean()
    total = warp + smooth - entropy + oof + occ
    leaves = (net12, net21) + ((w12, w21) if has_w else ())
    gs = [torch.zeros_like(x) if g is None else g for x, g in zip(leaves, torch.autograd.grad(total, leaves, allow_unused=True))]
    out = {'total': total, 'warp': warp, 'smooth': smooth, 'entropy': entropy, 'oof': oof, 'occ': occ, 'flow12_2': f12,
           'occu_mask12': first[0], 'valid_mask12': first[1], 'gnet12': gs[0], 'gnet21': gs[1]}
    if has_w:
        out.update(gweights12=gs[2], gweights21=gs[3])
    return {key: torch.as_tensor(v, dtype=dtype).detach().numpy() for key, v in out.items()}


# ---- the model case (sizes and input of tests/prob_ref.py) ------------------------------------------------------------
PERTURB = 0.02  # pwcnet2's parameter i (in parameters() order) is multiplied by 1 + PERTURB cos(i + 1)


def model_cfg():
    from arflow_amd.config import AttrDict
    return AttrDict(type='component', feature_norm=True, level_dropout=0.0, out_channels=[2, 2, 0], inv_cov=False, n_pyramids=2,
                    mixture_weights=False)


def prepare_component(model):
    """fill_deterministic on each sub-model; then pwcnet2's parameters get the stated perturbation (the two components would
    otherwise be one); eval mode."""
    import math
    from oracle.fixture_common import fill_deterministic
    fill_deterministic(model.pwcnet1)
    fill_deterministic(model.pwcnet2)
    with torch.no_grad():
        for i, p in enumerate(model.pwcnet2.parameters()):
            p.mul_(1.0 + PERTURB * math.cos(i + 1.0))
    return model.eval()


def collect_component(res):
    """The stored view of ComponentNet's forward direction, finest level first: {'out_component_<level>': pooled fp32}."""
    from oracle.fixture_common import pool_to_quarter
    from tests import prob_ref as P
    return {'out_component_%d' % level: pool_to_quarter(f.detach().float().cpu(), P.H).numpy()
            for level, f in enumerate(res['flows_fw'])}
