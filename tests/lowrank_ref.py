"""Shared by the low-rank tests and tools/make_lowrank_golden.py: the seeded input recipes, and a restatement in our own code
of what csrc/lowrank.hip and the 'lowrank' branch of arflow_amd/losses/uflow_elbo_loss.py compute (losses/uflow_elbo_loss.py
:180-188, :241-246, :362-381 of the reference).  TEST INFRASTRUCTURE ONLY.

std [B,2R,M,N]: channel 2k + c is column k of flow component c.  numpy, float64 unless a dtype is given:
    sampler   z[sB+b,c] = mean[b,c] + sum_k std[b,2k+c] eps[sB+b,2k+c]          (added in k order onto the mean)
    gram      G[b,c] = U U^T, U = std[b, c::2] as [R, M N];  logdet = log det G
    gradients of sum(gZ * z) + sum(glogdet * logdet):  gmean = sum_s gZ[sB+b],
              gstd[b,2i+c] = sum_s eps[sB+b,2i+c] gZ[sB+b,c] + 2 glogdet[b,c] (G^-1 U)[i]
The loss is restated in torch (float64) on the operators of oracle/ops.py, with autograd for its gradients.
"""
import numpy as np
import torch

from oracle import ops as O
from tests import elbo_ref as E

# csrc/lowrank.hip: pixels one stage-1 workgroup of the log-det reduces (CHUNK)
CHUNK = 1024


# ---- the operators ------------------------------------------------------------------------------------------------
def make_case(B, S, R, M, N, seed=23):
    """mean 1.5 N(0,1), std 0.1 N(0,1); eps, the output gradient gZ and glogdet ~ N(0,1).  -> dict of float32 arrays mean
    [B,2,M,N], std [B,2R,M,N], eps [S B,2R,1,1], gZ [S B,2,M,N], glogdet [B,2]."""
    rng = np.random.default_rng([seed, B, S, R, M, N])
    out = {'mean': 1.5 * rng.standard_normal((B, 2, M, N)), 'std': 0.1 * rng.standard_normal((B, 2 * R, M, N)),
           'eps': rng.standard_normal((S * B, 2 * R, 1, 1)), 'gZ': rng.standard_normal((S * B, 2, M, N)),
           'glogdet': rng.standard_normal((B, 2))}
    return {key: np.ascontiguousarray(v, dtype=np.float32) for key, v in out.items()}


def sampler(mean, std, eps, S, dtype=np.float64):
    """-> (z [S B,2,M,N], mag = |mean| + sum_k |std_k eps_k|, the bound's sum of the terms' magnitudes)."""
    mean, std, eps = (np.asarray(t, dtype=dtype) for t in (mean, std, eps))
    B, C, M, N = std.shape
    z = np.tile(mean, (S, 1, 1, 1))
    mag = np.abs(z)
    stdr = np.tile(std, (S, 1, 1, 1))
    for k in range(C // 2):
        term = stdr[:, 2 * k:2 * k + 2] * eps[:, 2 * k:2 * k + 2]
        z = z + term
        mag = mag + np.abs(term)
    return z, mag


def gram(std):
    """-> G [B,2,R,R] in float64."""
    std = np.asarray(std, dtype=np.float64)
    B, C, M, N = std.shape
    U = std.reshape(B, C // 2, 2, M * N).transpose(0, 2, 1, 3)  # [B,2,R,MN]
    return U @ U.transpose(0, 1, 3, 2)


def logdet(std):
    """-> (logdet [B,2], ginv [B,2,R,R]) in float64."""
    G = gram(std)
    sign, ld = np.linalg.slogdet(G)
    assert (sign > 0).all()
    return ld, np.linalg.inv(G)


def grads(std, eps, gZ, glogdet, S, ginv=None):
    """gZ / glogdet may be None.  -> (gmean, gstd, mag_mean, mag_std): the gradients in float64 and the sums of the terms'
    magnitudes.  ginv: the inverse to use in the second term (default: of the float64 Gram matrix)."""
    std = np.asarray(std, dtype=np.float64)
    B, C, M, N = std.shape
    R = C // 2
    gmean, mag_mean = np.zeros((B, 2, M, N)), np.zeros((B, 2, M, N))
    gstd, mag_std = np.zeros_like(std), np.zeros_like(std)
    if gZ is not None:
        gZ, eps = np.asarray(gZ, dtype=np.float64), np.asarray(eps, dtype=np.float64)
        for s in range(S):
            g = gZ[s * B:(s + 1) * B]
            gmean += g
            mag_mean += np.abs(g)
            for k in range(R):
                term = eps[s * B:(s + 1) * B, 2 * k:2 * k + 2] * g
                gstd[:, 2 * k:2 * k + 2] += term
                mag_std[:, 2 * k:2 * k + 2] += np.abs(term)
    if glogdet is not None:
        glogdet = np.asarray(glogdet, dtype=np.float64)
        if ginv is None:
            ginv = logdet(std)[1]
        ginv = np.asarray(ginv, dtype=np.float64)
        for c in range(2):
            U = std[:, c::2]  # [B,R,M,N]
            for i in range(R):
                terms = 2 * glogdet[:, c, None, None, None] * ginv[:, c, i, :, None, None] * U
                gstd[:, 2 * i + c] += terms.sum(1)
                mag_std[:, 2 * i + c] += np.abs(terms).sum(1)
    return gmean, gstd, mag_mean, mag_std


# ---- the loss ---------------------------------------------------------------------------------------------------
BASE = dict(E.BASE, approx='lowrank', columns=1)
# the cases of tests/golden/elbo_lowrank.npz: B = 2, 32 x 64 images, an 8 x 16 level 2
CASES = {
    'lr1': dict(columns=1, n_samples=1),
    'lr3': dict(columns=3, n_samples=2, edge_asymp=0.01),
    'lr15': dict(columns=15, n_samples=2),
    'lr16_nobk': dict(columns=16, n_samples=1, with_bk=False, w_oof=0.5, w_occ=0.3),
}
LOSS_B, LOSS_H, LOSS_W = E.LOSS_B, E.LOSS_H, E.LOSS_W
SCALARS, OUTPUTS = E.SCALARS, E.OUTPUTS


def case_cfg(tag):
    return E.Cfg(dict(BASE, **CASES[tag]))


def make_loss_case(tag, seed=37):
    """mean ~ 1.5 N(0,1), columns 0.1 N(0,1), images uniform, noise N(0,1).  -> dict of float32 arrays net12, net21
    [B,2+2R,h,w], im1, im2 [B,3,H,W] (the same pair in every case), eps12, eps21 [S B,2R,1,1]."""
    cfg = case_cfg(tag)
    B, H, W = LOSS_B, LOSS_H, LOSS_W
    h, w = H // 4, W // 4
    R = cfg.columns
    rng = np.random.default_rng([seed, sorted(CASES).index(tag)])
    out = {}
    for name in ('net12', 'net21'):
        out[name] = np.concatenate((1.5 * rng.standard_normal((B, 2, h, w)), 0.1 * rng.standard_normal((B, 2 * R, h, w))), 1)
    shared = np.random.default_rng(seed)  # one image pair for all cases
    for name in ('im1', 'im2'):
        out[name] = shared.uniform(0, 1, (B, 3, H, W))
    for name in ('eps12', 'eps21'):
        out[name] = rng.standard_normal((cfg.n_samples * B, 2 * R, 1, 1))
    return {key: np.ascontiguousarray(v, dtype=np.float32) for key, v in out.items()}


def loss(cfg, case, dtype=torch.float64):
    """The 'lowrank' loss of losses/uflow_elbo_loss.py:190-568.  case: the arrays of make_loss_case.  -> dict of numpy arrays:
    OUTPUTS (gnet12, gnet21: the gradients of `total`) and 'occ' (the occlusion penalty)."""
    t = {key: torch.from_numpy(np.asarray(v)).to(dtype) for key, v in case.items()}
    net12, net21 = t['net12'].requires_grad_(True), t['net21'].requires_grad_(True)
    S, B, R = cfg.n_samples, net12.shape[0], cfg.columns
    rep = lambda x: x.repeat(S, 1, 1, 1)  # noqa: E731

    def sample(net, eps):
        mean, std = net[:, 0:2], net[:, 2:2 + 2 * R]
        z = rep(mean)
        for k in range(R):
            z = z + rep(std[:, 2 * k:2 * k + 2]) * eps[:, 2 * k:2 * k + 2]
        return z, std

    f12, std12 = sample(net12, t['eps12'])
    f21, std21 = sample(net21, t['eps21'])
    im1, im2 = rep(t['im1']), rep(t['im2'])
    dirs = [(im1, im2, f12, f21, std12)]
    if cfg.with_bk:
        dirs.append((im2, im1, f21, f12, std21))
    warp = smooth = entropy = oof = occ = 0.
    first = None
    for im_a, im_b, f_ab, f_ba, std in dirs:
        coords = O.flow_to_warp(O.upsample(f_ab, True, 4.0))
        recons = O.resample(im_b.detach(), coords)
        valid = O.mask_invalid(coords)
        occ_small = torch.clamp(O.compute_range_map(f_ba), 0., 1.)
        mask = (O.upsample(occ_small, False, 4.0) * valid).detach()
        warp = warp + cfg.data_weight[0] * O.census_loss(im_a, recons, mask)
        if first is None:
            first = (occ_small, valid)
        hh, ww = std.shape[2:]
        U = std.reshape(B, R, 2, hh * ww).permute(0, 2, 1, 3)
        G = U @ U.transpose(2, 3)
        L = torch.linalg.cholesky(G)
        ld = 2 * torch.log(torch.diagonal(L, dim1=2, dim2=3)).sum(2)  # [B,2]
        entropy = entropy + cfg.w_entropy * (ld.sum(1) / (2 * hh * ww)).mean()
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
    g12, g21 = torch.autograd.grad(total, (net12, net21), allow_unused=True)
    g21 = torch.zeros_like(net21) if g21 is None else g21
    out = {'total': total, 'warp': warp, 'smooth': smooth, 'entropy': entropy, 'oof': oof, 'occ': occ, 'flow12_2': f12,
           'occu_mask12': first[0], 'valid_mask12': first[1], 'gnet12': g12, 'gnet21': g21}
    return {key: torch.as_tensor(v, dtype=dtype).detach().numpy() for key, v in out.items()}


# ---- the model cases (sizes and input of tests/prob_ref.py) --------------------------------------------------------
MODEL_CASES = {'L30': [2, 0, 30], 'L6': [2, 0, 6]}


def model_cfg(tag):
    from arflow_amd.config import AttrDict
    return AttrDict(type='uflow_prob', feature_norm=True, level_dropout=0.0, out_channels=list(MODEL_CASES[tag]),
                    inv_cov=False, n_pyramids=1, mixture_weights=False)


def stored_channels(tag, direction, level):
    """Channel indices kept per (case, direction, level), None = not stored (no committed file above 1 MiB): the flow pair at
    every level of both directions; the columns at the output level 2 and at the two upsampled levels in the forward
    direction (level 2: first, middle and last pair of the 30, all 6; levels 1 and 0: the last column)."""
    C = sum(MODEL_CASES[tag])
    if level >= 3:
        return [0, 1]
    if direction != 'fw':
        return [0, 1] if level == 2 else None
    if level == 2:
        return list(range(C)) if C <= 8 else [0, 1, 2, 3, 16, 17, C - 2, C - 1]
    return [0, 1, C - 1]


def prepare(model):
    from oracle.fixture_common import fill_deterministic
    fill_deterministic(model)
    return model.eval()


def collect(res, tag):
    """The stored view of a model's result: {'out_<tag>_<fw|bw>_<level>': pooled fp32 array of the stored channels}."""
    from oracle.fixture_common import pool_to_quarter
    from tests import prob_ref as P
    out = {}
    for direction in ('fw', 'bw'):
        for level, f in enumerate(res['flows_' + direction]):
            ch = stored_channels(tag, direction, level)
            if ch is not None:
                out['out_%s_%s_%d' % (tag, direction, level)] = pool_to_quarter(f.detach().float().cpu(), P.H)[:, ch].numpy()
    return out
