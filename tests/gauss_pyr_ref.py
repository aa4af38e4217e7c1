"""Definitions shared by tools/make_pwcliteprob_golden.py and the tests that replay tests/golden/elbo_pyramid.npz (DESIGN.md
section 27): the loss and model cases, their seeded inputs, a numpy float64 restatement of the pyramid sampler with its entropy
sums and closed-form gradient, a torch restatement of ElboLoss (losses/elbo_loss.py:9-146) on oracle/ops.py / oracle/losses.py,
and float64 restatements of the align_corners=True upsample and of the half-pixel x4 flow upsample with the per-pixel bounds
the kernel tests use.
TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from arflow_amd.config import AttrDict
from oracle import losses as OL
from oracle.fixture_common import fill_deterministic, synth_pair

EPS = 2.0 ** -24  # unit roundoff of fp32

# ---- loss cases ------------------------------------------------------------------------------------------------------------
LOSS_B, LOSS_H, LOSS_W = 2, 32, 64
LOSS_SIZES = [(32, 64), (16, 32), (8, 16), (4, 8), (2, 4)]
_BASE = dict(type='elbo', w_l1=0.15, w_ssim=0.85, w_ternary=0.0, alpha=10, w_entropy=0.1)
LOSS_CASES = {
    'full': dict(_BASE, warp_pad='border', occ_from_back=True, with_bk=True, w_smooth=75.0, w_scales=[1.0, 1.0, 1.0, 1.0, 0.0],
                 w_sm_scales=[1.0, 0.0, 0.0, 0.0, 0.0], w_en_scales=[1.0, 1.0, 1.0, 1.0, 1.0]),
    # the entropy-zip quirk: the computed scales 0, 2, 3 meet w_en_scales[0], [1], [2]
    'skip_mid': dict(_BASE, warp_pad='border', occ_from_back=True, with_bk=True, w_smooth=75.0, w_scales=[1.0, 0.0, 1.0, 1.0, 0.0],
                     w_sm_scales=[1.0, 0.0, 0.5, 0.0, 0.0], w_en_scales=[1.0, 0.5, 0.25, 0.125, 2.0]),
    'nobk_bidir': dict(_BASE, warp_pad='zeros', occ_from_back=False, with_bk=False, w_smooth=50.0, smooth_2nd=True,
                       w_scales=[1.0, 1.0, 1.0, 1.0, 0.0], w_sm_scales=[1.0, 0.5, 0.0, 0.0, 0.0],
                       w_en_scales=[1.0, 1.0, 1.0, 1.0, 1.0]),
}
LOSS_OUTPUTS = ('total', 'warp', 'smooth', 'entropy', 'absmean')
MASK_MARGIN = 1e-4  # no pixel of the thresholded quantity may lie this close to its threshold


def loss_cfg(tag):
    return AttrDict({k: (list(v) if isinstance(v, list) else v) for k, v in LOSS_CASES[tag].items()})


def computed_scales(cfg):
    return [i for i in range(len(LOSS_SIZES)) if cfg.w_scales[i] != 0]


def make_loss_inputs(seed):
    """-> {'img' [B,6,H,W], 'net_i' [B,8,h_i,w_i], 'eps_i' [B,4,h_i,w_i]} fp32, shared by all loss cases.  Flows of a few pixels
    at full resolution, log-variances around -2 (a standard deviation of about a third of a pixel); the nets and the noise
    are multiples of 2^-7 and the images of 2^-8, so that the stored fp32 arrays compress."""
    g = torch.Generator().manual_seed(seed)
    img, _ = synth_pair(LOSS_B, LOSS_H, LOSS_W, g)
    out = {'img': (img * 256).round() / 256}
    for i, (h, w) in enumerate(LOSS_SIZES):
        net = torch.randn(LOSS_B, 8, h, w, generator=g)
        s = 2.0 ** -i
        for d in (0, 4):
            base = F.interpolate(torch.randn(LOSS_B, 2, max(h // 4, 1), max(w // 4, 1), generator=g), (h, w), mode='bilinear',
                                 align_corners=False)
            net[:, d:d + 2] = 2.0 * s * base + 0.25 * s * net[:, d:d + 2]
            net[:, d + 2:d + 4] = -2.0 + 2.0 * math.log(s) + 0.5 * net[:, d + 2:d + 4]
        out['net_%d' % i] = (net * 128).round() / 128
        out['eps_%d' % i] = (torch.randn(LOSS_B, 4, h, w, generator=g) * 128).round() / 128
    return {k: v.float().contiguous() for k, v in out.items()}


# ---- the sampler in numpy float64 -----------------------------------------------------------------------------------------
def sample_np(net, eps):
    """net [B,8,h,w], eps [B,4,h,w] -> z [B,4,h,w] (float64), its parts (std * eps) and ent [2] = sum of the log-variances."""
    net, eps = np.asarray(net, np.float64), np.asarray(eps, np.float64)
    z, part = np.empty(eps.shape), np.empty(eps.shape)
    ent = np.empty(2)
    for d in range(2):
        mean, lv = net[:, 4 * d:4 * d + 2], net[:, 4 * d + 2:4 * d + 4]
        part[:, 2 * d:2 * d + 2] = np.exp(lv / 2.0) * eps[:, 2 * d:2 * d + 2]
        z[:, 2 * d:2 * d + 2] = mean + part[:, 2 * d:2 * d + 2]
        ent[d] = lv.sum()
    return z, part, ent


def sample_grad_np(net, eps, gz, gent):
    """Closed form: gmean = gz, glogvar = gz * std * eps / 2 + gent[d] -> gnet [B,8,h,w] and the magnitude of the product
    term |gz std eps / 2| (the bound's first term) in the log-variance channels."""
    net, eps = np.asarray(net, np.float64), np.asarray(eps, np.float64)
    gz = np.zeros(eps.shape) if gz is None else np.asarray(gz, np.float64)
    gnet, mag = np.zeros(net.shape), np.zeros(net.shape)
    for d in range(2):
        lv, g = net[:, 4 * d + 2:4 * d + 4], gz[:, 2 * d:2 * d + 2]
        prod = g * (0.5 * np.exp(lv / 2.0) * eps[:, 2 * d:2 * d + 2])
        gnet[:, 4 * d:4 * d + 2] = g
        gnet[:, 4 * d + 2:4 * d + 4] = prod + (0.0 if gent is None else float(gent[d]))
        mag[:, 4 * d + 2:4 * d + 4] = np.abs(prod)
    return gnet, mag


def pyramid_objective_np(nets, eps, wz, went):
    """sum_i <wz_i, z_i> + sum_{i,d} went[i,d] ent[i,d]: the scalar whose gradient sample_grad_np(., ., wz_i, went[i]) is."""
    total = 0.0
    for i, (net, e) in enumerate(zip(nets, eps)):
        z, _, ent = sample_np(net, e)
        total += float((np.asarray(wz[i], np.float64) * z).sum()) + float((np.asarray(went[i], np.float64) * ent).sum())
    return total


# ---- ElboLoss restated on the oracle ----------------------------------------------------------------------------------------
def elbo_loss_ref(cfg, output, target, eps):
    """losses/elbo_loss.py:54-146 with the recorded noise: eps holds one [B,4,h,w] tensor per scale with a non-zero w_scales
    entry.  The photometric / smoothness part is oracle.losses.unFlowLoss on the samples (the same statements as :79-115,
    :130-137); the entropy list has entries for the computed scales only and is zipped with w_en_scales from its start
    (:132, :138-139).  -> (total, warp, smooth, entropy, absmean), (mask1, mask2) of scale 0."""
    comp = [i for i in range(len(output)) if cfg.w_scales[i] != 0]
    assert len(eps) == len(comp)
    flows = [o[:, 0:4] for o in output]
    entropies = []
    for i, e in zip(comp, eps):
        o = output[i]
        zf = o[:, 0:2] + torch.exp(o[:, 2:4] / 2.0) * e[:, 0:2]
        zb = o[:, 4:6] + torch.exp(o[:, 6:8] / 2.0) * e[:, 2:4]
        flows[i] = torch.cat([zf, zb], 1)
        ent = torch.sum(o[:, 2:4], dim=1).mean() / 2.0
        if cfg.with_bk:
            ent = (ent + torch.sum(o[:, 6:8], dim=1).mean() / 2.0) / 2.0
        entropies.append(ent)
    inner = OL.unFlowLoss(cfg)
    _, warp, smooth, _ = inner(flows, target)
    entropy = cfg.w_entropy * sum(l * w for l, w in zip(entropies, cfg.w_en_scales))
    return (warp + smooth - entropy, warp, smooth, entropy, output[0].abs().mean()), \
        (inner.pyramid_occu_mask1[0], inner.pyramid_occu_mask2[0])


# ---- model cases ------------------------------------------------------------------------------------------------------------
MODEL_H, MODEL_W = 128, 192  # the coarsest level is 2 x 3
MODEL_CASES = {
    'U0': dict(upsample=False, reduce_dense=True, batch=2),
    'U1': dict(upsample=True, reduce_dense=False, batch=1),
    'clamp': dict(upsample=False, reduce_dense=True, batch=2, shift=12.0),  # clamp(max=10) binds
}
MODEL_KEYS = 60
MODEL_PARAMS = {True: 2243576, False: 3358892}  # by reduce_dense


def model_cfg(tag):
    c = MODEL_CASES[tag]
    return AttrDict(type='pwclite_prob', upsample=c['upsample'], n_frames=2, reduce_dense=c['reduce_dense'])


def make_model_input(tag):
    """-> the image pair [B,6,H,W] in [0,1] and its float64 sum (against a drift of the recipe)."""
    img, _ = synth_pair(MODEL_CASES[tag]['batch'], MODEL_H, MODEL_W, torch.Generator().manual_seed(4107))
    return img.contiguous(), float(img.double().sum())


def prepare(model, tag):
    """Deterministic weights, the case's shift of the log-variance biases of the context head, eval mode."""
    fill_deterministic(model)
    shift = MODEL_CASES[tag].get('shift')
    if shift is not None:
        last = model.context_networks.convs[6][0]
        with torch.no_grad():
            last.bias[2:4] += shift
    return model.eval()


def collect(res, tag):
    """{'out_<tag>_<fw|bw>_<level>': fp32 array}; the x4 outputs of an upsampling case average-pooled back by 4, as
    models.npz does (no committed file above 1 MiB)."""
    out = {}
    k = 4 if MODEL_CASES[tag]['upsample'] else 1
    for direction in ('fw', 'bw'):
        for level, f in enumerate(res['flows_' + direction]):
            f = f.detach().float().cpu()
            out['out_%s_%s_%d' % (tag, direction, level)] = (F.avg_pool2d(f, k) if k > 1 else f).numpy()
    return out


# ---- float64 restatement of the align_corners=True upsample and the kernels' bounds -------------------------------------------
def _taps(n, f):
    """Source indices and weights of the bilinear resize n -> f n with align_corners=True in float64."""
    N = f * n
    d = np.arange(N, dtype=np.float64)
    src = d * ((n - 1) / (N - 1) if N > 1 else 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = src - i0
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(1.0 - l1), torch.from_numpy(l1)


def _taps_half(n, f):
    """... with align_corners=False and the scale factor given (up_source, upsample_dev.hpp:14-28): src = max((d + 1/2) / f
    - 1/2, 0), both taps clamped.  The weights are multiples of 1 / (2 f): exact in fp32 for f = 2, 4, no coordinate term."""
    d = np.arange(f * n, dtype=np.float64)
    src = np.maximum((d + 0.5) / f - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = src - i0
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(1.0 - l1), torch.from_numpy(l1)


def up_half(x, f):
    """x f bilinear resize (align_corners=False, half-pixel centres) of a [..., h, w] tensor in x's dtype, blended in the
    order of up_blend."""
    return up_align(x, f, _taps_half)


def flow_up_half_ref(x, g, f=4, dtype=torch.float64, taps=_taps_half):
    """AF.flow_upsample(x, f, False) = f * up_half(x, f) and its adjoint for the fine gradient g, in `dtype` on the CPU, with
    the float64 bounds  6 EPS f sum w |x|  (the out_up rule, FWD_ROUNDINGS)  and  bwd_roundings(f) EPS f sum w |g|.
    taps=_taps (WRONG on purpose): the align_corners=True weights.  -> out, bound, gin, gbound"""
    x, g = x.detach().cpu(), g.detach().cpu()
    xv = x.to(dtype).requires_grad_(True)
    out = f * up_align(xv, f, taps)
    (gin,) = torch.autograd.grad(out, xv, g.to(dtype))
    xa = x.double().abs().requires_grad_(True)
    mag = f * up_align(xa, f, _taps_half)
    (gmag,) = torch.autograd.grad(mag, xa, g.double().abs())
    return out.detach(), FWD_ROUNDINGS * EPS * mag.detach(), gin, bwd_roundings(f) * EPS * gmag


def up_align(x, f, taps=_taps):
    """x f bilinear resize (align_corners=True) of a [..., h, w] tensor in x's dtype."""
    h, w = x.shape[-2:]
    ya, yb, wy0, wy1 = taps(h, f)
    xa, xb, wx0, wx1 = taps(w, f)
    wy0, wy1 = wy0.to(x.dtype).view(-1, 1), wy1.to(x.dtype).view(-1, 1)
    wx0, wx1 = wx0.to(x.dtype), wx1.to(x.dtype)
    top, bot = x[..., ya, :], x[..., yb, :]
    return wy0 * (wx0 * top[..., xa] + wx1 * top[..., xb]) + wy1 * (wx0 * bot[..., xa] + wx1 * bot[..., xb])


def _spread(x, f):
    """max tap - min tap of every fine pixel: over its 2 x 2 taps (clamped at the border) -> [..., f h, f w]."""
    h, w = x.shape[-2:]
    ya, yb = _taps(h, f)[:2]
    xa, xb = _taps(w, f)[:2]
    top, bot = x[..., ya, :], x[..., yb, :]
    taps = torch.stack([top[..., xa], top[..., xb], bot[..., xa], bot[..., xb]])
    return taps.amax(0) - taps.amin(0)


def chan_rule(C, factor, n_flow, n_diag, diag_bias, dtype):
    s = torch.ones(C, dtype=dtype)
    s[:n_flow] = factor
    b = torch.zeros(C, dtype=dtype)
    b[n_flow:n_flow + n_diag] = diag_bias
    return s.view(1, C, 1, 1), b.view(1, C, 1, 1)


FWD_ROUNDINGS = 6  # the out_up rule (tests/test_out_up_gpu.py): bias add, product, sum, product, sum on any path
COORD_ROUNDINGS = 4  # the source coordinate is a product of two fp32 roundings (<= 2 EPS max(h, w)), on two axes


def bwd_roundings(f):
    """A fine pixel's term passes at most 2 f + 1 fused multiply-adds of its row sum and 2 f + 1 of the sum over rows (a
    coarse cell is read by fewer than 2 f fine rows / columns), its two weights are rounded once each (1 - lambda) and a
    cell both of whose clamped taps coincide adds them, and the scale is exact."""
    return 2 * (2 * f + 1) + 4


def prob_upsample_ref(x, factor, n_flow, n_diag, diag_bias, dtype=torch.float64):
    """-> (out, bound): out[b,c] = s_c * resize(x[b,c] + b_c) in `dtype` on the CPU;
    bound = s_c (6 EPS sum_i w_i |x_i + b_c| + 4 EPS max(h, w) (max tap - min tap)) in float64."""
    x = x.detach().cpu()
    s, b = chan_rule(x.shape[1], factor, n_flow, n_diag, diag_bias, dtype)
    out = s * up_align(x.to(dtype) + b, factor)
    s64, b64 = chan_rule(x.shape[1], factor, n_flow, n_diag, diag_bias, torch.float64)
    a = x.double() + b64
    bound = s64 * (FWD_ROUNDINGS * EPS * up_align(a.abs(), factor) + COORD_ROUNDINGS * EPS * max(x.shape[-2:]) * _spread(a, factor))
    return out, bound


def prob_upsample_adjoint_ref(g, factor, n_flow, dtype=torch.float64):
    """Adjoint for the fine gradient g [B,C,f h,f w] -> (gcoarse in `dtype`, bound in float64): the forward rule transposed --
    s_c (R EPS sum w |g| + 4 EPS max(h, w) sum of |g| over the fine pixels that read the cell), R = bwd_roundings(factor): the
    gather's own count in place of the forward's six, as tests/test_out_up_gpu.py counts its adjoint apart from its forward."""
    g = g.detach().cpu()
    B, C, H2, W2 = g.shape
    h, w = H2 // factor, W2 // factor
    s, _ = chan_rule(C, factor, n_flow, 0, 0.0, dtype)
    x = torch.zeros(B, C, h, w, dtype=dtype, requires_grad=True)
    (gx,) = torch.autograd.grad(s * up_align(x, factor), x, g.to(dtype))
    s64, _ = chan_rule(C, factor, n_flow, 0, 0.0, torch.float64)
    x2 = torch.zeros(B, C, h, w, dtype=torch.float64, requires_grad=True)
    (gm,) = torch.autograd.grad(s64 * up_align(x2, factor), x2, g.double().abs())
    # the fine pixels that read cell (i, j): those one of whose two (clamped) taps per axis is the cell
    ya, yb = _taps(h, factor)[:2]
    xa, xb = _taps(w, factor)[:2]
    My = torch.zeros(h, H2, dtype=torch.float64)
    My[ya, torch.arange(H2)] = 1
    My[yb, torch.arange(H2)] = 1
    Mx = torch.zeros(w, W2, dtype=torch.float64)
    Mx[xa, torch.arange(W2)] = 1
    Mx[xb, torch.arange(W2)] = 1
    reach = torch.einsum('iy,bcyx,jx->bcij', My, g.double().abs(), Mx)
    bound = s64 * (bwd_roundings(factor) * EPS * gm / s64 + COORD_ROUNDINGS * EPS * max(h, w) * reach)
    return gx, bound


UP_SHAPES = [(1, 4, 1, 1), (2, 4, 3, 5), (1, 4, 2, 3), (2, 4, 24, 32)]  # the last: float4 stores
UP_FACTORS = (2, 4)
_up_cache = {}


def up_bias(factor):
    """2 ln factor as the fp32 value the kernel takes (the reference's fp32 addition rounds its constant the same way)."""
    return float(torch.tensor(2 * math.log(factor), dtype=torch.float32))


def up_case(shape, factor, n_flow=2, n_diag=2):
    """Seeded input, fine gradient and the float64 references with their bounds, computed once and left unchanged."""
    key = (shape, factor, n_flow, n_diag)
    if key not in _up_cache:
        B, C, h, w = shape
        g = torch.Generator().manual_seed(1000 * h + 10 * w + factor)
        x = 3.0 * torch.randn(B, C, h, w, generator=g)
        go = torch.randn(B, C, factor * h, factor * w, generator=g)
        ref, bound = prob_upsample_ref(x, factor, n_flow, n_diag, up_bias(factor))
        gref, gbound = prob_upsample_adjoint_ref(go, factor, n_flow)
        _up_cache[key] = dict(x=x, go=go, ref=ref, bound=bound, gref=gref, gbound=gbound)
    return _up_cache[key]
