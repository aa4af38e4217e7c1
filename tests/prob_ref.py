"""Definitions shared by tools/make_prob_golden.py and the tests that replay tests/golden/prob_models.npz: the cases of the
probabilistic model, its seeded input, what each case stores, and a float64 restatement of upsample_out
(models/uflow_prob_model.py:223-250) with the per-pixel error bounds the kernel tests use.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

from arflow_amd.config import AttrDict
from oracle.fixture_common import fill_deterministic, pool_to_quarter, synth_pair

H, W = 192, 256  # level 4 is then 6 x 8: the reference refuses a level not taller than the displacement 4

# E runs in train() mode after torch.manual_seed(E_SEED)
E_SEED = 123
CASES = {
    'A': dict(out_channels=[2, 2, 0], inv_cov=False),
    'B': dict(out_channels=[2, 2, 30], inv_cov=False),
    'C': dict(out_channels=[2, 2, 0], inv_cov=True),
    'D': dict(out_channels=[2, 2, 0], inv_cov=False, shift=(20.0, -20.0)),  # both clamp limits bind
    'E': dict(out_channels=[2, 2, 0], inv_cov=False, level_dropout=0.5),
}
PARAMS = {(2, 2, 0): 5909172, (2, 2, 30): 5961072}

# What is stored (no committed file above 1 MiB): channel indices per (case, direction, level), None = not stored.  Every
# channel group at every level is covered by at least one case: flow and log_diag everywhere by A (forward direction, all six
# levels), the rest group at the output level 2 and at the two upsampled levels by B; the backward direction (the second
# half of the 2B batch) at levels 2..5 by every case but D; the negative diag_bias at the upsampled levels by C.
B_REST2 = [4, 5, 10, 11, 16, 17, 22, 23, 28, 29, 32, 33]  # pairs of the 30 rest channels kept at level 2
B_REST01 = [32, 33]


def stored_channels(tag, direction, level):
    fw = direction == 'fw'
    if level >= 2:
        if tag == 'D' and not fw:
            return None
        return [0, 1, 2, 3] + (B_REST2 if (tag == 'B' and level == 2 and fw) else [])
    if not fw:
        return None
    return {'A': [0, 1, 2, 3], 'B': [0, 1, 2, 3] + B_REST01, 'C': [2, 3]}.get(tag)


def model_cfg(tag):
    c = CASES[tag]
    return AttrDict(type='uflow_prob', feature_norm=True, level_dropout=c.get('level_dropout', 0.0),
                    out_channels=list(c['out_channels']), inv_cov=c['inv_cov'], n_pyramids=1, mixture_weights=False)


def make_input():
    """-> img1, img2 [1,3,H,W] in [0,1], and the float64 sum of both against a drift of the recipe."""
    img, _ = synth_pair(1, H, W, torch.Generator().manual_seed(2207))
    return img[:, :3].contiguous(), img[:, 3:].contiguous(), float(img.double().sum())


def prepare(model, tag):
    """Deterministic weights, the case's bias shift, the case's mode."""
    fill_deterministic(model)
    shift = CASES[tag].get('shift')
    if shift is not None:
        last = [m for m in model._refine_model if isinstance(m, torch.nn.Conv2d)][-1]
        with torch.no_grad():
            last.bias[2] += shift[0]
            last.bias[3] += shift[1]
    if tag == 'E':
        model.train()
        torch.manual_seed(E_SEED)
    else:
        model.eval()
    return model


def collect(res, tag):
    """The stored view of a model's result: {'out_<tag>_<fw|bw>_<level>': pooled fp32 array of the stored channels}."""
    out = {}
    for direction in ('fw', 'bw'):
        for level, f in enumerate(res['flows_' + direction]):
            ch = stored_channels(tag, direction, level)
            if ch is not None:
                out['out_%s_%s_%d' % (tag, direction, level)] = pool_to_quarter(f.detach().float().cpu(), H)[:, ch].numpy()
    return out


# ---- float64 restatement of upsample_out and the kernels' error bounds -------------------------------------------------
def _taps(n, align=False, shift=0):
    """Source indices and weights of the x2 bilinear resize n -> 2n (ATen's align_corners=False map, float64; exact: every
    weight is a multiple of 1/4).  align / shift: the mutations the kernel tests must be able to tell apart."""
    d = np.arange(2 * n, dtype=np.float64)
    if align:
        src = d * ((n - 1) / (2 * n - 1) if n > 1 else 0.0)
    else:
        src = np.maximum(0.5 * (d + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = src - i0
    i0, i1 = np.clip(i0 + shift, 0, n - 1), np.clip(i1 + shift, 0, n - 1)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(1.0 - l1), torch.from_numpy(l1)


def up2(x, align=False, shift=0):
    """x2 bilinear resize of a [..., h, w] tensor in x's dtype, and of |x| (the bound's sum of w_i |a_i|)."""
    h, w = x.shape[-2:]
    ya, yb, wy0, wy1 = _taps(h, align, shift)
    xa, xb, wx0, wx1 = _taps(w, align, shift)
    wy0, wy1 = wy0.to(x.dtype).view(-1, 1), wy1.to(x.dtype).view(-1, 1)
    wx0, wx1 = wx0.to(x.dtype), wx1.to(x.dtype)
    top, bot = x[..., ya, :], x[..., yb, :]
    return wy0 * (wx0 * top[..., xa] + wx1 * top[..., xb]) + wy1 * (wx0 * bot[..., xa] + wx1 * bot[..., xb])


def chan_rule(C, n_flow, n_diag, diag_bias, dtype):
    s = torch.ones(C, dtype=dtype)
    s[:n_flow] = 2
    b = torch.zeros(C, dtype=dtype)
    b[n_flow:n_flow + n_diag] = diag_bias
    return s.view(1, C, 1, 1), b.view(1, C, 1, 1)


def upsample_out_ref(x, n_flow, n_diag, diag_bias, dtype=torch.float64):
    """-> (out, mag): out[b,c] = s_c * resize(x[b,c] + b_c) in `dtype` on the CPU; mag = s_c * sum_i w_i |x_i + b_c|."""
    x = x.detach().cpu().to(dtype)
    s, b = chan_rule(x.shape[1], n_flow, n_diag, diag_bias, dtype)
    return s * up2(x + b), s * up2((x + b).abs())


def upsample_out_adjoint_ref(g, n_flow, dtype=torch.float64):
    """Adjoint of upsample_out for the fine gradient g [B,C,2h,2w] -> (gcoarse, mag = s_c * sum w |g|), by autograd over the
    restatement (exact structure, float64 accumulation)."""
    g = g.detach().cpu().to(dtype)
    B, C, H2, W2 = g.shape
    s, _ = chan_rule(C, n_flow, 0, 0.0, dtype)
    x = torch.zeros(B, C, H2 // 2, W2 // 2, dtype=dtype, requires_grad=True)
    (gx,) = torch.autograd.grad(s * up2(x), x, g)
    x2 = torch.zeros_like(x, requires_grad=True)
    (gm,) = torch.autograd.grad(s * up2(x2), x2, g.abs())
    return gx, gm


EPS = 2.0 ** -24
FWD_ROUNDINGS = 6    # bound of tests/test_out_up_gpu.py: five roundings on any path of the blend
BWD_ROUNDINGS = 20   # at most 16 terms, eight roundings on any path
