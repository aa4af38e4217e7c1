"""Shared by the uncertainty-metric tests and tools/make_uncert_golden.py: the seeded input recipe and a float64 restatement
of what csrc/uncert.hip and arflow_amd/metrics.py compute (sp_plot, evaluate_uncertainty and CalibrationCurve of
utils/flow_utils.py:186-320): the shifted and resized entropy map, the three sums per threshold, the full sp_plot with the
reference's `break`, and the digitised histogram with the `band` of elements that sit on a bin edge, where an fp32 exp and
this restatement may legitimately disagree."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import flow_eval_ref as R

ALPHA, EPS, REFINEMENTS = 100.0, 1e-1, 10
ULP32 = 2.0 ** -23  # spacing of float32 relative to the binade's lower end


def make_case(B, h, w, H, W, C=4, seed=11):
    """gt: the flow and masks of flow_eval_ref.make_case, valid ~ Bernoulli(0.7) (30 % invalid pixels).  entropy: per
    channel a smooth sinusoid over the prediction grid, -0.3 + 1.3 sin(.) + N(0, 0.15^2), so that sigma = exp(entropy) covers
    the calibration bins and passes cc_max = 3.5.  pred: the ground-truth flow resized to h x w plus N(0,1) * exp(entropy / 2)
    px of error (correlated with the entropy, so that the sparsification curve falls), in the prediction's own pixel units.
    -> float32 tensors pred [B,2,h,w], gt [B,C,H,W], entropy [B,2,h,w]."""
    _, gt, _ = R.make_case(B, h, w, H, W, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    yy, xx = np.meshgrid(np.arange(h) / max(h, 1), np.arange(w) / max(w, 1), indexing='ij')
    ent = np.empty((B, 2, h, w))
    for b in range(B):
        for c in range(2):
            fx, fy, ph = rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0), rng.uniform(0, 2 * math.pi)
            ent[b, c] = -0.3 + 1.3 * np.sin(2 * math.pi * (fx * xx + fy * yy) + ph) + rng.normal(0.0, 0.15, (h, w))
    ent = torch.from_numpy(ent)
    small = F.interpolate(gt[:, :2].double(), (h, w), mode='bilinear', align_corners=False)
    small = small + torch.from_numpy(rng.normal(0.0, 1.0, (B, 2, h, w))) * torch.exp(ent / 2)
    pred = small * torch.tensor([w / W, h / H], dtype=torch.float64).view(1, 2, 1, 1)
    gt = gt.clone()
    gt[:, 2] = torch.from_numpy((rng.uniform(size=(B, H, W)) < 0.7).astype(np.float32))
    gt[:, 3] = gt[:, 2] * gt[:, 3]
    return pred.float().contiguous(), gt[:, :C].contiguous(), ent.float().contiguous()


def resize(x, H, W):
    """Half-pixel bilinear resize of x [B,C,h,w] to H x W in float64 (the map of flow_eval_ref.resize_scaled)."""
    x = x.double()
    h, w = x.shape[2:]
    y0, y1, ly = R._source(h, H)
    x0, x1, lx = R._source(w, W)
    ly, lx = ly.view(1, 1, H, 1), lx.view(1, 1, 1, W)
    top = (1 - lx) * x[:, :, y0][:, :, :, x0] + lx * x[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * x[:, :, y1][:, :, :, x0] + lx * x[:, :, y1][:, :, :, x1]
    return (1 - ly) * top + ly * bot


def entropy_map(ent, H, W):
    """Steps 2-4 of evaluate_uncertainty in float64: shift each channel by 2 log(W / w), 2 log(H / h), resize, add the
    channels.  -> [B,H,W]."""
    h, w = ent.shape[2:]
    shift = torch.tensor([-2 * math.log(w) + 2 * math.log(W), -2 * math.log(h) + 2 * math.log(H)], dtype=torch.float64)
    return resize(ent.double() + shift.view(1, 2, 1, 1), H, W).sum(1)


def sums(err, field, g, thr, alpha=ALPHA):
    """err, field, g [H,W] (any float dtype), thr [K] -> [K,3] float64: sum (1-m) g, sum m g, sum err m g with
    m = 1 / (1 + exp(-alpha (thr - field))) in float64."""
    err, field, g = (np.asarray(t, np.float64) for t in (err, field, g))
    a = alpha * (np.asarray(thr, np.float64)[:, None, None] - field[None])
    with np.errstate(over='ignore'):
        m = 1.0 / (1.0 + np.exp(-a))
    return np.stack([((1.0 - m) * g).sum((1, 2)), (m * g).sum((1, 2)), (err * m * g).sum((1, 2))], 1)


def sums_tol(err, field, g, thr, alpha=ALPHA, margin=2.0):
    """-> [K,3]: what the fp32 arithmetic of arflow_sparsify_sums may differ from sums() by, derived from its counted
    roundings (u = 2^-24; g is a 0 / 1 mask; every term is >= 0, so the terms' bounds add up to the sum's):
      d = (float)(thr - (double)field)   one rounding of the difference formed in double        |da| <= |a| u
      a = alpha * d                      one rounding                                           |da| <= |a| u
      m = 1 / (1 + e), e = expf(-a)      dm / m = -(1 - m) de / e and de / e = da + 2u (an expf within one ulp); the
                                         addition and the division round once each:    |dm| / m <= (2 |a| (1 - m) + 4) u
      m g, err (m g)                     one rounding each                                      1 u, 2 u
      the thread's 8 pixels in fp32      7 roundings of a partial sum of non-negative terms     7 u
      double from the wave reduction on                                                         nothing
    so a term m g is off by at most (2 |a| (1 - m) + 12) u of itself and a term err m g by (2 |a| (1 - m) + 13) u.  Past
    |a| = 88 expf overflows and m is 0 or subnormal in fp32: such a term is below 2^-126 in both arithmetics, which the
    absolute 2^-126 (1 + max err) per pixel covers.  `margin` = 2 on top.
    sum (1-m) g: |dm| <= m (2 |a| (1 - m) + 4) u <= 4.6 u, 1 - m rounds once and the partial sum adds 7 u: 13 u per unit
    of g, inside the absolute 2^-20 sum g it is held to."""
    err, field, g = (np.asarray(t, np.float64) for t in (err, field, g))
    a = alpha * (np.asarray(thr, np.float64)[:, None, None] - field[None])
    with np.errstate(over='ignore'):
        m = 1.0 / (1.0 + np.exp(-a))
    rel = (2.0 * np.minimum(np.abs(a), 88.0) * (1.0 - m) + 12.0) * 2.0 ** -24
    floor = 2.0 ** -126 * (1.0 + err.max()) * g.size
    return np.stack([np.full(len(a), 2.0 ** -20 * g.sum()), margin * (m * g * rel).sum((1, 2)) + floor,
                     margin * (err * m * g * (rel + 2.0 ** -24)).sum((1, 2)) + floor], 1)


def interp(x, xp, fp):
    """Piecewise-linear interpolation as np.interp defines it, written out: clamped ends, the last of tied points."""
    out = np.empty(len(x))
    n = len(xp)
    for i, v in enumerate(x):
        j = int(np.sum(xp <= v)) - 1
        if j < 0:
            out[i] = fp[0]
        elif j >= n - 1 or xp[j] == v:
            out[i] = fp[min(j, n - 1)]
        else:
            out[i] = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (v - xp[j]) + fp[j]
    return out


def sp_plot(err, field, g, n=25, alpha=ALPHA, eps=EPS, sums_fn=None):
    """The whole sp_plot for one sample on fp32 (or float64) fields -> (splot [n], resid: max|frac - grid_frac| at every
    check the reference makes, the final one included).  The bracket is the field's extremes -+ eps in float64."""
    sums_fn = sums_fn or (lambda thr: sums(err, field, g, thr, alpha))
    field = np.asarray(field)
    greatest = float(field.max()) + eps
    least = float(field.min()) - eps
    total = float(np.asarray(g, np.float64).sum())
    assert 1.0 / (1.0 + math.exp(alpha * eps)) <= eps, 'the widening loops are not restated'
    grid = np.linspace(greatest, least, n)
    gf = np.linspace(0, 1, n)
    s = sums_fn(grid)
    resid = []
    for _ in range(REFINEMENTS):
        resid.append(np.abs(s[:, 0] / total - gf).max())
        if resid[-1] <= eps:
            break
        grid = interp(gf, s[:, 0] / total, grid)
        s = sums_fn(grid)
    resid.append(np.abs(s[:, 0] / total - gf).max())
    return interp(gf, s[:, 0] / total, s[:, 2] / s[:, 1]), resid


def steps_of(resid, eps=EPS):
    """The refinements the reference ran, from its recorded checks (NaN-padded): the index of the first one <= eps."""
    r = np.asarray(resid, np.float64)
    ok = np.nonzero(r <= eps)[0]
    return int(ok[0]) if len(ok) else REFINEMENTS


def auc(splot):
    x = np.linspace(0, 1, len(splot))
    y = splot / splot[0]
    return float(np.sum(np.diff(x) * (y[1:] + y[:-1]) / 2.0))


def evaluate_uncertainty(gt, pred, ent, n=25, epe_dtype=np.float64):
    """The float64 restatement end to end -> dict of numpy arrays: epe, ent_map [B,H,W], valid [B,H,W], splots,
    oracle_splots [B,n], AUC, AUC_diff [B], steps [B,2].  epe_dtype=np.float32 rounds the two maps to the precision the
    reference holds them in before the curves are taken."""
    B, C, H, W = gt.shape
    epe = R.reference(pred, gt)['epe'].numpy().astype(epe_dtype)
    emap = entropy_map(ent, H, W).numpy().astype(epe_dtype)
    valid = gt[:, 2].double().numpy() if C == 4 else np.ones((B, H, W))
    out = {'epe': epe, 'ent_map': emap, 'valid': valid, 'splots': [], 'oracle_splots': [], 'AUC': [], 'AUC_diff': [],
           'steps': []}
    for b in range(B):
        sp, r0 = sp_plot(epe[b], emap[b], valid[b], n)
        so, r1 = sp_plot(epe[b], epe[b], valid[b], n)
        out['splots'].append(sp), out['oracle_splots'].append(so)
        out['AUC'].append(auc(sp)), out['AUC_diff'].append(auc(sp) - auc(so))
        out['steps'].append([steps_of(r0), steps_of(r1)])
    return {k: np.asarray(v) for k, v in out.items()}


def calib_errors(pred, gt):
    """|pred / n * n - gt| per channel in float32, n = W, H: the reference's two roundings (same-size prediction: its resize
    is the identity).  -> float32 [B,2,H,W]."""
    H, W = pred.shape[2:]
    p = pred.numpy()
    n = np.array([W, H], np.float32).reshape(1, 2, 1, 1)
    return np.abs(p / n * n - gt[:, :2].numpy())


def calib_hist(pred, gt, ent, edges):
    """-> (sums [nb+1,3] float64: count, sum e, sum e^2 per np.digitize bin of exp(entropy) in float64, band: the number of
    elements whose sigma lies within 4 float32 ulps of an edge)."""
    e = calib_errors(pred, gt).astype(np.float64).ravel()
    sigma = np.exp(ent.numpy().astype(np.float64)).ravel()
    edges = np.asarray(edges, np.float64)
    idx = (edges[None, :] <= sigma[:, None]).sum(1)
    nb = len(edges)
    out = np.zeros((nb + 1, 3))
    np.add.at(out[:, 0], idx, 1.0)
    np.add.at(out[:, 1], idx, e)
    np.add.at(out[:, 2], idx, e * e)
    near = np.abs(edges[None, :] - sigma[:, None]).min(1)
    band = int((near <= 4 * ULP32 * np.maximum(sigma, 2.0 ** -126)).sum())
    return out, band


def curve_from_sums(s, cc_max=3.5, cc_samples=100):
    """(vals, means, sigmas, numbers) of calibration_curve() from [nb+1,3] sums, in float64."""
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = s[:, 1] / s[:, 0]
        var = np.maximum(s[:, 2] / s[:, 0] - mean * mean, 0.0)
    vals = (np.arange(cc_samples + 1) + 0.5) * cc_max / (cc_samples - 1)
    return vals, mean, np.sqrt(var), s[:, 0].astype(np.int64)


def load_case(z, tag):
    """-> dict: pred, gt, ent (torch, float32) and every ref_* / sens_* array of the case (numpy)."""
    c = {k[:-2]: z.raw(k) for k in z._z.files if k.endswith('_' + tag)}
    gt = torch.from_numpy(c['flow'].copy())
    if 'valid' in c:
        gt = torch.cat([gt, torch.from_numpy(c['valid'].astype(np.float32))[:, None],
                        torch.from_numpy(c['noc'].astype(np.float32))[:, None]], 1)
    c['gt'], c['pred'], c['ent'] = gt.contiguous(), torch.from_numpy(c['pred'].copy()), torch.from_numpy(c['ent'].copy())
    B, _, H, W = gt.shape
    c['mask'] = gt[:, 2].numpy() if gt.shape[1] == 4 else np.ones((B, H, W), np.float32)
    return c


def curve_tol(sens, ref):
    """8 x sens, point by point: the fixture stores the noise floor of every point of every curve."""
    return 8.0 * sens

