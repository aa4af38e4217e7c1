"""Shared by the flow-evaluation tests and tools/make_flow_eval_golden.py: the seeded input recipe, and a float64
restatement of what arflow_flow_eval computes (include/arflow_hip.h; evaluate_flow of utils/flow_utils.py:121-183) --
scaling, half-pixel bilinear resize, end-point error, the eight sums, and the `band` of pixels that sit on one of the two
F1 thresholds, where an fp32 kernel and this restatement may legitimately disagree."""
import numpy as np
import torch
import torch.nn.functional as F

TAU = 1e-3  # half-width of the threshold band, px


def make_case(B, h, w, H, W, seed=7):
    """gt flow: bicubic upsample (align_corners=True) of 5x7 N(0, 12^2) noise; pred: that flow resized bilinearly to h x w
    plus N(0,1) * U(0,1) * 3 px of noise (in ground-truth pixels), in the prediction's own pixel units; valid ~
    Bernoulli(0.6), noc = valid * Bernoulli(0.7), move ~ Bernoulli(0.5).  -> float32 tensors pred [B,2,h,w], gt [B,4,H,W]
    (dense ground truth is gt[:, :2]), move [B,1,H,W]."""
    rng = np.random.default_rng(seed)
    coarse = torch.from_numpy(rng.normal(0.0, 12.0, (B, 2, 5, 7)))
    flow = F.interpolate(coarse, (H, W), mode='bicubic', align_corners=True)
    small = F.interpolate(flow, (h, w), mode='bilinear', align_corners=False)
    small = small + torch.from_numpy(rng.normal(0.0, 1.0, (B, 2, h, w)) * rng.uniform(0.0, 1.0, (B, 2, h, w)) * 3.0)
    pred = small * torch.tensor([w / W, h / H], dtype=torch.float64).view(1, 2, 1, 1)
    valid = torch.from_numpy((rng.uniform(size=(B, 1, H, W)) < 0.6).astype(np.float64))
    noc = valid * torch.from_numpy((rng.uniform(size=(B, 1, H, W)) < 0.7).astype(np.float64))
    move = torch.from_numpy((rng.uniform(size=(B, 1, H, W)) < 0.5).astype(np.float64))
    gt = torch.cat([flow, valid, noc], 1)
    return pred.float().contiguous(), gt.float().contiguous(), move.float().contiguous()


def _source(n_in, n_out):
    """Half-pixel source index of every output index: (i0, i1, lambda) in float64."""
    s = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5).clamp_min(0.0)
    i0 = s.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, s - i0


def resize_scaled(pred, H, W):
    """Steps 1, 2: (pred_u / w) * W, (pred_v / h) * H, then the bilinear resize to H x W; float64 [B,2,H,W]."""
    pred = pred.double()
    h, w = pred.shape[2:]
    p = torch.stack([pred[:, 0] / w * W, pred[:, 1] / h * H], 1)
    y0, y1, ly = _source(h, H)
    x0, x1, lx = _source(w, W)
    ly, lx = ly.view(1, 1, H, 1), lx.view(1, 1, 1, W)
    top = (1 - lx) * p[:, :, y0][:, :, :, x0] + lx * p[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * p[:, :, y1][:, :, :, x0] + lx * p[:, :, y1][:, :, :, x1]
    return (1 - ly) * top + ly * bot


def reference(pred, gt, move=None):
    """-> dict: epe [B,H,W], sums [B,8], band [B] (pixel counts), A = max(|gt flow|, |scaled pred|); all float64."""
    gt = gt.double()
    B, C, H, W = gt.shape
    up = resize_scaled(pred, H, W)
    h, w = pred.shape[2:]
    scaled = torch.stack([pred[:, 0].double() / w * W, pred[:, 1].double() / h * H], 1)
    epe = (up - gt[:, :2]).square().sum(1).sqrt()
    one = torch.ones_like(epe)
    valid, noc = (gt[:, 2], gt[:, 3]) if C == 4 else (one, one)
    mv = move.double()[:, 0] if move is not None else torch.zeros_like(epe)
    e = epe * valid
    thr = 0.05 * gt[:, :2].square().sum(1).sqrt().clamp_min(1e-10)
    bad = (e > 3.0) & (e > thr)  # e / max(|gt|, 1e-10) > 0.05
    band = (valid > 0) & (((epe - 3.0).abs() <= TAU) | ((epe - thr).abs() <= TAU))
    cols = [e, valid, epe * noc, noc, bad.double(), e * mv, valid * mv, torch.zeros_like(epe)]
    return {'epe': epe, 'sums': torch.stack([c.sum((1, 2)) for c in cols], 1), 'band': band.sum((1, 2)).double(),
            'A': float(max(gt[:, :2].abs().max(), scaled.abs().max()))}
