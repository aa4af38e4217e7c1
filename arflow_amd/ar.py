"""The augmentation-regularisation pass on the native kernels of csrc/ar.hip: the step that gives
ARFlow its name.  The first pass's prediction and its non-occlusion mask are moved into a new view, the model runs a second
time on the transformed pair and the disagreement is penalised.

THE ARITHMETIC.  theta is [a b tx; c d ty] per sample, float32 [B,6].  It maps an output pixel p' = (x', y') to the source
position s = (a x' + b y' + tx, c x' + d y' + ty), in pixel units; d(p') = s - p', L = [[a, b], [c, d]], det L != 0.

    img_t  = flow_warp(img, d, pad='zeros', align_corners=True)      utils/warp_utils.py:83-90; all frames share theta
    g      = flow_warp(flow, d, pad='zeros');  flow_t = L^-1 g:      u_t = ( d g_u - b g_v) / det
                                                                     v_t = (-c g_u + a g_v) / det
             (a source point q lands at L^-1 (q - t) in the output, so a displacement f(s) becomes L^-1 f(s))
    mask_t = flow_warp(noc, d, pad='zeros') * border_mask(d)         utils/warp_utils.py:119-134, strict: 0 < s_x < W - 1 and
                                                                     0 < s_y < H - 1; an absent noc reads as ones

    ar_loss = ( sum_{b,c,y,x} (|pred - flow_t| + eps)^q m ) / (2 B H W)  /  ( sum m / (B H W) + 1e-7 )
              (losses/penalty_functions.py:3-4 under a mask mean); the gradient is taken with respect to pred only:
              q (|e| + eps)^(q - 1) sign(e) m times the upstream gradient over the two denominators, sign(0) = 0

Every piece has an oracle in the reference (flow_warp, border_mask, abs_robust_loss).  THE WIRING is defined by this build:
it is named after the published ARFlow recipe and was NOT compared against that code, which is not part of the reference this
project mirrors (the fork dropped the step).  draw_ar_params' map and ranges, DEFAULT_ST_CFG and TrainStep's order of
operations are this build's reading of the recipe.

GPU only: a CPU tensor raises ArflowHipError.  ar_transform has no autograd: its outputs are targets or inputs.
"""
import math

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .augment import AugmentParams, _get, _size
from .ddp import global_denominator
from .functional import _call, _p, _stream

__all__ = ['ar_transform', 'ar_loss', 'draw_ar_params', 'theta_from_augment', 'identity_theta', 'DEFAULT_ST_CFG']

# the ranges of the published recipe's spatial transform, as this build reads them (zoom, rotation in radians, translation as
# a fraction of the image, horizontal flip); its squeeze, vertical flip and occlusion noise are not built
DEFAULT_ST_CFG = dict(zoom=(1.0, 1.5), rotate=0.2, trans=0.2, hflip=True)


def identity_theta(B):
    return torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float32).repeat(int(B), 1)


def draw_ar_params(st_cfg, B, hw, generator):
    """-> theta float32 [B,6] on the CPU, from ONE seeded CPU generator, drawn and composed in float64 and rounded once:
        s = c + R(phi) diag(+-1/z, 1/z) (p' - c) + tau         about c = ((W - 1) / 2, (H - 1) / 2)
        z ~ U[zoom[0], zoom[1]],  phi ~ U[-rotate, rotate] radians,  tau ~ U[-trans, trans] * (W, H),  the sign flipped with
        probability 1/2 when hflip is set.  Only what is configured is drawn (in that order); missing keys read as off."""
    B = int(B)
    H, W = _size(hw, 'hw')
    if B < 1:
        raise ValueError('B must be >= 1 (got %r)' % (B,))
    g = generator

    def uniform(lo, hi, n=B):
        return lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)

    zoom = _get(st_cfg, 'zoom', None)
    rotate, trans = float(_get(st_cfg, 'rotate', 0.0)), float(_get(st_cfg, 'trans', 0.0))
    z = torch.ones(B, dtype=torch.float64)
    phi = torch.zeros(B, dtype=torch.float64)
    taux, tauy = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    sign = torch.ones(B, dtype=torch.float64)
    if zoom is not None:
        lo, hi = (float(v) for v in zoom)
        if not 0.0 < lo <= hi:
            raise ValueError('zoom must be (lo, hi) with 0 < lo <= hi (got %r)' % (zoom,))
        z = uniform(lo, hi)
    if rotate < 0 or trans < 0:
        raise ValueError('rotate and trans must be >= 0 (got %r, %r)' % (rotate, trans))
    if rotate > 0:
        phi = uniform(-rotate, rotate)
    if trans > 0:
        taux, tauy = uniform(-trans, trans) * W, uniform(-trans, trans) * H
    if _get(st_cfg, 'hflip', False):
        sign = torch.where(torch.rand(B, generator=g) < 0.5, -sign, sign)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    cos, sin = torch.cos(phi), torch.sin(phi)
    a, b = cos * sign / z, -sin / z
    c, d = sin * sign / z, cos / z
    tx = cx - (a * cx + b * cy) + taux
    ty = cy - (c * cx + d * cy) + tauy
    return torch.stack([a, b, tx, c, d, ty], 1).to(torch.float32)


def theta_from_augment(params):
    """The theta of a BatchAugment geometry (arflow_amd.augment.AugmentParams: crop window, flip, optional align_corners=False
    resize) -> float32 [B,6]: output pixel x' of the augmented image is source column x1 + xc (x1 + tw - 1 - xc under a flip)
    with xc = (x' + 1/2) tw / w - 1/2, rows alike without the flip.  ar_transform(theta, flow=gt, out_hw=params.out_hw) then
    carries a ground-truth flow of the source's size along with the images (exactly without the resize; with it up to the
    resize's clamp of xc at the first and last half pixel)."""
    if not isinstance(params, AugmentParams):
        raise ValueError('params must be an AugmentParams (augment.draw_params makes one)')
    th, tw = params.crop_hw
    h, w = params.out_hw
    rx, ry = tw / float(w), th / float(h)
    ox, oy = 0.5 * rx - 0.5, 0.5 * ry - 0.5
    x1, y1, flip = params.x1.double(), params.y1.double(), params.flip
    a = torch.where(flip, torch.full_like(x1, -rx), torch.full_like(x1, rx))
    tx = torch.where(flip, x1 + (tw - 1) - ox, x1 + ox)
    zero = torch.zeros_like(x1)
    return torch.stack([a, zero, tx, zero, zero + ry, y1 + oy], 1).to(torch.float32)


def _check_theta(theta, B):
    if not isinstance(theta, torch.Tensor) or theta.dtype != torch.float32 or tuple(theta.shape) != (B, 6):
        raise ValueError('theta must be a float32 [%d,6] tensor (got %s %s)'
                         % (B, getattr(theta, 'dtype', type(theta).__name__), tuple(getattr(theta, 'shape', ()))))
    host = theta.detach().cpu()  # [B,6] floats: the one small copy the singular check needs
    if not torch.isfinite(host).all():
        raise ValueError('theta must be finite')
    det32 = host[:, 0] * host[:, 4] - host[:, 1] * host[:, 3]  # the kernel's own fp32 operations
    host = host.double()
    bad = (det32 == 0) | (host[:, 0] * host[:, 4] - host[:, 1] * host[:, 3] == 0)
    if bool(bad.any()):
        raise ValueError('theta has a singular row (det L = 0): sample %d' % int(bad.nonzero()[0]))


def _source(name, t, B, C, hw):
    """A float32 GPU tensor [B,C,Hs,Ws] (C None: any C >= 1) -> contiguous, detached."""
    if not isinstance(t, torch.Tensor):
        raise ValueError('%s must be a tensor (got %s)' % (name, type(t).__name__))
    if not t.is_cuda:
        raise _lib.ArflowHipError('arflow_amd.ar runs on the GPU only (%s is a %s tensor); there is no CPU fallback'
                                  % (name, t.device))
    if t.dtype != torch.float32:
        raise ValueError('%s must be float32 (got %s)' % (name, t.dtype))
    want_c = 'C' if C is None else str(C)
    if t.dim() != 4 or min(t.shape) < 1 or (C is not None and t.shape[1] != C) or (B is not None and t.shape[0] != B) \
            or (hw is not None and tuple(t.shape[2:]) != hw):
        raise ValueError('%s must be a non-empty [%s,%s,%s] tensor (got %s)'
                         % (name, 'B' if B is None else B, want_c, 'H,W' if hw is None else '%d,%d' % hw, tuple(t.shape)))
    return t.detach().contiguous()


def ar_transform(theta, img=None, flow=None, noc=None, out_hw=None, mask=True):
    """-> (img_t, flow_t, mask_t), one launch on the current stream; a group whose source is None comes back None, except
    that mask_t of an absent noc is the transform of ones whenever flow is given (the mask of the flow target).
    img [B,C,H,W] any C >= 1, flow [B,2,H,W], noc [B,1,H,W]; theta float32 [B,6] on the CPU or the device.  out_hw: the size
    of the outputs when it is not the sources' (a ground truth carried through a crop or a resize: theta_from_augment).
    mask=False leaves the mask group out when no noc is given.
    The singular-row check reads theta on the host: a theta that lives on the device costs a device-to-host copy and with it
    a synchronisation of the stream in front of the launch; hand over a CPU theta (as TrainStep does) to stay asynchronous."""
    given = [(n, t) for n, t in (('img', img), ('flow', flow), ('noc', noc)) if t is not None]
    if not given:
        raise ValueError('ar_transform needs at least one of img, flow, noc')
    first = given[0][1]
    if not isinstance(first, torch.Tensor) or first.dim() != 4:
        raise ValueError('%s must be a [B,C,H,W] tensor' % given[0][0])
    B, hw = int(first.shape[0]), tuple(int(v) for v in first.shape[2:])
    _check_theta(theta, B)
    img = None if img is None else _source('img', img, B, None, hw)
    flow = None if flow is None else _source('flow', flow, B, 2, hw)
    noc = None if noc is None else _source('noc', noc, B, 1, hw)
    dev = first.device
    for n, t in given:
        if t.device != dev:
            raise ValueError('%s is on %s, %s on %s' % (n, t.device, given[0][0], dev))
    H, W = hw if out_hw is None else _size(out_hw, 'out_hw')
    C = 0 if img is None else int(img.shape[1])
    img_t = None if img is None else torch.empty(B, C, H, W, device=dev, dtype=torch.float32)
    flow_t = None if flow is None else torch.empty(B, 2, H, W, device=dev, dtype=torch.float32)
    mask_t = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32) if (noc is not None or (flow is not None and mask)) else None
    with torch.cuda.device_of(first):
        th = theta.detach().to(dev).contiguous()
        _call('arflow_ar_transform', _p(th), _p(img), _p(img_t), C, _p(flow), _p(flow_t), _p(noc), _p(mask_t), B, hw[0], hw[1],
              H, W, _stream(), key=(B, C, hw[0], hw[1], H, W, flow is not None, mask_t is not None))
    return img_t, flow_t, mask_t


def _loss_args(pred, flow_t, mask, eps, q):
    eps, q = float(eps), float(q)
    if not (math.isfinite(eps) and math.isfinite(q)) or eps < 0 or q <= 0:
        raise ValueError('ar_loss needs eps >= 0 and q > 0 (got eps %r, q %r)' % (eps, q))
    if q < 1 and eps == 0:
        raise ValueError('ar_loss with q < 1 needs eps > 0: the gradient is unbounded where pred == flow_t (got q %r)' % (q,))
    if not isinstance(pred, torch.Tensor) or pred.dim() != 4 or pred.shape[1] != 2 or min(pred.shape) < 1:
        raise ValueError('pred must be a non-empty [B,2,H,W] tensor (got %s)' % (tuple(getattr(pred, 'shape', ())),))
    B, _, H, W = (int(v) for v in pred.shape)
    for name, t, C in (('pred', pred, 2), ('flow_t', flow_t, 2), ('mask', mask, 1)):
        if t is None and name == 'mask':
            continue
        _source(name, t, B, C, (H, W))
        if t.device != pred.device:
            raise ValueError('%s is on %s, pred on %s' % (name, t.device, pred.device))
    return B, H, W, eps, q


class _ArLoss(Function):
    """apply(pred, flow_t, mask, eps, q) -> the 0-d float64 loss: ONE node, two launches forward (partials, fold) and one
    backward.  The two sums become the loss inside the node (four scalar operations, no graph), so autograd sees one edge."""

    @staticmethod
    def forward(ctx, pred, flow_t, mask, eps, q):
        B, H, W, eps, q = _loss_args(pred, flow_t, mask, eps, q)
        pred, flow_t = pred.detach().contiguous(), flow_t.detach().contiguous()
        mask = None if mask is None else mask.detach().contiguous()
        parts = _lib.load().arflow_ar_loss_partials(B, H, W)
        _lib.check(min(parts, 0), 'arflow_ar_loss_partials')
        work = torch.empty(2 * parts, device=pred.device, dtype=torch.float64)
        sums = torch.empty(2, device=pred.device, dtype=torch.float64)
        with torch.cuda.device_of(pred):
            _call('arflow_ar_loss_fwd', _p(pred), _p(flow_t), _p(mask), _p(work), _p(sums), B, H, W, eps, q, _stream(),
                  key=(B, H, W, q == 1.0))
        n = float(B * H * W)
        # sums = (sum (|pred - flow_t| + eps)^q mask, sum mask); the mask sum is the mean over the ranks under
        # ARFLOW_GLOBAL_LOSS_NORM (ddp.global_denominator), as MvLoss and unFlowLoss treat theirs
        scale = (0.5 / n) / (global_denominator(sums[1]) / n + 1e-7)
        ctx.save_for_backward(pred, flow_t, mask, scale)
        ctx.cfg = (B, H, W, eps, q)
        return sums[0] * scale

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        if ctx.needs_input_grad[1]:
            raise NotImplementedError('no gradient with respect to the transformed flow flow_t')
        if ctx.needs_input_grad[2]:
            raise NotImplementedError('no gradient with respect to the mask')
        pred, flow_t, mask, scale = ctx.saved_tensors
        B, H, W, eps, q = ctx.cfg
        g0 = (gout.to(torch.float64) * scale).reshape(1)
        gpred = torch.empty_like(pred)
        with torch.cuda.device_of(pred):
            _call('arflow_ar_loss_bwd', _p(pred), _p(flow_t), _p(mask), _p(g0), _p(gpred), B, H, W, eps, q, _stream(),
                  key=(B, H, W, q == 1.0, 'bwd'))
        return gpred, None, None, None, None


def ar_loss(pred, flow_t, mask=None, eps=0.0, q=1.0):
    """-> the 0-d float64 loss of the module docstring; differentiable in pred alone (a gradient request for flow_t or mask
    raises NotImplementedError).  pred, flow_t [B,2,H,W], mask [B,1,H,W] or None (ones); q < 1 needs eps > 0."""
    return _ArLoss.apply(pred, flow_t, mask, eps, q)
