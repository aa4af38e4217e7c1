"""Flow rendering and original-size restore on the native kernels of csrc/render.hip.

    restore(flow, out_hw, entropy=None, stats=False)   inference.py:98-107: [B,2,h,w] -> NHWC [B,H,W,2] at the original size
    flow_stats(flow, layout='nchw')                    per sample (max(|u|,|v|), max(u,v)), [B,2]
    flow_rgb(flow, mode='rgb'|'wheel', ...)            uint8 [B,H,W,3]: np_flow2rgb / flow_to_image of utils/flow_utils.py
    torch_flow2rgb(tensor)                             drop-in: float [B,3,H,W], per-sample absmax normalisation
    flow_to_image(flow_hw2, max_flow=256)              drop-in for one [H,W,2] array or tensor
    entropy_image(entropy, as_uint8=True)              trainer/uflow_elbo_trainer.py:259-262

Everything is fp32 and on the GPU: a CPU tensor raises ArflowHipError, a wrong dtype, shape or layout raises ValueError
naming the argument.  A flow or entropy may be a channel slice of a wider tensor; it is read in place.  No autograd: a
tensor that requires grad is detached.
"""
from collections import namedtuple
from functools import partial

import numpy as np
import torch

from . import _lib
from ._planes import check_planes
from .functional import _call, _p, _stream

__all__ = ['restore', 'flow_stats', 'flow_rgb', 'torch_flow2rgb', 'flow_to_image', 'entropy_image', 'Restored']

LAYOUT_NCHW, LAYOUT_NHWC = 0, 1
OUT_U8, OUT_F32 = 0, 1
MODES = {'rgb': 0, 'wheel': 1}
MAX_DIM = 65535

Restored = namedtuple('Restored', ['flow', 'entropy', 'stats'])

_check = partial(check_planes, 'arflow_amd.render')


def _flow_arg(name, flow, layout):
    """-> (detached tensor, batch stride, layout code, B, H, W)"""
    if not isinstance(flow, torch.Tensor) or flow.dim() != 4 or min(flow.shape) < 1:
        raise ValueError('%s must be a non-empty 4-d tensor (got %s)' % (name, tuple(getattr(flow, 'shape', ()))))
    flow = flow.detach()
    if layout == 'nchw':
        if flow.shape[1] != 2:
            raise ValueError('%s must be [B,2,H,W] (got %s)' % (name, tuple(flow.shape)))
        B, _, H, W = (int(v) for v in flow.shape)
        return flow, _check(name, flow, (B, 2, H, W)), LAYOUT_NCHW, B, H, W
    if layout != 'nhwc':
        raise ValueError("layout must be 'nchw' or 'nhwc' (got %r)" % (layout,))
    if flow.shape[3] != 2:
        raise ValueError('%s must be [B,H,W,2] (got %s)' % (name, tuple(flow.shape)))
    B, H, W, _ = (int(v) for v in flow.shape)
    if not flow.is_cuda:
        raise _lib.ArflowHipError('arflow_amd.render runs on the GPU only (%s is a %s tensor); there is no CPU fallback'
                                  % (name, flow.device))
    if flow.dtype != torch.float32:
        raise ValueError('%s must be float32 (got %s)' % (name, flow.dtype))
    st = flow.stride()
    if st[3] != 1 or (W > 1 and st[2] != 2) or (H > 1 and st[1] != 2 * W) or (B > 1 and st[0] < 2 * H * W):
        raise ValueError('%s must be contiguous or a batch slice of a contiguous tensor' % name)
    return flow, (st[0] if B > 1 else 2 * H * W), LAYOUT_NHWC, B, H, W


def _dims_ok(*dims):
    if max(dims) > MAX_DIM:
        raise ValueError('B, H and W must be <= %d (got %r)' % (MAX_DIM, dims))


def restore(flow, out_hw, entropy=None, stats=False):
    """flow [B,2,h,w] (+ entropy [B,2,h,w]) -> Restored(flow [B,H,W,2], entropy [B,H,W,2] or None, stats [B,2] or None):
    the half-pixel bilinear resize to out_hw = (H, W), the flow times (W / w, H / h), the entropy plus
    (2 log W - 2 log w, 2 log H - 2 log h); stats are (max(|u|,|v|), max(u,v)) per sample of the restored flow."""
    H, W = (int(v) for v in out_hw)
    if H < 1 or W < 1:
        raise ValueError('out_hw must be positive (got %r)' % (tuple(out_hw),))
    flow, fb, _, B, h, w = _flow_arg('flow', flow, 'nchw')
    _dims_ok(B, h, w, H, W)
    eb = 0
    if entropy is not None:
        if not isinstance(entropy, torch.Tensor):
            raise ValueError('entropy must be a tensor (got %s)' % type(entropy).__name__)
        entropy = entropy.detach()
        eb = _check('entropy', entropy, (B, 2, h, w))
        if entropy.device != flow.device:
            raise ValueError('entropy is on %s, flow on %s' % (entropy.device, flow.device))
    out = torch.empty(B, H, W, 2, device=flow.device, dtype=torch.float32)
    out_e = torch.empty(B, H, W, 2, device=flow.device, dtype=torch.float32) if entropy is not None else None
    st = torch.empty(B, 2, device=flow.device, dtype=torch.float32) if stats else None
    with torch.cuda.device_of(flow):
        _call('arflow_restore_out', _p(flow), fb, _p(entropy), eb, _p(out), _p(out_e), _p(st), B, h, w, H, W, _stream(),
              key=(B, h, w, H, W))
    return Restored(out, out_e, st)


def flow_stats(flow, layout='nchw'):
    """-> [B,2] float32: per sample (max(|u|, |v|), max(u, v))."""
    flow, fb, lay, B, H, W = _flow_arg('flow', flow, layout)
    _dims_ok(B, H, W)
    st = torch.empty(B, 2, device=flow.device, dtype=torch.float32)
    with torch.cuda.device_of(flow):
        _call('arflow_flow_stats', _p(flow), fb, lay, _p(st), B, H, W, _stream(), key=(B, H, W, lay))
    return st


def _render(flow, fb, lay, B, H, W, scale, scale_stride, mode, out_kind):
    if out_kind == OUT_U8:
        out = torch.empty(B, H, W, 3, device=flow.device, dtype=torch.uint8)
    else:
        out = torch.empty(B, 3, H, W, device=flow.device, dtype=torch.float32)
    with torch.cuda.device_of(flow):
        _call('arflow_flow_render', _p(flow), fb, lay, _p(scale), scale_stride, _p(out), out_kind, mode, B, H, W, _stream(),
              key=(B, H, W, lay, mode, out_kind))
    return out


def _scale_for(flow, fb, lay, B, H, W, mode, max_value, max_flow, stats):
    """-> (tensor, stride): the renderer reads sample b's scale at tensor[b * stride]."""
    fixed = max_value if mode == 'rgb' else (None if max_flow is None else max(float(max_flow), 1.0))
    if fixed is not None:
        return torch.full((1,), float(fixed), device=flow.device, dtype=torch.float32), 0
    if stats is None:
        stats = torch.empty(B, 2, device=flow.device, dtype=torch.float32)
        with torch.cuda.device_of(flow):
            _call('arflow_flow_stats', _p(flow), fb, lay, _p(stats), B, H, W, _stream(), key=(B, H, W, lay))
    elif tuple(stats.shape) != (B, 2) or stats.dtype != torch.float32 or not stats.is_contiguous() or stats.device != flow.device:
        raise ValueError('stats must be the contiguous float32 [%d,2] tensor of restore / flow_stats' % B)
    return stats[:, (0 if mode == 'rgb' else 1):], 2


def flow_rgb(flow, mode='rgb', max_value=None, max_flow=256, layout='nchw', stats=None, as_uint8=True):
    """-> uint8 [B,H,W,3] (as_uint8=False: float [B,3,H,W]).  mode 'rgb' is np_flow2rgb, normalised by max_value or, for None,
    by each sample's max(|u|,|v|); mode 'wheel' is flow_to_image, normalised by max(max_flow, 1) or, for None, by each sample's
    max(u, v).  stats: the [B,2] tensor restore(..., stats=True) or flow_stats returned for this flow, to skip that pass.
    A scale that is not positive and finite renders white."""
    if mode not in MODES:
        raise ValueError("mode must be 'rgb' or 'wheel' (got %r)" % (mode,))
    flow, fb, lay, B, H, W = _flow_arg('flow', flow, layout)
    _dims_ok(B, H, W)
    scale, stride = _scale_for(flow, fb, lay, B, H, W, mode, max_value, max_flow, stats)
    return _render(flow, fb, lay, B, H, W, scale, stride, MODES[mode], OUT_U8 if as_uint8 else OUT_F32)


def torch_flow2rgb(tensor):
    """utils/flow_utils.py:99-107 without the trip through the host: [B,2,H,W] -> float [B,3,H,W] on the flow's device."""
    return flow_rgb(tensor, 'rgb', as_uint8=False)


def flow_to_image(flow, max_flow=256):
    """utils/flow_utils.py:67-81 for one [H,W,2] flow -> uint8 [H,W,3]; a numpy array comes back as a numpy array."""
    is_np = isinstance(flow, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32)).cuda() if is_np else flow
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != 2:
        raise ValueError('flow must be [H,W,2] (got %s)' % (tuple(getattr(t, 'shape', ())),))
    out = flow_rgb(t.unsqueeze(0), 'wheel', max_flow=max_flow, layout='nhwc')[0]
    return out.cpu().numpy() if is_np else out


def entropy_image(entropy, as_uint8=True):
    """entropy [B,C,H,W] (C <= 16) -> the summed map, shifted and scaled to [0,1] by the minimum and maximum of the whole batch:
    uint8 [B,H,W] (trunc(255 .)) or, as_uint8=False, float [B,1,H,W].  A constant map renders 0."""
    if not isinstance(entropy, torch.Tensor) or entropy.dim() != 4 or min(entropy.shape) < 1:
        raise ValueError('entropy must be a non-empty [B,C,H,W] tensor (got %s)' % (tuple(getattr(entropy, 'shape', ())),))
    entropy = entropy.detach()
    B, C, H, W = (int(v) for v in entropy.shape)
    if C > 16:
        raise ValueError('entropy must have at most 16 channels (got %d)' % C)
    xb = _check('entropy', entropy, (B, C, H, W))
    _dims_ok(B, H, W)
    mm = torch.empty(2, device=entropy.device, dtype=torch.float32)
    out = torch.empty((B, H, W) if as_uint8 else (B, 1, H, W), device=entropy.device,
                      dtype=torch.uint8 if as_uint8 else torch.float32)
    with torch.cuda.device_of(entropy):
        _call('arflow_scalar_stats', _p(entropy), xb, C, _p(mm), B, H, W, _stream(), key=(B, C, H, W))
        _call('arflow_scalar_render', _p(entropy), xb, C, _p(mm), _p(out), OUT_U8 if as_uint8 else OUT_F32, B, H, W, _stream(),
              key=(B, C, H, W, as_uint8))
    return out
