"""The fused ground-truth residual of MseLoss on the native kernels of csrc/mse.hip: resize_flow of
the target, S reparameterised samples of the level's diagonal Gaussian (or samples the 4-neighbour samplers wrote), their
squared error and the sums the entropy and off-diagonal terms need, in ONE call; the adjoint of all of it in one call.

net [B,C,h,w]: mean 0:2, log_diag 2:4, and in the given-z mode left 4:6 (its last column unused) and over 6:8 (its last row
unused).  target [B,2,H,W], any H, W >= 1.  eps / z [S B,2,h,w], sample s of item b at index s B + b.
    sums = (sum r^2, sum log_diag, sum left^2, sum over^2)      float64 [4], r = z - resize_flow(target, (h, w))
Everything is fp32 (sums float64) and on the GPU: a CPU tensor raises ArflowHipError, a wrong dtype, shape or layout raises
ValueError naming the argument.  net, target, eps and z may be channel slices of wider tensors (rows, planes and channels
dense, any batch stride): they are passed to the kernels in place.
"""
from functools import partial

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._planes import check_planes, work_buffer
from .functional import _call, _p, _stream

__all__ = ['mse_sums', 'resize_flow', 'MODE_COV', 'MODE_INV', 'MODE_GIVEN']

MODE_COV, MODE_INV, MODE_GIVEN = 0, 1, 2
MAX_SAMPLES = 65535  # S B

# the plane-layout rule (_planes.py); this module's checks have always reported under the pyramid sampler's name
_check = partial(check_planes, 'arflow_amd.gauss_pyr')


def _dims(net, target, ez, S, mode):
    """-> (B, C, h, w, H, W, net_bs, target_bs, ez_bs), everything checked."""
    S, mode = int(S), int(mode)
    if mode not in (MODE_COV, MODE_INV, MODE_GIVEN):
        raise ValueError('mode must be 0 (covariance), 1 (inv_cov) or 2 (given z) (got %r)' % (mode,))
    if S < 1:
        raise ValueError('n_samples must be >= 1 (got %r)' % (S,))
    if not isinstance(net, torch.Tensor) or net.dim() != 4 or min(net.shape) < 1:
        raise ValueError('net must be a non-empty [B,C,h,w] tensor (got %s)' % (tuple(getattr(net, 'shape', ())),))
    B, C, h, w = (int(v) for v in net.shape)
    if mode == MODE_GIVEN and (C < 8 or h < 2 or w < 2):
        raise ValueError('the 4-neighbour modes need net [B,>=8,>=2,>=2] (got %s)' % (tuple(net.shape),))
    if C < 4:
        raise ValueError('net must have at least 4 channels: mean and log_diag (got %s)' % (tuple(net.shape),))
    if not isinstance(target, torch.Tensor) or target.dim() != 4 or target.shape[0] != B or target.shape[1] != 2 \
            or min(target.shape) < 1:
        raise ValueError('target must be [%d,2,H,W] for net %s (got %s)' % (B, tuple(net.shape),
                                                                            tuple(getattr(target, 'shape', ()))))
    if S * B > MAX_SAMPLES:
        raise ValueError('n_samples * B must be <= %d (got %d * %d)' % (MAX_SAMPLES, S, B))
    H, W = int(target.shape[2]), int(target.shape[3])
    nb = _check('net', net, (B, C, h, w))
    tb = _check('target', target, (B, 2, H, W))
    eb = _check('z' if mode == MODE_GIVEN else 'eps', ez, (S * B, 2, h, w))
    for name, t in (('target', target), ('z' if mode == MODE_GIVEN else 'eps', ez)):
        if t.device != net.device:
            raise ValueError('%s is on %s, net on %s' % (name, t.device, net.device))
    return B, C, h, w, H, W, nb, tb, eb


def _fwd(net, target, ez, S, mode, align_corners, sums=None):
    """One call (map launch + fold launch) -> sums float64 [4]."""
    B, C, h, w, H, W, nb, tb, eb = _dims(net, target, ez, S, mode)
    work = work_buffer('arflow_mse_work_size', (B, h, w), net.device)
    if sums is None:
        sums = torch.empty(4, device=net.device, dtype=torch.float64)
    with torch.cuda.device_of(net):
        _call('arflow_mse_fwd', _p(net), nb, C, _p(target), tb, H, W, _p(ez), eb, B, int(S), h, w, int(mode),
              int(bool(align_corners)), _p(work), _p(sums), _stream(), key=(B, int(S), h, w, int(mode)))
    return sums


def _bwd(net, target, ez, S, mode, align_corners, gsums, gnet=None, gz=None):
    """One launch -> (gnet [B,C,h,w], every channel stored; gz [S B,2,h,w] in the given-z mode, else None)."""
    B, C, h, w, H, W, nb, tb, eb = _dims(net, target, ez, S, mode)
    gsums = gsums.contiguous()
    if tuple(gsums.shape) != (4,) or gsums.dtype != torch.float64 or not gsums.is_cuda:
        raise ValueError('gsums must be a float64 [4] GPU tensor')
    if gnet is None:
        gnet = torch.empty(B, C, h, w, device=net.device, dtype=torch.float32)
    gb = _check('gnet', gnet, (B, C, h, w))
    zb = 0
    if mode == MODE_GIVEN:
        if gz is None:
            gz = torch.empty(int(S) * B, 2, h, w, device=net.device, dtype=torch.float32)
        zb = _check('gz', gz, (int(S) * B, 2, h, w))
    else:
        gz = None
    with torch.cuda.device_of(net):
        _call('arflow_mse_bwd', _p(net), nb, C, _p(target), tb, H, W, _p(ez), eb, _p(gsums), _p(gnet), gb, _p(gz), zb, B, int(S),
              h, w, int(mode), int(bool(align_corners)), _stream(), key=(B, int(S), h, w, int(mode), 'bwd'))
    return gnet, gz


class _MseSums(Function):
    """apply(net, target, ez, S, mode, align_corners) -> sums: ONE node; its backward is one launch that stores the whole
    gradient of net (and of z in the given-z mode), so autograd sees neither a slice nor a repeat backward."""

    @staticmethod
    def forward(ctx, net, target, ez, S, mode, align_corners):
        sums = _fwd(net, target, ez, S, mode, align_corners)
        ctx.save_for_backward(net, target, ez)
        ctx.cfg = (int(S), int(mode), bool(align_corners))
        return sums

    @staticmethod
    @once_differentiable
    def backward(ctx, gsums):
        S, mode, align = ctx.cfg
        if ctx.needs_input_grad[1]:
            raise NotImplementedError('no gradient with respect to the target flow')
        if mode != MODE_GIVEN and ctx.needs_input_grad[2]:
            raise NotImplementedError('no gradient with respect to the noise eps')
        net, target, ez = ctx.saved_tensors
        gnet, gz = _bwd(net, target, ez, S, mode, align, gsums)
        return gnet, None, gz, None, None, None


def mse_sums(net, target, ez, n_samples=1, mode=MODE_COV, align_corners=False):
    """-> float64 [4]: (sum (z - gt)^2, sum log_diag, sum left^2, sum over^2).  ez is the noise eps in the sampling modes
    (MODE_COV: z = mean + exp(log_diag) eps, MODE_INV: z = mean + exp(-log_diag) eps) and the samples z themselves in
    MODE_GIVEN.  Gradients to net (and to z in MODE_GIVEN) only."""
    return _MseSums.apply(net, target, ez, n_samples, mode, align_corners)


def resize_flow(flow, new_shape, align_corners=False):
    """utils/flow_utils.py:110-118 in one launch: the bilinear resize of a [B,2,H,W] flow to new_shape = (h, w) with channel 0
    divided by W / w and channel 1 by H / h.  No autograd."""
    if not isinstance(flow, torch.Tensor) or flow.dim() != 4 or flow.shape[1] != 2 or min(flow.shape) < 1:
        raise ValueError('flow must be a non-empty [B,2,H,W] tensor (got %s)' % (tuple(getattr(flow, 'shape', ())),))
    h, w = (int(v) for v in new_shape)
    if h < 1 or w < 1:
        raise ValueError('new_shape must be positive (got %r)' % (tuple(new_shape),))
    B, _, H, W = (int(v) for v in flow.shape)
    flow = flow.detach()
    fb = _check('flow', flow, (B, 2, H, W))
    out = torch.empty(B, 2, h, w, device=flow.device, dtype=torch.float32)
    with torch.cuda.device_of(flow):
        _call('arflow_resize_flow', _p(flow), fb, H, W, _p(out), 2 * h * w, B, h, w, int(bool(align_corners)), _stream(),
              key=(B, H, W, h, w))
    return out
