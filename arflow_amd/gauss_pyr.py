"""The diagonal Gaussian sampler of ElboLoss over a whole pyramid on the native kernels of csrc/gauss_pyr.hip (DESIGN.md
section 27): losses/elbo_loss.py:17-27 reparam for both directions of every scale, and the sums of the log-variances its
entropy term needs (:117-124), in ONE launch; the adjoint of both in one launch.

nets[i] [B,8,h_i,w_i]: mean_fw 0:2, logvar_fw 2:4, mean_bw 4:6, logvar_bw 6:8 -- the tensor the trainer's cat(fw, bw) makes.
eps[i] [B,4,h_i,w_i]: the forward noise in channels 0:2, the backward noise in 2:4.
    z_i      = mean + exp(logvar / 2) * eps     [B,4,h_i,w_i]: (forward, backward) samples, the flow tensor unFlowLoss takes
    ent[i,d] = sum_{b,c,p} logvar_d             float64 [n,2]
Everything is fp32 (ent float64) and on the GPU: a CPU tensor raises ArflowHipError, a wrong dtype, shape or layout raises
ValueError naming the argument.  Each net / eps may be a channel slice of a wider tensor (rows, planes and channels dense, any
batch stride): it is passed to the kernels in place.  1 <= n <= 6 scales of one batch size.
"""
import ctypes
from functools import partial

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._planes import check_planes, plane_dense, work_buffer
from .functional import _call, _p, _stream

__all__ = ['reparam_pyramid', 'NMAX']

NMAX = 6


_check = partial(check_planes, __name__)  # the plane-layout rule (_planes.py) under this module's name


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[_p(t) for t in ts])


def _longs(v):
    return (ctypes.c_long * len(v))(*v)


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _dims(nets):
    """-> (B, [(h, w)]) of a list of nets, checked as far as their own shapes go."""
    if not isinstance(nets, (list, tuple)) or not 1 <= len(nets) <= NMAX:
        raise ValueError('nets must be a list of 1..%d tensors (got %s)' % (NMAX, len(nets) if isinstance(nets, (list, tuple))
                                                                            else type(nets).__name__))
    B, sizes = None, []
    for i, t in enumerate(nets):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 8:
            raise ValueError('nets[%d] must be a [B,8,h,w] tensor' % i)
        if min(t.shape) < 1:
            raise ValueError('nets[%d] must not be empty (got %s)' % (i, tuple(t.shape)))
        if B is None:
            B = t.shape[0]
        elif t.shape[0] != B:
            raise ValueError('nets[%d] has batch %d, nets[0] has %d' % (i, t.shape[0], B))
        sizes.append((int(t.shape[2]), int(t.shape[3])))
    return int(B), sizes


def _sample_fwd(nets, eps, zs=None, ent=None):
    """One call (sampler launch + fold launch) -> (zs, ent float64 [n,2])."""
    B, sizes = _dims(nets)
    n = len(nets)
    if not isinstance(eps, (list, tuple)) or len(eps) != n:
        raise ValueError('eps must be a list of %d tensors, one per scale' % n)
    dev = nets[0].device if isinstance(nets[0], torch.Tensor) else None
    if zs is None:
        zs = [torch.empty(B, 4, h, w, device=dev, dtype=torch.float32) for h, w in sizes]
    nb = [_check('nets[%d]' % i, t, (B, 8) + sizes[i]) for i, t in enumerate(nets)]
    eb = [_check('eps[%d]' % i, t, (B, 4) + sizes[i]) for i, t in enumerate(eps)]
    zb = [_check('out[%d]' % i, t, (B, 4) + sizes[i]) for i, t in enumerate(zs)]
    for i, t in enumerate(list(nets) + list(eps)):
        if t.device != dev:
            raise ValueError('%s[%d] is on %s, nets[0] on %s' % ('nets' if i < n else 'eps', i % n, t.device, dev))
    hs, ws = _ints([s[0] for s in sizes]), _ints([s[1] for s in sizes])
    work = work_buffer('arflow_gauss_pyr_work_size', (hs, ws, n, B), dev)
    if ent is None:
        ent = torch.empty(n, 2, device=dev, dtype=torch.float64)
    with torch.cuda.device_of(nets[0]):
        _call('arflow_gauss_pyr_sample_fwd', _ptrs(nets), _longs(nb), _ptrs(eps), _longs(eb), _ptrs(zs), _longs(zb), hs, ws, n, B,
              _p(work), _p(ent), _stream(), key=(B, n) + sizes[0])
    return zs, ent


def _sample_bwd(nets, eps, gzs, gent, gnets=None):
    """One launch -> gnets (every channel stored).  gzs: a list with None for an absent gradient, or None; gent: float64 [n,2]
    on the device, or None."""
    B, sizes = _dims(nets)
    n = len(nets)
    dev = nets[0].device
    nb = [_check('nets[%d]' % i, t, (B, 8) + sizes[i]) for i, t in enumerate(nets)]
    eb = [_check('eps[%d]' % i, t, (B, 4) + sizes[i]) for i, t in enumerate(eps)]
    if gnets is None:
        gnets = [torch.empty(B, 8, h, w, device=dev, dtype=torch.float32) for h, w in sizes]
    gb = [_check('gnets[%d]' % i, t, (B, 8) + sizes[i]) for i, t in enumerate(gnets)]
    gz_arr = gz_bs = None
    if gzs is not None and any(g is not None for g in gzs):
        gzs = list(gzs)
        zbs = []
        for i, g in enumerate(gzs):
            if g is None:
                zbs.append(0)
                continue
            h, w = sizes[i]
            g = gzs[i] = plane_dense(g, (B, 4, h, w))
            zbs.append(_check('gz[%d]' % i, g, (B, 4, h, w)))
        gz_arr, gz_bs = _ptrs(gzs), _longs(zbs)
    if gent is not None:
        gent = gent.contiguous()
        if tuple(gent.shape) != (n, 2) or gent.dtype != torch.float64 or not gent.is_cuda:
            raise ValueError('gent must be a float64 [%d,2] GPU tensor' % n)
    hs, ws = _ints([s[0] for s in sizes]), _ints([s[1] for s in sizes])
    with torch.cuda.device_of(nets[0]):
        _call('arflow_gauss_pyr_sample_bwd', gz_arr, gz_bs, _ptrs(nets), _longs(nb), _ptrs(eps), _longs(eb), _p(gent),
              _ptrs(gnets), _longs(gb), hs, ws, n, B, _stream(), key=(B, n) + sizes[0] + ('bwd',))
    return gnets


class _GaussPyramid(Function):
    """apply(n, net_0 .. net_{n-1}, eps_0 .. eps_{n-1}) -> (z_0 .. z_{n-1}, ent): ONE node for the whole pyramid.  Its backward
    is one launch that stores the full 8-channel gradient of every net, so autograd sees neither a slice nor a cat backward."""

    @staticmethod
    def forward(ctx, n, *t):
        n = int(n)
        nets, eps = list(t[:n]), list(t[n:])
        zs, ent = _sample_fwd(nets, eps)
        ctx.save_for_backward(*nets, *eps)
        ctx.n = n
        ctx.set_materialize_grads(False)
        return (*zs, ent)

    @staticmethod
    @once_differentiable
    def backward(ctx, *g):
        n = ctx.n
        if any(ctx.needs_input_grad[1 + n:]):
            raise NotImplementedError('no gradient with respect to the noise eps')
        saved = ctx.saved_tensors
        gzs, gent = g[:n], g[n]
        if gent is None and all(x is None for x in gzs):
            return (None,) * (1 + 2 * n)
        gnets = _sample_bwd(list(saved[:n]), list(saved[n:]), gzs, gent)
        return (None, *gnets) + (None,) * n


def reparam_pyramid(nets, eps=None):
    """nets: list of [B,8,h_i,w_i] (1..6 scales); eps: list of [B,4,h_i,w_i] ~ N(0,1), drawn on the device with torch.randn,
    finest scale first, when not given -> (samples: list of [B,4,h_i,w_i], ent: float64 [n,2] sums of the log-variances of
    the forward / backward direction).  Gradients to the nets only."""
    B, sizes = _dims(nets)
    if eps is None:
        eps = [torch.randn(B, 4, h, w, device=nets[0].device, dtype=torch.float32) for h, w in sizes]
    elif not isinstance(eps, (list, tuple)) or len(eps) != len(nets):
        raise ValueError('eps must be a list of %d tensors, one per scale' % len(nets))
    out = _GaussPyramid.apply(len(nets), *nets, *eps)
    return list(out[:-1]), out[-1]
