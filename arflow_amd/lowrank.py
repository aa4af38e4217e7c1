"""The low-rank covariance family on the native kernels of csrc/lowrank.hip: the sampler
``reparam_lowrank`` of losses/uflow_elbo_loss.py:180-188 and the Gram log-determinants of its entropy (:362-381).

std [B,2R,h,w]: channel 2k + c is column k of flow component c, 1 <= R <= 16.  Sample s of item b is plane s B + b; the noise
eps [S B,2R,1,1] is one scalar per sample and column.
    z[sB+b,c,p]  = mean[b,c,p] + sum_k std[b,2k+c,p] eps[sB+b,2k+c]
    logdet[b,c]  = log det (U U^T),  U = std[b, c::2] as [R, h w]
Everything is fp32 and on the GPU: a CPU tensor raises ArflowHipError, a wrong dtype, shape or layout raises ValueError naming
the argument.  mean and std may be channel slices of one wider tensor (rows, planes and channels dense, any batch stride): they
are passed to the kernels in place.  h w < R raises ValueError: the Gram matrix is then singular by construction.  A Gram matrix
that is singular to working precision gives NaN for its log-determinant (the reference's torch.logdet: -inf / NaN).
"""
from functools import partial

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._planes import check_planes, load_optional, plane_dense, save_optional, work_buffer
from .functional import _call, _p, _stream

__all__ = ['reparam_lowrank', 'gram_logdet', 'reparam_lowrank_pair', 'RMAX']

RMAX = 16


_check = partial(check_planes, __name__)  # the plane-layout rule (_planes.py) under this module's name


def _std_dims(std):
    """-> (B, R, M, N) of a std tensor, checked as far as its own shape goes."""
    if not isinstance(std, torch.Tensor) or std.dim() != 4:
        raise ValueError('std must be a [B,2R,h,w] tensor')
    B, C, M, N = std.shape
    if C % 2 or not 1 <= C // 2 <= RMAX:
        raise ValueError('std must have 2R channels, 1 <= R <= %d (got %d)' % (RMAX, C))
    if B < 1 or M < 1 or N < 1:
        raise ValueError('std must not be empty (got %s)' % (tuple(std.shape),))
    return B, C // 2, M, N


def _eps_check(eps, S, B, R, std):
    _check('eps', eps, (S * B, 2 * R, 1, 1))
    if eps.device != std.device:
        raise ValueError('eps is on %s, std on %s' % (eps.device, std.device))
    return eps.contiguous()  # (a [n,C,1,1] tensor of any stride: 2R floats per row)


def _sample_fwd(mean, std, eps, S, out):
    """One launch: out[sB+b] = mean[b] + columns(std[b]) eps[sB+b]; out [S B,2,M,N] or such a channel slice."""
    B, R, M, N = _std_dims(std)
    s_bs = _check('std', std, (B, 2 * R, M, N))
    m_bs = _check('mean', mean, (B, 2, M, N))
    if mean.device != std.device:
        raise ValueError('mean is on %s, std on %s' % (mean.device, std.device))
    eps = _eps_check(eps, S, B, R, std)
    z_bs = _check('out', out, (S * B, 2, M, N))
    with torch.cuda.device_of(std):
        _call('arflow_lowrank_sample_fwd', _p(mean), m_bs, _p(std), s_bs, _p(eps), _p(out), z_bs, B, S, R, M, N, _stream(),
              key=(B, S, R, M, N))
    return out


def _logdet_fwd(std, logdet=None, ginv=None):
    """One call (two launches): -> logdet [B,2], ginv [B,2,R,R] (contiguous; allocated when not given)."""
    B, R, M, N = _std_dims(std)
    s_bs = _check('std', std, (B, 2 * R, M, N))
    if M * N < R:
        raise ValueError('std: %d pixels cannot carry %d independent columns (the Gram matrix is singular)' % (M * N, R))
    work = work_buffer('arflow_lowrank_work_size', (B, R, M, N), std.device)
    if logdet is None:
        logdet = torch.empty(B, 2, device=std.device, dtype=torch.float32)
    if ginv is None:
        ginv = torch.empty(B, 2, R, R, device=std.device, dtype=torch.float32)
    with torch.cuda.device_of(std):
        _call('arflow_lowrank_logdet_fwd', _p(std), s_bs, _p(work), _p(logdet), _p(ginv), B, R, M, N, _stream(),
              key=(B, R, M, N))
    return logdet, ginv


def _bwd(std, eps, gZ, ginv, glogdet, S, want_gmean, gmean=None, gstd=None):
    """One launch -> (gmean [B,2,M,N] or None, gstd [B,2R,M,N]).  gZ [S B,2,M,N] and glogdet [B,2] may each be None.
    gmean / gstd: tensors or channel slices to store into."""
    B, R, M, N = _std_dims(std)
    s_bs = _check('std', std, (B, 2 * R, M, N))
    g_bs = 0
    if gZ is not None:
        gZ = plane_dense(gZ, (S * B, 2, M, N))
        g_bs = _check('gZ', gZ, (S * B, 2, M, N))
        eps = _eps_check(eps, S, B, R, std)
    if glogdet is not None:
        glogdet = glogdet.contiguous()
        if tuple(glogdet.shape) != (B, 2) or glogdet.dtype != torch.float32 or not glogdet.is_cuda:
            raise ValueError('glogdet must be a float32 [%d,2] GPU tensor' % B)
        if tuple(ginv.shape) != (B, 2, R, R) or ginv.dtype != torch.float32 or not ginv.is_contiguous():
            raise ValueError('ginv must be a contiguous float32 [%d,2,%d,%d] tensor' % (B, R, R))
    if gstd is None:
        gstd = torch.empty(B, 2 * R, M, N, device=std.device, dtype=torch.float32)
    gs_bs = _check('gstd', gstd, (B, 2 * R, M, N))
    gm_bs = 0
    if want_gmean:
        if gmean is None:
            gmean = torch.empty(B, 2, M, N, device=std.device, dtype=torch.float32)
        gm_bs = _check('gmean', gmean, (B, 2, M, N))
    else:
        gmean = None
    with torch.cuda.device_of(std):
        _call('arflow_lowrank_bwd', _p(std), s_bs, _p(eps if gZ is not None else None), _p(gZ), g_bs,
              _p(ginv if glogdet is not None else None), _p(glogdet), _p(gmean), gm_bs, _p(gstd), gs_bs, B, S, R, M, N,
              _stream(), key=(B, S, R, M, N))
    return gmean, gstd


class _LowRank(Function):
    """For `ndir` independent (mean, std, eps): the samples side by side in ONE [S B, 2 ndir, M, N] tensor (direction d in
    channels 2d, 2d + 1) and the log-determinants [ndir, B, 2], behind one node: apply(S, ndir, sample, logdet, mean_0, std_0,
    eps_0, mean_1, ...).  Forward: one sampler launch and one log-det call per direction; backward: ONE arflow_lowrank_bwd per
    direction, which reads std and the samples' gradient once for both terms.  sample / logdet False: that output is None and
    its launches do not run (mean / eps are then not read)."""

    @staticmethod
    def forward(ctx, S, ndir, sample, logdet, *t):
        S, ndir = int(S), int(ndir)
        if S < 1:
            raise ValueError('nsamples must be >= 1 (got %r)' % (S,))
        B, R, M, N = _std_dims(t[1])
        dev = t[1].device
        Z = torch.empty(S * B, 2 * ndir, M, N, device=dev, dtype=torch.float32) if sample else None
        ld = torch.empty(ndir, B, 2, device=dev, dtype=torch.float32) if logdet else None
        ginvs = []
        for d in range(ndir):
            mean, std, eps = t[3 * d:3 * d + 3]
            if _std_dims(std) != (B, R, M, N):
                raise ValueError('std of direction %d must be %s (got %s)' % (d, (B, 2 * R, M, N), tuple(std.shape)))
            if sample:
                _sample_fwd(mean, std, eps, S, Z[:, 2 * d:2 * d + 2])
            if logdet:
                ginvs.append(_logdet_fwd(std, logdet=ld[d])[1])
        save_optional(ctx, t, ginvs)
        ctx.cfg = (S, ndir, bool(sample), bool(logdet))
        ctx.set_materialize_grads(False)
        return Z, ld

    @staticmethod
    @once_differentiable
    def backward(ctx, gZ, gld):
        S, ndir, sample, logdet = ctx.cfg
        t, ginvs = load_optional(ctx)
        grads = []
        for d in range(ndir):
            mean, std, eps = t[3 * d:3 * d + 3]
            need = ctx.needs_input_grad[4 + 3 * d:4 + 3 * d + 3]
            if need[2]:
                raise NotImplementedError('no gradient with respect to the noise eps')
            g = gZ[:, 2 * d:2 * d + 2] if gZ is not None else None
            gl = gld[d] if gld is not None else None
            if g is None and gl is None:
                grads += [None, None, None]
                continue
            gmean, gstd = _bwd(std, eps, g, ginvs[d] if logdet else None, gl, S, mean is not None and need[0])
            grads += [gmean, gstd, None]
        return (None, None, None, None) + tuple(grads)


def _draw(std, nsamples):
    B, R, _, _ = _std_dims(std)
    return torch.randn(int(nsamples) * B, 2 * R, 1, 1, device=std.device, dtype=std.dtype)


def reparam_lowrank(mean, std, nsamples=1, eps=None):
    """Reparameterised samples of the low-rank family (losses/uflow_elbo_loss.py:180-188) in ONE launch: mean [B,2,h,w], std
    [B,2R,h,w], eps [nsamples B,2R,1,1] ~ N(0,1), drawn on the device when not given -> [nsamples B,2,h,w].  Gradients to mean
    and std."""
    if eps is None:
        eps = _draw(std, nsamples)
    return _LowRank.apply(nsamples, 1, True, False, mean, std, eps)[0]


def gram_logdet(std):
    """std [B,2R,h,w] -> [B,2]: log det (U_c U_c^T) with U_c = std[b, c::2] as [R, h w], accumulated and factored in float64
    on the device.  Gradient to std: 2 G^-1 U."""
    return _LowRank.apply(1, 1, False, True, None, std, None)[1][0]


def reparam_lowrank_pair(fw, bw, nsamples=1):
    """fw, bw: (mean, std, eps) of the two flow directions -> (flows [nsamples B,4,h,w] with the forward samples in channels
    0:2 and the backward samples in 2:4 -- the layout the pair kernels of the losses take --, logdet [2,B,2]) behind one
    autograd node."""
    return _LowRank.apply(nsamples, 2, True, True, fw[0], fw[1], fw[2], bw[0], bw[1], bw[2])
