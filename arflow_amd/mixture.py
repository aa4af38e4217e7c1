"""The Gaussian-mixture variational family on the native kernels of csrc/mixture.hip: the sampler
``reparam_gmm`` of losses/uflow_elbo_loss.py:159-178, the mixture log-density of its entropy (``gaussian_mixture_log_pdf``,
utils/misc_utils.py:67-101) and the per-pixel Monte-Carlo entropy ``mixture_entropy`` (utils/misc_utils.py:104-132).

mean, log_std [B,2K,h,w]: channel 2k + c is flow component c of mixture component k, 1 <= K <= 4; weights [B,K] (rows >= 0 that
sum to 1); comp [B,S] integers in 0..K-1, the component each sample is drawn from; eps [S B,2,h,w].  Sample s of item b is row
n = s B + b, z = comp[b,s], P = h w:
    flow[n,c,p] = mean[b,2z+c,p] + exp(log_std[b,2z+c,p]) eps[n,c,p]
    A[n,k]      = -sum_p sum_c (log_std[b,2k+c,p] + ((flow[n,c,p] - mean[b,2k+c,p]) / std[b,2k+c,p])^2 / 2)
    logpdf[n]   = (max_k A + log sum_k weights[b,k] exp(A[n,k] - max_k A)) / P
The samples are NOT detached inside logpdf: its gradient reaches mean and log_std through the sample, through the residual of
every component and through the log_std term, and the weights through the log-sum.
Everything is fp32 and on the GPU: a CPU tensor raises ArflowHipError, a wrong dtype, shape or layout raises ValueError naming
the argument.  mean and log_std may be channel slices of one wider tensor (rows, planes and channels dense, any batch stride):
they are passed to the kernels in place.  A value of comp outside 0..K-1 is clamped into the range by the kernels.
"""
from functools import partial

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._planes import check_planes, check_small, load_optional, plane_dense, save_optional, work_buffer
from .functional import _call, _p, _stream

__all__ = ['reparam_gmm', 'gaussian_mixture_log_pdf', 'reparam_gmm_pair', 'mixture_entropy', 'KMAX']

KMAX = 4


_check = partial(check_planes, __name__)  # the plane-layout rule and the small-tensor check (_planes.py) under this
_small = partial(check_small, __name__)   # module's name


def _dims(mean):
    """-> (B, K, M, N) of a mean tensor, checked as far as its own shape goes."""
    if not isinstance(mean, torch.Tensor) or mean.dim() != 4:
        raise ValueError('mean must be a [B,2K,h,w] tensor')
    B, C, M, N = mean.shape
    if C % 2 or not 1 <= C // 2 <= KMAX:
        raise ValueError('mean must have 2K channels, 1 <= K <= %d (got %d)' % (KMAX, C))
    if B < 1 or M < 1 or N < 1:
        raise ValueError('mean must not be empty (got %s)' % (tuple(mean.shape),))
    return B, C // 2, M, N


def _inputs(mean, log_std, comp, eps, S):
    """The checks every entry point shares -> (B, K, M, N, mean_bs, ls_bs, comp, eps_bs)."""
    B, K, M, N = _dims(mean)
    m_bs = _check('mean', mean, (B, 2 * K, M, N))
    l_bs = _check('log_std', log_std, (B, 2 * K, M, N))
    if log_std.device != mean.device:
        raise ValueError('log_std is on %s, mean on %s' % (log_std.device, mean.device))
    comp = _small('comp', comp, (B, S), torch.int64, mean)
    e_bs = _check('eps', eps, (S * B, 2, M, N))
    if eps.device != mean.device:
        raise ValueError('eps is on %s, mean on %s' % (eps.device, mean.device))
    return B, K, M, N, m_bs, l_bs, comp, e_bs


def _sample_fwd(mean, log_std, weights, comp, eps, S, out, logpdf=None):
    """Two launches: out[sB+b] = the samples ([S B,2,M,N] or such a channel slice), and -> (logpdf [S B], resp [S B,K],
    q [S B,K]); logpdf: a contiguous [S B] tensor to store into (allocated when not given)."""
    B, K, M, N, m_bs, l_bs, comp, e_bs = _inputs(mean, log_std, comp, eps, S)
    weights = _small('weights', weights, (B, K), torch.float32, mean)
    z_bs = _check('out', out, (S * B, 2, M, N))
    dev = mean.device
    work = work_buffer('arflow_mixture_work_size', (B, S, K, M, N), dev)
    if logpdf is None:
        logpdf = torch.empty(S * B, device=dev, dtype=torch.float32)
    resp = torch.empty(S * B, K, device=dev, dtype=torch.float32)
    q = torch.empty(S * B, K, device=dev, dtype=torch.float32)
    with torch.cuda.device_of(mean):
        _call('arflow_mixture_sample_fwd', _p(mean), m_bs, _p(log_std), l_bs, _p(eps), e_bs, _p(comp), _p(out), z_bs, _p(work),
              B, S, K, M, N, _stream(), key=(B, S, K, M, N))
        _call('arflow_mixture_logpdf_fwd', _p(work), _p(weights), _p(logpdf), _p(resp), _p(q), B, S, K, M, N, _stream(),
              key=(B, S, K, M, N))
    return logpdf, resp, q


def _bwd(mean, log_std, comp, eps, resp, glogpdf, gZ, S, gmean=None, glog_std=None):
    """One launch -> (gmean, glog_std) [B,2K,M,N].  glogpdf [S B] and gZ [S B,2,M,N] may each be None.  gmean / glog_std:
    tensors or channel slices to store into."""
    B, K, M, N, m_bs, l_bs, comp, e_bs = _inputs(mean, log_std, comp, eps, S)
    g_bs = 0
    if gZ is not None:
        gZ = plane_dense(gZ, (S * B, 2, M, N))
        g_bs = _check('gZ', gZ, (S * B, 2, M, N))
    if glogpdf is not None:
        glogpdf = _small('glogpdf', glogpdf, (S * B,), torch.float32, mean)
        resp = _small('resp', resp, (S * B, K), torch.float32, mean)
    if gmean is None:
        gmean = torch.empty(B, 2 * K, M, N, device=mean.device, dtype=torch.float32)
    if glog_std is None:
        glog_std = torch.empty(B, 2 * K, M, N, device=mean.device, dtype=torch.float32)
    gm_bs = _check('gmean', gmean, (B, 2 * K, M, N))
    gl_bs = _check('glog_std', glog_std, (B, 2 * K, M, N))
    with torch.cuda.device_of(mean):
        _call('arflow_mixture_bwd', _p(mean), m_bs, _p(log_std), l_bs, _p(eps), e_bs, _p(comp),
              _p(resp if glogpdf is not None else None), _p(glogpdf), _p(gZ), g_bs, _p(gmean), gm_bs, _p(glog_std), gl_bs,
              B, S, K, M, N, _stream(), key=(B, S, K, M, N))
    return gmean, glog_std


class _Mixture(Function):
    """For `ndir` independent (mean, log_std, weights, comp, eps): the samples side by side in ONE [S B, 2 ndir, M, N] tensor
    (direction d in channels 2d, 2d + 1) and the log-densities [ndir, S B], behind one node: apply(S, ndir, mean_0, log_std_0,
    weights_0, comp_0, eps_0, mean_1, ...).  log_std_d None: mean_d is the level-2 output [B,4K,M,N] = (means, log-stds) itself,
    and its gradient is ONE tensor whose two halves the backward launch writes.  Forward: one sampler launch and one small
    log-density launch per direction; backward: ONE arflow_mixture_bwd per direction (it recomputes the samples from eps:
    they are not saved), plus the weights' gradient sum_s glogpdf[n] q[n,k] / P in torch."""

    @staticmethod
    def forward(ctx, S, ndir, *t):
        S, ndir = int(S), int(ndir)
        if S < 1:
            raise ValueError('nsamples must be >= 1 (got %r)' % (S,))
        halves = [_Mixture._halves(t[5 * d], t[5 * d + 1]) for d in range(ndir)]
        B, K, M, N = _dims(halves[0][0])
        dev = halves[0][0].device
        Z = torch.empty(S * B, 2 * ndir, M, N, device=dev, dtype=torch.float32)
        lp = torch.empty(ndir, S * B, device=dev, dtype=torch.float32)
        keep = []
        for d in range(ndir):
            mean, log_std = halves[d]
            weights, comp, eps = t[5 * d + 2:5 * d + 5]
            if _dims(mean) != (B, K, M, N):
                raise ValueError('mean of direction %d must be %s (got %s)' % (d, (B, 2 * K, M, N), tuple(mean.shape)))
            _, resp, q = _sample_fwd(mean, log_std, weights, comp, eps, S, Z[:, 2 * d:2 * d + 2], logpdf=lp[d])
            keep += [resp, q]
        save_optional(ctx, t, keep)
        ctx.cfg = (S, ndir)
        ctx.set_materialize_grads(False)
        return Z, lp

    @staticmethod
    def _halves(mean, log_std):
        if log_std is not None:
            return mean, log_std
        if not isinstance(mean, torch.Tensor) or mean.dim() != 4 or mean.shape[1] % 4:
            raise ValueError('net must be a [B,4K,h,w] tensor (means, then log-stds)')
        C = mean.shape[1] // 2
        return mean[:, :C], mean[:, C:]

    @staticmethod
    @once_differentiable
    def backward(ctx, gZ, glp):
        S, ndir = ctx.cfg
        t, saved = load_optional(ctx)
        grads = []
        for d in range(ndir):
            joint = t[5 * d + 1] is None
            mean, log_std = _Mixture._halves(t[5 * d], t[5 * d + 1])
            weights, comp, eps = t[5 * d + 2:5 * d + 5]
            resp, q = saved[2 * d:2 * d + 2]
            need = ctx.needs_input_grad[2 + 5 * d:2 + 5 * d + 5]
            if need[3] or need[4]:
                raise NotImplementedError('no gradient with respect to the component draws or the noise eps')
            g = gZ[:, 2 * d:2 * d + 2] if gZ is not None else None
            gl = glp[d] if glp is not None else None
            if g is None and gl is None:
                grads += [None] * 5
                continue
            B, K, M, N = _dims(mean)
            gmean = glog_std = gnet = gw = None
            if need[0] or need[1]:
                if joint:
                    gnet = torch.empty(B, 4 * K, M, N, device=mean.device, dtype=torch.float32)
                    gmean, glog_std = gnet[:, :2 * K], gnet[:, 2 * K:]
                gmean, glog_std = _bwd(mean, log_std, comp, eps, resp, gl, g, S, gmean, glog_std)
            if need[2] and gl is not None:
                gw = (gl.reshape(S, B, 1) * q.view(S, B, K)).sum(0) / float(M * N)
            grads += [gnet, None, gw, None, None] if joint else [gmean, glog_std, gw, None, None]
        return (None, None) + tuple(grads)


def _draw(mean, weights, nsamples, comp, eps):
    """The draws the reference makes, in its order: torch.multinomial(weights, S, replacement=True), then the normal noise."""
    B, K, M, N = _dims(mean)
    S = int(nsamples)
    if comp is None:
        weights = _small('weights', weights, (B, K), torch.float32, mean)
        comp = torch.multinomial(weights.detach(), S, replacement=True)
    if eps is None:
        eps = torch.randn(S * B, 2, M, N, device=mean.device, dtype=torch.float32)
    return comp, eps


def reparam_gmm(mean, log_std, weights, nsamples=1, comp=None, eps=None):
    """Reparameterised samples of the mixture (losses/uflow_elbo_loss.py:159-178) in one pass: mean, log_std [B,2K,h,w], weights
    [B,K] -> [nsamples B,2,h,w].  The second argument is the LOG standard deviation (the reference passes exp(log_diag): the
    exponential is taken inside the kernel instead of in a pass of its own).  comp [B,nsamples] (int64): the component every
    sample is drawn from, torch.multinomial(weights, nsamples, replacement=True) on the device when not given; eps [nsamples
    B,2,h,w] ~ N(0,1), torch.randn on the device when not given.  Gradients to mean and log_std; none to comp or eps."""
    comp, eps = _draw(mean, weights, nsamples, comp, eps)
    return _Mixture.apply(nsamples, 1, mean, log_std, weights, comp, eps)[0]


def gaussian_mixture_log_pdf(flow, mean, log_std, weights, nsamples=1, comp=None, eps=None):
    """The mixture log-density per pixel count, [nsamples B,1] (utils/misc_utils.py:72-101 with per_pixel=False), of the
    samples the node itself draws from (comp, eps) as reparam_gmm does: `flow` must be None -- the density of an arbitrary flow
    tensor is not implemented (the loss never asks for it; the kernel evaluates the density where it forms the sample).
    -> (flow [nsamples B,2,h,w], logpdf [nsamples B,1]) behind one node: gradients to mean, log_std and weights through both."""
    if flow is not None:
        raise NotImplementedError('gaussian_mixture_log_pdf of a given flow tensor (pass flow=None: the samples are drawn '
                                  'from comp and eps inside the node)')
    comp, eps = _draw(mean, weights, nsamples, comp, eps)
    z, lp = _Mixture.apply(nsamples, 1, mean, log_std, weights, comp, eps)
    return z, lp[0].unsqueeze(1)


def reparam_gmm_pair(fw, bw, nsamples=1):
    """fw, bw: (net, weights, comp, eps) of the two flow directions, net [B,4K,h,w] = the K means then the K log-stds (the
    level-2 output of ComponentNet; it may be a channel slice) -> (flows [nsamples B,4,h,w] with the forward samples in
    channels 0:2 and the backward samples in 2:4 -- the layout the pair kernels of the losses take --, logpdf [2, nsamples B])
    behind one autograd node.  The gradient of each net is one tensor, both halves written by one launch."""
    return _Mixture.apply(nsamples, 2, fw[0], None, fw[1], fw[2], fw[3], bw[0], None, bw[1], bw[2], bw[3])


def mixture_entropy(mean, log_std, weights, n_samples=100, comp=None, eps=None):
    """Per-pixel Monte-Carlo entropy of the mixture (utils/misc_utils.py:104-132) in one launch: for each of n_samples draws a
    component comp[b,i] and noise eps[i B + b], minus the per-pixel mixture log-density of that sample, averaged -> [B,1,h,w]
    on the input's device (the reference allocates its accumulator on the CPU and so fails on a GPU tensor).  comp [B,n_samples]
    (int64) and eps [n_samples B,2,h,w] are drawn on the device when not given.  No gradient."""
    n = int(n_samples)
    if n < 1:
        raise ValueError('n_samples must be >= 1 (got %r)' % (n_samples,))
    B, K, M, N = _dims(mean)
    _check('mean', mean, (B, 2 * K, M, N))
    weights = _small('weights', weights, (B, K), torch.float32, mean).detach()
    comp, eps = _draw(mean, weights, n, comp, eps)
    _, _, _, _, m_bs, l_bs, comp, e_bs = _inputs(mean, log_std, comp, eps, n)
    mean, log_std = mean.detach(), log_std.detach()
    out = torch.empty(B, 1, M, N, device=mean.device, dtype=torch.float32)
    with torch.cuda.device_of(mean):
        _call('arflow_mixture_entropy_map', _p(mean), m_bs, _p(log_std), l_bs, _p(weights), _p(comp), _p(eps), e_bs, _p(out),
              B, n, K, M, N, _stream(), key=(B, n, K, M, N))
    return out
