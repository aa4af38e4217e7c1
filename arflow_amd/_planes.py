"""What the variational-family modules (lowrank, mixture, gauss_pyr, mse, the band half of triag_solve) share on the host
side: the plane-layout rule their kernels take, the check of a small dense tensor, the normalisation
of an incoming gradient, the float64 work buffer, and saving a tuple that may hold None.  `module` is the caller's
``__name__``: it is what the "runs on the GPU only" message names.
"""
import torch

from . import _lib


def check_planes(module, name, t, shape):
    """A [n,C,M,N] fp32 GPU tensor whose items are dense (any batch stride) -> its batch stride."""
    if not isinstance(t, torch.Tensor):
        raise ValueError('%s must be a tensor (got %s)' % (name, type(t).__name__))
    if not t.is_cuda:
        raise _lib.ArflowHipError('%s runs on the GPU only (%s is a %s tensor); there is no CPU fallback'
                                  % (module, name, t.device))
    if t.dtype != torch.float32:
        raise ValueError('%s must be float32 (got %s)' % (name, t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise ValueError('%s must be %s (got %s)' % (name, tuple(shape), tuple(t.shape)))
    n, C, M, N = shape
    st = t.stride()
    if (N > 1 and st[3] != 1) or (M > 1 and st[2] != N) or (C > 1 and st[1] != M * N) or (n > 1 and st[0] < C * M * N):
        raise ValueError('%s must be contiguous or a channel slice of a contiguous tensor' % name)
    return st[0] if n > 1 else C * M * N


def check_small(module, name, t, shape, dtype, like):
    """A small dense tensor (weights, comp, logpdf gradients) on the device of `like`, the mean -> contiguous."""
    if not isinstance(t, torch.Tensor):
        raise ValueError('%s must be a tensor (got %s)' % (name, type(t).__name__))
    if not t.is_cuda:
        raise _lib.ArflowHipError('%s runs on the GPU only (%s is a %s tensor); there is no CPU fallback'
                                  % (module, name, t.device))
    if t.dtype != dtype:
        raise ValueError('%s must be %s (got %s)' % (name, dtype, t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise ValueError('%s must be %s (got %s)' % (name, tuple(shape), tuple(t.shape)))
    if t.device != like.device:
        raise ValueError('%s is on %s, mean on %s' % (name, t.device, like.device))
    return t.contiguous()


def plane_dense(g, shape):
    """An incoming [n,C,M,N] gradient as check_planes takes it: g itself when its rows, planes and channels are dense, else
    g.contiguous() -- also a gradient expanded along the batch (stride 0), as a sum over the samples sends."""
    n, C, M, N = shape
    st = g.stride()
    if st[3] != 1 or st[2] != N or st[1] != M * N or (n > 1 and st[0] < C * M * N):
        return g.contiguous()
    return g


def work_buffer(fn_name, dims, device):
    """The float64 work buffer of a family: its size from the library's `fn_name`(*dims), a negative size raised as the
    error code it is."""
    n = getattr(_lib.load(), fn_name)(*dims)
    _lib.check(min(n, 0), fn_name)
    return torch.empty(n, device=device, dtype=torch.float64)


def save_optional(ctx, tensors, extra=()):
    """save_for_backward of `tensors`, any of which may be None, followed by the tensors of `extra` (none of them None)."""
    ctx.save_for_backward(*[x for x in tensors if x is not None], *extra)
    ctx.none = [x is None for x in tensors]


def load_optional(ctx):
    """-> (tensors with their Nones back in place, list of the extra tensors)."""
    saved = list(ctx.saved_tensors)
    return [None if is_none else saved.pop(0) for is_none in ctx.none], saved
