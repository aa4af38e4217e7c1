"""torch.autograd.Function wrappers over the C ABI (libarflow_hip.so).

Every op here runs ONLY on CUDA(ROCm) fp32 tensors through the hand-written gfx950 kernels; a CPU
tensor, a wrong dtype or a missing library raises.  Outputs are allocated with the torch caching
allocator and kernels are enqueued on ``torch.cuda.current_stream()`` -- no synchronisation.
"""
import contextlib

import torch

from . import _lib
from . import ddp as _ddp

PAD = {'zeros': 0, 'border': 1}
NORM_ARFLOW, NORM_UFLOW = 0, 1


def _need_gpu(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.ArflowHipError('arflow_amd ops run on the GPU only (got a %s tensor); there is no CPU '
                                      'fallback -- the CPU oracle lives in oracle/ and is test-only' % t.device)
        if t.dtype != torch.float32:
            raise _lib.ArflowHipError('arflow_amd ops are fp32 only (got %s)' % t.dtype)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _flow_view(flow):
    """Return (tensor, batch_stride) so that a [B,2,H,W] slice of a wider tensor is used in place."""
    B, two, H, W = flow.shape
    assert two == 2, 'flow must have 2 channels'
    st = flow.stride()
    if st[3] == 1 and st[2] == W and st[1] == H * W and (B == 1 or st[0] >= 2 * H * W):
        return flow, (st[0] if B > 1 else 2 * H * W)
    flow = flow.contiguous()
    return flow, 2 * H * W


_timing = None  # list of (name, key, start_event, end_event) while kernel timing is on


_paused = False


def start_kernel_timing():
    """Bracket every C-ABI launch with HIP events recorded on the launch stream (torch's current
    stream).  Used by bench.py for the per-kernel roofline; off by default."""
    global _timing
    _timing = []


def pause_kernel_timing(paused):
    """Keep the records but stop / resume bracketing launches (bench.py samples a subset of its steps: two
    event records per launch cost ~10 us of host time each, which a launch-bound step feels)."""
    global _paused
    _paused = bool(paused)


def stop_kernel_timing():
    """-> {(name, shape_key): [ms, ...]} ; synchronises."""
    global _timing
    rec, _timing = _timing or [], None
    torch.cuda.synchronize()
    out = {}
    for name, key, e0, e1 in rec:
        out.setdefault((name, key), []).append(e0.elapsed_time(e1))
    return out


SUM_COLS = 4  # ARFLOW_SUM_COLS of include/arflow_hip.h


def _new_sums(device, B, H, W):
    """Per-workgroup partial rows of a reduction kernel over a [B, *, H, W] problem (every row is written by the
    call: no initialisation needed)."""
    rows = _lib.load().arflow_sums_rows(int(B), int(H), int(W))
    if rows <= 0:
        _lib.check(rows, 'arflow_sums_rows')
    return torch.empty(rows * SUM_COLS, device=device, dtype=torch.float32)


def _fold_sums(buf, k):
    """Partial rows -> the k reduced quantities (one tiny reduction kernel, fixed order: reproducible)."""
    return buf.view(-1, SUM_COLS)[:, :k].sum(0)


def _call(name, *args, key=None):
    lib = _lib.load()
    if _timing is not None and key is not None and not _paused:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = getattr(lib, name)(*args)
        e1.record()
        _timing.append((name, key, e0, e1))
    else:
        rc = getattr(lib, name)(*args)
    _lib.check(rc, name)
    _lib.poll_stale_error(lib, name)


def _workspace(name, *args, device):
    """A uint8 tensor of the size the query `name`(*args) answers; a negative answer (an error) raises BEFORE any allocation."""
    nbytes = getattr(_lib.load(), name)(*args)
    if nbytes < 0:
        _lib.check(int(nbytes), name)
    return torch.empty(nbytes, device=device, dtype=torch.uint8)


# ---- deterministic mode ------------------------------------------------------
def set_deterministic(on):
    """Switch the library's process-wide deterministic mode (initial value: ARFLOW_DETERMINISTIC=1); returns the previous
    value.  While it is on, every op whose default kernels end in float atomics runs fixed-order kernels instead and is
    bitwise reproducible; ops that only have an atomic form raise ArflowHipError.  ``torch.use_deterministic_algorithms``
    is NOT consulted: under that flag ATen raises inside the models' own F.interpolate backward."""
    return bool(_lib.load().arflow_set_deterministic(int(bool(on))))


def is_deterministic():
    return bool(_lib.load().arflow_get_deterministic())


@contextlib.contextmanager
def deterministic(on=True):
    """``with AF.deterministic():`` -- the mode for the duration of the block; the previous value is restored on exit,
    also when the block raises."""
    prev = set_deterministic(on)
    try:
        yield
    finally:
        set_deterministic(prev)


def _samples_mode(cls):
    """Class decorator for the autograd nodes whose backward depends on the mode: the node samples it ONCE, in its
    forward, and its backward runs under that value whatever the process-wide switch says by then (and puts the switch
    back), so flipping the mode between forward and backward is safe."""
    fwd, bwd = cls.forward, cls.backward

    def forward(ctx, *args):
        ctx.det_mode = is_deterministic()
        return fwd(ctx, *args)

    def backward(ctx, *grads):
        if ctx.det_mode == is_deterministic():
            return bwd(ctx, *grads)
        with deterministic(ctx.det_mode):
            return bwd(ctx, *grads)

    forward.__doc__, backward.__doc__ = fwd.__doc__, bwd.__doc__
    cls.forward, cls.backward = staticmethod(forward), staticmethod(backward)
    return cls


# ------------------------------------------------------------------------------------------------
class CorrelationFunction(torch.autograd.Function):
    """Cost volume; mirrors CorrelationFunction of models/correlation_package/correlation.py:6-44
    (there an instance-style Function unusable on modern torch) with the arithmetic of
    models/correlation_native.py:13-23."""

    @staticmethod
    def forward(ctx, x1, x2, max_displacement, negative_slope=1.0):
        _need_gpu(x1, x2)
        if x1.shape != x2.shape or x1.dim() != 4:
            raise ValueError('correlation expects two [B,C,H,W] tensors of equal shape')
        B, C, H, W = x1.shape
        d = int(max_displacement)
        slope = float(negative_slope)
        # The fast kernels need 16-byte aligned rows (W % 4 == 0).  Coarse pyramid levels such as 6x10 or
        # 8x14 are not: zero-pad the width (identical results on the real columns -- the volume's own
        # padding is zero as well), run the aligned kernel, crop.  The C ABI itself accepts any W.
        wp = (-W) % 4 if (d == 4 and C % 4 == 0) else 0
        if wp:
            x1 = torch.nn.functional.pad(x1, (0, wp))
            x2 = torch.nn.functional.pad(x2, (0, wp))
        x1, x2 = x1.contiguous(), x2.contiguous()
        Wk = W + wp
        out = torch.empty(B, (2 * d + 1) ** 2, H, Wk, device=x1.device, dtype=torch.float32)
        # fused LeakyReLU: the backward selects the derivative from 12 bytes of sign words per pixel (fast
        # path) instead of keeping and re-reading the 324-byte volume; shapes without the fast path keep `out`
        planes = _lib.load().arflow_corr_sign_planes(C, Wk, d) if slope != 1.0 else 0
        sign = torch.empty(B, planes, H, Wk, device=x1.device, dtype=torch.int32) if planes else None
        with torch.cuda.device_of(x1):
            _call('arflow_corr_fwd', _p(x1), _p(x2), _p(out), _p(sign), B, C, H, Wk, d, slope, _stream(),
                  key=(B, C, H, Wk, d, planes))
        if slope != 1.0:
            ctx.save_for_backward(x1, x2, sign if planes else out)
        else:
            ctx.save_for_backward(x1, x2)
        ctx.d, ctx.slope, ctx.w, ctx.wp, ctx.planes = d, slope, W, wp, planes
        return out[..., :W].contiguous() if wp else out

    @staticmethod
    def backward(ctx, gout):
        x1, x2 = ctx.saved_tensors[:2]
        act = ctx.saved_tensors[2] if ctx.slope != 1.0 else None
        fout, sign = (None, act) if ctx.planes else (act, None)
        B, C, H, Wk = x1.shape
        if ctx.wp:
            gout = torch.nn.functional.pad(gout, (0, ctx.wp))
        gout = gout.contiguous()
        g1 = torch.empty_like(x1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(x2) if ctx.needs_input_grad[1] else None
        with torch.cuda.device_of(x1):
            _call('arflow_corr_bwd', _p(gout), _p(fout), _p(sign), _p(x1), _p(x2), _p(g1), _p(g2), B, C, H, Wk, ctx.d,
                  ctx.slope, _stream(), key=(B, C, H, Wk, ctx.d, 0 if act is None else (ctx.planes or (2 * ctx.d + 1) ** 2)))
        if ctx.wp:
            g1 = None if g1 is None else g1[..., :ctx.w].contiguous()
            g2 = None if g2 is None else g2[..., :ctx.w].contiguous()
        return g1, g2, None, None


def _storage(storage):
    if storage in (None, 'fp32', torch.float32):
        return None
    if storage in ('bf16', torch.bfloat16):
        return 'bf16'
    raise ValueError('storage must be None / "fp32" or "bf16" / torch.bfloat16, got %r' % (storage,))


class CorrelationBF16Function(torch.autograd.Function):
    """Cost volume with the features STORED as bf16 (opt-in; the reference's native path
    dispatches half as well, correlation_cuda_kernel.cu:352,369): the fp32 inputs are rounded to bf16 once, the kernels
    read (and autograd keeps) 2 bytes per feature, products are accumulated in fp32, volume and gradients are fp32."""

    @staticmethod
    def forward(ctx, x1, x2, max_displacement, negative_slope):
        for t in (x1, x2):
            if not t.is_cuda:
                raise _lib.ArflowHipError('arflow_amd ops run on the GPU only')
        if x1.shape != x2.shape or x1.dim() != 4:
            raise ValueError('correlation expects two [B,C,H,W] tensors of equal shape')
        B, C, H, W = x1.shape
        d, slope = int(max_displacement), float(negative_slope)
        b1, b2 = x1.to(torch.bfloat16).contiguous(), x2.to(torch.bfloat16).contiguous()
        out = torch.empty(B, (2 * d + 1) ** 2, H, W, device=x1.device, dtype=torch.float32)
        with torch.cuda.device_of(x1):
            _call('arflow_corr_fwd_bf16', _p(b1), _p(b2), _p(out), B, C, H, W, d, slope, _stream(), key=(B, C, H, W, d, 0))
        ctx.save_for_backward(b1, b2, out if slope != 1.0 else None)
        ctx.d, ctx.slope = d, slope
        return out

    @staticmethod
    def backward(ctx, gout):
        b1, b2, fout = ctx.saved_tensors
        B, C, H, W = b1.shape
        gout = gout.contiguous()
        g1 = torch.empty(B, C, H, W, device=b1.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        g2 = torch.empty(B, C, H, W, device=b1.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        with torch.cuda.device_of(b1):
            _call('arflow_corr_bwd_bf16', _p(gout), _p(fout), _p(b1), _p(b2), _p(g1), _p(g2), B, C, H, W, ctx.d, ctx.slope,
                  _stream(), key=(B, C, H, W, ctx.d, 0 if fout is None else (2 * ctx.d + 1) ** 2))
        return g1, g2, None, None


@_samples_mode
class CorrelationGeneralFunction(torch.autograd.Function):
    """Correlation with the CUDA extension's full parameter set (correlation_cuda.cc:10-16: pad_size, kernel_size,
    max_displacement, stride1, stride2); the configuration every model uses goes through CorrelationFunction."""

    @staticmethod
    def forward(ctx, x1, x2, pad_size, kernel_size, max_displacement, stride1, stride2):
        _need_gpu(x1, x2)
        if x1.shape != x2.shape or x1.dim() != 4:
            raise ValueError('correlation expects two [B,C,H,W] tensors of equal shape')
        x1, x2 = x1.contiguous(), x2.contiguous()
        B, C, H, W = x1.shape
        cfg = (int(pad_size), int(kernel_size), int(max_displacement), int(stride1), int(stride2))
        import ctypes
        oc, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.load().arflow_corr_general_out_size(H, W, *cfg, ctypes.addressof(oc), ctypes.addressof(oh),
                                                            ctypes.addressof(ow)), 'arflow_corr_general_out_size')
        out = torch.empty(B, oc.value, oh.value, ow.value, device=x1.device, dtype=torch.float32)
        with torch.cuda.device_of(x1):
            _call('arflow_corr_general_fwd', _p(x1), _p(x2), _p(out), B, C, H, W, *cfg, _stream())
        ctx.save_for_backward(x1, x2)
        ctx.cfg = cfg
        return out

    @staticmethod
    def backward(ctx, gout):
        x1, x2 = ctx.saved_tensors
        B, C, H, W = x1.shape
        gout = gout.contiguous()
        g1 = torch.empty_like(x1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(x2) if ctx.needs_input_grad[1] else None
        with torch.cuda.device_of(x1):
            _call('arflow_corr_general_bwd', _p(gout), _p(x1), _p(x2), _p(g1), _p(g2), B, C, H, W, *ctx.cfg, _stream())
        return g1, g2, None, None, None, None, None


def correlation_general(x1, x2, pad_size, kernel_size, max_displacement, stride1, stride2):
    return CorrelationGeneralFunction.apply(x1, x2, pad_size, kernel_size, max_displacement, stride1, stride2)


def correlation(x1, x2, max_displacement=4, negative_slope=1.0, storage=None):
    """Cost volume, optionally with the LeakyReLU every caller applies right after it fused into the
    kernel's store stage (and its derivative into the backward's load stage).  storage='bf16' (opt-in) keeps the
    features as bf16 in HBM: fp32 accumulation, fp32 volume and gradients."""
    if _storage(storage) == 'bf16':
        return CorrelationBF16Function.apply(x1, x2, max_displacement, negative_slope)
    return CorrelationFunction.apply(x1, x2, max_displacement, negative_slope)


class CorrConcatFunction(torch.autograd.Function):
    """cat([*before, leaky_relu(corr(x1, x2)), *after], dim=1) with the cost volume written by the kernel STRAIGHT
    into its channel slot of the concatenated buffer (arflow_corr_fwd_strided), and its gradient read in place from
    the gradient of that buffer (arflow_corr_bwd_strided): the decoders of the reference concatenate the volume with
    features and flow right after computing it (models/pwclite_uflow.py:218-222, models/pwclite.py:187-189,
    models/uflow_model.py:192-198) -- 81 of the 115-147 channels of that copy, forward, and a contiguous() of the
    81-channel gradient slice, backward, disappear.  The other members are copied into their slots."""

    @staticmethod
    def forward(ctx, x1, x2, max_displacement, negative_slope, n_before, *others):
        _need_gpu(x1, x2, *others)
        B, C, H, W = x1.shape
        d, slope = int(max_displacement), float(negative_slope)
        x1, x2 = x1.contiguous(), x2.contiguous()
        nvol = (2 * d + 1) ** 2
        chans = [int(t.shape[1]) for t in others]
        c0 = sum(chans[:n_before])
        ctot = nvol + sum(chans)
        buf = torch.empty(B, ctot, H, W, device=x1.device, dtype=torch.float32)
        planes = _lib.load().arflow_corr_sign_planes(C, W, d) if slope != 1.0 else 0
        sign = torch.empty(B, planes, H, W, device=x1.device, dtype=torch.int32) if planes else None
        vol = buf[:, c0:c0 + nvol]
        with torch.cuda.device_of(x1):
            _call('arflow_corr_fwd_strided', _p(x1), _p(x2), vol.data_ptr(), ctot * H * W, _p(sign), B, C, H, W, d, slope,
                  _stream(), key=(B, C, H, W, d, planes))
        off = 0
        for k, t in enumerate(others):
            if k == n_before:
                off += nvol
            buf[:, off:off + chans[k]].copy_(t)
            off += chans[k]
        # fast path with sign words keeps 12 B/px for the LeakyReLU derivative; otherwise the buffer itself (its
        # volume slot) is the saved forward output
        ctx.save_for_backward(x1, x2, sign if planes else (buf if slope != 1.0 else None))
        ctx.cfg = (d, slope, planes, n_before, chans, c0, nvol, ctot)
        return buf

    @staticmethod
    def backward(ctx, gbuf):
        x1, x2, act = ctx.saved_tensors
        d, slope, planes, n_before, chans, c0, nvol, ctot = ctx.cfg
        B, C, H, W = x1.shape
        gbuf = gbuf.contiguous()
        sign, fout = (act, None) if planes else (None, act)
        g1 = torch.empty_like(x1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(x2) if ctx.needs_input_grad[1] else None
        gvol = gbuf[:, c0:c0 + nvol]
        with torch.cuda.device_of(x1):
            _call('arflow_corr_bwd_strided', gvol.data_ptr(), ctot * H * W,
                  None if fout is None else fout[:, c0:c0 + nvol].data_ptr(), ctot * H * W, _p(sign), _p(x1), _p(x2),
                  _p(g1), _p(g2), B, C, H, W, d, slope, _stream(),
                  key=(B, C, H, W, d, 0 if act is None else (planes or nvol)))
        gothers, off = [], 0
        for k, c in enumerate(chans):
            if k == n_before:
                off += nvol
            gothers.append(gbuf[:, off:off + c] if ctx.needs_input_grad[5 + k] else None)
            off += c
        return (g1, g2, None, None, None) + tuple(gothers)


_CORR_CONCAT = __import__('os').environ.get('ARFLOW_CORR_CONCAT', '1') != '0'  # A/B switch for tools/ and bench.py


def corr_concat_supported(C, W, max_displacement=4):
    return bool(_lib.load().arflow_corr_strided_supported(int(C), int(W), int(max_displacement)))


def correlation_concat(x1, x2, before=(), after=(), max_displacement=4, negative_slope=1.0):
    """torch.cat([*before, leaky_relu(correlation(x1, x2)), *after], 1) without ever copying the cost volume (shapes
    the strided kernels do not take fall back to the plain op + torch.cat)."""
    B, C, H, W = x1.shape
    if x1.is_cuda and _CORR_CONCAT and corr_concat_supported(C, W, max_displacement):
        return CorrConcatFunction.apply(x1, x2, max_displacement, negative_slope, len(before), *before, *after)
    return torch.cat(list(before) + [correlation(x1, x2, max_displacement, negative_slope)] + list(after), 1)


# ------------------------------------------------------------------------------------------------
FEATNORM = {'joint': 0, 'avg': 1}
def _featnorm_acc(B, device):  # ARFLOW_FEATNORM_ACC_DOUBLES(B)
    return torch.empty(4 * (2048 + B), device=device, dtype=torch.float64)


class FeatureNormFunction(torch.autograd.Function):
    """(x1, x2) -> ((x1 - mu) / std, (x2 - mu) / std) with per-sample moments over both tensors:
    normalize_features of models/pwclite_uflow.py:30-38 ('joint') and of models/uflow_model.py:8-50 as
    PWCFlow calls it ('avg').  Two launches forward, two backward."""

    @staticmethod
    def forward(ctx, x1, x2, mode):
        _need_gpu(x1, x2)
        if x1.shape != x2.shape or x1.dim() < 2:
            raise ValueError('feature normalisation expects two tensors of equal shape [B, ...]')
        x1, x2 = x1.contiguous(), x2.contiguous()
        B = x1.shape[0]
        n = x1[0].numel()
        y1, y2 = torch.empty_like(x1), torch.empty_like(x2)
        acc = _featnorm_acc(B, x1.device)
        stats = torch.empty(B, 4, device=x1.device, dtype=torch.float32)
        with torch.cuda.device_of(x1):
            _call('arflow_featnorm_fwd', _p(x1), _p(x2), _p(y1), _p(y2), _p(acc), _p(stats), B, n, mode, _stream(),
                  key=(B, n))
        ctx.save_for_backward(x1, x2, stats)
        ctx.mode = mode
        return y1, y2

    @staticmethod
    def backward(ctx, g1, g2):
        x1, x2, stats = ctx.saved_tensors
        B = x1.shape[0]
        n = x1[0].numel()
        g1, g2 = g1.contiguous(), g2.contiguous()
        d1 = torch.empty_like(x1) if ctx.needs_input_grad[0] else None
        d2 = torch.empty_like(x2) if ctx.needs_input_grad[1] else None
        acc = _featnorm_acc(B, x1.device)
        with torch.cuda.device_of(x1):
            _call('arflow_featnorm_bwd', _p(g1), _p(g2), _p(x1), _p(x2), _p(stats), _p(acc), _p(d1), _p(d2), B, n,
                  ctx.mode, _stream(), key=(B, n))
        return d1, d2, None


def normalize_pair(x1, x2, mode='joint'):
    return FeatureNormFunction.apply(x1, x2, FEATNORM[mode])


# ------------------------------------------------------------------------------------------------
class LevelCfg:
    """Static description of one fused pyramid level (not a tensor: travels through autograd as a plain argument).

    layout: the channel order of the decoder's concatenated input as a list of 'vol' (cost volume + LeakyReLU), 'x1n'
    (normalised first map), 'flow' (the x2-upsampled flow, only with a coarse flow) and integers (index into the extra
    member tensors)."""

    def __init__(self, layout, norm_mode, slope=0.1, max_displacement=4, flow_is_coarse=True, up_align_corners=True,
                 pad='zeros', align_corners=True, coord_norm=NORM_ARFLOW):
        self.layout = list(layout)
        self.mode = FEATNORM[norm_mode]
        self.slope, self.d = float(slope), int(max_displacement)
        self.flow_is_coarse, self.up_align = bool(flow_is_coarse), bool(up_align_corners)
        self.pad, self.align, self.norm = PAD[pad], int(bool(align_corners)), int(coord_norm)


def level_supported(x1, flow, flow_is_coarse, max_displacement=4):
    """The fused level launches take the shapes of the tuned correlation kernels (W % 4 == 0, C % 4 == 0, d = 4)."""
    B, C, H, W = x1.shape
    if not (x1.is_cuda and x1.dtype == torch.float32 and _LEVEL_FUSED):
        return False
    if not _lib.load().arflow_corr_strided_supported(int(C), int(W), int(max_displacement)):
        return False
    if flow is not None and flow_is_coarse and (H % 2 or W % 2 or tuple(flow.shape[2:]) != (H // 2, W // 2)):
        return False
    return True


_LEVEL_FUSED = __import__('os').environ.get('ARFLOW_LEVEL_FUSED', '1') != '0'  # A/B switch for tools/ and tests


@_samples_mode
class LevelFunction(torch.autograd.Function):
    """One pyramid level in front of its flow estimator (models/pwclite_uflow.py:203-222,
    models/uflow_model.py:160-198):

        flow_up = interpolate(flow * 2, x2)                 (flow_is_coarse)
        x2w     = warp(x2, flow_up)                         (no flow: x2w = x2)
        x1n, x2n = normalize_features([x1, x2w])
        buf     = cat([..., leaky_relu(corr(x1n, x2n)), x1n, flow_up, ...], 1)

    forward = arflow_level_warp_fwd (or arflow_level_moments) + arflow_level_corr_fwd: the normalised second map, the
    moment / apply passes of the normalisation and the interpolate / mul / cat launches do not exist.  Returns
    (buf, flow_up) with a coarse flow, else buf."""

    @staticmethod
    def forward(ctx, x1, x2, flow, cfg, x1_rows, x2_rows, *members):
        """x1_rows / x2_rows (optional [B,rows,2] float64): partial moments of x1 / (at a level without flow) x2 from
        bias_leaky_relu_moments -- the launch that produced the maps; the warp launch then skips reading x1 and the
        level without a warp needs no moment pass."""
        _need_gpu(x1, x2, flow, *members)
        if x1.shape != x2.shape or x1.dim() != 4:
            raise ValueError('level expects two [B,C,H,W] feature maps of equal shape')
        x1, x2 = x1.contiguous(), x2.contiguous()
        B, C, H, W = x1.shape
        lib = _lib.load()
        nvol = (2 * cfg.d + 1) ** 2
        has_flow = flow is not None
        chans, offs, off = [], {}, 0
        for item in cfg.layout:
            c = {'vol': nvol, 'x1n': C, 'flow': 2}[item] if isinstance(item, str) else int(members[item].shape[1])
            offs[item] = off
            chans.append(c)
            off += c
        ctot = off
        if 'flow' in offs and not (has_flow and cfg.flow_is_coarse):
            raise ValueError("layout item 'flow' needs a coarse flow")
        buf = torch.empty(B, ctot, H, W, device=x1.device, dtype=torch.float32)
        bs = ctot * H * W
        rows = lib.arflow_level_acc_rows(B, C, H, W, int(has_flow))
        acc = torch.empty(4 * B * rows, device=x1.device, dtype=torch.float64)
        stats = torch.empty(B, 4, device=x1.device, dtype=torch.float32)
        sign = torch.empty(B, 3, H, W, device=x1.device, dtype=torch.int32) if cfg.slope != 1.0 else None
        flow_full = x2w = x1n = None
        fbs, fslot, fup = 0, None, None
        if has_flow:
            flow, fbs = _flow_view(flow)
            x2w = torch.empty_like(x2)
            if cfg.flow_is_coarse:
                flow_full = fup = torch.empty(B, 2, H, W, device=x1.device, dtype=torch.float32)
                fslot = buf[:, offs['flow']:].data_ptr() if 'flow' in offs else None
            else:
                flow_full = flow
        if 'x1n' in offs:
            x1n_ptr, x1n_bs = buf[:, offs['x1n']:].data_ptr(), bs
        else:
            x1n = torch.empty_like(x1)
            x1n_ptr, x1n_bs = x1n.data_ptr(), C * H * W
        for name, rows in (('x1_rows', x1_rows), ('x2_rows', x2_rows)):
            if rows is None:
                continue
            if rows.dtype != torch.float64 or rows.dim() != 3 or rows.shape[0] != B or rows.shape[2] != 2:
                raise ValueError('%s must be [B, rows, 2] float64' % name)
            if rows.device != x1.device:
                raise ValueError('%s must be on the device of the feature maps' % name)
        if x1_rows is not None:
            x1_rows = x1_rows.contiguous()
        if x2_rows is not None:
            x2_rows = x2_rows.contiguous() if (not has_flow and x1_rows is not None) else None
        with torch.cuda.device_of(x1):
            _call('arflow_level_fwd_m', _p(x1), _p(x2), _p(flow), fbs, int(cfg.flow_is_coarse and has_flow), int(cfg.up_align),
                  _p(fup), fslot, bs, _p(x2w), cfg.mode, buf[:, offs['vol']:].data_ptr(), bs, x1n_ptr, x1n_bs, _p(sign),
                  _p(stats), _p(acc), _p(x1_rows), 0 if x1_rows is None else int(x1_rows.shape[1]), _p(x2_rows),
                  0 if x2_rows is None else int(x2_rows.shape[1]), B, C, H, W, cfg.d, cfg.slope, cfg.pad, cfg.align, cfg.norm,
                  _stream(), key=(B, C, H, W, cfg.d, 3 if sign is not None else 0,
                                  int(has_flow) + int(has_flow and cfg.flow_is_coarse), int(x1_rows is not None)))
        for item in cfg.layout:
            if not isinstance(item, str):
                buf[:, offs[item]:offs[item] + int(members[item].shape[1])].copy_(members[item])
        ctx.save_for_backward(x1, x2, x2w, flow_full, stats, sign, buf if x1n is None else x1n)
        ctx.cfg, ctx.offs, ctx.ctot, ctx.n_members, ctx.has_flow = cfg, offs, ctot, len(members), has_flow  # noqa
        ctx.member_chans = [int(m.shape[1]) for m in members]
        if has_flow and cfg.flow_is_coarse:
            return buf, flow_full
        return buf

    @staticmethod
    def backward(ctx, gbuf, gflow_ext=None):
        x1, x2, x2w, flow_full, stats, sign, x1n_holder = ctx.saved_tensors
        cfg, offs, ctot = ctx.cfg, ctx.offs, ctx.ctot
        B, C, H, W = x1.shape
        nvol = (2 * cfg.d + 1) ** 2
        gbuf = gbuf.contiguous()
        bs = ctot * H * W
        if 'x1n' in offs:
            x1n_ptr, x1n_bs = x1n_holder[:, offs['x1n']:].data_ptr(), bs
        else:
            x1n_ptr, x1n_bs = x1n_holder.data_ptr(), C * H * W
        d1, gx2 = torch.empty_like(x1), torch.empty_like(x1)
        ws = torch.empty(_lib.load().arflow_level_bwd_ws_bytes(B, C, H, W), device=x1.device, dtype=torch.uint8)
        gflow_in = fl = gslot = None
        fbs = 0
        coarse = ctx.has_flow and cfg.flow_is_coarse
        if ctx.has_flow:
            fl, fbs = _flow_view(flow_full)
            gflow_in = torch.empty(B, 2, H // 2, W // 2, device=x1.device, dtype=torch.float32) if coarse else \
                torch.empty(B, 2, H, W, device=x1.device, dtype=torch.float32)
            if 'flow' in offs:
                gslot = gbuf[:, offs['flow']:].data_ptr()
            if gflow_ext is not None:
                gflow_ext = gflow_ext.contiguous()
        gdir = gbuf[:, offs['x1n']:].data_ptr() if 'x1n' in offs else None
        with torch.cuda.device_of(x1):
            _call('arflow_level_bwd', gbuf[:, offs['vol']:].data_ptr(), bs, _p(sign), x1n_ptr, x1n_bs, gdir, bs, _p(x1),
                  _p(x2), _p(x2w), _p(fl), fbs, gslot, bs, _p(gflow_ext), _p(stats), cfg.mode, _p(d1), _p(gx2), _p(gflow_in),
                  int(coarse), int(cfg.up_align), _p(ws), B, C, H, W, cfg.d, cfg.slope, cfg.pad, cfg.align, cfg.norm,
                  _stream(), key=(B, C, H, W, cfg.d, 3 if sign is not None else 0, int(ctx.has_flow) + int(coarse)))
        gm, k = [], 0
        for item in cfg.layout:
            if not isinstance(item, str):
                gm.append((item, gbuf[:, offs[item]:offs[item] + ctx.member_chans[item]]))
        gmembers = [None] * ctx.n_members
        for idx, g in gm:
            gmembers[idx] = g if ctx.needs_input_grad[6 + idx] else None
        return (d1, gx2, gflow_in, None, None, None) + tuple(gmembers)


def level(x1, x2, flow, cfg, *members, x1_rows=None, x2_rows=None):
    return LevelFunction.apply(x1, x2, flow, cfg, x1_rows, x2_rows, *members)


# ------------------------------------------------------------------------------------------------
@_samples_mode
class BiasLeakyReLUFunction(torch.autograd.Function):
    """y = leaky_relu(x + bias[None, :, None, None], slope), IN PLACE on x (the bias-free output of a
    convolution, which autograd does not need again); backward = LeakyReLU derivative and bias gradient in
    one pass.  Replaces the bias add + nn.LeakyReLU(0.1, inplace=True) behind every conv of the reference
    models (models/pwclite.py:10-23)."""

    @staticmethod
    def forward(ctx, x, bias, slope):
        _need_gpu(x)
        if not x.is_contiguous():
            raise ValueError('bias_leaky_relu expects a contiguous [B,C,...] tensor')
        B, C = x.shape[0], x.shape[1]
        hw = x[0, 0].numel()
        if bias is not None:
            _need_gpu(bias)
            bias = bias.contiguous()
        with torch.cuda.device_of(x):
            _call('arflow_bias_act_fwd', _p(x), _p(bias), _p(x), B, C, hw, float(slope), _stream(), key=(B, C, hw))
        ctx.mark_dirty(x)
        ctx.save_for_backward(x)
        ctx.slope, ctx.has_bias = float(slope), bias is not None
        return x

    @staticmethod
    def backward(ctx, gout):
        y, = ctx.saved_tensors
        B, C = y.shape[0], y.shape[1]
        hw = y[0, 0].numel()
        gout = gout.contiguous()
        gin = torch.empty_like(gout)
        gb = torch.empty(C, device=y.device, dtype=torch.float32) if (ctx.has_bias and ctx.needs_input_grad[1]) else None
        with torch.cuda.device_of(y):
            _call('arflow_bias_act_bwd', _p(gout), _p(y), _p(gin), _p(gb), B, C, hw, ctx.slope, _stream(), key=(B, C, hw))
        return gin, gb, None


def bias_leaky_relu(x, bias, slope=0.1):
    return BiasLeakyReLUFunction.apply(x, bias, slope)


_HEADCONV = __import__('os').environ.get('ARFLOW_HEADCONV', '1') != '0'  # A/B switch for tools/ and tests: 0 = MIOpen


class HeadConvFunction(torch.autograd.Function):
    """y = conv2d(x, w, bias) for w: [2, C, 3, 3], stride 1, padding 1 -- the flow heads built by conv(..., isReLU=False)
    (models/pwclite.py:10-23, :48-106) -- through the direct kernels of csrc/headconv.hip: one pass over x forward, one
    store stream for dx, one pass over x for dw and dbias; every result is bitwise reproducible."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_gpu(x, weight, bias)
        if x.dim() != 4 or tuple(weight.shape) != (2, x.shape[1], 3, 3):
            raise ValueError('head_conv expects x [B,C,H,W] and weight [2,C,3,3]')
        x, weight = x.contiguous(), weight.contiguous()
        if bias is not None:
            bias = bias.contiguous()
        y = _headconv_fwd(x, weight, bias)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = _headconv_dgrad(dy, weight, x) if ctx.needs_input_grad[0] else None
        dw, db = _headconv_wgrad(x, dy, weight, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        return dx, dw, db


# The three launches of csrc/headconv.hip without autograd, for HeadConvFunction and the head of DenseEstimatorFunction
def _headconv_fwd(x, w, b):
    """y [B,2,H,W] = conv2d(x, w, b, padding=1); every tensor contiguous (here and below), b may be None."""
    B, C, H, W = x.shape
    y = torch.empty(B, 2, H, W, device=x.device, dtype=torch.float32)
    with torch.cuda.device_of(x):
        _call('arflow_headconv_fwd', _p(x), _p(w), _p(b), _p(y), B, C, H, W, _stream())
    return y


def _headconv_dgrad(gy, w, like):
    """dx of that convolution, shaped like its input `like`."""
    B, C, H, W = like.shape
    dx = torch.empty_like(like)
    with torch.cuda.device_of(like):
        _call('arflow_headconv_bwd_data', _p(gy), _p(w), _p(dx), B, C, H, W, _stream())
    return dx


def _headconv_wgrad(x, gy, w, want_w, want_b):
    """(dw, db) in one pass over x, or (None, None); the kernel always forms dw, so where only the bias is wanted it is dropped."""
    if not (want_w or want_b):
        return None, None
    B, C, H, W = x.shape
    ws = _workspace('arflow_headconv_bwd_weight_ws_bytes', B, C, H, W, device=x.device)
    dw = torch.empty_like(w)
    db = torch.empty(2, device=x.device, dtype=torch.float32) if want_b else None
    with torch.cuda.device_of(x):
        _call('arflow_headconv_bwd_weight', _p(x), _p(gy), _p(dw), _p(db), _p(ws), B, C, H, W, _stream())
    return (dw if want_w else None), db


def head_conv(x, weight, bias):
    return HeadConvFunction.apply(x, weight, bias)


def head_conv_enabled():
    return _HEADCONV


# ------------------------------------------------------------------------------------------------
# Wide 3x3 convolutions on the bf16 matrix cores at fp32 accuracy (csrc/splitconv.hip)
_SPLITCONV = __import__('os').environ.get('ARFLOW_SPLITCONV', '1') != '0'  # A/B switch for tools/ and tests: 0 = MIOpen


def splitconv_enabled():
    return _SPLITCONV


def splitconv_takes(N, C, K, H, W):
    """Whether ONE convolution call -- x: [N,C,H,W] -> y: [N,K,H,W], 3x3, stride 1, padding 1 -- goes to the split-bf16 kernel.
    A layer's forward asks with its own (C, K), its data gradient with the two swapped: that is the call the kernel sees.
    The rule is read off profiles/splitconv_kbench.log: the kernel is taken only where it beat
    MIOpen's best solver by more than the spread of both."""
    if not _SPLITCONV:
        return False
    return _splitconv_rule(int(N), int(C), int(K), int(H), int(W))


def _size_floor(N, H, W, h, w):
    """The routing rules' floor: maps of at least h x w and 16 of them in the batch (they were measured at N = 16)."""
    return H * W >= h * w and N * H * W >= 16 * h * w


def _splitconv_rule(N, C, K, H, W):
    # measured at N = 16, channels 32 .. 597: faster on every call at 96x160 (1.13x .. 1.45x); at 48x80 on the calls with 128
    # output channels or at most 128 input channels (1.16x .. 1.50x; 403->96, 499->64, 563->32 forward and 64<->32 are not);
    # at 24x40 and 12x20 on none (the tiles do not fill the chip)
    if min(C, K) < 32 or not 64 <= max(C, K) <= 640:
        return False
    if _size_floor(N, H, W, 96, 160):
        return True
    if _size_floor(N, H, W, 48, 80):
        return max(C, K) >= 128 and (K >= 128 or C <= 128)
    return False


def splitconv(x, w, transpose_flip=False, out=None, bias=None, slope=None):
    """conv2d(x, w, padding=1) through arflow_splitconv_pack + arflow_splitconv_fwd_ex (no autograd); transpose_flip: the data
    gradient of that convolution for x = dy, i.e. conv2d(x, w.transpose(0, 1).flip(2, 3), padding=1).
    x may be a channel slice of a larger tensor (dense planes, free batch stride: read in place).  out: an [N,K,H,W] view with
    dense planes, e.g. a channel slot of a larger tensor, written in place and returned; it may share x's buffer but must not
    overlap x.  slope selects the epilogue: the result is leaky_relu(conv + bias, slope), bias [K] or None (bias needs slope)."""
    _need_gpu(x, w, out, bias)
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or x.shape[1] != w.shape[0 if transpose_flip else 1]:
        raise ValueError('splitconv expects x [N,C,H,W] and w [K,C,3,3] (transpose_flip: x [N,K,H,W])')
    x, x_bs = _batch_strided(x)
    w = w.contiguous()
    N, C, H, W = x.shape
    K = int(w.shape[1 if transpose_flip else 0])
    if bias is not None and (slope is None or bias.numel() != K):
        raise ValueError('splitconv: bias holds one value per output channel and needs slope (the epilogue is bias + LeakyReLU)')
    packed = _workspace('arflow_splitconv_pack_bytes', K, C, device=x.device)
    if out is None:
        y, y_bs = torch.empty(N, K, H, W, device=x.device, dtype=torch.float32), K * H * W
    else:
        y, y_bs = out, (int(out.stride(0)) if N > 1 else K * H * W)
        if tuple(y.shape) != (N, K, H, W) or _batch_strided(y)[0] is not y:
            raise ValueError('splitconv: out must be an [N,K,H,W] view with dense planes (a channel slot of a larger tensor)')
        if not _disjoint(x, x_bs, y, y_bs):
            raise ValueError('splitconv: out overlaps x')
    bias = None if bias is None else bias.contiguous()
    with torch.cuda.device_of(x):
        _call('arflow_splitconv_pack', _p(w), _p(packed), int(w.shape[0]), int(w.shape[1]), int(bool(transpose_flip)), _stream())
        _call('arflow_splitconv_fwd_ex', _p(x), x_bs, _p(packed), _p(y), y_bs, _p(bias), int(slope is not None),
              float(slope or 0.0), N, C, K, H, W, _stream())
    return y


def _disjoint(x, x_bs, y, y_bs):
    """Whether the batch-strided [N,C,H,W] views x and y share no element (byte ranges; conservative where the strides differ)."""
    N, hw = x.shape[0], x.shape[2] * x.shape[3]
    cx, cy = x.shape[1] * hw, y.shape[1] * hw
    d = (y.data_ptr() - x.data_ptr()) // 4  # y's first element, in floats from x's
    if d >= (N - 1) * x_bs + cx or d + (N - 1) * y_bs + cy <= 0:
        return True
    if x_bs != y_bs:
        return False
    r = d % x_bs  # same lattice of samples: y's channels must fall in the gap x leaves in every period
    return r >= cx and r + cy <= x_bs


_SPLITCONV_WGRAD = __import__('os').environ.get('ARFLOW_SPLITCONV_WGRAD', '1') != '0'  # A/B switch: 0 = MIOpen's weight gradients


def splitconv_wgrad_takes(N, C, K, H, W):
    """Whether the WEIGHT GRADIENT of the layer x: [N,C,H,W] -> y: [N,K,H,W] (3x3, stride 1, padding 1) goes to
    csrc/splitconv_wgrad.hip.  Asked by ConvAct and by DenseEstimatorFunction.backward with the same arguments, so the fused
    and the composed path run the same kernel for the same layer.  Off with ARFLOW_SPLITCONV_WGRAD=0 and with ARFLOW_SPLITCONV=0.
    The rule is read off profiles/splitconv_wgrad_kbench.log."""
    if not (_SPLITCONV and _SPLITCONV_WGRAD):
        return False
    return _splitconv_wgrad_rule(int(N), int(C), int(K), int(H), int(W))


def _splitconv_wgrad_rule(N, C, K, H, W):
    # never below N H W = 16 x 48 x 80 (the shapes of the existing tests keep MIOpen's dw); measured at N = 16 over the seven
    # (C, K) of section 17 and four map sizes with the 2 x 2 tiles of section 35 (profiles/wgrad_tile_kbench.log): the kernel's
    # max is below the min of MIOpen's solver plus its layout copies at 96x160 on the six wide layers -- 147->128 1.23x,
    # 275->128 1.36x, 403->96 1.55x, 499->64 1.55x, 563->32 1.46x, 597->128 1.39x (64->32 0.67x is not) -- and at 48x80 on
    # 275->128 1.10x, 403->96 1.23x, 499->64 1.51x, 597->128 1.27x (147->128 0.90x is not; 563->32 1.06x, a single tile of
    # output channels, is left where it was); on two calls at 24x40 (1.1x), which the floor keeps out
    # (every size condition goes through _size_floor, like the other rules': a test that patches the floor moves all of them)
    if _size_floor(N, H, W, 96, 160):
        return 128 <= C <= 640 and 32 <= K <= 128
    # (fewer maps of 96x160 or more were not measured: they keep MIOpen -- 16 maps of that size would pass the floor)
    return not _size_floor(16, H, W, 96, 160) and _size_floor(N, H, W, 48, 80) and 256 <= C <= 640 and 64 <= K <= 128


def _batch_strided(t):
    """t if its planes, rows and channels are dense (only the batch stride is free: a channel slice of a larger tensor),
    else a contiguous copy; and the batch stride in elements."""
    _, C, H, W = t.shape
    if t.stride(3) != 1 or t.stride(2) != W or t.stride(1) != H * W or (t.shape[0] > 1 and t.stride(0) < C * H * W):
        t = t.contiguous()
    return t, (int(t.stride(0)) if t.shape[0] > 1 else C * H * W)


def splitconv_wgrad(x, gy):
    """dw [K,C,3,3] of conv2d(x, w, padding=1) for the output gradient gy, through arflow_splitconv_wgrad (no autograd).
    x: [N,C,H,W], gy: [N,K,H,W]; either may be a channel slice of a larger tensor (read in place)."""
    _need_gpu(x, gy)
    if x.dim() != 4 or gy.dim() != 4 or x.shape[0] != gy.shape[0] or x.shape[2:] != gy.shape[2:]:
        raise ValueError('splitconv_wgrad expects x [N,C,H,W] and gy [N,K,H,W]')
    x, x_bs = _batch_strided(x)
    gy, gy_bs = _batch_strided(gy)
    N, C, H, W = x.shape
    K = int(gy.shape[1])
    ws = _workspace('arflow_splitconv_wgrad_ws_bytes', N, C, K, H, W, device=x.device)
    dw = torch.empty(K, C, 3, 3, device=x.device, dtype=torch.float32)
    with torch.cuda.device_of(x):
        _call('arflow_splitconv_wgrad', _p(x), x_bs, _p(gy), gy_bs, _p(dw), _p(ws), N, C, K, H, W, _stream())
    return dw


def _conv_args():
    return [1, 1], [1, 1], [1, 1], False, [0, 0], 1  # stride, padding, dilation, transposed, output_padding, groups


class Conv3x3Function(torch.autograd.Function):
    """y = conv2d(x, w, None, 1, 1) for a 3x3 kernel as one autograd node.  `fwd` / `dgrad` / `wgrad` say which of the
    forward, the data gradient and the weight gradient run the split-bf16 kernels; the others are the calls F.conv2d and its
    autograd make (aten.convolution / aten.convolution_backward: the same MIOpen problem keys as before)."""

    @staticmethod
    def forward(ctx, x, w, fwd, dgrad, wgrad=False):
        if fwd:
            y = splitconv(x, w)
        else:
            y = torch.ops.aten.convolution(x, w, None, *_conv_args())
        ctx.save_for_backward(x, w)
        ctx.dgrad, ctx.wgrad = bool(dgrad), bool(wgrad)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        dx, dw = _conv3x3_grads(x, w, gy.contiguous(), ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.dgrad, ctx.wgrad)
        return dx, dw, None, None, None


def _conv3x3_grads(x, w, gy, want_dx, want_dw, dx_native, dw_native):
    """(dx, dw) of conv2d(x, w, padding=1) for Conv3x3Function and the layers of DenseEstimatorFunction (no autograd): each on
    the split-bf16 kernel where dx_native / dw_native say so, what is left in ONE MIOpen call; an unwanted one is None."""
    dx = splitconv(gy, w, transpose_flip=True) if want_dx and dx_native else None
    dw = splitconv_wgrad(x, gy) if want_dw and dw_native else None
    left = [bool(want_dx and dx is None), bool(want_dw and dw is None), False]
    if any(left):
        dx_m, dw_m, _ = torch.ops.aten.convolution_backward(gy, x, w, None, *_conv_args(), left)
        dx, dw = (dx_m if left[0] else dx), (dw_m if left[1] else dw)
    return dx, dw


def conv3x3(x, w, fwd=True, dgrad=True, wgrad=False):
    """conv2d(x, w, padding=1), 3x3: forward, data gradient and (wgrad) weight gradient on the split-bf16 kernels; each can
    be left to MIOpen."""
    return Conv3x3Function.apply(x, w, bool(fwd), bool(dgrad), bool(wgrad))


# ------------------------------------------------------------------------------------------------
# The dense flow estimator as one autograd node (csrc/dense.hip)
_DENSE_BLOCK = __import__('os').environ.get('ARFLOW_DENSE_BLOCK', '1') != '0'  # A/B switch for tools/ and tests: 0 = composed path
DENSE_MAX_SRC = 8  # ARFLOW_DENSE_MAX_SRC of include/arflow_hip.h


def dense_block_enabled():
    return _DENSE_BLOCK


def _dense_src_type():
    import ctypes

    class DenseSrc(ctypes.Structure):  # arflow_dense_src
        _fields_ = [('ptr', ctypes.c_void_p), ('bstride', ctypes.c_long), ('scale', ctypes.c_void_p)]
    return DenseSrc


_DenseSrc = _dense_src_type()


def dense_cat(y, bias, x, slope):
    """torch.cat([bias_leaky_relu(y, bias, slope), x], 1) in one launch, into a fresh tensor (no autograd: the kernel
    behind DenseEstimatorFunction's forward)."""
    _need_gpu(y, bias, x)
    if y.dim() != 4 or x.dim() != 4 or y.shape[0] != x.shape[0] or y.shape[2:] != x.shape[2:]:
        raise ValueError('dense_cat expects y [B,oc,H,W] and x [B,C,H,W]')
    y, x = y.contiguous(), x.contiguous()
    bias = None if bias is None else bias.contiguous()
    B, oc, H, W = y.shape
    C = x.shape[1]
    out = torch.empty(B, oc + C, H, W, device=y.device, dtype=torch.float32)
    with torch.cuda.device_of(y):
        _call('arflow_dense_cat_fwd', _p(y), _p(bias), _p(x), _p(out), B, oc, C, H * W, float(slope), _stream(),
              key=(B, oc, C, H * W))
    return out


def dense_grad_gather(sources, oc, act=None, slope=0.1, want_bias=False):
    """gy = lrelu'(act[:, :oc]) * (s_0 + s_1 + ...) in one launch, the sum nested innermost first (acc = s_0; acc = s_1 + acc;
    ...).  sources: list of (tensor [B,*,H,W] with dense planes, first channel of the slice, per-sample scale [B] or None);
    act: the tensor whose first oc channels hold the saved activation (None: no activation factor).  Returns (gy packed
    [B,oc,H,W], bias gradient [oc] or None -- per-workgroup rows folded in a fixed order)."""
    import ctypes
    if not 1 <= len(sources) <= DENSE_MAX_SRC:
        raise ValueError('dense_grad_gather takes 1..%d sources' % DENSE_MAX_SRC)
    t0 = sources[0][0]
    B, _, H, W = t0.shape
    hw = H * W
    arr = (_DenseSrc * len(sources))()
    keep = []
    for j, (t, off, scale) in enumerate(sources):
        _need_gpu(t, scale)
        st = t.stride()
        if t.dim() != 4 or t.shape[0] != B or tuple(t.shape[2:]) != (H, W) or off < 0 or off + oc > t.shape[1]:
            raise ValueError('dense_grad_gather: source %d does not hold channels %d:%d of a [%d,*,%d,%d] tensor' % (j, off, off + oc, B, H, W))
        if st[3] != 1 or st[2] != W or st[1] != hw:
            t = t.contiguous()
            st = t.stride()
        if scale is not None:
            scale = scale.reshape(-1).contiguous()
            if scale.numel() != B:
                raise ValueError('dense_grad_gather: a scale holds one value per sample')
        keep.append((t, scale))
        arr[j].ptr = t.data_ptr() + 4 * off * hw
        arr[j].bstride = st[0] if B > 1 else t.shape[1] * hw
        arr[j].scale = _p(scale)
    act_bs = 0
    if act is not None:
        _need_gpu(act)
        ok = act.dim() == 4 and act.shape[0] == B and tuple(act.shape[2:]) == (H, W) and act.shape[1] >= oc
        if ok and act.is_contiguous():
            act_bs = act.shape[1] * hw
        elif ok and _batch_strided(act)[0] is act:  # a channel slice of a larger tensor (the in-place estimator's x6), read in place
            act_bs = int(act.stride(0)) if B > 1 else act.shape[1] * hw
        else:
            raise ValueError('dense_grad_gather: act must be a contiguous [B,>=oc,H,W] tensor')
    gy = torch.empty(B, oc, H, W, device=t0.device, dtype=torch.float32)
    rows = None
    if want_bias:
        n = _lib.load().arflow_dense_gbias_rows(B, hw)
        if n <= 0:
            _lib.check(n, 'arflow_dense_gbias_rows')
        rows = torch.empty(n, oc, device=t0.device, dtype=torch.float32)
    with torch.cuda.device_of(t0):
        _call('arflow_dense_grad_gather', ctypes.cast(arr, ctypes.c_void_p), len(sources), _p(act), act_bs, _p(gy), _p(rows), B,
              oc, hw, float(slope), _stream(), key=(B, oc, hw, len(sources), int(act is not None)))
    return gy, (None if rows is None else rows.sum(0))


_DENSE_INPLACE = __import__('os').environ.get('ARFLOW_DENSE_INPLACE', '1') != '0'  # A/B switch: 0 = dense_cat into fresh tensors


def dense_inplace_enabled():
    return _DENSE_INPLACE


def _inplace_wgrad_takes(N, C, K, H, W):
    """splitconv_wgrad_takes on the in-place path of DenseEstimatorFunction, where x_k is a channel slice of x_6: our kernel
    reads the slice in place, MIOpen's weight gradient would have ATen copy it contiguous first.  Measured per layer with the
    copy included (profiles/dense_inplace_kbench.log)."""
    if splitconv_wgrad_takes(N, C, K, H, W):
        return True
    return _SPLITCONV and _SPLITCONV_WGRAD and _inplace_wgrad_rule(int(N), int(C), int(K), int(H), int(W))


def _inplace_wgrad_rule(N, C, K, H, W):
    # the three layers _splitconv_wgrad_rule leaves to MIOpen at 96x160, measured at N = 16 against MIOpen's call on the slice
    # (solver + layout copies + ATen's contiguous copy of x_k): 275->128 -103 us and 403->96 -230 us, ranges apart; 147->128 -24 us,
    # ranges apart in one job and touching in three others -- a tie in time, taken for the 144 MB copy it does not allocate.
    # Never below that size.  (With the 2 x 2 tiles of section 35 _splitconv_wgrad_rule takes all three on its own -- in place the
    # kernel is 260 .. 850 us ahead of MIOpen + copy -- so this rule adds no layer today; it stays as the in-place path's own.)
    return _size_floor(N, H, W, 96, 160) and 128 <= C < 448 and 96 <= K <= 128


class DenseEstimatorFunction(torch.autograd.Function):
    """FlowEstimatorDense (models/pwclite.py:48-66) behind ONE autograd node:

        for k in 1..5:  x_{k+1} = cat([leaky_relu(conv2d(x_k, w_k) + b_k), x_k], 1)
        flow = conv2d(x_6, w_head) + b_head                         -> (x_6, flow)

    The convolutions are the calls the composed path makes (bias-free F.conv2d forward, aten.convolution_backward backward, or
    the split-bf16 kernel where splitconv_takes routes ConvAct's forward / data gradient to it);
    arflow_dense_cat_fwd writes activation and input into their slots of the next tensor, and backward the gradient of layer
    m's activation is gathered by ONE launch from every tensor that holds a slice of it -- the gradient of x_6, the head's
    data gradient and the data gradients of the layers above -- in the nesting autograd's accumulation has, so the values
    MIOpen's backward kernels receive are bit-identical to the composed path's.  Saves x_1 .. x_6 (the activations live
    inside them) and the weights.

    In place: where splitconv_takes routes all five layers' forwards, x_6 is allocated once, x copied
    into its tail, and layer k reads x_6[:, off_k:] and writes lrelu(conv + b_k) into x_6[:, off_k - oc_k:off_k] through the
    kernel's epilogue -- the positions torch.cat gives them; no dense_cat launch, x_1 .. x_5 are views of the one saved x_6.
    ARFLOW_DENSE_INPLACE=0 keeps the path above everywhere."""

    @staticmethod
    def forward(ctx, x, slope, *params):
        if len(params) != 12:
            raise ValueError('dense_estimator expects (w, b) of five layers and of the head')
        _need_gpu(x, *params)
        slope = float(slope)
        ws, bs = params[0:10:2], params[1:10:2]
        w_head, b_head = params[10], params[11]
        ocs = [int(w.shape[0]) for w in ws]
        B, C1, H, W = x.shape
        cins = [C1 + sum(ocs[:k]) for k in range(5)]
        inplace = _DENSE_INPLACE and all(splitconv_takes(B, c, oc, H, W) for c, oc in zip(cins, ocs))
        if inplace:
            off = sum(ocs)
            x6 = torch.empty(B, C1 + off, H, W, device=x.device, dtype=torch.float32)
            x6[:, off:].copy_(x)  # the only copy left: x_k = x6[:, off_k:] from here on
            for w, b, oc in zip(ws, bs, ocs):
                splitconv(x6[:, off:], w, out=x6[:, off - oc:off], bias=b, slope=slope)
                off -= oc
        else:
            xs = [x.contiguous()]
            for w, b in zip(ws, bs):
                xk = xs[-1]
                if splitconv_takes(xk.shape[0], xk.shape[1], w.shape[0], xk.shape[2], xk.shape[3]):  # ConvAct's routing, same kernel
                    y = splitconv(xk, w)
                else:
                    y = torch.nn.functional.conv2d(xk, w, None, 1, 1)
                xs.append(dense_cat(y, b, xk, slope))
            x6 = xs[-1]
        w_head = w_head.contiguous()
        flow = _headconv_fwd(x6, w_head, b_head.contiguous())
        if inplace:
            ctx.save_for_backward(x6, *ws, w_head)
        else:
            ctx.save_for_backward(*xs, *ws, w_head)
        ctx.slope, ctx.inplace = slope, inplace
        ctx.set_materialize_grads(False)
        return x6, flow

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gx6, gflow):
        if ctx.inplace:  # x_1 .. x_5 are channel suffixes of the one saved x_6
            x6, ws, w_head = ctx.saved_tensors[0], ctx.saved_tensors[1:6], ctx.saved_tensors[6]
            tail = [int(w.shape[0]) for w in ws]
            xs = [x6[:, sum(tail[m:]):] for m in range(5)] + [x6]
        else:
            xs, ws, w_head = ctx.saved_tensors[:6], ctx.saved_tensors[6:11], ctx.saved_tensors[11]
        need = ctx.needs_input_grad
        grads = [None] * 14
        if gx6 is None and gflow is None:
            return tuple(grads)
        x6 = xs[5]
        B, C6, H, W = x6.shape
        ocs = [int(w.shape[0]) for w in ws]
        # the lowest layer whose gradient chain has to be followed: 0 = down to the estimator's input
        lowest = 0 if need[0] else next((m for m in range(1, 6) if need[2 * m] or need[2 * m + 1]), 6)
        dx_head = None
        if gflow is not None:
            gflow = gflow.contiguous()
            if lowest < 6:
                dx_head = _headconv_dgrad(gflow, w_head, x6)
            grads[12], grads[13] = _headconv_wgrad(x6, gflow, w_head, need[12], need[13])
        if lowest == 6:
            return tuple(grads)
        # sources in the order autograd adds them: x_6's own gradient, the head's, then the layers' from the top down
        top = [t for t in (gx6, dx_head) if t is not None]
        dxs = []  # (dx_k, k) for k = 5, 4, ...: the gradient of layer k's input x_k
        for m in range(5, max(lowest, 1) - 1, -1):
            # x_k = [a_{k-1}, ..., a_1, x_1]: a_m starts at sum(oc_j, m < j < k)
            srcs = [(t, sum(ocs[m:5]), None) for t in top] + [(dx, sum(ocs[m:k - 1]), None) for dx, k in dxs]
            gy, gb = dense_grad_gather(srcs, ocs[m - 1], act=xs[m], slope=ctx.slope, want_bias=need[2 * m + 1])
            want_dx, want_dw = m > lowest, bool(need[2 * m])
            xm = xs[m - 1]
            # ConvAct's predicates, asked only for what is wanted (a layer of which only the bias is trained needs neither)
            dx_native = want_dx and splitconv_takes(B, ocs[m - 1], xm.shape[1], H, W)
            dw_native = want_dw and (_inplace_wgrad_takes if ctx.inplace else splitconv_wgrad_takes)(B, xm.shape[1], ocs[m - 1], H, W)
            dx, dw = _conv3x3_grads(xm, ws[m - 1], gy, want_dx, want_dw, dx_native, dw_native)
            grads[2 * m], grads[2 * m + 1] = dw, gb
            if want_dx:
                dxs.append((dx, m))
        if need[0]:
            srcs = [(t, sum(ocs), None) for t in top] + [(dx, sum(ocs[:k - 1]), None) for dx, k in dxs]
            grads[0] = dense_grad_gather(srcs, int(xs[0].shape[1]))[0]
        return tuple(grads)


def dense_estimator(x, slope, params):
    """(x6, flow) of FlowEstimatorDense; params = (w1, b1, ..., w5, b5, w_head, b_head)."""
    return DenseEstimatorFunction.apply(x, slope, *params)


# ------------------------------------------------------------------------------------------------
# The dilated context layers as phase mosaics on the split-bf16 kernels (csrc/phase.hip)
_DILATED_CHAIN = __import__('os').environ.get('ARFLOW_DILATED_CHAIN', '1') != '0'  # A/B switch for tools/ and tests: 0 = composed path
DILATED_CHAIN_LAYERS = ((128, 128, 2), (128, 128, 4), (128, 96, 8), (96, 64, 16))  # (C, K, dilation) of ContextNetwork's layers 2..5
# Which of the four weight gradients run arflow_splitconv_wgrad on the virtual tensors; the others are MIOpen's on NCHW copies
# that the permutation passes write as a second destination.  Read off profiles/dilated_kbench.log by section 30's rule -- the
# kernel's max below the min of MIOpen's solver plus its layout copies, at 16 x 96 x 160: d 2 (64 x 48 x 80) 496 (493 .. 498) us
# against 642 (642 .. 656), 1.30x; d 4, 8 and 16 0.70x, 0.76x and 0.66x (many small images: short chunks, and the mosaics'
# 1.2x .. 1.3x pixels), still behind with the two second destinations (20 .. 40 us each) on MIOpen's side.  ARFLOW_DILATED_WGRAD=0101 (one digit per layer) overrides it
# for tools/ and tests.
_DILATED_WGRAD_NATIVE = (True, False, False, False)


def dilated_chain_enabled():
    return _DILATED_CHAIN


def _dilated_wgrad_native():
    env = __import__('os').environ.get('ARFLOW_DILATED_WGRAD')
    if env and len(env) == 4 and set(env) <= {'0', '1'}:
        return tuple(c == '1' for c in env)
    return _DILATED_WGRAD_NATIVE


def phase_layout(N, H, W, d):
    """(Nv, Hv, Wv, Pg, Qg) of layout d of an [N, *, H, W] tensor (csrc/phase_plan.hpp); raises where d > H or d > W."""
    import ctypes
    out = (ctypes.c_int * 5)()
    _lib.check(_lib.load().arflow_phase_layout(int(N), int(H), int(W), int(d), ctypes.cast(out, ctypes.c_void_p)), 'arflow_phase_layout')
    return tuple(out)


def _phase_empty(N, C, H, W, d, device):
    if d == 1:
        return torch.empty(N, C, H, W, device=device, dtype=torch.float32)
    Nv, Hv, Wv, _, _ = phase_layout(N, H, W, d)
    return torch.empty(Nv, C, Hv, Wv, device=device, dtype=torch.float32)


def _phase_check(t, N, H, W, d, what):
    _need_gpu(t)
    Nv, Hv, Wv, _, _ = phase_layout(N, H, W, d)
    if t.dim() != 4 or (t.shape[0], t.shape[2], t.shape[3]) != (Nv, Hv, Wv) or not t.is_contiguous():
        raise ValueError('%s must be a contiguous [%d,C,%d,%d] tensor: layout %d of [%d,C,%d,%d]' % (what, Nv, Hv, Wv, d, N, H, W))


def phase_move(src, real, d_src, d_dst, d_dst2=0, out=None, out2=None):
    """src, layout d_src of an [N,C,H,W] tensor with real = (N, H, W), rewritten in layout d_dst and, for d_dst2 != 0, in that
    layout as well from the one read: (dst, dst2 or None).  Layout 1 is NCHW.  out / out2: tensors of the destinations' shapes
    to write into (every element is stored); they must not share memory with src.  No autograd."""
    N, H, W = (int(v) for v in real)
    _phase_check(src, N, H, W, d_src, 'phase_move: src')
    C = int(src.shape[1])
    dst = _phase_empty(N, C, H, W, d_dst, src.device) if out is None else out
    dst2 = (_phase_empty(N, C, H, W, d_dst2, src.device) if out2 is None else out2) if d_dst2 else None
    for t, d in ((out, d_dst), (out2 if d_dst2 else None, d_dst2)):
        if t is not None:
            _phase_check(t, N, H, W, d, 'phase_move: out')
            if t.shape[1] != C:
                raise ValueError('phase_move: out has %d channels, src %d' % (t.shape[1], C))
    with torch.cuda.device_of(src):
        _call('arflow_phase_move', _p(src), _p(dst), _p(dst2), N, C, H, W, int(d_src), int(d_dst), int(d_dst2), _stream())
    return dst, dst2


def phase_act_bwd(gout, y, real, d_a, d_b, d_b2=0, slope=0.1, want_bias=True):
    """gin = gout * (y > 0 ? 1 : slope) for gout and y in layout d_a, written in layout d_b (and d_b2), and the bias gradient
    over real pixels: (gin, gin2 or None, gbias [C] or None).  No autograd."""
    N, H, W = (int(v) for v in real)
    _phase_check(gout, N, H, W, d_a, 'phase_act_bwd: gout')
    _phase_check(y, N, H, W, d_a, 'phase_act_bwd: y')
    if y.shape != gout.shape:
        raise ValueError('phase_act_bwd: gout and y differ in shape')
    C = int(gout.shape[1])
    gin = _phase_empty(N, C, H, W, d_b, gout.device)
    gin2 = _phase_empty(N, C, H, W, d_b2, gout.device) if d_b2 else None
    rows = None
    if want_bias:
        n = _lib.load().arflow_phase_rows(N, H, W, int(d_b), int(d_b2))
        if n <= 0:
            _lib.check(n, 'arflow_phase_rows')
        rows = torch.empty(n, C, device=gout.device, dtype=torch.float64)
    with torch.cuda.device_of(gout):
        _call('arflow_phase_act_bwd', _p(gout), _p(y), _p(gin), _p(gin2), _p(rows), N, C, H, W, int(d_a), int(d_b), int(d_b2),
              float(slope), _stream())
    return gin, gin2, (None if rows is None else rows.sum(0).float())


def _dilated_wgrad_miopen(x, gy, w, d):
    args = [1, 1], [d, d], [d, d], False, [0, 0], 1
    return torch.ops.aten.convolution_backward(gy, x, w, None, *args, [False, True, False])[1]


class DilatedChainFunction(torch.autograd.Function):
    """ContextNetwork's layers 2..5 (models/pwclite.py:91-106) behind ONE autograd node:

        for k in 2..5:  x = leaky_relu(conv2d(x, w_k, padding=d_k, dilation=d_k) + b_k),   d = 2, 4, 8, 16

    Every convolution is the dilation-1 split-bf16 kernel on the layer's phase mosaic (layout d_k, csrc/phase_plan.hpp) with its
    bias + LeakyReLU epilogue; arflow_phase_move carries the activation from the layout of one layer to the layout of the next
    (five moves where the composed path has four bias / LeakyReLU passes), and backward arflow_phase_act_bwd does the same for
    the gradient while it applies the LeakyReLU derivative and sums the bias gradient.  Saves each layer's input in its own
    layout -- the previous layer's activation, element-aligned with the gradient that meets it -- and the NCHW output.  A weight
    gradient that _DILATED_WGRAD_NATIVE leaves to MIOpen gets its NCHW operands from the second destination of those passes."""

    @staticmethod
    def forward(ctx, x, slope, *params):
        if len(params) != 8:
            raise ValueError('dilated_chain expects (w, b) of four layers')
        _need_gpu(x, *params)
        ws, bs = params[0::2], params[1::2]
        shapes = tuple((int(w.shape[1]), int(w.shape[0]), d) for w, (_, _, d) in zip(ws, DILATED_CHAIN_LAYERS))
        if shapes != DILATED_CHAIN_LAYERS or x.dim() != 4 or x.shape[1] != shapes[0][0]:
            raise ValueError('dilated_chain: the layers are %s' % (DILATED_CHAIN_LAYERS,))
        slope = float(slope)
        ds = [d for _, _, d in DILATED_CHAIN_LAYERS]
        native = _dilated_wgrad_native()
        x = x.contiguous()
        N, _, H, W = x.shape
        real = (N, H, W)
        a, _ = phase_move(x, real, 1, ds[0])
        ins, plain = [], [x]
        for k in range(4):
            ins.append(a)
            y = splitconv(a, ws[k], bias=bs[k], slope=slope)
            if k == 3:
                a, _ = phase_move(y, real, ds[k], 1)
            else:
                a, a_plain = phase_move(y, real, ds[k], ds[k + 1], 0 if native[k + 1] else 1)
                plain.append(a_plain)
        ctx.save_for_backward(a, *ins, *plain, *ws)
        ctx.slope, ctx.real, ctx.native = slope, real, native
        return a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        saved = ctx.saved_tensors
        out, ins, plain, ws = saved[0], saved[1:5], saved[5:9], saved[9:13]
        need = ctx.needs_input_grad
        ds = [d for _, _, d in DILATED_CHAIN_LAYERS]
        grads = [None] * 10
        g, lay, yk = gout.contiguous(), 1, out
        for k in range(3, -1, -1):
            want_dw, want_db = need[2 + 2 * k], need[3 + 2 * k]
            native = ctx.native[k] or not want_dw
            gin, gin_plain, grads[3 + 2 * k] = phase_act_bwd(g, yk, ctx.real, lay, ds[k], 0 if native else 1, ctx.slope, want_db)
            if want_dw:
                grads[2 + 2 * k] = splitconv_wgrad(ins[k], gin) if native else _dilated_wgrad_miopen(plain[k], gin_plain, ws[k], ds[k])
            if k > 0 or need[0]:
                g, lay, yk = splitconv(gin, ws[k], transpose_flip=True), ds[k], ins[k]
        if need[0]:
            grads[0] = phase_move(g, ctx.real, ds[0], 1)[0]
        return tuple(grads)


def dilated_chain(x, slope, params):
    """ContextNetwork's layers 2..5 on x [N,128,H,W]; params = (w2, b2, ..., w5, b5)."""
    return DilatedChainFunction.apply(x, slope, *params)


def dilated_chain_takes(N, H, W):
    """Whether ContextNetwork routes its dilated layers to the node: measured at 16 x 96 x 160 and not below."""
    return _SPLITCONV and _DILATED_CHAIN and _size_floor(int(N), int(H), int(W), 96, 160)


@_samples_mode
class BiasLeakyReLUMomentsFunction(torch.autograd.Function):
    """bias_leaky_relu that also returns the partial moments (sum y, sum y^2) of its output as rows of 2 doubles
    ([B, rows, 2], arflow_bias_act_fwd_mom): normalize_features' moments taken where the feature map is produced."""

    @staticmethod
    def forward(ctx, x, bias, slope):
        _need_gpu(x)
        if not x.is_contiguous():
            raise ValueError('bias_leaky_relu expects a contiguous [B,C,...] tensor')
        B, C = x.shape[0], x.shape[1]
        hw = x[0, 0].numel()
        if bias is not None:
            _need_gpu(bias)
            bias = bias.contiguous()
        rows = _lib.load().arflow_bias_act_mom_rows(C, hw)
        mom = torch.empty(B, rows, 2, device=x.device, dtype=torch.float64)
        with torch.cuda.device_of(x):
            _call('arflow_bias_act_fwd_mom', _p(x), _p(bias), _p(x), _p(mom), B, C, hw, float(slope), _stream(), key=(B, C, hw))
        ctx.mark_dirty(x)
        ctx.mark_non_differentiable(mom)
        ctx.save_for_backward(x)
        ctx.slope, ctx.has_bias = float(slope), bias is not None
        return x, mom

    @staticmethod
    def backward(ctx, gout, gmom_unused):
        y, = ctx.saved_tensors
        B, C = y.shape[0], y.shape[1]
        hw = y[0, 0].numel()
        gout = gout.contiguous()
        gin = torch.empty_like(gout)
        gb = torch.empty(C, device=y.device, dtype=torch.float32) if (ctx.has_bias and ctx.needs_input_grad[1]) else None
        with torch.cuda.device_of(y):
            _call('arflow_bias_act_bwd', _p(gout), _p(y), _p(gin), _p(gb), B, C, hw, ctx.slope, _stream(), key=(B, C, hw))
        return gin, gb, None


def bias_leaky_relu_moments(x, bias, slope=0.1):
    return BiasLeakyReLUMomentsFunction.apply(x, bias, slope)


# ------------------------------------------------------------------------------------------------
@_samples_mode
class WarpFunction(torch.autograd.Function):
    """out = bilinear(src, grid + flow); with ``want_valid`` also the in-image mask of the sampling
    positions (mask_invalid(flow_to_warp(flow)), utils/uflow_utils.py:35-50) from the same launch."""

    @staticmethod
    def forward(ctx, src, flow, pad, align_corners, norm, want_valid=False):
        _need_gpu(src, flow)
        src = src.contiguous()
        flow, fbs = _flow_view(flow)
        B, C, Hs, Ws = src.shape
        _, _, H, W = flow.shape
        if flow.shape[0] != B:
            raise ValueError('batch mismatch between source and flow')
        out = torch.empty(B, C, H, W, device=src.device, dtype=torch.float32)
        valid = torch.empty(B, 1, H, W, device=src.device, dtype=torch.float32) if want_valid else None
        with torch.cuda.device_of(src):
            _call('arflow_warp_fwd', _p(src), _p(flow), _p(out), _p(valid), B, C, Hs, Ws, H, W, fbs, pad,
                  int(bool(align_corners)), norm, _stream(), key=(B, C, H, W))
        ctx.save_for_backward(src, flow)
        ctx.cfg = (pad, int(bool(align_corners)), norm, fbs)
        if want_valid:
            ctx.mark_non_differentiable(valid)
            return out, valid
        return out

    @staticmethod
    def backward(ctx, gout, *unused):
        src, flow = ctx.saved_tensors
        pad, ac, norm, fbs = ctx.cfg
        B, C, Hs, Ws = src.shape
        _, _, H, W = flow.shape
        gout = gout.contiguous()
        gsrc = torch.empty_like(src) if ctx.needs_input_grad[0] else None
        gflow = torch.empty(B, 2, H, W, device=src.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        with torch.cuda.device_of(src):
            _call('arflow_warp_bwd', _p(gout), _p(src), _p(flow), _p(gsrc), _p(gflow), B, C, Hs, Ws, H, W, fbs,
                  pad, ac, norm, _stream(), key=(B, C, H, W, gsrc is not None))
        return gsrc, gflow, None, None, None, None


@_samples_mode
class WarpUp2Function(torch.autograd.Function):
    """The front of a PWC pyramid level as the ARFlow model writes it (models/pwclite.py:178-180):

        flow_up = F.interpolate(flow * 2, scale_factor=2, mode='bilinear', align_corners=up_align)
        out     = flow_warp(src, flow_up)

    as ONE launch (arflow_level_warp_fwd: the upsample is evaluated in front of the warp's coordinate computation; the
    upsampled flow is still written once -- the estimator and the residual sum read it).  Backward: arflow_warp_bwd (both
    gradients w.r.t. the full-resolution flow) + arflow_up2_bwd (the upsample's adjoint as a gather).  Returns
    (out, flow_up)."""

    @staticmethod
    def forward(ctx, src, flow, pad, align_corners, norm, up_align):
        _need_gpu(src, flow)
        src = src.contiguous()
        flow, fbs = _flow_view(flow)
        B, C, H, W = src.shape
        if tuple(flow.shape) != (B, 2, H // 2, W // 2) or H % 2 or W % 2:
            raise ValueError('warp_up2 needs a [B,2,H/2,W/2] flow for a [B,C,H,W] source with even H, W')
        lib = _lib.load()
        out = torch.empty_like(src)
        flow_up = torch.empty(B, 2, H, W, device=src.device, dtype=torch.float32)
        acc = torch.empty(4 * B * lib.arflow_level_acc_rows(B, C, H, W, 1), device=src.device, dtype=torch.float64)  # (moments: unused)
        with torch.cuda.device_of(src):
            _call('arflow_level_warp_fwd', None, _p(src), _p(flow), fbs, 1, int(bool(up_align)), _p(flow_up), None, 0, _p(out),
                  _p(acc), B, C, H, W, pad, int(bool(align_corners)), norm, _stream(), key=(B, C, H, W, 1))
        ctx.save_for_backward(src, flow_up)
        ctx.cfg = (pad, int(bool(align_corners)), norm, int(bool(up_align)))
        return out, flow_up

    @staticmethod
    def backward(ctx, gout, gflow_up):
        src, flow_up = ctx.saved_tensors
        pad, ac, norm, up_align = ctx.cfg
        B, C, H, W = src.shape
        gout = gout.contiguous()
        gsrc = torch.empty_like(src) if ctx.needs_input_grad[0] else None
        gcoarse = None
        with torch.cuda.device_of(src):
            if ctx.needs_input_grad[1]:
                gfull = torch.empty(B, 2, H, W, device=src.device, dtype=torch.float32)
                _call('arflow_warp_bwd', _p(gout), _p(src), _p(flow_up), _p(gsrc), _p(gfull), B, C, H, W, H, W, 2 * H * W, pad, ac,
                      norm, _stream(), key=(B, C, H, W, gsrc is not None))
                if gflow_up is not None:
                    gfull = gfull + gflow_up  # what the estimator and the residual sum sent to the upsampled flow
                gcoarse = torch.empty(B, 2, H // 2, W // 2, device=src.device, dtype=torch.float32)
                _call('arflow_up2_bwd', _p(gfull), _p(gcoarse), B, H, W, up_align, _stream(), key=(B, H, W))
            elif gsrc is not None:
                _call('arflow_warp_bwd', _p(gout), _p(src), _p(flow_up), _p(gsrc), None, B, C, H, W, H, W, 2 * H * W, pad, ac, norm,
                      _stream(), key=(B, C, H, W, True))
        return gsrc, gcoarse, None, None, None, None


def warp_up2(src, flow_coarse, pad='zeros', align_corners=True, norm=None, up_align=True):
    """(flow_warp(src, up), up) with up = interpolate(flow_coarse * 2, x2, bilinear, align_corners=up_align) in one launch."""
    return WarpUp2Function.apply(src, flow_coarse, PAD[pad], align_corners, NORM_ARFLOW if norm is None else norm, up_align)


def warp_up2_supported(src, flow_coarse):
    return (src.is_cuda and src.dtype == torch.float32 and flow_coarse is not None and flow_coarse.is_cuda and src.shape[2] % 2 == 0
            and src.shape[3] % 2 == 0 and tuple(flow_coarse.shape[2:]) == (src.shape[2] // 2, src.shape[3] // 2)
            and flow_coarse.shape[1] == 2)


@_samples_mode
class WarpBF16Function(torch.autograd.Function):
    """Bilinear warp with the SOURCE stored as bf16 (opt-in): sampling arithmetic, output and
    both gradients fp32; the source is rounded to bf16 once and kept as such for the backward."""

    @staticmethod
    def forward(ctx, src, flow, pad, align_corners, norm):
        if not (src.is_cuda and flow.is_cuda):
            raise _lib.ArflowHipError('arflow_amd ops run on the GPU only')
        sb = src.to(torch.bfloat16).contiguous()
        flow, fbs = _flow_view(flow.float())
        B, C, Hs, Ws = sb.shape
        _, _, H, W = flow.shape
        out = torch.empty(B, C, H, W, device=src.device, dtype=torch.float32)
        with torch.cuda.device_of(src):
            _call('arflow_warp_fwd_bf16', _p(sb), _p(flow), _p(out), None, B, C, Hs, Ws, H, W, fbs, pad,
                  int(bool(align_corners)), norm, _stream(), key=(B, C, H, W))
        ctx.save_for_backward(sb, flow)
        ctx.cfg = (pad, int(bool(align_corners)), norm, fbs)
        return out

    @staticmethod
    def backward(ctx, gout):
        sb, flow = ctx.saved_tensors
        pad, ac, norm, fbs = ctx.cfg
        B, C, Hs, Ws = sb.shape
        _, _, H, W = flow.shape
        gout = gout.contiguous()
        gsrc = torch.empty(B, C, Hs, Ws, device=sb.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        gflow = torch.empty(B, 2, H, W, device=sb.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        with torch.cuda.device_of(sb):
            _call('arflow_warp_bwd_bf16', _p(gout), _p(sb), _p(flow), _p(gsrc), _p(gflow), B, C, Hs, Ws, H, W, fbs, pad, ac,
                  norm, _stream(), key=(B, C, H, W, gsrc is not None))
        return gsrc, gflow, None, None, None


@_samples_mode
class WarpNearestFunction(torch.autograd.Function):
    """flow_warp(mode='nearest') (utils/warp_utils.py:83-90): gradient w.r.t. the source only, like grid_sample."""

    @staticmethod
    def forward(ctx, src, flow, pad, align_corners, norm):
        _need_gpu(src, flow)
        src = src.contiguous()
        flow, fbs = _flow_view(flow.detach())
        B, C, Hs, Ws = src.shape
        _, _, H, W = flow.shape
        out = torch.empty(B, C, H, W, device=src.device, dtype=torch.float32)
        with torch.cuda.device_of(src):
            _call('arflow_warp_nearest_fwd', _p(src), _p(flow), _p(out), B, C, Hs, Ws, H, W, fbs, pad,
                  int(bool(align_corners)), norm, _stream())
        ctx.save_for_backward(flow)
        ctx.cfg = (pad, int(bool(align_corners)), norm, fbs, (B, C, Hs, Ws))
        return out

    @staticmethod
    def backward(ctx, gout):
        flow, = ctx.saved_tensors
        pad, ac, norm, fbs, (B, C, Hs, Ws) = ctx.cfg
        _, _, H, W = flow.shape
        gsrc = None
        if ctx.needs_input_grad[0]:
            gout = gout.contiguous()
            gsrc = torch.empty(B, C, Hs, Ws, device=gout.device, dtype=torch.float32)
            with torch.cuda.device_of(gout):
                _call('arflow_warp_nearest_bwd', _p(gout), _p(flow), _p(gsrc), B, C, Hs, Ws, H, W, fbs, pad, ac, norm,
                      _stream())
        # grid_sample's nearest mode returns a ZERO gradient for the grid (not None)
        gflow = torch.zeros(B, 2, H, W, device=gout.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        return gsrc, gflow, None, None, None


def warp_nearest(src, flow, pad='zeros', align_corners=True, norm=NORM_ARFLOW):
    return WarpNearestFunction.apply(src, flow, PAD[pad], align_corners, norm)


@_samples_mode
class WarpBicubicFunction(torch.autograd.Function):
    """flow_warp(mode='bicubic') (utils/warp_utils.py:83-90 -> grid_sample bicubic): both gradients."""

    @staticmethod
    def forward(ctx, src, flow, pad, align_corners, norm):
        _need_gpu(src, flow)
        src = src.contiguous()
        flow, fbs = _flow_view(flow)
        B, C, Hs, Ws = src.shape
        _, _, H, W = flow.shape
        out = torch.empty(B, C, H, W, device=src.device, dtype=torch.float32)
        with torch.cuda.device_of(src):
            _call('arflow_warp_bicubic_fwd', _p(src), _p(flow), _p(out), B, C, Hs, Ws, H, W, fbs, pad, int(bool(align_corners)),
                  norm, _stream())
        ctx.save_for_backward(src, flow)
        ctx.cfg = (pad, int(bool(align_corners)), norm, fbs)
        return out

    @staticmethod
    def backward(ctx, gout):
        src, flow = ctx.saved_tensors
        pad, ac, norm, fbs = ctx.cfg
        B, C, Hs, Ws = src.shape
        _, _, H, W = flow.shape
        gout = gout.contiguous()
        gsrc = torch.empty_like(src) if ctx.needs_input_grad[0] else None
        gflow = torch.empty(B, 2, H, W, device=src.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        with torch.cuda.device_of(src):
            _call('arflow_warp_bicubic_bwd', _p(gout), _p(src), _p(flow), _p(gsrc), _p(gflow), B, C, Hs, Ws, H, W, fbs, pad, ac,
                  norm, _stream())
        return gsrc, gflow, None, None, None


def warp_bicubic(src, flow, pad='zeros', align_corners=True, norm=NORM_ARFLOW):
    return WarpBicubicFunction.apply(src, flow, PAD[pad], align_corners, norm)


class FlowUpsampleFunction(torch.autograd.Function):
    """F.interpolate(flow * factor, scale_factor=factor, mode='bilinear', align_corners) in one launch, with a GATHER
    adjoint (arflow_flow_up_bwd): ATen's backward of that call scatters with float atomics, this one adds in a fixed
    order.  Does not depend on the mode: it is what the models call while the mode is on."""

    @staticmethod
    def forward(ctx, flow, factor, align_corners):
        _need_gpu(flow)
        if flow.dim() != 4 or flow.shape[1] != 2:
            raise ValueError('flow_upsample expects a [B,2,h,w] flow')
        flow = flow.contiguous()
        B, _, h, w = flow.shape
        factor = int(factor)
        out = torch.empty(B, 2, h * factor, w * factor, device=flow.device, dtype=torch.float32)
        with torch.cuda.device_of(flow):
            _call('arflow_flow_up_fwd', _p(flow), _p(out), B, h, w, factor, int(bool(align_corners)), _stream())
        ctx.cfg = (B, h, w, factor, int(bool(align_corners)))
        return out

    @staticmethod
    def backward(ctx, gout):
        B, h, w, factor, ac = ctx.cfg
        gout = gout.contiguous()
        gin = torch.empty(B, 2, h, w, device=gout.device, dtype=torch.float32)
        with torch.cuda.device_of(gout):
            _call('arflow_flow_up_bwd', _p(gout), _p(gin), B, h, w, factor, ac, _stream())
        return gin, None, None


def flow_upsample(flow, factor=2, align_corners=True):
    """flow [B,2,h,w] -> F.interpolate(flow * factor, scale_factor=factor, mode='bilinear', align_corners) for factor 2, 4."""
    return FlowUpsampleFunction.apply(flow, factor, align_corners)


# ---- output upsample of the probabilistic PWC model ----------------------------------------------
_OUT_UP = __import__('os').environ.get('ARFLOW_OUT_UP', '1') != '0'  # A/B switch for tools/ and tests: 0 = composed ATen path


def out_up_supported(x):
    """True where the model routes its output upsamples to out_upsample / out_tail: CUDA fp32, ARFLOW_OUT_UP not 0."""
    return bool(_OUT_UP and x.is_cuda and x.dtype == torch.float32)


def _plane_view(x):
    """Return (tensor, batch_stride) so that a [B,C,H,W] channel slice of a wider tensor is used in place (planes contiguous)."""
    B, C, H, W = x.shape
    st = x.stride()
    if st[3] == 1 and st[2] == W and st[1] == H * W and (B == 1 or st[0] >= C * H * W):
        return x, (st[0] if B > 1 else C * H * W)
    return x.contiguous(), C * H * W


# op name -> (entry-point stem, takes a factor argument).  out_upsample is the x2 align_corners=False resize, prob_upsample
# its align_corners=True sibling for factors 2 and 4 (DESIGN.md sections 22, 27, 38).
_CHAN_UP = {'out_upsample': ('arflow_out_up2', False), 'prob_upsample': ('arflow_prob_up', True)}


def _chan_up_bwd(op, g, B, C, h, w, factor, n_flow):
    """Adjoint of one step of `op`: g [B,C,factor h,factor w] (any channel slice with contiguous planes) -> [B,C,h,w]."""
    stem, has_factor = _CHAN_UP[op]
    f = (factor,) if has_factor else ()
    g, gbs = _plane_view(g)
    gin = torch.empty(B, C, h, w, device=g.device, dtype=torch.float32)
    with torch.cuda.device_of(g):
        _call(stem + '_bwd', _p(g), gbs, _p(gin), C * h * w, B, C, h, w, *f, n_flow, _stream(), key=(B, C, h, w, *f, 'bwd'))
    return gin


class ChannelUpsampleFunction(torch.autograd.Function):
    """out[:, c] = s_c * interpolate(x[:, c] + b_c, x factor, bilinear), s_c = factor for the first n_flow channels, b_c =
    diag_bias for the next n_diag, as one launch: op 'out_upsample' is models/uflow_prob_model.py:223-250 upsample_out
    (x2, align_corners=False), op 'prob_upsample' is models/pwclite_prob.py:183-186,216-217 (x2 or x4, align_corners=True).
    The adjoint is a gather (arflow_out_up2_bwd / arflow_prob_up_bwd): reproducible in either mode, so the node does not
    sample the mode."""

    @staticmethod
    def forward(ctx, out, x, op, factor, n_flow, n_diag, diag_bias):
        # (`out` first: autograd treats input 0 of a node that writes into a view as the tensor modified in place)
        _need_gpu(x, out)
        if x.dim() != 4:
            raise ValueError('%s expects a [B,C,h,w] tensor' % op)
        B, C, h, w = x.shape
        stem, has_factor = _CHAN_UP[op]
        factor, n_flow, n_diag = int(factor), int(n_flow), int(n_diag)
        if has_factor and factor not in (2, 4):
            raise ValueError('%s: factor must be 2 or 4 (got %r)' % (op, factor))
        if n_flow < 0 or n_diag < 0 or n_flow + n_diag > C:
            raise ValueError('%s: n_flow %d + n_diag %d exceed the %d channels' % (op, n_flow, n_diag, C))
        f = (factor,) if has_factor else ()
        x, xbs = _plane_view(x)
        if out is None:
            out = torch.empty(B, C, factor * h, factor * w, device=x.device, dtype=torch.float32)
        else:
            if tuple(out.shape) != (B, C, factor * h, factor * w):
                raise ValueError('%s: out must be [B,C,%dh,%dw]' % (op, factor, factor))
            view, _ = _plane_view(out)
            if view is not out:
                raise ValueError('%s: out must have contiguous planes (a channel slice of a contiguous buffer)' % op)
            ctx.mark_dirty(out)
        _, obs = _plane_view(out)
        with torch.cuda.device_of(x):
            _call(stem + '_fwd', _p(x), xbs, _p(out), obs, B, C, h, w, *f, n_flow, n_diag, float(diag_bias), _stream(),
                  key=(B, C, h, w, *f, 'fwd'))
        ctx.cfg = (op, B, C, h, w, factor, n_flow)
        return out

    @staticmethod
    def backward(ctx, gout):
        op, *dims = ctx.cfg
        return None, _chan_up_bwd(op, gout, *dims), None, None, None, None, None


def out_upsample(x, n_flow, n_diag, diag_bias, out=None):
    """x [B,C,h,w] (may be a channel slice) -> [B,C,2h,2w]; `out` may be a channel slice of a preallocated buffer (it is
    written in place and returned).  diag_bias is a constant: no gradient."""
    return ChannelUpsampleFunction.apply(out, x, 'out_upsample', 2, n_flow, n_diag, diag_bias)


class OutTailFunction(torch.autograd.Function):
    """The model's last two upsample_out calls (level 2 -> level 1 -> level 0) in one launch from one read of x; bitwise
    what two out_upsample calls give.  Backward: two arflow_out_up2_bwd launches (either gradient may be absent)."""

    @staticmethod
    def forward(ctx, x, n_flow, n_diag, diag_bias):
        _need_gpu(x)
        if x.dim() != 4:
            raise ValueError('out_tail expects a [B,C,h,w] tensor')
        B, C, h, w = x.shape
        n_flow, n_diag = int(n_flow), int(n_diag)
        if n_flow < 0 or n_diag < 0 or n_flow + n_diag > C:
            raise ValueError('out_tail: n_flow %d + n_diag %d exceed the %d channels' % (n_flow, n_diag, C))
        x, xbs = _plane_view(x)
        ctx.set_materialize_grads(False)
        out1 = torch.empty(B, C, 2 * h, 2 * w, device=x.device, dtype=torch.float32)
        out0 = torch.empty(B, C, 4 * h, 4 * w, device=x.device, dtype=torch.float32)
        with torch.cuda.device_of(x):
            _call('arflow_out_tail_fwd', _p(x), xbs, _p(out1), _p(out0), B, C, h, w, n_flow, n_diag, float(diag_bias),
                  _stream(), key=(B, C, h, w, 'tail'))
        ctx.cfg = (B, C, h, w, n_flow)
        return out1, out0

    @staticmethod
    def backward(ctx, g1, g0):
        B, C, h, w, n_flow = ctx.cfg
        if g0 is not None:
            g10 = _chan_up_bwd('out_upsample', g0, B, C, 2 * h, 2 * w, 2, n_flow)
            g1 = g10 if g1 is None else g1 + g10
        if g1 is None:
            return None, None, None, None
        return _chan_up_bwd('out_upsample', g1, B, C, h, w, 2, n_flow), None, None, None


def out_tail(x, n_flow, n_diag, diag_bias):
    """x [B,C,h,w] -> (out1 [B,C,2h,2w], out0 [B,C,4h,4w]) = (out_upsample(x), out_upsample(out_upsample(x)))."""
    return OutTailFunction.apply(x, n_flow, n_diag, diag_bias)


def prob_upsample(x, factor, n_flow, n_diag, diag_bias, out=None):
    """x [B,C,h,w] (may be a channel slice) -> [B,C,factor h,factor w], factor 2 or 4, align_corners=True; `out` may be a
    channel slice of a preallocated buffer (it is written in place and returned).  diag_bias is a constant: no gradient."""
    return ChannelUpsampleFunction.apply(out, x, 'prob_upsample', factor, n_flow, n_diag, diag_bias)


def interpolate_flow(flow, factor, align_corners):
    """The models' flow upsample: ATen's F.interpolate in default mode (unchanged), flow_upsample in deterministic mode."""
    if flow.is_cuda and flow.dtype == torch.float32 and is_deterministic():
        return flow_upsample(flow, factor, align_corners)
    return torch.nn.functional.interpolate(flow * factor, scale_factor=factor, mode='bilinear', align_corners=align_corners)


def warp(src, flow, pad='zeros', align_corners=True, norm=NORM_ARFLOW, storage=None):
    if _storage(storage) == 'bf16':
        return WarpBF16Function.apply(src, flow, PAD[pad], align_corners, norm)
    return WarpFunction.apply(src, flow, PAD[pad], align_corners, norm)


def warp_with_valid(src, flow, pad='zeros', align_corners=True, norm=NORM_ARFLOW):
    """(warped, valid mask) in one launch."""
    return WarpFunction.apply(src, flow, PAD[pad], align_corners, norm, True)


def _flow_map(name, flow, *extra):
    _need_gpu(flow)
    flow, fbs = _flow_view(flow.detach())
    B, _, H, W = flow.shape
    out = torch.empty(B, 1, H, W, device=flow.device, dtype=torch.float32)
    with torch.cuda.device_of(flow):
        _call(name, _p(flow), _p(out), B, H, W, fbs, *extra, _stream(), key=(B, H, W))
    return out


def splat_map(flow, variant):
    """variant 0: compute_range_map; 1: get_corresponding_map(grid + flow).  No gradient (the
    reference detaches / thresholds it: losses/uflow_loss.py:43, utils/warp_utils.py:112)."""
    return _flow_map('arflow_splat_map', flow, int(variant))


def coord_mask(flow, mode):
    """mode 0: mask_invalid(flow_to_warp(flow)); 1: border_mask(flow)."""
    return _flow_map('arflow_coord_mask', flow, int(mode))


def occ_bidir(flow12, flow21, scale=0.01, bias=0.5):
    _need_gpu(flow12, flow21)
    f12, s12 = _flow_view(flow12.detach())
    f21, s21 = _flow_view(flow21.detach())
    B, _, H, W = f12.shape
    out = torch.empty(B, 1, H, W, device=f12.device, dtype=torch.float32)
    with torch.cuda.device_of(f12):
        _call('arflow_occ_bidir', _p(f12), _p(f21), _p(out), B, H, W, s12, s21, float(scale), float(bias), _stream(),
              key=(B, H, W))
    return out


# ------------------------------------------------------------------------------------------------
class CensusLossFunction(torch.autograd.Function):
    """census_loss(image_a, image_b, mask, patch) of utils/uflow_utils.py:282-293 as one fused
    forward launch and one backward launch.  The mask is treated as a constant (the reference
    passes a detached mask, losses/uflow_loss.py:43,48)."""

    @staticmethod
    def forward(ctx, im_a, im_b, mask, patch_size):
        _need_gpu(im_a, im_b, mask)
        im_a, im_b, mask = im_a.contiguous(), im_b.contiguous(), mask.contiguous()
        B, C, H, W = im_a.shape
        if C != 3 or im_b.shape != im_a.shape or mask.shape != (B, 1, H, W):
            raise ValueError('census_loss expects [B,3,H,W] images and a [B,1,H,W] mask')
        r = int(patch_size) // 2
        buf = _new_sums(im_a.device, B, H, W)
        dham = torch.empty(B, 1, H, W, device=im_a.device, dtype=torch.float32)
        with torch.cuda.device_of(im_a):
            _call('arflow_census_fwd', _p(im_a), _p(im_b), _p(mask), None, _p(dham), _p(buf), B, H, W, r, _stream(),
                  key=(B, H, W))
        sums = _fold_sums(buf, 2)
        # sharded batch + global normalisation: divide by the mask sum of ALL ranks (ddp.global_denominator);
        # identity when that is off (the default)
        den = _ddp.global_denominator(sums[1]) + 1e-6 / _ddp.world_size()
        inv = 1.0 / den
        ctx.save_for_backward(im_a, im_b, dham, inv)
        ctx.r = r
        return sums[0] * inv

    @staticmethod
    def backward(ctx, gloss):
        im_a, im_b, dham, inv = ctx.saved_tensors
        B, _, H, W = im_a.shape
        scale = (gloss * inv).reshape(1).contiguous()
        ga = gb = None
        with torch.cuda.device_of(im_a):
            if ctx.needs_input_grad[1]:
                gb = torch.empty_like(im_b)
                _call('arflow_census_bwd', _p(im_a), _p(im_b), _p(dham), _p(scale), _p(gb), B, H, W, ctx.r, _stream(),
                      key=(B, H, W))
            if ctx.needs_input_grad[0]:
                ga = torch.empty_like(im_a)  # the distance is symmetric in (a, b)
                _call('arflow_census_bwd', _p(im_b), _p(im_a), _p(dham), _p(scale), _p(ga), B, H, W, ctx.r, _stream(),
                      key=(B, H, W))
        return ga, gb, None, None


class CensusWarpLossFunction(torch.autograd.Function):
    """One photometric direction of UFlowLoss (losses/uflow_loss.py:30-54) as ONE launch each way:
    census_loss(im_a, resample(im_b, flow_to_warp(flow)), upsample(clamp(occ_small,0,1), x4) * mask_invalid(...)),
    on the grey planes (x255) of the two images (``gray255``).  Returns (loss, mask).  Gradient w.r.t. the flow only
    (the reference detaches the sampled image and the mask, losses/uflow_loss.py:31,34,43,48)."""

    @staticmethod
    def forward(ctx, gray_a, gray_b, flow, occ_small, patch_size):
        _need_gpu(gray_a, gray_b, flow, occ_small)
        gray_a, gray_b = gray_a.detach().contiguous(), gray_b.detach().contiguous()
        flow, fbs = _flow_view(flow)
        B, C, H, W = gray_a.shape
        if C != 1 or gray_b.shape != gray_a.shape or flow.shape != (B, 2, H, W):
            raise ValueError('census_warp_loss expects [B,1,H,W] grey planes and a [B,2,H,W] flow')
        if occ_small is not None:
            occ_small = occ_small.detach().contiguous()
            if occ_small.shape != (B, 1, H // 4, W // 4):
                raise ValueError('occ_small must be the [B,1,H/4,W/4] range map')
        r = int(patch_size) // 2
        buf = _new_sums(gray_a.device, B, H, W)
        dham = torch.empty(B, 1, H, W, device=gray_a.device, dtype=torch.float32)
        mask = torch.empty(B, 1, H, W, device=gray_a.device, dtype=torch.float32)
        with torch.cuda.device_of(gray_a):
            _call('arflow_census_warp_fwd', _p(gray_a), _p(gray_b), _p(flow), fbs, _p(occ_small), _p(mask), _p(dham),
                  _p(buf), B, H, W, r, _stream(), key=(B, H, W))
        sums = _fold_sums(buf, 2)
        den = _ddp.global_denominator(sums[1]) + 1e-6 / _ddp.world_size()
        inv = 1.0 / den
        ctx.save_for_backward(gray_a, gray_b, flow, dham, inv)
        ctx.r, ctx.fbs = r, fbs
        ctx.mark_non_differentiable(mask)
        return sums[0] * inv, mask

    @staticmethod
    def backward(ctx, gloss, gmask_unused):
        gray_a, gray_b, flow, dham, inv = ctx.saved_tensors
        B, _, H, W = gray_a.shape
        scale = (gloss * inv).reshape(1).contiguous()
        gflow = torch.empty(B, 2, H, W, device=gray_a.device, dtype=torch.float32)
        with torch.cuda.device_of(gray_a):
            _call('arflow_census_warp_bwd', _p(gray_a), _p(gray_b), _p(flow), ctx.fbs, _p(dham), _p(scale), _p(gflow),
                  B, H, W, ctx.r, _stream(), key=(B, H, W))
        return None, None, gflow, None, None


class CensusWarpPairLossFunction(torch.autograd.Function):
    """BOTH photometric directions of UFlowLoss (losses/uflow_loss.py:30-54) as ONE launch each way.  The batch holds
    2B samples s = 2 b + direction: ``gray2`` the grey planes (x255) of the [B,6,H,W] pair viewed as [2B,3,H,W], ``flow2``
    the [B,4,H,W] (fw, bw) flows viewed as [2B,2,H,W], ``occ_small2`` the range maps of the 2B level-2 flows (sample s is
    masked by plane s ^ 1).  Returns (loss fw, loss bw, mask [2B,1,H,W]); gradient w.r.t. the flows only."""

    @staticmethod
    def forward(ctx, gray2, flow2, occ_small2, patch_size):
        _need_gpu(gray2, flow2, occ_small2)
        gray2 = gray2.detach().contiguous()
        flow2, fbs = _flow_view(flow2)
        B2, C, H, W = gray2.shape
        if C != 1 or B2 % 2 or flow2.shape != (B2, 2, H, W):
            raise ValueError('census_warp_pair_loss expects [2B,1,H,W] grey planes and [2B,2,H,W] flows')
        occ_small2 = occ_small2.detach().contiguous()
        if occ_small2.shape != (B2, 1, H // 4, W // 4):
            raise ValueError('occ_small2 must be the [2B,1,H/4,W/4] range maps')
        r = int(patch_size) // 2
        buf = _new_sums(gray2.device, B2, H, W)
        dham = torch.empty(B2, 1, H, W, device=gray2.device, dtype=torch.float32)
        mask = torch.empty(B2, 1, H, W, device=gray2.device, dtype=torch.float32)
        with torch.cuda.device_of(gray2):
            _call('arflow_census_warp_pair_fwd', _p(gray2), _p(flow2), fbs, _p(occ_small2), _p(mask), _p(dham), _p(buf), B2, H,
                  W, r, _stream(), key=(B2, H, W))
        sums = _fold_sums(buf, 4)
        den = torch.stack([_ddp.global_denominator(sums[1]), _ddp.global_denominator(sums[3])]) + 1e-6 / _ddp.world_size()
        inv = 1.0 / den
        ctx.save_for_backward(gray2, flow2, dham, inv)
        ctx.r, ctx.fbs = r, fbs
        ctx.mark_non_differentiable(mask)
        return sums[0] * inv[0], sums[2] * inv[1], mask

    @staticmethod
    def backward(ctx, g0, g1, gmask_unused):
        gray2, flow2, dham, inv = ctx.saved_tensors
        B2, _, H, W = gray2.shape
        scale = (torch.stack([g0.reshape(()), g1.reshape(())]) * inv).contiguous()
        gflow = torch.empty(B2, 2, H, W, device=gray2.device, dtype=torch.float32)
        with torch.cuda.device_of(gray2):
            _call('arflow_census_warp_pair_bwd', _p(gray2), _p(flow2), ctx.fbs, _p(dham), _p(scale), _p(gflow), B2, H, W, ctx.r,
                  _stream(), key=(B2, H, W))
        return None, gflow, None, None


def census_warp_pair_loss(gray2, flow2, occ_small2, patch_size=7):
    return CensusWarpPairLossFunction.apply(gray2, flow2, occ_small2, patch_size)


class UFlowPairLossFunction(torch.autograd.Function):
    """Both loss terms of UFlowLoss for both directions (losses/uflow_loss.py:30-102) behind ONE autograd node: forward =
    arflow_splat_smooth_fwd (range maps + smoothness sums of the level-2 flows) + arflow_census_warp_pair_fwd; backward = ONE
    launch (arflow_uflow_pair_bwd: census + warp backward and smoothness backward as workgroup roles).  Batch layout as
    CensusWarpPairLossFunction (sample s = 2 b + direction).  Returns (census loss fw, census loss bw, smoothness sums [2],
    mask [2B,1,H,W]); gradients w.r.t. the level-0 and level-2 flows."""

    @staticmethod
    def forward(ctx, gray2, small2, flow0, flow2, occ_zeroed, alpha, order, patch_size):
        _need_gpu(gray2, small2, flow0, flow2)
        gray2, small2 = gray2.detach().contiguous(), small2.detach().contiguous()
        flow0, fbs0 = _flow_view(flow0)
        flow2, fbs2 = _flow_view(flow2)
        B2, _, H, W = gray2.shape
        h, w = flow2.shape[2:]
        if B2 % 2 or flow0.shape != (B2, 2, H, W) or (h, w) != (H // 4, W // 4) or small2.shape != (B2, 3, h, w):
            raise ValueError('uflow_pair_loss: inconsistent shapes')
        r = int(patch_size) // 2
        pre = occ_zeroed is not None
        occ = occ_zeroed if pre else torch.empty(B2, 1, h, w, device=gray2.device, dtype=torch.float32)
        sbuf = _new_sums(gray2.device, B2, h, w)
        cbuf = _new_sums(gray2.device, B2, H, W)
        dham = torch.empty(B2, 1, H, W, device=gray2.device, dtype=torch.float32)
        mask = torch.empty(B2, 1, H, W, device=gray2.device, dtype=torch.float32)
        with torch.cuda.device_of(gray2):
            _call('arflow_splat_smooth_fwd', _p(flow2), _p(small2), _p(occ), _p(sbuf), B2, h, w, fbs2, 1.0, float(alpha),
                  int(order), 1, 1, int(pre), _stream(), key=(B2, 3, h, w))
            _call('arflow_census_warp_pair_fwd', _p(gray2), _p(flow0), fbs0, _p(occ), _p(mask), _p(dham), _p(cbuf), B2, H, W, r,
                  _stream(), key=(B2, H, W))
        sums = _fold_sums(cbuf, 4)
        den = torch.stack([_ddp.global_denominator(sums[1]), _ddp.global_denominator(sums[3])]) + 1e-6 / _ddp.world_size()
        inv = 1.0 / den
        ctx.save_for_backward(gray2, small2, flow0, flow2, dham, inv)
        ctx.cfg = (r, fbs0, fbs2, float(alpha), int(order))
        ctx.mark_non_differentiable(mask)
        return sums[0] * inv[0], sums[2] * inv[1], _fold_sums(sbuf, 2), mask

    @staticmethod
    def backward(ctx, g0, g1, gs, gmask_unused):
        gray2, small2, flow0, flow2, dham, inv = ctx.saved_tensors
        r, fbs0, fbs2, alpha, order = ctx.cfg
        B2, _, H, W = gray2.shape
        h, w = flow2.shape[2:]
        scale = (torch.stack([g0.reshape(()), g1.reshape(())]) * inv).contiguous()
        coef = gs.contiguous()
        gf0 = torch.empty(B2, 2, H, W, device=gray2.device, dtype=torch.float32)
        gf2 = torch.empty(B2, 2, h, w, device=gray2.device, dtype=torch.float32)
        with torch.cuda.device_of(gray2):
            _call('arflow_uflow_pair_bwd', _p(gray2), _p(flow0), fbs0, _p(dham), _p(scale), _p(gf0), B2, H, W, r, _p(flow2),
                  fbs2, _p(small2), _p(coef), _p(gf2), h, w, 1.0, alpha, order, 1, 1, _stream(), key=(B2, H, W))
        return None, None, gf0, gf2, None, None, None, None


def uflow_pair_loss(gray2, small2, flow0, flow2, occ_zeroed, alpha, order, patch_size=7):
    return UFlowPairLossFunction.apply(gray2, small2, flow0, flow2, occ_zeroed, alpha, order, patch_size)


def census_warp_supported(H, W):
    return bool(_lib.load().arflow_census_warp_supported(int(H), int(W)))


def census_warp_loss(gray_a, gray_b, flow, occ_small, patch_size=7):
    return CensusWarpLossFunction.apply(gray_a, gray_b, flow, occ_small, patch_size)


# ---- selectable penalties (csrc/penalty_dev.hpp) -------------------------------------------------
PEN_KINDS = {'identity': _lib.PEN_IDENTITY, 'charbonnier': _lib.PEN_CHARBONNIER, 'abs_robust_loss': _lib.PEN_ABS_ROBUST}


def make_penalty(name, pi=None, beta=None, squared=False):
    """The host descriptor (arflow_penalty_t) of a penalty: 'identity', 'charbonnier', 'abs_robust_loss', or 'gmm' with the
    mixture (pi, beta) -- the data-term form rho(h), or with squared=True the smoothness form rho(x^2).  The weights
    w_j = pi_j sqrt(beta_j) / sqrt(2 pi) are formed in float64 and rounded to fp32 once, like beta_j."""
    import math
    d = _lib.Penalty()
    if name in PEN_KINDS:
        d.kind, d.k = PEN_KINDS[name], 0
        return d
    if name != 'gmm':
        raise ValueError('penalty %r (known: identity, charbonnier, abs_robust_loss, gmm)' % (name,))
    from .losses.penalty_functions import check_mixture  # (imported here: that module builds on this one)
    pi, beta = check_mixture(pi, beta, "penalty 'gmm'")
    d.kind, d.k = (_lib.PEN_GMM_SQ if squared else _lib.PEN_GMM), len(pi)
    for j, (p, b) in enumerate(zip(pi, beta)):
        d.w[j] = p * math.sqrt(b) / math.sqrt(2.0 * math.pi)
        d.beta[j] = b
    return d


def _pen_ptr(pen):
    import ctypes
    return ctypes.addressof(pen)


class CensusPenLossFunction(torch.autograd.Function):
    """CensusLossFunction with the penalty `pen` (make_penalty) in place of abs_robust_loss: arflow_census_pen_fwd; the
    backward is CensusLossFunction's (arflow_census_bwd reads dham = pm rho'(ham))."""

    @staticmethod
    def forward(ctx, im_a, im_b, mask, patch_size, pen):
        _need_gpu(im_a, im_b, mask)
        im_a, im_b, mask = im_a.contiguous(), im_b.contiguous(), mask.contiguous()
        B, C, H, W = im_a.shape
        if C != 3 or im_b.shape != im_a.shape or mask.shape != (B, 1, H, W):
            raise ValueError('census_pen_loss expects [B,3,H,W] images and a [B,1,H,W] mask')
        r = int(patch_size) // 2
        buf = _new_sums(im_a.device, B, H, W)
        ham = torch.empty(B, 1, H, W, device=im_a.device, dtype=torch.float32)
        dham = torch.empty(B, 1, H, W, device=im_a.device, dtype=torch.float32)
        with torch.cuda.device_of(im_a):
            _call('arflow_census_pen_fwd', _p(im_a), _p(im_b), _p(mask), _p(ham), _p(dham), _p(buf), B, H, W, r, _pen_ptr(pen),
                  _stream(), key=(B, H, W))
        sums = _fold_sums(buf, 2)
        den = _ddp.global_denominator(sums[1]) + 1e-6 / _ddp.world_size()
        inv = 1.0 / den
        ctx.save_for_backward(im_a, im_b, dham, inv)
        ctx.r = r
        return sums[0] * inv

    @staticmethod
    def backward(ctx, gloss):
        return CensusLossFunction.backward(ctx, gloss) + (None,)


def census_pen_loss(im_a, im_b, mask, pen, patch_size=7):
    return CensusPenLossFunction.apply(im_a, im_b, mask, patch_size, pen)


def _valid_view(valid_flow, shape):
    if valid_flow is None:
        return None, 0
    valid_flow, vbs = _flow_view(valid_flow.detach())
    _need_gpu(valid_flow)
    if valid_flow.shape != shape:
        raise ValueError('valid_flow must have the shape of the flow')
    return valid_flow, vbs


class CensusWarpPenLossFunction(torch.autograd.Function):
    """CensusWarpLossFunction with the penalty `pen` and an optional validity flow (mask_invalid is taken of `valid_flow`
    while the warp samples at `flow`): arflow_census_warp_pen_fwd; backward arflow_census_warp_bwd, as there."""

    @staticmethod
    def forward(ctx, gray_a, gray_b, flow, occ_small, patch_size, pen, valid_flow):
        _need_gpu(gray_a, gray_b, flow, occ_small)
        gray_a, gray_b = gray_a.detach().contiguous(), gray_b.detach().contiguous()
        flow, fbs = _flow_view(flow)
        B, C, H, W = gray_a.shape
        if C != 1 or gray_b.shape != gray_a.shape or flow.shape != (B, 2, H, W):
            raise ValueError('census_warp_pen_loss expects [B,1,H,W] grey planes and a [B,2,H,W] flow')
        if occ_small is not None:
            occ_small = occ_small.detach().contiguous()
            if occ_small.shape != (B, 1, H // 4, W // 4):
                raise ValueError('occ_small must be the [B,1,H/4,W/4] range map')
        valid_flow, vbs = _valid_view(valid_flow, flow.shape)
        r = int(patch_size) // 2
        buf = _new_sums(gray_a.device, B, H, W)
        dham = torch.empty(B, 1, H, W, device=gray_a.device, dtype=torch.float32)
        mask = torch.empty(B, 1, H, W, device=gray_a.device, dtype=torch.float32)
        with torch.cuda.device_of(gray_a):
            _call('arflow_census_warp_pen_fwd', _p(gray_a), _p(gray_b), _p(flow), fbs, _p(occ_small), _p(mask), _p(dham),
                  _p(buf), B, H, W, r, _p(valid_flow), vbs, _pen_ptr(pen), _stream(), key=(B, H, W))
        sums = _fold_sums(buf, 2)
        den = _ddp.global_denominator(sums[1]) + 1e-6 / _ddp.world_size()
        inv = 1.0 / den
        ctx.save_for_backward(gray_a, gray_b, flow, dham, inv)
        ctx.r, ctx.fbs = r, fbs
        ctx.mark_non_differentiable(mask)
        return sums[0] * inv, mask

    @staticmethod
    def backward(ctx, gloss, gmask_unused):
        return CensusWarpLossFunction.backward(ctx, gloss, gmask_unused) + (None, None)


def census_warp_pen_loss(gray_a, gray_b, flow, occ_small, pen, valid_flow=None, patch_size=7):
    return CensusWarpPenLossFunction.apply(gray_a, gray_b, flow, occ_small, patch_size, pen, valid_flow)


class CensusWarpPairPenLossFunction(torch.autograd.Function):
    """CensusWarpPairLossFunction with the penalty `pen` and an optional validity flow: arflow_census_warp_pair_pen_fwd;
    backward arflow_census_warp_pair_bwd, as there."""

    @staticmethod
    def forward(ctx, gray2, flow2, occ_small2, patch_size, pen, valid_flow2):
        _need_gpu(gray2, flow2, occ_small2)
        gray2 = gray2.detach().contiguous()
        flow2, fbs = _flow_view(flow2)
        B2, C, H, W = gray2.shape
        if C != 1 or B2 % 2 or flow2.shape != (B2, 2, H, W):
            raise ValueError('census_warp_pair_pen_loss expects [2B,1,H,W] grey planes and [2B,2,H,W] flows')
        occ_small2 = occ_small2.detach().contiguous()
        if occ_small2.shape != (B2, 1, H // 4, W // 4):
            raise ValueError('occ_small2 must be the [2B,1,H/4,W/4] range maps')
        valid_flow2, vbs = _valid_view(valid_flow2, flow2.shape)
        r = int(patch_size) // 2
        buf = _new_sums(gray2.device, B2, H, W)
        dham = torch.empty(B2, 1, H, W, device=gray2.device, dtype=torch.float32)
        mask = torch.empty(B2, 1, H, W, device=gray2.device, dtype=torch.float32)
        with torch.cuda.device_of(gray2):
            _call('arflow_census_warp_pair_pen_fwd', _p(gray2), _p(flow2), fbs, _p(occ_small2), _p(mask), _p(dham), _p(buf), B2,
                  H, W, r, _p(valid_flow2), vbs, _pen_ptr(pen), _stream(), key=(B2, H, W))
        sums = _fold_sums(buf, 4)
        den = torch.stack([_ddp.global_denominator(sums[1]), _ddp.global_denominator(sums[3])]) + 1e-6 / _ddp.world_size()
        inv = 1.0 / den
        ctx.save_for_backward(gray2, flow2, dham, inv)
        ctx.r, ctx.fbs = r, fbs
        ctx.mark_non_differentiable(mask)
        return sums[0] * inv[0], sums[2] * inv[1], mask

    @staticmethod
    def backward(ctx, g0, g1, gmask_unused):
        return CensusWarpPairLossFunction.backward(ctx, g0, g1, gmask_unused) + (None, None)


def census_warp_pair_pen_loss(gray2, flow2, occ_small2, pen, valid_flow2=None, patch_size=7):
    return CensusWarpPairPenLossFunction.apply(gray2, flow2, occ_small2, patch_size, pen, valid_flow2)


class SmoothPenSumsFunction(torch.autograd.Function):
    """SmoothSumsFunction with the penalty `pen` applied to the SQUARED flow differences (losses/uflow_elbo_loss.py:507-533):
    arflow_smooth_pen_fwd / _bwd.  Gradient w.r.t. flow only."""

    @staticmethod
    def forward(ctx, flow, img, flow_scale, alpha, order, wmode, pen):
        _need_gpu(flow, img)
        flow, fbs = _flow_view(flow)
        img = img.contiguous()
        B, _, H, W = flow.shape
        Ci = img.shape[1]
        if img.shape[0] != B or img.shape[2:] != flow.shape[2:]:
            raise ValueError('smoothness: image and flow must share batch and spatial size')
        buf = _new_sums(flow.device, B, H, W)
        args = (B, Ci, H, W, fbs, float(flow_scale), float(alpha), int(order), int(wmode))
        with torch.cuda.device_of(flow):
            _call('arflow_smooth_pen_fwd', _p(flow), _p(img), _p(buf), *args, _pen_ptr(pen), _stream(), key=(B, Ci, H, W))
        ctx.save_for_backward(flow, img)
        ctx.args, ctx.pen = args, pen
        return _fold_sums(buf, 2)

    @staticmethod
    def backward(ctx, gsums):
        flow, img = ctx.saved_tensors
        B, _, H, W = flow.shape
        coef = gsums.contiguous()
        g = torch.empty(B, 2, H, W, device=flow.device, dtype=torch.float32)
        with torch.cuda.device_of(flow):
            _call('arflow_smooth_pen_bwd', _p(flow), _p(img), _p(coef), _p(g), *ctx.args, _pen_ptr(ctx.pen), _stream(),
                  key=(B, img.shape[1], H, W))
        return g, None, None, None, None, None, None


def smooth_pen_sums(flow, img, flow_scale, alpha, order, wmode, pen):
    return SmoothPenSumsFunction.apply(flow, img, flow_scale, alpha, order, wmode, pen)


def down4_gray(img, want_small=True, zero_plane=False):
    """(downsample(img, x1/4) or None, rgb_to_grayscale(img) * 255) from ONE read of the image (no gradient: the
    reference applies both to data only, losses/uflow_loss.py:59-60, utils/uflow_utils.py:248).  zero_plane=True also
    returns a zero-filled [B,1,H/4,W/4] plane cleared by the same launch (the splat target of splat_smooth)."""
    _need_gpu(img)
    img = img.detach().contiguous()
    B, C, H, W = img.shape
    if C != 3:
        raise ValueError('down4_gray expects a [B,3,H,W] image')
    small = torch.empty(B, 3, H // 4, W // 4, device=img.device, dtype=torch.float32) if want_small else None
    gray = torch.empty(B, 1, H, W, device=img.device, dtype=torch.float32)
    zero = torch.empty(B, 1, H // 4, W // 4, device=img.device, dtype=torch.float32) if zero_plane else None
    with torch.cuda.device_of(img):
        _call('arflow_down4_gray_z', _p(img), _p(small), _p(gray), _p(zero), B, H, W, _stream(), key=(B, H, W))
    return (small, gray, zero) if zero_plane else (small, gray)


class TernaryDistFunction(torch.autograd.Function):
    """Per-pixel soft census distance (sum over the patch); TernaryLoss core,
    losses/loss_blocks.py:12-62."""

    @staticmethod
    def forward(ctx, im_a, im_b, radius):
        _need_gpu(im_a, im_b)
        im_a, im_b = im_a.contiguous(), im_b.contiguous()
        B, C, H, W = im_a.shape
        if C != 3 or im_b.shape != im_a.shape:
            raise ValueError('ternary distance expects two [B,3,H,W] images')
        ham = torch.empty(B, 1, H, W, device=im_a.device, dtype=torch.float32)
        with torch.cuda.device_of(im_a):
            _call('arflow_census_fwd', _p(im_a), _p(im_b), None, _p(ham), None, None, B, H, W, int(radius), _stream())
        ctx.save_for_backward(im_a, im_b)
        ctx.r = int(radius)
        return ham

    @staticmethod
    def backward(ctx, gham):
        im_a, im_b = ctx.saved_tensors
        B, _, H, W = im_a.shape
        gham = gham.contiguous()
        ga = gb = None
        with torch.cuda.device_of(im_a):
            if ctx.needs_input_grad[0]:
                ga = torch.empty_like(im_a)
                _call('arflow_census_bwd', _p(im_b), _p(im_a), _p(gham), None, _p(ga), B, H, W, ctx.r, _stream())
            if ctx.needs_input_grad[1]:
                gb = torch.empty_like(im_b)
                _call('arflow_census_bwd', _p(im_a), _p(im_b), _p(gham), None, _p(gb), B, H, W, ctx.r, _stream())
        return ga, gb, None


# ------------------------------------------------------------------------------------------------
class PhotoSumsFunction(torch.autograd.Function):
    """[sum |im-recons|*mask, sum SSIMdist(recons*mask, im*mask), sum mask] in one launch
    (losses/flow_loss.py:13-27).  Gradient w.r.t. recons only."""

    @staticmethod
    def forward(ctx, im, recons, mask):
        _need_gpu(im, recons, mask)
        im, recons = im.contiguous(), recons.contiguous()
        mask = None if mask is None else mask.contiguous()
        B, C, H, W = im.shape
        buf = _new_sums(im.device, B, H, W)
        with torch.cuda.device_of(im):
            _call('arflow_photo_fwd', _p(im), _p(recons), _p(mask), None, _p(buf), B, C, H, W, _stream(),
                  key=(B, C, H, W))
        ctx.save_for_backward(im, recons, mask)
        return _fold_sums(buf, 3)

    @staticmethod
    def backward(ctx, gsums):
        im, recons, mask = ctx.saved_tensors
        B, C, H, W = im.shape
        coef = gsums[:2].contiguous()
        g = torch.empty_like(recons)
        with torch.cuda.device_of(im):
            _call('arflow_photo_bwd', _p(im), _p(recons), _p(mask), None, _p(coef), _p(g), B, C, H, W, _stream(),
                  key=(B, C, H, W))
        return None, g, None


class SSIMAnyFunction(torch.autograd.Function):
    """SSIM(x, y, md) distance map of losses/loss_blocks.py:65-84 for any md (md = 1: SSIMFunction, the tiled kernel)."""

    @staticmethod
    def forward(ctx, x, y, md):
        _need_gpu(x, y)
        x, y = x.contiguous(), y.contiguous()
        B, C, H, W = x.shape
        md = int(md)
        out = torch.empty(B, C, H - 2 * md, W - 2 * md, device=x.device, dtype=torch.float32)
        with torch.cuda.device_of(x):
            _call('arflow_ssim_fwd', _p(x), _p(y), _p(out), B, C, H, W, md, _stream())
        ctx.save_for_backward(x, y)
        ctx.md = md
        return out

    @staticmethod
    def backward(ctx, gmap):
        x, y = ctx.saved_tensors
        B, C, H, W = x.shape
        gmap = gmap.contiguous()
        gx = gy = None
        with torch.cuda.device_of(x):
            if ctx.needs_input_grad[0]:
                gx = torch.empty_like(x)
                _call('arflow_ssim_bwd', _p(x), _p(y), _p(gmap), _p(gx), B, C, H, W, ctx.md, _stream())
            if ctx.needs_input_grad[1]:
                gy = torch.empty_like(y)  # SSIM is symmetric in its arguments
                _call('arflow_ssim_bwd', _p(y), _p(x), _p(gmap), _p(gy), B, C, H, W, ctx.md, _stream())
        return gx, gy, None


class SSIMFunction(torch.autograd.Function):
    """SSIM(x, y, md=1) distance map of losses/loss_blocks.py:65-84."""

    @staticmethod
    def forward(ctx, x, y):
        _need_gpu(x, y)
        x, y = x.contiguous(), y.contiguous()
        B, C, H, W = x.shape
        out = torch.empty(B, C, H - 2, W - 2, device=x.device, dtype=torch.float32)
        sums = _new_sums(x.device, B, H, W)
        with torch.cuda.device_of(x):
            # kernel convention: SSIM(recons*mask, im*mask) -> x plays "recons", y plays "im"
            _call('arflow_photo_fwd', _p(y), _p(x), None, _p(out), _p(sums), B, C, H, W, _stream())
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, gmap):
        x, y = ctx.saved_tensors
        B, C, H, W = x.shape
        gmap = gmap.contiguous()
        coef = torch.zeros(2, device=x.device, dtype=torch.float32)
        gx = gy = None
        with torch.cuda.device_of(x):
            if ctx.needs_input_grad[0]:
                gx = torch.empty_like(x)
                _call('arflow_photo_bwd', _p(y), _p(x), None, _p(gmap), _p(coef), _p(gx), B, C, H, W, _stream())
            if ctx.needs_input_grad[1]:
                gy = torch.empty_like(y)  # SSIM is symmetric in its arguments
                _call('arflow_photo_bwd', _p(x), _p(y), None, _p(gmap), _p(coef), _p(gy), B, C, H, W, _stream())
        return gx, gy


# ------------------------------------------------------------------------------------------------
class SmoothSumsFunction(torch.autograd.Function):
    """[sum wx*pen(Dx flow), sum wy*pen(Dy flow)] (losses/loss_blocks.py:93-124,
    losses/uflow_loss.py:62-102).  Gradient w.r.t. flow only (the image is detached / data)."""

    @staticmethod
    def forward(ctx, flow, img, flow_scale, alpha, order, wmode, penalty):
        _need_gpu(flow, img)
        flow, fbs = _flow_view(flow)
        img = img.contiguous()
        B, _, H, W = flow.shape
        Ci = img.shape[1]
        if img.shape[0] != B or img.shape[2:] != flow.shape[2:]:
            raise ValueError('smoothness: image and flow must share batch and spatial size')
        buf = _new_sums(flow.device, B, H, W)
        args = (B, Ci, H, W, fbs, float(flow_scale), float(alpha), int(order), int(wmode), int(penalty))
        with torch.cuda.device_of(flow):
            _call('arflow_smooth_fwd', _p(flow), _p(img), _p(buf), *args, _stream(), key=(B, Ci, H, W))
        ctx.save_for_backward(flow, img)
        ctx.args = args
        return _fold_sums(buf, 2)

    @staticmethod
    def backward(ctx, gsums):
        flow, img = ctx.saved_tensors
        B, _, H, W = flow.shape
        coef = gsums.contiguous()
        g = torch.empty(B, 2, H, W, device=flow.device, dtype=torch.float32)
        with torch.cuda.device_of(flow):
            _call('arflow_smooth_bwd', _p(flow), _p(img), _p(coef), _p(g), *ctx.args, _stream(),
                  key=(B, img.shape[1], H, W))
        return g, None, None, None, None, None, None


def smooth_sums(flow, img, flow_scale, alpha, order, wmode, penalty):
    return SmoothSumsFunction.apply(flow, img, flow_scale, alpha, order, wmode, penalty)


class SplatSmoothFunction(torch.autograd.Function):
    """(smoothness sums of SmoothSumsFunction, compute_range_map(flow)) from ONE launch (arflow_splat_smooth_fwd): UFlowLoss
    takes both from the same level-2 flows.  ``range_out``: a ZERO-FILLED [B,1,H,W] plane (down4_gray(zero_plane=True)) or
    None (cleared here).  The range map carries no gradient (the reference detaches it, losses/uflow_loss.py:43)."""

    @staticmethod
    def forward(ctx, flow, img, range_out, flow_scale, alpha, order, wmode, penalty):
        _need_gpu(flow, img)
        flow, fbs = _flow_view(flow)
        img = img.contiguous()
        B, _, H, W = flow.shape
        if img.shape != (B, 3, H, W):
            raise ValueError('splat_smooth expects a [B,3,H,W] image at the resolution of the flow')
        pre = range_out is not None
        if not pre:
            range_out = torch.empty(B, 1, H, W, device=flow.device, dtype=torch.float32)
        buf = _new_sums(flow.device, B, H, W)
        args = (B, 3, H, W, fbs, float(flow_scale), float(alpha), int(order), int(wmode), int(penalty))
        with torch.cuda.device_of(flow):
            _call('arflow_splat_smooth_fwd', _p(flow), _p(img), _p(range_out), _p(buf), B, H, W, fbs, float(flow_scale),
                  float(alpha), int(order), int(wmode), int(penalty), int(pre), _stream(), key=(B, 3, H, W))
        ctx.save_for_backward(flow, img)
        ctx.args = args
        ctx.mark_non_differentiable(range_out)
        return _fold_sums(buf, 2), range_out

    @staticmethod
    def backward(ctx, gsums, g_unused):
        flow, img = ctx.saved_tensors
        B, _, H, W = flow.shape
        coef = gsums.contiguous()
        g = torch.empty(B, 2, H, W, device=flow.device, dtype=torch.float32)
        with torch.cuda.device_of(flow):
            _call('arflow_smooth_bwd', _p(flow), _p(img), _p(coef), _p(g), *ctx.args, _stream(), key=(B, 3, H, W))
        return g, None, None, None, None, None, None, None


def splat_smooth(flow, img, range_out, flow_scale, alpha, order, wmode, penalty):
    return SplatSmoothFunction.apply(flow, img, range_out, flow_scale, alpha, order, wmode, penalty)


# ------------------------------------------------------------------------------------------------
def down4(img):
    """downsample(img, is_flow=False, scale_factor=4) for H, W multiples of 4 (no gradient: the
    reference only applies it to images, losses/uflow_loss.py:59-60)."""
    _need_gpu(img)
    img = img.detach().contiguous()
    B, C, H, W = img.shape
    out = torch.empty(B, C, H // 4, W // 4, device=img.device, dtype=torch.float32)
    with torch.cuda.device_of(img):
        _call('arflow_down4', _p(img), _p(out), B * C, H, W, _stream(), key=(B * C, H, W))
    return out


def up4_clamp_mul(small, valid=None):
    """upsample(clamp(small,0,1), x4) * valid -- losses/uflow_loss.py:41-48, no gradient."""
    _need_gpu(small, valid)
    small = small.detach().contiguous()
    B, one, h, w = small.shape
    assert one == 1
    valid = None if valid is None else valid.detach().contiguous()
    out = torch.empty(B, 1, 4 * h, 4 * w, device=small.device, dtype=torch.float32)
    with torch.cuda.device_of(small):
        _call('arflow_up4_clamp_mul', _p(small), _p(valid), _p(out), B, h, w, _stream(), key=(B, h, w))
    return out


# ------------------------------------------------------------------------------------------------
# Fused warp + mask + L1/SSIM sums of one pyramid scale (csrc/photo_warp.hip)
_PHOTO_WARP = __import__('os').environ.get('ARFLOW_PHOTO_WARP', '1') != '0'  # A/B switch for tools/ and tests: 0 = composed path
MASK_MODE = {'plane': 0, 'nearest': 1, 'border': 2}


def photo_warp_enabled():
    return _PHOTO_WARP


def _group_views(views, C, H, W, what):
    """(base pointer, sample stride, second-group offset) in floats of G same-shaped [B,C,H,W] views whose planes are dense
    -- slices of one tensor or separate tensors: the kernel reads them where they are."""
    v0 = views[0]
    for v in views:
        if v.shape != v0.shape or v.stride() != v0.stride():
            raise ValueError('%s: the groups must share shape and strides' % what)
    B = v0.shape[0]
    st = v0.stride()
    if tuple(v0.shape[1:]) != (C, H, W) or st[3] != 1 or st[2] != W or (C > 1 and st[1] != H * W):
        raise ValueError('%s: expected [B,%d,%d,%d] views with dense planes, got %s strides %s' % (what, C, H, W, tuple(v0.shape), st))
    half = 0
    if len(views) == 2:
        d = views[1].data_ptr() - v0.data_ptr()
        assert d % 4 == 0
        half = d // 4
    return v0.data_ptr(), (st[0] if B > 1 else C * H * W), half


def photo_warp_supported(frames, flow, mask_size=None):
    """Can the fused pass run this scale?  frames: the full-resolution [B,3k,H0,W0] tensor the images are area-resized
    from; flow: this scale's flow; mask_size: (H, W) of a fine mask plane that is nearest-resized to this scale."""
    h, w = flow.shape[-2:]
    H0, W0 = frames.shape[-2:]
    if h < 3 or w < 3 or H0 % h or W0 % w or H0 // h != W0 // w:
        return False
    if mask_size is not None and (mask_size[0] % h or mask_size[1] % w):
        return False
    return all(t.is_cuda and t.dtype == torch.float32 for t in (frames, flow))


class PhotoWarpSumsFunction(torch.autograd.Function):
    """[G,3] = per group [sum |tgt-rec|*m, sum SSIMdist(rec*m, tgt*m), sum m] with rec = flow_warp(src, flow, pad), in one
    launch; the backward is one launch that writes d/d flow.  flow_a alone: a [B,2G,H,W] tensor holding the groups' flows
    in its channels; flow_a and flow_b: two [B,2,H,W] tensors.  No gradient w.r.t. images or mask."""

    @staticmethod
    def forward(ctx, flow_a, flow_b, tgt, src, mask, pad, mask_mode, mask_invert, want_mask):
        G = len(tgt)
        _need_gpu(flow_a, flow_b, *tgt, *src, *(mask or ()))
        B, C, H, W = tgt[0].shape
        if flow_b is None:
            if flow_a.shape != (B, 2 * G, H, W) or not flow_a.is_contiguous():
                flow_a = flow_a.contiguous()
            if flow_a.shape != (B, 2 * G, H, W):
                raise ValueError('flow must be [B,%d,H,W] for %d groups' % (2 * G, G))
            fl = (_p(flow_a), 2 * G * H * W, 2 * H * W)
        else:
            if G != 2:
                raise ValueError('two flow tensors need two groups')
            flow_a, flow_b = flow_a.contiguous(), flow_b.contiguous()
            fl = _group_views((flow_a, flow_b), 2, H, W, 'flow')
        tg = _group_views(tgt, C, H, W, 'target')
        sr = _group_views(src, C, H, W, 'source')
        mh, mw = H, W
        if mask_mode == MASK_MODE['border']:
            mk = (None, 0, 0)
        else:
            mh, mw = mask[0].shape[-2:]
            if mask_mode == MASK_MODE['plane'] and (mh, mw) != (H, W):
                raise ValueError('mask plane must have the size of the flow')
            mk = _group_views(mask, 1, mh, mw, 'mask')
        lib = _lib.load()
        nrows = lib.arflow_photo_warp_rows(G * B, H, W)
        if nrows <= 0:
            _lib.check(nrows, 'arflow_photo_warp_rows')
        rows = torch.empty(nrows, SUM_COLS, device=flow_a.device, dtype=torch.float32)
        mout = torch.empty(G * B, 1, H, W, device=flow_a.device, dtype=torch.float32) if want_mask else None
        ctx.common = (*tg, *sr, *fl, *mk, int(mask_mode), int(bool(mask_invert)), mh, mw)
        ctx.dims = (B, G, C, H, W, int(pad))
        with torch.cuda.device_of(flow_a):
            _call('arflow_photo_warp_fwd', *ctx.common, _p(mout), _p(rows), *ctx.dims, _stream(), key=(G * B, C, H, W))
        ctx.save_for_backward(flow_a, flow_b, *tgt, *src, *(mask or ()))  # (keeps the addressed storage alive)
        sums = rows.view(G, nrows // G, SUM_COLS)[:, :, :3].sum(1)  # fixed order: reproducible
        if want_mask:
            ctx.mark_non_differentiable(mout)
            return sums, mout
        return sums

    @staticmethod
    def backward(ctx, gsums, *unused):
        flow_a, flow_b = ctx.saved_tensors[:2]
        B, G, C, H, W, pad = ctx.dims
        coef = gsums[:, :2].contiguous()
        ga = torch.empty_like(flow_a)
        gb = None
        if flow_b is None:
            gf = (_p(ga), 2 * G * H * W, 2 * H * W)
        else:
            gb = torch.empty_like(flow_b)
            gf = _group_views((ga, gb), 2, H, W, 'flow gradient')
        with torch.cuda.device_of(flow_a):
            _call('arflow_photo_warp_bwd', *ctx.common, _p(coef), *gf, *ctx.dims, _stream(), key=(G * B, C, H, W))
        return ga, gb, None, None, None, None, None, None, None


def photo_warp_sums(tgt, src, flow, mask=None, pad='zeros', mask_mode='plane', mask_invert=False, want_mask=False):
    """Photometric sums of one pyramid scale without the warped image ever existing in memory.

    tgt, src: tuples of G (1 or 2) [B,C,H,W] views (C <= 3) -- target / source image of every group, read in place (slices
    of one tensor or separate tensors with equal strides).  flow: one [B,2G,H,W] tensor (group g = channels 2g:2g+2) or a
    tuple of two [B,2,H,W] tensors.  mask: tuple of G [B,1,h,w] views for mask_mode 'plane' (h, w = H, W) and 'nearest'
    (a fine plane, integer factors), ignored for 'border' (= border_mask(flow)); mask_invert uses 1 - mask.
    Returns the [G,3] sums (and the [G*B,1,H,W] mask planes used when want_mask)."""
    tgt, src = tuple(tgt), tuple(src)
    if isinstance(flow, (tuple, list)):
        fa, fb = flow if len(flow) == 2 else (flow[0], None)
    else:
        fa, fb = flow, None
    mask = None if mask is None else tuple(mask)
    if len(tgt) not in (1, 2) or len(src) != len(tgt) or (mask is not None and len(mask) != len(tgt)):
        raise ValueError('photo_warp_sums: one or two groups, the same number of targets, sources and masks')
    if mask is None and mask_mode != 'border':
        raise ValueError("photo_warp_sums: mask_mode %r needs a mask" % mask_mode)
    return PhotoWarpSumsFunction.apply(fa, fb, tgt, src, mask, PAD[pad], MASK_MODE[mask_mode], mask_invert, want_mask)


def area_pyramid(frames, sizes):
    """[F.interpolate(frames, s, mode='area') for s in sizes] in one launch (integer factors; every scale from the
    full-resolution pixels).  A size equal to the frames' own returns `frames` itself."""
    import ctypes
    _need_gpu(frames)
    frames = frames.contiguous()
    B, C, H, W = frames.shape
    sizes = [(int(h), int(w)) for h, w in sizes]
    n = len(sizes)
    arr = (ctypes.c_int * (2 * n))(*[v for s in sizes for v in s])
    host = ctypes.cast(arr, ctypes.c_void_p)
    buf = _workspace('arflow_area_pyramid_ws_bytes', B * C, H, W, host, n, device=frames.device).view(torch.float32)
    if buf.numel():
        with torch.cuda.device_of(frames):
            _call('arflow_area_pyramid', _p(frames), _p(buf), B * C, H, W, host, n, _stream(), key=(B * C, H, W, n))
    out, off = [], 0
    for h, w in sizes:
        if (h, w) == (H, W):
            out.append(frames)
        else:
            out.append(buf[off:off + B * C * h * w].view(B, C, h, w))
            off += B * C * h * w
    return out


# ---- ground-truth flow metrics -------------------------------------------------
EVAL_COLS = 8  # doubles per row of arflow_flow_eval


def flow_eval_sums(pred, gt, move=None, want_map=False):
    """The per-sample sums behind evaluate_flow (utils/flow_utils.py:121-183) in one launch: pred [B,2,h,w] is scaled,
    resized to the ground truth's size and compared with gt [B,C,H,W] (C = 2 dense, C = 4 with the valid and non-occluded
    masks in channels 2, 3); move: [B,1,H,W] moving mask or None.  -> sums [B,8] float64 on the device (columns: include/
    arflow_hip.h; arflow_amd.metrics.metrics_from_sums turns them into the reference's metrics), and the end-point-error
    map [B,1,H,W] as well if want_map.  No autograd, no synchronisation."""
    _need_gpu(pred, gt, move)
    if pred.dim() != 4 or pred.shape[1] != 2 or gt.dim() != 4 or gt.shape[0] != pred.shape[0]:
        raise ValueError('flow_eval_sums expects pred [B,2,h,w] and gt [B,C,H,W]')
    B, C, H, W = gt.shape
    if move is not None and tuple(move.shape) != (B, 1, H, W):
        raise ValueError('flow_eval_sums expects move [B,1,H,W]')
    h, w = pred.shape[2:]
    lib = _lib.load()
    nrows = lib.arflow_flow_eval_rows(int(H), int(W))
    if nrows <= 0:
        _lib.check(nrows, 'arflow_flow_eval_rows')
    with torch.no_grad():
        pred, gt = pred.detach().contiguous(), gt.detach().contiguous()
        move = None if move is None else move.detach().contiguous()
        rows = torch.empty(B, nrows, EVAL_COLS, device=gt.device, dtype=torch.float64)
        epe_map = torch.empty(B, 1, H, W, device=gt.device, dtype=torch.float32) if want_map else None
        with torch.cuda.device_of(gt):
            _call('arflow_flow_eval', _p(pred), _p(gt), _p(move), _p(rows), _p(epe_map), B, h, w, C, H, W, _stream(),
                  key=(B, h, w, C, H, W))
        sums = rows.sum(1)  # fixed order: reproducible
    return (sums, epe_map) if want_map else sums


# ---- uncertainty metrics ---------------------------------------------------------
PREP_COLS = 8       # doubles per row of arflow_uncert_prep: min / max of ent_map, min / max of epe_map, sum valid, 0, 0, 0
SPARSIFY_MAX_K = 32
CALIB_MAX_EDGES = 128


def _valid_plane(gt, B, H, W):
    """gt (contiguous, or None) -> (pointer of the validity plane of sample 0 or None, batch stride in floats).  A ground
    truth [B,4,H,W] keeps the mask in channel 2 and it is read where it lies; [B,2,H,W] has none (all ones); [B,1,H,W] is
    a mask on its own."""
    if gt is None or (gt.dim() == 4 and gt.shape[1] == 2):
        return None, 0
    if gt.dim() != 4 or gt.shape[1] not in (1, 4) or (gt.shape[0], gt.shape[2], gt.shape[3]) != (B, H, W):
        raise ValueError('expected a ground truth [B,2|4,H,W] or a mask [B,1,H,W] of the maps\' size, got %s'
                         % (tuple(gt.shape),))
    C = gt.shape[1]
    return gt.data_ptr() + (2 * H * W * 4 if C == 4 else 0), C * H * W


def _uncert_rows(H, W, which='arflow_uncert_rows'):
    n = getattr(_lib.load(), which)(int(H), int(W))
    if n <= 0:
        _lib.check(n, which)
    return n


def uncert_prep(ent, epe_map, gt=None):
    """Steps 2-4 of evaluate_uncertainty (utils/flow_utils.py:296-307) in one launch: ent [B,2,h,w] is shifted by
    -2 log w + 2 log W (channel 0) and -2 log h + 2 log H (channel 1), resized to epe_map's size [B,1,H,W] by the half-pixel
    bilinear rule and summed over its channels, all in fp32 and in the reference's order.  gt: the ground truth [B,2|4,H,W]
    whose channel 2 is the validity mask, or None.  -> ent_map [B,1,H,W] fp32, stats [B,5] float64 on the device: min and
    max of ent_map, min and max of epe_map (over all pixels, masked or not: the bracket of sp_plot, :193-194), sum valid.
    No autograd, no synchronisation."""
    import math
    import numpy as np
    _need_gpu(ent, epe_map, gt)
    if ent.dim() != 4 or ent.shape[1] != 2 or epe_map.dim() != 4 or epe_map.shape[:2] != (ent.shape[0], 1):
        raise ValueError('uncert_prep expects ent [B,2,h,w] and epe_map [B,1,H,W]')
    B, _, H, W = epe_map.shape
    h, w = ent.shape[2:]
    nrows = _uncert_rows(H, W)
    # a float32 array minus, then plus, a Python float: numpy rounds the scalar to float32 first
    off = [float(np.float32(2 * math.log(v))) for v in (w, W, h, H)]
    with torch.no_grad():
        ent, epe_map = ent.detach().contiguous(), epe_map.detach().contiguous()
        gt = None if gt is None else gt.detach().contiguous()
        vp, vs = _valid_plane(gt, B, H, W)
        rows = torch.empty(B, nrows, PREP_COLS, device=ent.device, dtype=torch.float64)
        ent_map = torch.empty(B, 1, H, W, device=ent.device, dtype=torch.float32)
        with torch.cuda.device_of(ent):
            _call('arflow_uncert_prep', _p(ent), _p(epe_map), vp, vs, _p(ent_map), _p(rows), *off, B, h, w, H, W, _stream(),
                  key=(B, h, w, H, W))
        stats = torch.stack([rows[:, :, 0].amin(1), rows[:, :, 1].amax(1), rows[:, :, 2].amin(1), rows[:, :, 3].amax(1),
                             rows[:, :, 4].sum(1)], 1)
    return ent_map, stats


def sparsify_sums(err, field0, field1, gt, thr, alpha):
    """The sums of sp_mask and splot (utils/flow_utils.py:187-190, :222) for a whole batch, F fields and K thresholds in one
    launch: err, field0, field1 (or None: F = 1) [B,1,H,W] fp32; gt as in uncert_prep, or a mask [B,1,H,W]; thr [B,F,K] float64 on the device,
    K <= 32.  -> [B,F,K,3] float64 on the device: sum (1-m) g, sum m g, sum err m g with m = expit(alpha (thr - field)).
    No autograd, no synchronisation."""
    _need_gpu(err, field0, field1, gt)
    B, one, H, W = err.shape
    F = 1 if field1 is None else 2
    if one != 1 or field0.shape != err.shape or (field1 is not None and field1.shape != err.shape):
        raise ValueError('sparsify_sums expects err, field0, field1 [B,1,H,W]')
    if thr.dim() != 3 or thr.shape[:2] != (B, F) or thr.dtype != torch.float64 or thr.device != err.device:
        raise ValueError('sparsify_sums expects thr [B,%d,K] float64 on %s' % (F, err.device))
    K = thr.shape[2]
    nrows = _uncert_rows(H, W)
    with torch.no_grad():
        err, field0 = err.detach().contiguous(), field0.detach().contiguous()
        field1 = None if field1 is None else field1.detach().contiguous()
        gt = None if gt is None else gt.detach().contiguous()
        thr = thr.detach().contiguous()
        vp, vs = _valid_plane(gt, B, H, W)
        rows = torch.empty(B, nrows, F, K, 3, device=err.device, dtype=torch.float64)
        with torch.cuda.device_of(err):
            _call('arflow_sparsify_sums', _p(err), _p(field0), _p(field1), vp, vs, _p(thr), float(alpha), _p(rows), B, H, W, K,
                  _stream(), key=(B, H, W, F, K))
        return rows.sum(1)  # fixed order: reproducible


def calib_hist_sums(pred, gt, ent, edges):
    """The pooled bins of CalibrationCurve.__call__ (utils/flow_utils.py:237-254) in one launch: pred, ent [B,2,H,W] and
    gt [B,2|4,H,W] of one size, edges [nb] ascending float64 on the device, nb <= 128.  -> [nb+1,3] float64 on the device:
    per np.digitize bin of exp(ent) the count, the sum and the sum of squares of |scaled pred - gt| over both channels of all
    samples (the validity mask is not applied, as in the reference).  No autograd, no synchronisation."""
    _need_gpu(pred, gt, ent)
    if pred.dim() != 4 or pred.shape[1] != 2 or gt.dim() != 4 or ent.shape != pred.shape:
        raise ValueError('calib_hist_sums expects pred, ent [B,2,H,W] and gt [B,C,H,W]')
    B, C, H, W = gt.shape
    if tuple(pred.shape) != (B, 2, H, W):
        raise ValueError('calib_hist_sums: the prediction %s must have the ground truth\'s size %s (the reference indexes '
                         'the error with the entropy\'s bins)' % (tuple(pred.shape[2:]), (H, W)))
    if edges.dim() != 1 or edges.dtype != torch.float64 or edges.device != pred.device:
        raise ValueError('calib_hist_sums expects edges [nb] float64 on %s' % pred.device)
    nb = edges.shape[0]
    nrows = _uncert_rows(H, W, 'arflow_calib_rows')
    with torch.no_grad():
        pred, gt, ent, edges = (t.detach().contiguous() for t in (pred, gt, ent, edges))
        rows = torch.empty(B, nrows, nb + 1, 3, device=pred.device, dtype=torch.float64)
        with torch.cuda.device_of(pred):
            _call('arflow_calib_hist', _p(pred), _p(gt), _p(ent), _p(edges), _p(rows), B, C, H, W, nb, _stream(),
                  key=(B, C, H, W, nb))
        return rows.sum((0, 1))  # fixed order: reproducible
