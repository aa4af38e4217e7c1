"""On-device batch augmentation on the native kernels of csrc/augment.hip: the raw uint8 batch is
uploaded once and BOTH versions the trainer needs (trainer/uflow_trainer.py:35-54) come out of one pass over it --

    img     geometric only                  -> the loss        transforms/geometric_transforms.py:7-15  crop -> hflip -> scale
    img_ph  geometric + photometric         -> the model       transforms/photometric_transforms.py:7-25  ColorJitter -> gamma
                                                                                                         -> channel permutation

src is [B,F,3,Hs,Ws] (or the same memory as [B,3F,Hs,Ws]), uint8 (torchvision's pil_to_tensor) or float32 in [0,1]; both outputs
are float32 [B,3F,h,w], the img_pair layout of the models and losses.  The per-sample parameters are drawn on the HOST by one
seeded CPU generator (draw_params) and travel as one small int32 table (include/arflow_hip.h, ARFLOW_AUG_*); all frames of a
sample share its row, as the reference's transforms see the stacked frames.  Ground truth is left untouched, as in the
reference (datasets/flow_datasets.py:37): BatchAugment.last_params tells a caller the windows and flips to crop its own targets.

GPU only: a CPU tensor raises ArflowHipError.  No autograd: these are inputs.
"""
import numpy as np
import torch

from . import _lib
from .functional import _call, _p, _stream

__all__ = ['AugmentParams', 'draw_params', 'augment_batch', 'BatchAugment', 'valid_transform', 'OPS']

OPS = ('brightness', 'contrast', 'saturation', 'hue')  # the operation numbers of the table's order word
ROW = 16
Y1, X1, FLAGS, ORDER, PERM, FACTOR, GAMMA = 0, 1, 2, 3, 4, 5, 9
FLIP, GAMMA_ON = 1, 32
IDENTITY_PERM = 0 | (1 << 2) | (2 << 4)
MAX_FRAMES = 5
GAMMA_RANGE = (0.7, 1.5)  # photometric_transforms.py:20


def active_bit(op):
    return 2 << op


def _get(cfg, key, default=0):
    """A missing key (or a missing config) reads as off."""
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        v = cfg.get(key, default)
    else:
        v = getattr(cfg, key, default)
    return default if v is None else v


def _size(v, name):
    if v is None:
        raise ValueError('%s is missing' % name)
    if isinstance(v, (int, float)):
        v = (int(v), int(v))
    v = tuple(int(s) for s in v)
    if len(v) != 2 or min(v) < 1:
        raise ValueError('%s must be (height, width) >= 1 (got %r)' % (name, v))
    return v


class AugmentParams:
    """The parameters of one batch: `table` int32 [B,16] on the CPU (the layout of include/arflow_hip.h), the window size
    every sample shares and what is configured.  y1 / x1 / flip / order / factors / gamma / perm read the table back."""

    def __init__(self, table, src_hw, crop_hw, scale_hw, photometric):
        self.table = table
        self.src_hw, self.crop_hw, self.scale_hw = tuple(src_hw), tuple(crop_hw), (None if scale_hw is None else tuple(scale_hw))
        self.photometric = bool(photometric)
        self._dev = {}

    B = property(lambda self: int(self.table.shape[0]))
    out_hw = property(lambda self: self.crop_hw if self.scale_hw is None else self.scale_hw)
    y1 = property(lambda self: self.table[:, Y1])
    x1 = property(lambda self: self.table[:, X1])
    flip = property(lambda self: (self.table[:, FLAGS] & FLIP) != 0)
    gamma_on = property(lambda self: (self.table[:, FLAGS] & GAMMA_ON) != 0)
    order = property(lambda self: torch.stack([(self.table[:, ORDER] >> (2 * k)) & 3 for k in range(4)], 1))
    perm = property(lambda self: torch.stack([(self.table[:, PERM] >> (2 * c)) & 3 for c in range(3)], 1))
    factors = property(lambda self: self.table[:, FACTOR:FACTOR + 4].contiguous().view(torch.float32))
    gamma = property(lambda self: self.table[:, GAMMA:GAMMA + 1].contiguous().view(torch.float32)[:, 0])

    def active(self, op):
        return (self.table[:, FLAGS] & active_bit(OPS.index(op) if isinstance(op, str) else op)) != 0

    def device_table(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.table.to(device)
        return self._dev[key]


def make_params(src_hw, crop_hw, y1, x1, flip=None, order=None, active=None, factors=None, gamma=None, perm=None, scale_hw=None):
    """A table from explicit values (what draw_params draws): y1, x1 [B] ints; flip [B] bools; order [B,4] a permutation of
    0..3 per sample; active [B,4] bools and factors [B,4] floats indexed by OPERATION (OPS); gamma [B] floats (None or nan:
    off); perm [B,3] (None: identity).  photometric is set when anything photometric is given."""
    y1 = np.asarray(y1, dtype=np.int64)
    B = y1.shape[0]
    t = np.zeros((B, ROW), dtype=np.int32)
    t[:, Y1], t[:, X1] = y1, np.asarray(x1, dtype=np.int64)
    flags = np.zeros(B, dtype=np.int64)
    if flip is not None:
        flags |= np.asarray(flip, dtype=bool) * FLIP
    order = np.tile(np.arange(4), (B, 1)) if order is None else np.asarray(order, dtype=np.int64)
    if order.shape != (B, 4) or (np.sort(order, 1) != np.arange(4)).any():
        raise ValueError('order must be [B,4], a permutation of 0..3 per sample')
    t[:, ORDER] = sum(order[:, k] << (2 * k) for k in range(4))
    if active is not None:
        active = np.asarray(active, dtype=bool)
        f32 = np.ascontiguousarray(np.asarray(factors, dtype=np.float32))
        if active.shape != (B, 4) or f32.shape != (B, 4):
            raise ValueError('active and factors must be [B,4]')
        flags |= sum(active[:, op] * active_bit(op) for op in range(4))
        t[:, FACTOR:FACTOR + 4] = f32.view(np.int32)
    if gamma is not None:
        gm = np.ascontiguousarray(np.asarray(gamma, dtype=np.float32))
        on = ~np.isnan(gm)
        flags |= on * GAMMA_ON
        t[:, GAMMA] = np.where(on, gm, np.float32(1)).astype(np.float32).view(np.int32)
    perm = np.tile(np.arange(3), (B, 1)) if perm is None else np.asarray(perm, dtype=np.int64)
    if perm.shape != (B, 3) or (np.sort(perm, 1) != np.arange(3)).any():
        raise ValueError('perm must be [B,3], a permutation of 0..2 per sample')
    t[:, PERM] = sum(perm[:, c] << (2 * c) for c in range(3))
    t[:, FLAGS] = flags
    photometric = active is not None or gamma is not None or (perm != np.arange(3)).any()
    return AugmentParams(torch.from_numpy(t), src_hw, crop_hw, scale_hw, photometric)


def _uniform(g, B, lo, hi):
    return (lo + (hi - lo) * torch.rand(B, generator=g, dtype=torch.float64)).to(torch.float32).numpy()


def draw_params(geometric_aug, photometric_aug, B, src_hw, generator):
    """The per-sample table of one batch from ONE seeded CPU generator.  Ranges as the reference and torchvision's
    ColorJitter.get_params draw them: brightness / contrast / saturation value v -> U[max(0, 1 - v), 1 + v], hue v in [0, 0.5] ->
    U[-v, v] (each inactive at 0), the four operations in a random order per sample whenever ColorJitter is present (any of the
    four non-zero, photometric_transforms.py:14), gamma U[0.7, 1.5] when cfg.gamma > 0, a random channel permutation with
    swap_channels, the crop origin uniform over the valid integers (geometric_transforms.py:47-48), a flip with probability
    1/2.  Only what is configured is drawn."""
    B = int(B)
    Hs, Ws = _size(src_hw, 'src_hw')
    g = generator
    if B < 1:
        raise ValueError('B must be >= 1 (got %r)' % (B,))
    th, tw = (Hs, Ws)
    if _get(geometric_aug, 'crop', False):
        th, tw = _size(_get(geometric_aug, 'crop_size', None) or _get(geometric_aug, 'para_crop', None), 'crop_size')
        if th > Hs or tw > Ws:
            raise ValueError('crop_size %r does not fit the source %r' % ((th, tw), (Hs, Ws)))
    y1 = torch.randint(0, Hs - th + 1, (B,), generator=g).numpy() if th < Hs else np.zeros(B, dtype=np.int64)
    x1 = torch.randint(0, Ws - tw + 1, (B,), generator=g).numpy() if tw < Ws else np.zeros(B, dtype=np.int64)
    flip = (torch.rand(B, generator=g) < 0.5).numpy() if _get(geometric_aug, 'hflip', False) else None
    scale_hw = _size(_get(geometric_aug, 'scale_size', None), 'scale_size') if _get(geometric_aug, 'scale', False) else None

    values = [float(_get(photometric_aug, k, 0)) for k in OPS]
    if min(values) < 0 or values[3] > 0.5:
        raise ValueError('brightness, contrast and saturation must be >= 0 and hue in [0, 0.5] (got %r)' % (values,))
    order = active = factors = gamma = perm = None
    if any(values):
        order = torch.rand(B, 4, generator=g).argsort(1).numpy()
        active = np.tile(np.array([v != 0 for v in values]), (B, 1))
        factors = np.ones((B, 4), dtype=np.float32)
        for op, v in enumerate(values):
            if v != 0:
                factors[:, op] = _uniform(g, B, -v, v) if op == 3 else _uniform(g, B, max(0.0, 1.0 - v), 1.0 + v)
    if _get(photometric_aug, 'gamma', 0) > 0:
        gamma = _uniform(g, B, *GAMMA_RANGE)
    swap = bool(_get(photometric_aug, 'swap_channels', False))
    if swap:
        perm = torch.rand(B, 3, generator=g).argsort(1).numpy()
    p = make_params((Hs, Ws), (th, tw), y1, x1, flip, order, active, factors, gamma, perm, scale_hw)
    p.photometric = bool(any(values)) or gamma is not None or swap
    return p


def _frames(src):
    """src as [B,F,3,Hs,Ws] contiguous -> (src, B, F, Hs, Ws, dtype code)."""
    if not isinstance(src, torch.Tensor):
        raise ValueError('src must be a tensor (got %s)' % type(src).__name__)
    if not src.is_cuda:
        raise _lib.ArflowHipError('arflow_amd.augment runs on the GPU only (src is a %s tensor); there is no CPU fallback'
                                  % src.device)
    if src.dtype not in (torch.uint8, torch.float32):
        raise ValueError('src must be uint8 or float32 (got %s)' % src.dtype)
    if src.dim() == 4 and src.shape[1] % 3 == 0:
        src = src.reshape(src.shape[0], src.shape[1] // 3, 3, src.shape[2], src.shape[3])
    if src.dim() != 5 or src.shape[2] != 3 or min(src.shape) < 1 or src.shape[1] > MAX_FRAMES:
        raise ValueError('src must be a non-empty [B,F,3,Hs,Ws] (or [B,3F,Hs,Ws]) tensor with F <= %d (got %s)'
                         % (MAX_FRAMES, tuple(src.shape)))
    B, F, _, Hs, Ws = (int(v) for v in src.shape)
    return src.contiguous(), B, F, Hs, Ws, (0 if src.dtype == torch.uint8 else 1)


def augment_batch(src, params, out_hw=None):
    """-> (img, img_ph), float32 [B,3F,h,w], on the current stream.  (h, w) is out_hw when given (a size other than the crop
    window's resizes bilinearly, align_corners=False), else the params' scale size, else the crop window.  img_ph is img when
    no photometric operation is configured."""
    src, B, F, Hs, Ws, dtype = _frames(src)
    if not isinstance(params, AugmentParams):
        raise ValueError('params must be an AugmentParams (draw_params makes one)')
    if params.B != B or params.src_hw != (Hs, Ws):
        raise ValueError('params were drawn for %d samples of %r, src is %s' % (params.B, params.src_hw, tuple(src.shape)))
    th, tw = params.crop_hw
    # the windows live on the device: their bounds are checked here, on the host copy
    t = params.table
    if int(t[:, Y1].min()) < 0 or int(t[:, Y1].max()) > Hs - th or int(t[:, X1].min()) < 0 or int(t[:, X1].max()) > Ws - tw:
        raise ValueError('a crop window %r leaves the source %r' % ((th, tw), (Hs, Ws)))
    if out_hw is not None:
        h, w = _size(out_hw, 'out_hw')
        scale = (h, w) != (th, tw)
    else:
        (h, w), scale = params.out_hw, params.scale_hw is not None
    img = torch.empty(B, 3 * F, h, w, device=src.device, dtype=torch.float32)
    img_ph = torch.empty_like(img) if params.photometric else None
    lib = _lib.load()
    with torch.cuda.device_of(src):
        tab = params.device_table(src.device)
        shape = (B, F, Hs, Ws, th, tw, h, w, int(scale))
        work = None
        if img_ph is not None and bool(params.active('contrast').any()):
            parts = lib.arflow_augment_partials(h, w)
            _lib.check(min(parts, 0), 'arflow_augment_partials')
            work = torch.empty(B * F * parts, device=src.device, dtype=torch.float64)
            _call('arflow_augment_stats', _p(src), dtype, _p(tab), _p(work), *shape, _stream(), key=shape + (dtype, 'stats'))
        _call('arflow_augment_apply', _p(src), dtype, _p(tab), _p(work), _p(img), _p(img_ph), *shape, _stream(),
              key=shape + (dtype, 'apply'))
    return img, (img if img_ph is None else img_ph)


class BatchAugment:
    """What a training loop holds: ``img, img_ph = aug(batch_uint8)``; the loss takes img, the model img_ph
    (TrainStep(img, img_pair_ph=img_ph)).  One seeded CPU generator draws every batch's table; last_params is the table of
    the last call (crop origins, flips, ...), for a caller that crops its own targets."""

    def __init__(self, geometric_aug=None, photometric_aug=None, seed=0):
        self.geometric_aug, self.photometric_aug = geometric_aug, photometric_aug
        self.generator = torch.Generator(device='cpu').manual_seed(int(seed))
        self.last_params = None

    def __call__(self, src):
        src, B, F, Hs, Ws, _ = _frames(src)
        self.last_params = draw_params(self.geometric_aug, self.photometric_aug, B, (Hs, Ws), self.generator)
        return augment_batch(src, self.last_params)


def valid_transform(test_shape):
    """datasets/get_dataset.py:26: Scale(test_shape) alone -> a callable, uint8 or float32 batch -> float32 [B,3F,h,w]."""
    aug = BatchAugment(geometric_aug=dict(scale=True, scale_size=_size(test_shape, 'test_shape')))
    return lambda src: aug(src)[0]
