"""CPU: the float64 restatement of the batch augmentation (tests/augment_ref.py) at anchors that are exact, against the
reference's own geometric transforms where a checkout is at hand (ARFLOW_REFERENCE), draw_params, the argument checks of the
raw entry points of csrc/augment.hip and the Python layer's wiring.  DESIGN.md section 36."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

from arflow_amd import augment as A
from tests import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-13  # the anchors are exact in float64 up to a few roundings of numbers in [0, 6]


def _pixels(cols):
    """[n] colours -> V [1,1,3,1,n] float64."""
    return R.V((torch.tensor(cols, dtype=torch.float64) / 255).t().reshape(1, 1, 3, 1, -1).contiguous())


def _f(v):
    return torch.tensor([v], dtype=torch.float64).reshape(1, 1, 1, 1, 1)


CHROMATIC = [c for c in R.COLOURS if max(c) != min(c)] + [(12, 200, 77), (250, 3, 128), (90, 91, 92)]


def test_hue_anchors():
    x = _pixels(CHROMATIC)
    assert (R.jitter(R.HUE, x, _f(0.0)).v - x.v).abs().max() <= TOL                      # 0: the identity
    up = R.jitter(R.HUE, x, _f(1.0 / 3.0)).v
    assert (up - x.v[:, :, [2, 0, 1]]).abs().max() <= TOL                                # +1/3: r <- b, g <- r, b <- g
    down = R.jitter(R.HUE, x, _f(-1.0 / 3.0)).v
    assert (down - x.v[:, :, [1, 2, 0]]).abs().max() <= TOL                              # -1/3: the opposite rotation
    half = R.jitter(R.HUE, x, _f(0.5)).v
    want = x.v.max(2, keepdim=True).values + x.v.min(2, keepdim=True).values - x.v
    assert (half - want).abs().max() <= TOL                                              # 1/2: max + min - x
    grey = _pixels([(128, 128, 128), (0, 0, 0), (255, 255, 255), (7, 7, 7)])
    for f in (0.0, 0.21, -0.5, 0.5):
        assert torch.equal(R.jitter(R.HUE, grey, _f(f)).v, grey.v)                       # cr = 0 passes through


def test_saturation_contrast_brightness_anchors():
    g = torch.Generator().manual_seed(0)
    x = R.V(torch.rand(2, 2, 3, 5, 7, generator=g, dtype=torch.float64))
    gray = 0.2989 * x.v[:, :, 0] + 0.587 * x.v[:, :, 1] + 0.114 * x.v[:, :, 2]
    zero = torch.zeros(2, 1, 1, 1, 1, dtype=torch.float64)
    sat = R.jitter(R.SATURATION, x, zero).v
    assert (sat - gray.unsqueeze(2)).abs().max() <= TOL                                  # saturation 0: gray in all channels
    con = R.jitter(R.CONTRAST, x, zero).v
    assert (con - gray.mean((-1, -2), keepdim=True).unsqueeze(2)).abs().max() <= TOL      # contrast 0: the FRAME's mean grey
    assert (con[:, 0] - con[:, 1]).abs().min() > 1e-4                                    # ... per frame, not per sample
    assert torch.equal(R.jitter(R.BRIGHTNESS, x, zero + 1.0).v, x.v)
    assert float(R.jitter(R.BRIGHTNESS, x, zero + 3.0).v.max()) == 1.0                   # every operation ends in a clamp


def test_operation_order_matters():
    src = torch.tensor([[10, 200], [90, 255]], dtype=torch.uint8).reshape(1, 1, 1, 2, 2).expand(1, 1, 3, 2, 2).contiguous()
    fac = [[1.8, 0.5, 1.0, 0.0]]
    act = [[True, True, False, False]]
    a = R.augment(src, A.make_params((2, 2), (2, 2), [0], [0], order=[[0, 1, 2, 3]], active=act, factors=fac))[1]
    b = R.augment(src, A.make_params((2, 2), (2, 2), [0], [0], order=[[1, 0, 2, 3]], active=act, factors=fac))[1]
    assert (a - b).abs().max() > 1e-2   # brightness then contrast clamps 200 * 1.8 first; the other way round it does not


def test_inactive_operations_are_skipped_and_gamma_perm_follow_their_definitions():
    src, p = R.frames_case(2)
    img, ph, _, _ = R.augment(src, p)
    x = img.reshape(6, 2, 3, 7, 10)
    want = (x * p.factors[:, 0].double().reshape(6, 1, 1, 1, 1)).clamp(0, 1)
    want = torch.pow(want, p.gamma.double().reshape(6, 1, 1, 1, 1)).clamp(0, 1)           # adjust_gamma: pow, clamp
    want = torch.stack([want[b][:, p.perm[b]] for b in range(6)])                        # image[..., ind, :, :]
    assert torch.equal(ph, want.reshape(6, 6, 7, 10))
    assert float(p.factors[:, 1:].sub(1).abs().max()) == 0 and not p.active('hue').any()


def test_bounds_of_the_gpu_cases_stay_under_the_cap():
    """What the GPU tests hold the kernels to is derived from the inputs alone; it may not exceed 1e-5."""
    cases = [R.orders_case((7, 10)), R.orders_case((8, 12)), R.frames_case(1), R.frames_case(3), R.contrast_case(),
             R.scale_case((13, 22), (13, 22), (16, 24)), R.scale_case((13, 22), (13, 22), (9, 10)),
             R.scale_case((16, 24), (16, 24), (16, 24)), R.scale_case((13, 22), (7, 10), (16, 24))]
    for src, p in cases:
        _, ph, e, eph = R.augment(src, p, track=True)
        assert torch.isfinite(eph).all() and 0 < float(eph.max()) <= R.BOUND_CAP and float(e.max()) <= 1e-6
        got = R.augment(src, p, dtype=torch.float32)[1].double()
        if p.scale_hw is None:  # the same formulas in ATen's fp32 (ATen's resize forms its coordinates otherwise)
            assert ((got - ph).abs() <= eph).all()


def test_tracked_resize_is_atens():
    src, p = R.scale_case((13, 22), (7, 10), (16, 24))
    for out_hw in ((16, 24), (9, 10), (7, 10), (5, 3)):
        a = R.geometric(src, p, out_hw, track=True).v
        b = R.geometric(src, p, out_hw).v
        assert a.shape == b.shape and (a - b).abs().max() <= 1e-14


# ---- against the reference's own classes ---------------------------------------------------------------------------------
def _reference_module():
    root = os.environ.get('ARFLOW_REFERENCE')
    path = os.path.join(root, 'transforms', 'geometric_transforms.py') if root else None
    if not path or not os.path.exists(path):
        pytest.skip('no checkout of the reference (ARFLOW_REFERENCE)')
    spec = importlib.util.spec_from_file_location('_ref_geometric_transforms', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Drawn:
    """Stands in for `random` inside the reference's module: hands out the values of one table row."""

    def __init__(self, x1, y1, flip):
        self.ints, self.flip = [x1, y1], flip       # RandomCrop draws x1, then y1

    def randint(self, lo, hi):
        v = self.ints.pop(0)
        assert lo <= v <= hi
        return v

    def random(self):
        return 0.25 if self.flip else 0.75


@pytest.mark.parametrize('scale_hw', [None, (16, 24), (5, 9)])
def test_geometric_stage_matches_the_reference_classes(scale_hw, monkeypatch):
    mod = _reference_module()
    src, p = R.orders_case((7, 10), scale_hw=scale_hw)
    got = R.augment(src, p, dtype=torch.float32)[0]
    for b in range(p.B):
        monkeypatch.setattr(mod, 'random', _Drawn(int(p.x1[b]), int(p.y1[b]), bool(p.flip[b])))
        x = src[b].float() / 255                                      # [F,3,H,W], what the dataset hands the transforms
        x = mod.RandomCrop(p.crop_hw)(x)
        x = mod.RandomHorizontalFlip()(x)
        if scale_hw is not None:
            x = mod.Scale(scale_hw)(x)
        x = x.reshape(-1, *x.shape[-2:])
        if scale_hw is None:
            assert torch.equal(got[b], x), b
        else:
            assert (got[b] - x).abs().max() <= 1e-6, b


# ---- draw_params ---------------------------------------------------------------------------------------------------------
GEO = dict(crop=True, crop_size=[7, 10], hflip=True)
PHO = dict(brightness=0.4, contrast=0.3, saturation=1.5, hue=0.5, gamma=1, swap_channels=True)


def test_draw_params_is_seeded():
    a = A.draw_params(GEO, PHO, 16, (13, 22), torch.Generator().manual_seed(5))
    b = A.draw_params(GEO, PHO, 16, (13, 22), torch.Generator().manual_seed(5))
    c = A.draw_params(GEO, PHO, 16, (13, 22), torch.Generator().manual_seed(6))
    assert torch.equal(a.table, b.table) and not torch.equal(a.table, c.table)
    assert a.table.dtype == torch.int32 and tuple(a.table.shape) == (16, 16) and a.photometric


def test_draw_params_ranges_over_many_draws():
    n = 10000
    p = A.draw_params(GEO, PHO, n, (13, 22), torch.Generator().manual_seed(0))
    assert 0 <= int(p.y1.min()) and int(p.y1.max()) == 13 - 7 and 0 <= int(p.x1.min()) and int(p.x1.max()) == 22 - 10
    assert int(p.y1.min()) == 0 and int(p.x1.min()) == 0
    assert 0.45 < float(p.flip.float().mean()) < 0.55
    f = p.factors.numpy()
    for op, (lo, hi) in enumerate([(0.6, 1.4), (0.7, 1.3), (0.0, 2.5), (-0.5, 0.5)]):
        assert np.float32(lo) <= f[:, op].min() and f[:, op].max() <= np.float32(hi), op
        assert f[:, op].min() < lo + 0.01 * (hi - lo) and f[:, op].max() > hi - 0.01 * (hi - lo), op   # the whole range is used
        assert p.active(op).all()
    gm = p.gamma.numpy()
    assert np.float32(0.7) <= gm.min() and gm.max() <= np.float32(1.5) and p.gamma_on.all()
    assert (np.sort(p.order.numpy(), 1) == np.arange(4)).all() and (np.sort(p.perm.numpy(), 1) == np.arange(3)).all()
    assert len({tuple(r) for r in p.order.tolist()}) == 24 and len({tuple(r) for r in p.perm.tolist()}) == 6


def test_draw_params_crop_edges_and_partial_configs():
    g = torch.Generator().manual_seed(1)
    p = A.draw_params(dict(crop=True, crop_size=[13, 10]), None, 500, (13, 22), g)        # th = Hs: y1 = 0 always
    assert not p.y1.any() and int(p.x1.max()) == 12 and not p.flip.any() and not p.photometric
    assert p.crop_hw == (13, 10) and p.out_hw == (13, 10)
    with pytest.raises(ValueError, match='crop_size'):
        A.draw_params(dict(crop=True, crop_size=[14, 10]), None, 2, (13, 22), g)
    p = A.draw_params(None, dict(hue=0.5), 500, (13, 22), g)                              # hue alone
    assert p.active('hue').all() and not (p.active('brightness') | p.active('contrast') | p.active('saturation')).any()
    assert len({tuple(r) for r in p.order.tolist()}) == 24 and p.photometric             # the order is still drawn
    assert p.crop_hw == (13, 22) and not p.gamma_on.any() and (p.perm == torch.arange(3)).all()
    p = A.draw_params(dict(scale=True, scale_size=[16, 24]), dict(gamma=0, swap_channels=False, hue=0), 3, (13, 22), g)
    assert p.out_hw == (16, 24) and not p.photometric
    p = A.draw_params({}, {}, 3, (13, 22), g)                                             # empty configs: nothing is on
    assert not p.photometric and p.out_hw == (13, 22) and not p.table[:, A.FLAGS].any()


def test_no_photometric_configuration_returns_one_tensor_twice():
    """img_ph is img: checked on the GPU in tests/test_augment_gpu.py; here that the decision is the parameters' alone."""
    assert 'img if img_ph is None else img_ph' in inspect.getsource(A.augment_batch)
    aug = A.BatchAugment()
    assert aug.last_params is None and aug.geometric_aug is None and aug.photometric_aug is None


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from arflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


NAMES = ('arflow_augment_stats', 'arflow_augment_apply', 'arflow_augment_partials')


def test_symbols_are_declared_exported_and_bound(lib):
    from arflow_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'arflow_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        m = re.search(r'\b%s\s*\(([^)]*)\)' % name, text)
        assert m, name
        assert hasattr(raw, name) and name in _lib.PROTOTYPES
        assert len([p for p in m.group(1).split(',') if p.strip()]) == len(_lib.PROTOTYPES[name]), name
    assert lib.arflow_abi_version() == 10 and _lib.ABI_VERSION == 10
    for k, v in dict(ROW=16, Y1=0, X1=1, FLAGS=2, ORDER=3, PERM=4, FACTOR=5, GAMMA=9, FLIP=1, GAMMA_ON=32, MAX_FRAMES=5).items():
        assert re.search(r'#define ARFLOW_AUG_%s %d\b' % (k, v), text) and getattr(A, k) == v, k
    assert A.active_bit(3) == 16 and '#define ARFLOW_AUG_ACTIVE(op) (2 << (op))' in text


def test_entry_points_check_their_arguments(lib):
    """Validation happens before any launch, so these are safe without a GPU."""
    ENULL, ESHAPE, EPARAM = -1001, -1002, -1003
    src, tab, work, img, ph = (ctypes.c_void_p(4096 * (i + 1) * 64) for i in range(5))
    good = dict(src=src, dtype=0, tab=tab, work=work, img=img, ph=ph, B=2, F=2, Hs=13, Ws=22, th=7, tw=10, h=7, w=10, scale=0)

    def tail(a):
        return (a['B'], a['F'], a['Hs'], a['Ws'], a['th'], a['tw'], a['h'], a['w'], a['scale'], None)

    def stats(**ch):
        a = dict(good, **ch)
        return lib.arflow_augment_stats(a['src'], a['dtype'], a['tab'], a['work'], *tail(a))

    def apply(**ch):
        a = dict(good, **ch)
        return lib.arflow_augment_apply(a['src'], a['dtype'], a['tab'], a['work'], a['img'], a['ph'], *tail(a))
    shared = [(dict(src=None), ENULL), (dict(tab=None), ENULL),
              (dict(B=0), ESHAPE), (dict(F=0), ESHAPE), (dict(F=6), ESHAPE), (dict(h=0, th=0), ESHAPE), (dict(w=0, tw=0), ESHAPE),
              (dict(B=40000), ESHAPE),                                  # B F > 65535
              (dict(th=14, h=14), ESHAPE), (dict(tw=23, w=23), ESHAPE),  # a crop window outside the source
              (dict(h=8), ESHAPE), (dict(w=12), ESHAPE),                # (h, w) != (th, tw) without scale
              (dict(dtype=2), EPARAM), (dict(dtype=-1), EPARAM), (dict(scale=2), EPARAM)]
    for change, want in shared:
        assert stats(**change) == want, ('stats', change)
        assert apply(**change) == want, ('apply', change)
    assert stats(work=None) == ENULL and apply(img=None) == ENULL
    for h, w in ((7, 10), (40, 70), (256, 448), (1, 1), (3, 2049), (640, 640)):
        assert lib.arflow_augment_partials(h, w) == -(-(h * -(-w // 4)) // 512), (h, w)
    assert lib.arflow_augment_partials(40, 70) == 2                      # the GPU test's frame spans more than one partial
    assert lib.arflow_augment_partials(0, 4) == ESHAPE and lib.arflow_augment_partials(4, -1) == ESHAPE
    assert lib.arflow_augment_partials(1 << 15, 1 << 15) == ESHAPE


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    from arflow_amd import _lib
    src, p = R.frames_case(2)
    with pytest.raises(_lib.ArflowHipError):
        A.augment_batch(src, p)
    with pytest.raises(_lib.ArflowHipError):
        A.BatchAugment(GEO, PHO)(src)
    with pytest.raises(_lib.ArflowHipError):
        A.valid_transform((16, 24))(src.float())


def test_make_params_round_trips_and_refuses_nonsense():
    src, p = R.orders_case((7, 10))
    assert len({tuple(r) for r in p.order.tolist()}) == 24 and p.active('contrast').all() and p.photometric
    assert p.flip.any() and not p.flip.all() and int(p.x1.max()) == 12 and (p.x1 % 2 == 1).any()
    assert int((~p.gamma_on).sum()) == 8 and float(p.gamma[p.gamma_on].min()) >= 1.0
    with pytest.raises(ValueError, match='order'):
        A.make_params((4, 4), (4, 4), [0], [0], order=[[0, 1, 1, 3]])
    with pytest.raises(ValueError, match='perm'):
        A.make_params((4, 4), (4, 4), [0], [0], perm=[[0, 0, 1]])


def test_train_step_takes_the_photometric_pair():
    from arflow_amd.train_step import TrainStep
    sig = inspect.signature(TrainStep.__call__)
    assert list(sig.parameters)[1:] == ['img_pair', 'target', 'img_pair_ph'] and sig.parameters['img_pair_ph'].default is None
