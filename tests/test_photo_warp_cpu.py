"""CPU: the fused warp + mask + L1/SSIM entry points (csrc/photo_warp.hip) are exported and bound, validate their
arguments before any launch, and the Python layer answers / refuses as documented -- no GPU needed."""
import ctypes
import os

import pytest
import torch

NEW = ['arflow_photo_warp_rows', 'arflow_photo_warp_fwd', 'arflow_photo_warp_bwd', 'arflow_area_pyramid_ws_bytes',
       'arflow_area_pyramid']
ENULL, ESHAPE, EPARAM = -1001, -1002, -1003


@pytest.fixture(scope='module')
def lib():
    from arflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_new_symbols_are_exported_and_bound(lib):
    from arflow_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), '..', '..', 'include', 'arflow_hip.h')).read()
    for n in NEW:
        assert hasattr(raw, n), n
        assert n in _lib.PROTOTYPES, n
        assert n + '(' in header, n
    assert lib.arflow_abi_version() == 10  # additive change


def _fwd(lib, **kw):
    one = ctypes.c_void_p(16)
    a = dict(tgt=one, src=one, flow=one, mask=one, mode=0, inv=0, mh=8, mw=8, mout=None, rows=one, B=1, G=2, C=3, H=8, W=8,
             pad=1)
    a.update(kw)
    return lib.arflow_photo_warp_fwd(a['tgt'], 0, 0, a['src'], 0, 0, a['flow'], 0, 0, a['mask'], 0, 0, a['mode'], a['inv'],
                                     a['mh'], a['mw'], a['mout'], a['rows'], a['B'], a['G'], a['C'], a['H'], a['W'], a['pad'],
                                     None)


def _bwd(lib, **kw):
    one = ctypes.c_void_p(16)
    a = dict(tgt=one, src=one, flow=one, mask=one, mode=0, mh=8, mw=8, coef=one, g=one, B=1, G=2, C=3, H=8, W=8, pad=1)
    a.update(kw)
    return lib.arflow_photo_warp_bwd(a['tgt'], 0, 0, a['src'], 0, 0, a['flow'], 0, 0, a['mask'], 0, 0, a['mode'], 0, a['mh'],
                                     a['mw'], a['coef'], a['g'], 0, 0, a['B'], a['G'], a['C'], a['H'], a['W'], a['pad'], None)


def test_photo_warp_argument_errors_without_gpu(lib):
    # validation happens before any launch, so these are safe on a CPU-only host
    for k in ('tgt', 'src', 'flow', 'rows', 'mask'):
        assert _fwd(lib, **{k: None}) == ENULL, k
    for k in ('tgt', 'src', 'flow', 'coef', 'g', 'mask'):
        assert _bwd(lib, **{k: None}) == ENULL, k
    for f in (_fwd, _bwd):
        assert f(lib, H=2) == ESHAPE and f(lib, W=2) == ESHAPE and f(lib, B=0) == ESHAPE and f(lib, G=0) == ESHAPE
        assert f(lib, C=4) == EPARAM          # images have at most 3 channels
        assert f(lib, pad=2) == EPARAM
        assert f(lib, mode=3) == EPARAM
        assert f(lib, mode=1, mh=12, mw=16) == ESHAPE  # nearest resize: integer factors only
        assert f(lib, mode=1, mh=4, mw=8) == ESHAPE
    assert lib.arflow_photo_warp_rows(16, 384, 640) == 16 * 24 * 10
    assert lib.arflow_photo_warp_rows(2, 3, 3) == 2
    assert lib.arflow_photo_warp_rows(2, 2, 8) == ESHAPE and lib.arflow_photo_warp_rows(0, 8, 8) == ESHAPE


def _sizes(*pairs):
    arr = (ctypes.c_int * (2 * len(pairs)))(*[v for p in pairs for v in p])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_area_pyramid_argument_errors_and_sizes_without_gpu(lib):
    one = ctypes.c_void_p(16)
    keep, s = _sizes((384, 640), (96, 160), (48, 80), (6, 10))
    assert lib.arflow_area_pyramid_ws_bytes(48, 384, 640, s, 4) == 4 * 48 * (96 * 160 + 48 * 80 + 6 * 10)
    assert lib.arflow_area_pyramid_ws_bytes(48, 384, 640, s, 1) == 0  # factor 1 produces nothing
    assert lib.arflow_area_pyramid(one, None, 48, 384, 640, s, 1, None) == 0  # ... and launches nothing
    assert lib.arflow_area_pyramid(None, one, 48, 384, 640, s, 4, None) == ENULL
    assert lib.arflow_area_pyramid(one, None, 48, 384, 640, s, 4, None) == ENULL
    assert lib.arflow_area_pyramid(one, one, 48, 384, 640, None, 4, None) == ENULL
    assert lib.arflow_area_pyramid(one, one, 0, 384, 640, s, 4, None) == ESHAPE
    keep2, bad = _sizes((100, 160))
    assert lib.arflow_area_pyramid(one, one, 48, 384, 640, bad, 1, None) == ESHAPE  # 384 / 100 is no integer
    assert lib.arflow_area_pyramid_ws_bytes(48, 384, 640, bad, 1) == ESHAPE
    keep3, many = _sizes(*[(96, 160)] * 9)
    assert lib.arflow_area_pyramid(one, one, 48, 384, 640, many, 9, None) == EPARAM
    del keep, keep2, keep3


class _Fake:
    """Stands in for a GPU tensor: photo_warp_supported() only looks at shape, device and dtype."""

    def __init__(self, shape, cuda=True, dtype=torch.float32):
        self.shape, self.is_cuda, self.dtype = torch.Size(shape), cuda, dtype


def test_photo_warp_supported_answers():
    from arflow_amd import functional as AF
    fr = _Fake((8, 6, 384, 640))
    for h, w in ((384, 640), (96, 160), (48, 80), (24, 40), (12, 20), (6, 10), (3, 5)):
        assert AF.photo_warp_supported(fr, _Fake((8, 4, h, w)), (384, 640)), (h, w)
    assert not AF.photo_warp_supported(fr, _Fake((8, 4, 100, 160)))       # non-integer area factor
    assert not AF.photo_warp_supported(fr, _Fake((8, 4, 96, 320)))        # H0 / h != W0 / w
    assert not AF.photo_warp_supported(_Fake((8, 6, 8, 640)), _Fake((8, 4, 2, 160)))   # h < 3
    assert not AF.photo_warp_supported(_Fake((8, 6, 384, 8)), _Fake((8, 4, 96, 2)))   # w < 3
    assert not AF.photo_warp_supported(fr, _Fake((8, 4, 96, 160)), (100, 160))         # mask: non-integer factor
    assert not AF.photo_warp_supported(_Fake((8, 6, 384, 640), cuda=False), _Fake((8, 4, 96, 160), cuda=False))
    assert not AF.photo_warp_supported(_Fake((8, 6, 384, 640), dtype=torch.float16), _Fake((8, 4, 96, 160)))
    assert not AF.photo_warp_supported(fr, _Fake((8, 4, 96, 160), dtype=torch.bfloat16))
    assert not AF.photo_warp_supported(torch.zeros(1, 6, 8, 8), torch.zeros(1, 4, 8, 8))


def test_new_ops_refuse_cpu_tensors_loudly():
    from arflow_amd import functional as AF, _lib
    im, flow = torch.zeros(2, 6, 8, 8), torch.zeros(2, 4, 8, 8)
    with pytest.raises(_lib.ArflowHipError):
        AF.photo_warp_sums((im[:, :3], im[:, 3:]), (im[:, 3:], im[:, :3]), flow, mask_mode='border')
    with pytest.raises(_lib.ArflowHipError):
        AF.area_pyramid(im, [(4, 4)])


def test_losses_keep_their_cpu_behaviour():
    """The fused path is for CUDA tensors only: on the CPU unFlowLoss still refuses through the op layer, and the
    w_ternary > 0 error of the reference survives."""
    from arflow_amd import _lib
    from arflow_amd.config import AttrDict
    from arflow_amd.losses import unFlowLoss
    cfg = AttrDict(w_l1=0.15, w_ssim=0.85, w_ternary=0.0, warp_pad='border', alpha=10, occ_from_back=True, with_bk=True,
                   w_smooth=75.0, w_scales=[1.0], w_sm_scales=[1.0])
    with pytest.raises(_lib.ArflowHipError):
        unFlowLoss(cfg)([torch.zeros(1, 4, 8, 8)], torch.zeros(1, 6, 8, 8))
