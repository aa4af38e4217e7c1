"""CPU: the host-side plumbing the variational families share (arflow_amd/_planes.py) -- the
plane-layout rule, the small-tensor check, the gradient normalisation and the save / load pair for tuples that may hold
None -- table-driven, on stand-in tensors that report is_cuda (the checks that follow the device check never touch memory)."""
import pytest
import torch

from arflow_amd import _lib, _planes as P

MOD = 'arflow_amd.somefamily'


class Fake(torch.Tensor):
    is_cuda = True


def fake(*shape, **kw):
    return torch.zeros(*shape, **kw).as_subclass(Fake)


# name, tensor, shape asked for, batch stride returned
ACCEPTED = [
    ('contiguous', lambda: fake(2, 6, 4, 5), (2, 6, 4, 5), 120),
    ('channel slice, front', lambda: fake(2, 8, 4, 5)[:, 0:2], (2, 2, 4, 5), 160),   # the parent's batch stride
    ('channel slice, back', lambda: fake(2, 8, 4, 5)[:, 2:], (2, 6, 4, 5), 160),
    ('channel slice, middle', lambda: fake(2, 11, 3, 5)[:, 1:5], (2, 4, 3, 5), 165),
    ('one item of a wider tensor', lambda: fake(3, 8, 4, 5)[1:2, 2:4], (1, 2, 4, 5), 40),  # n == 1: C M N whatever the stride
    ('one item, expanded from nothing', lambda: fake(1, 2, 4, 5).as_strided((1, 2, 4, 5), (7, 20, 5, 1)), (1, 2, 4, 5), 40),
    ('1x1 planes', lambda: fake(4, 7, 1, 1)[:, 1:], (4, 6, 1, 1), 7),
    ('one row of any row stride', lambda: fake(2, 1, 3, 5)[:, :, :1], (2, 1, 1, 5), 15),
    ('every other item', lambda: fake(4, 2, 4, 5)[::2], (2, 2, 4, 5), 80),
]


@pytest.mark.parametrize('case', ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_check_planes_accepts_and_returns_the_batch_stride(case):
    _, make, shape, stride = case
    assert P.check_planes(MOD, 'std', make(), shape) == stride


# name, argument, tensor, shape asked for, exception, message
REJECTED = [
    ('column-strided view', 'std', lambda: fake(2, 6, 4, 10)[..., ::2], (2, 6, 4, 5), ValueError,
     'std must be contiguous or a channel slice of a contiguous tensor'),
    ('row-strided view', 'mean', lambda: fake(2, 2, 8, 5)[:, :, ::2], (2, 2, 4, 5), ValueError,
     'mean must be contiguous or a channel slice'),
    ('every other channel', 'std', lambda: fake(2, 8, 4, 5)[:, ::2], (2, 4, 4, 5), ValueError,
     'std must be contiguous or a channel slice'),
    ('expanded along the batch', 'gZ', lambda: fake(1, 2, 4, 5).expand(3, 2, 4, 5), (3, 2, 4, 5), ValueError,
     'gZ must be contiguous or a channel slice'),
    ('wrong dtype', 'log_std', lambda: fake(2, 4, 3, 5, dtype=torch.float64), (2, 4, 3, 5), ValueError,
     'log_std must be float32'),
    ('wrong shape', 'mean', lambda: fake(2, 2, 4, 6), (2, 2, 4, 5), ValueError, r'mean must be \(2, 2, 4, 5\) \(got \(2, 2, 4, 6\)\)'),
    ('wrong rank', 'eps', lambda: fake(2, 4, 5), (2, 1, 4, 5), ValueError, 'eps must be'),
    ('not a tensor', 'out', lambda: None, (2, 2, 4, 5), ValueError, r'out must be a tensor \(got NoneType\)'),
    ('CPU tensor', 'eps', lambda: torch.zeros(2, 2, 4, 5), (2, 2, 4, 5), _lib.ArflowHipError,
     r'arflow_amd\.somefamily runs on the GPU only \(eps is a cpu tensor\); there is no CPU fallback'),
]


@pytest.mark.parametrize('case', REJECTED, ids=[c[0] for c in REJECTED])
def test_check_planes_rejects_and_names_the_argument(case):
    _, name, make, shape, exc, match = case
    with pytest.raises(exc, match=match):
        P.check_planes(MOD, name, make(), shape)


def test_the_device_check_comes_before_dtype_and_shape():
    with pytest.raises(_lib.ArflowHipError, match='std is a cpu tensor'):
        P.check_planes(MOD, 'std', torch.zeros(3, dtype=torch.float64), (2, 2, 4, 5))
    with pytest.raises(_lib.ArflowHipError, match='weights is a cpu tensor'):
        P.check_small(MOD, 'weights', torch.zeros(3, dtype=torch.float64), (2, 2), torch.float32, fake(1))


def test_check_small():
    like = fake(1)
    w = fake(4, 3)[:, :2]
    got = P.check_small(MOD, 'weights', w, (4, 2), torch.float32, like)
    assert got.is_contiguous() and got.shape == (4, 2)
    dense = fake(2, 3, dtype=torch.int64)
    assert P.check_small(MOD, 'comp', dense, (2, 3), torch.int64, like) is dense  # nothing to copy
    for name, t, shape, dtype, exc, match in [
            ('comp', fake(2, 3, dtype=torch.int32), (2, 3), torch.int64, ValueError, 'comp must be torch.int64'),
            ('comp', fake(3, 2, dtype=torch.int64), (2, 3), torch.int64, ValueError, r'comp must be \(2, 3\)'),
            ('weights', fake(2, 3), (2, 2), torch.float32, ValueError, r'weights must be \(2, 2\) \(got \(2, 3\)\)'),
            ('glogpdf', [1.0], (1,), torch.float32, ValueError, r'glogpdf must be a tensor \(got list\)'),
            ('weights', torch.zeros(2, 2), (2, 2), torch.float32, _lib.ArflowHipError,
             r'arflow_amd\.somefamily runs on the GPU only \(weights is a cpu tensor\)'),
            ('resp', fake(2, 2, device='meta'), (2, 2), torch.float32, ValueError, 'resp is on meta, mean on cpu')]:
        with pytest.raises(exc, match=match):
            P.check_small(MOD, name, t, shape, dtype, like)


def test_plane_dense():
    shape = (3, 2, 4, 5)
    dense = fake(*shape)
    assert P.plane_dense(dense, shape) is dense
    sl = fake(3, 5, 4, 5)[:, 1:3]
    assert P.plane_dense(sl, shape) is sl                       # a channel slice is passed in place
    for g in (fake(1, 2, 4, 5).expand(*shape),                   # expanded along the batch (stride 0): what a sum sends
              fake(3, 2, 4, 1).expand(*shape),                   # expanded along a row
              fake(3, 2, 4, 10)[..., ::2],                       # column-strided
              fake(3, 4, 4, 5)[:, ::2]):                         # every other channel
        got = P.plane_dense(g, shape)
        assert got is not g and got.is_contiguous() and torch.equal(got, g)
        assert P.check_planes(MOD, 'gZ', got, shape) == 40
    one = fake(1, 2, 4, 5).as_strided((1, 2, 4, 5), (0, 20, 5, 1))
    assert P.plane_dense(one, (1, 2, 4, 5)) is one               # one item: its batch stride is never used


class _Node(torch.autograd.Function):
    """forward saves its tensor arguments (None allowed) plus two extra tensors; backward hands back what it loaded."""
    loaded = None

    @staticmethod
    def forward(ctx, n_extra, *t):
        extra = [torch.full((2,), 10.0 + i) for i in range(n_extra)]
        P.save_optional(ctx, t, extra)
        return sum(x.sum() for x in t if x is not None)

    @staticmethod
    def backward(ctx, g):
        _Node.loaded = P.load_optional(ctx)
        return (None,) + tuple(None if x is None else g * torch.ones_like(x) for x in _Node.loaded[0])


@pytest.mark.parametrize('none_at', [(), (0,), (1,), (2,), (0, 2), (0, 1)])
@pytest.mark.parametrize('n_extra', [0, 2])
def test_save_and_load_optional_round_trip(none_at, n_extra):
    full = [torch.full((3,), float(i + 1), requires_grad=True) for i in range(3)]
    t = [None if i in none_at else x for i, x in enumerate(full)]
    _Node.apply(n_extra, *t).backward()
    got, extra = _Node.loaded
    assert len(got) == 3
    for i, x in enumerate(got):
        if i in none_at:
            assert x is None
        else:
            assert torch.equal(x, full[i]) and torch.equal(full[i].grad, torch.ones(3))
    assert [float(e[0]) for e in extra] == [10.0 + i for i in range(n_extra)]


def test_the_family_modules_share_the_one_rule():
    """No module keeps a copy: each reaches check_planes under its own name (mse has always reported as gauss_pyr)."""
    from arflow_amd import gauss_pyr, lowrank, mixture, mse, triag_solve
    cpu = torch.zeros(2, 2, 4, 5)
    for fn, module in ((lowrank._check, 'arflow_amd.lowrank'), (mixture._check, 'arflow_amd.mixture'),
                       (gauss_pyr._check, 'arflow_amd.gauss_pyr'), (mse._check, 'arflow_amd.gauss_pyr'),
                       (triag_solve._check_band, 'arflow_amd.triag_solve')):
        assert fn.func is P.check_planes
        with pytest.raises(_lib.ArflowHipError, match=module.replace('.', r'\.') + ' runs on the GPU only'):
            fn('x', cpu, (2, 2, 4, 5))
    assert mixture._small.func is P.check_small
