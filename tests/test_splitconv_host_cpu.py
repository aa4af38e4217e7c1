"""CPU: the host helpers the split-bf16 convolution family shares in arflow_amd/functional.py.  `_workspace` turns a negative
answer of a size query into an error before anything is allocated, at each of its call sites; `_size_floor` is the one floor
of the three routing rules, checked on either side of every floor they use."""
import pytest
import torch

ESHAPE = -1002


def _stub(monkeypatch, answer):
    """A library whose every entry answers `answer`; records (name, args)."""
    from arflow_amd import _lib, functional as AF
    asked = []

    class Lib:
        def __getattr__(self, name):
            if name == 'arflow_strerror':
                return lambda code: b'stub'
            return lambda *a: (asked.append((name, a)), answer)[1]
    monkeypatch.setattr(_lib, 'load', lambda: Lib())
    monkeypatch.setattr(AF, '_need_gpu', lambda *a: None)
    return asked


def _sites(AF):
    x, gy, w, w_head = torch.zeros(2, 5, 4, 6), torch.zeros(2, 3, 4, 6), torch.zeros(3, 5, 3, 3), torch.zeros(2, 5, 3, 3)
    return {
        'arflow_splitconv_pack_bytes': lambda: AF.splitconv(x, w),
        'arflow_splitconv_wgrad_ws_bytes': lambda: AF.splitconv_wgrad(x, gy),
        'arflow_headconv_bwd_weight_ws_bytes': lambda: AF._headconv_wgrad(x, gy[:, :2].contiguous(), w_head, True, True),
        'arflow_area_pyramid_ws_bytes': lambda: AF.area_pyramid(x, [(2, 3), (4, 6)]),
    }


QUERIES = ['arflow_headconv_bwd_weight_ws_bytes', 'arflow_splitconv_pack_bytes', 'arflow_splitconv_wgrad_ws_bytes',
           'arflow_area_pyramid_ws_bytes']


@pytest.mark.parametrize('name', QUERIES)
def test_workspace_raises_before_allocating(monkeypatch, name):
    from arflow_amd import _lib, functional as AF
    asked = _stub(monkeypatch, ESHAPE)
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: pytest.fail('torch.empty reached with a negative size'))
    with pytest.raises(_lib.ArflowHipError, match=name):
        AF._workspace(name, 1, 2, 3, device='cpu')
    assert asked == [(name, (1, 2, 3))]


@pytest.mark.parametrize('name', QUERIES)
def test_call_site_raises_before_allocating(monkeypatch, name):
    """The wrapper that asks `name` allocates nothing -- neither the workspace nor its outputs -- once the answer is negative.
    (Both head-conv backwards ask through _headconv_wgrad.)"""
    from arflow_amd import _lib, functional as AF
    site = _sites(AF)[name]  # the inputs are made before torch.empty is taken away
    asked = _stub(monkeypatch, ESHAPE)
    for alloc in ('empty', 'empty_like', 'zeros'):
        monkeypatch.setattr(torch, alloc, lambda *a, **k: pytest.fail('an allocation was reached with a negative size'))
    with pytest.raises(_lib.ArflowHipError, match=name):
        site()
    assert [n for n, _ in asked] == [name]


def test_workspace_is_a_byte_buffer_of_the_answered_size(monkeypatch):
    from arflow_amd import functional as AF
    _stub(monkeypatch, 24)
    ws = AF._workspace('arflow_splitconv_pack_bytes', 3, 5, device='cpu')
    assert ws.dtype == torch.uint8 and tuple(ws.shape) == (24,)
    _stub(monkeypatch, 0)
    assert AF._workspace('arflow_area_pyramid_ws_bytes', device='cpu').view(torch.float32).numel() == 0


def test_size_floor():
    from arflow_amd.functional import _size_floor
    for h, w in ((96, 160), (48, 80)):
        assert _size_floor(16, h, w, h, w) and _size_floor(17, h, w + 1, h, w)
        assert not _size_floor(15, h, w, h, w)          # maps large enough, too few of them
        assert not _size_floor(16, h, w - 1, h, w)
        assert not _size_floor(64, h // 2, w, h, w)     # pixels enough in the batch, maps too small
        assert _size_floor(8, 2 * h, w, h, w) and not _size_floor(7, 2 * h, w, h, w)  # fewer, larger maps: the batch's pixels count


# (rule, C, K, floor): channels the rule takes at that floor and -- for _splitconv_rule's upper floor -- at no lower one
FLOORS = [('_splitconv_rule', 403, 96, (96, 160)), ('_splitconv_rule', 147, 128, (48, 80)),
          ('_splitconv_wgrad_rule', 563, 32, (96, 160)), ('_inplace_wgrad_rule', 275, 128, (96, 160))]


@pytest.mark.parametrize('rule, C, K, floor', FLOORS)
def test_rules_on_either_side_of_their_floor(rule, C, K, floor):
    from arflow_amd import functional as AF
    takes = getattr(AF, rule)
    h, w = floor
    assert takes(16, C, K, h, w) and takes(16, C, K, h, w + 1) and takes(17, C, K, h, w) and takes(8, C, K, 2 * h, w)
    assert not takes(15, C, K, h, w)
    assert not takes(16, C, K, h, w - 1)
    assert not takes(16, C, K, h - 1, w)
    assert not takes(64, C, K, h // 2, w)
    assert not takes(7, C, K, 2 * h, w)
