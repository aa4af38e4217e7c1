"""CPU: the ground-truth flow metrics (csrc/flow_eval.hip, arflow_amd/metrics.py) -- the entry points are exported and
bound and validate their arguments before any launch; metrics_from_sums reproduces what the reference's evaluate_flow
returned for the fixture (tests/golden/flow_eval.npz, tools/make_flow_eval_golden.py); FlowMetrics accumulates batches of
unequal size correctly.  No GPU needed."""
import ctypes
import os

import pytest
import torch

from tests import flow_eval_ref as R

NEW = ['arflow_flow_eval_rows', 'arflow_flow_eval']
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


def _eval(lib, **kw):
    one = ctypes.c_void_p(16)
    a = dict(pred=one, gt=one, move=None, rows=one, emap=None, B=1, h=4, w=4, C=4, H=8, W=8)
    a.update(kw)
    return lib.arflow_flow_eval(a['pred'], a['gt'], a['move'], a['rows'], a['emap'], a['B'], a['h'], a['w'], a['C'], a['H'],
                                a['W'], None)


def test_flow_eval_argument_errors_without_gpu(lib):
    # validation happens before any launch, so these are safe on a CPU-only host
    one = ctypes.c_void_p(16)
    for k in ('pred', 'gt', 'rows'):
        assert _eval(lib, **{k: None}) == ENULL, k
    for k in ('B', 'h', 'w', 'H', 'W'):
        assert _eval(lib, **{k: 0}) == ESHAPE, k
        assert _eval(lib, **{k: -3}) == ESHAPE, k
    for C in (0, 1, 3, 5):
        assert _eval(lib, C=C) == EPARAM, C
    assert _eval(lib, C=2, move=one) == EPARAM      # moving masks need the sparse ground truth
    assert _eval(lib, pred=None, C=3, B=0) == ENULL  # pointers first, then shapes, then parameters
    assert _eval(lib, B=0, C=3) == ESHAPE
    assert lib.arflow_flow_eval_rows(0, 8) == ESHAPE and lib.arflow_flow_eval_rows(8, 0) == ESHAPE
    assert lib.arflow_flow_eval_rows(1, 1) == 1
    rows = lib.arflow_flow_eval_rows(436, 1024)
    assert rows >= 1 and lib.arflow_flow_eval_rows(437, 1024) >= rows


def test_flow_eval_refuses_cpu_and_non_fp32_tensors():
    from arflow_amd import functional as AF, _lib
    from arflow_amd.metrics import FlowMetrics
    pred, gt = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 8, 8)
    with pytest.raises(_lib.ArflowHipError):
        AF.flow_eval_sums(pred, gt)
    with pytest.raises(_lib.ArflowHipError):
        AF.flow_eval_sums(pred.double(), gt.double())
    with pytest.raises(_lib.ArflowHipError):
        FlowMetrics().update(pred, gt)


@pytest.fixture(scope='module')
def fixture_cases(golden):
    z = golden('flow_eval')
    cases = {}
    for tag in ('a', 'b'):
        gt = torch.cat([z['flow_' + tag], z['valid_' + tag].float(), z['noc_' + tag].float()], 1)
        pred, move = z['pred_' + tag], z['move_' + tag].float()
        cases[tag] = {'dense': (R.reference(pred, gt[:, :2]), z['ref_dense_' + tag]),
                      'sparse': (R.reference(pred, gt), z['ref_sparse_' + tag]),
                      'move': (R.reference(pred, gt, move), z['ref_move_' + tag])}
    return cases


@pytest.mark.parametrize('tag', ['a', 'b'])
@pytest.mark.parametrize('kind', ['dense', 'sparse', 'move'])
def test_metrics_from_sums_match_the_reference_fixture(fixture_cases, tag, kind):
    """The reference's returned list (batch means, float32 arithmetic) against metrics_from_sums of the float64
    restatement.  EPE-type values: rtol 2e-5 (the reference adds ~8e3 float32 terms pairwise, ~1e-6; the rest is margin).
    F1_all is a count behind two thresholds: it may differ by the pixels within TAU of one, 100 * band / sum valid."""
    from arflow_amd.metrics import metric_names, metrics_from_sums
    ref, want = fixture_cases[tag][kind]
    names = metric_names(kind != 'dense', kind == 'move')
    got = metrics_from_sums(ref['sums'], kind != 'dense', kind == 'move')
    assert got.shape == (ref['sums'].shape[0], len(names)) and got.dtype == torch.float64
    assert len(want) == len(names)
    mean = got.mean(0)
    for i, n in enumerate(names):
        if n == 'F1_all':
            band = float((100.0 * ref['band'] / ref['sums'][:, 1]).mean())
            assert band <= 0.5, 'the fixture has %.3f %% of its valid pixels on a threshold' % band
            tol = band
        else:
            tol = 2e-5 * abs(float(want[i]))
        print('%s %s %s: %.9g vs reference %.9g (tol %.3g)' % (tag, kind, n, float(mean[i]), float(want[i]), tol))
        assert abs(float(mean[i]) - float(want[i])) <= tol, (n, float(mean[i]), float(want[i]), tol)


def test_metrics_from_sums_edge_cases():
    from arflow_amd.metrics import metrics_from_sums
    # S0..S7 = sum epe*valid, sum valid, sum epe*noc, sum noc, sum bad, sum epe*valid*move, sum valid*move, 0
    s = torch.tensor([[30.0, 10.0, 12.0, 8.0, 2.0, 9.0, 3.0, 0.0],     # 2 occluded pixels
                      [30.0, 10.0, 30.0, 10.0, 0.0, 30.0, 10.0, 0.0],  # nothing occluded, everything moves
                      [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)  # no valid pixel
    m = metrics_from_sums(s, True, True)
    assert torch.allclose(m[0], torch.tensor([3.0, 1.5, 9.0, 20.0, 3.0, 3.0], dtype=torch.float64))
    # E_occ divides by max(sum(valid - noc), 1.0): 0 / 1; the static EPE of a sample where everything moves is 0 / 0
    assert float(m[1, 2]) == 0.0 and torch.isnan(m[1, 5]) and float(m[1, 4]) == 3.0
    assert torch.isnan(m[2, 0]) and torch.isnan(m[2, 1]) and torch.isnan(m[2, 3]) and float(m[2, 2]) == 0.0
    assert metrics_from_sums(s[:2], False).shape == (2, 1)
    # half an occluded pixel (soft masks): the reference's max(.., 1.0) keeps the denominator at 1
    assert float(metrics_from_sums(torch.tensor([[4.0, 2.5, 3.0, 2.0, 0, 0, 0, 0]], dtype=torch.float64), True)[0, 2]) == 1.0


def test_flow_metrics_accumulates_unequal_batches():
    """Three batches of 1, 4 and 2 samples equal one batch of all 7: the state is (metric totals, sample count)."""
    from arflow_amd.metrics import FlowMetrics, metrics_from_sums
    g = torch.Generator().manual_seed(3)
    s = torch.rand(7, 8, generator=g, dtype=torch.float64) * 50 + 1
    s[:, 0] += s[:, 2] + s[:, 5]  # keep the derived sums positive
    s[:, 1] += s[:, 3] + s[:, 6] + 2
    s[:, 7] = 0
    split, whole = FlowMetrics(), FlowMetrics()
    for part in (s[:1], s[1:5], s[5:]):
        split.update_from_sums(part, True, True)
    whole.update_from_sums(s, True, True)
    a, b = split.compute(), whole.compute()
    want = metrics_from_sums(s, True, True).mean(0)
    assert list(a) == ['EPE', 'E_noc', 'E_occ', 'F1_all', 'E_move', 'E_static'] == list(b)
    for i, n in enumerate(a):
        assert abs(a[n] - b[n]) <= 1e-12 * abs(b[n]) and abs(b[n] - float(want[i])) <= 1e-12 * abs(b[n]), n
    assert FlowMetrics().compute() == {}
    with pytest.raises(ValueError):
        split.update_from_sums(s[:1], False)  # a dense batch into a sparse meter
