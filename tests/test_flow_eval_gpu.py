"""GPU: arflow_flow_eval (csrc/flow_eval.hip) against the float64 restatement of tests/flow_eval_ref.py at the smallest
shapes that reach each path, and FlowMetrics / validate / the evaluate CLI on top of it.

Bounds (derived, not measured).  epe: atol = 32 * 2^-24 * A with A = max(|gt|, |scaled pred|) of the case -- two roundings
in the scaling, about six in the blend and three in the norm give <= ~11 * 2^-24 * A, the norm is 1-Lipschitz; the EPE-type
ratios are means of such errors.  The F1 count: kernel and restatement may disagree only on valid pixels whose epe lies
within TAU = 1e-3 of a threshold (TAU is >= 8 x the epe bound for A <= 64), so |sum bad - reference| <= |band|, after
asserting ON THE REFERENCE that the band holds <= 0.5 % of the valid pixels (a condition on the inputs)."""
import json

import numpy as np
import pytest
import torch

from tests import flow_eval_ref as R

pytestmark = pytest.mark.gpu

# name: (B, h, w, H, W, C, with_move)
CASES = {
    'same_c2': (2, 37, 53, 37, 53, 2, False),      # ratio 1, W % 4 != 0 (scalar path), partial tiles
    'same_c4': (2, 37, 53, 37, 53, 4, False),
    'up_move': (3, 20, 33, 61, 130, 4, True),      # non-integer ratio, scalar path, per-sample row partition
    'x4_c2': (2, 24, 80, 96, 320, 2, False),       # x4, float4 path, several tile rows and columns
    'x4_c4': (2, 24, 80, 96, 320, 4, False),
    'down': (1, 64, 96, 40, 52, 4, False),         # prediction larger than the ground truth
    'one': (1, 1, 1, 5, 7, 2, False),              # degenerate taps
}


def _inputs(name):
    B, h, w, H, W, C, with_move = CASES[name]
    pred, gt, move = R.make_case(B, h, w, H, W)
    return pred, gt[:, :C].contiguous(), (move if with_move else None)


def _launch(pred, gt, move):
    """The raw entry point with a NaN-filled row buffer -> (rows [B,n,8], epe_map [B,1,H,W])."""
    from arflow_amd import _lib, functional as AF
    B, C, H, W = gt.shape
    n = _lib.load().arflow_flow_eval_rows(H, W)
    rows = torch.full((B, n, 8), float('nan'), device='cuda', dtype=torch.float64)
    emap = torch.full((B, 1, H, W), float('nan'), device='cuda')
    AF._call('arflow_flow_eval', AF._p(pred), AF._p(gt), AF._p(move), AF._p(rows), AF._p(emap), B, pred.shape[2],
             pred.shape[3], C, H, W, AF._stream())
    return rows, emap


@pytest.fixture(scope='module')
def results():
    """Reference and kernel output of every case, computed once."""
    out = {}
    for name in CASES:
        pred, gt, move = _inputs(name)
        ref = R.reference(pred, gt, move)
        dev = [None if t is None else t.cuda() for t in (pred, gt, move)]
        rows, emap = _launch(*dev)
        out[name] = {'ref': ref, 'dev': dev, 'rows': rows.cpu(), 'epe': emap.cpu()[:, 0].double(),
                     'atol': 32 * 2.0 ** -24 * ref['A']}
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_inputs_keep_the_threshold_band_small(results, name):
    ref = results[name]['ref']
    assert ref['A'] <= 64.0, ref['A']
    share = ref['band'] / ref['sums'][:, 1]
    print(name, 'A %.2f band share %s' % (ref['A'], share.tolist()))
    assert bool((share <= 0.005).all()), share


@pytest.mark.parametrize('name', list(CASES))
def test_epe_map_matches_float64(results, name):
    r = results[name]
    err = float((r['epe'] - r['ref']['epe']).abs().max())
    print(name, 'epe_map max err %.3e, atol %.3e' % (err, r['atol']))
    assert not torch.isnan(r['epe']).any()
    assert err <= r['atol']


@pytest.mark.parametrize('name', list(CASES))
def test_rows_are_all_written_and_sums_match(results, name):
    r = results[name]
    rows, want, atol = r['rows'], r['ref']['sums'], r['atol']
    assert not torch.isnan(rows).any(), 'a row of the buffer was not written'
    got = rows.sum(1)
    assert torch.equal(got[:, 7], torch.zeros_like(got[:, 7]))
    for k in (1, 3, 6):  # mask sums are exact
        assert torch.equal(got[:, k], want[:, k]), (k, got[:, k], want[:, k])
    pairs = {'valid': (got[:, 0], want[:, 0], want[:, 1]), 'noc': (got[:, 2], want[:, 2], want[:, 3]),
             'occ': (got[:, 0] - got[:, 2], want[:, 0] - want[:, 2], want[:, 1] - want[:, 3]),
             'move': (got[:, 5], want[:, 5], want[:, 6]),
             'static': (got[:, 0] - got[:, 5], want[:, 0] - want[:, 5], want[:, 1] - want[:, 6])}
    for what, (a, b, den) in pairs.items():
        ok = den > 0
        if not bool(ok.any()):
            assert torch.equal(a, b), what  # an empty mask sums to exactly 0 on both sides
            continue
        err = float(((a - b)[ok] / den[ok]).abs().max())
        print(name, what, 'mean-epe err %.3e, atol %.3e' % (err, atol))
        assert err <= atol, what
    diff = (got[:, 4] - want[:, 4]).abs()
    print(name, 'bad', got[:, 4].tolist(), 'reference', want[:, 4].tolist(), 'band', r['ref']['band'].tolist())
    assert bool((diff <= r['ref']['band']).all())


@pytest.mark.parametrize('name', ['up_move', 'x4_c4'])
def test_two_calls_are_bitwise_equal_in_either_mode(results, name):
    from arflow_amd import functional as AF
    dev = results[name]['dev']
    first = None
    for on in (False, True):
        with AF.deterministic(on):
            for _ in range(2):
                rows, emap = _launch(*dev)
                if first is None:
                    first = (rows, emap)
                assert torch.equal(rows, first[0]) and torch.equal(emap, first[1])
    assert torch.equal(first[0].cpu(), results[name]['rows'])


def test_functional_wrapper_folds_the_rows(results):
    from arflow_amd import functional as AF
    r = results['up_move']
    sums, emap = AF.flow_eval_sums(*r['dev'], want_map=True)
    assert sums.shape == (3, 8) and sums.dtype == torch.float64 and sums.is_cuda
    assert torch.equal(sums.cpu(), r['rows'].sum(1)) and torch.equal(emap.cpu()[:, 0].double(), r['epe'])
    assert torch.equal(AF.flow_eval_sums(*r['dev']), sums)
    # an unaligned ground truth takes the scalar path to the same sums, bit for bit
    x4 = results['x4_c4']
    pad = torch.zeros(x4['dev'][1].numel() + 1, device='cuda')
    pad[1:] = x4['dev'][1].flatten()
    off = pad[1:].view_as(x4['dev'][1])  # same values, base 4 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 != 0
    assert torch.equal(AF.flow_eval_sums(x4['dev'][0], off).cpu(), x4['rows'].sum(1))


def _model_and_batches():
    from arflow_amd.inference import build_model
    model = build_model('pwclite', 2, None, seed=0).cuda()
    g = torch.Generator().manual_seed(5)
    batches = []
    for B in (2, 1):
        _, gt, move = R.make_case(B, 64, 64, 80, 100, seed=20 + B)
        batches.append((torch.rand(B, 6, 64, 64, generator=g).cuda(), gt.cuda(), move.cuda()))
    return model, batches


class _Recording(torch.nn.Module):
    """The model, keeping a copy of every flow it hands out: two forward passes of one model need not agree bit for bit
    (the convolution library may pick another algorithm), so the restatement is applied to what validate() scored."""

    def __init__(self, model):
        super().__init__()
        self.model, self.flows = model, []

    def forward(self, x):
        res = self.model(x)
        self.flows.append(res['flows_fw'][0].clone())
        return res


def test_flow_metrics_and_validate_on_a_seeded_model():
    from arflow_amd.metrics import FlowMetrics, metric_names, metrics_from_sums, validate
    model, batches = _model_and_batches()
    model = _Recording(model)
    model.train()
    got = validate(model, batches)
    assert model.training and model.model.training, 'validate() must restore training mode'
    assert len(model.flows) == len(batches)
    model.eval()
    assert validate(model, batches[:1]) and not model.training
    # the restatement on the model's own output
    per_sample, tol, meter = [], [], FlowMetrics()
    for flow, (img, gt, move) in zip(model.flows, batches):
        assert flow.shape[2:] == (64, 64) and not flow.requires_grad
        meter.update(flow, gt, move)
        ref = R.reference(flow.cpu(), gt.cpu(), move.cpu())
        assert ref['A'] <= 64.0 and bool((ref['band'] <= 0.005 * ref['sums'][:, 1]).all())
        per_sample.append(metrics_from_sums(ref['sums'], True, True))
        atol = 32 * 2.0 ** -24 * ref['A']
        t = torch.full_like(per_sample[-1], atol)
        t[:, 3] = 100.0 * ref['band'] / ref['sums'][:, 1]
        tol.append(t)
    want, tol = torch.cat(per_sample).mean(0), torch.cat(tol).mean(0)
    names = metric_names(True, True)
    same = meter.compute()
    assert list(got) == list(names) == list(same)
    for i, n in enumerate(names):
        print(n, got[n], same[n], float(want[i]), float(tol[i]))
        assert abs(got[n] - float(want[i])) <= float(tol[i]), n
        assert got[n] == same[n], n


def test_evaluate_cli_matches_flow_io_epe(tmp_path, capsys):
    from arflow_amd import evaluate, flow_io
    pred, gt, _ = R.make_case(1, 37, 53, 37, 53)
    a, b = pred[0].permute(1, 2, 0).numpy(), gt[0, :2].permute(1, 2, 0).numpy()
    flow_io.write_flow(str(tmp_path / 'pred.flo'), a)
    flow_io.write_flow(str(tmp_path / 'gt.flo'), b)
    out = evaluate.main(['--pred', str(tmp_path / 'pred.flo'), '--gt', str(tmp_path / 'gt.flo')])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = flow_io.epe(a, b)
    assert line == out and list(out) == ['EPE', 'pairs'] and out['pairs'] == 1
    assert abs(out['EPE'] - want) <= 1e-5 * want
    # two directories matched by file name
    for d in ('p', 'g'):
        (tmp_path / d).mkdir()
    for i in range(2):
        flow_io.write_flow(str(tmp_path / 'p' / ('%d.flo' % i)), a + i)
        flow_io.write_flow(str(tmp_path / 'g' / ('%d.flo' % i)), b)
    out = evaluate.main(['--pred', str(tmp_path / 'p'), '--gt', str(tmp_path / 'g')])
    want = np.mean([flow_io.epe(a + i, b) for i in range(2)])
    assert out['pairs'] == 2 and abs(out['EPE'] - want) <= 1e-5 * want
