"""GPU: the models' native convolution stack -- split-bf16 forward / data gradient / weight gradient, the dense estimator's
node (fresh tensors and in place), the dilated chain on phase mosaics, the head convolution, the bias + LeakyReLU epilogue --
as the models compose it, against the float64 twins of tests/conv_stack_ref.py (magnitude M, fixtures without kink flips
and the any-order cap gamma(n) are defined there; tests/test_conv_stack_cpu.py holds the fixtures' sign margins).

a. blocks.FlowEstimatorDense with every routing rule forced, on three paths -- the composed ConvAct chain, the node into
   fresh tensors, the node in place -- at ch_in 19 (channel tails, K chunks of 2 + 1) and 147 (the flagship's), maps 9 x 35
   (crosses the 32-pixel and the 8-row tile) and 20 x 8 (the 8 x 4 tile), N = 2, slopes 0.1 and 1.0: x6, flow, dx, six dw, six db.
b. blocks.ContextNetwork with the dilated node forced, ARFLOW_DILATED_WGRAD unset and 1111, at ch_in 37 and 597, maps
   19 x 35 (H % d != 0, W % d != 0 for every d) and 16 x 33 (H == d at d = 16): out, dx and all fourteen parameter gradients.
   Criteria of a and b, per tensor:
     1. e <= gamma(n), the any-order cap;
     2. e <= 2 x the e of the vendor path (every switch off: MIOpen's convolutions, torch.cat) on the same inputs against the
        same twin, the larger of two runs -- tests/test_splitconv_gpu.py's criterion 1;
     3. two calls bitwise equal (the composed path under AF.deterministic(): its bias gradient, arflow_bias_act_bwd's, ends in
        fp32 atomics in the default mode);
   and for the node: the gradient of x alone, and the gradients with one weight frozen, torch.equal to the full call's.
c. PWCLiteUflow in the benchmark's configuration at 2 x 192 x 256 with the routing floor patched so that its four levels route
   as the benchmark's do (tests/test_conv_stack_cpu.py asserts the table): the launches seen by a spy on AF._call are the
   table's, and the flows are within 1e-3 px EPE of the CPU oracle twin at every level in both directions.  (Its parameter
   gradients are the `native` case of tests/test_models_gpu.py::test_model_parameter_gradients_elementwise.)
d. That model twice under AF.deterministic() (with MIOpen's deterministic solvers for the layers that stay the vendor's, the
   reproducible setting of DESIGN.md section 14): flows and every parameter gradient torch.equal.

Measured on the MI355X, e in u = 2^-24 as native / vendor (the node in place resp. all four chain weight gradients native, the
worst dw and db; the three dense paths agree bit for bit; profiles/conv_stack_errors_vs_float64.log has every tensor and path,
and the fixtures' sign margins):
  dense 19x2x9x35 slope 0.1: x6 0.867 / 1.06  flow 0.0533 / 0.108  dx 0.287 / 0.322  dw[4] 0.277 / 0.943  db[4] 0.156 / 0.156
  dense 19x2x9x35 slope 1: x6 0.925 / 1.09  flow 0.0642 / 0.196  dx 0.294 / 0.294  dw[4] 0.365 / 0.908  db[4] 0.213 / 0.213
  dense 19x2x20x8 slope 0.1: x6 0.867 / 1.04  flow 0.0281 / 0.081  dx 0.272 / 0.464  dw[4] 0.45 / 0.89  db[4] 0.232 / 0.232
  dense 19x2x20x8 slope 1: x6 0.873 / 1.21  flow 0.0954 / 0.2  dx 0.437 / 0.437  dw[4] 0.491 / 1.39  db[4] 0.425 / 0.425
  dense 147x2x9x35 slope 0.1: x6 0.673 / 1.13  flow 0.0701 / 0.0987  dx 1.05 / 0.958  dw[4] 0.389 / 1.16  db[4] 0.154 / 0.15
  dense 147x2x9x35 slope 1: x6 0.673 / 1.27  flow 0.0696 / 0.138  dx 0.985 / 1.05  dw[4] 0.43 / 1.54  db[3] 0.173 / 0.173
  dense 147x2x20x8 slope 0.1: x6 0.661 / 1.17  flow 0.0887 / 0.16  dx 1.09 / 1.09  dw[4] 0.544 / 1.59  db[3] 0.27 / 0.27
  dense 147x2x20x8 slope 1: x6 0.695 / 1.17  flow 0.0947 / 0.207  dx 1.01 / 0.993  dw[4] 0.577 / 1.68  db[4] 0.241 / 0.241
  context 37x2x19x35 slope 0.1: out 0.0163 / 0.0274  dx 4.81e-08 / 1.03e-07  dw[5] 0.00336 / 0.0119  db[5] 0.036 / 0.0576
  context 37x2x19x35 slope 1: out 0.0618 / 0.0915  dx 2.88e-07 / 1.16e-06  dw[5] 0.00785 / 0.0321  db[5] 0.0505 / 0.0511
  context 37x2x16x33 slope 0.1: out 0.013 / 0.0224  dx 5.02e-08 / 1.37e-07  dw[5] 0.00171 / 0.00382  db[5] 0.0351 / 0.05
  context 37x2x16x33 slope 1: out 0.0734 / 0.141  dx 3.21e-07 / 9.93e-07  dw[5] 0.00724 / 0.0214  db[5] 0.0394 / 0.0635
  context 597x2x19x35 slope 0.1: out 0.00728 / 0.0118  dx 4.93e-08 / 1.91e-07  dw[5] 0.0011 / 0.00321  db[5] 0.0271 / 0.0377
  context 597x2x19x35 slope 1: out 0.0422 / 0.0693  dx 4.01e-07 / 1.27e-06  dw[5] 0.00706 / 0.0178  db[5] 0.0308 / 0.0562
  context 597x2x16x33 slope 0.1: out 0.0122 / 0.026  dx 5.29e-08 / 2.36e-07  dw[5] 0.00205 / 0.00729  db[5] 0.0408 / 0.0445
  context 597x2x16x33 slope 1: out 0.055 / 0.0668  dx 3.88e-07 / 1.61e-06  dw[5] 0.00582 / 0.0224  db[5] 0.0341 / 0.121
  whole model on its native paths: flow EPE 1.08e-07 .. 6.40e-06 px over the six levels of both directions (gate 1e-3)
"""
import collections
import functools

import pytest
import torch

from tests import conv_stack_ref as R
from tests.test_conv_stack_cpu import (BENCH_LEVELS, CONTEXT_CASES, CONTEXT_KEYS, DENSE_CASES, DENSE_KEYS, ROUTING, ROUTING_CONTEXT,
                                       SLOPES, _flat, patch_floor_to_benchmark)

pytestmark = pytest.mark.gpu

SWITCHES = ('_SPLITCONV', '_SPLITCONV_WGRAD', '_HEADCONV', '_DENSE_BLOCK', '_DENSE_INPLACE', '_DILATED_CHAIN')
RULES = ('_splitconv_rule', '_splitconv_wgrad_rule', '_inplace_wgrad_rule')


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    return functional


def _force_rules(mp, AF):
    for name in RULES:
        mp.setattr(AF, name, lambda *a: True)
    mp.setattr(AF, 'dilated_chain_takes', lambda *a: True)


def _vendor(mp, AF):
    for name in SWITCHES:
        mp.setattr(AF, name, False)


def _name(case, slope):
    return '%s slope %g' % ('x'.join(map(str, case)), slope)


def _errors(got, ref, mag, keys):
    return collections.OrderedDict((name, R.rel_err(a, b, m))
                                   for (name, a), (_, b), (_, m) in zip(_flat(got, keys), _flat(ref, keys), _flat(mag, keys)))


def _assert_bitwise(r1, r2, keys, what):
    for (name, a), (_, b) in zip(_flat(r1, keys), _flat(r2, keys)):
        assert torch.equal(a, b), '%s: %s differs between two calls in %d elements' % (what, name, int((a != b).sum()))


def _check(what, e_native, e_vendor, counts, keys):
    caps = [R.gamma(n) for _, n in _flat(counts, keys)]
    print('%s (e native / vendor, u): %s' % (what, '  '.join('%s %.3g / %.3g' % (k, e_native[k] / R.U, e_vendor[k] / R.U) for k in e_native)))
    bad = ['%s: e = %.3f u above the cap %.3f u' % (k, e_native[k] / R.U, cap / R.U) for k, cap in zip(e_native, caps) if not e_native[k] <= cap]
    bad += ['%s: e = %.3f u, more than twice the vendor path\'s %.3f u' % (k, e_native[k] / R.U, e_vendor[k] / R.U)
            for k in e_native if not e_native[k] <= 2.0 * e_vendor[k]]
    assert not bad, '%s: %s' % (what, '; '.join(bad))


# ---- a. the dense estimator -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_ref(case, slope):
    f = R.dense_fixture(*case, slope)
    ref = R.dense_grads(f['x'], f['params'], slope, f['g_x6'], f['g_flow'])
    mag = R.dense_magnitudes(f['x'], f['params'], f['g_x6'], f['g_flow'])
    return f, ref, mag, R.dense_counts(*case)


def _dense_module(f, ch_in):
    from arflow_amd.models import blocks
    m = blocks.FlowEstimatorDense(ch_in)
    layers = (m.conv1, m.conv2, m.conv3, m.conv4, m.conv5, m.conv_last)
    with torch.no_grad():
        for k, layer in enumerate(layers):
            layer[0].weight.copy_(f['params'][2 * k])
            layer[0].bias.copy_(f['params'][2 * k + 1])
            if k < 5:
                layer[1].negative_slope = f['slope']
    return m.cuda(), [p for layer in layers for p in (layer[0].weight, layer[0].bias)]


def _dense_run(f, ch_in, frozen=(), x_only=False):
    """One forward and backward of the module under the switches in force: the tensors of DENSE_KEYS on the CPU."""
    m, params = _dense_module(f, ch_in)
    for i in frozen:
        params[i].requires_grad_(False)
    x = f['x'].cuda().requires_grad_(True)
    x6, flow = m(x)
    wanted = [x] if x_only else [x] + [p for p in params if p.requires_grad]
    g = list(torch.autograd.grad([x6, flow], wanted, [f['g_x6'].cuda(), f['g_flow'].cuda()]))
    torch.cuda.synchronize()
    res = {'x6': x6.detach().cpu(), 'flow': flow.detach().cpu(), 'dx': g.pop(0).cpu()}
    if not x_only:
        full = [None if not p.requires_grad else g.pop(0).cpu() for p in params]
        res['dw'], res['db'] = full[0::2], full[1::2]
    return res


_VENDOR = {}


def _dense_vendor(AF, case, slope):
    """e per tensor of the vendor path, the larger of two runs (measured once per fixture, against the same twin)."""
    key = ('dense', case, slope)
    if key not in _VENDOR:
        f, ref, mag, _ = _dense_ref(case, slope)
        with pytest.MonkeyPatch.context() as mp:
            _vendor(mp, AF)
            runs = [_errors(_dense_run(f, case[0]), ref, mag, DENSE_KEYS) for _ in range(2)]
        _VENDOR[key] = collections.OrderedDict((k, max(runs[0][k], runs[1][k])) for k in runs[0])
    return _VENDOR[key]


def _dense_path(monkeypatch, AF, path):
    _force_rules(monkeypatch, AF)
    for name in SWITCHES:
        monkeypatch.setattr(AF, name, True)
    if path == 'composed':
        monkeypatch.setattr(AF, '_DENSE_BLOCK', False)
    elif path == 'node':
        monkeypatch.setattr(AF, '_DENSE_INPLACE', False)


def _spy(monkeypatch, AF):
    calls, real = [], AF._call

    def spy(name, *args, **kw):
        calls.append((name, args))
        return real(name, *args, **kw)
    monkeypatch.setattr(AF, '_call', spy)
    return calls


@pytest.mark.parametrize('path', ['composed', 'node', 'inplace'])
@pytest.mark.parametrize('slope', SLOPES)
@pytest.mark.parametrize('case', DENSE_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_dense_estimator_against_the_twin(monkeypatch, AF, case, slope, path):
    f, ref, mag, counts = _dense_ref(case, slope)
    e_vendor = _dense_vendor(AF, case, slope)
    _dense_path(monkeypatch, AF, path)
    calls = _spy(monkeypatch, AF)
    r1 = _dense_run(f, case[0])
    names = collections.Counter(n for n, _ in calls)
    # the path under test is the one that ran: every convolution native, and the node's own launches only on its paths
    assert names['arflow_splitconv_fwd_ex'] == 10 and names['arflow_splitconv_wgrad'] == 5 and names['arflow_headconv_fwd'] == 1, names
    assert names['arflow_dense_grad_gather'] == (0 if path == 'composed' else 6), names
    assert names['arflow_dense_cat_fwd'] == (5 if path == 'node' else 0), names
    assert names['arflow_bias_act_fwd'] == (5 if path == 'composed' else 0), names
    if path == 'composed':
        with AF.deterministic():
            r2, r3 = _dense_run(f, case[0]), _dense_run(f, case[0])
        _assert_bitwise(r2, r3, DENSE_KEYS, 'composed, deterministic mode')
        for k in ('x6', 'flow', 'dx', 'dw'):
            _assert_bitwise({k: r1[k]}, {k: r2[k]}, (k,), 'composed, default against deterministic mode')
    else:
        _assert_bitwise(r1, _dense_run(f, case[0]), DENSE_KEYS, path)
    assert not AF.is_deterministic()
    _check('dense %s %s' % (_name(case, slope), path), _errors(r1, ref, mag, DENSE_KEYS), e_vendor, counts, DENSE_KEYS)


@pytest.mark.parametrize('path', ['node', 'inplace'])
@pytest.mark.parametrize('case', [(19, 2, 9, 35), (147, 2, 20, 8)], ids=lambda c: 'x'.join(map(str, c)))
def test_dense_node_partial_gradients_equal_the_full_call(monkeypatch, AF, case, path):
    f = _dense_ref(case, 0.1)[0]
    _dense_path(monkeypatch, AF, path)
    full = _dense_run(f, case[0])
    only_x = _dense_run(f, case[0], x_only=True)
    assert torch.equal(only_x['dx'], full['dx']), 'dx alone differs from the full call\'s'
    for frozen in (4, 0):  # w_3: the chain below it is still followed; w_1: the lowest layer's weight gradient skipped
        part = _dense_run(f, case[0], frozen=(frozen,))
        assert part['dw'][frozen // 2] is None
        for (name, a), (_, b) in zip(_flat(part, DENSE_KEYS), _flat(full, DENSE_KEYS)):
            assert a is None or torch.equal(a, b), 'w_%d frozen: %s differs from the full call\'s' % (frozen // 2 + 1, name)


# ---- b. the context network -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _context_ref(case, slope):
    f = R.context_fixture(*case, slope)
    ref = R.context_grads(f['x'], f['params'], slope, f['g_out'])
    return f, ref, R.context_magnitudes(f['x'], f['params'], f['g_out']), R.context_counts(*case)


CONTEXT_STATE = ['convs.%d.0.%s' % (k, n) for k in range(7) for n in ('weight', 'bias')]


def _context_run(f, ch_in):
    from arflow_amd.models import blocks
    m = blocks.ContextNetwork(ch_in)
    assert list(m.state_dict().keys()) == CONTEXT_STATE
    with torch.no_grad():
        for k, layer in enumerate(m.convs):
            layer[0].weight.copy_(f['params'][2 * k])
            layer[0].bias.copy_(f['params'][2 * k + 1])
            if k < 6:
                layer[1].negative_slope = f['slope']
    m = m.cuda()
    params = [p for layer in m.convs for p in (layer[0].weight, layer[0].bias)]
    x = f['x'].cuda().requires_grad_(True)
    out = m(x)
    g = [t.cpu() for t in torch.autograd.grad(out, [x] + params, f['g_out'].cuda())]
    torch.cuda.synchronize()
    return {'out': out.detach().cpu(), 'dx': g[0], 'dw': g[1::2], 'db': g[2::2]}


def _context_vendor(AF, case, slope):
    key = ('context', case, slope)
    if key not in _VENDOR:
        f, ref, mag, _ = _context_ref(case, slope)
        with pytest.MonkeyPatch.context() as mp:
            _vendor(mp, AF)
            runs = [_errors(_context_run(f, case[0]), ref, mag, CONTEXT_KEYS) for _ in range(2)]
        _VENDOR[key] = collections.OrderedDict((k, max(runs[0][k], runs[1][k])) for k in runs[0])
    return _VENDOR[key]


@pytest.mark.parametrize('wgrad', [None, '1111'], ids=['wgrad_default', 'wgrad_1111'])
@pytest.mark.parametrize('slope', SLOPES)
@pytest.mark.parametrize('case', CONTEXT_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_context_network_against_the_twin(monkeypatch, AF, case, slope, wgrad):
    f, ref, mag, counts = _context_ref(case, slope)
    e_vendor = _context_vendor(AF, case, slope)
    _force_rules(monkeypatch, AF)
    for name in SWITCHES:
        monkeypatch.setattr(AF, name, True)
    if wgrad is None:
        monkeypatch.delenv('ARFLOW_DILATED_WGRAD', raising=False)
    else:
        monkeypatch.setenv('ARFLOW_DILATED_WGRAD', wgrad)
    calls = _spy(monkeypatch, AF)
    r1 = _context_run(f, case[0])
    names = collections.Counter(n for n, _ in calls)
    # layers 1 and 6 through ConvAct, the chain's four layers on their mosaics; five moves forward and one backward
    assert names['arflow_splitconv_fwd_ex'] == 12 and names['arflow_phase_move'] == 6 and names['arflow_phase_act_bwd'] == 4, names
    assert names['arflow_splitconv_wgrad'] == 2 + (1 if wgrad is None else 4), names
    # the default mode's bias gradient of layers 1 and 6 ends in fp32 atomics: their two-call comparison runs in the mode
    with AF.deterministic():
        r2, r3 = _context_run(f, case[0]), _context_run(f, case[0])
    assert not AF.is_deterministic()
    # (a chain layer whose weight gradient is left to MIOpen is left out: that solver may end in atomics,
    # tests/test_dilated_chain_gpu.py)
    lib = () if wgrad else (2, 3, 4)

    def fixed(r, db):
        return {'out': r['out'], 'dx': r['dx'], 'dw': [t for k, t in enumerate(r['dw']) if k not in lib], 'db': [r['db'][k] for k in db]}
    _assert_bitwise(fixed(r2, range(7)), fixed(r3, range(7)), CONTEXT_KEYS, 'deterministic mode')
    _assert_bitwise(fixed(r1, (1, 2, 3, 4, 6)), fixed(r2, (1, 2, 3, 4, 6)), CONTEXT_KEYS, 'default against deterministic mode')
    _check('context %s %s' % (_name(case, slope), 'wgrad ' + (wgrad or 'default')), _errors(r1, ref, mag, CONTEXT_KEYS), e_vendor,
           counts, CONTEXT_KEYS)


# ---- c, d. the benchmarked model on its native paths ----------------------------------------------------------------------
def _bench_model():
    import arflow_amd.models as M
    from arflow_amd.config import AttrDict
    from oracle.fixture_common import fill_deterministic
    cfg = AttrDict(level_dropout=0.0, feature_norm=True, align_corners=True, warp_pad='zeros', n_frames=2, reduce_dense=False)
    return fill_deterministic(M.PWCLiteUflow(cfg))


def _expected_launches(backward):
    """Launch counts the routing table gives for one decoder pass (both directions in one batch)."""
    fwd = sum(f for lv in ROUTING.values() for f, _, _ in lv['layers']) + ROUTING_CONTEXT['first'][0] + ROUTING_CONTEXT['sixth'][0] + 4
    n = {'arflow_splitconv_fwd_ex': fwd, 'arflow_splitconv_wgrad': 0, 'arflow_phase_move': 5, 'arflow_headconv_fwd': 5,
         'arflow_headconv_bwd_data': 0, 'arflow_headconv_bwd_weight': 0, 'arflow_dense_grad_gather': 0,
         'arflow_dense_cat_fwd': 5 * sum(not lv['inplace'] for lv in ROUTING.values())}
    if backward:
        n['arflow_splitconv_fwd_ex'] += (sum(d for lv in ROUTING.values() for _, d, _ in lv['layers']) + ROUTING_CONTEXT['first'][1] +
                                         ROUTING_CONTEXT['sixth'][1] + 4)
        n['arflow_splitconv_wgrad'] = (sum(w for lv in ROUTING.values() for _, _, w in lv['layers']) + ROUTING_CONTEXT['first'][2] +
                                       ROUTING_CONTEXT['sixth'][2] + 1)  # + the chain's d = 2 layer (_DILATED_WGRAD_NATIVE)
        n.update({'arflow_phase_move': 6, 'arflow_headconv_bwd_data': 5, 'arflow_headconv_bwd_weight': 5,
                  'arflow_dense_grad_gather': 6 * len(ROUTING)})
    return n


def _assert_launches(calls, backward):
    names = collections.Counter(n for n, _ in calls)
    want = _expected_launches(backward)
    assert {k: names[k] for k in want} == want
    # nothing of the split-bf16 stack at the two coarse levels: every call on a plain map is at 24 x 32 or 48 x 64 (the others
    # are the chain's, on its mosaics of the finest level)
    shapes = collections.Counter(tuple(a[8:13]) for n, a in calls if n == 'arflow_splitconv_fwd_ex')  # (N, C, K, H, W)
    plain = {s: c for s, c in shapes.items() if s[0] == 4}
    assert {s[3:] for s in plain} == {(24, 32), (48, 64)}, shapes
    assert sum(shapes.values()) - sum(plain.values()) == (8 if backward else 4), shapes
    assert {s[3:] for n, a in calls if n == 'arflow_splitconv_wgrad' for s in [tuple(a[6:11])] if s[0] == 4} <= {(24, 32), (48, 64)}


def test_benchmark_model_on_its_native_paths_vs_oracle_twin(monkeypatch, AF):
    from oracle.fixture_common import synth_pair
    from oracle.host_models import oracle_ops
    from tests.helpers import epe
    assert [s for s, _ in BENCH_LEVELS][2:] == [(48, 80), (96, 160)]
    x = synth_pair(2, 192, 256, torch.Generator().manual_seed(11))[0]
    torch.set_num_threads(16)
    patch_floor_to_benchmark(monkeypatch)
    calls = _spy(monkeypatch, AF)
    with torch.no_grad():
        hip = _bench_model().cuda().eval()(x.cuda(), with_bk=True)
    _assert_launches(calls, backward=False)
    ref_model = _bench_model().eval()
    with torch.no_grad(), oracle_ops(ref_model):
        ref = ref_model(x, with_bk=True)
    for k in ('flows_fw', 'flows_bw'):
        assert len(hip[k]) == len(ref[k])
        for i, (a, b) in enumerate(zip(hip[k], ref[k])):
            e = epe(a, b)
            print('native paths %s level %d (%s): EPE %.3e px' % (k, i, tuple(b.shape[2:]), e))
            assert e <= 1e-3, '%s level %d (%s): EPE %.3e px vs the oracle twin' % (k, i, tuple(b.shape[2:]), e)


def test_benchmark_model_is_reproducible_in_deterministic_mode(monkeypatch, AF):
    from arflow_amd import loss_blocks as LB
    from arflow_amd.warp_utils import flow_warp
    from oracle.fixture_common import synth_pair
    from tests.test_models_gpu import _smooth_objective
    x = synth_pair(2, 192, 256, torch.Generator().manual_seed(11))[0].cuda()
    patch_floor_to_benchmark(monkeypatch)
    calls = _spy(monkeypatch, AF)
    runs = []
    # DESIGN.md section 14's reproducible setting: the mode, and MIOpen asked for its deterministic solvers (the extractor's and
    # the coarse levels' convolutions are the vendor's; its default weight gradients end in atomics)
    with AF.deterministic(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        for _ in range(2):
            del calls[:]
            m = _bench_model().cuda().train()
            res = m(x, with_bk=True)
            loss = _smooth_objective(res['flows_fw'], res['flows_bw'], x, flow_warp, LB.smooth_grad_1st)
            grads = torch.autograd.grad(loss, list(m.parameters()))
            _assert_launches(calls, backward=True)
            runs.append(([f.detach() for k in ('flows_fw', 'flows_bw') for f in res[k]], grads, [n for n, _ in m.named_parameters()]))
    assert not AF.is_deterministic()
    for i, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
        assert torch.equal(a, b), 'flow %d differs between two runs in %d elements' % (i, int((a != b).sum()))
    for n, a, b in zip(runs[0][2], runs[0][1], runs[1][1]):
        assert torch.equal(a, b), 'gradient of %s differs between two runs in %d elements (max |diff| %.3e)' % (
            n, int((a != b).sum()), float((a - b).abs().max()))
