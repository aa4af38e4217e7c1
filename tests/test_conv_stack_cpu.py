"""CPU: the float64 twins of tests/conv_stack_ref.py against the product modules, the sign margins of every fixture the GPU
tests use, the mutations their bounds must catch, and the routing table of the benchmark's decoder."""
import pytest
import torch
import torch.nn.functional as F

import arflow_amd.functional as AF
from arflow_amd.models import blocks
from tests import conv_stack_ref as R

# the fixtures of tests/test_conv_stack_gpu.py: (ch_in, N, H, W)
DENSE_CASES = [(19, 2, 9, 35), (19, 2, 20, 8), (147, 2, 9, 35), (147, 2, 20, 8)]
CONTEXT_CASES = [(37, 2, 19, 35), (37, 2, 16, 33), (597, 2, 19, 35), (597, 2, 16, 33)]
SLOPES = (0.1, 1.0)


def _flat(res, keys):
    out = []
    for k in keys:
        v = res[k]
        out += [('%s[%d]' % (k, i), t) for i, t in enumerate(v)] if isinstance(v, list) else [(k, v)]
    return out


DENSE_KEYS = ('x6', 'flow', 'dx', 'dw', 'db')
CONTEXT_KEYS = ('out', 'dx', 'dw', 'db')


def _caps(counts, keys):
    return [R.gamma(n) for _, n in _flat(counts, keys)]


def _swap_bias_act(monkeypatch):
    monkeypatch.setattr(blocks, 'bias_act', lambda y, b, s: F.leaky_relu(y + b.view(1, -1, 1, 1), s))


@pytest.mark.parametrize('slope', SLOPES)
def test_dense_twin_equals_flow_estimator_dense(monkeypatch, slope):
    _swap_bias_act(monkeypatch)
    f = R.dense_fixture(19, 2, 9, 35, slope, seed=1)
    ref = R.dense_grads(f['x'], f['params'], slope, f['g_x6'], f['g_flow'])
    mag = R.dense_magnitudes(f['x'], f['params'], f['g_x6'], f['g_flow'])
    m = blocks.FlowEstimatorDense(19).double()
    layers = (m.conv1, m.conv2, m.conv3, m.conv4, m.conv5, m.conv_last)
    with torch.no_grad():
        for k, layer in enumerate(layers):
            layer[0].weight.copy_(f['params'][2 * k])
            layer[0].bias.copy_(f['params'][2 * k + 1])
            if k < 5:
                layer[1].negative_slope = slope
    x = f['x'].double().requires_grad_(True)
    x6, flow = m(x)
    params = [p for layer in layers for p in (layer[0].weight, layer[0].bias)]
    g = torch.autograd.grad([x6, flow], [x] + params, [f['g_x6'].double(), f['g_flow'].double()])
    got = {'x6': x6, 'flow': flow, 'dx': g[0], 'dw': list(g[1::2]), 'db': list(g[2::2])}
    for (name, a), (_, b), (_, mm) in zip(_flat(got, DENSE_KEYS), _flat(ref, DENSE_KEYS), _flat(mag, DENSE_KEYS)):
        e = R.rel_err(a, b, mm)
        assert e <= 1e-12, '%s: twin and module differ by %.3e M' % (name, e)


@pytest.mark.parametrize('slope', SLOPES)
def test_context_twin_equals_context_network(monkeypatch, slope):
    _swap_bias_act(monkeypatch)
    f = R.context_fixture(37, 2, 19, 35, slope, seed=1)
    ref = R.context_grads(f['x'], f['params'], slope, f['g_out'])
    mag = R.context_magnitudes(f['x'], f['params'], f['g_out'])
    m = blocks.ContextNetwork(37).double()
    with torch.no_grad():
        for k, layer in enumerate(m.convs):
            layer[0].weight.copy_(f['params'][2 * k])
            layer[0].bias.copy_(f['params'][2 * k + 1])
            if k < 6:
                layer[1].negative_slope = slope
    x = f['x'].double().requires_grad_(True)
    out = m(x)
    params = [p for layer in m.convs for p in (layer[0].weight, layer[0].bias)]
    g = torch.autograd.grad(out, [x] + params, f['g_out'].double())
    got = {'out': out, 'dx': g[0], 'dw': list(g[1::2]), 'db': list(g[2::2])}
    for (name, a), (_, b), (_, mm) in zip(_flat(got, CONTEXT_KEYS), _flat(ref, CONTEXT_KEYS), _flat(mag, CONTEXT_KEYS)):
        e = R.rel_err(a, b, mm)
        assert e <= 1e-12, '%s: twin and module differ by %.3e M' % (name, e)


@pytest.mark.parametrize('slope', SLOPES)
@pytest.mark.parametrize('case', DENSE_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_dense_fixture_sign_margin(case, slope):
    """min |z| / M(z) of every layer above that layer's cap: no correct fp32 evaluation flips a LeakyReLU branch, so the GPU
    tests compare every element."""
    f = R.dense_fixture(*case, slope)
    ref = R.dense_grads(f['x'], f['params'], slope, f['g_x6'], f['g_flow'])
    mag = R.dense_magnitudes(f['x'], f['params'], f['g_x6'], f['g_flow'])
    margins = R.sign_margins(ref['z'], mag['z'])
    caps = [R.gamma(n) for n in R.dense_counts(*case)['z']]
    print('dense %s slope %g: sign margin / cap per layer: %s' % (
        'x'.join(map(str, case)), slope, '  '.join('%.4f / %.2e' % mc for mc in zip(margins, caps))))
    for k, (z, b) in enumerate(zip(ref['z'], f['params'][1:10:2])):
        assert bool(((z > 0) == (b.view(1, -1, 1, 1) > 0)).all()), 'layer %d: a pre-activation left its bias\'s sign' % (k + 1)
        assert float(z.abs().min()) >= 0.7
    assert all(m > c for m, c in zip(margins, caps)), (margins, caps)


@pytest.mark.parametrize('slope', SLOPES)
@pytest.mark.parametrize('case', CONTEXT_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_context_fixture_sign_margin(case, slope):
    f = R.context_fixture(*case, slope)
    ref = R.context_grads(f['x'], f['params'], slope, f['g_out'])
    mag = R.context_magnitudes(f['x'], f['params'], f['g_out'])
    margins = R.sign_margins(ref['z'], mag['z'])
    caps = [R.gamma(n) for n in R.context_counts(*case)['z']]
    print('context %s slope %g: sign margin / cap per layer: %s' % (
        'x'.join(map(str, case)), slope, '  '.join('%.4f / %.2e' % mc for mc in zip(margins, caps))))
    for k, (z, b) in enumerate(zip(ref['z'], f['params'][1:12:2])):
        assert bool(((z > 0) == (b.view(1, -1, 1, 1) > 0)).all()), 'layer %d: a pre-activation left its bias\'s sign' % (k + 1)
    assert all(m > c for m, c in zip(margins, caps)), (margins, caps)


# ---- mutations: a twin with one mistake of the kind the native paths could share must leave the cap ---------------------
def _outside(mut, ref, mag, counts, keys):
    """names of the tensors whose e exceeds their cap"""
    caps = _caps(counts, keys)
    return [name for (name, a), (_, b), (_, mm), cap in zip(_flat(mut, keys), _flat(ref, keys), _flat(mag, keys), caps)
            if not R.rel_err(a, b, mm) <= cap]


@pytest.fixture(scope='module')
def dense_case():
    case = (19, 2, 9, 35)
    f = R.dense_fixture(*case, 0.1)
    args = (f['x'], f['params'], 0.1, f['g_x6'], f['g_flow'])
    return args, R.dense_grads(*args), R.dense_magnitudes(f['x'], f['params'], f['g_x6'], f['g_flow']), R.dense_counts(*case)


@pytest.fixture(scope='module')
def context_case():
    case = (37, 2, 19, 35)
    f = R.context_fixture(*case, 0.1)
    args = (f['x'], f['params'], 0.1, f['g_out'])
    return args, R.context_grads(*args), R.context_magnitudes(f['x'], f['params'], f['g_out']), R.context_counts(*case)


def test_unmutated_twins_are_inside_every_cap(dense_case, context_case):
    for (args, ref, mag, counts), fn, keys in ((dense_case, R.dense_grads, DENSE_KEYS), (context_case, R.context_grads, CONTEXT_KEYS)):
        assert _outside(fn(*args), ref, mag, counts, keys) == []


@pytest.mark.parametrize('mutate,must_catch', [('slot_order', {'x6', 'flow', 'dx'}), ('drop_source', {'dw[2]', 'db[2]'}),
                                               ('bias_slot', {'db[2]'})])
def test_dense_mutations_leave_the_cap(dense_case, mutate, must_catch):
    """x6's slots in the wrong order; one source dropped from the gather nest (a_3's gradient without dx_4: layer 3's own
    gradients lose a term of their size; further down the loss passes through weights scaled to 0.25 / max|conv| and stays inside the
    cap, which is why at least one tensor is asked for, not all; the forward cannot see it); layer 3's bias gradient taken from layer 4's slot (that one tensor only)."""
    args, ref, mag, counts = dense_case
    out = _outside(R.dense_grads(*args, mutate=mutate), ref, mag, counts, DENSE_KEYS)
    print('%s: outside the cap: %s' % (mutate, out))
    assert must_catch <= set(out), out
    if mutate != 'slot_order':
        assert not {'x6', 'flow'} & set(out), 'a backward mutation cannot move the forward: %s' % out
    if mutate == 'bias_slot':
        assert out == ['db[2]']


@pytest.mark.parametrize('mutate', ['dilation', 'swap_w2_w3', 'phase_shift'])
def test_context_mutations_leave_twice_the_fp32_error_but_not_the_cap(context_case, mutate):
    """Dilation 8 run as 4; w_2 and w_3 swapped (both 128 -> 128, so every shape still fits); phase (0, 0) of the d = 2
    mosaic shifted by one pixel -- a separator taken for a real pixel.

    The cap cannot tell any of the three apart, and the test says so: the context net is a serial chain, every layer of which
    multiplies M by sum |w| over 9 C taps while the value itself, a sum of random signs next to a bias of size 1, stays of
    size 1 -- M(z_6) is 58 on average where |z_6| is 1.1, and the gradients' M grows the same way from the other end -- so a
    mistake of the tensor's own size in the middle of the chain is 1e-5 M and less, inside gamma(n) = 3e-4.  (The dense
    estimator's mutations above are of size M: its concatenation keeps every activation one convolution away from x6, flow
    and the gradients.)  What tells them apart is the GPU tests' other criterion, e <= 2 x the e of the vendor's fp32 path,
    which stands at 1e-8 .. 1e-15 M here: every mutation exceeds twice the e of a plain fp32 evaluation on the CPU in dx and
    in each of the seven weight gradients (printed: by 26x at the least, by 1e6x in dx)."""
    (x, params, slope, g_out), ref, mag, counts = context_case
    kw = {}
    if mutate == 'dilation':
        kw['dilations'] = (1, 2, 4, 4, 16, 1, 1)
    elif mutate == 'swap_w2_w3':
        params = list(params)
        params[2], params[4] = params[4], params[2]
    else:
        kw['mutate'] = 'phase_shift'
    mut = R.context_grads(x, params, slope, g_out, **kw)
    assert _outside(mut, ref, mag, counts, CONTEXT_KEYS) == []
    plain = R.context_grads(*context_case[0], dtype=torch.float32)
    ratios = {}
    for (name, a), (_, p32), (_, b), (_, mm) in zip(_flat(mut, CONTEXT_KEYS), _flat(plain, CONTEXT_KEYS), _flat(ref, CONTEXT_KEYS),
                                                   _flat(mag, CONTEXT_KEYS)):
        ratios[name] = R.rel_err(a, b, mm) / R.rel_err(p32, b, mm)
    print('%s: e / e(fp32 on the CPU): %s' % (mutate, '  '.join('%s %.3g' % kv for kv in ratios.items())))
    for name in ['dx'] + ['dw[%d]' % k for k in range(7)]:
        assert ratios[name] > 2.0, (name, ratios[name])


def test_dense_mutations_leave_twice_the_fp32_error(dense_case):
    """The same stand-in for the dense estimator: far outside on the tensors the cap catches as well."""
    args, ref, mag, counts = dense_case
    plain = R.dense_grads(*args, dtype=torch.float32)
    assert _outside(plain, ref, mag, counts, DENSE_KEYS) == []
    for mutate, names in (('slot_order', ('x6', 'flow', 'dx')), ('drop_source', ('dx', 'dw[0]', 'dw[1]', 'dw[2]', 'db[2]')),
                          ('bias_slot', ('db[2]',))):
        mut = R.dense_grads(*args, mutate=mutate)
        for (name, a), (_, p32), (_, b), (_, mm) in zip(_flat(mut, DENSE_KEYS), _flat(plain, DENSE_KEYS), _flat(ref, DENSE_KEYS),
                                                       _flat(mag, DENSE_KEYS)):
            if name in names:
                assert R.rel_err(a, b, mm) > 2.0 * R.rel_err(p32, b, mm), (mutate, name)


# ---- routing ---------------------------------------------------------------------------------------------------------
# The benchmark's decoder: PWCLiteUflow, 8 pairs in both directions = decoder batch 16, 384 x 640 images.
# (level, layer C -> K): (forward, data gradient, weight gradient) on the split-bf16 kernels; per level whether the dense
# node runs in place; the in-place path's own weight-gradient rule adds no layer.
BENCH_LEVELS = [((12, 20), 115), ((24, 40), 147), ((48, 80), 147), ((96, 160), 147)]
NONE = [(0, 0, 0)] * 5
ROUTING = {
    (12, 20): {'layers': NONE, 'inplace': False},
    (24, 40): {'layers': NONE, 'inplace': False},
    (48, 80): {'layers': [(1, 1, 0),    # 147 -> 128
                          (1, 1, 1),    # 275 -> 128
                          (0, 1, 1),    # 403 -> 96
                          (0, 1, 1),    # 499 -> 64
                          (0, 1, 0)],   # 563 -> 32
               'inplace': False},
    (96, 160): {'layers': [(1, 1, 1)] * 5, 'inplace': True},
}
# the context net at the finest level: 597 -> 128, the dilated chain as one node, 64 -> 32
ROUTING_CONTEXT = {'first': (1, 1, 1), 'chain': True, 'sixth': (1, 1, 0)}


def routing_table(N, sizes):
    """The table the rules give for decoder batch N and [((H, W), ch_in)] levels, the context net at the last level."""
    table = {}
    for (H, W), ch_in in sizes:
        cins = [ch_in + sum(R.DENSE_OCS[:k]) for k in range(5)]
        layers = [(int(AF._splitconv_rule(N, c, k, H, W)), int(AF._splitconv_rule(N, k, c, H, W)),
                   int(AF._splitconv_wgrad_rule(N, c, k, H, W))) for c, k in zip(cins, R.DENSE_OCS)]
        inplace = all(fwd for fwd, _, _ in layers)
        assert not any(AF._inplace_wgrad_rule(N, c, k, H, W) and not w for c, k, (_, _, w) in zip(cins, R.DENSE_OCS, layers))
        table[(H, W)] = {'layers': layers, 'inplace': inplace}
    (H, W), ch_in = sizes[-1]
    ctx = {name: (int(AF._splitconv_rule(N, c, k, H, W)), int(AF._splitconv_rule(N, k, c, H, W)), int(AF._splitconv_wgrad_rule(N, c, k, H, W)))
           for name, c, k in (('first', ch_in + 450, 128), ('sixth', 64, 32))}
    ctx['chain'] = bool(AF._size_floor(N, H, W, 96, 160))
    return table, ctx


def patch_floor_to_benchmark(monkeypatch):
    """Let a 2 x 192 x 256 input (decoder batch 4, levels 6x8 .. 48x64) route as the benchmark's levels do."""
    real = AF._size_floor
    monkeypatch.setattr(AF, '_size_floor', lambda N, H, W, h, w: real(16, 2 * H, (5 * W) // 2, h, w))


def test_routing_table_of_the_benchmark_decoder(monkeypatch):
    table, ctx = routing_table(16, BENCH_LEVELS)
    assert table == ROUTING and ctx == ROUTING_CONTEXT
    assert AF.dilated_chain_takes(16, 96, 160) and not AF.dilated_chain_takes(16, 48, 80)
    small = [((6, 8), 115), ((12, 16), 147), ((24, 32), 147), ((48, 64), 147)]
    plain, plain_ctx = routing_table(4, small)
    assert all(v == {'layers': NONE, 'inplace': False} for v in plain.values()) and not plain_ctx['chain']
    patch_floor_to_benchmark(monkeypatch)
    patched, patched_ctx = routing_table(4, small)
    assert [patched[s] for s, _ in small] == [ROUTING[s] for s, _ in BENCH_LEVELS]
    assert patched_ctx == ROUTING_CONTEXT
    assert AF.dilated_chain_takes(4, 48, 64) and not AF.dilated_chain_takes(4, 24, 32)


def test_wgrad_rule_is_the_measured_table_through_the_one_floor():
    """_splitconv_wgrad_rule asks every size question through _size_floor; its answers are those of the expression it had
    (never below N H W = 16 x 48 x 80; the wide rule at 16 maps of 96 x 160; the narrow one for smaller maps only)."""
    def was(N, C, K, H, W):
        if N * H * W < 16 * 48 * 80:
            return False
        if H * W >= 96 * 160 and N * H * W >= 16 * 96 * 160:
            return 128 <= C <= 640 and 32 <= K <= 128
        return H * W < 96 * 160 and H * W >= 48 * 80 and N * H * W >= 16 * 48 * 80 and 256 <= C <= 640 and 64 <= K <= 128
    for N in (1, 4, 8, 15, 16, 17, 64, 256):
        for H, W in ((12, 20), (24, 40), (47, 80), (48, 80), (48, 81), (96, 159), (96, 160), (192, 320), (30, 128), (60, 256)):
            for C, K in ((147, 128), (275, 128), (403, 96), (499, 64), (563, 32), (597, 128), (64, 32), (127, 128), (641, 64)):
                assert AF._splitconv_wgrad_rule(N, C, K, H, W) == was(N, C, K, H, W), (N, C, K, H, W)
