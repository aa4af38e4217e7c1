"""GPU: the output-upsample kernels (csrc/upsample.hip; AF.out_upsample, AF.out_tail) per pixel against the float64
restatement of upsample_out (tests/prob_ref.py, pinned to the composed ATen path in tests/test_prob_model_cpu.py).

Bounds are derived, not tuned (EPS = 2^-24, the unit roundoff of fp32):
  forward   |out - ref| <= 6 EPS s_c sum_i w_i |a_i + b_c|.  The kernel's operation order is ATen's (up_blend):
            wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d) on a = in + b_c, then an exact x2.  The weights are 0, 1/4, 3/4 or 1;
            a product by 3/4 rounds, so the count is by depth: every tap passes the bias add, a product, an addition, a
            product and an addition -- five roundings, (1 + EPS)^5 - 1 < 6 EPS of the sum of magnitudes.  The issue's count
            (five, bound six) therefore stands although its products are not all exact.
  adjoint   |g - ref| <= 20 EPS s_c sum w |gfine|.  At most 16 terms: a fine pixel's term passes at most four fused
            multiply-adds of its row and four of the column of row sums (the weight of a cell both of whose clamped taps
            coincide, 1/4 + 3/4, is exact) -- eight roundings, inside the issue's twenty.
The bias is a value fp32 represents exactly (the kernel takes a float): the model's own constant is rounded the same way by
the reference's fp32 addition.
The tail kernel's tile is TAIL_TH x TAIL_TW = 8 x 16 level-2 cells; 9 x 17 and 9 x 18 are one cell larger in each direction
(scalar and float4 path)."""
import ctypes
import math

import pytest
import torch

from tests import prob_ref as R

pytestmark = pytest.mark.gpu

BIAS = float(torch.tensor(math.log(2.0), dtype=torch.float32))
TAIL_TILE = (8, 16)
SHAPES = [(1, 1), (2, 3), (5, 7), (12, 20), (TAIL_TILE[0] + 1, TAIL_TILE[1] + 1), (TAIL_TILE[0] + 1, TAIL_TILE[1] + 2)]
SPLITS = [(2, 2, 4), (2, 2, 34), (0, 2, 3), (2, 0, 2)]
B = 2


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    return functional


_cache = {}


def case(shape, split):
    """Seeded input, fine gradient and the float64 references, computed once per (shape, split) and left unchanged."""
    key = (shape, split)
    if key not in _cache:
        n_flow, n_diag, C = split
        h, w = shape
        g = torch.Generator().manual_seed(1000 * h + 10 * w + C)
        x = 3.0 * torch.randn(B, C, h, w, generator=g)
        go = torch.randn(B, C, 2 * h, 2 * w, generator=g)
        ref, mag = R.upsample_out_ref(x, n_flow, n_diag, BIAS)
        gref, gmag = R.upsample_out_adjoint_ref(go, n_flow)
        _cache[key] = dict(x=x, go=go, ref=ref, mag=mag, gref=gref, gmag=gmag)
    return _cache[key]


def fwd_excess(out, c):
    """max over pixels of |out - ref| - bound (<= 0: inside)."""
    return float(((out.detach().cpu().double() - c['ref']).abs() - R.FWD_ROUNDINGS * R.EPS * c['mag']).max())


def bwd_excess(g, c):
    return float(((g.detach().cpu().double() - c['gref']).abs() - R.BWD_ROUNDINGS * R.EPS * c['gmag']).max())


@pytest.mark.parametrize('split', SPLITS, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_forward_adjoint_and_tail_per_pixel(AF, shape, split):
    n_flow, n_diag, C = split
    c = case(shape, split)
    x = c['x'].cuda().requires_grad_(True)
    out = AF.out_upsample(x, n_flow, n_diag, BIAS)
    e = fwd_excess(out, c)
    print('forward excess %.3e' % e)
    assert out.shape == c['ref'].shape and e <= 0, 'forward outside 6 EPS sum w|a + b| by %.3e' % e
    (gx,) = torch.autograd.grad(out, x, c['go'].cuda())
    e = bwd_excess(gx, c)
    print('adjoint excess %.3e' % e)
    assert e <= 0, 'adjoint outside 20 EPS sum w|g| by %.3e' % e
    # the tail = two x2 calls, bit for bit, forward and backward
    x2 = c['x'].cuda().requires_grad_(True)
    o1 = AF.out_upsample(x2, n_flow, n_diag, BIAS)
    o0 = AF.out_upsample(o1, n_flow, n_diag, BIAS)
    x3 = c['x'].cuda().requires_grad_(True)
    t1, t0 = AF.out_tail(x3, n_flow, n_diag, BIAS)
    assert torch.equal(t1, o1) and torch.equal(t0, o0)
    g = torch.Generator().manual_seed(7)
    g1, g0 = torch.randn(o1.shape, generator=g).cuda(), torch.randn(o0.shape, generator=g).cuda()
    (ga,) = torch.autograd.grad([o1, o0], x2, [g1, g0])
    (gb,) = torch.autograd.grad([t1, t0], x3, [g1, g0])
    assert torch.equal(ga, gb)
    for only in (0, 1):  # either gradient may be absent
        x4 = c['x'].cuda().requires_grad_(True)
        t = AF.out_tail(x4, n_flow, n_diag, BIAS)
        x5 = c['x'].cuda().requires_grad_(True)
        p1 = AF.out_upsample(x5, n_flow, n_diag, BIAS)
        p = (p1, AF.out_upsample(p1, n_flow, n_diag, BIAS))
        gg = (g1, g0)[only]
        assert torch.equal(torch.autograd.grad(t[only], x4, gg)[0], torch.autograd.grad(p[only], x5, gg)[0])


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_reference_in_fp32_sits_inside_the_bounds(shape):
    """The float64 reference evaluated in fp32 on the CPU: the bounds hold for a plain fp32 evaluation, not just the kernel."""
    for split in SPLITS:
        c = case(shape, split)
        out32, _ = R.upsample_out_ref(c['x'], split[0], split[1], BIAS, dtype=torch.float32)
        assert fwd_excess(out32, c) <= 0
        g32, _ = R.upsample_out_adjoint_ref(c['go'], split[0], dtype=torch.float32)
        assert bwd_excess(g32, c) <= 0


def test_mutations_fall_outside_the_bounds():
    """What the bounds can tell apart, on the references themselves (float64, so the only difference is the mutation): the
    scale on a diag channel, the bias on a flow channel, align_corners=True weights and a one-cell shift all fall outside.
    The fifth mutation asked for, the bias added after the blend at a border pixel, cannot: the blend's weights sum to 1 at
    every pixel, so both orders agree up to roundings -- asserted here as inside the bound, see the comment below."""
    split, shape = (2, 2, 4), (5, 7)
    c = case(shape, split)
    x = c['x'].double()
    s, b = R.chan_rule(4, 2, 2, BIAS, torch.float64)
    muts = {
        'scale 2 on a diag channel': R.chan_rule(4, 3, 1, 0.0, torch.float64)[0] * R.up2(x + b),
        'bias on a flow channel': s * R.up2(x + R.chan_rule(4, 0, 3, BIAS, torch.float64)[1].roll(1, 1)),
        'align_corners=True weights': s * R.up2(x + b, align=True),
        'one-cell shift': s * R.up2(x + b, shift=1),
    }
    assert float((R.chan_rule(4, 0, 3, BIAS, torch.float64)[1].roll(1, 1).flatten() - torch.tensor([0, BIAS, BIAS, BIAS])).abs().max()) == 0
    for name, out in muts.items():
        assert fwd_excess(out, c) > 0, name
    gs = {
        'scale 2 on a diag channel': R.upsample_out_adjoint_ref(c['go'], 3)[0],
        'one-cell shift': torch.autograd.grad(s * R.up2(z := torch.zeros_like(x, requires_grad=True), shift=1), z, c['go'].double())[0],
        'align_corners=True weights': torch.autograd.grad(s * R.up2(z := torch.zeros_like(x, requires_grad=True), align=True), z,
                                                          c['go'].double())[0],
    }
    for name, g in gs.items():
        assert bwd_excess(g, c) > 0, name
    # "bias added after the blend at a border pixel" is NOT a distinguishable mutation: the blend's weights sum to 1 at every
    # pixel (at a border pixel one tap carries all of it), so blend(a + b) = blend(a) + b exactly and the two orders differ
    # by roundings only, inside the bound by construction.  What the order fixes is bitwise equality with the reference's
    # operation order, which the A/B comparison of the model (tests/test_prob_model_gpu.py) and the tail's bitwise test hold.
    after = s * R.up2(x) + s * b
    assert fwd_excess(after, c) <= 0


def test_channel_slice_source_and_unaligned_slot(AF):
    """Source = [:, 0:4] of a 34-channel tensor used in place; destination = a slot of a wider buffer whose address is not
    a multiple of 16 bytes (the x2 output's planes are 4 h w floats, so a channel offset alone cannot break the alignment:
    the buffer itself starts one float into its storage); NaN-prefilled, so every element is written and nothing else is."""
    for shape in ((12, 20), (5, 7)):
        h, w = shape
        c = case(shape, (2, 2, 4))
        wide = torch.full((B, 34, h, w), float('nan')).cuda()
        wide[:, 0:4] = c['x'].cuda()
        for lead in (0, 1):
            n = B * 9 * 4 * h * w
            flat = torch.full((n + lead,), float('nan'), device='cuda')
            buf = flat[lead:].view(B, 9, 2 * h, 2 * w)
            assert (buf.data_ptr() % 16 != 0) == bool(lead)
            out = AF.out_upsample(wide[:, 0:4], 2, 2, BIAS, out=buf[:, 3:7])
            assert out.data_ptr() == buf[:, 3:7].data_ptr()
            assert fwd_excess(buf[:, 3:7], c) <= 0
            assert bool(torch.isnan(buf[:, :3]).all()) and bool(torch.isnan(buf[:, 7:]).all())
            if lead:
                assert bool(torch.isnan(flat[:1]).all())
        # the adjoint reads a slot and writes every element; the tail reads the slice in place
        gwide = torch.full((B, 9, 2 * h, 2 * w), float('nan')).cuda()
        gwide[:, 3:7] = c['go'].cuda()
        x = wide.clone().nan_to_num(0.0).requires_grad_(True)
        y = AF.out_upsample(x[:, 0:4], 2, 2, BIAS)
        (gx,) = torch.autograd.grad(y, x, gwide[:, 3:7])
        assert bwd_excess(gx[:, 0:4], c) <= 0 and float(gx[:, 4:].abs().max()) == 0
        t1, t0 = AF.out_tail(wide[:, 0:4], 2, 2, BIAS)
        assert fwd_excess(t1, c) <= 0 and bool(torch.isfinite(t0).all())


def test_gradient_flows_through_a_slot(AF):
    c = case((5, 7), (2, 2, 4))
    x = c['x'].cuda().requires_grad_(True)
    buf = torch.zeros(B, 6, 10, 14, device='cuda')
    AF.out_upsample(x, 2, 2, BIAS, out=buf[:, 1:5])
    go = torch.zeros(B, 6, 10, 14, device='cuda')
    go[:, 1:5] = c['go'].cuda()
    (gx,) = torch.autograd.grad(buf, x, go)
    assert bwd_excess(gx, c) <= 0


def test_three_runs_are_bitwise_equal_in_both_modes(AF):
    c = case((12, 20), (2, 2, 34))
    x, go = c['x'].cuda(), c['go'].cuda()
    g0 = torch.randn(B, 34, 48, 80, generator=torch.Generator().manual_seed(3)).cuda()

    def run():
        xx = x.clone().requires_grad_(True)
        out = AF.out_upsample(xx, 2, 2, BIAS)
        (gx,) = torch.autograd.grad(out, xx, go)
        x2 = x.clone().requires_grad_(True)
        t1, t0 = AF.out_tail(x2, 2, 2, BIAS)
        (gt,) = torch.autograd.grad([t1, t0], x2, [go, g0])
        return out, gx, t1, t0, gt
    first = run()
    for _ in range(2):
        assert all(torch.equal(a, b) for a, b in zip(first, run()))
    with AF.deterministic():
        for _ in range(3):
            assert all(torch.equal(a, b) for a, b in zip(first, run()))


def test_bad_arguments_return_the_abi_codes(AF):
    """Validation happens before any launch: the codes of include/arflow_hip.h, nothing enqueued."""
    from arflow_amd import _lib
    lib = _lib.load()
    x = torch.zeros(2, 4, 3, 5, device='cuda')
    out = torch.full((2, 4, 6, 10), float('nan'), device='cuda')
    o0 = torch.full((2, 4, 12, 20), float('nan'), device='cuda')
    px, po, p0 = x.data_ptr(), out.data_ptr(), o0.data_ptr()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(i=px, ibs=60, o=po, obs=240, B=2, C=4, h=3, w=5, nf=2, nd=2)
    faults = [(dict(i=None), -1001), (dict(o=None), -1001), (dict(B=0), -1002), (dict(h=0), -1002), (dict(w=-1), -1002),
              (dict(C=0), -1002), (dict(ibs=59), -1002), (dict(obs=239), -1002), (dict(nf=-1), -1003), (dict(nf=3, nd=2), -1003)]
    for change, want in faults:
        a = dict(good, **change)
        assert lib.arflow_out_up2_fwd(a['i'], a['ibs'], a['o'], a['obs'], a['B'], a['C'], a['h'], a['w'], a['nf'], a['nd'],
                                      0.5, s) == want, change
        if 'nd' not in change:
            # the adjoint reads the fine tensor (stride >= 4 C h w) and writes the coarse one
            assert lib.arflow_out_up2_bwd(a['o'], a['obs'], a['i'], a['ibs'], a['B'], a['C'], a['h'], a['w'], a['nf'],
                                          s) == want, change
        if 'obs' not in change:
            assert lib.arflow_out_tail_fwd(a['i'], a['ibs'], a['o'], p0, a['B'], a['C'], a['h'], a['w'], a['nf'], a['nd'],
                                           0.5, s) == want, change
    assert lib.arflow_out_tail_fwd(px, 60, po, None, 2, 4, 3, 5, 2, 2, 0.5, s) == -1001
    assert lib.arflow_out_up2_bwd(po, 240, px, 60, 2, 4, 3, 5, 5, s) == -1003  # n_flow > C
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(o0).all()) and float(x.abs().max()) == 0
    with pytest.raises(ValueError):
        AF.out_upsample(x, 3, 2, 0.5)
    with pytest.raises(_lib.ArflowHipError):
        AF.out_upsample(x.cpu(), 2, 2, 0.5)
    assert not AF.out_up_supported(x.cpu()) and AF.out_up_supported(x)
