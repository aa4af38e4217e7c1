"""GPU: arflow_bias_act_fwd / _fwd_mom / _bwd (csrc/act.hip) on their own -- the kernels every bit-for-bit chain of the
convolution stack ends in (dense_cat, the in-place epilogue, phase_act_bwd and the gbias bounds all say "equals bias_act").

Shapes (B, C, HW) walk the launch geometry: a plane is cut into chunks of 4096 elements (256 threads x 16), one workgroup
each, float4 accesses where HW % 4 == 0 and scalar ones elsewhere:
    (1, 1, 1)      one element;
    (3, 5, 15)     one short chunk, scalar;
    (2, 3, 4221)   two chunks on the scalar path;
    (1, 2, 4160)   two chunks on the float4 path, the second holding 64 elements: three of its four waves are empty;
    (2, 2, 8192)   two full chunks.
Slopes 0.1, 0.25, 1.0, 0.0; with and without bias; the forward in place (y == x, which the header allows) and out of place
(the header allows no aliasing of gin, so the backward is out of place).  Every call goes straight to the C entry point: the
Python wrapper is in place only, and cannot hand over a misaligned view.

What is asserted:
  * forward: torch.equal with F.leaky_relu(x + b, slope) in fp32 on the CPU -- one correctly rounded add and one correctly
    rounded product per element, and the library is built with -ffp-contract=off, so nothing can differ;
  * backward: gin torch.equal with where(y > 0, g, g * slope);
  * moments: row (b C + c) chunks + j of [B][C chunks][2] holds the sums over elements [4096 j, 4096 (j + 1)) of plane (b, c),
    within 16 u sum|y| resp. 17 u sum y^2 of the float64 sums of the fp32 y (u = 2^-24: at most 16 values per thread in fp32,
    q by fma, double from the wave reduction on); every row written (NaN prefill); y bitwise the plain call's;
  * gbias, default mode (fp32 atomics, any order): inside gamma(B HW) sum|term|, and inside test_hip_parity.py's
    test_bias_leaky_relu bound (atol 1e-5 max(1, max|ref|) / 2, rtol 5e-6);
  * gbias, deterministic mode: |gbias - ref64| <= u |ref64| + B HW 2^-53 sum|term| (double accumulation, one rounding at the
    end), bitwise across two calls, for bias_grad_det_kernel<true> and <false>: the scalar form is reached at HW % 4 != 0 and,
    with HW % 4 == 0, through gout and y that start one float into their storage;
  * gbias = NULL: gin as with a gbias.
Every output buffer carries a NaN tail that must survive the call."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CHUNK = 4096
TAIL = 64
SHAPES = [(1, 1, 1), (3, 5, 15), (2, 3, 4221), (1, 2, 4160), (2, 2, 8192)]
SLOPES = [0.1, 0.25, 1.0, 0.0]


def gamma(n):
    return n * U / (1.0 - n * U)


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    return functional


def _inputs(shape, with_bias):
    """x, bias, gout on the CPU; a few pre-activations are exactly zero (the kink belongs to the slope branch)."""
    B, C, HW = shape
    gen = torch.Generator().manual_seed(1000 * C + HW)
    x = torch.randn(B, C, HW, generator=gen)
    bias = torch.randn(C, generator=gen) if with_bias else None
    g = torch.randn(B, C, HW, generator=gen)
    x[:, :, ::7] = 0.0 if bias is None else -bias.view(1, C, 1)
    return x, bias, g


def _guarded(shape, dtype=torch.float32, fill=float('nan'), lead=0):
    """A tensor of `shape` inside a NaN-filled buffer: `lead` elements before it, TAIL elements behind it."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((lead + n + TAIL,), fill, device='cuda', dtype=dtype)
    return buf, buf[lead:lead + n].view(*shape)


def _tail_untouched(buf, n, lead=0):
    return bool(torch.isnan(buf[lead + n:]).all()) and bool(torch.isnan(buf[:lead]).all())


def _forward(AF, x, bias, slope, inplace, mom=False):
    """(y, rows or None) from the C entry point; x, bias on the CPU."""
    B, C, HW = x.shape
    bc = None if bias is None else bias.cuda()
    if inplace:
        ybuf, y = _guarded(x.shape)
        y.copy_(x)
        xin = y
    else:
        xin = x.cuda()
        ybuf, y = _guarded(x.shape)
    rows = None
    if mom:
        n = AF._lib.load().arflow_bias_act_mom_rows(C, HW)
        assert n == C * -(-HW // CHUNK)
        mbuf, rows = _guarded((B, n, 2), torch.float64)
        AF._call('arflow_bias_act_fwd_mom', AF._p(xin), AF._p(bc), AF._p(y), AF._p(rows), B, C, HW, float(slope), AF._stream())
        torch.cuda.synchronize()
        assert _tail_untouched(mbuf, rows.numel())
    else:
        AF._call('arflow_bias_act_fwd', AF._p(xin), AF._p(bc), AF._p(y), B, C, HW, float(slope), AF._stream())
        torch.cuda.synchronize()
    assert _tail_untouched(ybuf, y.numel())
    return y.cpu(), (None if rows is None else rows.cpu())


def _forward_ref(x, bias, slope):
    return F.leaky_relu(x if bias is None else x + bias.view(1, -1, 1), slope)


def _backward(AF, g, y, slope, want_bias, lead=0):
    """(gin, gbias or None) from the C entry point; gout and y start `lead` floats into their storage."""
    B, C, HW = g.shape
    gbuf, gc = _guarded(g.shape, lead=lead)
    ybuf, yc = _guarded(g.shape, lead=lead)
    gc.copy_(g)
    yc.copy_(y)
    ibuf, gin = _guarded(g.shape)
    bbuf, gb = _guarded((C,))
    AF._call('arflow_bias_act_bwd', AF._p(gc), AF._p(yc), AF._p(gin), AF._p(gb if want_bias else None), B, C, HW, float(slope),
             AF._stream())
    torch.cuda.synchronize()
    assert _tail_untouched(ibuf, gin.numel()) and _tail_untouched(bbuf, C)
    if not want_bias:
        assert bool(torch.isnan(gb).all()), 'gbias = NULL, yet the buffer next to it was written'
    assert torch.equal(gc.cpu(), g) and torch.equal(yc.cpu(), y), 'the backward changed its inputs'
    return gin.cpu(), (gb.cpu() if want_bias else None)


def _backward_ref(g, y, slope):
    gin = torch.where(y > 0, g, g * slope)
    assert gin.dtype == torch.float32
    return gin, gin.double().sum((0, 2)), gin.double().abs().sum((0, 2))


@pytest.mark.parametrize('slope', SLOPES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_forward_is_the_fp32_expression_bit_for_bit(AF, shape, slope):
    for with_bias in (True, False):
        x, bias, _ = _inputs(shape, with_bias)
        ref = _forward_ref(x, bias, slope)
        assert int((ref == 0).sum()) > 0  # the fixture's exact zeros reach the kink
        for inplace in (False, True):
            y, _ = _forward(AF, x, bias, slope, inplace)
            assert torch.equal(y, ref), 'bias %s, in place %s: %d elements differ, max |diff| %.3e' % (
                with_bias, inplace, int((y != ref).sum()), float((y.double() - ref.double()).abs().max()))


@pytest.mark.parametrize('slope', SLOPES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_moment_rows_hold_each_chunk_of_each_plane(AF, shape, slope):
    B, C, HW = shape
    chunks = -(-HW // CHUNK)
    for with_bias in (True, False):
        x, bias, _ = _inputs(shape, with_bias)
        ref = _forward_ref(x, bias, slope)
        for inplace in (False, True):
            y, rows = _forward(AF, x, bias, slope, inplace, mom=True)
            assert torch.equal(y, ref), 'the moments call changes y (bias %s, in place %s)' % (with_bias, inplace)
            assert tuple(rows.shape) == (B, C * chunks, 2)
            assert bool(torch.isfinite(rows).all()), '%d row entries left unwritten' % int((~torch.isfinite(rows)).sum())
            y64 = ref.double()
            worst = [0.0, 0.0]
            for b in range(B):
                for c in range(C):
                    for j in range(chunks):
                        seg = y64[b, c, CHUNK * j:CHUNK * (j + 1)]
                        got = rows[b, c * chunks + j]
                        s, sa, q = float(seg.sum()), float(seg.abs().sum()), float((seg * seg).sum())
                        es, eq = abs(float(got[0]) - s), abs(float(got[1]) - q)
                        worst = [max(worst[0], es / (16 * U * sa) if sa else 0.0), max(worst[1], eq / (17 * U * q) if q else 0.0)]
                        assert es <= 16 * U * sa, 'sum of row (%d, %d, %d): %.9g vs %.9g, bound %.3e' % (b, c, j, float(got[0]), s, 16 * U * sa)
                        assert eq <= 17 * U * q, 'sum of squares of row (%d, %d, %d): %.9g vs %.9g, bound %.3e' % (
                            b, c, j, float(got[1]), q, 17 * U * q)
            print('moments %s slope %g bias %s in place %s: worst err / bound: sum %.3f, squares %.3f' % (
                shape, slope, with_bias, inplace, worst[0], worst[1]))


@pytest.mark.parametrize('slope', SLOPES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_backward_default_mode(AF, shape, slope):
    assert not AF.is_deterministic()
    B, C, HW = shape
    for with_bias in (True, False):
        x, bias, g = _inputs(shape, with_bias)
        y = _forward_ref(x, bias, slope)
        ref_gin, ref_gb, ref_abs = _backward_ref(g, y, slope)
        gin, gb = _backward(AF, g, y, slope, True)
        assert torch.equal(gin, ref_gin), '%d elements of gin differ' % int((gin != ref_gin).sum())
        err = (gb.double() - ref_gb).abs()
        any_order = gamma(B * HW) * ref_abs
        parity = 1e-5 * max(1.0, float(ref_gb.abs().max())) / 2 + 5e-6 * ref_gb.abs()
        print('gbias %s slope %g bias %s: worst err / any-order bound %.3f, / parity bound %.3f' % (
            shape, slope, with_bias, float((err / any_order.clamp_min(1e-300)).max()), float((err / parity).max())))
        assert bool((err <= any_order).all()), 'gbias outside gamma(B HW) sum|term|: err %s bound %s' % (err.tolist(), any_order.tolist())
        assert bool((err <= parity).all()), 'gbias outside the bound of test_bias_leaky_relu: err %s bound %s' % (err.tolist(), parity.tolist())
        gin0, none = _backward(AF, g, y, slope, False)
        assert none is None and torch.equal(gin0, ref_gin), 'gbias = NULL changes gin'


@pytest.mark.parametrize('lead', [0, 1], ids=['aligned', 'one_float_in'])
@pytest.mark.parametrize('slope', SLOPES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_backward_deterministic_mode(AF, shape, slope, lead):
    """lead = 1 with HW % 4 == 0 is bias_grad_det_kernel<false> on a shape the vector form would take; HW % 4 != 0 is the
    scalar form at either alignment."""
    B, C, HW = shape
    x, bias, g = _inputs(shape, True)
    y = _forward_ref(x, bias, slope)
    ref_gin, ref_gb, ref_abs = _backward_ref(g, y, slope)
    with AF.deterministic():
        gin, gb = _backward(AF, g, y, slope, True, lead)
        gin2, gb2 = _backward(AF, g, y, slope, True, lead)
        gin0, none = _backward(AF, g, y, slope, False, lead)
    assert not AF.is_deterministic()
    assert torch.equal(gin, ref_gin) and torch.equal(gin2, ref_gin), '%d elements of gin differ' % int((gin != ref_gin).sum())
    assert none is None and torch.equal(gin0, ref_gin), 'gbias = NULL changes gin'
    assert torch.equal(gb, gb2), 'deterministic gbias differs between two calls: %s vs %s' % (gb.tolist(), gb2.tolist())
    err = (gb.double() - ref_gb).abs()
    bound = U * ref_gb.abs() + B * HW * 2.0 ** -53 * ref_abs
    print('det gbias %s slope %g lead %d: worst err / bound %.3f' % (shape, slope, lead, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), 'deterministic gbias: err %s bound %s' % (err.tolist(), bound.tolist())
