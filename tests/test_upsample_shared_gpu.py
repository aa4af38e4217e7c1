"""GPU: the entry points of csrc/upsample.hip agree bit for bit wherever their definitions coincide.

Every one of them evaluates out[b,c] = s_c * resize(in[b,c] + b_c) with the same source indices and weights (up_source), the
same blend (up_blend) and, in the adjoint, the same fused multiply-add chain over ascending rows and columns; the adjoints
differ only in how many zero-weight fine pixels a coarse cell visits.  So with a zero bias, equal scales and finite inputs
without zeros (`a + 0.f` is then `a`, and a zero-weight tap adds nothing) two entry points that describe the same resize
return the same bits, forward and adjoint.  A later edit to one instantiation would break exactly that.

Planes: 1 x 1 (every tap clamped), 2 x 3 (under one adjoint window), 5 x 7 (odd: the scalar path), 9 x 17 (one cell past
the tail's 8 x 16 tile; 2 x 17 and 4 x 17 columns: the edge of the float4 path).  B = 2.

flow_upsample(., 4, align_corners=False) -- up_fwd_kernel at f = 4 without alignment and up_run_bwd_kernel<false> at f = 4, an
instantiation no other entry point uses -- has no sibling to agree with: it is held per pixel to the float64 restatement
tests/gauss_pyr_ref.py up_half (weights that are multiples of 1/8: exact, no coordinate term), forward within 6 EPS 4 sum w |a|
(the out_up rule of tests/test_out_up_gpu.py) and adjoint within bwd_roundings(4) EPS 4 sum w |g|; that a plain fp32 evaluation
sits inside both and that the align_corners=True weights fall outside is checked without a GPU in
tests/test_generic_ref_cpu.py."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

PLANES = [(1, 1), (2, 3), (5, 7), (9, 17)]
B = 2
BIAS = 0.75


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    return functional


def seeded_host(plane, C, scale=1):
    """A [B,C,scale h,scale w] tensor of seeded normal values: finite, and none of them zero."""
    h, w = plane
    g = torch.Generator().manual_seed(7000 + 100 * h + 10 * w + C + scale)
    t = torch.randn(B, C, scale * h, scale * w, generator=g)
    assert bool((t != 0).all())
    return t


def seeded(plane, C, scale=1):
    """... on the device"""
    return seeded_host(plane, C, scale).cuda()


def fwd_and_adjoint(fn, x, gout):
    x = x.clone().requires_grad_(True)
    y = fn(x)
    return y.detach(), torch.autograd.grad(y, x, gout)[0]


@pytest.mark.parametrize('plane', PLANES, ids=str)
def test_flow_upsample_is_out_upsample_of_two_flow_channels(AF, plane):
    f, g = seeded(plane, 2), seeded(plane, 2, 2)
    ya, ga = fwd_and_adjoint(lambda t: AF.flow_upsample(t, 2, False), f, g)
    yb, gb = fwd_and_adjoint(lambda t: AF.out_upsample(t, 2, 0, 0.0), f, g)
    assert torch.equal(ya, yb)
    assert torch.equal(ga, gb)


@pytest.mark.parametrize('factor', [2, 4])
@pytest.mark.parametrize('plane', PLANES, ids=str)
def test_flow_upsample_aligned_is_prob_upsample_of_two_flow_channels(AF, plane, factor):
    f, g = seeded(plane, 2), seeded(plane, 2, factor)
    ya, ga = fwd_and_adjoint(lambda t: AF.flow_upsample(t, factor, True), f, g)
    yb, gb = fwd_and_adjoint(lambda t: AF.prob_upsample(t, factor, 2, 0, 0.0), f, g)
    assert torch.equal(ya, yb)
    assert torch.equal(ga, gb)


@pytest.mark.parametrize('align', [0, 1])
@pytest.mark.parametrize('plane', PLANES, ids=str)
def test_level_adjoint_is_flow_upsample_adjoint(plane, align):
    from arflow_amd import _lib
    lib = _lib.load()
    h, w = plane
    g = seeded(plane, 2, 2)
    ga, gb = torch.empty(B, 2, h, w, device='cuda'), torch.empty(B, 2, h, w, device='cuda')
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.arflow_up2_bwd(g.data_ptr(), ga.data_ptr(), B, 2 * h, 2 * w, align, s) == 0
    assert lib.arflow_flow_up_bwd(g.data_ptr(), gb.data_ptr(), B, h, w, 2, align, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(ga, gb)


@pytest.mark.parametrize('plane', PLANES, ids=str)
def test_channel_rule_does_not_depend_on_the_neighbours(AF, plane):
    """(flow, log_diag, rest) in one call against each group in a call of its own."""
    x, g = seeded(plane, 6), seeded(plane, 6, 2)
    y, gx = fwd_and_adjoint(lambda t: AF.out_upsample(t, 2, 2, BIAS), x, g)
    for lo, (n_flow, n_diag) in ((0, (2, 0)), (2, (0, 2)), (4, (0, 0))):
        ys, gs = fwd_and_adjoint(lambda t: AF.out_upsample(t, n_flow, n_diag, BIAS), x[:, lo:lo + 2].contiguous(),
                                 g[:, lo:lo + 2].contiguous())
        assert torch.equal(y[:, lo:lo + 2], ys)
        assert torch.equal(gx[:, lo:lo + 2], gs)


@pytest.mark.parametrize('plane', PLANES, ids=str)
def test_flow_upsample_x4_half_pixel_per_pixel(AF, plane):
    """No element is left out; both outputs are handed over as fresh tensors and must come back finite."""
    from tests import gauss_pyr_ref as R
    x, g = seeded_host(plane, 2), seeded_host(plane, 2, 4)
    ref, bound, gref, gbound = R.flow_up_half_ref(x, g, 4)
    y, gx = fwd_and_adjoint(lambda t: AF.flow_upsample(t, 4, False), x.cuda(), g.cuda())
    for what, got, want, lim in (('forward', y, ref, bound), ('adjoint', gx, gref, gbound)):
        got = got.cpu().double()
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), what
        err = (got - want).abs()
        print('flow_upsample x4 half-pixel %s %s: worst err/bound %.4f' % (plane, what, float((err / lim).max())))
        assert bool((err <= lim).all()), '%s %s: %d elements out of bound' % (plane, what, int((~(err <= lim)).sum()))
