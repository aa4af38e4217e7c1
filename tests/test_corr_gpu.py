"""GPU: the cost-volume kernels (csrc/corr.hip, csrc/corr_v2.hpp) and the feature normalisation (csrc/featnorm.hip) PER
ELEMENT against the float64 restatements of tests/corr_ref.py, on every launch path: the three forward kernels of the fast
path (four channel groups, ring of 4, ring of 2) on both sides of their thresholds, its backward with every channel split
(even, uneven, cut back by the workgroup limit), both rings, the three activation modes and the three gradient requests,
the general path at every strip width and workgroup size in fp32 (bf16 storage at the middle one), the generic d > 4
kernels below and above their grid cap, and the normalisation's one-launch, two-launch and capped-grid forms with the
float4 and the scalar loops, centred and far off centre.

Every comparison is |got - ref64| <= bound per element with the bounds DERIVED in the docstring of tests/corr_ref.py
(u = 2^-24) and checked without a GPU in tests/test_corr_ref_cpu.py: the fp32 oracle sits inside each, every mutation of the
reference leaves by > 100x, every branch named here is reached by the shape lists.  No element is left out, no bound was
taken from what the kernels give.  Outputs of the raw entry points are handed over full of NaN and must come back finite;
the inputs must come back untouched; two runs must agree bit for bit (no kernel here has an atomic)."""
import pytest
import torch

from tests import corr_ref as R

pytestmark = pytest.mark.gpu
SITES = {}
NAN = float('nan')
ident = lambda v: str(v).replace(' ', '')  # noqa: E731


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    torch.set_num_threads(16)
    return functional


@pytest.fixture(scope='module', autouse=True)
def margin_summary():
    yield
    for site in sorted(SITES):
        print('MARGIN %-44s worst err/bound %.4f' % (site, SITES[site]))


def cu(t):
    return None if t is None else t.detach().cuda().contiguous()


def nan_like(shape):
    return torch.full(tuple(shape), NAN, device='cuda')


def assert_within(got, ref, bound, site, tag):
    """elementwise |got - ref| <= bound on finite values; prints the worst err / bound and keeps the worst per site"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, '%s | %s: shape %s vs %s' % (site, tag, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), '%s | %s: %d elements left unwritten or not finite' % (
        site, tag, int((~torch.isfinite(got)).sum()))
    err = (got - ref.double()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    w = R.worst(err, bound)
    SITES[site] = max(SITES.get(site, 0.0), w)
    print('%s | %s: max err %.3e, worst err/bound %.4f' % (site, tag, float(err.max()) if err.numel() else 0.0, w))
    assert bool((err <= bound).all()), '%s | %s: %d elements out of bound, worst err/bound %.3f' % (
        site, tag, int((~(err <= bound)).sum()), w)


def same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


# ---- raw entry points ------------------------------------------------------------------------------------------------
def raw_corr_fwd(AF, x1, x2, d, slope):
    """arflow_corr_fwd into a NaN-filled volume (x1, x2 on the GPU), without sign words"""
    B, C, H, W = x1.shape
    n = 2 * d + 1
    out = nan_like((B, n * n, H, W))
    AF._call('arflow_corr_fwd', AF._p(x1), AF._p(x2), AF._p(out), None, B, C, H, W, d, float(slope), AF._stream())
    return out


def raw_corr_bwd(AF, go, fout, sign, x1, x2, d, slope, want1=True, want2=True):
    """arflow_corr_bwd into NaN-filled gradients -> (gx1 or None, gx2 or None)"""
    B, C, H, W = x1.shape
    g1 = nan_like(x1.shape) if want1 else None
    g2 = nan_like(x2.shape) if want2 else None
    AF._call('arflow_corr_bwd', AF._p(go), AF._p(fout), AF._p(sign), AF._p(x1), AF._p(x2), AF._p(g1), AF._p(g2), B, C, H, W, d,
             float(slope), AF._stream())
    return g1, g2


def corr_case(shape, d, slope, bf16=False):
    """inputs, forward reference, masked output gradient and gradient reference of one recipe"""
    x1, x2, go = R.corr_inputs(*shape, d)
    if bf16:
        x1, x2 = R.bf16_round(x1), R.bf16_round(x2)
    fwd = R.corr_ref(x1, x2, d, slope)
    go = go * (~R.kink_mask(fwd)).float()
    return x1, x2, go, fwd, R.corr_grads_ref(go, fwd.pre, x1, x2, d, slope)


def check_forward(AF, shape, d, slopes, site):
    x1, x2, _ = R.corr_inputs(*shape, d)
    a, b = cu(x1), cu(x2)
    for slope in slopes:
        fwd = R.corr_ref(x1, x2, d, slope)
        out = raw_corr_fwd(AF, a, b, d, slope)
        assert_within(out, fwd.out, fwd.bound_out, site, '%s d=%d slope=%g' % (shape, d, slope))
        again = raw_corr_fwd(AF, a, b, d, slope)
        same_bits(out, again, 'two forward runs differ')
    assert torch.equal(a.cpu(), x1) and torch.equal(b.cpu(), x2), 'the forward wrote to its inputs'


# ---- fast path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,branch', R.FAST_FWD, ids=ident)
def test_fast_forward(AF, shape, branch):
    B, C, H, W = shape
    assert R.fast_eligible(C, W, 4) and R.fast_fwd_branch(B, C, H, W) == branch
    check_forward(AF, shape, 4, R.SLOPES, 'corr fast fwd ' + branch)


@pytest.mark.parametrize('shape,req,act', R.FAST_BWD, ids=ident)
def test_fast_backward(AF, shape, req, act):
    B, C, H, W = shape
    want1, want2 = req in ('both', 'gx1'), req in ('both', 'gx2')
    nm = int(want1) + int(want2)
    slope = 1.0 if act == 'none' else 0.1
    x1, x2, go, fwd, gr = corr_case(shape, 4, slope)
    site = 'corr fast bwd nsplit %d ring %d act %s' % (R.fast_bwd_nsplit(B, C, H, W, nm), R.fast_bwd_ring(B, H, W, nm), act)
    tag = '%s %s' % (shape, req)
    a, b, g = cu(x1), cu(x2), cu(go)

    def run():
        if act == 'sign':  # the autograd function: sign words from the forward, requests from requires_grad
            p, q = a.clone().requires_grad_(want1), b.clone().requires_grad_(want2)
            out = AF.correlation(p, q, 4, negative_slope=slope)
            out.backward(g)
            return out.detach(), p.grad, q.grad
        out = raw_corr_fwd(AF, a, b, 4, slope)
        g1, g2 = raw_corr_bwd(AF, g, out if act == 'out' else None, None, a, b, 4, slope, want1, want2)
        return out, g1, g2

    out, g1, g2 = run()
    assert_within(out, fwd.out, fwd.bound_out, 'corr fast fwd (backward cases)', tag)
    assert (g1 is None) == (not want1) and (g2 is None) == (not want2)
    if want1:
        assert_within(g1, gr.gx1, gr.bound1, site + ' gx1', tag)
    if want2:
        assert_within(g2, gr.gx2, gr.bound2, site + ' gx2', tag)
    _, h1, h2 = run()
    for u, v in ((g1, h1), (g2, h2)):
        if u is not None:
            same_bits(u, v, 'two backward runs differ')
    assert torch.equal(a.cpu(), x1) and torch.equal(b.cpu(), x2) and torch.equal(g.cpu(), go), 'an input was written to'


# ---- general and generic paths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,d,bwd', R.GENERAL, ids=ident)
def test_general_and_generic(AF, shape, d, bwd):
    B, C, H, W = shape
    path = R.corr_path(B, C, H, W, d)
    assert path != 'fast'
    n = 2 * d + 1
    if path == 'general':
        fsite = 'corr general fwd strip %d' % R.general_fwd_strip(B, H, W)
        bsite = 'corr general bwd %d threads' % R.general_bwd_threads(B, H, W)
    else:
        fsite = 'corr generic fwd' + (' (capped grid)' if R.generic_capped(B * n * n * H * W) else '')
        bsite = 'corr generic bwd'
    if not bwd:  # the 17 M element volume: one slope, which takes both branches of the select
        check_forward(AF, shape, d, (0.1,), fsite)
        return
    check_forward(AF, shape, d, R.SLOPES, fsite)
    for slope in R.SLOPES:
        x1, x2, go, fwd, gr = corr_case(shape, d, slope)
        a, b, g = cu(x1), cu(x2), cu(go)
        out = raw_corr_fwd(AF, a, b, d, slope)
        tag = '%s d=%d slope=%g' % (shape, d, slope)
        g1, g2 = raw_corr_bwd(AF, g, out if slope != 1.0 else None, None, a, b, d, slope)
        assert_within(g1, gr.gx1, gr.bound1, bsite + ' gx1', tag)
        assert_within(g2, gr.gx2, gr.bound2, bsite + ' gx2', tag)
        h1, _ = raw_corr_bwd(AF, g, out if slope != 1.0 else None, None, a, b, d, slope, True, False)
        _, h2 = raw_corr_bwd(AF, g, out if slope != 1.0 else None, None, a, b, d, slope, False, True)
        same_bits(g1, h1, 'gx1 alone differs from gx1 of the pair')
        same_bits(g2, h2, 'gx2 alone differs from gx2 of the pair')
        assert torch.equal(a.cpu(), x1) and torch.equal(b.cpu(), x2) and torch.equal(g.cpu(), go), 'an input was written to'


def test_bf16_storage_middle_strip(AF):
    B, C, H, W = R.BF16
    assert R.general_fwd_strip(B, H, W) == 4 and R.general_bwd_threads(B, H, W) == 128
    x1, x2, go, fwd, gr = corr_case(R.BF16, 4, 0.1, bf16=True)
    raw1, raw2, _ = R.corr_inputs(*R.BF16, 4)  # the function rounds the fp32 inputs itself
    a, b = cu(raw1).requires_grad_(True), cu(raw2).requires_grad_(True)
    out = AF.correlation(a, b, 4, negative_slope=0.1, storage='bf16')
    out.backward(cu(go))
    tag = str(R.BF16)
    assert_within(out, fwd.out, fwd.bound_out, 'corr bf16 fwd strip 4', tag)
    assert_within(a.grad, gr.gx1, gr.bound1, 'corr bf16 bwd 128 threads gx1', tag)
    assert_within(b.grad, gr.gx2, gr.bound2, 'corr bf16 bwd 128 threads gx2', tag)


# ---- feature normalisation -------------------------------------------------------------------------------------------
def raw_featnorm_fwd(AF, x1, x2, mode):
    B, n = x1.shape
    y1, y2, stats = nan_like((B, n)), nan_like((B, n)), nan_like((B, 4))
    acc = AF._featnorm_acc(B, x1.device).fill_(NAN)
    AF._call('arflow_featnorm_fwd', AF._p(x1), AF._p(x2), AF._p(y1), AF._p(y2), AF._p(acc), AF._p(stats), B, n, AF.FEATNORM[mode],
             AF._stream())
    return y1, y2, stats


def raw_featnorm_bwd(AF, g1, g2, x1, x2, stats, mode, want1=True, want2=True):
    B, n = x1.shape
    d1 = nan_like((B, n)) if want1 else None
    d2 = nan_like((B, n)) if want2 else None
    acc = AF._featnorm_acc(B, x1.device).fill_(NAN)
    AF._call('arflow_featnorm_bwd', AF._p(g1), AF._p(g2), AF._p(x1), AF._p(x2), AF._p(stats), AF._p(acc), AF._p(d1), AF._p(d2), B, n,
             AF.FEATNORM[mode], AF._stream())
    return d1, d2


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('recipe', R.FEAT, ids=ident)
def test_featnorm(AF, recipe, mode):
    B, n, offset, spread = recipe
    x1, x2, g1, g2 = R.feat_inputs(*recipe)
    fwd = R.featnorm_ref(x1, x2, mode)
    bwd = R.featnorm_grads_ref(g1, g2, x1, x2, mode)
    kind = 'centred' if offset == 0 else 'offset %g spread %g' % (offset, spread)
    site = 'featnorm %s %s %s' % (R.feat_path(B, n), mode, kind)
    tag = '(%d, %d) kappa %.3g' % (B, n, float(fwd.kappa.max()))
    a, b, ga, gb = cu(x1), cu(x2), cu(g1), cu(g2)
    y1, y2, stats = raw_featnorm_fwd(AF, a, b, mode)
    assert_within(y1, fwd.y1, fwd.bound1, site + ' y', tag + ' y1')
    assert_within(y2, fwd.y2, fwd.bound2, site + ' y', tag + ' y2')
    assert_within(stats, fwd.stats, fwd.stats_bound, site + ' stats', tag)
    for k, name in enumerate(('m1', 'm2', 'mu', 'sd')):
        print('%s | %s: %s err %.3e (bound %.3e)' % (site, tag, name, float((stats[:, k].cpu().double() - fwd.stats[:, k]).abs().max()),
                                                    float(fwd.stats_bound[:, k].max())))
    d1, d2 = raw_featnorm_bwd(AF, ga, gb, a, b, stats, mode)
    assert_within(d1, bwd.d1, bwd.bound1, site + ' dx', tag + ' d1')
    assert_within(d2, bwd.d2, bwd.bound2, site + ' dx', tag + ' d2')
    e1, none2 = raw_featnorm_bwd(AF, ga, gb, a, b, stats, mode, True, False)
    none1, e2 = raw_featnorm_bwd(AF, ga, gb, a, b, stats, mode, False, True)
    assert none1 is None and none2 is None
    same_bits(d1, e1, 'gx1 alone differs from gx1 of the pair')
    same_bits(d2, e2, 'gx2 alone differs from gx2 of the pair')
    z1, z2, zstats = raw_featnorm_fwd(AF, a, b, mode)
    same_bits(y1, z1, 'two forward runs differ')
    same_bits(y2, z2, 'two forward runs differ')
    same_bits(stats, zstats, 'two forward runs differ')
    for dev, host in ((a, x1), (b, x2), (ga, g1), (gb, g2)):
        assert torch.equal(dev.cpu(), host), 'an input was written to'
