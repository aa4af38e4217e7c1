"""GPU: the three kernel pairs of csrc/generic.hip that no shipped config reaches -- arflow_warp_nearest_fwd / _bwd,
arflow_warp_bicubic_fwd / _bwd, arflow_corr_general_fwd / _bwd -- PER ELEMENT against the float64 restatements of
tests/generic_ref.py, with the bounds derived in that file's docstring (u = 2^-24) and checked without a GPU in
tests/test_generic_ref_cpu.py.

Warps (one lane per pixel, grid (ceil(W / 256), H, B)): every field (noise, stretch, exact half-integer ties, integer / edge /
+-1e30 coordinates, everything far outside) x both paddings x both align flags on 9 x 13; source extents different from the
flow's under all three norms; 257 and 256 columns (a second workgroup with one lane, exactly one workgroup); one-pixel source
axes; one-pixel flow axes under norm UFLOW (norm ARFLOW divides by n_flow - 1 = 0 there, as the reference does: left out);
every pixel onto one cell; the flow out of channels 2:4 of a wider tensor.  NaN flows are left out.
Correlation: the parameter sets of generic_ref.CORR_CASES; the grid-stride loops' cap of 65535 * 16 workgroups needs more than
2.6e8 outputs and is not exercised.

The sampling coordinate is part of the operations' definition (fp32, restated in tests/warp_ref.py), so the rounding to the
nearest index, floor, the border clip and the tap validity are exact: no element is left out of any comparison, and where the
bound is 0 -- the whole nearest forward, integer coordinates, no tap inside the source, a cell nothing or one pixel lands
on, an output that reads zero padding only -- the result must be exact.  Outputs of the raw entry points are handed over
full of NaN and must come back finite; inputs must come back untouched."""
import pytest
import torch

from tests import generic_ref as R

pytestmark = pytest.mark.gpu
SITES = {}
NAN = float('nan')
ident = lambda c: c.name.replace(' ', '_')  # noqa: E731
ALL_WARP_CASES = R.WARP_CASES + [R.STRIDED_CASE]


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


@pytest.fixture(autouse=True)
def mode_off_afterwards():
    from arflow_amd import functional
    assert functional.is_deterministic() is False, 'a test before this one left deterministic mode on'
    yield
    left_on = functional.is_deterministic()
    functional.set_deterministic(False)
    assert not left_on, 'this test left deterministic mode on'


def cu(t):
    return t.detach().cuda().contiguous()


def nan_like(shape):
    return torch.full(tuple(shape), NAN, device='cuda')


def assert_within(got, ref, bound, site, tag):
    """elementwise |got - ref| <= bound, every element finite; prints the worst err / bound and keeps the worst per site"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, '%s | %s: shape %s vs %s' % (site, tag, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), '%s | %s: %d elements left unwritten or not finite' % (
        site, tag, int((~torch.isfinite(got)).sum()))
    err = (got - ref).abs()
    w = R.worst(err, bound)
    SITES[site] = max(SITES.get(site, 0.0), w)
    print('%s | %s: max err %.3e, worst err/bound %.4f' % (site, tag, float(err.max()), w))
    assert bool((err <= bound).all()), '%s | %s: %d elements out of bound, worst err/bound %.3f' % (
        site, tag, int((~(err <= bound)).sum()), w)


def within(got, iv, site, tag):
    assert_within(got, iv.v, iv.e, site, tag)


def same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


# ---- the warps: raw entry points ---------------------------------------------------------------------------------------
def flow_on_device(case, flow):
    """-> (flow tensor or view, batch stride, the tensor that owns the memory, its host copy)"""
    if case.name != R.STRIDED_CASE.name:
        f = cu(flow)
        return f, 2 * case.H * case.W, f, flow
    wide = torch.full((case.B, 4, case.H, case.W), 777.0)   # the other half would throw every pixel out of the image
    wide[:, 2:4] = flow
    wide_dev = cu(wide)
    view = wide_dev[:, 2:4]
    assert view.data_ptr() == wide_dev.data_ptr() + 4 * 2 * case.H * case.W
    return view, 4 * case.H * case.W, wide_dev, wide


def dims(case, fbs):
    return (case.B, case.C, case.Hs, case.Ws, case.H, case.W, fbs, R.PAD[case.pad], int(case.align), R.NORMS[case.norm])


def raw_fwd(AF, kind, case, s, f, fbs):
    out = nan_like((case.B, case.C, case.H, case.W))
    AF._call('arflow_warp_%s_fwd' % kind, AF._p(s), f.data_ptr(), AF._p(out), *dims(case, fbs), AF._stream())
    return out


def raw_nearest_bwd(AF, case, g, f, fbs):
    gsrc = nan_like((case.B, case.C, case.Hs, case.Ws))
    AF._call('arflow_warp_nearest_bwd', AF._p(g), f.data_ptr(), AF._p(gsrc), *dims(case, fbs), AF._stream())
    return gsrc


def raw_bicubic_bwd(AF, case, g, s, f, fbs, want_src, want_flow):
    gsrc = nan_like((case.B, case.C, case.Hs, case.Ws)) if want_src else None
    gflow = nan_like((case.B, 2, case.H, case.W)) if want_flow else None
    AF._call('arflow_warp_bicubic_bwd', AF._p(g), AF._p(s), f.data_ptr(), AF._p(gsrc), AF._p(gflow), *dims(case, fbs),
             AF._stream())
    return gsrc, gflow


@pytest.mark.parametrize('case', ALL_WARP_CASES, ids=ident)
def test_nearest_warp(AF, case):
    src, flow, gout, ref, _ = R.warp_case(case)
    s, g = cu(src), cu(gout)
    f, fbs, owner, host = flow_on_device(case, flow)
    out = raw_fwd(AF, 'nearest', case, s, f, fbs)
    within(out, ref.out, 'nearest fwd', case.name)
    assert torch.equal(out.cpu().double(), ref.out.v), '%s: the nearest forward is a copy: %d elements differ' % (
        case.name, int((out.cpu().double() != ref.out.v).sum()))
    gsrc = raw_nearest_bwd(AF, case, g, f, fbs)
    within(gsrc, ref.gsrc, 'nearest bwd gsrc', case.name)
    assert torch.equal(s.cpu(), src) and torch.equal(g.cpu(), gout) and torch.equal(owner.cpu(), host), 'an input was written to'


@pytest.mark.parametrize('case', ALL_WARP_CASES, ids=ident)
def test_bicubic_warp(AF, case):
    src, flow, gout, _, ref = R.warp_case(case)
    s, g = cu(src), cu(gout)
    f, fbs, owner, host = flow_on_device(case, flow)
    out = raw_fwd(AF, 'bicubic', case, s, f, fbs)
    within(out, ref.out, 'bicubic fwd', case.name)
    same_bits(out, raw_fwd(AF, 'bicubic', case, s, f, fbs), '%s: two forward runs differ' % case.name)
    gsrc, gflow = raw_bicubic_bwd(AF, case, g, s, f, fbs, True, True)
    within(gsrc, ref.gsrc, 'bicubic bwd gsrc', case.name + ' both')
    within(gflow, ref.gflow, 'bicubic bwd gflow', case.name + ' both')
    # either gradient alone (the other pointer null)
    none, gflow1 = raw_bicubic_bwd(AF, case, g, s, f, fbs, False, True)
    assert none is None
    same_bits(gflow, gflow1, '%s: gflow alone differs from the joint call' % case.name)
    same_bits(gflow1, raw_bicubic_bwd(AF, case, g, s, f, fbs, False, True)[1], '%s: two gflow runs differ' % case.name)
    gsrc1, none = raw_bicubic_bwd(AF, case, g, s, f, fbs, True, False)
    assert none is None
    within(gsrc1, ref.gsrc, 'bicubic bwd gsrc', case.name + ' alone')
    if float(ref.nq.max()) <= 1:   # one term per cell: no order to differ in
        same_bits(gsrc, gsrc1, '%s: gsrc alone differs from the joint call' % case.name)
    # deterministic mode: the forward and the gflow-only backward are the default mode's, bit for bit
    with AF.deterministic():
        same_bits(out, raw_fwd(AF, 'bicubic', case, s, f, fbs), '%s: deterministic forward differs' % case.name)
        same_bits(gflow, raw_bicubic_bwd(AF, case, g, s, f, fbs, False, True)[1], '%s: deterministic gflow differs' % case.name)
    assert torch.equal(s.cpu(), src) and torch.equal(g.cpu(), gout) and torch.equal(owner.cpu(), host), 'an input was written to'


# ---- the warps: autograd nodes and flow_warp(mode=...) -------------------------------------------------------------------
NODE_CASES = [R.WARP_BY_NAME[n] for n in ('half border align=False', '7x12->11x10 noise uflow border align=True',
                                          '7x12->4x17 noise abs zeros', 'strided')]


@pytest.mark.parametrize('case', NODE_CASES, ids=ident)
def test_autograd_nodes(AF, case):
    src, flow, gout, near, cub = R.warp_case(case)
    f, fbs, owner, host = flow_on_device(case, flow)
    for kind, fn, ref in (('nearest', AF.warp_nearest, near), ('bicubic', AF.warp_bicubic, cub)):
        s, fl = cu(src).requires_grad_(True), f.detach().requires_grad_(True)
        out = fn(s, fl, pad=case.pad, align_corners=case.align, norm=R.NORMS[case.norm])
        within(out, ref.out, 'autograd %s fwd' % kind, case.name)
        gs, gf = torch.autograd.grad(out, [s, fl], cu(gout))
        within(gs, ref.gsrc, 'autograd %s gsrc' % kind, case.name)
        if kind == 'nearest':
            assert gf is not None and tuple(gf.shape) == tuple(flow.shape) and bool((gf == 0).all()), \
                'the nearest warp returns a zero flow gradient, not None'
            assert torch.equal(out.detach().cpu().double(), ref.out.v)
        else:
            within(gf, ref.gflow, 'autograd bicubic gflow', case.name)
    assert torch.equal(owner.cpu(), host)


@pytest.mark.parametrize('case', [R.WARP_BY_NAME['half zeros align=True'], R.WARP_BY_NAME['noise border align=False']], ids=ident)
def test_flow_warp_modes(AF, case):
    """warp_utils.flow_warp(mode='nearest' | 'bicubic'): norm ARFLOW, padding and align flag passed through"""
    from arflow_amd import warp_utils
    src, flow, gout, near, cub = R.warp_case(case)
    assert case.norm == 'arflow'
    for mode, ref in (('nearest', near), ('bicubic', cub)):
        s, fl = cu(src).requires_grad_(True), cu(flow).requires_grad_(True)
        out = warp_utils.flow_warp(s, fl, pad=case.pad, mode=mode, align_corners=case.align)
        within(out, ref.out, 'flow_warp %s fwd' % mode, case.name)
        gs, gf = torch.autograd.grad(out, [s, fl], cu(gout))
        within(gs, ref.gsrc, 'flow_warp %s gsrc' % mode, case.name)
        if mode == 'nearest':
            assert gf is not None and bool((gf == 0).all())
        else:
            within(gf, ref.gflow, 'flow_warp bicubic gflow', case.name)


# ---- the general correlation -----------------------------------------------------------------------------------------------
def raw_corr_fwd(AF, case, a, b, shape):
    out = nan_like(shape)
    AF._call('arflow_corr_general_fwd', AF._p(a), AF._p(b), AF._p(out), case.B, case.C, case.H, case.W, *case.cfg, AF._stream())
    return out


def raw_corr_bwd(AF, case, g, a, b, want1, want2):
    g1 = nan_like(a.shape) if want1 else None
    g2 = nan_like(a.shape) if want2 else None
    AF._call('arflow_corr_general_bwd', AF._p(g), AF._p(a), AF._p(b), AF._p(g1), AF._p(g2), case.B, case.C, case.H, case.W,
             *case.cfg, AF._stream())
    return g1, g2


@pytest.mark.parametrize('case', R.CORR_CASES, ids=ident)
def test_general_correlation(AF, case):
    x1, x2, gout, ref = R.corr_case(case)
    a, b, g = cu(x1), cu(x2), cu(gout)
    out = raw_corr_fwd(AF, case, a, b, ref.out.v.shape)
    within(out, ref.out, 'corr general fwd', case.name)
    same_bits(out, raw_corr_fwd(AF, case, a, b, ref.out.v.shape), '%s: two forward runs differ' % case.name)
    g1, g2 = raw_corr_bwd(AF, case, g, a, b, True, True)
    within(g1, ref.gx1, 'corr general bwd gx1', case.name)
    within(g2, ref.gx2, 'corr general bwd gx2', case.name)
    r1, r2 = raw_corr_bwd(AF, case, g, a, b, True, True)
    same_bits(g1, r1, '%s: two gx1 runs differ' % case.name)
    same_bits(g2, r2, '%s: two gx2 runs differ' % case.name)
    o1, none = raw_corr_bwd(AF, case, g, a, b, True, False)
    assert none is None
    same_bits(g1, o1, '%s: gx1 alone differs from the joint call' % case.name)
    none, o2 = raw_corr_bwd(AF, case, g, a, b, False, True)
    assert none is None
    same_bits(g2, o2, '%s: gx2 alone differs from the joint call' % case.name)
    assert torch.equal(a.cpu(), x1) and torch.equal(b.cpu(), x2) and torch.equal(g.cpu(), gout), 'an input was written to'


@pytest.mark.parametrize('case', [c for c in R.CORR_CASES if c.cfg == R.CORR_DEFAULT], ids=ident)
def test_default_parameters_run_the_tuned_kernels_inside_the_same_bound(AF, case):
    """Correlation(4, 1, 4, 1, 1) is AF.correlation (the tuned kernels of csrc/corr.hip): the two float64 restatements are
    one function there, the tuned kernels lie inside THEIR bounds of tests/corr_ref.py around it ((C + 3) u S: they scale by
    the rounded 1 / C; (n^2 + 4) u A) and the general kernels, through their autograd node, inside the tighter ones of
    tests/generic_ref.py -- so the two kernel families agree within the sum of both."""
    from tests import corr_ref as CR
    x1, x2, gout, ref = R.corr_case(case)
    d = case.cfg[2]
    tf = CR.corr_ref(x1, x2, d)
    tg = CR.corr_grads_ref(gout, tf.pre, x1, x2, d)
    for mine, theirs in ((ref.out.v, tf.pre), (ref.gx1.v, tg.gx1), (ref.gx2.v, tg.gx2)):
        assert float((mine - theirs).abs().max()) <= 1e-12
    assert bool((ref.out.e <= tf.bound_pre).all()) and bool((ref.gx1.e <= tg.bound1).all())
    a, b = cu(x1).requires_grad_(True), cu(x2).requires_grad_(True)
    out = AF.correlation(a, b, d)
    assert_within(out, ref.out.v, tf.bound_pre, 'corr default tuned fwd', case.name)
    g1, g2 = torch.autograd.grad(out, [a, b], cu(gout))
    assert_within(g1, ref.gx1.v, tg.bound1, 'corr default tuned gx1', case.name)
    assert_within(g2, ref.gx2.v, tg.bound2, 'corr default tuned gx2', case.name)
    a, b = cu(x1).requires_grad_(True), cu(x2).requires_grad_(True)
    out = AF.correlation_general(a, b, *case.cfg)
    within(out, ref.out, 'corr default general fwd', case.name)
    g1, g2 = torch.autograd.grad(out, [a, b], cu(gout))
    within(g1, ref.gx1, 'corr default general gx1', case.name)
    within(g2, ref.gx2, 'corr default general gx2', case.name)


def test_correlation_module_routes_other_parameters_to_the_general_kernels(AF):
    from arflow_amd.correlation import Correlation
    case = next(c for c in R.CORR_CASES if c.cfg == (3, 3, 2, 2, 2))
    x1, x2, gout, ref = R.corr_case(case)
    pad, K, md, s1, s2 = case.cfg
    mod = Correlation(md, pad_size=pad, kernel_size=K, stride1=s1, stride2=s2)
    assert mod.general == case.cfg and mod.output_dim ** 2 == ref.out.v.shape[1]
    assert Correlation(4, pad_size=4, kernel_size=1, stride1=1, stride2=1).general is None, 'the default set is the tuned path'
    a = cu(x1).requires_grad_(True)
    for want in ((True, False), (False, True)):   # autograd asks for one gradient alone
        b = cu(x2).requires_grad_(True)
        out = mod(a, b)
        within(out, ref.out, 'corr general node fwd', case.name)
        (gr,) = torch.autograd.grad(out, [a if want[0] else b], cu(gout))
        within(gr, ref.gx1 if want[0] else ref.gx2, 'corr general node %s' % ('gx1' if want[0] else 'gx2'), case.name)
