"""GPU: the penalised entry points of DESIGN.md section 45 PER PIXEL against the float64 restatement of
tests/elbo_penalty_ref.py (bounds derived there, u = 2^-24, checked without a GPU in tests/test_elbo_penalty_cpu.py), and
UFlowElboLoss on every case of tests/golden/elbo_penalty.npz under the rule of tests/test_elbo_gpu.py (8 x the reference's
own fp32-versus-float64 gap, or the project bounds quoted there, whichever is larger).

Every `sums` buffer and every output plane is handed over full of NaN.  Equal images under a zero flow do NOT give a bitwise 0
distance through the FUSED entry points, penalised or not: the fp32 normalise / un-normalise round trip of the sampling
coordinate (utils/uflow_utils.py:71-76, reproduced by the kernels and by tests/census_ref.py) moves some coordinates by an ulp,
so the warped plane differs from the image in the last bits (the float64 restatement itself has h up to 5e-7 there), and the
column family's pair term is fma-contracted (census_dev.hpp pair_sq).  The exact 0 is pinned where the project pins it, on the
scalar 32 x 8 route of the standalone forward (W % 4 != 0); the fused case is held to the restatement under its bounds, with
h <= 1e-6, rho = -log sum w_j and dham = 0 to that order."""
import ctypes

import numpy as np
import pytest
import torch

from tests import census_ref as C
from tests import elbo_penalty_ref as P
from tests import elbo_ref as R
from tests import loss_kernels_ref as K

pytestmark = pytest.mark.gpu
NAN = float('nan')
SITES = {}
COMBOS = [('S', 'R'), ('N', 'Q'), ('C', 'Q')]
KIND_NAMES = {P.IDENTITY: 'identity', P.CHARBONNIER: 'charbonnier', P.ABS_ROBUST: 'abs_robust', P.GMM: 'gmm', P.GMM_SQ: 'gmm_sq'}


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    torch.set_num_threads(16)
    return functional


@pytest.fixture(autouse=True)
def mode_off_afterwards():
    from arflow_amd import functional
    assert functional.is_deterministic() is False, 'a test before this one left deterministic mode on'
    yield
    left_on = functional.is_deterministic()
    functional.set_deterministic(False)
    assert not left_on, 'this test left deterministic mode on'


@pytest.fixture(scope='module', autouse=True)
def margin_summary():
    yield
    for site in sorted(SITES):
        print('MARGIN %-44s worst err/bound %.4f' % (site, SITES[site]))


def cu(t):
    return t.detach().cuda()


def assert_within(got, ref, bound, site, tag):
    err = (torch.as_tensor(got).detach().cpu().double() - ref.double()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    w = C.worst(err, bound)
    SITES[site] = max(SITES.get(site, 0.0), w)
    print('%s | %s: max err %.3e, worst err/bound %.4f' % (site, tag, float(err.max()) if err.numel() else 0.0, w))
    assert bool((err <= bound).all()), '%s | %s: %d elements out of bound, worst err/bound %.3f' % (
        site, tag, int((~(err <= bound)).sum()), w)


def descriptor(kind):
    """(the host descriptor, the restatement's mixture) of a kind, with the ten-component mixtures of the reference's config"""
    from arflow_amd import functional as AF
    if kind == P.GMM:
        return AF.make_penalty('gmm', P.CENSUS_PI, P.CENSUS_BETA), P.mixture(P.CENSUS_PI, P.CENSUS_BETA)
    if kind == P.GMM_SQ:
        return AF.make_penalty('gmm', P.SMOOTH_PI, P.SMOOTH_BETA, squared=True), P.mixture(P.SMOOTH_PI, P.SMOOTH_BETA)
    return AF.make_penalty({v: k for k, v in P.KINDS.items()}[kind]), None


def nan_sums(AF, B, H, W):
    from arflow_amd import _lib
    return torch.full((_lib.load().arflow_sums_rows(B, H, W), AF.SUM_COLS), NAN, device='cuda')


def fold(buf, tag):
    assert bool(torch.isfinite(buf).all()), tag + ': a partial row was left unwritten'
    return buf.double().sum(0).cpu()


def check_sums(s2, ref, site, tag):
    assert_within(s2, ref.sums, ref.sums_bound, site + ' sums', tag)
    assert_within(s2[0] / (s2[1] + 1e-6), ref.loss, ref.loss_bound, site + ' loss', tag)


# ---- the fused forwards ---------------------------------------------------------------------------------------------
def fused_pen_forward(AF, ga, gb, flow, occ, R_, pen, valid_flow=None, pair=False):
    B, _, H, W = ga.shape
    a, f = cu(ga), cu(flow)
    b = None if pair else cu(gb)
    o = None if occ is None else cu(occ)
    v = None if valid_flow is None else cu(valid_flow)
    mask = torch.full((B, 1, H, W), NAN, device='cuda')
    dham = torch.full((B, 1, H, W), NAN, device='cuda')
    sums = nan_sums(AF, B, H, W)
    tail = (AF._p(o), mask.data_ptr(), dham.data_ptr(), sums.data_ptr(), B, H, W, R_, AF._p(v), 2 * H * W, ctypes.addressof(pen),
            AF._stream())
    if pair:
        AF._call('arflow_census_warp_pair_pen_fwd', a.data_ptr(), f.data_ptr(), 2 * H * W, *tail)
    else:
        AF._call('arflow_census_warp_pen_fwd', a.data_ptr(), b.data_ptr(), f.data_ptr(), 2 * H * W, *tail)
    torch.cuda.synchronize()
    return mask, dham, sums


def check_pen_forward(ref, mask, dham, occ, site, tag):
    if occ is None:
        assert torch.equal(mask.cpu().double(), ref.mask), tag + ': the validity mask is exact'
    else:
        assert_within(mask, ref.mask, ref.mask_bound, site + ' mask', tag)
    assert_within(dham, ref.dham, ref.dham_bound, site + ' dham', tag)
    z = (ref.pm == 0).expand_as(dham)
    assert float(dham.cpu()[z].abs().max() if bool(z.any()) else 0.0) == 0.0, tag + ': dham in the border band / at a masked pixel'


def run_fused(AF, kind, R_, shape, img, fl):
    B, H, W = shape
    ga, gb, flow, occ = C.fused_inputs(B, H, W, img, fl)
    pen, mix = descriptor(kind)
    tag = 'R%d %s %s%s %s' % (R_, shape, img, fl, KIND_NAMES[kind])
    ref = P.fused_pen_ref(ga, gb, flow, occ, R_, kind, mix)
    mask, dham, sums = fused_pen_forward(AF, ga, gb, flow, occ, R_, pen)
    check_pen_forward(ref, mask, dham, occ, 'fused ' + KIND_NAMES[kind], tag)
    s = fold(sums, tag)
    check_sums(s[:2], ref, 'fused ' + KIND_NAMES[kind], tag)
    assert float(s[2:].abs().max()) == 0.0, tag + ': columns 2, 3 belong to pair mode'


@pytest.mark.parametrize('kind', P.CENSUS_KINDS, ids=lambda k: KIND_NAMES[k])
def test_fused_penalised_forward_per_pixel(AF, kind):
    """the column family's shapes (W = 64 leaves R columns to a second tile, 124 two to a third, 60 one partial tile, 8 narrower
    than halo + wave; H = 8 / 32 / 36), radius 3, and radius 1 at one shape"""
    for shape in C.fused_shapes('column', 3):
        for img, fl in COMBOS:
            run_fused(AF, kind, 3, shape, img, fl)
    run_fused(AF, kind, 1, (1, 36, 64), 'S', 'R')


@pytest.mark.parametrize('kind', P.CENSUS_KINDS, ids=lambda k: KIND_NAMES[k])
def test_pair_penalised_forward_per_pixel(AF, kind):
    B2, H, W = C.PAIR_SHAPE['column']
    pen, mix = descriptor(kind)
    for R_, combos in ((3, COMBOS), (1, COMBOS[:1])):
        for img, fl in combos:
            gray2, flow2, occ2 = C.pair_inputs(B2, H, W, img, fl)
            tag = 'pair R%d %s %s%s %s' % (R_, (B2, H, W), img, fl, KIND_NAMES[kind])
            refs = P.pair_pen_ref(gray2, flow2, occ2, R_, kind, mix)
            mask, dham, sums = fused_pen_forward(AF, gray2, None, flow2, occ2, R_, pen, pair=True)
            s = fold(sums, tag)
            for d in (0, 1):
                check_pen_forward(refs[d], mask[d::2], dham[d::2], occ2, 'pair ' + KIND_NAMES[kind], tag + ' direction %d' % d)
                check_sums(s[2 * d:2 * d + 2], refs[d], 'pair ' + KIND_NAMES[kind], tag + ' direction %d' % d)


@pytest.mark.parametrize('kind', P.CENSUS_KINDS, ids=lambda k: KIND_NAMES[k])
def test_equal_images_and_zero_flow(AF, kind):
    """h is 0 up to the warp's coordinate round trip (the fp32 normalise / un-normalise of a zero flow is not the identity:
    the restatement, which takes the kernels' fp32 coordinate, has h <= 5e-7 here, not 0 -- see the module docstring): rho is
    -log sum_j w_j and dham is 0 for the mixture to that order, and the kernel meets the restatement under its bounds"""
    B, H, W = 1, 36, 64
    ga = C.grey('N', B, H, W, 0)
    flow = torch.zeros(B, 2, H, W)
    pen, mix = descriptor(kind)
    ref = P.fused_pen_ref(ga, ga, flow, None, 3, kind, mix)
    assert float(ref.ham.abs().max()) <= 1e-6
    if kind == P.GMM:
        n = float(ref.pm.sum())
        assert float(ref.dham.abs().max()) <= 4.0 * 1e-6  # rho' = bbar h, bbar <= max beta = 3.2
        assert abs(float(ref.sums[0]) + n * float(torch.log(mix[0].sum()))) <= 1e-9 * n
    mask, dham, sums = fused_pen_forward(AF, ga, ga, flow, None, 3, pen)
    check_pen_forward(ref, mask, dham, None, 'equal images ' + KIND_NAMES[kind], 'fused')
    check_sums(fold(sums, 'equal')[:2], ref, 'equal images ' + KIND_NAMES[kind], 'fused')


@pytest.mark.parametrize('shape', [(2, 8, 64), (1, 36, 124)], ids=str)
def test_abs_robust_descriptor_is_the_unpenalised_entry_point_bit_for_bit(AF, shape):
    B, H, W = shape
    pen, _ = descriptor(P.ABS_ROBUST)
    ga, gb, flow, occ = C.fused_inputs(B, H, W, 'S', 'R')
    new = fused_pen_forward(AF, ga, gb, flow, occ, 3, pen)
    old = [torch.full((B, 1, H, W), NAN, device='cuda'), torch.full((B, 1, H, W), NAN, device='cuda'), nan_sums(AF, B, H, W)]
    keep = [cu(t) for t in (ga, gb, flow, occ)]  # (held: a temporary's block would be handed to the next allocation)
    AF._call('arflow_census_warp_fwd', keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), 2 * H * W, keep[3].data_ptr(),
             old[0].data_ptr(), old[1].data_ptr(), old[2].data_ptr(), B, H, W, 3, AF._stream())
    for name, a, b in zip(('mask_out', 'dham', 'sums rows'), new, old):
        assert torch.equal(a, b), name
    if B % 2 == 0:
        gray2, flow2, occ2 = C.pair_inputs(B, H, W, 'N', 'R')
        new = fused_pen_forward(AF, gray2, None, flow2, occ2, 3, pen, pair=True)
        old = [torch.full((B, 1, H, W), NAN, device='cuda'), torch.full((B, 1, H, W), NAN, device='cuda'), nan_sums(AF, B, H, W)]
        keep = [cu(t) for t in (gray2, flow2, occ2)]
        AF._call('arflow_census_warp_pair_fwd', keep[0].data_ptr(), keep[1].data_ptr(), 2 * H * W, keep[2].data_ptr(),
                 old[0].data_ptr(), old[1].data_ptr(), old[2].data_ptr(), B, H, W, 3, AF._stream())
        for name, a, b in zip(('mask_out', 'dham', 'sums rows'), new, old):
            assert torch.equal(a, b), 'pair ' + name


def test_valid_flow(AF):
    """equal to `flow`: the bits of NULL.  A different one: mask_out and the sums change as the restatement says, the distances
    do not (IDENTITY: dham = pm, sums[0] / the mask's sum weighs the same h)."""
    B, H, W = 2, 36, 64
    ga, gb, flow, occ = C.fused_inputs(B, H, W, 'S', 'R')
    other = C.flow('Q', B, H, W) * 4.0  # integer displacements up to 12 pixels: another set of invalid pixels
    for kind in (P.GMM, P.IDENTITY):
        pen, mix = descriptor(kind)
        null = fused_pen_forward(AF, ga, gb, flow, occ, 3, pen)
        same = fused_pen_forward(AF, ga, gb, flow, occ, 3, pen, valid_flow=flow.clone())
        for a, b in zip(null, same):
            assert torch.equal(a, b)
        ref = P.fused_pen_ref(ga, gb, flow, occ, 3, kind, mix, valid_flow32=other)
        ref0 = P.fused_pen_ref(ga, gb, flow, occ, 3, kind, mix)
        assert int((ref.mask != ref0.mask).sum()) > 50 and torch.equal(ref.ham, ref0.ham)
        mask, dham, sums = fused_pen_forward(AF, ga, gb, flow, occ, 3, pen, valid_flow=other)
        assert not torch.equal(mask, null[0])
        check_pen_forward(ref, mask, dham, occ, 'valid_flow ' + KIND_NAMES[kind], 'single')
        check_sums(fold(sums, 'valid_flow')[:2], ref, 'valid_flow ' + KIND_NAMES[kind], 'single')
    # pair form
    gray2, flow2, occ2 = C.pair_inputs(B, H, W, 'S', 'R')
    pen, mix = descriptor(P.GMM)
    refs = P.pair_pen_ref(gray2, flow2, occ2, 3, P.GMM, mix, valid_flow2=other)
    mask, dham, sums = fused_pen_forward(AF, gray2, None, flow2, occ2, 3, pen, valid_flow=other, pair=True)
    s = fold(sums, 'pair valid_flow')
    for d in (0, 1):
        check_pen_forward(refs[d], mask[d::2], dham[d::2], occ2, 'valid_flow pair', 'direction %d' % d)
        check_sums(s[2 * d:2 * d + 2], refs[d], 'valid_flow pair', 'direction %d' % d)


# ---- the standalone forward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', P.CENSUS_KINDS, ids=lambda k: KIND_NAMES[k])
def test_standalone_penalised_forward(AF, kind):
    pen, mix = descriptor(kind)
    for R_, B, H, W in [(3, 2, 20, 68), (2, 1, 17, 35), (3, 1, 7, 7), (1, 1, 1, 1)]:
        im_a, im_b, mask = C.image('S', B, H, W, 0), C.image('S', B, H, W, 1), C.user_mask(B, H, W)
        tag = 'R%d %s %s' % (R_, (B, H, W), KIND_NAMES[kind])
        ref = P.standalone_pen_ref(im_a, im_b, mask, R_, kind, mix)
        ham = torch.full((B, 1, H, W), NAN, device='cuda')
        dham = torch.full((B, 1, H, W), NAN, device='cuda')
        sums = nan_sums(AF, B, H, W)
        keep = [cu(t) for t in (im_a, im_b, mask)]
        AF._call('arflow_census_pen_fwd', keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), ham.data_ptr(),
                 dham.data_ptr(), sums.data_ptr(), B, H, W, R_, ctypes.addressof(pen), AF._stream())
        assert_within(ham, ref.ham, ref.ham_bound, 'standalone ham', tag)
        assert_within(dham, ref.dham, ref.dham_bound, 'standalone dham ' + KIND_NAMES[kind], tag)
        check_sums(fold(sums, tag)[:2], ref, 'standalone ' + KIND_NAMES[kind], tag)
    # an image against itself on the scalar route (W % 4 != 0): h is exactly 0, and so is the mixture's dham
    B, H, W = 1, 17, 35
    im = C.image('N', B, H, W, 0)
    ham = torch.full((B, 1, H, W), NAN, device='cuda')
    dham = torch.full((B, 1, H, W), NAN, device='cuda')
    sums = nan_sums(AF, B, H, W)
    keep = [cu(im), cu(torch.ones(B, 1, H, W))]
    AF._call('arflow_census_pen_fwd', keep[0].data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), ham.data_ptr(),
             dham.data_ptr(), sums.data_ptr(), B, H, W, 3, ctypes.addressof(pen), AF._stream())
    assert float(ham.abs().max()) == 0.0
    if kind == P.GMM:
        assert float(dham.abs().max()) == 0.0
        n = (H - 6) * (W - 6)
        s = fold(sums, 'self')
        lw = float(torch.log(mix[0].sum()))  # k-term sum, logf, the 64u of the in-kernel tree (census_ref's figure)
        assert float(s[1]) == n and abs(float(s[0]) / n + lw) <= (64 + 16) * C.U * max(abs(lw), 1.0)


# ---- smoothness ---------------------------------------------------------------------------------------------------------
SMOOTH_SHAPES = [(1, 1, 2), (1, 2, 1), (2, 3, 5), (1, 8, 257), (2, 9, 16)]


def smooth_calls(AF, flow, img, alpha, order, pen, coef):
    B, _, H, W = flow.shape
    f, im = cu(flow), cu(img)
    sums = nan_sums(AF, B, H, W)
    g = torch.full((B, 2, H, W), NAN, device='cuda')
    args = (B, 3, H, W, 2 * H * W, 1.0, float(alpha), order, 1)
    AF._call('arflow_smooth_pen_fwd', f.data_ptr(), im.data_ptr(), sums.data_ptr(), *args, ctypes.addressof(pen), AF._stream())
    c = cu(torch.tensor(coef))
    AF._call('arflow_smooth_pen_bwd', f.data_ptr(), im.data_ptr(), c.data_ptr(), g.data_ptr(), *args, ctypes.addressof(pen),
             AF._stream())
    torch.cuda.synchronize()
    return sums, g


@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('kind', P.SMOOTH_KINDS, ids=lambda k: KIND_NAMES[k])
def test_smoothness_forward_and_backward(AF, kind, order):
    """a single difference, an odd shape, one column past the backward's 256-column row, a plain one; 'Q' flows hold a patch
    of exactly zero differences (loss_kernels_ref.smooth_flow); alpha 150 and 0 (the two sums the loss combines)"""
    pen, mix = descriptor(kind)
    for B, H, W in SMOOTH_SHAPES:
        img = K.smooth_image(B, 3, H, W)
        for fkind, alpha in (('Q', 150.0), ('R', 0.0)):
            flow = K.smooth_flow(fkind, B, H, W)
            tag = '%s order %d %s %s alpha %g' % (KIND_NAMES[kind], order, (B, H, W), fkind, alpha)
            ref = P.smooth_pen_ref(flow, img, 1.0, alpha, order, 1, kind, mix, coef=K.COEF)
            sums, g = smooth_calls(AF, flow, img, alpha, order, pen, K.COEF)
            assert_within(fold(sums, tag)[:2], ref.sums, ref.sums_bound, 'smooth sums ' + KIND_NAMES[kind], tag)
            assert_within(g, ref.grad, ref.grad_bound, 'smooth grad ' + KIND_NAMES[kind], tag)
            z = ref.g_abs == 0
            assert float(g.cpu()[z].abs().max() if bool(z.any()) else 0.0) == 0.0, tag + ': zero differences give a zero gradient'
            if kind == P.CHARBONNIER:  # arflow_smooth_fwd / _bwd with penalty = 1, bit for bit
                old_s, old_g = nan_sums(AF, B, H, W), torch.full((B, 2, H, W), NAN, device='cuda')
                args = (B, 3, H, W, 2 * H * W, 1.0, float(alpha), order, 1, 1)
                keep = [cu(flow), cu(img), cu(torch.tensor(K.COEF))]
                AF._call('arflow_smooth_fwd', keep[0].data_ptr(), keep[1].data_ptr(), old_s.data_ptr(), *args, AF._stream())
                AF._call('arflow_smooth_bwd', keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), old_g.data_ptr(), *args,
                         AF._stream())
                assert torch.equal(sums, old_s) and torch.equal(g, old_g), tag


# ---- the loss -----------------------------------------------------------------------------------------------------------
def _run(g, tag, pair=True, fused=True):
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    kind = P.CASES[tag]['inputs']
    cu_ = lambda name: torch.from_numpy(np.array(g.raw(name))).cuda()  # noqa: E731
    net12, net21 = cu_('net12_' + tag).requires_grad_(True), cu_('net21_' + tag).requires_grad_(True)
    loss = get_loss(AttrDict(P.case_cfg(tag)))
    loss.pair, loss.fused = pair, fused
    res = loss({'flows_fw': [None, None, net12], 'flows_bw': [None, None, net21]}, cu_('im1_' + kind), cu_('im2_' + kind),
               eps=(cu_('eps12_' + tag), cu_('eps21_' + tag)))
    g12, g21 = torch.autograd.grad(res[0], (net12, net21))
    out = dict(zip(R.OUTPUTS[:8], res))
    out.update(gnet12=g12, gnet21=g21)
    return {k: torch.as_tensor(v).detach().double().cpu().numpy() for k, v in out.items()}


def _against_the_reference(g, tag, got, what=''):
    bad = []
    for key in R.OUTPUTS:
        ref = g.raw('%s_%s' % (key, tag))
        assert got[key].shape == ref.shape, key
        bound = P.golden_bound(g, key, tag)
        err = np.abs(got[key] - ref)
        print('%s%s %-12s max err %.3e  max err / bound %.3f  max|ref| %.3e' % (tag, what, key, err.max(), (err / bound).max(),
                                                                                np.abs(ref).max()))
        if not (np.isfinite(got[key]).all() and (err <= bound).all()):
            bad.append(key)
    assert not bad, bad


@pytest.mark.parametrize('tag', list(P.CASES))
def test_loss_against_the_reference(golden, tag):
    g = golden('elbo_penalty')
    _against_the_reference(g, tag, _run(g, tag))


@pytest.mark.parametrize('pair,fused', [(False, True), (True, False)], ids=['per-direction', 'unfused'])
def test_every_route_of_the_all_mixture_case(golden, AF, pair, fused):
    """gmm_all_mean_sparse through the per-direction composition and through the unfused photometric path: against the
    fixture, and against the default route under the bounds tests/test_elbo_gpu.py uses for the same comparison"""
    g = golden('elbo_penalty')
    tag = 'gmm_all_mean_sparse'
    AF.start_kernel_timing()
    got = _run(g, tag, pair=pair, fused=fused)
    launched = {name for name, _ in AF.stop_kernel_timing()}
    want = 'arflow_census_warp_pen_fwd' if fused else 'arflow_census_pen_fwd'
    assert want in launched and 'arflow_census_warp_pair_pen_fwd' not in launched, launched
    assert {'arflow_smooth_pen_fwd', 'arflow_smooth_pen_bwd'} <= launched and 'arflow_uflow_pair_bwd' not in launched, launched
    _against_the_reference(g, tag, got, ' pair=%s fused=%s' % (pair, fused))
    if fused:
        one = _run(g, tag)
        for key in R.SCALARS:
            assert abs(one[key] - got[key]) <= 1e-7 + 2e-6 * abs(got[key]), key
        for key in ('flow12_2', 'valid_mask12', 'occu_mask12'):
            assert np.array_equal(one[key], got[key]), key
        for key in ('gnet12', 'gnet21'):
            err = np.abs(one[key] - got[key])
            assert (err <= 1e-7 * np.abs(got[key]).max() + 1e-12 + 1e-5 * np.abs(got[key])).all(), (key, float(err.max()))


def test_the_default_configuration_makes_the_calls_it_always_made(golden, AF, monkeypatch):
    """the names passed to functional._call during one forward and backward of elbo_ref.case_cfg('diag'): the one-launch
    backward, no penalised entry point; the outputs are those of tests/golden/elbo.npz under its bounds"""
    from tests import test_elbo_gpu as E
    names = []
    real = AF._call

    def recording(name, *args, **kw):
        names.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(AF, '_call', recording)
    g = golden('elbo')
    got, _ = E._run(g, 'diag')
    monkeypatch.setattr(AF, '_call', real)
    print(names)
    assert 'arflow_uflow_pair_bwd' in names and not [n for n in names if '_pen_' in n], names
    assert sorted(n for n in names if 'census' in n or 'smooth' in n or 'uflow' in n) == sorted([
        'arflow_splat_smooth_fwd', 'arflow_census_warp_pair_fwd', 'arflow_smooth_fwd', 'arflow_smooth_bwd', 'arflow_uflow_pair_bwd']), names
    E._against_the_reference(g, 'diag', got)


def test_deterministic_mode_reproduces_a_mixture_case(golden, AF):
    g = golden('elbo_penalty')
    with AF.deterministic():
        one, two = _run(g, 'gmm_all_mean_sparse'), _run(g, 'gmm_all_mean_sparse')
    for key in R.OUTPUTS:
        assert np.array_equal(one[key], two[key]), key


def test_one_training_step_with_the_reference_mixture_config(monkeypatch):
    """the penalty_*_pi / _beta keys of the reference's chairs_uflow_elbo_gmm.json through get_loss and one TrainStep on
    synthetic data: finite loss, finite gradients everywhere"""
    from arflow_amd import train_step as TS
    mcfg = dict(type='uflow_prob', feature_norm=True, level_dropout=0.1, out_channels=[2, 2, 0], inv_cov=False, n_pyramids=1,
                mixture_weights=False)
    lcfg = dict(R.BASE, w_smooth=4.0, w_entropy=0.05, data_penalty=['gmm'], penalty_smooth='gmm', **P.GMM_KEYS)
    monkeypatch.setitem(TS.WORKLOADS, 'pwcprobflow+uflow_elbo_gmm', (mcfg, lcfg))
    dev = torch.device('cuda')
    step = TS.TrainStep('pwcprobflow+uflow_elbo_gmm', dev, seed=1234)
    assert not step.loss.default
    loss = step(TS.synthetic_pairs(1, 64, 128, device=dev, seed=5))
    assert bool(torch.isfinite(loss)), float(loss)
    for n, p in step.model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
