"""GPU: the census kernels PER PIXEL against the float64 reference of tests/census_ref.py, off the sizes of the golden
fixtures: the standalone distance (census4, the scalar 32 x 8 tiles, census_any) and the three families of the fused warp +
mask + census direction -- column (census_col.hip, the default), ordered (census_warp.hip), pair-symmetric (census_sym.hip,
with TWO and FOUR chunks per strip: the carry buffer and its parity, which no other test reaches) -- for R = 1, 2, 3,
forward maps (mask, dham, the partial rows and their fold, the loss) through the raw entry points, the backward kernels alone
on a weight plane of the test's choosing, the pair forms, the census role of the one-launch UFlowLoss backward, and each
family once end to end through the autograd functions.

Every bound is derived in the docstring of tests/census_ref.py (u = 2^-24) and checked without a GPU in
tests/test_census_ref_cpu.py: the fp32 oracle sits inside each with 4x room, every mutation of the reference leaves by > 100x
on these same inputs -- so a kernel with that mistake fails here.  No element is left out of any comparison, no bound was taken
from what the kernels give.  Every `sums` buffer is handed over full of NaN: every partial row must come back finite.
Every test leaves deterministic mode off."""
import pytest
import torch

from tests import census_ref as C

pytestmark = pytest.mark.gpu
U = C.U
SITES = {}
NAN = float('nan')


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
    """elementwise |got - ref| <= bound; prints the worst err / bound of the call and keeps the worst per site"""
    err = (got.detach().cpu().double() - ref.double()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    w = C.worst(err, bound)
    SITES[site] = max(SITES.get(site, 0.0), w)
    print('%s | %s: max err %.3e, worst err/bound %.4f' % (site, tag, float(err.max()) if err.numel() else 0.0, w))
    assert bool((err <= bound).all()), '%s | %s: %d elements out of bound, worst err/bound %.3f' % (
        site, tag, int((~(err <= bound)).sum()), w)


def assert_zero_where(got, where, tag):
    got = got.detach().cpu()
    where = where.expand_as(got)
    assert float(got[where].abs().max() if bool(where.any()) else 0.0) == 0.0, tag


def select(monkeypatch, family):
    # read by the library at every call
    monkeypatch.setenv('ARFLOW_CENSUS_SYM', '1' if family == 'pair-symmetric' else '0')
    monkeypatch.setenv('ARFLOW_CENSUS_COL', '0' if family == 'ordered' else '1')


def nan_sums(AF, B, H, W):
    from arflow_amd import _lib
    rows = _lib.load().arflow_sums_rows(B, H, W)
    assert rows == C.sums_rows(B, H, W)
    return torch.full((rows, AF.SUM_COLS), NAN, device='cuda')


def fold(buf, tag):
    assert bool(torch.isfinite(buf).all()), tag + ': a partial row was left unwritten'
    return buf.double().sum(0).cpu()


def gpu_flow(AF, flow, as_slice):
    f = cu(C.strided(flow))[:, 2:4] if as_slice else cu(flow)
    f, fbs = AF._flow_view(f)
    if as_slice:
        assert fbs == 4 * flow.shape[2] * flow.shape[3], 'the slice is consumed in place'
    return f, fbs


def check_sums(s2, ref, site, tag):
    assert_within(s2, ref.sums, ref.sums_bound, site + ' sums', tag)
    loss = s2[0] / (s2[1] + 1e-6)
    assert_within(loss, ref.loss, ref.loss_bound, site + ' loss', tag)


# ---- the fused direction through the raw entry points ----------------------------------------------------------------
def fused_forward(AF, ga, gb, flow, occ, R, as_slice=False):
    B, _, H, W = ga.shape
    f, fbs = gpu_flow(AF, flow, as_slice)
    a, b = cu(ga), cu(gb)
    o = None if occ is None else cu(occ)
    mask = torch.full((B, 1, H, W), NAN, device='cuda')
    dham = torch.full((B, 1, H, W), NAN, device='cuda')
    sums = nan_sums(AF, B, H, W)
    AF._call('arflow_census_warp_fwd', a.data_ptr(), b.data_ptr(), f.data_ptr(), fbs, AF._p(o), mask.data_ptr(), dham.data_ptr(),
             sums.data_ptr(), B, H, W, R, AF._stream())
    return mask, dham, sums


def fused_backward(AF, ga, gb, flow, w, scale, R, as_slice=False):
    B, _, H, W = ga.shape
    f, fbs = gpu_flow(AF, flow, as_slice)
    a, b, wg = cu(ga), cu(gb), cu(w)
    sc = None if scale is None else torch.tensor([scale], device='cuda')
    g = torch.full((B, 2, H, W), NAN, device='cuda')
    AF._call('arflow_census_warp_bwd', a.data_ptr(), b.data_ptr(), f.data_ptr(), fbs, wg.data_ptr(), AF._p(sc), g.data_ptr(),
             B, H, W, R, AF._stream())
    return g


def check_forward(ref, mask, dham, sums, occ, site, tag):
    if occ is None:
        assert torch.equal(mask.cpu().double(), ref.mask), tag + ': the validity mask is exact'
    else:
        assert_within(mask, ref.mask, ref.mask_bound, site + ' mask', tag)
        assert_zero_where(mask, ref.warp.valid == 0, tag + ': mask at an invalid pixel')
    assert_within(dham, ref.dham, ref.dham_bound, site + ' dham', tag)
    assert_zero_where(dham, ref.pm == 0, tag + ': dham in the border band / at a masked pixel')
    return fold(sums, tag)


def check_grad(g, ref, site, tag):
    assert_within(g, ref.grad, ref.grad_bound, site, tag)
    assert_zero_where(g, ref.g_abs == 0, tag + ': a gradient element all of whose contributions are 0')


def run_fused_case(AF, family, R, shape, img, fl, as_slice=False, occ_on=True, backward=True):
    B, H, W = shape
    ga, gb, flow, occ = C.fused_inputs(B, H, W, img, fl)
    occ = occ if occ_on else None
    w = C.weight_plane(B, H, W)
    tag = '%s R%d %s %s%s%s%s' % (family, R, shape, img, fl, ' slice' if as_slice else '', '' if occ_on else ' no range map')
    ref = C.fused_ref(ga, gb, flow, occ, R, w=w)
    mask, dham, sums = fused_forward(AF, ga, gb, flow, occ, R, as_slice)
    s = check_forward(ref, mask, dham, sums, occ, family, tag)
    check_sums(s[:2], ref, family, tag)
    assert float(s[2:].abs().max()) == 0.0, tag + ': columns 2, 3 belong to pair mode'
    if backward:
        g = fused_backward(AF, ga, gb, flow, w, None, R, as_slice)
        check_grad(g, ref, family + ' d flow', tag)
        ref2 = C.fused_ref(ga, gb, flow, occ, R, w=w, scale=-0.7)
        check_grad(fused_backward(AF, ga, gb, flow, w, -0.7, R, as_slice), ref2, family + ' d flow', tag + ' scale -0.7')
    return ref


@pytest.mark.parametrize('R', [1, 2, 3])
@pytest.mark.parametrize('family', ['column', 'ordered', 'pair-symmetric'])
def test_fused_direction_per_pixel(AF, family, R, monkeypatch):
    """column: W = 64 leaves R columns to a second tile, 124 (R = 3) two columns to a third, 60 is one partial tile, 8 is
    narrower than halo + wave; H = 8 / 32 / 36: a partial tile, exactly one, a second tile of 4 rows.  ordered: 16 + 4 rows,
    64 + 4 columns; 8 x 8.  pair-symmetric, one chunk per strip: 16 x 60 (one strip + 4 columns), 32 x 116."""
    select(monkeypatch, family)
    for k, shape in enumerate(C.fused_shapes(family, R)):
        for img, fl in C.COMBOS:
            first = (img, fl) == C.COMBOS[0]
            run_fused_case(AF, family, R, shape, img, fl, as_slice=first and k == 0)
        run_fused_case(AF, family, R, shape, 'S', 'R', occ_on=False, backward=False)


@pytest.mark.parametrize('shape,R,n', [(C.SYM_N2, 1, 2), (C.SYM_N2, 2, 2), (C.SYM_N2, 3, 2), (C.SYM_N4, 3, 4)],
                         ids=lambda v: str(v).replace(' ', ''))
def test_pair_symmetric_strips_of_several_chunks(AF, shape, R, n, monkeypatch):
    """census_sym_strip_h gives n = 2 (eight strips of two chunks per image column) and n = 4 only once the launch has
    768 workgroups: the second and later iterations of the chunk loop -- rows received from the carry buffer, its parity
    double buffer, only the first chunk recomputing R rows -- run at no smaller size and in no other test."""
    assert C.sym_chunks(*shape, R) == n
    select(monkeypatch, 'pair-symmetric')
    run_fused_case(AF, 'pair-symmetric n=%d' % n, R, shape, 'S', 'R')


@pytest.mark.parametrize('family,shape', C.ROWS_SHAPES, ids=lambda v: str(v).replace(' ', ''))
def test_partial_rows_of_padding_workgroups(AF, family, shape, monkeypatch):
    """functional._new_sums hands the kernels an UNINITIALISED buffer on the promise that every row is written
    (af_store_partial, padding workgroups of the grid rounded up to 8): tile counts 1, 8, 1, 8, 4, 8 (R = 3; the other shapes
    of this file give 2, 3, 4, 6, 12 and 768)."""
    B, H, W = shape
    assert (C.family_tiles(family, B, H, W, 3) % 8 == 0) == (shape in [(4, 8, 64), (2, 20, 68), (2, 16, 60)])
    select(monkeypatch, family)
    run_fused_case(AF, family + ' rows', 3, shape, 'S', 'R', backward=False)


# ---- pair mode and the census role of the one-launch backward ---------------------------------------------------------
@pytest.mark.parametrize('R', [1, 2, 3])
@pytest.mark.parametrize('family', ['column', 'ordered'])
def test_pair_mode_per_pixel(AF, family, R, monkeypatch):
    """arflow_census_warp_pair_fwd / _bwd and arflow_uflow_pair_bwd's census role: sample s = 2 b + direction, image b and
    range map from plane s ^ 1, sums columns (0, 1) / (2, 3), one scale per direction; the flows are a slice of a wider
    tensor.  The reference is two calls of the single-direction one."""
    select(monkeypatch, family)
    B2, H, W = C.PAIR_SHAPE[family]
    scale2 = (0.7, -1.3)
    for img, fl in C.PAIR_COMBOS:
        gray2, flow2, occ2 = C.pair_inputs(B2, H, W, img, fl)
        w2 = C.weight_plane(B2, H, W)
        tag = '%s pair R%d %s %s%s' % (family, R, (B2, H, W), img, fl)
        refs = C.pair_ref(gray2, flow2, occ2, R, w2, scale2)
        f, fbs = gpu_flow(AF, flow2, True)
        g2, o2, wg = cu(gray2), cu(occ2), cu(w2)
        mask = torch.full((B2, 1, H, W), NAN, device='cuda')
        dham = torch.full((B2, 1, H, W), NAN, device='cuda')
        sums = nan_sums(AF, B2, H, W)
        AF._call('arflow_census_warp_pair_fwd', g2.data_ptr(), f.data_ptr(), fbs, o2.data_ptr(), mask.data_ptr(), dham.data_ptr(),
                 sums.data_ptr(), B2, H, W, R, AF._stream())
        s = fold(sums, tag)
        sc = torch.tensor(scale2, device='cuda')
        grads = {}
        g = torch.full((B2, 2, H, W), NAN, device='cuda')
        AF._call('arflow_census_warp_pair_bwd', g2.data_ptr(), f.data_ptr(), fbs, wg.data_ptr(), sc.data_ptr(), g.data_ptr(), B2, H, W,
                 R, AF._stream())
        grads['pair_bwd'] = g
        # the same role inside the one-launch backward; its smoothness role gets zero cotangents
        h, w_ = H // 4, W // 4
        fl2 = torch.zeros(B2, 2, h, w_, device='cuda')
        img2 = torch.rand(B2, 3, h, w_, device='cuda')
        coef = torch.zeros(2, device='cuda')
        g = torch.full((B2, 2, H, W), NAN, device='cuda')
        gf2 = torch.full((B2, 2, h, w_), NAN, device='cuda')
        AF._call('arflow_uflow_pair_bwd', g2.data_ptr(), f.data_ptr(), fbs, wg.data_ptr(), sc.data_ptr(), g.data_ptr(), B2, H, W, R,
                 fl2.data_ptr(), 2 * h * w_, img2.data_ptr(), coef.data_ptr(), gf2.data_ptr(), h, w_, 1.0, 150.0, 1, 1, 1, AF._stream())
        grads['uflow_pair_bwd'] = g
        assert float(gf2.abs().max()) == 0.0
        for d in (0, 1):
            ref = refs[d]
            site = '%s pair' % family
            assert_within(mask[d::2], ref.mask, ref.mask_bound, site + ' mask', tag)
            assert_within(dham[d::2], ref.dham, ref.dham_bound, site + ' dham', tag)
            assert_zero_where(dham[d::2], ref.pm == 0, tag)
            check_sums(s[2 * d:2 * d + 2], ref, site, tag + ' direction %d' % d)
            for name, g in grads.items():
                check_grad(g[d::2], ref, site + ' d flow', tag + ' %s direction %d' % (name, d))


# ---- end to end -------------------------------------------------------------------------------------------------------
def e2e_bound(ref):
    """the backward's scale is gloss / (s1 + 1e-6) from the kernels' own fp32 sums: + (8u + delta_s1 / den) G_abs"""
    return ref.grad_bound + ref.g_abs * (8 * U + float(ref.sums_bound[1] / (ref.sums[1] + 1e-6)))


@pytest.mark.parametrize('family', ['column', 'ordered', 'pair-symmetric'])
def test_census_warp_loss_end_to_end(AF, family, monkeypatch):
    select(monkeypatch, family)
    R = 3
    shape = C.fused_shapes(family, R)[0]
    B, H, W = shape
    ga, gb, flow, occ = C.fused_inputs(B, H, W, 'S', 'R')
    ref0 = C.fused_ref(ga, gb, flow, occ, R, w=None, fold_fp32=True)
    ref = C.fused_ref(ga, gb, flow, occ, R, w=None, scale=1.0 / float(ref0.sums[1] + 1e-6), fold_fp32=True)
    f = cu(flow).requires_grad_(True)
    loss, mask = AF.census_warp_loss(cu(ga), cu(gb), f, cu(occ), 2 * R + 1)
    g, = torch.autograd.grad(loss, [f])
    tag = '%s %s' % (family, shape)
    assert_within(mask, ref.mask, ref.mask_bound, family + ' e2e mask', tag)
    assert_within(loss, ref.loss, ref.loss_bound, family + ' e2e loss', tag)
    assert_within(g, ref.grad, e2e_bound(ref), family + ' e2e d flow', tag)
    assert_zero_where(g, ref.g_abs == 0, tag)


@pytest.mark.parametrize('family', ['column', 'ordered'])
def test_pair_losses_end_to_end(AF, family, monkeypatch):
    """AF.census_warp_pair_loss, and AF.uflow_pair_loss's level-0 gradient with zero level-2 flows: every level-2 pixel
    lands on itself, the range map is exactly 1 and the mask is the validity mask."""
    select(monkeypatch, family)
    R = 3
    B2, H, W = C.PAIR_SHAPE[family]
    gray2, flow2, occ2 = C.pair_inputs(B2, H, W, 'S', 'R')
    cot = (0.7, -1.3)

    def refs_for(occ):
        r0 = C.pair_ref(gray2, flow2, occ, R, None, (1.0, 1.0), fold_fp32=True)
        return C.pair_ref(gray2, flow2, occ, R, None, [c / float(r.sums[1] + 1e-6) for c, r in zip(cot, r0)], fold_fp32=True)
    f = cu(flow2).requires_grad_(True)
    l0, l1, mask = AF.census_warp_pair_loss(cu(gray2), f, cu(occ2), 2 * R + 1)
    g, = torch.autograd.grad([l0, l1], [f], [torch.tensor(c, device='cuda') for c in cot])
    for d, (ref, loss) in enumerate(zip(refs_for(occ2), (l0, l1))):
        tag = '%s census_warp_pair_loss direction %d' % (family, d)
        assert_within(mask[d::2], ref.mask, ref.mask_bound, family + ' e2e mask', tag)
        assert_within(loss, ref.loss, ref.loss_bound, family + ' e2e loss', tag)
        assert_within(g[d::2], ref.grad, e2e_bound(ref), family + ' e2e d flow', tag)
    ones = torch.ones(B2, 1, H // 4, W // 4)
    f0 = cu(flow2).requires_grad_(True)
    f2 = torch.zeros(B2, 2, H // 4, W // 4, device='cuda', requires_grad=True)
    small = torch.rand(B2, 3, H // 4, W // 4, device='cuda')
    l0, l1, s, mask = AF.uflow_pair_loss(cu(gray2), small, f0, f2, None, 150.0, 1, 2 * R + 1)
    zero2 = torch.zeros(2, device='cuda')
    g, = torch.autograd.grad([l0, l1, s], [f0], [torch.tensor(cot[0], device='cuda'), torch.tensor(cot[1], device='cuda'), zero2])
    for d, (ref, loss) in enumerate(zip(refs_for(ones), (l0, l1))):
        tag = '%s uflow_pair_loss direction %d' % (family, d)
        assert torch.equal(mask[d::2].cpu().double(), ref.warp.valid), tag + ': range map 1 -> the mask is the validity mask'
        assert_within(loss, ref.loss, ref.loss_bound, family + ' e2e loss', tag)
        assert_within(g[d::2], ref.grad, e2e_bound(ref), family + ' e2e d flow', tag)


# ---- standalone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.STANDALONE, ids=lambda c: 'R%d-%dx%dx%d' % c)
def test_standalone_per_pixel(AF, case):
    """census4 (W % 4 == 0: 20 x 68), the scalar 32 x 8 tiles (8 + 1 rows, 32 + 1 / 32 + 3 columns), census_any (R = 4), a
    7 x 7 image whose interior is one pixel, 1 x 9 and 1 x 1 (nothing but padding around the pixel): ham through the raw
    entry point and through TernaryDistFunction, dham / sums / loss with a mask, both image gradients for a weight plane."""
    R, B, H, W = case
    for img in ('S', 'N', 'C'):
        im_a, im_b = C.image(img, B, H, W, 0), C.image(img, B, H, W, 1)
        mask, w = C.user_mask(B, H, W), C.weight_plane(B, H, W)
        tag = 'R%d %s %s' % (R, (B, H, W), img)
        ref = C.standalone_ref(im_a, im_b, R, mask=mask, w=w)
        a, b = cu(im_a), cu(im_b).requires_grad_(True)
        # without a mask: the map alone
        ham = torch.full((B, 1, H, W), NAN, device='cuda')
        AF._call('arflow_census_fwd', a.data_ptr(), b.data_ptr(), None, ham.data_ptr(), None, None, B, H, W, R, AF._stream())
        assert_within(ham, ref.ham, ref.ham_bound, 'standalone ham', tag)
        if img == 'C':  # equal neighbours: every contribution is 0
            assert_zero_where(ham, ref.ham == 0, tag + ': ham where every pair is 0')
            assert bool((ref.ham == 0).any()) == (min(H, W) > 2 * R)
        # with a mask: ham, dham and the partial rows of one launch
        ham2 = torch.full((B, 1, H, W), NAN, device='cuda')
        dham = torch.full((B, 1, H, W), NAN, device='cuda')
        sums = nan_sums(AF, B, H, W)
        m = cu(mask)
        AF._call('arflow_census_fwd', a.data_ptr(), b.data_ptr(), m.data_ptr(), ham2.data_ptr(), dham.data_ptr(), sums.data_ptr(), B, H,
                 W, R, AF._stream())
        assert torch.equal(ham2, ham), tag
        assert_within(dham, ref.dham, ref.dham_bound, 'standalone dham', tag)
        assert_zero_where(dham, ref.pm == 0, tag + ': dham in the border band')
        check_sums(fold(sums, tag)[:2], ref, 'standalone', tag)
        # TernaryDistFunction and both gradients
        a2 = cu(im_a).requires_grad_(True)
        dist = AF.TernaryDistFunction.apply(a2, b, R)
        assert torch.equal(dist, ham), tag
        ga_, gb_ = torch.autograd.grad(dist, [a2, b], cu(w))
        check_grad(gb_, ref, 'standalone d im_b', tag)
        check_grad(ga_, C.standalone_ref(im_b, im_a, R, w=w), 'standalone d im_a', tag)
    if (H, W) == (1, 1):  # the same image on both sides: exactly 0 even in the zero padding
        same = cu(C.image('N', B, H, W, 0))
        ham = torch.full((B, 1, H, W), NAN, device='cuda')
        AF._call('arflow_census_fwd', same.data_ptr(), same.data_ptr(), None, ham.data_ptr(), None, None, B, H, W, R, AF._stream())
        assert float(ham.abs().max()) == 0.0


@pytest.mark.parametrize('case', C.E2E_STANDALONE, ids=lambda c: 'R%d-%dx%dx%d' % c)
def test_census_loss_end_to_end(AF, case):
    """uflow_utils.census_loss: one forward, one backward launch per image"""
    from arflow_amd import uflow_utils
    R, B, H, W = case
    im_a, im_b, mask = C.image('S', B, H, W, 0), C.image('S', B, H, W, 1), C.user_mask(B, H, W)
    ref0 = C.standalone_ref(im_a, im_b, R, mask=mask, fold_fp32=True)
    sc = 1.0 / float(ref0.sums[1] + 1e-6)
    a, b = cu(im_a).requires_grad_(True), cu(im_b).requires_grad_(True)
    loss = uflow_utils.census_loss(a, b, cu(mask), 2 * R + 1)
    ga_, gb_ = torch.autograd.grad(loss, [a, b])
    assert_within(loss, ref0.loss, ref0.loss_bound, 'standalone e2e loss', str(case))
    rel = float((ref0.dham_bound / ref0.dham.clamp_min(1e-300))[ref0.dham > 0].max())
    for got, (x, y), name in ((gb_, (im_a, im_b), 'd im_b'), (ga_, (im_b, im_a), 'd im_a')):
        ref = C.standalone_ref(x, y, R, mask=mask, w=ref0.dham, scale=sc, fold_fp32=True)
        bound = ref.grad_bound + ref.g_abs * (rel + 8 * U + float(ref0.sums_bound[1] / (ref0.sums[1] + 1e-6)))
        assert_within(got, ref.grad, bound, 'standalone e2e ' + name, str(case))
