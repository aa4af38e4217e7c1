"""GPU: the standalone loss kernels -- edge-aware smoothness, the forward splat, the coordinate / occlusion masks and the x4
resize helpers -- against the float64 references of tests/loss_kernels_ref.py, off the sizes of the golden fixtures: several
rows per workgroup and the second 256-column block of arflow_smooth_fwd, a runtime channel count, second order with both
weight forms and both penalties, strided flows, the default-mode splat kernels (fused with the smoothness sums or not,
LDS window and direct-atomic fallback), the smoothness role of the one-launch UFlowLoss backward with two x-blocks, the
128- and 256-thread blocks of the mask kernels, and the clamp / valid factor / zero plane of the resize helpers.

Bounds (u = 2^-24; derivations with the functions in tests/loss_kernels_ref.py, checked without a GPU in
tests/test_loss_kernels_cpu.py: the fp32 oracle sits inside each with 4x room, a subtly wrong reference leaves each by > 100x):
  smoothness term   r_t = (alpha s_t + 4) 2u: the rounded argument of __expf and its product with log2(e), v_exp_f32 at one
                    ulp (the ISA document's figure), pen / dpen and one multiply
  smoothness sums   |got - ref| <= sum_t t r_t + 64u sum_t t   (non-negative terms; 64 >= the depth of the summation tree)
  gradient, class Q |got - ref| <= G_abs (max r_t over the element's terms + 16u); where G_abs = 0 the result is exactly 0
  gradient, class R the same + the conditioning of the penalty-1 derivative; elements whose stencil touches a difference
                    with |v| < 1e-4 flow_scale max|flow| are left out (at most 0.5 %)
  splat             per cell count 2^-22 + n_add u value; a cell nothing lands on is exactly 0
  coord_mask        exact; occ_bidir exact wherever the reference's margin |lhs - rhs| / (lhs + rhs) exceeds 1e-4 (<= 0.5 % inside)
  up4_clamp_mul     8u (times |valid|): three lerps of values in [0, 1];  down4 4u max|img|;  grey 6u 255 max|img|
No bound here was taken from what the kernels give.  Every test leaves deterministic mode off."""
import pytest
import torch

from tests import loss_kernels_ref as R

pytestmark = pytest.mark.gpu
U = R.U
SITES = {}


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


def assert_within(got, ref, bound, site, tag, keep=None):
    """elementwise |got - ref| <= bound; prints the worst err / bound of the call and keeps the worst per site"""
    err = (got.detach().cpu().double() - ref.double()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    if keep is not None:
        err, bound = err[keep], bound[keep]
    w = R.worst(err, bound)
    SITES[site] = max(SITES.get(site, 0.0), w)
    print('%s | %s: max err %.3e, worst err/bound %.4f' % (site, tag, float(err.max()) if err.numel() else 0.0, w))
    assert bool((err <= bound).all()), '%s | %s: %d elements out of bound, worst err/bound %.3f' % (
        site, tag, int((~(err <= bound)).sum()), w)


# ---- smoothness ------------------------------------------------------------------------------------------------------
def smooth_gpu(AF, flow, img, fs, alpha, mode, strided=False):
    """-> (sums, gradient w.r.t. the tensor handed over) with cotangent R.COEF"""
    leaf = cu(R.strided(flow) if strided else flow).requires_grad_(True)
    f = leaf[:, 2:4] if strided else leaf
    if strided:
        assert AF._flow_view(f)[1] == 4 * flow.shape[2] * flow.shape[3], 'the slice is consumed in place'
    s = AF.smooth_sums(f, cu(img), fs, alpha, *mode)
    g, = torch.autograd.grad(s, [leaf], torch.tensor(R.COEF, device='cuda'))
    return s.detach(), g


def check_smooth(AF, tag, flow, img, fs, kind, mode, alpha, strided=False):
    thr = R.small_threshold(flow, fs) if kind == 'R' else None
    ref = R.smooth_ref(flow, img, fs, alpha, *mode, small_thr=thr)
    s, g = smooth_gpu(AF, flow, img, fs, alpha, mode, strided)
    tag = '%s %s fs %.3g mode %s alpha %g' % (kind, tag, fs, mode, alpha)
    assert_within(s, ref.sums, R.smooth_sum_bound(ref), 'smooth sums', tag)
    if strided:
        assert float(g[:, 0:2].abs().max()) == 0.0, tag + ': the other two channels get no gradient'
        g = g[:, 2:4]
    keep = None
    if kind == 'R':
        assert float(ref.touchy.float().mean()) <= 0.005, tag
        keep = ~ref.touchy
    else:
        # an element ALL of whose contributions are exactly 0 in the reference (v = 0 on the constant patch, or no term at
        # all) must come back exactly 0.  (A reference element that is 0 only because two equal weights cancel -- the image
        # is piecewise linear, so neighbouring weights often agree to the bit -- is held to the bound below instead: the
        # kernel adds the x and y contributions in one fma chain, ((a + b) - a) - b, which leaves a rounding residue;
        # measured 3.0e-8 .. 4.8e-7 on such elements at G_abs ~ 0.2 .. 5.)
        zero = ref.g_abs == 0
        if flow.shape[2] >= 4 and flow.shape[3] >= 6:
            assert bool(zero.any()), tag + ': the constant patch has interior elements'
        assert float(g.cpu()[zero].abs().max() if bool(zero.any()) else 0.0) == 0.0, tag + ': an exactly-zero gradient element'
    assert_within(g, ref.grad, R.smooth_grad_bound(ref, kind == 'R'), 'smooth grad ' + kind, tag, keep)
    return ref, s, g


@pytest.mark.parametrize('shape', R.SMALL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_smooth_small_shapes(AF, shape):
    """every (order, wmode, penalty), both alphas, both flow classes: one row per workgroup, 1 .. 3 x-blocks, and the
    runtime-channel path chan_absdiff<0> wherever Ci != 3"""
    B, Ci, H, W = shape
    img = R.smooth_image(*shape)
    flows = [('Q', R.smooth_flow('Q', B, H, W), fs) for fs in R.Q_SCALES] + [('R', R.smooth_flow('R', B, H, W), R.R_SCALE)]
    for kind, flow, fs in flows:
        for mode in R.MODES:
            for alpha in R.ALPHAS:
                ref, s, g = check_smooth(AF, str(shape), flow, img, fs, kind, mode, alpha)
                if max(H, W) <= mode[0]:  # no term at all: sums and gradient exactly 0
                    assert float(s.abs().max()) == 0.0 and float(g.abs().max()) == 0.0


def test_smooth_strided_flow(AF):
    """the flow is channels 2:4 of a [2,4,5,257] tensor (flow_bstride = 4 H W; the other channels hold NaN)"""
    B, Ci, H, W = R.STRIDED_SHAPE
    img = R.smooth_image(*R.STRIDED_SHAPE)
    for kind, fs in (('Q', 4.0), ('R', R.R_SCALE)):
        flow = R.smooth_flow(kind, B, H, W)
        for mode in R.MODES:
            for alpha in R.ALPHAS:
                check_smooth(AF, 'strided', flow, img, fs, kind, mode, alpha, strided=True)


@pytest.mark.parametrize('kind,fs', [('Q', 0.25), ('R', R.R_SCALE)], ids=['Q', 'R'])
@pytest.mark.parametrize('shape', R.ROW_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_smooth_rows_merged_per_workgroup(AF, shape, kind, fs):
    """rows = 2 and 8 rows per workgroup of smooth_fwd_kernel, H % rows = 1: the last workgroup leaves its loop early"""
    B, Ci, H, W = shape
    rows = R.smooth_rows(B, H, W)
    assert rows == {129: 2, 257: 8}[H] and H % rows == 1
    img = R.smooth_image(*shape)
    flow = R.smooth_flow(kind, B, H, W)
    for mode in R.ROW_MODES:
        for alpha in R.ALPHAS:
            check_smooth(AF, 'rows=%d %s' % (rows, shape), flow, img, fs, kind, mode, alpha)


# ---- fused splat + smoothness ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', R.SPLAT_SMOOTH_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_splat_smooth_default_mode(AF, shape):
    """splat_kernel<true>: partial 8 x 32 tiles, padding workgroups ((5,8,32): 5 tiles on a grid of 8), and the sums of a
    different kernel and summation tree than arflow_smooth_fwd"""
    B, H, W = shape
    flow, img = R.splat_smooth_inputs(B, H, W)
    rm_ref, cnt = R.splat_ref(R.abs_coords(flow), H, W, 0)
    rm_bound = R.splat_bound(rm_ref, cnt)
    for mode in R.SPLAT_SMOOTH_MODES:
        ref = R.smooth_ref(flow, img, 1.0, 150.0, *mode)
        sb = R.smooth_sum_bound(ref)
        plain = AF.smooth_sums(cu(flow), cu(img), 1.0, 150.0, *mode)
        for pre in (False, True):
            tag = '%s order %d %s' % (shape, mode[0], 'pre-zeroed' if pre else 'cleared inside')
            plane = torch.zeros(B, 1, H, W, device='cuda') if pre else None
            s, rm = AF.splat_smooth(cu(flow), cu(img), plane, 1.0, 150.0, *mode)
            assert_within(s, ref.sums, sb, 'splat_smooth sums', tag)
            assert_within(s, plain.cpu(), 2 * sb, 'splat_smooth sums vs smooth_sums', tag)
            assert_within(rm, rm_ref, rm_bound, 'splat_smooth range map', tag)
            assert float(rm.cpu()[cnt == 0].abs().max() if bool((cnt == 0).any()) else 0.0) == 0.0, tag
    if shape == (3, 17, 65):  # deterministic mode runs arflow_smooth_fwd itself: there the equality stays bitwise
        with AF.deterministic():
            s, rm = AF.splat_smooth(cu(flow), cu(img), None, 1.0, 150.0, 1, 1, 1)
            plain = AF.smooth_sums(cu(flow), cu(img), 1.0, 150.0, 1, 1, 1)
        assert torch.equal(s, plain)
        assert_within(rm, rm_ref, rm_bound, 'splat_smooth range map (deterministic)', str(shape))


# ---- splat -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(R.splat_cases()))
def test_splat_map_default_mode(AF, name):
    flow, n_add = R.splat_cases()[name]
    B, _, H, W = flow.shape
    coords = R.abs_coords(flow)
    for variant in (0, 1):
        ref, cnt = R.splat_ref(coords, H, W, variant)
        bound = R.splat_bound(ref, cnt, n_add)
        for absolute in (False, True):
            src = coords if absolute else flow
            if name == 'strided':
                g = cu(R.strided(src))[:, 2:4]
                assert AF._flow_view(g)[1] == 4 * H * W
            else:
                g = cu(src)
            got = AF.splat_map(g, variant | (2 if absolute else 0))
            tag = '%s variant %d' % (name, variant | (2 if absolute else 0))
            assert_within(got, ref, bound, 'splat_map ' + name, tag)
            assert float(got.cpu()[cnt == 0].abs().max() if bool((cnt == 0).any()) else 0.0) == 0.0, tag


# ---- the smoothness role of the one-launch UFlowLoss backward --------------------------------------------------------
@pytest.mark.parametrize('family', ['column', 'ordered'])
@pytest.mark.parametrize('shape', R.PAIR_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_uflow_pair_backward_smoothness_role(AF, shape, family, monkeypatch):
    """pair_bwd_smooth_col_kernel (default) and pair_bwd_smooth_kernel decode (b, y, x-block) from a linear workgroup id:
    w2 = 257 gives two x-blocks.  Zero census cotangents leave the level-2 gradient to the smoothness role alone: within the
    gradient bound of the reference, and bit for bit arflow_smooth_bwd's (the same device function, smooth_bwd_pixel<3>)."""
    monkeypatch.setenv('ARFLOW_CENSUS_COL', {'ordered': '0', 'column': '1'}[family])
    B2, H, W = shape
    h, w = H // 4, W // 4
    gen = torch.Generator().manual_seed(77 + W)
    gray = 255.0 * torch.rand(B2, 1, H, W, generator=gen)
    flow0 = 2.0 * torch.randn(B2, 2, H, W, generator=gen)
    small = R.smooth_image(B2, 3, h, w)
    coef = torch.tensor(R.COEF, device='cuda')
    zero = torch.zeros((), device='cuda')
    for kind in ('Q', 'R'):
        flow2 = R.smooth_flow(kind, B2, h, w)
        thr = R.small_threshold(flow2, 1.0) if kind == 'R' else None
        for order in (1, 2):
            tag = '%s %s %s order %d' % (family, shape, kind, order)
            f0, f2 = cu(flow0).requires_grad_(True), cu(flow2).requires_grad_(True)
            l0, l1, s, _ = AF.uflow_pair_loss(cu(gray), cu(small), f0, f2, None, 150.0, order)
            g2, = torch.autograd.grad([l0, l1, s], [f2], [zero, zero, coef])
            ref = R.smooth_ref(flow2, small, 1.0, 150.0, order, 1, 1, small_thr=thr)
            assert_within(s, ref.sums, R.smooth_sum_bound(ref), 'uflow_pair sums', tag)
            keep = ~ref.touchy if kind == 'R' else None
            assert_within(g2, ref.grad, R.smooth_grad_bound(ref, kind == 'R'), 'uflow_pair level-2 grad ' + kind, tag, keep)
            plain = smooth_gpu(AF, flow2, small, 1.0, 150.0, (order, 1, 1))[1]
            assert torch.equal(g2, plain), tag + ': not the gradient arflow_smooth_bwd writes'


# ---- masks -----------------------------------------------------------------------------------------------------------
def both_layouts(t):
    yield 'contiguous', cu(t)
    yield 'strided', cu(R.strided(t))[:, 2:4]


@pytest.mark.parametrize('shape', R.MASK_SHAPES + R.COORD_ONLY_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_coord_mask(AF, shape):
    """64-, 128- and 256-thread blocks (W < 96, < 192, >= 192), a second x-block (W = 257, 300), targets exactly on the
    interval ends"""
    fl = R.coord_mask_flow(*shape)
    coords = R.abs_coords(fl)
    for mode in range(4):
        src = coords if mode & 2 else fl
        ref = R.coord_mask_ref(src, mode)
        assert not torch.equal(ref, R.coord_mask_ref(src, mode ^ 1)), 'the inputs tell the two intervals apart'
        for layout, g in both_layouts(src):
            assert torch.equal(AF.coord_mask(g, mode).cpu(), ref), '%s mode %d %s' % (shape, mode, layout)


@pytest.mark.parametrize('shape', R.MASK_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_occ_bidir(AF, shape):
    f12, f21 = R.occ_flows(*shape)
    for scale, bias in ((0.01, 0.5), (0.05, 1.5)):
        dec, margin = R.occ_bidir_ref(f12, f21, scale, bias)
        safe = margin > 1e-4
        assert float((~safe).float().mean()) <= 0.005
        assert 0.0 < float(dec.mean()) < 1.0, 'both outcomes are present'
        for (la, a), (lb, b) in zip(both_layouts(f12), both_layouts(f21)):
            got = AF.occ_bidir(a, b, scale, bias).cpu()
            bad = int((got[safe] != dec[safe]).sum())
            print('occ_bidir %s scale %g bias %g %s: %d of %d differ outside the band (%d inside it)' % (
                shape, scale, bias, la, bad, int(safe.sum()), int((~safe).sum())))
            assert bad == 0
            assert bool(((got == 0) | (got == 1)).all())


# ---- resize helpers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', R.UP4_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_up4_clamp_mul(AF, shape):
    """inputs 2.5 randn: the clamp acts on both sides; with and without the valid factor; 4 w = 1028: five x-blocks"""
    small, valid = R.up4_inputs(*shape)
    assert_within(AF.up4_clamp_mul(cu(small)), R.up4_clamp_mul_ref(small), 8 * U, 'up4_clamp_mul', str(shape))
    assert_within(AF.up4_clamp_mul(cu(small), cu(valid)), R.up4_clamp_mul_ref(small, valid), 8 * U * valid.abs().double(),
                  'up4_clamp_mul valid', str(shape))


@pytest.mark.parametrize('shape', R.DOWN4_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_down4_and_gray(AF, shape):
    B, H, W = shape
    img = R.down4_input(B, H, W)
    mx = float(img.abs().max())
    small = AF.down4(cu(img))
    assert_within(small, R.down4_ref(img), 4 * U * mx, 'down4', str(shape))
    s2, gray = AF.down4_gray(cu(img))
    assert torch.equal(s2, small), 'down4_gray writes the small image of down4'
    assert_within(gray, R.gray255_ref(img), 6 * U * 255 * mx, 'down4_gray grey', str(shape))
    # the zero plane, handed over full of NaN
    s3 = torch.full_like(small, float('nan'))
    g3 = torch.full_like(gray, float('nan'))
    zero = torch.full((B, 1, H // 4, W // 4), float('nan'), device='cuda')
    gi = cu(img)
    AF._call('arflow_down4_gray_z', gi.data_ptr(), s3.data_ptr(), g3.data_ptr(), zero.data_ptr(), B, H, W, AF._stream())
    assert torch.equal(s3, small) and torch.equal(g3, gray)
    assert bool((zero == 0).all()), 'the zero plane comes back exactly 0'
    _, g4, z4 = AF.down4_gray(gi, want_small=False, zero_plane=True)
    assert torch.equal(g4, gray) and bool((z4 == 0).all())
