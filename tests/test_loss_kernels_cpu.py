"""CPU: everything tests/test_loss_kernels_gpu.py rests on, checked without a GPU.

1. Pins: the float64 references of tests/loss_kernels_ref.py reproduce the frozen results of the reference
   (tests/golden/photo.npz, masks.npz, aux.npz) within the fp32 rounding those fixtures carry, and agree with oracle.ops
   evaluated in float64 at ragged sizes.
2. The bounds are not too tight: for every input of the GPU tests the fp32 CPU evaluation of oracle.ops -- the arithmetic the
   kernels restate -- lies inside the stated bound with 4x room.
3. The inputs discriminate: a deliberately wrong reference (one subtle mutation at a time) leaves the true reference by more
   than 100x the bound in at least one element, for every GPU test input the mutation applies to -- so a kernel with that
   mistake fails the GPU test.
4. The exclusion caps (elements left out of a comparison) hold for the references alone.
5. C-ABI argument validation of the entry points these kernels sit behind (validation precedes any launch).
"""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import ops
from tests import loss_kernels_ref as R

U = R.U
D = torch.float64
ROOM, FAR = 4.0, 100.0


# ---- oracle.ops, any dtype, in the kernels' parametrisation ----------------------------------------------------------
def oracle_sums(flow, img, flow_scale, alpha, order, wmode, penalty):
    """the two smoothness sums as oracle.ops composes them (ops.smooth_grad_1st / smooth_grad_2nd for wmode 0,
    oracle.losses._smooth_terms_uflow for wmode 1), un-normalised, flow_scale on the difference"""
    pen = (lambda v: v.abs()) if penalty == 0 else ops.penalty_uflow
    if order == 1:
        wx, wy = ops._edge_weights(img, alpha)
        dx, dy = ops.gradient(flow)
    elif wmode == 0:
        wx, wy = ops._edge_weights(img, alpha)
        wx, wy = wx[:, :, :, 1:], wy[:, :, 1:, :]
        fx, fy = ops.gradient(flow)
        dx, dy = ops.gradient(fx)[0], ops.gradient(fy)[1]
    else:
        igx, igy = ops.image_grads(img, stride=2)
        wx = torch.exp(-(alpha * igx).abs().mean(1, keepdim=True))
        wy = torch.exp(-(alpha * igy).abs().mean(1, keepdim=True))
        fx, fy = ops.image_grads(flow)
        dx, dy = ops.image_grads(fx)[0], ops.image_grads(fy)[1]
    return torch.stack([(wx * pen(dx * flow_scale)).sum(), (wy * pen(dy * flow_scale)).sum()])


def oracle_sums_and_grad(flow, img, *args):
    f = flow.clone().requires_grad_(True)
    s = oracle_sums(f, img, *args)
    g, = torch.autograd.grad(R.COEF[0] * s[0] + R.COEF[1] * s[1], [f])
    return s.detach(), g


def smooth_inputs():
    """every (tag, flow, img, flow_scale, kind) the GPU smoothness tests use (modes and alphas are looped by the caller)"""
    for shape in R.SMALL_SHAPES + [R.STRIDED_SHAPE]:
        B, Ci, H, W = shape
        img = R.smooth_image(*shape)
        for k, fs in enumerate(R.Q_SCALES):
            yield 'Q%s fs%g' % (shape, fs), R.smooth_flow('Q', B, H, W), img, fs, 'Q'
        yield 'R%s' % (shape,), R.smooth_flow('R', B, H, W), img, R.R_SCALE, 'R'
    # the fused splat + smoothness launch and the level-2 grids of the one-launch backward (flow_scale 1, 3 channels)
    for B, H, W in R.SPLAT_SMOOTH_SHAPES + [(b, h // 4, w // 4) for b, h, w in R.PAIR_SHAPES]:
        flow, img = R.splat_smooth_inputs(B, H, W)
        yield 'splat-smooth R%s' % ((B, H, W),), flow, img, 1.0, 'R'
    for B, H, W in [(b, h // 4, w // 4) for b, h, w in R.PAIR_SHAPES]:
        yield 'pair Q%s' % ((B, H, W),), R.smooth_flow('Q', B, H, W), R.smooth_image(B, 3, H, W), 1.0, 'Q'


def close(a, b, atol, rtol, what):
    err = (a.to(D) - b.to(D)).abs()
    tol = atol + rtol * b.to(D).abs()
    assert bool((err <= tol).all()), '%s: worst err %.3e (tol %.3e)' % (what, float(err.max()), float(tol.max()))


# ---- 1. pins ---------------------------------------------------------------------------------------------------------
def test_smooth_ref_reproduces_the_reference_fixtures(golden):
    """photo.npz holds fp32 results: a mean over n ~ 500 terms carries about log2(n) u ~ 1e-6 relative, a gradient element
    a few u of the largest one.  Bounds: 3e-6 relative on the values, 3e-6 of max |ref| + 1e-5 relative on the gradients."""
    g = golden('photo')
    for name in g.names():
        im1, fl = g[name + '_im1'], g[name + '_flow']
        B, _, H, W = fl.shape
        for key, order, penalty, div in (('sm1_abs', 1, 0, 4.0), ('sm1_uflow', 1, 1, 4.0), ('sm2', 2, 0, 2.0)):
            coef = (1.0 / (div * B * 2 * H * (W - order)), 1.0 / (div * B * 2 * (H - order) * W))
            r = R.smooth_ref(fl, im1, 1.0, 10.0, order, 0, penalty, coef=coef)
            val = coef[0] * r.sums[0] + coef[1] * r.sums[1]
            ref, rg = g['%s_%s' % (name, key)], g['%s_%s_gf' % (name, key)]
            close(val, ref, 0, 3e-6, name + ' ' + key)
            close(r.grad, rg, 3e-6 * float(rg.abs().max()), 1e-5, name + ' ' + key + ' grad')


def test_splat_and_mask_refs_reproduce_the_reference_fixtures(golden):
    """masks.npz: a range map cell is a sum of <= ~10 fp32 weights of at most 1 (a few u each: 2e-6 + 1e-5 relative covers
    it, the oracle's own pin uses 1e-6 + 1e-5); masks are exact; the bidirectional mask outside its 1e-4 margin band."""
    g = golden('masks')
    for name in g.names():
        fl = g[name + '_flow']
        H, W = fl.shape[2:]
        coords = R.abs_coords(fl)
        close(R.splat_ref(coords, H, W, 0)[0], g[name + '_range_map'], 2e-6, 1e-5, name + ' range map')
        close(R.splat_ref(coords, H, W, 1)[0], g[name + '_corr_map'], 2e-6, 1e-5, name + ' corr map')
        assert torch.equal(R.coord_mask_ref(fl, 1), g[name + '_border_mask']), name
        assert torch.equal(R.coord_mask_ref(coords, 3), g[name + '_border_mask']), name
        dec, margin = R.occ_bidir_ref(fl, (-0.7 * fl.flip(-1)).contiguous())
        safe = margin > 1e-4
        assert float(safe.float().mean()) > 0.97
        assert torch.equal(dec[safe], g[name + '_occ_bidir'][safe]), name


def test_resize_refs_reproduce_the_reference_fixtures(golden):
    g = golden('aux')
    close(R.down4_ref(g['img']), g['down4'], 4 * U, 0, 'down4')  # |img| <= 1: three roundings
    close(R.up4_clamp_mul_ref(g['m']), g['up4'], 8 * U, 0, 'up4')


def test_refs_agree_with_the_oracle_in_float64():
    gen = torch.Generator().manual_seed(5)
    B, Ci, H, W = 2, 4, 7, 11
    img, flow = torch.rand(B, Ci, H, W, generator=gen).double(), torch.randn(B, 2, H, W, generator=gen).double()
    for order, wmode, penalty in R.MODES:
        for fs in (1.0, 0.3):
            s, gr = oracle_sums_and_grad(flow, img, fs, 7.0, order, wmode, penalty)
            r = R.smooth_ref(flow, img, fs, 7.0, order, wmode, penalty)
            close(r.sums, s, 0, 1e-13, 'sums %s' % ((order, wmode, penalty),))
            close(r.grad, gr, 1e-14, 1e-12, 'grad')
            assert bool((r.g_abs >= r.grad.abs() * (1 - 1e-12)).all())
    # multiples of 1/64: x + u is exact in fp32, so the float64 oracle sees the same coordinates
    fl = torch.round(3.0 * torch.randn(2, 2, 9, 13, generator=gen) * 64) / 64
    coords = R.abs_coords(fl)
    close(R.splat_ref(coords, 9, 13, 0)[0], ops.compute_range_map(fl.double()), 1e-14, 1e-13, 'range map')
    close(R.splat_ref(coords, 9, 13, 1)[0], ops.get_corresponding_map(coords.double()), 1e-14, 1e-13, 'corr map')
    assert int(R.splat_ref(coords, 9, 13, 0)[1].sum()) <= 4 * fl.numel() // 2
    assert torch.equal(R.coord_mask_ref(fl, 1), ops.border_mask(fl))
    assert torch.equal(R.coord_mask_ref(fl, 0), ops.mask_invalid(ops.flow_to_warp(fl)))
    f21 = -fl + 0.45 * torch.randn(2, 2, 9, 13, generator=gen)
    for scale, bias in ((0.01, 0.5), (0.05, 1.5)):
        dec, margin = R.occ_bidir_ref(fl, f21, scale, bias)
        want = ops.get_occu_mask_bidirection(fl.double(), f21.double(), scale, bias)
        assert torch.equal(dec[margin > 1e-9].double(), want[margin > 1e-9])
        assert 0 < float(dec.mean()) < 1
    small = 2.5 * torch.randn(2, 1, 3, 5, generator=gen)
    close(R.up4_clamp_mul_ref(small), ops.upsample(small.double().clamp(0, 1), False, 4.0), 1e-15, 0, 'up4')
    img = torch.randn(2, 3, 8, 12, generator=gen)
    close(R.down4_ref(img), ops.downsample(img.double(), False, 4.0), 1e-15, 0, 'down4')
    close(R.gray255_ref(img), ops.rgb_to_grayscale(img.double()) * 255, 1e-12, 0, 'gray')


# ---- 2.-4. smoothness ------------------------------------------------------------------------------------------------
def test_smooth_inputs_are_what_the_bounds_assume():
    for shape in R.SMALL_SHAPES + R.ROW_SHAPES:
        B, Ci, H, W = shape
        q = R.smooth_flow('Q', B, H, W)
        for axis in (2, 3):
            for order in (1, 2):
                if q.shape[axis] <= order:
                    continue
                d32, d64 = q, q.double()
                for _ in range(order):
                    n = d32.shape[axis] - 1
                    d32 = d32.narrow(axis, 1, n) - d32.narrow(axis, 0, n)
                    d64 = d64.narrow(axis, 1, n) - d64.narrow(axis, 0, n)
                assert torch.equal(d32.double(), d64), 'class Q: a difference is not exact in fp32'
                for fs in R.Q_SCALES:
                    assert torch.equal((d32 * fs).double(), d64 * fs)
        if H >= 4 and W >= 6:
            assert float((q[:, :, :H // 2, 1:W // 3] - q[:, :, :H // 2, :W // 3 - 1]).abs().max()) == 0.0
    # the weights span 1e-20 .. 1 at both alphas
    img = R.smooth_image(2, 4, 5, 257)
    for alpha in R.ALPHAS:
        r = R.smooth_ref(R.smooth_flow('R', 2, 5, 257), img, 1.0, alpha, 1, 0, 0)
        w = torch.exp(-r.expo[0])
        assert float(w.max()) > 0.5 and float(w.min()) < (1e-19 if alpha == 150.0 else 0.06), (alpha, float(w.min()))
    assert [R.smooth_rows(s[0], s[2], s[3]) for s in R.ROW_SHAPES] == [2, 8]
    assert all(s[2] % R.smooth_rows(s[0], s[2], s[3]) == 1 for s in R.ROW_SHAPES)
    assert all(R.smooth_rows(s[0], s[2], s[3]) == 1 for s in R.SMALL_SHAPES)


def check_smooth_case(tag, flow, img, fs, kind, mode, alpha, mutations=True):
    order, wmode, penalty = mode
    thr = R.small_threshold(flow, fs) if kind == 'R' else None
    r = R.smooth_ref(flow, img, fs, alpha, order, wmode, penalty, small_thr=thr)
    sb, gb = R.smooth_sum_bound(r), R.smooth_grad_bound(r, kind == 'R')
    keep = ~r.touchy
    if kind == 'R':
        assert float(r.touchy.float().mean()) <= 0.005, '%s: %.4f of the elements left out' % (tag, float(r.touchy.float().mean()))
    # 2. fp32 oracle inside the bound with 4x room
    s32, g32 = oracle_sums_and_grad(flow.float().contiguous(), img.float(), fs, alpha, order, wmode, penalty)
    ws = R.worst((s32.double() - r.sums).abs(), sb)
    wg = R.worst(((g32.double() - r.grad).abs())[keep], gb[keep])
    assert ws * ROOM <= 1.0 and wg * ROOM <= 1.0, '%s: fp32 oracle at %.3f (sums), %.3f (grad) of the bound' % (tag, ws, wg)
    if kind == 'Q':
        assert float(g32[r.g_abs == 0].abs().max() if bool((r.g_abs == 0).any()) else 0.0) == 0.0
    if not mutations:
        return ws, wg
    # 3. mutations
    B, _, H, W = flow.shape
    muts = [('lastcol', dict(mutate='lastcol'))]
    if order == 2:
        muts += [('wmode', dict(wmode=1 - wmode)), ('stencil', dict(mutate='stencil'))]
    if img.shape[1] != 3:
        muts.append(('div3', dict(mutate='div3')))
    if penalty == 1 and fs != 1.0:
        muts.append(('scale_after', dict(mutate='scale_after')))
    if H * W < 64:  # (1x1, 2x2, 3x3: there for the empty sums and the borders; a handful of terms cannot tell every mutation)
        muts = []
    for name, kw in muts:
        args = dict(wmode=wmode, small_thr=None)
        args.update(kw)
        m = R.smooth_ref(flow, img, fs, alpha, order, args.pop('wmode'), penalty, **args)
        far = max(R.worst((m.sums - r.sums).abs(), sb), R.worst((m.grad - r.grad).abs()[keep], gb[keep]))
        assert far > FAR, '%s: mutation %s stays within %.1f x the bound' % (tag, name, far)
    return ws, wg


@pytest.mark.parametrize('alpha', R.ALPHAS)
def test_smooth_bounds_and_mutations_small_shapes(alpha):
    for tag, flow, img, fs, kind in smooth_inputs():
        for mode in R.MODES:
            check_smooth_case('%s %s alpha %g' % (tag, mode, alpha), flow, img, fs, kind, mode, alpha)


@pytest.mark.parametrize('kind,fs', [('Q', 0.25), ('R', R.R_SCALE)], ids=['Q', 'R'])
@pytest.mark.parametrize('shape', R.ROW_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_smooth_bounds_and_mutations_row_merging_shapes(shape, kind, fs):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    B, Ci, H, W = shape
    img = R.smooth_image(*shape)
    flow = R.smooth_flow(kind, B, H, W)
    for mode in R.ROW_MODES:
        for alpha in R.ALPHAS:  # (the mutations once per mode: at alpha 150, UFlowLoss's edge constant)
            check_smooth_case('%s%s %s alpha %g' % (kind, shape, mode, alpha), flow, img, fs, kind, mode, alpha,
                              mutations=alpha == 150.0)


# ---- 2.-4. splat -----------------------------------------------------------------------------------------------------
def test_splat_bounds_and_mutation():
    cases = dict(R.splat_cases())
    cases.update(('smooth %dx%dx%d' % shp, (R.splat_smooth_inputs(*shp)[0], None)) for shp in R.SPLAT_SMOOTH_SHAPES)
    for name, (flow, n_add) in cases.items():
        B, _, H, W = flow.shape
        coords = R.abs_coords(flow)
        for variant in (0, 1):
            ref, cnt = R.splat_ref(coords, H, W, variant)
            bound = R.splat_bound(ref, cnt, n_add)
            got = ops.compute_range_map(flow.contiguous()) if variant == 0 else ops.get_corresponding_map(coords)
            w = R.worst((got.double() - ref).abs(), bound)
            assert w * ROOM <= 1.0, '%s variant %d: fp32 oracle at %.3f of the bound' % (name, variant, w)
            assert float(got[cnt == 0].abs().max() if bool((cnt == 0).any()) else 0.0) == 0.0
            mut = R.splat_ref(coords, H, W, variant, mutate='edge')[0]
            far = R.worst((mut - ref).abs(), bound)
            if name != 'collapse' and H * W >= 64:  # (nothing lands on the last column there; 1 x 1 has no neighbour)
                assert far > FAR, '%s variant %d: a dropped edge tap stays within %.1f x the bound' % (name, variant, far)
    # what the cases are there to reach
    spread = R.abs_coords(R.splat_cases()['spread'][0])
    for ty in range(8):
        for tx in range(5):
            t = spread[0, :, ty * 8:ty * 8 + 8, tx * 32:tx * 32 + 32]
            ok = (t[0] > -1) & (t[0] < 160) & (t[1] > -1) & (t[1] < 64)
            xs, ys = t[0][ok], t[1][ok]
            assert float(xs.max() - xs.min()) > 130 or float(ys.max() - ys.min()) > 66, 'spread: a tile fits the LDS window'
    edge = R.abs_coords(R.splat_cases()['edge'][0])[0]
    for v in (0.0, 39.0, -1.0, 40.0, -0.5, 39.5):
        assert bool((edge[0] == v).any())
    for v in (0.0, 5.0, -1.0, 6.0, -0.5, 5.5):
        assert bool((edge[1] == v).any())


# ---- 2.-4. masks -----------------------------------------------------------------------------------------------------
def test_mask_inputs_and_mutation():
    for B, H, W in R.MASK_SHAPES + R.COORD_ONLY_SHAPES:
        fl = R.coord_mask_flow(B, H, W)
        coords = R.abs_coords(fl)
        for mode in range(4):
            ref = R.coord_mask_ref(coords if mode & 2 else fl, mode)
            want = ops.border_mask(fl) if mode & 1 else ops.mask_invalid(ops.flow_to_warp(fl))
            assert torch.equal(ref, want)
            assert not torch.equal(ref, R.coord_mask_ref(coords if mode & 2 else fl, mode, mutate='swap')), (B, H, W, mode)
    for B, H, W in R.MASK_SHAPES:
        f12, f21 = R.occ_flows(B, H, W)
        for scale, bias in ((0.01, 0.5), (0.05, 1.5)):
            dec, margin = R.occ_bidir_ref(f12, f21, scale, bias)
            band = margin <= 1e-4
            assert float(band.float().mean()) <= 0.005, (B, H, W)
            got = ops.get_occu_mask_bidirection(f12, f21, scale, bias)
            assert torch.equal(got[~band], dec[~band]), (B, H, W)
            if (scale, bias) == (0.01, 0.5):
                assert 0.65 <= float(dec.mean()) <= 0.92, (B, H, W, float(dec.mean()))
            else:
                assert 0.05 <= float(dec.mean()) <= 0.95, (B, H, W, float(dec.mean()))


# ---- 2.-4. resize helpers --------------------------------------------------------------------------------------------
def test_resize_bounds_and_mutations():
    for B, h, w in R.UP4_SHAPES:
        small, valid = R.up4_inputs(B, h, w)
        if small.numel() >= 100:  # roughly a third on each side of the clamp
            assert float((small < 0).float().mean()) > 0.15 and float((small > 1).float().mean()) > 0.15
        for v in (None, valid):
            ref = R.up4_clamp_mul_ref(small, v)
            got = ops.upsample(small.clamp(0, 1), False, 4.0)
            got = got if v is None else got * v
            bound = 8 * U * (1.0 if v is None else v.abs().double())
            wr = R.worst((got.double() - ref).abs(), bound)
            assert wr * ROOM <= 1.0, ('up4', B, h, w, wr)
            far = R.worst((R.up4_clamp_mul_ref(small, v, mutate='noclamp') - ref).abs(), bound)
            assert far > FAR, ('up4 without the clamp', B, h, w, far)
            if v is not None and small.numel() > 8:  # (2 x 1 x 1: both values may clamp to 0)
                far = R.worst((R.up4_clamp_mul_ref(small, v, mutate='novalid') - ref).abs(), bound)
                assert far > FAR, ('up4 ignoring valid', B, h, w, far)
    for B, H, W in R.DOWN4_SHAPES:
        img = R.down4_input(B, H, W)
        mx = float(img.abs().max())
        wr = R.worst((ops.downsample(img, False, 4.0).double() - R.down4_ref(img)).abs(), 4 * U * mx)
        assert wr * ROOM <= 1.0, ('down4', B, H, W, wr)
        wr = R.worst(((ops.rgb_to_grayscale(img) * 255).double() - R.gray255_ref(img)).abs(), 6 * U * 255 * mx)
        assert wr * ROOM <= 1.0, ('gray', B, H, W, wr)
        assert torch.equal(R.down4_ref(img), F.interpolate(img.double(), scale_factor=0.25, mode='bilinear', align_corners=False))


# ---- 5. argument errors ----------------------------------------------------------------------------------------------
ENULL, ESHAPE, EPARAM = -1001, -1002, -1003


@pytest.fixture(scope='module')
def lib():
    from arflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_argument_errors_without_gpu(lib):
    """validation happens before any launch, so these are safe on a CPU-only host (tests/test_abi_cpu.py)"""
    one = ctypes.c_void_p(16)
    H, W = 8, 8

    def smooth(name, **kw):  # (flow, img, sums) / (flow, img, coef, gflow), B, Ci, H, W, fbs, fscale, alpha, order, wmode, penalty
        a = dict(ptrs=[one] * (3 if name == 'arflow_smooth_fwd' else 4), B=1, Ci=3, fbs=2 * H * W, order=1, wmode=0, penalty=0)
        a.update(kw)
        return getattr(lib, name)(*a['ptrs'], a['B'], a['Ci'], H, W, a['fbs'], 1.0, 10.0, a['order'], a['wmode'], a['penalty'], None)

    def nulls(n):
        return [[None if j == i else one for j in range(n)] for i in range(n)]

    for name, n in (('arflow_smooth_fwd', 3), ('arflow_smooth_bwd', 4)):
        for p in nulls(n):
            assert smooth(name, ptrs=p) == ENULL, name
        assert smooth(name, B=0) == ESHAPE and smooth(name, fbs=2 * H * W - 1) == ESHAPE, name
        assert smooth(name, order=3) == EPARAM and smooth(name, wmode=2) == EPARAM and smooth(name, penalty=2) == EPARAM, name

    def flow_map(name, ptrs=(one, one), B=1, fbs=2 * H * W, last=0):
        return getattr(lib, name)(*ptrs, B, H, W, fbs, last, None)

    for name in ('arflow_splat_map', 'arflow_coord_mask'):
        for p in nulls(2):
            assert flow_map(name, ptrs=p) == ENULL, name
        assert flow_map(name, B=0) == ESHAPE and flow_map(name, fbs=2 * H * W - 1) == ESHAPE, name
        assert flow_map(name, last=4) == EPARAM and flow_map(name, last=-1) == EPARAM, name

    def splat_smooth(ptrs=(one,) * 4, B=1, fbs=2 * H * W, order=1, wmode=1, penalty=1):
        return lib.arflow_splat_smooth_fwd(*ptrs, B, H, W, fbs, 1.0, 150.0, order, wmode, penalty, 0, None)

    for p in nulls(4):
        assert splat_smooth(ptrs=p) == ENULL
    assert splat_smooth(B=0) == ESHAPE and splat_smooth(fbs=2 * H * W - 1) == ESHAPE
    assert splat_smooth(order=3) == EPARAM and splat_smooth(wmode=2) == EPARAM and splat_smooth(penalty=2) == EPARAM

    def occ(ptrs=(one,) * 3, B=1, s12=2 * H * W, s21=2 * H * W):
        return lib.arflow_occ_bidir(*ptrs, B, H, W, s12, s21, 0.01, 0.5, None)

    for p in nulls(3):
        assert occ(ptrs=p) == ENULL
    assert occ(B=0) == ESHAPE and occ(s12=2 * H * W - 1) == ESHAPE and occ(s21=2 * H * W - 1) == ESHAPE

    assert lib.arflow_up4_clamp_mul(None, None, one, 1, 2, 2, None) == ENULL
    assert lib.arflow_up4_clamp_mul(one, None, None, 1, 2, 2, None) == ENULL
    assert lib.arflow_up4_clamp_mul(one, None, one, 0, 2, 2, None) == ESHAPE
    assert lib.arflow_up4_clamp_mul(one, None, one, 1, 16384, 2, None) == ESHAPE  # 4 h = 65536 > 65535 (the grid's y extent)

    assert lib.arflow_down4_gray_z(None, one, one, one, 1, 8, 8, None) == ENULL
    assert lib.arflow_down4_gray_z(one, one, None, one, 1, 8, 8, None) == ENULL
    assert lib.arflow_down4_gray_z(one, one, one, one, 0, 8, 8, None) == ESHAPE
    assert lib.arflow_down4_gray_z(one, one, one, one, 1, 6, 8, None) == ESHAPE  # H = 6: not a multiple of 4
    assert lib.arflow_down4_gray_z(one, one, one, one, 1, 8, 6, None) == ESHAPE
