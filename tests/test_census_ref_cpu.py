"""CPU: everything tests/test_census_gpu.py rests on, checked without a GPU.

1. Pins: the float64 reference of tests/census_ref.py reproduces the census vectors of the frozen reference results
   (tests/golden/photo.npz, general.npz; losses.npz holds none) within the fp32 rounding those fixtures carry, and agrees with
   oracle.ops evaluated in float64 to a few float64 ulps: per-pixel distance, mask, loss and both gradients.  The restated
   fp32 sampling coordinate equals oracle.ops.resample's bit for bit.
2. The bounds are not too tight: for every input of the GPU tests the fp32 CPU evaluation of oracle.ops lies inside each
   bound with 4x room.
3. The bounds are not vacuous: each mutation of the reference leaves the true reference by more than 100x the bound on at
   least one element of every shape it can affect (exemptions are named with their reason).
4. The strip rule of census_sym.hip, restated, gives the chunk counts the GPU shapes are meant to produce.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import ops
from tests import census_ref as C

U, D = C.U, C.D
ROOM, FAR = 4.0, 100.0


def within(got, ref, bound, what, room=1.0):
    err = (got.to(D) - ref.to(D)).abs()
    b = torch.as_tensor(bound, dtype=D).expand_as(err) / room
    assert bool((err <= b).all()), '%s: worst err/bound %.3f (x%g room), max err %.3e' % (what, C.worst(err, b), room, float(err.max()))


def ulps64(a, b, n, what, scale=None):
    """|a - b| <= n float64 ulps of `scale` (default: max|b|, at least 1)"""
    s = float(b.abs().max()) if scale is None else float(scale)
    err = float((a.to(D) - b.to(D)).abs().max()) if a.numel() else 0.0
    assert err <= n * 2.0 ** -52 * max(s, 1.0), '%s: %.3e' % (what, err)


# ---- oracle.ops in the kernels' parametrisation, any dtype -----------------------------------------------------------
def transform(plane, R):
    """census_transform (ops.census_transform minus its grey conversion) of a x255 grey plane"""
    diff = ops._neighbour_stack(plane, R) - plane
    return diff / torch.sqrt(.81 + diff * diff)


def oracle_ham(pa, pb, R):
    return ops.soft_hamming(transform(pa, R), transform(pb, R))


def robust_slope(ham, pm):
    """d/d ham of sum abs_robust_loss(ham) pm by autograd -- except at ham = 0 exactly (equal neighbourhoods, image class C),
    where autograd's sign(0) = 0 and the kernels write the limit 0.4 * 0.01^-0.6 pm: the value never matters, every
    d ham / d input is 0 there too.  The limit is what the reference states."""
    hd = ham.clone().requires_grad_(True)
    g, = torch.autograd.grad((ops.abs_robust_loss(hd) * pm).sum(), [hd])
    return torch.where(ham == 0, pm * 0.4 * (ham.abs() + 0.01) ** -0.6, g)


def capture_coords(src, flow):
    """(warped, ix, iy): ops.resample(src, ops.flow_to_warp(flow)) and the coordinates it hands to its sampler"""
    seen = {}
    orig = ops.sample_bilinear

    def spy(s, ix, iy, pad='zeros'):
        seen['ix'], seen['iy'] = ix, iy
        return orig(s, ix, iy, pad)
    ops.sample_bilinear = spy
    try:
        out = ops.resample(src, ops.flow_to_warp(flow))
    finally:
        ops.sample_bilinear = orig
    return out, seen['ix'], seen['iy']


def oracle_fused(ga, gb, flow, occ, R, w=None, dtype=torch.float32):
    """the composition of test_fused_census_warp_vs_unfused_path_and_oracle on grey planes, in `dtype`, always at the fp32
    sampling coordinate.  -> (ham, mask, dham, sums, loss, d/d flow of sum w ham (w None: of the loss))"""
    fl = flow.float().clone().requires_grad_(True)
    if dtype == torch.float32:
        warped = ops.resample(gb.float(), ops.flow_to_warp(fl))
    else:
        _, ix, iy = capture_coords(gb.float(), flow.float())
        f64 = flow.to(D).clone().requires_grad_(True)
        fl = f64  # value of the fp32 coordinate, unit derivative
        warped = ops.sample_bilinear(gb.to(D), ix.to(D) + (f64[:, 0] - f64[:, 0].detach()),
                                     iy.to(D) + (f64[:, 1] - f64[:, 1].detach()), 'zeros')
    valid = ops.mask_invalid(ops.flow_to_warp(flow.float())).to(dtype)
    mask = valid if occ is None else F.interpolate(occ.to(dtype).clamp(0, 1), scale_factor=4, mode='bilinear',
                                                   align_corners=False) * valid
    ham = oracle_ham(ga.to(dtype), warped, R)
    B, _, H, W = ham.shape
    pm = mask * C.interior(B, H, W, R).to(dtype)
    dham = robust_slope(ham.detach(), pm)
    sums = torch.stack([(ops.abs_robust_loss(ham) * pm).sum(), pm.sum()])
    loss = sums[0] / (sums[1] + 1e-6)
    g, = torch.autograd.grad(loss if w is None else (w.to(dtype) * ham).sum(), [fl])
    return ham.detach(), mask, dham, sums.detach(), loss.detach(), g


def oracle_standalone(im_a, im_b, R, mask, w, dtype=torch.float32):
    a, b = im_a.to(dtype), im_b.to(dtype).clone().requires_grad_(True)
    ham = ops.soft_hamming(ops.census_transform(a, 2 * R + 1), ops.census_transform(b, 2 * R + 1))
    gb, = torch.autograd.grad((w.to(dtype) * ham).sum(), [b])
    B, _, H, W = ham.shape
    pm = mask.to(dtype) * C.interior(B, H, W, R).to(dtype)
    dham = robust_slope(ham.detach(), pm)
    sums = torch.stack([(ops.abs_robust_loss(ham.detach()) * pm).sum(), pm.sum()])
    return ham.detach(), dham, sums, sums[0] / (sums[1] + 1e-6), gb


def fp32_dgb(pa, pb, w, R):
    """d/d grey_b(p) sum_q w(q) ham(q) WRITTEN OUT as the backward kernels restate it, in fp32 on oracle.ops' neighbour
    stack: (w(p) + w(p + o)) h'(e) t'(d_b) with t' = 0.81 rsqrt(0.81 + d^2)^3.  oracle.ops' own fp32 autograd cannot serve
    for the room check of a gradient: its backward forms t' as 1 / s - d^2 / s^3 and the corner difference of the warp as a
    sum of four +- tap x weight products, both of which cancel (measured: 67x the standalone bound on class N images,
    19 000x the flow-gradient bound where a sample straddles the image's edge), while the kernels subtract first."""
    pa, pb, w = pa.float(), pb.float(), w.float()
    da, db = ops._neighbour_stack(pa, R) - pa, ops._neighbour_stack(pb, R) - pb
    ua, ub = torch.rsqrt(.81 + da * da), torch.rsqrt(.81 + db * db)
    e = da * ua - db * ub
    q = 1.0 / (0.1 + e * e)
    return ((w + ops._neighbour_stack(w, R)) * ((0.2 * e * q * q) * (0.81 * ub * ub * ub))).sum(1, keepdim=True)


# ---- 1. pins ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 8, 64), (1, 36, 124), (2, 20, 68), (1, 8, 8)], ids=str)
def test_sampling_coordinate_equals_the_oracles_bit_for_bit(shape):
    for kind in ('Q', 'R'):
        fl = C.flow(kind, *shape)
        _, ix, iy = capture_coords(C.grey('S', *shape), fl)
        rx, ry, cx, cy = C.sample_coords(fl)
        assert ix.dtype == torch.float32 and torch.equal(ix, rx) and torch.equal(iy, ry)
        co = ops.flow_to_warp(fl)
        assert torch.equal(co[:, 0], cx) and torch.equal(co[:, 1], cy)
        assert torch.equal(ops.mask_invalid(co).to(D), C.warp_ref(C.grey('S', *shape), fl).valid)


def cancel(grad):
    """what the frozen GRADIENTS carry on top of the bounds: they are the reference's fp32 autograd, which cancels (see
    fp32_dgb); 1e-4 max|g| is the tolerance tests/test_hip_parity.py has always held the census gradients to"""
    return 1e-4 * float(grad.abs().max())


def test_reference_reproduces_the_golden_census_vectors(golden):
    g = golden('photo')
    for name in g.names():
        im1, im2, mask = g[name + '_im1'], g[name + '_im2'], g[name + '_mask']
        for md, sd in ((1, False), (3, True)):
            tag = '%s_ternary_%d_%d' % (name, md, int(sd))
            div = 1.0 if sd else float((2 * md + 1) ** 2)
            ref = C.standalone_ref(im1, im2, md, w=g[tag + '_g'] / div)
            within(g[tag + '_dist'] * div, ref.ham, ref.ham_bound, tag + ' dist', 1 / ROOM)
            within(g[tag + '_gb'], ref.grad, ROOM * ref.grad_bound + cancel(ref.grad), tag + ' gb')
            ref_a = C.standalone_ref(im2, im1, md, w=g[tag + '_g'] / div)
            within(g[tag + '_ga'], ref_a.grad, ROOM * ref_a.grad_bound + cancel(ref_a.grad), tag + ' ga')
        for ps in (7, 3):
            ref = C.standalone_ref(im1, im2, ps // 2, mask=mask, fold_fp32=True)
            within(g['%s_census_%d' % (name, ps)], ref.loss, ref.loss_bound, name + ' census loss', 1 / ROOM)
            sc = 1.0 / float(ref.sums[1] + 1e-6)
            rg = C.standalone_ref(im1, im2, ps // 2, mask=mask, w=ref.dham, scale=sc)
            extra = rg.g_abs * float((ref.dham_bound / ref.dham.clamp_min(1e-300))[ref.dham > 0].max())
            within(g['%s_census_%d_gb' % (name, ps)], rg.grad, ROOM * (rg.grad_bound + extra) + cancel(rg.grad), name + ' census gb')
    g = golden('general')
    for md, sd in ((4, True), (5, False)):
        tag = 'tern%d_%d' % (md, int(sd))
        div = 1.0 if sd else float((2 * md + 1) ** 2)
        ref = C.standalone_ref(g['im1'], g['im2'], md, w=g[tag + '_g'] / div)
        within(g[tag + '_dist'] * div, ref.ham, ref.ham_bound, tag + ' dist', 1 / ROOM)
        within(g[tag + '_gb'], ref.grad, ROOM * ref.grad_bound + cancel(ref.grad), tag + ' gb')


@pytest.mark.parametrize('R', [1, 2, 3, 4])
def test_reference_agrees_with_the_oracle_in_float64(R):
    B, H, W = 2, 12, 20
    for img in ('S', 'N'):
        im_a, im_b = C.image(img, B, H, W, 0), C.image(img, B, H, W, 1)
        mask, w = C.user_mask(B, H, W), C.weight_plane(B, H, W)
        ref = C.standalone_ref(im_a, im_b, R, mask=mask, w=w)
        ham, dham, sums, loss, gb = oracle_standalone(im_a, im_b, R, mask, w, D)
        ulps64(ref.ham, ham, 64, 'ham')
        ulps64(ref.ham, ops.ternary_loss(im_a.to(D), im_b.to(D), R, True)[0], 64, 'ternary_loss')
        ulps64(ref.dham, dham, 64, 'dham')
        ulps64(ref.sums, sums, 64, 'sums')
        ulps64(ref.loss, loss, 64, 'loss')
        ulps64(ref.loss, ops.census_loss(im_a.to(D), im_b.to(D), mask.to(D), 2 * R + 1), 64, 'census_loss')
        ulps64(ref.grad, gb, 256, 'd im_b')
        if R > 3:
            continue
        for fl in ('Q', 'R'):
            ga, gb_, flow, occ = C.fused_inputs(B, H, W, img, fl)
            for o in (occ, None):
                ref = C.fused_ref(ga, gb_, flow, o, R, w=w)
                ham, m, dham, sums, loss, gf = oracle_fused(ga, gb_, flow, o, R, w, D)
                ulps64(ref.ham, ham, 64, 'fused ham')
                ulps64(ref.mask, m, 8, 'fused mask')
                ulps64(ref.dham, dham, 64, 'fused dham')
                ulps64(ref.loss, loss, 64, 'fused loss')
                ulps64(ref.grad, gf, 256, 'fused d flow', scale=gf.abs().max())
                e2e = C.fused_ref(ga, gb_, flow, o, R, w=None, scale=1.0 / float(ref.sums[1] + 1e-6))
                ulps64(e2e.grad, oracle_fused(ga, gb_, flow, o, R, None, D)[5], 256, 'fused d loss / d flow')


# ---- the inputs of the GPU file ---------------------------------------------------------------------------------------
def fused_small_cases():
    for family in ('column', 'ordered', 'pair-symmetric'):
        for R in (1, 2, 3):
            for shape in C.fused_shapes(family, R):
                for img, fl in C.COMBOS:
                    yield family, R, shape, img, fl


def distinct_fused_inputs():
    seen = set()
    rows = [(f, 3, shape, 'S', 'R') for f, shape in C.ROWS_SHAPES]
    for _, R, shape, img, fl in list(fused_small_cases()) + rows:
        if (R, shape, img, fl) not in seen:
            seen.add((R, shape, img, fl))
            yield R, shape, img, fl


# ---- 2. not too tight -------------------------------------------------------------------------------------------------
def check_room_fused(ga, gb, flow, occ, R, w, tag):
    ref = C.fused_ref(ga, gb, flow, occ, R, w=w)
    ham, mask, dham, sums, loss, gf = oracle_fused(ga, gb, flow, occ, R, w)
    within(ham, ref.ham, ref.ham_bound, tag + ' ham', ROOM)
    within(mask, ref.mask, ref.mask_bound, tag + ' mask', ROOM)
    within(dham, ref.dham, ref.dham_bound, tag + ' dham', ROOM)
    within(sums, ref.sums, ref.sums_bound, tag + ' sums', ROOM)
    within(loss, ref.loss, ref.loss_bound, tag + ' loss', ROOM)
    w32 = C.warp_ref(gb, flow, dtype=torch.float32)
    warped32 = ops.resample(gb.float(), ops.flow_to_warp(flow.float()))
    corner = torch.cat([w32.sx, w32.sy], 1)
    within(corner * fp32_dgb(ga, warped32, w, R), ref.grad, ref.grad_bound, tag + ' d flow', ROOM)
    sc = 1.0 / float(ref.sums[1] + 1e-6)
    e2e = C.fused_ref(ga, gb, flow, occ, R, w=None, scale=sc)
    sc32 = 1.0 / (sums[1] + 1e-6)
    within(sc32 * corner * fp32_dgb(ga, warped32, dham, R), e2e.grad, e2e.grad_bound, tag + ' d loss / d flow', ROOM)


def test_fp32_oracle_sits_inside_the_fused_bounds_with_room():
    for R, (B, H, W), img, fl in distinct_fused_inputs():
        ga, gb, flow, occ = C.fused_inputs(B, H, W, img, fl)
        check_room_fused(ga, gb, flow, occ, R, C.weight_plane(B, H, W), 'R%d %s %s%s' % (R, (B, H, W), img, fl))
        if (img, fl) == ('S', 'R'):
            check_room_fused(ga, gb, flow, None, R, C.weight_plane(B, H, W), 'R%d %s no range map' % (R, (B, H, W)))
    for fam, (B2, H, W) in C.PAIR_SHAPE.items():
        for img, fl in C.PAIR_COMBOS:
            gray2, flow2, occ2 = C.pair_inputs(B2, H, W, img, fl)
            for R in (1, 2, 3):
                for d in (0, 1):
                    check_room_fused(C.pair_split(gray2, d), C.pair_split(gray2, d ^ 1), C.pair_split(flow2, d),
                                     C.pair_split(occ2, d ^ 1), R, C.pair_split(C.weight_plane(B2, H, W), d),
                                     'pair %s R%d %s%s dir %d' % (fam, R, img, fl, d))


@pytest.mark.parametrize('shape,R', [(C.SYM_N2, 1), (C.SYM_N2, 2), (C.SYM_N2, 3), (C.SYM_N4, 3)], ids=str)
def test_fp32_oracle_sits_inside_the_bounds_at_the_multi_chunk_shapes(shape, R):
    B, H, W = shape
    ga, gb, flow, occ = C.fused_inputs(B, H, W, 'S', 'R')
    check_room_fused(ga, gb, flow, occ, R, C.weight_plane(B, H, W), str(shape))


def test_fp32_oracle_sits_inside_the_standalone_bounds_with_room():
    for R, B, H, W in C.STANDALONE:
        for img in ('S', 'N', 'C'):
            im_a, im_b = C.image(img, B, H, W, 0), C.image(img, B, H, W, 1)
            mask, w = C.user_mask(B, H, W), C.weight_plane(B, H, W)
            ref = C.standalone_ref(im_a, im_b, R, mask=mask, w=w)
            ham, dham, sums, loss, gb = oracle_standalone(im_a, im_b, R, mask, w)
            tag = 'R%d %s %s' % (R, (B, H, W), img)
            within(ham, ref.ham, ref.ham_bound, tag + ' ham', ROOM)
            within(dham, ref.dham, ref.dham_bound, tag + ' dham', ROOM)
            within(sums, ref.sums, ref.sums_bound, tag + ' sums', ROOM)
            within(loss, ref.loss, ref.loss_bound, tag + ' loss', ROOM)
            g32 = fp32_dgb(ops.rgb_to_grayscale(im_a) * 255, ops.rgb_to_grayscale(im_b) * 255, w, R)
            within(g32 * 255.0 * torch.tensor(C.GREY_W).view(1, 3, 1, 1), ref.grad, ref.grad_bound, tag + ' d im_b', ROOM)
            if img == 'C':  # equal neighbours: exactly 0 away from the zero padding
                inn = C.interior(B, H, W, R)
                assert float(ref.ham[inn].abs().max() if bool(inn.any()) else 0.0) == 0.0


# ---- 3. not vacuous ---------------------------------------------------------------------------------------------------
def leaves(mut, ref, fields, what):
    """the mutated reference is further than FAR x the bound from the true one on at least one element of one field"""
    best = 0.0
    for f in fields:
        a, b, bound = getattr(mut, f), getattr(ref, f), getattr(ref, f + '_bound')
        best = max(best, C.worst((a - b).abs(), bound))
    assert best > FAR, '%s: mutated reference within %.1f x the bound' % (what, best)
    return best


def test_every_mutation_leaves_the_fused_bounds():
    """Classes S and N with either flow class at every small shape of every family (class C is left out: constant planes
    cannot tell a dropped tap).  'valid_open' needs samples exactly on the image's edge: class Q flows.  'tap_axis' and
    'tap_clamp' need fractional or outside samples: class R flows.  Every mutation holds on class N as well as on S.
    Exempt: none of the shapes (the smallest, 8 x 8, has a 2 x 2 interior for R = 3 and every pixel has a full set of pairs)."""
    for R, (B, H, W), img, fl in distinct_fused_inputs():
        if img == 'C':
            continue
        ga, gb, flow, occ = C.fused_inputs(B, H, W, img, fl)
        w = C.weight_plane(B, H, W)
        ref = C.fused_ref(ga, gb, flow, occ, R, w=w)
        tag = 'R%d %s %s%s ' % (R, (B, H, W), img, fl)
        for m in C.MUTATIONS_CORE:
            leaves(C.fused_ref(ga, gb, flow, occ, R, w=w, mutate=m), ref, ['ham'], tag + m)
            leaves(C.fused_ref(ga, gb, flow, occ, R, w=w, mutate=m), ref, ['grad'], tag + m + ' (gradient)')
        leaves(C.fused_ref(ga, gb, flow, occ, R, w=w, mutate='closed_right'), ref, ['dham'], tag + 'closed_right')
        leaves(C.fused_ref(ga, gb, flow, occ, R, w=w, mutate='closed_right'), ref, ['sums'], tag + 'closed_right (sums)')
        leaves(C.fused_ref(ga, gb, flow, occ, R, w=w, mutate='dham_nopm'), ref, ['dham'], tag + 'dham_nopm')
        if fl == 'Q':
            leaves(C.fused_ref(ga, gb, flow, occ, R, w=w, mutate='valid_open'), ref, ['mask'], tag + 'valid_open')
        else:
            for m in ('tap_axis', 'tap_clamp'):
                leaves(C.fused_ref(ga, gb, flow, occ, R, w=w, mutate=m), ref, ['ham'], tag + m)
                leaves(C.fused_ref(ga, gb, flow, occ, R, w=w, mutate=m), ref, ['grad'], tag + m + ' (gradient)')


def test_pair_mutations_leave_the_bounds():
    for fam, (B2, H, W) in C.PAIR_SHAPE.items():
        gray2, flow2, occ2 = C.pair_inputs(B2, H, W, 'S', 'R')
        w2 = C.weight_plane(B2, H, W)
        ref = C.pair_ref(gray2, flow2, occ2, 3, w2, (0.7, -1.3))
        occ_same = C.pair_ref(gray2, flow2, occ2, 3, w2, (0.7, -1.3), mutate='pair_occ_same')
        swapped = C.pair_ref(gray2, flow2, occ2, 3, w2, (0.7, -1.3), mutate='pair_scale_swap')
        for d in (0, 1):
            leaves(occ_same[d], ref[d], ['mask'], fam + ' pair_occ_same')
            leaves(occ_same[d], ref[d], ['dham'], fam + ' pair_occ_same (dham)')
            leaves(swapped[d], ref[d], ['grad'], fam + ' pair_scale_swap')


def test_every_mutation_leaves_the_standalone_bounds():
    """Exempt: 1 x 1 (every neighbour is padding, d = -grey on both sides: every pair is saturated, t = -1 + O(1e-5), the
    whole distance is of the size of its bound and no mutation of it can show); the interior test at sizes without an
    interior ring (min(H, W) <= 2R); 'lastcol' where the dropped offset (R, R) is padding for every pixel (min(H, W) <= R:
    1 x 9).  7 x 7 with R = 3 has one interior pixel and is not exempt."""
    for R, B, H, W in C.STANDALONE:
        if H * W == 1:
            continue
        for img in ('S', 'N'):
            im_a, im_b = C.image(img, B, H, W, 0), C.image(img, B, H, W, 1)
            mask, w = C.user_mask(B, H, W), C.weight_plane(B, H, W)
            ref = C.standalone_ref(im_a, im_b, R, mask=mask, w=w)
            tag = 'R%d %s %s ' % (R, (B, H, W), img)
            for m in C.MUTATIONS_CORE:
                if m == 'lastcol' and min(H, W) <= R:
                    continue
                mut = C.standalone_ref(im_a, im_b, R, mask=mask, w=w, mutate=m)
                leaves(mut, ref, ['ham'], tag + m)
                leaves(mut, ref, ['grad'], tag + m + ' (gradient)')
            if min(H, W) > 2 * R:
                leaves(C.standalone_ref(im_a, im_b, R, mask=mask, w=w, mutate='closed_right'), ref, ['dham'], tag + 'closed_right')
            leaves(C.standalone_ref(im_a, im_b, R, mask=mask, w=w, mutate='dham_nopm'), ref, ['dham'], tag + 'dham_nopm')


# ---- 4. the strip rule ------------------------------------------------------------------------------------------------
def test_strip_rule_gives_the_intended_chunk_counts():
    for R in (1, 2, 3):
        for shape in C.SYM_SHAPES:
            assert C.sym_chunks(*shape, R) == 1
        assert C.sym_chunks(*C.SYM_N2, R) == 2
        B, H, W = C.SYM_N2
        assert B * -(-W // 56) * -(-H // (32 - R)) == 768 and -(-H // (32 - R)) == 8, 'eight strips of two chunks'
    assert C.sym_chunks(*C.SYM_N4, 3) == 4
    B, H, W = C.SYM_N4
    assert B * -(-H // 61) == 768
    # every size of the suite before this file ran one chunk per strip; the benchmark's config 2 runs three
    for shape in [(2, 96, 160), (1, 100, 236), (3, 40, 132), (2, 48, 64)]:
        assert C.sym_chunks(*shape, 3) == 1
    assert C.sym_chunks(8, 384, 640, 3) == 3
    # the partial rows: per family a tile count that is no multiple of 8 and one that is (R = 3)
    assert [C.family_tiles(f, *shape, 3) for f, shape in C.ROWS_SHAPES] == [1, 8, 1, 8, 4, 8]
