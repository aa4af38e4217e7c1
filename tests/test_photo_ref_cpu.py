"""CPU: the float64 photometric reference (tests/photo_ref.py) that tests/test_photo_gpu.py holds the SSIM / L1 kernels and the
fused warp pass to -- checked here, without a GPU, on every input of the GPU cases:

1. Oracle inside the bound: the fp32 evaluation of oracle.ops (ssim, flow_warp, border_mask; autograd for the gradients) --
   the arithmetic the kernels restate, in another summation order -- lies inside every per-element bound.  The worst ratio
   of every quantity is printed; nothing here comes near 1/2 (DESIGN.md section 33 lists the figures).
2. Mutations caught: every deliberately wrong reference leaves the true one by at least 10x the bound in at least one
   element of one compared quantity, at every case designated for it (photo_ref.sums_mutations / pw_mutations say which
   cases can express which mutation; single-window shapes cannot express the tile mutations).
3. Second witness: ssim_ref agrees with oracle.ops.ssim run in float64 to 1e-12, and the fp32 maps stored in
   tests/golden/photo.npz lie inside its bound.
4. The exclusion cap holds for the reference alone, and the case lists reach the launch geometry they are named for.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import photo_ref as R

MIN_MUT = 10.0


@pytest.fixture(scope='module')
def O():
    from oracle import ops
    return ops


def _ratio(got, ref, keep=None):
    err, bound = (got.double() - ref.v).abs(), ref.e
    if keep is not None:
        err, bound = err[keep], bound[keep]
    return R.worst(err, bound)


def _sum_ratio(got, ref):
    return R.worst((torch.as_tensor(float(got), dtype=R.D) - ref.v).abs(), ref.e)


@functools.lru_cache(maxsize=None)
def _sums_ref(c, wts):
    im, rec, mask, _ = R.sums_inputs(c)
    return R.photo_sums_ref(im, rec, mask, wts)


# ---- 1. oracle inside the bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.SUMS_CASES, ids=str)
def test_oracle_inside_the_bound_standalone(O, c):
    im, rec, mask, up = R.sums_inputs(c)
    m = mask if mask is not None else torch.ones(c.B, 1, c.H, c.W)
    r = rec.clone().requires_grad_(True)
    l1, dist = (im - r).abs() * m, O.ssim(r * m, im * m)
    worst = {}
    for wts in R.WEIGHTS:
        ref = _sums_ref(c, wts)
        g, = torch.autograd.grad(wts[0] * l1.sum() + wts[1] * dist.sum(), [r], retain_graph=True)
        worst['grad %s' % (wts,)] = _ratio(g, ref.grad, ~ref.kink.expand_as(g))
    worst['map'] = _ratio(dist.detach(), ref.dist)
    for k, s in enumerate((l1.detach().double().sum(), dist.detach().double().sum(), m.double().sum())):
        worst['sum %d' % k] = _sum_ratio(s, ref.sums[k])
    a, b = rec.clone().requires_grad_(True), im.clone().requires_grad_(True)
    y = O.ssim(a, b)
    ga, gb = torch.autograd.grad(y, [a, b], up)
    ra, rb = R.photo_sums_ref(im, rec, None, gmap=up), R.photo_sums_ref(rec, im, None, gmap=up)
    worst['plain map'] = _ratio(y.detach(), ra.dist)
    worst['map grad a'] = _ratio(ga, ra.grad, ~ra.kink.expand_as(ga))
    worst['map grad b'] = _ratio(gb, rb.grad, ~rb.kink.expand_as(gb))
    print(c, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('case', R.ANY_CASES, ids=str)
@pytest.mark.parametrize('cls', ['blur', 'noise'])
def test_oracle_inside_the_bound_any_window(O, case, cls):
    md, B, C, H, W = case
    im, rec = R.images(cls, B, C, H, W)
    up = torch.randn(B, C, H - 2 * md, W - 2 * md, generator=R._gen(3, H, W))
    a, b = rec.clone().requires_grad_(True), im.clone().requires_grad_(True)
    y = O.ssim(a, b, md)
    ga, gb = torch.autograd.grad(y, [a, b], up)
    r = R.ssim_ref(rec, im, md)
    g1, k1 = R.ssim_any_grad_ref(rec, im, up, md)
    g2, k2 = R.ssim_any_grad_ref(im, rec, up, md)
    worst = (_ratio(y.detach(), r.dist), _ratio(ga, g1, ~k1.expand_as(ga)), _ratio(gb, g2, ~k2.expand_as(gb)))
    print(case, cls, 'map %.3f grad %.3f %.3f' % worst)
    assert max(worst) <= 1.0
    assert float(k1.double().mean()) <= R.KINK_CAP and float(k2.double().mean()) <= R.KINK_CAP


def _oracle_pw(O, c, i, mask=None):
    """the composed fp32 path of one case: sums [G][3], the mask planes, d / d flow per group"""
    fr = [f.clone().requires_grad_(True) for f in i.flow]
    sums, masks, obj = [], [], 0.
    for g in range(c.G):
        if mask is not None:
            m = mask[g]
        elif c.mode == 'border':
            m = O.border_mask(fr[g].detach())
        else:
            m = i.mask[g]
            if c.mode == 'nearest':
                m = F.interpolate(m, (c.H, c.W), mode='nearest')
        m = 1 - m if (c.invert and mask is None) else m
        rec = O.flow_warp(i.src[g], fr[g], pad=c.pad)
        l1, ss = ((i.tgt[g] - rec).abs() * m).sum(), O.ssim(rec * m, i.tgt[g] * m).sum()
        sums.append((l1.detach(), ss.detach(), m.sum()))
        masks.append(m)
        obj = obj + c.coef[g][0] * l1 + c.coef[g][1] * ss
    return sums, torch.cat(masks, 0), torch.autograd.grad(obj, fr)


@pytest.mark.parametrize('c', R.PW_CASES, ids=lambda c: c.name)
def test_oracle_inside_the_bound_fused(O, c):
    i = R.pw_inputs(c)
    ref = R.pw_case_ref(c)
    sums, masks, gf = _oracle_pw(O, c, i)
    assert torch.equal(masks, ref.mask_out), 'the mask planes are exact'
    ws = max(_sum_ratio(sums[g][k], ref.sums[g][k]) for g in range(c.G) for k in range(3))
    wg = max(R.worst((gf[g].double() - ref.gflow[g])[~ref.kink[g]].abs(), ref.bound_gflow[g][~ref.kink[g]])
             for g in range(c.G))
    share = max(float(k.double().mean()) for k in ref.kink)
    print('%-40s sums %.3f  d/d flow %.3f  kink share %.4f' % (c.name, ws, wg, share))
    assert ws <= 1.0 and wg <= 1.0
    assert share <= R.KINK_CAP
    assert all(bool((b[~k] > 0).any()) for b, k in zip(ref.bound_gflow, ref.kink)), 'a bound that is 0 everywhere is vacuous'


@pytest.mark.parametrize('pad', ['zeros', 'border'])
@pytest.mark.parametrize('shape', R.PROBE_SHAPES, ids=str)
def test_oracle_inside_the_bound_probes(O, shape, pad):
    H, W = shape
    c, i = R.probe_inputs(H, W, pad)
    rec = [R.probe_warp(i, g, pad) for g in range(2)]
    worst, outside, integer = 0.0, 0, 0
    for (y, x) in R.probe_pixels(H, W):
        plane = torch.zeros(1, 1, H, W)
        plane[0, 0, y, x] = 1.0
        sums, _, _ = _oracle_pw(O, c, i, mask=[plane, plane])
        for g in range(2):
            ref = R.probe_ref(rec[g], i.tgt[g], y, x)
            worst = max(worst, max(_sum_ratio(sums[g][k], ref[k]) for k in range(3)))
            outside += int(bool((rec[g].v[0, :, y, x] == 0).all()))
            integer += int(bool((rec[g].e[0, :, y, x] == 0).all()))
    print(shape, pad, 'probes %d  worst %.3f  outside %d  exact %d' % (len(R.probe_pixels(H, W)), worst, outside, integer))
    assert worst <= 1.0
    assert integer > 0 and (pad == 'border' or outside > 0), 'probes must reach taps outside and integer coordinates'


# ---- 2. mutations ---------------------------------------------------------------------------------------------------------
def _sums_distance(a, b):
    """largest error / bound of mutated reference `a` against the true `b` over map, sums and gradient"""
    r = [R.worst((a.dist.v - b.dist.v).abs(), b.dist.e), R.worst((a.grad.v - b.grad.v).abs(), b.grad.e)]
    r += [R.worst((a.sums[k].v - b.sums[k].v).abs(), b.sums[k].e) for k in range(3)]
    return max(r)


@pytest.mark.parametrize('c', R.SUMS_CASES, ids=str)
def test_mutations_are_caught_standalone(c):
    im, rec, mask, _ = R.sums_inputs(c)
    for mu in R.sums_mutations(c):
        d = max(_sums_distance(R.photo_sums_ref(im, rec, mask, w, mutate=mu), _sums_ref(c, w)) for w in R.WEIGHTS)
        print('%s %-12s %.1f' % (c, mu, d))
        assert d >= MIN_MUT, (c, mu, d)


@pytest.mark.parametrize('c', R.PW_CASES, ids=lambda c: c.name)
def test_mutations_are_caught_fused(c):
    ref = R.pw_case_ref(c)
    for mu in R.pw_mutations(c):
        mr = R.pw_case_ref(c, mu)
        d = max([R.worst((mr.sums[g][k].v - ref.sums[g][k].v).abs(), ref.sums[g][k].e) for g in range(c.G) for k in range(3)]
                + [R.worst((mr.gflow[g] - ref.gflow[g])[~ref.kink[g]].abs(), ref.bound_gflow[g][~ref.kink[g]])
                   for g in range(c.G)])
        if not torch.equal(mr.mask_out, ref.mask_out):
            d = float('inf')   # the planes are compared exactly
        print('%-40s %-14s %.1f' % (c.name, mu, d))
        assert d >= MIN_MUT, (c.name, mu, d)


@pytest.mark.parametrize('shape', R.PROBE_SHAPES[1:], ids=str)
def test_tile_mutations_are_caught_by_a_probe(shape):
    """what the three sums of a whole image cannot see: a dropped halo column / row moves one probe's
    SSIM sum by far more than its bound"""
    H, W = shape
    c, i = R.probe_inputs(H, W, 'border')
    rec = R.probe_warp(i, 0, 'border')
    # an anchor in the last column / row of a full tile exists from W = 66 / H = 18 on (17 x 65 has none: exempt)
    # (the shifted anchor is left to the whole-image cases: a one-pixel window looks the same from the next anchor)
    for mu in (['halo_col'] if W - 2 > 63 else []) + (['halo_row'] if H - 2 > 15 else []):
        d = 0.0
        for (y, x) in R.probe_pixels(H, W):
            a, b = R.probe_ref(rec, i.tgt[0], y, x, mu), R.probe_ref(rec, i.tgt[0], y, x)
            d = max(d, R.worst((a[1].v - b[1].v).abs(), b[1].e))
        print(shape, mu, '%.1f' % d)
        assert d >= MIN_MUT, (shape, mu, d)


def test_every_mutation_is_designated_somewhere():
    seen = set()
    for c in R.SUMS_CASES:
        seen.update(R.sums_mutations(c))
    for c in R.PW_CASES:
        seen.update(R.pw_mutations(c))
    assert seen == set(R.MUTATIONS), set(R.MUTATIONS) - seen


# ---- 3. second witness ------------------------------------------------------------------------------------------------------
def test_ssim_ref_agrees_with_the_oracle_in_float64(O):
    for c in R.SUMS_CASES:
        im, rec, _, _ = R.sums_inputs(c)
        err = float((O.ssim(rec.double(), im.double()) - R.ssim_ref(rec, im).dist.v).abs().max())
        assert err <= 1e-12, (c, err)
    for md, B, C, H, W in R.ANY_CASES:
        im, rec = R.images('blur', B, C, H, W)
        err = float((O.ssim(rec.double(), im.double(), md) - R.ssim_ref(rec, im, md).dist.v).abs().max())
        assert err <= 1e-12, (md, H, W, err)


def test_window_statistics_inside_their_bounds():
    """win_ref: the fp32 pooling of the oracle's formula (means, E[x x] - mu mu, E[x y] - mu_x mu_y) inside the bound of
    each statistic"""
    for cls in ('blur', 'low', 'near', 'noise'):
        y, x = R.images(cls, 2, 3, 19, 68)
        w = R.win_ref(x, y)
        mx, my = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
        got = {'mx': mx, 'my': my, 'sx': F.avg_pool2d(x * x, 3, 1) - mx * mx, 'sy': F.avg_pool2d(y * y, 3, 1) - my * my,
               'sxy': F.avg_pool2d(x * y, 3, 1) - mx * my}
        worst = {k: _ratio(v, getattr(w, k)) for k, v in got.items()}
        print(cls, {k: round(v, 3) for k, v in worst.items()})
        assert max(worst.values()) <= 1.0, (cls, worst)
        assert bool((w.sx.e > 0).all()) and float(w.mx.e.max()) <= 10 * R.U, 'mean bound: 9 u mean|x|'


def test_ssim_ref_agrees_with_the_golden_maps(golden):
    """photo.npz holds fp32 maps of the reference's own fp32 evaluation: the file's tolerance is the bound of that arithmetic"""
    g = golden('photo')
    for name in g.names():
        if name + '_ssim' not in g:
            continue
        r = R.ssim_ref(g[name + '_im1'], g[name + '_im2'])
        w = R.worst((g[name + '_ssim'].double() - r.dist.v).abs(), r.dist.e)
        print('%s: golden map at %.3f of the bound' % (name, w))
        assert w <= 1.0, name


# ---- 4. caps and geometry -----------------------------------------------------------------------------------------------------
def test_exclusion_cap_holds_for_the_reference_alone():
    for c in R.SUMS_CASES:
        im, rec, mask, up = R.sums_inputs(c)
        refs = [_sums_ref(c, (0.3, 0.7)), R.photo_sums_ref(im, rec, None, gmap=up), R.photo_sums_ref(rec, im, None, gmap=up)]
        for ref in refs:
            assert float(ref.kink.double().mean()) <= R.KINK_CAP, c


def test_case_lists_reach_their_launch_geometry():
    for cases, kernel, (th, tw) in ((R.PX1_CASES, 'px1', (8, 32)), (R.P4_CASES, 'photo4', (16, 64))):
        assert all(R.kernel_of(c.W) == kernel for c in cases)
        tiles = {R.n_tiles(kernel, c.B, c.H, c.W) for c in cases}
        assert {1, 7, 9, 17} <= tiles, tiles                       # padding workgroups, per = 1, 2, 3
        assert any(t % 8 for t in tiles)
        assert {c.W % tw for c in cases if c.W > tw} >= {1, 2, 3} or kernel == 'photo4'   # (photo4: multiples of 4 only)
        assert {c.H % th for c in cases if c.H > th} >= {1, 2, 3}
        assert {c.C for c in cases} == {1, 2, 3}
        assert {c.mask for c in cases} == {'none', 'binary', 'frac', 'rect'}
        assert {c.cls for c in cases} == {'noise', 'blur', 'near', 'low'}
    for c in R.SUMS_CASES:
        if c.mask == 'rect':   # whole windows are zero
            m = R.mask_of('rect', c.B, c.H, c.W)
            assert bool((F.max_pool2d(m, 5, 1) == 0).any()), c
    pw = R.PW_CASES
    assert {c.C for c in pw} == {1, 2, 3} and {c.G for c in pw} == {1, 2} and {c.B for c in pw} == {1, 3}
    assert {(c.mode, c.invert) for c in pw} >= {(m, v) for m in ('plane', 'nearest', 'border') for v in (False, True)}
    assert {c.fyx for c in pw if c.mode == 'nearest'} == {(1, 1), (2, 4), (4, 2)}
    assert {(c.H, c.W) for c in pw} == {(3, 3), (5, 7), (16, 64), (17, 65), (19, 67), (33, 130)}
    assert {c.addr for c in pw} == {'flow4', 'shared'} and {c.pad for c in pw} == {'zeros', 'border'}
