"""CPU: everything tests/test_corr_gpu.py rests on, checked without a GPU.

1. Pins: the float64 restatements of tests/corr_ref.py reproduce the frozen results of the reference (tests/golden/corr.npz:
   volume and both gradients at d = 1 .. 4; tests/golden/aux.npz: both normalisations) within the bounds -- those fixtures were
   computed in fp32 -- and agree with oracle.ops evaluated in float64 to TOL64 (below).
2. The bounds are not too tight: for every recipe small enough, oracle.ops evaluated in fp32 lies inside each bound.
3. The bounds are not vacuous: every mutation leaves the bound on a named recipe; the ratio is printed.  The Bessel-type
   mutations are shown where 1 / (2n) is far above the bound: the small, centred recipes.
4. Coverage: with the restated launch predicates, every branch the GPU tests are meant to reach is reached by a recipe and
   every boundary pair lies on both sides of its threshold.
5. The LeakyReLU kink zeroes fewer than 0.1 % of the output gradients of every recipe.

TOL64: two float64 evaluations of the same sum of k terms differ by at most ~k 2^-53 times the sum of magnitudes; with
k <= 169 and a few operations around it 1e-12 relative to the companion sum is two orders above that and nine below the
fp32 bounds.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import ops
from tests import corr_ref as R

U, D = R.U, R.D
TOL64 = 1e-12


def ratio(got, ref, bound):
    return R.worst((got.to(D) - ref.to(D)).abs(), bound)


def within(got, ref, bound, what):
    w = ratio(got, ref, bound)
    print('%-60s worst err/bound %.4f' % (what, w))
    assert w <= 1.0, '%s: worst err/bound %.3f' % (what, w)


def close64(got, ref, scale, what):
    err = float((got.to(D) - ref.to(D)).abs().max())
    assert err <= TOL64 * max(float(scale), 1e-30), '%s: %.3e against scale %.3e' % (what, err, float(scale))


def oracle_corr(x1, x2, go, d, slope, dtype):
    a, b = x1.to(dtype).clone().requires_grad_(True), x2.to(dtype).clone().requires_grad_(True)
    pre = ops.correlation(a, b, d)
    out = F.leaky_relu(pre, slope)
    g1, g2 = torch.autograd.grad((out * go.to(dtype)).sum(), [a, b])
    return pre.detach(), out.detach(), g1, g2


def oracle_featnorm(x1, x2, g1, g2, mode, dtype):
    B, n = x1.shape
    a = x1.to(dtype).view(B, n, 1, 1).clone().requires_grad_(True)
    b = x2.to(dtype).view(B, n, 1, 1).clone().requires_grad_(True)
    y1, y2 = ops.normalize_features_joint([a, b]) if mode == 'joint' else ops.normalize_features_uflow([a, b])
    d1, d2 = torch.autograd.grad((y1.view(B, n) * g1.to(dtype)).sum() + (y2.view(B, n) * g2.to(dtype)).sum(), [a, b])
    return y1.detach().view(B, n), y2.detach().view(B, n), d1.view(B, n), d2.view(B, n)


def masked_go(go, fwd):
    return go * (~R.kink_mask(fwd)).to(go.dtype)


# ---- 1. pins ----------------------------------------------------------------------------------------------------------
def test_corr_ref_reproduces_the_golden_volume_and_gradients(golden):
    g = golden('corr')
    seen = set()
    for name in g.names():
        x1, x2, go, d = g[name + '_x1'], g[name + '_x2'], g[name + '_g'], int(g[name + '_d'])
        seen.add(d)
        fwd = R.corr_ref(x1, x2, d)
        within(g[name + '_y'], fwd.pre, fwd.bound_pre, 'golden %s volume' % name)
        gr = R.corr_grads_ref(go, fwd.pre, x1, x2, d)
        within(g[name + '_gx1'], gr.gx1, gr.bound1, 'golden %s gx1' % name)
        within(g[name + '_gx2'], gr.gx2, gr.bound2, 'golden %s gx2' % name)
    assert seen == {1, 2, 3, 4}


def test_featnorm_ref_reproduces_the_golden_normalisations(golden):
    g = golden('aux')
    f1, f2 = g['f1'].flatten(1), g['f2'].flatten(1)
    for mode, key in (('joint', 'nj'), ('avg', 'nu')):
        ref = R.featnorm_ref(f1, f2, mode, partial=16)  # the fixtures are plain fp32
        within(g[key + '_1'].flatten(1), ref.y1, ref.bound1, 'golden %s y1' % mode)
        within(g[key + '_2'].flatten(1), ref.y2, ref.bound2, 'golden %s y2' % mode)


@pytest.mark.parametrize('shape,d', R.CORR_CPU, ids=lambda v: str(v).replace(' ', ''))
def test_corr_ref_equals_the_oracle_in_float64_and_bounds_it_in_fp32(shape, d):
    x1, x2, go = R.corr_inputs(*shape, d)
    if shape == R.BF16:
        x1, x2 = R.bf16_round(x1), R.bf16_round(x2)
    for slope in R.SLOPES:
        fwd = R.corr_ref(x1, x2, d, slope)
        go_m = masked_go(go, fwd)
        gr = R.corr_grads_ref(go_m, fwd.pre, x1, x2, d, slope)
        pre, out, g1, g2 = oracle_corr(x1, x2, go_m, d, R.slope32(slope), D)
        close64(pre, fwd.pre, fwd.S.max(), 'pre')
        close64(out, fwd.out, fwd.S.max(), 'out')
        close64(g1, gr.gx1, gr.A1.max(), 'gx1')
        close64(g2, gr.gx2, gr.A2.max(), 'gx2')
        tag = '%s d=%d slope=%g fp32 oracle ' % (shape, d, slope)
        pre, out, g1, g2 = oracle_corr(x1, x2, go_m, d, slope, torch.float32)
        within(pre, fwd.pre, fwd.bound_pre, tag + 'pre')
        within(out, fwd.out, fwd.bound_out, tag + 'out')
        within(g1, gr.gx1, gr.bound1, tag + 'gx1')
        within(g2, gr.gx2, gr.bound2, tag + 'gx2')


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('recipe', R.FEAT_CPU, ids=lambda v: str(v).replace(' ', ''))
def test_featnorm_ref_equals_the_oracle_in_float64_and_bounds_it_in_fp32(recipe, mode):
    x1, x2, g1, g2 = R.feat_inputs(*recipe)
    # partial=16: fp32 torch has no loop that is double from the first value; the float4 loops' bound is the one it is held to
    fwd, bwd = R.featnorm_ref(x1, x2, mode, partial=16), R.featnorm_grads_ref(g1, g2, x1, x2, mode, partial=16)
    y1, y2, d1, d2 = oracle_featnorm(x1, x2, g1, g2, mode, D)
    # the oracle's own float64 cancels in the same places as the bound says fp32 does: scale by kappa
    k = float(fwd.kappa.max())
    close64(y1, fwd.y1, k * fwd.y1.abs().max(), 'y1')
    close64(y2, fwd.y2, k * fwd.y2.abs().max(), 'y2')
    scale = k * max(float(bwd.d1.abs().max()), float(bwd.d2.abs().max()), float((g1.abs().max() / fwd.sd.min())))
    close64(d1, bwd.d1, scale, 'd1')
    close64(d2, bwd.d2, scale, 'd2')
    tag = '%s %s fp32 oracle ' % (recipe, mode)
    y1, y2, d1, d2 = oracle_featnorm(x1, x2, g1, g2, mode, torch.float32)
    within(y1, fwd.y1, fwd.bound1, tag + 'y1')
    within(y2, fwd.y2, fwd.bound2, tag + 'y2')
    within(d1, bwd.d1, bwd.bound1, tag + 'd1')
    within(d2, bwd.d2, bwd.bound2, tag + 'd2')


def test_the_derived_featnorm_bound_at_offset_25_is_not_tighter_than_the_parity_tolerance():
    """the figure the docstring of tests/corr_ref.py and DESIGN.md quote: at kappa near 480 the worst case of the 16-value fp32
    partials allows more than the atol = 4e-4 of tests/test_hip_parity.py -- and is within 2x of the closed form"""
    x1, x2, _, _ = R.feat_inputs(2, 792, 25.0, 1.0)
    for mode in R.MODES:
        ref = R.featnorm_ref(x1, x2, mode)
        k = float(ref.kappa.max())
        worst = float(torch.maximum(ref.bound1, ref.bound2).max())
        closed = float(ref.y1.abs().max()) * U * 23 * k + 16 * U * 25.0
        print('%s: kappa %.0f, largest forward bound %.3e, closed form %.3e' % (mode, k, worst, closed))
        assert 300 < k < 700 and worst > 4e-4 and 0.5 * closed < worst < 2 * closed


def test_at_kappa_8e5_only_the_scalar_loops_keep_a_bound():
    """offset 1 / spread 1e-3: the float4 loops' 16-value fp32 partials can cancel the whole variance (bound infinite: the GPU
    test then only asks for finite outputs); the scalar loops, double from the first value, are held to the fp32 rounding of
    mu, u |mu| / sd, plus a few u of |y|"""
    for (B, n), finite in (((2, 792), False), ((2, 16388), False), ((2, 20487), True)):
        x1, x2, g1, g2 = R.feat_inputs(B, n, 1.0, 1e-3)
        for mode in R.MODES:
            ref, gr = R.featnorm_ref(x1, x2, mode), R.featnorm_grads_ref(g1, g2, x1, x2, mode)
            assert 5e5 < float(ref.kappa.min()) and ref.partial == (1 if finite else 16)
            worst = float(torch.maximum(ref.bound1, ref.bound2).max())
            print('(%d, %d) %s: kappa %.3g, largest forward bound %.3e' % (B, n, mode, float(ref.kappa.max()), worst))
            assert bool(torch.isfinite(gr.bound1).all()) == finite
            if finite:
                floor = U * float((ref.mu.abs() / ref.sd).max())
                assert floor < worst < floor + 1e-5
            else:
                assert worst == float('inf')


# ---- 3. mutations -----------------------------------------------------------------------------------------------------
CORR_MUT_RECIPES = [((2, 12, 20, 36), 4), ((1, 7, 9, 11), 2), ((2, 3, 9, 14), 6)]


@pytest.mark.parametrize('mutate', R.CORR_MUTATIONS_FWD + R.CORR_MUTATIONS_BWD)
def test_every_correlation_mutation_leaves_the_bound(mutate):
    for shape, d in CORR_MUT_RECIPES:
        x1, x2, go = R.corr_inputs(*shape, d)
        fwd = R.corr_ref(x1, x2, d, 0.1)
        go_m = masked_go(go, fwd)
        if mutate in R.CORR_MUTATIONS_FWD:
            bad = R.corr_ref(x1, x2, d, 0.1, mutate)
            w = ratio(bad.out, fwd.out, fwd.bound_out)
            inside = fwd.bound_out > 0  # a displacement outside the image has bound 0: any value there is infinitely far
            print('   (inside the image alone: %.3g)' % ratio(bad.out[inside], fwd.out[inside], fwd.bound_out[inside]))
        else:
            gr = R.corr_grads_ref(go_m, fwd.pre, x1, x2, d, 0.1)
            bad = R.corr_grads_ref(go_m, fwd.pre, x1, x2, d, 0.1, mutate)
            w = max(ratio(bad.gx1, gr.gx1, gr.bound1), ratio(bad.gx2, gr.gx2, gr.bound2))
        print('corr mutation %-12s on %s d=%d: worst err/bound %.3g' % (mutate, shape, d, w))
        assert w > 100.0, (mutate, shape, d, w)


FEAT_MUT_RECIPES = [(1, 2, 0.0, 1.0), (3, 5, 0.0, 1.0), (2, 792, 0.0, 1.0)]  # small and centred: 1 / (2n) >> bound


@pytest.mark.parametrize('mutate', sorted(set(R.FEAT_MUTATIONS_FWD + R.FEAT_MUTATIONS_BWD)))
def test_every_featnorm_mutation_leaves_the_bound(mutate):
    mode = 'avg' if mutate in ('bessel_avg', 'avg_centre_mu') else 'joint'
    for recipe in FEAT_MUT_RECIPES:
        x1, x2, g1, g2 = R.feat_inputs(*recipe)
        w = {}
        if mutate in R.FEAT_MUTATIONS_FWD:
            ref, bad = R.featnorm_ref(x1, x2, mode), R.featnorm_ref(x1, x2, mode, mutate)
            w['y'] = max(ratio(bad.y1, ref.y1, ref.bound1), ratio(bad.y2, ref.y2, ref.bound2))
            w['sd'] = ratio(bad.stats[:, 3], ref.stats[:, 3], ref.stats_bound[:, 3])
        if mutate in R.FEAT_MUTATIONS_BWD:
            ref, bad = R.featnorm_grads_ref(g1, g2, x1, x2, mode), R.featnorm_grads_ref(g1, g2, x1, x2, mode, mutate)
            w['dx'] = max(ratio(bad.d1, ref.d1, ref.bound1), ratio(bad.d2, ref.d2, ref.bound2))
        print('featnorm mutation %-18s (%s) on %s: worst err/bound %s' % (
            mutate, mode, recipe, ', '.join('%s %.3g' % kv for kv in sorted(w.items()))))
        assert all(v > 100.0 for v in w.values()), (mutate, recipe, w)


def test_the_no_G_mutation_also_shows_on_the_large_recipes():
    """the output gradients carry a mean, so the G term is visible at every size, not only where n is small"""
    x1, x2, g1, g2 = R.feat_inputs(2, 16388, 0.0, 1.0)
    ref, bad = R.featnorm_grads_ref(g1, g2, x1, x2, 'joint'), R.featnorm_grads_ref(g1, g2, x1, x2, 'joint', 'no_G')
    w = ratio(bad.d1, ref.d1, ref.bound1)
    print('featnorm mutation no_G on (2, 16388): worst err/bound %.3g' % w)
    assert w > 100.0


# ---- 4. coverage ------------------------------------------------------------------------------------------------------
def test_fast_forward_recipes_reach_every_branch_and_straddle_every_threshold():
    for shape, want in R.FAST_FWD:
        B, C, H, W = shape
        assert R.corr_path(B, C, H, W, 4) == 'fast' and R.fast_fwd_branch(B, C, H, W) == want, shape
    t = {s: R.fast_tiles(s[0], s[2], s[3]) for s, _ in R.FAST_FWD}
    assert (t[160, 32, 8, 4], t[161, 32, 8, 4]) == (160, 161)          # the four-group boundary, same C
    assert (t[767, 4, 8, 4], t[768, 4, 8, 4]) == (767, 768)            # ring of 4 | ring of 2
    assert t[80, 8, 33, 36] >= 768 and 33 % 8 and 36 % 32               # ragged ring of 2
    assert t[1, 4, 3, 4] == 1 and 4 // 4 == 1                           # a single tile, a single chunk
    assert t[1, 20, 17, 68] == 9 and t[1, 8, 100, 4] == 13              # padding ids: 7 and 3 idle workgroups
    assert {R.fast_grid_pad(v) for v in t.values()} >= {0, 3, 4, 5, 7}
    assert (48 // 4) % 4 == 0 and 48 // 4 // 4 == 3                     # three chunks per group
    assert (12 // 4) % 4 and (20 // 4) % 4                              # channel counts the four groups cannot take


def test_fast_backward_recipes_reach_every_split_ring_mode_and_request():
    nm = {'both': 2, 'gx1': 1, 'gx2': 1}
    seen = set()
    for shape, req, act in R.FAST_BWD:
        B, C, H, W = shape
        assert R.fast_eligible(C, W, 4)
        ns = R.fast_bwd_nsplit(B, C, H, W, nm[req])
        seen.add((ns, (C // 4) % ns != 0, R.fast_bwd_ring(B, H, W, nm[req]), act, req))
    splits = {(s[0], s[1]) for s in seen}
    assert splits >= {(1, False), (2, True), (4, True), (8, False)}    # C/4 = 1; 3 over 2; 5 and 6 over 4; 8 over 8
    assert R.fast_bwd_nsplit(2, 20, 20, 36, 2) == 4 and R.fast_bwd_nsplit(2, 24, 20, 36, 2) == 4  # 2+1+1+1 and 2+2+1+1
    # cut back by tiles * nsplit <= 1024: the channels alone would allow 8
    assert R.fast_bwd_nsplit(40, 32, 8, 36, 2) == 4 < R.fast_bwd_nsplit_uncut(32) == 8
    assert R.fast_tiles(40, 8, 36, 2) * 8 > 1024 >= R.fast_tiles(40, 8, 36, 2) * 4
    rings = {(s[2], s[4]) for s in seen}
    assert rings >= {(2, 'both'), (2, 'gx1'), (2, 'gx2'), (3, 'both'), (3, 'gx1'), (3, 'gx2')}
    assert R.fast_tiles(384, 8, 4, 2) == 768 and R.fast_tiles(768, 8, 4, 1) == 768   # exactly at the ring threshold
    assert {(s[3], s[4]) for s in seen} == {(a, r) for a in ('none', 'sign', 'out') for r in ('both', 'gx1', 'gx2')}


def test_general_recipes_reach_every_strip_and_the_capped_generic_grid():
    strips, threads, ds = set(), set(), set()
    for shape, d, bwd in R.GENERAL:
        B, C, H, W = shape
        path = R.corr_path(B, C, H, W, d)
        assert path == ('generic' if d > 4 else 'general'), (shape, d)
        if path == 'general':
            strips.add((R.general_fwd_strip(B, H, W), d))
            threads.add((R.general_bwd_threads(B, H, W), d))
            ds.add(d)
    assert ds == {1, 2, 3, 4}
    assert {s for s, d in strips if d == 4} == {2, 4, 8} and {t for t, d in threads if d == 4} == {64, 128, 256}
    assert (256, 2) in threads
    assert R.general_fwd_strip(1, 91, 91) == 4 and R.general_fwd_strip(1, 130, 253) == 8
    assert R.general_bwd_threads(1, 93, 90) == 128 and R.general_bwd_threads(1, 258, 255) == 256
    assert R.generic_capped(169 * 316 * 316) and not R.generic_capped(169 * 315 * 315)  # the smallest square that is
    assert not R.generic_capped(2 * 169 * 9 * 14)
    B, C, H, W = R.BF16
    assert R.general_fwd_strip(B, H, W) == 4 and R.general_bwd_threads(B, H, W) == 128


def test_featnorm_recipes_reach_every_path_and_straddle_the_thresholds():
    paths = {(B, n): R.feat_path(B, n) for B, n, _, _ in R.FEAT}
    assert set(paths.values()) == {'small/v4', 'small/scalar', 'large/v4', 'large/scalar', 'capped/v4', 'capped/scalar'}
    assert paths[2, 16384] == 'small/v4' and paths[2, 16388] == 'large/v4'         # the boundary pair, both vectorised
    assert paths[2, 16383] == 'small/scalar' and paths[2, 16385] == 'large/scalar'
    assert paths[512, 20484] == 'capped/v4' and paths[512, 20487] == 'capped/scalar'
    want, allowed = R.feat_rows(512, 20484)
    # second trip of the capped moment pass: 5121 float4 over 4 blocks of 1024: one full block, one single float4, two idle
    assert (want, allowed) == (6, 4) and 4 * 1024 < 20484 // 4 < 4 * 1024 + 1024 + 2
    assert R.feat_rows(2, 20487) == (6, 1024)
    for B, n in R.FEAT_OFFSET_SHAPES:
        for o, s in R.FEAT_OFFSETS:
            assert (B, n, o, s) in R.FEAT
    assert 4 * (2048 + 512) >= 4 * 4 * 512   # ARFLOW_FEATNORM_ACC_DOUBLES(B) holds the capped rows


# ---- 5. the kink ------------------------------------------------------------------------------------------------------
KINK = sorted({(s, 4) for s, _, a in R.FAST_BWD if a != 'none'} | {(s, d) for s, d, b in R.GENERAL if b} | {(R.BF16, 4)})


@pytest.mark.parametrize('shape,d', KINK, ids=lambda v: str(v).replace(' ', ''))
def test_the_kink_zeroes_less_than_a_thousandth_of_the_output_gradients(shape, d):
    x1, x2, _ = R.corr_inputs(*shape, d)
    if shape == R.BF16:
        x1, x2 = R.bf16_round(x1), R.bf16_round(x2)
    fwd = R.corr_ref(x1, x2, d, 0.1)
    share = float(R.kink_mask(fwd).double().mean())
    print('%s d=%d: %.5f %% of go zeroed' % (shape, d, 100 * share))
    assert share < 1e-3
