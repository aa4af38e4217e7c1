"""CPU: everything tests/test_generic_gpu.py rests on (tests/generic_ref.py), and the half-pixel x4 upsample restatement
(tests/gauss_pyr_ref.py up_half), checked without a GPU.

1. Definition.  With the coordinate taken in float64 the restatements of the nearest and bicubic warps equal
   F.grid_sample(src.double(), grid64, mode, padding_mode, align_corners) to 1e-10 on the `noise` cases, bicubic with both
   gradients.  Pixels whose float64 coordinate lies within 1e-9 of an integer (bicubic) or of a half-integer (nearest) may be
   left out of THIS comparison (at most 2 %, asserted; on the noise fields there are none, asserted).  With the fp32 coordinate
   they equal the reference's own vectors of tests/golden/general.npz at the tolerances of tests/test_oracle_golden.py.
   corr_general_ref equals oracle.ops.correlation_general in float64 to 1e-12 and its explicit gradient formulas equal that
   expression's autograd to 1e-12; arflow_corr_general_out_size (host code) returns the restated geometry and the ABI codes.
2. The bounds hold for a plain fp32 evaluation of each restatement in the kernel's operation order; the worst err / bound
   per quantity is printed.
3. Every mutation puts at least one element of at least one case outside the bound (by how many bounds is printed);
   half_away and floor_half are caught by the `half` fields alone.
4. The ties are really there: the `half` cases hold >= 30 pixels per axis whose fp32 coordinate is exactly k + 0.5 with even
   k; the `exact` cases hold the special coordinates and the +-1e30 columns.
5. Coverage of the case lists.
6. flow_upsample(., 4, False): a plain fp32 evaluation sits inside both bounds, the align_corners=True weights fall outside.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import gauss_pyr_ref as G
from tests import generic_ref as R
from tests import warp_ref as W
from tests.conftest import assert_close

D, F32 = R.D, R.F32
ident = lambda c: c.name.replace(' ', '_')  # noqa: E731
NOISE_CASES = [c for c in R.WARP_CASES + [R.STRIDED_CASE] if c.field == 'noise']
HALF_CASES = [c for c in R.WARP_CASES if c.field == 'half']
EXACT_CASES = [c for c in R.WARP_CASES if c.field == 'exact']


def ratio(got, iv):
    return R.worst((got.to(D) - iv.v).abs(), iv.e)


def args_of(case):
    src, flow, gout = W.inputs(case)
    return src, flow, R.PAD[case.pad], case.align, R.NORMS[case.norm], gout


# ---- 1. definition -------------------------------------------------------------------------------------------------------
def grid64(flow, Hs, Ws, norm):
    """the normalised grid of the reference's flow_warp (norm ARFLOW: by the flow's extents) / resample (by the source's)"""
    B, _, H, Wf = flow.shape
    xs = torch.arange(Wf, dtype=D).view(1, 1, Wf).expand(B, H, Wf)
    ys = torch.arange(H, dtype=D).view(1, H, 1).expand(B, H, Wf)
    if norm == W.NORM_ARFLOW:
        gx, gy = 2.0 * (xs + flow[:, 0]) / (Wf - 1) - 1.0, 2.0 * (ys + flow[:, 1]) / (H - 1) - 1.0
    else:
        px, py = (flow[:, 0], flow[:, 1]) if norm == W.NORM_UFLOW_ABS else (xs + flow[:, 0], ys + flow[:, 1])
        gx, gy = 2.0 * px / max(Ws - 1, 1) - 1.0, 2.0 * py / max(Hs - 1, 1) - 1.0
    return torch.stack([gx, gy], -1)


@pytest.mark.parametrize('case', NOISE_CASES, ids=ident)
@pytest.mark.parametrize('mode', ('nearest', 'bicubic'))
def test_float64_restatement_is_grid_sample(case, mode):
    src, flow, pad, align, norm, gout = args_of(case)
    ix, iy, _, _ = W.coords(flow, case.Hs, case.Ws, norm, align, dtype=D)
    off = 0.5 if mode == 'nearest' else 0.0
    near = torch.zeros_like(ix, dtype=torch.bool)
    for c, n in ((ix, case.Ws), (iy, case.Hs)):
        if n == 1 and norm != W.NORM_ARFLOW:   # x * (n - 1): the coordinate is the integer 0 itself on either side, not near it
            assert bool((c == 0).all())
            continue
        near |= (c - off - torch.round(c - off)).abs() < 1e-9
    share = float(near.double().mean())
    assert share <= 0.02 and share == 0.0, '%s: %.3f of the pixels within 1e-9 of a discontinuity' % (case.name, share)
    keep = (~near).unsqueeze(1).to(D)
    s, f = src.double().requires_grad_(True), flow.double().requires_grad_(True)
    out = F.grid_sample(s, grid64(f, case.Hs, case.Ws, norm), mode=mode, padding_mode=case.pad,
                        align_corners=align if norm == W.NORM_ARFLOW else True)
    gs, gf = torch.autograd.grad(out, [s, f], gout.double() * keep)
    fn = R.nearest_ref if mode == 'nearest' else R.bicubic_ref
    ref = fn(src, flow, pad, align, norm, gout.double() * keep, coord_dtype=D)
    err = {'out': float(((out.detach() - ref.out.v) * keep).abs().max()), 'gsrc': float((gs - ref.gsrc.v).abs().max())}
    gflow = ref.gflow if mode == 'nearest' else ref.gflow.v
    err['gflow'] = float(((gf - gflow) * keep).abs().max())
    print('%-40s %-8s |restatement - grid_sample| out %.2e gsrc %.2e gflow %.2e' % (case.name, mode, err['out'], err['gsrc'],
                                                                                    err['gflow']))
    assert max(err.values()) <= 1e-10, err


def test_restatements_equal_the_reference_vectors(golden):
    g = golden('general')
    for name in g['wnames']:
        for pad in ('zeros', 'border'):
            for ac in (True, False):
                tag = '%s_%s_%d' % (name, pad, int(ac))
                a = (g[name + '_x'], g[name + '_flow'], R.PAD[pad], ac, W.NORM_ARFLOW, g[name + '_g'])
                n = R.nearest_ref(*a)
                assert_close(n.out.v, g[tag + '_y'], 0, 0, tag)
                assert_close(n.gsrc.v, g[tag + '_gx'], 1e-6, 1e-6, tag + ' gx')
                b = R.bicubic_ref(*a)
                mx = float(g[name + '_x'].abs().max())
                assert_close(b.out.v, g[tag + '_cub_y'], 4e-6 * mx, 1e-5, tag + ' bicubic')
                assert_close(b.gsrc.v, g[tag + '_cub_gx'], 1e-5, 1e-5, tag + ' bicubic gx')
                assert_close(b.gflow.v, g[tag + '_cub_gf'], 1e-5 * (1 + float(g[tag + '_cub_gf'].abs().max())), 1e-4,
                             tag + ' bicubic gflow')


@pytest.mark.parametrize('case', R.CORR_CASES, ids=ident)
def test_correlation_restatement_is_the_oracle_and_its_autograd(case):
    from oracle import ops
    x1, x2, gout, ref = R.corr_case(case)
    a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    out = ops.correlation_general(a, b, *case.cfg)
    assert out.shape == ref.out.v.shape
    g1, g2 = torch.autograd.grad(out, [a, b], gout.double())
    err = (float((out.detach() - ref.out.v).abs().max()), float((g1 - ref.gx1.v).abs().max()),
           float((g2 - ref.gx2.v).abs().max()))
    print('%-40s |restatement - oracle| out %.2e gx1 %.2e gx2 %.2e' % ((case.name,) + err))
    assert max(err) <= 1e-12
    # an element with no non-zero term is exactly 0, with bound 0
    for iv, nt in ((ref.gx1, ref.nt1), (ref.gx2, ref.nt2)):
        assert bool((iv.v[nt == 0] == 0).all()) and bool((iv.e[nt == 0] == 0).all())


def test_correlation_border_in_the_padding_is_exactly_zero():
    """(7, 3, 4, 1, 2): the window of output row oy is the frame rows oy + md - kr .. oy + md + kr = oy + 3 .. oy + 5, the image
    starts at frame row pad = 7: output rows and columns 0 and 1 read x1's zero padding only.  (The window is anchored at
    oy s1 + md, not at kr + md: the far border, rows up to 16 + 5 = 21 over an image that ends at 19, is not all padding.)"""
    case = next(c for c in R.CORR_CASES if c.cfg == (7, 3, 4, 1, 2))
    ref = R.corr_case(case)[3]
    edge = torch.ones_like(ref.out.v, dtype=torch.bool)
    edge[:, :, 2:, 2:] = False
    assert bool((ref.out.v[edge] == 0).all()) and bool((ref.out.e[edge] == 0).all())
    assert bool((ref.out.e[:, 12, 2:, 2:] > 0).all()), 'behind it the undisplaced channel reads the image everywhere'


def out_size(H, Wd, cfg):
    from arflow_amd import _lib
    oc, oh, ow = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    rc = _lib.load().arflow_corr_general_out_size(H, Wd, *cfg, ctypes.addressof(oc), ctypes.addressof(oh), ctypes.addressof(ow))
    return rc, oc.value, oh.value, ow.value


def test_out_size_entry_point_returns_the_restated_geometry():
    for case in R.CORR_CASES:
        kr, dr, Ho, Wo = R.corr_geometry(case.H, case.W, case.cfg)
        assert out_size(case.H, case.W, case.cfg) == (0, (2 * dr + 1) ** 2, Ho, Wo), case.name
    ESHAPE, EPARAM = -1002, -1003   # include/arflow_hip.h
    assert out_size(13, 12, (2, 4, 2, 1, 1))[0] == EPARAM      # an even kernel size
    assert out_size(13, 12, (2, 3, 2, 0, 1))[0] == EPARAM      # a zero stride
    assert out_size(13, 12, (2, 3, 2, 1, 0))[0] == EPARAM
    assert out_size(13, 12, (0, 3, 6, 1, 1))[0] == ESHAPE      # 12 - 2 (1 + 6) < 0: no output
    assert out_size(13, 12, (0, 1, 6, 1, 1))[0] == ESHAPE      # exactly 0 columns
    assert out_size(13, 12, (0, 1, 6, 1, 1))[1:] == (-7, -7, -7), 'nothing is written on an error'


# ---- 2. the bounds hold for a plain fp32 evaluation ------------------------------------------------------------------------
WORST = {}


def note(site, w):
    WORST[site] = max(WORST.get(site, 0.0), w)


@pytest.fixture(scope='module', autouse=True)
def summary():
    yield
    for site in sorted(WORST):
        print('FP32-ON-CPU %-28s worst err/bound %.4f' % (site, WORST[site]))


@pytest.mark.parametrize('case', R.WARP_CASES + [R.STRIDED_CASE], ids=ident)
def test_fp32_warps_lie_inside_every_bound(case):
    src, flow, gout, near, cub = R.warp_case(case)
    a = (src, flow, R.PAD[case.pad], case.align, R.NORMS[case.norm], gout)
    out, gs = R.nearest_f32(*a)
    assert torch.equal(out.double(), near.out.v), 'the nearest forward is a copy'
    w = {'nearest gsrc': ratio(gs, near.gsrc)}
    c = R.bicubic_f32(*a)
    w.update({'bicubic out': ratio(c.out, cub.out), 'bicubic gflow': ratio(c.gflow, cub.gflow),
              'bicubic gsrc': ratio(c.gsrc, cub.gsrc)})
    print('%-40s %s' % (case.name, ' '.join('%s %.4f' % kv for kv in w.items())))
    for k, v in w.items():
        note(k, v)
        assert v <= 1.0, '%s: %s leaves its bound: %.3f' % (case.name, k, v)
    # structure of the bounds: nothing lands / one pixel lands -> exact; integer coordinates -> the source value itself
    assert bool((near.gsrc.e[(near.nq <= 1).unsqueeze(1).expand_as(near.gsrc.e)] == 0).all())
    assert bool((cub.gsrc.v[(cub.nq == 0).unsqueeze(1).expand_as(cub.gsrc.v)] == 0).all())
    ex = cub.exact.reshape(case.B, 1, case.H, case.W).expand_as(cub.out.e)
    assert bool((cub.out.e[ex] == 0).all()) and torch.equal(c.out[ex].double(), cub.out.v[ex])
    for t in (near.gsrc, cub.out, cub.gflow, cub.gsrc):
        assert bool(torch.isfinite(t.v).all()) and bool(torch.isfinite(t.e).all()) and bool((t.e >= 0).all())


@pytest.mark.parametrize('case', R.CORR_CASES, ids=ident)
def test_fp32_correlation_lies_inside_every_bound(case):
    x1, x2, gout, ref = R.corr_case(case)
    out, g1, g2 = R.corr_general_f32(x1, x2, case.cfg, gout)
    w = {'corr out': ratio(out, ref.out), 'corr gx1': ratio(g1, ref.gx1), 'corr gx2': ratio(g2, ref.gx2)}
    print('%-40s %s' % (case.name, ' '.join('%s %.4f' % kv for kv in w.items())))
    for k, v in w.items():
        note(k, v)
        assert v <= 1.0, '%s: %s leaves its bound: %.3f' % (case.name, k, v)


# ---- 3. mutations --------------------------------------------------------------------------------------------------------
def outside(got, iv):
    """by how many bounds the worst element of `got` lies off (inf for a bound of 0, or another shape)"""
    if got.shape != iv.v.shape:
        return float('inf')
    return R.worst((got - iv.v).abs(), iv.e)


def _warp_mutation(fn, key, mutation, cases):
    best = {}
    for case in cases:
        ref = R.warp_case(case)[key]
        mut = fn(*args_of(case), mutate=mutation)
        for q in ('out', 'gsrc') + (('gflow',) if key == 4 else ()):
            best[q] = max(best.get(q, 0.0), outside(getattr(mut, q).v, getattr(ref, q)))
    return best


@pytest.mark.parametrize('mutation', R.NEAREST_MUTATIONS)
def test_every_nearest_mutation_leaves_its_bound(mutation):
    cases = HALF_CASES if mutation in ('half_away', 'floor_half') else R.WARP_CASES
    best = _warp_mutation(R.nearest_ref, 3, mutation, cases)
    print('nearest %-18s out %.3g gsrc %.3g bounds' % (mutation, best['out'], best['gsrc']))
    assert best['out'] > 1.0 and best['gsrc'] > 1.0


@pytest.mark.parametrize('mutation', R.BICUBIC_MUTATIONS)
def test_every_bicubic_mutation_leaves_its_bound(mutation):
    best = _warp_mutation(R.bicubic_ref, 4, mutation, R.WARP_CASES)
    print('bicubic %-22s out %.3g gflow %.3g gsrc %.3g bounds' % (mutation, best['out'], best['gflow'], best['gsrc']))
    must = {'grad_counts_zero_taps': ('gflow',), 'lose_pair': ('gsrc',)}.get(mutation, ('out', 'gflow', 'gsrc'))
    for q in must:
        assert best[q] > 1.0, '%s: %s stays inside' % (mutation, q)


@pytest.mark.parametrize('mutation', R.CORR_MUTATIONS)
def test_every_correlation_mutation_leaves_its_bound(mutation):
    best = {'out': 0.0, 'gx1': 0.0, 'gx2': 0.0}
    for case in R.CORR_CASES[:-1]:
        x1, x2, gout, ref = R.corr_case(case)
        kr, dr, Ho, Wo = R.corr_geometry(case.H, case.W, case.cfg, mutation)
        if (kr, dr, Ho, Wo) != ref.geometry:   # another output shape: seen by the shape alone
            mut = R.corr_general_ref(x1, x2, case.cfg, None, mutation)
            assert mut.out.v.shape != ref.out.v.shape
            best = {k: float('inf') for k in best}
            continue
        mut = R.corr_general_ref(x1, x2, case.cfg, gout, mutation)
        for q in best:
            best[q] = max(best[q], outside(getattr(mut, q).v, getattr(ref, q)))
    print('correlation %-16s out %.3g gx1 %.3g gx2 %.3g bounds' % (mutation, best['out'], best['gx1'], best['gx2']))
    must = ('gx1', 'gx2') if mutation == 'ext_bwd_window' else ('out', 'gx1', 'gx2')
    for q in must:
        assert best[q] > 1.0, '%s: %s stays inside' % (mutation, q)


# ---- 4. the ties and the special coordinates are there ---------------------------------------------------------------------
TIE_EXTRA = [R._w('5x257->6x300 half %s align=%s' % (n, a), 1, 1, 5, 257, 'half', (), Hs=6, Ws=300, norm=n, align=a)
             for n in R.NORMS for a in (True, False)]


@pytest.mark.parametrize('case', HALF_CASES + TIE_EXTRA, ids=ident)
def test_half_fields_hold_ties_on_even_integers(case):
    flow = W.build_field(case)
    ix, iy, _, _ = W.coords(flow, case.Hs, case.Ws, R.NORMS[case.norm], case.align)
    n = []
    for c in (ix, iy):
        c = c.double()
        k = torch.floor(c)
        n.append(int(((c - k == 0.5) & (k % 2 == 0)).sum()))
    print('%-40s ties on an even integer: x %d y %d' % (case.name, *n))
    assert min(n) >= 30


@pytest.mark.parametrize('case', EXACT_CASES, ids=ident)
def test_exact_fields_hold_every_special_coordinate(case):
    info = {}
    flow = W.build_field(case, info)
    ix, iy, _, _ = W.coords(flow, case.Hs, case.Ws, R.NORMS[case.norm], case.align)
    for c, n in ((ix, case.Ws), (iy, case.Hs)):
        inner = (c > 0) & (c < n - 1)
        assert int((inner & (c == c.floor())).sum()) >= 16, 'integer coordinates'
        assert int((inner & (c - c.floor() == 0.5)).sum()) >= 16, 'half coordinates'
        if case in R.EXACT_EXTRA:
            for v in (0.0, n - 1.0, float(n)) + ((-1.0,) if case.W == 65 else ()):
                assert int((c == v).sum()) >= 4, 'coordinate %g' % v
    assert info['exact_share'] == 1.0 or case.W != 65
    assert bool((ix > 1e29).any()) and bool((iy < -1e29).any()) and bool(torch.isfinite(flow).all())
    cub = R.warp_case(case)[4]
    assert int(cub.exact.sum()) >= 32


# ---- 5. coverage -----------------------------------------------------------------------------------------------------------
def test_case_lists_cover_what_they_claim():
    cases = R.WARP_CASES
    assert {(c.pad, c.align, c.norm) for c in cases} == {(p, a, n) for p in R.PAD for a in (True, False) for n in R.NORMS}
    assert {c.field for c in cases} == {'noise', 'stretch', 'half', 'exact', 'far', 'point'}
    for f in ('noise', 'stretch', 'half', 'exact', 'far'):
        assert {(c.pad, c.align) for c in R.BASE_CASES if c.field == f} == {(p, a) for p in R.PAD for a in (True, False)}
    assert any(c.W == 257 for c in cases) and any(c.W == 256 for c in cases)
    assert any(c.Hs == 1 and c.pad == 'border' for c in cases) and any(c.Ws == 1 and c.pad == 'border' for c in cases)
    assert any(c.H == 1 and c.norm == 'uflow' for c in cases) and any(c.W == 1 and c.norm == 'uflow' for c in cases)
    assert not any((c.H == 1 or c.W == 1) and c.norm == 'arflow' for c in cases), 'n_flow - 1 = 0: left out'
    for n in R.NORMS:
        for p in R.PAD:
            assert any(c.norm == n and c.pad == p and (c.Hs, c.Ws) == (11, 10) for c in cases)
            assert any(c.norm == n and c.pad == p and (c.Hs, c.Ws) == (4, 17) for c in cases)
    for c in R.POINT_CASES:
        _, _, _, near, cub = R.warp_case(c)
        assert float(near.nq.max()) == 117 and int((near.nq > 0).sum()) == 1
        assert int((cub.nq == 117).sum()) == 16 and int((cub.nq > 0).sum()) == 16
    # cases where a source-gradient-only call can be compared bit for bit (every cell n_q <= 1), and cases where it cannot
    one = [c.name for c in cases if float(R.warp_case(c)[4].nq.max()) <= 1]
    assert len(one) >= 1 and len(one) < len(cases), one
    cfgs = [c.cfg for c in R.CORR_CASES]
    for cfg in ((4, 1, 4, 1, 1), (0, 1, 2, 1, 1), (7, 3, 4, 1, 2), (3, 3, 2, 2, 2), (2, 5, 3, 3, 2), (5, 3, 4, 2, 1),
                (1, 3, 0, 1, 1)):
        assert any(c.cfg == cfg and (c.B, c.C, c.H, c.W) == (2, 3, 13, 12) for c in R.CORR_CASES), cfg
    assert any(c.C == 1 and c.cfg == R.CORR_DEFAULT for c in R.CORR_CASES)
    assert any((c.B, c.C, c.H, c.W) == (1, 2, 20, 300) for c in R.CORR_CASES)
    assert any(md % s2 for _, _, md, _, s2 in cfgs)
    assert any(R.corr_geometry(c.H, c.W, c.cfg)[2:] != R.corr_geometry(c.H, c.W, c.cfg, 'floor_size')[2:] for c in R.CORR_CASES)
    for c in R.CORR_CASES:   # several workgroups of 256 only where it is asked for: the tests stay small
        kr, dr, Ho, Wo = R.corr_geometry(c.H, c.W, c.cfg)
        assert c.B * (2 * dr + 1) ** 2 * Ho * Wo <= 60000


# ---- 6. flow_upsample(., 4, align_corners=False) ---------------------------------------------------------------------------
def test_upsample_x4_half_pixel_bounds_hold_in_fp32_and_tell_the_align_flag():
    from tests.test_upsample_shared_gpu import PLANES, seeded_host
    told = 0
    for plane in PLANES:
        x, g = seeded_host(plane, 2), seeded_host(plane, 2, 4)
        ref, bound, gref, gbound = G.flow_up_half_ref(x, g, 4)
        want = 4.0 * F.interpolate(x.double(), scale_factor=4, mode='bilinear', align_corners=False)
        assert float((ref - want).abs().max()) <= 1e-12, 'up_half is the half-pixel resize'
        out, _, gin, _ = G.flow_up_half_ref(x, g, 4, dtype=torch.float32)
        w = (R.worst((out.double() - ref).abs(), bound), R.worst((gin.double() - gref).abs(), gbound))
        print('x4 half-pixel %-8s fp32 on the CPU: worst err/bound forward %.4f adjoint %.4f' % (plane, *w))
        assert max(w) <= 1.0
        mo, _, mg, _ = G.flow_up_half_ref(x, g, 4, taps=G._taps)
        m = (R.worst((mo - ref).abs(), bound), R.worst((mg - gref).abs(), gbound))
        print('x4 half-pixel %-8s align_corners=True weights: forward %.3g adjoint %.3g bounds' % (plane, *m))
        if plane != (1, 1):   # one cell: every weight is 1 under either flag
            assert min(m) > 1.0
            told += 1
    assert told >= 3
