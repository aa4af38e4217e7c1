"""CPU: everything tests/test_warp_gpu.py rests on, checked without a GPU.

1. Coordinates: the fp32 restatement of the sampling coordinate (tests/warp_ref.py: coord_axis) against the same formula
   in float64, inside K_C u (|c| + n_src) (derived in that file's docstring) -- the restatement itself is not wrong.
2. The bounds are not too tight: on integer, half-integer and random coordinates, for every padding, align flag and norm
   mode, the fp32 results of oracle.ops (flow_warp / resample) and of torch.nn.functional.grid_sample on the CPU -- output
   and both gradients through autograd -- lie inside each bound of the float64 reference; the larger of the two worst
   err / bound must stay <= 0.5.  The comparators carry their own fp32 roundings, two per tap and accumulation where the
   kernels' fma has one, and for the flow gradient about eight whatever C is (ATen multiplies every tap by its weight
   and the output gradient, then scales twice); the flow-gradient bound (K_G + C) u grows with C, so these recipes use
   C = 8, where half of it leaves room for a comparator that is itself correct.
3. The bounds are not vacuous: every mutation of the reference leaves its bound by more than 100x on a case of the lists.
4. Coverage: every case reaches the branch it names; the union of labels over the lists covers every label, every
   channel split in {1, 2, 4} and both chunk sizes; the exact-coordinate fields contain every special value.
5. Drift: the constants the launch-path restatement uses are read out of csrc/warp.hip and csrc/common.hpp.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import ops
from tests import warp_ref as R

U, D = R.U, R.D
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'arflow_amd', 'csrc')
ident = lambda v: str(v).replace(' ', '_')  # noqa: E731


def ratio(got, ref, bound):
    return R.worst((got.to(D) - ref.to(D)).abs(), bound)


# ---- 1. coordinates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in R.CASES if c.field in ('stretch', 'noise')], ids=lambda c: ident(c.name))
def test_fp32_coordinate_against_float64(case):
    flow = R.build_field(case)
    norm = R.NORMS[case.norm]
    ix, iy, dx, dy = R.coords(flow, case.Hs, case.Ws, norm, case.align)
    jx, jy, ex, ey = R.coords(flow, case.Hs, case.Ws, norm, case.align, dtype=D)
    wx = ratio(ix, jx, R.K_C * U * (jx.abs() + case.Ws))
    wy = ratio(iy, jy, R.K_C * U * (jy.abs() + case.Hs))
    wd = max(ratio(dx, ex, 3 * U * ex.abs()), ratio(dy, ey, 3 * U * ey.abs()))  # two roundings + the conversion
    print('%-44s coordinate worst err/bound x %.4f y %.4f, dc/du %.4f' % (case.name, wx, wy, wd))
    assert wx <= 1.0 and wy <= 1.0 and wd <= 1.0


# ---- 2. the reference against torch ------------------------------------------------------------------------------------
def torch_grid(flow, Hs, Ws, norm, align):
    """the normalised grid the reference hands to grid_sample, in fp32 torch ops"""
    B, _, H, W = flow.shape
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(B, H, W)
    if norm == R.NORM_ARFLOW:
        gx = 2.0 * (xs + flow[:, 0]) / torch.tensor(float(W - 1)) - 1.0
        gy = 2.0 * (ys + flow[:, 1]) / torch.tensor(float(H - 1)) - 1.0
    else:
        px, py = (flow[:, 0], flow[:, 1]) if norm == R.NORM_UFLOW_ABS else (xs + flow[:, 0], ys + flow[:, 1])
        gx = 2.0 * px / torch.tensor(float(max(Ws - 1, 1))) - 1.0
        gy = 2.0 * py / torch.tensor(float(max(Hs - 1, 1))) - 1.0
    return torch.stack([gx, gy], -1)


def comparators(case, src, flow, gout):
    """[(name, out, gsrc, gflow)] in fp32 on the CPU"""
    norm = R.NORMS[case.norm]
    res = []
    align = case.align if norm == R.NORM_ARFLOW else True
    s, f = src.clone().requires_grad_(True), flow.clone().requires_grad_(True)
    out = F.grid_sample(s, torch_grid(f, case.Hs, case.Ws, norm, align), mode='bilinear', padding_mode=case.pad,
                        align_corners=align)
    gs, gf = torch.autograd.grad((out * gout).sum(), [s, f])
    res.append(('grid_sample', out.detach(), gs, gf))
    s, f = src.clone().requires_grad_(True), flow.clone().requires_grad_(True)
    if norm == R.NORM_ARFLOW:
        out = ops.flow_warp(s, f, pad=case.pad, align_corners=case.align)
    elif case.pad == 'zeros':
        out = ops.resample(s, f if norm == R.NORM_UFLOW_ABS else ops.flow_to_warp(f))
    else:
        return res   # the reference's resample has no border padding: grid_sample alone
    gs, gf = torch.autograd.grad((out * gout).sum(), [s, f])
    res.append(('oracle', out.detach(), gs, gf))
    return res


TORCH_CASES = [
    R._c('%s %s align=%s %s %s' % (fld, n, a, p, 'x'.join(map(str, sz))), 2, 8, 16, 64, fld, args, 'narrow', Hs=sz[0], Ws=sz[1],
         norm=n, align=a, pad=p)
    for fld, args in (('exact', ()), ('half', ()), ('noise', (3.0,)))
    for n in ('arflow', 'uflow', 'abs') for a in ((True, False) if n == 'arflow' else (True,)) for p in ('zeros', 'border')
    for sz in ((16, 64), (12, 32))
]


@pytest.mark.parametrize('case', TORCH_CASES, ids=lambda c: ident(c.name))
def test_fp32_torch_lies_inside_half_of_every_bound(case):
    src, flow, gout = R.inputs(case)
    if case.field == 'exact':   # +-1e30: ATen's grid_sample casts the floor of such a coordinate to an integer (undefined)
        flow = flow.clamp(-1e4, 1e4)
    ref = R.warp_ref(src, flow, R.PAD[case.pad], case.align, R.NORMS[case.norm], gout)
    worst = 0.0
    pow2 = all(n & (n - 1) == 0 for n in (case.Hs, case.Ws))
    for name, out, gs, gf in comparators(case, src, flow, gout):
        if name == 'grid_sample' and not case.align and case.norm == 'arflow' and not pow2:
            # ATen's vectorised CPU kernel forms (g + 1) (n / 2) - 1/2 in ONE rounding (a contracted multiply-add) where
            # GridSampler.h, the GPU kernel of the reference and oracle.ops round the product first: another fp32
            # coordinate unless n is a power of two.  The oracle alone is compared there.
            continue
        w = (ratio(out, ref.out, ref.bound_out), ratio(gs, ref.gsrc, ref.bound_gsrc), ratio(gf, ref.gflow, ref.bound_gflow))
        print('%-52s %-11s worst err/bound out %.4f gsrc %.4f gflow %.4f' % (case.name, name, *w))
        worst = max(worst, *w)
    if R.NORMS[case.norm] == R.NORM_ARFLOW or case.pad == 'zeros':
        valid = ops.mask_invalid(flow if case.norm == 'abs' else ops.flow_to_warp(flow))
        assert torch.equal(valid.to(D), ref.valid)
    assert worst <= 0.5, '%s: worst err/bound %.3f' % (case.name, worst)


# ---- 3. mutations ----------------------------------------------------------------------------------------------------------
MUTATION_CASES = {
    'tap_col': 'noise 24x96', 'tap_row': 'noise 24x96', 'drop_se': 'noise 24x96', 'swap_w': 'wide 24x96',
    'align': '16x64->12x32 arflow align=False zeros', 'border_grad': 'edge border 13x40', 'nsrc_nflow': '12x32->16x64 arflow',
    'tail_double': 'C=5', 'lose_pair': 'tile onto a point',
}


@pytest.mark.parametrize('mutation', R.MUTATIONS)
def test_every_mutation_leaves_its_bound_by_100x(mutation):
    case = R.BY_NAME[MUTATION_CASES[mutation]]
    ref, mut = R.case_ref(case), R.case_ref(case, mutation)
    w = {'out': ratio(mut.out, ref.out, ref.bound_out), 'gflow': ratio(mut.gflow, ref.gflow, ref.bound_gflow),
         'gsrc': ratio(mut.gsrc, ref.gsrc, ref.bound_gsrc)}
    print('%-12s on %-40s out %.3g gflow %.3g gsrc %.3g' % (mutation, case.name, w['out'], w['gflow'], w['gsrc']))
    must = {'border_grad': ('gflow',), 'lose_pair': ('gsrc',)}.get(mutation, ('out', 'gflow', 'gsrc'))
    for k in must:
        assert w[k] > 100.0, '%s: %s stays within %.1f bounds on %s' % (mutation, k, w[k], case.name)


# ---- 4. coverage -----------------------------------------------------------------------------------------------------------
ALL_CASES = R.CASES + R.BF16_CASES + [R.STRIDED_CASE]


@pytest.mark.parametrize('case', ALL_CASES, ids=lambda c: ident(c.name) + ('_bf16' if c.bf16 else ''))
def test_case_reaches_the_branch_it_names(case):
    p = R.case_paths(case)
    assert case.fwd in p.fwd, '%s: forward tiles are %s' % (case.name, sorted(set(p.fwd)))
    assert case.src in p.src, '%s: source-gradient tiles are %s' % (case.name, sorted(set(p.src)))
    assert p.split_bwd == case.split
    assert p.chunk == (3 if case.C <= 3 and not case.bf16 else 2)
    assert case.B * case.C * max(case.H * case.W, case.Hs * case.Ws) <= 8 * 72 * 160


def test_lists_cover_every_label_split_and_chunk():
    fwd, src, splits, chunks, tails, paddings, tilecounts = set(), set(), set(), set(), set(), set(), set()
    for case in ALL_CASES:
        p = R.case_paths(case)
        fwd |= set(p.fwd)
        src |= set(p.src)
        splits.add(p.split_bwd)
        chunks.add((p.chunk, case.bf16))
        if case.C % p.chunk:
            tails.add((p.chunk, p.split_bwd > 1))
        paddings.add(p.padding)
        tilecounts.add(p.tiles)
    assert fwd == set(R.FWD_LABELS) and src == set(R.SRC_LABELS)
    assert splits == {1, 2, 4}
    assert chunks == {(3, False), (2, False), (2, True)}
    assert tails >= {(3, False), (2, False), (2, True)}, 'a clamped tail chunk at every chunk size, with and without a split'
    assert 1 in tilecounts and 9 in tilecounts and 0 in paddings and 7 in paddings
    # source size != flow size in both directions under every norm mode, on a staged window
    for n in ('arflow', 'uflow', 'abs'):
        for bigger in (True, False):
            assert any(c.norm == n and (c.Ws > c.W) == bigger and c.Ws != c.W and c.Ws % 4 == 0 for c in R.SIZE_CASES)
    assert {(c.pad, c.align) for c in R.CASES} == {('zeros', True), ('zeros', False), ('border', True), ('border', False)}


@pytest.mark.parametrize('case', R.EXACT_CASES, ids=lambda c: ident(c.name))
def test_exact_fields_hold_every_special_coordinate(case):
    info = {}
    flow = R.build_field(case, info)
    ix, iy, _, _ = R.coords(flow, case.Hs, case.Ws, R.NORMS[case.norm], case.align)
    for c, n in ((ix, case.Ws), (iy, case.Hs)):
        inner = (c > 0) & (c < n - 1)
        assert int((inner & (c == c.floor())).sum()) >= 16, 'integer coordinates'
        assert int((inner & (c - c.floor() == 0.5)).sum()) >= 16, 'half coordinates'
        for v in (0.0, n - 1.0, float(n)) + ((-1.0,) if case.W == 65 else ()):
            assert int((c == v).sum()) >= 4, 'coordinate %g' % v
    assert info['exact_share'] == 1.0 or case.W != 65
    assert bool((ix > 1e29).any()) and bool((iy < -1e29).any()) and bool(torch.isfinite(flow).all())
    ref = R.case_ref(case)
    assert int(ref.taps.exact.sum()) >= 32
    if case.pad == 'border':   # a pixel clipped onto a source pixel on both axes: bound 0
        assert int((ref.bound_out.sum(1) == 0).sum()) >= 32
    for t in (ref.out, ref.gflow, ref.gsrc, ref.bound_out, ref.bound_gflow, ref.bound_gsrc):
        assert bool(torch.isfinite(t).all())


# ---- 5. drift --------------------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _ints(text, pattern):
    m = re.search(pattern, text)
    assert m, 'pattern %r not found' % pattern
    return tuple(int(g) for g in m.groups())


def test_restated_constants_match_the_source():
    warp, common = _src('warp.hip'), _src('common.hpp')
    fwd = warp[warp.index('namespace fwd_win {'):warp.index('}  // namespace fwd_win')]
    assert _ints(fwd, r'constexpr int TX = (\d+), TY = (\d+), NT = (\d+), HMAX = (\d+);') == (R.TX, R.TY, R.TX * R.TY, R.FWD_HMAX)
    assert _ints(fwd, r'constexpr int WQ_NARROW = (\d+), WQ_WIDE = (\d+), WMAX = 4 \* WQ_WIDE;') == (R.WQ_NARROW, R.WQ_WIDE)
    assert re.search(r'wd\.fits = !wd\.empty && \(Ws & 3\) == 0 && wd\.bh <= HMAX && aw <= WMAX;', fwd)
    assert re.search(r'wd\.wq = aw <= 4 \* WQ_NARROW \? WQ_NARROW : WQ_WIDE;', fwd)
    lds = warp[warp.index('namespace lds_scatter {'):warp.index('}  // namespace lds_scatter')]
    assert _ints(lds, r'constexpr int TX = (\d+), TY = (\d+), NT = TX \* TY;') == (R.TX, R.TY)
    assert _ints(lds, r'constexpr int WMAX = (\d+), HMAX = (\d+), NCELL = WMAX \* HMAX, CCH = (\d+);') == (R.SRC_WMAX, R.SRC_HMAX, 4)
    assert re.search(r'const bool priv = bw <= WMAX && bh <= HMAX;', lds)
    split = common[common.index('static inline unsigned af_channel_split'):]
    assert _ints(split, r'while \(\(long\)n \* 2 <= C / (\d+) && tiles \* n \* 2 <= (\d+)\) n \*= 2;') == (R.SPLIT_CHUNK,
                                                                                                      R.SPLIT_WORKGROUPS)
    assert re.search(r'return 8u \* \(unsigned\)\(\(T \+ 7\) / 8\);', common)
    # chunk sizes: 3 for C <= 3 in fp32, else 2; the bf16 entry points have the one instantiation
    assert len(re.findall(r'if \(C <= 3\)', warp)) == 2
    assert re.search(r'warp_fwd_kernel<3>', warp) and re.search(r'warp_fwd_kernel<2>', warp)
    assert re.search(r'warp_fwd_kernel<2, bf16_t>', warp) and re.search(r'warp_bwd_flow_kernel<2, TS>', warp)
    det = _src('det_scatter.hip')
    assert _ints(det, r'constexpr int TX = (\d+), TY = (\d+), NT = TX \* TY;') == (R.TX, R.TY)
