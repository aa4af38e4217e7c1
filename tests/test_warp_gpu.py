"""GPU: the stand-alone bilinear warp -- arflow_warp_fwd, arflow_warp_bwd, their bf16-storage forms (csrc/warp.hip) and the
deterministic source gradient arflow_warp_bwd selects (csrc/det_scatter.hip) -- PER ELEMENT against the float64 restatement
of tests/warp_ref.py, on every launch path: the staged window at either pitch, the three reasons for the direct gathers
(unaligned rows, a window too tall, too broad), empty tiles, windows against the source edge, partial tiles, tile counts that
are no multiple of 8, every chunk size with and without a clamped tail chunk, channel splits 1 / 2 / 4, source extents
different from the flow's in every norm mode, the LDS list and the direct atomics of the source gradient, a strided flow.

Every comparison is |got - ref64| <= bound per element with the bounds DERIVED in the docstring of tests/warp_ref.py
(u = 2^-24) and checked without a GPU in tests/test_warp_ref_cpu.py.  The sampling coordinate is part of the operation's
definition (fp32, restated there), so floor, the border clip and `valid` are exact: no element is left out, and where the
bound is 0 (no tap inside the source, integer coordinates, an active border clip, a source cell nothing lands on) the result
must be exact.  Outputs of the raw entry points are handed over full of NaN and must come back finite; the inputs must come
back untouched.  The forward, and the flow gradient without a channel split, must agree bit for bit over two runs; in
deterministic mode all outputs must over three (every test leaves the mode off: autouse fixture).

The per-pixel statement of the nearest and bicubic warps (csrc/generic.hip) is tests/test_generic_gpu.py, on the restatement
of tests/generic_ref.py; that of warp_up2 and of the level kernels is tests/test_level_gpu.py."""
import pytest
import torch

from tests import warp_ref as R

pytestmark = pytest.mark.gpu
SITES = {}
REFS = {}
NAN = float('nan')
ident = lambda c: c.name.replace(' ', '_')  # noqa: E731


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


def same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


def case_data(case):
    """inputs and float64 reference of a case, computed once per module"""
    key = (case.name, case.bf16)
    if key not in REFS:
        src, flow, gout = R.inputs(case)
        REFS[key] = (src, flow, gout, R.warp_ref(src, flow, R.PAD[case.pad], case.align, R.NORMS[case.norm], gout),
                     R.case_paths(case))
    return REFS[key]


# ---- raw entry points ------------------------------------------------------------------------------------------------
def dev_src(case, src):
    return cu(src).to(torch.bfloat16).contiguous() if case.bf16 else cu(src)


def raw_fwd(AF, case, s, f, fbs, want_valid):
    """arflow_warp_fwd[_bf16] into NaN-filled outputs"""
    out = nan_like((case.B, case.C, case.H, case.W))
    valid = nan_like((case.B, 1, case.H, case.W)) if want_valid else None
    AF._call('arflow_warp_fwd_bf16' if case.bf16 else 'arflow_warp_fwd', AF._p(s), f.data_ptr(), AF._p(out), AF._p(valid),
             case.B, case.C, case.Hs, case.Ws, case.H, case.W, fbs, R.PAD[case.pad], int(case.align), R.NORMS[case.norm],
             AF._stream())
    return out, valid


def raw_bwd(AF, case, g, s, f, fbs, want_src, want_flow):
    """arflow_warp_bwd[_bf16] into NaN-filled gradients (no memset in front: in default mode the launcher zero-fills what
    its atomics add to, in deterministic mode every element is written by its owner)"""
    gsrc = nan_like((case.B, case.C, case.Hs, case.Ws)) if want_src else None
    gflow = nan_like((case.B, 2, case.H, case.W)) if want_flow else None
    AF._call('arflow_warp_bwd_bf16' if case.bf16 else 'arflow_warp_bwd', AF._p(g), AF._p(s), f.data_ptr(), AF._p(gsrc),
             AF._p(gflow), case.B, case.C, case.Hs, case.Ws, case.H, case.W, fbs, R.PAD[case.pad], int(case.align),
             R.NORMS[case.norm], AF._stream())
    return gsrc, gflow


def fwd_site(case, paths):
    return 'warp fwd%s chunk %d' % (' bf16' if case.bf16 else '', paths.chunk)


def check_forward(AF, case, flow_dev=None, fbs=None):
    src, flow, gout, ref, paths = case_data(case)
    s = dev_src(case, src)
    f = cu(flow) if flow_dev is None else flow_dev
    fbs = 2 * case.H * case.W if fbs is None else fbs
    for want_valid in (False, True):
        out, valid = raw_fwd(AF, case, s, f, fbs, want_valid)
        assert_within(out, ref.out, ref.bound_out, fwd_site(case, paths), '%s valid=%s' % (case.name, want_valid))
        again, valid2 = raw_fwd(AF, case, s, f, fbs, want_valid)
        same_bits(out, again, '%s: two forward runs differ' % case.name)
        if want_valid:
            assert torch.equal(valid.cpu().double(), ref.valid), '%s: valid map differs in %d pixels' % (
                case.name, int((valid.cpu().double() != ref.valid).sum()))
            same_bits(valid, valid2, '%s: two valid maps differ' % case.name)
    assert torch.equal(s.float().cpu(), src), 'the forward wrote to its source'
    if flow_dev is None:
        assert torch.equal(f.cpu(), flow), 'the forward wrote to its flow'


def check_backward(AF, case, det, requests=('gsrc', 'gflow', 'both'), runs=1, flow_dev=None, fbs=None):
    src, flow, gout, ref, paths = case_data(case)
    s, g = dev_src(case, src), cu(gout)
    f = cu(flow) if flow_dev is None else flow_dev
    fbs = 2 * case.H * case.W if fbs is None else fbs
    mode = 'det' if det else 'default'
    kind = ' bf16' if case.bf16 else ''
    for req in requests:
        want_src, want_flow = req in ('gsrc', 'both'), req in ('gflow', 'both')
        first = None
        for r in range(runs):
            gsrc, gflow = raw_bwd(AF, case, g, s, f, fbs, want_src, want_flow)
            assert (gsrc is None) == (not want_src) and (gflow is None) == (not want_flow)
            if r == 0:
                tag = '%s %s' % (case.name, req)
                if want_src:
                    labels = '+'.join(sorted(set(paths.src) - {'empty'})) or 'empty'
                    site = 'warp bwd gsrc %s%s %s' % (mode, kind, 'fixed order' if det else labels)
                    assert_within(gsrc, ref.gsrc, ref.bound_gsrc, site, tag)
                if want_flow:
                    split = 1 if det else paths.split_bwd
                    site = 'warp bwd gflow %s%s chunk %d split %d' % (mode, kind, paths.chunk, split)
                    assert_within(gflow, ref.gflow, ref.bound_gflow, site, tag)
                first = (gsrc, gflow)
                continue
            if det and want_src:
                same_bits(first[0], gsrc, '%s %s: deterministic gsrc differs in run %d' % (case.name, req, r))
            if want_flow and (det or paths.split_bwd == 1):
                same_bits(first[1], gflow, '%s %s: gflow differs in run %d' % (case.name, req, r))
    assert torch.equal(s.float().cpu(), src) and torch.equal(g.cpu(), gout), 'the backward wrote to its inputs'
    if flow_dev is None:
        assert torch.equal(f.cpu(), flow), 'the backward wrote to its flow'


# ---- fp32 storage ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CASES, ids=ident)
def test_forward(AF, case):
    check_forward(AF, case)


@pytest.mark.parametrize('case', R.CASES, ids=ident)
def test_backward_default_mode(AF, case):
    check_backward(AF, case, det=False, runs=2)


@pytest.mark.parametrize('case', R.CASES, ids=ident)
def test_backward_deterministic_mode(AF, case):
    with AF.deterministic():
        check_forward(AF, case)
        src, flow, _, _, _ = case_data(case)
        s, f = dev_src(case, src), cu(flow)
        outs = [raw_fwd(AF, case, s, f, 2 * case.H * case.W, False)[0] for _ in range(3)]
        same_bits(outs[0], outs[1], '%s: deterministic forward differs in run 1' % case.name)
        same_bits(outs[0], outs[2], '%s: deterministic forward differs in run 2' % case.name)
        check_backward(AF, case, det=True, requests=('gsrc', 'gflow'))
        check_backward(AF, case, det=True, requests=('both',), runs=3)


# ---- bf16 storage ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.BF16_CASES, ids=ident)
def test_bf16_storage(AF, case):
    assert case.bf16
    check_forward(AF, case)
    check_backward(AF, case, det=False, runs=2)
    with AF.deterministic():
        check_backward(AF, case, det=True, requests=('both',), runs=3)


# ---- a flow consumed out of a wider tensor ---------------------------------------------------------------------------
@pytest.mark.parametrize('half', (0, 1))
def test_strided_flow(AF, half):
    case = R.STRIDED_CASE
    _, flow, _, _, _ = case_data(case)
    wide = torch.full((case.B, 4, case.H, case.W), 777.0)   # the other half would throw every pixel out of the image
    wide[:, 2 * half:2 * half + 2] = flow
    wide_dev = cu(wide)
    view = wide_dev[:, 2 * half:2 * half + 2]
    assert view.data_ptr() == wide_dev.data_ptr() + 4 * 2 * half * case.H * case.W
    fbs = 4 * case.H * case.W
    check_forward(AF, case, view, fbs)
    check_backward(AF, case, det=False, flow_dev=view, fbs=fbs)
    with AF.deterministic():
        check_backward(AF, case, det=True, requests=('both',), runs=3, flow_dev=view, fbs=fbs)
    assert torch.equal(wide_dev.cpu(), wide), 'the kernels wrote to the flow tensor'


# ---- the flow gradient of a short chunk does not depend on what LDS held before -----------------------------------------
@pytest.mark.parametrize('name,bf16', [('C=1', False), ('C=2', False), ('C=1', True)], ids=lambda v: str(v).replace('=', ''))
def test_flow_gradient_ignores_unstaged_window_planes(AF, name, bf16):
    """With C below the chunk size the window planes of the chunk's missing channels are never staged.  A forward over a
    NaN source in front leaves NaN in the LDS those planes occupy (on every CU: 2048 tiles); the flow gradient, whose
    missing channels carry a zero output gradient, must not pick them up."""
    case = R.BY_NAME[name]._replace(bf16=bf16)
    poison = R._c('poison', 32, 3, 64, 256, 'stretch', R.SHIFT, 'narrow')
    nan_src = nan_like((poison.B, poison.C, poison.Hs, poison.Ws))
    raw_fwd(AF, poison, nan_src, cu(R.build_field(poison)), 2 * poison.H * poison.W, False)
    check_backward(AF, case, det=False, requests=('gflow',))


# ---- the autograd nodes pass extents, stride and flags through ---------------------------------------------------------
@pytest.mark.parametrize('storage', (None, 'bf16'))
def test_autograd_nodes(AF, storage):
    base = R.BY_NAME['16x64->12x32 uflow']
    case = base._replace(B=2, C=5, bf16=storage == 'bf16', name=base.name + ' B2 C5')
    src, flow, gout, ref, paths = case_data(case)
    wide = torch.zeros(case.B, 4, case.H, case.W)
    wide[:, 2:4] = flow
    wide_dev = cu(wide)
    s, f = cu(src).requires_grad_(True), wide_dev[:, 2:4].requires_grad_(True)
    kind = ' bf16' if case.bf16 else ''
    if storage is None:
        out, valid = AF.warp_with_valid(s, f, pad=case.pad, align_corners=case.align, norm=R.NORMS[case.norm])
        assert torch.equal(valid.cpu().double(), ref.valid)
        plain = AF.warp(s, f, pad=case.pad, align_corners=case.align, norm=R.NORMS[case.norm])
        same_bits(out.detach(), plain.detach(), 'warp and warp_with_valid differ')
    else:
        out = AF.warp(s, f, pad=case.pad, align_corners=case.align, norm=R.NORMS[case.norm], storage='bf16')
    assert_within(out, ref.out, ref.bound_out, 'autograd warp%s fwd' % kind, case.name)
    gs, gf = torch.autograd.grad(out, [s, f], cu(gout))
    assert_within(gs, ref.gsrc, ref.bound_gsrc, 'autograd warp%s gsrc' % kind, case.name)
    assert_within(gf, ref.gflow, ref.bound_gflow, 'autograd warp%s gflow' % kind, case.name)
