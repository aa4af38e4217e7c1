"""GPU: deterministic mode.  With the mode on, every op whose default kernels end in float atomics --
the warp's source gradient and channel-split flow gradient, the forward splat, the fused level's backward, the bias
gradient -- must be BITWISE reproducible: `torch.equal` over three calls on the same inputs in the same process.  Each is
also held against the CPU oracle at the bound its default form is held to, so "reproducible" cannot mean "reproducibly wrong".

Bounds.  atol 1e-5 / rtol 1e-4 is the project's bound for the warp gradients and the splat.  Where every
target pixel lands on ONE cell the sum has n = H W terms and the bound is the sequential-summation bound of fp32,
n 2^-24 A + 1e-4 |ref| with A = sum w |g| (the oracle's backward of |gout|: the weights are non-negative) -- derived, not
measured.  The oracle's sampling coordinates are computed in fp32 exactly as the reference computes them (oracle/ops.py:
flow_warp keeps the normalise / un-normalise round trip in the working precision); the taps are then blended and the
gradients accumulated in float64.

Every test leaves the mode off (context managers, checked by an autouse fixture): the rest of the suite assumes default dispatch."""
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    return functional


@pytest.fixture(scope='module')
def O():
    from oracle import ops
    torch.set_num_threads(16)
    return ops


@pytest.fixture(autouse=True)
def mode_off_afterwards():
    from arflow_amd import functional
    assert functional.is_deterministic() is False, 'a test before this one left deterministic mode on'
    yield
    left_on = functional.is_deterministic()
    functional.set_deterministic(False)
    assert not left_on, 'this test left deterministic mode on'


def cu(t):
    return t.detach().cuda()


def assert_bitwise(runs, what):
    """runs: one tuple of tensors per call."""
    for k, other in enumerate(runs[1:], 1):
        for i, (a, b) in enumerate(zip(runs[0], other)):
            assert a.shape == b.shape
            same = torch.equal(a, b)
            assert same, '%s: output %d of call %d differs from call 0 in %d elements (max |diff| %.3e)' % (
                what, i, k, int((a != b).sum()), float((a.double() - b.double()).abs().max()))


def assert_within(actual, ref, tol, what):
    """elementwise |actual - ref| <= tol (tol a tensor); prints the worst ratio before it asserts"""
    err, tol = (actual.detach().cpu().double() - ref.double()).abs(), tol.double()
    ratio = float((err / tol.clamp_min(1e-300)).max())
    print('%s: max err %.3e, worst err/tol %.3f' % (what, float(err.max()), ratio))
    assert bool((err <= tol).all()), '%s: %d elements out of tolerance, worst err/tol %.3f' % (what, int((~(err <= tol)).sum()),
                                                                                             ratio)


# ---- 1. warp -------------------------------------------------------------------------------------------------------------
B1, C1, H1, W1 = 2, 5, 19, 45


def oracle_warp64(O, src, flow, pad, align):
    """O.flow_warp with the coordinates in fp32 (its own arithmetic, line for line) and the blend in float64."""
    B, _, H, W = flow.shape
    xs, ys = O._pixel_grid(B, H, W, flow)
    gx = 2.0 * (xs + flow[:, 0]) / (W - 1) - 1.0
    gy = 2.0 * (ys + flow[:, 1]) / (H - 1) - 1.0
    ix = O._unnormalize(gx, src.shape[3], align)
    iy = O._unnormalize(gy, src.shape[2], align)
    return O.sample_bilinear(src.double(), ix.double(), iy.double(), pad)


def warp_fields(gen, pad):
    """name -> (flow [B,2,H,W], every target pixel lands on one source cell)"""
    ys, xs = torch.meshgrid(torch.arange(H1, dtype=torch.float32), torch.arange(W1, dtype=torch.float32), indexing='ij')
    smooth = F.interpolate(torch.randn(B1, 2, 3, 5, generator=gen), (H1, W1), mode='bilinear', align_corners=True)
    fields = {
        'a-smooth': (smooth, False),
        'b-rough': (6.0 * torch.randn(B1, 2, H1, W1, generator=gen), False),
        # every pixel samples (7.25, 3.5): u = 7.25 - x and v = 3.5 - y are exact
        'c-collapse': (torch.stack([7.25 - xs, 3.5 - ys])[None].repeat(B1, 1, 1, 1), True),
        # everything out of bounds; `border` clips every pixel onto the last row and column's corner: a collapse too
        'd-outside': (torch.full((B1, 2, H1, W1), 1000.0), pad == 'border'),
    }
    if pad == 'border':
        half = smooth.clone()
        half[:, 0, :, :W1 // 2] = -100.0  # the left half of the field is clipped onto column 0
        fields['e-half-clipped'] = (half, False)
    return fields


def warp_reference(O, src, flow, gout, pad, align):
    s, f = src.clone().requires_grad_(True), flow.clone().requires_grad_(True)
    y = oracle_warp64(O, s, f, pad, align)
    gs, gf = torch.autograd.grad(y, [s, f], gout.double())
    s2 = src.clone().requires_grad_(True)
    ga, = torch.autograd.grad(oracle_warp64(O, s2, flow, pad, align), [s2], gout.double().abs())  # A = sum w |g|
    return gs, gf, ga


def run_warp(AF, src, flow, gout, pad, align, **kw):
    runs = []
    for _ in range(3):
        s, f = cu(src).requires_grad_(True), cu(flow).requires_grad_(True)
        y = AF.warp(s, f, pad=pad, align_corners=align, **kw)
        runs.append(tuple(t.clone() for t in torch.autograd.grad(y, [s, f], cu(gout))))
    return runs


def check_warp_grads(gs, gf, ref, collapse, n_terms, tag):
    rs, rf, ra = ref
    if collapse:
        tol = n_terms * 2.0 ** -24 * ra + 1e-4 * rs.abs()
    else:
        tol = 1e-5 + 1e-4 * rs.abs()
    assert_within(gs, rs, tol, tag + ' gsrc')
    assert_within(gf, rf, 1e-5 + 1e-4 * rf.abs(), tag + ' gflow')


@pytest.mark.parametrize('src_size', [(H1, W1), (11, 23)], ids=lambda s: 'src%dx%d' % s)
@pytest.mark.parametrize('pad,align', [('zeros', True), ('border', True), ('zeros', False)], ids=lambda v: str(v))
def test_warp_gradients_bitwise_and_vs_oracle(AF, O, pad, align, src_size):
    gen = torch.Generator().manual_seed(101 + 7 * align + (3 if pad == 'border' else 0) + src_size[0])
    src = torch.randn(B1, C1, *src_size, generator=gen)
    gout = torch.randn(B1, C1, H1, W1, generator=gen)
    for name, (flow, collapse) in warp_fields(gen, pad).items():
        tag = '%s %s align=%s src %dx%d' % (name, pad, align, src_size[0], src_size[1])
        with AF.deterministic():
            runs = run_warp(AF, src, flow, gout, pad, align)
        assert_bitwise(runs, tag)
        gs, gf = runs[0]
        if name == 'd-outside' and pad == 'zeros':
            assert float(gs.abs().max()) == 0.0 and float(gf.abs().max()) == 0.0, tag + ': no tap inside the source'
        check_warp_grads(gs, gf, warp_reference(O, src, flow, gout, pad, align), collapse, H1 * W1, tag)


def test_warp_up2_and_bf16_storage_rough_field(AF, O):
    """field (b) through the two other nodes that end in arflow_warp_bwd[_bf16]"""
    gen = torch.Generator().manual_seed(202)
    B, C, H, W = 2, 5, 20, 46  # warp_up2 needs even sizes: a 10 x 23 coarse flow
    src = torch.randn(B, C, H, W, generator=gen)
    gout = torch.randn(B, C, H, W, generator=gen)
    gup = torch.randn(B, 2, H, W, generator=gen)
    fc = 3.0 * torch.randn(B, 2, H // 2, W // 2, generator=gen)
    with AF.deterministic():
        runs = []
        for _ in range(3):
            s, f = cu(src).requires_grad_(True), cu(fc).requires_grad_(True)
            y, up = AF.warp_up2(s, f, pad='zeros', align_corners=True, up_align=True)
            runs.append((y.detach().clone(), up.detach().clone()) + tuple(
                t.clone() for t in torch.autograd.grad([y, up], [s, f], [cu(gout), cu(gup)])))
    assert_bitwise(runs, 'warp_up2')
    s, f = src.clone().requires_grad_(True), fc.clone().requires_grad_(True)
    up = F.interpolate(f * 2, scale_factor=2, mode='bilinear', align_corners=True)
    rs, rf = torch.autograd.grad([oracle_warp64(O, s, up, 'zeros', True), up], [s, f], [gout.double(), gup])
    assert_within(runs[0][2], rs, 1e-5 + 1e-4 * rs.abs(), 'warp_up2 gsrc')
    assert_within(runs[0][3], rf, 1e-5 + 1e-4 * rf.abs(), 'warp_up2 gflow (coarse)')

    flow = 6.0 * torch.randn(B1, 2, H1, W1, generator=gen)
    src = torch.randn(B1, C1, H1, W1, generator=gen)
    gout = torch.randn(B1, C1, H1, W1, generator=gen)
    with AF.deterministic():
        runs = run_warp(AF, src, flow, gout, 'zeros', True, storage='bf16')
    assert_bitwise(runs, 'bf16 storage')
    stored = src.to(torch.bfloat16).float()  # what the kernels sample
    check_warp_grads(runs[0][0], runs[0][1], warp_reference(O, stored, flow, gout, 'zeros', True), False, 0, 'bf16 storage')


# ---- 2. splat ------------------------------------------------------------------------------------------------------------
def splat_cases():
    gen = torch.Generator().manual_seed(303)
    H, W = 40, 64
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    # every pixel lands on (7.25, 3.5): 2560 contributions per cell group, more than a 2^-22 fixed-point 32-bit sum holds
    yield 'collapse 40x64', torch.stack([7.25 - xs, 3.5 - ys])[None].repeat(2, 1, 1, 1)
    yield 'rough 19x45', 6.0 * torch.randn(2, 2, 19, 45, generator=gen)


@pytest.mark.parametrize('variant', [0, 1])
def test_splat_bitwise_and_vs_oracle(AF, O, variant):
    for name, flow in splat_cases():
        B, _, H, W = flow.shape
        xs, ys = O._pixel_grid(B, H, W, flow)
        coords = torch.stack([xs, ys], 1) + flow  # fp32, the kernels' own x + u
        ref = O.compute_range_map(flow) if variant == 0 else O.get_corresponding_map(coords)
        for absolute in (False, True):
            tag = '%s variant %d %s' % (name, variant, 'absolute' if absolute else 'relative')
            with AF.deterministic():
                runs = [(AF.splat_map(cu(coords if absolute else flow), variant | (2 if absolute else 0)).clone(),)
                        for _ in range(3)]
            assert_bitwise(runs, tag)
            got = runs[0][0].cpu()
            assert_close(got, ref, 1e-5, 1e-4, tag)
            assert float(got[ref == 0].abs().max()) == 0.0, tag + ': a cell nothing lands on must be exactly 0'
        if variant == 0:  # the fused splat + smoothness call of UFlowLoss
            gen = torch.Generator().manual_seed(H)
            img = torch.rand(B, 3, H, W, generator=gen)
            with AF.deterministic():
                runs = []
                for pre in (False, True, False):  # with and without a caller-cleared plane
                    s, rm = AF.splat_smooth(cu(flow), cu(img), torch.zeros(B, 1, H, W, device='cuda') if pre else None, 1.0,
                                            150.0, 1, 1, 1)
                    runs.append((s.clone(), rm.clone()))
                plain = AF.smooth_sums(cu(flow), cu(img), 1.0, 150.0, 1, 1, 1)
            assert_bitwise(runs, name + ' splat_smooth')
            assert_close(runs[0][1], ref, 1e-5, 1e-4, name + ' splat_smooth range map')
            assert torch.equal(runs[0][0], plain), 'the smoothness sums are those of arflow_smooth_fwd'


# ---- 3. level ------------------------------------------------------------------------------------------------------------
def level_shapes():
    from tests.test_level_gpu import PAD_ALIGN_SHAPES, SPLIT, level_branch
    # 96 x 160 at B = 2 instead of 16: still the tiled forward and the both-roles backward
    assert level_branch(2, 32, 96, 160, env={}) == ('tiled', 'both')
    picked = [s for s in PAD_ALIGN_SHAPES if s[:4] in ((2, 32, 12, 16), (3, 8, 6, 44))] + [(2, 32, 96, 160, 'tiled', 'both'),
                                                                                          SPLIT + ('tiled4', 'split')]
    assert [s[4:] for s in picked] == [('small', 'both'), ('tiled', 'both'), ('tiled', 'both'), ('tiled4', 'split')]
    return picked


@pytest.mark.parametrize('shape', level_shapes(), ids=lambda s: 'x'.join(map(str, s[:4])) + '-' + s[5])
def test_level_bitwise_and_vs_oracle(AF, O, shape):
    from tests.test_level_gpu import check_branch, run_level_case, smooth_inputs
    check_branch(shape, shape[4], shape[5])  # the kernels the DEFAULT mode takes here: the forms the mode replaces
    gen, x1, x2, flow_c, member = smooth_inputs(shape, sum(shape[:4]))
    B, C, H, W = shape[:4]
    gbuf = torch.randn(B, 81 + C + 2 + 5, H, W, generator=gen).cuda()
    gflow = torch.randn(B, 2, H, W, generator=gen).cuda()
    cfg = AF.LevelCfg(['vol', 'x1n', 'flow', 0], 'joint', 0.1, 4, True, True, 'zeros', True)
    with AF.deterministic():
        runs = []
        for _ in range(3):
            a, b, m, fc = [cu(t).requires_grad_(True) for t in (x1, x2, member, flow_c)]
            buf, flow = AF.level(a, b, fc, cfg, m)
            grads = torch.autograd.grad((buf * gbuf).sum() + (flow * gflow).sum(), [a, b, m, fc])
            runs.append((buf.detach().clone(), flow.detach().clone()) + tuple(g.clone() for g in grads))
        assert_bitwise(runs, 'level %s' % (shape[:4],))
        # ... and equal to the oracle within that file's own bounds (2e-5 scale + 1e-6, rtol 1e-4), still in the mode
        run_level_case(AF, O, x1, x2, flow_c, member, 'zeros', True, True, 'deterministic %s' % (shape[:4],))


# ---- 4. bias gradient ----------------------------------------------------------------------------------------------------
def test_bias_gradient_bitwise_and_vs_torch(AF):
    gen = torch.Generator().manual_seed(404)
    shape = (2, 3, 33, 67)  # HW = 2211: not a multiple of 4, several workgroups per plane in the elementwise pass
    x, bias, go = torch.randn(*shape, generator=gen), torch.randn(3, generator=gen), torch.randn(*shape, generator=gen)
    # the torch composition in fp32 (its elementwise gradient is the kernel's, term for term), its bias sum taken exactly
    a, bb = x.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    ra, = torch.autograd.grad(F.leaky_relu(a + bb.view(1, -1, 1, 1), 0.1), [a], go)
    rb = ra.double().sum((0, 2, 3))
    with AF.deterministic():
        runs = []
        for _ in range(3):
            xc, bc = cu(x).requires_grad_(True), cu(bias).requires_grad_(True)
            y = AF.bias_leaky_relu(xc * 1.0, bc, 0.1)
            runs.append(tuple(t.clone() for t in torch.autograd.grad(y, [xc, bc], cu(go))))
    assert_bitwise(runs, 'bias_leaky_relu backward')
    assert_close(runs[0][0], ra, 1e-7, 1e-7, 'gx')
    assert_close(runs[0][1], rb, 0, 1e-5, 'gbias')


# ---- 5. flow upsample ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('align', [True, False], ids=['align1', 'align0'])
@pytest.mark.parametrize('factor', [2, 4])
def test_flow_upsample_forward_adjoint_bitwise(AF, factor, align):
    for h, w in ((5, 7), (12, 20)):
        gen = torch.Generator().manual_seed(h * factor + align)
        flow = 3.0 * torch.randn(2, 2, h, w, generator=gen)
        gout = torch.randn(2, 2, h * factor, w * factor, generator=gen)
        fr = flow.clone().requires_grad_(True)
        ref = F.interpolate(fr * factor, scale_factor=factor, mode='bilinear', align_corners=align)
        rg, = torch.autograd.grad(ref, [fr], gout)
        runs = []
        for _ in range(3):
            f = cu(flow).requires_grad_(True)
            y = AF.flow_upsample(f, factor, align)
            g, = torch.autograd.grad(y, [f], cu(gout))
            runs.append((y.detach().clone(), g.clone()))
        tag = 'flow_upsample x%d align=%s %dx%d' % (factor, align, h, w)
        assert_bitwise(runs, tag)
        assert_close(runs[0][0], ref, 2e-6 * float(ref.detach().abs().max()), 0, tag + ' forward')
        assert_close(runs[0][1], rg, 1e-5, 1e-4, tag + ' adjoint')
        # the models' call: ATen in default mode (unchanged), this op in the mode
        assert torch.equal(AF.interpolate_flow(cu(flow), factor, align),
                           F.interpolate(cu(flow) * factor, scale_factor=factor, mode='bilinear', align_corners=align))
        with AF.deterministic():
            assert torch.equal(AF.interpolate_flow(cu(flow), factor, align), runs[0][0])


# ---- 6. losses end to end ------------------------------------------------------------------------------------------------
def loss_cases():
    from arflow_amd.config import AttrDict
    from arflow_amd import losses as L
    uflow = AttrDict(edge_constant=150, w_smooth=4.0, w_census=1.0, with_bk=True, smooth_order=1)
    unflow = AttrDict(w_l1=0.15, w_ssim=0.85, w_ternary=0.0, warp_pad='border', with_bk=True, smooth_2nd=True,
                      occ_from_back=True, alpha=10, w_smooth=75.0, w_scales=[1.0, 1.0, 1.0], w_sm_scales=[1.0, 0.0, 0.0])
    full = AttrDict(w_l1=0.0, w_ssim=0.0, w_ternary=1.0, ternary_distance=3, warp_pad='border', align_corners=False,
                    occ_type='wang1', with_bk=True, alpha=10, w_smooth=4.0)
    # (name, module, scales of the flow pyramid)
    return [('UFlowLoss pair path', lambda: L.UFlowLoss(uflow), (1, 2, 4)),
            ('unFlowLoss occ_from_back', lambda: L.unFlowLoss(unflow), (1, 4, 8)),
            ('FullResLoss wang1', lambda: L.FullResLoss(full), (1, 2, 4))]


@pytest.mark.parametrize('case', loss_cases(), ids=lambda c: c[0].split()[0])
def test_losses_bitwise_and_equal_to_default_mode(AF, case):
    from oracle.fixture_common import synth_pair
    name, make, scales = case
    gen = torch.Generator().manual_seed(606)
    B, H, W = 2, 32, 64  # multiples of 4 (census_warp_supported) with a [B,4,H/4,W/4] level: UFlowLoss takes _both_directions
    assert AF.census_warp_supported(H, W)
    img = synth_pair(B, H, W, gen)[0].cuda()
    flows = [(3.0 / s) * torch.randn(B, 4, H // s, W // s, generator=gen).cuda() for s in scales]

    def once():
        f = [t.clone().requires_grad_(True) for t in flows]
        out = make()(f, img)
        grads = torch.autograd.grad(out[0], f, allow_unused=True)
        return tuple(o.detach().clone() for o in out) + tuple(g.clone() for g in grads if g is not None)

    default = once()
    with AF.deterministic():
        runs = [once() for _ in range(3)]
    assert_bitwise(runs, name)
    assert_close(runs[0][0], default[0], 0, 1e-5, name + ': loss in the mode vs default mode')


# ---- 7. mode hygiene -----------------------------------------------------------------------------------------------------
def test_mode_is_sampled_in_forward_and_default_mode_is_untouched(AF, O):
    gen = torch.Generator().manual_seed(707)
    src = torch.randn(B1, C1, H1, W1, generator=gen)
    gout = torch.randn(B1, C1, H1, W1, generator=gen)
    flow = 6.0 * torch.randn(B1, 2, H1, W1, generator=gen)  # field (b)
    with AF.deterministic():
        inside = run_warp(AF, src, flow, gout, 'zeros', True)[0]
        s, f = cu(src).requires_grad_(True), cu(flow).requires_grad_(True)
        y = AF.warp(s, f, pad='zeros', align_corners=True)  # forward in the mode ...
    assert AF.is_deterministic() is False
    late = torch.autograd.grad(y, [s, f], cu(gout))  # ... backward after it was switched off: the node kept its value
    assert AF.is_deterministic() is False
    assert_bitwise([inside, late], 'backward outside the context of its forward')
    # the other way round: a default-mode forward keeps the default backward when the mode is switched on in between
    s, f = cu(src).requires_grad_(True), cu(flow).requires_grad_(True)
    y = AF.warp(s, f, pad='zeros', align_corners=True)
    with AF.deterministic():
        gs, gf = torch.autograd.grad(y, [s, f], cu(gout))
        assert AF.is_deterministic() is True
    # default mode on the same inputs still matches the oracle
    check_warp_grads(gs, gf, warp_reference(O, src, flow, gout, 'zeros', True), False, 0, 'default mode')


def test_atomic_only_ops_raise_in_the_mode(AF):
    from arflow_amd import _lib
    gen = torch.Generator().manual_seed(808)
    src = torch.randn(1, 2, 8, 12, generator=gen).cuda().requires_grad_(True)
    flow = torch.randn(1, 2, 8, 12, generator=gen).cuda()
    with AF.deterministic():
        y = AF.warp_nearest(src, flow)
        with pytest.raises(_lib.ArflowHipError, match='deterministic'):
            torch.autograd.grad(y.sum(), [src])
    y = AF.warp_nearest(src, flow)
    torch.autograd.grad(y.sum(), [src])  # default mode: as before
