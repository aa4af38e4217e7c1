"""GPU: the pyramid sampler (csrc/gauss_pyr.hip; arflow_amd.gauss_pyr.reparam_pyramid) and the align_corners=True upsample
(csrc/upsample.hip; AF.prob_upsample) per element against the float64 restatements of tests/gauss_pyr_ref.py.

Bounds are derived, not tuned (u = 2^-24, the unit roundoff of fp32):
  z     |z - ref| <= u |z| + 8 u |std eps|.  z = mean + RN(expf(logvar / 2) eps): one rounding of the sum (u |z|); the product
        carries the halving (exact), an expf of up to 3 ulp = 6 u and its own rounding -- inside 8 u of the product.
  ent   rtol 1e-12 against the float64 sum: the terms are float64 from the load on, so only the order of a few thousand
        float64 additions differs (2^-53 per addition).
  gnet  |g - ref| <= 8 u (|gz std eps / 2| + |gent|) + u |g|: the product term as above with two more roundings, gent rounded
        to fp32 once, and the final sum.  gmean = gz is exact.
  prob_upsample: tests/gauss_pyr_ref.py prob_upsample_ref / prob_upsample_adjoint_ref -- the out_up rule 6 u sum w |a + b| plus
        the weight term 4 u max(h, w) (max tap - min tap); the adjoint is the same rule transposed.  tests/
        test_elbo_pyramid_cpu.py holds ATen's own fp32 resize to the same bounds.
Sizes: 1 x 1 x 1; 2 x 3 x 5 (scalar path); 2 x 8 x 12 (float4 path); 1 x 40 x 52 (2 h w = 4160 elements: five 1024-element chunks
per row, the last one partial); a ragged five-scale launch 16 x 24 ... 1 x 2 mixing both paths, and a six-scale one."""
import numpy as np
import pytest
import torch

from tests import gauss_pyr_ref as R

pytestmark = pytest.mark.gpu
U = R.EPS

SINGLE = [(1, 1, 1), (2, 3, 5), (2, 8, 12), (1, 40, 52)]
RAGGED = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]
_cache = {}


def pyramid(B, sizes):
    """Seeded nets, noise, weights of the objective and the float64 references, computed once per key and left unchanged."""
    key = (B, tuple(sizes))
    if key not in _cache:
        g = torch.Generator().manual_seed(100 * B + 7 * len(sizes) + sizes[0][0])
        c = dict(nets=[], eps=[], wz=[], z=[], part=[], ent=[], gnet=[], gmag=[])
        c['went'] = torch.randn(len(sizes), 2, generator=g, dtype=torch.float64)
        for i, (h, w) in enumerate(sizes):
            net = torch.randn(B, 8, h, w, generator=g)
            net[:, 2:4] = 1.5 * net[:, 2:4] - 1.0
            net[:, 6:8] = 1.5 * net[:, 6:8] - 1.0
            eps, wz = torch.randn(B, 4, h, w, generator=g), torch.randn(B, 4, h, w, generator=g)
            z, part, ent = R.sample_np(net.numpy(), eps.numpy())
            gnet, gmag = R.sample_grad_np(net.numpy(), eps.numpy(), wz.numpy(), c['went'][i].numpy())
            for k, v in zip(('nets', 'eps', 'wz', 'z', 'part', 'ent', 'gnet', 'gmag'), (net, eps, wz, z, part, ent, gnet, gmag)):
                c[k].append(v)
        _cache[key] = c
    return _cache[key]


def check_forward(c, zs, ent):
    for i, z in enumerate(zs):
        err = np.abs(z.detach().double().cpu().numpy() - c['z'][i])
        bound = U * np.abs(c['z'][i]) + 8 * U * np.abs(c['part'][i])
        print('scale %d: z max err / bound %.3f' % (i, float((err / np.maximum(bound, 1e-300)).max())))
        assert z.dtype == torch.float32 and (err <= bound).all(), i
    e = ent.detach().cpu().numpy()
    assert ent.dtype == torch.float64 and e.shape == (len(zs), 2)
    ref = np.stack(c['ent'])
    assert (np.abs(e - ref) <= 1e-12 * np.abs(ref)).all(), (e, ref)


def check_backward(c, gnets, gz_scales=None, with_gent=True):
    """gz_scales: the scales whose sample received a gradient (default: all)."""
    for i, g in enumerate(gnets):
        with_gz = gz_scales is None or i in gz_scales
        went = c['went'][i].numpy() if with_gent else np.zeros(2)
        ref, mag = c['gnet'][i], c['gmag'][i]
        if not (with_gz and with_gent):
            ref, mag = R.sample_grad_np(c['nets'][i].numpy(), c['eps'][i].numpy(), c['wz'][i].numpy() if with_gz else None,
                                        went if with_gent else None)
        gent_mag = np.zeros_like(mag)
        for d in range(2):
            gent_mag[:, 4 * d + 2:4 * d + 4] = abs(went[d])
        err = np.abs(g.detach().double().cpu().numpy() - ref)
        bound = 8 * U * (mag + gent_mag) + U * np.abs(ref)
        assert (err <= bound).all(), (i, float(err.max()))
        assert np.array_equal(g[:, 0:2].cpu().numpy(), ref[:, 0:2].astype(np.float32))  # gmean = gz, exactly
        assert np.array_equal(g[:, 4:6].cpu().numpy(), ref[:, 4:6].astype(np.float32))


def run(c, with_gz=True, with_gent=True):
    from arflow_amd.gauss_pyr import reparam_pyramid
    nets = [n.cuda().requires_grad_(True) for n in c['nets']]
    zs, ent = reparam_pyramid(nets, [e.cuda() for e in c['eps']])
    obj = 0.
    if with_gz:
        obj = obj + sum((z.double() * w.cuda().double()).sum() for z, w in zip(zs, c['wz']))
    if with_gent:
        obj = obj + (ent * c['went'].cuda()).sum()
    return zs, ent, torch.autograd.grad(obj, nets)


@pytest.mark.parametrize('shape', SINGLE, ids=str)
def test_single_scale(shape):
    B, h, w = shape
    c = pyramid(B, [(h, w)])
    zs, ent, gnets = run(c)
    check_forward(c, zs, ent)
    check_backward(c, gnets)


@pytest.mark.parametrize('sizes', [RAGGED, RAGGED + [(1, 1)]], ids=['five', 'six'])
def test_ragged_pyramid_in_one_launch(sizes):
    from arflow_amd import functional as AF
    c = pyramid(2, sizes)
    AF.start_kernel_timing()
    zs, ent, gnets = run(c)
    launched = [name for name, _ in AF.stop_kernel_timing()]
    assert launched == ['arflow_gauss_pyr_sample_fwd', 'arflow_gauss_pyr_sample_bwd'], launched  # one call each for all scales
    check_forward(c, zs, ent)
    check_backward(c, gnets)


def test_absent_gradients():
    """gz = NULL (only the entropy sums are used), no entropy gradient, and a gradient into one sample only."""
    from arflow_amd.gauss_pyr import reparam_pyramid
    c = pyramid(2, RAGGED)
    check_backward(c, run(c, with_gz=False)[2], gz_scales=())
    check_backward(c, run(c, with_gent=False)[2], with_gent=False)
    nets = [n.cuda().requires_grad_(True) for n in c['nets']]
    zs, ent = reparam_pyramid(nets, [e.cuda() for e in c['eps']])
    g = torch.autograd.grad((zs[1].double() * c['wz'][1].cuda().double()).sum() + (ent * c['went'].cuda()).sum(), nets)
    check_backward(c, g, gz_scales=(1,))
    assert float(g[0][:, 0:2].abs().max()) == 0 and float(g[1][:, 0:2].abs().max()) > 0


def test_noise_is_drawn_on_the_device():
    from arflow_amd.gauss_pyr import reparam_pyramid
    c = pyramid(2, RAGGED)
    nets = [n.cuda() for n in c['nets']]
    a, ea = reparam_pyramid(nets)
    b, eb = reparam_pyramid(nets)
    assert [tuple(z.shape) for z in a] == [(2, 4) + s for s in RAGGED]
    assert not torch.equal(a[0], b[0]) and torch.equal(ea, eb) and bool(torch.isfinite(a[0]).all())


def test_channel_slices_and_nan_surroundings():
    """Inputs are channel slices of wider tensors (a batch stride of their own); outputs are slots of NaN-filled buffers, at
    an address that is / is not a multiple of 16 bytes: every element is written and nothing around it."""
    from arflow_amd import gauss_pyr as GP
    sizes = [(8, 12), (3, 5)]
    c = pyramid(2, sizes)
    for lead in (0, 1):
        nets, eps, zs, gzs, gnets, bufs = [], [], [], [], [], []
        for i, (h, w) in enumerate(sizes):
            wide = torch.full((2, 12, h, w), float('nan')).cuda()
            wide[:, 2:10] = c['nets'][i].cuda()
            nets.append(wide[:, 2:10])
            ewide = torch.full((2, 6, h, w), float('nan')).cuda()
            ewide[:, 1:5] = c['eps'][i].cuda()
            eps.append(ewide[:, 1:5])
            gwide = torch.full((2, 6, h, w), float('nan')).cuda()
            gwide[:, 2:6] = c['wz'][i].cuda()
            gzs.append(gwide[:, 2:6])
            for C, store in ((4, zs), (8, gnets)):
                flat = torch.full((2 * (C + 3) * h * w + lead,), float('nan'), device='cuda')
                buf = flat[lead:].view(2, C + 3, h, w)
                bufs.append((flat, buf, C))
                store.append(buf[:, 1:1 + C])
        ent = torch.full((4, 2), float('nan'), device='cuda', dtype=torch.float64)
        GP._sample_fwd(nets, eps, zs=zs, ent=ent[1:3])
        check_forward(c, zs, ent[1:3])
        GP._sample_bwd(nets, eps, gzs, c['went'].cuda(), gnets=gnets)
        check_backward(c, gnets)
        assert bool(torch.isnan(ent[0]).all()) and bool(torch.isnan(ent[3]).all())
        for flat, buf, C in bufs:
            assert bool(torch.isnan(buf[:, :1]).all()) and bool(torch.isnan(buf[:, 1 + C:]).all())
            assert bool(torch.isfinite(buf[:, 1:1 + C]).all())
            if lead:
                assert bool(torch.isnan(flat[:1]).all())


def test_runs_are_bitwise_equal_in_both_modes():
    from arflow_amd import functional as AF
    c = pyramid(1, [(40, 52)])
    r = pyramid(2, RAGGED)
    first = [run(c), run(r)]
    flat = lambda t: list(t[0]) + [t[1]] + list(t[2])  # noqa: E731
    second = [run(c), run(r)]
    with AF.deterministic():
        third = [run(c), run(r)]
    for other in (second, third):
        for a, b in zip(first, other):
            assert all(torch.equal(x, y) for x, y in zip(flat(a), flat(b)))


# ---- prob_upsample -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    return functional


def fwd_excess(out, c):
    return float(((out.detach().cpu().double() - c['ref']).abs() - c['bound']).max())


def bwd_excess(g, c):
    return float(((g.detach().cpu().double() - c['gref']).abs() - c['gbound']).max())


@pytest.mark.parametrize('factor', R.UP_FACTORS)
@pytest.mark.parametrize('shape', R.UP_SHAPES, ids=str)
def test_prob_upsample_forward_adjoint_and_identity(AF, shape, factor):
    c = R.up_case(shape, factor)
    x = c['x'].cuda().requires_grad_(True)
    out = AF.prob_upsample(x, factor, 2, 2, R.up_bias(factor))
    e = fwd_excess(out, c)
    print('forward excess %.3e' % e)
    assert out.shape == c['ref'].shape and e <= 0, 'forward outside its bound by %.3e' % e
    (gx,) = torch.autograd.grad(out, x, c['go'].cuda())
    e = bwd_excess(gx, c)
    print('adjoint excess %.3e' % e)
    assert gx.shape == x.shape and e <= 0, 'adjoint outside its bound by %.3e' % e
    # <up(x) - up(0), g> = <x, up^T(g)> in float64 accumulation, to the sum of the two bounds (up is affine: the bias)
    zero = AF.prob_upsample(torch.zeros_like(x), factor, 2, 2, R.up_bias(factor))
    ref0, bound0 = R.prob_upsample_ref(torch.zeros_like(c['x']), factor, 2, 2, R.up_bias(factor))
    assert float(((zero.cpu().double() - ref0).abs() - bound0).max()) <= 0
    go = c['go'].double()
    lhs = float(((out.detach().cpu().double() - zero.cpu().double()) * go).sum())
    rhs = float((c['x'].double() * gx.cpu().double()).sum())
    slack = float(((c['bound'] + bound0) * go.abs()).sum() + (c['gbound'] * c['x'].double().abs()).sum())
    print('identity: %.6e vs %.6e, slack %.3e' % (lhs, rhs, slack))
    assert abs(lhs - rhs) <= slack


@pytest.mark.parametrize('factor', R.UP_FACTORS)
def test_prob_upsample_slice_into_slot(AF, factor):
    """Source = a channel slice of a wider tensor; destination = a slot of a wider NaN-filled buffer at an address that is /
    is not a multiple of 16 bytes; the adjoint reads a slot."""
    for shape in ((2, 4, 24, 32), (2, 4, 3, 5)):
        B, C, h, w = shape
        c = R.up_case(shape, factor)
        wide = torch.full((B, 9, h, w), float('nan')).cuda()
        wide[:, 3:7] = c['x'].cuda()
        for lead in (0, 1):
            flat = torch.full((B * 7 * factor * factor * h * w + lead,), float('nan'), device='cuda')
            buf = flat[lead:].view(B, 7, factor * h, factor * w)
            out = AF.prob_upsample(wide[:, 3:7], factor, 2, 2, R.up_bias(factor), out=buf[:, 2:6])
            assert out.data_ptr() == buf[:, 2:6].data_ptr() and fwd_excess(buf[:, 2:6], c) <= 0
            assert bool(torch.isnan(buf[:, :2]).all()) and bool(torch.isnan(buf[:, 6:]).all())
            if lead:
                assert bool(torch.isnan(flat[:1]).all())
        gwide = torch.full((B, 7, factor * h, factor * w), float('nan')).cuda()
        gwide[:, 2:6] = c['go'].cuda()
        x = wide.clone().nan_to_num(0.0).requires_grad_(True)
        y = AF.prob_upsample(x[:, 3:7], factor, 2, 2, R.up_bias(factor))
        (gx,) = torch.autograd.grad(y, x, gwide[:, 2:6])
        assert bwd_excess(gx[:, 3:7], c) <= 0 and float(gx[:, :3].abs().max()) == 0 and float(gx[:, 7:].abs().max()) == 0


def test_prob_upsample_channel_rules_and_reproducibility(AF):
    """n_flow / n_diag other than (2, 2): the flow-only and the log-variance-only calls of the model's levels; three runs in
    either mode give equal bits."""
    shape = (2, 2, 3, 5)
    for factor, n_flow, n_diag in ((2, 0, 2), (2, 2, 0), (4, 0, 2)):
        c = R.up_case(shape, factor, n_flow, n_diag)
        x = c['x'].cuda().requires_grad_(True)
        out = AF.prob_upsample(x, factor, n_flow, n_diag, R.up_bias(factor))
        assert fwd_excess(out, c) <= 0
        assert bwd_excess(torch.autograd.grad(out, x, c['go'].cuda())[0], c) <= 0
    c = R.up_case((2, 4, 24, 32), 4)

    def once():
        x = c['x'].cuda().requires_grad_(True)
        out = AF.prob_upsample(x, 4, 2, 2, R.up_bias(4))
        return out, torch.autograd.grad(out, x, c['go'].cuda())[0]
    first = once()
    assert all(torch.equal(a, b) for a, b in zip(first, once()))
    with AF.deterministic():
        assert all(torch.equal(a, b) for a, b in zip(first, once()))
    with pytest.raises(ValueError):
        AF.prob_upsample(c['x'].cuda(), 3, 2, 2, 0.5)
    with pytest.raises(ValueError):
        AF.prob_upsample(c['x'].cuda(), 2, 3, 2, 0.5)
