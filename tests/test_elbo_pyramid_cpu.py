"""CPU: the pieces around PWCLiteProb + ElboLoss that need no GPU -- the restatements of
tests/gauss_pyr_ref.py against what the REFERENCE computed (tests/golden/elbo_pyramid.npz, elbo_pyramid_models.npz; made by
tools/make_pwcliteprob_golden.py), the sampler's closed-form gradient against central differences, the error codes of the new
entry points, argument and construction errors, the factories, PWCLiteProb's key list, parameter counts and the three model
cases with the oracle ops patched in (the project's gate for network outputs: EPE <= 1e-3 per channel pair,
tests/test_prob_model_cpu.py::compare), ATen's own fp32 resize inside the upsample bound, the workload entry and the CLI."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import arflow_amd.models as M
from arflow_amd.config import AttrDict as C
from tests import gauss_pyr_ref as R
from tests.helpers import epe, oracle_ops


# ---- the loss restatement against the reference ---------------------------------------------------------------------------
def _inputs(g, dtype=torch.float64):
    nets = [g['net_%d' % i].to(dtype) for i in range(len(R.LOSS_SIZES))]
    eps = [g['eps_%d' % i].to(dtype) for i in range(len(R.LOSS_SIZES))]
    return nets, eps, g['img'].to(dtype)


@pytest.mark.parametrize('tag', list(R.LOSS_CASES))
def test_restatement_equals_the_fixture(golden, tag):
    g = golden('elbo_pyramid')
    assert int(g['seed']) >= 5100
    cfg = R.loss_cfg(tag)
    nets, eps, img = _inputs(g)
    nets = [n.requires_grad_(True) for n in nets]
    res, masks = R.elbo_loss_ref(cfg, nets, img, [eps[i] for i in R.computed_scales(cfg)])
    for name, v in zip(R.LOSS_OUTPUTS, res):
        ref = float(g['%s_%s' % (name, tag)])
        assert abs(float(v.detach()) - ref) <= 1e-10 * max(1.0, abs(ref)), (name, float(v.detach()), ref)
    assert torch.equal(masks[0].double(), g['mask1_' + tag].double()) and torch.equal(masks[1].double(), g['mask2_' + tag].double())
    assert 0.02 < float(1 - masks[0].mean()) < 0.98  # the masks are not trivial
    grads = torch.autograd.grad(res[0], nets, allow_unused=True)
    for i, gr in enumerate(grads):
        ref = g['gnet%d_%s' % (i, tag)]
        got = torch.zeros_like(ref) if gr is None else gr
        assert float((got - ref).abs().max()) <= 1e-10 * max(1.0, float(ref.abs().max())), i
        if cfg.w_scales[i] == 0:
            assert float(ref.abs().max()) == 0


def test_fixture_pins_the_entropy_zip_quirk(golden):
    """skip_mid: scales 0, 2, 3 are computed and meet w_en_scales[0], [1], [2] -- not [0], [2], [3]."""
    g = golden('elbo_pyramid')
    cfg = R.loss_cfg('skip_mid')
    B = R.LOSS_B
    per = {}
    for i in R.computed_scales(cfg):
        _, _, ent = R.sample_np(g['net_%d' % i].numpy(), g['eps_%d' % i].numpy())
        h, w = R.LOSS_SIZES[i]
        per[i] = (ent[0] / (B * h * w) / 2 + ent[1] / (B * h * w) / 2) / 2
    quirk = cfg.w_entropy * sum(per[i] * cfg.w_en_scales[k] for k, i in enumerate(sorted(per)))
    aligned = cfg.w_entropy * sum(per[i] * cfg.w_en_scales[i] for i in per)
    ref = float(g['entropy_skip_mid'])
    assert abs(quirk - ref) <= 1e-12 * abs(ref) and abs(aligned - ref) > 1e-3 * abs(ref)


def test_closed_form_gradient_against_central_differences():
    rng = np.random.default_rng(5)
    sizes = [(3, 5), (1, 2)]
    nets = [rng.standard_normal((2, 8, h, w)) for h, w in sizes]
    eps = [rng.standard_normal((2, 4, h, w)) for h, w in sizes]
    wz = [rng.standard_normal((2, 4, h, w)) for h, w in sizes]
    went = rng.standard_normal((2, 2))
    step = 1e-6
    for i in range(2):
        g, _ = R.sample_grad_np(nets[i], eps[i], wz[i], went[i])
        num = np.zeros_like(g)
        it = np.nditer(nets[i], flags=['multi_index'])
        for _ in it:
            k = it.multi_index
            old = nets[i][k]
            nets[i][k] = old + step
            up = R.pyramid_objective_np(nets, eps, wz, went)
            nets[i][k] = old - step
            dn = R.pyramid_objective_np(nets, eps, wz, went)
            nets[i][k] = old
            num[k] = (up - dn) / (2 * step)
        assert np.abs(num - g).max() <= 1e-7 * max(1.0, np.abs(g).max())


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from arflow_amd import _lib
    return _lib.load()


def test_error_codes_of_the_new_entry_points(lib):
    """Validation happens before anything is launched, so these are safe on a host without a GPU."""
    ENULL, ESHAPE, EPARAM = -1001, -1002, -1003
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    longs = lambda *v: (ctypes.c_long * len(v))(*v)  # noqa: E731
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)  # noqa: E731
    h, w = ints(4, 2), ints(6, 3)
    assert lib.arflow_gauss_pyr_work_size(h, w, 2, 3) == 2 * 3 * 1 + 2 * 3 * 1  # one chunk per (b, d) row at either scale
    assert lib.arflow_gauss_pyr_work_size(ints(40), ints(52), 1, 1) == 2 * 5  # 2 * 40 * 52 = 4160 elements: 5 chunks of 1024
    assert lib.arflow_gauss_pyr_work_size(h, w, 0, 3) == EPARAM and lib.arflow_gauss_pyr_work_size(h, w, 7, 3) == EPARAM
    assert lib.arflow_gauss_pyr_work_size(h, w, 2, 0) == ESHAPE and lib.arflow_gauss_pyr_work_size(ints(4, 0), w, 2, 3) == ESHAPE
    assert lib.arflow_gauss_pyr_work_size(None, w, 2, 3) == ENULL
    one = 16
    good = dict(net=ptrs(one, one), nbs=longs(8 * 24, 8 * 6), eps=ptrs(one, one), ebs=longs(4 * 24, 4 * 6), z=ptrs(one, one),
                zbs=longs(4 * 24, 4 * 6), h=h, w=w, n=2, B=3, work=one, ent=one)

    def fwd(**change):
        a = dict(good, **change)
        return lib.arflow_gauss_pyr_sample_fwd(a['net'], a['nbs'], a['eps'], a['ebs'], a['z'], a['zbs'], a['h'], a['w'], a['n'],
                                               a['B'], a['work'], a['ent'], None)

    def bwd(**change):
        a = dict(good, gz=ptrs(one, None), gent=one, **change)
        return lib.arflow_gauss_pyr_sample_bwd(a['gz'], a['zbs'], a['net'], a['nbs'], a['eps'], a['ebs'], a['gent'], a['z'],
                                               a['nbs'], a['h'], a['w'], a['n'], a['B'], None)
    for call in (fwd, bwd):
        assert call(net=None) == ENULL and call(net=ptrs(one, None)) == ENULL and call(eps=ptrs(None, one)) == ENULL
        assert call(z=None) == ENULL and call(h=None) == ENULL
        assert call(n=0) == EPARAM and call(n=7) == EPARAM
        assert call(B=0) == ESHAPE and call(w=ints(6, -3)) == ESHAPE
        assert call(nbs=longs(8 * 24 - 1, 8 * 6)) == ESHAPE and call(ebs=longs(4 * 24, 4 * 6 - 1)) == ESHAPE
    assert fwd(work=None) == ENULL and fwd(ent=None) == ENULL and fwd(zbs=longs(4 * 24 - 1, 4 * 6)) == ESHAPE
    assert bwd(zbs=longs(4 * 24 - 1, 4 * 6)) == ESHAPE  # the stride of a gz that is given
    # the align_corners=True upsample: the checks of arflow_out_up2_* plus the factor
    up = dict(i=one, ibs=60, o=one, obs=60 * 16, B=2, C=4, h=3, w=5, f=4, nf=2, nd=2)
    faults = [(dict(i=None), ENULL), (dict(o=None), ENULL), (dict(B=0), ESHAPE), (dict(h=0), ESHAPE), (dict(w=-1), ESHAPE),
              (dict(ibs=59), ESHAPE), (dict(obs=60 * 16 - 1), ESHAPE), (dict(f=3), EPARAM), (dict(f=1), EPARAM),
              (dict(nf=-1), EPARAM), (dict(nf=3, nd=2), EPARAM),
              (dict(h=2049, ibs=4 * 2049 * 5, obs=16 * 4 * 2049 * 5), ESHAPE), (dict(w=2049, ibs=4 * 3 * 2049, obs=16 * 4 * 3 * 2049), ESHAPE)]
    # (the last two: strides large enough for the item, so that only the h, w <= 2048 limit of these entry points can object)
    for change, want in faults:
        a = dict(up, **change)
        assert lib.arflow_prob_up_fwd(a['i'], a['ibs'], a['o'], a['obs'], a['B'], a['C'], a['h'], a['w'], a['f'], a['nf'], a['nd'],
                                      0.5, None) == want, change
        if 'nd' not in change:
            assert lib.arflow_prob_up_bwd(a['o'], a['obs'], a['i'], a['ibs'], a['B'], a['C'], a['h'], a['w'], a['f'], a['nf'],
                                          None) == want, change
    lib.arflow_take_stale_error()


def test_argument_and_construction_errors():
    from arflow_amd import _lib, functional as AF
    from arflow_amd.gauss_pyr import reparam_pyramid
    from arflow_amd.losses import ElboLoss
    net, eps = torch.zeros(2, 8, 3, 5), torch.zeros(2, 4, 3, 5)
    with pytest.raises(_lib.ArflowHipError, match='GPU only'):
        reparam_pyramid([net], [eps])
    with pytest.raises(ValueError, match=r'nets\[0\] must be a \[B,8,h,w\]'):
        reparam_pyramid([eps], [eps])
    with pytest.raises(ValueError, match='1..6'):
        reparam_pyramid([net] * 7, [eps] * 7)
    with pytest.raises(ValueError, match='1..6'):
        reparam_pyramid([])
    with pytest.raises(ValueError, match='batch'):
        reparam_pyramid([net, torch.zeros(3, 8, 2, 2)], [eps, eps])
    with pytest.raises(ValueError, match='one per scale'):
        reparam_pyramid([net], [eps, eps])
    with pytest.raises(_lib.ArflowHipError):
        AF.prob_upsample(net, 2, 2, 2, 0.5)
    loss = ElboLoss(R.loss_cfg('skip_mid'))
    outs = [torch.zeros(2, 8, h, w) for h, w in R.LOSS_SIZES]
    with pytest.raises(ValueError, match='non-zero w_scales entry: 3'):
        loss(outs, torch.zeros(2, 6, 32, 64), eps=[eps] * 4)
    with pytest.raises(ValueError, match=r'output\[0\] must be \[B,8,h,w\]'):
        loss([o[:, :4] for o in outs], torch.zeros(2, 6, 32, 64))
    with pytest.raises(NotImplementedError):
        M.get_model(R.model_cfg('U0'))(torch.zeros(1, 9, 64, 64))


def test_all_scales_skipped_behaves_as_unflow_loss():
    """w_scales all zero: nothing is sampled (so this runs without a GPU); the terms are unFlowLoss' own and the reference's
    empty entropy list sums to 0."""
    from arflow_amd.losses import ElboLoss, unFlowLoss
    cfg = R.loss_cfg('full')
    cfg.w_scales = [0.0] * 5
    outs = [torch.randn(2, 8, h, w, generator=torch.Generator().manual_seed(h)) for h, w in R.LOSS_SIZES]
    img = torch.rand(2, 6, 32, 64, generator=torch.Generator().manual_seed(1))
    got = ElboLoss(cfg)(outs, img)
    ref = unFlowLoss(cfg)([o[:, 0:4] for o in outs], img)
    assert got[0] == ref[0] and got[1] == ref[1] and got[2] == ref[2] and got[3] == 0
    assert float(got[4]) == float(outs[0].abs().mean())


def test_factories_dispatch():
    from arflow_amd.losses import ElboLoss, get_loss, unFlowLoss
    loss = get_loss(R.loss_cfg('full'))
    assert isinstance(loss, ElboLoss) and isinstance(loss.flow_loss, unFlowLoss) and loss.flow_loss.cfg is loss.cfg
    assert isinstance(M.get_model(R.model_cfg('U1')), M.PWCLiteProb)
    with pytest.raises(NotImplementedError):
        get_loss(C(type='mse'))


# ---- the model ----------------------------------------------------------------------------------------------------------------
def run_case(tag, device='cpu', oracle=True):
    x, insum = R.make_model_input(tag)
    model = R.prepare(M.get_model(R.model_cfg(tag)), tag).to(device)
    torch.set_num_threads(8)
    with torch.no_grad():
        if oracle:
            with oracle_ops(model):
                res = model(x.to(device), with_bk=True)
        else:
            res = model(x.to(device), with_bk=True)
    return model, res, insum


def compare(g, tag, res, gate=1e-3):
    assert len(res['flows_fw']) == 5 and len(res['flows_bw']) == 5
    k = 4 if R.MODEL_CASES[tag]['upsample'] else 1
    for d in ('flows_fw', 'flows_bw'):
        for lvl, f in enumerate(res[d]):
            assert tuple(f.shape) == (R.MODEL_CASES[tag]['batch'], 4, k * R.MODEL_H // 2 ** (lvl + 2), k * R.MODEL_W // 2 ** (lvl + 2))
    got = R.collect(res, tag)
    assert len(got) == 10
    for name, arr in got.items():
        ref = g[name]
        arr = torch.from_numpy(arr)
        assert arr.shape == ref.shape, name
        for c in (0, 2):
            e = epe(arr[:, c:c + 2], ref[:, c:c + 2])
            print('%s channels %d:%d EPE %.3e' % (name, c, c + 2, e))
            assert e <= gate, '%s channels %d:%d: EPE %.3e vs the reference' % (name, c, c + 2, e)


@pytest.mark.parametrize('tag', list(R.MODEL_CASES))
def test_model_matches_the_reference(golden, tag):
    g = golden('elbo_pyramid_models')
    model, res, insum = run_case(tag)
    assert insum == float(g['insum_' + tag]), 'the seeded input drifted from the one the fixture was made with'
    keys = g['keys_' + tag]
    assert list(model.state_dict().keys()) == keys and len(keys) == R.MODEL_KEYS
    n = model.num_parameters()
    assert n == int(g['params_' + tag]) == R.MODEL_PARAMS[R.MODEL_CASES[tag]['reduce_dense']]
    compare(g, tag, res)


def test_clamp_binds_in_the_clamp_case_only(golden):
    g = golden('elbo_pyramid_models')
    top = lambda tag: max(float(g['out_%s_%s_%d' % (tag, d, l)][:, 2:4].max()) for d in ('fw', 'bw') for l in range(5))  # noqa: E731
    assert top('clamp') == 10.0 and top('U0') < 10.0
    assert float((g['out_clamp_fw_0'][:, 2:4] == 10.0).float().mean()) > 0.5


def test_init_weights_as_pwclite():
    m = M.PWCLiteProb(R.model_cfg('U0'))
    torch.manual_seed(0)
    m.init_weights()
    w = m.context_networks.convs[2][0].weight
    assert abs(float(w.detach().std()) / (2.0 / w[0].numel()) ** 0.5 - 1) < 0.05
    assert all(float(p.detach().abs().max()) == 0 for n, p in m.named_parameters() if n.endswith('bias'))
    assert m.flow_estimators.predict_flow[0].out_channels == 4 and m.context_networks.convs[6][0].out_channels == 4


def test_existing_blocks_keep_two_channel_heads():
    from arflow_amd.models import blocks
    assert blocks.FlowEstimatorDense(10).conv_last[0].out_channels == 2
    assert blocks.FlowEstimatorReduce(10).predict_flow[0].out_channels == 2
    assert blocks.ContextNetwork(10).convs[6][0].out_channels == 2


# ---- the upsample bound without a GPU ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('factor', R.UP_FACTORS)
@pytest.mark.parametrize('shape', R.UP_SHAPES, ids=str)
def test_aten_fp32_resize_sits_inside_the_upsample_bound(shape, factor):
    """F.interpolate(align_corners=True) in fp32 on the CPU -- the composed path the model keeps for CPU tensors -- against
    the float64 restatement: inside the forward bound at every pixel, and its autograd adjoint inside the transposed bound.
    The float64 restatement itself equals ATen's float64 resize."""
    c = R.up_case(shape, factor)
    bias = R.up_bias(factor)
    interp = lambda t: torch.nn.functional.interpolate(t, scale_factor=factor, mode='bilinear', align_corners=True)  # noqa: E731

    def composed(x):
        return torch.cat([interp(x[:, 0:2] * factor), interp(x[:, 2:4] + bias)], 1)
    assert torch.allclose(composed(c['x'].double()), c['ref'], rtol=0, atol=1e-13)
    x = c['x'].clone().requires_grad_(True)
    out = composed(x)
    excess = float(((out.detach().double() - c['ref']).abs() - c['bound']).max())
    print('forward excess %.3e' % excess)
    assert excess <= 0
    (gx,) = torch.autograd.grad(out, x, c['go'])
    excess = float(((gx.double() - c['gref']).abs() - c['gbound']).max())
    print('adjoint excess %.3e' % excess)
    assert excess <= 0
    # the restatement evaluated in fp32 as well
    out32, _ = R.prob_upsample_ref(c['x'], factor, 2, 2, bias, dtype=torch.float32)
    assert float(((out32.double() - c['ref']).abs() - c['bound']).max()) <= 0


def test_upsample_bound_tells_mutations_apart():
    c = R.up_case((2, 4, 3, 5), 2)
    x = c['x'].double()
    s, b = R.chan_rule(4, 2, 2, 2, R.up_bias(2), torch.float64)
    half_pixel = torch.nn.functional.interpolate(x + b, scale_factor=2, mode='bilinear', align_corners=False) * s
    muts = {'align_corners=False': half_pixel, 'no bias': s * R.up_align(x, 2), 'scale on a log-variance channel': 2 * R.up_align(x + b, 2)}
    for name, out in muts.items():
        assert float(((out - c['ref']).abs() - c['bound']).max()) > 0, name


# ---- workload and CLI ---------------------------------------------------------------------------------------------------------
def test_workload_entry_builds_model_and_loss():
    from arflow_amd.losses import ElboLoss, get_loss
    from arflow_amd.train_step import WORKLOADS
    mcfg, lcfg = WORKLOADS['pwcliteprob+elbo_loss']
    model, loss = M.get_model(C(mcfg)), get_loss(C(lcfg))
    assert isinstance(model, M.PWCLiteProb) and isinstance(loss, ElboLoss)
    assert model.upsample and model.reduce_dense and model.num_parameters() == R.MODEL_PARAMS[True]
    ref = WORKLOADS['pwclite+unflow_loss'][1]
    for k in ('w_l1', 'w_ssim', 'w_ternary', 'warp_pad', 'alpha', 'occ_from_back', 'with_bk', 'w_smooth'):
        assert lcfg[k] == ref[k], k
    assert lcfg['w_scales'] == [1.0] * 5 and lcfg['w_sm_scales'] == ref['w_sm_scales'][:5]
    assert lcfg['w_en_scales'] == [1.0] * 5 and lcfg['w_entropy'] == 0.1


def test_cli_arch_pwclite_prob(monkeypatch):
    from arflow_amd import inference
    model = inference.build_model('pwclite_prob', 2)
    assert isinstance(model, M.PWCLiteProb) and model.upsample and not model.training
    with pytest.raises(ValueError, match='two frames'):
        inference.build_model('pwclite_prob', 3)
    frames = [torch.rand(3, 64, 64, generator=torch.Generator().manual_seed(i)) for i in (1, 2)]
    with oracle_ops(model):
        flow, ent = inference.infer(model, frames, torch.device('cpu'), want_entropy=True)
        with torch.no_grad():
            res = model(torch.cat(frames, 0).unsqueeze(0), with_bk=False)
    full = res['flows_fw'][0][0].permute(1, 2, 0).numpy()
    assert flow.shape == ent.shape == (64, 64, 2)
    assert np.array_equal(flow, full[..., 0:2]) and np.array_equal(ent, full[..., 2:4] / 2)  # log sigma, not log variance
    with pytest.raises(ValueError, match='entropy'):
        inference.infer(inference.build_model('pwclite', 2), frames, torch.device('cpu'), want_entropy=True)
    # the parser takes the value (and --entropy-out with it); without a GPU the CLI then stops at its device check
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(sys, 'argv', ['inference', '--arch', 'pwclite_prob', '-i', 'a.png', 'b.png', '--entropy-out', 'e.npy'])
    with pytest.raises(SystemExit, match='needs a GPU'):
        inference.main()
