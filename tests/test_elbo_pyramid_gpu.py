"""GPU: ElboLoss and PWCLiteProb on the gfx950 kernels against what the reference computed
(tests/golden/elbo_pyramid.npz, elbo_pyramid_models.npz).

Loss bounds: the rule of tests/test_elbo_gpu.py -- each output is held to the larger of 8 x the stored gap between the
reference's OWN fp32 and float64 runs times the output's largest magnitude, and tests/test_elbo_gpu.py::_project_bound
(5e-8 + 3e-6 |ref| for loss terms, 2e-7 + 2e-4 max|ref| + 2e-3 |ref| for gradients); the scale-0 masks are compared for
equality (the fixture's inputs keep every pixel of the thresholded quantity 1e-4 away from its threshold).
Model: the project's gate for network outputs, EPE <= 1e-3 per channel pair; parameter gradients against the oracle twin under
the fixed bound tests/test_models_gpu.py applies to pwclite2 (1e-3 of max|g| with the activations linear)."""
import numpy as np
import pytest
import torch

from tests import gauss_pyr_ref as R
from tests.helpers import oracle_ops
from tests.test_elbo_gpu import _project_bound
from tests.test_elbo_pyramid_cpu import compare, run_case

pytestmark = pytest.mark.gpu


def _run_loss(g, tag, pair=True):
    from arflow_amd.losses import get_loss
    cfg = R.loss_cfg(tag)
    cu = lambda name: torch.from_numpy(np.array(g.raw(name))).cuda()  # noqa: E731
    nets = [cu('net_%d' % i).requires_grad_(True) for i in range(len(R.LOSS_SIZES))]
    loss = get_loss(cfg)
    loss.flow_loss.pair = pair
    res = loss(nets, cu('img'), eps=[cu('eps_%d' % i) for i in R.computed_scales(cfg)])
    grads = torch.autograd.grad(res[0], nets, allow_unused=True)
    out = dict(zip(R.LOSS_OUTPUTS, res))
    out.update(mask1=loss.pyramid_occu_mask1[0], mask2=loss.pyramid_occu_mask2[0])
    for i, gr in enumerate(grads):
        out['gnet%d' % i] = torch.zeros_like(nets[i]) if gr is None else gr
    return {k: torch.as_tensor(v).detach().double().cpu().numpy() for k, v in out.items()}


def _against_the_reference(g, tag, got):
    bad = []
    for key in sorted(got):
        ref = g.raw('%s_%s' % (key, tag)).astype(np.float64)
        assert got[key].shape == ref.shape, key
        if key.startswith('mask'):
            print('%s %-8s %d pixels differ, %d occluded' % (tag, key, int((got[key] != ref).sum()), int((ref == 0).sum())))
            if not np.array_equal(got[key], ref):
                bad.append(key)
            continue
        kind = 'grad' if key.startswith('gnet') else 'term'
        bound = np.maximum(8 * float(g.raw('noise_%s_%s' % (key, tag))) * np.abs(ref).max(), _project_bound(kind, ref))
        err = np.abs(got[key] - ref)
        print('%s %-8s max err %.3e  max err / bound %.3f  max|ref| %.3e' % (tag, key, err.max(), (err / bound).max(),
                                                                            np.abs(ref).max()))
        if not (np.isfinite(got[key]).all() and (err <= bound).all()):
            bad.append(key)
    assert not bad, bad


@pytest.mark.parametrize('tag', list(R.LOSS_CASES))
def test_loss_against_the_reference(golden, tag):
    g = golden('elbo_pyramid')
    got = _run_loss(g, tag)
    _against_the_reference(g, tag, got)
    total = got['warp'] + got['smooth'] - got['entropy']
    assert abs(total - got['total']) <= 5e-8 + 3e-6 * abs(total)


def test_full_with_the_sequential_flow_loss(golden):
    """The internal unFlowLoss with pair = False (one direction after the other, the reference's order): the same bounds, and
    the launches say which path ran."""
    from arflow_amd import functional as AF
    g = golden('elbo_pyramid')
    launched = {}
    for pair in (True, False):
        AF.start_kernel_timing()
        got = _run_loss(g, 'full', pair=pair)
        launched[pair] = {name for name, _ in AF.stop_kernel_timing()}
    assert 'arflow_photo_warp_fwd' in launched[True] and 'arflow_photo_warp_fwd' not in launched[False], launched
    assert {'arflow_gauss_pyr_sample_fwd', 'arflow_gauss_pyr_sample_bwd'} <= launched[True] & launched[False]
    _against_the_reference(g, 'full', got)


def test_noise_on_the_device_and_reproducibility(golden):
    """eps=None draws on the device: two calls differ; with the stored noise two calls agree bit for bit, also in
    deterministic mode."""
    from arflow_amd import functional as AF
    from arflow_amd.losses import ElboLoss
    g = golden('elbo_pyramid')
    cu = lambda name: torch.from_numpy(np.array(g.raw(name))).cuda()  # noqa: E731
    loss = ElboLoss(R.loss_cfg('full'))
    nets = [cu('net_%d' % i) for i in range(5)]
    a, b = loss(nets, cu('img')), loss(nets, cu('img'))
    assert bool(torch.isfinite(a[0])) and float(a[0]) != float(b[0]) and float(a[3]) == float(b[3])
    one = _run_loss(g, 'full')
    with AF.deterministic():
        two, three = _run_loss(g, 'full'), _run_loss(g, 'full')
    for key in one:
        assert np.array_equal(two[key], three[key]), key
    for key in ('entropy', 'absmean', 'mask1', 'mask2'):  # the sampler and the masks do not depend on the mode
        assert np.array_equal(one[key], two[key]), key


def test_entropy_weights_are_read_on_every_call(golden):
    """cfg.w_entropy / cfg.w_en_scales changed between two calls of one loss object (a weight schedule) take effect, as in the
    reference, which reads cfg on every call."""
    from arflow_amd.losses import ElboLoss
    g = golden('elbo_pyramid')
    cu = lambda name: torch.from_numpy(np.array(g.raw(name))).cuda()  # noqa: E731
    cfg = R.loss_cfg('full')
    loss = ElboLoss(cfg)
    nets, eps, img = [cu('net_%d' % i) for i in range(5)], [cu('eps_%d' % i) for i in range(4)], cu('img')
    first = float(loss(nets, img, eps=eps)[3])
    cfg.w_entropy = 0.2
    assert abs(float(loss(nets, img, eps=eps)[3]) - 2 * first) <= 3e-6 * abs(2 * first)
    cfg.w_entropy, cfg.w_en_scales = 0.1, [0.0, 0.0, 0.0, 0.0, 0.0]
    assert float(loss(nets, img, eps=eps)[3]) == 0


# ---- the model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', list(R.MODEL_CASES))
def test_model_cases_on_the_kernels(golden, tag):
    g = golden('elbo_pyramid_models')
    _, res, insum = run_case(tag, device='cuda', oracle=False)
    assert insum == float(g['insum_' + tag])
    compare(g, tag, res)


def test_wiring_warp_up2_prob_upsample_and_no_interpolate():
    """Per direction the reference calls F.interpolate nine times on the log-variance path (four x2, five x4) and as often on
    the flow; here every level above the coarsest folds the flow's x2 into the warp launch, the log-variance comes up with
    prob_upsample(.., 2, 0, 2), the five outputs are one prob_upsample(state, 4, 2, 2) each, and ATen's resize is never
    called.  Both directions run as one pass at batch 2B."""
    import torch.nn.functional as F
    import arflow_amd.functional as AF
    import arflow_amd.models as M
    x, _ = R.make_model_input('U1')
    model = R.prepare(M.get_model(R.model_cfg('U1')), 'U1').cuda()
    calls = {'warp': [], 'up': [], 'interp': 0}
    old = (AF.warp_up2, AF.prob_upsample, F.interpolate)

    def warp(src, flow, **kw):
        calls['warp'].append((tuple(src.shape[2:]), tuple(flow.shape)))
        return old[0](src, flow, **kw)

    def up(t, factor, n_flow, n_diag, bias, out=None):
        calls['up'].append((tuple(t.shape), factor, n_flow, n_diag, round(float(bias), 6)))
        return old[1](t, factor, n_flow, n_diag, bias, out)

    def interp(*a, **k):
        calls['interp'] += 1
        return old[2](*a, **k)
    AF.warp_up2, AF.prob_upsample, F.interpolate = warp, up, interp
    try:
        with torch.no_grad():
            res = model(x.cuda(), with_bk=True)
    finally:
        AF.warp_up2, AF.prob_upsample, F.interpolate = old
    sizes = [(2, 3), (4, 6), (8, 12), (16, 24), (32, 48)]
    assert calls['warp'] == [(sizes[k], (2, 2) + sizes[k - 1]) for k in range(1, 5)], calls
    ln2, ln4 = round(2 * float(np.log(2)), 6), round(2 * float(np.log(4)), 6)
    assert calls['up'] == [((2, 2) + s, 2, 0, 2, ln2) for s in sizes[:4]] + [((2, 4) + s, 4, 2, 2, ln4) for s in sizes], calls
    assert calls['interp'] == 0 and len(res['flows_fw']) == 5 and res['flows_fw'][0].shape == (1, 4, 128, 192)


def _objective(res, x, warp, smooth):
    """tests/test_models_gpu.py::_smooth_objective (threshold-free photometric + smoothness, continuous in the flows) on the
    flow channels of all ten outputs, plus a term that is linear in the log-variance channels with weights of one sign (the
    area-resized target's luminance), so that no parameter's gradient is a near-cancellation."""
    import torch.nn.functional as F
    from tests.test_models_gpu import _smooth_objective
    total = _smooth_objective([f[:, 0:2] for f in res['flows_fw']], [f[:, 0:2] for f in res['flows_bw']], x, warp, smooth)
    for k, img in (('flows_fw', x[:, :3]), ('flows_bw', x[:, 3:6])):
        for lv, f in enumerate(res[k]):
            lum = F.interpolate(img, tuple(f.shape[2:]), mode='area').mean(1, keepdim=True)
            total = total + 0.1 * (f[:, 2:4] * lum).mean() / (lv + 1)
    return total


def _param_grads(dev, hip, x):
    """The model's parameter gradients with the HIP ops (hip=True) or with the oracle ops patched in, the LeakyReLU behind
    every conv replaced by the identity on either side (`linear` of tests/test_models_gpu.py::_param_grads)."""
    import arflow_amd.models as M
    import arflow_amd.models.blocks as mb
    from arflow_amd import loss_blocks as LB
    from arflow_amd.config import AttrDict as C
    from arflow_amd.warp_utils import flow_warp
    from oracle import ops as O
    m = R.prepare(M.get_model(C(type='pwclite_prob', upsample=True, n_frames=2, reduce_dense=True)), 'U0').to(dev).train()
    xx = x.to(dev)
    if hip:
        old = mb.bias_act
        mb.bias_act = lambda y, b, s: old(y, b, 1.0)
        try:
            # (the model asks `blocks.bias_act is AF.bias_leaky_relu` before it takes its native upsample: asked here, with the
            # slope-1 wrapper in place, it would keep the ATen resize -- the wrapper is the same kernel, so say yes)
            m._native_up = lambda t: True
            res = m(xx, with_bk=True)
        finally:
            mb.bias_act = old
        loss = _objective(res, xx, flow_warp, LB.smooth_grad_1st)
    else:
        with oracle_ops(m):
            mb.bias_act = lambda y, b, s: y + b.view(1, -1, 1, 1)  # restored by oracle_ops on exit
            res = m(xx, with_bk=True)
            loss = _objective(res, xx, O.flow_warp, O.smooth_grad_1st)
    g = torch.autograd.grad(loss, list(m.parameters()), allow_unused=True)
    return float(loss.detach()), [None if t is None else t.detach().cpu().double() for t in g], [n for n, _ in m.named_parameters()]


def test_parameter_gradients_elementwise_vs_the_oracle_twin():
    """Whole-model backward, element-wise per parameter tensor, under the FIXED bound tests/test_models_gpu.py::
    test_model_parameter_gradients_elementwise applies to ('pwclite2', linear): activations behind the convs replaced by the
    identity, the model on the kernels against the oracle twin on the CPU, 1e-3 of max|g| per parameter, strictly; the
    losses agree to 2e-6.  The workload's model (upsample, reduce_dense) at 1 x 128 x 192; the objective reaches all ten outputs,
    so every prob_upsample adjoint (x2 and x4), the clamp, the warp_up2 backward and the 4-channel heads run.
    That test's other form -- LeakyReLU kept, bound widened by the oracle twin's own GPU-vs-CPU spread -- is not used here: with
    an earlier objective the oracle twin on the GPU against the oracle twin on the CPU gave 3.0e-3, 3.0e-3 and 1.0e-1 of max|g|
    in three sessions on the same code (a kink that MIOpen's choice of convolution flips; the kernels sat 7.5e-6 from the twin
    in the first two), which measures the oracle against itself and says nothing about the kernels."""
    from tests.test_models_gpu import _worst_rel
    x, _ = R.make_model_input('U1')
    torch.set_num_threads(16)
    l_hip, g_hip, names = _param_grads('cuda', True, x)
    l_cpu, g_cpu, _ = _param_grads('cpu', False, x)
    print('losses: kernels %.8e, oracle twin on the CPU %.8e' % (l_hip, l_cpu))
    assert abs(l_hip - l_cpu) <= 2e-6 * abs(l_cpu), (l_hip, l_cpu)
    w = _worst_rel(g_hip, g_cpu, names)
    print('worst parameter %s: %.3e of max|g|' % (w[1], w[0]))
    assert w[0] <= 1e-3, 'worst parameter gradient vs the CPU oracle twin: %s differs by %.3e of its max' % (w[1], w[0])
    grads = dict(zip(names, g_hip))
    assert float(grads['context_networks.convs.6.0.weight'][2:4].abs().max()) > 0  # the log-variance head is reached
    assert all(g is not None for g in g_hip)


def test_three_training_steps_of_the_workload():
    """TrainStep('pwcliteprob+elbo_loss') at batch 2, 128 x 192: the loss stays finite, every parameter has a finite gradient
    and the parameters move."""
    from arflow_amd.train_step import TrainStep, synthetic_pairs
    dev = torch.device('cuda')
    step = TrainStep('pwcliteprob+elbo_loss', dev, seed=1234)
    x = synthetic_pairs(2, 128, 192, device=dev, seed=5)
    head = step.model.context_networks.convs[6][0]
    before = head.weight.detach().clone()
    for i in range(3):
        loss = step(x)
        assert bool(torch.isfinite(loss)), (i, float(loss))
        for n, p in step.model.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (i, n)
        assert float(head.weight.grad[2:4].abs().max()) > 0, i
    assert not torch.equal(before, head.weight.detach())
