"""GPU: UFlowElboLoss with approx 'mixture' on every loss case of tests/golden/elbo_mixture.npz -- what the reference's own loss
computed in float64 on the stored inputs, the stored noise and the stored component draws --, ComponentNet against the
fixture's `component` case, and one training step of the componentnet+uflow_elbo_mixture workload.

Bounds: the rule of tests/test_elbo_gpu.py (KIND and _project_bound are imported from there).  Each output is held to the larger of
  * 8 x the stored gap between the reference's OWN fp32 and float64 runs, times the output's largest magnitude, and
  * the bound the project applies to the same kernels in tests/test_bench_shapes_gpu.py: 5e-8 + 3e-6 |ref| for loss terms,
    2e-6 + 1e-5 |ref| for masks, 2e-7 + 2e-4 max|ref| + 2e-3 |ref| for gradients (the weights' gradients are gradients).
The total is recomputed from the returned terms.  The launches are the mixture kernels' and none of the banded or the low-rank
family's.  ComponentNet: EPE <= 1e-3 on every stored channel pair, the gate tests/test_prob_model_gpu.py applies to PWCProbFlow."""
import numpy as np
import pytest
import torch

from tests import mixture_ref as R
from tests.test_elbo_gpu import KIND, _project_bound

pytestmark = pytest.mark.gpu

KINDS = dict(KIND, gweights12='grad', gweights21='grad')


def _case(g, tag):
    names = ['net12', 'net21', 'eps12', 'eps21', 'comp12', 'comp21'] + (['weights12', 'weights21'] if tag in R.WEIGHTED else [])
    case = {k: g.raw('%s_%s' % (k, tag)) for k in names}
    case.update(im1=g.raw('im1'), im2=g.raw('im2'))
    return case


def _run(g, tag, of=0):
    """of: the index of the returned term whose gradients are taken (0: the total, 3: the entropy term)."""
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    t = {k: torch.from_numpy(np.array(v)).cuda() for k, v in _case(g, tag).items()}
    net12, net21 = t['net12'].requires_grad_(True), t['net21'].requires_grad_(True)
    res_dict = {'flows_fw': [None, None, net12], 'flows_bw': [None, None, net21]}
    leaves = [net12, net21]
    if tag in R.WEIGHTED:
        res_dict.update(weights_fw=t['weights12'].requires_grad_(True), weights_bw=t['weights21'].requires_grad_(True))
        leaves += [res_dict['weights_fw'], res_dict['weights_bw']]
    loss = get_loss(AttrDict(R.case_cfg(tag)))
    res = loss(res_dict, t['im1'], t['im2'], eps=(t['eps12'], t['eps21']), comp=(t['comp12'], t['comp21']))
    grads = torch.autograd.grad(res[of], leaves, allow_unused=True)
    grads = [torch.zeros_like(x) if gr is None else gr for x, gr in zip(leaves, grads)]
    out = dict(zip(R.OUTPUTS[:8], res))
    out.update(zip(('gnet12', 'gnet21', 'gweights12', 'gweights21'), grads))
    return {k: torch.as_tensor(v).detach().double().cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('tag', list(R.CASES))
def test_loss_against_the_reference(golden, tag):
    from arflow_amd import functional as AF
    g = golden('elbo_mixture')
    AF.start_kernel_timing()
    got = _run(g, tag)
    launched = {name for name, _ in AF.stop_kernel_timing()}
    assert {'arflow_mixture_sample_fwd', 'arflow_mixture_logpdf_fwd', 'arflow_mixture_bwd'} <= launched, launched
    assert not {n for n in launched if n.startswith(('arflow_band_', 'arflow_lowrank_'))}, launched
    assert set(got) == set(R.case_outputs(tag))
    bad = []
    for key in R.case_outputs(tag):
        ref = g.raw('%s_%s' % (key, tag))
        assert got[key].shape == ref.shape, key
        bound = np.maximum(8 * float(g.raw('noise_%s_%s' % (key, tag))) * np.abs(ref).max(), _project_bound(KINDS[key], ref))
        err = np.abs(got[key] - ref)
        print('%s %-12s max err %.3e  max err / bound %.3f  max|ref| %.3e' % (tag, key, err.max(), (err / bound).max(),
                                                                              np.abs(ref).max()))
        if not (np.isfinite(got[key]).all() and (err <= bound).all()):
            bad.append(key)
    assert not bad, bad
    if tag in R.WEIGHTED:
        assert np.abs(g.raw('gweights12_' + tag)).max() > 0 and np.abs(g.raw('gweights21_' + tag)).max() > 0
    # the total, recomputed from the returned terms in float64 (the occlusion penalty is not returned: from the restatement)
    cfg = R.case_cfg(tag)
    total = got['warp'] + got['smooth'] - got['entropy'] + got['oof']
    if cfg.w_occ > 0:
        occ = float(R.loss(cfg, _case(g, tag))['occ'])
        assert occ > 0
        total = total + occ
    assert abs(total - got['total']) <= 5e-8 + 3e-6 * abs(total)


def test_draws_on_the_device_and_both_modes_reproduce(golden):
    """eps=None, comp=None: two calls differ; with the stored noise and draws, two calls agree bit for bit, loss and gradients,
    in deterministic mode; the samples, the entropy term and the entropy term's gradients (all that the mixture kernels alone
    decide: the family has no atomics) agree bit for bit with the mode off as well, and between the modes."""
    from arflow_amd import functional as AF
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.uflow_elbo_loss import UFlowElboLoss
    g = golden('elbo_mixture')
    tag = 'mix2_tie'
    cu = lambda name: torch.from_numpy(np.array(g.raw(name))).cuda()  # noqa: E731
    loss = UFlowElboLoss(AttrDict(R.case_cfg(tag)))
    nets = {'flows_fw': [None, None, cu('net12_' + tag)], 'flows_bw': [None, None, cu('net21_' + tag)]}
    a, b = loss(nets, cu('im1'), cu('im2')), loss(nets, cu('im1'), cu('im2'))
    assert a[5].shape == (4, 2, 8, 16) and bool(torch.isfinite(a[0])) and bool(torch.isfinite(b[0])) and not torch.equal(a[5], b[5])
    with AF.deterministic():
        one, two = _run(g, tag), _run(g, tag)
    for key in R.OUTPUTS:
        assert np.array_equal(one[key], two[key]), key
    # the entropy term and its gradients pass through the mixture node alone: the same bits in either mode
    with AF.deterministic():
        on = _run(g, tag, of=3)
    with AF.deterministic(False):
        three, four = _run(g, tag, of=3), _run(g, tag, of=3)
    assert np.abs(on['gnet12']).max() > 0 and np.abs(on['gnet21']).max() > 0
    for key in ('entropy', 'flow12_2', 'gnet12', 'gnet21'):
        assert np.array_equal(three[key], four[key]) and np.array_equal(on[key], three[key]), key


def test_component_net_against_the_reference(golden):
    import arflow_amd.models as M
    from tests import prob_ref as P
    from tests.helpers import epe
    g = golden('elbo_mixture')
    img1, img2, insum = P.make_input()
    assert insum == float(g['insum'])
    model = R.prepare_component(M.get_model(R.model_cfg())).cuda()
    with torch.no_grad():
        res = model(img1.cuda(), img2.cuda(), with_bk=True)
    assert sorted(res) == ['flows_bw', 'flows_fw'] and len(res['flows_fw']) == 6 and len(res['flows_bw']) == 6
    assert all(f.shape[1] == 8 for f in res['flows_fw'] + res['flows_bw'])
    got = R.collect_component(res)
    assert len(got) == 6
    for name, arr in got.items():
        ref = torch.as_tensor(np.asarray(g[name]))
        arr = torch.from_numpy(arr)
        assert arr.shape == ref.shape, name
        for c in range(0, arr.shape[1], 2):
            e = epe(arr[:, c:c + 2], ref[:, c:c + 2])
            print('%s channels %d:%d EPE %.3e' % (name, c, c + 2, e))
            assert e <= 1e-3, '%s stored channels %d:%d: EPE %.3e vs the reference' % (name, c, c + 2, e)
    f2 = res['flows_fw'][2]
    assert float((f2[:, 0:2] - f2[:, 2:4]).abs().max()) > 1e-3  # two components, not one twice


def test_one_training_step_of_the_mixture_workload():
    """TrainStep('componentnet+uflow_elbo_mixture') at batch 1, 64 x 128: finite loss, every parameter of both sub-models
    receives a finite gradient, and the mean and the log-std channels of both last refinement convolutions a non-zero one.
    (64 x 128 is the size of the low-rank workload's step test and the smallest the model takes: at 64 x 64 the top pyramid
    level is 2 x 2 and PWCProbFlow refuses it with the reference's 'Max displacement of 4 is too large'.)"""
    from arflow_amd.train_step import TrainStep, synthetic_pairs
    dev = torch.device('cuda')
    step = TrainStep('componentnet+uflow_elbo_mixture', dev, seed=1234)
    x = synthetic_pairs(1, 64, 128, device=dev, seed=5)
    loss = step(x)
    assert bool(torch.isfinite(loss)), float(loss)
    names = [n for n, _ in step.model.named_parameters()]
    assert any(n.startswith('pwcnet1.') for n in names) and any(n.startswith('pwcnet2.') for n in names)
    for n, p in step.model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    for sub in (step.model.pwcnet1, step.model.pwcnet2):
        last = sub._refine_model[12]
        assert last.out_channels == 4
        assert float(last.weight.grad[0:2].abs().max()) > 0 and float(last.weight.grad[2:4].abs().max()) > 0
