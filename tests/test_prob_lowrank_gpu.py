"""GPU: PWCProbFlow without log-diagonal channels (out_channels [2, 0, N], the low-rank family's model) on the fused and on
the composed path against the reference's outputs (tests/golden/elbo_lowrank.npz), under the gate tests/test_prob_model_gpu.py
applies to its cases A-E (EPE <= 1e-3 on every stored channel pair), and one training step of the new workload."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lowrank_ref as R
from tests import prob_ref as P
from tests.helpers import epe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compare(g, tag, res, gate=1e-3):
    assert len(res['flows_fw']) == 6 and len(res['flows_bw']) == 6
    nall = sum(R.MODEL_CASES[tag])
    for k in ('flows_fw', 'flows_bw'):
        for lvl, f in enumerate(res[k]):
            assert f.shape[1] == (nall if lvl <= 2 else 2), (tag, k, lvl, f.shape)
    got = R.collect(res, tag)
    assert got, tag
    for name, arr in got.items():
        ref = torch.as_tensor(np.asarray(g[name]))
        arr = torch.from_numpy(arr)
        assert arr.shape == ref.shape, name
        for c in range(0, arr.shape[1], 2):
            e = epe(arr[:, c:c + 2], ref[:, c:c + 2])
            print('%s channels %d:%d EPE %.3e' % (name, c, c + 2, e))
            assert e <= gate, '%s stored channels %d:%d: EPE %.3e vs the reference' % (name, c, c + 2, e)


@pytest.fixture(scope='module')
def inputs(golden):
    g = golden('elbo_lowrank')
    img1, img2, insum = P.make_input()
    assert insum == float(g['insum'])
    return g, img1, img2


@pytest.mark.parametrize('tag', list(R.MODEL_CASES))
def test_goldens_on_the_fused_path(inputs, tag):
    """Every level runs the fused level without a rest member, the two final levels come from out_tail, and no kernel sees a
    zero-channel tensor."""
    import arflow_amd.functional as AF
    import arflow_amd.models as M
    g, img1, img2 = inputs
    model = R.prepare(M.get_model(R.model_cfg(tag))).cuda()
    calls = {'level': [], 'up': [], 'tail': []}
    old = (AF.level, AF.out_upsample, AF.out_tail)

    def level(x1, x2, flow, c, *members, **kw):
        assert all(m.shape[1] > 0 for m in members)
        calls['level'].append(list(c.layout))
        return old[0](x1, x2, flow, c, *members, **kw)

    def up(x, *a, **kw):
        calls['up'].append(tuple(x.shape))
        return old[1](x, *a, **kw)

    def tail(x, n_flow, n_diag, bias):
        calls['tail'].append((tuple(x.shape), n_flow, n_diag))
        return old[2](x, n_flow, n_diag, bias)
    AF.level, AF.out_upsample, AF.out_tail = level, up, tail
    try:
        with torch.no_grad():
            res = model(img1.cuda(), img2.cuda(), with_bk=True)
    finally:
        AF.level, AF.out_upsample, AF.out_tail = old
    assert calls['level'] == [[0, 'vol', 1]] + [[0, 'flow', 'vol', 1]] * 3 and calls['up'] == [], calls
    assert calls['tail'] == [((2, sum(R.MODEL_CASES[tag]), 48, 64), 2, 0)], calls
    compare(g, tag, res)


CHILD = """
import sys, torch
sys.path.insert(0, %r)
from tests import lowrank_ref as R, prob_ref as P
import arflow_amd.functional as AF
import arflow_amd.models as M
assert not AF.out_up_supported(torch.zeros(1, device='cuda'))
img1, img2, _ = P.make_input()
out = {}
for tag in R.MODEL_CASES:
    model = R.prepare(M.get_model(R.model_cfg(tag))).cuda()
    with torch.no_grad():
        res = model(img1.cuda(), img2.cuda(), with_bk=True)
    out[tag] = {k: [t.cpu() for t in v] for k, v in res.items()}
torch.save(out, sys.argv[1])
"""


def test_goldens_on_the_composed_path(inputs, tmp_path):
    """ARFLOW_OUT_UP=0 in a fresh child process (the switch is read at import): the composed ATen upsamples, both models."""
    g, _, _ = inputs
    path = str(tmp_path / 'off.pt')
    subprocess.run([sys.executable, '-c', CHILD % ROOT, path], check=True, env=dict(os.environ, ARFLOW_OUT_UP='0'), cwd=ROOT,
                   timeout=300)
    off = torch.load(path)
    for tag in R.MODEL_CASES:
        compare(g, tag, off[tag])


def test_one_training_step_of_the_lowrank_workload():
    """TrainStep('pwcprobflow+uflow_elbo_lowrank') at batch 1, 64 x 128: finite loss, finite gradients everywhere, and non-zero
    gradients for the column channels (2..32) of the level-1 head and of the last refinement conv."""
    from arflow_amd.train_step import TrainStep, synthetic_pairs
    dev = torch.device('cuda')
    step = TrainStep('pwcprobflow+uflow_elbo_lowrank', dev, seed=1234)
    x = synthetic_pairs(1, 64, 128, device=dev, seed=5)
    head, last = step.model._flow_layers[1][5], step.model._refine_model[12]
    assert head.out_channels == 32 and last.out_channels == 32
    loss = step(x)
    assert bool(torch.isfinite(loss)), float(loss)
    for n, p in step.model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    for conv in (head, last):
        assert float(conv.weight.grad[2:].abs().max()) > 0 and float(conv.bias.grad[2:].abs().max()) > 0
