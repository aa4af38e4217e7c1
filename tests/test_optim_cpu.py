"""CPU: the float64 restatement of tests/optim_ref.py against tests/golden/optim.npz (torch.optim.Adam / SGD, the reference's own
AdamW and clip_grad_norm_, recorded by tools/make_optim_golden.py), the decay groups against the reference's name lists, the
chunk table, the host-only entry points and their error codes, and the discriminating power of the derived bounds.  DESIGN.md
section 37.  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from arflow_amd import _lib
from arflow_amd import optim as OPT
from arflow_amd.config import AttrDict
from tests import optim_ref as R

_cache = {}


def fixture(golden):
    """The fixture's arrays and the restatement's trajectory of every case, computed once and left unchanged."""
    if not _cache:
        z = golden('optim')
        p0, g = z.raw('p0'), z.raw('g')
        _cache.update(z=z, p0=p0, g=g, idx=z.raw('idx'),
                      traj={case: R.trajectory(R.case_cfg(case, g), p0, g) for case in R.CASES})
    return _cache


def test_inputs_are_the_seeded_ones(golden):
    f = fixture(golden)
    p0, g = R.make_inputs()
    assert np.array_equal(f['p0'], p0) and np.array_equal(f['g'], g)
    assert tuple(f['z'].raw('sizes')) == R.SIZES and tuple(f['z']['names']) == R.NAMES
    clips = R.clip_values(g)
    assert float(f['z'].raw('clip_on')) == clips['on'] and float(f['z'].raw('clip_slack')) == clips['slack']
    norms = np.sqrt((g.astype(np.float64) ** 2).sum(1))
    assert (norms > clips['on']).all() and (norms < clips['slack']).all()
    assert ((np.sign(g[0]) * np.sign(g[1])) < 0).sum() > R.N // 4     # signs flip between steps
    assert (g == 0).all(0).sum() > 50 and f['idx'].max() == R.N - 1


@pytest.mark.parametrize('case', R.CASES)
def test_restatement_matches_the_recorded_optimisers(golden, case):
    """Every recorded element of p, m (and v) after each of the three steps, to 1e-12 relative."""
    f = fixture(golden)
    for t, (p, m, v) in enumerate(f['traj'][case]):
        for key, got in (('p', p), ('m', m), ('v', v)):
            if got is None:
                assert 'v_' + case not in f['z']
                continue
            want = f['z'].raw('%s_%s' % (key, case))[t]
            err = np.abs(got.v[f['idx']] - want)
            assert (err <= 1e-12 * np.abs(want)).all(), (case, key, t, float((err / np.maximum(np.abs(want), 1e-300)).max()))


def test_schedule_matches_exponential_lr(golden):
    s = R.SCHEDULE
    want = fixture(golden)['z'].raw('lr_schedule')
    got = R.schedule(s['lr'], s['lr_decay_factor'], s['lr_decay_start_epoch'], s['epochs'])
    assert np.abs(got - want).max() <= 1e-12 * want.max()
    assert got[0] == got[1] == s['lr'] and got[2] < got[1]


def test_decay_groups_match_the_reference_for_every_workload(golden):
    from arflow_amd.models import get_model
    from arflow_amd.train_step import WORKLOADS
    z = fixture(golden)['z']
    for name, (mcfg, _) in WORKLOADS.items():
        model = get_model(AttrDict(mcfg))
        decay, no_decay = OPT.decay_groups(model, 1e-6, 0.0)
        assert decay['names'] == z['decay_' + name] and no_decay['names'] == z['no_decay_' + name], name
        assert decay['weight_decay'] == 1e-6 and no_decay['weight_decay'] == 0.0
        params = dict(model.named_parameters())
        assert all(params[n] is p for g in (decay, no_decay) for n, p in zip(g['names'], g['params']))
        assert len(decay['names']) + len(no_decay['names']) == len(params)


def test_decay_groups_sort_and_refuse_an_unclassified_parameter():
    class Odd(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.b = torch.nn.Conv2d(2, 2, 1)
            self.a = torch.nn.BatchNorm2d(2)
            self.gain = torch.nn.Parameter(torch.ones(1))
    with pytest.raises(AssertionError, match='were not separated into either decay/no_decay set'):
        OPT.decay_groups(Odd(), 1e-6, 0.0)
    m = Odd()
    del m.gain
    decay, no_decay = OPT.decay_groups(m, 1e-6, 0.0)
    assert decay['names'] == ['b.weight'] and no_decay['names'] == ['a.bias', 'a.weight', 'b.bias']


def test_chunk_table_covers_every_element_once():
    """The fixture's sizes, laid out as the reducer lays them (reverse order, packed): every flat element in exactly one row,
    no row across a span, the address moving with the offset, the group's decay in every row."""
    spans, off = [], 0
    for i, n in reversed(list(enumerate(R.SIZES))):
        spans.append((0x10000 * (i + 1), off, n, 1e-6 if i % 2 == 0 else 0.0))
        off += n
    tab = OPT.chunk_table(spans)
    assert tab.dtype == np.int64 and tab.shape[1] == OPT.ROW
    assert tab.shape[0] == sum((n + OPT.CHUNK - 1) // OPT.CHUNK for n in R.SIZES)
    seen = np.zeros(R.N, dtype=np.int64)
    for addr, o, cnt, bits in tab:
        assert 1 <= cnt <= OPT.CHUNK
        seen[o:o + cnt] += 1
        owner = [s for s in spans if s[1] <= o and o + cnt <= s[1] + s[2]]
        assert len(owner) == 1, 'a row crosses a span'
        assert addr == owner[0][0] + 4 * (o - owner[0][1])
        assert np.int64(bits).view(np.float64) == owner[0][3]
    assert (seen == 1).all()
    assert OPT.chunk_table([(4096, 0, OPT.CHUNK, 0.0)]).shape[0] == 1 and OPT.chunk_table([(4096, 0, OPT.CHUNK + 1, 0.0)]).shape[0] == 2


def test_partials_and_error_codes_need_no_gpu():
    lib = _lib.load()
    ENULL, ESHAPE, EPARAM = -1001, -1002, -1003
    assert lib.arflow_optim_partials(0) == ESHAPE and lib.arflow_optim_partials(-5) == ESHAPE
    assert [lib.arflow_optim_partials(n) for n in (1, 4096, 4097, R.N)] == [1, 1, 2, 3]
    assert lib.arflow_optim_partials(5909172) == 241 and lib.arflow_optim_partials(2 ** 33) == 256
    counts = [lib.arflow_optim_partials(n) for n in range(1, 3000000, 40961)]
    assert 1 <= min(counts) and max(counts) <= 256
    assert lib.arflow_optim_gradnorm(None, 16, 8, None) == ENULL and lib.arflow_optim_gradnorm(16, None, 8, None) == ENULL
    assert lib.arflow_optim_gradnorm(16, 16, 0, None) == ESHAPE and lib.arflow_optim_gradnorm(18, 16, 8, None) == EPARAM

    def call(table=64, nrows=1, grad=64, s1=64, s2=64, n=8, part=None, nparts=0, skipped=None, rule=0, first=0, lr=1e-4, bc1=0.1,
             sqbc2=0.03, eps=1e-8, b1=0.9, b2=0.999, clip=-1.0):
        return lib.arflow_optim_step(table, nrows, grad, s1, s2, n, part, nparts, skipped, rule, first, lr, bc1, sqbc2, eps, b1, b2,
                                     clip, None)
    for kw in (dict(table=None), dict(grad=None), dict(s1=None), dict(s2=None), dict(part=None, nparts=1)):
        assert call(**kw) == ENULL, kw
    for kw in (dict(nrows=0), dict(n=0), dict(part=64, nparts=2), dict(part=64, nparts=-1)):
        assert call(**kw) == ESHAPE, kw
    for kw in (dict(rule=3), dict(rule=-1), dict(first=2), dict(clip=1.0), dict(skipped=64), dict(lr=float('nan')), dict(clip=float('inf')),
               dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0), dict(bc1=0.0), dict(sqbc2=1.5), dict(grad=66), dict(s1=65), dict(table=68),
               dict(part=68, nparts=1, clip=1.0)):
        assert call(**kw) == EPARAM, kw
    assert call(rule=2, s2=None, grad=None) == ENULL     # sgd takes no second state buffer; the rest is still checked


def test_unknown_optim_raises_as_the_reference_does():
    with pytest.raises(NotImplementedError, match='rmsprop'):
        OPT.FlatOptimizer(None, AttrDict(optim='rmsprop', lr=1e-4))


def test_cpu_gradients_are_refused():
    from arflow_amd.ddp import FlatGradAllReduce
    reducer = FlatGradAllReduce(torch.nn.Linear(3, 2))
    with pytest.raises(_lib.ArflowHipError, match='GPU only'):
        OPT.FlatOptimizer(reducer, AttrDict(R.RULE_CFG['adam']))


def test_train_step_without_train_cfg_keeps_torch_adam():
    from arflow_amd.train_step import TrainStep
    step = TrainStep('pwclite_uflow+uflow_loss', torch.device('cpu'))
    assert type(step.opt) is torch.optim.Adam
    assert step.opt.defaults['lr'] == 1e-4 and step.opt.defaults['betas'] == (0.9, 0.999) and step.opt.defaults['weight_decay'] == 0


def moved(golden, mutate, cases):
    """max over the cases, steps, arrays and elements of |mutated - restated| / bound."""
    f = fixture(golden)
    worst = 0.0
    for case in cases:
        mut = R.trajectory(R.case_cfg(case, f['g']), f['p0'], f['g'], mutate=mutate)
        for (p, m, v), (pm, mm, vm) in zip(f['traj'][case], mut):
            for a, b in ((p, pm), (m, mm), (v, vm)):
                if a is not None:
                    assert np.isfinite(a.e).all()
                    worst = max(worst, float((np.abs(a.v - b.v) / a.e.clip(1e-300)).max()))
    return worst


@pytest.mark.parametrize('mutate,cases', [
    ('no_bc2', ('adam_off', 'adamw_off')), ('eps_in_sqrt', ('adam_off', 'adamw_off')),
    ('decay_bias', ('adam_off', 'adamw_off', 'sgd_off')), ('adamw_decay_lr', ('adamw_off',)),
    ('l2_after_moments', ('adam_off',)), ('coef_unclamped', ('adam_slack', 'adamw_slack', 'sgd_slack'))])
def test_bounds_tell_each_mutation_from_the_rule(golden, mutate, cases):
    """A wrong reading of a rule moves some element by at least 10 times its derived bound, in EVERY case it applies to."""
    assert mutate in R.MUTATIONS
    for case in cases:
        ratio = moved(golden, mutate, (case,))
        print('%s on %s: max move / bound %.3g' % (mutate, case, ratio))
        assert ratio >= 10.0, (mutate, case, ratio)


def test_bounds_stay_small(golden):
    """A sanity cap on the derived bounds themselves, not a tolerance of the kernel: they are those of a few dozen fp32 roundings,
    so after three steps no parameter's bound may exceed 1e-5 of max(|p|, lr) (the cap tests/augment_ref.py puts on its own bounds,
    here relative to the scale of a parameter and of one update) and every bound is finite.  What the bounds can tell apart is
    pinned by the mutation test above."""
    f = fixture(golden)
    for case in R.CASES:
        lr = R.case_cfg(case, f['g'])['lr']
        for p, m, v in f['traj'][case]:
            assert all(np.isfinite(a.e).all() for a in (p, m, v) if a is not None)
        p = f['traj'][case][-1][0]
        ratio = float((p.e / np.maximum(np.abs(p.v), lr)).max())
        print('%s: max bound / max(|p|, lr) %.3g' % (case, ratio))
        assert ratio <= 1e-5, (case, ratio)
