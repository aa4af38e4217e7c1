"""GPU: the fused optimiser step (csrc/optim.hip; arflow_amd.optim.FlatOptimizer, TrainStep(train_cfg=...)) per element against
the float64 restatement of tests/optim_ref.py.  DESIGN.md section 37.

The bound of every parameter and state element after every step is derived by tests/optim_ref.py from the inputs alone (each fp32
operation of the kernel carried as value and absolute error bound, u = 2^-24); tests/test_optim_cpu.py holds the restatement to
torch's optimisers and the reference's AdamW (tests/golden/optim.npz) and shows that a wrong reading of a rule moves an element
by >= 10 bounds.  Each test prints its largest error / bound ratio.
Shapes: the fixture's 1-D tensors of 1, 2, 3, 5, 16, CHUNK - 1, CHUNK + 1 and 2 CHUNK + 3 elements (8222 in all: 11 table rows,
3 norm partials).  The reducer lays them out in reverse, so the longest sits at flat offset 0 (float4 rows and a 3-element scalar
row) and every tensor behind it starts off the 16-byte grid (scalar rows); `shifted` moves every parameter one float off 16
bytes as well."""
import copy

import numpy as np
import pytest
import torch

from arflow_amd import functional as AF
from arflow_amd import optim as OPT
from arflow_amd.config import AttrDict
from arflow_amd.ddp import FlatGradAllReduce
from tests import optim_ref as R

pytestmark = pytest.mark.gpu
_cache = {}

# the `train` section of configs/chairs_uflow_elbo.json
CHAIRS_TRAIN = dict(batch_size=4, valid_batch_size=4, beta=0.999, bias_decay=0, epoch_num=1000, epoch_size=1000, lr=0.0001,
                    lr_decay_start_epoch=800, lr_decay_factor=0.98, beta1=0.9, beta2=0.999, eps=1e-08, momentum=0.9, n_gpu=1,
                    optim='adam', pretrained_model=None, print_freq=10, record_freq=10, save_iter=0, valid_freq=10, valid_size=0,
                    weight_decay=1e-06, workers=4, sp_samples=100, clip=-1.0, track_auc=False)


def fixture(golden):
    """The fixture's inputs and the restatement's trajectory (values and bounds) of every case, computed once, left unchanged."""
    if not _cache:
        z = golden('optim')
        p0, g = z.raw('p0'), z.raw('g')
        assert tuple(z.raw('sizes')) == R.SIZES and tuple(z['names']) == R.NAMES
        _cache.update(p0=p0, g=g, traj={})
    return _cache


def reference(golden, case):
    f = fixture(golden)
    if case not in f['traj']:
        f['traj'][case] = R.trajectory(R.case_cfg(case, f['g']), f['p0'], f['g'])
    return f['traj'][case]


class Holder(torch.nn.Linear):
    """One 1-D fixture tensor as `weight` (a Linear's: decayed) or `bias`."""

    def __init__(self, kind, value):
        torch.nn.Module.__init__(self)
        self.in_features = self.out_features = 0
        self.register_parameter('weight', torch.nn.Parameter(value) if kind == 'weight' else None)
        self.register_parameter('bias', torch.nn.Parameter(value) if kind == 'bias' else None)


def off_grid(value):
    """The same values in storage that starts one float behind a 16-byte boundary."""
    buf = torch.empty(value.numel() + 8, device=value.device, dtype=value.dtype)
    start = (1 - buf.data_ptr() // 4) % 4
    out = buf[start:start + value.numel()]
    out.copy_(value)
    assert out.data_ptr() % 16 == 4
    return out


def build(p0, shifted=False):
    """-> (module, reducer): the fixture's tensors as t0.weight, t1.bias, ... on the GPU."""
    model, off = torch.nn.Module(), 0
    for name, n in zip(R.NAMES, R.SIZES):
        mod, kind = name.split('.')
        value = torch.from_numpy(p0[off:off + n].copy()).cuda()
        model.add_module(mod, Holder(kind, off_grid(value) if shifted else value))
        off += n
    assert [n for n, _ in model.named_parameters()] == list(R.NAMES)
    return model, FlatGradAllReduce(model)


def load_gradient(model, reducer, g):
    reducer.zero_grad()
    off = 0
    for p in model.parameters():
        p.grad.copy_(torch.from_numpy(g[off:off + p.numel()].copy()))
        off += p.numel()
    assert off == reducer.flat.numel()


def in_name_order(model, reducer, flat):
    """A flat buffer of the reducer's layout -> the order of R.NAMES."""
    where = {id(p): (o, n) for p, o, n in reducer._spans}
    return torch.cat([flat[where[id(p)][0]:where[id(p)][0] + where[id(p)][1]] for p in model.parameters()])


def snapshot(model, reducer, opt):
    p = torch.cat([q.detach().reshape(-1) for q in model.parameters()]).clone()
    m = in_name_order(model, reducer, opt.exp_avg).clone()
    v = None if opt.exp_avg_sq is None else in_name_order(model, reducer, opt.exp_avg_sq).clone()
    return p, m, v


def run(cfg, p0, g, shifted=False, steps=R.STEPS):
    model, reducer = build(p0, shifted)
    opt = OPT.FlatOptimizer(reducer, AttrDict(cfg))
    out = []
    for t in range(steps):
        load_gradient(model, reducer, g[t])
        opt.step()
        out.append(snapshot(model, reducer, opt))
    return out, (model, reducer, opt)


def excess(name, got, ref):
    """The number of elements of `got` outside ref.v +- ref.e; prints the largest error / bound."""
    want, bound = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (ref.v, ref.e))
    err = np.abs(got.double().cpu().numpy() - want)
    ratio = float((err / bound.clip(1e-300)).max()) if err.max() > 0 else 0.0
    print('%s: max err %.3e, max bound %.3e, max err / bound %.3f' % (name, err.max(), bound.max(), ratio))
    return int((~(err <= bound)).sum())


def check_trajectory(name, got, ref):
    for t, ((p, m, v), (rp, rm, rv)) in enumerate(zip(got, ref)):
        assert excess('%s step %d p' % (name, t + 1), p, rp) == 0
        assert excess('%s step %d m' % (name, t + 1), m, rm) == 0
        assert (v is None) == (rv is None)
        if v is not None:
            assert excess('%s step %d v' % (name, t + 1), v, rv) == 0


@pytest.mark.parametrize('shifted', [False, True], ids=['aligned', 'shifted'])
@pytest.mark.parametrize('case', R.CASES)
def test_three_steps_within_the_derived_bounds(golden, case, shifted):
    """Every case of the fixture (four rules x clip active, slack, off): parameters and state after each of three steps; then
    the same with every parameter's storage one float off 16-byte alignment (no float4 row left)."""
    f = fixture(golden)
    got, (model, reducer, opt) = run(R.case_cfg(case, f['g']), f['p0'], f['g'], shifted)
    check_trajectory('%s %s' % (case, 'shifted' if shifted else 'aligned'), got, reference(golden, case))
    assert all((p.data_ptr() % 16 == 4) == shifted for p in model.parameters())
    # the clip scales the gradient as it is read: the stored gradient is the unclipped one
    assert np.array_equal(in_name_order(model, reducer, reducer.flat).cpu().numpy(), f['g'][-1])
    assert opt.t == R.STEPS and int(opt._table.shape[0]) == 11


def test_norm_launch_only_where_it_is_needed(golden):
    f = fixture(golden)

    def launches(case, **extra):
        model, reducer = build(f['p0'])
        opt = OPT.FlatOptimizer(reducer, AttrDict(dict(R.case_cfg(case, f['g']), **extra)))
        load_gradient(model, reducer, f['g'][0])
        AF.start_kernel_timing()
        opt.step()
        return [name for name, _ in AF.stop_kernel_timing()]
    assert sorted(launches('adam_on')) == ['arflow_optim_gradnorm', 'arflow_optim_step']
    assert sorted(launches('sgd_slack')) == ['arflow_optim_gradnorm', 'arflow_optim_step']
    assert launches('adam_off') == ['arflow_optim_step'] and launches('adamw_off') == ['arflow_optim_step']
    assert sorted(launches('adam_off', skip_nonfinite=True)) == ['arflow_optim_gradnorm', 'arflow_optim_step']


@pytest.mark.parametrize('case', ['adam_on', 'adamw_on', 'sgd_on'])
def test_two_runs_give_the_same_bits(golden, case):
    f = fixture(golden)
    cfg = R.case_cfg(case, f['g'])
    first, _ = run(cfg, f['p0'], f['g'])
    again, _ = run(cfg, f['p0'], f['g'])
    with AF.deterministic():
        det, _ = run(cfg, f['p0'], f['g'])
    for a, b, c in zip(first, again, det):
        for x, y, z in zip(a, b, c):
            assert x is None or (torch.equal(x, y) and torch.equal(x, z))


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_nonfinite_guard_skips_the_step(golden, bad):
    """One good step, then a gradient with one non-finite element: parameters and state keep their bits and the device counter
    is 1; a good step after it is taken.  Without the guard the same gradient reaches the parameters."""
    f = fixture(golden)
    cfg = dict(R.case_cfg('adam_off', f['g']), skip_nonfinite=True)
    got, (model, reducer, opt) = run(cfg, f['p0'], f['g'], steps=1)
    assert excess('guarded good step p', got[0][0], reference(golden, 'adam_off')[0][0]) == 0 and opt.skipped_steps() == 0
    poisoned = f['g'][1].copy()
    poisoned[R.N - 7] = bad
    load_gradient(model, reducer, poisoned)
    opt.step()
    after = snapshot(model, reducer, opt)
    assert all(torch.equal(a, b) for a, b in zip(after, got[0]))
    assert opt.skipped_steps() == 1
    load_gradient(model, reducer, f['g'][1])
    opt.step()
    moved = snapshot(model, reducer, opt)
    assert opt.skipped_steps() == 1 and not torch.equal(moved[0], after[0]) and bool(torch.isfinite(moved[0]).all())
    _, (model2, reducer2, opt2) = run(dict(cfg, skip_nonfinite=False), f['p0'], f['g'], steps=1)
    load_gradient(model2, reducer2, poisoned)
    opt2.step()
    assert not bool(torch.isfinite(snapshot(model2, reducer2, opt2)[0]).all()) and opt2.skipped_steps() == 0


def test_moved_parameter_storage_is_followed(golden):
    """After p.data = p.data.clone() the next step updates the NEW storage (the table is rebuilt on the host) and leaves the
    old one alone; the trajectory stays within the bounds."""
    f = fixture(golden)
    got, (model, reducer, opt) = run(R.case_cfg('adam_off', f['g']), f['p0'], f['g'], steps=1)
    old = [p.data for p in model.parameters()]
    kept = [t.clone() for t in old]
    for p in model.parameters():
        p.data = p.data.clone()
    assert all(p.data_ptr() != t.data_ptr() for p, t in zip(model.parameters(), old))
    load_gradient(model, reducer, f['g'][1])
    opt.step()
    ref = reference(golden, 'adam_off')[1]
    assert excess('moved storage p', snapshot(model, reducer, opt)[0], ref[0]) == 0
    assert all(torch.equal(a, b) for a, b in zip(old, kept))


@pytest.mark.parametrize('case', ['adam_on', 'sgd_off'])
def test_state_round_trip_continues_the_trajectory(golden, case):
    f = fixture(golden)
    cfg = R.case_cfg(case, f['g'])
    got, (model, reducer, opt) = run(cfg, f['p0'], f['g'], steps=2)
    state = copy.deepcopy(opt.state_dict())
    assert state['step'] == 2 and state['lr'] == cfg['lr'] and state['optim'] == cfg['optim']
    model2, reducer2 = build(got[1][0].cpu().numpy())
    opt2 = OPT.FlatOptimizer(reducer2, AttrDict(cfg))
    opt2.load_state_dict(state)
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and opt2.t == 2
    for o, m, r in ((opt, model, reducer), (opt2, model2, reducer2)):
        load_gradient(m, r, f['g'][2])
        o.step()
    a, b = snapshot(model, reducer, opt), snapshot(model2, reducer2, opt2)
    assert all(x is None or torch.equal(x, y) for x, y in zip(a, b))
    check_trajectory(case + ' restored', [b], [reference(golden, case)[2]])
    with pytest.raises(ValueError, match='optim'):
        OPT.FlatOptimizer(reducer2, AttrDict(R.RULE_CFG['adamw'])).load_state_dict(state)


def test_epoch_end_follows_the_schedule(golden):
    s = R.SCHEDULE
    model, reducer = build(fixture(golden)['p0'])
    opt = OPT.FlatOptimizer(reducer, AttrDict(dict(R.RULE_CFG['adam'], **{k: s[k] for k in ('lr', 'lr_decay_factor', 'lr_decay_start_epoch')})))
    got = [opt.epoch_end(i) for i in s['epochs']]
    assert np.abs(np.asarray(got) - golden('optim').raw('lr_schedule')).max() <= 1e-12 * s['lr'] and opt.lr == got[-1]


def real_step(seed):
    from arflow_amd.train_step import TrainStep
    dev = torch.device('cuda')
    step = TrainStep('pwclite_uflow+uflow_loss', dev, seed=seed, train_cfg=AttrDict(CHAIRS_TRAIN))
    assert type(step.opt) is OPT.FlatOptimizer
    return step


def test_real_model_step_agrees_with_torch_adam():
    """TrainStep('pwclite_uflow+uflow_loss', train_cfg = the train section of chairs_uflow_elbo.json) at 2 x 64 x 96: one backward
    pass, then FlatOptimizer.step() against (a) the float64 restatement within its bounds and (b) torch.optim.Adam with the same
    two groups on a deep copy fed the cloned gradients.  torch's fp32 chain (lerp, addcmul, sqrt, div, add, addcdiv) has no more
    roundings than the kernel's, so it lies within the same bound of the float64 value: the two agree within twice the bound."""
    from arflow_amd.train_step import synthetic_pairs
    step = real_step(3)
    twin = copy.deepcopy(step.model)
    x = synthetic_pairs(2, 64, 96, device=torch.device('cuda'), seed=5)
    res = step.model(x, with_bk=True)
    out = step.loss([torch.cat([fw, bw], 1) for fw, bw in zip(res['flows_fw'], res['flows_bw'])], x)
    step.reducer.zero_grad()
    out[0].backward()
    step.reducer.finish()
    names = [n for n, _ in step.model.named_parameters()]
    before = {n: p.detach().clone() for n, p in step.model.named_parameters()}
    grads = {n: p.grad.detach().clone() for n, p in step.model.named_parameters()}
    assert sum(float(g.abs().sum()) > 0 for g in grads.values()) > len(names) // 2
    for n, p in twin.named_parameters():
        p.grad = grads[n].clone()
    groups = OPT.decay_groups(twin, CHAIRS_TRAIN['weight_decay'], CHAIRS_TRAIN['bias_decay'])
    ref_opt = torch.optim.Adam([dict(params=g['params'], weight_decay=g['weight_decay']) for g in groups], CHAIRS_TRAIN['lr'],
                               betas=(CHAIRS_TRAIN['beta1'], CHAIRS_TRAIN['beta2']), eps=CHAIRS_TRAIN['eps'])
    ref_opt.step()
    step.opt.step()
    sizes = [before[n].numel() for n in names]
    p0 = torch.cat([before[n].reshape(-1) for n in names])       # the restatement in float64 on the device: 7.2 M elements
    g = torch.cat([grads[n].reshape(-1) for n in names])
    cfg = dict(CHAIRS_TRAIN)
    decay_of = {n: grp['weight_decay'] for grp in OPT.decay_groups(step.model, cfg['weight_decay'], cfg['bias_decay']) for n in grp['names']}
    wd = torch.cat([torch.full((k,), decay_of[n], dtype=torch.float64) for n, k in zip(names, sizes)]).cuda()
    zero = R.V(torch.zeros_like(p0))
    rp, rm, rv = R.step(cfg, 1, R.V(p0), g, zero, zero, wd, R.V(1.0))
    got = torch.cat([p.detach().reshape(-1) for p in step.model.parameters()])
    twin_p = torch.cat([p.detach().reshape(-1) for p in twin.parameters()])
    assert excess('real model p vs float64', got, rp) == 0
    assert excess('real model m vs float64', in_name_order(step.model, step.reducer, step.opt.exp_avg), rm) == 0
    assert excess('real model v vs float64', in_name_order(step.model, step.reducer, step.opt.exp_avg_sq), rv) == 0
    assert excess('real model p vs torch.optim.Adam', got, R.V(twin_p, 2.0 * rp.e)) == 0
    assert float((got - p0).abs().max()) > 0.5 * CHAIRS_TRAIN['lr']
    # bias elements carry no decay, weights do: the groups reached the table
    tab = step.opt._table.cpu().numpy()
    assert set(np.unique(tab[:, 3].view(np.float64))) == {0.0, 1e-6}


def test_checkpoint_round_trip(tmp_path):
    """save / restore: {'epoch', 'state_dict', 'optimizer'}; the first two in the reference's layout (its load_checkpoint pops
    'epoch' and takes 'state_dict'), so the file's state_dict loads into a fresh model."""
    from arflow_amd.models import get_model
    step = real_step(3)
    g = torch.Generator(device='cpu').manual_seed(1)
    for _ in range(2):
        step.reducer.zero_grad()
        step.reducer.flat.copy_(1e-3 * torch.randn(step.reducer.flat.numel(), generator=g))
        step.opt.step()
    step.opt.epoch_end(900)
    path = str(tmp_path / 'model_ckpt.pth.tar')
    step.save(path, 17)
    other = real_step(4)
    ptrs = [p.data_ptr() for p in other.model.parameters()]
    assert not torch.equal(next(other.model.parameters()), next(step.model.parameters()))
    assert other.restore(path) == 17
    assert ptrs == [p.data_ptr() for p in other.model.parameters()]
    for a, b in zip(step.model.state_dict().values(), other.model.state_dict().values()):
        assert torch.equal(a, b)
    assert other.opt.t == 2 and other.opt.lr == step.opt.lr == CHAIRS_TRAIN['lr'] * CHAIRS_TRAIN['lr_decay_factor']
    assert torch.equal(other.opt.exp_avg, step.opt.exp_avg) and torch.equal(other.opt.exp_avg_sq, step.opt.exp_avg_sq)
    weights = torch.load(path, map_location='cpu')
    assert sorted(weights) == ['epoch', 'optimizer', 'state_dict'] and weights.pop('epoch') == 17
    fresh = get_model(step.model_cfg)
    fresh.load_state_dict(weights['state_dict'])
    for (k, a), b in zip(fresh.state_dict().items(), other.model.state_dict().values()):
        assert torch.equal(a, b.cpu()), k
    # both continue identically
    for s in (step, other):
        s.reducer.zero_grad()
        s.reducer.flat.fill_(1e-3)
        s.opt.step()
    assert all(torch.equal(a, b) for a, b in zip(step.model.parameters(), other.model.parameters()))
