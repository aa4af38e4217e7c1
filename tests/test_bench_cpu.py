"""bench.py helpers that do not need a GPU: the algorithmic-byte formulas and the lookup of
the PMC traffic table kept under profiles/."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_algorithmic_bytes_follow_the_survey_formulas():
    import bench
    B, C, H, W = 16, 32, 96, 160
    px = B * H * W
    assert bench.algorithmic_bytes('arflow_corr_fwd', (B, C, H, W, 4)) == 4 * px * (2 * C + 81)
    assert bench.algorithmic_bytes('arflow_corr_fwd', (B, C, H, W, 4, 3)) == 4 * px * (2 * C + 81 + 3)
    assert bench.algorithmic_bytes('arflow_corr_bwd', (B, C, H, W, 4, 0)) == 4 * px * (81 + 4 * C)
    assert bench.algorithmic_bytes('arflow_corr_bwd', (B, C, H, W, 4, 3)) == 4 * px * (81 + 3 + 4 * C)
    assert bench.algorithmic_bytes('arflow_warp_fwd', (B, C, H, W)) == 4 * px * (2 * C + 2)
    assert bench.algorithmic_bytes('arflow_warp_bwd', (B, C, H, W, True)) == 4 * px * (3 * C + 4)
    assert bench.algorithmic_bytes('arflow_warp_bwd', (8, 3, 384, 640, False)) == 4 * 8 * 384 * 640 * (2 * 3 + 4)
    assert bench.algorithmic_bytes('arflow_census_fwd', (8, 384, 640)) == 4 * 8 * 384 * 640 * 8
    assert bench.algorithmic_bytes('arflow_featnorm_fwd', (B, C * H * W)) == 16 * B * C * H * W
    assert bench.algorithmic_bytes('arflow_bias_act_bwd', (B, 128, H * W)) == 12 * B * 128 * H * W
    assert bench.algorithmic_bytes('no_such_entry', (1,)) == 0


def test_pmc_traffic_table_covers_the_benchmark_shapes():
    import bench
    path = os.path.join(ROOT, 'profiles', 'r01_pmc_traffic.json')
    table = json.load(open(path))
    assert all(set(v) >= {'fetch_kb', 'write_kb', 'hbm_bytes'} for v in table.values())
    shapes = [('arflow_census_bwd', (8, 384, 640)), ('arflow_census_fwd', (8, 384, 640)),
              ('arflow_corr_fwd', (16, 32, 96, 160, 4, 3)), ('arflow_corr_bwd', (16, 32, 96, 160, 4, 3)),
              ('arflow_warp_fwd', (16, 32, 96, 160)), ('arflow_warp_bwd', (16, 32, 96, 160, True)),
              ('arflow_warp_fwd', (8, 3, 384, 640)), ('arflow_warp_bwd', (8, 3, 384, 640, False)),
              ('arflow_featnorm_fwd', (16, 491520)), ('arflow_featnorm_bwd', (16, 491520))]
    for name, shape in shapes:
        t, src = bench.pmc_traffic(name, shape)
        a = bench.algorithmic_bytes(name, shape)
        assert t is not None and src['file'].startswith('profiles/'), (name, shape)
        assert 0.9 * a <= t <= 2.5 * a, (name, shape, t, a)  # measured HBM traffic within 2.5x of the compulsory bytes
    assert bench.pmc_traffic('arflow_corr_fwd', (1, 5, 9, 11, 4, 0)) == (None, None)  # not a profiled shape


def test_assert_close_rejects_nan():
    """A kernel returning NaN/Inf must fail every parity test: `err > tol` is False for NaN."""
    import pytest
    import torch
    from tests.conftest import assert_close
    ref = torch.ones(4, 5)
    assert_close(ref.clone(), ref, 1e-6, 1e-6)
    for poison in (float('nan'), float('inf'), -float('inf')):
        bad = ref.clone()
        bad[2, 3] = poison
        with pytest.raises(AssertionError):
            assert_close(bad, ref, 1e-6, 1e-6, 'poisoned')
    with pytest.raises(AssertionError):
        assert_close(ref + 1e-3, ref, 1e-6, 1e-6)


def test_valu_slot_model_against_issued_instructions():
    """the hand-counted 'algorithmic v_fma slots' of bench.valu_slots() for the VALU-bound kernels must stay
    below what the kernels actually ISSUE (SQ_INSTS_VALU x 64 lanes, PMC pass profiles/r02_pmc_valu.json) and within a
    stated factor of it: an op-count model that exceeded the issued instructions, or fell under a third of them, would
    make the VALU roofline fraction meaningless."""
    import json
    import os
    import bench
    table = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r02_pmc_valu.json')))
    cases = [('arflow_census_warp_fwd', (8, 384, 640)), ('arflow_census_warp_bwd', (8, 384, 640)),
             ('arflow_census_fwd', (8, 384, 640)), ('arflow_census_bwd', (8, 384, 640)),
             ('arflow_photo_fwd', (8, 3, 384, 640)), ('arflow_photo_bwd', (8, 3, 384, 640))]
    checked = 0
    for name, shape in cases:
        keys = [k for k in bench.kernel_keys(name, shape) if k in table and 'SQ_INSTS_VALU' in table[k]]
        if not keys:
            continue
        issued = sum(table[k]['SQ_INSTS_VALU'] for k in keys) * 64.0
        # transcendentals count TRANS_SLOTS slots but are ONE issued instruction: compare the plain-instruction count
        plain = bench.valu_slots(name, shape, trans_slots=1.0)
        ratio = plain / issued
        assert 0.33 <= ratio <= 1.25, '%s: modelled %.3g slots vs %.3g issued lane-instructions (ratio %.2f)' % (name, plain, issued, ratio)
        checked += 1
    assert checked >= 4


def test_dump_outputs_names_dtype_budget_and_sample(tmp_path):
    """bench.py --dump-outputs: every array of the last step lands as float32 <name>.npy, small arrays whole, the total
    under 64 MB, and a cut array is the same fixed sample of its elements every time (runs stay comparable)."""
    import types
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    step = types.SimpleNamespace(last=torch.tensor(1.5), reducer=types.SimpleNamespace(flat=torch.randn(17 * 2 ** 20, generator=g)))
    flows = [torch.randn(2, 2, 8 // s, 12 // s, generator=g) for s in (1, 2)]
    res = {'flows_fw': flows, 'flows_bw': [[f + 1 for f in flows], [f + 2 for f in flows]]}
    dirs = [str(tmp_path / n) for n in ('a', 'b')]
    for d in dirs:
        bench.dump_outputs(d, step, res)
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(['loss.npy', 'grads.npy', 'flows_fw_0.npy', 'flows_fw_1.npy', 'flows_bw_0_0.npy',
                            'flows_bw_0_1.npy', 'flows_bw_1_0.npy', 'flows_bw_1_1.npy'])
    total = sum(os.path.getsize(os.path.join(dirs[0], n)) for n in names)
    assert total <= 64 * 2 ** 20
    a = {n[:-4]: np.load(os.path.join(dirs[0], n)) for n in names}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a['loss'].tolist() == [1.5]
    assert np.array_equal(a['flows_fw_1'], flows[1].numpy()) and np.array_equal(a['flows_bw_1_0'], flows[0].numpy() + 2)
    flat = step.reducer.flat.numpy()
    keep = a['grads'].size
    assert 0 < keep < flat.size  # the one array over its share: a sample, by the rule bench.dump_outputs() states
    assert np.array_equal(a['grads'], flat[np.sort(np.random.default_rng(0).choice(flat.size, keep, replace=False))])
    for n in a:
        assert np.array_equal(a[n], np.load(os.path.join(dirs[1], n + '.npy'))), n


def test_checkpoint_restore_repeats_the_first_step():
    """bench.Checkpoint: after restore(), a training step computes exactly what the first step of a freshly built model and
    optimizer computes -- seeded weights, zero Adam moments, step count 0 -- however many steps ran before."""
    import types
    import torch
    import bench

    def build():
        torch.manual_seed(0)
        model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
        return types.SimpleNamespace(model=model, opt=torch.optim.Adam(model.parameters(), lr=1e-2))

    x = torch.randn(8, 6, generator=torch.Generator().manual_seed(1))

    def train(s):
        s.opt.zero_grad()
        s.model(x).square().mean().backward()
        s.opt.step()
        return [p.detach().clone() for p in s.model.parameters()]

    fresh = train(build())
    s = build()
    start = bench.Checkpoint(s)
    start.restore()  # before the first step: no optimizer state yet
    assert all(torch.equal(a, b) for a, b in zip(train(s), fresh))
    for _ in range(3):
        train(s)
    start.restore()
    assert all(torch.equal(p, w) for p, w in zip(s.model.parameters(), start.weights))
    assert all(int(s.opt.state[p]['step']) == 0 for p in s.model.parameters())
    assert all(torch.equal(a, b) for a, b in zip(train(s), fresh))
