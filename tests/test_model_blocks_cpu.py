"""CPU: the pieces the host models share (arflow_amd/models/blocks.py, uflow_model.py): the level-dropout draw, the
fw/bw pair pass over the extractor's batch, and the refinement walk."""
import pytest
import torch
import torch.nn as nn

from arflow_amd.models import blocks
from arflow_amd.models.uflow_model import refine


def test_level_drops_draws_pass_major_from_the_cpu_rng():
    torch.manual_seed(123)
    d = blocks.level_drops(True, 0.5, 5, 2, 3, torch.device('cpu'))
    torch.manual_seed(123)
    expect = torch.tensor([[float(torch.rand(1) > 0.5) for _ in range(5)] for _ in range(2)])  # [pass, level]
    assert d.dtype == torch.float32 and d.shape == (5, 6, 1, 1, 1)
    assert torch.equal(d, expect.t().repeat_interleave(3, dim=1).view(5, 6, 1, 1, 1))
    assert blocks.level_drops(False, 0.5, 5, 2, 3, torch.device('cpu')) is None
    assert blocks.level_drops(True, 0, 5, 2, 3, torch.device('cpu')) is None


B = 2


@pytest.fixture(scope='module')
def extractor_output():
    """A 2B pyramid of 3 levels and its moment rows, every sample's values distinct."""
    g = torch.Generator().manual_seed(7)
    pyr = [torch.randn(2 * B, 3, 4 << l, 5 << l, generator=g) + 10 * torch.arange(2 * B).view(-1, 1, 1, 1) for l in range(3)]
    moms = [torch.randn(2 * B, 2 + l, 2, generator=g, dtype=torch.float64) + 10 * torch.arange(2 * B).view(-1, 1, 1)
            for l in range(3)]
    return pyr, moms


def recording_run(seen):
    def run(pyr1, pyr2, n_passes, moments):
        seen.append((pyr1, pyr2, n_passes, moments))
        return [p + q for p, q in zip(pyr1, pyr2)]
    return run


def same(got, want):
    return len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))


def test_pair_pass_both_directions_is_one_2b_pass(extractor_output):
    pyr, moms = extractor_output
    seen = []
    res = blocks.pair_pass(pyr, moms, B, True, recording_run(seen))
    (pyr1, pyr2, n_passes, (rows1, rows2)), = seen
    assert n_passes == 2
    assert same(pyr1, pyr)
    assert same(pyr2, [torch.cat([p[B:], p[:B]], 0) for p in pyr])
    assert same(rows1, moms)
    assert same(rows2, [torch.cat([t[B:], t[:B]], 0) for t in moms])
    flows = [p + torch.cat([p[B:], p[:B]], 0) for p in pyr]
    assert list(res) == ['flows_fw', 'flows_bw']
    assert same(res['flows_fw'], [f[:B] for f in flows]) and same(res['flows_bw'], [f[B:] for f in flows])


def test_pair_pass_forward_only_takes_the_two_halves(extractor_output):
    pyr, moms = extractor_output
    seen = []
    res = blocks.pair_pass(pyr, moms, B, False, recording_run(seen))
    (pyr1, pyr2, n_passes, (rows1, rows2)), = seen
    assert n_passes == 1
    assert same(pyr1, [p[:B] for p in pyr]) and same(pyr2, [p[B:] for p in pyr])
    assert same(rows1, [t[:B] for t in moms]) and same(rows2, [t[B:] for t in moms])
    assert list(res) == ['flows_fw']
    assert same(res['flows_fw'], [p[:B] + p[B:] for p in pyr])


@pytest.mark.parametrize('with_bk', [True, False])
def test_pair_pass_hands_on_no_moments_unless_every_level_has_them(extractor_output, with_bk):
    pyr, moms = extractor_output
    for m in (None, [moms[0], None, moms[2]]):
        seen = []
        blocks.pair_pass(pyr, m, B, with_bk, recording_run(seen))
        assert seen[0][3] is None


def test_refine_equals_the_sequential_bit_for_bit(monkeypatch):
    monkeypatch.setattr(blocks, 'bias_act', lambda y, b, s: torch.nn.functional.leaky_relu(y + b.view(1, -1, 1, 1), s))
    torch.manual_seed(3)
    mods = nn.ModuleList([nn.Conv2d(4, 6, 3, padding='same', dilation=2), nn.LeakyReLU(0.1), nn.Conv2d(6, 2, 3, padding='same')])
    x = torch.randn(1, 4, 5, 7)
    with torch.no_grad():
        assert torch.equal(refine(mods, x), nn.Sequential(*mods)(x))
