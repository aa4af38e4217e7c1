#!/usr/bin/env python3
"""Per-kernel microbenchmark on the BASELINE shapes: HIP-event time per launch, algorithmic GB/s and
fraction of the 8 TB/s HBM roofline.  Calls the C ABI directly (no autograd overhead).

    python tools/kbench.py [--iters 50] [--filter corr] [--levels uflow|pwclite]
    python tools/kbench.py --filter gauss_pyr      # the pyramid sampler node and an ElboLoss step
    python tools/kbench.py --filter mse            # one MseLoss step, fused against composed ATen ops
    python tools/kbench.py --filter augment        # the batch augmentation, fused against composed ATen ops
    python tools/kbench.py --filter optim          # the fused optimiser step against torch.optim.Adam(fused=True)
    python tools/kbench.py --filter ar             # the AR transform and loss, fused against composed ATen ops
    python tools/kbench.py --filter penalty_em     # one EM update of the penalty fit and log_gmm against their torch formulations
    python tools/kbench.py --filter render         # restore + stats + flow picture, fused against composed ATen ops
    python tools/kbench.py --filter elbo_penalty   # one UFlowElboLoss step with the fitted mixture penalties against the default step and the unfused composition
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# --tree DIR: import arflow_amd (and its built library) from another checkout of the project, for the legs of a bench that the
# other checkout can run too (--filter elbo_penalty: the default step); read here because it decides what the imports below find
TREE = os.path.abspath(sys.argv[sys.argv.index('--tree') + 1]) if '--tree' in sys.argv[1:-1] else None
if TREE:
    sys.path.insert(0, TREE)
import torch  # noqa: E402

from arflow_amd import _lib  # noqa: E402
from bench import algorithmic_bytes, HBM_PEAK_GBS  # noqa: E402


def p(t):
    return None if t is None else t.data_ptr()


EXACT_FILTERS = ('ar',)
MANIFEST = []  # (calls in the segment) per timed op, in launch order: tools/pmc_calls.py cuts the counter trace with it
_marker = None


def timeit(fn, iters):
    st = torch.cuda.current_stream()
    if _marker is not None:
        _marker(len(MANIFEST))  # one af_marker_kernel dispatch in front of every op's segment
    MANIFEST.append({'name': None, 'shape': None, 'calls': 5 + iters})
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def band_bench(dev, g, B=8, S=4, M=96, N=160, launches=30, repeats=5):
    """z = mean + L eps and its backward at B = 8, S = 4 on the 96 x 160 level, k = 0 and 3 -- the fused
    kernels (one launch each way, through the autograd node users call) next to the reference's formulation restated in
    torch ops (repeat the coefficients S times, (k+1)^2 x slice / mul / pad / add, and ATen's autograd of that), which is
    what a user has without the kernels.  HIP events around `launches` calls after 5 warm-ups, `repeats` times: median and
    the spread (min .. max) of the repeats; the raw launches through the C ABI are timed next to them.  Then one whole UFlowElboLoss forward + backward at 384 x 640, k = 3."""
    import statistics
    import torch.nn.functional as F
    from arflow_amd import functional as AF, triag_solve as T
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.uflow_elbo_loss import UFlowElboLoss

    def torch_formulation(mean, diag, off, eps, k):  # losses/uflow_elbo_loss.py:142-147 + utils/triag_solve.py:29-43
        A = torch.cat((diag, off), 1).repeat(S, 1, 1, 1)
        Y = torch.zeros_like(eps)
        for i in range(k + 1):
            for j in range(k + 1):
                ind = i * (k + 1) + j
                a = A[:, 2 * ind:2 * ind + 2]
                if i > 0 and j > 0:
                    Y = Y + F.pad(a[:, :, 0:-i, 0:-j] * eps[:, :, 0:-i, 0:-j], (j, 0, i, 0))
                elif i > 0:
                    Y = Y + F.pad(a[:, :, 0:-i, :] * eps[:, :, 0:-i, :], (0, 0, i, 0))
                elif j > 0:
                    Y = Y + F.pad(a[:, :, :, 0:-j] * eps[:, :, :, 0:-j], (j, 0, 0, 0))
                else:
                    Y = Y + a * eps
        return mean.repeat(S, 1, 1, 1) + Y

    def spread(fns, settle=100):
        """{name: fn} -> {name: (median, min, max)} us per call.  These paths are launch-bound, and the host time of one
        call was seen at two levels in one process, so every function first runs `settle` times and
        the functions are then timed in alternation, one window each per round: drift hits all of them alike."""
        for fn in fns.values():
            for _ in range(settle):
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name in fns}
        for _ in range(repeats):
            for name, fn in fns.items():
                t[name].append(timeit(fn, launches))
                MANIFEST[-1].update(name='band/' + name, shape=[B, S, M, N])
        return {name: (statistics.median(v), min(v), max(v)) for name, v in t.items()}

    for k in (0, 3):
        n2 = 2 * ((k + 1) ** 2 - 1)
        mean = torch.randn(B, 2, M, N, device=dev, generator=g).requires_grad_(True)
        diag = torch.exp(-1 + 0.3 * torch.randn(B, 2, M, N, device=dev, generator=g)).requires_grad_(True)
        off = (0.1 * torch.randn(B, n2, M, N, device=dev, generator=g)).requires_grad_(True)
        eps = torch.randn(S * B, 2, M, N, device=dev, generator=g)
        w = torch.randn(S * B, 2, M, N, device=dev, generator=g)
        leaves = (mean, diag, off) if k else (mean, diag)

        def fused_fwd():
            with torch.no_grad():
                T.reparam_triag(mean, diag, off if k else None, k, nsamples=S, eps=eps)

        def torch_fwd():
            with torch.no_grad():
                torch_formulation(mean, diag, off, eps, k)

        def fused_both():
            torch.autograd.grad(T.reparam_triag(mean, diag, off if k else None, k, nsamples=S, eps=eps), leaves, w)

        def torch_both():
            torch.autograd.grad(torch_formulation(mean, diag, off, eps, k), leaves, w)

        same = torch.equal(T.reparam_triag(mean, diag, off if k else None, k, nsamples=S, eps=eps),
                           torch_formulation(mean, diag, off, eps, k))
        # algorithmic bytes: forward = coefficients + mean + eps + z; backward = coefficients + eps + gz in, all gradients out
        plane = 4 * 2 * M * N
        fwd_b = plane * (B * (n2 // 2 + 1) + B + 2 * S * B)
        bwd_b = plane * (B * (n2 // 2 + 1) + 2 * S * B) + plane * (B * (n2 // 2 + 1) + B)
        # the two launches alone, through the C ABI (no autograd node, no allocation)
        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        d_, m_, o_ = diag.detach(), mean.detach(), (off.detach() if k else None)
        z, gX, gm, gd = torch.empty_like(eps), torch.empty_like(eps), torch.empty_like(m_), torch.empty_like(d_)
        go = torch.empty_like(o_) if k else None
        pl, ob = 2 * M * N, n2 * M * N

        def launch_fwd():
            lib.arflow_band_mv_fwd(p(m_), pl, p(d_), pl, p(o_), ob, p(eps), pl, p(z), pl, B, S, M, N, k, 0, st)

        def launch_bwd():
            lib.arflow_band_mv_bwd(p(d_), pl, p(o_), ob, p(eps), pl, p(w), pl, p(gX), pl, p(gm), pl, p(gd), pl, p(go), ob, B, S,
                                   M, N, k, 0, st)

        res = spread({'launch fwd': launch_fwd, 'launch bwd': launch_bwd, 'fused fwd': fused_fwd, 'torch fwd': torch_fwd,
                      'fused fwd+bwd': fused_both, 'torch fwd+bwd': torch_both})
        for name, (med, lo, hi) in res.items():
            nb = bwd_b if name == 'launch bwd' else fwd_b if name.endswith(' fwd') else fwd_b + bwd_b
            print('band k=%d %-14s %9.1f us  (min %.1f .. max %.1f)  %8.1f GB/s algorithmic' % (k, name, med, lo, hi, nb / med / 1e3),
                  flush=True)
        for what in ('fwd', 'fwd+bwd'):
            f, t = res['fused ' + what], res['torch ' + what]
            print('band k=%d %s: fused is %.2fx the torch formulation; ranges %s; same forward bits: %s' % (
                k, what, t[0] / f[0], 'apart' if f[2] < t[1] else 'OVERLAP', same), flush=True)

    # one whole loss step at the flagship size
    H, W, k = 384, 640, 3
    cfg = AttrDict(type='uflow_elbo', edge_constant=150, edge_asymp=0.01, w_smooth=4.0, penalty_smooth='charbonnier',
                   closed_form_smooth=False, data_loss=['census'], data_weight=[1.0], data_penalty=['abs_robust_loss'],
                   w_entropy=0.1, w_oof=0.0, w_occ=0.0, with_bk=True, approx='sparse', cov_supp=k, inv_cov=False,
                   approx_entropy=False, occ_type='sample', n_samples=S, offdiag_reg=0.0, natural_grad=False)
    loss = UFlowElboLoss(cfg)
    nets = [torch.cat((1.5 * torch.randn(B, 2, M, N, device=dev, generator=g), -1 + 0.3 * torch.randn(B, 2, M, N, device=dev, generator=g),
                       0.1 * torch.randn(B, 30, M, N, device=dev, generator=g)), 1).requires_grad_(True) for _ in range(2)]
    ims = [torch.rand(B, 3, H, W, device=dev, generator=g) for _ in range(2)]

    def step():
        out = loss({'flows_fw': [None, None, nets[0]], 'flows_bw': [None, None, nets[1]]}, ims[0], ims[1])
        torch.autograd.grad(out[0], nets)

    med, lo, hi = spread({'loss': step}, settle=20)['loss']
    AF.start_kernel_timing()
    step()
    calls = AF.stop_kernel_timing()
    print('UFlowElboLoss fwd+bwd B=%d S=%d %dx%d k=%d: %9.1f us  (min %.1f .. max %.1f); %d library launches: %s' % (
        B, S, H, W, k, med, lo, hi, sum(len(v) for v in calls.values()), sorted({n for n, _ in calls})), flush=True)


def lowrank_bench(dev, g, S=4, R=15, launches=30, repeats=5):
    """the low-rank node (sampler + Gram log-determinants, one backward launch) at B = 8 on the 96 x 160
    level and at B = 4 on 64 x 112, next to the reference's formulation restated in torch ops (repeat std S-fold, mul, two
    strided channel sums, cat; two bmm and torch.logdet; ATen's autograd of all that).  Protocol of band_bench: 100 untimed
    calls, the functions timed in alternation, `repeats` rounds, median (min .. max); the raw launches through the C ABI next
    to them, with algorithmic bytes."""
    import statistics
    from arflow_amd import lowrank as LR

    def torch_formulation(mean, std, eps):  # losses/uflow_elbo_loss.py:180-188, :362-370
        B, C, h, w = std.shape
        e = std.repeat(S, 1, 1, 1) * eps
        z = mean.repeat(S, 1, 1, 1) + torch.cat((e[:, 0::2].sum(1, keepdim=True), e[:, 1::2].sum(1, keepdim=True)), 1)
        u, v = std[:, 0::2].reshape(B, C // 2, h * w), std[:, 1::2].reshape(B, C // 2, h * w)
        ld = torch.stack((torch.logdet(torch.matmul(u, u.transpose(1, 2))), torch.logdet(torch.matmul(v, v.transpose(1, 2)))), 1)
        return z, ld

    def spread(fns, shape, settle=100):
        for fn in fns.values():
            for _ in range(settle):
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name in fns}
        for _ in range(repeats):
            for name, fn in fns.items():
                t[name].append(timeit(fn, launches))
                MANIFEST[-1].update(name='lowrank/' + name, shape=shape)
        return {name: (statistics.median(v), min(v), max(v)) for name, v in t.items()}

    for B, M, N in ((8, 96, 160), (4, 64, 112)):
        net = torch.cat((1.5 * torch.randn(B, 2, M, N, device=dev, generator=g),
                         0.1 * torch.randn(B, 2 * R, M, N, device=dev, generator=g)), 1).requires_grad_(True)
        eps = torch.randn(S * B, 2 * R, 1, 1, device=dev, generator=g)
        w = torch.randn(S * B, 2, M, N, device=dev, generator=g)
        wl = torch.randn(B, 2, device=dev, generator=g)

        def fused(grad):
            z, ld = LR._LowRank.apply(S, 1, True, True, net[:, 0:2], net[:, 2:], eps)
            if grad:
                torch.autograd.grad((z, ld[0]), net, (w, wl))

        def plain(grad):
            z, ld = torch_formulation(net[:, 0:2], net[:, 2:], eps)
            if grad:
                torch.autograd.grad((z, ld), net, (w, wl))

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    fn(False)
            return run

        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        d = net.detach()
        nb, pl = d.stride(0), M * N
        z = torch.empty(S * B, 2, M, N, device=dev)
        work = torch.empty(lib.arflow_lowrank_work_size(B, R, M, N), device=dev, dtype=torch.float64)
        ld, ginv = torch.empty(B, 2, device=dev), torch.empty(B, 2, R, R, device=dev)
        gnet = torch.empty_like(d)
        mean_p, std_p = p(d), p(d[:, 2:])

        def launch_fwd():
            lib.arflow_lowrank_sample_fwd(mean_p, nb, std_p, nb, p(eps), p(z), 2 * pl, B, S, R, M, N, st)

        def launch_logdet():
            lib.arflow_lowrank_logdet_fwd(std_p, nb, p(work), p(ld), p(ginv), B, R, M, N, st)

        def launch_bwd():
            lib.arflow_lowrank_bwd(std_p, nb, p(eps), p(w), 2 * pl, p(ginv), p(wl), p(gnet), nb, p(gnet[:, 2:]), nb, B, S, R, M, N, st)

        res = spread({'launch fwd': launch_fwd, 'launch logdet': launch_logdet, 'launch bwd': launch_bwd,
                      'fused fwd': no_grad(fused), 'torch fwd': no_grad(plain), 'fused fwd+bwd': lambda: fused(True),
                      'torch fwd+bwd': lambda: plain(True)}, [B, S, R, M, N])
        # algorithmic bytes: forward std + mean + eps + z; log-det std; backward std + gZ in, gstd + gmean out
        std_b, mean_b, z_b = 4 * B * 2 * R * pl, 4 * B * 2 * pl, 4 * S * B * 2 * pl
        nbytes = {'launch fwd': std_b + mean_b + 4 * eps.numel() + z_b, 'launch logdet': std_b,
                  'launch bwd': std_b + z_b + std_b + mean_b}
        tag = 'lowrank B=%d S=%d R=%d %dx%d' % (B, S, R, M, N)
        for name, (med, lo, hi) in res.items():
            gbs = '%8.1f GB/s algorithmic' % (nbytes[name] / med / 1e3) if name in nbytes else ''
            print('%s %-14s %9.1f us  (min %.1f .. max %.1f)  %s' % (tag, name, med, lo, hi, gbs), flush=True)
        for what in ('fwd', 'fwd+bwd'):
            f, t = res['fused ' + what], res['torch ' + what]
            print('%s %s: fused is %.2fx the torch formulation; ranges %s' % (tag, what, t[0] / f[0],
                                                                             'apart' if f[2] < t[1] else 'OVERLAP'), flush=True)


def mixture_bench(dev, g, B=4, S=6, K=2, M=96, N=160, launches=30, repeats=5):
    """the mixture node (sampler + log-density forward, one backward launch) at the workload's level-2
    shape at 384 x 640 (B = 4, S = 6, K = 2, 96 x 160), next to the reference's formulation restated in torch ops (multinomial
    draws given; four gathers, transposes and a cat for the sample; mean and log_std repeated S-fold, exp, the K error maps,
    their squares, the log-determinants, two reductions over the pixels, the weighted log-sum-exp; ATen's autograd of all
    that).  Protocol of lowrank_bench: 100 untimed calls, the functions timed in alternation, `repeats` rounds, median (min ..
    max); the raw launches through the C ABI next to them, with algorithmic bytes."""
    import statistics
    from arflow_amd import mixture as MX

    def torch_formulation(mean, log_std, weights, comp, eps):  # losses/uflow_elbo_loss.py:159-178, utils/misc_utils.py:67-101
        std = torch.exp(log_std)
        z = comp[:, :, None, None].repeat(1, 1, M, N)
        pick = lambda t, c: torch.gather(t, 1, 2 * z + c).transpose(1, 0).reshape(-1, 1, M, N)  # noqa: E731
        flow = torch.cat((pick(mean, 0), pick(mean, 1)), 1) + torch.cat((pick(std, 0), pick(std, 1)), 1) * eps
        mean_r, ls_r, w_r = mean.repeat(S, 1, 1, 1), log_std.repeat(S, 1, 1, 1), weights.repeat(S, 1)
        std_r = torch.exp(ls_r)
        u = (flow[:, [0]] - mean_r[:, 0::2]) / std_r[:, 0::2]
        v = (flow[:, [1]] - mean_r[:, 1::2]) / std_r[:, 1::2]
        x = -torch.sum(ls_r[:, 0::2] + ls_r[:, 1::2], dim=(2, 3)) - torch.sum(u * u + v * v, dim=(2, 3)) / 2
        top, _ = torch.max(x, dim=1, keepdim=True)
        return flow, (top + torch.log(torch.sum(w_r * torch.exp(x - top), dim=1, keepdim=True))) / (M * N)

    def spread(fns, shape, settle=100):
        for fn in fns.values():
            for _ in range(settle):
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name in fns}
        for _ in range(repeats):
            for name, fn in fns.items():
                t[name].append(timeit(fn, launches))
                MANIFEST[-1].update(name='mixture/' + name, shape=shape)
        return {name: (statistics.median(v), min(v), max(v)) for name, v in t.items()}

    net = torch.cat((1.5 * torch.randn(B, 2 * K, M, N, device=dev, generator=g),
                     -1 + 0.3 * torch.randn(B, 2 * K, M, N, device=dev, generator=g)), 1).requires_grad_(True)
    weights = torch.full((B, K), 1.0 / K, device=dev)
    comp = torch.multinomial(weights, S, replacement=True, generator=g)
    eps = torch.randn(S * B, 2, M, N, device=dev, generator=g)
    w = torch.randn(S * B, 2, M, N, device=dev, generator=g)
    wl = torch.randn(S * B, device=dev, generator=g)

    def fused(grad):
        z, lp = MX._Mixture.apply(S, 1, net, None, weights, comp, eps)
        if grad:
            torch.autograd.grad((z, lp[0]), net, (w, wl))

    def plain(grad):
        z, lp = torch_formulation(net[:, :2 * K], net[:, 2 * K:], weights, comp, eps)
        if grad:
            torch.autograd.grad((z, lp[:, 0]), net, (w, wl))

    def no_grad(fn):
        def run():
            with torch.no_grad():
                fn(False)
        return run

    with torch.no_grad():  # the two formulations agree before they are timed
        (za, la), (zb, lb) = MX._Mixture.apply(S, 1, net, None, weights, comp, eps), torch_formulation(net[:, :2 * K], net[:, 2 * K:], weights, comp, eps)
    print('mixture: max |flow - torch| %.3e, max |logpdf - torch| %.3e' % (float((za - zb).abs().max()), float((la[0] - lb[:, 0]).abs().max())), flush=True)

    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    d = net.detach()
    nb, pl = d.stride(0), M * N
    z = torch.empty(S * B, 2, M, N, device=dev)
    work = torch.empty(lib.arflow_mixture_work_size(B, S, K, M, N), device=dev, dtype=torch.float64)
    lp, resp, q = torch.empty(S * B, device=dev), torch.empty(S * B, K, device=dev), torch.empty(S * B, K, device=dev)
    gnet = torch.empty_like(d)
    mean_p, ls_p = p(d), p(d[:, 2 * K:])

    def launch_fwd():
        lib.arflow_mixture_sample_fwd(mean_p, nb, ls_p, nb, p(eps), 2 * pl, p(comp), p(z), 2 * pl, p(work), B, S, K, M, N, st)

    def launch_logpdf():
        lib.arflow_mixture_logpdf_fwd(p(work), p(weights), p(lp), p(resp), p(q), B, S, K, M, N, st)

    def launch_bwd():
        lib.arflow_mixture_bwd(mean_p, nb, ls_p, nb, p(eps), 2 * pl, p(comp), p(resp), p(wl), p(w), 2 * pl, p(gnet), nb,
                               p(gnet[:, 2 * K:]), nb, B, S, K, M, N, st)

    launch_fwd()
    launch_logpdf()
    res = spread({'launch fwd': launch_fwd, 'launch logpdf': launch_logpdf, 'launch bwd': launch_bwd,
                  'fused fwd': no_grad(fused), 'torch fwd': no_grad(plain), 'fused fwd+bwd': lambda: fused(True),
                  'torch fwd+bwd': lambda: plain(True)}, [B, S, K, M, N])
    # algorithmic bytes: forward mean + log_std + eps in, flow out; backward mean + log_std + eps + gZ in, both gradients out
    par_b, smp_b = 4 * B * 4 * K * pl, 4 * S * B * 2 * pl
    nbytes = {'launch fwd': par_b + 2 * smp_b, 'launch bwd': par_b + 2 * smp_b + par_b}
    tag = 'mixture B=%d S=%d K=%d %dx%d' % (B, S, K, M, N)
    for name, (med, lo, hi) in res.items():
        gbs = '%8.1f GB/s algorithmic' % (nbytes[name] / med / 1e3) if name in nbytes else ''
        print('%s %-14s %9.1f us  (min %.1f .. max %.1f)  %s' % (tag, name, med, lo, hi, gbs), flush=True)
    for what in ('fwd', 'fwd+bwd'):
        f, t = res['fused ' + what], res['torch ' + what]
        print('%s %s: fused is %.2fx the torch formulation; ranges %s' % (tag, what, t[0] / f[0],
                                                                         'apart' if f[2] < t[1] else 'OVERLAP'), flush=True)


def out_up_bench(dev, g, B2=8, launches=30, repeats=5):
    """the output upsample of PWCProbFlow -- AF.out_upsample / AF.out_tail (one launch each way) next to
    the composed ATen path the model runs with ARFLOW_OUT_UP=0 (split, bias add, F.interpolate per group, x2, cat, and
    ATen's autograd of that), at the workload's own shapes with 2B = 8: C = 4 at the 12x20, 24x40 and 48x80 inputs, and the
    tail (two steps) at 34 x 96 x 160.  The two versions alternate, `repeats` windows of `launches` calls each: median and
    (min .. max).  Bytes are algorithmic: every input element read once, every output element written once (backward: the
    fine gradients read once, the coarse one written once); the share is of the HBM3E spec peak, 8 TB/s.  Then, the kernels
    alone, the other entry points of csrc/upsample.hip: prob_upsample, flow_upsample and the raw arflow_up2_bwd."""
    import math
    import statistics
    import torch.nn.functional as F
    from arflow_amd import functional as AF
    bias = math.log(2.0)

    def composed(x, n_flow=2, n_diag=2):
        up = lambda v: F.interpolate(v, scale_factor=2.0, mode='bilinear', align_corners=False)  # noqa: E731
        parts = [up(x[:, :n_flow]) * 2.0, up(x[:, n_flow:n_flow + n_diag] + bias)]
        if x.shape[1] > n_flow + n_diag:
            parts.append(up(x[:, n_flow + n_diag:]))
        return torch.cat(parts, 1)

    def spread(fns):
        for fn in fns.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name in fns}
        for _ in range(repeats):
            for name, fn in fns.items():
                t[name].append(timeit(fn, launches))
                MANIFEST[-1].update(name='out_up/' + name, shape=[])
        return {name: (statistics.median(v), min(v), max(v)) for name, v in t.items()}

    def report(tag, res, nbytes):
        for what in ('fwd', 'bwd'):
            f, t = res['fused ' + what], res['aten ' + what]
            nb = nbytes[what]
            print('out_up %-22s %s  fused %8.1f us (%.1f .. %.1f) %7.1f GB/s %5.2f%% of the 8 TB/s HBM peak | ATen %8.1f us '
                  '(%.1f .. %.1f) %7.1f GB/s | %.2fx, ranges %s' % (
                      tag, what, f[0], f[1], f[2], nb / f[0] / 1e3, 100 * nb / f[0] / 1e3 / HBM_PEAK_GBS, t[0], t[1], t[2],
                      nb / t[0] / 1e3, t[0] / f[0], 'apart' if (f[2] < t[1] or t[2] < f[1]) else 'OVERLAP'), flush=True)

    for C, h, w in ((4, 12, 20), (4, 24, 40), (4, 48, 80)):
        x = torch.randn(B2, C, h, w, device=dev, generator=g).requires_grad_(True)
        go = torch.randn(B2, C, 2 * h, 2 * w, device=dev, generator=g)
        yf, ya = AF.out_upsample(x, 2, 2, bias), composed(x)

        def ffwd():
            with torch.no_grad():
                AF.out_upsample(x, 2, 2, bias)

        def afwd():
            with torch.no_grad():
                composed(x)
        res = spread({'fused fwd': ffwd, 'aten fwd': afwd,
                      'fused bwd': lambda: torch.autograd.grad(yf, x, go, retain_graph=True),
                      'aten bwd': lambda: torch.autograd.grad(ya, x, go, retain_graph=True)})
        n = 4 * B2 * C * h * w
        report('x2 %s' % [B2, C, h, w], res, {'fwd': 5 * n, 'bwd': 5 * n})
    C, h, w = 34, 96, 160
    x = torch.randn(B2, C, h, w, device=dev, generator=g).requires_grad_(True)
    g1 = torch.randn(B2, C, 2 * h, 2 * w, device=dev, generator=g)
    g0 = torch.randn(B2, C, 4 * h, 4 * w, device=dev, generator=g)
    tf = AF.out_tail(x, 2, 2, bias)
    a1 = composed(x)
    ta = (a1, composed(a1))
    print('out_up tail: same bits as the composed path: out1 %s, out0 %s' % (torch.equal(tf[0], ta[0]), torch.equal(tf[1], ta[1])))

    def tfwd():
        with torch.no_grad():
            AF.out_tail(x, 2, 2, bias)

    def tafwd():
        with torch.no_grad():
            composed(composed(x))
    res = spread({'fused fwd': tfwd, 'aten fwd': tafwd,
                  'fused bwd': lambda: torch.autograd.grad(tf, x, [g1, g0], retain_graph=True),
                  'aten bwd': lambda: torch.autograd.grad(ta, x, [g1, g0], retain_graph=True)})
    n = 4 * B2 * C * h * w
    # forward: x read, out1 and out0 written; backward: g0 and g1 read, gx written (the level-1 gradient in between is
    # the composed algorithm's own traffic, not counted)
    report('tail %s' % [B2, C, h, w], res, {'fwd': 21 * n, 'bwd': 21 * n})

    # the rest of the upsample family, the kernels alone: prob_upsample at PWCLiteProb's finest level,
    # flow_upsample at [16, 2, 48, 80] and the raw x2 adjoint of the level backward at its own fine sizes
    def solo(tag, make, x, go):
        y = make(x)

        def fwd():
            with torch.no_grad():
                make(x)
        res = spread({'fwd': fwd, 'bwd': lambda: torch.autograd.grad(y, x, go, retain_graph=True)})
        for what, (med, lo, hi) in res.items():
            print('out_up %-34s %s  fused %8.1f us (%.1f .. %.1f)' % (tag, what, med, lo, hi), flush=True)

    for f, C, nf, nd, h, w in ((4, 4, 2, 2, 96, 160), (2, 2, 0, 2, 48, 80)):
        x = torch.randn(16, C, h, w, device=dev, generator=g).requires_grad_(True)
        go = torch.randn(16, C, f * h, f * w, device=dev, generator=g)
        solo('prob_upsample x%d %s' % (f, [16, C, h, w]), lambda t: AF.prob_upsample(t, f, nf, nd, 2 * math.log(f)), x, go)
    for f in (2, 4):
        x = torch.randn(16, 2, 48, 80, device=dev, generator=g).requires_grad_(True)
        go = torch.randn(16, 2, f * 48, f * 80, device=dev, generator=g)
        solo('flow_upsample x%d %s' % (f, [16, 2, 48, 80]), lambda t: AF.flow_upsample(t, f, True), x, go)
    from arflow_amd import _lib
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    for H, W in ((96, 160), (12, 20)):
        gf = torch.randn(16, 2, H, W, device=dev, generator=g)
        gc = torch.empty(16, 2, H // 2, W // 2, device=dev)
        res = spread({'bwd': lambda: lib.arflow_up2_bwd(p(gf), p(gc), 16, H, W, 1, st)})
        print('out_up %-34s bwd  fused %8.1f us (%.1f .. %.1f)' % ('arflow_up2_bwd %s' % [16, 2, H, W], *res['bwd']), flush=True)
    # the nodes above are host-bound (tens of us of autograd around a launch of a few): the same entry points as bare C-ABI
    # launches back to back, which is what resolves a change to a kernel
    def raw(tag, C, h, w, f, fwd, bwd):
        a, b = torch.randn(16, C, h, w, device=dev, generator=g), torch.randn(16, C, f * h, f * w, device=dev, generator=g)
        assert fwd(p(a), p(b), C, h, w) == 0 and bwd(p(b), p(a), C, h, w) == 0
        res = spread({'fwd': lambda: fwd(p(a), p(b), C, h, w), 'bwd': lambda: bwd(p(b), p(a), C, h, w)})
        for what, (med, lo, hi) in res.items():
            print('out_up %-34s %s  launch %7.1f us (%.1f .. %.1f)' % ('%s %s' % (tag, [16, C, h, w]), what, med, lo, hi), flush=True)

    for C, h, w in ((4, 48, 80), (34, 96, 160)):  # (the second: long enough to show the kernel, not the launch rate)
        raw('arflow_out_up2', C, h, w, 2,
            lambda a, b, C, h, w: lib.arflow_out_up2_fwd(a, C * h * w, b, 4 * C * h * w, 16, C, h, w, 2, 2, bias, st),
            lambda b, a, C, h, w: lib.arflow_out_up2_bwd(b, 4 * C * h * w, a, C * h * w, 16, C, h, w, 2, st))
    for f, C, h, w in ((4, 4, 96, 160), (2, 2, 48, 80)):
        raw('arflow_prob_up x%d' % f, C, h, w, f,
            lambda a, b, C, h, w: lib.arflow_prob_up_fwd(a, C * h * w, b, f * f * C * h * w, 16, C, h, w, f, 2, C - 2, bias, st),
            lambda b, a, C, h, w: lib.arflow_prob_up_bwd(b, f * f * C * h * w, a, C * h * w, 16, C, h, w, f, 2, st))
    for f in (2, 4):
        for ac in (0, 1):
            raw('arflow_flow_up x%d align %d' % (f, ac), 2, 48, 80, f,
                lambda a, b, C, h, w: lib.arflow_flow_up_fwd(a, b, 16, h, w, f, ac, st),
                lambda b, a, C, h, w: lib.arflow_flow_up_bwd(b, a, 16, h, w, f, ac, st))


def gauss_pyr_bench(dev, g, B=8, H=384, W=640, launches=30, repeats=5):
    """the pyramid sampler node (arflow_amd.gauss_pyr.reparam_pyramid: one launch for all scales and both
    directions, one fold launch, one adjoint launch) at the five scales of a 384 x 640 pair with B = 8 -- 384 x 640 ... 24 x 40,
    the upsampled outputs of PWCLiteProb -- next to the reference's formulation restated in torch ops (per scale and direction
    slice, repeat, exp, mul, add; the two channel sums and means of the entropy; cat; and ATen's autograd of all that), and
    one whole ElboLoss step (forward + backward to the nets) next to unFlowLoss fed by torch-made samples.  HIP events around
    `launches` calls after 5 warm-ups, the versions in alternation, `repeats` rounds: median (min .. max)."""
    import statistics
    from arflow_amd.config import AttrDict
    from arflow_amd.gauss_pyr import reparam_pyramid
    from arflow_amd.losses import get_loss
    from arflow_amd.losses.flow_loss import unFlowLoss
    from arflow_amd.train_step import WORKLOADS, synthetic_pairs
    sizes = [(H >> k, W >> k) for k in range(5)]
    nets = [(0.5 * torch.randn(B, 8, h, w, device=dev, generator=g)).requires_grad_(True) for h, w in sizes]
    eps = [torch.randn(B, 4, h, w, device=dev, generator=g) for h, w in sizes]
    gz = [torch.randn(B, 4, h, w, device=dev, generator=g) for h, w in sizes]
    gent = torch.randn(5, 2, device=dev, generator=g, dtype=torch.float64)

    def torch_node(nets):
        zs, ents = [], []
        for net, e in zip(nets, eps):
            parts = []
            for d in (0, 1):
                mean, lv = net[:, 4 * d:4 * d + 2].repeat(1, 1, 1, 1), net[:, 4 * d + 2:4 * d + 4].repeat(1, 1, 1, 1)
                parts.append(mean + torch.exp(lv / 2.0) * e[:, 2 * d:2 * d + 2])
                ents.append(torch.sum(net[:, 4 * d + 2:4 * d + 4], dim=1).sum())
            zs.append(torch.cat(parts, 1))
        return zs, torch.stack(ents).view(5, 2)

    def objective(zs, ent):
        return sum((z * w).sum() for z, w in zip(zs, gz)) + (ent.double() * gent).sum()

    def spread(fns, tag):
        t = {name: [] for name in fns}
        for _ in range(repeats):
            for name, fn in fns.items():
                t[name].append(timeit(fn, launches))
                MANIFEST[-1].update(name='gauss_pyr/' + name, shape=[])
        for name, v in t.items():
            print('gauss_pyr %-28s %-22s %9.1f us (%.1f .. %.1f)' % (tag, name, statistics.median(v), min(v), max(v)), flush=True)
        return t

    def hip_fwd():
        with torch.no_grad():
            reparam_pyramid(nets, eps)

    def aten_fwd():
        with torch.no_grad():
            torch_node(nets)
    zh, eh = reparam_pyramid(nets, eps)
    za, ea = torch_node(nets)
    oh, oa = objective(zh, eh), objective(za, ea)
    spread({'kernels fwd': hip_fwd, 'torch fwd': aten_fwd,
            'kernels bwd': lambda: torch.autograd.grad(oh, nets, retain_graph=True),
            'torch bwd': lambda: torch.autograd.grad(oa, nets, retain_graph=True)}, 'node %s x5' % [B, 8, H, W])
    n = sum(B * h * w for h, w in sizes)
    print('gauss_pyr algorithmic bytes: fwd %d (8 + 4 read, 4 written per pixel), bwd %d (8 + 4 + 4 read, 8 written)'
          % (4 * 16 * n, 4 * 24 * n))
    # the align_corners=True upsample alone, at the model's finest level with 2B = 16: the x4 of the state and the x2 of the
    # log-variance, next to the composed ATen expression the model keeps for CPU tensors
    import math
    import torch.nn.functional as F
    from arflow_amd import functional as AF
    for f, C, nf, nd, h, w in ((4, 4, 2, 2, H // 4, W // 4), (2, 2, 0, 2, H // 8, W // 8)):
        bias = 2 * math.log(f)
        x = torch.randn(2 * B, C, h, w, device=dev, generator=g).requires_grad_(True)
        go = torch.randn(2 * B, C, f * h, f * w, device=dev, generator=g)

        def composed(t):
            up = lambda v: F.interpolate(v, scale_factor=f, mode='bilinear', align_corners=True)  # noqa: E731
            parts = ([up(t[:, :nf] * f)] if nf else []) + [up(t[:, nf:nf + nd] + bias)]
            return parts[0] if len(parts) == 1 else torch.cat(parts, 1)
        yk, ya = AF.prob_upsample(x, f, nf, nd, bias), composed(x)

        def kfwd():
            with torch.no_grad():
                AF.prob_upsample(x, f, nf, nd, bias)

        def afwd():
            with torch.no_grad():
                composed(x)
        spread({'kernels fwd': kfwd, 'ATen fwd': afwd,
                'kernels bwd': lambda: torch.autograd.grad(yk, x, go, retain_graph=True),
                'ATen bwd': lambda: torch.autograd.grad(ya, x, go, retain_graph=True)}, 'prob_upsample x%d %s' % (f, [2 * B, C, h, w]))
    lcfg = AttrDict(WORKLOADS['pwcliteprob+elbo_loss'][1])
    elbo, plain = get_loss(lcfg), unFlowLoss(lcfg)
    img = synthetic_pairs(B, H, W, device=dev, seed=3)

    def elbo_step():
        torch.autograd.grad(elbo(nets, img, eps=eps)[0], nets)

    def torch_step():
        zs, ent = torch_node(nets)
        coef = torch.tensor([[0.1 / (B * h * w) / 4] * 2 for h, w in sizes], device=dev)
        torch.autograd.grad(plain(zs, img)[0] - (ent * coef).sum(), nets)
    spread({'ElboLoss step': elbo_step, 'unFlowLoss + torch samples': torch_step}, 'loss %s' % [B, 6, H, W])


def mse_bench(dev, g, B=16, h=96, w=128, H=384, W=512, launches=30, repeats=5):
    """one MseLoss step -- forward plus backward to the level-2 output -- at 16 x (96 x 128 from 384 x 512),
    S = 1 and S = 4, for a diagonal mode (inv_cov) and the shipped 4-neighbour inv_cov mode, next to the reference's formulation
    composed of ATen ops on the same GPU (losses/mse_loss.py:60-148: interpolate, two in-place divides, repeats, exp, mul, add,
    sub, square, mean, sum, mean; the 4-neighbour solve is BackwardSubst in both versions).  HIP events around `launches` steps
    after 5 warm-ups, the versions in alternation, `repeats` rounds: median (min .. max); GPU kernels per step counted by
    torch.profiler where it is available."""
    import statistics
    import torch.nn.functional as F
    from arflow_amd.config import AttrDict
    from arflow_amd.losses import get_loss
    from arflow_amd.triag_solve import BackwardSubst
    net = torch.randn(B, 8, h, w, device=dev, generator=g)
    net[:, 2:4] = 0.5 * net[:, 2:4] - 1.0
    net[:, 4:8] = 0.3 * torch.rand(B, 4, h, w, device=dev, generator=g) - 0.15
    net.requires_grad_(True)
    target = 3.0 * torch.randn(B, 2, H, W, device=dev, generator=g)

    def composed(cfg, eps):
        S = cfg.n_samples
        mean, ld = net[:, 0:2], net[:, 2:4]
        off = 0
        if cfg.diag:
            z = mean.repeat(S, 1, 1, 1) + torch.exp(-ld.repeat(S, 1, 1, 1)) * eps
        else:
            left, over = net[:, 4:6, :, :-1], net[:, 6:8, :-1, :]
            off = cfg.offdiag_reg * (torch.mean(torch.square(left)) + torch.mean(torch.square(over))) / 2.0
            rep = lambda t: t.repeat(S, 1, 1, 1)  # noqa: E731
            z = rep(mean) + BackwardSubst.apply(rep(torch.exp(ld)), rep(left), rep(over), None, eps)
        ent = -cfg.w_entropy * torch.sum(ld, dim=1).mean()
        gt = F.interpolate(target, (h, w), mode='bilinear', align_corners=False)
        gt[:, 0] /= W / float(w)
        gt[:, 1] /= H / float(h)
        return cfg.w_mse * torch.mean(torch.square(z - gt.repeat(S, 1, 1, 1))) - ent + off

    def kernels_per_step(fn):
        try:
            from torch.profiler import ProfilerActivity, profile
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            return sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        except Exception as e:  # the profiler is an extra: the timings do not depend on it
            return 'n/a (%s)' % type(e).__name__

    for diag in (True, False):
        for S in (1, 4):
            cfg = AttrDict(type='mse', w_mse=1.0, w_entropy=0.1, diag=diag, diag_dominant=False, inv_cov=True,
                           approx_entropy=False, offdiag_reg=1000.0, n_samples=S)
            loss = get_loss(cfg)
            eps = torch.randn(S * B, 2, h, w, device=dev, generator=g)
            fns = {'fused step': lambda: torch.autograd.grad(loss([None, None, net], target, eps=eps)[0], net),
                   'composed ATen step': lambda: torch.autograd.grad(composed(cfg, eps), net)}
            a, b = float(loss([None, None, net], target, eps=eps)[0].detach()), float(composed(cfg, eps).detach())
            t = {name: [] for name in fns}
            for _ in range(repeats):
                for name, fn in fns.items():
                    t[name].append(timeit(fn, launches))
                    MANIFEST[-1].update(name='mse/' + name, shape=[])
            tag = '%s inv_cov S=%d %s<-%s' % ('diag' if diag else '4-neighbour', S, [B, h, w], [H, W])
            for name, v in t.items():
                print('mse %-44s %-20s %9.1f us (%.1f .. %.1f)  GPU kernels per step: %s'
                      % (tag, name, statistics.median(v), min(v), max(v), kernels_per_step(fns[name])), flush=True)
            print('mse %-44s composed / fused = %.2f   (loss %.6f fused, %.6f composed)'
                  % (tag, statistics.median(t['composed ATen step']) / statistics.median(t['fused step']), a, b), flush=True)


def augment_bench(dev, jsonl, B=64, src_hw=(384, 512), crop_hw=(256, 448), launches=20, repeats=5):
    """arflow_amd.augment.augment_batch (one launch; two where contrast is active) on B = 64 uint8 pairs of
    384 x 512 cropped to 256 x 448 -- configs/chairs_uflow_elbo.json: hflip, crop, hue 0.5, swap_channels -- and the same
    geometry under the full jitter (brightness, contrast, saturation 0.4, hue 0.5, gamma, swap), next to the same transform
    composed of ATen operations on the same device (tests/augment_ref.py in float32: index gather for crop and flip, the
    formulas of the four operations per group of samples that share an operation at a step, pow, index permutation).  HIP
    events around `launches` calls after 5 warm-ups, the versions in alternation, `repeats` rounds: median (min .. max).
    Algorithmic bytes: the crop windows of the source once + both outputs once."""
    import statistics
    from arflow_amd import augment as A
    from tests import augment_ref as R
    cpu = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (B, 2, 3) + tuple(src_hw), dtype=torch.uint8, generator=cpu).to(dev)
    geo = dict(crop=True, crop_size=list(crop_hw), hflip=True)
    cases = {'hue+swap (chairs_uflow_elbo.json)': dict(hue=0.5, swap_channels=True),
             'full jitter, contrast active': dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.5, gamma=1, swap_channels=True)}
    th, tw = crop_hw
    nbytes = B * 2 * 3 * th * tw * (1 + 2 * 4)
    with open(jsonl, 'a') as out:
        for tag, pho in cases.items():
            params = A.draw_params(geo, pho, B, src_hw, cpu)
            fns = {'fused': lambda: A.augment_batch(src, params), 'composed ATen': lambda: R.augment(src, params, dtype=torch.float32)}
            a, b = fns['fused'](), fns['composed ATen']()
            diff = [float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max())]
            del a, b
            t = {name: [] for name in fns}
            for _ in range(repeats):
                for name, fn in fns.items():
                    t[name].append(timeit(fn, launches))
                    MANIFEST[-1].update(name='augment/' + name, shape=[])
            line = {'bench': 'augment', 'case': tag, 'shape': [B, 2, 3] + list(src_hw), 'crop': list(crop_hw), 'dtype': 'uint8',
                    'algorithmic_bytes': nbytes, 'max_abs_diff_img': diff[0], 'max_abs_diff_img_ph': diff[1]}
            for name, v in t.items():
                key = name.split()[0]
                line.update({key + '_us': statistics.median(v), key + '_us_min': min(v), key + '_us_max': max(v)})
                print('augment %-36s %-14s %9.1f us (%.1f .. %.1f)' % (tag, name, statistics.median(v), min(v), max(v)), flush=True)
            gbs = nbytes / line['fused_us'] / 1e3
            line.update(fused_gbs=gbs, fused_fraction_of_hbm_peak=gbs / HBM_PEAK_GBS, hbm_peak_gbs=HBM_PEAK_GBS,
                        composed_over_fused=line['composed_us'] / line['fused_us'])
            print('augment %-36s composed / fused = %.2f   fused %.0f GB/s = %.1f%% of HBM peak   (max |diff| img %.1e, img_ph %.1e)'
                  % (tag, line['composed_over_fused'], gbs, 100 * gbs / HBM_PEAK_GBS, diff[0], diff[1]), flush=True)
            out.write(json.dumps(line) + '\n')


def ar_bench(dev, jsonl, B=8, hw=(384, 640), launches=20, repeats=5, steps=10):
    """the fused transform (arflow_ar_transform, one launch: 6 image channels, the flow and the mask of B = 8
    pairs of 384 x 640 under the drawn theta of ar.DEFAULT_ST_CFG) next to the same transform composed of ATen operations on the
    same device (tests/ar_ref.composed: three grid_sample calls, the border mask, the 2 x 2 product), and the loss node forward +
    backward next to its ATen formulation.  HIP events around `launches` calls after 5 warm-ups, the versions in alternation,
    `repeats` rounds: median (min .. max).  Algorithmic bytes: every plane read once and written once (transform: 9 + 9 planes;
    loss: pred, flow_t, mask forward and backward, the gradient stored: 12 planes).  Then the step time of pwclite+unflow_loss
    with and without ar_cfg, `steps` steps per round after 3 warm-ups, in alternation."""
    import statistics
    from arflow_amd import ar as AR
    from arflow_amd.functional import _call, _stream
    from arflow_amd.train_step import TrainStep, synthetic_pairs
    from tests import ar_ref as R
    H, W = hw
    cpu = torch.Generator().manual_seed(0)
    theta = AR.draw_ar_params(AR.DEFAULT_ST_CFG, B, hw, cpu).to(dev)
    img = torch.rand(B, 6, H, W, generator=cpu).to(dev)
    flow = (3.0 * torch.randn(B, 2, H, W, generator=cpu)).to(dev)
    noc = (torch.rand(B, 1, H, W, generator=cpu) > 0.2).float().to(dev)

    def fused():
        out = [torch.empty_like(img), torch.empty_like(flow), torch.empty_like(noc)]
        _call('arflow_ar_transform', p(theta), p(img), p(out[0]), 6, p(flow), p(out[1]), p(noc), p(out[2]), B, H, W, H, W, _stream())
        return out

    pred = (flow + torch.randn(B, 2, H, W, generator=cpu).to(dev))
    eps, q = 0.01, 0.4

    def node(loss):
        x = pred.clone().requires_grad_(True)
        loss(x, flow, noc, eps, q).backward()
        return x.grad
    cases = {'transform': ({'fused': fused, 'composed ATen': lambda: R.composed(theta, img, flow, noc)}, 18 * B * H * W * 4),
             'loss fwd+bwd': ({'fused': lambda: node(AR.ar_loss), 'composed ATen': lambda: node(R.composed_loss)}, 12 * B * H * W * 4)}
    with open(jsonl, 'a') as out:
        for tag, (fns, nbytes) in cases.items():
            a, b = fns['fused'](), fns['composed ATen']()
            diff = max(float((x - y).abs().max()) for x, y in (zip(a, b) if tag == 'transform' else [(a, b)]))
            del a, b
            t = {name: [] for name in fns}
            for _ in range(repeats):
                for name, fn in fns.items():
                    t[name].append(timeit(fn, launches))
                    MANIFEST[-1].update(name='ar/%s/%s' % (tag, name), shape=[])
            line = {'bench': 'ar', 'case': tag, 'shape': [B, 6 + 2 + 1, H, W], 'st_cfg': {k: list(v) if isinstance(v, tuple) else v
                                                                                        for k, v in AR.DEFAULT_ST_CFG.items()},
                    'algorithmic_bytes': nbytes, 'max_abs_diff': diff}
            for name, v in t.items():
                key = name.split()[0]
                line.update({key + '_us': statistics.median(v), key + '_us_min': min(v), key + '_us_max': max(v)})
                print('ar %-14s %-14s %9.1f us (%.1f .. %.1f)' % (tag, name, statistics.median(v), min(v), max(v)), flush=True)
            gbs = nbytes / line['fused_us'] / 1e3
            line.update(fused_gbs=gbs, fused_fraction_of_hbm_peak=gbs / HBM_PEAK_GBS, hbm_peak_gbs=HBM_PEAK_GBS,
                        composed_over_fused=line['composed_us'] / line['fused_us'])
            print('ar %-14s composed / fused = %.2f   fused %.0f GB/s = %.1f%% of HBM peak   (max |diff| %.1e)'
                  % (tag, line['composed_over_fused'], gbs, 100 * gbs / HBM_PEAK_GBS, diff), flush=True)
            out.write(json.dumps(line) + '\n')
        # the whole step, with and without the second pass
        x = synthetic_pairs(B, H, W, device=dev, seed=5)
        ar_cfg = dict(w_ar=0.01, ar_eps=eps, ar_q=q, mask_st=True, st_cfg=AR.DEFAULT_ST_CFG)
        runs = {'plain': TrainStep('pwclite+unflow_loss', dev, seed=0), 'ar_cfg': TrainStep('pwclite+unflow_loss', dev, seed=0, ar_cfg=ar_cfg)}
        t = {name: [] for name in runs}
        for r in range(repeats):
            for name, step in runs.items():
                for _ in range(3 if r == 0 else 1):
                    step(x)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    step(x)
                e1.record()
                torch.cuda.synchronize()
                t[name].append(e0.elapsed_time(e1) / steps)
        line = {'bench': 'ar', 'case': 'step pwclite+unflow_loss', 'shape': [B, 6, H, W], 'steps': steps}
        for name, v in t.items():
            line.update({name + '_ms': statistics.median(v), name + '_ms_min': min(v), name + '_ms_max': max(v)})
            print('ar step %-8s %8.2f ms (%.2f .. %.2f)' % (name, statistics.median(v), min(v), max(v)), flush=True)
        line['ar_over_plain'] = line['ar_cfg_ms'] / line['plain_ms']
        out.write(json.dumps(line) + '\n')


def render_bench(dev, jsonl, B=8, hw=(384, 640), out_hw=(436, 1024), launches=20, repeats=5):
    """what arflow_amd.predict does per batch after the model call -- the flow [B,2,h,w] restored to
    NHWC at the original size with its per-sample statistics (arflow_amd.render.restore, one pass) and the uint8 flow picture
    normalised by the sample's max |f| (flow_rgb, one pass) -- next to the same outputs composed of ATen operations on the same
    device: F.interpolate, the two scalings, permute().contiguous(), abs / amax, the colour expression and .to(torch.uint8).  The
    parent has no such path, so the composition is the baseline.  HIP events around `launches` calls after 5 warm-ups, the
    versions in alternation, `repeats` rounds: median (min .. max).  Bytes: what each side's operations read and write, counted
    per operation from the shapes (an elementwise ATen operation reads its inputs and writes its output once)."""
    import statistics
    import torch.nn.functional as F
    from arflow_amd import render
    (h, w), (H, W) = hw, out_hw
    flow = 6.0 * torch.randn(B, 2, h, w, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    scale = torch.tensor([W / w, H / h], device=dev).view(1, 2, 1, 1)

    def fused():
        r = render.restore(flow, out_hw, stats=True)
        return r.flow, render.flow_rgb(r.flow, 'rgb', layout='nhwc', stats=r.stats)

    def composed():
        up = F.interpolate(flow, out_hw, mode='bilinear', align_corners=False) * scale
        nhwc = up.permute(0, 2, 3, 1).contiguous()
        n = up / up.abs().amax((1, 2, 3), keepdim=True)
        c = torch.stack([1 + n[:, 0], 1 - 0.5 * (n[:, 0] + n[:, 1]), 1 + n[:, 1]], -1).clamp(0, 1)
        return nhwc, (c * 255.0).to(torch.uint8)
    small, big = 4 * B * 2 * h * w, 4 * B * 2 * H * W  # the flow at the test size / at the original size, in bytes
    plane = big // 2
    bytes_fused = (small + big) + (big + 3 * B * H * W)  # restore: in, out;  picture: in, out
    # interpolate (in, out), * scale (r, w), permute copy (r, w), abs (r, w), amax (r), / (r, w), 1 + n_u (r, w), n_u + n_v (2r, w),
    # 0.5 * (r, w), 1 - (r, w), 1 + n_v (r, w), stack (3r, 3w), clamp (3r, 3w), * 255 (3r, 3w), to uint8 (3r, 3 B H W)
    bytes_composed = (small + big) + 2 * big + 2 * big + 2 * big + big + 2 * big + 2 * plane + 3 * plane + 2 * plane + 2 * plane \
        + 2 * plane + 6 * plane + 6 * plane + 6 * plane + 3 * plane + 3 * B * H * W
    fns = {'fused': fused, 'composed ATen': composed}
    a, b = fused(), composed()
    diff_flow = float((a[0] - b[0]).abs().max())
    diff_u8 = int((a[1].int() - b[1].int()).abs().max())
    del a, b
    t = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            t[name].append(timeit(fn, launches))
            MANIFEST[-1].update(name='render/' + name, shape=[])
    line = {'bench': 'render', 'shape': [B, 2, h, w], 'out_hw': [H, W], 'bytes_fused': bytes_fused, 'bytes_composed': bytes_composed,
            'max_abs_diff_flow': diff_flow, 'max_abs_diff_u8': diff_u8}
    for name, v in t.items():
        key = name.split()[0]
        line.update({key + '_us': statistics.median(v), key + '_us_min': min(v), key + '_us_max': max(v)})
        print('render %-14s %9.1f us (%.1f .. %.1f)' % (name, statistics.median(v), min(v), max(v)), flush=True)
    # the device's share of the fused call: HIP events around each entry point (AF.start_kernel_timing), 20 calls after the warm-up
    from arflow_amd import functional as AF
    AF.start_kernel_timing()
    for _ in range(launches):
        fused()
    per_call = {name: statistics.median(ms) * 1e3 for (name, _), ms in AF.stop_kernel_timing().items()}
    line['entry_point_us'] = per_call
    dev_us = sum(per_call.values())
    for name, us in per_call.items():
        print('render   %-20s %7.1f us between events' % (name, us), flush=True)
    gbs = bytes_fused / line['fused_us'] / 1e3
    line.update(fused_gbs=gbs, fused_fraction_of_hbm_peak=gbs / HBM_PEAK_GBS, hbm_peak_gbs=HBM_PEAK_GBS,
                composed_over_fused=line['composed_us'] / line['fused_us'], entry_points_us=dev_us,
                entry_points_gbs=bytes_fused / dev_us / 1e3)
    print('render composed / fused = %.2f   fused %.0f GB/s = %.1f%% of HBM peak   bytes %.1f MB against %.1f MB   (max |diff| flow '
          '%.1e, picture %d levels)' % (line['composed_over_fused'], gbs, 100 * gbs / HBM_PEAK_GBS, bytes_fused / 1e6,
                                        bytes_composed / 1e6, diff_flow, diff_u8), flush=True)
    with open(jsonl, 'a') as out:
        out.write(json.dumps(line) + '\n')


def optim_bench(dev, jsonl, launches=20, repeats=5):
    """arflow_amd.optim.FlatOptimizer.step() (one launch; two with the clip) on the parameters of
    PWCProbFlow [2,2,0] (5,909,172 elements) under the train section of configs/chairs_uflow_elbo.json, next to what TrainStep
    does today on the same flat gradient buffer: torch.optim.Adam(fused=True), plus torch.nn.utils.clip_grad_norm_ for the clip
    case.  HIP events around `launches` calls after 5 warm-ups, the legs in alternation, `repeats` rounds: median (min .. max).
    Algorithmic bytes: 7 x 4 N for the step (p, m, v read and written, g read), 4 N more for the norm."""
    import statistics
    from arflow_amd.config import AttrDict
    from arflow_amd.ddp import FlatGradAllReduce
    from arflow_amd.models import get_model
    from arflow_amd.optim import FlatOptimizer
    STREAM_GBS = 6300.0  # what a plain device-to-device stream reaches of the 8 TB/s peak (tools/copy_bw.py measures it)
    mcfg = AttrDict(type='uflow_prob', feature_norm=True, level_dropout=0.1, out_channels=[2, 2, 0], inv_cov=False, n_pyramids=1,
                    mixture_weights=False)
    train = dict(optim='adam', lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-6, bias_decay=0.0)
    cpu = torch.Generator().manual_seed(0)
    with open(jsonl, 'a') as out:
        for tag, clip in (('adam, clip off', -1.0), ('adam, clip 1.0', 1.0)):
            legs = {}
            for name in ('fused', 'torch'):
                torch.manual_seed(0)
                model = get_model(mcfg)
                model.init_weights()
                model.to(dev)
                reducer = FlatGradAllReduce(model)
                reducer.flat.copy_(1e-3 * torch.randn(reducer.flat.numel(), generator=torch.Generator().manual_seed(1)))
                if name == 'fused':
                    opt = FlatOptimizer(reducer, AttrDict(dict(train, clip=clip)))
                    legs[name] = (opt.step, model, reducer, opt)
                else:
                    params = list(model.parameters())
                    opt = torch.optim.Adam(params, fused=True, lr=train['lr'], betas=(0.9, 0.999), eps=1e-8)

                    def torch_step(params=params, opt=opt, clip=clip):
                        if clip > 0:
                            torch.nn.utils.clip_grad_norm_(params, clip)
                        opt.step()
                    legs[name] = (torch_step, model, reducer, opt)
            n = legs['fused'][2].flat.numel()
            nbytes = 4 * n * (8 if clip > 0 else 7)
            t = {name: [] for name in legs}
            for _ in range(repeats):
                for name, leg in legs.items():
                    t[name].append(timeit(leg[0], launches))
                    MANIFEST[-1].update(name='optim/' + name, shape=[n])
            line = {'bench': 'optim', 'case': tag, 'model': 'PWCProbFlow [2,2,0]', 'elements': n, 'tensors': len(legs['fused'][2]._spans),
                    'table_rows': int(legs['fused'][3]._table.shape[0]), 'algorithmic_bytes': nbytes, 'launches': launches, 'rounds': repeats}
            for name, v in t.items():
                line.update({name + '_us': statistics.median(v), name + '_us_min': min(v), name + '_us_max': max(v)})
                print('optim %-18s %-8s %9.1f us (%.1f .. %.1f)' % (tag, name, statistics.median(v), min(v), max(v)), flush=True)
            gbs = nbytes / line['fused_us'] / 1e3
            line.update(fused_gbs=gbs, stream_gbs=STREAM_GBS, fused_fraction_of_stream=gbs / STREAM_GBS,
                        torch_over_fused=line['torch_us'] / line['fused_us'])
            print('optim %-18s torch / fused = %.2f   fused %.0f GB/s = %.1f%% of the %.0f GB/s a stream reaches   (%d elements, %d rows)'
                  % (tag, line['torch_over_fused'], gbs, 100 * gbs / STREAM_GBS, STREAM_GBS, n, line['table_rows']), flush=True)
            out.write(json.dumps(line) + '\n')


def penalty_em_bench(dev, jsonl, m=3000000, init_vars=None, launches=20, repeats=5):
    """one EM.update() at the script's size (m = 3e6 fp32 samples, k = 10, x1 = 1) on the fused pass
    (arflow_em_stats + arflow_em_fold + the k-sized torch ops) next to the reference's formulation -- the methods of class EM of
    train_penalty_em.py transcribed here as torch float64 device ops, the m x k matrix xi materialised -- and log_gmm forward +
    backward at 8 x 1 x 384 x 640 (fp32) next to its torch composition.  HIP events around `launches` calls after 5 warm-ups, the
    legs in alternation, `repeats` rounds: median (min .. max).  Algorithmic bytes: the update reads x0 and x1 once (8 m); log_gmm
    reads x twice and the upstream gradient once and writes out and gx (5 x 4 n).  `pass` is update_xi's two launches alone: the
    difference to `fused` is the k-sized torch ops (digamma, lgamma, the M-step, the objective: launch-bound)."""
    import math
    import statistics
    from arflow_amd import penalty_em as P
    init_vars = list(P.INIT_VARS) if init_vars is None else init_vars
    k = len(init_vars)
    cpu = torch.Generator().manual_seed(0)
    scale = torch.tensor([0.05, 0.5, 3.0])[torch.arange(m) % 3]
    x0 = (torch.randn(m, generator=cpu) * scale).to(dev)
    x1 = torch.ones_like(x0)

    class TorchEM:  # the reference's EM, its operations in its order, float64 on the device
        def __init__(self):
            f64 = dict(device=dev, dtype=torch.float64)
            self.alpha, self.mu_0, self.beta_0, self.a, self.b = torch.ones(k, **f64), 0, 1e-3, 1, 1
            self.mu, self.beta = torch.zeros(k, **f64), 1 / torch.tensor(init_vars, **f64)
            self.alpha_bar = self.alpha.clone()

        def update(self, x):
            x0, x1 = x[0].double(), x[1].double()
            log_pi = torch.special.digamma(self.alpha_bar) - torch.special.digamma(torch.sum(self.alpha_bar, dim=0, keepdim=True))
            arg = -self.beta[None, :] * ((x0[:, None] - self.mu[None, :]) ** 2) / 2 + log_pi[None, :]
            num = torch.sqrt(self.beta)[None, :] * torch.exp(arg - torch.max(arg, dim=1, keepdim=True).values)
            xi = num / torch.sum(num, dim=1, keepdim=True)
            self.alpha_bar = self.alpha + torch.sum(x1[:, None] * xi, dim=0)
            self.pi = self.alpha_bar / torch.sum(self.alpha_bar, dim=0, keepdim=True)
            num = 2 * self.a - 1 + torch.sum(xi * x1[:, None], dim=0)
            den = 2 * self.b + self.beta_0 * (self.mu - self.mu_0) ** 2 + torch.sum(xi * x1[:, None] * (x0[:, None] - self.mu[None, :]) ** 2, dim=0)
            self.beta = num / den
            sum_i = torch.sum(xi * x1[:, None] * (torch.log(self.beta)[None, :] - math.log(2 * math.pi)
                              - self.beta[None, :] * (x0[:, None] - self.mu[None, :]) ** 2) / 2 - x1[:, None] * torch.xlogy(xi, xi), dim=0)
            sum_j = torch.sum((self.a - 1 / 2) * torch.log(self.beta) - (self.beta_0 * self.beta * (self.mu - self.mu_0) ** 2) / 2
                              - self.b * self.beta + sum_i)
            return sum_j + torch.sum(torch.lgamma(self.alpha_bar)) - torch.lgamma(torch.sum(self.alpha_bar))

    def one_update(cls, x):
        def run():
            em = cls()  # every call starts from the initial state: the same arithmetic each time
            return em.update(x), em.beta
        return run
    fused_em = lambda: P.EM(k=k, init_vars=init_vars, device=dev)  # noqa: E731
    em0 = fused_em()
    logw0 = em0._logw().contiguous()
    # `pass`: the two launches of update_xi alone (arflow_em_stats + arflow_em_fold), without the k-sized torch ops around them
    legs = {'fused': one_update(fused_em, [x0, None]), 'fused_x1': one_update(fused_em, [x0, x1]), 'torch': one_update(TorchEM, [x0, x1]),
            'pass': lambda: P.em_stats(x0, None, logw0, em0.beta, em0.mu), 'pass_x1': lambda: P.em_stats(x0, x1, logw0, em0.beta, em0.mu)}
    n = 8 * 1 * 384 * 640
    lx = (3.0 * torch.randn(8, 1, 384, 640, generator=cpu)).to(dev)
    pi = torch.full((k,), 1.0 / k, dtype=torch.float64)
    beta = 1 / torch.tensor(init_vars, dtype=torch.float64)

    def torch_log_gmm(x):
        p, b = pi.to(x.device, x.dtype), beta.to(x.device, x.dtype)
        arg = -b * torch.square(x).unsqueeze(-1) / 2
        w = p * torch.sqrt(b) / math.sqrt(2 * math.pi)
        c = torch.max(arg, dim=-1).values
        return c + torch.log(torch.sum(w * torch.exp(arg - c.unsqueeze(-1)), dim=-1))

    def node(fn):
        def run():
            x = lx.clone().requires_grad_(True)
            fn(x).sum().backward()
            return x.grad
        return run
    lg_legs = {'fused': node(lambda x: P.log_gmm(x, pi, beta)), 'torch': node(torch_log_gmm)}
    with open(jsonl, 'a') as out:
        for bench, fns, nbytes, extra in (('update', legs, 8 * m, {'m': m, 'k': k, 'partials': -(-m // P.em_share(m))}),
                                          ('log_gmm fwd+bwd', lg_legs, 20 * n, {'shape': [8, 1, 384, 640], 'k': k})):
            a, b = fns['fused'](), fns['torch']()
            if bench == 'update':
                diff = max(abs(float(a[0]) - float(b[0])) / abs(float(b[0])), float(((a[1] - b[1]).abs() / b[1]).max()))
            else:
                diff = float((a - b).abs().max())
            del a, b
            t = {name: [] for name in fns}
            for _ in range(repeats):
                for name, fn in fns.items():
                    t[name].append(timeit(fn, launches))
                    MANIFEST[-1].update(name='penalty_em/%s/%s' % (bench, name), shape=[])
            line = dict({'bench': 'penalty_em', 'case': bench, 'algorithmic_bytes': nbytes, 'launches': launches, 'rounds': repeats,
                         'max_diff_fused_vs_torch': diff}, **extra)
            for name, v in t.items():
                line.update({name + '_us': statistics.median(v), name + '_us_min': min(v), name + '_us_max': max(v)})
                print('penalty_em %-16s %-9s %9.1f us (%.1f .. %.1f)' % (bench, name, statistics.median(v), min(v), max(v)), flush=True)
            gbs = nbytes / line['fused_us'] / 1e3
            line.update(fused_gbs=gbs, fused_fraction_of_hbm_peak=gbs / HBM_PEAK_GBS, torch_over_fused=line['torch_us'] / line['fused_us'])
            if bench == 'update':  # the pass alone: bytes per second and float64 exp evaluations per nanosecond (k per sample)
                line.update(pass_gbs=4 * m / line['pass_us'] / 1e3, pass_x1_gbs=8 * m / line['pass_x1_us'] / 1e3,
                            pass_exp_per_ns=k * m / line['pass_us'] / 1e3)
            print('penalty_em %-16s torch / fused = %.2f   fused %.0f GB/s = %.1f%% of HBM peak   (difference %.1e)'
                  % (bench, line['torch_over_fused'], gbs, 100 * gbs / HBM_PEAK_GBS, diff), flush=True)
            out.write(json.dumps(line) + '\n')


ELBO_PENALTY_BASE = dict(type='uflow_elbo', edge_constant=150, edge_asymp=0.01, w_smooth=4.0, penalty_smooth='charbonnier',
                         closed_form_smooth=False, data_loss=['census'], data_weight=[1.0], data_penalty=['abs_robust_loss'],
                         w_entropy=0.1, w_oof=0.0, w_occ=0.0, with_bk=True, approx='diag', cov_supp=0, inv_cov=False,
                         approx_entropy=False, occ_type='sample', n_samples=4, offdiag_reg=0.0, natural_grad=False)


def elbo_penalty_inputs(dev, B=8, M=96, N=160, seed=7):
    """the loss case of band_bench at approx 'diag': two [B,4,M,N] level-2 outputs (mean 1.5 N(0,1), log-std -1 + 0.3 N(0,1))
    and a uniform-noise image pair at 4M x 4N, from a generator of their own"""
    g = torch.Generator(device=dev).manual_seed(seed)
    nets = [torch.cat((1.5 * torch.randn(B, 2, M, N, device=dev, generator=g), -1 + 0.3 * torch.randn(B, 2, M, N, device=dev, generator=g)),
                      1).requires_grad_(True) for _ in range(2)]
    ims = [torch.rand(B, 3, 4 * M, 4 * N, device=dev, generator=g) for _ in range(2)]
    return nets, ims


def elbo_penalty_bench(dev, jsonl, B=8, S=4, M=96, N=160, launches=20, repeats=5, settle=40):
    """one UFlowElboLoss step (forward + backward to the level-2 outputs) at the shape of band_bench's loss
    case (B = 8, S = 4, 384 x 640, a 96 x 160 level 2), approx 'diag', with
      default   abs_robust_loss + charbonnier (the unchanged path: one-launch backward),
      gmm       the ten-component mixtures of the reference's chairs_uflow_elbo_gmm.json for both penalties (the penalised pair
                forward, arflow_smooth_pen_fwd / _bwd, two-launch backward),
      torch     the same objective composed without the penalised kernels: the differentiable warp and census distance nodes,
                -log_gmm on the distance map, the squared-mixture torch node on torch-made flow differences.
    `settle` untimed calls of every leg, then HIP events around `launches` steps after 5 warm-ups, the legs in alternation,
    `repeats` rounds: median (min .. max).  With --tree DIR (another checkout, e.g. the parent commit's, built) only the default
    leg runs, on that checkout's package, and the line carries tree = DIR's last component; the comparison (a) of the default
    step at two commits is two such invocations writing to one --jsonl file."""
    import statistics
    from arflow_amd import functional as AF, uflow_utils as U
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    nets, ims = elbo_penalty_inputs(dev, B, M, N)
    H, W = 4 * M, 4 * N
    eps = tuple(torch.randn(S * B, 2, M, N, device=dev, generator=torch.Generator(device=dev).manual_seed(11 + d)) for d in (0, 1))

    def run(loss):
        out = loss({'flows_fw': [None, None, nets[0]], 'flows_bw': [None, None, nets[1]]}, ims[0], ims[1], eps=eps)
        return out, torch.autograd.grad(out[0], nets)

    def measure(legs, line):
        for fn in legs.values():  # (launch-bound steps: the host time of a call settles after some tens of calls, as in band_bench)
            for _ in range(settle):
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name in legs}
        for _ in range(repeats):
            for name, fn in legs.items():
                t[name].append(timeit(fn, launches))
                MANIFEST[-1].update(name='elbo_penalty/' + name, shape=[B, S, H, W])
        for name, v in t.items():
            line.update({name + '_us': statistics.median(v), name + '_us_min': min(v), name + '_us_max': max(v)})
            print('elbo_penalty %-8s %9.1f us (%.1f .. %.1f)' % (name, statistics.median(v), min(v), max(v)), flush=True)
        return line
    default = get_loss(AttrDict(dict(ELBO_PENALTY_BASE, n_samples=S)))
    line = {'bench': 'elbo_penalty', 'tree': os.path.basename(TREE) if TREE else 'this', 'shape': [B, S, H, W], 'approx': 'diag',
            'launches': launches, 'rounds': repeats}
    if TREE:
        import arflow_amd
        assert os.path.abspath(arflow_amd.__file__).startswith(TREE + os.sep), arflow_amd.__file__
        with open(jsonl, 'a') as out_file:
            out_file.write(json.dumps(measure({'default': lambda: run(default)}, line)) + '\n')
        return
    from arflow_amd.losses.penalty_functions import get_penalty
    from tests import elbo_penalty_ref as PR
    gmm_cfg = dict(ELBO_PENALTY_BASE, n_samples=S, data_penalty=['gmm'], penalty_smooth='gmm', **PR.GMM_KEYS)
    losses = {'default': default, 'gmm': get_loss(AttrDict(gmm_cfg))}
    pen_data = get_penalty('gmm', pi=PR.CENSUS_PI, beta=PR.CENSUS_BETA)
    pen_smooth = get_penalty('gmm', pi=PR.SMOOTH_PI, beta=PR.SMOOTH_BETA, squared=True)
    cfg = AttrDict(gmm_cfg)

    def composed():
        """the objective of the 'gmm' leg on the unpenalised nodes (data + sampled smoothness - entropy)"""
        total = 0.
        rep = lambda t: t.repeat(S, 1, 1, 1)  # noqa: E731
        z = [rep(n[:, 0:2]) + rep(torch.exp(n[:, 2:4])) * e for n, e in zip(nets, eps)]
        for d in (0, 1):
            im_a, im_b = rep(ims[d]), rep(ims[d ^ 1])
            f0 = AF.interpolate_flow(z[d], 4, False)
            recons, valid = AF.warp_with_valid(im_b, f0, pad='zeros', align_corners=True, norm=AF.NORM_UFLOW)
            mask = AF.up4_clamp_mul(AF.splat_map(z[d ^ 1], 0), valid)
            pm = torch.nn.functional.pad(mask[:, :, 3:-3, 3:-3], (3, 3, 3, 3))
            ham = AF.TernaryDistFunction.apply(im_a, recons, 3)
            total = total + cfg.data_weight[0] * (pen_data(ham) * pm).sum() / (pm.sum() + 1e-6)
            small = rep(AF.down4(ims[d]))
            gx, gy = U.image_grads(small)
            wx = cfg.edge_asymp + (1 - cfg.edge_asymp) * torch.exp(-torch.mean(torch.abs(cfg.edge_constant * gx), 1, keepdim=True))
            wy = cfg.edge_asymp + (1 - cfg.edge_asymp) * torch.exp(-torch.mean(torch.abs(cfg.edge_constant * gy), 1, keepdim=True))
            dx, dy = U.image_grads(z[d])
            total = total + (wx / 2 * cfg.w_smooth * pen_smooth(dx ** 2)).mean() + (wy / 2 * cfg.w_smooth * pen_smooth(dy ** 2)).mean()
            total = total - cfg.w_entropy * nets[d][:, 2:4].sum(1).mean()
        return total

    def torch_step():
        torch.autograd.grad(composed(), nets)
    legs = {'default': lambda: run(losses['default']), 'gmm': lambda: run(losses['gmm']), 'torch': torch_step}
    (out, grads), ref = run(losses['gmm']), composed()
    diff = abs(float(out[0].detach()) - float(ref.detach())) / abs(float(ref.detach()))
    gdiff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads, torch.autograd.grad(ref, nets)))
    AF.start_kernel_timing()
    run(losses['gmm'])
    calls = AF.stop_kernel_timing()
    line.update(k=len(PR.CENSUS_PI), total_rel_diff_gmm_vs_torch=diff, grad_rel_diff_gmm_vs_torch=gdiff,
                gmm_library_launches=sorted({n for n, _ in calls}))
    measure(legs, line)
    line.update(gmm_over_default=line['gmm_us'] / line['default_us'], torch_over_gmm=line['torch_us'] / line['gmm_us'])
    print('elbo_penalty gmm / default = %.3f   torch / gmm = %.2f   (total differs by %.1e, gradients by %.1e of their maximum)'
          % (line['gmm_over_default'], line['torch_over_gmm'], diff, gdiff), flush=True)
    with open(jsonl, 'a') as out_file:
        out_file.write(json.dumps(line) + '\n')


def main():
    if os.environ.get('ARFLOW_LIB_PATH'):  # an alternative build of the library (A/B timing; tools only)
        _lib.LIB_PATH = os.environ['ARFLOW_LIB_PATH']
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--filter', default='')
    ap.add_argument('--tree', default='', help='another checkout of the project to import arflow_amd from (see TREE above)')
    ap.add_argument('--levels', default='uflow')
    ap.add_argument('--batch', type=int, default=16, help='model-side batch (2B: both directions stacked)')
    ap.add_argument('--size', type=int, nargs=2, default=[384, 640])
    ap.add_argument('--jsonl', default='', help='--filter augment, optim, ar, penalty_em and elbo_penalty append their result lines here '
                    '(default: profiles/augment_kbench.jsonl, profiles/optim_kbench.jsonl, profiles/ar_kbench.jsonl, '
                    'profiles/penalty_em_kbench.jsonl, profiles/elbo_penalty_kbench.jsonl)')
    ap.add_argument('--manifest', default='', help='write the ordered (name, shape, calls) list of the timed ops here')
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device('cuda')
    s = torch.cuda.current_stream().cuda_stream
    global _marker
    _marker = lambda tag: lib.arflow_profile_marker(int(tag), s)
    H0, W0 = args.size
    B2 = args.batch
    if args.levels == 'uflow':
        levels = [(32, H0 // 32, W0 // 32), (32, H0 // 16, W0 // 16), (32, H0 // 8, W0 // 8), (32, H0 // 4, W0 // 4)]
    else:
        levels = [(192, H0 // 64, W0 // 64), (128, H0 // 32, W0 // 32), (96, H0 // 16, W0 // 16),
                  (64, H0 // 8, W0 // 8), (32, H0 // 4, W0 // 4)]
    g = torch.Generator(device='cuda').manual_seed(0)
    rows = []

    def rec(name, shape, us):
        nb = algorithmic_bytes(name, shape)
        gbs = nb / us / 1e3
        rows.append((name, shape, us, gbs))
        MANIFEST[-1].update(name=name, shape=list(shape), us=us)  # the segment timeit() has just run
        print('%-22s %-26s %9.1f us %9.1f GB/s  %5.1f%% of HBM peak' % (name, list(shape), us, gbs, 100 * gbs / HBM_PEAK_GBS), flush=True)

    def want(n):
        # a token in EXACT_FILTERS is a substring of other ops' names ('ar' of 'warp'): it selects the bench of that name only
        return any(f == n if f in EXACT_FILTERS else f in n for f in args.filter.split('|'))

    for C, h, w in levels:
        x1 = torch.randn(B2, C, h, w, device=dev, generator=g)
        x2 = torch.randn(B2, C, h, w, device=dev, generator=g)
        out = torch.empty(B2, 81, h, w, device=dev)
        go = torch.randn(B2, 81, h, w, device=dev, generator=g)
        g1, g2 = torch.empty_like(x1), torch.empty_like(x2)
        fl = 2.0 * torch.randn(B2, 2, h, w, device=dev, generator=g)
        wout = torch.empty_like(x1)
        gfl = torch.empty_like(fl)
        planes = lib.arflow_corr_sign_planes(C, w, 4)
        sign = torch.zeros(B2, planes, h, w, device=dev, dtype=torch.int32) if planes else None
        if want('corr_fwd') or want('corr_bwd'):
            rec('arflow_corr_fwd', (B2, C, h, w, 4, planes), timeit(lambda: lib.arflow_corr_fwd(p(x1), p(x2), p(out), p(sign), B2, C, h, w, 4, 0.1, s), args.iters))
        if want('corr_bwd'):
            rec('arflow_corr_bwd', (B2, C, h, w, 4, planes or 81), timeit(lambda: lib.arflow_corr_bwd(p(go), None if planes else p(out), p(sign), p(x1), p(x2), p(g1), p(g2), B2, C, h, w, 4, 0.1, s), args.iters))
        if want('warp_fwd'):
            rec('arflow_warp_fwd', (B2, C, h, w), timeit(lambda: lib.arflow_warp_fwd(p(x2), p(fl), p(wout), None, B2, C, h, w, h, w, 2 * h * w, 0, 1, 0, s), args.iters))
        if want('warp_bwd'):
            rec('arflow_warp_bwd', (B2, C, h, w, True), timeit(lambda: lib.arflow_warp_bwd(p(x1), p(x2), p(fl), p(g2), p(gfl), B2, C, h, w, h, w, 2 * h * w, 0, 1, 0, s), args.iters))
        if want('featnorm'):
            n = C * h * w
            acc = torch.empty(4 * (2048 + B2), device=dev, dtype=torch.float64)
            stt = torch.empty(B2, 4, device=dev)
            rec('arflow_featnorm_fwd', (B2, n), timeit(lambda: lib.arflow_featnorm_fwd(p(x1), p(x2), p(g1), p(g2), p(acc), p(stt), B2, n, 0, s), args.iters))
            rec('arflow_featnorm_bwd', (B2, n), timeit(lambda: lib.arflow_featnorm_bwd(p(x1), p(x2), p(x1), p(x2), p(stt), p(acc), p(g1), p(g2), B2, n, 0, s), args.iters))
        if want('level'):
            has_flow = (h, w) != (levels[0][1], levels[0][2])
            fc = 0.7 * torch.randn(B2, 2, h // 2, w // 2, device=dev, generator=g) if has_flow else None
            ctot = 81 + C + 2 + 32
            buf = torch.zeros(B2, ctot, h, w, device=dev)
            gbuf = torch.randn(B2, ctot, h, w, device=dev, generator=g)
            bs = ctot * h * w
            fup, x2w = torch.empty(B2, 2, h, w, device=dev), torch.empty_like(x2)
            lsign = torch.zeros(B2, 3, h, w, device=dev, dtype=torch.int32)
            lstats = torch.empty(B2, 4, device=dev)
            lacc = torch.empty(4 * B2 * lib.arflow_level_acc_rows(B2, C, h, w, int(has_flow)), device=dev, dtype=torch.float64)
            ws = torch.empty(lib.arflow_level_bwd_ws_bytes(B2, C, h, w), device=dev, dtype=torch.uint8)
            gfc = torch.empty(B2, 2, h // 2, w // 2, device=dev)
            gext = torch.randn(B2, 2, h, w, device=dev, generator=g)
            vol, x1n, fslot = buf[:, :81], buf[:, 81:81 + C], buf[:, 81 + C:]
            fk = 2 if has_flow else 0

            def lfwd():
                lib.arflow_level_fwd(p(x1), p(x2), p(fc), 2 * (h // 2) * (w // 2), int(has_flow), 1, p(fup) if has_flow else None,
                                     fslot.data_ptr() if has_flow else None, bs, p(x2w) if has_flow else None, 0, vol.data_ptr(), bs,
                                     x1n.data_ptr(), bs, p(lsign), p(lstats), p(lacc), B2, C, h, w, 4, 0.1, 0, 1, 0, s)

            def lbwd():
                lib.arflow_level_bwd(gbuf[:, :81].data_ptr(), bs, p(lsign), x1n.data_ptr(), bs, gbuf[:, 81:].data_ptr(), bs, p(x1),
                                     p(x2), p(x2w) if has_flow else None, p(fup) if has_flow else None, 2 * h * w,
                                     gbuf[:, 81 + C:].data_ptr() if has_flow else None, bs, p(gext) if has_flow else None,
                                     p(lstats), 0, p(g1), p(g2), p(gfc) if has_flow else None, int(has_flow), 1, p(ws), B2, C, h,
                                     w, 4, 0.1, 0, 1, 0, s)
            # the form the models call (arflow_level_fwd_m): the maps' moments come from the conv epilogue that produced them
            mrows = lib.arflow_bias_act_mom_rows(C, h * w)
            bias0 = torch.zeros(C, device=dev)
            r1 = torch.empty(B2, mrows, 2, device=dev, dtype=torch.float64)
            r2 = torch.empty(B2, mrows, 2, device=dev, dtype=torch.float64)
            lib.arflow_bias_act_fwd_mom(p(x1), p(bias0), p(x1), p(r1), B2, C, h * w, 1.0, s)  # slope 1, bias 0: x unchanged
            lib.arflow_bias_act_fwd_mom(p(x2), p(bias0), p(x2), p(r2), B2, C, h * w, 1.0, s)

            def lfwd_m():
                lib.arflow_level_fwd_m(p(x1), p(x2), p(fc), 2 * (h // 2) * (w // 2), int(has_flow), 1, p(fup) if has_flow else None,
                                       fslot.data_ptr() if has_flow else None, bs, p(x2w) if has_flow else None, 0, vol.data_ptr(), bs,
                                       x1n.data_ptr(), bs, p(lsign), p(lstats), p(lacc), p(r1), mrows, None if has_flow else p(r2),
                                       0 if has_flow else mrows, B2, C, h, w, 4, 0.1, 0, 1, 0, s)
            rec('arflow_level_fwd', (B2, C, h, w, 4, 3, fk), timeit(lfwd, args.iters))
            rec('arflow_level_fwd_m', (B2, C, h, w, 4, 3, fk, 1), timeit(lfwd_m, args.iters))
            rec('arflow_level_bwd', (B2, C, h, w, 4, 3, fk), timeit(lbwd, args.iters))
    if want('headconv'):  # the two-channel flow heads of the flagship (csrc/headconv.hip); tools/headconv_miopen.py times MIOpen's
        for C, h, w in ((595, H0 // 4, W0 // 4), (595, H0 // 8, W0 // 8), (595, H0 // 16, W0 // 16), (563, H0 // 32, W0 // 32),
                        (32, H0 // 4, W0 // 4)):
            x = torch.randn(B2, C, h, w, device=dev, generator=g)
            wt = 0.05 * torch.randn(2, C, 3, 3, device=dev, generator=g)
            bias = torch.randn(2, device=dev, generator=g)
            y, dy = torch.empty(B2, 2, h, w, device=dev), torch.randn(B2, 2, h, w, device=dev, generator=g)
            dx, dw, db = torch.empty_like(x), torch.empty_like(wt), torch.empty_like(bias)
            ws = torch.empty(lib.arflow_headconv_bwd_weight_ws_bytes(B2, C, h, w), device=dev, dtype=torch.uint8)
            wide = 4 * B2 * h * w * (C + 2)  # the wide tensor once plus the two-channel side; weights are noise

            def hrec(name, us):
                MANIFEST[-1].update(name=name, shape=[B2, C, h, w], us=us)
                print('%-22s %-26s %9.1f us %9.1f GB/s  %5.1f%% of HBM peak' % (name, [B2, C, h, w], us, wide / us / 1e3, 100 * wide / us / 1e3 / HBM_PEAK_GBS), flush=True)
            hrec('arflow_headconv_fwd', timeit(lambda: lib.arflow_headconv_fwd(p(x), p(wt), p(bias), p(y), B2, C, h, w, s), args.iters))
            hrec('arflow_headconv_bwd_data', timeit(lambda: lib.arflow_headconv_bwd_data(p(dy), p(wt), p(dx), B2, C, h, w, s), args.iters))
            hrec('arflow_headconv_bwd_weight', timeit(lambda: lib.arflow_headconv_bwd_weight(p(x), p(dy), p(dw), p(db), p(ws), B2, C, h, w, s), args.iters))
            del x, dx, ws
    if want('splitconv'):  # the wide 3x3 layers on the split-bf16 kernel (csrc/splitconv.hip) next to MIOpen's call, same buffers
        import torch.nn.functional as F
        conv_args = ([1, 1], [1, 1], [1, 1], False, [0, 0], 1)
        layers = ((147, 128), (275, 128), (403, 96), (499, 64), (563, 32), (597, 128), (64, 32))
        U = 2.0 ** -24

        def sc_call(x, wt, packed, y, tf):
            N, C, h, w = x.shape
            K = y.shape[1]
            lib.arflow_splitconv_pack(p(wt), p(packed), wt.shape[0], wt.shape[1], tf, s)
            return lib.arflow_splitconv_fwd(p(x), p(packed), p(y), N, C, K, h, w, s)

        def spread(fn):  # three rounds of --iters: (median, min, max) in us
            ts = sorted(timeit(fn, args.iters) for _ in range(3))
            MANIFEST[-1].update(name='splitconv', shape=[], us=ts[1])
            return ts[1], ts[0], ts[2]

        def err_vs_float64(Cl, Kl, h, w):
            """e = max |err| / S against float64 on the CPU, S the same operation on absolute values; inputs mean 3, std 1; one
            sample at this resolution (the chain length is set by the channels).  -> (fwd kernel, fwd MIOpen, dgrad kernel, dgrad MIOpen)"""
            gc = torch.Generator().manual_seed(Cl * 1000 + Kl)
            x, wt, gy = (3.0 + torch.randn(*sh, generator=gc) for sh in ((1, Cl, h, w), (Kl, Cl, 3, 3), (1, Kl, h, w)))
            ref_y = F.conv2d(x.double(), wt.double(), None, 1, 1)
            s_y = F.conv2d(x.double().abs(), wt.double().abs(), None, 1, 1)
            wT = wt.transpose(0, 1).flip(2, 3).double()
            ref_dx, s_dx = F.conv2d(gy.double(), wT, None, 1, 1), F.conv2d(gy.double().abs(), wT.abs(), None, 1, 1)
            xd, wd, gd = x.to(dev), wt.to(dev), gy.to(dev)
            pk = torch.empty(lib.arflow_splitconv_pack_bytes(max(Cl, Kl), max(Cl, Kl)), device=dev, dtype=torch.uint8)
            y, dx = torch.empty(1, Kl, h, w, device=dev), torch.empty(1, Cl, h, w, device=dev)
            assert sc_call(xd, wd, pk, y, 0) == 0 and sc_call(gd, wd, pk, dx, 1) == 0
            ym = F.conv2d(xd, wd, None, 1, 1)
            dxm = torch.ops.aten.convolution_backward(gd, xd, wd, None, *conv_args, [True, False, False])[0]
            e = lambda got, ref, sc: float(((got.double().cpu() - ref).abs() / sc).max()) / U
            return e(y, ref_y, s_y), e(ym, ref_y, s_y), e(dx, ref_dx, s_dx), e(dxm, ref_dx, s_dx)

        print('splitconv: time in us as median (min .. max) of 3 x %d calls; kernel = pack + forward; TF = fp32-equivalent TFLOP/s of the kernel' % args.iters)
        for _, h, w in levels[::-1]:
            for Cl, Kl in layers:
                x = torch.randn(B2, Cl, h, w, device=dev, generator=g)
                gy = torch.randn(B2, Kl, h, w, device=dev, generator=g)
                wt = 0.05 * torch.randn(Kl, Cl, 3, 3, device=dev, generator=g)
                y, dx = torch.empty_like(gy), torch.empty_like(x)
                pk = torch.empty(lib.arflow_splitconv_pack_bytes(max(Cl, Kl), max(Cl, Kl)), device=dev, dtype=torch.uint8)
                assert sc_call(x, wt, pk, y, 0) == 0 and sc_call(gy, wt, pk, dx, 1) == 0
                flop = 2.0 * B2 * h * w * Cl * Kl * 9
                for what, mine, theirs in (
                        ('fwd  ', lambda: sc_call(x, wt, pk, y, 0), lambda: F.conv2d(x, wt, None, 1, 1)),
                        ('dgrad', lambda: sc_call(gy, wt, pk, dx, 1),
                         lambda: torch.ops.aten.convolution_backward(gy, x, wt, None, *conv_args, [True, False, False]))):
                    a, b = spread(mine), spread(theirs)
                    cin, cout = (Cl, Kl) if what == 'fwd  ' else (Kl, Cl)
                    for k, m in enumerate(MANIFEST[-6:]):  # the six segments above: tools/pmc_kernels.py finds the layer by them
                        m.update(name='splitconv/%s %s' % ('kernel' if k < 3 else 'miopen', what.strip()), shape=[B2, cin, cout, h, w])
                    print('splitconv %s %-22s kernel %8.1f (%8.1f .. %8.1f)  MIOpen %8.1f (%8.1f .. %8.1f)  %5.2fx  %6.1f TF' % (
                        what, [B2, cin, cout, h, w], a[0], a[1], a[2], b[0], b[1], b[2], b[0] / a[0], flop / a[0] / 1e6), flush=True)
                del x, gy, y, dx
        h, w = levels[0][1], levels[0][2]
        for Cl, Kl in layers:
            print('splitconv error %4d->%-4d at 1x%dx%d: fwd %6.2f / %6.2f u   dgrad %6.2f / %6.2f u   (kernel / MIOpen, u = 2^-24)' % (
                (Cl, Kl, h, w) + err_vs_float64(Cl, Kl, h, w)), flush=True)
    if want('dense_inplace'):  # the five dense layers at the top level as the in-place estimator calls them
        conv_args = ([1, 1], [1, 1], [1, 1], False, [0, 0], 1)
        _, h, w = levels[-1]
        hw = h * w

        def di_spread(fn):  # three rounds of --iters: (median, min, max) in us
            ts = sorted(timeit(fn, args.iters) for _ in range(3))
            MANIFEST[-1].update(name='dense_inplace', shape=[], us=ts[1])
            return ts[1], ts[0], ts[2]
        print('dense_inplace: time in us as median (min .. max) of 3 x %d calls.  fwd = arflow_splitconv_pack + arflow_splitconv_fwd on packed '
              'tensors; fwd_ex = pack + arflow_splitconv_fwd_ex reading x6[:, K:] and writing lrelu(conv + b) into x6[:, :K]; wgrad: our '
              'kernel reading the slice in place | MIOpen on the slice (ATen copies it contiguous first) | MIOpen on a packed x' % args.iters)
        for Cl, Kl in ((147, 128), (275, 128), (403, 96), (499, 64), (563, 32)):
            x6 = torch.randn(B2, Kl + Cl, h, w, device=dev, generator=g)
            xs = x6[:, Kl:]
            x = xs.contiguous()
            gy = 3.0 + torch.randn(B2, Kl, h, w, device=dev, generator=g)
            wt = 0.05 * torch.randn(Kl, Cl, 3, 3, device=dev, generator=g)
            bias = torch.randn(Kl, device=dev, generator=g)
            y, dw = torch.empty_like(gy), torch.empty_like(wt)
            pk = torch.empty(lib.arflow_splitconv_pack_bytes(Kl, Cl), device=dev, dtype=torch.uint8)
            ws = torch.empty(lib.arflow_splitconv_wgrad_ws_bytes(B2, Cl, Kl, h, w), device=dev, dtype=torch.uint8)
            bs = (Kl + Cl) * hw

            def plain():
                lib.arflow_splitconv_pack(p(wt), p(pk), Kl, Cl, 0, s)
                return lib.arflow_splitconv_fwd(p(x), p(pk), p(y), B2, Cl, Kl, h, w, s)

            def ex():
                lib.arflow_splitconv_pack(p(wt), p(pk), Kl, Cl, 0, s)
                return lib.arflow_splitconv_fwd_ex(p(xs), bs, p(pk), p(x6), bs, p(bias), 1, 0.1, B2, Cl, Kl, h, w, s)

            def ex_packed():  # the epilogue alone: packed tensors
                lib.arflow_splitconv_pack(p(wt), p(pk), Kl, Cl, 0, s)
                return lib.arflow_splitconv_fwd_ex(p(x), Cl * hw, p(pk), p(y), Kl * hw, p(bias), 1, 0.1, B2, Cl, Kl, h, w, s)

            def ex_plain():  # the strides alone: slice in, slot out, plain store
                lib.arflow_splitconv_pack(p(wt), p(pk), Kl, Cl, 0, s)
                return lib.arflow_splitconv_fwd_ex(p(xs), bs, p(pk), p(x6), bs, None, 0, 0.0, B2, Cl, Kl, h, w, s)

            def wg():
                return lib.arflow_splitconv_wgrad(p(xs), bs, p(gy), Kl * hw, p(dw), p(ws), B2, Cl, Kl, h, w, s)
            assert plain() == 0 and ex() == 0 and ex_packed() == 0 and ex_plain() == 0 and wg() == 0
            a, b, b1, b2 = di_spread(plain), di_spread(ex), di_spread(ex_packed), di_spread(ex_plain)
            tag = '%-24s' % [B2, Cl, Kl, h, w]
            print('dense_inplace fwd    %s %8.1f (%8.1f .. %8.1f)' % ((tag,) + a), flush=True)
            print('dense_inplace fwd_ex %s %8.1f (%8.1f .. %8.1f)   %+6.1f us against fwd' % ((tag,) + b + (b[0] - a[0],)), flush=True)
            print('dense_inplace fwd_ex %s %8.1f (%8.1f .. %8.1f)   %+6.1f us  packed tensors, epilogue on' % ((tag,) + b1 + (b1[0] - a[0],)), flush=True)
            print('dense_inplace fwd_ex %s %8.1f (%8.1f .. %8.1f)   %+6.1f us  slice in, slot out, plain store' % ((tag,) + b2 + (b2[0] - a[0],)), flush=True)
            c = di_spread(wg)
            d = di_spread(lambda: torch.ops.aten.convolution_backward(gy, xs, wt, None, *conv_args, [False, True, False]))
            e = di_spread(lambda: torch.ops.aten.convolution_backward(gy, x, wt, None, *conv_args, [False, True, False]))
            print('dense_inplace wgrad  %s kernel %8.1f (%8.1f .. %8.1f) | MIOpen + copy %8.1f (%8.1f .. %8.1f) | MIOpen packed %8.1f '
                  '(%8.1f .. %8.1f) | kernel - (MIOpen + copy) %+7.1f us' % ((tag,) + c + d + e + (c[0] - d[0],)), flush=True)
            del x6, xs, x, gy, ws
    if want('splitconv_wgrad'):  # the wide layers' weight gradient (csrc/splitconv_wgrad.hip) next to MIOpen's call, same buffers
        conv_args = ([1, 1], [1, 1], [1, 1], False, [0, 0], 1)
        layers = ((147, 128), (275, 128), (403, 96), (499, 64), (563, 32), (597, 128), (64, 32))
        U = 2.0 ** -24

        def wg_spread(fn):  # three rounds of --iters: (median, min, max) in us
            ts = sorted(timeit(fn, args.iters) for _ in range(3))
            MANIFEST[-1].update(name='splitconv_wgrad', shape=[], us=ts[1])
            return ts[1], ts[0], ts[2]

        def wg_call(x, gy, dw, ws):
            N, C, h, w = x.shape
            return lib.arflow_splitconv_wgrad(p(x), C * h * w, p(gy), gy.shape[1] * h * w, p(dw), p(ws), N, C, gy.shape[1], h, w, s)

        print('splitconv_wgrad: time in us as median (min .. max) of 3 x %d calls; kernel = partial sums + finish; MIOpen = '
              'aten.convolution_backward [False, True, False] with the layout copies it launches; TF = fp32-equivalent TFLOP/s of the kernel' % args.iters)
        for _, h, w in levels[::-1]:
            for Cl, Kl in layers:
                x = 3.0 + torch.randn(B2, Cl, h, w, device=dev, generator=g)
                gy = 3.0 + torch.randn(B2, Kl, h, w, device=dev, generator=g)
                wt = torch.empty(Kl, Cl, 3, 3, device=dev)
                dw = torch.empty_like(wt)
                ws = torch.empty(lib.arflow_splitconv_wgrad_ws_bytes(B2, Cl, Kl, h, w), device=dev, dtype=torch.uint8)
                assert wg_call(x, gy, dw, ws) == 0
                flop = 2.0 * B2 * h * w * Cl * Kl * 9
                a = wg_spread(lambda: wg_call(x, gy, dw, ws))
                b = wg_spread(lambda: torch.ops.aten.convolution_backward(gy, x, wt, None, *conv_args, [False, True, False]))
                print('splitconv_wgrad %-24s kernel %8.1f (%8.1f .. %8.1f)  MIOpen %8.1f (%8.1f .. %8.1f)  %5.2fx  %6.1f TF' % (
                    [B2, Cl, Kl, h, w], a[0], a[1], a[2], b[0], b[1], b[2], b[0] / a[0], flop / a[0] / 1e6), flush=True)
                if (h, w) == (levels[-1][1], levels[-1][2]):  # the full reduction, once: e against float64 on the CPU
                    # over the first 8 x 8 channel pairs: the same reduction length at 1/1000 of the float64 work
                    xd, gd = x[:, :8].double().cpu(), gy[:, :8].double().cpu()
                    w0 = torch.zeros(8, 8, 3, 3, dtype=torch.float64, requires_grad=True)
                    ref = torch.autograd.grad(torch.nn.functional.conv2d(xd, w0, None, 1, 1), w0, gd)[0]
                    sc = torch.autograd.grad(torch.nn.functional.conv2d(xd.abs(), w0, None, 1, 1), w0, gd.abs())[0]
                    e = lambda t: float(((t[:8, :8].double().cpu() - ref).abs() / sc).max()) / U
                    lib_e = max(e(torch.ops.aten.convolution_backward(gy, x, wt, None, *conv_args, [False, True, False])[1]) for _ in range(2))
                    print('splitconv_wgrad error %4d->%-4d at %dx%dx%d (%d terms): dw %6.2f / %6.2f u   (kernel / MIOpen, u = 2^-24)' % (
                        Cl, Kl, B2, h, w, B2 * h * w, e(dw), lib_e), flush=True)
                del x, gy, ws
    if want('dilated'):  # the context network's dilated layers as phase mosaics (csrc/phase.hip)
        import statistics
        from arflow_amd import functional as AF
        _, h, w = levels[-1]
        real = (B2, h, w)

        def alternate(fns, rounds=5):  # {name: fn} -> {name: (median, min, max)} us; one window each per round, in alternation
            t = {name: [] for name in fns}
            for _ in range(rounds):
                for name, fn in fns.items():
                    t[name].append(timeit(fn, args.iters))
                    MANIFEST[-1].update(name='dilated ' + name, shape=[], us=t[name][-1])
            return {name: (statistics.median(v), min(v), max(v)) for name, v in t.items()}

        fmt = lambda v: '%8.1f (%8.1f .. %8.1f)' % v
        print('dilated: time in us as median (min .. max) of 5 x %d calls in alternation at %dx%dx%d; kernel = this tree on the virtual '
              'tensors (forward and data gradient: pack + convolution with its epilogue), MIOpen = the ATen call with the layout copies '
              'it launches; TF = fp32-equivalent TFLOP/s of the REAL convolution' % (args.iters, B2, h, w))
        for Cl, Kl, d in AF.DILATED_CHAIN_LAYERS:
            cargs = ([1, 1], [d, d], [d, d], False, [0, 0], 1)
            x = 3.0 + torch.randn(B2, Cl, h, w, device=dev, generator=g)
            gy = 3.0 + torch.randn(B2, Kl, h, w, device=dev, generator=g)
            wt = torch.randn(Kl, Cl, 3, 3, device=dev, generator=g)
            bias = torch.randn(Kl, device=dev, generator=g)
            xv, gv = AF.phase_move(x, real, 1, d)[0], AF.phase_move(gy, real, 1, d)[0]
            flop = 2.0 * B2 * h * w * Cl * Kl * 9
            tag = '%3d->%-3d d %-2d %s' % (Cl, Kl, d, 'x'.join(map(str, xv.shape[0:1] + xv.shape[2:])))
            for name, ours, theirs in (
                    ('fwd  ', lambda: AF.splitconv(xv, wt, bias=bias, slope=0.1), lambda: torch.ops.aten.convolution(x, wt, None, *cargs)),
                    ('dgrad', lambda: AF.splitconv(gv, wt, transpose_flip=True),
                     lambda: torch.ops.aten.convolution_backward(gy, x, wt, None, *cargs, [True, False, False])),
                    ('wgrad', lambda: AF.splitconv_wgrad(xv, gv),
                     lambda: torch.ops.aten.convolution_backward(gy, x, wt, None, *cargs, [False, True, False]))):
                r = alternate({'kernel': ours, 'MIOpen': theirs})
                print('dilated %s %s kernel %s  MIOpen %s  %5.2fx  %6.1f TF  %s' % (
                    name, tag, fmt(r['kernel']), fmt(r['MIOpen']), r['MIOpen'][0] / r['kernel'][0], flop / r['kernel'][0] / 1e6,
                    'kernel max < MIOpen min' if r['kernel'][2] < r['MIOpen'][1] else 'ranges touch'), flush=True)
            del x, gy, xv, gv
        # the permutation passes, next to the passes they replace; GB/s = one read (two for act_bwd) + the writes of the REAL map
        chain = [(128, 1, 2), (128, 2, 4), (128, 4, 8), (96, 8, 16), (64, 16, 1)]
        for Cl, da, db in chain:
            t = torch.randn(B2, Cl, h, w, device=dev, generator=g)
            t2 = torch.randn(B2, Cl, h, w, device=dev, generator=g)
            sv, yv = AF.phase_move(t, real, 1, da)[0], AF.phase_move(t2, real, 1, da)[0]
            o1, o2 = AF._phase_empty(B2, Cl, h, w, db, dev), AF._phase_empty(B2, Cl, h, w, 1, dev)
            bvec = torch.randn(Cl, device=dev, generator=g)
            gb = torch.empty(Cl, device=dev)
            nbytes = 4.0 * B2 * Cl * h * w
            r = alternate({
                'move': lambda: AF.phase_move(sv, real, da, db, out=o1),
                'move+2nd': lambda: AF.phase_move(sv, real, da, db, 1, out=o1, out2=o2),
                'bias_act_fwd': lambda: lib.arflow_bias_act_fwd(p(t), p(bvec), p(t), B2, Cl, h * w, 0.1, s),
                'act_bwd': lambda: AF.phase_act_bwd(sv, yv, real, da, db, 0, 0.1),
                'act_bwd+2nd': lambda: AF.phase_act_bwd(sv, yv, real, da, db, 1, 0.1),
                'bias_act_bwd': lambda: lib.arflow_bias_act_bwd(p(t), p(t2), p(o2), p(gb), B2, Cl, h * w, 0.1, s)})
            passes = {'move': 2, 'move+2nd': 3, 'bias_act_fwd': 2, 'act_bwd': 3, 'act_bwd+2nd': 4, 'bias_act_bwd': 3}
            for name, v in r.items():
                print('dilated pass %3d ch  %2d -> %-2d  %-13s %s us  %7.1f GB/s  %4.1f%% of HBM peak' % (
                    Cl, da, db, name, fmt(v), passes[name] * nbytes / v[0] / 1e3, 100 * passes[name] * nbytes / v[0] / 1e3 / HBM_PEAK_GBS), flush=True)
            del t, t2, sv, yv, o1, o2
    if want('dense'):  # the dense estimator's concatenating epilogue and gradient gather (csrc/dense.hip), five layers x four levels
        import ctypes
        from arflow_amd.functional import _DenseSrc
        ocs = (128, 128, 96, 64, 32)
        for li, (_, h, w) in enumerate(levels[-4:]):
            hw = h * w
            cin = 115 if li == 0 else 147  # volume 81 + features 32 + flow 2 (+ 32 upsampled context channels below the top)
            plane = 4 * B2 * hw

            def drec(name, shape, us, planes):
                MANIFEST[-1].update(name=name, shape=list(shape), us=us)
                gbs = planes * plane / us / 1e3
                print('%-22s %-26s %9.1f us %9.1f GB/s  %5.1f%% of HBM peak  (%d planes)' % (name, list(shape), us, gbs, 100 * gbs / HBM_PEAK_GBS, planes), flush=True)
            # the yardstick of the same run: the in-place epilogue and its backward at 128 channels
            t = torch.randn(B2, 128, h, w, device=dev, generator=g)
            t2, t3 = torch.randn(B2, 128, h, w, device=dev, generator=g), torch.empty(B2, 128, h, w, device=dev)
            b128, gb128 = torch.randn(128, device=dev, generator=g), torch.empty(128, device=dev)
            drec('arflow_bias_act_fwd', (B2, 128, hw), timeit(lambda: lib.arflow_bias_act_fwd(p(t), p(b128), p(t), B2, 128, hw, 0.1, s), args.iters), 2 * 128)
            drec('arflow_bias_act_bwd', (B2, 128, hw), timeit(lambda: lib.arflow_bias_act_bwd(p(t2), p(t), p(t3), p(gb128), B2, 128, hw, 0.1, s), args.iters), 3 * 128)
            del t, t2, t3
            chans = [cin + sum(ocs[:k]) for k in range(6)]  # channels of x_1 .. x_6
            G = [torch.randn(B2, chans[5], h, w, device=dev, generator=g) for _ in range(2)]  # gradient of x_6, the head's data gradient
            DX = {k: torch.randn(B2, chans[k - 1], h, w, device=dev, generator=g) for k in range(2, 6)}  # dx_k: gradient of x_k
            DX[1] = torch.randn(B2, cin, h, w, device=dev, generator=g)
            for m in range(1, 6):
                C, oc = chans[m - 1], ocs[m - 1]
                y = torch.randn(B2, oc, h, w, device=dev, generator=g)
                x = torch.randn(B2, C, h, w, device=dev, generator=g)
                bias = torch.randn(oc, device=dev, generator=g)
                out = torch.empty(B2, oc + C, h, w, device=dev)
                drec('arflow_dense_cat_fwd', (B2, oc, C, hw), timeit(lambda: lib.arflow_dense_cat_fwd(p(y), p(bias), p(x), p(out), B2, oc, C, hw, 0.1, s), args.iters), 2 * (oc + C))
                srcs = [(G[0], sum(ocs[m:5])), (G[1], sum(ocs[m:5]))] + [(DX[k], sum(ocs[m:k - 1])) for k in range(5, m, -1)]
                arr = (_DenseSrc * len(srcs))()
                for j, (tt, off) in enumerate(srcs):
                    arr[j].ptr, arr[j].bstride, arr[j].scale = tt.data_ptr() + 4 * off * hw, tt.shape[1] * hw, None
                gy = torch.empty(B2, oc, h, w, device=dev)
                rows = torch.empty(lib.arflow_dense_gbias_rows(B2, hw), oc, device=dev)
                drec('arflow_dense_grad_gather', (B2, oc, hw, len(srcs), 1), timeit(lambda: lib.arflow_dense_grad_gather(
                    ctypes.cast(arr, ctypes.c_void_p), len(srcs), p(out), (oc + C) * hw, p(gy), p(rows), B2, oc, hw, 0.1, s), args.iters), oc * (len(srcs) + 2))
                del y, x, out, gy
            srcs = [(G[0], sum(ocs)), (G[1], sum(ocs))] + [(DX[k], sum(ocs[:k - 1])) for k in range(5, 0, -1)]
            arr = (_DenseSrc * len(srcs))()
            for j, (tt, off) in enumerate(srcs):
                arr[j].ptr, arr[j].bstride, arr[j].scale = tt.data_ptr() + 4 * off * hw, tt.shape[1] * hw, None
            gx = torch.empty(B2, cin, h, w, device=dev)
            drec('arflow_dense_grad_gather', (B2, cin, hw, len(srcs), 0), timeit(lambda: lib.arflow_dense_grad_gather(
                ctypes.cast(arr, ctypes.c_void_p), len(srcs), None, 0, p(gx), None, B2, cin, hw, 0.1, s), args.iters), cin * (len(srcs) + 1))
            del G, DX, gx
    # loss side: B = batch/2 image pairs at full resolution, per direction
    B = max(1, B2 // 2)
    im1 = torch.rand(B, 3, H0, W0, device=dev, generator=g)
    im2 = torch.rand(B, 3, H0, W0, device=dev, generator=g)
    mask = torch.ones(B, 1, H0, W0, device=dev)
    fl0 = 2.0 * torch.randn(B, 2, H0, W0, device=dev, generator=g)
    fl2 = 1.0 * torch.randn(B, 2, H0 // 4, W0 // 4, device=dev, generator=g)
    rec3 = torch.empty_like(im1)
    dham = torch.empty(B, 1, H0, W0, device=dev)
    sums = torch.empty(4 * lib.arflow_sums_rows(B, H0, W0), device=dev)  # rows of the largest problem timed below
    gfl0 = torch.empty_like(fl0)
    sm = torch.empty(B, 3, H0 // 4, W0 // 4, device=dev)
    coef = torch.ones(2, device=dev)
    gfl2 = torch.empty_like(fl2)
    one = torch.ones(1, device=dev)
    if want('warp_fwd'):
        rec('arflow_warp_fwd', (B, 3, H0, W0), timeit(lambda: lib.arflow_warp_fwd(p(im2), p(fl0), p(rec3), None, B, 3, H0, W0, H0, W0, 2 * H0 * W0, 0, 1, 1, s), args.iters))
    if want('warp_bwd'):
        rec('arflow_warp_bwd', (B, 3, H0, W0, False), timeit(lambda: lib.arflow_warp_bwd(p(im1), p(im2), p(fl0), None, p(gfl0), B, 3, H0, W0, H0, W0, 2 * H0 * W0, 0, 1, 1, s), args.iters))
    if want('census_fwd'):
        rec('arflow_census_fwd', (B, H0, W0), timeit(lambda: lib.arflow_census_fwd(p(im1), p(im2), p(mask), None, p(dham), p(sums), B, H0, W0, 3, s), args.iters))
    if want('census_bwd'):
        rec('arflow_census_bwd', (B, H0, W0), timeit(lambda: lib.arflow_census_bwd(p(im1), p(im2), p(dham), p(one), p(rec3), B, H0, W0, 3, s), args.iters))
    if want('census_warp'):
        occ = torch.rand(B, 1, H0 // 4, W0 // 4, device=dev, generator=g) * 1.5
        maskw = torch.empty(B, 1, H0, W0, device=dev)
        gr1, gr2 = torch.empty(B, 1, H0, W0, device=dev), torch.empty(B, 1, H0, W0, device=dev)
        rec('arflow_down4_gray', (B, H0, W0), timeit(lambda: lib.arflow_down4_gray(p(im1), p(sm), p(gr1), B, H0, W0, s), args.iters))
        _marker(len(MANIFEST))  # an untimed launch: its own (nameless) segment
        MANIFEST.append({'name': None, 'shape': None, 'calls': 1})
        lib.arflow_down4_gray(p(im2), None, p(gr2), B, H0, W0, s)
        # a smooth flow (x4 bilinear upsample of a 2 px field, what the models emit) next to the white-noise one
        fls = torch.nn.functional.interpolate(fl2 * 2, scale_factor=4, mode='bilinear', align_corners=False).contiguous()
        rec('arflow_census_warp_fwd', (B, H0, W0, 'smooth'), timeit(lambda: lib.arflow_census_warp_fwd(p(gr1), p(gr2), p(fls), 2 * H0 * W0, p(occ), p(maskw), p(dham), p(sums), B, H0, W0, 3, s), args.iters))
        rec('arflow_census_warp_bwd', (B, H0, W0, 'smooth'), timeit(lambda: lib.arflow_census_warp_bwd(p(gr1), p(gr2), p(fls), 2 * H0 * W0, p(dham), p(one), p(gfl0), B, H0, W0, 3, s), args.iters))
        rec('arflow_census_warp_fwd', (B, H0, W0), timeit(lambda: lib.arflow_census_warp_fwd(p(gr1), p(gr2), p(fl0), 2 * H0 * W0, p(occ), p(maskw), p(dham), p(sums), B, H0, W0, 3, s), args.iters))
        rec('arflow_census_warp_bwd', (B, H0, W0), timeit(lambda: lib.arflow_census_warp_bwd(p(gr1), p(gr2), p(fl0), 2 * H0 * W0, p(dham), p(one), p(gfl0), B, H0, W0, 3, s), args.iters))
    if want('pair'):  # UFlowLoss as bench.py runs it: both directions as ONE batch of 2B = --batch samples (sample s = 2 b + direction)
        B2p = B2
        imgs = torch.rand(B2p, 3, H0, W0, device=dev, generator=g)
        smallp = torch.empty(B2p, 3, H0 // 4, W0 // 4, device=dev)
        grayp = torch.empty(B2p, 1, H0, W0, device=dev)
        occp = torch.empty(B2p, 1, H0 // 4, W0 // 4, device=dev)
        fl2p = 1.0 * torch.randn(B2p, 2, H0 // 4, W0 // 4, device=dev, generator=g)
        fl0p = torch.nn.functional.interpolate(fl2p * 4, scale_factor=4, mode='bilinear', align_corners=False).contiguous()
        dhamp = torch.empty(B2p, 1, H0, W0, device=dev)
        maskp = torch.empty(B2p, 1, H0, W0, device=dev)
        sump = torch.empty(4 * lib.arflow_sums_rows(B2p, H0, W0), device=dev)
        sums2 = torch.empty(4 * lib.arflow_sums_rows(B2p, H0 // 4, W0 // 4), device=dev)
        gf0p, gf2p = torch.empty_like(fl0p), torch.empty_like(fl2p)
        sc2, cf2 = torch.ones(2, device=dev), torch.ones(2, device=dev)
        h4, w4 = H0 // 4, W0 // 4
        rec('arflow_down4_gray_z', (B2p, H0, W0), timeit(lambda: lib.arflow_down4_gray_z(p(imgs), p(smallp), p(grayp), p(occp), B2p, H0, W0, s), args.iters))
        # (the range map keeps accumulating over the timed calls -- it is cleared by arflow_down4_gray_z in a step; same work)
        rec('arflow_splat_smooth_fwd', (B2p, 3, h4, w4), timeit(lambda: lib.arflow_splat_smooth_fwd(p(fl2p), p(smallp), p(occp), p(sums2), B2p, h4, w4, 2 * h4 * w4, 1.0, 150.0, 1, 1, 1, 1, s), args.iters))
        rec('arflow_census_warp_pair_fwd', (B2p, H0, W0), timeit(lambda: lib.arflow_census_warp_pair_fwd(p(grayp), p(fl0p), 2 * H0 * W0, p(occp), p(maskp), p(dhamp), p(sump), B2p, H0, W0, 3, s), args.iters))
        rec('arflow_uflow_pair_bwd', (B2p, H0, W0), timeit(lambda: lib.arflow_uflow_pair_bwd(p(grayp), p(fl0p), 2 * H0 * W0, p(dhamp), p(sc2), p(gf0p), B2p, H0, W0, 3, p(fl2p), 2 * h4 * w4, p(smallp), p(cf2), p(gf2p), h4, w4, 1.0, 150.0, 1, 1, 1, s), args.iters))
    if want('photo_fwd'):
        rec('arflow_photo_fwd', (B, 3, H0, W0), timeit(lambda: lib.arflow_photo_fwd(p(im1), p(im2), p(mask), None, p(sums), B, 3, H0, W0, s), args.iters))
    if want('photo_bwd'):
        rec('arflow_photo_bwd', (B, 3, H0, W0), timeit(lambda: lib.arflow_photo_bwd(p(im1), p(im2), p(mask), None, p(coef), p(rec3), B, 3, H0, W0, s), args.iters))
    if want('splat'):
        rec('arflow_splat_map', (B, H0 // 4, W0 // 4), timeit(lambda: lib.arflow_splat_map(p(fl2), p(dham), B, H0 // 4, W0 // 4, 2 * (H0 // 4) * (W0 // 4), 0, s), args.iters))
    if args.levels == 'pwclite':  # unFlowLoss works at full resolution
        if want('smooth_fwd'):
            rec('arflow_smooth_fwd', (B, 3, H0, W0), timeit(lambda: lib.arflow_smooth_fwd(p(fl0), p(im1), p(sums), B, 3, H0, W0, 2 * H0 * W0, 1.0 / 384, 10.0, 1, 0, 0, s), args.iters))
        if want('smooth_bwd'):
            rec('arflow_smooth_bwd', (B, 3, H0, W0), timeit(lambda: lib.arflow_smooth_bwd(p(fl0), p(im1), p(coef), p(gfl0), B, 3, H0, W0, 2 * H0 * W0, 1.0 / 384, 10.0, 1, 0, 0, s), args.iters))
        if want('splat_map'):
            rec('arflow_splat_map', (B, H0, W0), timeit(lambda: lib.arflow_splat_map(p(fl0), p(dham), B, H0, W0, 2 * H0 * W0, 1, s), args.iters))
    if want('smooth_fwd'):
        rec('arflow_smooth_fwd', (B, 3, H0 // 4, W0 // 4), timeit(lambda: lib.arflow_smooth_fwd(p(fl2), p(sm), p(sums), B, 3, H0 // 4, W0 // 4, 2 * (H0 // 4) * (W0 // 4), 1.0, 150.0, 1, 1, 1, s), args.iters))
    if want('smooth_bwd'):
        rec('arflow_smooth_bwd', (B, 3, H0 // 4, W0 // 4), timeit(lambda: lib.arflow_smooth_bwd(p(fl2), p(sm), p(coef), p(gfl2), B, 3, H0 // 4, W0 // 4, 2 * (H0 // 4) * (W0 // 4), 1.0, 150.0, 1, 1, 1, s), args.iters))
    if want('down4'):
        rec('arflow_down4', (B * 3, H0, W0), timeit(lambda: lib.arflow_down4(p(im1), p(sm), B * 3, H0, W0, s), args.iters))
    if want('up4'):
        rec('arflow_up4_clamp_mul', (B, H0 // 4, W0 // 4), timeit(lambda: lib.arflow_up4_clamp_mul(p(sm), p(mask), p(dham), B, H0 // 4, W0 // 4, s), args.iters))
    if want('triag'):  # the sparse triangular solves (csrc/triag.hip) at the 1/4-resolution grid of the flagship: 2 * batch * nsamples planes
        for P, M, N in ((16, H0 // 4, W0 // 4), (64, H0 // 4, W0 // 4), (16, H0 // 16, W0 // 16), (64, H0 // 16, W0 // 16)):
            A = torch.exp(0.4 * torch.randn(1, P, M, N, device=dev, generator=g))
            Bc, Cc, Dc = [0.6 * torch.rand(1, P, M - i, N - j, device=dev, generator=g) - 0.3 for i, j in ((0, 1), (1, 0), (1, 1))]
            X = torch.randn(1, P, M, N, device=dev, generator=g)
            Y, gX, gA, gB, gC, gD = [torch.empty_like(t) for t in (X, X, A, Bc, Cc, Dc)]
            steps = -(-M // 64) * (N + 63)  # the dependent chain

            def trec(name, us, floats):
                MANIFEST[-1].update(name=name, shape=[P, M, N], us=us)
                gbs = 4 * floats / us / 1e3
                print('%-22s %-26s %9.1f us %9.1f GB/s  %5.1f%% of HBM peak  (%d dependent steps, %.0f ns each)' % (
                    name, [P, M, N], us, gbs, 100 * gbs / HBM_PEAK_GBS, steps, 1e3 * us / steps), flush=True)
            if (M, N) == (H0 // 4, W0 // 4):  # the solves at the small grid are launch-bound: not timed
                for upper in (0, 1):
                    trec('arflow_triag_solve' + ('/upper' if upper else ''), timeit(lambda: lib.arflow_triag_solve(
                        p(A), p(Bc), p(Cc), p(Dc), p(X), p(Y), P, M, N, upper, s), args.iters), 6 * P * M * N)
                trec('arflow_triag_solve_bwd', timeit(lambda: lib.arflow_triag_solve_bwd(
                    p(A), p(Bc), p(Cc), p(Dc), p(Y), p(X), p(gX), p(gA), p(gB), p(gC), p(gD), P, M, N, 0, s), args.iters), 11 * P * M * N)
            trec('arflow_triag_inverse_diagonal', timeit(lambda: lib.arflow_triag_inverse_diagonal(
                p(A), p(Bc), p(Cc), p(gA), P, M, N, s), max(3, args.iters // 10)), 4 * P * M * N)
    if want('lowrank'):  # the low-rank sampler and Gram log-determinant (csrc/lowrank.hip) against the torch formulation
        lowrank_bench(dev, g)
    if want('mixture'):  # the mixture sampler + log-density node (csrc/mixture.hip) against the torch formulation
        mixture_bench(dev, g)
    if want('band'):  # the fused sparse-covariance sampler (csrc/band.hip) against the reference's formulation in torch ops
        band_bench(dev, g)
    if want('out_up'):  # the probabilistic model's output upsample (csrc/upsample.hip) against the composed ATen path, and the rest of the upsample family alone
        out_up_bench(dev, g)
    if want('gauss_pyr'):  # the pyramid sampler node and one ElboLoss step (csrc/gauss_pyr.hip) against the torch formulation
        gauss_pyr_bench(dev, g)
    if want('mse'):  # one MseLoss step on the fused residual kernels (csrc/mse.hip) against the composed ATen formulation
        mse_bench(dev, g)
    if want('augment'):  # the batch augmentation (csrc/augment.hip) against the same transform composed of ATen operations
        augment_bench(dev, args.jsonl or os.path.join(ROOT, 'profiles', 'augment_kbench.jsonl'))
    if want('optim'):  # the fused optimiser step (csrc/optim.hip) against torch.optim.Adam(fused=True) on the same flat buffer
        optim_bench(dev, args.jsonl or os.path.join(ROOT, 'profiles', 'optim_kbench.jsonl'))
    if want('ar'):  # the AR transform and loss (csrc/ar.hip) against the same arithmetic composed of ATen operations
        ar_bench(dev, args.jsonl or os.path.join(ROOT, 'profiles', 'ar_kbench.jsonl'))
    if want('render'):  # restore + stats + flow picture (csrc/render.hip) against the same outputs composed of ATen operations
        render_bench(dev, args.jsonl or os.path.join(ROOT, 'profiles', 'render_kbench.jsonl'))
    if want('penalty_em'):  # one EM update and log_gmm (csrc/penalty_em.hip) against the reference's formulation in torch ops
        penalty_em_bench(dev, args.jsonl or os.path.join(ROOT, 'profiles', 'penalty_em_kbench.jsonl'))
    if want('elbo_penalty'):  # one UFlowElboLoss step: default penalties, the fitted mixtures, and the mixtures composed of unpenalised nodes
        elbo_penalty_bench(dev, args.jsonl or os.path.join(ROOT, 'profiles', 'elbo_penalty_kbench.jsonl'))
    if args.manifest:
        json.dump(MANIFEST, open(args.manifest, 'w'), indent=1)
    if not rows:  # only ops that keep their own byte model (the head convolutions) were selected
        return
    tot_us = sum(r[2] for r in rows)
    tot_b = sum(algorithmic_bytes(r[0], r[1]) for r in rows)
    print(json.dumps({'kernels': len(rows), 'sum_us': tot_us, 'sum_GB': tot_b / 1e9, 'aggregate_GBps': tot_b / tot_us / 1e3,
                      'aggregate_frac_of_hbm_peak': tot_b / tot_us / 1e3 / HBM_PEAK_GBS}))


if __name__ == '__main__':
    main()
