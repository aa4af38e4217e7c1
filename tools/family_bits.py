#!/usr/bin/env python
"""Bit fingerprints of the variational-family entry points, of the metric launchers that share their plumbing (DESIGN.md
section 29) and of the bilinear upsamples (family out_up: every entry point of csrc/upsample.hip):
for every entry point, plane, layout and family parameter the inputs come from a CPU generator with a fixed seed, the raw C-ABI call runs once, and every output tensor, the float64 work and rows buffers included, is fingerprinted
by the first 12 hex digits of the sha256 of its bytes.  One line per entry point, parameters and plane:

    name parameters plane  tensor[shape] contig=<hash> slice=<hash> offset1=<hash>  tensor[shape] ...

Two builds compute the same thing iff their outputs of this tool are equal line for line:

    python tools/family_bits.py > after.txt
    python tools/family_bits.py --root <checkout of another commit, built> > parent.txt

Only the C ABI is used (_lib, functional._call), so the tool runs unchanged against any build of the same ABI version.
Planes (per item): 1x1; 3x5 (under a wave, scalar); 8x8 (one wave, vector); 5x52 (260 pixels: past one 256-thread
workgroup, vector); 25x41 (1025: past one 1024-pixel chunk, scalar); 32x36 (1152: past one chunk, vector).  Layouts:
contiguous; channel slices of a tensor one channel wider; a view that starts one float into a larger buffer (the base is
misaligned, so the scalar kernel must be chosen even where the plane is a multiple of 4).  B = 2 throughout.

Two families have shapes of their own instead of the planes and layouts: `featnorm` (csrc/featnorm.hip on
every launch path) and `level` (the fused pyramid level, forward and backward); their lines start with the entry point and its
parameters, and every tensor is dense (`contig`).
"""
import argparse
import ctypes
import hashlib
import math
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--only', default='', help='comma-separated families (lowrank, mixture, band, pyramid, mse, flow_eval, uncert, out_up, '
                'featnorm, level)')
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from arflow_amd import _lib  # noqa: E402
from arflow_amd.functional import _call, _p, _stream  # noqa: E402

PLANES = [(1, 1), (3, 5), (8, 8), (5, 52), (25, 41), (32, 36)]
LAYOUTS = ('contig', 'slice', 'offset1')
B = 2
DEV = torch.device('cuda:0')
GEN = torch.Generator().manual_seed(20240229)
LIB = _lib.load()


def randn(*shape, scale=1.0):
    return scale * torch.randn(*shape, generator=GEN)


def lay(t, layout):
    """The CPU tensor t [n,C,M,N] on the device in `layout` (a view; its batch stride is t.stride(0) of the view)."""
    n, C, M, N = t.shape
    if layout == 'contig':
        return t.to(DEV)
    if layout == 'slice':
        wide = torch.zeros(n, C + 1, M, N, device=DEV)
        v = wide[:, 1:]
    else:
        buf = torch.zeros(t.numel() + 1, device=DEV)
        v = buf[1:].view(n, C, M, N)
    v.copy_(t)
    return v


def out(layout, *shape):
    return lay(torch.zeros(*shape), layout)


ROWS = {}  # (name, params, plane) -> {tensor[shape]: [layout=hash, ...]}, in the order of the calls


def show(name, params, plane, layout, **tensors):
    show_row('%s %s %dx%d' % (name, params, plane[0], plane[1]), layout, **tensors)


def show_row(head, layout, **tensors):
    torch.cuda.synchronize()
    row = ROWS.setdefault(head, {})
    for key, t in tensors.items():
        if t is None:
            continue
        digest = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:12]
        row.setdefault('%s[%s]' % (key, 'x'.join(map(str, t.shape))), []).append('%s=%s' % (layout, digest))


def work(fn, *dims):
    n = getattr(LIB, fn)(*dims)
    _lib.check(min(n, 0), fn)
    return torch.zeros(n, device=DEV, dtype=torch.float64)


def lowrank(plane, layout):
    M, N = plane
    for R in (1, 3, 16):
        for S in (1, 3):
            par = 'R=%d,S=%d' % (R, S)
            mean, std = lay(randn(B, 2, M, N), layout), lay(randn(B, 2 * R, M, N, scale=0.5), layout)
            eps = randn(S * B, 2 * R, 1, 1).to(DEV)
            z = out(layout, S * B, 2, M, N)
            _call('arflow_lowrank_sample_fwd', _p(mean), mean.stride(0), _p(std), std.stride(0), _p(eps), _p(z), z.stride(0), B, S,
                  R, M, N, _stream())
            show('lowrank_sample_fwd', par, plane, layout, z=z)
            gZ, glogdet = lay(randn(S * B, 2, M, N), layout), randn(B, 2).to(DEV)
            ginv = None
            if M * N >= R:  # fewer pixels than columns: the Gram matrix is singular by construction
                wk = work('arflow_lowrank_work_size', B, R, M, N)
                logdet, ginv = torch.zeros(B, 2, device=DEV), torch.zeros(B, 2, R, R, device=DEV)
                _call('arflow_lowrank_logdet_fwd', _p(std), std.stride(0), _p(wk), _p(logdet), _p(ginv), B, R, M, N, _stream())
                show('lowrank_logdet_fwd', par, plane, layout, work=wk, logdet=logdet, ginv=ginv)
            gmean, gstd = out(layout, B, 2, M, N), out(layout, B, 2 * R, M, N)
            _call('arflow_lowrank_bwd', _p(std), std.stride(0), _p(eps), _p(gZ), gZ.stride(0), _p(ginv),
                  _p(glogdet if ginv is not None else None), _p(gmean), gmean.stride(0), _p(gstd), gstd.stride(0), B, S, R, M, N,
                  _stream())
            show('lowrank_bwd', par, plane, layout, gmean=gmean, gstd=gstd)


def mixture(plane, layout):
    M, N = plane
    for K in (2, 4):
        for S in (1, 3):
            par = 'K=%d,S=%d' % (K, S)
            mean, ls = lay(randn(B, 2 * K, M, N), layout), lay(randn(B, 2 * K, M, N, scale=0.3), layout)
            eps = lay(randn(S * B, 2, M, N), layout)
            weights = torch.softmax(randn(B, K), 1).to(DEV)
            comp = torch.randint(0, K, (B, S), generator=GEN).to(DEV)
            flow = out(layout, S * B, 2, M, N)
            wk = work('arflow_mixture_work_size', B, S, K, M, N)
            dims = (B, S, K, M, N, _stream())
            _call('arflow_mixture_sample_fwd', _p(mean), mean.stride(0), _p(ls), ls.stride(0), _p(eps), eps.stride(0), _p(comp),
                  _p(flow), flow.stride(0), _p(wk), *dims)
            logpdf, resp, q = (torch.zeros(*s, device=DEV) for s in ((S * B,), (S * B, K), (S * B, K)))
            _call('arflow_mixture_logpdf_fwd', _p(wk), _p(weights), _p(logpdf), _p(resp), _p(q), *dims)
            show('mixture_sample_fwd', par, plane, layout, flow=flow, work=wk, logpdf=logpdf, resp=resp, q=q)
            gZ, glogpdf = lay(randn(S * B, 2, M, N), layout), randn(S * B).to(DEV)
            gmean, gls = out(layout, B, 2 * K, M, N), out(layout, B, 2 * K, M, N)
            _call('arflow_mixture_bwd', _p(mean), mean.stride(0), _p(ls), ls.stride(0), _p(eps), eps.stride(0), _p(comp), _p(resp),
                  _p(glogpdf), _p(gZ), gZ.stride(0), _p(gmean), gmean.stride(0), _p(gls), gls.stride(0), *dims)
            show('mixture_bwd', par, plane, layout, gmean=gmean, glog_std=gls)
            ent = torch.zeros(B, 1, M, N, device=DEV)
            _call('arflow_mixture_entropy_map', _p(mean), mean.stride(0), _p(ls), ls.stride(0), _p(weights), _p(comp), _p(eps),
                  eps.stride(0), _p(ent), *dims)
            show('mixture_entropy_map', par, plane, layout, out=ent)


def band(plane, layout):
    M, N = plane
    S = 2
    for k in (0, 1, 3):
        ntap = (k + 1) ** 2
        for tr in (0, 1):
            par = 'k=%d,T=%d' % (k, tr)
            mean, diag = lay(randn(B, 2, M, N), layout), lay(randn(B, 2, M, N), layout)
            off = lay(randn(B, 2 * (ntap - 1), M, N), layout) if k else None
            X, Y = lay(randn(S * B, 2, M, N), layout), out(layout, S * B, 2, M, N)
            o_bs = off.stride(0) if k else 0
            _call('arflow_band_mv_fwd', _p(mean), mean.stride(0), _p(diag), diag.stride(0), _p(off), o_bs, _p(X), X.stride(0),
                  _p(Y), Y.stride(0), B, S, M, N, k, tr, _stream())
            show('band_mv_fwd', par, plane, layout, Y=Y)
            gY = lay(randn(S * B, 2, M, N), layout)
            gX, gmean, gdiag = out(layout, S * B, 2, M, N), out(layout, B, 2, M, N), out(layout, B, 2, M, N)
            goff = out(layout, B, 2 * (ntap - 1), M, N) if k else None
            _call('arflow_band_mv_bwd', _p(diag), diag.stride(0), _p(off), o_bs, _p(X), X.stride(0), _p(gY), gY.stride(0), _p(gX),
                  gX.stride(0), _p(gmean), gmean.stride(0), _p(gdiag), gdiag.stride(0), _p(goff), goff.stride(0) if k else 0,
                  B, S, M, N, k, tr, _stream())
            show('band_mv_bwd', par, plane, layout, gX=gX, gmean=gmean, gdiag=gdiag, goff=goff)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[_p(t) for t in ts])


def _longs(v):
    return (ctypes.c_long * len(v))(*v)


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def pyramid(plane, layout):
    for n in (1, 3):
        sizes = [(-(-plane[0] // 2 ** i), -(-plane[1] // 2 ** i)) for i in range(n)]
        nets = [lay(randn(B, 8, h, w, scale=0.5), layout) for h, w in sizes]
        eps = [lay(randn(B, 4, h, w), layout) for h, w in sizes]
        zs = [out(layout, B, 4, h, w) for h, w in sizes]
        hs, ws = _ints([s[0] for s in sizes]), _ints([s[1] for s in sizes])
        wk = work('arflow_gauss_pyr_work_size', hs, ws, n, B)
        ent = torch.zeros(n, 2, device=DEV, dtype=torch.float64)
        bs = lambda ts: _longs([t.stride(0) for t in ts])  # noqa: E731
        _call('arflow_gauss_pyr_sample_fwd', _ptrs(nets), bs(nets), _ptrs(eps), bs(eps), _ptrs(zs), bs(zs), hs, ws, n, B, _p(wk),
              _p(ent), _stream())
        show('gauss_pyr_sample_fwd', 'n=%d' % n, plane, layout, work=wk, ent=ent, **{'z%d' % i: z for i, z in enumerate(zs)})
        gzs = [lay(randn(B, 4, h, w), layout) for h, w in sizes]
        gent = randn(n, 2).double().to(DEV)
        gnets = [out(layout, B, 8, h, w) for h, w in sizes]
        _call('arflow_gauss_pyr_sample_bwd', _ptrs(gzs), bs(gzs), _ptrs(nets), bs(nets), _ptrs(eps), bs(eps), _p(gent),
              _ptrs(gnets), bs(gnets), hs, ws, n, B, _stream())
        show('gauss_pyr_sample_bwd', 'n=%d' % n, plane, layout, **{'gnet%d' % i: g for i, g in enumerate(gnets)})


def mse(plane, layout):
    h, w = plane
    H, W, S = 2 * h + 1, 2 * w + 3, 2
    for mode in (0, 1, 2):
        if mode == 2 and (h < 2 or w < 2):
            continue  # the 4-neighbour mode needs a 2x2 plane
        C = 8 if mode == 2 else 5
        net, tgt = lay(randn(B, C, h, w, scale=0.5), layout), lay(randn(B, 2, H, W, scale=3.0), layout)
        ez = lay(randn(S * B, 2, h, w), layout)
        wk = work('arflow_mse_work_size', B, h, w)
        sums = torch.zeros(4, device=DEV, dtype=torch.float64)
        _call('arflow_mse_fwd', _p(net), net.stride(0), C, _p(tgt), tgt.stride(0), H, W, _p(ez), ez.stride(0), B, S, h, w, mode, 0,
              _p(wk), _p(sums), _stream())
        show('mse_fwd', 'mode=%d' % mode, plane, layout, work=wk, sums=sums)
        gsums = randn(4).double().to(DEV)
        gnet = out(layout, B, C, h, w)
        gz = out(layout, S * B, 2, h, w) if mode == 2 else None
        _call('arflow_mse_bwd', _p(net), net.stride(0), C, _p(tgt), tgt.stride(0), H, W, _p(ez), ez.stride(0), _p(gsums), _p(gnet),
              gnet.stride(0), _p(gz), gz.stride(0) if mode == 2 else 0, B, S, h, w, mode, 0, _stream())
        show('mse_bwd', 'mode=%d' % mode, plane, layout, gnet=gnet, gz=gz)


def _gt(C, H, W, layout):
    gt = randn(B, C, H, W, scale=4.0)
    if C == 4:
        gt[:, 2:] = (torch.rand(B, 2, H, W, generator=GEN) > 0.3).float()
    return lay(gt, layout)


def flow_eval(plane, layout):
    if layout == 'slice':
        return  # the entry point takes dense tensors: no batch stride to vary
    H, W = plane
    h, w = -(-H // 2), -(-W // 2)
    for C in (2, 4):
        pred, gt = randn(B, 2, h, w, scale=2.0).to(DEV), _gt(C, H, W, layout)
        move = lay((torch.rand(B, 1, H, W, generator=GEN) > 0.5).float(), layout) if C == 4 else None
        nrows = LIB.arflow_flow_eval_rows(H, W)
        rows = torch.zeros(B, nrows, 8, device=DEV, dtype=torch.float64)
        epe = out(layout, B, 1, H, W)
        _call('arflow_flow_eval', _p(pred), _p(gt), _p(move), _p(rows), _p(epe), B, h, w, C, H, W, _stream())
        show('flow_eval', 'C=%d' % C, plane, layout, rows=rows, epe_map=epe)


def uncert(plane, layout):
    if layout == 'slice':
        return
    H, W = plane
    h, w = -(-H // 2), -(-W // 2)
    for C in (2, 4):
        par = 'C=%d' % C
        gt = _gt(C, H, W, layout)
        vp, vs = (gt.data_ptr() + 2 * H * W * 4, 4 * H * W) if C == 4 else (None, 0)
        ent, epe = randn(B, 2, h, w).to(DEV), lay(randn(B, 1, H, W).abs(), layout)
        nrows = LIB.arflow_uncert_rows(H, W)
        rows = torch.zeros(B, nrows, 8, device=DEV, dtype=torch.float64)
        ent_map = out(layout, B, 1, H, W)
        shift = [float(torch.tensor(2 * math.log(v), dtype=torch.float32)) for v in (w, W, h, H)]
        _call('arflow_uncert_prep', _p(ent), _p(epe), vp, vs, _p(ent_map), _p(rows), *shift, B, h, w, H, W, _stream())
        show('uncert_prep', par, plane, layout, rows=rows, ent_map=ent_map)
        K = 5
        for F in (1, 2):
            f0, f1 = lay(randn(B, 1, H, W), layout), lay(randn(B, 1, H, W), layout) if F == 2 else None
            thr = randn(B, F, K).double().to(DEV)
            srows = torch.zeros(B, nrows, F, K, 3, device=DEV, dtype=torch.float64)
            _call('arflow_sparsify_sums', _p(epe), _p(f0), _p(f1), vp, vs, _p(thr), 100.0, _p(srows), B, H, W, K, _stream())
            show('sparsify_sums', par + ',F=%d' % F, plane, layout, rows=srows)
        pred, ent2 = lay(randn(B, 2, H, W, scale=2.0), layout), lay(randn(B, 2, H, W, scale=0.7), layout)
        edges = torch.linspace(0.2, 3.0, 7, dtype=torch.float64).to(DEV)
        crows = torch.zeros(B, LIB.arflow_calib_rows(H, W), 8, 3, device=DEV, dtype=torch.float64)
        _call('arflow_calib_hist', _p(pred), _p(gt), _p(ent2), _p(edges), _p(crows), B, C, H, W, 7, _stream())
        show('calib_hist', par, plane, layout, rows=crows)


def signed_zeros(t):
    """t with some entries +0.0 and some -0.0: the bias add of the output upsamples turns a -0.0 tap into +0.0 (also where the
    bias is 0), the flow upsample has no such add and keeps it, so a moved `+ 0.f` shows in the hashes.  All values finite."""
    v = t.view(-1)
    v[::7] = 0.0
    v[3::11] = -0.0
    return t


def out_up(plane, layout):
    h, w = plane
    C, n_flow, n_diag, bias = 4, 2, 1, 0.5
    x = lay(signed_zeros(randn(B, C, h, w)), layout)
    o2 = out(layout, B, C, 2 * h, 2 * w)
    _call('arflow_out_up2_fwd', _p(x), x.stride(0), _p(o2), o2.stride(0), B, C, h, w, n_flow, n_diag, bias, _stream())
    show('out_up2_fwd', 'C=4', plane, layout, out=o2)
    gx = out(layout, B, C, h, w)
    g2 = lay(signed_zeros(randn(B, C, 2 * h, 2 * w)), layout)
    _call('arflow_out_up2_bwd', _p(g2), g2.stride(0), _p(gx), gx.stride(0), B, C, h, w, n_flow, _stream())
    show('out_up2_bwd', 'C=4', plane, layout, gcoarse=gx)
    for factor in (2, 4):
        o = out(layout, B, C, factor * h, factor * w)
        _call('arflow_prob_up_fwd', _p(x), x.stride(0), _p(o), o.stride(0), B, C, h, w, factor, n_flow, n_diag, bias, _stream())
        show('prob_up_fwd', 'factor=%d' % factor, plane, layout, out=o)
        gx, gf = out(layout, B, C, h, w), lay(signed_zeros(randn(B, C, factor * h, factor * w)), layout)
        _call('arflow_prob_up_bwd', _p(gf), gf.stride(0), _p(gx), gx.stride(0), B, C, h, w, factor, n_flow, _stream())
        show('prob_up_bwd', 'factor=%d' % factor, plane, layout, gcoarse=gx)
    if layout == 'slice':
        return  # the remaining entry points take dense tensors: no batch stride to vary
    o1, o0 = out(layout, B, C, 2 * h, 2 * w), out(layout, B, C, 4 * h, 4 * w)
    _call('arflow_out_tail_fwd', _p(x), x.stride(0), _p(o1), _p(o0), B, C, h, w, n_flow, n_diag, bias, _stream())
    show('out_tail_fwd', 'C=4', plane, layout, out1=o1, out0=o0)
    flow = lay(signed_zeros(randn(B, 2, h, w)), layout)
    for factor in (2, 4):
        for align in (0, 1):
            par = 'factor=%d,align=%d' % (factor, align)
            o = out(layout, B, 2, factor * h, factor * w)
            _call('arflow_flow_up_fwd', _p(flow), _p(o), B, h, w, factor, align, _stream())
            show('flow_up_fwd', par, plane, layout, out=o)
            gx, gf = out(layout, B, 2, h, w), lay(signed_zeros(randn(B, 2, factor * h, factor * w)), layout)
            _call('arflow_flow_up_bwd', _p(gf), _p(gx), B, h, w, factor, align, _stream())
            show('flow_up_bwd', par, plane, layout, gcoarse=gx)
    for align in (0, 1):  # the level's x2 adjoint: its fine plane is twice the tool's plane
        gx, gf = out(layout, B, 2, h, w), lay(signed_zeros(randn(B, 2, 2 * h, 2 * w)), layout)
        _call('arflow_up2_bwd', _p(gf), _p(gx), B, 2 * h, 2 * w, align, _stream())
        show('up2_bwd', 'align=%d' % align, plane, layout, gcoarse=gx)


# (B, n) of tests/corr_ref.py::FEAT_SHAPES, the smallest that reach each launch path of csrc/featnorm.hip
FEAT_SHAPES = [(1, 2), (3, 5),  # one workgroup per sample, scalar loops
               (2, 16384),  # one workgroup per sample, float4 loops, at the threshold
               (2, 16385), (2, 16388),  # two launches: scalar, float4
               (512, 20484), (512, 20487)]  # capped grid (a second trip of the grid-stride loops): float4, scalar


def featnorm():
    """arflow_featnorm_fwd / _bwd / arflow_level_moments, both modes; backward with both gradients, gx1 alone, gx2 alone.
    (The second gradient of y1 that is added on load, g1b, has no stand-alone entry point: the `level` family passes it as
    gx1n_direct in every backward, and its level without a flow is this backward with g1b.)"""
    for B, n in FEAT_SHAPES:
        x1, x2 = (randn(B, n) + 0.3).to(DEV), (randn(B, n, scale=1.5) - 0.2).to(DEV)
        g1, g2 = randn(B, n).to(DEV), randn(B, n).to(DEV)
        nacc = 4 * (2048 + B)  # ARFLOW_FEATNORM_ACC_DOUBLES(B)
        acc = torch.zeros(nacc, device=DEV, dtype=torch.float64)
        _call('arflow_level_moments', _p(x1), _p(x2), _p(acc), B, n, _stream())
        show_row('level_moments B=%d,n=%d' % (B, n), 'contig', acc=acc)
        for mode in (0, 1):
            head = 'B=%d,n=%d,mode=%d' % (B, n, mode)
            y1, y2, stats = torch.zeros(B, n, device=DEV), torch.zeros(B, n, device=DEV), torch.zeros(B, 4, device=DEV)
            acc = torch.zeros(nacc, device=DEV, dtype=torch.float64)
            _call('arflow_featnorm_fwd', _p(x1), _p(x2), _p(y1), _p(y2), _p(acc), _p(stats), B, n, mode, _stream())
            show_row('featnorm_fwd ' + head, 'contig', y1=y1, y2=y2, stats=stats, acc=acc)
            for want in ('both', 'gx1', 'gx2'):
                d1 = torch.zeros(B, n, device=DEV) if want != 'gx2' else None
                d2 = torch.zeros(B, n, device=DEV) if want != 'gx1' else None
                acc = torch.zeros(nacc, device=DEV, dtype=torch.float64)
                _call('arflow_featnorm_bwd', _p(g1), _p(g2), _p(x1), _p(x2), _p(stats), _p(acc), _p(d1), _p(d2), B, n, mode,
                      _stream())
                show_row('featnorm_bwd %s,%s' % (head, want), 'contig', gx1=d1, gx2=d2, acc=acc)


# (B, C, H, W) of tests/test_level_gpu.py: one workgroup per sample (twice), tiled with both backward roles in one launch, SPLIT
LEVEL_SHAPES = [(1, 32, 10, 12), (2, 32, 12, 16), (2, 8, 48, 80), (20, 8, 126, 220)]


def level():
    """arflow_level_fwd / _fwd_m / _warp_fwd + _corr_fwd / _bwd: both modes; a coarse flow, a fine flow, no flow; with and
    without the moment rows of arflow_bias_act_fwd_mom; backward in deterministic mode (every output) and in the default mode
    (the outputs that do not pass through float atomics: gx1, and all of them at the level without a flow)."""
    D, SLOPE, PAD, ALIGN, NORM, UP_ALIGN = 4, 0.1, 0, 1, 0, 1
    for B, C, H, W in LEVEL_SHAPES:
        hw, n = H * W, C * H * W
        x1, x2 = (randn(B, C, H, W) + 0.3).to(DEV), (randn(B, C, H, W) + 0.1).to(DEV)
        nr = LIB.arflow_bias_act_mom_rows(C, hw)
        r1, r2 = (torch.zeros(B, nr, 2, device=DEV, dtype=torch.float64) for _ in range(2))
        for x, r in ((x1, r1), (x2, r2)):  # in place: the maps ARE the outputs whose moments the rows hold
            _call('arflow_bias_act_fwd_mom', _p(x), None, _p(x), _p(r), B, C, hw, SLOPE, _stream())
        flows = dict(coarse=randn(B, 2, H // 2, W // 2, scale=1.5).to(DEV), fine=randn(B, 2, H, W, scale=3.0).to(DEV), none=None)
        ctot = 81 + C + 2
        bs = ctot * hw
        gbuf, gext = randn(B, ctot, H, W).to(DEV), randn(B, 2, H, W).to(DEV)
        for mode in (0, 1):
            for kind, flow in flows.items():
                coarse, has_flow = int(kind == 'coarse'), flow is not None
                fbs = 0 if flow is None else flow[0].numel()
                nacc = 4 * B * LIB.arflow_level_acc_rows(B, C, H, W, int(has_flow))
                for rows in (0, 1):
                    head = '%dx%dx%dx%d mode=%d,flow=%s,rows=%d' % (B, C, H, W, mode, kind, rows)
                    buf = torch.zeros(B, ctot, H, W, device=DEV)
                    fup = torch.zeros(B, 2, H, W, device=DEV) if coarse else None
                    x2w = torch.zeros(B, C, H, W, device=DEV) if has_flow else None
                    sign = torch.zeros(B, 3, H, W, device=DEV, dtype=torch.int32)
                    stats = torch.zeros(B, 4, device=DEV)
                    acc = torch.zeros(nacc, device=DEV, dtype=torch.float64)
                    common = (_p(x1), _p(x2), _p(flow), fbs, coarse, UP_ALIGN, _p(fup), buf[:, 81 + C:].data_ptr() if coarse else None,
                              bs, _p(x2w), mode, _p(buf), bs, buf[:, 81:].data_ptr(), bs, _p(sign), _p(stats), _p(acc))
                    tail = (B, C, H, W, D, SLOPE, PAD, ALIGN, NORM, _stream())
                    if rows:
                        _call('arflow_level_fwd_m', *common, _p(r1), nr, None if has_flow else _p(r2), 0 if has_flow else nr, *tail)
                    else:
                        _call('arflow_level_fwd', *common, *tail)
                    show_row('level_fwd ' + head, 'contig', buf=buf, flow_up=fup, x2w=x2w, sign=sign, stats=stats, acc=acc)
                    fl = fup if coarse else flow
                    for det in (1, 0):
                        prev = LIB.arflow_set_deterministic(det)
                        ws = torch.zeros(LIB.arflow_level_bwd_ws_bytes(B, C, H, W) + 256, device=DEV, dtype=torch.uint8)
                        wp = (ws.data_ptr() + 255) & ~255
                        gx1, gx2 = torch.zeros(B, C, H, W, device=DEV), torch.zeros(B, C, H, W, device=DEV)
                        gflow = torch.zeros_like(flow) if has_flow else None
                        _call('arflow_level_bwd', _p(gbuf), bs, _p(sign), buf[:, 81:].data_ptr(), bs, gbuf[:, 81:].data_ptr(), bs,
                              _p(x1), _p(x2), _p(x2w), _p(fl), 2 * hw, gbuf[:, 81 + C:].data_ptr() if coarse else None, bs,
                              _p(gext) if coarse else None, _p(stats), mode, _p(gx1), _p(gx2), _p(gflow), coarse, UP_ALIGN, wp,
                              *tail)
                        torch.cuda.synchronize()
                        LIB.arflow_set_deterministic(prev)
                        keep = det or not has_flow
                        show_row('level_bwd %s,det=%d' % (head, det), 'contig', gx1=gx1, gx2=gx2 if keep else None,
                                 gflow=gflow if keep else None)
                if not has_flow:
                    continue
                # the two stages on their own (always the tiled kernels)
                head = '%dx%dx%dx%d mode=%d,flow=%s' % (B, C, H, W, mode, kind)
                fup = torch.zeros(B, 2, H, W, device=DEV) if coarse else None
                x2w, acc = torch.zeros(B, C, H, W, device=DEV), torch.zeros(nacc, device=DEV, dtype=torch.float64)
                _call('arflow_level_warp_fwd', _p(x1), _p(x2), _p(flow), fbs, coarse, UP_ALIGN, _p(fup), None, 0, _p(x2w), _p(acc),
                      B, C, H, W, PAD, ALIGN, NORM, _stream())
                show_row('level_warp_fwd ' + head, 'contig', flow_up=fup, x2w=x2w, acc=acc)
                out, x1n = torch.zeros(B, 81, H, W, device=DEV), torch.zeros(B, C, H, W, device=DEV)
                sign, stats = torch.zeros(B, 3, H, W, device=DEV, dtype=torch.int32), torch.zeros(B, 4, device=DEV)
                _call('arflow_level_corr_fwd', _p(x1), _p(x2w), _p(acc), nacc // (4 * B), mode, _p(out), 81 * hw, _p(x1n), n, _p(sign),
                      _p(stats), B, C, H, W, D, SLOPE, _stream())
                show_row('level_corr_fwd ' + head, 'contig', out=out, x1n=x1n, sign=sign, stats=stats)


FAMILIES = dict(lowrank=lowrank, mixture=mixture, band=band, pyramid=pyramid, mse=mse, flow_eval=flow_eval, uncert=uncert,
                out_up=out_up)
# families with shapes of their own (the launch paths of the feature normalisation and of the fused pyramid level, DESIGN.md
# section 43): run once, dense tensors
SHAPED = dict(featnorm=featnorm, level=level)

if __name__ == '__main__':
    only = [f for f in args.only.split(',') if f] or list(FAMILIES) + list(SHAPED)
    for fam in only:
        if fam in SHAPED:
            SHAPED[fam]()
            continue
        for plane in PLANES:
            for layout in LAYOUTS:
                FAMILIES[fam](plane, layout)
    for head, row in ROWS.items():
        print(head + ''.join('  %s %s' % (key, ' '.join(hashes)) for key, hashes in row.items()))
