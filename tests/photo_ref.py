"""Shared by tests/test_photo_ref_cpu.py and tests/test_photo_gpu.py: a float64 restatement, in plain torch on the CPU, of the
photometric family -- the 3x3 SSIM distance and the L1 term (csrc/ssim_dev.hpp; the 8 x 32 one-pixel and the 16 x 64 `photo4`
kernels of csrc/ssim.hip; the any-window kernels of csrc/generic.hip) and the fused warp + mask + L1/SSIM pass
(csrc/photo_warp.hip) -- with the per-element error bounds the GPU tests hold the kernels to, the case lists and deliberate
mutations.  Nothing here imports the oracle or the product; the warp and the border mask come from tests/warp_ref.py and
tests/loss_kernels_ref.py.

Reference arithmetic: losses/loss_blocks.py:65-84 (SSIM), losses/flow_loss.py:13-27 (the three sums), utils/warp_utils.py
:83-90, :119-134 (flow_warp, border_mask) as the kernels' comments cite them.  u = 2^-24, U1 = u (1 + 2^-20).

THE OPERATION
    x = rec m, y = im m;  per channel and window w (anchor (wy, wx), N = 9 pixels, un-padded):
        mx = E[x], my = E[y], sx = E[x x] - mx mx, sy = E[y y] - my my, sxy = E[x y] - mx my
        n1 = 2 mx my + C1, n2 = 2 sxy + C2, d1 = mx mx + my my + C1, d2 = sx + sy + C2,  C1 = 0.01^2, C2 = 0.03^2
        S = n1 n2 / (d1 d2),  v = (1 - S) / 2,  dist = clamp(v, 0, 1)
    sums = [sum |im - rec| m,  sum dist,  sum m]
    d dist_w / d x_r = A_w + B_w x_r + C_w y_r where 0 <= v <= 1 (torch.clamp: closed; the any-window backward: open), with
        k = -1/2 up_w 2/9,  C = k n1 / d,  B = -k (n / d^2) d1,  A = k ((my n2 - n1 my) / d - (n / d^2)(mx d2 - d1 mx))
    d / d rec_r = m_r (c_l1 sign(rec_r - im_r) + sum over the <= 9 windows holding r of (A_w + B_w x_r + C_w y_r))
    fused pass: rec = flow_warp(src, flow, pad) (coordinate in fp32 as warp_ref defines it, everything behind it float64),
        m = the plane, its nearest resize m[y fy, x fx], or border_mask(flow) (fp32 x + u, open interval), 1 - m in fp32 where
        inverted (the kernel's own single rounding: the mask planes are exact);  d / d flow = warp's flow gradient of d / d rec.

BOUNDS.  Every quantity is carried as (value, absolute error bound) through the kernel's operations IN THE KERNEL'S ORDER
    (_add, _mul, _div below: |a| db + |b| da + da db for a product, (da + |q| db) / (|b| - db) for a quotient, plus r U1 times
    the largest magnitude the rounded result can have; r = number of roundings of the operation).  No constant is fitted.
        WinAcc::add          x x, y y, x y: 1 rounding each; the nine terms in row-major order: 8 additions (the first onto
                             0.f is exact), each term passes through at most 8  -> _chain(.., 8)          ssim_dev.hpp:58-64
        finish               div9 = IEEE x / 9: 1;  mx mx: 1;  the subtraction: 1                         ssim_dev.hpp:65-73
                             => means 8 + 1 = 9 u mean|x|, second moments 1 + 8 + 1 = 10 u mean(x x), then the cancellation
        ssim_terms           2 mx exact, products 1, additions 1.  The kernel's C1 = fl(fl(0.01) fl(0.01)) and the oracle's
                             fl(1e-4) both lie within C_ERR of 0.01^2 (computed below, not assumed)       ssim_dev.hpp:17,28
        ssim_dist            n1 n2: 1, d1 d2: 1, fdiv_pos within 1 ulp of the IEEE quotient (2 u), 1 - q: 1, / 2 exact:
                             dS <= (|n2| dn1 + |n1| dn2) / (d1 d2) + |S| (dd1 / d1 + dd2 / d2) + 4 u |S|, ddist <= dS / 2 + u |v|
                             A window with x == y element for element (all-zero windows of a masked image are) has n == d
                             BIT FOR BIT (2 mx mx = mx mx + mx mx, 2 sxy = sx + sy exactly), the Newton step of fdiv_pos then
                             returns exactly 1 (the correction is q - delta (1 + eps) = 1 - delta eps, |delta eps| << u), so
                             dist = 0 exactly: bound 0.                                                   ssim_dev.hpp:43-47,87-91
        ssim_dist_grad       k: 2 / 9 rounded (1) and the product (1); frcp_pos within 1 ulp (2 u); every further product and
                             difference 1, in the order written                                           ssim_dev.hpp:96-108
        Coef::add, gather    the nine windows' A, B, C: 8 additions each (absent windows are exact zeros)  ssim_dev.hpp:111-118
        rec_grad             sign(rec - im) is exact (a difference of two floats has the right sign); ((c_l1 sg + a) + b x) +
                             c y: 2 products, 3 additions; times m: 1                                     ssim_dev.hpp:120-124
        x = rec m, y = im m  1 rounding unless m is 0 or 1
    any-window kernels (md != 1): the same statistics with N = (2 md + 1)^2 (N - 1 additions, IEEE / N, IEEE quotient); the
        backward adds per pixel the N windows' g (-1/2 dS) by fmaf (N roundings), dS in the order of generic.hip:290-291.
    Sums: the sum of the term bounds plus depth u sum|term|.
    depth = per-thread chain + 6 (wave butterfly, common.hpp:92-96) + 4 (block: waves 0..3 onto 0.f, :115-121) + (T - 1)
        (the fold over the T tile rows that are not zero rows, ANY order: torch's .sum over the rows is taken on trust as a sum)
        per-thread chain    L1                         SSIM        mask
        one-pixel 8 x 32    2 C   (<= 2 owned slots)   C           0        ssim.hip:42-62
        photo4 16 x 64      3 + 2 + C (4-term tree,    4 C         2        ssim.hip:163-178, :198-216
                            2 staging rounds, channels)
        fused pass          (C - 1) + 5 (5 slots)      4 C         5        photo_warp.hip:95-130
    Fused pass: rec carries warp_ref's forward bound (K_F = 7); d / d flow = warp_ref's flow-gradient bound with |gr| as the
    upstream, plus |dc/du| sum_c dgr_c |s_c| (s_c the corner difference of channel c).

KINKS (named, left out of GRADIENT comparisons only; the share is capped at KINK_CAP = 0.5 % per case)
    L1 kink      fused pass only: a pixel-channel with |tgt - rec64| <= the warp's forward bound and that bound > 0 (where the
                 warp is exact -- integer coordinates -- rec is the source value bit for bit and the sign is defined, 0 included)
    clamp kink   a window whose v is within its bound of 0 or 1, unless x == y element for element there: then A + B x + C y
                 vanishes identically (S is at its maximum), the contribution is 0 on either side of the clamp
    Consequence: 'the clamp's open and closed interval swapped' cannot be expressed as a mutation of this operation.  v = 0
    needs x == y on the window, where the passed gradient is 0 anyway; v = 1 needs S = -1, and n1 <= d1, |n2| < d2 make S > -1.
    The interval that IS observable is the border mask's (0 < x + u < W - 1, open): mutation 'border_closed'.
"""
import collections
import types

import numpy as np
import torch
import torch.nn.functional as F

from tests.loss_kernels_ref import D, U, _gen, coord_mask_ref, worst  # noqa: F401 (re-exported)
from tests.warp_ref import NORM_ARFLOW, PAD, U1, _snap, coords, warp_ref

C1, C2 = 0.01 ** 2, 0.03 ** 2
_f = np.float32
# the kernel's constants (constexpr fp32 products) and the oracle's (the float64 literal rounded once) against the formula's
C1_ERR = max(abs(float(_f(0.01) * _f(0.01)) - C1), abs(float(_f(C1)) - C1))
C2_ERR = max(abs(float(_f(0.03) * _f(0.03)) - C2), abs(float(_f(C2)) - C2))
KINK_CAP = 0.005
TILES = {'px1': (8, 32), 'photo4': (16, 64), 'pw': (16, 64)}
MUTATIONS = ('mean8', 'pool_after', 'c1c2', 'mask_once', 'sign0', 'halo_col', 'halo_row', 'anchor_shift', 'chan_last',
             'nearest_fx', 'invert_border', 'border_closed', 'half_tgt')


# ======================================================================================================================
# (value, bound) arithmetic: one function per fp32 operation of the kernels
# ======================================================================================================================
Iv = collections.namedtuple('Iv', 'v e')


def _iv(v, e=None):
    v = torch.as_tensor(v, dtype=D)
    return Iv(v, torch.zeros_like(v) if e is None else torch.as_tensor(e, dtype=D).expand_as(v))


def _rnd(v, e0, r):
    return Iv(v, e0 + r * U1 * (v.abs() + e0))


def _add(a, b, r=1):
    return _rnd(a.v + b.v, a.e + b.e, r)


def _sub(a, b, r=1):
    return _rnd(a.v - b.v, a.e + b.e, r)


def _mul(a, b, r=1):
    return _rnd(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e, r)


def _div(a, b, r=1):
    q = a.v / b.v
    lo = b.v.abs() - b.e
    assert bool((lo > 0).all()), 'a denominator is not separated from 0'
    return _rnd(q, (a.e + q.abs() * b.e) / lo, r)


def _scale(a, c):
    """times a power of two, or a constant division whose rounding the caller counts: exact here"""
    return Iv(a.v * c, a.e * abs(c))


def _chain(t, nadd, dim=0):
    """sum over `dim` where every term passes through at most `nadd` roundings"""
    return Iv(t.v.sum(dim), t.e.sum(dim) + nadd * U1 * (t.v.abs() + t.e).sum(dim))


def _pick(cond, a, b):
    return Iv(torch.where(cond, a.v, b.v), torch.where(cond, a.e, b.e))


# ======================================================================================================================
# windows
# ======================================================================================================================
def _shifts(t, md, mutate=None, tile=None, origin=(0, 0)):
    """[N, B, C, Ho, Wo]: element (i, j) (row-major) of the window anchored at every (wy, wx)"""
    k = 2 * md + 1
    H, W = t.shape[-2:]
    Ho, Wo = H - 2 * md, W - 2 * md
    out = []
    wy = torch.arange(Ho).view(Ho, 1)
    wx = torch.arange(Wo).view(1, Wo)
    ay, ax = wy + origin[0], wx + origin[1]   # anchors in image coordinates (t may be a crop)
    if mutate == 'anchor_shift':  # the last anchor column of a tile reads the window one column further
        wx = torch.where((ax % tile[1] == tile[1] - 1) & (wx + 1 < Wo), wx + 1, wx)
    for i in range(k):
        for j in range(k):
            s = t[..., (wy + i).expand(Ho, Wo), (wx + j).expand(Ho, Wo)]
            if mutate == 'halo_col' and j == 2:   # column TW + 1 of the staged tile never arrives
                s = s * (ax % tile[1] != tile[1] - 1).to(D)
            if mutate == 'halo_row' and i == 2:
                s = s * (ay % tile[0] != tile[0] - 1).to(D)
            out.append(s)
    return torch.stack(out, 0)


def _win(X, Y, md=1, mutate=None, tile=None, origin=(0, 0)):
    """X, Y: Iv [B, C, H, W].  -> namespace of Iv [B, C, Ho, Wo]: mx, my, sx, sy, sxy, n1, n2, d1, d2, n, d, S, v, dist;
    same: bool, x == y element for element (inputs exact): dist is exactly 0 there."""
    N = (2 * md + 1) ** 2
    xs = Iv(_shifts(X.v, md, mutate, tile, origin), _shifts(X.e, md, mutate, tile, origin))
    ys = Iv(_shifts(Y.v, md, mutate, tile, origin), _shifts(Y.e, md, mutate, tile, origin))
    o = types.SimpleNamespace()
    div = 8.0 if mutate == 'mean8' else float(N)

    def mean(t):   # N - 1 additions, then the correctly rounded division by N
        s = _chain(t, N - 1)
        return _rnd(s.v / div, s.e / div, 1)
    o.mx, o.my = mean(xs), mean(ys)
    if mutate == 'pool_after':   # products of the pooled values instead of pooled products
        exx, eyy, exy = _mul(o.mx, o.mx), _mul(o.my, o.my), _mul(o.mx, o.my)
    else:
        exx, eyy, exy = mean(_mul(xs, xs)), mean(_mul(ys, ys)), mean(_mul(xs, ys))
    o.sx = _sub(exx, _mul(o.mx, o.mx))
    o.sy = _sub(eyy, _mul(o.my, o.my))
    o.sxy = _sub(exy, _mul(o.mx, o.my))
    c1, c2 = _iv(torch.tensor(C1, dtype=D), C1_ERR), _iv(torch.tensor(C2, dtype=D), C2_ERR)
    if mutate == 'c1c2':
        c1, c2 = c2, c1
    o.n1 = _add(_mul(_scale(o.mx, 2.0), o.my), c1)
    o.n2 = _add(_scale(o.sxy, 2.0), c2)
    o.d1 = _add(_add(_mul(o.mx, o.mx), _mul(o.my, o.my)), c1)
    o.d2 = _add(_add(o.sx, o.sy), c2)
    o.n, o.d = _mul(o.n1, o.n2), _mul(o.d1, o.d2)
    o.same = ((xs.v == ys.v) & (xs.e == 0) & (ys.e == 0)).all(0)
    S = _div(o.n, o.d, 2)
    o.S = Iv(S.v, torch.where(o.same, torch.zeros_like(S.e), S.e))
    v = _scale(_sub(_iv(torch.ones(())), o.S), 0.5)
    o.v = Iv(v.v, torch.where(o.same, torch.zeros_like(v.e), v.e))
    o.dist = Iv(o.v.v.clamp(0.0, 1.0), o.v.e)
    o.kink = ((o.v.v.abs() <= o.v.e) | ((o.v.v - 1.0).abs() <= o.v.e)) & ~o.same
    return o


def win_ref(x, y, md=1):
    """the five window statistics of two [B, C, H, W] images, float64, each with its bound: namespace of Iv"""
    return _win(_iv(x), _iv(y), md)


def ssim_ref(x, y, md=1, mutate=None, tile=None):
    """-> namespace: dist (Iv: the SSIM distance map and its bound per window), kink, same, and the statistics"""
    return _win(_iv(x), _iv(y), md, mutate, tile)


def _coefs(w, up, open_interval=False):
    """ssim_dist_grad: A, B, C (Iv) of every window; up: [B, C, Ho, Wo] upstream coefficient"""
    k = _mul(_iv(-0.5 * up), _iv(torch.tensor(2.0 / 9.0, dtype=D), U * 2.0 / 9.0))
    idn = _div(_iv(torch.ones(())), w.d, 2)
    nd2 = _mul(_mul(w.n, idn), idn)
    Cc = _mul(_mul(k, w.n1), idn)
    Bc = _mul(_mul(_scale(k, -1.0), nd2), w.d1)
    t1 = _mul(_sub(_mul(w.my, w.n2), _mul(w.n1, w.my)), idn)
    t2 = _mul(nd2, _sub(_mul(w.mx, w.d2), _mul(w.d1, w.mx)))
    A = _mul(k, _sub(t1, t2))
    v = w.v.v
    ok = ((v > 0) & (v < 1)) if open_interval else ((v >= 0) & (v <= 1))
    z = _iv(torch.zeros_like(v))
    return _pick(ok, A, z), _pick(ok, Bc, z), _pick(ok, Cc, z)


def _gather9(t, H, W):
    """Coef::add over the windows anchored at (y - i, x - j), i, j = 0..2: [B, C, Ho, Wo] -> [B, C, H, W]"""
    p = Iv(F.pad(t.v, (2, 2, 2, 2)), F.pad(t.e, (2, 2, 2, 2)))
    st = Iv(torch.stack([p.v[..., 2 - i:2 - i + H, 2 - j:2 - j + W] for i in range(3) for j in range(3)], 0),
            torch.stack([p.e[..., 2 - i:2 - i + H, 2 - j:2 - j + W] for i in range(3) for j in range(3)], 0))
    return _chain(st, 8)


def _pixel_kink(wk, H, W):
    """a pixel of any channel's kink window -> [B, 1, H, W] bool"""
    k = F.pad(wk.any(1, keepdim=True).to(D), (2, 2, 2, 2))
    return torch.stack([k[..., 2 - i:2 - i + H, 2 - j:2 - j + W] for i in range(3) for j in range(3)], 0).sum(0) > 0


def _masked(t, m, e=None):
    """x = t m as the kernels stage it: one rounding unless the mask value is 0 or 1"""
    t = _iv(t, e)
    if m is None:
        return t
    p = _mul(t, _iv(m), 0)
    exact = (m == 0) | (m == 1)
    return Iv(p.v, torch.where(exact.expand_as(p.v), p.e, p.e + U1 * (p.v.abs() + p.e)))


def depth(kernel, what, C, tiles):
    chain = {'px1': {'l1': 2 * C, 'ss': C, 'm': 0}, 'photo4': {'l1': 5 + C, 'ss': 4 * C, 'm': 2},
             'pw': {'l1': C + 4, 'ss': 4 * C, 'm': 5}}[kernel][what]
    return chain + 6 + 4 + max(tiles - 1, 0)


def n_tiles(kernel, B, H, W):
    th, tw = TILES[kernel]
    return B * (-(-H // th)) * (-(-W // tw))


def kernel_of(W):
    return 'photo4' if W % 4 == 0 else 'px1'


def _total(t, d, dims=None):
    dims = tuple(range(t.v.dim())) if dims is None else dims
    return Iv(t.v.sum(dims), t.e.sum(dims) + d * U1 * (t.v.abs() + t.e).sum(dims))


def _rec_grad(m, c_l1, sg, a, b, c, X, Y, mutate=None, rec=None, im=None):
    if mutate == 'mask_once':   # the coefficients multiply rec and im, not rec m and im m
        X, Y = rec, im
    inner = _add(_add(_add(_iv(c_l1 * sg), a), _mul(b, X)), _mul(c, Y))
    return inner if m is None else _mul(_iv(m), inner)


# ======================================================================================================================
# the stand-alone kernels
# ======================================================================================================================
def photo_sums_ref(im, rec, mask, coef=(1.0, 1.0), gmap=None, mutate=None, kernel=None):
    """im, rec [B, C, H, W], mask [B, 1, H, W] or None (fp32 values).  -> namespace (Iv: float64 value and bound)
        sums   [3]                 sum |im - rec| m, sum dist, sum m
        dist   [B, C, H-2, W-2]    the distance map of (rec m, im m)
        grad   [B, C, H, W]        d / d rec of coef[0] s0 + coef[1] s1 -- or, with gmap [B, C, H-2, W-2], of sum gmap dist
        kink   [B, 1, H, W] bool   pixels left out of gradient comparisons (clamp kink)"""
    assert mutate is None or mutate in MUTATIONS
    B, C, H, W = im.shape
    kernel = kernel or kernel_of(W)
    tile, T = TILES[kernel], n_tiles(kernel, B, H, W)
    im, rec = im.to(D), rec.to(D)
    m = None if mask is None else mask.to(D)
    X, Y = _masked(rec, m), _masked(im, m)
    w = _win(X, Y, 1, mutate if mutate in ('mean8', 'pool_after', 'c1c2', 'halo_col', 'halo_row', 'anchor_shift') else None,
             tile)
    o = types.SimpleNamespace(dist=w.dist, win=w)
    l1 = _sub(_iv(im), _iv(rec))
    l1 = Iv(l1.v.abs(), l1.e)
    if m is not None:
        l1 = _mul(l1, _iv(m))
    dist = w.dist
    if mutate == 'chan_last':
        keep = (torch.arange(C) < C - 1).view(1, C, 1, 1).to(D)
        l1, dist = Iv(l1.v * keep, l1.e), Iv(dist.v * keep, dist.e)
    msum = _iv(m if m is not None else torch.ones(B, 1, H, W, dtype=D))
    o.sums = [_total(l1, depth(kernel, 'l1', C, T)), _total(dist, depth(kernel, 'ss', C, T)),
              _total(msum, depth(kernel, 'm', C, T))]
    c_l1 = 0.0 if gmap is not None else float(coef[0])
    up = gmap.to(D) if gmap is not None else torch.full_like(w.v.v, float(coef[1]))
    A, Bc, Cc = _coefs(w, up)
    diff = rec - im
    sg = torch.sign(diff)
    if mutate == 'sign0':
        sg = torch.where(diff == 0, torch.ones_like(sg), sg)
    g = _rec_grad(m, c_l1, sg, _gather9(A, H, W), _gather9(Bc, H, W), _gather9(Cc, H, W), X, Y, mutate, _iv(rec), _iv(im))
    if mutate == 'chan_last':
        g = Iv(g.v * keep, g.e)
    o.grad = g
    o.kink = _pixel_kink(w.kink, H, W)
    return o


def ssim_any_grad_ref(x, y, gmap, md):
    """d / d x of sum gmap dist for the any-window kernels (generic.hip:269-295): per pixel the N windows that hold it, each
    term -1/2 g dS with dS in the kernel's order, added by fmaf.  -> (Iv [B, C, H, W], kink [B, 1, H, W])"""
    B, C, H, W = x.shape
    k = 2 * md + 1
    N = float(k * k)
    X, Y = _iv(x.to(D)), _iv(y.to(D))
    w = _win(X, Y, md)
    Nn = _iv(torch.tensor(N))
    S = w.S
    den = _mul(_mul(Nn, w.d1), w.d2)
    nb1, nb2 = _mul(Nn, w.d1), _mul(Nn, w.d2)
    ok = (w.v.v > 0) & (w.v.v < 1)
    pad = k - 1

    def shifted(t, i, j, fill=0.0):
        p = Iv(F.pad(t.v, (pad, pad, pad, pad), value=fill), F.pad(t.e, (pad, pad, pad, pad)))
        return Iv(p.v[..., pad - i:pad - i + H, pad - j:pad - j + W], p.e[..., pad - i:pad - i + H, pad - j:pad - j + W])
    terms_v, terms_e = [], []
    okp = F.pad(ok.to(D), (pad, pad, pad, pad))
    for i in range(k):
        for j in range(k):
            my, mx = shifted(w.my, i, j), shifted(w.mx, i, j)
            a1, a2 = shifted(w.n1, i, j), shifted(w.n2, i, j)
            dn = shifted(den, i, j, 1.0)
            b1, b2 = shifted(nb1, i, j, 1.0), shifted(nb2, i, j, 1.0)
            s = shifted(S, i, j)
            g = shifted(_iv(gmap.to(D)), i, j)
            p1 = _div(_add(_mul(_scale(my, 2.0), a2), _mul(_scale(a1, 2.0), _sub(Y, my))), dn)
            p2 = _mul(s, _add(_div(_scale(mx, 2.0), b1), _div(_mul(_iv(torch.tensor(2.0)), _sub(X, mx)), b2)))
            t = _mul(g, _scale(_sub(p1, p2), -0.5), 0)   # the product is rounded inside the fmaf: counted by the chain
            live = okp[..., pad - i:pad - i + H, pad - j:pad - j + W]
            terms_v.append(t.v * live)
            terms_e.append(t.e * live)
    acc = _chain(Iv(torch.stack(terms_v, 0), torch.stack(terms_e, 0)), int(N))
    kp = F.pad(w.kink.any(1, keepdim=True).to(D), (pad, pad, pad, pad))
    kink = torch.stack([kp[..., pad - i:pad - i + H, pad - j:pad - j + W] for i in range(k) for j in range(k)], 0).sum(0) > 0
    return acc, kink


# ======================================================================================================================
# the fused pass
# ======================================================================================================================
def mask_plane_ref(flow, mask, mask_mode, mask_invert, mutate=None):
    """the [B, 1, H, W] fp32 plane a group uses, exactly (pw::pixel, photo_warp.hip:57-66)"""
    B, _, H, W = flow.shape
    if mask_mode == 'border':
        m = coord_mask_ref(flow, 0 if mutate == 'border_closed' else 1)
        if mutate == 'invert_border':
            return m
    elif mask_mode == 'nearest':
        fy, fx = mask.shape[-2] // H, mask.shape[-1] // W
        if mutate == 'nearest_fx':
            fy = fx
        mw = mask.shape[-1]   # mk[(y fy) mask_w + x fx] inside the sample's plane
        idx = ((torch.arange(H) * fy).view(H, 1) * mw + (torch.arange(W) * fx).view(1, W)).clamp_max(mask[0, 0].numel() - 1)
        m = mask.reshape(B, 1, -1)[:, :, idx.reshape(-1)].reshape(B, 1, H, W)
    else:
        m = mask
    m = m.float()
    return (1.0 - m) if mask_invert else m


def photo_warp_ref(tgt, src, flow, mask, pad, mask_mode, mask_invert, coef=None, mutate=None):
    """tgt, src: lists of G [B, C, H, W]; flow: list of G [B, 2, H, W]; mask: list of G planes or None ('border');
    coef [G][2] = (c_l1, c_ss) of each group.  -> namespace
        sums [G][3] (Iv),  mask_out [G*B, 1, H, W] (fp32, exact),  gflow, bound_gflow, kink: lists of G [B, 2, H, W]"""
    assert mutate is None or mutate in MUTATIONS
    G = len(tgt)
    B, C, H, W = tgt[0].shape
    coef = coef or [_r32(0.3, 0.7)] * G
    T = n_tiles('pw', B, H, W)
    o = types.SimpleNamespace(sums=[], gflow=[], bound_gflow=[], kink=[], rec=[], masks=[])
    for g in range(G):
        sg_src = src[0] if (mutate == 'half_tgt') else src[g]
        m32 = mask_plane_ref(flow[g], None if mask is None else mask[g], mask_mode, mask_invert, mutate)
        o.masks.append(m32)
        m = m32.to(D)
        wr = warp_ref(sg_src, flow[g], PAD[pad], True, NORM_ARFLOW)
        t = tgt[g].to(D)
        X, Y = _masked(wr.out, m, wr.bound_out), _masked(t, m)
        w = _win(X, Y, 1, mutate if mutate in ('mean8', 'pool_after', 'c1c2', 'halo_col', 'halo_row', 'anchor_shift') else None,
                 TILES['pw'])
        rec = Iv(wr.out, wr.bound_out)
        l1 = _sub(_iv(t), rec)
        l1 = _mul(Iv(l1.v.abs(), l1.e), _iv(m))
        dist = w.dist
        keep = (torch.arange(C) < (C - 1 if mutate == 'chan_last' else C)).view(1, C, 1, 1).to(D)
        l1, dist = Iv(l1.v * keep, l1.e), Iv(dist.v * keep, dist.e)
        o.sums.append([_total(l1, depth('pw', 'l1', C, T)), _total(dist, depth('pw', 'ss', C, T)),
                       _total(_iv(m), depth('pw', 'm', C, T))])
        c_l1, c_ss = float(coef[g][0]), float(coef[g][1])
        A, Bc, Cc = _coefs(w, torch.full_like(w.v.v, c_ss))
        diff = wr.out - t
        sg = torch.sign(diff)
        if mutate == 'sign0':
            sg = torch.where(diff == 0, torch.ones_like(sg), sg)
        gr = _rec_grad(m, c_l1, sg, _gather9(A, H, W), _gather9(Bc, H, W), _gather9(Cc, H, W), X, Y, mutate, rec, _iv(t))
        gr = Iv(gr.v * keep, gr.e)
        wg = warp_ref(sg_src, flow[g], PAD[pad], True, NORM_ARFLOW, gout=gr.v)
        extra = torch.zeros_like(wg.gflow)
        for c in range(C):   # |dc/du| dgr_c |s_c|, channel by channel
            one = torch.zeros_like(gr.e)
            one[:, c] = gr.e[:, c]
            extra += warp_ref(sg_src, flow[g], PAD[pad], True, NORM_ARFLOW, gout=one).gflow.abs()
        o.gflow.append(wg.gflow)
        o.bound_gflow.append(wg.bound_gflow + extra * (1.0 + 8 * U1))
        l1k = ((diff.abs() <= wr.bound_out) & (wr.bound_out > 0)).any(1, keepdim=True) & (m != 0) & (c_l1 != 0)
        o.kink.append((l1k | _pixel_kink(w.kink, H, W)).expand(B, 2, H, W))
        o.rec.append(rec)
    o.mask_out = torch.cat(o.masks, 0)
    return o


# ======================================================================================================================
# inputs
# ======================================================================================================================
def images(cls, B, C, H, W, seed=0):
    """(im, rec) fp32, about [0, 1].  'noise' U[0,1); 'blur' its 5x5 box blur (3x3 below that size), like the workload's frames;
    'near' rec = im + 0.01 n on a blurred im; 'low' 0.9 + 0.05 noise (low contrast on a high mean: sigma = E[x x] - mu mu
    cancels hardest while dist stays clear of 0).  Every class carries a 2 x 2 patch where rec == im exactly (the L1 sign at
    0) when the image has room."""
    gen = _gen(41, B, C, H, W, seed)
    a, b = torch.rand(B, C, H, W, generator=gen), torch.rand(B, C, H, W, generator=gen)

    def blur(t):
        k = 5 if min(H, W) >= 5 else 3
        return F.avg_pool2d(F.pad(t, (k // 2,) * 4, mode='reflect'), k, 1)
    if cls == 'blur':
        a, b = blur(a), blur(b)
    elif cls == 'near':
        a = blur(a)
        b = a + 0.01 * torch.randn(B, C, H, W, generator=gen)
    elif cls == 'low':
        a, b = 0.9 + 0.05 * a, 0.9 + 0.05 * b
    elif cls != 'noise':
        raise KeyError(cls)
    if H >= 5 and W >= 5:
        b[:, :, 1:3, 1:3] = a[:, :, 1:3, 1:3]
    return a.contiguous(), b.contiguous()


def mask_of(kind, B, H, W, seed=0):
    """None; 'binary' rand > 0.2; 'frac' U[0,1) values (what up4_clamp_mul produces); 'rect' binary with a zero rectangle
    of at least 5 x 5 (whole windows zero) -- the rectangle straddles the first tile corner where the image reaches it"""
    if kind == 'none':
        return None
    gen = _gen(43, B, H, W, seed)
    r = torch.rand(B, 1, H, W, generator=gen)
    if kind == 'frac':
        return r.contiguous()
    m = (r > 0.2).float()
    if kind == 'rect':
        y0, x0 = max(min(H - 6, 5), 0), max(min(W - 7, 28), 0)
        m[:, :, y0:y0 + 6, x0:x0 + 7] = 0.0
    return m.contiguous()


SCase = collections.namedtuple('SCase', 'B C H W cls mask')
# one-pixel tiling (W % 4 != 0), 8 x 32 tiles: a last tile of 1 / 2 / 3 columns or rows; tile counts 1, 7, 9, 17 at 3 x 3
PX1_CASES = [
    SCase(1, 1, 3, 3, 'noise', 'none'), SCase(7, 3, 3, 3, 'near', 'binary'), SCase(9, 2, 3, 3, 'low', 'frac'),
    SCase(17, 3, 3, 3, 'noise', 'binary'),
    SCase(2, 3, 8, 34, 'blur', 'rect'), SCase(1, 2, 9, 33, 'near', 'frac'), SCase(2, 1, 10, 35, 'low', 'binary'),
    SCase(1, 3, 11, 67, 'blur', 'frac'), SCase(3, 3, 11, 67, 'low', 'rect'), SCase(1, 3, 10, 35, 'noise', 'none'),
]
# photo4 (W % 4 == 0), 16 x 64 tiles; tile counts 1, 7, 9, 17 at the one-tile shapes
P4_CASES = [
    SCase(1, 1, 3, 4, 'noise', 'none'), SCase(7, 3, 16, 64, 'blur', 'binary'), SCase(9, 2, 3, 4, 'noise', 'frac'),
    SCase(17, 3, 3, 4, 'near', 'binary'),
    SCase(2, 3, 17, 68, 'blur', 'rect'), SCase(1, 2, 18, 72, 'near', 'frac'), SCase(1, 3, 19, 132, 'blur', 'frac'),
    SCase(2, 1, 16, 64, 'low', 'rect'), SCase(1, 3, 19, 132, 'low', 'none'), SCase(3, 3, 18, 72, 'noise', 'binary'),
]
SUMS_CASES = PX1_CASES + P4_CASES
def _r32(*v):
    """weights as the kernels receive them: fp32"""
    return tuple(float(_f(x)) for x in v)


WEIGHTS = [(1.0, 0.0), (0.0, 1.0), _r32(0.3, 0.7)]
ANY_CASES = [(2, 1, 2, 7, 9), (3, 1, 2, 9, 12), (2, 2, 3, 11, 20), (3, 1, 1, 7, 7)]   # (md, B, C, H, W)


def sums_inputs(c):
    im, rec = images(c.cls, c.B, c.C, c.H, c.W)
    up = torch.randn(c.B, c.C, c.H - 2, c.W - 2, generator=_gen(47, c.B, c.C, c.H, c.W))
    return im, rec, mask_of(c.mask, c.B, c.H, c.W), up


def sums_mutations(c):
    """the mutations a stand-alone case can express"""
    th, tw = TILES[kernel_of(c.W)]
    mu = ['mean8', 'pool_after', 'c1c2']
    if c.C > 1:
        mu.append('chan_last')
    if c.mask == 'frac':
        mu.append('mask_once')
    if c.H >= 5 and c.W >= 5:
        mu.append('sign0')
    if c.W - 2 > tw - 1:    # an anchor in the last column of a full tile exists
        mu += ['halo_col'] + (['anchor_shift'] if c.W - 2 > tw else [])
    if c.H - 2 > th - 1:
        mu.append('halo_row')
    return mu


PCase = collections.namedtuple('PCase', 'name B G C H W pad mode invert addr cls mask fyx coef field')
_MIX = (_r32(0.3, 0.7), _r32(0.6, 1.4))


def _p(name, B, G, C, H, W, pad='zeros', mode='plane', invert=False, addr='flow4', cls='blur', mask='binary', fyx=(1, 1),
       coef=_MIX, field='smooth'):
    return PCase(name, B, G, C, H, W, pad, mode, invert, addr, cls, mask, fyx, coef[:G], field)


# the fused pass, per-pixel gradient: C, G, B, both addressings, the three mask modes with and without inversion, nearest
# factors with fy != fx, fractional planes, single-term and unequal weights, shapes from one window to 3 x 3 tiles
PW_CASES = [
    _p('3x3 C1 G1 B1', 1, 1, 1, 3, 3, cls='noise', mask='frac', coef=(_r32(0.4, 1.1),)),
    _p('5x7 C2 G2 B1 shared', 1, 2, 2, 5, 7, addr='shared', mask='frac', pad='border', coef=((0.0, 1.0), (1.0, 0.0))),
    _p('16x64 C3 G2 B3 plane invert', 3, 2, 3, 16, 64, invert=True),
    _p('16x64 C3 G1 B3 border', 3, 1, 3, 16, 64, mode='border', pad='border', cls='noise', coef=((0.0, 1.0),)),
    _p('17x65 C3 G2 B1 border invert', 1, 2, 3, 17, 65, mode='border', invert=True, addr='shared', field='edge'),
    _p('17x65 C2 G2 B3 nearest 2x4', 3, 2, 2, 17, 65, mode='nearest', fyx=(2, 4), pad='border'),
    _p('19x67 C3 G2 B1 nearest 4x2 invert', 1, 2, 3, 19, 67, mode='nearest', fyx=(4, 2), invert=True, addr='shared'),
    _p('19x67 C1 G2 B3 frac', 3, 2, 1, 19, 67, mask='frac', cls='low', coef=((1.0, 0.0), (0.0, 1.0))),
    _p('33x130 C3 G2 B1 rect', 1, 2, 3, 33, 130, mask='rect', pad='border', field='exact'),
    _p('33x130 C3 G1 B1 nearest 1x1', 1, 1, 3, 33, 130, mode='nearest', fyx=(1, 1), cls='near'),
    _p('5x7 C3 G2 B3 border', 3, 2, 3, 5, 7, mode='border', field='edge'),
]


EXACT_PATCHES = ((slice(2, 6), slice(3, 9)), (slice(18, 22), slice(60, 70)))   # the second across the tile corner (16, 64)


def pw_flow(c, g):
    """[B, 2, H, W]: 'smooth' a coarse field of ~ a quarter of the extent + 0.3 pixel noise (a share leaves the image);
    'edge' in addition columns / rows whose x + u, y + v land exactly on 0, W - 1, H - 1 (open against closed interval);
    'exact' in addition a zero-flow patch (integer coordinates: the warp is exact there, rec == src bit for bit)"""
    B, H, W = c.B, c.H, c.W
    gen = _gen(53, B, H, W, g, c.C)
    coarse = 0.25 * min(H, W) * torch.randn(B, 2, 3, 3, generator=gen)
    f = F.interpolate(coarse, (H, W), mode='bilinear', align_corners=True) + 0.3 * torch.randn(B, 2, H, W, generator=gen)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    if c.field == 'edge':
        f[:, 0, :, 1] = (0.0 - xs[..., 1])
        f[:, 0, :, W // 2] = (W - 1.0) - xs[..., W // 2]
        f[:, 1, 1, :] = (0.0 - ys[:, 1])
        f[:, 1, H // 2, :] = (H - 1.0) - ys[:, H // 2]
        f[:, :, H - 2:, W - 2:] = 0.0   # inside for both intervals except on the border itself
    if c.field == 'exact':
        # zero flow nudged by a few ulp until the fp32 coordinate IS the pixel (the normalise round trip is not the identity);
        # pixels no neighbour reaches keep the smooth field (rec would be within a rounding of tgt: an L1 kink for nothing)
        tx, ty = xs.to(D).expand(B, H, W).contiguous(), ys.to(D).expand(B, H, W).contiguous()
        z, _ = _snap(torch.zeros(B, 2, H, W), tx, ty, H, W, NORM_ARFLOW, True)
        ix, iy, _, _ = coords(z, H, W, NORM_ARFLOW, True)
        hit = ((ix.to(D) == tx) & (iy.to(D) == ty)).unsqueeze(1).expand(B, 2, H, W)
        for sl in EXACT_PATCHES:
            f[(slice(None), slice(None)) + sl] = torch.where(hit, z, f)[(slice(None), slice(None)) + sl]
    return f.contiguous()


def pw_inputs(c):
    """-> namespace tgt, src, flow, mask (lists of G; mask None for 'border').  addr 'flow4': two images, each the other's
    source; 'shared': one target, two sources.  Where the field is 'exact' the images agree on the zero-flow patches
    (rec == tgt there: the L1 sign at 0)"""
    o = types.SimpleNamespace(flow=[], mask=None if c.mode == 'border' else [])
    a, b = images(c.cls, c.B, c.C, c.H, c.W, seed=1)
    b2 = images(c.cls, c.B, c.C, c.H, c.W, seed=2)[1]
    if c.field == 'exact':
        for t in (b, b2):
            for sl in EXACT_PATCHES:
                t[(slice(None), slice(None)) + sl] = a[(slice(None), slice(None)) + sl]
    if c.addr == 'flow4':    # two images, each the other's source
        o.tgt, o.src = [a, b][:c.G], [b, a][:c.G]
    else:                    # one target, two sources
        o.tgt, o.src = [a, a][:c.G], [b, b2][:c.G]
    for g in range(c.G):
        o.flow.append(pw_flow(c, g))
        if c.mode != 'border':
            fy, fx = c.fyx if c.mode == 'nearest' else (1, 1)
            m = mask_of(c.mask, c.B, c.H * fy, c.W * fx, seed=g)
            o.mask.append((1.0 - m) if c.invert else m)   # the plane the kernel inverts back: the same share of ones
    return o


def pw_mutations(c):
    mu = ['mean8', 'pool_after', 'c1c2']
    if c.C > 1:
        mu.append('chan_last')
    if c.G == 2:
        mu.append('half_tgt')
    if c.mode == 'plane' and c.mask == 'frac':
        mu.append('mask_once')
    if c.mode == 'nearest' and c.fyx[0] != c.fyx[1]:
        mu.append('nearest_fx')
    if c.mode == 'border' and c.invert:
        mu.append('invert_border')
    if c.mode == 'border' and c.field == 'edge':
        mu.append('border_closed')
    if c.field == 'exact':
        mu.append('sign0')
    if c.W - 2 > 63:
        mu += ['halo_col'] + (['anchor_shift'] if c.W - 2 > 64 else [])
    if c.H - 2 > 15:
        mu.append('halo_row')
    return mu


def pw_case_ref(c, mutate=None):
    i = pw_inputs(c)
    return photo_warp_ref(i.tgt, i.src, i.flow, i.mask, c.pad, c.mode, c.invert, c.coef, mutate)


# forward probes: B = 1, G = 2, a plane that is 1 at one pixel per group
PROBE_SHAPES = [(16, 64), (17, 65), (18, 66), (19, 67), (33, 130)]


def probe_pixels(H, W):
    """the corners, and the first and last two rows and columns of every 16 x 64 tile, crossed with a few positions"""
    ys = sorted({y for t in range(0, H, 16) for y in (t, t + 1, t + 14, t + 15) if y < H} | {0, H - 1, H - 2})
    xs = sorted({x for t in range(0, W, 64) for x in (t, t + 1, t + 62, t + 63) if x < W} | {0, W - 1, W - 2})
    px = {(y, x) for y in (0, H - 1) for x in (0, W - 1)}
    for k, y in enumerate(ys):
        px.add((y, xs[k % len(xs)]))
        px.add((y, xs[(k + 3) % len(xs)]))
    for k, x in enumerate(xs):
        px.add((ys[k % len(ys)], x))
        px.add((ys[(k + 2) % len(ys)], x))
    return sorted(px)


def probe_warp(i, g, pad):
    """rec (Iv) of group g of probe inputs: computed once per shape, every probe reads its neighbourhood out of it"""
    wr = warp_ref(i.src[g], i.flow[g], PAD[pad], True, NORM_ARFLOW)
    return Iv(wr.out, wr.bound_out)


def probe_ref(rec, tgt, y, x, mutate=None):
    """the three sums of one group under a plane that is 1 at (y, x) alone: the pixel's sum_c |tgt - rec|, the SSIM distance
    of the windows that hold it (every other window is all-zero: exactly 0), and 1.  Only the 5 x 5 neighbourhood enters."""
    _, C, H, W = tgt.shape
    y0, y1, x0, x1 = max(y - 2, 0), min(y + 3, H), max(x - 2, 0), min(x + 3, W)
    m = torch.zeros(1, 1, y1 - y0, x1 - x0, dtype=D)
    m[0, 0, y - y0, x - x0] = 1.0
    r = Iv(rec.v[:, :, y0:y1, x0:x1], rec.e[:, :, y0:y1, x0:x1])
    t = tgt[:, :, y0:y1, x0:x1].to(D)
    w = _win(_masked(r.v, m, r.e), _masked(t, m), 1, mutate, TILES['pw'], (y0, x0))
    l1 = _sub(_iv(t), r)
    l1 = _mul(Iv(l1.v.abs(), l1.e), _iv(m))
    T = n_tiles('pw', 1, H, W)
    return [_total(l1, depth('pw', 'l1', C, T)), _total(w.dist, depth('pw', 'ss', C, T)), _iv(torch.ones((), dtype=D))]


def probe_inputs(H, W, pad):
    """images, and per group a flow that sends taps outside, onto the border and onto integer coordinates"""
    c = _p('probe', 1, 2, 3, H, W, pad=pad, field='exact' if H > 22 else 'edge')
    i = pw_inputs(c)
    for g in range(2):
        i.flow[g][:, :, ::5, ::7] = torch.tensor([3.0, -2.0] if g == 0 else [-1.0, 1.0]).view(1, 2, 1, 1)   # integer
        i.flow[g][:, 0, :, :2] -= 4.0          # leaves on the left
        i.flow[g][:, 1, H - 2:, :] += 3.0      # leaves at the bottom
    return c, i
