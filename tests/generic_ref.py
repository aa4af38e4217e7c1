"""Shared by tests/test_generic_ref_cpu.py and tests/test_generic_gpu.py: float64 restatements, in plain torch on the CPU, of
the three kernel pairs of csrc/generic.hip that had no per-element pin -- the nearest warp, the bicubic warp and the general
correlation -- with the per-element error bounds the GPU tests hold the kernels to, the case lists and deliberate mutations.
Nothing here imports the oracle or the product.  The sampling coordinate, its fields and the case tuple come from
tests/warp_ref.py, the (value, bound) arithmetic from tests/photo_ref.py.  u = 2^-24, U1 = u (1 + 2^-20).

THE OPERATIONS
  Both warps take the fp32 sampling coordinate c of warp_ref.coords (af_sample_coord, one rounding per operation: part of the
  operation's definition) and do everything behind it in float64, so floor, nearbyint, the border clip and the tap validity
  are exact comparisons: no element is left out of any comparison and there is no exclusion cap.  NaN flows are left out (as in
  warp_ref: nothing to restate); coordinates of +-1e30 are in.
  nearest (generic.hip nearest_index, :17-31)
      border padding clips c to [0, n - 1]; r = nearbyint(c) (round half to EVEN); out = src[ry, rx] where 0 <= r <= n - 1 on
      both axes, else 0.  gsrc[q] = sum of g over the n_q pixels landing on q.  The flow gradient is exactly zero.
  bicubic (bicubic_taps / cubic_coeffs / cubic_coeffs_grad, :66-111; the kernels :113-172), A = -0.75
      f = floor(c), t = c - f; taps at f - 1 + i, i = 0..3; border padding clips EACH TAP's position to [0, n - 1] (not the
      coordinate), zeros padding reads 0 outside;  cx = cubic(tx), cy = cubic(ty) with
          cubic(t) = (w(t + 1), v(t), v(1 - t), w((1 - t) + 1))
          w(p) = ((A p - 5A) p + 8A) p - 4A,  v(x) = ((A + 2) x - (A + 3)) x x + 1
      row_j = ((v_j0 cx0 + v_j1 cx1) + v_j2 cx2) + v_j3 cx3,  out = ((row_0 cy0 + row_1 cy1) + row_2 cy2) + row_3 cy3
      gflow_x = dc/du_x * (0 - sum_c sum_{j, i: tap reads a value} ((v cx'_i) cy_j) g_c)   (y alike with cy'_j, cx_i)
          cx' = cubic'(t): the derivative of the four polynomials in the Horner forms of cubic_coeffs_grad.  The clipping
          of a tap's position is ignored (as in ATen: the value at the clipped position is used), a tap that reads zero is
          skipped.
      gsrc[c, q] = sum over the (pixel, tap) pairs landing on q of (g cx_i) cy_j

  general correlation (corr_general_fwd_kernel / corr_general_bwd_kernel, :297-367; geometry corr_general_cfg, :487-499)
      kr = (K - 1) / 2, dr = md / s2 (integer), ds = 2 dr + 1, Ho = ceil((H + 2 pad - 2 (kr + md)) / s1), Wo alike; p = the
      image in the frame padded by `pad`, ZERO everywhere else (also outside the padded frame);
      out[n, tc, oy, ox] = 1 / (K^2 C) sum_{j, i in [-kr, kr]} sum_c p1[c, y1 + j, x1 + i] p2[c, y1 + j + tj s2, x1 + i + ti s2]
          y1 = oy s1 + md, x1 = ox s1 + md, tc = (tj + dr) ds + (ti + dr)
      gx1[c, y, x] = 1 / (K^2 C) sum_tc sum_{j, i} [oy = (y + pad - md - j) / s1, ox alike, integral and in range]
                     gout[tc, oy, ox] p2[c, y + pad + tj s2, x + pad + ti s2]
      gx2[c, y, x] = 1 / (K^2 C) sum_tc sum_{j, i} [oy = (y + pad - tj s2 - j - md) / s1, ox alike, integral and in range]
                     gout[tc, oy, ox] p1[c, y + pad - tj s2, x + pad - ti s2]

BOUNDS.  Every fp32 operation of the kernels rounds once (-ffp-contract=off); quantities are carried as (value, bound) through
  the kernels' operations in the kernels' order with photo_ref's _add / _sub / _mul / _chain.  No constant is fitted.
  nearest forward      0: a copy.  The output equals the source value, or 0, bit for bit.
  nearest gsrc         n_q float atomics into the zero-filled tensor (the first onto 0.f is exact), any order:
                       (n_q - 1) U1 sum |g|.  Exactly 0 where n_q = 0, exact where n_q = 1.                      generic.hip:58
  bicubic t            c - f is exact in fp32 except in the cell [-1, 0), where it is c + 1: ONE rounding (warp_ref's BOUNDS
                       paragraph has the argument); carried as U1 t there.                                      generic.hip:95
  bicubic coefficients t + 1, 1 - t, (1 - t) + 1, -1 - t, 2 - t: one rounding each; then every *, +, - of the Horner forms in
                       the order written, one rounding each.  The intermediate terms cancel (w(1) = 0 through 3, -3, 0), so
                       the error comes out absolute, about 10 u, not relative to the coefficient.      generic.hip:66-84
                       t = 0 exactly: the fp32 coefficients are exactly (0, 1, 0, 0) (3 - 6 = -3, -3 + 3 = 0; 1.25 - 2.25 =
                       -1, -1 + 1 = 0; 2.25 2 - 6 = -1.5, -1.5 2 + 3 = 0): carried without error.
  bicubic forward      the products and sums of row_j and of the column, one rounding each, as written.  No tap inside the
                       source: value and bound 0.  Integer coordinates on both axes: the output is the source value bit for
                       bit, the bound is set to 0.                                                             generic.hip:130-132
  bicubic gflow        per term three products; one chain of n subtractions, n = C times the number of taps that read a
                       value (<= 16 C); then the product with dc/du (fp32, part of the coordinate's definition) :162-170
  bicubic gsrc         per pair two products, then n_q float atomics, any order: sum of the term bounds + n_q U1 sum |term|.
                       Exactly 0 where nothing lands.                                                          generic.hip:159
  correlation forward  one fmaf chain of n = K^2 C terms (each passes at most n roundings), then the IEEE division:
                       (n + 1) U1 sum |a b| / n.                                                               generic.hip:320-325
  correlation gx1, gx2 one fmaf chain over the n_t terms that are not identically zero (an fmaf with a zero factor leaves
                       the sum as it is), then the product with the rounded 1 / (K^2 C): (n_t + 2) U1 sum |g p| / (K^2 C);
                       n_t per element from this restatement run on ones.  No non-zero term: exactly 0.        generic.hip:340-365
  The grid-stride loops' cap of 65535 * 16 workgroups needs more than 2.6e8 outputs and is not exercised.

MUTATIONS (WRONG on purpose)
  nearest      'half_away' round half away from zero; 'floor_half' floor(c + 0.5); 'clip_after_round' the border clip applied to
               the rounded index AFTER the range test, so that border padding reads zero outside like zeros padding (a clip
               between the rounding and the range test cannot be told from the clip in front of the rounding: the end points
               are integers, and a monotone map that fixes the integers commutes with it); 'align'; 'nsrc_nflow'
  bicubic      'a_half' A = -0.5; 'clip_coord' border padding clips the coordinate (and zeroes dc/du there) as the bilinear
               warp does and no tap; 'tap_shift' taps at f + i; 'grad_counts_zero_taps' under zeros padding the flow gradient
               takes a tap outside the source at its clipped position instead of skipping it; 'align'; 'nsrc_nflow';
               'lose_pair' the first (pixel, tap) pair lost from gsrc
  correlation  'div_c' divides by C; 'swap_t' tc = (ti + dr) ds + (tj + dr); 'dr_md' dr = md; 'floor_size' a floor output size;
               'ext_bwd_window' the gradients sum over the output window floor((y' - kr - md) / s1) .. floor((y' + kr - md) / s1)
               of the CUDA extension's backward, whatever the offset inside the kernel window; 'pad_shift' y1 = oy s1
"""
import collections
import types

import torch
import torch.nn.functional as F

from tests import warp_ref as W
from tests.photo_ref import Iv, _add, _chain, _iv, _mul, _pick, _sub
from tests.warp_ref import D, F32, NORMS, PAD, U1, worst  # noqa: F401 (re-exported)

A_CUBIC = -0.75
NEAREST_MUTATIONS = ('half_away', 'floor_half', 'clip_after_round', 'align', 'nsrc_nflow')
BICUBIC_MUTATIONS = ('a_half', 'clip_coord', 'tap_shift', 'grad_counts_zero_taps', 'align', 'nsrc_nflow', 'lose_pair')
CORR_MUTATIONS = ('div_c', 'swap_t', 'dr_md', 'floor_size', 'ext_bwd_window', 'pad_shift')


def _coords(flow, Hs, Ws, norm, align, mutate, dtype):
    return W.coords(flow, Hs, Ws, norm, align, dtype, mutate if mutate in ('align', 'nsrc_nflow') else None)


# ======================================================================================================================
# nearest warp
# ======================================================================================================================
def _round(c, mutate):
    if mutate == 'half_away':
        return torch.sign(c) * torch.floor(c.abs() + 0.5)
    if mutate == 'floor_half':
        return torch.floor(c + 0.5)
    return torch.round(c)   # half to even, as nearbyintf in the default rounding mode


def nearest_ref(src, flow, pad, align, norm, gout=None, mutate=None, coord_dtype=F32):
    """src [B, C, Hs, Ws], flow [B, 2, H, W] fp32, gout [B, C, H, W] or None -> namespace (float64)
        out (Iv, bound 0), ok [B, H, W], idx [B, H, W] (flat source index), c = (ix, iy) as float64 (after the border clip);
        gsrc (Iv), nq [B, Hs, Ws], gflow (exactly zero) when gout is given.
    coord_dtype=float64 is for the comparison with F.grid_sample in float64 only."""
    assert mutate is None or mutate in NEAREST_MUTATIONS
    B, C, Hs, Ws = src.shape
    _, _, H, Wf = flow.shape
    ix, iy, _, _ = _coords(flow, Hs, Ws, norm, align, mutate, coord_dtype)
    ok = torch.ones(B, H, Wf, dtype=torch.bool)
    r, cs = [], []
    for c, n in ((ix, Ws), (iy, Hs)):
        c = c.to(D)
        if pad == PAD['border'] and mutate != 'clip_after_round':
            c = c.clamp(0.0, float(n - 1))
        rr = _round(c, mutate)
        ok &= (rr >= 0) & (rr <= n - 1)
        r.append(rr)
        cs.append(c)
    zero = torch.zeros_like(r[0])
    xi, yi = torch.where(ok, r[0], zero).long(), torch.where(ok, r[1], zero).long()
    if mutate == 'clip_after_round':   # after the range test: no effect
        xi, yi = xi.clamp(0, Ws - 1), yi.clamp(0, Hs - 1)
    idx = (yi * Ws + xi).reshape(B, 1, -1)
    okf = ok.reshape(B, 1, -1).to(D)
    s = src.to(D).reshape(B, C, Hs * Ws)
    out = (s.gather(2, idx.expand(B, C, H * Wf)) * okf).reshape(B, C, H, Wf)
    o = types.SimpleNamespace(out=_iv(out), ok=ok, idx=idx.reshape(B, H, Wf), c=tuple(cs))
    if gout is None:
        return o
    g = gout.to(D).reshape(B, C, H * Wf) * okf
    gs, A, nq = s.new_zeros(B, C, Hs * Ws), s.new_zeros(B, C, Hs * Ws), s.new_zeros(B, 1, Hs * Ws)
    gs.scatter_add_(2, idx.expand(B, C, H * Wf), g)
    A.scatter_add_(2, idx.expand(B, C, H * Wf), g.abs())
    nq.scatter_add_(2, idx, okf)
    o.gsrc = Iv(gs.reshape(B, C, Hs, Ws), ((nq - 1.0).clamp_min(0.0) * U1 * A).reshape(B, C, Hs, Ws))
    o.nq = nq.reshape(B, Hs, Ws)
    o.gflow = torch.zeros(B, 2, H, Wf, dtype=D)
    return o


def nearest_f32(src, flow, pad, align, norm, gout):
    """the same operation in plain fp32 on the CPU, in the kernel's order -> out, gsrc (fp32)"""
    B, C, Hs, Ws = src.shape
    _, _, H, Wf = flow.shape
    ix, iy, _, _ = W.coords(flow, Hs, Ws, norm, align)
    if pad == PAD['border']:
        ix, iy = ix.clamp(0.0, float(Ws - 1)), iy.clamp(0.0, float(Hs - 1))
    rx, ry = torch.round(ix), torch.round(iy)
    ok = (rx >= 0) & (rx <= Ws - 1) & (ry >= 0) & (ry <= Hs - 1)
    zero = torch.zeros_like(rx)
    idx = (torch.where(ok, ry, zero).long() * Ws + torch.where(ok, rx, zero).long()).reshape(B, 1, -1).expand(B, C, H * Wf)
    okf = ok.reshape(B, 1, -1).to(F32)
    out = src.reshape(B, C, -1).gather(2, idx) * okf
    gs = torch.zeros(B, C, Hs * Ws).scatter_add_(2, idx, gout.reshape(B, C, -1) * okf)
    return out.reshape(B, C, H, Wf), gs.reshape(B, C, Hs, Ws)


# ======================================================================================================================
# bicubic warp: one body, two arithmetics -- (value, bound) in float64, and plain fp32
# ======================================================================================================================
class _IvAlg:
    iv = True
    add, sub, mul = staticmethod(_add), staticmethod(_sub), staticmethod(_mul)

    @staticmethod
    def k(c):
        return _iv(torch.tensor(float(c), dtype=D))

    @staticmethod
    def lift(t):
        return _iv(t.to(D))

    @staticmethod
    def neg(a):
        return Iv(-a.v, a.e)


class _F32Alg:
    iv = False
    add, sub, mul = staticmethod(torch.add), staticmethod(torch.sub), staticmethod(torch.mul)

    @staticmethod
    def k(c):
        return torch.tensor(float(c), dtype=F32)

    @staticmethod
    def lift(t):
        return t.to(F32)

    @staticmethod
    def neg(a):
        return -a


def cubic_coeffs(t, al, A=A_CUBIC):
    """cubic_coeffs, generic.hip:66-73, operation by operation"""
    k, add, sub, mul = al.k, al.add, al.sub, al.mul
    one = k(1.0)

    def outer(p):   # ((A p - 5A) p + 8A) p - 4A
        return sub(mul(add(mul(sub(mul(k(A), p), k(5.0 * A)), p), k(8.0 * A)), p), k(4.0 * A))

    def inner(x):   # ((A + 2) x - (A + 3)) x x + 1
        return add(mul(mul(sub(mul(k(A + 2.0), x), k(A + 3.0)), x), x), one)
    x2 = sub(one, t)
    return [outer(add(t, one)), inner(t), inner(x2), outer(add(x2, one))]


def cubic_coeffs_grad(t, al, A=A_CUBIC):
    """cubic_coeffs_grad, generic.hip:74-84"""
    k, add, sub, mul = al.k, al.add, al.sub, al.mul
    x = sub(k(-1.0), t)
    g0 = sub(mul(sub(mul(k(-3.0 * A), x), k(10.0 * A)), x), k(8.0 * A))
    x = al.neg(t)
    g1 = mul(sub(mul(k(-3.0 * (A + 2.0)), x), k(2.0 * (A + 3.0))), x)
    x = sub(k(1.0), t)
    g2 = mul(sub(mul(k(3.0 * (A + 2.0)), x), k(2.0 * (A + 3.0))), x)
    x = sub(k(2.0), t)
    g3 = add(mul(sub(mul(k(3.0 * A), x), k(10.0 * A)), x), k(8.0 * A))
    return [g0, g1, g2, g3]


def _exact_coeffs(t, co):
    """where t is exactly 0 the fp32 coefficients are exactly (0, 1, 0, 0): carried without error"""
    at0 = (t.v == 0) & (t.e == 0)
    return [_pick(at0, _iv(torch.full_like(t.v, float(i == 1))), c) for i, c in enumerate(co)]


def _bicubic(src, flow, pad, align, norm, gout, mutate, al, coord_dtype=F32):
    B, C, Hs, Ws = src.shape
    _, _, H, Wf = flow.shape
    N = H * Wf
    A = -0.5 if mutate == 'a_half' else A_CUBIC
    ix, iy, dx, dy = _coords(flow, Hs, Ws, norm, align, mutate, coord_dtype)
    wide = D if al.iv else F32
    dxm = torch.full((B, N), float(dx), dtype=wide)
    dym = torch.full((B, N), float(dy), dtype=wide)
    border = pad == PAD['border']
    if mutate == 'clip_coord' and border:
        for c, n, dm in ((ix, Ws, dxm), (iy, Hs, dym)):
            dm[((c <= 0) | (c >= float(n - 1))).reshape(B, N)] = 0.0
            c.clamp_(0.0, float(n - 1))
        border = False
    o = types.SimpleNamespace()
    co, cg, pos, tt = [], [], [], []
    for c, n in ((ix, Ws), (iy, Hs)):
        c = c.reshape(B, N)
        f = torch.floor(c)
        if al.iv:   # float64 behind the fp32 coordinate; the one rounding of c + 1 in the cell [-1, 0)
            t64 = c.to(D) - f.to(D)
            t = Iv(t64, torch.where(f == -1, U1 * t64, torch.zeros_like(t64)) if coord_dtype == F32 else torch.zeros_like(t64))
            co.append(_exact_coeffs(t, cubic_coeffs(t, al, A)))
        else:
            t = c - f
            co.append(cubic_coeffs(t, al, A))
        cg.append(cubic_coeffs_grad(t, al, A))
        tt.append(t)
        first = f.to(D) + (0.0 if mutate == 'tap_shift' else -1.0)
        pos.append([first + i for i in range(4)])
    cx, cy = co
    gxc, gyc = cg
    o.exact = ((tt[0].v == 0) & (tt[1].v == 0)) if al.iv else None
    # taps: validity, flat index of the (clipped) position
    ok, idx = [[None] * 4 for _ in range(4)], [[None] * 4 for _ in range(4)]
    for j in range(4):
        for i in range(4):
            x, y = pos[0][i], pos[1][j]
            inside = (x >= 0) & (x <= Ws - 1) & (y >= 0) & (y <= Hs - 1)
            ok[j][i] = torch.ones_like(inside) if border else inside
            idx[j][i] = (y.clamp(0, Hs - 1).long() * Ws + x.clamp(0, Ws - 1).long())
    s = al.lift(src).v if al.iv else al.lift(src)
    s = s.reshape(B, C, Hs * Ws)

    def read(j, i, mask):
        return s.gather(2, idx[j][i].reshape(B, 1, N).expand(B, C, N)) * mask.reshape(B, 1, N).to(s.dtype)

    def per_pixel(a):   # [B, N] coefficient -> broadcast over channels
        return Iv(a.v.reshape(B, 1, N), a.e.reshape(B, 1, N)) if al.iv else a.reshape(B, 1, N)

    def wrap(t):
        return _iv(t) if al.iv else t
    v = [[wrap(read(j, i, ok[j][i])) for i in range(4)] for j in range(4)]
    cxp, cyp = [per_pixel(a) for a in cx], [per_pixel(a) for a in cy]
    add, mul, sub = al.add, al.mul, al.sub
    rows = [add(add(add(mul(v[j][0], cxp[0]), mul(v[j][1], cxp[1])), mul(v[j][2], cxp[2])), mul(v[j][3], cxp[3]))
            for j in range(4)]
    out = add(add(add(mul(rows[0], cyp[0]), mul(rows[1], cyp[1])), mul(rows[2], cyp[2])), mul(rows[3], cyp[3]))
    if al.iv:
        e = out.e * (~o.exact).reshape(B, 1, N).to(D)
        o.out = Iv(out.v.reshape(B, C, H, Wf), e.reshape(B, C, H, Wf))
    else:
        o.out = out.reshape(B, C, H, Wf)
    if gout is None:
        return o
    g = al.lift(gout)
    g = Iv(g.v.reshape(B, C, N), g.e.reshape(B, C, N)) if al.iv else g.reshape(B, C, N)
    # ---- flow gradient: one subtraction chain over c, j, i
    gxp, gyp = [per_pixel(a) for a in gxc], [per_pixel(a) for a in gyc]
    tx_terms, ty_terms = [], []
    ntap = torch.zeros(B, N, dtype=D)
    for j in range(4):
        for i in range(4):
            m = torch.ones_like(ok[j][i]) if (mutate == 'grad_counts_zero_taps' and not border) else ok[j][i]
            vv = wrap(read(j, i, m))
            ntap += m.to(D)
            tx_terms.append(mul(mul(mul(vv, gxp[i]), cyp[j]), g))
            ty_terms.append(mul(mul(mul(vv, gyp[j]), cxp[i]), g))
    if al.iv:
        def total(terms, dm):
            st = Iv(torch.stack([t.v for t in terms]), torch.stack([t.e for t in terms]))   # [16, B, C, N]
            flat = Iv(st.v.permute(0, 2, 1, 3).reshape(16 * C, B, N), st.e.permute(0, 2, 1, 3).reshape(16 * C, B, N))
            chain = _chain(flat, ntap * C)
            return mul(Iv(dm, torch.zeros_like(dm)), Iv(-chain.v, chain.e))
        gx, gy = total(tx_terms, dxm), total(ty_terms, dym)
        o.gflow = Iv(torch.stack([gx.v, gy.v], 1).reshape(B, 2, H, Wf), torch.stack([gx.e, gy.e], 1).reshape(B, 2, H, Wf))
    else:
        gix, giy = torch.zeros(B, N), torch.zeros(B, N)
        for c in range(C):
            for k in range(16):
                gix = gix - tx_terms[k][:, c]
                giy = giy - ty_terms[k][:, c]
        o.gflow = torch.stack([dxm * gix, dym * giy], 1).reshape(B, 2, H, Wf)
    # ---- source gradient: (g cx_i) cy_j scattered
    gs = torch.zeros(B, C, Hs * Ws, dtype=wide)
    E, Asum, nq = gs.clone(), gs.clone(), torch.zeros(B, 1, Hs * Ws, dtype=D)
    lost = mutate != 'lose_pair'
    for j in range(4):
        for i in range(4):
            m = ok[j][i].reshape(B, 1, N).clone()
            if not lost and bool(m.any()):
                m.view(-1)[int(torch.nonzero(m.view(-1))[0])] = False
                lost = True
            term = mul(mul(g, cxp[i]), cyp[j])
            ind = idx[j][i].reshape(B, 1, N)
            mf = m.to(wide)
            if al.iv:
                gs.scatter_add_(2, ind.expand(B, C, N), term.v * mf)
                E.scatter_add_(2, ind.expand(B, C, N), term.e * mf)
                Asum.scatter_add_(2, ind.expand(B, C, N), (term.v.abs() + term.e) * mf)
                nq.scatter_add_(2, ind, m.to(D))
            else:
                gs.scatter_add_(2, ind.expand(B, C, N), term * mf)
    if al.iv:
        o.gsrc = Iv(gs.reshape(B, C, Hs, Ws), ((E + nq * U1 * Asum) * (nq > 0).to(D)).reshape(B, C, Hs, Ws))
        o.nq = nq.reshape(B, Hs, Ws)
    else:
        o.gsrc = gs.reshape(B, C, Hs, Ws)
    return o


def bicubic_ref(src, flow, pad, align, norm, gout=None, mutate=None, coord_dtype=F32):
    """-> namespace out, gflow, gsrc (Iv: float64 value, bound), nq [B, Hs, Ws], exact [B, H W] (integer coordinates)"""
    assert mutate is None or mutate in BICUBIC_MUTATIONS
    return _bicubic(src, flow, pad, align, norm, gout, mutate, _IvAlg, coord_dtype)


def bicubic_f32(src, flow, pad, align, norm, gout):
    """the same operation in plain fp32 on the CPU, every operation in the kernel's order -> out, gflow, gsrc (fp32)"""
    return _bicubic(src, flow, pad, align, norm, gout, None, _F32Alg)


# ======================================================================================================================
# warp cases (warp_ref.Case; its fwd / src / split labels are not used here)
# ======================================================================================================================
def _w(name, B, C, H, Wf, field, args=(), Hs=None, Ws=None, norm='arflow', align=True, pad='zeros'):
    return W._c(name, B, C, H, Wf, field, args, '-', src='-', Hs=Hs, Ws=Ws, norm=norm, align=align, pad=pad)


FIELDS = (('noise', (2.5,)), ('stretch', (1.3, 0.8, -1.7, 1.2)), ('half', ()), ('exact', ()), ('far', (1e4,)))
# every field x padding x align flag on 9 x 13, B3 C5
BASE_CASES = [_w('%s %s align=%s' % (f, p, a), 3, 5, 9, 13, f, args, align=a, pad=p)
              for f, args in FIELDS for p in ('zeros', 'border') for a in (True, False)]
# the source extent differs from the flow's: every norm, both paddings (and both align flags on the first)
SIZE_CASES = (
    [_w('7x12->11x10 noise %s %s align=%s' % (n, p, a), 2, 3, 7, 12, 'noise', (2.5,), Hs=11, Ws=10, norm=n, pad=p, align=a)
     for n in NORMS for p in ('zeros', 'border') for a in (True, False)]
    + [_w('7x12->4x17 noise %s %s' % (n, p), 2, 3, 7, 12, 'noise', (2.5,), Hs=4, Ws=17, norm=n, pad=p)
       for n in NORMS for p in ('zeros', 'border')]
    + [_w('7x12->11x10 half %s' % n, 2, 3, 7, 12, 'half', (), Hs=11, Ws=10, norm=n, pad='border') for n in NORMS]
)
# two workgroups in x with one lane in the second; exactly one workgroup
WIDE_CASES = [_w('5x257', 1, 1, 5, 257, 'stretch', (1.01, 1.1, -1.5, -0.6)),
              _w('3x256', 2, 2, 3, 256, 'stretch', (0.99, 0.9, 1.5, 0.3), pad='border')]
# a one-pixel source axis: border padding clamps to index 0.  Norm ARFLOW with align_corners multiplies by n_src - 1 = 0 and
# the field builder would divide by it: align=False there, and UFLOW (its max(n - 1, 1)) next to it
THIN_CASES = (
    [_w('6x9->%dx%d arflow %s' % (hs, ws, p), 2, 3, 6, 9, 'stretch', (0.9, 0.8, -0.7, 0.6), Hs=hs, Ws=ws, align=False, pad=p)
     for hs, ws in ((1, 9), (6, 1)) for p in ('zeros', 'border')]
    + [_w('6x9->%dx%d uflow border' % (hs, ws), 2, 3, 6, 9, 'noise', (1.5,), Hs=hs, Ws=ws, norm='uflow', pad='border')
       for hs, ws in ((1, 9), (6, 1))]
    # a one-pixel FLOW axis under norm UFLOW.  Norm ARFLOW divides by n_flow - 1 = 0 there, as the reference does: left out
    + [_w('%dx%d uflow %s' % (h, w, p), 1, 2, h, w, 'noise', (1.5,), norm='uflow', pad=p)
       for h, w in ((1, 8), (8, 1)) for p in ('zeros', 'border')]
)
# every pixel onto one source cell: n_q = 117 for nearest, 16 cells of n_q = 117 for bicubic
POINT_CASES = [_w('point %s' % p, 1, 2, 9, 13, 'point', (6.25, 3.25, False), pad=p) for p in ('zeros', 'border')]
# 9 x 13 divides by 12 and 8: the round trip of the coordinate does not reach every special value there (a fifth of the
# targets is missed by an ulp, 0 itself without align_corners).  64 x 16 with align_corners and 65 x 17 over a 64 x 16 source
# without (warp_ref.EXACT_CASES: the divisors are powers of two, the coordinate is p + u - 1/2 exactly) reach all of them.
EXACT_EXTRA = [_w('exact 16x64 %s' % p, 1, 2, 16, 64, 'exact', (), pad=p) for p in ('zeros', 'border')] + [
    _w('exact 17x65->16x64 align=False %s' % p, 1, 2, 17, 65, 'exact', (), Hs=16, Ws=64, align=False, pad=p)
    for p in ('zeros', 'border')]
WARP_CASES = BASE_CASES + SIZE_CASES + WIDE_CASES + THIN_CASES + POINT_CASES + EXACT_EXTRA
# the flow consumed out of channels 2:4 of a [B, 4, H, W] tensor
STRIDED_CASE = _w('strided', 2, 3, 9, 13, 'noise', (2.5,), pad='border', align=False)
WARP_BY_NAME = {c.name: c for c in WARP_CASES + [STRIDED_CASE]}
_warp_cache = {}


def warp_case(case):
    """-> src, flow, gout (fp32), nearest_ref, bicubic_ref: computed once per process and left unchanged"""
    if case.name not in _warp_cache:
        src, flow, gout = W.inputs(case)
        a = (src, flow, PAD[case.pad], case.align, NORMS[case.norm], gout)
        _warp_cache[case.name] = (src, flow, gout, nearest_ref(*a), bicubic_ref(*a))
    return _warp_cache[case.name]


# ======================================================================================================================
# general correlation
# ======================================================================================================================
def corr_geometry(H, Wd, cfg, mutate=None):
    """corr_general_cfg, generic.hip:487-499 -> kr, dr, Ho, Wo"""
    pad, K, md, s1, s2 = cfg
    kr = (K - 1) // 2
    dr = md if mutate == 'dr_md' else md // s2
    ph, pw = H + 2 * pad - 2 * (kr + md), Wd + 2 * pad - 2 * (kr + md)
    if mutate == 'floor_size':
        return kr, dr, ph // s1, pw // s1
    return kr, dr, -(-ph // s1), -(-pw // s1)


def _fma(a, b, s):
    """fmaf on fp32 tensors: the product of two fp32 numbers is exact in float64"""
    return (a.double() * b.double() + s.double()).float()


def _frame(x, pad, margin):
    """the zero-extended padded frame: frame coordinate Y sits at array index Y + margin"""
    return F.pad(x, [pad + margin] * 4)


def _corr_forward(x1, x2, cfg, mutate=None, f32=False):
    """-> out, sum |a b| [B, ds^2, Ho, Wo] (float64), or the fp32 evaluation in the kernel's order (fmaf chain, division)"""
    pad, K, md, s1, s2 = cfg
    B, C, H, Wd = x1.shape
    kr, dr, Ho, Wo = corr_geometry(H, Wd, cfg, mutate)
    ds = 2 * dr + 1
    M = kr + dr * s2 + s1 + md
    dt = F32 if f32 else D
    P1, P2 = _frame(x1.to(dt), pad, M), _frame(x2.to(dt), pad, M)
    ys = torch.arange(Ho) * s1 + (0 if mutate == 'pad_shift' else md) + M
    xs = torch.arange(Wo) * s1 + (0 if mutate == 'pad_shift' else md) + M
    out = torch.zeros(B, ds * ds, Ho, Wo, dtype=dt)
    mag = torch.zeros(B, ds * ds, Ho, Wo, dtype=D)
    for tj in range(-dr, dr + 1):
        for ti in range(-dr, dr + 1):
            tc = (ti + dr) * ds + (tj + dr) if mutate == 'swap_t' else (tj + dr) * ds + (ti + dr)
            acc = torch.zeros(B, Ho, Wo, dtype=dt)
            for j in range(-kr, kr + 1):
                for i in range(-kr, kr + 1):
                    a = P1[:, :, (ys + j)[:, None], (xs + i)[None, :]]
                    b = P2[:, :, (ys + j + tj * s2)[:, None], (xs + i + ti * s2)[None, :]]
                    if f32:
                        for c in range(C):
                            acc = _fma(a[:, c], b[:, c], acc)
                    else:
                        acc = acc + (a * b).sum(1)
                        mag[:, tc] += (a * b).abs().sum(1)
            den = torch.tensor(float(K * K * C), dtype=F32) if f32 else float(C if mutate == 'div_c' else K * K * C)
            out[:, tc] = acc / den
    return out, mag


def _slots(Yv, n_out, kr, md, s1, ext):
    """for frame rows Yv (role coordinate y1 + j = Yv): the output rows that read them, as (index, mask) pairs.
    The gradient of the forward: one per offset j with (Yv - md - j) / s1 integral and in range.  ext (the mutation): every
    row of the window floor((Yv - kr - md) / s1) .. floor((Yv + kr - md) / s1)."""
    res = []
    if ext:
        lo = torch.div(Yv - kr - md, s1, rounding_mode='floor')
        hi = torch.div(Yv + kr - md, s1, rounding_mode='floor')
        for a in range(2 * kr // s1 + 2):
            o = lo + a
            res.append((o.clamp(0, n_out - 1), (o <= hi) & (o >= 0) & (o < n_out)))
        return res
    for j in range(-kr, kr + 1):
        n = Yv - md - j
        o = torch.div(n, s1, rounding_mode='floor')
        res.append((o.clamp(0, n_out - 1), (n >= 0) & (n % s1 == 0) & (o < n_out)))
    return res


def _corr_backward(gout, x1, x2, cfg, mutate=None, f32=False):
    """the explicit gather formulas -> (gx1, sum |g p|), (gx2, sum |g p|) in float64; with f32 the kernel's fmaf chains
    (tc, j, i ascending) and the product with the rounded 1 / (K^2 C), the magnitudes then None"""
    pad, K, md, s1, s2 = cfg
    B, C, H, Wd = x1.shape
    kr, dr, Ho, Wo = corr_geometry(H, Wd, cfg, mutate)
    ds = 2 * dr + 1
    assert tuple(gout.shape) == (B, ds * ds, Ho, Wo)
    M = kr + dr * s2 + s1 + md
    dt = F32 if f32 else D
    P1, P2 = _frame(x1.to(dt), pad, M), _frame(x2.to(dt), pad, M)
    g = gout.to(dt)
    Y, X = torch.arange(H) + pad, torch.arange(Wd) + pad
    ext = mutate == 'ext_bwd_window'
    acc = [torch.zeros(B, C, H, Wd, dtype=dt) for _ in range(2)]
    mag = [torch.zeros(B, C, H, Wd, dtype=D) for _ in range(2)]
    for tc in range(ds * ds):
        a, b = tc // ds - dr, tc % ds - dr
        tj, ti = ((b, a) if mutate == 'swap_t' else (a, b))
        tj, ti = tj * s2, ti * s2
        gt = g[:, tc]
        shift = 0 if mutate != 'pad_shift' else md   # y1 = oy s1: the role coordinate moves by md
        for role, sy, sx, P in ((0, 0, 0, P2), (1, -tj, -ti, P1)):
            # role 0 (x1): (Y, X) = (y1 + j, x1 + i), partner p2 at (Y + tj, X + ti)
            # role 1 (x2): (Y, X) = (y1 + j + tj, x1 + i + ti), partner p1 at (Y - tj, X - ti)
            py, px = (Y + tj, X + ti) if role == 0 else (Y - tj, X - ti)
            partner = P[:, :, (py + M)[:, None], (px + M)[None, :]]
            rows = _slots(Y + sy + shift, Ho, kr, md, s1, ext)
            cols = _slots(X + sx + shift, Wo, kr, md, s1, ext)
            for oy, my in rows:
                for ox, mx in cols:
                    m = (my[:, None] & mx[None, :]).to(dt)
                    gsel = (gt[:, oy][:, :, ox] * m).unsqueeze(1)
                    if f32:
                        acc[role] = _fma(gsel.expand_as(partner), partner, acc[role])
                    else:
                        acc[role] += gsel * partner
                        mag[role] += (gsel * partner).abs()
    den = float(C if mutate == 'div_c' else K * K * C)
    if f32:
        inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(K * K * C), dtype=F32)
        return (acc[0] * inv, None), (acc[1] * inv, None)
    return (acc[0] / den, mag[0]), (acc[1] / den, mag[1])


def corr_general_ref(x1, x2, cfg, gout=None, mutate=None):
    """x1, x2 [B, C, H, W] fp32, cfg = (pad, K, md, s1, s2), gout [B, ds^2, Ho, Wo] or None
    -> namespace out, gx1, gx2 (Iv: float64 value, bound), nt1, nt2 (terms per gradient element), geometry (kr, dr, Ho, Wo)"""
    assert mutate is None or mutate in CORR_MUTATIONS
    pad, K, md, s1, s2 = cfg
    B, C, H, Wd = x1.shape
    n = K * K * C
    out, mag = _corr_forward(x1, x2, cfg, mutate)
    o = types.SimpleNamespace(out=Iv(out, (n + 1) * U1 * mag / n), geometry=corr_geometry(H, Wd, cfg, mutate))
    if gout is None:
        return o
    (g1, m1), (g2, m2) = _corr_backward(gout, x1, x2, cfg, mutate)
    one = torch.ones_like(x1)
    (c1, _), (c2, _) = _corr_backward(torch.ones_like(gout), one, one, cfg, mutate)   # run on ones: the count of terms / n
    o.nt1, o.nt2 = (c1 * n).round(), (c2 * n).round()
    o.gx1 = Iv(g1, (o.nt1 + 2) * (o.nt1 > 0).to(D) * U1 * m1 / n)
    o.gx2 = Iv(g2, (o.nt2 + 2) * (o.nt2 > 0).to(D) * U1 * m2 / n)
    return o


def corr_general_f32(x1, x2, cfg, gout):
    """plain fp32 on the CPU in the kernels' order -> out, gx1, gx2"""
    out, _ = _corr_forward(x1, x2, cfg, f32=True)
    (g1, _), (g2, _) = _corr_backward(gout, x1, x2, cfg, f32=True)
    return out, g1, g2


CorrCase = collections.namedtuple('CorrCase', 'name B C H W cfg')


def _k(B, C, H, Wd, cfg):
    return CorrCase('B%d C%d %dx%d pad%d K%d md%d s1_%d s2_%d' % ((B, C, H, Wd) + cfg), B, C, H, Wd, cfg)


CORR_DEFAULT = (4, 1, 4, 1, 1)
CORR_CASES = [
    _k(2, 3, 13, 12, CORR_DEFAULT),     # the tuned kernels' configuration: must agree with AF.correlation
    _k(2, 3, 13, 12, (0, 1, 2, 1, 1)),  # no padding: the output is smaller than the input
    _k(2, 3, 13, 12, (7, 3, 4, 1, 2)),  # pad > kr + md: the output's border lies wholly in the zero padding
    _k(2, 3, 13, 12, (3, 3, 2, 2, 2)),
    _k(2, 3, 13, 12, (2, 5, 3, 3, 2)),  # s2 does not divide md; ceil != floor for the output height
    _k(2, 3, 13, 12, (5, 3, 4, 2, 1)),
    _k(2, 3, 13, 12, (1, 3, 0, 1, 1)),  # md = 0: one output channel
    _k(2, 1, 13, 12, CORR_DEFAULT),     # C = 1
    _k(1, 2, 20, 300, (1, 3, 1, 1, 1)),  # the flat index spans several workgroups, forward and backward
]
_corr_cache = {}


def corr_inputs(case):
    gen = W._gen(211, case.B, case.C, case.H, case.W, *case.cfg)
    x1 = torch.randn(case.B, case.C, case.H, case.W, generator=gen)
    x2 = torch.randn(case.B, case.C, case.H, case.W, generator=gen)
    kr, dr, Ho, Wo = corr_geometry(case.H, case.W, case.cfg)
    gout = torch.randn(case.B, (2 * dr + 1) ** 2, Ho, Wo, generator=gen)
    return x1, x2, gout


def corr_case(case):
    """-> x1, x2, gout (fp32), corr_general_ref: computed once per process and left unchanged"""
    if case.name not in _corr_cache:
        x1, x2, gout = corr_inputs(case)
        _corr_cache[case.name] = (x1, x2, gout, corr_general_ref(x1, x2, case.cfg, gout))
    return _corr_cache[case.name]
