"""Shared by tests/test_warp_ref_cpu.py and tests/test_warp_gpu.py: a float64 restatement, in plain torch on the CPU, of the
bilinear flow warp (csrc/warp.hip with csrc/taps.hpp and csrc/common.hpp; its deterministic source gradient in
csrc/det_scatter.hip) -- forward, `valid` map, flow gradient and source gradient -- together with the per-element error
bounds the GPU tests hold the kernels to, the launch predicates of the kernels restated, the case lists, their fields and
deliberate mutations.  Nothing here imports the oracle or the product.

Reference arithmetic: utils/warp_utils.py:7-23, 83-90 (flow_warp), utils/uflow_utils.py:6-77 (flow_to_warp, mask_invalid,
resample) and ATen/native/GridSampler.h:27-83, which they call.  u = 2^-24 is the unit roundoff of fp32.

THE OPERATION
    coordinate (fp32, ONE rounding per operation: it is part of the operation's definition -- the reference itself forms it
    in fp32 through its normalise / un-normalise round trip, af_sample_coord / af_clip_border of common.hpp claim to
    reproduce it bit for bit; coord_axis below is that statement, and the kernels must agree with it to the bit):
        norm ARFLOW     g = 2 (p + u) / (n_flow - 1) - 1;  c = ((g + 1) / 2) (n_src - 1)        [align_corners]
                                                           c = ((g + 1) n_src - 1) / 2          [not]
                        dc/du = (2 / (n_flow - 1)) ((n_src - 1) / 2  or  n_src / 2)
        norm UFLOW      g = 2 (p + u) / max(n_src - 1, 1) - 1;  c = ((g + 1) / 2) (n_src - 1)   (the align flag is not read)
                        dc/du = (2 / max(n_src - 1, 1)) ((n_src - 1) / 2)
        norm UFLOW_ABS  as UFLOW with `u` the absolute position (p is not added)
        border padding  c <= 0 -> 0, c >= n_src - 1 -> n_src - 1, and dc/du = 0 there (fp32 comparisons: exact)
    everything behind the coordinate is float64 here:
        f = floor(c), w1 = c - f, w0 = (f + 1) - c  (exact in float64; in fp32 exact outside the two cells around 0, see BOUNDS)
        tap k = (x0 + (k & 1), y0 + (k >> 1)), weight w_k = wx[k & 1] wy[k >> 1], inside the source or not (exact)
        out[c, p]   = sum_k inside_k w_k src[c, tap_k]
        valid[p]    = 0 <= fp32(p + u) <= n_flow - 1 on both axes (ABS: u itself) -- the FLOW's extents, exact
        gflow_x[p]  = dc/du_x sum_c g[c, p] ((v1 - v0) wy0 + (v3 - v2) wy1),   v_k = src[c, tap_k] or 0 outside
        gflow_y[p]  = dc/du_y sum_c g[c, p] ((v2 - v0) wx0 + (v3 - v1) wx1)
        gsrc[c, q]  = sum over the (pixel p, tap k) pairs that land on q of w_k(p) g[c, p]
    Since floor is taken of the SAME fp32 number on both sides, floor, the border clip, the tap validity and `valid` are
    exact comparisons, and the flow gradient is defined at exactly integer coordinates too: the one-sided derivative of
    the cell floor picks, as in ATen.  No element is left out of any comparison and there is no exclusion cap.
    NaN flows are left out: the reference's cast of floor(NaN) to an integer is undefined behaviour, there is nothing
    to restate.  Coordinates of +-1e30 are in (the 'exact' fields): every tap is outside, (f + 1) - c = 0.

BOUNDS (U1 = u (1 + 2^-20): the second-order terms of (1 + u)^k, k <= 300, and this file's own float64 roundings)
  The weights.  w1 = c - f is exact in fp32 (Sterbenz for c >= 1; c itself or c + 1 in the two cells around 0 -- the
    latter is NOT: see below).  w0 = (f + 1) - c is exact wherever |c| >= 1/2, but in the first cell it is 1 - c, and for
    0 < c < 1/2 that difference needs bits below 2^-24: ONE rounding.  In the cell [-1, 0) it is w1 = c + 1 that rounds.
    So in the cells next to 0, on each axis, one weight carries a rounding (taps.hpp make_taps :26-29); float64 holds
    all of them exactly.  The longest path of every bound below runs through such a pixel: + 1 per axis.
  Forward, K_F = 7:  |out - ref| <= K_F U1 sum_k inside_k |w_k src_k|.  Longest path, the north-west tap:
        wx0, wy0 (first cell)        2   (taps.hpp:27, :29)
        w_0 = wx0 * wy0              1   (plan_taps, taps.hpp:53)
        a_0 * w_0                    1   (tap_blend, taps.hpp:62)
        three fmaf of the later taps 3   (taps.hpp:63-65: each rounds the running sum once)
    A tap outside adds nothing (the select keeps r).  No tap inside: the bound is 0, the output exactly 0.  Integer
    coordinates on both axes (all of border padding's clipped pixels are): every w_k is 0 or 1, every product and sum
    is exact -- the bound is set to 0 there (`exact`), the output equals the source value bit for bit.
    The staged window (LDS) and the direct gathers feed the same tap_blend: one bound.
  valid: exact.
  Flow gradient, K_G = 5, n_c = C:
        |gflow_x - ref| <= (K_G + n_c) U1 |dc/du_x| sum_c |g_c| ((|v1| + |v0|) wy0 + (|v3| + |v2|) wy1)
    (y alike) -- tap_corner_grad (taps.hpp:82-85) with absolute values:
        wy0 (first cell)             1
        v1 - v0                      1
        (..) * wy0                   1
        the sum of the two products  1   (-ffp-contract=off: no fma here)
        gix = fmaf(g, sx, gix)       n_c = C: a term passes through at most C roundings of the chain (warp.hip:487, :582)
        gix * t.dx                   1   (flow_grad::total, warp.hip:524)
    A channel split (gridDim.y = s > 1) shortens each chain to <= C / s + 1 channels and adds the s partial products
    into the zero-filled tensor with float atomics in any order (flow_grad::store): s - 1 more roundings, and
    C / s + 1 + s - 1 <= C for every C >= 8 the split is taken at.  dc/du is part of the coordinate's definition (fp32,
    two roundings, restated in coord_axis); where the border clip is active it is 0 and the result exactly 0.
  Source gradient, K_S = 4:  |gsrc[c, q] - ref| <= (n_q + K_S) U1 sum over the n_q pairs of |w_k g|.
        wx, wy (first cell)          2
        w_k = wx * wy                1   (warp.hip:838; plan_taps for the deterministic kernel)
        n_t fmaf of the tile's list  n_t (warp.hip:1005; direct atomics: the product g * w, 1, and one atomic each)
        one float atomic per tile and cell into the zero-filled tensor, T tiles: <= T roundings, any order
    A term passes through its own tile's n_t and at most T atomics; every other tile holds at least one pair, so
    n_t + T <= n_q + 1.  Deterministic mode (det_scatter.hip:148) is one chain of n_q fmaf: n_q + 3.  A cell nothing lands
    on has n_q = 0 and is exactly 0 in both modes (zero-fill resp. the owner's plain store of acc = 0).
  bf16 storage: the source is rounded to bf16 first (bf16_round); the kernels widen it exactly, the same bounds hold.
  Coordinate against float64 (CPU test only), K_C = 6:  |c32 - c64| <= K_C u (|c| + n_src).  Per operation, in units of
    the coordinate: p + u and the division 2 u (|c| + 1/2); g = q - 1: u (|c| + 1/2 + n / 2); g + 1: u (|c| + 1/2); the
    product with n_src: u (|c| + 1/2); - 1: u |c|; the halvings are exact.  6 u |c| + u (n / 2 + 2) <= 6 u (|c| + n).
"""
import collections
import types

import torch

from tests.loss_kernels_ref import D, U, _gen, worst  # noqa: F401 (re-exported)

F32 = torch.float32
U1 = U * (1.0 + 2.0 ** -20)
K_F, K_G, K_S, K_C = 7, 5, 4, 6
NORM_ARFLOW, NORM_UFLOW, NORM_UFLOW_ABS = 0, 1, 2
NORMS = {'arflow': NORM_ARFLOW, 'uflow': NORM_UFLOW, 'abs': NORM_UFLOW_ABS}
PAD = {'zeros': 0, 'border': 1}
MUTATIONS = ('tap_col', 'tap_row', 'drop_se', 'swap_w', 'align', 'border_grad', 'nsrc_nflow', 'tail_double', 'lose_pair')


def bf16_round(t):
    return t.to(torch.bfloat16).float()


# ======================================================================================================================
# coordinates
# ======================================================================================================================
def _t(v, dtype):
    return torch.tensor(float(v), dtype=dtype)


def coord_axis(p, u, n_flow, n_src, norm, align, dtype=F32):
    """af_sample_coord (common.hpp:171-184) in `dtype`, one rounding per operation.  p, u: tensors of `dtype`.
    -> (coordinate, dc/du as a 0-dim tensor of `dtype`)"""
    if norm != NORM_ARFLOW:
        den = _t(max(n_src - 1, 1), dtype)
        pos = u if norm == NORM_UFLOW_ABS else p + u
        g = (2.0 * pos) / den - 1.0
        dc = (_t(2.0, dtype) / den) * (_t(n_src - 1, dtype) / 2.0)
        return ((g + 1.0) / 2.0) * _t(n_src - 1, dtype), dc
    den = _t(n_flow - 1, dtype)
    g = (2.0 * (p + u)) / den - 1.0
    dc = (_t(2.0, dtype) / den) * ((_t(n_src - 1, dtype) if align else _t(n_src, dtype)) / 2.0)
    if align:
        return ((g + 1.0) / 2.0) * _t(n_src - 1, dtype), dc
    return ((g + 1.0) * _t(n_src, dtype) - 1.0) / 2.0, dc


def coords(flow, Hs, Ws, norm, align, dtype=F32, mutate=None):
    """flow [B, 2, H, W] fp32 -> ix, iy [B, H, W] and the two dc/du, in `dtype` (fp32: the operation's definition;
    float64: what the CPU test compares it with).  mutate (WRONG on purpose): 'align', 'nsrc_nflow'."""
    B, _, H, W = flow.shape
    if mutate == 'align':
        align = not align
    xs = torch.arange(W, dtype=dtype).view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H, dtype=dtype).view(1, H, 1).expand(B, H, W)
    fl = flow.to(dtype)
    nfx, nsx, nfy, nsy = (Ws, W, Hs, H) if mutate == 'nsrc_nflow' else (W, Ws, H, Hs)
    ix, dx = coord_axis(xs, fl[:, 0], nfx, nsx, norm, align, dtype)
    iy, dy = coord_axis(ys, fl[:, 1], nfy, nsy, norm, align, dtype)
    return ix, iy, dx, dy


def valid_ref(flow, norm):
    """[B, 1, H, W] float64 of 0 / 1: mask_invalid(flow_to_warp(flow)) with the sum taken in fp32 (warp.hip:239-244)"""
    B, _, H, W = flow.shape
    xs = torch.arange(W, dtype=F32).view(1, 1, W)
    ys = torch.arange(H, dtype=F32).view(1, H, 1)
    cx = flow[:, 0] if norm == NORM_UFLOW_ABS else xs + flow[:, 0]
    cy = flow[:, 1] if norm == NORM_UFLOW_ABS else ys + flow[:, 1]
    return ((cx >= 0) & (cx <= float(W - 1)) & (cy >= 0) & (cy <= float(H - 1))).unsqueeze(1).to(D)


def _taps(flow, Hs, Ws, pad, align, norm, mutate=None):
    """the four taps of every pixel, from the fp32 coordinate on in float64"""
    ix, iy, dx, dy = coords(flow, Hs, Ws, norm, align, F32, mutate if mutate in ('align', 'nsrc_nflow') else None)
    dxm = torch.full(ix.shape, float(dx), dtype=D)
    dym = torch.full(iy.shape, float(dy), dtype=D)
    if pad == PAD['border']:  # af_clip_border, common.hpp:188-199
        for c, n, dm in ((ix, Ws, dxm), (iy, Hs, dym)):
            clipped = (c <= 0) | (c >= float(n - 1))
            c.clamp_(0.0, float(n - 1))
            if mutate != 'border_grad':
                dm[clipped] = 0.0
    ix, iy = ix.to(D), iy.to(D)
    fx, fy = torch.floor(ix), torch.floor(iy)
    t = types.SimpleNamespace(ix=ix, iy=iy, dx=dxm, dy=dym)
    t.wx = (fx + 1.0 - ix, ix - fx)
    t.wy = (fy + 1.0 - iy, iy - fy)
    t.exact = (ix == fx) & (iy == fy)
    t.vx = ((fx >= 0) & (fx <= Ws - 1), (fx + 1 >= 0) & (fx + 1 <= Ws - 1))
    t.vy = ((fy >= 0) & (fy <= Hs - 1), (fy + 1 >= 0) & (fy + 1 <= Hs - 1))
    # north-west corner as an integer; pixels without a valid tap on an axis get 0 (taps.hpp:35-36)
    t.x0 = torch.where(t.vx[0] | t.vx[1], fx, torch.zeros_like(fx)).long()
    t.y0 = torch.where(t.vy[0] | t.vy[1], fy, torch.zeros_like(fy)).long()
    wa, wb = (t.wy, t.wx) if mutate == 'swap_w' else (t.wx, t.wy)
    sx, sy = int(mutate == 'tap_col'), int(mutate == 'tap_row')
    t.k = []
    for k in range(4):
        i, j = k & 1, k >> 1
        ok = t.vx[i] & t.vy[j]
        if mutate == 'drop_se' and k == 3:
            ok = torch.zeros_like(ok)
        xi = (t.x0 + i + sx).clamp(0, Ws - 1)
        yi = (t.y0 + j + sy).clamp(0, Hs - 1)
        t.k.append(types.SimpleNamespace(ok=ok, w=wa[i] * wb[j], idx=(yi * Ws + xi)))
    return t


# ======================================================================================================================
# the operation
# ======================================================================================================================
def warp_ref(src, flow, pad, align, norm, gout=None, mutate=None):
    """src [B, C, Hs, Ws], flow [B, 2, H, W] (fp32), gout [B, C, H, W] or None.  -> namespace (all float64)
        out, bound_out [B, C, H, W];  valid [B, 1, H, W];  taps (see _taps)
        gflow, bound_gflow [B, 2, H, W];  gsrc, bound_gsrc [B, C, Hs, Ws];  nq [B, Hs, Ws]   (when gout is given)
    mutate (WRONG on purpose): 'tap_col' / 'tap_row' every tap read one column / row further, 'drop_se' the south-east tap
    dropped, 'swap_w' the x and y weights exchanged, 'align' align_corners flipped, 'border_grad' the border clip's zeroed
    gradient not zeroed, 'nsrc_nflow' source and flow extents exchanged in the coordinate, 'tail_double' the last channel
    counted twice, 'lose_pair' the first (pixel, tap) pair that lands inside the source lost from the source gradient."""
    assert mutate is None or mutate in MUTATIONS
    B, C, Hs, Ws = src.shape
    _, _, H, W = flow.shape
    t = _taps(flow, Hs, Ws, pad, align, norm, mutate)
    s = src.to(D).reshape(B, C, Hs * Ws)
    o = types.SimpleNamespace(taps=t, valid=valid_ref(flow, norm))
    v = []
    out, S = s.new_zeros(B, C, H * W), s.new_zeros(B, C, H * W)
    for tk in t.k:
        a = s.gather(2, tk.idx.reshape(B, 1, -1).expand(B, C, H * W)) * tk.ok.reshape(B, 1, -1).to(D)
        v.append(a)
        out += a * tk.w.reshape(B, 1, -1)
        S += a.abs() * tk.w.reshape(B, 1, -1)
    if mutate == 'tail_double':
        out[:, C - 1] *= 2.0
    o.out = out.reshape(B, C, H, W)
    o.bound_out = (K_F * U1 * S * (~t.exact).reshape(B, 1, -1).to(D)).reshape(B, C, H, W)
    if gout is None:
        return o
    g = gout.to(D).reshape(B, C, H * W)
    if mutate == 'tail_double':
        g = g.clone()
        g[:, C - 1] *= 2.0
    wx0, wx1, wy0, wy1 = (w.reshape(B, 1, -1) for w in (t.wx[0], t.wx[1], t.wy[0], t.wy[1]))
    if mutate == 'swap_w':
        wx0, wx1, wy0, wy1 = wy0, wy1, wx0, wx1
    gx = (g * ((v[1] - v[0]) * wy0 + (v[3] - v[2]) * wy1)).sum(1)
    gy = (g * ((v[2] - v[0]) * wx0 + (v[3] - v[1]) * wx1)).sum(1)
    ax = (g.abs() * ((v[1].abs() + v[0].abs()) * wy0 + (v[3].abs() + v[2].abs()) * wy1)).sum(1)
    ay = (g.abs() * ((v[2].abs() + v[0].abs()) * wx0 + (v[3].abs() + v[1].abs()) * wx1)).sum(1)
    dx, dy = t.dx.reshape(B, -1), t.dy.reshape(B, -1)
    o.gflow = torch.stack([gx * dx, gy * dy], 1).reshape(B, 2, H, W)
    o.bound_gflow = ((K_G + C) * U1 * torch.stack([ax * dx.abs(), ay * dy.abs()], 1)).reshape(B, 2, H, W)
    gs, A, nq = s.new_zeros(B, C, Hs * Ws), s.new_zeros(B, C, Hs * Ws), s.new_zeros(B, 1, Hs * Ws)
    lost = mutate != 'lose_pair'
    for tk in t.k:
        ok = tk.ok.reshape(B, 1, -1).clone()
        if not lost and bool(ok.any()):
            ok.view(-1)[int(torch.nonzero(ok.view(-1))[0])] = False
            lost = True
        idx = tk.idx.reshape(B, 1, -1)
        term = g * (tk.w.reshape(B, 1, -1) * ok.to(D))
        gs.scatter_add_(2, idx.expand(B, C, H * W), term)
        A.scatter_add_(2, idx.expand(B, C, H * W), term.abs())
        nq.scatter_add_(2, idx, ok.to(D))
    o.gsrc = gs.reshape(B, C, Hs, Ws)
    o.nq = nq.reshape(B, Hs, Ws)
    o.bound_gsrc = ((nq + K_S) * (nq > 0).to(D) * U1 * A).reshape(B, C, Hs, Ws)
    return o


# ======================================================================================================================
# launch paths, RESTATED.  The CPU test reads the constants out of warp.hip / common.hpp and fails when they drift; they
# only label the cases and let the CPU test assert that the lists reach every branch; no kernel result depends on them.
# ======================================================================================================================
TX, TY = 32, 8                     # fwd_win / lds_scatter / det tile
FWD_HMAX, WQ_NARROW, WQ_WIDE = 24, 12, 18
FWD_WMAX = 4 * WQ_WIDE
SRC_WMAX, SRC_HMAX = 128, 64       # lds_scatter
SPLIT_WORKGROUPS, SPLIT_CHUNK = 2048, 4   # af_channel_split
FWD_LABELS = ('narrow', 'wide', 'gather-unaligned', 'gather-tall', 'gather-broad', 'empty')
SRC_LABELS = ('list', 'direct', 'empty')


def _up(a, b):
    return -(-a // b)


def channel_split(tiles, C):
    """af_channel_split, common.hpp:67-71"""
    n = 1
    while n * 2 <= C // SPLIT_CHUNK and tiles * n * 2 <= SPLIT_WORKGROUPS:
        n *= 2
    return n


def launch_paths(flow, C, Hs, Ws, pad, align, norm, bf16=False):
    """-> namespace fwd, src: one label per 8 x 32 tile ((b, ty, tx) order) for warp_fwd_kernel / warp_bwd_flow_kernel
    (src_window, warp.hip:89-106) and lds_scatter::warp_bwd_src_kernel (warp.hip:826-836); tiles; split (the forward's
    and the backward's gridDim.y; 1 for the forward's 3-channel chunk); chunk (channels per staged chunk), src_chunk;
    padding (ids of the rounded-up grid that run no tile, af_grid_for_tiles)."""
    B, _, H, W = flow.shape
    t = _taps(flow, Hs, Ws, pad, align, norm)
    anyv = (t.vx[0] | t.vx[1]) & (t.vy[0] | t.vy[1])
    big = 1 << 30
    lo_x = torch.where(anyv, t.x0 + (~t.vx[0]).long(), torch.full_like(t.x0, big))
    lo_y = torch.where(anyv, t.y0 + (~t.vy[0]).long(), torch.full_like(t.y0, big))
    hi_x = torch.where(anyv, t.x0 + t.vx[1].long(), torch.full_like(t.x0, -big))
    hi_y = torch.where(anyv, t.y0 + t.vy[1].long(), torch.full_like(t.y0, -big))
    fwd, src = [], []
    for b in range(B):
        for ty in range(_up(H, TY)):
            for tx in range(_up(W, TX)):
                sl = (b, slice(ty * TY, ty * TY + TY), slice(tx * TX, tx * TX + TX))
                x0, y0, x1, y1 = int(lo_x[sl].min()), int(lo_y[sl].min()), int(hi_x[sl].max()), int(hi_y[sl].max())
                if x1 < x0:
                    fwd.append('empty')
                    src.append('empty')
                    continue
                bw, bh = x1 - x0 + 1, y1 - y0 + 1
                aw = x1 - (x0 & ~3) + 1
                if Ws % 4 != 0:
                    fwd.append('gather-unaligned')
                elif bh > FWD_HMAX:
                    fwd.append('gather-tall')
                elif aw > FWD_WMAX:
                    fwd.append('gather-broad')
                else:
                    fwd.append('narrow' if aw <= 4 * WQ_NARROW else 'wide')
                src.append('list' if bw <= SRC_WMAX and bh <= SRC_HMAX else 'direct')
    tiles = len(fwd)
    chunk = 3 if (C <= 3 and not bf16) else 2
    split = channel_split(tiles, C)
    return types.SimpleNamespace(fwd=fwd, src=src, tiles=tiles, split_bwd=split, split_fwd=1 if chunk == 3 else split,
                                 chunk=chunk, src_chunk=4, padding=8 * _up(tiles, 8) - tiles)


# ======================================================================================================================
# fields: built from TARGET coordinates (source pixels), so that a case reaches its branch by construction
# ======================================================================================================================
def flow_for_target(tx, ty, H, W, Hs, Ws, norm, align):
    """tx, ty [B, H, W] float64 target coordinates -> the fp32 flow [B, 2, H, W] whose coordinate is (about) the target"""
    xs = torch.arange(W, dtype=D).view(1, 1, W)
    ys = torch.arange(H, dtype=D).view(1, H, 1)

    def axis(t, p, nf, ns):
        if norm == NORM_ARFLOW:
            pos = t * (nf - 1) / (ns - 1) if align else (t + 0.5) * (nf - 1) / ns
            return pos - p
        return t if norm == NORM_UFLOW_ABS else t - p
    return torch.stack([axis(tx, xs, W, Ws), axis(ty, ys, H, Hs)], 1).to(F32).contiguous()


def _snap(flow, tx, ty, Hs, Ws, norm, align):
    """nudges each flow component by up to 4 ulp so that the fp32 coordinate EQUALS the target wherever one of the
    neighbours does (the round trip is not the identity); -> (flow, share of the components that hit exactly)"""
    best = flow.clone()
    hit = torch.zeros_like(flow, dtype=torch.bool)
    tgt = torch.stack([tx, ty], 1)
    for k in (0, 1, -1, 2, -2, 3, -3, 4, -4):
        cand = flow.clone()
        for _ in range(abs(k)):
            cand = torch.nextafter(cand, torch.full_like(cand, float('inf') if k > 0 else float('-inf')))
        ix, iy, _, _ = coords(cand, Hs, Ws, norm, align)
        ok = (torch.stack([ix, iy], 1).to(D) == tgt) & ~hit
        best[ok] = cand[ok]
        hit |= ok
    return best, float(hit.double().mean())


def build_field(case, info=None):
    """the fp32 flow [B, 2, H, W] of a case (seeded by the case; see CASES for what each field is for).  info: a dict that
    receives 'exact_share', the share of an 'exact' field's components whose fp32 coordinate equals its target"""
    B, H, W, Hs, Ws = case.B, case.H, case.W, case.Hs, case.Ws
    norm, align = NORMS[case.norm], case.align
    x = torch.arange(W, dtype=D).view(1, 1, W).expand(B, H, W)
    y = torch.arange(H, dtype=D).view(1, H, 1).expand(B, H, W)
    bshift = torch.arange(B, dtype=D).view(B, 1, 1) * 0.37   # samples differ
    f, a = case.field, case.args
    if f == 'stretch':     # a = (sx, sy, ox, oy): tx = sx x + ox, ty = sy y + oy
        tx, ty = a[0] * x + a[2] + bshift, a[1] * y + a[3] + 0.5 * bshift
    elif f == 'far':       # everything leaves the image
        return torch.full((B, 2, H, W), float(a[0]), dtype=F32)
    elif f == 'point':     # a = (px, py, per_tile): every pixel (of its tile / of the sample) onto one point
        tx = torch.full_like(x, a[0]) + (torch.div(x, TX, rounding_mode='floor') * 3.0 if a[2] else 0.0)
        ty = torch.full_like(y, a[1]) + (torch.div(y, TY, rounding_mode='floor') * 2.0 if a[2] else 0.0)
    elif f == 'noise':     # a = (sigma,): identity + sigma randn, in flow pixels
        gen = _gen(83, B, H, W, Hs, Ws)
        n = torch.randn(B, 2, H, W, generator=gen, dtype=D) * a[0]
        tx, ty = (x + n[:, 0]) * (Ws - 1) / max(W - 1, 1), (y + n[:, 1]) * (Hs - 1) / max(H - 1, 1)
    elif f == 'half':      # exactly half-integer coordinates on both axes (snapped like 'exact')
        tx = torch.floor(x * (Ws - 2) / max(W - 1, 1)) + 0.5
        ty = torch.floor(y * (Hs - 2) / max(H - 1, 1)) + 0.5
        flow, share = _snap(flow_for_target(tx, ty, H, W, Hs, Ws, norm, align), tx, ty, Hs, Ws, norm, align)
        if info is not None:
            info['exact_share'] = share
        return flow.contiguous()
    elif f == 'exact':     # integer, half and edge coordinates, column by column; +-1e30 in two columns
        pat = [None, 0.5, -1.0, Ws - 1.0, float(Ws), Ws - 1.5, 0.0, -0.5]
        tx, ty = x.clone(), y.clone()
        for i in range(W):
            p = pat[i % len(pat)]
            tx[:, :, i] = float(min(i, Ws - 1)) if p is None else p
        for j in range(H):
            p = [None, 0.5, None, -1.0, Hs - 1.0, float(Hs), None, Hs - 1.5][j % 8]
            ty[:, j, :] = float(min(j, Hs - 1)) if p is None else p
        tx, ty = tx.contiguous(), ty.contiguous()
        flow = flow_for_target(tx, ty, H, W, Hs, Ws, norm, align)
        flow, share = _snap(flow, tx, ty, Hs, Ws, norm, align)
        if info is not None:
            info['exact_share'] = share
        flow[:, 0, :, W - 1] = 1e30
        flow[:, 1, :, W - 2] = -1e30
        return flow.contiguous()
    else:
        raise KeyError(f)
    return flow_for_target(tx.contiguous(), ty.contiguous(), H, W, Hs, Ws, norm, align)


def inputs(case):
    """(src [B, C, Hs, Ws], flow [B, 2, H, W], gout [B, C, H, W]) fp32; the source is bf16-representable for bf16 cases"""
    gen = _gen(97, case.B, case.C, case.H, case.W, case.Hs, case.Ws)
    src = torch.randn(case.B, case.C, case.Hs, case.Ws, generator=gen)
    gout = torch.randn(case.B, case.C, case.H, case.W, generator=gen)
    if case.bf16:
        src = bf16_round(src)
    return src.contiguous(), build_field(case), gout.contiguous()


def case_ref(case, mutate=None):
    src, flow, gout = inputs(case)
    return warp_ref(src, flow, PAD[case.pad], case.align, NORMS[case.norm], gout, mutate)


def case_paths(case):
    return launch_paths(build_field(case), case.C, case.Hs, case.Ws, PAD[case.pad], case.align, NORMS[case.norm], case.bf16)


# ======================================================================================================================
# case lists.  `fwd` / `src`: the label (forward + flow-gradient kernels / source-gradient kernel) the case exists for --
# the CPU test asserts that at least one tile of the case carries it; `split`: the backward's channel split it must get.
# ======================================================================================================================
Case = collections.namedtuple('Case', 'name B C H W Hs Ws norm align pad field args fwd src split bf16')


def _c(name, B, C, H, W, field, args, fwd, src='list', Hs=None, Ws=None, norm='arflow', align=True, pad='zeros', split=1,
       bf16=False):
    return Case(name, B, C, H, W, H if Hs is None else Hs, W if Ws is None else Ws, norm, align, pad, field, args, fwd, src,
                split, bf16)


SHIFT = (1.0, 1.0, 2.5, 0.25)   # x + 2.5, y + 0.25: the box starts at column 2, its aligned start 0 lies left of it
WINDOW_CASES = [
    # horizontal stretch of x by 1.2 / 1.8 / 2.6: 39 / 58 / 83 floats from the aligned start of the first tile
    _c('narrow 16x64', 1, 4, 16, 64, 'stretch', (1.2, 1.0, 0.3, 0.25), 'narrow'),
    _c('wide 24x96', 1, 4, 24, 96, 'stretch', (1.8, 1.0, 0.3, 0.25), 'wide'),          # 9 tiles: 7 padding ids
    _c('broad 24x96', 1, 4, 24, 96, 'stretch', (2.6, 1.0, 0.3, 0.25), 'gather-broad'),
    _c('tall 16x32<-40x32', 1, 4, 16, 32, 'stretch', (1.0, 3.5, 0.3, 0.2), 'gather-tall', Hs=40),   # 26 rows > HMAX
    _c('narrow W=30', 1, 4, 16, 30, 'stretch', (1.2, 1.0, 0.3, 0.25), 'gather-unaligned'),
    _c('wide W=70', 1, 4, 24, 70, 'stretch', (1.8, 1.0, 0.3, 0.25), 'gather-unaligned'),
    _c('broad W=70', 1, 4, 24, 70, 'stretch', (2.6, 3.5, 0.3, 0.25), 'gather-unaligned'),
    # the window against the source edge: aligned start left of the box; second tile's window (from column 32, 48 floats)
    # runs past Ws = 64 (the !pl.ok slots of window_plan); a tile half outside the output; one tile in total
    _c('edge 16x64', 2, 4, 16, 64, 'stretch', SHIFT, 'narrow'),
    _c('edge 13x40', 1, 4, 13, 40, 'stretch', SHIFT, 'narrow'),
    _c('one tile 5x20', 1, 4, 5, 20, 'stretch', SHIFT, 'narrow'),
    _c('edge border 13x40', 1, 5, 13, 40, 'stretch', (1.2, 1.3, -3.3, -2.25), 'narrow', pad='border'),
    # empty tiles: everything leaves the image; border padding collapses it onto the last source pixel
    _c('empty zeros', 1, 4, 13, 40, 'far', (500.0,), 'empty', src='empty'),
    _c('empty border', 1, 4, 13, 40, 'far', (500.0,), 'narrow', pad='border'),
]
EXACT_CASES = [
    _c('exact %s %s' % (n, p), 1, 3 if p == 'zeros' else 4, 16, 64, 'exact', (), 'wide', norm=n, pad=p)
    for n in ('arflow', 'uflow', 'abs') for p in ('zeros', 'border')
]
# flow extents 17 x 65 over a 16 x 64 source without align_corners: the divisors are powers of two and the coordinate is
# p + u - 1/2 EXACTLY, so -1 and n_src themselves are reached (through n - 1 = 63 the round trip steps over -1)
EXACT_CASES.append(_c('exact arflow align=False 17x65', 1, 3, 17, 65, 'exact', (), 'wide', Hs=16, Ws=64, align=False))
CHANNEL_CASES = [
    _c('C=%d' % C, 1, C, 16, 64, 'stretch', SHIFT, 'narrow', split=s)
    for C, s in ((1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (7, 1), (8, 2), (9, 2), (16, 4), (18, 4))
]
# source size != flow size in both directions, every norm mode, staged windows; both align flags and paddings
SIZE_CASES = (
    [_c('12x32->16x64 %s' % n, 1, 4, 16, 64, 'stretch', (0.45, 0.7, 1.3, 0.25), 'narrow', Hs=12, Ws=32, norm=n)
     for n in ('arflow', 'uflow', 'abs')]
    + [_c('16x64->12x32 %s' % n, 1, 4, 12, 32, 'stretch', (1.9, 1.3, 1.3, 0.25), 'wide', Hs=16, Ws=64, norm=n)
       for n in ('arflow', 'uflow', 'abs')]
    + [_c('16x64->12x32 arflow align=False %s' % p, 1, 5, 12, 32, 'stretch', (1.9, 1.3, -2.7, -1.25), 'wide', Hs=16, Ws=64,
          align=False, pad=p) for p in ('zeros', 'border')]
    + [_c('uflow border', 1, 4, 16, 64, 'stretch', (1.2, 1.3, -3.3, -2.25), 'narrow', norm='uflow', pad='border'),
       # Hs = 1 and Ws = 4 under UFLOW: the max(n - 1, 1) denominator
       _c('degenerate 1x4 uflow', 1, 2, 5, 20, 'stretch', (0.15, 1.0, 0.1, 0.0), 'narrow', Hs=1, Ws=4, norm='uflow'),
       _c('degenerate 1x4 abs', 1, 2, 5, 20, 'stretch', (0.15, 1.0, 0.1, 0.0), 'narrow', Hs=1, Ws=4, norm='abs')]
)
# source-gradient lists: 256 entries in each of 4 cells; a whole sample onto one point across 8 tiles; noise; a box wider
# than 128 columns and one taller than 64 rows (direct atomics)
SRC_CASES = [
    _c('tile onto a point', 1, 4, 16, 64, 'point', (5.5, 3.5, True), 'narrow'),
    _c('sample onto a point', 2, 5, 16, 128, 'point', (70.25, 9.75, False), 'narrow'),
    _c('noise 24x96', 2, 6, 24, 96, 'noise', (3.0,), 'narrow'),
    _c('box 140 columns 16x160', 1, 4, 16, 160, 'stretch', (4.5, 1.0, 0.3, 0.25), 'gather-broad', src='direct'),
    _c('box 65 rows 72x32', 1, 4, 72, 32, 'stretch', (1.0, 9.1, 0.3, 0.3), 'gather-tall', src='direct'),
]
CASES = WINDOW_CASES + EXACT_CASES + CHANNEL_CASES + SIZE_CASES + SRC_CASES
# bf16 storage: the window cases, the channel cases (C = 3 takes the chunk of 2 here) and one gather-unaligned case
BF16_CASES = [c._replace(bf16=True) for c in WINDOW_CASES[:4] + [WINDOW_CASES[5], WINDOW_CASES[7]] + CHANNEL_CASES]
# the flow consumed out of a [B, 4, H, W] tensor through flow_bstride, either half
STRIDED_CASE = _c('strided', 2, 5, 13, 40, 'stretch', SHIFT, 'narrow')
BY_NAME = {c.name: c for c in CASES}
