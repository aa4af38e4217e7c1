"""Shared by tests/test_census_ref_cpu.py and tests/test_census_gpu.py: float64 restatements, in plain torch on the CPU, of
what the census kernels compute PER PIXEL -- the standalone soft census distance (csrc/photo.hip, generic.hip) and the
fused warp + mask + census direction of UFlowLoss (csrc/census_col.hip, census_warp.hip, census_sym.hip), forward maps,
folded sums, loss and the gradients of the backward kernels -- together with the error bounds the GPU tests hold the
kernels to and the seeded inputs and shapes of those tests.  Nothing here imports the oracle or the product.

Reference arithmetic: utils/uflow_utils.py:6-77 (flow_to_warp, mask_invalid, resample), :227-293 (grey, census_transform,
soft_hamming, zero_mask_border, census_loss), losses/uflow_loss.py:30-54, losses/loss_blocks.py:12-62.

    ham(p)  = sum_o h(e(p, o)),  h(e) = e^2 / (0.1 + e^2),  e = t(d_a) - t(d_b),  t(d) = d / sqrt(0.81 + d^2),
    d_a     = grey_a(p + o) - grey_a(p)   (grey = 0 outside the image), o over the (2R+1)^2 - 1 offsets of the patch
    mask    = up4(clamp(occ, 0, 1)) * valid,   valid = [0 <= x + u <= W-1][0 <= y + v <= H-1] on the fp32 sums
    pm      = mask inside [R, n-R) in both axes, else 0
    dham    = pm 0.4 (ham + 0.01)^-0.6,   sums = (sum (ham + 0.01)^0.4 pm, sum pm),   loss = s0 / (s1 + 1e-6)
    d/d grey_b(p) sum_q w(q) ham(q) = sum_o (w(p) + w(p + o)) h'(e(p, o)) t'(d_b(p, o))       (h' odd, t' even; w = 0 outside)

The warped grey plane: the sampling coordinate is restated in fp32 torch ops exactly as the kernels and oracle.ops.resample
compute it (pos = x + u, g = 2 pos / max(n-1, 1) - 1, ((g + 1) / 2) (n - 1): every op is a single IEEE operation), so are the
floor of make_taps (csrc/taps.hpp); the four weights are the EXACT ones of that fp32 coordinate and the four zero-padded taps
are blended in float64.  (make_taps' fp32 weights ix - fx and (fx + 1) - ix are exact except for |ix| < 1, where the coordinate
has a finer ulp than the weight; their distance from the exact weights is computed, not bounded, and enters E_b.)
A float64 coordinate would differ by ulp(W) times the image slope, far beyond any arithmetic bound; the floor and the
validity compare are the only discontinuities and kernel and reference take them at the same fp32 number, so NO pixel is
left out of any comparison.

Bounds, u = 2^-24 (first order in u unless a second-order term is written; checked without a GPU by the CPU test: the fp32
oracle sits inside each with 4x room, each mutation leaves by > 100x).  Taken on trust, from the ISA document, not
measured here and not stated by the guides: v_rsq_f32, v_rcp_f32, v_log_f32, v_exp_f32 at one ulp (= 2u relative).

  grey plane     standalone: 6u 255 max|img| (three products, two sums, the x255; in-kernel).  Fused: grey a is an input
                 (0); grey b is the blend of four taps, E_b = 5u sum_k |a_k| w_k (the weight product, the first product and
                 three fused accumulations over same-signed terms) + sum_k |a_k| |w_k(fp32) - w_k|.  A zero-padded
                 neighbour is exact.
  d              delta_d = u |d| + E(p) + E(p + o)                                      (one subtraction)
  t              4u |t| + t'(d) delta_d        (fma half an ulp into rsq's argument, rsq 2u, one product; t' = 0.81 (0.81 + d^2)^-1.5)
  e              delta_e = sum_{a,b} (t' delta_d + 4u |t|) + u |e|
  pair           |h'(e)| delta_e + 10 delta_e^2 + 6u h      (|h''| <= 2 / 0.1 = 20; e^2, 0.1 + e^2, rcp 2u, the product)
  ham            sum of the pair bounds + (2R+1)^2 u ham    (non-negative terms, any order of addition)
  x^q            x = ham + 0.01, q in {0.4, -0.6} as exp2(q log2 x): relative |q| (delta_ham / x + u) +
                 ln2 (2u max(|log2 x|, 1) + 2u |q log2 x|) + 2u: v_log_f32 at one ulp of its result -- taken as an ABSOLUTE
                 2u near x = 1, where an ulp of the result vanishes --, the rounded product q log2 x and the constant q,
                 v_exp_f32 at one ulp; + 3u for the products with 0.4 and pm
  mask           exact without a range map (valid is exact), else 8u valid (section 18's up4_clamp_mul figure)
  dham           pm f rel(x^-0.6) + delta_pm f,  f = 0.4 x^-0.6
  sums           sum of the term bounds + 64u sum of the terms (non-negative; 64 >= the depth of the in-kernel tree: <= 16 per
                 lane, 6 + 2 across the workgroup; the GPU test folds the partial rows itself in float64) for the raw entry
                 points; + 64u more where torch folds the rows in fp32
  loss           (delta_s0 + loss delta_s1) / (s1 + 1e-6) + 4u loss
  gradient       element = S c_ch(p) sum_o gs_o c_o with gs = w(p) + w(p + o), c = h'(e) t'(d_b), c_ch = the corner
                 difference of the warp (fused) or 255 x the colour weight (standalone):
                 G_abs (20 + (2R+1)^2 + 12) u + |S| |c_ch|_abs sum_o |gs_o| delta_c_o,   G_abs = |S| |c_ch|_abs sum_o |gs_o c_o|,
                 delta_c = |h''| t'_b delta_e + |h'| |t''_b| delta_d_b  (the conditioning of the pair derivative through
                 delta_d and the roundings of t and e);  20u: two rsq (one of them cubed), rcp, seven products;
                 (2R+1)^2 u: the accumulation; 12u: gs, the constants, the scale, the corner difference in its absolute
                 form |v1 - v0| wy0 + |v3 - v2| wy1 and d coord / d flow = (2 / (n-1)) ((n-1) / 2) in fp32.
                 + |S| |sum_o gs_o c_o| (|v1 - v0| |dwy0| + |v3 - v2| |dwy1|) for the fp32 weights of the corner difference.
                 Where G_abs = 0 the kernel's element must be exactly 0.
  factor 2       The bounds of ham and of the gradients are TWICE the first-order worst case above.  Plain fp32 torch
                 arithmetic (the oracle) comes within 0.37 of the first-order figure at 668 160 pixels x 48 pairs (0.27 at
                 2 x 8 x 64), mostly through E_b: five roundings of five allowed.  Section 18's rule that the fp32 oracle
                 keep 4x room therefore needs a factor on top; it also covers the second-order terms dropped and keeps
                 the four trusted one-ulp figures from being load-bearing.
"""
import math
import types

import torch
import torch.nn.functional as F

from tests.loss_kernels_ref import D, U, _gen, gray255_ref, strided, up4_clamp_mul_ref, worst  # noqa: F401 (re-exported)

LN2 = math.log(2.0)
SAFETY = 2.0  # on the first-order worst case of the distance and of the gradients (see the docstring)
GREY_W = (0.2989, 0.5870, 0.1140)
MUTATIONS_CORE = ('lastcol', 'centre2', 'swap_const', 'clamp_nb')           # the distance itself: every path
MUTATIONS_LOSS = ('closed_right', 'dham_nopm')                              # the interior test and dham: every path
MUTATIONS_WARP = ('valid_open', 'tap_axis', 'tap_clamp')                    # the fused paths
MUTATIONS_PAIR = ('pair_occ_same', 'pair_scale_swap')                       # pair mode


# ======================================================================================================================
# the distance and its derivative
# ======================================================================================================================
def offsets(R, mutate=None):
    """the (dy, dx) of the patch without the centre.  mutate (WRONG on purpose): 'lastcol' drops the offset (R, R) -- the last
    column of the patch's last row --, 'centre2' reads the centre again in place of the offset (0, 1)."""
    out = []
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if (dy, dx) == (0, 0) or (mutate == 'lastcol' and (dy, dx) == (R, R)):
                continue
            out.append((0, 0) if (mutate == 'centre2' and (dy, dx) == (0, 1)) else (dy, dx))
    return out


def _padded(p, R, clamp=False):
    return F.pad(p, (R, R, R, R), mode='replicate' if clamp else 'constant')


def _nb(pp, R, dy, dx, H, W):
    return pp[..., R + dy:R + dy + H, R + dx:R + dx + W]


def census_core(ga, gb, R, ea=0.0, eb=0.0, w=None, mutate=None):
    """ga, gb: grey planes [B,1,H,W] (x255), float64.  ea, eb: their absolute error planes (or scalars).  w: weight plane
    [B,1,H,W] or None.  -> namespace
      ham, ham_bound                           per pixel
      dgb, dgb_abs, dgb_cond   (w given)       d/d gb(p) sum_q w(q) ham(q), the same sum over absolute values, the
                                               conditioning term sum_o |gs_o| delta_c_o
    mutate: offsets(), 'swap_const' (0.81 and 0.1 swapped), 'clamp_nb' (neighbours clamped instead of zero-padded)."""
    ga, gb = ga.to(D), gb.to(D)
    B, _, H, W = ga.shape
    c1, c2 = (0.1, 0.81) if mutate == 'swap_const' else (0.81, 0.1)
    clamp = mutate == 'clamp_nb'
    ea = torch.as_tensor(ea, dtype=D).expand_as(ga)
    eb = torch.as_tensor(eb, dtype=D).expand_as(gb)
    pa, pb = _padded(ga, R, clamp), _padded(gb, R, clamp)
    pea, peb = _padded(ea, R), _padded(eb, R)
    out = types.SimpleNamespace(ham=torch.zeros_like(ga), ham_bound=torch.zeros_like(ga))
    if w is not None:
        w = w.to(D)
        pw = _padded(w, R)
        out.dgb, out.dgb_abs, out.dgb_cond = torch.zeros_like(ga), torch.zeros_like(ga), torch.zeros_like(ga)
    for dy, dx in offsets(R, mutate):
        da, db = _nb(pa, R, dy, dx, H, W) - ga, _nb(pb, R, dy, dx, H, W) - gb
        dda = U * da.abs() + ea + _nb(pea, R, dy, dx, H, W)
        ddb = U * db.abs() + eb + _nb(peb, R, dy, dx, H, W)
        ra, rb = c1 + da * da, c1 + db * db
        ta, tb = da / ra.sqrt(), db / rb.sqrt()
        tpa, tpb = c1 / ra ** 1.5, c1 / rb ** 1.5
        e = ta - tb
        sq = e * e
        q = 1.0 / (c2 + sq)
        h = sq * q
        hp = 2.0 * c2 * e * q * q
        de = tpa * dda + tpb * ddb + 4 * U * (ta.abs() + tb.abs()) + U * e.abs()
        out.ham += h
        out.ham_bound += hp.abs() * de + (1.0 / c2) * de * de + 6 * U * h
        if w is not None:
            gs = w + _nb(pw, R, dy, dx, H, W)
            c = hp * tpb
            hpp = 2.0 * c2 * (c2 - 3.0 * sq) * q ** 3
            tppb = -3.0 * c1 * db / rb ** 2.5
            out.dgb += gs * c
            out.dgb_abs += (gs * c).abs()
            out.dgb_cond += gs.abs() * (hpp.abs() * tpb * de + hp.abs() * tppb.abs() * ddb)
    out.ham_bound = SAFETY * (out.ham_bound + (2 * R + 1) ** 2 * U * out.ham)
    return out


def ham_ref(grey_a, grey_b, R, mutate=None):
    """per-pixel soft census distance of two grey planes (x255): the fp32 values taken as float64"""
    return census_core(grey_a, grey_b, R, mutate=mutate).ham


def grad_rel(R):
    return (20 + (2 * R + 1) ** 2 + 12) * U


def pow_rel(x, q, dx):
    """relative error of exp2(q log2 x) for x = ham + 0.01 with absolute error dx (before x's own rounding)"""
    lg = torch.log2(x)
    return abs(q) * (dx / x + U) + LN2 * (2 * U * lg.abs().clamp_min(1.0) + 2 * U * (q * lg).abs()) + 2 * U


def interior(B, H, W, R, mutate=None):
    """[B,1,H,W] bool: R <= x < W - R and R <= y < H - R (zero_mask_border).  mutate='closed_right': <= n - R (WRONG)."""
    ext = 1 if mutate == 'closed_right' else 0
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    ok = (xs >= R) & (xs < W - R + ext) & (ys >= R) & (ys < H - R + ext)
    return ok.view(1, 1, H, W).expand(B, 1, H, W)


def reduce_ref(core, mask, mask_err, R, mutate=None, fold_fp32=False):
    """mask [B,1,H,W] float64 with absolute error mask_err -> adds pm, dham, dham_bound, terms, sums, sums_bound, loss,
    loss_bound to the namespace of census_core.  mutate: 'closed_right', 'dham_nopm' (dham without the border zeroing)."""
    B, _, H, W = core.ham.shape
    inn = interior(B, H, W, R, mutate)
    mask = mask.to(D)
    mask_err = torch.as_tensor(mask_err, dtype=D).expand_as(mask)
    pm = torch.where(inn, mask, torch.zeros_like(mask))
    pme = torch.where(inn, mask_err, torch.zeros_like(mask))
    x = core.ham + 0.01
    f = 0.4 * x ** -0.6
    core.pm = pm
    pmd, pmde = (mask, mask_err) if mutate == 'dham_nopm' else (pm, pme)
    core.dham = pmd * f
    core.dham_bound = pmd * f * (pow_rel(x, -0.6, core.ham_bound) + 3 * U) + pmde * f
    t0 = x ** 0.4
    core.terms = t0 * pm
    tb = pm * t0 * (pow_rel(x, 0.4, core.ham_bound) + 3 * U) + pme * t0
    depth = (128 if fold_fp32 else 64) * U
    core.sums = torch.stack([core.terms.sum(), pm.sum()])
    core.sums_bound = torch.stack([tb.sum() + depth * core.terms.sum(), pme.sum() + depth * pm.sum()])
    den = core.sums[1] + 1e-6
    core.loss = core.sums[0] / den
    core.loss_bound = (core.sums_bound[0] + core.loss * core.sums_bound[1]) / den + 4 * U * core.loss
    return core


# ======================================================================================================================
# standalone: arflow_census_fwd / arflow_census_bwd
# ======================================================================================================================
def standalone_ref(im_a, im_b, R, mask=None, w=None, scale=1.0, mutate=None, fold_fp32=False):
    """im_a, im_b [B,3,H,W] fp32.  -> census_core's namespace on the float64 grey planes with the in-kernel grey error
    6u 255 max|img| (+ reduce_ref's fields when a mask is given; the mask is an input: exact) and, with a weight plane w,
    grad = scale d/d im_b sum_p w(p) ham(p) [B,3,H,W] with grad_bound and g_abs."""
    ga, gb = gray255_ref(im_a), gray255_ref(im_b)
    ea = 6 * U * 255.0 * float(im_a.abs().max())
    eb = 6 * U * 255.0 * float(im_b.abs().max())
    core = census_core(ga, gb, R, ea, eb, w, mutate)
    if mask is not None:
        reduce_ref(core, mask, 0.0, R, mutate, fold_fp32)
    if w is not None:
        cw = torch.tensor(GREY_W, dtype=D).view(1, 3, 1, 1) * 255.0 * float(scale)
        core.grad = cw * core.dgb
        core.g_abs = cw.abs() * core.dgb_abs
        core.grad_bound = SAFETY * (core.g_abs * grad_rel(R) + cw.abs() * core.dgb_cond)
    return core


# ======================================================================================================================
# the warped grey plane
# ======================================================================================================================
def sample_coords(flow32):
    """fp32 sampling coordinates (ix, iy) [B,H,W] of af_sample_coord (ARFLOW_NORM_UFLOW) / oracle.ops.resample, and the
    fp32 absolute positions (cx, cy) the validity test takes"""
    f = flow32.float()
    B, _, H, W = f.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    cx, cy = xs + f[:, 0], ys + f[:, 1]

    def coord(pos, n):
        g = 2.0 * pos / float(max(n - 1, 1)) - 1.0
        return ((g + 1.0) / 2.0) * float(n - 1)
    return coord(cx, W), coord(cy, H), cx, cy


def warp_ref(gb32, flow32, mutate=None, dtype=D):
    """-> namespace: warped [B,1,H,W] float64 (zero-padded bilinear sample of the fp32 plane gb32 at the fp32 coordinate),
    err (E_b), sx, sy (d sample / d coordinate: the corner differences), sx_abs, sy_abs (their absolute forms), valid
    [B,1,H,W] float64 (mask_invalid, closed).  mutate (WRONG on purpose): 'tap_axis' the north-east tap's weight is
    wy1 wy0, 'tap_clamp' a tap outside the image reads the clamped position, 'valid_open' the open interval."""
    g = gb32.to(dtype)
    B, _, H, W = g.shape
    ix, iy, cx, cy = sample_coords(flow32)
    fx, fy = torch.floor(ix), torch.floor(iy)
    # exact weights of the fp32 coordinate, and how far the fp32 differences of make_taps are from them: ix - fx and
    # (fx + 1) - ix are exact in fp32 EXCEPT for |ix| < 1, where the coordinate has a finer ulp than the weight (0.7 = 1 - 0.3)
    xd, yd, fxd, fyd = ix.to(D), iy.to(D), fx.to(D), fy.to(D)
    wx1, wx0, wy1, wy0 = xd - fxd, (fxd + 1.0) - xd, yd - fyd, (fyd + 1.0) - yd
    ex1, ex0 = ((ix - fx).to(D) - wx1).abs(), (((fx + 1.0) - ix).to(D) - wx0).abs()
    ey1, ey0 = ((iy - fy).to(D) - wy1).abs(), (((fy + 1.0) - iy).to(D) - wy0).abs()
    if dtype != D:  # the fp32 evaluation (CPU test): make_taps' own weights, everything below in fp32
        wx1, wx0, wy1, wy0 = ix - fx, (fx + 1.0) - ix, iy - fy, (fy + 1.0) - iy
    flat = g.reshape(B, H * W)
    v, wt, we = [], [], []
    for dyk, wy, ey in ((0, wy0, ey0), (1, wy1, ey1)):
        for dxk, wx, ex in ((0, wx0, ex0), (1, wx1, ex1)):
            xi, yi = fx + dxk, fy + dyk
            ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long().reshape(B, -1)
            val = flat.gather(1, idx).view(B, H, W)
            if mutate != 'tap_clamp':
                val = torch.where(ok, val, torch.zeros_like(val))
            v.append(val)
            wt.append(wy1 * wy0 if (mutate == 'tap_axis' and (dyk, dxk) == (0, 1)) else wx * wy)
            we.append(ex * wy + wx * ey + ex * ey)
    out = types.SimpleNamespace()
    out.warped = sum(a * b for a, b in zip(v, wt)).unsqueeze(1)
    out.err = sum(a.abs() * (5 * U * b + c) for a, b, c in zip(v, wt, we)).unsqueeze(1)
    out.sx = ((v[1] - v[0]) * wy0 + (v[3] - v[2]) * wy1).unsqueeze(1)
    out.sy = ((v[2] - v[0]) * wx0 + (v[3] - v[1]) * wx1).unsqueeze(1)
    out.sx_abs = ((v[1] - v[0]).abs() * wy0 + (v[3] - v[2]).abs() * wy1).unsqueeze(1)
    out.sy_abs = ((v[2] - v[0]).abs() * wx0 + (v[3] - v[1]).abs() * wx1).unsqueeze(1)
    out.sx_err = ((v[1] - v[0]).abs() * ey0 + (v[3] - v[2]).abs() * ey1).unsqueeze(1)
    out.sy_err = ((v[2] - v[0]).abs() * ex0 + (v[3] - v[1]).abs() * ex1).unsqueeze(1)
    if mutate == 'valid_open':
        ok = (cx > 0) & (cx < W - 1) & (cy > 0) & (cy < H - 1)
    else:
        ok = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
    out.valid = ok.to(D).unsqueeze(1)
    return out


# ======================================================================================================================
# fused: arflow_census_warp_fwd / _bwd and the pair forms
# ======================================================================================================================
def fused_ref(ga32, gb32, flow32, occ, R, w=None, scale=1.0, mutate=None, fold_fp32=False):
    """One photometric direction on fp32 grey planes [B,1,H,W], flow [B,2,H,W], range map occ [B,1,H/4,W/4] or None.
    -> namespace with census_core's and reduce_ref's fields, mask, mask_bound, and for a weight plane w (float32 [B,1,H,W]; None
    = the reference's own dham): grad = scale d/d flow sum_p w(p) ham(p) [B,2,H,W], grad_bound, g_abs."""
    wp = warp_ref(gb32, flow32, mutate)
    if occ is None:
        mask, merr = wp.valid, 0.0
    else:
        mask, merr = up4_clamp_mul_ref(occ, wp.valid), 8 * U * wp.valid
    pre = None
    if w is None:  # the end-to-end gradient: the weight is the reference's own dham
        pre = reduce_ref(census_core(ga32.to(D), wp.warped, R, 0.0, wp.err, None, mutate), mask, merr, R, mutate, fold_fp32)
        w_used = pre.dham
    else:
        w_used = w.to(D)
    core = census_core(ga32.to(D), wp.warped, R, 0.0, wp.err, w_used, mutate)
    reduce_ref(core, mask, merr, R, mutate, fold_fp32)
    core.mask, core.mask_bound, core.warp = mask, torch.as_tensor(merr, dtype=D).expand_as(mask), wp
    s = abs(float(scale))
    cabs = torch.cat([wp.sx_abs, wp.sy_abs], 1)
    core.grad = float(scale) * torch.cat([wp.sx, wp.sy], 1) * core.dgb
    core.g_abs = s * cabs * core.dgb_abs
    core.grad_bound = SAFETY * (core.g_abs * grad_rel(R) + s * cabs * core.dgb_cond + s * torch.cat([wp.sx_err, wp.sy_err], 1) * core.dgb_abs)
    if w is None:
        # the weight itself carries dham's bound: sum_o (dw(p) + dw(p + o)) |c_o| <= ... taken with the largest relative
        # bound of the weights the element uses (the patch maximum of dham_bound / dham, 0 / 0 = 0)
        rel = torch.where(pre.dham > 0, pre.dham_bound / pre.dham.clamp_min(1e-300), torch.zeros_like(pre.dham))
        relmax = F.max_pool2d(rel, 2 * R + 1, 1, R)
        core.grad_bound = core.grad_bound + core.g_abs * relmax
    return core


def pair_split(t2, direction):
    return t2[direction::2]


def pair_ref(gray2, flow2, occ2, R, w2=None, scale2=(1.0, 1.0), mutate=None, fold_fp32=False):
    """arflow_census_warp_pair_*: sample s = 2 b + direction, image a plane s, image b and range map plane s ^ 1, one scale
    per direction: TWO calls of fused_ref.  -> [direction 0, direction 1].  mutate: 'pair_occ_same' (range map plane s),
    'pair_scale_swap' (WRONG on purpose), else passed on."""
    out = []
    sc = tuple(scale2)[::-1] if mutate == 'pair_scale_swap' else tuple(scale2)
    for d in (0, 1):
        occ = None if occ2 is None else pair_split(occ2, d if mutate == 'pair_occ_same' else d ^ 1)
        out.append(fused_ref(pair_split(gray2, d), pair_split(gray2, d ^ 1), pair_split(flow2, d), occ, R,
                             None if w2 is None else pair_split(w2, d), sc[d], mutate, fold_fp32))
    return out


def interleave(a, b):
    """two [B,...] tensors -> [2B,...] with a at the even samples"""
    return torch.stack([a, b], 1).reshape((-1,) + tuple(a.shape[1:]))


# ======================================================================================================================
# census_sym_strip_h (csrc/census_sym.hip), restated
# ======================================================================================================================
def sym_chunks(B, H, W, R):
    n = 4
    while n > 1 and B * -(-W // 56) * -(-H // (16 * n - R)) < 768:
        n -= 1
    return n


def family_tiles(family, B, H, W, R):
    """workgroups that own a tile in a fused forward launch (the grid is this count rounded up to a multiple of 8; the rest
    are padding workgroups): census_col.hip 64 - R columns x 32 rows, census_warp.hip 64 x 16, census_sym.hip 56-column strips
    of 16 n - R rows"""
    up = lambda a, b: -(-a // b)
    if family == 'column':
        return up(W, 64 - R) * up(H, 32) * B
    if family == 'ordered':
        return up(W, 64) * up(H, 16) * B
    return up(W, 56) * up(H, 16 * sym_chunks(B, H, W, R) - R) * B


def sums_rows(B, H, W):
    """arflow_sums_rows (csrc/api.hip)"""
    return max(8 * ((-(-W // 32) * -(-H // 8) * B + 7) // 8), -(-W // 256) * H * B)


# ======================================================================================================================
# inputs
# ======================================================================================================================
def image(kind, B, H, W, which=0):
    """[B,3,H,W] fp32.  'S': low contrast, 0.5 + 0.004 randn -- neighbouring grey differences of about one level (almost all
    within +-3), where t(d) is in its linear range and the distance is sensitive to every tap.  'N': rand(), full range: the
    transform saturates.  'C': constant (0.37 for image a, 0.61 for image b)."""
    gen = _gen(41 + which, B, H, W)
    if kind == 'S':
        return (0.5 + 0.004 * torch.randn(B, 3, H, W, generator=gen)).contiguous()
    if kind == 'N':
        return torch.rand(B, 3, H, W, generator=gen)
    return torch.full((B, 3, H, W), (0.37, 0.61)[which])


def grey(kind, B, H, W, which=0):
    """[B,1,H,W] fp32 grey plane (x255) of image(): the input of the fused kernels"""
    return gray255_ref(image(kind, B, H, W, which)).float()


def flow(kind, B, H, W):
    """'Q': integer displacements in -3 .. 3 (every sample is an exact grey value, many land exactly on the first / last row
    and column, those near the border leave the image).  'R': 2.5 randn.  Both: the first two rows are pushed 30 pixels
    out (validity mask, zero padding)."""
    gen = _gen(51 if kind == 'Q' else 52, B, H, W)
    if kind == 'Q':
        f = torch.randint(-3, 4, (B, 2, H, W), generator=gen).float()
    else:
        f = 2.5 * torch.randn(B, 2, H, W, generator=gen)
    f[:, :, :2] += 30.0
    return f


def range_map(B, H, W):
    """[B,1,H/4,W/4] in [-0.2, 1.4]: both clamps act"""
    return 1.6 * torch.rand(B, 1, H // 4, W // 4, generator=_gen(53, B, H, W)) - 0.2


def weight_plane(B, H, W):
    """positive fp32 noise, non-zero in the border band and at invalid pixels too"""
    return 0.05 + torch.rand(B, 1, H, W, generator=_gen(54, B, H, W))


def user_mask(B, H, W):
    return torch.rand(B, 1, H, W, generator=_gen(55, B, H, W))


# (family, R) -> [(B, H, W)]: the smallest shapes at which each tiling can go wrong
COL_SHAPES = [(2, 8, 64), (1, 32, 60), (2, 36, 8), (1, 36, 64)]      # + (1, 36, 124) for R = 3
ORD_SHAPES = [(2, 20, 68), (1, 8, 8)]
SYM_SHAPES = [(2, 16, 60), (1, 32, 116)]
SYM_N2 = (48, 232, 60)
SYM_N4 = (96, 428, 8)
PAIR_SHAPE = {'column': (2, 36, 64), 'ordered': (2, 20, 68)}
PAIR_COMBOS = [('S', 'R'), ('N', 'Q')]
ROWS_SHAPES = [('column', (1, 32, 60)), ('column', (4, 8, 64)), ('ordered', (1, 8, 8)), ('ordered', (2, 20, 68)),
               ('pair-symmetric', (1, 16, 60)), ('pair-symmetric', (2, 16, 60))]  # tile counts 1, 8, 1, 8, 4, 8 at R = 3
E2E_STANDALONE = [(3, 2, 20, 68), (2, 1, 17, 35), (4, 2, 12, 21)]
COMBOS = [('S', 'R'), ('S', 'Q'), ('N', 'R'), ('N', 'Q'), ('C', 'Q'), ('C', 'R')]
STANDALONE = [(3, 2, 20, 68), (3, 2, 9, 33), (2, 1, 17, 35), (1, 2, 17, 35), (4, 2, 12, 21), (3, 1, 7, 7), (1, 1, 1, 1),
              (3, 1, 1, 9), (2, 1, 1, 1)]  # (R, B, H, W)


def fused_shapes(family, R):
    if family == 'column':
        return COL_SHAPES + ([(1, 36, 124)] if R == 3 else [])
    return {'ordered': ORD_SHAPES, 'pair-symmetric': SYM_SHAPES}[family]


def fused_inputs(B, H, W, img, fl):
    """(grey a, grey b, flow, range map) of one fused case"""
    return grey(img, B, H, W, 0), grey(img, B, H, W, 1), flow(fl, B, H, W), range_map(B, H, W)


def pair_inputs(B2, H, W, img, fl):
    """(grey planes [B2,1,H,W], flows [B2,2,H,W], range maps [B2,1,H/4,W/4]); B2 even"""
    return (interleave(grey(img, B2 // 2, H, W, 0), grey(img, B2 // 2, H, W, 1)), flow(fl, B2, H, W), range_map(B2, H, W))
