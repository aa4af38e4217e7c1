"""Shared by tests/test_loss_kernels_cpu.py and tests/test_loss_kernels_gpu.py: float64 restatements, in plain torch on the
CPU, of what the standalone loss kernels compute -- edge-aware smoothness (csrc/smooth.hip, smooth_dev.hpp), the forward
splat, the coordinate and occlusion masks (csrc/warp.hip) and the x4 resize helpers -- together with the error bounds the GPU
tests hold the kernels to, and the seeded input recipes of those tests (so that the CPU file can check every bound and
every input without a GPU).

Reference arithmetic: losses/loss_blocks.py:87-124, losses/uflow_loss.py:56-102, utils/uflow_utils.py:80-204,
utils/warp_utils.py:26-134, as oracle/ops.py restates them in the working precision.  Nothing here imports the oracle or the
product; the CPU test pins these functions to the frozen results of the reference (tests/golden/*.npz) and to the oracle.

u = 2^-24 is the unit roundoff of fp32 (half an ulp of 1).
"""
import types

import torch
import torch.nn.functional as F

U = 2.0 ** -24
D = torch.float64


# ======================================================================================================================
# smoothness
# ======================================================================================================================
def _nar(t, axis, start, n):
    return t.narrow(axis, start, n) if n > 0 else t.narrow(axis, 0, 0)


def _stencil(order, mutate):
    if order == 1:
        return (-1.0, 1.0)
    return (1.0, -1.0, 1.0) if mutate == 'stencil' else (1.0, -2.0, 1.0)


def _pen(v, penalty):
    return v.abs() if penalty == 0 else torch.sqrt(v * v + 1e-6)


def _dpen(v, penalty):
    return torch.sign(v) if penalty == 0 else v / torch.sqrt(v * v + 1e-6)


def _scatter(A, st, axis, n):
    """out[.., i + k, ..] += st[k] * A[.., i, ..]: the adjoint of the difference stencil along `axis` (length n)."""
    shape = list(A.shape)
    shape[axis] = n
    out = A.new_zeros(shape)
    m = A.shape[axis]
    for k, c in enumerate(st):
        if m > 0:
            out.narrow(axis, k, m).add_(A * c)
    return out


def _scatter_max(A, order, axis, n, fill):
    shape = list(A.shape)
    shape[axis] = n
    out = A.new_full(shape, fill)
    m = A.shape[axis]
    for k in range(order + 1):
        if m > 0:
            seg = out.narrow(axis, k, m)
            seg.copy_(torch.maximum(seg, A))
    return out


def smooth_ref(flow, img, flow_scale, alpha, order, wmode, penalty, coef=(0.7, -1.3), small_thr=None, mutate=None):
    """Float64 restatement of arflow_smooth_fwd / arflow_smooth_bwd for any channel count Ci.

    x-term anchored at (y, x), x < W - order:  v = flow_scale * D flow  with D f = f[x+1] - f[x] (order 1) or
    (f[x+2] - f[x+1]) - (f[x+1] - f[x]) (order 2);  s = mean_c |img[xa] - img[xb]| with (xa, xb) = (x+1, x) for order 1,
    (x+2, x+1) for order 2 / wmode 0 (smooth_grad_2nd: the first-order weights shifted by one) and (x+2, x) for order 2 /
    wmode 1 (UFlowLoss smooth_order=2: image_grads with stride 2);  term t = exp(-alpha s) * pen(v), pen = |v| (penalty 0)
    or sqrt(v^2 + 1e-6) (penalty 1), summed over both flow channels.  The y-term is the same along rows.

    Returns a namespace:
      sums    [2]  (sum of the x-terms, sum of the y-terms)
      grad    d(coef[0] sums[0] + coef[1] sums[1]) / d flow, [B,2,H,W]; d|v|/dv = sign(v), 0 at v = 0
      g_abs   the same sum with every stencil coefficient, dpen and weight replaced by its absolute value
      expo    (alpha * s of the x-terms [B,1,H,W-o], of the y-terms [B,1,H-o,W])
      terms   (t of the x-terms [B,2,H,W-o], of the y-terms)        v: the differences, same layout
      rmax    [B,1,H,W] the largest exponent alpha * s among the terms an element enters (0 where it enters none)
      cond    [B,2,H,W] conditioning term of the penalty-1 derivative (see smooth_grad_bound), 0 for penalty 0
      touchy  [B,2,H,W] bool: the element's stencil touches a difference with |v| < small_thr (all False without a threshold)
    `mutate` builds a deliberately WRONG restatement (tests/test_loss_kernels_cpu.py): 'stencil' {1,-1,1} for {1,-2,1},
    'lastcol' drops the last valid difference column / row, 'div3' divides the channel sum by 3, 'scale_after' applies
    flow_scale after the penalty."""
    f, im = flow.to(D), img.to(D)
    B, _, H, W = f.shape
    Ci = im.shape[1]
    o = int(order)
    st = _stencil(o, mutate)
    fs = float(flow_scale)
    out = types.SimpleNamespace(sums=torch.zeros(2, dtype=D), grad=torch.zeros_like(f), g_abs=torch.zeros_like(f),
                                cond=torch.zeros_like(f), touchy=torch.zeros(f.shape, dtype=torch.bool),
                                rmax=torch.zeros(B, 1, H, W, dtype=D), expo=[], terms=[], v=[])
    for i, axis in enumerate((3, 2)):
        n = f.shape[axis]
        m = n - o - (1 if mutate == 'lastcol' else 0)
        d = sum(c * _nar(f, axis, k, m) for k, c in enumerate(st)) if o == 1 or mutate == 'stencil' else \
            (_nar(f, axis, 2, m) - _nar(f, axis, 1, m)) - (_nar(f, axis, 1, m) - _nar(f, axis, 0, m))
        lo = 0 if (o == 1 or wmode == 1) else 1
        s = (_nar(im, axis, o, m) - _nar(im, axis, lo, m)).abs().sum(1, keepdim=True) / (3.0 if mutate == 'div3' else Ci)
        expo = float(alpha) * s
        w = torch.exp(-expo)
        if mutate == 'scale_after':
            v, post = d, fs
        else:
            v, post = d * fs, 1.0
        t = w * _pen(v, penalty) * post
        lin = coef[i] * fs * w  # d t / d D f = fs * w * dpen(v)
        out.sums[i] = t.sum()
        out.grad += _scatter(lin * _dpen(v, penalty), st, axis, n)
        absst = tuple(abs(c) for c in st)
        out.g_abs += _scatter(lin.abs() * _dpen(v, penalty).abs(), absst, axis, n)
        out.rmax = torch.maximum(out.rmax, _scatter_max(expo, o, axis, n, 0.0))
        if penalty == 1:
            span = sum(c * _nar(f, axis, k, m).abs() for k, c in enumerate(absst))
            out.cond += _scatter(lin.abs() * (4 * U * fs) * span * 1e-6 / (v * v + 1e-6) ** 1.5, absst, axis, n)
        if small_thr is not None:
            out.touchy |= _scatter((v.abs() < small_thr).to(D), (1.0,) * (o + 1), axis, n) > 0
        out.expo.append(expo)
        out.terms.append(t)
        out.v.append(v)
    return out


def term_rel(expo):
    """r_t = (alpha s_t + 4) 2u, the relative error of one term w * pen(v) as the kernels evaluate it.  __expf(x) is
    v_exp_f32(x * log2(e)): the product rounds the argument by |x| u, which the exponential turns into a relative |x| u
    (|x| = alpha s), and the rounded factors of x (the channel mean, its product with alpha) add as much again: alpha s 2u.
    v_exp_f32 itself is taken at one ulp = 2u (the ISA document's figure), and pen (one fma, one sqrt), the sum of the two
    channels' penalties and the product with the weight round three times more: 3 * 2u in ulps, 8u in all."""
    return (expo + 4.0) * 2 * U


def smooth_sum_bound(ref):
    """[2]: |got - ref| <= sum_t t r_t + 64u sum_t t.  All terms are non-negative, so a summation tree of depth d over them
    is off by at most d u sum_t t: 16 for the per-thread chain (8 rows x 2 penalties), 6 for the wave, 4 for the block, the
    rest (38) for the fold of the partial rows, which torch sums in a tree no deeper than that."""
    return torch.stack([(t * term_rel(e)).sum() + 64 * U * t.sum() for t, e in zip(ref.terms, ref.expo)])


def smooth_grad_bound(ref, conditioned=False):
    """[B,2,H,W]: |got - ref| <= G_abs (max_t r_t + 16u) [+ cond].  An element is a sum of at most 2 (order + 1) products
    coef * fscale * st * w * dpen: each is off by its r_t relative (the weight; dpen = +-1, or v / sqrt(v^2 + 1e-6) from an
    exactly representable v) and the fma chain, the coefficient products coef * fscale and w * st * c add 16u at most.
    conditioned: v itself carries the rounding of the fp32 differences, at most 4u flow_scale (|r0| + 2|r1| + |r2|), which
    d dpen / d v = 1e-6 / (v^2 + 1e-6)^1.5 turns into an error of the derivative (ref.cond; 0 for penalty 0, where only the
    sign matters and the elements next to a tiny |v| are left out)."""
    b = ref.g_abs * (term_rel(ref.rmax) + 16 * U)
    return b + ref.cond if conditioned else b


# ---- inputs of the smoothness tests -------------------------------------------------------------------------------
MODES = [(1, 0, 0), (1, 0, 1), (2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1)]  # (order, wmode, penalty)
ALPHAS = (10.0, 150.0)
COEF = (0.7, -1.3)
SMALL_SHAPES = [(1, 3, 1, 1), (1, 3, 2, 2), (2, 3, 3, 3), (2, 1, 7, 255), (2, 4, 5, 257), (1, 2, 9, 513)]  # (B, Ci, H, W)
STRIDED_SHAPE = (2, 3, 5, 257)
ROW_SHAPES = [(16, 3, 129, 257), (32, 3, 257, 257)]  # rows = 2 and 8; H % rows = 1: the last workgroup holds one row
ROW_MODES = [(1, 0, 0), (2, 1, 1)]
Q_SCALES = (0.25, 1.0, 4.0)
R_SCALE = 1 / 3.7


def smooth_rows(B, H, W):
    """rows per workgroup of smooth_fwd_kernel (csrc/smooth.hip: arflow_smooth_fwd)"""
    return min(max(-(-W // 256) * H * B // 2048, 1), 8)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _coarse_noise(gen, B, C, H, W):
    c = torch.randn(B, C, H // 8 + 2, W // 8 + 2, generator=gen)
    return F.interpolate(c, size=(H, W), mode='bilinear', align_corners=True)


def smooth_image(B, Ci, H, W):
    """Low contrast, 0.5 + 0.02 * smooth noise, with a +0.3 step across W // 2: at alpha 10 and at alpha 150 the weights
    span 1e-20 .. 1 (exp(-150 * 0.3) = 3e-20 on the step).  A rand() image at alpha 150 underflows every weight."""
    img = 0.5 + 0.02 * _coarse_noise(_gen(1, B, Ci, H, W), B, Ci, H, W)
    img[..., W // 2:] += 0.3
    return img.contiguous()


def smooth_flow(kind, B, H, W, channels=2):
    """'Q': multiples of 1/64 (2.5 randn, rounded) with a constant patch over [:H//2, :W//3]: every first and second
    difference is exact in fp32 (|values| < 2^5, so all differences are multiples of 2^-6 below 2^8), stays exact under a
    power-of-two flow_scale, and is exactly 0 inside the patch.  'R': plain 2.5 randn."""
    gen = _gen(2 if kind == 'Q' else 3, B, H, W, channels)
    f = 2.5 * torch.randn(B, channels, H, W, generator=gen)
    if kind == 'Q':
        f = torch.round(f * 64) / 64
        f[:, :, :H // 2, :W // 3] = torch.tensor([1.25, -0.5] * (channels // 2)).view(1, channels, 1, 1)
    return f


def small_threshold(flow, flow_scale):
    return 1e-4 * float(flow_scale) * float(flow.abs().max())


# ======================================================================================================================
# forward splat
# ======================================================================================================================
def splat_ref(coords32, H, W, variant, mutate=None):
    """compute_range_map (variant 0) / get_corresponding_map (variant 1) in float64 on fp32 ABSOLUTE coordinates [B,2,H,W]
    (the kernel's single rounded add x + u is the caller's, in fp32: with |u| ~ 80 the fp32 and the float64 sum differ
    enough to move a range map by 1.2e-5).  -> (map [B,1,H,W] float64, count [B,1,H,W] int64: the taps that land in each
    cell, zero-weight taps included).  mutate='edge': WRONG on purpose, the south-east tap is dropped on the last column."""
    c = coords32.to(D)
    B = c.shape[0]
    x, y = c[:, 0].reshape(B, -1), c[:, 1].reshape(B, -1)
    fx, fy = torch.floor(x), torch.floor(y)
    out = torch.zeros(B, H * W, dtype=D)
    cnt = torch.zeros(B, H * W, dtype=torch.int64)
    for di in (0, 1):
        for dj in (0, 1):
            yi, xj = fy + di, fx + dj
            ok = (yi >= 0) & (yi <= H - 1) & (xj >= 0) & (xj <= W - 1)  # variant 1: "the clamped index is the raw one"
            if (variant & 1) == 0:
                oy, ox = y - fy, x - fx
                w = (oy if di else 1.0 - oy) * (ox if dj else 1.0 - ox)
            else:
                w = (1.0 - (x - xj).abs()) * (1.0 - (y - yi).abs())
            if mutate == 'edge' and di and dj:
                ok = ok & (xj != W - 1)
            idx = (yi.clamp(0, H - 1) * W + xj.clamp(0, W - 1)).long()
            out.scatter_add_(1, idx, torch.where(ok, w, torch.zeros_like(w)))
            cnt.scatter_add_(1, idx, ok.long())
    return out.view(B, 1, H, W), cnt.view(B, 1, H, W)


def splat_bound(value, count, n_add=None):
    """Per cell: count * 2^-22 + n_add * u * value.  Per tap: the two factors 1 - o (or o) and their product are below 1
    and round by at most u/2 each, the 2^-22 fixed-point weight of the LDS path by 2^-23: 3.5u <= 2^-22.  n_add: float
    additions (and the int -> float conversion of a flushed cell) that meet in the cell, each off by at most u times the
    final value since every addend is non-negative: `count` in general (the direct-atomic path, or one flush per tile with
    a tile per tap), the tiles per image where the whole image lands in one LDS window."""
    n_add = count.to(D) if n_add is None else float(n_add)
    return count.to(D) * 2.0 ** -22 + n_add * U * value


def abs_coords(flow):
    """fp32 x + u, y + v (the kernels' own rounded add) -> [B,2,H,W] fp32"""
    B, _, H, W = flow.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    return torch.stack([xs + flow[:, 0], ys + flow[:, 1]], 1)


def splat_cases():
    """name -> (flow [B,2,H,W] fp32, n_add of splat_bound or None)"""
    cases = {}
    cases['ragged'] = (2.5 * torch.randn(2, 2, 9, 33, generator=_gen(11)), None)
    cases['wide'] = (6.0 * torch.randn(1, 2, 5, 257, generator=_gen(12)), None)
    # targets spread over the whole image and beyond: every tile's window exceeds 128 x 64 -> the direct-atomic fallback
    cases['spread'] = (80.0 * torch.randn(1, 2, 64, 160, generator=_gen(13)), None)
    H, W = 40, 64
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    # every pixel lands on (7.25, 3.5) (u = 7.25 - x, v = 3.5 - y are exact): 256 contributions per tile and cell in a
    # 2 x 2 window -- the LDS path -- and one flush per tile: n_add = the 5 x 2 tiles of an image
    cases['collapse'] = (torch.stack([7.25 - xs, 3.5 - ys])[None].repeat(2, 1, 1, 1), 10)
    # targets exactly on 0, W-1, -1, W and half a pixel outside, in x and in y (H = 6, W = 40: one row per y target)
    H, W = 6, 40
    tx = torch.tensor([0.0, W - 1.0, -1.0, float(W), -0.5, W - 0.5, -1.5, W + 0.5, 3.0, 3.25, W - 1.5])
    ty = torch.tensor([0.0, H - 1.0, -1.0, float(H), -0.5, H - 0.5])
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    cx = tx[torch.arange(W) % len(tx)][None, :].expand(H, W)
    cy = ty[:, None].expand(H, W)
    edge = torch.stack([cx - xs, cy - ys])[None]
    cases['edge'] = (torch.cat([edge, edge.flip(-1).neg()], 0).contiguous(), None)
    cases['strided'] = (3.0 * torch.randn(2, 2, 9, 33, generator=_gen(14)), None)  # passed as channels 2:4 of a [B,4,H,W] tensor
    return cases


SPLAT_SMOOTH_SHAPES = [(1, 1, 1), (2, 7, 31), (2, 9, 33), (3, 17, 65), (1, 5, 257), (5, 8, 32)]  # (B, H, W)
SPLAT_SMOOTH_MODES = [(1, 1, 1), (2, 1, 1)]  # UFlowLoss: wmode 1, penalty 1, alpha 150
# level-2 grids of the one-launch UFlowLoss backward: (B2, H, W) of the images -> flows [B2,2,H/4,W/4]; w2 = 257: two x-blocks
PAIR_SHAPES = [(2, 8, 1028), (4, 12, 36)]


def splat_smooth_inputs(B, H, W):
    """(flow 2.5 randn, image) of the fused range map + smoothness launch; flow_scale 1"""
    return smooth_flow('R', B, H, W), smooth_image(B, 3, H, W)


# ======================================================================================================================
# masks
# ======================================================================================================================
MASK_SHAPES = [(2, 9, 63), (1, 17, 96), (2, 5, 191), (1, 3, 192), (1, 4, 257), (1, 33, 130)]
COORD_ONLY_SHAPES = [(3, 1, 1), (1, 1, 300)]


def coord_mask_ref(flow32, mode, mutate=None):
    """arflow_coord_mask, exact: fp32 x + u (mode & 2: the input IS the coordinate), then the closed test 0 <= c <= n-1 (mode
    & 1 == 0: mask_invalid) or the open one (border_mask).  mutate='swap': the two intervals swapped (WRONG on purpose)."""
    c = flow32.float() if mode & 2 else abs_coords(flow32.float())
    H, W = c.shape[2:]
    cx, cy = c[:, 0:1], c[:, 1:2]
    closed = (mode & 1) == 0
    if mutate == 'swap':
        closed = not closed
    if closed:
        ok = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
    else:
        ok = (cx > 0) & (cx < W - 1) & (cy > 0) & (cy < H - 1)
    return ok.float()


def coord_mask_flow(B, H, W):
    """4 randn, with a patch of pixels whose x + u and y + v land exactly on 0, W-1 and H-1 (where the closed and the open
    interval differ): column x of rows 0 .. gets u = target - x, exact in fp32."""
    f = 4.0 * torch.randn(B, 2, H, W, generator=_gen(21, B, H, W))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    n = min(W, 12)
    tx = torch.tensor([0.0, W - 1.0, (W - 1) / 2.0])[torch.arange(n) % 3]
    ty = torch.tensor([(H - 1) / 2.0, (H - 1) / 2.0, 0.0, H - 1.0])[torch.arange(n) % 4]
    for r in range(min(H, 2)):
        f[:, 0, r, :n] = tx - xs[r, :n]
        f[:, 1, r, :n] = ty - ys[r, :n]
    return f


def occ_flows(B, H, W):
    """f12 smooth (3 x upsampled coarse noise), f21 = -f12 + 0.45 randn: both outcomes of the test are present"""
    gen = _gen(22, B, H, W)
    f12 = 3.0 * _coarse_noise(gen, B, 2, H, W)
    f21 = -f12 + 0.45 * torch.randn(B, 2, H, W, generator=gen)
    return f12.contiguous(), f21.contiguous()


def occ_bidir_ref(f12, f21, scale=0.01, bias=0.5):
    """get_occu_mask_bidirection (utils/warp_utils.py:93-100) in float64: f21 sampled bilinearly at p + f12(p) with zeros
    outside, |f12 + f21w|^2 > scale (|f12|^2 + |f21w|^2) + bias.  -> (decision [B,1,H,W] float32, margin |lhs - rhs| /
    (lhs + rhs)).  (The normalise / un-normalise round trip of flow_warp is the identity in exact arithmetic.)"""
    a, s = f12.to(D), f21.to(D)
    B, _, H, W = a.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=D), torch.arange(W, dtype=D), indexing='ij')
    ix, iy = xs + a[:, 0], ys + a[:, 1]
    fx, fy = torch.floor(ix), torch.floor(iy)
    wx1, wy1 = ix - fx, iy - fy
    flat = s.reshape(B, 2, H * W)
    warped = torch.zeros_like(a)
    for dy, wy in ((0, 1 - wy1), (1, wy1)):
        for dx, wx in ((0, 1 - wx1), (1, wx1)):
            xi, yi = fx + dx, fy + dy
            ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long().reshape(B, 1, -1).expand(B, 2, H * W)
            warped += flat.gather(2, idx).view(B, 2, H, W) * (wx * wy * ok.to(D)).unsqueeze(1)
    lhs = ((a + warped) ** 2).sum(1, keepdim=True)
    rhs = scale * ((a ** 2).sum(1, keepdim=True) + (warped ** 2).sum(1, keepdim=True)) + bias
    return (lhs > rhs).float(), (lhs - rhs).abs() / (lhs + rhs)


def strided(t):
    """the same values as channels 2:4 of a [B,4,H,W] tensor (flow_bstride = 4 H W); channels 0:2 hold NaN"""
    B, _, H, W = t.shape
    wide = torch.full((B, 4, H, W), float('nan'))
    wide[:, 2:4] = t
    return wide


# ======================================================================================================================
# resize helpers
# ======================================================================================================================
UP4_SHAPES = [(2, 1, 1), (1, 3, 5), (2, 5, 65), (1, 2, 257)]  # (B, h, w)
DOWN4_SHAPES = [(1, 4, 4), (2, 8, 1028), (3, 12, 260)]  # (B, H, W)


def up4_clamp_mul_ref(small, valid=None, mutate=None):
    """upsample(clamp(small, 0, 1), x4, bilinear, align_corners=False) * valid (losses/uflow_loss.py:41-48), float64, written
    out: source coordinate max(0.25 (d + 0.5) - 0.5, 0), both taps clamped.  mutate: 'noclamp', 'novalid' (WRONG on purpose)."""
    s = small.to(D)
    if mutate != 'noclamp':
        s = s.clamp(0.0, 1.0)
    B, _, h, w = s.shape

    def taps(n_in):
        src = (0.25 * (torch.arange(4 * n_in, dtype=D) + 0.5) - 0.5).clamp_min(0.0)
        i0 = src.floor().long().clamp_max(n_in - 1)
        i1 = (i0 + 1).clamp_max(n_in - 1)
        return i0, i1, src - i0
    y0, y1, ly = taps(h)
    x0, x1, lx = taps(w)
    rows = s[:, :, y0] * (1 - ly)[:, None] + s[:, :, y1] * ly[:, None]
    out = rows[..., x0] * (1 - lx) + rows[..., x1] * lx
    if valid is not None and mutate != 'novalid':
        out = out * valid.to(D)
    return out


def down4_ref(img):
    """downsample(img, x1/4, bilinear, align_corners=False) on a multiple-of-4 grid: the mean of the central 2 x 2 of every
    4 x 4 block (source coordinate 4 i + 1.5)."""
    i = img.to(D)
    return 0.25 * (i[:, :, 1::4, 1::4] + i[:, :, 1::4, 2::4] + i[:, :, 2::4, 1::4] + i[:, :, 2::4, 2::4])


def gray255_ref(img):
    """rgb_to_grayscale(img) * 255 (utils/uflow_utils.py:227-231, 248), float64"""
    i = img.to(D)
    return ((i[:, 0] * 0.2989 + i[:, 1] * 0.5870 + i[:, 2] * 0.1140) * 255.0).unsqueeze(1)


def up4_inputs(B, h, w):
    gen = _gen(31, B, h, w)
    return 2.5 * torch.randn(B, 1, h, w, generator=gen), torch.randn(B, 1, 4 * h, 4 * w, generator=gen)


def down4_input(B, H, W):
    return torch.randn(B, 3, H, W, generator=_gen(32, B, H, W))


def worst(err, bound):
    """max err / bound over the elements (0 / 0 counts as 0, x / 0 as inf)"""
    if err.numel() == 0:
        return 0.0
    err = err.to(D)
    bound = torch.as_tensor(bound, dtype=D).expand_as(err)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')),
                                                                         torch.zeros_like(err)))
    return float(r.max())
