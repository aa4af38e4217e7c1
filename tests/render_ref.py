"""Shared by tests/test_render_cpu.py, tests/test_render_gpu.py and tools/make_render_golden.py: a float64 restatement, in
numpy on the CPU, of the five operations of csrc/render.hip, a numpy-fp32 emulation of the kernels' operation order, the
error bounds the GPU tests hold the kernels to, the seeded inputs and the deliberate mutations.  Nothing here imports the
oracle or the product.

THE OPERATIONS (inference.py:98-107, utils/flow_utils.py:67-96, trainer/uflow_elbo_trainer.py:245,259-262)
    restore   axis(d, n_in, n_out): src = max(0, (d + 1/2) n_in / n_out - 1/2), i0 = min(floor(src), n_in - 1),
              i1 = min(i0 + 1, n_in - 1), l1 = src - i0, l0 = 1 - l1;  blend = l0y (l0x p00 + l1x p01) + l1y (l0x p10 + l1x p11)
              flow_out = blend (W / w, H / h), ent_out = blend + (2 log W - 2 log w, 2 log H - 2 log h), NHWC
              stats = (max(|u|, |v|), max(u, v)) per sample of flow_out
    rgb       n = f / scale;  (1 + n_u, 1 - (n_u + n_v) / 2, 1 + n_v) clipped to [0,1];  uint8 = trunc(255 c)
    wheel     h = mod(atan2(v, u) / 2 pi + 1, 1), s = clip(8 |f| / scale, 0, 1), val = clip(8 - s, 0, 1) (= 1), hsv_to_rgb:
              i = floor(6 h), f = 6 h - i, p = val (1 - s), q = val (1 - s f), t = val (1 - s (1 - f)),
              (r,g,b) = (val,t,p) (q,val,p) (p,val,t) (p,q,val) (t,p,val) (val,p,q) for i mod 6 = 0..5;  uint8 = trunc(255 c)
    a scale that is not positive and finite: n = 0 (rgb), s = 0 (wheel) -- both white.  The reference casts NaN there.
    scalar    e = sum_c x_c;  (e - min) / (max - min), min and max over the whole batch;  max == min renders 0

BOUNDS, u = 2^-24, U1 = u (1 + 2^-20) (the slack covers the second-order terms).  No constant is fitted.
    restore, per output element, M = the largest |tap| of its four taps, s the scale factor:
        l1 = fl(src - i0) from a float64 src: 1 rounding, <= u;  l0 = fl(1 - l1): <= u / 2 more    -> (dl0 + dl1) M <= 3 u M
        top / bot = fl(fl(l0 p0) + fl(l1 p1)): the products u (l0 + l1) M = u M, the sum u M         -> 5 u M each
        blend = fl(fl(l0y top) + fl(l1y bot)): weights 3 u M, carried 5 u M, products u M, sum u M   -> K_BLEND = 10 u M
        flow: fl(blend s) in float64, rounded once: u |out|;  entropy: fl(blend + shift), rounded once: u |out|
    the golden file's restore (tools/make_render_golden.py: the reference's lines through a float64 half-pixel resize): the
        two fp32 roundings of p / w * W (of the two additions of the shift) on every tap and the cast of the result: 3 u more
    wheel, per channel in units of the 8-bit level, with A_ULP = 4 ulp for atan2f and S_ULP = 1 ulp for sqrtf:
        dh   = A_ULP ulp(|angle|) / 2 pi + u / 2 (2 pi as a float) + u / 2 (the quotient) + 2 u (the sum, in [1/2, 3/2])
        df   = 6 dh + 4 u (6 h < 8);  f = 6 h - i is exact
        ds   = s (3/2 u (u u + v v: two squares, one sum, halved by the root) + S_ULP 2 u + u (the quotient)) < 5 u s; 0 where
               s is 0 or clipped with that margin
        role val: exact (8 - s >= 7 clips to 1);  role p: ds + u |1 - s| (s times 1 is exact)
        role q (g = f) / t (g = 1 - f, dg = df + u g): ds g + s dg + u s g + u |1 - s g|
        within df of a sector boundary the neighbouring sector's roles are as good: s df more on every channel
        level: d = 255 dc + u 255 c; 0 where dc = 0 (the channel is exactly 0 or 1 there in fp32 too, and 255 c is exact)
        A channel may be floor(q - d) .. floor(q + d); where these two differ the channel is `inside a band`.
    scalar: de = (C - 1) u sum|x_c|;  r = (e - min) / range: (2 de + u |e - min| + r (2 de + u range)) / range + u r
"""
import numpy as np

U = 2.0 ** -24
U1 = U * (1 + 2.0 ** -20)
K_BLEND = 10
K_GOLDEN = 3
A_ULP = 4  # atan2f: an assumption, twice the 2 ulp CUDA documents; nobody measured it on this runtime
S_ULP = 1  # sqrtf: correctly rounded by default under hipcc; one ulp allowed
F32 = np.float32

# (B, h, w, H, W): non-integer upscale, downscale, identity, degenerate axis, W no multiple of 4 (even: the wide store's path
# with a partial last workgroup), B = 3 with an odd W (the scalar path)
RESTORE_SHAPES = [(2, 12, 20, 31, 53), (2, 12, 20, 5, 7), (1, 8, 12, 8, 12), (2, 1, 9, 4, 9), (2, 12, 20, 10, 134),
                  (3, 6, 5, 9, 11)]
RENDER_SHAPES = [(3, 5, 7), (2, 33, 67)]  # odd sizes: the scalar path; (2, 32, 68) below: the wide path
RENDER_SHAPES_WIDE = [(2, 32, 68)]
SEED = 7


def make_flow(seed, B, h, w, amp=6.0):
    """Seeded [B,2,h,w] fp32 flow whose largest magnitude per sample is NEGATIVE (so absmax and the signed max differ)."""
    g = np.random.default_rng(seed)
    f = (amp * g.standard_normal((B, 2, h, w))).astype(F32)
    f[:, 0, 0, 0] = F32(-4.5 * amp)
    return f


def make_entropy(seed, B, h, w):
    g = np.random.default_rng(seed + 1000)
    return (-1.0 + 1.5 * g.standard_normal((B, 2, h, w))).astype(F32)


def make_wheel_flow(seed, B, H, W):
    """make_flow plus the named pixels: sample 0 holds one pixel on the negative u axis (v = +0) and one on the positive
    u axis; the LAST sample is all zero when B >= 3."""
    f = make_flow(seed, B, H, W)
    f[0, :, H // 2, W // 2] = (-3.0, 0.0)
    f[0, :, H // 2, W // 2 - 1] = (2.5, 0.0)
    if B >= 3:
        f[B - 1] = 0
    return f


# ---- restore ------------------------------------------------------------------------------------------------------------
def axis64(n_in, n_out, align=False):
    d = np.arange(n_out, dtype=np.float64)
    if align:
        src = d * ((n_in - 1) / (n_out - 1)) if n_out > 1 else np.zeros(n_out)
    else:
        src = np.maximum((d + 0.5) * (float(n_in) / float(n_out)) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def _taps(x, ay, ax):
    (y0, y1, _), (x0, x1, _) = ay, ax
    return x[..., y0[:, None], x0[None, :]], x[..., y0[:, None], x1[None, :]], x[..., y1[:, None], x0[None, :]], \
        x[..., y1[:, None], x1[None, :]]


def blend64(x, out_hw, align=False):
    """x [...,h,w] -> (float64 blend [...,H,W], the largest |tap| per output element)"""
    h, w = x.shape[-2:]
    H, W = out_hw
    ay, ax = axis64(h, H, align), axis64(w, W, align)
    p00, p01, p10, p11 = _taps(x.astype(np.float64), ay, ax)
    ly, lx = ay[2][:, None], ax[2][None, :]
    out = (1 - ly) * ((1 - lx) * p00 + lx * p01) + ly * ((1 - lx) * p10 + lx * p11)
    return out, np.maximum(np.maximum(abs(p00), abs(p01)), np.maximum(abs(p10), abs(p11)))


def blend32(x, out_hw, align=False):
    """the kernel's order (resize_dev.hpp): float64 coordinate, l1 rounded once, fp32 products and sums, no contraction"""
    h, w = x.shape[-2:]
    H, W = out_hw
    ay, ax = axis64(h, H, align), axis64(w, W, align)
    p00, p01, p10, p11 = _taps(x.astype(F32), ay, ax)
    l1y, l1x = ay[2].astype(F32)[:, None], ax[2].astype(F32)[None, :]
    l0y, l0x = F32(1) - l1y, F32(1) - l1x
    top = l0x * p00 + l1x * p01
    bot = l0x * p10 + l1x * p11
    out = l0y * top + l1y * bot
    assert out.dtype == F32
    return out


def restore_factors(h, w, H, W):
    import math
    return (float(W) / float(w), float(H) / float(h)), (2 * math.log(W) - 2 * math.log(w), 2 * math.log(H) - 2 * math.log(h))


def restore64(flow, out_hw, ent=None, mutate=None):
    """-> dict(flow [B,H,W,2] float64, flow_bound, ent, ent_bound, stats [B,2] float64)"""
    B, _, h, w = flow.shape
    H, W = out_hw
    scale, shift = restore_factors(h, w, H, W)
    v, M = blend64(flow, out_hw)
    s = np.array(scale)[None, :, None, None]
    out = v * s
    res = {'flow': np.moveaxis(out, 1, -1), 'flow_bound': np.moveaxis((K_BLEND * U1 * M * s + U1 * abs(out)), 1, -1)}
    if ent is not None:
        e, Me = blend64(ent, out_hw)
        eo = e + np.array(shift)[None, :, None, None]
        res['ent'] = np.moveaxis(eo, 1, -1)
        res['ent_bound'] = np.moveaxis(K_BLEND * U1 * Me + U1 * abs(eo), 1, -1)
    res['stats'] = stats64(res['flow'])
    return res


def golden_extra_bound(flow, out_hw, ent=None):
    """what the golden file's own fp32 roundings add to restore64's bounds: (flow part, entropy part or None)"""
    B, _, h, w = flow.shape
    scale, shift = restore_factors(h, w, *out_hw)
    _, M = blend64(flow, out_hw)
    fb = np.moveaxis(K_GOLDEN * U1 * M * np.array(scale)[None, :, None, None], 1, -1)
    eb = None
    if ent is not None:
        _, Me = blend64(ent, out_hw)
        big = 2 * max(abs(np.log(out_hw[0])), abs(np.log(out_hw[1])), abs(np.log(h)), abs(np.log(w)))
        eb = np.moveaxis(K_GOLDEN * U1 * (Me + big), 1, -1)
    return fb, eb


def stats64(flow_nhwc, mutate=None):
    a = np.asarray(flow_nhwc)
    B = a.shape[0]
    absmax = abs(a).reshape(B, -1).max(1)
    smax = a.reshape(B, -1).max(1)
    return np.stack([smax if mutate == 'signed_absmax' else absmax, smax], 1)


def restore32(flow, out_hw, ent=None, mutate=None):
    """the kernel's fp32 order -> dict(flow [B,H,W,2] fp32, ent, stats [B,2] fp32).  mutate: 'align', 'inverse_scale',
    'shift_sign', 'swap_uv', 'signed_absmax'."""
    B, _, h, w = flow.shape
    H, W = out_hw
    scale, shift = restore_factors(h, w, H, W)
    if mutate == 'inverse_scale':
        scale = (1 / scale[0], 1 / scale[1])
    if mutate == 'shift_sign':
        shift = (-shift[0], -shift[1])
    align = mutate == 'align'
    v = blend32(flow, out_hw, align).astype(np.float64)
    out = (v * np.array(scale)[None, :, None, None]).astype(F32)
    pack = (lambda t: np.ascontiguousarray(np.moveaxis(t[:, ::-1], 1, -1))) if mutate == 'swap_uv' else \
        (lambda t: np.ascontiguousarray(np.moveaxis(t, 1, -1)))
    res = {'flow': pack(out), 'ent': None}
    if ent is not None:
        e = blend32(ent, out_hw, align).astype(np.float64)
        res['ent'] = pack((e + np.array(shift)[None, :, None, None]).astype(F32))
    res['stats'] = stats64(res['flow'], mutate).astype(F32)
    return res


# ---- colour ---------------------------------------------------------------------------------------------------------------
def _scale_ok(s):
    return np.isfinite(s) & (s > 0)


def rgb32(flow, scale, as_uint8):
    """np_flow2rgb's fp32 sequence.  flow [B,2,H,W] fp32, scale [B] fp32 -> uint8 [B,H,W,3] or fp32 [B,3,H,W]."""
    flow, scale = flow.astype(F32), np.asarray(scale, F32).reshape(-1, 1, 1, 1)
    ok = _scale_ok(scale)
    with np.errstate(all='ignore'):
        n = np.where(ok, flow / np.where(ok, scale, F32(1)), F32(0)).astype(F32)
    c = np.stack([F32(1) + n[:, 0], F32(1) - F32(0.5) * (n[:, 0] + n[:, 1]), F32(1) + n[:, 1]], 1).clip(0, 1)
    assert c.dtype == F32
    return np.moveaxis((F32(255) * c).astype(np.uint8), 1, -1) if as_uint8 else c


def rgb64(flow, scale):
    """-> float64 [B,3,H,W] in [0,1]"""
    flow, scale = flow.astype(np.float64), np.asarray(scale, np.float64).reshape(-1, 1, 1, 1)
    ok = _scale_ok(scale)
    n = np.where(ok, flow / np.where(ok, scale, 1.0), 0.0)
    return np.stack([1 + n[:, 0], 1 - 0.5 * (n[:, 0] + n[:, 1]), 1 + n[:, 1]], 1).clip(0, 1)


_ROLES = np.array([[0, 3, 1], [2, 0, 1], [1, 0, 3], [1, 2, 0], [3, 1, 0], [0, 1, 2]])  # sector -> role of (r, g, b): 0 val 1 p 2 q 3 t


def _sectors(h, s, val, shift=0):
    h6 = h * 6
    i = np.floor(h6).astype(np.int64)
    f = h6 - i
    roles = _ROLES[(i + shift) % 6]  # [..., 3]
    cand = np.stack([val, val * (1 - s), val * (1 - s * f), val * (1 - s * (1 - f))], -1)
    c = np.take_along_axis(cand, roles, -1)
    return np.where((s == 0)[..., None], val[..., None], c), f, roles


def wheel64(flow, scale, mutate=None):
    """flow [B,2,H,W], scale [B] -> (q = 255 c float64 [B,H,W,3], d the level bound [B,H,W,3]).  mutate: 'sector'."""
    u, v = flow[:, 0].astype(np.float64), flow[:, 1].astype(np.float64)
    scale = np.asarray(scale, np.float64).reshape(-1, 1, 1)
    ok = _scale_ok(scale)
    mag = np.sqrt(u * u + v * v)
    ang = np.arctan2(v, u)
    h = np.mod(ang / (2 * np.pi) + 1, 1)
    s_raw = np.where(ok, 8 * mag / np.where(ok, scale, 1.0), 0.0)
    s = np.clip(s_raw, 0, 1)
    val = np.clip(8 - s, 0, 1)
    c, f, roles = _sectors(h, s, val, 1 if mutate == 'sector' else 0)
    dh = A_ULP * np.spacing(np.abs(ang).astype(F32)).astype(np.float64) / (2 * np.pi) + 3 * U
    df = 6 * dh + 4 * U
    ds = np.where((s_raw == 0) | (s_raw * (1 - 5 * U) >= 1), 0.0, 5 * U * np.minimum(s_raw, 1 + 5 * U))
    g = np.stack([np.zeros_like(f), np.ones_like(f), f, 1 - f], -1)
    dg = np.stack([np.zeros_like(f), np.zeros_like(f), df, df + U * (1 - f)], -1)
    sg = s[..., None] * g
    dc_role = ds[..., None] * g + s[..., None] * dg + U * np.where(g == 1, 0.0, sg) + U * abs(1 - sg)
    dc_role[..., 0] = 0
    dc = np.take_along_axis(dc_role, roles, -1)
    near = (f < df) | (f > 1 - df)
    dc = dc + np.where(near, s * df, 0.0)[..., None]
    dc = np.where((s == 0)[..., None], 0.0, dc)
    q = 255 * c
    # dc == 0: the channel is exactly 0 or 1 in fp32 as well (val; s == 0; p with s clipped), and 255 c is then exact
    assert np.all((dc > 0) | (c == 0) | (c == 1))
    return q, np.where(dc == 0, 0.0, (255 * dc + U * q) * (1 + 2.0 ** -20))


def wheel32(flow, scale):
    """the kernel's fp32 order (libm's atan2 and sqrt stand in for the device's) -> uint8 [B,H,W,3]"""
    u, v = flow[:, 0].astype(F32), flow[:, 1].astype(F32)
    scale = np.asarray(scale, F32).reshape(-1, 1, 1)
    ok = _scale_ok(scale)
    mag = np.sqrt(u * u + v * v)
    h = np.arctan2(v, u) / F32(6.2831855) + F32(1)
    h = h - np.floor(h)
    with np.errstate(all='ignore'):
        s = np.where(ok, (mag * F32(8) / np.where(ok, scale, F32(1))).clip(0, 1), F32(0)).astype(F32)
    val = (F32(8) - s).clip(0, 1)
    h6 = h * F32(6)
    i = h6.astype(np.int32)
    f = h6 - i.astype(F32)
    cand = np.stack([val, val * (F32(1) - s), val * (F32(1) - s * f), val * (F32(1) - s * (F32(1) - f))], -1)
    c = np.where((s == 0)[..., None], val[..., None], np.take_along_axis(cand, _ROLES[i % 6], -1))
    assert c.dtype == F32
    return (F32(255) * c).astype(np.uint8)


def level_range(q, d):
    """-> (lo, hi) int64: the levels trunc(255 c) may take when q = 255 c is known to within d"""
    return np.clip(np.floor(q - d), 0, 255).astype(np.int64), np.clip(np.floor(q + d), 0, 255).astype(np.int64)


def band_check(got, q, d):
    """-> (number of channel values outside [lo, hi], share of channel values inside a band)"""
    lo, hi = level_range(q, d)
    got = np.asarray(got).astype(np.int64)
    return int(((got < lo) | (got > hi)).sum()), float((lo != hi).mean())


# ---- scalar ----------------------------------------------------------------------------------------------------------------
def scalar32(x, as_uint8):
    """x [B,C,H,W] fp32 -> uint8 [B,H,W] / fp32 [B,H,W] in the kernel's order"""
    x = x.astype(F32)
    e = x[:, 0]
    for c in range(1, x.shape[1]):
        e = e + x[:, c]
    mn, rng = e.min(), e.max() - e.min()
    r = (e - mn) / rng if rng > 0 else np.zeros_like(e)
    assert r.dtype == F32
    return (F32(255) * r).astype(np.uint8) if as_uint8 else r


def scalar64(x):
    """-> (r float64 [B,H,W], its bound)"""
    x = x.astype(np.float64)
    e, de = x.sum(1), (x.shape[1] - 1) * U1 * abs(x).sum(1)
    mn, rng = e.min(), e.max() - e.min()
    if rng <= 0:
        return np.zeros_like(e), np.zeros_like(e)
    r = (e - mn) / rng
    dmax = de.max()
    return r, ((de + dmax) + U1 * abs(e - mn) + r * (2 * dmax + U1 * rng)) / rng + U1 * r
