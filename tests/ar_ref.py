"""Shared by tests/test_ar_cpu.py, tests/test_ar_gpu.py and tools/kbench.py: a float64 restatement, in plain torch on the CPU,
of the augmentation-regularisation arithmetic of csrc/ar.hip (arflow_amd/ar.py states it), and the same
transform composed of ATen operations (composed(): the "today" side of the kernel benchmark).  Nothing here imports the oracle.

THE ARITHMETIC (restated from the definitions)
    s = (a x' + b y' + tx, c x' + d y' + ty);   bilinear sample with zero padding at s (flow_warp(., s - p', pad='zeros'));
    flow_t = L^-1 g:  u_t = (d g_u - b g_v) / det,  v_t = (a g_v - c g_u) / det;   mask_t = sample(noc or ones) *
    [0 < s_x < Ws - 1 and 0 < s_y < Hs - 1];   loss = sum (|pred - flow_t| + eps)^q m / (2 N) / (sum m / N + 1e-7), N = B H W.

BOUND.  With track=True every quantity is carried as (value, absolute error bound) through the KERNEL's fp32 operations in the
kernel's order (class V, in the manner of tests/augment_ref.py): a sum or difference adds the operands' bounds, a product
|a| db + |b| da + da db, a quotient (da + |q| db) / (|b| - db), each plus u |result| for the operation's one rounding, u = 2^-24
-- except that an operation on EXACT operands (bound 0) whose float64 result is a float32 number rounds to itself: bound 0.
(That keeps the anchors exact: an identity, a flip or an integer translation has s, weights 1 and 0 and every product exact.)
    s            three roundings: (a x' + b y') + tx through V; the bound of s is (dsx, dsy)
    sample       the zero-padded bilinear interpolant F is continuous and piecewise bilinear, so evaluating it at the kernel's
                 s instead of the exact one moves it by at most Gx dsx + Gy dsy, Gx / Gy the largest absolute difference of
                 horizontal / vertical neighbours within two pixels of the cell; the kernel's own roundings -- l1 = s -
                 floor(s), l0 = 1 - l1, four weight products, four tap products, three sums -- go through V at the exact s,
                 and where s lies within its bound of an integer (the kernel may sit in the neighbouring cell) another
                 27 u Pmax is added (1 + 2 per weight factor, 1 per product, 6 u per tap product, 3 sums; Pmax the largest
                 |tap| within two pixels)
    flow         det = a d - b c, the two numerators and the two IEEE quotients through V
    mask         the border decision is the exact s's; where s lies within its bound of 0, Ws - 1 or Hs - 1 the kernel may
                 decide otherwise and the bound is 1 (the tests' caps forbid that: their cases keep s away from the border or
                 exactly on it)
    loss         e = pred - flow_t and t = |e| + eps through V; powf within 2 ulp of pow (4 u |z|) plus the larger of
                 |pow(t +- dt) - pow(t)| (pow is monotone); the products with m and the sums are float64 on both sides
    gradient     k = (float)g0 * q, pw = powf(t, q - 1) (the exponent's own rounding: |z ln t| u |q - 1|), (k pw) m through V
No constant is fitted.
"""
import math

import torch
import torch.nn.functional as Fn

U = 2.0 ** -24
PAD = 3  # s is clamped into [-2, Ws + 1]: taps -2 .. Ws + 2


def _representable(z):
    return z.float().double() == z


class V:
    """A float64 tensor and the bound of the fp32 kernel's absolute error on it (None: not tracked)."""

    def __init__(self, v, e=None):
        self.v, self.e = v, e

    tracked = property(lambda self: self.e is not None)

    def _other(self, o):
        if isinstance(o, V):
            return o
        o = torch.as_tensor(o, dtype=torch.float64)
        return V(o, torch.zeros_like(o) if self.tracked else None)

    @staticmethod
    def _rn(z, e):
        if e is None:
            return V(z)
        exact = (e == 0) & _representable(z)
        return V(z, torch.where(exact, torch.zeros_like(e), e + U * z.abs()))

    def __add__(self, o):
        o = self._other(o)
        return self._rn(self.v + o.v, self.e + o.e if self.tracked else None)

    __radd__ = __add__

    def __sub__(self, o):
        o = self._other(o)
        return self._rn(self.v - o.v, self.e + o.e if self.tracked else None)

    def __rsub__(self, o):
        return self._other(o) - self

    def __mul__(self, o):
        o = self._other(o)
        e = self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e if self.tracked else None
        return self._rn(self.v * o.v, e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._other(o)
        q = self.v / o.v
        e = None
        if self.tracked:
            den = o.v.abs() - o.e
            e = torch.where(den > 0, (self.e + q.abs() * o.e) / den.clamp_min(1e-300), torch.full_like(q, float('inf')))
        return self._rn(q, e)

    def __neg__(self):
        return V(-self.v, self.e)

    def abs(self):
        return V(self.v.abs(), self.e)  # 1-Lipschitz, exact


def exact(t, track):
    t = t.double()
    return V(t, torch.zeros_like(t) if track else None)


def where(m, a, b):
    return V(torch.where(m, a.v, b.v), torch.where(m, a.e, b.e) if a.tracked else None)


MUTATIONS = ('L', 'LT', 'nodet', 'swap', 'nonstrict')


def _pool5(t):
    """[C,Hp,Wp] >= 0 -> the largest value within two pixels, same shape."""
    return Fn.max_pool2d(t[None], 5, 1, 2)[0]


def _sample(plane, sx, sy, track, mutate):
    """plane [C,Hs,Ws] float64, sx / sy V [H,W] -> V [C,H,W]: the zero-padded bilinear sample in the kernel's order."""
    C, Hs, Ws = plane.shape
    P = Fn.pad(plane, (PAD, PAD, PAD, PAD))
    cx, cy = sx.v.clamp(-2.0, Ws + 1.0), sy.v.clamp(-2.0, Hs + 1.0)
    fx, fy = cx.floor(), cy.floor()
    zero = torch.zeros_like(cx) if track else None
    # outside the clamp every tap is outside the plane: the value is exactly 0 on both sides whatever the weights
    l1x = V._rn(cx - fx, zero)
    l1y = V._rn(cy - fy, zero)
    l0x, l0y = 1.0 - l1x, 1.0 - l1y
    x0, y0 = fx.long(), fy.long()

    def tap(dy, dx):
        return exact(P[:, y0 + dy + PAD, x0 + dx + PAD], track)

    def w(ly, lx, dy, dx):
        ok = (y0 + dy >= 0) & (y0 + dy < Hs) & (x0 + dx >= 0) & (x0 + dx < Ws)
        return where(ok, ly * lx, exact(torch.zeros_like(cx), track))
    w00, w01, w10, w11 = w(l0y, l0x, 0, 0), w(l0y, l1x, 0, 1), w(l1y, l0x, 1, 0), w(l1y, l1x, 1, 1)
    p01, p10 = (tap(1, 0), tap(0, 1)) if mutate == 'swap' else (tap(0, 1), tap(1, 0))
    out = ((w00 * tap(0, 0) + w01 * p01) + w10 * p10) + w11 * tap(1, 1)
    if track:
        gx = _pool5(Fn.pad((P[:, :, 1:] - P[:, :, :-1]).abs(), (0, 1)))
        gy = _pool5(Fn.pad((P[:, 1:, :] - P[:, :-1, :]).abs(), (0, 0, 0, 1)))
        pm = _pool5(P.abs())
        yi, xi = y0 + PAD, x0 + PAD
        near = ((sx.e > 0) & ((cx - cx.round()).abs() <= sx.e)) | ((sy.e > 0) & ((cy - cy.round()).abs() <= sy.e))
        out.e = out.e + gx[:, yi, xi] * sx.e + gy[:, yi, xi] * sy.e + near * (27 * U) * pm[:, yi, xi]
    return out


def transform(theta, img=None, flow=None, noc=None, out_hw=None, track=False, mutate=None):
    """theta float32 [B,6]; img [B,C,Hs,Ws], flow [B,2,Hs,Ws], noc [B,1,Hs,Ws] float32 (or None), all on the CPU ->
    dict(img_t, flow_t, mask_t [, e_img, e_flow, e_mask], s=(sx, sy) float64 [B,H,W]); a group without a source is None, except
    mask_t (ones for an absent noc).  mutate: one of MUTATIONS, a deliberately wrong restatement."""
    assert mutate is None or mutate in MUTATIONS
    first = next(t for t in (img, flow, noc) if t is not None)
    B, (Hs, Ws) = first.shape[0], first.shape[2:]
    H, W = (Hs, Ws) if out_hw is None else out_hw
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    res = {k: [] for k in ('img_t', 'flow_t', 'mask_t', 'e_img', 'e_flow', 'e_mask', 'sx', 'sy')}
    for n in range(B):
        a, b, tx, c, d, ty = (exact(theta[n, k], track) for k in range(6))
        X, Y = exact(xs, track), exact(ys, track)
        sx, sy = (a * X + b * Y) + tx, (c * X + d * Y) + ty
        res['sx'].append(sx.v), res['sy'].append(sy.v)
        if img is not None:
            o = _sample(img[n].double(), sx, sy, track, mutate)
            res['img_t'].append(o.v), res['e_img'].append(o.e)
        if flow is not None:
            g = _sample(flow[n].double(), sx, sy, track, mutate)
            gu, gv = V(g.v[0], g.e[0] if track else None), V(g.v[1], g.e[1] if track else None)
            det = a * d - b * c
            if mutate == 'L':
                u, v = a * gu + b * gv, c * gu + d * gv
            elif mutate == 'LT':
                u, v = a * gu + c * gv, b * gu + d * gv
            elif mutate == 'nodet':
                u, v = d * gu - b * gv, a * gv - c * gu
            else:
                u, v = (d * gu - b * gv) / det, (a * gv - c * gu) / det
            res['flow_t'].append(torch.stack([u.v, v.v])), res['e_flow'].append(torch.stack([u.e, v.e]) if track else None)
        src = torch.ones(1, Hs, Ws, dtype=torch.float64) if noc is None else noc[n].double()
        m = _sample(src, sx, sy, track, mutate)
        if mutate == 'nonstrict':
            inside = (sx.v >= 0) & (sx.v <= Ws - 1) & (sy.v >= 0) & (sy.v <= Hs - 1)
        else:
            inside = (sx.v > 0) & (sx.v < Ws - 1) & (sy.v > 0) & (sy.v < Hs - 1)
        res['mask_t'].append(m.v * inside)
        if track:
            edge = torch.minimum(torch.minimum(sx.v.abs(), (sx.v - (Ws - 1)).abs()) - sx.e,
                                 torch.minimum(sy.v.abs(), (sy.v - (Hs - 1)).abs()) - sy.e)
            unsure = (edge <= 0) & ~((sx.e == 0) & (sy.e == 0))
            res['e_mask'].append(torch.where(unsure[None], torch.ones_like(m.e), m.e * inside))

    def cat(k):
        return torch.stack(res[k]) if res[k] and res[k][0] is not None else None
    out = {k: cat(k) for k in ('img_t', 'flow_t', 'mask_t', 'e_img', 'e_flow', 'e_mask')}
    out['s'] = (torch.stack(res['sx']), torch.stack(res['sy']))
    return out


def border_margin(s, src_hw):
    """The smallest distance of any s from 0, Ws - 1 (x) or 0, Hs - 1 (y)."""
    sx, sy = s
    Hs, Ws = src_hw
    return float(torch.minimum(torch.minimum(sx.abs(), (sx - (Ws - 1)).abs()), torch.minimum(sy.abs(), (sy - (Hs - 1)).abs())).min())


def _pow(t, q, track, dexp=0.0):
    z = torch.pow(t.v, q)
    if not track:
        return V(z)
    hi, lo = torch.pow(t.v + t.e, q), torch.pow((t.v - t.e).clamp_min(0.0), q)
    e = torch.maximum((hi - z).abs(), (z - lo).abs()) + 4 * U * z.abs()
    if dexp:
        e = e + (z * t.v.clamp_min(1e-300).log()).abs() * dexp
    return V(z, e)


def loss(pred, flow_t, mask=None, eps=0.0, q=1.0, track=False):
    """float32 CPU tensors -> (loss, grad [B,2,H,W]) float64, and with track (loss, grad, e_loss, e_grad): the bounds of the
    fp32 kernels' errors.  eps and q are taken as the float32 numbers the kernels receive."""
    B, _, H, W = pred.shape
    N = float(B * H * W)
    eps, q = float(torch.tensor(eps, dtype=torch.float32)), float(torch.tensor(q, dtype=torch.float32))
    m = torch.ones(B, 1, H, W, dtype=torch.float64) if mask is None else mask.double()
    e = exact(pred, track) - exact(flow_t, track)
    t = e.abs() + eps
    v = t if q == 1.0 else _pow(t, q, track)
    den = m.sum() / N + 1e-7
    value = (v.v * m).sum() / (2 * N) / den
    g0 = 1.0 / (2 * N) / den
    k = V(g0, U * g0.abs() if track else None) * q   # (float)g0: one rounding of a float64 number
    if q == 1.0:
        pw = exact(torch.ones_like(t.v), track)
    else:
        q1 = float(torch.tensor(q, dtype=torch.float32) - 1.0)  # the kernel's fp32 q - 1
        pw = _pow(t, q1, track, dexp=U * abs(q1))
    g = (k * pw) * exact(m, track)
    sign = torch.sign(e.v)
    grad = g.v * sign
    if not track:
        return value, grad
    e_loss = (v.e * m).sum() / (2 * N) / den + 1e-14 * value.abs()
    # where e is not separated from its bound the kernel's sign may differ (it cannot at e == 0 from exact operands)
    e_grad = torch.where(e.v.abs() > e.e, g.e, g.e + g.v.abs())
    return value, grad, e_loss, e_grad


def composed(theta, img=None, flow=None, noc=None):
    """The same transform from ATen operations on the tensors' device, float32: what a caller composes today -- the grid of
    the reference's flow_warp (normalised, align_corners=True), one grid_sample per group, the border mask and the 2 x 2
    product.  -> (img_t, flow_t, mask_t)."""
    first = next(t for t in (img, flow, noc) if t is not None)
    B, _, H, W = first.shape
    dev = first.device
    th = theta.to(dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                            indexing='ij')
    a, b, tx, c, d, ty = (th[:, k].reshape(B, 1, 1) for k in range(6))
    sx, sy = a * xs + b * ys + tx, c * xs + d * ys + ty
    grid = torch.stack([2.0 * sx / (W - 1) - 1.0, 2.0 * sy / (H - 1) - 1.0], -1)

    def warp(t):
        return Fn.grid_sample(t, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    img_t = None if img is None else warp(img)
    flow_t = None
    if flow is not None:
        g = warp(flow)
        det = (a * d - b * c)
        flow_t = torch.stack([(d * g[:, 0] - b * g[:, 1]) / det, (a * g[:, 1] - c * g[:, 0]) / det], 1)
    inside = ((sx > 0) & (sx < W - 1) & (sy > 0) & (sy < H - 1)).unsqueeze(1).float()
    mask_t = (inside if noc is None else warp(noc) * inside)
    return img_t, flow_t, mask_t


def composed_loss(pred, flow_t, mask=None, eps=0.0, q=1.0):
    """The loss from ATen operations (losses/penalty_functions.py:3-4 under the mask mean), differentiable in pred."""
    B, _, H, W = pred.shape
    m = torch.ones(B, 1, H, W, device=pred.device, dtype=pred.dtype) if mask is None else mask
    return (torch.pow((pred - flow_t).abs() + eps, q) * m).mean() / (m.mean() + 1e-7)


# ---- the cases the tests run (built from seeds; the bounds depend on these inputs alone) ---------------------------------
def centred(z, phi, hw, tau=(0.0, 0.0), flip=False):
    """One row of theta in float64 -> float32: s = c + R(phi) diag(+-1/z, 1/z) (p' - c) + tau."""
    H, W = hw
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    sg = -1.0 if flip else 1.0
    a, b, c, d = math.cos(phi) * sg / z, -math.sin(phi) / z, math.sin(phi) * sg / z, math.cos(phi) / z
    return [a, b, cx - (a * cx + b * cy) + tau[0], c, d, cy - (c * cx + d * cy) + tau[1]]


def case(hw, C, seed=0, integer_shift=False):
    """B = 3: zoom 1.3 with rotation 0.2; zoom 0.8 (zero padding shows); flip + translation (whole pixels with
    integer_shift, which puts s exactly on the border in a column and a row) -> (theta, img, flow, noc) float32 on the CPU.
    noc lies in [0.5, 1]: a border decision taken the other way moves mask_t by at least 0.5."""
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    shift = (-5.0, 3.0) if integer_shift else (-5.37, 3.21)
    flip_row = [-1.0, 0.0, (W - 1) + shift[0], 0.0, 1.0, shift[1]]
    theta = torch.tensor([centred(1.3, 0.2, hw), centred(0.8, 0.0, hw, tau=(0.31, -0.27)), flip_row], dtype=torch.float64).float()
    img = torch.rand(3, C, H, W, generator=g)
    flow = 3.0 * torch.randn(3, 2, H, W, generator=g)
    noc = 0.5 + 0.5 * torch.rand(3, 1, H, W, generator=g)
    return theta, img, flow, noc


def mutation_cap(hw, C):
    """Half the smallest of the five mutations' largest errors on the case's inputs: what a derived bound may not exceed.  (The
    non-strict border only shows where some s lies exactly on the border: it runs on the whole-pixel variant of the case.)"""
    worst = []
    for mut in MUTATIONS:
        args = case(hw, C, integer_shift=(mut == 'nonstrict'))
        good, bad = transform(*args), transform(*args, mutate=mut)
        worst.append(max(float((good[k] - bad[k]).abs().max()) for k in ('img_t', 'flow_t', 'mask_t')))
    return min(worst) / 2.0


def loss_case(hw=(37, 53), seed=1):
    """B = 3 at 37 x 53: pred and flow_t a few pixels apart, equal exactly on a block; a fractional mask -> (pred, flow_t, m)."""
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    flow_t = 3.0 * torch.randn(3, 2, H, W, generator=g)
    pred = flow_t + torch.randn(3, 2, H, W, generator=g)
    pred[:, :, 5:9, 7:20] = flow_t[:, :, 5:9, 7:20]
    m = torch.rand(3, 1, H, W, generator=g)
    return pred, flow_t, m
