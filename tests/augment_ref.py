"""Shared by tests/test_augment_cpu.py, tests/test_augment_gpu.py and tools/kbench.py: a restatement, in plain torch, of the
whole batch augmentation of csrc/augment.hip from a parameter table (arflow_amd.augment.AugmentParams) -- float64 on the CPU it
is the tests' reference, float32 on the device it is the "composed from ATen operations" side of the kernel benchmark.  Nothing
here imports the oracle; the product is imported for the table's layout only.

THE TRANSFORM (restated from the definitions, nothing copied)
    geometric    transforms/geometric_transforms.py:28-69: RandomCrop (a window (y1, x1, th, tw)), RandomHorizontalFlip
                 (torch.flip of the last axis), Scale (F.interpolate bilinear, align_corners=False), in that order
    photometric  transforms/photometric_transforms.py:7-53: torchvision's ColorJitter (tensor path of
                 torchvision.transforms.functional, from its published formulas -- torchvision is not installed where this was
                 written, so NOTHING here was compared against it), RandomGamma (pow, clamp), RandomSwapChannels (an index
                 permutation of the three channels of every frame)
        gray = 0.2989 r + 0.587 g + 0.114 b         blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1)
        brightness  blend(x, 0, f)     contrast  blend(x, mean over the frame of gray(x), f)     saturation  blend(x, gray(x), f)
        hue         the hexcone round trip of hue() below
    in the sample's operation order, inactive operations skipped; every frame of a sample uses the sample's parameters.

BOUND.  With track=True every quantity is carried as (value, absolute error bound) through the KERNEL's fp32 operations in the
kernel's order (class V): a sum or difference adds the operands' bounds, a product |a| db + |b| da + da db, a quotient
(da + |q| db) / (|b| - db), each plus u |result| for the operation's one rounding, u = 2^-24; max, min and clamp are
1-Lipschitz and exact, and a value beyond 0 or 1 by more than its bound is clamped to the same number on both sides (bound
0); the constants 0.2989, 0.587, 0.114 carry their fp32 rounding.  No constant is fitted.
    source       uint8 / 255 is ONE correctly rounded division: u |v|; a float32 source is exact
    scale        resize() below: the kernel's taps and weights (rf_axis of csrc/resize_dev.hpp: the coordinate in float64, l1
                 rounded to fp32 once, l0 = 1 - l1 one more rounding) and its blend l0y (l0x p00 + l1x p01) + l1y (l0x p10 +
                 l1x p11), carried through V like everything else; the CPU tests hold it to F.interpolate
    mean         per-pixel fp32 gray, summed in float64 (nothing at this scale), the quotient rounded to fp32 once
    hue          the branches (which channel is the maximum, the sector i, the wrap of h at 1) are the REFERENCE's; the
                 kernel may take a neighbouring branch where its operands differ from the reference's by their bounds, and the
                 transform is continuous across every one of them (at r == g == max: bc - gc == 2 + rc - bc; at phi -> 1 of
                 sector i the triple equals sector i + 1 at phi = 0; h is a point on a circle), so the neighbouring branch's
                 result lies within the same propagated bound.  Where the chroma cr is not separated from its own bound
                 (cr <= 4 dcr, dcr > 0) the hue is undefined on either side and the quotient bound is void; there p, q and t all
                 lie in [v (1 - s), v], so the bound is cr + dcr + dv + 4 u instead.  Where the smallest channel is exactly 0 on
                 both sides (value 0, bound 0) the saturation s = maxc / maxc is exactly 1: bound 0
    gamma        powf within 2 ulp of pow (4 u |z|), plus the larger of |pow(x +- dx) - pow(x)| (pow is monotone)
A wrong sector or branch of the hue code moves an output by >= 1e-2; the tests require max(bound) <= 1e-5 (BOUND_CAP).
"""
import torch
import torch.nn.functional as Fn

from arflow_amd import augment as A

U = 2.0 ** -24
BOUND_CAP = 1e-5
BRIGHTNESS, CONTRAST, SATURATION, HUE = range(4)


class V:
    """A tensor, and (tracked) the bound of the fp32 kernel's absolute error on it."""

    def __init__(self, v, e=None):
        self.v, self.e = v, e

    tracked = property(lambda self: self.e is not None)

    def _other(self, o):
        if isinstance(o, V):
            return o
        o = torch.as_tensor(o, dtype=self.v.dtype, device=self.v.device)
        return V(o, torch.zeros_like(o) if self.tracked else None)

    def _rn(self, z, e):
        return V(z, None if e is None else e + U * z.abs())

    def __add__(self, o):
        o = self._other(o)
        return self._rn(self.v + o.v, self.e + o.e if self.tracked else None)

    def __sub__(self, o):
        o = self._other(o)
        return self._rn(self.v - o.v, self.e + o.e if self.tracked else None)

    def __rsub__(self, o):
        return self._other(o) - self

    __radd__ = __add__

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

    def clamp01(self):
        """1-Lipschitz and exact; a value that lies beyond 0 or 1 by more than its bound is clamped on BOTH sides: bound 0."""
        if not self.tracked:
            return V(self.v.clamp(0.0, 1.0))
        both = (self.v + self.e <= 0) | (self.v - self.e >= 1)
        return V(self.v.clamp(0.0, 1.0), torch.where(both, torch.zeros_like(self.e), self.e))

    def __getitem__(self, idx):
        return V(self.v[idx], self.e[idx] if self.tracked else None)

    def put(self, idx, o):
        self.v[idx] = o.v
        if self.tracked:
            self.e[idx] = o.e

    def clone(self):
        return V(self.v.clone(), self.e.clone() if self.tracked else None)


def const(x, c):
    """An fp32 constant of the kernel that is no float32 number."""
    t = torch.as_tensor(c, dtype=x.v.dtype, device=x.v.device)
    return V(t, U * t.abs() if x.tracked else None)


def vmax(a, b):
    return V(torch.maximum(a.v, b.v), torch.maximum(a.e, b.e) if a.tracked else None)


def vmin(a, b):
    return V(torch.minimum(a.v, b.v), torch.maximum(a.e, b.e) if a.tracked else None)


def where(m, a, b):
    return V(torch.where(m, a.v, b.v), torch.where(m, a.e, b.e) if a.tracked else None)


def stack(vs, dim):
    return V(torch.stack([t.v for t in vs], dim), torch.stack([t.e for t in vs], dim) if vs[0].tracked else None)


def gray(x):
    """x [n,F,3,h,w] -> [n,F,h,w], the kernel's order: (0.2989 r + 0.587 g) + 0.114 b."""
    return const(x, 0.2989) * x[:, :, 0] + const(x, 0.587) * x[:, :, 1] + const(x, 0.114) * x[:, :, 2]


def blend(a, b, f):
    f = a._other(f)
    return (f * a + (1.0 - f) * b).clamp01()


def hue(x, f):
    """x [n,F,3,h,w], f [n,1,1,1] (exact float32 numbers)."""
    r, g, b = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    maxc, minc = vmax(vmax(r, g), b), vmin(vmin(r, g), b)
    cr = maxc - minc
    eq = cr.v == 0
    one = V(torch.ones_like(cr.v), torch.zeros_like(cr.v) if x.tracked else None)
    s = cr / where(eq, one, maxc)
    if x.tracked:  # a channel that is exactly 0 on both sides: cr = maxc - 0 is maxc itself and maxc / maxc is exactly 1
        s = where((minc.v == 0) & (minc.e == 0) & ~eq, one, s)
    dv = where(eq, one, cr)
    rc, gc, bc = (maxc - r) / dv, (maxc - g) / dv, (maxc - b) / dv
    is_r, is_g = maxc.v == r.v, maxc.v == g.v
    h = where(is_r, bc - gc, where(is_g, (2.0 + rc) - bc, (4.0 + gc) - rc))
    h = h / 6.0 + 1.0
    h = h - torch.floor(h.v)
    h = h + f
    h = h - torch.floor(h.v)
    h6 = h * 6.0
    i = torch.floor(h6.v)
    ph = V(h6.v - i, h6.e)
    v = maxc
    p = (v * (1.0 - s)).clamp01()
    q = (v * (1.0 - s * ph)).clamp01()
    t = (v * (1.0 - s * (1.0 - ph))).clamp01()
    sector = i.long() % 6
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = []
    for ch in range(3):
        o = table[5][ch]
        for k in range(4, -1, -1):
            o = where(sector == k, table[k][ch], o)
        out.append(o)
    out = stack(out, 2)
    if x.tracked:
        near = (cr.v <= 4 * cr.e) & (cr.e > 0)
        flat = cr.v + cr.e + maxc.e + 4 * U
        out.e = torch.where(near.unsqueeze(2), flat.unsqueeze(2).expand_as(out.e), out.e)
    return out


def jitter(op, x, f):
    """One ColorJitter operation on x [n,F,3,h,w] with the factors f [n,1,1,1,1]."""
    if op == BRIGHTNESS:
        return (x._other(f) * x).clamp01()
    if op == CONTRAST:
        gr = gray(x)
        m = gr.v.mean((-1, -2), keepdim=True)
        mean = V(m, gr.e.mean((-1, -2), keepdim=True) + U * m.abs() if x.tracked else None)
        return blend(x, V(mean.v.unsqueeze(2), mean.e.unsqueeze(2) if x.tracked else None), f)
    if op == SATURATION:
        gr = gray(x)
        return blend(x, V(gr.v.unsqueeze(2), gr.e.unsqueeze(2) if x.tracked else None), f)
    return hue(x, f[:, :, 0])


def gamma(x, gm):
    z = torch.pow(x.v, gm)
    e = None
    if x.tracked:
        hi, lo = torch.pow((x.v + x.e).clamp(0.0, None), gm), torch.pow((x.v - x.e).clamp(0.0, None), gm)
        e = torch.maximum(hi - z, z - lo) + 4 * U * z.abs()
    return V(z, e).clamp01()


def _axis(n_in, n_out, dtype, track):
    """rf_axis with align_corners = False -> (i0, i1, l0, l1), the weights as V [n_out]."""
    d = torch.arange(n_out, dtype=torch.float64)
    pos = ((d + 0.5) * (float(n_in) / float(n_out)) - 0.5).clamp_min(0.0)
    i0 = pos.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    l1 = (pos - i0.double()).to(dtype)
    l1 = V(l1, U * l1.abs() if track else None)
    return i0, i1, 1.0 - l1, l1


def resize(x, out_hw):
    """V [B,F,3,th,tw] -> V [B,F,3,h,w], bilinear, align_corners = False, in the kernel's order of operations."""
    h, w = out_hw
    th, tw = x.v.shape[-2:]
    dev = x.v.device
    y0, y1, ly0, ly1 = _axis(th, h, x.v.dtype, x.tracked)
    x0, x1, lx0, lx1 = _axis(tw, w, x.v.dtype, x.tracked)

    def tap(yi, xi):
        yi, xi = yi.to(dev), xi.to(dev)
        return V(x.v[..., yi, :][..., xi], x.e[..., yi, :][..., xi] if x.tracked else None)

    def col(l):
        return V(l.v.to(dev)[:, None], l.e.to(dev)[:, None] if x.tracked else None)
    lx0, lx1 = V(lx0.v.to(dev), lx0.e.to(dev) if x.tracked else None), V(lx1.v.to(dev), lx1.e.to(dev) if x.tracked else None)
    top = lx0 * tap(y0, x0) + lx1 * tap(y0, x1)
    bot = lx0 * tap(y1, x0) + lx1 * tap(y1, x1)
    return col(ly0) * top + col(ly1) * bot


def geometric(src, params, out_hw=None, dtype=torch.float64, track=False):
    """src [B,F,3,Hs,Ws] uint8 or float -> V [B,F,3,h,w]: crop, flip, scale."""
    dev = src.device
    B, F = src.shape[:2]
    th, tw = params.crop_hw
    flip = params.flip
    rows = params.y1.long()[:, None] + torch.arange(th)[None]
    ar = torch.arange(tw)[None]
    cols = params.x1.long()[:, None] + torch.where(flip[:, None], tw - 1 - ar, ar)
    bi = torch.arange(B)
    x = src[bi[:, None, None].to(dev), :, :, rows[:, :, None].to(dev), cols[:, None, :].to(dev)]  # [B,th,tw,F,3]
    x = x.permute(0, 3, 4, 1, 2)
    if src.dtype == torch.uint8:
        x = x.to(dtype) / 255
        e = U * x.abs() if track else None
    else:
        x = x.to(dtype)
        e = torch.zeros_like(x) if track else None
    h, w = params.out_hw if out_hw is None else tuple(out_hw)
    scale = params.scale_hw is not None if out_hw is None else (h, w) != (th, tw)
    if scale and track:
        return resize(V(x, e), (h, w))
    if scale:
        x = Fn.interpolate(x.reshape(B, 3 * F, th, tw), size=(h, w), mode='bilinear', align_corners=False).reshape(B, F, 3, h, w)
    return V(x.contiguous(), e)


def photometric(x, params):
    """V [B,F,3,h,w] -> V [B,F,3,h,w]: the operations in each sample's order, gamma, the channel permutation."""
    dev, dtype = x.v.device, x.v.dtype
    B = x.v.shape[0]
    x = x.clone()
    order, factors = params.order, params.factors
    for k in range(4):
        for op in range(4):
            sel = ((order[:, k] == op) & params.active(op)).nonzero()[:, 0]
            if sel.numel() == 0:
                continue
            f = factors[sel, op].to(dtype).to(dev)[:, None, None, None, None]
            if sel.numel() == B:
                x = jitter(op, x, f)
            else:
                idx = sel.to(dev)
                x.put(idx, jitter(op, x[idx], f))
    sel = params.gamma_on.nonzero()[:, 0]
    if sel.numel():
        idx = sel.to(dev)
        x.put(idx, gamma(x[idx], params.gamma[sel].to(dtype).to(dev)[:, None, None, None, None]))
    perm = params.perm
    if (perm != torch.arange(3)[None]).any():
        bi = torch.arange(B)[:, None].to(dev)
        x = V(x.v[bi, :, perm.to(dev)].permute(0, 2, 1, 3, 4), x.e[bi, :, perm.to(dev)].permute(0, 2, 1, 3, 4) if x.tracked else None)
    return x


def augment(src, params, out_hw=None, dtype=torch.float64, track=False):
    """-> (img, img_ph, bound, bound_ph): [B,3F,h,w] in `dtype`; the bounds None without track."""
    if src.dim() == 4:
        src = src.reshape(src.shape[0], src.shape[1] // 3, 3, src.shape[2], src.shape[3])
    g = geometric(src, params, out_hw, dtype, track)
    p = photometric(g, params) if params.photometric else g
    B, F, _, h, w = g.v.shape

    def flat(t):
        return None if t is None else t.reshape(B, 3 * F, h, w)
    return flat(g.v), flat(p.v), flat(g.e), flat(p.e)


# ---- the cases the GPU tests run (built from seeds; the bounds depend on these inputs alone) --------------------------------
COLOURS = [(255, 0, 0), (255, 255, 0), (0, 255, 0), (0, 255, 255), (0, 0, 255), (255, 0, 255),        # the six sector boundaries
           (200, 100, 50), (100, 200, 50), (50, 200, 100), (50, 100, 200), (100, 50, 200), (200, 50, 100),  # inside each sector
           (128, 128, 128), (0, 0, 0), (255, 255, 255), (7, 7, 7)]                                     # grey, black, white


def orders_case(crop_hw, src_hw=(13, 22), F=2, seed=0, scale_hw=None):
    """B = 24 samples, one per order of the four operations, every operation active with factors a moderate jitter draws
    (brightness and contrast 0.2, saturation 0.3, hue 0.5), mixed flips, crop origins at 0, at the far corner and at odd x1,
    gamma in [1, 1.5] on two samples of three (behind the jitter an exponent below 1 turns the absolute error e of a channel
    near 0 into e^gamma, 2e-5 at e = 2e-7, for ANY fp32 evaluation: the exponents below 1 are in frames_case, on exact zeros),
    all six channel permutations, COLOURS planted inside every crop window -> (src, params)."""
    import itertools
    g = torch.Generator().manual_seed(seed)
    B, (Hs, Ws), (th, tw) = 24, src_hw, crop_hw
    src = torch.randint(0, 256, (B, F, 3, Hs, Ws), dtype=torch.uint8, generator=g)
    orders = list(itertools.permutations(range(4)))
    perms = list(itertools.permutations(range(3)))
    y1 = [(0, Hs - th, (Hs - th) // 2)[b % 3] for b in range(B)]
    x1 = [(0, Ws - tw, min(1, Ws - tw), min(5, Ws - tw))[b % 4] for b in range(B)]
    flip = [bool((b // 2) % 2) for b in range(B)]
    u = torch.rand(B, 5, generator=g, dtype=torch.float64)
    factors = torch.stack([0.8 + 0.4 * u[:, 0], 0.8 + 0.4 * u[:, 1], 0.7 + 0.6 * u[:, 2], u[:, 3] - 0.5], 1).float().numpy()
    gamma = [float('nan') if b % 3 == 0 else float(1.0 + 0.5 * u[b, 4]) for b in range(B)]
    for b in range(B):
        for k, col in enumerate(COLOURS):
            yy, xx = y1[b] + k // tw, x1[b] + k % tw
            src[b, :, :, yy, xx] = torch.tensor(col, dtype=torch.uint8)[None]
    params = A.make_params((Hs, Ws), (th, tw), y1, x1, flip, orders, [[True] * 4] * B, factors, gamma,
                           [perms[b % 6] for b in range(B)], scale_hw)
    return src, params


def frames_case(F, src_hw=(13, 22), crop_hw=(7, 10), seed=1):
    """B = 6 samples of F frames: brightness alone in front of gamma over its whole range [0.7, 1.5] (0 stays exactly 0 and
    every other value keeps a relative error, so pow is well conditioned), the six channel permutations, mixed flips."""
    import itertools
    g = torch.Generator().manual_seed(seed)
    B, (Hs, Ws), (th, tw) = 6, src_hw, crop_hw
    src = torch.randint(0, 256, (B, F, 3, Hs, Ws), dtype=torch.uint8, generator=g)
    src[:, :, :, :, ::5] = 0
    u = torch.rand(B, 2, generator=g, dtype=torch.float64)
    factors = torch.ones(B, 4, dtype=torch.float64)
    factors[:, 0] = 0.6 + 0.8 * u[:, 0]
    active = [[True, False, False, False]] * B
    gamma = [0.7, 1.5] + [float(0.7 + 0.8 * u[b, 1]) for b in range(2, B)]
    y1 = [(0, Hs - th, 3)[b % 3] for b in range(B)]
    x1 = [(Ws - tw, 0, 7)[b % 3] for b in range(B)]
    params = A.make_params((Hs, Ws), (th, tw), y1, x1, [bool(b % 2) for b in range(B)], None, active, factors.float().numpy(), gamma,
                           list(itertools.permutations(range(3))))
    return src, params


def scale_case(src_hw, crop_hw, out_hw, seed=2):
    """B = 8 samples of 2 frames resized crop_hw -> out_hw behind mixed flips, with what the shipped configs train with (hue
    0.5 and the channel swap).  The resize leaves every value with an absolute error of a few u, which the full jitter of
    orders_case would carry past BOUND_CAP; the hue round trip alone keeps it at about a dozen times that."""
    import itertools
    g = torch.Generator().manual_seed(seed)
    B, (Hs, Ws), (th, tw) = 8, src_hw, crop_hw
    src = torch.randint(0, 256, (B, 2, 3, Hs, Ws), dtype=torch.uint8, generator=g)
    for k, col in enumerate(COLOURS):
        src[:, :, :, (Hs - th) + k // tw, (Ws - tw) + k % tw] = torch.tensor(col, dtype=torch.uint8)[None, None]
    factors = torch.ones(B, 4, dtype=torch.float64)
    factors[:, 3] = torch.rand(B, generator=g, dtype=torch.float64) - 0.5
    perms = list(itertools.permutations(range(3)))
    y1 = [(0, Hs - th)[b % 2] for b in range(B)]
    x1 = [(Ws - tw, 0, (Ws - tw) // 2)[b % 3] for b in range(B)]
    params = A.make_params((Hs, Ws), (th, tw), y1, x1, [bool((b // 2) % 2) for b in range(B)], None, [[False, False, False, True]] * B,
                           factors.float().numpy(), None, [perms[b % 6] for b in range(B)], out_hw)
    return src, params


def contrast_case(src_hw=(40, 70), seed=3):
    """B = 4 samples of 2 whole 40 x 70 frames (more than one partial sum per frame), contrast first, second, third and last
    in the order, behind brightness / saturation / hue as the order has it; sample 3 has contrast alone."""
    g = torch.Generator().manual_seed(seed)
    B, (Hs, Ws) = 4, src_hw
    src = torch.randint(0, 256, (B, 2, 3, Hs, Ws), dtype=torch.uint8, generator=g)
    orders = [(1, 0, 2, 3), (0, 1, 2, 3), (2, 3, 1, 0), (0, 2, 3, 1)]
    u = torch.rand(B, 4, generator=g, dtype=torch.float64)
    factors = torch.stack([0.8 + 0.4 * u[:, 0], 0.6 + 0.8 * u[:, 1], 0.7 + 0.6 * u[:, 2], u[:, 3] - 0.5], 1).float().numpy()
    active = [[True] * 4, [True] * 4, [True] * 4, [False, True, False, False]]
    params = A.make_params((Hs, Ws), (Hs, Ws), [0] * B, [0] * B, [False, True, False, True], orders, active, factors)
    return src, params
