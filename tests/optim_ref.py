"""Shared by tests/test_optim_cpu.py, tests/test_optim_gpu.py and tools/make_optim_golden.py: a numpy float64 restatement of the
three update rules of csrc/optim.hip, the gradient clip and the learning-rate schedule, with the error bound of the fp32 kernel
per element.  Nothing here imports the oracle or torch (a torch tensor handed in is used through its own methods); the product is
imported for CHUNK only.

THE RULES (restated from the definitions: torch.optim.Adam / SGD as documented, the reference's AdamW from
utils/torch_utils.py:146-159 -- nothing copied).  g: the gradient times coef; wd: the element's group decay; t = 1, 2, ...
    bc1 = 1 - beta1^t   bc2 = 1 - beta2^t
    adam    g += wd p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
    adamw   the moments from g alone;  p -= (lr sqrt(bc2) / bc1) m / (sqrt(v) + eps);  then p -= wd p   (not scaled by lr)
    sgd     g += wd p;  buf = g at t = 1, else mu buf + g;  p -= lr buf
    clip    total = sqrt(sum g^2) over ALL parameters;  coef = min(1, clip / (total + 1e-6))   (clip_grad_norm_);  off: coef = 1
    schedule  lr *= factor at the end of every epoch i with i >= lr_decay_start_epoch (ExponentialLR under base_trainer.py:52-54)

BOUND.  Every quantity is carried as (value, absolute error bound) through the KERNEL's fp32 operations in the kernel's order
(the header of csrc/optim.hip; class V): a sum or difference adds the operands' bounds, a product |a| db + |b| da + da db, a
quotient (da + |q| db) / (|b| - db), a square root sqrt(v) - sqrt(max(v - dv, 0)) (the larger side, sqrt is concave), each plus
u (|result| + propagated bound) + 2^-149 for the operation's one rounding (u = 2^-24; the last term covers a subnormal
result).  The scalars the kernel rounds to fp32 once (the betas, 1 - beta, eps, wd, lr, sqrt(bc2), the step sizes) carry u |c|.
coef is formed in float64 from float64 partial sums of exact squares and rounded once: u coef + 1e-12 coef (the summation
order; n 2^-53 is far below); where clip / (total + 1e-6) exceeds 1 by more than 1e-9 both sides clamp to exactly 1: bound 0.
The inputs (parameters, gradients) are fp32 numbers: bound 0.  The state carries its bound from step to step.  No constant is
fitted.  Bitwise equality with torch's own kernels is neither required nor expected (torch forms m by lerp and p by addcdiv).

MUTATIONS (the discriminating-power test): each is a wrong reading of a rule that a correct kernel must be told from.
"""
import numpy as np

from arflow_amd.optim import CHUNK

U = 2.0 ** -24
ETA = 2.0 ** -149
SIZES = (1, 2, 3, 5, 16, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3)
NAMES = tuple('t%d.%s' % (i, 'weight' if i % 2 == 0 else 'bias') for i in range(len(SIZES)))
N = sum(SIZES)
STEPS = 3
MUTATIONS = ('no_bc2', 'eps_in_sqrt', 'decay_bias', 'adamw_decay_lr', 'l2_after_moments', 'coef_unclamped')

# the train sections of the fixture's trajectories; every one runs with clip 'on' (norm > clip), 'slack' (norm < clip), 'off'.
# adamw: the reference's class does not scale its decay by lr, so the shipped 1e-6 moves a parameter by 1e-6 |p| a step, 8 times
# the fp32 bound of that parameter; 1e-2 (a customary AdamW value) makes the lr-scaled mutation visible at >= 10 bounds
RULE_CFG = {
    'adam0': dict(optim='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, bias_decay=0.0),
    'adam': dict(optim='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-6, bias_decay=0.0),
    'adamw': dict(optim='adamw', lr=1e-3, momentum=0.9, beta=0.999, weight_decay=1e-2, bias_decay=0.0),
    'sgd': dict(optim='sgd', lr=1e-2, momentum=0.9, weight_decay=1e-6, bias_decay=0.0),
}
CLIPS = ('on', 'slack', 'off')
CASES = tuple('%s_%s' % (r, c) for r in RULE_CFG for c in CLIPS)
SCHEDULE = dict(lr=1e-4, lr_decay_factor=0.98, lr_decay_start_epoch=3, epochs=(1, 2, 3, 4, 5))


def make_inputs():
    """Seeded fp32 parameters [N] and three gradient sets [3, N] in the order of SIZES / NAMES: magnitudes spread over decades,
    signs that flip between steps on about half of the elements, and exact zeros (a parameter element without gradient)."""
    rng = np.random.RandomState(20261020)
    p = (rng.randn(N) * 10.0 ** rng.uniform(-3, 0, N)).astype(np.float32)
    mag = 10.0 ** rng.uniform(-5, -1, N)
    g = np.stack([rng.randn(N) * mag * np.where(rng.rand(N) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, N) for _ in range(STEPS)])
    g[:, ::97] = 0.0          # never a gradient
    g[1, 5::89] = 0.0         # none in the second step only
    return p, g.astype(np.float32)


def clip_values(g):
    """clip 'on' is a quarter of the smallest of the three gradient norms, 'slack' four times the largest."""
    norms = np.sqrt((g.astype(np.float64) ** 2).sum(1))
    return {'on': float(0.25 * norms.min()), 'slack': float(4.0 * norms.max()), 'off': -1.0}


def case_cfg(case, g):
    rule, clip = case.rsplit('_', 1)
    return dict(RULE_CFG[rule], clip=clip_values(g)[clip])


def decay_vector(names, sizes, weight_decay, bias_decay, mutate=None):
    """Per element: the decay of its tensor's group (a name ending in `bias`: bias_decay)."""
    out = []
    for nm, n in zip(names, sizes):
        bias = nm.endswith('bias') and mutate != 'decay_bias'
        out.append(np.full(n, bias_decay if bias else weight_decay, dtype=np.float64))
    return np.concatenate(out)


def schedule(lr, factor, start, epochs):
    out = []
    for i in epochs:
        if i >= start:
            lr = lr * factor
        out.append(lr)
    return np.asarray(out, dtype=np.float64)


def _where(mask, a, b):
    return a.where(mask, b) if hasattr(a, 'where') else np.where(mask, a, b)


class V:
    """An array, and the bound of the fp32 kernel's absolute error on it.  Arrays are numpy float64; a torch float64 tensor (the
    GPU test restates a whole model's step on the device) passes through the same operations; scalars stay Python floats."""

    def __init__(self, v, e=None):
        if np.isscalar(v):
            v = float(v)
        elif isinstance(v, np.ndarray) or isinstance(v, (list, tuple)):
            v = np.asarray(v, dtype=np.float64)
        else:
            v = v.double()
        self.v = v
        self.e = v * 0.0 if e is None else e

    @staticmethod
    def of(o):
        return o if isinstance(o, V) else V(o)

    @staticmethod
    def _rn(z, e):
        return V(z, e + U * (abs(z) + e) + ETA)

    def __add__(self, o):
        o = V.of(o)
        return V._rn(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = V.of(o)
        return V._rn(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = V.of(o)
        return V._rn(self.v * o.v, abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = V.of(o)
        q = self.v / o.v
        den = abs(o.v) - o.e + q * 0.0     # of q's shape also where the divisor is a scalar
        e = _where(den > 0, (self.e + abs(q) * o.e) / den.clip(min=1e-300), np.inf)
        return V._rn(q, e)

    def sqrt(self):
        r = self.v ** 0.5
        return V._rn(r, r - (self.v - self.e).clip(min=0.0) ** 0.5)

    def where(self, mask, other):
        return V(_where(mask, self.v, other.v), _where(mask, self.e, other.e))


def const(c):
    """A double the kernel rounds to fp32 once."""
    return V(float(c), U * abs(float(c)))


def clip_coef(g, clip, mutate=None):
    """-> V scalar.  g: the whole flat gradient (fp32 values)."""
    if not clip > 0:
        return V(1.0)
    total = np.sqrt((np.asarray(g, dtype=np.float64) ** 2).sum())
    raw = clip / (total + 1e-6)
    if mutate == 'coef_unclamped':
        return V(raw, raw * (U + 1e-12))
    if raw > 1.0 + 1e-9:
        return V(1.0)
    c = min(1.0, raw)
    return V(c, c * (U + 1e-12))


def step(cfg, t, p, g, m, v, wd, coef, mutate=None):
    """One step of rule cfg['optim'] -> (p, m, v) as V (v is None for sgd).  p, m, v: V; g: fp32 values; wd: float64 per element
    (decay_vector); coef: V scalar (clip_coef)."""
    rule = cfg['optim']
    lr = cfg['lr']
    g = coef * V(g)
    has = wd != 0
    wdc = V(wd, U * abs(wd))
    if rule == 'sgd':
        mu = cfg['momentum']
        g = (g + wdc * p).where(has, g)
        m = g if t == 1 else const(mu) * m + g
        return p - const(lr) * m, m, None
    if rule == 'adam':
        b1, b2, eps = cfg['beta1'], cfg['beta2'], cfg['eps']
        if mutate != 'l2_after_moments':
            g = (g + wdc * p).where(has, g)
    else:
        b1, b2, eps = cfg['momentum'], cfg['beta'], 1e-8
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    m = const(b1) * m + const(1.0 - b1) * g
    v = const(b2) * v + const(1.0 - b2) * (g * g)
    root = (v + const(eps)).sqrt() if mutate == 'eps_in_sqrt' else v.sqrt()
    if rule == 'adam':
        d = root if mutate == 'no_bc2' else root / const(np.sqrt(bc2))
        if mutate != 'eps_in_sqrt':
            d = d + const(eps)
        p = p - const(lr / bc1) * (m / d)
        if mutate == 'l2_after_moments':
            p = (p - const(lr) * (wdc * p)).where(has, p)
        return p, m, v
    d = root if mutate == 'eps_in_sqrt' else root + const(eps)
    p = p - const(lr / bc1 if mutate == 'no_bc2' else lr * np.sqrt(bc2) / bc1) * (m / d)
    decay = const(lr) * (wdc * p) if mutate == 'adamw_decay_lr' else wdc * p
    return (p - decay).where(has, p), m, v


def trajectory(cfg, p0, g, names=NAMES, sizes=SIZES, mutate=None):
    """STEPS steps from p0 [N] with the gradients g [STEPS, N] -> a list of (p, m, v) as V after each step."""
    wd = decay_vector(names, sizes, cfg['weight_decay'], cfg['bias_decay'], mutate)
    p, m, v = V(p0), V(np.zeros(len(p0))), V(np.zeros(len(p0)))
    out = []
    for t in range(1, len(g) + 1):
        coef = clip_coef(g[t - 1], cfg.get('clip', -1.0), mutate)
        p, m, v = step(cfg, t, p, g[t - 1], m, v, wd, coef, mutate)
        out.append((p, m, v))
    return out
