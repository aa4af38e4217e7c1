"""Shared by tests/test_penalty_em_cpu.py, tests/test_penalty_em_gpu.py and tools/make_penalty_em_golden.py: a float64
restatement, in plain torch on the CPU, of the one-pass EM fit of the Gaussian-mixture penalty (csrc/penalty_em.hip,
arflow_amd/penalty_em.py) -- the four sufficient statistics, the update built on them, log_gmm and its gradient -- with the
error bounds the GPU tests hold the kernels to, the seeded inputs and deliberate mutations.  Nothing here imports the oracle
or the product.

Reference arithmetic: train_penalty_em.py:86-220 (class EM), losses/uflow_elbo_loss.py:99-105 (log_gmm).

THE OPERATION (float64; x a sample, w its weight, j a component)
    logw_j = digamma(alpha_bar_j) - digamma(sum alpha_bar) + log(beta_j) / 2
    a_j = -beta_j (x - mu_j)^2 / 2 + logw_j     c = max_j a_j     e_j = exp(a_j - c)     den = sum_j e_j
    xi_j = e_j / den                            log xi_j = a_j - c - log(den)
    S0_j = sum w xi_j    S1_j = sum w xi_j x    S2_j = sum w xi_j (x - mu_j)^2    H_j = sum w xi_j log xi_j
    update():   alpha_bar = alpha + S0,  pi = alpha_bar / sum alpha_bar,  beta = (2a - 1 + S0) / (2b + beta_0 (mu - mu_0)^2 + S2)
    objective = sum_j [(a - 1/2) log beta - beta_0 beta (mu - mu_0)^2 / 2 - b beta + (S0 (log beta - log 2 pi) - beta S2) / 2 - H]
                + sum_j lgamma(alpha_bar_j) - lgamma(sum alpha_bar)           (xi of the OLD parameters, the NEW beta, alpha_bar)
    a moved mean mu' = mu + d keeps xi:  S2' = S2 - 2 d (S1 - mu S0) + d^2 S0

BOUNDS, u = 2^-53.  Assumed of the device functions, from the ROCm device-library documentation (taken on trust, not
measured): float64 exp and log are accurate to 1 ulp (relative E_EXP u = E_LOG u = 2 u).  First order in u:
    a_j        d = x - mu: 1 rounding, d d: 1, the product with -beta: 1 (/ 2 exact), + logw: 1
               da_j = 3 u beta_j q_j / 2 + u |a_j|;    s_j = a_j - c: 1 more: ds_j = da_j + da_c + u |s_j|  (c = a of the argmax)
    e_j        relative re_j = ds_j + E_EXP u        (a component whose e_j underflows contributes 0 on both sides)
    den        positive terms, k - 1 additions: relative rden = sum_j e_j re_j / den + (k - 1) u
    xi_j       rxi_j = re_j + rden + u;   t_j = w xi_j: rt_j = rxi_j + u
    terms      S0: t_j rt_j;   S1: |t_j x| (rt_j + u);   S2: t_j q_j (rt_j + 3 u)  (q formed again: 2 roundings, the product 1)
               H: lxi_j = s_j - L, L = log(den):  dlxi_j = ds_j + (rden + E_LOG u |L|) + u |lxi_j|;  |t_j| dlxi_j + |t_j lxi_j| (rt_j + u)
    sums       the sum of the term bounds + depth u sum |term|;  depth = the lane's chain ceil(share / 256) + 6 (wave butterfly) +
               4 (waves 0..3 onto 0.0) + the number of partials (index-order fold).  S0, S2 >= 0 and H <= 0 termwise, so
               sum |term| = |sum|: the bound is RELATIVE for them; S1 is bounded against sum |t_j x|.
    factor 2   the restatement itself rounds as the kernel does (float64 torch ops, another order of addition): its own error obeys
               the same expression, so a comparison of the two is held to TWICE the bound (SAFETY).
    update()   first order through the k-sized formulas (update_bounds): alpha_bar: dS0;  pi_j: dS0_j / sum + pi_j sum dS0 / sum;
               beta: beta (dS0 / num + dS2 / den);  objective: sum_j |g_S0| dS0 + beta dS2 / 2 + dH + |g_beta| dbeta + |g_ab| dS0 with
               g_S0 = (log beta - log 2 pi) / 2, g_beta = (a - 1/2 + S0 / 2) / beta - beta_0 (mu - mu_0)^2 / 2 - b - S2 / 2,
               g_ab = digamma(alpha_bar_j) - digamma(sum alpha_bar);  + K_OPS u times the sum of the absolute values of the
               objective's terms for torch's own k-sized float64 arithmetic (K_OPS = 64: digamma / lgamma / log at a few ulp and
               about a dozen additions; the terms are added in another order than the reference adds its m x k array).
    mu moves   the re-centring identity subtracts terms of the size of S2 + 2 |d (S1 - mu S0)| + d^2 S0 to leave S2'; on the recorded
               sequence (MU_START, |d| <= 0.24) that sum is at most 3.7 S2' for every component; the statistics themselves carry
               the relative bounds above (at most 1.5e-14 from MU_START on the fixture), so S2' is good to 3.7 x 3 x 1.5e-14 < 2e-13
               and beta, the objective and the second mean move follow it: the sequence is compared at rtol 1e-11, fifty times
               that (the reference sums its m x k array directly, without this term).
    log_gmm    in the dtype of x (v = its unit roundoff): arg_j = -beta_j x^2 / 2: 3 roundings (beta to the dtype, x x, the product);
               an exponent error 3 v |arg_j| on a term of relative weight exp(arg_j - c) is at most 3 v (|c| + 1) of the sum; exp, log, the
               products with w_j and the k additions: a few v; the last addition v |out|:  |dout| <= 8 v (1 + |c| + |out|) (LG_K = 8).
               gradient -(sum r_j beta_j) x: relative 3 v (|c| + 1) + 8 v against sum r_j beta_j |x|  (all terms of one sign).
"""
import math
import types

import numpy as np
import torch

D = torch.float64
U = 2.0 ** -53
E_EXP = 2.0   # float64 exp: 1 ulp
E_LOG = 2.0   # float64 log: 1 ulp
SAFETY = 2.0
K_OPS = 64.0
LG_K = 8.0
LOG2PI = math.log(2 * math.pi)

M = 4099
SCALES = (0.05, 0.5, 3.0)
INIT_VARS = [0.001, 0.005, 0.01, 0.05, 0.1, 0.5, 1, 5, 10, 50]  # train_penalty_em.py:52
N_UPDATES = 8
EM_NT, EM_UNIT, EM_MAX_PARTS = 256, 1024, 1024  # csrc/penalty_em.hip
MUTATIONS = ('no_weight', 'no_sqrt_beta', 'drop_last', 'xlogx_product')
PRIOR = dict(mu_0=0.0, beta_0=1e-3, a=1.0, b=1.0)


def make_samples(m=M, seed=1234):
    """-> (x0 fp32 [m]: normal draws at three scales in turn, x1 fp32 [m] in [0.1, 1.1)), numpy"""
    rng = np.random.RandomState(seed)
    scale = np.asarray(SCALES)[np.arange(m) % len(SCALES)]
    x0 = (rng.standard_normal(m) * scale).astype(np.float32)
    x1 = (0.1 + rng.random_sample(m)).astype(np.float32)
    return x0, x1


def share(m):
    units = -(-int(m) // EM_UNIT)
    return EM_UNIT * -(-units // EM_MAX_PARTS)


def partials(m):
    return -(-int(m) // share(m))


def depth(m):
    return -(-min(share(m), int(m)) // EM_NT) + 6 + 4 + partials(m)


def logw_of(alpha_bar, beta, mutate=None):
    lw = torch.special.digamma(alpha_bar) - torch.special.digamma(alpha_bar.sum())
    return lw if mutate == 'no_sqrt_beta' else lw + torch.log(beta) / 2


def stats_ref(x0, x1, logw, beta, mu, mutate=None):
    """x0 [m], x1 [m] or None, logw / beta / mu [k] (anything torch.as_tensor takes) -> namespace of float64 k-vectors S0, S1,
    S2, H and their bounds bS0 .. bH (already times SAFETY), and xi [m, k].  mutate (WRONG on purpose): 'no_weight' drops x1,
    'drop_last' leaves out the last sample, 'xlogx_product' forms xi log(xi) from the underflowed xi (0 * -inf = NaN);
    'no_sqrt_beta' is logw_of's."""
    x = torch.as_tensor(x0).to(D).reshape(-1)
    w = torch.ones_like(x) if x1 is None or mutate == 'no_weight' else torch.as_tensor(x1).to(D).reshape(-1)
    logw, beta, mu = (torch.as_tensor(t).to(D).reshape(-1) for t in (logw, beta, mu))
    m, k = x.numel(), beta.numel()
    if mutate == 'drop_last':
        x, w = x[:-1], w[:-1]
    d = x[:, None] - mu[None, :]
    q = d * d
    half = beta[None, :] * q / 2
    a = -half + logw[None, :]
    c, arg = a.max(dim=1, keepdim=True)
    s = a - c
    e = torch.exp(s)
    den = e.sum(dim=1, keepdim=True)
    L = torch.log(den)
    xi = e / den
    lxi = torch.log(xi) if mutate == 'xlogx_product' else s - L
    t = w[:, None] * xi
    terms = dict(S0=t, S1=t * x[:, None], S2=t * q, H=t * lxi)
    # bounds
    da = 3 * U * half + U * a.abs()
    ds = da + torch.gather(da, 1, arg) + U * s.abs()
    re = ds + E_EXP * U
    rden = (e * re).sum(dim=1, keepdim=True) / den + (k - 1) * U
    rt = re + rden + 2 * U
    dlxi = ds + rden + E_LOG * U * L.abs() + U * lxi.abs()
    tb = dict(S0=t * rt, S1=terms['S1'].abs() * (rt + U), S2=terms['S2'] * (rt + 3 * U),
              H=t * dlxi + terms['H'].abs() * (rt + U))
    out = types.SimpleNamespace(xi=xi)
    for name in ('S0', 'S1', 'S2', 'H'):
        setattr(out, name, terms[name].sum(dim=0))
        setattr(out, 'b' + name, SAFETY * (tb[name].sum(dim=0) + depth(m) * U * terms[name].abs().sum(dim=0)))
    return out


class EMRef:
    """class EM of train_penalty_em.py:86-220 on the four statistics, float64 on the CPU.  mutate='new_beta_in_xi' (WRONG on
    purpose): objective() forms xi again from the NEW beta and alpha_bar instead of pairing the stored statistics with them."""

    def __init__(self, init_vars=INIT_VARS, mutate=None):
        k = len(init_vars)
        self.k, self.mutate = k, mutate
        self.alpha = torch.ones(k, dtype=D)
        self.mu_0, self.beta_0, self.a, self.b = PRIOR['mu_0'], PRIOR['beta_0'], PRIOR['a'], PRIOR['b']
        self.pi = torch.ones(k, dtype=D) / k
        self.mu = torch.zeros(k, dtype=D)
        self.beta = 1 / torch.tensor(init_vars, dtype=D)
        self.alpha_bar = self.alpha.clone()
        self.st = None

    def update_xi(self, x):
        smut = self.mutate if self.mutate in MUTATIONS else None
        self.st = stats_ref(x[0], x[1], logw_of(self.alpha_bar, self.beta, smut), self.beta, self.mu, smut)

    def update_pi(self, x=None):
        self.alpha_bar = self.alpha + self.st.S0
        self.pi = self.alpha_bar / self.alpha_bar.sum()

    def _move_mu(self, mu):
        d = mu - self.mu
        self.st.S2 = self.st.S2 - 2 * d * (self.st.S1 - self.mu * self.st.S0) + d * d * self.st.S0
        self.mu = mu

    def update_mu_ml(self, x=None):
        self._move_mu(self.st.S1 / self.st.S0)

    def update_mu_map(self, x=None):
        self._move_mu((self.beta_0 * self.mu_0 + self.st.S1) / (self.beta_0 + self.st.S0))

    def update_beta_map(self, x=None):
        self.beta = (2 * self.a - 1 + self.st.S0) / (2 * self.b + self.beta_0 * (self.mu - self.mu_0) ** 2 + self.st.S2)

    def objective_terms(self):
        st, lb = self.st, torch.log(self.beta)
        return [(self.a - 0.5) * lb, -(self.beta_0 * self.beta * (self.mu - self.mu_0) ** 2) / 2, -self.b * self.beta,
                st.S0 * (lb - LOG2PI) / 2, -self.beta * st.S2 / 2, -st.H, torch.lgamma(self.alpha_bar),
                -torch.lgamma(self.alpha_bar.sum()).reshape(1)]

    def objective(self, x=None):
        if self.mutate == 'new_beta_in_xi':
            keep = self.st
            self.update_xi(x)
            val = sum(t.sum() for t in self.objective_terms())
            self.st = keep
            return val
        return sum(t.sum() for t in self.objective_terms())

    def update(self, x):
        self.update_xi(x)
        self.update_pi(x)
        self.update_beta_map(x)
        return self.objective(x)


def update_bounds(em):
    """The bounds of alpha_bar, pi, beta and the objective after em.update(x) (em: an EMRef that has just run it), first order
    from the statistics' bounds (the docstring's `update()` entry).  -> namespace alpha_bar, pi, beta [k], objective (scalar)."""
    st = em.st
    tot = em.alpha_bar.sum()
    num = 2 * em.a - 1 + st.S0
    den = 2 * em.b + em.beta_0 * (em.mu - em.mu_0) ** 2 + st.S2
    b_ab = st.bS0 + 2 * U * em.alpha_bar
    b_pi = b_ab / tot + em.pi * b_ab.sum() / tot + 4 * U * em.pi
    b_beta = em.beta * (st.bS0 / num + st.bS2 / den + 4 * U)
    lb = torch.log(em.beta)
    g_s0 = (lb - LOG2PI) / 2
    g_beta = (em.a - 0.5 + st.S0 / 2) / em.beta - em.beta_0 * (em.mu - em.mu_0) ** 2 / 2 - em.b - st.S2 / 2
    g_ab = torch.special.digamma(em.alpha_bar) - torch.special.digamma(tot)
    mag = sum(t.abs().sum() for t in em.objective_terms())
    b_obj = (g_s0.abs() * st.bS0 + em.beta * st.bS2 / 2 + st.bH + g_beta.abs() * b_beta + g_ab.abs() * b_ab).sum() + K_OPS * U * mag
    return types.SimpleNamespace(alpha_bar=b_ab, pi=b_pi, beta=b_beta, objective=b_obj)


def trajectory(x0, x1, init_vars=INIT_VARS, n=N_UPDATES, mutate=None):
    """n updates from the initial state -> dict of float64 arrays pi, alpha_bar, beta [n, k] and objective [n]"""
    em = EMRef(init_vars, mutate)
    rec = {'pi': [], 'alpha_bar': [], 'beta': [], 'objective': []}
    for _ in range(n):
        obj = em.update([x0, x1])
        for key, v in (('pi', em.pi), ('alpha_bar', em.alpha_bar), ('beta', em.beta), ('objective', obj)):
            rec[key].append(v.clone().numpy())
    return {key: np.stack(v) for key, v in rec.items()}


def trajectory_deviation(t, ref):
    """the largest relative deviation of pi, beta and the objective at the LAST update"""
    return max(float(np.max(np.abs(t[key][-1] - ref[key][-1]) / np.abs(ref[key][-1]))) for key in ('pi', 'beta', 'objective'))


def permutation_deviation(x0, x1, n_perm=8, seed=99):
    """How far the float64 trajectory moves when the samples are added in another order: the largest trajectory_deviation
    over n_perm seeded permutations (the GPU test's trajectory tolerance is 10 x this)."""
    ref = trajectory(x0, x1)
    rng = np.random.RandomState(seed)
    worst = 0.0
    for _ in range(n_perm):
        p = rng.permutation(len(x0))
        worst = max(worst, trajectory_deviation(trajectory(x0[p], None if x1 is None else x1[p]), ref))
    return worst


MU_START = [0.3, -0.2, 0.1, 0.0, -0.4, 0.25, 0.05, -0.1, 0.6, -0.5]  # the non-zero means of the recorded mu sequence


def mu_sequence(em, x):
    """update_xi, update_mu_ml, update_beta_map, objective, update_mu_map, update_beta_map, objective from em.mu = MU_START
    -> dict of arrays (works for EMRef, the reference's EM and the product's EM alike: only the reference's names are used)"""
    em.mu = torch.as_tensor(MU_START, dtype=em.beta.dtype, device=em.beta.device)
    out = {}
    em.update_xi(x)
    em.update_mu_ml(x)
    out['mu_ml'] = em.mu
    em.update_beta_map(x)
    out['beta_ml'] = em.beta
    out['obj_ml'] = em.objective(x)
    em.update_mu_map(x)
    out['mu_map'] = em.mu
    em.update_beta_map(x)
    out['beta_map'] = em.beta
    out['obj_map'] = em.objective(x)
    return {key: v.detach().cpu().numpy().astype(np.float64) for key, v in out.items()}


# ---- log_gmm ---------------------------------------------------------------------------------------------------------
LG_PI = [0.05, 0.1, 0.15, 0.2, 0.1, 0.1, 0.1, 0.1, 0.05, 0.05]
LG_BETA = [1000.0, 200.0, 100.0, 20.0, 10.0, 2.0, 1.0, 0.2, 0.1, 0.02]


def log_gmm_grid():
    """fp32 grid reaching |x| = 30, with 0 and a few tiny values"""
    g = np.concatenate([np.linspace(-30, 30, 121), [0.0, 1e-3, -1e-3, 1e-20, 0.07, -0.07, 29.999]])
    return g.astype(np.float32)


def log_gmm_ref(x, pi, beta):
    """-> (out, grad, c, gabs) float64 on the CPU: the log-density, d out / d x, the largest exponent and sum r_j beta_j |x|"""
    x = torch.as_tensor(x).to(D)
    pi, beta = torch.as_tensor(pi, dtype=D), torch.as_tensor(beta, dtype=D)
    arg = -beta * (x * x).unsqueeze(-1) / 2
    w = pi * torch.sqrt(beta) / math.sqrt(2 * math.pi)
    c = arg.max(dim=-1).values
    p = w * torch.exp(arg - c.unsqueeze(-1))
    den = p.sum(dim=-1)
    rb = (p * beta).sum(dim=-1) / den
    return c + torch.log(den), -rb * x, c, rb * x.abs()


def log_gmm_bounds(out, c, gabs, dtype):
    v = 2.0 ** -24 if dtype == torch.float32 else U
    return LG_K * v * (1 + c.abs() + out.abs()), (3 * (c.abs() + 1) + LG_K) * v * gabs


# ---- residual collection ---------------------------------------------------------------------------------------------
RES_SHAPE = (2, 16, 24)  # B, H, W of the image pair; the flow is [B, 2, 4, 6]
EDGE_CONSTANT, EDGE_ASYMP, SUBSAMPLE = 150.0, 0.01, 0.5


def residual_inputs(seed=7):
    """-> dict of fp32 torch CPU tensors: im1, im2 [B,3,H,W] (smooth + noise), flow12, flow21 [B,2,H/4,W/4]"""
    B, H, W = RES_SHAPE
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    base = 0.5 + 0.3 * torch.sin(0.4 * xs + 0.2 * ys).view(1, 1, H, W)
    im1 = (base + 0.15 * torch.rand(B, 3, H, W, generator=g, dtype=torch.float32)).clamp(0, 1)
    im2 = (base.roll(1, 3) + 0.15 * torch.rand(B, 3, H, W, generator=g, dtype=torch.float32)).clamp(0, 1)
    flow12 = 0.6 * torch.randn(B, 2, H // 4, W // 4, generator=g, dtype=torch.float32)
    flow21 = 0.6 * torch.randn(B, 2, H // 4, W // 4, generator=g, dtype=torch.float32)
    return dict(im1=im1, im2=im2, flow12=flow12, flow21=flow21)


def collect_rand(shapes, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(*s, generator=g, dtype=torch.float32) for s in shapes]
