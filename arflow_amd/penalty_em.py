"""The reference's train_penalty_em.py on the native kernels of csrc/penalty_em.hip: collect the
pre-penalty residuals of the data and smoothness terms, fit a zero-mean Gaussian scale mixture to them by variational MAP-EM
(class EM, train_penalty_em.py:86-220) and rescale it to the full width at half maximum of the hand-made penalty it replaces.

The reference's EM keeps the m x k responsibility matrix ``xi`` and forms about fifteen temporaries of that size per update.
Every quantity of ``EM.update`` is a function of four k-vectors of sums over the samples,

    S0_j = sum x1 xi_j      S1_j = sum x1 xi_j x      S2_j = sum x1 xi_j (x - mu_j)^2      H_j = sum x1 xi_j log xi_j

so ``update_xi`` runs ONE pass (arflow_em_stats: xi of a sample lives in registers) and stores these; the other methods read
them.  The k-sized work (digamma, the M-step, the objective) is torch float64 on the device; nothing is read back per update.

Stated differences from the reference:
  * ``self.xi`` is not materialised (it stays None); ``responsibilities(x)`` returns it through torch ops for small m;
  * the parameters are float64 device tensors whatever torch's default dtype is (the script runs in the default, float32);
    the samples may be float32 or float64 and are widened per sample;
  * ``update_mu_ml`` / ``update_mu_map`` move ``mu`` and re-centre the stored S2 on the new ``mu`` by the identity
    S2' = S2 - 2 d (S1 - mu S0) + d^2 S0, d = mu' - mu (float64), which is what the reference's stored xi would give;
  * ``data_loss_no_penalty`` returns ``(losses, weights, occu_mask_2, valid_mask_0)`` as the reference does; for
    occ_type='none' the reference's own return statement names two variables that branch never binds -- here occu_mask_2 is
    None and valid_mask_0 is the mask in that case.

GPU only: a CPU tensor raises ArflowHipError.
"""
import math

import numpy as np
import torch

from . import _lib
from . import functional as AF
from . import uflow_utils as U
from .functional import _call, _p, _stream

__all__ = ['EM', 'fit_penalty', 'fwhm_scale', 'gaussian_mixture', 'robust_l1_fwhm', 'abs_robust_loss_fwhm', 'log_gmm',
           'data_loss_no_penalty', 'smooth_loss_no_penalty', 'collect_samples', 'em_stats', 'em_share', 'penalty_cfg', 'KMAX', 'INIT_VARS']

KMAX = 16         # ARFLOW_EM_KMAX of include/arflow_hip.h
EM_UNIT = 1024    # ARFLOW_EM_UNIT
EM_MAX_PARTS = 1024  # ARFLOW_EM_MAX_PARTS
INIT_VARS = [0.001, 0.005, 0.01, 0.05, 0.1, 0.5, 1, 5, 10, 50]  # train_penalty_em.py:52


def em_share(m):
    """The samples one workgroup of arflow_em_stats takes for m samples (pure host; mirrors csrc/penalty_em.hip)."""
    units = -(-int(m) // EM_UNIT)
    return EM_UNIT * -(-units // EM_MAX_PARTS)


def _need_samples(*tensors):
    dtype = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.ArflowHipError('arflow_amd.penalty_em runs on the GPU only (got a %s tensor); there is no CPU fallback'
                                      % t.device)
        if t.dtype not in (torch.float32, torch.float64) or (dtype is not None and t.dtype != dtype):
            raise _lib.ArflowHipError('arflow_amd.penalty_em takes float32 or float64 tensors of one dtype (got %s)' % t.dtype)
        dtype = t.dtype
    return dtype


def _split(x):
    """x = [x0, x1] or a [2, m] tensor -> (x0, x1); x1 may be None (all ones)."""
    x0, x1 = x[0], x[1]
    if x0.dim() != 1 or (x1 is not None and x1.shape != x0.shape):
        raise ValueError('EM expects x = [x0, x1] with two m-vectors (or a [2, m] tensor)')
    return x0.detach().contiguous(), None if x1 is None else x1.detach().contiguous()


def em_partials(x0, x1, logw, beta, mu):
    """arflow_em_stats -> part [nparts, 4, k] float64: the per-workgroup partial sums (S0, S1, S2, H)."""
    dtype = _need_samples(x0, x1)
    m, k = x0.numel(), logw.numel()
    if not 1 <= k <= KMAX:
        raise ValueError('EM supports 1 <= k <= %d components (got %d)' % (KMAX, k))
    for t in (logw, beta, mu):
        if t.dtype != torch.float64 or t.device != x0.device or t.numel() != k or not t.is_contiguous():
            raise ValueError('logw, beta, mu must be contiguous float64 k-vectors on the samples\' device')
    nparts = _lib.load().arflow_em_partials(m)
    _lib.check(min(nparts, 0), 'arflow_em_partials')
    part = torch.empty(nparts, 4, k, device=x0.device, dtype=torch.float64)
    with torch.cuda.device_of(x0):
        _call('arflow_em_stats', _p(x0), _p(x1), m, int(dtype == torch.float64), _p(logw), _p(beta), _p(mu), k, _p(part),
              _stream(), key=(m, k))
    return part


def em_stats(x0, x1, logw, beta, mu):
    """-> stats [4, k] float64 (S0, S1, S2, H): the partials of em_partials added in index order (arflow_em_fold)."""
    part = em_partials(x0, x1, logw, beta, mu)
    k = logw.numel()
    stats = torch.empty(4, k, device=x0.device, dtype=torch.float64)
    with torch.cuda.device_of(x0):
        _call('arflow_em_fold', _p(part), part.shape[0], k, _p(stats), _stream(), key=(part.shape[0], k))
    return stats


class EM:
    """train_penalty_em.py:86-220 with the reference's names and argument convention (x = [x0, x1]: samples and weights, or a
    [2, m] tensor; x1 may be None for unit weights).  ``update_xi`` stores the four statistics S0, S1, S2, H instead of xi."""

    def __init__(self, k=10, init_vars=[0.01, 0.05, 0.1, 0.25, 0.5, 1, 5, 10, 100, 1000], device=None):
        if not 1 <= k <= KMAX:
            raise ValueError('EM supports 1 <= k <= %d components (got %d)' % (KMAX, k))
        if len(init_vars) != k:
            raise ValueError('init_vars has %d entries for k = %d' % (len(init_vars), k))
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != 'cuda':
            raise _lib.ArflowHipError('arflow_amd.penalty_em runs on the GPU only (got device %s); there is no CPU fallback' % dev)
        f64 = dict(device=dev, dtype=torch.float64)
        # Prior parameters
        self.k = k
        self.alpha = torch.ones(k, **f64)
        self.mu_0 = 0
        self.beta_0 = 1e-3
        self.a = 1
        self.b = 1
        # Variational parameters
        self.pi = torch.ones(k, **f64) / k
        self.mu = torch.zeros(k, **f64)
        self.beta = 1 / torch.tensor(init_vars, **f64)
        self.alpha_bar = self.alpha.clone()
        self.xi = None  # never materialised: see responsibilities()
        self.S0 = self.S1 = self.S2 = self.H = None

    def _logw(self):
        return (torch.special.digamma(self.alpha_bar) - torch.special.digamma(torch.sum(self.alpha_bar, dim=0, keepdim=True))
                + torch.log(self.beta) / 2)

    def _stats(self):
        if self.S0 is None:
            raise RuntimeError('EM: call update_xi(x) first (the statistics of xi are not there yet)')

    def update_xi(self, x):
        x0, x1 = _split(x)
        stats = em_stats(x0, x1, self._logw().contiguous(), self.beta.contiguous(), self.mu.contiguous())
        self.S0, self.S1, self.S2, self.H = stats[0], stats[1], stats[2], stats[3]

    def responsibilities(self, x):
        """xi [m, k] in float64 through torch ops, the reference's update_xi: for inspection at small m."""
        x0 = x[0].detach().to(torch.float64)
        arg = -self.beta[None, :] * ((x0[:, None] - self.mu[None, :]) ** 2) / 2 + self._logw()[None, :]
        return torch.softmax(arg, dim=1)

    def update_pi(self, x=None):
        self._stats()
        alpha_bar = self.alpha + self.S0
        self.pi = alpha_bar / torch.sum(alpha_bar, dim=0, keepdim=True)
        self.alpha_bar = alpha_bar

    def _move_mu(self, mu):
        d = mu - self.mu
        self.S2 = self.S2 - 2 * d * (self.S1 - self.mu * self.S0) + d * d * self.S0
        self.mu = mu

    def update_mu_ml(self, x=None):
        self._stats()
        self._move_mu(self.S1 / self.S0)

    def update_mu_map(self, x=None):
        self._stats()
        self._move_mu((self.beta_0 * self.mu_0 + self.S1) / (self.beta_0 + self.S0))

    def update_beta_map(self, x=None):
        self._stats()
        num = 2 * self.a - 1 + self.S0
        den = 2 * self.b + self.beta_0 * (self.mu - self.mu_0) ** 2 + self.S2
        self.beta = num / den

    def objective(self, x=None):
        self._stats()
        # Summation over data - i (xi of the LAST update_xi, the current beta)
        sum_i = (self.S0 * (torch.log(self.beta) - math.log(2 * math.pi)) - self.beta * self.S2) / 2 - self.H
        # Summation over components - j
        sum_j = torch.sum((self.a - 1 / 2) * torch.log(self.beta) - (self.beta_0 * self.beta * (self.mu - self.mu_0) ** 2) / 2
                          - self.b * self.beta + sum_i)
        # Log of the integral
        log_integral = torch.sum(torch.lgamma(self.alpha_bar)) - torch.lgamma(torch.sum(self.alpha_bar))
        return sum_j + log_integral

    def update(self, x):
        self.update_xi(x)
        self.update_pi(x)
        self.update_beta_map(x)
        return self.objective(x)


def fit_penalty(samples, weights=None, init_vars=INIT_VARS, n_iter=30):
    """The script's fit (train_penalty_em.py:291-303): n_iter updates of EM(k=len(init_vars)) on the samples.
    -> (pi, mu, beta, objectives [n_iter]), float64 on the samples' device; nothing is read back on the way."""
    em = EM(k=len(init_vars), init_vars=init_vars, device=samples.device)
    x = [samples.reshape(-1), None if weights is None else weights.reshape(-1)]
    obj = [em.update(x) for _ in range(int(n_iter))]
    return em.pi, em.mu, em.beta, torch.stack(obj)


# ---- full width at half maximum (train_penalty_em.py:63-84, 319-321) ------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def gaussian_mixture(x, pi, mu, beta):
    arg = -beta[None, :] * (x[:, None] - mu[None, :]) ** 2
    w = pi * np.sqrt(beta) / np.sqrt(2 * np.pi)
    return np.sum(w[None, :] * np.exp(arg / 2), axis=1)


def robust_l1_fwhm(eps=0.001):
    return 2 * np.sqrt((eps + np.log(2)) ** 2 - eps ** 2)


def abs_robust_loss_fwhm(eps=0.01, q=0.4):
    return 2 * (np.power(eps ** q + np.log(2), 1 / q) - eps)


def fwhm_scale(pi, mu, beta, reference_fwhm, lo=1e-6, hi=100.0):
    """The factor a for which the mixture (pi, mu, a beta) has the full width at half maximum `reference_fwhm`: the root of
    f(a) = p(fwhm / 2; a beta) - p(0; a beta) / 2 on the script's bracket [1e-6, 100], by bisection (host, float64) until the
    bracket no longer shrinks.  Raises where f does not change sign on the bracket, as scipy's root_scalar does."""
    pi, mu, beta = _np(pi), _np(mu), _np(beta)
    half = np.array([reference_fwhm / 2])

    def f(a):
        return float(gaussian_mixture(half, pi, mu, a * beta)[0] - gaussian_mixture(np.array([0.0]), pi, mu, a * beta)[0] / 2)
    flo, fhi = f(lo), f(hi)
    if flo == 0.0:
        return lo
    if fhi == 0.0:
        return hi
    if (flo > 0) == (fhi > 0):
        raise ValueError('fwhm_scale: f(a) has the same sign at both ends of [%g, %g]' % (lo, hi))
    while True:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            return mid
        fm = f(mid)
        if fm == 0.0:
            return mid
        if (fm > 0) == (flo > 0):
            lo, flo = mid, fm
        else:
            hi = mid


# ---- log-density of the fitted mixture (losses/uflow_elbo_loss.py:99-105) -------------------------------------------
class LogGmmFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, beta):
        dtype = _need_samples(x)
        xc = x.contiguous()
        out = torch.empty_like(xc)
        if xc.numel():
            with torch.cuda.device_of(xc):
                _call('arflow_log_gmm_fwd', _p(xc), xc.numel(), int(dtype == torch.float64), _p(w), _p(beta), w.numel(), _p(out),
                      _stream(), key=(xc.numel(), w.numel()))
        ctx.save_for_backward(xc, w, beta)
        return out

    @staticmethod
    def backward(ctx, gout):
        xc, w, beta = ctx.saved_tensors
        gout = gout.contiguous()
        gx = torch.empty_like(xc)
        if xc.numel():
            with torch.cuda.device_of(xc):
                _call('arflow_log_gmm_bwd', _p(xc), _p(gout), xc.numel(), int(xc.dtype == torch.float64), _p(w), _p(beta),
                      w.numel(), _p(gx), _stream(), key=(xc.numel(), w.numel()))
        return gx, None, None


def log_gmm(x, pi, beta):
    """log sum_j pi_j N(x; 0, 1 / beta_j) elementwise, any shape, k <= 16, float32 or float64 (computed in x's dtype), as one
    autograd node; the gradient is with respect to x only: -sum_j r_j beta_j x with r the posterior weights."""
    pi = torch.as_tensor(pi, dtype=torch.float64).to(x.device).reshape(-1)
    beta = torch.as_tensor(beta, dtype=torch.float64).to(x.device).reshape(-1).contiguous()
    if pi.numel() != beta.numel() or not 1 <= pi.numel() <= KMAX:
        raise ValueError('log_gmm expects pi and beta of one length k, 1 <= k <= %d' % KMAX)
    w = (pi * torch.sqrt(beta) / math.sqrt(2 * math.pi)).contiguous()
    return LogGmmFunction.apply(x, w, beta)


def penalty_cfg(pi, beta, scale=1.0):
    """A fitted mixture as the config entries UFlowElboLoss reads: {'pi': [...], 'beta': [scale * beta ...]} of Python floats
    (scale: what fwhm_scale returned).  Assign them to penalty_census_pi / penalty_census_beta (data_penalty ['gmm']) or
    penalty_smooth_pi / penalty_smooth_beta (penalty_smooth 'gmm')."""
    pi = [float(v) for v in torch.as_tensor(pi, dtype=torch.float64).reshape(-1).tolist()]
    beta = [float(scale) * float(v) for v in torch.as_tensor(beta, dtype=torch.float64).reshape(-1).tolist()]
    if len(pi) != len(beta) or not 1 <= len(pi) <= KMAX:
        raise ValueError('penalty_cfg expects pi and beta of one length k, 1 <= k <= %d' % KMAX)
    return {'pi': pi, 'beta': beta}


# ---- residual collection (losses/uflow_elbo_loss.py:18-96, train_penalty_em.py:235-289) -----------------------------
def data_loss_no_penalty(im1_0, im2_0, flow12_2, flow21_2, occ_type, data_loss, mean12_2=None, mean21_2=None):
    """losses/uflow_elbo_loss.py:18-78 for occ_type 'sample' / 'none' and data_loss == ['census']: the per-pixel census
    distance of im1_0 and the warped im2_0 before the penalty, and its normalised weight.  No gradient."""
    if occ_type not in ('sample', 'none'):
        raise NotImplementedError('Occlusion type {} not implemented!'.format(occ_type))
    for t in data_loss:
        if t != 'census':
            raise NotImplementedError('Data loss {} not implemented!'.format(t))
    flow12_0 = U.upsample(flow12_2.detach(), is_flow=True, scale_factor=4.0)
    im1_recons = U.resample_flow(im2_0.detach(), flow12_0)
    valid_mask_0 = U.mask_invalid_flow(flow12_0)
    occu_mask_2 = None
    if occ_type == 'sample':
        range_2 = U.compute_range_map(flow21_2.detach())
        occu_mask_2 = torch.clamp(range_2, min=0., max=1.)
        mask_0 = AF.up4_clamp_mul(range_2, valid_mask_0)  # upsample(clamp(range map, 0, 1), x4) * valid
    else:
        mask_0 = valid_mask_0
    pixel_loss, pixel_weight = [], []
    for _ in data_loss:
        l, w = U.census_loss_no_penalty(im1_0.detach(), im1_recons, mask_0)
        pixel_loss.append(l)
        pixel_weight.append(w)
    return pixel_loss, pixel_weight, occu_mask_2, valid_mask_0


def smooth_loss_no_penalty(im1_0, flow12_2, edge_constant, edge_asymp):
    """losses/uflow_elbo_loss.py:81-96: the flow differences at level 2 and their edge weights (halved)."""
    im1_2 = U.downsample(im1_0.detach(), is_flow=False, scale_factor=4.0)
    im1_gx, im1_gy = U.image_grads(im1_2)
    weights1_x = edge_asymp + (1.0 - edge_asymp) * torch.exp(-torch.mean(torch.abs(edge_constant * im1_gx), 1, keepdim=True))
    weights1_y = edge_asymp + (1.0 - edge_asymp) * torch.exp(-torch.mean(torch.abs(edge_constant * im1_gy), 1, keepdim=True))
    flow12_x, flow12_y = U.image_grads(flow12_2)
    return flow12_x, weights1_x / 2., flow12_y, weights1_y / 2.


def collect_samples(loss_list, weight_list, subsample, rand=None):
    """The script's subsampling loop (train_penalty_em.py:279-289) -> x [2, m]: every weight map is divided by its maximum; an
    entry is kept where the weight exceeds 1e-6 and its uniform draw exceeds `subsample`; x[1] is 1 (the script drops the
    weights).  rand: one tensor per entry, of the weight's shape (default: torch.rand_like), so that a test is deterministic."""
    data_list = []
    for i, (loss, weight) in enumerate(zip(loss_list, weight_list)):
        weight = weight / torch.max(weight)
        draw = torch.rand_like(weight) if rand is None else rand[i].to(weight.device)
        binary_mask = (weight > 1e-6) * (draw > subsample)
        x0 = torch.masked_select(loss, binary_mask)
        data_list.append(torch.stack([x0, torch.ones_like(x0)]))
    return torch.cat(data_list, dim=-1)
