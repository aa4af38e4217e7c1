"""Shared by tests/test_elbo_penalty_cpu.py, tests/test_elbo_penalty_gpu.py and tools/make_elbo_penalty_golden.py: float64
restatements, in plain torch on the CPU, of the selectable penalties of UFlowElboLoss (csrc/penalty_dev.hpp, DESIGN.md section
45), of the penalised census reduction (on tests/census_ref.py, imported, with a validity flow), of the penalised smoothness
sums and gradients, and of the loss with occ_type 'mean' -- together with the error bounds the GPU tests hold the kernels to
and the seeded inputs of tests/golden/elbo_penalty.npz.

    kind          rho(x)                                   rho'(x)
    IDENTITY      x                                        1
    CHARBONNIER   sqrt(x + 1e-6)                           1 / (2 sqrt(x + 1e-6))
    ABS_ROBUST    (|x| + 0.01)^0.4                         0.4 (|x| + 0.01)^-0.6 sign(x)
    GMM           -log sum_j w_j exp(-beta_j x^2 / 2)      (sum_j r_j beta_j) x        r = posterior weights
    GMM_SQ        -log sum_j w_j exp(-beta_j x / 2)        (sum_j r_j beta_j) / 2
    w_j = pi_j sqrt(beta_j) / sqrt(2 pi), formed in float64 and rounded to fp32 once, like beta_j: the restatement takes the
    ROUNDED values, so that rounding is not an error of the kernel.

Bounds, u = 2^-24, for an argument x with absolute error dx (the census distance's own bound census_ref.ham_bound, or the
rounding of a squared flow difference).  What the kernels use: IEEE addition, product, division and sqrtf (correctly rounded:
u relative each), expf and logf of the device library -- NOT the v_exp_f32 / v_log_f32 approximations -- taken at 2u relative
(their documented 1 ulp), and for ABS_ROBUST exp2f / __log2f exactly as ham_loss_terms (census_ref.pow_rel).
  IDENTITY      d rho = dx, d rho' = 0
  CHARBONNIER   y = x + 1e-6, dy = dx + u y; d rho = rho (dy / (2 y) + u); d rho' = rho' (dy / (2 y) + 2u)
  ABS_ROBUST    census_ref.pow_rel(|x| + 0.01, q, dx) + 3u, relative, q = 0.4 and -0.6
  GMM, GMM_SQ   q = x^2 (dq = 2 |x| dx + dx^2 + u q) or q = x (dq = dx); arg_j = -beta_j q / 2 is off by
                beta_j dq / 2 + 2u |arg_j| (two roundings), a_j = arg_j - c by u |a_j| more; expf and the product with w_j act
                like 3u on the argument.  -log sum w_j exp(arg_j) does not depend on the shift c and is 1-Lipschitz in the
                largest argument error E = max_j (.), so
                    d rho  = E + (k + 2) u + 2u |log den| + u (|c| + |rho|)     (k-term sum of positive terms, logf, the sum c + log)
                and with bbar = sum_j r_j beta_j, d bbar / d arg_j = r_j (beta_j - bbar):
                    d bbar = E sum_j r_j |beta_j - bbar| + bbar (2 k + 8) u      (two k-term sums, the products, the division)
                    d rho' = |x| d bbar + bbar dx + u |rho'|  (GMM)      d bbar / 2 + u |rho'|  (GMM_SQ)
  Every figure is first order in u and dx; like census_ref the bounds are taken TWICE (SAFETY) for what that drops.
"""
import math
import types

import numpy as np
import torch

from tests import census_ref as C
from tests import elbo_ref as R
from tests.loss_kernels_ref import _nar, _scatter, _scatter_max

U, D, SAFETY = C.U, C.D, C.SAFETY
IDENTITY, CHARBONNIER, ABS_ROBUST, GMM, GMM_SQ = range(5)
KINDS = {'identity': IDENTITY, 'charbonnier': CHARBONNIER, 'abs_robust_loss': ABS_ROBUST}
CENSUS_KINDS = (IDENTITY, CHARBONNIER, ABS_ROBUST, GMM)
SMOOTH_KINDS = (IDENTITY, CHARBONNIER, ABS_ROBUST, GMM_SQ)

# the ten-component mixtures of the reference's configs/chairs_uflow_elbo_gmm.json (data: recorded results of its EM script)
SMOOTH_PI = [0.6142385, 0.18683255, 0.08458639, 0.04736304, 0.034026437, 0.015653124, 0.012009228, 0.0030902755,
             0.0015197212, 0.0006806806]
SMOOTH_BETA = [3.1092725, 0.06315372, 0.009403812, 0.003426427, 0.0025579904, 0.0007372764, 0.00044421712, 0.0003139402,
               4.7309068e-06, 3.0201633e-07]
CENSUS_PI = [0.067531064, 0.00531184, 0.0020924346, 0.0002076141, 3.0250165e-05, 0.0025382563, 0.0066334084, 0.040437143,
             0.07933466, 0.79588336]
CENSUS_BETA = [3.2448268, 0.02025179, 0.010151853, 0.0020836794, 1.637905e-05, 5.2829646e-06, 4.249092e-06, 2.1278456e-06,
               1.2758659e-06, 1.7127788e-07]


# ======================================================================================================================
# the penalties
# ======================================================================================================================
def mixture(pi, beta, mutate=None, fp32=True):
    """(w, beta) float64 tensors of a mixture; fp32: rounded to fp32 once, as the descriptor holds them.
    mutate='weights_without_sqrt_beta' (WRONG on purpose): w = pi / sqrt(2 pi)."""
    pi, beta = torch.tensor(pi, dtype=D), torch.tensor(beta, dtype=D)
    w = pi / math.sqrt(2 * math.pi) if mutate == 'weights_without_sqrt_beta' else pi * torch.sqrt(beta) / math.sqrt(2 * math.pi)
    if fp32:
        w, beta = w.float().to(D), beta.float().to(D)
    return w, beta


def _mix(x, P, sq):
    w, beta = P
    q = x if sq else x * x
    arg = -beta * q.unsqueeze(-1) / 2
    c = arg.max(-1).values
    t = w * torch.exp(arg - c.unsqueeze(-1))
    den = t.sum(-1)
    r = t / den.unsqueeze(-1)
    bbar = (r * beta).sum(-1)
    return types.SimpleNamespace(q=q, arg=arg, c=c, den=den, r=r, bbar=bbar, rho=-(c + torch.log(den)))


def rho(kind, x, P=None):
    """-> (rho(x), rho'(x)), float64, elementwise"""
    x = x.to(D)
    if kind == IDENTITY:
        return x, torch.ones_like(x)
    if kind == CHARBONNIER:
        r = torch.sqrt(x + 1e-6)
        return r, 0.5 / r
    if kind == ABS_ROBUST:
        y = x.abs() + 0.01
        return y ** 0.4, 0.4 * y ** -0.6 * torch.where(x < 0, -torch.ones_like(x), torch.ones_like(x))
    m = _mix(x, P, kind == GMM_SQ)
    return m.rho, (m.bbar / 2 if kind == GMM_SQ else m.bbar * x)


def rho_bound(kind, x, dx, P=None):
    """-> (bound of rho, bound of rho'), absolute, for an argument with absolute error dx (see the module docstring)"""
    x = x.to(D)
    dx = torch.as_tensor(dx, dtype=D).expand_as(x)
    r, d = rho(kind, x, P)
    if kind == IDENTITY:
        return SAFETY * dx, torch.zeros_like(x)
    if kind == CHARBONNIER:
        y = x + 1e-6
        rel = (dx + U * y) / (2 * y)
        return SAFETY * r * (rel + U), SAFETY * d * (rel + 2 * U)
    if kind == ABS_ROBUST:
        y = x.abs() + 0.01
        return (SAFETY * r * (C.pow_rel(y, 0.4, dx) + 3 * U), SAFETY * d.abs() * (C.pow_rel(y, -0.6, dx) + 3 * U))
    sq = kind == GMM_SQ
    m = _mix(x, P, sq)
    w, beta = P
    k = beta.numel()
    dq = dx if sq else 2 * x.abs() * dx + dx * dx + U * m.q
    a = m.arg - m.c.unsqueeze(-1)
    E = (beta * dq.unsqueeze(-1) / 2 + 2 * U * m.arg.abs() + U * a.abs()).max(-1).values + 3 * U
    drho = E + (k + 2) * U + 2 * U * torch.log(m.den).abs() + U * (m.c.abs() + m.rho.abs())
    dbbar = E * (m.r * (beta - m.bbar.unsqueeze(-1)).abs()).sum(-1) + m.bbar * (2 * k + 8) * U
    dd = dbbar / 2 + U * d.abs() if sq else x.abs() * dbbar + m.bbar * dx + U * d.abs()
    return SAFETY * drho, SAFETY * dd


# ======================================================================================================================
# the penalised census reduction
# ======================================================================================================================
def reduce_pen(core, mask, mask_err, R_, kind, P=None, fold_fp32=False):
    """census_ref.reduce_ref under penalty `kind`: adds pm, dham, dham_bound, terms, sums, sums_bound, loss, loss_bound to the
    namespace of census_core.  ABS_ROBUST is reduce_ref itself."""
    if kind == ABS_ROBUST:
        return C.reduce_ref(core, mask, mask_err, R_, None, fold_fp32)
    B, _, H, W = core.ham.shape
    inn = C.interior(B, H, W, R_)
    mask = mask.to(D)
    mask_err = torch.as_tensor(mask_err, dtype=D).expand_as(mask)
    pm = torch.where(inn, mask, torch.zeros_like(mask))
    pme = torch.where(inn, mask_err, torch.zeros_like(mask))
    r, d = rho(kind, core.ham, P)
    dr, dd = rho_bound(kind, core.ham, core.ham_bound, P)
    core.pm = pm
    core.dham = pm * d
    core.dham_bound = pm * (dd + U * d.abs()) + pme * d.abs()
    core.terms = r * pm
    tb = pm * (dr + U * r.abs()) + pme * r.abs()
    depth = (128 if fold_fp32 else 64) * U
    core.sums = torch.stack([core.terms.sum(), pm.sum()])
    core.sums_bound = torch.stack([tb.sum() + depth * core.terms.abs().sum(), pme.sum() + depth * pm.sum()])
    den = core.sums[1] + 1e-6
    core.loss = core.sums[0] / den
    core.loss_bound = (core.sums_bound[0] + core.loss.abs() * core.sums_bound[1]) / den + 4 * U * core.loss.abs()
    return core


def fused_pen_ref(ga32, gb32, flow32, occ, R_, kind, P=None, valid_flow32=None, fold_fp32=False):
    """arflow_census_warp_pen_fwd: census_ref.fused_ref's forward with the penalty and, when given, mask_invalid taken of
    valid_flow32 while the warp samples at flow32.  -> namespace with ham, ham_bound, mask, mask_bound, reduce_pen's fields."""
    wp = C.warp_ref(gb32, flow32)
    valid = wp.valid if valid_flow32 is None else C.warp_ref(gb32, valid_flow32).valid
    if occ is None:
        mask, merr = valid, 0.0
    else:
        mask, merr = C.up4_clamp_mul_ref(occ, valid), 8 * U * valid
    core = C.census_core(ga32.to(D), wp.warped, R_, 0.0, wp.err)
    reduce_pen(core, mask, merr, R_, kind, P, fold_fp32)
    core.mask, core.mask_bound = mask, torch.as_tensor(merr, dtype=D).expand_as(mask)
    return core


def pair_pen_ref(gray2, flow2, occ2, R_, kind, P=None, valid_flow2=None, fold_fp32=False):
    """arflow_census_warp_pair_pen_fwd: sample s = 2 b + direction; image b and the range map are plane s ^ 1"""
    out = []
    for d in (0, 1):
        out.append(fused_pen_ref(C.pair_split(gray2, d), C.pair_split(gray2, d ^ 1), C.pair_split(flow2, d),
                                 None if occ2 is None else C.pair_split(occ2, d ^ 1), R_, kind, P,
                                 None if valid_flow2 is None else C.pair_split(valid_flow2, d), fold_fp32))
    return out


def standalone_pen_ref(im_a, im_b, mask, R_, kind, P=None, fold_fp32=False):
    """arflow_census_pen_fwd: census_ref.standalone_ref's distance, then the penalised reduction under the given mask"""
    core = C.standalone_ref(im_a, im_b, R_)
    return reduce_pen(core, mask, 0.0, R_, kind, P, fold_fp32)


# ======================================================================================================================
# the penalised smoothness
# ======================================================================================================================
def smooth_pen_ref(flow, img, flow_scale, alpha, order, wmode, kind, P=None, coef=(0.7, -1.3)):
    """arflow_smooth_pen_fwd / _bwd: loss_kernels_ref.smooth_ref's differences and edge weights with rho(v^2) as the penalty,
    d rho / d v = 2 v rho'(v^2).  -> namespace sums [2], sums_bound [2], grad [B,2,H,W], grad_bound, g_abs.
    Bounds: a weight exp(-alpha s) is off by (alpha s + 1) 2u relative (loss_kernels_ref.term_rel without the penalty's share);
    v by dv = 4u flow_scale sum_k |st_k| |f_k| (the fp32 differences), x = v^2 by 2 |v| dv + u x; rho and rho' by rho_bound;
    the sum of the two channels, the product with the weight and the k-term chains add the 64u / 16u of smooth_sum_bound /
    smooth_grad_bound."""
    f, im = flow.to(D), img.to(D)
    B, _, H, W = f.shape
    Ci = im.shape[1]
    o = int(order)
    st = (-1.0, 1.0) if o == 1 else (1.0, -2.0, 1.0)
    absst = tuple(abs(c) for c in st)
    fs = float(flow_scale)
    out = types.SimpleNamespace(sums=torch.zeros(2, dtype=D), sums_bound=torch.zeros(2, dtype=D), grad=torch.zeros_like(f),
                                grad_bound=torch.zeros_like(f), g_abs=torch.zeros_like(f))
    rmax = torch.zeros(B, 1, H, W, dtype=D)
    for i, axis in enumerate((3, 2)):
        n = f.shape[axis]
        m = n - o
        d = sum(c * _nar(f, axis, k, m) for k, c in enumerate(st)) if o == 1 else \
            (_nar(f, axis, 2, m) - _nar(f, axis, 1, m)) - (_nar(f, axis, 1, m) - _nar(f, axis, 0, m))
        lo = 0 if (o == 1 or wmode == 1) else 1
        s = (_nar(im, axis, o, m) - _nar(im, axis, lo, m)).abs().sum(1, keepdim=True) / Ci
        expo = float(alpha) * s
        w = torch.exp(-expo)
        wrel = (expo + 1.0) * 2 * U
        v = d * fs
        dv = 4 * U * fs * sum(c * _nar(f, axis, k, m).abs() for k, c in enumerate(absst))
        x = v * v
        dx = 2 * v.abs() * dv + U * x
        r, dr_ = rho(kind, x, P)
        rb, db = rho_bound(kind, x, dx, P)
        t = w * r
        out.sums[i] = t.sum()
        out.sums_bound[i] = (w * rb + t.abs() * (wrel + 4 * U)).sum() + 64 * U * t.abs().sum()
        lin = coef[i] * fs * w
        dpen = 2 * v * dr_
        out.grad += _scatter(lin * dpen, st, axis, n)
        out.g_abs += _scatter(lin.abs() * dpen.abs(), absst, axis, n)
        out.grad_bound += _scatter(lin.abs() * (2 * v.abs() * db + 2 * dv * dr_.abs()), absst, axis, n)
        rmax = torch.maximum(rmax, _scatter_max(expo, o, axis, n, 0.0))
    out.grad_bound = out.grad_bound + out.g_abs * ((rmax + 4.0) * 2 * U + 16 * U)
    return out


# ======================================================================================================================
# the loss: cases of tests/golden/elbo_penalty.npz and its restatement
# ======================================================================================================================
GMM_KEYS = dict(penalty_census_pi=CENSUS_PI, penalty_census_beta=CENSUS_BETA, penalty_smooth_pi=SMOOTH_PI,
                penalty_smooth_beta=SMOOTH_BETA)
# 'inputs': 'spread' = the structured image pair and flows (the census distances spread over the mixture's components),
# 'noise' = the recipe of tests/elbo_ref.py (smoothness cases; edge_asymp 0.5: on noise images the edge weights vanish)
CASES = {
    'mean': dict(cfg=dict(occ_type='mean', n_samples=2), inputs='spread', log_std=-1.0),
    'mean_occ': dict(cfg=dict(occ_type='mean', n_samples=2, w_occ=0.3), inputs='spread', log_std=-1.0),
    'data_identity': dict(cfg=dict(data_penalty=['identity']), inputs='spread', log_std=-4.5),
    'data_charbonnier': dict(cfg=dict(data_penalty=['charbonnier']), inputs='spread', log_std=-4.5),
    'smooth_identity': dict(cfg=dict(penalty_smooth='identity', edge_asymp=0.5), inputs='noise'),
    'smooth_abs_robust': dict(cfg=dict(penalty_smooth='abs_robust_loss', edge_asymp=0.5), inputs='noise'),
    'gmm_data': dict(cfg=dict(data_penalty=['gmm']), inputs='spread', log_std=-4.5),
    'gmm_smooth': dict(cfg=dict(penalty_smooth='gmm', n_samples=2, edge_asymp=0.5), inputs='noise'),
    'gmm_closed1': dict(cfg=dict(penalty_smooth='gmm', closed_form_smooth=True, order_smooth=1, edge_asymp=0.5), inputs='noise'),
    'gmm_closed2_iso': dict(cfg=dict(penalty_smooth='gmm', closed_form_smooth=True, order_smooth=2, isotropic_smooth=True,
                                     edge_asymp=0.5), inputs='noise'),
    'gmm_all_mean_sparse': dict(cfg=dict(approx='sparse', cov_supp=1, data_penalty=['gmm'], penalty_smooth='gmm',
                                         occ_type='mean', n_samples=2, edge_asymp=0.5, offdiag_reg=0.01),
                                inputs='spread', log_std=-4.5),
}
DATA_CASES = ('data_identity', 'data_charbonnier', 'gmm_data', 'gmm_all_mean_sparse')  # the tool asserts their spread
OUTPUTS = R.OUTPUTS
MUTATIONS = {  # mutation -> the case it must leave the bounds of
    'gmm_sq_on_distance': 'gmm_data', 'gmm_on_squared_difference': 'gmm_smooth', 'weights_without_sqrt_beta': 'gmm_data',
    'mean_validity_from_sample': 'mean', 'mean_range_map_from_sample': 'mean', 'charbonnier_on_h_squared': 'data_charbonnier'}


def case_cfg(tag):
    return R.Cfg(dict(R.BASE, **GMM_KEYS, **CASES[tag]['cfg']))


def spread_images(seed=47):
    """The image pair of the 'spread' cases [B,3,H,W]: a smooth pattern (a few sinusoids per channel) plus a little noise;
    the second image is the first displaced by (4, 2) pixels -- the mean flow of the cases -- so that the census distance is
    near 0 where the flow is right and large where it is not."""
    B, H, W = R.LOSS_B, R.LOSS_H, R.LOSS_W
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(-8, H + 8, dtype=np.float64), np.arange(-8, W + 8, dtype=np.float64), indexing='ij')
    big = np.zeros((B, 3, H + 16, W + 16))
    for b in range(B):
        for c in range(3):
            for _ in range(4):
                fy, fx, ph = rng.uniform(0.05, 0.25), rng.uniform(0.05, 0.25), rng.uniform(0, 2 * np.pi)
                big[b, c] += 0.11 * np.sin(fy * ys + fx * xs + ph)
    big = 0.5 + big
    im1 = big[:, :, 8:8 + H, 8:8 + W] + 0.0005 * rng.standard_normal((B, 3, H, W))
    im2 = big[:, :, 8 - 2:8 - 2 + H, 8 - 4:8 - 4 + W] + 0.0005 * rng.standard_normal((B, 3, H, W))  # im2(p + (4, 2)) = im1(p)
    return np.clip(im1, 0, 1), np.clip(im2, 0, 1)


def make_case(tag, seed=59):
    """-> dict of float32 arrays net12, net21, im1, im2, eps12, eps21 (the layout of elbo_ref.make_loss_case).
    'noise' cases: elbo_ref's recipe for 'diag'.  'spread' cases: mean flow (1, 0.5) at level 2 = (4, 2) pixels forward and its
    negative backward, + 0.005 N(0,1), and + 0.6 N(0,1) on the right half (wrong flow: large distances there); log_std from the
    case; off-diagonals 0.005 N(0,1)."""
    spec = CASES[tag]
    cfg = case_cfg(tag)
    B, H, W = R.LOSS_B, R.LOSS_H, R.LOSS_W
    h, w = H // 4, W // 4
    k = cfg.cov_supp if cfg.approx == 'sparse' else 0
    n = (k + 1) ** 2 - 1
    rng = np.random.default_rng([seed, sorted(CASES).index(tag)])
    out = {}
    if spec['inputs'] == 'noise':
        base = R.make_loss_case('diag')
        out['im1'], out['im2'] = base['im1'], base['im2']
        for name in ('net12', 'net21'):
            out[name] = np.concatenate((1.5 * rng.standard_normal((B, 2, h, w)), -1 + 0.3 * rng.standard_normal((B, 2, h, w))), 1)
    else:
        out['im1'], out['im2'] = spread_images()
        for name, sign in (('net12', 1.0), ('net21', -1.0)):
            mean = sign * np.array([1.0, 0.5]).reshape(1, 2, 1, 1) + 0.005 * rng.standard_normal((B, 2, h, w))
            mean[..., w // 2:] += 0.6 * rng.standard_normal((B, 2, h, w - w // 2))
            out[name] = np.concatenate((mean, spec['log_std'] + 0.3 * rng.standard_normal((B, 2, h, w)),
                                        0.005 * rng.standard_normal((B, 2 * n, h, w))), 1)
    for name in ('eps12', 'eps21'):
        out[name] = rng.standard_normal((cfg.n_samples * B, 2, h, w))
    return {key: np.ascontiguousarray(v, dtype=np.float32) for key, v in out.items()}


def _penalty_fns(cfg, mutate):
    """(data penalty on the distance, smoothness penalty on the squared difference) as float64 callables"""
    def data(hm):
        name = cfg.data_penalty[0]
        if name == 'gmm':
            P = mixture(cfg.penalty_census_pi, cfg.penalty_census_beta, mutate, fp32=False)
            return rho(GMM_SQ if mutate == 'gmm_sq_on_distance' else GMM, hm, P)[0]
        if name == 'charbonnier' and mutate == 'charbonnier_on_h_squared':
            return torch.sqrt(hm * hm + 1e-6)
        return rho(KINDS[name], hm)[0]

    def smooth(x_sq):
        name = cfg.penalty_smooth
        if name == 'gmm':
            P = mixture(cfg.penalty_smooth_pi, cfg.penalty_smooth_beta, mutate, fp32=False)
            return rho(GMM if mutate == 'gmm_on_squared_difference' else GMM_SQ, x_sq, P)[0]
        return rho(KINDS[name], x_sq)[0]
    return data, smooth


def loss(cfg, case, dtype=torch.float64, mutate=None):
    """elbo_ref.loss with the selectable penalties and occ_type 'mean' (losses/uflow_elbo_loss.py:18-78, :383-533).
    -> dict of numpy arrays: OUTPUTS and 'occ'.  mutate: one of MUTATIONS (WRONG on purpose)."""
    from oracle import ops as O
    t = {key: torch.from_numpy(np.asarray(v)).to(dtype) for key, v in case.items()}
    net12, net21 = t['net12'].requires_grad_(True), t['net21'].requires_grad_(True)
    S, B = cfg.n_samples, net12.shape[0]
    k = cfg.cov_supp if cfg.approx == 'sparse' else 0
    n = (k + 1) ** 2 - 1
    rep = lambda x: x.repeat(S, 1, 1, 1)  # noqa: E731
    pen_data, pen_smooth = _penalty_fns(cfg, mutate)

    def sample(net, eps):
        mean, log_diag, off = net[:, 0:2], net[:, 2:4], net[:, 4:4 + 2 * n]
        diag = torch.exp(log_diag)
        z = rep(mean) + R._product_t(rep(torch.cat((diag, off), 1)), eps, k)
        return z, mean, log_diag, diag, off

    f12, mean12, ld12, diag12, off12 = sample(net12, t['eps12'])
    f21, mean21, ld21, diag21, off21 = sample(net21, t['eps21'])
    im1, im2 = rep(t['im1']), rep(t['im2'])
    dirs = [(im1, im2, f12, f21, mean12, mean21, ld12, diag12, off12)]
    if cfg.with_bk:
        dirs.append((im2, im1, f21, f12, mean21, mean12, ld21, diag21, off21))
    mean_occ = cfg.occ_type == 'mean'

    warp = smooth = entropy = oof = occ = offdiag = 0.
    first = None
    for im_a, im_b, f_ab, f_ba, mean, mean_ba, ld, diag, off in dirs:
        coords = O.flow_to_warp(O.upsample(f_ab, True, 4.0))
        recons = O.resample(im_b.detach(), coords)
        if mean_occ:
            v_of = f_ab if mutate == 'mean_validity_from_sample' else rep(mean)
            r_of = f_ba if mutate == 'mean_range_map_from_sample' else rep(mean_ba)
        else:
            v_of, r_of = f_ab, f_ba
        valid = O.mask_invalid(O.flow_to_warp(O.upsample(v_of, True, 4.0)))
        occ_small = torch.clamp(O.compute_range_map(r_of), 0., 1.)
        mask = (O.upsample(occ_small, False, 4.0) * valid).detach()
        ham = O.soft_hamming(O.census_transform(im_a, 7), O.census_transform(recons, 7))
        pm = O.zero_mask_border(mask, 7)
        warp = warp + cfg.data_weight[0] * (pen_data(ham) * pm).sum() / (pm.sum() + 1e-6)
        if first is None:
            first = (occ_small, valid)
        entropy = entropy + cfg.w_entropy * ld.sum(1).mean()
        im_small = O.downsample(im_a[:B], False, 4.0)
        if not cfg.closed_form_smooth:
            wx, wy = R._edge_weights(cfg, rep(im_small), 1)
            dx, dy = O.image_grads(f_ab)
            smooth = smooth + (wx / 2 * cfg.w_smooth * pen_smooth(dx ** 2)).mean() \
                + (wy / 2 * cfg.w_smooth * pen_smooth(dy ** 2)).mean()
        else:
            if cfg.order_smooth == 1:
                wx, wy = (v / 2 for v in R._edge_weights(cfg, im_small, 1))
                Ex = (mean[..., 1:] - mean[..., :-1]) ** 2 + diag[..., 1:] ** 2 + diag[..., :-1] ** 2
                Ey = (mean[:, :, 1:] - mean[:, :, :-1]) ** 2 + diag[:, :, 1:] ** 2 + diag[:, :, :-1] ** 2
            else:
                wx, wy = R._edge_weights(cfg, im_small, 2)
                Ex = (mean[..., :-2] - 2 * mean[..., 1:-1] + mean[..., 2:]) ** 2 \
                    + diag[..., :-2] ** 2 + 4 * diag[..., 1:-1] ** 2 + diag[..., 2:] ** 2
                Ey = (mean[:, :, :-2] - 2 * mean[:, :, 1:-1] + mean[:, :, 2:]) ** 2 \
                    + diag[:, :, :-2] ** 2 + 4 * diag[:, :, 1:-1] ** 2 + diag[:, :, 2:] ** 2
            if cfg.isotropic_smooth:
                Ex, Ey = Ex.mean(1), Ey.mean(1)
            smooth = smooth + (wx * cfg.w_smooth * pen_smooth(Ex)).mean() + (wy * cfg.w_smooth * pen_smooth(Ey)).mean()
        if cfg.w_occ > 0:
            occ = occ + cfg.w_occ * (1 / (100.0 * occ_small + 1) * f_ab ** 2).mean()
        if cfg.approx == 'sparse':
            offdiag = offdiag + (off ** 2).mean()
    total = warp + smooth - entropy + oof + occ
    if cfg.approx == 'sparse':
        total = total + cfg.offdiag_reg * offdiag
    g12, g21 = torch.autograd.grad(total, (net12, net21))
    out = {'total': total, 'warp': warp, 'smooth': smooth, 'entropy': entropy, 'oof': oof, 'occ': occ, 'flow12_2': f12,
           'occu_mask12': first[0], 'valid_mask12': first[1], 'gnet12': g12, 'gnet21': g21}
    return {key: torch.as_tensor(v, dtype=dtype).detach().numpy() for key, v in out.items()}


# ---- the rule of tests/test_elbo_gpu.py ---------------------------------------------------------------------------------
KIND = {'total': 'term', 'warp': 'term', 'smooth': 'term', 'entropy': 'term', 'oof': 'term', 'flow12_2': 'term',
        'occu_mask12': 'mask', 'valid_mask12': 'mask', 'gnet12': 'grad', 'gnet21': 'grad'}


def project_bound(kind, ref):
    a = np.abs(ref)
    if kind == 'term':
        return 5e-8 + 3e-6 * a
    if kind == 'mask':
        return 2e-6 + 1e-5 * a
    return 2e-7 + 2e-4 * a.max() + 2e-3 * a


def golden_bound(g, key, tag):
    """8 x the stored fp32-versus-float64 gap of the reference times the output's largest magnitude, or the project bound,
    whichever is larger"""
    ref = g.raw('%s_%s' % (key, tag))
    return np.maximum(8 * float(g.raw('noise_%s_%s' % (key, tag))) * np.abs(ref).max(), project_bound(KIND[key], ref))
