"""losses/penalty_functions.py: the penalty callables by name, plus the fitted Gaussian scale mixture of penalty_em
(DESIGN.md section 45).  `get_penalty(name)` is the reference's function; 'gmm' is what its chairs_uflow_elbo_gmm.json asks
for: x -> -log_gmm(x, pi, beta) for the data term and, with squared=True, x_sq -> -log sum_j w_j exp(-beta_j x_sq / 2) for the
smoothness term, which receives squared differences."""
import math

import torch

from ..penalty_em import KMAX, log_gmm


def abs_robust_loss(diff, eps=0.01, q=0.4):
    return torch.pow((torch.abs(diff) + eps), q)


def charbonnier(x_sq, eps=0.001):
    return torch.sqrt(x_sq + eps ** 2)


def charbonnier_prime(x_sq, eps=0.001):
    return 1 / (2 * torch.sqrt(x_sq + eps ** 2))


def identity(x):
    return x


def identity_prime(x):
    return torch.ones_like(x)


def check_mixture(pi, beta, what='gmm'):
    """The mixture lists of a config -> (pi, beta) as Python floats; ValueError for missing or unequal-length lists, more than
    KMAX entries, a non-positive or non-finite beta, a negative or non-finite pi, no weight on the widest component."""
    if pi is None or beta is None:
        raise ValueError('%s: the mixture needs both pi and beta' % what)
    pi, beta = [float(v) for v in pi], [float(v) for v in beta]
    if len(pi) != len(beta):
        raise ValueError('%s: pi has %d entries, beta %d' % (what, len(pi), len(beta)))
    if not 1 <= len(pi) <= KMAX:
        raise ValueError('%s: %d components (supported: 1..%d)' % (what, len(pi), KMAX))
    if any(not (math.isfinite(b) and b > 0.0) for b in beta):
        raise ValueError('%s: every beta must be finite and positive' % what)
    if any(not (math.isfinite(p) and p >= 0.0) for p in pi):
        raise ValueError('%s: every pi must be finite and non-negative' % what)
    if not max(p for p, b in zip(pi, beta) if b == min(beta)) > 0.0:  # (else the density underflows to 0 at large arguments)
        raise ValueError('%s: the component with the smallest beta must have a positive pi' % what)
    return pi, beta


class NegLogGmmSqFunction(torch.autograd.Function):
    """x_sq -> -log sum_j w_j exp(-beta_j x_sq / 2) as ONE autograd node, in the evaluation order of
    losses/uflow_elbo_loss.py:99-105.  Its gradient, (sum_j r_j beta_j) / 2 with r the posterior weights, is finite at
    x_sq = 0, where that of -log_gmm(sqrt(x_sq)) is 0 * inf.  Plain torch (any device, float32 or float64): it serves the
    closed-form smoothness, which is plain torch."""

    @staticmethod
    def forward(ctx, x_sq, w, beta):
        arg = -beta * x_sq.unsqueeze(-1) / 2
        c = torch.max(arg, dim=-1).values
        t = w * torch.exp(arg - c.unsqueeze(-1))
        den = torch.sum(t, dim=-1)
        ctx.save_for_backward(torch.sum(t * beta, dim=-1) / den / 2)
        return -(c + torch.log(den))

    @staticmethod
    def backward(ctx, gout):
        d, = ctx.saved_tensors
        return gout * d, None, None


def neg_log_gmm_sq(x_sq, pi, beta):
    pi = torch.as_tensor(pi, dtype=torch.float64).to(x_sq.device).reshape(-1)
    beta = torch.as_tensor(beta, dtype=torch.float64).to(x_sq.device).reshape(-1)
    w = (pi * torch.sqrt(beta) / math.sqrt(2 * math.pi)).to(x_sq.dtype)
    return NegLogGmmSqFunction.apply(x_sq, w, beta.to(x_sq.dtype))


def get_penalty(name, derivative=False, pi=None, beta=None, squared=False):
    if name == 'identity':
        return identity_prime if derivative else identity
    if name == 'charbonnier':
        return charbonnier_prime if derivative else charbonnier
    if name == 'abs_robust_loss':
        if derivative:
            raise NotImplementedError('derivative not implemented for abs_robust_loss penalty!')
        return abs_robust_loss
    if name == 'gmm':
        if derivative:
            raise NotImplementedError('derivative not implemented for gmm penalty!')
        pi, beta = check_mixture(pi, beta)
        if squared:
            return lambda x_sq: neg_log_gmm_sq(x_sq, pi, beta)
        return lambda x: -log_gmm(x, pi, beta)  # GPU only, like log_gmm
    raise NotImplementedError('penalty: %r (supported: identity, charbonnier, abs_robust_loss, gmm)' % (name,))
