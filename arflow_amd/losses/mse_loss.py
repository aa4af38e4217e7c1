"""MseLoss (the supervised objective of the probabilistic models) on the gfx950 kernels -- the constructor keys, inputs and
4-tuple result of losses/mse_loss.py:9-148, without its two .cuda() lines and its .item() NaN prints.

output[2] = net [B,C,h,w]: mean 0:2, log_diag 2:4, and with diag = false left = net[:, 4:6, :, :-1], over = net[:, 6:8, :-1, :].
target [B,2,H,W] is the ground-truth flow at any size; gt = resize_flow(target, (h, w), align_corners) (a missing
cfg.align_corners reads as False, resize_flow's default).  n_samples reparameterised samples z (sample s of item b at index
s B + b of eps [S B,2,h,w]) give
    loss_mse     = w_mse mean((z - gt)^2)
    loss_entropy = +- w_entropy mean_{b,y,x} sum_c log_diag      (+ for a covariance, - for inv_cov; always log_diag, also under
                   diag_dominant), or with diag = false, inv_cov and approx_entropy (:127-130, n_samples == 1 only)
                   w_entropy mean sum_c (J^T (z - mean.detach()))^2 / 2 on the detached coefficients
    loss_offdiag = 0 (the integer) with diag, else offdiag_reg (mean(left^2) + mean(over^2)) / 2
    total        = loss_mse - loss_entropy + loss_offdiag
The diagonal modes are ONE C-ABI call forward and one backward (arflow_amd/mse.py: the samples stay in registers).  The
4-neighbour modes add the sampler: mean + J eps through the differentiable matrix_vector_product of triag_solve.py, or
reparam_triag_inv (BackwardSubst) for inv_cov, both with D = None -- the reference's text names these operators with four
arguments but leaves their import commented out (:5); the fused call then reads the samples.  The terms that come from the
fused sums are float64 scalars (the sums are accumulated in float64 and are not rounded back).  No host sync anywhere."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import mse as M
from ..triag_solve import matrix_vector_product, matrix_vector_product_T, reparam_triag_inv


class MseLoss(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self._coef = {}
        self._mode()

    def _mode(self):
        """-> (diag, inv_cov, n_samples, approx_entropy) of the config as it stands.  A config that does not select one of the
        modes built here raises NotImplementedError naming the key or the setting, at construction as UFlowElboLoss does (the
        reference constructs anything and fails with an AttributeError inside the first step), and again in forward, since the
        config is read on every call."""
        cfg = self.cfg
        missing = [k for k in ('w_mse', 'w_entropy', 'diag', 'inv_cov', 'n_samples') if k not in cfg]
        if not missing and not cfg.diag:
            missing = [k for k in ('diag_dominant', 'approx_entropy', 'offdiag_reg') if k not in cfg]
        if missing:
            raise NotImplementedError('MseLoss: the config does not set %s (the keys of configs/chairs_uflow_mse.json:8-16 select '
                                      'the mode; there is no default one)' % ', '.join(missing))
        diag, inv, S = bool(cfg.diag), bool(cfg.inv_cov), cfg.n_samples
        if isinstance(S, bool) or not isinstance(S, (int, float)) or int(S) != S or S < 1:
            raise NotImplementedError('n_samples: %r (supported: an integer >= 1)' % (S,))
        approx = (not diag) and inv and bool(cfg.approx_entropy)
        if approx and S != 1:
            raise NotImplementedError('approx_entropy with n_samples = %d: the reference expression (losses/mse_loss.py:127-130) '
                                      'is shape-consistent for n_samples == 1 only' % S)
        return diag, inv, int(S), approx

    def _coefs(self, B, S, h, w, device, approx):
        """float64 [2,4]: row 0 is what the four sums are multiplied by to give (loss_mse, loss_entropy, the left and the over
        half of loss_offdiag); row 1 their signed weights in the total (mse - entropy + offdiag; the entropy's is 0 with
        approx_entropy, whose entropy term is not a sum of log_diag)."""
        cfg = self.cfg
        diag, inv = bool(cfg.diag), bool(cfg.inv_cov)
        reg = 0.0 if diag else float(cfg.offdiag_reg)
        # cfg is read on every call, as the reference reads it: a changed weight makes a new entry
        key = (B, S, h, w, device, float(cfg.w_mse), float(cfg.w_entropy), inv, reg, approx)
        if key not in self._coef:
            ent = float(cfg.w_entropy) / float(B * h * w)
            row = [float(cfg.w_mse) / float(S * B * 2 * h * w), -ent if inv else ent,
                   reg / 2.0 / float(B * 2 * h * max(w - 1, 1)), reg / 2.0 / float(B * 2 * max(h - 1, 1) * w)]
            signed = [row[0], 0.0 if approx else -row[1], row[2], row[3]]
            self._coef[key] = torch.tensor([row, signed], dtype=torch.float64, device=device)
        return self._coef[key]

    def forward(self, output, target, eps=None):
        """output: the model's list of outputs (only output[2] is read); target [B,2,H,W]; eps [n_samples B,2,h,w] ~ N(0,1),
        drawn on the device when not given -> (total, loss_mse, loss_entropy, loss_offdiag)."""
        cfg = self.cfg
        net = output[2]
        diag, inv, S, approx = self._mode()
        align = bool(cfg.align_corners) if 'align_corners' in cfg else False
        if not isinstance(net, torch.Tensor) or net.dim() != 4 or min(net.shape) < 1:
            raise ValueError('output[2] must be a non-empty [B,C,h,w] tensor (got %s)' % (tuple(getattr(net, 'shape', ())),))
        B, C, h, w = (int(v) for v in net.shape)
        if diag and C < 4:
            raise ValueError('output[2] must have at least 4 channels with diag: mean and log_diag (got %s)' % (tuple(net.shape),))
        if not diag and (C < 8 or h < 2 or w < 2):
            raise ValueError('output[2] must be [B,>=8,>=2,>=2] without diag: mean, log_diag, left, over (got %s)'
                             % (tuple(net.shape),))
        if not isinstance(target, torch.Tensor) or target.dim() != 4 or target.shape[0] != B or target.shape[1] != 2 \
                or min(target.shape) < 1:
            raise ValueError('target must be [%d,2,H,W] for output[2] %s (got %s)'
                             % (B, tuple(net.shape), tuple(getattr(target, 'shape', ()))))
        if eps is None:
            eps = torch.randn(S * B, 2, h, w, device=net.device, dtype=torch.float32)
        elif not isinstance(eps, torch.Tensor) or tuple(eps.shape) != (S * B, 2, h, w):
            raise ValueError('eps must be [%d,2,%d,%d]: n_samples * B samples (got %s)'
                             % (S * B, h, w, tuple(getattr(eps, 'shape', ()))))
        target = target.detach()
        coef = self._coefs(B, S, h, w, net.device, approx)
        # total = mse - entropy + offdiag as ONE weighted sum of the four sums (a mul and a sum, whose backward is one mul)
        # instead of selects, a sub and an add, whose backward scatters each select into a zero-filled vector
        if diag:
            terms = M.mse_sums(net, target, eps, S, M.MODE_INV if inv else M.MODE_COV, align) * coef
            return terms[1].sum(), terms[0, 0], terms[0, 1], 0
        mean, log_diag = net[:, 0:2], net[:, 2:4]
        left, over = net[:, 4:6, :, :-1], net[:, 6:8, :-1, :]
        d = torch.exp(log_diag)
        if cfg.diag_dominant:  # :81-85
            d = d + F.pad(torch.abs(left), (1, 0)) + F.pad(torch.abs(over), (0, 0, 1, 0))
        if inv:
            z = reparam_triag_inv(mean, d, left, over, None, nsamples=S, eps=eps)
        else:
            rep = lambda t: t.repeat(S, 1, 1, 1)  # noqa: E731
            z = rep(mean) + matrix_vector_product(rep(d), rep(left), rep(over), None, eps)
        terms = M.mse_sums(net, target, z, S, M.MODE_GIVEN, align) * coef
        total, loss_mse, loss_offdiag = terms[1].sum(), terms[0, 0], terms[0, 2] + terms[0, 3]
        if approx:
            tmp = matrix_vector_product_T(d.detach(), left.detach(), over.detach(), None, z - mean.detach())
            loss_entropy = float(cfg.w_entropy) * torch.sum(tmp * tmp / 2, dim=1).mean()
            total = total - loss_entropy
        else:
            loss_entropy = terms[0, 1]
        return total, loss_mse, loss_entropy, loss_offdiag
