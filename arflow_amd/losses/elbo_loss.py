"""ElboLoss (the ELBO form of ARFlow's pyramid loss) on the gfx950 kernels -- same constructor keys, inputs and 5-tuple result
as losses/elbo_loss.py:9-146, without its two .cuda() lines.

output[i] [B,8,h_i,w_i]: mean_fw 0:2, logvar_fw 2:4, mean_bw 4:6, logvar_bw 6:8.  Per scale with a non-zero w_scales entry the
reference draws one sample per direction (:90-91), runs unFlowLoss' L1 / SSIM + smoothness objective on the samples and takes
the entropy term sum_c logvar . mean() / 2 per direction (:117-128).  Here ONE reparam_pyramid call (arflow_amd/gauss_pyr.py:
one sampler launch for all scales and both directions, one adjoint launch) gives the [B,4,h,w] (forward, backward) samples --
directly the flow tensors unFlowLoss takes -- and the float64 sums of the log-variances; the samples then go through an
internal unFlowLoss(cfg): its fused stacked path with with_bk, its sequential path without.  w_ternary > 0 and
w_scales[0] == 0 therefore fail exactly as unFlowLoss does.

Reference quirk, reproduced as it stands: the skip branch of a scale with w_scales[i] == 0 (:74-77) appends zeros to the
warp and smoothness lists but NOTHING to pyramid_entropy, so the entropies of the COMPUTED scales are zipped with w_en_scales
FROM ITS START (:138-139): with w_scales [1, 0, 1] the entropy of scale 2 is weighted by w_en_scales[1], not [2]."""
import torch
import torch.nn as nn

from ..gauss_pyr import reparam_pyramid
from .flow_loss import unFlowLoss


class ElboLoss(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.flow_loss = unFlowLoss(cfg)
        self._coef = {}

    def _entropy_coef(self, sizes, B, device):
        """[n,2] float64: what each sum of log-variances is multiplied by (:117-128, :138-139, :143) -- 1 / (B h w) / 2 per
        direction, halved again and both directions with with_bk, times the k-th w_en_scales entry for the k-th computed
        scale (the quirk above: zip stops at the shorter list) and w_entropy."""
        cfg = self.cfg
        # cfg is read on every call, as the reference and unFlowLoss read it: a changed weight makes a new entry
        key = (tuple(sizes), B, device, tuple(float(v) for v in cfg.w_en_scales), float(cfg.w_entropy), bool(cfg.with_bk))
        if key not in self._coef:
            rows = []
            for k, (h, w) in enumerate(sizes):
                wk = float(cfg.w_en_scales[k]) if k < len(cfg.w_en_scales) else 0.
                c = wk / float(B * h * w) / 2.0
                rows.append([c / 2.0, c / 2.0] if cfg.with_bk else [c, 0.0])
            self._coef[key] = torch.tensor(rows, dtype=torch.float64, device=device) * float(cfg.w_entropy)
        return self._coef[key]

    def forward(self, output, target, eps=None):
        """output: n x [B,8,h,w]; target: image pairs [B,6,H,W]; eps: one [B,4,h,w] noise tensor per scale whose w_scales
        entry is non-zero (forward noise in channels 0:2, backward in 2:4), drawn on the device when not given
        -> (total, warp_loss, smooth_loss, entropy, output[0].abs().mean())."""
        cfg = self.cfg
        computed = [i for i in range(len(output)) if cfg.w_scales[i] != 0]
        nets = [output[i] for i in computed]
        for i, t in zip(computed, nets):
            if t.dim() != 4 or t.shape[1] != 8:
                raise ValueError('output[%d] must be [B,8,h,w]: (mean, log-variance) of both directions (got %s)'
                                 % (i, tuple(t.shape)))
        if eps is not None and len(eps) != len(nets):
            raise ValueError('eps must hold one tensor per scale with a non-zero w_scales entry: %d (got %d)'
                             % (len(nets), len(eps)))
        if not nets:  # every scale skipped: nothing to sample, and the reference's empty entropy list sums to 0 (:138-143)
            _, warp_loss, smooth_loss, _ = self.flow_loss([t[:, 0:4] for t in output], target)
            return warp_loss + smooth_loss - 0.0, warp_loss, smooth_loss, 0.0, output[0].abs().mean()
        samples, ent = reparam_pyramid(nets, eps)
        # a skipped scale is never read by unFlowLoss: a four-channel view keeps its place in the list
        flows = [t[:, 0:4] for t in output]
        for i, z in zip(computed, samples):
            flows[i] = z
        _, warp_loss, smooth_loss, _ = self.flow_loss(flows, target)
        self.pyramid_occu_mask1 = self.flow_loss.pyramid_occu_mask1
        self.pyramid_occu_mask2 = self.flow_loss.pyramid_occu_mask2
        B = nets[0].shape[0]
        coef = self._entropy_coef([tuple(t.shape[-2:]) for t in nets], B, ent.device)
        entropy = (ent * coef).sum().to(torch.float32)
        total_loss = warp_loss + smooth_loss - entropy  # :144: the maximum-entropy solution is sought
        return total_loss, warp_loss, smooth_loss, entropy, output[0].abs().mean()
