"""PWCProbFlow (probabilistic UFlow port) host model on the gfx950 ops; contract of models/uflow_prob_model.py:149-517.
This is what configs/chairs_uflow_elbo*.json instantiate (``"model": {"type": "uflow_prob"}``): PWCFlow with wider heads.
Every level carries out_channels = [L, M, N] channels -- L = 2 flow channels (used for warping), M log-diagonal channels of
the covariance / precision factor, N further channels (the off-diagonal band) that only the output level produces -- and
brings them to the next level with upsample_out (:223-250): AF.out_upsample / AF.out_tail.
M = 0 is the low-rank family (out_channels [2, 0, 2 columns]): the pyramid then carries the flow pair
alone, and no zero-channel tensor is built or handed to a kernel.
ComponentNet (``"type": "component"``, :109-147) is the mixture family's model: two PWCProbFlow with
out_channels [2, 2, 0], one per mixture component, their outputs joined per level as (mean1, mean2, log_diag1, log_diag2)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as func

from .. import functional as AF
from .. import uflow_utils
from ..config import AttrDict
from . import blocks
# normalize_features, cost_volume_concat and uflow_utils.resample_flow are called as attributes of the uflow_model module
# (mum.*), never bound here: oracle.host_models.oracle_ops substitutes exactly those attributes, and blocks.bias_act, so a
# twin of this model runs on the oracle ops as it stands
from . import uflow_model as mum
from .blocks import init_conv_weights, level_drops, pair_pass
from .uflow_model import PWCFeaturePyramid, build_flow_layers, build_refinement_model, dense_level, refine


class PWCProbFlow(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        if cfg.n_pyramids != 1:
            raise NotImplementedError('PWCProbFlow: n_pyramids = %r (only 1: ComponentNet / mixtures are out of scope)'
                                      % (cfg.n_pyramids,))
        if cfg.mixture_weights:
            raise NotImplementedError('PWCProbFlow: mixture_weights = %r (MixtureWeightsNet is out of scope)'
                                      % (cfg.mixture_weights,))
        if len(cfg.out_channels) != 3 or cfg.out_channels[0] != 2:
            raise NotImplementedError('PWCProbFlow: out_channels = %r (one flow pair: out_channels[0] must be 2)'
                                      % (list(cfg.out_channels),))
        self._leaky_relu_alpha = 0.1
        self._drop_out_rate = cfg.level_dropout
        self._num_context_up_channels = 32
        self._num_levels = 5
        self._normalize_before_cost_volume = cfg.feature_norm
        self._out_channels = [int(c) for c in cfg.out_channels]
        self._inv_cov = bool(cfg.inv_cov)
        # added to the log-diagonal at every x2 upsample (:170): the standard deviation doubles with the resolution
        self._diag_bias = -math.log(2) if cfg.inv_cov else math.log(2)
        # registration order matters for state_dict order: refine, flow layers, upsample, pyramid(s)
        n01, nall = sum(self._out_channels[0:2]), sum(self._out_channels)
        self._refine_model = build_refinement_model(32 + nall, nall, self._leaky_relu_alpha)  # :479-502: all L + M + N channels
        # :440-477: every level's input has context_up and out_up (the top level too); the head emits L + M + N channels at
        # level 1 and L + M at levels 2..4
        self._flow_layers = build_flow_layers([81 + 32 + n01 + self._num_context_up_channels] * (self._num_levels - 1),
                                              [nall] + [n01] * (self._num_levels - 2), self._leaky_relu_alpha)
        self._context_up_layers = nn.ModuleList(
            [nn.ConvTranspose2d(32, 32, kernel_size=(4, 4), stride=2, padding=1) for _ in range(self._num_levels)])
        self._feature_pyramid_extractor = nn.ModuleList([PWCFeaturePyramid() for _ in range(cfg.n_pyramids)])

    def init_weights(self):
        init_conv_weights(self, 'kaiming')  # :209-221: kaiming-normal fan_in, zero biases

    def _drops(self, n_passes, batch_per_pass, device):
        """One multiplier per level 4..1, then one for the refinement."""
        return level_drops(self.training, self._drop_out_rate, self._num_levels, n_passes, batch_per_pass, device)

    def _native_up(self, x):
        """A twin that has swapped bias_act out keeps the composed ATen upsample: the convention of blocks.HeadConv.native."""
        return AF.out_up_supported(x) and blocks.bias_act is AF.bias_leaky_relu

    def upsample_out(self, out):
        """:223-250.  One launch on the GPU path, else the composed ATen path group by group."""
        n0, n1, _ = self._out_channels
        if self._native_up(out):
            return AF.out_upsample(out, n0, n1, self._diag_bias)
        ups = [uflow_utils.upsample(out[:, 0:n0], is_flow=True)]
        if n1 > 0:
            ups.append(uflow_utils.upsample(out[:, n0:n0 + n1] + self._diag_bias, is_flow=False))
        if out.size(1) > n0 + n1:
            ups.append(uflow_utils.upsample(out[:, n0 + n1:], is_flow=False))
        return torch.cat(ups, dim=1)

    def forward_2_frames(self, feature_pyramid1, feature_pyramid2, drops=None, moments=None):
        """:252-389.  moments: as PWCFlow.forward_2_frames."""
        n0, n1, n2 = self._out_channels
        n01 = n0 + n1
        alpha = self._leaky_relu_alpha
        norm = self._normalize_before_cost_volume
        context = out = context_up = None
        outs = []
        k = 0
        top = self._num_levels - 1
        for level in range(top, 0, -1):
            features1, features2 = feature_pyramid1[level], feature_pyramid2[level]
            B, _, H, W = features1.shape
            r1 = moments[0][level] if moments is not None else None
            if level == top:
                # :263-273: zero context_up, zero flow, and log_diag planes chosen so that the diag_bias of the upsamples
                # down to the output level leaves ~0 there.  The warp by the zero flow is the identity and is not run.
                start = features1.new_zeros(B, self._num_context_up_channels + n0, H, W)
                if n1 > 0:
                    start = torch.cat([start, features1.new_full((B, n1, H, W), -(self._num_levels - 3) * self._diag_bias)], 1)
                out_up = start[:, self._num_context_up_channels:]
                if norm and AF.level_supported(features1, None, True):
                    r2 = moments[1][level] if moments is not None else None
                    cfg = AF.LevelCfg([0, 'vol', 1], 'avg', alpha, 4)
                    x_in = AF.level(features1, features2, None, cfg, start, features1, x1_rows=r1, x2_rows=r2)
                else:
                    f1n, w2n = mum.normalize_features([features1, features2], normalize=norm, center=norm,
                                                      moments_across_channels=True, moments_across_images=True)
                    x_in = mum.cost_volume_concat(f1n, w2n, (start,), (features1,), max_displacement=4, negative_slope=alpha)
            elif norm and AF.level_supported(features1, out[:, 0:2], True):
                # the fused level upsamples and warps with the flow pair itself ('flow' slot); the other channels of
                # out_up come from the output-upsample kernel and travel as a member
                if n1 == 0:  # the flow pair is all that comes up the pyramid: no rest member
                    cfg = AF.LevelCfg([0, 'flow', 'vol', 1], 'avg', alpha, 4, True, False, 'zeros', True, AF.NORM_UFLOW)
                    x_in, out_up = AF.level(features1, features2, out[:, 0:2], cfg, context_up, features1, x1_rows=r1)
                else:
                    if self._native_up(out):
                        rest_up = AF.out_upsample(out[:, n0:], 0, n1, self._diag_bias)
                    else:
                        rest_up = uflow_utils.upsample(out[:, n0:] + self._diag_bias, is_flow=False)
                    cfg = AF.LevelCfg([0, 'flow', 1, 'vol', 2], 'avg', alpha, 4, True, False, 'zeros', True, AF.NORM_UFLOW)
                    x_in, flow_up = AF.level(features1, features2, out[:, 0:2], cfg, context_up, rest_up, features1,
                                             x1_rows=r1)
                    out_up = torch.cat([flow_up, rest_up], 1)
            else:
                out_up = self.upsample_out(out)
                warped2 = mum.uflow_utils.resample_flow(features2, out_up[:, 0:2])  # :282
                f1n, w2n = mum.normalize_features([features1, warped2], normalize=norm, center=norm,
                                                  moments_across_channels=True, moments_across_images=True)
                x_in = mum.cost_volume_concat(f1n, w2n, (context_up, out_up), (features1,), max_displacement=4,
                                              negative_slope=alpha)
            context, out = dense_level(self._flow_layers[level], x_in, None if drops is None else drops[k])
            k += 1
            if out.shape[1] > n01:  # :337-341: the output level's head is wider than what came up the pyramid
                out_up = func.pad(out_up, (0, 0, 0, 0, 0, out.shape[1] - n01))
            out = out + out_up
            context_up = self._context_up_layers[level](context)
            outs.insert(0, out)
        refinement = refine(self._refine_model, torch.cat([context, out], dim=1))
        if drops is not None:
            refinement = refinement * drops[k]
        refined = out + refinement
        # :375-381: log(precision) / 2 not too small, log(variance) / 2 neither too small nor too large
        if n1 > 0:
            log_diag = refined[:, n0:n01]
            log_diag = torch.clamp(log_diag, min=-5.0) if self._inv_cov else torch.clamp(log_diag, max=10.0, min=-10.0)
            outs[0] = torch.cat([refined[:, 0:n0], log_diag, refined[:, n01:]], dim=1)
        else:  # the clamp acts on an empty slice
            outs[0] = refined
        if self._native_up(outs[0]):
            out_1, out_0 = AF.out_tail(outs[0], n0, n1, self._diag_bias)
        else:
            out_1 = self.upsample_out(outs[0])
            out_0 = self.upsample_out(out_1)
        outs.insert(0, out_1)
        outs.insert(0, out_0)
        return outs

    def forward(self, img1, img2, with_bk=True):
        B = img1.size(0)
        extractor = self._feature_pyramid_extractor[0]
        pyr_all = extractor(torch.cat([img1, img2], 0))
        return pair_pass(pyr_all, extractor.pyramid_moments, B, with_bk,
                         lambda p1, p2, n_passes, m: self.forward_2_frames(p1, p2, self._drops(n_passes, B, img1.device), m))


def flows_concat(flow1, flow2):
    """:98-106: per level, the two components' means and then their log-diagonals."""
    return [torch.cat((a[:, 0:2], b[:, 0:2], a[:, 2:4], b[:, 2:4]), dim=1) for a, b in zip(flow1, flow2)]


class ComponentNet(nn.Module):
    """:109-147: one PWCProbFlow ([2, 2, 0], one pyramid) per mixture component; state-dict keys pwcnet1.*, pwcnet2.*."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        if cfg.mixture_weights:
            raise NotImplementedError('ComponentNet: mixture_weights = %r (MixtureWeightsNet cannot run in the reference '
                                      'either: DESIGN.md section 26)' % (cfg.mixture_weights,))
        cfg1, cfg2 = AttrDict(dict(cfg)), AttrDict(dict(cfg))
        for c in (cfg1, cfg2):
            c.out_channels = [2, 2, 0]
            c.mixture_weights = False
            c.n_pyramids = 1
        self.pwcnet1 = PWCProbFlow(cfg1)
        self.pwcnet2 = PWCProbFlow(cfg2)

    def init_weights(self):
        self.pwcnet1.init_weights()
        self.pwcnet2.init_weights()

    def forward(self, img1, img2, with_bk=True):
        # pwcnet1, then pwcnet2: level dropout consumes the CPU generator in the reference's sequence
        res1 = self.pwcnet1(img1, img2, with_bk=with_bk)
        res2 = self.pwcnet2(img1, img2, with_bk=with_bk)
        return {key: flows_concat(res1[key], res2[key]) for key in res1}
