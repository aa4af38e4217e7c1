"""PWCLiteProb host model on the gfx950 ops: the probabilistic form of ARFlow's PWCLite.  Same constructor
cfg keys (upsample, n_frames, reduce_dense), forward contract and state_dict layout as models/pwclite_prob.py:110-235: every
pyramid level carries a (flow, log-variance) state of 2 + 2 channels, the estimator and the context network emit residuals of
both, and each of the five outputs is cat(flow, log_var) -- at four times the level's resolution with `upsample`, for ALL
levels (PWCLite upsamples only the finest).

On the GPU the level's flow x2 upsample is folded into the warp launch (AF.warp_up2, as PWCLite), the log-variance comes up
with AF.prob_upsample(.., 2, 0, 2, 2 ln 2), the cost volume is written straight into the estimator input, and with `upsample`
one AF.prob_upsample(state, 4, 2, 2, 2 ln 4) per level writes the [B,4,4h,4w] output directly: no cat of the two groups, no
F.interpolate.  CPU tensors, and a twin that has swapped blocks.bias_act out
(oracle.host_models.oracle_ops), keep the ATen expressions of the reference."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as AF
from ..correlation import Correlation
from . import blocks
# flow_warp is called as an attribute of the pwclite module (mp.flow_warp), never bound here: oracle_ops substitutes exactly
# that attribute, so a twin of this model runs on the oracle ops as it stands
from . import pwclite as mp
from .blocks import ContextNetwork, FeatureExtractor, FlowEstimatorDense, FlowEstimatorReduce, conv, init_conv_weights, pair_pass

LOG_VAR_MAX = 10.0  # :207


class PWCLiteProb(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.search_range = 4
        self.ch_out = 4
        self.num_chs = [3, 16, 32, 64, 96, 128, 192]
        self.output_level = 4
        self.num_levels = 7
        self.leakyRELU = nn.LeakyReLU(0.1, inplace=True)
        self.feature_pyramid_extractor = FeatureExtractor(self.num_chs)
        self.upsample = cfg.upsample
        self.n_frames = cfg.n_frames
        self.reduce_dense = cfg.reduce_dense
        self.corr = Correlation(pad_size=self.search_range, kernel_size=1, max_displacement=self.search_range,
                                stride1=1, stride2=1, corr_multiply=1)
        self.dim_corr = (self.search_range * 2 + 1) ** 2
        self.num_ch_in = 32 + (self.dim_corr + self.ch_out) * (self.n_frames - 1)
        est = FlowEstimatorReduce if self.reduce_dense else FlowEstimatorDense
        self.flow_estimators = est(self.num_ch_in, self.ch_out)
        self.context_networks = ContextNetwork((self.flow_estimators.feat_dim + self.ch_out) * (self.n_frames - 1), self.ch_out)
        self.conv_1x1 = nn.ModuleList([conv(c, 32, kernel_size=1, stride=1, dilation=1)
                                       for c in (192, 128, 96, 64, 32)])
        self._caps = {}  # device -> the clamp's per-channel maximum (not a buffer: the state_dict is the reference's)

    def num_parameters(self):
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    def init_weights(self):
        init_conv_weights(self, 'kaiming')

    def _native_up(self, x):
        """A twin that has swapped bias_act out keeps the ATen resize: the convention of blocks.HeadConv.native."""
        return AF.out_up_supported(x) and blocks.bias_act is AF.bias_leaky_relu

    def _cap(self, x):
        key = (x.device, x.dtype)
        if key not in self._caps:
            self._caps[key] = torch.tensor([math.inf, math.inf, LOG_VAR_MAX, LOG_VAR_MAX], dtype=x.dtype,
                                           device=x.device).view(1, 4, 1, 1)
        return self._caps[key]

    def up(self, x, factor, n_flow, n_diag):
        """F.interpolate(flow * factor, x factor) of the first n_flow channels and F.interpolate(log_var + 2 ln factor, x
        factor) of the next n_diag, bilinear, align_corners=True (:183-186, :216-217)."""
        bias = 2 * math.log(factor)
        if self._native_up(x):
            return AF.prob_upsample(x, factor, n_flow, n_diag, bias)
        parts = []
        if n_flow:
            parts.append(F.interpolate(x[:, :n_flow] * factor, scale_factor=factor, mode='bilinear', align_corners=True))
        if n_diag:
            parts.append(F.interpolate(x[:, n_flow:n_flow + n_diag] + bias, scale_factor=factor, mode='bilinear',
                                       align_corners=True))
        return parts[0] if len(parts) == 1 else torch.cat(parts, 1)

    def forward_2_frames(self, x1_pyramid, x2_pyramid):
        """:163-220.  state = cat(flow, log_var) [B,4,h,w] throughout."""
        outputs = []
        b, _, h, w = x1_pyramid[0].shape
        dev = x1_pyramid[0].device
        flow = torch.zeros(b, 2, h, w, dtype=torch.float32, device=dev)
        log_var = torch.ones(b, 2, h, w, dtype=torch.float32, device=dev)
        state = None
        for l, (x1, x2) in enumerate(zip(x1_pyramid, x2_pyramid)):
            if l == 0:
                x2_warp = x2
            else:
                flow, log_var = state[:, 0:2], state[:, 2:4]
                if AF.warp_up2_supported(x2, flow):
                    x2_warp, flow = AF.warp_up2(x2, flow, up_align=True)
                else:
                    flow = self.up(flow, 2, 2, 0)
                    x2_warp = mp.flow_warp(x2, flow)
                log_var = self.up(log_var, 2, 0, 2)
            x1_1by1 = self.conv_1x1[l](x1)
            # corr + LeakyReLU(0.1) in one kernel, written straight into the estimator's concatenated input
            x_in = self.corr.concat(x1, x2_warp, after=(x1_1by1, flow, log_var), negative_slope=0.1)
            x_intm, res = self.flow_estimators(x_in)
            # (not x_in[:, -4:]: the backward of that slice zero-fills a gradient as wide as the whole estimator input)
            state = torch.cat([flow, log_var], 1) + res
            state = state + self.context_networks(torch.cat([x_intm, state], dim=1))
            state = torch.clamp(state, max=self._cap(state))  # :207: the log-variance channels only
            outputs.append(state)
            if l == self.output_level:
                break
        if self.upsample:
            outputs = [self.up(s, 4, 2, 2) for s in outputs]  # :215-217: all five levels
        return outputs[::-1]

    def forward(self, x, with_bk=False):
        """:222-235 -> {'flows_fw': [...], 'flows_bw': [...]} finest first, each [B,4,h,w] = (flow, log_var)."""
        n_frames = x.size(1) // 3
        if n_frames != 2 or x.size(1) != 6:
            raise NotImplementedError
        B = x.size(0)
        # one extractor pass over both frames (batch 2B); the image level the reference appends to its pyramids is never read
        pyr_all = self.feature_pyramid_extractor(torch.cat([x[:, 0:3], x[:, 3:6]], 0))
        return pair_pass(pyr_all, None, B, with_bk, lambda p1, p2, n_passes, m: self.forward_2_frames(p1, p2))
