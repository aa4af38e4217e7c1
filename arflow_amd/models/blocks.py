"""Shared conv building blocks of the PWC-style host models (plain torch.nn; MIOpen does the convs).
Module / parameter names follow the reference so its checkpoints load by name."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as AF

bias_act = AF.bias_leaky_relu  # (conv output, bias, slope) -> activation; substituted by oracle.host_models on CPU


class ConvAct(nn.Sequential):
    """Sequential(Conv2d(bias=True), LeakyReLU) with the reference's parameter names (``0.weight``,
    ``0.bias``), evaluated as bias-free MIOpen convolution + ONE fused bias/LeakyReLU pass (and one fused
    LeakyReLU-derivative/bias-gradient pass backward) instead of conv, bias add, LeakyReLU and a separate
    full-tensor reduction for the bias gradient."""

    want_moments = False  # set on the conv that OUTPUTS a pyramid level: its epilogue also leaves that map's moments
    last_moments = None

    def split_route(self, x):
        """(forward, data gradient) on the split-bf16 kernel (AF.conv3x3): a CUDA fp32 4-D input of a 3x3 / stride 1 / padding 1 /
        dilation 1 layer under the package's own bias_act -- the conditions HeadConv.native spells out -- at a shape
        AF.splitconv_takes routes; the data gradient asks with the channel counts swapped, which is the call the kernel sees."""
        if not self._split_kind(x):
            return False, False
        c = self[0]
        N, C, H, W = x.shape
        return AF.splitconv_takes(N, C, c.out_channels, H, W), AF.splitconv_takes(N, c.out_channels, C, H, W)

    def split_wgrad_route(self, x):
        """The weight gradient on the split-bf16 kernel: the same kind of layer and input, at a shape
        AF.splitconv_wgrad_takes routes (asked with the layer's own (C, K))."""
        if not self._split_kind(x):
            return False
        N, C, H, W = x.shape
        return AF.splitconv_wgrad_takes(N, C, self[0].out_channels, H, W)

    def _split_kind(self, x):
        c = self[0]
        return (AF.splitconv_enabled() and bias_act is AF.bias_leaky_relu and x.is_cuda and x.dtype == torch.float32 and
                x.dim() == 4 and c.weight.dtype == torch.float32 and c.kernel_size == (3, 3) and c.stride == (1, 1) and
                c.padding == (1, 1) and c.dilation == (1, 1) and c.groups == 1 and c.padding_mode == 'zeros')

    def forward(self, x):
        c, act = self[0], self[1]
        fwd, dgrad = self.split_route(x)
        wgrad = self.split_wgrad_route(x)
        if fwd or dgrad or wgrad:
            y = AF.conv3x3(x, c.weight, fwd, dgrad, wgrad)
        else:
            y = F.conv2d(x, c.weight, None, c.stride, c.padding, c.dilation, c.groups)
        if self.want_moments and y.is_cuda and bias_act is AF.bias_leaky_relu:
            y, self.last_moments = AF.bias_leaky_relu_moments(y, c.bias, act.negative_slope)
            return y
        self.last_moments = None
        return bias_act(y, c.bias, act.negative_slope)


class HeadConv(nn.Sequential):
    """Sequential(Conv2d(bias=True)) with the reference's parameter names (``0.weight``, ``0.bias``): the layers conv()
    builds with isReLU=False, i.e. the two-channel flow heads.  A CUDA fp32 input of a 3x3 / stride 1 / padding 1 /
    dilation 1 / two-output layer goes through the direct kernels (AF.head_conv); any other layer, every CPU tensor and
    a twin that has swapped `bias_act` out keep F.conv2d."""

    def native(self, x):
        c = self[0]
        return (AF.head_conv_enabled() and bias_act is AF.bias_leaky_relu and x.is_cuda and x.dtype == torch.float32 and
                x.dim() == 4 and c.weight.dtype == torch.float32 and c.out_channels == 2 and c.kernel_size == (3, 3) and
                c.stride == (1, 1) and c.padding == (1, 1) and c.dilation == (1, 1) and c.groups == 1 and
                c.padding_mode == 'zeros')

    def forward(self, x):
        c = self[0]
        if self.native(x):
            return AF.head_conv(x, c.weight, c.bias)
        return F.conv2d(x, c.weight, c.bias, c.stride, c.padding, c.dilation, c.groups)


def conv(in_planes, out_planes, kernel_size=3, stride=1, dilation=1, isReLU=True):
    """models/pwclite.py:10-23 -- Sequential(Conv2d[, LeakyReLU(0.1)]) -> keys ``<name>.0.weight``."""
    layers = [nn.Conv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, dilation=dilation,
                        padding=((kernel_size - 1) * dilation) // 2, bias=True)]
    if isReLU:
        layers.append(nn.LeakyReLU(0.1, inplace=True))
        return ConvAct(*layers)
    return HeadConv(*layers)


def deconv(in_planes, out_planes, kernel_size=4, stride=2, padding=1):
    """models/pwclite_uflow.py:26-27."""
    return nn.ConvTranspose2d(in_planes, out_planes, kernel_size, stride, padding, bias=True)


class FeatureExtractor(nn.Module):
    """models/pwclite.py:26-45 (2 convs per level) / models/pwclite_uflow.py:40-62 (3 convs per level,
    input rescaled to [-1,1])."""

    def __init__(self, num_chs, convs_per_level=2, rescale_input=False, moments=False):
        """moments=True (not in the reference's signature): the last conv of every level also leaves the partial moments
        of its output (normalize_features' sums, taken in the fused bias/LeakyReLU epilogue) in `pyramid_moments`,
        coarsest first like the pyramid -- [B, rows, 2] float64 per level, or None off the GPU path."""
        super().__init__()
        self.num_chs = num_chs
        self.rescale_input = rescale_input
        self.convs = nn.ModuleList()
        for ch_in, ch_out in zip(num_chs[:-1], num_chs[1:]):
            layers = [conv(ch_in, ch_out, stride=2)] + [conv(ch_out, ch_out) for _ in range(convs_per_level - 1)]
            layers[-1].want_moments = bool(moments)
            self.convs.append(nn.Sequential(*layers))
        self.pyramid_moments = None

    def forward(self, x):
        if self.rescale_input:
            x = x * 2. - 1.
        pyramid, moms = [], []
        for level in self.convs:
            x = level(x)
            pyramid.append(x)
            moms.append(level[-1].last_moments)
        self.pyramid_moments = moms[::-1]
        return pyramid[::-1]


class FlowEstimatorDense(nn.Module):
    """models/pwclite.py:48-66; ch_out as models/pwclite_prob.py:49-50 (a head wider than two channels keeps F.conv2d and the
    tensor expression below: HeadConv.native and the dense node are two-channel)."""

    def __init__(self, ch_in, ch_out=2):
        super().__init__()
        self.conv1 = conv(ch_in, 128)
        self.conv2 = conv(ch_in + 128, 128)
        self.conv3 = conv(ch_in + 256, 96)
        self.conv4 = conv(ch_in + 352, 64)
        self.conv5 = conv(ch_in + 416, 32)
        self.feat_dim = ch_in + 448
        self.conv_last = conv(ch_in + 448, ch_out, isReLU=False)

    def native(self, x):
        """The whole estimator as one autograd node (AF.dense_estimator) under the rule HeadConv.native applies: a CUDA fp32
        4-D input and the package's own bias_act (a twin that has swapped it out keeps the tensor expression below)."""
        return AF.dense_block_enabled() and self.conv_last.native(x) and self.conv1[0].weight.dtype == torch.float32

    def forward(self, x):
        layers = (self.conv1, self.conv2, self.conv3, self.conv4, self.conv5)
        if self.native(x):
            params = [p for layer in layers + (self.conv_last,) for p in (layer[0].weight, layer[0].bias)]
            return AF.dense_estimator(x, self.conv1[1].negative_slope, params)
        for layer in layers:
            x = torch.cat([layer(x), x], dim=1)
        return x, self.conv_last(x)


class FlowEstimatorReduce(nn.Module):
    """models/pwclite.py:69-88; ch_out as models/pwclite_prob.py:72."""

    def __init__(self, ch_in, ch_out=2):
        super().__init__()
        self.conv1 = conv(ch_in, 128)
        self.conv2 = conv(128, 128)
        self.conv3 = conv(128 + 128, 96)
        self.conv4 = conv(128 + 96, 64)
        self.conv5 = conv(96 + 64, 32)
        self.feat_dim = 32
        self.predict_flow = conv(64 + 32, ch_out, isReLU=False)

    def forward(self, x):
        x1 = self.conv1(x)
        x2 = self.conv2(x1)
        x3 = self.conv3(torch.cat([x1, x2], dim=1))
        x4 = self.conv4(torch.cat([x2, x3], dim=1))
        x5 = self.conv5(torch.cat([x3, x4], dim=1))
        return x5, self.predict_flow(torch.cat([x4, x5], dim=1))


class ContextNetwork(nn.Module):
    """models/pwclite.py:91-106 -- 7 dilated convs; ch_out as models/pwclite_prob.py:93."""

    def __init__(self, ch_in, ch_out=2):
        super().__init__()
        self.convs = nn.Sequential(
            conv(ch_in, 128, 3, 1, 1), conv(128, 128, 3, 1, 2), conv(128, 128, 3, 1, 4), conv(128, 96, 3, 1, 8),
            conv(96, 64, 3, 1, 16), conv(64, 32, 3, 1, 1), conv(32, ch_out, isReLU=False))

    def native(self, x):
        """Layers 2..5 -- the dilated ones -- as one autograd node on the split-bf16 kernels (AF.dilated_chain) under the rule
        ConvAct._split_kind applies: a CUDA fp32 4-D input, the package's own bias_act, the reference's four layer shapes, at a
        size AF.dilated_chain_takes routes (a twin that has swapped bias_act out, and every smaller map, keep the Sequential)."""
        if not (bias_act is AF.bias_leaky_relu and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
            return False
        convs = [layer[0] for layer in self.convs[1:5]]
        kind = all(c.weight.dtype == torch.float32 and c.kernel_size == (3, 3) and c.stride == (1, 1) and c.padding == c.dilation and
                   c.dilation[0] == c.dilation[1] and c.groups == 1 and c.padding_mode == 'zeros' and c.bias is not None for c in convs)
        shapes = tuple((c.in_channels, c.out_channels, c.dilation[0]) for c in convs)
        slopes = {layer[1].negative_slope for layer in self.convs[1:5]}
        return (kind and shapes == AF.DILATED_CHAIN_LAYERS and len(slopes) == 1 and
                AF.dilated_chain_takes(x.shape[0], x.shape[2], x.shape[3]))

    def forward(self, x):
        if not self.native(x):
            return self.convs(x)
        x = self.convs[0](x)
        params = [p for layer in self.convs[1:5] for p in (layer[0].weight, layer[0].bias)]
        x = AF.dilated_chain(x, self.convs[1][1].negative_slope, params)
        return self.convs[6](self.convs[5](x))


def init_conv_weights(module, scheme):
    """kaiming-normal (models/pwclite.py:149-159) or xavier-uniform (models/pwclite_uflow.py:179-191),
    zero bias, over Conv2d and ConvTranspose2d in named_modules() order."""
    for layer in module.modules():
        if isinstance(layer, (nn.Conv2d, nn.ConvTranspose2d)):
            if scheme == 'kaiming':
                nn.init.kaiming_normal_(layer.weight)
            else:
                nn.init.xavier_uniform_(layer.weight)
            if layer.bias is not None:
                nn.init.constant_(layer.bias, 0)


def level_drops(training, rate, n, n_passes, batch_per_pass, device):
    """Level-dropout multipliers [n, n_passes * batch_per_pass, 1, 1, 1], or None outside training / at rate 0.  Drawn from
    the CPU RNG in the reference's order: the n draws of a pass (one per level, then one for the context / refinement net;
    models/pwclite_uflow.py:226-229,240-242) before those of the next pass."""
    if not (training and rate > 0):
        return None
    vals = [[float(torch.rand(1) > rate) for _ in range(n)] for _ in range(n_passes)]
    t = torch.tensor(vals, dtype=torch.float32)                      # [passes, n]
    t = t.repeat_interleave(batch_per_pass, dim=0).t().contiguous()  # [n, passes*B]
    return t.to(device, non_blocking=True).view(n, -1, 1, 1, 1)


def pair_pass(pyr_all, moms, B, with_bk, run):
    """The two-frame pass over the extractor's output for the batch (frame1; frame2): `pyr_all` its 2B pyramid, `moms` the
    rows of partial moments per level or None, run(pyr1, pyr2, n_passes, moments) the model's decoder (moments = (rows of
    the first maps, rows of the second maps) or None when any level has none).  with_bk: the forward and the backward flow
    are estimated in ONE pass at batch 2B -- every op on the path is per-sample, so the result equals the reference's two
    sequential passes (models/pwclite.py:267-269) while every launch covers twice the pixels.  The first maps of the 2B
    (fw; bw) samples are the extractor's batch as it stands (no copy), the second maps its two halves swapped; the same
    holds for the moment rows."""
    have_m = moms is not None and all(t is not None for t in moms)
    if with_bk:
        swapped = [torch.cat([p[B:], p[:B]], 0) for p in pyr_all]
        m = (list(moms), [torch.roll(t, B, 0) for t in moms]) if have_m else None
        flows = run(list(pyr_all), swapped, 2, m)
        return {'flows_fw': [f[:B] for f in flows], 'flows_bw': [f[B:] for f in flows]}
    m = ([t[:B] for t in moms], [t[B:] for t in moms]) if have_m else None
    return {'flows_fw': run([p[:B] for p in pyr_all], [p[B:] for p in pyr_all], 1, m)}
