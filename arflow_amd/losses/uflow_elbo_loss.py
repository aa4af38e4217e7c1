"""UFlowElboLoss on the gfx950 kernels -- the constructor, inputs and 8-tuple result of losses/uflow_elbo_loss.py:108-568
(DESIGN.md section 21).

Per step (with_bk, the usual case): the samples of BOTH directions are drawn by two launches of the fused sampler
(csrc/band.hip: z = mean + L eps, the coefficients read once for all n_samples) straight into one [S B,4,h,w] (fw, bw)
tensor, which then IS the batch of 2 S B samples n = 2 (s B + b) + direction that UFlowLoss's one-pass pair kernels take:
one upsample, one launch for the grey planes and x1/4 copies of the B image pairs (repeated to S B), range maps +
smoothness sums, census of both directions, and ONE launch backward for all of it.  What the reference computes with
`data_loss: ['census']`, `data_penalty: ['abs_robust_loss']`, `occ_type: 'sample'` is exactly UFlowLoss's census term on the
sampled flows, and its sampled charbonnier smoothness is edge_asymp s(0) + (1 - edge_asymp) s(edge_constant) with s(alpha)
UFlowLoss's first-order smoothness at edge constant alpha.

Supported: approx 'diag' (inv_cov, approx_entropy, closed_form_smooth with order_smooth 1 / 2 and isotropic_smooth) and
'sparse' (inv_cov false, cov_supp 1..3, offdiag_reg) and 'lowrank' (inv_cov false, columns 1..16: the sampler and the Gram
log-determinants of csrc/lowrank.hip; approx_entropy is not consulted, as in the reference); any
n_samples; with_bk; w_oof, w_occ; and 'mixture' (inv_cov false, n_components 2..4: the sampler, the mixture log-density and
their one backward launch of csrc/mixture.hip; level-2 outputs of 4 n_components channels = the
components' means, then their log-stds; weights from res_dict['weights_fw'] / ['weights_bw'] or uniform; approx_entropy is not
consulted, as in the reference).  UFlowElboLoss itself takes data_penalty ['abs_robust_loss'], penalty_smooth 'charbonnier' and
occ_type 'sample' and refuses every other value of the three at construction; UFlowElboPenLoss, the subclass get_loss returns
for any other setting, takes: data_penalty[0] in abs_robust_loss, identity, charbonnier,
gmm (mixture from penalty_census_pi / penalty_census_beta); penalty_smooth in charbonnier, identity, abs_robust_loss, gmm
(penalty_smooth_pi / penalty_smooth_beta), sampled and in both closed forms; occ_type 'sample' or 'mean' (range map of the
partner's MEAN flow, validity of the x4 upsample of the own mean; not with approx 'mixture', which has no single mean).  The
default setting (abs_robust_loss, charbonnier, sample) makes exactly the calls described above; any other runs the penalised
census forward (arflow_census_warp_pair_pen_fwd and its siblings) and, for the smoothness, arflow_smooth_pen_fwd / _bwd: the
backward is then arflow_census_warp_pair_bwd plus a smoothness backward, two launches.  Everything else raises
NotImplementedError naming the value; a malformed mixture raises ValueError.  A missing `isotropic_smooth` / `order_smooth` reads as False / 1 (the reference
raises AttributeError on its own chairs_uflow_elbo_nondiag.json, which omits them).
"""
import torch
import torch.nn as nn

from .. import functional as AF
from ..lowrank import RMAX, reparam_lowrank_pair
from ..mixture import KMAX, reparam_gmm_pair
from ..triag_solve import reparam_triag_pair
from ..uflow_utils import census_loss, flow_to_warp, image_grads
from .penalty_functions import check_mixture, get_penalty


def _charbonnier(x_sq, eps=0.001):
    """losses/penalty_functions.py:6-7."""
    return torch.sqrt(x_sq + eps ** 2)


def range_map(flow):
    """compute_range_map (utils/uflow_utils.py:80-160) in plain torch, differentiable in the flow: the w_occ term takes its
    gradient through the bilinear splat weights.  flow [B,2,h,w] -> [B,1,h,w]."""
    B, _, h, w = flow.shape
    coords = flow_to_warp(flow)
    fl = torch.floor(coords)
    frac = coords - fl
    ix, iy = fl[:, 0].long(), fl[:, 1].long()
    base = torch.arange(B, device=flow.device).view(B, 1, 1) * (h * w)
    counts = torch.zeros(B * h * w, dtype=flow.dtype, device=flow.device)
    for di in range(2):
        for dj in range(2):
            yy, xx = iy + di, ix + dj
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            wy = (1. - di) - (-1) ** di * frac[:, 1]
            wx = (1. - dj) - (-1) ** dj * frac[:, 0]
            counts = counts.index_add(0, (base + yy * w + xx)[ok], (wy * wx)[ok])
    return counts.view(B, 1, h, w)


class UFlowElboLoss(nn.Module):
    # what this class takes; UFlowElboPenLoss below widens the three sets (get_loss chooses between the two)
    DATA_PENALTIES = ('abs_robust_loss',)
    SMOOTH_PENALTIES = ('charbonnier',)
    OCC_TYPES = ('sample',)

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.fused = True  # False: the unfused photometric path (warp, mask upsample and census as separate launches)
        self.pair = True   # False: the two directions one after the other (the reference's order)
        if cfg.approx not in ('diag', 'sparse', 'lowrank', 'mixture'):
            raise NotImplementedError("approx: %r (supported: 'diag', 'sparse', 'lowrank', 'mixture')" % (cfg.approx,))
        if cfg.approx == 'mixture':
            K = getattr(cfg, 'n_components', None)
            if isinstance(K, bool) or not isinstance(K, (int, float)) or int(K) != K or not 2 <= int(K) <= KMAX:
                raise NotImplementedError("approx: 'mixture' with n_components: %r (supported: 2..%d; one component is "
                                          "approx: 'diag')" % (K, KMAX))
        if cfg.approx == 'lowrank':
            columns = getattr(cfg, 'columns', None)
            if columns is None:
                raise NotImplementedError("approx: 'lowrank' needs `columns` (1..%d), the number of columns per flow "
                                          "component" % RMAX)
            if int(columns) != columns or not 1 <= int(columns) <= RMAX:
                raise NotImplementedError('columns: %r (supported: 1..%d)' % (columns, RMAX))
            if cfg.inv_cov:
                raise NotImplementedError("inv_cov: True with approx: 'lowrank'")
        if cfg.occ_type not in self.OCC_TYPES:
            raise NotImplementedError("occ_type: %r (supported by %s: %s)" % (cfg.occ_type, type(self).__name__, list(self.OCC_TYPES)))
        if cfg.occ_type == 'mean' and cfg.approx == 'mixture':
            raise NotImplementedError("occ_type: 'mean' with approx: 'mixture' (a mixture has no single mean flow)")
        if list(cfg.data_loss) != ['census']:
            raise NotImplementedError("data_loss: %r (supported: ['census'])" % (list(cfg.data_loss),))
        data_penalty = list(cfg.data_penalty)
        if len(data_penalty) != 1 or data_penalty[0] not in self.DATA_PENALTIES:
            raise NotImplementedError("data_penalty: %r (supported by %s: one of %s)"
                                      % (data_penalty, type(self).__name__, list(self.DATA_PENALTIES)))
        if cfg.penalty_smooth not in self.SMOOTH_PENALTIES:
            raise NotImplementedError("penalty_smooth: %r (supported by %s: %s)"
                                      % (cfg.penalty_smooth, type(self).__name__, list(self.SMOOTH_PENALTIES)))
        # the default setting keeps the calls it has always made; everything else goes through the penalised entry points
        self.default = (data_penalty[0], cfg.penalty_smooth, cfg.occ_type) == ('abs_robust_loss', 'charbonnier', 'sample')
        census_mix = smooth_mix = (None, None)
        if data_penalty[0] == 'gmm':
            census_mix = check_mixture(getattr(cfg, 'penalty_census_pi', None), getattr(cfg, 'penalty_census_beta', None),
                                       "data_penalty 'gmm' (penalty_census_pi / penalty_census_beta)")
        if cfg.penalty_smooth == 'gmm':
            smooth_mix = check_mixture(getattr(cfg, 'penalty_smooth_pi', None), getattr(cfg, 'penalty_smooth_beta', None),
                                       "penalty_smooth 'gmm' (penalty_smooth_pi / penalty_smooth_beta)")
        self.data_pen = AF.make_penalty(data_penalty[0], *census_mix)
        # the sampled smoothness of a non-default penalty: the descriptor of rho over the SQUARED differences (None: charbonnier,
        # arflow_smooth_fwd's own penalty 1); the closed forms, plain torch, take the callable
        self.smooth_pen = None if cfg.penalty_smooth == 'charbonnier' else AF.make_penalty(cfg.penalty_smooth, *smooth_mix,
                                                                                          squared=True)
        self.smooth_fn = _charbonnier if cfg.penalty_smooth == 'charbonnier' else get_penalty(
            cfg.penalty_smooth, pi=smooth_mix[0], beta=smooth_mix[1], squared=True)
        self.closed = bool(getattr(cfg, 'closed_form_smooth', False))
        self.isotropic = bool(getattr(cfg, 'isotropic_smooth', False))
        self.order = int(getattr(cfg, 'order_smooth', 1))
        if self.closed and (cfg.approx != 'diag' or self.order not in (1, 2)):
            raise NotImplementedError('closed_form_smooth with approx: %r, order_smooth: %r (supported: diag with 1 or 2)' %
                                      (cfg.approx, self.order))
        if not self.closed and self.isotropic:
            raise NotImplementedError('isotropic_smooth: True with sampled smoothness (closed_form_smooth: False)')
        if cfg.approx == 'sparse' and not cfg.inv_cov and int(cfg.cov_supp) not in (1, 2, 3):
            raise NotImplementedError('cov_supp: %r (supported: 1..3)' % (cfg.cov_supp,))

    # ---- the pieces -------------------------------------------------------------------------------------------
    def _split(self, net):
        """Level-2 output [B,C,h,w] -> mean, log_diag, diag = exp(+-log_diag), offdiag (None for 'diag') as channel slices;
        'lowrank': mean, None, None, std [B,2 columns,h,w]; 'mixture': the K means [B,2K,h,w], the K log-stds, None, None."""
        cfg = self.cfg
        if cfg.approx == 'mixture':
            K = int(cfg.n_components)
            if net.shape[1] != 4 * K:
                raise ValueError('approx mixture with n_components %d needs %d level-2 channels (got %d)' % (K, 4 * K, net.shape[1]))
            return net[:, 0:2 * K], net[:, 2 * K:4 * K], None, None
        if cfg.approx == 'lowrank':
            R = int(cfg.columns)
            if net.shape[1] != 2 + 2 * R:
                raise ValueError('approx lowrank with columns %d needs %d level-2 channels (got %d)' % (R, 2 + 2 * R, net.shape[1]))
            return net[:, 0:2], None, None, net[:, 2:2 + 2 * R]
        mean, log_diag = net[:, 0:2], net[:, 2:4]
        off = None
        if cfg.approx == 'sparse':
            n = (int(cfg.cov_supp) + 1) ** 2 - 1
            off = net[:, 4:4 + 2 * n]
            if off.shape[1] != 2 * n:
                raise ValueError('approx sparse with cov_supp %d needs %d level-2 channels (got %d)' %
                                 (cfg.cov_supp, 4 + 2 * n, net.shape[1]))
        diag = torch.exp(-log_diag if (cfg.approx == 'diag' and cfg.inv_cov) else log_diag)
        return mean, log_diag, diag, off

    def _smooth_weights(self, small, stride, halve):
        cfg = self.cfg
        gx, gy = image_grads(small, stride)
        ea = float(getattr(cfg, 'edge_asymp', 0.0))
        wx = ea + (1.0 - ea) * torch.exp(-torch.mean(torch.abs(cfg.edge_constant * gx), 1, keepdim=True))
        wy = ea + (1.0 - ea) * torch.exp(-torch.mean(torch.abs(cfg.edge_constant * gy), 1, keepdim=True))
        return (wx / 2., wy / 2.) if halve else (wx, wy)

    def _closed_smooth(self, mean, diag, small):
        """The expected squared differences of a diagonal Gaussian in closed form (losses/uflow_elbo_loss.py:406-502), in
        plain torch on the [B,2,h,w] level-2 tensors: first order with the halved edge weights of smooth_loss_no_penalty,
        second order with the stride-2 image gradients and unhalved weights, as the reference has them.  With
        isotropic_smooth the reference's mean over the channels drops that axis, and its product with the [B,1,..]
        weights then pairs every sample's weights with every sample's differences; that is reproduced as it stands."""
        cfg = self.cfg
        if self.order == 1:
            wx, wy = self._smooth_weights(small, 1, True)
            Ex = (mean[:, :, :, 1:] - mean[:, :, :, :-1]) ** 2 + diag[:, :, :, 1:] ** 2 + diag[:, :, :, :-1] ** 2
            Ey = (mean[:, :, 1:] - mean[:, :, :-1]) ** 2 + diag[:, :, 1:] ** 2 + diag[:, :, :-1] ** 2
        else:
            wx, wy = self._smooth_weights(small, 2, False)
            Ex = ((mean[:, :, :, :-2] - 2 * mean[:, :, :, 1:-1] + mean[:, :, :, 2:]) ** 2
                  + diag[:, :, :, 0:-2] ** 2 + 4 * diag[:, :, :, 1:-1] ** 2 + diag[:, :, :, 2:] ** 2)
            Ey = ((mean[:, :, :-2] - 2 * mean[:, :, 1:-1] + mean[:, :, 2:]) ** 2
                  + diag[:, :, 0:-2] ** 2 + 4 * diag[:, :, 1:-1] ** 2 + diag[:, :, 2:] ** 2)
        if self.isotropic:
            Ex, Ey = torch.mean(Ex, dim=1), torch.mean(Ey, dim=1)
        return torch.mean(wx * cfg.w_smooth * self.smooth_fn(Ex)) + torch.mean(wy * cfg.w_smooth * self.smooth_fn(Ey))

    def _sampled_smooth(self, s_alpha, flow2, small, n_per_direction):
        """s_alpha: the smoothness sums at edge_constant, or None (computed here); -> the sampled charbonnier term."""
        cfg = self.cfg
        ea = float(getattr(cfg, 'edge_asymp', 0.0))
        if s_alpha is None:
            s_alpha = AF.smooth_sums(flow2, small, 1.0, float(cfg.edge_constant), 1, 1, 1)
        s = s_alpha
        if ea != 0.0:  # weights ea + (1 - ea) exp(-alpha |grad|): the constant part is the same sum at alpha = 0
            s = ea * AF.smooth_sums(flow2, small, 1.0, 0.0, 1, 1, 1) + (1.0 - ea) * s_alpha
        h, w = flow2.shape[2:]
        nx, ny = float(n_per_direction * 2 * h * (w - 1)), float(n_per_direction * 2 * (h - 1) * w)
        return cfg.w_smooth * (s[0] / nx + s[1] / ny) / 2.

    def _sampled_smooth_pen(self, flow2, small, n_per_direction):
        """_sampled_smooth under a non-default smoothness penalty (arflow_smooth_pen_fwd / _bwd)."""
        cfg = self.cfg
        if self.smooth_pen is None:
            return self._sampled_smooth(None, flow2, small, n_per_direction)
        ea = float(getattr(cfg, 'edge_asymp', 0.0))
        s = AF.smooth_pen_sums(flow2, small, 1.0, float(cfg.edge_constant), 1, 1, self.smooth_pen)
        if ea != 0.0:
            s = ea * AF.smooth_pen_sums(flow2, small, 1.0, 0.0, 1, 1, self.smooth_pen) + (1.0 - ea) * s
        h, w = flow2.shape[2:]
        nx, ny = float(n_per_direction * 2 * h * (w - 1)), float(n_per_direction * 2 * (h - 1) * w)
        return cfg.w_smooth * (s[0] / nx + s[1] / ny) / 2.

    def _direction_pen(self, a, b, flow_ab0, occ_small, valid_flow0):
        """_direction under the penalty self.data_pen: occ_small is the range map that masks this direction (of the partner's
        samples, or of its mean), valid_flow0 the flow mask_invalid is taken of (None: flow_ab0)."""
        if a['gray'] is not None:
            l_c, _ = AF.census_warp_pen_loss(a['gray'], b['gray'], flow_ab0, occ_small, self.data_pen, valid_flow0, 7)
            return l_c
        recons, valid = AF.warp_with_valid(b['im'].detach(), flow_ab0, pad='zeros', align_corners=True, norm=AF.NORM_UFLOW)
        if valid_flow0 is not None:
            valid = AF.coord_mask(valid_flow0, 0)
        return AF.census_pen_loss(a['im'], recons, AF.up4_clamp_mul(occ_small, valid), self.data_pen, 7)

    def _pen_terms(self, im1_0, im2_0, flows2, f0, mean12, mean21, S, with_bk, grey):
        """The data term and the sampled smoothness of every non-default setting -> (loss_warp, loss_smooth or None, the range
        map [S B,1,h,w] masking the forward direction, the validity flow of the forward direction or None, small1, small2).
        f0: flows0 [2 S B,2,H,W] (with_bk) or the forward level-0 flows."""
        cfg = self.cfg
        SB, _, h, w = flows2.shape
        B = SB // S
        H, W = 4 * h, 4 * w
        flow12_2, flow21_2 = flows2[:, 0:2], flows2[:, 2:4]
        mean = cfg.occ_type == 'mean'
        vf_fw = vf_bw = None
        if mean:  # everything detached: the masks carry no gradient (losses/uflow_elbo_loss.py:42-50)
            m12, m21 = mean12.detach().contiguous(), mean21.detach().contiguous()
            range21 = AF.splat_map(m21, 0).repeat(S, 1, 1, 1)
            vf_fw = AF.interpolate_flow(m12, 4, False).repeat(S, 1, 1, 1)
            if with_bk:
                range12 = AF.splat_map(m12, 0).repeat(S, 1, 1, 1)
                vf_bw = AF.interpolate_flow(m21, 4, False).repeat(S, 1, 1, 1)
        else:
            range21 = AF.splat_map(flow21_2, 0)
            if with_bk:
                range12 = AF.splat_map(flow12_2, 0)
        loss_smooth = None
        if grey and self.pair and with_bk:
            small, gray = AF.down4_gray(torch.cat((im1_0, im2_0), 1).view(2 * B, 3, H, W))
            small_rep, gray_rep = small.repeat(S, 1, 1, 1), gray.repeat(S, 1, 1, 1)
            occ = torch.stack((range12, range21), 1).view(2 * SB, 1, h, w)  # plane n masks sample n ^ 1
            vf = torch.stack((vf_fw, vf_bw), 1).view(2 * SB, 2, H, W) if mean else None
            l_fw, l_bw, _ = AF.census_warp_pair_pen_loss(gray_rep, f0, occ, self.data_pen, vf, 7)
            loss_warp = cfg.data_weight[0] * l_fw + cfg.data_weight[0] * l_bw
            small1, small2 = small.view(B, 2, 3, h, w)[:, 0], small.view(B, 2, 3, h, w)[:, 1]
            if not self.closed:
                loss_smooth = self._sampled_smooth_pen(flows2.view(2 * SB, 2, h, w), small_rep, SB)
        else:
            one, two = self._prepare(im1_0, S, grey), self._prepare(im2_0, S, grey)
            f0_fw, f0_bw = (f0.view(SB, 2, 2, H, W)[:, 0], f0.view(SB, 2, 2, H, W)[:, 1]) if with_bk else (f0, None)
            loss_warp = cfg.data_weight[0] * self._direction_pen(one, two, f0_fw, range21, vf_fw)
            if with_bk:
                loss_warp = loss_warp + cfg.data_weight[0] * self._direction_pen(two, one, f0_bw, range12, vf_bw)
            small1, small2 = one['small1'], two['small1']
            if not self.closed:
                loss_smooth = self._sampled_smooth_pen(flow12_2, one['small'], SB)
                if with_bk:
                    loss_smooth = loss_smooth + self._sampled_smooth_pen(flow21_2, two['small'], SB)
        return loss_warp, loss_smooth, range21, vf_fw, small1, small2

    def _direction(self, a, b, flow_ab0, flow_ba2):
        """One photometric direction as UFlowLoss._direction composes it -> (census loss, range map of the partner)."""
        occ_small = AF.splat_map(flow_ba2, 0)
        if a['gray'] is not None:
            l_c, _ = AF.census_warp_loss(a['gray'], b['gray'], flow_ab0, occ_small, 7)
        else:
            recons, valid = AF.warp_with_valid(b['im'].detach(), flow_ab0, pad='zeros', align_corners=True, norm=AF.NORM_UFLOW)
            l_c = census_loss(a['im'], recons, AF.up4_clamp_mul(occ_small, valid))
        return l_c, occ_small

    def _mixture_samples(self, res_dict, net12, net21, S, eps, comp):
        """The mixture's samples of both directions and their log-densities (:224-237, :307-309) -> (flows [S B,4,h,w], logpdf
        [2,S B]).  What is not given is drawn in the reference's order: components then noise, forward direction first."""
        B, _, h, w = net12.shape
        K = int(self.cfg.n_components)
        if 'weights_fw' in res_dict:
            weights = (res_dict['weights_fw'], res_dict['weights_bw'])
        else:
            weights = (torch.full((B, K), 1.0 / K, device=net12.device, dtype=net12.dtype),) * 2
        dirs = []
        for d, net in enumerate((net12, net21)):
            c = comp[d] if comp is not None else torch.multinomial(weights[d].detach(), S, replacement=True)
            e = eps[d] if eps is not None else torch.randn((S * B, 2, h, w), device=net.device, dtype=net.dtype)
            dirs.append((net, weights[d], c, e))
        return reparam_gmm_pair(dirs[0], dirs[1], S)

    def _prepare(self, im, S, grey):
        if grey:
            small, gray = AF.down4_gray(im)
            return {'im': None, 'small': small.repeat(S, 1, 1, 1), 'gray': gray.repeat(S, 1, 1, 1), 'small1': small}
        small = AF.down4(im)
        return {'im': im.repeat(S, 1, 1, 1), 'small': small.repeat(S, 1, 1, 1), 'gray': None, 'small1': small}

    # ---- forward ----------------------------------------------------------------------------------------------
    def forward(self, res_dict, im1_0, im2_0, eps=None, comp=None):
        """res_dict['flows_fw'][2], ['flows_bw'][2]: the level-2 outputs [B,C,h,w] (mean, log_diag, off-diagonals; 'lowrank':
        mean, columns; 'mixture': means, log-stds); im1_0, im2_0 [B,3,4h,4w]; eps: (eps12, eps21), each [S B,2,h,w] ('lowrank':
        [S B,2 columns,1,1]), drawn on the device (forward direction first) when None; comp ('mixture' only): (comp12, comp21),
        each [B,S] int64, the recorded component draws, torch.multinomial on the device when None.  -> (total, loss_warp, loss_smooth, loss_entropy, loss_oof, flow12_2, occu_mask12, valid_mask12)."""
        cfg = self.cfg
        if cfg.natural_grad:
            raise NotImplementedError("Natural gradient is not implemented!")
        if cfg.approx == 'sparse' and cfg.inv_cov:
            raise NotImplementedError("Sparse precision matrix representation is not implemented!")
        mixture = cfg.approx == 'mixture'
        if mixture and cfg.inv_cov:
            raise NotImplementedError('Inverse covariance parametrization is not implemented for mixture variational '
                                      'approximation.')
        if comp is not None and not mixture:
            raise ValueError('comp: component draws belong to approx mixture (approx is %r)' % (cfg.approx,))
        net12, net21 = res_dict['flows_fw'][2], res_dict['flows_bw'][2]
        S, with_bk = int(cfg.n_samples), bool(cfg.with_bk)
        B, _, h, w = net12.shape
        H, W = im1_0.shape[2:]
        if (H, W) != (4 * h, 4 * w):
            raise ValueError('the images must be 4x the level-2 output (%dx%d vs %dx%d)' % (H, W, h, w))
        k = int(cfg.cov_supp) if cfg.approx == 'sparse' else 0
        mean12, log_diag12, diag12, off12 = self._split(net12)
        mean21, log_diag21, diag21, off21 = self._split(net21)

        # reparameterisation: both directions into one (fw, bw) tensor
        lowrank = cfg.approx == 'lowrank'
        if mixture:
            flows2, logpdf = self._mixture_samples(res_dict, net12, net21, S, eps, comp)  # [S B,4,h,w], [2,S B]
        else:
            if eps is None:
                shape = (S * B, off12.shape[1], 1, 1) if lowrank else (S * B, 2, h, w)
                eps12 = torch.randn(shape, device=net12.device, dtype=net12.dtype)
                eps21 = torch.randn(shape, device=net12.device, dtype=net12.dtype)
            else:
                eps12, eps21 = eps
            if lowrank:  # off12, off21: the columns
                flows2, logdet = reparam_lowrank_pair((mean12, off12, eps12), (mean21, off21, eps21), S)  # [S B,4,h,w], [2,B,2]
            else:
                flows2 = reparam_triag_pair((mean12, diag12, off12, eps12), (mean21, diag21, off21, eps21), k, S)  # [S B,4,h,w]
        flow12_2, flow21_2 = flows2[:, 0:2], flows2[:, 2:4]

        # entropy
        sign = -1.0 if cfg.inv_cov else 1.0
        if mixture:  # :358-361: minus the mean log-density of the samples, per direction
            loss_entropy = -cfg.w_entropy * logpdf[0].mean()
            if with_bk:
                loss_entropy = loss_entropy - cfg.w_entropy * logpdf[1].mean()
        elif lowrank:  # :362-381: (logdet G_u + logdet G_v) / (2 h w), mean over the batch, per direction
            loss_entropy = cfg.w_entropy * (logdet[0].sum(1) / (2 * h * w)).mean()
            if with_bk:
                loss_entropy = loss_entropy + cfg.w_entropy * (logdet[1].sum(1) / (2 * h * w)).mean()
        elif cfg.approx == 'diag' and not cfg.inv_cov and cfg.approx_entropy:
            t12 = (flow12_2 - mean12.detach().repeat(S, 1, 1, 1)) / diag12.detach().repeat(S, 1, 1, 1)
            loss_entropy = cfg.w_entropy * torch.sum(t12 * t12 / 2, dim=1).mean()
            if with_bk:
                t21 = (flow21_2 - mean21.detach().repeat(S, 1, 1, 1)) / diag21.detach().repeat(S, 1, 1, 1)
                loss_entropy = loss_entropy + cfg.w_entropy * torch.sum(t21 * t21 / 2, dim=1).mean()
        else:
            loss_entropy = sign * cfg.w_entropy * torch.sum(log_diag12, dim=1).mean()
            if with_bk:
                loss_entropy = loss_entropy + sign * cfg.w_entropy * torch.sum(log_diag21, dim=1).mean()

        # data term on level 0, sampled smoothness on level 2
        grey = self.fused and AF.census_warp_supported(H, W)
        if with_bk:
            flows0 = AF.interpolate_flow(flows2.view(2 * S * B, 2, h, w), 4, False)  # [2 S B,2,H,W], n = 2 (s B + b) + direction
            f0_fw, f0_bw = flows0.view(S * B, 2, 2, H, W)[:, 0], flows0.view(S * B, 2, 2, H, W)[:, 1]
        else:  # the backward samples are only read at level 2, for the range map
            f0_fw, f0_bw = AF.interpolate_flow(flow12_2.contiguous(), 4, False), None
        valid_mask12 = AF.coord_mask(f0_fw, 0)
        s_alpha = None
        if not self.default:
            loss_warp, loss_smooth, range21, vf_fw, small1, small2 = self._pen_terms(
                im1_0, im2_0, flows2, flows0 if with_bk else f0_fw, mean12, mean21, S, with_bk, grey)
            if vf_fw is not None:
                valid_mask12 = AF.coord_mask(vf_fw, 0)
        elif grey and self.pair and with_bk:
            small, gray = AF.down4_gray(torch.cat((im1_0, im2_0), 1).view(2 * B, 3, H, W))
            small_rep, gray_rep = small.repeat(S, 1, 1, 1), gray.repeat(S, 1, 1, 1)
            occ = torch.zeros(2 * S * B, 1, h, w, device=net12.device, dtype=torch.float32)
            l_fw, l_bw, s_alpha, _ = AF.uflow_pair_loss(gray_rep, small_rep, flows0, flows2.view(2 * S * B, 2, h, w), occ,
                                                        float(cfg.edge_constant), 1, 7)
            loss_warp = cfg.data_weight[0] * l_fw + cfg.data_weight[0] * l_bw
            occ = occ.view(S * B, 2, 1, h, w)
            range21 = occ[:, 1]
            small1, small2 = small.view(B, 2, 3, h, w)[:, 0], small.view(B, 2, 3, h, w)[:, 1]
            if not self.closed:
                loss_smooth = self._sampled_smooth(s_alpha, flows2.view(2 * S * B, 2, h, w), small_rep, S * B)
        else:
            one, two = self._prepare(im1_0, S, grey), self._prepare(im2_0, S, grey)
            l_c, range21 = self._direction(one, two, f0_fw, flow21_2)
            loss_warp = cfg.data_weight[0] * l_c
            if with_bk:
                l_c, _ = self._direction(two, one, f0_bw, flow12_2)
                loss_warp = loss_warp + cfg.data_weight[0] * l_c
            small1, small2 = one['small1'], two['small1']
            if not self.closed:
                loss_smooth = self._sampled_smooth(None, flow12_2, one['small'], S * B)
                if with_bk:
                    loss_smooth = loss_smooth + self._sampled_smooth(None, flow21_2, two['small'], S * B)
        if self.closed:
            loss_smooth = self._closed_smooth(mean12, diag12, small1)
            if with_bk:
                loss_smooth = loss_smooth + self._closed_smooth(mean21, diag21, small2)

        # out-of-frame and occlusion penalties: plain torch on the level-2 samples
        loss_oof = 0
        if cfg.w_oof > 0.0:
            for f in ((flow12_2, flow21_2) if with_bk else (flow12_2,)):
                warp = flow_to_warp(f)
                u = torch.clamp(warp[:, 0], max=0) ** 2 + torch.clamp(warp[:, 0] - float(w - 1), min=0) ** 2
                v = torch.clamp(warp[:, 1], max=0) ** 2 + torch.clamp(warp[:, 1] - float(h - 1), min=0) ** 2
                loss_oof = loss_oof + cfg.w_oof * (u + v).mean()
        loss_occ = 0
        if cfg.w_occ > 0.0:  # the reference differentiates this term through the range map as well
            # occ_type 'mean': the masks data_loss_no_penalty returned, the range maps of the (repeated) mean flows
            occ_of12, occ_of21 = (mean12.repeat(S, 1, 1, 1), mean21.repeat(S, 1, 1, 1)) if cfg.occ_type == 'mean' else (flow12_2, flow21_2)
            occu_mask12 = torch.clamp(range_map(occ_of21), min=0., max=1.)
            loss_occ = cfg.w_occ * (1 / (100.0 * occu_mask12 + 1) * torch.square(flow12_2)).mean()
            if with_bk:
                occu_mask21 = torch.clamp(range_map(occ_of12), min=0., max=1.)
                loss_occ = loss_occ + cfg.w_occ * (1 / (100.0 * occu_mask21 + 1) * torch.square(flow21_2)).mean()
        else:
            occu_mask12 = torch.clamp(range21, min=0., max=1.)

        total = loss_warp + loss_smooth - loss_entropy + loss_oof + loss_occ
        if cfg.approx == 'sparse':
            loss_offdiag = torch.mean(torch.square(off12))
            if with_bk:
                loss_offdiag = loss_offdiag + torch.mean(torch.square(off21))
            total = total + cfg.offdiag_reg * loss_offdiag
        return total, loss_warp, loss_smooth, loss_entropy, loss_oof, flow12_2, occu_mask12, valid_mask12


class UFlowElboPenLoss(UFlowElboLoss):
    """UFlowElboLoss with the selectable penalties and mean-flow masks of DESIGN.md section 45: what get_loss returns for
    type 'uflow_elbo' whenever (data_penalty, penalty_smooth, occ_type) is not (abs_robust_loss, charbonnier, sample).  The
    base class keeps refusing those settings, as it always has; with the default triple this class makes the base's calls."""
    DATA_PENALTIES = ('abs_robust_loss', 'identity', 'charbonnier', 'gmm')
    SMOOTH_PENALTIES = ('charbonnier', 'identity', 'abs_robust_loss', 'gmm')
    OCC_TYPES = ('sample', 'mean')


def takes_default_path(cfg):
    """True where UFlowElboLoss itself runs the config's penalties and masks (get_loss's choice of class)"""
    return (list(cfg.data_penalty), cfg.penalty_smooth, cfg.occ_type) == (['abs_robust_loss'], 'charbonnier', 'sample')
