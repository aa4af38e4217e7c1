"""unFlowLoss (ARFlow pyramid loss) on the gfx950 kernels -- same constructor, inputs and 4-tuple
result as losses/flow_loss.py:8-114."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as AF
from ..loss_blocks import smooth_grad_1st, smooth_grad_2nd
from ..ddp import global_denominator
from ..warp_utils import flow_warp, get_occu_mask_backward, get_occu_mask_bidirection


class unFlowLoss(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg

    def loss_photomatric(self, im1_scaled, im1_recons, occu_mask1):
        """losses/flow_loss.py:13-27 as ONE fused launch: L1, SSIM and mask sums together."""
        cfg = self.cfg
        if cfg.w_ternary > 0:
            # float * (dist, mask) tuple in the reference (flow_loss.py:23-25, loss_blocks.py:62)
            raise TypeError("unsupported operand type(s) for *: 'float' and 'tuple' "
                            '(unFlowLoss with w_ternary > 0 is broken in the reference as well)')
        b, c, h, w = im1_scaled.shape
        s = AF.PhotoSumsFunction.apply(im1_scaled, im1_recons, occu_mask1)
        total = 0.
        if cfg.w_l1 > 0:
            total = total + cfg.w_l1 * s[0] / float(b * c * h * w)
        if cfg.w_ssim > 0:
            total = total + cfg.w_ssim * s[1] / float(b * c * (h - 2) * (w - 2))
        # mask.mean() of the gathered batch when global normalisation is on (ddp.global_denominator), else this rank's
        return total / (global_denominator(s[2]) / float(b * h * w))

    def loss_smooth(self, flow, im1_scaled, scale):
        cfg = self.cfg
        if 'smooth_2nd' in cfg and cfg.smooth_2nd:
            s = AF.smooth_sums(flow, im1_scaled, scale, cfg.alpha, 2, 0, 0)
            b, _, h, w = flow.shape
            return (s[0] / float(b * 2 * h * (w - 2))) / 2. + (s[1] / float(b * 2 * (h - 2) * w)) / 2.
        s = AF.smooth_sums(flow, im1_scaled, scale, cfg.alpha, 1, 0, 0)
        b, _, h, w = flow.shape
        return (s[0] / float(b * 2 * h * (w - 1)) / 2.) / 2. + (s[1] / float(b * 2 * (h - 1) * w) / 2.) / 2.

    pair = True  # False: the two directions one after the other (the reference's order)

    def _photo_from_sums(self, s, b, c, h, w):
        """loss_photomatric on the three sums of one direction."""
        cfg = self.cfg
        total = 0.
        if cfg.w_l1 > 0:
            total = total + cfg.w_l1 * s[0] / float(b * c * h * w)
        if cfg.w_ssim > 0:
            total = total + cfg.w_ssim * s[1] / float(b * c * (h - 2) * (w - 2))
        return total / (global_denominator(s[2]) / float(b * h * w))

    def _occlusion_planes(self, flow):
        """Finest scale, fused path: the occlusion plane of each direction as a [B,1,h,w] view (the mask is 1 - plane,
        formed inside the fused pass).  flow: contiguous [B,4,h,w] = 2B two-channel flows interleaved, used in place."""
        B, _, h, w = flow.shape
        if self.cfg.occ_from_back:  # direction 1 is occluded where flow 2 -> 1 leaves holes, and vice versa
            occ = get_occu_mask_backward(flow.view(2 * B, 2, h, w), th=0.2).view(B, 2, h, w)
            return occ[:, 1:2], occ[:, 0:1]
        return get_occu_mask_bidirection(flow[:, :2], flow[:, 2:]), get_occu_mask_bidirection(flow[:, 2:], flow[:, :2])

    def _forward_stacked(self, output, target):
        """with_bk as ONE pass over 2B samples (first B: direction 1 -> 2, last B: direction 2 -> 1; every op on this path is
        per sample).  Per pyramid scale the photometric sums of both directions come from one fused launch
        (AF.photo_warp_sums: warp, mask and L1/SSIM; images, flows and occlusion planes are read where they are, the area
        resizes of all scales come from one AF.area_pyramid launch) and the smoothness term is launched only where its weight
        is non-zero.  A scale the fused pass does not cover (AF.photo_warp_supported), or ARFLOW_PHOTO_WARP=0, takes the
        composed path: one area resize, one warp, one mask resize and one photometric launch per direction -- the
        photometric sums stay per direction (each is divided by its own mask mean, losses/flow_loss.py:27)."""
        cfg = self.cfg
        B = target.shape[0]
        target = target.contiguous()
        size0 = output[0].shape[-2:]
        fused = [AF.photo_warp_enabled() and cfg.w_scales[i] != 0 and AF.photo_warp_supported(target, flow, size0)
                 for i, flow in enumerate(output)]
        if any(fused) and cfg.w_ternary > 0:
            self.loss_photomatric(None, None, None)  # raises: broken in the reference as well
        sizes = [tuple(flow.shape[-2:]) for flow, u in zip(output, fused) if u]
        pyramid = dict(zip(sizes, AF.area_pyramid(target, sizes))) if sizes else {}
        imgs = None
        warp_losses, smooth_losses = [], []
        self.pyramid_occu_mask1, self.pyramid_occu_mask2 = [], []
        s, m0, planes, invert = 1., None, None, False
        for i, flow in enumerate(output):
            if cfg.w_scales[i] == 0:
                warp_losses.append(0)
                smooth_losses.append(0)
                continue
            _, _, h, w = flow.shape
            if i == 0:
                s = min(h, w)
            if fused[i]:
                flow = flow.contiguous()
                im = pyramid[(h, w)]  # [B,6,h,w]: image 1 and 2 of every pair
                if i == 0:
                    planes, invert = self._occlusion_planes(flow.detach()), True
                sums, m = AF.photo_warp_sums((im[:, :3], im[:, 3:]), (im[:, 3:], im[:, :3]), flow, planes, pad=cfg.warp_pad,
                                             mask_mode='plane' if i == 0 else 'nearest', mask_invert=invert, want_mask=True)
                if i == 0:
                    m0 = m
                self.pyramid_occu_mask1.append(m[:B])
                self.pyramid_occu_mask2.append(m[B:])
                warp_losses.append((self._photo_from_sums(sums[0], B, 3, h, w) + self._photo_from_sums(sums[1], B, 3, h, w)) / 2.)
                # 2B two-channel flows / 2B images, interleaved and in place; the mean over them IS the directions' average
                smooth_losses.append(self.loss_smooth(flow.view(2 * B, 2, h, w), im.view(2 * B, 3, h, w), 1.0 / s)
                                     if cfg.w_sm_scales[i] != 0 else 0)
                continue
            if imgs is None:
                imgs = torch.cat([target[:, :3], target[:, 3:]], 0)
            im = F.interpolate(imgs, (h, w), mode='area')
            f = torch.cat([flow[:, :2], flow[:, 2:]], 0)
            rec = flow_warp(torch.roll(im, B, 0), f, pad=cfg.warp_pad)
            if i == 0:
                fsw = torch.roll(f, B, 0)
                m = 1 - (get_occu_mask_backward(fsw, th=0.2) if cfg.occ_from_back else get_occu_mask_bidirection(f, fsw))
                m0 = m
                planes, invert = (m0[:B], m0[B:]), False
            else:
                m = F.interpolate(m0, (h, w), mode='nearest')
            self.pyramid_occu_mask1.append(m[:B])
            self.pyramid_occu_mask2.append(m[B:])
            warp_losses.append((self.loss_photomatric(im[:B], rec[:B], m[:B]) + self.loss_photomatric(im[B:], rec[B:], m[B:])) / 2.)
            smooth_losses.append(self.loss_smooth(f, im, 1.0 / s))  # the mean over 2B samples IS the directions' average
        warp_loss = sum(l * w for l, w in zip(warp_losses, cfg.w_scales))
        smooth_loss = cfg.w_smooth * sum(l * w for l, w in zip(smooth_losses, cfg.w_sm_scales))
        return warp_loss + smooth_loss, warp_loss, smooth_loss, output[0].abs().mean()

    def forward(self, output, target):
        cfg = self.cfg
        if self.pair and cfg.with_bk and target.is_cuda and all(f.shape[1] == 4 for f in output):
            return self._forward_stacked(output, target)
        im1_origin, im2_origin = target[:, :3], target[:, 3:]
        warp_losses, smooth_losses = [], []
        self.pyramid_occu_mask1, self.pyramid_occu_mask2 = [], []
        s = 1.
        for i, flow in enumerate(output):
            if cfg.w_scales[i] == 0:
                warp_losses.append(0)
                smooth_losses.append(0)
                continue
            _, _, h, w = flow.shape
            im1 = F.interpolate(im1_origin, (h, w), mode='area')
            im2 = F.interpolate(im2_origin, (h, w), mode='area')
            rec1 = flow_warp(im2, flow[:, :2], pad=cfg.warp_pad)
            rec2 = flow_warp(im1, flow[:, 2:], pad=cfg.warp_pad)
            if i == 0:
                if cfg.occ_from_back:
                    m1 = 1 - get_occu_mask_backward(flow[:, 2:], th=0.2)
                    m2 = 1 - get_occu_mask_backward(flow[:, :2], th=0.2)
                else:
                    m1 = 1 - get_occu_mask_bidirection(flow[:, :2], flow[:, 2:])
                    m2 = 1 - get_occu_mask_bidirection(flow[:, 2:], flow[:, :2])
            else:
                m1 = F.interpolate(self.pyramid_occu_mask1[0], (h, w), mode='nearest')
                m2 = F.interpolate(self.pyramid_occu_mask2[0], (h, w), mode='nearest')
            self.pyramid_occu_mask1.append(m1)
            self.pyramid_occu_mask2.append(m2)

            l_warp = self.loss_photomatric(im1, rec1, m1)
            if i == 0:
                s = min(h, w)
            l_smooth = self.loss_smooth(flow[:, :2], im1, 1.0 / s)
            if cfg.with_bk:
                l_warp = (l_warp + self.loss_photomatric(im2, rec2, m2)) / 2.
                l_smooth = (l_smooth + self.loss_smooth(flow[:, 2:], im2, 1.0 / s)) / 2.
            warp_losses.append(l_warp)
            smooth_losses.append(l_smooth)

        warp_loss = sum(l * w for l, w in zip(warp_losses, cfg.w_scales))
        smooth_loss = cfg.w_smooth * sum(l * w for l, w in zip(smooth_losses, cfg.w_sm_scales))
        return warp_loss + smooth_loss, warp_loss, smooth_loss, output[0].abs().mean()
