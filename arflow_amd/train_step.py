"""Synthetic-data training step: the inner loop of the reference trainer
(trainer/uflow_trainer.py:30-91: model(img_pair, with_bk=True) -> cat(fw,bw) per level -> loss ->
zero_grad / backward / optimizer.step) as a reusable object, with one-process-per-GPU gradient
all-reduce instead of DataParallel and without the per-step host syncs (``loss.item()`` NaN assert,
trainer/uflow_trainer.py:57-61, is replaced by an on-device isfinite flag read at the end)."""
import torch

from .config import AttrDict
from .ddp import FlatGradAllReduce
from .losses import get_loss
from .models import get_model

# name -> (model cfg, loss cfg); hyper-parameters from configs/chairs_uflow.json:17-48 where present
WORKLOADS = {
    # BASELINE config 2: "PWCLite 2-frame fwd+bwd ... (correlation d=4 + warp + uflow_loss)".  The ARFlow
    # PWCLite class cannot feed UFlowLoss, so it is the UFlow-structured PWCLite.
    'pwclite_uflow+uflow_loss': (
        dict(type='pwclite_uflow', level_dropout=0.1, feature_norm=True, align_corners=True, warp_pad='zeros',
             n_frames=2, reduce_dense=False),
        dict(type='uflow', edge_constant=150, w_smooth=4.0, w_census=1.0, with_bk=True, smooth_order=1)),
    'pwclite+unflow_loss': (
        dict(type='pwclite', upsample=True, n_frames=2, reduce_dense=True),
        dict(type='unflow', w_l1=0.15, w_ssim=0.85, w_ternary=0.0, warp_pad='border', alpha=10, occ_from_back=True,
             with_bk=True, w_smooth=75.0, w_scales=[1.0, 1.0, 1.0, 1.0, 1.0, 0.0],
             w_sm_scales=[1.0, 0.0, 0.0, 0.0, 0.0, 0.0])),
    # build-defined (the reference ships no config for the pair): the probabilistic PWCLite and the ELBO form of the loss above,
    # its weights on the model's five scales
    'pwcliteprob+elbo_loss': (
        dict(type='pwclite_prob', upsample=True, n_frames=2, reduce_dense=True),
        dict(type='elbo', w_l1=0.15, w_ssim=0.85, w_ternary=0.0, warp_pad='border', alpha=10, occ_from_back=True,
             with_bk=True, w_smooth=75.0, w_scales=[1.0, 1.0, 1.0, 1.0, 1.0], w_sm_scales=[1.0, 0.0, 0.0, 0.0, 0.0],
             w_en_scales=[1.0, 1.0, 1.0, 1.0, 1.0], w_entropy=0.1)),
    # BASELINE config 5: 3-frame PWCLite (forward_3_frames) + the build-defined multi-view objective
    'pwclite3+mv_loss': (
        dict(type='pwclite', upsample=True, n_frames=3, reduce_dense=True),
        dict(type='mv', w_l1=0.15, w_ssim=0.85, alpha=10, w_smooth=75.0, w_scales=[1.0, 1.0, 1.0, 1.0, 0.0],
             w_sm_scales=[1.0, 0.0, 0.0, 0.0, 0.0])),
    # BASELINE config 4: configs/chairs_uflow.json (model type 'uflow' = PWCFlow)
    'pwcflow+uflow_loss': (
        dict(type='uflow', feature_norm=True, level_dropout=0.1),
        dict(type='uflow', edge_constant=150, w_smooth=4.0, w_census=1.0, with_bk=True, smooth_order=1)),
    # configs/chairs_uflow_elbo_nondiag.json:23-55 (model type 'uflow_prob' = PWCProbFlow, banded covariance factor)
    'pwcprobflow+uflow_elbo_loss': (
        dict(type='uflow_prob', feature_norm=True, level_dropout=0.1, out_channels=[2, 2, 30], inv_cov=False, n_pyramids=1,
             mixture_weights=False),
        dict(type='uflow_elbo', edge_constant=150, edge_asymp=0.01, w_smooth=4.0, penalty_smooth='charbonnier',
             closed_form_smooth=False, data_loss=['census'], data_weight=[1.0], data_penalty=['abs_robust_loss'],
             w_entropy=0.1, w_oof=0.0, w_occ=0.0, with_bk=True, approx='sparse', n_components=1, cov_supp=3, inv_cov=False,
             approx_entropy=False, occ_type='sample', n_samples=4, offdiag_reg=0.0, natural_grad=False)),
    # configs/chairs_uflow_elbo_lowrank.json:7-39 (PWCProbFlow without log-diagonal channels, 15 columns per flow component)
    'pwcprobflow+uflow_elbo_lowrank': (
        dict(type='uflow_prob', feature_norm=True, level_dropout=0.0, out_channels=[2, 0, 30], inv_cov=False, n_pyramids=1,
             mixture_weights=False),
        dict(type='uflow_elbo', edge_constant=150, edge_asymp=0.01, w_smooth=4.0, penalty_smooth='charbonnier',
             closed_form_smooth=False, data_loss=['census'], data_weight=[1.0], data_penalty=['abs_robust_loss'],
             w_entropy=0.1, w_oof=0.0, w_occ=0.0, with_bk=True, approx='lowrank', columns=15, n_components=1, inv_cov=False,
             approx_entropy=False, occ_type='sample', n_samples=4, offdiag_reg=0.0, natural_grad=False)),
    # configs/chairs_uflow_elbo_mixture.json:10-36 with the model that can run it: ComponentNet (one PWCProbFlow [2,2,0] per
    # mixture component) and uniform weights; the keys the file omits as the other ELBO workloads set them
    'componentnet+uflow_elbo_mixture': (
        dict(type='component', feature_norm=True, level_dropout=0.1, out_channels=[2, 2, 0], inv_cov=False, n_pyramids=2,
             mixture_weights=False),
        dict(type='uflow_elbo', edge_constant=150, edge_asymp=0.01, w_smooth=4.0, penalty_smooth='charbonnier',
             closed_form_smooth=False, data_loss=['census'], data_weight=[1.0], data_penalty=['abs_robust_loss'],
             w_entropy=0.3, w_oof=0.0, w_occ=0.0, with_bk=True, approx='mixture', n_components=2, inv_cov=False,
             approx_entropy=False, occ_type='sample', n_samples=6, offdiag_reg=0.0, natural_grad=False)),
    # configs/chairs_uflow_mse.json:8-22: the supervised objective on the level-2 output of PWCProbFlow (out_channels 8 =
    # mean, log-diagonal and the 4-neighbour coefficients of a precision factor); the step takes a ground-truth flow
    'pwcprobflow+mse_loss': (
        dict(type='uflow_prob', feature_norm=True, level_dropout=0.1, out_channels=[2, 2, 4], inv_cov=True, n_pyramids=1,
             mixture_weights=False),
        dict(type='mse', w_mse=1.0, w_entropy=0.1, diag=False, diag_dominant=False, inv_cov=True, approx_entropy=False,
             offdiag_reg=1000.0, n_samples=1)),
}


def synthetic_pairs(batch, height, width, frames=2, device='cuda', seed=0):
    """U[0,1) images smoothed by one 5x5 box blur so census / SSIM see structure."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    x = torch.rand(batch, 3 * frames, height, width, generator=g)
    x = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (2, 2, 2, 2), mode='reflect'), 5, 1)
    return x.to(device)


def synthetic_flow(batch, height, width, device='cuda', seed=0):
    """A smooth ground-truth flow of a few pixels for the supervised workloads: N(0, 1) on a grid 16 times coarser, resized
    bilinearly and scaled by 4."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    coarse = torch.randn(batch, 2, max(height // 16, 1), max(width // 16, 1), generator=g)
    flow = 4.0 * torch.nn.functional.interpolate(coarse, (height, width), mode='bilinear', align_corners=True)
    return flow.to(device)


class TrainStep:
    def __init__(self, workload, device, lr=1e-4, seed=0, n_buckets=4, feature_storage='fp32', train_cfg=None, ar_cfg=None):
        """train_cfg: the `train` section of a config (optim, lr, decay groups, clip, lr schedule): the step is then taken by
        arflow_amd.optim.FlatOptimizer on the flat gradient buffer and `lr` is ignored.  None: torch.optim.Adam as below.
        ar_cfg: the augmentation-regularisation pass (arflow_amd.ar; build-defined wiring): w_ar, ar_eps
        (0.0), ar_q (1.0), mask_st (True) and st_cfg (ar.draw_ar_params; missing keys read as off).  None: no second pass."""
        mcfg, lcfg = WORKLOADS[workload]
        if ar_cfg is not None and lcfg['type'] in ('mse', 'elbo', 'uflow_elbo'):
            raise ValueError('ar_cfg is wired into the unsupervised flow losses only, not into loss type %r' % lcfg['type'])
        self.ar_cfg = ar_cfg
        self.ar_generator = None if ar_cfg is None else torch.Generator(device='cpu').manual_seed(int(seed))
        self.last_ar = None
        if feature_storage != 'fp32':
            if mcfg['type'] != 'pwclite_uflow':
                raise ValueError('feature_storage=%r is wired into the pwclite_uflow model only' % feature_storage)
            mcfg = dict(mcfg, feature_storage=feature_storage)
        self.model_cfg, self.loss_cfg = AttrDict(mcfg), AttrDict(lcfg)
        torch.manual_seed(seed)
        self.model = get_model(self.model_cfg)
        self.model.init_weights()
        self.model.to(device).train()
        self.loss = get_loss(self.loss_cfg)
        import os
        self.reducer = FlatGradAllReduce(self.model, n_buckets=n_buckets,
                                         force_collectives=os.environ.get('ARFLOW_FORCE_COLLECTIVES') == '1')
        self.reducer.broadcast_parameters(0)
        # optional gathered-batch loss normalisation (one scalar all-reduce per masked term)
        from . import ddp
        ddp.enable_global_loss_norm(os.environ.get('ARFLOW_GLOBAL_LOSS_NORM') == '1')
        # Adam, lr 1e-4, betas (0.9, 0.999), eps 1e-8, no decay: configs/chairs_uflow.json:29-48
        kw = dict(lr=lr, betas=(0.9, 0.999), eps=1e-8)
        if train_cfg is not None:
            from .optim import FlatOptimizer
            self.opt = FlatOptimizer(self.reducer, train_cfg)
        else:
            try:
                self.opt = torch.optim.Adam(self.model.parameters(), fused=(device.type == 'cuda'), **kw)
            except (TypeError, RuntimeError):
                self.opt = torch.optim.Adam(self.model.parameters(), **kw)
        self.last = None
        self._target = None

    def __call__(self, img_pair, target=None, img_pair_ph=None):
        """img_pair_ph: the photometrically augmented version of img_pair (arflow_amd.augment).  The model sees it, the loss
        always sees img_pair (trainer/uflow_trainer.py:47-54); None: the model sees img_pair too."""
        model_in = img_pair if img_pair_ph is None else img_pair_ph
        if model_in.shape != img_pair.shape:
            raise ValueError('img_pair_ph must have the shape of img_pair %s (got %s)'
                             % (tuple(img_pair.shape), tuple(model_in.shape)))
        if self.loss_cfg.type == 'mse':  # supervised: the forward direction alone against the ground-truth flow
            if target is None:  # a seeded synthetic flow of the batch's shape, made once
                shape = (img_pair.shape[0],) + tuple(img_pair.shape[2:])
                if self._target is None or self._target[0] != shape:
                    self._target = (shape, synthetic_flow(*shape, device=img_pair.device, seed=7))
                target = self._target[1]
            res = self.model(model_in[:, :3], model_in[:, 3:], with_bk=False)
            return self._step(self.loss(res['flows_fw'], target))
        if self.loss_cfg.type == 'uflow_elbo':  # trainer/uflow_elbo_trainer.py: the model and the loss take the two frames
            res = self.model(model_in[:, :3], model_in[:, 3:], with_bk=True)
            out = self.loss(res, img_pair[:, :3], img_pair[:, 3:])
            return self._step(out)
        res = self.model(model_in, with_bk=True)
        if self.loss_cfg.type == 'mv':
            out = self.loss(res['flows_fw'], res['flows_bw'], img_pair)
        else:
            flows = [torch.cat([fw, bw], 1) for fw, bw in zip(res['flows_fw'], res['flows_bw'])]
            out = self.loss(flows, img_pair)
        if self.ar_cfg is not None:
            out = self._ar_pass(out, res, model_in)
        return self._step(out)

    def _ar_pass(self, out, res, model_in):
        """The second pass (arflow_amd.ar): the first pass's finest forward flow and, with mask_st and a loss that exposes one
        (unFlowLoss.pyramid_occu_mask1), its non-occlusion mask are moved through a drawn theta together with the model's
        input; the model runs again on the transformed frames without the backward direction and w_ar * ar_loss joins the
        first loss, so one backward serves both.  The targets carry no gradient."""
        from . import ar
        from .augment import _get
        cfg = self.ar_cfg
        flow = res['flows_fw'][0][:, :2].detach()
        B, _, H, W = (int(v) for v in model_in.shape)
        if tuple(flow.shape[-2:]) != (H, W):
            raise ValueError('the AR pass needs the finest flow at the input size %r (got %r)' % ((H, W), tuple(flow.shape[-2:])))
        noc = None
        masks = getattr(self.loss, 'pyramid_occu_mask1', None)
        if _get(cfg, 'mask_st', True) and masks:
            noc = masks[0].detach()
        theta = ar.draw_ar_params(_get(cfg, 'st_cfg', None), B, (H, W), self.ar_generator)
        img_t, flow_t, mask_t = ar.ar_transform(theta, img=model_in, flow=flow, noc=noc)
        pred = self.model(img_t, with_bk=False)['flows_fw'][0][:, :2]
        self.last_ar = ar.ar_loss(pred, flow_t, mask_t, eps=float(_get(cfg, 'ar_eps', 0.0)), q=float(_get(cfg, 'ar_q', 1.0)))
        total = out[0] + float(_get(cfg, 'w_ar', 0.0)) * self.last_ar.to(out[0].dtype)
        self.last_ar = self.last_ar.detach()
        return (total,) + tuple(out[1:])

    def _step(self, out):
        self.reducer.zero_grad()
        out[0].backward()
        self.reducer.finish()
        self.opt.step()
        self.last = out[0].detach()
        return self.last

    def save(self, path, epoch):
        """{'epoch', 'state_dict'} as trainer/base_trainer.py:155-156 writes them (utils/torch_utils.load_checkpoint reads the
        file), plus 'optimizer': the state of whichever optimiser the step holds."""
        torch.save({'epoch': int(epoch), 'state_dict': self.model.state_dict(), 'optimizer': self.opt.state_dict()}, path)

    def restore(self, path):
        """Load what save() wrote into the model and the optimiser, in place (parameter storage does not move) -> epoch."""
        ckpt = torch.load(path, map_location=next(self.model.parameters()).device)
        self.model.load_state_dict(ckpt['state_dict'])
        self.opt.load_state_dict(ckpt['optimizer'])
        return ckpt['epoch']
