#!/usr/bin/env python3
"""Two- / three-frame inference CLI with the contract the reference's README documents
(README.md:32-50:  inference.py -m <ckpt> -s 384 640 -i img1 img2 [img0 img1 img2]); the fork's own
inference.py only drives its probabilistic models.

    python -m arflow_amd.inference -s 384 640 -i a.png b.png [-m ckpt.pth.tar] [-o flow.flo] [--arch pwclite|pwclite_prob|pwclite_uflow|uflow|uflow_prob]
                                [--columns R] [--entropy-out ent.npy] [--orig-size] [--vis-out flow.ppm] [--vis-mode rgb|wheel]
                                [--entropy-vis ent.pgm]

Runs on the GPU through the HIP kernels.  Without -m the network is seeded-random (no checkpoint ships
with the reference: .MISSING_LARGE_BLOBS), which still exercises the whole path.  --arch uflow_prob is PWCProbFlow with
out_channels [2, 2, 0]; --entropy-out writes its full-resolution log-diagonal channels flows_fw[0][:, 2:4] as [H,W,2] -- what
the reference's ELBO trainer evaluates as the per-component entropy for `diag`, and for `sparse` without inv_cov
(trainer/uflow_elbo_trainer.py:175,191), and what `python -m arflow_amd.evaluate --entropy` reads.  With --columns R the model
is the low-rank family's (out_channels [2, 0, 2R], configs/chairs_uflow_elbo_lowrank.json) and --entropy-out writes the map
the reference's inference and validation compute for it (inference.py:76-84, trainer/uflow_elbo_trainer.py:193-197):
upsample(log(sum_k std_k^2) / 2 + 2 log 4, x4, align_corners=False) of the level-2 columns, in plain torch.  --arch pwclite_prob is
PWCLiteProb (upsample, reduce_dense); its channels 2:4 are the log VARIANCE, so --entropy-out writes flows_fw[0][:, 2:4] / 2,
the log standard deviation `evaluate --entropy` reads.

--orig-size restores the flow and --entropy-out to the FIRST image's own size (arflow_amd.render.restore: inference.py:98-107);
--vis-out writes the flow picture (--vis-mode rgb: np_flow2rgb by the flow's max |f|; wheel: flow_to_image, max_flow 256) and
--entropy-vis the entropy picture, .ppm / .pgm / .png by extension.  These four take two frames and go through
arflow_amd.predict.run; without them the output is what it always was.
"""
import argparse
import math

import numpy as np
import torch

from .config import AttrDict
from .flow_io import write_flow
from .models import PWCLiteProb, get_model


def load_image(path, size):
    from PIL import Image
    img = Image.open(path).convert('RGB')
    if size is not None:
        img = img.resize((size[1], size[0]), Image.BILINEAR)
    return torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1)


def build_model(kind, n_frames, ckpt=None, seed=0, columns=0):
    if kind == 'pwclite':
        cfg = AttrDict(type='pwclite', upsample=True, n_frames=n_frames, reduce_dense=True)
    elif kind == 'pwclite_prob':
        if n_frames != 2:
            raise ValueError('PWCLiteProb takes two frames')
        cfg = AttrDict(type='pwclite_prob', upsample=True, n_frames=2, reduce_dense=True)
    elif kind == 'pwclite_uflow':
        cfg = AttrDict(type='pwclite_uflow', level_dropout=0.0, feature_norm=True, align_corners=True, warp_pad='zeros',
                       n_frames=2, reduce_dense=False)
    elif kind == 'uflow':
        cfg = AttrDict(type='uflow', level_dropout=0.0, feature_norm=True)
    elif kind == 'uflow_prob':
        cfg = AttrDict(type='uflow_prob', level_dropout=0.0, feature_norm=True,
                       out_channels=[2, 0, 2 * columns] if columns else [2, 2, 0], inv_cov=False, n_pyramids=1,
                       mixture_weights=False)
    else:
        raise NotImplementedError(kind)
    model = get_model(cfg)
    if ckpt:
        load_state(model, ckpt)
    else:
        torch.manual_seed(seed)
        model.init_weights()
    return model.eval()


def load_state(model, ckpt):
    # same container as utils/torch_utils.py:39-51: {'epoch':..., 'state_dict':...}; tensors only
    blob = torch.load(ckpt, map_location='cpu', weights_only=True)
    state = blob.get('state_dict', blob)
    model.load_state_dict({k.replace('module.', '', 1): v for k, v in state.items()})


@torch.no_grad()
def infer(model, frames, device, want_entropy=False):
    """frames: list of [3,H,W] tensors in [0,1] -> forward flow of the (middle) reference frame, [H,W,2]; with want_entropy
    (PWCProbFlow only) also its log-diagonal channels -- for the low-rank family (no log-diagonal channels) the entropy map of
    lowrank_entropy_map --, [H,W,2]."""
    x = torch.cat(frames, 0).unsqueeze(0).to(device)
    prob = hasattr(model, 'upsample_out')
    lite_prob = isinstance(model, PWCLiteProb)  # (flow, log-variance) outputs
    if want_entropy and not (prob or lite_prob):
        raise ValueError('only the probabilistic models (--arch uflow_prob, pwclite_prob) have an entropy output')
    if lite_prob and len(frames) != 2:
        raise ValueError('PWCLiteProb takes two frames')
    if prob:
        if len(frames) != 2:
            raise ValueError('PWCProbFlow takes two frames')
        res = model(x[:, :3], x[:, 3:], with_bk=False)
    else:
        res = model(x, with_bk=False) if len(frames) == 2 else model(x)
    out = res['flows_fw'][0][0].permute(1, 2, 0).float().cpu().numpy()
    if lite_prob:
        return (out[..., 0:2], out[..., 2:4] / 2) if want_entropy else out[..., 0:2]
    if want_entropy:
        if model._out_channels[1] == 0:
            ent = lowrank_entropy_map(res['flows_fw'][2][:, 2:])
            return out[..., 0:2], ent[0].permute(1, 2, 0).float().cpu().numpy()
        return out[..., 0:2], out[..., 2:4]
    return out[..., 0:2]


def lowrank_entropy_map(std):
    """std [B,2R,h,w], the level-2 columns (channel 2k + c: column k of flow component c) -> [B,2,4h,4w]: the marginal
    log standard deviation log(sum_k std_k^2) / 2 per component, brought to full resolution (inference.py:76-84)."""
    ent = torch.log(torch.stack((std[:, 0::2].square().sum(1), std[:, 1::2].square().sum(1)), 1)) / 2
    return torch.nn.functional.interpolate(ent + 2 * math.log(4), scale_factor=4, mode='bilinear', align_corners=False)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('-m', '--model', default=None, help='checkpoint (.pth.tar with state_dict)')
    ap.add_argument('-s', '--test_shape', default=[384, 640], type=int, nargs=2)
    ap.add_argument('-i', '--img_list', nargs='+', required=True)
    ap.add_argument('-o', '--output', default=None, help='write the flow as .flo')
    ap.add_argument('--arch', default='pwclite', choices=['pwclite', 'pwclite_prob', 'pwclite_uflow', 'uflow', 'uflow_prob'])
    ap.add_argument('--columns', default=0, type=int, help='uflow_prob: the low-rank family with this many columns (1..16)')
    ap.add_argument('--entropy-out', default=None, help='write the log standard deviation as .npy [H,W,2] (uflow_prob, pwclite_prob)')
    ap.add_argument('--orig-size', action='store_true', help="restore the flow and --entropy-out to the first image's own size")
    ap.add_argument('--vis-out', default=None, help='write the flow picture (.ppm or .png)')
    ap.add_argument('--vis-mode', default='rgb', choices=['rgb', 'wheel'])
    ap.add_argument('--entropy-vis', default=None, help='write the entropy picture (.pgm or .png)')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('arflow_amd.inference needs a GPU: the correlation / warp kernels have no CPU fallback')
    device = torch.device('cuda')
    frames = [load_image(p, args.test_shape) for p in args.img_list]
    if args.columns and (args.arch != 'uflow_prob' or not 1 <= args.columns <= 16):
        raise SystemExit('--columns takes 1..16 and needs --arch uflow_prob')
    model = build_model(args.arch, len(frames), args.model, columns=args.columns).to(device)
    if args.orig_size or args.vis_out or args.entropy_vis:
        flow = _restored(args, model, frames, device)
    elif args.entropy_out:
        flow, ent = infer(model, frames, device, want_entropy=True)
        np.save(args.entropy_out, np.ascontiguousarray(ent))
    else:
        flow = infer(model, frames, device)
    print('flow %s  mean |u|=%.4f |v|=%.4f' % (flow.shape, np.abs(flow[..., 0]).mean(), np.abs(flow[..., 1]).mean()))
    if args.output:
        write_flow(args.output, flow)


def _restored(args, model, frames, device):
    """The path of --orig-size / --vis-out / --entropy-vis: one arflow_amd.predict.run over the single pair -> the flow."""
    from . import predict
    from .flow_io import write_image
    if len(frames) != 2:
        raise SystemExit('--orig-size, --vis-out and --entropy-vis take two frames')
    rule = predict.entropy_rule(args.arch, columns=args.columns) if args.entropy_out or args.entropy_vis else None
    if (args.entropy_out or args.entropy_vis) and rule is None:
        raise SystemExit('only the probabilistic models (--arch uflow_prob, pwclite_prob) have an entropy output')
    out_hw = tuple(args.test_shape)
    if args.orig_size:
        from PIL import Image
        with Image.open(args.img_list[0]) as im:
            out_hw = (im.size[1], im.size[0])
    got = {}
    predict.run(model, [(['pair'], frames[0][None].to(device), frames[1][None].to(device))], lambda key: out_hw,
                lambda key, kind, a: got.__setitem__(kind, a), rule, args.vis_mode if args.vis_out else None,
                bool(args.entropy_vis))
    if args.entropy_out:
        np.save(args.entropy_out, np.ascontiguousarray(got['entropy']))
    if args.vis_out:
        write_image(args.vis_out, got['vis'])
    if args.entropy_vis:
        write_image(args.entropy_vis, got['entropy_vis'])
    return got['flow']


if __name__ == '__main__':
    main()
