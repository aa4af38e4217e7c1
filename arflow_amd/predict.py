#!/usr/bin/env python3
"""Directory inference: the reference's inference.py (TestHelper.run, inference.py:34-119) as a GPU pipeline.

    python -m arflow_amd.predict --frames DIR | --pairs FILE  --out DIR  [-s H W] [--batch N] [-m ckpt]
                                 [--arch ... [--columns R] | -c config.json]
                                 [--vis rgb|wheel] [--entropy-vis] [--ext ppm|png]

Consecutive sorted frames of DIR form the pairs (or FILE names two paths per line).  Pairs are grouped by the ORIGINAL size
of their first frame into batches of at most N; every batch is one model call at the test size, one arflow_amd.render.restore
to the original size and one device-to-host copy per output kind.  Written per pair, named after its first frame:
    <stem>.flo           the flow [H,W,2] at the frame's own size
    <stem>.npy           the entropy [H,W,2] (log standard deviation per component), probabilistic models only
    <stem>.ppm           --vis: the flow picture (rgb: np_flow2rgb by the sample's max |f|; wheel: flow_to_image, max_flow 256)
    <stem>_entropy.pgm   --entropy-vis: the summed entropy, scaled to the sample's own minimum and maximum
which is what `python -m arflow_amd.evaluate --pred OUT --gt ... --entropy OUT` reads.

The entropy per family, as inference.py:55-84: `diag`, and `sparse` without inv_cov: channels 2:4 of flows_fw[0];
PWCLiteProb (log VARIANCE): the same channels divided by 2; `lowrank`: arflow_amd.inference.lowrank_entropy_map of the level-2
columns.  Refused: `mixture` / ComponentNet (the reference calls mixture_entropy without its `weights` argument and restores two
channels of a one-channel map: there is nothing to mirror) and `sparse` with inv_cov (the loss that would train it raises in
the reference and here).  The entropy picture is normalised per SAMPLE, not per batch as the trainer's, so a picture does
not depend on which frames shared its batch.
"""
import argparse
import os

import numpy as np
import torch

from . import render
from .config import AttrDict, load_json
from .flow_io import write_flow, write_image
from .inference import build_model, load_image, load_state, lowrank_entropy_map
from .models import PWCLiteProb, get_model

ARCHS = ['pwclite', 'pwclite_prob', 'pwclite_uflow', 'uflow', 'uflow_prob']
IMAGE_EXT = ('.png', '.jpg', '.jpeg', '.ppm', '.bmp')


# ---- pairing and grouping (file names only) ------------------------------------------------------------------------------
def pairs_from_frames(names):
    """Consecutive sorted frames -> [(first, second), ...]."""
    names = sorted(names)
    return list(zip(names[:-1], names[1:]))


def pairs_from_file(path):
    pairs = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if not parts or parts[0].startswith('#'):
                continue
            if len(parts) != 2:
                raise ValueError('%s:%d: two paths per line (got %d)' % (path, n, len(parts)))
            pairs.append((parts[0], parts[1]))
    return pairs


def stem_of(path):
    return os.path.splitext(os.path.basename(path))[0]


def group_by_size(pairs, size_of, batch):
    """Pairs grouped by size_of(first frame) = (H, W) into lists of at most `batch`, each pair once; groups in the order
    their first pair appears, pairs in their own order.  Two pairs with the same stem would write the same files: refused."""
    if batch < 1:
        raise ValueError('batch must be >= 1 (got %r)' % (batch,))
    stems = [stem_of(a) for a, _ in pairs]
    if len(set(stems)) != len(stems):
        raise ValueError('two pairs share the output name %r' % sorted(s for s in set(stems) if stems.count(s) > 1)[0])
    by_size = {}
    for p in pairs:
        by_size.setdefault(tuple(size_of(p[0])), []).append(p)
    return [(hw, group[i:i + batch]) for hw, group in by_size.items() for i in range(0, len(group), batch)]


# ---- the entropy rule ------------------------------------------------------------------------------------------------------
def entropy_rule(model_type, approx=None, inv_cov=False, columns=0):
    """-> None (no entropy output), 'channels', 'half' or 'lowrank'; raises ValueError for what is refused."""
    if model_type == 'component' or approx == 'mixture':
        raise ValueError("the mixture family (approx 'mixture', model type 'component') has no directory inference: the "
                         "reference calls mixture_entropy without its weights argument and restores two channels of a "
                         "one-channel map, so there is nothing to mirror")
    if approx == 'sparse' and inv_cov:
        raise ValueError("approx 'sparse' with inv_cov has no directory inference: the loss that would train it raises in the "
                         "reference and here")
    if model_type == 'pwclite_prob':
        return 'half'
    if model_type != 'uflow_prob':
        return None
    if approx == 'lowrank' or columns:
        return 'lowrank'
    if approx in (None, 'diag', 'sparse'):
        return 'channels'
    raise NotImplementedError('Invalid approximation %r' % (approx,))


def model_from_config(cfg, ckpt=None, seed=0):
    """cfg: the reference's JSON layout (`model`, `loss`) -> (model in eval mode, entropy rule)."""
    loss = cfg.get('loss', AttrDict())
    rule = entropy_rule(cfg.model.type, loss.get('approx'), bool(loss.get('inv_cov', False)), int(loss.get('columns', 0) or 0))
    model = get_model(cfg.model)
    if ckpt:
        load_state(model, ckpt)
    else:
        torch.manual_seed(seed)
        model.init_weights()
    return model.eval(), rule


# ---- the core --------------------------------------------------------------------------------------------------------------
def forward(model, img1, img2):
    """One model call on [n,3,h,w] frames -> flows_fw."""
    if hasattr(model, 'upsample_out'):
        return model(img1, img2, with_bk=False)['flows_fw']
    return model(torch.cat((img1, img2), 1), with_bk=False)['flows_fw']


def entropy_of(flows, rule):
    """[n,2,h,w] at the test size, a channel slice where the family allows it."""
    if rule == 'channels':
        return flows[0][:, 2:4]
    if rule == 'half':
        return flows[0][:, 2:4] / 2
    if rule == 'lowrank':
        return lowrank_entropy_map(flows[2][:, 2:])
    raise ValueError('unknown entropy rule %r' % (rule,))


@torch.no_grad()
def run(model, batches, out_hw_of, sink, rule=None, vis=None, entropy_vis=False):
    """batches: iterable of (keys, img1 [n,3,h,w], img2 [n,3,h,w]) on the GPU, every key of a batch with the same
    out_hw_of(key) = (H, W).  sink(key, kind, array) receives numpy arrays: kind 'flow' [H,W,2] float32, 'entropy' [H,W,2]
    float32 (rule given), 'vis' [H,W,3] uint8 (vis 'rgb' or 'wheel'), 'entropy_vis' [H,W] uint8.  -> number of pairs."""
    if entropy_vis and rule is None:
        raise ValueError('only the probabilistic models have an entropy picture')
    done = 0
    for keys, img1, img2 in batches:
        sizes = {tuple(out_hw_of(k)) for k in keys}
        if len(sizes) != 1 or len(keys) != img1.shape[0]:
            raise ValueError('a batch holds %d frames and keys of sizes %s' % (img1.shape[0], sorted(sizes)))
        flows = forward(model, img1, img2)
        ent = entropy_of(flows, rule) if rule else None
        r = render.restore(flows[0][:, 0:2], sizes.pop(), ent, stats=vis is not None)
        outs = {'flow': r.flow}
        if ent is not None:
            outs['entropy'] = r.entropy
        if vis:
            outs['vis'] = render.flow_rgb(r.flow, vis, layout='nhwc', stats=r.stats)
        if entropy_vis:
            planes = r.entropy.permute(0, 3, 1, 2).contiguous()
            outs['entropy_vis'] = torch.cat([render.entropy_image(planes[b:b + 1]) for b in range(len(keys))])
        for kind, t in outs.items():
            host = t.cpu().numpy()
            for b, k in enumerate(keys):
                sink(k, kind, host[b])
        done += len(keys)
    return done


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
def file_sink(out_dir, ext):
    def sink(key, kind, a):
        stem = os.path.join(out_dir, stem_of(key))
        if kind == 'flow':
            write_flow(stem + '.flo', a)
        elif kind == 'entropy':
            np.save(stem + '.npy', np.ascontiguousarray(a))
        elif kind == 'vis':
            write_image(stem + ('.ppm' if ext == 'ppm' else '.png'), a)
        else:
            write_image(stem + '_entropy' + ('.pgm' if ext == 'ppm' else '.png'), a)
    return sink


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--frames', help='directory of frames; consecutive sorted frames form the pairs')
    src.add_argument('--pairs', help='text file with two image paths per line')
    ap.add_argument('--out', required=True, help='output directory')
    ap.add_argument('-s', '--test_shape', default=[384, 640], type=int, nargs=2)
    ap.add_argument('--batch', default=4, type=int)
    ap.add_argument('-m', '--model', default=None, help='checkpoint (.pth.tar with state_dict)')
    ap.add_argument('--arch', default=None, choices=ARCHS)
    ap.add_argument('--columns', default=0, type=int, help='uflow_prob: the low-rank family with this many columns (1..16)')
    ap.add_argument('-c', '--config', default=None, help="the reference's JSON config: its `model` and `loss` sections are read")
    ap.add_argument('--vis', default=None, choices=['rgb', 'wheel'])
    ap.add_argument('--entropy-vis', action='store_true')
    ap.add_argument('--ext', default='ppm', choices=['ppm', 'png'])
    args = ap.parse_args(argv)
    if args.config and args.arch:
        raise SystemExit('give --arch or -c, not both')
    if args.columns and (args.arch != 'uflow_prob' or not 1 <= args.columns <= 16):
        raise SystemExit('--columns takes 1..16 and needs --arch uflow_prob')
    if not torch.cuda.is_available():
        raise SystemExit('arflow_amd.predict needs a GPU: the kernels have no CPU fallback')
    device = torch.device('cuda')
    try:
        if args.config:
            model, rule = model_from_config(load_json(args.config), args.model)
        else:
            arch = args.arch or 'pwclite'
            rule = entropy_rule(arch, columns=args.columns)
            model = build_model(arch, 2, args.model, columns=args.columns)
    except ValueError as e:
        raise SystemExit(str(e))
    model = model.to(device)
    if args.entropy_vis and rule is None:
        raise SystemExit('--entropy-vis needs a probabilistic model')
    if args.frames:
        names = [os.path.join(args.frames, n) for n in os.listdir(args.frames) if n.lower().endswith(IMAGE_EXT)]
        pairs = pairs_from_frames(names)
    else:
        pairs = pairs_from_file(args.pairs)
    if not pairs:
        raise SystemExit('no pairs: a directory needs at least two frames')
    from PIL import Image
    size = {}

    def size_of(path):
        if path not in size:
            with Image.open(path) as im:
                size[path] = (im.size[1], im.size[0])
        return size[path]
    os.makedirs(args.out, exist_ok=True)
    groups = group_by_size(pairs, size_of, args.batch)

    def batches():
        for _, group in groups:
            img1 = torch.stack([load_image(a, args.test_shape) for a, _ in group]).to(device)
            img2 = torch.stack([load_image(b, args.test_shape) for _, b in group]).to(device)
            yield [a for a, _ in group], img1, img2
    n = run(model, batches(), size_of, file_sink(args.out, args.ext), rule, args.vis, args.entropy_vis)
    print('%d pairs in %d batches -> %s' % (n, len(groups), args.out))


if __name__ == '__main__':
    main()
