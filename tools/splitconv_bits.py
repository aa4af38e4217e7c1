#!/usr/bin/env python
"""Bit fingerprints of the split-bf16 convolution kernels (csrc/splitconv.hip, csrc/splitconv_wgrad.hip; DESIGN.md section
32): for every case the inputs come from a CPU generator seeded by the case's own parameters, the raw C-ABI calls run once,
and every output is fingerprinted by the first 12 hex digits of the sha256 of its bytes.  One line per case:

    fwd C=33,K=64,6x20 PW=32  y=<hash> dx=<hash> slot_bias=<hash> slot_nobias=<hash>
    wgrad 1x33x64x5x160  dw=<hash> dw_slice=<hash>

y: the forward x [N,C,H,W] -> [N,K,H,W]; dx: the transpose_flip call (a data gradient: the weights are [C,K,3,3]) on the same
x; slot_*: arflow_splitconv_fwd_ex reading the channel slice x6[:, K:K+C] and writing lrelu(conv + bias, 0.1) into the slot
x6[:, :K] of the same tensor, with and without a bias -- the WHOLE of x6 (one spare channel behind the slice included) is
hashed, so a write outside the slot shows.  dw: the weight gradient of contiguous x and dy; dw_slice: x read as a channel
slice of a tensor one channel wider.

Two builds compute the same thing iff their outputs of this tool are equal line for line:

    python tools/splitconv_bits.py > after.txt
    python tools/splitconv_bits.py --root <checkout of another commit, built> > parent.txt

Cases: the smallest that reach every edge of the operand pipeline.  Forward: C in {1, 32, 33, 70} (one block of 32 input
channels: the prologue's request is also the last; a block and a one-channel tail; three blocks), K in {1, 33, 64, 96} (one
tile; two; two; a chunk of two and a chunk of one), N = 2, and five maps.  5x7, 6x20 and 3x40 all select the 32 x 1 pixel
tile by the host's rule (pixel_tile below restates it), so 9x13 (16 x 2) and 17x7 (8 x 4) are there as well.  Weight
gradient: 2x3x2x5x7, 1x17x33x13x21, 3x40x96x9x35, 1x33x64x5x160 (three strips, the last with two steps) and 1x8x40x6x24
(three groups: a half-empty step).

--cases retile: a second list for the 4 x 1 wave tile of the KT = 2 launches, recorded in
tests/golden/splitconv_retile_bits.txt: K in {40, 65, 160} (a partly filled second tile of a wave pair; chunks of 2 + 1 and
2 + 2 + 1 tiles with their first-tile offsets), C in {64, 70}, N = 2, and the maps 8x32 (all eight 32 x 1 tiles live), 4x33
(pixel tiles 4..7, the four of waves 1 and 3, wholly outside the map; two tiles across) and 9x13 (16 x 2).
"""
import argparse
import hashlib
import os
import sys

import torch

CS = (1, 32, 33, 70)
KS = (1, 33, 64, 96)
N_FWD = 2
MAPS = ((5, 7), (6, 20), (3, 40), (9, 13), (17, 7))
WGRAD_CASES = ((2, 3, 2, 5, 7), (1, 17, 33, 13, 21), (3, 40, 96, 9, 35), (1, 33, 64, 5, 160), (1, 8, 40, 6, 24))
RETILE_CS = (64, 70)
RETILE_KS = (40, 65, 160)
RETILE_MAPS = ((8, 32), (4, 33), (9, 13))
SLOPE = 0.1
NAN_BITS = 0x7FC07FC0  # a NaN as float32 and as two bf16


def pixel_tile(H, W):
    """The pixel tile's width arflow_splitconv_fwd_ex chooses: 32 x 1, else 16 x 2 or 8 x 4 where that pads fewer pixels."""
    def waste(pw):
        th = 8 * (32 // pw)
        return -(-W // pw) * pw * (-(-H // th) * th)
    PW = 32
    if waste(16) < waste(PW):
        PW = 16
    if waste(8) < waste(PW):
        PW = 8
    return PW


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:12]


def embed(t, fill_bits, pad=4096, dtype=torch.float32):
    """A copy of the CPU tensor t on the device in the middle of a larger allocation whose other elements (pad 4-byte words
    on either side) hold fill_bits; -> (view, whole buffer)."""
    words = t.numel() * t.element_size() // 4
    buf = torch.full((words + 2 * pad,), fill_bits, dtype=torch.int32, device='cuda:0')
    view = buf[pad:pad + words].view(dtype).view(t.shape)
    view.copy_(t)
    return view, buf


class Runner:
    """The raw calls, through the package found under `root`."""

    def __init__(self, root):
        sys.path.insert(0, os.path.abspath(root))
        from arflow_amd import _lib
        from arflow_amd.functional import _call, _p, _stream
        self.lib, self.check, self.call, self.p, self.stream = _lib.load(), _lib.check, _call, _p, _stream
        self.dev = torch.device('cuda:0')

    def pack_bytes(self, K, C):
        n = self.lib.arflow_splitconv_pack_bytes(K, C)
        self.check(min(n, 0), 'arflow_splitconv_pack_bytes')
        return n

    def fwd(self, x, w, tf, y, bias=None, act=0, packed=None):
        """x, y: [N,*,H,W] views with dense planes; w: [K,C,3,3], or [C,K,3,3] with tf; packed: a uint8 view or None."""
        N, C, H, W = x.shape
        K = y.shape[1]
        if packed is None:
            packed = torch.empty(self.pack_bytes(K, C), device=self.dev, dtype=torch.uint8)
        self.call('arflow_splitconv_pack', self.p(w), self.p(packed), int(w.shape[0]), int(w.shape[1]), int(tf), self.stream())
        self.call('arflow_splitconv_fwd_ex', self.p(x), x.stride(0), self.p(packed), self.p(y), y.stride(0), self.p(bias), int(act),
                  SLOPE if act else 0.0, N, C, K, H, W, self.stream())
        return y

    def ws_bytes(self, N, C, K, H, W):
        n = self.lib.arflow_splitconv_wgrad_ws_bytes(N, C, K, H, W)
        self.check(min(n, 0), 'arflow_splitconv_wgrad_ws_bytes')
        return n

    def wgrad(self, x, dy, ws=None):
        N, C, H, W = x.shape
        K = dy.shape[1]
        if ws is None:
            ws = torch.empty(self.ws_bytes(N, C, K, H, W), device=self.dev, dtype=torch.uint8)
        dw = torch.empty(K, C, 3, 3, device=self.dev)
        self.call('arflow_splitconv_wgrad', self.p(x), x.stride(0), self.p(dy), dy.stride(0), self.p(dw), self.p(ws), N, C, K, H, W,
                  self.stream())
        return dw


def fwd_inputs(C, K, H, W):
    """CPU inputs of a forward case: x, w [K,C,3,3], w' [C,K,3,3] for the transpose_flip call, bias [K]."""
    g = torch.Generator().manual_seed(((C * 131 + K) * 131 + H) * 131 + W)
    x = torch.randn(N_FWD, C, H, W, generator=g)
    w = 0.2 * torch.randn(K, C, 3, 3, generator=g)
    wt = 0.2 * torch.randn(C, K, 3, 3, generator=g)
    bias = torch.randn(K, generator=g)
    return x, w, wt, bias


def wgrad_inputs(N, C, K, H, W):
    g = torch.Generator().manual_seed((((N * 131 + C) * 131 + K) * 131 + H) * 131 + W + 7)
    return torch.randn(N, C, H, W, generator=g), torch.randn(N, K, H, W, generator=g)


def fwd_case(run, C, K, H, W):
    """-> {'y': hash, 'dx': hash, 'slot_bias': hash, 'slot_nobias': hash}"""
    x, w, wt, bias = fwd_inputs(C, K, H, W)
    xd, wd, wtd, bd = (t.to(run.dev) for t in (x, w, wt, bias))
    out = {}
    out['y'] = digest(run.fwd(xd, wd, 0, torch.zeros(N_FWD, K, H, W, device=run.dev)))
    out['dx'] = digest(run.fwd(xd, wtd, 1, torch.zeros(N_FWD, K, H, W, device=run.dev)))
    for key, b in (('slot_bias', bd), ('slot_nobias', None)):
        x6 = torch.zeros(N_FWD, K + C + 1, H, W, device=run.dev)
        x6[:, K:K + C].copy_(xd)
        run.fwd(x6[:, K:K + C], wd, 0, x6[:, :K], bias=b, act=1)
        out[key] = digest(x6)
    torch.cuda.synchronize()
    return out


def wgrad_case(run, N, C, K, H, W):
    x, dy = wgrad_inputs(N, C, K, H, W)
    xd, dyd = x.to(run.dev), dy.to(run.dev)
    wide = torch.zeros(N, C + 1, H, W, device=run.dev)
    wide[:, 1:].copy_(xd)
    out = {'dw': digest(run.wgrad(xd, dyd)), 'dw_slice': digest(run.wgrad(wide[:, 1:], dyd))}
    torch.cuda.synchronize()
    return out


def fwd_head(C, K, H, W):
    return 'fwd C=%d,K=%d,%dx%d PW=%d' % (C, K, H, W, pixel_tile(H, W))


def wgrad_head(N, C, K, H, W):
    return 'wgrad %dx%dx%dx%dx%d' % (N, C, K, H, W)


def fmt(head, hashes):
    return head + ' ' + ''.join(' %s=%s' % kv for kv in hashes.items())


FLAGSHIP_LAYERS = ((147, 128), (275, 128), (403, 96), (499, 64), (563, 32), (597, 128), (64, 32))
FLAGSHIP_MAPS = ((96, 160), (48, 80))


def flagship_lines(run, N=16):
    """The wide layers at the sizes and batch of the flagship step (not in the golden file: too slow for a test)."""
    for H, W in FLAGSHIP_MAPS:
        for C, K in FLAGSHIP_LAYERS:
            g = torch.Generator().manual_seed(C * 1009 + K + H)
            x, gy = torch.randn(N, C, H, W, generator=g).to(run.dev), torch.randn(N, K, H, W, generator=g).to(run.dev)
            w, bias = (0.05 * torch.randn(K, C, 3, 3, generator=g)).to(run.dev), torch.randn(K, generator=g).to(run.dev)
            out = {'y': digest(run.fwd(x, w, 0, torch.zeros(N, K, H, W, device=run.dev))),
                   'dx': digest(run.fwd(gy, w, 1, torch.zeros(N, C, H, W, device=run.dev)))}
            x6 = torch.zeros(N, K + C, H, W, device=run.dev)
            x6[:, K:].copy_(x)
            run.fwd(x6[:, K:], w, 0, x6[:, :K], bias=bias, act=1)
            out['slot_bias'] = digest(x6[:, :K])
            out['dw'] = digest(run.wgrad(x, gy))
            yield fmt('flagship %dx%dx%dx%dx%d' % (N, C, K, H, W), out)


def all_lines(run):
    for H, W in MAPS:
        for C in CS:
            for K in KS:
                yield fmt(fwd_head(C, K, H, W), fwd_case(run, C, K, H, W))
    for case in WGRAD_CASES:
        yield fmt(wgrad_head(*case), wgrad_case(run, *case))


def retile_lines(run):
    for H, W in RETILE_MAPS:
        for C in RETILE_CS:
            for K in RETILE_KS:
                yield fmt(fwd_head(C, K, H, W), fwd_case(run, C, K, H, W))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--flagship', action='store_true', help='the flagship step\'s layers at 16x96x160 and 16x48x80 instead of the cases')
    ap.add_argument('--cases', choices=('default', 'retile'), default='default', help='which case list (see the module docstring)')
    args = ap.parse_args()
    run = Runner(args.root)
    for line in (flagship_lines(run) if args.flagship else retile_lines(run) if args.cases == 'retile' else all_lines(run)):
        print(line, flush=True)
