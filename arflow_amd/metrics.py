"""Ground-truth flow metrics and the validation pass, and the uncertainty metrics on top of them
(DESIGN.md section 19): sparsification curves with their AUC, and the calibration curve.

The reference validates against ground truth after every epoch (trainer/uflow_trainer.py:94-170) with evaluate_flow
(utils/flow_utils.py:121-183): the full-resolution flow goes to the host, cv2.resize and numpy run per sample -- one device
synchronise and one device-to-host copy per batch.  Here one launch per batch (functional.flow_eval_sums) leaves eight sums
per sample on the device, the ratios are formed there, and the first host read is FlowMetrics.compute().
"""
import math

import torch

from . import functional as AF

NAMES_DENSE = ('EPE',)
NAMES_SPARSE = ('EPE', 'E_noc', 'E_occ', 'F1_all')
NAMES_MOVE = ('E_move', 'E_static')


def metric_names(sparse, with_move=False):
    """The order evaluate_flow returns (utils/flow_utils.py:177-183)."""
    if not sparse:
        return NAMES_DENSE
    return NAMES_SPARSE + (NAMES_MOVE if with_move else ())


def metrics_from_sums(sums, sparse, with_move=False):
    """sums [B,8] (columns of arflow_flow_eval: sum epe*valid, sum valid, sum epe*noc, sum noc, sum bad, sum epe*valid*move,
    sum valid*move, 0) -> the per-sample terms of evaluate_flow, [B,K] float64 in metric_names() order, with the
    reference's own arithmetic (utils/flow_utils.py:148-175): max(sum(valid - noc), 1.0) under E_occ, * 100 in F1_all, and
    NaN for a sample without valid pixels.  Pure torch: works on CPU tensors too."""
    s = sums.to(torch.float64)
    epe = s[:, 0] / s[:, 1]
    if not sparse:
        return epe[:, None]
    cols = [epe, s[:, 2] / s[:, 3], (s[:, 0] - s[:, 2]) / (s[:, 1] - s[:, 3]).clamp_min(1.0), s[:, 4] / s[:, 1] * 100.0]
    if with_move:
        cols += [s[:, 5] / s[:, 6], (s[:, 0] - s[:, 5]) / (s[:, 1] - s[:, 6])]
    return torch.stack(cols, 1)


class FlowMetrics:
    """Running mean of the per-sample metrics over a validation set (AverageMeter of trainer/uflow_trainer.py:115,133).
    State: one [K+1] float64 vector on the device -- the K metric totals and the sample count; update() only enqueues
    work, compute() is the first host read (after one all-reduce of that vector when torch.distributed is initialised)."""

    def __init__(self):
        self.names = None
        self.state = None

    def update_from_sums(self, sums, sparse, with_move=False):
        """Add a batch given its [B,8] sums (any device)."""
        names = metric_names(sparse, with_move)
        if self.names is None:
            self.names = names
            self.state = torch.zeros(len(names) + 1, device=sums.device, dtype=torch.float64)
        elif names != self.names:
            raise ValueError('FlowMetrics: batch yields %s, earlier batches %s' % (names, self.names))
        m = metrics_from_sums(sums, sparse, with_move)
        self.state += torch.cat([m.sum(0), m.new_full((1,), float(m.shape[0]))])

    def update(self, pred, gt, move=None):
        """pred [B,2,h,w], gt [B,2|4,H,W], move [B,1,H,W] or None: GPU tensors."""
        self.update_from_sums(AF.flow_eval_sums(pred, gt, move), gt.shape[1] == 4, move is not None)

    def compute(self):
        """-> {name: mean over all samples seen (on every rank)}."""
        if self.state is None:
            return {}
        state = self.state.clone()
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(state)
        vals = state.tolist()
        return {n: v / vals[-1] for n, v in zip(self.names, vals)}


# ---- uncertainty metrics ---------------------------------------------------------
def _linspace(start, stop, n):
    """np.linspace(start, stop, n) for every row of the float64 tensors start, stop [...]: arange(n) * step + start with
    the last point set to stop -- numpy's own arithmetic (torch.linspace fills from both ends and differs in the last bit)."""
    i = torch.arange(n, device=start.device, dtype=torch.float64)
    y = i * ((stop - start) / (n - 1))[..., None] + start[..., None]
    return torch.cat([y[..., :-1], stop[..., None]], -1)


def interp(x, xp, fp):
    """np.interp(x, xp, fp) along the last axis of float64 tensors of one leading shape, restated with torch ops: the
    interval is j = (number of xp <= x) - 1 (numpy's binary search on an ascending xp: with ties the LAST of the equal
    points), x below xp[0] gives fp[0], x at or above xp[-1] gives fp[-1], x equal to xp[j] gives fp[j] without forming a
    slope, otherwise slope * (x - xp[j]) + fp[j] with slope = (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]); a NaN from that
    (infinite fp) is retried from the right end of the interval, as numpy does."""
    n = xp.shape[-1]
    if n == 1:
        return torch.where(torch.isnan(x), x, fp.expand_as(x))
    xp, fp = xp.contiguous(), fp.contiguous()
    j = torch.searchsorted(xp, x.contiguous(), right=True) - 1
    jc = j.clamp(0, n - 2)
    x0, x1, y0, y1 = xp.gather(-1, jc), xp.gather(-1, jc + 1), fp.gather(-1, jc), fp.gather(-1, jc + 1)
    slope = (y1 - y0) / (x1 - x0)
    r = slope * (x - x0) + y0
    r2 = slope * (x - x1) + y1
    r = torch.where(torch.isnan(r), torch.where(torch.isnan(r2) & (y0 == y1), y0, r2), r)
    r = torch.where(x0 == x, y0, r)
    r = torch.where(j >= n - 1, fp[..., -1:].expand_as(r), r)
    r = torch.where(j < 0, fp[..., :1].expand_as(r), r)
    return torch.where(torch.isnan(x), x, r)


SP_REFINEMENTS = 10  # utils/flow_utils.py:209


def sp_curves(lo, hi, total, sums_fn, n=25, alpha=100.0, eps=1e-1):
    """sp_plot of utils/flow_utils.py:186-227 for a stack of curves.  lo, hi [...]: min and max of each curve's entropy
    field; total [...]: sum of the mask; sums_fn(thr [...,K] float64) -> [...,K,3]
    float64: sum (1-m) g, sum m g, sum err m g for m = expit(alpha (thr - field)).  -> (splot [...,n] float64, converged
    [...] bool, steps [...] int64: the refinements the reference would have run before its `break`, 10 if it never left).

    No host read unless expit(-alpha eps) > eps: the bracket is [lo - eps, hi + eps] in float64.  The reference widens it
    while the end fractions are further than eps from 1 and 0; they are within
    expit(-alpha eps) by construction, so with the defaults (4.5e-5 against 0.1) its loops cannot run.  Otherwise they are
    run here as the reference runs them, one K = 1 evaluation and ONE SCALAR READ per step.
    Always 1 + 10 evaluations: a curve that has met max|frac - grid_frac| <= eps keeps its grid and its sums from then on
    (torch.where), which is the reference's `break` without a branch on device data."""
    least = lo.double() - eps
    greatest = hi.double() + eps
    total = total.double()

    def frac_of(s):
        return s[..., 0] / total[..., None]

    if 1.0 / (1.0 + math.exp(alpha * eps)) > eps:
        for end, target in ((0, 1.0), (1, 0.0)):
            for _ in range(100000):
                thr = (least if end == 0 else greatest)[..., None]
                bad = (frac_of(sums_fn(thr))[..., 0] - target).abs() > eps
                if not bool(bad.any()):  # the scalar read
                    break
                step = 1e-3 * (greatest - least)
                if end == 0:
                    least = torch.where(bad, least - step, least)
                else:
                    greatest = torch.where(bad, greatest + step, greatest)
            else:
                raise RuntimeError('sp_plot: the threshold bracket did not reach fraction %g' % target)

    grid = _linspace(greatest, least, n)
    gf = _linspace(torch.zeros_like(least), torch.ones_like(least), n)
    s = sums_fn(grid)
    done = torch.zeros_like(least, dtype=torch.bool)
    steps = torch.zeros_like(least, dtype=torch.int64)
    for _ in range(SP_REFINEMENTS):
        done = done | ((frac_of(s) - gf).abs().amax(-1) <= eps)
        steps = steps + (~done).long()
        grid = torch.where(done[..., None], grid, interp(gf, frac_of(s), grid))
        s = torch.where(done[..., None, None], s, sums_fn(grid))
    frac = frac_of(s)
    converged = (frac - gf).abs().amax(-1) <= eps
    return interp(gf, frac, s[..., 2] / s[..., 1]), converged, steps


def _as_batch(t):
    return t[None] if t.dim() == 2 else t


def sp_plot(error, entropy, gt_mask, n=25, alpha=100.0, eps=1e-1, sums_fn=None, return_steps=False):
    """The sparsification curve of utils/flow_utils.py:186-227: error, entropy, gt_mask [B,H,W] (or [H,W], a batch of one)
    float32 -> (splot [B,n] float64, converged [B] bool), and the refinement count [B] as well if return_steps.  On GPU
    tensors every evaluation is one functional.sparsify_sums launch for the whole batch and nothing is read on the host
    (see sp_curves for the one exception); sums_fn(thr [B,1,K]) -> [B,1,K,3] replaces the kernel, so the refinement runs
    on CPU tensors too."""
    error, entropy, gt_mask = _as_batch(error), _as_batch(entropy), _as_batch(gt_mask)
    if sums_fn is None:
        err, ent, g = error[:, None], entropy[:, None], gt_mask[:, None]

        def sums_fn(thr):
            return AF.sparsify_sums(err, ent, None, g, thr, alpha)
    flat = entropy.flatten(1)
    out = sp_curves(flat.amin(1)[:, None], flat.amax(1)[:, None], gt_mask.double().sum((1, 2))[:, None], sums_fn, n, alpha,
                    eps)
    out = tuple(t[:, 0] for t in out)
    return out if return_steps else out[:2]


def _trapz_unit(y):
    """np.trapz(y, x=np.linspace(0, 1, n)) along the last axis: sum(diff(x) * (y[1:] + y[:-1]) / 2)."""
    x = _linspace(y.new_zeros(()), y.new_ones(()), y.shape[-1])
    return ((x[1:] - x[:-1]) * (y[..., 1:] + y[..., :-1]) / 2.0).sum(-1)


def auc_from_curves(splots):
    """[..., n] curves -> the area under splot / splot[0] over the uniform fraction grid (utils/flow_utils.py:316-318)."""
    return _trapz_unit(splots / splots[..., :1])


def evaluate_uncertainty(gt, pred, entropy, sp_samples=25):
    """evaluate_uncertainty of utils/flow_utils.py:281-320 on the device: gt [B,2|4,H,W], pred [B,2,h,w], entropy
    [B,2,h,w].  One flow_eval_sums(want_map=True), one uncert_prep, eleven sparsify_sums (both curves of every sample in
    each); nothing is read on the host.  -> dict of device tensors: 'AUC', 'AUC_diff' [B] (NaN for a sample without valid
    pixels; the reference returns their batch means), 'splots', 'oracle_splots' [B,n], 'converged' [B,2] bool and 'steps'
    [B,2] (entropy curve, oracle curve)."""
    _, epe_map = AF.flow_eval_sums(pred, gt, want_map=True)
    ent_map, stats = AF.uncert_prep(entropy, epe_map, gt)

    def sums_fn(thr):
        return AF.sparsify_sums(epe_map, ent_map, epe_map, gt, thr, 100.0)
    splots, converged, steps = sp_curves(stats[:, [0, 2]], stats[:, [1, 3]], stats[:, [4, 4]], sums_fn, sp_samples)
    auc = auc_from_curves(splots)
    return {'AUC': auc[:, 0], 'AUC_diff': auc[:, 0] - auc[:, 1], 'splots': splots[:, 0], 'oracle_splots': splots[:, 1],
            'converged': converged, 'steps': steps}


def _all_reduced(state):
    state = state.clone()
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.all_reduce(state)
    return state


class UncertaintyMetrics:
    """Running means of evaluate_uncertainty over a validation set (trainer/uflow_elbo_trainer.py:203-210, :286-295).
    State: one [2 + 2n + 2] float64 vector on the device -- the totals of AUC and AUC_diff, the two summed curves, the count
    of samples with a curve that did not converge (the reference prints a warning) and the sample count; update() only
    enqueues
    work, compute() is the first host read (after one all-reduce of that vector when torch.distributed is initialised)."""

    def __init__(self, sp_samples=25):
        self.n = sp_samples
        self.state = None

    def update_from_result(self, res):
        """Add a batch given evaluate_uncertainty()'s dict (any device)."""
        B = res['AUC'].shape[0]
        add = torch.cat([res['AUC'].sum()[None], res['AUC_diff'].sum()[None], res['splots'].sum(0),
                         res['oracle_splots'].sum(0), (~res['converged'].all(-1)).double().sum()[None],
                         res['AUC'].new_full((1,), float(B))])
        self.state = add if self.state is None else self.state + add

    def update(self, pred, gt, entropy):
        """pred, entropy [B,2,h,w], gt [B,2|4,H,W]: GPU tensors."""
        self.update_from_result(evaluate_uncertainty(gt, pred, entropy, self.n))

    def compute(self):
        """-> {'AUC', 'AUC_diff': means over all samples seen (on every rank), 'splot', 'oracle_splot': the mean curves as
        lists, 'not_converged': the number of samples with a curve that did not converge}."""
        if self.state is None:
            return {}
        v = _all_reduced(self.state).tolist()
        n, cnt = self.n, v[-1]
        return {'AUC': v[0] / cnt, 'AUC_diff': v[1] / cnt, 'splot': [x / cnt for x in v[2:2 + n]],
                'oracle_splot': [x / cnt for x in v[2 + n:2 + 2 * n]], 'not_converged': int(v[-2])}


class CalibrationCurve:
    """CalibrationCurve of utils/flow_utils.py:230-277: the per-channel errors |scaled pred - gt| of all samples pooled in
    the np.digitize bins of sigma = exp(entropy) over linspace(0, cc_max, cc_samples).  State: [cc_samples + 1, 3] float64
    on the device (count, sum, sum of squares per bin) instead of the reference's lists of every error; update() only
    enqueues work."""

    def __init__(self, cc_max=3.5, cc_samples=100):
        if not 2 <= cc_samples <= AF.CALIB_MAX_EDGES:
            raise ValueError('CalibrationCurve: cc_samples must be 2..%d' % AF.CALIB_MAX_EDGES)
        self.cc_max, self.cc_samples = cc_max, cc_samples
        self.state = None
        self._edges = None

    def edges(self, device):
        if self._edges is None or self._edges.device != torch.device(device):
            z = torch.zeros((), dtype=torch.float64)
            self._edges = _linspace(z, z + self.cc_max, self.cc_samples).to(device)
        return self._edges

    def update_from_sums(self, sums):
        """Add [cc_samples + 1, 3] bin sums (any device)."""
        if tuple(sums.shape) != (self.cc_samples + 1, 3):
            raise ValueError('CalibrationCurve: expected sums [%d,3]' % (self.cc_samples + 1))
        self.state = sums.double().clone() if self.state is None else self.state + sums

    def update(self, pred, gt, entropy):
        """pred, entropy [B,2,H,W] and gt [B,2|4,H,W] of ONE size (ValueError otherwise: the reference's boolean index
        only works then): GPU tensors."""
        self.update_from_sums(AF.calib_hist_sums(pred, gt, entropy, self.edges(pred.device)))

    def calibration_curve(self):
        """-> (vals, means, sigmas, numbers), four lists over the cc_samples + 1 bins as the reference returns them: the
        bin's nominal value (idx + 0.5) cc_max / (cc_samples - 1), the mean and the population standard deviation of its
        errors (NaN for an empty bin) and its count.  The first host read."""
        if self.state is None:
            s = torch.zeros(self.cc_samples + 1, 3, dtype=torch.float64)
        else:
            s = _all_reduced(self.state)
        cnt = s[:, 0]
        mean = s[:, 1] / cnt
        sigma = (s[:, 2] / cnt - mean * mean).clamp_min(0.0).sqrt()  # clamp_min keeps the NaN of an empty bin
        vals = [(i + 0.5) * self.cc_max / (self.cc_samples - 1) for i in range(self.cc_samples + 1)]
        return vals, mean.tolist(), sigma.tolist(), [int(c) for c in cnt.tolist()]


@torch.no_grad()
def validate(model, batches, entropy_of=None):
    """trainer/uflow_trainer.py:116-133 without the loss call and the tensorboard images: eval mode, no_grad,
    model(img_pair), score res['flows_fw'][0].  batches yields (img_pair, gt) or (img_pair, gt, move).  The model's
    training mode is restored.  -> FlowMetrics.compute().
    entropy_of: None, or a function res_dict -> entropy [B,2,h,w] of the scored flow (trainer/uflow_elbo_trainer.py:183-189
    takes it from inverse_diagonal); the result then gains UncertaintyMetrics.compute()'s entries (:203-210, :286-295)."""
    was_training = model.training
    model.eval()
    meter = FlowMetrics()
    umeter = UncertaintyMetrics() if entropy_of is not None else None
    try:
        for batch in batches:
            img_pair, gt = batch[0], batch[1]
            move = batch[2] if len(batch) > 2 else None
            res = model(img_pair)
            meter.update(res['flows_fw'][0], gt, move)
            if umeter is not None:
                umeter.update(res['flows_fw'][0], gt, entropy_of(res))
    finally:
        model.train(was_training)
    out = meter.compute()
    if umeter is not None:
        out.update(umeter.compute())
    return out
