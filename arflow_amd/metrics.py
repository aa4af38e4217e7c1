"""Ground-truth flow metrics and the validation pass.

The reference validates against ground truth after every epoch (trainer/uflow_trainer.py:94-170) with evaluate_flow
(utils/flow_utils.py:121-183): the full-resolution flow goes to the host, cv2.resize and numpy run per sample -- one device
synchronise and one device-to-host copy per batch.  Here one launch per batch (functional.flow_eval_sums) leaves eight sums
per sample on the device, the ratios are formed there, and the first host read is FlowMetrics.compute().
"""
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


@torch.no_grad()
def validate(model, batches):
    """trainer/uflow_trainer.py:116-133 without the loss call and the tensorboard images: eval mode, no_grad,
    model(img_pair), score res['flows_fw'][0].  batches yields (img_pair, gt) or (img_pair, gt, move).  The model's
    training mode is restored.  -> FlowMetrics.compute()."""
    was_training = model.training
    model.eval()
    meter = FlowMetrics()
    try:
        for batch in batches:
            img_pair, gt = batch[0], batch[1]
            move = batch[2] if len(batch) > 2 else None
            meter.update(model(img_pair)['flows_fw'][0], gt, move)
    finally:
        model.train(was_training)
    return meter.compute()
