"""CPU, world_size 2 over gloo: FlowMetrics.compute() all-reduces its (metric totals, sample count) vector, so two ranks
that saw different samples -- and different numbers of them -- report the single-process means."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sums():
    g = torch.Generator().manual_seed(11)
    s = torch.rand(5, 8, generator=g, dtype=torch.float64) * 40 + 1
    s[:, 0] += s[:, 2] + s[:, 5]
    s[:, 1] += s[:, 3] + s[:, 6] + 2
    s[:, 7] = 0
    return s


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    from arflow_amd.metrics import FlowMetrics
    s = _sums()
    mine = s[:2] if rank == 0 else s[2:]  # 2 samples on rank 0, 3 on rank 1, in two updates there
    m = FlowMetrics()
    for part in ((mine,) if rank == 0 else (mine[:1], mine[1:])):
        m.update_from_sums(part, True, True)
    q.put((rank, m.compute()))
    dist.barrier()
    dist.destroy_process_group()


def test_flow_metrics_world2_equals_single_process():
    from arflow_amd.metrics import FlowMetrics
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0, 'rank failed'
    out = dict(q.get() for _ in range(2))
    single = FlowMetrics()
    single.update_from_sums(_sums(), True, True)
    want = single.compute()
    assert sorted(out) == [0, 1] and len(want) == 6
    for rank in (0, 1):
        assert list(out[rank]) == list(want)
        for n in want:
            assert abs(out[rank][n] - want[n]) <= 1e-12 * abs(want[n]), (rank, n, out[rank][n], want[n])
