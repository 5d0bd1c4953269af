"""world_size-2 gloo test (CPU) of the rank reduction of the segmentation evaluation: summing the int64 confusion counts and
the double[2] loss accumulators over the ranks (mgunet.allreduce_eval_state, what SegmentationEvaluator.compute calls) gives
exactly the single-process result.  The per-rank counts come from numpy here -- the device kernel needs a GPU."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mgunet
from mgunet.metrics import confusion_matrix_host

C = 3


def _data():
    rng = np.random.default_rng(77)
    y = rng.integers(0, C, (4, 24, 20))
    y[rng.random(y.shape) < 0.05] = -100
    p = rng.integers(0, C, (4, 24, 20))
    batch_loss = rng.random(4) * 2           # one per image-batch: what the finalize kernel adds to loss_acc[0]
    return y, p, batch_loss


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        y, p, bl = _data()
        lo, hi = mgunet.shard_batch(y.shape[0], rank, world)
        cm = torch.from_numpy(confusion_matrix_host(y[lo:hi], p[lo:hi], C))
        acc = torch.tensor([float(np.sum(bl[lo:hi])), float(hi - lo)], dtype=torch.float64)
        cm_in, acc_in = cm.clone(), acc.clone()
        rcm, racc = mgunet.allreduce_eval_state(cm, acc)
        assert torch.equal(cm, cm_in) and torch.equal(acc, acc_in)   # the evaluator's own state is left as it is
        q.put((rank, rcm.numpy(), racc.numpy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_confusion_and_loss_reduction():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    for pr in procs:
        pr.join(60)
        assert pr.exitcode == 0
    y, p, bl = _data()
    full = confusion_matrix_host(y, p, C)
    for _, cm, acc in res:
        assert cm.dtype == np.int64 and np.array_equal(cm, full)
        assert acc[1] == 4 and acc[0] == pytest.approx(np.sum(bl), rel=1e-15)
    single = mgunet.metrics_from_confusion(full)
    multi = mgunet.metrics_from_confusion(res[0][1])
    assert np.array_equal(np.array(single["iou_per_class"]), np.array(multi["iou_per_class"]))


def test_single_process_reduction_is_a_copy():
    cm = torch.arange(9, dtype=torch.int64).view(3, 3)
    rcm, racc = mgunet.allreduce_eval_state(cm, None)
    assert racc is None and torch.equal(rcm, cm) and rcm.data_ptr() != cm.data_ptr()
