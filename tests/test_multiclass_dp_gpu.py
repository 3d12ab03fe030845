"""GPU: the epoch's confusion matrix of a 3-class run summed across data-parallel ranks -- 2 ranks sharing the one GPU of the test
box over gloo, as tests/test_data_parallel_gpu.py runs them."""
import os
import socket
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, str(REPO))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 1, 0, 8
    cfg.model.dropout, cfg.model.num_classes = 0.3, 3
    torch.manual_seed(70 + rank)                      # different initial weights per rank: the Trainer broadcasts rank 0's
    model = create_model("crnn", num_classes=3, dropout=0.3, dropout_seed=5)
    wave, y = make_synthetic_batch(32, 24000, seed=9)
    y = (torch.arange(32) * 5 % 3).to(y.dtype)
    batches = [(wave[16 * s + 8 * rank:16 * s + 8 * rank + 8], y[16 * s + 8 * rank:16 * s + 8 * rank + 8]) for s in range(2)]
    t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=Path(out_dir) / f"ck{rank}", device="cuda:0")
    assert t.world_size == world and t.criterion.num_classes == 3 and t._confusion is not None
    t.train_epoch(0)
    out = {"train_local": t._confusion.cpu().clone(), "train": t.train_metrics_tracker.compute(),
           "train_m": t.train_metrics_tracker._m.copy()}
    _, vm = t.validate_epoch(0)
    out.update(val_local=t._confusion.cpu().clone(), val=vm)
    torch.save(out, Path(out_dir) / f"r{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_report_the_sum_of_their_matrices(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wakeword_trainer_home_amd.training import MetricResults
    mp.start_processes(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    r = [torch.load(tmp_path / f"r{k}.pt", weights_only=False) for k in (0, 1)]
    for part, n in (("train", 16), ("val", 8)):
        local = [x[part + "_local"].numpy() for x in r]
        assert [int(m.sum()) for m in local] == [n, n]                        # each rank counted its own clips
        total = local[0] + local[1]
        want = MetricResults.from_confusion(total)
        assert r[0][part] == want and r[1][part] == want and want.total_samples == 2 * n
    assert (r[0]["train_m"] == r[0]["train_local"].numpy() + r[1]["train_local"].numpy()).all()
    # the ranks saw different clips: their matrices' rows are the label counts of their own shards
    assert r[0]["train_local"].sum(dim=1).tolist() == [5, 5, 6] and r[1]["train_local"].sum(dim=1).tolist() == [6, 5, 5]
