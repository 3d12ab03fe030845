"""Run-to-run spread of the list-fed Trainer: three Trainers with the same initial weights over ONE list of six batches (cnn_small,
fp32, B=8, 1.5 s clips, 2 epochs of 3).  The yardstick of tests/test_data_pipeline_gpu.py's loader-against-lists comparison."""
import sys
import tempfile
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from wakeword_trainer_home_amd.config import get_preset
from wakeword_trainer_home_amd.data import make_synthetic_batch
from wakeword_trainer_home_amd.models import create_model
from wakeword_trainer_home_amd.training import Trainer
DEV = "cuda:0"
class Rec:
    def __init__(s): s.loss = []
    def on_batch_end(s, i, loss, acc): s.loss.append(loss)
wave, y = make_synthetic_batch(48, 24000, seed=6, device=DEV, pos_rate=0.4, dtype=torch.int16)
batches = [(wave[i:i + 8], y[i:i + 8], {}) for i in range(0, 48, 8)]
torch.manual_seed(5)
init = {k: v.clone() for k, v in create_model("cnn_small", dropout=0.0).state_dict().items()}
runs = []
for r in range(3):
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 2, 0, 8
    cfg.optimizer.mixed_precision = False
    m = create_model("cnn_small", dropout=0.0); m.load_state_dict(init)
    t = Trainer(m, batches[:3], batches[:1], cfg, checkpoint_dir=Path(tempfile.mkdtemp()), device=DEV)
    rec = Rec(); t.add_callback(rec)
    class Swap:
        def on_epoch_start(s, e, t=t): t.train_loader = batches[3 * e:3 * e + 3]
    t.add_callback(Swap())
    t.train()
    runs.append(rec.loss)
    print("run", r, [repr(v) for v in rec.loss], flush=True)
a = np.array(runs)
print("max spread", np.abs(a - a[0]).max(), "bit-equal", bool((a == a[0]).all()))
