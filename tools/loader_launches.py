"""320 loader launches of one geometry / strategy and nothing else, to run under rocprofv3 --kernel-trace --stats:
    loader_launches.py B n_out none|balanced|weighted [L]      (L = bank row length, default n_out; L > n_out crops)"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from wakeword_trainer_home_amd.data import DeviceBatchLoader, DeviceClipBank
B, n_out, strategy = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
L = int(sys.argv[4]) if len(sys.argv) > 4 else n_out
bank = DeviceClipBank.synthetic(B * 64, L, seed=1, device="cuda:0")
if strategy == "weighted":
    bank.hard_negative = (torch.arange(len(bank), device="cuda:0") % 16 == 1) & (bank.labels == 0)
loader = DeviceBatchLoader(bank, B, n_out, strategy=strategy, seed=3, hard_negative_weight=2.0, drop_last=True)
for e in range(5):
    loader.set_epoch(e)
    for _ in loader:
        pass
torch.cuda.synchronize()
