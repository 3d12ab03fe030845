"""Baseline for the LSTMWakeword step of tools/bench_models.py: the same model shape as plain torch.nn (nn.LSTM(40, 128, 2,
bidirectional, dropout 0.3) -> Dropout -> Linear, i.e. MIOpen's RNN kernels) and one autograd training step on (B, 151, 40)
features already on the device (no front end): forward, cross-entropy, backward, clip, AdamW.

    python tools/bench_torch_lstm.py 512 [fp32|bf16]      -> one JSON line"""
import json
import sys
import time

import torch
import torch.nn as nn

dev = "cuda:0"
B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
mode = sys.argv[2] if len(sys.argv) > 2 else "fp32"
torch.manual_seed(0)
lstm = nn.LSTM(40, 128, num_layers=2, batch_first=True, dropout=0.3, bidirectional=True).to(dev)
fc = nn.Sequential(nn.Dropout(0.3), nn.Linear(256, 2)).to(dev)
params = list(lstm.parameters()) + list(fc.parameters())
opt = torch.optim.AdamW(params, lr=1e-3)
x = torch.randn(B, 151, 40, device=dev)
y = torch.randint(0, 2, (B,), device=dev)


def step():
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16"):
        _, (h, _) = lstm(x)
        loss = nn.functional.cross_entropy(fc(torch.cat([h[-2], h[-1]], 1)), y)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(params, 1.0)
    opt.step()


for _ in range(5):
    step()
torch.cuda.synchronize()
n = 30 if B <= 1024 else 12
t0 = time.perf_counter()
for _ in range(n):
    step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / n
print(json.dumps({"model": "torch.nn.LSTM (MIOpen) + Linear, no front end", "batch": B, "mode": mode,
                  "ms_per_step": round(dt * 1e3, 3), "samples_per_s": round(B / dt, 1)}))
