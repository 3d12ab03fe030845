"""Yardstick for the TCNWakeword step of tools/bench_models.py: the same model as plain torch.nn in the reference's own
formulation (nn.Conv1d(padding=(k-1) d, dilation=d) on (B, C, T), ReLU, Dropout, trim, residual; AdaptiveAvgPool1d -> Dropout ->
Linear -- MIOpen's convolution kernels) and one autograd training step on (B, 40, 151) features already on the device (no front
end): forward, cross-entropy, backward, clip, AdamW.

    python tools/bench_torch_tcn.py 512 [fp32|bf16|fp16]      -> one JSON line"""
import json
import sys
import time

import torch
import torch.nn as nn

dev = "cuda:0"
B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
mode = sys.argv[2] if len(sys.argv) > 2 else "fp32"
T = 151


class Block(nn.Module):
    def __init__(self, cin, cout, k, d, p):
        super().__init__()
        self.conv1 = nn.Conv1d(cin, cout, k, padding=(k - 1) * d, dilation=d)
        self.conv2 = nn.Conv1d(cout, cout, k, padding=(k - 1) * d, dilation=d)
        self.drop = nn.Dropout(p)
        self.downsample = nn.Conv1d(cin, cout, 1) if cin != cout else None

    def forward(self, x):
        out = self.drop(torch.relu(self.conv1(x)))
        out = self.drop(torch.relu(self.conv2(out)))[:, :, :x.size(2)]
        return torch.relu(out + (x if self.downsample is None else self.downsample(x)))


torch.manual_seed(0)
chans = [40, 64, 128, 256]
model = nn.Sequential(*[Block(chans[i], chans[i + 1], 3, 2 ** i, 0.3) for i in range(3)], nn.AdaptiveAvgPool1d(1), nn.Flatten(),
                      nn.Dropout(0.3), nn.Linear(256, 2)).to(dev)
params = list(model.parameters())
opt = torch.optim.AdamW(params, lr=1e-3)
x = torch.randn(B, 40, T, device=dev)
y = torch.randint(0, 2, (B,), device=dev)
amp = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(mode)


def step():
    with torch.autocast("cuda", dtype=amp or torch.bfloat16, enabled=amp is not None):
        loss = nn.functional.cross_entropy(model(x).float(), y)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(params, 1.0)
    opt.step()


for _ in range(5):
    step()
torch.cuda.synchronize()
n = 30
t0 = time.perf_counter()
for _ in range(n):
    step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / n
print(json.dumps({"model": "torch.nn.Conv1d TCN (MIOpen) + Linear, no front end", "batch": B, "mode": mode,
                  "ms_per_step": round(dt * 1e3, 3), "samples_per_s": round(B / dt, 1),
                  "conv_tflops": round(6 * B * T * 432640 / dt / 1e12, 2)}))
