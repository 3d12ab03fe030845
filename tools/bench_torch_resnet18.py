"""Yardstick for the ResNet18Wakeword step of tools/bench_models.py: the same model as plain torch.nn (nn.Conv2d / nn.BatchNorm2d /
max_pool2d -- MIOpen's kernels -- in channels-last memory format, torchvision's resnet18 restated with the reference's one-channel
conv1 and Dropout -> Linear head) and one autograd training step on (B, 1, F, T) features already on the device (no front end):
forward, cross-entropy, backward, clip, AdamW.  16-bit modes run under torch.autocast.

    python tools/bench_torch_resnet18.py 128 [fp32|bf16|fp16] [F T]      -> one JSON line"""
import json
import sys
import time

import torch
import torch.nn as nn

dev = "cuda:0"


class Block(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False), nn.BatchNorm2d(cout)
        self.conv2, self.bn2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False), nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        out = self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x)))))
        return torch.relu(out + (x if self.downsample is None else self.downsample(x)))


class ResNet18(nn.Module):
    def __init__(self, num_classes=2, dropout=0.3):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(1, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
        cfg = [(64, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1), (256, 512, 2), (512, 512, 1)]
        self.blocks = nn.Sequential(*[Block(*c) for c in cfg])
        self.fc = nn.Sequential(nn.Dropout(dropout), nn.Linear(512, num_classes))

    def forward(self, x):
        x = nn.functional.max_pool2d(torch.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        return self.fc(self.blocks(x).mean((2, 3)))


def conv_flop(F, T):
    """Forward multiply-adds x 2 of the convolutions of one sample (6 M K N over fwd + dX + dW = 3 x this)."""
    size = lambda n, k, s: (n + 2 * (k // 2) - k) // s + 1
    h, w = size(F, 7, 2), size(T, 7, 2)
    flop = 2 * h * w * 49 * 64
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    cin = 64
    for cout, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):
        h2, w2 = size(h, 3, stride), size(w, 3, stride)
        flop += 2 * h2 * w2 * (9 * cin * cout + 9 * cout * cout)           # block 0: conv1, conv2
        if stride != 1 or cin != cout:
            flop += 2 * h2 * w2 * cin * cout                                # its 1x1 downsample
        flop += 2 * h2 * w2 * 2 * 9 * cout * cout                           # block 1
        h, w, cin = h2, w2, cout
    return flop


def torch_step_ms(B, mode, F=40, T=151, n=20):
    torch.manual_seed(0)
    model = ResNet18().to(dev).to(memory_format=torch.channels_last)
    params = list(model.parameters())
    opt = torch.optim.AdamW(params, lr=1e-3)
    x = torch.randn(B, 1, F, T, device=dev).contiguous(memory_format=torch.channels_last)
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
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


if __name__ == "__main__":
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    mode = sys.argv[2] if len(sys.argv) > 2 else "fp32"
    F, T = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (40, 151)
    ms = torch_step_ms(B, mode, F, T)
    print(json.dumps({"model": "torch.nn resnet18 (MIOpen, channels-last) + Linear, no front end", "batch": B, "mode": mode,
                      "features": [1, F, T], "ms_per_step": round(ms, 3), "samples_per_s": round(B / ms * 1e3, 1),
                      "conv_tflops": round(3 * B * conv_flop(F, T) / ms / 1e9, 2)}))
