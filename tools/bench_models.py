"""BASELINE configs 3 and 5 on one GPU (MobileNetV3 with the reference head at the per-GPU and the global batch; CRNN (conv front-end + 2-layer bidirectional GRU) training step -- log-mel front end,
forward, native loss, backward, clip, AdamW -- at batch 4096 (and 512), inputs resident in HBM.  Secondary measurement:
bench.py's headline line stays BASELINE config 2."""
import contextlib
import gc
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from wakeword_trainer_home_amd import _native as nat
from wakeword_trainer_home_amd.config import get_preset
from wakeword_trainer_home_amd.data import make_synthetic_batch
from wakeword_trainer_home_amd.models import create_model, LSTMWakeword, ResNet18Wakeword, TCNWakeword
from wakeword_trainer_home_amd.training import Trainer

dev = "cuda:0"
CONFIGS = (("crnn", 512, "bf16"), ("crnn", 4096, "bf16"), ("gru", 4096, "fp32"), ("mobilenetv3", 256, "bf16"),
           ("mobilenetv3", 2048, "bf16"))
GRAPH = "--graph" in sys.argv                 # replay the step as a captured HIP graph (Trainer hip_graph mode)
# --storage (resnet18 | tcn): also run the step with 16-bit activation storage (storage = the matrix mode) -- the fp32-storage arm first,
# the storage arm second, resnet18's torch yardstick once, between them (after the first arm), all in this process
# --storage-only: the storage arm alone (a profiler run of that arm)
STORAGE_ONLY = "--storage-only" in sys.argv
STORAGE = "--storage" in sys.argv or STORAGE_ONLY
argv = [a for a in sys.argv[1:] if a not in ("--graph", "--storage", "--storage-only")]
if argv:                                      # e.g.  bench_models.py crnn 4096 fp16 [--graph]  |  lstm 512 fp32  |  tcn 512 bf16
    CONFIGS = ((argv[0], int(argv[1]), argv[2]),)          # | resnet18 128 bf16 [N_MELS N_SAMPLES: 128 40000 = the preset's features]
N_MELS, N_SAMPLES = (int(argv[3]), int(argv[4])) if len(argv) > 4 else (40, 24000)
if STORAGE and (len(CONFIGS) != 1 or CONFIGS[0][0] not in ("resnet18", "tcn") or CONFIGS[0][2] == "fp32"):
    sys.exit("--storage: resnet18 or tcn in a 16-bit matrix mode only, e.g.  bench_models.py resnet18 128 bf16 128 40000 --storage  |  "
             "bench_models.py tcn 512 bf16 --storage")
TORCH_MS = None
RUNS = ([] if STORAGE_ONLY else [c + (None,) for c in CONFIGS]) + ([CONFIGS[0] + (CONFIGS[0][2],)] if STORAGE else [])
for arch, B, act, storage in RUNS:
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.batch_size = B
    cfg.data.n_mels = N_MELS
    cfg.training.hip_graph, cfg.training.hip_graph_auto = GRAPH, False       # the eager line is eager for every model
    torch.manual_seed(0)
    kw = {"act_dtype": act} if arch == "crnn" else {"mode": act}
    if storage:
        kw["storage"] = storage
    # (the factory does not offer "lstm" and "tcn" yet: the reference's LSTMWakeword / TCNWakeword are built directly; the TCN
    # sees (B, 1, 40, 151) feature batches: 6 B T 432 640 FLOP per step in its convolutions, timed under "linear_mfma")
    # resnet18 likewise: its convolutions' own 6 M K N FLOP (tools/bench_torch_resnet18.conv_flop) give conv_tflops, and the step of
    # the plain-torch formulation (nn.Conv2d / BatchNorm2d / max_pool2d, channels-last, same dtype) is timed in the same run
    direct = {"lstm": LSTMWakeword, "tcn": TCNWakeword, "resnet18": ResNet18Wakeword}
    model = direct[arch](dropout=0.3, **kw) if arch in direct else create_model(arch, dropout=0.3, **kw)
    with contextlib.redirect_stdout(sys.stderr):
        tr = Trainer(model, [], [], cfg, checkpoint_dir=Path(tempfile.mkdtemp()), device=dev)
    tr.model.train()
    pool = [make_synthetic_batch(B, N_SAMPLES, seed=i, device=dev) for i in range(2)]
    classes = ["logmel_specaug", "conv_stem_fwd", "dwconv3x3_fwd", "pwconv1x1_fwd", "pwconv1x1_bwd", "dwconv3x3_bwd", "conv_stem_bwd",
               "finalize", "gru", "linear_mfma", "nhwc_layers", "lstm"]

    def step(i):
        (tr._step_autograd_async if tr._async_autograd else tr._step_generic)(*pool[i % 2], i)

    for i in range(5):
        step(i)
    torch.cuda.synchronize()
    n = 30 if B <= 1024 else 12
    gc.collect()
    gc.disable()          # as timeit does: a generation-2 collection inside the loop is a one-off 50-80 ms host pause (seen: one 76 ms
    t0 = time.perf_counter()      # step among thirty 2.9 ms ones made "crnn 512 fp16" read 5.3 ms instead of 2.94)
    for i in range(n):
        step(5 + i)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    gc.enable()
    nat.prof_enable(dev, classes)
    tr.use_hip_graph = False                   # the per-class event timing needs host-issued launches
    step(100)
    torch.cuda.synchronize()
    prof = {k: round(v[0], 3) for k, v in nat.prof_collect(dev).items()}
    nat.prof_enable(dev, [])
    extra = {}
    if arch == "resnet18":
        from bench_torch_resnet18 import conv_flop, torch_step_ms
        F_, T_ = N_MELS, nat.num_frames(N_SAMPLES, cfg.data.hop_length)
        pool = []                              # (the native step's clips make room for the torch model's activations)
        torch.cuda.empty_cache()
        if TORCH_MS is None:                   # (one torch run serves both storage arms)
            TORCH_MS = torch_step_ms(B, act, F_, T_)
        t_ms = TORCH_MS
        extra = {"features": [1, F_, T_], "conv_tflops": round(3 * B * conv_flop(F_, T_) / dt / 1e12, 2),
                 "torch_ms_per_step_no_front_end": round(t_ms, 3), "native_over_torch": round(dt * 1e3 / t_ms, 3)}
    print(json.dumps({"model": arch, "batch": B, "conv_storage": act if arch == "crnn" else (storage or "fp32" if arch in ("resnet18", "tcn") else None), "matrix_mode": act,
                      "hip_graph": tr._graph is not None, "loss_scale": tr.scaler.get_scale() if tr.loss_scale is not None else None,
                      "ms_per_step": round(dt * 1e3, 3),
                      "samples_per_s": round(B / dt, 1),
                      **({"conv_tflops": round(6 * B * 151 * 432640 / dt / 1e12, 2)} if arch == "tcn" else {}), **extra,
                      "class_ms_one_step": prof}))
    del tr, model, pool
    torch.cuda.empty_cache()
