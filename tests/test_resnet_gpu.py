"""The dense Conv2d kernels (ww_conv2d_fwd / _bwd), the one-channel stem, MaxPool2d(3, 2, 1) and ResNet18Wakeword on the MI355X.

References: the float64 restatements of tests/resnet_cases.py (pinned on the CPU to the reference's own ResNet18Wakeword through
tests/golden/g11_resnet18.npz), with ``oracle.rounding.mround`` at the device's rounding points for the 16-bit matrix modes and
``oracle.gru.dropout_bt_mask`` for the head dropout.  No bound here comes from what the device gave: the layer's round-off bound is
5e-7 sum|a b| per element (the fp32 MFMA chain at K = 4608), the fp32 model is held to 4x the error float32 CPU torch makes on the
same case (stored in the fixture), the 16-bit models to 4x the error the operand rounding itself makes (computed here).  The
measured values are printed (-rP) and recorded in profiles/r11_resnet18_parity_measured.txt."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests.resnet_cases import (ResNetRestated, golden_case, layer_case, layer_inputs, maxpool_bwd, maxpool_fwd, out_size, sampled_rel,
                                stem_case)

gpu = pytest.mark.gpu
DEV = "cuda:0"
_MD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
_MT = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}
_MODES = ["fp32", "bf16", "fp16"]
# (B, H, W, Cin, Cout, k, stride): one pixel and one tap; only the centre tap inside the image; M tiles that span rows and samples,
# odd sizes, channel counts below a tile (both strides); even sizes and the 1x1 stride-2 downsample whose dx is zero at odd pixels;
# 160-byte rows; K = 2304 and eight column tiles; K = 4608 with M = 4; M = 1360: more than one dW row range
_SHAPES = [(1, 1, 1, 4, 4, 1, 1), (1, 1, 1, 4, 4, 3, 1), (2, 5, 7, 8, 12, 3, 1), (2, 5, 7, 8, 12, 3, 2), (3, 6, 4, 64, 128, 3, 2),
           (3, 6, 4, 64, 128, 1, 2), (5, 10, 9, 40, 64, 3, 1), (2, 3, 3, 256, 512, 3, 2), (1, 2, 2, 512, 512, 3, 1),
           (4, 20, 17, 64, 64, 3, 1)]
_IDS = ["-".join(map(str, s)) for s in _SHAPES]
# (B, H, W, Cout, k, stride): an image smaller than the kernel; stride 1; the fixture's stem
_STEMS = [(1, 5, 3, 64, 7, 2), (3, 13, 8, 16, 3, 1), (2, 40, 33, 64, 7, 2)]
_POOLS = [(1, 1, 1, 4), (2, 5, 7, 8), (2, 20, 17, 64)]
_LAYER_REF = {}


def _layer_ref(shape, integer, mode):
    """Inputs and the restated layer, computed once per (shape, data kind, rounding)."""
    key = (shape, integer, _MT[mode] if not integer else None)
    d_in = layer_inputs(*shape, seed=sum(shape) + 17 * int(integer), integer=integer)
    if key not in _LAYER_REF:
        _LAYER_REF[key] = layer_case(d_in["x"], d_in["w"], d_in["dy"], shape[6], mtype=key[2])
    return d_in, _LAYER_REF[key]


def _f(t):
    return t.float().to(DEV)


def _layer_gpu(d_in, stride, mode, **kw):
    from wakeword_trainer_home_amd import _native as nat
    x, w, dy = _f(d_in["x"]), _f(d_in["w"]), _f(d_in["dy"])
    y = nat.conv2d_fwd(x, w, stride, mode=_MD[mode])
    dx, dw = nat.conv2d_bwd(x, w, dy, stride, mode=_MD[mode], **kw)
    return dict(y=y, dx=dx, dw=dw)


# ------------------------------------------------------------------------------------------ the layers
@gpu
@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("shape", _SHAPES, ids=_IDS)
def test_conv2d_is_exact_on_integer_data(shape, mode):
    """Integer-valued x, dy in [-4, 4] and W in [-2, 2]: every product and sum is exact in fp32 and in the 16-bit operand types (all
    sums stay below 2^24), so y, dx and dw equal the float64 restatement BIT FOR BIT in every mode.  Also: dx added to a given
    tensor, no dx at all, and a dx buffer full of NaN that comes back fully written (stride 2: also the pixels no output read)."""
    from wakeword_trainer_home_amd import _native as nat
    stride = shape[6]
    d_in, ref = _layer_ref(shape, True, mode)
    assert max(ref[n + "_abs"].max().item() for n in ("y", "dx", "dw")) < 2 ** 24
    got = _layer_gpu(d_in, stride, mode)
    for n in ("y", "dx", "dw"):
        assert tuple(got[n].shape) == tuple(ref[n].shape), n
        assert torch.equal(got[n].cpu().double(), ref[n]), (n, (got[n].cpu().double() - ref[n]).abs().max().item())
    x, w, dy = _f(d_in["x"]), _f(d_in["w"]), _f(d_in["dy"])
    base = torch.full_like(x, 3.0)
    dx2, dw2 = nat.conv2d_bwd(x, w, dy, stride, mode=_MD[mode], dx=base)
    assert dx2 is base and torch.equal(base.cpu().double(), ref["dx"] + 3.0) and torch.equal(dw2, got["dw"])
    dx3, dw3 = nat.conv2d_bwd(x, w, dy, stride, mode=_MD[mode], need_dx=False)
    assert dx3 is None and torch.equal(dw3, got["dw"])
    nan = torch.full_like(x, float("nan"))
    dx4, _ = nat.conv2d_bwd(x, w, dy, stride, mode=_MD[mode], dx=nan, accumulate=False)
    assert dx4 is nan and torch.equal(nan.cpu().double(), ref["dx"])


@gpu
@pytest.mark.parametrize("shape", _STEMS, ids=["-".join(map(str, s)) for s in _STEMS])
def test_stem_is_exact_on_integer_data(shape):
    from wakeword_trainer_home_amd import _native as nat
    B, H, W, Cout, k, stride = shape
    d_in = layer_inputs(B, H, W, 4, Cout, k, stride, seed=sum(shape), integer=True)
    x, w = d_in["x"][..., 0].contiguous(), d_in["w"][:, :1].contiguous()
    ry, rdw = stem_case(x, w, d_in["dy"], stride)
    y = nat.conv2d_stem_fwd(_f(x), _f(w), stride)
    assert tuple(y.shape) == (B, out_size(H, k, stride), out_size(W, k, stride), Cout) and torch.equal(y.cpu().double(), ry)
    dw = nat.conv2d_stem_bwd_dw(_f(x), _f(d_in["dy"]), tuple(w.shape), stride)
    assert torch.equal(dw.cpu().double(), rdw)
    # deferred: queued (more than one block of partials) or written at once, equal after the flush either way
    slot = torch.full(tuple(w.shape), float("nan"), device=DEV)
    nat.conv2d_stem_bwd_dw(_f(x), _f(d_in["dy"]), tuple(w.shape), stride, dw_out=slot, defer=True)
    nat.deferred_flush(DEV)
    torch.cuda.synchronize()
    assert nat.load().ww_deferred_reduce_pending(nat.ctx(DEV)) == 0 and torch.equal(slot.cpu().double(), rdw)


@gpu
@pytest.mark.parametrize("shape", _POOLS, ids=["-".join(map(str, s)) for s in _POOLS])
def test_maxpool_is_exact_and_first_maximum_takes_the_gradient(shape):
    """Integer data in [0, 2] (most windows tie, as after a ReLU) and in [-4, -1] (padding must never win)."""
    from wakeword_trainer_home_amd import _native as nat
    g = torch.Generator().manual_seed(sum(shape))
    for lo, hi in ((0, 2), (-4, -1)):
        x = torch.randint(lo, hi + 1, shape, generator=g).double()
        ry, idx = maxpool_fwd(x)
        dy = torch.randint(-4, 5, tuple(ry.shape), generator=g).double()
        y = nat.maxpool3x3s2_fwd(_f(x))
        dx = nat.maxpool3x3s2_bwd(_f(x), _f(dy))
        assert torch.equal(y.cpu().double(), ry)
        assert torch.equal(dx.cpu().double(), maxpool_bwd(idx, dy, shape[1], shape[2]))


@gpu
@pytest.mark.parametrize("mode", _MODES)
def test_deferred_weight_gradient_equals_immediate(mode):
    """M = 1360: ten row ranges.  Under ww_ctx_set_deferred_reduce the sum of the partial products is queued (one item) and run
    by the flush; on integer data both orders of summation are exact, so the results are equal bit for bit."""
    from wakeword_trainer_home_amd import _native as nat
    shape = _SHAPES[-1]
    d_in, ref = _layer_ref(shape, True, mode)
    lib, cx = nat.load(), nat.ctx(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    slot = torch.full(tuple(d_in["w"].shape), float("nan"), device=DEV)
    got = _layer_gpu(d_in, shape[6], mode, dw_out=slot, defer=True)
    assert lib.ww_deferred_reduce_pending(cx) == 1
    nat.deferred_flush(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    torch.cuda.synchronize()
    assert got["dw"] is slot and torch.equal(slot.cpu().double(), ref["dw"])


_ROUNDOFF = 5e-7          # per element: |got - ref| <= 5e-7 sum|a b| (the guide's 3.5e-7 at K = 4096, with margin for K = 4608)


@gpu
@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("shape", _SHAPES[-3:], ids=_IDS[-3:])
def test_conv2d_roundoff_against_restatement(shape, mode):
    """N(0,1) data.  fp32: an exact fma chain in K order, so every element of y, dx, dw is within 5e-7 sum|a b| of the float64
    restatement.  16-bit modes: the same bound against the restatement that rounds the operands, since only the fp32 accumulation
    order separates the two."""
    d_in, ref = _layer_ref(shape, False, mode)
    got = _layer_gpu(d_in, shape[6], mode)
    worst = {}
    for n in ("y", "dx", "dw"):
        err, scale = (got[n].cpu().double() - ref[n]).abs(), ref[n + "_abs"]
        assert not (err[scale == 0] != 0).any(), n
        worst[n] = (err / scale.clamp_min(1e-300)).max().item()
    print(f"resnet-layer roundoff {'-'.join(map(str, shape))} {mode}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()) + " (x sum|a b|)")
    for n, e in worst.items():
        assert e <= _ROUNDOFF, (n, e)


# ------------------------------------------------------------------------------------------ the model
def _spy_relu_outputs(monkeypatch):
    """Record the output of every ReLU of the model's forward (BatchNorm+ReLU passes and add+ReLU), in forward order."""
    from wakeword_trainer_home_amd import _native as nat
    seen, bn, add = [], nat.bn_act_fwd, nat.add_relu_fwd

    def spy_bn(x, bnp, act, Cn):
        out = bn(x, bnp, act, Cn)
        if act == nat.LIN_RELU:
            seen.append(out[0])
        return out

    def spy_add(a, b):
        y = add(a, b)
        seen.append(y)
        return y
    monkeypatch.setattr(nat, "bn_act_fwd", spy_bn)
    monkeypatch.setattr(nat, "add_relu_fwd", spy_add)
    return seen


def _flips(seen, oracle):
    assert len(seen) == len(oracle.pres) == 17
    return [int(((a != 0).cpu() != m).sum()) for a, m in zip(seen, oracle.relu_masks)]


def _model(sd, **kw):
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    model = ResNet18Wakeword(**kw)
    model.load_state_dict(sd)
    return model.to(DEV)


@gpu
def test_resnet18_matches_reference_fixture(monkeypatch):
    """tests/golden/g11_resnet18.npz was produced by the reference's own ResNet18Wakeword in float64, on parameters whose ReLU inputs
    all keep >= 4e-5 from zero: no ReLU decision of the fp32 device run differs from the float64 restatement's, and the eval
    logits, train logits, loss, running statistics and every parameter gradient are within 4x the error float32 CPU torch makes
    on the same case (fixture ``err.*``; the fp32 MFMA chain sums K up to 4608 in strict sequence, about 3.5x the error of
    blocked sums)."""
    sd, g = golden_case()
    model = _model(sd, dropout=0.0)
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    oracle = ResNetRestated(sd)
    _, _, go = oracle.loss_and_grads(torch.from_numpy(g["x"]).double(), torch.from_numpy(g["y"]))
    model.eval()
    with torch.no_grad():
        ev = model(x)
        # eval logits do not depend on the batch's other rows
        alone = model(x[1:].contiguous())
        swapped = model(torch.stack([x[1], x[0]]))
    model.train()
    seen = _spy_relu_outputs(monkeypatch)
    out = model(x)
    flips = _flips(seen, oracle)
    loss = torch.nn.functional.cross_entropy(out, y)
    loss.backward()
    e_ev = (ev.cpu().double() - torch.from_numpy(g["logits_eval"])).abs().max().item()
    e_tr = (out.detach().cpu().double() - torch.from_numpy(g["logits_train"])).abs().max().item()
    e_loss = abs(loss.item() - float(g["loss"]))
    named = dict(model.named_parameters())
    e_s = {n: sampled_rel(p.grad, g, n) for n, p in named.items()}
    e_w = {n: (p.grad.cpu().double() - go[n]).abs().max().item() / g["gmax"][n] for n, p in named.items()}
    state = model.state_dict()
    e_r = {k: (state[k].cpu().double() - torch.from_numpy(v)).abs().max().item() / np.abs(v).max() for k, v in g["rstat"].items()}
    ratio = lambda e, b: max(e[n] / b[n] for n in e)
    print(f"resnet18 fixture fp32: ReLU flips {sum(flips)} of {int(g['relu_inputs'])} (margin {float(g['relu_margin']):.2e}); device error (x the "
          f"float32-CPU error): eval {e_ev:.2e} ({e_ev / float(g['err.logits_eval']):.2f}x) train {e_tr:.2e} ({e_tr / float(g['err.logits_train']):.2f}x) "
          f"loss {e_loss:.2e} ({e_loss / float(g['err.loss']):.2f}x) running stats max {max(e_r.values()):.2e} ({ratio(e_r, g['err.rstat']):.2f}x) "
          f"grads sampled max {max(e_s.values()):.2e} ({ratio(e_s, g['err.grad']):.2f}x) whole max {max(e_w.values()):.2e} ({ratio(e_w, g['err.grad']):.2f}x)")
    worst = sorted(((e_w[n] / g["err.grad"][n], n, e_w[n], g["err.grad"][n]) for n in e_w), reverse=True)[:3]
    print("resnet18 fixture fp32: largest gradient ratios " + "; ".join(f"{n} {e:.2e} / {b:.2e} = {r:.2f}x" for r, n, e, b in worst))
    assert sum(flips) == 0, flips
    assert torch.equal(alone[0], ev[1]) and torch.equal(swapped[0], ev[1]) and torch.equal(swapped[1], ev[0])
    assert e_ev <= 4 * float(g["err.logits_eval"]) and e_tr <= 4 * float(g["err.logits_train"]) and e_loss <= 4 * float(g["err.loss"])
    for k in e_r:
        assert e_r[k] <= 4 * g["err.rstat"][k], (k, e_r[k], g["err.rstat"][k])
    for n in e_s:
        assert e_s[n] <= 4 * g["err.grad"][n] and e_w[n] <= 4 * g["err.grad"][n], (n, e_s[n], e_w[n], g["err.grad"][n])
    # num_batches_tracked advances by one per training forward
    assert all(int(v) == 1 for k, v in state.items() if k.endswith("num_batches_tracked"))
    model(x)
    assert all(int(v) == 2 for k, v in model.state_dict().items() if k.endswith("num_batches_tracked"))


@gpu
def test_resnet18_with_head_dropout_matches_restatement():
    """The fixture case with dropout 0.3 against the restatement that draws the _HiddenDropout mask (oracle.gru.dropout_bt_mask,
    stream 15); two consecutive forwards draw different masks (the Philox step advances).  Same network, same input, the mask only
    scales the 512 pooled features: held to the fixture's 4x float32-CPU errors."""
    sd, g = golden_case()
    model = _model(sd, dropout=0.3, dropout_seed=21)
    model.train()
    model.sample_offset = 5
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    outs, worst = [], dict(logits=0.0, loss=0.0, grads=0.0)
    for step in range(2):
        oracle = ResNetRestated(sd, dropout=0.3, seed=21)
        ref, lo, go = oracle.loss_and_grads(torch.from_numpy(g["x"]).double(), torch.from_numpy(g["y"]), step=step, sample_offset=5)
        model.load_state_dict(sd)            # (the running statistics the first step moved)
        model.zero_grad()
        out = model(x)
        loss = torch.nn.functional.cross_entropy(out, y)
        loss.backward()
        outs.append(out.detach().cpu())
        worst["logits"] = max(worst["logits"], (out.detach().cpu().double() - ref).abs().max().item() / float(g["err.logits_train"]))
        worst["loss"] = max(worst["loss"], abs(loss.item() - lo) / float(g["err.loss"]))
        worst["grads"] = max([worst["grads"]] + [(p.grad.cpu().double() - go[n]).abs().max().item() / go[n].abs().max().item() / g["err.grad"][n]
                                                 for n, p in model.named_parameters()])
    print("resnet18 dropout 0.3 (x the float32-CPU error of the fixture case): " + " ".join(f"{k}={v:.2f}x" for k, v in worst.items()))
    assert not torch.equal(outs[0], outs[1])
    for k, v in worst.items():
        assert v <= 4.0, (k, v)


@gpu
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_resnet18_16bit_modes_match_rounding_restatement(mode, monkeypatch):
    """The fixture case against the restatement that rounds the matrix operands.  Logits, loss and per-tensor gradient
    |got - ref|_2 / |ref|_2 are within 4x the same figures of that rounded CPU model against float64 (what the rounding itself
    costs); ReLU flips are printed, not asserted."""
    sd, g = golden_case()
    x64, y64 = torch.from_numpy(g["x"]).double(), torch.from_numpy(g["y"])
    exact = ResNetRestated(sd)
    ref0, lo0, go0 = exact.loss_and_grads(x64, y64)
    oracle = ResNetRestated(sd, mtype=_MT[mode])
    ref, lo, go = oracle.loss_and_grads(x64, y64)
    l2 = lambda a, b: ((a - b).norm() / b.norm()).item()
    cpu = dict(logits=(ref - ref0).abs().max().item(), loss=abs(lo - lo0), grads_l2={n: l2(go[n], go0[n]) for n in go})
    model = _model(sd, dropout=0.0, mode=mode)
    model.train()
    seen = _spy_relu_outputs(monkeypatch)
    out = model(torch.from_numpy(g["x"]).to(DEV))
    flips = sum(_flips(seen, oracle))
    loss = torch.nn.functional.cross_entropy(out, y64.to(DEV))
    loss.backward()
    dev = dict(logits=(out.detach().cpu().double() - ref).abs().max().item(), loss=abs(loss.item() - lo),
               grads_l2={n: l2(p.grad.cpu().double(), go[n]) for n, p in model.named_parameters()})
    rmax = max(dev["grads_l2"][n] / cpu["grads_l2"][n] for n in go)
    print(f"resnet18 {mode}: ReLU flips {flips} of {int(g['relu_inputs'])}; device vs rounding restatement | rounded CPU vs float64: "
          f"logits {dev['logits']:.2e} | {cpu['logits']:.2e} loss {dev['loss']:.2e} | {cpu['loss']:.2e} "
          f"grads l2 max {max(dev['grads_l2'].values()):.2e} | {max(cpu['grads_l2'].values()):.2e} (largest ratio {rmax:.2f}x)")
    assert dev["logits"] <= 4 * cpu["logits"] and dev["loss"] <= 4 * cpu["loss"]
    for n in go:
        assert dev["grads_l2"][n] <= 4 * cpu["grads_l2"][n], (n, dev["grads_l2"][n], cpu["grads_l2"][n])


# ------------------------------------------------------------------------------------------ the Trainer
def _trainer_cfg(batch_size=8, epochs=1):
    from wakeword_trainer_home_amd.config import get_preset
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = epochs, 0, batch_size
    cfg.loss.label_smoothing = 0.0
    return cfg


@gpu
def test_trainer_drives_resnet18(tmp_path):
    """train_epoch / validate_epoch on waveform batches (native front end -> (8,1,40,35) features -> ResNet18Wakeword -> native
    loss, the sync-free step with the fused clip + optimizer); the first-step loss equals the CPU pipeline's
    (oracle.train_step.frontend -> the float64 restatement) within 1e-3."""
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    from wakeword_trainer_home_amd.training import Trainer
    from wakeword_trainer_home_amd.training.optimizer_factory import FlatFusedOptimizer
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from oracle.train_step import frontend
    cfg = _trainer_cfg()
    torch.manual_seed(9)
    model = ResNet18Wakeword(dropout=0.0)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    wave, y = make_synthetic_batch(24, 5440, seed=5)                 # 5440 samples: 35 frames
    y[::3] = 1
    batches = [(wave[i:i + 8], y[i:i + 8], [{"path": "s"}] * 8) for i in range(0, 24, 8)]
    t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path, device=DEV)
    assert isinstance(t.optimizer, FlatFusedOptimizer) and t._async_autograd
    losses = []
    t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: losses.append(l)})())
    t.train_epoch(0)
    assert len(losses) == 3 and all(np.isfinite(losses))
    a = cfg.augmentation
    spec = dict(freq_mask_param=a.freq_mask_param, time_mask_param=a.time_mask_param, n_freq_masks=a.n_freq_masks,
                n_time_masks=a.n_time_masks, freq_mask_prob=a.freq_mask_prob, time_mask_prob=a.time_mask_prob)
    x0, _ = frontend(batches[0][0].numpy(), spec, seed=a.seed, step=0)
    x0 = torch.as_tensor(x0).double()
    assert tuple(x0.shape) == (8, 1, 40, 35)
    _, ref, _ = ResNetRestated(sd).loss_and_grads(x0, batches[0][1])
    assert abs(losses[0] - ref) < 1e-3, (losses[0], ref)
    loss, m = t.validate_epoch(0)
    assert m.total_samples == 8 and np.isfinite(loss)


@gpu
def test_graph_replays_equal_eager_steps_bit_for_bit(tmp_path):
    """hip_graph=True: the captured step (forward, loss, backward with deferred partial sums, gather, fused clip + optimizer)
    replayed over two epochs of two full batches and a ragged one (8, 8, 5 rows) equals the eager steps bit for bit: loss trace,
    every parameter and buffer, and the optimizer moments.  Dropout 0.3: the replays draw fresh masks."""
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    from wakeword_trainer_home_amd.training import Trainer
    wave, y = make_synthetic_batch(21, 5440, seed=6)
    y[::3] = 1
    batches = [(wave[8 * i:8 * i + 8], y[8 * i:8 * i + 8]) for i in range(3)]
    assert len(batches[-1][0]) == 5
    runs = []
    for graph in (False, True):
        cfg = _trainer_cfg(epochs=2)
        cfg.optimizer.mixed_precision = False
        cfg.training.hip_graph, cfg.training.hip_graph_auto = graph, False
        cfg.training.checkpoint_frequency = "best_only"
        torch.manual_seed(11)
        model = ResNet18Wakeword(dropout=0.3, dropout_seed=2)
        t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path / f"g{int(graph)}", device=DEV)
        rec = []
        t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: rec.append((i, l))})())
        res = t.train()
        runs.append((t, rec, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                     copy.deepcopy(t.optimizer.state_dict()), res))
    assert runs[1][0]._graph is not None and runs[0][0]._graph is None
    assert len(runs[1][1]) == 6
    assert runs[0][1] == runs[1][1], "loss traces differ"
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    for (ka, va), (kb, vb) in zip(sorted(runs[0][3]["state"].items()), sorted(runs[1][3]["state"].items())):
        for f in va:
            assert torch.equal(torch.as_tensor(va[f]).cpu(), torch.as_tensor(vb[f]).cpu()), (ka, f)


@gpu
def test_nonfinite_batch_is_skipped_on_device(tmp_path):
    """A batch with a NaN sample changes no parameter (the fused optimizer gets the flag on the device) and is not reported."""
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    from wakeword_trainer_home_amd.training import Trainer
    cfg = _trainer_cfg()
    torch.manual_seed(2)
    model = ResNet18Wakeword(dropout=0.0)
    wave, y = make_synthetic_batch(24, 5440, seed=6)
    bad = wave[8:16].clone()
    bad[3, 100] = float("nan")
    batches = [(wave[:8], y[:8]), (bad, y[8:16]), (wave[16:], y[16:])]
    t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path, device=DEV)
    assert t._async_autograd and t.deferred_metrics
    seen = []
    t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: seen.append((i, l))})())
    snaps = []
    orig = t._step_autograd_async
    pnames = [n for n, _ in model.named_parameters()]

    def spy(inputs, targets, idx):
        snaps.append({k: v.clone() for k, v in model.state_dict().items() if k in pnames})
        return orig(inputs, targets, idx)
    t._step_autograd_async = spy
    t.train_epoch(0)
    after = {k: v.clone() for k, v in model.state_dict().items() if k in pnames}
    assert [i for i, _ in seen] == [0, 2] and all(np.isfinite(l) for _, l in seen)
    assert any(not torch.equal(snaps[0][k], snaps[1][k]) for k in snaps[0])
    assert all(torch.equal(snaps[1][k], snaps[2][k]) for k in snaps[1])
    assert any(not torch.equal(snaps[2][k], after[k]) for k in after)


# ------------------------------------------------------------------------------------------ argument checks
@gpu
def test_argument_checks_return_error_codes():
    """Channel counts that are no multiple of 4, an even or too large k, a stride of 0 or 3 and a short scratch region come back as
    error codes (with a message in ww_last_error) before any launch: the output buffers keep their sentinel.  The bindings raise
    WW_E_INVALID as ValueError, the others as NativeError."""
    from wakeword_trainer_home_amd import _native as nat
    lib, cx = nat.load(), nat.ctx(DEV)
    B, H, W, Cin, Cout, k = 2, 5, 7, 8, 12, 3
    z = lambda *s: torch.zeros(*s, device=DEV)
    x, w, y = z(B, H, W, Cin), z(Cout, Cin, k, k), torch.full((B, H, W, Cout), 7.0, device=DEV)
    dx, dw = torch.full((B, H, W, Cin), 7.0, device=DEV), torch.full((Cout, Cin, k, k), 7.0, device=DEV)
    nbytes = lib.ww_conv2d_scratch_bytes(B, H, W, Cin, Cout, k, 1)
    scratch = z(nbytes // 4)
    p = lambda t: C.c_void_p(t.data_ptr())
    fwd = lambda cin, cout, kk, st, sb, mode=0: lib.ww_conv2d_fwd(cx, mode, p(x), p(w), B, H, W, cin, cout, kk, st, p(y), p(scratch), sb, None)
    assert fwd(6, Cout, k, 1, nbytes) == -1 and b"multiples of 4" in lib.ww_last_error()
    assert fwd(Cin, 10, k, 1, nbytes) == -1
    assert fwd(Cin, Cout, 2, 1, nbytes) == -1 and b"kernel_size" in lib.ww_last_error()
    assert fwd(Cin, Cout, 9, 1, nbytes) == -1 and fwd(Cin, Cout, 0, 1, nbytes) == -1
    assert fwd(Cin, Cout, k, 3, nbytes) == -1 and b"stride" in lib.ww_last_error()
    assert fwd(Cin, Cout, k, 0, nbytes) == -1
    assert fwd(Cin, Cout, k, 1, nbytes - 4) == -3 and b"scratch too small" in lib.ww_last_error()
    assert fwd(Cin, Cout, k, 1, nbytes, mode=7) == -1
    bwd = lambda cin, kk, st, sb: lib.ww_conv2d_bwd(cx, 0, p(x), p(w), p(y), B, H, W, cin, Cout, kk, st, p(dx), 0, p(dw), p(scratch), sb, None)
    assert bwd(6, k, 1, nbytes) == -1 and bwd(Cin, 4, 1, nbytes) == -1 and bwd(Cin, k, 3, nbytes) == -1 and bwd(Cin, k, 1, 16) == -3
    img, sw, sy = z(B, H, W), torch.full((16, 1, 7, 7), 7.0, device=DEV), torch.full((B, 3, 4, 16), 7.0, device=DEV)
    stem = lambda c, kk, st: lib.ww_conv2d_stem_fwd(cx, p(img), p(sw), B, H, W, c, kk, st, p(sy), None)
    assert stem(18, 7, 2) == -1 and stem(132, 7, 2) == -1 and stem(16, 6, 2) == -1 and stem(16, 7, 4) == -1
    assert lib.ww_conv2d_stem_bwd_dw(cx, p(img), p(sy), B, H, W, 16, 7, 2, p(sw), p(scratch), 16, None) == -3
    assert lib.ww_maxpool3x3s2_fwd(cx, p(x), B, H, W, 6, p(y), None) == -1 and b"multiple of 4" in lib.ww_last_error()
    assert lib.ww_maxpool3x3s2_bwd(cx, p(x), p(y), B, H, W, 0, p(dx), None) == -1
    torch.cuda.synchronize()
    for t in (y, dx, dw, sw, sy):
        assert t.eq(7.0).all()          # nothing was launched
    with pytest.raises(ValueError, match="multiples of 4"):
        nat.conv2d_fwd(z(B, H, W, 6), z(Cout, 6, k, k))
    with pytest.raises(ValueError, match="kernel_size"):
        nat.conv2d_fwd(x, z(Cout, Cin, 2, 2))
    with pytest.raises(ValueError, match="stride"):
        nat.conv2d_fwd(x, w, stride=3)
    with pytest.raises(ValueError):
        nat.conv2d_fwd(x, z(Cout, Cin + 4, k, k))                       # x and weight disagree about Cin: caught at the binding
    with pytest.raises(ValueError):
        nat.maxpool3x3s2_fwd(z(B, H, W, 6))
