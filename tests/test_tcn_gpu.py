"""The causal dilated Conv1d kernels (ww_tconv1d_fwd / _bwd) and TCNWakeword on the MI355X.

References: the float64 restatements of tests/tcn_cases.py (pinned on the CPU to the reference's own TCNWakeword through
tests/golden/g10_tcn.npz), with ``oracle.rounding.mround`` at the device's rounding points for the 16-bit matrix modes and
``oracle.gru.dropout_bt_mask`` for the dropout masks.  Round-off bounds are 10x (or less) what was measured on the MI355X; the
measured values are printed (-rP) and recorded in profiles/r09_tcn_parity_measured.txt."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests.tcn_cases import GOLDEN, TCNRestated, golden_case, layer_case, layer_inputs, rel, sampled_rel

gpu = pytest.mark.gpu
DEV = "cuda:0"
_MD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
_MT = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}
_MODES = ["fp32", "bf16", "fp16"]
# (B, T, Cin, Cout, k, d): one row and one tap; (k-1) d >= T; M tiles that span samples (T = 33, 67, 19 against 64-row tiles) with
# K tails (k Cin = 80, 192, 60 against 32- / 64-deep stages) and Cin = 40 rows (160 B: 16-B, not 64-B aligned); channel counts
# below a tile (12 -> 20); more than one row range in the weight gradient (B T = 260); three column tiles and K = 768
_SHAPES = [(1, 1, 4, 4, 1, 1), (2, 5, 40, 64, 3, 4), (5, 33, 40, 64, 2, 1), (3, 67, 64, 128, 3, 2), (3, 19, 12, 20, 5, 3),
           (2, 130, 128, 256, 3, 4), (2, 70, 256, 256, 3, 4)]
_IDS = ["-".join(map(str, s)) for s in _SHAPES]
_LAYER_REF = {}


def _layer_ref(shape, integer, mode, relu, residual):
    """Inputs and the restated layer, computed once per (shape, data kind, rounding, epilogue)."""
    key = (shape, integer, _MT[mode] if not integer else None, relu, residual)
    B, T, Cin, Cout, k, d = shape
    d_in = layer_inputs(B, T, Cin, Cout, k, seed=sum(shape) + 17 * int(integer), integer=integer)
    if key not in _LAYER_REF:
        _LAYER_REF[key] = layer_case(d_in["x"], d_in["w"], d_in["b"], d_in["dy"], d, relu=relu, residual=d_in["res"] if residual else None,
                                     mtype=key[2])
    return d_in, _LAYER_REF[key]


def _layer_gpu(d_in, d, mode, relu, residual, **kw):
    from wakeword_trainer_home_amd import _native as nat
    f = lambda t: t.float().to(DEV)
    x, w, b, dy = f(d_in["x"]), f(d_in["w"]), f(d_in["b"]), f(d_in["dy"])
    y = nat.tconv1d_fwd(x, w, b, d, relu=relu, residual=f(d_in["res"]) if residual else None, mode=_MD[mode])
    dx, dw, db = nat.tconv1d_bwd(x, w, dy, d, y=y if relu else None, mode=_MD[mode], **kw)
    return dict(y=y, dx=dx, dw=dw, db=db)


# ------------------------------------------------------------------------------------------ the layer
@gpu
@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("shape", _SHAPES, ids=_IDS)
def test_layer_is_exact_on_integer_data(shape, mode):
    """Integer-valued x, dy, residual in [-4, 4], W in [-2, 2] and bias: every product and sum is exact in fp32 and in the 16-bit
    operand types, so y, dx, dw and db equal the float64 restatement BIT FOR BIT in every mode -- plain, with the ReLU epilogue
    and with the "add the residual, then ReLU" epilogue.  Also: dx added to a given tensor, and no dx at all."""
    from wakeword_trainer_home_amd import _native as nat
    d = shape[5]
    for relu, residual in ((False, False), (True, False), (True, True), (False, True)):
        d_in, ref = _layer_ref(shape, True, mode, relu, residual)
        got = _layer_gpu(d_in, d, mode, relu, residual)
        for n in ("y", "dx", "dw", "db"):
            assert torch.equal(got[n].cpu().double(), ref[n]), (n, relu, residual, (got[n].cpu().double() - ref[n]).abs().max().item())
    # accumulate into dx / skip dx (the last epilogue's tensors)
    f = lambda t: t.float().to(DEV)
    base = torch.full_like(f(d_in["x"]), 3.0)
    dx2, dw2, db2 = nat.tconv1d_bwd(f(d_in["x"]), f(d_in["w"]), f(d_in["dy"]), d, mode=_MD[mode], dx=base)
    assert dx2 is base and torch.equal(base.cpu().double(), ref["dx"] + 3.0)
    dx3, dw3, db3 = nat.tconv1d_bwd(f(d_in["x"]), f(d_in["w"]), f(d_in["dy"]), d, mode=_MD[mode], need_dx=False)
    assert dx3 is None and torch.equal(dw3, dw2) and torch.equal(db3, db2) and torch.equal(dw3.cpu().double(), ref["dw"])


@gpu
@pytest.mark.parametrize("mode", _MODES)
def test_layer_masks_with_two_saved_outputs_and_a_scale(mode):
    """The block's conv2: dpre = dy * scale where y != 0 and y2 != 0 (scale a power of two: still exact)."""
    from wakeword_trainer_home_amd import _native as nat
    from tests.tcn_cases import conv_bwd
    shape = _SHAPES[3]
    B, T, Cin, Cout, k, d = shape
    d_in, _ = _layer_ref(shape, True, mode, False, False)
    g = torch.Generator().manual_seed(3)
    y1 = torch.randint(-1, 2, (B, T, Cout), generator=g).double()
    y2 = torch.randint(0, 2, (B, T, Cout), generator=g).double()
    f = lambda t: t.float().to(DEV)
    dx, dw, db = nat.tconv1d_bwd(f(d_in["x"]), f(d_in["w"]), f(d_in["dy"]), d, y=f(y1), y2=f(y2), mask_scale=2.0, mode=_MD[mode])
    rx, rw, rb = conv_bwd(d_in["x"], d_in["w"], d_in["dy"] * 2.0 * (y1 != 0) * (y2 != 0), d)
    assert torch.equal(dx.cpu().double(), rx) and torch.equal(dw.cpu().double(), rw) and torch.equal(db.cpu().double(), rb)


@gpu
@pytest.mark.parametrize("mode", _MODES)
def test_deferred_weight_gradient_equals_immediate(mode):
    """B T = 260: two row ranges.  Under ww_ctx_set_deferred_reduce the sum of the partial products is queued (one item) and
    run by the flush; on integer data both orders of summation are exact, so the results are equal bit for bit."""
    from wakeword_trainer_home_amd import _native as nat
    shape = _SHAPES[5]
    d_in, ref = _layer_ref(shape, True, mode, False, False)
    lib, cx = nat.load(), nat.ctx(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    slot_w = torch.full(tuple(d_in["w"].shape), float("nan"), device=DEV)
    slot_b = torch.full((shape[3],), float("nan"), device=DEV)
    got = _layer_gpu(d_in, shape[5], mode, False, False, dw_out=slot_w, db_out=slot_b, defer=True)
    assert lib.ww_deferred_reduce_pending(cx) == 1
    nat.deferred_flush(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    torch.cuda.synchronize()
    assert got["dw"] is slot_w and torch.equal(slot_w.cpu().double(), ref["dw"]) and torch.equal(slot_b.cpu().double(), ref["db"])


# Round-off of the layer on N(0,1) data, linear epilogue (no ReLU: no mask flips), against the restatement that rounds what the mode
# rounds: the error of y and dx relative to the largest |entry| of the tensor, of dw and db likewise.  Bounds: 10x the largest
# value measured over the three shapes -- fp32 1.03e-6, bf16 3.52e-7, fp16 5.75e-7 (profiles/r09_tcn_parity_measured.txt).  The fp32
# figures are of the order the MFMA f32 chain predicts (1e-7 sum|a b|); in the 16-bit modes only the fp32 accumulation order
# separates device and restatement.
_LAYER_BOUND = {"fp32": 1.0e-5, "bf16": 3.5e-6, "fp16": 5.7e-6}


@gpu
@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("shape", _SHAPES[-3:], ids=_IDS[-3:])
def test_layer_roundoff_against_restatement(shape, mode):
    d_in, ref = _layer_ref(shape, False, mode, False, False)
    got = _layer_gpu(d_in, shape[5], mode, False, False)
    errs = {n: rel(got[n].cpu().double(), ref[n]) for n in ("y", "dx", "dw", "db")}
    print(f"tcn-layer roundoff {'-'.join(map(str, shape))} {mode}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for n, e in errs.items():
        assert e <= _LAYER_BOUND[mode], (n, e)


# ------------------------------------------------------------------------------------------ the model
def _spy_conv_outputs(monkeypatch):
    """Record every ww_tconv1d_fwd output of the model's forward: per block h1, h2, out."""
    from wakeword_trainer_home_amd import _native as nat
    seen, orig = [], nat.tconv1d_fwd

    def spy(*a, **k):
        y = orig(*a, **k)
        seen.append(y)
        return y
    monkeypatch.setattr(nat, "tconv1d_fwd", spy)
    return seen


# fp32 model against the reference fixture: (eval | train logits absolute, loss absolute, gradients relative to the reference
# gradient's largest entry, at the fixture's samples and whole against the restatement); 10x the largest value measured over both
# cases and the two orientation inputs: logits 2.98e-8, loss 5.96e-8, gradients 2.90e-6 (profiles/r09_tcn_parity_measured.txt)
_MODEL_BOUND = dict(logits=2.9e-7, loss=5.9e-7, grads=2.9e-5)
_CASES = [("", {}), ("small.", dict(num_channels=[32, 48], kernel_size=2))]


@gpu
@pytest.mark.parametrize("prefix,kw", _CASES)
def test_tcnwakeword_matches_reference_fixture(prefix, kw, monkeypatch):
    """tests/golden/g10_tcn.npz was produced by the reference's own TCNWakeword, on inputs whose float64 ReLU inputs all keep
    >= 1e-6 from zero: EVERY ReLU decision of the fp32 device run equals the float64 restatement's, and the eval and train
    logits, the loss and every parameter gradient meet the fixture within fp32 round-off."""
    from wakeword_trainer_home_amd.models import TCNWakeword
    sd, g = golden_case(prefix)
    model = TCNWakeword(dropout=0.0, **kw)
    model.load_state_dict(sd)
    model.to(DEV)
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)          # (B, F, T)
    oracle = TCNRestated(sd)
    _, _, go, _ = oracle.loss_and_grads(torch.from_numpy(g["x"]).double().transpose(1, 2), torch.from_numpy(g["y"]))
    model.eval()
    with torch.no_grad():
        ev = model(x)
    model.train()
    seen = _spy_conv_outputs(monkeypatch)
    out = model(x)
    assert len(seen) == len(oracle.relu_masks)
    flips = [int(((a != 0).cpu() != m).sum()) for a, m in zip(seen, oracle.relu_masks)]
    loss = torch.nn.functional.cross_entropy(out, y)
    loss.backward()
    e_ev = (ev.cpu() - torch.from_numpy(g["logits_eval"])).abs().max().item()
    e_tr = (out.detach().cpu() - torch.from_numpy(g["logits_train"])).abs().max().item()
    e_loss = abs(loss.item() - float(g["loss"]))
    e_s = {n: sampled_rel(p.grad, g, n) for n, p in model.named_parameters()}
    e_w = {n: (p.grad.cpu().double() - go[n]).abs().max().item() / g["gmax"][n] for n, p in model.named_parameters()}
    print(f"tcn-model fixture '{prefix}': ReLU flips {sum(flips)} (margin {float(g['relu_margin']):.2e}) eval {e_ev:.2e} train {e_tr:.2e} "
          f"loss {e_loss:.2e} grads sampled {max(e_s.values()):.2e} whole {max(e_w.values()):.2e}")
    assert sum(flips) == 0, flips
    assert e_ev <= _MODEL_BOUND["logits"] and e_tr <= _MODEL_BOUND["logits"] and e_loss <= _MODEL_BOUND["loss"]
    for n in e_s:
        assert e_s[n] <= _MODEL_BOUND["grads"] and e_w[n] <= _MODEL_BOUND["grads"], (n, e_s[n], e_w[n])
    # the Trainer's (B,1,F,T) feature batches and (B,T,F) sequences give the same logits as (B,F,T)
    with torch.no_grad():
        model.eval()
        assert torch.equal(model(x[:, None].contiguous()), ev)
        assert torch.equal(model(x.transpose(1, 2).contiguous()), ev)


@gpu
def test_public_forward_reads_orientations_as_the_reference_does():
    """The reference's own ``forward`` on (4,37,40) (it transposes: (B,T,F)) and on the square (2,40,40) (it does not: (B,F,T))."""
    from wakeword_trainer_home_amd.models import TCNWakeword
    sd, _ = golden_case("")
    g = np.load(GOLDEN)
    model = TCNWakeword()
    model.load_state_dict(sd)
    model.to(DEV).eval()
    with torch.no_grad():
        for name in ("btf", "sq"):
            got = model(torch.from_numpy(g[f"fwd.x_{name}"]).to(DEV)).cpu()
            e = (got - torch.from_numpy(g[f"fwd.logits_{name}"])).abs().max().item()
            print(f"tcn-model forward {name}: {e:.2e}")
            assert e <= _MODEL_BOUND["logits"], (name, e)
        with pytest.raises(ValueError):
            model(torch.zeros(2, 39, 41, device=DEV))


# dropout 0.3, fp32: (logits absolute, loss absolute, gradients and dx relative to their largest entry); 10x the larger value
# measured over the two models: logits 6.24e-8, loss 5.77e-8, gradients 4.81e-7 (profiles/r09_tcn_parity_measured.txt)
_DROP_BOUND = dict(logits=6.2e-7, loss=5.7e-7, grads=4.8e-6)


@gpu
@pytest.mark.parametrize("channels", [[64, 128, 256], [32, 32]], ids=["default", "identity-skip"])
def test_tcnwakeword_with_dropout_matches_restatement(channels):
    """Training forwards with dropout 0.3 against the restatement that draws oracle.gru.dropout_bt_mask with streams 16 + 2i,
    17 + 2i and 15; two consecutive forwards draw different masks (the Philox step advances)."""
    from wakeword_trainer_home_amd.models import TCNWakeword
    torch.manual_seed(len(channels))
    model = TCNWakeword(num_channels=channels, dropout=0.3, dropout_seed=21).to(DEV)
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    oracle = TCNRestated(sd, dropout=0.3, seed=21)
    B, T = 6, 23
    x = torch.randn(B, T, 40)
    y = torch.randint(0, 2, (B,))
    model.train()
    model.sample_offset = 5
    outs, worst = [], dict(logits=0.0, loss=0.0, grads=0.0)
    for step in range(2):
        xd = x.to(DEV).requires_grad_(True)
        out = model(xd)
        loss = torch.nn.functional.cross_entropy(out, y.to(DEV))
        model.zero_grad()
        loss.backward()
        ref, lo, go, dxo = oracle.loss_and_grads(x.double(), y, step=step, sample_offset=5)
        outs.append(out.detach().cpu())
        worst["logits"] = max(worst["logits"], (out.detach().cpu().double() - ref).abs().max().item())
        worst["loss"] = max(worst["loss"], abs(loss.item() - lo))
        worst["grads"] = max([worst["grads"], rel(xd.grad.cpu().double(), dxo)] +
                             [rel(p.grad.cpu().double(), go[n]) for n, p in model.named_parameters()])
    print(f"tcn-model dropout {channels}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert not torch.equal(outs[0], outs[1])
    for k, v in worst.items():
        assert v <= _DROP_BOUND[k], (k, v)


# whole model in the 16-bit modes at B = 4, T = 45 against the rounding restatement (the fixture's default case, dropout 0):
# (logits absolute, loss absolute, gradients relative to their largest entry, gradients as |got - ref|_2 / |ref|_2 per tensor); 10x
# measured (profiles/r09_tcn_parity_measured.txt).  A ReLU input within fp32 accumulation round-off of zero may decide differently on
# the device (the count is printed, not asserted).  Measured: bf16 no flip, fp16 one -- a flipped unit moves its bias gradient
# entry by the whole of that entry, which is what the fp16 "grads" figure (4.4e-2, against bf16's 6.0e-4) is; the norm figure
# (bf16 2.2e-4, fp16 7.1e-3) weighs such an entry by its share of the tensor.
_MODEL16_BOUND = {"bf16": dict(logits=5.3e-5, loss=8.8e-6, grads=6.0e-3, grads_l2=2.2e-3),
                  "fp16": dict(logits=7.8e-6, loss=5.2e-7, grads=4.3e-1, grads_l2=7.0e-2)}


@gpu
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_tcnwakeword_16bit_modes_match_rounding_restatement(mode, monkeypatch):
    from wakeword_trainer_home_amd.models import TCNWakeword
    sd, g = golden_case("")
    model = TCNWakeword(dropout=0.0, mode=mode)
    model.load_state_dict(sd)
    model.to(DEV).train()
    oracle = TCNRestated(sd, mtype=_MT[mode])
    ref, lo, go, _ = oracle.loss_and_grads(torch.from_numpy(g["x"]).double().transpose(1, 2), torch.from_numpy(g["y"]))
    seen = _spy_conv_outputs(monkeypatch)
    out = model(torch.from_numpy(g["x"]).to(DEV))
    flips = sum(int(((a != 0).cpu() != m).sum()) for a, m in zip(seen, oracle.relu_masks))
    loss = torch.nn.functional.cross_entropy(out, torch.from_numpy(g["y"]).to(DEV))
    loss.backward()
    errs = dict(logits=(out.detach().cpu().double() - ref).abs().max().item(), loss=abs(loss.item() - lo),
                grads=max(rel(p.grad.cpu().double(), go[n]) for n, p in model.named_parameters()),
                grads_l2=max(((p.grad.cpu().double() - go[n]).norm() / go[n].norm()).item() for n, p in model.named_parameters()))
    print(f"tcn-model {mode}: ReLU flips {flips} of {sum(m.numel() for m in oracle.relu_masks)} " +
          " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= _MODEL16_BOUND[mode][k], (k, v)


# ------------------------------------------------------------------------------------------ the Trainer
def _trainer_cfg(batch_size=8, epochs=1):
    from wakeword_trainer_home_amd.config import get_preset
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = epochs, 0, batch_size
    cfg.loss.label_smoothing = 0.0
    return cfg


@gpu
def test_trainer_drives_tcnwakeword(tmp_path):
    """train_epoch / validate_epoch on waveform batches (native front end -> (8,1,40,T) features -> TCNWakeword -> native loss,
    the sync-free step with the fused clip + optimizer); the first-step loss equals the CPU pipeline's
    (oracle.train_step.frontend -> the float64 restatement) within 1e-3."""
    from wakeword_trainer_home_amd.models import TCNWakeword
    from wakeword_trainer_home_amd.training import Trainer
    from wakeword_trainer_home_amd.training.optimizer_factory import FlatFusedOptimizer
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from oracle.train_step import frontend
    cfg = _trainer_cfg()
    torch.manual_seed(9)
    model = TCNWakeword(dropout=0.0)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    wave, y = make_synthetic_batch(24, 7040, seed=5)                 # 7040 samples: 45 frames
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
    assert tuple(x0.shape) == (8, 1, 40, 45)
    _, ref, _, _ = TCNRestated(sd).loss_and_grads(x0[:, 0].transpose(1, 2), batches[0][1])
    assert abs(losses[0] - ref) < 1e-3, (losses[0], ref)
    loss, m = t.validate_epoch(0)
    assert m.total_samples == 8 and np.isfinite(loss)


@gpu
def test_graph_replays_equal_eager_steps_bit_for_bit(tmp_path):
    """hip_graph=True: the captured step (forward, loss, backward with deferred partial sums, gather, fused clip + optimizer)
    replayed over two epochs of 4 full batches and a ragged one (8, 8, 8, 8, 5 rows) equals the eager steps bit for bit: loss
    trace, every parameter and the optimizer moments.  Dropout 0.3: the replays draw fresh masks."""
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.models import TCNWakeword
    from wakeword_trainer_home_amd.training import Trainer
    wave, y = make_synthetic_batch(37, 7040, seed=6)
    y[::3] = 1
    batches = [(wave[8 * i:8 * i + 8], y[8 * i:8 * i + 8]) for i in range(5)]
    assert len(batches[-1][0]) == 5
    runs = []
    for graph in (False, True):
        cfg = _trainer_cfg(epochs=2)
        cfg.optimizer.mixed_precision = False
        cfg.training.hip_graph, cfg.training.hip_graph_auto = graph, False
        cfg.training.checkpoint_frequency = "best_only"
        torch.manual_seed(11)
        model = TCNWakeword(dropout=0.3, dropout_seed=2)
        t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path / f"g{int(graph)}", device=DEV)
        rec = []
        t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: rec.append((i, l))})())
        res = t.train()
        runs.append((t, rec, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                     copy.deepcopy(t.optimizer.state_dict()), res))
    assert runs[1][0]._graph is not None and runs[0][0]._graph is None
    assert len(runs[1][1]) == 10
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
    from wakeword_trainer_home_amd.models import TCNWakeword
    from wakeword_trainer_home_amd.training import Trainer
    cfg = _trainer_cfg()
    torch.manual_seed(2)
    model = TCNWakeword(dropout=0.0)
    wave, y = make_synthetic_batch(24, 7040, seed=6)
    bad = wave[8:16].clone()
    bad[3, 100] = float("nan")
    batches = [(wave[:8], y[:8]), (bad, y[8:16]), (wave[16:], y[16:])]
    t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path, device=DEV)
    assert t._async_autograd and t.deferred_metrics
    seen = []
    t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: seen.append((i, l))})())
    snaps = []
    orig = t._step_autograd_async

    def spy(inputs, targets, idx):
        snaps.append({k: v.clone() for k, v in model.state_dict().items()})
        return orig(inputs, targets, idx)
    t._step_autograd_async = spy
    t.train_epoch(0)
    after = {k: v.clone() for k, v in model.state_dict().items()}
    assert [i for i, _ in seen] == [0, 2] and all(np.isfinite(l) for _, l in seen)
    assert any(not torch.equal(snaps[0][k], snaps[1][k]) for k in snaps[0])
    assert all(torch.equal(snaps[1][k], snaps[2][k]) for k in snaps[1])
    assert any(not torch.equal(snaps[2][k], after[k]) for k in after)


# ------------------------------------------------------------------------------------------ argument checks
@gpu
def test_argument_checks_return_error_codes():
    """Channel counts that are no multiple of 4, k = 0 or 9, a dilation of 0 and a short scratch region come back as error codes
    (with a message in ww_last_error) before any launch; the bindings raise WW_E_INVALID as ValueError, the others as NativeError."""
    from wakeword_trainer_home_amd import _native as nat
    lib, cx = nat.load(), nat.ctx(DEV)
    B, T, Cin, Cout, k = 2, 5, 8, 12, 3
    z = lambda *s: torch.zeros(*s, device=DEV)
    x, w, b, y = z(B, T, Cin), z(Cout, Cin, k), z(Cout), torch.full((B, T, Cout), 7.0, device=DEV)
    nbytes = lib.ww_tconv1d_scratch_bytes(B, T, Cin, Cout, k)
    scratch = z(nbytes // 4)
    p = lambda t: C.c_void_p(t.data_ptr())
    fwd = lambda cin, cout, kk, d, sb: lib.ww_tconv1d_fwd(cx, 0, p(x), p(w), p(b), B, T, cin, cout, kk, d, 0, None, p(y), p(scratch), sb, None)
    assert fwd(6, Cout, k, 1, nbytes) == -1 and b"multiples of 4" in lib.ww_last_error()
    assert fwd(Cin, 10, k, 1, nbytes) == -1
    assert fwd(Cin, Cout, 0, 1, nbytes) == -1 and b"kernel_size" in lib.ww_last_error()
    assert fwd(Cin, Cout, 9, 1, nbytes) == -1
    assert fwd(Cin, Cout, k, 0, nbytes) == -1 and b"dilation" in lib.ww_last_error()
    assert fwd(Cin, Cout, k, 1, nbytes - 4) == -3 and b"scratch too small" in lib.ww_last_error()
    assert lib.ww_tconv1d_fwd(cx, 7, p(x), p(w), p(b), B, T, Cin, Cout, k, 1, 0, None, p(y), p(scratch), nbytes, None) == -1    # mode
    bwd = lambda cin, kk, sb: lib.ww_tconv1d_bwd(cx, 0, p(x), p(w), None, None, 1.0, p(y), B, T, cin, Cout, kk, 1, None, 0, p(w), p(b),
                                                 p(scratch), sb, None)
    assert bwd(6, k, nbytes) == -1 and bwd(Cin, 9, nbytes) == -1 and bwd(Cin, 0, nbytes) == -1 and bwd(Cin, k, 16) == -3
    torch.cuda.synchronize()
    assert y.eq(7.0).all() and w.eq(0).all() and b.eq(0).all()          # nothing was launched
    with pytest.raises(ValueError, match="multiples of 4"):
        nat.tconv1d_fwd(z(B, T, 6), z(Cout, 6, k), b)
    with pytest.raises(ValueError, match="kernel_size"):
        nat.tconv1d_fwd(x, z(Cout, Cin, 9), b)
    with pytest.raises(ValueError):
        nat.tconv1d_fwd(x, z(Cout, Cin + 4, k), b)                       # x and weight disagree about Cin: caught at the binding
