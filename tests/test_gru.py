"""GRU layer kernels against torch.nn.GRU on the CPU in float64 -- the module the reference's
GRUWakeword wraps (src/models/architectures.py:228-235), so its arithmetic IS the reference's.  fp32 device vs float64:
outputs <= 2e-5 abs (76 recurrent steps of fp32 sigmoid/tanh), gradients <= 2e-4 relative to each tensor's largest entry."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


@pytest.fixture(params=[8, 16])
def gru_rows(request, monkeypatch):
    """Both workgroup shapes of the recurrent kernels (8 or 16 batch rows per workgroup; the library picks by batch size)."""
    monkeypatch.setenv("WW_GRU_ROWS", str(request.param))
    return request.param


@pytest.mark.parametrize("B,T,I", [(5, 7, 40), (33, 76, 64), (16, 3, 9), (70, 20, 256)])
@pytest.mark.parametrize("reverse", [False, True])
def test_gru_direction_matches_torch(B, T, I, reverse, gru_rows):
    from wakeword_trainer_home_amd import _native as nat
    H = 128
    torch.manual_seed(B + T)
    ref = torch.nn.GRU(I, H, num_layers=1, batch_first=True, bidirectional=True).double()
    sfx = "_reverse" if reverse else ""
    w_ih, w_hh = getattr(ref, "weight_ih_l0" + sfx), getattr(ref, "weight_hh_l0" + sfx)
    b_ih, b_hh = getattr(ref, "bias_ih_l0" + sfx), getattr(ref, "bias_hh_l0" + sfx)
    x = torch.randn(B, T, I, dtype=torch.float64, requires_grad=True)
    h0 = torch.randn(2, B, H, dtype=torch.float64) * 0.3
    out, hn = ref(x, h0)
    sl = slice(H, 2 * H) if reverse else slice(0, H)
    dy = torch.randn(B, T, H, dtype=torch.float64)
    dhn = torch.randn(B, H, dtype=torch.float64)
    loss = (out[:, :, sl] * dy).sum() + (hn[1 if reverse else 0] * dhn).sum()
    loss.backward()

    f = lambda t: t.detach().float().to(DEV)
    ybuf = torch.zeros(B, T, 2 * H, device=DEV)                     # the direction writes its half of a (B,T,2H) buffer
    ws = nat.gru_workspace(B, T, I, H, DEV)
    xd = f(x)
    h_n = nat.gru_fwd(xd, f(w_ih), f(w_hh), f(b_ih), f(b_hh), ybuf[:, :, sl], ws, h0=f(h0[1 if reverse else 0]), reverse=reverse)
    assert (ybuf[:, :, sl].cpu().double() - out[:, :, sl].detach()).abs().max().item() <= 2e-5
    assert (h_n.cpu().double() - hn[1 if reverse else 0].detach()).abs().max().item() <= 2e-5
    other = slice(0, H) if reverse else slice(H, 2 * H)
    assert ybuf[:, :, other].abs().max().item() == 0.0             # nothing written outside its half
    dybuf = torch.zeros(B, T, 2 * H, device=DEV)
    dybuf[:, :, sl] = f(dy)
    dx = torch.full((B, T, I), 1.0, device=DEV)
    dw_ih, dw_hh, db_ih, db_hh, dh0 = nat.gru_bwd(xd, f(w_ih), f(w_hh), dybuf[:, :, sl], f(dhn), ws, reverse=reverse, dx=dx,
                                                  accumulate_dx=True, want_dh0=True)
    tol = 2e-4
    assert _rel(dx.cpu().double() - 1.0, x.grad) <= tol                  # accumulated onto the ones
    assert _rel(dw_ih.cpu().double(), w_ih.grad) <= tol
    assert _rel(dw_hh.cpu().double(), w_hh.grad) <= tol
    assert _rel(db_ih.cpu().double(), b_ih.grad) <= tol
    assert _rel(db_hh.cpu().double(), b_hh.grad) <= tol
    # dh0 = d loss / d h0 of this direction
    h0g = h0.clone().requires_grad_(True)
    out2, hn2 = ref(x.detach(), h0g)
    ((out2[:, :, sl] * dy).sum() + (hn2[1 if reverse else 0] * dhn).sum()).backward()
    assert _rel(dh0.cpu().double(), h0g.grad[1 if reverse else 0]) <= tol


@pytest.mark.parametrize("B,T,I", [(5, 7, 40), (33, 76, 64), (70, 20, 256)])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_gru_bidirectional_layer_in_one_launch(B, T, I, mode, gru_rows):
    """ww_gru_bidir_fwd/bwd (both directions as the two rows of ONE recurrent launch) against float64 torch.nn.GRU
    (bidirectional=True) in the fp32 mode, and BIT-identical to the two per-direction launches it replaces in either mode
    (same kernels, same per-direction arithmetic) -- except dx: one product over both directions' (dGi, W_ih) pairs here, a
    product plus an accumulating one there: the same terms in another order of fp32 additions."""
    from wakeword_trainer_home_amd import _native as nat
    H = 128
    torch.manual_seed(B * T)
    ref = torch.nn.GRU(I, H, num_layers=1, batch_first=True, bidirectional=True).double()
    x = torch.randn(B, T, I, dtype=torch.float64, requires_grad=True)
    out, hn = ref(x)
    dy = torch.randn(B, T, 2 * H, dtype=torch.float64)
    dhn = torch.randn(2, B, H, dtype=torch.float64)
    ((out * dy).sum() + (hn * dhn).sum()).backward()
    f = lambda t: t.detach().float().to(DEV)
    m = {"fp32": torch.float32, "bf16": torch.bfloat16}[mode]
    names = [["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"], ["weight_ih_l0_reverse", "weight_hh_l0_reverse",
                                                                            "bias_ih_l0_reverse", "bias_hh_l0_reverse"]]
    params = [[f(getattr(ref, n)) for n in ns] for ns in names]
    xd, dyd = f(x), f(dy)
    ws = [nat.gru_workspace(B, T, I, H, DEV) for _ in range(2)]
    y = torch.zeros(B, T, 2 * H, device=DEV)
    h_n = nat.gru_bidir_fwd(xd, params, y, ws, mode=m)
    dx = torch.zeros(B, T, I, device=DEV)
    grads = nat.gru_bidir_bwd(xd, params, dyd, [f(dhn[0]), f(dhn[1])], ws, dx=dx, mode=m)
    # the per-direction launches
    ws1 = [nat.gru_workspace(B, T, I, H, DEV) for _ in range(2)]
    y1 = torch.zeros(B, T, 2 * H, device=DEV)
    h1 = [nat.gru_fwd(xd, *params[d], y1[:, :, d * H:(d + 1) * H], ws1[d], reverse=(d == 1), mode=m) for d in range(2)]
    dx1 = torch.zeros(B, T, I, device=DEV)
    g1 = [nat.gru_bwd(xd, params[d][0], params[d][1], dyd[:, :, d * H:(d + 1) * H], f(dhn[d]), ws1[d], reverse=(d == 1), dx=dx1,
                      accumulate_dx=(d == 1), mode=m) for d in range(2)]
    assert torch.equal(y, y1) and torch.equal(h_n[0], h1[0]) and torch.equal(h_n[1], h1[1])
    ddx = (dx - dx1).abs().max().item() / max(dx1.abs().max().item(), 1e-30)
    print(f"bidirectional dx, one product vs product + accumulate: max |diff| / max |dx| = {ddx:.2e}")
    assert ddx <= 2e-6
    for d in range(2):
        for a, b in zip(grads[d], g1[d][:4]):
            assert torch.equal(a, b)
    if mode == "fp32":
        assert (y.cpu().double() - out.detach()).abs().max().item() <= 2e-5
        assert (torch.stack(h_n).cpu().double() - hn.detach()).abs().max().item() <= 2e-5
        assert _rel(dx.cpu().double(), x.grad) <= 2e-4
        for d in range(2):
            for a, n in zip(grads[d], names[d]):
                assert _rel(a.cpu().double(), getattr(ref, n).grad) <= 2e-4, n


def test_gru_argument_checks():
    from wakeword_trainer_home_amd import _native as nat
    with pytest.raises(nat.NativeError, match="128 only"):
        nat.gru_workspace(4, 5, 8, 64, DEV)
    ws = nat.gru_workspace(4, 5, 8, 128, DEV)
    x = torch.zeros(4, 5, 8, device=DEV)
    w_ih, w_hh = torch.zeros(384, 8, device=DEV), torch.zeros(384, 128, device=DEV)
    b = torch.zeros(384, device=DEV)
    with pytest.raises(ValueError):
        nat.gru_fwd(x, w_ih, w_hh, b, b, torch.zeros(4, 5, 64, device=DEV), ws)
    with pytest.raises(nat.NativeError):
        nat.gru_fwd(x, w_ih, w_hh, b, b, torch.zeros(4, 5, 128, device=DEV), ws[:100])       # workspace too small
    with pytest.raises(ValueError):
        nat.gru_fwd(x.transpose(0, 1), w_ih, w_hh, b, b, torch.zeros(5, 4, 128, device=DEV), ws)
    y = torch.zeros(4, 5, 128, device=DEV)
    with pytest.raises(ValueError):                                        # h0 of the wrong batch size
        nat.gru_fwd(x, w_ih, w_hh, b, b, y, ws, h0=torch.zeros(3, 128, device=DEV))
    with pytest.raises(ValueError):                                        # h0 not float32
        nat.gru_fwd(x, w_ih, w_hh, b, b, y, ws, h0=torch.zeros(4, 128, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(ValueError):                                        # dh_n of the wrong shape
        nat.gru_bwd(x, w_ih, w_hh, y, torch.zeros(4, 64, device=DEV), ws)
    # the C entry points themselves (WW_E_INVALID = -1), before any launch
    import ctypes as C
    lib, cx, p = nat.load(), nat.ctx(DEV), lambda t: C.c_void_p(t.data_ptr())
    B, T, I, H = 4, 5, 8, 128
    assert lib.ww_gru_bwd(cx, 0, p(x), I, p(w_ih), p(w_hh), p(y), H - 4, None, B, T, I, H, 0, p(ws), ws.numel() * 4, None, I, 0,
                          p(w_ih), p(w_hh), p(b), p(b), None, None) == -1           # dy row stride smaller than H
    gw, gb = torch.zeros(384, 8, device=DEV), torch.zeros(384, device=DEV)
    dirs = (nat.GruDir * 2)()
    for k in range(2):
        dirs[k].w_ih, dirs[k].w_hh, dirs[k].ws = w_ih.data_ptr(), w_hh.data_ptr(), ws.data_ptr()       # one workspace for both
        dirs[k].dw_ih, dirs[k].dw_hh, dirs[k].db_ih, dirs[k].db_hh = gw.data_ptr(), w_hh.data_ptr(), gb.data_ptr(), b.data_ptr()
    y2 = torch.zeros(B, T, 2 * H, device=DEV)
    assert lib.ww_gru_bidir_bwd(cx, 0, p(x), I, C.byref(dirs), p(y2), 2 * H, B, T, I, H, ws.numel() * 4, None, I, None) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ model level
def _golden():
    from pathlib import Path
    return np.load(Path(__file__).parent / "golden" / "g7_gru.npz")


def _sd_from_golden(g):
    return {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}


def test_gruwakeword_matches_reference_fixture():
    """tests/golden/g7_gru.npz was produced by the reference's own GRUWakeword (make_golden.py g7): same state_dict keys,
    eval logits, training loss and every parameter gradient."""
    from wakeword_trainer_home_amd.models import create_model
    g = _golden()
    sd = _sd_from_golden(g)
    model = create_model("gru", num_classes=2, input_size=40, hidden_size=128, num_layers=2, bidirectional=True, dropout=0.0)
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.load_state_dict(sd)
    model.to(DEV)
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    model.eval()
    with torch.no_grad():
        ev = model(x)
    assert (ev.cpu() - torch.from_numpy(g["logits_eval"])).abs().max().item() <= 2e-5
    model.train()
    out = model(x)
    loss = torch.nn.functional.cross_entropy(out, y)
    loss.backward()
    assert abs(loss.item() - float(g["loss"])) <= 1e-5
    for n, p in model.named_parameters():
        ref = torch.from_numpy(g["grad." + n])
        assert _rel(p.grad.cpu(), ref) <= 5e-4, n
    # (B,1,F,T) feature batches, as the Trainer produces them, give the same logits
    with torch.no_grad():
        model.eval()
        ev4 = model(x.transpose(1, 2)[:, None].contiguous())
    assert torch.equal(ev4, ev)


@pytest.mark.parametrize("layers,bidir", [(2, True), (1, True), (2, False)])
def test_gruwakeword_with_dropout_matches_oracle(layers, bidir):
    from wakeword_trainer_home_amd.models import create_model
    from oracle.gru import GRUWakewordOracle
    torch.manual_seed(layers * 3 + int(bidir))
    model = create_model("gru", input_size=40, num_layers=layers, bidirectional=bidir, dropout=0.3, dropout_seed=21).to(DEV)
    oracle = GRUWakewordOracle(40, 128, layers, 2, bidir, dropout=0.3, seed=21)
    oracle.load_reference_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    B, T = 9, 23
    x = torch.randn(B, T, 40)
    y = torch.randint(0, 2, (B,))
    model.train()
    model.sample_offset = 5
    for step in range(2):
        xd = x.to(DEV).requires_grad_(True)
        out = model(xd)
        loss = torch.nn.functional.cross_entropy(out, y.to(DEV))
        model.zero_grad()
        loss.backward()
        xo = x.double().requires_grad_(True)
        ref = oracle(xo, step=step, sample_offset=5, training=True)
        lo = torch.nn.functional.cross_entropy(ref, y)
        oracle.zero_grad()
        lo.backward()
        assert (out.detach().cpu().double() - ref.detach()).abs().max().item() <= 5e-5, step
        assert _rel(xd.grad.cpu().double(), xo.grad) <= 5e-4
        nd = 2 if bidir else 1
        for k in range(layers):
            for sfx in ("", "_reverse")[:nd]:
                for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    gd = getattr(model.gru, f"{name}_l{k}{sfx}").grad.cpu().double()
                    go = getattr(oracle.layers[k], f"{name}_l0{sfx}").grad
                    assert _rel(gd, go) <= 5e-4, (step, name, k, sfx)
        assert _rel(model.fc[1].weight.grad.cpu().double(), oracle.fc.weight.grad) <= 5e-4


@pytest.mark.parametrize("act", ["fp32", "bf16"])
def test_crnn_matches_oracle(act):
    """conv front-end + frequency pooling + GRU against oracle/crnn.py (torch.nn conv stack + nn.GRU, float64)."""
    from wakeword_trainer_home_amd.models import create_model
    from oracle.crnn import CRNNOracle
    from tests.golden_util import make_inputs
    torch.manual_seed(3)
    model = create_model("crnn", dropout=0.3, dropout_seed=4, act_dtype=act).to(DEV)
    keys = list(model.state_dict().keys())
    assert keys[0] == "front.stem.conv.weight" and "rnn.gru.weight_hh_l1_reverse" in keys and keys[-1] == "rnn.fc.1.bias"
    assert not any("classifier" in k for k in keys)
    oracle = CRNNOracle(dropout=0.3, seed=4)
    oracle.load_device_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    x, y = make_inputs(5, 12)
    model.train()
    oracle.train()
    xd = x.to(DEV)
    out = model(xd)
    assert out.shape == (12, 2)
    loss = torch.nn.functional.cross_entropy(out, y.to(DEV))
    loss.backward()
    ref = oracle(x, step=0, training=True)
    lo = torch.nn.functional.cross_entropy(ref, y)
    lo.backward()
    tol = 2e-4 if act == "fp32" else 3e-2
    assert (out.detach().cpu().double() - ref.detach()).abs().max().item() <= tol
    assert abs(loss.item() - lo.item()) <= tol
    gd = torch.cat([p.grad.flatten().cpu().double() for n, p in model.named_parameters() if n.startswith("rnn.")])
    go = torch.cat([p.grad.flatten() for p in oracle.rnn.parameters()])
    assert len(gd) == len(go)
    # whole-vector bounds: at B=12 a single fp32 ReLU decision within round-off of zero moves individual conv gradients
    assert ((gd - go).norm() / go.norm()).item() <= (2e-3 if act == "fp32" else 8e-2)
    fd = torch.cat([p.grad.flatten().cpu().double() for n, p in model.named_parameters() if n.startswith("front.")])
    fo = torch.cat([p.grad.flatten() for n, p in oracle.front.named_parameters() if not n.startswith("classifier")])
    if act == "fp32":
        assert ((fd - fo).norm() / fo.norm()).item() <= 2e-2
    else:      # bf16 storage of 9 activation / 9 gradient tensors at B=12: direction of the conv-stack gradient (cf. test_bf16_mode.py)
        assert (fd @ fo / (fd.norm() * fo.norm())).item() > 0.97
    model.eval()                      # running statistics were updated by ONE training forward on both sides
    oracle.eval()
    with torch.no_grad():
        ev = model(xd)
        ev_ref = oracle(x, training=False)
    assert (ev.cpu().double() - ev_ref).abs().max().item() <= (5e-4 if act == "fp32" else 5e-2)


@pytest.mark.parametrize("arch", ["crnn", "gru"])
def test_trainer_drives_recurrent_models(tmp_path, arch):
    """Trainer.train_epoch / validate_epoch on waveform batches with the recurrent models (generic autograd path: native
    front end -> model -> native loss -> torch AdamW); first-step loss == the oracle pipeline's."""
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from oracle.train_step import frontend
    from oracle.crnn import CRNNOracle
    from oracle.gru import GRUWakewordOracle
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 1, 0, 8
    cfg.loss.label_smoothing = 0.0
    torch.manual_seed(9)
    model = create_model(arch, dropout=0.0)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    wave, y = make_synthetic_batch(24, 24000, seed=5)
    y[::3] = 1
    batches = [(wave[i:i + 8], y[i:i + 8], [{"path": "s"}] * 8) for i in range(0, 24, 8)]
    t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path, device=DEV)
    losses = []

    class Rec:
        def on_batch_end(self, batch_idx, loss, acc):
            losses.append(loss)
    t.add_callback(Rec())
    t.train_epoch(0)
    assert len(losses) == 3 and all(np.isfinite(losses))
    a = cfg.augmentation
    spec = dict(freq_mask_param=a.freq_mask_param, time_mask_param=a.time_mask_param, n_freq_masks=a.n_freq_masks,
                n_time_masks=a.n_time_masks, freq_mask_prob=a.freq_mask_prob, time_mask_prob=a.time_mask_prob)
    x0, _ = frontend(batches[0][0].numpy(), spec, seed=a.seed, step=0)
    if arch == "crnn":
        oracle = CRNNOracle(dropout=0.0)
        oracle.load_device_state_dict(sd)
    else:
        oracle = GRUWakewordOracle(40, dropout=0.0)
        oracle.load_reference_state_dict(sd)
    oracle.train()
    ref = torch.nn.functional.cross_entropy(oracle(torch.as_tensor(x0), training=True), batches[0][1]).item()
    assert abs(losses[0] - ref) < 1e-3, (losses[0], ref)
    loss, m = t.validate_epoch(0)
    assert m.total_samples == 8 and np.isfinite(loss)


def test_gruwakeword_bf16_matrix_mode():
    """mode='bf16': the projection / weight-gradient GEMMs take bf16 operands (fp32 accumulation), the recurrence stays fp32.
    Against the float64 oracle: logits within 2e-2, gradient direction cos > 0.999."""
    from wakeword_trainer_home_amd.models import create_model
    from oracle.gru import GRUWakewordOracle
    torch.manual_seed(1)
    model = create_model("gru", input_size=40, dropout=0.0, mode="bf16").to(DEV)
    oracle = GRUWakewordOracle(40, dropout=0.0)
    oracle.load_reference_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    x = torch.randn(33, 50, 40)
    y = torch.randint(0, 2, (33,))
    model.train()
    out = model(x.to(DEV))
    torch.nn.functional.cross_entropy(out, y.to(DEV)).backward()
    ref = oracle(x, training=True)
    torch.nn.functional.cross_entropy(ref, y).backward()
    assert (out.detach().cpu().double() - ref.detach()).abs().max().item() <= 2e-2
    gd = torch.cat([p.grad.flatten().cpu().double() for p in model.parameters()])
    go = torch.cat([p.grad.flatten() for p in oracle.parameters()])
    assert (gd @ go / (gd.norm() * go.norm())).item() > 0.999


@pytest.mark.parametrize("reverse", [False, True])
def test_gru_direction_bf16_mode(reverse, gru_rows):
    """mode=bf16: h and W_hh enter the per-step MFMA as bf16 (fp32 accumulation, fp32 state): outputs within 2e-2 of the
    float64 nn.GRU over 76 steps, weight-gradient direction cos > 0.999."""
    from wakeword_trainer_home_amd import _native as nat
    B, T, I, H = 40, 76, 64, 128
    torch.manual_seed(5)
    ref = torch.nn.GRU(I, H, num_layers=1, batch_first=True, bidirectional=True).double()
    sfx = "_reverse" if reverse else ""
    P = [getattr(ref, n + "_l0" + sfx) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    x = torch.randn(B, T, I, dtype=torch.float64)
    out, hn = ref(x)
    sl = slice(H, 2 * H) if reverse else slice(0, H)
    dy = torch.randn(B, T, H, dtype=torch.float64)
    (out[:, :, sl] * dy).sum().backward()
    f = lambda t: t.detach().float().to(DEV)
    y = torch.empty(B, T, H, device=DEV)
    ws = nat.gru_workspace(B, T, I, H, DEV)
    nat.gru_fwd(f(x), *[f(p) for p in P], y, ws, reverse=reverse, mode=torch.bfloat16)
    assert (y.cpu().double() - out[:, :, sl].detach()).abs().max().item() <= 2e-2
    dw_ih, dw_hh, db_ih, db_hh, _ = nat.gru_bwd(f(x), f(P[0]), f(P[1]), f(dy), None, ws, reverse=reverse, mode=torch.bfloat16)
    for got, p in ((dw_ih, P[0]), (dw_hh, P[1]), (db_ih, P[2]), (db_hh, P[3])):
        a, b = got.cpu().double().flatten(), p.grad.flatten()
        assert (a @ b / (a.norm() * b.norm())).item() > 0.999


def test_async_autograd_step_skips_nonfinite_batch_on_device(tmp_path):
    """The sync-free step of a HIP-backed autograd model: a batch with a non-finite loss changes no parameter (the fused
    optimizer gets the flag on the device), is not reported to callbacks and still counts in the epoch average's
    denominator (reference quirk Q5, trainer.py:177-179,228)."""
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 1, 0, 8
    torch.manual_seed(2)
    model = create_model("gru", dropout=0.0)
    wave, y = make_synthetic_batch(24, 24000, seed=6)
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
    avg, _ = t.train_epoch(0)
    after = {k: v.clone() for k, v in model.state_dict().items()}
    assert [i for i, _ in seen] == [0, 2] and all(np.isfinite(l) for _, l in seen)
    changed01 = any(not torch.equal(snaps[0][k], snaps[1][k]) for k in snaps[0])
    same12 = all(torch.equal(snaps[1][k], snaps[2][k]) for k in snaps[1])          # the NaN batch left everything untouched
    changed2 = any(not torch.equal(snaps[2][k], after[k]) for k in after)
    assert changed01 and same12 and changed2
    assert abs(avg - (seen[0][1] + seen[1][1]) / 3) < 1e-6


# ------------------------------------------------------------------------------------------ layers against the restated reference
# oracle/gru.py:gru_restated rounds exactly what the device rounds to the matrix type (x, W_ih, each step's h_{t-1} and W_hh,
# dGi / dGh, the operands of the dW and dX products) and nothing else, so only fp32 accumulation order, the fast gate functions of
# the 16-bit modes (gate_sigmoid<true>, ~2e-7) and the rare 16-bit rounding that flips because the device's fp32 operand differs
# from the float64 one in its last bits stay between the two.  Error measures: y, h_n and dh0 absolute (all O(1)); dx and the four
# parameter gradients relative to each tensor's largest entry.  In the 16-bit modes a flip does not stay alone: it moves the next
# step's operands by ~1e-5, which flips more of them, so the errors settle at the level where the reference itself moves when its
# inputs are perturbed by 2e-7 (measured on the CPU: up to 2.4e-3 for bf16 gradients at B=7, T=13).  The forward stays well
# inside the mode's own error (restated vs exact GRU: bf16 3e-3..5e-3, fp16 3e-4..6e-4 on y).  Measured on the MI355X, largest
# over both workgroup shapes and every case of a mode (y|h_n, dh0, gradients): fp32 7.6e-7, 7.3e-7, 1.1e-6; bf16 2.7e-4,
# 7.8e-4, 2.4e-3; fp16 3.9e-5, 1.1e-4, 1.9e-4.  Bounds: 2-3x those in bf16 and fp16, 7-9x in fp32 (the device sums in a fixed
# order: the results repeat).
_MT = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}
_GRU_BOUND = {"fp32": (5e-6, 5e-6, 1e-5), "bf16": (8e-4, 2e-3, 5e-3), "fp16": (1e-4, 3e-4, 5e-4)}     # (y|h_n, dh0, gradients)
_REF_CACHE = {}

# Single-direction cases (ww_gru_fwd / ww_gru_bwd), with the host branch each one reaches:
#   t1_b1       B = 1, T = 1, I = 9: one step, one batch row, the k_gemm projection (I % 64 != 0)
#   b7_i64      B = 7 (< 8 rows), I = 64, B*T = 91 >= 35: the ww_gemm16_nt_bias projection (16-bit modes)
#   b9_i64_kg   B = 9 (> 8 rows), I = 64, B*T = 27 < 35: the 16-bit copies do not fit the dGh region -> k_gemm
#   b17_i256    B = 17 (> 16 rows), I = 256, B*T = 204 >= 192: ww_gemm16_nt_bias
#   b19_i256_kg I = 256, B*T = 190 < 192: k_gemm
#   x_ld67      x a column view with row stride 67 (ldx % 4 != 0): k_gemm although B*T = 54 would fit gemm16; vecA/vecB = 0 in dW_ih
#   y_off1      y / dy column views at a 4-byte offset of rows of 132 floats: y_vec = dy_vec = 0 from the pointer alone
#   dy_none     no dy, only dh_n
#   split       B = 64, T = 80: B*T = 5120 >= 4096 -> the dW_hh / dW_ih products split K 64 ways (k_splitk_sum)
# every case has an h0 and asks for dh0.
_DIR_CASES = {
    "t1_b1": dict(B=1, T=1, I=9, reverse=False),
    "b7_i64": dict(B=7, T=13, I=64, reverse=True),
    "b9_i64_kg": dict(B=9, T=3, I=64, reverse=False),
    "b17_i256": dict(B=17, T=12, I=256, reverse=False),
    "b19_i256_kg": dict(B=19, T=10, I=256, reverse=True),
    "x_ld67": dict(B=9, T=6, I=64, reverse=True, ldx=67),
    "y_off1": dict(B=17, T=5, I=64, reverse=False, yoff=1),
    "dy_none": dict(B=8, T=7, I=40, reverse=True, no_dy=True),
    "split": dict(B=64, T=80, I=64, reverse=False),
}


def _gru_inputs(B, T, I, seed, nd):
    """fp32-representable float64 inputs: nn.GRU's initialisation, x ~ N(0,1), h0 ~ 0.3 N(0,1), dy / dh_n ~ N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    H, k = 128, 128 ** -0.5
    q = lambda t: t.float().double()
    P = [[q((torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k) for s in ((3 * H, I), (3 * H, H), (3 * H,), (3 * H,))]
         for _ in range(nd)]
    x = q(torch.randn(B, T, I, generator=g, dtype=torch.float64))
    h0 = [q(0.3 * torch.randn(B, H, generator=g, dtype=torch.float64)) for _ in range(nd)]
    dy = q(torch.randn(B, T, nd * H, generator=g, dtype=torch.float64))
    dhn = [q(torch.randn(B, H, generator=g, dtype=torch.float64)) for _ in range(nd)]
    return P, x, h0, dy, dhn


def _check_restated(tag, mode, got, ref):
    """got / ref: dicts of the same keys.  Prints the measured errors (-s) and checks them against the mode's bounds."""
    b_fwd, b_dh0, b_rel = _GRU_BOUND[mode]
    errs = {}
    for k, r in ref.items():
        a = got[k].detach().cpu().double()
        errs[k] = (a - r).abs().max().item() if k.startswith(("y", "h_n", "dh0")) else _rel(a, r)
    print(f"restated-gru {tag} {mode}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, e in errs.items():
        assert e <= (b_fwd if k.startswith(("y", "h_n")) else b_dh0 if k.startswith("dh0") else b_rel), (tag, mode, k, e)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", list(_DIR_CASES))
def test_gru_direction_matches_restated_reference(case, mode, gru_rows):
    """ww_gru_fwd / ww_gru_bwd in each matrix mode against oracle/gru.py:gru_restated (bounds and the branch each case
    reaches: see _GRU_BOUND / _DIR_CASES above): y, h_n, dx, dW_ih, dW_hh, db_ih, db_hh and dh0; nothing written outside y."""
    from wakeword_trainer_home_amd import _native as nat
    from oracle.gru import gru_restated
    c = _DIR_CASES[case]
    B, T, I, rev, H = c["B"], c["T"], c["I"], c["reverse"], 128
    P, x, h0, dy, dhn = _gru_inputs(B, T, I, 1 + list(_DIR_CASES).index(case), 1)
    P, h0, dhn, dy = P[0], h0[0], dhn[0], (None if c.get("no_dy") else dy)
    key = ("dir", case, mode)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = gru_restated(x, *P, h0=h0, dy=dy, dh_n=dhn, mtype=_MT[mode], reverse=rev)
    ref = _REF_CACHE[key]
    f = lambda t: t.float().to(DEV)
    if c.get("ldx"):
        xd = torch.zeros(B, T, c["ldx"], device=DEV)[:, :, :I]
        xd.copy_(f(x))
    else:
        xd = f(x)
    off = c.get("yoff", 0)
    ld = H + 4 if off else H
    ybuf = torch.full((B, T, ld), 7.0, device=DEV)
    y = ybuf[:, :, off:off + H]
    assert (y.data_ptr() % 16 != 0) == bool(off)
    md = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[mode]
    ws = nat.gru_workspace(B, T, I, H, DEV)
    Pd = [f(p) for p in P]
    h_n = nat.gru_fwd(xd, *Pd, y, ws, h0=f(h0), reverse=rev, mode=md)
    if off:
        assert torch.equal(ybuf[:, :, :off], torch.full_like(ybuf[:, :, :off], 7.0))
        assert torch.equal(ybuf[:, :, off + H:], torch.full_like(ybuf[:, :, off + H:], 7.0))
    dyd = None
    if dy is not None:
        dybuf = torch.full((B, T, ld), float("nan"), device=DEV)       # columns outside the view must never be read
        dyd = dybuf[:, :, off:off + H]
        dyd.copy_(f(dy))
    dx = torch.zeros(B, T, I, device=DEV)
    dw_ih, dw_hh, db_ih, db_hh, dh0 = nat.gru_bwd(xd, Pd[0], Pd[1], dyd, f(dhn), ws, reverse=rev, dx=dx, want_dh0=True, mode=md)
    got = dict(y=y, h_n=h_n, dh0=dh0, dx=dx, dw_ih=dw_ih, dw_hh=dw_hh, db_ih=db_ih, db_hh=db_hh)
    _check_restated(f"{case}/rows{gru_rows}", mode, got, {k: ref[k] for k in got})


# Bidirectional cases (ww_gru_bidir_fwd / _bwd, both directions in one recurrent launch, dX as one ww_gemm_seg2 product):
#   t1_b1     B = 1, T = 1, I = 9: k_gemm projections
#   b9_i64    B = 9, B*T = 54: ww_gemm16_nt_bias, the second direction reusing the first one's 16-bit x (xh_shared)
#   b7_i256   B = 7, B*T = 35 < 192: k_gemm
#   y_off1    y / dy column views at a 4-byte offset (rows of 260 floats): y_vec = dy_vec = 0
#   dy_none   no dy, only dh_n of both directions
#   split     B = 64, T = 80: split-K dW products of both directions
_BIDIR_CASES = {
    "t1_b1": dict(B=1, T=1, I=9),
    "b9_i64": dict(B=9, T=6, I=64),
    "b7_i256": dict(B=7, T=5, I=256),
    "y_off1": dict(B=17, T=4, I=40, yoff=1),
    "dy_none": dict(B=16, T=5, I=64, no_dy=True),
    "split": dict(B=64, T=80, I=64),
}


def _bidir_ref(case, mode):
    from oracle.gru import gru_restated
    c = _BIDIR_CASES[case]
    B, T, I, H = c["B"], c["T"], c["I"], 128
    P, x, h0, dy, dhn = _gru_inputs(B, T, I, 101 + list(_BIDIR_CASES).index(case), 2)
    dy = None if c.get("no_dy") else dy
    key = ("bidir", case, mode)
    if key not in _REF_CACHE:
        o = [gru_restated(x, *P[d], h0=h0[d], dy=None if dy is None else dy[:, :, d * H:(d + 1) * H], dh_n=dhn[d],
                          mtype=_MT[mode], reverse=(d == 1)) for d in range(2)]
        ref = {"y": torch.cat([o[0]["y"], o[1]["y"]], 2), "dx": o[0]["dx"] + o[1]["dx"]}
        for d in range(2):
            for k in ("h_n", "dh0", "dw_ih", "dw_hh", "db_ih", "db_hh"):
                ref[f"{k}{d}"] = o[d][k]
        _REF_CACHE[key] = ref
    return c, (P, x, h0, dy, dhn), _REF_CACHE[key]


def _bidir_run(c, inputs, mode, outs=None, defer=False):
    from wakeword_trainer_home_amd import _native as nat
    P, x, h0, dy, dhn = inputs
    B, T, I, H = c["B"], c["T"], c["I"], 128
    f = lambda t: t.float().to(DEV)
    md = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[mode]
    off = c.get("yoff", 0)
    ld = 2 * H + 4 if off else 2 * H
    ybuf = torch.full((B, T, ld), 7.0, device=DEV)
    y = ybuf[:, :, off:off + 2 * H]
    params = [[f(p) for p in P[d]] for d in range(2)]
    ws = [nat.gru_workspace(B, T, I, H, DEV) for _ in range(2)]
    xd = f(x)
    h_n = nat.gru_bidir_fwd(xd, params, y, ws, mode=md, h0=[f(h0[0]), f(h0[1])])
    if off:
        assert torch.equal(ybuf[:, :, :off], torch.full_like(ybuf[:, :, :off], 7.0))
        assert torch.equal(ybuf[:, :, off + 2 * H:], torch.full_like(ybuf[:, :, off + 2 * H:], 7.0))
    dyd = None
    if dy is not None:
        dybuf = torch.full((B, T, ld), float("nan"), device=DEV)
        dyd = dybuf[:, :, off:off + 2 * H]
        dyd.copy_(f(dy))
    dx = torch.zeros(B, T, I, device=DEV)
    dh0 = [torch.empty(B, H, device=DEV) for _ in range(2)]
    grads = nat.gru_bidir_bwd(xd, params, dyd, [f(dhn[0]), f(dhn[1])], ws, dx=dx, mode=md, outs=outs, defer=defer, dh0=dh0)
    got = {"y": y, "dx": dx}
    for d in range(2):
        got[f"h_n{d}"], got[f"dh0{d}"] = h_n[d], dh0[d]
        for k, g in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), grads[d]):
            got[f"{k}{d}"] = g
    return got


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", list(_BIDIR_CASES))
def test_gru_bidirectional_matches_restated_reference(case, mode, gru_rows):
    """ww_gru_bidir_fwd / _bwd in each matrix mode against two restated directions (bounds and the branch each case reaches:
    see _GRU_BOUND / _BIDIR_CASES above): y (both halves), both h_n and dh0, the summed dx, all eight parameter gradients."""
    c, inputs, ref = _bidir_ref(case, mode)
    got = _bidir_run(c, inputs, mode)
    _check_restated(f"bidir-{case}/rows{gru_rows}", mode, got, ref)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_gru_split_dw_deferred_equals_immediate(mode):
    """B*T = 5120: the split-K weight-gradient products under ww_ctx_set_deferred_reduce keep dW_hh and dW_ih partials in the
    two halves of the partial region and queue one 768-column bias item per direction (db_ih | db_hh adjacent in a flat
    bucket, nn.GRU's parameter order): 6 queued items, one flush.  Deferred == immediate to round-off (the flush sums in
    double, the immediate kernels in float: measured 2.9e-7 rel, bound 2e-6 as for the linear layers), and the deferred
    gradients also meet the restated reference."""
    from wakeword_trainer_home_amd import _native as nat
    c, inputs, ref = _bidir_ref("split", mode)
    now = _bidir_run(c, inputs, mode)
    I, H = c["I"], 128
    sizes = [3 * H * I, 3 * H * H, 3 * H, 3 * H]
    bucket = torch.full((2 * sum(sizes),), float("nan"), device=DEV)
    outs, o = [], 0
    for d in range(2):
        slots = []
        for s, shape in zip(sizes, ((3 * H, I), (3 * H, H), (3 * H,), (3 * H,))):
            slots.append(bucket[o:o + s].view(shape))
            o += s
        outs.append(tuple(slots))
    lib, cx = nat.load(), nat.ctx(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    later = _bidir_run(c, inputs, mode, outs=outs, defer=True)
    assert lib.ww_deferred_reduce_pending(cx) == 6
    nat.deferred_flush(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(bucket).any()
    worst = 0.0
    for d in range(2):
        for k in ("dw_ih", "dw_hh", "db_ih", "db_hh"):
            e = _rel(later[f"{k}{d}"].double(), now[f"{k}{d}"].double())
            worst = max(worst, e)
            assert e <= 2e-6, (k, d, e)
    print(f"restated-gru deferred-vs-immediate {mode}: {worst:.2e}")
    _check_restated("bidir-split-deferred", mode, {k: v for k, v in later.items() if k.startswith(("dw", "db"))},
                    {k: v for k, v in ref.items() if k.startswith(("dw", "db"))})
