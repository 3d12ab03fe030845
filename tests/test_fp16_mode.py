"""GPU: fp16 activation-storage mode (WW_ACT_F16; BASELINE config 5 names fp16) -- the reference's own reduced precision is
fp16 autocast + ``GradScaler`` (src/training/trainer.py:172,182-193; src/training/optimizer_factory.py:403-420).  Here the
16-bit type is the STORAGE / matrix-operand type of the HIP kernels (arithmetic, statistics, parameters stay fp32) and the
scaler lives on the device: the loss kernel multiplies dL/dlogits by the scale, the fused optimizer divides it out, skips
on overflow and applies GradScaler's growth / backoff rule.  Tolerances are fp16-sized (11-bit mantissa) and stated."""
import numpy as np
import pytest
import torch

from tests.golden_util import load_trace, make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cos(a, b):
    return (a @ b / (a.norm() * b.norm())).item()


@pytest.mark.parametrize("B,Fd,T,p", [(4, 40, 151, 0.3), (6, 13, 50, 0.0), (5, 8, 12, 0.0)])
def test_cnn_small_fp16_close_to_oracle(B, Fd, T, p):
    """Whole model, fp16 storage vs the float64 oracle: logits within 4e-3 of their scale, gradient direction cos > 0.9995
    (bf16 storage holds 3e-2 / 0.995: three more mantissa bits).  The upstream gradient is multiplied by 1024 on the way in
    and divided out of the results -- what the loss scale does in training -- so the stored gradients sit in fp16's range."""
    from oracle.cnn_small import CNNSmallOracle
    from wakeword_trainer_home_amd.models import create_model
    torch.manual_seed(5)
    oracle = CNNSmallOracle(dropout=p, dropout_seed=3).double()
    model = create_model("cnn_small", dropout=p, dropout_seed=3, act_dtype="fp16")
    model.load_state_dict({k: v.float() for k, v in oracle.state_dict().items()})
    model.to(DEV).train()
    oracle.train()
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(B, 1, Fd, T, generator=gen, dtype=torch.float64) * 2 - 4
    dlog = torch.randn(B, 2, generator=gen, dtype=torch.float64) / B
    out = model(x.float().to(DEV))
    out.backward((dlog * 1024.0).float().to(DEV))
    ref = oracle(x)
    ref.backward(dlog)
    assert (out.detach().cpu().double() - ref.detach()).abs().max() < 4e-3 * max(ref.abs().max().item(), 1.0)
    gn = torch.cat([q.grad.flatten().cpu().double() for q in model.parameters()]) / 1024.0
    go = torch.cat([q.grad.flatten() for q in oracle.parameters()])
    assert torch.isfinite(gn).all()
    assert _cos(gn, go) > (0.9995 if Fd * T > 1000 else 0.998), _cos(gn, go)      # (13 x 50 maps: 0.99949-0.99952 measured)
    assert abs(gn.norm().item() / go.norm().item() - 1.0) < 1e-2


def _trainer(tmp_path, golden_dir, amp, init_scale=None):
    from wakeword_trainer_home_amd.config import WakewordConfig
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    meta, tr = load_trace(golden_dir, "default_b128")
    cfg = WakewordConfig()
    for sec in ("loss", "optimizer", "training"):
        for k, v in meta["cfg"][sec].items():
            if hasattr(getattr(cfg, sec), k):
                setattr(getattr(cfg, sec), k, v)
    cfg.model.architecture, cfg.optimizer.mixed_precision, cfg.optimizer.amp_dtype = "cnn_small", True, amp
    model = create_model("cnn_small", dropout=0.0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in tr["init"].items()})
    xtr, ytr = make_inputs(meta["train_seed"], meta["n_train"])
    xva, yva = make_inputs(meta["val_seed"], meta["n_val"])
    DL, TD = torch.utils.data.DataLoader, torch.utils.data.TensorDataset
    t = Trainer(model, DL(TD(xtr, ytr), batch_size=128), DL(TD(xva, yva), batch_size=128), cfg, checkpoint_dir=tmp_path, device=DEV)
    if init_scale is not None:
        from wakeword_trainer_home_amd import _native as nat
        t.scaler.state.copy_(nat.loss_scale_new("cpu", init_scale))
    return t, meta, tr


def test_trainer_fp16_tracks_reference_trace(golden_dir, tmp_path):
    """mixed_precision=True + amp_dtype='fp16' through the Trainer on the reference's B=128 trace (captured from the real
    reference Trainer in fp32): per-step loss within 2.5e-4 (10x the 2.2e-5 measured on MI355X); the scaler is the device one, its scale stayed at GradScaler's
    initial 65536 and its growth tracker counted every applied step; the checkpoint's scaler_state_dict has GradScaler's keys."""
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.training.optimizer_factory import DeviceGradScaler
    t, meta, tr = _trainer(tmp_path, golden_dir, "fp16")
    assert t.model.act == nat.ACT_F16 and isinstance(t.scaler, DeviceGradScaler)
    losses = []
    t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: losses.append(l)})())
    t.train()
    d = np.abs(np.array(losses) - tr["step_loss"])
    assert len(losses) == len(tr["step_loss"]) and d.max() < 2.5e-4, d
    sd = t.scaler.state_dict()
    assert set(sd) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    assert sd["scale"] == 65536.0 and sd["_growth_tracker"] == len(losses) == t.optimizer.step_count()
    ck = torch.load(tmp_path / "best_model.pt", map_location="cpu", weights_only=False)
    assert ck["scaler_state_dict"]["scale"] == 65536.0
    print(f"fp16 storage: max |loss - ref| = {d.max():.2e}")


def test_overflowing_scale_backs_off_and_skips_like_gradscaler(golden_dir, tmp_path):
    """Start from a loss scale far too large (2^40): the scaled gradients overflow fp16 -> the step is skipped on the device
    (parameters bit-unchanged, optimizer step count unchanged) and the scale halves, again and again, until a step fits --
    GradScaler.update()'s backoff.  Then training proceeds; growth_interval applied steps later the scale doubles."""
    from wakeword_trainer_home_amd import _native as nat
    t, meta, tr = _trainer(tmp_path, golden_dir, "fp16", init_scale=2.0 ** 40)
    t.scaler.state.copy_(nat.loss_scale_new("cpu", 2.0 ** 40, growth_interval=3))
    x, y = make_inputs(meta["train_seed"], 128)
    t.model.train()
    before = t.model.flat_param.clone()
    scales, applied = [], []
    for i in range(40):
        t._step_native(x, y, i)
        t._flush_pending()
        scales.append(t.scaler.get_scale())
        applied.append(t.optimizer.step_count())
        if applied[-1] == 0:
            assert torch.equal(t.model.flat_param, before)        # skipped steps leave the parameters alone
    first = next(i for i, a in enumerate(applied) if a > 0)
    assert first >= 5                                             # 2^40 has to come down a long way (9 halvings measured)
    assert all(scales[i] == 2.0 ** (39 - i) for i in range(first))            # halved once per skipped step
    assert torch.isfinite(t.model.flat_param).all() and not torch.equal(t.model.flat_param, before)
    # growth: every 3 consecutive applied steps double the scale (an overflow in between resets the count and halves it)
    assert any(b > a for a, b in zip(scales[first:], scales[first + 1:])), scales
    assert applied[-1] >= 20


def test_fp16_graph_replay_is_bit_exact(tmp_path):
    """The loss scale and its slot are device state too: a replayed fp16 step equals the eager one bit for bit, scaler included."""
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    x, y = make_inputs(4, 16 * 6)
    batches = [(x[16 * i:16 * i + 16], y[16 * i:16 * i + 16]) for i in range(6)]
    out = []
    for graph in (False, True):
        cfg = get_preset("cnn_small_logmel40")
        cfg.training.epochs, cfg.training.batch_size, cfg.optimizer.warmup_epochs = 2, 16, 0
        cfg.optimizer.mixed_precision, cfg.optimizer.amp_dtype, cfg.training.hip_graph = True, "fp16", graph
        cfg.training.hip_graph_auto = False
        torch.manual_seed(2)
        model = create_model("cnn_small", dropout=0.3, dropout_seed=1)
        t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path / str(graph), device=DEV)
        losses = []
        t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: losses.append(l)})())
        t.train()
        out.append((losses, model.flat_param.clone(), t.scaler.state_dict(), t._graph is not None))
    assert out[1][3] and not out[0][3]
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


# ------------------------------------------------------------------------------------------ single conv layers in fp16 storage
EPS_F16 = 2.0 ** -10          # one RNE rounding is <= 2^-11 relative; 2^-10 leaves room for fp32 order effects (cf. EPS_BF16)


def _rh(t):
    """round a float64/32 tensor to fp16 and back (what the device stores)."""
    return t.float().half().double()


@pytest.mark.parametrize("kind", ["dw", "pw"])
@pytest.mark.parametrize("B,H,W", [(3, 20, 76), (2, 7, 25), (5, 17, 10)])
def test_conv_fwd_layers_fp16(kind, B, H, W):
    """tests/test_bf16_mode.py:test_conv_fwd_layers_bf16 in fp16 storage: one rounding (depthwise) or three (pointwise: the
    stored output and both MFMA operands) of 2^-11, and statistics of exactly the stored tensor.  Measured (of the output's
    scale): depthwise 4.3e-4 against 2^-10 = 9.8e-4, pointwise 5.8e-4 against 2.9e-3."""
    from wakeword_trainer_home_amd import _native as nat
    from tests.test_hip_kernels import cu, nhwc, rel_err, _bn_tensors
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(31)
    y_in = _rh(torch.randn(B, 64, H, W, generator=g, dtype=torch.float64))
    s_in = torch.rand(64, generator=g, dtype=torch.float64) + 0.5
    t_in = torch.randn(64, generator=g, dtype=torch.float64) * 0.5
    a = torch.relu(y_in * s_in[None, :, None, None] + t_in[None, :, None, None])
    if kind == "dw":
        w = torch.randn(64, 1, 3, 3, generator=g, dtype=torch.float64) * 0.3
        ref = F.conv2d(a, w, padding=1, groups=64)
    else:
        w = torch.randn(64, 64, 1, 1, generator=g, dtype=torch.float64) * 0.2
        ref = F.conv2d(a, w)
    gamma, beta, rm, rv = _bn_tensors(2)
    ga, be, rm_g, rv_g = cu(gamma), cu(beta), cu(rm), cu(rv)          # (the BN struct holds raw pointers: keep them alive)
    bn = nat.make_bn(ga, be, rm_g, rv_g)
    fn = nat.dwconv3x3_fwd if kind == "dw" else nat.pwconv1x1_fwd
    y, ss, mr = fn(cu(nhwc(y_in), torch.float16), cu(torch.cat([s_in, t_in])), cu(w), bn, nat.layer_scratch(DEV))
    assert y.dtype == torch.float16
    yd = y.float().cpu().double()
    tol = EPS_F16 * (3 if kind == "pw" else 1)
    print(f"fp16 conv fwd {kind} {B}x{H}x{W}: y={((yd - nhwc(ref)).abs().max() / nhwc(ref).abs().max()).item():.2e}")
    assert (yd - nhwc(ref)).abs().max() <= tol * nhwc(ref).abs().max()
    mean = yd.mean(dim=(0, 1, 2))
    var = yd.var(dim=(0, 1, 2), unbiased=False)
    assert np.abs(mr[:64].cpu().numpy() - mean.numpy()).max() < 1e-5 * (mean.abs().max().item() + 1)
    assert rel_err(mr[64:].cpu(), 1.0 / torch.sqrt(var + 1e-5)) < 2e-5


@pytest.mark.parametrize("scale", [1024.0, 65536.0])
@pytest.mark.parametrize("kind", ["dw", "pw"])
@pytest.mark.parametrize("B,H,W", [(3, 20, 76), (2, 7, 25)])
def test_conv_bwd_layers_fp16(kind, B, H, W, scale):
    """tests/test_bf16_mode.py:test_conv_bwd_layers_bf16 in fp16 storage.  The incoming gradient has a real gradient's size
    (~1/pixels) and is multiplied by the loss scale on the way in, as the device scaler does -- 1024 or GradScaler's 65536 --
    and the results are divided by it: bounds of 2^-11 per rounding as the bf16 file's 2^-8, and the stored gradients finite.
    Measured (both scales alike): g_in depthwise 3.0e-4 against 9.8e-4, pointwise 5.0e-4 against 2.9e-3; dW pointwise 5.6e-4
    against 2 x 2^-10, depthwise (fp32 operands) 2.0e-7 against 2e-6."""
    from wakeword_trainer_home_amd import _native as nat
    from tests.test_hip_kernels import cu, nhwc, rel_err, _coef_from
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(41)
    y_in = _rh(torch.randn(B, 64, H, W, generator=gen, dtype=torch.float64))
    bn_in, bn_out = torch.nn.BatchNorm2d(64).double(), torch.nn.BatchNorm2d(64).double()
    with torch.no_grad():
        for bn in (bn_in, bn_out):
            bn.weight.copy_(torch.rand(64, generator=gen, dtype=torch.float64) + 0.5)
            bn.bias.copy_(torch.randn(64, generator=gen, dtype=torch.float64) * 0.3)
    shape = (64, 1, 3, 3) if kind == "dw" else (64, 64, 1, 1)
    w = (torch.randn(*shape, generator=gen, dtype=torch.float64) * 0.25).requires_grad_(True)
    z_in = bn_in(y_in)
    z_in.retain_grad()
    a = torch.relu(z_in)
    y_raw = F.conv2d(a, w, padding=1, groups=64) if kind == "dw" else F.conv2d(a, w)
    y = y_raw + (_rh(y_raw.detach()) - y_raw.detach())
    z = bn_out(y)
    g0 = torch.randn(B, 64, H, W, generator=gen, dtype=torch.float64) * (torch.rand(B, 64, H, W, generator=gen) > 0.4) / (B * H * W)
    g = _rh(g0 * scale)                                   # the scaled gradient as the device stores it
    (z * g).sum().backward()
    coef, _, _ = _coef_from(g, y.detach(), bn_out.weight.detach())
    mean_in = y_in.mean(dim=(0, 2, 3))
    rstd_in = 1.0 / torch.sqrt(y_in.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    scale_in = bn_in.weight.detach() * rstd_in
    ss_in = torch.cat([scale_in, bn_in.bias.detach() - mean_in * scale_in])
    F16 = torch.float16
    args = dict(y_out=cu(nhwc(y.detach()), F16), coef=cu(coef), y_in=cu(nhwc(y_in), F16), ss_in=cu(ss_in),
                mr_in=cu(torch.cat([mean_in, rstd_in])), gamma_in=cu(bn_in.weight.detach()), w=cu(w.detach()),
                scratch=nat.layer_scratch(DEV))
    if kind == "dw":
        g_in, dw, coef_in, dgamma, dbeta = nat.dwconv3x3_bwd(cu(nhwc(g), F16), **args)
    else:
        g_in, dw, coef_in, dgamma, dbeta = nat.pwconv1x1_bwd(cu(nhwc(g), F16), None, ss_out=None, **args)
    assert g_in.dtype == F16 and torch.isfinite(g_in).all()
    gi = g_in.float().cpu().double() / scale
    ref_gi = nhwc(z_in.grad) / scale
    tol = EPS_F16 * (3 if kind == "pw" else 1)
    print(f"fp16 conv bwd {kind} {B}x{H}x{W} x{scale:g}: g_in={((gi - ref_gi).abs().max() / ref_gi.abs().max()).item():.2e} "
          f"dw={rel_err(dw.cpu().reshape(-1) / scale, w.grad.reshape(-1) / scale):.2e}")
    assert (gi - ref_gi).abs().max() <= tol * ref_gi.abs().max()
    # pointwise: dy and relu(bn(y_in)) rounded to fp16 for the MFMA, two roundings (measured 5.6e-4); depthwise: fp32 operands
    assert rel_err(dw.cpu().reshape(-1) / scale, w.grad.reshape(-1) / scale) < (2 * EPS_F16 if kind == "pw" else 2e-6)
    yhat_in = (nhwc(y_in) - mean_in) * rstd_in
    assert rel_err(dbeta.cpu() / scale, gi.sum(dim=(0, 1, 2))) < 1e-4
    assert rel_err(dgamma.cpu() / scale, (gi * yhat_in).sum(dim=(0, 1, 2))) < 1e-4


@pytest.mark.parametrize("kind", ["dw", "pw"])
def test_conv_fwd_fp16_rounding_edges(kind):
    """The fp16 storage of the conv layers (Act<ww_f16>::round2 / st2 in the depthwise kernel, st4 in the pointwise one, both
    through pack2) at the edges of its contract: RNE, subnormals kept, overflow to inf -- never 65504 or NaN.  BN-apply is the
    identity (scale 1, shift 0) and the filter is diagonal (pointwise) or its centre tap only (depthwise), so y[p][c] =
    a_p w_c: a product of two fp16 values, exact in fp32.  The stored fp16 must equal torch's ``fp32_result.to(float16)`` bit
    for bit (signed zeros included) over all 64 x 64 products, among them ties (3 x 683 = 2049 -> 2048, 7 x 293 = 2051 ->
    2052), subnormal results and ties (1.5 x 2^-24 -> 2^-23, 0.5 x 2^-24 -> 0), 152 x 431 = 65512 -> 65504 and
    1365 x 48 = 65520, 255 x 257 -> inf."""
    from wakeword_trainer_home_amd import _native as nat
    from tests.test_hip_kernels import cu, _bn_tensors
    q = 2.0 ** -24
    g = torch.Generator().manual_seed(3)
    a_vals = [3.0, 7.0, 152.0, 1365.0, 255.0, 2.0 ** -14, q, 3 * q, 1.0, 2.0 ** -10, 65504.0, 0.5, 1.5, 2.0 ** -7]
    w_vals = [683.0, 293.0, 431.0, 48.0, 257.0, 2.0 ** -5, 0.5, -0.5, 1.0, -1.0, 2.0, 2.0 ** -12, -683.0, 1.0 + 2.0 ** -10,
              0.75, 65504.0, -2.0 ** -12]
    a = torch.tensor(a_vals + (torch.rand(64 - len(a_vals), generator=g) * 8).half().tolist(), dtype=torch.float64)
    w = torch.tensor(w_vals + (torch.randn(64 - len(w_vals), generator=g) * 300).half().tolist(), dtype=torch.float64)
    y_in = a.reshape(1, 8, 8, 1).expand(1, 8, 8, 64).contiguous()                 # NHWC: pixel p holds a_p in every channel
    ss_in = torch.cat([torch.ones(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)])
    if kind == "dw":
        wt = torch.zeros(64, 1, 3, 3, dtype=torch.float64)
        wt[:, 0, 1, 1] = w
    else:
        wt = torch.diag(w).reshape(64, 64, 1, 1)
    exact = a[:, None] * w[None, :]                                               # (pixel, channel)
    assert torch.equal(exact.float().double(), exact) and torch.equal(a.half().double(), a) and torch.equal(w.half().double(), w)
    want = exact.float().half()
    gamma, beta, rm, rv = _bn_tensors(2)
    ga, be, rm_g, rv_g = cu(gamma), cu(beta), cu(rm), cu(rv)          # (the BN struct holds raw pointers: keep them alive)
    bn = nat.make_bn(ga, be, rm_g, rv_g)
    fn = nat.dwconv3x3_fwd if kind == "dw" else nat.pwconv1x1_fwd
    y, _, _ = fn(cu(y_in, torch.float16), cu(ss_in), cu(wt), bn, nat.layer_scratch(DEV))
    got = y.cpu().reshape(64, 64)
    bad = got.view(torch.int16) != want.view(torch.int16)
    assert not bad.any(), [(exact[i, j].item(), got[i, j].item(), want[i, j].item()) for i, j in bad.nonzero()[:8].tolist()]
    A, W = {v: i for i, v in enumerate(a_vals)}, {v: i for i, v in enumerate(w_vals)}
    assert got[A[3.0], W[683.0]].item() == 2048.0 and got[A[7.0], W[293.0]].item() == 2052.0
    assert got[A[3 * q], W[0.5]].item() == 2 * q and got[A[q], W[0.5]].item() == 0.0 and got[A[2.0 ** -14], W[2.0 ** -5]].item() == 2.0 ** -19
    assert got[A[152.0], W[431.0]].item() == 65504.0 and got[A[1365.0], W[48.0]].item() == float("inf")
    assert got[A[255.0], W[257.0]].item() == float("inf") and got[A[65504.0], W[-683.0]].item() == float("-inf")
    assert not torch.isnan(got).any()


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("B,Fd,T", [(4, 40, 151), (6, 13, 50), (5, 8, 12)])
def test_cnn_small_fp16_per_tensor_matches_restatement(B, Fd, T, p):
    """tests/test_bf16_mode.py:test_cnn_small_bf16_per_tensor_matches_restatement in fp16 storage, at GradScaler's 65536 loss
    scale."""
    from wakeword_trainer_home_amd import _native as nat
    from tests.test_cnn_front import check_cnn_small
    check_cnn_small(nat, "fp16", B, Fd, T, p, seed=B + Fd)
