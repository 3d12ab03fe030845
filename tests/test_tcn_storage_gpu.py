"""16-bit activation storage of the causal Conv1d path (ww_tconv1d_st_fwd / _bwd, ww_dropout_bt_st, ww_add_relu_st_fwd,
ww_seq_round_st) and TCNWakeword(storage=...) on the MI355X.

Reference: the float64 restatement of tests/tcn_storage_cases.py, which rounds exactly where the device stores a tensor (pinned on the
CPU to TCNRestated, and through it to the reference's own class, by test_tcn_storage_host.py).  Three kinds of bound:
  * integer data: the device returns the restatement's bits (every fp32 sum is exact, test_tcn_storage_host.py);
  * one op on N(0,1) data, against the restated op seeded with the device's own stored inputs: |got - unrounded ref| <= A +
    half_ulp(|ref| + A, S), A = _LAYER_BOUND[mode] max|ref| -- the round-off test_tcn_gpu.py pins for the same MFMA chain on the same
    operands, plus the one rounding of the store;
  * the whole model against the chained restatement: 10x what was measured on the MI355X (roundings that fall the other way after
    an A-sized difference move the end-to-end figures by a storage ulp each); the measured values are printed (-rP) and recorded in
    profiles/r17_tcn_storage_parity_measured.txt."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.rounding import mround
from tests.resnet_storage_cases import half_ulp
from tests.tcn_cases import conv_bwd, golden_case, layer_inputs, rel
from tests.tcn_storage_cases import ST_SHAPES, BlockStages, TCNStorageRestated, block_params, drop_scale, st_layer
from tests.test_tcn_gpu import _LAYER_BOUND

gpu = pytest.mark.gpu
DEV = "cuda:0"
_ST = {"bf16": torch.bfloat16, "fp16": torch.float16}
_IDS = ["-".join(map(str, s)) for s in ST_SHAPES]
_EPILOGUES = ((False, False), (True, False), (True, True), (False, True))      # (relu, residual)
_REF = {}


def _nat():
    from wakeword_trainer_home_amd import _native as nat
    return nat


def _s(t, st):
    """A float64 tensor of values S holds -> the device tensor in S."""
    return t.float().to(st).to(DEV)


def _f(t):
    return t.float().to(DEV)


def _d(t):
    return t.detach().cpu().double()


def _int_case(shape, st, relu, residual):
    """Integer inputs and the restated layer, computed once per (shape, storage, epilogue)."""
    key = (shape, st, relu, residual)
    B, T, Cin, Cout, k, d = shape
    d_in = layer_inputs(B, T, Cin, Cout, k, seed=sum(shape) + 17, integer=True)
    if key not in _REF:
        _REF[key] = st_layer(d_in["x"], d_in["w"], d_in["b"], d_in["dy"], d, st, relu=relu, residual=d_in["res"] if residual else None)
    return d_in, _REF[key]


def _layer_gpu(d_in, d, st, relu, residual, **kw):
    nat = _nat()
    x, w, b, dy = _s(d_in["x"], st), _f(d_in["w"]), _f(d_in["b"]), _s(d_in["dy"], st)
    y = nat.tconv1d_st_fwd(x, w, b, d, relu=relu, residual=_s(d_in["res"], st) if residual else None)
    dx, dw, db = nat.tconv1d_st_bwd(x, w, dy, d, y=y if relu else None, **kw)
    return dict(y=y, dx=dx, dw=dw, db=db)


def _hold(what, got, ref_raw, st, mode):
    """|got - unrounded ref| <= A + half_ulp(|ref| + A, S) elementwise; -> the largest error as a fraction of its bound."""
    A = _LAYER_BOUND[mode] * ref_raw.abs().max().item()
    bound = A + half_ulp(ref_raw.abs() + A, st)
    frac = ((_d(got) - ref_raw).abs() / bound).max().item()
    print(f"tcn-storage {what} {mode}: worst error / bound = {frac:.3f} (A = {A:.2e})")
    assert frac <= 1.0, (what, frac)
    return A


# ------------------------------------------------------------------------------------------ 1. the layer on integer data
@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("shape", ST_SHAPES, ids=_IDS)
def test_layer_is_the_rounded_exact_result_on_integer_data(shape, mode):
    """y, dx, dw, db equal the restatement BIT FOR BIT over the four epilogues (bf16 rounds the integers above 256, ties to even);
    also dx accumulated onto a tensor of 3s, and no dx at all."""
    nat, st, d = _nat(), _ST[mode], shape[5]
    for relu, residual in _EPILOGUES:
        d_in, ref = _int_case(shape, st, relu, residual)
        got = _layer_gpu(d_in, d, st, relu, residual)
        assert got["y"].dtype is st and got["dx"].dtype is st and got["dw"].dtype is torch.float32 and got["db"].dtype is torch.float32
        for n in ("y", "dx", "dw", "db"):
            assert torch.equal(_d(got[n]), ref[n]), (n, relu, residual, (_d(got[n]) - ref[n]).abs().max().item())
    # (the last epilogue's tensors: no ReLU, so dpre is dy itself)
    x, w, dy = _s(d_in["x"], st), _f(d_in["w"]), _s(d_in["dy"], st)
    base = torch.full_like(x, 3.0)
    acc = st_layer(d_in["x"], d_in["w"], d_in["b"], d_in["dy"], d, st, dx_in=torch.full_like(d_in["x"], 3.0))
    dx2, dw2, db2 = nat.tconv1d_st_bwd(x, w, dy, d, dx=base)
    assert dx2 is base and torch.equal(_d(base), acc["dx"])
    dx3, dw3, db3 = nat.tconv1d_st_bwd(x, w, dy, d, need_dx=False)
    assert dx3 is None and torch.equal(dw3, dw2) and torch.equal(db3, db2) and torch.equal(_d(dw3), ref["dw"]) and torch.equal(_d(db3), ref["db"])


@gpu
@pytest.mark.parametrize("mode", list(_ST))
def test_layer_masks_with_two_saved_outputs_and_a_scale(mode):
    """The block's conv2: dpre = S(dy * scale) where the stored y != 0 and y2 != 0 (scale a power of two: still exact).  A stored
    -0 masks like +0."""
    nat, st = _nat(), _ST[mode]
    shape = ST_SHAPES[3]
    B, T, Cin, Cout, k, d = shape
    d_in, _ = _int_case(shape, st, False, False)
    g = torch.Generator().manual_seed(3)
    y1 = torch.randint(-1, 2, (B, T, Cout), generator=g).double()
    y2 = torch.randint(0, 2, (B, T, Cout), generator=g).double()
    y2d = _s(y2, st)
    y2d[0, 0, :4] = -0.0
    y2[0, 0, :4] = 0.0
    dx, dw, db = nat.tconv1d_st_bwd(_s(d_in["x"], st), _f(d_in["w"]), _s(d_in["dy"], st), d, y=_s(y1, st), y2=y2d, mask_scale=2.0)
    rx, rw, rb = conv_bwd(d_in["x"], d_in["w"], d_in["dy"] * 2.0 * (y1 != 0) * (y2 != 0), d, st)
    assert torch.equal(_d(dx), mround(rx, st)) and torch.equal(_d(dw), rw) and torch.equal(_d(db), rb)


@gpu
@pytest.mark.parametrize("mode", list(_ST))
def test_deferred_weight_gradient_equals_immediate(mode):
    """B T = 260: two row ranges.  Under the deferred reduction the sum of the partial products is queued (one item) and run by the
    flush; on integer data both orders of summation are exact, so the results are equal bit for bit."""
    nat, st = _nat(), _ST[mode]
    shape = ST_SHAPES[5]
    d_in, ref = _int_case(shape, st, False, False)
    lib, cx = nat.load(), nat.ctx(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    slot_w = torch.full(tuple(d_in["w"].shape), float("nan"), device=DEV)
    slot_b = torch.full((shape[3],), float("nan"), device=DEV)
    got = _layer_gpu(d_in, shape[5], st, False, False, dw_out=slot_w, db_out=slot_b, defer=True)
    assert lib.ww_deferred_reduce_pending(cx) == 1
    nat.deferred_flush(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    torch.cuda.synchronize()
    assert got["dw"] is slot_w and torch.equal(_d(slot_w), ref["dw"]) and torch.equal(_d(slot_b), ref["db"])
    assert torch.equal(_d(got["dx"]), ref["dx"])


# ------------------------------------------------------------------------------------------ 2. the layer's round-off
@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("shape", ST_SHAPES[-3:], ids=_IDS[-3:])
def test_layer_roundoff_against_restatement(shape, mode):
    """N(0,1) data rounded to S, linear epilogue (no mask to flip).  y and dx: the chain's round-off plus half an ulp of S; dw and db
    are fp32 results and keep the chain's bound relative to their largest entry."""
    st = _ST[mode]
    B, T, Cin, Cout, k, d = shape
    d_in = layer_inputs(B, T, Cin, Cout, k, seed=sum(shape), integer=False)
    d_in = {n: (mround(v, st) if n in ("x", "dy", "res") else v) for n, v in d_in.items()}
    ref = st_layer(d_in["x"], d_in["w"], d_in["b"], d_in["dy"], d, st)
    got = _layer_gpu(d_in, d, st, False, False)
    tag = "-".join(map(str, shape))
    _hold(f"layer {tag} y", got["y"], ref["y_raw"], st, mode)
    _hold(f"layer {tag} dx", got["dx"], ref["dx_raw"], st, mode)
    errs = {n: rel(_d(got[n]), ref[n]) for n in ("dw", "db")}
    print(f"tcn-storage layer {tag} {mode}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for n, e in errs.items():
        assert e <= _LAYER_BOUND[mode], (n, e)


# ------------------------------------------------------------------------------------------ 3. dropout
@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("shape", [(3, 7, 40), (2, 5, 8), (2, 9, 24)], ids=lambda s: "-".join(map(str, s)))
def test_dropout_bt_st_follows_the_philox_law_and_rounds_once(shape, mode):
    """A non-zero sample offset, a step beyond 2^32, stream ids 0, 1 and 15: the zero pattern is oracle.gru.dropout_bt_mask bit for
    bit, a kept value is S(x * scale) in fp32 arithmetic exactly, in place equals out of place, p = 0 is the identity."""
    from oracle.gru import dropout_bt_mask
    nat, st = _nat(), _ST[mode]
    B, T, Cc = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, T, Cc, generator=g).to(st)
    x[x == 0] = 1.0
    xd = x.to(DEV)
    p, step, off = 0.3, 2 ** 32 + 3, 5
    scale = torch.tensor(drop_scale(p, st), dtype=torch.float32)
    kept = (x.float() * scale).to(st)
    assert (kept != 0).all()
    for sid in (0, 1, 15):
        keep = torch.from_numpy(dropout_bt_mask(B, T, Cc, float(np.float32(p)), 9, step, off, sid))
        assert 0 < keep.sum() < keep.numel() or Cc * B * T < 100
        out = nat.dropout_bt_st(xd, p, seed=9, step=step, sample_offset=off, stream_id=sid)
        assert out.dtype is st and torch.equal(xd.cpu(), x)
        assert torch.equal(out.cpu() != 0, keep), sid
        assert torch.equal(out.cpu(), torch.where(keep, kept, torch.zeros_like(kept))), sid
        buf = xd.clone()
        assert nat.dropout_bt_st(buf, p, seed=9, step=step, sample_offset=off, stream_id=sid, out=buf) is buf and torch.equal(buf, out)
    assert torch.equal(nat.dropout_bt_st(xd, 0.0, seed=9, step=step, sample_offset=off, stream_id=1), xd)


# ------------------------------------------------------------------------------------------ 4. the input rounder
@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("shape", [(3, 40, 45), (2, 8, 1)], ids=lambda s: "-".join(map(str, s)))
def test_seq_round_st_transposes_and_rounds(shape, mode):
    nat, st = _nat(), _ST[mode]
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(*shape, generator=g) * 3.0).to(DEV)                     # (B, F, T)
    want = x.transpose(1, 2).to(st).contiguous()
    got = nat.seq_round_st(x, st)
    assert got.dtype is st and got.is_contiguous() and torch.equal(got, want)
    assert torch.equal(nat.seq_round_st(x[:, None].contiguous(), st), want)              # the Trainer's (B, 1, F, T)
    btf = x.transpose(1, 2).contiguous()
    assert torch.equal(nat.seq_round_st(btf, st, transposed=False), want)


@gpu
@pytest.mark.parametrize("mode", list(_ST))
def test_add_relu_st_is_the_rounded_sum(mode):
    nat, st = _nat(), _ST[mode]
    g = torch.Generator().manual_seed(8)
    a, b = torch.randn(3, 19, 24, generator=g).to(st).to(DEV), torch.randn(3, 19, 24, generator=g).to(st).to(DEV)
    assert torch.equal(nat.add_relu_st_fwd(a, b), (a.float() + b.float()).clamp_min(0.0).to(st))


# ------------------------------------------------------------------------------------------ 5. one block, stage by stage
def _spy(monkeypatch, nat, name, pick):
    seen, orig = [], getattr(nat, name)

    def spy(*a, **k):
        r = orig(*a, **k)
        seen.append(pick(r).clone())           # (a clone: the dropout pass and the accumulating dX write in place afterwards)
        return r
    monkeypatch.setattr(nat, name, spy)
    return seen


@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("cin,cout", [(40, 64), (32, 32)], ids=["downsample", "identity"])
def test_temporal_block_st_every_stored_tensor_meets_its_ops_bound(cin, cout, mode, monkeypatch):
    """Dropout 0.3, T = 23, B = 6, dilation 2.  Each stored tensor is held to the restated stage that made it, SEEDED WITH THE
    DEVICE'S OWN stored predecessors: convolution outputs, out, dh1 and dx under the layer bound plus half an ulp (a ReLU decision may
    differ only where the restated pre-activation is within A of zero), the dropout passes bit for bit."""
    from oracle.gru import dropout_bt_mask
    from wakeword_trainer_home_amd.models.tcn import TemporalBlock
    nat, st = _nat(), _ST[mode]
    B, T, d, p = 6, 23, 2, 0.3
    torch.manual_seed(cin)
    blk = TemporalBlock(cin, cout, 3, d, dropout=p, mode=mode, storage=mode, stream_ids=(18, 19)).to(DEV).train()
    blk.dropout_seed, blk.dropout_step, blk.sample_offset = 7, 4, 3
    g = torch.Generator().manual_seed(cout)
    x = mround(torch.randn(B, T, cin, generator=g).double(), st)
    dout = mround(torch.randn(B, T, cout, generator=g).double(), st)
    ys = _spy(monkeypatch, nat, "tconv1d_st_fwd", lambda r: r)
    dxs = _spy(monkeypatch, nat, "tconv1d_st_bwd", lambda r: r[0])
    xd = _s(x, st).requires_grad_(True)
    out = blk(xd)
    saved = out.grad_fn.saved_tensors
    h1, h2, o = (_d(t) for t in saved[1:4])
    out.backward(_s(dout, st))
    assert out.dtype is st and xd.grad.dtype is st and len(ys) == (3 if cin != cout else 2) and len(dxs) == len(ys)
    sd = {n: _d(q) for n, q in blk.state_dict().items()}
    keep = [torch.from_numpy(dropout_bt_mask(B, T, cout, float(np.float32(p)), 7, 4, 3, s)).double() for s in (2, 3)]
    S = BlockStages(block_params(sd, ""), d, st, keep[0], keep[1], drop_scale(p, st))
    tag = f"block {cin}->{cout}"
    # forward: y1 -> h1 -> y2 -> h2 -> out
    r1 = S.h1(x)
    A = _hold(tag + " y1", ys[0], r1["y_raw"], st, mode)
    flips = (_d(ys[0]) != 0) != (r1["pre"] > 0)
    assert (r1["pre"][flips].abs() <= A).all()
    assert torch.equal(h1, mround(_d(ys[0]) * (keep[0] * S.scale), st)) and torch.equal(h1 != 0, (keep[0] != 0) & (_d(ys[0]) != 0))
    r2 = S.h2(h1)
    A = _hold(tag + " y2", ys[1], r2["y_raw"], st, mode)
    flips = (_d(ys[1]) != 0) != (r2["pre"] > 0)
    assert (r2["pre"][flips].abs() <= A).all()
    assert torch.equal(h2, mround(_d(ys[1]) * (keep[1] * S.scale), st))
    ro = S.out(x, h2)
    A = _hold(tag + " out", out, ro["raw"], st, mode)
    assert torch.equal(o, _d(out)) and (ro["pre"][(o != 0) != (ro["pre"] > 0)].abs() <= A).all()
    # backward: the skip path, conv2 (dh1), conv1 (dx) -- in the order the block runs them
    sk = S.bwd_skip(x, o, dout)
    dskip = _d(dxs[0]) if S.down else sk["dx"]
    if S.down:
        _hold(tag + " dskip", dxs[0], sk["dx_raw"], st, mode)
    c2 = S.bwd_conv2(h1, h2, o, dout)
    _hold(tag + " dh1", dxs[-2], c2["dx_raw"], st, mode)
    c1 = S.bwd_conv1(x, h1, _d(dxs[-2]), dskip)
    _hold(tag + " dx", xd.grad, c1["dx_raw"], st, mode)
    assert torch.equal(xd.grad, dxs[-1])
    grads = {"conv2.weight": c2["dw"], "conv2.bias": c2["db"], "conv1.weight": c1["dw"], "conv1.bias": c1["db"]}
    if S.down:
        grads.update({"downsample.weight": sk["dw"], "downsample.bias": sk["db"]})
    errs = {n: rel(_d(q.grad), grads[n]) for n, q in blk.named_parameters()}
    print(f"tcn-storage {tag} {mode}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert set(errs) == set(grads)
    for n, e in errs.items():
        assert e <= _LAYER_BOUND[mode], (n, e)


# ------------------------------------------------------------------------------------------ 6. the model
# TCNWakeword(mode=S, storage=S) against the chained restatement on both fixture cases, dropout 0 / 0.3 / eval: (logits absolute, loss
# absolute, gradients as |got - ref|_2 / |ref|_2 per tensor and relative to their largest entry); 10x the largest value measured on the
# MI355X over those runs (profiles/r17_tcn_storage_parity_measured.txt).  The block test above is the tight guard; this one catches wiring.
# Measured: bf16 logits 1.30e-8, loss 3.56e-8, grads_l2 5.82e-6, grads 3.76e-5 (no stored value fell the other way: what is left is fp32
# round-off); fp16 logits 3.70e-6, loss 5.46e-7, grads_l2 5.42e-4, grads 1.10e-3 (a few stored values one fp16 ulp apart).
_MODEL_BOUND = {"bf16": dict(logits=1.3e-7, loss=3.6e-7, grads_l2=5.8e-5, grads=3.8e-4),
                "fp16": dict(logits=3.7e-5, loss=5.5e-6, grads_l2=5.4e-3, grads=1.1e-2)}
_CASES = [("", {}), ("small.", dict(num_channels=[32, 48], kernel_size=2))]


def _model(sd, **kw):
    from wakeword_trainer_home_amd.models import TCNWakeword
    m = TCNWakeword(**kw)
    m.load_state_dict(sd)
    return m.to(DEV)


@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("prefix,kw", _CASES, ids=["default", "small"])
def test_tcnwakeword_st_matches_chained_restatement(prefix, kw, mode):
    st = _ST[mode]
    sd, g = golden_case(prefix)
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])                  # (B, F, T)
    xr = x.double().transpose(1, 2)
    worst = dict(logits=0.0, loss=0.0, grads_l2=0.0, grads=0.0)
    for dropout in (0.0, 0.3):
        model = _model(sd, dropout=dropout, dropout_seed=5, mode=mode, storage=mode, **kw)
        oracle = TCNStorageRestated(sd, dropout=dropout, seed=5, st=st)
        model.eval()
        with torch.no_grad():
            ev = model(x.to(DEV))
        worst["logits"] = max(worst["logits"], (_d(ev) - oracle.forward(xr, training=False)).abs().max().item())
        model.train()
        out = model(x.to(DEV))
        loss = torch.nn.functional.cross_entropy(out, y.to(DEV))
        loss.backward()
        ref, lo, go, _ = oracle.loss_and_grads(xr, y)
        assert out.dtype is torch.float32 and all(q.grad.dtype is torch.float32 and torch.isfinite(q.grad).all() for q in model.parameters())
        e = dict(logits=(_d(out) - ref).abs().max().item(), loss=abs(loss.item() - lo),
                 grads_l2=max(((_d(q.grad) - go[n]).norm() / go[n].norm()).item() for n, q in model.named_parameters()),
                 grads=max(rel(_d(q.grad), go[n]) for n, q in model.named_parameters()))
        print(f"tcn-storage model '{prefix}' {mode} dropout {dropout}: eval {(_d(ev) - oracle.forward(xr, training=False)).abs().max().item():.2e} " +
              " ".join(f"{k}={v:.2e}" for k, v in e.items()))
        worst = {k: max(worst[k], e[k]) for k in worst}
    for k, v in worst.items():
        assert v <= _MODEL_BOUND[mode][k], (k, v)


@gpu
@pytest.mark.parametrize("mode", list(_ST))
def test_tcnwakeword_st_properties(mode):
    """The three input orientations give the same bits; two identical training steps give identical bits; checkpoints interchange
    with the fp32-storage model (keys, shapes and dtypes identical, both ways)."""
    sd, g = golden_case("")
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    model = _model(sd, dropout=0.0, mode=mode, storage=mode).eval()
    with torch.no_grad():
        ev = model(x)
        assert torch.isfinite(ev).all() and torch.equal(model(x[:, None].contiguous()), ev) and torch.equal(model(x.transpose(1, 2).contiguous()), ev)
        assert torch.equal(model(x[1:].contiguous())[0], ev[1])
    runs = []
    for _ in range(2):
        m = _model(sd, dropout=0.3, dropout_seed=4, mode=mode, storage=mode).train()
        out = m(x)
        torch.nn.functional.cross_entropy(out, y).backward()
        runs.append((out.detach().clone(), [q.grad.clone() for q in m.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    wide = _model(sd, dropout=0.0, mode=mode)
    a, b = wide.state_dict(), model.state_dict()
    assert list(a) == list(b) and all(a[k].dtype is b[k].dtype and a[k].shape == b[k].shape for k in a)
    model.load_state_dict(a)
    wide.load_state_dict(b)
    assert all(torch.equal(model.state_dict()[k], sd[k].to(DEV)) for k in sd)
    # the input's own gradient (off the training path) exists and is finite
    xg = x.clone().requires_grad_(True)
    model.train()
    model(xg).sum().backward()
    assert xg.grad is not None and xg.grad.shape == x.shape and torch.isfinite(xg.grad).all() and xg.grad.abs().max() > 0


@gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_storage_fp32_is_the_model_built_without_the_argument(mode):
    sd, g = golden_case("")
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    runs = []
    for kw in ({}, {"storage": "fp32"}):
        m = _model(sd, dropout=0.3, dropout_seed=2, mode=mode, **kw).train()
        out = m(x)
        torch.nn.functional.cross_entropy(out, y).backward()
        runs.append((out.detach(), [q.grad for q in m.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


# ------------------------------------------------------------------------------------------ 7. the Trainer
def _trainer_cfg(batch_size=8, epochs=1):
    from wakeword_trainer_home_amd.config import get_preset
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = epochs, 0, batch_size
    cfg.loss.label_smoothing = 0.0
    cfg.optimizer.mixed_precision = False
    cfg.training.checkpoint_frequency = "best_only"
    return cfg


def _batches(n, seed):
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    wave, y = make_synthetic_batch(n, 7040, seed=seed)                 # 7040 samples: 45 frames
    y[::3] = 1
    return [(wave[i:i + 8], y[i:i + 8]) for i in range(0, n, 8)]


@gpu
@pytest.mark.parametrize("mode", list(_ST))
def test_trainer_trains_and_graph_replays_equal_eager_steps_bit_for_bit(mode, tmp_path):
    """The public train() over two epochs of 3 steps of batch 8, eager and hip_graph=True: finite losses that change, and the replays
    equal the eager steps bit for bit (loss trace, parameters, optimizer moments).  fp16 runs under the DeviceGradScaler.  The graph key names the
    storage."""
    from wakeword_trainer_home_amd.models import TCNWakeword
    from wakeword_trainer_home_amd.training import Trainer
    from wakeword_trainer_home_amd.training.optimizer_factory import DeviceGradScaler, FlatFusedOptimizer
    batches = _batches(24, seed=6)
    runs = []
    for graph in (False, True):
        cfg = _trainer_cfg(epochs=2)
        cfg.training.hip_graph, cfg.training.hip_graph_auto = graph, False
        torch.manual_seed(11)
        model = TCNWakeword(dropout=0.3, dropout_seed=2, mode=mode, storage=mode)
        t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path / f"g{int(graph)}", device=DEV)
        assert isinstance(t.optimizer, FlatFusedOptimizer) and t._async_autograd
        assert isinstance(getattr(t, "scaler", None), DeviceGradScaler) == (mode == "fp16")
        rec = []
        t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: rec.append((i, l))})())
        t.train()
        runs.append((t, rec, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, copy.deepcopy(t.optimizer.state_dict())))
    assert runs[1][0]._graph is not None and runs[0][0]._graph is None
    assert len(runs[1][1]) == 6 and all(np.isfinite(l) for _, l in runs[0][1]) and len({l for _, l in runs[0][1]}) > 1
    assert runs[0][1] == runs[1][1], "loss traces differ"
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    for (ka, va), (kb, vb) in zip(sorted(runs[0][3]["state"].items()), sorted(runs[1][3]["state"].items())):
        for f in va:
            assert torch.equal(torch.as_tensor(va[f]).cpu(), torch.as_tensor(vb[f]).cpu()), (ka, f)
    t = runs[1][0]
    shape = (8, 1, 40, 45)
    key = t._graph_key(shape)
    assert key in t._graphs
    wide = Trainer._graph_mode_key(type("T", (), {"model": TCNWakeword(mode=mode)})())
    assert t._graph_mode_key() != wide
    blk = t.model.tcn.network[0]
    blk.storage = torch.float32
    assert t._graph_key(shape) != key and t._graph_key(shape) not in t._graphs
    blk.storage = _ST[mode]
    assert t._graph_key(shape) == key


@gpu
def test_fp16_step_scaled_to_overflow_is_skipped_on_the_device(tmp_path):
    """A loss scale of 2^40: S(dpooled / T) and everything after it overflow fp16, the fused optimizer gets the flag on the device,
    no parameter moves and the scale halves; at the scaler's own 65536 the same batch is applied."""
    from wakeword_trainer_home_amd.models import TCNWakeword
    from wakeword_trainer_home_amd.training import Trainer
    nat = _nat()
    cfg = _trainer_cfg()
    torch.manual_seed(2)
    model = TCNWakeword(dropout=0.0, mode="fp16", storage="fp16")
    batches = _batches(8, seed=6)
    t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path, device=DEV)
    assert t.scaler.get_scale() == 65536.0
    t.scaler.state.copy_(nat.loss_scale_new("cpu", 2.0 ** 40))
    before = {k: v.clone() for k, v in model.state_dict().items()}
    t.train_epoch(0)
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    assert t.scaler.get_scale() == 2.0 ** 39
    t.scaler.state.copy_(nat.loss_scale_new("cpu", 65536.0))
    t.train_epoch(1)
    torch.cuda.synchronize()
    assert any(not torch.equal(before[k], v) for k, v in model.state_dict().items())
    assert all(torch.isfinite(v).all() for v in model.state_dict().values())


# ------------------------------------------------------------------------------------------ 8. argument checks
@gpu
def test_argument_checks_return_error_codes_before_any_launch():
    """Null arguments, WW_ACT_F32 or an unknown code as the storage, channel counts that are no multiple of 8, misaligned pointers, k
    outside 1..8 and a dilation of 0 are WW_E_INVALID, a short scratch is WW_E_WORKSPACE -- before any launch: the output buffers
    keep their sentinel.  The bindings raise WW_E_INVALID as ValueError."""
    nat = _nat()
    lib, cx = nat.load(), nat.ctx(DEV)
    B, T, Cin, Cout, k = 2, 5, 8, 16, 3
    h = lambda *s: torch.full(s, 7.0, device=DEV, dtype=torch.bfloat16)
    f = lambda *s: torch.full(s, 7.0, device=DEV)
    x, w, b, y, dx, dw, db = h(B, T, Cin), f(Cout, Cin, k), f(Cout), h(B, T, Cout), h(B, T, Cin), f(Cout, Cin, k), f(Cout)
    nbytes = lib.ww_tconv1d_st_scratch_bytes(1, B, T, Cin, Cout, k)
    scratch = f(nbytes // 4 + 4)
    p = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + off)
    fwd = lambda st=1, cin=Cin, cout=Cout, kk=k, d=1, sb=nbytes, xx=p(x): lib.ww_tconv1d_st_fwd(cx, st, xx, p(w), p(b), B, T, cin, cout, kk, d, 0,
                                                                                             None, p(y), p(scratch), sb, None)
    assert fwd(st=0) == -1 and b"storage" in lib.ww_last_error()
    assert fwd(st=3) == -1 and fwd(cin=12) == -1 and b"multiples of 8" in lib.ww_last_error()
    assert fwd(cout=20) == -1 and fwd(xx=None) == -1 and fwd(kk=0) == -1 and b"kernel_size" in lib.ww_last_error()
    assert fwd(kk=9) == -1 and fwd(d=0) == -1 and b"dilation" in lib.ww_last_error()
    assert fwd(xx=p(x, 2)) == -1 and b"aligned" in lib.ww_last_error()
    assert fwd(sb=nbytes - 4) == -3 and b"scratch too small" in lib.ww_last_error()
    bwd = lambda st=1, cin=Cin, kk=k, d=1, sb=nbytes, gg=p(y): lib.ww_tconv1d_st_bwd(cx, st, p(x), p(w), None, None, 1.0, gg, B, T, cin, Cout, kk, d,
                                                                                     p(dx), 0, p(dw), p(db), p(scratch), sb, None)
    assert bwd(st=0) == -1 and bwd(cin=12) == -1 and bwd(gg=None) == -1 and bwd(kk=9) == -1 and bwd(d=0) == -1
    assert bwd(gg=p(y, 2)) == -1 and bwd(sb=16) == -3
    drop = lambda st=1, c=Cin, xx=p(x), pp=0.3, sid=1: lib.ww_dropout_bt_st(cx, st, xx, B, T, c, pp, 0, 0, 0, sid, p(dx), None)
    assert drop(st=0) == -1 and drop(c=12) == -1 and drop(xx=None) == -1 and drop(pp=1.0) == -1 and drop(xx=p(x, 2)) == -1
    assert drop(sid=16) not in (0, -1)                                      # WW_E_UNSUPPORTED
    add = lambda st=1, n=x.numel(), aa=p(x): lib.ww_add_relu_st_fwd(cx, st, aa, p(x), n, p(dx), None)
    assert add(st=0) == -1 and add(n=12) == -1 and add(aa=None) == -1 and add(aa=p(x, 2)) == -1
    img = f(B, Cin, T)
    rnd = lambda st=1, ff=Cin, xx=p(img), tr=1, oo=p(dx): lib.ww_seq_round_st(cx, st, xx, B, T, ff, tr, oo, None)
    assert rnd(st=0) == -1 and rnd(ff=12) == -1 and rnd(xx=None) == -1 and rnd(oo=p(dx, 2)) == -1 and rnd(tr=0, xx=p(img, 4)) == -1
    torch.cuda.synchronize()
    for t in (y, dx, dw, db):
        assert t.eq(7.0).all()          # nothing was launched
    with pytest.raises(ValueError, match="multiples of 8"):
        nat.tconv1d_st_fwd(h(B, T, 12), f(Cout, 12, k), b)
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        nat.tconv1d_st_fwd(f(B, T, Cin), w, b)
    with pytest.raises(ValueError, match="one dtype"):
        nat.tconv1d_st_bwd(x, w, y.half(), 1)
    with pytest.raises(ValueError):
        nat.tconv1d_st_fwd(x, f(Cout, Cin + 8, k), b)                       # x and weight disagree about Cin: caught at the binding
