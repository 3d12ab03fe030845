"""LSTM layer kernels (ww_lstm_*) and LSTMWakeword, the reference's LSTM model (src/models/architectures.py: nn.LSTM(input,
128, num_layers, batch_first=True, dropout, bidirectional) -> final hidden states of the last layer -> Dropout -> Linear).

References: torch.nn.LSTM on the CPU in float64 (its arithmetic IS the reference's); the reference's own model through
tests/golden/g8_lstm.npz (make_golden_lstm.py); a float64 restatement of the stack with the build's Philox dropout masks
(oracle.gru.dropout_bt_mask, the ww_dropout_bt law); and a float64 restatement of one direction that rounds exactly what the
16-bit matrix modes round (oracle.rounding.mround)."""
import copy
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.lstm_cases import _BOUND, _inputs, lstm_restated

gpu = pytest.mark.gpu
DEV = "cuda:0"
H = 128
_MD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
_MT = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}


def _rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


def _golden():
    return np.load(Path(__file__).parent / "golden" / "g8_lstm.npz")


def _case(g, prefix):
    """-> (state dict, fixture arrays) of one case.  The fixture keeps the parameters as a seed of make_golden_lstm's
    reference_params (plus sampled values to confirm the regeneration) and the gradients as samples + their largest |entry|."""
    from tests.golden.make_golden_lstm import reference_params, sample_index
    keys = [str(k) for k in g[prefix + "keys"]]
    shapes = {k: g[prefix + "shape." + k] for k in keys}
    params = reference_params(int(g[prefix + "param_seed"]), keys, shapes)
    for k in keys:
        assert np.array_equal(params[k].reshape(-1)[sample_index(params[k].size)], g[prefix + "psamp." + k]), k
    sd = {k: torch.from_numpy(params[k]) for k in keys}
    arrays = {k: g[prefix + k] for k in ("x", "y", "logits_eval", "logits_train", "loss")}
    arrays["gsamp"] = {k: g[prefix + "gsamp." + k] for k in keys}
    arrays["gmax"] = {k: float(g[prefix + "gmax." + k]) for k in keys}
    return sd, arrays


def _sampled_rel(grad, g, name):
    """Error of a gradient at the fixture's sampled entries, relative to the reference gradient's largest |entry|."""
    from tests.golden.make_golden_lstm import sample_index
    got = grad.detach().cpu().double().reshape(-1)[torch.from_numpy(sample_index(grad.numel()))]
    return (got - torch.from_numpy(g["gsamp"][name]).double()).abs().max().item() / g["gmax"][name]


# ------------------------------------------------------------------------------------------ CPU
def test_constructor_defaults_are_the_reference_ones():
    from wakeword_trainer_home_amd.models import LSTMWakeword
    m = LSTMWakeword()
    assert (m.lstm.input_size, m.hidden_size, m.num_layers, m.bidirectional) == (40, 128, 2, True)
    assert m.lstm.dropout == pytest.approx(0.3) and m.fc[0].p == pytest.approx(0.3)
    assert m.lstm.dropout_seed == 0 and m.lstm.mode == torch.float32 and m.hip_backed
    assert m.fc[1].weight.shape == (2, 256)
    assert LSTMWakeword(num_layers=1).lstm.dropout == 0.0           # nn.LSTM: no inter-layer dropout for one layer
    k = 128 ** -0.5                                                  # nn.LSTM.reset_parameters: U(-1/sqrt(H), 1/sqrt(H))
    assert all(p.abs().max().item() <= k for n, p in m.named_parameters() if n.startswith("lstm."))


def test_state_dict_matches_reference_fixture():
    from wakeword_trainer_home_amd.models import LSTMWakeword
    from wakeword_trainer_home_amd.models.architectures import LSTMWakeword as FromArch
    assert FromArch is LSTMWakeword
    g = _golden()
    for prefix, kw in (("", {}), ("uni.", dict(num_layers=1, bidirectional=False))):
        sd, _ = _case(g, prefix)
        m = LSTMWakeword(dropout=0.0, **kw)
        assert list(m.state_dict().keys()) == [str(k) for k in g[prefix + "keys"]]
        assert all(tuple(v.shape) == tuple(g[prefix + "shape." + k]) for k, v in m.state_dict().items())
        m.load_state_dict(sd)
        assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert tuple(g["shape.lstm.weight_ih_l0"]) == (512, 40) and len(g["keys"]) == 18 and len(g["uni.keys"]) == 6


@pytest.mark.parametrize("prefix,layers,bidir", [("", 2, True), ("uni.", 1, False)])
def test_float64_restatement_matches_reference_fixture(prefix, layers, bidir):
    """The float64 model the GPU tests compare whole gradients with (LSTMOracle) is the reference's LSTMWakeword: its eval and
    train logits, loss and sampled parameter gradients equal the fixture's to float32 round-off."""
    sd, g = _case(_golden(), prefix)
    oracle = LSTMOracle(layers, bidir, dropout=0.0)
    oracle.load_reference_state_dict(sd)
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    with torch.no_grad():
        ev = oracle(x, training=False)
    assert (ev - torch.from_numpy(g["logits_eval"]).double()).abs().max().item() <= 1e-5
    out = oracle(x, training=True)
    loss = torch.nn.functional.cross_entropy(out, y)
    loss.backward()
    assert (out.detach() - torch.from_numpy(g["logits_train"]).double()).abs().max().item() <= 1e-5
    assert abs(loss.item() - float(g["loss"])) <= 1e-6
    grads = oracle.reference_grads()
    assert sorted(grads) == sorted(g["gsamp"])
    for n, gr in grads.items():
        assert _sampled_rel(gr, g, n) <= 1e-5, n


def test_cpu_forward_has_no_fallback():
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.models import LSTMWakeword
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        LSTMWakeword()(torch.zeros(2, 5, 40))


def test_hidden_size_other_than_128_raises():
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.models import LSTMWakeword
    with pytest.raises(nat.NativeError, match="hidden_size == 128"):
        LSTMWakeword(hidden_size=64)


def test_factory_still_refuses_lstm():
    from wakeword_trainer_home_amd.models import create_model
    with pytest.raises(ValueError, match="outside this build"):
        create_model("lstm")


# ------------------------------------------------------------------------------------------ restatements
class LSTMOracle(torch.nn.Module):
    """The reference model in float64 with single-layer nn.LSTM modules and the build's Philox masks between layers (stream
    1 + k) and in front of fc (stream 15)."""

    def __init__(self, num_layers=2, bidirectional=True, dropout=0.3, seed=0):
        super().__init__()
        nd = 2 if bidirectional else 1
        self.layers = torch.nn.ModuleList([torch.nn.LSTM(40 if k == 0 else nd * H, H, batch_first=True,
                                                         bidirectional=bidirectional) for k in range(num_layers)]).double()
        self.fc = torch.nn.Linear(nd * H, 2).double()
        self.p = float(np.float32(dropout)) if num_layers > 1 else 0.0
        self.p_fc = float(np.float32(dropout))
        self.seed, self.nd = seed, nd

    def load_reference_state_dict(self, sd):
        for k, layer in enumerate(self.layers):
            for sfx in ("", "_reverse")[:self.nd]:
                for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    getattr(layer, f"{name}_l0{sfx}").data.copy_(sd[f"lstm.{name}_l{k}{sfx}"].double())
        self.fc.weight.data.copy_(sd["fc.1.weight"].double())
        self.fc.bias.data.copy_(sd["fc.1.bias"].double())

    def reference_grads(self):
        """{reference state-dict key: gradient} of the parameters (lstm.weight_ih_l1_reverse ... fc.1.bias)."""
        out = {}
        for k, layer in enumerate(self.layers):
            for n, p in layer.named_parameters():
                out["lstm." + n.replace("_l0", f"_l{k}")] = p.grad
        out["fc.1.weight"], out["fc.1.bias"] = self.fc.weight.grad, self.fc.bias.grad
        return out

    def forward(self, x, step=0, sample_offset=0, training=True):
        from oracle.gru import dropout_bt_mask
        if x.dim() == 4:
            x = x[:, 0].transpose(1, 2)
        x = x.double()
        B, T, _ = x.shape
        for k, layer in enumerate(self.layers):
            x, (hn, _) = layer(x)
            if training and self.p > 0 and k + 1 < len(self.layers):
                keep = torch.from_numpy(dropout_bt_mask(B, T, x.shape[2], self.p, self.seed, step, sample_offset, 1 + k))
                x = x * keep.double() * (1.0 / (1.0 - self.p))
        h = torch.cat([hn[0], hn[1]], dim=1) if self.nd == 2 else hn[0]
        if training and self.p_fc > 0:
            keep = torch.from_numpy(dropout_bt_mask(B, 1, h.shape[1], self.p_fc, self.seed, step, sample_offset, 15))[:, 0]
            h = h * keep.double() * (1.0 / (1.0 - self.p_fc))
        return self.fc(h)


# ------------------------------------------------------------------------------------------ GPU: one direction
@pytest.fixture(params=[8, 16])
def lstm_rows(request, monkeypatch):
    """Both workgroup shapes of the recurrent kernels (8 or 16 batch rows per workgroup; the library picks by batch size)."""
    monkeypatch.setenv("WW_LSTM_ROWS", str(request.param))
    return request.param


# (B, T, I, reverse, with h0 / c0, with dc_n): every B in {1, 7, 16, 40, 512}, T in {1, 31, 76}, I in {40, 64, 256}
_DIR = [(1, 1, 40, False, False, False), (7, 31, 64, True, True, True), (16, 76, 256, False, True, False),
        (40, 31, 40, True, False, True), (512, 76, 64, False, True, True), (40, 76, 256, True, True, False),
        (7, 1, 256, True, True, True)]


@gpu
@pytest.mark.parametrize("B,T,I,reverse,states,dcn", _DIR)
def test_lstm_direction_matches_float64_torch(B, T, I, reverse, states, dcn, lstm_rows):
    """ww_lstm_fwd / ww_lstm_bwd (fp32) against float64 torch.nn.LSTM: y, h_n, c_n <= 2e-5 abs; dX, dW_ih, dW_hh, both
    biases, dh0 and dc0 <= 2e-4 relative to each tensor's largest entry."""
    from wakeword_trainer_home_amd import _native as nat
    d = _inputs(B, T, I, B * 7 + T + I, 1)
    w_ih, w_hh, b_ih, b_hh = [p.clone().requires_grad_(True) for p in d["P"][0]]
    x = d["x"].clone().requires_grad_(True)
    h0 = (d["h0"][0] if states else torch.zeros(B, H, dtype=torch.float64)).clone().requires_grad_(True)
    c0 = (d["c0"][0] if states else torch.zeros(B, H, dtype=torch.float64)).clone().requires_grad_(True)
    ref = torch.nn.LSTM(I, H, batch_first=True).double()
    with torch.no_grad():
        for n, p in zip(("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"), (w_ih, w_hh, b_ih, b_hh)):
            getattr(ref, n).copy_(p)
    xin = x.flip(1) if reverse else x
    out, (hn, cn) = ref(xin, (h0[None], c0[None]))
    out = out.flip(1) if reverse else out
    dy, dhn = d["dy"], d["dhn"][0]
    dcn_t = d["dcn"][0] if dcn else torch.zeros(B, H, dtype=torch.float64)
    ((out * dy).sum() + (hn[0] * dhn).sum() + (cn[0] * dcn_t).sum()).backward()
    gx, gh0, gc0 = x.grad, h0.grad, c0.grad
    gp = [getattr(ref, n).grad for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]

    f = lambda t: t.detach().float().to(DEV)
    ybuf = torch.zeros(B, T, 2 * H, device=DEV)                    # the direction writes one half of a (B,T,2H) buffer
    sl = slice(H, 2 * H) if reverse else slice(0, H)
    ws = nat.lstm_workspace(B, T, I, H, DEV)
    Pd = [f(p) for p in d["P"][0]]
    h_n, c_n = nat.lstm_fwd(f(x), *Pd, ybuf[:, :, sl], ws, h0=f(h0) if states else None, c0=f(c0) if states else None,
                            reverse=reverse)
    assert (ybuf[:, :, sl].cpu().double() - out.detach()).abs().max().item() <= 2e-5
    assert (h_n.cpu().double() - hn[0].detach()).abs().max().item() <= 2e-5
    assert (c_n.cpu().double() - cn[0].detach()).abs().max().item() <= 2e-5
    other = slice(0, H) if reverse else slice(H, 2 * H)
    assert ybuf[:, :, other].abs().max().item() == 0.0
    dybuf = torch.zeros(B, T, 2 * H, device=DEV)
    dybuf[:, :, sl] = f(dy)
    dx = torch.full((B, T, I), 1.0, device=DEV)
    g = nat.lstm_bwd(f(x), Pd[0], Pd[1], dybuf[:, :, sl], f(dhn), f(dcn_t) if dcn else None, ws, reverse=reverse, dx=dx,
                     accumulate_dx=True, want_dh0=True)
    tol = 2e-4
    assert _rel(dx.cpu().double() - 1.0, gx) <= tol
    for got, want, name in zip(g[:4], gp, ("dw_ih", "dw_hh", "db_ih", "db_hh")):
        assert _rel(got.cpu().double(), want) <= tol, name
    assert _rel(g[4].cpu().double(), gh0) <= tol
    assert _rel(g[5].cpu().double(), gc0) <= tol


# ------------------------------------------------------------------------------------------ GPU: bidirectional layer
def _bidir(d, B, T, I, mode, outs=None, defer=False):
    from wakeword_trainer_home_amd import _native as nat
    f = lambda t: t.float().to(DEV)
    md = _MD[mode]
    params = [[f(p) for p in d["P"][k]] for k in range(2)]
    xd, dyd = f(d["x"]), f(d["dy"])
    ws = [nat.lstm_workspace(B, T, I, H, DEV) for _ in range(2)]
    y = torch.zeros(B, T, 2 * H, device=DEV)
    h_n, c_n = nat.lstm_bidir_fwd(xd, params, y, ws, mode=md, h0=[f(t) for t in d["h0"]], c0=[f(t) for t in d["c0"]])
    dx = torch.zeros(B, T, I, device=DEV)
    dh0 = [torch.empty(B, H, device=DEV) for _ in range(2)]
    dc0 = [torch.empty(B, H, device=DEV) for _ in range(2)]
    grads = nat.lstm_bidir_bwd(xd, params, dyd, [f(t) for t in d["dhn"]], ws, dx=dx, mode=md, outs=outs, defer=defer, dh0=dh0,
                               dc_n=[f(t) for t in d["dcn"]], dc0=dc0)
    got = {"y": y, "dx": dx}
    for k in range(2):
        got[f"h_n{k}"], got[f"c_n{k}"], got[f"dh0{k}"], got[f"dc0{k}"] = h_n[k], c_n[k], dh0[k], dc0[k]
        for n, g in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), grads[k]):
            got[f"{n}{k}"] = g
    return got


@gpu
@pytest.mark.parametrize("B,T,I", [(7, 31, 40), (40, 13, 256), (64, 80, 64)])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_bidirectional_layer_in_one_launch_equals_two_launches(B, T, I, mode, lstm_rows):
    """ww_lstm_bidir_fwd / _bwd (both directions as the two rows of ONE recurrent launch) are BIT-identical to the two
    per-direction launches -- except dx: one product over both directions' (dG, W_ih) pairs there, a product plus an accumulating
    one here (the same terms in another order of fp32 additions, <= 2e-6 relative)."""
    from wakeword_trainer_home_amd import _native as nat
    d = _inputs(B, T, I, B + T + I, 2)
    got = _bidir(d, B, T, I, mode)
    f = lambda t: t.float().to(DEV)
    md = _MD[mode]
    y1 = torch.zeros(B, T, 2 * H, device=DEV)
    dx1 = torch.zeros(B, T, I, device=DEV)
    for k in range(2):
        Pd = [f(p) for p in d["P"][k]]
        ws = nat.lstm_workspace(B, T, I, H, DEV)
        h_n, c_n = nat.lstm_fwd(f(d["x"]), *Pd, y1[:, :, k * H:(k + 1) * H], ws, h0=f(d["h0"][k]), c0=f(d["c0"][k]),
                                reverse=(k == 1), mode=md)
        assert torch.equal(h_n, got[f"h_n{k}"]) and torch.equal(c_n, got[f"c_n{k}"])
        g = nat.lstm_bwd(f(d["x"]), Pd[0], Pd[1], f(d["dy"][:, :, k * H:(k + 1) * H]), f(d["dhn"][k]), f(d["dcn"][k]), ws,
                         reverse=(k == 1), dx=dx1, accumulate_dx=(k == 1), want_dh0=True, mode=md)
        for n, t in zip(("dw_ih", "dw_hh", "db_ih", "db_hh", "dh0", "dc0"), g):
            assert torch.equal(t, got[f"{n}{k}"]), (n, k)
    assert torch.equal(y1, got["y"])
    ddx = _rel(got["dx"].double(), dx1.double())
    print(f"lstm bidirectional dx, one product vs product + accumulate ({mode}): {ddx:.2e}")
    assert ddx <= 2e-6


_REF = {}


def _check(tag, mode, got, ref):
    b_fwd, b_st, b_rel = _BOUND[mode]
    errs = {}
    for k, r in ref.items():
        a = got[k].detach().cpu().double()
        errs[k] = (a - r).abs().max().item() if k.startswith(("y", "h_n", "c_n", "dh0", "dc0")) else _rel(a, r)
    print(f"restated-lstm {tag} {mode}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, e in errs.items():
        lim = b_fwd if k.startswith(("y", "h_n", "c_n")) else b_st if k.startswith(("dh0", "dc0")) else b_rel
        assert e <= lim, (tag, mode, k, e)
    return errs


def _bidir_ref(B, T, I, mode):
    key = (B, T, I, mode)
    d = _inputs(B, T, I, 1000 + B + T + I, 2)
    if key not in _REF:
        o = [lstm_restated(d["x"], *d["P"][k], h0=d["h0"][k], c0=d["c0"][k], dy=d["dy"][:, :, k * H:(k + 1) * H], dh_n=d["dhn"][k],
                           dc_n=d["dcn"][k], mtype=_MT[mode], reverse=(k == 1)) for k in range(2)]
        ref = {"y": torch.cat([o[0]["y"], o[1]["y"]], 2), "dx": o[0]["dx"] + o[1]["dx"]}
        for k in range(2):
            for n in ("h_n", "c_n", "dh0", "dc0", "dw_ih", "dw_hh", "db_ih", "db_hh"):
                ref[f"{n}{k}"] = o[k][n]
        _REF[key] = ref
    return d, _REF[key]


@gpu
@pytest.mark.parametrize("B,T,I", [(7, 31, 40), (17, 12, 256), (40, 76, 64)])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_matrix_modes_match_restated_reference(B, T, I, mode, lstm_rows):
    """Each matrix mode against the float64 restatement that rounds what the device rounds (lstm_restated): both halves of y,
    h_n, c_n, dh0, dc0 of both directions, dx and all eight parameter gradients.  Measured errors are printed (-rP)."""
    d, ref = _bidir_ref(B, T, I, mode)
    got = _bidir(d, B, T, I, mode)
    _check(f"B{B}-T{T}-I{I}/rows{lstm_rows}", mode, got, ref)


@gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_split_dw_deferred_equals_immediate(mode):
    """B*T = 5120: the split-K weight-gradient products under ww_ctx_set_deferred_reduce keep dW_hh / dW_ih partials apart and
    queue one 1024-column bias item per direction (db_ih | db_hh adjacent, nn.LSTM's order): 6 items, one flush.  The flush sums
    the same partials in double where the immediate kernels sum in float, so deferred == immediate to round-off (<= 2e-6, the
    GRU's and the linear layers' bound), and the deferred gradients meet the restated reference."""
    from wakeword_trainer_home_amd import _native as nat
    B, T, I = 64, 80, 64
    d, ref = _bidir_ref(B, T, I, mode)
    now = _bidir(d, B, T, I, mode)
    sizes = [4 * H * I, 4 * H * H, 4 * H, 4 * H]
    bucket = torch.full((2 * sum(sizes),), float("nan"), device=DEV)
    outs, o = [], 0
    for _ in range(2):
        slots = []
        for s, shape in zip(sizes, ((4 * H, I), (4 * H, H), (4 * H,), (4 * H,))):
            slots.append(bucket[o:o + s].view(shape))
            o += s
        outs.append(tuple(slots))
    lib, cx = nat.load(), nat.ctx(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    later = _bidir(d, B, T, I, mode, outs=outs, defer=True)
    assert lib.ww_deferred_reduce_pending(cx) == 6
    nat.deferred_flush(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(bucket).any()
    worst = 0.0
    for k in range(2):
        for n in ("dw_ih", "dw_hh", "db_ih", "db_hh"):
            e = _rel(later[f"{n}{k}"].double(), now[f"{n}{k}"].double())
            worst = max(worst, e)
            assert e <= 2e-6, (n, k, e)
    print(f"restated-lstm deferred-vs-immediate {mode}: {worst:.2e}")
    _check("split-deferred", mode, {k: v for k, v in later.items() if k.startswith(("dw", "db"))},
           {k: v for k, v in ref.items() if k.startswith(("dw", "db"))})


# ------------------------------------------------------------------------------------------ GPU: the model
@gpu
@pytest.mark.parametrize("prefix,kw", [("", {}), ("uni.", dict(num_layers=1, bidirectional=False))])
def test_lstmwakeword_matches_reference_fixture(prefix, kw):
    """tests/golden/g8_lstm.npz was produced by the reference's own LSTMWakeword: eval logits <= 2e-5, training loss <= 1e-5,
    every parameter gradient <= 5e-4 relative at the fixture's sampled entries and, whole, against the float64 LSTMOracle
    (pinned to the same fixture on the CPU); (B,1,F,T) feature batches give the same logits as (B,T,F)."""
    from wakeword_trainer_home_amd.models import LSTMWakeword
    sd, g = _case(_golden(), prefix)
    model = LSTMWakeword(dropout=0.0, **kw)
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
    oracle = LSTMOracle(model.num_layers, model.bidirectional, dropout=0.0)
    oracle.load_reference_state_dict(sd)
    torch.nn.functional.cross_entropy(oracle(torch.from_numpy(g["x"]), training=True), torch.from_numpy(g["y"])).backward()
    go = oracle.reference_grads()
    for n, p in model.named_parameters():
        assert _sampled_rel(p.grad, g, n) <= 5e-4, n
        assert _rel(p.grad.cpu().double(), go[n]) <= 5e-4, n
    with torch.no_grad():
        model.eval()
        ev4 = model(x.transpose(1, 2)[:, None].contiguous())
    assert torch.equal(ev4, ev)


@gpu
@pytest.mark.parametrize("layers,bidir", [(2, True), (1, True), (2, False)])
def test_lstmwakeword_with_dropout_matches_restatement(layers, bidir):
    from wakeword_trainer_home_amd.models import LSTMWakeword
    torch.manual_seed(layers * 5 + int(bidir))
    model = LSTMWakeword(num_layers=layers, bidirectional=bidir, dropout=0.3, dropout_seed=21).to(DEV)
    oracle = LSTMOracle(layers, bidir, dropout=0.3, seed=21)
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
        assert abs(loss.item() - lo.item()) <= 2e-5, step
        assert (out.detach().cpu().double() - ref.detach()).abs().max().item() <= 5e-5, step
        assert _rel(xd.grad.cpu().double(), xo.grad) <= 5e-4
        for k in range(layers):
            for sfx in ("", "_reverse")[:2 if bidir else 1]:
                for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    gd = getattr(model.lstm, f"{name}_l{k}{sfx}").grad.cpu().double()
                    go = getattr(oracle.layers[k], f"{name}_l0{sfx}").grad
                    assert _rel(gd, go) <= 5e-4, (step, name, k, sfx)
        assert _rel(model.fc[1].weight.grad.cpu().double(), oracle.fc.weight.grad) <= 5e-4


# ------------------------------------------------------------------------------------------ GPU: the Trainer
def _trainer_cfg(batch_size=8, epochs=1):
    from wakeword_trainer_home_amd.config import get_preset
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = epochs, 0, batch_size
    cfg.loss.label_smoothing = 0.0
    return cfg


@gpu
def test_trainer_drives_lstmwakeword(tmp_path):
    """train_epoch / validate_epoch on waveform batches (native front end -> LSTMWakeword -> native loss, the sync-free step
    with the fused clip + optimizer); the first-step loss equals the CPU pipeline's (oracle.train_step.frontend -> the float64
    LSTM) within 1e-3."""
    from wakeword_trainer_home_amd.models import LSTMWakeword
    from wakeword_trainer_home_amd.training import Trainer
    from wakeword_trainer_home_amd.training.optimizer_factory import FlatFusedOptimizer
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from oracle.train_step import frontend
    cfg = _trainer_cfg()
    torch.manual_seed(9)
    model = LSTMWakeword(dropout=0.0)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    wave, y = make_synthetic_batch(24, 24000, seed=5)
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
    oracle = LSTMOracle(dropout=0.0)
    oracle.load_reference_state_dict(sd)
    ref = torch.nn.functional.cross_entropy(oracle(torch.as_tensor(x0), training=True), batches[0][1]).item()
    assert abs(losses[0] - ref) < 1e-3, (losses[0], ref)
    loss, m = t.validate_epoch(0)
    assert m.total_samples == 8 and np.isfinite(loss)


@gpu
def test_graph_replays_equal_eager_steps_bit_for_bit(tmp_path):
    """hip_graph=True: the captured step (forward, loss, backward with deferred partial sums, gather, fused clip + optimizer)
    replayed over two epochs of 4 full batches and a ragged one (8, 8, 8, 8, 5 rows) equals the eager steps bit for bit: loss
    trace, every parameter and the optimizer moments."""
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.models import LSTMWakeword
    from wakeword_trainer_home_amd.training import Trainer
    wave, y = make_synthetic_batch(37, 24000, seed=6)
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
        model = LSTMWakeword(dropout=0.3, dropout_seed=2)
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
    from wakeword_trainer_home_amd.models import LSTMWakeword
    from wakeword_trainer_home_amd.training import Trainer
    cfg = _trainer_cfg()
    torch.manual_seed(2)
    model = LSTMWakeword(dropout=0.0)
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
    t.train_epoch(0)
    after = {k: v.clone() for k, v in model.state_dict().items()}
    assert [i for i, _ in seen] == [0, 2] and all(np.isfinite(l) for _, l in seen)
    assert any(not torch.equal(snaps[0][k], snaps[1][k]) for k in snaps[0])
    assert all(torch.equal(snaps[1][k], snaps[2][k]) for k in snaps[1])
    assert any(not torch.equal(snaps[2][k], after[k]) for k in after)


# ------------------------------------------------------------------------------------------ GPU: argument checks
@gpu
def test_argument_checks_return_error_codes():
    """Wrong I, a short or misaligned workspace and H != 128 come back as errors from the C-ABI's error code, before any launch
    (the bindings raise WW_E_INVALID as ValueError and the other codes as NativeError, as for every entry point)."""
    from wakeword_trainer_home_amd import _native as nat
    import ctypes as C
    lib, cx = nat.load(), nat.ctx(DEV)
    assert lib.ww_lstm_workspace_bytes(4, 5, 8, 64) == 0
    with pytest.raises(nat.NativeError, match="128 only"):
        nat.lstm_workspace(4, 5, 8, 64, DEV)
    B, T, I = 4, 5, 8
    ws = nat.lstm_workspace(B, T, I, H, DEV)
    x = torch.zeros(B, T, I, device=DEV)
    w_ih, w_hh, b = torch.zeros(4 * H, I, device=DEV), torch.zeros(4 * H, H, device=DEV), torch.zeros(4 * H, device=DEV)
    y = torch.zeros(B, T, H, device=DEV)
    with pytest.raises(ValueError):                                        # wrong I at the binding
        nat.lstm_fwd(torch.zeros(B, T, I + 4, device=DEV), w_ih, w_hh, b, b, y, ws)
    with pytest.raises(nat.NativeError, match="workspace too small"):
        nat.lstm_fwd(x, w_ih, w_hh, b, b, y, ws[:100])
    with pytest.raises(ValueError, match="256-byte aligned"):                # WW_E_INVALID
        nat.lstm_fwd(x, w_ih, w_hh, b, b, y, torch.zeros(ws.numel() + 64, device=DEV)[1:1 + ws.numel()])
    p = lambda t: C.c_void_p(t.data_ptr())
    args = lambda h, i, wsb: (cx, 0, p(x), I, p(w_ih), p(w_hh), p(b), p(b), None, None, B, T, i, h, 0, p(y), H, None, None,
                              p(ws), wsb, None)
    assert lib.ww_lstm_fwd(*args(64, I, ws.numel() * 4)) == -4                  # WW_E_UNSUPPORTED: H != 128
    assert lib.ww_lstm_fwd(*args(H, 0, ws.numel() * 4)) == -1                   # bad I
    assert lib.ww_lstm_fwd(*args(H, I, 1024)) == -3                             # WW_E_WORKSPACE
    bigger = nat.lstm_workspace(B, T, 4 * I, H, DEV)
    assert lib.ww_lstm_fwd(cx, 0, p(x), I, p(w_ih), p(w_hh), p(b), p(b), None, None, B, T, 4 * I, H, 0, p(y), H, None, None,
                           p(bigger), bigger.numel() * 4, None) == -1          # ldx (8) smaller than I (32)
    assert lib.ww_lstm_bwd(cx, 0, p(x), I, p(w_ih), p(w_hh), None, H, None, None, B, T, I, H, 0, p(ws), ws.numel() * 4, None, I,
                           0, p(w_ih), p(w_hh), p(b), p(b), None, None, None) == -1   # no dy / dh_n / dc_n
    torch.cuda.synchronize()
