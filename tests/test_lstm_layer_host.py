"""What tests/test_lstm_layer_gpu.py rests on, checked on the CPU: the restated direction equals float64 torch.nn.LSTM in every call
form of the case tables; the restated model equals LSTMOracle (autograd over nn.LSTM) loss and gradient; the identities of the
layer's index maps hold exactly on the restatement; every case falls in the remainder / alignment class it is there for; and the
+-1-ulp movement of each restated reference is the one recorded beside the cases (tests/lstm_cases.py)."""
import pytest
import torch

from tests import lstm_cases as K
from tests.lstm_cases import H, lstm_restated


def _torch_lstm(c, d, k=0, nd=1):
    """float64 autograd over nn.LSTM of direction k of a case -> the tensors of dir_reference."""
    B, T, I = c["B"], c["T"], c["I"]
    reverse = c["reverse"] if nd == 1 else k == 1
    ref = torch.nn.LSTM(I, H, batch_first=True).double()
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    with torch.no_grad():
        for n, p in zip(names, d["P"][k]):
            getattr(ref, n).copy_(p)
    P = [getattr(ref, n) for n in names]
    x = d["x"].clone().requires_grad_(True)
    z = lambda t: (torch.zeros(B, H, dtype=torch.float64) if t is None else t.clone()).requires_grad_(True)
    h0, c0 = z(d["h0"][k]), z(d["c0"][k])
    out, (hn, cn) = ref(x.flip(1) if reverse else x, (h0[None], c0[None]))
    out = out.flip(1) if reverse else out
    loss = 0.0
    if d["dy"] is not None:
        loss = loss + (out * d["dy"][:, :, k * H:(k + 1) * H]).sum()
    if d["dhn"][k] is not None:
        loss = loss + (hn[0] * d["dhn"][k]).sum()
    if d["dcn"][k] is not None:
        loss = loss + (cn[0] * d["dcn"][k]).sum()
    loss.backward()
    return dict(y=out.detach(), h_n=hn[0].detach(), c_n=cn[0].detach(), dx=x.grad, dw_ih=P[0].grad, dw_hh=P[1].grad, db_ih=P[2].grad,
                db_hh=P[3].grad, dh0=h0.grad, dc0=c0.grad)


@pytest.mark.parametrize("name", list(K.DIR_CASES))
def test_restated_direction_is_torch_lstm_in_every_call_form(name):
    """mtype None: lstm_restated == float64 nn.LSTM to 1e-12, every tensor the call form returns (dy = None, dc_n only, one state
    missing, no states included)."""
    c, d, ref = K.cached_reference("dir", name, "fp32")
    want = _torch_lstm(c, d)
    for k, r in ref.items():
        assert (r - want[k]).abs().max().item() <= 1e-12, (name, k)


@pytest.mark.parametrize("name", list(K.BIDIR_CASES))
def test_restated_pair_is_torch_lstm_in_every_call_form(name):
    c, d, ref = K.cached_reference("bidir", name, "fp32")
    w = [_torch_lstm(c, d, k, 2) for k in range(2)]
    assert (ref["y"] - torch.cat([w[0]["y"], w[1]["y"]], 2)).abs().max().item() <= 1e-12
    assert (ref["dx"] - (w[0]["dx"] + w[1]["dx"])).abs().max().item() <= 1e-12
    for k in range(2):
        for n in ("h_n", "c_n", *K.GRAD_KEYS) + (("dh0", "dc0") if c.get("ds0", True) else ()):
            assert (ref[f"{n}{k}"] - w[k][n]).abs().max().item() <= 1e-12, (name, n, k)


@pytest.mark.parametrize("table,nd", [(K.DIR_CASES, 1), (K.BIDIR_CASES, 2)], ids=["dir", "bidir"])
def test_every_case_falls_in_the_class_it_names(table, nd):
    """B % 8, B % 16, T & 1 of every case, ldx % 4 of the strided x, the byte offset and row stride of the y / dy views, lddx - I
    of the dx view are what the case's `hits` says -- and the classes the tables are there for are all present."""
    for name, c in table.items():
        assert K.case_hits(c, nd) == c["hits"], name
    if nd == 1:
        hit = {n: c["hits"] for n, c in table.items()}
        assert hit["b8"]["B8"] == 0 and hit["b8"]["B16"] == 8                   # one 8-row group full, half a 16-row group
        assert hit["b16"]["B8"] == 0 and hit["b16"]["B16"] == 0                 # both forms exactly full
        assert hit["b17"]["B8"] == 1 and hit["b17"]["B16"] == 1                 # one past full in both
        assert hit["b25"]["B8"] == 1 and hit["b25"]["B16"] == 9                 # ragged: the 16-row form's last group > 8 rows
        assert (table["t1_b1"]["T"], table["t2"]["T"], table["t3"]["T"]) == (1, 2, 3)
        assert {hit[n]["Tpar"] for n in ("t1_b1", "t2", "t3")} == {0, 1}        # hs[T & 1] at both parities
        assert hit["x_ld67"]["ldx4"] != 0                                       # vecA = vecB = 0
        assert hit["y_off1"]["ybytes16"] != 0 and hit["y_off1"]["ldy4"] == 0    # y_vec = 0 from the pointer alone
        assert hit["dx_view_acc"]["lddx_over"] > 0
        assert {c["reverse"] for c in table.values()} == {False, True}
    else:
        assert table["y_off1"]["hits"]["ybytes16"] != 0 and table["y_off1"]["hits"]["ldy4"] == 0
    for c in table.values():                                                     # every call keeps a way for the gradient in
        assert c.get("dy", True) or c.get("dhn", True) or c.get("dcn", True)


# ------------------------------------------------------------------------------------------ identities, exact in float64
ID = dict(B=13, T=7, I=40, roll=5, t0=3)


def _id_run(d, reverse, **over):
    a = dict(x=d["x"], h0=d["h0"][0], c0=d["c0"][0], dy=d["dy"], dh_n=d["dhn"][0], dc_n=d["dcn"][0])
    a.update(over)
    return lstm_restated(a.pop("x"), *d["P"][0], reverse=reverse, **a)


@pytest.mark.parametrize("reverse", [False, True])
def test_rows_identity_on_the_restatement(reverse):
    """Rolling the batch rolls every per-row result exactly (each row is computed from its own row alone); the batch-summed
    gradients agree to 1e-12."""
    d = K._inputs(ID["B"], ID["T"], ID["I"], 5, 1)
    r = lambda t: t.roll(ID["roll"], 0)
    plain = _id_run(d, reverse)
    rolled = _id_run(d, reverse, x=r(d["x"]), h0=r(d["h0"][0]), c0=r(d["c0"][0]), dy=r(d["dy"]), dh_n=r(d["dhn"][0]),
                     dc_n=r(d["dcn"][0]))
    for k in ("y", "h_n", "c_n", "dx", "dh0", "dc0"):
        assert torch.equal(rolled[k].roll(-ID["roll"], 0), plain[k]), k
    for k in K.GRAD_KEYS:
        assert K._rel(rolled[k], plain[k]) <= 1e-12, k


def test_time_identity_on_the_restatement():
    """reverse=True on x is reverse=False on x flipped in time, with y / dy / dx flipped and the states equal -- exactly."""
    d = K._inputs(ID["B"], ID["T"], ID["I"], 6, 1)
    rev = _id_run(d, True)
    fwd = _id_run(d, False, x=d["x"].flip(1), dy=d["dy"].flip(1))
    for k in ("y", "dx"):
        assert torch.equal(rev[k], fwd[k].flip(1)), k
    for k in ("h_n", "c_n", "dh0", "dc0"):
        assert torch.equal(rev[k], fwd[k]), k
    for k in K.GRAD_KEYS:
        assert K._rel(rev[k], fwd[k]) <= 1e-12, k


@pytest.mark.parametrize("reverse", [False, True])
def test_causality_on_the_restatement(reverse):
    """dy at one step t0 only and no final-state gradients: dx after t0 (in the direction's own time order) is exactly zero and
    every row up to t0 carries a non-zero entry."""
    d = K._inputs(ID["B"], ID["T"], ID["I"], 7, 1)
    t0 = ID["t0"]
    dy = torch.zeros_like(d["dy"])
    dy[:, t0] = d["dy"][:, t0]
    dx = _id_run(d, reverse, dy=dy, dh_n=None, dc_n=None)["dx"]
    late, early = (slice(0, t0), slice(t0, None)) if reverse else (slice(t0 + 1, None), slice(0, t0 + 1))
    assert (dx[:, late] == 0).all()
    assert (dx[:, early] != 0).any(2).all()


def test_chaining_on_the_restatement():
    """T = 7 at once equals T = 4 then T = 3 with the states handed on, backward with the state gradients handed back."""
    d = K._inputs(ID["B"], ID["T"], ID["I"], 8, 1)
    whole = _id_run(d, False)
    a = _id_run(d, False, x=d["x"][:, :4], dy=None, dh_n=None, dc_n=None)
    b = _id_run(d, False, x=d["x"][:, 4:], h0=a["h_n"], c0=a["c_n"], dy=d["dy"][:, 4:])
    a = _id_run(d, False, x=d["x"][:, :4], dy=d["dy"][:, :4], dh_n=b["dh0"], dc_n=b["dc0"])
    assert (torch.cat([a["y"], b["y"]], 1) - whole["y"]).abs().max().item() <= 1e-12
    assert (torch.cat([a["dx"], b["dx"]], 1) - whole["dx"]).abs().max().item() <= 1e-12
    for k in ("dh0", "dc0"):
        assert (a[k] - whole[k]).abs().max().item() <= 1e-12, k
    for k in ("h_n", "c_n"):
        assert (b[k] - whole[k]).abs().max().item() <= 1e-12, k
    for k in K.GRAD_KEYS:
        assert K._rel(a[k] + b[k], whole[k]) <= 1e-12, k


def test_abs_sums_bound_the_gradient_terms():
    """The a-priori bound of the GPU identities is built from abs_sums: the sum of |term| of every element of the batch-summed
    gradients.  It dominates |gradient| elementwise and scales linearly with the inputs' signs removed."""
    d = K._inputs(5, 3, 9, 9, 1)
    o = _id_run(d, False)
    for k in K.GRAD_KEYS:
        assert (o["abs_sums"][k] >= o[k].abs() * (1 - 1e-12)).all(), k
        assert o["abs_sums"][k].shape == o[k].shape


# ------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("layers,bidir", [(2, True), (1, True), (2, False)])
def test_restated_model_is_lstm_oracle(layers, bidir):
    """mtype None: model_restated (hand-written backward) == LSTMOracle (autograd over nn.LSTM with the same Philox masks):
    logits, loss, dx and every parameter gradient to 1e-12, over two dropout steps, and the eval logits."""
    from tests.test_lstm import LSTMOracle
    torch.manual_seed(layers * 3 + int(bidir))
    oracle = LSTMOracle(layers, bidir, dropout=0.3, seed=21)
    sd = {}
    for k, layer in enumerate(oracle.layers):
        for n, p in layer.named_parameters():
            sd["lstm." + n.replace("_l0", f"_l{k}")] = p.detach().clone()
    sd["fc.1.weight"], sd["fc.1.bias"] = oracle.fc.weight.detach().clone(), oracle.fc.bias.detach().clone()
    B, T = 5, 6
    x = torch.randn(B, T, 40, dtype=torch.float64)
    y = torch.randint(0, 2, (B,))
    for step in range(2):
        xo = x.clone().requires_grad_(True)
        logits = oracle(xo, step=step, sample_offset=5, training=True)
        loss = torch.nn.functional.cross_entropy(logits, y)
        oracle.zero_grad()
        loss.backward()
        got = K.model_restated(sd, x, y, layers, bidir, 0.3, 21, step, 5, None, True)
        assert (got["logits"] - logits.detach()).abs().max().item() <= 1e-12
        assert abs(got["loss"].item() - loss.item()) <= 1e-12
        assert (got["dx"] - xo.grad).abs().max().item() <= 1e-12
        want = oracle.reference_grads()
        assert sorted(want) == sorted(got["grads"])
        for n, g in want.items():
            assert (got["grads"][n] - g).abs().max().item() <= 1e-12, (step, n)
    with torch.no_grad():
        ev = oracle(x, training=False)
    assert (K.model_restated(sd, x, None, layers, bidir, 0.3, 21, 0, 5, None, False)["logits"] - ev).abs().max().item() <= 1e-12


def test_model_setup_is_the_gpu_tests_model():
    from wakeword_trainer_home_amd.models import LSTMWakeword
    sd, x, y = K.model_setup()
    m = LSTMWakeword(num_layers=K.MODEL["num_layers"], bidirectional=K.MODEL["bidirectional"], dropout=K.MODEL["dropout"],
                     dropout_seed=K.MODEL["dropout_seed"], mode="bf16")
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert all(v.dtype == torch.float32 for v in sd.values()) and x.dtype == torch.float32
    assert tuple(x.shape) == (K.MODEL["B"], K.MODEL["T"], 40) and 0 < int(y.sum()) < K.MODEL["B"]


# ------------------------------------------------------------------------------------------ the +-1-ulp probes
def _agrees(measured, recorded):
    """A recorded movement stands for the measured one: not below it, and no more than a quarter above."""
    return measured <= recorded <= 1.25 * measured


@pytest.mark.parametrize("kind,table", [("dir", K.DIR_CASES), ("bidir", K.BIDIR_CASES)], ids=["dir", "bidir"])
def test_reference_moves_are_the_recorded_ones(kind, table):
    """Every case and mode: where the restated reference moves by more than the mode's bound when its fp32 inputs move by +-1
    ulp, REF_MOVES holds that movement (and the GPU test holds that tensor to 4x it); everywhere else REF_MOVES has no entry
    and _BOUND stands."""
    seen = set()
    for name in table:
        for mode in K.MODES:
            moves = K.ulp_moves(kind, name, mode)
            rec = K.REF_MOVES.get((kind, name, mode), {})
            over = {k: m for k, m in moves.items() if m > K.bound_of(mode, k)}
            print(f"lstm-ref-moves {kind}-{name} {mode}: " + " ".join(f"{k}={v:.2e}" for k, v in moves.items()))
            assert sorted(over) == sorted(rec), (kind, name, mode, over, rec)
            for k, m in over.items():
                assert _agrees(m, rec[k]), (kind, name, mode, k, m, rec[k])
            seen.add((kind, name, mode))
    assert all(key in seen for key in K.REF_MOVES if key[0] == kind)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_model_reference_moves_are_the_recorded_ones(mode):
    moves = K.model_moves(mode)
    print(f"lstm-model-moves {mode}: " + " ".join(f"{k}={v:.2e}" for k, v in moves.items()))
    assert sorted(moves) == sorted(K.MODEL_MOVES[mode])
    for k, m in moves.items():
        assert _agrees(m, K.MODEL_MOVES[mode][k]), (mode, k, m, K.MODEL_MOVES[mode][k])
