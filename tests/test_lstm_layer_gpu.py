"""The LSTM layer (ww_lstm_fwd / _bwd, ww_lstm_bidir_fwd / _bwd) per call form and matrix mode, its index maps as identities that
need no tolerance, and LSTMWakeword in the 16-bit modes.  Cases, the branch each one reaches, bounds and the restated float64
references are in tests/lstm_cases.py; what these tests rest on is checked on the CPU in tests/test_lstm_layer_host.py.  Every
test runs in both workgroup shapes of the recurrent kernels (WW_LSTM_ROWS = 8, 16).  Measured errors are printed (-s / -rP:
profiles/r15_lstm_paths_measured.txt)."""
import pytest
import torch

from tests import lstm_cases as K
from tests.lstm_cases import H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 7.0


@pytest.fixture(params=[8, 16], autouse=True)
def lstm_rows(request, monkeypatch):
    """Both workgroup shapes of the recurrent kernels (8 or 16 batch rows per workgroup; the library picks by batch size)."""
    monkeypatch.setenv("WW_LSTM_ROWS", str(request.param))
    return request.param


def _f(t):
    return None if t is None else t.float().to(DEV)


class _Workspace:
    """lstm_workspace(...)-sized leading view of a larger buffer whose tail holds a sentinel that must come back untouched."""
    TAIL = 4096

    def __init__(self, nat, B, T, I):
        n = nat.lstm_workspace(B, T, I, H, DEV).numel()
        self.buf = torch.full((n + self.TAIL,), GUARD, device=DEV)
        self.ws = self.buf[:n]
        assert self.ws.data_ptr() % 256 == 0

    def check(self):
        tail = self.buf[self.ws.numel():]
        assert torch.equal(tail, torch.full_like(tail, GUARD)), "the kernels wrote past the workspace"


def _guards_intact(buf, off, width):
    assert torch.equal(buf[:, :, :off], torch.full_like(buf[:, :, :off], GUARD))
    assert torch.equal(buf[:, :, off + width:], torch.full_like(buf[:, :, off + width:], GUARD))


def _y_view(B, T, width, off):
    """-> (buffer of 7.0, the (B,T,width) view `off` floats into rows of width + 4 -- or the whole contiguous buffer)."""
    buf = torch.full((B, T, width + 4 if off else width), GUARD, device=DEV)
    y = buf[:, :, off:off + width]
    assert (y.data_ptr() % 16 != 0) == bool(off)
    return buf, y


def _dy_view(dy, off):
    """dy on the device, as a view `off` floats into rows of NaN (columns outside the view must never be read)."""
    if dy is None:
        return None
    B, T, W = dy.shape
    if not off:
        return _f(dy)
    buf = torch.full((B, T, W + 4), float("nan"), device=DEV)
    v = buf[:, :, off:off + W]
    v.copy_(_f(dy))
    return v


def run_direction(mode, x, P, reverse, h0=None, c0=None, dy=None, dhn=None, dcn=None, ds0=True, want_dx=True, ldx=0, yoff=0,
                  dx_old=None):
    """One ww_lstm_fwd + ww_lstm_bwd on float64 CPU inputs -> {tensor: device tensor} of what the call form returns."""
    from wakeword_trainer_home_amd import _native as nat
    B, T, I = x.shape
    md = K._MD[mode]
    if ldx:
        xd = torch.zeros(B, T, ldx, device=DEV)[:, :, :I]
        xd.copy_(_f(x))
    else:
        xd = _f(x)
    Pd = [_f(p) for p in P]
    ws = _Workspace(nat, B, T, I)
    ybuf, y = _y_view(B, T, H, yoff)
    h_n, c_n = nat.lstm_fwd(xd, *Pd, y, ws.ws, h0=_f(h0), c0=_f(c0), reverse=reverse, mode=md)
    _guards_intact(ybuf, yoff, H)
    got = {"y": y, "h_n": h_n, "c_n": c_n}
    dx = dxbuf = None
    if dx_old is not None:
        dxbuf = torch.full((B, T, I + 4), GUARD, device=DEV)
        dx = dxbuf[:, :, :I]
        dx.copy_(_f(dx_old))
    elif want_dx:
        dx = torch.full((B, T, I), float("nan"), device=DEV)           # written, not accumulated into
    g = nat.lstm_bwd(xd, Pd[0], Pd[1], _dy_view(dy, yoff), _f(dhn), _f(dcn), ws.ws, reverse=reverse, dx=dx,
                     accumulate_dx=dx_old is not None, want_dh0=ds0, mode=md)
    torch.cuda.synchronize()
    ws.check()
    got.update(zip(K.GRAD_KEYS, g[:4]))
    if ds0:
        got["dh0"], got["dc0"] = g[4], g[5]
    else:
        assert g[4] is None and g[5] is None
    if dx_old is not None:
        _guards_intact(dxbuf, 0, I)
        got["dx"] = dx - _f(dx_old)
    elif want_dx:
        got["dx"] = dx
    return got


def run_pair(mode, d, ds0=True, yoff=0):
    """One ww_lstm_bidir_fwd + _bwd on an _inputs dict (entries the call form leaves out are None)."""
    from wakeword_trainer_home_amd import _native as nat
    B, T, I = d["x"].shape
    md = K._MD[mode]
    params = [[_f(p) for p in d["P"][k]] for k in range(2)]
    xd = _f(d["x"])
    ws = [_Workspace(nat, B, T, I) for _ in range(2)]
    ybuf, y = _y_view(B, T, 2 * H, yoff)
    pair = lambda ts: None if ts[0] is None and ts[1] is None else [_f(t) for t in ts]
    h_n, c_n = nat.lstm_bidir_fwd(xd, params, y, [w.ws for w in ws], mode=md, h0=pair(d["h0"]), c0=pair(d["c0"]))
    _guards_intact(ybuf, yoff, 2 * H)
    dx = torch.full((B, T, I), float("nan"), device=DEV)
    dh0 = [torch.empty(B, H, device=DEV) for _ in range(2)] if ds0 else None
    dc0 = [torch.empty(B, H, device=DEV) for _ in range(2)] if ds0 else None
    grads = nat.lstm_bidir_bwd(xd, params, _dy_view(d["dy"], yoff), pair(d["dhn"]) or (None, None), [w.ws for w in ws], dx=dx, mode=md,
                               dh0=dh0, dc_n=pair(d["dcn"]), dc0=dc0)
    torch.cuda.synchronize()
    for w in ws:
        w.check()
    got = {"y": y, "dx": dx}
    for k in range(2):
        got[f"h_n{k}"], got[f"c_n{k}"] = h_n[k], c_n[k]
        if ds0:
            got[f"dh0{k}"], got[f"dc0{k}"] = dh0[k], dc0[k]
        got.update({f"{n}{k}": g for n, g in zip(K.GRAD_KEYS, grads[k])})
    return got


# ------------------------------------------------------------------------------------------ A, A': call forms
@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", list(K.DIR_CASES))
def test_lstm_direction_call_forms_match_restated_reference(name, mode, lstm_rows):
    """ww_lstm_fwd / ww_lstm_bwd in each matrix mode and call form (lstm_cases.DIR_CASES names the branch each case reaches)
    against lstm_restated: y, h_n, c_n, the four parameter gradients, dx and dh0 / dc0 where the form asks for them, within
    _BOUND[mode]; nothing written outside y, dx or the workspace."""
    c, d, _ = K.cached_reference("dir", name, mode)
    got = run_direction(mode, d["x"], d["P"][0], c["reverse"], h0=d["h0"][0], c0=d["c0"][0], dy=d["dy"], dhn=d["dhn"][0],
                        dcn=d["dcn"][0], ds0=c.get("ds0", True), want_dx=c.get("dx", True), ldx=c.get("ldx", 0),
                        yoff=c.get("yoff", 0), dx_old=d.get("dx_old"))
    K.check_case("dir", name, mode, f"rows{lstm_rows}", got)


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", list(K.BIDIR_CASES))
def test_lstm_bidirectional_call_forms_match_restated_reference(name, mode, lstm_rows):
    """ww_lstm_bidir_fwd / _bwd (both directions in one launch) in each matrix mode and call form (lstm_cases.BIDIR_CASES)
    against two restated directions: both halves of y, the summed dx, h_n, c_n and all eight parameter gradients, dh0 / dc0
    where asked for, within _BOUND[mode]."""
    c, d, _ = K.cached_reference("bidir", name, mode)
    got = run_pair(mode, d, ds0=c.get("ds0", True), yoff=c.get("yoff", 0))
    K.check_case("bidir", name, mode, f"rows{lstm_rows}", got)


# ------------------------------------------------------------------------------------------ B: identities
IDB, IDT, IDI, ROLL, T0 = 13, 7, 40, 5, 3
_ID_REF = {}


def _id_inputs(seed):
    d = K._inputs(IDB, IDT, IDI, seed, 1)
    return dict(x=d["x"], P=d["P"][0], h0=d["h0"][0], c0=d["c0"][0], dy=d["dy"], dhn=d["dhn"][0], dcn=d["dcn"][0])


def _id_run(mode, a, reverse, **kw):
    return run_direction(mode, a["x"], a["P"], reverse, h0=a["h0"], c0=a["c0"], dy=a["dy"], dhn=a["dhn"], dcn=a["dcn"], **kw)


def _bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _sum_bound(mode, a, reverse):
    """Per element of the batch-summed gradients: 2 * M * 2^-24 * sum |a||b| over the M = B*T rows, in float64 from the
    absolute values (lstm_restated's abs_sums).  Two device runs add the SAME M products per element in different orders;
    each fp32 sum of M terms is within M * 2^-24 * sum|terms| of the exact sum, so the two are within twice that of each other."""
    key = (mode, id(a["x"]), reverse)
    if key not in _ID_REF:
        o = K.lstm_restated(a["x"], *a["P"], h0=a["h0"], c0=a["c0"], dy=a["dy"], dh_n=a["dhn"], dc_n=a["dcn"], mtype=K._MT[mode],
                            reverse=reverse)
        _ID_REF[key] = {k: 2.0 * IDB * IDT * 2.0 ** -24 * v for k, v in o["abs_sums"].items()}
    return _ID_REF[key]


def _sums_agree(tag, mode, one, two, bound):
    for k in K.GRAD_KEYS:
        diff = (one[k].cpu().double() - two[k].cpu().double()).abs()
        print(f"lstm-paths identity-{tag} {mode} {k}: worst difference / bound = {(diff / bound[k]).max().item():.2e}")
        assert (diff <= bound[k]).all(), (tag, mode, k)


_ROWS_IN = _id_inputs(41)
_TIME_IN = _id_inputs(42)
_CAUSE_IN = _id_inputs(43)
_CHAIN_IN = _id_inputs(44)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("mode", K.MODES)
def test_rolling_the_batch_rolls_the_results_bit_for_bit(mode, reverse, lstm_rows):
    """B = 13 rolled by 5: every (batch row, unit) element of a step is one MFMA chain over the same k order whichever row,
    workgroup or lane holds it (crow0, the permlane32_swap hand-over, erow / ec0), and every row of the projection and dX
    products is independent of its place in the B*T rows -- so y, h_n, c_n, dx, dh0, dc0 of the rolled run, rolled back, are
    the plain run's bits.  The batch-summed gradients add the same terms in another order (_sum_bound)."""
    a = _ROWS_IN
    r = lambda t: t.roll(ROLL, 0)
    plain = _id_run(mode, a, reverse)
    rolled = _id_run(mode, {k: (v if k == "P" else r(v)) for k, v in a.items()}, reverse)
    for k in ("y", "h_n", "c_n", "dx", "dh0", "dc0"):
        assert _bits_equal(rolled[k].roll(-ROLL, 0), plain[k]), (mode, k)
    _sums_agree(f"rows-rev{int(reverse)}/rows{lstm_rows}", mode, plain, rolled, _sum_bound(mode, a, reverse))


@pytest.mark.parametrize("mode", K.MODES)
def test_reverse_is_forward_on_flipped_time_bit_for_bit(mode, lstm_rows):
    """reverse=True on x is reverse=False on x flipped in time (`reverse ? T - 1 - it : it` in load_gi, flush, prefetch and
    step): y and dx flipped, h_n, c_n (hs[T & 1], T odd), dh0, dc0 equal, bit for bit; weight and bias gradients within
    _sum_bound."""
    a = _TIME_IN
    rev = _id_run(mode, a, True)
    fwd = _id_run(mode, dict(a, x=a["x"].flip(1), dy=a["dy"].flip(1)), False)
    for k in ("y", "dx"):
        assert _bits_equal(rev[k], fwd[k].flip(1)), (mode, k)
    for k in ("h_n", "c_n", "dh0", "dc0"):
        assert _bits_equal(rev[k], fwd[k]), (mode, k)
    _sums_agree(f"time/rows{lstm_rows}", mode, rev, fwd, _sum_bound(mode, a, True))


@pytest.mark.parametrize("yoff", [0, 1])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("mode", K.MODES)
def test_a_gradient_at_one_step_reaches_no_later_step(mode, reverse, yoff, lstm_rows):
    """dy non-zero at t0 = 3 only, no dh_n / dc_n: dx after t0 in the direction's own time order (t > t0 forward, t < t0
    reverse) is exactly zero (-0 counts) and every (b, t) row up to t0 has a non-zero entry; with dy_vec 1 (contiguous dy) and
    0 (dy one float into rows of 132)."""
    a = _CAUSE_IN
    dy = torch.zeros_like(a["dy"])
    dy[:, T0] = a["dy"][:, T0]
    dx = _id_run(mode, dict(a, dy=dy, dhn=None, dcn=None), reverse, yoff=yoff)["dx"]
    late, early = (slice(0, T0), slice(T0, None)) if reverse else (slice(T0 + 1, None), slice(0, T0 + 1))
    assert (dx[:, late] == 0).all()
    assert (dx[:, early] != 0).any(2).all()


@pytest.mark.parametrize("mode", K.MODES)
def test_two_chained_calls_equal_one(mode, lstm_rows):
    """T = 7 at once, and as T = 4 then T = 3 with (h_n, c_n) handed on as (h0, c0) and, backwards, the second part's (dh0, dc0)
    as the first part's (dh_n, dc_n).  Both runs are within the mode's bound of the same restated reference (on the CPU the
    chained restatement IS the whole one), so they are within twice the bound of each other: y, h_n, c_n 2 b_fwd; dh0, dc0
    2 b_st; dx 2 b_rel of its largest entry."""
    a = _CHAIN_IN
    whole = _id_run(mode, a, False)
    cut = lambda t, s: t[:, s].contiguous()
    first, second = slice(0, 4), slice(4, IDT)
    from wakeword_trainer_home_amd import _native as nat
    md = K._MD[mode]
    Pd = [_f(p) for p in a["P"]]
    x1, x2 = _f(cut(a["x"], first)), _f(cut(a["x"], second))
    w1, w2 = _Workspace(nat, IDB, 4, IDI), _Workspace(nat, IDB, IDT - 4, IDI)
    y1, y2 = torch.empty(IDB, 4, H, device=DEV), torch.empty(IDB, IDT - 4, H, device=DEV)
    hm, cm = nat.lstm_fwd(x1, *Pd, y1, w1.ws, h0=_f(a["h0"]), c0=_f(a["c0"]), mode=md)
    h_n, c_n = nat.lstm_fwd(x2, *Pd, y2, w2.ws, h0=hm, c0=cm, mode=md)
    dx1, dx2 = torch.empty_like(x1), torch.empty_like(x2)
    g2 = nat.lstm_bwd(x2, Pd[0], Pd[1], _f(cut(a["dy"], second)), _f(a["dhn"]), _f(a["dcn"]), w2.ws, dx=dx2, want_dh0=True, mode=md)
    g1 = nat.lstm_bwd(x1, Pd[0], Pd[1], _f(cut(a["dy"], first)), g2[4], g2[5], w1.ws, dx=dx1, want_dh0=True, mode=md)
    torch.cuda.synchronize()
    w1.check()
    w2.check()
    chained = {"y": torch.cat([y1, y2], 1), "h_n": h_n, "c_n": c_n, "dx": torch.cat([dx1, dx2], 1), "dh0": g1[4], "dc0": g1[5]}
    errs = K.errors(chained, {k: whole[k].cpu().double() for k in chained})
    print(f"lstm-paths identity-chain/rows{lstm_rows} {mode}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, e in errs.items():
        assert e <= 2.0 * K.bound_of(mode, k), (mode, k, e)


# ------------------------------------------------------------------------------------------ C: the model
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_lstmwakeword_16bit_modes_match_restated_model(mode, lstm_rows):
    """LSTMWakeword(mode = bf16 | fp16): the stack, the inter-layer dropout and the MFMALinear head in the matrix mode, two
    training steps (sample_offset 5) and the eval logits against lstm_cases.model_restated.  Per tensor -- logits and loss
    absolute, dx and every parameter gradient relative to its largest entry -- the bound is the larger of the _BOUND[mode] entry
    and 8x the tensor's +-1-ulp movement (lstm_cases.model_bound)."""
    from wakeword_trainer_home_amd.models import LSTMWakeword
    M = K.MODEL
    sd, x, y = K.model_setup()
    model = LSTMWakeword(num_layers=M["num_layers"], bidirectional=M["bidirectional"], dropout=M["dropout"],
                         dropout_seed=M["dropout_seed"], mode=mode)
    model.load_state_dict(sd)
    model.to(DEV)
    assert model.lstm.mode == K._MD[mode] and model.fc[1].mode == K._MD[mode]
    model.train()
    model.sample_offset = M["sample_offset"]
    for step in range(M["steps"]):
        xd = x.to(DEV).requires_grad_(True)
        out = model(xd)
        loss = torch.nn.functional.cross_entropy(out, y.to(DEV))
        model.zero_grad()
        loss.backward()
        got = {"logits": out, "loss": loss, "dx": xd.grad}
        got.update({"grad." + n: p.grad for n, p in model.named_parameters()})
        ref = K.model_reference(mode, step)
        assert sorted(got) == sorted(ref)
        errs = K.model_errors(got, ref)
        for k, v in errs.items():
            print(f"lstm-paths model/rows{lstm_rows} {mode} step {step} {k}: error {v:.2e}, _BOUND {K.model_base_bound(mode, k):.1e}, "
                  f"8 x movement {8.0 * K.MODEL_MOVES[mode][k]:.1e}")
        bad = {k: (e, K.model_bound(mode, k)) for k, e in errs.items() if not e <= K.model_bound(mode, k)}
        assert not bad, (mode, step, bad)
    model.eval()
    with torch.no_grad():
        ev = model(x.to(DEV))
    e = K.model_errors({"logits": ev}, K.model_reference(mode, 0, training=False))["logits"]
    print(f"lstm-paths model/rows{lstm_rows} {mode} eval logits: error {e:.2e}, _BOUND {K.model_base_bound(mode, 'logits_eval'):.1e}, "
          f"8 x movement {8.0 * K.MODEL_MOVES[mode]['logits_eval']:.1e}")
    assert e <= K.model_bound(mode, "logits_eval")
