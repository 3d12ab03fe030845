"""GPU: the support kernels whose grid is capped on the host, run past one pass of that grid, and ww_dropout_bt on its own.

Every shape lives in tests/grid_pass_cases.py; that each one makes a second (ragged) pass is asserted on the CPU through the
library's own plan queries (tests/test_grid_passes_host.py).  Every comparison is bit for bit against a plain NumPy / float64
restatement, except the 16-bit input projection of the GRU, which is held to the bounds of
test_gru.py::test_gru_direction_matches_restated_reference (the measured errors are printed, -rP)."""
import types

import numpy as np
import pytest
import torch

from tests import data_pipeline_cases as D
from tests import grid_pass_cases as K
from tests.evaluation_cases import host_windows
from tests.test_data_pipeline_gpu import _bank_case, _run_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _first_bad(got, ref):
    bad = np.argwhere(np.where(np.isnan(ref), ~np.isnan(got), K.bits(got) != K.bits(ref)))
    return f"{len(bad)} differ, first at {bad[0].tolist() if len(bad) else None}"


# ------------------------------------------------------------------------------------------ loader gather
@pytest.mark.parametrize("B,training", K.LOADER_RUNS)
def test_loader_gather_over_two_and_three_trips(B, training):
    """k_loader_batch with S = 2 of 3 passes (B = 1100: workgroup 0 of a row makes two trips, workgroup 1 one) and S = 1 of 3
    (B = 2048: three trips), rows alternating between 16-byte and 2-byte alignment, odd and even crop offsets."""
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.data import DeviceClipBank
    c = K.LOADER
    assert nat.plan_loader(B, c["n_out"])["trips"] == K.LOADER_TRIPS[B]
    bank, lengths, labels = _bank_case(c["n_out"], c["L"], c["n_clips"])
    dev_bank = DeviceClipBank(torch.from_numpy(bank), torch.from_numpy(labels), torch.from_numpy(lengths), device=DEV)
    cdf = D.cdf_table(D.zero_run_weights(c["n_clips"], seed=3))
    cdf_dev = torch.from_numpy(cdf).to(DEV)
    for epoch in c["epochs"]:
        ref_w, ref_t, ref_i, off = D.batch(bank, lengths, labels, c["n_out"], "weighted", c["seed"], epoch, c["rank"], c["world"],
                                           c["k0"], B, cdf=cdf, training=training)
        got_w, got_t, got_i = _run_batch(dev_bank, "weighted", c["seed"], epoch, c["rank"], c["world"], c["k0"], B, c["n_out"],
                                         training, cdf_dev=cdf_dev)
        assert np.array_equal(got_i, ref_i) and np.array_equal(got_t, ref_t)
        bad = np.argwhere(got_w != ref_w)
        assert bad.size == 0, f"first mismatch (row, sample) {bad[0]} of {len(bad)}; clip {ref_i[bad[0][0]]} off {off[bad[0][0]]}"
        if training:
            assert (off % 2 == 1).any() and ((off > 0) & (off % 2 == 0)).any()
        else:
            assert not off.any()


@pytest.mark.parametrize("rel", ["equal", "above"])
def test_loader_bank_two_bytes_past_a_16_byte_boundary(rel):
    """The bank is a contiguous view that starts 2 bytes past a 16-byte boundary and ends where its last clip ends: the source
    shift of clip 0 is that of no aligned bank, its aligned window starts in front of the bank, and the last clip's last window
    would end behind it.  B = 9, every clip once, in order."""
    n_out, n = 250, 9
    L = n_out if rel == "equal" else n_out + 37
    bank, lengths, labels = _bank_case(n_out, L, 12)
    bank, lengths, labels = bank[:n].copy(), lengths[:n].copy(), labels[:n].copy()
    lengths[0] = lengths[n - 1] = L                          # the first and the last clip are full
    buf = torch.full((n * L + 1 + 8,), 31000, dtype=torch.int16, device=DEV)
    view = buf[1:1 + n * L].view(n, L)
    view.copy_(torch.from_numpy(bank))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 2 and view.is_contiguous()
    dev_bank = types.SimpleNamespace(wave=view, lengths=torch.from_numpy(lengths).to(torch.int32).to(DEV),
                                     labels=torch.from_numpy(labels).to(DEV))
    for training in (False, True):
        for epoch in (0, 3):
            ref_w, ref_t, ref_i, off = D.batch(bank, lengths, labels, n_out, "none", 5, epoch, 0, 1, 0, n, shuffle=False, training=training)
            got_w, got_t, got_i = _run_batch(dev_bank, "none", 5, epoch, 0, 1, 0, n, n_out, training, shuffle=False)
            assert np.array_equal(got_i, np.arange(n)) and np.array_equal(got_i, ref_i) and np.array_equal(got_t, ref_t)
            bad = np.argwhere(got_w != ref_w)
            assert bad.size == 0, f"first mismatch (row, sample) {bad[0]} of {len(bad)}; off {off[bad[0][0]]}"
            assert np.array_equal(got_w[n - 1, -8:], bank[n - 1, off[n - 1] + n_out - 8:off[n - 1] + n_out])


# ------------------------------------------------------------------------------------------ wave windows
@pytest.mark.parametrize("chunk,order", list(zip(K.WINDOW_CHUNKS, ("zero_tiny", "tiny_zero"))))
def test_wave_windows_second_trip(chunk, order):
    """W = 4099: workgroups 0 .. 2 take a second window each, with another peak than their first one (larger and smaller), and
    those second windows are the all-zero, the 1e-30 and the NaN window; every window equals NumPy's float32 x / peak."""
    from wakeword_trainer_home_amd import _native as nat
    assert nat.plan_passes("wave_windows", K.WINDOW_W)["passes"] == 2
    wave = K.window_recording(chunk, order)
    out, peaks = nat.wave_windows(_dev(wave), chunk)
    with np.errstate(invalid="ignore"):
        ref_out, ref_peaks = host_windows(wave, chunk)
    out, peaks = out.cpu().numpy(), peaks.cpu().numpy()
    assert out.shape == (K.WINDOW_W, chunk) and peaks.shape == (K.WINDOW_W,)
    assert np.array_equal(peaks, ref_peaks, equal_nan=True), np.flatnonzero(~((peaks == ref_peaks) | np.isnan(ref_peaks)))[:8]
    rows = np.flatnonzero((K.bits(out) != K.bits(ref_out)).any(axis=1))
    assert rows.size == 0, f"windows {rows[:8]} of {rows.size} differ"


# ------------------------------------------------------------------------------------------ add + ReLU, ReLU mask
@pytest.mark.parametrize("n", K.EW_TINY + (K.EW_N,))
def test_add_relu_and_relu_mask_conventions(n):
    """y = where(a + b < 0, 0, a + b): NaN stays NaN, -0 stays -0; dx = where(y != 0, dy, 0): a zero of either sign stops the
    gradient, a NaN in y passes it.  +0, -0, NaN, +-inf and subnormals in the first 256 elements and in the second pass."""
    from wakeword_trainer_home_amd import _native as nat
    a, b = K.ew_inputs(n)
    y = nat.add_relu_fwd(_dev(a), _dev(b)).cpu().numpy()
    ref = K.add_relu_ref(a, b)
    assert K.same_floats(y, ref), _first_bad(y, ref)
    dy, ys = K.ew_inputs(n, seed=1)
    dx = nat.relu_mask_bwd(_dev(dy), _dev(ys)).cpu().numpy()
    ref = K.relu_mask_ref(dy, ys)
    assert K.same_floats(dx, ref), _first_bad(dx, ref)
    # and on the forward's own output
    dx = nat.relu_mask_bwd(_dev(dy), _dev(y)).cpu().numpy()
    ref = K.relu_mask_ref(dy, y)
    assert K.same_floats(dx, ref), _first_bad(dx, ref)


# ------------------------------------------------------------------------------------------ fp32 max-pool
def test_maxpool_fp32_past_one_pass():
    """(4, 260, 260, 64): 1 081 600 output quads (2 passes forward), 4 326 400 input quads (5 passes backward); integer data in
    [0, 2] (most windows tie), integer gradients: exact, the first maximum takes the gradient."""
    from wakeword_trainer_home_amd import _native as nat
    from tests.resnet_cases import maxpool_bwd, maxpool_fwd
    shape = K.POOL_SHAPE
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randint(0, 3, shape, generator=g).float()
    ry, idx = maxpool_fwd(x)
    dy = torch.randint(-4, 5, tuple(ry.shape), generator=g).float()
    y = nat.maxpool3x3s2_fwd(x.to(DEV))
    dx = nat.maxpool3x3s2_bwd(x.to(DEV), dy.to(DEV))
    assert y.dtype is torch.float32 and torch.equal(y.cpu(), ry)
    assert torch.equal(dx.cpu(), maxpool_bwd(idx, dy, shape[1], shape[2]))


# ------------------------------------------------------------------------------------------ TCN dpre
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_tconv_dpre_past_one_pass(mode):
    """ww_tconv1d_bwd at (4, 4100, 4, 256, 1, 1): k_tconv_dpre over 1 049 600 float4s, 16 rows into its second pass, with two
    saved outputs and a scale of 2.  Integer data, sums below 2^24: dx, dw and db equal the float64 restatement."""
    from wakeword_trainer_home_amd import _native as nat
    from tests.tcn_cases import conv_bwd, layer_inputs
    B, T, Cin, Cout, k, d = K.DPRE_SHAPE
    d_in = layer_inputs(B, T, Cin, Cout, k, seed=sum(K.DPRE_SHAPE), integer=True)
    g = torch.Generator().manual_seed(3)
    y1 = torch.randint(-1, 2, (B, T, Cout), generator=g).double()
    y2 = torch.randint(0, 2, (B, T, Cout), generator=g).double()
    f = lambda t: t.float().to(DEV)
    md = {"fp32": torch.float32, "bf16": torch.bfloat16}[mode]
    dx, dw, db = nat.tconv1d_bwd(f(d_in["x"]), f(d_in["w"]), f(d_in["dy"]), d, y=f(y1), y2=f(y2), mask_scale=K.DPRE_SCALE, mode=md)
    rx, rw, rb = conv_bwd(d_in["x"], d_in["w"], d_in["dy"] * K.DPRE_SCALE * (y1 != 0) * (y2 != 0), d)
    assert rw.abs().max() < 2 ** 24 and rb.abs().max() < 2 ** 24 and rx.abs().max() < 2 ** 24
    assert rx[-1, -16:].abs().sum() > 0                      # the rows of the second pass carry gradient
    assert torch.equal(db.cpu().double(), rb)
    assert torch.equal(dx.cpu().double(), rx), f"dx rows {torch.nonzero((dx.cpu().double() != rx).any(2))[:4].tolist()}"
    assert torch.equal(dw.cpu().double(), rw)


# ------------------------------------------------------------------------------------------ 16-bit input projection of the GRU
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_gru_projection_copies_past_one_pass(mode):
    """ww_gru_fwd at (1040, 64, 256) in a 16-bit mode: k_to16_pair converts 4 284 416 float4s, the last 1024 rows of x and all
    of W_ih in its second trip.  Batch rows are independent: y and h_n of samples 0, 1023, 1024 and 1039 against gru_restated
    run on those four samples, inside the bounds test_gru_direction_matches_restated_reference holds the mode to."""
    from oracle.gru import gru_restated
    from tests.test_gru import _GRU_BOUND, _MT, _gru_inputs
    from wakeword_trainer_home_amd import _native as nat
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < 2 * 2 ** 30:
        pytest.skip("less than 2 GB of device memory free")
    B, T, I = K.PROJ_SHAPE
    H = 128
    assert nat.plan_passes("to16_pair", (B * T * I + 3 * H * I) // 4)["passes"] == 2
    P, x, h0, _, _ = _gru_inputs(B, T, I, 77, 1)
    P, h0 = P[0], h0[0]
    sel = list(K.PROJ_SAMPLES)
    ref = gru_restated(x[sel], *P, h0=h0[sel], mtype=_MT[mode])
    f = lambda t: t.float().to(DEV)
    md = {"bf16": torch.bfloat16, "fp16": torch.float16}[mode]
    ws = nat.gru_workspace(B, T, I, H, DEV)
    y = torch.full((B, T, H), 7.0, device=DEV)
    h_n = nat.gru_fwd(f(x), *[f(p) for p in P], y, ws, h0=f(h0), mode=md)
    torch.cuda.synchronize()
    bound = _GRU_BOUND[mode][0]
    e_y = (y[sel].cpu().double() - ref["y"]).abs().amax((1, 2))
    e_h = (h_n[sel].cpu().double() - ref["h_n"]).abs().amax(1)
    print(f"gru projection {mode} (B, T, I) = {(B, T, I)}, samples {sel}: max |y - ref| = {[f'{v:.2e}' for v in e_y.tolist()]}, "
          f"max |h_n - ref| = {[f'{v:.2e}' for v in e_h.tolist()]}; bound {bound:.0e}")
    assert torch.isfinite(y).all()
    assert e_y.max().item() <= bound and e_h.max().item() <= bound, (mode, e_y.tolist(), e_h.tolist())
    del ws, y
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ ww_dropout_bt
def _dropout(nat, x, case, **kw):
    return nat.dropout_bt(x, case["p"], seed=case["seed"], step=case["step"], sample_offset=case["sample_offset"],
                          stream_id=case["stream_id"], **kw)


def _dropout_case(nat, name, case, keep=None):
    x = K.dropout_case_x(case["shape"], seed=len(name))
    keep = K.dropout_keep(case) if keep is None else keep
    ref = K.dropout_ref(x, keep, case["p"])
    xd = _dev(x)
    got = _dropout(nat, xd, case).cpu().numpy()
    assert K.same_floats(got, ref), (name, _first_bad(got, ref))
    neg0, nan = np.signbit(x) & (x == 0), np.isnan(x)
    assert np.signbit(got[neg0 & keep]).all() and np.isnan(got[nan & keep]).all()          # a kept -0 / NaN stays
    assert np.array_equal(K.bits(got[~keep]), np.zeros(int((~keep).sum()), np.int32))       # dropped: +0, a NaN too
    # its own backward: the same arguments draw the same mask
    dy = np.random.default_rng(1).standard_normal(case["shape"]).astype(F32)
    gd = _dropout(nat, _dev(dy), case).cpu().numpy()
    assert np.array_equal(K.bits(gd), K.bits(K.dropout_ref(dy, keep, case["p"]))), name
    return x, xd, got, keep


@pytest.mark.parametrize("name", list(K.DROP_SMALL))
def test_dropout_bt_small_cases(name):
    """Partial last quads (C = 1 .. 5), seed and step beyond 2^32, a sample offset whose low word wraps inside the batch and one
    beyond 2^40, p = 0 (a bit copy) and p = 0.999: out = where(keep, x * scale, +0) bit for bit, keep = oracle.gru.dropout_bt_mask."""
    from wakeword_trainer_home_amd import _native as nat
    case = K.DROP_SMALL[name]
    x, xd, got, keep = _dropout_case(nat, name, case)
    if name == "p0":
        assert keep.all() and K.same_floats(got, x)
    if name == "p999":
        assert 0 < keep.sum() < keep.size // 100
    if name == "offset_wraps":                               # rows 3 .. 5 are samples 0 .. 2 of the stream
        low = dict(case, shape=(3,) + case["shape"][1:], sample_offset=0)
        assert K.same_floats(_dropout(nat, xd[3:].contiguous(), low).cpu().numpy(), got[3:])


@pytest.mark.parametrize("name,case", [("big", K.DROP_BIG), ("ragged", K.DROP_RAGGED)])
def test_dropout_bt_past_one_pass(name, case):
    """(2, 4096, 1024) with stream 15: t, c >> 2 and the stream id at the limits of their counter fields, two full passes;
    (33, 1000, 127): 1 056 000 quads, every row ending in a partial one."""
    from wakeword_trainer_home_amd import _native as nat
    B, T, C = case["shape"]
    assert nat.plan_passes("dropout_bt", B * T * ((C + 3) // 4))["passes"] == 2
    _dropout_case(nat, name, case, keep=K.dropout_keep_cached(name, case))


def test_dropout_bt_strided_rows_leave_the_rest_untouched():
    from wakeword_trainer_home_amd import _native as nat
    case = K.DROP_STRIDED
    B, T, C = case["shape"]
    x = K.dropout_case_x(case["shape"], seed=4)
    wide = torch.full((B, T, case["ld_x"]), float("nan"), device=DEV)             # columns outside the slice must not be read
    xs = wide[:, :, case["col_x"]:case["col_x"] + C]
    xs.copy_(_dev(x))
    sentinel = -12345.0
    obuf = torch.full((B, T, case["ld_out"]), sentinel, device=DEV)
    out = obuf[:, :, case["col_out"]:case["col_out"] + C]
    assert xs.stride(1) == case["ld_x"] and out.stride(1) == case["ld_out"] and xs.data_ptr() % 16 and out.data_ptr() % 16
    res = _dropout(nat, xs, case, out=out)
    assert res is out
    keep = K.dropout_keep(case)
    ref = K.dropout_ref(x, keep, case["p"])
    got = obuf.cpu().numpy()
    assert K.same_floats(got[:, :, case["col_out"]:case["col_out"] + C], ref)
    assert (got[:, :, :case["col_out"]] == sentinel).all() and (got[:, :, case["col_out"] + C:] == sentinel).all()
    assert keep.any() and not keep.all()
    # strided in, contiguous out gives the same
    assert K.same_floats(_dropout(nat, xs, case).cpu().numpy(), ref)


def test_dropout_bt_argument_checks():
    from wakeword_trainer_home_amd import _native as nat
    z = lambda *s: torch.zeros(*s, device=DEV)
    for shape, kw in (((1, 4097, 4), {}), ((1, 2, 1025), {}), ((1, 2, 4), dict(stream_id=16)), ((1, 2, 4), dict(stream_id=-1))):
        with pytest.raises(nat.NativeError, match="T <= 4096, C <= 1024, stream_id < 16"):
            nat.dropout_bt(z(*shape), 0.3, **kw)
    for p in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="not in"):
            nat.dropout_bt(z(1, 2, 4), p)
    base = z(64)
    for narrow in ("x", "out"):                              # a row stride of 3 below C = 4: overlapping rows
        rows = base.as_strided((2, 3, 4), (9, 3, 1))
        with pytest.raises(ValueError, match="bad shape"):
            if narrow == "x":
                nat.dropout_bt(rows, 0.3)
            else:
                nat.dropout_bt(z(2, 3, 4), 0.3, out=rows)
    assert not base.any()
    # the limits themselves are accepted
    assert nat.dropout_bt(z(1, 4096, 4), 0.3, stream_id=15).shape == (1, 4096, 4) and nat.dropout_bt(z(1, 2, 1024), 0.0).shape == (1, 2, 1024)
