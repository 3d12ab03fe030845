"""GPU: the CRNN's conv front-end (ww_cnn_front_fwd / ww_cnn_front_bwd: the cnn_small conv stack, k_freqpool_fwd and
k_freqpool_bwd) called directly, with a random dseq and no GRU, against the restated conv stack (oracle/conv_stack.py) in
fp32, bf16 and fp16 storage.

Every one of the 27 gradient tensors, seq and the 18 running statistics is compared per tensor (error = max |got - ref| /
max |ref|).  The BatchNorm affine parameters are random: at gamma 1 / beta 0 the dgamma of the stem and of the pointwise
BatchNorms is structurally ~1e-6 of the rest and a wrong one would go unseen, so each test also asserts that no reference
tensor is negligible.  The ReLU decisions handed to the restatement are the device's own, from a layer-by-layer chain of
the conv entry points (tests/test_hip_kernels.py:_device_conv_chain), whose running statistics must equal the model's bit
for bit.  fp16 runs at GradScaler's 65536 loss scale, as config 5."""
import numpy as np
import pytest
import torch

from oracle.conv_stack import NL, PARAM_NAMES, cnn_params, conv_stack_restated, grad_names, widx
from tests.test_hip_kernels import DEV, _device_conv_chain, cu

pytestmark = pytest.mark.gpu

ACTS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
LOSS_SCALE = {"fp32": 1.0, "bf16": 1.0, "fp16": 65536.0}
# Per-tensor bounds.  fp32: cnn_small's 1e-4 (tests/test_hip_kernels.py).  16-bit: 9x the error measured on the MI355X for that
# tensor, the largest over the shapes of its test (tests/golden/conv_stack_16bit_errors.json; every test prints a MEASURED
# line).  They differ by three orders of magnitude between tensors, so one bound for all would be blind where it matters:
# a rounding flip of a 16-bit value (2^-9 or 2^-12 relative) moves the BatchNorm-backward sums of these small batches a
# great deal -- a 3e-7 perturbation of every value before its rounding moves the stem's dgamma by 2e-2 in bf16 -- while the
# last layer's dbeta is a sum of exactly the rounded values the restatement has and agrees to fp32 round-off.
FP32_BOUND = 1e-4
BOUND_FACTOR = 9.0
_MEASURED = {}


def bound(kind, act, name):
    if act == "fp32":
        return FP32_BOUND
    if not _MEASURED:
        import json
        from pathlib import Path
        _MEASURED.update(json.loads((Path(__file__).parent / "golden" / "conv_stack_16bit_errors.json").read_text()))
    return BOUND_FACTOR * _MEASURED[kind][act][name]


NEGLIGIBLE = 1e-3     # no reference gradient tensor may be smaller than this fraction of the median tensor
E_INVALID, E_WORKSPACE = -1, -3      # WW_E_INVALID, WW_E_WORKSPACE (include/wwhip.h)


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wakeword_trainer_home_amd import _native
    _native.load()
    return _native


def front_model(seed, mom=0.1, eps=1e-5):
    """float64 CNNSmallOracle (dropout 0) with random BatchNorm affine parameters and running statistics."""
    from oracle.cnn_small import CNNSmallOracle
    torch.manual_seed(seed)
    model = CNNSmallOracle(dropout=0.0).double()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.momentum, m.eps = mom, eps
    return model


def run_front(nat, params, x, act, dseq=None, training=True, mom=0.1, eps=1e-5, grads=None):
    """ww_cnn_front_fwd (+ ww_cnn_front_bwd with dseq) on device copies of the 45 tensors; the pointer tables have 47
    entries, 45 and 46 null.  -> seq, params (running statistics updated), grads."""
    P = [cu(p) for p in params[:45]]
    G = [torch.zeros_like(p) for p in P] if grads is None else grads
    xg = x.float().to(DEV).contiguous()
    B, F, T = x.shape[0], x.shape[2], x.shape[3]
    code = nat.act_code(ACTS[act])
    ws = torch.empty(nat.cnn_small_workspace_bytes(B, F, T, code) // 4, dtype=torch.float32, device=DEV)
    seq = torch.empty(B, (T + 1) // 2, 64, dtype=torch.float32, device=DEV)
    pa, ga = nat.ptr_array(P + [None, None]), nat.ptr_array(G + [None, None])
    nat.cnn_front_fwd(pa, xg, ws, seq, training=training, bn_momentum=mom, bn_eps=eps, act=code)
    if dseq is not None:
        nat.cnn_front_bwd(pa, ga, xg, dseq.float().to(DEV).contiguous(), ws, act=code)
    torch.cuda.synchronize()
    return seq.cpu().double(), P, G


def rel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def freqpool_of(y8, ss8):
    """seq restated from a device y8 (NHWC) / ss8: mean over H of relu(fma(y, scale, shift)) in float64."""
    y, s = y8.cpu().double(), ss8.cpu().double()
    return torch.relu(y * s[:64] + s[64:]).mean(dim=1)


def check_front(nat, act, B, F, T, seed=0, mom=0.1, eps=1e-5, scale=None):
    model = front_model(seed, mom, eps)
    params = cnn_params(model)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, 1, F, T, generator=gen, dtype=torch.float64) * 2 - 4
    Wo = (T + 1) // 2
    S = LOSS_SCALE[act] if scale is None else scale
    dseq = torch.randn(B, Wo, 64, generator=gen, dtype=torch.float64) / (B * Wo) * S
    chain = _device_conv_chain(nat, model, x, act=ACTS[act], momentum=mom, eps=eps)
    seq, P, G = run_front(nat, params, x, act, dseq, mom=mom, eps=eps)
    # the chain ran the same kernels on the same inputs: same running statistics, bit for bit
    for l in range(NL):
        assert torch.equal(P[widx(l) + 3], chain["running_mean"][l]), (l, "running_mean")
        assert torch.equal(P[widx(l) + 4], chain["running_var"][l]), (l, "running_var")
    # seq is the frequency pooling of the chain's last layer within the fp32 rounding of an H-term sum
    H = (F + 1) // 2
    ref_pool = freqpool_of(chain["y"][8], chain["ss"][8])
    assert ((seq - ref_pool).abs() <= (H + 2) * 2.0 ** -24 * ref_pool + 1e-30).all()
    o = conv_stack_restated(params, x, mtype=None if act == "fp32" else ACTS[act], momentum=mom, eps=eps,
                            masks=chain["mask"], head="freq", dout=dseq)
    errs = {"seq": rel(seq, o["seq"])}
    for n in grad_names("freq"):
        errs[n] = rel(G[PARAM_NAMES.index(n)].cpu() / S, o["grads"][n] / S)
    for l in range(NL):
        errs[PARAM_NAMES[widx(l) + 3]] = rel(P[widx(l) + 3], o["running_mean"][l])
        errs[PARAM_NAMES[widx(l) + 4]] = rel(P[widx(l) + 4], o["running_var"][l])
    _report_and_check("front", f"cnn_front {act} B={B} F={F} T={T} mom={mom} eps={eps}", errs, o["grads"], act)
    assert all(torch.isfinite(g).all() for g in G)
    return o


def check_cnn_small(nat, act, B, F, T, p, seed=0):
    """cnn_small (GAP -> dropout -> classifier head) in ``act`` storage against the same restatement with the device's ReLU
    decisions: logits, the 29 gradients and the 18 running statistics per tensor (tests/test_bf16_mode.py, test_fp16_mode.py)."""
    from oracle.cnn_small import CNNSmallOracle, dropout_keep_mask
    torch.manual_seed(seed)
    model = CNNSmallOracle(dropout=p, dropout_seed=77).double()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    params = cnn_params(model)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, 1, F, T, generator=gen, dtype=torch.float64) * 2 - 4
    S = LOSS_SCALE[act]
    dlog = torch.randn(B, 2, generator=gen, dtype=torch.float64) / B * S
    step = 4
    keep = dropout_keep_mask(B, 64, p, 77, step) if p > 0 else None
    chain = _device_conv_chain(nat, model, x, act=ACTS[act])
    P = [cu(t) for t in params]
    G = [torch.zeros_like(t) for t in P]
    xg = x.float().to(DEV).contiguous()
    code = nat.act_code(ACTS[act])
    ws = torch.empty(nat.cnn_small_workspace_bytes(B, F, T, code) // 4, dtype=torch.float32, device=DEV)
    logits = torch.empty(B, 2, dtype=torch.float32, device=DEV)
    pa, ga = nat.ptr_array(P), nat.ptr_array(G)
    nat.cnn_small_fwd(pa, xg, ws, logits, training=True, dropout_p=p, seed=77, step=step, act=code)
    nat.cnn_small_bwd(pa, ga, xg, dlog.float().to(DEV).contiguous(), ws, dropout_p=p, seed=77, step=step, act=code)
    torch.cuda.synchronize()
    for l in range(NL):
        assert torch.equal(P[widx(l) + 3], chain["running_mean"][l]) and torch.equal(P[widx(l) + 4], chain["running_var"][l]), l
    o = conv_stack_restated(params, x, mtype=None if act == "fp32" else ACTS[act], masks=chain["mask"], head="gap", dout=dlog,
                            keep=keep, dropout_p=p)
    errs = {"logits": rel(logits.cpu(), o["logits"])}
    for n in grad_names("gap"):
        errs[n] = rel(G[PARAM_NAMES.index(n)].cpu() / S, o["grads"][n] / S)
    for l in range(NL):
        errs[PARAM_NAMES[widx(l) + 3]] = rel(P[widx(l) + 3], o["running_mean"][l])
        errs[PARAM_NAMES[widx(l) + 4]] = rel(P[widx(l) + 4], o["running_var"][l])
    _report_and_check("cnn_small", f"cnn_small {act} B={B} F={F} T={T} p={p}", errs, o["grads"], act)
    assert all(torch.isfinite(g).all() for g in G)


def _report_and_check(kind, tag, errs, ref_grads, act):
    import json
    print(f"\nMEASURED {json.dumps({'kind': kind, 'act': act, 'tag': tag, 'errs': errs})}")
    worst = max(errs, key=errs.get)
    print(f"{tag}: worst {worst} {errs[worst]:.2e}")
    bad = {n: (e, bound(kind, act, n)) for n, e in errs.items() if not e <= bound(kind, act, n)}
    assert not bad, f"{tag}: over the bound (error, bound): {bad}"
    if ref_grads:
        mags = {n: g.abs().max().item() for n, g in ref_grads.items()}
        med = float(np.median(list(mags.values())))
        small = {n: m / med for n, m in mags.items() if m < NEGLIGIBLE * med}
        assert not small, f"{tag}: negligible reference tensors: {small}"


# shapes: the preset (40 mels x 1.51 s) and the default config (128 mels x 2.5 s); odd F and T; the smallest input (a 1 x 1
# map); B * ceil(T/2) = 19456 > 16384, past k_freqpool_fwd's grid cap (2048 blocks x 8 items) and k_freqpool_bwd's
# partial-row cap (1024 x 8)
SHAPES = [(4, 40, 151), (2, 128, 251), (3, 13, 49), (16, 1, 1), (256, 2, 151)]


@pytest.mark.parametrize("act", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("B,F,T", SHAPES)
def test_front_matches_restatement(nat, act, B, F, T):
    # a 1 x 1 map: 16 values per BatchNorm channel give rstd up to ~300 and g_l up to ~12 per unit of dseq, which overflows fp16
    # at 65536 (the restatement says so); GradScaler would back off, to 1024 here
    scale = 1024.0 if act == "fp16" and F * T == 1 else None
    check_front(nat, act, B, F, T, seed=B + F + T, scale=scale)


@pytest.mark.parametrize("act", ["fp32", "bf16", "fp16"])
def test_front_takes_the_callers_momentum_and_eps(nat, act):
    """bn_momentum / bn_eps reach every layer: running statistics, seq and gradients follow a non-default pair."""
    check_front(nat, act, 3, 24, 37, seed=5, mom=0.3, eps=1e-2)


@pytest.mark.parametrize("act", ["fp32", "bf16", "fp16"])
def test_front_eval_mode(nat, act):
    """training=0: scale / shift from the running statistics, which stay untouched, and seq from them."""
    model = front_model(9, mom=0.2, eps=1e-3)
    params = cnn_params(model)
    x = torch.randn(3, 1, 20, 31, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2 - 4
    chain = _device_conv_chain(nat, model, x, act=ACTS[act], momentum=0.2, eps=1e-3, training=False)
    seq, P, _ = run_front(nat, params, x, act, training=False, mom=0.2, eps=1e-3)
    for i in range(45):
        assert torch.equal(P[i].cpu(), params[i].float()), PARAM_NAMES[i]
    ref_pool = freqpool_of(chain["y"][8], chain["ss"][8])
    assert ((seq - ref_pool).abs() <= 12 * 2.0 ** -24 * ref_pool + 1e-30).all()
    o = conv_stack_restated(params, x, mtype=None if act == "fp32" else ACTS[act], eps=1e-3, training=False,
                            masks=chain["mask"], head="freq")
    _report_and_check("front_eval", f"cnn_front eval {act}", {"seq": rel(seq, o["seq"])}, {}, act)


@pytest.mark.parametrize("act", ["fp32", "bf16"])
def test_crnn_accumulates_front_gradients(act):
    """CRNNWakeword's accumulate path: a second forward + backward without zeroing the gradients gives exactly twice the
    first gradients (the front-end's ww_cnn_front_bwd writes into a temporary that is added to .grad)."""
    from wakeword_trainer_home_amd.models.recurrent import CRNNWakeword
    torch.manual_seed(4)
    model = CRNNWakeword(dropout=0.0, act_dtype=act).to(DEV).train()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    gen = torch.Generator().manual_seed(8)
    x = (torch.randn(3, 1, 40, 51, generator=gen) * 2 - 4).to(DEV)
    w = torch.randn(3, 2, generator=gen).to(DEV)
    (model(x) * w).sum().backward()
    first = {n: p.grad.clone() for n, p in model.named_parameters()}
    assert all(p.grad is not None for p in model.parameters())
    (model(x) * w).sum().backward()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert torch.equal(p.grad, 2 * first[n]), n
    assert any(first[n].abs().max().item() > 0 for n in first if n.startswith("front.stem.bn"))


def test_front_argument_checks(nat):
    """Null seq, dseq, or a conv layer's gradient buffer, a workspace too small or not 256-byte aligned: an error code and no
    launch (seq, gradients, running statistics and workspace untouched).  Entries 45 / 46 may be null."""
    lib = nat.load()
    model = front_model(1)
    params = cnn_params(model)
    B, F, T = 2, 10, 12
    x = torch.randn(B, 1, F, T, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    P = [cu(p) for p in params[:45]]
    G = [torch.full_like(p, 7.0) for p in P]
    xg = x.float().to(DEV).contiguous()
    code = nat.ACT_F32
    need = nat.cnn_small_workspace_bytes(B, F, T, code)
    ws = torch.full((need // 4 + 64,), 3.0, dtype=torch.float32, device=DEV)
    seq = torch.full((B, (T + 1) // 2, 64), 5.0, dtype=torch.float32, device=DEV)
    dseq = torch.ones_like(seq)
    stream = nat._stream(torch.device(DEV))
    ctx = nat.ctx(torch.device(DEV))
    snap = lambda: [t.clone() for t in [seq, ws] + P + G]

    def fwd(pa, wsp, wsb, seqp):
        return lib.ww_cnn_front_fwd(ctx, code, pa, xg.data_ptr(), B, F, T, 1, 0.1, 1e-5, wsp, wsb, seqp, stream)

    def bwd(pa, ga, wsp, wsb, dseqp):
        return lib.ww_cnn_front_bwd(ctx, code, pa, ga, xg.data_ptr(), dseqp, B, F, T, wsp, wsb, stream)

    pa = nat.ptr_array(P + [None, None])
    ga = nat.ptr_array(G + [None, None])
    before = snap()
    cases = [
        ("fwd seq null", fwd(pa, ws.data_ptr(), need, None), E_INVALID),
        ("fwd workspace small", fwd(pa, ws.data_ptr(), need - 4, seq.data_ptr()), E_WORKSPACE),
        ("fwd workspace unaligned", fwd(pa, ws.data_ptr() + 4, need, seq.data_ptr()), E_INVALID),
        ("bwd dseq null", bwd(pa, ga, ws.data_ptr(), need, None), E_INVALID),
        ("bwd grads null", bwd(pa, None, ws.data_ptr(), need, dseq.data_ptr()), E_INVALID),
        ("bwd workspace small", bwd(pa, ga, ws.data_ptr(), need - 256, dseq.data_ptr()), E_WORKSPACE),
        ("bwd workspace unaligned", bwd(pa, ga, ws.data_ptr() + 128, need, dseq.data_ptr()), E_INVALID),
    ]
    for i in range(45):
        if PARAM_NAMES[i].endswith(("running_mean", "running_var")):
            continue
        gi = nat.ptr_array([None if j == i else g for j, g in enumerate(G)] + [None, None])
        cases.append((f"bwd grads[{i}] null", bwd(pa, gi, ws.data_ptr(), need, dseq.data_ptr()), E_INVALID))
    for i in (0, 3, 44):
        pi = nat.ptr_array([None if j == i else p for j, p in enumerate(P)] + [None, None])
        cases.append((f"fwd params[{i}] null", fwd(pi, ws.data_ptr(), need, seq.data_ptr()), E_INVALID))
        cases.append((f"bwd params[{i}] null", bwd(pi, ga, ws.data_ptr(), need, dseq.data_ptr()), E_INVALID))
    torch.cuda.synchronize()
    bad = [(what, rc, want) for what, rc, want in cases if rc != want]
    assert not bad, bad
    assert all(torch.equal(a, b) for a, b in zip(before, snap())), "a rejected call wrote something"
    # the same tables with valid arguments do run (45 / 46 null in both)
    assert fwd(pa, ws.data_ptr(), need, seq.data_ptr()) == 0
    assert bwd(pa, ga, ws.data_ptr(), need, dseq.data_ptr()) == 0
    torch.cuda.synchronize()
    assert not torch.equal(seq, before[0]) and not torch.equal(G[0], before[2 + 45])
