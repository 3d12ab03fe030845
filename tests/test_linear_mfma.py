"""MFMA dense layers / the MobileNetV3 classifier head against torch's own Linear / Hardswish on the
CPU (float64), with the build's Philox dropout mask applied explicitly (oracle/mlp_head.py).
fp32 mode: relative error <= 2e-6 of the tensor's scale (fp32 MFMA accumulation order vs float64).
bf16 / fp16 modes: compared with the oracle's restatement of that mode (operands rounded to the matrix type, exact products,
wide sums): <= 2e-5 (bf16), <= 4e-6 (fp16, measured 4.5e-7); and against the float64 result within 3 roundings (2**-8 bf16, 2**-11 fp16) of the accumulated magnitude."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


_MT = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}


def _rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


@pytest.mark.parametrize("M,K,N", [(2048, 576, 1024), (77, 576, 1024), (130, 40, 2), (1, 7, 3), (64, 64, 64), (200, 1024, 2),
                                   (4096, 64, 1024), (8192, 24, 20), (8192, 200, 64), (300, 30, 300)])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_linear_fwd_bwd_matches_torch(M, K, N, mode):
    """Each mode against its restatement (operands rounded to the matrix type, wide sums).  The launch_gemm / pair choice each
    shape reaches in the 16-bit modes is data now: tests/gemm_cases.py LEGACY_CLAIMS, asserted through ww_gemm_plan by
    test_gemm_paths_host.py::test_what_the_older_linear_test_reaches (per launch path and bit for bit: test_gemm_paths_gpu.py)."""
    from wakeword_trainer_home_amd import _native as nat
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    dy = torch.randn(M, N, generator=g)
    md = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[mode]
    y = nat.linear_mfma_fwd(x.to(DEV), w.to(DEV), b.to(DEV), mode=md)
    dx, dw, db = nat.linear_mfma_bwd(x.to(DEV), w.to(DEV), None, dy.to(DEV), mode=md)
    r = (lambda t: t.to(md).double())
    y_ref = r(x) @ r(w).t() + b.double()
    dx_ref = r(dy) @ r(w)
    dw_ref = r(dy).t() @ r(x)
    db_ref = dy.double().sum(0)
    tol = {"fp32": 2e-6, "bf16": 2e-5, "fp16": 4e-6}[mode]       # fp16 measured: y 2.8e-7, dx 4.5e-7, dW 3.7e-7, db 3.7e-8
    print(f"linear {mode} {M}x{K}x{N}: y={_rel(y.cpu().double(), y_ref):.2e} dx={_rel(dx.cpu().double(), dx_ref):.2e} "
          f"dw={_rel(dw.cpu().double(), dw_ref):.2e} db={_rel(db.cpu().double(), db_ref):.2e}")
    assert _rel(y.cpu().double(), y_ref) <= tol
    assert _rel(dx.cpu().double(), dx_ref) <= tol
    assert _rel(dw.cpu().double(), dw_ref) <= tol
    assert _rel(db.cpu().double(), db_ref) <= (4e-7 if mode == "fp16" else 2e-6)
    if mode != "fp32":      # and the mode itself stays within three roundings (2^-8 bf16, 2^-11 fp16) of the exact product
        y64 = x.double() @ w.double().t() + b.double()
        assert _rel(y.cpu().double(), y64) <= 3 * 2.0 ** (-8 if mode == "bf16" else -11)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("B", [2048, 37])
def test_mobilenetv3_head_matches_oracle(B, mode):
    from wakeword_trainer_home_amd.models.heads import MobileNetV3Head
    from oracle.mlp_head import MLPHeadOracle
    torch.manual_seed(B)
    head = MobileNetV3Head(576, 1024, 2, dropout=0.3, mode=mode, dropout_seed=5).to(DEV)
    assert list(head.state_dict().keys()) == ["0.weight", "0.bias", "3.weight", "3.bias"]      # the reference's classifier keys
    oracle = MLPHeadOracle(576, 1024, 2, dropout=0.3, seed=5)
    oracle.classifier.load_state_dict({k: v.cpu().double() for k, v in head.state_dict().items()})
    x = torch.randn(B, 576)
    y = torch.randint(0, 2, (B,))
    head.train()
    head[0].sample_offset = 11
    for step in range(2):                                   # the dropout stream advances per training forward
        xd = x.to(DEV).requires_grad_(True)
        out = head(xd)
        loss = torch.nn.functional.cross_entropy(out, y.to(DEV))
        head.zero_grad()
        loss.backward()
        xo = x.double().requires_grad_(True)
        ref = oracle(xo, step=step, sample_offset=11, training=True, mtype=_MT[mode])
        lo = torch.nn.functional.cross_entropy(ref, y)
        oracle.zero_grad()
        lo.backward()
        # bf16: h is re-rounded on the device from fp32, in the oracle from float64.  fp16 measured: out 7.1e-5, loss 9.7e-8,
        # parameter gradients 3.6e-3, dx 4.7e-3, eval out 2.5e-5 -> bounds 7e-4 (out, loss), 2.5e-4 (eval), the shared 2e-2
        tol = {"fp32": 5e-6, "bf16": 2e-3, "fp16": 7e-4}[mode]
        print(f"head {mode} B={B} step {step}: out={_rel(out.detach().cpu().double(), ref.detach()):.2e} loss={abs(loss.item() - lo.item()):.2e} "
              f"grads={max(_rel(p.grad.cpu().double(), q.grad) for p, q in zip(head.parameters(), oracle.classifier.parameters())):.2e} "
              f"dx={_rel(xd.grad.cpu().double(), xo.grad):.2e}")
        assert _rel(out.detach().cpu().double(), ref.detach()) <= tol
        assert abs(loss.item() - lo.item()) <= tol
        for (n, p), q in zip(head.named_parameters(), oracle.classifier.parameters()):
            assert _rel(p.grad.cpu().double(), q.grad) <= (2e-5 if mode == "fp32" else 2e-2), (step, n)
        assert _rel(xd.grad.cpu().double(), xo.grad) <= (2e-5 if mode == "fp32" else 2e-2)
    head.eval()                                             # eval: no dropout
    with torch.no_grad():
        ev = head(x.to(DEV))
    eerr = _rel(ev.cpu().double(), oracle(x.double(), training=False, mtype=_MT[mode]).detach())
    print(f"head {mode} B={B} eval: {eerr:.2e}")
    assert eerr <= {"fp32": 5e-6, "bf16": 2e-3, "fp16": 2.5e-4}[mode]


_EDGE = np.array([0.0, 3.0, -3.0, np.nextafter(np.float32(3), np.float32(4)), np.nextafter(np.float32(3), np.float32(0)),
                  np.nextafter(np.float32(-3), np.float32(-4)), np.nextafter(np.float32(-3), np.float32(0)),
                  np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny], dtype=np.float32)


@pytest.mark.parametrize("M,K,N", [(96, 40, 72), (1500, 24, 130)])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("act", ["relu", "hardswish", "hardsigmoid"])
def test_linear_epilogue_activation_edges(act, p, mode, M, K, N):
    """linear_mfma_fwd(want_pre=True) / linear_mfma_bwd(pre=...) with a ReLU / Hardswish / Hardsigmoid epilogue, with and without
    dropout, against float64 restated operands.  The first rows of x are zero, so there the pre-activation IS the bias, which
    carries 0, +-3, one fp32 ulp to either side of +-3 and the smallest normal of either sign: torch's conventions at the kinks
    (relu'(0) = 0, hardswish'(-3) = 0 and (3) = 1, hardsigmoid'(+-3) = 0) are pinned exactly there.  The reference's
    activation decisions elsewhere are taken at the device's own fp32 pre-activations, and its dpre is formed in fp32 as
    k_linear_dpre forms it, so that the 16-bit modes round the same values."""
    import torch.nn.functional as Fn
    from oracle.cnn_small import dropout_keep_mask
    from wakeword_trainer_home_amd import _native as nat
    code = {"relu": nat.LIN_RELU, "hardswish": nat.LIN_HARDSWISH, "hardsigmoid": nat.LIN_HARDSIGMOID}[act]
    f64 = {"relu": torch.relu, "hardswish": Fn.hardswish, "hardsigmoid": Fn.hardsigmoid}[act]
    md = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[mode]
    g = torch.Generator().manual_seed(M + N + int(10 * p))
    Z = 4                                                   # zero rows
    x = torch.randn(M, K, generator=g)
    x[:Z] = 0
    w = torch.randn(N, K, generator=g) * (3 / K ** 0.5)
    b = torch.randn(N, generator=g) * 2
    b[:len(_EDGE)] = torch.from_numpy(_EDGE)
    dy = torch.randn(M, N, generator=g)
    seed, step, off = 9, 5, 3
    y, pre = nat.linear_mfma_fwd(x.to(DEV), w.to(DEV), b.to(DEV), act=code, dropout_p=p, seed=seed, step=step, sample_offset=off,
                                 mode=md, want_pre=True)
    dx, dw, db = nat.linear_mfma_bwd(x.to(DEV), w.to(DEV), pre, dy.to(DEV), act=code, dropout_p=p, seed=seed, step=step,
                                     sample_offset=off, mode=md)
    y, pre, dx, dw, db = (t.cpu().double() for t in (y, pre, dx, dw, db))
    r = (lambda t: t.to(md).double()) if mode != "fp32" else (lambda t: t.double())
    pre_ref = r(x) @ r(w).t() + b.double()
    assert torch.equal(pre[:Z], b.double().expand(Z, N))    # zero rows: exactly the bias
    keep = torch.from_numpy(dropout_keep_mask(M, N, p, seed, step, off).astype(np.float64))
    scale = float(np.float32(1.0 / (1.0 - float(np.float32(p))))) if p > 0 else 1.0
    z = pre.clone().requires_grad_(True)                    # the device's fp32 pre-activations, in float64
    h = f64(z) * keep * scale
    (h * dy.double()).sum().backward()
    y_ref = h.detach()
    # dpre as k_linear_dpre forms it in fp32 (dy * scale, then * act'), so that its 16-bit rounding is the device's
    slope = (z.grad / (dy.double() * keep * scale)).where(keep > 0, torch.zeros(()))   # torch's act'(pre)
    if act == "hardswish":                                  # the device's z * fp32(1/3) + 0.5, rounded once
        inner = (pre > -3) & (pre < 3)
        slope = torch.where(inner, (pre * float(np.float32(1 / 3)) + 0.5).float().double(), slope)
    g32 = torch.where(keep > 0, dy * np.float32(scale), torch.zeros(())) if p > 0 else dy.clone()
    dpre = (g32 * slope.float()).double()
    dx_ref, dw_ref, db_ref = r(dpre) @ r(w), r(dpre).t() @ r(x), dpre.sum(0)
    tol = {"fp32": 2e-6, "bf16": 2e-5, "fp16": 4e-6}[mode]
    errs = {"pre": _rel(pre, pre_ref), "y": _rel(y, y_ref), "y_edge": _rel(y[:Z], y_ref[:Z]), "dx": _rel(dx, dx_ref),
            "dx_edge": _rel(dx[:Z], dx_ref[:Z]), "dw": _rel(dw, dw_ref), "db": _rel(db, db_ref)}
    print(f"linear {act} p={p} {mode} {M}x{K}x{N}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v <= tol}
    assert not bad, bad
    # the planted columns' derivative in the REFERENCE is torch's convention at the kinks, which it relies on (the device's own
    # derivative there is pinned through dx_edge and db above: the zero rows' dpre is all they are made of)
    kink = slope[:Z, :len(_EDGE)]
    want = {"relu": [0, 1, 0, 1, 1, 0, 0, 1, 0], "hardswish": [0.5, 1, 0, 1, 1.5, 0, -0.5, 0.5, 0.5],
            "hardsigmoid": [1 / 6, 0, 0, 0, 1 / 6, 0, 1 / 6, 1 / 6, 1 / 6]}[act]
    for j, v in enumerate(want):
        kept = keep[:Z, j] > 0
        assert torch.allclose(kink[kept, j], torch.full_like(kink[kept, j], float(v)), rtol=1e-6, atol=1e-6), (act, _EDGE[j])


def test_linear_argument_checks():
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.models.heads import MFMALinear
    x = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError):
        nat.linear_mfma_fwd(x, torch.zeros(3, 9, device=DEV))
    with pytest.raises(ValueError):
        nat.linear_mfma_fwd(x, torch.zeros(3, 8, device=DEV), dropout_p=1.0)
    with pytest.raises(ValueError):
        nat.linear_mfma_fwd(x, torch.zeros(3, 8, device=DEV), act=9)
    with pytest.raises(ValueError):
        nat.linear_mfma_bwd(x, torch.zeros(3, 8, device=DEV), None, torch.zeros(4, 3, device=DEV), act=nat.LIN_HARDSWISH)
    with pytest.raises(ValueError):
        MFMALinear(8, 3, activation="relu")
    with pytest.raises(nat.NativeError):
        MFMALinear(8, 3)(torch.zeros(4, 8))


def test_deferred_partial_sums_equal_the_immediate_ones():
    """ww_ctx_set_deferred_reduce: the weight-gradient calls queue their "sum the partials" step and ONE ww_deferred_reduce_flush
    launch runs all of them -- several items of different sizes / split counts in one batch, against the float64 products and
    against the immediate (per-call) sums of the same partials.  Shapes: a split-K dW (M = 30720 rows, 60 splits), a small one
    (no split: nothing is queued), a depthwise 5x5 weight gradient and the stem's."""
    from wakeword_trainer_home_amd import _native as nat
    g = torch.Generator().manual_seed(3)
    lib, cx = nat.load(), nat.ctx(DEV)
    jobs = []
    for M, K, N in ((30720, 96, 576), (7680, 576, 96), (40, 16, 8)):
        x, w, dy = torch.randn(M, K, generator=g).to(DEV), (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV), torch.randn(M, N, generator=g).to(DEV)
        jobs.append(("pw", x, w, dy))
    xdw, wdw = torch.randn(32, 5, 19, 96, generator=g).to(DEV), torch.randn(96, 1, 5, 5, generator=g).to(DEV)
    dydw = torch.randn(32, 5, 19, 96, generator=g).to(DEV)
    xs, dys = torch.randn(16, 40, 151, generator=g).to(DEV), torch.randn(16, 20, 76, 16, generator=g).to(DEV)
    now = [nat.linear_mfma_bwd(x, w, None, dy, mode=torch.bfloat16, need_db=False)[1] for _, x, w, dy in jobs]
    now.append(nat.dwconv_nhwc_bwd(xdw, wdw, dydw, 5, 1)[1])
    now.append(nat.stem3x3s2_bwd_dw(xs, dys, (16, 1, 3, 3)))
    assert lib.ww_deferred_reduce_pending(cx) == 0
    later = [nat.linear_mfma_bwd(x, w, None, dy, mode=torch.bfloat16, need_db=False, defer=True)[1] for _, x, w, dy in jobs]
    later.append(nat.dwconv_nhwc_bwd(xdw, wdw, dydw, 5, 1, defer=True)[1])
    later.append(nat.stem3x3s2_bwd_dw(xs, dys, (16, 1, 3, 3), defer=True))
    assert lib.ww_deferred_reduce_pending(cx) == 4                      # the (40,16,8) product has no split to defer
    nat.deferred_flush(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    torch.cuda.synchronize()
    for a, b in zip(now, later):
        # same partials; the flush sums them in double, the immediate kernels in float / two-level double: round-off apart
        assert _rel(b.double(), a.double()) <= 2e-6
    r = lambda t: t.cpu().bfloat16().double()
    for (_, x, w, dy), dw in zip(jobs, later):
        assert _rel(dw.cpu().double(), r(dy).t() @ r(x)) <= 2e-5
    ref = torch.nn.functional.conv2d(xdw.cpu().double().permute(0, 3, 1, 2).reshape(1, 32 * 96, 5, 19),
                                     dydw.cpu().double().permute(0, 3, 1, 2).reshape(32 * 96, 1, 5, 19), padding=2, groups=32 * 96)
    assert _rel(later[3].cpu().double().reshape(96, 5, 5), ref.reshape(32, 96, 5, 5).sum(0)) <= 2e-5
