"""The restated 16-bit references the GPU tests compare the matrix modes with (oracle/gru.py:gru_restated,
oracle/rounding.py:mround, the matrix type of oracle/mlp_head.py), checked on the CPU: without rounding the GRU restatement IS torch.nn.GRU (forward and autograd
backward, float64, to ~1e-12), and its rounding is round-to-nearest-even with overflow to inf, as an independent float64
restatement of RNE says and as torch's own ``.to(dtype)`` does."""
import math

import numpy as np
import pytest
import torch

from oracle.gru import gru_restated
from oracle.rounding import mround

MT = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.mark.parametrize("B,T,I,reverse,with_dy", [(3, 5, 9, False, True), (2, 4, 16, True, True), (4, 1, 7, False, True),
                                                   (3, 6, 5, True, False)])
def test_unrounded_restatement_is_torch_gru(B, T, I, reverse, with_dy):
    H = 128
    torch.manual_seed(B * 100 + T * 10 + I)
    ref = torch.nn.GRU(I, H, num_layers=1, batch_first=True, bidirectional=True).double()
    sfx = "_reverse" if reverse else ""
    P = [getattr(ref, n + "_l0" + sfx) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    x = torch.randn(B, T, I, dtype=torch.float64, requires_grad=True)
    h0 = (torch.randn(2, B, H, dtype=torch.float64) * 0.5).requires_grad_(True)
    out, hn = ref(x, h0)
    d = 1 if reverse else 0
    sl = slice(H, 2 * H) if reverse else slice(0, H)
    dy = torch.randn(B, T, H, dtype=torch.float64) if with_dy else None
    dhn = torch.randn(B, H, dtype=torch.float64)
    loss = (hn[d] * dhn).sum() + ((out[:, :, sl] * dy).sum() if with_dy else 0.0)
    loss.backward()
    o = gru_restated(x, *P, h0=h0[d], dy=dy, dh_n=dhn, mtype=None, reverse=reverse)
    err = lambda a, b: (a - b).abs().max().item()
    assert err(o["y"], out[:, :, sl].detach()) <= 1e-12
    assert err(o["h_n"], hn[d].detach()) <= 1e-12
    assert err(o["dx"], x.grad) <= 1e-12
    assert err(o["dh0"], h0.grad[d]) <= 1e-12
    for k, p in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), P):
        assert err(o[k], p.grad) <= 1e-11, k
    # forward only: the same outputs, no gradients
    f = gru_restated(x, *P, h0=h0[d], mtype=None, reverse=reverse)
    assert torch.equal(f["y"], o["y"]) and "dx" not in f


def _rne(v, mtype):
    """Independent RNE of float64 values to bf16 / fp16: quantum 2^(e - p + 1) with e = max(floor(log2|v|), emin), numpy's
    round-half-even, overflow (|rounded| > max finite) to inf."""
    p, emin, emax = {torch.bfloat16: (8, -126, 127), torch.float16: (11, -14, 15)}[mtype]
    fmax = (2.0 - 2.0 ** (1 - p)) * 2.0 ** emax
    out = np.empty_like(v)
    for i, x in enumerate(v):
        if x == 0.0 or not math.isfinite(x):
            out[i] = x
            continue
        e = max(math.floor(math.log2(abs(x))), emin)
        q = 2.0 ** (e - p + 1)
        r = float(np.round(x / q)) * q
        out[i] = math.copysign(math.inf, x) if abs(r) > fmax else r
    return out


@pytest.mark.parametrize("mt", ["bf16", "fp16"])
def test_restated_rounding_is_rne_and_torchs(mt):
    """Ties (odd and even neighbours), fp16 / bf16 subnormals and their ties, the largest finite values, the first value that
    rounds up to inf and random fp32 data: mround == the independent RNE == torch's ``.to(dtype)``."""
    mtype = MT[mt]
    p, emin, emax = {torch.bfloat16: (8, -126, 127), torch.float16: (11, -14, 15)}[mtype]
    fmax = (2.0 - 2.0 ** (1 - p)) * 2.0 ** emax
    q1, qs = 2.0 ** (1 - p), 2.0 ** (emin - p + 1)        # quantum at 1.0, subnormal quantum
    vals = [1.0 + q1 / 2, 1.0 + 3 * q1 / 2, 1.0 + q1 / 4, 1.0 + 3 * q1 / 4, -(1.0 + q1 / 2), 3.0 + 3 * q1,
            qs / 2, 3 * qs / 2, 5 * qs / 2, qs / 4, 0.75 * qs, -3 * qs / 2, 2.0 ** emin * (1 - q1 / 2),
            fmax, fmax * (1 + q1 / 8), fmax + 2.0 ** (emax - p), -(fmax + 2.0 ** (emax - p)), fmax + 2.0 ** (emax - p) * 0.99,
            0.0, -0.0]
    g = torch.Generator().manual_seed(1)
    rnd = (torch.randn(4000, generator=g) * torch.exp2(torch.randint(-30, 20, (4000,), generator=g).float())).double()
    v = torch.cat([torch.tensor(vals, dtype=torch.float64), rnd])
    v = v.float().double()                                        # the device rounds fp32 values
    a = mround(v, mtype)
    assert torch.equal(a, v.float().to(mtype).double())
    b = torch.from_numpy(_rne(v.numpy(), mtype))
    same = (a == b) | (torch.isnan(a) & torch.isnan(b))
    assert bool(same.all()), v[~same][:8]
    # the edges really are edges: ties went to even, fp16 overflow is inf, subnormals survive
    assert a[0].item() == 1.0 and a[1].item() == 1.0 + 2 * q1
    assert a[6].item() == 0.0 and a[7].item() == 2 * qs and a[8].item() == 2 * qs
    assert a[13].item() == fmax and a[15].item() == math.inf and a[16].item() == -math.inf and a[17].item() == fmax


def test_head_oracle_matrix_type():
    """oracle/mlp_head.py: ``bf16=True`` is ``mtype=torch.bfloat16``; fp16 rounds the operands of both products to fp16."""
    from oracle.mlp_head import MLPHeadOracle
    torch.manual_seed(0)
    o = MLPHeadOracle(24, 32, 3, dropout=0.0)
    x = torch.randn(5, 24, dtype=torch.float64)
    a = o(x, training=False, bf16=True)
    assert torch.equal(a, o(x, training=False, mtype=torch.bfloat16))
    l0, l3 = o.classifier[0], o.classifier[3]
    r = lambda t: t.float().half().double()
    ref = r(torch.nn.functional.hardswish(r(x) @ r(l0.weight).t() + l0.bias)) @ r(l3.weight).t() + l3.bias
    assert (o(x, training=False, mtype=torch.float16) - ref).abs().max().item() <= 1e-12
    assert not torch.equal(o(x, training=False, mtype=torch.float16), o(x, training=False))


# ---------------------------------------------------------------------------------------------------------- the conv stack
def _conv_model(seed, p=0.0, mom=0.1, eps=1e-5):
    """CNNSmallOracle with random BatchNorm affine parameters and running statistics (at the default init the stem's and the
    pointwise BNs' dgamma are structurally ~0) and the given momentum / eps on every BatchNorm."""
    from oracle.cnn_small import CNNSmallOracle
    torch.manual_seed(seed)
    model = CNNSmallOracle(dropout=p, dropout_seed=11).double()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.momentum, m.eps = mom, eps
    return model


def _capture(model):
    """forward hooks: every conv output y_l and every BatchNorm output z_l (its .grad is dL/dz_l after a backward)."""
    convs = [model.stem.conv] + [c for blk in model.blocks for c in (blk.dw, blk.pw)]
    bns = [model.stem.bn] + [c for blk in model.blocks for c in (blk.dw_bn, blk.pw_bn)]
    ys, zs = [], []

    def keep_z(m, i, o):
        o.retain_grad()
        zs.append(o)

    for c in convs:
        c.register_forward_hook(lambda m, i, o: ys.append(o.detach()))
    for b in bns:
        b.register_forward_hook(keep_z)
    return ys, zs


@pytest.mark.parametrize("head,B,Fd,T,p", [("freq", 3, 13, 17, 0.0), ("freq", 4, 2, 9, 0.0), ("gap", 3, 11, 14, 0.0),
                                           ("gap", 5, 7, 9, 0.4)])
def test_unrounded_conv_stack_restatement_is_autograd(head, B, Fd, T, p):
    """Without rounding and masks, oracle/conv_stack.py IS autograd of CNNSmallOracle (GAP head, dropout included) and of
    CRNNOracle.front + mean over frequency: y_l, z_l's gradient, running statistics, the head's output and every gradient to
    ~1e-12, at a non-default momentum and eps."""
    from oracle.cnn_small import dropout_keep_mask
    from oracle.conv_stack import conv_stack_restated, cnn_params, grad_names, NL
    mom, eps = 0.25, 1e-3
    model = _conv_model(B * 10 + Fd, p=p, mom=mom, eps=eps)
    params = cnn_params(model)
    model.dropout_step = 3
    g = torch.Generator().manual_seed(Fd * T)
    x = torch.randn(B, 1, Fd, T, generator=g, dtype=torch.float64) * 2 - 4
    ys, zs = _capture(model)
    model.train()
    if head == "freq":
        from oracle.crnn import CRNNOracle
        crnn = CRNNOracle(dropout=0.0)
        crnn.front = f = model                       # CRNNOracle.forward's front-end, up to the GRU
        h = torch.relu(f.stem.bn(f.stem.conv(x)))
        for blk in f.blocks:
            h = blk(h)
        ref = h.mean(dim=2).transpose(1, 2)
        dout = torch.randn(ref.shape, generator=g, dtype=torch.float64)
        keep = None
    else:
        ref = model(x)
        dout = torch.randn(ref.shape, generator=g, dtype=torch.float64)
        keep = dropout_keep_mask(B, 64, p, 11, 3) if p > 0 else None
        assert keep is None or not keep.all()
    (ref * dout).sum().backward()
    o = conv_stack_restated(params, x, momentum=mom, eps=eps, head=head, dout=dout, keep=keep, dropout_p=p)
    err = lambda a, b: (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
    assert err(o["seq" if head == "freq" else "logits"], ref.detach()) <= 1e-12
    bns = [model.stem.bn] + [c for blk in model.blocks for c in (blk.dw_bn, blk.pw_bn)]
    for l in range(NL):
        assert err(o["y"][l], ys[l]) <= 1e-12, l
        assert err(o["g"][l], zs[l].grad) <= 1e-11, l
        assert err(o["running_mean"][l], bns[l].running_mean) <= 1e-12, l
        assert err(o["running_var"][l], bns[l].running_var) <= 1e-12, l
    names = grad_names(head)
    assert sorted(o["grads"]) == sorted(names)
    ref_grads = dict(model.named_parameters())
    for n in names:
        assert err(o["grads"][n], ref_grads[n].grad) <= 1e-10, n


@pytest.mark.parametrize("mt", [None, "bf16", "fp16"])
@pytest.mark.parametrize("head", ["freq", "gap"])
def test_conv_stack_restatement_own_masks_and_rounding(mt, head):
    """Handed its own ReLU decisions, the restatement computes exactly what it computes without masks; in a 16-bit mode every
    stored y_l and g_l is a value of the storage type, and the rounding changes the result (it is not silently skipped)."""
    from oracle.conv_stack import conv_stack_restated, cnn_params, NL
    mtype = MT.get(mt)
    model = _conv_model(7)
    g = torch.Generator().manual_seed(2)
    B, Fd, T = 3, 9, 15
    x = torch.randn(B, 1, Fd, T, generator=g, dtype=torch.float64) * 2 - 4
    dout = torch.randn((B, 8, 64) if head == "freq" else (B, 2), generator=g, dtype=torch.float64) * 1000
    kw = dict(mtype=mtype, head=head, dout=dout, momentum=0.2, eps=1e-4)
    a = conv_stack_restated(cnn_params(model), x, **kw)
    b = conv_stack_restated(cnn_params(model), x, masks=a["mask"], **kw)
    for k in ("y", "g", "scale", "shift", "running_mean", "running_var"):
        assert all(torch.equal(u, v) for u, v in zip(a[k], b[k])), k
    assert all(torch.equal(a["grads"][n], b["grads"][n]) for n in a["grads"])
    if mtype is None:
        return
    for l in range(NL):
        assert torch.equal(mround(a["y"][l], mtype), a["y"][l]), l
        if head == "freq" or l < 8:                  # GAP's layer-8 gradient is the fp32 pooled gradient
            assert torch.equal(mround(a["g"][l], mtype), a["g"][l]), l
    c = conv_stack_restated(cnn_params(model), x, masks=a["mask"], **{**kw, "mtype": None})
    assert not torch.equal(c["grads"]["blocks.3.pw.weight"], a["grads"]["blocks.3.pw.weight"])


def test_conv_stack_restatement_eval_mode():
    """training=False: scale / shift from the running statistics, which stay as they are; the output is the module's in
    eval mode."""
    from oracle.conv_stack import conv_stack_restated, cnn_params, NL
    model = _conv_model(3, mom=0.3, eps=1e-2)
    x = torch.randn(2, 1, 10, 12, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    model.eval()
    ref = model(x).detach()
    o = conv_stack_restated(cnn_params(model), x, training=False, eps=1e-2, head="gap")
    assert (o["logits"] - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    bns = [model.stem.bn] + [c for blk in model.blocks for c in (blk.dw_bn, blk.pw_bn)]
    for l in range(NL):
        assert torch.equal(o["running_mean"][l], bns[l].running_mean) and torch.equal(o["running_var"][l], bns[l].running_var)
    with pytest.raises(ValueError):
        conv_stack_restated(cnn_params(model), x, training=False, head="gap", dout=torch.zeros(2, 2, dtype=torch.float64))


def _mnv3(seed):
    """float64 MobileNetV3Oracle with random BatchNorm affine parameters and running statistics, SE and head biases."""
    from oracle.mobilenetv3 import MobileNetV3Oracle
    torch.manual_seed(seed)
    m = MobileNetV3Oracle(2, dropout=0.3, seed=6)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0, 0.2)
                mod.running_mean.normal_(0, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
            elif isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear)) and mod.bias is not None:
                mod.bias.normal_(0, 0.2)
    return m


@pytest.mark.parametrize("se_rounded", [False, True])
def test_unrounded_mobilenetv3_restatement_is_autograd(se_rounded):
    """mtype None: the rounding-aware walk (RoundedLinear GEMMs, the composed SE with se_rounded) is the plain float64 model --
    logits, every gradient, the running statistics after the step and the eval logits, to ~1e-12 per tensor."""
    import copy
    import torch.nn.functional as Fn
    a = _mnv3(2)
    b = copy.deepcopy(a)
    x = torch.randn(3, 1, 24, 30, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2 - 4
    y = torch.tensor([0, 1, 1])
    outs = []
    for m, kw in ((a, {}), (b, {"restate": True, "se_rounded": se_rounded})):
        m.train()
        out = m(x, step=2, **kw)
        Fn.cross_entropy(out, y).backward()
        m.eval()
        with torch.no_grad():
            outs.append((out.detach(), m(x, training=False, **kw)))
    err = lambda u, v: (u - v).abs().max().item() / max(v.abs().max().item(), 1e-300)
    assert err(outs[1][0], outs[0][0]) <= 1e-12 and err(outs[1][1], outs[0][1]) <= 1e-12
    grads = list(b.named_parameters())
    assert len(grads) == 142
    scale = max(q.grad.abs().max().item() for q in a.parameters())
    for (n, p), q in zip(grads, a.parameters()):
        # (the projection BatchNorms' dbeta is structurally zero -- a 1x1 conv + BatchNorm follows -- hence the floor)
        assert (p.grad - q.grad).abs().max().item() <= 1e-11 * max(q.grad.abs().max().item(), 1e-4 * scale), n
    for (n, u), v in zip(b.named_buffers(), a.buffers()):
        assert torch.equal(u, v) if not u.is_floating_point() else err(u, v) <= 1e-12, n


@pytest.mark.parametrize("mt", ["bf16", "fp16"])
def test_rounded_linear_rounds_dpre_w_and_x(mt):
    """RoundedLinear: forward R(x) R(W)^T + b; backward dX = R(dpre) R(W), dW = R(dpre)^T R(x), db = colsum(dpre) -- against an
    explicit computation, and differing from the unrounded one (the rounding is really applied)."""
    from oracle.mobilenetv3 import RoundedLinear
    mtype = MT[mt]
    g = torch.Generator().manual_seed(4)
    x = torch.randn(7, 5, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(3, 5, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(3, generator=g, dtype=torch.float64).requires_grad_(True)
    dpre = torch.randn(7, 3, generator=g, dtype=torch.float64)
    R = lambda t: mround(t.detach(), mtype)
    y = RoundedLinear.apply(x, w, b, mtype)
    assert torch.equal(y.detach(), R(x) @ R(w).t() + b.detach())
    y.backward(dpre)
    assert torch.equal(x.grad, R(dpre) @ R(w))
    assert torch.equal(w.grad, R(dpre).t() @ R(x))
    assert torch.equal(b.grad, dpre.sum(0))
    assert not torch.equal(x.grad, dpre @ w.detach()) and not torch.equal(w.grad, dpre.t() @ x.detach())


@pytest.mark.parametrize("mt", ["bf16", "fp16"])
def test_mobilenetv3_restatement_rounding_takes_effect(mt):
    """A matrix type moves the restated model, the eval stem rounds its operands, and se_rounded changes the result (the
    composed SE rounds its FCs)."""
    import copy
    mtype = MT[mt]
    m = _mnv3(3)
    x = torch.randn(2, 1, 16, 20, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 2 - 4
    err = lambda u, v: (u - v).abs().max().item() / max(v.abs().max().item(), 1e-300)
    outs = {}
    for kw in ({}, {"mtype": mtype}, {"mtype": mtype, "se_rounded": True}):
        mm = copy.deepcopy(m).train()
        outs[len(kw)] = mm(x, restate=True, **kw).detach()
    assert err(outs[1], outs[0]) > 0
    assert err(outs[2], outs[1]) > 0
    mm = copy.deepcopy(m).eval()
    mm.mobilenet.features[0][0].weight.data += 1e-3          # the eval stem GEMM sees its operands rounded: a change far
    e0 = mm(x, training=False, restate=True, mtype=mtype)     # below the rounding quantum of most weights moves nothing
    mm.mobilenet.features[0][0].weight.data += 1e-9
    assert torch.equal(e0, mm(x, training=False, restate=True, mtype=mtype))
