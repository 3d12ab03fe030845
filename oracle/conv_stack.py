"""Restated conv stack of cnn_small and of the CRNN front-end (ww_model.hip, ww_conv_fwd.hip, ww_conv_bwd.hip): stem + 4 x
(depthwise 3x3, pointwise 1x1), each with BatchNorm + ReLU, then either the CRNN's mean over frequency or cnn_small's
GAP -> dropout -> Linear(64, 2).  float64, forward and backward, with exactly the values the device rounds to its storage /
matrix type rounded and nothing else.  Test infrastructure only.

Rounding points, read off the kernels (``mtype`` None restates the fp32 mode, i.e. is the exact float64 model):
  forward : every stored y_l is the fp32 result rounded RNE to the storage type, and the layer's BatchNorm statistics are
            those of the stored tensor; consumers apply fma(y, scale, shift) and ReLU in fp32.  The pointwise layers' MFMA
            operands relu(z) and W are rounded (k_pw_fwd_bf16); the stem (fp32 x, fp32 W) and the depthwise layers (fp32
            taps) take fp32 operands.  Frequency pooling and GAP sum relu(z) in fp32.
  backward: every stored g_l = dL/dz_l is rounded, and the BatchNorm-backward sums (dgamma, dbeta, the coefficients of
            dy = A g + Bc y + Cc) are sums of the stored g_l against the stored y_l.  The pointwise layers round dy and W for
            dX = dy W, and dy and relu(z) for dW (k_pw_bwd_bf16); depthwise and stem use fp32 dy, taps and activations.
            k_freqpool_bwd stores round(z > 0 ? dseq * (1/H) : 0).  GAP's layer-8 gradient (the pooled gradient) is never
            stored: it stays fp32.
A 16-bit backward is usually fed a loss-scaled upstream gradient (fp16: 65536, as GradScaler); the scale is the caller's.

``masks`` (optional): the ReLU decisions to use, one (B,64,H,W) bool tensor per layer, e.g. the device's own, so that a
value within round-off of 0 lands on the same side as on the device."""
import numpy as np
import torch
import torch.nn.functional as F

from .rounding import mround

# the C-ABI pointer order of ww_cnn_small_fwd / ww_cnn_front_fwd (include/wwhip.h), as state_dict names
PARAM_NAMES = ["stem.conv.weight", "stem.bn.weight", "stem.bn.bias", "stem.bn.running_mean", "stem.bn.running_var"]
for _i in range(4):
    for _c in ("dw", "pw"):
        PARAM_NAMES += [f"blocks.{_i}.{_c}.weight"] + [f"blocks.{_i}.{_c}_bn.{_k}" for _k in
                                                      ("weight", "bias", "running_mean", "running_var")]
PARAM_NAMES += ["classifier.weight", "classifier.bias"]
NL = 9                                              # conv layers: 0 stem, 1 + 2i depthwise i, 2 + 2i pointwise i


def widx(l):
    """pointer index of conv layer l's weight; its BatchNorm's gamma, beta, running mean, running var follow it."""
    return 0 if l == 0 else 5 * l


def grad_names(head="gap"):
    """names of the parameters with a gradient (all but the running statistics; the classifier's with the GAP head only:
    27 or 29), in pointer order."""
    return [n for n in PARAM_NAMES[:45 if head == "freq" else 47] if not n.endswith(("running_mean", "running_var"))]


def conv_stack_restated(params, x, mtype=None, momentum=0.1, eps=1e-5, training=True, masks=None, head="freq",
                        dout=None, keep=None, dropout_p=0.0):
    """params: the 45 (head "freq") or 47 (head "gap") tensors in PARAM_NAMES order, or a dict by name; x (B,1,F,T).
    head "freq": -> seq (B, ceil(T/2), 64); ``dout`` is dseq.  head "gap": -> logits (B,2); ``dout`` is dlogits, ``keep`` the
    (B,64) dropout keep-mask (None: no dropout) and ``dropout_p`` its rate.
    -> dict of float64 tensors: per layer (lists of 9) y (NCHW, as stored), scale, shift, mean, rstd, running_mean,
    running_var, mask; the head's output; with ``dout`` (training only) also g (the stored dL/dz_l, NCHW) and grads (a dict
    by name of every parameter gradient)."""
    f64 = lambda t: None if t is None else torch.as_tensor(t).detach().double().cpu()
    if isinstance(params, dict):
        params = [params.get(n) for n in PARAM_NAMES]
    P = [f64(p) for p in params]
    x = f64(x)
    R = lambda t: mround(t, mtype)
    out = {k: [] for k in ("y", "scale", "shift", "mean", "rstd", "running_mean", "running_var", "mask")}
    a_in, ops = x, []
    for l in range(NL):
        w = P[widx(l)]
        gamma, beta, rm, rv = P[widx(l) + 1:widx(l) + 5]
        if l == 0:
            op = (x, w)
            y = F.conv2d(x, w, stride=2, padding=1)
        elif l % 2 == 1:
            op = (a_in, w)
            y = F.conv2d(a_in, w, padding=1, groups=64)
        else:
            op = (R(a_in), R(w))
            y = F.conv2d(*op)
        ops.append(op)
        y = R(y)
        if training:
            n = y.numel() // 64
            mean = y.mean(dim=(0, 2, 3))
            var = y.var(dim=(0, 2, 3), unbiased=False)
            rstd = 1.0 / torch.sqrt(var + eps)
            rm_new = (1.0 - momentum) * rm + momentum * mean
            rv_new = (1.0 - momentum) * rv + momentum * (var * n / (n - 1) if n > 1 else var)
        else:
            mean, rstd, rm_new, rv_new = rm, 1.0 / torch.sqrt(rv + eps), rm, rv
        scale = gamma * rstd
        shift = beta - mean * scale
        z = y * scale[None, :, None, None] + shift[None, :, None, None]
        m = (z > 0) if masks is None else masks[l].to(torch.bool).cpu()
        a_in = z * m
        for k, v in zip(out, (y, scale, shift, mean, rstd, rm_new, rv_new, m)):
            out[k].append(v)
    H, W = a_in.shape[2], a_in.shape[3]
    if head == "freq":
        out["seq"] = a_in.mean(dim=2).transpose(1, 2).contiguous()
    elif head == "gap":
        pd = a_in.mean(dim=(2, 3))
        kscale = None
        if keep is not None:
            # the device's fp32 1/(1-p), as the oracle (oracle/cnn_small.py) and k_head_fwd take it
            drop_scale = float(np.float32(1.0 / (1.0 - float(np.float32(dropout_p)))))
            kscale = torch.as_tensor(np.asarray(keep, dtype=np.float64)) * drop_scale
            pd = pd * kscale
        out["logits"] = pd @ P[45].t() + P[46]
    else:
        raise ValueError(f"head must be 'freq' or 'gap', got {head!r}")
    if dout is None:
        return out
    if not training:
        raise ValueError("the backward needs the training-mode forward")
    dout = f64(dout)
    m8 = out["mask"][8]
    grads = {}
    if head == "freq":
        if mtype is None:
            d = dout / H
        else:                                        # fp32 product dseq * (1/H), then the storage rounding
            d = (dout.float() * torch.tensor(1.0 / H, dtype=torch.float32)).double()
        g = R(m8 * d.transpose(1, 2)[:, :, None, :])
    else:
        grads["classifier.weight"] = dout.t() @ pd
        grads["classifier.bias"] = dout.sum(0)
        dp = dout @ P[45]
        if kscale is not None:
            dp = dp * kscale
        g = m8 * (dp / (H * W))[:, :, None, None]  # the pooled gradient: not stored, fp32
    gs = [None] * NL
    for l in range(NL - 1, -1, -1):
        gs[l] = g
        y, mean, rstd, gamma = out["y"][l], out["mean"][l], out["rstd"][l], P[widx(l) + 1]
        yhat = (y - mean[None, :, None, None]) * rstd[None, :, None, None]
        n = y.numel() // 64
        dbeta = g.sum(dim=(0, 2, 3))
        dgamma = (g * yhat).sum(dim=(0, 2, 3))
        dy = (gamma * rstd)[None, :, None, None] * (g - (dbeta / n)[None, :, None, None]
                                                    - yhat * (dgamma / n)[None, :, None, None])
        name = PARAM_NAMES[widx(l)][:-len("weight")]
        bn = name[:-1] + "_bn." if l else "stem.bn."
        grads[bn + "weight"], grads[bn + "bias"] = dgamma, dbeta
        a_op, w_op = (t.clone().requires_grad_(True) for t in ops[l])
        if l == 0:
            yy = F.conv2d(a_op, w_op, stride=2, padding=1)
        elif l % 2 == 1:
            yy = F.conv2d(a_op, w_op, padding=1, groups=64)
        else:
            yy = F.conv2d(a_op, w_op)
            dy = R(dy)                               # the MFMA operand of dX and dW
        da, dw = torch.autograd.grad(yy, (a_op, w_op), dy)
        grads[name + "weight"] = dw
        if l > 0:
            g = R(out["mask"][l - 1] * da)
    out["g"] = gs
    out["grads"] = grads
    return out


def cnn_params(module):
    """PARAM_NAMES-ordered copies of a CNNSmallOracle's (or its device twin's) tensors, taken before a training forward
    updates the running statistics in place; classifier entries None when it has none."""
    sd = module.state_dict()
    return [None if sd.get(n) is None else sd[n].detach().clone() for n in PARAM_NAMES]
