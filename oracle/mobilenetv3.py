"""Oracle of ``MobileNetV3Wakeword`` (src/models/architectures.py:68-123): torchvision's ``mobilenet_v3_small`` with a
one-channel stem and the reference's classifier.  torchvision (pinned 0.16.2 by the reference's requirements.txt:7) is NOT
installed here and cannot be fetched, so the body is restated from its published definition
(torchvision/models/mobilenetv3.py: ``_mobilenet_v3_conf("mobilenet_v3_small")``, ``InvertedResidual``, ``SqueezeExcitation``
with ReLU / Hardsigmoid, ``Conv2dNormActivation``, BatchNorm eps 1e-3 momentum 0.01) in plain torch.nn with the SAME module
tree, hence the same ``state_dict`` keys (``mobilenet.features.N.block.M...``, ``mobilenet.classifier.{0,3}``).
**parity unpinned** w.r.t. torchvision itself (no fixture can be generated); arithmetic = torch.nn.  Test infrastructure.

``forward(..., restate=True, mtype=None | torch.bfloat16 | torch.float16)`` restates ``MobileNetV3Wakeword``'s matrix modes in
float64, forward and backward, rounding exactly what the device rounds (oracle/rounding.py:mround) and nothing else.  Rounding
points, read off models/mobilenet.py and the kernels (where this list and the kernels disagree, the kernels win):
  * only the ``ww_linear_mfma_*`` GEMMs round: every 1x1 convolution (expand, project, the last 96 -> 576; in training
    ``ww_conv1x1_bn_act_fwd``) and both head Linears.  Forward R(x) R(W)^T with wide sums; the BatchNorm statistics are those
    of the unrounded product and the residual is added unrounded.  Backward (``ww_linear_mfma_bwd``): dpre = dy * dropout *
    act'(pre) unrounded, dX = R(dpre) R(W), dW = R(dpre)^T R(x), db = colsum(dpre) unrounded (``RoundedLinear``);
  * every activation tensor stays fp32 in memory; the direct training stem (``ww_stem3x3s2_*``), the depthwise layers,
    BatchNorm + activation and the fused squeeze-excitation (``ww_se_*``: fp32 FMA in every matrix mode) do not round;
  * eval runs the stem as ``im2col3x3s2`` + a GEMM in the matrix type: its patches and weights ARE rounded there (the stem's
    BatchNorm in eval mode selects this path here);
  * ``se_rounded=True`` restates the composed squeeze-excitation (``_SEFn`` where ``se_supported`` is False): both FCs go
    through ``linear_mfma`` with ReLU / Hardsigmoid epilogues, so they round like any other GEMM.
With ``mtype=None`` the restatement is the float64 model itself (tests/test_restated_oracles.py checks it against autograd of
the plain forward)."""
from functools import partial

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .cnn_small import dropout_keep_mask
from .rounding import mround

# input, kernel, expanded, out, use_se, activation, stride            (mobilenet_v3_small, width 1.0)
SMALL_CONF = ((16, 3, 16, 16, True, "RE", 2), (16, 3, 72, 24, False, "RE", 2), (24, 3, 88, 24, False, "RE", 1),
              (24, 5, 96, 40, True, "HS", 2), (40, 5, 240, 40, True, "HS", 1), (40, 5, 240, 40, True, "HS", 1),
              (40, 5, 120, 48, True, "HS", 1), (48, 5, 144, 48, True, "HS", 1), (48, 5, 288, 96, True, "HS", 2),
              (96, 5, 576, 96, True, "HS", 1), (96, 5, 576, 96, True, "HS", 1))
LAST_CONV, LAST_CHANNEL = 576, 1024


def make_divisible(v, divisor=8):
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def se_channels(expanded):
    return make_divisible(expanded // 4, 8)


BN = partial(nn.BatchNorm2d, eps=0.001, momentum=0.01)


def cna(cin, cout, k, stride=1, groups=1, act=None):
    layers = [nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), BN(cout)]
    if act is not None:
        layers.append(act())
    return nn.Sequential(*layers)


class SqueezeExcitation(nn.Module):
    def __init__(self, c, cs):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1, self.fc2 = nn.Conv2d(c, cs, 1), nn.Conv2d(cs, c, 1)
        self.activation, self.scale_activation = nn.ReLU(), nn.Hardsigmoid()

    def forward(self, x):
        s = self.scale_activation(self.fc2(self.activation(self.fc1(self.avgpool(x)))))
        return s * x


class InvertedResidual(nn.Module):
    def __init__(self, cin, k, exp, cout, use_se, act, stride):
        super().__init__()
        a = nn.Hardswish if act == "HS" else nn.ReLU
        layers = []
        if exp != cin:
            layers.append(cna(cin, exp, 1, act=a))
        layers.append(cna(exp, exp, k, stride, groups=exp, act=a))
        if use_se:
            layers.append(SqueezeExcitation(exp, se_channels(exp)))
        layers.append(cna(exp, cout, 1, act=None))
        self.block = nn.Sequential(*layers)
        self.use_res_connect = stride == 1 and cin == cout

    def forward(self, x):
        y = self.block(x)
        return x + y if self.use_res_connect else y


class _MobileNet(nn.Module):
    def __init__(self, num_classes, dropout):
        super().__init__()
        feats = [cna(1, 16, 3, 2, act=nn.Hardswish)]
        feats += [InvertedResidual(*c) for c in SMALL_CONF]
        feats.append(cna(SMALL_CONF[-1][3], LAST_CONV, 1, act=nn.Hardswish))
        self.features = nn.Sequential(*feats)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Linear(LAST_CONV, LAST_CHANNEL), nn.Hardswish(), nn.Dropout(dropout),
                                        nn.Linear(LAST_CHANNEL, num_classes))


class MobileNetV3Oracle(nn.Module):
    def __init__(self, num_classes=2, dropout=0.3, seed=0, dtype=torch.float64):
        super().__init__()
        self.mobilenet = _MobileNet(num_classes, dropout).to(dtype)
        self.p, self.seed, self.dtype = float(np.float32(dropout)), seed, dtype

    def forward(self, x, step=0, sample_offset=0, training=True, mtype=None, se_rounded=False, restate=None):
        """restate (default: when ``mtype`` or ``se_rounded`` is given): the rounding-aware walk of the same modules (see the
        module docstring); otherwise plain torch.nn.  ``training`` switches the head's dropout; BatchNorm follows .train()."""
        m = self.mobilenet
        if restate is None:
            restate = mtype is not None or se_rounded
        lin = (lambda h, layer: RoundedLinear.apply(h, layer.weight, layer.bias, mtype)) if restate else (lambda h, layer: layer(h))
        if restate:
            h = x.to(self.dtype)
            for i, f in enumerate(m.features):
                h = _inverted_residual(f, h, mtype, se_rounded) if isinstance(f, InvertedResidual) else _cna(f, h, mtype, stem=i == 0)
            h = h.mean(dim=(2, 3))
        else:
            h = m.avgpool(m.features(x.to(self.dtype))).flatten(1)
        c = m.classifier
        h = F.hardswish(lin(h, c[0]))
        if training and self.p > 0:
            keep = torch.from_numpy(dropout_keep_mask(h.shape[0], h.shape[1], self.p, self.seed, step, sample_offset))
            h = h * keep.to(self.dtype) * (1.0 / (1.0 - self.p))
        return lin(h, c[3])


class RoundedLinear(torch.autograd.Function):
    """y = R(x) R(W)^T (+ b) and its backward as ``ww_linear_mfma_bwd`` computes it: the incoming gradient is dpre (whatever
    epilogue follows -- activation, dropout -- is differentiated by autograd, unrounded), dX = R(dpre) R(W),
    dW = R(dpre)^T R(x), db = colsum(dpre).  R = mround(., mtype); mtype None: the exact linear."""

    @staticmethod
    def forward(ctx, x, w, b, mtype):
        ctx.save_for_backward(x, w)
        ctx.mtype, ctx.has_b = mtype, b is not None
        y = mround(x, mtype) @ mround(w, mtype).t()
        return y + b if b is not None else y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gr = mround(g, ctx.mtype)
        return gr @ mround(w, ctx.mtype), gr.t() @ mround(x, ctx.mtype), (g.sum(0) if ctx.has_b else None), None


def _pointwise(x, w, mtype, b=None):
    """1x1 convolution of NCHW x as the device's GEMM over the pixels."""
    B, C, H, W = x.shape
    y = RoundedLinear.apply(x.permute(0, 2, 3, 1).reshape(-1, C), w.reshape(w.shape[0], C), b, mtype)
    return y.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _cna(seq, x, mtype, stem=False):
    conv, bn = seq[0], seq[1]
    if conv.kernel_size == (1, 1) and conv.groups == 1:
        y = _pointwise(x, conv.weight, mtype)
    elif stem and not bn.training:                      # eval stem: patches + GEMM in the matrix type
        y = F.conv2d(mround(x, mtype), mround(conv.weight, mtype), None, conv.stride, conv.padding)
    else:
        y = F.conv2d(x, conv.weight, None, conv.stride, conv.padding, groups=conv.groups)
    a = bn(y)
    return seq[2](a) if len(seq) > 2 else a


def _se(se, x, mtype, rounded):
    if not rounded:
        return se(x)
    s = x.mean(dim=(2, 3))
    h = torch.relu(RoundedLinear.apply(s, se.fc1.weight.flatten(1), se.fc1.bias, mtype))
    g = F.hardsigmoid(RoundedLinear.apply(h, se.fc2.weight.flatten(1), se.fc2.bias, mtype))
    return x * g[:, :, None, None]


def _inverted_residual(ir, x, mtype, se_rounded):
    h = x
    for layer in ir.block:
        h = _se(layer, h, mtype, se_rounded) if isinstance(layer, SqueezeExcitation) else _cna(layer, h, mtype)
    return x + h if ir.use_res_connect else h
