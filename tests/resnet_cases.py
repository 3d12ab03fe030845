"""Float64 restatements of the dense Conv2d layer, MaxPool2d(3, 2, 1), the BasicBlock and ResNet18Wakeword, shared by
test_resnet_host.py and test_resnet_gpu.py.

The convolution, the pool and the classifier are written out by hand, forward and backward (autograd only chains them through
``torch.autograd.Function``s whose backward is the hand-written one), so the points where the 16-bit matrix modes round are explicit:
an operand is rounded (``oracle.rounding.mround``) where the device stages it for the matrix cores -- x and W in the forward product,
dy and W in the dX product, dy and x in the dW product, likewise in ``fc`` -- and nothing else is (the one-channel stem, BatchNorm,
ReLU, the pool, the mean and the loss stay wide).  ``mtype=None`` is the exact layer / model."""
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from oracle.rounding import mround

GOLDEN = Path(__file__).parent / "golden" / "g11_resnet18.npz"
LAYERS = ((64, 1), (128, 2), (256, 2), (512, 2))
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


# ------------------------------------------------------------------------------------------ one layer, channels-last
def out_size(n, k, stride):
    return (n + 2 * (k // 2) - k) // stride + 1


def _taps(xp, k, stride, Ho, Wo):
    """The k*k displaced views (B,Ho,Wo,C) of the padded input, in (r, s) order."""
    for r in range(k):
        for s in range(k):
            yield r, s, xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride]


def conv2d_fwd(x, w, stride=1, mtype=None):
    """x (B,H,W,Cin), w (Cout,Cin,k,k) float64 -> y (B,Ho,Wo,Cout): nn.Conv2d(stride, padding=k//2, bias=False)."""
    B, H, W, _ = x.shape
    k, p = w.shape[2], w.shape[2] // 2
    Ho, Wo = out_size(H, k, stride), out_size(W, k, stride)
    xp, wr = F.pad(mround(x, mtype), (0, 0, p, p, p, p)), mround(w, mtype)
    y = torch.zeros(B, Ho, Wo, w.shape[0], dtype=torch.float64)
    for r, s, xs in _taps(xp, k, stride, Ho, Wo):
        y += xs @ wr[:, :, r, s].t()
    return y


def conv2d_bwd(x, w, dy, stride=1, mtype=None):
    """-> (dx, dw) of conv2d_fwd for the gradient dy of its output."""
    B, H, W, Cin = x.shape
    k, p = w.shape[2], w.shape[2] // 2
    Ho, Wo = dy.shape[1], dy.shape[2]
    xp, wr, gr = F.pad(mround(x, mtype), (0, 0, p, p, p, p)), mround(w, mtype), mround(dy, mtype)
    dxp, dw = torch.zeros(B, H + 2 * p, W + 2 * p, Cin, dtype=torch.float64), torch.zeros_like(w)
    for r, s, xs in _taps(xp, k, stride, Ho, Wo):
        dxp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride] += gr @ wr[:, :, r, s]
        dw[:, :, r, s] = torch.einsum("bhwn,bhwc->nc", gr, xs)
    return dxp[:, p:p + H, p:p + W].contiguous(), dw


def layer_case(x, w, dy, stride, mtype=None):
    """The layer as ww_conv2d_fwd / _bwd run it, and the same on absolute values: ``*_abs`` = sum |a b| of every output element,
    the scale of its round-off."""
    y = conv2d_fwd(x, w, stride, mtype)
    dx, dw = conv2d_bwd(x, w, dy, stride, mtype)
    ya = conv2d_fwd(x.abs(), w.abs(), stride, mtype)
    dxa, dwa = conv2d_bwd(x.abs(), w.abs(), dy.abs(), stride, mtype)
    return dict(y=y, dx=dx, dw=dw, y_abs=ya, dx_abs=dxa, dw_abs=dwa)


def layer_inputs(B, H, W, Cin, Cout, k, stride, seed, integer):
    """float64 inputs that float32 holds exactly.  integer: x, dy in [-4, 4], W in [-2, 2], all integers -- every product and sum is
    exact in fp32 and in both 16-bit operand types.  Every sample and every image row has a pattern of its own (independent draws,
    and channel 0 is a ramp whose phase depends on sample and row), so a read across a row or sample boundary cannot cancel.
    Otherwise x, dy ~ N(0,1) and W in nn.Conv2d's initialisation range."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_size(H, k, stride), out_size(W, k, stride)
    if integer:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
        x = ri(-4, 4, B, H, W, Cin)
        x[..., 0] = ((torch.arange(B)[:, None, None] * 5 + torch.arange(H)[None, :, None] * 3 + torch.arange(W)[None, None, :]) % 9 - 4).double()
        return dict(x=x, w=ri(-2, 2, Cout, Cin, k, k), dy=ri(-4, 4, B, Ho, Wo, Cout))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()
    bound = (Cin * k * k) ** -0.5
    w = ((torch.rand(Cout, Cin, k, k, generator=g, dtype=torch.float64) * 2 - 1) * bound).float().double()
    return dict(x=rn(B, H, W, Cin), w=w, dy=rn(B, Ho, Wo, Cout))


def stem_case(x, w, dy, stride):
    """The one-channel stem: x (B,H,W), w (C,1,k,k), dy (B,Ho,Wo,C) -> (y, dw)."""
    y = conv2d_fwd(x[..., None], w, stride)
    _, dw = conv2d_bwd(x[..., None], w, dy, stride)
    return y, dw


# ------------------------------------------------------------------------------------------ MaxPool2d(3, 2, 1)
def maxpool_fwd(x):
    """x (B,H,W,C) -> (y (B,Ho,Wo,C), idx: flat h*W + w of the FIRST maximal element of each window in row-major order)."""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.full((B, Ho, Wo, C), -float("inf"), dtype=x.dtype)
    idx = torch.full((B, Ho, Wo, C), -1, dtype=torch.long)
    ho, wo = torch.arange(Ho), torch.arange(Wo)
    for r in range(3):
        for s in range(3):
            hi, wi = 2 * ho + r - 1, 2 * wo + s - 1
            vh, vw = (hi >= 0) & (hi < H), (wi >= 0) & (wi < W)
            if not vh.any() or not vw.any():
                continue
            v = x[:, hi[vh]][:, :, wi[vw]]
            flat = (hi[vh][:, None] * W + wi[vw][None, :])[None, :, :, None].expand_as(v)
            cur_y, cur_i = y[:, vh][:, :, vw], idx[:, vh][:, :, vw]
            take = v > cur_y                                   # strictly greater: the first maximal element keeps the window
            sub_y, sub_i = torch.where(take, v, cur_y), torch.where(take, flat, cur_i)
            hsel, wsel = torch.nonzero(vh)[:, 0], torch.nonzero(vw)[:, 0]
            y[:, hsel[:, None], wsel[None, :]] = sub_y
            idx[:, hsel[:, None], wsel[None, :]] = sub_i
    return y, idx


def maxpool_bwd(idx, dy, H, W):
    """dx (B,H,W,C): each window's gradient lands on the element ``idx`` names."""
    B, Ho, Wo, C = dy.shape
    dx = torch.zeros(B, H * W, C, dtype=dy.dtype)
    dx.scatter_add_(1, idx.reshape(B, Ho * Wo, C), dy.reshape(B, Ho * Wo, C))
    return dx.reshape(B, H, W, C)


# ------------------------------------------------------------------------------------------ autograd shells around the hand-written pieces
class _Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, mtype):
        ctx.save_for_backward(x, w)
        ctx.args = (stride, mtype)
        return conv2d_fwd(x, w, stride, mtype)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx, dw = conv2d_bwd(x, w, dy, *ctx.args)
        return dx, dw, None, None


class _Pool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y, idx = maxpool_fwd(x)
        ctx.idx, ctx.hw = idx, x.shape[1:3]
        return y

    @staticmethod
    def backward(ctx, dy):
        return maxpool_bwd(ctx.idx, dy, *ctx.hw)


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w, b, mtype):
        ctx.save_for_backward(h, w)
        ctx.mtype = mtype
        return mround(h, mtype) @ mround(w, mtype).t() + b

    @staticmethod
    def backward(ctx, g):
        h, w = ctx.saved_tensors
        gr = mround(g, ctx.mtype)
        return gr @ mround(w, ctx.mtype), gr.t() @ mround(h, ctx.mtype), g.sum(0), None


def _bn(x, sd, pre, training):
    """nn.BatchNorm2d on the last axis of a channels-last tensor; updates sd[pre + running_*] in training mode."""
    shape = x.shape
    y = F.batch_norm(x.reshape(-1, shape[-1]), sd[pre + "running_mean"], sd[pre + "running_var"], sd[pre + "weight"], sd[pre + "bias"],
                     training, BN_MOMENTUM, BN_EPS)
    return y.reshape(shape)


def basic_block(x, sd, pre, stride, training, mtype=None, pres=None):
    """torchvision's BasicBlock on (B,H,W,C) float64 from the entries ``pre + ...`` of a state dict; ``pres`` collects the two
    ReLU inputs."""
    p1 = _bn(_Conv.apply(x, sd[pre + "conv1.weight"], stride, mtype), sd, pre + "bn1.", training)
    o = _bn(_Conv.apply(p1.clamp_min(0.0), sd[pre + "conv2.weight"], 1, mtype), sd, pre + "bn2.", training)
    idn = x
    if pre + "downsample.0.weight" in sd:
        idn = _bn(_Conv.apply(x, sd[pre + "downsample.0.weight"], stride, mtype), sd, pre + "downsample.1.", training)
    p2 = o + idn
    if pres is not None:
        pres += [p1, p2]
    return p2.clamp_min(0.0)


class ResNetRestated:
    """ResNet18Wakeword in float64 from a reference state dict (keys ``resnet.*``), with the build's Philox mask in front of
    ``fc`` (stream 15, one row per sample).  Running statistics live in ``self.sd`` and move as nn.BatchNorm2d moves them."""

    def __init__(self, sd, dropout=0.0, seed=0, mtype=None):
        self.sd = {k: (v.detach().double().cpu().clone() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in sd.items()}
        self.p = float(np.float32(dropout))
        self.seed, self.mtype = seed, mtype
        self.params = [k for k in self.sd if k.endswith(("weight", "bias"))]

    def keep_mask(self, B, C, step, sample_offset):
        """The _HiddenDropout law: ww_dropout_bt on (B, 1, C), stream 15 -> keep / (1 - p)."""
        from oracle.gru import dropout_bt_mask
        return torch.from_numpy(dropout_bt_mask(B, 1, C, self.p, self.seed, step, sample_offset, 15))[:, 0].double() / (1.0 - self.p)

    def forward(self, x, training=True, step=0, sample_offset=0):
        """x (B,1,F,T) float64 -> logits; ``self.pres`` = the 17 ReLU inputs in forward order (stem, then two per block)."""
        sd, mt = self.sd, self.mtype
        self.pres = []
        p = _bn(_Conv.apply(x[:, 0, :, :, None], sd["resnet.conv1.weight"], 2, None), sd, "resnet.bn1.", training)
        self.pres.append(p)
        h = _Pool.apply(p.clamp_min(0.0))
        for i, (_, stride) in enumerate(LAYERS):
            for j in range(2):
                h = basic_block(h, sd, f"resnet.layer{i + 1}.{j}.", stride if j == 0 else 1, training, mt, self.pres)
        pooled = h.mean((1, 2))
        if training and self.p > 0:
            pooled = pooled * self.keep_mask(pooled.shape[0], pooled.shape[1], step, sample_offset)
        if training:
            for k in sd:
                if k.endswith("num_batches_tracked"):
                    sd[k] = sd[k] + 1
        return _Linear.apply(pooled, sd["resnet.fc.1.weight"], sd["resnet.fc.1.bias"], mt)

    @property
    def relu_masks(self):
        return [p.detach() > 0 for p in self.pres]

    def loss_and_grads(self, x, y, training=True, step=0, sample_offset=0):
        """Mean cross-entropy of forward(x) against y -> (logits, loss, {key: gradient})."""
        for k in self.params:
            self.sd[k].requires_grad_(True)
            self.sd[k].grad = None
        logits = self.forward(x, training, step, sample_offset)
        loss = F.cross_entropy(logits, y)
        loss.backward()
        grads = {k: self.sd[k].grad.clone() for k in self.params}
        for k in self.params:
            self.sd[k].requires_grad_(False)
        return logits.detach(), loss.item(), grads


# ------------------------------------------------------------------------------------------ the fixture
def golden_case():
    """-> (state dict, fixture arrays) of g11_resnet18.npz; the parameters are regenerated from the stored seed and confirmed
    against the stored samples."""
    from tests.golden.make_golden_resnet18 import reference_params, sample_index
    g = np.load(GOLDEN)
    keys = [str(k) for k in g["keys"]]
    shapes = {k: tuple(int(s) for s in g["shape." + k]) for k in keys}
    params = reference_params(int(g["param_seed"]), keys, shapes)
    for k in keys:
        assert np.array_equal(params[k].reshape(-1)[sample_index(params[k].size)], g["psamp." + k]), k
    sd = {k: torch.from_numpy(np.asarray(params[k])) for k in keys}
    arrays = {k: g[k] for k in ("x", "y", "logits_eval", "logits_train", "loss", "relu_margin", "relu_inputs", "err.logits_eval",
                                "err.logits_train", "err.loss")}
    arrays["keys"], arrays["shapes"] = keys, shapes
    pkeys = [k for k in keys if k.endswith(("weight", "bias"))]
    arrays["gsamp"] = {k: g["gsamp." + k] for k in pkeys}
    arrays["gmax"] = {k: float(g["gmax." + k]) for k in pkeys}
    arrays["err.grad"] = {k: float(g["err.grad." + k]) for k in pkeys}
    skeys = [k for k in keys if "running_" in k]
    arrays["rstat"] = {k: g["rstat." + k] for k in skeys}
    arrays["err.rstat"] = {k: float(g["err.rstat." + k]) for k in skeys}
    return sd, arrays


def sampled_rel(grad, arrays, name):
    """Error of a gradient at the fixture's sampled entries, relative to the reference gradient's largest |entry|."""
    from tests.golden.make_golden_resnet18 import sample_index
    got = torch.as_tensor(grad).detach().cpu().double().reshape(-1)[torch.from_numpy(sample_index(grad.numel()))]
    return (got - torch.from_numpy(arrays["gsamp"][name]).double()).abs().max().item() / arrays["gmax"][name]


def rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)
