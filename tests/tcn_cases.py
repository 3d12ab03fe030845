"""Float64 restatements of the causal dilated Conv1d layer and of TCNWakeword, shared by test_tcn_host.py and test_tcn_gpu.py.

Everything is written out by hand (no autograd), so the points where the 16-bit matrix modes round are explicit: an operand is
rounded (``oracle.rounding.mround``) where the device stages it for the matrix cores -- x and W in the forward product, dpre and W
in the dX product, dpre and x in the dW product -- and nothing else is (bias, residual, ReLU, dropout, the bias gradient, the
mean over time and the loss stay wide).  ``mtype=None`` is the exact layer / model."""
from pathlib import Path

import numpy as np
import torch

from oracle.rounding import mround

GOLDEN = Path(__file__).parent / "golden" / "g10_tcn.npz"


# ------------------------------------------------------------------------------------------ one layer
def conv_fwd(x, w, b, d, mtype=None):
    """x (B,T,Cin), w (Cout,Cin,k), b (Cout) float64 -> bias + causal convolution (B,T,Cout); steps before t = 0 read as 0."""
    B, T, _ = x.shape
    k = w.shape[2]
    xr, wr = mround(x, mtype), mround(w, mtype)
    y = b.expand(B, T, -1).clone()
    for j in range(k):
        s = (k - 1 - j) * d
        if s < T:
            y[:, s:] += xr[:, :T - s] @ wr[:, :, j].t()
    return y


def conv_bwd(x, w, dpre, d, mtype=None):
    """-> (dx, dw, db) of conv_fwd for the gradient dpre of its output."""
    B, T, _ = x.shape
    k = w.shape[2]
    xr, wr, gr = mround(x, mtype), mround(w, mtype), mround(dpre, mtype)
    dx, dw = torch.zeros_like(x), torch.zeros_like(w)
    for j in range(k):
        s = (k - 1 - j) * d
        if s < T:
            dx[:, :T - s] += gr[:, s:] @ wr[:, :, j]
            dw[:, :, j] = torch.einsum("btn,btc->nc", gr[:, s:], xr[:, :T - s])
    return dx, dw, dpre.sum((0, 1))


def layer_case(x, w, b, dy, d, relu=False, residual=None, mtype=None):
    """The layer as ww_tconv1d_fwd / _bwd run it: y = [relu](conv + bias [+ residual]); dpre = dy where y != 0 (relu)."""
    y = conv_fwd(x, w, b, d, mtype)
    if residual is not None:
        y = y + residual
    if relu:
        y = y.clamp_min(0.0)
    dpre = dy * (y != 0) if relu else dy
    dx, dw, db = conv_bwd(x, w, dpre, d, mtype)
    return dict(y=y, dx=dx, dw=dw, db=db)


def layer_inputs(B, T, Cin, Cout, k, seed, integer):
    """float64 inputs that float32 holds exactly.  integer: x, dy, residual in [-4, 4], W in [-2, 2], bias in [-3, 3], all
    integers -- every product and sum is exact in fp32 and in both 16-bit operand types.  Every sample has a pattern of its own
    (independent draws, and channel 0 is a ramp whose phase depends on the sample), so a read across a sample boundary cannot
    cancel.  Otherwise: x, dy, residual ~ N(0,1), W and bias in nn.Conv1d's initialisation range."""
    g = torch.Generator().manual_seed(seed)
    if integer:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
        x = ri(-4, 4, B, T, Cin)
        x[:, :, 0] = ((torch.arange(B)[:, None] * 3 + torch.arange(T)[None, :]) % 9 - 4).double()     # distinct per sample
        return dict(x=x, w=ri(-2, 2, Cout, Cin, k), b=ri(-3, 3, Cout), dy=ri(-4, 4, B, T, Cout), res=ri(-4, 4, B, T, Cout))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()
    bound = (Cin * k) ** -0.5
    un = lambda *s: ((torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * bound).float().double()
    return dict(x=rn(B, T, Cin), w=un(Cout, Cin, k), b=un(Cout), dy=rn(B, T, Cout), res=rn(B, T, Cout))


# ------------------------------------------------------------------------------------------ the model
class TCNRestated:
    """TCNWakeword in float64 from a reference state dict: blocks ``tcn.network.{i}`` with dilation 2^i, the build's Philox masks
    after each of a block's two ReLUs (streams 16 + 2i, 17 + 2i) and in front of fc (stream 15)."""

    def __init__(self, sd, dropout=0.0, seed=0, mtype=None):
        self.sd = {k: v.detach().double().cpu() for k, v in sd.items()}
        self.n_blocks = 0
        while f"tcn.network.{self.n_blocks}.conv1.weight" in self.sd:
            self.n_blocks += 1
        self.p = float(np.float32(dropout))
        self.seed, self.mtype = seed, mtype

    def _keep(self, B, T, C, training, step, sample_offset, stream_id):
        from oracle.gru import dropout_bt_mask
        if not training or self.p <= 0:
            return None
        return torch.from_numpy(dropout_bt_mask(B, T, C, self.p, self.seed, step, sample_offset, stream_id)).double() / (1.0 - self.p)

    def forward(self, x, training=True, step=0, sample_offset=0):
        """x (B,T,F) float64 -> logits (B, classes); keeps what backward() needs, and ``relu_masks`` (three per block)."""
        sd, mt = self.sd, self.mtype
        B, T, _ = x.shape
        self.saved, self.relu_masks = [], []
        for i in range(self.n_blocks):
            pre = f"tcn.network.{i}."
            d = 2 ** i
            w1, b1, w2, b2 = (sd[pre + n] for n in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"))
            a1 = conv_fwd(x, w1, b1, d, mt)
            k1 = self._keep(B, T, a1.shape[2], training, step, sample_offset, 16 + 2 * i)
            h1 = a1.clamp_min(0.0) * (1.0 if k1 is None else k1)
            a2 = conv_fwd(h1, w2, b2, d, mt)
            k2 = self._keep(B, T, a2.shape[2], training, step, sample_offset, 17 + 2 * i)
            h2 = a2.clamp_min(0.0) * (1.0 if k2 is None else k2)
            down = pre + "downsample.weight" in sd
            res = conv_fwd(x, sd[pre + "downsample.weight"], sd[pre + "downsample.bias"], 1, mt) if down else x
            out = (h2 + res).clamp_min(0.0)
            self.relu_masks += [a1 > 0, a2 > 0, (h2 + res) > 0]
            self.saved.append((x, h1, h2, out, k1, k2, a1 > 0, a2 > 0))
            x = out
        pooled = x.mean(1)
        kf = self._keep(B, 1, pooled.shape[1], training, step, sample_offset, 15)
        self.kf = None if kf is None else kf[:, 0]
        self.hd = pooled if self.kf is None else pooled * self.kf
        self.T = T
        return mround(self.hd, mt) @ mround(sd["fc.3.weight"], mt).t() + sd["fc.3.bias"]

    def backward(self, dlogits):
        """-> ({state-dict key: gradient}, dx)"""
        sd, mt = self.sd, self.mtype
        g = {}
        gr = mround(dlogits, mt)
        g["fc.3.weight"] = gr.t() @ mround(self.hd, mt)
        g["fc.3.bias"] = dlogits.sum(0)
        dh = gr @ mround(sd["fc.3.weight"], mt)
        if self.kf is not None:
            dh = dh * self.kf
        dout = (dh / self.T)[:, None, :].expand(-1, self.T, -1)
        for i in reversed(range(self.n_blocks)):
            pre = f"tcn.network.{i}."
            d = 2 ** i
            x, h1, h2, out, k1, k2, m1, m2 = self.saved[i]
            dsum = dout * (out > 0)
            if pre + "downsample.weight" in sd:
                dx, g[pre + "downsample.weight"], g[pre + "downsample.bias"] = conv_bwd(x, sd[pre + "downsample.weight"], dsum, 1, mt)
            else:
                dx = dsum.clone()
            da2 = dsum * (1.0 if k2 is None else k2) * m2
            dh1, g[pre + "conv2.weight"], g[pre + "conv2.bias"] = conv_bwd(h1, sd[pre + "conv2.weight"], da2, d, mt)
            da1 = dh1 * (1.0 if k1 is None else k1) * m1
            dx1, g[pre + "conv1.weight"], g[pre + "conv1.bias"] = conv_bwd(x, sd[pre + "conv1.weight"], da1, d, mt)
            dout = dx + dx1
        return g, dout

    def loss_and_grads(self, x, y, training=True, step=0, sample_offset=0):
        """Mean cross-entropy of forward(x) against y -> (logits, loss, {key: gradient}, dx)."""
        logits = self.forward(x, training, step, sample_offset).requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(logits, y)
        loss.backward()
        grads, dx = self.backward(logits.grad)
        return logits.detach(), loss.item(), grads, dx


def golden_case(prefix=""):
    """-> (state dict, fixture arrays) of one case of g10_tcn.npz; the parameters are regenerated from the stored seed and
    confirmed against the stored samples."""
    from tests.golden.make_golden_tcn import reference_params, sample_index
    g = np.load(GOLDEN)
    keys = [str(k) for k in g[prefix + "keys"]]
    shapes = {k: g[prefix + "shape." + k] for k in keys}
    params = reference_params(int(g[prefix + "param_seed"]), keys, shapes)
    for k in keys:
        assert np.array_equal(params[k].reshape(-1)[sample_index(params[k].size)], g[prefix + "psamp." + k]), k
    sd = {k: torch.from_numpy(params[k]) for k in keys}
    arrays = {k: g[prefix + k] for k in ("x", "y", "logits_eval", "logits_train", "loss", "relu_margin")}
    arrays["keys"], arrays["shapes"] = keys, shapes
    arrays["gsamp"] = {k: g[prefix + "gsamp." + k] for k in keys}
    arrays["gmax"] = {k: float(g[prefix + "gmax." + k]) for k in keys}
    return sd, arrays


def sampled_rel(grad, arrays, name):
    """Error of a gradient at the fixture's sampled entries, relative to the reference gradient's largest |entry|."""
    from tests.golden.make_golden_tcn import sample_index
    got = torch.as_tensor(grad).detach().cpu().double().reshape(-1)[torch.from_numpy(sample_index(grad.numel()))]
    return (got - torch.from_numpy(arrays["gsamp"][name]).double()).abs().max().item() / arrays["gmax"][name]


def rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)
