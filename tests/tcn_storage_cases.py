"""Float64 restatement of the causal Conv1d layer, of a TemporalBlock and of TCNWakeword with 16-bit ACTIVATION STORAGE
(``storage="bf16" | "fp16"``), shared by test_tcn_storage_host.py and test_tcn_storage_gpu.py.

The contract: arithmetic is wide, a value is rounded (RNE to the storage type S, ``oracle.rounding.mround``: through fp32, as the
device's fp32 arithmetic followed by its store does) exactly where the device stores a tensor and nowhere else:
  x0   = S(features)
  y    = S([relu](acc + bias [+ residual]))         acc over the stored input and S(W)
  h    = S(y * keep * 1/(1-p))                       the dropout pass (h = y without dropout)
  out  = S(relu(h2 + (x | acc_d + bias_d)))          the downsample convolution's own output is never stored
  dpre = S(dy * scale * [y != 0] * [y2 != 0])        masks read off the STORED outputs
  dx   = S(acc) | S(acc + dx_in)                     over the stored dpre and S(W^T)
  dw, db: wide sums over the stored dpre and the stored input;  the head's gradient is S(dpooled / T).
The pieces are tests/tcn_cases.py's conv_fwd / conv_bwd with ``mtype`` = S (rounding a stored operand again changes nothing; W is
rounded there).  ``st=None`` has no storage point and equals ``TCNRestated`` bit for bit (test_tcn_storage_host.py).  Every stage
returns its stored tensors both unrounded (``*_raw``) and rounded, and takes its stored predecessors as arguments, so a test can seed
it with what the device stored."""
import numpy as np
import torch

from oracle.rounding import mround
from tests.tcn_cases import conv_bwd, conv_fwd

ST_NAMES = ("ww_tconv1d_st_scratch_bytes", "ww_tconv1d_st_fwd", "ww_tconv1d_st_bwd", "ww_dropout_bt_st", "ww_add_relu_st_fwd",
            "ww_seq_round_st")
# (B, T, Cin, Cout, k, d): one row, one tap, minimum channels; (k-1) d >= T with 80-byte rows and a K tail of 40 in 64; M tiles that
# span samples; channel counts below a tile and N no multiple of 64; B T = 260: two dW row ranges; K = 768 and four column tiles
ST_SHAPES = [(1, 1, 8, 8, 1, 1), (2, 5, 40, 64, 3, 4), (5, 33, 40, 64, 2, 1), (3, 67, 64, 128, 3, 2), (3, 19, 24, 40, 5, 3),
             (2, 130, 128, 256, 3, 4), (2, 70, 256, 256, 3, 4)]


def drop_scale(p, st):
    """1 / (1 - p) of the float32 p: the device's own factor (rounded to float32) under storage, TCNRestated's float64 one without."""
    p32 = float(np.float32(p))
    if p32 <= 0:
        return 1.0
    s = 1.0 / (1.0 - p32)
    return s if st is None else float(np.float32(s))


# ------------------------------------------------------------------------------------------ one layer
def st_layer(x, w, b, dy, d, st, relu=False, residual=None, y2=None, scale=1.0, dx_in=None):
    """ww_tconv1d_st_fwd / _bwd on stored x, dy, residual, y2, dx_in (float64 values that S holds) -> every tensor of the call."""
    pre = conv_fwd(x, w, b, d, st)
    if residual is not None:
        pre = pre + residual
    y_raw = pre.clamp_min(0.0) if relu else pre
    y = mround(y_raw, st)
    dpre_raw = dy * scale
    if relu:
        dpre_raw = dpre_raw * (y != 0)
    if y2 is not None:
        dpre_raw = dpre_raw * (y2 != 0)
    dpre = mround(dpre_raw, st)
    dx_raw, dw, db = conv_bwd(x, w, dpre, d, st)
    if dx_in is not None:
        dx_raw = dx_raw + dx_in
    return dict(pre=pre, y_raw=y_raw, y=y, dpre_raw=dpre_raw, dpre=dpre, dx_raw=dx_raw, dx=mround(dx_raw, st), dw=dw, db=db)


# ------------------------------------------------------------------------------------------ one block, stage by stage
class BlockStages:
    """A TemporalBlock under storage.  P: w1, b1, w2, b2 and, for a downsample block, wd, bd.  keep1 / keep2: the dropout masks
    (0 | 1, float64) or None; scale: ``drop_scale``.  Every stage takes the STORED tensors it reads."""

    def __init__(self, P, d, st, keep1=None, keep2=None, scale=1.0):
        self.P, self.d, self.st, self.keep, self.scale = P, d, st, (keep1, keep2), scale
        self.down = "wd" in P

    def _conv_drop(self, x, w, b, keep):
        pre = conv_fwd(x, w, b, self.d, self.st)
        y_raw = pre.clamp_min(0.0)
        y = mround(y_raw, self.st)
        h_raw = y if keep is None else y * (keep * self.scale)
        return dict(pre=pre, y_raw=y_raw, y=y, h_raw=h_raw, h=mround(h_raw, self.st))

    def h1(self, x):
        return self._conv_drop(x, self.P["w1"], self.P["b1"], self.keep[0])

    def h2(self, h1):
        return self._conv_drop(h1, self.P["w2"], self.P["b2"], self.keep[1])

    def out(self, x, h2):
        res = conv_fwd(x, self.P["wd"], self.P["bd"], 1, self.st) if self.down else x
        pre = h2 + res
        raw = pre.clamp_min(0.0)
        return dict(pre=pre, raw=raw, st=mround(raw, self.st))

    def _bwd(self, x, w, dy, d, masks, scale, dx_in=None):
        dpre_raw = dy * scale
        for m in masks:
            dpre_raw = dpre_raw * (m != 0)
        dpre = mround(dpre_raw, self.st)
        dx_raw, dw, db = conv_bwd(x, w, dpre, d, self.st)
        if dx_in is not None:
            dx_raw = dx_raw + dx_in
        return dict(dpre_raw=dpre_raw, dpre=dpre, dx_raw=dx_raw, dx=mround(dx_raw, self.st), dw=dw, db=db)

    def bwd_skip(self, x, out, dout):
        """The skip path's input gradient: the downsample convolution's backward, or dout where out != 0 (exact)."""
        if self.down:
            return self._bwd(x, self.P["wd"], dout, 1, (out,), 1.0)
        dx = dout * (out != 0)
        return dict(dx_raw=dx, dx=dx)

    def bwd_conv2(self, h1, h2, out, dout):
        return self._bwd(h1, self.P["w2"], dout, self.d, (out, h2), self.scale)

    def bwd_conv1(self, x, h1, dh1, dx_skip):
        return self._bwd(x, self.P["w1"], dh1, self.d, (h1,), self.scale, dx_in=dx_skip)


def block_params(sd, pre):
    P = {a: sd[pre + n] for a, n in (("w1", "conv1.weight"), ("b1", "conv1.bias"), ("w2", "conv2.weight"), ("b2", "conv2.bias"))}
    if pre + "downsample.weight" in sd:
        P["wd"], P["bd"] = sd[pre + "downsample.weight"], sd[pre + "downsample.bias"]
    return P


# ------------------------------------------------------------------------------------------ the model
class TCNStorageRestated:
    """TCNWakeword(mode=S, storage=S) in float64 from a state dict (``st=None``: TCNRestated's arithmetic, bit for bit).  Keeps
    ``stored``: {name: (unrounded, rounded)} of every tensor the device stores, in the order it stores them."""

    def __init__(self, sd, dropout=0.0, seed=0, st=None):
        self.sd = {k: v.detach().double().cpu() for k, v in sd.items()}
        self.n_blocks = 0
        while f"tcn.network.{self.n_blocks}.conv1.weight" in self.sd:
            self.n_blocks += 1
        self.p = float(np.float32(dropout))
        self.seed, self.st = seed, st
        self.scale = drop_scale(dropout, st)

    def _mask(self, B, T, C, training, step, sample_offset, stream_id):
        from oracle.gru import dropout_bt_mask
        if not training or self.p <= 0:
            return None
        return torch.from_numpy(dropout_bt_mask(B, T, C, self.p, self.seed, step, sample_offset, stream_id)).double()

    def forward(self, x, training=True, step=0, sample_offset=0):
        """x (B,T,F) float64 features -> logits (B, classes)."""
        sd, st = self.sd, self.st
        B, T, _ = x.shape
        self.stored, self.blocks = {"x0": (x, mround(x, st))}, []
        x = self.stored["x0"][1]
        for i in range(self.n_blocks):
            P = block_params(sd, f"tcn.network.{i}.")
            C = P["w1"].shape[0]
            blk = BlockStages(P, 2 ** i, st, self._mask(B, T, C, training, step, sample_offset, 16 + 2 * i),
                              self._mask(B, T, C, training, step, sample_offset, 17 + 2 * i), self.scale)
            h1 = blk.h1(x)
            h2 = blk.h2(h1["h"])
            out = blk.out(x, h2["h"])
            self.stored.update({f"{i}.y1": (h1["y_raw"], h1["y"]), f"{i}.h1": (h1["h_raw"], h1["h"]), f"{i}.y2": (h2["y_raw"], h2["y"]),
                                f"{i}.h2": (h2["h_raw"], h2["h"]), f"{i}.out": (out["raw"], out["st"])})
            self.blocks.append((blk, x, h1["h"], h2["h"], out["st"]))
            x = out["st"]
        pooled = x.mean(1)
        kf = self._mask(B, 1, pooled.shape[1], training, step, sample_offset, 15)
        # (the head's dropout is an fp32 pass of its own: TCNRestated's factor)
        self.kf = None if kf is None else kf[:, 0] / (1.0 - self.p)
        self.hd = pooled if self.kf is None else pooled * self.kf
        self.T = T
        return mround(self.hd, st) @ mround(sd["fc.3.weight"], st).t() + sd["fc.3.bias"]

    def backward(self, dlogits):
        """-> ({state-dict key: gradient}, dx)"""
        sd, st = self.sd, self.st
        g = {}
        gr = mround(dlogits, st)
        g["fc.3.weight"] = gr.t() @ mround(self.hd, st)
        g["fc.3.bias"] = dlogits.sum(0)
        dh = gr @ mround(sd["fc.3.weight"], st)
        if self.kf is not None:
            dh = dh * self.kf
        raw = (dh / self.T)[:, None, :].expand(-1, self.T, -1)
        dout = mround(raw, st)
        self.stored["dpool"] = (raw, dout)
        for i in reversed(range(self.n_blocks)):
            pre = f"tcn.network.{i}."
            blk, x, h1, h2, out = self.blocks[i]
            sk = blk.bwd_skip(x, out, dout)
            if blk.down:
                g[pre + "downsample.weight"], g[pre + "downsample.bias"] = sk["dw"], sk["db"]
            c2 = blk.bwd_conv2(h1, h2, out, dout)
            g[pre + "conv2.weight"], g[pre + "conv2.bias"] = c2["dw"], c2["db"]
            c1 = blk.bwd_conv1(x, h1, c2["dx"], sk["dx"])
            g[pre + "conv1.weight"], g[pre + "conv1.bias"] = c1["dw"], c1["db"]
            self.stored.update({f"{i}.dskip": (sk["dx_raw"], sk["dx"]), f"{i}.dpre2": (c2["dpre_raw"], c2["dpre"]),
                                f"{i}.dh1": (c2["dx_raw"], c2["dx"]), f"{i}.dpre1": (c1["dpre_raw"], c1["dpre"]),
                                f"{i}.dx": (c1["dx_raw"], c1["dx"])})
            dout = c1["dx"]
        return g, dout

    def loss_and_grads(self, x, y, training=True, step=0, sample_offset=0):
        """Mean cross-entropy of forward(x) against y -> (logits, loss, {key: gradient}, dx)."""
        logits = self.forward(x, training, step, sample_offset).requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(logits, y)
        loss.backward()
        grads, dx = self.backward(logits.grad)
        return logits.detach(), loss.item(), grads, dx
