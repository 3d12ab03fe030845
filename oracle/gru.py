"""Oracle of the recurrent model: the reference's ``GRUWakeword`` (src/models/architectures.py:198-267: nn.GRU(input, 128,
num_layers, batch_first=True, dropout, bidirectional) -> final hidden states of the last layer concatenated -> Dropout ->
Linear) in plain torch on the CPU.  The GRU arithmetic is torch.nn.GRU's own; torch's dropout RNG cannot be reproduced on
the device, so the stack is unrolled into single-layer nn.GRU modules with the build's Philox masks applied explicitly
between layers and in front of ``fc`` (mask law: ww_dropout_bt, include/wwhip.h).  ``load_reference_state_dict`` takes a
state_dict with the reference's keys (``gru.weight_ih_l0`` ... ``fc.1.bias``).  Test infrastructure only."""
import numpy as np
import torch
import torch.nn as nn

from .philox import philox4x32_10, make_key, prob_threshold
from .rounding import mround

TAG_DROPOUT = 1


def dropout_bt_mask(B, T, C, p, seed=0, step=0, sample_offset=0, stream_id=0):
    """(B,T,C) bool keep-mask of ww_dropout_bt."""
    if p <= 0.0:
        return np.ones((B, T, C), dtype=bool)
    cq = (C + 3) // 4
    b = (np.arange(B, dtype=np.uint64) + np.uint64(sample_offset))[:, None, None]
    t = np.arange(T, dtype=np.uint64)[None, :, None]
    q = np.arange(cq, dtype=np.uint64)[None, None, :]
    field = (np.uint64(TAG_DROPOUT) << np.uint64(24)) | (np.uint64(stream_id) << np.uint64(20)) | (t << np.uint64(8)) | q
    ctr = np.empty((B, T, cq, 4), dtype=np.uint32)
    ctr[..., 0] = np.uint32(step & 0xFFFFFFFF)
    ctr[..., 1] = np.uint32((step >> 32) & 0xFFFFFFFF)
    ctr[..., 2] = np.broadcast_to(b, (B, T, cq)).astype(np.uint32)
    ctr[..., 3] = np.broadcast_to(field, (B, T, cq)).astype(np.uint32)
    r = philox4x32_10(ctr.reshape(-1, 4), make_key(seed)).astype(np.uint64).reshape(B, T, cq * 4)[:, :, :C]
    return r >= np.uint64(prob_threshold(p))


class GRUWakewordOracle(nn.Module):
    def __init__(self, input_size=40, hidden_size=128, num_layers=2, num_classes=2, bidirectional=True, dropout=0.3,
                 seed=0, dtype=torch.float64):
        super().__init__()
        nd = 2 if bidirectional else 1
        self.layers = nn.ModuleList([nn.GRU(input_size if k == 0 else nd * hidden_size, hidden_size, num_layers=1,
                                            batch_first=True, bidirectional=bidirectional) for k in range(num_layers)]).to(dtype)
        self.fc = nn.Linear(nd * hidden_size, num_classes).to(dtype)
        self.p = float(np.float32(dropout)) if num_layers > 1 else 0.0
        self.p_fc = float(np.float32(dropout))
        self.seed, self.dtype, self.nd, self.H = seed, dtype, nd, hidden_size

    def load_reference_state_dict(self, sd):
        for k, layer in enumerate(self.layers):
            for sfx in ("", "_reverse")[:self.nd]:
                for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    getattr(layer, f"{name}_l0{sfx}").data.copy_(sd[f"gru.{name}_l{k}{sfx}"].to(self.dtype))
        self.fc.weight.data.copy_(sd["fc.1.weight"].to(self.dtype))
        self.fc.bias.data.copy_(sd["fc.1.bias"].to(self.dtype))

    def forward(self, x, step=0, sample_offset=0, training=True):
        if x.dim() == 4:                                   # (B,1,F,T) features, as the Trainer hands them over
            x = x[:, 0].transpose(1, 2)
        x = x.to(self.dtype)
        B, T, _ = x.shape
        hn = None
        for k, layer in enumerate(self.layers):
            x, hn = layer(x)
            if training and self.p > 0 and k + 1 < len(self.layers):
                keep = torch.from_numpy(dropout_bt_mask(B, T, x.shape[2], self.p, self.seed, step, sample_offset, 1 + k))
                x = x * keep.to(self.dtype) * (1.0 / (1.0 - self.p))
        h = torch.cat([hn[0], hn[1]], dim=1) if self.nd == 2 else hn[0]
        if training and self.p_fc > 0:
            keep = torch.from_numpy(dropout_bt_mask(B, 1, h.shape[1], self.p_fc, self.seed, step, sample_offset, 15))[:, 0]
            h = h * keep.to(self.dtype) * (1.0 / (1.0 - self.p_fc))
        return self.fc(h)


# ---------------------------------------------------------------------------------------------------------------------------------
# Restated layer of the device's matrix modes (ww_gru.hip): one GRU direction, forward and backward, in float64 with exactly the
# values the device rounds to the matrix type rounded and nothing else.  Rounding points, read off the kernels:
#   forward : the input projection's operands x and W_ih (k_to16_pair / ww_gemm16_nt_bias or k_gemm's operand staging); each
#             step's h_{t-1} and W_hh (the per-step MFMA operands of k_gru_fwd); b_ih, b_hh, gates and state stay wide
#   backward: dGi = [dr, dz, dn] and dGh = [dr, dz, dn * r] leave k_gru_bwd in the matrix type, and the per-step product
#             dGh W_hh takes them and W_hh rounded; the dW_hh / dW_ih / dX products round their other operand (h_{t-1}, x,
#             W_ih) while staging it.  The bias gradients are sums of the UNrounded dGi / dGh.
# `mtype` None restates the fp32 parity mode, i.e. is the exact GRU; torch.bfloat16 / torch.float16 the two 16-bit modes.

def gru_restated(x, w_ih, w_hh, b_ih, b_hh, h0=None, dy=None, dh_n=None, mtype=None, reverse=False):
    """One direction, batch-first.  x (B,T,I); h0, dh_n (B,H) or None; dy (B,T,H) or None (forward only when both dy and
    dh_n are None).  -> dict with y, h_n and, with a backward, dx, dw_ih, dw_hh, db_ih, db_hh, dh0 (float64 tensors)."""
    f64 = lambda t: None if t is None else torch.as_tensor(t).detach().double().cpu()
    x, w_ih, w_hh, b_ih, b_hh, h0, dy, dh_n = map(f64, (x, w_ih, w_hh, b_ih, b_hh, h0, dy, dh_n))
    B, T, I = x.shape
    H = w_hh.shape[1]
    rw_ih, rw_hh = mround(w_ih, mtype), mround(w_hh, mtype)
    gi = mround(x, mtype) @ rw_ih.t() + b_ih                       # (B,T,3H)
    h = torch.zeros(B, H, dtype=torch.float64) if h0 is None else h0
    order = range(T - 1, -1, -1) if reverse else range(T)
    y = torch.empty(B, T, H, dtype=torch.float64)
    sv = {}
    for t in order:
        gh = mround(h, mtype) @ rw_hh.t() + b_hh
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, t, 2 * H:] + r * gh[:, 2 * H:])
        sv[t] = (r, z, n, gh[:, 2 * H:], h)
        h = (1.0 - z) * n + z * h
        y[:, t] = h
    out = {"y": y, "h_n": h}
    if dy is None and dh_n is None:
        return out
    dh = torch.zeros(B, H, dtype=torch.float64) if dh_n is None else dh_n.clone()
    dgi = torch.empty(B, T, 3 * H, dtype=torch.float64)
    dgh = torch.empty(B, T, 3 * H, dtype=torch.float64)
    hp_all = torch.empty(B, T, H, dtype=torch.float64)
    for t in reversed(list(order)):
        r, z, n, hn, hp = sv[t]
        if dy is not None:
            dh = dh + dy[:, t]
        dan = dh * (1.0 - z) * (1.0 - n * n)
        dar = dan * hn * r * (1.0 - r)
        daz = dh * (hp - n) * z * (1.0 - z)
        dgi[:, t] = torch.cat([dar, daz, dan], 1)
        dgh[:, t] = torch.cat([dar, daz, dan * r], 1)
        hp_all[:, t] = hp
        dh = dh * z + mround(dgh[:, t], mtype) @ rw_hh
    rgi, rgh = mround(dgi.reshape(B * T, 3 * H), mtype), mround(dgh.reshape(B * T, 3 * H), mtype)
    out.update(dh0=dh, db_ih=dgi.sum((0, 1)), db_hh=dgh.sum((0, 1)),
               dw_hh=rgh.t() @ mround(hp_all.reshape(B * T, H), mtype),
               dw_ih=rgi.t() @ mround(x.reshape(B * T, I), mtype),
               dx=(rgi @ rw_ih).reshape(B, T, I))
    return out
