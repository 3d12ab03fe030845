"""``LSTMWakeword`` with the constructor, ``forward`` contract and ``state_dict`` keys of the reference class
(``src/models/architectures.py``: ``lstm.weight_ih_l0`` ... ``lstm.bias_hh_l1_reverse``, ``fc.1.weight``, ``fc.1.bias``), running on
``ww_lstm_*`` (one persistent MFMA kernel per layer for both directions), ``ww_dropout_bt`` and the MFMA ``fc``.  Like
``GRUWakeword`` it also accepts the (B,1,F,T) feature batches the Trainer produces.  Hidden size 128 (the reference default) is
the implemented size; dropout masks come from the GRU's Philox streams (inter-layer ``1 + k``, head 15)."""
import math

import torch
import torch.nn as nn

from .. import _native as nat
from .flat_buckets import FlatBuckets, grad_slot
from .heads import MFMALinear
from .recurrent import _HiddenDropout


class _LSTMStackFn(torch.autograd.Function):
    """All layers and directions of the stack; parameters arrive flat in nn.LSTM's ``_flat_weights`` order.  A bidirectional
    layer is ONE recurrent launch per pass (ww_lstm_bidir_*: gridDim.y = 2), eager and under graph capture alike."""

    @staticmethod
    def forward(ctx, x, mod, step, *params):
        L, nd, H = mod.num_layers, mod.num_directions, mod.hidden_size
        B, T, _ = x.shape
        dev = x.device
        p = mod.dropout if (mod.training and L > 1) else 0.0
        inputs, workspaces, h_last = [x], [], []
        cur = x
        for k in range(L):
            out = torch.empty((B, T, nd * H), dtype=torch.float32, device=dev)
            ws_k = [nat.lstm_workspace(B, T, cur.shape[2], H, dev) for _ in range(nd)]
            pk = [params[4 * (k * nd + d):4 * (k * nd + d) + 4] for d in range(nd)]
            if nd == 2:
                h_k, _ = nat.lstm_bidir_fwd(cur, pk, out, ws_k, mode=mod.mode)
            else:
                h_k = [nat.lstm_fwd(cur, *pk[0], out, ws_k[0], mode=mod.mode)[0]]
            workspaces.append(ws_k)
            if k == L - 1:
                h_last = h_k
            if p > 0 and k + 1 < L:
                out = nat.dropout_bt(out, p, seed=mod.dropout_seed, step=step, sample_offset=mod.sample_offset, stream_id=1 + k)
            cur = out
            if k + 1 < L:
                inputs.append(cur)
        ctx.mod, ctx.step, ctx.p = mod, step, p
        ctx.inputs, ctx.workspaces = inputs, workspaces
        ctx.param_objs = params            # the Parameter objects themselves: their gradient-bucket slots (grad_slot)
        ctx.save_for_backward(*params)
        return torch.cat(h_last, dim=1) if nd == 2 else h_last[0]

    @staticmethod
    def backward(ctx, dh):
        mod, params = ctx.mod, ctx.saved_tensors
        L, nd, H = mod.num_layers, mod.num_directions, mod.hidden_size
        grads = [None] * len(params)
        dh = dh.contiguous()
        dev = dh.device
        dy = None                                  # gradient of layer k's (dropped-out) output, (B,T,nd*H)
        for k in reversed(range(L)):
            xin = ctx.inputs[k]
            need_dx = k > 0 or ctx.needs_input_grad[0]
            dx = torch.empty_like(xin) if need_dx else None
            dhn = [dh[:, d * H:(d + 1) * H].contiguous() if k == L - 1 else None for d in range(nd)]
            idx = [4 * (k * nd + d) for d in range(nd)]
            # gradients born in their slots of the model's flat bucket (autograd adopts them without reading), so the sums of the
            # weight-gradient / bias partials can wait for the ONE flush at the end of the backward pass
            slots = [tuple(grad_slot(q) for q in ctx.param_objs[i:i + 4]) for i in idx]
            have = all(s_ is not None for d_ in slots for s_ in d_)
            if nd == 2:
                g = nat.lstm_bidir_bwd(xin, [params[i:i + 2] for i in idx], dy, dhn, ctx.workspaces[k], dx=dx, mode=mod.mode,
                                       outs=slots if have else None, defer=have and nat.defer_begin(dev))
            else:
                g = [nat.lstm_bwd(xin, params[idx[0]], params[idx[0] + 1], dy, dhn[0], None, ctx.workspaces[k][0], dx=dx,
                                  mode=mod.mode)[:4]]
            for d in range(nd):
                grads[idx[d]:idx[d] + 4] = g[d]
            dy = dx
            if k > 0 and ctx.p > 0:                # backward of the inter-layer dropout: the same mask on the gradient
                dy = nat.dropout_bt(dy, ctx.p, seed=mod.dropout_seed, step=ctx.step, sample_offset=mod.sample_offset,
                                    stream_id=k)
        ctx.workspaces = ctx.inputs = None
        return (dy if ctx.needs_input_grad[0] else None, None, None) + tuple(grads)


class NativeLSTM(nn.Module):
    """Parameter container with nn.LSTM's names/initialisation; ``forward(x (B,T,I)) -> h_n of the last layer (B, nd*H)``."""

    def __init__(self, input_size, hidden_size=128, num_layers=2, bidirectional=True, dropout=0.0, dropout_seed=0,
                 mode="fp32"):
        super().__init__()
        self.mode = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}.get(mode, mode)
        nat.act_code(self.mode)
        if hidden_size != 128:
            raise nat.NativeError(f"the HIP LSTM kernels implement hidden_size == 128 (the reference default), got {hidden_size}")
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.num_directions = 2 if bidirectional else 1
        self.dropout, self.dropout_seed = float(dropout), dropout_seed
        self.dropout_step, self.sample_offset = 0, 0
        k = 1.0 / math.sqrt(hidden_size)
        self._names = []
        for layer in range(num_layers):
            for d in range(self.num_directions):
                sfx = "_reverse" if d == 1 else ""
                isz = input_size if layer == 0 else hidden_size * self.num_directions
                for name, shape in ((f"weight_ih_l{layer}{sfx}", (4 * hidden_size, isz)),
                                    (f"weight_hh_l{layer}{sfx}", (4 * hidden_size, hidden_size)),
                                    (f"bias_ih_l{layer}{sfx}", (4 * hidden_size,)), (f"bias_hh_l{layer}{sfx}", (4 * hidden_size,))):
                    self.register_parameter(name, nn.Parameter(torch.empty(shape).uniform_(-k, k)))     # nn.LSTM.reset_parameters
                    self._names.append(name)

    def forward(self, x):
        if not x.is_cuda:
            raise nat.NativeError("the LSTM runs on hand-written HIP kernels only: the input is on "
                                  f"'{x.device}', need an MI355X ('cuda') device -- there is no CPU fallback")
        if x.dim() != 3 or x.shape[2] != self.input_size:
            raise ValueError(f"expected input (B,T,{self.input_size}), got {tuple(x.shape)}")
        nat.defer_reset(x.device)              # (a previous backward pass that raised midway must not leave its queue behind)
        step = self.dropout_step
        if self.training and self.dropout > 0 and self.num_layers > 1:
            self.dropout_step += 1
        return _LSTMStackFn.apply(x.float().contiguous(), self, step, *[getattr(self, n) for n in self._names])


class LSTMWakeword(FlatBuckets, nn.Module):
    """The reference's LSTMWakeword: ``fc(dropout(cat(h_n[-2], h_n[-1])))`` (bidirectional) or ``fc(dropout(h_n[-1]))``.  Its
    parameters live in one flat bucket (fused clip + optimizer, one all-reduce, graph-capturable step)."""
    hip_backed = True      # every op is a HIP kernel of this build: the Trainer may run its sync-free step (no host reads)

    def __init__(self, input_size: int = 40, hidden_size: int = 128, num_layers: int = 2, num_classes: int = 2,
                 bidirectional: bool = True, dropout: float = 0.3, dropout_seed: int = 0, mode: str = "fp32"):
        super().__init__()
        self.hidden_size, self.num_layers, self.bidirectional = hidden_size, num_layers, bidirectional
        self.lstm = NativeLSTM(input_size, hidden_size, num_layers, bidirectional, dropout if num_layers > 1 else 0.0,
                               dropout_seed, mode=mode)
        self.lstm.fc_step = 0
        out = hidden_size * 2 if bidirectional else hidden_size
        self.fc = nn.Sequential(_HiddenDropout(dropout, self.lstm), MFMALinear(out, num_classes, mode=mode))

    @property
    def sample_offset(self):
        return self.lstm.sample_offset

    @sample_offset.setter
    def sample_offset(self, v):
        self.lstm.sample_offset = v

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() == 4:                                    # (B,1,F,T) feature batch -> (B,T,F)
            if x.shape[1] != 1:
                raise ValueError(f"expected (B,1,F,T) features or (B,T,F) sequences, got {tuple(x.shape)}")
            x = x[:, 0].transpose(1, 2)
        self.lstm.fc_step = self.lstm.dropout_step          # one Philox step per training forward, shared by all masks
        h = self.lstm(x.contiguous())
        if self.training and self.lstm.dropout == 0 and self.fc[0].p > 0:
            self.lstm.dropout_step += 1                     # single-layer stacks: the fc dropout alone advances the stream
        return self.fc(h)
