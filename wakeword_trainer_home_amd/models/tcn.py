"""``TCNWakeword`` with the constructor, ``forward`` contract and ``state_dict`` keys of the reference class
(``src/models/architectures.py:270-434``: ``tcn.network.{i}.conv1.weight`` ... ``tcn.network.{i}.downsample.bias``, ``fc.3.weight``,
``fc.3.bias``), running on ``ww_tconv1d_fwd/bwd`` (causal dilated Conv1d as a shifted-row GEMM on the matrix cores),
``ww_dropout_bt``, ``ww_pool_hw_fwd`` and the MFMA ``fc``.  The reference's ``TemporalBlock`` pads both sides by ``(k-1) d``,
convolves twice and keeps the first ``T`` outputs: on those it is a causal convolution whose hidden activation is zero before
``t = 0``, which is what the kernels compute -- in the channels-last ``(B, T, C)`` layout of the recurrent models.  Weights keep
``nn.Conv1d``'s ``(Cout, Cin, k)`` layout, so checkpoints interchange with the reference.  Like ``GRUWakeword`` it also accepts the
``(B,1,F,T)`` feature batches the Trainer produces.

One ``TemporalBlock`` is ONE autograd node of 3 convolution launches forward (the last one carries "add the residual, then
ReLU") plus two ``ww_dropout_bt`` passes in training; its backward reads every ReLU and dropout mask off the saved outputs
(``output != 0``), so nothing but the block's three activations is kept.

``storage="bf16" | "fp16"`` (opt-in; it must equal the matrix ``mode``) keeps every (B, T, C) activation tensor -- the input features,
each block's h1, h2 and out -- and every gradient of one in that type in HBM (the ``_st`` entry points: ``ww_tconv1d_st_fwd/bwd``,
``ww_dropout_bt_st``, ``ww_add_relu_st_fwd``, ``ww_seq_round_st``, ``ww_mean_hw_st_fwd/bwd``).  Arithmetic stays fp32 and a value is
rounded exactly where a tensor is stored; parameters, their gradients, the pooled vector and the head stay fp32, so the state dict is
the same.  The default, ``storage="fp32"``, is the path above, bit for bit."""
import ctypes

import torch
import torch.nn as nn

from .. import _native as nat
from .flat_buckets import FlatBuckets, grad_slot
from .heads import MFMALinear
from .mobilenet import _PoolFn
from .recurrent import _HiddenDropout
from .resnet import _MeanFn
from .storage import _storage

MAX_BLOCKS = 8


def _bt_stream(stream_id):
    """The 4-bit stream field of ww_dropout_bt for a TCN stream id.  The Philox counter word of that law is
    ``TAG_DROPOUT<<24 | stream_id<<20 | t<<8 | c>>2`` (``oracle.gru.dropout_bt_mask``): an id of 16..31 sets the tag's own bit once
    more, so it names the same counter word as ``id - 16``, which is the value the kernel takes."""
    if not 16 <= stream_id < 32:
        raise ValueError(f"TCN dropout stream ids are 16..31, got {stream_id}")
    return stream_id & 15


def _drop_scale(p):
    """ww_dropout_bt's own factor: 1 / (1 - p) of the float32 p, rounded to float32."""
    return ctypes.c_float(1.0 / (1.0 - ctypes.c_float(p).value)).value if p > 0 else 1.0


def _wide(mod):
    return mod.storage is torch.float32


def _conv_fwd(mod, x, w, b, d, relu=False, residual=None):
    if _wide(mod):
        return nat.tconv1d_fwd(x, w, b, d, relu=relu, residual=residual, mode=mod.mode)
    return nat.tconv1d_st_fwd(x, w, b, d, relu=relu, residual=residual)


def _conv_bwd(mod, x, w, dy, d, **kw):
    if _wide(mod):
        return nat.tconv1d_bwd(x, w, dy, d, mode=mod.mode, **kw)
    return nat.tconv1d_st_bwd(x, w, dy, d, **kw)


def _input(mod, x):
    """A stand-alone layer's or block's input in the module's storage type."""
    return x.float().contiguous() if _wide(mod) else x.to(mod.storage).contiguous()


class _ConvFn(torch.autograd.Function):
    """A stand-alone NativeCausalConv1d: y = [relu](conv(x) + bias)."""

    @staticmethod
    def forward(ctx, x, weight, bias, mod):
        y = _conv_fwd(mod, x, weight, bias, mod.dilation, relu=mod.relu)
        ctx.save_for_backward(x, weight, y if mod.relu else None)
        ctx.mod = mod
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        mod = ctx.mod
        sw, sb = grad_slot(mod.weight), grad_slot(mod.bias)
        defer = sw is not None and sb is not None and nat.defer_begin(x.device)
        dx, dw, db = _conv_bwd(mod, x, weight, dy.contiguous(), mod.dilation, y=y, need_dx=ctx.needs_input_grad[0],
                               dw_out=sw if defer else None, db_out=sb if defer else None, defer=defer)
        return dx, dw, db, None


class NativeCausalConv1d(nn.Module):
    """``nn.Conv1d(in_channels, out_channels, kernel_size, padding=(k-1) d, dilation=d)`` cut to its first T outputs, on
    (B, T, C) channels-last sequences.  ``weight`` (Cout, Cin, k) and ``bias`` (Cout) are nn.Conv1d's, with its initialisation.
    ``storage``: the type of x, y and their gradients (see the module text)."""

    def __init__(self, in_channels, out_channels, kernel_size, dilation=1, relu=False, mode="fp32", storage="fp32"):
        super().__init__()
        mode, storage = _storage(mode, storage)
        if storage is not torch.float32 and (in_channels % 8 or out_channels % 8):
            raise nat.NativeError(f"16-bit activation storage takes channel counts that are multiples of 8, got "
                                  f"{in_channels} -> {out_channels}")
        if in_channels < 4 or out_channels < 4 or in_channels % 4 or out_channels % 4:
            raise nat.NativeError(f"the HIP causal Conv1d kernels take channel counts that are positive multiples of 4, got "
                                  f"{in_channels} -> {out_channels}")
        if not 1 <= kernel_size <= 8 or dilation < 1:
            raise nat.NativeError(f"the HIP causal Conv1d kernels take 1 <= kernel_size <= 8 and dilation >= 1, got "
                                  f"{kernel_size}, {dilation}")
        ref = nn.Conv1d(in_channels, out_channels, kernel_size, dilation=dilation)          # torch's own initialisation
        self.weight = nn.Parameter(ref.weight.detach().clone())
        self.bias = nn.Parameter(ref.bias.detach().clone())
        self.in_channels, self.out_channels, self.kernel_size, self.dilation = in_channels, out_channels, kernel_size, dilation
        self.relu = bool(relu)
        self.mode, self.storage = mode, storage

    def forward(self, x):
        if not x.is_cuda:
            raise nat.NativeError("NativeCausalConv1d runs on hand-written HIP kernels only: the input is on "
                                  f"'{x.device}', need an MI355X ('cuda') device -- there is no CPU fallback")
        if x.dim() != 3 or x.shape[2] != self.in_channels:
            raise ValueError(f"expected input (B,T,{self.in_channels}), got {tuple(x.shape)}")
        return _ConvFn.apply(_input(self, x), self.weight, self.bias, self)


class _BlockFn(torch.autograd.Function):
    """h1 = drop(relu(conv1(x))); h2 = drop(relu(conv2(h1))); out = relu(h2 + (x | downsample(x))).  Saved: h1, h2, out."""

    @staticmethod
    def forward(ctx, x, blk, step, *params):
        w1, b1, w2, b2 = params[:4]
        net = blk._net[0]
        p = blk.dropout if blk.training else 0.0
        d = blk.dilation

        def drop(h, sid):
            if p <= 0:
                return h
            kw = dict(seed=net.dropout_seed, step=step, sample_offset=net.sample_offset, stream_id=_bt_stream(sid))
            # (16-bit storage: in place -- the convolution's output is read by nothing else)
            return nat.dropout_bt(h, p, **kw) if _wide(blk) else nat.dropout_bt_st(h, p, out=h, **kw)
        h1 = drop(_conv_fwd(blk, x, w1, b1, d, relu=True), blk.stream_ids[0])
        h2 = drop(_conv_fwd(blk, h1, w2, b2, d, relu=True), blk.stream_ids[1])
        if blk.downsample is not None:       # the 1x1 convolution's epilogue adds h2 and applies the block's last ReLU
            out = _conv_fwd(blk, x, params[4], params[5], 1, relu=True, residual=h2)
        else:
            out = nat.add_relu_fwd(h2, x) if _wide(blk) else nat.add_relu_st_fwd(h2, x)
        ctx.blk, ctx.p = blk, p
        ctx.save_for_backward(x, h1, h2, out, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, h1, h2, out, *params = ctx.saved_tensors
        blk, p = ctx.blk, ctx.p
        d = blk.dilation
        scale = _drop_scale(p)
        dout = dout.contiguous()
        need_dx = ctx.needs_input_grad[0]
        mods = [blk.conv1, blk.conv2] + ([blk.downsample] if blk.downsample is not None else [])
        # gradients born in their slots of the model's flat bucket, so the sums of the weight-gradient partials can wait for the
        # ONE flush at the end of the backward pass
        slots = [(grad_slot(m.weight), grad_slot(m.bias)) for m in mods]
        defer = all(s is not None for pair in slots for s in pair) and nat.defer_begin(x.device)
        if not defer:
            slots = [(None, None)] * len(mods)
        grads = [None] * len(params)
        if blk.downsample is not None:       # dsum = dout * [out != 0] feeds the skip and conv2 alike
            dx, grads[4], grads[5] = _conv_bwd(blk, x, params[4], dout, 1, y=out, need_dx=need_dx, dw_out=slots[2][0],
                                               db_out=slots[2][1], defer=defer)
        elif need_dx:
            dx = nat.relu_mask_bwd(dout, out) if _wide(blk) else nat.relu_mask_st_bwd(dout, out)
        else:
            dx = None
        dh1, grads[2], grads[3] = _conv_bwd(blk, h1, params[2], dout, d, y=out, y2=h2, mask_scale=scale, dw_out=slots[1][0],
                                            db_out=slots[1][1], defer=defer)
        dx, grads[0], grads[1] = _conv_bwd(blk, x, params[0], dh1, d, y=h1, mask_scale=scale, need_dx=need_dx, dx=dx,
                                           dw_out=slots[0][0], db_out=slots[0][1], defer=defer)
        return (dx, None, None) + tuple(grads)


class TemporalBlock(nn.Module):
    """The reference's TemporalBlock (stride 1, padding (k-1) d).  ``stream_ids``: the Philox streams of its two dropouts."""

    def __init__(self, in_channels, out_channels, kernel_size, dilation, dropout=0.3, mode="fp32", stream_ids=(16, 17), net=None,
                 storage="fp32"):
        super().__init__()
        st = dict(mode=mode, storage=storage)
        self.conv1 = NativeCausalConv1d(in_channels, out_channels, kernel_size, dilation, relu=True, **st)
        self.conv2 = NativeCausalConv1d(out_channels, out_channels, kernel_size, dilation, relu=True, **st)
        self.downsample = NativeCausalConv1d(in_channels, out_channels, 1, **st) if in_channels != out_channels else None
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        self.dropout, self.dilation, self.mode, self.storage = float(dropout), dilation, self.conv1.mode, self.conv1.storage
        self.stream_ids = tuple(stream_ids)
        for s in self.stream_ids:
            _bt_stream(s)
        # not a submodule: only read for seed / step / sample offset (a block used alone is its own owner)
        self._net = [net if net is not None else self]
        if net is None:
            self.dropout_seed, self.dropout_step, self.sample_offset = 0, 0, 0

    def forward(self, x, step=None):
        if not x.is_cuda:
            raise nat.NativeError("TemporalBlock runs on hand-written HIP kernels only: the input is on "
                                  f"'{x.device}', need an MI355X ('cuda') device -- there is no CPU fallback")
        if x.dim() != 3 or x.shape[2] != self.conv1.in_channels:
            raise ValueError(f"expected input (B,T,{self.conv1.in_channels}), got {tuple(x.shape)}")
        if step is None:
            step = self._net[0].dropout_step
        params = [self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias]
        if self.downsample is not None:
            params += [self.downsample.weight, self.downsample.bias]
        return _BlockFn.apply(_input(self, x), self, step, *params)


class TemporalConvNet(nn.Module):
    """The reference's TemporalConvNet on (B, T, C) sequences: block i has dilation 2^i and the dropout streams 16 + 2i, 17 + 2i."""

    def __init__(self, input_channels=40, num_channels=(64, 128, 256), kernel_size=3, dropout=0.3, dropout_seed=0, mode="fp32",
                 storage="fp32"):
        super().__init__()
        self.mode, self.storage = _storage(mode, storage)
        num_channels = list(num_channels)
        if not 1 <= len(num_channels) <= MAX_BLOCKS:
            raise nat.NativeError(f"the TCN takes 1..{MAX_BLOCKS} blocks (two dropout streams each out of ids 16..31), got {len(num_channels)}")
        self.dropout, self.dropout_seed = float(dropout), dropout_seed
        self.dropout_step, self.sample_offset, self.fc_step = 0, 0, 0
        self.network = nn.Sequential(*[
            TemporalBlock(input_channels if i == 0 else num_channels[i - 1], c, kernel_size, 2 ** i, dropout=dropout, mode=mode,
                          stream_ids=(16 + 2 * i, 17 + 2 * i), net=self, storage=storage) for i, c in enumerate(num_channels)])

    def forward(self, x):
        step = self.dropout_step
        for blk in self.network:
            x = blk(x, step)
        return x


class _TimeMean(nn.Module):
    """``nn.AdaptiveAvgPool1d(1)`` + ``nn.Flatten()`` of the reference head on a (B, T, C) sequence -> (B, C) fp32.  A 16-bit
    sequence goes through ww_mean_hw_st_fwd with HW = T; its gradient is stored as S(dpooled / T)."""

    def forward(self, h):
        return (_PoolFn if h.dtype is torch.float32 else _MeanFn).apply(h[:, :, None, :])


class TCNWakeword(FlatBuckets, nn.Module):
    """The reference's TCNWakeword.  Its parameters live in one flat bucket (fused clip + optimizer, one all-reduce,
    graph-capturable step).  ``forward`` takes (B,1,F,T) feature batches, (B,T,F) or (B,F,T) sequences (module docstring)."""
    hip_backed = True      # every op is a HIP kernel of this build: the Trainer may run its sync-free step (no host reads)

    def __init__(self, input_size: int = 40, num_channels: list = [64, 128, 256], kernel_size: int = 3, num_classes: int = 2,
                 dropout: float = 0.3, dropout_seed: int = 0, mode: str = "fp32", storage: str = "fp32"):
        super().__init__()
        self.input_size = input_size
        self.tcn = TemporalConvNet(input_channels=input_size, num_channels=num_channels, kernel_size=kernel_size, dropout=dropout,
                                   dropout_seed=dropout_seed, mode=mode, storage=storage)
        self.mode, self.storage = self.tcn.mode, self.tcn.storage
        # indices as in the reference: AdaptiveAvgPool1d(1), Flatten(), Dropout(dropout), Linear(num_channels[-1], num_classes)
        self.fc = nn.Sequential(_TimeMean(), nn.Identity(), _HiddenDropout(dropout, self.tcn),
                                MFMALinear(list(num_channels)[-1], num_classes, mode=mode))

    @property
    def sample_offset(self):
        return self.tcn.sample_offset

    @sample_offset.setter
    def sample_offset(self, v):
        self.tcn.sample_offset = v

    def _sequence(self, x):
        """-> (B, T, F).  The reference transposes a 3-D input when size(1) < size(2) and then needs size(1) == input_size, so it
        reads (B,T,F) for T < F and (B,F,T) for T >= F; the same reading wherever its forward runs at all, and (B,T,F) beyond."""
        F = self.input_size
        if x.dim() == 4:
            if x.shape[1] != 1 or x.shape[2] != F:
                raise ValueError(f"expected (B,1,{F},T) features, got {tuple(x.shape)}")
            return x[:, 0].transpose(1, 2)
        if x.dim() == 3 and x.shape[1] == F:
            return x.transpose(1, 2)
        if x.dim() == 3 and x.shape[2] == F:
            return x
        raise ValueError(f"expected (B,1,{F},T) features, (B,T,{F}) or (B,{F},T) sequences, got {tuple(x.shape)}")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        seq = self._sequence(x)
        if not x.is_cuda:
            raise nat.NativeError("TCNWakeword runs on hand-written HIP kernels only: the input is on "
                                  f"'{x.device}', need an MI355X ('cuda') device -- there is no CPU fallback")
        nat.defer_reset(x.device)              # (a previous backward pass that raised midway must not leave its queue behind)
        net = self.tcn
        net.fc_step = net.dropout_step         # one Philox step per training forward, shared by all masks
        if self.storage is torch.float32:
            h = net(seq.float().contiguous())
        elif x.requires_grad:                   # (off the training path: the rounding's gradient through torch's own ops)
            h = net(seq.float().to(self.storage).contiguous())
        else:                                   # one native pass: S(features) as (B, T, F), transposing where the input is (.., F, T)
            h = net(nat.seq_round_st(x.float().contiguous(), self.storage, transposed=not (x.dim() == 3 and seq is x)))
        if self.training and net.dropout > 0:
            net.dropout_step += 1
        return self.fc(h)
