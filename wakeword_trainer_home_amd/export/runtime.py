"""``QuantizedCNNSmall``, ``QuantizedTCN``, ``QuantizedResNet18``, ``QuantizedLSTM``, ``QuantizedCRNN`` and ``QuantizedMobileNetV3``: an
int8 bundle on the device, run with integer arithmetic only (``ww_q8_cnn_small_fwd``, ``ww_tq8_tcn_fwd``, ``ww_rq8_resnet18_fwd``,
``ww_lq8_lstm_fwd``, ``ww_cq8_crnn_fwd``, ``ww_mq8_mobilenetv3_fwd``)."""
import numpy as np
import torch
import torch.nn as nn

from .. import _native as nat
from .bundle import check_bundle
from .reference import CONVS, LSTM_DIRS, LSTM_HIDDEN, mbv3_blocks, resnet_blocks, tcn_blocks


def effective_bias(q_b: np.ndarray, q_w: np.ndarray, z_in: int) -> np.ndarray:
    """q_b - z_in * sum(q_w) per output channel, wrapped to int32: what the kernels add to sum q_w q_in (include/wwhip.h)."""
    return (q_b.astype(np.int64) - int(z_in) * q_w.astype(np.int64).sum(axis=1)).astype(np.int32)


def device_conv(arrays: dict, name: str, z_in: int):
    """The four tensors of one conv as the kernels read them: w (taps,64) for the 3x3 convs, (64,64) [out][in] for 1x1."""
    w = arrays[name + ".w"]
    return (np.ascontiguousarray(w if name.startswith("pw") else w.T), effective_bias(arrays[name + ".b"], w, z_in),
            arrays[name + ".m"], arrays[name + ".sh"])


def _padded_channels(arrays: dict, name: str, bias_eff: np.ndarray, cpo: int):
    """Effective bias, mult and shift of a conv over ``cpo`` padded output channels: the pad channels get 0, 2^30 and 31, so they
    come out as the zero point of the tensor written."""
    cout = len(bias_eff)
    bias, mult, shift = np.zeros(cpo, np.int32), np.full(cpo, 2 ** 30, np.int32), np.full(cpo, 31, np.int32)
    bias[:cout] = bias_eff
    mult[:cout], shift[:cout] = arrays[name + ".m"], arrays[name + ".sh"]
    return bias, mult, shift


CONV4 = ("w", "b", "m", "sh")
LAYER8 = ("ih_w", "ih_b", "ih_m", "ih_sh", "hh_w", "hh_b", "hh_m", "hh_sh")
RNN_TAIL = ("fc.w", "fc.b", "fc.scale", "tab.sigmoid", "tab.tanh")


class _QuantizedNet(nn.Module):
    """The frame of the six int8 networks: the bundle's tensors as buffers in the order of the native pointer table (``None``
    where a layer has none), the table rebuilt when a buffer moves, one workspace per input size, and ``forward`` as one native
    call on the current stream, no host synchronisation.  Eval only, no parameters.  A subclass names its architecture, builds
    ``io``, adds its tensors, and says how a workspace is sized (``WORKSPACE``) and which entry point runs (``FORWARD``)."""

    hip_backed = True
    WORKSPACE = FORWARD = None
    FREE_T = False            # the bundle takes any T >= 1: workspaces are kept per (B, T), a few of them, not per B
    ALIGN_INPUT = True        # ww_q8_quantize reads float4: a misaligned input is copied (ww_tq8_quantize_bt takes any address)
    REFUSE_STRIDED = False    # a non-contiguous input is refused, not copied

    def __init__(self, header: dict, arrays: dict, architecture):
        super().__init__()
        check_bundle(header, arrays)
        name, kind = type(self).__name__, header["kind"]
        if architecture is None:
            if kind != "int8":
                raise ValueError(f"{name} needs an int8 bundle, got kind {kind!r}")
        elif kind != "int8" or header["architecture"] != architecture:
            raise ValueError(f"{name} needs an int8 {architecture} bundle, got kind {kind!r} of {header['architecture']!r}")
        self.header = dict(header)
        self.num_classes = int(header["num_classes"])
        if not self.FREE_T:                                        # the bundle is for ONE feature shape: another is refused
            self.feature_shape = tuple(int(v) for v in header["feature_shape"])
        self._names = []
        self._tab, self._key, self._ws = None, None, {}

    def _add(self, name, a):
        if a is None:
            setattr(self, name, None)
        else:
            self.register_buffer(name, torch.from_numpy(np.ascontiguousarray(a).copy()), persistent=False)
        self._names.append(name)

    def _add_group(self, prefix, tensors, suffixes=CONV4):
        for suffix, a in zip(suffixes, tensors):
            self._add(f"{prefix}_{suffix}", a)

    def _add_tail(self, arrays, keys=("fc.w", "fc.b", "fc.scale")):
        for key in keys:
            self._add(key.replace(".", "_"), arrays[key])

    def _group(self, prefix, suffixes=CONV4):
        return tuple(getattr(self, f"{prefix.replace('.', '_')}_{s}") for s in suffixes)

    def conv(self, name):
        """(w, bias_eff, mult, shift) of one conv by its name in the bundle, for the per-layer entry points."""
        return self._group(name)

    def layer(self, k):
        """(w_ih, bias_eff, mult, shift, w_hh, bias, mult, shift) of recurrent layer ``k``, for the per-kernel entry points."""
        return self._group(f"l{k}", LAYER8)

    def _finish(self, nptr):
        assert len(self._names) == nptr
        self.eval()

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError(f"{type(self).__name__} is an inference network: it has no training mode")
        return super().train(False)

    def _table(self):
        tensors = [getattr(self, n) for n in self._names]
        key = tuple(None if t is None else t.data_ptr() for t in tensors)
        if self._key != key:
            self._tab, self._key = nat.ptr_array(tensors), key
        return self._tab

    def workspace(self, B, T=None):
        """The uint8 workspace of the last forward at this batch size -- and, where T is free, this length; the network's
        ``_native.*_workspace_views`` names its parts."""
        return self._ws[B if T is None else (B, T)]

    def _workspace_bytes(self, B, F, T):
        return self.WORKSPACE(B, F, T)

    def _run(self, tab, x, ws, logits):
        self.FORWARD(tab, self.io, x, ws, logits)

    def _features(self, x):
        """The input as (B,F,T), or a ValueError: here the rule of a bundle made for ONE feature shape."""
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3 or tuple(x.shape[1:]) != self.feature_shape:
            raise ValueError(f"this int8 bundle is for features of shape {self.feature_shape}, got {tuple(x.shape)}")
        return x

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self._features(x)
        if x.dtype != torch.float32:
            raise ValueError(f"features must be float32, got {x.dtype}")
        if self.FREE_T and (x.shape[0] < 1 or x.shape[2] < 1):
            raise ValueError(f"an empty batch or sequence: {tuple(x.shape)}")
        if self.REFUSE_STRIDED:
            nat._dev(x, self.fc_w)
        if not x.is_contiguous() or (self.ALIGN_INPUT and x.data_ptr() % 16):
            x = x.clone(memory_format=torch.contiguous_format)
        B, F, T = x.shape
        dev = nat._dev(x, self.fc_w)
        key = (B, T) if self.FREE_T else B
        ws = self._ws.get(key)
        if ws is None or ws.device != dev:
            if self.FREE_T and len(self._ws) >= 4:                 # T is free: keep a few shapes, not every one ever seen
                self._ws.clear()
            ws = self._ws[key] = torch.empty(self._workspace_bytes(B, F, T), dtype=torch.uint8, device=dev)
        logits = torch.empty((B, self.num_classes), dtype=torch.float32, device=dev)
        self._run(self._table(), x, ws, logits)
        return logits


def device_tcn_conv(arrays: dict, name: str, z_in: int):
    """The four tensors of one TCN conv as ``ww_tq8_conv1d_fwd`` reads them: w (Cpo,k,Cpi) [out][tap][in], zero in its pad rows
    and columns; the effective bias, mult and shift (Cpo), the pad channels 0, 2^30 and 31 (they come out as -128)."""
    w = arrays[name + ".w"]
    cout, cin, k = w.shape
    cpo, cpi = nat.tq8_pad(cout), nat.tq8_pad(cin)
    wd = np.zeros((cpo, k, cpi), np.int8)
    wd[:cout, :, :cin] = w.transpose(0, 2, 1)
    return (wd,) + _padded_channels(arrays, name, effective_bias(arrays[name + ".b"], w.reshape(cout, cin * k), z_in), cpo)


class QuantizedTCN(_QuantizedNet):
    """An int8 ``TCNWakeword`` bundle on the device: ``forward((B,1,F,T) float32) -> (B,num_classes) float32`` is one native
    call (``ww_tq8_tcn_fwd``).  The bundle is for ONE feature shape (the pooling multiplier holds 1/T)."""

    ALIGN_INPUT = False
    FORWARD = staticmethod(nat.tq8_tcn_fwd)

    def __init__(self, header: dict, arrays: dict):
        super().__init__(header, arrays, "TCNWakeword")
        tcn = header["tcn"]
        self.input_size, self.kernel_size = int(tcn["input_size"]), int(tcn["kernel_size"])
        self.channels = [int(c) for c in tcn["num_channels"]]
        if self.channels[-1] > 1024:
            raise ValueError(f"the pooling kernel sums at most 1024 channels, got {self.channels[-1]}")
        z_x = int(arrays["input_zero"][0])
        self.io = io = nat.Tq8Io(float(arrays["input_scale"][0]), z_x, int(arrays["pool.m"][0]), int(arrays["pool.sh"][0]),
                                 len(self.channels), self.kernel_size, self.input_size, self.num_classes)
        for i, cin, cout, _, down in tcn_blocks(tcn):
            z_in = z_x if i == 0 else -128
            io.channels[i] = cout
            io.add_mult[i], io.add_shift[i] = int(arrays[f"b{i}.add.m"][0]), int(arrays[f"b{i}.add.sh"][0])
            if not down:
                io.skip_mult[i], io.skip_shift[i] = int(arrays[f"b{i}.skip.m"][0]), int(arrays[f"b{i}.skip.sh"][0])
            for conv, z in (("conv1", z_in), ("conv2", -128), ("down", z_in)):
                self._add_group(f"b{i}_{conv}", device_tcn_conv(arrays, f"b{i}.{conv}", z) if conv != "down" or down else (None,) * 4)
        self._add_tail(arrays)
        self._finish(nat.TQ8_BLOCK_NPTR * len(self.channels) + 3)

    def conv(self, block, name):
        """(w, bias_eff, mult, shift) of ``conv1`` / ``conv2`` / ``down`` of a block, for the per-layer entry points."""
        return self._group(f"b{block}_{name}")

    def _workspace_bytes(self, B, F, T):
        return nat.tq8_tcn_workspace_bytes(B, F, T, self.channels)


def device_resnet_conv(arrays: dict, name: str, z_in: int):
    """The four tensors of one ResNet conv as the kernels read them: w (Cout,k*k,Cin) [out][tap][in] -- the stem's (64,64)
    [channel][tap], its 49 taps padded with zero weights to one 64-deep K chunk -- and the effective bias, mult and shift (Cout)."""
    w = arrays[name + ".w"]
    cout, cin, k, _ = w.shape
    if name == "stem":
        wd = np.zeros((64, 64), np.int8)
        wd[:, :49] = w.reshape(64, 49)
    else:
        wd = w.transpose(0, 2, 3, 1).reshape(cout, k * k, cin)
    return (np.ascontiguousarray(wd), effective_bias(arrays[name + ".b"], w.reshape(cout, -1), z_in), arrays[name + ".m"],
            arrays[name + ".sh"])


class QuantizedResNet18(_QuantizedNet):
    """An int8 ``ResNet18Wakeword`` bundle on the device: ``forward((B,1,F,T) float32) -> (B,num_classes) float32`` is one native
    call (``ww_rq8_resnet18_fwd``).  The bundle is for ONE feature shape (the pooling multiplier holds 1/HW)."""

    WORKSPACE, FORWARD = staticmethod(nat.rq8_resnet18_workspace_bytes), staticmethod(nat.rq8_resnet18_fwd)

    def __init__(self, header: dict, arrays: dict):
        super().__init__(header, arrays, "ResNet18Wakeword")
        z_x = int(arrays["input_zero"][0])
        self.io = io = nat.Rq8Io(float(arrays["input_scale"][0]), z_x, int(arrays["pool.m"][0]), int(arrays["pool.sh"][0]),
                                 self.num_classes)
        self._add_group("stem", device_resnet_conv(arrays, "stem", z_x))
        self.blocks = [name for name, *_ in resnet_blocks()]
        for i, (name, _, _, _, down) in enumerate(resnet_blocks()):
            io.res_mult[i], io.res_shift[i] = int(arrays[name + ".res.m"][0]), int(arrays[name + ".res.sh"][0])
            for conv in ("conv1", "conv2", "down"):
                self._add_group(f"{name.replace('.', '_')}_{conv}",
                                device_resnet_conv(arrays, f"{name}.{conv}", -128) if conv != "down" or down else (None,) * 4)
        self._add_tail(arrays)
        self._finish(nat.RQ8_NPTR)                                 # conv(): ``stem`` or ``l{s}.{b}.conv1|conv2|down``


def device_rnn_layer(arrays: dict, layer: int, num_directions: int, z_in: int):
    """The eight tensors of one LSTM or GRU layer as ``ww_lq8_proj_fwd`` and ``ww_lq8_lstm_layer_fwd`` / ``ww_cq8_gru_layer_fwd``
    read them, the directions stacked (forward first): w_ih (nd*G, Kp), G = 512 or 384 gate rows, with zero pad columns, its
    EFFECTIVE bias, mult, shift; w_hh (nd*G, 128), the law's q_bh, mult, shift.  The layout does not depend on the gate count."""
    names = [f"l{layer}.{d}" for d in LSTM_DIRS[:num_directions]]
    w_ih = np.concatenate([arrays[n + ".ih.w"] for n in names])
    wd = np.zeros((w_ih.shape[0], nat.tq8_pad(w_ih.shape[1])), np.int8)
    wd[:, :w_ih.shape[1]] = w_ih
    cat = lambda key: np.concatenate([arrays[n + key] for n in names])       # noqa: E731
    return (wd, effective_bias(cat(".ih.b"), w_ih, z_in), cat(".ih.m"), cat(".ih.sh"),
            np.ascontiguousarray(cat(".hh.w")), cat(".hh.b"), cat(".hh.m"), cat(".hh.sh"))


device_lstm_layer = device_gru_layer = device_rnn_layer


class QuantizedLSTM(_QuantizedNet):
    """An int8 ``LSTMWakeword`` bundle on the device: ``forward`` takes (B,1,F,T) float32 features or (B,T,F) sequences, any
    T >= 1, and returns (B,num_classes) float32 from one native call (``ww_lq8_lstm_fwd``).  The bundle is for one
    ``input_size``; it is not tied to one T (its law holds no 1/T)."""

    FREE_T = True
    ALIGN_INPUT = False
    FORWARD = staticmethod(nat.lq8_lstm_fwd)

    def __init__(self, header: dict, arrays: dict):
        super().__init__(header, arrays, "LSTMWakeword")
        e = header["lstm"]
        self.input_size, self.num_layers = int(e["input_size"]), int(e["num_layers"])
        self.num_directions, self.hidden_size = 2 if e["bidirectional"] else 1, LSTM_HIDDEN
        z_x = int(arrays["input_zero"][0])
        self.io = nat.Lq8Io(float(arrays["input_scale"][0]), z_x, self.input_size, self.num_layers, self.num_directions,
                            self.num_classes)
        for k in range(self.num_layers):
            self._add_group(f"l{k}", device_rnn_layer(arrays, k, self.num_directions, z_x if k == 0 else 0), LAYER8)
        self._add_tail(arrays, RNN_TAIL)
        self._finish(nat.LQ8_LAYER_NPTR * self.num_layers + nat.LQ8_TAIL_NPTR)

    def _features(self, x):
        F = self.input_size
        if x.dim() == 4 and x.shape[1] == 1 and x.shape[2] == F:
            return x[:, 0]
        if x.dim() == 3 and x.shape[2] == F:
            return x.transpose(1, 2)                               # (B,T,F) sequences -> (B,F,T): the kernel's input form
        raise ValueError(f"this int8 bundle is for features of shape (B,1,{F},T) or sequences (B,T,{F}), got {tuple(x.shape)}")

    def _workspace_bytes(self, B, F, T):
        return nat.lq8_lstm_workspace_bytes(B, T, F, self.num_layers, self.num_directions)


class QuantizedCRNN(_QuantizedNet):
    """An int8 ``CRNNWakeword`` bundle on the device: ``forward((B,1,F,T) float32) -> (B,num_classes) float32`` is one native
    call (``ww_cq8_crnn_fwd``).  The bundle is for ONE number of feature rows F (the frequency-mean multiplier holds 1/H'); it
    takes any T >= 1."""

    FREE_T = True
    REFUSE_STRIDED = True
    FORWARD = staticmethod(nat.cq8_crnn_fwd)

    def __init__(self, header: dict, arrays: dict):
        super().__init__(header, arrays, "crnn")
        e = header["crnn"]
        self.feature_rows, self.num_layers = int(header["feature_shape"][0]), int(e["num_layers"])
        self.num_directions, self.hidden_size = 2 if e["bidirectional"] else 1, LSTM_HIDDEN
        z_x = int(arrays["input_zero"][0])
        self.io = nat.Cq8Io(float(arrays["input_scale"][0]), z_x, int(arrays["fmean.m"][0]), int(arrays["fmean.sh"][0]),
                            self.num_layers, self.num_directions, self.num_classes)
        front = {k[len("front."):]: v for k, v in arrays.items() if k.startswith("front.")}
        for name in CONVS:
            self._add_group(name, device_conv(front, name, z_x if name == "stem" else -128))
        for k in range(self.num_layers):
            self._add_group(f"l{k}", device_rnn_layer(arrays, k, self.num_directions, -128 if k == 0 else 0), LAYER8)
        self._add_tail(arrays, RNN_TAIL)
        self._finish(nat.CQ8_CONV_NPTR + nat.CQ8_LAYER_NPTR * self.num_layers + nat.CQ8_TAIL_NPTR)

    def _features(self, x):
        F = self.feature_rows
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3 or x.shape[1] != F:
            raise ValueError(f"this int8 bundle is for features of shape (B,1,{F},T), got {tuple(x.shape)}")
        return x

    def _workspace_bytes(self, B, F, T):
        return nat.cq8_crnn_workspace_bytes(B, F, T, self.num_layers, self.num_directions)


def device_mbv3_conv(arrays: dict, name: str, z_in: int, kind: str):
    """The tensors of one MobileNetV3 conv as the ``ww_mq8_*`` kernels read them, channel counts padded to 64 (``kind``: ``pw`` --
    w (Cpo, Cpi) [out][in] -- or ``dw`` / ``stem`` -- w (taps, Cp) [tap][channel]): zero weights in the pad rows and columns; the
    effective bias, mult and shift, the pad channels 0, 2^30 and 31 (they come out as the output's zero point); the layer's
    Hardswish table, or None."""
    w = arrays[name + ".w"]
    cout = w.shape[0]
    cpo = nat.tq8_pad(cout)
    if kind == "pw":
        wd = np.zeros((cpo, nat.tq8_pad(w.shape[1])), np.int8)
        wd[:cout, :w.shape[1]] = w
    else:
        wd = np.zeros((w.shape[1], cpo), np.int8)
        wd[:, :cout] = w.T
    return (wd,) + _padded_channels(arrays, name, effective_bias(arrays[name + ".b"], w, z_in), cpo) + (arrays.get(name + ".tab"),)


class QuantizedMobileNetV3(_QuantizedNet):
    """An int8 ``MobileNetV3Wakeword`` bundle on the device: ``forward((B,1,F,T) float32) -> (B,num_classes) float32`` is one native
    call (``ww_mq8_mobilenetv3_fwd``).  The bundle is for ONE feature shape (its pooling multipliers hold 1/HW)."""

    CONV5 = CONV4 + ("tab",)
    WORKSPACE, FORWARD = staticmethod(nat.mq8_mobilenetv3_workspace_bytes), staticmethod(nat.mq8_mobilenetv3_fwd)

    def __init__(self, header: dict, arrays: dict):
        super().__init__(header, arrays, "mobilenetv3")
        one = lambda key: int(arrays[key][0])        # noqa: E731
        self.io = io = nat.Mq8Io(float(arrays["input_scale"][0]), one("input_zero"), self.num_classes, one("stem.zu"), one("stem.zo"),
                                 one("last.zu"), one("last.zo"), one("cls0.zu"), one("cls0.zo"), one("pool.m"), one("pool.sh"))
        self._add_group("stem", device_mbv3_conv(arrays, "stem", io.in_zero, "stem"), self.CONV5)
        z = io.stem_zo
        self.blocks = mbv3_blocks(*self.feature_shape)
        for i, b in enumerate(self.blocks):
            p = f"b{i}."
            for layer, kind in (("expand", "pw"), ("dw", "dw")):
                if layer == "expand" and not b["expand"]:
                    self._add_group(f"b{i}_expand", (None,) * 5, self.CONV5)
                    continue
                self._add_group(f"b{i}_{layer}", device_mbv3_conv(arrays, p + layer, z, kind), self.CONV5)
                z = one(p + layer + ".zo") if b["hs"] else -128
                if b["hs"]:
                    getattr(io, "exp_zu" if layer == "expand" else "dw_zu")[i] = one(p + layer + ".zu")
                    getattr(io, "exp_zo" if layer == "expand" else "dw_zo")[i] = z
            for fc in ("fc1", "fc2"):
                self._add_group(f"b{i}_{fc}", [arrays[f"{p}{fc}.{s}"] if b["se"] else None for s in CONV4])
            if b["se"]:
                io.sepool_mult[i], io.sepool_shift[i] = one(p + "pool.m"), one(p + "pool.sh")
                io.gate_mult[i], io.gate_shift[i] = one(p + "gate.m"), one(p + "gate.sh")
            self._add_group(f"b{i}_project", device_mbv3_conv(arrays, p + "project", z, "pw")[:4])
            if b["res"]:
                io.res_mult[i], io.res_shift[i] = one(p + "res.m"), one(p + "res.sh")
            z = 0
        self._add_group("last", device_mbv3_conv(arrays, "last", 0, "pw"), self.CONV5)
        self._add_group("cls0", device_mbv3_conv(arrays, "cls0", io.last_zo, "pw"), self.CONV5)
        self._add_tail(arrays)
        self._finish(nat.MQ8_NPTR)

    def conv(self, name):
        """(w, bias_eff, mult, shift, tab) of ``stem``, ``b{i}.expand|dw|project``, ``last`` or ``cls0``; (w, q_b, mult, shift) of
        ``b{i}.fc1|fc2``: what the per-layer entry points take.  A layer without a table has ``None`` there."""
        return tuple(getattr(self, f"{name.replace('.', '_')}_{s}", None) for s in self.CONV5)


class QuantizedCNNSmall(_QuantizedNet):
    """An int8 ``cnn_small`` bundle on the device: ``forward((B,1,F,T) float32) -> (B,2) float32`` is one native call
    (``ww_q8_cnn_small_fwd``).  The bundle is for ONE feature shape (the pooling multiplier holds 1/HW).  ``form``: ``"pair"`` runs
    depthwise and pointwise as two launches, ``"fused"`` as one; both give the same bits.  The header's ``architecture`` is not
    checked: an int8 bundle of no other known architecture is taken for cnn_small's."""

    FORMS = {"pair": nat.Q8_PAIR, "fused": nat.Q8_FUSED}
    DEFAULT_FORM = "fused"
    WORKSPACE = staticmethod(nat.q8_cnn_small_workspace_bytes)

    def __init__(self, header: dict, arrays: dict, form: str = None):
        super().__init__(header, arrays, None)
        self.num_classes = 2
        self.set_form(form or self.DEFAULT_FORM)
        z_x = int(arrays["input_zero"][0])
        self.io = nat.Q8Io(float(arrays["input_scale"][0]), z_x, int(arrays["pool.m"][0]), int(arrays["pool.sh"][0]))
        for name in CONVS:
            self._add_group(name, device_conv(arrays, name, z_x if name == "stem" else -128))
        self._add_tail(arrays)
        self._finish(nat.Q8_NPTR)

    def set_form(self, form: str):
        if form not in self.FORMS:
            raise ValueError(f"form must be one of {sorted(self.FORMS)}, got {form!r}")
        self.form = form
        return self

    def _run(self, tab, x, ws, logits):
        nat.q8_cnn_small_fwd(tab, self.io, x, ws, logits, self.FORMS[self.form])
