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


def device_tcn_conv(arrays: dict, name: str, z_in: int):
    """The four tensors of one TCN conv as ``ww_tq8_conv1d_fwd`` reads them: w (Cpo,k,Cpi) [out][tap][in], zero in its pad rows
    and columns; the effective bias, mult and shift (Cpo), the pad channels 0, 2^30 and 31 (they come out as -128)."""
    w = arrays[name + ".w"]
    cout, cin, k = w.shape
    cpo, cpi = nat.tq8_pad(cout), nat.tq8_pad(cin)
    wd = np.zeros((cpo, k, cpi), np.int8)
    wd[:cout, :, :cin] = w.transpose(0, 2, 1)
    bias, mult, shift = np.zeros(cpo, np.int32), np.full(cpo, 2 ** 30, np.int32), np.full(cpo, 31, np.int32)
    bias[:cout] = effective_bias(arrays[name + ".b"], w.reshape(cout, cin * k), z_in)
    mult[:cout], shift[:cout] = arrays[name + ".m"], arrays[name + ".sh"]
    return wd, bias, mult, shift


class QuantizedTCN(nn.Module):
    """An int8 ``TCNWakeword`` bundle on the device: ``forward((B,1,F,T) float32) -> (B,num_classes) float32`` is one native
    call (``ww_tq8_tcn_fwd``), no host synchronisation.  Eval only, no parameters.  The bundle is for ONE feature shape (the
    pooling multiplier holds 1/T): another shape is refused."""

    hip_backed = True

    def __init__(self, header: dict, arrays: dict):
        super().__init__()
        check_bundle(header, arrays)
        if header["kind"] != "int8" or header["architecture"] != "TCNWakeword":
            raise ValueError(f"QuantizedTCN needs an int8 TCNWakeword bundle, got kind {header['kind']!r} of "
                             f"{header['architecture']!r}")
        self.header = dict(header)
        self.feature_shape = tuple(int(v) for v in header["feature_shape"])
        self.num_classes = int(header["num_classes"])
        tcn = header["tcn"]
        self.input_size, self.kernel_size = int(tcn["input_size"]), int(tcn["kernel_size"])
        self.channels = [int(c) for c in tcn["num_channels"]]
        if self.channels[-1] > 1024:
            raise ValueError(f"the pooling kernel sums at most 1024 channels, got {self.channels[-1]}")
        z_x = int(arrays["input_zero"][0])
        io = nat.Tq8Io(float(arrays["input_scale"][0]), z_x, int(arrays["pool.m"][0]), int(arrays["pool.sh"][0]),
                       len(self.channels), self.kernel_size, self.input_size, self.num_classes)
        self._names = []
        for i, cin, cout, _, down in tcn_blocks(tcn):
            z_in = z_x if i == 0 else -128
            io.channels[i] = cout
            io.add_mult[i], io.add_shift[i] = int(arrays[f"b{i}.add.m"][0]), int(arrays[f"b{i}.add.sh"][0])
            if not down:
                io.skip_mult[i], io.skip_shift[i] = int(arrays[f"b{i}.skip.m"][0]), int(arrays[f"b{i}.skip.sh"][0])
            for conv, z in (("conv1", z_in), ("conv2", -128), ("down", z_in)):
                tensors = device_tcn_conv(arrays, f"b{i}.{conv}", z) if conv != "down" or down else (None,) * 4
                for suffix, a in zip(("w", "b", "m", "sh"), tensors):
                    self._add(f"b{i}_{conv}_{suffix}", a)
        for key in ("fc.w", "fc.b", "fc.scale"):
            self._add(key.replace(".", "_"), arrays[key])
        assert len(self._names) == nat.TQ8_BLOCK_NPTR * len(self.channels) + 3
        self.io = io
        self._tab, self._key, self._ws = None, None, {}
        self.eval()

    def _add(self, name, a):
        if a is None:
            setattr(self, name, None)
        else:
            self.register_buffer(name, torch.from_numpy(np.ascontiguousarray(a).copy()), persistent=False)
        self._names.append(name)

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("QuantizedTCN is an inference network: it has no training mode")
        return super().train(False)

    def conv(self, block, name):
        """(w, bias_eff, mult, shift) of ``conv1`` / ``conv2`` / ``down`` of a block, for the per-layer entry points."""
        return tuple(getattr(self, f"b{block}_{name}_{s}") for s in ("w", "b", "m", "sh"))

    def _table(self):
        tensors = [getattr(self, n) for n in self._names]
        key = tuple(None if t is None else t.data_ptr() for t in tensors)
        if self._key != key:
            self._tab, self._key = nat.ptr_array(tensors), key
        return self._tab

    def workspace(self, B):
        """The uint8 workspace of the last forward at this batch size (``_native.tq8_workspace_views`` names its parts)."""
        return self._ws[B]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3 or tuple(x.shape[1:]) != self.feature_shape:
            raise ValueError(f"this int8 bundle is for features of shape {self.feature_shape}, got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"features must be float32, got {x.dtype}")
        if not x.is_contiguous():
            x = x.contiguous()
        B, (F, T) = x.shape[0], self.feature_shape
        dev = nat._dev(x, self.fc_w)
        ws = self._ws.get(B)
        if ws is None or ws.device != dev:
            ws = self._ws[B] = torch.empty(nat.tq8_tcn_workspace_bytes(B, F, T, self.channels), dtype=torch.uint8, device=dev)
        logits = torch.empty((B, self.num_classes), dtype=torch.float32, device=dev)
        nat.tq8_tcn_fwd(self._table(), self.io, x, ws, logits)
        return logits


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


class QuantizedResNet18(nn.Module):
    """An int8 ``ResNet18Wakeword`` bundle on the device: ``forward((B,1,F,T) float32) -> (B,num_classes) float32`` is one native
    call (``ww_rq8_resnet18_fwd``), no host synchronisation.  Eval only, no parameters.  The bundle is for ONE feature shape (the
    pooling multiplier holds 1/HW): another shape is refused."""

    hip_backed = True

    def __init__(self, header: dict, arrays: dict):
        super().__init__()
        check_bundle(header, arrays)
        if header["kind"] != "int8" or header["architecture"] != "ResNet18Wakeword":
            raise ValueError(f"QuantizedResNet18 needs an int8 ResNet18Wakeword bundle, got kind {header['kind']!r} of "
                             f"{header['architecture']!r}")
        self.header = dict(header)
        self.feature_shape = tuple(int(v) for v in header["feature_shape"])
        self.num_classes = int(header["num_classes"])
        z_x = int(arrays["input_zero"][0])
        io = nat.Rq8Io(float(arrays["input_scale"][0]), z_x, int(arrays["pool.m"][0]), int(arrays["pool.sh"][0]), self.num_classes)
        self._names = []
        for suffix, a in zip(("w", "b", "m", "sh"), device_resnet_conv(arrays, "stem", z_x)):
            self._add(f"stem_{suffix}", a)
        self.blocks = [name for name, *_ in resnet_blocks()]
        for i, (name, _, _, _, down) in enumerate(resnet_blocks()):
            io.res_mult[i], io.res_shift[i] = int(arrays[name + ".res.m"][0]), int(arrays[name + ".res.sh"][0])
            for conv in ("conv1", "conv2", "down"):
                tensors = device_resnet_conv(arrays, f"{name}.{conv}", -128) if conv != "down" or down else (None,) * 4
                for suffix, a in zip(("w", "b", "m", "sh"), tensors):
                    self._add(f"{name.replace('.', '_')}_{conv}_{suffix}", a)
        for key in ("fc.w", "fc.b", "fc.scale"):
            self._add(key.replace(".", "_"), arrays[key])
        assert len(self._names) == nat.RQ8_NPTR
        self.io = io
        self._tab, self._key, self._ws = None, None, {}
        self.eval()

    def _add(self, name, a):
        if a is None:
            setattr(self, name, None)
        else:
            self.register_buffer(name, torch.from_numpy(np.ascontiguousarray(a).copy()), persistent=False)
        self._names.append(name)

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("QuantizedResNet18 is an inference network: it has no training mode")
        return super().train(False)

    def conv(self, name):
        """(w, bias_eff, mult, shift) of ``stem`` or ``l{s}.{b}.conv1|conv2|down``, for the per-layer entry points."""
        return tuple(getattr(self, f"{name.replace('.', '_')}_{s}") for s in ("w", "b", "m", "sh"))

    def _table(self):
        tensors = [getattr(self, n) for n in self._names]
        key = tuple(None if t is None else t.data_ptr() for t in tensors)
        if self._key != key:
            self._tab, self._key = nat.ptr_array(tensors), key
        return self._tab

    def workspace(self, B):
        """The uint8 workspace of the last forward at this batch size (``_native.rq8_workspace_views`` names its parts)."""
        return self._ws[B]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3 or tuple(x.shape[1:]) != self.feature_shape:
            raise ValueError(f"this int8 bundle is for features of shape {self.feature_shape}, got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"features must be float32, got {x.dtype}")
        if not x.is_contiguous() or x.data_ptr() % 16:
            x = x.clone(memory_format=torch.contiguous_format)
        B, (F, T) = x.shape[0], self.feature_shape
        dev = nat._dev(x, self.fc_w)
        ws = self._ws.get(B)
        if ws is None or ws.device != dev:
            ws = self._ws[B] = torch.empty(nat.rq8_resnet18_workspace_bytes(B, F, T), dtype=torch.uint8, device=dev)
        logits = torch.empty((B, self.num_classes), dtype=torch.float32, device=dev)
        nat.rq8_resnet18_fwd(self._table(), self.io, x, ws, logits)
        return logits


def device_lstm_layer(arrays: dict, layer: int, num_directions: int, z_in: int):
    """The eight tensors of one LSTM layer as ``ww_lq8_proj_fwd`` and ``ww_lq8_lstm_layer_fwd`` read them, the directions stacked
    (forward first): w_ih (nd*512, Kp) with zero pad columns, its EFFECTIVE bias, mult, shift; w_hh (nd*512, 128), the law's q_bh,
    mult, shift."""
    names = [f"l{layer}.{d}" for d in LSTM_DIRS[:num_directions]]
    w_ih = np.concatenate([arrays[n + ".ih.w"] for n in names])
    wd = np.zeros((w_ih.shape[0], nat.tq8_pad(w_ih.shape[1])), np.int8)
    wd[:, :w_ih.shape[1]] = w_ih
    cat = lambda key: np.concatenate([arrays[n + key] for n in names])       # noqa: E731
    return (wd, effective_bias(cat(".ih.b"), w_ih, z_in), cat(".ih.m"), cat(".ih.sh"),
            np.ascontiguousarray(cat(".hh.w")), cat(".hh.b"), cat(".hh.m"), cat(".hh.sh"))


class QuantizedLSTM(nn.Module):
    """An int8 ``LSTMWakeword`` bundle on the device: ``forward`` takes (B,1,F,T) float32 features or (B,T,F) sequences, any
    T >= 1, and returns (B,num_classes) float32 from one native call (``ww_lq8_lstm_fwd``), no host synchronisation.  Eval only,
    no parameters.  The bundle is for one ``input_size``; it is not tied to one T (its law holds no 1/T)."""

    hip_backed = True

    def __init__(self, header: dict, arrays: dict):
        super().__init__()
        check_bundle(header, arrays)
        if header["kind"] != "int8" or header["architecture"] != "LSTMWakeword":
            raise ValueError(f"QuantizedLSTM needs an int8 LSTMWakeword bundle, got kind {header['kind']!r} of "
                             f"{header['architecture']!r}")
        self.header = dict(header)
        e = header["lstm"]
        self.input_size, self.num_layers = int(e["input_size"]), int(e["num_layers"])
        self.num_directions, self.hidden_size = 2 if e["bidirectional"] else 1, LSTM_HIDDEN
        self.num_classes = int(header["num_classes"])
        z_x = int(arrays["input_zero"][0])
        self.io = nat.Lq8Io(float(arrays["input_scale"][0]), z_x, self.input_size, self.num_layers, self.num_directions,
                            self.num_classes)
        self._names = []
        for k in range(self.num_layers):
            tensors = device_lstm_layer(arrays, k, self.num_directions, z_x if k == 0 else 0)
            for suffix, a in zip(("ih_w", "ih_b", "ih_m", "ih_sh", "hh_w", "hh_b", "hh_m", "hh_sh"), tensors):
                self._add(f"l{k}_{suffix}", a)
        for key in ("fc.w", "fc.b", "fc.scale", "tab.sigmoid", "tab.tanh"):
            self._add(key.replace(".", "_"), arrays[key])
        assert len(self._names) == nat.LQ8_LAYER_NPTR * self.num_layers + nat.LQ8_TAIL_NPTR
        self._tab, self._key, self._ws = None, None, {}
        self.eval()

    def _add(self, name, a):
        self.register_buffer(name, torch.from_numpy(np.ascontiguousarray(a).copy()), persistent=False)
        self._names.append(name)

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("QuantizedLSTM is an inference network: it has no training mode")
        return super().train(False)

    def layer(self, k):
        """(w_ih, bias_eff, mult, shift, w_hh, bias, mult, shift) of layer ``k``, for the per-kernel entry points."""
        return tuple(getattr(self, f"l{k}_{s}") for s in ("ih_w", "ih_b", "ih_m", "ih_sh", "hh_w", "hh_b", "hh_m", "hh_sh"))

    def _table(self):
        tensors = [getattr(self, n) for n in self._names]
        key = tuple(t.data_ptr() for t in tensors)
        if self._key != key:
            self._tab, self._key = nat.ptr_array(tensors), key
        return self._tab

    def workspace(self, B, T):
        """The uint8 workspace of the last forward at this batch size and length (``_native.lq8_workspace_views`` names its
        parts)."""
        return self._ws[(B, T)]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        F = self.input_size
        if x.dim() == 4 and x.shape[1] == 1 and x.shape[2] == F:
            x = x[:, 0]
        elif x.dim() == 3 and x.shape[2] == F:
            x = x.transpose(1, 2)                                  # (B,T,F) sequences -> (B,F,T): the kernel's input form
        else:
            raise ValueError(f"this int8 bundle is for features of shape (B,1,{F},T) or sequences (B,T,{F}), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"features must be float32, got {x.dtype}")
        if x.shape[0] < 1 or x.shape[2] < 1:
            raise ValueError(f"an empty batch or sequence: {tuple(x.shape)}")
        if not x.is_contiguous():
            x = x.contiguous()
        B, T = x.shape[0], x.shape[2]
        dev = nat._dev(x, self.fc_w)
        ws = self._ws.get((B, T))
        if ws is None or ws.device != dev:
            if len(self._ws) >= 4:                                 # T is free: keep a few shapes, not every one ever seen
                self._ws.clear()
            ws = self._ws[(B, T)] = torch.empty(nat.lq8_lstm_workspace_bytes(B, T, F, self.num_layers, self.num_directions),
                                                dtype=torch.uint8, device=dev)
        logits = torch.empty((B, self.num_classes), dtype=torch.float32, device=dev)
        nat.lq8_lstm_fwd(self._table(), self.io, x, ws, logits)
        return logits


def device_gru_layer(arrays: dict, layer: int, num_directions: int, z_in: int):
    """The eight tensors of one GRU layer as ``ww_lq8_proj_fwd`` and ``ww_cq8_gru_layer_fwd`` read them, the directions stacked
    (forward first): w_ih (nd*384, Kp) with zero pad columns, its EFFECTIVE bias, mult, shift; w_hh (nd*384, 128), the law's q_bh,
    mult, shift."""
    return device_lstm_layer(arrays, layer, num_directions, z_in)       # the layout does not depend on the gate count


class QuantizedCRNN(nn.Module):
    """An int8 ``CRNNWakeword`` bundle on the device: ``forward((B,1,F,T) float32) -> (B,num_classes) float32`` is one native
    call (``ww_cq8_crnn_fwd``) on the current stream, no host synchronisation.  Eval only, no parameters.  The bundle is for ONE
    number of feature rows F (the frequency-mean multiplier holds 1/H'); it takes any T >= 1."""

    hip_backed = True

    def __init__(self, header: dict, arrays: dict):
        super().__init__()
        check_bundle(header, arrays)
        if header["kind"] != "int8" or header["architecture"] != "crnn":
            raise ValueError(f"QuantizedCRNN needs an int8 crnn bundle, got kind {header['kind']!r} of {header['architecture']!r}")
        self.header = dict(header)
        e = header["crnn"]
        self.feature_rows, self.num_layers = int(header["feature_shape"][0]), int(e["num_layers"])
        self.num_directions, self.hidden_size = 2 if e["bidirectional"] else 1, LSTM_HIDDEN
        self.num_classes = int(header["num_classes"])
        z_x = int(arrays["input_zero"][0])
        self.io = nat.Cq8Io(float(arrays["input_scale"][0]), z_x, int(arrays["fmean.m"][0]), int(arrays["fmean.sh"][0]),
                            self.num_layers, self.num_directions, self.num_classes)
        front = {k[len("front."):]: v for k, v in arrays.items() if k.startswith("front.")}
        self._names = []
        for name in CONVS:
            for suffix, a in zip(("w", "b", "m", "sh"), device_conv(front, name, z_x if name == "stem" else -128)):
                self._add(f"{name}_{suffix}", a)
        for k in range(self.num_layers):
            tensors = device_gru_layer(arrays, k, self.num_directions, -128 if k == 0 else 0)
            for suffix, a in zip(("ih_w", "ih_b", "ih_m", "ih_sh", "hh_w", "hh_b", "hh_m", "hh_sh"), tensors):
                self._add(f"l{k}_{suffix}", a)
        for key in ("fc.w", "fc.b", "fc.scale", "tab.sigmoid", "tab.tanh"):
            self._add(key.replace(".", "_"), arrays[key])
        assert len(self._names) == nat.CQ8_CONV_NPTR + nat.CQ8_LAYER_NPTR * self.num_layers + nat.CQ8_TAIL_NPTR
        self._tab, self._key, self._ws = None, None, {}
        self.eval()

    def _add(self, name, a):
        self.register_buffer(name, torch.from_numpy(np.ascontiguousarray(a).copy()), persistent=False)
        self._names.append(name)

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("QuantizedCRNN is an inference network: it has no training mode")
        return super().train(False)

    def conv(self, name):
        """(w, bias_eff, mult, shift) of one conv of the front end, for the per-layer entry points."""
        return tuple(getattr(self, f"{name}_{s}") for s in ("w", "b", "m", "sh"))

    def layer(self, k):
        """(w_ih, bias_eff, mult, shift, w_hh, bias, mult, shift) of GRU layer ``k``, for the per-kernel entry points."""
        return tuple(getattr(self, f"l{k}_{s}") for s in ("ih_w", "ih_b", "ih_m", "ih_sh", "hh_w", "hh_b", "hh_m", "hh_sh"))

    def _table(self):
        tensors = [getattr(self, n) for n in self._names]
        key = tuple(t.data_ptr() for t in tensors)
        if self._key != key:
            self._tab, self._key = nat.ptr_array(tensors), key
        return self._tab

    def workspace(self, B, T):
        """The uint8 workspace of the last forward at this batch size and length (``_native.cq8_workspace_views`` names its
        parts)."""
        return self._ws[(B, T)]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        F = self.feature_rows
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3 or x.shape[1] != F:
            raise ValueError(f"this int8 bundle is for features of shape (B,1,{F},T), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"features must be float32, got {x.dtype}")
        if x.shape[0] < 1 or x.shape[2] < 1:
            raise ValueError(f"an empty batch or sequence: {tuple(x.shape)}")
        dev = nat._dev(x, self.fc_w)
        if not x.is_contiguous() or x.data_ptr() % 16:
            x = x.clone(memory_format=torch.contiguous_format)
        B, T = x.shape[0], x.shape[2]
        ws = self._ws.get((B, T))
        if ws is None or ws.device != dev:
            if len(self._ws) >= 4:                                 # T is free: keep a few shapes, not every one ever seen
                self._ws.clear()
            ws = self._ws[(B, T)] = torch.empty(nat.cq8_crnn_workspace_bytes(B, F, T, self.num_layers, self.num_directions),
                                                dtype=torch.uint8, device=dev)
        logits = torch.empty((B, self.num_classes), dtype=torch.float32, device=dev)
        nat.cq8_crnn_fwd(self._table(), self.io, x, ws, logits)
        return logits


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
    bias, mult, shift = np.zeros(cpo, np.int32), np.full(cpo, 2 ** 30, np.int32), np.full(cpo, 31, np.int32)
    bias[:cout] = effective_bias(arrays[name + ".b"], w, z_in)
    mult[:cout], shift[:cout] = arrays[name + ".m"], arrays[name + ".sh"]
    return wd, bias, mult, shift, arrays.get(name + ".tab")


class QuantizedMobileNetV3(nn.Module):
    """An int8 ``MobileNetV3Wakeword`` bundle on the device: ``forward((B,1,F,T) float32) -> (B,num_classes) float32`` is one native
    call (``ww_mq8_mobilenetv3_fwd``) on the current stream, no host synchronisation.  Eval only, no parameters.  The bundle is for
    ONE feature shape (its pooling multipliers hold 1/HW): another shape is refused."""

    hip_backed = True

    def __init__(self, header: dict, arrays: dict):
        super().__init__()
        check_bundle(header, arrays)
        if header["kind"] != "int8" or header["architecture"] != "mobilenetv3":
            raise ValueError(f"QuantizedMobileNetV3 needs an int8 mobilenetv3 bundle, got kind {header['kind']!r} of "
                             f"{header['architecture']!r}")
        self.header = dict(header)
        self.feature_shape = tuple(int(v) for v in header["feature_shape"])
        self.num_classes = int(header["num_classes"])
        one = lambda key: int(arrays[key][0])        # noqa: E731
        io = nat.Mq8Io(float(arrays["input_scale"][0]), one("input_zero"), self.num_classes, one("stem.zu"), one("stem.zo"),
                       one("last.zu"), one("last.zo"), one("cls0.zu"), one("cls0.zo"), one("pool.m"), one("pool.sh"))
        self._names = []
        self._add_conv("stem", device_mbv3_conv(arrays, "stem", io.in_zero, "stem"))
        z = io.stem_zo
        self.blocks = mbv3_blocks(*self.feature_shape)
        for i, b in enumerate(self.blocks):
            p = f"b{i}."
            for layer, kind in (("expand", "pw"), ("dw", "dw")):
                if layer == "expand" and not b["expand"]:
                    self._add_conv(f"b{i}_expand", (None,) * 5)
                    continue
                self._add_conv(f"b{i}_{layer}", device_mbv3_conv(arrays, p + layer, z, kind))
                z = one(p + layer + ".zo") if b["hs"] else -128
                if b["hs"]:
                    getattr(io, "exp_zu" if layer == "expand" else "dw_zu")[i] = one(p + layer + ".zu")
                    getattr(io, "exp_zo" if layer == "expand" else "dw_zo")[i] = z
            for fc in ("fc1", "fc2"):
                for s in ("w", "b", "m", "sh"):
                    self._add(f"b{i}_{fc}_{s}", arrays[f"{p}{fc}.{s}"] if b["se"] else None)
            if b["se"]:
                io.sepool_mult[i], io.sepool_shift[i] = one(p + "pool.m"), one(p + "pool.sh")
                io.gate_mult[i], io.gate_shift[i] = one(p + "gate.m"), one(p + "gate.sh")
            self._add_conv(f"b{i}_project", device_mbv3_conv(arrays, p + "project", z, "pw")[:4])
            if b["res"]:
                io.res_mult[i], io.res_shift[i] = one(p + "res.m"), one(p + "res.sh")
            z = 0
        self._add_conv("last", device_mbv3_conv(arrays, "last", 0, "pw"))
        self._add_conv("cls0", device_mbv3_conv(arrays, "cls0", io.last_zo, "pw"))
        for key in ("fc.w", "fc.b", "fc.scale"):
            self._add(key.replace(".", "_"), arrays[key])
        assert len(self._names) == nat.MQ8_NPTR
        self.io = io
        self._tab, self._key, self._ws = None, None, {}
        self.eval()

    def _add(self, name, a):
        if a is None:
            setattr(self, name, None)
        else:
            self.register_buffer(name, torch.from_numpy(np.ascontiguousarray(a).copy()), persistent=False)
        self._names.append(name)

    def _add_conv(self, name, tensors):
        for suffix, a in zip(("w", "b", "m", "sh", "tab"), tensors):
            self._add(f"{name}_{suffix}", a)

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("QuantizedMobileNetV3 is an inference network: it has no training mode")
        return super().train(False)

    def conv(self, name):
        """(w, bias_eff, mult, shift, tab) of ``stem``, ``b{i}.expand|dw|project``, ``last`` or ``cls0``; (w, q_b, mult, shift) of
        ``b{i}.fc1|fc2``: what the per-layer entry points take."""
        return tuple(getattr(self, f"{name.replace('.', '_')}_{s}", None) for s in ("w", "b", "m", "sh", "tab"))

    def _table(self):
        tensors = [getattr(self, n) for n in self._names]
        key = tuple(None if t is None else t.data_ptr() for t in tensors)
        if self._key != key:
            self._tab, self._key = nat.ptr_array(tensors), key
        return self._tab

    def workspace(self, B):
        """The uint8 workspace of the last forward at this batch size (``_native.mq8_workspace_views`` names its parts)."""
        return self._ws[B]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3 or tuple(x.shape[1:]) != self.feature_shape:
            raise ValueError(f"this int8 bundle is for features of shape {self.feature_shape}, got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"features must be float32, got {x.dtype}")
        if not x.is_contiguous() or x.data_ptr() % 16:
            x = x.clone(memory_format=torch.contiguous_format)
        B, (F, T) = x.shape[0], self.feature_shape
        dev = nat._dev(x, self.fc_w)
        ws = self._ws.get(B)
        if ws is None or ws.device != dev:
            ws = self._ws[B] = torch.empty(nat.mq8_mobilenetv3_workspace_bytes(B, F, T), dtype=torch.uint8, device=dev)
        logits = torch.empty((B, self.num_classes), dtype=torch.float32, device=dev)
        nat.mq8_mobilenetv3_fwd(self._table(), self.io, x, ws, logits)
        return logits


class QuantizedCNNSmall(nn.Module):
    """``forward((B,1,F,T) float32 on the device) -> (B,2) float32``: one native call, no host synchronisation.

    Eval only, no parameters.  The bundle is for ONE feature shape (the pooling multiplier holds 1/HW): another shape is
    refused.  ``form``: ``"pair"`` runs depthwise and pointwise as two launches, ``"fused"`` as one; both give the same bits.
    """

    hip_backed = True
    FORMS = {"pair": nat.Q8_PAIR, "fused": nat.Q8_FUSED}
    DEFAULT_FORM = "fused"

    def __init__(self, header: dict, arrays: dict, form: str = None):
        super().__init__()
        check_bundle(header, arrays)
        if header["kind"] != "int8":
            raise ValueError(f"QuantizedCNNSmall needs an int8 bundle, got kind {header['kind']!r}")
        self.header = dict(header)
        self.feature_shape = tuple(int(v) for v in header["feature_shape"])
        self.num_classes = 2
        self.set_form(form or self.DEFAULT_FORM)
        z_x = int(arrays["input_zero"][0])
        self.io = nat.Q8Io(float(arrays["input_scale"][0]), z_x, int(arrays["pool.m"][0]), int(arrays["pool.sh"][0]))
        self._names = []
        for name in CONVS:
            for suffix, a in zip(("w", "b", "m", "sh"), device_conv(arrays, name, z_x if name == "stem" else -128)):
                self._add(f"{name}_{suffix}", a)
        for key in ("fc.w", "fc.b", "fc.scale"):
            self._add(key.replace(".", "_"), arrays[key])
        assert len(self._names) == nat.Q8_NPTR
        self._tab, self._key, self._ws = None, None, {}
        self.eval()

    def _add(self, name, a):
        self.register_buffer(name, torch.from_numpy(np.ascontiguousarray(a).copy()), persistent=False)
        self._names.append(name)

    def set_form(self, form: str):
        if form not in self.FORMS:
            raise ValueError(f"form must be one of {sorted(self.FORMS)}, got {form!r}")
        self.form = form
        return self

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("QuantizedCNNSmall is an inference network: it has no training mode")
        return super().train(False)

    def conv(self, name):
        """(w, bias_eff, mult, shift) of one conv, for the per-layer entry points."""
        return tuple(getattr(self, f"{name}_{s}") for s in ("w", "b", "m", "sh"))

    def _table(self):
        tensors = [getattr(self, n) for n in self._names]
        key = tuple(t.data_ptr() for t in tensors)
        if self._key != key:
            self._tab, self._key = nat.ptr_array(tensors), key
        return self._tab

    def workspace(self, B):
        """The uint8 workspace of the last forward at this batch size (``_native.q8_workspace_views`` names its parts)."""
        return self._ws[B]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3 or tuple(x.shape[1:]) != self.feature_shape:
            raise ValueError(f"this int8 bundle is for features of shape {self.feature_shape}, got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"features must be float32, got {x.dtype}")
        if not x.is_contiguous() or x.data_ptr() % 16:
            x = x.clone(memory_format=torch.contiguous_format)
        B, (F, T) = x.shape[0], self.feature_shape
        dev = nat._dev(x, self.fc_w)
        ws = self._ws.get(B)
        if ws is None or ws.device != dev:
            ws = self._ws[B] = torch.empty(nat.q8_cnn_small_workspace_bytes(B, F, T), dtype=torch.uint8, device=dev)
        logits = torch.empty((B, 2), dtype=torch.float32, device=dev)
        nat.q8_cnn_small_fwd(self._table(), self.io, x, ws, logits, self.FORMS[self.form])
        return logits
