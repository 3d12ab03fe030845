"""The reference's export panel (``src/export/onnx_exporter.py``) without ONNX: neither an ONNX writer nor a runtime exists
on the build machine, so ``export`` writes self-describing bundles (``bundle.py``) instead -- fp32, fp16 (weights only, as
the reference's ``QFloat16`` call) and int8 (``cnn_small``, ``crnn``, ``mobilenetv3``, ``TCNWakeword``, ``ResNet18Wakeword`` and
``LSTMWakeword``; the law is DESIGN.md "Export") -- and the int8 bundle runs on the device with integer arithmetic
(``runtime.QuantizedCNNSmall``, ``runtime.QuantizedTCN``, ``runtime.QuantizedResNet18``, ``runtime.QuantizedLSTM``,
``runtime.QuantizedCRNN``, ``runtime.QuantizedMobileNetV3``).  Names,
signatures, result keys and failure behaviour are the reference's; ``ONNXExporter``, ``export_model_to_onnx``, ``validate_onnx_model`` and ``benchmark_onnx_model`` stay as
aliases.  Parity with onnxruntime's ``quantize_dynamic`` is not claimed."""
import logging
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Callable, Dict, Iterable, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from .. import _native as nat
from .bundle import STATE_PREFIX, BundleError, check_bundle, float_arrays, load_bundle, make_header, write_bundle
from .quantize import (QuantizationError, check_crnn_args, check_lstm_args, check_tcn_args, quantize_cnn_small, quantize_crnn,
                       quantize_lstm, quantize_mobilenetv3, quantize_resnet18, quantize_tcn)
from .reference import CONVS, mbv3_range_names
from .runtime import QuantizedCNNSmall, QuantizedCRNN, QuantizedLSTM, QuantizedMobileNetV3, QuantizedResNet18, QuantizedTCN

logger = logging.getLogger(__name__)


@dataclass
class ExportConfig:
    """The reference's fields and defaults (``onnx_exporter.py:25-34``).  ``opset_version``, ``dynamic_batch`` and ``optimize``
    are recorded in the bundle's header and otherwise inert: a bundle has no opset, takes any batch size, and there is no
    graph to optimise.  ``verbose`` logs the calibrated ranges."""
    output_path: Path
    opset_version: int = 14
    dynamic_batch: bool = True
    quantize_fp16: bool = False
    quantize_int8: bool = False
    optimize: bool = True
    verbose: bool = False


_FACTORY_NAMES = {"CNNSmallWakeword": "cnn_small", "MobileNetV3Wakeword": "mobilenetv3", "CRNNWakeword": "crnn",
                  "GRUWakeword": "gru"}


def _architecture(model: nn.Module) -> str:
    """The factory's name of the model's class (what ``load_exported_model`` builds it from), else the class name."""
    if getattr(model, "features_only", False):
        return type(model).__name__
    return _FACTORY_NAMES.get(type(model).__name__, type(model).__name__)


def _state_numpy(model: nn.Module) -> Dict[str, np.ndarray]:
    return {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


def _calibration_batch(x, dev, feature_extractor, F, T=None, sequences=False):
    """One calibration batch as float32 (B,1,F,T) features on the device: waveforms (B,N) go through ``feature_extractor``, (B,F,T)
    gets its channel dimension, and another shape is refused.  ``T``: ``None`` for any length.  ``sequences``: a 3-dim batch that
    was given as such is (B,T,F) sequences and stays as it is (the LSTM)."""
    x = torch.as_tensor(x).to(dev)
    waveforms = x.dim() == 2
    if waveforms:
        if feature_extractor is None:
            raise QuantizationError("calibration waveforms need a feature_extractor")
        x = feature_extractor(x)
    if x.dim() == 3 and (waveforms or not sequences):
        x = x[:, None]
    if sequences:
        ok = (x.dim() == 4 and x.shape[1] == 1 and x.shape[2] == F) or (x.dim() == 3 and x.shape[2] == F)
        if not ok or x.numel() == 0:
            raise QuantizationError(f"calibration batch of shape {tuple(x.shape)}: expected (B,1,{F},T) or (B,T,{F})")
        return x.float()
    if x.dim() != 4 or tuple(x.shape[1:3]) != (1, F) or (x.shape[3] != T if T is not None else x.shape[3] < 1):
        raise QuantizationError(f"calibration batch of shape {tuple(x.shape)}: expected (B,1,{F},{'T' if T is None else T})")
    return x.float().contiguous()


def _calibrate_conv_stack(model, batches, feature_shape, dev, feature_extractor, whole=None):
    """The loop ``calibrate_cnn_small`` and ``calibrate_crnn`` share, over a ``CNNSmallWakeword`` conv stack in eval mode: the
    input's minimum and maximum and the maximum of every conv's post-ReLU output, through the model's own per-layer entry points
    with ``training = 0``.  ``feature_shape``: (F, T), T ``None`` for any length.  One more maximum per batch: that of ``whole(x)``
    (a forward of the model itself, run before the layers) or, without ``whole``, that of the pooled vector.
    -> (lo, hi, a_max (9), that maximum, samples), tensors on the device."""
    F, T = feature_shape
    convs = [(model.stem.conv, model.stem.bn)]
    for blk in model.blocks:
        convs += [(blk.dw, blk.dw_bn), (blk.pw, blk.pw_bn)]
    scratch = nat.layer_scratch(dev)
    lo = torch.full((), float("inf"), device=dev)
    hi = torch.full((), float("-inf"), device=dev)
    a_max = torch.full((len(convs),), float("-inf"), device=dev)
    t_max = torch.full((), float("-inf"), device=dev)
    seen = 0
    with torch.no_grad():
        for x in batches:
            x = _calibration_batch(x, dev, feature_extractor, F, T)
            lo, hi = torch.minimum(lo, x.min()), torch.maximum(hi, x.max())
            if whole is not None:
                t_max = torch.maximum(t_max, whole(x).max())
            # built per batch, after ``whole``: a model's first forward may move its parameters into a flat bucket (FlatBuckets),
            # and these structs hold their addresses
            bns = [nat.make_bn(bn.weight, bn.bias, bn.running_mean, bn.running_var, 0.1, bn.eps, training=False) for _, bn in convs]
            y = ss = mr = None
            for i, ((conv, _), bn) in enumerate(zip(convs, bns)):
                if i == 0:
                    y, ss, mr = nat.conv_stem_fwd(x, conv.weight, bn, scratch)
                elif i % 2:
                    y, ss, mr = nat.dwconv3x3_fwd(y, ss, conv.weight, bn, scratch)
                else:
                    y, ss, mr = nat.pwconv1x1_fwd(y, ss, conv.weight, bn, scratch)
                a_max[i] = torch.maximum(a_max[i], torch.relu(y * ss[:64] + ss[64:]).max())
            if whole is None:
                t_max = torch.maximum(t_max, (nat.gap_fwd(y, ss, mr)[:, 0, :] / float(y.shape[1] * y.shape[2])).max())
            seen += x.shape[0]
    if seen == 0:
        raise QuantizationError("the calibration data is empty")
    return lo, hi, a_max, t_max, seen


def calibrate_cnn_small(model, batches: Iterable[torch.Tensor], feature_shape, device, feature_extractor=None) -> dict:
    """Ranges of the fp32 model in eval mode over the calibration batches: the input's minimum and maximum, the maximum of
    every conv's post-ReLU output and of the pooled vector.  Runs the model's own per-layer entry points with
    ``training = 0``; the maxima are torch reductions on the device and come to the host once, at the end."""
    dev = torch.device(device)
    lo, hi, a_max, p_max, seen = _calibrate_conv_stack(model, batches, tuple(feature_shape), dev, feature_extractor)
    return {"x_min": float(lo), "x_max": float(hi), "a_max": [float(v) for v in a_max.cpu()], "p_max": float(p_max),
            "samples": seen}


def crnn_entry(model) -> dict:
    """The header's ``crnn`` entry of a ``CRNNWakeword``: what its constructor needs besides ``num_classes``."""
    return {"hidden_size": int(model.rnn.hidden_size), "num_layers": int(model.rnn.num_layers),
            "bidirectional": bool(model.rnn.bidirectional)}


def calibrate_crnn(model, batches: Iterable[torch.Tensor], feature_rows, device, feature_extractor=None) -> dict:
    """Ranges of the fp32 ``CRNNWakeword`` in eval mode over the calibration batches: the input's minimum and maximum, the nine
    conv maxima of ``model.front`` (through the per-layer entry points ``calibrate_cnn_small`` uses) and ``f_max``, the maximum
    of ``model.front``'s output sequence.  The GRU stack has fixed scales.  T may differ from batch to batch.  Torch reductions
    on the device and one read-back."""
    dev = torch.device(device)
    front = model.front
    was_training = front.training
    front.eval()
    try:
        lo, hi, a_max, f_max, seen = _calibrate_conv_stack(front, batches, (int(feature_rows), None), dev, feature_extractor, front)
    finally:
        front.train(was_training)
    got = torch.cat([lo[None], hi[None], a_max, f_max[None]]).cpu().tolist()                    # the one read-back
    return {"x_min": got[0], "x_max": got[1], "a_max": got[2:11], "f_max": got[11], "samples": seen}


def tcn_entry(model) -> dict:
    """The header's ``tcn`` entry of a ``TCNWakeword``: what its constructor needs besides ``num_classes``."""
    blocks = list(model.tcn.network)
    return {"input_size": int(model.input_size), "num_channels": [int(b.conv1.out_channels) for b in blocks],
            "kernel_size": int(blocks[0].conv1.kernel_size)}


def calibrate_tcn(model, batches: Iterable[torch.Tensor], feature_shape, device, feature_extractor=None) -> dict:
    """Ranges of the fp32 ``TCNWakeword`` in eval mode over the calibration batches: the input's minimum and maximum, per block
    the maxima of h1, h2 and the block output (``a_max``, three per block), and that of the pooled vector.  Runs the model's own
    layer entry points (``ww_tconv1d_fwd``, ``ww_add_relu_fwd``, its time mean) on fp32 activations, no dropout; the maxima are
    torch reductions on the device and come to the host once, at the end."""
    F, T = feature_shape
    dev = torch.device(device)
    blocks = list(model.tcn.network)
    lo = torch.full((), float("inf"), device=dev)
    hi = torch.full((), float("-inf"), device=dev)
    a_max = torch.full((3 * len(blocks),), float("-inf"), device=dev)
    p_max = torch.full((), float("-inf"), device=dev)
    seen = 0
    with torch.no_grad():
        for x in batches:
            x = _calibration_batch(x, dev, feature_extractor, F, T)
            lo, hi = torch.minimum(lo, x.min()), torch.maximum(hi, x.max())
            h = x[:, 0].transpose(1, 2).contiguous()
            for i, blk in enumerate(blocks):
                d, mode = blk.dilation, blk.mode
                h1 = nat.tconv1d_fwd(h, blk.conv1.weight, blk.conv1.bias, d, relu=True, mode=mode)
                h2 = nat.tconv1d_fwd(h1, blk.conv2.weight, blk.conv2.bias, d, relu=True, mode=mode)
                if blk.downsample is not None:
                    h = nat.tconv1d_fwd(h, blk.downsample.weight, blk.downsample.bias, 1, relu=True, residual=h2, mode=mode)
                else:
                    h = nat.add_relu_fwd(h2, h)
                for j, t in enumerate((h1, h2, h)):
                    a_max[3 * i + j] = torch.maximum(a_max[3 * i + j], t.max())
            p_max = torch.maximum(p_max, model.fc[0](h).max())
            seen += x.shape[0]
    if seen == 0:
        raise QuantizationError("the calibration data is empty")
    return {"x_min": float(lo), "x_max": float(hi), "a_max": [float(v) for v in a_max.cpu()], "p_max": float(p_max),
            "samples": seen}


def calibrate_resnet18(model, batches: Iterable[torch.Tensor], feature_shape, device, feature_extractor=None) -> dict:
    """Ranges of the ``ResNet18Wakeword`` in eval mode, on fp32 activations, over the calibration batches: the input's minimum and
    maximum, the stem's post-ReLU maximum, per block the maxima of h1 and of the block output, max |ds| of the three downsample
    outputs, and the pooled vector's maximum.  Runs the model's own layer entry points (``ww_conv2d_stem_fwd``, ``ww_bn_act_fwd``
    with running statistics, ``ww_maxpool3x3s2_fwd``, ``ww_conv2d_fwd``, ``ww_add_relu_fwd``, ``ww_pool_hw_fwd``); the ranges are
    torch reductions on the device and come to the host once, at the end."""
    F, T = feature_shape
    dev = torch.device(device)
    net = model.resnet
    blocks = [blk for i in range(4) for blk in getattr(net, f"layer{i + 1}")]

    def bn(mod, y, act):
        bnp = nat.make_bn(mod.weight, mod.bias, mod.running_mean, mod.running_var, momentum=mod.momentum, eps=mod.eps, training=False)
        return nat.bn_act_fwd(y, bnp, act, y.shape[-1])[0]
    lo = torch.full((), float("inf"), device=dev)
    hi = torch.full((), float("-inf"), device=dev)
    m = {k: torch.full((n,), float("-inf"), device=dev) for k, n in (("stem", 1), ("h1", 8), ("ds", 3), ("out", 8), ("p", 1))}
    seen = 0
    with torch.no_grad():
        for x in batches:
            x = _calibration_batch(x, dev, feature_extractor, F, T)
            lo, hi = torch.minimum(lo, x.min()), torch.maximum(hi, x.max())
            a = bn(net.bn1, nat.conv2d_stem_fwd(x[:, 0].contiguous(), net.conv1.weight, net.conv1.stride), nat.LIN_RELU)
            m["stem"][0] = torch.maximum(m["stem"][0], a.max())
            h = nat.maxpool3x3s2_fwd(a)
            n_ds = 0
            for i, blk in enumerate(blocks):
                h1 = bn(blk.bn1, nat.conv2d_fwd(h, blk.conv1.weight, blk.stride, mode=blk.mode), nat.LIN_RELU)
                o2 = bn(blk.bn2, nat.conv2d_fwd(h1, blk.conv2.weight, 1, mode=blk.mode), nat.LIN_NONE)
                if blk.downsample is not None:
                    idn = bn(blk.downsample[1], nat.conv2d_fwd(h, blk.downsample[0].weight, blk.stride, mode=blk.mode), nat.LIN_NONE)
                    m["ds"][n_ds] = torch.maximum(m["ds"][n_ds], idn.abs().max())
                    n_ds += 1
                else:
                    idn = h
                h = nat.add_relu_fwd(o2, idn)
                m["h1"][i], m["out"][i] = torch.maximum(m["h1"][i], h1.max()), torch.maximum(m["out"][i], h.max())
            B, H, W, Cn = h.shape
            m["p"][0] = torch.maximum(m["p"][0], nat.pool_hw_fwd(h.reshape(B, H * W, Cn)).max())
            seen += x.shape[0]
    if seen == 0:
        raise QuantizationError("the calibration data is empty")
    got = torch.cat([lo[None], hi[None]] + [m[k] for k in ("stem", "h1", "ds", "out", "p")]).cpu().tolist()      # the one read-back
    return {"x_min": got[0], "x_max": got[1], "stem_max": got[2], "h1_max": got[3:11], "ds_max": got[11:14], "out_max": got[14:22],
            "p_max": got[22], "samples": seen}


def calibrate_mobilenetv3(model, batches: Iterable[torch.Tensor], feature_shape, device, feature_extractor=None) -> dict:
    """Ranges of the fp32 ``MobileNetV3Wakeword`` in eval mode over the calibration batches: the input's minimum and maximum and
    ``ranges``, {name: [min, max]} over ``reference.mbv3_range_names()`` -- every conv's output, the Hardswish layers' pre-activations
    (``<layer>.u``), each squeeze-excitation's hidden vector, each block's output, the head's hidden vector.  Runs the model's own
    eval entry points (``ww_im2col3x3s2`` + ``ww_linear_mfma_fwd`` for the stem, ``ww_dwconv_nhwc_fwd``, ``ww_linear_mfma_fwd`` for
    the 1x1 convs and the Linears, ``ww_bn_act_fwd`` with running statistics -- ``LIN_NONE`` where the pre-activation is wanted,
    Hardswish then being a torch op --, ``ww_pool_hw_fwd``, ``ww_scale_bc_fwd``); the ranges are torch reductions on the device
    and come to the host once, at the end."""
    F, T = feature_shape
    dev = torch.device(device)
    net = model.mobilenet
    names = mbv3_range_names()
    lo = torch.full((len(names) + 1,), float("inf"), device=dev)
    hi = torch.full((len(names) + 1,), float("-inf"), device=dev)
    at = {n: i + 1 for i, n in enumerate(names)}

    def see(name, t):
        i = at[name] if name else 0
        lo[i], hi[i] = torch.minimum(lo[i], t.min()), torch.maximum(hi[i], t.max())
        return t

    def cba(mod, h, name, out_name=None, residual=None):
        """one ConvBNAct in eval mode, its ranges recorded -> its output"""
        conv, bn = mod[0], mod[1]
        if mod.stem:
            B, _, H, W = h.shape
            y = nat.linear_mfma_fwd(nat.im2col3x3s2(h.reshape(B, H, W).contiguous()), conv.weight.reshape(conv.weight.shape[0], 9), None,
                                    mode=mod.mode).reshape(B, (H + 1) // 2, (W + 1) // 2, -1)
        elif mod.depthwise:
            y = nat.dwconv_nhwc_fwd(h.contiguous(), conv.weight.contiguous(), conv.k, conv.stride)
        else:
            y = nat.linear_mfma_fwd(h.reshape(-1, h.shape[-1]), conv.weight.reshape(conv.weight.shape[0], -1), None,
                                    mode=mod.mode).reshape(*h.shape[:-1], -1)
        bnp = nat.make_bn(bn.weight, bn.bias, bn.running_mean, bn.running_var, momentum=bn.momentum, eps=bn.eps, training=False)
        if mod.act == nat.LIN_HARDSWISH:
            a = torch.nn.functional.hardswish(see(name + ".u", nat.bn_act_fwd(y, bnp, nat.LIN_NONE, y.shape[-1])[0]))
        else:
            a = nat.bn_act_fwd(y, bnp, mod.act, y.shape[-1])[0]
        if residual is not None:
            a = nat.add_f32(a, residual.contiguous())
        return see(out_name or name, a)
    seen = 0
    with torch.no_grad():
        for x in batches:
            x = see("", _calibration_batch(x, dev, feature_extractor, F, T))
            h = cba(net.features[0], x, "stem")
            for i, blk in enumerate(list(net.features)[1:-1]):
                p, h_in = f"b{i}.", h
                layers = list(blk.block)
                if len(layers) - (1 if any(hasattr(m, "fc1") for m in layers) else 0) == 3:
                    h = cba(layers.pop(0), h, p + "expand")
                h = cba(layers.pop(0), h, p + "dw")
                if hasattr(layers[0], "fc1"):
                    se = layers.pop(0)
                    B, H, W, Cn = h.shape
                    x3 = h.reshape(B, H * W, Cn).contiguous()
                    w1, w2 = se.fc1.weight.reshape(se.fc1.weight.shape[0], -1), se.fc2.weight.reshape(se.fc2.weight.shape[0], -1)
                    hid = see(p + "h", nat.linear_mfma_fwd(nat.pool_hw_fwd(x3), w1, se.fc1.bias, act=nat.LIN_RELU, mode=se.mode))
                    gate = nat.linear_mfma_fwd(hid, w2, se.fc2.bias, act=nat.LIN_HARDSIGMOID, mode=se.mode)
                    h = nat.scale_bc_fwd(x3, gate).reshape(B, H, W, Cn)
                h = cba(layers[0], h, p + "project", p + "out", residual=h_in if blk.use_res_connect else None)
            h = cba(net.features[-1], h, "last")
            B, H, W, Cn = h.shape
            cls = net.classifier[0]
            pre = see("cls0.u", nat.linear_mfma_fwd(nat.pool_hw_fwd(h.reshape(B, H * W, Cn).contiguous()), cls.weight, cls.bias, mode=cls.mode))
            see("hidden", torch.nn.functional.hardswish(pre))
            seen += x.shape[0]
    if seen == 0:
        raise QuantizationError("the calibration data is empty")
    got = torch.stack([lo, hi], dim=1).cpu().tolist()                     # the one read-back
    return {"x_min": got[0][0], "x_max": got[0][1], "ranges": {n: got[at[n]] for n in names}, "samples": seen}


def lstm_entry(model) -> dict:
    """The header's ``lstm`` entry of an ``LSTMWakeword``: what its constructor needs besides ``num_classes``."""
    return {"input_size": int(model.lstm.input_size), "hidden_size": int(model.hidden_size), "num_layers": int(model.num_layers),
            "bidirectional": bool(model.bidirectional)}


def calibrate_lstm(model, batches: Iterable[torch.Tensor], input_size, device, feature_extractor=None) -> dict:
    """The input's minimum and maximum over the calibration batches -- all an ``LSTMWakeword`` bundle calibrates: hidden state,
    gates and cell have fixed scales.  Batches are (B,1,F,T) features, (B,T,F) sequences or (B,N) waveforms, which go through
    ``feature_extractor``; T may differ from batch to batch.  Torch reductions on the device and one read-back."""
    dev = torch.device(device)
    F = int(input_size)
    lo = torch.full((), float("inf"), device=dev)
    hi = torch.full((), float("-inf"), device=dev)
    seen = 0
    with torch.no_grad():
        for x in batches:
            x = _calibration_batch(x, dev, feature_extractor, F, sequences=True)
            lo, hi = torch.minimum(lo, x.min()), torch.maximum(hi, x.max())
            seen += x.shape[0]
    if seen == 0:
        raise QuantizationError("the calibration data is empty")
    got = torch.stack([lo, hi]).cpu().tolist()                    # the one read-back
    return {"x_min": got[0], "x_max": got[1], "samples": seen}


class ModelExporter:
    """The reference's ``ONNXExporter`` (``onnx_exporter.py:37-193``).  ``calibration``: an iterable of feature batches
    ``(B,1,F,T)`` -- or of waveforms ``(B,N)``, which go through ``feature_extractor`` (default: a mel ``FeatureExtractor``
    with ``n_mels = F``) -- that the int8 export takes its ranges from.  It is never replaced by random data."""

    def __init__(self, model: nn.Module, sample_input_shape: Tuple[int, ...], device: str = "cuda", calibration=None,
                 feature_extractor=None, architecture: Optional[str] = None):
        self.architecture = architecture         # the factory name to record; default: looked up from the model's class
        self.model, self.sample_input_shape, self.device = model, tuple(int(v) for v in sample_input_shape), device
        self.calibration, self.feature_extractor = calibration, feature_extractor
        self.model.to(device)
        self.model.eval()
        logger.info("ModelExporter initialized with input shape: %s", self.sample_input_shape)

    def export(self, config: ExportConfig) -> Dict[str, Any]:
        output_path = Path(config.output_path)
        logger.info("Exporting model to: %s", output_path)
        try:
            output_path.parent.mkdir(parents=True, exist_ok=True)
        except Exception as e:                                    # noqa: BLE001 -- as the reference: any failure is reported
            logger.error("Failed to create output directory: %s", e)
            return {"success": False, "error": f"Directory creation failed: {e}"}
        was_training = self.model.training
        self.model.eval()
        try:
            try:
                dummy = torch.randn(*self.sample_input_shape).to(self.device)
            except Exception as e:                                # noqa: BLE001
                return {"success": False, "error": f"Input tensor creation failed: {e}"}
            try:
                with torch.no_grad():
                    test_output = self.model(dummy)
                    if not torch.isfinite(test_output).all():
                        logger.error("Model produces non-finite outputs")
                        return {"success": False, "error": "Model outputs contain NaN or Inf"}
                arch = self.architecture or _architecture(self.model)
                if type(self.model).__name__ == "ResNet18Wakeword":
                    arch = "ResNet18Wakeword"                      # the factory does not build the class: bundles go by its own name
                state = _state_numpy(self.model)
                if type(self.model).__name__ == "LSTMWakeword":
                    arch = "LSTMWakeword"                          # likewise: create_model("lstm") is switched off
                more = {"tcn": tcn_entry(self.model)} if arch == "TCNWakeword" and hasattr(self.model, "tcn") else {}
                if arch == "LSTMWakeword" and hasattr(self.model, "lstm"):
                    more = {"lstm": lstm_entry(self.model)}
                if arch == "crnn" and hasattr(self.model, "rnn") and hasattr(self.model, "front"):
                    more = {"crnn": crnn_entry(self.model)}
                header = make_header("fp32", arch, int(test_output.shape[1]), self.sample_input_shape,
                                     [k for k in state if k.endswith("weight")], config, **more)
                write_bundle(output_path, header, float_arrays(state, fp16=False))
                if not output_path.exists():
                    return {"success": False, "error": "Export completed but file not found"}
                size_mb = output_path.stat().st_size / (1024 * 1024)
                results = {"success": True, "path": str(output_path), "opset_version": config.opset_version,
                           "dynamic_batch": config.dynamic_batch, "file_size_mb": size_mb}
                for kind, wanted, write in (("fp16", config.quantize_fp16, self._write_fp16),
                                            ("int8", config.quantize_int8, self._write_int8)):
                    if not wanted:
                        continue
                    try:
                        path = write(output_path, header, state, config)
                        mb = path.stat().st_size / (1024 * 1024)
                        results[f"{kind}_path"], results[f"{kind}_size_mb"] = str(path), mb
                        results[f"{kind}_reduction"] = (1 - mb / size_mb) * 100
                    except Exception as e:                        # noqa: BLE001
                        logger.error("%s quantization failed: %s", kind.upper(), e)
                        results[f"{kind}_error"] = str(e)
                return results
            except Exception as e:                                # noqa: BLE001
                logger.exception("Export failed: %s", e)
                return {"success": False, "error": str(e)}
        finally:
            if was_training:
                self.model.train()

    def _write_fp16(self, output_path: Path, header: dict, state: dict, config: ExportConfig) -> Path:
        path = output_path.parent / f"{output_path.stem}_fp16.npz"
        return write_bundle(path, dict(header, kind="fp16"), float_arrays(state, fp16=True))

    def _write_int8(self, output_path: Path, header: dict, state: dict, config: ExportConfig) -> Path:
        entry = _INT8.get(header["architecture"])
        if entry is None:
            raise QuantizationError("int8 export covers cnn_small only among the factory's architectures -- with crnn, whose conv "
                                    "stack is cnn_small's, and mobilenetv3 -- and TCNWakeword, ResNet18Wakeword and LSTMWakeword; not "
                                    f"{header['architecture']!r}")
        if self.calibration is None:
            raise QuantizationError("int8 export needs calibration data (ModelExporter(..., calibration=batches)); "
                                    "it is never calibrated on random input")
        F, T = self.sample_input_shape[-2:]
        fe = self.feature_extractor
        if fe is None:
            from ..data.feature_extraction import FeatureExtractor
            fe = FeatureExtractor(n_mels=F, device=self.device)
        entry.check(header)
        cal = entry.calibrate(self.model, self.calibration, F, T, self.device, fe)
        if config.verbose:
            logger.info("calibrated ranges: %s", cal)
        arrays, scales = entry.quantize(self.model, state, header, F, T, cal)
        h = dict(header, kind="int8", layers=entry.layers(arrays), feature_shape=[int(F), int(T)], scales=scales, calibration=cal)
        check_bundle(h, arrays)
        return write_bundle(output_path.parent / f"{output_path.stem}_int8.npz", h, arrays)


@dataclass(frozen=True)
class _Int8:
    """What the int8 export of one architecture is made of.  ``check(header)`` refuses arguments the law does not cover;
    ``calibrate(model, batches, F, T, device, feature_extractor)`` -> the ranges; ``quantize(model, state, header, F, T, cal)`` ->
    (arrays, scales); ``layers(arrays)`` -> the header's layer names; ``runtime``: the class that runs the bundle."""
    runtime: type
    check: Callable
    calibrate: Callable
    quantize: Callable
    layers: Callable


def _check_crnn_header(header):
    if "crnn" not in header:
        raise QuantizationError("the header of a crnn bundle holds no crnn entry (hidden_size, num_layers, bidirectional)")
    check_crnn_args(header["crnn"], header["num_classes"])


def _conv_layers(tail):
    return lambda arrays: [k[:-2] for k in arrays if k.endswith(".w") and k != "fc.w"] + tail


_INT8 = {
    "cnn_small": _Int8(
        QuantizedCNNSmall, lambda header: None,
        lambda model, batches, F, T, dev, fe: calibrate_cnn_small(model, batches, (F, T), dev, fe),
        lambda model, state, header, F, T, cal: quantize_cnn_small(state, (F, T), cal["x_min"], cal["x_max"], cal["a_max"], cal["p_max"],
                                                                   eps=model.stem.bn.eps),
        lambda arrays: CONVS + ["pool", "fc"]),
    "TCNWakeword": _Int8(
        QuantizedTCN, lambda header: check_tcn_args(header["tcn"], header["num_classes"]),
        lambda model, batches, F, T, dev, fe: calibrate_tcn(model, batches, (F, T), dev, fe),
        lambda model, state, header, F, T, cal: quantize_tcn(state, header["tcn"], (F, T), cal["x_min"], cal["x_max"], cal["a_max"],
                                                             cal["p_max"]),
        lambda arrays: [k[:-2] for k in arrays if k.endswith(".w") and k.startswith("b")] + ["pool", "fc"]),
    "ResNet18Wakeword": _Int8(
        QuantizedResNet18, lambda header: None,
        lambda model, batches, F, T, dev, fe: calibrate_resnet18(model, batches, (F, T), dev, fe),
        lambda model, state, header, F, T, cal: quantize_resnet18(state, (F, T), cal, eps=model.resnet.bn1.eps),
        _conv_layers(["pool", "fc"])),
    "LSTMWakeword": _Int8(
        QuantizedLSTM, lambda header: check_lstm_args(header["lstm"], header["num_classes"]),
        lambda model, batches, F, T, dev, fe: calibrate_lstm(model, batches, F, dev, fe),
        lambda model, state, header, F, T, cal: quantize_lstm(state, header["lstm"], cal["x_min"], cal["x_max"]),
        lambda arrays: [k[:-2] for k in arrays if k.endswith(".w")]),
    "crnn": _Int8(
        QuantizedCRNN, _check_crnn_header,
        lambda model, batches, F, T, dev, fe: calibrate_crnn(model, batches, F, dev, fe),
        lambda model, state, header, F, T, cal: quantize_crnn(state, header["crnn"], F, cal, eps=model.front.stem.bn.eps),
        _conv_layers(["fmean", "fc"])),
    "mobilenetv3": _Int8(
        QuantizedMobileNetV3, lambda header: None,
        lambda model, batches, F, T, dev, fe: calibrate_mobilenetv3(model, batches, (F, T), dev, fe),
        lambda model, state, header, F, T, cal: quantize_mobilenetv3(state, (F, T), cal, eps=model.mobilenet.features[0][1].eps),
        _conv_layers(["pool", "fc"])),
}


def export_model(checkpoint_path: Path, output_path: Path, opset_version: int = 14, dynamic_batch: bool = True,
                 quantize_fp16: bool = False, quantize_int8: bool = False, device: str = "cuda", calibration=None) -> Dict:
    """Checkpoint -> bundles (``onnx_exporter.py:257-347``); the checkpoint is read by ``load_model_for_evaluation``."""
    from ..evaluation.evaluator import load_model_for_evaluation
    model, info = load_model_for_evaluation(Path(checkpoint_path), device)
    config = info["config"]
    sample_rate, duration = config.data.sample_rate, config.data.audio_duration
    n_frames = int(sample_rate * duration) // config.data.hop_length + 1
    shape = (1, 1, config.data.n_mels, n_frames)
    from ..data.feature_extraction import FeatureExtractor
    fe = FeatureExtractor(sample_rate=sample_rate, n_mels=config.data.n_mels, n_fft=getattr(config.data, "n_fft", 1024),
                          hop_length=config.data.hop_length, device=device)
    exporter = ModelExporter(model, shape, device, calibration=calibration, feature_extractor=fe,
                             architecture=config.model.architecture)
    results = exporter.export(ExportConfig(output_path=Path(output_path), opset_version=opset_version,
                                           dynamic_batch=dynamic_batch, quantize_fp16=quantize_fp16,
                                           quantize_int8=quantize_int8, optimize=True, verbose=False))
    results.update(architecture=config.model.architecture, sample_rate=sample_rate, duration=duration, input_shape=shape)
    return results


def load_exported_model(path: Path, device: str = "cuda") -> nn.Module:
    """A bundle as a module in eval mode on ``device``: the factory's architecture with the stored weights (fp16 widened to
    fp32) or, for an int8 bundle, ``QuantizedCNNSmall`` / ``QuantizedTCN`` / ``QuantizedResNet18`` / ``QuantizedLSTM`` /
    ``QuantizedCRNN`` / ``QuantizedMobileNetV3``.  A ``crnn`` bundle is built from its header's ``crnn`` entry where it has one.  A
    ``TCNWakeword`` bundle is built from its header's ``tcn`` entry, an ``LSTMWakeword`` bundle from its ``lstm`` entry and a
    ``ResNet18Wakeword`` bundle from ``num_classes`` alone (the factory does not offer those classes).  ``ModelEvaluator`` and ``RecordingScanner`` take any of them."""
    header, arrays = load_bundle(path)
    check_bundle(header, arrays)
    if header["kind"] == "int8":
        return _INT8.get(header["architecture"], _INT8["cnn_small"]).runtime(header, arrays).to(device)
    if header["architecture"] == "ResNet18Wakeword":
        from ..models import ResNet18Wakeword
        model = ResNet18Wakeword(num_classes=header["num_classes"])
    elif header["architecture"] == "LSTMWakeword":
        from ..models import LSTMWakeword
        from .bundle import check_lstm_entry
        check_lstm_entry(header)
        e = header["lstm"]
        model = LSTMWakeword(input_size=e["input_size"], hidden_size=e["hidden_size"], num_layers=e["num_layers"],
                             num_classes=header["num_classes"], bidirectional=e["bidirectional"])
    elif header["architecture"] == "crnn" and "crnn" in header:
        from ..models import create_model
        from .bundle import check_crnn_entry
        check_crnn_entry(header)
        e = header["crnn"]
        model = create_model(architecture="crnn", num_classes=header["num_classes"], pretrained=False, hidden_size=e["hidden_size"],
                             num_layers=e["num_layers"], bidirectional=e["bidirectional"])
    elif header["architecture"] == "TCNWakeword":
        from ..models import TCNWakeword
        from .bundle import check_tcn_entry
        F, channels, k = check_tcn_entry(header)
        model = TCNWakeword(input_size=F, num_channels=channels, kernel_size=k, num_classes=header["num_classes"])
    else:
        from ..models import create_model
        model = create_model(architecture=header["architecture"], num_classes=header["num_classes"], pretrained=False)
    state = {}
    for k, v in arrays.items():
        if k.startswith(STATE_PREFIX):
            t = torch.from_numpy(np.ascontiguousarray(v))
            state[k[len(STATE_PREFIX):]] = t.float() if t.is_floating_point() else t
    model.load_state_dict(state)
    model.to(device)
    model.eval()
    return model


def validate_exported_model(path: Path, pytorch_model: Optional[nn.Module] = None, sample_input: Optional[torch.Tensor] = None,
                            device: str = "cuda") -> Dict:
    """The reference's ``validate_onnx_model`` (``:350-438``) and its keys; never raises on a malformed bundle."""
    results: Dict[str, Any] = {"valid": False, "error": None}
    try:
        path = Path(path)
        header, arrays = load_bundle(path)
        check_bundle(header, arrays)
        results["valid"] = True
        results["graph"] = len(header["layers"])
        results["inputs"] = [("input", [0] + list(header["input_shape"][1:]))]      # 0: the batch dimension is free
        results["outputs"] = [("output", [0, header["num_classes"]])]
        results["file_size_mb"] = path.stat().st_size / (1024 * 1024)
        if sample_input is not None:
            model = load_exported_model(path, device)
            with torch.no_grad():
                out = model(sample_input.to(device)).cpu().numpy()
            results["inference_success"] = True
            results["output_shape"] = out.shape
            if pytorch_model is not None:
                pytorch_model.eval()
                pytorch_model.to(device)
                with torch.no_grad():
                    ref = pytorch_model(sample_input.to(device)).cpu().numpy()
                results["max_difference"] = float(np.abs(ref - out).max())
                results["mean_difference"] = float(np.abs(ref - out).mean())
                results["numerically_equivalent"] = bool(results["max_difference"] < 1e-3)
    except Exception as e:                                        # noqa: BLE001 -- as the reference: any failure is the answer
        logger.error("Validation failed: %s", e)
        results["valid"] = False
        results["error"] = str(e)
    return results


def _time_forwards(model, x, num_runs: int) -> float:
    """ms per forward: device events around ``num_runs`` forwards after 10 warm-up runs, one synchronisation at the end."""
    with torch.no_grad():
        for _ in range(10):
            model(x)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(num_runs):
            model(x)
        end.record()
    end.synchronize()
    return start.elapsed_time(end) / num_runs


def benchmark_exported_model(path: Path, pytorch_model: nn.Module, sample_input: torch.Tensor, num_runs: int = 100,
                             device: str = "cuda") -> Dict:
    """The reference's ``benchmark_onnx_model`` (``:441-517``); ``onnx_time_ms`` repeats ``exported_time_ms`` for callers
    that read the reference's key."""
    if num_runs < 1:
        raise ValueError("num_runs must be at least 1")
    pytorch_model.eval()
    pytorch_model.to(device)
    x = sample_input.to(device)
    exported = load_exported_model(path, device)
    t_torch = _time_forwards(pytorch_model, x, num_runs)
    t_exp = _time_forwards(exported, x, num_runs)
    return {"pytorch_time_ms": t_torch, "exported_time_ms": t_exp, "onnx_time_ms": t_exp, "speedup": t_torch / t_exp,
            "num_runs": num_runs}


ONNXExporter = ModelExporter
export_model_to_onnx = export_model
validate_onnx_model = validate_exported_model
benchmark_onnx_model = benchmark_exported_model
__all__ = ["ExportConfig", "ModelExporter", "ONNXExporter", "export_model", "export_model_to_onnx", "load_exported_model",
           "validate_exported_model", "validate_onnx_model", "benchmark_exported_model", "benchmark_onnx_model",
           "QuantizedCNNSmall", "QuantizedTCN", "QuantizedResNet18", "QuantizedLSTM", "BundleError", "QuantizationError",
           "calibrate_cnn_small", "calibrate_tcn", "calibrate_resnet18", "calibrate_lstm", "QuantizedCRNN", "calibrate_crnn",
           "QuantizedMobileNetV3", "calibrate_mobilenetv3"]
