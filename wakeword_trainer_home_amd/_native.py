"""ctypes binding of libwwhip.so (include/wwhip.h) -- the only door to the HIP hot path.

There is deliberately NO fallback: if the shared library is missing, or a tensor is not
on an MI355X, these wrappers raise.  PyTorch is used for device memory and streams only.
"""
import contextlib
import ctypes as C
import math
import os
from pathlib import Path

import torch

_LIB_PATH = Path(__file__).resolve().parent / "csrc" / "libwwhip.so"
_lib = None
_ctx = {}

ABI_VERSION = 17
BWD_ALL, BWD_LATE, BWD_EARLY = 0, 1, 2
ACT_F32, ACT_BF16, ACT_F16 = 0, 1, 2
LOSS_CE, LOSS_FOCAL = 0, 1
REDUCE_MEAN, REDUCE_SUM, REDUCE_NONE = 0, 1, 2
DIV_BATCH, DIV_WEIGHT_SUM = 0, 1
WAVE_F32, WAVE_I16 = 0, 1
CNN_SMALL_NPTR = 47


class NativeError(RuntimeError):
    pass


class FeatCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("n_fft", C.c_int32), ("hop", C.c_int32), ("n_mels", C.c_int32),
                ("n_mfcc", C.c_int32), ("f_min", C.c_float), ("f_max", C.c_float), ("log_eps", C.c_float)]


class SpecAugCfg(C.Structure):
    _fields_ = [("freq_mask_param", C.c_int32), ("time_mask_param", C.c_int32), ("n_freq_masks", C.c_int32),
                ("n_time_masks", C.c_int32), ("freq_mask_prob", C.c_float), ("time_mask_prob", C.c_float)]


class BN(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p),
                ("running_var", C.c_void_p), ("momentum", C.c_float), ("eps", C.c_float), ("training", C.c_int32)]


class AudioAugCfg(C.Structure):
    _fields_ = [("rir_prob", C.c_float), ("noise_prob", C.c_float), ("snr_min_db", C.c_float), ("snr_max_db", C.c_float)]


class AudioTsmCfg(C.Structure):
    _fields_ = [("stretch_prob", C.c_float), ("rate_min", C.c_float), ("rate_max", C.c_float), ("pitch_prob", C.c_float),
                ("semis_min", C.c_int32), ("semis_max", C.c_int32)]


class LinearEpi(C.Structure):
    _fields_ = [("act", C.c_int32), ("dropout_p", C.c_float), ("seed", C.c_uint64), ("step", C.c_uint64),
                ("sample_offset", C.c_uint64)]


LIN_NONE, LIN_HARDSWISH, LIN_RELU, LIN_HARDSIGMOID = 0, 1, 2, 3


class OptimCfg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("momentum", C.c_float), ("max_norm", C.c_float)]


OPT_ADAM, OPT_ADAMW, OPT_SGD = 0, 1, 2


class GruDir(C.Structure):
    """ww_gru_dir: one direction of a bidirectional GRU layer (include/wwhip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("w_ih", "w_hh", "b_ih", "b_hh", "h0", "h_n", "ws", "dh_n", "dw_ih", "dw_hh", "db_ih",
                                          "db_hh", "dh0")]


class LstmDir(C.Structure):
    """ww_lstm_dir: one direction of a bidirectional LSTM layer (include/wwhip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0", "h_n", "c_n", "ws", "dh_n", "dc_n", "dw_ih",
                                          "dw_hh", "db_ih", "db_hh", "dh0", "dc0")]


class StepCtl(C.Structure):
    _fields_ = [("step", C.c_uint64), ("lr", C.c_float), ("parity", C.c_int32), ("loss_scale", C.c_float),
                ("growth_tracker", C.c_int32), ("reserved", C.c_int32 * 2)]


STEP_CTL_BYTES = C.sizeof(StepCtl)


class LossScale(C.Structure):
    _fields_ = [("scale", C.c_float * 2), ("growth_tracker", C.c_int32 * 2), ("growth_factor", C.c_float),
                ("backoff_factor", C.c_float), ("growth_interval", C.c_int32), ("reserved", C.c_int32)]


LOSS_SCALE_BYTES = C.sizeof(LossScale)


def loss_scale_new(dev, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, growth_tracker=0):
    """Device ww_loss_scale (uint8[32] tensor) with torch.amp.GradScaler's defaults; both slots start equal."""
    host = LossScale((C.c_float * 2)(init_scale, init_scale), (C.c_int32 * 2)(growth_tracker, growth_tracker),
                     growth_factor, backoff_factor, growth_interval, 0)
    return torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)


def loss_scale_read(t, slot=0) -> dict:
    s = LossScale.from_buffer_copy(bytes(t.cpu().numpy().tobytes()))
    return {"scale": s.scale[slot], "growth_tracker": s.growth_tracker[slot], "growth_factor": s.growth_factor,
            "backoff_factor": s.backoff_factor, "growth_interval": s.growth_interval}


class StepStats(C.Structure):
    _fields_ = [("loss", C.c_float), ("grad_norm", C.c_float), ("correct", C.c_int32), ("tp", C.c_int32),
                ("tn", C.c_int32), ("fp", C.c_int32), ("fn", C.c_int32), ("nonfinite", C.c_int32),
                ("bad_target", C.c_int32), ("count", C.c_int32), ("found_inf", C.c_float), ("reserved", C.c_int32)]


STEP_STATS_BYTES = C.sizeof(StepStats)

class Q8Io(C.Structure):
    """ww_q8_io: the scalars of an int8 bundle (include/wwhip.h)."""
    _fields_ = [("in_scale", C.c_float), ("in_zero", C.c_int32), ("pool_mult", C.c_int32), ("pool_shift", C.c_int32)]


Q8_NPTR, Q8_NACT, Q8_PAIR, Q8_FUSED = 39, 9, 0, 1
TQ8_MAX_BLOCKS, TQ8_BLOCK_NPTR = 8, 12


class Tq8Io(C.Structure):
    """ww_tq8_io: the scalars of an int8 TCNWakeword bundle (include/wwhip.h)."""
    _fields_ = [("in_scale", C.c_float), ("in_zero", C.c_int32), ("pool_mult", C.c_int32), ("pool_shift", C.c_int32),
                ("n_blocks", C.c_int32), ("kernel_size", C.c_int32), ("input_size", C.c_int32), ("num_classes", C.c_int32),
                ("channels", C.c_int32 * TQ8_MAX_BLOCKS), ("add_mult", C.c_int32 * TQ8_MAX_BLOCKS),
                ("add_shift", C.c_int32 * TQ8_MAX_BLOCKS), ("skip_mult", C.c_int32 * TQ8_MAX_BLOCKS),
                ("skip_shift", C.c_int32 * TQ8_MAX_BLOCKS)]


RQ8_NPTR, RQ8_RELU, RQ8_SIGNED, RQ8_ADD = 103, 0, 1, 2
RQ8_PLANES = (64, 128, 256, 512)


class Rq8Io(C.Structure):
    """ww_rq8_io: the scalars of an int8 ResNet18Wakeword bundle (include/wwhip.h)."""
    _fields_ = [("in_scale", C.c_float), ("in_zero", C.c_int32), ("pool_mult", C.c_int32), ("pool_shift", C.c_int32),
                ("num_classes", C.c_int32), ("res_mult", C.c_int32 * 8), ("res_shift", C.c_int32 * 8)]


LQ8_MAX_LAYERS, LQ8_LAYER_NPTR, LQ8_TAIL_NPTR, LQ8_HIDDEN = 8, 8, 5, 128


class Lq8Io(C.Structure):
    """ww_lq8_io: the scalars of an int8 LSTMWakeword bundle (include/wwhip.h)."""
    _fields_ = [("in_scale", C.c_float), ("in_zero", C.c_int32), ("input_size", C.c_int32), ("num_layers", C.c_int32),
                ("num_directions", C.c_int32), ("num_classes", C.c_int32)]


CQ8_MAX_LAYERS, CQ8_CONV_NPTR, CQ8_LAYER_NPTR, CQ8_TAIL_NPTR, CQ8_NACT, CQ8_HIDDEN = 8, 36, 8, 5, 5, 128


class Cq8Io(C.Structure):
    """ww_cq8_io: the scalars of an int8 CRNNWakeword bundle (include/wwhip.h)."""
    _fields_ = [("in_scale", C.c_float), ("in_zero", C.c_int32), ("fmean_mult", C.c_int32), ("fmean_shift", C.c_int32),
                ("num_layers", C.c_int32), ("num_directions", C.c_int32), ("num_classes", C.c_int32)]


MQ8_BLOCKS, MQ8_BLOCK_NPTR, MQ8_NPTR, MQ8_LAST, MQ8_HIDDEN, MQ8_RELU, MQ8_HSWISH, MQ8_SIGNED = 11, 22, 260, 576, 1024, 0, 1, 2


class Mq8Io(C.Structure):
    """ww_mq8_io: the scalars of an int8 MobileNetV3Wakeword bundle (include/wwhip.h)."""
    _fields_ = [("in_scale", C.c_float), ("in_zero", C.c_int32), ("num_classes", C.c_int32)] + \
               [(k, C.c_int32) for k in ("stem_zu", "stem_zo", "last_zu", "last_zo", "cls_zu", "cls_zo", "pool_mult", "pool_shift")] + \
               [(k, C.c_int32 * MQ8_BLOCKS) for k in ("exp_zu", "exp_zo", "dw_zu", "dw_zo", "sepool_mult", "sepool_shift", "gate_mult",
                                                      "gate_shift", "res_mult", "res_shift")]


_vp, _i, _f, _u64, _sz = C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_size_t
_SIGS = {
    "ww_abi_version": (C.c_int, []),
    "ww_last_error": (C.c_char_p, []),
    "ww_ctx_create": (C.c_int, [_i, C.POINTER(_vp)]),
    "ww_ctx_destroy": (C.c_int, [_vp]),
    "ww_ctx_bind_step_ctl": (C.c_int, [_vp, _vp]),
    "ww_ctx_set_logmel_workgroups": (C.c_int, [_vp, C.c_int]),
    "ww_ctx_set_grid_cap": (C.c_int, [_vp, C.c_int]),
    "ww_ctx_set_dw_wide_addr": (C.c_int, [_vp, C.c_int]),
    "ww_step_ctl_advance": (C.c_int, [_vp, _vp]),
    "ww_feat_num_frames": (C.c_int, [_i, _i]),
    "ww_feat_mel_tables": (C.c_int, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp]),
    "ww_logmel_fwd": (C.c_int, [_vp, _vp, _i, _i, _i, C.POINTER(FeatCfg), _vp, C.POINTER(SpecAugCfg), _u64, _u64, _u64,
                                _vp, _vp]),
    "ww_specaug_apply": (C.c_int, [_vp, _vp, _i, _i, _i, C.POINTER(SpecAugCfg), _u64, _u64, _u64, _vp, _vp]),
    "ww_audio_augment_scratch_bytes": (_sz, [_i, _i]),
    "ww_audio_rir_spectra_bytes": (_sz, [_i]),
    "ww_audio_rir_spectra": (C.c_int, [_vp, _vp, _i, _i, _vp, _sz, _vp]),
    "ww_audio_augment": (C.c_int, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _i, _i, C.POINTER(AudioAugCfg), _u64, _u64,
                                   _u64, _vp, _vp, _sz, _vp]),
    "ww_audio_tsm_max_grains": (C.c_int, [_i, _i]),
    "ww_audio_tsm_scratch_bytes": (_sz, [_i, _i, _i]),
    "ww_audio_tsm": (C.c_int, [_vp, _vp, _vp, _i, _i, C.POINTER(AudioTsmCfg), _u64, _u64, _u64, _vp, _vp, _vp, _sz, _vp]),
    "ww_gemm16_nt": (C.c_int, [_vp, _i, _vp, _vp, _vp, _i, C.c_long, C.c_long, C.c_long, _vp]),
    "ww_linear_mfma_fwd": (C.c_int, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, C.POINTER(LinearEpi), _vp, _vp, _vp]),
    "ww_linear_mfma_bwd_scratch_bytes": (_sz, [_i, _i, _i]),
    "ww_linear_mfma_bwd": (C.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, C.POINTER(LinearEpi), _vp, _vp, _vp, _vp, _sz,
                                     _vp]),
    "ww_tconv1d_scratch_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "ww_tconv1d_fwd": (C.c_int, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ww_tconv1d_bwd": (C.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _f, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "ww_add_relu_fwd": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    "ww_relu_mask_bwd": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    "ww_conv2d_scratch_bytes": (_sz, [_i] * 7),
    "ww_conv2d_fwd": (C.c_int, [_vp, _i, _vp, _vp] + [_i] * 7 + [_vp, _vp, _sz, _vp]),
    "ww_conv2d_bwd": (C.c_int, [_vp, _i, _vp, _vp, _vp] + [_i] * 7 + [_vp, _i, _vp, _vp, _sz, _vp]),
    "ww_conv2d_stem_scratch_bytes": (_sz, [_i, _i]),
    "ww_conv2d_stem_fwd": (C.c_int, [_vp, _vp, _vp] + [_i] * 6 + [_vp, _vp]),
    "ww_conv2d_stem_bwd_dw": (C.c_int, [_vp, _vp, _vp] + [_i] * 6 + [_vp, _vp, _sz, _vp]),
    "ww_maxpool3x3s2_fwd": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "ww_maxpool3x3s2_bwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "ww_conv2d_st_scratch_bytes": (_sz, [_i] * 7),
    "ww_conv2d_st_fwd": (C.c_int, [_vp, _i, _vp, _vp] + [_i] * 7 + [_vp, _vp, _vp, _sz, _vp]),
    "ww_conv2d_st_bwd": (C.c_int, [_vp, _i, _vp, _vp, _vp] + [_i] * 7 + [_vp, _i, _vp, _vp, _sz, _vp]),
    "ww_bn_act_st_fwd": (C.c_int, [_vp, _i, _vp, C.c_long, _i, C.POINTER(BN), _i, _vp, _vp, _vp, C.c_long, _vp, _vp, _vp, _vp, _vp]),
    "ww_bn_act_st_bwd": (C.c_int, [_vp, _i, _vp, _vp, C.c_long, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "ww_conv2d_stem_st_fwd": (C.c_int, [_vp, _i, _vp, _vp] + [_i] * 6 + [_vp, _vp]),
    "ww_conv2d_stem_st_bwd_dw": (C.c_int, [_vp, _i, _vp, _vp] + [_i] * 6 + [_vp, _vp, _sz, _vp]),
    "ww_maxpool3x3s2_st_fwd": (C.c_int, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "ww_maxpool3x3s2_st_bwd": (C.c_int, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "ww_mean_hw_st_fwd": (C.c_int, [_vp, _i, _vp, _i, _i, _i, _vp, _vp]),
    "ww_mean_hw_st_bwd": (C.c_int, [_vp, _i, _vp, _i, _i, _i, _vp, _vp]),
    "ww_relu_mask_st_bwd": (C.c_int, [_vp, _i, _vp, _vp, _sz, _vp, _vp]),
    "ww_tconv1d_st_scratch_bytes": (_sz, [_i] * 6),
    "ww_tconv1d_st_fwd": (C.c_int, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ww_tconv1d_st_bwd": (C.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _f, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "ww_dropout_bt_st": (C.c_int, [_vp, _i, _vp, _i, _i, _i, _f, _u64, _u64, _u64, _i, _vp, _vp]),
    "ww_add_relu_st_fwd": (C.c_int, [_vp, _i, _vp, _vp, _sz, _vp, _vp]),
    "ww_seq_round_st": (C.c_int, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "ww_dropout_bt": (C.c_int, [_vp, _vp, C.c_long, _i, _i, _i, _f, _u64, _u64, _u64, _i, _vp, C.c_long, _vp]),
    "ww_nhwc_scratch_bytes": (_sz, [_i]),
    "ww_bn_act_fwd": (C.c_int, [_vp, _vp, C.c_long, _i, C.POINTER(BN), _i, _vp, _vp, _vp, _vp, _vp]),
    "ww_bn_act_bwd": (C.c_int, [_vp, _vp, _vp, C.c_long, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "ww_conv1x1_bn_act_fwd": (C.c_int, [_vp, _i, _vp, _vp, _i, _i, _i, C.POINTER(BN), _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ww_dwconv_bn_act_fwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, C.POINTER(BN), _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ww_dwconv_nhwc_fwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "ww_dwconv_nhwc_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "ww_pool_hw_fwd": (C.c_int, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "ww_scale_bc_fwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "ww_scale_bc_bwd_gate": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "ww_scale_pool_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "ww_se_bwd_scratch_bytes": (_sz, [_i, _i, _i]),
    "ww_se_fwd": (C.c_int, [_vp, _vp, _i, _i, _i, _i] + [_vp] * 9),
    "ww_se_bwd": (C.c_int, [_vp] * 8 + [_i, _i, _i, _i] + [_vp] * 6 + [_sz, _vp]),
    "ww_stem3x3s2_bn_act_fwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, C.POINTER(BN), _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ww_stem3x3s2_bwd_dw": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "ww_im2col3x3s2": (C.c_int, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "ww_add_f32": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    "ww_nhwc_plan_dw": (C.c_int, [_i] * 8 + [C.POINTER(C.c_int)]),
    "ww_nhwc_plan_bn": (C.c_int, [_i, C.c_long, _i, _i, _i, _i, C.POINTER(C.c_int)]),
    "ww_nhwc_plan_stem": (C.c_int, [_i] * 4 + [C.POINTER(C.c_int)]),
    "ww_nhwc_plan_ew": (C.c_int, [C.c_long, _i, _i, C.POINTER(C.c_int)]),
    "ww_conv1x1_row_tile": (C.c_int, [_i] * 4),
    "ww_se_plan": (C.c_int, [_i] * 4 + [C.POINTER(C.c_int)]),
    "ww_pass_plan": (C.c_int, [_i, C.c_long, C.POINTER(C.c_long)]),
    "ww_dw_plan": (C.c_int, [_i, _i, _i, _i, _i, C.POINTER(C.c_long)]),
    "ww_loader_plan": (C.c_int, [_i, _i, C.POINTER(C.c_int)]),
    "ww_gemm_plan": (C.c_int, [_i] * 8 + [C.POINTER(C.c_long)]),
    "ww_gru_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "ww_gru_fwd": (C.c_int, [_vp, _i, _vp, C.c_long, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, C.c_long, _vp, _vp, _sz, _vp]),
    "ww_gru_bidir_fwd": (C.c_int, [_vp, _i, _vp, C.c_long, _vp, _i, _i, _i, _i, _vp, C.c_long, _sz, _vp]),
    "ww_gru_bidir_bwd": (C.c_int, [_vp, _i, _vp, C.c_long, _vp, _vp, C.c_long, _i, _i, _i, _i, _sz, _vp, C.c_long, _vp]),
    "ww_gru_bwd": (C.c_int, [_vp, _i, _vp, C.c_long, _vp, _vp, _vp, C.c_long, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, C.c_long, _i,
                             _vp, _vp, _vp, _vp, _vp, _vp]),
    "ww_lstm_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "ww_lstm_fwd": (C.c_int, [_vp, _i, _vp, C.c_long, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, C.c_long, _vp, _vp, _vp,
                              _sz, _vp]),
    "ww_lstm_bwd": (C.c_int, [_vp, _i, _vp, C.c_long, _vp, _vp, _vp, C.c_long, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, C.c_long,
                              _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ww_lstm_bidir_fwd": (C.c_int, [_vp, _i, _vp, C.c_long, _vp, _i, _i, _i, _i, _vp, C.c_long, _sz, _vp]),
    "ww_lstm_bidir_bwd": (C.c_int, [_vp, _i, _vp, C.c_long, _vp, _vp, C.c_long, _i, _i, _i, _i, _sz, _vp, C.c_long, _vp]),
    "ww_clip_optim_step": (C.c_int, [_vp, C.POINTER(OptimCfg), _vp, _vp, _vp, _vp, _sz, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ww_layer_scratch_bytes": (_sz, []),
    "ww_conv_stem_fwd": (C.c_int, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, C.POINTER(BN), _vp, _vp, _vp, _vp]),
    "ww_dwconv3x3_fwd": (C.c_int, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, C.POINTER(BN), _vp, _vp, _vp, _vp]),
    "ww_pwconv1x1_fwd": (C.c_int, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, C.POINTER(BN), _vp, _vp, _vp, _vp]),
    "ww_gap_fwd": (C.c_int, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "ww_head_fwd": (C.c_int, [_vp, _vp, _i, _i, _vp, _vp, _f, _i, _u64, _u64, _u64, _vp, _vp, _vp]),
    "ww_head_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _vp, _f, _i, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp,
                              _vp, _vp, _vp]),
    "ww_pwconv1x1_bwd": (C.c_int, [_vp, _i] + [_vp] * 10 + [_i, _i, _i] + [_vp] * 7),
    "ww_dwconv3x3_bwd": (C.c_int, [_vp, _i] + [_vp] * 8 + [_i, _i, _i] + [_vp] * 7),
    "ww_conv_stem_bwd": (C.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "ww_conv_stem_bwd_recompute": (C.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "ww_cnn_small_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "ww_cnn_small_fwd": (C.c_int, [_vp, _i, C.POINTER(_vp), _vp, _i, _i, _i, _i, _f, _f, _f, _u64, _u64, _u64, _vp, _sz,
                                   _vp, _vp]),
    "ww_cnn_front_fwd": (C.c_int, [_vp, _i, C.POINTER(_vp), _vp, _i, _i, _i, _i, _f, _f, _vp, _sz, _vp, _vp]),
    "ww_cnn_front_bwd": (C.c_int, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), _vp, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "ww_cnn_small_bwd": (C.c_int, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), _vp, _vp, _i, _i, _i, _f, _u64, _u64, _u64,
                                   _vp, _sz, _i, _vp]),
    "ww_ce2_loss_fwd_bwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "ww_ce2_loss_weighted_fwd_bwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _f, _f, _f, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i,
                                               _vp]),
    "ww_cen_loss_fwd_bwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _f, _f, _f, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i,
                                      _vp]),
    "ww_grad_norm_clip": (C.c_int, [_vp, _vp, _sz, _f, _vp, _vp, _vp]),
    "ww_eval_accumulate": (C.c_int, [_vp, _vp, _i, _vp, _i, _vp, _i, C.c_double, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "ww_eval_accumulate_classes": (C.c_int, [_vp, _vp, _i, _vp, _i, _vp, _i, C.c_double, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "ww_wave_num_windows": (C.c_long, [C.c_long, _i]),
    "ww_wave_windows": (C.c_int, [_vp, _vp, C.c_long, _i, _i, _vp, _vp, _vp]),
    "ww_wave_num_windows_hop": (C.c_long, [C.c_long, _i, _i]),
    "ww_wave_windows_at": (C.c_int, [_vp, _vp, C.c_long, _i, _i, C.c_long, _i, _i, _vp, _vp, _vp]),
    "ww_feat_windows": (C.c_int, [_vp, _vp, _i, C.c_long, _i, _i, C.c_long, _i, _vp, _vp]),
    "ww_detect_accumulate": (C.c_int, [_vp, _vp, _i, _i, _i, _vp, _i, C.c_double, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "ww_loader_indices": (C.c_int, [_vp, _i, _i, _i, _vp, _i, _u64, _u64, _i, _i, C.c_int64, _i, _vp, _vp]),
    "ww_loader_batch": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _u64, _u64, _i, _i, C.c_int64, _i, _i, _vp, _vp,
                                  _vp, _vp]),
    "ww_q8_quantize": (C.c_int, [_vp, _vp, C.c_long, _f, _i, _vp, _vp]),
    "ww_q8_stem_fwd": (C.c_int, [_vp] * 6 + [_i] * 4 + [_vp, _vp]),
    "ww_q8_dwconv3x3_fwd": (C.c_int, [_vp] * 6 + [_i] * 4 + [_vp, _vp]),
    "ww_q8_pwconv1x1_fwd": (C.c_int, [_vp] * 6 + [C.c_long, _vp, _vp]),
    "ww_q8_dwpw_fwd": (C.c_int, [_vp] * 10 + [_i] * 4 + [_vp, _vp]),
    "ww_q8_gap_fc_fwd": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ww_q8_cnn_small_workspace_bytes": (_sz, [_i, _i, _i]),
    "ww_q8_cnn_small_fwd": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(Q8Io), _vp, _i, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "ww_tq8_quantize_bt": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _vp]),
    "ww_tq8_conv1d_fwd": (C.c_int, [_vp] * 6 + [_i] * 7 + [_vp, _i, _i, _vp, _vp]),
    "ww_tq8_skip_add_fwd": (C.c_int, [_vp, _vp, _vp, C.c_long] + [_i] * 6 + [_vp, _vp]),
    "ww_tq8_pool_fc_fwd": (C.c_int, [_vp, _vp] + [_i] * 6 + [_vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "ww_tq8_tcn_workspace_bytes": (_sz, [_i, _i, _i, _i, C.POINTER(C.c_int32)]),
    "ww_tq8_tcn_fwd": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(Tq8Io), _vp, _i, _i, _vp, _sz, _vp, _vp]),
    "ww_rq8_conv2d_fwd": (C.c_int, [_vp] * 6 + [_i] * 9 + [_vp, _i, _i, _i, _vp, _vp]),
    "ww_rq8_stem_fwd": (C.c_int, [_vp] * 6 + [_i] * 4 + [_vp, _vp]),
    "ww_rq8_maxpool_fwd": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "ww_rq8_resnet18_workspace_bytes": (_sz, [_i, _i, _i]),
    "ww_rq8_resnet18_fwd": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(Rq8Io), _vp, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "ww_lq8_proj_fwd": (C.c_int, [_vp] * 6 + [C.c_long, _i, _i, _vp, _vp]),
    "ww_lq8_lstm_layer_fwd": (C.c_int, [_vp] * 8 + [_i, _i, _i, _vp, _vp, _vp]),
    "ww_lq8_head_fwd": (C.c_int, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "ww_lq8_lstm_workspace_bytes": (_sz, [_i] * 5),
    "ww_lq8_lstm_fwd": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(Lq8Io), _vp, _i, _i, _vp, _sz, _vp, _vp]),
    "ww_cq8_fmean_fwd": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "ww_cq8_gru_layer_fwd": (C.c_int, [_vp] * 8 + [_i, _i, _i, _vp, _vp, _vp]),
    "ww_cq8_crnn_workspace_bytes": (_sz, [_i] * 5),
    "ww_cq8_crnn_fwd": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(Cq8Io), _vp, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "ww_mq8_conv1x1_fwd": (C.c_int, [_vp] * 6 + [C.c_long] + [_i] * 5 + [_vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _vp]),
    "ww_mq8_dwconv_fwd": (C.c_int, [_vp] * 6 + [_i] * 9 + [_vp, _vp, _vp]),
    "ww_mq8_stem_fwd": (C.c_int, [_vp] * 6 + [_i] * 6 + [_vp, _vp, _vp]),
    "ww_mq8_se_fwd": (C.c_int, [_vp, _vp] + [_i] * 8 + [_vp] * 12),
    "ww_mq8_gate_fwd": (C.c_int, [_vp, _vp, _vp] + [_i] * 6 + [_vp, _vp]),
    "ww_mq8_head_fwd": (C.c_int, [_vp, _vp] + [_i] * 5 + [_vp] * 4 + [_i, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "ww_mq8_mobilenetv3_workspace_bytes": (_sz, [_i, _i, _i]),
    "ww_mq8_mobilenetv3_fwd": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(Mq8Io), _vp, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "ww_prof_num_classes": (C.c_int, []),
    "ww_prof_class_name": (C.c_char_p, [_i]),
    "ww_ctx_set_deferred_reduce": (C.c_int, [_vp, _i]),
    "ww_deferred_reduce_pending": (C.c_int, [_vp]),
    "ww_deferred_reduce_flush": (C.c_int, [_vp, _vp]),
    "ww_deferred_reduce_discard": (C.c_int, [_vp]),
    "ww_prof_enable": (C.c_int, [_vp, C.c_uint32]),
    "ww_prof_collect": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "ww_prob_threshold": (_u64, [C.c_double]),
    "ww_philox4x32_10": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
}
EXPORTS = tuple(_SIGS)


def lib_path() -> Path:
    return _LIB_PATH


def load():
    """dlopen libwwhip.so (once).  Raises NativeError if it has not been built."""
    global _lib
    if _lib is None:
        if not _LIB_PATH.exists():
            raise NativeError(
                f"{_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(or `make -C {_LIB_PATH.parent}`); there is no CPU fallback for the HIP hot path")
        lib = C.CDLL(os.fspath(_LIB_PATH))
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.ww_abi_version() != ABI_VERSION:
            raise NativeError(f"libwwhip ABI {lib.ww_abi_version()} != binding {ABI_VERSION}: rebuild")
        _lib = lib
    return _lib


def _check(rc, what):
    if rc != 0:
        msg = _lib.ww_last_error().decode(errors="replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise NativeError(f"{what} failed ({rc}): {msg}")


def ctx(device) -> int:
    """Per-device ww_ctx handle (created on first use)."""
    idx = device.index if isinstance(device, torch.device) else torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    h = _ctx.get(idx)
    if h is not None:
        return h
    lib = load()
    if idx not in _ctx:
        h = _vp()
        with torch.cuda.device(idx):
            _check(lib.ww_ctx_create(idx, C.byref(h)), "ww_ctx_create")
        _ctx[idx] = h
    return _ctx[idx]


def _dev(*tensors):
    d = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise NativeError("the HIP hot path needs tensors on an MI355X ('cuda') device; got a CPU tensor "
                              "(there is no CPU fallback)")
        if not t.is_contiguous():
            raise ValueError("non-contiguous tensor passed to the native path")
        d = t.device if d is None else d
        if t.device != d:
            raise ValueError("tensors on different devices")
    return d


def _dev_rows(*tensors):
    """Device check for (B,T,F) row-strided views (validated separately by _bt_rows); no contiguity requirement."""
    d = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise NativeError("the HIP hot path needs tensors on an MI355X ('cuda') device; got a CPU tensor "
                              "(there is no CPU fallback)")
        d = t.device if d is None else d
        if t.device != d:
            raise ValueError("tensors on different devices passed to the native path")
    return d


def _p(t):
    return None if t is None else t.data_ptr()


_ACT = {torch.float32: ACT_F32, torch.bfloat16: ACT_BF16, torch.float16: ACT_F16}


def act_code(dtype) -> int:
    """storage type of the conv-stack activation tensors: 'fp32'/torch.float32 or 'bf16'/torch.bfloat16."""
    if isinstance(dtype, str):
        dtype = {"fp32": torch.float32, "f32": torch.float32, "float32": torch.float32, "bf16": torch.bfloat16,
                 "bfloat16": torch.bfloat16, "fp16": torch.float16, "f16": torch.float16, "float16": torch.float16,
                 "half": torch.float16}.get(dtype.lower())
    if dtype not in _ACT:
        raise ValueError("activation storage must be float32, bfloat16 or float16")
    return _ACT[dtype]


def act_torch_dtype(code):
    return {ACT_BF16: torch.bfloat16, ACT_F16: torch.float16}.get(code, torch.float32)


def _stream(dev):
    """Raw handle of torch's current stream on `dev` (the C-ABI launches on it).  torch.cuda.current_stream(dev).cuda_stream
    builds a Stream object per call (4 us); the raw getter is the same value."""
    idx = dev.index if isinstance(dev, torch.device) else torch.device(dev).index
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice() if idx is None else idx)


class _NullGuard:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NULL_GUARD = _NullGuard()


def _guard(dev):
    """Device guard around a C-ABI call: a no-op when `dev` is already the current device (one process per GPU: always),
    torch.cuda.device(dev) otherwise."""
    idx = dev.index if isinstance(dev, torch.device) else torch.device(dev).index
    if idx is None or idx == torch._C._cuda_getDevice():
        return _NULL_GUARD
    return torch.cuda.device(dev)


def num_frames(n, hop):
    return load().ww_feat_num_frames(n, hop)


MELQ_TAB = 172


def mel_tables(cfg):
    """Host only: the mel filterbank of ``cfg`` as the kernels read it -> dict(start, len (n_mels,) int32; w compact band weights;
    melq_tab (MELQ_TAB,) int32 and melq_w: the matrix-pipe form of the n_fft-1024 kernel, see include/wwhip.h)."""
    import numpy as np
    M = int(cfg.n_mels)
    start, length = np.zeros(M, np.int32), np.zeros(M, np.int32)
    n_w, n_q = C.c_int32(0), C.c_int32(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(load().ww_feat_mel_tables(C.byref(cfg), ptr(start), ptr(length), None, 0, C.byref(n_w), None, None, 0, C.byref(n_q)),
           "ww_feat_mel_tables")
    w, qtab, qw = np.zeros(max(n_w.value, 1), np.float32), np.zeros(MELQ_TAB, np.int32), np.zeros(max(n_q.value, 1), np.float32)
    _check(load().ww_feat_mel_tables(C.byref(cfg), ptr(start), ptr(length), ptr(w), w.size, C.byref(n_w), ptr(qtab), ptr(qw),
                                     qw.size, C.byref(n_q)), "ww_feat_mel_tables")
    return dict(start=start, len=length, w=w[:n_w.value], melq_tab=qtab, melq_w=qw[:n_q.value])


def prob_threshold(p):
    return load().ww_prob_threshold(float(p))


def philox(ctr, key):
    c = (C.c_uint32 * 4)(*ctr)
    k = (C.c_uint32 * 2)(*key)
    o = (C.c_uint32 * 4)()
    load().ww_philox4x32_10(c, k, o)
    return list(o)


def make_feat_cfg(sample_rate=16000, n_fft=1024, hop=160, n_mels=40, n_mfcc=0, f_min=0.0, f_max=0.0, log_eps=1e-6):
    return FeatCfg(sample_rate, n_fft, hop, n_mels, n_mfcc, f_min, f_max, log_eps)


def make_specaug_cfg(freq_mask_param=15, time_mask_param=35, n_freq_masks=2, n_time_masks=2, freq_mask_prob=1.0,
                     time_mask_prob=1.0):
    return SpecAugCfg(freq_mask_param, time_mask_param, n_freq_masks, n_time_masks, freq_mask_prob, time_mask_prob)


def logmel_fwd(wave, cfg: FeatCfg, specaug: SpecAugCfg = None, seed=0, step=0, sample_offset=0, want_idx=False):
    """wave (B,N) f32|i16 cuda -> (B,1,F,T) f32 [, mask_idx (B,K,2) i32]."""
    dev = _dev(wave)
    if wave.dim() != 2:
        raise ValueError(f"waveform batch must be (B,N), got {tuple(wave.shape)}")
    if wave.dtype == torch.float32:
        dt = WAVE_F32
    elif wave.dtype == torch.int16:
        dt = WAVE_I16
    else:
        raise ValueError(f"waveform dtype must be float32 or int16, got {wave.dtype}")
    B, N = wave.shape
    if cfg.hop <= 0:
        raise ValueError("hop must be positive")
    T = 1 + N // cfg.hop
    F = cfg.n_mfcc if cfg.n_mfcc > 0 else cfg.n_mels
    out = torch.empty((B, 1, F, T), dtype=torch.float32, device=dev)
    idx = None
    if want_idx and specaug is not None:
        idx = torch.zeros((B, specaug.n_freq_masks + specaug.n_time_masks, 2), dtype=torch.int32, device=dev)
    with _guard(dev):
        _check(load().ww_logmel_fwd(ctx(dev), _p(wave), dt, B, N, C.byref(cfg), _p(out),
                                    C.byref(specaug) if specaug is not None else None, seed, step, sample_offset,
                                    _p(idx), _stream(dev)), "ww_logmel_fwd")
    return (out, idx) if want_idx else out


def specaug_apply_(x, specaug: SpecAugCfg, seed=0, step=0, sample_offset=0, want_idx=False):
    """in-place on x (B,1,F,T) or (B,F,T) f32 cuda."""
    dev = _dev(x)
    if x.dtype != torch.float32 or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1):
        raise ValueError(f"features must be float32 (B,1,F,T) or (B,F,T), got {x.dtype} {tuple(x.shape)}")
    B, F, T = x.shape[0], x.shape[-2], x.shape[-1]
    idx = None
    if want_idx:
        idx = torch.zeros((B, specaug.n_freq_masks + specaug.n_time_masks, 2), dtype=torch.int32, device=dev)
    with _guard(dev):
        _check(load().ww_specaug_apply(ctx(dev), _p(x), B, F, T, C.byref(specaug), seed, step, sample_offset, _p(idx),
                                       _stream(dev)), "ww_specaug_apply")
    return idx


def audio_rir_spectra(rirs):
    """RIR bank (R,L) f32 cuda -> spectra for the FFT form of ww_audio_augment (compute once per bank)."""
    dev = _dev(rirs)
    if rirs.dim() != 2 or rirs.dtype != torch.float32:
        raise ValueError("rirs must be a float32 (count, length) tensor")
    R, L = rirs.shape
    nbytes = load().ww_audio_rir_spectra_bytes(R)
    spectra = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_audio_rir_spectra(ctx(dev), _p(rirs), R, L, _p(spectra), nbytes, _stream(dev)),
               "ww_audio_rir_spectra")
    return spectra


def audio_augment(wave, rirs, noises, rir_prob, noise_prob, snr_min_db, snr_max_db, seed=0, step=0, sample_offset=0,
                  want_choices=False, rir_spectra=None):
    """wave (B,N) f32 cuda -> augmented copy [, choices int32 (B,4)]; rirs (R,L) / noises (K,Nn) f32 cuda or None.
    ``rir_spectra`` (from ``audio_rir_spectra``) selects the FFT convolution; None the direct time-domain form."""
    dev = _dev(wave, rirs, noises)
    if wave.dim() != 2 or wave.dtype != torch.float32:
        raise ValueError(f"waveform batch must be float32 (B,N), got {wave.dtype} {tuple(wave.shape)}")
    for name, t in (("rirs", rirs), ("noises", noises)):
        if t is not None and (t.dim() != 2 or t.dtype != torch.float32):
            raise ValueError(f"{name} must be a float32 (count, length) tensor")
    B, N = wave.shape
    out = torch.empty_like(wave)
    R, L = (0, 0) if rirs is None else rirs.shape
    K, Nn = (0, 0) if noises is None else noises.shape
    nbytes = load().ww_audio_augment_scratch_bytes(B, N)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    choices = torch.empty((B, 4), dtype=torch.int32, device=dev) if want_choices else None
    cfg = AudioAugCfg(rir_prob, noise_prob, snr_min_db, snr_max_db)
    with _guard(dev):
        _check(load().ww_audio_augment(ctx(dev), _p(wave), _p(out), B, N, _p(rirs), R, L, _p(rir_spectra), _p(noises), K, Nn, C.byref(cfg),
                                       seed, step, sample_offset, _p(choices), _p(scratch), nbytes, _stream(dev)),
               "ww_audio_augment")
    return (out, choices) if want_choices else out


def audio_tsm_max_grains(N, semis_max):
    return load().ww_audio_tsm_max_grains(N, semis_max)


def audio_tsm(wave, stretch_prob, rate_min, rate_max, pitch_prob, semis_min, semis_max, seed=0, step=0, sample_offset=0,
              want_choices=False, delta_out=None, out=None, scratch=None):
    """wave (B,N) f32 cuda -> time-stretched / pitch-shifted copy of the same shape [, choices int32 (B,3): stretched?, float
    bits of the rate, semitones].  ``delta_out``: int16 (B, audio_tsm_max_grains(N, semis_max)) that receives the search
    offsets of the selected clips.  ``out`` / ``scratch`` default to fresh tensors."""
    dev = _dev(wave, delta_out, out, scratch)
    if wave.dim() != 2 or wave.dtype != torch.float32:
        raise ValueError(f"waveform batch must be float32 (B,N), got {wave.dtype} {tuple(wave.shape)}")
    if int(semis_min) != semis_min or int(semis_max) != semis_max:
        raise ValueError(f"pitch shifts are whole semitones, got ({semis_min}, {semis_max})")
    B, N = wave.shape
    semis_min, semis_max = int(semis_min), int(semis_max)
    if out is None:
        out = torch.empty_like(wave)
    elif out.shape != wave.shape or out.dtype != torch.float32:
        raise ValueError("out must be float32 of the waveform's shape")
    if delta_out is not None and (delta_out.dtype != torch.int16 or -12 <= semis_max <= 12 and
                                  tuple(delta_out.shape) != (B, audio_tsm_max_grains(N, semis_max))):
        raise ValueError("delta_out must be int16 (B, audio_tsm_max_grains(N, semis_max))")
    if scratch is None:
        scratch = torch.empty(max(load().ww_audio_tsm_scratch_bytes(B, N, semis_max) // 4, 1), dtype=torch.float32, device=dev)
    choices = torch.empty((B, 3), dtype=torch.int32, device=dev) if want_choices else None
    cfg = AudioTsmCfg(stretch_prob, rate_min, rate_max, pitch_prob, semis_min, semis_max)
    with _guard(dev):
        _check(load().ww_audio_tsm(ctx(dev), _p(wave), _p(out), B, N, C.byref(cfg), seed, step, sample_offset, _p(choices),
                                   _p(delta_out), _p(scratch), scratch.numel() * scratch.element_size(), _stream(dev)),
               "ww_audio_tsm")
    return (out, choices) if want_choices else out


def _lin_check(x, w, bias):
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1] or x.dtype != torch.float32 or w.dtype != torch.float32:
        raise ValueError(f"linear: need float32 x (M,K) and weight (N,K), got {tuple(x.shape)} and {tuple(w.shape)}")
    if bias is not None and (bias.dim() != 1 or bias.shape[0] != w.shape[0] or bias.dtype != torch.float32):
        raise ValueError("linear: bias must be float32 (N,)")


def linear_mfma_fwd(x, w, bias=None, act=LIN_NONE, dropout_p=0.0, seed=0, step=0, sample_offset=0, mode=torch.float32,
                    want_pre=False):
    """y = dropout(act(x @ w.T + bias)) on the matrix cores -> y [, pre]."""
    dev = _dev(x, w, bias)
    _lin_check(x, w, bias)
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=torch.float32, device=dev)
    pre = torch.empty((M, N), dtype=torch.float32, device=dev) if want_pre else None
    epi = LinearEpi(act, dropout_p, seed, step, sample_offset)
    with _guard(dev):
        _check(load().ww_linear_mfma_fwd(ctx(dev), act_code(mode), _p(x.contiguous()), _p(w.contiguous()), _p(bias), M, K, N,
                                         C.byref(epi), _p(pre), _p(y), _stream(dev)), "ww_linear_mfma_fwd")
    return (y, pre) if want_pre else y


def gemm16_nt(a, b, out_dtype=torch.float32):
    """a (M,K) @ b (N,K).T for bf16 / fp16 operands resident in HBM (fp32 accumulation) -> (M,N) float32 or the operand type."""
    dev = _dev(a, b)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or a.dtype != b.dtype or a.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"gemm16_nt: need two bf16 or two fp16 matrices (M,K), (N,K), got {tuple(a.shape)} {a.dtype}, {tuple(b.shape)} {b.dtype}")
    if out_dtype not in (torch.float32, a.dtype):
        raise ValueError("gemm16_nt: out_dtype must be float32 or the operand type")
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty((a.shape[0], b.shape[0]), dtype=out_dtype, device=dev)
    with _guard(dev):
        _check(load().ww_gemm16_nt(ctx(dev), act_code(a.dtype), _p(a), _p(b), _p(out), int(out_dtype == torch.float32),
                                   a.shape[0], b.shape[0], a.shape[1], _stream(dev)), "ww_gemm16_nt")
    return out


def _out(buf, shape, dev):
    """`buf` (a caller's contiguous fp32 tensor of `shape`'s size -- e.g. a gradient-bucket slot) or a fresh tensor."""
    if buf is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if buf.dtype != torch.float32 or not buf.is_contiguous() or buf.numel() != math.prod(shape) or buf.device != dev:
        raise ValueError("output buffer must be a contiguous float32 tensor of the result's size on the same device")
    return buf


# ---- deferred partial sums (include/wwhip.h: ww_ctx_set_deferred_reduce).  The backward nodes of the autograd models queue the
# "sum the partials" step of their weight-gradient kernels; ONE launch at the end of the backward pass (an autograd-engine
# callback) runs them all.  A queued gradient is not valid before the flush, so a node may only defer a gradient that autograd
# ADOPTS without reading it: a fresh bucket slot (models/flat_buckets.grad_slot) of a parameter that has no gradient yet.
_defer = {}          # device -> {"armed": the end-of-backward callback is queued, "keep": partial buffers alive until the flush}


def defer_begin(dev):
    """Called from a backward node: True when partial sums may be deferred in this backward pass (arms the flush callback)."""
    dev = torch.device(dev)
    st = _defer.setdefault(dev, {"armed": False, "keep": []})
    if not st["armed"]:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(lambda d=dev: _defer_end(d))
        except Exception:                          # not inside an autograd backward pass: nothing would flush
            return False
        st["armed"] = True
    return True


def defer_reset(dev):
    """Start of a forward pass: whatever a previous backward pass left queued or armed is stale (that pass raised before its
    end-of-backward callback ran) -- forget it, so the next backward arms a fresh flush.  A forward that runs INSIDE a backward
    pass (a checkpointed region's recompute) leaves the queue alone: it belongs to the running pass, whose callback flushes it."""
    if torch._C._current_graph_task_id() >= 0:
        return
    st = _defer.get(torch.device(dev))
    if st is not None and (st["armed"] or st["keep"]):
        _check(load().ww_deferred_reduce_discard(ctx(torch.device(dev))), "ww_deferred_reduce_discard")
        st["armed"] = False
        st["keep"].clear()


def _defer_end(dev):
    deferred_flush(dev)
    _defer[dev]["armed"] = False


def deferred_flush(dev):
    """Run everything queued so far as one launch on the current stream (also used before a mid-backward all-reduce)."""
    dev = torch.device(dev)
    st = _defer.get(dev)
    if st is None or not st["keep"]:
        return
    with _guard(dev):
        _check(load().ww_deferred_reduce_flush(ctx(dev), _stream(dev)), "ww_deferred_reduce_flush")
    st["keep"].clear()


class _deferring:
    """with _deferring(dev, scratch): the C call inside queues its partial-sum step; `scratch` lives until the flush."""

    def __init__(self, dev, *keep):
        self.dev, self.keep = torch.device(dev), keep

    def __enter__(self):
        _check(load().ww_ctx_set_deferred_reduce(ctx(self.dev), 1), "ww_ctx_set_deferred_reduce")

    def __exit__(self, *exc):
        load().ww_ctx_set_deferred_reduce(ctx(self.dev), 0)
        _defer.setdefault(self.dev, {"armed": False, "keep": []})["keep"].extend(self.keep)


def linear_mfma_bwd(x, w, pre, dy, act=LIN_NONE, dropout_p=0.0, seed=0, step=0, sample_offset=0, mode=torch.float32,
                    need_dx=True, need_db=True, dw_out=None, db_out=None, defer=False):
    """-> (dx | None, dw, db | None).  dw_out / db_out: write the parameter gradients there (returned as given).
    defer: queue the split-K sum of dw (valid after deferred_flush)."""
    dev = _dev(x, w, pre, dy)
    _lin_check(x, w, None)
    M, K = x.shape
    N = w.shape[0]
    if tuple(dy.shape) != (M, N) or dy.dtype != torch.float32:
        raise ValueError(f"linear backward: dy must be float32 {(M, N)}, got {tuple(dy.shape)}")
    dx = torch.empty((M, K), dtype=torch.float32, device=dev) if need_dx else None
    dw = _out(dw_out, (N, K), dev)
    db = _out(db_out, (N,), dev) if need_db else None
    nbytes = load().ww_linear_mfma_bwd_scratch_bytes(M, K, N)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    epi = LinearEpi(act, dropout_p, seed, step, sample_offset)
    xc, dyc = x.contiguous(), dy.contiguous()
    with _guard(dev), (_deferring(dev, scratch) if defer else contextlib.nullcontext()):
        _check(load().ww_linear_mfma_bwd(ctx(dev), act_code(mode), _p(xc), _p(w.contiguous()), _p(pre),
                                         _p(dyc), M, K, N, C.byref(epi), _p(dx), _p(dw), _p(db), _p(scratch), nbytes,
                                         _stream(dev)), "ww_linear_mfma_bwd")
    return dx, dw, db


def _bt_rows(t, name):
    """(B,T,F) tensor (possibly a column slice of a wider buffer) -> row stride, checking the (b,t) rows are equidistant."""
    if t.dim() != 3 or t.dtype != torch.float32 or t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
        raise ValueError(f"{name} must be float32 (B,T,F) with contiguous features and equidistant (b,t) rows")
    return t.stride(1)


def dropout_bt(x, p, seed=0, step=0, sample_offset=0, stream_id=0, out=None):
    """Philox dropout of a (B,T,C) tensor (rows may be strided); also its own backward when applied to the gradient."""
    dev = _dev_rows(x, out)
    ldx = _bt_rows(x, "x")
    B, T, Cc = x.shape
    if out is None:
        out = torch.empty((B, T, Cc), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_dropout_bt(ctx(dev), _p(x), ldx, B, T, Cc, p, seed, step, sample_offset, stream_id, _p(out),
                                    _bt_rows(out, "out"), _stream(dev)), "ww_dropout_bt")
    return out


# ---- causal dilated Conv1d (TCNWakeword); activations are contiguous fp32 (B, T, C) tensors
def _tconv_check(x, w):
    if x.dim() != 3 or w.dim() != 3 or x.shape[2] != w.shape[1] or x.dtype != torch.float32 or w.dtype != torch.float32:
        raise ValueError(f"tconv1d: need float32 x (B,T,Cin) and weight (Cout,Cin,k), got {tuple(x.shape)} and {tuple(w.shape)}")


def _tconv_scratch(B, T, Cin, Cout, k, dev):
    # (0 bytes = a shape the kernels refuse: the call itself reports which argument)
    return torch.empty(max(load().ww_tconv1d_scratch_bytes(B, T, Cin, Cout, k) // 4, 4), dtype=torch.float32, device=dev)


def tconv1d_fwd(x, w, bias, dilation=1, relu=False, residual=None, mode=torch.float32):
    """y = [relu](causal_conv1d(x, w, dilation) + bias [+ residual]); x (B,T,Cin), w (Cout,Cin,k) -> y (B,T,Cout)."""
    dev = _dev(x, w, bias, residual)
    _tconv_check(x, w)
    B, T, Cin = x.shape
    Cout, _, k = w.shape
    if residual is not None and (tuple(residual.shape) != (B, T, Cout) or residual.dtype != torch.float32):
        raise ValueError(f"tconv1d: residual must be float32 {(B, T, Cout)}, got {tuple(residual.shape)}")
    y = torch.empty((B, T, Cout), dtype=torch.float32, device=dev)
    scratch = _tconv_scratch(B, T, Cin, Cout, k, dev)
    with _guard(dev):
        _check(load().ww_tconv1d_fwd(ctx(dev), act_code(mode), _p(x), _p(w), _p(bias), B, T, Cin, Cout, k, dilation, int(relu),
                                     _p(residual), _p(y), _p(scratch), scratch.numel() * 4, _stream(dev)), "ww_tconv1d_fwd")
    return y


def tconv1d_bwd(x, w, dy, dilation=1, y=None, y2=None, mask_scale=1.0, mode=torch.float32, need_dx=True, dx=None, dw_out=None,
                db_out=None, defer=False):
    """-> (dx | None, dw, db).  y / y2: saved outputs whose zeros mask dy (times mask_scale).  dx given: the input gradient is
    ADDED to it.  defer: queue the sum of the dw partials (valid after deferred_flush)."""
    dev = _dev(x, w, dy, y, y2, dx)
    _tconv_check(x, w)
    B, T, Cin = x.shape
    Cout, _, k = w.shape
    for t in (dy, y, y2):
        if t is not None and (tuple(t.shape) != (B, T, Cout) or t.dtype != torch.float32):
            raise ValueError(f"tconv1d backward: dy / y / y2 must be float32 {(B, T, Cout)}, got {tuple(t.shape)}")
    accumulate = dx is not None
    if dx is None and need_dx:
        dx = torch.empty((B, T, Cin), dtype=torch.float32, device=dev)
    dw = _out(dw_out, (Cout, Cin, k), dev)
    db = _out(db_out, (Cout,), dev)
    scratch = _tconv_scratch(B, T, Cin, Cout, k, dev)
    with _guard(dev), (_deferring(dev, scratch) if defer else contextlib.nullcontext()):
        _check(load().ww_tconv1d_bwd(ctx(dev), act_code(mode), _p(x), _p(w), _p(y), _p(y2), mask_scale, _p(dy), B, T, Cin, Cout, k,
                                     dilation, _p(dx), int(accumulate), _p(dw), _p(db), _p(scratch), scratch.numel() * 4,
                                     _stream(dev)), "ww_tconv1d_bwd")
    return dx, dw, db


def add_relu_fwd(a, b):
    dev = _dev(a, b)
    y = torch.empty_like(a)
    with _guard(dev):
        _check(load().ww_add_relu_fwd(ctx(dev), _p(a), _p(b), a.numel(), _p(y), _stream(dev)), "ww_add_relu_fwd")
    return y


def relu_mask_bwd(dy, y):
    dev = _dev(dy, y)
    dx = torch.empty_like(dy)
    with _guard(dev):
        _check(load().ww_relu_mask_bwd(ctx(dev), _p(dy), _p(y), dy.numel(), _p(dx), _stream(dev)), "ww_relu_mask_bwd")
    return dx


# ---- dense Conv2d, the one-channel stem and MaxPool2d(3, 2, 1) (ResNet18Wakeword); contiguous fp32 (B, H, W, C) activations
def _conv2d_check(x, w):
    if (x.dim() != 4 or w.dim() != 4 or x.shape[3] != w.shape[1] or w.shape[2] != w.shape[3] or x.dtype != torch.float32
            or w.dtype != torch.float32):
        raise ValueError(f"conv2d: need float32 x (B,H,W,Cin) and weight (Cout,Cin,k,k), got {tuple(x.shape)} and {tuple(w.shape)}")


def _conv2d_scratch(B, H, W, Cin, Cout, k, stride, dev):
    # (0 bytes = a shape the kernels refuse: the call itself reports which argument)
    return torch.empty(max(load().ww_conv2d_scratch_bytes(B, H, W, Cin, Cout, k, stride) // 4, 4), dtype=torch.float32, device=dev)


def conv2d_fwd(x, w, stride=1, mode=torch.float32):
    """y = conv2d(x, w, stride, padding=k//2); x (B,H,W,Cin), w (Cout,Cin,k,k) -> y (B,Ho,Wo,Cout)."""
    dev = _dev(x, w)
    _conv2d_check(x, w)
    B, H, W, Cin = x.shape
    Cout, _, k, _ = w.shape
    y = torch.empty((B, *_dw_out_hw(H, W, k, max(stride, 1)), Cout), dtype=torch.float32, device=dev)
    scratch = _conv2d_scratch(B, H, W, Cin, Cout, k, stride, dev)
    with _guard(dev):
        _check(load().ww_conv2d_fwd(ctx(dev), act_code(mode), _p(x), _p(w), B, H, W, Cin, Cout, k, stride, _p(y), _p(scratch),
                                    scratch.numel() * 4, _stream(dev)), "ww_conv2d_fwd")
    return y


def conv2d_bwd(x, w, dy, stride=1, mode=torch.float32, need_dx=True, dx=None, dw_out=None, defer=False, accumulate=True):
    """-> (dx | None, dw).  dx given: the input gradient is ADDED to it (accumulate=False: written over it); else every pixel of
    a fresh dx is written.  defer: queue the sum of the dw partials (valid after deferred_flush)."""
    dev = _dev(x, w, dy, dx)
    _conv2d_check(x, w)
    B, H, W, Cin = x.shape
    Cout, _, k, _ = w.shape
    oshape = (B, *_dw_out_hw(H, W, k, max(stride, 1)), Cout)
    if tuple(dy.shape) != oshape or dy.dtype != torch.float32:
        raise ValueError(f"conv2d backward: dy must be float32 {oshape}, got {tuple(dy.shape)}")
    if dx is not None and (tuple(dx.shape) != tuple(x.shape) or dx.dtype != torch.float32):
        raise ValueError(f"conv2d backward: dx must be float32 {tuple(x.shape)}, got {tuple(dx.shape)}")
    accumulate = bool(accumulate) and dx is not None
    if dx is None and need_dx:
        dx = torch.empty((B, H, W, Cin), dtype=torch.float32, device=dev)
    dw = _out(dw_out, (Cout, Cin, k, k), dev)
    scratch = _conv2d_scratch(B, H, W, Cin, Cout, k, stride, dev)
    with _guard(dev), (_deferring(dev, scratch) if defer else contextlib.nullcontext()):
        _check(load().ww_conv2d_bwd(ctx(dev), act_code(mode), _p(x), _p(w), _p(dy), B, H, W, Cin, Cout, k, stride, _p(dx),
                                    int(accumulate), _p(dw), _p(scratch), scratch.numel() * 4, _stream(dev)), "ww_conv2d_bwd")
    return dx, dw


def _stem_check(x, w):
    if x.dim() != 3 or w.dim() != 4 or w.shape[1] != 1 or w.shape[2] != w.shape[3] or x.dtype != torch.float32 or w.dtype != torch.float32:
        raise ValueError(f"conv2d stem: need float32 x (B,H,W) and weight (C,1,k,k), got {tuple(x.shape)} and {tuple(w.shape)}")


def conv2d_stem_fwd(x, w, stride=2):
    """x (B,H,W) one-channel images, w (C,1,k,k) -> y (B,Ho,Wo,C): Conv2d(1, C, k, stride, k//2, bias=False), direct."""
    dev = _dev(x, w)
    _stem_check(x, w)
    B, H, W = x.shape
    Cn, k = w.shape[0], w.shape[2]
    y = torch.empty((B, *_dw_out_hw(H, W, k, max(stride, 1)), Cn), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_conv2d_stem_fwd(ctx(dev), _p(x), _p(w), B, H, W, Cn, k, stride, _p(y), _stream(dev)), "ww_conv2d_stem_fwd")
    return y


def conv2d_stem_bwd_dw(x, dy, w_shape, stride=2, dw_out=None, defer=False):
    """dw (C,1,k,k) of conv2d_stem_fwd.  defer: queue the sum of the partials (valid after deferred_flush)."""
    dev = _dev(x, dy)
    B, H, W = x.shape
    Cn, _, k, _ = w_shape
    oshape = (B, *_dw_out_hw(H, W, k, max(stride, 1)), Cn)
    if x.dtype != torch.float32 or tuple(dy.shape) != oshape or dy.dtype != torch.float32:
        raise ValueError(f"conv2d stem backward: dy must be float32 {oshape}, got {tuple(dy.shape)}")
    dw = _out(dw_out, tuple(w_shape), dev)
    scratch = torch.empty(max(load().ww_conv2d_stem_scratch_bytes(Cn, k) // 4, 4), dtype=torch.float32, device=dev)
    with _guard(dev), (_deferring(dev, scratch) if defer else contextlib.nullcontext()):
        _check(load().ww_conv2d_stem_bwd_dw(ctx(dev), _p(x), _p(dy), B, H, W, Cn, k, stride, _p(dw), _p(scratch), scratch.numel() * 4,
                                            _stream(dev)), "ww_conv2d_stem_bwd_dw")
    return dw


def maxpool3x3s2_fwd(x):
    """MaxPool2d(3, 2, 1) on x (B,H,W,C) -> (B,(H-1)//2+1,(W-1)//2+1,C)."""
    dev = _dev(x)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"maxpool3x3s2: need float32 x (B,H,W,C), got {tuple(x.shape)}")
    B, H, W, Cn = x.shape
    y = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cn), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_maxpool3x3s2_fwd(ctx(dev), _p(x), B, H, W, Cn, _p(y), _stream(dev)), "ww_maxpool3x3s2_fwd")
    return y


def maxpool3x3s2_bwd(x, dy):
    """dx of maxpool3x3s2_fwd: dy goes to the first maximal element of each window (row-major), recomputed from x."""
    dev = _dev(x, dy)
    B, H, W, Cn = x.shape
    if tuple(dy.shape) != (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cn) or dy.dtype != torch.float32 or x.dtype != torch.float32:
        raise ValueError(f"maxpool3x3s2 backward: dy {tuple(dy.shape)} does not belong to x {tuple(x.shape)}")
    dx = torch.empty_like(x)
    with _guard(dev):
        _check(load().ww_maxpool3x3s2_bwd(ctx(dev), _p(x), _p(dy), B, H, W, Cn, _p(dx), _stream(dev)), "ww_maxpool3x3s2_bwd")
    return dx


# ---- the same layers with 16-bit activation storage (ResNet18Wakeword(storage=...)): activations and their gradients are contiguous
# bf16 / fp16 tensors, the storage code is their dtype's; parameters, weight gradients, BatchNorm vectors and the pooled mean are fp32
def _st_code(*tensors):
    """The storage code of 16-bit activation tensors that must all have one dtype."""
    dt = tensors[0].dtype
    if dt not in (torch.bfloat16, torch.float16) or any(t is not None and t.dtype != dt for t in tensors):
        raise ValueError(f"16-bit activation storage: need bfloat16 or float16 tensors of one dtype, got {[t.dtype for t in tensors if t is not None]}")
    return _ACT[dt]


def _conv2d_st_check(x, w):
    if x.dim() != 4 or w.dim() != 4 or x.shape[3] != w.shape[1] or w.shape[2] != w.shape[3] or w.dtype != torch.float32:
        raise ValueError(f"conv2d: need 16-bit x (B,H,W,Cin) and float32 weight (Cout,Cin,k,k), got {tuple(x.shape)} and {tuple(w.shape)}")


def _conv2d_st_scratch(B, H, W, Cin, Cout, k, stride, dev):
    return torch.empty(max(load().ww_conv2d_st_scratch_bytes(B, H, W, Cin, Cout, k, stride) // 4, 4), dtype=torch.float32, device=dev)


def conv2d_st_fwd(x, w, stride=1, stats=False):
    """y = S(conv2d(x, S(w), stride, padding=k//2)); x (B,H,W,Cin) in S = bf16 | fp16, w (Cout,Cin,k,k) fp32 -> y (B,Ho,Wo,Cout) in S.
    stats: -> (y, part), part (ceil(M / 64), 2 Cout) fp32 = per 64-row tile the column sums of the stored y and of its squares, for
    bn_act_st_fwd(part=...)."""
    dev = _dev(x, w)
    _conv2d_st_check(x, w)
    code = _st_code(x)
    B, H, W, Cin = x.shape
    Cout, _, k, _ = w.shape
    y = torch.empty((B, *_dw_out_hw(H, W, k, max(stride, 1)), Cout), dtype=x.dtype, device=dev)
    scratch = _conv2d_st_scratch(B, H, W, Cin, Cout, k, stride, dev)
    part = torch.empty(((y.numel() // max(Cout, 1) + 63) // 64, 2 * Cout), dtype=torch.float32, device=dev) if stats else None
    with _guard(dev):
        _check(load().ww_conv2d_st_fwd(ctx(dev), code, _p(x), _p(w), B, H, W, Cin, Cout, k, stride, _p(y), _p(part), _p(scratch),
                                       scratch.numel() * 4, _stream(dev)), "ww_conv2d_st_fwd")
    return (y, part) if stats else y


def conv2d_st_bwd(x, w, dy, stride=1, need_dx=True, dx=None, dw_out=None, defer=False, accumulate=True):
    """conv2d_bwd on 16-bit x, dy, dx: -> (dx | None, dw fp32).  dx given: dx = S(dX + float(dx)) (accumulate=False: written over)."""
    dev = _dev(x, w, dy, dx)
    _conv2d_st_check(x, w)
    code = _st_code(x, dy, dx)
    B, H, W, Cin = x.shape
    Cout, _, k, _ = w.shape
    oshape = (B, *_dw_out_hw(H, W, k, max(stride, 1)), Cout)
    if tuple(dy.shape) != oshape:
        raise ValueError(f"conv2d backward: dy must be {oshape}, got {tuple(dy.shape)}")
    if dx is not None and tuple(dx.shape) != tuple(x.shape):
        raise ValueError(f"conv2d backward: dx must be {tuple(x.shape)}, got {tuple(dx.shape)}")
    accumulate = bool(accumulate) and dx is not None
    if dx is None and need_dx:
        dx = torch.empty((B, H, W, Cin), dtype=x.dtype, device=dev)
    dw = _out(dw_out, (Cout, Cin, k, k), dev)
    scratch = _conv2d_st_scratch(B, H, W, Cin, Cout, k, stride, dev)
    with _guard(dev), (_deferring(dev, scratch) if defer else contextlib.nullcontext()):
        _check(load().ww_conv2d_st_bwd(ctx(dev), code, _p(x), _p(w), _p(dy), B, H, W, Cin, Cout, k, stride, _p(dx), int(accumulate),
                                       _p(dw), _p(scratch), scratch.numel() * 4, _stream(dev)), "ww_conv2d_st_bwd")
    return dx, dw


def bn_act_st_fwd(x, bn: BN, act, Cn, res=None, res_ss=None, want_y=True, part=None):
    """x (..., C) in S -> (y | None, ss (2C), mr (2C)): y = S(act(bn(x) + idn)), idn = 0 | res | res * res_ss[:C] + res_ss[C:];
    want_y=False: the statistics only.  part: the statistics partials conv2d_st_fwd(stats=True) left for x."""
    dev = _dev(x, res, res_ss, part)
    if part is not None and (part.dtype != torch.float32 or part.dim() != 2 or part.shape[1] != 2 * Cn):
        raise ValueError("bn_act_st_fwd: part must be float32 (rows, 2C)")
    code = _st_code(x, res)
    if res is not None and res.shape != x.shape:
        raise ValueError(f"bn_act_st_fwd: the residual {tuple(res.shape)} does not have x's shape {tuple(x.shape)}")
    if res_ss is not None and (res_ss.dtype != torch.float32 or res_ss.numel() != 2 * Cn):
        raise ValueError("bn_act_st_fwd: res_ss must be float32 (2C)")
    M = x.numel() // Cn
    y = torch.empty_like(x) if want_y else None
    ss = torch.empty(2 * Cn, dtype=torch.float32, device=dev)
    mr = torch.empty(2 * Cn, dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_bn_act_st_fwd(ctx(dev), code, _p(x), M, Cn, C.byref(bn), act, _p(res), _p(res_ss), _p(part),
                                       0 if part is None else part.shape[0], _p(y), _p(ss), _p(mr),
                                       _p(nhwc_scratch(Cn, dev)), _stream(dev)), "ww_bn_act_st_fwd")
    return y, ss, mr


def bn_act_st_bwd(x, da, ss, mr, act, training, Cn, dgamma_out=None, dbeta_out=None):
    dev = _dev(x, da, ss, mr)
    code = _st_code(x, da)
    if da.shape != x.shape:
        raise ValueError(f"bn_act_st_bwd: da {tuple(da.shape)} does not have x's shape {tuple(x.shape)}")
    M = x.numel() // Cn
    dx = torch.empty_like(x)
    dgamma = _out(dgamma_out, (Cn,), dev)
    dbeta = _out(dbeta_out, (Cn,), dev)
    with _guard(dev):
        _check(load().ww_bn_act_st_bwd(ctx(dev), code, _p(x), _p(da), M, Cn, _p(ss), _p(mr), act, int(training), _p(dx), _p(dgamma),
                                       _p(dbeta), _p(nhwc_scratch(Cn, dev)), _stream(dev)), "ww_bn_act_st_bwd")
    return dx, dgamma, dbeta


def conv2d_stem_st_fwd(x, w, stride=2, storage=torch.bfloat16):
    """conv2d_stem_fwd with the output stored in `storage`: fp32 x (B,H,W), w (C,1,k,k) -> y (B,Ho,Wo,C) = S(conv(x, w))."""
    dev = _dev(x, w)
    _stem_check(x, w)
    B, H, W = x.shape
    Cn, k = w.shape[0], w.shape[2]
    y = torch.empty((B, *_dw_out_hw(H, W, k, max(stride, 1)), Cn), dtype=storage, device=dev)
    with _guard(dev):
        _check(load().ww_conv2d_stem_st_fwd(ctx(dev), _st_code(y), _p(x), _p(w), B, H, W, Cn, k, stride, _p(y), _stream(dev)),
               "ww_conv2d_stem_st_fwd")
    return y


def conv2d_stem_st_bwd_dw(x, dy, w_shape, stride=2, dw_out=None, defer=False):
    """dw (C,1,k,k) fp32 of conv2d_stem_st_fwd from a 16-bit dy."""
    dev = _dev(x, dy)
    B, H, W = x.shape
    Cn, _, k, _ = w_shape
    oshape = (B, *_dw_out_hw(H, W, k, max(stride, 1)), Cn)
    if x.dtype != torch.float32 or tuple(dy.shape) != oshape:
        raise ValueError(f"conv2d stem backward: dy must be {oshape}, got {tuple(dy.shape)}")
    dw = _out(dw_out, tuple(w_shape), dev)
    scratch = torch.empty(max(load().ww_conv2d_stem_scratch_bytes(Cn, k) // 4, 4), dtype=torch.float32, device=dev)
    with _guard(dev), (_deferring(dev, scratch) if defer else contextlib.nullcontext()):
        _check(load().ww_conv2d_stem_st_bwd_dw(ctx(dev), _st_code(dy), _p(x), _p(dy), B, H, W, Cn, k, stride, _p(dw), _p(scratch),
                                               scratch.numel() * 4, _stream(dev)), "ww_conv2d_stem_st_bwd_dw")
    return dw


def maxpool3x3s2_st_fwd(x):
    dev = _dev(x)
    if x.dim() != 4:
        raise ValueError(f"maxpool3x3s2: need x (B,H,W,C), got {tuple(x.shape)}")
    B, H, W, Cn = x.shape
    y = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cn), dtype=x.dtype, device=dev)
    with _guard(dev):
        _check(load().ww_maxpool3x3s2_st_fwd(ctx(dev), _st_code(x), _p(x), B, H, W, Cn, _p(y), _stream(dev)), "ww_maxpool3x3s2_st_fwd")
    return y


def maxpool3x3s2_st_bwd(x, dy):
    dev = _dev(x, dy)
    B, H, W, Cn = x.shape
    if tuple(dy.shape) != (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cn):
        raise ValueError(f"maxpool3x3s2 backward: dy {tuple(dy.shape)} does not belong to x {tuple(x.shape)}")
    dx = torch.empty_like(x)
    with _guard(dev):
        _check(load().ww_maxpool3x3s2_st_bwd(ctx(dev), _st_code(x, dy), _p(x), _p(dy), B, H, W, Cn, _p(dx), _stream(dev)),
               "ww_maxpool3x3s2_st_bwd")
    return dx


def mean_hw_st_fwd(x):
    """x (B,HW,C) in S -> the mean over HW, (B,C) fp32."""
    dev = _dev(x)
    B, HW, Cn = x.shape
    s = torch.empty((B, Cn), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_mean_hw_st_fwd(ctx(dev), _st_code(x), _p(x), B, HW, Cn, _p(s), _stream(dev)), "ww_mean_hw_st_fwd")
    return s


def mean_hw_st_bwd(dmean, HW, storage):
    """dmean (B,C) fp32 -> dx (B,HW,C) = S(dmean / HW)."""
    dev = _dev(dmean)
    if dmean.dim() != 2 or dmean.dtype != torch.float32:
        raise ValueError("mean_hw_st_bwd: need a float32 (B,C) gradient")
    B, Cn = dmean.shape
    dx = torch.empty((B, HW, Cn), dtype=storage, device=dev)
    with _guard(dev):
        _check(load().ww_mean_hw_st_bwd(ctx(dev), _st_code(dx), _p(dmean), B, HW, Cn, _p(dx), _stream(dev)), "ww_mean_hw_st_bwd")
    return dx


def relu_mask_st_bwd(dy, y):
    dev = _dev(dy, y)
    if dy.shape != y.shape:
        raise ValueError("relu_mask_st_bwd: dy and y differ in shape")
    dx = torch.empty_like(dy)
    with _guard(dev):
        _check(load().ww_relu_mask_st_bwd(ctx(dev), _st_code(dy, y), _p(dy), _p(y), dy.numel(), _p(dx), _stream(dev)), "ww_relu_mask_st_bwd")
    return dx


# ---- the causal Conv1d layer with 16-bit activation storage (TCNWakeword(storage=...)): contiguous bf16 / fp16 (B, T, C) tensors
def _tconv_st_check(x, w, *more):
    if x.dim() != 3 or w.dim() != 3 or x.shape[2] != w.shape[1] or w.dtype != torch.float32:
        raise ValueError(f"tconv1d: need 16-bit x (B,T,Cin) and float32 weight (Cout,Cin,k), got {tuple(x.shape)} and {tuple(w.shape)}")
    for t in (x,) + more:
        if t is not None and not t.is_contiguous():
            raise ValueError("tconv1d: 16-bit activation tensors must be contiguous")


def _tconv_st_scratch(code, B, T, Cin, Cout, k, dev):
    return torch.empty(max(load().ww_tconv1d_st_scratch_bytes(code, B, T, Cin, Cout, k) // 4, 4), dtype=torch.float32, device=dev)


def tconv1d_st_fwd(x, w, bias, dilation=1, relu=False, residual=None):
    """y = S([relu](causal_conv1d(x, S(w), dilation) + bias [+ residual])); x (B,T,Cin) and residual in S = bf16 | fp16 -> y in S."""
    dev = _dev(x, w, bias, residual)
    _tconv_st_check(x, w, residual)
    code = _st_code(x, residual)
    B, T, Cin = x.shape
    Cout, _, k = w.shape
    if residual is not None and tuple(residual.shape) != (B, T, Cout):
        raise ValueError(f"tconv1d: residual must be {(B, T, Cout)}, got {tuple(residual.shape)}")
    if bias.dtype != torch.float32 or tuple(bias.shape) != (Cout,):
        raise ValueError(f"tconv1d: bias must be float32 ({Cout},), got {bias.dtype} {tuple(bias.shape)}")
    y = torch.empty((B, T, Cout), dtype=x.dtype, device=dev)
    scratch = _tconv_st_scratch(code, B, T, Cin, Cout, k, dev)
    with _guard(dev):
        _check(load().ww_tconv1d_st_fwd(ctx(dev), code, _p(x), _p(w), _p(bias), B, T, Cin, Cout, k, dilation, int(relu), _p(residual),
                                        _p(y), _p(scratch), scratch.numel() * 4, _stream(dev)), "ww_tconv1d_st_fwd")
    return y


def tconv1d_st_bwd(x, w, dy, dilation=1, y=None, y2=None, mask_scale=1.0, need_dx=True, dx=None, dw_out=None, db_out=None,
                   defer=False):
    """tconv1d_bwd on 16-bit x, dy, y, y2, dx: -> (dx | None, dw fp32, db fp32).  dx given: dx = S(dX + float(dx))."""
    dev = _dev(x, w, dy, y, y2, dx)
    _tconv_st_check(x, w, dy, y, y2, dx)
    code = _st_code(x, dy, y, y2, dx)
    B, T, Cin = x.shape
    Cout, _, k = w.shape
    for t in (dy, y, y2):
        if t is not None and tuple(t.shape) != (B, T, Cout):
            raise ValueError(f"tconv1d backward: dy / y / y2 must be {(B, T, Cout)}, got {tuple(t.shape)}")
    if dx is not None and tuple(dx.shape) != (B, T, Cin):
        raise ValueError(f"tconv1d backward: dx must be {(B, T, Cin)}, got {tuple(dx.shape)}")
    accumulate = dx is not None
    if dx is None and need_dx:
        dx = torch.empty((B, T, Cin), dtype=x.dtype, device=dev)
    dw = _out(dw_out, (Cout, Cin, k), dev)
    db = _out(db_out, (Cout,), dev)
    scratch = _tconv_st_scratch(code, B, T, Cin, Cout, k, dev)
    with _guard(dev), (_deferring(dev, scratch) if defer else contextlib.nullcontext()):
        _check(load().ww_tconv1d_st_bwd(ctx(dev), code, _p(x), _p(w), _p(y), _p(y2), mask_scale, _p(dy), B, T, Cin, Cout, k, dilation,
                                        _p(dx), int(accumulate), _p(dw), _p(db), _p(scratch), scratch.numel() * 4, _stream(dev)),
               "ww_tconv1d_st_bwd")
    return dx, dw, db


def dropout_bt_st(x, p, seed=0, step=0, sample_offset=0, stream_id=0, out=None):
    """dropout_bt on a contiguous 16-bit (B,T,C) tensor: out = S(keep ? x / (1 - p) : 0); out may be x (in place)."""
    dev = _dev(x, out)
    if x.dim() != 3 or not x.is_contiguous() or (out is not None and (out.shape != x.shape or not out.is_contiguous())):
        raise ValueError("dropout_bt_st: need contiguous (B,T,C) tensors of one shape")
    if out is None:
        out = torch.empty_like(x)
    B, T, Cc = x.shape
    with _guard(dev):
        _check(load().ww_dropout_bt_st(ctx(dev), _st_code(x, out), _p(x), B, T, Cc, p, seed, step, sample_offset, stream_id, _p(out),
                                       _stream(dev)), "ww_dropout_bt_st")
    return out


def add_relu_st_fwd(a, b):
    dev = _dev(a, b)
    if a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous():
        raise ValueError("add_relu_st_fwd: need two contiguous tensors of one shape")
    y = torch.empty_like(a)
    with _guard(dev):
        _check(load().ww_add_relu_st_fwd(ctx(dev), _st_code(a, b), _p(a), _p(b), a.numel(), _p(y), _stream(dev)), "ww_add_relu_st_fwd")
    return y


def seq_round_st(x, storage, transposed=True):
    """The network input in S: x float32 (B,F,T) (transposed: also a contiguous (B,1,F,T) batch) or (B,T,F) -> (B,T,F) in S."""
    dev = _dev(x)
    if x.dim() == 4 and x.shape[1] == 1:
        x = x[:, 0]
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"seq_round_st: need a contiguous float32 (B,F,T) or (B,T,F) tensor, got {x.dtype} {tuple(x.shape)}")
    B, T, F = (x.shape[0], x.shape[2], x.shape[1]) if transposed else x.shape
    out = torch.empty((B, T, F), dtype=storage, device=dev)
    with _guard(dev):
        _check(load().ww_seq_round_st(ctx(dev), _st_code(out), _p(x), B, T, F, int(transposed), _p(out), _stream(dev)), "ww_seq_round_st")
    return out


# ---- generic channels-last layers (MobileNetV3 body); activations are contiguous fp32 (M, C) / (B, H, W, C) tensors
_nhwc_scratch = {}


def nhwc_scratch(Cn, dev):
    """Scratch of one layer call, cached per (C, device): calls on one stream are ordered, so the buffer can be shared."""
    key = (Cn, dev)
    buf = _nhwc_scratch.get(key)
    if buf is None:
        buf = _nhwc_scratch[key] = torch.empty(load().ww_nhwc_scratch_bytes(Cn) // 4, dtype=torch.float32, device=dev)
    return buf


def _partials_scratch(Cn, dev, defer):
    """Scratch for a weight-gradient call: a buffer of its own when the sum of the partials is deferred (it must outlive the
    next layer call, which overwrites the cached one), else the cached per-(C, device) scratch."""
    if defer:
        return torch.empty(load().ww_nhwc_scratch_bytes(Cn) // 4, dtype=torch.float32, device=dev)
    return nhwc_scratch(Cn, dev)


def _conv_bn_act_outs(shape, dev):
    """(y pre-BN, a, ss (2C), mr (2C)) of a conv + BatchNorm + activation call whose output has `shape` = (..., C)."""
    new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
    return new(*shape), new(*shape), new(2 * shape[-1]), new(2 * shape[-1])


def _dw_out_hw(H, W, k, stride):
    """Output size of a k x k convolution with padding k // 2."""
    return (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1


def bn_act_fwd(x, bn: BN, act, Cn):
    """x (..., C) -> (y, ss (2C), mr (2C))."""
    dev = _dev(x)
    M = x.numel() // Cn
    y = torch.empty_like(x)
    ss = torch.empty(2 * Cn, dtype=torch.float32, device=dev)
    mr = torch.empty(2 * Cn, dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_bn_act_fwd(ctx(dev), _p(x), M, Cn, C.byref(bn), act, _p(y), _p(ss), _p(mr), _p(nhwc_scratch(Cn, dev)),
                                    _stream(dev)), "ww_bn_act_fwd")
    return y, ss, mr


def bn_act_bwd(x, da, ss, mr, act, training, Cn, dgamma_out=None, dbeta_out=None):
    dev = _dev(x, da, ss, mr)
    M = x.numel() // Cn
    dx = torch.empty_like(x)
    dgamma = _out(dgamma_out, (Cn,), dev)
    dbeta = _out(dbeta_out, (Cn,), dev)
    with _guard(dev):
        _check(load().ww_bn_act_bwd(ctx(dev), _p(x), _p(da), M, Cn, _p(ss), _p(mr), act, int(training), _p(dx), _p(dgamma),
                                    _p(dbeta), _p(nhwc_scratch(Cn, dev)), _stream(dev)), "ww_bn_act_bwd")
    return dx, dgamma, dbeta


def conv1x1_bn_act_fwd(x, w, bn: BN, act, mode=torch.float32, residual=None):
    """Training-mode conv (x (M,K) @ w (N,K)^T) + BatchNorm + activation with the statistics taken in the GEMM's epilogue.
    residual (M,N), optional: added to the activated output in the same pass.  -> (y pre-BN (M,N), a (M,N), ss (2N), mr (2N))."""
    dev = _dev(x, w, residual)
    M, K = x.shape
    N = w.shape[0]
    y, a, ss, mr = _conv_bn_act_outs((M, N), dev)
    scratch = nhwc_scratch(N, dev)
    if scratch.numel() < ((M + 63) // 64) * 2 * N:          # very tall and narrow: a scratch of its own size
        scratch = torch.empty(((M + 63) // 64) * 2 * N, dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_conv1x1_bn_act_fwd(ctx(dev), act_code(mode), _p(x), _p(w), M, K, N, C.byref(bn), act, _p(residual), _p(y), _p(a),
                                            _p(ss), _p(mr), _p(scratch), scratch.numel() * 4, _stream(dev)), "ww_conv1x1_bn_act_fwd")
    return y, a, ss, mr


def dwconv_bn_act_fwd(x, w, k, stride, bn: BN, act):
    """Depthwise conv + BatchNorm + activation -> (y pre-BN, a, ss, mr); the LDS kernel takes the statistics where it applies."""
    dev = _dev(x, w)
    B, H, W, Cn = x.shape
    y, a, ss, mr = _conv_bn_act_outs((B, *_dw_out_hw(H, W, k, stride), Cn), dev)
    with _guard(dev):
        _check(load().ww_dwconv_bn_act_fwd(ctx(dev), _p(x), _p(w), B, H, W, Cn, k, stride, C.byref(bn), act, _p(y), _p(a), _p(ss),
                                           _p(mr), _p(nhwc_scratch(Cn, dev)), _stream(dev)), "ww_dwconv_bn_act_fwd")
    return y, a, ss, mr


def dwconv_nhwc_fwd(x, w, k, stride):
    dev = _dev(x, w)
    B, H, W, Cn = x.shape
    y = torch.empty((B, *_dw_out_hw(H, W, k, stride), Cn), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_dwconv_nhwc_fwd(ctx(dev), _p(x), _p(w), B, H, W, Cn, k, stride, _p(y), _stream(dev)), "ww_dwconv_nhwc_fwd")
    return y


def dwconv_nhwc_bwd(x, w, dy, k, stride, need_dx=True, dw_out=None, defer=False):
    """defer: queue the sum of the weight-gradient partials (dw valid after deferred_flush)."""
    dev = _dev(x, w, dy)
    B, H, W, Cn = x.shape
    dx = torch.empty_like(x) if need_dx else None
    dw = _out(dw_out, tuple(w.shape), dev)
    scratch = _partials_scratch(Cn, dev, defer)
    with _guard(dev), (_deferring(dev, scratch) if defer else contextlib.nullcontext()):
        _check(load().ww_dwconv_nhwc_bwd(ctx(dev), _p(x), _p(w), _p(dy), B, H, W, Cn, k, stride, _p(dx), _p(dw),
                                         _p(scratch), _stream(dev)), "ww_dwconv_nhwc_bwd")
    return dx, dw


def pool_hw_fwd(x):
    dev = _dev(x)
    B, HW, Cn = x.shape
    s = torch.empty((B, Cn), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_pool_hw_fwd(ctx(dev), _p(x), B, HW, Cn, _p(s), _stream(dev)), "ww_pool_hw_fwd")
    return s


def scale_bc_fwd(x, gate):
    dev = _dev(x, gate)
    B, HW, Cn = x.shape
    y = torch.empty_like(x)
    with _guard(dev):
        _check(load().ww_scale_bc_fwd(ctx(dev), _p(x), _p(gate), B, HW, Cn, _p(y), _stream(dev)), "ww_scale_bc_fwd")
    return y


def scale_bc_bwd_gate(x, dy):
    dev = _dev(x, dy)
    B, HW, Cn = x.shape
    dg = torch.empty((B, Cn), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_scale_bc_bwd_gate(ctx(dev), _p(x), _p(dy), B, HW, Cn, _p(dg), _stream(dev)), "ww_scale_bc_bwd_gate")
    return dg


def scale_pool_bwd(dy, gate, dpool, shape):
    """dx (B,HW,C) = dy*gate + dpool/HW (either term may be absent)."""
    dev = _dev(dy, gate, dpool)
    B, HW, Cn = shape
    dx = torch.empty(shape, dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_scale_pool_bwd(ctx(dev), _p(dy), _p(gate), _p(dpool), B, HW, Cn, _p(dx), _stream(dev)),
               "ww_scale_pool_bwd")
    return dx


def se_supported(Cn, Cs, *tensors):
    """Shapes (and 16-byte alignment of the float4-read tensors) the one-launch squeeze-excitation kernels take -- ww_se_fwd's
    documented limits."""
    return (Cn % 4 == 0 and Cs % 4 == 0 and 4 <= Cn <= 1024 and 4 <= Cs <= 256
            and all(t.data_ptr() % 16 == 0 for t in tensors))


def se_fwd(x, w1, b1, w2, b2):
    """x (B,HW,C), w1 (Cs,C), w2 (C,Cs) -> (y, s (B,C), pre1 (B,Cs), pre2 (B,C)); one launch."""
    dev = _dev(x, w1, b1, w2, b2)
    B, HW, Cn = x.shape
    Cs = w1.shape[0]
    y = torch.empty_like(x)
    s = torch.empty((B, Cn), dtype=torch.float32, device=dev)
    pre1 = torch.empty((B, Cs), dtype=torch.float32, device=dev)
    pre2 = torch.empty((B, Cn), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_se_fwd(ctx(dev), _p(x), B, HW, Cn, Cs, _p(w1), _p(b1), _p(w2), _p(b2), _p(y), _p(s), _p(pre1), _p(pre2),
                                _stream(dev)), "ww_se_fwd")
    return y, s, pre1, pre2


def se_bwd(x, dy, s, pre1, pre2, w1, w2, outs=(None, None, None, None)):
    """-> (dx, dw1, db1, dw2, db2); two launches.  outs: optional buffers for (dw1, db1, dw2, db2)."""
    dev = _dev(x, dy, s, pre1, pre2, w1, w2)
    B, HW, Cn = x.shape
    Cs = w1.shape[0]
    dx = torch.empty_like(x)
    dw1, dw2 = _out(outs[0], (Cs, Cn), dev), _out(outs[2], (Cn, Cs), dev)
    db1 = _out(outs[1], (Cs,), dev)
    db2 = _out(outs[3], (Cn,), dev)
    nbytes = load().ww_se_bwd_scratch_bytes(B, Cn, Cs)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_se_bwd(ctx(dev), _p(x), _p(dy), _p(s), _p(pre1), _p(pre2), _p(w1), _p(w2), B, HW, Cn, Cs, _p(dx), _p(dw1),
                                _p(db1), _p(dw2), _p(db2), _p(scratch), nbytes, _stream(dev)), "ww_se_bwd")
    return dx, dw1, db1, dw2, db2


def stem_supported(Cn):
    return Cn % 4 == 0 and 4 <= Cn <= 64


def stem3x3s2_bn_act_fwd(x, w, bn: BN, act):
    """x (B,H,W) one-channel images, w (C,1,3,3): direct 3x3 stride-2 convolution + training-mode BatchNorm + activation.
    -> (y pre-BN (B,Ho,Wo,C), a, ss, mr)."""
    dev = _dev(x, w)
    B, H, W = x.shape
    Cn = w.shape[0]
    y, a, ss, mr = _conv_bn_act_outs((B, (H + 1) // 2, (W + 1) // 2, Cn), dev)
    with _guard(dev):
        _check(load().ww_stem3x3s2_bn_act_fwd(ctx(dev), _p(x), _p(w), B, H, W, Cn, C.byref(bn), act, _p(y), _p(a), _p(ss), _p(mr),
                                              _p(nhwc_scratch(Cn, dev)), _stream(dev)), "ww_stem3x3s2_bn_act_fwd")
    return y, a, ss, mr


def stem3x3s2_bwd_dw(x, dy, w_shape, dw_out=None, defer=False):
    dev = _dev(x, dy)
    B, H, W = x.shape
    Cn = dy.shape[-1]
    dw = _out(dw_out, tuple(w_shape), dev)
    scratch = _partials_scratch(Cn, dev, defer)
    with _guard(dev), (_deferring(dev, scratch) if defer else contextlib.nullcontext()):
        _check(load().ww_stem3x3s2_bwd_dw(ctx(dev), _p(x), _p(dy), B, H, W, Cn, _p(dw), _p(scratch), _stream(dev)),
               "ww_stem3x3s2_bwd_dw")
    return dw


def im2col3x3s2(x):
    """x (B,H,W) one-channel images -> (B*ceil(H/2)*ceil(W/2), 9) patches."""
    dev = _dev(x)
    B, H, W = x.shape
    cols = torch.empty((B * ((H + 1) // 2) * ((W + 1) // 2), 9), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_im2col3x3s2(ctx(dev), _p(x), B, H, W, _p(cols), _stream(dev)), "ww_im2col3x3s2")
    return cols


def add_f32(a, b):
    dev = _dev(a, b)
    y = torch.empty_like(a)
    with _guard(dev):
        _check(load().ww_add_f32(ctx(dev), _p(a), _p(b), a.numel(), _p(y), _stream(dev)), "ww_add_f32")
    return y


# ---- host-only plan queries (include/wwhip.h ww_nhwc_plan_*): what the layer library launches for a shape; no device needed
def _plan(fn, names, *args):
    out = (C.c_int * len(names))()
    _check(getattr(load(), fn)(*args, out), fn)
    return dict(zip(names, out))


def plan_dw(which, B, H, W, Cn, k, stride, aligned=True):
    """which: 'fwd' | 'dx' | 'dw' -> the depthwise launch's plan (LDS kernel or gather, images per workgroup, grid ...)."""
    return _plan("ww_nhwc_plan_dw", ("lds", "V", "grid", "nimg", "G_c", "CC4", "groups", "R"),
                 ("fwd", "dx", "dw").index(which), B, H, W, Cn, k, stride, int(aligned))


def plan_bn(which, M, Cn, chunks=0, training=True, aligned=True):
    """which: 'fwd' | 'bwd' | 'partials' (the BatchNorm half of a conv + BatchNorm call that left `chunks` rows of partials)."""
    return _plan("ww_nhwc_plan_bn", ("chunks", "rows_per_chunk", "R", "fused", "CG4", "G_c", "tile_R", "rows_per_block", "grid", "V"),
                 ("fwd", "bwd", "partials").index(which), M, Cn, chunks, int(training), int(aligned))


def plan_stem(B, H, W, Cn):
    return _plan("ww_nhwc_plan_stem", ("blocks", "L"), B, H, W, Cn)


def plan_ew(n, Cn, aligned=True):
    return _plan("ww_nhwc_plan_ew", ("grid", "V"), n, Cn, int(aligned))


def plan_se(B, HW, Cn, Cs):
    return _plan("ww_se_plan", ("img", "grid"), B, HW, Cn, Cs)


PASS_LAUNCHES = ("ew", "dropout_bt", "wave_windows", "to16_pair")      # WW_PASS_* of include/wwhip.h, in order


def plan_passes(launch, n):
    """The pass plan of a capped-grid support launch over n items (ww_pass_plan; `launch` one of PASS_LAUNCHES) ->
    {grid, per_pass, passes}: workgroups, items one pass of the grid holds, passes the kernel's loop makes."""
    out = (C.c_long * 2)()
    _check(load().ww_pass_plan(PASS_LAUNCHES.index(launch), int(n), out), "ww_pass_plan")
    return {"grid": out[0], "per_pass": out[1], "passes": -(-int(n) // out[1])}


def plan_dw_strips(B, H, W, dtype=torch.float32, wide=False):
    """The dispatch of dwconv3x3_fwd / _bwd for a (B, H, W, 64) tensor (ww_dw_plan) -> {ncs, nseg, hs_len, items, waves,
    interior_waves, addr_bits}; ``wide`` = what set_dw_wide_addr would hold."""
    out = (C.c_long * 7)()
    _check(load().ww_dw_plan(int(B), int(H), int(W), act_code(dtype), int(bool(wide)), out), "ww_dw_plan")
    return dict(zip(("ncs", "nseg", "hs_len", "items", "waves", "interior_waves", "addr_bits"), out))


GEMM_PLAN_FWD = ("epi", "cfg", "shallow", "stage_k", "vecA", "vecB", "gx", "gy", "gz")
GEMM_PLAN_BWD = ("dpre", "dpre_grid", "paired", "refused", "dx_cfg", "dx_shallow", "dw_cfg", "dw_shallow", "kps", "nz", "nbw", "nbx",
                 "splitk_sum", "splitk_grid", "env_pair", "env_pair_tall", "dw_min_rows", "dx_cfg_plain", "splits", "dx_vecA",
                 "dx_vecB", "dw_vecA", "dw_vecB", "db_grid")
PAIR_REFUSALS = ("paired", "off", "dx_cfg2", "dw_tile", "dw_shallow", "tall_off", "no_dx")       # WW_PAIR_* of include/wwhip.h, in order


def plan_gemm(which, M, K, N, mode=torch.float32, full_epilogue=False, aligned=True, need_dx=True):
    """What linear_mfma_fwd (which = "fwd") / linear_mfma_bwd ("bwd") launch for (M, K, N) (ww_gemm_plan: the launchers' own
    dispatch code, no device) -> a dict of GEMM_PLAN_FWD / GEMM_PLAN_BWD; "refused" is one of PAIR_REFUSALS."""
    out = (C.c_long * 24)()
    _check(load().ww_gemm_plan(("fwd", "bwd").index(which), act_code(mode), int(M), int(K), int(N), int(bool(full_epilogue)),
                               int(bool(aligned)), int(bool(need_dx)), out), "ww_gemm_plan")
    p = dict(zip(GEMM_PLAN_FWD if which == "fwd" else GEMM_PLAN_BWD, out))
    if which == "bwd":
        p["refused"] = PAIR_REFUSALS[p["refused"]]
    return p


def plan_loader(B, n_out):
    """ww_loader_batch's split of a row (ww_loader_plan) -> {S, passes, trips}: workgroups per row, passes of 256 chunks in
    a row, and the trips of workgroup s = 0 .. S-1 of a row."""
    p = _plan("ww_loader_plan", ("S", "passes"), int(B), int(n_out))
    p["trips"] = tuple(len(range(s, p["passes"], p["S"])) for s in range(p["S"]))
    return p


def conv1x1_row_tile(M, K, N, mode=torch.float32):
    """Rows per BatchNorm statistics partial of conv1x1_bn_act_fwd (the GEMM's row tile)."""
    return load().ww_conv1x1_row_tile(act_code(mode), M, K, N)


# ---- recurrent layers (include/wwhip.h ww_gru_* / ww_lstm_*): one implementation, parameterised by the cell's gate count,
# C entry points, per-direction struct and recurrent states (GRU: h; LSTM: h, c).  x (B,T,I) and y / dy (B,T,nd*H) may be
# row-strided views; the states and their gradients are contiguous float32 (B,H) or None (zeros / not wanted).
class _Cell:
    def __init__(self, name, gates, prefix, dir_struct, states):
        self.name, self.gates, self.prefix, self.dir_struct, self.states = name, gates, prefix, dir_struct, states


_GRU = _Cell("GRU", 3, "ww_gru", GruDir, ("h",))
_LSTM = _Cell("LSTM", 4, "ww_lstm", LstmDir, ("h", "c"))


def _rnn_workspace(cell, B, T, I, H, dev):
    n = getattr(load(), cell.prefix + "_workspace_bytes")(B, T, I, H)
    if n == 0:
        raise NativeError(f"{cell.name} shape B={B} T={T} I={I} H={H} is not implemented (hidden size 128 only)")
    return torch.empty(n // 4, dtype=torch.float32, device=dev)


def _state_ok(cell, ts, B, H, what):
    if any(t is not None and (tuple(t.shape) != (B, H) or t.dtype != torch.float32 or not t.is_contiguous()) for t in ts):
        raise ValueError(f"{cell.name} {what} must be contiguous float32 (B,H)")


def _rnn_shapes(cell, x, params, y, nd):
    B, T, I = x.shape
    H = params[0][1].shape[1]
    G = cell.gates * H
    if tuple(y.shape) != (B, T, nd * H) or any(tuple(p[0].shape) != (G, I) or tuple(p[1].shape) != (G, H) for p in params):
        raise ValueError(f"{cell.name} parameter / output shapes do not match (w_ih ({cell.gates}H,I), w_hh ({cell.gates}H,H), "
                         f"y (B,T,{nd if nd > 1 else ''}H))")
    return B, T, I, H


def _rnn_fwd(cell, x, w_ih, w_hh, b_ih, b_hh, y, ws, s0, reverse, mode):
    """One direction; s0: the initial states.  -> the final states."""
    dev = _dev(w_ih, w_hh, b_ih, b_hh, ws, *s0)
    _dev_rows(x, y)
    ldx, ldy = _bt_rows(x, "x"), _bt_rows(y, "y")
    B, T, I, H = _rnn_shapes(cell, x, [(w_ih, w_hh)], y, 1)
    _state_ok(cell, s0, B, H, " / ".join(s + "0" for s in cell.states))
    s_n = [torch.empty((B, H), dtype=torch.float32, device=dev) for _ in cell.states]
    fn = cell.prefix + "_fwd"
    with _guard(dev):
        _check(getattr(load(), fn)(ctx(dev), act_code(mode), _p(x), ldx, _p(w_ih.contiguous()), _p(w_hh.contiguous()), _p(b_ih),
                                   _p(b_hh), *map(_p, s0), B, T, I, H, int(reverse), _p(y), ldy, *map(_p, s_n), _p(ws),
                                   ws.numel() * 4, _stream(dev)), fn)
    return s_n


def _rnn_bwd(cell, x, w_ih, w_hh, dy, ds_n, ws, reverse, dx, accumulate_dx, want_ds0, mode):
    """Backward of the one-direction _rnn_fwd that filled ``ws``: -> (dw_ih, dw_hh, db_ih, db_hh, *ds0)."""
    dev = _dev(w_ih, w_hh, ws, *ds_n)
    _dev_rows(x, dy, dx)
    B, T, I = x.shape
    H = w_hh.shape[1]
    ldx = _bt_rows(x, "x")
    ldy = _bt_rows(dy, "dy") if dy is not None else H
    lddx = _bt_rows(dx, "dx") if dx is not None else I
    _state_ok(cell, ds_n, B, H, " / ".join(f"d{s}_n" for s in cell.states))
    dw_ih, dw_hh = torch.empty_like(w_ih), torch.empty_like(w_hh)
    db_ih, db_hh = (torch.empty(cell.gates * H, dtype=torch.float32, device=dev) for _ in range(2))
    ds0 = [torch.empty((B, H), dtype=torch.float32, device=dev) if want_ds0 else None for _ in cell.states]
    fn = cell.prefix + "_bwd"
    with _guard(dev):
        _check(getattr(load(), fn)(ctx(dev), act_code(mode), _p(x), ldx, _p(w_ih.contiguous()), _p(w_hh.contiguous()), _p(dy), ldy,
                                   *map(_p, ds_n), B, T, I, H, int(reverse), _p(ws), ws.numel() * 4, _p(dx), lddx,
                                   int(accumulate_dx), _p(dw_ih), _p(dw_hh), _p(db_ih), _p(db_hh), *map(_p, ds0), _stream(dev)), fn)
    return (dw_ih, dw_hh, db_ih, db_hh, *ds0)


def _rnn_bidir_fwd(cell, x, params, y, ws, s0, mode):
    """Both directions, ONE recurrent launch; s0[j] = [(B,H) | None] x 2 for state j.  -> s_n[j] = [forward, reverse]."""
    dev = _dev(*params[0], *params[1], ws[0], ws[1], *(t for s in s0 for t in s))
    _dev_rows(x, y)
    ldx, ldy = _bt_rows(x, "x"), _bt_rows(y, "y")
    B, T, I, H = _rnn_shapes(cell, x, params, y, 2)
    _state_ok(cell, [t for s in s0 for t in s], B, H, " / ".join(s + "0" for s in cell.states))
    s_n = [[torch.empty((B, H), dtype=torch.float32, device=dev) for _ in range(2)] for _ in cell.states]
    keep = [[t.contiguous() for t in p] for p in params]
    dirs = (cell.dir_struct * 2)()
    for k in range(2):
        dirs[k].w_ih, dirs[k].w_hh, dirs[k].b_ih, dirs[k].b_hh = (t.data_ptr() for t in keep[k])
        dirs[k].ws = ws[k].data_ptr()
        for j, s in enumerate(cell.states):
            setattr(dirs[k], s + "0", _p(s0[j][k]))
            setattr(dirs[k], s + "_n", s_n[j][k].data_ptr())
    fn = cell.prefix + "_bidir_fwd"
    with _guard(dev):
        _check(getattr(load(), fn)(ctx(dev), act_code(mode), _p(x), ldx, C.byref(dirs), B, T, I, H, _p(y), ldy,
                                   min(ws[0].numel(), ws[1].numel()) * 4, _stream(dev)), fn)
    return s_n


def _rnn_bidir_bwd(cell, x, params, dy, ds_n, ws, dx, mode, outs, defer, ds0):
    """Backward of _rnn_bidir_fwd; ds_n[j] / ds0[j] = [(B,H) | None] x 2 for state j.  -> [(dw_ih, dw_hh, db_ih, db_hh)] x 2."""
    dev = _dev(params[0][0], params[1][0], ws[0], ws[1], *(t for s in ds0 for t in s))
    _dev_rows(x, dy, dx)
    B, T, I = x.shape
    H = params[0][1].shape[1]
    ldx = _bt_rows(x, "x")
    ldy = _bt_rows(dy, "dy") if dy is not None else 2 * H
    lddx = _bt_rows(dx, "dx") if dx is not None else I
    _state_ok(cell, [t for s in ds0 + ds_n for t in s], B, H, "state gradients")
    keep = [[p[0].contiguous(), p[1].contiguous()] for p in params]
    if outs is None:
        outs = [(None, None, None, None)] * 2
    G = cell.gates * H
    grads = [(_out(o[0], tuple(p[0].shape), dev), _out(o[1], tuple(p[1].shape), dev), _out(o[2], (G,), dev), _out(o[3], (G,), dev))
             for p, o in zip(params, outs)]
    dirs = (cell.dir_struct * 2)()
    for k in range(2):
        dirs[k].w_ih, dirs[k].w_hh = keep[k][0].data_ptr(), keep[k][1].data_ptr()
        dirs[k].ws = ws[k].data_ptr()
        for j, s in enumerate(cell.states):
            setattr(dirs[k], f"d{s}_n", _p(ds_n[j][k]))
            setattr(dirs[k], f"d{s}0", _p(ds0[j][k]))
        dirs[k].dw_ih, dirs[k].dw_hh, dirs[k].db_ih, dirs[k].db_hh = (g.data_ptr() for g in grads[k])
    fn = cell.prefix + "_bidir_bwd"
    with _guard(dev), (_deferring(dev, ws[0], ws[1]) if defer else contextlib.nullcontext()):
        _check(getattr(load(), fn)(ctx(dev), act_code(mode), _p(x), ldx, C.byref(dirs), _p(dy), ldy, B, T, I, H,
                                   min(ws[0].numel(), ws[1].numel()) * 4, _p(dx), lddx, _stream(dev)), fn)
    return grads


def gru_workspace(B, T, I, H, dev):
    return _rnn_workspace(_GRU, B, T, I, H, dev)


def gru_fwd(x, w_ih, w_hh, b_ih, b_hh, y, ws, h0=None, reverse=False, mode=torch.float32):
    """One GRU direction: x (B,T,I) -> writes y (B,T,H) (may be a column slice of a (B,T,2H) buffer); returns h_n (B,H)."""
    return _rnn_fwd(_GRU, x, w_ih, w_hh, b_ih, b_hh, y, ws, (h0,), reverse, mode)[0]


def gru_bwd(x, w_ih, w_hh, dy, dh_n, ws, reverse=False, dx=None, accumulate_dx=False, want_dh0=False, mode=torch.float32):
    """Backward of the gru_fwd that filled ``ws``: -> (dw_ih, dw_hh, db_ih, db_hh, dh0 | None); dx written/accumulated in place."""
    return _rnn_bwd(_GRU, x, w_ih, w_hh, dy, (dh_n,), ws, reverse, dx, accumulate_dx, want_dh0, mode)


def gru_bidir_fwd(x, params, y, ws, mode=torch.float32, h0=None):
    """Both directions of a bidirectional layer, ONE recurrent launch: x (B,T,I); params = [(w_ih, w_hh, b_ih, b_hh)] x 2
    (forward, reverse); y (B,T,2H) written; ws = two gru_workspace tensors; h0 = [(B,H) | None] x 2 (None: zeros).
    -> [h_n forward, h_n reverse], each (B,H)."""
    return _rnn_bidir_fwd(_GRU, x, params, y, ws, [h0 or (None, None)], mode)[0]


def gru_bidir_bwd(x, params, dy, dh_n, ws, dx=None, mode=torch.float32, outs=None, defer=False, dh0=None):
    """Backward of gru_bidir_fwd: dy (B,T,2H) or None, dh_n = [(B,H) | None] x 2; dx (B,T,I) written when given.
    -> [(dw_ih, dw_hh, db_ih, db_hh)] x 2.  outs: the same structure of tensors to write the gradients into (bucket slots);
    defer: queue the sums of the weight-gradient / bias partials (valid after deferred_flush; ``ws`` is kept until then);
    dh0 = [(B,H) | None] x 2: where to write the gradient of each direction's h0."""
    return _rnn_bidir_bwd(_GRU, x, params, dy, [dh_n], ws, dx, mode, outs, defer, [dh0 or (None, None)])


def lstm_workspace(B, T, I, H, dev):
    return _rnn_workspace(_LSTM, B, T, I, H, dev)


def lstm_fwd(x, w_ih, w_hh, b_ih, b_hh, y, ws, h0=None, c0=None, reverse=False, mode=torch.float32):
    """One LSTM direction: x (B,T,I) -> writes y (B,T,H) (may be a column slice of a (B,T,2H) buffer); returns (h_n, c_n)."""
    return tuple(_rnn_fwd(_LSTM, x, w_ih, w_hh, b_ih, b_hh, y, ws, (h0, c0), reverse, mode))


def lstm_bwd(x, w_ih, w_hh, dy, dh_n, dc_n, ws, reverse=False, dx=None, accumulate_dx=False, want_dh0=False, mode=torch.float32):
    """Backward of the lstm_fwd that filled ``ws``: -> (dw_ih, dw_hh, db_ih, db_hh, dh0 | None, dc0 | None); dx written or
    accumulated in place."""
    return _rnn_bwd(_LSTM, x, w_ih, w_hh, dy, (dh_n, dc_n), ws, reverse, dx, accumulate_dx, want_dh0, mode)


def lstm_bidir_fwd(x, params, y, ws, mode=torch.float32, h0=None, c0=None):
    """Both directions of a bidirectional layer, ONE recurrent launch: x (B,T,I); params = [(w_ih, w_hh, b_ih, b_hh)] x 2
    (forward, reverse); y (B,T,2H) written; ws = two lstm_workspace tensors; h0 / c0 = [(B,H) | None] x 2 (None: zeros).
    -> ([h_n forward, h_n reverse], [c_n forward, c_n reverse]), each (B,H)."""
    return tuple(_rnn_bidir_fwd(_LSTM, x, params, y, ws, [h0 or (None, None), c0 or (None, None)], mode))


def lstm_bidir_bwd(x, params, dy, dh_n, ws, dx=None, mode=torch.float32, outs=None, defer=False, dh0=None, dc_n=None, dc0=None):
    """Backward of lstm_bidir_fwd: dy (B,T,2H) or None, dh_n / dc_n = [(B,H) | None] x 2; dx (B,T,I) written when given.
    -> [(dw_ih, dw_hh, db_ih, db_hh)] x 2.  outs / defer as in gru_bidir_bwd; dh0 / dc0 = [(B,H) | None] x 2: where to write
    the gradients of each direction's initial states."""
    return _rnn_bidir_bwd(_LSTM, x, params, dy, [dh_n, dc_n or (None, None)], ws, dx, mode, outs, defer,
                          [dh0 or (None, None), dc0 or (None, None)])


def step_ctl_new(dev, step=0, lr=0.0, parity=0):
    """A device control block (uint8[32] tensor) initialised to (step, lr, parity); see include/wwhip.h ww_step_ctl."""
    host = StepCtl(step, lr, parity, 1.0, 0)
    return torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)


def step_ctl_write(ctl, step=None, lr=None, parity=None):
    """Update fields of a control block from the host (small async copies on the current stream, between replays)."""
    if step is not None:
        ctl[0:8].copy_(torch.frombuffer(bytearray(int(step).to_bytes(8, "little")), dtype=torch.uint8), non_blocking=False)
    if lr is not None:
        ctl[8:12].view(torch.float32).fill_(float(lr))
    if parity is not None:
        ctl[12:16].view(torch.int32).fill_(int(parity))


def step_ctl_read(ctl) -> dict:
    s = StepCtl.from_buffer_copy(bytes(ctl.cpu().numpy().tobytes()))
    return {"step": s.step, "lr": s.lr, "parity": s.parity, "loss_scale": s.loss_scale, "growth_tracker": s.growth_tracker}


def set_logmel_workgroups(dev, n: int):
    """Persistent workgroups of the log-mel kernel for the launches that follow on ``dev``: 0 = fill the device (the front
    end alone), n > 0 = at most n (a front end running beside a training step; results do not depend on it)."""
    _check(load().ww_ctx_set_logmel_workgroups(ctx(dev), int(n)), "ww_ctx_set_logmel_workgroups")


def set_grid_cap(dev, n: int):
    """Test / tuning parameter: the persistent conv-stack launches that follow on ``dev`` use at most n workgroups (0 = no
    cap), so a workgroup walks many items.  Read when a launch is issued: a captured graph keeps its grids."""
    _check(load().ww_ctx_set_grid_cap(ctx(dev), int(n)), "ww_ctx_set_grid_cap")


def set_dw_wide_addr(dev, on: bool):
    """Test switch: the depthwise conv launches that follow on ``dev`` take their 64-bit address form whatever the tensor's
    size (False = by size, the default).  Results do not depend on it."""
    _check(load().ww_ctx_set_dw_wide_addr(ctx(dev), int(bool(on))), "ww_ctx_set_dw_wide_addr")


def bind_step_ctl(dev, ctl):
    """Bind (ctl = uint8[32] device tensor) or unbind (None) the device-resident step control of ``dev``'s context."""
    if ctl is not None and (not ctl.is_cuda or ctl.numel() < STEP_CTL_BYTES or ctl.dtype != torch.uint8):
        raise ValueError("the step control block must be a uint8 device tensor of at least 32 bytes")
    _check(load().ww_ctx_bind_step_ctl(ctx(dev), _p(ctl)), "ww_ctx_bind_step_ctl")


def step_ctl_advance(dev):
    with _guard(dev):
        _check(load().ww_step_ctl_advance(ctx(dev), _stream(dev)), "ww_step_ctl_advance")


def clip_optim_step_(cfg: OptimCfg, flat_params, flat_grads, exp_avg, exp_avg_sq, step_state, parity, norm_out=None,
                     stats=None, stats_host=None, found_inf_extra=None, stats_host_alt=None, loss_scale=None):
    """In place: clip flat_grads to cfg.max_norm, then one Adam/AdamW/SGD step on flat_params (skipped on found_inf).
    ``stats_host``: pinned uint8[48] host tensor the kernel copies the step's ww_step_stats into.
    ``found_inf_extra``: float32[1] device tensor; non-zero also skips the step (data parallel: some rank's bad batch)."""
    dev = _dev(flat_params, flat_grads, exp_avg, exp_avg_sq, step_state, norm_out, stats, found_inf_extra, loss_scale)
    if stats_host is not None and not (stats_host.is_pinned() and stats_host.numel() * stats_host.element_size() >= STEP_STATS_BYTES):
        raise ValueError("stats_host must be a pinned host tensor of at least 48 bytes")
    if flat_params.dtype != torch.float32 or flat_grads.dtype != torch.float32 or flat_params.numel() != flat_grads.numel():
        raise ValueError("parameter and gradient buckets must be float32 and of equal length")
    if step_state.dtype != torch.int64 or step_state.numel() != 2:
        raise ValueError("step_state must be an int64 tensor of two elements")
    with _guard(dev):
        _check(load().ww_clip_optim_step(ctx(dev), C.byref(cfg), _p(flat_params), _p(flat_grads), _p(exp_avg), _p(exp_avg_sq),
                                         flat_params.numel(), _p(step_state), parity, _p(norm_out), _p(stats),
                                         None if stats_host is None else C.c_void_p(stats_host.data_ptr()),
                                         None if stats_host_alt is None else C.c_void_p(stats_host_alt.data_ptr()),
                                         _p(found_inf_extra), _p(loss_scale), _stream(dev)), "ww_clip_optim_step")


def layer_scratch(dev):
    return torch.empty(load().ww_layer_scratch_bytes() // 4, dtype=torch.float32, device=dev)


def make_bn(gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, training=True):
    return BN(_p(gamma), _p(beta), _p(running_mean), _p(running_var), momentum, eps, 1 if training else 0)


def conv_stem_fwd(x, w, bn: BN, scratch, act=torch.float32):
    dev = _dev(x, w, scratch)
    B, Hin, Win = x.shape[0], x.shape[-2], x.shape[-1]
    Ho, Wo = (Hin + 1) // 2, (Win + 1) // 2
    y = torch.empty((B, Ho, Wo, 64), dtype=act, device=dev)
    ss = torch.empty(128, dtype=torch.float32, device=dev)
    mr = torch.empty(128, dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_conv_stem_fwd(ctx(dev), act_code(act), _p(x), _p(w), B, Hin, Win, _p(y), C.byref(bn), _p(ss), _p(mr),
                                       _p(scratch), _stream(dev)), "ww_conv_stem_fwd")
    return y, ss, mr


def _conv_fwd(name, y_in, ss_in, w, bn, scratch):
    dev = _dev(y_in, ss_in, w, scratch)
    B, H, W, Cc = y_in.shape
    if Cc != 64:
        raise ValueError("conv stack width is 64")
    y = torch.empty_like(y_in)
    ss = torch.empty(128, dtype=torch.float32, device=dev)
    mr = torch.empty(128, dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(getattr(load(), name)(ctx(dev), act_code(y_in.dtype), _p(y_in), _p(ss_in), _p(w), B, H, W, _p(y), C.byref(bn), _p(ss), _p(mr),
                                     _p(scratch), _stream(dev)), name)
    return y, ss, mr


def dwconv3x3_fwd(y_in, ss_in, w, bn, scratch):
    return _conv_fwd("ww_dwconv3x3_fwd", y_in, ss_in, w, bn, scratch)


def pwconv1x1_fwd(y_in, ss_in, w, bn, scratch):
    return _conv_fwd("ww_pwconv1x1_fwd", y_in, ss_in, w, bn, scratch)


def gap_fwd(y, ss, mr):
    dev = _dev(y, ss, mr)
    B, H, W, _ = y.shape
    pool = torch.empty((B, 3, 64), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_gap_fwd(ctx(dev), act_code(y.dtype), _p(y), _p(ss), _p(mr), B, H, W, _p(pool), _stream(dev)),
               "ww_gap_fwd")
    return pool


def head_fwd(pool, HW, fc_w, fc_b, dropout_p=0.0, training=True, seed=0, step=0, sample_offset=0):
    dev = _dev(pool, fc_w, fc_b)
    B = pool.shape[0]
    pd = torch.empty((B, 64), dtype=torch.float32, device=dev)
    logits = torch.empty((B, 2), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_head_fwd(ctx(dev), _p(pool), B, HW, _p(fc_w), _p(fc_b), dropout_p, int(training), seed, step,
                                  sample_offset, _p(pd), _p(logits), _stream(dev)), "ww_head_fwd")
    return pd, logits


def head_bwd(dlogits, pd, pool, HW, fc_w, gamma_last, mr_last, dropout_p=0.0, training=True, seed=0, step=0,
             sample_offset=0):
    dev = _dev(dlogits, pd, pool, fc_w, gamma_last, mr_last)
    B = pool.shape[0]
    f32 = dict(dtype=torch.float32, device=dev)
    dfc_w, dfc_b = torch.empty((2, 64), **f32), torch.empty(2, **f32)
    dpool, coef = torch.empty((B, 64), **f32), torch.empty(192, **f32)
    dgamma, dbeta = torch.empty(64, **f32), torch.empty(64, **f32)
    with _guard(dev):
        _check(load().ww_head_bwd(ctx(dev), _p(dlogits), _p(pd), _p(pool), B, HW, _p(fc_w), dropout_p, int(training),
                                  seed, step, sample_offset, _p(gamma_last), _p(mr_last), _p(dfc_w), _p(dfc_b),
                                  _p(dpool), _p(coef), _p(dgamma), _p(dbeta), _stream(dev)), "ww_head_bwd")
    return dfc_w, dfc_b, dpool, coef, dgamma, dbeta


def pwconv1x1_bwd(g, dpool, y_out, ss_out, coef, y_in, ss_in, mr_in, gamma_in, w, scratch):
    dev = _dev(g, dpool, y_out, ss_out, coef, y_in, ss_in, mr_in, gamma_in, w, scratch)
    B, H, W, _ = y_out.shape
    f32 = dict(dtype=torch.float32, device=dev)
    g_in, dw = torch.empty_like(y_in), torch.empty((64, 64), **f32)
    coef_in, dgamma, dbeta = torch.empty(192, **f32), torch.empty(64, **f32), torch.empty(64, **f32)
    with _guard(dev):
        _check(load().ww_pwconv1x1_bwd(ctx(dev), act_code(y_out.dtype), _p(g), _p(dpool), _p(y_out), _p(ss_out), _p(coef), _p(y_in), _p(ss_in),
                                       _p(mr_in), _p(gamma_in), _p(w), B, H, W, _p(g_in), _p(dw), _p(coef_in),
                                       _p(dgamma), _p(dbeta), _p(scratch), _stream(dev)), "ww_pwconv1x1_bwd")
    return g_in, dw, coef_in, dgamma, dbeta


def dwconv3x3_bwd(g, y_out, coef, y_in, ss_in, mr_in, gamma_in, w, scratch):
    dev = _dev(g, y_out, coef, y_in, ss_in, mr_in, gamma_in, w, scratch)
    B, H, W, _ = y_out.shape
    f32 = dict(dtype=torch.float32, device=dev)
    g_in, dw = torch.empty_like(y_in), torch.empty((64, 1, 3, 3), **f32)
    coef_in, dgamma, dbeta = torch.empty(192, **f32), torch.empty(64, **f32), torch.empty(64, **f32)
    with _guard(dev):
        _check(load().ww_dwconv3x3_bwd(ctx(dev), act_code(y_out.dtype), _p(g), _p(y_out), _p(coef), _p(y_in), _p(ss_in), _p(mr_in),
                                       _p(gamma_in), _p(w), B, H, W, _p(g_in), _p(dw), _p(coef_in), _p(dgamma),
                                       _p(dbeta), _p(scratch), _stream(dev)), "ww_dwconv3x3_bwd")
    return g_in, dw, coef_in, dgamma, dbeta


def conv_stem_bwd(g, y_out, coef, x, scratch, w=None):
    """``w`` (the stem weights) selects the form the whole-model backward runs: y_out is recomputed from x, not read."""
    dev = _dev(g, y_out, coef, x, scratch, w)
    B, Hin, Win = x.shape[0], x.shape[-2], x.shape[-1]
    dw = torch.empty((64, 1, 3, 3), dtype=torch.float32, device=dev)
    with _guard(dev):
        if w is None:
            _check(load().ww_conv_stem_bwd(ctx(dev), act_code(y_out.dtype), _p(g), _p(y_out), _p(coef), _p(x), B, Hin, Win, _p(dw),
                                           _p(scratch), _stream(dev)), "ww_conv_stem_bwd")
        else:
            _check(load().ww_conv_stem_bwd_recompute(ctx(dev), act_code(g.dtype), _p(g), _p(w), _p(coef), _p(x), B, Hin, Win,
                                                     _p(dw), _p(scratch), _stream(dev)), "ww_conv_stem_bwd_recompute")
    return dw


def cnn_small_workspace_bytes(B, F, T, act=ACT_F32):
    return load().ww_cnn_small_workspace_bytes(B, F, T, act)


def ptr_array(tensors):
    arr = (_vp * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def cnn_small_fwd(params, x, ws, logits, training, bn_momentum=0.1, bn_eps=1e-5, dropout_p=0.0, seed=0, step=0,
                  sample_offset=0, act=ACT_F32):
    dev = _dev(x, ws, logits)
    B, F, T = x.shape[0], x.shape[-2], x.shape[-1]
    with _guard(dev):
        _check(load().ww_cnn_small_fwd(ctx(dev), act, params, _p(x), B, F, T, int(training), bn_momentum, bn_eps, dropout_p,
                                       seed, step, sample_offset, _p(ws), ws.numel() * ws.element_size(), _p(logits),
                                       _stream(dev)), "ww_cnn_small_fwd")


def cnn_small_bwd(params, grads, x, dlogits, ws, dropout_p=0.0, seed=0, step=0, sample_offset=0, act=ACT_F32,
                  part=BWD_ALL):
    dev = _dev(x, ws, dlogits)
    B, F, T = x.shape[0], x.shape[-2], x.shape[-1]
    with _guard(dev):
        _check(load().ww_cnn_small_bwd(ctx(dev), act, params, grads, _p(x), _p(dlogits), B, F, T, dropout_p, seed, step,
                                       sample_offset, _p(ws), ws.numel() * ws.element_size(), part, _stream(dev)),
               "ww_cnn_small_bwd")


def cnn_front_fwd(params, x, ws, seq, training, bn_momentum=0.1, bn_eps=1e-5, act=ACT_F32):
    dev = _dev(x, ws, seq)
    B, F, T = x.shape[0], x.shape[-2], x.shape[-1]
    with _guard(dev):
        _check(load().ww_cnn_front_fwd(ctx(dev), act, params, _p(x), B, F, T, int(training), bn_momentum, bn_eps, _p(ws),
                                       ws.numel() * ws.element_size(), _p(seq), _stream(dev)), "ww_cnn_front_fwd")


def cnn_front_bwd(params, grads, x, dseq, ws, act=ACT_F32):
    dev = _dev(x, ws, dseq)
    B, F, T = x.shape[0], x.shape[-2], x.shape[-1]
    with _guard(dev):
        _check(load().ww_cnn_front_bwd(ctx(dev), act, params, grads, _p(x), _p(dseq), B, F, T, _p(ws),
                                       ws.numel() * ws.element_size(), _stream(dev)), "ww_cnn_front_bwd")


def ce2_loss_fwd_bwd(logits, targets, kind=LOSS_CE, label_smoothing=0.0, focal_alpha=0.25, focal_gamma=2.0,
                     stats=None, found_inf_out=None, loss_scale=None, loss_scale_slot=0):
    """-> (loss (1,) f32, dlogits (B,2) f32, stats uint8[STEP_STATS_BYTES]).  ``found_inf_out``: float32[1] device tensor
    that also receives the step's found_inf flag (the spare slot of a data-parallel gradient bucket)."""
    dev = _dev(logits, targets, stats, found_inf_out, loss_scale)
    if logits.dim() != 2 or logits.shape[1] != 2 or logits.dtype != torch.float32:
        raise ValueError(f"native loss needs float32 logits of shape (B,2), got {logits.dtype} {tuple(logits.shape)}")
    if targets.dim() != 1 or targets.shape[0] != logits.shape[0] or targets.dtype != torch.int64:
        raise ValueError("targets must be int64 of shape (B,)")
    B = logits.shape[0]
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits)
    if stats is None:
        stats = torch.zeros(STEP_STATS_BYTES, dtype=torch.uint8, device=dev)
    with _guard(dev):
        _check(load().ww_ce2_loss_fwd_bwd(ctx(dev), _p(logits), _p(targets), B, kind, label_smoothing, focal_alpha,
                                          focal_gamma, _p(loss), _p(dl), _p(stats), _p(found_inf_out), _p(loss_scale),
                                          int(loss_scale_slot), _stream(dev)),
               "ww_ce2_loss_fwd_bwd")
    return loss, dl, stats


def ce2_loss_weighted_fwd_bwd(logits, targets, kind=LOSS_CE, label_smoothing=0.0, focal_alpha=0.25, focal_gamma=2.0,
                              class_weight=None, reduction=REDUCE_MEAN, mean_divisor=DIV_BATCH, stats=None, found_inf_out=None,
                              loss_scale=None, loss_scale_slot=0):
    """Per-class weights and mean / sum / none (include/wwhip.h has the table) -> (loss (1,) f32, loss_vec (B,) f32 or None,
    dlogits (B,2) f32, stats uint8[STEP_STATS_BYTES]).  ``class_weight``: float32 device tensor [w_neg, w_pos], read by the
    kernel through its pointer; None = ones.  ``loss_vec`` is returned for REDUCE_NONE only; ``loss`` is then the mean under
    ``mean_divisor``."""
    dev = _dev(logits, targets, class_weight, stats, found_inf_out, loss_scale)
    if logits.dim() != 2 or logits.shape[1] != 2 or logits.dtype != torch.float32:
        raise ValueError(f"native loss needs float32 logits of shape (B,2), got {logits.dtype} {tuple(logits.shape)}")
    if targets.dim() != 1 or targets.shape[0] != logits.shape[0] or targets.dtype != torch.int64:
        raise ValueError("targets must be int64 of shape (B,)")
    if class_weight is not None and (class_weight.dtype != torch.float32 or tuple(class_weight.shape) != (2,)):
        raise ValueError(f"class_weight must be float32 of shape (2,), got {class_weight.dtype} {tuple(class_weight.shape)}")
    B = logits.shape[0]
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    loss_vec = torch.empty(B, dtype=torch.float32, device=dev) if reduction == REDUCE_NONE else None
    dl = torch.empty_like(logits)
    if stats is None:
        stats = torch.zeros(STEP_STATS_BYTES, dtype=torch.uint8, device=dev)
    with _guard(dev):
        _check(load().ww_ce2_loss_weighted_fwd_bwd(ctx(dev), _p(logits), _p(targets), B, kind, label_smoothing, focal_alpha,
                                                   focal_gamma, _p(class_weight), int(reduction), int(mean_divisor), _p(loss),
                                                   _p(loss_vec), _p(dl), _p(stats), _p(found_inf_out), _p(loss_scale),
                                                   int(loss_scale_slot), _stream(dev)),
               "ww_ce2_loss_weighted_fwd_bwd")
    return loss, loss_vec, dl, stats


LOSS_MAX_CLASSES = 64                 # WW_LOSS_MAX_CLASSES


def _num_classes_of(logits, what):
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"{what} needs float32 logits of shape (B,C), got {logits.dtype} {tuple(logits.shape)}")
    C_ = int(logits.shape[1])
    if not 2 <= C_ <= LOSS_MAX_CLASSES:
        raise ValueError(f"{what}: num_classes = {C_} outside [2, {LOSS_MAX_CLASSES}]")
    return C_


def cen_loss_fwd_bwd(logits, targets, kind=LOSS_CE, label_smoothing=0.0, focal_alpha=0.25, focal_gamma=2.0,
                     class_weight=None, reduction=REDUCE_MEAN, mean_divisor=DIV_BATCH, stats=None, found_inf_out=None,
                     loss_scale=None, loss_scale_slot=0, confusion=None):
    """The C-class entry (ww_cen_loss_fwd_bwd; include/wwhip.h has the formulas and the table), C = logits.shape[1] in
    [2, LOSS_MAX_CLASSES] -> (loss (1,) f32, loss_vec (B,) f32 or None, dlogits (B,C) f32, stats uint8[STEP_STATS_BYTES]).
    ``class_weight``: float32 device tensor (C,), read through its pointer; None = ones.  ``confusion``: int64 device tensor
    (C,C) indexed [target, pred] that the launch adds this batch to unless it sets found_inf; None = nothing is counted."""
    C_ = _num_classes_of(logits, "native loss")
    if targets.dim() != 1 or targets.shape[0] != logits.shape[0] or targets.dtype != torch.int64:
        raise ValueError("targets must be int64 of shape (B,)")
    if class_weight is not None and (class_weight.dtype != torch.float32 or tuple(class_weight.shape) != (C_,)):
        raise ValueError(f"class_weight must be float32 of shape ({C_},), got {class_weight.dtype} {tuple(class_weight.shape)}")
    if confusion is not None and (confusion.dtype != torch.int64 or tuple(confusion.shape) != (C_, C_)):
        raise ValueError(f"confusion must be int64 of shape ({C_}, {C_}), got {confusion.dtype} {tuple(confusion.shape)}")
    dev = _dev(logits, targets, class_weight, stats, found_inf_out, loss_scale, confusion)
    B = logits.shape[0]
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    loss_vec = torch.empty(B, dtype=torch.float32, device=dev) if reduction == REDUCE_NONE else None
    dl = torch.empty_like(logits)
    if stats is None:
        stats = torch.zeros(STEP_STATS_BYTES, dtype=torch.uint8, device=dev)
    with _guard(dev):
        _check(load().ww_cen_loss_fwd_bwd(ctx(dev), _p(logits), _p(targets), B, C_, kind, label_smoothing, focal_alpha,
                                          focal_gamma, _p(class_weight), int(reduction), int(mean_divisor), _p(loss),
                                          _p(loss_vec), _p(dl), _p(stats), _p(found_inf_out), _p(confusion), _p(loss_scale),
                                          int(loss_scale_slot), _stream(dev)),
               "ww_cen_loss_fwd_bwd")
    return loss, loss_vec, dl, stats


def grad_norm_clip_(flat, max_norm, norm_out=None, stats=None):
    """clip_grad_norm_ on a flat bucket.  `stats` (uint8[STEP_STATS_BYTES], optional): its grad_norm / found_inf
    fields are updated on the device."""
    dev = _dev(flat, norm_out, stats)
    if norm_out is None and stats is None:
        norm_out = torch.empty(1, dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_grad_norm_clip(ctx(dev), _p(flat), flat.numel(), float(max_norm), _p(norm_out), _p(stats),
                                        _stream(dev)), "ww_grad_norm_clip")
    return norm_out


FOUND_INF_FLOAT_INDEX = StepStats.found_inf.offset // 4

SCORE_LOGITS, SCORE_CONF = 0, 1
EVAL_MAX_THRESHOLDS = 1024
EVAL_COUNTERS = ("tp", "tn", "fp", "fn", "count", "bad_target", "nan_score", "reserved")   # ww_eval_counters: 8 x uint64


def eval_accumulate(scores, targets, thresholds, decision, conf, pred, bins, offset, hist, counters):
    """One batch of the score stage (ww_eval_accumulate), launched on the current stream; nothing is read back.
    scores (B,2) f32 logits or (B,) f32 confidences; targets (B,) i64 or None; thresholds (K,) f64 ascending;
    conf f32 / pred u8 / bins i32|None are dataset-long and written at [offset, offset+B); hist i64 (2,K+1) and
    counters i64 (8,) (EVAL_COUNTERS) are added to."""
    dev = _dev(scores, targets, thresholds, conf, pred, bins, hist, counters)
    if scores.dtype != torch.float32 or not (scores.dim() == 1 or (scores.dim() == 2 and scores.shape[1] == 2)):
        raise ValueError(f"scores must be float32 (B,2) logits or (B,) confidences, got {scores.dtype} {tuple(scores.shape)}")
    kind = SCORE_LOGITS if scores.dim() == 2 else SCORE_CONF
    B, K = scores.shape[0], thresholds.numel()
    if targets is not None and (targets.dtype != torch.int64 or targets.shape != (B,)):
        raise ValueError("targets must be int64 of shape (B,)")
    if thresholds.dtype != torch.float64 or thresholds.dim() != 1:
        raise ValueError("thresholds must be a 1-D float64 tensor")
    if conf.dtype != torch.float32 or pred.dtype != torch.uint8 or (bins is not None and bins.dtype != torch.int32):
        raise ValueError("conf / pred / bins must be float32 / uint8 / int32")
    offset = int(offset)
    if offset < 0 or any(t is not None and (t.dim() != 1 or t.numel() < offset + B) for t in (conf, pred, bins)):
        raise ValueError(f"per-sample outputs must be 1-D and hold offset + B = {offset + B} elements")
    if hist.dtype != torch.int64 or hist.numel() != 2 * (K + 1) or counters.dtype != torch.int64 or counters.numel() != 8:
        raise ValueError(f"hist must be int64 with 2*(K+1) = {2 * (K + 1)} elements and counters int64 with 8")
    with _guard(dev):
        _check(load().ww_eval_accumulate(ctx(dev), _p(scores), kind, _p(targets), B, _p(thresholds), K, float(decision),
                                         _p(conf), _p(pred), _p(bins), offset, _p(hist), _p(counters), _stream(dev)),
               "ww_eval_accumulate")


def eval_accumulate_classes(logits, targets, thresholds, decision, conf, pred, bins, offset, hist, counters):
    """eval_accumulate for logits (B,C), C in [2, LOSS_MAX_CLASSES] (ww_eval_accumulate_classes): the confidence is
    softmax(row)[1], the counters compare targets 0 and 1 with the argmax over C columns, targets 2..C-1 stay out of hist."""
    C_ = _num_classes_of(logits, "eval_accumulate_classes")
    B, K = logits.shape[0], thresholds.numel()
    if targets is not None and (targets.dtype != torch.int64 or targets.shape != (B,)):
        raise ValueError("targets must be int64 of shape (B,)")
    if thresholds.dtype != torch.float64 or thresholds.dim() != 1:
        raise ValueError("thresholds must be a 1-D float64 tensor")
    if conf.dtype != torch.float32 or pred.dtype != torch.uint8 or (bins is not None and bins.dtype != torch.int32):
        raise ValueError("conf / pred / bins must be float32 / uint8 / int32")
    offset = int(offset)
    if offset < 0 or any(t is not None and (t.dim() != 1 or t.numel() < offset + B) for t in (conf, pred, bins)):
        raise ValueError(f"per-sample outputs must be 1-D and hold offset + B = {offset + B} elements")
    if hist.dtype != torch.int64 or hist.numel() != 2 * (K + 1) or counters.dtype != torch.int64 or counters.numel() != 8:
        raise ValueError(f"hist must be int64 with 2*(K+1) = {2 * (K + 1)} elements and counters int64 with 8")
    dev = _dev(logits, targets, thresholds, conf, pred, bins, hist, counters)
    with _guard(dev):
        _check(load().ww_eval_accumulate_classes(ctx(dev), _p(logits), C_, _p(targets), B, _p(thresholds), K, float(decision),
                                                 _p(conf), _p(pred), _p(bins), offset, _p(hist), _p(counters), _stream(dev)),
               "ww_eval_accumulate_classes")


def wave_num_windows(n_samples, chunk):
    return int(load().ww_wave_num_windows(int(n_samples), int(chunk)))


def wave_windows(wave, chunk):
    """wave (S,) f32 cuda -> (out (W,chunk) f32: the 50 %-overlap windows, each divided by its own peak; peaks (W,) f32)."""
    dev = _dev(wave)
    if wave.dim() != 1 or wave.dtype != torch.float32:
        raise ValueError(f"recording must be a 1-D float32 tensor, got {wave.dtype} {tuple(wave.shape)}")
    chunk = int(chunk)
    if chunk < 2:
        raise ValueError("chunk must be at least 2 samples")
    S = wave.shape[0]
    W = wave_num_windows(S, chunk)
    if W >= 2 ** 31:
        raise ValueError(f"{W} windows: scan the recording in pieces")
    out = torch.empty((W, chunk), dtype=torch.float32, device=dev)
    peaks = torch.empty((W,), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_wave_windows(ctx(dev), _p(wave), S, chunk, W, _p(out), _p(peaks), _stream(dev)), "ww_wave_windows")
    return out, peaks


DETECT_MAX_SMOOTH = 64        # WW_DETECT_MAX_SMOOTH
DETECT_TILE = 1024            # WW_DETECT_TILE: windows of the smoothed sequence staged through LDS per trip of ww_detect_accumulate
WAVE_SPLIT_CHUNK = 32768      # WW_WAVE_SPLIT_CHUNK: windows longer than this are cut by several workgroups each
DETECT_COUNTS = ("triggers", "hits", "false_alarms", "duplicates")


def wave_num_windows_hop(n_samples, chunk, hop):
    return int(load().ww_wave_num_windows_hop(int(n_samples), int(chunk), int(hop)))


def wave_windows_at(wave, chunk, hop, w0, n, normalize=True, out=None, peaks=None):
    """wave (S,) f32 cuda -> (out (n,chunk) f32: windows w0 .. w0+n-1 at hop `hop`, each divided by its own peak when
    `normalize` (ww_wave_windows' law) or copied; peaks (n,) f32).  `out` / `peaks` may be passed in to be reused."""
    dev = _dev(wave, out, peaks)
    if wave.dim() != 1 or wave.dtype != torch.float32:
        raise ValueError(f"recording must be a 1-D float32 tensor, got {wave.dtype} {tuple(wave.shape)}")
    chunk, hop, w0, n = int(chunk), int(hop), int(w0), int(n)
    if not 1 <= hop <= chunk:
        raise ValueError(f"hop must be in [1, chunk = {chunk}], got {hop}")
    S = wave.shape[0]
    W = wave_num_windows_hop(S, chunk, hop)
    if w0 < 0 or n < 0 or w0 + n > W or n >= 2 ** 31:
        raise ValueError(f"windows [{w0}, {w0 + n}) are not among the {W} windows of {S} samples")
    if out is None:
        out = torch.empty((n, chunk), dtype=torch.float32, device=dev)
    if peaks is None:
        peaks = torch.empty((n,), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or out.shape != (n, chunk) or peaks.dtype != torch.float32 or peaks.shape != (n,):
        raise ValueError(f"out / peaks must be float32 ({n},{chunk}) / ({n},)")
    with _guard(dev):
        _check(load().ww_wave_windows_at(ctx(dev), _p(wave), S, chunk, hop, w0, n, 1 if normalize else 0, _p(out), _p(peaks),
                                         _stream(dev)), "ww_wave_windows_at")
    return out, peaks


def feat_windows(feat, Tw, step, w0, n, out=None):
    """feat (F,Ttot) f32 cuda -> out (n,1,F,Tw) f32 with out[i,0,f,t] = feat[f, (w0+i)*step + t] (ww_feat_windows)."""
    dev = _dev(feat, out)
    if feat.dim() != 2 or feat.dtype != torch.float32:
        raise ValueError(f"the feature map must be a 2-D float32 tensor, got {feat.dtype} {tuple(feat.shape)}")
    Tw, step, w0, n = int(Tw), int(step), int(w0), int(n)
    F, Ttot = feat.shape
    if F < 1 or Tw < 1 or step < 1 or w0 < 0 or n < 0 or n >= 2 ** 31 or (n > 0 and (w0 + n - 1) * step + Tw > Ttot):
        raise ValueError(f"windows [{w0}, {w0 + n}) of {Tw} columns at step {step} do not fit a ({F},{Ttot}) map")
    if out is None:
        out = torch.empty((n, 1, F, Tw), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or out.shape != (n, 1, F, Tw):
        raise ValueError(f"out must be float32 ({n},1,{F},{Tw})")
    with _guard(dev):
        _check(load().ww_feat_windows(ctx(dev), _p(feat), F, Ttot, Tw, step, w0, n, _p(out), _stream(dev)), "ww_feat_windows")
    return out


def detect_accumulate(conf, M, R, thresholds, decision, events, smoothed, counts, decision_counts, triggers, n_triggers):
    """The detector over one recording's confidences (ww_detect_accumulate), launched on the current stream; nothing is read
    back.  conf (W,) f32; thresholds (K,) f64 ascending; events (E,2) i32 inclusive ascending window intervals or None;
    smoothed (W,) f32 or None; counts i64 (K,4) and decision_counts i64 (4,) (DETECT_COUNTS) are added to; triggers i32
    (max_triggers,) takes the decision threshold's first trigger windows and n_triggers i32 (1,) their full number."""
    dev = _dev(conf, thresholds, events, smoothed, counts, decision_counts, triggers, n_triggers)
    if conf.dim() != 1 or conf.dtype != torch.float32:
        raise ValueError(f"conf must be a 1-D float32 tensor, got {conf.dtype} {tuple(conf.shape)}")
    W, K = conf.shape[0], thresholds.numel()
    if W >= 2 ** 31:
        raise ValueError(f"{W} windows: scan the recording in pieces")
    if thresholds.dtype != torch.float64 or thresholds.dim() != 1:
        raise ValueError("thresholds must be a 1-D float64 tensor")
    E = 0
    if events is not None:
        if events.dtype != torch.int32 or events.dim() != 2 or events.shape[1] != 2:
            raise ValueError("events must be int32 of shape (E,2)")
        E = events.shape[0]
    if smoothed is not None and (smoothed.dtype != torch.float32 or smoothed.shape != (W,)):
        raise ValueError(f"smoothed must be float32 ({W},)")
    if counts.dtype != torch.int64 or counts.numel() != 4 * K or decision_counts.dtype != torch.int64 or decision_counts.numel() != 4:
        raise ValueError(f"counts must be int64 with 4*K = {4 * K} elements and decision_counts int64 with 4")
    if triggers.dtype != torch.int32 or triggers.dim() != 1 or n_triggers.dtype != torch.int32 or n_triggers.numel() != 1:
        raise ValueError("triggers must be 1-D int32 and n_triggers int32 with one element")
    with _guard(dev):
        _check(load().ww_detect_accumulate(ctx(dev), _p(conf), W, int(M), int(R), _p(thresholds), K, float(decision),
                                           _p(events) if E else None, E, _p(smoothed), _p(counts), _p(decision_counts),
                                           _p(triggers) if triggers.numel() else None, triggers.numel(), _p(n_triggers),
                                           _stream(dev)), "ww_detect_accumulate")


SAMPLER_PERM, SAMPLER_TABLE = 0, 1
_U64 = (1 << 64) - 1


def _loader_table(strategy, cdf, n_clips):
    if strategy == SAMPLER_PERM:
        return 0
    if strategy != SAMPLER_TABLE:
        raise ValueError(f"unknown sampler strategy code {strategy}")
    if cdf is None or cdf.dtype != torch.float64 or cdf.dim() != 1 or not 1 <= cdf.numel() <= n_clips:
        raise ValueError("the table sampler needs a 1-D float64 cumulative table of 1..n_clips entries on the device")
    return cdf.numel()


def loader_indices(n_clips, strategy, shuffle, cdf, seed, epoch, rank, world, k0, count, device=None, out=None):
    """Clip indices of samples k0 .. k0+count-1 of `rank` in `epoch` (ww_loader_indices) -> int32 (count,) cuda."""
    if out is None:
        if cdf is None and device is None:
            raise ValueError("loader_indices needs a device, an output tensor or a table")
        out = torch.empty((int(count),), dtype=torch.int32, device=cdf.device if device is None else device)
    dev = _dev(out, cdf)
    if out.dtype != torch.int32 or out.numel() != count:
        raise ValueError("out must be int32 with `count` elements")
    n_cdf = _loader_table(strategy, cdf, n_clips)
    with _guard(dev):
        _check(load().ww_loader_indices(ctx(dev), int(n_clips), int(strategy), int(bool(shuffle)), _p(cdf), n_cdf, int(seed) & _U64,
                                        int(epoch) & _U64, int(rank), int(world), int(k0), int(count), _p(out), _stream(dev)),
               "ww_loader_indices")
    return out


def loader_batch(bank, length, label, strategy, shuffle, training, cdf, seed, epoch, rank, world, k0, out, targets, clip_index):
    """One batch of the loader (ww_loader_batch), launched on the current stream; nothing is read back.  bank (n_clips, L) i16,
    length (n_clips,) i32, label (n_clips,) u8; out (B, n_out) i16 (rows n_out apart, any 2-byte alignment), targets (B,) i64,
    clip_index (B,) i32."""
    dev = _dev(bank, length, label, cdf, out, targets, clip_index)
    if bank.dtype != torch.int16 or bank.dim() != 2 or out.dtype != torch.int16 or out.dim() != 2:
        raise ValueError("bank and out must be 2-D int16")
    n_clips, L = bank.shape
    B, n_out = out.shape
    if n_clips >= 2 ** 31 or L >= 2 ** 31 or n_out >= 2 ** 31:
        raise ValueError("the bank holds at most 2^31-1 clips of 2^31-1 samples")
    if length.dtype != torch.int32 or length.shape != (n_clips,) or label.dtype != torch.uint8 or label.shape != (n_clips,):
        raise ValueError("length must be int32 (n_clips,) and label uint8 (n_clips,)")
    if targets.dtype != torch.int64 or targets.shape != (B,) or clip_index.dtype != torch.int32 or clip_index.shape != (B,):
        raise ValueError("targets must be int64 (B,) and clip_index int32 (B,)")
    n_cdf = _loader_table(strategy, cdf, n_clips)
    with _guard(dev):
        _check(load().ww_loader_batch(ctx(dev), _p(bank), _p(length), _p(label), n_clips, L, int(strategy), int(bool(shuffle)),
                                      int(bool(training)), _p(cdf), n_cdf, int(seed) & _U64, int(epoch) & _U64, int(rank),
                                      int(world), int(k0), B, n_out, _p(out), _p(targets), _p(clip_index), _stream(dev)),
               "ww_loader_batch")


# ---- int8 inference of an exported cnn_small bundle (ww_q8.hip).  Tensors are int8 / int32 / float32 device tensors,
# activations int8 NHWC; conv arguments are (w, bias_eff, mult, shift) as include/wwhip.h lays them out.
def _q8_conv_check(w, bias, mult, shift, taps):
    if w.dtype != torch.int8 or tuple(w.shape) != (taps, 64) or any(t.dtype != torch.int32 or t.numel() != 64
                                                                     for t in (bias, mult, shift)):
        raise ValueError(f"int8 conv parameters: w int8 ({taps},64), bias / mult / shift int32 (64)")


def q8_quantize(x, scale, zero):
    dev = _dev(x)
    if x.dtype != torch.float32:
        raise ValueError("q8_quantize: float32 features")
    out = torch.empty(x.shape, dtype=torch.int8, device=dev)
    with _guard(dev):
        _check(load().ww_q8_quantize(ctx(dev), _p(x), x.numel(), float(scale), int(zero), _p(out), _stream(dev)), "ww_q8_quantize")
    return out


def q8_stem_fwd(xq, w, bias, mult, shift, zero):
    dev = _dev(xq, w, bias, mult, shift)
    _q8_conv_check(w, bias, mult, shift, 9)
    if xq.dtype != torch.int8 or xq.dim() != 3:
        raise ValueError("q8_stem_fwd: int8 (B,F,T) features")
    B, F, T = xq.shape
    out = torch.empty((B, (F + 1) // 2, (T + 1) // 2, 64), dtype=torch.int8, device=dev)
    with _guard(dev):
        _check(load().ww_q8_stem_fwd(ctx(dev), _p(xq), _p(w), _p(bias), _p(mult), _p(shift), B, F, T, int(zero), _p(out),
                                     _stream(dev)), "ww_q8_stem_fwd")
    return out


def _q8_act_check(a):
    if a.dtype != torch.int8 or a.dim() != 4 or a.shape[3] != 64:
        raise ValueError("int8 activations are (B,H,W,64)")


def q8_dwconv3x3_fwd(a, w, bias, mult, shift, zero=-128):
    dev = _dev(a, w, bias, mult, shift)
    _q8_conv_check(w, bias, mult, shift, 9)
    _q8_act_check(a)
    out = torch.empty_like(a)
    with _guard(dev):
        _check(load().ww_q8_dwconv3x3_fwd(ctx(dev), _p(a), _p(w), _p(bias), _p(mult), _p(shift), a.shape[0], a.shape[1], a.shape[2],
                                          int(zero), _p(out), _stream(dev)), "ww_q8_dwconv3x3_fwd")
    return out


def q8_pwconv1x1_fwd(a, w, bias, mult, shift):
    dev = _dev(a, w, bias, mult, shift)
    _q8_conv_check(w, bias, mult, shift, 64)
    _q8_act_check(a)
    out = torch.empty_like(a)
    with _guard(dev):
        _check(load().ww_q8_pwconv1x1_fwd(ctx(dev), _p(a), _p(w), _p(bias), _p(mult), _p(shift), a.numel() // 64, _p(out),
                                          _stream(dev)), "ww_q8_pwconv1x1_fwd")
    return out


def q8_dwpw_fwd(a, dw, pw, zero=-128):
    """``dw`` / ``pw``: (w, bias, mult, shift) of the depthwise and the pointwise conv; one kernel, bit-equal to the pair."""
    dev = _dev(a, *dw, *pw)
    _q8_conv_check(*dw, 9)
    _q8_conv_check(*pw, 64)
    _q8_act_check(a)
    out = torch.empty_like(a)
    with _guard(dev):
        _check(load().ww_q8_dwpw_fwd(ctx(dev), _p(a), *[_p(t) for t in dw], *[_p(t) for t in pw], a.shape[0], a.shape[1], a.shape[2],
                                     int(zero), _p(out), _stream(dev)), "ww_q8_dwpw_fwd")
    return out


def q8_gap_fc_fwd(a, pool_mult, pool_shift, fc_w, fc_bias, fc_scale):
    dev = _dev(a, fc_w, fc_bias, fc_scale)
    _q8_act_check(a)
    if (fc_w.dtype, fc_bias.dtype, fc_scale.dtype) != (torch.int8, torch.int32, torch.float32) or tuple(fc_w.shape) != (2, 64) \
            or fc_bias.numel() != 2 or fc_scale.numel() != 2:
        raise ValueError("q8_gap_fc_fwd: fc_w int8 (2,64), fc_bias int32 (2), fc_scale float32 (2)")
    B = a.shape[0]
    pool = torch.empty((B, 64), dtype=torch.int8, device=dev)
    logits = torch.empty((B, 2), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_q8_gap_fc_fwd(ctx(dev), _p(a), B, a.shape[1] * a.shape[2], int(pool_mult), int(pool_shift), _p(fc_w),
                                       _p(fc_bias), _p(fc_scale), _p(pool), _p(logits), _stream(dev)), "ww_q8_gap_fc_fwd")
    return pool, logits


def q8_cnn_small_workspace_bytes(B, F, T):
    return load().ww_q8_cnn_small_workspace_bytes(B, F, T)


def q8_cnn_small_fwd(tab, io: Q8Io, x, ws, logits, form=Q8_PAIR):
    """``tab``: ``ptr_array`` of the Q8_NPTR bundle tensors; x float32 (B,F,T) or (B,1,F,T); ws uint8; logits float32 (B,2)."""
    dev = _dev(x, ws, logits)
    B, F, T = x.shape[0], x.shape[-2], x.shape[-1]
    with _guard(dev):
        _check(load().ww_q8_cnn_small_fwd(ctx(dev), tab, C.byref(io), _p(x), B, F, T, int(form), _p(ws),
                                          ws.numel() * ws.element_size(), _p(logits), _stream(dev)), "ww_q8_cnn_small_fwd")


def q8_workspace_views(ws, B, F, T):
    """The tensors ww_q8_cnn_small_fwd left in ``ws`` (uint8), by stage name: xq (B,F,T), the nine activations (B,H,W,64)
    in execution order, pool (B,64) -- the layout include/wwhip.h states."""
    H, W = (F + 1) // 2, (T + 1) // 2
    r256 = lambda n: (n + 255) // 256 * 256       # noqa: E731
    i8 = ws.view(torch.int8)
    out, off, act = {"xq": i8[:B * F * T].view(B, F, T)}, r256(B * F * T), B * H * W * 64
    for name in ["stem"] + [f"{k}{j}" for j in range(4) for k in ("dw", "pw")]:
        out[name] = i8[off:off + act].view(B, H, W, 64)
        off += r256(act)
    out["pool"] = i8[off:off + B * 64].view(B, 64)
    return out


# ---- int8 inference of an exported TCNWakeword bundle (ww_q8_tcn.hip).  Activations are int8 (B,T,Cp) rows, Cp a multiple of 64;
# conv arguments are (w (Cpo,k,Cpi), bias_eff, mult, shift), padded as include/wwhip.h lays them out.
def tq8_pad(c):
    return (int(c) + 63) // 64 * 64


def _tq8_act_check(a, what):
    if a.dtype != torch.int8 or a.dim() != 3 or a.shape[2] % 64:
        raise ValueError(f"{what}: int8 activations are (B,T,Cp), Cp a multiple of 64")


def tq8_quantize_bt(x, scale, zero):
    """x float32 (B,F,T) -> int8 (B,T,Fp); the pad channels hold ``zero``."""
    dev = _dev(x)
    if x.dtype != torch.float32 or x.dim() != 3:
        raise ValueError("tq8_quantize_bt: float32 (B,F,T) features")
    B, F, T = x.shape
    out = torch.empty((B, T, tq8_pad(F)), dtype=torch.int8, device=dev)
    with _guard(dev):
        _check(load().ww_tq8_quantize_bt(ctx(dev), _p(x), B, F, T, out.shape[2], float(scale), int(zero), _p(out), _stream(dev)),
               "ww_tq8_quantize_bt")
    return out


def tq8_conv1d_fwd(a, w, bias, mult, shift, dilation, zero=-128, residual=None, res_mult=0, res_shift=0):
    """``residual`` (B,T,Cpo) with its multiplier and shift selects the epilogue that carries the block's add and last ReLU."""
    dev = _dev(a, w, bias, mult, shift, residual)
    _tq8_act_check(a, "tq8_conv1d_fwd")
    if w.dtype != torch.int8 or w.dim() != 3 or w.shape[2] != a.shape[2] or w.shape[0] % 64 or \
            any(t.dtype != torch.int32 or t.numel() != w.shape[0] for t in (bias, mult, shift)):
        raise ValueError("tq8_conv1d_fwd: w int8 (Cpo,k,Cpi), bias / mult / shift int32 (Cpo)")
    B, T, Cpi = a.shape
    Cpo, k = w.shape[0], w.shape[1]
    if residual is not None and (residual.dtype != torch.int8 or tuple(residual.shape) != (B, T, Cpo)):
        raise ValueError("tq8_conv1d_fwd: residual int8 (B,T,Cpo)")
    out = torch.empty((B, T, Cpo), dtype=torch.int8, device=dev)
    with _guard(dev):
        _check(load().ww_tq8_conv1d_fwd(ctx(dev), _p(a), _p(w), _p(bias), _p(mult), _p(shift), B, T, Cpi, Cpo, k, int(dilation),
                                        int(zero), _p(residual), int(res_mult), int(res_shift), _p(out), _stream(dev)),
               "ww_tq8_conv1d_fwd")
    return out


def tq8_skip_add_fwd(a, h2, zero, skip_mult, skip_shift, add_mult, add_shift):
    dev = _dev(a, h2)
    _tq8_act_check(a, "tq8_skip_add_fwd")
    if h2.dtype != torch.int8 or h2.shape != a.shape:
        raise ValueError("tq8_skip_add_fwd: h2 int8 of the input's shape")
    out = torch.empty_like(a)
    with _guard(dev):
        _check(load().ww_tq8_skip_add_fwd(ctx(dev), _p(a), _p(h2), a.shape[0] * a.shape[1], a.shape[2], int(zero), int(skip_mult),
                                          int(skip_shift), int(add_mult), int(add_shift), _p(out), _stream(dev)),
               "ww_tq8_skip_add_fwd")
    return out


def tq8_pool_fc_fwd(a, C_real, pool_mult, pool_shift, fc_w, fc_bias, fc_scale):
    """a int8 (B,T,Cp) with ``C_real`` channels -> (pool int8 (B,C_real), logits float32 (B,num_classes))."""
    dev = _dev(a, fc_w, fc_bias, fc_scale)
    _tq8_act_check(a, "tq8_pool_fc_fwd")
    nc = fc_w.shape[0]
    if (fc_w.dtype, fc_bias.dtype, fc_scale.dtype) != (torch.int8, torch.int32, torch.float32) or \
            tuple(fc_w.shape) != (nc, C_real) or fc_bias.numel() != nc or fc_scale.numel() != nc:
        raise ValueError("tq8_pool_fc_fwd: fc_w int8 (num_classes,C), fc_bias int32 (num_classes), fc_scale float32 (num_classes)")
    B, T, Cp = a.shape
    pool = torch.empty((B, C_real), dtype=torch.int8, device=dev)
    logits = torch.empty((B, nc), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_tq8_pool_fc_fwd(ctx(dev), _p(a), B, T, int(C_real), Cp, int(pool_mult), int(pool_shift), _p(fc_w), _p(fc_bias),
                                         _p(fc_scale), nc, _p(pool), _p(logits), _stream(dev)), "ww_tq8_pool_fc_fwd")
    return pool, logits


def tq8_tcn_workspace_bytes(B, F, T, channels):
    ch = (C.c_int32 * len(channels))(*[int(c) for c in channels])
    return load().ww_tq8_tcn_workspace_bytes(B, F, T, len(channels), ch)


def tq8_tcn_fwd(tab, io: Tq8Io, x, ws, logits):
    """``tab``: ``ptr_array`` of the bundle's tensors (TQ8_BLOCK_NPTR per block, then fc_w, fc_bias, fc_scale); x float32
    (B,F,T) or (B,1,F,T); ws uint8; logits float32 (B,num_classes)."""
    dev = _dev(x, ws, logits)
    with _guard(dev):
        _check(load().ww_tq8_tcn_fwd(ctx(dev), tab, C.byref(io), _p(x), x.shape[0], x.shape[-1], _p(ws),
                                     ws.numel() * ws.element_size(), _p(logits), _stream(dev)), "ww_tq8_tcn_fwd")


def tq8_workspace_views(ws, B, F, T, channels):
    """The tensors ww_tq8_tcn_fwd left in ``ws`` (uint8), by stage name, PADDED: xq (B,T,Fp), per block b{i}.h1, b{i}.h2, b{i}.out
    (B,T,Cp_i), pool (B,C_last) -- the layout include/wwhip.h states."""
    r256 = lambda n: (n + 255) // 256 * 256       # noqa: E731
    i8 = ws.view(torch.int8)
    Fp = tq8_pad(F)
    out, off = {"xq": i8[:B * T * Fp].view(B, T, Fp)}, r256(B * T * Fp)
    for i, c in enumerate(channels):
        n = B * T * tq8_pad(c)
        for s in ("h1", "h2", "out"):
            out[f"b{i}.{s}"] = i8[off:off + n].view(B, T, tq8_pad(c))
            off += r256(n)
    out["pool"] = i8[off:off + B * channels[-1]].view(B, channels[-1])
    return out


# ---- int8 inference of an exported ResNet18Wakeword bundle (ww_q8_resnet.hip).  Activations are int8 NHWC (B,H,W,C), C a multiple
# of 64; conv arguments are (w (Cout,k*k,Cin), bias_eff, mult, shift) as include/wwhip.h lays them out.
def rq8_half(n):
    """The output size of every stride-2 layer of the model: (7, pad 3), (3, pad 1) and (1, pad 0) all give (n - 1) // 2 + 1."""
    return (int(n) - 1) // 2 + 1


def rq8_conv2d_fwd(a, w, bias, mult, shift, k, stride, zero=-128, epilogue=RQ8_RELU, residual=None, res_zero=-128, res_mult=0,
                   res_shift=0):
    """``epilogue``: RQ8_RELU, RQ8_SIGNED (the downsample conv, z_out = 0) or RQ8_ADD with ``residual`` (B,Ho,Wo,Cout), its zero
    point, multiplier and shift: conv2 carrying the block's add and last ReLU."""
    dev = _dev(a, w, bias, mult, shift, residual)
    if a.dtype != torch.int8 or a.dim() != 4 or a.shape[3] % 64:
        raise ValueError("rq8_conv2d_fwd: int8 activations are (B,H,W,C), C a multiple of 64")
    if w.dtype != torch.int8 or w.dim() != 3 or w.shape[2] != a.shape[3] or w.shape[1] != k * k or w.shape[0] % 64 or \
            any(t.dtype != torch.int32 or t.numel() != w.shape[0] for t in (bias, mult, shift)):
        raise ValueError("rq8_conv2d_fwd: w int8 (Cout,k*k,Cin), bias / mult / shift int32 (Cout)")
    B, H, W, Cin = a.shape
    Cout = w.shape[0]
    Ho, Wo = (rq8_half(H), rq8_half(W)) if stride == 2 else (H, W)
    if residual is not None and (residual.dtype != torch.int8 or tuple(residual.shape) != (B, Ho, Wo, Cout)):
        raise ValueError("rq8_conv2d_fwd: residual int8 (B,Ho,Wo,Cout)")
    out = torch.empty((B, Ho, Wo, Cout), dtype=torch.int8, device=dev)
    with _guard(dev):
        _check(load().ww_rq8_conv2d_fwd(ctx(dev), _p(a), _p(w), _p(bias), _p(mult), _p(shift), B, H, W, Cin, Cout, int(k), int(stride),
                                        int(zero), int(epilogue), _p(residual), int(res_zero), int(res_mult), int(res_shift), _p(out),
                                        _stream(dev)), "ww_rq8_conv2d_fwd")
    return out


def rq8_stem_fwd(xq, w, bias, mult, shift, zero):
    dev = _dev(xq, w, bias, mult, shift)
    if xq.dtype != torch.int8 or xq.dim() != 3:
        raise ValueError("rq8_stem_fwd: int8 (B,F,T) features")
    if w.dtype != torch.int8 or tuple(w.shape) != (64, 64) or any(t.dtype != torch.int32 or t.numel() != 64 for t in (bias, mult, shift)):
        raise ValueError("rq8_stem_fwd: w int8 (64,64) [channel][tap, 49 padded to 64], bias / mult / shift int32 (64)")
    B, F, T = xq.shape
    out = torch.empty((B, rq8_half(F), rq8_half(T), 64), dtype=torch.int8, device=dev)
    with _guard(dev):
        _check(load().ww_rq8_stem_fwd(ctx(dev), _p(xq), _p(w), _p(bias), _p(mult), _p(shift), B, F, T, int(zero), _p(out),
                                      _stream(dev)), "ww_rq8_stem_fwd")
    return out


def rq8_maxpool_fwd(a):
    dev = _dev(a)
    if a.dtype != torch.int8 or a.dim() != 4 or a.shape[3] % 16:
        raise ValueError("rq8_maxpool_fwd: int8 activations are (B,H,W,C), C a multiple of 16")
    B, H, W, Cn = a.shape
    out = torch.empty((B, rq8_half(H), rq8_half(W), Cn), dtype=torch.int8, device=dev)
    with _guard(dev):
        _check(load().ww_rq8_maxpool_fwd(ctx(dev), _p(a), B, H, W, Cn, _p(out), _stream(dev)), "ww_rq8_maxpool_fwd")
    return out


def rq8_resnet18_workspace_bytes(B, F, T):
    return load().ww_rq8_resnet18_workspace_bytes(B, F, T)


def rq8_resnet18_fwd(tab, io: Rq8Io, x, ws, logits):
    """``tab``: ``ptr_array`` of the RQ8_NPTR bundle tensors; x float32 (B,F,T) or (B,1,F,T); ws uint8; logits float32
    (B,num_classes)."""
    dev = _dev(x, ws, logits)
    with _guard(dev):
        _check(load().ww_rq8_resnet18_fwd(ctx(dev), tab, C.byref(io), _p(x), x.shape[0], x.shape[-2], x.shape[-1], _p(ws),
                                          ws.numel() * ws.element_size(), _p(logits), _stream(dev)), "ww_rq8_resnet18_fwd")


def rq8_stage_shapes(F, T):
    """[(H, W)] of the stem output, then of stages 1..4 (stage 1 is the max pool's output size)."""
    out = [(rq8_half(F), rq8_half(T))]
    for _ in range(4):
        out.append((rq8_half(out[-1][0]), rq8_half(out[-1][1])))
    return out


def rq8_workspace_views(ws, B, F, T):
    """The tensors ww_rq8_resnet18_fwd left in ``ws`` (uint8), by stage name: xq (B,F,T), stem, pool0, per block l{s}.{b}.h1,
    l{s}.{b}.ds (blocks 0 of stages 2-4) and l{s}.{b}.out, all (B,H,W,C), then pool (B,512) -- the layout include/wwhip.h states."""
    r256 = lambda n: (n + 255) // 256 * 256       # noqa: E731
    i8 = ws.view(torch.int8)
    hw = rq8_stage_shapes(F, T)
    out, off = {}, 0

    def take(name, *shape):
        nonlocal off
        n = 1
        for v in shape:
            n *= v
        out[name] = i8[off:off + n].view(*shape)
        off += r256(n)
    take("xq", B, F, T)
    take("stem", B, *hw[0], 64)
    take("pool0", B, *hw[1], 64)
    for s, planes in enumerate(RQ8_PLANES):
        for b in range(2):
            take(f"l{s + 1}.{b}.h1", B, *hw[s + 1], planes)
            if s > 0 and b == 0:
                take(f"l{s + 1}.{b}.ds", B, *hw[s + 1], planes)
            take(f"l{s + 1}.{b}.out", B, *hw[s + 1], planes)
    take("pool", B, 512)
    return out


# ---- int8 inference of an exported LSTMWakeword bundle (ww_q8_lstm.hip).  Activations are int8 (B,T,Kp) rows, Kp a multiple of 64;
# a layer's tensors are stacked over its directions, as include/wwhip.h lays them out.
def lq8_proj_fwd(a, w, bias, mult, shift):
    """a int8 (B,T,Kp), w int8 (G,Kp), bias (effective) / mult / shift int32 (G), G = 512 or 1024 (an LSTM's gate rows) or 384 or
    768 (a GRU's) -> u int16 (B,T,G)."""
    dev = _dev(a, w, bias, mult, shift)
    _tq8_act_check(a, "lq8_proj_fwd")
    if w.dtype != torch.int8 or w.dim() != 2 or w.shape[1] != a.shape[2] or w.shape[0] not in (384, 512, 768, 1024) or \
            any(t.dtype != torch.int32 or t.numel() != w.shape[0] for t in (bias, mult, shift)):
        raise ValueError("lq8_proj_fwd: w int8 (G,Kp), G = 512 or 1024 (384 or 768 for a GRU), bias / mult / shift int32 (G)")
    B, T, Kp = a.shape
    u = torch.empty((B, T, w.shape[0]), dtype=torch.int16, device=dev)
    with _guard(dev):
        _check(load().ww_lq8_proj_fwd(ctx(dev), _p(a), _p(w), _p(bias), _p(mult), _p(shift), B * T, Kp, w.shape[0], _p(u),
                                      _stream(dev)), "ww_lq8_proj_fwd")
    return u


# what tells the two int8 recurrences apart in the binding: (entry point, gate rows of a direction)
_Q8_LSTM, _Q8_GRU = ("lq8_lstm_layer_fwd", 512), ("cq8_gru_layer_fwd", 384)


def _q8_rnn_layer_fwd(cell, u, w_hh, bias, mult, shift, tab_sigmoid, tab_tanh):
    entry, rows = cell
    dev = _dev(u, w_hh, bias, mult, shift, tab_sigmoid, tab_tanh)
    G = w_hh.shape[0]
    if u.dtype != torch.int16 or u.dim() != 3 or u.shape[2] != G or G not in (rows, 2 * rows) or \
            w_hh.dtype != torch.int8 or tuple(w_hh.shape) != (G, 128) or \
            any(t.dtype != torch.int32 or t.numel() != G for t in (bias, mult, shift)) or \
            any(t.dtype != torch.int16 or t.numel() != 4096 for t in (tab_sigmoid, tab_tanh)) or not u.is_contiguous():
        raise ValueError(f"{entry}: u int16 (B,T,G), w_hh int8 (G,128), bias / mult / shift int32 (G), tables int16 (4096)")
    B, T, nd = u.shape[0], u.shape[1], G // rows
    y = torch.empty((B, T, nd * 128), dtype=torch.int8, device=dev)
    s_n = torch.empty((B, nd * 128), dtype=torch.int16, device=dev)
    with _guard(dev):
        _check(getattr(load(), "ww_" + entry)(ctx(dev), _p(u), _p(w_hh), _p(bias), _p(mult), _p(shift), _p(tab_sigmoid), _p(tab_tanh),
                                              B, T, nd, _p(y), _p(s_n), _stream(dev)), "ww_" + entry)
    return y, s_n


def lq8_lstm_layer_fwd(u, w_hh, bias, mult, shift, tab_sigmoid, tab_tanh):
    """u int16 (B,T,nd*512), w_hh int8 (nd*512,128), bias / mult / shift int32 (nd*512), the two int16 (4096) tables ->
    (y int8 (B,T,nd*128), c_n int16 (B,nd*128))."""
    return _q8_rnn_layer_fwd(_Q8_LSTM, u, w_hh, bias, mult, shift, tab_sigmoid, tab_tanh)


def lq8_head_fwd(y, fc_w, fc_bias, fc_scale):
    """y int8 (B,T,nd*128) -> (hcat int8 (B,nd*128), logits float32 (B,num_classes))."""
    dev = _dev(y, fc_w, fc_bias, fc_scale)
    nc = fc_w.shape[0]
    if y.dtype != torch.int8 or y.dim() != 3 or y.shape[2] not in (128, 256) or \
            (fc_w.dtype, fc_bias.dtype, fc_scale.dtype) != (torch.int8, torch.int32, torch.float32) or \
            tuple(fc_w.shape) != (nc, y.shape[2]) or fc_bias.numel() != nc or fc_scale.numel() != nc:
        raise ValueError("lq8_head_fwd: y int8 (B,T,nd*128), fc_w int8 (num_classes,nd*128), fc_bias int32, fc_scale float32")
    B, T, Cn = y.shape
    hcat = torch.empty((B, Cn), dtype=torch.int8, device=dev)
    logits = torch.empty((B, nc), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_lq8_head_fwd(ctx(dev), _p(y), B, T, Cn // 128, _p(fc_w), _p(fc_bias), _p(fc_scale), nc, _p(hcat), _p(logits),
                                      _stream(dev)), "ww_lq8_head_fwd")
    return hcat, logits


def lq8_lstm_workspace_bytes(B, T, input_size, num_layers, num_directions):
    return load().ww_lq8_lstm_workspace_bytes(B, T, input_size, num_layers, num_directions)


def lq8_lstm_fwd(tab, io: Lq8Io, x, ws, logits):
    """``tab``: ``ptr_array`` of the bundle's tensors (LQ8_LAYER_NPTR per layer, then fc_w, fc_bias, fc_scale, tab_sigmoid,
    tab_tanh); x float32 (B,F,T); ws uint8; logits float32 (B,num_classes)."""
    dev = _dev(x, ws, logits)
    with _guard(dev):
        _check(load().ww_lq8_lstm_fwd(ctx(dev), tab, C.byref(io), _p(x), x.shape[0], x.shape[-1], _p(ws),
                                      ws.numel() * ws.element_size(), _p(logits), _stream(dev)), "ww_lq8_lstm_fwd")


def _r256(n):
    return (n + 255) // 256 * 256


def _q8_rnn_views(out, i8, off, B, T, num_layers, nd, rows, state):
    """Carves the per-layer u | y | state regions of a recurrent stack from ``i8`` at byte ``off`` into ``out``; returns the offset
    past the last layer."""
    for k in range(num_layers):
        for name, dtype, shape in ((f"l{k}.u", torch.int16, (B, T, nd * rows)), (f"l{k}.y", torch.int8, (B, T, nd * 128)),
                                   (f"l{k}.{state}", torch.int16, (B, nd * 128))):
            n = math.prod(shape) * dtype.itemsize
            out[name] = i8[off:off + n].view(dtype).view(shape)
            off += _r256(n)
    return off


def lq8_workspace_views(ws, B, T, input_size, num_layers, num_directions):
    """The tensors ww_lq8_lstm_fwd left in ``ws`` (uint8), by stage name: xq (B,T,Fp) PADDED, per layer l{k}.u int16 (B,T,nd*512),
    l{k}.y int8 (B,T,nd*128) and l{k}.c int16 (B,nd*128), directions stacked, then hcat (B,nd*128) -- the layout include/wwhip.h
    states."""
    i8, nd = ws.view(torch.int8), num_directions
    Fp = tq8_pad(input_size)
    out, off = {"xq": i8[:B * T * Fp].view(B, T, Fp)}, _r256(B * T * Fp)
    off = _q8_rnn_views(out, i8, off, B, T, num_layers, nd, 512, "c")
    out["hcat"] = i8[off:off + B * nd * 128].view(B, nd * 128)
    return out


# ---- int8 inference of an exported CRNNWakeword bundle (ww_q8_crnn.hip).  The conv stack is the q8_* family's, the projection
# lq8_proj_fwd at G = nd*384, the head lq8_head_fwd; a layer's tensors are stacked over its directions.
def cq8_fmean_fwd(a, mult, shift):
    """a int8 (B,H,W,64), z = -128 -> the frequency mean, int8 (B,W,64) rows."""
    dev = _dev(a)
    _q8_act_check(a)
    if not a.is_contiguous():
        raise ValueError("cq8_fmean_fwd: contiguous activations")
    B, H, W, _ = a.shape
    out = torch.empty((B, W, 64), dtype=torch.int8, device=dev)
    with _guard(dev):
        _check(load().ww_cq8_fmean_fwd(ctx(dev), _p(a), B, H, W, int(mult), int(shift), _p(out), _stream(dev)), "ww_cq8_fmean_fwd")
    return out


def cq8_gru_layer_fwd(u, w_hh, bias, mult, shift, tab_sigmoid, tab_tanh):
    """u int16 (B,T,nd*384), w_hh int8 (nd*384,128), bias / mult / shift int32 (nd*384), the two int16 (4096) tables ->
    (y int8 (B,T,nd*128), h_n int16 (B,nd*128))."""
    return _q8_rnn_layer_fwd(_Q8_GRU, u, w_hh, bias, mult, shift, tab_sigmoid, tab_tanh)


def cq8_crnn_workspace_bytes(B, F, T, num_layers, num_directions):
    return load().ww_cq8_crnn_workspace_bytes(B, F, T, num_layers, num_directions)


def cq8_crnn_fwd(tab, io: Cq8Io, x, ws, logits):
    """``tab``: ``ptr_array`` of the bundle's tensors (CQ8_CONV_NPTR of the conv stack, CQ8_LAYER_NPTR per layer, then fc_w,
    fc_bias, fc_scale, tab_sigmoid, tab_tanh); x float32 (B,F,T); ws uint8; logits float32 (B,num_classes)."""
    dev = _dev(x, ws, logits)
    with _guard(dev):
        _check(load().ww_cq8_crnn_fwd(ctx(dev), tab, C.byref(io), _p(x), x.shape[0], x.shape[-2], x.shape[-1], _p(ws),
                                      ws.numel() * ws.element_size(), _p(logits), _stream(dev)), "ww_cq8_crnn_fwd")


def cq8_workspace_views(ws, B, F, T, num_layers, num_directions):
    """The tensors ww_cq8_crnn_fwd left in ``ws`` (uint8), by stage name: xq (B,F,T), front.stem and front.pw0 .. front.pw3
    (B,H',W',64), seq (B,W',64), per layer l{k}.u int16 (B,W',nd*384), l{k}.y int8 (B,W',nd*128) and l{k}.h int16 (B,nd*128),
    directions stacked, then hcat (B,nd*128) -- the layout include/wwhip.h states."""
    i8, nd = ws.view(torch.int8), num_directions
    H, W = (F + 1) // 2, (T + 1) // 2
    out, off, act = {"xq": i8[:B * F * T].view(B, F, T)}, _r256(B * F * T), B * H * W * 64
    for name in ["stem"] + [f"pw{j}" for j in range(4)]:
        out["front." + name] = i8[off:off + act].view(B, H, W, 64)
        off += _r256(act)
    out["seq"] = i8[off:off + B * W * 64].view(B, W, 64)
    off = _q8_rnn_views(out, i8, off + _r256(B * W * 64), B, W, num_layers, nd, 384, "h")
    out["hcat"] = i8[off:off + B * nd * 128].view(B, nd * 128)
    return out


# ---- int8 inference of an exported MobileNetV3Wakeword bundle (ww_q8_mobilenet.hip).  Activations are int8 NHWC (B,H,W,Cp), Cp the
# channel count rounded up to 64; conv arguments are (w, bias_eff, mult, shift[, tab]) as include/wwhip.h lays them out.
def _mq8_conv_check(what, w, bias, mult, shift, tab, epilogue):
    n = w.shape[0 if what == "conv1x1" else -1]
    if w.dtype != torch.int8 or any(t.dtype != torch.int32 or t.numel() != n for t in (bias, mult, shift)):
        raise ValueError(f"mq8_{what}_fwd: w int8, bias / mult / shift int32, one per output channel")
    if (tab is not None) != (epilogue == MQ8_HSWISH) or (tab is not None and (tab.dtype != torch.int8 or tab.numel() != 256)):
        raise ValueError(f"mq8_{what}_fwd: the Hardswish epilogue, and only it, takes an int8 table of 256 entries")


def mq8_conv1x1_fwd(a, w, bias, mult, shift, zero=-128, epilogue=MQ8_RELU, zero_u=0, tab=None, residual=None, res_mult=0, res_shift=0,
                    gate=None, gate_mult=0, gate_shift=0):
    """a int8 (..., Cin) -> (..., Cout); w int8 (Cout, Cin), both multiples of 64.  ``residual`` (..., Cout) with its multiplier and
    shift goes with MQ8_SIGNED: the projection conv carrying the block's skip connection.  ``gate`` uint8 (B, Cin) with a (B,H,W,Cin)
    selects the fused gate form: the conv reads clamp(zero + R((a - zero) gate, gate_mult, gate_shift)) in place of a."""
    dev = _dev(a, w, bias, mult, shift, tab, residual, gate)
    if gate is not None and (a.dim() != 4 or gate.dtype != torch.uint8 or tuple(gate.shape) != (a.shape[0], a.shape[3])):
        raise ValueError("mq8_conv1x1_fwd: the fused gate form takes a (B,H,W,Cin) and gate uint8 (B,Cin)")
    if a.dtype != torch.int8 or a.shape[-1] % 64 or w.dim() != 2 or w.shape[1] != a.shape[-1] or w.shape[0] % 64:
        raise ValueError("mq8_conv1x1_fwd: int8 activations (..., Cin), w int8 (Cout, Cin), channel counts multiples of 64")
    _mq8_conv_check("conv1x1", w, bias, mult, shift, tab, epilogue)
    out = torch.empty((*a.shape[:-1], w.shape[0]), dtype=torch.int8, device=dev)
    if residual is not None and (residual.dtype != torch.int8 or residual.shape != out.shape):
        raise ValueError("mq8_conv1x1_fwd: residual int8 of the output's shape")
    with _guard(dev):
        _check(load().ww_mq8_conv1x1_fwd(ctx(dev), _p(a), _p(w), _p(bias), _p(mult), _p(shift), a.numel() // a.shape[-1], a.shape[-1],
                                         w.shape[0], int(zero), int(epilogue), int(zero_u), _p(tab), _p(residual), int(res_mult),
                                         int(res_shift), _p(gate), a.shape[1] * a.shape[2] if gate is not None else 0, int(gate_mult),
                                         int(gate_shift), _p(out), _stream(dev)), "ww_mq8_conv1x1_fwd")
    return out


def mq8_dwconv_fwd(a, w, bias, mult, shift, k, stride, zero=-128, epilogue=MQ8_RELU, zero_u=0, tab=None):
    """a int8 (B,H,W,Cp); w int8 (k*k, Cp) [tap][channel]."""
    dev = _dev(a, w, bias, mult, shift, tab)
    if a.dtype != torch.int8 or a.dim() != 4 or a.shape[3] % 16 or tuple(w.shape) != (k * k, a.shape[3]):
        raise ValueError("mq8_dwconv_fwd: int8 activations (B,H,W,Cp), Cp a multiple of 16, w int8 (k*k, Cp)")
    _mq8_conv_check("dwconv", w, bias, mult, shift, tab, epilogue)
    B, H, W, Cp = a.shape
    Ho, Wo = (rq8_half(H), rq8_half(W)) if stride == 2 else (H, W)
    out = torch.empty((B, Ho, Wo, Cp), dtype=torch.int8, device=dev)
    with _guard(dev):
        _check(load().ww_mq8_dwconv_fwd(ctx(dev), _p(a), _p(w), _p(bias), _p(mult), _p(shift), B, H, W, Cp, int(k), int(stride), int(zero),
                                        int(epilogue), int(zero_u), _p(tab), _p(out), _stream(dev)), "ww_mq8_dwconv_fwd")
    return out


def mq8_stem_fwd(xq, w, bias, mult, shift, zero, zero_u, tab):
    """xq int8 (B,F,T); w int8 (9, Cp) [tap][channel] -> (B,(F-1)//2+1,(T-1)//2+1,Cp), the Hardswish epilogue."""
    dev = _dev(xq, w, bias, mult, shift, tab)
    if xq.dtype != torch.int8 or xq.dim() != 3 or w.dim() != 2 or w.shape[0] != 9 or w.shape[1] % 16:
        raise ValueError("mq8_stem_fwd: int8 (B,F,T) features, w int8 (9, Cp), Cp a multiple of 16")
    _mq8_conv_check("stem", w, bias, mult, shift, tab, MQ8_HSWISH)
    B, F, T = xq.shape
    out = torch.empty((B, rq8_half(F), rq8_half(T), w.shape[1]), dtype=torch.int8, device=dev)
    with _guard(dev):
        _check(load().ww_mq8_stem_fwd(ctx(dev), _p(xq), _p(w), _p(bias), _p(mult), _p(shift), B, F, T, w.shape[1], int(zero), int(zero_u),
                                      _p(tab), _p(out), _stream(dev)), "ww_mq8_stem_fwd")
    return out


def mq8_se_fwd(a, C_real, zero, pool_mult, pool_shift, fc1, fc2):
    """a int8 (B,H,W,Cp) with ``C_real`` channels; ``fc1`` = (w (Csq,C), q_b, mult, shift), ``fc2`` = (w (C,Csq), q_b, mult, shift), the
    law's own biases -> (pool int8 (B,Cp), h int8 (B,Csq), gate uint8 (B,Cp))."""
    dev = _dev(a, *fc1, *fc2)
    if a.dtype != torch.int8 or a.dim() != 4 or a.shape[3] != tq8_pad(C_real):
        raise ValueError("mq8_se_fwd: int8 activations (B,H,W,Cp), Cp = C rounded up to 64")
    Csq = fc1[0].shape[0]
    if tuple(fc1[0].shape) != (Csq, C_real) or tuple(fc2[0].shape) != (C_real, Csq) or fc1[0].dtype != torch.int8 or \
            fc2[0].dtype != torch.int8 or any(t.dtype != torch.int32 or t.numel() != n for ts, n in ((fc1[1:], Csq), (fc2[1:], C_real)) for t in ts):
        raise ValueError("mq8_se_fwd: fc1 (w int8 (Csq,C), b / m / sh int32 (Csq)), fc2 (w int8 (C,Csq), b / m / sh int32 (C))")
    B, H, W, Cp = a.shape
    pool = torch.empty((B, Cp), dtype=torch.int8, device=dev)
    h = torch.empty((B, Csq), dtype=torch.int8, device=dev)
    gate = torch.empty((B, Cp), dtype=torch.uint8, device=dev)
    with _guard(dev):
        _check(load().ww_mq8_se_fwd(ctx(dev), _p(a), B, H * W, int(C_real), Cp, Csq, int(zero), int(pool_mult), int(pool_shift),
                                    *[_p(t) for t in fc1], *[_p(t) for t in fc2], _p(pool), _p(h), _p(gate), _stream(dev)), "ww_mq8_se_fwd")
    return pool, h, gate


def mq8_gate_fwd(a, gate, zero, gate_mult, gate_shift):
    dev = _dev(a, gate)
    if a.dtype != torch.int8 or a.dim() != 4 or a.shape[3] % 16 or gate.dtype != torch.uint8 or tuple(gate.shape) != (a.shape[0], a.shape[3]):
        raise ValueError("mq8_gate_fwd: int8 activations (B,H,W,Cp), gate uint8 (B,Cp)")
    out = torch.empty_like(a)
    with _guard(dev):
        _check(load().ww_mq8_gate_fwd(ctx(dev), _p(a), _p(gate), a.shape[0], a.shape[1] * a.shape[2], a.shape[3], int(zero), int(gate_mult),
                                      int(gate_shift), _p(out), _stream(dev)), "ww_mq8_gate_fwd")
    return out


def mq8_head_fwd(a, zero, pool_mult, pool_shift, cls0, zero_u, tab, zero_h, fc_w, fc_bias, fc_scale):
    """a int8 (B,H,W,576); ``cls0`` = (w (1024,576), bias_eff, mult, shift) -> (pool int8 (B,576), hidden int8 (B,1024), logits)."""
    dev = _dev(a, *cls0, tab, fc_w, fc_bias, fc_scale)
    nc = fc_w.shape[0]
    if a.dtype != torch.int8 or a.dim() != 4 or a.shape[3] != MQ8_LAST or tuple(cls0[0].shape) != (MQ8_HIDDEN, MQ8_LAST):
        raise ValueError("mq8_head_fwd: int8 activations (B,H,W,576), classifier.0 weights int8 (1024,576)")
    _mq8_conv_check("conv1x1", *cls0, tab, MQ8_HSWISH)
    if (fc_w.dtype, fc_bias.dtype, fc_scale.dtype) != (torch.int8, torch.int32, torch.float32) or \
            tuple(fc_w.shape) != (nc, MQ8_HIDDEN) or fc_bias.numel() != nc or fc_scale.numel() != nc:
        raise ValueError("mq8_head_fwd: fc_w int8 (num_classes,1024), fc_bias int32 (num_classes), fc_scale float32 (num_classes)")
    B = a.shape[0]
    pool = torch.empty((B, MQ8_LAST), dtype=torch.int8, device=dev)
    hidden = torch.empty((B, MQ8_HIDDEN), dtype=torch.int8, device=dev)
    logits = torch.empty((B, nc), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(load().ww_mq8_head_fwd(ctx(dev), _p(a), B, a.shape[1] * a.shape[2], int(zero), int(pool_mult), int(pool_shift),
                                      *[_p(t) for t in cls0], int(zero_u), _p(tab), int(zero_h), _p(fc_w), _p(fc_bias), _p(fc_scale), nc,
                                      _p(pool), _p(hidden), _p(logits), _stream(dev)), "ww_mq8_head_fwd")
    return pool, hidden, logits


def mq8_mobilenetv3_workspace_bytes(B, F, T):
    return load().ww_mq8_mobilenetv3_workspace_bytes(B, F, T)


def mq8_mobilenetv3_fwd(tab, io: Mq8Io, x, ws, logits):
    """``tab``: ``ptr_array`` of the MQ8_NPTR bundle tensors (None where a block has none); x float32 (B,F,T) or (B,1,F,T); ws uint8;
    logits float32 (B,num_classes)."""
    dev = _dev(x, ws, logits)
    with _guard(dev):
        _check(load().ww_mq8_mobilenetv3_fwd(ctx(dev), tab, C.byref(io), _p(x), x.shape[0], x.shape[-2], x.shape[-1], _p(ws),
                                             ws.numel() * ws.element_size(), _p(logits), _stream(dev)), "ww_mq8_mobilenetv3_fwd")


def mq8_workspace_views(ws, B, F, T):
    """The tensors ww_mq8_mobilenetv3_fwd left in ``ws`` (uint8), by stage name, PADDED to 64 channels: xq (B,F,T), stem, per block
    b{i}.expand (where the block has one), b{i}.dw, the squeeze-excitation's b{i}.pool (B,Cp), b{i}.h (B,Csq), b{i}.gate uint8 (B,Cp)
    and b{i}.y, b{i}.out; last, pool (B,576), hidden (B,1024) -- the layout include/wwhip.h states."""
    from .export.reference import mbv3_blocks
    r256 = lambda n: (n + 255) // 256 * 256       # noqa: E731
    i8 = ws.view(torch.int8)
    out, off = {}, 0

    def take(name, *shape):
        nonlocal off
        n = 1
        for v in shape:
            n *= v
        out[name] = i8[off:off + n].view(*shape)
        off += r256(n)
    take("xq", B, F, T)
    take("stem", B, rq8_half(F), rq8_half(T), 64)
    blocks = mbv3_blocks(F, T)
    for i, b in enumerate(blocks):
        ep = tq8_pad(b["exp"])
        if b["expand"]:
            take(f"b{i}.expand", B, *b["hw_in"], ep)
        take(f"b{i}.dw", B, *b["hw"], ep)
        if b["se"]:
            take(f"b{i}.pool", B, ep)
            take(f"b{i}.h", B, b["se"])
            take(f"b{i}.gate", B, ep)
            out[f"b{i}.gate"] = out[f"b{i}.gate"].view(torch.uint8)
            take(f"b{i}.y", B, *b["hw"], ep)
        take(f"b{i}.out", B, *b["hw"], tq8_pad(b["cout"]))
    take("last", B, *blocks[-1]["hw"], MQ8_LAST)
    take("pool", B, MQ8_LAST)
    take("hidden", B, MQ8_HIDDEN)
    return out


def prof_classes():
    lib = load()
    return [lib.ww_prof_class_name(i).decode() for i in range(lib.ww_prof_num_classes())]


def prof_enable(dev, names=None):
    """Time the given kernel classes (None = all, [] = off) with HIP events on the launch stream."""
    classes = prof_classes()
    mask = 0
    for i, n in enumerate(classes):
        if names is None or n in names:
            mask |= 1 << i
    _check(load().ww_prof_enable(ctx(dev), mask), "ww_prof_enable")


def prof_collect(dev):
    """-> {class: (total_ms, launches)} since the last collect (waits for the recorded events)."""
    classes = prof_classes()
    ms = (C.c_float * len(classes))()
    cnt = (C.c_int32 * len(classes))()
    _check(load().ww_prof_collect(ctx(dev), ms, cnt), "ww_prof_collect")
    return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(classes) if cnt[i]}


def decode_stats(stats_cpu: torch.Tensor) -> dict:
    s = StepStats.from_buffer_copy(bytes(stats_cpu.numpy().tobytes()))
    return {k: getattr(s, k) for k, _ in StepStats._fields_}
