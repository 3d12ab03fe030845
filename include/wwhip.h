/*
 * wwhip.h -- C-ABI of libwwhip.so: the MI355X (gfx950) hot path of the wakeword
 * training inner loop.
 *
 * The reference (sarpel/wakeword_trainer_home) is pure Python and has no FFI layer
 * (SURVEY.md F2); this ABI is what a maintainer binds with ctypes underneath the
 * reference's own Python interfaces (INTEGRATION.md shows the stub).  Every entry
 * point cites the reference interface whose device work it replaces.
 *
 * Conventions
 *   - extern "C"; every function returns int: 0 = ok, <0 = WW_E_* ; the message for
 *     the calling thread's last failure is ww_last_error().
 *   - All tensor arguments are DEVICE pointers owned by the caller (PyTorch-allocated);
 *     the library never frees or retains them.  Scratch is caller-provided.
 *   - Every launch goes to the hipStream_t passed as `stream` (void*; NULL = default
 *     stream).  No entry point synchronises the device or allocates device memory,
 *     except ww_ctx_create (uploads constant tables once).
 *   - Activations inside the conv stack are channels-last  [B][H][W][64] -- the memory format the
 *     reference trains in (src/training/trainer.py:71,165) -- stored as fp32 (WW_ACT_F32, the parity
 *     mode) or bf16 (WW_ACT_BF16; the counterpart of the reference's optimizer.mixed_precision switch,
 *     src/training/trainer.py:92,172).  Arithmetic, statistics and parameters are always fp32.
 *   - A ww_ctx is used by one host thread at a time (the training thread).
 */
#ifndef WWHIP_H
#define WWHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 17: ww_pass_plan / ww_loader_plan (host-only pass plans of the capped-grid support launches) were added; no existing
 * signature, struct, constant or result changed.  ww_dw_plan / ww_ctx_set_dw_wide_addr came later under the same number: pure
 * additions again, as is ww_gemm_plan, and as are the detection scan's entry points (ww_wave_windows_at, ww_feat_windows,
 * ww_detect_accumulate). */
#define WW_ABI_VERSION 17

#define WW_OK 0
#define WW_E_INVALID (-1)     /* bad argument (shape, null pointer, unsupported size) */
#define WW_E_HIP (-2)         /* a HIP runtime call failed */
#define WW_E_WORKSPACE (-3)   /* caller workspace too small */
#define WW_E_UNSUPPORTED (-4) /* valid request outside what the kernels implement */

typedef struct ww_ctx ww_ctx;
typedef void *ww_stream_t; /* hipStream_t */

int ww_abi_version(void);
const char *ww_last_error(void);
int ww_ctx_create(int device, ww_ctx **out);
int ww_ctx_destroy(ww_ctx *ctx);

/* ------------------------------------------------------------------ device-resident step control (HIP graph replay)
 * A captured HIP graph bakes every by-value launch argument, but three things change from one training step to the next:
 * the Philox step of SpecAugment / audio augmentation / dropout, the optimizer's learning rate (schedulers,
 * src/training/optimizer_factory.py:281-333) and its step_state slot.  While a control block is BOUND to the ctx, every
 * entry point reads them from this 32-byte device struct at kernel RUN time:
 *   Philox step  = the call's `step` argument (now an OFFSET: 0 = the batch being trained, 1 = the batch whose input stage
 *                  runs one step ahead) + ctl->step;
 *   ww_clip_optim_step: lr = ctl->lr (cfg->lr ignored), parity = ctl->parity (argument ignored), and the step record goes
 *                  to stats_host_alt instead of stats_host when that parity is 1 (two pinned buffers, so the host may
 *                  read step k's record while step k+1 is running).
 * ww_step_ctl_advance is the one-thread kernel that opens a step: step += 1, parity ^= 1 (the first node of the captured
 * graph).  The host owns the struct's memory and writes lr / the initial step through ordinary copies between replays.
 * The reference has no graph capture; BASELINE config 5 asks for a "hipGraph-captured step".       */
typedef struct {
    uint64_t step;      /* launched-step counter */
    float lr;
    int32_t parity;     /* 0 | 1 */
    float loss_scale;   /* fp16 storage mode: the dynamic loss scale (ww_ce2_loss_fwd_bwd multiplies dlogits by it) */
    int32_t growth_tracker;
    int32_t reserved[2];
} ww_step_ctl;
int ww_ctx_bind_step_ctl(ww_ctx *ctx, const ww_step_ctl *ctl_dev /* device memory, 8-byte aligned; NULL unbinds */);
int ww_step_ctl_advance(ww_ctx *ctx, ww_stream_t stream);

/* ------------------------------------------------------------------ features
 * Replaces FeatureExtractor.__call__ (src/data/feature_extraction.py -- ABSENT from the
 * reference snapshot; contract from src/evaluation/evaluator.py:86-94,122-128 and the
 * shape law of src/export/onnx_exporter.py:316-320: (1, n_feat, N//hop + 1)), batched.
 * Spec: DESIGN.md "Feature spec" (periodic Hann, center/reflect, |rFFT|^2, HTK mel,
 * log(mel+eps); MFCC = orthonormal DCT-II).  n_mfcc == 0 selects log-mel.            */
typedef struct {
    int32_t sample_rate; /* src/config/defaults.py:15  (16000) */
    int32_t n_fft;       /* :18 (1024: the size the fused kernel is built for; any other power of two in [64, 4096]
                            takes a general radix-2 kernel -- validator.py:129 accepts 256 ... 4096) */
    int32_t hop;         /* :19 (160) */
    int32_t n_mels;      /* :20 (128; BASELINE config 2 uses 40); <= 128 */
    int32_t n_mfcc;      /* :17 ; 0 = log-mel output, else <= n_mels */
    float f_min;
    float f_max;   /* <= 0 -> sample_rate/2 */
    float log_eps; /* 1e-6 */
} ww_feat_cfg;

/* Replaces SpecAugment.__call__ (src/data/augmentation.py -- ABSENT; ctor pinned by
 * tests/test_training_pipeline.py:252-257, probabilities by src/config/defaults.py:90-91).
 * Integer index law: DESIGN.md "SpecAugment spec" / oracle/specaugment.py.            */
typedef struct {
    int32_t freq_mask_param;
    int32_t time_mask_param;
    int32_t n_freq_masks; /* n_freq_masks + n_time_masks <= 16 */
    int32_t n_time_masks;
    float freq_mask_prob;
    float time_mask_prob;
} ww_specaug_cfg;

#define WW_WAVE_F32 0
#define WW_WAVE_I16 1

int ww_feat_num_frames(int n_samples, int hop);

/* Host only (no GPU, no context): the HTK mel filterbank ww_logmel_fwd uses for cfg, as the kernels read it.  Replaces what
 * the reference gets from torchaudio's MelSpectrogram inside FeatureExtractor (src/data/feature_extraction.py is absent from
 * the snapshot; called from src/training/trainer.py:165-170 through the data pipeline).
 *   start, len (n_mels ints each): first spectrum bin / number of bins of each triangular band
 *   w (w_cap floats, nullable): the bands' weights back to back, *n_w of them
 *   melq_tab (WW_MELQ_TAB ints, nullable), melq_w (melq_cap floats, nullable), *n_melq_w (nullable): for n_fft 1024, the
 *   same weights in the form the v_mfma_f32_4x4x1 band sums of the STFT kernel read: [0] passes P, [1] 4-band quads NQ,
 *   [2+2p] steps of pass p, [3+2p] offset of its weights, [10+32p+2b] first bin of block b, [11+32p+2b] its unit number,
 *   [138+q] first unit of quad q; weight of (pass p, step t, lane) at melq_w[offset_p + 64 t + lane] = 1/4 of the weight of
 *   band 4*quad + lane%4 at bin first_bin(block lane/4) + t.                                                              */
#define WW_MELQ_TAB 172
int ww_feat_mel_tables(const ww_feat_cfg *cfg, int32_t *start, int32_t *len, float *w, int w_cap, int32_t *n_w,
                       int32_t *melq_tab, float *melq_w, int melq_cap, int32_t *n_melq_w);

/* wave (B,N) f32|i16  ->  out (B,1,n_feat,T) f32, optionally SpecAugment-masked in the
 * same pass.  mask_idx (nullable): int32 (B, n_f+n_t, 2) rows (start,width).           */
int ww_logmel_fwd(ww_ctx *ctx, const void *wave, int wave_dtype, int B, int N, const ww_feat_cfg *cfg,
                  float *out, const ww_specaug_cfg *sa, uint64_t seed, uint64_t step,
                  uint64_t sample_offset, int32_t *mask_idx, ww_stream_t stream);

/* How many persistent workgroups the log-mel kernel is launched with from now on: 0 (default) = one full residency round
 * of the device -- the front end running alone (feature extraction, validation); n > 0 = at most n -- a front end that
 * runs on a side stream BESIDE a training step, where its resident workgroups take registers / LDS from the conv kernels
 * (Trainer: one per CU).  A launch parameter only: results are identical for every n.            */
int ww_ctx_set_logmel_workgroups(ww_ctx *ctx, int n);

/* In-place SpecAugment on ready-made features x (B,1,F,T).                             */
int ww_specaug_apply(ww_ctx *ctx, float *x, int B, int F, int T, const ww_specaug_cfg *sa,
                     uint64_t seed, uint64_t step, uint64_t sample_offset, int32_t *mask_idx,
                     ww_stream_t stream);

/* ------------------------------------------------------------------ waveform augmentation
 * Replaces the RIR / background-noise part of AudioAugmentation.__call__ (src/data/augmentation.py -- ABSENT; ctor
 * tests/test_training_pipeline.py:230-236, knobs src/config/defaults.py:81-87).  Law: DESIGN.md "Audio augmentation
 * spec" / oracle/audio_augment.py.  rirs (R,L) f32, L <= 8192; noises (K,Nn) f32, Nn >= N; either bank may be absent
 * (NULL, 0).  choice_out (nullable): int32 (B,4) = rir index|-1, noise index|-1, noise offset, float bits of snr_db.
 * wave_out must not alias wave_in.                                                                                   */
typedef struct {
    float rir_prob;    /* defaults.py:87 */
    float noise_prob;  /* background_noise_prob, defaults.py:82 */
    float snr_min_db;  /* noise_snr_min, :83 */
    float snr_max_db;  /* noise_snr_max, :84 */
} ww_audio_aug_cfg;
size_t ww_audio_augment_scratch_bytes(int B, int N);
/* Optional, once per RIR bank: spectra for the FFT (overlap-save, 16384-point) form of the convolution, which
 * ww_audio_augment uses when `rir_spectra` is non-NULL; NULL selects the direct time-domain form (short RIRs). */
size_t ww_audio_rir_spectra_bytes(int R);
int ww_audio_rir_spectra(ww_ctx *ctx, const float *rirs, int R, int L, void *spectra, size_t spectra_bytes,
                         ww_stream_t stream);
int ww_audio_augment(ww_ctx *ctx, const float *wave_in, float *wave_out, int B, int N, const float *rirs, int R, int L,
                     const void *rir_spectra, const float *noises, int K, int Nn, const ww_audio_aug_cfg *cfg, uint64_t seed, uint64_t step,
                     uint64_t sample_offset, int32_t *choice_out, void *scratch, size_t scratch_bytes,
                     ww_stream_t stream);

/* Time-stretch and pitch-shift of the clean clip (they precede the RIR and the noise): time-domain WSOLA, then a
 * windowed-sinc resampler; the length N is kept.  Law: DESIGN.md "Time-stretch / pitch-shift spec" (the build's own; draw 2
 * of the audio Philox stream, draws 0 and 1 are ww_audio_augment's).  0.5 <= rate_min <= rate_max <= 2.0 and
 * -12 <= semis_min <= semis_max <= 12, else WW_E_INVALID.  A clip with neither effect is a bit-exact copy.
 * choice_out (nullable): int32 (B,3) = stretched?, float bits of the rate, semitones.  delta_out (nullable): int16
 * (B, ww_audio_tsm_max_grains(N, semis_max)); entry m-1 of a selected clip holds the search offset d_m of grain m, the
 * entries past the clip's last grain and the rows of copied clips are left as they were.  scratch holds the WSOLA output of
 * every clip (ww_audio_tsm_scratch_bytes).  wave_out must not alias wave_in.                                          */
typedef struct {
    float stretch_prob;  /* time_stretch_prob */
    float rate_min;      /* time_stretch_min */
    float rate_max;      /* time_stretch_max */
    float pitch_prob;    /* pitch_shift_prob */
    int32_t semis_min;   /* pitch_shift_min */
    int32_t semis_max;   /* pitch_shift_max */
} ww_audio_tsm_cfg;
int ww_audio_tsm_max_grains(int N, int semis_max);
size_t ww_audio_tsm_scratch_bytes(int B, int N, int semis_max);
int ww_audio_tsm(ww_ctx *ctx, const float *wave_in, float *wave_out, int B, int N, const ww_audio_tsm_cfg *cfg, uint64_t seed,
                 uint64_t step, uint64_t sample_offset, int32_t *choice_out, int16_t *delta_out, void *scratch,
                 size_t scratch_bytes, ww_stream_t stream);

/* ------------------------------------------------------------------ conv stack layers
 * Replace nn.Conv2d / nn.BatchNorm2d(train) / nn.ReLU as the reference composes them
 * (stem form: src/models/architectures.py:99-102; depthwise-separable blocks are the
 * torchvision MobileNetV3 building block the reference imports at :91-95).
 *
 * A "layer" here = conv producing the PRE-BatchNorm tensor y, plus the per-channel batch
 * statistics of y.  BatchNorm+ReLU of a layer is applied by its CONSUMER while loading
 * (scale/shift vector `ss` = [scale(64) | shift(64)]), so normalised activations never
 * touch HBM.  `mr` = [mean(64) | rstd(64)] is kept for backward.                        */
typedef struct {
    const float *gamma;  /* (64) BatchNorm2d.weight */
    const float *beta;   /* (64) BatchNorm2d.bias */
    float *running_mean; /* (64) updated when training != 0 */
    float *running_var;  /* (64) */
    float momentum;      /* 0.1 */
    float eps;           /* 1e-5 */
    int32_t training;    /* 1: batch statistics (+running update); 0: running statistics */
} ww_bn_t;

#define WW_C 64              /* channel width of the conv stack */
#define WW_ACT_F32 0         /* storage type of the activation tensors y_l / g_l (void* arguments) */
#define WW_ACT_BF16 1
#define WW_ACT_F16 2         /* fp16 storage / matrix operands: the reference's own AMP type (fp16 autocast + GradScaler,
                                src/training/trainer.py:172,182-193); gradients carry the loss scale (ww_loss_scale) */
#define WW_MAX_PARTIALS 1024 /* rows of a reduction slab */
/* scratch for one layer call: partial-sum slabs */
size_t ww_layer_scratch_bytes(void);

/* x (B,Hin,Win) f32 (C=1)  ->  y (B,Ho,Wo,64), Ho=(Hin+1)/2, Wo=(Win+1)/2 ; 3x3 s2 p1 */
int ww_conv_stem_fwd(ww_ctx *ctx, int act_dtype, const float *x, const float *w, int B, int Hin, int Win, void *y,
                     const ww_bn_t *bn, float *ss_out, float *mr_out, void *scratch, ww_stream_t stream);
/* depthwise 3x3 p1 on relu(bn(y_in)) */
int ww_dwconv3x3_fwd(ww_ctx *ctx, int act_dtype, const void *y_in, const float *ss_in, const float *w, int B, int H,
                     int W, void *y, const ww_bn_t *bn, float *ss_out, float *mr_out, void *scratch,
                     ww_stream_t stream);
/* pointwise 1x1 (64->64) on relu(bn(y_in)); f32 MFMA */
int ww_pwconv1x1_fwd(ww_ctx *ctx, int act_dtype, const void *y_in, const float *ss_in, const float *w, int B, int H,
                     int W, void *y, const ww_bn_t *bn, float *ss_out, float *mr_out, void *scratch,
                     ww_stream_t stream);
/* AdaptiveAvgPool2d(1) of relu(bn(y)):  pool (B,3,64) = [sum relu(z) | sum_{z>0} yhat | count_{z>0}] */
int ww_gap_fwd(ww_ctx *ctx, int act_dtype, const void *y, const float *ss, const float *mr, int B, int H, int W,
               float *pool, ww_stream_t stream);
/* dropout(Philox) + nn.Linear(64,2) (classifier of cnn_small; reference head form
 * src/models/architectures.py:105-111).  pd (B,64) = dropped pooled vector (kept for bwd) */
int ww_head_fwd(ww_ctx *ctx, const float *pool, int B, int HW, const float *fc_w, const float *fc_b,
                float dropout_p, int training, uint64_t seed, uint64_t step, uint64_t sample_offset, float *pd,
                float *logits, ww_stream_t stream);

/* ---- backward.  `coef` (192) = per-channel [A | Bc | Cc] with  dy = A*dz + Bc*y + Cc
 * (BatchNorm backward folded into one fma chain); produced for the INPUT layer of each
 * call together with that layer's dgamma/dbeta.                                          */
int ww_head_bwd(ww_ctx *ctx, const float *dlogits, const float *pd, const float *pool, int B, int HW,
                const float *fc_w, float dropout_p, int training, uint64_t seed, uint64_t step,
                uint64_t sample_offset, const float *gamma_last, const float *mr_last, float *dfc_w,
                float *dfc_b, float *dpool, float *coef_last, float *dgamma_last, float *dbeta_last,
                ww_stream_t stream);
/* g == NULL -> this is the last conv layer: dz = dpool[b][c] * [z>0] (dpool carries 1/HW).
 * WW_ACT_BF16: y_out is not read -- the kernel recomputes it from y_in with the forward's MFMA chain and rounding
 * (bit-identical to the stored tensor); it must still be passed (fp32 mode reads it).  B*H*W < 2^31.            */
int ww_pwconv1x1_bwd(ww_ctx *ctx, int act_dtype, const void *g, const float *dpool, const void *y_out,
                     const float *ss_out, const float *coef, const void *y_in, const float *ss_in, const float *mr_in,
                     const float *gamma_in, const float *w, int B, int H, int W, void *g_in, float *dw,
                     float *coef_in, float *dgamma_in, float *dbeta_in, void *scratch, ww_stream_t stream);
int ww_dwconv3x3_bwd(ww_ctx *ctx, int act_dtype, const void *g, const void *y_out, const float *coef, const void *y_in,
                     const float *ss_in, const float *mr_in, const float *gamma_in, const float *w, int B,
                     int H, int W, void *g_in, float *dw, float *coef_in, float *dgamma_in,
                     float *dbeta_in, void *scratch, ww_stream_t stream);
int ww_conv_stem_bwd(ww_ctx *ctx, int act_dtype, const void *g, const void *y_out, const float *coef, const float *x,
                     int B, int Hin, int Win, float *dw, void *scratch, ww_stream_t stream);
/* The form the whole-model backward runs: the stem's output is not read but recomputed from x and the stem weights w
 * (64,1,3,3) with the forward kernel's fma chain and rounding, i.e. bit-identical to the tensor ww_conv_stem_fwd stored. */
int ww_conv_stem_bwd_recompute(ww_ctx *ctx, int act_dtype, const void *g, const float *w, const float *coef,
                               const float *x, int B, int Hin, int Win, float *dw, void *scratch, ww_stream_t stream);

/* A test and tuning parameter, not a performance setting.  Every kernel of the conv stack (the layer calls above, the
 * whole-model calls below and the CRNN front end's frequency pooling) is persistent: a workgroup walks item, item + grid,
 * ... and carries prefetched items, LDS double buffers and accumulators from one trip to the next.  n > 0 launches each of
 * them with min(grid, n) workgroups, and hands that many partial rows to the finalize launch, so that a small tensor
 * already takes many trips per workgroup; 0 (default) = no cap, the grids are exactly the uncapped ones.  Results do not
 * depend on n beyond the order of fp32 partial sums.  The cap is read when a launch is issued: a captured graph keeps
 * the grids it was captured with.  The log-mel kernel has its own knob (ww_ctx_set_logmel_workgroups).                  */
int ww_ctx_set_grid_cap(ww_ctx *ctx, int n);

/* A test switch, not a performance setting.  The depthwise kernels address a tensor as a scalar base plus one 32-bit byte
 * offset per lane when its byte size fits 32 bits, and with 64-bit lane addresses otherwise (ww_dw_plan reports which).  on = 1
 * makes ww_dwconv3x3_fwd / _bwd and the whole-model calls take the 64-bit form at any size, so that a small tensor tests it; 0
 * (default) = by size.  Results do not depend on it.  Read when a launch is issued.                                        */
int ww_ctx_set_dw_wide_addr(ww_ctx *ctx, int on);

/* ------------------------------------------------------------------ whole model
 * cnn_small (added to create_model, src/models/architectures.py:437):
 * stem + 4 x (dw,pw) + GAP + dropout + Linear(64,2).  params/grads: arrays of
 * WW_CNN_SMALL_NPTR device pointers in state_dict order:
 *   0 stem.conv.weight  1 stem.bn.weight  2 stem.bn.bias  3 stem.bn.running_mean  4 stem.bn.running_var
 *   5+10i .. : blocks.i.dw.weight, dw_bn.{weight,bias,running_mean,running_var},
 *              blocks.i.pw.weight, pw_bn.{weight,bias,running_mean,running_var}      (i = 0..3)
 *   45 classifier.weight   46 classifier.bias
 * (grads: running_* slots are ignored).                                                  */
#define WW_CNN_SMALL_NPTR 47
size_t ww_cnn_small_workspace_bytes(int B, int F, int T, int act_dtype);
int ww_cnn_small_fwd(ww_ctx *ctx, int act_dtype, void *const *params, const float *x, int B, int F, int T, int training,
                     float bn_momentum, float bn_eps, float dropout_p, uint64_t seed, uint64_t step,
                     uint64_t sample_offset, void *ws, size_t ws_bytes, float *logits, ww_stream_t stream);
/* must follow a training-mode ww_cnn_small_fwd on the same ws/x.  part: WW_BWD_ALL, or the backward in two calls --
 * WW_BWD_LATE (classifier + blocks 3, 2: gradient slots 25..46) then WW_BWD_EARLY (blocks 1, 0 + stem: slots 0..24) -- so a
 * data-parallel caller can start the all-reduce of the late layers' gradients while the early layers' backward runs
 * (the reference is single-GPU, README.md:253-254). */
#define WW_BWD_ALL 0
#define WW_BWD_LATE 1
#define WW_BWD_EARLY 2
int ww_cnn_small_bwd(ww_ctx *ctx, int act_dtype, void *const *params, void *const *grads, const float *x, const float *dlogits,
                     int B, int F, int T, float dropout_p, uint64_t seed, uint64_t step, uint64_t sample_offset,
                     void *ws, size_t ws_bytes, int part, ww_stream_t stream);

/* ------------------------------------------------------------------ loss + step glue
 * Replaces LabelSmoothingCrossEntropy.forward (src/models/losses.py:66-98), the eps==0
 * nn.CrossEntropyLoss branch (:256) and FocalLoss.forward (:170-197) for C == 2, plus their
 * autograd, plus the per-batch accuracy / confusion counters of
 * src/training/trainer.py:196-200 + src/training/metrics.py:105-116.  Two entries: the unweighted mean
 * (what the reference Trainer builds, trainer.py:84) and one with per-class weights and mean / sum / none. */
#define WW_LOSS_CE 0
#define WW_LOSS_FOCAL 1
typedef struct {
    float loss;
    float grad_norm; /* written by ww_grad_norm_clip */
    int32_t correct, tp, tn, fp, fn;
    int32_t nonfinite;  /* != 0 if the loss is not finite (trainer.py:177) */
    int32_t bad_target; /* != 0 if any target is outside [0,2) (losses.py:72) */
    int32_t count;      /* B */
    float found_inf;    /* 1.0 if this step must not update parameters (non-finite loss, bad target, or -- after
                           ww_grad_norm_clip -- non-finite gradient norm), else 0.0.  Layout-compatible with the
                           `found_inf` tensor of PyTorch's fused optimizers, so the reference's "skip the batch"
                           (trainer.py:177-179) needs no host round trip before optimizer.step(). */
    int32_t reserved;
} ww_step_stats;
/* Dynamic loss scaling of the fp16 storage mode (WW_ACT_F16) -- torch.amp.GradScaler's state and update rule
 * (create_grad_scaler, src/training/optimizer_factory.py:403-420; scale -> unscale_ -> step -> update,
 * src/training/trainer.py:182-193) kept and advanced on the DEVICE: ww_ce2_loss_fwd_bwd multiplies dL/dlogits by
 * scale[slot], every gradient down to the flat bucket then carries that factor, ww_clip_optim_step divides it out before the
 * norm / clip / update, and writes scale[slot^1], growth_tracker[slot^1]: non-finite gradients -> scale * backoff_factor and
 * the step is skipped; an applied step -> tracker + 1, and scale * growth_factor once it reaches growth_interval; a batch
 * skipped for its loss or targets leaves both unchanged.  slot alternates like ww_clip_optim_step's parity (it IS that parity).
 * GradScaler's defaults: scale 65536, growth 2, backoff 0.5, interval 2000.                                            */
typedef struct {
    float scale[2];
    int32_t growth_tracker[2];
    float growth_factor, backoff_factor;
    int32_t growth_interval;
    int32_t reserved;
} ww_loss_scale;
/* found_inf_out (nullable): receives stats->found_inf as a float of its own -- a data-parallel caller points it at the
 * spare last element of its flat gradient bucket, so the all-reduce of the gradients also tells every rank that SOME rank
 * must skip this batch (ww_clip_optim_step's found_inf_extra reads it back).  loss_scale (nullable) / loss_scale_slot: see
 * ww_loss_scale; with a bound ww_step_ctl the slot is the block's parity.                                              */
int ww_ce2_loss_fwd_bwd(ww_ctx *ctx, const float *logits, const int64_t *targets, int B, int loss_kind,
                        float label_smoothing, float focal_alpha, float focal_gamma, float *loss_out,
                        float *dlogits, ww_step_stats *stats, float *found_inf_out, const ww_loss_scale *loss_scale,
                        int loss_scale_slot, ww_stream_t stream);
/* The same kernel layout with per-class weights and a choice of reduction: the `weight` tensor the reference's three losses
 * take (src/models/losses.py:89-92, :199-202, :256; create_loss_function passes class_weights through, :245-264) and their
 * reduction argument (:95-102).  l_b, g_b = the per-sample loss and gradient of the entry above before its 1/B,
 * w_b = class_weight[y_b], s = the loss scale:
 *
 *   reduction, mean_divisor        loss                      dlogits[b]
 *   MEAN, WW_DIV_BATCH             sum w_b l_b / B           s w_b g_b / B          (loss * weight).mean(): smoothed CE, focal
 *   MEAN, WW_DIV_WEIGHT_SUM        sum w_b l_b / sum w_b     s w_b g_b / sum w_b    nn.CrossEntropyLoss(weight=...), :256
 *   SUM                            sum w_b l_b               s w_b g_b
 *   NONE                           loss_vec[b] = w_b l_b     s w_b g_b              the caller applies the upstream gradient
 *
 * loss_out and stats->loss hold the reduced value; for NONE the MEAN value under the given mean_divisor (read only for MEAN
 * and NONE).  class_weight: 2 floats in DEVICE memory, [w_neg, w_pos], read at run time (a captured graph sees a later
 * in-place change); NULL = ones.  Sums run in double in one fixed order.  The counters ignore the weights; a target outside
 * [0,2) is clamped and flagged as above and takes the weight of the class it was clamped to.  sum w_b == 0 under
 * WW_DIV_WEIGHT_SUM gives 0/0 = NaN as torch does: nonfinite and found_inf are set and the step is skipped; under
 * WW_DIV_BATCH the same batch gives loss 0 and zero gradients.  With class_weight NULL or (1, 1), MEAN is bit-identical to
 * the entry above under either divisor.  loss_vec: B floats, required for NONE, unused (may be NULL) otherwise. */
#define WW_REDUCE_MEAN 0
#define WW_REDUCE_SUM 1
#define WW_REDUCE_NONE 2
#define WW_DIV_BATCH 0
#define WW_DIV_WEIGHT_SUM 1
int ww_ce2_loss_weighted_fwd_bwd(ww_ctx *ctx, const float *logits, const int64_t *targets, int B, int loss_kind,
                                 float label_smoothing, float focal_alpha, float focal_gamma, const float *class_weight,
                                 int reduction, int mean_divisor, float *loss_out, float *loss_vec, float *dlogits,
                                 ww_step_stats *stats, float *found_inf_out, const ww_loss_scale *loss_scale,
                                 int loss_scale_slot, ww_stream_t stream);
/* The same losses for C = num_classes columns, 2 <= C <= WW_LOSS_MAX_CLASSES (anything else is WW_E_INVALID): what the
 * reference's three losses compute for any width (src/models/losses.py:66-102, :163-212, :256).  logits and dlogits are (B,C),
 * class_weight is C floats in DEVICE memory read at run time (NULL = ones), w_b = class_weight[y_b].  Per sample, with
 * p = softmax(z), lp = log_softmax(z) and onehot of the target y:
 *   CE, smoothing eps   s = onehot (1-eps) + (1-onehot) eps/(C-1);  l = -sum_j s_j lp_j;  g = p - s
 *   focal               pt = clamp(p[y], 1e-7, 1-1e-7), fw = (1-pt)^gamma, a_t = alpha if y == 1 else 1-alpha (class 1 is the
 *                       wakeword for every C), ce = -lp[y];  l = a_t fw ce;
 *                       g_j = a_t (fw (p_j - onehot_j) + dfw ce p[y] (onehot_j - p_j)), dfw = -gamma (1-pt)^(gamma-1) strictly
 *                       inside the clamp and for gamma != 0, else 0
 * and the table of the entry above holds unchanged, s = the loss scale:
 *
 *   reduction, mean_divisor        loss                      dlogits[b][j]
 *   MEAN, WW_DIV_BATCH             sum w_b l_b / B           s w_b g_bj / B
 *   MEAN, WW_DIV_WEIGHT_SUM        sum w_b l_b / sum w_b     s w_b g_bj / sum w_b
 *   SUM                            sum w_b l_b               s w_b g_bj
 *   NONE                           loss_vec[b] = w_b l_b     s w_b g_bj
 *
 * loss_out, stats->loss, loss_vec, found_inf_out, loss_scale / loss_scale_slot and the ww_step_ctl parity are those of the entry
 * above; sums run in double in one fixed order.  A target outside [0,C) is clamped to 0 or C-1, takes that class's weight and
 * sets bad_target and found_inf.  The counters keep the reference's meaning (src/training/metrics.py:105-116): pred = the first
 * index of the row maximum under > (a NaN never wins), correct = #(pred == y), tp = #(pred==1 & y==1), tn = #(pred==0 & y==0),
 * fp = #(pred==1 & y==0), fn = #(pred==0 & y==1), count = B -- so tp+tn+fp+fn < count once classes 2.. occur.
 * confusion (nullable): C x C uint64 in DEVICE memory indexed [target][pred], added to and never reset here; the batch is
 * counted in LDS and added only when this launch leaves found_inf at 0 (finite loss, no bad target) -- the batches the
 * reference's tracker sees (src/training/trainer.py:177-200).  Integer adds only: independent of any order.
 * One block, one thread per sample; rows are walked from global memory, never held in a per-thread array. */
#define WW_LOSS_MAX_CLASSES 64
int ww_cen_loss_fwd_bwd(ww_ctx *ctx, const float *logits, const int64_t *targets, int B, int num_classes, int loss_kind,
                        float label_smoothing, float focal_alpha, float focal_gamma, const float *class_weight,
                        int reduction, int mean_divisor, float *loss_out, float *loss_vec, float *dlogits,
                        ww_step_stats *stats, float *found_inf_out, uint64_t *confusion /* nullable */,
                        const ww_loss_scale *loss_scale, int loss_scale_slot, ww_stream_t stream);
/* Replaces clip_gradients -> torch.nn.utils.clip_grad_norm_
 * (src/training/optimizer_factory.py:446-452) on one flat gradient bucket.  max_norm <= 0:
 * only the norm is computed.  norm_out (nullable) receives the pre-clip L2 norm.          */
int ww_grad_norm_clip(ww_ctx *ctx, float *flat_grads, size_t n, float max_norm, float *norm_out,
                      ww_step_stats *stats /* nullable: grad_norm and found_inf are updated */, ww_stream_t stream);
/* ------------------------------------------------------------------ dense layers on the matrix cores (K8)
 * nn.Linear (+ Hardswish + Dropout) forward/backward: the classifier the reference puts on MobileNetV3,
 *   Sequential(Linear(576,1024), Hardswish(), Dropout(p), Linear(1024,num_classes))   (src/models/architectures.py:105-111).
 * x (M,K), w (N,K) = nn.Linear.weight, bias (N) nullable, y/pre/dy (M,N), dx (M,K), dw (N,K), db (N); all fp32, row-major.
 * mode WW_ACT_F32: fp32 MFMA (v_mfma_f32_32x32x2_f32), parity mode; WW_ACT_BF16: operands rounded to bf16, fp32
 * accumulation (v_mfma_f32_32x32x16_bf16).  epi (nullable): activation, then dropout drawn from the Philox stream
 * ctr = (step, sample_offset + row, TAG_DROPOUT<<24 | col>>2), lane col&3 (dropout_p = 0 in eval).  `pre` receives the
 * pre-activation the backward of the activation needs.                                                              */
#define WW_LIN_NONE 0
#define WW_LIN_HARDSWISH 1
#define WW_LIN_RELU 2          /* squeeze-excitation fc1 */
#define WW_LIN_HARDSIGMOID 3   /* squeeze-excitation fc2 (scale_activation of torchvision's MobileNetV3) */
typedef struct {
    int32_t act;
    float dropout_p;
    uint64_t seed, step, sample_offset;
} ww_linear_epi;
int ww_linear_mfma_fwd(ww_ctx *ctx, int mode, const float *x, const float *w, const float *bias, int M, int K, int N,
                       const ww_linear_epi *epi, float *pre /* nullable */, float *y, ww_stream_t stream);
size_t ww_linear_mfma_bwd_scratch_bytes(int M, int K, int N);
int ww_linear_mfma_bwd(ww_ctx *ctx, int mode, const float *x, const float *w, const float *pre /* nullable if no act */,
                       const float *dy, int M, int K, int N, const ww_linear_epi *epi, float *dx /* nullable */, float *dw,
                       float *db /* nullable */, void *scratch, size_t scratch_bytes, ww_stream_t stream);

/* The GEMM core for callers that keep operands in 16 bits IN HBM: C (M,N) = A (M,K) . B (N,K)^T, A / B bf16 (WW_ACT_BF16) or fp16
 * (WW_ACT_F16) row-major and 16-byte aligned, fp32 accumulation, C fp32 (c_f32 != 0) or the operand type.  K must be a
 * multiple of 64; M and N are free.  128 x 128 tiles, LDS-DMA operand staging.  B is in nn.Linear.weight
 * orientation, so y = x W^T needs no transpose; dx = dy W and dW = dy^T x take transposed copies of their right operand.   */
int ww_gemm16_nt(ww_ctx *ctx, int dtype, const void *A, const void *B, void *C, int c_f32, long M, long N, long K,
                 ww_stream_t stream);

/* ------------------------------------------------------------------ generic channels-last layers
 * Building blocks of bodies with varying channel counts (torchvision's mobilenet_v3_small, as MobileNetV3Wakeword
 * instantiates it: src/models/architectures.py:91-102).  Activations are fp32 row-major (M = B*H*W, C) matrices, so 1x1
 * convolutions and the squeeze-excitation FCs are ww_linear_mfma_* calls; these entry points cover the rest.
 * scratch: ww_nhwc_scratch_bytes(C) bytes.  act: WW_LIN_*.                                                         */
size_t ww_nhwc_scratch_bytes(int C);
/* BatchNorm2d (+activation): y = act(bn(x)); ss (2C) = scale|shift and mr (2C) = mean|rstd are kept for the backward.   */
int ww_bn_act_fwd(ww_ctx *ctx, const float *x, long M, int C, const ww_bn_t *bn, int act, float *y, float *ss, float *mr,
                  void *scratch, ww_stream_t stream);
int ww_bn_act_bwd(ww_ctx *ctx, const float *x, const float *da, long M, int C, const float *ss, const float *mr, int act,
                  int training, float *dx, float *dgamma, float *dbeta, void *scratch, ww_stream_t stream);
/* Conv2dNormActivation in TRAINING mode as the producer + one pass (torchvision's Conv2dNormActivation, the unit MobileNetV3 is
 * built from -- src/models/architectures.py:91-102): the convolution's own kernel leaves the BatchNorm statistics partials (the
 * GEMM epilogue's column sums per row tile / the LDS depthwise kernel's per image group), and the BatchNorm(+activation) apply
 * pass finishes them itself: 2 launches instead of conv + statistics + finish + apply (very tall layers keep the finish launch).
 * y = pre-BatchNorm output (kept for the backward), a = act(bn(y)); ss / mr as ww_bn_act_fwd.  scratch: ww_nhwc_scratch_bytes(C_out).
 * ww_conv1x1_bn_act_fwd: x (M,K) rows = pixels (or 3x3 patches of the stem), w (N,K), matrix mode as ww_linear_mfma_fwd.
 * ww_dwconv_bn_act_fwd: shapes the LDS kernel does not take (more than 128 input pixels per image, C % 4 != 0) and eval mode
 * run ww_dwconv_nhwc_fwd + ww_bn_act_fwd inside.                                                                      */
int ww_conv1x1_bn_act_fwd(ww_ctx *ctx, int mode, const float *x, const float *w, int M, int K, int N, const ww_bn_t *bn, int act,
                          const float *residual /* nullable (M,N): a = act(bn(y)) + residual, the block's skip connection */,
                          float *y, float *a, float *ss, float *mr, void *scratch, size_t scratch_bytes, ww_stream_t stream);
int ww_dwconv_bn_act_fwd(ww_ctx *ctx, const float *x, const float *w, int B, int H, int W, int C, int k, int stride,
                         const ww_bn_t *bn, int act, float *y, float *a, float *ss, float *mr, void *scratch, ww_stream_t stream);
/* depthwise Conv2d(C, C, k, stride, padding=k/2, groups=C, bias=False): x (B,H,W,C), w (C,1,k,k), k in {3,5}, stride in {1,2} */
int ww_dwconv_nhwc_fwd(ww_ctx *ctx, const float *x, const float *w, int B, int H, int W, int C, int k, int stride, float *y,
                       ww_stream_t stream);
int ww_dwconv_nhwc_bwd(ww_ctx *ctx, const float *x, const float *w, const float *dy, int B, int H, int W, int C, int k,
                       int stride, float *dx /* nullable */, float *dw, void *scratch, ww_stream_t stream);
/* AdaptiveAvgPool2d(1) on (B,HW,C) -> (B,C); per-(b,c) scaling y = x*gate and its two gradients; dx = dy*gate + dpool/HW   */
int ww_pool_hw_fwd(ww_ctx *ctx, const float *x, int B, int HW, int C, float *s, ww_stream_t stream);
int ww_scale_bc_fwd(ww_ctx *ctx, const float *x, const float *gate, int B, int HW, int C, float *y, ww_stream_t stream);
int ww_scale_bc_bwd_gate(ww_ctx *ctx, const float *x, const float *dy, int B, int HW, int C, float *dgate, ww_stream_t stream);
int ww_scale_pool_bwd(ww_ctx *ctx, const float *dy /* nullable */, const float *gate, const float *dpool /* nullable */, int B,
                      int HW, int C, float *dx, ww_stream_t stream);
/* Squeeze-excitation as torchvision's mobilenet_v3_small builds it (the model src/models/architectures.py:91-102 instantiates):
 * y = x * hardsigmoid(W2 relu(W1 mean_hw(x) + b1) + b2), x / y (B,HW,C), w1 (Cs,C), w2 (C,Cs) in nn.Conv2d(.,.,1) layout.  ONE launch
 * forward (a workgroup owns whole images), TWO backward (dx + per-image pre-activation gradients, then the four parameter
 * gradients as fixed-order sums over the batch); fp32 arithmetic whatever the model's matrix mode.  s (B,C), pre1 (B,Cs),
 * pre2 (B,C) are kept for the backward.  C % 4 == 0, Cs % 4 == 0, C <= 1024, Cs <= 256, else WW_E_UNSUPPORTED (callers then compose the block
 * from ww_pool_hw_fwd / ww_linear_mfma_* / ww_scale_bc_*).                                                              */
size_t ww_se_bwd_scratch_bytes(int B, int C, int Cs);
int ww_se_fwd(ww_ctx *ctx, const float *x, int B, int HW, int C, int Cs, const float *w1, const float *b1, const float *w2,
              const float *b2, float *y, float *s, float *pre1, float *pre2, ww_stream_t stream);
int ww_se_bwd(ww_ctx *ctx, const float *x, const float *dy, const float *s, const float *pre1, const float *pre2, const float *w1,
              const float *w2, int B, int HW, int C, int Cs, float *dx, float *dw1, float *db1, float *dw2, float *db2,
              void *scratch, size_t scratch_bytes, ww_stream_t stream);
/* The one-channel stem of MobileNetV3Wakeword (src/models/architectures.py:94-101 replaces torchvision's first conv by
 * Conv2d(1, 16, 3, stride 2, padding 1, bias=False)) as a direct convolution: x (B,H,W), w (C,1,3,3), C % 4 == 0, C <= 64.
 * Forward in training mode = convolution (which leaves the BatchNorm statistics partials) + the finishing apply pass, as
 * ww_conv1x1_bn_act_fwd; ww_stem3x3s2_bwd_dw is its weight gradient (the input needs none).  scratch: ww_nhwc_scratch_bytes(C). */
int ww_stem3x3s2_bn_act_fwd(ww_ctx *ctx, const float *x, const float *w, int B, int H, int W, int C, const ww_bn_t *bn, int act,
                            float *y, float *a, float *ss, float *mr, void *scratch, ww_stream_t stream);
int ww_stem3x3s2_bwd_dw(ww_ctx *ctx, const float *x, const float *dy, int B, int H, int W, int C, float *dw, void *scratch,
                        ww_stream_t stream);
/* 3x3 stride-2 pad-1 patches of a one-channel image (B,H,W) -> (B*ceil(H/2)*ceil(W/2), 9): the stem conv becomes a GEMM */
int ww_im2col3x3s2(ww_ctx *ctx, const float *x, int B, int H, int W, float *cols, ww_stream_t stream);
int ww_add_f32(ww_ctx *ctx, const float *a, const float *b, size_t n, float *y, ww_stream_t stream);
/* Host-only plan queries: the kernel form and grid the entry points above launch for a shape, computed by the code they launch
 * from.  Nothing is allocated or launched and no device is needed.  aligned: every base pointer of the call is 16-byte aligned;
 * 0 reports the call with ALL of them off that grid (a call with only some off it, such as a misaligned residual beside aligned
 * x and y, takes the same launches but may keep V = 4 in those that do not touch the misaligned tensor).
 * ww_nhwc_plan_dw: which = 0 ww_dwconv_nhwc_fwd (in training mode ww_dwconv_bn_act_fwd takes its statistics in the conv kernel
 *   exactly when this is the LDS plan, one partial row per image group), 1 / 2 the dx / dw launch of ww_dwconv_nhwc_bwd;
 *   out[8] = {LDS kernel 1 / gather 0, V, workgroups, images per workgroup, channel groups G_c, channel float4s per group CC4,
 *   image groups (dw gather: pixel chunks), row lanes R (dw gather)}; the LDS-only fields are 0 for a gather plan.
 * ww_nhwc_plan_bn: which = 0 ww_bn_act_fwd, 1 ww_bn_act_bwd, 2 the BatchNorm half of a conv + BatchNorm call whose producer left
 *   `chunks` rows of partials (ww_conv1x1_bn_act_fwd: ceil(M / ww_conv1x1_row_tile), ww_dwconv_bn_act_fwd: image groups,
 *   ww_stem3x3s2_bn_act_fwd: workgroups); out[10] = {chunks, rows per chunk, row lanes of the statistics launch, 1 if the apply
 *   pass finishes the partials itself / 0 for finish launch + elementwise apply, then CG4, G_c, R, rows per workgroup of the
 *   finishing pass (0 if not taken), workgroups and V of the apply launch}.
 * ww_nhwc_plan_stem: out[2] = {workgroups of the persistent grid, pixel lanes per workgroup}.
 * ww_nhwc_plan_ew: an elementwise pass over n floats of a (..., C) tensor (ww_add_f32: C = 4; ww_im2col3x3s2: aligned = 0);
 *   out[2] = {workgroups of 256 threads, V}.                                                                            */
int ww_nhwc_plan_dw(int which, int B, int H, int W, int C, int k, int stride, int aligned, int *out);
int ww_nhwc_plan_bn(int which, long M, int C, int chunks, int training, int aligned, int *out);
int ww_nhwc_plan_stem(int B, int H, int W, int C, int *out);
int ww_nhwc_plan_ew(long n, int C, int aligned, int *out);
int ww_se_plan(int B, int HW, int C, int Cs, int *out);      /* ww_se_fwd / _bwd: out[2] = {images per workgroup, workgroups} */
int ww_conv1x1_row_tile(int mode, int M, int K, int N);      /* rows per statistics partial of ww_conv1x1_bn_act_fwd; 0: bad argument */
/* Host-only pass plans of the support launches whose grid is capped on the host and whose kernel walks its n items in passes of
 * that grid (`for (i = ...; i < n; i += one pass)`), computed by the function the launch site takes its grid from; no context,
 * no device.  ww_pass_plan: out[2] = {workgroups of 256 threads, items one pass holds}; the launch makes ceil(n / out[1]) passes.
 *   WW_PASS_EW           the element-wise launches of the Conv1d / Conv2d families: ww_add_relu_fwd and ww_relu_mask_bwd (n
 *                        floats), the masked gradient of ww_tconv1d_bwd (n = B T Cout / 4 float4s), ww_maxpool3x3s2_fwd / _bwd
 *                        (n = B Ho Wo C / 4 resp. B H W C / 4 channel quads), the weight packing and the sum of dW partials
 *   WW_PASS_DROPOUT_BT   ww_dropout_bt: n = B T ceil(C / 4) channel quads
 *   WW_PASS_WAVE_WINDOWS ww_wave_windows: n = W windows, one workgroup each
 *   WW_PASS_TO16_PAIR    the 16-bit copies of x and W_ih in front of ww_gru_fwd's input projection (16-bit modes, I % 64 == 0):
 *                        n = (B T I + 384 I) / 4 float4s, four per thread and pass
 * ww_loader_plan: ww_loader_batch launches out[0] = S workgroups per row of out[1] = `passes` x 256 chunks of 8 samples; workgroup
 * s of a row takes passes s, s + S, ...: ceil(passes / S) trips, one fewer for the workgroups from passes % S on when S does not
 * divide passes.                                                                                                              */
#define WW_PASS_EW 0
#define WW_PASS_DROPOUT_BT 1
#define WW_PASS_WAVE_WINDOWS 2
#define WW_PASS_TO16_PAIR 3
int ww_pass_plan(int launch, long n, long *out);
int ww_loader_plan(int B, int n_out, int *out);
/* Host-only: the dispatch of ww_dwconv3x3_fwd / _bwd for a (B, H, W, 64) tensor of act_dtype, from the code the launchers run; no
 * context, no device (wide = what ww_ctx_set_dw_wide_addr would hold).  An item is one 4-column strip of one row segment of one
 * image and a wave holds items 2k, 2k + 1 at any grid.  out[7] = {ncs strips per row, nseg row segments per image, hs_len rows per
 * segment, items, waves (item pairs) of the launch, how many of them take the interior body (both strips have all six window
 * columns inside the image; no column clamps, selects or guards), address form: 32 or 64}.                                      */
int ww_dw_plan(int B, int H, int W, int act_dtype, int wide, long *out);
/* Host-only: what ww_linear_mfma_fwd (which = 0) / ww_linear_mfma_bwd (which = 1) launch for (M, K, N) in `mode`, from the
 * functions the launchers themselves decide through; no context, no device (ABI 17, additive).  full_epilogue: forward 1 when a
 * pre-activation copy, an activation or dropout is requested (the EPI 1 kernels), backward 1 when an activation or dropout is
 * (k_linear_dpre runs).  aligned: 1 when every base pointer is on a 16-byte boundary; the leading-dimension half of the float4
 * rule follows from the shape.  need_dx: backward, 0 when dx is NULL.  A block tile cfg is 0 = 64 x 64, 1 = 128 x 64,
 * 2 = 128 x 128; shallow = the 32-deep K stage of the 16-bit modes.  out[24], unused entries 0:
 *   forward:  {0 EPI kind 1 / 2, 1 cfg, 2 shallow, 3 K per LDS stage, 4 vecA (x), 5 vecB (w), 6-8 grid x / y / z}
 *   backward: {0 k_linear_dpre runs, 1 its grid, 2 dX and dW in one k_gemm_pair launch, 3 the rule that refused the pair
 *              (WW_PAIR_*), 4 dX cfg as launched (after the tall remap), 5 dX shallow, 6 dW cfg, 7 dW shallow, 8 contraction rows
 *              per dW split, 9 dW splits nz, 10 workgroups of the dW side nbw, 11 of the dX side nbx (0 without dx), 12
 *              k_splitk_sum is launched (or its sum queued when the context defers), 13 its grid, 14-16 WW_GEMM_PAIR,
 *              WW_GEMM_PAIR_TALL and the effective WW_DW_MIN_ROWS as the library read them, 17 dX cfg before the remap, 18 splits
 *              asked for, 19-22 vec of dX's A (dpre) and B (w), dW's A (dpre) and B (x), 23 workgroups of the bias-gradient sum} */
#define WW_PAIR_OK 0          /* paired */
#define WW_PAIR_OFF 1         /* WW_GEMM_PAIR=0 */
#define WW_PAIR_DX_CFG2 2     /* dX wants 128 x 128 tiles */
#define WW_PAIR_DW_TILE 3     /* dW wants a tile other than 64 x 64 */
#define WW_PAIR_DW_SHALLOW 4  /* dW wants the shallow stage (M <= 32, 16-bit modes) */
#define WW_PAIR_TALL_OFF 5    /* a tall deep dX under WW_GEMM_PAIR_TALL=0 */
#define WW_PAIR_NO_DX 6       /* dx == NULL: dW alone */
int ww_gemm_plan(int which, int mode, int M, int K, int N, int full_epilogue, int aligned, int need_dx, long *out);

/* ------------------------------------------------------------------ conv front-end of the CRNN
 * cnn_small's conv stack (stem + 4 depthwise-separable blocks) without GAP / classifier, followed by the mean over the
 * frequency axis of the last layer's activations: x (B,1,F,T) -> seq (B, ceil(T/2), 64) fp32, the input sequence of the
 * recurrent layers.  Same parameter / gradient pointer tables and workspace as ww_cnn_small_fwd/bwd (entries 45, 46 --
 * the classifier -- are not read and may be NULL).  The reference has no CRNN: the topology is this
 * build's, assembled from the reference's conv idiom and its GRUWakeword.                                          */
int ww_cnn_front_fwd(ww_ctx *ctx, int act_dtype, void *const *params, const float *x, int B, int F, int T, int training,
                     float bn_momentum, float bn_eps, void *ws, size_t ws_bytes, float *seq, ww_stream_t stream);
int ww_cnn_front_bwd(ww_ctx *ctx, int act_dtype, void *const *params, void *const *grads, const float *x, const float *dseq,
                     int B, int F, int T, void *ws, size_t ws_bytes, ww_stream_t stream);

/* ------------------------------------------------------------------ causal dilated Conv1d on the matrix cores (TCNWakeword)
 * The convolution of the reference's TemporalBlock (src/models/architectures.py:323-372: nn.Conv1d(Cin, Cout, k, padding=(k-1)d,
 * dilation=d), of whose output the first T steps are kept -- on those a causal convolution), channels-last:
 *   y[b,t,n] = bias[n] + sum_j sum_c x[b, t - (k-1-j) d, c] w[n,c,j]          (steps before t = 0 read as 0)
 * x (B,T,Cin), y / dy / residual (B,T,Cout), w (Cout,Cin,k) = nn.Conv1d.weight, bias (Cout); all fp32, contiguous, 16-byte
 * aligned.  mode as ww_linear_mfma_*: WW_ACT_F32 = v_mfma_f32_32x32x2_f32 (parity mode), WW_ACT_BF16 / WW_ACT_F16 = operands rounded
 * when staged, fp32 accumulation.  1 <= k <= 8, d >= 1 (also (k-1) d >= T), B, T >= 1, Cin and Cout positive multiples of 4;
 * anything else is WW_E_INVALID before any launch.  scratch: ww_tconv1d_scratch_bytes(B,T,Cin,Cout,k) bytes (WW_E_WORKSPACE).
 * fwd epilogue: + bias, then + residual (nullable), then ReLU (relu != 0) -- "y = relu(conv + residual)" closes a TemporalBlock.
 * bwd: dpre = dy * mask_scale where y != 0 and y2 != 0 (both nullable: the layer's saved outputs carry its ReLU and dropout
 * masks, mask_scale = 1/(1-p) of a dropout that followed); dx (nullable; added to when accumulate_dx != 0), dw (Cout,Cin,k) and
 * db (Cout) in a fixed summation order: dw as row-range partial products summed in order -- queued instead while
 * ww_ctx_set_deferred_reduce is in force (the scratch must then live until the flush).                                     */
size_t ww_tconv1d_scratch_bytes(int B, int T, int Cin, int Cout, int k);
int ww_tconv1d_fwd(ww_ctx *ctx, int mode, const float *x, const float *w, const float *bias, int B, int T, int Cin, int Cout, int k,
                   int dilation, int relu, const float *residual /* nullable */, float *y, void *scratch, size_t scratch_bytes,
                   ww_stream_t stream);
int ww_tconv1d_bwd(ww_ctx *ctx, int mode, const float *x, const float *w, const float *y /* nullable */, const float *y2 /* nullable */,
                   float mask_scale, const float *dy, int B, int T, int Cin, int Cout, int k, int dilation, float *dx /* nullable */,
                   int accumulate_dx, float *dw, float *db, void *scratch, size_t scratch_bytes, ww_stream_t stream);
/* The identity skip of a TemporalBlock whose channel counts agree: y = relu(a + b), and dx = dy where y != 0                */
int ww_add_relu_fwd(ww_ctx *ctx, const float *a, const float *b, size_t n, float *y, ww_stream_t stream);
int ww_relu_mask_bwd(ww_ctx *ctx, const float *dy, const float *y, size_t n, float *dx, ww_stream_t stream);

/* ------------------------------------------------------------------ dense Conv2d on the matrix cores (ResNet18Wakeword)
 * nn.Conv2d(Cin, Cout, k, stride, padding = k/2, bias=False), channels-last, as an implicit GEMM (M = pixels, K = k*k*Cin, N = Cout;
 * no patch matrix in memory):
 *   y[b,ho,wo,n] = sum_{r,s,c} x[b, ho*stride + r - k/2, wo*stride + s - k/2, c] w[n,c,r,s]      (pixels outside the image read as 0)
 * x / dx (B,H,W,Cin), y / dy (B,Ho,Wo,Cout) with Ho = (H + 2(k/2) - k)/stride + 1 (Wo likewise), w / dw (Cout,Cin,k,k) =
 * nn.Conv2d.weight; all fp32, contiguous, 16-byte aligned.  mode as ww_tconv1d_*: WW_ACT_F32 = v_mfma_f32_32x32x2_f32 (parity mode),
 * WW_ACT_BF16 / WW_ACT_F16 = operands rounded when staged, fp32 accumulation.  k odd in 1..7, stride 1 or 2, B, H, W >= 1, Cin and
 * Cout positive multiples of 4; anything else is WW_E_INVALID before any launch.  scratch: ww_conv2d_scratch_bytes(...) bytes
 * (WW_E_WORKSPACE; 0 for a shape the kernels refuse).
 * bwd: dx (nullable; added to when accumulate_dx != 0, else EVERY pixel is written -- also those no output read, as zeros) and dw
 * in a fixed summation order: pixel-range partial products summed in order -- queued instead while ww_ctx_set_deferred_reduce is
 * in force (the scratch must then live until the flush).                                                                      */
size_t ww_conv2d_scratch_bytes(int B, int H, int W, int Cin, int Cout, int k, int stride);
int ww_conv2d_fwd(ww_ctx *ctx, int mode, const float *x, const float *w, int B, int H, int W, int Cin, int Cout, int k, int stride,
                  float *y, void *scratch, size_t scratch_bytes, ww_stream_t stream);
int ww_conv2d_bwd(ww_ctx *ctx, int mode, const float *x, const float *w, const float *dy, int B, int H, int W, int Cin, int Cout, int k,
                  int stride, float *dx /* nullable */, int accumulate_dx, float *dw, void *scratch, size_t scratch_bytes,
                  ww_stream_t stream);
/* The one-channel stem nn.Conv2d(1, C, k, stride, k/2, bias=False) (the reference replaces resnet18's conv1 by Conv2d(1,64,7,2,3)) as
 * a direct fp32 convolution: x (B,H,W) -> y (B,Ho,Wo,C), w (C,1,k,k); k odd in 1..7, stride 1 or 2, C a multiple of 4 in 4..128.
 * The image may be smaller than the kernel.  ww_conv2d_stem_bwd_dw is its weight gradient (the input needs none), summed in a fixed
 * order or queued as above; scratch: ww_conv2d_stem_scratch_bytes(C, k).                                                      */
size_t ww_conv2d_stem_scratch_bytes(int C, int k);
int ww_conv2d_stem_fwd(ww_ctx *ctx, const float *x, const float *w, int B, int H, int W, int C, int k, int stride, float *y,
                       ww_stream_t stream);
int ww_conv2d_stem_bwd_dw(ww_ctx *ctx, const float *x, const float *dy, int B, int H, int W, int C, int k, int stride, float *dw,
                          void *scratch, size_t scratch_bytes, ww_stream_t stream);
/* nn.MaxPool2d(3, 2, 1) on (B,H,W,C) -> (B,(H-1)/2+1,(W-1)/2+1,C), C a positive multiple of 4.  Padding never wins; the gradient goes
 * to the FIRST maximal element of a window in row-major order (torch's rule), recomputed from x: a gather per input pixel over the
 * at most 4 windows that contain it, no atomics.                                                                              */
int ww_maxpool3x3s2_fwd(ww_ctx *ctx, const float *x, int B, int H, int W, int C, float *y, ww_stream_t stream);
int ww_maxpool3x3s2_bwd(ww_ctx *ctx, const float *x, const float *dy, int B, int H, int W, int C, float *dx, ww_stream_t stream);

/* ------------------------------------------------------------------ the same layers with 16-bit ACTIVATION STORAGE (`_st`)
 * Every (B,H,W,C) activation tensor and every activation gradient (the void* arguments) is bf16 (storage = WW_ACT_BF16) or fp16
 * (WW_ACT_F16) in HBM, contiguous and 16-byte aligned; features in, parameters, weight gradients, BatchNorm vectors and the pooled
 * mean stay fp32.  Arithmetic is fp32; a value is rounded (round to nearest even; fp16 overflow -> inf, the loss scaler's signal)
 * exactly where a tensor is stored.  storage = WW_ACT_F32, a channel count that is no multiple of 8 (a 16-byte access is 8
 * elements) or a null pointer is WW_E_INVALID before any launch; shapes, k and stride otherwise as for the fp32 entry points.
 *
 * ww_conv2d_st_fwd / _bwd: ww_conv2d_fwd / _bwd whose matrix mode IS the storage type: the operands go from HBM into the LDS tiles as
 * they are, the weights are rounded once when they are re-laid per tap, products accumulate in fp32 (blocked, as ww_conv2d_*).
 *   y = S(conv(x, S(w)));  dx = S(dX(dy, S(w)) + (accumulate_dx ? float(dx) : 0));  dw (fp32) = dW(dy, x) in the fixed order of
 * ww_conv2d_bwd (partials queued while ww_ctx_set_deferred_reduce is in force).  scratch: ww_conv2d_st_scratch_bytes(...).
 * stat_part (forward, nullable): ceil(M / 64) rows of 2 Cout floats, M = B Ho Wo; the kernel leaves in row t the per-column sums of the
 * STORED values of output rows [64 t, 64 t + 64) and of their squares ([sum (Cout) | sum of squares (Cout)], fp32, fixed order, no
 * atomics) -- BatchNorm's statistics without another pass over y: hand them to ww_bn_act_st_fwd.                                 */
size_t ww_conv2d_st_scratch_bytes(int B, int H, int W, int Cin, int Cout, int k, int stride);
int ww_conv2d_st_fwd(ww_ctx *ctx, int storage, const void *x, const float *w, int B, int H, int W, int Cin, int Cout, int k, int stride,
                     void *y, float *stat_part /* nullable */, void *scratch, size_t scratch_bytes, ww_stream_t stream);
int ww_conv2d_st_bwd(ww_ctx *ctx, int storage, const void *x, const float *w, const void *dy, int B, int H, int W, int Cin, int Cout,
                     int k, int stride, void *dx /* nullable */, int accumulate_dx, float *dw, void *scratch, size_t scratch_bytes,
                     ww_stream_t stream);
/* BatchNorm(+activation) of a 16-bit x (M, C), C a multiple of 8 in 8..1024.  Training: the statistics are those of the STORED x
 * (column sums in fp64 per row chunk, fp32 partials, finished in fp64 in a fixed order); eval: the running statistics.  ss
 * (scale|shift, 2C) and mr (mean|rstd, 2C) are written and the running statistics move exactly as in ww_bn_act_fwd.
 *   y = S(act(fma(x, scale, shift) + idn)),  idn = 0 (res == NULL) | float(res) | fma(float(res), res_ss[0:C], res_ss[C:2C])
 * -- with res / res_ss the tail of a BasicBlock, relu(bn2(c2) + (x | bn_d(cd))), is one pass with one rounding.  y == NULL: only the
 * statistics (ss, mr, running statistics).  scratch: ww_nhwc_scratch_bytes(C).
 * stat_part / stat_rows (nullable / ignored then; ignored in eval mode): a producer's statistics partials of x in the layout above;
 * they are finished in fp64 in row order (more than 1024 rows: folded to 256 first, each the fp64 sum of consecutive rows), and
 * the column-statistics pass over x is not run.
 * bwd: the two passes of ww_bn_act_bwd; x, da in S, dx = S(...), dgamma / dbeta fp32 (C each).                                  */
int ww_bn_act_st_fwd(ww_ctx *ctx, int storage, const void *x, long M, int C, const ww_bn_t *bn, int act, const void *res /* nullable */,
                     const float *res_ss /* nullable */, const float *stat_part /* nullable */, long stat_rows, void *y /* nullable */,
                     float *ss, float *mr, void *scratch, ww_stream_t stream);
int ww_bn_act_st_bwd(ww_ctx *ctx, int storage, const void *x, const void *da, long M, int C, const float *ss, const float *mr, int act,
                     int training, void *dx, float *dgamma, float *dbeta, void *scratch, ww_stream_t stream);
/* The one-channel stem with an S output (x, w fp32: y = S(conv(x, w))) and its weight gradient from an S dy (dw fp32); C a multiple
 * of 8 in 8..128.  MaxPool2d(3, 2, 1) in S: the forward selects and never rounds, the backward rounds the fp32 sum of the (at most
 * four) window gradients of a pixel once.                                                                                      */
int ww_conv2d_stem_st_fwd(ww_ctx *ctx, int storage, const float *x, const float *w, int B, int H, int W, int C, int k, int stride,
                          void *y, ww_stream_t stream);
int ww_conv2d_stem_st_bwd_dw(ww_ctx *ctx, int storage, const float *x, const void *dy, int B, int H, int W, int C, int k, int stride,
                             float *dw, void *scratch, size_t scratch_bytes, ww_stream_t stream);
int ww_maxpool3x3s2_st_fwd(ww_ctx *ctx, int storage, const void *x, int B, int H, int W, int C, void *y, ww_stream_t stream);
int ww_maxpool3x3s2_st_bwd(ww_ctx *ctx, int storage, const void *x, const void *dy, int B, int H, int W, int C, void *dx,
                           ww_stream_t stream);
/* mean (B,C) fp32 = the mean over HW of x (B,HW,C) in S, summed in a fixed order;  dx (B,HW,C) = S(dmean[b][c] / HW).
 * ww_relu_mask_st_bwd: dx = dy where the stored y != 0, else 0 (n elements, a multiple of 8; exact).                              */
int ww_mean_hw_st_fwd(ww_ctx *ctx, int storage, const void *x, int B, int HW, int C, float *mean, ww_stream_t stream);
int ww_mean_hw_st_bwd(ww_ctx *ctx, int storage, const float *dmean, int B, int HW, int C, void *dx, ww_stream_t stream);
int ww_relu_mask_st_bwd(ww_ctx *ctx, int storage, const void *dy, const void *y, size_t n, void *dx, ww_stream_t stream);

/* ------------------------------------------------------------------ the causal Conv1d layer with 16-bit ACTIVATION STORAGE
 * ww_tconv1d_fwd / _bwd with every (B,T,C) activation tensor and its gradient in S = bf16 | fp16 (`storage`: WW_ACT_BF16 |
 * WW_ACT_F16 -- also the matrix mode).  Arithmetic is fp32; a value is rounded (RNE) exactly where a tensor is stored and nowhere
 * else.  w, bias, dw, db stay fp32.  Channel counts are multiples of 8, tensors contiguous and 16-byte aligned, 1 <= k <= 8,
 * dilation >= 1; anything else (a null argument, an unknown storage code) is WW_E_INVALID before any launch, a scratch below
 * ww_tconv1d_st_scratch_bytes(...) bytes WW_E_WORKSPACE.
 *   fwd : y = S([relu](acc + bias [+ float(residual)])), acc the fp32 chain over the stored x and S(w) (rounded once, when packed)
 *   bwd : dpre = S(dy * mask_scale * [y != 0] * [y2 != 0]) -- the masks are read off the STORED outputs (dpre is dy itself without
 *         masks and with mask_scale == 1);  dx = S(acc) or S(acc + float(dx));  dw: fp32 partials over the stored dpre and x, summed
 *         in range order here or by the deferred flush (ww_defer);  db = the fp32 sum, in a fixed order, of the stored dpre.
 * ww_dropout_bt_st: ww_dropout_bt's Philox law on contiguous rows, out = S(keep ? float(x) * (1 / (1 - p)) : 0); out may be x.
 * ww_add_relu_st_fwd: y = S(relu(float(a) + float(b))), n elements (a multiple of 8).
 * ww_seq_round_st: out (B,T,F) = S(x); x fp32 is (B,F,T) (transposed != 0: the Trainer's (B,1,F,T) batches) or (B,T,F).          */
size_t ww_tconv1d_st_scratch_bytes(int storage, int B, int T, int Cin, int Cout, int k);
int ww_tconv1d_st_fwd(ww_ctx *ctx, int storage, const void *x, const float *w, const float *bias, int B, int T, int Cin, int Cout,
                      int k, int dilation, int relu, const void *residual /* nullable */, void *y, void *scratch, size_t scratch_bytes,
                      ww_stream_t stream);
int ww_tconv1d_st_bwd(ww_ctx *ctx, int storage, const void *x, const float *w, const void *y /* nullable */,
                      const void *y2 /* nullable */, float mask_scale, const void *dy, int B, int T, int Cin, int Cout, int k,
                      int dilation, void *dx /* nullable */, int accumulate_dx, float *dw, float *db, void *scratch,
                      size_t scratch_bytes, ww_stream_t stream);
int ww_dropout_bt_st(ww_ctx *ctx, int storage, const void *x, int B, int T, int C, float p, uint64_t seed, uint64_t step,
                     uint64_t sample_offset, int stream_id, void *out, ww_stream_t stream);
int ww_add_relu_st_fwd(ww_ctx *ctx, int storage, const void *a, const void *b, size_t n, void *y, ww_stream_t stream);
int ww_seq_round_st(ww_ctx *ctx, int storage, const float *x, int B, int T, int F, int transposed, void *out, ww_stream_t stream);

/* ------------------------------------------------------------------ GRU layer, one direction
 * torch.nn.GRU's cell and parameter layout (gate order r|z|n; w_ih (3H,I), w_hh (3H,H), b_ih, b_hh (3H)) -- what the
 * reference's GRUWakeword wraps (src/models/architectures.py:228-235).  batch_first: x (B,T,I) with row stride ldx
 * between consecutive (b,t) rows, y (B,T,H) with row stride ldy (a bidirectional layer's two directions write the two
 * halves of one (B,T,2H) buffer: ldy = 2H, y offset by H for the reverse direction).  reverse != 0 runs t = T-1..0.
 * h0 nullable (zeros).  H = 128 only.  ws (ww_gru_workspace_bytes, 256-byte aligned) keeps the projections and the
 * gates between ww_gru_fwd and the ww_gru_bwd of the same (layer, direction).  ww_gru_bwd: dy (nullable) is the
 * gradient of y, dh_n (nullable) of the final hidden state; dx is written, or added to when accumulate_dx != 0.     */
size_t ww_gru_workspace_bytes(int B, int T, int I, int H);
/* Dropout on a (B,T,C) tensor of row-strided rows (nn.GRU's inter-layer dropout, the Dropout in front of GRUWakeword.fc,
 * architectures.py:232,239): out = keep ? x/(1-p) : 0 with keep from Philox ctr = (step, sample_offset + b,
 * TAG_DROPOUT<<24 | stream_id<<20 | t<<8 | c>>2), lane c&3.  Applying it to the gradient is its backward.          */
int ww_dropout_bt(ww_ctx *ctx, const float *x, long ldx, int B, int T, int C, float p, uint64_t seed, uint64_t step,
                  uint64_t sample_offset, int stream_id, float *out, long ldo, ww_stream_t stream);
int ww_gru_fwd(ww_ctx *ctx, int mode /* WW_ACT_F32 | WW_ACT_BF16: matrix type of the projection GEMMs */, const float *x, long ldx, const float *w_ih, const float *w_hh, const float *b_ih,
               const float *b_hh, const float *h0, int B, int T, int I, int H, int reverse, float *y, long ldy, float *h_n,
               void *ws, size_t ws_bytes, ww_stream_t stream);
int ww_gru_bwd(ww_ctx *ctx, int mode, const float *x, long ldx, const float *w_ih, const float *w_hh, const float *dy, long ldy,
               const float *dh_n, int B, int T, int I, int H, int reverse, void *ws, size_t ws_bytes, float *dx, long lddx,
               int accumulate_dx, float *dw_ih, float *dw_hh, float *db_ih, float *db_hh, float *dh0, ww_stream_t stream);

/* Both directions of a bidirectional layer (nn.GRU(bidirectional=True), architectures.py:228-235) with ONE recurrent launch per
 * pass: the persistent kernel runs direction 0 (t = 0..T-1) and direction 1 (t = T-1..0) as the two rows of its grid -- twice
 * the resident workgroups of a per-direction launch, no second stream, so a captured HIP graph keeps the concurrency that two
 * streams give an eager step.  y / dy: (B,T,2H) with row stride ldy >= 2H, direction d owns columns [d*H, (d+1)*H).  Each
 * direction has its own workspace (ww_gru_workspace_bytes, 256-byte aligned, kept from forward to backward).  Backward-only
 * members may be NULL in the forward call and vice versa; h0 / h_n / dh_n / dh0 are nullable.  dx = sum over both directions. */
typedef struct ww_gru_dir {
    const float *w_ih, *w_hh, *b_ih, *b_hh;      /* nn.GRU layout: (3H,I), (3H,H), (3H), (3H); gate order r|z|n */
    const float *h0;                             /* (B,H) initial state or NULL (zeros) */
    float *h_n;                                  /* (B,H) final state out, or NULL */
    void *ws;
    const float *dh_n;                           /* backward: gradient of h_n, or NULL */
    float *dw_ih, *dw_hh, *db_ih, *db_hh;        /* backward: parameter gradients (written) */
    float *dh0;                                  /* backward: gradient of h0 out, or NULL */
} ww_gru_dir;
int ww_gru_bidir_fwd(ww_ctx *ctx, int mode, const float *x, long ldx, const ww_gru_dir *dir /* [2] */, int B, int T, int I, int H,
                     float *y, long ldy, size_t ws_bytes, ww_stream_t stream);
int ww_gru_bidir_bwd(ww_ctx *ctx, int mode, const float *x, long ldx, const ww_gru_dir *dir /* [2] */, const float *dy, long ldy,
                     int B, int T, int I, int H, size_t ws_bytes, float *dx, long lddx, ww_stream_t stream);

/* ------------------------------------------------------------------ LSTM layer (the reference's LSTMWakeword)
 * torch.nn.LSTM's cell and parameter layout (gate order i|f|g|o; w_ih (4H,I), w_hh (4H,H), b_ih, b_hh (4H)) -- what the
 * reference's LSTMWakeword wraps (src/models/architectures.py: nn.LSTM(input, 128, num_layers, batch_first=True,
 * bidirectional)).  Same conventions as the GRU entry points above: x (B,T,I) with row stride ldx, y (B,T,H) with row stride
 * ldy, reverse != 0 runs t = T-1..0, H = 128 only, ws (ww_lstm_workspace_bytes, 256-byte aligned) kept from ww_lstm_fwd to the
 * ww_lstm_bwd of the same (layer, direction).  h0 / c0 nullable (zeros); h_n / c_n (B,H) outputs, nullable.  ww_lstm_bwd: dy,
 * dh_n and dc_n are nullable (at least one given); dx is written, or added to when accumulate_dx != 0; dh0 / dc0 nullable. */
size_t ww_lstm_workspace_bytes(int B, int T, int I, int H);
int ww_lstm_fwd(ww_ctx *ctx, int mode, const float *x, long ldx, const float *w_ih, const float *w_hh, const float *b_ih,
                const float *b_hh, const float *h0, const float *c0, int B, int T, int I, int H, int reverse, float *y, long ldy,
                float *h_n, float *c_n, void *ws, size_t ws_bytes, ww_stream_t stream);
int ww_lstm_bwd(ww_ctx *ctx, int mode, const float *x, long ldx, const float *w_ih, const float *w_hh, const float *dy, long ldy,
                const float *dh_n, const float *dc_n, int B, int T, int I, int H, int reverse, void *ws, size_t ws_bytes, float *dx,
                long lddx, int accumulate_dx, float *dw_ih, float *dw_hh, float *db_ih, float *db_hh, float *dh0, float *dc0,
                ww_stream_t stream);
/* Both directions of a bidirectional layer with ONE recurrent launch per pass (as ww_gru_bidir_*): y / dy (B,T,2H) with row
 * stride ldy >= 2H, direction d owns columns [d*H, (d+1)*H); one workspace per direction; dx = sum over both directions.   */
typedef struct ww_lstm_dir {
    const float *w_ih, *w_hh, *b_ih, *b_hh;      /* nn.LSTM layout: (4H,I), (4H,H), (4H), (4H); gate order i|f|g|o */
    const float *h0, *c0;                        /* (B,H) initial states or NULL (zeros) */
    float *h_n, *c_n;                            /* (B,H) final states out, or NULL */
    void *ws;
    const float *dh_n, *dc_n;                    /* backward: gradients of h_n / c_n, or NULL */
    float *dw_ih, *dw_hh, *db_ih, *db_hh;        /* backward: parameter gradients (written) */
    float *dh0, *dc0;                            /* backward: gradients of h0 / c0 out, or NULL */
} ww_lstm_dir;
int ww_lstm_bidir_fwd(ww_ctx *ctx, int mode, const float *x, long ldx, const ww_lstm_dir *dir /* [2] */, int B, int T, int I, int H,
                      float *y, long ldy, size_t ws_bytes, ww_stream_t stream);
int ww_lstm_bidir_bwd(ww_ctx *ctx, int mode, const float *x, long ldx, const ww_lstm_dir *dir /* [2] */, const float *dy, long ldy,
                      int B, int T, int I, int H, size_t ws_bytes, float *dx, long lddx, ww_stream_t stream);

/* Deferred partial sums.  The parameter-gradient kernels of the generic layers (ww_linear_mfma_bwd's split-K dW product,
 * ww_dwconv_nhwc_bwd, ww_stem3x3s2_bwd_dw) end in "sum the per-block partials into the gradient" -- a 4-5 us launch each that
 * nothing needs before the optimizer.  While ww_ctx_set_deferred_reduce(ctx, 1) is in force those calls QUEUE that last step
 * (their `scratch` argument then holds the partials and must stay untouched until the flush; dw / the gradient output is not
 * valid before it) and ww_deferred_reduce_flush runs everything queued as ONE launch (fixed order, double accumulation).
 * The autograd models flush at the end of backward (and before a mid-backward all-reduce).  Replaces nothing in the reference:
 * its weight gradients come out of cuDNN / cuBLAS calls (src/training/trainer.py:182).                                      */
int ww_ctx_set_deferred_reduce(ww_ctx *ctx, int on);
int ww_deferred_reduce_pending(ww_ctx *ctx);
int ww_deferred_reduce_flush(ww_ctx *ctx, ww_stream_t stream);
int ww_deferred_reduce_discard(ww_ctx *ctx);      /* forget what is queued (the backward pass that queued it did not complete) */

/* Fused clip + optimizer step on flat fp32 buckets.  Replaces, for one step, the reference's
 * clip_gradients(...) ; optimizer.step()  (src/training/trainer.py:185-193) with torch.optim's own update rules
 * (create_optimizer, src/training/optimizer_factory.py:165-199: Adam, AdamW, SGD with nesterov=True).
 * max_norm <= 0: norm only.  exp_avg doubles as SGD's momentum buffer; exp_avg_sq is unused for SGD (may be NULL).
 * step_state: int64[2] on the device, both 0 initially; call k reads slot[parity] and writes slot[parity^1]
 * (callers alternate parity 0,1,0,...).  When stats->found_inf != 0 (or the gradient norm is not finite) nothing is
 * updated and the step count does not advance -- the reference's "skip this batch" (trainer.py:177-179).
 * stats_host (nullable): PINNED host memory (hipHostMalloc / torch pin_memory) that receives a copy of *stats, written
 * by the kernel itself -- the step's single device->host record without a copy command in the stream.              */
enum { WW_OPT_ADAM = 0, WW_OPT_ADAMW = 1, WW_OPT_SGD = 2 };
typedef struct {
    int32_t kind;
    float lr, beta1, beta2, eps, weight_decay, momentum;
    float max_norm;    /* gradient_clip (src/config/defaults.py:48) */
} ww_optim_cfg;
int ww_clip_optim_step(ww_ctx *ctx, const ww_optim_cfg *cfg, float *flat_params, float *flat_grads, float *exp_avg,
                       float *exp_avg_sq, size_t n, int64_t *step_state, int parity, float *norm_out,
                       ww_step_stats *stats /* nullable */, ww_step_stats *stats_host /* nullable */,
                       ww_step_stats *stats_host_alt /* nullable; see ww_step_ctl */,
                       const float *found_inf_extra /* nullable: != 0 -> skip (another rank's verdict) */,
                       ww_loss_scale *loss_scale /* nullable: fp16 mode, slot = parity */, ww_stream_t stream);

/* ------------------------------------------------------------------ evaluation: the score stage after the logits
 * Replaces, per batch, what the reference's evaluator does on the host after copying the logits back: softmax and the
 * positive-class confidence (src/evaluation/evaluator.py:136-137, 220-221, 305-306, 379-380), the threshold decision
 * (:138, :222, :307; src/evaluation/inference.py:209-210), the 100-threshold ROC loop (evaluator.py:389-408) and the argmax
 * confusion counts MetricsCalculator.calculate takes from the collected logits (evaluator.py:321-324, src/training/metrics.py:
 * 105-116).  One launch per batch, no host synchronisation; the caller reads everything back once per dataset.
 *   scores      WW_SCORE_LOGITS: fp32 (B,2);  WW_SCORE_CONF: fp32 (B), already the positive-class confidence
 *   targets     int64 (B), nullable (nothing is counted per class then)
 *   thresholds  fp64 (K) on the device, ascending, 1 <= K <= WW_EVAL_MAX_THRESHOLDS;  decision: one fp64 threshold, not NaN
 * Per sample i, written at index offset + i of the dataset-long buffers conf / pred / bin (bin nullable):
 *   conf  fp32: exp(l1-m) / (exp(l0-m) + exp(l1-m)), m = max(l0,l1), or the copied score
 *   pred  uint8: (double)conf >= decision
 *   bin   int32: number of table entries t with (double)conf >= t  (NaN -> 0)
 * Accumulators, added to and never reset here: hist uint64 [2][K+1] indexed [target][bin] (targets 0 and 1 only) and the
 * counters below.  tp/tn/fp/fn compare the target with torch.argmax of the logits (a tie goes to class 0, a NaN logit wins,
 * the first NaN wins when both are); with WW_SCORE_CONF the predicted class is pred.  Every comparison is fp64 on the fp32
 * value, so the reference's three comparison semantics differ only in the table the host passes (DESIGN.md "Evaluation").
 * Counting is integer only (LDS partial histogram, then one atomic add per non-empty counter per workgroup): reproducible. */
#define WW_SCORE_LOGITS 0
#define WW_SCORE_CONF 1
#define WW_EVAL_MAX_THRESHOLDS 1024
typedef struct {
    uint64_t tp, tn, fp, fn;   /* argmax confusion counts over the samples whose target is 0 or 1 */
    uint64_t count;            /* samples seen */
    uint64_t bad_target;       /* targets outside {0,1} */
    uint64_t nan_score;        /* samples whose confidence is NaN */
    uint64_t reserved;
} ww_eval_counters;
int ww_eval_accumulate(ww_ctx *ctx, const float *scores, int score_kind, const int64_t *targets, int B,
                       const double *thresholds, int K, double decision, float *conf, uint8_t *pred, int32_t *bin,
                       size_t offset, uint64_t *hist, ww_eval_counters *counters, ww_stream_t stream);
/* The WW_SCORE_LOGITS form for logits (B,C), 2 <= C = num_classes <= WW_LOSS_MAX_CLASSES: conf = softmax(row)[1] with the
 * maximum over all C columns subtracted (src/evaluation/evaluator.py:379-380); pred, bin, hist and the counters as above, with
 * tp/tn/fp/fn from torch.argmax over the C columns (first maximum wins, a NaN wins, the first NaN wins) on targets 0 and 1.
 * Targets 2..C-1 are valid: they count in `count` only and stay out of hist, as the reference's ROC loop leaves them out
 * (evaluator.py:393-399); bad_target counts targets outside [0,C).  Already-computed confidences need no such form. */
int ww_eval_accumulate_classes(ww_ctx *ctx, const float *logits, int num_classes, const int64_t *targets, int B,
                               const double *thresholds, int K, double decision, float *conf, uint8_t *pred, int32_t *bin,
                               size_t offset, uint64_t *hist, ww_eval_counters *counters, ww_stream_t stream);
/* The chunking of MicrophoneInference's buffer loop (src/evaluation/inference.py:150-153) applied to a whole recording
 * wave (S) fp32 on the device: window w = wave[w*(chunk/2) .. +chunk), W = 0 if S < chunk else (S - chunk)/(chunk/2) + 1 (host
 * only: the first function below); out (W,chunk), peaks (W).  Each window is divided by its own peak max|x| when that is > 0
 * (:190-191) with a correctly rounded division -- bit-equal to NumPy's float32 x / peak; an all-zero window stays zero, a window
 * holding a NaN is copied unscaled (np.max returns the NaN and NaN > 0 is false) and its peak is NaN.  W must be the rule's. */
long ww_wave_num_windows(long S, int chunk);
int ww_wave_windows(ww_ctx *ctx, const float *wave, long S, int chunk, int W, float *out, float *peaks, ww_stream_t stream);

/* ------------------------------------------------------------------ evaluation: the dense detection scan
 * What the reference does not have: windows at any hop, a smoothed posterior, a refractory period after a trigger, triggers
 * matched to labelled keyword occurrences, counted at every threshold of a table -- false alarms per hour against miss rate.
 * One read-back per recording (DESIGN.md "Evaluation", evaluation/detection.py restates every law below in NumPy).
 *
 * Windows at a free hop, by slab.  W = 0 if S < chunk else (S - chunk)/hop + 1, 1 <= hop <= chunk (host only: the first
 * function below, 0 for a hop outside that range).  Window w0 + i = wave[(w0+i)*hop .. +chunk) for i in [0, n), 0 <= w0,
 * w0 + n <= W: out (n,chunk), peaks (n).  peaks[i] = max|x| of the window, NaN if it holds a NaN, always written.
 * normalize = 1: ww_wave_windows' law -- divided by its peak when that is > 0, correctly rounded; a zero window stays zero; a
 * window holding a NaN is copied unscaled.  normalize = 0: a plain copy.  An hour of windows is never materialised: the
 * caller cuts a slab, runs it through the front end and the model, and reuses the buffer.  One workgroup per window and
 * trip; honours ww_ctx_set_grid_cap, as ww_feat_windows does.  A window of more than WW_WAVE_SPLIT_CHUNK samples -- a whole
 * recording divided by its own peak is ONE window with chunk = hop = S -- is spread over a workgroup per 8192 samples instead
 * (an integer atomic maximum for the peak, then the division: the same bits). */
#define WW_WAVE_SPLIT_CHUNK 32768
long ww_wave_num_windows_hop(long S, int chunk, int hop);
int ww_wave_windows_at(ww_ctx *ctx, const float *wave, long S, int chunk, int hop, long w0, int n, int normalize, float *out,
                       float *peaks, ww_stream_t stream);
/* Windows of a feature map computed once over the whole recording: feat (F,Ttot) fp32, out (n,1,F,Tw),
 * out[i][0][f][t] = feat[f][(w0+i)*step + t], bit copied.  (w0+n-1)*step + Tw <= Ttot. */
int ww_feat_windows(ww_ctx *ctx, const float *feat, int F, long Ttot, int Tw, int step, long w0, int n, float *out,
                    ww_stream_t stream);
/* The detector over the W per-window confidences of one recording (conf fp32 (W) on the device).
 *   smoothing   1 <= M <= WW_DETECT_MAX_SMOOTH:  s_w = fp32( (0.0 + sum of fp64(conf_j), j = max(0, w-M+1) .. w, added in
 *               ascending j) / count ), the division in fp64, count = the number of terms.  A NaN propagates.
 *   triggers    one machine per table entry t and one for `decision`, each restarting at w = 0 on every call; R >= 1 is the
 *               refractory length in windows.  next_ok = 0; for w = 0 .. W-1: if w >= next_ok and fp64(s_w) >= t, trigger at
 *               w and set next_ok = w + R.  A NaN never triggers.  The comparison is fp64 on the fp32 value, as above.
 *   matching    events int32 (E,2) on the device, E >= 0: inclusive window-index intervals [a_e, b_e], a_e <= b_e < a_{e+1}.
 *               A trigger inside an event not yet hit by this threshold in this call is a hit, one inside an event already
 *               hit is a duplicate, one outside every event is a false alarm: triggers = hits + false alarms + duplicates.
 * thresholds fp64 (K) on the device, ascending, 1 <= K <= WW_EVAL_MAX_THRESHOLDS; decision: one fp64, not NaN.
 * Outputs: smoothed fp32 (W), nullable; counts uint64 (K,4) = {triggers, hits, false alarms, duplicates} per table entry and
 * decision_counts uint64 (4), both added to and never reset here; triggers int32 (max_triggers): the decision threshold's
 * trigger windows in order, the first max_triggers of them; n_triggers int32 (1): their full number in this call, which may
 * exceed max_triggers (written, not added to).  W = 0 is valid and changes nothing, n_triggers included.
 * False alarms are NOT monotone in the threshold: a lower threshold can trigger earlier and its refractory period swallow a
 * later false alarm, so every table entry runs its own machine -- one lane each; the smoothed sequence is staged through LDS
 * in tiles of WW_DETECT_TILE windows, events are consumed with a per-lane cursor.  Integer counting: reproducible. */
#define WW_DETECT_MAX_SMOOTH 64
#define WW_DETECT_TILE 1024
int ww_detect_accumulate(ww_ctx *ctx, const float *conf, int W, int M, int R, const double *thresholds, int K, double decision,
                         const int32_t *events, int E, float *smoothed, uint64_t *counts, uint64_t *decision_counts,
                         int32_t *triggers, int max_triggers, int32_t *n_triggers, ww_stream_t stream);

/* ------------------------------------------------------------------ loader: batches from a device-resident clip bank
 * The reference feeds its trainer from a host DataLoader over WakewordDataset (src/data, absent from the snapshot;
 * src/training/trainer.py:154-157 unpacks its batches).  Here the clips live on the device and ONE launch per batch draws
 * the clip of every sample, copies it (crop or zero-pad) and writes targets and clip indices.  Nothing is read back, and no
 * index tensor exists between the draw and the copy.  The laws are DESIGN.md §4 "Loader"; in short, with
 * g = rank + world * k the epoch position of this rank's k-th sample and Philox4x32-10 keyed by `seed`:
 *   WW_SAMPLER_PERM   shuffle != 0: clip = perm(g), a 4-round Feistel permutation of [0, n_clips) that depends on (seed,
 *                     epoch) alone -- the same on every rank, so the ranks' shards are disjoint; shuffle == 0: clip = g.
 *                     g must stay below n_clips (WW_E_INVALID otherwise).
 *   WW_SAMPLER_TABLE  with replacement: clip = first i with cdf[i] > u53(g, epoch) * 2^-53 * cdf[n_cdf-1], at most n_cdf-1;
 *                     cdf = fp64 inclusive cumulative weights on the device, n_cdf <= n_clips entries (the host cuts the
 *                     table after the last non-zero weight), last entry > 0.
 *   bank    int16 [n_clips][L], row stride L;  length int32 [n_clips], 0 <= length <= L (clamped);  label uint8 [n_clips]
 *   out     int16 (B, n_out), rows n_out apart, any 2-byte alignment: length > n_out -> n_out samples from offset
 *           mulhi32(philox(g, epoch)[0], length - n_out + 1) when training, 0 otherwise; else the clip, then zeros
 *   targets int64 (B) = label[clip];  clip_index int32 (B) = clip
 * k0 is the first sample of the launch (k = k0 .. k0 + B - 1); only the low 32 bits of epoch enter the counters.
 * ww_loader_indices writes the drawn clips alone, for any k0 / count. */
#define WW_SAMPLER_PERM 0
#define WW_SAMPLER_TABLE 1
int ww_loader_indices(ww_ctx *ctx, int n_clips, int strategy, int shuffle, const double *cdf /* TABLE only */, int n_cdf,
                      uint64_t seed, uint64_t epoch, int rank, int world, int64_t k0, int count, int32_t *index_out,
                      ww_stream_t stream);
int ww_loader_batch(ww_ctx *ctx, const int16_t *bank, const int32_t *length, const uint8_t *label, int n_clips, int L,
                    int strategy, int shuffle, int training, const double *cdf /* TABLE only */, int n_cdf, uint64_t seed,
                    uint64_t epoch, int rank, int world, int64_t k0, int B, int n_out, int16_t *out, int64_t *targets,
                    int32_t *clip_index, ww_stream_t stream);

/* ------------------------------------------------------------------ int8 inference of an exported cnn_small bundle
 * The reference exports through ONNX and leaves the quantised network to onnxruntime (src/export/onnx_exporter.py:225-254); here
 * the export package writes an int8 bundle and these entry points run it with integer arithmetic only -- the law is DESIGN.md
 * "Export".  Activations are int8 NHWC (B,H,W,64); every tensor is 16-byte aligned.  Per conv:
 *   w      int8: stem and depthwise (9,64) [tap kh*3+kw][channel], pointwise (64,64) [out][in]
 *   bias   int32 (64): the EFFECTIVE bias q_b - z_in * sum(q_w over the channel's weights), wrapped to 32 bits -- with the
 *          border filled with z_in, sum q_w q_in + bias is the law's sum q_w (q_in - z_in) + q_b in two's complement
 *   mult   int32 (64) in [2^30, 2^31), shift int32 (64) in [1, 62]
 *   q_out = clamp(-128 + ((int64(acc) * mult + 2^(shift-1)) >> shift), -128, 127)          (z_out = -128: the ReLU)
 * ww_q8_quantize: q = clamp(rne(x / scale) + zero, -128, 127), one correctly rounded fp32 division; NaN -> zero, +-inf saturate.
 * ww_q8_stem_fwd: xq int8 (B,F,T) -> (B,(F+1)/2,(T+1)/2,64), 3x3 stride 2 pad 1.  ww_q8_dwconv3x3_fwd: 3x3 pad 1 per channel.
 * ww_q8_pwconv1x1_fwd: (N,64) -> (N,64) on v_mfma_i32_16x16x64_i8.  ww_q8_dwpw_fwd: the last two as one kernel, bit-equal.
 * ww_q8_gap_fc_fwd: S[c] = sum_hw (q + 128); pool_out int8 (B,64) = the requantised S (pool_mult, pool_shift);
 *   logits[k] = float32(sum_c fc_w[k][c] (pool[c] + 128) + fc_bias[k]) * fc_scale[k] -- fc_bias is the law's q_b, not an
 *   effective bias; fc_w int8 (2,64), fc_bias int32 (2), fc_scale fp32 (2).
 * The whole model: tab = WW_Q8_NPTR device pointers [stem w, bias, mult, shift] + 4 x [dw w, bias, mult, shift, pw w, bias, mult,
 * shift] + [fc_w, fc_bias, fc_scale]; io on the host.  The workspace holds, each rounded up to 256 bytes: xq (B*F*T), then
 * WW_Q8_NACT activation tensors of B*H*W*64 (stem, dw0, pw0, .. dw3, pw3), then pool (B*64).  form WW_Q8_FUSED leaves the dw
 * slots unwritten.  Nothing synchronises with the host. */
#define WW_Q8_NPTR 39
#define WW_Q8_NACT 9
#define WW_Q8_PAIR 0
#define WW_Q8_FUSED 1
typedef struct {
    float in_scale;      /* s_x */
    int32_t in_zero;     /* z_x */
    int32_t pool_mult;   /* m_p */
    int32_t pool_shift;  /* sh_p */
} ww_q8_io;
int ww_q8_quantize(ww_ctx *ctx, const float *x, long n, float scale, int zero, int8_t *out, ww_stream_t stream);
int ww_q8_stem_fwd(ww_ctx *ctx, const int8_t *xq, const int8_t *w, const int32_t *bias, const int32_t *mult, const int32_t *shift,
                   int B, int F, int T, int zero, int8_t *out, ww_stream_t stream);
int ww_q8_dwconv3x3_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult,
                        const int32_t *shift, int B, int H, int W, int zero, int8_t *out, ww_stream_t stream);
int ww_q8_pwconv1x1_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult,
                        const int32_t *shift, long N, int8_t *out, ww_stream_t stream);
int ww_q8_dwpw_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w_dw, const int32_t *bias_dw, const int32_t *mult_dw,
                   const int32_t *shift_dw, const int8_t *w_pw, const int32_t *bias_pw, const int32_t *mult_pw,
                   const int32_t *shift_pw, int B, int H, int W, int zero, int8_t *out, ww_stream_t stream);
int ww_q8_gap_fc_fwd(ww_ctx *ctx, const int8_t *in, int B, int HW, int pool_mult, int pool_shift, const int8_t *fc_w,
                     const int32_t *fc_bias, const float *fc_scale, int8_t *pool_out, float *logits, ww_stream_t stream);
size_t ww_q8_cnn_small_workspace_bytes(int B, int F, int T);
int ww_q8_cnn_small_fwd(ww_ctx *ctx, const void *const *tab, const ww_q8_io *io, const float *x, int B, int F, int T, int form,
                        void *ws, size_t ws_bytes, float *logits, ww_stream_t stream);

/* ------------------------------------------------------------------ int8 inference of an exported TCNWakeword bundle
 * The same law with one more rule, the residual add (DESIGN.md "Export", subsection "TCN"); ww_q8_tcn.hip.  Activations are int8
 * rows (B*T, Cp), Cp = the channel count rounded up to 64; pad channels hold the tensor's zero point (z_x for the quantised
 * features, -128 for everything a conv or an add writes).  Every tensor is 16-byte aligned.  Per conv (k taps, dilation d):
 *   w      int8 (Cpo, k, Cpi) [out][tap][in]; pad rows and pad columns are zero
 *   bias   int32 (Cpo): the EFFECTIVE bias q_b - z_in * sum(q_w); mult int32 (Cpo) in [2^30, 2^31), shift int32 (Cpo) in [1, 62];
 *          pad channels: bias 0, mult 2^30, shift 31, so they come out as -128
 *   acc[t][n] = sum_j sum_c w[n][j][c] * in[t - (k-1-j) d][c] + bias[n], a source time below 0 reading `zero`
 *   residual == NULL:  out = clamp(-128 + R(acc, mult, shift), -128, 127), R(a, m, sh) = (int64(a) m + 2^(sh-1)) >> sh
 *   residual (N, Cpo): out = clamp(-128 + R(acc, mult, shift) + R(residual + 128, res_mult, res_shift), -128, 127) -- the
 *          downsample conv carrying the block's add and last ReLU
 * ww_tq8_quantize_bt: x fp32 (B,F,T) -> int8 (B*T, Fp), the input rule of ww_q8_quantize, transposed; pad channels = zero.
 * ww_tq8_skip_add_fwd: out = clamp(-128 + R(in - zero, skip_mult, skip_shift) + R(h2 + 128, add_mult, add_shift), -128, 127).
 * ww_tq8_pool_fc_fwd: S[c] = sum_t (q + 128); pool_out int8 (B, C) = the requantised S; logits (B, num_classes) =
 *   float32(sum_c fc_w[k][c] (pool[c] + 128) + fc_bias[k]) * fc_scale[k]; fc_w int8 (num_classes, C), UNPADDED, fc_bias the law's q_b.
 * The whole model: tab = per block WW_TQ8_BLOCK_NPTR device pointers [conv1 w, bias, mult, shift, conv2 .., downsample ..] (the last
 * four NULL for an identity skip), then [fc_w, fc_bias, fc_scale]; io on the host.  Block i has dilation 2^i.  The workspace holds,
 * each rounded up to 256 bytes: xq (B*T*Fp), then per block h1, h2, out (B*T*Cp_i each), then pool (B*C_last) -- that sum is what
 * the workspace-size entry point returns.  Nothing synchronises with the host. */
#define WW_TQ8_MAX_BLOCKS 8
#define WW_TQ8_BLOCK_NPTR 12
typedef struct {
    float in_scale;                         /* s_x */
    int32_t in_zero;                        /* z_x */
    int32_t pool_mult, pool_shift;
    int32_t n_blocks, kernel_size, input_size, num_classes;
    int32_t channels[WW_TQ8_MAX_BLOCKS];    /* unpadded */
    int32_t add_mult[WW_TQ8_MAX_BLOCKS], add_shift[WW_TQ8_MAX_BLOCKS];
    int32_t skip_mult[WW_TQ8_MAX_BLOCKS], skip_shift[WW_TQ8_MAX_BLOCKS];   /* identity skips only */
} ww_tq8_io;
int ww_tq8_quantize_bt(ww_ctx *ctx, const float *x, int B, int F, int T, int Fp, float scale, int zero, int8_t *out,
                       ww_stream_t stream);
int ww_tq8_conv1d_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult,
                      const int32_t *shift, int B, int T, int Cpi, int Cpo, int k, int dilation, int zero, const int8_t *residual,
                      int res_mult, int res_shift, int8_t *out, ww_stream_t stream);
int ww_tq8_skip_add_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *h2, long N, int Cp, int zero, int skip_mult, int skip_shift,
                        int add_mult, int add_shift, int8_t *out, ww_stream_t stream);
int ww_tq8_pool_fc_fwd(ww_ctx *ctx, const int8_t *in, int B, int T, int C, int Cp, int pool_mult, int pool_shift, const int8_t *fc_w,
                       const int32_t *fc_bias, const float *fc_scale, int num_classes, int8_t *pool_out, float *logits,
                       ww_stream_t stream);
size_t ww_tq8_tcn_workspace_bytes(int B, int F, int T, int n_blocks, const int32_t *channels);
int ww_tq8_tcn_fwd(ww_ctx *ctx, const void *const *tab, const ww_tq8_io *io, const float *x, int B, int T, void *ws, size_t ws_bytes,
                   float *logits, ww_stream_t stream);

/* ------------------------------------------------------------------ int8 inference of an exported ResNet18Wakeword bundle
 * The same law with the rules of its subsection "ResNet18" (DESIGN.md "Export"); ww_q8_resnet.hip.  Activations are int8 NHWC
 * (B,H,W,C), C a multiple of 64; every tensor is 16-byte aligned.  Per conv (k = 1 or 3, stride 1 or 2, pad k / 2):
 *   w      int8 (Cout, k*k, Cin) [out][tap kh*k+kw][in]
 *   bias   int32 (Cout): the EFFECTIVE bias q_b - z_in * sum(q_w); mult int32 (Cout) in [2^30, 2^31), shift int32 (Cout) in [1, 62]
 *   acc[b,ho,wo,n] = sum_{kh,kw,c} w[n][kh*k+kw][c] * in[b, ho s - p + kh, wo s - p + kw, c] + bias[n], a source pixel outside the
 *   image reading `zero`;  R(a, m, sh) = (int64(a) m + 2^(sh-1)) >> sh
 *   WW_RQ8_RELU:   out = clamp(-128 + R(acc, mult, shift), -128, 127)
 *   WW_RQ8_SIGNED: out = clamp(R(acc, mult, shift), -128, 127)                                    (the downsample conv, z_out = 0)
 *   WW_RQ8_ADD:    out = clamp(-128 + R(acc, mult, shift) + R(residual - res_zero, res_mult, res_shift), -128, 127), residual (N, Cout)
 * ww_rq8_stem_fwd: xq int8 (B,F,T) -> (B,(F-1)/2+1,(T-1)/2+1,64), 7x7 stride 2 pad 3, RELU epilogue; w (64,64) [channel][tap kh*7+kw],
 *   the taps 49..63 zero: a pixel's window padded to 64 bytes is one K chunk of the matrix instruction.
 * ww_rq8_maxpool_fwd: 3x3 stride 2 pad 1, the maximum over the window positions inside the image.
 * The whole model: tab = WW_RQ8_NPTR device pointers [stem w, bias, mult, shift] + 8 x [conv1 w, bias, mult, shift, conv2 ..,
 * downsample ..] (the last four NULL except in blocks 2, 4 and 6) + [fc_w, fc_bias, fc_scale]; io on the host.  Quantisation is
 * ww_q8_quantize, pooling and the classifier ww_tq8_pool_fc_fwd.  The workspace holds, each rounded up to 256 bytes: xq (B*F*T),
 * stem, pool0, then per block h1, ds (blocks 2, 4, 6 only) and out, then pool (B*512).  Nothing synchronises with the host. */
#define WW_RQ8_NPTR 103
#define WW_RQ8_RELU 0
#define WW_RQ8_SIGNED 1
#define WW_RQ8_ADD 2
typedef struct {
    float in_scale;                         /* s_x */
    int32_t in_zero;                        /* z_x */
    int32_t pool_mult, pool_shift;
    int32_t num_classes;
    int32_t res_mult[8], res_shift[8];      /* m_r, sh_r of each block's add */
} ww_rq8_io;
int ww_rq8_conv2d_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult,
                      const int32_t *shift, int B, int H, int W, int Cin, int Cout, int k, int stride, int zero, int epilogue,
                      const int8_t *residual, int res_zero, int res_mult, int res_shift, int8_t *out, ww_stream_t stream);
int ww_rq8_stem_fwd(ww_ctx *ctx, const int8_t *xq, const int8_t *w, const int32_t *bias, const int32_t *mult, const int32_t *shift,
                    int B, int F, int T, int zero, int8_t *out, ww_stream_t stream);
int ww_rq8_maxpool_fwd(ww_ctx *ctx, const int8_t *in, int B, int H, int W, int C, int8_t *out, ww_stream_t stream);
size_t ww_rq8_resnet18_workspace_bytes(int B, int F, int T);
int ww_rq8_resnet18_fwd(ww_ctx *ctx, const void *const *tab, const ww_rq8_io *io, const float *x, int B, int F, int T, void *ws,
                        size_t ws_bytes, float *logits, ww_stream_t stream);

/* ------------------------------------------------------------------ int8 inference of an exported LSTMWakeword bundle
 * The same law with the rules of its subsection "LSTM" (DESIGN.md "Export"); ww_q8_lstm.hip.  Hidden size 128; a direction has 512
 * gate rows in torch's order i, f, g, o; nd = 1 or 2 directions, forward first.  Every tensor is 16-byte aligned.
 * ww_lq8_proj_fwd: the input projection of all nd directions of a layer over N = B*T rows.
 *   in     int8 (N, Kp), Kp a multiple of 64: the quantised features (ww_tq8_quantize_bt, pad channels = z_x) or the previous
 *          layer's y (Kp = nd * 128)
 *   w      int8 (G, Kp), G = nd * 512, the directions stacked; pad columns are zero.  G = nd * 384 is accepted too: the same
 *          projection over a GRU's r, z, n rows (ww_cq8_* below)
 *   bias   int32 (G): the EFFECTIVE bias q_bi - z_in * sum(q_wi); mult int32 (G) in [2^30, 2^31), shift int32 (G) in [1, 62]
 *   u[n][r] = clamp(R(sum_k w[r][k] in[n][k] + bias[r], mult[r], shift[r]), -32768, 32767) as int16 (N, G): Q8 gate pre-activations;
 *   R(a, m, sh) = (int64(a) m + 2^(sh-1)) >> sh
 * ww_lq8_lstm_layer_fwd: the recurrence of one layer, all directions in one launch.  w_hh int8 (G, 128); bias int32 (G) is the
 *   law's q_bh (q_h has zero point 0); mult, shift as above; tab_sigmoid, tab_tanh int16 (4096) are the bundle's tables.  Per
 *   direction and step, with q_h = 0 and c = 0 before the first: a = u[t] + R(sum_k w_hh[r][k] q_h[k] + bias[r], mult[r], shift[r]);
 *   i, f, o = look(sigmoid, a), g = look(tanh, a), look(tab, a) = tab[clamp(a, -2048, 2047) + 2048];
 *   c = clamp((f c + ((i g + 8) >> 4) + 2^14) >> 15, -32768, 32767); h16 = (o look(tanh, (c + 4) >> 3) + 2^14) >> 15;
 *   q_h = clamp((h16 + 128) >> 8, -128, 127).  The reverse direction walks t = T-1 .. 0.  y int8 (B*T, nd*128) holds q_h of every step
 *   in time order, the forward direction's 128 channels first; c_n int16 (B, nd*128) the cell after each direction's last step.
 *   WW_LQ8_TABLES=global in the environment reads the tables through the caches instead of LDS (same bits; the A/B switch).
 * ww_lq8_head_fwd: hcat int8 (B, nd*128) = [y[b][T-1][0:128], y[b][0][128:256]]; logits (B, num_classes) =
 *   float32(sum_k fc_w[c][k] hcat[k] + fc_bias[c]) * fc_scale[c]; fc_w int8 (num_classes, nd*128), fc_bias the law's q_b.
 * The whole model: tab = per layer WW_LQ8_LAYER_NPTR device pointers [w_ih, bias, mult, shift, w_hh, bias, mult, shift] (directions
 * stacked, as above), then WW_LQ8_TAIL_NPTR: [fc_w, fc_bias, fc_scale, tab_sigmoid, tab_tanh]; io on the host; x fp32 (B,F,T).  The
 * workspace holds, each rounded up to 256 bytes: xq (B*T*Fp), then per layer u (B*T*nd*512 int16), y (B*T*nd*128), c_n (B*nd*128
 * int16), then hcat (B*nd*128) -- that sum is what the workspace-size entry point returns.  Nothing synchronises with the host. */
#define WW_LQ8_MAX_LAYERS 8
#define WW_LQ8_LAYER_NPTR 8
#define WW_LQ8_TAIL_NPTR 5
typedef struct {
    float in_scale;                         /* s_x */
    int32_t in_zero;                        /* z_x */
    int32_t input_size, num_layers, num_directions, num_classes;
} ww_lq8_io;
int ww_lq8_proj_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult, const int32_t *shift,
                    long N, int Kp, int G, int16_t *u, ww_stream_t stream);
int ww_lq8_lstm_layer_fwd(ww_ctx *ctx, const int16_t *u, const int8_t *w_hh, const int32_t *bias, const int32_t *mult,
                          const int32_t *shift, const int16_t *tab_sigmoid, const int16_t *tab_tanh, int B, int T, int num_directions,
                          int8_t *y, int16_t *c_n, ww_stream_t stream);
int ww_lq8_head_fwd(ww_ctx *ctx, const int8_t *y, int B, int T, int num_directions, const int8_t *fc_w, const int32_t *fc_bias,
                    const float *fc_scale, int num_classes, int8_t *hcat, float *logits, ww_stream_t stream);
size_t ww_lq8_lstm_workspace_bytes(int B, int T, int input_size, int num_layers, int num_directions);
int ww_lq8_lstm_fwd(ww_ctx *ctx, const void *const *tab, const ww_lq8_io *io, const float *x, int B, int T, void *ws, size_t ws_bytes,
                    float *logits, ww_stream_t stream);

/* ------------------------------------------------------------------ int8 inference of an exported CRNNWakeword bundle
 * The same law with the rules of its subsections "GRU" and "CRNN" (DESIGN.md "Export"); ww_q8_crnn.hip.  The conv stack is
 * cnn_small's (ww_q8_quantize, ww_q8_stem_fwd, ww_q8_dwpw_fwd), the projection ww_lq8_proj_fwd at G = nd * 384, the head
 * ww_lq8_head_fwd.  Hidden size 128; a direction has 384 gate rows in torch's order r, z, n; nd = 1 or 2 directions, forward first.
 * Every tensor is 16-byte aligned.
 * ww_cq8_fmean_fwd: the frequency mean.  in int8 NHWC (B,H,W,64), z = -128 (H the frequency axis, W the time axis);
 *   S[b][w][c] = sum_h (in[b][h][w][c] + 128); out int8 (B*W, 64) rows = clamp(-128 + R(S, mult, shift), -128, 127);
 *   R(a, m, sh) = (int64(a) m + 2^(sh-1)) >> sh.  Persistent; honours ww_ctx_set_grid_cap.
 * ww_cq8_gru_layer_fwd: the recurrence of one GRU layer, all directions in one launch.  u int16 (B*T, G), G = nd * 384: the Q8
 *   input projection; w_hh int8 (G, 128); bias int32 (G) is the law's q_bh (q_h has zero point 0); mult int32 (G) in [2^30, 2^31),
 *   shift int32 (G) in [1, 62]; tab_sigmoid, tab_tanh int16 (4096) are the bundle's tables.  Per direction and step, with q_h = 0
 *   and h16 = 0 before the first: v = R(sum_k w_hh[row][k] q_h[k] + bias[row], mult[row], shift[row]) in int64, unclamped;
 *   r = look(sigmoid, u_r + v_r), z = look(sigmoid, u_z + v_z), n = look(tanh, u_n + ((r v_n + 2^14) >> 15)), the product in int64,
 *   look(tab, a) = tab[clamp(a, -2048, 2047) + 2048]; h16 = ((32768 - z) n + z h16 + 2^14) >> 15 (|h16| <= 32767, no clamp);
 *   q_h = clamp((h16 + 128) >> 8, -128, 127).  The reverse direction walks t = T-1 .. 0.  y int8 (B*T, nd*128) holds q_h of every step
 *   in time order, the forward direction's 128 channels first; h_n int16 (B, nd*128) is h16 after each direction's last step.
 * The whole model: tab = WW_CQ8_CONV_NPTR device pointers [stem w, bias, mult, shift] + 4 x [dw w, bias, mult, shift, pw w, bias,
 * mult, shift] (as ww_q8_cnn_small_fwd), then per layer WW_CQ8_LAYER_NPTR [w_ih, bias, mult, shift, w_hh, bias, mult, shift]
 * (directions stacked, w_ih's bias the EFFECTIVE bias, as ww_lq8_lstm_fwd), then WW_CQ8_TAIL_NPTR: [fc_w, fc_bias, fc_scale,
 * tab_sigmoid, tab_tanh]; io on the host; x fp32 (B,F,T), any T >= 1.  Launches: quantize, stem, 4 x dwpw, fmean, per layer
 * (projection, recurrence), head.  With H' = (F+1)/2, W' = (T+1)/2 the workspace holds, each rounded up to 256 bytes: xq (B*F*T),
 * WW_CQ8_NACT activation tensors of B*H'*W'*64 (stem, pw0 .. pw3: the depthwise outputs stay in registers), seq (B*W'*64), per
 * layer u (B*W'*nd*384 int16), y (B*W'*nd*128), h_n (B*nd*128 int16), then hcat (B*nd*128) -- that sum is what the
 * workspace-size entry point returns.  Nothing synchronises with the host. */
#define WW_CQ8_MAX_LAYERS 8
#define WW_CQ8_CONV_NPTR 36
#define WW_CQ8_LAYER_NPTR 8
#define WW_CQ8_TAIL_NPTR 5
#define WW_CQ8_NACT 5
typedef struct {
    float in_scale;                         /* s_x */
    int32_t in_zero;                        /* z_x */
    int32_t fmean_mult, fmean_shift;        /* m_f, sh_f */
    int32_t num_layers, num_directions, num_classes;
} ww_cq8_io;
int ww_cq8_fmean_fwd(ww_ctx *ctx, const int8_t *in, int B, int H, int W, int mult, int shift, int8_t *out, ww_stream_t stream);
int ww_cq8_gru_layer_fwd(ww_ctx *ctx, const int16_t *u, const int8_t *w_hh, const int32_t *bias, const int32_t *mult,
                         const int32_t *shift, const int16_t *tab_sigmoid, const int16_t *tab_tanh, int B, int T, int num_directions,
                         int8_t *y, int16_t *h_n, ww_stream_t stream);
size_t ww_cq8_crnn_workspace_bytes(int B, int F, int T, int num_layers, int num_directions);
int ww_cq8_crnn_fwd(ww_ctx *ctx, const void *const *tab, const ww_cq8_io *io, const float *x, int B, int F, int T, void *ws,
                    size_t ws_bytes, float *logits, ww_stream_t stream);

/* ------------------------------------------------------------------ int8 inference of a MobileNetV3Wakeword bundle (ww_q8_mobilenet.hip)
 * The int8 law's subsection "MobileNetV3" (DESIGN.md 5.6).  Activations are int8 NHWC (B,H,W,Cp), Cp = the channel count rounded up
 * to 64; pad channels hold the tensor's zero point and meet zero weights, pad OUTPUT channels have zero weights, a zero bias, mult 2^30
 * and shift 31, so they come out as the zero point of the tensor written.  Conv bias arguments are the EFFECTIVE bias
 * q_b - z_in * sum(q_w); the squeeze-excitation's and classifier.3's are the law's q_b.  Epilogues, R as everywhere:
 *   WW_MQ8_RELU:   out = clamp(-128 + R(acc, mult, shift), -128, 127)
 *   WW_MQ8_HSWISH: u = clamp(zero_u + R(acc, mult, shift), -128, 127), out = tab[u + 128]          (tab: the layer's int8 table, 256)
 *   WW_MQ8_SIGNED: out = clamp(R(acc, mult, shift) [+ R(residual, res_mult, res_shift)], -128, 127) (z_out = 0; residual (N, Cout), z = 0)
 * conv1x1: in (N, Cin), w (Cout, Cin), a GEMM on v_mfma_i32_16x16x64_i8, persistent under the grid cap; rows are pixels of the whole batch.
 * dwconv: w (k k, Cp) [tap][channel], k = 3 or 5, stride 1 or 2, pad k / 2, output (n - 1) / 2 + 1 at stride 2; window positions outside
 * the image read as `zero`.  stem: xq (B,F,T) -> (B,(F-1)/2+1,(T-1)/2+1,Cp), 3x3 stride 2 pad 1, w (9, Cp), Hardswish epilogue.
 * se: one workgroup per image -- pool = clamp(zero + R(sum_hw (q - zero), pool_mult, pool_shift)) (B, Cp), h = fc1 + ReLU (B, Csq),
 * gate = clamp(R(fc2 acc, m2, sh2), 0, 255) uint8 (B, Cp), pad gates 0; w1 (Csq, C), w2 (C, Csq) unpadded.
 * gate: y = clamp(zero + R((q - zero) * gate, gate_mult, gate_shift), -128, 127) -- the PASS form of the gate multiply.  The FUSED form:
 * conv1x1 with `gate` (N / HW, Cin) applies the same expression to the pixel fragments it loads (signed epilogue only), so `in` is the
 * un-gated tensor and no y is stored; both forms give the same bits.  The whole forward picks by WW_MQ8_GATE=pass | fused in the
 * environment, read at every call (default: pass); in the fused form the workspace's y tensors are not written.
 * head: in (B, HW, 576) -> pool (B, 576), hidden (B, 1024) = classifier.0 under the Hardswish epilogue (w0 (1024, 576), effective
 * bias), logits[c] = float(sum w[c] (hidden - zero_h) + fc_bias[c]) * fc_scale[c].
 * The whole model: tab = WW_MQ8_NPTR device pointers [stem w, bias, mult, shift, tab] + 11 x [expand w, bias, mult, shift, tab,
 * dw w, bias, mult, shift, tab, fc1 w, b, m, sh, fc2 w, b, m, sh, project w, bias, mult, shift] + [last w, bias, mult, shift, tab,
 * cls0 w, bias, mult, shift, tab, fc w, bias, scale]; entries a block does not have (no expand conv, no squeeze-excitation, the table
 * of a ReLU layer) are NULL.  The workspace keeps every tensor the launches write, each at a 256-byte boundary, in the order xq, stem,
 * per block [expand], dw, [pool, h, gate, y], out, then last, pool, hidden. */
#define WW_MQ8_BLOCKS 11
#define WW_MQ8_BLOCK_NPTR 22
#define WW_MQ8_NPTR 260
#define WW_MQ8_LAST 576
#define WW_MQ8_HIDDEN 1024
#define WW_MQ8_RELU 0
#define WW_MQ8_HSWISH 1
#define WW_MQ8_SIGNED 2
typedef struct {
    float in_scale;
    int32_t in_zero, num_classes;
    int32_t stem_zu, stem_zo, last_zu, last_zo, cls_zu, cls_zo;   /* zero points of the Hardswish pre-activations and outputs */
    int32_t pool_mult, pool_shift;
    int32_t exp_zu[WW_MQ8_BLOCKS], exp_zo[WW_MQ8_BLOCKS], dw_zu[WW_MQ8_BLOCKS], dw_zo[WW_MQ8_BLOCKS];
    int32_t sepool_mult[WW_MQ8_BLOCKS], sepool_shift[WW_MQ8_BLOCKS], gate_mult[WW_MQ8_BLOCKS], gate_shift[WW_MQ8_BLOCKS];
    int32_t res_mult[WW_MQ8_BLOCKS], res_shift[WW_MQ8_BLOCKS];
} ww_mq8_io;
int ww_mq8_conv1x1_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult, const int32_t *shift,
                       long N, int Cin, int Cout, int zero, int epilogue, int zero_u, const int8_t *tab, const int8_t *residual,
                       int res_mult, int res_shift, const uint8_t *gate /* nullable */, int HW, int gate_mult, int gate_shift, int8_t *out,
                       ww_stream_t stream);
int ww_mq8_dwconv_fwd(ww_ctx *ctx, const int8_t *in, const int8_t *w, const int32_t *bias, const int32_t *mult, const int32_t *shift,
                      int B, int H, int W, int Cp, int k, int stride, int zero, int epilogue, int zero_u, const int8_t *tab, int8_t *out,
                      ww_stream_t stream);
int ww_mq8_stem_fwd(ww_ctx *ctx, const int8_t *xq, const int8_t *w, const int32_t *bias, const int32_t *mult, const int32_t *shift,
                    int B, int F, int T, int Cp, int zero, int zero_u, const int8_t *tab, int8_t *out, ww_stream_t stream);
int ww_mq8_se_fwd(ww_ctx *ctx, const int8_t *in, int B, int HW, int C, int Cp, int Csq, int zero, int pool_mult, int pool_shift,
                  const int8_t *w1, const int32_t *b1, const int32_t *m1, const int32_t *sh1, const int8_t *w2, const int32_t *b2,
                  const int32_t *m2, const int32_t *sh2, int8_t *pool_out, int8_t *h_out, uint8_t *gate_out, ww_stream_t stream);
int ww_mq8_gate_fwd(ww_ctx *ctx, const int8_t *in, const uint8_t *gate, int B, int HW, int Cp, int zero, int gate_mult, int gate_shift,
                    int8_t *out, ww_stream_t stream);
int ww_mq8_head_fwd(ww_ctx *ctx, const int8_t *in, int B, int HW, int zero, int pool_mult, int pool_shift, const int8_t *w0,
                    const int32_t *b0, const int32_t *m0, const int32_t *sh0, int zero_u, const int8_t *tab, int zero_h,
                    const int8_t *fc_w, const int32_t *fc_bias, const float *fc_scale, int num_classes, int8_t *pool_out,
                    int8_t *hidden_out, float *logits, ww_stream_t stream);
size_t ww_mq8_mobilenetv3_workspace_bytes(int B, int F, int T);
int ww_mq8_mobilenetv3_fwd(ww_ctx *ctx, const void *const *tab, const ww_mq8_io *io, const float *x, int B, int F, int T, void *ws,
                           size_t ws_bytes, float *logits, ww_stream_t stream);

/* ------------------------------------------------------------------ collectives: deliberately NOT in this ABI
 * SURVEY.md §8b sketched two more entry points, `ww_comm_init` (ctx, nccl_unique_id, rank, world) and `ww_allreduce_f32`
 * (ctx, buf, n, avg, comm_stream).
 * They are waived: the exchange step of this path is ONE averaged all-reduce of the flat fp32 gradient bucket (two
 * ranges of it, see WW_BWD_LATE/EARLY above), and the host side of the boundary is Python on PyTorch-ROCm, whose
 * torch.distributed "nccl" backend IS RCCL over xGMI -- a second communicator owned by this library would duplicate
 * rendezvous, stream ordering and error handling that the host already has, and would add nothing on the device side
 * (RCCL's kernels are the collective; there is no fused reduce+clip kernel to hide behind an entry point).  What the ABI
 * does provide for data parallelism: gradients in one contiguous bucket (`grads` table -> flat buffer), the backward in
 * two calls so the first range can be reduced under the second, the found_inf slot that travels with the gradients
 * (ww_ce2_loss_fwd_bwd / ww_clip_optim_step), and Philox streams addressed by GLOBAL sample index (sample_offset).
 * The reference itself is single-GPU (README.md:253-254).                                                            */

/* ------------------------------------------------------------------ measurement
 * Opt-in timing of kernel classes with hipEvents recorded on the launch stream around the
 * class's main kernel (bench.py's roofline leg; no reference counterpart -- the reference never
 * measures, src/ui/panel_training.py:69,484).  ww_prof_collect synchronises on the recorded events
 * and returns, per class, the summed milliseconds and the number of launches since the last call. */
int ww_prof_num_classes(void);
const char *ww_prof_class_name(int cls);
int ww_prof_enable(ww_ctx *ctx, uint32_t class_mask);
int ww_prof_collect(ww_ctx *ctx, float *ms_sum, int32_t *count);

/* floor(p * 2^32) clamped to [0, 2^32] -- the integer probability threshold of the specs  */
uint64_t ww_prob_threshold(double p);
/* Philox4x32-10, exported so host tests can pin the device RNG's law (oracle/philox.py)   */
void ww_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* WWHIP_H */
