/*
 * ake_hip.h -- C ABI of libake_hip.so, the MI355X (gfx950) implementation of the
 * key-estimation hot path:  waveform -> CQT log-magnitude -> PitchClassNet forward.
 *
 * The reference (flo-stilz/Audio-Key-Estimation) is pure Python and defines no FFI;
 * each entry point below names the reference call it stands in for (file:line into
 * the reference tree).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - every function returns AKE_OK (0) or a negative error code; no C++ exception
 *     crosses the ABI; ake_last_error() returns a thread-local message;
 *   - "dev" pointers are device (HIP) pointers, "host" pointers are host memory;
 *   - compute entry points never allocate and never synchronise: the caller passes
 *     a workspace (size from the matching *_workspace_bytes) and a hipStream_t;
 *     they are safe to capture into a hipGraph;
 *   - one handle may be used from one stream at a time (the workspace is the
 *     per-call state; handles are immutable after creation / finalize);
 *   - all tensors are dense row-major float32, NCHW as in the reference; the *_pcm16_f32 entries take their AUDIO as 16-bit PCM
 *     (int16, sample s = s / 32768) and are float32 everywhere else.
 */
#ifndef AKE_HIP_H
#define AKE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AKE_OK 0
#define AKE_ERR_INVALID (-1)     /* bad argument / shape */
#define AKE_ERR_HIP (-2)         /* a HIP runtime call failed */
#define AKE_ERR_STATE (-3)       /* handle not finalized, tensor missing, ... */
#define AKE_ERR_WORKSPACE (-4)   /* workspace too small */
#define AKE_ERR_UNSUPPORTED (-5) /* architecture flag outside the default family */

typedef void* ake_stream_t; /* hipStream_t */

int ake_version(void);
const char* ake_last_error(void);
/* Always 0: there is one build, and it never looks at the environment, so nothing a process inherits can change results or precision.
 * (Kept for ABI compatibility: it once told a diagnostic build apart.) */
int ake_build_has_diag(void);

/* ------------------------------------------------------------------------------------------
 * CQT front end.  Replaces
 *     librosa.cqt(y, sr, hop_length=round(sr/frames), bins_per_octave=36, n_bins=36*octaves)
 *     -> torch.abs -> torch.log(1 + .)                 KeyDataset.py:485, 490-499
 * (also equivariance_test.py:161-169).  Definition: oracle/cqt_oracle.py (direct form);
 * evaluated here octave-recursively (half-band decimators + per-phase filter banks).
 * ---------------------------------------------------------------------------------------- */
typedef struct ake_cqt_plan ake_cqt_plan;

typedef struct ake_cqt_config {
    int sample_rate;      /* Hz, e.g. 22050 */
    int hop_length;       /* samples between frame centres; KeyDataset.py:485 */
    int n_bins;           /* 36 * octaves; KeyDataset.py:491 */
    int bins_per_octave;  /* 36 */
    double fmin;          /* Hz of bin 0; <=0 selects librosa's default C1 = 32.7032 Hz */
    int q_mode;           /* 0: Q = (r^2+1)/(r^2-1) (librosa >= 0.10); 1: Q = 1/(r-1) (<= 0.9) */
    int decim_half_len;   /* half length of the half-band decimator; <=0 selects 23 (47 taps) */
    double decim_beta;    /* Kaiser beta of the decimator; <=0 selects 8.0 */
    int engine;           /* 0: fastest available (3 where it applies); 1: one kernel per decimation stage + f32 filter bank (first version, kept
                             as the in-library cross-check); 2: fused decimator cascade + f32 bank (bit-identical to 1);
                             3: fused cascade writing split-bf16 level signals + bf16x3 MFMA bank (needs <= 8 octaves);
                             5 (opt-in): the half-band stages of levels 0-4 as Toeplitz products on bf16 MFMA with the clips as the N
                             dimension, chained through registers (cqt_stream.h), deeper levels and the bank as engine 3 (6-8 octaves,
                             47-tap decimator; measured level with engine 3 at 256 clips, so 0 never selects it).  4 was removed. */
} ake_cqt_config;

/* hop = round(sample_rate / frames_per_second) (KeyDataset.py:485), n_bins = 36 * octaves. */
int ake_cqt_default_config(ake_cqt_config* cfg, int sample_rate, int frames_per_second, int octaves);
/* Builds the filter tables in double precision on the host and uploads them to the current device. */
int ake_cqt_plan_create(const ake_cqt_config* cfg, ake_cqt_plan** out);
void ake_cqt_plan_destroy(ake_cqt_plan* plan);
int ake_cqt_plan_n_bins(const ake_cqt_plan* plan);
int ake_cqt_plan_hop(const ake_cqt_plan* plan);
/* 1 + n_samples / hop  (librosa center=True framing). */
int64_t ake_cqt_num_frames(const ake_cqt_plan* plan, int64_t n_samples);
/* The half-support H of the plan, in samples: frame t depends only on the samples [t * hop - H, t * hop + H].  A host-only query, an
 * upper bound from the plan's own tables: per level l, the filter bank's taps around the frame centre on the level's grid (uh, the
 * centre rounded down to the grid), through the l half-band stages below it (half_len taps to either side, each):
 *   H = max_l ( uh_l * 2^l + (2^l - 1) + half_len * (2^l - 1) )
 * -1 for a null plan.  A stream of audio uses it to tell which frames are final (KeyEstimator.stream). */
int64_t ake_cqt_plan_half_support(const ake_cqt_plan* plan);
/*
 * The workspace contract, for every entry point that takes (workspace, workspace_bytes) with the size its *_workspace_bytes returns:
 *   - the content of the workspace on entry is arbitrary (fresh memory, what a call of another shape or route left, NaN patterns): a call
 *     writes everything it later reads, so one buffer sized for the largest request serves every shape in turn;
 *   - a call writes nothing outside [workspace, workspace + workspace_bytes) and its documented outputs, and an output is written as exactly
 *     its documented bytes (no store is rounded up past a [batch][11] row);
 *   - the one exception: ake_pcnet_backward_f32 reads what ake_pcnet_forward_train_f32 left in the same workspace (documented there).
 */
size_t ake_cqt_workspace_bytes(const ake_cqt_plan* plan, int batch, int64_t n_samples);
/*
 * audio_dev : [batch][audio_stride] float32, first n_samples of each row are the clip
 * out_dev   : [batch][n_bins][out_frames] float32 = log(1 + |CQT|); frames >= num_frames are
 *             written as 0 (the zero padding KeyDataset.__getitem__ appends, KeyDataset.py:245)
 */
int ake_cqt_logmag_f32(const ake_cqt_plan* plan, const float* audio_dev, int batch, int64_t n_samples,
                       int64_t audio_stride, float* out_dev, int64_t out_frames, void* workspace,
                       size_t workspace_bytes, ake_stream_t stream);

/* Ragged batch (clips of different lengths in one call).  Row i holds n_samples_dev[i] <= n_max samples
 * (device array, int64); whatever follows them in the row is never read (hardware range checking returns 0, the transform's
 * zero padding).  Clip i gets 1 + n_samples[i] / hop frames; frames beyond them are written as 0, as KeyDataset.__getitem__
 * pads to the longest clip (KeyDataset.py:245).  Workspace as for (batch, n_max).  Engine 3 (the default up to 8 octaves). */
int ake_cqt_logmag_ragged_f32(const ake_cqt_plan* plan, const float* audio_dev, int batch, int64_t n_max,
                              int64_t audio_stride, const int64_t* n_samples_dev, float* out_dev, int64_t out_frames,
                              void* workspace, size_t workspace_bytes, ake_stream_t stream);

/* Per-clip hops (the reference's whole-song mode, --frames 0: hop_i = n_i / window_size + 1, KeyDataset.py:485-490).  Clip i has
 * n_i = n_clip_dev[i] samples (int64; null: every clip has n_max), hop hop_dev[i] (int32, device) and T_i = 1 + n_i / hop_i frames.
 * out_dev = [batch][n_bins][out_frames]: clip i's first min(T_i, out_frames) frames, then zeros.  The plan must be engine 3 with an odd
 * hop_length (hop_twos == 0: it holds a phase table for every phase; create it with hop_length = 1) -- engines 1, 2 and 5 give
 * AKE_ERR_UNSUPPORTED, an even hop AKE_ERR_INVALID.  Hops < 1 are the caller's contract: the results for such a clip are unspecified
 * (the kernels read them as 1 and stay in bounds).  Workspace from ake_cqt_workspace_bytes_hops, sized by out_frames (the frame counts
 * are only known on the device); no host synchronisation. */
size_t ake_cqt_workspace_bytes_hops(const ake_cqt_plan* plan, int batch, int64_t n_max, int64_t out_frames);
int ake_cqt_logmag_hops_f32(const ake_cqt_plan* plan, const float* audio_dev, int batch, int64_t n_max, int64_t audio_stride,
                            const int64_t* n_clip_dev, const int32_t* hop_dev, float* out_dev, int64_t out_frames, void* workspace,
                            size_t workspace_bytes, ake_stream_t stream);

/* Frames-major output: the same transform left as the filter bank writes it, out_dev = [batch][num_frames][n_bins] -- no transpose
 * pass (a 48 MB round trip per 256 clips).  For consumers that can read that order: ake_pcnet_forward_frames_major_f32, and
 * ake_pipeline_forward_f32 uses the pair internally.  Engine 3, equal-length clips (ake_cqt_frames_major_supported). */
int ake_cqt_frames_major_supported(const ake_cqt_plan* plan);
int ake_cqt_logmag_frames_major_f32(const ake_cqt_plan* plan, const float* audio_dev, int batch, int64_t n_samples,
                                    int64_t audio_stride, float* out_dev, void* workspace, size_t workspace_bytes,
                                    ake_stream_t stream);

/* 16-bit PCM audio (what decoders and WAV files deliver): sample s stands for float(s) * 2^-15, which is exact, so this entry gives the
 * results of the four float entries above on the converted audio, bit for bit, without a float32 copy of the audio being written.  One
 * entry for all four forms:
 *   n_clip_dev   null: every row holds n_max samples; else row i holds n_clip_dev[i] <= n_max (int64, device)  -- the ragged form
 *   hop_dev      null: the plan's hop; else per-clip hops (int32, device) as ake_cqt_logmag_hops_f32, same requirements on the plan
 *   frames_major != 0: out_dev = [batch][out_frames][n_bins] as ake_cqt_logmag_frames_major_f32 (n_clip_dev and hop_dev null, and
 *                out_frames == ake_cqt_num_frames); 0: out_dev = [batch][n_bins][out_frames], out_frames the padded frame count
 * Engine 3 only: engines 1, 2 and 5 give AKE_ERR_UNSUPPORTED.  audio_dev must be 4-byte aligned and audio_stride (in samples) even,
 * AKE_ERR_INVALID otherwise: the kernel loads whole 4-byte words.  Sample i < n_i of a row contributes its value and sample i >= n_i
 * exactly zero, whatever lies there; the kernel may read up to the end of the 4-byte word that holds a row's last sample (one sample
 * behind an odd n_i, inside the row's own stride), and no further.  Workspace: ake_cqt_workspace_bytes, or
 * ake_cqt_workspace_bytes_hops with hop_dev -- the existing *_workspace_bytes functions serve every PCM entry unchanged. */
int ake_cqt_logmag_pcm16_f32(const ake_cqt_plan* plan, const int16_t* audio_dev, int batch, int64_t n_max, int64_t audio_stride,
                             const int64_t* n_clip_dev, const int32_t* hop_dev, float* out_dev, int64_t out_frames, int frames_major,
                             void* workspace, size_t workspace_bytes, ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * PitchClassNet forward (inference: eval-mode BatchNorm folded into the convolutions).
 * Replaces  PitchClassNet.forward(mel, seq_length)   models.py:747-817
 * and everything it calls (models.py:22-106, 135-143, 168-243, 246-399).
 * ---------------------------------------------------------------------------------------- */
typedef struct ake_pcnet ake_pcnet;

typedef struct ake_pcnet_config {
    int pitches;        /* CQT bins = 36*octaves; models.py:653 */
    int pitch_classes;  /* 12 */
    int num_layers;     /* opt.num_layers, default 2 */
    int kernel_size;    /* opt.kernel_size, default 7; 3 and 5 are built too (every convolution then runs the generic kernels) */
    int conv_layers;    /* opt.conv_layers, default 3 */
    int n_filters;      /* opt.n_filters, default 4 */
    int head_layers;    /* opt.head_layers, default 2 */
    int time_pool_size; /* opt.time_pool_size, default 2 */
    int genre;          /* opt.genre: 1 adds the 11-way genre head */
    int max_pool;       /* opt.max_pool (models.py:766-797, sample-0 quirk kept) */
    /* Non-default architecture variants (models.py:108-133,145-166,456-648): only_semitones must be 0 (it does not run in the reference either),
     * ake_pcnet_create returns AKE_ERR_UNSUPPORTED otherwise. */
    int resblock;       /* opt.resblock (models.py:181-187, 218-224, 402-454): 1 builds the residual-block stacks (inference and training) */
    int denseblock;     /* opt.denseblock (models.py:188-189, 225-226, 456-648): 1 builds the DenseNet-style stacks (pre-activation BatchNorm applied on
                         * load, 1-wide bottlenecks, features concatenated in place); not combinable with the other variants; inference only */
    int stay_sixth;     /* opt.stay_sixth (models.py:322-323, 336, 366-367): 1 keeps the pitch stream at semitone resolution after layer 0 */
    int only_semitones;
    int p2pc_conv;      /* opt.p2pc_conv (models.py:108-133): 1 folds the octaves with a learned dilated conv + BN + LeakyReLU instead of the max */
    int pc2p_mem;       /* opt.pc2p_mem (models.py:145-166): 1 adds the summed up_sixth map to the pitch stream instead of concatenating */
    /* opt.local (sliding-window key tracking, models.py:720-722): 0 = off, else the heads' pooling window
     * W = opt.frames * opt.loc_window_size - head_layers * (kernel_size - 1).  The layers then do not pool over time
     * (models.py:348, 394: time_pool_size is ignored) and the forward is ake_pcnet_forward_local_f32.  Inference only. */
    int local;
    /* Arithmetic of the INFERENCE convolutions (training always uses f32-equivalent products).  Storage, accumulation and every
     * non-convolution op are f32 in both modes.
     *   AKE_PRECISION_MIXED (0, default): the 7x7 pitch convolutions, the semitone convolutions and layer 0's pitch-class stack multiply f16
     *       activations with f16 weights (per-channel power-of-two scaled), one MFMA product; the last layer's pitch-class stack and the heads
     *       use 3-term split-bf16 products.  Outputs within ~2e-5 of the float64 reference on seeded and on trained weights (budget 1e-3).
     *   AKE_PRECISION_F32X3 (1): no operand is rounded below 2^-17: exact-f32 MFMA / VALU kernels for the pitch, semitone and layer-0
     *       convolutions, 3-term split-bf16 products (hi*hi + lo*hi + hi*lo) for the pitch-class stack and the heads.  ~4x slower. */
    int precision;
} ake_pcnet_config;
#define AKE_PRECISION_MIXED 0
#define AKE_PRECISION_F32X3 1
/* the precision a handle runs its inference convolutions in (AKE_PRECISION_*) */
int ake_pcnet_precision(const ake_pcnet* net);

int ake_pcnet_default_config(ake_pcnet_config* cfg, int octaves, int genre);
int ake_pcnet_create(const ake_pcnet_config* cfg, ake_pcnet** out);
void ake_pcnet_destroy(ake_pcnet* net);

int ake_pcnet_pitches(const ake_pcnet* net);

/* The float entries of the reference state_dict this configuration expects
 * (models.py:993 / eval.py:115 strict=True): names and shapes, for host-side validation. */
int ake_pcnet_num_tensors(const ake_pcnet* net);
int ake_pcnet_tensor_info(const ake_pcnet* net, int index, const char** name, int64_t shape[4], int* ndim);
/* Hand one state_dict entry (host float32, reference layout) to the handle. */
int ake_pcnet_set_tensor(ake_pcnet* net, const char* name, const float* host_data, const int64_t* shape, int ndim);
/* All tensors set -> fold BatchNorm (running stats, eps 1e-5), repack for the kernels, upload. */
int ake_pcnet_finalize(ake_pcnet* net);
/* Device-resident parameters (training: models.py:1017-1027 updates the weights every optimizer step).  params_dev is
 * ONE flat float32 buffer holding every float entry of the state_dict at ake_pcnet_grad_offset(name)
 * (ake_pcnet_grad_floats() floats; valid right after ake_pcnet_create).  Rebuilds every packed weight -- eval-mode
 * BatchNorm folding included, bit-identical to set_tensor + finalize -- with two kernels on `stream`; replaces
 * set_tensor/finalize for callers whose weights live on the device.  The buffer is only read during the call. */
int ake_pcnet_load_from_device_f32(ake_pcnet* net, const float* params_dev, ake_stream_t stream);
/* The same, but only what the TRAINING-mode entry points read (ake_pcnet_forward_train_f32, ake_pcnet_backward_f32): the MFMA fragments of the
 * inference kernels are left stale (half of the repack launches of a training step) and inference calls return AKE_ERR_STATE until the
 * next ake_pcnet_load_from_device_f32.  models.py:1017-1027 updates the weights every optimizer step; eval happens once per epoch. */
int ake_pcnet_load_for_training_f32(ake_pcnet* net, const float* params_dev, ake_stream_t stream);
/* nn.BatchNorm2d's train-mode side effect, on the flat parameter buffer: running_mean/var <- (1-m)*running + m*(batch mean,
 * UNBIASED batch variance), from the bn_stats a training forward returned.  Reference default momentum 0.1. */
int ake_pcnet_update_running_stats_f32(const ake_pcnet* net, const float* bn_stats_dev, float* params_dev, float momentum,
                                       ake_stream_t stream);
/* --denseblock: the reference checkpoints norm1 + conv1 of every dense layer (torch.utils.checkpoint, models.py:484-489, 553), so autograd's
 * BACKWARD runs that half a second time in train mode and its BatchNorm blends the batch statistics into the running ones once more
 * (num_batches_tracked counts 2 per step for those layers).  Call this after ake_pcnet_backward_f32 with the bn_stats of the forward the
 * backward belonged to: it repeats the blend for exactly those layers.  *channels (nullable) receives how many BatchNorm channels that is;
 * a no-op (0 channels) for every other configuration. */
int ake_pcnet_update_recomputed_running_stats_f32(const ake_pcnet* net, const float* bn_stats_dev, float* params_dev, float momentum, int* channels,
                                                  ake_stream_t stream);

size_t ake_pcnet_workspace_bytes(const ake_pcnet* net, int batch, int frames);
/*
 * mel_dev        : [batch][1][pitches][frames] float32 (log-CQT, zero padded to `frames`)
 * seq_length_dev : [batch] int64 valid frames per clip, or NULL (models.py:786-797 branch)
 * key_out_dev    : [batch][12]  sigmoid pitch-class membership           (models.py:802)
 * tonic_out_dev  : [batch][12]  tonic logits                             (models.py:800)
 * genre_out_dev  : [batch][11]  genre logits, ignored unless cfg.genre   (models.py:804)
 */
int ake_pcnet_forward_f32(const ake_pcnet* net, const float* mel_dev, int batch, int frames,
                          const int64_t* seq_length_dev, float* key_out_dev, float* tonic_out_dev,
                          float* genre_out_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream);

/* --local forward (net created with cfg.local = W > 0; models.py:805-810).  Tm = frames - head_layers * (kernel_size - 1) map
 * frames, Tq = Tm - W + 1 pooled frames (ake_pcnet_local_frames).  Outputs, in the reference's memory order (it *reshapes*
 * [B][1][12][Tq] to (B, Tq, 12) -- same bytes):
 *   key_out_dev, tonic_out_dev : [batch][12 * Tq]   sliding max over W frames of the head maps; sigmoid on key
 *   genre_out_dev              : [batch][11 * Tm]   the genre head's map */
int ake_pcnet_local_frames(const ake_pcnet* net, int frames, int* pooled_frames, int* map_frames);
/* The forward with mel as ake_cqt_logmag_frames_major_f32 leaves it, [batch][frames][pitches]: the two kernels that read the CQT (layer 0
 * and the first pitch convolution) transpose while staging.  Only the default architecture on the fused inference path takes it:
 * ake_pcnet_accepts_frames_major(net, batch, frames) != 0; otherwise AKE_ERR_UNSUPPORTED.  Same results as ake_pcnet_forward_f32 on the
 * transposed tensor, bit for bit. */
int ake_pcnet_accepts_frames_major(const ake_pcnet* net, int batch, int frames);
int ake_pcnet_forward_frames_major_f32(const ake_pcnet* net, const float* mel_frames_major_dev, int batch, int frames,
                                       const int64_t* seq_length_dev, float* key_out_dev, float* tonic_out_dev, float* genre_out_dev,
                                       void* workspace, size_t workspace_bytes, ake_stream_t stream);

int ake_pcnet_forward_local_f32(const ake_pcnet* net, const float* mel_dev, int batch, int frames, float* key_out_dev,
                                float* tonic_out_dev, float* genre_out_dev, void* workspace, size_t workspace_bytes,
                                ake_stream_t stream);

/* Training-mode forward: BatchNorm uses the statistics of this batch (nn.BatchNorm2d in train(), as
 * equivariance_test.py:178 runs the net and as training_step does, models.py:952).  Convolutions keep their raw
 * outputs and per-channel sums; normalisation + LeakyReLU are applied by the next reader, never as a pass of their own.
 * bn_stats_out (optional, device): [sum of BN channels][3] = batch mean, biased batch variance, elements per channel, in
 * the layer order of ake_pcnet_bn_info -- what the caller needs for torch's running_mean / running_var update
 * (momentum 0.1, unbiased variance).  The whole batch is processed in one pass (no chunking).
 * A net created with local > 0 (--local, models.py:805-810) takes seq_length_dev = NULL and writes the per-frame outputs of
 * ake_pcnet_forward_local_f32: key / tonic (B, T', 12), genre (B, Tm, 11) with (T', Tm) from ake_pcnet_local_frames. */
int ake_pcnet_num_bn(const ake_pcnet* net);
int ake_pcnet_bn_info(const ake_pcnet* net, int index, const char** name, int* channels, int* channel_offset);
size_t ake_pcnet_train_workspace_bytes(const ake_pcnet* net, int batch, int frames);
int ake_pcnet_forward_train_f32(const ake_pcnet* net, const float* mel_dev, int batch, int frames,
                                const int64_t* seq_length_dev, float* key_out_dev, float* tonic_out_dev,
                                float* genre_out_dev, float* bn_stats_out_dev, void* workspace, size_t workspace_bytes,
                                ake_stream_t stream);

/* Backward pass of the training-mode forward (what autograd does for the reference's training_step, models.py:952-963).
 * Must follow ake_pcnet_forward_train_f32 on the same (mel, batch, frames, seq_length, workspace): the workspace holds the raw
 * convolution outputs and BatchNorm batch statistics it needs.  d_*_dev are dLoss/d(key_out, tonic_out, genre_out); key_out_dev
 * is the forward's key output (for the sigmoid derivative).  grads_out_dev receives dLoss/d(parameter) for every float entry of
 * the state_dict, flat, at ake_pcnet_grad_offset(name) (ake_pcnet_grad_floats() floats in total; running statistics get zeros).
 * accumulate != 0 adds to grads_out_dev instead of overwriting it (accumulate_grad_batches, train_model.py:118).
 * For a --local net d_* and key_out carry the per-frame shapes of the local forward (the sliding-window max routes each frame's
 * gradient to the first maximum of its window, as nn.MaxPool2d does).
 * Any num_layers; --resblock / --pc2p_mem / --p2pc_conv / --stay_sixth train too; --denseblock: AKE_ERR_UNSUPPORTED. */
size_t ake_pcnet_grad_floats(const ake_pcnet* net);
int64_t ake_pcnet_grad_offset(const ake_pcnet* net, const char* name);
int ake_pcnet_backward_f32(const ake_pcnet* net, const float* mel_dev, int batch, int frames, const int64_t* seq_length_dev,
                           const float* key_out_dev, const float* d_key_dev, const float* d_tonic_dev, const float* d_genre_dev,
                           float* grads_out_dev, int accumulate, void* workspace, size_t workspace_bytes, ake_stream_t stream);

/* Fused Adam over flat buffers, torch.optim.Adam semantics as the reference configures it (models.py:1017-1027:
 * betas (0.9, 0.999), eps 1e-8, weight_decay = --reg as L2 added to the gradient, bias correction with `step` = 1, 2, ...):
 *   g = grad * grad_scale + weight_decay * p;  m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g
 *   p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)
 * trainable_dev (nullable): one byte per element, 0 = leave untouched (running statistics inside the flat buffer).
 * grad_scale folds the 1/world_size of a summed all-reduce (and 1/accumulate_grad_batches if the caller did not scale the loss). */
int ake_adam_step_f32(float* params_dev, const float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev,
                      const unsigned char* trainable_dev, size_t count, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int step, float grad_scale, ake_stream_t stream);

/* Everything PitchClassNet.general_step computes behind the forward, in one launch (replaces models.py:826-905: label argmax / genre
 * mask, key_weight * BCE(key) + tonic_weight * CE(tonic) + genre_weight * CE(genre rows whose one-hot label sums to 1; dropped when there
 * is none) [+ 1 - mean cosine(key, key_labels) with use_cos], and models.py:1065-1116: the MIREX categories over the 21-row key-signature
 * table, utils/key_signatures.py:19-42).  One-hot label tensors are float32 or int64 (the *_i64 flags); genre_* nullable (--genre off).
 * scalars_out_dev[10] = loss, accuracy, mirex_score, correct, fifths, relative, parallel, other, accuracy_tonic, accuracy_genre
 * (general_step's return order).  d_*_dev (all or none): dloss/d(key_out | tonic_out | genre_out), what loss.backward() hands to
 * ake_pcnet_backward_f32. */
int ake_general_step_f32(const float* key_out_dev, const float* tonic_out_dev, const float* genre_out_dev, const float* key_labels_dev,
                         const void* tonic_labels_dev, int tonic_labels_i64, const void* genre_labels_dev, int genre_labels_i64,
                         const void* key_signature_id_dev, int key_signature_i64, int batch, float key_weight, float tonic_weight,
                         float genre_weight, int use_cos, float* scalars_out_dev, float* d_key_dev, float* d_tonic_dev, float* d_genre_dev,
                         ake_stream_t stream);
/* The same with a weight per row: sample_weight_dev [batch] float32, values >= 0 (anything else counts as 0), nullable.  NULL runs
 * ake_general_step_f32's arithmetic, bit for bit.  Otherwise, with w_i the weights, Wsum = sum_i w_i and m_i the genre mask:
 *   loss = key_weight * sum_i w_i sum_j BCE_ij / (12 Wsum) + tonic_weight * sum_i w_i CE_i / Wsum
 *          + genre_weight * sum_i w_i m_i CE_i / sum_i w_i m_i   (an exact 0 when that denominator is 0)
 *          [+ 1 - sum_i w_i cos_i / Wsum with use_cos]
 * the nine metrics are the same weighted means (`other` = 1 - the four categories; accuracy_genre over sum_i w_i m_i), and d_*_dev the
 * derivatives of exactly this loss.  A row with w_i = 0 is not read: it contributes exact zeros to the loss, the metrics and its own
 * gradient rows, whatever its outputs and labels hold.  Wsum = 0: all ten scalars and all gradients are exact zeros.  One launch, double
 * sums in a fixed-order tree, no atomics: bit-reproducible.  Under data-parallel training every rank normalises by its own Wsum. */
int ake_general_step_weighted_f32(const float* key_out_dev, const float* tonic_out_dev, const float* genre_out_dev, const float* key_labels_dev,
                                  const void* tonic_labels_dev, int tonic_labels_i64, const void* genre_labels_dev, int genre_labels_i64,
                                  const void* key_signature_id_dev, int key_signature_i64, int batch, float key_weight, float tonic_weight,
                                  float genre_weight, int use_cos, const float* sample_weight_dev, float* scalars_out_dev, float* d_key_dev,
                                  float* d_tonic_dev, float* d_genre_dev, ake_stream_t stream);

/* general_step of a --local net (models.py:861-876, 898-909): per-frame outputs key_out (after the sigmoid) and tonic_out (logits),
 * [batch][out_frames][12] as the forward returns them; labels with their own row count, key_labels [batch][label_frames][12] float32,
 * tonic_labels [batch][label_frames][12] and key_signature_id [batch][label_frames][24] one-hot, float32 or int64 (the *_i64 flags;
 * float tonic labels are truncated as .long() does, key-signature labels are not).  valid_frames_dev[batch] (int32, on the device):
 * n_i = seq_length_i - loc_window_size * frames + 1, the rows of clip i that are scored; the contract is 3 <= n_i <= min(out_frames,
 * label_frames), and values outside [0, min(out_frames, label_frames)] are read clamped to it (results unspecified, reads in bounds).
 * scalars_out_dev[10], general_step's order: loss = key_weight * mean_i BCE_i + tonic_weight * mean_i CE_i (BCE_i over the clip's
 * n_i * 12 elements, CE_i over its n_i frames); accuracy, mirex_score, correct, fifths, relative, parallel, other: each clip's MIREX
 * categories over its n_i frames / n_i (the table match of ake_general_step_f32), mean over the clips; accuracy_tonic: per clip over
 * its first n_i - 2 frames (the reference's seq_length - (span + 1)), mean over the clips (a clip with n_i <= 2 adds 0); 0.
 * d_key_dev / d_tonic_dev (both or none) [batch][out_frames][12]: dloss/d(key_out | tonic_out), rows t >= n_i exact zeros.
 * Two launches (per-chunk partial sums in the workspace, then a fixed-order reduction): bit-reproducible.  Workspace from
 * ake_general_step_local_workspace_bytes(batch, out_frames) (0 for batch < 1 or out_frames < 1). */
size_t ake_general_step_local_workspace_bytes(int batch, int out_frames);
int ake_general_step_local_f32(const float* key_out_dev, const float* tonic_out_dev, const float* key_labels_dev, const void* tonic_labels_dev,
                               int tonic_labels_i64, const void* key_signature_id_dev, int key_signature_i64, const int* valid_frames_dev,
                               int batch, int out_frames, int label_frames, float key_weight, float tonic_weight, float* scalars_out_dev,
                               float* d_key_dev, float* d_tonic_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream);

/* Debug tap: copy an intermediate activation of the LAST forward call out of the workspace.
 * name is the reference module path whose output it is (e.g. "model.1.p2p.layer.8").
 * After ake_pcnet_forward_train_f32 (and before the backward pass) "train:<buffer>" names buffers of the training workspace; for every
 * BatchNorm of the default architecture family, by state_dict prefix: "train:raw/<bn prefix>" = the raw convolution output it normalises,
 * [batch][C][H][T], and "train:aff/<bn prefix>" = its [C][3] (scale, shift, negative slope) table, shape {C, 3, 1, 1} -- the pair the
 * backward kernels re-derive every LeakyReLU sign and max-pool winner from.  Other architectures: AKE_ERR_INVALID. */
int ake_pcnet_tap_info(const ake_pcnet* net, const char* name, int batch, int frames, int64_t shape[4]);
/* Inference fuses the semitone conv into the last pitch conv of a stack and runs the last layer's pitch-class stack as one
 * launch, so "model.i.p2p.layer.8" and the last layer's "pc2pc.layer.{2,5,8}" are never written (tap_info says so).
 * ake_debug_keep_taps(1) (process-wide, before the forward) keeps every nameable activation in memory (slower); returns the old value. */
int ake_debug_keep_taps(int on);
int ake_pcnet_tap_copy(const ake_pcnet* net, const char* name, int batch, int frames, const void* workspace,
                       float* out_dev, ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Audio preparation in front of the CQT (not in the reference, which takes channel 0 at the file's own
 * rate: KeyDataset.py:479-485 -- channel = 0 and rate_in == rate_out reproduce exactly that): channel selection or mono
 * mix-down and polyphase resampling = scipy.signal.resample_poly(x, up, down) with its default Kaiser(5.0) filter, on the
 * device, for ragged batches.
 * in_dev[clip * clip_stride + c * channel_stride + i]; channel >= 0 selects one channel, -1 takes the mean of all;
 * n_in_clip_dev (or null): samples of each clip (<= n_in); out_dev[clip * out_stride + k], k < ake_resampler_out_len(n_in),
 * zero behind a shorter clip; n_out_clip_dev (or null) receives every clip's output length ceil(n * up / down).
 * ---------------------------------------------------------------------------------------- */
typedef struct ake_resampler ake_resampler;
int ake_resampler_create(int rate_in, int rate_out, ake_resampler** out);
void ake_resampler_destroy(ake_resampler* r);
int64_t ake_resampler_out_len(const ake_resampler* r, int64_t n_in);
int ake_resample_f32(const ake_resampler* r, const float* in_dev, int batch, int channels, int64_t n_in, int64_t clip_stride,
                     int64_t channel_stride, int channel, const int64_t* n_in_clip_dev, float* out_dev, int64_t out_stride,
                     int64_t* n_out_clip_dev, ake_stream_t stream);
/* The same from 16-bit PCM (sample s = s / 32768), read in place at in_dev[clip * clip_stride + c * channel_stride + i * sample_stride]
 * (strides in samples): planar (B, C, n) storage has sample_stride 1, interleaved (B, n, C) storage -- what decoders hand over -- has
 * channel_stride 1 and sample_stride C.  Output float32 mono, bit-identical to ake_resample_f32 on the converted planar audio. */
int ake_resample_pcm16_f32(const ake_resampler* r, const int16_t* in_dev, int batch, int channels, int64_t n_in, int64_t clip_stride,
                           int64_t channel_stride, int64_t sample_stride, int channel, const int64_t* n_in_clip_dev, float* out_dev,
                           int64_t out_stride, int64_t* n_out_clip_dev, ake_stream_t stream);

/* The same resampler on audio that arrives in chunks, all recordings in lockstep (KeyEstimator.stream(source_rate=...),
 * ake_amd.StreamResampler; host model metrics.stream_resample).  Output k depends on the inputs ceil((k down - half) / up) ..
 * floor((k down + half) / up), so it is final once the latter has arrived:
 *   ake_stream_resample_out_count(r, n_in, flush) (host only; -1 for a null r or a negative n_in) = the outputs that are final after n_in
 *   inputs: without flush 0 if n_in up - half - 1 < 0, else (n_in up - half - 1) / down + 1; with flush ceil(n_in up / down) =
 *   ake_resampler_out_len (the rest see nothing behind the end, as the offline outputs do); with up == down, n_in.
 * A call takes the next m samples of every recording, chunk_dev[rec * rec_stride + c * channel_stride + i (* sample_stride)], after the
 * n_before it has been given so far, and writes the outputs k in [out_count(n_before, 0), out_count(n_before + m, flush)) to
 * out_dev[rec * out_stride + (k - first)]; *k_out (a host integer, required) is their number, computed on the host; out_dev behind it
 * is not touched.  The outputs equal ake_resample_f32 / ake_resample_pcm16_f32 on the concatenated audio BIT FOR BIT, however the audio
 * is cut into calls: the same order of channel additions, the same ascending fmaf chain from the same first input (never below 0; under
 * flush never beyond the last), the 1 / channels scale last, the 16-bit form converting float(s) * 2^-15 where the offline one does.
 * channel >= 0 takes that channel, -1 the mean.  m = 0 is allowed (with flush: flush only); m may be shorter than the filter.
 * state_dev: ake_stream_resample_state_bytes(r, recordings) bytes (0 for a null r or recordings outside 1..65535), 16-byte aligned: per
 * recording a ring of the last 2 half / up + 1 (rounded up to a multiple of 4) inputs as float32, input i at slot i % ring, channels
 * summed and not yet scaled -- the same values from float32 and 16-bit chunks.  With n_before == 0 it is not read, so a fresh stream needs
 * no initialising launch; up == down (a channel pick or mix alone) never touches it.  The device keeps no count: the host passes n_before.
 * Launches: stream_resample_kernel (512 outputs a workgroup, the tile's input mixed once into LDS; reads the ring), then
 * stream_resample_tail_kernel (writes the ring from the chunk's end) -- two, so that no workgroup reads what another writes.  A call with
 * no output skips the first, m == 0 or up == down the second; a call with neither launches nothing.  Plain loads and stores, no atomics.
 * AKE_ERR_INVALID: a null r, state_dev or k_out, chunk_dev with m > 0, out_dev with *k_out > 0; recordings outside 1..65535; channels < 1;
 * channel outside -1..channels-1; m or n_before negative; rec_stride or channel_stride negative, sample_stride < 1, out_stride < *k_out;
 * a misaligned state.  AKE_ERR_WORKSPACE: state_bytes below the query.  AKE_ERR_UNSUPPORTED: a ratio down / up so large (beyond about 30)
 * that a tile's input exceeds 64 KiB of LDS.  Nothing is launched after any of them. */
int64_t ake_stream_resample_out_count(const ake_resampler* r, int64_t n_in, int flush);
size_t ake_stream_resample_state_bytes(const ake_resampler* r, int recordings);
int ake_stream_resample_f32(const ake_resampler* r, const float* chunk_dev, int recordings, int channels, int64_t m, int64_t rec_stride,
                            int64_t channel_stride, int channel, int64_t n_before, int flush, void* state_dev, size_t state_bytes,
                            float* out_dev, int64_t out_stride, int64_t* k_out, ake_stream_t stream);
int ake_stream_resample_pcm16_f32(const ake_resampler* r, const int16_t* chunk_dev, int recordings, int channels, int64_t m, int64_t rec_stride,
                                  int64_t channel_stride, int64_t sample_stride, int channel, int64_t n_before, int flush, void* state_dev,
                                  size_t state_bytes, float* out_dev, int64_t out_stride, int64_t* k_out, ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Whole hot path for a batch of equal-length clips: CQT then forward
 * (DatasetLoader.get_all -> __getitem__ -> general_step's forward; KeyDataset.py:469-509,
 * 242-256, models.py:846).  seq_length of every clip = num_frames(n_samples).
 * ---------------------------------------------------------------------------------------- */
size_t ake_pipeline_workspace_bytes(const ake_cqt_plan* plan, const ake_pcnet* net, int batch, int64_t n_samples);
int ake_pipeline_forward_f32(const ake_cqt_plan* plan, const ake_pcnet* net, const float* audio_dev, int batch,
                             int64_t n_samples, int64_t audio_stride, float* key_out_dev, float* tonic_out_dev,
                             float* genre_out_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream);
/* The same for a ragged batch (ake_cqt_logmag_ragged_f32): seq_length of clip i = 1 + n_samples[i] / hop, computed on the
 * device; workspace as ake_pipeline_workspace_bytes(plan, net, batch, n_max). */
int ake_pipeline_forward_ragged_f32(const ake_cqt_plan* plan, const ake_pcnet* net, const float* audio_dev, int batch,
                                    int64_t n_max, int64_t audio_stride, const int64_t* n_samples_dev, float* key_out_dev,
                                    float* tonic_out_dev, float* genre_out_dev, void* workspace, size_t workspace_bytes,
                                    ake_stream_t stream);
/* Both of the above from 16-bit PCM audio (ake_cqt_logmag_pcm16_f32: alignment, engine 3): n_samples_dev null = equal-length clips of
 * n_max samples.  The frames-major route is chosen exactly where ake_pipeline_forward_f32 chooses it; same outputs as the float entries on
 * the converted audio, bit for bit.  Workspace: ake_pipeline_workspace_bytes(plan, net, batch, n_max). */
int ake_pipeline_forward_pcm16_f32(const ake_cqt_plan* plan, const ake_pcnet* net, const int16_t* audio_dev, int batch, int64_t n_max,
                                   int64_t audio_stride, const int64_t* n_samples_dev, float* key_out_dev, float* tonic_out_dev,
                                   float* genre_out_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Key tracking over a long recording (not in the reference, whose --local nets return rows that are not time frames, models.py:806-807):
 * ONE CQT per recording, the clip-level net on sliding windows of its frames, and a decode of every window to a key label.
 *   - A recording of n samples is transformed once at the plan's hop: T = 1 + n / hop frames (ake_cqt_num_frames).
 *   - Window w is frames [w * stride_frames, w * stride_frames + window_frames) of the recording's own transform.  The net runs on it
 *     exactly as on a clip of window_frames frames with seq_length = window_frames; time-circular convolutions wrap at the window's ends.
 *   - Recording i has count_i = (T_i - window_frames) / stride_frames + 1 windows, 0 if T_i < window_frames.
 *   - The one difference from cutting the audio into clips and transforming each: a frame near a window edge sees the recording's real
 *     neighbouring audio where a separately transformed clip sees zero padding.  Intended.
 * A --local net is refused (AKE_ERR_UNSUPPORTED): it has its own per-frame forward, and its rows are not time frames.
 * ---------------------------------------------------------------------------------------- */
/* The net on every window of `recordings` equally long transforms.  mel_dev: [recordings][total_frames][pitches] (frames_major != 0, as
 * ake_cqt_logmag_frames_major_f32 leaves it) or [recordings][pitches][total_frames].  Outputs [recordings][windows][12 | 12 | 11] with
 * windows = (total_frames - window_frames) / stride_frames + 1 (total_frames >= window_frames).  The windows are gathered into the
 * [B][1][pitches][window_frames] tensor of ake_pcnet_forward_f32 and run 256 at a time, which is what the workspace query sizes: any
 * architecture variant and precision runs, with the results of ake_pcnet_forward_f32 on the materialised windows, bit for bit. */
size_t ake_pcnet_forward_windows_workspace_bytes(const ake_pcnet* net, int recordings, int total_frames, int window_frames, int stride_frames);
int ake_pcnet_forward_windows_f32(const ake_pcnet* net, const float* mel_dev, int frames_major, int recordings, int total_frames,
                                  int window_frames, int stride_frames, float* key_out_dev, float* tonic_out_dev, float* genre_out_dev,
                                  void* workspace, size_t workspace_bytes, ake_stream_t stream);
/* (key, tonic) rows -> key labels, one launch.  key_dev [rows][12] sigmoid outputs, tonic_dev [rows][12] logits.  Per row:
 *   sig_dev        0..20: first-maximum cosine match of the key row over the 21-row key-signature table (utils/key_signatures.py:19-42),
 *                  the arithmetic and tie rule of PitchClassNet.mirex_score (models.py:1065-1083; norms clamped at 1e-8), in float32;
 *   tonic_id_dev   0..11: first maximum of the tonic logits;
 *   confidence_dev that maximum cosine;
 *   key_id_dev     the project's 24-way label (0-11 minor, 12-23 major, tonic = id mod 12; KeyDataset.py:524-527): 12 + tonic if tonic
 *                  is the major tonic of table row sig, tonic if it is that tonic + 9 mod 12 (the relative minor), else -1
 *                  (signature and tonic disagree).
 * counts_dev (nullable, int32 [rows / windows_per_recording]): row r is window r % windows_per_recording of recording
 * r / windows_per_recording; windows at index >= the recording's count get key_id = sig = tonic_id = -1 and confidence 0. */
int ake_decode_keys_f32(const float* key_dev, const float* tonic_dev, int rows, const int32_t* counts_dev, int windows_per_recording,
                        int32_t* key_id_dev, int32_t* sig_dev, int32_t* tonic_id_dev, float* confidence_dev, ake_stream_t stream);
/* Waveforms -> track, on one stream with no host round trip: the CQT of the whole recordings (frames-major where the plan can), the
 * windows forward, the decode.  With W = (T - window_frames) / stride_frames + 1 and T = ake_cqt_num_frames(n_samples) >= window_frames:
 * key / tonic / genre outputs [recordings][W][12 | 12 | 11], key_id / sig / tonic_id (int32) and confidence [recordings][W],
 * counts_dev (int32) [recordings].  The ragged form takes row i's length n_samples_dev[i] <= n_max (int64, device) as
 * ake_pipeline_forward_ragged_f32 does and derives count_i on the device; windows at index >= count_i decode to -1 (their key / tonic
 * / genre rows are the net's outputs on frames that are partly the zero padding behind the recording's end). */
size_t ake_pipeline_track_workspace_bytes(const ake_cqt_plan* plan, const ake_pcnet* net, int recordings, int64_t n_samples, int window_frames,
                                          int stride_frames);
int ake_pipeline_track_f32(const ake_cqt_plan* plan, const ake_pcnet* net, const float* audio_dev, int recordings, int64_t n_samples,
                           int64_t audio_stride, int window_frames, int stride_frames, float* key_out_dev, float* tonic_out_dev,
                           float* genre_out_dev, int32_t* key_id_dev, int32_t* sig_dev, int32_t* tonic_id_dev, float* confidence_dev,
                           int32_t* counts_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream);
int ake_pipeline_track_ragged_f32(const ake_cqt_plan* plan, const ake_pcnet* net, const float* audio_dev, int recordings, int64_t n_max,
                                  int64_t audio_stride, const int64_t* n_samples_dev, int window_frames, int stride_frames, float* key_out_dev,
                                  float* tonic_out_dev, float* genre_out_dev, int32_t* key_id_dev, int32_t* sig_dev, int32_t* tonic_id_dev,
                                  float* confidence_dev, int32_t* counts_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream);
/* Both from 16-bit PCM recordings (ake_cqt_logmag_pcm16_f32: alignment, engine 3): lengths_dev null = ake_pipeline_track_f32, else
 * ake_pipeline_track_ragged_f32; same route, same outputs.  Workspace: ake_pipeline_track_workspace_bytes. */
int ake_pipeline_track_pcm16_f32(const ake_cqt_plan* plan, const ake_pcnet* net, const int16_t* audio_dev, int recordings, int64_t n_max,
                                 int64_t audio_stride, const int64_t* lengths_dev, int window_frames, int stride_frames, float* key_out_dev,
                                 float* tonic_out_dev, float* genre_out_dev, int32_t* key_id_dev, int32_t* sig_dev, int32_t* tonic_id_dev,
                                 float* confidence_dev, int32_t* counts_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A smooth key track: per-window log-scores of the 24 keys from the two heads, then a first-order Viterbi decode over them.  Both run on
 * the outputs of ake_pipeline_track*_f32 (same stream, right after it), which keep their signatures and results.  Every decoded window
 * holds a key 0..23: a tonic that does not fit the signature scores low instead of decoding to -1.
 * ---------------------------------------------------------------------------------------- */
/* emis_dev [rows][24] in the 24-way label order (0-11 minor, 12-23 major, tonic t_k = k mod 12).  With p = key_dev[row] (the sigmoid
 * memberships, trained with BCE) and tonic_dev[row] the logits (trained with cross-entropy):
 *   maj(k) = k - 12 if k >= 12, else (k + 3) mod 12;   S_k[j] = 1 if (j - maj(k)) mod 12 is in {0,2,4,5,7,9,11}, else 0
 *   e[row][k] = log_softmax(tonic)[t_k] + signature_weight / 12 * sum_j ( S_k[j] * max(log p_j, -100) + (1 - S_k[j]) * max(log1p(-p_j), -100) )
 * (the -100 clamp is nn.BCELoss's).  counts_dev / windows_per_recording as in ake_decode_keys_f32: rows behind a recording's count are
 * written as 0.  The three buffers are 16-byte aligned (rows move as 16-byte pieces). */
int ake_key_emissions_f32(const float* key_dev, const float* tonic_dev, int rows, const int32_t* counts_dev, int windows_per_recording,
                          float signature_weight, float* emis_dev, ake_stream_t stream);
/* Viterbi over emis_dev [recordings][windows][24], one wave per recording.  log_trans_dev [24][24]: log-probability of moving from key i
 * (row) to key j; log_prior_dev [24], NULL = zeros; counts_dev (int32 [recordings], NULL = every recording has `windows`), clamped to
 * 0..windows.  In float32, additions, subtractions and comparisons only (no product, so nothing to contract), so that a host
 * restatement (metrics.viterbi_keys) is bit-identical:
 *   d_0[j] = prior[j] + e[0][j]
 *   m[j]   = max_i ( d_{w-1}[i] + A[i][j] ),  bp_w[j] = the smallest i that attains it,   d_w[j] = m[j] + e[w][j]
 *   then d_w[j] -= max_j d_w[j]   at every step, w = 0 included (the scores stay bounded for any number of windows)
 * The last state is the smallest j attaining max d; the path follows bp backwards.  path_dev (int32 [recordings][windows]) holds -1 at
 * w >= count; a recording of count 0 holds only -1.  All of A, the prior and the emissions must be finite: write a forbidden
 * transition as a large negative number, not as -infinity (max - max would be NaN).
 * The workspace holds the back-pointers, one byte per state and window.  The backtrace stages them through LDS
 * ake_viterbi_chunk_windows() windows at a time. */
size_t ake_viterbi_keys_workspace_bytes(int recordings, int windows);
int ake_viterbi_chunk_windows(void);
int ake_viterbi_keys_f32(const float* emis_dev, int recordings, int windows, const int32_t* counts_dev, const float* log_trans_dev,
                         const float* log_prior_dev, int32_t* path_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream);

/* Posterior key probabilities: the forward-backward pass over the same emis_dev [recordings][windows][24], with log_trans_dev,
 * log_prior_dev and counts_dev as ake_viterbi_keys_f32 takes them (all finite; counts clamped to 0..windows).  For a recording of
 * n = count windows, in float32 and the log domain (LSE = log-sum-exp, taken about its largest term):
 *   a_0[j] = prior[j] + e[0][j]
 *   a_w[j] = e[w][j] + LSE_i ( a_{w-1}[i] + A[i][j] )                     w = 1..n-1
 *   c_w = LSE_j a_w[j];  a_w[j] -= c_w                                    every step, w = 0 included
 *   b_{n-1}[i] = 0
 *   b_w[i] = LSE_j ( A[i][j] + e[w+1][j] + b_{w+1}[j] );  then b_w[i] -= LSE_i b_w[i]
 *   post_w[j]  = softmax_j ( a_w[j] + b_w[j] )                                                   w = 0..n-1
 *   xi_w[i][j] = softmax over all 576 (i, j) of ( a_{w-1}[i] + A[i][j] + e[w][j] + b_w[j] )      w = 1..n-1
 *   loglik = sum_w c_w;   xi_sum[i][j] = sum_{w=1..n-1} xi_w[i][j]   (expected transition counts; they add up to n - 1)
 * The log domain stays finite for everything the Viterbi kernel accepts (forbidden transitions written as -1e4, emissions near -240).
 * Outputs: post_dev [recordings][windows][24], probabilities: every row below the count sums to 1, rows at or behind it are zeros;
 * loglik_dev [recordings], 0 for a count of 0; xi_sum_dev [recordings][24][24], nullable, zeros for counts 0 and 1; path_post_dev
 * [recordings][windows], nullable: post[r][w][path_dev[r][w]] for path_dev (int32 [recordings][windows], the Viterbi path), 0 where the
 * path holds -1 -- path_post_dev without path_dev is AKE_ERR_INVALID.  The emissions are log-scores, not normalised likelihoods, so
 * loglik is a log-score of the recording under A (the quantity an EM fit of A raises), not a likelihood of the audio.
 * Launches: the two serial chains side by side (one wave per recording and direction), then one kernel over (recording, window); with
 * xi_sum_dev a third adds the per-chunk transition sums (ake_key_posteriors_chunk_windows() windows each) in chunk order.  No atomics:
 * two runs on the same inputs are bit-identical.  The workspace holds a, b and the per-chunk sums; it and post_dev are 16-byte
 * aligned. */
size_t ake_key_posteriors_workspace_bytes(int recordings, int windows);
int ake_key_posteriors_chunk_windows(void);
int ake_key_posteriors_f32(const float* emis_dev, int recordings, int windows, const int32_t* counts_dev, const float* log_trans_dev,
                           const float* log_prior_dev, const int32_t* path_dev, float* post_dev, float* loglik_dev, float* xi_sum_dev,
                           float* path_post_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream);

/* The smoother with carried state, for audio that arrives in pieces: the k new windows emis_dev [recordings][k][24] of a stream that has
 * seen windows_before windows so far, one wave per recording.  log_trans_dev and log_prior_dev as ake_viterbi_keys_f32 takes them, all
 * finite.  Every new window w runs
 *   - ake_viterbi_keys_f32's step, operation for operation (d_w, bp_w; the same tie rules), and
 *   - ake_key_posteriors_f32's forward step (a_w, normalised by c_w at every step, w = 0 included);
 * filtered_dev [recordings][k][24] (nullable) = a_w: exp of it is the probability of each key given the windows up to w.
 * The fixed-lag path: after the step of window w >= lag the kernel follows `lag` back-pointers from the smallest j attaining max d_w and
 * writes the label of window w - lag, which is what ake_viterbi_keys_f32 on windows 0..w gives for it.  flush != 0 (the recording ends
 * here): after the last step the windows still inside the lag, min(lag, windows_before + k) of them, are written from the last best
 * state, so they hold the Viterbi path of the whole recording.  path_dev is int32 [recordings][*k_out], the windows from
 * max(0, windows_before - lag) on, in order; *k_out (a host integer, required) is computed on the host:
 *   (flush ? windows_before + k : max(0, windows_before + k - lag)) - max(0, windows_before - lag)
 * k = 0 is allowed (with flush: flush only); a call with nothing to step and nothing to write launches nothing.
 * state_dev holds, per recording, d[24], a[24] and a ring of the last `lag` back-pointer rows (24 bytes a window):
 * ake_key_stream_state_bytes(recordings, lag) bytes (0 for a bad shape), 16-byte aligned.  It is read once in front of the first step and
 * written once behind the last; with windows_before == 0 it is not read, so a fresh stream needs no initialising launch.  The device
 * keeps no count: the host passes windows_before, and the same lag at every call of a stream.  Results do not depend on how a
 * stream's windows are cut into calls, to the bit.
 * AKE_ERR_INVALID: lag outside 0..255, k < 0, recordings < 1, windows_before < 0, a null required pointer (log_trans_dev, state_dev,
 * k_out; emis_dev with k > 0; path_dev with *k_out > 0), a misaligned state.  AKE_ERR_WORKSPACE: state_bytes below the query. */
size_t ake_key_stream_state_bytes(int recordings, int lag);
int ake_key_stream_step_f32(const float* emis_dev, int recordings, int k, int64_t windows_before, int lag, int flush,
                            const float* log_trans_dev, const float* log_prior_dev, void* state_dev, size_t state_bytes,
                            float* filtered_dev, int32_t* path_dev, int* k_out, ake_stream_t stream);

/* Fixed-lag posteriors and a running log-likelihood beside the step above: called right after it, on the same stream, with the same
 * recordings, k, windows_before, lag and flush, on the same emis_dev and on the filtered_dev [recordings][k][24] the step wrote (both
 * required with k > 0).  With a_u the filtered rows and c_u what their steps subtracted, window v with end window s runs
 *   b_s[i] = 0
 *   b_u[i] = LSE_j ( A[i][j] + e[u+1][j] + b_{u+1}[j] );  then b_u[i] -= LSE_i b_u[i]          u = s-1 .. v
 *   post_v[j] = softmax_j ( a_v[j] + b_v[j] )
 * in float32 and the log domain, as ake_key_posteriors_f32's backward chain (finite for what that accepts).  Window v is written once
 * window s = v + lag has been stepped, so post_v is what ake_key_posteriors_f32 on windows 0..v + lag gives for it: the posterior given
 * the evidence the step's label of v was decided on.  flush != 0: the windows still inside the lag end at the stream's last window and
 * hold the posteriors of the whole recording.  lag 0: post = softmax(filtered).  The written windows are the step's: post_dev is
 * [recordings][*k_out][24] and *k_out (a host integer, required) the step's formula.  path_dev int32 [recordings][*k_out] (nullable):
 * the step's path_dev of the same call; path_post_dev [recordings][*k_out] (nullable) = post[r][v][path[r][v]], 0 where the path holds
 * -1 -- path_post_dev without path_dev is AKE_ERR_INVALID.  loglik_dev [recordings][k] (nullable): the sum of c_u up to each new
 * window, what ake_key_posteriors_f32 gives as loglik on windows 0..w; the sum is carried in a double and rounded on the way out.
 * state_dev holds, per recording, that double (in a 16-byte piece), then the last `lag` rows of e and the last `lag` rows of a, row
 * w % lag for window w (one row each for lag 0): ake_key_stream_posteriors_state_bytes(recordings, lag) bytes (0 for a bad shape),
 * 16-byte aligned.  With windows_before == 0 it is not read, and written whole.  The device keeps no count.
 * Launches: key_stream_sweep_kernel, one wave per (recording, written window), each running its <= lag backward steps on rows that
 * exist before the launch (from the call's inputs or the state, which it only reads); then key_stream_loglik_kernel, one wave per
 * recording, which recomputes c_w by the step's own forward step from a_{w-1} and e_w, adds them in window order, and moves the new
 * rows into the state.  *k_out == 0 skips the first, k == 0 the second (the state stands); a call with neither launches nothing.
 * No atomics: reruns are bit-identical, and results do not depend on how a stream's windows are cut into calls, to the bit.
 * AKE_ERR_INVALID and AKE_ERR_WORKSPACE as the step entry's (filtered_dev as emis_dev, post_dev as its path_dev). */
size_t ake_key_stream_posteriors_state_bytes(int recordings, int lag);
int ake_key_stream_posteriors_f32(const float* emis_dev, const float* filtered_dev, int recordings, int k, int64_t windows_before,
                                  int lag, int flush, const float* log_trans_dev, const float* log_prior_dev, const int32_t* path_dev,
                                  void* state_dev, size_t state_bytes, float* post_dev, float* path_post_dev, float* loglik_dev,
                                  int* k_out, ake_stream_t stream);

/* The front end of a stream of audio in lockstep (csrc/stream.hip), both in one launch each, plain loads and stores, no atomics.
 * ake_stream_history_*: the audio history [recordings][history_stride] float32 moves `drop` samples to the front -- `keep` samples
 * survive, history[r][i] = history[r][i + drop] for i < keep -- and the m new samples of chunk_dev [recordings][chunk_stride] follow
 * them at history[r][keep + i]; _pcm16: the chunk is 16-bit PCM, converted as float(s) * 2^-15 (exact).  The move is ordered (a row is
 * one workgroup's, tile by tile towards the back), so source and destination may overlap.  keep + m <= history_stride and
 * drop + keep <= history_stride, AKE_ERR_INVALID otherwise; keep = 0 or m = 0 are allowed.
 * ake_stream_frames_f32: the frame cache.  dst_dev receives keep frames of old_dev from frame `drop` on, then n_new frames of mel_dev
 * (a transform's output of mel_frames frames) from frame `first` on; frames_major != 0: all three are [recordings][frames][pitches]
 * with pitches a multiple of 4 and 16-byte aligned buffers, else [recordings][pitches][frames].  old_dev holds old_frames frames and
 * dst_dev keep + n_new; dst_dev overlaps neither source.  AKE_ERR_INVALID for ranges outside their tensors. */
int ake_stream_history_f32(float* history_dev, int recordings, int64_t history_stride, int64_t drop, int64_t keep, const float* chunk_dev,
                           int64_t chunk_stride, int64_t m, ake_stream_t stream);
int ake_stream_history_pcm16(float* history_dev, int recordings, int64_t history_stride, int64_t drop, int64_t keep,
                             const int16_t* chunk_dev, int64_t chunk_stride, int64_t m, ake_stream_t stream);
int ake_stream_frames_f32(float* dst_dev, const float* old_dev, const float* mel_dev, int frames_major, int recordings, int pitches,
                          int old_frames, int drop, int keep, int mel_frames, int first, int n_new, ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A loss over a sequence of windows, for training the net for the smoothed track: the conditional log-likelihood of the labelled windows
 * in a linear-chain CRF whose unary scores are ake_key_emissions_f32's and whose chain is ake_key_posteriors_f32's, with its gradient
 * with respect to the two heads' outputs and the transition.  Host model: metrics.key_sequence_loss.
 * ---------------------------------------------------------------------------------------- */
/* key_dev / tonic_dev [recordings][windows][12] (sigmoid memberships, tonic logits), labels_dev int32 [recordings][windows] (a key 0..23;
 * anything else = unlabelled), counts_dev, log_trans_dev and log_prior_dev as ake_key_posteriors_f32 takes them (all finite).  With
 *   e[r][w][k]   = ake_key_emissions_f32's score (same formula, same clamps, same signature_weight)
 *   e~[r][w][k]  = e[r][w][k] if label[r][w] is outside 0..23 or k == label[r][w], else -1e4 (AKE_SEQUENCE_CLAMP: finite, as the chains
 *                  require; its exponential is 0)
 *   loglik(x)    = ake_key_posteriors_f32's sum_w c_w over x, post / xi_sum its posteriors and transition sums (post~, xi~_sum over e~)
 *   N            = the windows with w < count[r] and a label in 0..23, over the whole call
 *   loss         = ( sum_r loglik(e[r]) - sum_r loglik(e~[r]) ) / N          (0, with zero gradients, when N == 0)
 * an unlabelled window is marginalised; with every window labelled this is -(score(path) - log Z) / N.  Gradients, for w < count:
 *   g[r][w][k]   = ( post[r][w][k] - post~[r][w][k] ) / N                                       (d loss / d e; d_emis_dev)
 *   d_trans[i][j] = sum_r ( xi_sum[r][i][j] - xi~_sum[r][i][j] ) / N                            (log_prior gets none)
 *   d_tonic[j]   = g[j] + g[j + 12] - softmax(tonic)[j] * sum_k g[k]
 *   d_key[j]     = signature_weight / 12 * ( sum_k S_k[j] g[k] * u(p_j) - sum_k (1 - S_k[j]) g[k] * v(p_j) )
 *   u(p) = 1 / p where p >= FLT_MIN and log p > -100, else 0;   v(p) = 1 / (1 - p) where 1 - p >= FLT_MIN and log1p(-p) > -100, else 0
 * (the derivative is 0 where nn.BCELoss's clamp is active and for subnormal arguments).
 * Outputs: scalars_dev [4] = loss, sum_r loglik / N, sum_r loglik~ / N, N; d_key_dev / d_tonic_dev [recordings][windows][12] and
 * d_emis_dev [recordings][windows][24] (nullable), zeros at w >= count; d_trans_dev [24][24], nullable.
 * Launches: 4 -- the emissions of both sets; the four chains of a recording (free / clamped x forward / backward) side by side, one wave
 * each; one block for N and the scalars (the two sums are large and nearly equal: subtracted per recording and added in recording
 * order); one thread per window for the gradients -- and 2 more with d_trans_dev: the per-chunk transition sums of both sets
 * (key_posteriors_kernel's code on float32 copies of the scores), then their difference in chunk and recording order.  The emissions
 * (ake_key_emissions_f32's arithmetic, instantiated in double), the chains (the recurrences of ake_key_posteriors_f32) and the gradient
 * run in double and are rounded to float32 once, on the way out: the gradient is a difference of two nearly equal posteriors, which
 * float32 log-scores carry only to |log-odds| * 2^-24.  No float atomics: two runs on the same inputs are bit-identical.  No
 * device-to-host copy, no synchronisation; the only memory used is the workspace and the outputs.  The
 * workspace, key_dev, tonic_dev, d_key_dev, d_tonic_dev and d_emis_dev are 16-byte aligned.  AKE_ERR_INVALID for recordings < 1,
 * windows < 1 and null required pointers, AKE_ERR_WORKSPACE for a workspace below ake_key_sequence_loss_workspace_bytes. */
size_t ake_key_sequence_loss_workspace_bytes(int recordings, int windows);
int ake_key_sequence_loss_f32(const float* key_dev, const float* tonic_dev, const int32_t* labels_dev, int recordings, int windows,
                              const int32_t* counts_dev, const float* log_trans_dev, const float* log_prior_dev, float signature_weight,
                              float* scalars_dev, float* d_key_dev, float* d_tonic_dev, float* d_trans_dev, float* d_emis_dev, void* workspace,
                              size_t workspace_bytes, ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A track against key annotations, one launch, integers only: two runs on the same inputs are bit-identical.
 * ---------------------------------------------------------------------------------------- */
/* pred_dev (int32 [recordings][windows], -1..23: key_id or the Viterbi path) against the annotations of every recording:
 * seg_start_dev (int64 [recordings][max_segments], in samples), seg_key_dev (int32, 0..23, -1 = an unlabelled stretch) and seg_count_dev
 * (int32 [recordings], clamped to 0..max_segments).  Segment s < count runs from its start to the next segment's start, the last one without
 * end; the starts ascend and segment 0 starts at 0 (entries at or behind the count are not read).  counts_dev (int32 [recordings], NULL =
 * every recording has `windows`), clamped to 0..windows.  Frame f is centred on sample f * hop, so with f0 = w * stride_frames window w
 * covers the samples lo = f0 * hop .. hi = (f0 + window_frames - 1) * hop inclusive, and its centre sample is
 * (2 * f0 + window_frames - 1) * hop / 2 (integer division), in int64.
 *   truth[r][w]    the key of the last segment that starts at or before the centre sample; -1 for w >= count, for an unlabelled segment
 *                  and for a recording without segments
 *   pure           truth >= 0 and every segment that overlaps lo..hi (start <= hi and next start > lo) carries truth's key
 *   category[r][w] -1 where truth is -1, else: 0 correct (pred == truth), 1 fifth (same mode, tonic difference mod 12 in {5, 7}),
 *                  2 relative (other mode, the same scale), 3 parallel (other mode, the same tonic), 4 other (any other decoded key),
 *                  5 undecoded (pred < 0): the relations and MIREX weights 1 / 0.5 / 0.3 / 0.2 / 0 / 0 of the transition matrix
 *   tally[r][0][c] windows of category c; tally[r][1][c] the pure ones among them
 *   changes[r][0]  the number of w in 1..count-1 with pred[w] != pred[w-1];  changes[r][1] the same for truth
 * truth_dev and category_dev (int32 [recordings][windows]) are nullable; tally_dev is int32 [recordings][2][6], changes_dev int32
 * [recordings][2].  A recording with count 0 or seg_count 0 gets zeros in both (and -1 in truth and category).
 * One block per recording, the counts meet through integer LDS atomics (order-independent). */
int ake_track_score_i32(const int32_t* pred_dev, const int32_t* counts_dev, const int64_t* seg_start_dev, const int32_t* seg_key_dev,
                        const int32_t* seg_count_dev, int recordings, int windows, int max_segments, int hop, int window_frames,
                        int stride_frames, int32_t* truth_dev, int32_t* category_dev, int32_t* tally_dev, int32_t* changes_dev,
                        ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training batches from annotated recordings, assembled on the device: window positions from a counter-based generator, the windows
 * gathered from the recordings' cached transforms (one CQT per recording, as the track makes it), their labels and a weight per window
 * from the annotations.  Two launches per batch, no host round trip.  Host models: metrics.draw_windows / metrics.window_labels.
 * ---------------------------------------------------------------------------------------- */
/* `batch` window positions, one launch, one thread per slot, integers only (identical to a Python-int restatement).  The population:
 * every start frame of every recording that is long enough, prefix_dev[i] (int64 [recordings + 1], device) = the exclusive sum of
 * max(0, T_i - window_frames + 1), N = prefix_dev[recordings].  Slot j = first_slot + b takes one Philox4x32-10 block (the synthesiser's
 * generator) with counter (j low 32, j high 32, epoch, 0x57494E44) and key (seed low, seed high); x = word0 | word1 << 32,
 * index = (x * N) >> 64, recording_out_dev[b] = the last i < recordings with prefix[i] <= index, start_out_dev[b] = index - prefix[i].
 * So a slot's draw depends on (seed, epoch, j) alone, not on how the slots are split into calls.  N > 0 is the caller's contract: N lives
 * in device memory, where this entry cannot see it without waiting for the stream (ake_amd checks it where the lengths are known, on the
 * host); with N <= 0 both outputs get -1.  AKE_ERR_INVALID for recordings < 1, batch < 0 or first_slot < 0. */
int ake_draw_windows_i32(const int64_t* prefix_dev, int recordings, uint64_t seed, uint32_t epoch, int64_t first_slot, int batch,
                         int32_t* recording_out_dev, int32_t* start_out_dev, ake_stream_t stream);
/* One launch: window b = frames [start_dev[b], start_dev[b] + window_frames) of recording recording_dev[b] (both int32 [batch], device),
 * copied out of mel_dev -- [recordings][total_frames][pitches] (frames_major != 0) or [recordings][pitches][total_frames] -- into
 * mel_out_dev [batch][1][pitches][window_frames], with the window's labels.  The host cannot see the list: entries are read clamped
 * (recording to 0..recordings-1, start to 0..total_frames-window_frames), so every load stays inside mel_dev and the annotations whatever
 * the list holds; results for out-of-range entries are unspecified.  batch <= 65535.
 * Labels, from the annotations of ake_track_score_i32 (seg_start_dev, seg_key_dev, seg_count_dev, max_segments) with its geometry at the
 * window's own start: lo = start * hop, hi = (start + window_frames - 1) * hop, centre = (2 * start + window_frames - 1) * hop / 2;
 *   truth      the key of the last segment that starts at or before centre (-1: none, or unlabelled)
 *   purity     float32(double(c) / double(hi - lo + 1)), c = the samples of lo..hi inside segments that carry truth
 *   weight     0 if truth < 0 or purity < min_purity, else 1 (uniform != 0) or purity
 *   key_labels_dev [batch][12] the scale of key truth, tonic_labels_dev [batch][12] one-hot at truth mod 12, key_signature_id_dev
 *   [batch][24] one-hot at truth (all three zeros for truth < 0), seq_length_dev [batch] int64 = window_frames, weight_dev [batch].
 * The three annotation pointers and the five label outputs are passed all together or all NULL (gather only); mel_out_dev NULL: labels
 * only (mel_dev is then not read). */
int ake_window_batch_f32(const float* mel_dev, int frames_major, int recordings, int total_frames, int pitches, int window_frames, int hop,
                         const int32_t* recording_dev, const int32_t* start_dev, int batch, const int64_t* seg_start_dev,
                         const int32_t* seg_key_dev, const int32_t* seg_count_dev, int max_segments, float min_purity, int uniform,
                         float* mel_out_dev, float* key_labels_dev, float* tonic_labels_dev, float* key_signature_id_dev,
                         int64_t* seq_length_dev, float* weight_dev, ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Additive synthesiser: recordings from lists of enveloped sinusoidal partials plus Gaussian noise, peak-normalised, float32, ragged.
 * It makes test audio whose key changes are known (synthetic.make_modulating_batch_device); host model: synthetic.synth_partials_reference.
 * ---------------------------------------------------------------------------------------- */
/* Structure of arrays, all on the device.  offsets_dev (int32 [recordings + 1]): recording r owns the partials offsets[r] .. offsets[r+1]
 * - 1 (an empty range is legal).  Per partial: cps_dev (float64, cycles per sample = f / sample rate, 0 < cps < 0.5), phase_dev (float64,
 * turns, in [0, 1)), amp_dev (float32), start_dev / end_dev (int64): the partial sounds on the samples start <= t < end, which may be
 * negative or reach beyond the recording (it is clipped).  fade >= 0 samples, one value per call.  n_dev (int64 [recordings]) samples of
 * every row, at most n_max; stride (floats between rows) a multiple of 4 and >= n_max; out_dev 16-byte aligned.  For t < n_r:
 *   y[t]  = sum over the partials p of r with start_p <= t < end_p of  amp_p * g_in * g_out * sin(2 pi frac(cps_p * t + phase_p))
 *           + noise_sigma * z_r[t]
 *   g_in  = 1 if fade == 0 or t - start >= fade,        else 0.5 - 0.5 cos(pi (t - start + 0.5) / fade)
 *   g_out = 1 if fade == 0 or m = end - 1 - t >= fade,  else 0.5 - 0.5 cos(pi (m + 0.5) / fade)
 * so a partial that ends at E and one that starts at E - fade cross-fade with envelopes that sum to 1.  Samples n_r <= t < stride are
 * written as 0.  cps * t + phase is one float64 fma and its fraction (minus its floor) is taken in float64; only the fraction is rounded
 * to float32, so the phase error does not grow with t.  Sine, cosine and logarithm are the accurate library forms.
 * Noise: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key (seed_dev[r] low 32 bits, high 32
 * bits), counter (b low, b high, r, 0) with b = t >> 2.  Its words x_0..x_3 give u_k = ((x_k >> 9) + 0.5) * 2^-23 (exact, never 0) and the
 * samples 4b .. 4b+3 get R(u_0) cos(2 pi u_1), R(u_0) sin(2 pi u_1), R(u_2) cos(2 pi u_3), R(u_2) sin(2 pi u_3), R(u) = sqrt(-2 ln u).
 * With noise_sigma == 0 nothing is drawn and seed_dev may be NULL.
 * peak > 0: a second pass scales every recording so that max |y| over t < n_r is peak (an all-zero recording stays zero); peak == 0: no
 * normalisation, and no workspace is needed.  The maximum is an integer atomicMax on the float's bit pattern, one per block, so two runs
 * are bit-identical; the workspace (ake_synth_partials_workspace_bytes) holds it.
 * A thread makes 4 consecutive samples (one 16-byte store), a block 1024 samples of one recording: it compacts the partials that
 * overlap its tile into LDS, ake_synth_batch_partials() candidates at a time and in their own order, so any number of partials runs. */
size_t ake_synth_partials_workspace_bytes(int recordings);
int ake_synth_batch_partials(void);
int ake_synth_partials_f32(const int32_t* offsets_dev, const double* cps_dev, const double* phase_dev, const float* amp_dev,
                           const int64_t* start_dev, const int64_t* end_dev, int fade, int recordings, const int64_t* n_dev, int64_t n_max,
                           int64_t stride, float noise_sigma, const int64_t* seed_dev, float peak, float* out_dev, void* workspace,
                           size_t workspace_bytes, ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Tuning: how far a recording sits from A4 = 440 Hz, and the resampler that puts it back.  Not in the reference (its librosa 0.9.2
 * transform runs at tuning = 0.0).  Opt-in: nothing else in this library calls either.  Host models: metrics.estimate_tuning and
 * metrics.retune_reference.
 * ---------------------------------------------------------------------------------------- */
/* The estimate, from a log-CQT with 3 bins per semitone and in-tune notes on the bins k = 0 (mod 3) (36 bins per octave from C1):
 * mel_dev is [batch][pitches][frames] (frames_major == 0, as ake_cqt_logmag*_f32 write it) or [batch][frames][pitches] (frames_major
 * != 0, ake_cqt_logmag_frames_major_f32).  counts_dev (int32 [batch], nullable): recording i has counts[i] frames, clamped to
 * 0..frames; the ragged transforms write zeros behind a recording's frames, which add nothing, so their output needs no counts.  With
 * m = expm1(mel) and P_j the sum of m^2 over the bins k = j (mod 3) and the recording's frames:
 *   z = P_0 + P_1 e^{2 pi i / 3} + P_2 e^{4 pi i / 3}
 *   cents_dev[i]    = 100 arg(z) / (2 pi), in (-50, 50], positive = sharp
 *   strength_dev[i] = |z| / (P_0 + P_1 + P_2), in [0, 1]: 1 when all the power sits on one bin position, 0 when the three carry the same
 * A recording without power gets (0, 0), never NaN.  A recording whose strength is below min_strength gets cents 0 (the decision is
 * made on the device, on the strength in double).  pitches that are no multiple of 3: AKE_ERR_UNSUPPORTED.
 * Two launches: blocks of (64 frames, one recording) reduce their tile to the three sums in double (expm1 in double), then one thread
 * per recording adds its chunks in chunk order and evaluates atan2 in double.  No floating-point atomics: two runs on the same input
 * are bit-identical.  The workspace (8-byte aligned) holds the per-chunk sums. */
size_t ake_tuning_workspace_bytes(int batch, int frames);
int ake_tuning_estimate_f32(const float* mel_dev, int frames_major, int batch, int pitches, int frames, const int32_t* counts_dev,
                            float min_strength, float* cents_dev, float* strength_dev, void* workspace, size_t workspace_bytes,
                            ake_stream_t stream);
/* The tuning track: the same estimate over sliding windows of frames, for recordings whose tuning drifts (a tape that changes speed),
 * and the curve that ake_retune_curve_f32 follows.  mel_dev, frames_major, counts_dev and pitches as above; window_frames >= 1,
 * stride_frames >= 1.  Recording i with T_i frames has W_i = 1 + (T_i - window_frames) / stride_frames windows when T_i >= window_frames,
 * one window over all its frames when 0 < T_i < window_frames, none when T_i = 0; window w covers the frames
 * [w stride_frames, min(w stride_frames + window_frames, T_i)).  Every output row has W = ake_tuning_track_windows(frames, window_frames,
 * stride_frames) columns, the count of a recording of `frames` frames (-1 for a bad geometry), so a caller sizes them without a read-back.
 *   cents_raw_dev, strength_dev float32 [batch][W]: the formulas above on each window's three sums, which are added in double in ascending
 *     frame order; min_strength is not applied to them; columns >= W_i hold 0.
 *   curve_dev float32 [batch][W], per recording in window order: a window with strength < min_strength takes the value of the nearest
 *     earlier window that is not (the leading ones that of the first such window; 0 everywhere when there is none); then +-100 is added
 *     so that each value lies within 50 of the unwrapped value before it (v + 100 floor((before - v) / 100 + 0.5)); then the value is
 *     clamped to +-50 -- a drift that leaves the semitone saturates, it does not jump; columns >= W_i repeat the last valid value.  The
 *     decisions are made on the doubles.
 *   window_counts_dev int32 [batch]: W_i.
 * Three launches: every frame's three sums once (not once per overlapping window), a thread per window, a thread per recording.  No
 * floating-point atomics: two runs give the same bits.  The workspace (8-byte aligned) holds the per-frame sums and the windows'
 * doubles.  Refusals as ake_tuning_estimate_f32's, and AKE_ERR_INVALID for a bad geometry; nothing is launched after any of them.
 * Host model: metrics.tuning_track. */
int ake_tuning_track_windows(int frames, int window_frames, int stride_frames);
size_t ake_tuning_track_workspace_bytes(int batch, int frames, int window_frames, int stride_frames);
int ake_tuning_track_f32(const float* mel_dev, int frames_major, int batch, int pitches, int frames, const int32_t* counts_dev,
                         int window_frames, int stride_frames, float min_strength, float* cents_raw_dev, float* strength_dev,
                         float* curve_dev, int32_t* window_counts_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream);
/* Retuning: row i is resampled by rho_i = 2^(cents_dev[i] / 1200), which undoes a detuning of cents_dev[i] (float32 [batch]; NaN is read
 * as 0, values beyond +-50 as +-50).  in_dev [batch][in_stride], row i holds lengths_dev[i] samples (int64, clamped to 0..n_max; NULL:
 * n_max).  n_out_i = floor(n_i * rho_i), written to lengths_out_dev (int64 [batch], nullable), and
 *   y[k] = sum_j x[j] h(k / rho_i - j)   over |k / rho_i - j| < Z,   x = 0 outside [0, n_i)
 *   h(d) = c sinc(c d) I0(beta sqrt(1 - (d / Z)^2)) / I0(beta),   Z = 32, beta = 9, c = 0.94
 * One filter for every row: c < 2^(-50/1200) = 0.9715, so nothing above the new Nyquist frequency folds back below 0.94 of it;
 * content above 0.94 of the old Nyquist frequency is discarded.  h is held at 256 entries per sample and blended linearly between
 * neighbours; k / rho_i is computed in double and only its fraction rounded to float32; the 64 taps are added by fmaf in ascending j.
 * out_dev [batch][out_stride]: columns [0, ake_retune_out_len(n_max)) of every row are written, zeros at and behind n_out_i;
 * out_stride >= ake_retune_out_len(n_max) = floor(n_max * 2^(50/1200)) + 1 (2^(50/1200) is one double literal, 1.029302236643492, for this
 * function and for the kernel's ratio at +-50 cents, so n_out_i < the width always), the longest possible row plus one, so a caller sizes the
 * buffer without reading a ratio back.  A row with cents == 0 is copied bit for bit.  One launch.  The PCM form reads int16 in place
 * (any base, any stride >= n_max) and gives the float form's results on the converted audio (s / 32768), bit for bit.
 * The first call on a device uploads the filter table (32 KiB, a synchronous copy): make it before capturing into a graph. */
int64_t ake_retune_out_len(int64_t n);
int ake_retune_f32(const float* in_dev, int batch, int64_t n_max, int64_t in_stride, const int64_t* lengths_dev, const float* cents_dev,
                   float* out_dev, int64_t out_stride, int64_t* lengths_out_dev, ake_stream_t stream);
int ake_retune_pcm16_f32(const int16_t* in_dev, int batch, int64_t n_max, int64_t in_stride, const int64_t* lengths_dev,
                         const float* cents_dev, float* out_dev, int64_t out_stride, int64_t* lengths_out_dev, ake_stream_t stream);
/* Retuning along a curve: ake_retune_f32 with a ratio that is piecewise linear in the input position (host models
 * metrics.retune_curve_reference, retune_curve_forward, retune_curve_positions).  cents_dev float32 [batch][cents_stride], `knots` >= 1
 * values a row (ake_tuning_track_f32's curve goes straight in); knot i sits at input sample p_i = knot_first + i knot_step (knot_first
 * >= 0, knot_step >= 64) and carries rho_i = 2^(cents_i / 1200), read as ake_retune_f32 reads its cents.  rho is rho_0 in front of the
 * first knot, rho_{knots-1} behind the last, linear in p between two.  The output index of input position p is
 *   K(p) = rho_0 p in front of the first knot;  K_0 = rho_0 p_0,  K_{i+1} = K_i + knot_step (rho_i + rho_{i+1}) / 2  (double, ascending i)
 *   K(p) = K_i + rho_i u + (rho_{i+1} - rho_i) u^2 / (2 knot_step),  u = p - p_i, inside segment i
 * n_out_i = floor(K(n_i)) < ake_retune_out_len(n_max), the buffer's width as before.  Output k reads the position K^{-1}(k): with s the
 * last segment with K_s <= k, c = k - K_s and a = (rho_{s+1} - rho_s) / (2 knot_step), u = 2 c / (rho_s + sqrt(rho_s^2 + 4 a c)); k / rho_0 in
 * front of the first knot, c / rho_{knots-1} behind the last.  The position is kept as the integer p_s + floor(u) and the fraction
 * u - floor(u); only the fraction is rounded to float32.  Taps, table, blend and sum order are ake_retune_f32's own code.  A row whose
 * clamped cents are all exactly 0 is copied bit for bit.  The PCM form gives the float form's results bit for bit.
 * Two launches: a prefix launch writes rho_i, K_i, n_out_i and the copy flag into the workspace (ake_retune_curve_workspace_bytes(batch,
 * knots), 8-byte aligned; 0 for a batch outside 1..65535 or knots outside 1..2^22), then the resampling launch.
 * ake_retune_curve_positions: positions_dev double [batch][m] = K^{-1}(out_index_dev[batch][m]) by the device function the resampler
 * uses (the prefix launch, then a thread per index).
 * AKE_ERR_INVALID: a null argument (lengths_dev and lengths_out_dev may be null), a bad batch or n_max, knots < 1, knot_step outside
 * 64..2^32, knot_first outside 0..2^40, in_stride < n_max, out_stride < the width, cents_stride < knots, m < 1, a misaligned workspace;
 * AKE_ERR_WORKSPACE: workspace_bytes below the query.  Nothing is launched after any of them. */
size_t ake_retune_curve_workspace_bytes(int batch, int knots);
int ake_retune_curve_f32(const float* in_dev, int batch, int64_t n_max, int64_t in_stride, const int64_t* lengths_dev, const float* cents_dev,
                         int knots, int64_t cents_stride, int64_t knot_first, int64_t knot_step, float* out_dev, int64_t out_stride,
                         int64_t* lengths_out_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream);
int ake_retune_curve_pcm16_f32(const int16_t* in_dev, int batch, int64_t n_max, int64_t in_stride, const int64_t* lengths_dev,
                               const float* cents_dev, int knots, int64_t cents_stride, int64_t knot_first, int64_t knot_step, float* out_dev,
                               int64_t out_stride, int64_t* lengths_out_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream);
int ake_retune_curve_positions(const float* cents_dev, int batch, int knots, int64_t cents_stride, int64_t knot_first, int64_t knot_step,
                               const int64_t* out_index_dev, int64_t m, double* positions_dev, void* workspace, size_t workspace_bytes,
                               ake_stream_t stream);

/* The retuner on audio that arrives in chunks, all recordings in lockstep (KeyEstimator.stream(retune_cents=...), ake_amd.StreamRetuner;
 * host model metrics.stream_retune).  Z, the table, beta and the cutoff are ake_retune_f32's.
 *   ake_retune_ratio(cents, rho_out, stream): rho = 2^(cents / 1200) as retune_kernel itself computes it (NaN as 0, the literal at the
 *   +-50 clamp), by a one-thread launch of the kernel's own device function and a copy back; it waits for `stream`.  The host's exp2 may
 *   differ from the device's in the last place, and one ulp of rho moves read positions and counts.  Call it once per stream; every
 *   other entry here takes `cents` and this rho, and none of them reads anything back.
 * With inv = 1.0 / rho, output k reads the inputs floor(k inv) - 31 .. floor(k inv) + 32 (zeros outside [0, n)), so it is final once
 * floor(double(k) * inv) + 32 <= n_in - 1.
 *   ake_stream_retune_out_count(cents, rho, n_in, flush) (host only; -1 for n_in outside 0..2^40 or a rho outside
 *   [1 / 1.029302236643492, 1.029302236643492]) = the size of that prefix, found by testing this very double expression around
 *   floor((n_in - 32) * rho); with flush floor(double(n_in) * rho), the offline count (never above ake_retune_out_len(n_in) - 1); with
 *   cents == 0 after the clamp, n_in: such a stream is a stateless copy, output k is input k.
 * A call takes the next m samples of every recording, chunk_dev[rec * rec_stride + i], after the n_before it has been given so far, and
 * writes the outputs k in [out_count(n_before, 0), out_count(n_before + m, flush)) to out_dev[rec * out_stride + (k - first)]; *k_out (a
 * host integer, required) is their number; out_dev behind it is not touched.  The outputs equal ake_retune_f32 / ake_retune_pcm16_f32 on
 * the concatenated audio BIT FOR BIT, however the audio is cut into calls: the kernels share the offline kernel's per-sample code.
 * ONE RATIO PER CALL: all recordings of a call share cents and rho.  Recordings with ratios of their own would finish different numbers
 * of samples per push; that needs streams that do not advance in lockstep, which are not built.
 * state_dev: ake_stream_retune_state_bytes(recordings) = recordings * 256 bytes (0 for recordings outside 1..65535), 16-byte aligned: per
 * recording a ring of the last 64 inputs as float32 (16-bit samples converted, s / 32768, before they are stored), input i at slot i % 64.
 * With n_before == 0 it is not read, so a fresh stream needs no initialising launch; cents == 0 never touches it.
 * Launches: stream_retune_kernel (1024 outputs a workgroup in four tiles of 256, the table and each tile's input staged in LDS; reads
 * the ring), then stream_retune_tail_kernel (writes the ring from the chunk's end) -- two, so that no workgroup reads what another
 * writes.  A call with no output skips the first; m == 0, cents == 0 or flush the second; a call with neither launches nothing.  Plain
 * loads and stores, no atomics.  The first filtering call on a device uploads the filter table, as ake_retune_f32's does.
 * AKE_ERR_INVALID: a null state_dev or k_out, chunk_dev with m > 0, out_dev with *k_out > 0; recordings outside 1..65535; m or n_before
 * outside 0..2^40; rec_stride negative; out_stride < *k_out; a rho outside the range above (NaN included); a misaligned state.
 * AKE_ERR_WORKSPACE: state_bytes below the query.  Nothing is launched after any of them. */
int ake_retune_ratio(float cents, double* rho_out, ake_stream_t stream);
int64_t ake_stream_retune_out_count(float cents, double rho, int64_t n_in, int flush);
size_t ake_stream_retune_state_bytes(int recordings);
int ake_stream_retune_f32(const float* chunk_dev, int recordings, int64_t m, int64_t rec_stride, float cents, double rho, int64_t n_before,
                          int flush, void* state_dev, size_t state_bytes, float* out_dev, int64_t out_stride, int64_t* k_out,
                          ake_stream_t stream);
int ake_stream_retune_pcm16_f32(const int16_t* chunk_dev, int recordings, int64_t m, int64_t rec_stride, float cents, double rho,
                                int64_t n_before, int flush, void* state_dev, size_t state_bytes, float* out_dev, int64_t out_stride,
                                int64_t* k_out, ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Key-profile emissions: a key track without a trained net (Krumhansl-Schmuckler).  Not in the reference.  Opt-in: nothing else in this
 * library calls it.  Host model: metrics.profile_emissions.
 * ---------------------------------------------------------------------------------------- */
/* mel_dev, frames_major and counts_dev (frames of every recording, clamped to 0..frames; nullable) as in ake_tuning_estimate_f32: a
 * log-CQT L with 3 bins per semitone from C, in-tune notes on the bins k = 0 (mod 3).  Bin k belongs to semitone (k + 1) / 3 and pitch
 * class ((k + 1) / 3) % 12; semitone 0 lacks its flat-side bin and the top bin is the flat side of a semitone above the range, both kept
 * as they come.  pitches that are no multiple of 3: AKE_ERR_UNSUPPORTED.  compression: 0 v = L, 1 v = expm1(L), 2 v = expm1(L)^2;
 * anything else AKE_ERR_INVALID.
 *   c[r][t][j] = sum of v[r][k][t] over the bins k of pitch class j, in ascending k
 *   x[r][w][j] = sum of c[r][t][j] over t = w * stride_frames .. w * stride_frames + window_frames - 1, in ascending t
 * Recording r with n_r frames has (n_r - window_frames) / stride_frames + 1 windows (0 if n_r < window_frames); windows must equal
 * ake_profile_windows(frames, window_frames, stride_frames), that count for n_r = frames (AKE_ERR_INVALID otherwise; -1 from
 * ake_profile_windows for frames < 1, window_frames < 0 or stride_frames < 1, which the entry refuses likewise).  window_frames == 0 is
 * the whole-clip mode: windows == 1, one window over the recording's own n_r frames, none for n_r == 0.
 * profiles_dev is float32 [2][12], rows minor and major, tonic first, finite and not constant within a row (the caller's contract; a
 * constant row scores 0 everywhere).  Key k (0..11 minor, 12..23 major, tonic k % 12) has the profile q_k[j] = row[(j - tonic) % 12];
 * r_k is the Pearson correlation of x and q_k over the 12 pitch classes, in double, every sum in ascending j with the means taken
 * first; the rows' means and centred norms are computed once per block.
 *   emissions_out [recordings][windows][24] = sharpness * r_k   (sharpness NaN or <= 0: AKE_ERR_INVALID)
 *   key_id_out    [recordings][windows]     = the smallest k that attains the maximum r_k, decided on the double values
 *   confidence_out[recordings][windows]     = that r_k
 *   chroma_out    [recordings][windows][12] = x / sum_j x_j
 * A window with sum_j (x_j - mean)^2 <= 1e-12 * 12 * mean^2 (all-zero chroma included) is silent: zeros, and -1 in key_id_out.  Windows
 * at or behind a recording's count get the same.  Every output element is written.
 * Two launches: blocks of (64 frames, one recording) write c in double into the workspace (expm1 in double; zeros for frames at or
 * behind n_r, so what the workspace held never matters), then one block per (window, recording) adds its frames and scores them.  No
 * floating-point atomics: two runs on the same input are bit-identical.  The workspace (8-byte aligned) holds c. */
size_t ake_profile_workspace_bytes(int recordings, int frames);
int ake_profile_windows(int frames, int window_frames, int stride_frames);
int ake_profile_emissions_f32(const float* mel_dev, int frames_major, int recordings, int pitches, int frames, const int32_t* counts_dev,
                              int window_frames, int stride_frames, int windows, const float* profiles_dev /* [2][12] */, int compression,
                              float sharpness, float* chroma_out, float* emissions_out, int32_t* key_id_out, float* confidence_out,
                              void* workspace, size_t workspace_bytes, ake_stream_t stream);

/* Tuned chroma (csrc/profile_tuned.hip): ake_profile_emissions_f32 on a detuned recording without retuning it.  The class boundaries
 * move by the detuning and split the one bin each crosses.  Host model: metrics.profile_emissions(cents=...).  Every argument of
 * ake_profile_emissions_f32 means what it means there, with the same refusals and outputs, except that pitches must be a multiple of 36
 * (whole octaves; AKE_ERR_UNSUPPORTED otherwise).  Window (r, w) reads its detuning from
 * cents_dev[r * cents_rec_stride + w * cents_win_stride] (float32 cents; NaN reads as 0, beyond +-50 as +-50; strides in elements, not
 * negative; a window stride of 0 gives one value per recording); only windows in front of a recording's count are read.  A null
 * cents_dev is AKE_ERR_UNSUPPORTED.  With p = k % 36 the folded position of bin k:
 *   F[r][t][p]  = sum of v[r][p + 36 o][t] over the octaves o, ascending
 *   FW[p]       = sum of F[r][t][p] over the window's frames, ascending t
 *   delta = 3.0 * c / 100.0,  n = floor(delta - 1.0) in {-3 .. 0},  g = delta - 1.0 - n in [0, 1)
 *   x[r][w][j]  = (((1 - g) FW[b0] + FW[b1]) + FW[b2]) + g FW[b3],   b_i = (3 j + n + i) % 36
 * in double, every product rounded before it is added, a term of weight 0 left out.  At c = 0 that is FW[3j-1] + FW[3j] + FW[3j+1],
 * ake_profile_emissions_f32's classes (in another order of addition).  Everything behind x is that entry's scoring.
 * Two launches: blocks of (64 frames, one recording) write F in double into the workspace (zeros for frames at or behind n_r, so what
 * the workspace held never matters), then one block per (window, recording) adds its frames, cuts the classes and scores them.  No
 * atomics: two runs on the same input are bit-identical, and so are the two layouts.  The workspace (8-byte aligned) holds F:
 * ake_profile_tuned_workspace_bytes (0 for recordings outside 1..65535 or frames < 1); too small or null: AKE_ERR_WORKSPACE.  A refused
 * call launches nothing. */
size_t ake_profile_tuned_workspace_bytes(int recordings, int frames);
int ake_profile_emissions_tuned_f32(const float* mel_dev, int frames_major, int recordings, int pitches, int frames, const int32_t* counts_dev,
                                    int window_frames, int stride_frames, int windows, const float* profiles_dev /* [2][12] */,
                                    int compression, float sharpness, const float* cents_dev, int64_t cents_rec_stride,
                                    int64_t cents_win_stride, float* chroma_out, float* emissions_out, int32_t* key_id_out,
                                    float* confidence_out, void* workspace, size_t workspace_bytes, ake_stream_t stream);

/* The profile method and a tuning meter on a stream of audio in lockstep (csrc/stream_profile.hip; KeyEstimator.stream(method="profile",
 * tuning_meter=True)).  Host models: metrics.stream_profile and metrics.stream_tuning.
 * state_dev holds, per recording, a ring of per-frame chroma, double [recordings][ring_frames][12] with the stream's frame t in row
 * t % ring_frames (c[t][j] as above), and behind all rings the running sums P_0, P_1, P_2 of ake_tuning_estimate_f32 as double
 * [recordings][3]: ake_stream_profile_state_bytes(recordings, ring_frames) bytes (0 for recordings outside 1..65535 or ring_frames < 1),
 * 16-byte aligned.  The device keeps no count: frames_before and first_window are the host's.
 * ake_stream_frame_stats_f32 takes the n_new frames from frame `first` on of a transform's output mel_dev (mel_frames frames,
 * [recordings][pitches][mel_frames], or [recordings][mel_frames][pitches] with frames_major != 0), the stream's frames frames_before ..
 * frames_before + n_new - 1.  parts: 1 the chroma, 2 the tuning, 3 both; the part that is off is neither read nor written.
 *   chroma: c[t][j] in double, ake_profile_emissions_f32's sum to the bit (compression 0 / 1 / 2 as there), into the ring row of every
 *     new frame, whether a window needs it or not, so the ring's bytes after N frames do not depend on how they were cut into calls;
 *     of more than ring_frames new frames the last ring_frames are written.
 *   tuning: p_j(t) = the sum of expm1(L)^2 over the bins k = j (mod 3) of frame t, in ascending k, in double; P_j += p_j(t) in ascending
 *     t; then cents_out / strength_out float32 [recordings] by ake_tuning_estimate_f32's formulas on P (atan2 in double, strength
 *     clamped to 1, (0, 0) without power, cents = 0 where the double strength < min_strength): the estimate over every frame so far.
 * With frames_before == 0 the state is not read, and every part that is on is written whole (ring rows no frame has reached: zeros).
 * n_new == 0 launches nothing and leaves the state and the two outputs alone (there is no read-out without new frames: a caller keeps
 * the last call's outputs).  One launch, stream_frame_stats_kernel: a workgroup per recording walks the new frames in tiles of 64, the
 * loads of twelve bins in flight at a time; the squared magnitudes of the tuning part are computed an element per thread into the LDS
 * (up to 4623 bins; beyond, by the thread that adds them), and the frame-order addition is one thread's per P_j, behind a barrier.
 * ake_stream_profile_emissions_f32 scores the k windows from first_window on of a stream that has `frames` frames so far (frames_before
 * + n_new of the last call): window w covers the frames w * stride_frames .. w * stride_frames + window_frames - 1, read from the ring
 * in ascending t, then ake_profile_emissions_f32's scoring (means first, Pearson correlation in double, the silence rule, the first
 * maximum on the doubles).  Outputs [recordings][k][...]: chroma_out (12), emissions_out (24), key_id_out, confidence_out as there;
 * tonic_out (12) = max(emissions[t], emissions[12 + t]); tonic_id_out = key_id % 12, or -1; signature_id_out =
 * key_signature_dev[key_id] (int32 [24], the caller's table), or -1 for a silent window.  One launch, stream_profile_score_kernel, a
 * block per (new window, recording); k == 0 launches nothing.
 * No atomics: reruns are bit-identical, and neither the outputs nor the state depend on how a stream's frames are cut into calls.
 * AKE_ERR_INVALID: null arguments, recordings outside 1..65535, ring_frames < 1 (emissions: < window_frames), window_frames < 1,
 * stride_frames < 1, first / n_new outside mel_frames, parts outside 1..3, compression outside 0..2 (with the chroma part), min_strength
 * NaN (with the tuning part), sharpness NaN or <= 0, a window that ends behind `frames` or begins in front of frames - ring_frames (its
 * frames are not yet, or no longer, in the ring).  AKE_ERR_UNSUPPORTED: pitches % 3 != 0.  AKE_ERR_WORKSPACE: state_bytes short.
 * Nothing is launched on a refusal. */
size_t ake_stream_profile_state_bytes(int recordings, int ring_frames);
int ake_stream_frame_stats_f32(const float* mel_dev, int frames_major, int recordings, int pitches, int mel_frames, int first, int n_new,
                               int64_t frames_before, int ring_frames, int parts, int compression, float min_strength, void* state_dev,
                               size_t state_bytes, float* cents_out, float* strength_out, ake_stream_t stream);
int ake_stream_profile_emissions_f32(const void* state_dev, size_t state_bytes, int recordings, int ring_frames, int64_t frames,
                                     int window_frames, int stride_frames, int64_t first_window, int k, const float* profiles_dev /* [2][12] */,
                                     float sharpness, const int32_t* key_signature_dev /* [24] */, float* chroma_out, float* emissions_out,
                                     int32_t* key_id_out, float* confidence_out, float* tonic_out, int32_t* tonic_id_out,
                                     int32_t* signature_id_out, ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Key changes to the frame (csrc/changes.hip): where, between the centres of two windows of a key track that carry different keys,
 * the key changes.  Not in the reference.  Opt-in: nothing else in this library calls it.  Host model: metrics.key_changes.
 * ---------------------------------------------------------------------------------------- */
/* mel_dev, frames_major, pitches, frames, profiles_dev and compression as in ake_profile_emissions_f32; frame_counts_dev (nullable)
 * gives every recording's frames T_r, clamped to 0..frames.  labels_dev is int32 [recordings][windows], a key 0..23 per window of
 * window_frames frames, stride_frames apart (anything else is no key); window_counts_dev (nullable) the windows of every recording,
 * clamped to 0..windows and to the (T_r - window_frames) / stride_frames + 1 windows that T_r frames hold.
 * s[t][k] is frame t's Pearson correlation with key k's profile: ake_profile_emissions_f32's with window_frames = stride_frames =
 * sharpness = 1, in double and unfused, the silence rule included (a silent frame scores 0 for every key).
 * With m_w = w * stride_frames + window_frames / 2, boundary w (between the windows w and w + 1) exists iff w + 1 < the recording's
 * window count and a = labels[w], b = labels[w + 1] are two different keys.  Its span is lo = max(m_w - slack_frames, 0) ..
 * hi = min(m_{w+1} + slack_frames, T_r), with lo = max(lo, m_w) if w >= 1 and labels[w - 1] != a, and hi = min(hi, m_{w+1}) if
 * w + 2 < the window count and labels[w + 2] != b: the spans on either side of a run of one window share one frame at the most (those
 * of a run of k windows lie apart when (k - 1) * stride_frames >= 2 * slack_frames), and there the change frames never decrease.
 *   d_i = s[lo + i][a] - s[lo + i][b],  C_0 = 0,  C_{i+1} = C_i + d_i in ascending i,  j* = the smallest j in 0..hi-lo with C_j maximal
 *   change_frame_out [recordings][windows - 1] = lo + j*: the frames below it belong to a, the rest to b
 *   gain_out         [recordings][windows - 1] = C_{j*} - C_{g - lo}, g = clamp(m_w + (stride_frames + 1) / 2, lo, hi), the grid's place
 *   contrast_out     [recordings][windows - 1] = (2 C_{j*} - C_{hi-lo}) / (hi - lo), the mean advantage of each side's own key, in -2..2
 * Where there is no boundary: -1, 0, 0.  Every output element is written by every call; two runs give the same bits.
 * One launch, key_changes_kernel, a workgroup per (boundary, recording), no workspace; the C_j are added by one thread, in order.
 * windows < 2: AKE_OK, nothing launched.  AKE_ERR_INVALID: null arguments (the two counts excepted), recordings outside 1..65535,
 * pitches, frames < 1, windows < 0, compression outside 0..2, window_frames < 1, stride_frames < 1, slack_frames < 0.
 * AKE_ERR_UNSUPPORTED: pitches % 3 != 0; stride_frames + 2 * slack_frames > 1024, the longest span the kernel holds. */
int ake_key_changes_f32(const float* mel_dev, int frames_major, int recordings, int pitches, int frames, const int32_t* frame_counts_dev,
                        const int32_t* labels_dev, int windows, const int32_t* window_counts_dev, int window_frames, int stride_frames,
                        int slack_frames, const float* profiles_dev /* [2][12] */, int compression, int32_t* change_frame_out,
                        float* gain_out, float* contrast_out, ake_stream_t stream);

/* The same inside a key stream (csrc/stream_changes.hip; KeyEstimator.stream(refine=True)).  Host model: metrics.stream_key_changes.
 * Joined over a stream's calls the three outputs are ake_key_changes_f32's on the joined frames and labels with frame_counts = the
 * stream's frames and window_counts = its decided windows at the end, to the bit: both kernels call csrc/changes.h.
 * chroma_state_dev is the state of ake_stream_frame_stats_f32 with its chroma part on (ring_frames rows a recording, frame t in row
 * t % ring_frames), read only, after the call that brought the stream to `frames` frames.  labels_dev is int32 [recordings][k]: the
 * labels of the windows labels_before .. labels_before + k - 1, decided since the last call (a stream's key_id, or its smooth_key_id,
 * which trails the windows by the lag until the flush).  label_state_dev carries the labels of earlier calls: int32
 * [recordings][label_ring], window v in slot v % label_ring, ake_stream_key_changes_state_bytes(recordings, label_ring) bytes (0 for
 * recordings outside 1..65535 or label_ring < 1).  The device keeps no count: labels_before, first_boundary and n_boundaries are the
 * host's.
 * With L = labels_before + k, boundary w (between the windows w and w + 1, m_w as above) is final iff w + 2 < L and
 * frames >= m_{w+1} + slack_frames, or flush != 0 (the recordings end here: T_r = frames, the window count is L) and w + 1 < L
 * (metrics.stream_changes_ready counts them).  A call computes the boundaries first_boundary .. first_boundary + n_boundaries - 1, all of
 * which must be final; a stream passes those that became final with this call, each once.
 *   change_frame_out, gain_out, contrast_out [recordings][n_boundaries]: as ake_key_changes_f32 defines them, change_frame_out counting
 *   the stream's frames; -1, 0, 0 where the two windows do not carry two different keys.  Every element is written.
 * One launch, stream_key_changes_kernel, a workgroup per (boundary, recording): the four labels out of the ring or the call's own,
 * the span's chroma rows out of the chroma ring (a frame per thread, all of a span of up to 1024 frames in one pass), the ordered sum
 * by one thread.  The first workgroup of every recording also writes the call's labels into the label ring (alone, where a call
 * brings labels and completes no boundary); the ring must be long enough that these slots and the ones the call reads cannot meet:
 * k <= label_ring, and L - max(first_boundary - 1, 0) <= label_ring where that window was decided before this call.
 * With labels_before == 0 the label state is not read and is written whole (-1 in the slots no window has reached).  k == 0 with
 * n_boundaries == 0 launches nothing.  No atomics, no workspace: reruns are bit-identical, and neither the outputs nor the label state
 * depend on how a stream's labels and frames are cut into calls.
 * AKE_ERR_INVALID: null arguments (labels_dev with k == 0 and the outputs with n_boundaries == 0 excepted), recordings outside
 * 1..65535, ring_frames or label_ring < 1, window_frames < 1, stride_frames < 1, slack_frames < 0, k or n_boundaries outside 0..65535,
 * frames, labels_before or first_boundary outside 0..2^30, a decided window that ends behind `frames`, and counts that break the
 * rule: a boundary whose labels are not yet known, one whose frames have not yet arrived, one whose first frame
 * max(m_w - slack_frames, 0) lies in front of frames - ring_frames (no longer in the chroma ring), and label slots that would meet.
 * AKE_ERR_UNSUPPORTED: stride_frames + 2 * slack_frames > 1024.  AKE_ERR_WORKSPACE: either state's bytes short.  Nothing is launched
 * on a refusal. */
size_t ake_stream_key_changes_state_bytes(int recordings, int label_ring);
int ake_stream_key_changes_f32(const void* chroma_state_dev, size_t chroma_state_bytes, int recordings, int ring_frames, int64_t frames,
                               const int32_t* labels_dev, int k, int64_t labels_before, int flush, int window_frames, int stride_frames,
                               int slack_frames, const float* profiles_dev /* [2][12] */, void* label_state_dev, size_t label_state_bytes,
                               int label_ring, int64_t first_boundary, int n_boundaries, int32_t* change_frame_out, float* gain_out,
                               float* contrast_out, ake_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-kernel timing with hipEvents recorded on the launch stream (bench.py roofline leg).
 * ---------------------------------------------------------------------------------------- */
int ake_prof_enable(const char* name_filter /* substring, NULL or "" = all */, int on);
int ake_prof_collect(void);                 /* synchronises the recorded events, accumulates */
int ake_prof_reset(void);
int ake_prof_num_entries(void);
int ake_prof_entry(int index, const char** kernel_name, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* AKE_HIP_H */
