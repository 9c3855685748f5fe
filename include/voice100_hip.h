/* voice100_hip.h -- C ABI of libvoice100_hip.so: the MI355X (gfx950) kernels behind the
 * Voice100 non-autoregressive CNN hot path.
 *
 * The reference (kaiidams/voice100 v1.6.0) has no FFI of its own: the path is plain
 * torch.nn modules.  Each entry point below therefore cites the
 * reference call it stands in for; voice100_amd/ (Python, ctypes) mirrors the reference's
 * module interface on top of these.  INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'd / torch CUDA tensor storage), 16-byte
 *     aligned, contiguous; activations are fp32 [B][C][T] unless stated otherwise;
 *   - no allocation, no host synchronisation inside: outputs and workspaces ("stats",
 *     "partial") are caller-allocated, `stream` is a hipStream_t (NULL = default stream);
 *   - return value: 0 = launched; 1 = invalid/unsupported shape or mode; 2 = launch error;
 *     3 = a required pointer is NULL.  The Python layer raises RuntimeError on != 0;
 *   - re-entrant; the only global state is the opt-in timing table below; one stream per process is the
 *     intended use.
 */
#ifndef VOICE100_HIP_H
#define VOICE100_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- input-transform modes shared by the depthwise and pointwise kernels ------------------
 *   0 NONE            v
 *   1 AFFINE_RELU6    clamp(v*a[c] + b[c], 0, 6)      BatchNorm affine + ReLU6 of the producer
 *                                                      (asr.py:36-37) applied on load
 *   2 AFFINE2         a[c]*v + b[c]*v2 + c[c]         BatchNorm backward applied on load       */

/* ---- K2 depthwise -------------------------------------------------------------------------
 * y[b,c,t] = sum_j w[c][flip ? K-1-j : j] * in[b,c, t*stride - pad + j], zero padded, `in` being the
 * transformed (and, for upsample U > 1, zero-stuffed by U) input.
 * Replaces nn.Conv1d(groups=C) of ConvBNActivate, voice100/models/asr.py:31-35,49 (forward) and its
 * autograd backward-data (flip=1, pad=K-1-pad; strided layers: stride=1, upsample=S).
 * out_mode: 0 raw + stats(sum y, sum y^2)   1 clamp(y*out_a+out_b,0,6)  (eval-mode BN+ReLU6 folded)
 *           2 y *= [0 < aux*out_a+out_b < 6] + stats(sum y, sum y*aux) (ReLU6 backward)   3 raw
 * stats: [G][C][2] slab, G = v100_dw_num_groups(B, C). */
int v100_dw_num_groups(int B, int C);
int v100_dwconv(const float* x, const float* x2, const float* w, const float* in_a, const float* in_b,
                const float* in_c, int in_mode, float* y, const float* aux, const float* out_a,
                const float* out_b, int out_mode, float* stats, int G, int B, int C, int Tin, int Tout,
                int K, int stride, int pad, int flip, int upsample, int force_generic, void* stream);

/* dw[c][j] = sum_{b,t} g'[b,c,t] * x'[b,c, t*stride - pad + j]; g' / x' are g / x after g_mode / x_mode.
 * Replaces the weight gradient of the same nn.Conv1d(groups=C).  partial: [G][C][K] workspace. */
int v100_dwconv_wgrad(const float* g, const float* g2, const float* ga, const float* gb, const float* gc,
                      int g_mode, const float* x, const float* xa, const float* xb, int x_mode,
                      float* partial, float* dw, int G, int B, int C, int Tin, int Tout, int K, int stride,
                      int pad, int force_generic, void* stream);

/* Backward of the training-mode depthwise stage of an InvertedResidual in ONE call (autograd of asr.py:49 with the
 * BatchNorm backward of the stage after it applied on load and the ReLU6 / BatchNorm backward sums of the stage
 * before it on the way out):   g' = ga*g + gb*g2 + gc,   xin = relu6(xa*xpre + xb),
 *   dxin[b,c,u] = [0 < xa*xpre+xb < 6] * sum_j w[c][j] * g'[b,c,(u + pad - j)/stride]   -> dxin, stats (sum, sum*xpre)
 *   dw[c][j]    = sum_{b,t} g'[b,c,t] * xin[b,c,t*stride - pad + j]                      -> dw (wpartial: [G][C][K])
 * Tin / Tout are the forward conv's input / output lengths.  Stride 1 with a specialised K runs as one fused kernel
 * (the window walk of the data gradient also accumulates the weight gradient); other shapes, or force_split != 0,
 * run v100_dwconv_wgrad + v100_dwconv. */
int v100_dwconv_bwd(const float* g, const float* g2, const float* w, const float* ga, const float* gb,
                    const float* gc, const float* xpre, const float* xa, const float* xb, float* dxin,
                    float* stats, float* wpartial, float* dw, int G, int B, int C, int Tin, int Tout, int K,
                    int stride, int pad, int force_split, void* stream);

/* ---- K1 pointwise (1x1 conv as GEMM on MFMA) ----------------------------------------------
 * Y[b][m][t] = epilogue( sum_k A[m][k] * x'[b][k][t] (+ bias[m]) )
 * Replaces nn.Conv1d(kernel_size=1): asr.py:47 (pw), :51 (pw-linear), :91 (LinearCharDecoder),
 * tts.py:26,77 (heads); with A = W^T it is their backward-data.
 * epi_mode: 0 store   1 store + stats(sum, sum^2)   2 clamp(y*ea+eb,0,6)   3 y*ea+eb (+R)
 *           4 y *= [0 < R*ea+eb < 6] + stats(sum y, sum y*R)   5 y + R
 * stats: [v100_pw_num_parts(B,T)][M][2].  use_bf16: 1 = operands rounded to bf16 (A_bf16 = bf16 copy of A), fp32
 * accumulate; 2 = IEEE fp16 operands (A_bf16 = fp16 copy, v100_weight_prep_f16), inference combinations only
 * (x_mode 0 with epi_mode 0 / 2 / 3, anything else returns the shape status); 0 = exact fp32 MFMA. */
int v100_pw_num_parts(int B, int T);
int v100_pw_gemm(const float* A, const void* A_bf16, const float* X, const float* X2, const float* xa,
                 const float* xb, const float* xc, int x_mode, float* Y, const float* bias, const float* ea,
                 const float* eb, const float* R, int epi_mode, float* stats, int B, int M, int K, int T,
                 int use_bf16, void* stream);
/* The data gradient of Dropout(p) -> Conv1d(k=1) (asr.py:85-94) in one kernel: Y[b][m][t] = keep[b][m][t] ? (sum_k A[m][k] X[b][k][t]) / (1 - p) : 0
 * with keep the byte mask v100_dropout_fwd wrote.  The small-K form only (K <= 32: the vocabulary head's 29 classes; M >= 64, T % 4 == 0):
 * v100_pw_gemm_dropmask_supported tells, anything else returns the shape status.  use_bf16 as v100_pw_gemm (0 / 1). */
int v100_pw_gemm_dropmask_supported(int B, int M, int K, int T, int use_bf16);
int v100_pw_gemm_dropmask(const float* A, const void* A_bf16, const float* X, float* Y, const void* keep, float p, int B, int M, int K,
                          int T, int use_bf16, void* stream);

/* dW[m][k] = sum_{b,t} g'[b][m][t] * x'[b][k][t]   (weight gradient of the same 1x1 conv).
 * partial: [S][M][K] workspace, S = v100_pw_wgrad_splits(B, M, K): S <= B splits the batch, S = B * TS (small weight matrices)
 * also cuts every utterance's t range into TS chunks. */
int v100_pw_wgrad_splits(int B, int M, int K);
int v100_pw_wgrad(const float* G, const float* G2, const float* ga, const float* gb, const float* gc, int g_mode,
                  const float* X, const float* xa, const float* xb, int x_mode, float* partial, float* dW,
                  int S, int B, int M, int K, int T, int use_bf16, void* stream);

/* fp32 [rows][cols] weight -> optional bf16 copy, transposed fp32 copy, transposed bf16 copy. */
int v100_weight_prep(const float* w, int rows, int cols, void* w_bf16, float* wt, void* wt_bf16, void* stream);
/* w16[i] = IEEE half(w[i]): the weight copy of the fp16 inference precision (use_bf16 = 2 below) */
int v100_weight_prep_f16(const float* w, int rows, int cols, void* w16, void* stream);

/* ---- K3 BatchNorm1d (asr.py:36,52; eps 1e-5, momentum 0.1) ----------------------------------
 * finalize_train: slab of (sum x, sum x^2) -> scale = gamma*rstd, shift = beta - mean*scale, saved
 * mean/rstd, running stats (unbiased variance) and num_batches_tracked updated in place. */
int v100_bn_finalize_train(const float* stats, int parts, long long count, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, long long* num_batches_tracked, float momentum,
                           float eps, float* scale, float* shift, float* save_mean, float* save_rstd, int C, void* stream);
/* eval: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean*scale */
int v100_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                        float eps, float* scale, float* shift, int C, void* stream);
/* backward: slab of (sum dz, sum dz*a) -> da = p*dz + q*a + r coefficients, dgamma, dbeta */
int v100_bn_bwd_finalize(const float* partial, int parts, long long count, const float* gamma, const float* mean,
                         const float* rstd, float* p, float* q, float* r, float* dgamma, float* dbeta, int C, void* stream);
/* FROZEN statistics under autograd (a block in eval() inside a training model: nn.BatchNorm1d normalises with the running statistics
 * and back-propagates through that fixed affine, asr.py:36,52 in eval mode): frozen_coeffs = eval_coeffs plus (mean, rstd) = (running_mean,
 * 1 / sqrt(running_var + eps)) for the backward; bwd_finalize_frozen: p = gamma * rstd, q = r = 0, dgamma / dbeta as in training. */
int v100_bn_frozen_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                          float eps, float* scale, float* shift, float* mean, float* rstd, int C, void* stream);
int v100_bn_bwd_finalize_frozen(const float* partial, int parts, long long count, const float* gamma, const float* mean,
                                const float* rstd, float* p, float* q, float* r, float* dgamma, float* dbeta, int C, void* stream);

/* ---- per-channel elementwise / layout glue --------------------------------------------------*/
/* partial[g][c] = (sum u, sum u*v) over (b in group g, t); v NULL -> sum u*u */
int v100_chan_reduce2(const float* u, const float* v, float* partial, int G, int B, int C, int T, void* stream);
int v100_slab_sum0(const float* partial, int parts, float* out, int C, void* stream);
/* out = A[c]*u + Bc[c]*v + Cc[c]  (block output y = BN3(a3) + x, asr.py:55-59; BN3 backward) */
int v100_chan_affine2(const float* u, const float* v, const float* A, const float* Bc, const float* Cc, float* out,
                      int B, int C, int T, void* stream);
/* out = u*m*s  (nn.Dropout(0.2) with a pre-drawn keep mask, asr.py:90) */
int v100_mul_scale(const float* u, const float* m, float s, float* out, long long n, void* stream);
/* nn.Dropout(p), training mode (asr.py:90), one pass: element i is kept when a 32-bit uniform mixed from (seed, i) is >= p * 2^32;
 * y = keep ? x / (1 - p) : 0, mask[i] = keep (one byte per element, for v100_dropout_bwd: dx = mask ? dy / (1 - p) : 0).
 * Tensor storage must be 16-byte aligned (float4 path); n elements. */
int v100_dropout_fwd(const float* x, long long seed, float p, float* y, void* mask, long long n, void* stream);
int v100_dropout_bwd(const float* dy, const void* mask, float p, float* dx, long long n, void* stream);
/* [B][R][Cc] -> [B][Cc][R]  (torch.transpose(x,1,2) at the model edges, asr.py:111,114; tts.py:177,179) */
int v100_transpose_last2(const float* in, float* out, int B, int R, int Cc, void* stream);
/* out[b][c][t] = table[idx[b][t]][c]  (nn.Embedding + transpose, tts.py:81-83,176-177) and its backward */
int v100_embedding_bct(const long long* idx, const float* table, float* out, int B, int V, int C, int T, void* stream);
int v100_embedding_bwd(const long long* idx, const float* g, float* dtable, int B, int V, int C, int T, void* stream);


/* ---- K8 log-mel batch augmentation ---------------------------------------------------------
 * All of BatchSpectrogramAugumentation.forward (voice100/audio.py:27-108) in one pass over
 * x [B][Tin][F] -> y [B][Tout][F]; the random decisions are drawn by the caller in the reference's
 * order and passed as numbers (0 / 0.f = that op is off).  tm_s / tm_e / tm_a are HOST arrays of
 * n_tmask (<= 3) normalised [start, end) time spans and fill values; len = int32 lengths after the
 * stretch (device).  mix: 1 = mixaudio, 0 = maskaudio (one of the two always runs, audio.py:46-49). */
int v100_augment_fused(const float* x, const int* len, const float* uniform, float* y, int B, int Tin, int Tout,
                       int F, int stretch_rate, float pitch_rate, float amp, int n_tmask, const int* tm_s,
                       const int* tm_e, const float* tm_a, int fm_on, int fm_s, int fm_e, float fm_a, int noise_on,
                       float noise_low, float noise_high, float noise_std, int mix, float log_offset, void* stream);
/* The same pass fed the lengths BEFORE the stretch (len_raw, int32, device): it derives len * stretch_rate / 100 (audio.py:58)
 * itself and also writes it to len_out [B] and (len_out + 1) / 2 -- ConvVoiceEncoder.output_length, asr.py:80-81 -- to half_out [B]
 * (either may be null): the integer tensor ops of a training step folded into the pass that reads the lengths anyway. */
int v100_augment_fused_len(const float* x, const int* len_raw, int* len_out, int* half_out, const float* uniform, float* y,
                           int B, int Tin, int Tout, int F, int stretch_rate, float pitch_rate, float amp, int n_tmask,
                           const int* tm_s, const int* tm_e, const float* tm_a, int fm_on, int fm_s, int fm_e, float fm_a,
                           int noise_on, float noise_low, float noise_high, float noise_std, int mix, float log_offset,
                           void* stream);
/* ... and, for F == 64, the same values TRANSPOSED into yt [B, 64, Tout] by the same pass (null: not written): the layout the encoder
 * takes (torch.transpose(audio, 1, 2), asr.py:111), which otherwise costs a launch that reads y back. */
int v100_augment_fused_len_t(const float* x, const int* len_raw, int* len_out, int* half_out, const float* uniform, float* y,
                             float* yt, int B, int Tin, int Tout, int F, int stretch_rate, float pitch_rate, float amp, int n_tmask,
                             const int* tm_s, const int* tm_e, const float* tm_a, int fm_on, int fm_s, int fm_e, float fm_a,
                             int noise_on, float noise_low, float noise_high, float noise_std, int mix, float log_offset,
                             void* stream);

/* ---- K4 / K7 / K9 glue (csrc/features.hip) -------------------------------------------------
 * shift_copy: out[b][out_coff+c][u*out_mul+out_add] (=|+=) in[b][in_coff+c][u*in_mul+in_add] (0 when that
 * index is out of range) + bias[c], u in [0,n).  Builds the tap-stacked GEMM operand of
 * nn.ConvTranspose1d(512,256,k=5,stride=2,padding=2) (voice100/models/tts.py:22), interleaves its even/odd
 * output phases, and the inverse moves for its backward. */
int v100_shift_copy(const float* in, float* out, const float* bias, int B, int C, int Tin, int Tout, int in_ctot,
                    int in_coff, int out_ctot, int out_coff, int in_mul, int in_add, int out_mul, int out_add, int n,
                    int accumulate, void* stream);
/* frames[b][n][t] = x[b][reflect(t*hop + n + (n_fft-win)/2 - n_fft/2)]: torchaudio Spectrogram(center=True,
 * pad_mode="reflect") framing used by MelSpectrogramAudioTransform, voice100/data_modules.py:276-281 */
int v100_stft_frames(const float* x, float* frames, int B, int N, int T, int hop, int win, int n_fft, void* stream);
/* pw[b][f][t] = spec[b][f][t]^2 + spec[b][F+f][t]^2 */
int v100_power_spectrum(const float* spec, float* pw, int B, int F, int T, void* stream);
/* out[b][t][c] = log(in[b][c][t] + offset)   (data_modules.py:290-291) */
int v100_log_transpose(const float* in, float* out, int B, int C, int T, float offset, void* stream);
/* The whole of MelSpectrogramAudioTransform.forward's arithmetic (voice100/data_modules.py:276-291) in ONE launch: x [B][N] waveform ->
 * out [B][T][n_mels] = log(mel + log_offset), T = 1 + N / hop, torchaudio-0.13.1 MelSpectrogram defaults (center, reflect padding,
 * power 2).  One wave per frame: windowed load, 256-point complex radix-4 FFT of the 512 real samples, real-input split, power,
 * triangular filters, log (csrc/mel.hip).  n_fft = 512 and n_mels <= 64 only (the reference's configuration; 1 otherwise -- the
 * caller then uses the framing / DFT-GEMM / filterbank-GEMM kernels above).  Tables (device, built by the caller in double):
 * window [512] (the win_length Hann window centred in n_fft zeros), tw256 [256][2] / tw512 [257][2] = (cos, -sin)(2 pi k / 256 | 512),
 * mel_start / mel_count [n_mels] = first bin and number of bins (<= 32) of each filter, mel_w [n_mels][32] its weights. */
int v100_log_mel_fused(const float* x, float* out, const float* window, const float* tw256, const float* tw512, const int* mel_start,
                       const int* mel_count, const float* mel_w, int B, int N, int T, int hop, int n_fft, int n_mels, float log_offset,
                       void* stream);
/* K21: the same kernel body over a batch of utterances of different lengths, padded as the reference's collate pads
 * (generate_audio_text_batch, data_modules.py:446-455: each utterance transformed alone, then pad_sequence with log(1e-6)).
 * x [B][N] fp32, lengths [B] int32 on the device (entries are clamped to [0, N]); with n = lengths[b] and
 * T_b = n > n_fft / 2 ? 1 + n / hop : 0, frames t < T_b of out [B][T][n_mels] are those of v100_log_mel_fused on x[b][0 .. n) alone,
 * bit for bit (the reflection is taken at n), frames t >= T_b hold `fill` (the caller passes (float)log(log_offset), what
 * pad_sequence writes; no device logf), and out_len[b] = T_b (int32, device).  x[b][i] is never read for i >= n.  T may be
 * smaller than 1 + N / hop (the caller knows the longest utterance: T = 1 + max(lengths) / hop); frames t >= T are not written,
 * out_len[b] is T_b all the same.  Status as v100_log_mel_fused, plus 3 on a NULL lengths or out_len. */
int v100_log_mel_fused_len(const float* x, const int* lengths, float* out, int* out_len, const float* window, const float* tw256,
                           const float* tw512, const int* mel_start, const int* mel_count, const float* mel_w, int B, int N, int T,
                           int hop, int n_fft, int n_mels, float log_offset, float fill, void* stream);
/* AlignTextToAudioModel.predict epilogue (tts.py:197-200, _layers_v1.py:132-138): x [B][T][2+S+Cap] ->
 * f0 = gate(x0 < 0 ? 0 : x1*std+mean), logspc, codeap un-normalised */
int v100_world_unnormalize(const float* x, float* f0, float* logspc, float* codeap, const float* f0_mean, const float* f0_std,
                           const float* ls_mean, const float* ls_std, const float* ca_mean, const float* ca_std,
                           int B, int T, int S, int Cap, void* stream);
/* ---- K12 WORLDLoss, value + gradient in one pass (voice100/models/_layers_v1.py:37-93), with the target preparation of
 * AlignTextToAudioModel._calc_batch_loss (voice100/models/tts.py:203-206: hasf0 = f0 >= 30, WORLDNorm.normalize) --------
 * pred [B][Tp][A], A = 2 + S + Cap: the decoder output as is (hasf0 logit, f0_hat, logspc_hat[S], codeap_hat[Cap] per frame).
 * Targets f0 [B][Tt], logspc [B][Tt][S], codeap [B][Tt][Cap], length [B] int32; frames t < min(Tp, Tt) count
 * (adjust_size, _layers_v1.py:27-34) and of those t < length[b] (generate_padding_mask, :14-24).
 * f0_mean .. ca_std: the six WORLDNorm vectors (then the targets are RAW and hasf0 may be NULL = raw f0 >= 30), or all NULL
 * (targets already normalised; hasf0 [B][Tt] required).  w: [S] logspc weights (use_mel_weights) or NULL = mean over S.
 * l1: 0 squared error, 1 absolute error.  Writes loss[4] = (hasf0, f0, logspc, codeap) terms, each sum / sum(mask), and
 * unit [B][Tp][A] = d loss_term(a) / d pred for a unit upstream gradient.  partial: v100_world_loss_parts(B, Tp) x 4 floats. */
int v100_world_loss_parts(int B, int Tp);
int v100_world_loss(const float* pred, const float* f0, const float* hasf0, const float* logspc, const float* codeap,
                    const int* length, const float* f0_mean, const float* f0_std, const float* ls_mean, const float* ls_std,
                    const float* ca_mean, const float* ca_std, const float* w, float* partial, float* loss, float* unit,
                    int B, int Tp, int Tt, int S, int Cap, int l1, void* stream);
/* dpred[b][t][a] = unit[b][t][a] * gout[term(a)], gout [4] on the device */
int v100_world_loss_bwd(const float* unit, const float* gout, float* dpred, int B, int Tp, int S, int Cap, void* stream);
/* y = max(exp(x) - offset, 0)   (WORLDVocoder.decode, voice100/vocoder.py:99) */
int v100_exp_clip(const float* x, float* y, float offset, long long n, void* stream);

/* ---- WORLD synthesis (csrc/world.hip; SURVEY.md 8f rank 4, first half) -- PARITY PARTIALLY PINNED ----
 * pyworld.decode_aperiodicity + pyworld.synthesize as WORLDVocoder.decode calls them (voice100/vocoder.py:100-101).
 * pyworld 0.3.2 (C++ WORLD) is not in the reference tree: the kernels follow the published algorithm as restated in
 * oracle/world_synth.py.  fft_size 512 (16 kHz): one WAVE per pulse, fp32 with the tables below; any other power of two up to 2048 (1024:
 * the 22.05 kHz models): one workgroup per pulse in fp64, tw256 / tw512 / dc_remover may be NULL.
 *   v100_world_randn_host    HOST function, HOST pointer: the first n values of WORLD's randn() after randn_reseed() (every
 *                            Synthesis call reseeds: one fixed sequence for all utterances; callers upload it once)
 *   v100_world_decode_aperiodicity   coded [rows][nb] dB -> ap [rows][fft_size/2+1]
 *   v100_world_synthesize    f0 [B][T], sp / ap [B][T][257] -- or, instead of ap (then NULL), coded_ap [B][T][nb] in dB, decoded per
 *                            pulse without ever rounding an aperiodicity near 1 to fp32 (the reference decodes in double) --,
 *                            frames [B] int32 (NULL: every utterance has T frames),
 *                            randn_table [table_len >= samples per utterance], tw256 [256][2] / tw512 [257][2] = cos, -sin
 *                            of 2 pi k / 256 and / 512, dc_remover [512] (oracle.world_synth.dc_remover), all built in double
 *                            by the caller -> y [B][Ymax] fp32, Ymax = (int)(T * frame_period_ms * fs / 1000), zero beyond
 *                            an utterance's own length; n_pulses [B] (-1 and a NaN row: more than max_pulses pulses). */
/* ---- channel-major inference layout (round 4; csrc/block.hip v100_ir_fwd_eval with shape[10] == 2) --------------------------
 * Activations [C][B][P], P = v100_row_pitch16(T, B): one [C x (B P)] matrix with every utterance's (padded) row back to back, so a 1x1
 * convolution is ONE GEMM over all B P columns (asr.py:47,51 on 1-second chunks: full 128-column tiles instead of 51 of 128) and a
 * channel's rows are contiguous for the depthwise kernel.  Block inputs / outputs fp32, hidden tensors in the GEMM operand format
 * (bf16, or fp16 at precision "fp16").  v100_bct_to_cm: [B][C][T] fp32 -> [C][B][P] (padding zeroed); v100_cm_to_btc: [C][B][P] ->
 * [B][T][C] (the model-edge transpose of the logits, asr.py:114). */
int v100_bct_to_cm(const float* in, float* out, int B, int C, int T, void* stream);
int v100_cm_to_btc(const float* in, float* out, int B, int C, int T, void* stream);

int v100_world_randn_host(float* host_out, long long n);
int v100_world_decode_aperiodicity(const float* coded, float* ap, long long rows, int nb, int fs, int fft_size, void* stream);
long long v100_world_synth_workspace_bytes(int B, int T, int fs, double frame_period_ms, int fft_size, int max_pulses);
int v100_world_synthesize(const float* f0, const float* sp, const float* ap, const float* coded_ap, int nb, const int* frames, const float* randn_table,
                          long long table_len, const float* tw256, const float* tw512, const float* dc_remover, float* y,
                          int* n_pulses, void* workspace, int B, int T, int fs, double frame_period_ms, int fft_size,
                          int max_pulses, void* stream);

/* ---- K11 dense k-tap conv blocks of the v2 models (csrc/layernorm.hip) -------------------
 * ConvLayerBlock / ConvTransposeLayerBlock, voice100/models/_layers_v2.py:29-89: conv -> LayerNorm over channels
 * -> exact GELU.  The dense convolution runs on the K1 GEMM over an im2col copy (rows tap-major: j*Cin + c);
 * col2im is its adjoint (backward-data), a gather.  ln_gelu_fwd: out = gelu(layer_norm_C(y) * gamma + beta) on
 * [B][C][T] (C <= 1024), saving mean / rstd [B][T]; ln_gelu_bwd: dy plus per-tile partial sums
 * partial[v100_ln_num_parts(B,T)][C][2] = (dgamma, dbeta), summed over parts by v100_slab_sum2. */
int v100_im2col(const float* x, float* cols, int B, int Cin, int Tin, int Tout, int k, int stride, int pad, void* stream);
int v100_col2im(const float* dcols, float* dx, int B, int Cin, int Tin, int Tout, int k, int stride, int pad, void* stream);
/* Stride-1 dense convolutions and the two output phases of ConvTranspose1d(k5,s2,p2) WITHOUT the im2col copy
 * (csrc/pointwise*.hip, "tap-addressed X"): the GEMM's contraction index is k = tap*cx + c and row k is row c of a
 * zero-padded copy Xp [B][cx][Tx] of the input, read from column t + shifts[tap] (0 <= shift <= 15, T + shift <= Tx):
 *   Y[b][m][t]        = sum_{tap,c} A[m][tap*cx + c] * Xp[b][c][t + shifts[tap]]  (+ bias[m]) (+ R[b][m][t], bf16/fp32 only)
 *   dW[m][tap*cx + c] = sum_{b,t<T} G[b][m*Tg + g_off + t] * Xp[b][c][t + shifts[tap]]      (G rows of pitch Tg)
 * nn.Conv1d(Cin,Cout,k,padding=(k-1)/2) forward: Xp = pad(x, (k-1)/2), shifts = 0..k-1, A[m][j*Cin+c] = W[m][c][j];
 * its backward-data is the same GEMM on pad(dy) with the taps reversed.  `shifts` is a HOST array of ntap (<= 8) ints.
 * v100_pad_copy: dst[b][c][lpad + i] = src[b][c][src_off + i*src_step], i < n, zero elsewhere in the Tx-long row
 * (src_step 2 splits a ConvTranspose gradient into its even / odd phases).  v100_pw_taps_supported = 1 when the two
 * GEMM entry points accept the shape at that precision (bf16/fp16 need cx % 64 == 0); otherwise use im2col. */
int v100_pad_copy(const float* src, float* dst, int B, int C, int Tsrc, int src_step, int src_off, int n, int Tx, int lpad, void* stream);
int v100_pw_taps_supported(int B, int M, int cx, int ntap, int T, int Tx, int use_bf16);
int v100_pw_gemm_taps(const float* A, const void* A_bf16, const float* Xp, float* Y, const float* bias, const float* R,
                      int B, int M, int cx, int T, int Tx, int ntap, const int* shifts, int use_bf16, void* stream);
int v100_pw_wgrad_taps(const float* G, int Tg, int g_off, const float* Xp, float* partial, float* dW, int S, int B, int M,
                       int cx, int T, int Tx, int ntap, const int* shifts, int use_bf16, void* stream);
int v100_ln_num_parts(int B, int T);
int v100_slab_sum2(const float* partial, int parts, float* out0, float* out1, int C, void* stream);
int v100_ln_gelu_fwd(const float* y, const float* gamma, const float* beta, float eps, float* out, float* mean,
                     float* rstd, int B, int C, int T, void* stream);
int v100_ln_gelu_bwd(const float* dout, const float* y, const float* gamma, const float* beta, const float* mean,
                     const float* rstd, float* dy, float* partial, int B, int C, int T, void* stream);

/* ---- opt-in kernel timing (bench.py roofline): HIP events on the launch stream for the hot kernels (tags 0-4) and, with tag 5
 * ("other"), in the dispatch packet of every other launch of the library (roofline_step.kernel_ms).
 * tags: 0 depthwise fwd, 1 depthwise bwd, 2 depthwise bwd-weight (stand-alone), 3 pointwise GEMM, 4 pointwise bwd-weight.
 * The depthwise launches are timed with the dispatch packet's own start/stop timestamps (hipExtLaunchKernelGGL: no
 * marker packets, the pair reads what rocprofv3 reports as the kernel's duration); the GEMM tags bracket their launches
 * with hipEventRecord (~3 us of queue time per launch, so time only what is read).
 * enable(mask): bit t of mask switches tag t on (0 = all off); a non-zero mask clears the counters.  read()
 * synchronises the device and returns the summed ms, launch count and (for the depthwise tags) the algorithmic bytes
 * of those launches: fp32 in + out + taps + BN coefficients. */
/* kernel launches issued by the library in this process so far (bench.py: launches per step measured in the run itself) */
long long v100_launch_count(void);
/* dst = src, nbytes (a multiple of 16) in 16-byte pieces: the device-copy yardstick bench.py reports beside the HBM-bound
 * kernels' GB/s ("fraction of both nominal and measured-copy bandwidth") */
int v100_copy_probe(const void* src, void* dst, long long nbytes, void* stream);
int v100_timing_enable(int tag_mask);
int v100_timing_read(int tag, double* ms, long long* count, double* bytes);
/* The depthwise streaming kernels' access pattern as a pure copy (bench.py yardstick only): dst[b][c][:] = src[b][c][:] for
 * row_bytes-byte rows of a [B][C][row_bytes] tensor, one workgroup per channel, one row per wave at a time, nontemporal.
 * row_bytes % 1024 == 0. */
int v100_rows_copy_probe(const void* src, void* dst, int B, int C, int row_bytes, void* stream);

/* ---- "act16": bf16 STORAGE of the big hidden tensors in bf16-operand training (csrc/block.hip) ---------------
 * In bf16 mode the reference under autocast keeps its conv activations in bf16; here the two tensors a block saves for
 * backward (a1 = expand output, a2 = depthwise output, each 4x the block's width) and optionally the two hidden gradients
 * (act16 level 2; level 3 adds the project output a3, saved for backward, and its gradient da3; level 4 a bf16 shadow of the block
 * output for the next block's X operand, v100_chan_affine2_shadow) are stored as bf16 [B][C][P], P = v100_row_pitch16(T, B) (pitched rows: every 4- / 8-sample access stays 8 / 16-byte aligned for any
 * T).  Callers must size every such tensor with v100_row_pitch16: the kernels address rows by it, and a tensor sized by another
 * rule is written out of bounds.  Accumulators, BatchNorm statistics and reductions stay fp32.  io16 masks select which operands are such tensors:
 *   v100_pw_gemm_io:   1 X, 2 X2, 4 Y, 8 R        v100_pw_wgrad_io: 1 G, 2 G2, 4 X
 *   v100_dwconv_*_io:  1 x (first stream), 2 x2, 4 aux (a1), 8 y; 16 = the tensors are CHANNEL-MAJOR [C][B][P] (rows of up to 768
 *                      outputs; the layout probe of round 4: tools/bench_dw_regimes.py --cm, tests/test_gpu_act16.py)
 * Same arithmetic as v100_pw_gemm / v100_pw_wgrad / v100_dwconv / v100_dwconv_bwd (bf16 operands); only the combinations the
 * block executor issues exist, anything else returns 1 (no fallback). */
int v100_pw_gemm_io(const void* A_bf16, const void* X, const void* X2, const float* xa, const float* xb, const float* xc,
                    int x_mode, void* Y, const float* ea, const float* eb, const void* R, int epi_mode, float* stats,
                    int B, int M, int K, int T, int io16, void* stream);
int v100_pw_wgrad_io(const void* G, const void* G2, const float* ga, const float* gb, const float* gc, int g_mode,
                     const void* X, const float* xa, const float* xb, int x_mode, float* partial, float* dW, int S, int B,
                     int M, int K, int T, int io16, void* stream);
/* Several such weight gradients in ONE launch (csrc/wgrad_group.h, csrc/pointwise_bf16_group.hip), each workgroup carrying one
 * tile through the whole contraction: no split-K slabs, no reduce launch.  The workgroup walks the contraction in the order of the S
 * splits of v100_pw_wgrad_io and sums their partial tiles in slab order, so every dW equals v100_pw_wgrad_io(..., S, ...) bit for bit.
 * Only the two finished-gradient forms of the InvertedResidual backward (asr.py:45-59; csrc/block.hip v100_ir_stack_bwd): g_mode 0,
 * io16 = 1 | 4, x_mode 1 (project) or 0 (expand on da1), any S that takes.
 * A TIER is a tile shape with its kernel; the two tiers share eligibility, placement and launch, and differ in nothing else.
 * The wide tier (these three; csrc/pointwise_bf16_wgrad_group.h): project M % 256 == 0, K % 128 == 0; expand M % 128 == 0, K % 256 == 0.
 * n <= 16 problems; ptrs (HOST, 5 per problem): G X xa xb dW; dims (HOST, 8 per problem): B M K T S g_mode x_mode io16.
 * Status: 3 for NULL tables, 1 for n outside 1..16, then per problem 3 for a NULL operand before 1 for one that does not qualify.
 * _supported: 1 when a problem qualifies; _tiles: its workgroups (0: not whole tiles). */
int v100_pw_wgrad_group_supported(int B, int M, int K, int T, int S, int g_mode, int x_mode, int io16);
int v100_pw_wgrad_group_tiles(int M, int K, int x_mode);
int v100_pw_wgrad_group(int n, const void* const* ptrs, const int* dims, void* stream);
/* The small tier (csrc/pointwise_bf16_wgrad_small.h): 128 x 128 tiles, for gradients with too few of the tiles above to fill the
 * chip (256 x 1024: 8 of those, 16 of these): both x_modes with M % 128 == 0 and K % 128 == 0, same tables, status and bit-identity. */
int v100_pw_wgrad_group_small_supported(int B, int M, int K, int T, int S, int g_mode, int x_mode, int io16);
int v100_pw_wgrad_group_small_tiles(int M, int K, int x_mode);
int v100_pw_wgrad_group_small(int n, const void* const* ptrs, const int* dims, void* stream);
int v100_dw_mfma_supported(int K, int stride);
/* Row pitch, in elements, of every 16-bit-stored activation tensor [B][C][P] the _io entry points address: a multiple of 8 (16-byte
 * rows); for B > 1 and T >= 256 a multiple of 64 (rows start on 128-byte lines: a time-stretched 1136-byte row otherwise shares its
 * boundary lines with its neighbours and they are fetched twice).  The ONE rule (csrc/common.h v100_pitch16): callers allocate with it. */
int v100_row_pitch16(int T, int B);
int v100_dwconv_fwd_train_io(const void* a1, const float* w, const float* in_a, const float* in_b, void* a2, float* stats,
                             int G, int B, int C, int T, int K, int io16, void* stream);
int v100_dwconv_bwd_io(const void* g, const void* g2, const float* w, const float* ga, const float* gb, const float* gc,
                       const void* xpre, const float* xa, const float* xb, void* dxin, float* stats, float* wpartial,
                       float* dw, int G, int B, int C, int T, int K, int io16, void* stream);
/* v100_dwconv_bwd_io with every tensor bf16-stored, ONE group, finishing BatchNorm 1's backward itself: the kernel owns the channel's
 * sums (stats [C][2] = sum dz1, sum dz1*a1) after its last row, forms (p, q, r) -> pqr [3][C] and (dgamma, dbeta) from the saved mean /
 * rstd / gamma of BatchNorm 1 and writes the FINISHED gradient da1 = p*dz1 + q*a1 + r (bf16, rounded once) where v100_dwconv_bwd_io
 * writes dz1 -- the operand the expand weight gradient and the expand backward-data GEMM consume (autograd of asr.py:45-49).
 * B <= 32, T <= 512, specialised K only; 1 otherwise (no fallback). */
int v100_dwconv_bwd_da1_io(const void* g, const void* g2, const float* w, const float* ga, const float* gb, const float* gc,
                           const void* xpre, const float* xa, const float* xb, void* da1_out, float* stats, float* dw,
                           const float* bn1_gamma, const float* bn1_mean, const float* bn1_rstd, float* pqr, float* dgamma,
                           float* dbeta, int B, int C, int T, int K, void* stream);
/* The eval-mode depthwise stage on 16-bit hidden tensors (inference at precision "bf16" / "fp16"), as the block executor issues it --
 * exposed for the kernel tests (tests/test_gpu_eval_dw_oracle.py):
 *   h2[b][c][t] = round16(relu6(fmaf(sum_j h1[b][c][t - (K-1)/2 + j] * q(w[c][j]), out_a[c], out_b[c]))),  t < T, zeros outside [0, T)
 * with fp32 accumulation; q = ONE rounding of the fp32 tap to the storage format (bf16; all 24 bits with V100_DW_DIGITS=3, which
 * the fp16 form does not read).  flags: 1 = channel-major, 2 = fp16 (else bf16).
 * Operands: h1 and h2 are [B][C][P], or [C][B][P] when channel-major, P = v100_row_pitch16(T, B); w [C][K] and out_a / out_b [C] fp32
 * (the folded BatchNorm 2).  The pitch padding [T, P) of a row:
 *   h1: the 8-sample run that straddles T is LOADED whole (elements [T, (T + 7) & ~7) are read), and every element at or past T is
 *       replaced by zero before it is used: the result does not depend on the padding's bits (NaN included).  The producing GEMM
 *       makes no promise about them either: batch-major (epilogue 2, 16-bit Y) it stores whole 4-sample groups, so
 *       [T, (T + 3) & ~3) of a row holds relu6(fmaf(acc, ea, eb)) of columns that are not part of the tensor and the rest of the
 *       padding is never written; channel-major the whole [C][B P] matrix is ONE GEMM and the padding columns are ordinary
 *       output columns (relu6 of whatever their X columns held).
 *   h2: stored in whole 4-sample groups: [T, (T + 3) & ~3) is overwritten with values that are NOT part of the result (the window
 *       at those positions still reaches real samples) -- finite for finite operands --; [(T + 3) & ~3, P) is not written.
 * K: odd and one of the specialised sizes (v100_dw_mfma_supported).  T <= 768: the streaming kernel, both layouts and formats;
 * longer rows: the general kernel, bf16 and [B][C][P] only.  Anything else returns 1, NULL operands 3 (no fallback). */
int v100_dwconv_fwd_eval_io(const void* h1, const float* w, const float* out_a, const float* out_b, void* h2, int B, int C, int T,
                            int K, int flags, void* stream);
/* the two block-boundary passes with a bf16-stored operand: io16 of v100_chan_reduce2_io: 2 = v is bf16 (sums of dy, dy*a3);
 * of v100_chan_affine2_io: 1 = u is bf16 (y = s3*a3 + t3 (+ x)), 6 = v and out are bf16 (da3 = p*dy + q*a3 + r) */
int v100_chan_reduce2_io(const void* u, const void* v, float* partial, int G, int B, int C, int T, int io16, void* stream);
/* the forward block output (asr.py:55-59) with a bf16 shadow beside it (act16 level 4): out = A*u + Cc (+ v) as fp32 [B][C][T] AND
 * rounded to bf16 in shadow [B][C][v100_row_pitch16(T, B)]; u is bf16 (pitched) when u_bf16, else fp32.  The shadow is what the NEXT block's
 * expand GEMM / expand weight gradient read as X (io16 bit PW_IO_X / WG_IO_X): same results, half the operand bytes. */
int v100_chan_affine2_shadow(const void* u, const float* v, const float* A, const float* Cc, float* out, void* shadow,
                             int B, int C, int T, int u_bf16, void* stream);
int v100_chan_affine2_io(const void* u, const void* v, const float* A, const float* Bc, const float* Cc, void* out,
                         int B, int C, int T, int io16, void* stream);
/* 1 when v100_ir_fwd_train / v100_ir_bwd accept shape[10] (act16) != 0 for this block */
int v100_ir_act16_supported(const int* shape);

/* ---- Adam step of every parameter in one launch (torch.optim.Adam as configured by asr.py:169-176 / tts.py:132-135, 239-241:
 * grad += weight_decay * p; m = lerp(m, grad, 1-beta1); v = beta2*v + (1-beta2)*grad^2; p -= lr/(1-beta1^step) * m /
 * (sqrt(v)/sqrt(1-beta2^step) + eps)).  chunks: DEVICE array of nchunks records {int tensor; int count; long long offset}
 * (count <= v100_adam_chunk_elems() elements of one tensor each); params / grads / exp_avg / exp_avg_sq: DEVICE arrays of float
 * pointers indexed by tensor.  Hyper-parameters are doubles: 1 - beta is formed in double, as torch does (1.f - 0.999f is 1.3e-5 off). */
int v100_adam_chunk_elems(void);
int v100_adam_step(const void* chunks, int nchunks, const void* params, const void* grads, const void* exp_avg,
                   const void* exp_avg_sq, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                   void* stream);

/* ---- gradient clipping (torch.nn.utils.clip_grad_norm_ / clip_grad_value_; Lightning's gradient_clip_val), on the chunk table and
 * gradient-pointer table of v100_adam_step.
 * norm_type: 2 = Euclidean norm, -1 = infinity norm (max |g|, NaN propagated).  clip_mode: 1 = norm, 2 = value.
 * partials: DEVICE array of doubles, one per chunk: the sum of squares of the chunk's gradient elements (fp32 within a lane, fp64
 * across lanes) for norm_type 2, max |g| for -1.  A norm that spans several chunk tables (param groups) gives each table its own range
 * at a fixed offset of one buffer and passes the whole buffer (npartials entries) to the consuming call.
 * Norm mode (two launches): v100_grad_norm_partials writes partials[0, nchunks); the consuming call (v100_adam_step_clip or v100_grad_clip)
 * reduces partials[0, npartials) in every workgroup in one fixed order to the total norm -- so every workgroup, launch and run agrees bit
 * for bit, with no atomics -- forms coef = min(clip / (total + 1e-6), 1) in fp32 (NaN stays NaN) and scales g by it before anything else
 * reads g; with coef == 1 nothing is written back.  total_norm (DEVICE float, may be NULL) receives the total.
 * Value mode (one launch): g = clamp(g, -clip, clip); partials, npartials, norm_type and total_norm are not read.
 * The clipped gradient is written back through `grads` (what p.grad holds after torch's in-place clip).
 * Return codes: 0 ok; 1 bad nchunks / npartials / norm_type / clip_mode / step; 2 launch error; 3 a required pointer is NULL. */
int v100_grad_norm_partials(const void* chunks, int nchunks, const void* grads, void* partials, int norm_type, void* stream);
/* v100_adam_step on the clipped gradient (the weight-decay term is added after the clip, as torch.optim.Adam does after a clip). */
int v100_adam_step_clip(const void* chunks, int nchunks, const void* params, const void* grads, const void* exp_avg,
                        const void* exp_avg_sq, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                        int clip_mode, double clip, const void* partials, int npartials, int norm_type, void* total_norm, void* stream);
/* the clip alone, in place: grads scaled by the coefficient (norm) or clamped (value); multi-tensor over the chunk table */
int v100_grad_clip(const void* chunks, int nchunks, const void* grads, int clip_mode, double clip, const void* partials, int npartials,
                   int norm_type, void* total_norm, void* stream);

/* ---- K10 log_softmax + CTC (asr.py:148-152: F.log_softmax(-1) then nn.CTCLoss(blank, 'mean', zero_infinity=True)) --
 * logits [B][T][V] fp32, targets [B][Lmax] int64, in_len / tgt_len [B] int32 (device).  Writes nll[b] =
 * -log p(target_b | logits_b) (inf when infeasible; 0 for a row with no frame and no label) and grad[b][t][c] = d nll_b / d logits[b][t][c] (zero for
 * padded frames and infeasible utterances); the caller forms mean_b(nll_b / tgt_len_b) and scales grad.
 * workspace: v100_ctc_workspace_floats(B, T, Lmax) floats.  Limits: V <= 128, Lmax <= 2047
 * (256 threads x up to 16 lattice states each).  Labels outside [0, V) are treated as blank (the host wrapper can validate
 * them first: VOICE100_CHECK_IDS=1). */
int v100_ctc_workspace_floats(int B, int T, int Lmax);
/* v100_ctc_loss plus the 'mean' reduction in the library: loss[0] = mean over b of (nll_b finite ? nll_b / max(tgt_len_b, 1) : 0),
 * grad = d loss[0] / d logits */
int v100_ctc_loss_mean(const float* logits, const long long* targets, const int* in_len, const int* tgt_len, float* workspace,
                       float* nll, float* loss, float* grad, int B, int T, int V, int Lmax, int blank, void* stream);
int v100_ctc_loss(const float* logits, const long long* targets, const int* in_len, const int* tgt_len, float* workspace,
                  float* nll, float* grad, int B, int T, int V, int Lmax, int blank, void* stream);
/* v100_ctc_loss_mean with the gradient laid out [B, V, T] when grad_bvt != 0 (the logits stay [B, T, V]): the layout of the tensor
 * the reference transposes the logits FROM (asr.py:114), so the backward of that transpose needs no pass over the gradient. */
int v100_ctc_loss_mean_t(const float* logits, const long long* targets, const int* in_len, const int* tgt_len, float* workspace,
                         float* nll, float* loss, float* grad, int grad_bvt, int B, int T, int V, int Lmax, int blank, void* stream);
/* Up to 1024 lattice states (Lmax <= 511) the lattice runs as a wave pipeline whose neighbouring waves hand edge states over either
 * once per frame or once per group of frames; a host rule on T and the wave count picks (csrc/ctc.hip), and both give the same bits.
 * v100_ctc_lattice_plan (HOST only, no GPU call): what the rule picks at this shape: -1 not the pipeline, 0 per frame, else the
 * group's frames.  v100_ctc_lattice_ring_frames(): frames a wave of the grouped form can run ahead of its neighbour (lengths beyond
 * it wrap the hand-over ring).  Test hook v100_ctc_lattice_form: force a form process-wide: 0 per frame, 1 grouped, -1 the rule. */
int v100_ctc_lattice_plan(int T, int Lmax);
int v100_ctc_lattice_ring_frames(void);
int v100_ctc_lattice_form(int form);

/* ---- block executor (csrc/block.hip): the whole kernel chain of one InvertedResidual block (asr.py:40-59) per call.
 * shape = {B, Cin, hid, Cout, T, K, stride, residual, bf16, flags, act16} (11 ints; act16: see "act16" above -- then the
 * caller passes a1 / a2 as bf16 [B][hid][v100_row_pitch16(T, B)]); coef = 12 vectors of max(hid, Cout) floats (BN
 * scale/shift/mean/rstd of the three BatchNorms) written by forward and read by backward.  flags = an OR of the three V100_IR_*
 * bits below; every other bit is reserved to the stack executor and must be 0.
 * Pointer tables (device pointers unless noted):
 *  fwd: x | w1 g1 b1 rm1 rv1 nbt1 | wd g2 b2 rm2 rv2 nbt2 | w3 g3 b3 rm3 rv3 nbt3 | a1 a2 a3 y coef workspace prep   (26)
 *       | x16 y16 (28: only with V100_IR_SHADOW_SLOTS; each may be NULL): the bf16 shadow [B][C][v100_row_pitch16(T, B)] of x
 *       (written by the previous block) and of y (for the next block), read at act16 level >= 4
 *  bwd: x a1 a2 a3 | w1 wd w3 | g1 g2 g3 | coef | dy | dx (NULL = skip) | dW1 dg1 db1 dWd dg2 db2 dW3 dg3 db3 | workspace prep (24)
 *       | x16 (25: only with V100_IR_SHADOW_SLOTS; may be NULL) | the block's region for deferred weight gradients (26: read
 *       only with the stack executor's reserved defer bit, never by a caller of this header)
 * prep = v100_ir_prep_bytes(shape) bytes: bf16 / transposed weight copies written by forward (unless V100_IR_PREPPED: the
 * caller has filled it, e.g. with v100_ir_prep_batched for the n <= 32 blocks of a stack in one launch; shapes = n x 11
 * ints) and reused by backward.  `shape(s)` and the tables are HOST arrays. */
enum {
    V100_IR_PREPPED = 1,        /* prep is filled already: forward does not prepare the weights */
    V100_IR_SHADOW_SLOTS = 2,   /* the pointer tables carry the x16 / y16 slots */
    V100_IR_FROZEN = 8          /* BatchNorm normalises with its running statistics and updates nothing (a block in eval() that
                                 * takes part in autograd); act16 must be 0 */
};
long long v100_ir_prep_bytes(const int* shape);
long long v100_ir_fwd_workspace_bytes(const int* shape);
/* eval mode (inference): folded BatchNorm coefficients + bf16 weight copies in a caller-owned cache (refill with
 * v100_ir_eval_prep whenever a parameter or running statistic changes), then 3 launches per block and call.
 * Pointer tables (HOST arrays of device pointers):
 *  prep: w1 | g1 b1 rm1 rv1 | g2 b2 rm2 rv2 | w3 | g3 b3 rm3 rv3 | cache   (15; cache = v100_ir_eval_cache_bytes(shape) bytes)
 *  fwd:  x | w1 wd w3 | cache | h1 h2 y                                    (8)
 * The eval entry points read the nine leading ints of `shape` (v100_ir_eval_cache_bytes may be given no more), ignore the flags, and
 * read shape[10] NOT as the training act16 level but as the layout of the forward's tensors (v100_ir_eval_prep does not read it):
 *  0  x [B,Cin,T], h1 [B,hid,T], h2 [B,hid,T'], y [B,Cout,T'], all fp32; any operand format
 *  1  h1 / h2 bf16 [B][hid][v100_row_pitch16(T, B)], x and y as at 0; bf16 operands and a shape with v100_ir_act16_supported
 *  2  channel-major: x [Cin][B P] fp32, h1 / h2 [hid][B P] in the 16-bit operand format (bf16, or fp16 at bf16 = 2), y [Cout][B P]
 *     fp32, P = v100_row_pitch16(T, B); stride 1, T <= 768, B P <= 0x7fffff00, and a shape whose bf16 twin has v100_ir_act16_supported
 * (any other non-zero value is taken as 1).  A combination outside these rules returns 1 (bad shape). */
long long v100_ir_eval_cache_bytes(const int* shape);
int v100_ir_eval_prep(const int* shape, const void* const* ptrs, void* stream);
int v100_ir_fwd_eval(const int* shape, const void* const* ptrs, void* stream);
/* n eval-mode blocks back to back in ONE host call (inference at the configs' own sizes is bound by the host's per-call cost, not by
 * the GPU): shapes = n x 11 ints, ptrs = n x 8 pointers, each block's in v100_ir_fwd_eval's order (block i's y is block i+1's x:
 * the caller lays the buffers out).  HOST arrays.  Stops at the first block that fails and returns its code. */
int v100_ir_stack_fwd_eval(int n, const int* shapes, const void* const* ptrs, void* stream);
int v100_ir_prep_batched(const int* shapes, const void* const* w1s, const void* const* w3s, void* const* preps, int n, void* stream);
int v100_ir_fwd_train(const int* shape, const void* const* ptrs, void* stream);
long long v100_ir_bwd_workspace_bytes(const int* shape);
int v100_ir_bwd(const int* shape, const void* const* ptrs, void* stream);

/* ---- stack executor: a run of consecutive InvertedResidual blocks (ConvVoiceEncoder.layers, asr.py:67-76; VoiceDecoder.layers[0:4] /
 * [5:8], tts.py:17-25; TextToAlignTextModel.layers[0:4], tts.py:72-76) forward / backward in ONE host call each: the sequencing of
 * v100_ir_prep_batched + v100_ir_fwd_train per block (resp. v100_ir_bwd in reverse), same kernels and results.
 * desc (HOST ints): {n, B, T, bf16, act16_level, want_last_shadow} then n x {cin, hid, cout, k, stride, residual}.
 * v100_ir_stack_plan fills plan (HOST, 8 per block + 6 long longs): per block the byte offsets into the activation blob of
 * a1, a2, a3, y, y16 (-1: none), coef, prep and the block's output length; then {blob_bytes, bwd_ws_bytes, grad_floats, ...}; returns
 * blob_bytes (-1: bad descriptor).  The caller allocates the blob (kept until backward), the backward workspace and the gradient
 * buffer: grad_floats floats, per block dW1 dg1 db1 dWd dg2 db2 dW3 dg3 db3.
 * params (HOST pointer table, 18 per block): w1 g1 b1 rm1 rv1 nbt1 | wd g2 b2 rm2 rv2 nbt2 | w3 g3 b3 rm3 rv3 nbt3.
 * x16 (may be NULL): bf16 shadow [B][cin][v100_row_pitch16(T, B)] of x (act16 level 4). */
long long v100_ir_stack_plan(const int* desc, long long* plan);
int v100_ir_stack_fwd_train(const int* desc, const void* const* params, const void* x, const void* x16, void* blob, void* stream);
int v100_ir_stack_bwd(const int* desc, const void* const* params, const void* x, const void* x16, const void* blob, const void* dy,
                      void* dx, void* grads, void* ws, void* stream);
/* v100_ir_stack_bwd defers the two 1x1 weight gradients (asr.py:47,51: the pw / pw-linear convs) of blocks on the finished-gradient
 * path whose gradients both qualify for v100_pw_wgrad_group with >= min_problem_tiles tiles (32), keeps their operands da3 / da1
 * in per-block regions of the backward workspace and flushes them in one grouped launch once >= min_flush_tiles (192) wait and the
 * next block would not fit the same launch, or in the ordinary per-problem launches when the walk ends with fewer.  Same results.
 * v100_ir_stack_wgrad_plan (HOST only, no GPU call) tells what happens for a descriptor: out = 3 per block {defers, byte offset of
 * the block's region in ws or -1, flush right after this block's backward: tiles (> 0 grouped, < 0 per problem, 0 none)}, then
 * {bwd_ws_bytes, bytes of the shared part in front of the regions}.  have_x16: the caller passes x16 (block 0 defers only then).
 * v100_ir_stack_wgrad_group_thresholds replaces the two defaults process-wide (tests: the grouped path at small shapes); it
 * changes bwd_ws_bytes of v100_ir_stack_plan, so set it before planning. */
int v100_ir_stack_wgrad_plan(const int* desc, int have_x16, int min_problem_tiles, int min_flush_tiles, long long* out);
int v100_ir_stack_wgrad_group_thresholds(int min_problem_tiles, int min_flush_tiles);
/* Tier 2: once such a flush is enqueued its blocks' regions are dead, and a later block of the walk below min_problem_tiles whose
 * gradients qualify for v100_pw_wgrad_group_small parks its da3 / da1 there (first fit; no bytes of its own) and waits for one
 * small-tile launch: where the next block cannot join, at 16 problems, or where the walk ends -- grouped if >= min_flush_small
 * workgroups (96) wait, else per problem.  A stack without a tier-1 flush behaves as before.  v100_ir_stack_wgrad_plan2: the same
 * table for tier 2 ({defers, byte offset of the borrowed region or -1, flush: workgroups}), then the same two totals.
 * v100_ir_stack_wgrad_group2_threshold sets min_flush_small process-wide; 0 turns tier 2 off. */
int v100_ir_stack_wgrad_plan2(const int* desc, int have_x16, int min_problem_tiles, int min_flush_tiles, int min_flush_small, long long* out);
int v100_ir_stack_wgrad_group2_threshold(int min_flush_small);

/* ---- SURVEY 8(f) "next" rows: integer decode / alignment steps on the device (csrc/decode.hip), bit-exact ----
 * greedy CTC decode: argmax per frame (first maximum), collapse repeats, drop blanks (voice100/text.py:99-104);
 * out [B][T] int64 (zero padded), out_len [B]. */
int v100_ctc_greedy_decode(const float* logits, const int* lens, long long* out, int* out_len, int B, int T, int V, int blank, void* stream);
/* ctc_best_path (voice100/models/align.py:18-66) batched: logp [B][T][V] log-probabilities, labels [B][Lmax] int64;
 * back_ws: B*T*(2*Lmax+1) int16; path [B][T] int32 = index into the blank-expanded labels; score [B]. */
int v100_ctc_best_path(const float* logp, const long long* labels, const int* in_len, const int* lab_len, void* back_ws, int* path,
                       float* score, int B, int T, int V, int Lmax, int max_move, void* stream);
/* K20, forced alignment in one launch (csrc/align.hip): the Viterbi of v100_ctc_best_path with everything voice100/align_text.py:39-56
 * writes per utterance.  path [B][T] int32 and score [B] are bit-identical to v100_ctc_best_path; best_labels [B][T] int64 is the
 * blank-extended label at each path position; align [B][2*Lmax+1] int32 is the number of frames the path spends at each extended
 * position (0 beyond 2*lab_len+1); path and best_labels are 0 beyond in_len.  in_len / lab_len may be NULL (T / Lmax everywhere).
 * moves_ws: v100_ctc_align_workspace_bytes(B, T, Lmax) bytes (one byte per frame and state; 0 = unsupported shape).
 * T <= 12000, 2*Lmax+1 <= 4096, 1 <= max_move <= 8, else 1; a NULL pointer 3; both before anything touches a device.
 * v100_ctc_align_block(): frames per staged block of emissions (lengths around it and its multiples are the kernel's seams). */
long long v100_ctc_align_workspace_bytes(int B, int T, int Lmax);
int v100_ctc_align_block(void);
int v100_ctc_align(const float* logp, const long long* labels, const int* in_len, const int* lab_len, void* moves_ws, int* path,
                   long long* best_labels, int* align, float* score, int B, int T, int V, int Lmax, int max_move, void* stream);
/* K29, forced alignment of long recordings in one launch (csrc/align_long.hip): a banded Viterbi over the CTC topology (stay, advance,
 * skip a blank between two different labels; first maximum wins; one fp32 add per frame and state).  logp [B][T][V] log-probabilities,
 * labels [B][Lmax] int64, in_len / lab_len [B] or NULL (clamped to [.., T] / [0, Lmax] on the device), free_logp [B][T] or NULL:
 * what the first and the last extended position emit instead of the blank's log-probability.  Only `band` consecutive positions are
 * live; every v100_ctc_align_long_block() frames the window is re-centred on its best position (it never moves back; the two
 * positions that emit free_logp bound every other score and do not count as the best) and the scores are renormalised into an fp64
 * offset.  score [B] fp64; ok [B] int32 = 0 where the end position is not live in the last window (too
 * few frames, no frame, or a band that lost the path): that row has score -inf and zeros in path and align.  path [B][T] int32 =
 * extended positions, 0 beyond in_len; align [B][2*Lmax+1] int32 = frames per extended position, 0 beyond 2*lab_len+1.
 * ws: v100_ctc_align_long_workspace_bytes(B, T, Lmax, band) bytes (two bits per frame and window slot, and the window's start per
 * block; 0 = unsupported shape).  B >= 1, 1 <= T <= 2^20, 0 <= Lmax <= 2^19, V >= 2, band a multiple of 64 in [64, 8192], else 1;
 * a NULL required pointer 3; both before anything touches a device. */
long long v100_ctc_align_long_workspace_bytes(int B, int T, int Lmax, int band);
int v100_ctc_align_long_block(void);
int v100_ctc_align_long(const float* logp, const long long* labels, const int* in_len, const int* lab_len, const float* free_logp, void* ws,
                        double* score, int* ok, int* path, int* align, int B, int T, int V, int Lmax, int band, int blank, void* stream);
/* K31, the CTC pause cutter (csrc/cut_points.hip): where to cut recordings of up to 2^20 frames into pieces of at most max_frames
 * frames for a batched decode.  logits [B][T][V] fp32, lengths [B] or NULL (clamped to [0, T] on the device; nothing beyond a row's
 * length is read).  The rule, which tests/_cut_points_ref.py defines and the device equals exactly: a frame is silent where
 * logits[blank] - max of the others (one fp32 subtraction; NaN is not silent) exceeds margin; the recording is trimmed to its non-silent
 * frames; every silent run of min_gap frames or more is a cut (min_gap 0: none); what lies between cuts and is longer than
 * C = max_frames - 2 pad is split left to right at its longest silent run that leaves min_frames on both sides and at most C on the
 * left (ties to the latest), or, where there is none, forced at the first maximum of the margin in the second half of the reach.
 * v100_ctc_cut_points fills the workspace and n_seg [B] int32, the number of pieces per row: two launches, nothing is read back.
 * v100_ctc_cut_points_table, called with S >= 1 and the same T and pad, then writes start, end, forced [B][S] int32 from the workspace:
 * the pieces widened by min(pad, half the silence shared with a neighbour), by min(pad, what is there) at the recording's two ends and
 * not at all on a forced side; forced = 1 on the piece that begins at a forced cut; zeros beyond n_seg (and pieces beyond S are left
 * out).  ws: v100_ctc_cut_points_workspace_bytes(B, T) bytes (0 = unsupported).  B >= 1, 1 <= T <= 2^20, 2 <= V <= 128,
 * 0 <= blank < V, 2 <= max_frames <= 4096, pad >= 0, min_frames >= 1, max_frames - 2 pad >= 2 min_frames, min_gap >= 0, margin not NaN,
 * 1 <= S <= T, else 1; a NULL pointer 3; both before anything touches a device.  v100_ctc_cut_points_span() / _pass(): frames per
 * thread and per pass of the run scan (lengths around them and their multiples are the kernel's seams). */
long long v100_ctc_cut_points_workspace_bytes(int B, int T);
int v100_ctc_cut_points_span(void);
int v100_ctc_cut_points_pass(void);
int v100_ctc_cut_points(const float* logits, const int* lengths, void* ws, int* n_seg, int B, int T, int V, int blank, int max_frames,
                        int min_gap, float margin, int pad, int min_frames, void* stream);
int v100_ctc_cut_points_table(const void* ws, int* start, int* end, int* forced, int B, int T, int S, int pad, void* stream);
/* K23, batched edit distance (csrc/edit_distance.hip): the Levenshtein distance (unit costs for substitution, insertion and
 * deletion) between hyp [B][Th] int64 and ref [B][Tr] int64, rows of hyp_len / ref_len [B] int32 ids (clamped to [0, width] on the
 * device; nothing beyond a row's length is read; ids compare on all 64 bits).  levels: 1 = id level (a token is one id), 2 = word
 * level (a token is a maximal run of ids != sep inside the row's length: str.split() on the decoded text; two words are equal iff
 * they have the same length and the same ids), 3 = both from ONE launch; nl = 2 for levels == 3, else 1.  Outputs, level-major (the
 * id level first): dist, hyp_n, ref_n [nl][B] int32 = the distance and the two token counts (the lengths at the id level);
 * totals [nl][3] int64, into which the launch ADDS the batch sums of {dist, hyp_n, ref_n} (the caller zeroes it; integer adds, so
 * the result does not depend on their order).  The three per-row outputs go together; they or totals may be NULL, not both.
 * ws: v100_edit_distance_workspace_bytes(B, Th, Tr) bytes (the tokens and word bounds of both levels; -1 = unsupported shape).
 * B >= 1, 1 <= Th, Tr <= 4096, levels in 1..3, else 1; a NULL required pointer 3; both before anything touches a device. */
long long v100_edit_distance_workspace_bytes(int B, int Th, int Tr);
int v100_edit_distance(const long long* hyp, const int* hyp_len, const long long* ref, const int* ref_len, void* ws, int* dist,
                       int* hyp_n, int* ref_n, long long* totals, int B, int Th, int Tr, int levels, long long sep, void* stream);
/* K24, CTC prefix beam search in one launch (csrc/beam.hip): logits [B][T][V] fp32 (the kernel takes the log-softmax itself),
 * lens [B] int32 or NULL (every row T frames; clamped to [0, T] on the device, nothing beyond a row's length is read).  A beam of W
 * distinct prefixes, each with the log probability of all its alignments ending in blank / in a label; contributions to the same
 * prefix merge; the W best totals survive a frame.  Outputs, best first: ids [B][nbest][T] int64 (0 beyond each hypothesis),
 * ids_len [B][nbest] int32, scores [B][nbest] fp32 = total log probability of the transcript; -inf with length 0 where the beam holds
 * fewer than nbest hypotheses; a row of length 0 gives the empty hypothesis with score 0.  Ties: the lower candidate index (beam
 * entry, then class), so two calls give equal bits.
 * ws: v100_ctc_beam_workspace_bytes(B, T, V, W) bytes (per utterance the prefix trie, 1 + W T nodes, and its child table of
 * 2 W T slots rounded up to a power of two; -1 = unsupported shape).
 * B >= 1, 1 <= T <= 4096, 2 <= V <= 128, 1 <= W <= 64, 1 <= nbest <= W, 0 <= blank < V, else 1; a NULL required pointer 3; both
 * before anything touches a device. */
long long v100_ctc_beam_workspace_bytes(int B, int T, int V, int W);
int v100_ctc_beam_search(const float* logits, const int* lens, void* ws, long long* ids, int* ids_len, float* scores, int B, int T, int V,
                         int W, int nbest, int blank, void* stream);
/* K25, the same search with an n-gram language model fused into the per-frame selection (shallow fusion): the beam is ranked by
 * key = log p_ctc + alpha log p_lm + beta length.  The LM is a deterministic automaton over the logits' own label ids, back-off
 * already resolved: lm_logp [S][V] fp32 natural log, lm_next [S][V] int32 (the state after (state, label); clamped to [0, S) on the
 * device), lm_final [S] fp32 = log p(end of sentence | state), added (times alpha) before the final ranking iff use_eos.  The blank
 * column of both tables never enters a result.  An extension of an entry by c adds lm_logp[state][c] to its LM sum and 1 to its length; a
 * stay keeps both; the CTC recurrences never see the LM, and a candidate whose CTC total is -inf or NaN stays no candidate.
 * Outputs as K24's, with scores = the key, ctc_scores [B][nbest] = K24's score of the same transcript, lm_scores [B][nbest] = the
 * LM sum (lm_final included iff use_eos); -inf, -inf, 0 where there is no hypothesis.  alpha = beta = 0, use_eos = 0 gives K24's
 * ids, lengths and (in ctc_scores) scores bit for bit.  ws: v100_ctc_beam_workspace_bytes, as K24.
 * K24's limits, and 1 <= S, S V <= 2^28, 0 <= start_state < S, alpha and beta finite, else 1; a NULL pointer (lens excepted) 3;
 * both before anything touches a device. */
int v100_ctc_beam_search_lm(const float* logits, const int* lens, void* ws, long long* ids, int* ids_len, float* scores,
                            const float* lm_logp, const int* lm_next, const float* lm_final, int S, int start_state, float alpha,
                            float beta, int use_eos, float* ctc_scores, float* lm_scores, int B, int T, int V, int W, int nbest,
                            int blank, void* stream);
/* K32, the same search without a frame limit (the resumable form of csrc/beam.hip): the beam survives between launches, so logits
 * can be pushed chunk by chunk, and any split into chunks gives the bits of one call over all the frames.  The caller owns two
 * buffers and ZEROES BOTH ONCE, when the stream is created; the library never zeroes them:
 *   ws:    v100_ctc_beam_stream_workspace_bytes(B, max_frames, V, W) bytes = B x (8 P + 4 ((1 + W max_frames + 3) & ~3)), P the
 *          power of two >= max(64, 2 W max_frames): per row the child table and the trie's nodes for max_frames frames.  The
 *          table's size enters the hash, so the capacity is fixed for the life of the stream; 20 to 36 bytes x W x max_frames a row;
 *   state: v100_ctc_beam_stream_state_bytes(B, W) bytes = B x ((32 + 40 W + 15) & ~15): per row {started, nbeam, frames, 0} int32,
 *          {offset, lmoff} fp64, then pb, pnb, tot fp32, node, par, last, len, state int32, lm, bias fp32, W of each, in beam order.
 * Both helpers are host-only and return -1 on an unsupported shape.
 * push: logits [B][T][V] fp32 and lens [B] int32 or NULL as K24's, 1 <= T <= 4096: row b runs clamp(lens[b], 0, T) more frames,
 *   and never more than max_frames in all (the device clamps; the caller should count).  A row without frames keeps its state bit
 *   for bit.  The LM form takes K25's tables and weights; they must be the same in every push of a stream.
 * read: the current n best, outputs as K24's / K25's with ids [B][nbest][width]; a hypothesis' length is clamped to
 *   min(the row's frames so far, width).  It runs no frame and stores nothing, so it may be called at any time, and twice.  The LM
 *   form adds alpha lm_final[state] before the ranking iff `final`, exactly as K25's last ranking does with use_eos.  Reading the
 *   labels back costs one dependent load per label of each hypothesis.
 * Everything that comes out of `state` is clamped on the device before it is used as an index: a damaged state gives wrong text,
 * never an access outside the row's buffers.
 * B >= 1, 2 <= V <= 128, 1 <= W <= 64, max_frames >= 1 with W max_frames < 2^25 (the trie's keys stay below 2^32), 0 <= blank < V,
 * 1 <= nbest <= W, width >= 1 and K25's limits on the LM, else 1; a NULL pointer (lens excepted) 3; both before anything touches a
 * device. */
long long v100_ctc_beam_stream_workspace_bytes(int B, int max_frames, int V, int W);
long long v100_ctc_beam_stream_state_bytes(int B, int W);
int v100_ctc_beam_stream_push(const float* logits, const int* lens, void* ws, void* state, int B, int T, int max_frames, int V, int W,
                              int blank, void* stream);
int v100_ctc_beam_stream_push_lm(const float* logits, const int* lens, void* ws, void* state, const float* lm_logp, const int* lm_next,
                                 const float* lm_final, int S, int start_state, float alpha, float beta, int B, int T, int max_frames,
                                 int V, int W, int blank, void* stream);
int v100_ctc_beam_stream_read(const void* ws, const void* state, long long* ids, int* ids_len, float* scores, int B, int max_frames,
                              int V, int W, int nbest, int width, void* stream);
int v100_ctc_beam_stream_read_lm(const void* ws, const void* state, long long* ids, int* ids_len, float* scores, const float* lm_final,
                                 int S, int start_state, float alpha, float beta, int final, float* ctc_scores, float* lm_scores, int B,
                                 int max_frames, int V, int W, int nbest, int width, void* stream);
/* K26, word timestamps and confidences (csrc/ctc_segment.hip): the CTC forward-backward over all alignments of a GIVEN transcript
 * in one launch, reduced per label and per word.  It is the posterior of the alignments given the transcript, not a posterior of
 * the transcript being right.  logits [B][T][V] fp32 (the kernel takes the log-softmax itself), labels [B][Lmax] int64; in_len /
 * lab_len [B] int32 or NULL (= T / Lmax everywhere), clamped to [0, T] / [0, Lmax] on the device; nothing beyond a row's lengths is
 * read.  With gamma_t(i) the posterior probability that frame t is spent in label i:
 *   log_prob [B]           log p(labels | logits), the sum over all alignments (= -nll of K10, K24's score of that transcript)
 *   duration [B][Lmax]     sum_t gamma_t(i), the expected number of frames
 *   log_conf [B][Lmax]     sum_t gamma_t(i) log_softmax(logits[t])[l_i] / duration[i]
 *   start, end [B][Lmax]   the medians of the label's first frame and of one past its last frame: start < end <= next start <= T_b
 * and per word, a maximal run of labels != sep inside the row's length ([B][(Lmax + 1) / 2]): word_first (its first label), word_count,
 * word_start = start[first], word_end = end[last], word_log_conf = the same ratio over the word's labels; n_words [B].  The six word
 * pointers are all NULL (no word level) or all given.  Beyond lab_len / n_words everything is 0.  An infeasible row (p = 0: too few
 * frames, a label equal to blank or outside [0, V)) gets log_prob -inf and start = end = 0, duration 0, log_conf -inf for its labels
 * and words; T_b = 0 gives log_prob 0 iff the row has no label.  No float atomics: two calls give equal bits.
 * ws: v100_ctc_segment_workspace_bytes(B, T, Lmax) bytes (-1 = unsupported shape).  v100_ctc_segment_block(): frames per staged block
 * of emissions (lengths around it and its multiples are the kernel's seams).
 * B >= 1, 1 <= T <= 4096, 2 <= V <= 128, 1 <= Lmax <= 2047, 0 <= blank < V, else 1; a NULL required pointer, or some but not all of
 * the word pointers, 3; both before anything touches a device. */
long long v100_ctc_segment_workspace_bytes(int B, int T, int Lmax);
int v100_ctc_segment_block(void);
int v100_ctc_segment(const float* logits, const int* in_len, const long long* labels, const int* lab_len, void* ws, float* log_prob,
                     int* start, int* end, float* duration, float* log_conf, int* word_first, int* word_count, int* word_start,
                     int* word_end, float* word_log_conf, int* n_words, int B, int T, int V, int Lmax, int blank, long long sep,
                     void* stream);
/* K33, the same for chapter-length recordings (csrc/ctc_segment_long.hip): K26's forward-backward restricted to a corridor.  Frames
 * come in blocks of v100_ctc_segment_long_block() = 16; lo [B][ceil(T/16)] int32 is the first live state of each block and band = W the
 * number of live states: state s of the n = 2 L + 1 is live at frame t iff lo[t >> 4] <= s < lo[t >> 4] + W.  alpha, beta and the
 * enter / leave terms are zero at every dead state and everything else follows, so every output is the posterior over the
 * alignments that stay inside the corridor; lo = 0 with band >= n is K26's quantity.  tests/_ctc_segment_long_ref.py defines it in
 * float64.  Memory safety does not rest on lo: the device clamps each value to [0, hi], hi = (max(n - W, 0) + 1) & ~1, clears bit 0
 * and takes the running maximum.  Inputs and outputs are K26's, with log_prob [B] in fp64 and ok [B] int32 = 1 where p > 0; a row
 * with p = 0 (the corridor misses the end, too few frames, a label equal to blank or outside [0, V)) gets ok 0 and K26's infeasible
 * outputs, its words still delimited; T_b = 0 gives ok 1 and log_prob 0 iff the row has no label.  Exponents are integers relative
 * to their block, with one int64 offset per block, so 2^20 frames of any logits stay exact; an emission below 2^-(2^22) counts as 0.
 * Two launches (the second sums the words); no float atomics: two calls give equal bits.
 * ws: v100_ctc_segment_long_workspace_bytes(B, T, Lmax, band) bytes = 12 B T band / 2 for alpha and the entering share per frame and
 * live label, plus 12 bytes per block and 4 per label, each part rounded up to 16 (a host helper; 0 = unsupported shape).
 * B >= 1, 1 <= T <= 2^20, 0 <= Lmax <= 2^19, 2 <= V <= 128, 0 <= blank < V, band a multiple of 64 in [64, 1024], else 1; a NULL
 * required pointer (in_len and lab_len excepted), or some but not all of the word pointers, 3; both before anything touches a device. */
long long v100_ctc_segment_long_workspace_bytes(int B, int T, int Lmax, int band);
int v100_ctc_segment_long_block(void);
int v100_ctc_segment_long(const float* logits, const int* in_len, const long long* labels, const int* lab_len, const int* lo, void* ws,
                          double* log_prob, int* ok, int* start, int* end, float* duration, float* log_conf, int* word_first,
                          int* word_count, int* word_start, int* word_end, float* word_log_conf, int* n_words, int B, int T, int V,
                          int Lmax, int band, int blank, long long sep, void* stream);
/* K27, objective scores of synthesised WORLD features (csrc/dtw.hip): dynamic time warping between x [B][Tx][D] fp32 (the hypothesis)
 * and y [B][Ty][D] fp32 (the reference), rows of x_len / y_len [B] int32 frames (NULL = full width; clamped to [0, width] on the
 * device; nothing beyond a row's length is read), and the sums along the warping path.  With n, m the two lengths of a pair:
 *   d(i,j) = sqrt(sum_{k = skip}^{D-1} (x[i][k] - y[j][k])^2)              (skip leading dimensions left out: MCD leaves out c0)
 *   mode 0, DTW: C(0,0) = d(0,0), C(i,j) = d(i,j) + min(C(i-1,j-1), C(i-1,j), C(i,j-1)), predecessors outside the matrix absent, a
 *     tie to the first candidate in that order; cost = C(n-1,m-1); the path is the backtrace from (n-1,m-1) to (0,0), reported
 *     forwards, path_len in [max(n,m), n+m-1];
 *   mode 1, identity: the path is (i,i) for i < min(n,m), cost the sum of d(i,i).
 * f0x [B][Tx], f0y [B][Ty] fp32 in Hz, both or neither; a frame is voiced iff f0 >= f0_floor.  Over the path's pairs: voiced = both
 * frames voiced, vuv_errors = exactly one voiced, f0_sq_cents = sum (1200 log2(f0x/f0y))^2 and f0_sq_hz = sum (f0x - f0y)^2 over the
 * voiced pairs (all 0 without the f0 inputs).  A pair with n = 0 or m = 0 gives zeros everywhere.
 * d is fp32 from differences with the root rounded once; the cumulative cost and the f0 sums are fp64.
 * Outputs per row: cost, f0_sq_cents, f0_sq_hz [B] fp64; path_len, voiced, vuv_errors [B] int32; these six go together.  path
 * [B][Tx+Ty-1][2] int32 (needs the six; zero beyond path_len) or NULL.  totals [6] fp64, into which the launches ADD the batch sums
 * {pairs, cost, voiced, vuv_errors, f0_sq_cents, f0_sq_hz} (the caller zeroes it; the counts are sums of integers below 2^53 and
 * stay exact).  The per-row outputs or totals may be NULL, not both.
 * ws: v100_dtw_workspace_bytes(B, Tx, Ty, D, want_path) bytes (the distance matrices, 2-bit backpointers, and with want_path the
 * reversed paths; -1 = unsupported shape).
 * B >= 1, 1 <= Tx, Ty <= 4096, 0 <= skip < D, D - skip <= 64, mode 0 or 1, else 1; a NULL required pointer (x, y, ws, one f0 track
 * without the other, some but not all per-row outputs, no output at all) 3; both before anything touches a device. */
long long v100_dtw_workspace_bytes(int B, int Tx, int Ty, int D, int want_path);
int v100_dtw_score(const float* x, const int* x_len, const float* y, const int* y_len, const float* f0x, const float* f0y, void* ws,
                   double* cost, int* path_len, int* voiced, int* vuv_errors, double* f0_sq_cents, double* f0_sq_hz, int* path,
                   double* totals, int B, int Tx, int Ty, int D, int skip, float f0_floor, int mode, void* stream);
/* TextToAlignTextModel.align (voice100/models/tts.py:89-110) batched: text [B][Lmax] int64, align [B][Lmax][2] float64
 * (gap, length), out [B][Tmax] int64 (zero padded; rows longer than Tmax are cut), out_len [B].  out == NULL: only out_len is
 * written (head + int(sum(align)) + tail per utterance), so the caller can size `out` with one read-back. */
int v100_align_expand(const long long* text, const double* align, const int* text_len, long long* out, int* out_len, int B, int Lmax,
                      int Tmax, int head, int tail, void* stream);


/* ---- WORLD analysis (csrc/world_analysis.hip; SURVEY.md 8f rank 4, second half) -- PARITY UNPINNED -------------------------------
 * pyworld.dio / cheaptrick / d4c / code_aperiodicity as WORLDVocoder.encode calls them (voice100/vocoder.py:61-74), in fp64 (the
 * reference converts the waveform to double).  pyworld 0.3.2 (C++ WORLD) is not in the reference tree: the kernels follow the
 * published algorithms as restated in oracle/world_analysis.py.  Waveforms x [B][pitch] fp32 with lengths [B] (samples); frame t of
 * an utterance sits at t * frame_period_ms / 1000 s and an utterance of n samples has v100_world_frames(fs, n, frame_period_ms) =
 * (int)(1000 n / fs / frame_period_ms) + 1 frames; Tmax = that of max_len is the row pitch of every per-frame array.
 *   v100_world_randn_host_f64   HOST function, HOST pointer: WORLD's randn() sequence in double (the safeguard noise of the
 *                               analysis: every call of cheaptrick / d4c restarts it); v100_world_randn_bound(kind, T, fs, fft_size)
 *                               = draws T frames can consume (kind 0 cheaptrick, 1 d4c): the least table_len to pass.
 *   v100_world_dio_bands        number of DIO bands; half_lengths [bands] (HOST) = matlab_round(fs / boundary_f0 / 2) of each.
 *   v100_world_dio              speed = 1 (no decimation).  lowcut [2 hc + 1], hc = matlab_round(fs / 50): the centred taps of
 *                               DesignLowCutFilter; nuttall [bands][4 hmax]: row i = NuttallWindow(4 half_lengths[i]), hmax = the
 *                               largest half length, both built in double by the caller -> f0 [B][Tmax] (0 = unvoiced, 0 beyond an
 *                               utterance's frames).
 *   v100_world_cheaptrick       f0 [B][Tmax] double; twiddle [fft_size/2][2] = cos, -sin of 2 pi k / fft_size; offsets [B][Tmax]
 *                               int64 scratch -> sp [B][Tmax][fft_size/2+1] double and/or logsp = (float) log(sp + log_offset)
 *                               (vocoder.py:70); rows of frames the table or LDS cannot serve come back NaN.
 *   v100_world_d4c              twiddle [1024][2] for the internal 2048-point FFTs, nuttall [window_length] = NuttallWindow(
 *                               (int)(3000 * 2048 / fs) * 2 + 1) -> ap [B][Tmax][fft_size/2+1] double and/or coded (double) /
 *                               coded32 (float) [B][Tmax][bands of 3 kHz] = pyworld.code_aperiodicity of it (vocoder.py:72-73). */
int v100_world_randn_host_f64(double* host_out, long long n);
long long v100_world_randn_bound(int kind, int T, int fs, int fft_size);
int v100_world_frames(int fs, int length, double frame_period_ms);
int v100_world_dio_bands(int fs, double f0_floor, double f0_ceil, double channels_in_octave, int* half_lengths, int max_bands);
long long v100_world_dio_workspace_bytes(int B, int max_len, int fs, double f0_floor, double f0_ceil, double channels_in_octave,
                                         double frame_period_ms);
int v100_world_dio(const float* x, const int* lengths, int B, int max_len, int pitch, int fs, double f0_floor, double f0_ceil,
                   double channels_in_octave, double frame_period_ms, double allowed_range, const double* lowcut,
                   const double* nuttall, double* f0, void* workspace, void* stream);
int v100_world_cheaptrick(const float* x, const int* lengths, const double* f0, int B, int max_len, int pitch, int fs,
                          double frame_period_ms, double q1, int fft_size, const double* randn_table, long long table_len,
                          const double* twiddle, double* sp, float* logsp, double log_offset, long long* offsets, void* stream);
long long v100_world_d4c_workspace_bytes(int B, int max_len, int fs, double frame_period_ms);
int v100_world_d4c(const float* x, const int* lengths, const double* f0, int B, int max_len, int pitch, int fs, double frame_period_ms,
                   double threshold, int fft_size, const double* randn_table, long long table_len, const double* twiddle,
                   const double* nuttall, int window_length, double* ap, double* coded, float* coded32, void* workspace, void* stream);

/* ---- K15 LSTM recurrence (csrc/lstm.hip) -----------------------------------------------------------------
 * The recurrent part of nn.LSTM(H, H, bidirectional) over packed, ragged sequences (_asr_v2.py:32-34, the module; :46, its call on a
 * PackedSequence).  The input projection xproj = x W_ih^T + b_ih and the gradients of W_ih, W_hh and x are v100_pw_gemm / v100_pw_wgrad.
 * H % 16 == 0, 16 <= H <= 1024; ndir 1 or 2 (one launch runs both directions); 1 <= lens[b] <= T (int32, device).  Gate order i, f, g, o.
 *   xproj [ndir][B][4H][T], y [B][ndir H][T] (0 at t >= lens[b]), h_n / c_n / dh_n / dc_n [ndir][B][H]; direction 1 runs t = lens[b]-1 .. 0.
 *   Training (act, cs, hprev all given, or none for inference): act [ndir][T][B][4H] gate activations and cs [ndir][T][B][H] cell states
 *   by step, hprev [ndir][B][H][T] the h each t read (the X of the dW_hh GEMM).  Backward: dgates [ndir][B][4H][T] = d(pre-activation
 *   gates), 0 at t >= lens[b]; dh_n / dc_n may be NULL (zero).
 *   w_prep: W_hh of each direction laid out by v100_lstm_weight_prep (backward = 0 for v100_lstm_fwd, 1 for v100_lstm_bwd), size
 *   v100_lstm_weight_bytes.  ws: v100_lstm_ws_bytes (backward as above).  sync: v100_lstm_sync_words(B, ndir) 32-bit words, zeroed by
 *   the call itself; after the call sync[0] != 0 means a hand-off of the persistent form gave up waiting (sync[0] - 1 = the step):
 *   the outputs are then invalid and the caller raises.
 *   use_bf16: 0 exact fp32 MFMA, 1 bf16 operands, 2 fp16 operands (inference only); fp32 accumulate and fp32 cell state in every mode.
 *   persistent: 1 = one launch for all steps when the grid is resident (v100_lstm_persistent_ok), else one launch per step; 0 = one
 *   launch per step.  Both forms compute bit-identical results.
 *   v100_lstm_geometry (host only, no GPU): out[4] = {U hidden units per workgroup, G = H / U workgroups per (direction, 16-sequence
 *   slice), 1 if the W_hh slice is staged in LDS (else read from global memory: step form only), dynamic LDS bytes per workgroup} of
 *   the forward (backward = 0) or backward recurrence; 1 for a shape v100_lstm_fwd / v100_lstm_bwd reject (fp16 has no backward). */
long long v100_lstm_weight_bytes(int H, int ndir, int use_bf16, int backward);
int v100_lstm_geometry(int H, int use_bf16, int backward, int* out);
long long v100_lstm_ws_bytes(int B, int H, int ndir, int backward);
int v100_lstm_sync_words(int B, int ndir);
int v100_lstm_persistent_ok(int B, int H, int ndir, int use_bf16, int backward);
int v100_lstm_weight_prep(const float* w_hh0, const float* w_hh1, int H, int ndir, int use_bf16, int backward, void* out,
                          void* stream);
int v100_lstm_fwd(const float* xproj, const void* w_prep, const float* b_hh0, const float* b_hh1, const int* lens, float* y,
                  float* h_n, float* c_n, float* act, float* cs, float* hprev, void* ws, unsigned* sync, int B, int T, int H,
                  int ndir, int use_bf16, int persistent, void* stream);
int v100_lstm_bwd(const float* dy, const float* dh_n, const float* dc_n, const void* w_prep, const int* lens, const float* act,
                  const float* cs, float* dgates, void* ws, unsigned* sync, int B, int T, int H, int ndir, int use_bf16,
                  int persistent, void* stream);

/* ---- The v2 TTS models (voice100/models/_align_v2.py, _tts_v2.py) -------------------------------------
 * K16 v2 WORLDLoss, value + gradient in one pass (_layers_v2.py:116-163, with AlignTextToAudio._calc_batch_loss, _tts_v2.py:98-101).
 * pred [B][Tp][A], A = 2 + S + 2 Cap: hasf0 logit, f0_hat, logspc_hat[S], hascodeap logits[Cap], codeap_hat[Cap] per frame.
 * RAW targets f0 [B][Tt], logspc [B][Tt][S], codeap [B][Tt][Cap], length [B] int32, and the six WORLDNorm vectors (all required):
 * hasf0 = f0 >= 30 and hascodeap = codeap < -0.2 are formed on the raw values, then the targets are normalised.  Frames with
 * t < min(Tp, Tt) and t < length[b] count; loss[5] = (hasf0 BCE, f0 error * hasf0, mean_S logspc error, mean_Cap hascodeap BCE,
 * mean_Cap codeap error * hascodeap), each summed over those frames and divided by their number.  l1: 0 squared error, 1 absolute.
 * unit [B][Tp][A] = d loss_term(a) / d pred for unit upstream gradients (0 on frames that do not count).  partial:
 * v100_world_loss_parts(B, Tp) x 5 floats, added in a fixed order (deterministic, no atomics). */
int v100_world_loss_v2(const float* pred, const float* f0, const float* logspc, const float* codeap, const int* length,
                       const float* f0_mean, const float* f0_std, const float* ls_mean, const float* ls_std,
                       const float* ca_mean, const float* ca_std, float* partial, float* loss, float* unit,
                       int B, int Tp, int Tt, int S, int Cap, int l1, void* stream);
/* dpred[b][t][a] = unit[b][t][a] * gout[term(a)], gout [5] on the device */
int v100_world_loss_v2_bwd(const float* unit, const float* gout, float* dpred, int B, int Tp, int S, int Cap, void* stream);
/* K17 TextToAlignText's masked L1 loss (_align_v2.py:80-88): pred [B][L][2] fp32, align [B][W] int64 with W >= 2L (the first 2L
 * entries are the (gap, len) pairs), text_len [B] int32.  loss[0] = sum over rows i < text_len[b] of mean_k |log(align + 1) - pred|
 * divided by sum_b min(text_len[b], L); unit [B][L][2] = its gradient for a unit upstream gradient.  partial:
 * v100_align_loss_parts(B, L) floats, added in a fixed order. */
int v100_align_loss_parts(int B, int L);
int v100_align_loss(const float* pred, const long long* align, const int* text_len, float* partial, float* loss, float* unit,
                    int B, int L, int W, void* stream);
/* dpred = unit * gout[0], gout [1] on the device */
int v100_align_loss_bwd(const float* unit, const float* gout, float* dpred, int B, int L, void* stream);
/* TextToAlignText.align, the v2 expansion (_align_v2.py:48-73) batched, with v100_align_expand's two-pass contract: text [B][Lmax]
 * int64, align [B][Lmax][2] float64 (gap, length), out [B][Tmax] int64 zero padded, out_len [B].  Per utterance over its own
 * text_len rows: length = head + trunc(sum(align) - align[0][0]) + tail, the sum in fp64 in index order; the running position is
 * fp64, spans start at max(trunc(t), previous end) and end at max(trunc(t), start + 1), so every token gets at least one frame.
 * Where the last span's end passes `length` (the reference raises IndexError) the length is that end.  out == NULL: only
 * out_len is written. */
int v100_align_expand_v2(const long long* text, const double* align, const int* text_len, long long* out, int* out_len, int B,
                         int Lmax, int Tmax, int head, int tail, void* stream);
/* AlignTextToAudio.predict epilogue (_tts_v2.py:80-94): x [B][T][2+S+2Cap] -> f0 = (x0 < 0 ? 0 : x1*std+mean), logspc = x*std+mean,
 * codeap = (hascodeap logit < 0 ? 0 : x*std+mean), per codeap feature */
int v100_world_unnormalize_v2(const float* x, float* f0, float* logspc, float* codeap, const float* f0_mean, const float* f0_std,
                              const float* ls_mean, const float* ls_std, const float* ca_mean, const float* ca_std,
                              int B, int T, int S, int Cap, void* stream);

/* ---- K22 the phone head's masked cross-entropy of AlignTextToAudioMultiTaskModel (voice100/models/tts.py:328-331; csrc/phone_loss.hip),
 * value + gradient in one pass.  logits [B][V][L] fp32, channel first as the 1x1 head writes them; target [B][L] int64;
 * target_len [B] int32.  Column (b, l) counts iff l < min(max(target_len[b], 0), L):
 *   loss[0] = sum over counted columns of (logsumexp_v logits[b][:][l] - logits[b][target][l]) / sum_b clamp(target_len[b], 0, L)
 *   unit [B][V][L] = d loss / d logits for a unit upstream gradient = (softmax - onehot) / that sum, 0 in every other column.
 * torch's CrossEntropyLoss semantics: target == -100 (ignore_index) adds no loss and has a zero gradient but still counts in the
 * divisor when inside the length; every length 0 gives 0 / 0 = NaN.  Any other target outside [0, V) (torch raises) is never used
 * as an index: that column's loss is NaN.  Columns that do not count are never loaded.  partial: v100_masked_ce_parts(B, L)
 * floats (one per workgroup of 64 columns; -1 on B or L < 1), added in block order by a second launch: no atomics, bit-identical
 * from call to call.  1 on B, V or L < 1; 3 on a NULL pointer. */
int v100_masked_ce_parts(int B, int L);
int v100_masked_ce(const float* logits, const long long* target, const int* target_len, float* partial, float* loss, float* unit,
                   int B, int V, int L, void* stream);
/* dlogits = unit * gout[0], gout [1] on the device */
int v100_masked_ce_bwd(const float* unit, const float* gout, float* dlogits, int B, int V, int L, void* stream);

/* ---- sample-rate conversion (csrc/resample.hip): torchaudio.functional.resample's default method ("sinc_interpolation", Hann
 * window) for a rate pair reduced to o / n (orig / gcd, new / gcd).  An utterance of len samples gives
 * v100_resample_out_len(len, o, n) = ceil(n len / o) outputs (a HOST helper, 64-bit: 2^31 - 1 samples at 16 -> 22.05 kHz pass
 * 2^31 outputs; -1 on len < 0, o < 1 or n < 1), and
 *   y[q n + p] = sum_j K[p][j] x[q o + j - width],  x zero outside [0, len),
 * K the [n][2 width + o] polyphase bank.  A phase's taps are non-zero on at most 2 width + 1 consecutive positions, so the kernel
 * takes the bank in COMPACT form: starts [n] int (first tap kept of each phase, floor(p o / n) as voice100_amd.audio_io builds
 * it) and taps [n][L] fp32 (row p = K[p][starts[p] .. starts[p] + L), zero where that runs past the dense row), both on the device.
 * x [B][Nmax], y [B][Mmax] fp32; lens [B] int32 on the device, NULL = every row has Nmax samples (entries are clamped to
 * [0, Nmax]).  The kernel writes row b's min(out_len, Mmax) outputs, zeros from there to Mmax, and that count to out_lens[b]
 * (NULL = not wanted).  fp32 fused multiply-adds in tap order, so a row's values do not depend on what else is in the batch.
 * One workgroup serves v100_resample_tile() consecutive outputs of one utterance.  1 on B, Nmax, Mmax, o, n, width or L < 1 and
 * on B > 65535; 3 on a NULL x, taps, starts or y. */
long long v100_resample_out_len(long long len, int o, int n);
int v100_resample_tile(void);
int v100_resample_sinc(const float* x, const int* lens, const float* taps, const int* starts, float* y, int* out_lens, int B,
                       int Nmax, int Mmax, int o, int n, int width, int L, void* stream);

/* ---- K28 FLAC decoding (csrc/flac.hip): the frame regions of B FLAC files -> PCM, four launches and no read-back.
 * bytes [nbytes] uint8 on the device: the files' frame regions (everything from the first frame on), each beginning on a multiple of
 * 16 and followed by zero bytes up to the next multiple of 16 plus 16 more; nbytes a multiple of 16, 16 <= nbytes < 2^31.
 * table [B][16] int32 on the device, per file: {byte begin, byte end (exclusive), channels, bits per sample, minimum and maximum block
 * size, total samples, output row, first slot, slots, first table entry, table entries (a power of two >= 2 slots), first staging int,
 * 0, 0, 0}; slots bounds the frame candidates of the file (total samples / minimum block size plus slack), its staging area is
 * slots x channels x maximum block size ints.  S, H, stage_ints: the sums over the files; max_file_bytes: the longest frame region.
 * ws: v100_flac_workspace_bytes(B, S, H, stage_ints) bytes (-1 = unsupported).
 * Outputs: wave [B][Cw][Nmax] fp32 = sample / 2^(bits - 1), Cw == 1: channel 0 only; pcm [B][Cp][Nmax] int32 or NULL; both are written
 * inside each file's total samples only (the caller zeroes them); lengths [B] int32 = total samples; status [B][2] int32 = {0, frames}
 * or {code, where}: 1 more frame candidates than slots (where = byte offset), 2 no frame where frame `where` must begin, 3 a reserved
 * code in frame `where`, 4 that frame runs past the file's end, 5 its CRC-16 does not match, 6 its sample position does not follow,
 * 7 it passes total samples, 8 the file ends after `where` frames short of total samples.  A frame counts only on the chain that
 * starts at `begin`; no input bytes, however corrupt, make the kernels read or write outside the buffers described here.
 * 1 on a bad shape; 3 on a NULL pointer (pcm may be NULL). */
long long v100_flac_workspace_bytes(int B, int S, int H, long long stage_ints);
int v100_flac_decode(const unsigned char* bytes, long long nbytes, const int* table, void* ws, float* wave, int* pcm, int* lengths,
                     int* status, int B, int S, int H, long long stage_ints, int max_file_bytes, int Cw, int Cp, int Nmax, void* stream);

/* ---- K30 FLAC encoding (csrc/flac_enc.hip): B items -> their FLAC frames, four launches and no read-back.
 * Input: wave [R][C][N] fp32 (quantised as clamp(rint(x 2^(bits-1))), ties to even), or, when wave is NULL, pcm [R][C][N] int32;
 * C 1 or 2, bits_per_sample 8, 16 or 24, N < 2^31.  ftab [F][8] int32 on the device, one row per frame, frames in file order and files
 * in item order: {input row, first sample within the row, samples (1 .. block_size; only an item's last frame is shorter), frame
 * number within the item, item, 0, 0, 0} -- items are segments of rows, so pieces of one long recording are encoded without a copy.
 * 16 <= block_size <= 4608, max_lpc_order 0 .. 12 (0 = fixed predictors only), max_partition_order 0 .. 6.  rate_code / rate_extra:
 * the frame header's sample-rate code (0 .. 11, 13, 14) and the 16-bit value that follows codes 13 and 14.
 * ws: v100_flac_encode_workspace_bytes(F, C) bytes (-1 = unsupported).
 * Outputs: out [out_bytes] uint8 (zeroed by the call; out_bytes a multiple of 4): the frames, contiguous, in ftab's order; the caller
 * sizes it for the verbatim form, sum over frames of 18 + ceil((16 + (C bits + (C == 2)) samples) / 8), which no frame exceeds.
 * report [F] int32 = each frame's bytes.  status [B][2] int32 = {0, 0} or {code, 0x7FFFFFFF - the item's first offending sample}:
 * 1 a non-finite sample, 2 an int32 sample outside the width (both are encoded as 0 / clamped, the item is to be refused),
 * 3 an internal inconsistency (the frame is left zero), 4 a frame-table row outside the input.
 * 1 on a bad shape; 3 on a NULL pointer (one of wave and pcm may be NULL). */
long long v100_flac_encode_workspace_bytes(int F, int C);
int v100_flac_encode(const float* wave, const int* pcm, const int* ftab, void* ws, unsigned char* out, int* report, int* status,
                     int B, int F, int R, int C, long long N, int bits_per_sample, int block_size, int max_lpc_order,
                     int max_partition_order, int rate_code, int rate_extra, long long out_bytes, void* stream);

/* ---- K19 WORLD feature statistics (csrc/world_stat.hip): one accumulation step of voice100/calc_stat.py:40-56 over a padded batch.
 * f0 [B][T], logspc [B][T][S], codeap [B][T][A] fp32, f0_len [B] int32, all on the device and contiguous (4-byte alignment is
 * enough).  Frame (b, t) is valid iff t < min(max(f0_len[b], 0), T).  The call ADDS to moments, float64 [4 + 2S + 2A]:
 *   [0]               sum of f0 over valid frames with f0 > 30.0f
 *   [1]               sum of f0^2 over the same frames
 *   [2]               the number of those frames
 *   [3]               the number of valid frames
 *   [4 .. 4+S)        sum of logspc per column over valid frames
 *   [4+S .. 4+2S)     sum of logspc^2 per column over valid frames
 *   [4+2S .. 4+2S+A)  sum of codeap per band over valid frames with codeap < -0.2f (tested per element)
 *   [4+2S+A .. end)   sum of codeap^2 per band over the same elements
 * Every product and sum is float64 (the products are exact); the two thresholds are compared in fp32, as torch compares an fp32
 * tensor with a Python scalar (f0 == 30.0f and codeap == (float)-0.2 are excluded).  An invalid frame is never loaded, so the
 * padding may hold NaN or Inf; a NaN in a valid frame propagates for logspc and fails both tests for f0 and codeap.  Sums of
 * shards add: moments of two calls, processes or ranks may be added element by element.
 * Two launches, no floating-point atomics, bit-identical from run to run: workgroups write partial rows of 4 + 2S + 2A doubles
 * (partial: v100_world_stat_parts(B, T, S) rows, a function of the three only; need not be zeroed), a second launch adds the rows
 * -- 64 runs of consecutive rows, each in index order, the 64 sums then pairwise in a fixed order -- and then adds the total to moments.
 * 1 <= S <= 1024, 1 <= A <= 8, B >= 1, T >= 1; anything else returns 1 (v100_world_stat_parts: -1), a NULL pointer 3, both before
 * anything touches a device. */
int v100_world_stat_parts(int B, int T, int S);
int v100_world_stat_accum(const float* f0, const int* f0_len, const float* logspc, const float* codeap, double* partial,
                          double* moments, int B, int T, int S, int A, void* stream);

/* ---- K34 n-best rescoring with a word-level back-off n-gram model (csrc/rescore.hip): one launch, no read-back.
 * ids [B][nbest][T] int64, lens [B][nbest] int32 (clamped to [0, T] on the device), first [B][nbest] fp32: what the beam search
 * returns; a hypothesis whose first-pass score is -inf (or NaN) is absent.  A word is a maximal run of ids != sep inside the length.
 * The model, as lm.WordNGramLM.compile() lays it out (voice100_amd/lm.py), on the device: pool [pool_len] int64, the spellings;
 * wtab [wtab_len] int32, wtab_len / 4 slots (a power of two) of {word id or -1, pool offset, length, 0}; ng [ng_len] int32, per order
 * n a table of meta[order + n - 1] slots (a power of two) beginning at int32 meta[n - 1], a slot being n word ids (the first -1:
 * empty), then log p and the back-off weight as fp32 bits.  meta [2 order] int64 is HOST memory.  Word ids: 0 <unk>, 1 <s>, 2 </s>,
 * then the vocabulary.  has_bos / has_eos: the model lists <s> / </s>; use_eos: add log p(</s> | ...) where it does.
 * key = first + lm_weight * lm + word_bonus * words in fp64; rank = the number of hypotheses with a greater key, or an equal key and a
 * lower index; absent ones follow in their order.  Outputs, all [B][nbest] but out_ids [B][nbest][T], by rank r: out_order = the
 * first-pass index, out_ids / out_lens / out_first = that hypothesis' row, length and first-pass score as given, out_scores = (fp32)
 * key, out_lm = (fp32) lm, out_nw / out_oov = its words and how many of them are <unk>; -inf, 0, 0, 0 for an absent one.
 * ws: v100_nbest_rescore_workspace_bytes(B, nbest, T) bytes (-1 = unsupported), need not be zeroed.  No table content and no id can
 * move an access outside the buffers described here or keep a loop running.
 * Limits: B >= 1, 1 <= nbest <= 64, 1 <= T <= 4096, 1 <= order <= 8, pool_len, wtab_len, ng_len < 2^31, finite weights; anything else,
 * or a meta that does not fit ng_len, returns 1; a NULL pointer 3; both before anything touches a device. */
long long v100_nbest_rescore_workspace_bytes(int B, int nbest, int T);
int v100_nbest_rescore(const long long* ids, const int* lens, const float* first, const long long* pool, long long pool_len,
                       const int* wtab, long long wtab_len, const int* ng, long long ng_len, const long long* meta, int order,
                       int has_bos, int has_eos, void* ws, long long* out_ids, int* out_lens, float* out_scores, float* out_first,
                       float* out_lm, int* out_nw, int* out_oov, int* out_order, int B, int nbest, int T, long long sep,
                       double lm_weight, double word_bonus, int use_eos, void* stream);

/* ---- K35 minimum-Bayes-risk selection over an n-best list, and the list's distances to a reference (csrc/mbr.hip): three launches
 * on `stream` (tokenise once per utterance, one wave per pair, finalise), no read-back.
 * ids [B][nbest][T] int64, lens [B][nbest] int32 (clamped to [0, T] on the device), scores [B][nbest] fp32: what the beam search or
 * K34 returns; a hypothesis whose score is -inf (or NaN) is absent, one of length 0 with a finite score is present and empty.
 * ref [B][Tr] int64 and ref_len [B] int32 (clamped to [0, Tr]): the reference rows, or both NULL and Tr = 0: no reference (ref_dist
 * and ref_n may then be NULL too and are not written).
 * A token is one id (words = 0), or a maximal run of ids != sep inside the row's length (words != 0); two words are equal iff their
 * lengths and ids are (K23's rule; the hash only finds candidates).
 * In the GIVEN order: dist [B][nbest][nbest] int32 = the Levenshtein distance (unit costs) between the token sequences of hypotheses i
 * and j, symmetric, 0 on the diagonal, -1 where either is absent; ref_dist [B][nbest] = the distance to the reference, -1 for an absent
 * hypothesis; ref_n [B] = the reference's tokens; expected_len [B] fp32 = sum_j p_j tokens_j.
 * p_i = exp(scale (s_i - s_max)) / sum over the present j, fp64 from the fp32 scores, summed in index order, 0 for an absent one;
 * risk_i = sum_j p_j dist[i][j], an fp64 sum in the order j = 0 .. nbest - 1, stored as fp32, +inf for an absent one.
 * rank = the number of hypotheses with a smaller STORED fp32 risk, or an equal one and a lower index; absent ones follow in their
 * order.  By rank r, all [B][nbest] but out_ids [B][nbest][T]: out_order = the given index, out_ids / out_lens / out_scores = that
 * hypothesis' row (moved whole), length and score as given, out_risk, out_post (fp32 p), out_ntok = its tokens (0 for an absent one).
 * ws: v100_nbest_mbr_workspace_bytes(B, nbest, T, Tr) bytes (-1 = unsupported), need not be zeroed: the kernels initialise what they
 * read.  No id and nothing in the workspace can move an access outside the buffers described here or keep a loop running.
 * Limits: B >= 1, 1 <= nbest <= 64, 1 <= T <= 4096, 1 <= Tr <= 4096 with a reference and Tr = 0 without, finite scale >= 0; anything
 * else returns 1; a NULL required pointer (or only one of ref / ref_len) 3; both before anything touches a device. */
long long v100_nbest_mbr_workspace_bytes(int B, int nbest, int T, int Tr);
int v100_nbest_mbr(const long long* ids, const int* lens, const float* scores, const long long* ref, const int* ref_len, void* ws,
                   long long* out_ids, int* out_lens, float* out_scores, float* out_risk, float* out_post, int* out_ntok,
                   int* out_order, int* dist, int* ref_dist, int* ref_n, float* expected_len, int B, int nbest, int T, int Tr,
                   int words, long long sep, double scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VOICE100_HIP_H */
