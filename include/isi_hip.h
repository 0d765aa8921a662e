/*
 * isi_hip.h -- C-ABI of the MI355X (gfx950) compute library behind the
 * `interactive_spectrogram_inpainting.vqvae` module API.
 *
 * Boundary B4 of SURVEY.md section 8(b): plain `extern "C"` functions, raw
 * device pointers + sizes + the caller's HIP stream (passed as void*), no
 * allocation inside (workspace is passed in), no global mutable state,
 * re-entrant.  Every function returns 0 on success or a negative ISI_E_* code;
 * nothing is thrown across the boundary.
 *
 * The reference has no native code: each entry point replaces the stock
 * torch.nn op(s) reached from the cited reference line(s).  Paths are relative
 * to the reference repository root.
 *
 * All activations handled by this library are fp32.  Internal activations are
 * channels-last (N,H,W,C); tensors crossing the reference's API are N,C,H,W and
 * are described to the kernels by explicit element strides.
 */
#ifndef ISI_HIP_H
#define ISI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISI_OK 0
#define ISI_E_INVALID (-1)     /* bad argument / unsupported shape            */
#define ISI_E_LAUNCH (-2)      /* HIP launch or runtime failure               */
#define ISI_E_WORKSPACE (-3)   /* workspace too small                         */
#define ISI_E_UNSUPPORTED (-4) /* configuration outside the implemented range */

/* Library / build identification ("isi_hip gfx950 <n>"). */
const char *isi_version(void);
/* Last HIP error string seen by this thread's most recent failing call. */
const char *isi_last_error(void);

/* sizeof() of the structs below as compiled into the library, so that FFI
 * bindings can verify their own layout: which = 0 isi_src, 1 isi_dst,
 * 2 isi_conv_w, 3 isi_encoder_w, 4 isi_decoder_w, 5 isi_codebook_w,
 * 6 isi_vqvae_w, 7 isi_vqvae_out, 8 isi_attn_args, 9 isi_prior_w,
 * 10 isi_prior_state, 11 isi_attn_bwd_args, 12 isi_reduce_job, 13 isi_prior_rows,
 * 14 isi_prior_code_bias, 15 isi_adam_tensor, 16 isi_adam_hyper, 17 isi_decode_stage_args,
 * 18 isi_decode_single_source_args.
 * Returns 0 for an unknown id. */
size_t isi_abi_struct_bytes(int which);

/* x = max(x, 0) in place over n floats: the in-place nn.ReLU with which
 * RosinalityResBlock overwrites its caller's tensor (encoder_decoder.py:23). */
int isi_relu_inplace_f32(float *x, int64_t n, void *stream);

/* ------------------------------------------------ audio <-> spectrogram */
/* HBM-bound stages of the GANSynth front-end the reference reaches through the absent
 * GANsynth_pytorch.spectrograms_helper (SpectrogramsHelper.to_spectrogram / to_audio;
 * utils/misc.py:10-29, train_vqvae.py:392-400, sample.py:599, flask_server.py:596,1016);
 * specification: oracle/spectrogram_oracle.py (parity unpinned).  The contractions
 * (windowed DFT, mel projections and their inverses) are isi_conv2d_f32 calls.
 *   stft  [B,T,2F]  real block | imaginary block, DC bin dropped (F = n_fft / 2)
 *   a, ph [B,T,F]   channels-last intermediates
 *   spec  [B,2,F,T] channel 0 log-magnitude (mel: log mel power), channel 1 instantaneous
 *                   frequency in units of pi
 * isi_spec_polar: mel = 0: a = log(|X| + 1e-6), ph = angle; mel = 1: a = |X|^2, ph = unwrapped angle.
 * isi_spec_finish: spec0 = mel ? log(a + 1e-6) : a, spec1 = wrapped time difference of ph / pi.
 * isi_spec_inverse_prepare: a = exp(spec0), ph = running sum over time of spec1 * pi.
 * isi_spec_to_stft: mag = mel ? sqrt(max(a, 0) + 1e-6) : a; stft = mag (cos ph | sin ph).
 * isi_overlap_add: audio[b,n] = sum_t frames[b,t,left + n - t*hop], frames [B,T,n_fft]. */
int isi_spec_polar_f32(const float *stft, float *a, float *ph, int B, int T, int F, int mel,
                       void *stream);
int isi_spec_finish_f32(const float *a, const float *ph, float *spec, int B, int T, int F,
                        int mel, void *stream);
int isi_spec_inverse_prepare_f32(const float *spec, float *a, float *ph, int B, int T, int F,
                                 void *stream);
int isi_spec_to_stft_f32(const float *a, const float *ph, float *stft, int64_t rows, int F,
                         int mel, void *stream);
int isi_overlap_add_f32(const float *frames, float *audio, int B, int T, int n_fft, int hop,
                        int left, int64_t L, void *stream);
/* Adjoints of isi_spec_to_stft_f32 and isi_spec_inverse_prepare_f32: the backward of `to_audio`, which the
 * reference obtains from autograd through GANsynth_pytorch when a `_fromSpectrogram` loss trains the VQ-VAE
 * (utils/losses/spectral.py:106-118, train_vqvae.py:88-96).  `a`, `ph` are the forward's inputs. */
int isi_spec_to_stft_bwd_f32(const float *a, const float *ph, const float *dx, float *da, float *dph,
                             int64_t rows, int F, int mel, void *stream);
int isi_spec_inverse_prepare_bwd_f32(const float *spec, const float *da, const float *dph,
                                     float *dspec, int B, int T, int F, void *stream);
/* Phase-locked splice (not in the reference): keep an original sound's own STFT frames where w == 0 and, inside every
 * run of frames with w > 0, continue the original's phase with the decoded phase increments.  Per (b, k) row, with
 * phi_o = angle and Ao = modulus of the original's bin, psi = ph, As = isi_spec_to_stft's magnitude of `a` under `mel`,
 * a run = a maximal range [t0, t1) of frames with w > 0, wrap = principal value in (-pi, pi]:
 *   w == 0:            out = the original's two floats, bit for bit
 *   both neighbours:   c = wrap(phi_o[t1] - phi_o[t0-1] - (psi[t1] - psi[t0-1])) / (t1 - t0 + 1)
 *                      phi[t] = phi_o[t0-1] + (psi[t] - psi[t0-1]) + (t - t0 + 1) c
 *   t0 == 0 only:      phi[t] = phi_o[t1] - (psi[t1] - psi[t])
 *   t1 == T only:      phi[t] = phi_o[t0-1] + (psi[t] - psi[t0-1])
 *   the whole row:     phi[t] = psi[t]; with w == 1 the bits isi_spec_to_stft_f32 writes
 *   magnitude:         As where w == 1, else exp((1 - w) log Ao + w log As); 0 when Ao or As is not positive
 *   out = magnitude (cos phi | sin phi)
 * stft_orig, stft_out [B,T,2F]; a, ph [B,T,F]; w [w_batch,T,F], w_batch 1 or B, weights in [0, 1] (anything not > 0
 * counts as 0).  Inputs and output must not overlap.
 * isi_spec_splice_blend: g[n] = share of the squared periodic-Hann analysis window, over the frames t of [0, T_frames)
 * that reach sample n with a non-zero window value (0 < n + n_fft - hop - t hop < n_fft), that belongs to frames with
 * touched[b,t] != 0; out[n] = orig[n] bit for bit where g == 0, else orig[n] + g (ola[n] - orig[n]).  g is exactly 1
 * where every such frame is touched.  audio_* [B,L], touched [B,T_frames] bytes; hop must divide n_fft. */
int isi_spec_splice_f32(const float *stft_orig, const float *a, const float *ph, const float *w, int w_batch,
                        float *stft_out, int B, int T, int F, int mel, void *stream);
int isi_spec_splice_blend_f32(const float *audio_orig, const float *audio_ola, const unsigned char *touched,
                              float *audio_out, int B, int T_frames, int n_fft, int hop, int64_t L, void *stream);
/* Re-timing of an STFT with identity phase locking (not in the reference): the step that turns the analysis STFT, or
 * isi_spec_to_stft_f32's output, into a time stretch and, with isi_resample_f32 behind the inverse, a transposition.
 * X [B,T,2F] (real block | imaginary block, DC dropped: bin j is DFT bin j + 1 of n_fft = 2F), pos [pos_batch,T_out]
 * (pos_batch 1 or B): the source position of every output frame, in frames, on the device; out [B,T_out,2F].
 * Source, per (b, t, j): P = fl(fl(re re) + fl(im im)) in float32 without FMA, A = sqrt P, phi = atan2(im, re),
 * Omega_j = 2 pi ((j + 1) hop mod n_fft) / n_fft, dev[t] = wrap(phi[t+1] - phi[t] - Omega_j) for t <= T - 2, wrap =
 * principal value in (-pi, pi].  Bin j is a peak of frame t iff P > 0 and for d = 1, 2: P[j] > P[j-d] and
 * P[j] >= P[j+d] (neighbours outside [0, F) do not object); near[t,j] = the peak nearest to j, the lower one on a tie,
 * j itself in a frame without a peak.
 * Output frame u: p = pos[u] clamped to [0, T-1] (a NaN counts as 0; no content of pos leads to an access outside the
 * arrays), t = min(floor p, T - 2), f = p - t, ta = f < 0.5 ? t : t + 1,
 *   M[j] = (1 - f) A[t,j] + f A[t+1,j],   D[j] = Omega_j + ((1 - f) dev[max(t-1,0),j] + f dev[t,j]),
 *   u == 0:  Phi[j] = phi[t,j] + f (2 pi (j + 1) hop / n_fft + dev[t,j])
 *   u > 0:   n = near[ta,j], Phi[j] = wrap((Phi_before[n] + D[n]) + (phi[ta,j] - phi[ta,n]))
 *   out = M (cos Phi | sin Phi).
 * The leading copy run: with c the largest count such that pos[0] is an integer in [0, T-1] and pos[u] == pos[0] + u
 * <= T - 1 for every u < c, frames u < c are the source's two floats of frame pos[u], bit for bit, and Phi of frame
 * c - 1 is that frame's phi: pos = 0, 1, ..., T - 1 returns X.
 * workspace: isi_stft_stretch_workspace_bytes(B, T, F) bytes (host only; 0 for sizes the call refuses), four [B,T,F]
 * planes the call fills: A, phi, dev (float32; dev of frame T - 1 is 0) and near (int32) -- readable afterwards.
 * Refused before any launch: a null or misaligned pointer, B, F or T_out < 1, T < 2, pos_batch outside {1, B}, hop < 1 or
 * not dividing 2F (ISI_E_INVALID); F > ISI_STFT_STRETCH_MAX_F, T > 2^24 (positions are float32 frame numbers), X or
 * out above 2^30 - 4 elements (ISI_E_UNSUPPORTED); a workspace too small (ISI_E_WORKSPACE).  Inputs, output and
 * workspace must not overlap. */
#define ISI_STFT_STRETCH_MAX_F 2048
size_t isi_stft_stretch_workspace_bytes(int B, int T, int F);
int isi_stft_stretch_f32(const float *X, const float *pos, int pos_batch, float *out, void *workspace,
                         size_t workspace_bytes, int B, int T, int T_out, int F, int hop, void *stream);
/* Formant correction of STFT frames by the true envelope (not in the reference; GANsynth_pytorch/stretch.py and bend.py;
 * DESIGN.md section 6j; specification tests/formant_spec.py): `transpose` and `bend` move the pitch by reading the sound
 * faster or slower, so a component at f in the stretched sound ends at rho f and should carry the envelope's value there.
 * Y [B,T,2F] in isi_stft_stretch_f32's layout, ratio [ratio_batch,T] (ratio_batch 1 or B) on the device, cos_table [2F]:
 * cos(pi i / F) made by the caller in float64 and rounded once; out [B,T,2F]; env [B,T,F+1] or NULL.  depth and max_gain
 * are in nepers.  Per frame (b, t), with n = order, I = iterations:
 *   P_j = fl(fl(re re) + fl(im im)) in float32 without FMA; Pmax = max_j P_j, NaN if any P_j is.
 *   rho = ratio clamped to [1/4, 4]; a NaN counts as 1.
 *   The frame is copied bit for bit unless 0 < Pmax < +inf, and when rho == 1.
 *   L_j = max(1/2 ln P_j, 1/2 ln Pmax - depth); on k = 0 .. F: Lx_0 = L_0 (the dropped DC bin takes bin 1's value), Lx_k = L_{k-1}.
 *   S(A): c_q = (1 / 2F) [A_0 + (-1)^q A_F + 2 sum_{k=1}^{F-1} A_k cos(pi q k / F)], q = 0 .. n - 1,
 *         w_q = (1 + cos(pi q / n)) / 2,   V_k = w_0 c_0 + 2 sum_{q=1}^{n-1} w_q c_q cos(pi q k / F).
 *   A(0) = Lx; for i = 1 .. I: V(i) = S(A(i-1)), A(i) = max(Lx, V(i)); V = V(I).  The count is fixed.
 *   x = min(fl(rho k), F) in float32, i = min(floor x, F - 1), f = x - i, V_x = (1 - f) V_i + f V_{i+1},
 *   out_j = exp(clamp(V_x - V_k, -max_gain, +max_gain)) (re_j, im_j), k = j + 1.  Phases are untouched.
 * cos(pi q k / F) is cos_table[(q k) mod 2F]; the sums are float32 fma chains in a fixed order (a frame's bits depend on
 * that frame and its ratio alone, not on B, T or the launch).  env receives V of every frame: a frame copied because
 * rho == 1 still has its row computed; a frame copied because of Pmax has the row +0.0.
 * No content of ratio leads to an access outside the arrays.  No atomics, no allocation, no host synchronisation;
 * stream-ordered.  Refused before any launch: a null (env excepted) or misaligned pointer, B, T or F < 1, F < 2, order
 * outside [2, min(F, ISI_FORMANT_MAX_ORDER)], iterations outside [1, ISI_FORMANT_MAX_ITERATIONS], ratio_batch outside
 * {1, B}, a depth or max_gain that is NaN, negative or infinite, Y, out and env overlapping -- out == Y is not supported
 * -- (ISI_E_INVALID); F > ISI_STFT_STRETCH_MAX_F, an array above 2^30 - 4 elements (ISI_E_UNSUPPORTED). */
#define ISI_FORMANT_MAX_ORDER 256
#define ISI_FORMANT_MAX_ITERATIONS 64
int isi_formant_shift_f32(const float *Y, const float *ratio, int ratio_batch, const float *cos_table, float *out,
                          float *env, int B, int T, int F, int order, int iterations, float depth, float max_gain,
                          void *stream);
/* One scale of the multi-scale spectral loss (reference utils/losses/spectral.py:78-118, where the STFTs come
 * from torch.stft): xp / xt = STFT rows [B*T][RS] (re block | im block of F bins, RS >= 2F) of the predicted and
 * the target audio.  fwd: per (sample, chunk of rows_per_block frames) the sums
 *   sum |dm|, sum dm^2, sum |dl|, sum dl^2,  dm = |Xp| - |Xt|, dl = log(|Xp| + eps) - log(|Xt| + eps)
 * into partial[B][ceil(T / rows_per_block)][4] (L1 / MSE means and per-sample L2 norms are sums of these).
 * bwd: dx = d/dXp of sum_b clin[b] g(dm) + clog[b] g(dl), g' = sign (kind 0) or identity (kind 1). */
int isi_spec_distance_fwd_f32(const float *xp, const float *xt, float *partial, int B, int T, int F,
                              int RS, float eps, int rows_per_block, void *stream);
int isi_spec_distance_bwd_f32(const float *xp, const float *xt, float *dx, const float *clin,
                              const float *clog, int B, int T, int F, int RS, float eps, int kind,
                              void *stream);
/* Per-channel affine map of a dense [B,2,H,W] spectrogram plus the masked-phase rule, one pass:
 * y0 = a0 x0 + b0; y1 = a1 x1 + b1, set to 0 where the log-magnitude (channel 0 of `ref` when given,
 * else y0) is <= thr (use_mask != 0).  Replaces GANsynth_pytorch's DataNormalizer.normalize /
 * denormalize and make_masked_phase_transform at the reference's call sites vqvae.py:254-255,297-302
 * (package absent from the tree; semantics in oracle/spectrogram_oracle.py).  HW % 4 == 0. */
int isi_spec_affine_mask_f32(const float *x, const float *ref, float *y, int64_t B, int64_t HW,
                             float a0, float b0, float a1, float b1, float thr, int use_mask,
                             void *stream);

/* ------------------------------------------------ sample-rate conversion */
/* Band-limited resampling of uploads and of audio output: the reference's /analyze-audio hands whatever the
 * browser recorded to `spectrograms_helper.from_wavfile(path, duration_n=...)`, which converts it to the models'
 * rate with sox / torchaudio (flask_server.py:557-568, 624-667); those packages are absent, the arithmetic is
 * specified in tests/resample_spec.py.  A polyphase Kaiser-windowed sinc ("kaiser best": 64 zero crossings,
 * rolloff 0.9475937167399596, beta 14.769656459379492):
 *   g = gcd(fs_in, fs_out), orig = fs_in / g, new = fs_out / g, f0 = rolloff * min(orig, new),
 *   width = ceil(64 * orig / f0), taps = 2 * width + orig, N_out = ceil(L * new / orig),
 *   y[q * new + r] = sum_i h[r][i] * x[q * orig + i - width], x = 0 outside [0, L), i ascending in fp32 fma.
 * isi_resample_geometry (host only): ISI_E_INVALID for rates <= 0; ISI_E_UNSUPPORTED beyond the caps
 * taps <= 16384 (one frame's stage fits 64 KB of LDS) and new * taps <= 2^22 table floats -- the four outputs
 * are written in that case too (saturated at INT_MAX).
 * isi_resample_out_len (host only): ceil(L * new / orig); ISI_E_INVALID for L < 0 or a ratio term <= 0.
 * isi_resample_f32: y[b, 0:N_out] from x[b, 0:L], rows x_stride / y_stride floats apart, any float-aligned bases;
 * table [taps, new] TAP-MAJOR fp32 on the device (h[r][i] at i * new + r), made by the caller.  No atomics, no
 * host synchronisation, no allocation; stream-ordered; the summation order of an output does not depend on B
 * or L.  Checked before any launch: null pointers, B / L / orig / new / width <= 0, a stride shorter than the
 * row (ISI_E_INVALID); L >= 2^31 or the two caps above (ISI_E_UNSUPPORTED). */
int isi_resample_geometry(int fs_in, int fs_out, int *orig, int *new_, int *width, int *taps);
int64_t isi_resample_out_len(int64_t L, int orig, int new_);
int isi_resample_f32(const float *x, int64_t x_stride, float *y, int64_t y_stride, int B, int64_t L,
                     int orig, int new_, int width, const float *table, void *stream);

/* Time-warped read (not in the reference): the same windowed sinc with a position and a cutoff PER OUTPUT SAMPLE, for
 * reading a sound along an arbitrary time map -- vibrato, glides, pitch flattening (GANsynth_pytorch/bend.py; DESIGN.md
 * section 6i; specification tests/warp_resample_spec.py):
 *   y[b, n] = sum_m c h(c (p - m)) x[b, m]  over the integers m in [0, L) with |c (p - m)| < 64, m ascending, fp32 fma
 *   p = pos[b or 0, n] in source samples, c = min(max(cut[b or 0, n], ISI_WARP_CUT_MIN), 1), a NaN cut counts as the minimum
 *   h(t) = sinc(t) I0(beta sqrt(1 - (t / 64)^2)) / I0(beta), the constants of isi_resample_f32 ("kaiser best")
 * x is 0 outside [0, L).  A position that is NaN or infinite, or whose support does not meet [0, L), gives +0.0; no
 * content of pos or cut leads to an access outside the arrays, |p| beyond 2^31 included.  pos is DOUBLE: a float32
 * position near sample 60 000 is good to 2^-8 sample only, a -38 dB phase error at 8 kHz; floor(p) and the fraction are
 * taken once per output in double, every tap distance is then an exact small integer plus that fraction in fp32.  The
 * weights are evaluated in the kernel (no table): within 4.02 x 2^-24 c of the float64 weight, the tap products are
 * summed by fma.  At most 2 * 64 / ISI_WARP_CUT_MIN + 1 = 641 taps per output.
 * x[b, 0:L] and y[b, 0:N_out], rows x_stride / y_stride floats apart, any float-aligned bases; pos (8-byte aligned) and
 * cut [pos_batch, N_out] dense, pos_batch 1 or B.  No atomics, no allocation, no host synchronisation; stream-ordered;
 * the bits of an output depend on its own p, c and the samples under its support -- not on B, the row or the launch.
 * Checked before any launch: null or misaligned pointers, B / L / N_out < 1, pos_batch outside {1, B}, a stride shorter
 * than the row (ISI_E_INVALID); L or N_out >= 2^31, 2^31 workgroups (ISI_E_UNSUPPORTED). */
#define ISI_WARP_CUT_MIN 0.2f
int isi_warp_resample_f32(const float *x, int64_t x_stride, const double *pos, const float *cut, int pos_batch,
                          float *y, int64_t y_stride, int B, int64_t L, int64_t N_out, void *stream);

/* ------------------------------------------------ pitch of an uploaded sound */
/* Both priors are conditioned on the pitch; for an upload nobody knows it.  YIN (de Cheveigne & Kawahara 2002) on
 * the sound brought to 48 kHz (specification tests/pitch_spec.py).  With T =
 * (L - W - tau_max) / hop + 1 frames, frame t starting at s = t * hop:
 *   d[b][t][tau] = sum_{j < W} (x[b][s + j] - x[b][s + j + tau])^2, tau = 0 .. tau_max;  e[b][t] = sum_{j < W} x[b][s + j]^2
 *   cs(tau) = sum_{k = 1 .. tau} d(k), d'(0) = 1, d'(tau) = d(tau) * tau / cs(tau), 1 where cs = 0
 *   tau* = the smallest tau in [tau_min, tau_max) with d'(tau) < threshold, then tau -> tau + 1 while tau + 1 < tau_max
 *          and d'(tau + 1) < d'(tau); with no lag under the threshold the argmin of d' over [tau_min, tau_max), the
 *          lowest tau on ties
 *   period = tau* + (a - c) / (2 v), a, b, c = d(tau* - 1), d(tau*), d(tau* + 1), v = a - 2 b + c, if v > 0, else tau*
 *   aperiodicity = d'(tau*)
 * isi_pitch_frames (host only): T, or ISI_E_INVALID for W <= 0, hop <= 0, tau_max < 0 or L < W + tau_max.
 * isi_pitch_difference_f32: x[b, 0:L], rows x_stride floats apart, any float-aligned base -> d [B][T][tau_max + 1] and
 * energy [B][T], dense fp32.  The direct form, not E_a + E_tau - 2 corr: every term is one subtraction rounded to fp32
 * and one fp32 fma into the lag's sum, j ascending, so d is relatively accurate at the dip, where it is orders below
 * the frame energy: |d - d64| <= (W + 4) 2^-24 d64 against the float64 sum over the same fp32 samples.  The bits of
 * d[b][t][tau] and energy[b][t] depend on that frame's samples, W and tau alone -- not on B, L, t, the alignment or the
 * launch.  Checked before any launch: null pointers, B / L / W / hop <= 0, tau_max < 3, L < W + tau_max, a stride
 * shorter than the row, a pointer not aligned to a float (ISI_E_INVALID); W + tau_max > 15360 -- one frame's samples
 * are staged in LDS --, L >= 2^31, 2^31 workgroups (ISI_E_UNSUPPORTED).
 * isi_pitch_pick_f32: d [n_frames][tau_max + 1] -> period [n_frames] (in samples), aperiodicity [n_frames].  The
 * cumulative sum is an fp32 prefix sum: the choice equals the float64 one wherever every comparison it makes has a
 * relative gap above (tau_max + 2) 2^-24.  Checked before any launch: null pointers, n_frames <= 0, tau_min < 1,
 * tau_max < tau_min + 2, a threshold that is NaN or outside (0, 1] (ISI_E_INVALID); tau_max >= 15360, n_frames >= 2^31
 * (ISI_E_UNSUPPORTED).
 * Both: no atomics, no allocation, no host synchronisation; stream-ordered. */
int64_t isi_pitch_frames(int64_t L, int W, int hop, int tau_max);
int isi_pitch_difference_f32(const float *x, int64_t x_stride, float *d, float *energy, int B, int64_t L, int W,
                             int hop, int tau_max, void *stream);
int isi_pitch_pick_f32(const float *d, int64_t n_frames, int tau_min, int tau_max, float threshold, float *period,
                       float *aperiodicity, void *stream);

/* ------------------------------------------------ query-by-example search of a code database */
/* "The stored sounds most like this one": weighted code-distance sums of Q query codemaps against N stored ones
 * (specification tests/code_search_spec.py).  For one layer with codebook E [K, D]:
 *   T[a][b]    = sum_d (E[a][d] - E[b][d])^2                      d ascending, fp32 fma
 *   dist[j][n] = sum_c w[j][c] * T[query[j][c]][codes[n][c]]      query cells >= K (the priors' mask token) count nothing
 * isi_code_distance_table_f32: codebook [K, D] row-major -> table [K, K].  T[a][a] is exactly 0 and T is bitwise
 * symmetric; |T - T64| <= (D + 4) 2^-24 T64 against the float64 sum of the same fp32 codebook.  ISI_E_INVALID for a
 * null or float-misaligned pointer, K <= 0, D <= 0; ISI_E_UNSUPPORTED for K > 65535.
 * isi_code_search_workspace_bytes (host only): scratch of isi_code_search_f32, ceil(C / 256) * Q * N floats; 0 for
 * sizes the search refuses.
 * isi_code_search_f32: codes uint16 [N, C], query uint16 [Q, C], weights fp32 [Q, C] or NULL (1 on every cell),
 * table fp32 [K, K], allowed uint8 [N] or NULL, dist fp32 [Q, N].  Items with allowed[n] == 0 get +inf.
 * accumulate = 1 adds the sums to what dist holds (a second layer: the caller scales the weights by its factor).
 * A stored code >= K is the index builder's error: it is clamped to K - 1, nothing is read outside the table.
 * Deterministic and item-local: the bits of dist[j][n] depend on query[j], weights[j], codes[n] and the table only --
 * not on N, Q, alignment, the launch geometry or the run.  Each product w * T is rounded once; the products of 256
 * consecutive cells are added in cell order, the sums of those runs in run order; no atomics.  Against the float64
 * sum of the same fp32 products' factors: |dist - spec| <= (C + 2) 2^-24 sum_c |w[c] T[..]|; exact when the table
 * holds small non-negative integers, the weights are 0 or 1 and the sums stay below 2^24.
 * No allocation, no host synchronisation; stream-ordered.  Checked before any launch: a null codes / query / table /
 * dist / workspace, a misaligned pointer (2 bytes for codes and query, 4 for the others), N, C or K <= 0, Q outside
 * 1..64, accumulate outside {0, 1} (ISI_E_INVALID); a workspace smaller than isi_code_search_workspace_bytes
 * (ISI_E_WORKSPACE); K > 16384 -- one table row per staged cell must fit 64 KB of LDS; the quantiser's own limit is
 * far below --, C > 256 * 65535, Q * N >= 2^39 (ISI_E_UNSUPPORTED).  isi_last_error() names the argument. */
int isi_code_distance_table_f32(const float *codebook, float *table, int K, int D, void *stream);
size_t isi_code_search_workspace_bytes(int64_t N, int64_t C, int K, int Q);
int isi_code_search_f32(const uint16_t *codes, const uint16_t *query, const float *weights, const float *table,
                        const uint8_t *allowed, float *dist, int64_t N, int64_t C, int K, int Q, int accumulate,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------ search of a code database by encoder vectors */
/* The asymmetric distance (specification tests/code_soft_search_spec.py): the query is not a
 * codemap but one vector per cell -- an encoder's output before it is snapped to a code, or a blend of codes -- and is
 * compared with the stored codes' vectors, dist(z, x) = sum_c w[c] |z[c] - E[x[c]]|^2.  The searches take it as per-cell
 * ROWS of K floats, so any other per-cell cost can be searched the same way:
 *   R[c][k]    = sum_d (z[c][d] - E[k][d])^2                      d ascending, fp32 fma (the table's expression)
 *   dist[j][n] = sum_c w[j][c] * R[j][c][codes[n][c]]
 * isi_code_query_rows_f32: z fp32 [cells, D] with a row stride of z_stride >= D floats (an NHWC activation is read in
 * place), codebook [K, D] row-major -> rows fp32 [cells, K].  Where z[c] equals codebook row a bit for bit, rows[c][:]
 * equals isi_code_distance_table_f32's T[a][:] bit for bit; |R - R64| <= (D + 4) 2^-24 R64; a non-finite vector gives a
 * non-finite row by IEEE rules and touches no other row.  ISI_E_INVALID for a null or float-misaligned pointer, cells,
 * K or D <= 0, z_stride < D; ISI_E_UNSUPPORTED for K > 65535 and cells * K >= 2^39.
 * isi_code_search_rows_f32: isi_code_search_f32 with rows fp32 [Q, C, K] in place of query and table.  A cell whose
 * weight is exactly 0 contributes +0 whatever its row holds, NaN and inf included: that is this search's mask (there is no
 * mask token).  Everything else is isi_code_search_f32's contract word for word -- weights >= 0 or NULL, one rounding per
 * product, runs of 256 cells in cell order and the run sums in run order, no atomics, stored codes >= K clamped to K - 1,
 * allowed, accumulate, item-local and deterministic results, |dist - spec| <= (C + 2) 2^-24 sum_c |w R| -- and with
 * rows[j][c] = T[query[j][c]] gathered by the caller (mask-token cells under weight 0) dist equals isi_code_search_f32's
 * bit for bit.  The workspace is isi_code_search_workspace_bytes's; the refusals are isi_code_search_f32's, with `rows`
 * where it names query and table. */
int isi_code_query_rows_f32(const float *z, int64_t z_stride, const float *codebook, float *rows, int64_t cells, int K, int D,
                            void *stream);
int isi_code_search_rows_f32(const uint16_t *codes, const float *rows, const float *weights, const uint8_t *allowed,
                             float *dist, int64_t N, int64_t C, int K, int Q, int accumulate, void *workspace,
                             size_t workspace_bytes, void *stream);

/* ------------------------------------------------ shift-invariant search of a code database */
/* "Which stored sound contains something like this fragment, wherever it sits in time" (DESIGN.md section 6c;
 * specification tests/code_shift_search_spec.py).  codes uint16 [N, F, T], query uint16 [Q, F, W] with 1 <= W <= T,
 * weights fp32 [Q, F, W] >= 0 or NULL (1 on every cell), table fp32 [K, K]; offsets o_s = shift0 + s * step for
 * s = 0 .. S-1, every one inside the stored map: shift0 + (S - 1) * step + W <= T.
 *   dist[j][s][n] = sum_f sum_t w[j][f][t] * T[query[j][f][t]][codes[n][f][t + o_s]]
 * dist is fp32 [Q, S, N] (N innermost).  A query cell >= K counts nothing, a stored code >= K is clamped to K - 1, as in
 * isi_code_search_f32.  Summation order (part of the contract): each product is rounded once; query cells are numbered
 * c = f * W + t; the products of a run of 256 consecutive c are added in c order from 0, the run sums in run order; no
 * atomics.  So the bits of dist[j][s][n] depend on query[j], weights[j], the item's codes, the table, W and o_s only --
 * not on N, Q, S, step, alignment, the launch geometry or the run; at W == T, S == 1, shift0 == 0 they are
 * isi_code_search_f32's with C = F * T; |dist - spec| <= (F W + 2) 2^-24 sum |w T[..]|; exact for small integer tables,
 * 0/1 weights and sums below 2^24.  An item's codes are not fetched from memory once per offset: a fetched code serves up
 * to min(W, S) look-ups.  accumulate = 1 adds to what dist holds (a second layer: step = the layers' time ratio r,
 * shift0 = r * the top layer's, W = r * the top layer's, the same S; the caller scales the weights by the layer factor).
 * isi_code_shift_search_workspace_bytes (host only): ceil(F W / 256) * Q * S * N floats of per-run sums when F W > 256;
 * 16 bytes when F W <= 256 (one run: dist is written directly, but the pointer is still checked); 0 for sizes the
 * search refuses.
 * No allocation, no host synchronisation; stream-ordered.  Checked before any launch, isi_last_error() names the
 * argument: a null codes / query / table / dist / workspace, a misaligned pointer (2 bytes for codes and query, 4 for the
 * others), N, F, T, W, S, K or step <= 0, shift0 < 0, W > T, shift0 + (S - 1) * step + W > T, Q outside 1..64,
 * accumulate outside {0, 1} (ISI_E_INVALID); a workspace smaller than isi_code_shift_search_workspace_bytes
 * (ISI_E_WORKSPACE); K > 16384 (one table row per staged cell must fit 64 KB of LDS), F * W > 256 * 65535,
 * F * T >= 2^31, Q * S * N >= 2^39, more than 2^31 - 1 workgroups (ISI_E_UNSUPPORTED).
 * isi_code_shift_best_f32: best[j][n] = min_s dist[j][s][n] and best_shift[j][n] = the smallest s that attains it
 * (int32); where allowed[n] == 0 (allowed uint8 [N] or NULL) best is +inf and best_shift -1.  ISI_E_INVALID for a null
 * or misaligned dist / best / best_shift, N or S <= 0, Q outside 1..64; ISI_E_UNSUPPORTED for Q * S * N >= 2^39.
 * isi_code_shift_search_rows_f32: the same search by encoder vectors (section above): window rows fp32 [Q, F * W, K],
 * cell c = f * W + t, in place of query and table,
 *   dist[j][s][n] = sum_f sum_t w[j][f][t] * R[j][f * W + t][codes[n][f][t + o_s]]
 * with isi_code_shift_search_f32's summation order, workspace and refusals (`rows` where it names query and table) and
 * isi_code_search_rows_f32's zero-weight rule.  With gathered table rows it equals isi_code_shift_search_f32 bit for
 * bit; at W == T, S == 1, shift0 == 0 it equals isi_code_search_rows_f32 bit for bit.  isi_code_shift_best_f32 serves
 * both. */
size_t isi_code_shift_search_workspace_bytes(int64_t N, int F, int T, int W, int S, int K, int Q);
int isi_code_shift_search_f32(const uint16_t *codes, const uint16_t *query, const float *weights, const float *table,
                              float *dist, int64_t N, int F, int T, int W, int shift0, int step, int S, int K, int Q,
                              int accumulate, void *workspace, size_t workspace_bytes, void *stream);
int isi_code_shift_search_rows_f32(const uint16_t *codes, const float *rows, const float *weights, float *dist, int64_t N,
                                   int F, int T, int W, int shift0, int step, int S, int K, int Q, int accumulate,
                                   void *workspace, size_t workspace_bytes, void *stream);
int isi_code_shift_best_f32(const float *dist, const uint8_t *allowed, float *best, int32_t *best_shift, int64_t N, int S,
                            int Q, void *stream);

/* ------------------------------------------------ time-warped search of a code database */
/* "Which stored sound is like this one, played a little faster or slower" (specification
 * tests/code_warp_search_spec.py).  A grid has W query columns and T item columns.  The query is n_parts in {1, 2} parts
 * (a top layer, a bottom layer, or both); part p has F rows, r >= 1 columns of its own per grid column (top: 1; bottom
 * beside a top part: T_b / T_t), a codebook size K, stored codes uint16 [N, F, T r], per-cell cost rows fp32
 * [Q, F * W r, K] with cell c = f * (W r) + (i r + u) -- the rows of isi_code_search_rows_f32; a codemap query is rows
 * gathered from the code distance table by the caller, mask-token cells under weight 0 -- and weights fp32 [Q, F, W r] >= 0
 * or NULL (1 on every cell).
 *   cost[i][t] = sum_p sum_f sum_u fl(w_p[f][i r + u] * rows_p[c][min(codes_p[n][f][t r + u], K - 1)])
 * in fp32 from +0, each product rounded once, added in the order parts, f ascending, u ascending; a cell whose weight is
 * exactly 0 adds +0 whatever its row holds, NaN and inf included.  Query column i is matched to one item column p(i) with
 * p(i+1) - p(i) in {0, 1, 2} (hold, step, skip), lo <= p(i) - i <= hi and 0 <= p(i) <= T - 1; every query column counts
 * once, so the distances of different paths and items compare.  With lo == hi == o the only path is p(i) = o + i.
 *   D[0][t] = cost[0][t];   D[i][t] = fl(cost[i][t] + min(D[i-1][t-1], D[i-1][t], D[i-1][t-2]))   (+inf off the band)
 *   dist = min_t D[W-1][t],  end = the smallest t that attains it;  +inf and -1 without a path or where allowed[n] == 0
 * The minimum is taken by strict comparisons in the order t-1, t, t-2: that is the path's tie rule; it never changes dist,
 * which is the minimum over all admissible paths of the path's left-to-right fp32 sum.
 * isi_code_warp_search_f32: dist fp32 [Q, N], end int32 [Q, N] or NULL, allowed uint8 [N] or NULL.  Deterministic and
 * item-local: the bits of dist[j][n] depend on the query's rows and weights, the item's codes, T, W, lo and hi only -- not
 * on N, Q, the item's position, alignment, the launch geometry or the run; no atomics.  Widening the band never increases
 * a distance.  Exact when the rows hold small non-negative integers, the weights are 0 or 1 and the sums stay below 2^24.
 * For rows >= 0 under non-zero weight |dist - dist64| <= (V + W + 2) 2^-24 dist64, V = sum_p F_p r_p, dist64 the same
 * recurrence in float64 on the same fp32 factors.  Negative or non-finite rows under a non-zero weight follow IEEE rules
 * through the expressions above and touch nothing outside the buffers.  A stored code >= K is clamped to K - 1.  A fetched
 * code serves every (query column, band position) pair of a group of columns that reaches it.  W may exceed T (lo < 0).
 * isi_code_warp_path_f32: the same recurrence for M chosen items per query, items int64 [Q, M] -> path int32 [Q, M, W]
 * (p(i), backtracked on the device from `end`) and dist fp32 [Q, M], bit for bit the search's (allowed is not applied).
 * An item outside [0, N) gets +inf and a path of -1 throughout, as does an item without a path.  The workspace
 * (isi_code_warp_path_workspace_bytes, host only: Q M W (hi - lo + 1) bytes of back-pointers rounded up to 16; 0 for
 * sizes the call refuses) is scratch.  Not tuned: one wavefront per (query, item).
 * No allocation, no host synchronisation; stream-ordered.  Checked before any launch, isi_last_error() names the
 * argument: a null parts / codes / rows / dist (path: items / path / dist / workspace), a misaligned pointer (2 bytes for
 * codes, 8 for items, 4 for the others), N, T, W, F, r or K <= 0, n_parts outside 1..2, Q outside 1..64, M outside 1..64,
 * lo > hi, a band that leaves the first or the last query column without an admissible cell (hi < 0, lo > T - 1,
 * W - 1 + hi < 0 or W - 1 + lo > T - 1) (ISI_E_INVALID); hi - lo + 1 > 64, K > 16384, W > 4096, Q * N >= 2^39,
 * F * max(W, T) * r >= 2^31 (ISI_E_UNSUPPORTED); a workspace smaller than isi_code_warp_path_workspace_bytes
 * (ISI_E_WORKSPACE). */
typedef struct isi_warp_part {
  const uint16_t *codes;   /* [N, F, T r]                 */
  const float *rows;       /* [Q, F * W r, K]             */
  const float *weights;    /* [Q, F, W r] or NULL         */
  int F, r, K;
} isi_warp_part;
int isi_code_warp_search_f32(const isi_warp_part *parts, int n_parts, const uint8_t *allowed, float *dist, int32_t *end,
                             int64_t N, int T, int W, int lo, int hi, int Q, void *stream);
size_t isi_code_warp_path_workspace_bytes(int M, int W, int lo, int hi, int Q);
int isi_code_warp_path_f32(const isi_warp_part *parts, int n_parts, const int64_t *items, int M, int32_t *path, float *dist,
                           void *workspace, size_t workspace_bytes, int64_t N, int T, int W, int lo, int hi, int Q,
                           void *stream);

/* ------------------------------------------------- measurement (bench.py) */
/* Per-launch timing with HIP events recorded on the launch stream.  State is
 * per calling thread; `on` = 1 starts (earlier records cleared), 0 pauses, 2 resumes without
 * clearing (bench.py times every n-th step only).  isi_prof_read blocks
 * until the recorded events have completed and returns, for one kernel id in
 * [0, isi_prof_num_kernels()), the number of launches, their summed duration
 * (ms) and their summed algorithmic FLOPs / bytes. */
/* Execution switches (A/B comparisons in tests, measurements): each is read from the environment variable of the
 * same name once, at first use of the library; isi_knob_set changes it afterwards (process-wide, not thread-safe
 * against concurrent launches).  Names: ISI_CONV_FLUSH (accumulator flush period of the LDS-DMA convolution, default
 * 3, 0 = never), ISI_NO_PAIRS, ISI_NO_CONV_FIRST, ISI_NO_VQ_FUSION, ISI_NO_CODE_TABLES (dec_t's first convolution and
 * upsample[0] as matrix work even where isi_vqvae_w carries their code tables), ISI_NO_CONV_PAIR_KERNEL,
 * ISI_NO_RESBLOCK_PAIR_KERNEL, ISI_NO_CONVT_PAIR_KERNEL, ISI_NO_TAIL_FUSION, ISI_NO_WGRAD_HALO (per-tap weight-gradient
 * kernel instead of the halo-staged one), ISI_NO_GEMM_KERNEL (linear layers and their weight gradients on the 1x1
 * convolution kernels instead of the GEMM kernels), ISI_CONV_PAIR_BM, ISI_CONV_PAIR_ALL,
 * ISI_RESPAIR_TH, ISI_RES_TH, ISI_CONVT_TH, ISI_CONVT_PAIR_TH, ISI_DECODE_NT, ISI_PRIOR_GRAPH,
 * ISI_DECODE_MFMA_ROWS (rows from which a decoding stage runs as matrix tiles, 16), ISI_DECODE_NO_STAT_HANDOFF (every
 * decoding launch forms the LayerNorm statistics of its residual rows itself), ISI_DECODE_STATS_GLOBAL (the tile kernel's
 * input statistics from a second load of the rows), ISI_ATTN_NO_FWD3 / ISI_ATTN_FWD3_ALL (the plane-staged attention
 * forward never / also for single-term products), ISI_DECODE_ATTN_SEPARATE_SPLITS (two key splits of the
 * cached attention as two workgroups + a merging launch) -- all select between kernels that
 * compute the SAME result (to rounding).  The ablation switches ISI_CONV_ABLATE / ISI_VQ_DBG / ISI_RESPAIR_ABL
 * (wrong results by design) exist only in -DISI_MEASURE builds: the default build rejects them. */
int isi_knob_set(const char *name, int value);
int isi_knob_get(const char *name, int *value);
int isi_prof_enable(int on);
int isi_prof_num_kernels(void);
const char *isi_prof_kernel_name(int kernel_id);
int isi_prof_read(int kernel_id, long long *launches, double *ms, double *flops,
                  double *bytes);

/* ---------------------------------------------------------------- packing */

/* Conv2d weight [Cout,Cin,KH,KW] (torch layout) -> [Cout][Kpad] with
 * k = (kh*KW + kw)*Cin + ci, zero padded up to Kpad = roundup(KH*KW*Cin, 32).
 * Replaces nothing in the reference: layout preparation for
 * isi_conv2d_f32 (encoder_decoder.py:95-112,138; vqvae.py:149-150,175-177). */
int isi_pack_conv_weight_f32(const float *w, float *packed, int Cout, int Cin,
                             int KH, int KW, void *stream);
/* isi_pack_conv_weight_f32 followed by isi_split_conv_weight_f16 at packed + isi_packed_conv_weight_floats(...), in one
 * launch: the layout ISI_CONV_W16 / isi_vqvae_w.w16 expect (packed: twice the packed size, 16-byte aligned). */
int isi_pack_conv_weight_w16_f32(const float *w, float *packed, int Cout, int Cin,
                                 int KH, int KW, void *stream);
/* Packed weight of the INPUT-GRADIENT convolution of a stride-1 nn.Conv2d with weight w [Cout][Cin][KH][KW]
 * (autograd's conv backward-data behind train_vqvae.py:181): [Cin][KH*KW*Cout padded to 32] with the window rotated by
 * 180 degrees -- what isi_pack_conv_weight_f32 would make of w.flip(2, 3).transpose(0, 1), in one launch.  Run it
 * through isi_conv2d_f32 with padding K - 1 - p. */
int isi_pack_conv_dgrad_weight_f32(const float *w, float *packed, int Cout, int Cin, int KH,
                                   int KW, void *stream);
/* nn.Linear weight w [N][K] -> operand of its input-gradient GEMM dX = dY W (autograd's linear backward behind
 * train_autoregressive_model.py:199-201): out[0 .. K N) = W^T ([K][N] fp32: the "packed weight" of a 1x1 convolution
 * with K outputs and N inputs), out[K N .. 2 K N) = its split-bf16 pair copy (groups of 8 as {hi[8] | lo[8]}).  Pass it
 * to isi_conv2d_f32 / isi_linear_f32 with ISI_CONV_BF16X3 | ISI_CONV_W16_BF16: the GEMM kernel stages the weight tile by plain copies.  N, K
 * multiples of 32; out: 2 K N floats, 16-byte aligned. */
int isi_pack_linear_wT_bf16(const float *w, float *out, int N, int K, void *stream);
/* The same for n weights in ONE launch: `table` = n rows of four 64-bit words {w, out, N, K} in device memory (w, out:
 * addresses; every N, K a multiple of 32; out: 2 N K floats each).  blocks_per_weight: workgroups per weight (each walks its
 * weight's 32 x 32 tiles with that stride). */
int isi_pack_linear_wT_bf16_multi(const void *table, int n, int blocks_per_weight, void *stream);
/* Every weight layout a VQ-VAE training step needs, re-packed by ONE launch per optimizer step (vqvae/_train.py
 * PackGroup; the reference re-uses nn.Conv2d weights in place, train_vqvae.py:181-183 -- the layouts are this library's):
 * `table` = n entries of 8 int64 in device memory {kind, src, dst, d0, d1, KH, KW, aux}:
 *   kind 0 / 1: isi_pack_conv_weight_f32 / isi_pack_conv_weight_w16_f32 of a weight [d0 = Cout][d1 = Cin][KH][KW];
 *   kind 2: isi_pack_conv_dgrad_weight_f32 of the same; kind 3 / 4: isi_pack_convT_k4s2_weight_f32 of [d0 = Cin][d1 = Cout][4][4]
 *   in the phase-matrix layout (4: followed by isi_split_conv_weight_f16); kind 5: the few-channel layout + pair copy;
 *   kind 6: isi_pack_codebook_f32 of embed [d0 = D][d1 = K] (codes at dst, |e|^2 at aux).  Bit-identical to those calls. */
int isi_pack_multi(const void *table, int n, int blocks_per_entry, void *stream);
/* Split-f16 pair copy of a packed weight (any of the packed layouts; n_floats % 4 == 0, 16-byte aligned):
 * every quad of floats becomes {hi0..hi3 | lo0..lo3}, the f16 pieces of 1024 w, in the same 16 bytes. */
int isi_split_conv_weight_f16(const float *packed_w, float *out, int64_t n_floats, void *stream);
size_t isi_packed_conv_weight_floats(int Cout, int Cin, int KH, int KW);

/* ConvTranspose2d(k=4,s=2,p=1) weight [Cin,Cout,4,4] -> 4 phase matrices
 * [phase=py*2+px][Cout][Kpad], k = (ty*2+tx)*Cin + ci, tap (ty,tx) of phase
 * (py,px) reading torch tap (ky,kx) = (3-py-2ty, 3-px-2tx).
 * When Cout <= 4 and Cin % 32 == 0 (the decoder's last layer) the layout is
 * instead [(ky*4+kx)*Cout+co][Cin] for the small-Cout kernel (GEMM + col2im gather); the choice is a
 * function of (Cin, Cout) only and isi_conv_transpose2d_k4s2_f32 applies the
 * same rule.  (encoder_decoder.py:199-215; vqvae.py:193-201). */
int isi_pack_convT_k4s2_weight_f32(const float *w, float *packed, int Cin,
                                   int Cout, void *stream);
size_t isi_packed_convT_k4s2_weight_floats(int Cin, int Cout);

/* Codebook `embed` [D,K] (column = code, bottleneck.py:47-51) -> row-major
 * [K][D] plus e2[K] = sum_d embed[d,k]^2 (the third term of bottleneck.py:59). */
int isi_pack_codebook_f32(const float *embed, float *codes_kd, float *e2, int D,
                          int K, void *stream);

/* ------------------------------------------------------------ convolution */

/* One source of a (possibly channel-concatenated) convolution input. */
typedef struct isi_src {
  const float *ptr;
  int C;                   /* channels taken from this source              */
  int64_t sn, sc, sh, sw;  /* element strides                              */
} isi_src;

typedef struct isi_dst {
  float *ptr;
  int64_t sn, sc, sh, sw; /* element strides of the FULL output tensor     */
} isi_dst;

/* `relu` argument of the convolution entry points is a flag word: */
#define ISI_CONV_RELU 1   /* rectify the output                                            */
#define ISI_CONV_BF16X3 2 /* opt-in: split-bf16 products (a_hi b_hi + a_hi b_lo + a_lo b_hi on
                           * the bf16 matrix pipe, fp32 accumulate; per-product relative error
                           * ~2^-16 instead of 2^-24).  Default is exact fp32.              */
#define ISI_CONV_BF16X6 4 /* opt-in: six-term split (x = hi + mid + lo exactly; hi.hi, hi.mid, mid.hi,
                           * hi.lo, lo.hi, mid.mid): every term above 2^-24 of a product is kept --
                           * fp32-grade products at 6/16 of the fp32 pipe's matrix time.   */
#define ISI_CONV_F16X3 8  /* opt-in: split-f16 products (two 11-bit pieces, three terms on the f16 matrix
                           * pipe): per-product relative error ~2^-23 like ISI_CONV_BF16X6 at the
                           * cost of ISI_CONV_BF16X3, inside f16's RANGE -- activations must satisfy
                           * |x| < 16384 and weights |w| < 64 (operands are scaled by 2^2 / 2^10 before
                           * the split; the scaling is undone exactly).  An operand outside the range
                           * gives Inf / NaN in the output, never a silently wrong value.        */

#define ISI_CONV_W16_BF16 256 /* with ISI_CONV_BF16X3 on a GEMM-shaped launch (isi_linear_f32, 1x1 isi_conv2d_f32): the packed
                           * weight is followed by its split-bf16 pair copy (isi_pack_linear_wT_bf16).  A bit of its own: the
                           * split-f16 copy of ISI_CONV_W16 at the same address would give silently wrong products.      */
#define ISI_CONV_W16 16   /* with ISI_CONV_F16X3: the packed weight is followed in memory by its split-f16 pair copy
                           * (isi_split_conv_weight_f16 written at packed_w + the packed size in floats: the weights'
                           * pieces are then prepared once instead of every time a tile is staged; same results bit
                           * for bit).  Ignored by the launches that do not run split products.          */

/* Activations as split-f16 PAIRS (with ISI_CONV_F16X3 | ISI_CONV_W16): an element's 4 bytes hold hi = f16(4 x) in the
 * low half and lo = f16(4 x - hi) in the high half, the pieces the split-f16 kernels otherwise compute from the fp32
 * value every time they stage it (once per tap and output tile).  A producer writes them once in its epilogue
 * (ISI_CONV_OUT_PAIR), a consumer reads them with a de-interleave (ISI_CONV_IN0_PAIR / ISI_CONV_IN1_PAIR per source).
 * Both need the launch to run the split-f16 kernel with pack-time weight pieces (ISI_CONV_F16X3 | ISI_CONV_W16, vectorised
 * channels-last sources, Cout > 32, K >= 128; the fused residual block likewise) -- the 2-channel first layer can write
 * them too; other launches return ISI_E_UNSUPPORTED.
 * Same matrix operands bit for bit; a residual-block skip connection reads (hi + lo) / 4, within 2^-24 of x.
 * isi_pair_encode_f32 / isi_pair_decode_f32 convert whole tensors (tests, boundaries).                        */
#define ISI_CONV_IN0_PAIR 32
#define ISI_CONV_IN1_PAIR 64
#define ISI_CONV_OUT_PAIR 128
int isi_pair_encode_f32(const float *x, float *pairs, int64_t n, void *stream);
int isi_pair_decode_f32(const float *pairs, float *x, int64_t n, void *stream);

/* Conv2d, groups=1, square stride, symmetric zero padding, fp32.
 *   out = [relu]( conv(cat(src0, src1), W) + bias [+ residual] )
 * src1.ptr may be NULL (single source); residual.ptr may be NULL.  `residual`
 * has the logical shape of the output.  `packed_w` comes from
 * isi_pack_conv_weight_f32.  Replaces nn.Conv2d (+ nn.ReLU, + the residual add
 * and torch.cat) at encoder_decoder.py:22-35,95-112,138 and vqvae.py:260,270-272,282. */
int isi_conv2d_f32(const isi_src *src0, const isi_src *src1,
                   const float *packed_w, const float *bias,
                   const isi_src *residual, const isi_dst *dst, int B, int H,
                   int W, int Cout, int KH, int KW, int stride, int pad,
                   int relu, void *stream);

/* ConvTranspose2d(kernel 4, stride 2, padding 1), groups=1, fp32:
 *   out[B, 2H, 2W, Cout] = [relu]( convT(src, W) + bias )
 * computed as four stride-1 2x2 phase convolutions.  `packed_w` comes from
 * isi_pack_convT_k4s2_weight_f32.  Replaces nn.ConvTranspose2d (+ nn.ReLU) at
 * encoder_decoder.py:199-215 and vqvae.py:193-201. */
int isi_conv_transpose2d_k4s2_f32(const isi_src *src, const float *packed_w,
                                  const float *bias, const isi_dst *dst, int B,
                                  int H, int W, int Cout, int relu,
                                  void *stream);

/* The decoder's tail in the pair pipeline (RosinalityDecoder, vqvae/encoder_decoder.py:196-209):
 *   ConvTranspose2d(Cin -> Cmid = 64, k4 s2 p1) + ReLU + ConvTranspose2d(64 -> Cout <= 2, k4 s2 p1)
 * without the [B, 2H, 2W, 64] activation between them: the first kernel projects every pixel of its result onto the
 * second layer's 16 taps x Cout outputs while it still sits in registers (Y', 32 floats per pixel), the second one is
 * left with the col2im sum.  in_pair: dense channels-last pair-format [B, H, W, Cin]; packed_w1: the packed phase
 * matrices of layer 1 followed by their split-f16 pair copy (isi_pack_convT_k4s2_weight_f32 + isi_split_conv_weight_f16);
 * packed_w2: the packed weight of layer 2 ([16 Cout][64], isi_pack_convT_k4s2_weight_f32); yprime_ws: workspace of
 * B * 2H * 2W * 32 floats; dst: [B, Cout, 4H, 4W] fp32, arbitrary strides.  Same products as the two calls of
 * isi_conv_transpose2d_k4s2_f32 (ISI_CONV_F16X3 | ISI_CONV_W16, pair hand-over), other summation order. */
int isi_decoder_tail_f32(const float *in_pair, const float *packed_w1, const float *bias1, const float *packed_w2,
                         const float *bias2, float *yprime_ws, const isi_dst *dst, int B, int H, int W, int Cin, int Cmid,
                         int Cout, void *stream);

/* Fused RosinalityResBlock on a rectified input r (encoder_decoder.py:22-35):
 *   out = [relu]( r + conv1x1(relu(conv3x3(r) + b3)) + b1 )
 * in/out dense channels-last [B,H,W,C]; packed_w3 = isi_pack_conv_weight_f32 of
 * conv.1 ([R,C,3,3]), packed_w1 of conv.3 ([C,R,1,1]).  Available when
 * isi_resblock_fusable(C, R) (C % 32 == 0, C <= 128, R <= 32); otherwise compose
 * two isi_conv2d_f32 calls. */
int isi_resblock_fusable(int C, int R);
int isi_resblock_f32(const float *in, const float *packed_w3, const float *b3,
                     const float *packed_w1, const float *b1, float *out, int B,
                     int H, int W, int C, int R, int relu, void *stream);

/* Training-mode forms of the pair pipeline's producers (train_vqvae.py:168-181: `out, latent_loss, ... = model(img)` under
 * model.train()): the same launches as isi_conv2d_f32 / isi_conv_transpose2d_k4s2_f32 / isi_resblock_f32 with
 * ISI_CONV_F16X3 | ISI_CONV_W16 | ISI_CONV_OUT_PAIR (pair-format sources, except the 2-channel first layer), which ALSO
 * write what the hand-written backward reads back -- `twin`: the output once more as dense channels-last fp32
 * [B,OH,OW,Cout] (weight-gradient operand, ReLU masks); `hidden` (residual block): relu(conv3x3(r) + b3) as dense fp32
 * [B,H,W,R].  The next layer keeps staging the pair tensor by LDS-DMA; nothing is converted twice.  Launches that would
 * not reach a kernel with the twin epilogue return ISI_E_UNSUPPORTED (ask the *_route predicates first: 1 = yes). */
int isi_conv2d_twin_f32(const isi_src *src0, const isi_src *src1, const float *packed_w, const float *bias,
                        const isi_dst *dst, float *twin, int B, int H, int W, int Cout, int KH, int KW, int stride,
                        int pad, int flags, void *stream);
int isi_conv_transpose2d_k4s2_twin_f32(const isi_src *src, const float *packed_w, const float *bias, const isi_dst *dst,
                                       float *twin, int B, int H, int W, int Cout, int flags, void *stream);
int isi_resblock_tape_f32(const float *in, const float *packed_w3, const float *b3, const float *packed_w1, const float *b1,
                          float *out, float *twin, float *hidden, int B, int H, int W, int C, int R, int flags, void *stream);
int isi_conv2d_pair_route(int C0, int C1, int Cout, int KH, int KW);
/* 1 if isi_conv_wgrad_torch_f32 (three-term products, dense channels-last operands) would run the halo-staged kernel for
 * this plain convolution -- the weight-gradient kernel that also reads PAIR-format sources: flags ISI_CONV_IN0_PAIR /
 * ISI_CONV_IN1_PAIR in the flag word of isi_conv_wgrad_f32 / _torch_f32 / _deferred_f32 (other launches: ISI_E_UNSUPPORTED). */
int isi_conv_wgrad_halo_route(int Cout, int C0, int C1, int KH, int KW, int stride, int pad, int OH, int OW);
int isi_conv_transpose2d_pair_route(int Cin, int Cout);
int isi_resblock_pair_route(int B, int H, int W, int C, int R);

/* ----------------------------------------------------- training (backward) */
/* These replace the autograd kernels behind `loss.backward()` (train_vqvae.py:181)
 * and the in-forward EMA codebook update (vqvae/bottleneck.py:79-92).
 * Input gradients of the convolutions reuse the forward entry points:
 *   d/dx Conv2d(k, s=1)      = isi_conv2d_f32 with the flipped / transposed weight
 *   d/dx Conv2d(k4,s2,p1)    = isi_conv_transpose2d_k4s2_f32 with the same weight tensor
 *   d/dx ConvTranspose(k4s2) = isi_conv2d_f32(k4,s2,p1) with the same weight tensor. */

/* The two convolutions with a GATED epilogue: out = gate > 0 ? (conv + bias + residual) : 0, where `gate` is an fp32
 * tensor laid out exactly like `dst` (same strides).  With gate = the rectified activation a layer consumed, the
 * input-gradient convolution applies that ReLU's backward mask itself (autograd's threshold_backward behind
 * train_vqvae.py:181; encoder_decoder.py:24,31,95-112 `nn.ReLU`) instead of a separate pass over the gradient.
 * fp32 tensors only (no ISI_CONV_*_PAIR), one launch (the implicit-GEMM kernels). */
#define ISI_CONV_GATE_PAIR 512 /* the gate of a gated convolution is a pair-format tensor (ISI_CONV_OUT_PAIR layout, same shape
                                * and strides as the output): an element passes where its hi piece is positive -- the training
                                * forward's pair tensors serve as ReLU masks without an fp32 copy (Cout % 8 == 0) */
int isi_conv2d_gated_f32(const isi_src *src0, const isi_src *src1, const float *packed_w,
                         const float *bias, const isi_src *residual, const float *gate,
                         const isi_dst *dst, int B, int H, int W, int Cout, int KH, int KW,
                         int stride, int pad, int flags, void *stream);
int isi_conv_transpose2d_k4s2_gated_f32(const isi_src *src, const float *packed_w,
                                        const float *bias, const float *gate, const isi_dst *dst,
                                        int B, int H, int W, int Cout, int flags, void *stream);

/* Which kernel would the call run?  The arguments of isi_conv2d_gated_f32 / isi_conv_transpose2d_k4s2_gated_f32 (`gate`
 * may be NULL: the plain call), the same validation and planning, NOTHING launched and no device asked (pointers are
 * looked at for null-ness and alignment only).  Returns a negative status where the call would be refused, else
 *   family | (BN / 32) << 4 | MODE << 8 | PREC << 10 | OUTP << 13 | slice_major << 14
 * family = ISI_CONV_ROUTE_IGEMM: the implicit-GEMM kernel's instance -- BN: tile width 32 / 64 / 128; MODE: loader,
 * 0 uniform (vectorised channels-last sources, a 32-wide K chunk inside one source), 1 dual-source, 2 scalar gather;
 * PREC: products, 0 exact fp32, 1 bf16x3, 2 bf16x6, 3 f16x3, 4 f16x3 with the pack-time weight pieces; OUTP: pair-format
 * output; slice_major: K walked slice-major (for each 32-channel slice all taps) instead of tap-major.
 * Every other family is a hand-off to a kernel of its own, reported and not looked into (the other fields are 0).
 * Rules the answer makes visible: only the uniform loader runs split products -- a split flag on a dual-source or
 * gather launch is IGNORED (PREC 0, exact fp32), as it is for K < 128 (bf16x3 at Cout > 32: K < 64; at Cout <= 32 bf16x3
 * needs K >= 128 like the other modes); with Cout <= 32 there is no PREC 4 instance: ISI_CONV_W16 reports PREC 3 and the weight pieces are not read (same results bit for bit). */
#define ISI_CONV_ROUTE_IGEMM 1            /* conv_igemm_f32_kernel                                                  */
#define ISI_CONV_ROUTE_PAIR_DMA 2         /* the LDS-DMA kernel of the pair pipeline (isi_conv2d_pair_route shapes)   */
#define ISI_CONV_ROUTE_FIRST 3            /* the 2-channel first layer's kernel                                     */
#define ISI_CONV_ROUTE_GEMM 4             /* a dense 1x1 over rows: the linear layers' GEMM (isi_linear_route)      */
#define ISI_CONV_ROUTE_CONVT_SMALL 5      /* transposed, few output channels: GEMM + col2im gather                  */
#define ISI_CONV_ROUTE_CONVT_SMALL_PAIR 6 /* ... its pair-format-input form                                         */
#define ISI_CONV_ROUTE_CONVT_PAIR 7       /* transposed: the fused-phase LDS-DMA kernel (isi_conv_transpose2d_pair_route) */
int isi_conv2d_route(const isi_src *src0, const isi_src *src1, const float *packed_w, const float *bias,
                     const isi_src *residual, const float *gate, const isi_dst *dst, int B, int H, int W, int Cout,
                     int KH, int KW, int stride, int pad, int flags);
int isi_conv_transpose2d_k4s2_route(const isi_src *src, const float *packed_w, const float *bias, const float *gate,
                                    const isi_dst *dst, int B, int H, int W, int Cout, int flags);

/* Weight gradient dW (packed like the forward weight: [nphase][Cout][Kpad]) of a
 * convolution (transposed = 0) or ConvTranspose2d(k4,s2,p1) (transposed = 1) whose input
 * was cat(src0, src1) [B,*,H,W] and whose output gradient is dy, dense channels-last
 * [B, OH, OW, Cout] (transposed: [B, 2H, 2W, Cout]).  Deterministic split reduction;
 * workspace of isi_conv_wgrad_workspace_floats(Cout, K, M, nphase) floats with
 * K = KH*KW*Cin (transposed: 4*Cin), M = B*OH*OW (transposed: B*H*W), nphase = 1 (4).
 * db [Cout] (optional) receives the bias gradient = column sums of dy, computed on the
 * staged dY tiles at no extra pass.  `transposed` is a flag word: bit 0 = transposed
 * convolution, ISI_CONV_BF16X3 / ISI_CONV_BF16X6 select split-bf16 products (vectorised
 * channels-last operands only; other layouts use the fp32 pipe). */
size_t isi_conv_wgrad_workspace_floats(int Cout, int K, int M, int nphase);
int isi_conv_wgrad_f32(const isi_src *src0, const isi_src *src1, const float *dy,
                       float *dw_packed, float *db, float *workspace, size_t workspace_floats,
                       int B, int H, int W, int Cout, int KH, int KW, int stride, int pad,
                       int transposed, void *stream);
/* The same gradient written in torch's weight layout [Cout][cin_keep][KH][KW] (the parameter's own `.grad`
 * storage: no packed intermediate, no permuting copy): the k padding and the input channels >= cin_keep (a source
 * zero-padded to a multiple of 4 channels) are dropped.  Plain convolutions only (bit 0 of `flags` clear); a
 * ConvTranspose2d's gradient is the adjoint stride-2 convolution's with the roles of input and output gradient
 * swapped (train_vqvae.py:181 via autograd; vqvae/_train.py conv_wgrad). */
int isi_conv_wgrad_torch_f32(const isi_src *src0, const isi_src *src1, const float *dy,
                             float *dw_torch, int cin_keep, float *db, float *workspace,
                             size_t workspace_floats, int B, int H, int W, int Cout, int KH, int KW,
                             int stride, int pad, int flags, void *stream);
/* The same call with its split REDUCTION deferred (round 5): the pixel-reduction GEMM is launched, the sum over its splits
 * (into dw_torch / db) is returned as up to 4 jobs in `jobs_out` instead of being launched behind it.  The caller runs the
 * jobs of many layers in one launch (isi_reduce_jobs_f32: the job table travels in the kernel arguments, 48 jobs per
 * launch) before anything reads the gradients -- the end of the step, or a data-parallel bucket's all-reduce -- and keeps
 * every `workspace` alive until then.  A VQ-VAE training step ran 31 reduction launches of ~9 us (train_vqvae.py:181). */
typedef struct isi_reduce_job {
  const float *partial;     /* [nsplit] slices of `stride` floats                                   */
  float *out;               /* n floats (or the torch-layout weight gradient when map_Kpad != 0)    */
  int64_t n, stride;
  int32_t nsplit, accumulate, vec;
  int32_t map_K, map_Kpad, map_cin, map_taps, map_keep;   /* packed [Cout][Kpad] -> torch [Cout][keep][taps] */
} isi_reduce_job;
int isi_conv_wgrad_deferred_f32(const isi_src *src0, const isi_src *src1, const float *dy, float *dw_torch, int cin_keep,
                                float *db, float *workspace, size_t workspace_floats, int B, int H, int W, int Cout, int KH,
                                int KW, int stride, int pad, int flags, void *stream, isi_reduce_job *jobs_out, int *n_jobs);
int isi_reduce_jobs_f32(const isi_reduce_job *jobs, int n_jobs, void *stream);

/* ------------------------------------------------ Adam with device-resident hyper-parameters */
/* `optim.Adam(params, lr, eps)` + `clip_grad_norm_` + `optimizer.step()` of the training scripts (train_vqvae.py:181-192,777,
 * train_autoregressive_model.py:256-263,624-640): plain Adam, no amsgrad, no weight decay.  Per element:
 *   g' = g * coef;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g' g';  p -= step_size * m / (sqrt(v) * inv_sqrt_bc2 + eps)
 * g' is an fp32 product (clip_grad_norm_ scales the fp32 gradient); the three other lines are evaluated in double from the
 * double hyper-parameters and each result is rounded to fp32 once (torch's fused Adam evaluates its moment lines in double
 * too: its betas are doubles).  Note that m and v of the p line are the unrounded double values.
 * Every per-step quantity is READ FROM DEVICE MEMORY: `hyper` [n_groups] (one isi_adam_hyper per param group, written by the
 * host in double: step_size = lr / (1 - b1^t), inv_sqrt_bc2 = 1 / sqrt(1 - b2^t); the step count is the host's) and `coef` (NULL: 1).  A step recorded into a HIP graph therefore follows any host-side schedule of lr and
 * betas (utils/training/scheduler.py CycleScheduler moves beta1 every step): the host rewrites 64 bytes per group before a
 * replay.  The tensor table travels by value in the kernel arguments (64 entries per launch; no address lives in device
 * memory).  Every tensor is cut into chunks of 2048 elements counted from its own start, one workgroup each; a chunk whose
 * four addresses agree mod 16 moves 16 bytes per lane (with < 4 leading / trailing elements one by one), any other chunk
 * element by element -- sliced parameters and gradients that are views into a flat bucket need no copy.
 * Global-norm clipping: isi_grad_sumsq_f32 writes sum(g^2) of every chunk to partials[isi_adam_num_chunks(table)] (same
 * table form; only g and n are read), isi_grad_clip_coef_f32 (one workgroup, fixed order, double accumulation) writes
 * norm_coef[0] = total_norm and norm_coef[1] = min(1, max_norm / (total_norm + 1e-6)); pass &norm_coef[1] as `coef`.  No
 * atomics: results are bit-reproducible.  A non-finite norm gives a non-finite coefficient and propagates into p, like
 * clip_grad_norm_(error_if_nonfinite=False).  g itself is left unscaled.
 * Checked before any launch: ISI_E_INVALID for a null table / pointer, n <= 0, a pointer not aligned to a float, a group
 * outside [0, n_groups), n_groups <= 0, a null hyper block, n_partials != isi_adam_num_chunks, max_norm <= 0 or NaN;
 * ISI_E_UNSUPPORTED for a tensor beyond 2^35 elements.  An empty table is a no-op for isi_adam_step_f32. */
typedef struct isi_adam_tensor {
  float *p;                 /* parameter, n floats                    */
  const float *g;           /* its gradient                           */
  float *m, *v;             /* exp_avg, exp_avg_sq                    */
  int64_t n;
  int32_t group;            /* index into `hyper`                     */
  int32_t reserved;
} isi_adam_tensor;
typedef struct isi_adam_hyper {
  double b1, one_minus_b1, b2, one_minus_b2, eps, step_size, inv_sqrt_bc2, reserved;
} isi_adam_hyper;
int64_t isi_adam_num_chunks(const isi_adam_tensor *tensors, int n_tensors);
int isi_grad_sumsq_f32(const isi_adam_tensor *tensors, int n_tensors, float *partials, int64_t n_partials, void *stream);
int isi_grad_clip_coef_f32(const float *partials, int64_t n_partials, float max_norm, float *norm_coef, void *stream);
int isi_adam_step_f32(const isi_adam_tensor *tensors, int n_tensors, const isi_adam_hyper *hyper, int n_groups,
                      const float *coef, void *stream);
/* The element-wise operators below read and write float4: a call whose arguments do not fit is refused with
 * ISI_E_INVALID before any launch (tests/test_train_ops_host.py), never run on a slower path.
 * dy = y > 0 ? dy : 0 (a selection: a NaN of dy under the mask gives 0): ReLU backward through an output rectified in
 * the producer's epilogue.  Any n >= 0; dy and y 16-byte aligned. */
int isi_relu_bwd_f32(float *dy, const float *y, int64_t n, void *stream);
/* a += alpha * b.  n % 4 == 0; a and b 16-byte aligned. */
int isi_axpy_f32(float *a, const float *b, float alpha, int64_t n, void *stream);
/* Quantiser backward (bottleneck.py:94-95): dz = dq + 2 g_diff (z - q_st) / n.  n > 0, n % 4 == 0; dz, dq, z and q_st
 * 16-byte aligned (g_diff: one float on the device). */
int isi_vq_bwd_f32(float *dz, const float *dq, const float *z, const float *q_st,
                   const float *g_diff, int64_t n, void *stream);
/* out[m][c] = (y[m][c] > 0) * (a[m][c] + b[m][c]) over M rows of C channels: two gradient contributions summed and masked by
 * the ReLU of the tensor they belong to in one pass; `a` may be a channel slice of a wider channels-last tensor (row stride
 * lda), b / y dense [M, C] or NULL (no second term / no mask).  Same, for the quantiser backward, with dq read through a
 * row stride (isi_vq_bwd_f32 on a channel slice without a dense copy first).  C (D) and lda (ldq) multiples of 4,
 * lda >= C (ldq >= D); every pointer given 16-byte aligned. */
/* src [B, C <= 4, H, W] (any strides) -> dense channels-last [B, H, W, 4] with the channels >= C zero: the 2-channel
 * spectrogram side as an operand of the vectorised weight-gradient kernels (train_vqvae.py:181 through vqvae/_train.py). */
int isi_pad_channels4_f32(const isi_src *src, float *out_nhwc4, int B, int H, int W, void *stream);
int isi_add_gate_rows_f32(float *out, const float *a, int64_t lda, const float *b, const float *y, int64_t M, int C, void *stream);
int isi_vq_bwd_rows_f32(float *dz, const float *dq, int64_t ldq, const float *z, const float *q_st, const float *g_diff,
                        int64_t M, int D, void *stream);
/* Reconstruction loss of the VQ-VAE training step (reference train_vqvae.py:168-176, `nn.MSELoss()`): out[0] = mean((a - b)^2)
 * over n elements (dense, 16-byte aligned), fixed summation order; `workspace`: isi_mse_loss_num_partials(n) floats.
 * Backward: da = 2 (a - b) g[0] / n, db = -da (either may be null); g: the incoming scalar gradient on the device. */
int isi_mse_loss_num_partials(int64_t n);
int isi_mse_loss_f32(const float *a, const float *b, int64_t n, float *workspace, float *out, void *stream);
int isi_mse_loss_bwd_f32(const float *a, const float *b, const float *g, int64_t n, float *da, float *db, void *stream);

/* out[C] = column sums of x [M, C] (bias gradients); workspace isi_colsum_num_partials(M)*C floats.  x_stride >= C (floats
 * between rows; less is refused); no alignment requirement: a dense, 16-byte aligned x with C a power of two <= 1024 and
 * M * C % 4 == 0 is streamed as float4, everything else by scalar loads.  Fixed summation order on either route. */
int isi_colsum_num_partials(int64_t M);
int isi_colsum_f32(const float *x, int64_t x_stride, float *out, float *workspace, int64_t M,
                   int C, void *stream);
/* embed_sum_dk [D,K] = z^T @ onehot(idx) (bottleneck.py:83): the pixel-reduction GEMM of
 * isi_conv_wgrad_f32 with the one-hot operand generated on the fly (never materialised);
 * deterministic.  workspace: isi_vq_embed_sum_workspace_floats(D, K, N) floats. */
size_t isi_vq_embed_sum_workspace_floats(int D, int K, int64_t N);
int isi_vq_embed_sum_f32(const float *z, const int64_t *idx, float *embed_sum_dk,
                         float *workspace, size_t workspace_floats, int64_t N, int D, int K,
                         void *stream);
/* EMA codebook update (bottleneck.py:80-92) on the [D,K] buffers from batch statistics
 * counts [K] (float) and embed_sum_dk [D,K] (all-reduced across ranks by the caller). */
int isi_vq_ema_update_f32(float *embed, float *cluster_size, float *embed_avg,
                          const float *counts, const float *embed_sum_dk, int D, int K,
                          float decay, float eps, void *stream);
/* EMA codebook with random restarts of dead codes (QuantizedBottleneckWithRestarts; the
 * specification is DESIGN.md's and tests/restarts_spec.py's).  restart_state: device int64 [4] =
 * {seed, step, restarts at the last step, restarts in total}.
 * isi_vq_restart_row: the batch row code k is redrawn from (host export of the function the
 * kernel calls): mix(mix(seed ^ mix(step)) + k) mod N, mix = splitmix64's finaliser.
 * isi_vq_restart_candidates_f32: cand_out [K*D + K] = the candidate vector of every code
 * k with k mod world == rank, gathered from this rank's z [N,D] (zeros for the other codes),
 * followed by K flag words (1.0f: the chosen row has a non-finite component and was written
 * as zeros).  seed and step are read from restart_state on the device.
 * isi_vq_ema_update_restart_f32: isi_vq_ema_update_f32 that replaces every code whose updated
 * cluster size is below `threshold` (every code when `initialize` and step == 0), unless
 * flagged, by its candidate: cluster_size = threshold, embed_avg = threshold * cand, embed = cand
 * exactly.  cand: [K*D + K] as written above (summed over the ranks).  Advances
 * restart_state.  K <= 65536. */
uint64_t isi_vq_restart_row(uint64_t seed, uint64_t step, int k, int64_t N);
int isi_vq_restart_candidates_f32(const float *z, int64_t N, int D, int K,
                                  const int64_t *restart_state, int rank, int world,
                                  float *cand_out, void *stream);
int isi_vq_ema_update_restart_f32(float *embed, float *cluster_size, float *embed_avg,
                                  const float *counts, const float *embed_sum_dk,
                                  const float *cand, int D, int K, float decay, float eps,
                                  float threshold, int initialize, int64_t *restart_state,
                                  void *stream);

/* ------------------------------------------------------ transformer prior */
/* The prior's layers are instantiated by the reference from the absent package
 * VQCPCB.transformer.transformer_custom (priors/transformer.py:12-15,370-417);
 * their arithmetic is specified in oracle/prior_oracle.py (parity unpinned). */

/* Multi-head attention with relative-position logits, flash style:
 *   logit[i,j] = (q_i.k_j + q_i.e[h, r(i,j)]) * scale + mask(i,j)
 *   r(i,j) = floor(i/Cq) - floor(j/Ck) + Ek - 1 ;  out_i = softmax_j(logit) v_j
 * q/k/v/out are addressed as [seq, batch, head, head_dim] with element strides
 * (ss, sb, sh) and contiguous head_dim (16, 32 or 64).  rel_embeddings
 * [H, rel_rows, head_dim] may be NULL (no bias).  mask_mode: 0 none, 1 causal
 * (j <= i), 2 anti-causal (j >= i); dense_mask [Sq,Sk] additive, may be NULL (an entry may be -inf: that pair has
 * weight 0).  A query row with no allowed pair, or with only -inf logits (anti-causal rows beyond the last key, an all -inf
 * row of dense_mask) is an EMPTY row: every kernel writes out = 0 and lse = 1e30f for it, no NaN. */
typedef struct isi_attn_args {
  const float *q, *k, *v, *rel_embeddings, *dense_mask;
  float *out;
  int Sq, Sk, B, H, head_dim;
  int64_t q_ss, q_sb, q_sh, k_ss, k_sb, k_sh, v_ss, v_sb, v_sh, o_ss, o_sb, o_sh;
  int Cq, Ck, Ek, rel_rows;
  int mask_mode;
  float scale;
  float *lse;   /* optional [B,H,Sq]: log-sum-exp of every query's logits (kept for the backward) */
  int precision; /* products of the three contractions: 0 = fp32 matrix pipe, 1 = three-term split-bf16
                  * (hi.hi + hi.lo + lo.hi on the bf16 pipe, fp32 accumulation; logits / softmax fp32),
                  * 2 = single-term bf16 (operands rounded to bf16, fp32 accumulation / logits / softmax),
                  * 3 = single-term f16 (operands rounded to f16: 11 significand bits, |q k v e| < 65504; error
                  * ~4e-4 of the output's maximum where mode 2 gives ~3e-3; its backward runs three-term products) */
  float *logits; /* optional [B,H,Sq,logits_ld] (16-bit modes only, precision >= 1): the forward stores the logit of every
                  * (query, key) pair the mask allows -- (q.k + q.e[r]) * scale * log2(e) + mask * log2(e), i.e. in units
                  * of exp2; -inf where dense_mask is; the rows of the one-row tail kernel included -- and isi_rel_attention_bwd_f32, handed the same buffer, reads them instead of forming
                  * Q K^T, the band product Q E^T and its skew a second and a third time (60 % of the backward's time at
                  * S = 1025).  Entries of masked pairs are never read.  NULL: nothing is stored / everything is recomputed */
  int64_t logits_ld; /* row stride of `logits` in floats: a multiple of 4, >= Sk rounded up to a multiple of 32 */
  void *workspace;   /* optional, isi_rel_attention_workspace_bytes(args) bytes, 256-byte aligned, forward only: with it the
                      * 16-bit modes (precision >= 1, Cq = Ck = 1, head_dim 32 / 64) first split K, V and the table into
                      * 16-bit planes (one launch) and then run the LDS-DMA-staged kernel (rel_attention_fwd3.hip) on them;
                      * same arithmetic and results as without.  NULL: the register-staged kernels. */
  size_t workspace_bytes;
} isi_attn_args;
int isi_rel_attention_f32(const isi_attn_args *args, void *stream);
/* 0 when the call would not use a workspace (precision 0, several channels per event, head_dim 16, planes >= 2 GiB) */
size_t isi_rel_attention_workspace_bytes(const isi_attn_args *args);

/* Backward of isi_rel_attention_f32 (replaces autograd through the attention of the absent
 * VQCPCB.transformer.transformer_custom behind `loss.backward()`,
 * train_autoregressive_model.py:257).  fwd = the forward call's arguments with out = its
 * output and lse = the log-sum-exp it wrote.  d_out has the strides of out; dq / dk / dv
 * are written with the strides of q / k / v (e.g. slices of one [S,B,3d] buffer); d_rel
 * [H, rel_rows, head_dim] is overwritten (NULL iff rel_embeddings is NULL).  workspace:
 * isi_rel_attention_bwd_workspace_floats(&fwd) floats, 16-byte aligned.  dK and dV are
 * reduced in a fixed order on every route (no atomics), dQ and dE whenever Ck == 1 or there is no
 * table: every element of G then receives at most one term.  With several channels per key event
 * (Ck > 1) the keys of one event are added into their element of G with float atomics -- by the
 * lanes of one wave instruction, and in the split pair (precision >= 1) by two waves where an event
 * straddles a 32-key tile (32 % Ck != 0) -- in an order the hardware chooses: dQ (through G E) and
 * dE may then differ in their last bits between two calls. */
typedef struct isi_attn_bwd_args {
  isi_attn_args fwd;
  const float *d_out;
  float *dq, *dk, *dv, *d_rel;
  float *workspace;
  size_t workspace_floats;
} isi_attn_bwd_args;
size_t isi_rel_attention_bwd_workspace_floats(const isi_attn_args *fwd);
int isi_rel_attention_bwd_f32(const isi_attn_bwd_args *args, void *stream);

/* isi_layernorm_f32 / isi_layernorm_bwd_f32 with the dropout that precedes the residual add in the absent package's
 * layers folded in (train mode): out = LayerNorm(drop(x) + residual), drop = inverted dropout whose keep mask is a
 * counter-based hash of (drop_seed, flat element index) -- the same function the backward evaluates again, so no mask
 * is stored and no dropout kernel runs.  The backward returns dz = d loss / d (drop(x) + residual) (the residual's
 * gradient) and dx = the gradient of x (dz where kept, scaled by 1 / (1 - drop_p)).  drop_p = 0: the plain kernels. */
int isi_layernorm_dropout_f32(const float *x, const float *residual, const float *gamma, const float *beta,
                              float *out, int64_t M, int D, float eps, float drop_p, uint64_t drop_seed,
                              void *stream);
int isi_layernorm_dropout_bwd_f32(const float *x, const float *residual, const float *gamma, const float *dy,
                                  float *dz, float *dx, float *dgamma, float *dbeta, float *workspace, int64_t M,
                                  int D, float eps, float drop_p, uint64_t drop_seed, void *stream);

/* A device-resident 64-bit term added to the seed of every fused dropout (the linear layer's epilogue, the LayerNorm
 * kernels): a training step replayed from a HIP graph carries its seeds as launch constants, so the owner of the graph
 * advances this counter between replays (one element-wise add inside the graph) to draw fresh masks per step.  The
 * forward and backward launches of one step read the same value.  NULL (the default) = no such term.  Process-wide. */
int isi_set_dropout_seed_base(const void *device_u64);

/* One linear layer of the prior (`nn.Linear` inside the absent package's layers, priors/transformer.py:370-417): rows
 *   out[m, n] = sum_k x[m, k] w[n, k] + bias[n] (+ residual[m, n]) (ReLU) (gate) (dropout)
 * on the split-product GEMM kernel, with the element-wise tails of a training step folded into its epilogue:
 *   gate       out = gate[m, n] > 0 ? value * gate_scale : 0  -- a ReLU's backward mask (and the inverse keep probability
 *              of a dropout that followed the ReLU) applied by the input-gradient GEMM;
 *   drop_p     inverted dropout of the (rectified) output: element (m, n) is kept iff a counter-based hash of
 *              (drop_seed, m * ldo + n) clears drop_p, kept values are scaled by 1 / (1 - drop_p).  The mask is a pure
 *              function of (seed, index): nothing is stored; a dropped element of a rectified output is 0 and gates its
 *              own gradient.  (`F.dropout` in train mode: same distribution, not torch's random stream.)
 * flags: ISI_CONV_RELU | one of ISI_CONV_BF16X3 / ISI_CONV_F16X3 | ISI_CONV_W16 as for isi_conv2d_f32.  Shapes the GEMM
 * kernel does not take (K % 32, K < 128, N <= 32, M < 256) return ISI_E_UNSUPPORTED: the caller keeps isi_conv2d_f32.
 * Refused before any launch: a row stride shorter than its row (ldx < K, ldo < N, a residual's ldr < N) and drop_p < 0 or
 * NaN: ISI_E_INVALID; drop_p >= 1, a gate's ldg < N, and x, out, residual, gate or the weight spanning more than
 * 2^30 - 4 elements ((M - 1) ld + width; the kernel's byte offsets are 32-bit and 2^32 - 16 marks "out of range"):
 * ISI_E_UNSUPPORTED. */
typedef struct isi_linear_args {
  const float *x;
  int64_t ldx;
  const float *packed_w, *bias, *residual;
  int64_t ldr;
  const float *gate;
  int64_t ldg;
  float gate_scale;
  float *out;
  int64_t ldo;
  int M, N, K, flags;
  float drop_p;
  uint64_t drop_seed;
} isi_linear_args;
int isi_linear_f32(const isi_linear_args *args, void *stream);
/* Which kernel isi_linear_f32 would launch for this shape on the current device, nothing launched:
 * 0 = refused (outside the GEMM kernel); else tile | tail_rows << 8 with tile 1 = 128x64, 2 = 128x128,
 * 3 = 256x128, 4 = 256x256.  Reads the device's CU count and ISI_GEMM_NARROW_BELOW / ISI_GEMM_NO_WIDE. */
int isi_linear_route(int M, int N, int K, int flags);

/* Backward of isi_layernorm_f32: dz = d loss / d (x + residual) (the gradient of both x and
 * residual), dgamma / dbeta [D] (overwritten; deterministic two-stage reduction).
 * workspace: isi_layernorm_bwd_workspace_floats(M, D) floats. */
size_t isi_layernorm_bwd_workspace_floats(int64_t M, int D);
int isi_layernorm_bwd_f32(const float *x, const float *residual, const float *gamma, const float *dy,
                          float *dz, float *dgamma, float *dbeta, float *workspace, int64_t M,
                          int D, float eps, void *stream);

/* LabelSmoothingLoss (utils/losses/prediction.py:5-20) over rows of logits [M,K] with
 * int64 targets [M]: row_loss[m] = sum_k -true_dist[k] log_softmax(logits[m])[k]; when
 * dlogits is not NULL also (softmax * sum_k true_dist[k] - true_dist) * grad_scale (the
 * gradient of the mean loss for grad_scale = upstream / M), in the same pass.  true_dist is
 * smoothing / (num_classes - 1) in all K columns and 1 - smoothing at the target: it sums to 1
 * for K == num_classes, and the gradient is then (softmax - true_dist) * grad_scale. */
int isi_label_smoothing_loss_f32(const float *logits, const int64_t *target, float *row_loss,
                                 float *dlogits, int64_t M, int K, int num_classes,
                                 float smoothing, float grad_scale, void *stream);


/* out[m,:] = LayerNorm(x[m,:] + residual[m,:]) * gamma + beta  (residual may be NULL). */
int isi_layernorm_f32(const float *x, const float *residual, const float *gamma,
                      const float *beta, float *out, int64_t M, int D, float eps,
                      void *stream);

/* Single-token decoding: out[m,n] = [relu](x[m,:].W[n,:] + bias[n] + residual[m,n])
 * for M <= 8 rows; W in torch layout [N,K].  (Whole sequences go through
 * isi_conv2d_f32 with a 1x1 kernel, which is a GEMM.) */
int isi_linear_rows_f32(const float *x, int x_stride, const float *W, const float *bias,
                        const float *residual, int res_stride, float *out, int out_stride,
                        int M, int N, int K, int relu, void *stream);

/* One stage of the KV-cached decoding loop on M <= 256 new rows (sample.py:268-305 -> priors/transformer.py:763-774 evaluate a
 * whole decoder pass per token; the loop evaluates its stages on the new rows only):
 *   out[m][n] = act( sum_k LN(x)[m][k] W[n][k] + bias[n] + LN_res(res)[m][n] )
 * LN = LayerNorm over the row with (ln_g, ln_b) (nullable: none), LN_res likewise with (res_g, res_b) over the N features of
 * the residual row (nullable; res nullable), act = ReLU when `relu`.  Kernels by row count: one row = one memory round trip
 * (GEMV), up to ISI_DECODE_MFMA_ROWS (16) rows the register-resident GEMV looping over groups of rows (each row: the operations and the order
 * of its one-row result), beyond that 32-row tiles on the fp32 matrix pipe (exact fp32 products, another summation order).
 * K a multiple of 4 (8 for the tiles), <= 2048; x, W 16-byte aligned.  `workspace`: isi_decode_stage_workspace_floats(M, N, K)
 * floats, 16-byte aligned (K-chunk sums of the tile kernel; may be null: the chunks then run one after the other). */
size_t isi_decode_stage_workspace_floats(int M, int N, int K);
int isi_decode_stage_f32(const float *x, int x_stride, const float *ln_g, const float *ln_b, const float *W, const float *bias,
                         const float *res, int res_stride, const float *res_g, const float *res_b, float *out, int out_stride,
                         int M, int N, int K, int relu, float eps, float *workspace, size_t workspace_floats, void *stream);

/* The same stage as the decoding loop describes it (isi_abi_struct_bytes(17) = sizeof(isi_decode_stage_args)): everything
 * isi_prior_sample_run puts into a stage's launch, so that every route of the loop's stage kernels can be run alone.
 *   columns [0, split) of the result go to `out` (row stride out_stride), columns [split, N) to `out2` (nullable: split == N),
 *   an fp32 array (out2_format = ISI_KV_F32) or a bf16 array (ISI_KV_BF16: rounded to nearest-even; 16-byte aligned);
 *   out2_stride and out2_pos count elements of that format.
 * The position: x, res and out2 move on by x_pos, res_pos, out2_pos elements per sequence position.  `p` is the position by
 * value: the host advances the pointers.  With `counter` (a device int) the kernels read the position there; `p` is then not
 * used.  With `row_pos` (device, [steps][M]) row m stands at row_pos[t * M + m], t = p (the launch gets row_pos + p * M) or
 * t = *counter (the whole array beside the counter), and moves by that position; only the batched kernels address rows so.
 * A stage none of whose addresses moves takes neither counter nor row_pos (ISI_E_INVALID).
 * The hand-off: with ln_g, stat_out ([M][2], 8-byte aligned) receives the input rows' (mean, 1 / sqrt(var + eps)); with res_g,
 * res_stat gives the residual rows' statistics, which are then not formed from the rows.
 * part (one row, K <= 512, no ln_g): the input row is the merge of an attention's key-split partials
 * [K / part_hd heads][part_ns <= 8][part_hd + 4], each (o[part_hd], max, sum, -, -); x is then not read.
 * The kernel is the loop's own choice from M, N, K, the fields and ISI_DECODE_MFMA_ROWS; `kernel` reports it (ISI_STAGE_*).
 * (The tiles take a LayerNorm over K <= 2048, and a normalised residual of more than 512 features only with res_stat.)
 * A field the chosen kernel would not read is refused (ISI_E_UNSUPPORTED, the message names it): stat_out, res_stat or part on
 * the groups-of-8 kernel, part beyond one row of K <= 512, row_pos where K > 2048.  Refusals precede every launch and
 * write nothing but `kernel`.  workspace as for isi_decode_stage_f32. */
#define ISI_STAGE_ONE_ROW 0
#define ISI_STAGE_TILES 1
#define ISI_STAGE_ROWS_IN_REGISTERS 2
#define ISI_STAGE_GROUPS_OF_8 3
#define ISI_STAGE_REFUSED 4
typedef struct isi_decode_stage_args {
  const float *x; int x_stride;
  const float *ln_g, *ln_b;
  const float *W, *bias;
  const float *res; int res_stride;
  const float *res_g, *res_b;
  float *out; int out_stride;
  void *out2; int out2_stride, out2_format;
  int split, M, N, K, relu;
  float eps;
  int p;
  const int *counter;
  const int *row_pos;
  int64_t x_pos, res_pos, out2_pos;
  float *stat_out;
  const float *res_stat;
  const float *part; int part_ns, part_hd;
  float *workspace; size_t workspace_floats;
  int kernel;              /* out */
} isi_decode_stage_args;
int isi_decode_stage_ex_f32(isi_decode_stage_args *args, void *stream);

/* The single-source cross-attention block of the loop alone (isi_prior_state.cross_out; isi_abi_struct_bytes(18)):
 *   y2[m] = LN1(y1[m]) + table[(pos_m / Cd) * table_B + m * table_sb],  stat_out[m] = (mean, 1 / sqrt(var + eps)) of y2[m]
 * for B rows of d <= 1024 features; table_B, table_sb = (B, 1), or (1, 0) for a table all rows share; stat_out nullable.
 * pos_m = p, or *counter (p then holds the same value for the host's check), or with row_pos ([steps][B], device) row m's
 * own row_pos[t * B + m], t = p or *counter; row_pos_host is its host copy.  Cd >= 1 and every pos_m / Cd < S_src, checked
 * on the host before the launch. */
typedef struct isi_decode_single_source_args {
  const float *y1, *ln_g, *ln_b, *table;
  float *y2, *stat_out;
  int p;
  const int *counter;
  const int *row_pos, *row_pos_host;
  int Cd, S_src, B, d;
  float eps;
  int table_B, table_sb;
} isi_decode_single_source_args;
int isi_decode_single_source_f32(const isi_decode_single_source_args *args, void *stream);

/* Decoding step: ONE query row per (batch, head) at sequence position q_pos
 * against args->Sk cached keys/values (same logits as isi_rel_attention_f32;
 * args->Sq, q_ss, o_ss, mask_mode and dense_mask are ignored: the caller passes
 * Sk = q_pos + 1 for causal self-attention).  With a workspace of
 * isi_rel_attention_decode_workspace_floats(B, H, head_dim) floats the keys are split
 * over up to 8 workgroups per (batch, head) and merged by a second small kernel;
 * workspace may be NULL (single workgroup per head). */
size_t isi_rel_attention_decode_workspace_floats(int B, int H, int head_dim);
int isi_rel_attention_decode_f32(const isi_attn_args *args, int q_pos, float *workspace,
                                 void *stream);
/* The same step with args->k / args->v read as bf16 arrays (one 16-bit plane, the upper half of the fp32 pattern;
 * strides in elements as before): every element is widened exactly (bits << 16), then q, the relative table,
 * logits, softmax, accumulation and out are fp32 as in isi_rel_attention_decode_f32 -- the result is that entry's on
 * keys / values rounded to bf16 beforehand, up to the order in which the keys are summed (a lane holds 8 elements of
 * a row instead of 4, so twice the rows are in flight).  Rows beyond the keys in use may hold anything.  q, k, v and
 * rel_embeddings 16-byte aligned, k / v strides multiples of 8 elements, q strides of 4 (else ISI_E_INVALID).  Same
 * workspace, same split rule.  This is the cached attention of isi_prior_state.kv_format = ISI_KV_BF16. */
int isi_rel_attention_decode_kv16_f32(const isi_attn_args *args, int q_pos, float *workspace,
                                      void *stream);
/* The same step against keys / values WITHOUT a batch dimension: every one of the args->B query rows attends the same
 * args->Sk rows of args->k / args->v (N variations of one request share the encoder memory).  args->k_sb and args->v_sb
 * must be 0 (else ISI_E_INVALID); kv_format = ISI_KV_F32 or ISI_KV_BF16 says how k / v are read (bf16 widened exactly, as
 * above).  One workgroup owns a head, a key split and a block of 16 rows and fetches every key / value / table row once
 * for all of them: the bytes read per call do not grow with B beyond the number of row blocks.  Logits, softmax and
 * accumulation in fp32 as in isi_rel_attention_decode_f32; the keys are summed in another order (equal up to rounding).
 * B 1..256, head_dim 16 / 32 / 64; q, k, v, rel_embeddings 16-byte aligned, k / v strides multiples of 4 elements (bf16:
 * 8), q strides of 4.  Rows beyond the keys in use may hold anything.  workspace:
 * isi_rel_attention_decode_shared_workspace_floats(B, H, head_dim) floats (up to 8 key splits and the merge launch of
 * the entries above), or NULL for one split.  isi_prior_state.memory_shared = 1 runs the cross-attention this way. */
size_t isi_rel_attention_decode_shared_workspace_floats(int B, int H, int head_dim);
int isi_rel_attention_decode_shared_f32(const isi_attn_args *args, int q_pos, float *workspace, int kv_format,
                                        void *stream);

/* One categorical draw per row (sample.py:286-295): logits/temperature ->
 * top_k_top_p_filtering (sample.py:36-65) -> softmax -> inverse-CDF draw with the
 * host-supplied uniform u[row] in [0, 1) (first class of non-zero probability whose
 * cumulative probability exceeds u * total; if rounding leaves none, the last such
 * class): a class removed by a filter or given as -inf is never drawn.  filtered
 * [rows, n] (optional) receives the filtered logits (-inf where removed).  n <= 1024;
 * every row has a finite logit. */
int isi_sample_row_f32(const float *logits, int stride, int rows, int n, float temperature,
                       int top_k, float top_p, const float *u, int64_t *out,
                       float *filtered, void *stream);
/* The same draw with a logit bias: row r adds bias[bias_row[r] * bias_stride + c] to logit c BEFORE temperature and
 * filters -- lg = (logit + bias) * (1 / temperature), two separately rounded fp32 operations, then isi_sample_row_f32's
 * filters and draw unchanged.  bias is a table [bias_count, bias_stride] on the device, bias_stride >= n; bias_row [rows]
 * int32 on the device picks a table row per launch row, or NULL: table row 0 on every row.  An index outside
 * [0, bias_count) (-1 by convention) means no bias for that row; the table is not read for it, whatever the value.  A
 * bias of -inf bans the class: it takes the path of a -inf logit and is never drawn.  +inf and NaN biases are outside the
 * contract (the library never reads a device array on the host: the caller checks), and every row keeps a finite biased
 * logit.  filtered receives the biased, scaled, filtered logits.  NULL bias, bias_count <= 0, bias_stride < n, stride < n
 * or isi_sample_row_f32's bad arguments: ISI_E_INVALID before any launch.  It is the decode loop's kernel and arithmetic
 * (isi_prior_code_bias, isi_prior_sample_run_bias). */
int isi_sample_row_bias_f32(const float *logits, int stride, int rows, int n, float temperature,
                            int top_k, float top_p, const float *u, int64_t *out, float *filtered,
                            const float *bias, int bias_stride, int bias_count, const int32_t *bias_row,
                            void *stream);
/* The same draw, and log_prob[row] = the MODEL's log-probability of the drawn token: log softmax of the row's raw
 * logits (temperature 1, nothing filtered, natural log, fp32) at out[row] -- the value does not depend on temperature,
 * top_k or top_p.  It is the decode loop's kernel and arithmetic (isi_prior_state.token_log_probs) and agrees bit for
 * bit with isi_token_log_prob_f32 on the same logits.  n <= 1024, stride >= n. */
int isi_sample_row_log_prob_f32(const float *logits, int stride, int rows, int n, float temperature,
                                int top_k, float top_p, const float *u, int64_t *out,
                                float *log_prob, void *stream);
/* Log-probabilities of GIVEN codes: out[r] = log softmax(logits[r, 0:n])[codes[r]] = logit - max - log sum exp(logit - max),
 * natural log, fp32; one workgroup per row, any n >= 1 (rows beyond 1024 classes are walked by 1024 threads).  The
 * reductions run in a fixed order (wave reductions, one exchange of the wave totals): for n <= 1024 the result equals
 * the in-loop value of isi_prior_state.token_log_probs bit for bit on equal logits.  A code outside [0, n) gives NaN for
 * its row and reads nothing out of range.  Null pointers, rows <= 0, n <= 0 or stride < n: ISI_E_INVALID before any launch. */
int isi_token_log_prob_f32(const float *logits, int stride, int rows, int n, const int64_t *codes, float *out,
                           void *stream);
/* Statistics of the MODEL's distribution per row (raw logits, temperature 1, nothing filtered, natural log, fp32), one
 * workgroup per row, one read of the row; any n >= 1 (beyond 1024 classes 1024 threads walk the row), stride >= n:
 *   log_prob[r]  = log softmax(logits[r, 0:n])[codes[r]] -- isi_token_log_prob_f32's arithmetic and workgroup size: equal to
 *                  it bit for bit on equal logits;
 *   entropy[r]   = -sum_i p_i ln p_i in nats; a -inf logit contributes 0;
 *   rank[r]      = the number of classes with a larger logit than codes[r], plus the number with an equal logit and a lower
 *                  index (the tie rule of isi_sample_row_f32's sort): 0 is the mode.  An integer, exact;
 *   top_codes[r, 0:top_n], top_log_probs[r, 0:top_n] = the top_n classes in descending logit order, ties by lower index, and
 *                  their log-probabilities (each bit-equal to isi_token_log_prob_f32 of that class); 0 <= top_n <= 16, and
 *                  where n < top_n the tail holds -1 and -inf.
 * Every output pointer may be NULL: that output is skipped.  codes may be NULL when log_prob and rank are.  A code outside
 * [0, n) gives NaN for log_prob and -1 for rank, reads nothing out of range and leaves the row's other outputs correct.
 * The reductions run in a fixed order (wave reductions, one exchange of the wave totals): the results are functions of the
 * row, n and the workgroup size alone.  Every row has a finite logit; NaN logits are outside the contract.  Null logits,
 * rows <= 0, n <= 0, stride < n, top_n outside 0 .. 16, or codes == NULL with log_prob or rank given: ISI_E_INVALID before
 * any launch. */
int isi_token_stats_f32(const float *logits, int stride, int rows, int n, const int64_t *codes, float *log_prob,
                        float *entropy, int32_t *rank, int top_n, int64_t *top_codes, float *top_log_probs, void *stream);

/* Native key/value-cached sampling loop of the decoder (replaces the per-token
 * full decoder pass of sample.py:268-305).  Weights are the torch-layout
 * parameters themselves ([N,K] row-major), no packing. */
#define ISI_MAX_LAYERS 16
typedef struct isi_attn_w {
  const float *in_proj_weight, *in_proj_bias;   /* [3d,d], [3d]                      */
  const float *out_proj_weight, *out_proj_bias; /* [d,d], [d]                        */
  const float *rel_embeddings;                  /* [H, rel_rows, d/H] or NULL        */
  int rel_rows;
} isi_attn_w;
typedef struct isi_decoder_layer_w {
  isi_attn_w self_attn, cross_attn;
  const float *linear1_w, *linear1_b, *linear2_w, *linear2_b;
  const float *norm1_w, *norm1_b, *norm2_w, *norm2_b, *norm3_w, *norm3_b;
} isi_decoder_layer_w;
typedef struct isi_prior_w {
  int d_model, nhead, dim_feedforward, n_layers, n_class;
  int Cd, Ed, Ce, Ee;          /* channels / events (incl. start symbol) of decoder and encoder sequences */
  isi_decoder_layer_w layers[ISI_MAX_LAYERS];
  const float *logits_w, *logits_b;             /* project_transformer_outputs_to_logits */
  const float *embed_table;                     /* [n_class, eff_dim] = Linear(Embedding) of target tokens */
  int eff_dim;
} isi_prior_w;
typedef struct isi_prior_state {
  float *x_seq;            /* [S_t, B, d] decoder input rows; rows of sampled tokens are rewritten    */
  float *kv_cache;         /* [n_layers, S_t, B, 2d] self-attention keys|values                       */
  const float *memory_kv;  /* [n_layers, S_src, B, 2d] projected encoder memory keys|values           */
  int64_t *codes;          /* [B, S] codes in sequence order (in: known codes, out: sampled)          */
  const uint8_t *mask;     /* [S] HOST array, 1 = sample this position                                */
  const float *uniforms;   /* [S, B] device, uniforms in [0,1)                                        */
  float *scratch;          /* device, isi_prior_decode_scratch_floats(w, B) floats                    */
  size_t scratch_floats;
  int S_t, S_src, S, B, start_len;
  int memory_shared;       /* 0 (default): memory_kv / cross_out carry a batch dimension.  1: all B rows share ONE source */
                           /* -- memory_kv is [n_layers, S_src, 1, 2d], cross_out [n_layers, S_src, 1, d] (below).  The    */
                           /* field takes the four bytes that padded start_len up to the next pointer: size and every      */
                           /* other offset of the struct are what they were, and a zeroed struct means 0                   */
  const float *cross_out;  /* [n_layers, S_src, B, d] or NULL: single-source cross-attention (below)          */
  int kv_format;           /* ISI_KV_F32 (0): kv_cache / memory_kv are fp32 arrays; ISI_KV_BF16 (1): bf16 arrays of  */
                           /* the same logical shape (below); anything else: ISI_E_INVALID                            */
  float *token_log_probs;  /* [B, S] device or NULL (default): beside every committed code, the model's log-probability of */
                           /* it (below); other entries are left untouched.  Appended behind kv_format: every other offset  */
                           /* is what it was, the struct grows by one pointer, and a zeroed struct means off               */
} isi_prior_state;
#define ISI_KV_F32 0
#define ISI_KV_BF16 1
size_t isi_prior_decode_scratch_floats(const isi_prior_w *w, int B);
/* Enqueues positions [p_begin, p_end) of the decoder (one new row each, all layers),
 * and for every masked position the logits head, the draw (isi_sample_row_f32
 * semantics) and the write of the sampled token into codes / the next input row.
 * B <= 256 (rows are processed in groups of 8).  Execution switch ISI_PRIOR_GRAPH = W (default 8): windows of W consecutive
 * positions that are all sampled / all kept are replayed from hipGraphs captured on a private stream (every
 * position-dependent address read from a device counter): the host leaves the loop.  The executables are kept by the
 * library, keyed on the bytes of *w, *state (the host mask aside), the sampling parameters and the switches -- a later call
 * with equal arguments replays them, nothing is captured again and the call never waits for the stream (at most 8 argument
 * sets are kept; the least recently used one is dropped once its last replay has finished).  While the CALLER is capturing `stream`
 * and with ISI_PRIOR_GRAPH = 0: ~66 direct launches per position.  Same kernels, same codes either way.
 * Single-source cross-attention (state->cross_out != NULL): decoder row p attends source row p / Cd only (the aligned
 * decoder layer, the identity memory mask).  The softmax over one key is 1, so a layer's cross-attention block at row p
 * is row p / Cd of cross_out[l] = out_proj(V(memory)) (biases included); one launch per layer forms
 * LN1(y1) + cross_out[l][p / Cd] in place of the query GEMV, the cached attention and the out-projection, and
 * memory_kv may be NULL (it is not read).  Requires Ce == 1 (else ISI_E_UNSUPPORTED) and (S_t - 1) / Cd < S_src
 * (else ISI_E_INVALID), both checked before any launch.
 * 16-bit caches (state->kv_format = ISI_KV_BF16, opt-in; fp32 is the default and is bit for bit what it was): kv_cache
 * and memory_kv point at bf16 arrays -- half the bytes the cached attention streams per position, half the footprint.  The
 * launch that forms q | k,v rounds k,v to nearest-even as it stores them into the cache slot (NaN stays NaN; bf16 has
 * fp32's range, nothing overflows); the caller fills memory_kv and any prefilled cache rows in the same format.  The
 * cached attention widens the rows exactly and computes in fp32 (isi_rel_attention_decode_kv16_f32); x_seq, cross_out,
 * the scratch rows and every weight stay fp32.  Sampled codes may differ from an fp32-cache run's (keys and values
 * carry 8 significand bits); the format is part of the graph cache key.
 * Shared memory (state->memory_shared = 1, opt-in; 0 takes exactly the launches it took): the B rows are variations of ONE
 * request -- same source sequence, hence one encoder memory.  memory_kv is [n_layers, S_src, 1, 2d] (in kv_format) and
 * cross_out [n_layers, S_src, 1, d]: B times fewer bytes to hold and, per position, to read.  From 48 rows on the
 * cross-attention runs as isi_rel_attention_decode_shared_f32; below, the per-row kernel reads the one copy with batch stride
 * 0 (the launches of a batched memory, every row on the same cache lines); the single-source launch reads its table row
 * with batch stride 0.  kv_cache, x_seq, codes and uniforms keep their batch dimension.  Part of the
 * graph cache key like every field.  isi_prior_sample_run_rows refuses it (ISI_E_UNSUPPORTED).
 * Token log-probabilities (state->token_log_probs != NULL, opt-in; NULL takes exactly the launches it took): the draw of
 * every committed token also stores token_log_probs[b * S + i] = log softmax(logits)[token] of the MODEL's distribution --
 * the row's raw logits, temperature 1, nothing filtered, natural log, fp32 -- so the value does not depend on temperature,
 * top_k or top_p, scores of calls with different sampling settings compare, and they equal what a teacher-forced pass
 * followed by isi_token_log_prob_f32 gives.  Two more block reductions in the draw's workgroup (fixed order: the value
 * does not depend on the launch form); no other launch of a position changes.  Works in every form of the loop: ragged
 * plans (rows that do not commit write nothing), memory_shared, single-source cross-attention, both kv_formats, direct
 * launches and graph replay -- the pointer is part of the graph cache key like every field. */
int isi_prior_sample_run(const isi_prior_w *w, const isi_prior_state *state, int p_begin,
                         int p_end, float temperature, int top_k, float top_p, void *stream);

/* Ragged batches: independent requests decoded together, each row at its OWN position.  Step t of the plan moves row b
 * to decoder position pos[t][b] (the whole stack on that row, its k|v into cache slot pos[t][b]) and, where
 * commit[t][b], draws token pos[t][b] - (start_len - 1) of row b with uniform u[(pos - start_len + 1) * B + b] and writes
 * the code and the token's embedding into input row pos + 1.  Rows advance by 0 or 1 per step; a row that has finished
 * stays at its last position with commit = 0 (it recomputes the same cache slot with the same bits and writes nothing
 * else).  Per-row sampling parameters: temperature / top_k / top_p [B] on the device, or NULL for the call's scalars. */
typedef struct isi_prior_rows {
  const int32_t *pos;          /* [n_steps, B] device: decoder position of row b at step t                 */
  const uint8_t *commit;       /* [n_steps, B] device: 1 = draw and commit row b's token at step t          */
  const int32_t *pos_host;     /* [n_steps, B] HOST copy of pos: validation and planning only               */
  const uint8_t *commit_host;  /* [n_steps, B] HOST copy of commit: validation, and which steps sample       */
  const float *temperature;    /* [B] device or NULL (then the call's scalar); likewise top_k, top_p        */
  const int32_t *top_k;
  const float *top_p;
  int n_steps;
} isi_prior_rows;
/* Steps [t_begin, t_end) of the plan *rows (isi_abi_struct_bytes(13) = sizeof(isi_prior_rows)).  state->mask is not
 * read.  Before any launch the host checks, from the host copies, 0 <= pos < S_t, steps of 0 or 1 per row, and that
 * every commit names a token in [0, S) (else ISI_E_INVALID); B outside 1..256 gives ISI_E_UNSUPPORTED (a single request
 * is better served by isi_prior_sample_run).  The library never reads a device array on the host.  Graph replay as isi_prior_sample_run:
 * W = ISI_PRIOR_GRAPH steps per graph, windows whose steps all sample (some row commits) or all keep; the cache key
 * holds the bytes of *rows except its two host pointers.  Same kernels as isi_prior_sample_run, instantiated with the
 * row's own position in every position-dependent address (x / residual rows, cache slot, key count and relative term of
 * the attention, source row of single-source cross-attention, uniform, commit). */
int isi_prior_sample_run_rows(const isi_prior_w *w, const isi_prior_state *state, const isi_prior_rows *rows,
                              int t_begin, int t_end, float temperature, int top_k, float top_p, void *stream);

/* Code palettes and logit bias in the loop: a table of bias rows and, per token, the index of the row its draw uses.  The
 * struct travels BESIDE isi_prior_state (whose size and offsets are what they were) into the two entries below. */
typedef struct isi_prior_code_bias {
  const float *code_bias;          /* [code_bias_count, n_class] device: logit bias rows; -inf bans a class                */
  const int32_t *code_bias_index;  /* [code_bias_batch, S] device, SEQUENCE order (that of codes): the row of every token, */
                                   /* -1 = none                                                                             */
  int code_bias_count;             /* rows of code_bias                                                                     */
  int code_bias_batch;             /* 1: one index row for all B rows; B: one per row                                       */
} isi_prior_code_bias;
/* isi_prior_sample_run / isi_prior_sample_run_rows with a code bias (isi_abi_struct_bytes(14) = sizeof(isi_prior_code_bias)).
 * bias == NULL or a zeroed struct means off: exactly the launches of the entry without the argument.  On: the draw of
 * token i of row b adds code_bias[r, 0:n_class], r = code_bias_index[(code_bias_batch == 1 ? 0 : b) * S + i], to the logits
 * before temperature and filters (isi_sample_row_bias_f32's arithmetic: (logit + bias) * (1 / temperature)).  r outside
 * [0, code_bias_count) -- -1 by convention -- means no bias for that token and reads nothing from the table.  A -inf bias
 * bans a class (a palette is a row of 0 and -inf); +inf and NaN are outside the contract and every row keeps a finite
 * biased logit -- the caller's checks: the library never reads a device array on the host.  state->token_log_probs stays
 * the MODEL's log-probability: it is unaffected by the bias, as by temperature and filters.  Checked before any launch
 * (ISI_E_INVALID): exactly one of the two pointers set, code_bias_count <= 0 with the pointers set, code_bias_batch not 1
 * or B.  Works in every form of the loop: ragged plans (the index is by token, not by step), memory_shared, single-source
 * cross-attention, both kv_formats, token_log_probs, direct launches and graph replay -- the bytes of *bias are part of the
 * graph cache key beside those of *state, and the arrays' contents are read at replay time, as the uniforms are. */
int isi_prior_sample_run_bias(const isi_prior_w *w, const isi_prior_state *state, const isi_prior_code_bias *bias,
                              int p_begin, int p_end, float temperature, int top_k, float top_p, void *stream);
int isi_prior_sample_run_rows_bias(const isi_prior_w *w, const isi_prior_state *state, const isi_prior_rows *rows,
                                   const isi_prior_code_bias *bias, int t_begin, int t_end, float temperature, int top_k,
                                   float top_p, void *stream);

/* ----------------------------------------------------------- quantization */

/* L2 nearest-neighbour vector quantisation, eval mode
 * (QuantizedBottleneck.forward, bottleneck.py:53-61,75-77,94-101).
 *   z        [N, D]   channels-last pre-quantisation vectors
 *   codes_kd [K, D], e2 [K]  from isi_pack_codebook_f32
 *   idx_out  [N] int64   argmin_k ( (|z|^2 - 2 z.e_k) + |e_k|^2 ), ties -> lowest k
 *   q_out    [N, D]   z + (e_idx - z)      (straight-through value, :95)
 *   counts   [K] int32  histogram of idx (caller zeroes; accumulated)
 *   sse_part [isi_vq_num_partials(N)] fp32 per-workgroup sum (e_idx - z)^2
 * Requirements: D in {8,16,32,64}; with Kp = K rounded up to 32: Kp*(D+4)*4 + Kp*8 <= 150 KiB
 * (the LDS image is padded with rows that can never win).
 * A vector with a non-finite component gets idx -1 and q = NaN, is not counted, and makes its workgroup's partial NaN.
 * A code vector with a non-finite component (its e2 is +inf or NaN) never wins: its distance is not below +inf, and the
 * matrix pipe confines it to its own row, so every other code ranks as if it were absent (what isi_vq_nearest_topm_f32
 * documents for the same stage); a codebook of such codes alone answers every vector with -1.
 * Refused on the host before any launch: a null pointer, N <= 0, K <= 0, z, codes_kd or q_out not 16-byte aligned
 * (ISI_E_INVALID); another D, or a codebook beyond the LDS bound above (ISI_E_UNSUPPORTED). */
int isi_vq_nearest_f32(const float *z, const float *codes_kd, const float *e2,
                       int64_t *idx_out, float *q_out, int32_t *counts,
                       float *sse_part, int64_t N, int D, int K, void *stream);
/* Same, with a flag word: ISI_CONV_F16X3 computes z.e_k with split-f16 products (three f16 MFMA terms, per-product
 * error ~2^-23; |z| < 16384, |e| < 64) when D == 64 and the codebook's two f16 planes fit in LDS -- with Kp = K rounded
 * up to 32: Kp*264 + Kp/8 + 48 bytes <= 150 KiB, that is K <= 576 --, five times fewer matrix-pipe cycles than the
 * exact-fp32 products that bound isi_vq_nearest_f32.  0 = exact; so is the flag at another D or a larger K, which the
 * exact kernel's own bound then refuses (K > 544 at D = 64).
 * On the split-f16 route a vector with a non-finite component or one beyond the range (|z| >= 16384) gets idx -1,
 * q = NaN, and makes the squared error NaN; so does every vector when a code vector is not finite.  FINITE code vectors beyond the range (|e| >= 64: the unused codes of a
 * trained codebook) are exact: they are kept out of the f16 search and the fp32 decision proves per vector that none of
 * them can win ((min |e_far| - |z|)^2 > winner's distance) or compares the winner with each of them in fp32. */
int isi_vq_nearest_flags_f32(const float *z, const float *codes_kd, const float *e2,
                             int64_t *idx_out, float *q_out, int32_t *counts,
                             float *sse_part, int64_t N, int D, int K, int flags, void *stream);
int isi_vq_num_partials(int64_t N);

/* quantize_conv (1x1, vqvae.py:260,272: Conv2d(C0 [+ C1] -> D, 1) on cat(src0, src1)) FUSED with the search above
 * (SURVEY K4 + K5): z = W a + bias is produced in registers and consumed by the distance products, it never goes to
 * memory.  Pair pipeline only: sources in the pair format (ISI_CONV_*_PAIR, channels-last, 32-channel multiples),
 * `packed_w16` = the packed 1x1 weight's blocked pair copy (ISI_CONV_W16: packed weight + D * Kpad floats), D = 64.
 * Pixel n = (b H + y) W + x reads src0 / src1 through their strides.  Outputs as isi_vq_nearest_f32 (bit-identical
 * to isi_conv2d_f32(ISI_CONV_F16X3 | ISI_CONV_W16) followed by it from C0 + C1 = 128 on, where that convolution runs the
 * split products; below it runs exact-fp32 products and its z is another rounding of the same sum -- idx and counts
 * still agree away from near-ties); `q_pair_out` (nullable): pair-format copy of q.
 * `workspace`: isi_vq_conv1x1_workspace_floats(C0, C1, D) floats, 16-byte aligned (a fragment-major copy of the
 * weight is written there by a small pre-kernel). */
int isi_vq_conv1x1_nearest_f32(const isi_src *src0, const isi_src *src1, const float *packed_w16, const float *bias,
                               const float *codes_kd, const float *e2, int64_t *idx_out, float *q_out,
                               float *q_pair_out, int32_t *counts, float *sse_part, float *workspace, int B, int H,
                               int W, int D, int K, void *stream);
/* The same launch for the TRAINING step (train_vqvae.py:168-192 -> bottleneck.py:53-101): `z_out` ([N][64] fp32,
 * nullable) also receives z -- the commitment gradient 2 (z - q) / numel and the EMA sums of bottleneck.py:75-92 read it --
 * and `counts` is zeroed by the launch's pre-kernel (isi_vq_conv1x1_nearest_f32 expects zeroed counts). */
int isi_vq_conv1x1_nearest_tape_f32(const isi_src *src0, const isi_src *src1, const float *packed_w16, const float *bias,
                                    const float *codes_kd, const float *e2, int64_t *idx_out, float *q_out,
                                    float *q_pair_out, float *z_out, int32_t *counts, float *sse_part, float *workspace,
                                    int B, int H, int W, int D, int K, void *stream);
size_t isi_vq_conv1x1_workspace_floats(int C0, int C1, int D);
/* Pack-time half of the fused launch: the fragment-major copy ([D][Kpad] floats) of a packed 1x1 weight's pair copy.  A
 * weight laid out {packed [D][Kpad] | pair copy | fragments} with isi_vqvae_w.w16 = 2 lets isi_vqvae_run skip the pre-kernel in
 * front of each search (its two histograms are then zeroed by one launch). */
int isi_vq_pack_fragments_f32(const float *packed_w16, float *frag_out, int Kpad, void *stream);
/* The LDS content the fused search works on -- both f16 planes of the codebook, |e|^2 adjusted for far and non-finite
 * codes, the far-code words -- as ONE image of isi_vq_planes_bytes(K) bytes (16-byte aligned), made once per codebook
 * instead of by every workgroup of every launch (isi_codebook_w.planes).  D = 64. */
size_t isi_vq_planes_bytes(int K);
int isi_vq_pack_planes_f32(const float *codes_kd, const float *e2, void *planes_out, int D, int K, void *stream);
/* Code tables: the two layers of the forward that read nothing but the quantised TOP map -- dec_t's first 3x3 convolution
 * (encoder_decoder.py:138 through vqvae.py:265) and upsample_top_to_bottom[0] (ConvTranspose2d k4 s2 p1, vqvae.py:193-201,281)
 * -- are linear in it, and each of its pixels is one of the K codebook rows: the per-pixel products W[tap] . E[id] are
 * made once per version of the codebook and of the weight, and the layers become sums of gathered rows.
 *   which = 0: T3 [tap = kh*3 + kw][K][Cout3],   T3[t][k][n]     = sum_c W3[n][t*D + c]      E[k][c]
 *   which = 1: TU [phase = py*2 + px][tap = ty*2 + tx][K][CoutU], TU[ph][t][k][n] = sum_c Wph[ph][n][t*D + c] E[k][c]
 * w3_packed / wT_packed: the fp32 sections of isi_pack_conv_weight_f32 ([Cout3][D][3][3]) / isi_pack_convT_k4s2_weight_f32
 * ([D][CoutU][4][4], phase-matrix layout); codes_kd [K][D].  Every entry is accumulated in double and rounded to fp32
 * once.  Behind its last block a table carries one pad row of Cout floats of -0.0, which a tap outside the map gathers
 * (adding -0.0 changes no bit).  isi_vq_code_tables_bytes: size of one table with its pad row (0 for a bad argument); the
 * gather needs (16 K + 1) Cout < 2^30.  isi_vq_pack_code_tables_f32: one launch per
 * table given (either output may be NULL), no allocation, no synchronisation; tables 16-byte aligned, Cout multiples of 4.
 * isi_vq_code_gather_f32: ONE launch that writes, from ids [B, H, W] (int64, low word read),
 *   out3[b,y,x,:]        = [relu3]( bias3 + sum_{taps inside the map} T3[tap][ids[b, y+kh-1, x+kw-1]] )       [B, H, W, C3]
 *   outU[b,2y+py,2x+px,:] = [reluU]( biasU + sum_{taps inside the map} TU[ph][t][ids[b, y-1+py+ty, x-1+px+tx]] ) [B, 2H, 2W, CU]
 * dense channels-last, fp32 or (out*_pair != 0, C % 8 == 0) in the pair format of ISI_CONV_OUT_PAIR.  Either half may be
 * left out (NULL table).  Taps are added in ascending tap order after the bias and a tap outside the map adds nothing: an
 * output pixel's bits depend on its window's codes alone.  A code outside [0, K) -- the search's -1 -- is never used as
 * an address: every output pixel whose window contains it is written as NaN.  The ReLU propagates NaN. */
size_t isi_vq_code_tables_bytes(int which, int K, int Cout);
int isi_vq_pack_code_tables_f32(const float *w3_packed, int Cout3, const float *wT_packed, int CoutU, const float *codes_kd, int D,
                                int K, float *t3_out, float *tu_out, void *stream);
int isi_vq_code_gather_f32(const int64_t *ids, const float *t3, const float *bias3, float *out3, int C3, int out3_pair, int relu3,
                           const float *tu, const float *biasU, float *outU, int CU, int outU_pair, int reluU, int B, int H, int W,
                           int K, void *stream);
/* 1 when the fused launch covers the shape (D = 64, 32-channel multiples, C0 + C1 <= 256, both code planes in LDS) */
int isi_vq_conv1x1_fusable(int C0, int C1, int D, int K);

/* diff = sum(sse_part)/(N*D); perplexity = exp(-sum p log(max(p,1e-7))),
 * p = counts/N  (bottleneck.py:94,97-100).  Writes out2[0]=diff, out2[1]=perplexity. */
int isi_vq_finalize_f32(const float *sse_part, int n_part, const int32_t *counts,
                        int K, int64_t N, int D, float *out2, void *stream);

/* embed_code: out[N, D] = codes_kd[idx[n], :]  (bottleneck.py:103-104).
 * Index range is not reported from the device: callers validate 0 <= idx < K
 * (out-of-range values are clamped so that no read leaves the codebook).  D % 4 == 0; codes_kd and out
 * 16-byte aligned (rows are copied as float4; a misaligned pointer is refused with ISI_E_INVALID). */
int isi_embed_code_f32(const int64_t *idx, const float *codes_kd, float *out,
                       int64_t N, int D, int K, void *stream);

/* embed_mix: per-cell weighted mixtures of codebook rows, the step in front of VQVAE.decode that renders "70 % of this
 * sound, 30 % of that one".  For N cells, M sources (1 <= M <= 8), codes_kd [K][D], ids [M][N] int64 and weights [M][N]
 * fp32 (source m starts ids_stride / w_stride ELEMENTS behind source m - 1), out [N][D] with ldo FLOATS between two cells:
 *   out[n, :] = sum over m ascending, of the terms with w[m, n] != 0, of  w[m, n] * codes_kd[id[m, n], :]
 * A term whose weight compares equal to zero (+0.0 or -0.0) does not exist: its id is never looked at (it may be -1, K,
 * the priors' mask token, 2^40) and its codebook row may hold NaN.  A term with a non-zero weight (NaN included) and an id
 * outside [0, K) makes all D channels of that cell NaN, and only that cell's; such an id is never used as an address (the
 * rule of isi_vq_code_gather_f32).  One lane's arithmetic is acc = -0.0f, then acc = fmaf(w, e, acc) for each existing
 * term, m ascending.  Hence: a cell whose only existing term has weight 1 equals the codebook row bit for bit, -0.0 entries
 * included; a cell with no existing term is -0.0; the bits of a cell depend on that cell's ids and weights alone, not on
 * N, the batch or the launch geometry.  Against the float64 sum the error is at most T 2^-24 sum_m |w_m e_m| (1 + 2^-20),
 * T the number of existing terms: one rounding per fma, each bounded by 2^-24 of a partial sum the absolute sum dominates.
 * Refused on the host before any launch (ISI_E_INVALID): a null pointer; N <= 0; M outside 1..8; D <= 0 or not a multiple
 * of 4; K <= 0; codes_kd or out not 16-byte aligned, or ldo not a multiple of 4; ldo < D; ids_stride < N or w_stride < N.
 * Index range (ISI_E_UNSUPPORTED at or beyond it): N D / 4 < 2^31 (the launch's lanes are numbered in 32 bits),
 * ids_stride and w_stride < 2^56, ldo < 2^31 (addresses are formed in 64 bits from these).  One launch, no workspace. */
int isi_embed_mix_f32(const int64_t *ids, int64_t ids_stride, const float *weights, int64_t w_stride,
                      const float *codes_kd, float *out, int64_t ldo, int64_t N, int M, int D, int K, void *stream);

/* vq_nearest_topm: the M nearest codes of each vector (1 <= M <= 8), in order, among the codes its palette allows, with
 * their distances -- "render this sound with that sound's codes", a sound as per-cell mixtures, the codebook's own
 * alternatives for a cell.  z [N][D], codes_kd [K][D], e2 [K] as for isi_vq_nearest_f32 (isi_pack_codebook_f32).
 * Palettes: allowed is [P][ceil(K / 32)] 32-bit words, bit k & 31 of word k >> 5 in row p says that code k is in palette
 * p; allowed_row [N] names each vector's row (NULL: row 0 for every vector).  allowed == NULL: every code is allowed, and
 * then P must be 0 and allowed_row NULL.  (The prior's code_bias / code_bias_map shape: a small table and a per-cell map.)
 * Outputs, in the [M][N] layout with a stride in ELEMENTS that isi_embed_mix_f32 reads: ids_out[m * ids_stride + n] is the
 * code of rank m of vector n, dist_out[m * dist_stride + n] its distance.  Nothing else of the two buffers is written.
 *   d[n,k] = (|z_n|^2 - 2 z_n.e_k) + e2[k]   in fp32, with the products, their order and the |z|^2 sum of
 *            isi_vq_nearest_f32's exact kernel (fp32 matrix pipe: no operand range beyond fp32's own)
 *   rank m = the m-th smallest (d, k) pair in lexicographic order over the allowed codes k < K with d < +inf
 * Ties -- duplicate code vectors included -- go to the lower code first.  Hence: without a palette rank 0 equals
 * isi_vq_nearest_f32's idx_out, index for index, on any data; and a vector's results depend on that vector, its palette
 * row and the codebook alone, not on N, the batch or the launch geometry.
 * A palette with fewer than M such codes fills the missing ranks with id -1 and distance +inf (an empty row: all of them).
 * An allowed_row value outside [0, P) is never used as an address: that vector is answered like an empty palette.
 * A vector with a non-finite component (its fp32 |z|^2 is not finite) gets id -1 and distance NaN at every rank.
 * A non-finite code vector is never returned: e2 already carries it (+inf or NaN), so its distance is not < +inf, and the
 * matrix pipe confines it to its own row -- other codes' ranks are what they would be without it.  (A finite code whose
 * |e|^2 overflows fp32 counts as non-finite.)  Padding codes of the last 32-code tile and palette bits at positions >= K
 * are ignored.
 * Refused on the host before any launch (ISI_E_INVALID): a null z, codes_kd, e2, ids_out or dist_out; N <= 0; M outside
 * 1..8; D not 8, 16, 32 or 64; K <= 0; ids_stride < N or dist_stride < N; allowed_row without allowed; P != 0 without
 * allowed; P <= 0 with allowed; z or codes_kd not 16-byte aligned.  ISI_E_UNSUPPORTED: P > 64 (the palette rows live in
 * LDS); a codebook beyond isi_vq_nearest_f32's LDS budget, (Kp (D + 4) + 2 Kp + 8) floats with Kp = K rounded up to 32,
 * plus P Kp / 32 words, above 150 KiB; N >= 2^40 or a stride >= 2^56.  One launch, no workspace. */
int isi_vq_nearest_topm_f32(const float *z, const float *codes_kd, const float *e2, const uint32_t *allowed, int P,
                            const int32_t *allowed_row, int64_t *ids_out, int64_t ids_stride, float *dist_out,
                            int64_t dist_stride, int64_t N, int D, int K, int M, void *stream);

/* ------------------------------------------------- whole VQ-VAE-2 forward */

#define ISI_MAX_STAGES 4
#define ISI_MAX_RES 8

typedef struct isi_conv_w {
  const float *w;    /* packed weight */
  const float *bias; /* [Cout]        */
  int Cin, Cout;
} isi_conv_w;

typedef struct isi_encoder_w { /* RosinalityEncoder, encoder_decoder.py:38-126 */
  int n_down;                          /* number of k4 s2 convs              */
  isi_conv_w down[ISI_MAX_STAGES];
  isi_conv_w conv3;                    /* k3 conv after the strided stack    */
  int n_res;
  isi_conv_w res3[ISI_MAX_RES];        /* ResBlock conv.1 (k3, C -> R)       */
  isi_conv_w res1[ISI_MAX_RES];        /* ResBlock conv.3 (k1, R -> C)       */
} isi_encoder_w;

typedef struct isi_decoder_w { /* RosinalityDecoder, encoder_decoder.py:129-227 */
  isi_conv_w conv3;
  int n_res;
  isi_conv_w res3[ISI_MAX_RES];
  isi_conv_w res1[ISI_MAX_RES];
  int n_up;
  isi_conv_w up[ISI_MAX_STAGES];       /* packed transposed convs            */
} isi_decoder_w;

typedef struct isi_codebook_w {
  const float *codes_kd; /* [K][D] */
  const float *e2;       /* [K]    */
  int D, K;
  const void *planes;    /* optional (NULL: derived per launch): isi_vq_pack_planes_f32 of codes_kd / e2, read by the
                          * fused searches of isi_vqvae_run; must be re-made whenever the codebook changes */
} isi_codebook_w;

typedef struct isi_vqvae_w { /* VQVAE.__init__, vqvae.py:126-216 */
  int in_channel;
  isi_encoder_w enc_b, enc_t;
  isi_conv_w quantize_conv_t, quantize_conv_b;
  isi_codebook_w quantize_t, quantize_b;
  isi_decoder_w dec_t, dec;
  int n_upsample;
  isi_conv_w upsample[ISI_MAX_STAGES];
  int w16;       /* 1: every packed convolution weight above is followed by its isi_split_conv_weight_f16 copy
                  * (used when precision == 4); 2: ... and quantize_conv_t / _b by a third section, the fragment-major
                  * copy of isi_vq_pack_fragments_f32                                                  */
  int precision; /* products of the convolutions (data and accumulation are always fp32):
                  * 0: fp32 matrix pipe everywhere.  1: ISI_CONV_BF16X3 in `dec` and `upsample` only
                  * (no code index depends on them).  2: ISI_CONV_BF16X3 in every convolution (near-tie
                  * indices move).  3: ISI_CONV_BF16X6 (fp32-grade six-term split) in every layer that
                  * feeds a code index, ISI_CONV_BF16X3 in `dec` and `upsample`.  4: ISI_CONV_F16X3
                  * (fp32-grade three-term split-f16 products, f16 operand range) in every convolution. */
  int no_quantize; /* 1: UnquantizedBottleneck (bottleneck.py:107-119, selected at vqvae.py:152-160): the two
                    * codebook searches are skipped, quant_t / quant_b receive the 1x1 convolutions' outputs,
                    * id_t / id_b are not written, scalars = {0, inf, 0, inf}; the codebooks may be null */
  const float *code_table_conv3;    /* optional (NULL: the layer runs as a convolution): isi_vq_pack_code_tables_f32's table of
                                     * dec_t.conv3 over quantize_t's codebook; must be re-made whenever either changes */
  const float *code_table_upsample; /* the same for upsample[0]; used by calls that both encode and decode */
} isi_vqvae_w;

/* Outputs of VQVAE.encode / forward (vqvae.py:245-278).  Any pointer may be
 * NULL except the ones the requested mode needs. */
typedef struct isi_vqvae_out {
  float *dec;        /* [B, in_channel, H, W]  NCHW      (forward/decode)   */
  float *quant_t;    /* [B, Ht, Wt, D]  channels-last    (encode/forward; null in a FORWARD call: the map stays in the
                      * pair format the decoders read and no fp32 copy is written -- the fused search's stores bound it) */
  float *quant_b;    /* [B, Hb, Wb, D]  channels-last                        */
  int64_t *id_t;     /* [B, Ht, Wt]                                          */
  int64_t *id_b;     /* [B, Hb, Wb]                                          */
  float *scalars;    /* [5]: diff_t, perplexity_t, diff_b, perplexity_b, diff_t + diff_b (what VQVAE.forward returns as
                      * `diff`, vqvae.py:263,275,277)                                                        */
} isi_vqvae_out;

#define ISI_MODE_ENCODE 1  /* VQVAE.encode        vqvae.py:251-278 */
#define ISI_MODE_DECODE 2  /* VQVAE.decode        vqvae.py:280-286 (quant_t/b are inputs) */
#define ISI_MODE_FORWARD 3 /* VQVAE.forward       vqvae.py:245-249 */

/* Bytes of scratch `isi_vqvae_run` needs for this shape. */
/* 1 if isi_vqvae_run keeps this model's internal activations in the split-f16 pair format (precision 4, w16, every
 * layer that would read a pair tensor able to: see ISI_CONV_*_PAIR), 0 if it runs on fp32 activations. */
int isi_vqvae_pair_activations(const isi_vqvae_w *w);
size_t isi_vqvae_workspace_bytes(const isi_vqvae_w *w, int B, int H, int W);

/* x: [B, in_channel, H, W] NCHW contiguous fp32 (ignored in DECODE mode).
 * H and W must be divisible by the total down-sampling factor. */
int isi_vqvae_run(const isi_vqvae_w *w, int mode, const float *x, int B, int H,
                  int W, const isi_vqvae_out *out, void *workspace,
                  size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISI_HIP_H */
