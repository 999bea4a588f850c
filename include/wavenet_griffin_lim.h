/* wavenet_griffin_lim.h -- the Griffin-Lim baseline's part of the C ABI of
 * libwavenet_hip.so (gfx950 / MI355X): csrc/wn_griffin_lim.hip, bound by
 * wavenet/_lib.py's GRIFFIN_LIM_SIGNATURES, driven by wavenet/griffin_lim.py.
 * The contract of wavenet_hip.h holds for every entry (plain C, caller-owned
 * buffers, asynchronous on `stream`, WN_OK or a negative WN_ERR_* code, all
 * checks before any launch, no atomics, one summation order).  A clip's output
 * is a function of its own data, its length and the tables: not of B, the
 * clip's position or its neighbours.  wavenet/griffin_lim.py: GriffinLim.
 * reference states the whole rule in numpy float32, tests/gl_ref.py restates it
 * in float64.
 *
 * The frame grid is wn_melspec's: F = ceil(T / hop); clip b has n[b] =
 * lengths ? min(max(lengths[b], 0), T) : T samples and Fb = ceil(n[b] / hop)
 * real frames; frame f is centred at c_f = f * hop + hop / 2 and is
 *   frame[j] = x[c_f - n_fft / 2 + j] * window[j]    x = 0 outside [0, n[b])
 * `window` (device float [n_fft]) and `basis` (device float
 * [ceil(n_bins / 32)][n_fft][cos 32 | sin 32]) are wn_melspec's tables; n_fft
 * is a multiple of 64 in [64, 2048], 1 <= hop <= n_fft, n_bins = n_fft / 2 + 1,
 * 1 <= B <= 65535, 1 <= T <= 2^30.  Every line below is ONE float32 operation
 * per operator, no fused multiply-add, unless it says MFMA.
 *
 * ---- wn_stft: audio -> complex spectrogram, out [B][F][n_bins][re, im].
 * Per real frame f < Fb and bin k:
 *   w[j]  = x[c_f - n_fft / 2 + j] * window[j]
 *   re[k] = sum_j cos[j][k] * w[j]      im[k] = sum_j sin[j][k] * w[j]
 * each sum one fp32 MFMA (v_mfma_f32_32x32x2_f32) accumulator from zero, j
 * ascending in pairs, and out stores (re[k], -im[k]): the e^{-i} DFT that
 * torch.stft computes and torch.view_as_complex reads.  The stored im of bin 0 and of
 * the Nyquist bin is an exact +0; the Nyquist bin's cos row is (-1)^j, not the
 * table's.  Frames f >= Fb are exact zeros.  Nothing at or behind n[b] is
 * read.  The samples are read from memory where they are used: there is no
 * LDS staging of the tile's samples and so no edge to stand either side of.
 *
 * ---- wn_istft: complex spectrogram -> audio, the least-squares inverse.
 * Per real frame f < Fb and sample j of it, with the stored (re, im):
 *   C    = sum_{k=0}^{n_fft/2-1} cos[j][k] * a[k]   a[0] = 0.5 * re[0], else re[k]
 *   S    = sum_{k=0}^{n_fft/2-1} s[j][k]  * b[k]    b[0] = 0.5 * re[n_fft / 2],
 *                                                   s[j][0] = (-1)^j; else
 *                                                   b[k] = -im[k], s = sin
 *          (two MFMA accumulators from zero, k ascending in pairs)
 *   y    = (C + S) * scale                          scale = float32(2 / n_fft)
 *   v[j] = y * window[j]
 * that is y_f[j] = (1 / n_fft) (re[0] + (-1)^j re[n_fft/2] + 2 sum_{k=1}^
 * {n_fft/2-1} (re[k] cos(2 pi j k / n_fft) - im[k] sin(2 pi j k / n_fft))).  The
 * imaginary parts of bins 0 and Nyquist are not read.  v goes to `scratch`
 * [B][F][n_fft] (frames f >= Fb are neither read nor written).  Then, with
 * j_f(t) = t - (c_f - n_fft / 2), for t < n[b]:
 *   num  = sum_f v_f[j_f(t)]                        from zero, f ascending over
 *   den  = sum_f window[j_f(t)] * window[j_f(t)]    the real frames covering t
 *   x[t] = den > 1e-8f ? num / den : 0
 * and x[t] = +0 for n[b] <= t < T.  What a frame holds outside [0, n[b]) is
 * dropped.  Two launches: the frames, then the gather.
 *
 * ---- wn_mel_to_magnitude: raw log-mel frames [B][F][n_mels] (natural log of
 * power) -> magnitudes [B][F][n_bins].  Fb = nframes ? min(max(nframes[b], 0),
 * F) : F.  Per real frame:
 *   M[m] = expf(in[m])
 *   P[k] = sum_m pinv[k][m] * M[m]      from zero, m ascending, every product
 *                                       rounded before it is added
 *   A[k] = sqrtf(P[k] < 0 ? 0 : P[k])   (a NaN passes)
 * Frames f >= Fb are exact zeros and are not read.
 *
 * ---- wn_gl_init: the starting spectrum c0 [B][F][n_bins][2] from A.
 *   p  = mode == 0 && 0 < k < n_fft / 2
 *        ? draw_bits(seed ^ 0x6772696666696E4C, (keys[b] << 40) | (f * n_bins + k)) & 1023
 *        : 0                            (draw_bits: csrc/wn_common.h, 64-bit)
 *   c0 = (A * tab[p][0], A * tab[p][1]) tab: device float [1024][2], (cos, sin)
 *                                       of 2 pi p / 1024, rounded from float64
 * mode 1 is all phases zero.  One float32 multiply per component.
 *
 * ---- wn_gl_project: one iteration's analysis half.  (re, im) as wn_stft
 * stores them, the same bits; then per frame f < F and bin k:
 *   m2 = re * re + im * im
 *   m2 > 1e-30f:  r = A / sqrtf(m2),  t = (re * r, im * r)
 *   else:         t = (A, 0)
 *   c  = t + alpha * (t - t_prev)       per component: d = t - t_prev, e =
 *                                       alpha * d, c = t + e
 * Frames f >= Fb: t = c = exact zeros, A and t_prev not read.  t_out may be
 * t_prev (every element is read before it is written, by the same lane).
 * With trace != NULL also, in float64, the float32 values widened first:
 *   g = sqrtf(m2) - A                   (float32)
 *   trace[b][0] = sum g * g      trace[b][1] = sum A * A
 * over the real frames and the n_bins bins.  The summation order: tile q of
 * clip b holds the frames 32 q .. 32 q + 31; lane (i, h), i = frame - 32 q, of
 * wave w adds, from zero, its terms of the bin chunks c = w, w + 8, ... <
 * n_fft / 64 ascending and inside a chunk the bins 32 c + 8 u + 4 h + e, u = 0
 * .. 3 outer, e = 0 .. 3 inner, the Nyquist bin right behind bin 0; the 64
 * lanes by the xor butterfly (32, 16, 8, 4, 2, 1), the eight waves in the
 * order 0 .. 7 from zero, one pair per tile to `partials`; a second launch adds
 * a clip's tiles in ascending order from zero.
 */
#ifndef WAVENET_GRIFFIN_LIM_H_
#define WAVENET_GRIFFIN_LIM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* x: device float, clip b at + b * ld_x, T samples; lengths: device int32 [B]
 * or NULL; out: device float [B][F][n_bins][2].  A NULL pointer but lengths:
 * WN_ERR_NULL.  A shape outside the limits above, ld_x < T: WN_ERR_BAD_SHAPE.
 * basis 16-byte, out 8-byte, everything else 4-byte aligned, else
 * WN_ERR_MISALIGNED.  One launch. */
int wn_stft(const float* x, long ld_x, int B, int T, const int32_t* lengths,
            const float* window, const float* basis, int n_fft, int hop,
            int n_bins, float* out, void* stream);

/* Host only, no device: the bytes of wn_istft's `scratch`, B * F * n_fft
 * floats.  -1 for arguments wn_istft refuses. */
long wn_istft_scratch_bytes(int B, int T, int n_fft, int hop);

/* spec: device float [B][F][n_bins][2]; scratch: device float,
 * wn_istft_scratch_bytes(B, T, n_fft, hop) bytes; x: device float, clip b at
 * + b * ld_x, T samples written.  Checks as wn_stft (spec 8-byte aligned). */
int wn_istft(const float* spec, int B, int T, const int32_t* lengths,
             const float* window, const float* basis, int n_fft, int hop,
             int n_bins, float* scratch, float* x, long ld_x, void* stream);

/* frames: device float [B][F][n_mels]; nframes: device int32 [B] or NULL;
 * pinv: device float [n_bins][n_mels]; out: device float [B][F][n_bins].
 * n_mels outside [1, 128], n_bins outside [1, 1025], B outside [1, 65535],
 * F < 1, B * F > 2^31 - 1: WN_ERR_BAD_SHAPE. */
int wn_mel_to_magnitude(const float* frames, int B, int F, int n_mels,
                        const int32_t* nframes, const float* pinv, int n_bins,
                        float* out, void* stream);

/* A: device float [B][F][n_bins]; keys: device int64 [B], each in [0, 2^24);
 * tab: device float [1024][2]; c0: device float [B][F][n_bins][2].  mode 0:
 * random phases, 1: zero phases, anything else WN_ERR_UNSUPPORTED.  n_bins
 * must be n_fft / 2 + 1 of an n_fft within the limits: it names the Nyquist
 * bin.  B outside [1, 65535], F < 1, B * F > 2^31 - 1, F * n_bins >= 2^40 (the
 * counter's low 40 bits hold f * n_bins + k, the key lies above them):
 * WN_ERR_BAD_SHAPE. */
int wn_gl_init(const float* A, int B, int F, int n_bins, const int64_t* keys,
               uint64_t seed, int mode, const float* tab, float* c0,
               void* stream);

/* Host only, no device: the doubles of wn_gl_project's `partials` (two per
 * tile of 32 frames per clip).  -1 for B outside [1, 65535], T outside
 * [1, 2^30] or hop < 1. */
long wn_gl_project_partials(int B, int T, int hop);

/* x, lengths, window, basis as wn_stft; A: device float [B][F][n_bins];
 * t_prev, t_out, c_out: device float [B][F][n_bins][2], 8-byte aligned (t_out
 * may be t_prev; c_out may be neither); alpha in [0, 1); trace: device double
 * [B][2] or NULL; partials: device double [wn_gl_project_partials(B, T, hop)],
 * required exactly when trace is given (one without the other: WN_ERR_NULL).
 * alpha outside [0, 1), c_out == t_out, c_out == t_prev, or A the same
 * pointer as t_prev, t_out or c_out: WN_ERR_BAD_SHAPE (t_out == t_prev is the
 * only aliasing there may be; operands that overlap in part are the caller's
 * to avoid).  One launch, two with a trace. */
int wn_gl_project(const float* x, long ld_x, int B, int T, const int32_t* lengths,
                  const float* window, const float* basis, int n_fft, int hop,
                  int n_bins, const float* A, const float* t_prev, float alpha,
                  float* t_out, float* c_out, double* trace, double* partials,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* WAVENET_GRIFFIN_LIM_H_ */
