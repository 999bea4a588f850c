/* wavenet_lpc.h -- linear prediction's part of the C ABI of libwavenet_hip.so
 * (gfx950 / MI355X): csrc/wn_lpc.hip, bound by wavenet/_lib.py's
 * LPC_SIGNATURES, driven by wavenet/lpc.py.  The contract of wavenet_hip.h
 * holds for every entry (plain C, caller-owned buffers, asynchronous on
 * `stream`, WN_OK or a negative WN_ERR_* code, all checks before any launch, no
 * atomics, one summation order).  A clip's output is a function of its own
 * data, its length and the tables: not of B, the clip's position or its
 * neighbours.  wavenet/lpc.py: LinearPrediction.reference_* state the rules in
 * numpy, tests/lpc_ref.py restates them independently in float64.
 *
 * The frame grid is wn_melspec's: frame f(u) = u / hop (integer division) is
 * the frame of sample u.  1 <= order <= 32, 1 <= hop <= 4096, 1 <= B <= 65535,
 * 1 <= T <= 2^30.  Every line below is ONE rounded operation per operator, no
 * fused multiply-add.
 *
 * ---- wn_lpc_from_mel: raw log-mel frames [B][F][n_mels] (natural log of
 * power) -> predictor coefficients [B][F][order].  Fb = nframes ?
 * min(max(nframes[b], 0), F) : F.  Per real frame, float32:
 *   M[m] = expf(in[m])
 *   P[k] = sum_m pinv[k][m] * M[m]      from zero, m ascending, every product
 *                                       rounded before it is added
 *   P[k] = P[k] < 0 ? 0 : P[k]          (a NaN passes)
 * that is wn_mel_to_magnitude's arithmetic in front of its square root (the
 * table arrives transposed, pinv_t[m][k] = pinv[k][m]).  Then
 * in float64, for i = 0 .. order:
 *   p_q[i] = sum_k ctab[k][i] * (double)P[k]  from zero over k = q, q + 8, q +
 *                                             16, ... < n_bins ascending, every
 *                                             product rounded before it is
 *                                             added; q = 0 .. 7
 *   r[i] = ((p_0[i] + p_1[i]) + ... ) + p_7[i]
 *   r[i] = r[i] * lagwin[i]
 * ctab (device double [n_bins][order + 1]) holds w_k cos(2 pi i k / n_fft) /
 * n_fft, w_k = 1 at bin 0 and at the Nyquist bin and 2 elsewhere: the inverse
 * DFT of the power spectrum at lag i.  lagwin (device double [order + 1]) holds
 * exp(-(2 pi lag_window i / sample_rate)^2 / 2), lagwin[0] = 1 + noise.  Both
 * come from the host.
 *   !(r[0] > 1e-30): out = exact zeros (the identity filter; a NaN frame and a
 *   frame of -inf mels land here)
 * else Levinson-Durbin in float64, a[0] = 1, err = r[0], for i = 1 .. order:
 *   acc = r[i]
 *   acc = acc + a[j] * r[i - j]         j = 1 .. i - 1 ascending
 *   k   = -acc / err
 *   !(|k| < 1): stop; a[i .. order] stay zero, the lower ones stand
 *   t[j] = a[j] + k * a[i - j]          j = 1 .. i - 1 (from the old a)
 *   a[j] = t[j];  a[i] = k
 *   err = err * (1 - k * k)
 * and out[i - 1] = (float)(-a[i]): x[t] ~ sum_i out[i - 1] x[t - i].  Frames f
 * >= Fb are exact zeros and are not read.  Every output is finite.
 *
 * ---- wn_lpc_analysis: x -> excitation e, parallel.  n[b] = lengths ?
 * min(max(lengths[b], 0), T) : T.  For t < n[b], float32:
 *   acc = +0
 *   acc = acc + coeffs[b][f(t - i)][i - 1] * x[t - i]    i = order down to 1,
 *                                                        only where t - i >= 0
 *   e[t] = (x[t] - acc) * gain
 * and e[t] = +0 for n[b] <= t < T; nothing at or behind n[b] is read.  A
 * workgroup serves wn_lpc_analysis_tile() samples of one clip.
 *
 * ---- wn_lpc_synthesis: e -> y, the serial inverse.  For t < n[b]:
 *   y[t] = e[t] * inv_gain + acc        acc as above over y in place of x
 * computed in the transposed direct form, which is the same chain of
 * operations: s_i <- s_{i+1} + coeffs[b][f(t)][i - 1] * y[t] for i = 1 ..
 * order with s_{order+1} = +0 and all s = +0 in front of the clip, and
 * y[t + 1] = e[t + 1] * inv_gain + s_1.  y[t] = +0 for n[b] <= t < T.  One wave
 * per clip, tap i on lane i - 1.
 */
#ifndef WAVENET_LPC_H_
#define WAVENET_LPC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* frames: device float [B][F][n_mels]; nframes: device int32 [B] or NULL;
 * pinv_t: device float [n_mels][n_bins]; ctab: device double [n_bins][order + 1];
 * lagwin: device double [order + 1]; out: device float [B][F][order].  A NULL
 * pointer but nframes: WN_ERR_NULL.  n_mels outside [1, 128], n_bins outside
 * [2, 1025], order outside [1, 32] or above n_bins - 1, B outside [1, 65535],
 * F < 1, B * F > 2^31 - 1: WN_ERR_BAD_SHAPE.  ctab and lagwin 8-byte,
 * everything else 4-byte aligned, else WN_ERR_MISALIGNED.  One launch. */
int wn_lpc_from_mel(const float* frames, int B, int F, int n_mels,
                    const int32_t* nframes, const float* pinv_t, int n_bins,
                    const double* ctab, const double* lagwin, int order,
                    float* out, void* stream);

/* Host only, no device: the samples one workgroup of wn_lpc_analysis serves. */
int wn_lpc_analysis_tile(void);

/* x: device float, clip b at + b * ld_x, T samples; coeffs: device float
 * [B][F][order]; lengths: device int32 [B] or NULL; out: device float, clip b
 * at + b * ld_out, T samples written.  out must not be, or overlap, x.  The
 * frames a clip needs are those below ceil(n[b] / hop): F * hop < T without
 * lengths is WN_ERR_BAD_SHAPE, with lengths a frame index is held below F (the
 * caller checks its lengths).  Any row of coeffs[b] up to F - 1 may be READ,
 * also one at or behind ceil(n[b] / hop) (wn_lpc_synthesis loads the row of
 * the frame after the current one ahead of its use): all F rows must be
 * readable memory; what such a row holds reaches no output.  A NULL pointer but lengths: WN_ERR_NULL.  A
 * shape outside the limits above, ld < T, gain not finite or not positive:
 * WN_ERR_BAD_SHAPE.  4-byte alignment, else WN_ERR_MISALIGNED; where x (out)
 * is 16-byte aligned with ld_x (ld_out) a multiple of 4 the tile is loaded
 * (stored) 16 bytes at a time.  One launch. */
int wn_lpc_analysis(const float* x, long ld_x, const float* coeffs, int F,
                    int order, int hop, const int32_t* lengths, int B, int T,
                    float gain, float* out, long ld_out, void* stream);

/* e, coeffs, lengths, out and the checks as wn_lpc_analysis; out may be e
 * itself (the same pointer and ld), and may overlap it in no other way.  One
 * launch. */
int wn_lpc_synthesis(const float* e, long ld_e, const float* coeffs, int F,
                     int order, int hop, const int32_t* lengths, int B, int T,
                     float inv_gain, float* out, long ld_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* WAVENET_LPC_H_ */
