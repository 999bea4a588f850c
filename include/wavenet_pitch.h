/* wavenet_pitch.h -- the pitch tracker's part of the C ABI of
 * libwavenet_hip.so (gfx950 / MI355X): csrc/wn_pitch.hip, bound by
 * wavenet/_lib.py's PITCH_SIGNATURES, driven by wavenet/pitch.py.  The
 * contract of wavenet_hip.h holds for every entry (plain C, caller-owned
 * buffers, asynchronous on `stream`, WN_OK or a negative WN_ERR_* code, all
 * checks before any launch).
 *
 * The rule (wavenet/pitch.py: PitchTracker.reference states it in numpy,
 * tests/pitch_ref.py restates it in float64): a YIN-style tracker on the
 * local-conditioning frame grid of wn_melspec -- frame f sits beside samples
 * f * hop .. f * hop + hop - 1, is centred at c = f * hop + hop / 2, and there
 * are F = ceil(T / hop) frames.
 *
 * Settings: sample_rate (float32); hop in [1, 4096]; window W, a multiple of
 * 64 in [64, 2048]; the lag range tau_min + 2 <= tau_max <= 1024, tau_min >=
 * 2; threshold in (0, 1); silence >= 0 (a mean square).  The lag range of a
 * frequency range fmin < fmax, computed in double from the float32 values:
 *   tau_min = max(2, floor(sample_rate / fmax))
 *   tau_max = ceil(sample_rate / fmin)
 *
 * Per frame, with N = W + tau_max, s = c - N / 2 (integer division) and
 *   y[j] = x[s + j] where 0 <= s + j < n[b], else 0,        j < N
 * (nothing at or behind n[b] is read):
 *
 * 1. e = sum_{j < W} y[j]^2 in float32, in this order: with 256 lanes, lane t
 *    chains p = fmaf(y[j], y[j], p) from 0 over j = t, t + 256, ... ascending;
 *    the 64 lanes of a wave are added by the xor butterfly (32, 16, 8, 4, 2,
 *    1), the four waves in the order ((w0 + w1) + w2) + w3.  If e <=
 *    silence * W (a float32 product) the frame is SILENT: f0 = 0, aper = 1,
 *    lag = 0, its cmnd row is all 1.
 * 2. d[tau] = sum_{j < W} (y[j] - y[j + tau])^2, tau = 1 .. tau_max, float32,
 *    in the direct form (no autocorrelation identity: no cancellation), in
 *    this order: the W values of j are cut into 8 consecutive segments of
 *    W / 8; segment k chains q_k = fmaf(v, v, q_k) from 0 with v = y[j] -
 *    y[j + tau] (one float32 subtraction) over its j ascending;
 *    d[tau] = ((((((q0 + q1) + q2) + q3) + q4) + q5) + q6) + q7.
 * 3. S[tau] = sum_{k = 1 .. tau} d[k] in float64, sequentially, ascending.
 *    c'[tau] = float32(d[tau] * tau / S[tau]) (float64 product -- exact -- and
 *    division, rounded once more to float32) where S[tau] > 0, else 1;
 *    c'[0] = 1.
 * 4. The pick.  The first tau in [tau_min, tau_max - 1] with c'[tau] <
 *    threshold; then, while tau + 1 <= tau_max - 1 and c'[tau + 1] < c'[tau],
 *    tau + 1: the frame is VOICED.  Without one, tau is the smallest index
 *    that attains the minimum of c' over that range: UNVOICED.
 * 5. lag = tau and aper = c'[tau], voiced or not.  A voiced frame gets, in
 *    float32 with a, b, g = c'[tau - 1], c'[tau], c'[tau + 1]:
 *      den   = (a - 2 b) + g
 *      delta = den > 0 ? clamp(0.5 (a - g) / den, -0.5, 0.5) : 0
 *      f0    = sample_rate / (tau + delta)
 *    an unvoiced frame f0 = 0.  "Voiced" is f0 > 0 everywhere downstream.
 * 6. Frames f >= ceil(n[b] / hop) are exact zeros in every output.
 *
 * No atomics.  A frame's bits are a function of its own N samples and the
 * settings: not of B, the other clips or the frame's position in the launch.
 *
 * The kernel: one workgroup of 256 lanes (four waves) per frame.  The N
 * samples are staged in LDS once, shifted by three floats so that y[j + 4 g +
 * 1], j % 4 == 0, is 16-byte aligned, beside an aligned copy of y[0 .. W).  A
 * work unit is (segment k, lag group g): the four lags 4 g + 1 .. 4 g + 4 over
 * segment k; the units are dealt to the lanes in the order k * groups + g, so
 * the lanes of a wave read the same y[j .. j + 3] (one 16-byte LDS broadcast)
 * and lane-consecutive 32 bytes of y[j + tau]: three 16-byte LDS reads feed 16
 * subtract + fma pairs.  The segment sums go through LDS; lane 0 runs the
 * float64 prefix; c', the first lag under the threshold and the minimum are
 * found by all lanes (wave shuffles, then the four waves in order); lane 0
 * walks down, interpolates and writes f0, aper and lag.  Staging ALWAYS fits:
 * the launch asks for
 *   wn_pitch_lds_bytes = 4 * (NS + W + 8 * G4) + 64 bytes,
 *   NS = (N + 8) rounded up to 4,  G4 = tau_max rounded up to 4,
 * 53344 bytes at most (W 2048, tau_max 1024); there is no path that reads
 * samples from memory where they are used. */
#ifndef WAVENET_PITCH_H_
#define WAVENET_PITCH_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no device: the lag range of (sample_rate, fmax) / (sample_rate,
 * fmin) by the formulas above; -1 for a value that is not positive and finite
 * or a lag beyond 2^30.  wavenet/pitch.py computes the same numbers. */
int wn_pitch_tau_min(float sample_rate, float fmax);
int wn_pitch_tau_max(float sample_rate, float fmin);

/* Host only, no device: the dynamic LDS of a launch in bytes (above); -1 for
 * a window, tau_max or hop outside the ranges above. */
long wn_pitch_lds_bytes(int window, int tau_max, int hop);

/* audio float [B][ld] (ld >= T); lengths: device int32 [B] (n[b], clamped to
 * [0, T] by the kernel, read when it runs) or NULL (n[b] = T).  Outputs, F =
 * ceil(T / hop): f0, aper float [B][F]; lag int32 [B][F]; cmnd float
 * [B][F][tau_max + 1] (c'[0 .. tau_max] of every frame) or NULL (not
 * written; the other outputs have the same bits either way).
 * NULL audio, f0, aper or lag: WN_ERR_NULL.  Settings outside the ranges
 * above, B outside [1, 65535], T outside [1, 2^30], ld < T:
 * WN_ERR_BAD_SHAPE.  Every pointer 4-byte aligned, else WN_ERR_MISALIGNED.
 * All of it before any launch. */
int wn_pitch_track(const float* audio, const int32_t* lengths, long ld, int B,
                   int T, int hop, int window, int tau_min, int tau_max,
                   float threshold, float silence, float sample_rate,
                   float* f0, float* aper, int32_t* lag, float* cmnd,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* WAVENET_PITCH_H_ */
