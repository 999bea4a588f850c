/* wavenet_resample.h -- the sample-rate converter's part of the C ABI of
 * libwavenet_hip.so (gfx950 / MI355X): csrc/wn_resample.hip, bound by
 * wavenet/_lib.py's RESAMPLE_SIGNATURES, driven by wavenet/resample.py.  The
 * contract of wavenet_hip.h holds for every entry (plain C, caller-owned
 * buffers, asynchronous on `stream`, WN_OK or a negative WN_ERR_* code, all
 * checks before any launch, no atomics, one summation order).  A clip's output
 * is a function of its own samples, its length and the taps: not of B, the
 * clip's position, T or where an output falls in the kernel's tiles.
 * wavenet/resample.py: Resampler.reference states the rule in numpy float32,
 * tests/resample_ref.py restates it independently in float64.
 *
 * up / down is the reduced ratio rate_out / rate_in, m = max(up, down), Hh =
 * half_width * m, and h32[-Hh .. Hh] the float32 taps (the host's: a Kaiser-
 * windowed sinc of cutoff 1 / m with gain up).  1 <= up, down <= 1024, 0 <=
 * Hh, 2 Hh + 1 <= 65537, 1 <= B <= 65535, 1 <= T <= 2^30 and T_out =
 * ceil(T up / down) <= 2^30.
 *
 * The taps arrive by phase: with LP = (2 Hh + up) / up (integer division: the
 * taps of the longest phase) and LPS = LP | 1,
 *   tab[r * LPS + t] = h32[r + t * up - Hh]    0 <= r < up, r + t * up <= 2 Hh
 * and zeros elsewhere (never multiplied): up * LPS floats.
 *
 * ---- wn_resample: n[b] = lengths ? min(max(lengths[b], 0), T) : T, n_out[b]
 * = ceil(n[b] up / down).  For k < n_out[b], every line ONE rounded float32
 * operation, no fused multiply-add:
 *   c   = k * down + Hh                 (exact integers)
 *   jh  = c / up                        (integer division)
 *   r   = c - jh * up
 *   acc = +0
 *   acc = acc + tab[r * LPS + t] * x[jh - t]
 *                                       t = (2 Hh - r) / up down to 0, only
 *                                       where 0 <= jh - t < n[b]
 *   y[k] = acc
 * which is y[k] = sum_j h32[k down - j up] x[j] over 0 <= j < n[b] with |k down
 * - j up| <= Hh, j ascending, the product rounded before it is added.  y[k] =
 * +0 for n_out[b] <= k < T_out; nothing at or behind n[b] is read; a NaN
 * sample reaches the outputs whose taps cover it and no other.  up == down (1
 * / 1) is a copy, y[k] = x[k] for k < n[b], and tab is not read (the
 * windowed sinc is a unit impulse only up to rounding: its 2 Hh side taps of
 * 1e-17 would let a NaN reach 2 Hh neighbours for nothing).
 *
 * A workgroup serves wn_resample_tile() outputs of one clip.
 */
#ifndef WAVENET_RESAMPLE_H_
#define WAVENET_RESAMPLE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no device: the outputs one workgroup of wn_resample serves. */
int wn_resample_tile(void);

/* x: device float, clip b at + b * ld_x, T samples; lengths: device int32 [B]
 * or NULL; tab: device float [up * LPS] as above; out: device float, clip b at
 * + b * ld_out, T_out = ceil(T up / down) samples written.  out must not
 * overlap x.  A NULL pointer but lengths: WN_ERR_NULL.  A shape outside the
 * limits above, up and down not coprime, ld_x < T, ld_out < T_out:
 * WN_ERR_BAD_SHAPE.  4-byte alignment, else WN_ERR_MISALIGNED.  One launch. */
int wn_resample(const float* x, long ld_x, const int32_t* lengths, int B, int T,
                int up, int down, int Hh, const float* tab, float* out,
                long ld_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* WAVENET_RESAMPLE_H_ */
