/* wavenet_stoi.h -- STOI / ESTOI's part of the C ABI of libwavenet_hip.so
 * (gfx950 / MI355X): csrc/wn_stoi.hip, bound by wavenet/_lib.py's
 * STOI_SIGNATURES, driven by wavenet/stoi.py.  The contract of wavenet_hip.h
 * holds for every entry (plain C, caller-owned buffers, asynchronous on
 * `stream`, WN_OK or a negative WN_ERR_* code, all checks before any launch, no
 * atomics, one summation order).  A clip's numbers are a function of its own
 * samples and length only: not of B, the clip's position, T or its
 * neighbours.  wavenet/stoi.py: Stoi.reference states the rule in numpy (steps
 * 2 - 4 in float32, step 5 in float64), tests/stoi_ref.py restates it
 * independently in float64.
 *
 * Short-time objective intelligibility (Taal, Hendriks, Heusdens, Jensen 2011)
 * and its extended form (Jensen, Taal 2016) of a generated signal y against
 * the original x, both at 10 kHz (step 1, the resampling, is wn_resample's),
 * n = n[b] samples each.  Frame length 256, hop 128, DFT length 512, 15
 * third-octave bands, 30 frames per segment, c = 10^(15/20) =
 * 5.623413251903491, eps = 2^-52.  1 <= B <= 65535, 1 <= T <= 2^30.
 *
 * 2. Window and frames.  w[i] = sin^2(pi (i + 1) / 257), i < 256, float64
 *    rounded to float32 (the caller's `window`).  Frame f starts at 128 f; Fs =
 *    (n - 256) / 128 + 1 (integer division), 0 for n < 256.
 * 3. Silent frames, decided on x alone, float32, one rounded operation per
 *    line:
 *      p    = w[i] * x[128 f + i]
 *      q    = p * p
 *      E[f] = E[f] + q                  from +0, i = 0 .. 255 ascending
 *      Emax = max(+0, E[f] over f)      (a NaN E[f] is passed over)
 *      thr  = Emax * 1e-4f
 *      frame f is kept iff E[f] > thr   (a NaN frame is dropped)
 *    The kept frames k_0 < ... < k_{M-1} define both compacted signals,
 *      x'[128 i + j] = 0 + w[j + 128] * x[128 k_{i-1} + j + 128]   (i >= 1)
 *                        + w[j]       * x[128 k_i + j]             j < 128
 *      x'[128 i + j] = 0 + w[j]       * x[128 k_i + j]
 *                        + w[j - 128] * x[128 k_{i+1} + j - 128]   (i + 1 < M)
 *                                                           128 <= j < 256
 *    every product rounded, the earlier frame's addend first; y' the same with
 *    y at the SAME k_i.
 * 4. Band amplitudes of compacted frame i < M, float32:
 *      v[j]  = x'[128 i + j] * w[j]                         j < 256
 *      re[k] = re[k] + cos[(k j) mod 512] * v[j]            from +0, j ascending
 *      im[k] = im[k] + sin[(k j) mod 512] * v[j]            from +0, j ascending
 *      P[k]  = re[k] * re[k] + im[k] * im[k]                (three operations)
 *      X[b][i] = sqrtf(P[L_b] + P[L_b + 1] + ... + P[U_b - 1])   from +0,
 *                                                           k ascending
 *    cos | sin: the caller's `basis`, float [2][512], cos(2 pi q / 512) and
 *    sin(2 pi q / 512) in float64 rounded to float32.  No fused multiply-add.
 *    L = 7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174 and U_b =
 *    L_{b+1}, U_14 = 219: the bins nearest to 150 * 2^(b/3) * 2^(-+1/6) Hz on
 *    the 10000 / 512 Hz grid (wn_stoi_band_edge).  Y from y' the same way.
 * 5. Segments, float64 (the float32 amplitudes widened).  Segment s = 0 .. M
 *    - 30 holds frames s .. s + 29; sum_m runs over them, sum_b over the bands.
 *    STOI, per band, with x = X[b][.], y = Y[b][.]:
 *      alpha = sqrt(sum_m x^2) / (sqrt(sum_m y^2) + eps)
 *      y     = min(alpha * y, (1 + c) * x)
 *      x     = x - (sum_m x) / 30;  y = y - (sum_m y) / 30
 *      x     = x / (sqrt(sum_m x^2) + eps);  y likewise
 *      d_b   = sum_m x * y
 *    and the segment's value is (sum_b d_b) / 15.  ESTOI, on the 15 x 30
 *    blocks X and Y, unclipped: every row (band) is made zero-mean and divided
 *    by (its norm + eps) as above, then every column (frame) is made zero-mean
 *    over the 15 bands and divided by (its norm + eps), and the segment's
 *    value is (sum_m sum_b x * y) / 30.
 *    A sum over m is taken over the lanes of one wave, frame m on lane m, by the
 *    prefix network of wn_common.h's wave_scan_f64 (six steps: row shifts by 1,
 *    2, 4, 8, then the broadcasts of lanes 15 and 31); a sum over b runs b
 *    ascending from zero.
 * 6. Per clip: segments[b] = max(M - 29, 0), kept[b] = M, and stoi_sum[b],
 *    estoi_sum[b] the float64 sums of the segments' values: thread t of 256
 *    adds the segments t, t + 256, ... ascending from zero, and the 256
 *    partial sums are added t ascending from zero.  n < 256, Emax not above
 *    zero and M < 30 all give segments 0 and sums +0.0.
 *
 * Nothing at or behind n[b] is read.
 */
#ifndef WAVENET_STOI_H_
#define WAVENET_STOI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no device: band edge i of the kernels, i = 0 .. 15 (L_0 .. L_14,
 * U_14); -1 outside. */
int wn_stoi_band_edge(int i);

/* Host only: the bytes of wn_stoi's scratch for B clips of T samples (frame
 * energies, kept-frame indices, both signals' band amplitudes, the segments'
 * values); a negative WN_ERR_* for a shape outside the limits. */
long wn_stoi_scratch_bytes(int B, int T);

/* gen, org: device float at 10 kHz, clip b at + b * ld, T samples; lengths:
 * device int32 [B] or NULL (n[b] = min(max(lengths[b], 0), T), else T);
 * window: device float [256]; basis: device float [2][512]; scratch: device,
 * wn_stoi_scratch_bytes(B, T) bytes, 8-byte aligned, its contents afterwards
 * unspecified; stoi_sum, estoi_sum: device double [B]; segments, kept: device
 * int32 [B].  A NULL pointer but lengths: WN_ERR_NULL.  B outside [1, 65535],
 * T outside [1, 2^30], ld < T: WN_ERR_BAD_SHAPE.  scratch and the sums 8-byte,
 * everything else 4-byte aligned, else WN_ERR_MISALIGNED.  Four launches
 * (frames and the keep decision; band amplitudes; segments; per-clip sums);
 * clips shorter than 256 samples take part in the first and the last only. */
int wn_stoi(const float* gen, long ld_gen, const float* org, long ld_org,
            const int32_t* lengths, int B, int T, const float* window,
            const float* basis, void* scratch, double* stoi_sum,
            double* estoi_sum, int32_t* segments, int32_t* kept, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* WAVENET_STOI_H_ */
