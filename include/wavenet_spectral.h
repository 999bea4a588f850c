/* wavenet_spectral.h -- the synthesis metrics' part of the C ABI of
 * libwavenet_hip.so (gfx950 / MI355X): csrc/wn_spectral.hip, bound by
 * wavenet/_lib.py's SPECTRAL_SIGNATURES, driven by wavenet/spectral.py.  The
 * contract of wavenet_hip.h holds for every entry (plain C, caller-owned
 * buffers, asynchronous on `stream`, WN_OK or a negative WN_ERR_* code, all
 * checks before any launch).
 *
 * ---- wn_stft_distance: one resolution of the multi-resolution STFT distance
 * (spectral convergence and log STFT magnitude, the Parallel WaveGAN
 * definition) between a generated and an original signal.  wavenet/spectral.py:
 * StftDistance.reference states the rule in numpy, tests/stft_ref.py restates
 * it in float64.
 *
 * The frame grid is wn_melspec's: F = ceil(T / hop); clip b has n[b] =
 * lengths ? min(max(lengths[b], 0), T) : T samples and Fb = ceil(n[b] / hop)
 * real frames; frame f is centred at c = f * hop + hop / 2 and is
 *   frame[j] = x[c - n_fft / 2 + j] * window[j]      x = 0 outside [0, n[b])
 * for both signals; nothing at or behind n[b] is read in either.
 *
 * Per real frame f < Fb and bin k < n_bins = n_fft / 2 + 1, with (re_g, im_g)
 * and (re_o, im_o) the float32 DFTs of the generated and the original frame
 * (sums of float32 products with the basis table; im of bin 0 and of the
 * Nyquist bin is an exact zero, what it is -- the table's sin(pi j) = 1.2e-16
 * is not read -- and the Nyquist bin's cos row is (-1)^j).
 * Every line is ONE float32 operation per operator, no fused multiply-add:
 *   Pg = re_g * re_g + im_g * im_g
 *   Po = re_o * re_o + im_o * im_o
 *   Cg = Pg < floor_ ? floor_ : Pg                     (a NaN passes)
 *   Co = Po < floor_ ? floor_ : Po
 *   mg = sqrtf(Cg)
 *   mo = sqrtf(Co)
 *   d  = mo - mg
 *   l  = fabsf(logf(Co) - logf(Cg)) * 0.5f
 * then in float64, the float32 values widened first:
 *   sc_num[b]  += (double)d * (double)d
 *   sc_den[b]  += (double)mo * (double)mo
 *   log_sum[b] += (double)l
 * Frames f >= Fb add nothing, and no padding bin is ever summed (the floor_
 * would otherwise leak into sc_den).
 *
 * The summation order, the only one: tile t of clip b holds the frames
 * 32 t .. 32 t + 31; inside it lane (i, h), i = frame - 32 t, h = 0 or 1, of
 * wave w adds, from zero, its terms of the bin chunks c = w, w + 8, ... <
 * n_fft / 64 in ascending order and inside a chunk the bins 32 c + 8 q + 4 h +
 * e, q = 0 .. 3 outer, e = 0 .. 3 inner, the Nyquist bin n_fft / 2 right
 * behind bin 0; the 64 lanes of a wave are added by the xor
 * butterfly (32, 16, 8, 4, 2, 1), the eight waves in the order 0, 1, ... 7
 * from zero; a clip's tiles are added in ascending order from zero (a tile
 * behind the clip's last frame is +0.0).  No atomics.  Clip b's three numbers
 * are a function of its own samples, n[b] and the tables: not of B, T, the
 * clip's position or its neighbours.  gen == org gives sc_num = log_sum =
 * +0.0.  A NaN sample reaches its own clip's numbers only.
 *
 * ---- wn_cepstral_distance: the sum over a clip's real frames of the
 * distance of the mel cepstra (DCT-II of the log-mel spectrum, c0 excluded) of
 * two RAW log-mel tensors (natural log of power).  wavenet/spectral.py:
 * cepstral_reference states the rule in numpy.
 *
 * Fb = nframes ? min(max(nframes[b], 0), F) : F.  Per real frame:
 *   d[m] = (double)(a[m] - b[m])                      ONE float32 subtraction
 *   e[n] = sum_m dct[n][m] * d[m]     float64, from zero, m ascending, every
 *                                     product rounded before it is added
 *   s    = sum_n e[n] * e[n]          float64: the xor butterfly (32, ... 1)
 *                                     over 64 lanes, lane n holding e[n]^2,
 *                                     lanes n >= K holding zeros
 *   r    = sqrt(0.5 * s)
 * (the cepstrum of log AMPLITUDE is half that of log power: r =
 * sqrt(2 sum (e / 2)^2)).  mcd_sum[b] = sum_f r: chunk k of a clip holds the
 * frames 64 k .. 64 k + 63; wave w of its workgroup adds the frames 64 k + w,
 * 64 k + w + 4, ... in ascending order from zero, the four waves are added in
 * the order 0, 1, 2, 3 from zero, a clip's chunks in ascending order from
 * zero.  No atomics; a clip's number does not depend on the batch; a == b
 * gives +0.0; frames at or behind Fb are not read.
 */
#ifndef WAVENET_SPECTRAL_H_
#define WAVENET_SPECTRAL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no device: the doubles of wn_stft_distance's `partials` (three
 * per tile of 32 frames per clip).  -1 for B outside [1, 65535], T outside
 * [1, 2^30] or hop < 1. */
long wn_stft_distance_partials(int B, int T, int hop);

/* Host only, no device: 1 where wn_stft_distance stages both signals' tile
 * samples in LDS at this (n_fft, hop), 0 where it reads them from memory (and
 * for arguments wn_stft_distance refuses).  The two paths give the same bits;
 * tests stand either side of the edge. */
int wn_stft_distance_staged(int n_fft, int hop);

/* gen, org: device float, clip b at + b * ld_gen / + b * ld_org, T samples;
 * lengths: device int32 [B] or NULL; window: device float [n_fft]; basis:
 * device float [ceil(n_bins / 32)][n_fft][64], wn_melspec's tables; sc_num,
 * sc_den, log_sum: device double [B]; partials: device double
 * [wn_stft_distance_partials(B, T, hop)], scratch.
 * A NULL pointer but lengths: WN_ERR_NULL.  n_fft not a multiple of 64 in
 * [64, 2048], hop outside [1, n_fft], n_bins != n_fft / 2 + 1, floor_ not a
 * positive finite number, B outside [1, 65535], T outside [1, 2^30], ld_gen
 * or ld_org < T: WN_ERR_BAD_SHAPE.  basis 16-byte, the double arrays 8-byte,
 * everything else 4-byte aligned, else WN_ERR_MISALIGNED.  All of it before
 * any launch.  Two launches: the tiles, then the clips' sums. */
int wn_stft_distance(const float* gen, long ld_gen, const float* org, long ld_org,
                     int B, int T, const int32_t* lengths, const float* window,
                     const float* basis, int n_fft, int hop, int n_bins,
                     float floor_, double* sc_num, double* sc_den,
                     double* log_sum, double* partials, void* stream);

/* Host only, no device: the doubles of wn_cepstral_distance's `partials` (one
 * per chunk of 64 frames per clip).  -1 for B < 1, F < 1 or B * F > 2^31 - 1. */
long wn_cepstral_distance_partials(int B, int F);

/* a, b: device float [B][F][C]; nframes: device int32 [B] or NULL; dct: device
 * double [K][C], dct[n - 1][m] = sqrt(2 / C) cos(pi n (m + 1/2) / C), n = 1 ..
 * K; mcd_sum: device double [B]; partials: device double
 * [wn_cepstral_distance_partials(B, F)], scratch.
 * A NULL pointer but nframes: WN_ERR_NULL.  C outside [1, 512], K outside
 * [1, min(C - 1, 64)], B < 1, F < 1, B * F > 2^31 - 1: WN_ERR_BAD_SHAPE.  The
 * double arrays 8-byte, everything else 4-byte aligned, else
 * WN_ERR_MISALIGNED.  All of it before any launch. */
int wn_cepstral_distance(const float* a, const float* b, int B, int F, int C,
                         const int32_t* nframes, const double* dct, int K,
                         double* mcd_sum, double* partials, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* WAVENET_SPECTRAL_H_ */
