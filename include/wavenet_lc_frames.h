/* wavenet_lc_frames.h -- the conditioning-frame assembler's part of the C ABI
 * of libwavenet_hip.so (gfx950 / MI355X): csrc/wn_lc_frames.hip, bound by
 * wavenet/_lib.py's LC_FRAMES_SIGNATURES, driven by wavenet/frontend.py's
 * MelPitchSpec.  The contract of wavenet_hip.h holds for every entry (plain C,
 * caller-owned buffers, asynchronous on `stream`, WN_OK or a negative WN_ERR_*
 * code, all checks before any launch).
 *
 * The rule (wavenet/frontend.py: MelPitchSpec.reference and
 * reference_channels state it in numpy, tests/lc_frames_ref.py restates it in
 * float64 Python loops): the local-conditioning frames of a mel + F0 front
 * end, out[b][f][0 .. ld_out), from the log-mel frames mel[b][f][0 .. M) and
 * the F0 track f0[b][f] of the same clips on the same frame grid.
 *
 * Fb = nframes ? min(max(nframes[b], 0), F) : F real frames in clip b.
 *
 * Mel channels, c < M, on a real frame f < Fb.  Every line is ONE float32
 * operation, no fused multiply-add (the rule of wn_feature_normalize):
 *   without a normaliser (shift == scale == NULL)
 *     out[b][f][c] = mel[b][f][c]
 *   with one
 *     d = mel[b][f][c] - shift[c]
 *     v = d * scale[c]
 *     out[b][f][c] = v < lo ? lo : (v > hi ? hi : v)       a NaN stays a NaN
 *
 * Pitch channels, on a real frame.  Frame f is voiced iff f < Fb and
 * f0[b][f] > 0 (a NaN is unvoiced).  Every line is ONE float64 operation:
 *   q    = (double)f0[b][f] / fmin
 *   l    = log2(q)
 *   r0   = l / span                          span = log2(fmax / fmin), the host's
 *   r[f] = r0 < 0 ? 0 : (r0 > 1 ? 1 : r0)
 *   out[b][f][c0 + 1] = voiced ? 1 : 0                     both modes
 *   mode 0 ("zero"):   out[b][f][c0] = voiced ? (float)r[f] : 0
 *   mode 1 ("interp"): a voiced frame as in mode 0; an unvoiced real frame
 *     with a = the nearest voiced frame before it, e = the nearest behind it:
 *       both:    w = (double)(f - a) / (double)(e - a)
 *                d = r[e] - r[a]
 *                s = d * w
 *                out[b][f][c0] = (float)(r[a] + s)
 *       only e:  out[b][f][c0] = (float)r[e]
 *       only a:  out[b][f][c0] = (float)r[a]
 *       neither: out[b][f][c0] = 0
 *
 * Frames f >= Fb: every channel the call owns is an exact zero; nothing of
 * mel or f0 is read there.  The call owns columns [0, M) with a mel, c0 and
 * c0 + 1 with an f0; no other column of out is ever written.  mel == NULL
 * leaves [0, M) untouched, f0 == NULL leaves c0 and c0 + 1 untouched.
 * out == mel with ld_out == ld_mel (in place) is allowed: c0 >= M is required.
 *
 * No atomics.  Clip b's bits are a function of its own rows, nframes[b] and
 * the settings: not of B or the other clips.
 *
 * The kernel: workgroups of 1024 lanes, a grid of B x Y.  The mel part is a
 * strided copy, a clip's rows split over its Y <= 1024 workgroups (256 rows
 * each at least), four rows in flight per lane, in 16-byte accesses where M,
 * ld_mel and ld_out are multiples of 4 and mel, out, shift and scale are
 * 16-byte aligned, else in 4-byte ones; every element is read and written by
 * one lane.  The pitch part is one workgroup per clip (the first of its Y): it
 * walks the clip in chunks of
 * wn_lc_frames_chunk() frames, a lane per frame: mode 1 first walks DOWN from
 * the last real chunk with a suffix-min scan of the voiced frame indices,
 * carrying the running minimum (the nearest voiced frame behind) across
 * chunks, and parks each frame's index as an int32 in the frame's own voicing
 * slot out[b][f][c0 + 1]; then both modes walk UP with a prefix-max scan,
 * carrying the running maximum (the nearest voiced frame before), and the lane
 * that parked an index reads it back and writes both channels.  No workspace.
 */
#ifndef WAVENET_LC_FRAMES_H_
#define WAVENET_LC_FRAMES_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no device: the frames one scan step of the pitch part covers (a
 * chunk).  Tests stand on its multiples. */
int wn_lc_frames_chunk(void);

/* mel: device float [B][F][ld_mel] or NULL; shift, scale: device float [M],
 * both or neither; f0: device float [B][F] or NULL; nframes: device int32 [B]
 * (clamped to [0, F] by the kernel, read when it runs) or NULL (Fb = F); out:
 * device float [B][F][ld_out].
 * NULL out, mel and f0 both NULL, one of shift / scale alone: WN_ERR_NULL.
 * B outside [1, 65535], F outside [1, 2^30], M outside [0, 512], ld_out < 1,
 * ld_out < M or a leading dimension above 2^20; with a mel: M < 1, ld_mel < M,
 * with a normaliser lo > hi or a NaN bound; with an f0: c0 < M, c0 + 2 >
 * ld_out, mode not 0 or 1, fmin or span not a positive finite number:
 * WN_ERR_BAD_SHAPE.  Every pointer 4-byte aligned, else WN_ERR_MISALIGNED.
 * All of it before any launch. */
int wn_lc_frames(const float* mel, long ld_mel, int M, const float* shift,
                 const float* scale, float lo, float hi, const float* f0,
                 int mode, double fmin, double span, const int32_t* nframes,
                 int B, int F, float* out, long ld_out, int c0, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* WAVENET_LC_FRAMES_H_ */
