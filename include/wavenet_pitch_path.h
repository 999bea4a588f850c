/* wavenet_pitch_path.h -- the pitch path's part of the C ABI of
 * libwavenet_hip.so (gfx950 / MI355X): csrc/wn_pitch_path.hip, bound by
 * wavenet/_lib.py's PITCH_PATH_SIGNATURES, driven by wavenet/pitch.py's
 * PitchPath.  The contract of wavenet_hip.h holds for every entry (plain C,
 * caller-owned buffers, asynchronous on `stream`, WN_OK or a negative WN_ERR_*
 * code, all checks before any launch).
 *
 * The rule (wavenet/pitch.py: PitchPath.reference states it in numpy float32,
 * tests/pitch_path_ref.py restates its direct O(N^2) form in float64): a
 * dynamic-programming (Viterbi) path over the frames of one clip, through the
 * lag candidates the tracker of wavenet_pitch.h left in its c' rows.
 *
 * Inputs per clip: cmnd[f][0 .. tau_max], the tracker's c' rows; lag[f] of the
 * tracker (0: the frame is silent); Fb real frames; two float32 tables of
 * tau_max + 1 entries, made on the host in float64 and rounded once,
 *   pen[k]  = float32(jump * log2(max(k, 1)))
 *   bias[k] = float32(octave_bias * (log2(max(k, 1)) - log2(tau_min)))
 * and the float32 scalars `switch` and `unvoiced`.
 *
 * States: s = 0 .. N - 1 is the voiced lag tau_min + s, N = tau_max - tau_min
 * (2 <= N <= 1022: the lags the tracker may pick); state N is unvoiced.
 * p[s] = pen[tau_min + s].  Every line is ONE float32 operation, no fused
 * multiply-add:
 *
 *   loc[s] = cmnd[f][tau_min + s] + bias[tau_min + s]
 *   lu     = lag[f] == 0 ? 0 : unvoiced
 *   frame 0:  nV = loc, nU = lu
 *   frame f > 0, from the previous V[0 .. N) and U:
 *     A[k]  = V[k] - p[k]            Bk[k] = V[k] + p[k]
 *     ma[s] = min_{k <= s} A[k],  ia[s] the smallest such k
 *     mb[s] = min_{k >= s} Bk[k], ib[s] the smallest such k
 *     L = ma[s] + p[s]               R = mb[s] - p[s]
 *     vv = L <= R ? L : R            predecessor ia[s] : ib[s]
 *     fu = U + switch
 *     pv = vv <= fu ? vv : fu        predecessor (the voiced one) : N
 *     nV[s] = pv + loc[s]
 *     kb = the smallest index of min V,  fv = V[kb] + switch
 *     U <= fv ? nU = U + lu, predecessor N : nU = fv + lu, predecessor kb
 *   normalise (every frame, frame 0 included):
 *     m = min(min nV, nU);  V = nV - m;  U = nU - m;  cost += m in float64
 *   end, after frame Fb - 1: the last state is N if U <= min V, else the
 *     smallest index of min V; the stored predecessors lead back to frame 0.
 *
 * Outputs per frame: a voiced state gives lag = tau, aper = cmnd[f][tau] and
 * f0 by step 5 of wavenet_pitch.h (the same den, delta, clamp and division in
 * float32, a, b, g = cmnd[f][tau - 1 .. tau + 1]); the unvoiced state f0 = 0,
 * lag = 0, aper = 1.  Frames f >= Fb are exact zeros in every output; Fb = 0
 * writes zeros and cost = 0.  cost[b] is float64: the sum of the frames' m.
 *
 * Min with "the smallest index at ties" is associative, so any scan shape
 * gives the same bits; the two one-sided minima are the exact decomposition of
 * min_k V[k] + jump |log2 tau_s - log2 tau_k|: a frame costs O(N), not O(N^2).
 *
 * EVERY PREDECESSOR INDEX IS VALID, in [0, N], whatever bits the inputs hold,
 * NaN and infinities included: an index is only ever copied from a state's
 * own index (clamped to N - 1 on the lanes behind the last state) or is the
 * constant N, both branches of every comparison name such an index, and the
 * walk back clamps what it reads.  A bad input can give a meaningless path,
 * never a read or a write outside the operands.
 *
 * No atomics.  Clip b's bits are a function of its own rows, nframes[b] and
 * the settings: not of B or the other clips.
 *
 * The kernel: one workgroup per clip; a lane owns four consecutive states in
 * registers, so 64 lanes (one wave, no cross-wave traffic) serve N <= 256 and
 * 256 lanes (four waves) every larger N.  Per frame: the lane scans its four
 * states, the wave runs an inclusive min-with-index scan upwards for A (and
 * for min V) and the mirrored one downwards for Bk, by DPP row shifts, the
 * waves' totals cross through 24 LDS words and one barrier; a second barrier
 * carries the frame's minimum m.  The next frame's c' values are loaded before the scans.  Predecessors
 * go to the workspace as int16 rows [B][F][N + 1].  After the last frame lane
 * 0 walks back and writes `lag`; then all lanes write f0 and aper.  The grid
 * is B workgroups: the recurrence is serial in f and does not fill the device;
 * what counts is the time per frame of the chain. */
#ifndef WAVENET_PITCH_PATH_H_
#define WAVENET_PITCH_PATH_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no device: the bytes of the predecessor workspace, int16
 * [B][F][tau_max - tau_min + 1]; -1 for B outside [1, 65535], F outside
 * [1, 2^20] or lags outside 2 <= tau_min, tau_min + 2 <= tau_max <= 1024. */
long wn_pitch_path_workspace_bytes(int B, int F, int tau_min, int tau_max);

/* cmnd float [B][F][tau_max + 1] and lag_in int32 [B][F] as wn_pitch_track
 * wrote them; nframes: device int32 [B] (Fb, clamped to [0, F] by the kernel,
 * read when it runs) or NULL (Fb = F); pen, bias: device float [tau_max + 1];
 * workspace: wn_pitch_path_workspace_bytes bytes.  Outputs: f0, aper float
 * [B][F]; lag int32 [B][F]; cost double [B].
 * NULL cmnd, lag_in, pen, bias, workspace, f0, aper, lag or cost: WN_ERR_NULL.
 * B, F or the lags outside the limits above: WN_ERR_BAD_SHAPE.  Every pointer
 * 4-byte aligned (cost 8, workspace 2), else WN_ERR_MISALIGNED.  All of it
 * before any launch. */
int wn_pitch_path(const float* cmnd, const int32_t* lag_in,
                  const int32_t* nframes, int B, int F, int tau_min,
                  int tau_max, const float* pen, const float* bias,
                  float switch_cost, float unvoiced_cost, float sample_rate,
                  void* workspace, float* f0, float* aper, int32_t* lag,
                  double* cost, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* WAVENET_PITCH_PATH_H_ */
