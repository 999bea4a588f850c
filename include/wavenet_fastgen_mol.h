/* wavenet_fastgen_mol.h -- batched fast generation for mixture-of-logistics
 * models, a part of the C ABI of libwavenet_hip.so (gfx950 / MI355X):
 * csrc/wn_fastgen_mol.hip, bound by wavenet/_lib.py's FASTGEN_MOL_SIGNATURES,
 * driven by wavenet/fastgen.py (WaveNetModel.generate_mixture_batch).  The
 * contract of wavenet_hip.h holds for every entry (plain C, caller-owned
 * buffers, asynchronous on `stream`, WN_OK or a negative WN_ERR_* code, all
 * checks before any launch, no atomics, one summation order, every choice of a
 * kernel a function of the arguments).
 *
 * The generator is wn_fastgen_batch_*'s (wavenet_hip.h): B streams in lock
 * step, Bp = wn_fastgen_batch_rows(B) rows, ring state of
 * wn_fastgen_batch_state_floats floats, the past-tap pre-activations, the
 * conditioned-bias ring of wn_fastgen_lc_bias, the skip / post1 / logits tiles
 * and the control block ctl[8] (base, n_given, params_every, temperature bits,
 * row stride of samples_io, rows per stream of params_out; words 6, 7 unused)
 * are those, with Q = 3 Kp logits columns.  Its two ends differ.
 *
 * ---- input: levels.  hist: int32 [Bp][64]; slot T & 63 of stream b's row
 * holds the level the stream consumed at step T, -1 "no sample".  The causal
 * layer (filter W [K0][32], 1 <= K0 <= 32) is the rule of training's scalar
 * input with the reference's centring delay:
 *   x[col] = sum_k W[k][col] * c(hist[(T - s_k) & 63]),
 *   s_k = (K0 - 1 - k) + (K0 - 1) / 2,  c(j) = (float)(2 j - 65535) / 65535,
 * k ascending from +0, one fused multiply-add a tap; a tap whose slot holds no
 * level in 0 .. 65535 is skipped (training's zero padding).  For K0 > 2 the
 * newest (K0 - 1) / 2 levels are not read: the reference's delay.  The reach
 * is at most 46 < 64 slots.
 *
 * ---- output: the mixture.  From the pending logits row [3 Kp] the parameters
 * are wn_mol_params_row's and the draw is wn_mol_sample's (wavenet_mol.h), bit
 * for bit: both share one body with those entries.  counter = the step that
 * produced the logits, or that step - origins[b] where origins is given.
 * Temperature (ctl[3]) >= 0; 0 draws x = mu_k.  The drawn level goes into
 * samples_io[b][local + 1]; every params_every-th step the row [3][K] goes to
 * params_out[b][local / params_every].  Steps with local + 1 < n_given draw
 * nothing (the level is given).
 */
#ifndef WAVENET_FASTGEN_MOL_H_
#define WAVENET_FASTGEN_MOL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Zero rings, cursors = 0, every history slot of all Bp rows = -1.  state
 * 16-byte aligned.  1 <= B <= 256. */
int wn_fastgen_mol_init(float* state, long state_floats, int32_t* cursors,
                        int32_t* hist, int B, void* stream);

/* The past-tap pre-activations of the step the cursors are at
 * (wn_fastgen_batch_pre); lc_ring: NULL (then lc_R, lc_stride are not read)
 * or the conditioned-bias ring.  One launch. */
int wn_fastgen_mol_pre(const float* layer0, long layer_stride,
                       const float* gc_bias_fg, int bias_stream_stride,
                       const int32_t* dilations_dev, int L, int B,
                       const float* state, const int32_t* cursors, float* pre,
                       const float* lc_ring, int lc_R, int lc_stride,
                       void* stream);

/* One lock-step step, five launches.  params_causal: [K0][32]; K: components;
 * logits: [Bp][3 Kp]; params_out: [B][ctl[5]][3][K] or NULL; lc_ring, origins:
 * NULL or as wn_fastgen_batch_step_lc / _q.  seeds 8-byte aligned. */
int wn_fastgen_mol_step(const float* params_causal, int K0,
                        const float* layer0, long layer_stride,
                        const float* skip_w, const float* skip_bsum,
                        const float* post1_w, const float* post1_b,
                        const float* post2_w, const float* post2_b,
                        const float* gc_bias_fg, int bias_stream_stride,
                        const int32_t* dilations_dev, int L, int S, int K,
                        int B, float* state, int32_t* cursors, int32_t* hist,
                        int32_t* samples_io, const int32_t* ctl,
                        const uint64_t* seeds, float* params_out,
                        int use_biases, float log_scale_min, float* pre,
                        float* z_all, float* h1, float* h2, float* logits,
                        const float* lc_ring, int lc_R, int lc_stride,
                        const int32_t* origins, void* stream);

/* The last step's parameters and draw; clears the pending flag. */
int wn_fastgen_mol_finish(int K, float log_scale_min, int B, int32_t* cursors,
                          int32_t* samples_io, const int32_t* ctl,
                          const uint64_t* seeds, float* params_out,
                          const float* logits, const int32_t* origins,
                          void* stream);

/* Streams with flags[b] != 0 become fresh ones at the step the cursors are
 * at: ring columns zeroed, their 64 history slots -1, origins[b] = cursors[0].
 * The other streams' words are not written.  One launch. */
int wn_fastgen_mol_restart(float* state, const int32_t* dilations_dev, int L,
                           int B, const int32_t* cursors, int32_t* hist,
                           int32_t* origins, const int32_t* flags,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* WAVENET_FASTGEN_MOL_H_ */
