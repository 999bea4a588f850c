/* wavenet_mol.h -- the mixture-of-logistics output head's part of the C ABI of
 * libwavenet_hip.so (gfx950 / MI355X): csrc/wn_mol.hip, bound by
 * wavenet/_lib.py's MOL_SIGNATURES, driven by wavenet/mol.py.  The contract of
 * wavenet_hip.h holds for every entry (plain C, caller-owned buffers,
 * asynchronous on `stream`, WN_OK or a negative WN_ERR_* code, all checks
 * before any launch, no atomics, one summation order).  wavenet/mol.py states
 * the rule in numpy (levels_reference, sample_reference, loss_reference);
 * tests/mol_ref.py restates it independently in float64.
 *
 * ---- levels.  C = 65536 levels, every line ONE rounded float32 operation:
 *   y  = fminf(fmaxf(y, -1), 1)            (a NaN sample reads as -1)
 *   t  = y + 1
 *   t  = t * 32767.5                       ((C - 1) / 2, exact)
 *   j  = rintf(t)                          (ties to even), 0 <= j <= C - 1
 *   c  = (float)(2 j - 65535) / 65535      (exact integer, one division)
 * c(0) = -1 and c(C - 1) = 1 exactly, c(C - 1 - j) = -c(j).  The network reads
 * c(j[t]) and the target of row t is j[t + 1]: training and generation see the
 * same grid.
 *
 * ---- head.  K components, Kp = K rounded up to a multiple of 4; a row of
 * logits is [pi | mu | beta_raw], each block Kp floats (3 Kp <= 96).  Columns
 * k >= K of each block are not read and get gradient exactly 0.
 *
 * ---- row loss, target level j.  The logits are float32; everything below is
 * float64, no fused multiply-add, and each output is rounded to float32 once:
 * a component e^-14 wide next to a bin of 2 / 65535 puts terms twelve orders
 * of magnitude apart into one sum, and a float32 chain of the dozen operations
 * behind a gradient entry loses four to seven ulps.  c = (2 j - 65535) / 65535
 * (the exact centre's nearest double: the bins tile [-1 - h, 1 + h]), h = 1 /
 * 65535, h2 = 2 / 65535, log2h = log(h2).  Per component k < K:
 *   beta = fmaxf(beta_raw, log_scale_min)
 *   is   = exp(-beta)
 *   d    = c - mu
 *   a    = (d + h) * is
 *   b    = (d - h) * is
 *   D    = h2 * is                          (= a - b without the cancellation)
 *   ea   = exp(-|a|)         eb = exp(-|b|)
 *   spa  = fmax(-a, 0) + log1p(ea)          softplus(-a)
 *   spb  = fmax(b, 0) + log1p(eb)           softplus(b)
 *   sna  = a <= 0 ? 1 / (1 + ea) : ea / (1 + ea)        sigmoid(-a)
 *   sb   = b >= 0 ? 1 / (1 + eb) : eb / (1 + eb)        sigmoid(b)
 *   lt   = D >= 1 ? log(-expm1(-D))
 *                 : (log2h - beta) + log(D > 0 ? -expm1(-D) / D : 1)
 *   gt   = D > 0 ? D / expm1(D) : 1
 * lt is log(1 - e^-D) on both branches: below 1 it is split into log D = log2h
 * - beta and the remainder, so that a scale whose e^-beta underflows still has
 * a finite term.  No density approximation and no probability floor anywhere.
 *   interior (0 < j < C - 1):  lp = (-spa - spb) + lt
 *                              dmu = is * (sb - sna)
 *                              dbeta = (b * sb - a * sna) - gt
 *   j == 0:                    lp = -spa,  dmu = -(is * sna),  dbeta = -(a * sna)
 *   j == C - 1:                lp = -spb,  dmu = is * sb,      dbeta = b * sb
 * (dmu, dbeta: the derivatives of lp by mu and by beta.)  The edges are the
 * true outer bins, so sum_j exp(lp(j)) = 1.  Then over k < K, with sums and
 * maxima taken as: component k = 4 i + s belongs to lane s; a lane folds its
 * components i ascending, the four lanes combine as (s0 + s1) + (s2 + s3):
 *   mp  = max pi_k           sp = sum exp(pi_k - mp)
 *   w_k = ((pi_k - mp) - log(sp)) + lp_k
 *   mw  = max w_k            sw = sum exp(w_k - mw)
 *   nll = (float)-(mw + log(sw))
 *   r_k = exp(w_k - mw) / sw                p_k = exp(pi_k - mp) / sp
 *   g_pi = (float)((p_k - r_k) * inv)   g_mu = (float)(-(r_k * dmu) * inv)
 *   g_beta = beta_raw < log_scale_min ? 0 : (float)(-(r_k * dbeta) * inv)
 * inv: float32 1 / (B T), or *inv_den.  Every output is finite for finite
 * logits while the gradient itself fits float32.  The loss partials add the
 * float32 nll of the rows in float64 and are rounded once.
 *
 * ---- which rows.  n[b] = lengths ? min(max(lengths[b], 0), T) : T, s[b] =
 * starts ? min(max(starts[b], 0), T) : 0.  Row (b, t) has the target
 * levels[b][t + 1] iff s[b] <= t + 1 < n[b] and that level lies in [0, C - 1];
 * every other row adds nothing to the loss and its 3 Kp gradient columns are
 * exactly 0.  A row's nll and gradient bits are a function of its own logits,
 * its target, K, log_scale_min and inv: not of B, T or where it lies.
 *
 * ---- wn_mol_params_row: out[0][k] = (float)((pi_k - m) - log(sum_k exp(pi_k -
 * m))) in float64, m the maximum and the sum taken k ascending; out[1][k] =
 * mu_k; out[2][k] = fmaxf(beta_raw_k, log_scale_min).
 *
 * ---- wn_mol_sample, row r, float64 throughout:
 *   u1 = draw_uniform(seeds[r], 2 counters[r])        (csrc/wn_common.h)
 *   u2 = draw_uniform(seeds[r], 2 counters[r] + 1)
 *   p_k = exp(params[r][0][k]); total = sum p_k, k ascending
 *   k  = the first k with u1 * total < p_0 + ... + p_k (else the last p_k > 0)
 *   x  = mu_k                                         temperature == 0
 *   x  = mu_k + (exp(beta_k) * temperature) * (log(u2) - log(1 - u2))
 *   x  = fmin(fmax(x, -1), 1)                         (u2 = 0 gives -1)
 *   j  = rint((x + 1) * 32767.5); levels_out[r] = j, centres_out[r] = c(j)
 */
#ifndef WAVENET_MOL_H_
#define WAVENET_MOL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* audio: device float [B][T]; lengths: device int32 [B] or NULL; levels_out:
 * device int32 [B][T]; centres_out: device float [B][T].  Samples at or behind
 * n[b] are not read: level 0 and centre +0 come out.  centres_out may be
 * audio.  B, T >= 1, B T < 2^31, else WN_ERR_BAD_SHAPE; 4-byte alignment.
 * One launch. */
int wn_mol_quantize(const float* audio, const int32_t* lengths,
                    int32_t* levels_out, float* centres_out, int B, int T,
                    void* stream);

/* logits: device float, row i at + i * ld, 3 Kp columns read; levels: device
 * int32 [B][T]; starts, lengths: device int32 [B] or NULL; inv_den: device
 * float [1] or NULL (then 1 / (B T)); dlogits: NULL (forward only), logits (in
 * place) or another buffer of the same ld that does not overlap it;
 * loss_partials: device float [wn_xent_partials(B T)], every one written,
 * their sum the sum of nll over the rows with a target.  1 <= K <= 32, -32 <=
 * log_scale_min <= -1, ld >= 3 Kp and ld % 4 == 0 (else WN_ERR_UNSUPPORTED),
 * logits / dlogits 16-byte aligned.  One launch. */
int wn_mol_loss(const float* logits, long ld, const int32_t* levels,
                const int32_t* starts, const int32_t* lengths,
                const float* inv_den, float* dlogits, float* loss_partials,
                int B, int T, int K, float log_scale_min, void* stream);

/* Host only: the floats of wn_mol_score's scratch. */
long wn_mol_score_scratch_floats(long rows);

/* The rows' nll by wn_mol_loss's row arithmetic, bit for bit.  row_nll: device
 * float [B][T] or NULL, 0 where a row has no target; clip_nll: device double
 * [B], clip b's rows summed in float64 in one fixed order; clip_count: device
 * int32 [B], its rows with a target.  Two launches. */
int wn_mol_score(const float* logits, long ld, const int32_t* levels,
                 const int32_t* starts, const int32_t* lengths, float* row_nll,
                 double* clip_nll, int32_t* clip_count, float* scratch, int B,
                 int T, int K, float log_scale_min, void* stream);

/* logits_row: device float [3 Kp]; out: device float [3][K].  One launch. */
int wn_mol_params_row(const float* logits_row, int K, float log_scale_min,
                      float* out, void* stream);

/* params: device float [R][3][K] as wn_mol_params_row writes them; seeds,
 * counters: device uint64 [R]; levels_out: device int32 [R]; centres_out:
 * device float [R].  temperature >= 0 and finite, 1 <= R < 2^31.  One launch,
 * a lane per row. */
int wn_mol_sample(const float* params, const uint64_t* seeds,
                  const uint64_t* counters, float temperature,
                  int32_t* levels_out, float* centres_out, int R, int K,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* WAVENET_MOL_H_ */
