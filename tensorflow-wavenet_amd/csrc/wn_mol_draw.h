// The mixture-of-logistics head's two row rules, stated once for the kernels
// that apply them (include/wavenet_mol.h has them in words): wn_mol_params_row
// and wn_mol_sample (wn_mol.hip) and the batched generator's mixture draw
// (wn_fastgen_mol.hip).  float64, no fused multiply-add, whatever the file
// that includes this sets.
#pragma once
#include "wn_common.h"
#include <cmath>

#define MOL_TOP 65535        // C - 1, the highest level
#define MOL_MAXK 32

__device__ __forceinline__ float mol_centre(int j) {
  return (float)(2 * j - MOL_TOP) / 65535.0f;
}

// component k of a row's parameters: out[0][k] = log_softmax(pi)[k] (the
// maximum and the sum taken over the K components ascending), out[1][k] =
// mu_k, out[2][k] = the clamped beta_k.  row: [3 Kp] logits, out: [3][K].
__device__ __forceinline__ void mol_params_component(const float* row, int K,
                                                     float lsm, int k,
                                                     float* out) {
#pragma clang fp contract(off)
  const int Kp = (K + 3) & ~3;
  double m = -INFINITY;
  for (int i = 0; i < K; ++i) m = fmax(m, (double)row[i]);
  double se = 0.0;
  for (int i = 0; i < K; ++i) se += exp((double)row[i] - m);
  out[k] = (float)(((double)row[k] - m) - log(se));
  out[K + k] = row[Kp + k];
  out[2 * K + k] = fmaxf(row[2 * Kp + k], lsm);
}

// the draw from one row's parameters p [3][K] -> the level
__device__ __forceinline__ int mol_draw_level(const float* p, int K,
                                              uint64_t seed, uint64_t ctr,
                                              float temperature) {
#pragma clang fp contract(off)
  const double u1 = draw_uniform(seed, 2 * ctr);
  const double u2 = draw_uniform(seed, 2 * ctr + 1);
  double total = 0.0;
  for (int k = 0; k < K; ++k) total += exp((double)p[k]);
  const double t = u1 * total;
  double cum = 0.0;
  int pick = -1, last = 0;
  for (int k = 0; k < K; ++k) {
    const double pk = exp((double)p[k]);
    cum += pk;
    if (pk > 0.0) last = k;
    if (pick < 0 && t < cum) pick = k;
  }
  if (pick < 0) pick = last;
  double x = (double)p[K + pick];
  if (temperature != 0.f) {
    const double sc = exp((double)p[2 * K + pick]) * (double)temperature;
    const double lg = log(u2) - log(1.0 - u2);
    x = x + sc * lg;
  }
  x = fmin(fmax(x, -1.0), 1.0);
  double q = x + 1.0;
  q = q * 32767.5;
  return (int)rint(q);
}
