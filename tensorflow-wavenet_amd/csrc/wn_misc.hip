// Streaming (HBM-bound) kernels around the MFMA core: mu-law companding, the
// one-hot "conv" of the causal layer as a 2-row gather, fused softmax
// cross-entropy, optimizers with TensorFlow update rules, global-conditioning
// helpers, and the thin exported ops (causal_conv, time_to_batch, ...).
#include "wn_common.h"
#include <stdlib.h>
#include <cmath>

// ---------------------------------------------------------------------------
// mu-law  (wavenet/ops.py:65-85)
//
// Bit-exactness: ops.py:65-73 is a float32 chain whose only non-IEEE-exact
// step is log().  The chain is DEFINED here with the correctly rounded
// float32 log (double log rounded once).  encode() is a monotone step
// function of x on [-1,1], so the device encodes by binary search over the
// Q-1 float32 decision thresholds of that chain (built once on the host by
// wn_mu_law_thresholds_host) -- exact by construction, independent of the
// device's logf.  |x| > 1 (outside the table) evaluates the chain itself.
// ---------------------------------------------------------------------------
#pragma clang fp contract(off)
static inline int mu_chain_host(float x, int Q) {
  const float mu = (float)(Q - 1);
  const float ax = std::fabs(x);
  const float arg = 1.0f + mu * ax;
  const float num = (float)std::log((double)arg);
  const float den = (float)std::log((double)(1.0f + mu));
  const float mag = num / den;
  const float sgn = (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f);
  float v = sgn * mag;
  v = v + 1.0f;
  v = v / 2.0f;
  v = v * mu;
  v = v + 0.5f;
  return (int)v;
}

static inline uint32_t f2key(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static inline float key2f(uint32_t k) {
  uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

__device__ __forceinline__ int mu_chain_dev(float x, int Q) {
  // same chain on the device for |x| > 1; double log keeps it within the
  // definition above (OCML double log, rounded once to float).
  const float mu = (float)(Q - 1);
  const float arg = __fadd_rn(1.0f, __fmul_rn(mu, fabsf(x)));
  const float num = (float)log((double)arg);
  const float den = (float)log((double)__fadd_rn(1.0f, mu));
  const float mag = __fdiv_rn(num, den);
  const float sgn = (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f);
  float v = __fmul_rn(sgn, mag);
  v = __fadd_rn(v, 1.0f);
  v = __fdiv_rn(v, 2.0f);
  v = __fmul_rn(v, mu);
  v = __fadd_rn(v, 0.5f);
  return (int)v;
}

__global__ void mu_law_encode_kernel(const float* __restrict__ audio,
                                     int32_t* __restrict__ codes, long n,
                                     const float* __restrict__ thr, int Q) {
  extern __shared__ float sthr[];
  for (int i = threadIdx.x; i < Q - 1; i += blockDim.x) sthr[i] = thr[i];
  __syncthreads();
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n;
       idx += (long)gridDim.x * blockDim.x) {
    const float x = audio[idx];
    int code;
    if (x >= -1.f && x <= 1.f) {
      int lo = 0, hi = Q - 1;  // count of thresholds <= x  (upper bound)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sthr[mid] <= x) lo = mid + 1; else hi = mid;
      }
      code = lo;
    } else {
      code = mu_chain_dev(x, Q);
    }
    codes[idx] = code;
  }
}

__device__ __forceinline__ float mu_decode_dev(int code, int Q) {
  const float mu = (float)(Q - 1);
  const float s = __fsub_rn(__fmul_rn(2.0f, __fdiv_rn((float)code, mu)), 1.0f);
  const float p = (float)pow((double)__fadd_rn(1.0f, mu), (double)fabsf(s));
  const float mag = __fmul_rn(__fdiv_rn(1.0f, mu), __fsub_rn(p, 1.0f));
  const float sgn = (s > 0.f) ? 1.f : ((s < 0.f) ? -1.f : 0.f);
  return __fmul_rn(sgn, mag);
}

__global__ void mu_law_decode_kernel(const int32_t* __restrict__ codes,
                                     float* __restrict__ audio, long n,
                                     const float* __restrict__ lut, int Q) {
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n;
       idx += (long)gridDim.x * blockDim.x) {
    const int c = codes[idx];
    audio[idx] = (c >= 0 && c < Q) ? lut[c] : mu_decode_dev(c, Q);
  }
}

// ---------------------------------------------------------------------------
// causal layer on one-hot input == gather   (model.py:227-234, 518-531)
//   x0[t] = sum_k Wc[k][q[t - s_k]],  s_k = (K-1-k) + (K-1)/2
//   (K = filter_width; K = 2: Wc[0][q[t-1]] + Wc[1][q[t]]; terms with t < s_k
//   vanish; an out-of-range code is an all-zero one-hot row)
// Wc: [K][Q][32] (R padded to 32).  8 threads x 16 B per row.
// ---------------------------------------------------------------------------
__global__ void causal_gather_kernel(const int32_t* __restrict__ q,
                                     const float* __restrict__ Wc,
                                     float* __restrict__ x0, long rows, int T,
                                     int Q, int K, int ldw) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long row = idx >> 3;
  const int c4 = (idx & 7) * 4;
  if (row >= rows) return;
  const int t = (int)(row % T);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const int extra = (K - 1) / 2;       // TF 'SAME' centring for K > 2
  for (int k = 0; k < K; ++k) {
    const int s = (K - 1 - k) + extra;
    if (t < s) continue;
    const int code = q[row - s];
    if (code >= 0 && code < Q)
      v += *reinterpret_cast<const f32x4*>(Wc + ((long)k * Q + code) * ldw + c4);
  }
  *reinterpret_cast<f32x4*>(x0 + row * 32 + c4) = v;
}

// ---------------------------------------------------------------------------
// causal layer on scalar input (scalar_input=True, model.py:143-153, 646-648):
//   x0[t][c] = sum_k audio[t - s_k] * W[k][0][c],  s_k = (K0-1-k) + (K0-1)/2
// (dilation 1; the extra (K0-1)/2 delay is TF's 'SAME' centring inside
// causal_conv for K0 > 2, ops.py:46-62).  W: [K0][32].
// ---------------------------------------------------------------------------
__global__ void scalar_causal_fwd_kernel(const float* __restrict__ audio,
                                         const float* __restrict__ W,
                                         float* __restrict__ x0, long rows,
                                         int T, int K0, int ldw) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long row = idx >> 3;
  const int c4 = (idx & 7) * 4;
  if (row >= rows) return;
  const int t = (int)(row % T);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const int extra = (K0 - 1) / 2;
  for (int k = 0; k < K0; ++k) {
    const int s = (K0 - 1 - k) + extra;
    if (t - s < 0) continue;
    const float a = audio[row - s];
    const f32x4 w = *reinterpret_cast<const f32x4*>(W + (long)k * ldw + c4);
    v += a * w;
  }
  *reinterpret_cast<f32x4*>(x0 + row * 32 + c4) = v;
}

// dW[k][c] = sum_rows audio[row - s_k] * dx0[row][c] into slabs [splits][K0*32]
__global__ __launch_bounds__(1024) void scalar_causal_wgrad_kernel(
    const float* __restrict__ audio, const float* __restrict__ dx0,
    float* __restrict__ slabs, long rows, long rows_per_split, int T, int K0) {
  const int c = threadIdx.x & 31;
  const long r0 = (long)blockIdx.x * rows_per_split;
  long r1 = r0 + rows_per_split;
  if (r1 > rows) r1 = rows;
  // thread (k, c): taps k, k + 32, ... (initial_filter_width > 32: one pass
  // over the rows per 32 taps)
  for (int k = threadIdx.x >> 5; k < K0; k += 32) {
    const int s = (K0 - 1 - k) + (K0 - 1) / 2;
    float acc = 0.f;
    int t = (int)(r0 % T);
    for (long r = r0; r < r1; ++r) {
      if (t >= s) acc = fmaf(audio[r - s], dx0[r * 32 + c], acc);
      if (++t == T) t = 0;
    }
    slabs[(long)blockIdx.x * K0 * 32 + k * 32 + c] = acc;
  }
}

// ---------------------------------------------------------------------------
// fused softmax cross-entropy, forward + backward   (model.py:654-666)
// One wave per row.  target of row (b,t) = q[b][t+1]; the last row of every
// clip has the all-zero label row the reference pads in (model.py:659): its
// loss term is 0 but it stays in the mean's denominator, and with
// tf_quirk != 0 it back-propagates softmax/(B*T) like TF's fused kernel
// (backprop = softmax - labels).
//
// MASKED (wn_xent_masked): clip b has lengths[b] real samples and right
// padding after them, and is treated as a clip of T = lengths[b] fed alone:
// row lengths[b] - 1 is its label-less last row, rows t >= lengths[b] add
// nothing to the loss and get an all-zero dlogits row without an exponential
// being evaluated.  1 / denominator arrives in inv_n like 1 / (B*T) does.
// One body for both kernels: lengths[b] = T takes exactly the unmasked
// arithmetic, so the two agree bit for bit there.
// ---------------------------------------------------------------------------
// row -> its clip's length (T when nothing is masked)
template <bool MASKED>
__device__ __forceinline__ int xent_len(long row, int T,
                                        const int32_t* lengths) {
  return MASKED ? min(max(lengths[row / T], 0), T) : T;
}

template <bool MASKED>
__device__ __forceinline__ void xent_body(
    const float* __restrict__ logits, long ld, const int32_t* __restrict__ q,
    const int32_t* __restrict__ lengths, float* __restrict__ dlogits,
    float* __restrict__ loss_partials, long rows, int T, int Q, float inv_n,
    int tf_quirk) {
  __shared__ float wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float lsum = 0.f;
  const long nwaves = (long)gridDim.x * 4;
  if (Q == 256) {
    // one 16-byte load per lane holds the whole row: a single pass, each exp
    // evaluated once, the next row's load in flight under the reductions
    long row = (long)blockIdx.x * 4 + wave;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < rows) v = *reinterpret_cast<const f32x4*>(logits + row * ld + lane * 4);
    for (; row < rows; row += nwaves) {
      const long nrow = row + nwaves;
      f32x4 vn = {0.f, 0.f, 0.f, 0.f};
      if (nrow < rows)
        vn = *reinterpret_cast<const f32x4*>(logits + nrow * ld + lane * 4);
      const int t = (int)(row % T);
      const int len = xent_len<MASKED>(row, T, lengths);
      if (MASKED && t >= len) {              // padding
        if (dlogits)
          *reinterpret_cast<f32x4*>(dlogits + row * ld + lane * 4) =
              f32x4{0.f, 0.f, 0.f, 0.f};
        v = vn;
        continue;
      }
      const int label = (t + 1 < len) ? q[row + 1] : -1;
      const bool has_label = label >= 0 && label < Q;
      float m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      float e[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) e[k] = expf(v[k] - m);
      float se = (e[0] + e[1]) + (e[2] + e[3]);
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) se += __shfl_xor(se, o);
      const float lse = m + logf(se);
      if (has_label) {
        // the label's logit lives in lane label >> 2
        const float mine = (label >> 2) == lane ? v[label & 3] : 0.f;
        float ll = mine;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ll += __shfl_xor(ll, o);
        if (lane == 0) lsum += lse - ll;
      }
      if (dlogits) {
        const float inv_se = 1.f / se;
        const bool back = has_label || tf_quirk;
        f32x4 g;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float p = back ? e[k] * inv_se : 0.f;
          if (has_label && lane * 4 + k == label) p -= 1.f;
          g[k] = p * inv_n;
        }
        *reinterpret_cast<f32x4*>(dlogits + row * ld + lane * 4) = g;
      }
      v = vn;
    }
  } else
  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += nwaves) {
    const float* lp = logits + row * ld;
    const int t = (int)(row % T);
    const int len = xent_len<MASKED>(row, T, lengths);
    if (MASKED && t >= len) {                // padding
      if (dlogits)
        for (int c = lane * 4; c < Q; c += 256)
          *reinterpret_cast<f32x4*>(dlogits + row * ld + c) =
              f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    const int label = (t + 1 < len) ? q[row + 1] : -1;
    const bool has_label = label >= 0 && label < Q;
    float m = -INFINITY;
    for (int c = lane * 4; c < Q; c += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(lp + c);
      m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float se = 0.f;
    for (int c = lane * 4; c < Q; c += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(lp + c);
      se += expf(v[0] - m) + expf(v[1] - m) + expf(v[2] - m) + expf(v[3] - m);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) se += __shfl_xor(se, o);
    const float lse = m + logf(se);
    if (has_label && lane == 0) lsum += lse - lp[label];
    const float inv_se = 1.f / se;
    const bool back = has_label || tf_quirk;
    if (dlogits) {
      float* dp = dlogits + row * ld;
      for (int c = lane * 4; c < Q; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(lp + c);
        f32x4 g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float p = back ? expf(v[e] - m) * inv_se : 0.f;
          if (has_label && c + e == label) p -= 1.f;
          g[e] = p * inv_n;
        }
        *reinterpret_cast<f32x4*>(dp + c) = g;
      }
    }
  }
  if (lane == 0) wsum[wave] = lsum;
  __syncthreads();
  if (threadIdx.x == 0)
    loss_partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(256) void xent_kernel(
    const float* __restrict__ logits, long ld, const int32_t* __restrict__ q,
    float* __restrict__ dlogits, float* __restrict__ loss_partials, long rows,
    int T, int Q, float inv_n, int tf_quirk) {
  xent_body<false>(logits, ld, q, nullptr, dlogits, loss_partials, rows, T, Q,
                   inv_n, tf_quirk);
}

// lengths [B] and 1 / denominator are read from device memory: a recorded
// launch replays with this call's values
__global__ __launch_bounds__(256) void xent_masked_kernel(
    const float* __restrict__ logits, long ld, const int32_t* __restrict__ q,
    const int32_t* __restrict__ lengths, const float* __restrict__ inv_den,
    float* __restrict__ dlogits, float* __restrict__ loss_partials, long rows,
    int T, int Q, int tf_quirk) {
  xent_body<true>(logits, ld, q, lengths, dlogits, loss_partials, rows, T, Q,
                  *inv_den, tf_quirk);
}

// ---------------------------------------------------------------------------
// scoring (wn_xent_score): per-row negative log-likelihood, per-clip sums,
// target counts and arg-max hits of held-out data.  Forward only.
//
// xent_score_rows_kernel: one wave per row, xent_body's float32 formulas
// (max, expf, sum, m + logf(se), the same shuffle trees) on the rows that
// have a target -- t + 1 < len_b and 0 <= q[b][t + 1] < Q -- and nothing but
// a stored 0 for the others (the label-less last row, a code out of range,
// padding): no exponential is evaluated there.  It writes nll[row] and
// flag[row] = 0 (no target) | 1 (target) | 3 (target, and the lowest index of
// the row's maximum over [0, Q) is the target; never for a row whose
// logsumexp is NaN).  Columns >= Q are not read.
// xent_score_clips_kernel: one workgroup per clip.  Thread i sums rows i,
// i + 1024, ... below len_b - 1 in float64 (integers for the flags), a fixed
// LDS tree finishes: a function of the rows' values and len_b alone, whatever
// order the workgroups of either kernel ran in.  No atomics.
// ---------------------------------------------------------------------------
#define SCORE_CLIP_THREADS 1024

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(256) void xent_score_rows_kernel(
    const float* __restrict__ logits, long ld, const int32_t* __restrict__ q,
    const int32_t* __restrict__ lengths, float* __restrict__ nll,
    int32_t* __restrict__ flag, long rows, int T, int Q) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long nwaves = (long)gridDim.x * 4;
  const int none = 0x7fffffff;
  if (Q == 256) {
    // xent_body's single pass: one 16-byte load per lane holds the row, the
    // next row's load in flight under the reductions
    long row = (long)blockIdx.x * 4 + wave;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < rows) v = *reinterpret_cast<const f32x4*>(logits + row * ld + lane * 4);
    for (; row < rows; row += nwaves) {
      const long nrow = row + nwaves;
      f32x4 vn = {0.f, 0.f, 0.f, 0.f};
      if (nrow < rows)
        vn = *reinterpret_cast<const f32x4*>(logits + nrow * ld + lane * 4);
      const int t = (int)(row % T);
      const int len = lengths ? min(max(lengths[row / T], 0), T) : T;
      const int label = (t + 1 < len) ? q[row + 1] : -1;
      if (!(label >= 0 && label < Q)) {      // no target: nothing to evaluate
        if (lane == 0) {
          nll[row] = 0.f;
          flag[row] = 0;
        }
        v = vn;
        continue;
      }
      float m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      float e[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) e[k] = expf(v[k] - m);
      float se = (e[0] + e[1]) + (e[2] + e[3]);
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) se += __shfl_xor(se, o);
      const float lse = m + logf(se);
      const float mine = (label >> 2) == lane ? v[label & 3] : 0.f;
      float ll = mine;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) ll += __shfl_xor(ll, o);
      int best = none;                       // lowest index holding the maximum
#pragma unroll
      for (int k = 3; k >= 0; --k) best = v[k] == m ? lane * 4 + k : best;
      best = wave_min_i32(best);
      if (lane == 0) {
        nll[row] = lse - ll;
        flag[row] = (best == label && lse == lse) ? 3 : 1;
      }
      v = vn;
    }
    return;
  }
  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += nwaves) {
    const float* lp = logits + row * ld;
    const int t = (int)(row % T);
    const int len = lengths ? min(max(lengths[row / T], 0), T) : T;
    const int label = (t + 1 < len) ? q[row + 1] : -1;
    if (!(label >= 0 && label < Q)) {
      if (lane == 0) {
        nll[row] = 0.f;
        flag[row] = 0;
      }
      continue;
    }
    float m = -INFINITY;
    for (int c = lane * 4; c < Q; c += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(lp + c);
      m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float se = 0.f;
    int best = none;
    for (int c = lane * 4; c < Q; c += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(lp + c);
      se += expf(v[0] - m) + expf(v[1] - m) + expf(v[2] - m) + expf(v[3] - m);
#pragma unroll
      for (int k = 3; k >= 0; --k) best = v[k] == m ? min(best, c + k) : best;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) se += __shfl_xor(se, o);
    best = wave_min_i32(best);
    const float lse = m + logf(se);
    if (lane == 0) {
      nll[row] = lse - lp[label];
      flag[row] = (best == label && lse == lse) ? 3 : 1;
    }
  }
}

__global__ __launch_bounds__(SCORE_CLIP_THREADS) void xent_score_clips_kernel(
    const float* __restrict__ nll, const int32_t* __restrict__ flag,
    const int32_t* __restrict__ lengths, double* __restrict__ clip_nll,
    int32_t* __restrict__ clip_count, int32_t* __restrict__ clip_correct,
    int T) {
  __shared__ double rs[SCORE_CLIP_THREADS];
  __shared__ int rc[SCORE_CLIP_THREADS], rh[SCORE_CLIP_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = lengths ? min(max(lengths[b], 0), T) : T;
  const float* pn = nll + (long)b * T;
  const int32_t* pf = flag + (long)b * T;
  double s = 0.0;
  int c = 0, h = 0;
  // (rows t >= len - 1 have no target: zeros by construction, not read)
  for (int t = tid; t < len - 1; t += SCORE_CLIP_THREADS) {
    const int f = pf[t];
    s += (double)pn[t];
    c += f & 1;
    h += f >> 1;
  }
  rs[tid] = s;
  rc[tid] = c;
  rh[tid] = h;
  __syncthreads();
  for (int k = SCORE_CLIP_THREADS / 2; k > 0; k >>= 1) {
    if (tid < k) {
      rs[tid] += rs[tid + k];
      rc[tid] += rc[tid + k];
      rh[tid] += rh[tid + k];
    }
    __syncthreads();
  }
  if (tid == 0) {
    clip_nll[b] = rs[0];
    clip_count[b] = rc[0];
    clip_correct[b] = rh[0];
  }
}

// softmax of ONE row in float64, cast to float32 (model.py:584-585, 620-621)
__global__ void softmax64_row_kernel(const float* __restrict__ logits, int Q,
                                     float* __restrict__ proba) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double m = -INFINITY;
  for (int c = tid; c < Q; c += 256) m = fmax(m, (double)logits[c]);
  red[tid] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
    __syncthreads();
  }
  m = red[0];
  __syncthreads();
  double se = 0.0;
  for (int c = tid; c < Q; c += 256) se += exp((double)logits[c] - m);
  red[tid] = se;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  se = red[0];
  for (int c = tid; c < Q; c += 256)
    proba[c] = (float)(exp((double)logits[c] - m) / se);
}

// ---------------------------------------------------------------------------
// optimizers, TensorFlow-0.10 update rules (wavenet/ops.py:6-24)
//   g' = g * grad_scale + l2 * p * (l2_mask ? l2_mask[i] : 1)
// ---------------------------------------------------------------------------
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v,
                            long n, float lr_t, float b1, float b2, float eps,
                            float grad_scale, float l2,
                            const float* __restrict__ l2_mask) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const float w = p[i];
    float gg = g[i] * grad_scale;
    if (l2 != 0.f) gg += l2 * w * (l2_mask ? l2_mask[i] : 1.f);
    const float mm = b1 * m[i] + (1.f - b1) * gg;
    const float vv = b2 * v[i] + (1.f - b2) * gg * gg;
    m[i] = mm;
    v[i] = vv;
    p[i] = w - lr_t * mm / (sqrtf(vv) + eps);
  }
}

__global__ void momentum_kernel(float* __restrict__ p,
                                const float* __restrict__ g,
                                float* __restrict__ acc, long n, float lr,
                                float mom, float grad_scale, float l2,
                                const float* __restrict__ l2_mask) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const float w = p[i];
    float gg = g[i] * grad_scale;
    if (l2 != 0.f) gg += l2 * w * (l2_mask ? l2_mask[i] : 1.f);
    const float a = mom * acc[i] + gg;
    acc[i] = a;
    p[i] = w - lr * a;
  }
}

__global__ void rmsprop_kernel(float* __restrict__ p,
                               const float* __restrict__ g,
                               float* __restrict__ ms, float* __restrict__ mo,
                               long n, float lr, float decay, float mom,
                               float eps, float grad_scale, float l2,
                               const float* __restrict__ l2_mask) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const float w = p[i];
    float gg = g[i] * grad_scale;
    if (l2 != 0.f) gg += l2 * w * (l2_mask ? l2_mask[i] : 1.f);
    const float s = decay * ms[i] + (1.f - decay) * gg * gg;
    const float mm = mom * mo[i] + lr * gg / sqrtf(s + eps);
    ms[i] = s;
    mo[i] = mm;
    p[i] = w - mm;
  }
}

// sum of squares / 2 (tf.nn.l2_loss) partials, with optional mask
__global__ void l2_partials_kernel(const float* __restrict__ p, long n,
                                   const float* __restrict__ mask,
                                   float* __restrict__ partials) {
  __shared__ float red[256];
  float s = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const float w = p[i];
    s += w * w * (mask ? mask[i] : 1.f);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (unsigned k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = 0.5f * red[0];
}

// ---------------------------------------------------------------------------
// global-norm clipping (tf.clip_by_global_norm) and EMA weights
// (tf.train.ExponentialMovingAverage) inside the optimizer launches.
//
// grad_norm_partials_kernel: GNORM_PARTS float64 sums of g[i]^2.  Partial k
// covers elements [k * per, min(n, (k + 1) * per)), per = the multiple of 4
// next above n / GNORM_PARTS; inside it thread t takes the 16-byte groups
// t, t + 1024, ... in order, a wave is summed by a shuffle tree and the 16
// wave sums in order.  Grid, block and ranges depend on (n, GNORM_PARTS) only:
// the bits are a function of the bucket and n, not of the device.
//
// The *_clip kernels are the kernels above, element for element, behind a
// prologue in which EVERY workgroup sums the same partials in the same order
// (float64), forms  norm = grad_scale * sqrt(sum)  and
// factor = clip_norm / max(norm, clip_norm)  (NaN for a non-finite norm, as
// TensorFlow) and scales by  grad_scale * (float)factor  -- grad_scale itself
// when norm <= clip_norm, so the update is then the plain kernel's bit for bit
// -- and an epilogue  s -= (1 - decay) * (s - p_new)  on the shadow weights.
// ---------------------------------------------------------------------------
#define GNORM_PARTS 256
#define GNORM_THREADS 1024

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
  return v;  // lane 0: the wave's sum
}

__global__ __launch_bounds__(GNORM_THREADS) void grad_norm_partials_kernel(
    const float* __restrict__ g, long n, long per,
    double* __restrict__ partials) {
  __shared__ double red[GNORM_THREADS / 64];
  const long lo = (long)blockIdx.x * per;
  const long hi = lo + per < n ? lo + per : n;
  double s = 0.0;
  for (long i = lo + 4L * threadIdx.x; i < hi; i += 4L * GNORM_THREADS) {
    if (i + 4 <= hi) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) s += (double)v[e] * (double)v[e];
    } else {
      for (long j = i; j < hi; ++j) s += (double)g[j] * (double)g[j];
    }
  }
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < GNORM_THREADS / 64; ++w) t += red[w];
    partials[blockIdx.x] = t;
  }
}

// the effective gradient scale of a *_clip kernel (256 threads, all of them
// call it); partials == nullptr: grad_scale
__device__ __forceinline__ float clip_scale(const double* __restrict__ partials,
                                            float clip_norm, float grad_scale,
                                            float* __restrict__ norm_out) {
  if (!partials) return grad_scale;
  __shared__ double red[4];
  const double s = wave_sum_f64(partials[threadIdx.x]);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const double sum = ((red[0] + red[1]) + red[2]) + red[3];
  const double norm = (double)grad_scale * sqrt(sum);
  const double cn = (double)clip_norm;
  const double factor = isfinite(norm) ? cn / (norm > cn ? norm : cn)
                                       : (double)NAN;
  if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = (float)norm;
  return grad_scale * (float)factor;
}

__global__ __launch_bounds__(256) void adam_clip_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, long n, float lr_t, float b1, float b2, float eps,
    float grad_scale, float l2, const float* __restrict__ l2_mask,
    const double* __restrict__ partials, float clip_norm,
    float* __restrict__ ema, float ema_decay, float* __restrict__ norm_out) {
  const float scale = clip_scale(partials, clip_norm, grad_scale, norm_out);
  const float keep = 1.f - ema_decay;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const float w = p[i];
    float gg = g[i] * scale;
    if (l2 != 0.f) gg += l2 * w * (l2_mask ? l2_mask[i] : 1.f);
    const float mm = b1 * m[i] + (1.f - b1) * gg;
    const float vv = b2 * v[i] + (1.f - b2) * gg * gg;
    m[i] = mm;
    v[i] = vv;
    const float pn = w - lr_t * mm / (sqrtf(vv) + eps);
    p[i] = pn;
    if (ema) {
      const float s = ema[i];
      ema[i] = s - keep * (s - pn);
    }
  }
}

__global__ __launch_bounds__(256) void momentum_clip_kernel(
    float* __restrict__ p, const float* __restrict__ g,
    float* __restrict__ acc, long n, float lr, float mom, float grad_scale,
    float l2, const float* __restrict__ l2_mask,
    const double* __restrict__ partials, float clip_norm,
    float* __restrict__ ema, float ema_decay, float* __restrict__ norm_out) {
  const float scale = clip_scale(partials, clip_norm, grad_scale, norm_out);
  const float keep = 1.f - ema_decay;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const float w = p[i];
    float gg = g[i] * scale;
    if (l2 != 0.f) gg += l2 * w * (l2_mask ? l2_mask[i] : 1.f);
    const float a = mom * acc[i] + gg;
    acc[i] = a;
    const float pn = w - lr * a;
    p[i] = pn;
    if (ema) {
      const float s = ema[i];
      ema[i] = s - keep * (s - pn);
    }
  }
}

__global__ __launch_bounds__(256) void rmsprop_clip_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ ms,
    float* __restrict__ mo, long n, float lr, float decay, float mom,
    float eps, float grad_scale, float l2, const float* __restrict__ l2_mask,
    const double* __restrict__ partials, float clip_norm,
    float* __restrict__ ema, float ema_decay, float* __restrict__ norm_out) {
  const float scale = clip_scale(partials, clip_norm, grad_scale, norm_out);
  const float keep = 1.f - ema_decay;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const float w = p[i];
    float gg = g[i] * scale;
    if (l2 != 0.f) gg += l2 * w * (l2_mask ? l2_mask[i] : 1.f);
    const float s = decay * ms[i] + (1.f - decay) * gg * gg;
    const float mm = mom * mo[i] + lr * gg / sqrtf(s + eps);
    ms[i] = s;
    mo[i] = mm;
    const float pn = w - mm;
    p[i] = pn;
    if (ema) {
      const float e = ema[i];
      ema[i] = e - keep * (e - pn);
    }
  }
}

// ---------------------------------------------------------------------------
// global conditioning   (model.py:272-284, 533-562)
// The GC 1x1 conv of a [B,1,G] embedding broadcast over T is a per-(clip,
// layer) bias:  bias_fg[l][b][0:32] = bf_l + emb[id_b] * Wgcf_l, [32:64] gate.
// ---------------------------------------------------------------------------
__global__ void gc_bias_kernel(const float* __restrict__ layer0, long layer_stride,
                               long off_bias, long off_gc, int G,
                               const float* __restrict__ emb, int card,
                               const int32_t* __restrict__ ids,
                               float* __restrict__ out, int B, int ch) {
  const int l = blockIdx.x, b = blockIdx.y;
  const float* blk = layer0 + (long)l * layer_stride;
  for (int c = threadIdx.x; c < 2 * ch; c += blockDim.x) {
    float v = blk[off_bias + c];  // bf (0..ch-1) then bg (ch..2ch-1)
    if (emb) {
      const int id = ids[b];
      if (id >= 0 && id < card) {
        // Wgcf [G][ch] at off_gc, Wgcg [G][ch] at off_gc + G*ch
        const float* w = blk + off_gc + (c >= ch ? (long)G * ch : 0) + (c % ch);
        const float* e = emb + (long)id * G;
        for (int g = 0; g < G; ++g) v += e[g] * w[(long)g * ch];
      }
    }
    out[((long)l * B + b) * 2 * ch + c] = v;
  }
}

__global__ __launch_bounds__(256) void colsum_clip_kernel(
    const float* __restrict__ P0, const float* __restrict__ P1, int T,
    int rows_per_chunk, float* __restrict__ part) {
  __shared__ float red[8][64];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int c = threadIdx.x & 31, w = threadIdx.x >> 5;
  const int t0 = chunk * rows_per_chunk;
  const int t1 = min(T, t0 + rows_per_chunk);
  const float* p0 = P0 + (long)b * T * 32;
  const float* p1 = P1 + (long)b * T * 32;
  float s0 = 0.f, s1 = 0.f;
  for (int t = t0 + w; t < t1; t += 8) {
    s0 += p0[(long)t * 32 + c];
    s1 += p1[(long)t * 32 + c];
  }
  red[w][c] = s0;
  red[w][32 + c] = s1;
  __syncthreads();
  if (threadIdx.x < 64) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) v += red[k][threadIdx.x];
    part[((long)b * gridDim.x + chunk) * 64 + threadIdx.x] = v;
  }
}

// dWgc_l = emb[ids]^T dsum_l ; demb[id_b] += sum_l dsum_l[b] Wgc_l^T
// dsum: [L][B][64] (f | g).  grid.x = L (+1 block for the embedding rows).
__global__ void gc_grad_kernel(const float* __restrict__ layer0, long layer_stride,
                               long off_gc, int G, const float* __restrict__ emb,
                               int card, const int32_t* __restrict__ ids,
                               const float* __restrict__ dsum, int L, int B,
                               float* __restrict__ glayer0,
                               float* __restrict__ part, int ch) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < L) {
    const int l = blockIdx.x;
    float* gw = glayer0 + (long)l * layer_stride + off_gc;
    for (int e = tid; e < 2 * G * ch; e += blockDim.x) {
      const int which = e / (G * ch), g = (e / ch) % G, c = e % ch;
      float s = 0.f;
      for (int b = 0; b < B; ++b) {
        const int id = ids[b];
        if (id < 0 || id >= card) continue;
        s += emb[(long)id * G + g] * dsum[((long)l * B + b) * 2 * ch + which * ch + c];
      }
      gw[e] = s;
    }
  } else {
    // embedding rows, stage 1 (one workgroup per layer): the layer's share
    // part[l][b][g] = dsum_l[b] . Wgc_l[g] of every clip's embedding gradient
    const int l = blockIdx.x - L;
    const float* w = layer0 + (long)l * layer_stride + off_gc;
    for (int e = tid; e < B * G; e += blockDim.x) {
      const int b = e / G, gi = e - b * G;
      const float* ds = dsum + ((long)l * B + b) * 2 * ch;
      float s = 0.f;
      for (int c = 0; c < ch; ++c)
        s += ds[c] * w[(long)gi * ch + c] + ds[ch + c] * w[(long)(G + gi) * ch + c];
      part[((long)l * B + b) * G + gi] = s;
    }
  }
}

// embedding rows, stage 2 (one workgroup): tmp[b][g] = sum_l part[l][b][g] in
// layer order, then the rows are added clip by clip in a fixed order
// (deterministic when several clips share an id).
__global__ void gc_grad_emb_kernel(const float* __restrict__ part, int L, int B,
                                   int G, int card,
                                   const int32_t* __restrict__ ids,
                                   float* __restrict__ gemb) {
  extern __shared__ float tmp[];      // [B][G]
  const int tid = threadIdx.x;
  for (int e = tid; e < card * G; e += blockDim.x) gemb[e] = 0.f;
  for (int e = tid; e < B * G; e += blockDim.x) {
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += part[(long)l * B * G + e];
    tmp[e] = s;
  }
  __syncthreads();
  for (int gi = tid; gi < G; gi += blockDim.x) {
    for (int b = 0; b < B; ++b) {
      const int id = ids[b];
      if (id < 0 || id >= card) continue;
      gemb[(long)id * G + gi] += tmp[b * G + gi];
    }
  }
}

__global__ void causal_conv_kernel(const float* __restrict__ x,
                                   const float* __restrict__ w,
                                   float* __restrict__ y, int B, int T, int Cin,
                                   int Cout, int K, int d) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * T * Cout;
  if (idx >= total) return;
  const int co = (int)(idx % Cout);
  const long bt = idx / Cout;
  const int t = (int)(bt % T);
  const long b = bt / T;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) {
    // ops.py:46-62 closed form incl. TF 'SAME' centring for K > 2
    const long shift = (long)(K - 1 - k + (K - 1) / 2) * d;
    if (t - shift < 0) continue;
    const float* xr = x + ((b * T) + (t - shift)) * Cin;
    const float* wk = w + (long)k * Cin * Cout + co;
    for (int ci = 0; ci < Cin; ++ci) acc += xr[ci] * wk[(long)ci * Cout];
  }
  y[idx] = acc;
}

// time_to_batch (ops.py:27-34): out[(p*B + b), u, c] = in[b, u*d + p, c] (0 pad)
__global__ void time_to_batch_kernel(const float* __restrict__ in,
                                     float* __restrict__ out, int B, int T,
                                     int C, int d, int U) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * d * U * C;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  long r = idx / C;
  const int u = (int)(r % U);
  r /= U;  // r = p*B + b
  const int b = (int)(r % B), p = (int)(r / B);
  const long t = (long)u * d + p;
  out[idx] = t < T ? in[((long)b * T + t) * C + c] : 0.f;
}

// batch_to_time (ops.py:37-43): out[b, u*d + p, c] = in[(p*B + b), u, c]
__global__ void batch_to_time_kernel(const float* __restrict__ in,
                                     float* __restrict__ out, int B, int U,
                                     int C, int d) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * d * U * C;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  long r = idx / C;
  const int tt = (int)(r % ((long)U * d));
  const int b = (int)(r / ((long)U * d));
  const int u = tt / d, p = tt % d;
  out[idx] = in[(((long)p * B + b) * U + u) * C + c];
}

// y += a * x * (mask ? mask : 1)   (gradient of the L2 term, model.py:674-680)
__global__ void axpy_kernel(float* __restrict__ y, const float* __restrict__ x,
                            float a, const float* __restrict__ mask, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    y[i] += a * x[i] * (mask ? mask[i] : 1.f);
}

__global__ void fill_kernel(float* __restrict__ p, long n, float v) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    p[i] = v;
}

// sum over layers of the skip biases (epilogue bias of the skip GEMM)
__global__ void sum_rows_kernel(const float* __restrict__ in, int rows, int n,
                                float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  // loads of a batch of rows are issued together (the sum itself stays in row
  // order): 50 dependent round trips were 20 us for 100 KB
  float s = 0.f;
  int r = 0;
  for (; r + 16 <= rows; r += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = in[(long)(r + u) * n + c];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += v[u];
  }
  for (; r < rows; ++r) s += in[(long)r * n + c];
  out[c] = s;
}

static inline int grid1d(long n, int block, int cap = 2048) {
  long g = (n + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

extern "C" {

int wn_reduce_slabs(const float* slabs, int num_slabs, long slab_stride,
                    int batch, long in_batch_stride, long offset, long n,
                    float* dst, long out_batch_stride, int replicate,
                    long rep_stride, void* stream);

int wn_version(void) { return 100; }

const char* wn_error_string(int code) {
  switch (code) {
    case WN_OK: return "ok";
    case WN_ERR_BAD_SHAPE: return "bad shape";
    case WN_ERR_UNSUPPORTED: return "unsupported configuration";
    case WN_ERR_MISALIGNED: return "pointer or leading dimension not 16-byte aligned";
    case WN_ERR_LAUNCH: return "kernel launch failed";
    case WN_ERR_NULL: return "null pointer";
    default: return "unknown error";
  }
}

int wn_mu_law_thresholds_host(int Q, float* thr_out) {
  if (!thr_out) return WN_ERR_NULL;
  if (Q < 2) return WN_ERR_BAD_SHAPE;
  const uint32_t lo0 = f2key(-1.0f), hi0 = f2key(1.0f);
  for (int k = 1; k < Q; ++k) {
    uint32_t lo = lo0, hi = hi0;
    if (mu_chain_host(key2f(lo), Q) >= k) { thr_out[k - 1] = key2f(lo); continue; }
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (mu_chain_host(key2f(mid), Q) >= k) hi = mid; else lo = mid;
    }
    thr_out[k - 1] = key2f(hi);
  }
  return WN_OK;
}

int wn_mu_law_decode_table_host(int Q, float* lut_out) {
  if (!lut_out) return WN_ERR_NULL;
  if (Q < 2) return WN_ERR_BAD_SHAPE;
  const float mu = (float)(Q - 1);
  for (int c = 0; c < Q; ++c) {
    float s = (float)c / mu;
    s = 2.0f * s;
    s = s - 1.0f;
    const float p = (float)std::pow((double)(1.0f + mu), (double)std::fabs(s));
    float mag = 1.0f / mu;
    const float pm1 = p - 1.0f;
    mag = mag * pm1;
    const float sgn = (s > 0.f) ? 1.f : ((s < 0.f) ? -1.f : 0.f);
    lut_out[c] = sgn * mag;
  }
  return WN_OK;
}

int wn_mu_law_encode(const float* audio, int32_t* codes, long n,
                     const float* thr_dev, int Q, void* stream) {
  if (!audio || !codes || !thr_dev) return WN_ERR_NULL;
  if (n <= 0 || Q < 2 || Q > 8192) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(mu_law_encode_kernel, dim3(grid1d(n, 256)), dim3(256),
                     (Q - 1) * sizeof(float), (hipStream_t)stream, audio, codes,
                     n, thr_dev, Q);
  return wn_check_launch();
}

int wn_mu_law_decode(const int32_t* codes, float* audio, long n,
                     const float* lut_dev, int Q, void* stream) {
  if (!audio || !codes || !lut_dev) return WN_ERR_NULL;
  if (n <= 0 || Q < 2) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(mu_law_decode_kernel, dim3(grid1d(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, codes, audio, n, lut_dev, Q);
  return wn_check_launch();
}

int wn_causal_gather(const int32_t* q, const float* Wc, float* x0, int B,
                     int T, int Q, int K, int ldw, void* stream) {
  if (!q || !Wc || !x0) return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || Q <= 0 || K <= 0 || ldw < 32 || (ldw & 3))
    return WN_ERR_BAD_SHAPE;
  if (!wn_aligned16(Wc) || !wn_aligned16(x0)) return WN_ERR_MISALIGNED;
  const long rows = (long)B * T;
  const long threads = rows * 8;
  hipLaunchKernelGGL(causal_gather_kernel, dim3((unsigned)((threads + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, q, Wc, x0, rows, T, Q,
                     K, ldw);
  return wn_check_launch();
}

int wn_scalar_causal_fwd(const float* audio, const float* W, int ldw, float* x0,
                         int B, int T, int K0, void* stream) {
  if (!audio || !W || !x0) return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || K0 <= 0 || ldw < 32 || (ldw & 3)) return WN_ERR_BAD_SHAPE;
  if (!wn_aligned16(W) || !wn_aligned16(x0)) return WN_ERR_MISALIGNED;
  const long rows = (long)B * T, threads = rows * 8;
  hipLaunchKernelGGL(scalar_causal_fwd_kernel,
                     dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, audio, W, x0, rows, T, K0, ldw);
  return wn_check_launch();
}

int wn_scalar_causal_wgrad(const float* audio, const float* dx0, float* slabs,
                           int splits, int B, int T, int K0, void* stream) {
  if (!audio || !dx0 || !slabs) return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || K0 <= 0 || splits <= 0) return WN_ERR_BAD_SHAPE;
  const long rows = (long)B * T;
  const long rps = (rows + splits - 1) / splits;
  hipLaunchKernelGGL(scalar_causal_wgrad_kernel, dim3(splits), dim3(1024), 0,
                     (hipStream_t)stream, audio, dx0, slabs, rows, rps, T, K0);
  return wn_check_launch();
}

// ---------------------------------------------------------------------------
// Causal-layer weight gradient for one-hot input, filter width 2
// (model.py:227-234 under autodiff): dWc[tap][v][:] = sum over rows whose code
// q[t - (1 - tap)] == v of dx0[t][:].  It is a segmented sum, not a GEMM: 16 MB
// of dx0 are read once.  Every wave owns a private [2 taps][Q][32] table in
// LDS and walks a contiguous range of rows in program order, which keeps the
// result independent of scheduling; the per-wave tables go out as slabs for
// wn_reduce_slabs.  Replaces two one-hot MFMA contractions (2 x 110 us at
// B*T = 128000).  Round 3: 90 -> 34 us (one wave per SIMD: what bounds it is
// the number of instructions on the row chain, not HBM and not the LDS round
// trip: four rows per LDS round trip took 45 -> 43 us, a deeper load ring
// nothing, the per-row address arithmetic out of the vector unit 42 -> 34).
// ---------------------------------------------------------------------------
#define CWG_QMAX 256
#define CWG_NB 32     // rows per batch
__global__ __launch_bounds__(128) void causal_wgrad_kernel(
    const int32_t* __restrict__ q, const float* __restrict__ dx0,
    float* __restrict__ slabs, long rows, long rows_per_slab, int T, int Q) {
  // per wave: [2 taps][Q + 1][32]; row Q of a tap table is a dump for rows
  // without a code (the first sample of a clip for tap 0, rows past the range)
  __shared__ __attribute__((aligned(16))) float tab[2 * 2 * (CWG_QMAX + 1) * 32];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;        // channel, tap
  const int trows = Q + 1;
  float* wtab = tab + (size_t)wave * 2 * trows * 32;
  {
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    for (int i = lane; i < 2 * trows * 8; i += 64) reinterpret_cast<f32x4*>(wtab)[i] = z4;
  }
  __builtin_amdgcn_wave_barrier();
  const long slab = (long)blockIdx.x * 2 + wave;
  const long r0 = slab * rows_per_slab;
  long r1 = r0 + rows_per_slab;
  if (r1 > rows) r1 = rows;
  // Half-wave h accumulates tap h (tap 0 pairs dx0[t] with the PREVIOUS code),
  // lane c owns channel c: one row per step, 32 consecutive floats of one
  // table row, plain read-add-write in program order (a wave's LDS operations
  // execute in order, so rows that share a code simply chain; LDS float
  // atomics measured ~400 cycles per instruction here, hence none).  Nothing
  // on that chain but the LDS round trip: a batch's 32 rows of dx0 and its
  // codes are requested one batch ahead (one coalesced code load per lane:
  // lane (j, h) holds the table offset of row j for tap h), the 32 table
  // addresses are spread to the lanes before the chain starts, rows without a
  // code go to the dump row instead of around a branch.
  const int shift = 1 - h;
  const int lane_off = (h * trows * 32 + c) * 4;            // bytes inside wtab
  auto fetch_codes = [&](long rb, int tb) -> int {
    const long row = rb + c;                                // this lane's row
    int code = Q;
    if (row < r1) {
      int t = tb + c;                                       // tb: clip position of row rb
      if (t >= T) t %= T;
      if (t - shift >= 0) {
        const int v = q[row - shift];
        if (v >= 0 && v < Q) code = v;
      }
    }
    return code * 128;                                      // byte offset of the table row
  };
  // dx0 rows through a buffer resource based at the slab's first row: the
  // row offset is scalar, the lane's part (c * 4) loop-invariant -- no vector
  // address arithmetic per row (one wave per SIMD: the kernel is bound by the
  // number of instructions it issues).  Rows past the slab re-read its last
  // row (their code is the dump row): the scalar offset is clamped on the
  // scalar unit, the hardware's range check covers the VGPR offset only.
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(dx0 + (r0 < r1 ? r0 : 0) * 32), 0,
      r0 < r1 ? (int)((r1 - r0) * 128) : 0, 0x00020000);
  const int so_last = r0 < r1 ? (int)((r1 - r0 - 1) * 128) : 0;
  auto fetch_rows = [&](long rb, float (&vv)[CWG_NB]) {
    const int so = __builtin_amdgcn_readfirstlane((int)((rb - r0) * 128));
#pragma unroll
    for (int u = 0; u < CWG_NB; ++u)
      vv[u] = __builtin_bit_cast(
          float, __builtin_amdgcn_raw_buffer_load_b32(rs, c * 4, min(so + u * 128, so_last), 0));
  };
  // a ring of four batches: three are in flight while one is accumulated (a
  // batch of 32 rows is worked off in ~0.7 us, a load takes ~2 us to arrive)
  float ring[4][CWG_NB];
  int codes[4] = {0, 0, 0, 0};
  long fb = r0;                                  // next batch to request
  int tb = r0 < r1 ? (int)(r0 % T) : 0;          // its clip position
  auto request = [&](int slot) {
    if (fb < r1) {
      codes[slot] = fetch_codes(fb, tb);
      fetch_rows(fb, ring[slot]);
    }
    fb += CWG_NB;
    tb += CWG_NB;
    if (tb >= T) tb %= T;
  };
  request(0);
  request(1);
  request(2);
  for (long rb = r0; rb < r1; rb += 4 * CWG_NB) {
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {
      if (rb + sl * CWG_NB >= r1) break;
      request((sl + 3) & 3);
      const float (&v)[CWG_NB] = ring[sl];
      // table address of row u for this lane's tap: lane (u, h)'s offset
      int addr[CWG_NB];
#pragma unroll
      for (int u = 0; u < CWG_NB; ++u)
        addr[u] = __builtin_amdgcn_ds_bpermute(((lane & 32) | u) * 4, codes[sl]) + lane_off;
      // four rows per LDS round trip: the four cells are read together, row k
      // continues from the newest earlier row of the group with the same cell
      // (else from the value read), the four results are written in row order
      // -- bit for bit the row-by-row chain
#pragma unroll
      for (int u = 0; u < CWG_NB; u += 4) {
        float* cell[4];
        float x[4], y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          cell[k] = reinterpret_cast<float*>(reinterpret_cast<char*>(wtab) + addr[u + k]);
          x[k] = *cell[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float from = x[k];
#pragma unroll
          for (int m = 0; m < k; ++m)       // ascending: the newest match wins
            from = addr[u + m] == addr[u + k] ? y[m] : from;
          y[k] = from + v[u + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) *cell[k] = y[k];
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  // (a slab whose row range is empty still writes its zeros)
  f32x4* out = reinterpret_cast<f32x4*>(slabs + slab * (2L * Q * 32));
#pragma unroll
  for (int tap = 0; tap < 2; ++tap) {
    const f32x4* src = reinterpret_cast<const f32x4*>(wtab + tap * trows * 32);
    for (int i = lane; i < Q * 8; i += 64) out[tap * Q * 8 + i] = src[i];
  }
}

int wn_causal_wgrad_slabs(long rows) {
  long n = rows / 256;           // >= 256 rows per wave
  // (500 slabs: kernel 34 -> 23 us, their reduction 11 -> 19 us)
  if (n > 256) n = 256;
  if (n < 2) n = 2;
  return (int)(n & ~1L);         // two waves per workgroup
}

int wn_causal_wgrad(const int32_t* q, const float* dx0, float* slabs,
                    int num_slabs, int B, int T, int Q, void* stream) {
  if (!q || !dx0 || !slabs) return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || Q <= 0 || num_slabs < 2 || (num_slabs & 1))
    return WN_ERR_BAD_SHAPE;
  if (Q > CWG_QMAX) return WN_ERR_UNSUPPORTED;
  const long rows = (long)B * T;
  const long rps = (rows + num_slabs - 1) / num_slabs;
  hipLaunchKernelGGL(causal_wgrad_kernel, dim3(num_slabs / 2), dim3(128), 0,
                     (hipStream_t)stream, q, dx0, slabs, rows, rps, T, Q);
  return wn_check_launch();
}

int wn_xent_partials(long rows) {
  long g = (rows + 3) / 4;
  if (g > 1024) g = 1024;
  return (int)g;
}

int wn_xent(const float* logits, long ld, const int32_t* q, float* dlogits,
            float* loss_partials, int B, int T, int Q, int tf_quirk,
            void* stream) {
  if (!logits || !q || !loss_partials) return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || Q <= 0) return WN_ERR_BAD_SHAPE;
  if ((Q & 3) || (ld & 3)) return WN_ERR_UNSUPPORTED;
  if (!wn_aligned16(logits) || (dlogits && !wn_aligned16(dlogits)))
    return WN_ERR_MISALIGNED;
  const long rows = (long)B * T;
  const float inv_n = 1.0f / (float)rows;
  hipLaunchKernelGGL(xent_kernel, dim3(wn_xent_partials(rows)), dim3(256), 0,
                     (hipStream_t)stream, logits, ld, q, dlogits,
                     loss_partials, rows, T, Q, inv_n, tf_quirk);
  return wn_check_launch();
}

int wn_xent_masked(const float* logits, long ld, const int32_t* q,
                   const int32_t* lengths, const float* inv_den,
                   float* dlogits, float* loss_partials, int B, int T, int Q,
                   int tf_quirk, void* stream) {
  if (!logits || !q || !lengths || !inv_den || !loss_partials)
    return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || Q <= 0) return WN_ERR_BAD_SHAPE;
  if ((Q & 3) || (ld & 3)) return WN_ERR_UNSUPPORTED;
  if (!wn_aligned16(logits) || (dlogits && !wn_aligned16(dlogits)) ||
      ((uintptr_t)lengths & 3) || ((uintptr_t)inv_den & 3))
    return WN_ERR_MISALIGNED;
  const long rows = (long)B * T;
  hipLaunchKernelGGL(xent_masked_kernel, dim3(wn_xent_partials(rows)),
                     dim3(256), 0, (hipStream_t)stream, logits, ld, q, lengths,
                     inv_den, dlogits, loss_partials, rows, T, Q, tf_quirk);
  return wn_check_launch();
}

long wn_xent_score_scratch_floats(long rows) {
  return rows > 0 ? 2 * rows : 0;          // flags [rows], row values [rows]
}

int wn_xent_score(const float* logits, long ld, const int32_t* q,
                  const int32_t* lengths, float* row_nll, double* clip_nll,
                  int32_t* clip_count, int32_t* clip_correct, float* scratch,
                  int B, int T, int Q, void* stream) {
  if (!logits || !q || !clip_nll || !clip_count || !clip_correct || !scratch)
    return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || Q <= 0 || ld < Q) return WN_ERR_BAD_SHAPE;
  if ((Q & 3) || (ld & 3)) return WN_ERR_UNSUPPORTED;
  if (!wn_aligned16(logits) || ((uintptr_t)lengths & 3) ||
      ((uintptr_t)row_nll & 3) || ((uintptr_t)clip_nll & 7) ||
      ((uintptr_t)clip_count & 3) || ((uintptr_t)clip_correct & 3) ||
      ((uintptr_t)scratch & 3))
    return WN_ERR_MISALIGNED;
  const long rows = (long)B * T;
  int32_t* flag = reinterpret_cast<int32_t*>(scratch);
  // (without row_nll the row values go to the scratch: the per-clip sums
  // read the same bits either way)
  float* nll = row_nll ? row_nll : scratch + rows;
  hipLaunchKernelGGL(xent_score_rows_kernel, dim3(wn_xent_partials(rows)),
                     dim3(256), 0, (hipStream_t)stream, logits, ld, q, lengths,
                     nll, flag, rows, T, Q);
  hipLaunchKernelGGL(xent_score_clips_kernel, dim3(B),
                     dim3(SCORE_CLIP_THREADS), 0, (hipStream_t)stream, nll,
                     flag, lengths, clip_nll, clip_count, clip_correct, T);
  return wn_check_launch();
}

int wn_softmax64_row(const float* logits_row, int Q, float* proba,
                     void* stream) {
  if (!logits_row || !proba) return WN_ERR_NULL;
  if (Q <= 0) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(softmax64_row_kernel, dim3(1), dim3(256), 0,
                     (hipStream_t)stream, logits_row, Q, proba);
  return wn_check_launch();
}

int wn_adam(float* p, const float* g, float* m, float* v, long n, float lr_t,
            float beta1, float beta2, float eps, float grad_scale, float l2,
            const float* l2_mask, void* stream) {
  if (!p || !g || !m || !v) return WN_ERR_NULL;
  if (n <= 0) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(adam_kernel, dim3(grid1d(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, p, g, m, v, n, lr_t, beta1, beta2,
                     eps, grad_scale, l2, l2_mask);
  return wn_check_launch();
}

int wn_momentum(float* p, const float* g, float* acc, long n, float lr,
                float momentum, float grad_scale, float l2,
                const float* l2_mask, void* stream) {
  if (!p || !g || !acc) return WN_ERR_NULL;
  if (n <= 0) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(momentum_kernel, dim3(grid1d(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, p, g, acc, n, lr, momentum,
                     grad_scale, l2, l2_mask);
  return wn_check_launch();
}

int wn_rmsprop(float* p, const float* g, float* ms, float* mom, long n,
               float lr, float decay, float momentum, float eps,
               float grad_scale, float l2, const float* l2_mask,
               void* stream) {
  if (!p || !g || !ms || !mom) return WN_ERR_NULL;
  if (n <= 0) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(rmsprop_kernel, dim3(grid1d(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, p, g, ms, mom, n, lr, decay,
                     momentum, eps, grad_scale, l2, l2_mask);
  return wn_check_launch();
}

int wn_grad_norm_partials_count(void) { return GNORM_PARTS; }

int wn_grad_norm_partials(const float* g, long n, double* partials,
                          void* stream) {
  if (!g || !partials) return WN_ERR_NULL;
  if (n <= 0) return WN_ERR_BAD_SHAPE;
  if (!wn_aligned16(g) || ((uintptr_t)partials & 7)) return WN_ERR_MISALIGNED;
  // elements per partial: a multiple of 4, so that every range starts on a
  // 16-byte boundary
  const long per = ((n + 4L * GNORM_PARTS - 1) / (4L * GNORM_PARTS)) * 4;
  hipLaunchKernelGGL(grad_norm_partials_kernel, dim3(GNORM_PARTS),
                     dim3(GNORM_THREADS), 0, (hipStream_t)stream, g, n, per,
                     partials);
  return wn_check_launch();
}

// the added arguments of the *_clip entry points
static int clip_args_check(const double* partials, int nparts, float clip_norm,
                           const float* ema, float ema_decay,
                           const float* norm_out) {
  if (partials) {
    if (nparts != GNORM_PARTS) return WN_ERR_BAD_SHAPE;
    if (!(clip_norm > 0.f) || !std::isfinite(clip_norm))
      return WN_ERR_BAD_SHAPE;
    if ((uintptr_t)partials & 7) return WN_ERR_MISALIGNED;
  }
  if (ema) {
    if (!(ema_decay >= 0.f && ema_decay < 1.f)) return WN_ERR_BAD_SHAPE;
    if ((uintptr_t)ema & 3) return WN_ERR_MISALIGNED;
  }
  if ((uintptr_t)norm_out & 3) return WN_ERR_MISALIGNED;
  return WN_OK;
}

int wn_adam_clip(float* p, const float* g, float* m, float* v, long n,
                 float lr_t, float beta1, float beta2, float eps,
                 float grad_scale, float l2, const float* l2_mask,
                 const double* partials, int nparts, float clip_norm,
                 float* ema, float ema_decay, float* norm_out, void* stream) {
  if (!p || !g || !m || !v) return WN_ERR_NULL;
  if (n <= 0) return WN_ERR_BAD_SHAPE;
  const int rc = clip_args_check(partials, nparts, clip_norm, ema, ema_decay,
                                 norm_out);
  if (rc != WN_OK) return rc;
  hipLaunchKernelGGL(adam_clip_kernel, dim3(grid1d(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, p, g, m, v, n, lr_t, beta1, beta2,
                     eps, grad_scale, l2, l2_mask, partials, clip_norm, ema,
                     ema_decay, norm_out);
  return wn_check_launch();
}

int wn_momentum_clip(float* p, const float* g, float* acc, long n, float lr,
                     float momentum, float grad_scale, float l2,
                     const float* l2_mask, const double* partials, int nparts,
                     float clip_norm, float* ema, float ema_decay,
                     float* norm_out, void* stream) {
  if (!p || !g || !acc) return WN_ERR_NULL;
  if (n <= 0) return WN_ERR_BAD_SHAPE;
  const int rc = clip_args_check(partials, nparts, clip_norm, ema, ema_decay,
                                 norm_out);
  if (rc != WN_OK) return rc;
  hipLaunchKernelGGL(momentum_clip_kernel, dim3(grid1d(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, p, g, acc, n, lr, momentum,
                     grad_scale, l2, l2_mask, partials, clip_norm, ema,
                     ema_decay, norm_out);
  return wn_check_launch();
}

int wn_rmsprop_clip(float* p, const float* g, float* ms, float* mom, long n,
                    float lr, float decay, float momentum, float eps,
                    float grad_scale, float l2, const float* l2_mask,
                    const double* partials, int nparts, float clip_norm,
                    float* ema, float ema_decay, float* norm_out,
                    void* stream) {
  if (!p || !g || !ms || !mom) return WN_ERR_NULL;
  if (n <= 0) return WN_ERR_BAD_SHAPE;
  const int rc = clip_args_check(partials, nparts, clip_norm, ema, ema_decay,
                                 norm_out);
  if (rc != WN_OK) return rc;
  hipLaunchKernelGGL(rmsprop_clip_kernel, dim3(grid1d(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, p, g, ms, mom, n, lr, decay,
                     momentum, eps, grad_scale, l2, l2_mask, partials,
                     clip_norm, ema, ema_decay, norm_out);
  return wn_check_launch();
}

int wn_l2_partials_count(void) { return 256; }

int wn_l2_partials(const float* p, long n, const float* mask, float* partials,
                   void* stream) {
  if (!p || !partials) return WN_ERR_NULL;
  if (n <= 0) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(l2_partials_kernel, dim3(256), dim3(256), 0,
                     (hipStream_t)stream, p, n, mask, partials);
  return wn_check_launch();
}

int wn_gc_bias(const float* layer0, long layer_stride, long off_bias,
               long off_gc, int G, const float* emb, int card,
               const int32_t* ids, float* out, int L, int B, int ch,
               void* stream) {
  if (!layer0 || !out) return WN_ERR_NULL;
  if (emb && !ids) return WN_ERR_NULL;
  if (L <= 0 || B <= 0 || ch < 32) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(gc_bias_kernel, dim3(L, B), dim3(2 * ch < 1024 ? 2 * ch : 1024), 0,
                     (hipStream_t)stream, layer0, layer_stride, off_bias,
                     off_gc, G, emb, card, ids, out, B, ch);
  return wn_check_launch();
}

int wn_colsum_clip_chunks(int T) {
  int c = (T + 511) / 512;
  if (c > 64) c = 64;
  return c < 1 ? 1 : c;
}

// out[b][0:32] = sum_t P0[b][t][:], out[b][32:64] = sum_t P1[b][t][:];
// `part` is caller scratch of B * wn_colsum_clip_chunks(T) * 64 floats.
int wn_colsum_clip(const float* plane0, const float* plane1, int B, int T,
                   float* part, float* out, void* stream) {
  if (!plane0 || !plane1 || !part || !out) return WN_ERR_NULL;
  if (B <= 0 || T <= 0) return WN_ERR_BAD_SHAPE;
  const int chunks = wn_colsum_clip_chunks(T);
  const int rpc = (T + chunks - 1) / chunks;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(colsum_clip_kernel, dim3(chunks, B), dim3(256), 0, s,
                     plane0, plane1, T, rpc, part);
  // fixed-order sum over the chunks (reduce_slabs_kernel lives in wn_gemm.hip)
  return wn_reduce_slabs(part, chunks, 64, B, (long)chunks * 64, 0, 64, out, 64,
                         1, 0, stream);
}

// scratch: L * B * G floats (the per-layer shares of the embedding gradient)
int wn_gc_grad(const float* layer0, long layer_stride, long off_gc, int G,
               const float* emb, int card, const int32_t* ids,
               const float* dsum, int L, int B, float* glayer0, float* gemb,
               float* scratch, int ch, void* stream) {
  if (!layer0 || !emb || !ids || !dsum || !glayer0 || !gemb || !scratch)
    return WN_ERR_NULL;
  if (L <= 0 || B <= 0 || G <= 0 || card <= 0 || ch < 32) return WN_ERR_BAD_SHAPE;
  if ((size_t)B * G * sizeof(float) > 48 * 1024) return WN_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gc_grad_kernel, dim3(2 * L), dim3(256), 0, s, layer0,
                     layer_stride, off_gc, G, emb, card, ids, dsum, L, B,
                     glayer0, scratch, ch);
  hipLaunchKernelGGL(gc_grad_emb_kernel, dim3(1), dim3(256),
                     (size_t)B * G * sizeof(float), s, scratch, L, B, G, card,
                     ids, gemb);
  return wn_check_launch();
}

int wn_causal_conv(const float* x, const float* w, float* y, int B, int T,
                   int Cin, int Cout, int K, int dilation, void* stream) {
  if (!x || !w || !y) return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || Cin <= 0 || Cout <= 0 || K <= 0 || dilation <= 0)
    return WN_ERR_BAD_SHAPE;
  const long total = (long)B * T * Cout;
  hipLaunchKernelGGL(causal_conv_kernel, dim3((unsigned)((total + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, x, w, y, B, T, Cin,
                     Cout, K, dilation);
  return wn_check_launch();
}

int wn_time_to_batch(const float* in, float* out, int B, int T, int C,
                     int dilation, void* stream) {
  if (!in || !out) return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || C <= 0 || dilation <= 0) return WN_ERR_BAD_SHAPE;
  const int U = (T + dilation - 1) / dilation;
  const long total = (long)B * dilation * U * C;
  hipLaunchKernelGGL(time_to_batch_kernel, dim3((unsigned)((total + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, in, out, B, T, C,
                     dilation, U);
  return wn_check_launch();
}

int wn_batch_to_time(const float* in, float* out, int B_out, int U, int C,
                     int dilation, void* stream) {
  if (!in || !out) return WN_ERR_NULL;
  if (B_out <= 0 || U <= 0 || C <= 0 || dilation <= 0) return WN_ERR_BAD_SHAPE;
  const long total = (long)B_out * dilation * U * C;
  hipLaunchKernelGGL(batch_to_time_kernel, dim3((unsigned)((total + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, in, out, B_out, U, C,
                     dilation);
  return wn_check_launch();
}

int wn_axpy(float* y, const float* x, float a, const float* mask, long n,
            void* stream) {
  if (!y || !x) return WN_ERR_NULL;
  if (n <= 0) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(axpy_kernel, dim3(grid1d(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, y, x, a, mask, n);
  return wn_check_launch();
}

int wn_fill(float* p, long n, float value, void* stream) {
  if (!p) return WN_ERR_NULL;
  if (n <= 0) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(fill_kernel, dim3(grid1d(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, p, n, value);
  return wn_check_launch();
}

int wn_sum_rows(const float* in, int rows, int n, float* out, void* stream) {
  if (!in || !out) return WN_ERR_NULL;
  if (rows <= 0 || n <= 0) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(sum_rows_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, in, rows, n, out);
  return wn_check_launch();
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Learned upsampling of frame-rate local-conditioning features (WaveNet paper
// 2.5).  Layer i (scale s_i) is a transposed convolution over time with
// kernel = stride = s_i and, over the feature axis, a 3-tap kernel with zero
// padding and one scalar bias:
//   out[c] = b_i + W_i[j][0] u[c-1] + W_i[j][1] u[c] + W_i[j][2] u[c+1]
// for output slot j of an input row u.  Timeline position p = off[b] + t takes
// frame p / hop and the slot digits of p % hop, most significant first.  A
// row is computed from its frame, its slot and the weights alone, in one
// fixed order (explicit FMAs): its bits do not depend on the batch, the clip
// length, the offset or the call.
//
// Segment layout (`up`): filters W_i[s_i][3] of all layers back to back, then
// (use_bias) the m biases.  Per launch: frames [B][F][Lc], off[b] int32.
// ---------------------------------------------------------------------------
#define LCUP_MAX_LAYERS 8
#define LCUP_MAX_LC 512
#define LCUP_CPL (LCUP_MAX_LC / 64)          // channels per lane

struct LcUpGeom {
  int m, hop, Lc, use_bias;
  int s[LCUP_MAX_LAYERS];    // scales
  int suf[LCUP_MAX_LAYERS];  // s_{i+1} * ... * s_m (slot digit divisor)
  int fo[LCUP_MAX_LAYERS];   // filter offset of layer i in the segment
  int bo;                    // offset of the biases
};

__device__ __forceinline__ int lcup_slot(const LcUpGeom& g, int i, int j) {
  return (j / g.suf[i]) % g.s[i];
}

// one layer of one row: buf_in / buf_out hold Lc + 2 floats with a zero at
// either end (index c + 1 is channel c)
__device__ __forceinline__ void lcup_layer(const LcUpGeom& g,
                                           const float* __restrict__ up, int i,
                                           int j, const float* bin, float* bout,
                                           int lane) {
  const int slot = lcup_slot(g, i, j);
  const float* w = up + g.fo[i] + 3 * slot;
  const float w0 = w[0], w1 = w[1], w2 = w[2];
  const float b = g.use_bias ? up[g.bo + i] : 0.f;
#pragma unroll
  for (int k = 0; k < LCUP_CPL; ++k) {
    const int c = lane + 64 * k;
    if (c < g.Lc) {
      float a = b;
      a = fmaf(w0, bin[c], a);
      a = fmaf(w1, bin[c + 1], a);
      a = fmaf(w2, bin[c + 2], a);
      bout[c + 1] = a;
    }
  }
}

// the frame row of row r into buf (zero ends); returns the slot index p % hop
__device__ __forceinline__ int lcup_load(const LcUpGeom& g,
                                         const float* __restrict__ frames,
                                         int F, const int32_t* __restrict__ off,
                                         int T, long r, float* buf, int lane) {
  const int b = (int)(r / T), t = (int)(r - (long)b * T);
  const long p = (long)off[b] + t;
  long f = p / g.hop;
  if (f > F - 1) f = F - 1;          // (the host checks coverage; never read past)
  const float* src = frames + ((long)b * F + f) * g.Lc;
#pragma unroll
  for (int k = 0; k < LCUP_CPL; ++k) {
    const int c = lane + 64 * k;
    if (c < g.Lc) buf[c + 1] = src[c];
  }
  if (lane == 0) {
    buf[0] = 0.f;
    buf[g.Lc + 1] = 0.f;
  }
  return (int)(p % g.hop);
}

// forward: one wave per row, four rows per workgroup, ping-pong rows in LDS
__global__ __launch_bounds__(256) void lc_upsample_fwd_kernel(
    LcUpGeom g, const float* __restrict__ frames, int F,
    const int32_t* __restrict__ off, const float* __restrict__ up,
    float* __restrict__ out, int ldo, int T, long N) {
  __shared__ float lds[4][2][LCUP_MAX_LC + 2];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + wv;
  const bool live = r < N;
  float* b0 = lds[wv][0];
  float* b1 = lds[wv][1];
  if (lane == 0) b1[0] = b1[g.Lc + 1] = 0.f;
  const int j = live ? lcup_load(g, frames, F, off, T, r, b0, lane) : 0;
  __syncthreads();
  for (int i = 0; i < g.m; ++i) {
    if (live) lcup_layer(g, up, i, j, (i & 1) ? b1 : b0, (i & 1) ? b0 : b1, lane);
    __syncthreads();
  }
  if (!live) return;
  const float* res = (g.m & 1) ? b1 : b0;
  float* dst = out + r * ldo;
  for (int c = lane; c < ldo; c += 64) dst[c] = c < g.Lc ? res[c + 1] : 0.f;
}

__device__ __forceinline__ float lcup_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// backward: one wave per workgroup owning rows [w * rpw, (w + 1) * rpw).  Per
// row: the layer chain again (every layer's input kept in LDS), then d row
// back through the layers; the (layer, slot, tap) and bias partials add up in
// LDS in row order and go to the workgroup's slab at the end.
// CTX (the frame-context variant): the gradient at the layer-0 input, summed
// in registers in row order over the run of rows that share a frame (a
// segment).  A segment that starts at the workgroup's first row goes to
// dpart[w][0], one that ends at its last row (and does not start at its
// first) to dpart[w][1], every other one straight to dfr[b][f]: no two
// workgroups write the same float.  lc_context_dfix_kernel adds the parts.
template <bool CTX>
__global__ __launch_bounds__(64) void lc_upsample_bwd_kernel(
    LcUpGeom g, const float* __restrict__ frames, int F,
    const int32_t* __restrict__ off, const float* __restrict__ up,
    const float* __restrict__ drows, int ldd, int T, long N, long rpw,
    float* __restrict__ slabs, long slab_stride, int nacc,
    float* __restrict__ dfr, float* __restrict__ dpart) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  const int W = g.Lc + 2;
  float* U = lds;                              // [m + 1][W]
  float* G0 = U + (g.m + 1) * W;               // [2][W]
  float* acc = G0 + 2 * W;                     // [nacc]
  for (int e = lane; e < nacc; e += 64) acc[e] = 0.f;
  for (int e = lane; e < 2 * W; e += 64) G0[e] = 0.f;
  for (int i = 1; i <= g.m; ++i)
    if (lane == 0) U[i * W] = U[i * W + g.Lc + 1] = 0.f;
  __syncthreads();
  const long r0 = (long)blockIdx.x * rpw;
  const long r1 = r0 + rpw < N ? r0 + rpw : N;
  float dacc[LCUP_CPL];
  long seg_key = -1, seg_r = r0;      // (b * F + frame) and first row
  if constexpr (CTX) {
#pragma unroll
    for (int k = 0; k < LCUP_CPL; ++k) dacc[k] = 0.f;
  }
  for (long r = r0; r < r1; ++r) {
    if constexpr (CTX) {
      const int b = (int)(r / T);
      const long key = (long)b * F + ((long)off[b] + (r - (long)b * T)) / g.hop;
      if (key != seg_key) {
        if (seg_key >= 0) {
          // a segment that ended before r1: dpart[w][0] or interior
          float* dst = seg_r == r0
                           ? dpart + (long)blockIdx.x * 2 * g.Lc
                           : dfr + seg_key * g.Lc;
#pragma unroll
          for (int k = 0; k < LCUP_CPL; ++k) {
            const int c = lane + 64 * k;
            if (c < g.Lc) dst[c] = dacc[k];
            dacc[k] = 0.f;
          }
        }
        seg_key = key;
        seg_r = r;
      }
    }
    const int j = lcup_load(g, frames, F, off, T, r, U, lane);
    __syncthreads();
    for (int i = 0; i < g.m; ++i) {
      lcup_layer(g, up, i, j, U + i * W, U + (i + 1) * W, lane);
      __syncthreads();
    }
    float* gc = G0;
    float* gn = G0 + W;
    const float* dr = drows + r * ldd;
#pragma unroll
    for (int k = 0; k < LCUP_CPL; ++k) {
      const int c = lane + 64 * k;
      if (c < g.Lc) gc[c + 1] = dr[c];
    }
    __syncthreads();
    for (int i = g.m - 1; i >= 0; --i) {
      const float* u = U + i * W;
      float p0 = 0.f, p1 = 0.f, p2 = 0.f, pb = 0.f;
#pragma unroll
      for (int k = 0; k < LCUP_CPL; ++k) {
        const int c = lane + 64 * k;
        if (c < g.Lc) {
          const float d = gc[c + 1];
          p0 = fmaf(d, u[c], p0);
          p1 = fmaf(d, u[c + 1], p1);
          p2 = fmaf(d, u[c + 2], p2);
          pb += d;
        }
      }
      p0 = lcup_wave_sum(p0);
      p1 = lcup_wave_sum(p1);
      p2 = lcup_wave_sum(p2);
      pb = lcup_wave_sum(pb);
      const int slot = lcup_slot(g, i, j);
      const int fw = g.fo[i] + 3 * slot;
      if (lane == 0) {
        acc[fw] += p0;
        acc[fw + 1] += p1;
        acc[fw + 2] += p2;
        if (g.use_bias) acc[g.bo + i] += pb;
      }
      if (i > 0) {
        // d u[c] = W0 d out[c + 1] + W1 d out[c] + W2 d out[c - 1]
        const float* w = up + fw;
        const float w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
        for (int k = 0; k < LCUP_CPL; ++k) {
          const int c = lane + 64 * k;
          if (c < g.Lc) {
            float a = w0 * gc[c + 2];
            a = fmaf(w1, gc[c + 1], a);
            a = fmaf(w2, gc[c], a);
            gn[c + 1] = a;
          }
        }
        float* t = gc;
        gc = gn;
        gn = t;
      } else if constexpr (CTX) {
        // the layer-0 input's gradient, the same three taps
        const float* w = up + fw;
        const float w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
        for (int k = 0; k < LCUP_CPL; ++k) {
          const int c = lane + 64 * k;
          if (c < g.Lc) {
            float a = w0 * gc[c + 2];
            a = fmaf(w1, gc[c + 1], a);
            a = fmaf(w2, gc[c], a);
            dacc[k] += a;
          }
        }
      }
      __syncthreads();
    }
  }
  if constexpr (CTX) {
    // the last segment: dpart[w][0] if it is also the first, else [w][1]
    float* dst = dpart + ((long)blockIdx.x * 2 + (seg_r == r0 ? 0 : 1)) * g.Lc;
#pragma unroll
    for (int k = 0; k < LCUP_CPL; ++k) {
      const int c = lane + 64 * k;
      if (seg_key >= 0 && c < g.Lc) dst[c] = dacc[k];
    }
  }
  __syncthreads();
  float* dst = slabs + (long)blockIdx.x * slab_stride;
  for (int e = lane; e < nacc; e += 64) dst[e] = acc[e];
}

// d frames [B][F][Lc] of the frame-context variant: frame f of clip b
// gathers rows [max(0, f hop - o), min(T, (f + 1) hop - o)) of the clip
// (o = off[b] < hop).  A frame inside one workgroup's rows that is neither its
// first nor its last segment was written by that workgroup; the others add
// the workgroups' parts in workgroup order; a frame without rows is zero.
__global__ __launch_bounds__(256) void lc_context_dfix_kernel(
    const int32_t* __restrict__ off, int hop, int Lc, int F, int T, long N,
    long rpw, const float* __restrict__ dpart, float* __restrict__ dfr,
    long total) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % Lc);
  const long bf = e / Lc;
  const int b = (int)(bf / F), f = (int)(bf - (long)b * F);
  const long o = off[b];
  long t0 = (long)f * hop - o, t1 = t0 + hop;
  if (t0 < 0) t0 = 0;
  if (t1 > T) t1 = T;
  if (t0 >= t1) {
    dfr[e] = 0.f;
    return;
  }
  const long ra = (long)b * T + t0, rb = (long)b * T + t1;
  const long wlo = ra / rpw, whi = (rb - 1) / rpw;
  if (wlo == whi) {
    const long s = wlo * rpw, x = s + rpw < N ? s + rpw : N;
    if (ra == s)
      dfr[e] = dpart[(wlo * 2) * Lc + c];
    else if (rb == x)
      dfr[e] = dpart[(wlo * 2 + 1) * Lc + c];
    return;                           // (else: written by the workgroup)
  }
  float a = 0.f;
  for (long w = wlo; w <= whi; ++w)
    a += dpart[(w * 2 + (ra <= w * rpw ? 0 : 1)) * Lc + c];
  dfr[e] = a;
}

// ---------------------------------------------------------------------------
// Frame-context convolution in front of the upsampler: a convolution over
// frames with kernel 2p + 1, Lc -> Lc channels, no bias,
//   ctx[b][f][j] = sum_{k, c} W[k][c][j] x[b][f + k][c]
// on x [B][Fx][Lc], the frames staged with p frames of context either side
// (window frame f + k is clip frame f + k - p; zeros outside the clip) and W
// [2p + 1][Lc][Lc].  The window of output frame f is the contiguous run
// x[b][f] .. x[b][f + 2p], K = (2p + 1) Lc floats, summed in kc order: an
// output's bits depend on its window and W only.
// ---------------------------------------------------------------------------
#define LCCTX_MAX_P 8

// forward: one wave per output frame, lane = channel j (+ 64 k); the window
// value is the same for the whole wave
__global__ __launch_bounds__(256) void lc_context_fwd_kernel(
    const float* __restrict__ x, int Fx, const float* __restrict__ w, int K,
    int Lc, float* __restrict__ ctx, int Fw, long rows) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int b = (int)(r / Fw), f = (int)(r - (long)b * Fw);
  const float* xr = x + ((long)b * Fx + f) * Lc;
  float a[LCUP_CPL];
#pragma unroll
  for (int k = 0; k < LCUP_CPL; ++k) a[k] = 0.f;
  for (int kc = 0; kc < K; ++kc) {
    const float v = xr[kc];
    const float* wr = w + (long)kc * Lc;
#pragma unroll
    for (int k = 0; k < LCUP_CPL; ++k) {
      const int c = lane + 64 * k;
      if (c < Lc) a[k] = fmaf(wr[c], v, a[k]);
    }
  }
  float* dst = ctx + r * Lc;
#pragma unroll
  for (int k = 0; k < LCUP_CPL; ++k) {
    const int c = lane + 64 * k;
    if (c < Lc) dst[c] = a[k];
  }
}

// weight gradient dW[kc][j] = sum_r x[r's window][kc] dctx[r][j]: one wave per
// (kc, slab); slab s sums rows [s rps, (s + 1) rps) of the B * Fw output
// frames in order into slabs[s][kc][j] (wn_reduce_slabs adds the slabs)
__global__ __launch_bounds__(256) void lc_context_wgrad_kernel(
    const float* __restrict__ x, int Fx, const float* __restrict__ d, int Fw,
    int K, int Lc, long rows, long rps, float* __restrict__ slabs,
    long slab_stride) {
  const int lane = threadIdx.x & 63;
  const long kc = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (kc >= K) return;
  const long r0 = (long)blockIdx.y * rps;
  const long r1 = r0 + rps < rows ? r0 + rps : rows;
  float a[LCUP_CPL];
#pragma unroll
  for (int k = 0; k < LCUP_CPL; ++k) a[k] = 0.f;
  for (long r = r0; r < r1; ++r) {
    const int b = (int)(r / Fw), f = (int)(r - (long)b * Fw);
    const float v = x[((long)b * Fx + f) * Lc + kc];
    const float* dr = d + r * Lc;
#pragma unroll
    for (int k = 0; k < LCUP_CPL; ++k) {
      const int c = lane + 64 * k;
      if (c < Lc) a[k] = fmaf(v, dr[c], a[k]);
    }
  }
  float* dst = slabs + (long)blockIdx.y * slab_stride + kc * Lc;
#pragma unroll
  for (int k = 0; k < LCUP_CPL; ++k) {
    const int c = lane + 64 * k;
    if (c < Lc) dst[c] = a[k];
  }
}

static int lcup_geom(const int* scales, int m, int Lc, int use_bias,
                     LcUpGeom* g, int* nacc) {
  if (!scales) return WN_ERR_NULL;
  if (m < 1 || m > LCUP_MAX_LAYERS || Lc < 1 || Lc > LCUP_MAX_LC)
    return WN_ERR_BAD_SHAPE;
  long hop = 1;
  for (int i = 0; i < m; ++i) {
    if (scales[i] < 2) return WN_ERR_BAD_SHAPE;
    hop *= scales[i];
    if (hop > 4096) return WN_ERR_BAD_SHAPE;
  }
  g->m = m;
  g->hop = (int)hop;
  g->Lc = Lc;
  g->use_bias = use_bias ? 1 : 0;
  int fo = 0, suf = 1;
  for (int i = m - 1; i >= 0; --i) {
    g->suf[i] = suf;
    suf *= scales[i];
  }
  for (int i = 0; i < LCUP_MAX_LAYERS; ++i) {
    g->s[i] = i < m ? scales[i] : 1;
    if (i >= m) g->suf[i] = 1;
    g->fo[i] = fo;
    if (i < m) fo += 3 * scales[i];
  }
  g->bo = fo;
  *nacc = fo + (use_bias ? m : 0);
  return WN_OK;
}

extern "C" {

int wn_lc_upsample_floats(const int* scales, int m, int use_bias) {
  LcUpGeom g;
  int n = 0;
  if (lcup_geom(scales, m, 1, use_bias, &g, &n) != WN_OK) return 0;
  return n;
}

int wn_lc_upsample_fwd(const float* frames, int F, const int32_t* off,
                       const float* up, const int* scales, int m, int Lc,
                       int use_bias, float* rows, int ld_rows, int B, int T,
                       void* stream) {
  if (!frames || !off || !up || !rows) return WN_ERR_NULL;
  LcUpGeom g;
  int nacc = 0;
  const int rc = lcup_geom(scales, m, Lc, use_bias, &g, &nacc);
  if (rc != WN_OK) return rc;
  if (F < 1 || B < 1 || T < 1 || ld_rows < Lc) return WN_ERR_BAD_SHAPE;
  const long N = (long)B * T;
  hipLaunchKernelGGL(lc_upsample_fwd_kernel, dim3((unsigned)((N + 3) / 4)),
                     dim3(256), 0, (hipStream_t)stream, g, frames, F, off, up,
                     rows, ld_rows, T, N);
  return wn_check_launch();
}

int wn_lc_upsample_bwd_slabs(long rows, int nacc) {
  if (rows <= 0 || nacc <= 0) return 0;
  long n = (rows + 31) / 32;                   // >= 32 rows per workgroup
  long cap = (16L << 20) / nacc;               // <= 64 MB of slabs
  if (cap < 64) cap = 64;
  if (n > 4096) n = 4096;
  if (n > cap) n = cap;
  return (int)(n < 1 ? 1 : n);
}

int wn_lc_upsample_bwd(const float* frames, int F, const int32_t* off,
                       const float* up, const int* scales, int m, int Lc,
                       int use_bias, const float* drows, int ld_drows, int B,
                       int T, float* slabs, int num_slabs, long slab_stride,
                       void* stream) {
  if (!frames || !off || !up || !drows || !slabs) return WN_ERR_NULL;
  LcUpGeom g;
  int nacc = 0;
  const int rc = lcup_geom(scales, m, Lc, use_bias, &g, &nacc);
  if (rc != WN_OK) return rc;
  if (F < 1 || B < 1 || T < 1 || ld_drows < Lc || num_slabs < 1 ||
      slab_stride < nacc)
    return WN_ERR_BAD_SHAPE;
  const long N = (long)B * T;
  const long rpw = (N + num_slabs - 1) / num_slabs;
  const size_t lds = sizeof(float) * ((size_t)(m + 3) * (Lc + 2) + nacc);
  if (lds > 64 * 1024) return WN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(lc_upsample_bwd_kernel<false>, dim3((unsigned)num_slabs),
                     dim3(64), lds, (hipStream_t)stream, g, frames, F, off, up,
                     drows, ld_drows, T, N, rpw, slabs, slab_stride, nacc,
                     nullptr, nullptr);
  return wn_check_launch();
}

int wn_lc_upsample_bwd_ctx(const float* frames, int F, const int32_t* off,
                           const float* up, const int* scales, int m, int Lc,
                           int use_bias, const float* drows, int ld_drows,
                           int B, int T, float* slabs, int num_slabs,
                           long slab_stride, float* dframes, float* dpart,
                           void* stream) {
  if (!frames || !off || !up || !drows || !slabs || !dframes || !dpart)
    return WN_ERR_NULL;
  LcUpGeom g;
  int nacc = 0;
  const int rc = lcup_geom(scales, m, Lc, use_bias, &g, &nacc);
  if (rc != WN_OK) return rc;
  if (F < 1 || B < 1 || T < 1 || ld_drows < Lc || num_slabs < 1 ||
      slab_stride < nacc)
    return WN_ERR_BAD_SHAPE;
  // every row's frame inside the F frames (offsets < hop on the device)
  if ((long)(T + g.hop - 2) / g.hop + 1 > F) return WN_ERR_BAD_SHAPE;
  const long N = (long)B * T;
  const long rpw = (N + num_slabs - 1) / num_slabs;
  const size_t lds = sizeof(float) * ((size_t)(m + 3) * (Lc + 2) + nacc);
  if (lds > 64 * 1024) return WN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(lc_upsample_bwd_kernel<true>, dim3((unsigned)num_slabs),
                     dim3(64), lds, (hipStream_t)stream, g, frames, F, off, up,
                     drows, ld_drows, T, N, rpw, slabs, slab_stride, nacc,
                     dframes, dpart);
  const long total = (long)B * F * Lc;
  hipLaunchKernelGGL(lc_context_dfix_kernel, dim3((unsigned)((total + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, off, g.hop, Lc, F, T, N,
                     rpw, dpart, dframes, total);
  return wn_check_launch();
}

int wn_lc_context_fwd(const float* x, int Fx, const float* w, int p, int Lc,
                      float* ctx, int Fw, int B, void* stream) {
  if (!x || !w || !ctx) return WN_ERR_NULL;
  if (p < 0 || p > LCCTX_MAX_P || Lc < 1 || Lc > LCUP_MAX_LC || Fw < 1 ||
      B < 1 || Fx < Fw + 2 * p)
    return WN_ERR_BAD_SHAPE;
  const long rows = (long)B * Fw;
  hipLaunchKernelGGL(lc_context_fwd_kernel, dim3((unsigned)((rows + 3) / 4)),
                     dim3(256), 0, (hipStream_t)stream, x, Fx, w,
                     (2 * p + 1) * Lc, Lc, ctx, Fw, rows);
  return wn_check_launch();
}

int wn_lc_context_wgrad_slabs(long rows, int nacc) {
  if (rows <= 0 || nacc <= 0) return 0;
  long n = (rows + 31) / 32;                   // >= 32 frames per slab
  long cap = (16L << 20) / nacc;               // <= 64 MB of slabs
  if (cap < 1) cap = 1;
  if (n > 256) n = 256;
  if (n > cap) n = cap;
  return (int)(n < 1 ? 1 : n);
}

int wn_lc_context_wgrad(const float* x, int Fx, const float* dctx, int Fw,
                        int p, int Lc, int B, float* slabs, int num_slabs,
                        long slab_stride, void* stream) {
  if (!x || !dctx || !slabs) return WN_ERR_NULL;
  if (p < 0 || p > LCCTX_MAX_P || Lc < 1 || Lc > LCUP_MAX_LC || Fw < 1 ||
      B < 1 || Fx < Fw + 2 * p || num_slabs < 1 || num_slabs > 65535)
    return WN_ERR_BAD_SHAPE;
  const int K = (2 * p + 1) * Lc;
  if (slab_stride < (long)K * Lc) return WN_ERR_BAD_SHAPE;
  const long rows = (long)B * Fw;
  const long rps = (rows + num_slabs - 1) / num_slabs;
  hipLaunchKernelGGL(lc_context_wgrad_kernel,
                     dim3((unsigned)((K + 3) / 4), (unsigned)num_slabs),
                     dim3(256), 0, (hipStream_t)stream, x, Fx, dctx, Fw, K, Lc,
                     rows, rps, slabs, slab_stride);
  return wn_check_launch();
}

}  // extern "C"
