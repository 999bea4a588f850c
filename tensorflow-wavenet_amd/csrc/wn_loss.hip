// Fused softmax cross-entropy of the training step (plain and per-clip
// masked), held-out scoring on the same row arithmetic, and the float64
// softmax of one row.
#include "wn_common.h"
#include <cmath>

#pragma clang fp contract(off)

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
//
// WINDOW (wn_xent_window): clip b also has starts[b] leading samples of
// history, fed to the network but predicted by nobody: row t has a target iff
// starts[b] <= t + 1 < lengths[b].  Rows with t + 1 < starts[b] are treated
// like padding (nothing to the loss, an all-zero dlogits row, no exponential);
// row lengths[b] - 1 stays the label-less last row.  starts[b] = 0 takes
// exactly the masked arithmetic.
// ---------------------------------------------------------------------------
// clip b's length: lengths[b] clamped to [0, T]
__device__ __forceinline__ int clip_len(const int32_t* __restrict__ lengths,
                                        long b, int T) {
  return min(max(lengths[b], 0), T);
}

// clip b's history: starts[b] clamped to [0, T]; 0 without starts
__device__ __forceinline__ int clip_start(const int32_t* __restrict__ starts,
                                          long b, int T) {
  return starts ? min(max(starts[b], 0), T) : 0;
}

// One row's float32 softmax statistics, by one wave: maximum, sum of
// exp(logit - m), m + logf(se).  Loss and scoring both take them from here, so
// a scored row is the loss kernel's row bit for bit.
struct XentRow {
  float m, se, lse;
};

// Q == 256: lane l holds logits 4 l .. 4 l + 3 in v; e[k] = exp(v[k] - m)
__device__ __forceinline__ XentRow xent_row256(const f32x4& v, float e[4]) {
  XentRow r;
  r.m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) r.m = fmaxf(r.m, __shfl_xor(r.m, o));
#pragma unroll
  for (int k = 0; k < 4; ++k) e[k] = expf(v[k] - r.m);
  r.se = (e[0] + e[1]) + (e[2] + e[3]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) r.se += __shfl_xor(r.se, o);
  r.lse = r.m + logf(r.se);
  return r;
}

// the label's logit of such a row, in every lane: it lives in lane label >> 2
__device__ __forceinline__ float xent_logit256(const f32x4& v, int lane,
                                               int label) {
  float ll = (label >> 2) == lane ? v[label & 3] : 0.f;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ll += __shfl_xor(ll, o);
  return ll;
}

// any Q (a multiple of 4): lane l walks the 16-byte groups l, l + 64, ... of
// the row at lp, once for the maximum and once for the sum (the label's logit
// is lp[label]).  ARGMAX: the second pass also leaves this lane's lowest index
// holding the maximum in *best (INT_MAX for none); without ARGMAX best is
// never dereferenced, and the loss passes nullptr.
template <bool ARGMAX>
__device__ __forceinline__ XentRow xent_row(const float* __restrict__ lp, int Q,
                                            int lane, int* best) {
  XentRow r;
  r.m = -INFINITY;
  for (int c = lane * 4; c < Q; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(lp + c);
    r.m = fmaxf(fmaxf(r.m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) r.m = fmaxf(r.m, __shfl_xor(r.m, o));
  r.se = 0.f;
  if (ARGMAX) *best = 0x7fffffff;
  for (int c = lane * 4; c < Q; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(lp + c);
    r.se += expf(v[0] - r.m) + expf(v[1] - r.m) + expf(v[2] - r.m) +
            expf(v[3] - r.m);
    if (ARGMAX) {
#pragma unroll
      for (int k = 3; k >= 0; --k)
        *best = v[k] == r.m ? min(*best, c + k) : *best;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) r.se += __shfl_xor(r.se, o);
  r.lse = r.m + logf(r.se);
  return r;
}

template <bool MASKED, bool WINDOW>
__device__ __forceinline__ void xent_body(
    const float* __restrict__ logits, long ld, const int32_t* __restrict__ q,
    const int32_t* __restrict__ starts, const int32_t* __restrict__ lengths,
    float* __restrict__ dlogits,
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
      const int len = MASKED ? clip_len(lengths, row / T, T) : T;
      if (MASKED && (t >= len ||             // padding, history
                     (WINDOW && t + 1 < clip_start(starts, row / T, T)))) {
        if (dlogits)
          *reinterpret_cast<f32x4*>(dlogits + row * ld + lane * 4) =
              f32x4{0.f, 0.f, 0.f, 0.f};
        v = vn;
        continue;
      }
      const int label = (t + 1 < len) ? q[row + 1] : -1;
      const bool has_label = label >= 0 && label < Q;
      float e[4];
      const XentRow r = xent_row256(v, e);
      if (has_label) {
        const float ll = xent_logit256(v, lane, label);
        if (lane == 0) lsum += r.lse - ll;
      }
      if (dlogits) {
        const float inv_se = 1.f / r.se;
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
    const int len = MASKED ? clip_len(lengths, row / T, T) : T;
    if (MASKED && (t >= len ||               // padding, history
                   (WINDOW && t + 1 < clip_start(starts, row / T, T)))) {
      if (dlogits)
        for (int c = lane * 4; c < Q; c += 256)
          *reinterpret_cast<f32x4*>(dlogits + row * ld + c) =
              f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    const int label = (t + 1 < len) ? q[row + 1] : -1;
    const bool has_label = label >= 0 && label < Q;
    const XentRow r = xent_row<false>(lp, Q, lane, nullptr);
    if (has_label && lane == 0) lsum += r.lse - lp[label];
    const float inv_se = 1.f / r.se;
    const bool back = has_label || tf_quirk;
    if (dlogits) {
      float* dp = dlogits + row * ld;
      for (int c = lane * 4; c < Q; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(lp + c);
        f32x4 g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float p = back ? expf(v[e] - r.m) * inv_se : 0.f;
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
  xent_body<false, false>(logits, ld, q, nullptr, nullptr, dlogits,
                          loss_partials, rows, T, Q, inv_n, tf_quirk);
}

// lengths [B] and 1 / denominator are read from device memory: a recorded
// launch replays with this call's values
__global__ __launch_bounds__(256) void xent_masked_kernel(
    const float* __restrict__ logits, long ld, const int32_t* __restrict__ q,
    const int32_t* __restrict__ lengths, const float* __restrict__ inv_den,
    float* __restrict__ dlogits, float* __restrict__ loss_partials, long rows,
    int T, int Q, int tf_quirk) {
  xent_body<true, false>(logits, ld, q, nullptr, lengths, dlogits,
                         loss_partials, rows, T, Q, *inv_den, tf_quirk);
}

// starts [B] is read from device memory like lengths and 1 / denominator
__global__ __launch_bounds__(256) void xent_window_kernel(
    const float* __restrict__ logits, long ld, const int32_t* __restrict__ q,
    const int32_t* __restrict__ starts, const int32_t* __restrict__ lengths,
    const float* __restrict__ inv_den, float* __restrict__ dlogits,
    float* __restrict__ loss_partials, long rows, int T, int Q, int tf_quirk) {
  xent_body<true, true>(logits, ld, q, starts, lengths, dlogits, loss_partials,
                        rows, T, Q, *inv_den, tf_quirk);
}

// ---------------------------------------------------------------------------
// scoring (wn_xent_score): per-row negative log-likelihood, per-clip sums,
// target counts and arg-max hits of held-out data.  Forward only.
//
// xent_score_rows_kernel: one wave per row, xent_body's row functions
// (xent_row256, xent_row) on the rows that have a target -- t + 1 < len_b and
// 0 <= q[b][t + 1] < Q -- and nothing but a stored 0 for the others (the
// label-less last row, a code out of range, padding): no exponential is
// evaluated there.  It writes nll[row] and flag[row] = 0 (no target) |
// 1 (target) | 3 (target, and the lowest index of the row's maximum over
// [0, Q) is the target; never for a row whose logsumexp is NaN).  Columns
// >= Q are not read.
// xent_score_clips_kernel: one workgroup per clip.  Thread i sums rows i,
// i + 1024, ... below len_b - 1 in float64 (integers for the flags), a fixed
// LDS tree finishes: a function of the rows' values and len_b alone, whatever
// order the workgroups of either kernel ran in.  No atomics.
//
// starts (wn_xent_score_window, nullable): rows with t + 1 < starts[b] have
// no target either; the per-clip sums then run over rows max(starts[b] - 1, 0)
// .. len_b - 2 in the same order.
// ---------------------------------------------------------------------------
#define SCORE_CLIP_THREADS 1024

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(256) void xent_score_rows_kernel(
    const float* __restrict__ logits, long ld, const int32_t* __restrict__ q,
    const int32_t* __restrict__ starts, const int32_t* __restrict__ lengths,
    float* __restrict__ nll, int32_t* __restrict__ flag, long rows, int T,
    int Q) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long nwaves = (long)gridDim.x * 4;
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
      const int len = lengths ? clip_len(lengths, row / T, T) : T;
      const int label =
          (t + 1 < len && t + 1 >= clip_start(starts, row / T, T)) ? q[row + 1] : -1;
      if (!(label >= 0 && label < Q)) {      // no target: nothing to evaluate
        if (lane == 0) {
          nll[row] = 0.f;
          flag[row] = 0;
        }
        v = vn;
        continue;
      }
      float e[4];
      const XentRow r = xent_row256(v, e);
      const float ll = xent_logit256(v, lane, label);
      int best = 0x7fffffff;                 // lowest index holding the maximum
#pragma unroll
      for (int k = 3; k >= 0; --k) best = v[k] == r.m ? lane * 4 + k : best;
      best = wave_min_i32(best);
      if (lane == 0) {
        nll[row] = r.lse - ll;
        flag[row] = (best == label && r.lse == r.lse) ? 3 : 1;
      }
      v = vn;
    }
    return;
  }
  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += nwaves) {
    const float* lp = logits + row * ld;
    const int t = (int)(row % T);
    const int len = lengths ? clip_len(lengths, row / T, T) : T;
    const int label =
        (t + 1 < len && t + 1 >= clip_start(starts, row / T, T)) ? q[row + 1] : -1;
    if (!(label >= 0 && label < Q)) {
      if (lane == 0) {
        nll[row] = 0.f;
        flag[row] = 0;
      }
      continue;
    }
    int best;
    const XentRow r = xent_row<true>(lp, Q, lane, &best);
    best = wave_min_i32(best);
    if (lane == 0) {
      nll[row] = r.lse - lp[label];
      flag[row] = (best == label && r.lse == r.lse) ? 3 : 1;
    }
  }
}

__global__ __launch_bounds__(SCORE_CLIP_THREADS) void xent_score_clips_kernel(
    const float* __restrict__ nll, const int32_t* __restrict__ flag,
    const int32_t* __restrict__ starts, const int32_t* __restrict__ lengths,
    double* __restrict__ clip_nll,
    int32_t* __restrict__ clip_count, int32_t* __restrict__ clip_correct,
    int T) {
  __shared__ double rs[SCORE_CLIP_THREADS];
  __shared__ int rc[SCORE_CLIP_THREADS], rh[SCORE_CLIP_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = lengths ? clip_len(lengths, b, T) : T;
  const float* pn = nll + (long)b * T;
  const int32_t* pf = flag + (long)b * T;
  double s = 0.0;
  int c = 0, h = 0;
  // (rows t >= len - 1 and rows t + 1 < start have no target: zeros by
  // construction, not read)
  const int t0 = max(clip_start(starts, b, T) - 1, 0);
  for (int t = t0 + tid; t < len - 1; t += SCORE_CLIP_THREADS) {
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

extern "C" {

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

int wn_xent_window(const float* logits, long ld, const int32_t* q,
                   const int32_t* starts, const int32_t* lengths,
                   const float* inv_den, float* dlogits, float* loss_partials,
                   int B, int T, int Q, int tf_quirk, void* stream) {
  if (!logits || !q || !starts || !lengths || !inv_den || !loss_partials)
    return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || Q <= 0) return WN_ERR_BAD_SHAPE;
  if ((Q & 3) || (ld & 3)) return WN_ERR_UNSUPPORTED;
  if (!wn_aligned16(logits) || (dlogits && !wn_aligned16(dlogits)) ||
      ((uintptr_t)starts & 3) || ((uintptr_t)lengths & 3) ||
      ((uintptr_t)inv_den & 3))
    return WN_ERR_MISALIGNED;
  const long rows = (long)B * T;
  hipLaunchKernelGGL(xent_window_kernel, dim3(wn_xent_partials(rows)),
                     dim3(256), 0, (hipStream_t)stream, logits, ld, q, starts,
                     lengths, inv_den, dlogits, loss_partials, rows, T, Q,
                     tf_quirk);
  return wn_check_launch();
}

long wn_xent_score_scratch_floats(long rows) {
  return rows > 0 ? 2 * rows : 0;          // flags [rows], row values [rows]
}

int wn_xent_score_window(const float* logits, long ld, const int32_t* q,
                         const int32_t* starts, const int32_t* lengths,
                         float* row_nll, double* clip_nll, int32_t* clip_count,
                         int32_t* clip_correct, float* scratch, int B, int T,
                         int Q, void* stream) {
  if (!logits || !q || !clip_nll || !clip_count || !clip_correct || !scratch)
    return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || Q <= 0 || ld < Q) return WN_ERR_BAD_SHAPE;
  if ((Q & 3) || (ld & 3)) return WN_ERR_UNSUPPORTED;
  if (!wn_aligned16(logits) || ((uintptr_t)starts & 3) ||
      ((uintptr_t)lengths & 3) || ((uintptr_t)row_nll & 3) || ((uintptr_t)clip_nll & 7) ||
      ((uintptr_t)clip_count & 3) || ((uintptr_t)clip_correct & 3) ||
      ((uintptr_t)scratch & 3))
    return WN_ERR_MISALIGNED;
  const long rows = (long)B * T;
  int32_t* flag = reinterpret_cast<int32_t*>(scratch);
  // (without row_nll the row values go to the scratch: the per-clip sums
  // read the same bits either way)
  float* nll = row_nll ? row_nll : scratch + rows;
  hipLaunchKernelGGL(xent_score_rows_kernel, dim3(wn_xent_partials(rows)),
                     dim3(256), 0, (hipStream_t)stream, logits, ld, q, starts,
                     lengths, nll, flag, rows, T, Q);
  hipLaunchKernelGGL(xent_score_clips_kernel, dim3(B),
                     dim3(SCORE_CLIP_THREADS), 0, (hipStream_t)stream, nll,
                     flag, starts, lengths, clip_nll, clip_count, clip_correct,
                     T);
  return wn_check_launch();
}

int wn_xent_score(const float* logits, long ld, const int32_t* q,
                  const int32_t* lengths, float* row_nll, double* clip_nll,
                  int32_t* clip_count, int32_t* clip_correct, float* scratch,
                  int B, int T, int Q, void* stream) {
  return wn_xent_score_window(logits, ld, q, nullptr, lengths, row_nll,
                              clip_nll, clip_count, clip_correct, scratch, B,
                              T, Q, stream);
}

int wn_softmax64_row(const float* logits_row, int Q, float* proba,
                     void* stream) {
  if (!logits_row || !proba) return WN_ERR_NULL;
  if (Q <= 0) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(softmax64_row_kernel, dim3(1), dim3(256), 0,
                     (hipStream_t)stream, logits_row, Q, proba);
  return wn_check_launch();
}

}  // extern "C"
