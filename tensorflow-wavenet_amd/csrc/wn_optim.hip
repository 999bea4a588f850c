// Optimizers with TensorFlow update rules over the flat parameter buffer,
// with and without global-norm clipping and EMA shadow weights, and the L2 and
// gradient-norm partial sums.
#include "wn_common.h"
#include <cmath>

#pragma clang fp contract(off)

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
// global-norm clipping (tf.clip_by_global_norm): the norm's partial sums.
//
// grad_norm_partials_kernel: GNORM_PARTS float64 sums of g[i]^2.  Partial k
// covers elements [k * per, min(n, (k + 1) * per)), per = the multiple of 4
// next above n / GNORM_PARTS; inside it thread t takes the 16-byte groups
// t, t + 1024, ... in order, a wave is summed by a shuffle tree and the 16
// wave sums in order.  Grid, block and ranges depend on (n, GNORM_PARTS) only:
// the bits are a function of the bucket and n, not of the device.
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

// ---------------------------------------------------------------------------
// optimizers, TensorFlow-0.10 update rules (wavenet/ops.py:6-24)
//   g' = g * scale + l2 * p * (l2_mask ? l2_mask[i] : 1)
//
// A rule's step(i, w, g') stores element i's new slots and returns the new
// parameter; every kernel below is optim_update, the one element loop, around
// a rule.  The *_clip kernels (tf.clip_by_global_norm, tf.train.
// ExponentialMovingAverage) add a prologue in which EVERY workgroup sums the
// same float64 partials in the same order, norm = grad_scale * sqrt(sum),
// factor = clip_norm / max(norm, clip_norm) (NaN for a non-finite norm, as
// TensorFlow), scale = grad_scale * (float)factor -- grad_scale itself when
// norm <= clip_norm: the plain kernel's update bit for bit -- and an epilogue
// s -= (1 - decay) * (s - p_new) on the shadow weights.
// ---------------------------------------------------------------------------
struct AdamRule {
  float *m, *v;
  float lr_t, b1, b2, eps;
  __device__ __forceinline__ float step(long i, float w, float gg) const {
    const float mm = b1 * m[i] + (1.f - b1) * gg;
    const float vv = b2 * v[i] + (1.f - b2) * gg * gg;
    m[i] = mm;
    v[i] = vv;
    return w - lr_t * mm / (sqrtf(vv) + eps);
  }
};

struct MomentumRule {
  float* acc;
  float lr, mom;
  __device__ __forceinline__ float step(long i, float w, float gg) const {
    const float a = mom * acc[i] + gg;
    acc[i] = a;
    return w - lr * a;
  }
};

struct RmspropRule {
  float *ms, *mo;
  float lr, decay, mom, eps;
  __device__ __forceinline__ float step(long i, float w, float gg) const {
    const float s = decay * ms[i] + (1.f - decay) * gg * gg;
    const float mm = mom * mo[i] + lr * gg / sqrtf(s + eps);
    ms[i] = s;
    mo[i] = mm;
    return w - mm;
  }
};

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

// the added arguments of a *_clip kernel
struct ClipEma {
  const double* partials;
  float clip_norm;
  float* ema;
  float ema_decay;
  float* norm_out;
};

// CLIP = false: no prologue, no shadow, `ce` unused.  `bdim` is blockDim.x,
// read by the kernel: the compiler folds it to the uniform workgroup size in
// a __global__ function only.
template <bool CLIP, class Rule>
__device__ __forceinline__ void optim_update(
    unsigned bdim, float* __restrict__ p, const float* __restrict__ g, long n,
    float grad_scale, float l2, const float* __restrict__ l2_mask,
    Rule rule, ClipEma ce) {
  float scale = grad_scale, keep = 0.f;
  if constexpr (CLIP) {
    scale = clip_scale(ce.partials, ce.clip_norm, grad_scale, ce.norm_out);
    keep = 1.f - ce.ema_decay;
  }
  for (long i = (long)blockIdx.x * bdim + threadIdx.x; i < n;
       i += (long)gridDim.x * bdim) {
    const float w = p[i];
    float gg = g[i] * scale;
    if (l2 != 0.f) gg += l2 * w * (l2_mask ? l2_mask[i] : 1.f);
    const float pn = rule.step(i, w, gg);
    p[i] = pn;
    if constexpr (CLIP) {
      if (ce.ema) {
        const float s = ce.ema[i];
        ce.ema[i] = s - keep * (s - pn);
      }
    }
  }
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v,
                            long n, float lr_t, float b1, float b2, float eps,
                            float grad_scale, float l2,
                            const float* __restrict__ l2_mask) {
  optim_update<false>(blockDim.x, p, g, n, grad_scale, l2, l2_mask,
                      AdamRule{m, v, lr_t, b1, b2, eps}, ClipEma{});
}

__global__ void momentum_kernel(float* __restrict__ p,
                                const float* __restrict__ g,
                                float* __restrict__ acc, long n, float lr,
                                float mom, float grad_scale, float l2,
                                const float* __restrict__ l2_mask) {
  optim_update<false>(blockDim.x, p, g, n, grad_scale, l2, l2_mask,
                      MomentumRule{acc, lr, mom}, ClipEma{});
}

__global__ void rmsprop_kernel(float* __restrict__ p,
                               const float* __restrict__ g,
                               float* __restrict__ ms, float* __restrict__ mo,
                               long n, float lr, float decay, float mom,
                               float eps, float grad_scale, float l2,
                               const float* __restrict__ l2_mask) {
  optim_update<false>(blockDim.x, p, g, n, grad_scale, l2, l2_mask,
                      RmspropRule{ms, mo, lr, decay, mom, eps}, ClipEma{});
}

__global__ __launch_bounds__(256) void adam_clip_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, long n, float lr_t, float b1, float b2, float eps,
    float grad_scale, float l2, const float* __restrict__ l2_mask,
    const double* __restrict__ partials, float clip_norm,
    float* __restrict__ ema, float ema_decay, float* __restrict__ norm_out) {
  optim_update<true>(blockDim.x, p, g, n, grad_scale, l2, l2_mask,
                     AdamRule{m, v, lr_t, b1, b2, eps},
                     ClipEma{partials, clip_norm, ema, ema_decay, norm_out});
}

__global__ __launch_bounds__(256) void momentum_clip_kernel(
    float* __restrict__ p, const float* __restrict__ g,
    float* __restrict__ acc, long n, float lr, float mom, float grad_scale,
    float l2, const float* __restrict__ l2_mask,
    const double* __restrict__ partials, float clip_norm,
    float* __restrict__ ema, float ema_decay, float* __restrict__ norm_out) {
  optim_update<true>(blockDim.x, p, g, n, grad_scale, l2, l2_mask,
                     MomentumRule{acc, lr, mom},
                     ClipEma{partials, clip_norm, ema, ema_decay, norm_out});
}

__global__ __launch_bounds__(256) void rmsprop_clip_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ ms,
    float* __restrict__ mo, long n, float lr, float decay, float mom,
    float eps, float grad_scale, float l2, const float* __restrict__ l2_mask,
    const double* __restrict__ partials, float clip_norm,
    float* __restrict__ ema, float ema_decay, float* __restrict__ norm_out) {
  optim_update<true>(blockDim.x, p, g, n, grad_scale, l2, l2_mask,
                     RmspropRule{ms, mo, lr, decay, mom, eps},
                     ClipEma{partials, clip_norm, ema, ema_decay, norm_out});
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

// what the six optimizer entry points share: null pointers, n, the verdict of
// clip_args_check (WN_OK for a plain one), then the launch over n elements
template <class Kernel, class... Args>
static int optim_launch(Kernel kernel, bool have_ptrs, long n, int clip_rc,
                        void* stream, Args... args) {
  if (!have_ptrs) return WN_ERR_NULL;
  if (n <= 0) return WN_ERR_BAD_SHAPE;
  if (clip_rc != WN_OK) return clip_rc;
  hipLaunchKernelGGL(kernel, dim3(grid1d(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, args...);
  return wn_check_launch();
}

extern "C" {

int wn_adam(float* p, const float* g, float* m, float* v, long n, float lr_t,
            float beta1, float beta2, float eps, float grad_scale, float l2,
            const float* l2_mask, void* stream) {
  return optim_launch(adam_kernel, p && g && m && v, n, WN_OK, stream, p, g, m,
                      v, n, lr_t, beta1, beta2, eps, grad_scale, l2, l2_mask);
}

int wn_momentum(float* p, const float* g, float* acc, long n, float lr,
                float momentum, float grad_scale, float l2,
                const float* l2_mask, void* stream) {
  return optim_launch(momentum_kernel, p && g && acc, n, WN_OK, stream, p, g,
                      acc, n, lr, momentum, grad_scale, l2, l2_mask);
}

int wn_rmsprop(float* p, const float* g, float* ms, float* mom, long n,
               float lr, float decay, float momentum, float eps,
               float grad_scale, float l2, const float* l2_mask,
               void* stream) {
  return optim_launch(rmsprop_kernel, p && g && ms && mom, n, WN_OK, stream, p,
                      g, ms, mom, n, lr, decay, momentum, eps, grad_scale, l2,
                      l2_mask);
}

int wn_adam_clip(float* p, const float* g, float* m, float* v, long n,
                 float lr_t, float beta1, float beta2, float eps,
                 float grad_scale, float l2, const float* l2_mask,
                 const double* partials, int nparts, float clip_norm,
                 float* ema, float ema_decay, float* norm_out, void* stream) {
  return optim_launch(
      adam_clip_kernel, p && g && m && v, n,
      clip_args_check(partials, nparts, clip_norm, ema, ema_decay, norm_out),
      stream, p, g, m, v, n, lr_t, beta1, beta2, eps, grad_scale, l2, l2_mask,
      partials, clip_norm, ema, ema_decay, norm_out);
}

int wn_momentum_clip(float* p, const float* g, float* acc, long n, float lr,
                     float momentum, float grad_scale, float l2,
                     const float* l2_mask, const double* partials, int nparts,
                     float clip_norm, float* ema, float ema_decay,
                     float* norm_out, void* stream) {
  return optim_launch(
      momentum_clip_kernel, p && g && acc, n,
      clip_args_check(partials, nparts, clip_norm, ema, ema_decay, norm_out),
      stream, p, g, acc, n, lr, momentum, grad_scale, l2, l2_mask, partials,
      clip_norm, ema, ema_decay, norm_out);
}

int wn_rmsprop_clip(float* p, const float* g, float* ms, float* mom, long n,
                    float lr, float decay, float momentum, float eps,
                    float grad_scale, float l2, const float* l2_mask,
                    const double* partials, int nparts, float clip_norm,
                    float* ema, float ema_decay, float* norm_out,
                    void* stream) {
  return optim_launch(
      rmsprop_clip_kernel, p && g && ms && mom, n,
      clip_args_check(partials, nparts, clip_norm, ema, ema_decay, norm_out),
      stream, p, g, ms, mom, n, lr, decay, momentum, eps, grad_scale, l2,
      l2_mask, partials, clip_norm, ema, ema_decay, norm_out);
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

int wn_l2_partials_count(void) { return 256; }

int wn_l2_partials(const float* p, long n, const float* mask, float* partials,
                   void* stream) {
  if (!p || !partials) return WN_ERR_NULL;
  if (n <= 0) return WN_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(l2_partials_kernel, dim3(256), dim3(256), 0,
                     (hipStream_t)stream, p, n, mask, partials);
  return wn_check_launch();
}

}  // extern "C"
