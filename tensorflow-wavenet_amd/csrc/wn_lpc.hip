// Linear prediction (include/wavenet_lpc.h states the rules; wavenet/lpc.py's
// LinearPrediction.reference_* restate them in numpy, tests/lpc_ref.py in
// float64): predictor coefficients from raw log-mel frames, the parallel
// analysis filter and the serial all-pole synthesis filter.
//
// * lpc_from_mel_kernel: a workgroup per frame.  Lanes run over the bins for
//   P (wn_mel_to_magnitude's arithmetic, the table transposed so that a wave
//   reads whole rows), lane (q, i) sums the bins q, q + 8, ... of lag i in
//   float64, and wave 0 runs the recursion with a[j] and r[j] on lane j: the
//   products of a step in parallel, their sum in the stated order through
//   v_readlane, no LDS round trip per term.
// * lpc_analysis_kernel: a workgroup per LPC_TILE samples of one clip; the
//   tile, LPC_HALO samples in front of it and the coefficient rows of the
//   frames it touches are staged in LDS (the rows are read from memory where
//   more than LPC_CS floats of them would be needed: hops of a few samples).
// * lpc_synthesis_kernel: strictly serial in the sample index, so one wave
//   walks one clip and what counts is the time per sample.  Lane i - 1 owns
//   the state s_i of the transposed direct form; per sample the chain is one
//   v_readfirstlane (s_1), one add (y), one multiply and one DPP-shifted add.
//   A frame's coefficients are loaded one frame ahead of their use; the
//   excitation is loaded, and the result stored, 64 samples at a time.
#include "wn_common.h"

#define LPC_MAX_ORDER 32
#define LPC_MAX_MELS 128
#define LPC_MAX_BINS 1025
#define LPC_MAX_HOP 4096
#define LPC_TILE 1024
#define LPC_HALO 32
#define LPC_CS 8192

// ---------------------------------------------------------------------------
// Coefficients from raw log-mel frames.
// ---------------------------------------------------------------------------
#define LPC_PARTS 8   // interleaved partial sums of the autocorrelation

__device__ __forceinline__ double lpc_shfl(double x, int src) {
  const long long v = __double_as_longlong(x);
  const int lo = __shfl((int)v, src, 64), hi = __shfl((int)(v >> 32), src, 64);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__global__ __launch_bounds__(256) void lpc_from_mel_kernel(
    const float* __restrict__ frames, int F, int n_mels, const int32_t* __restrict__ nframes,
    const float* __restrict__ pinv_t, int n_bins, const double* __restrict__ ctab,
    const double* __restrict__ lagwin, int order, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float M[LPC_MAX_MELS];
  __shared__ float Ps[LPC_MAX_BINS];
  __shared__ double part[LPC_PARTS][LPC_MAX_ORDER + 1];
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  int nf = F;
  if (nframes) {
    nf = nframes[b];
    nf = nf < 0 ? 0 : (nf > F ? F : nf);
  }
  for (int f = blockIdx.x; f < F; f += gridDim.x) {   // (workgroup-uniform)
    float* o = out + ((long)b * F + f) * order;
    if (f >= nf) {
      if (tid < order) o[tid] = 0.f;
      continue;
    }
    __syncthreads();                          // (the previous frame's LDS is read)
    if (tid < n_mels) M[tid] = expf(frames[((long)b * F + f) * n_mels + tid]);
    __syncthreads();
    for (int k = tid; k < n_bins; k += 256) {   // (lanes over the bins: coalesced rows)
      float p = 0.f;
      for (int m = 0; m < n_mels; ++m) p += pinv_t[(long)m * n_bins + k] * M[m];
      Ps[k] = p < 0.f ? 0.f : p;              // (a NaN passes)
    }
    __syncthreads();
    // partial sum q of lag i: the bins q, q + 8, ... ascending
    for (int idx = tid; idx < LPC_PARTS * (order + 1); idx += 256) {
      const int q = idx / (order + 1), i = idx - q * (order + 1);
      double acc = 0.0;
      for (int k = q; k < n_bins; k += LPC_PARTS)
        acc = acc + ctab[(long)k * (order + 1) + i] * (double)Ps[k];
      part[q][i] = acc;
    }
    __syncthreads();
    if (tid < 64) {                           // wave 0: lane j owns r[j] and a[j]
      const int lane = tid;
      double r = 0.0;
      if (lane <= order) {
        r = part[0][lane];
        for (int q = 1; q < LPC_PARTS; ++q) r = r + part[q][lane];
        r = r * lagwin[lane];
      }
      const double r0 = readlane_f64(r, 0);
      double a = 0.0;                         // a[lane]; a[0] is never read
      if (r0 > 1e-30) {                       // (wave-uniform)
        double err = r0;
        for (int i = 1; i <= order; ++i) {
          // lane j, 1 <= j < i: a[j] * r[i - j] and a[i - j]
          const int src = (i - lane) & 63;
          const double rr = lpc_shfl(r, src), ar = lpc_shfl(a, src);
          const double pr = a * rr;
          double acc = readlane_f64(r, i);
          for (int j = 1; j < i; ++j) acc = acc + readlane_f64(pr, j);
          const double k = -acc / err;
          if (!(fabs(k) < 1.0)) break;
          const double up = a + k * ar;
          a = (lane >= 1 && lane < i) ? up : (lane == i ? k : a);
          err = err * (1.0 - k * k);
        }
      }
      if (lane >= 1 && lane <= order) o[lane - 1] = (float)(-a);
    }
  }
}

// ---------------------------------------------------------------------------
// Analysis: e[t] = (x[t] - sum_i c[f(t - i)][i - 1] x[t - i]) * gain.
// ---------------------------------------------------------------------------
struct LpcArgs {
  const float* in;
  const float* coeffs;
  const int32_t* lengths;
  float* out;
  long ld_in, ld_out;
  int F, order, hop, T;
  float g;
  int vin, vout;
};

__device__ __forceinline__ int lpc_len(const int32_t* lengths, int b, int T) {
  int n = T;
  if (lengths) {
    n = lengths[b];
    n = n < 0 ? 0 : (n > T ? T : n);
  }
  return n;
}

__global__ __launch_bounds__(256) void lpc_analysis_kernel(LpcArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float xs[LPC_HALO + LPC_TILE];
  __shared__ __attribute__((aligned(16))) float es[LPC_TILE];
  __shared__ float cs[LPC_CS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int t0 = blockIdx.x * LPC_TILE;
  const int n = lpc_len(a.lengths, b, a.T);
  const float* x = a.in + (long)b * a.ld_in;
  float* e = a.out + (long)b * a.ld_out;
  const int order = a.order, hop = a.hop;
  int m = n - t0;                               // real samples of the tile
  m = m < 0 ? 0 : (m > LPC_TILE ? LPC_TILE : m);
  int f_lo = 0, nfr = 0;
  bool staged = false;
  if (m > 0) {                                  // (workgroup-uniform)
    if (tid < LPC_HALO) {
      const int t = t0 - LPC_HALO + tid;
      xs[tid] = t >= 0 ? x[t] : 0.f;
    }
    for (int v = tid; v < LPC_TILE / 4; v += 256) {
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      if (a.vin && 4 * v + 3 < m) {
        q = *reinterpret_cast<const float4*>(x + t0 + 4 * v);
      } else {
        if (4 * v + 0 < m) q.x = x[t0 + 4 * v + 0];
        if (4 * v + 1 < m) q.y = x[t0 + 4 * v + 1];
        if (4 * v + 2 < m) q.z = x[t0 + 4 * v + 2];
        if (4 * v + 3 < m) q.w = x[t0 + 4 * v + 3];
      }
      *reinterpret_cast<float4*>(xs + LPC_HALO + 4 * v) = q;
    }
    // the frames of the samples t0 - order .. t0 + m - 2 that exist
    const int u_hi = t0 + m - 2;
    if (u_hi >= 0) {
      const int u_lo = t0 - order < 0 ? 0 : t0 - order;
      f_lo = u_lo / hop;
      nfr = u_hi / hop - f_lo + 1;
      staged = (long)nfr * order <= LPC_CS;
    }
    if (staged) {
      const float* cf = a.coeffs + (long)b * a.F * order;
      for (int idx = tid; idx < nfr * order; idx += 256) {
        int fr = f_lo + idx / order;
        fr = fr < a.F ? fr : a.F - 1;
        cs[idx] = cf[(long)fr * order + idx % order];
      }
    }
  }
  __syncthreads();
  if (m > 0) {
    const float* cf = a.coeffs + (long)b * a.F * order;
    for (int q = 0; q < LPC_TILE / 256; ++q) {
      const int j = tid + 256 * q;
      float v = 0.f;
      if (j < m) {
        const int t = t0 + j;
        int i = order < t ? order : t;          // taps with t - i >= 0
        int f = 0, rem = 0;
        if (i > 0) {
          f = (t - i) / hop;
          rem = (t - i) - f * hop;
        }
        float acc = 0.f;
        for (; i >= 1; --i) {
          float c;
          if (staged) {
            c = cs[(f - f_lo) * order + i - 1];
          } else {
            const int fr = f < a.F ? f : a.F - 1;
            c = cf[(long)fr * order + i - 1];
          }
          acc = acc + c * xs[LPC_HALO + j - i];
          if (++rem == hop) {
            rem = 0;
            ++f;
          }
        }
        v = (xs[LPC_HALO + j] - acc) * a.g;
      }
      es[j] = v;
    }
  }
  __syncthreads();
  for (int v = tid; v < LPC_TILE / 4; v += 256) {
    const int t = t0 + 4 * v;
    if (t >= a.T) break;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m > 0) q = *reinterpret_cast<const float4*>(es + 4 * v);
    if (a.vout && t + 3 < a.T) {
      *reinterpret_cast<float4*>(e + t) = q;
    } else {
      e[t] = q.x;
      if (t + 1 < a.T) e[t + 1] = q.y;
      if (t + 2 < a.T) e[t + 2] = q.z;
      if (t + 3 < a.T) e[t + 3] = q.w;
    }
  }
}

// ---------------------------------------------------------------------------
// Synthesis: the transposed direct form, one wave per clip.
// ---------------------------------------------------------------------------
// s_{i+1} as lane i sees it: the lane above's state, +0 for the last lane (and
// for a source lane that is switched off).  Orders up to 16 stay inside one
// 16-lane row (row_shl:1); the wider ones shift across the wave (wave_shl:1).
template <bool WIDE>
__device__ __forceinline__ float lpc_shift(float s) {
  return WIDE ? dpp_f32<0x130, 0xf>(0.f, s) : dpp_f32<0x101, 0xf>(0.f, s);
}

// ALIGNED: hop is a multiple of 64, so a frame edge can only be a chunk's first
// sample and a full chunk runs unrolled under the taps' own execution mask.
template <bool WIDE, bool ALIGNED>
__global__ __launch_bounds__(64) void lpc_synthesis_kernel(LpcArgs a) {
#pragma clang fp contract(off)
  __shared__ float ys[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = lpc_len(a.lengths, b, a.T);
  // (no __restrict__: out may be the excitation itself)
  const float* e = a.in + (long)b * a.ld_in;
  float* y = a.out + (long)b * a.ld_out;
  const int order = a.order, hop = a.hop, F = a.F;
  const float* cf = a.coeffs + (long)b * F * order;
  const bool tap = lane < order;
  float s = 0.f;                                // s_{lane + 1}
  float av = tap ? cf[lane] : 0.f;              // frame 0's row
  float an = tap ? cf[(long)(1 < F ? 1 : F - 1) * order + lane] : 0.f;
  int f = 0, edge = hop;                        // edge: frame f + 1's first sample
  float ev = lane < n ? e[lane] : 0.f;
  for (int t0 = 0; t0 < n; t0 += 64) {          // (wave-uniform)
    const int tn = t0 + 64 + lane;
    const float en = tn < n ? e[tn] : 0.f;      // (read before y[t0 ..] is stored)
    const float eg = ev * a.g;
    const int m = n - t0 < 64 ? n - t0 : 64;
    if (ALIGNED && m == 64) {
      if (t0 == edge) {                         // into frame f + 1, its row on hand
        av = an;
        ++f;
        edge += hop;
        const int fn = f + 1 < F ? f + 1 : F - 1;
        an = tap ? cf[(long)fn * order + lane] : 0.f;
      }
      if (tap) {                                // (lanes >= order keep s = +0)
#pragma unroll
        for (int j = 0; j < 64; ++j) {
          const float et = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(eg), j));
          const float s1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s)));
          const float yt = et + s1;
          const float pr = av * yt;
          s = lpc_shift<WIDE>(s) + pr;
          ys[j] = yt;                           // (every tap lane holds the same yt)
        }
      }
      __syncthreads();
      y[t0 + lane] = ys[lane];
      __syncthreads();
    } else {
      float yo = 0.f;
      for (int j = 0; j < m; ++j) {
        if (t0 + j == edge) {
          av = an;
          ++f;
          edge += hop;
          const int fn = f + 1 < F ? f + 1 : F - 1;
          an = tap ? cf[(long)fn * order + lane] : 0.f;
        }
        const float et = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(eg), j));
        const float s1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s)));
        const float yt = et + s1;
        const float pr = av * yt;
        const float nx = lpc_shift<WIDE>(s) + pr;
        s = tap ? nx : 0.f;
        yo = lane == j ? yt : yo;
      }
      if (lane < m) y[t0 + lane] = yo;
    }
    ev = en;
  }
  for (long t = (long)n + lane; t < a.T; t += 64) y[t] = 0.f;
}

// ---------------------------------------------------------------------------
// Host entry points.
// ---------------------------------------------------------------------------
static inline bool lpc_mis(const void* p, uintptr_t mask) {
  return (reinterpret_cast<uintptr_t>(p) & mask) != 0;
}

extern "C" {

int wn_lpc_from_mel(const float* frames, int B, int F, int n_mels,
                    const int32_t* nframes, const float* pinv_t, int n_bins,
                    const double* ctab, const double* lagwin, int order,
                    float* out, void* stream) {
  if (!frames || !pinv_t || !ctab || !lagwin || !out) return WN_ERR_NULL;
  if (n_mels < 1 || n_mels > LPC_MAX_MELS || n_bins < 2 || n_bins > LPC_MAX_BINS ||
      order < 1 || order > LPC_MAX_ORDER || order > n_bins - 1 || B < 1 || B > 65535 ||
      F < 1 || (long)B * (long)F > 2147483647L)
    return WN_ERR_BAD_SHAPE;
  if (lpc_mis(frames, 3u) || lpc_mis(nframes, 3u) || lpc_mis(pinv_t, 3u) || lpc_mis(out, 3u) ||
      lpc_mis(ctab, 7u) || lpc_mis(lagwin, 7u))
    return WN_ERR_MISALIGNED;
  const unsigned gx = (unsigned)(F < (1 << 20) ? F : (1 << 20));
  hipLaunchKernelGGL(lpc_from_mel_kernel, dim3(gx, (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, frames, F, n_mels, nframes, pinv_t, n_bins, ctab,
                     lagwin, order, out);
  return wn_check_launch();
}

int wn_lpc_analysis_tile(void) { return LPC_TILE; }

static int lpc_filter_check(const float* in, long ld_in, const float* coeffs, int F, int order,
                            int hop, const int32_t* lengths, int B, int T, float g,
                            const float* out, long ld_out, bool alias_ok) {
  if (!in || !coeffs || !out) return WN_ERR_NULL;
  if (order < 1 || order > LPC_MAX_ORDER || hop < 1 || hop > LPC_MAX_HOP || B < 1 ||
      B > 65535 || T < 1 || T > (1 << 30) || F < 1 || ld_in < T || ld_out < T ||
      (long)B * (long)F > 2147483647L || !(g > 0.f) || !(g < INFINITY))
    return WN_ERR_BAD_SHAPE;
  if (!lengths && (long)F * hop < T) return WN_ERR_BAD_SHAPE;
  if (lpc_mis(in, 3u) || lpc_mis(out, 3u) || lpc_mis(coeffs, 3u) || lpc_mis(lengths, 3u))
    return WN_ERR_MISALIGNED;
  if (in == out && !(alias_ok && ld_in == ld_out)) return WN_ERR_BAD_SHAPE;
  return WN_OK;
}

int wn_lpc_analysis(const float* x, long ld_x, const float* coeffs, int F,
                    int order, int hop, const int32_t* lengths, int B, int T,
                    float gain, float* out, long ld_out, void* stream) {
  const int rc = lpc_filter_check(x, ld_x, coeffs, F, order, hop, lengths, B, T, gain, out,
                                  ld_out, false);
  if (rc != WN_OK) return rc;
  LpcArgs a;
  a.in = x; a.coeffs = coeffs; a.lengths = lengths; a.out = out;
  a.ld_in = ld_x; a.ld_out = ld_out;
  a.F = F; a.order = order; a.hop = hop; a.T = T; a.g = gain;
  a.vin = wn_aligned16(x) && ld_x % 4 == 0;
  a.vout = wn_aligned16(out) && ld_out % 4 == 0;
  hipLaunchKernelGGL(lpc_analysis_kernel, dim3((unsigned)((T + LPC_TILE - 1) / LPC_TILE),
                                               (unsigned)B),
                     dim3(256), 0, (hipStream_t)stream, a);
  return wn_check_launch();
}

int wn_lpc_synthesis(const float* e, long ld_e, const float* coeffs, int F,
                     int order, int hop, const int32_t* lengths, int B, int T,
                     float inv_gain, float* out, long ld_out, void* stream) {
  const int rc = lpc_filter_check(e, ld_e, coeffs, F, order, hop, lengths, B, T, inv_gain, out,
                                  ld_out, true);
  if (rc != WN_OK) return rc;
  LpcArgs a;
  a.in = e; a.coeffs = coeffs; a.lengths = lengths; a.out = out;
  a.ld_in = ld_e; a.ld_out = ld_out;
  a.F = F; a.order = order; a.hop = hop; a.T = T; a.g = inv_gain;
  a.vin = a.vout = 0;
  void (*k)(LpcArgs);
  if (hop % 64 == 0)
    k = order > 16 ? lpc_synthesis_kernel<true, true> : lpc_synthesis_kernel<false, true>;
  else
    k = order > 16 ? lpc_synthesis_kernel<true, false> : lpc_synthesis_kernel<false, false>;
  hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, a);
  return wn_check_launch();
}

}  // extern "C"
