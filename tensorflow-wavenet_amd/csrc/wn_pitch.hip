// Pitch tracker (include/wavenet_pitch.h states the rule and the summation
// orders; wavenet/pitch.py restates it in numpy, tests/pitch_ref.py in
// float64): F0, aperiodicity and lag per frame of the local-conditioning grid,
// YIN's cumulative-mean-normalised difference in its direct form.
//
// One workgroup of 256 lanes owns one frame.  LDS, in floats:
//   ys   [NS]      y shifted by three: ys[i + 3] = y[i], zeros around, so that
//                  y[j + 4 g + 1] with j % 4 == 0 is 16-byte aligned
//   ya   [W]       y[0 .. W), aligned: the broadcast operand
//   part [8][G4]   segment sums q_k[tau] at [k][tau - 1]; afterwards
//                  [0][..] d, [2..3][..] S as doubles, [4..][..] c'
//   red  [16]      the waves' partial results
// A work unit (k, g) = segment k of W / 8 values of j, lags 4 g + 1 .. 4 g + 4;
// unit u = k * groups + g goes to lane u % 256, so a wave's lanes share j (a
// broadcast read of ya) and read consecutive 32 bytes of ys.  Per four j a lane
// issues three ds_read_b128 for 16 subtract + fma pairs.
#include "wn_common.h"

#define PITCH_THREADS 256
#define PITCH_SEGS 8
#define PITCH_MAX_W 2048
#define PITCH_MAX_TAU 1024
#define PITCH_MAX_HOP 4096
#define PITCH_NONE 0x7fffffff

struct PitchArgs {
  const float* audio;
  const int32_t* lengths;
  long ld;
  float* f0;
  float* aper;
  int32_t* lag;
  float* cmnd;
  int T, F, hop, W, tau_min, tau_max, NS, G4;
  float threshold, silence, sr;
};

__device__ __forceinline__ float pitch_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(PITCH_THREADS) void pitch_track_kernel(PitchArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float pitch_lds[];
  float* ys = pitch_lds;
  float* ya = ys + a.NS;
  float* part = ya + a.W;
  float* red = part + PITCH_SEGS * a.G4;
  int* redi = reinterpret_cast<int*>(red);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, f = blockIdx.x;
  const int W = a.W, tmax = a.tau_max, N = W + tmax, G4 = a.G4;
  int n = a.lengths ? a.lengths[b] : a.T;
  n = n < 0 ? 0 : (n > a.T ? a.T : n);
  const int nF = (n + a.hop - 1) / a.hop;       // the clip's real frames
  const long o = (long)b * a.F + f;
  float* crow = a.cmnd ? a.cmnd + o * (tmax + 1) : nullptr;

  if (f >= nF) {                                // (workgroup-uniform)
    if (tid == 0) {
      a.f0[o] = 0.f;
      a.aper[o] = 0.f;
      a.lag[o] = 0;
    }
    if (crow)
      for (int t = tid; t <= tmax; t += PITCH_THREADS) crow[t] = 0.f;
    return;
  }

  // ---- stage y (zeros outside the clip and in the pad)
  const float* clip = a.audio + (long)b * a.ld;
  const long s0 = (long)f * a.hop + a.hop / 2 - N / 2;
  for (int i = tid; i < a.NS; i += PITCH_THREADS) {
    const int j = i - 3;
    const long g = s0 + j;
    float v = 0.f;
    if (j >= 0 && j < N && g >= 0 && g < n) v = clip[g];
    ys[i] = v;
    if (j >= 0 && j < W) ya[j] = v;
  }
  __syncthreads();

  // ---- 1. the energy of y[0 .. W)
  {
    float p = 0.f;
    for (int j = tid; j < W; j += PITCH_THREADS) p = __builtin_fmaf(ya[j], ya[j], p);
    p = pitch_wave_sum(p);
    if (lane == 0) red[wave] = p;
  }
  __syncthreads();
  const float e = ((red[0] + red[1]) + red[2]) + red[3];
  if (e <= a.silence * (float)W) {              // (workgroup-uniform)
    if (tid == 0) {
      a.f0[o] = 0.f;
      a.aper[o] = 1.f;
      a.lag[o] = 0;
    }
    if (crow)
      for (int t = tid; t <= tmax; t += PITCH_THREADS) crow[t] = 1.f;
    return;
  }

  // ---- 2. the segment sums of the difference function
  const int groups = G4 >> 2, seg = W / PITCH_SEGS;
  const f32x4* ya4 = reinterpret_cast<const f32x4*>(ya);
  const f32x4* ys4 = reinterpret_cast<const f32x4*>(ys);
  for (int u = tid; u < PITCH_SEGS * groups; u += PITCH_THREADS) {
    const int k = u / groups, g = u - k * groups;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int j0 = k * seg;
    // (ys index of y[j + 4 g + 1] is j + 4 g + 4)
    for (int j = j0; j < j0 + seg; j += 4) {
      const f32x4 x = ya4[j >> 2];
      const f32x4 lo = ys4[(j >> 2) + g + 1];
      const f32x4 hi = ys4[(j >> 2) + g + 2];
      const float w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          const float v = x[jj] - w[jj + l];
          acc[l] = __builtin_fmaf(v, v, acc[l]);
        }
    }
    *reinterpret_cast<f32x4*>(part + k * G4 + 4 * g) = acc;
  }
  __syncthreads();
  for (int i = tid; i < tmax; i += PITCH_THREADS) {
    float d = part[i];
#pragma unroll
    for (int k = 1; k < PITCH_SEGS; ++k) d = d + part[k * G4 + i];
    part[i] = d;                                // d[i + 1]
  }
  __syncthreads();

  // ---- 3. the float64 prefix (sequential), then c' by all lanes
  double* S = reinterpret_cast<double*>(part + 2 * G4);   // S[tau] at [tau - 1]
  float* cm = part + 4 * G4;                              // c'[0 .. tau_max]
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < G4; i += 4) {
      const f32x4 d = *reinterpret_cast<const f32x4*>(part + i);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (i + q < tmax) {
          s += (double)d[q];
          S[i + q] = s;
        }
    }
  }
  __syncthreads();
  for (int t = tid; t <= tmax; t += PITCH_THREADS) {
    float c = 1.f;
    if (t > 0) {
      const double s = S[t - 1];
      if (s > 0.0) c = (float)((double)part[t - 1] * (double)t / s);
    }
    cm[t] = c;
    if (crow) crow[t] = c;
  }
  __syncthreads();

  // ---- 4. the pick: the first lag under the threshold, and the minimum
  int first = PITCH_NONE, besti = PITCH_NONE;
  float bestv = INFINITY;
  for (int t = a.tau_min + tid; t <= tmax - 1; t += PITCH_THREADS) {
    const float c = cm[t];
    if (c < a.threshold && first == PITCH_NONE) first = t;
    if (c < bestv) {
      bestv = c;
      besti = t;
    }
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const int of = __shfl_xor(first, m, 64);
    const int oi = __shfl_xor(besti, m, 64);
    const float ov = __shfl_xor(bestv, m, 64);
    first = of < first ? of : first;
    if (ov < bestv || (ov == bestv && oi < besti)) {
      bestv = ov;
      besti = oi;
    }
  }
  if (lane == 0) {
    redi[4 + wave] = first;
    red[8 + wave] = bestv;
    redi[12 + wave] = besti;
  }
  __syncthreads();
  if (tid == 0) {
    first = redi[4];
    bestv = red[8];
    besti = redi[12];
    for (int w = 1; w < PITCH_THREADS / 64; ++w) {
      const int of = redi[4 + w], oi = redi[12 + w];
      const float ov = red[8 + w];
      first = of < first ? of : first;
      if (ov < bestv || (ov == bestv && oi < besti)) {
        bestv = ov;
        besti = oi;
      }
    }
    int tau;
    float f0 = 0.f;
    if (first != PITCH_NONE) {
      tau = first;
      while (tau + 1 <= tmax - 1 && cm[tau + 1] < cm[tau]) ++tau;
      // ---- 5. parabolic interpolation
      const float ca = cm[tau - 1], cb = cm[tau], cg = cm[tau + 1];
      const float den = (ca - 2.f * cb) + cg;
      float delta = 0.f;
      if (den > 0.f) {
        delta = 0.5f * (ca - cg) / den;
        delta = delta < -0.5f ? -0.5f : (delta > 0.5f ? 0.5f : delta);
      }
      f0 = a.sr / ((float)tau + delta);
    } else {
      // (no value compared below infinity: NaNs only; any lag of the range)
      tau = besti == PITCH_NONE ? a.tau_min : besti;
    }
    a.f0[o] = f0;
    a.aper[o] = cm[tau];
    a.lag[o] = tau;
  }
}

static bool pitch_settings_ok(int hop, int window, int tau_max) {
  return hop >= 1 && hop <= PITCH_MAX_HOP && window >= 64 &&
         window <= PITCH_MAX_W && window % 64 == 0 && tau_max >= 4 &&
         tau_max <= PITCH_MAX_TAU;
}

static long pitch_lds_floats(int window, int tau_max, int* NS, int* G4) {
  *NS = (window + tau_max + 8 + 3) / 4 * 4;
  *G4 = (tau_max + 3) / 4 * 4;
  return (long)*NS + window + (long)PITCH_SEGS * *G4 + 16;
}

extern "C" {

int wn_pitch_tau_min(float sample_rate, float fmax) {
  if (!(sample_rate > 0.f) || !(fmax > 0.f) || !(sample_rate < INFINITY) ||
      !(fmax < INFINITY))
    return -1;
  const double t = floor((double)sample_rate / (double)fmax);
  if (t > 1073741824.0) return -1;
  return t < 2.0 ? 2 : (int)t;
}

int wn_pitch_tau_max(float sample_rate, float fmin) {
  if (!(sample_rate > 0.f) || !(fmin > 0.f) || !(sample_rate < INFINITY) ||
      !(fmin < INFINITY))
    return -1;
  const double t = ceil((double)sample_rate / (double)fmin);
  if (t > 1073741824.0) return -1;
  return (int)t;
}

long wn_pitch_lds_bytes(int window, int tau_max, int hop) {
  if (!pitch_settings_ok(hop, window, tau_max)) return -1;
  int NS, G4;
  return 4L * pitch_lds_floats(window, tau_max, &NS, &G4);
}

int wn_pitch_track(const float* audio, const int32_t* lengths, long ld, int B,
                   int T, int hop, int window, int tau_min, int tau_max,
                   float threshold, float silence, float sample_rate,
                   float* f0, float* aper, int32_t* lag, float* cmnd,
                   void* stream) {
  if (!audio || !f0 || !aper || !lag) return WN_ERR_NULL;
  if (!pitch_settings_ok(hop, window, tau_max) || tau_min < 2 ||
      tau_min + 2 > tau_max || !(threshold > 0.f) || !(threshold < 1.f) ||
      !(silence >= 0.f) || !(silence < INFINITY) || !(sample_rate > 0.f) ||
      !(sample_rate < INFINITY) || B < 1 || B > 65535 || T < 1 ||
      T > (1 << 30) || ld < T)
    return WN_ERR_BAD_SHAPE;
  if ((reinterpret_cast<uintptr_t>(audio) & 3u) ||
      (reinterpret_cast<uintptr_t>(lengths) & 3u) ||
      (reinterpret_cast<uintptr_t>(f0) & 3u) ||
      (reinterpret_cast<uintptr_t>(aper) & 3u) ||
      (reinterpret_cast<uintptr_t>(lag) & 3u) ||
      (reinterpret_cast<uintptr_t>(cmnd) & 3u))
    return WN_ERR_MISALIGNED;
  PitchArgs a;
  a.audio = audio;
  a.lengths = lengths;
  a.ld = ld;
  a.f0 = f0;
  a.aper = aper;
  a.lag = lag;
  a.cmnd = cmnd;
  a.T = T;
  a.F = (T + hop - 1) / hop;
  a.hop = hop;
  a.W = window;
  a.tau_min = tau_min;
  a.tau_max = tau_max;
  a.threshold = threshold;
  a.silence = silence;
  a.sr = sample_rate;
  const size_t lds = 4 * (size_t)pitch_lds_floats(window, tau_max, &a.NS, &a.G4);
  if (hipFuncSetAttribute((const void*)pitch_track_kernel,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return WN_ERR_LAUNCH;
  hipLaunchKernelGGL(pitch_track_kernel, dim3((unsigned)a.F, (unsigned)B),
                     dim3(PITCH_THREADS), lds, (hipStream_t)stream, a);
  return wn_check_launch();
}

}  // extern "C"
