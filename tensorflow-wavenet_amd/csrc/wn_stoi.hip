// STOI and ESTOI of clip pairs at 10 kHz (include/wavenet_stoi.h states the
// rule; wavenet/stoi.py's Stoi.reference restates it in numpy, tests/
// stoi_ref.py in float64).  Four launches:
//
// * stoi_frames_kernel: a workgroup per clip.  Thread t computes the energies
//   of the frames t, t + 256, ... of the original (the serial 256-term sum of
//   the rule), the workgroup takes their maximum, and the keep flags are
//   scanned 256 frames at a time (ballot and popcount inside a wave, the four
//   wave totals through LDS) into the ascending list k_i of kept frames.  Ten
//   minutes of audio are 47 k frames: 184 per thread.
// * stoi_bands_kernel: a workgroup per kept frame i.  Lane j forms sample j of
//   compacted frame i of both signals from the frames k_{i-1}, k_i, k_{i+1}
//   (the compacted signals never exist in memory), bin k = 7 + t of the 212
//   bins the bands cover runs its DFT on thread t over the windowed frame in
//   LDS, and 15 threads add the bands.  The DFT is the plain one of the rule,
//   not wn_stft's MFMA path: 2 x 212 x 256 complex terms per frame, 10 G
//   multiply-adds for ten minutes.  The frame samples are read as broadcasts;
//   the twiddles cos | sin[(k j) mod 512] of a 32-lane half fall on (k j) mod 32
//   banks, gcd(j, 32) lanes per bank with different words: 3.5-way on the
//   average over j.  tools/stoi_time.py measures what that costs.
// * stoi_segments_kernel: a wave per segment, frame m of the 30 on lane m, in
//   float64: a band's 30 amplitudes of both signals sit one per lane, every
//   sum over frames is one DPP prefix network (wave_scan_f64), and the ESTOI
//   columns are serial in each lane over its 15 row-normalised values.
// * stoi_sum_kernel: a workgroup per clip adds the segments' values in the
//   stated order.
#include "wn_common.h"

#define STOI_FRAME 256
#define STOI_HOP 128
#define STOI_NFFT 512
#define STOI_BANDS 15
#define STOI_SEG 30
#define STOI_EDGES {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219}
#define STOI_BIN0 7
#define STOI_NBINS 212          // bins 7 .. 218
#define STOI_CLIP 5.623413251903491   // 10^(15/20)
#define STOI_EPS 2.220446049250313e-16  // 2^-52

static const int stoi_edges_host[STOI_BANDS + 1] = STOI_EDGES;
__constant__ int stoi_edges[STOI_BANDS + 1] = STOI_EDGES;

static inline long stoi_frames_of(long n) {
  return n < STOI_FRAME ? 0 : (n - STOI_FRAME) / STOI_HOP + 1;
}

struct StoiArgs {
  const float* gen;
  const float* org;
  const int32_t* lengths;
  const float* window;
  const float* basis;
  long ld_gen, ld_org;
  int T, Fm, Sm;              // Fm, Sm: frames and segments of T, at least 1
  float* E;                   // [B][Fm]
  int32_t* kidx;              // [B][Fm]
  float* bx;                  // [B][Fm][15], the original's amplitudes
  float* by;                  // the generated signal's
  double* segv;               // [B][Sm][2]
  double* stoi_sum;
  double* estoi_sum;
  int32_t* segments;
  int32_t* kept;
};

__device__ __forceinline__ int stoi_len(const int32_t* lengths, int b, int T) {
  int n = T;
  if (lengths) {
    n = lengths[b];
    n = n < 0 ? 0 : (n > T ? T : n);
  }
  return n;
}

__global__ __launch_bounds__(256) void stoi_frames_kernel(StoiArgs a) {
#pragma clang fp contract(off)
  __shared__ float w[STOI_FRAME];
  __shared__ float red[256];
  __shared__ int wt[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = stoi_len(a.lengths, b, a.T);
  const int Fs = n < STOI_FRAME ? 0 : (n - STOI_FRAME) / STOI_HOP + 1;
  const float* x = a.org + (long)b * a.ld_org;
  float* E = a.E + (long)b * a.Fm;
  int32_t* kidx = a.kidx + (long)b * a.Fm;
  w[tid] = a.window[tid];
  __syncthreads();
  float mx = 0.f;
  for (int f = tid; f < Fs; f += 256) {         // f < Fs: 128 f + 255 < n
    const float* xf = x + (long)STOI_HOP * f;
    float e = 0.f;
    for (int i = 0; i < STOI_FRAME; ++i) {
      const float p = w[i] * xf[i];
      const float q = p * p;
      e = e + q;
    }
    E[f] = e;
    mx = fmaxf(mx, e);                          // (passes over a NaN)
  }
  red[tid] = mx;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  const float thr = red[0] * 1e-4f;
  const int lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int f0 = 0; f0 < Fs; f0 += 256) {        // (workgroup-uniform)
    const int f = f0 + tid;
    const bool keep = f < Fs && E[f] > thr;     // (this thread wrote E[f])
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wt[wave] = __popcll(bal);
    __syncthreads();
    int off = base, total = 0;
    for (int v = 0; v < 4; ++v) {
      if (v < wave) off += wt[v];
      total += wt[v];
    }
    if (keep) kidx[off + __popcll(bal & ((1ull << lane) - 1ull))] = f;
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    a.kept[b] = base;
    a.segments[b] = base >= STOI_SEG ? base - (STOI_SEG - 1) : 0;
  }
}

// sample j of compacted frame i of the signal s (kc = k_i; kp = k_{i-1} or -1;
// kn = k_{i+1} or -1)
__device__ __forceinline__ float stoi_compact(const float* __restrict__ s, const float* w, int j,
                                              int kp, int kc, int kn) {
#pragma clang fp contract(off)
  float v = 0.f;
  if (j < STOI_HOP) {
    if (kp >= 0) v = v + w[j + STOI_HOP] * s[(long)STOI_HOP * kp + j + STOI_HOP];
    v = v + w[j] * s[(long)STOI_HOP * kc + j];
  } else {
    v = v + w[j] * s[(long)STOI_HOP * kc + j];
    if (kn >= 0) v = v + w[j - STOI_HOP] * s[(long)STOI_HOP * kn + j - STOI_HOP];
  }
  return v * w[j];
}

__global__ __launch_bounds__(256) void stoi_bands_kernel(StoiArgs a) {
#pragma clang fp contract(off)
  __shared__ float w[STOI_FRAME];
  __shared__ float cs[STOI_NFFT], sn[STOI_NFFT];
  __shared__ float fx[STOI_FRAME], fy[STOI_FRAME];
  __shared__ float px[STOI_NBINS], py[STOI_NBINS];
  const int b = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
  const int M = a.kept[b];
  if (i >= M) return;                           // (workgroup-uniform)
  const int32_t* kidx = a.kidx + (long)b * a.Fm;
  w[tid] = a.window[tid];
  cs[tid] = a.basis[tid];
  cs[tid + 256] = a.basis[tid + 256];
  sn[tid] = a.basis[STOI_NFFT + tid];
  sn[tid + 256] = a.basis[STOI_NFFT + tid + 256];
  __syncthreads();
  const int kc = kidx[i];
  const int kp = i >= 1 ? kidx[i - 1] : -1;
  const int kn = i + 1 < M ? kidx[i + 1] : -1;
  fx[tid] = stoi_compact(a.org + (long)b * a.ld_org, w, tid, kp, kc, kn);
  fy[tid] = stoi_compact(a.gen + (long)b * a.ld_gen, w, tid, kp, kc, kn);
  __syncthreads();
  if (tid < STOI_NBINS) {
    const int k = STOI_BIN0 + tid;
    float xr = 0.f, xi = 0.f, yr = 0.f, yi = 0.f;
    for (int j = 0; j < STOI_FRAME; ++j) {
      const int q = (k * j) & (STOI_NFFT - 1);
      const float c = cs[q], s = sn[q], vx = fx[j], vy = fy[j];
      xr = xr + c * vx;
      xi = xi + s * vx;
      yr = yr + c * vy;
      yi = yi + s * vy;
    }
    px[tid] = xr * xr + xi * xi;
    py[tid] = yr * yr + yi * yi;
  }
  __syncthreads();
  if (tid < STOI_BANDS) {
    float sx = 0.f, sy = 0.f;
    for (int k = stoi_edges[tid]; k < stoi_edges[tid + 1]; ++k) {
      sx = sx + px[k - STOI_BIN0];
      sy = sy + py[k - STOI_BIN0];
    }
    const long o = ((long)b * a.Fm + i) * STOI_BANDS + tid;
    a.bx[o] = sqrtf(sx);
    a.by[o] = sqrtf(sy);
  }
}

// the sum of x over the wave's lanes, the same value in every lane (all 64
// lanes must be executing)
__device__ __forceinline__ double stoi_wsum(double x) {
  return readlane_f64(wave_scan_f64(x), 63);
}

__global__ __launch_bounds__(256) void stoi_segments_kernel(StoiArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= a.segments[b]) return;               // (wave-uniform; no barrier below)
  const bool real = lane < STOI_SEG;
  const long o = ((long)b * a.Fm + s + (real ? lane : 0)) * STOI_BANDS;
  const double eps = STOI_EPS, inv_n = 1.0 / STOI_SEG;
  double rx[STOI_BANDS], ry[STOI_BANDS];        // the row-normalised blocks
  double dsum = 0.0;
#pragma unroll
  for (int q = 0; q < STOI_BANDS; ++q) {
    const double x = real ? (double)a.bx[o + q] : 0.0;
    const double y = real ? (double)a.by[o + q] : 0.0;
    const double alpha = sqrt(stoi_wsum(x * x)) / (sqrt(stoi_wsum(y * y)) + eps);
    const double yc = fmin(alpha * y, (1.0 + STOI_CLIP) * x);
    const double mx = stoi_wsum(x) * inv_n, myc = stoi_wsum(yc) * inv_n, my = stoi_wsum(y) * inv_n;
    const double x0 = real ? x - mx : 0.0;
    const double c0 = real ? yc - myc : 0.0;
    const double y0 = real ? y - my : 0.0;
    const double xn = x0 / (sqrt(stoi_wsum(x0 * x0)) + eps);
    const double cn = c0 / (sqrt(stoi_wsum(c0 * c0)) + eps);
    dsum = dsum + stoi_wsum(xn * cn);
    rx[q] = xn;
    ry[q] = y0 / (sqrt(stoi_wsum(y0 * y0)) + eps);
  }
  // this lane's column: zero-mean over the bands, unit norm
  double cmx = 0.0, cmy = 0.0;
#pragma unroll
  for (int q = 0; q < STOI_BANDS; ++q) {
    cmx = cmx + rx[q];
    cmy = cmy + ry[q];
  }
  cmx = cmx / STOI_BANDS;
  cmy = cmy / STOI_BANDS;
  double nx = 0.0, ny = 0.0;
#pragma unroll
  for (int q = 0; q < STOI_BANDS; ++q) {
    rx[q] = rx[q] - cmx;
    ry[q] = ry[q] - cmy;
    nx = nx + rx[q] * rx[q];
    ny = ny + ry[q] * ry[q];
  }
  nx = sqrt(nx) + eps;
  ny = sqrt(ny) + eps;
  double e = 0.0;
#pragma unroll
  for (int q = 0; q < STOI_BANDS; ++q) e = e + (rx[q] / nx) * (ry[q] / ny);
  const double es = stoi_wsum(real ? e : 0.0);
  if (lane == 0) {
    double* v = a.segv + ((long)b * a.Sm + s) * 2;
    v[0] = dsum / STOI_BANDS;
    v[1] = es * inv_n;
  }
}

__global__ __launch_bounds__(256) void stoi_sum_kernel(StoiArgs a) {
#pragma clang fp contract(off)
  __shared__ double ps[256], pe[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int S = a.segments[b];
  const double* v = a.segv + (long)b * a.Sm * 2;
  double s0 = 0.0, s1 = 0.0;
  for (int s = tid; s < S; s += 256) {
    s0 = s0 + v[2 * (long)s];
    s1 = s1 + v[2 * (long)s + 1];
  }
  ps[tid] = s0;
  pe[tid] = s1;
  __syncthreads();
  if (tid == 0) {
    double t0 = 0.0, t1 = 0.0;
    for (int t = 0; t < 256; ++t) {
      t0 = t0 + ps[t];
      t1 = t1 + pe[t];
    }
    a.stoi_sum[b] = t0;
    a.estoi_sum[b] = t1;
  }
}

static inline bool stoi_mis(const void* p, uintptr_t mask) {
  return (reinterpret_cast<uintptr_t>(p) & mask) != 0;
}

extern "C" {

int wn_stoi_band_edge(int i) {
  return i >= 0 && i <= STOI_BANDS ? stoi_edges_host[i] : -1;
}

long wn_stoi_scratch_bytes(int B, int T) {
  if (B < 1 || B > 65535 || T < 1 || T > (1 << 30)) return WN_ERR_BAD_SHAPE;
  const long F = stoi_frames_of(T), Fm = F > 0 ? F : 1;
  const long S = F >= STOI_SEG ? F - (STOI_SEG - 1) : 0, Sm = S > 0 ? S : 1;
  return 16L * B * Sm + 4L * B * Fm * (2 + 2 * STOI_BANDS);
}

int wn_stoi(const float* gen, long ld_gen, const float* org, long ld_org,
            const int32_t* lengths, int B, int T, const float* window,
            const float* basis, void* scratch, double* stoi_sum,
            double* estoi_sum, int32_t* segments, int32_t* kept, void* stream) {
  if (!gen || !org || !window || !basis || !scratch || !stoi_sum || !estoi_sum || !segments ||
      !kept)
    return WN_ERR_NULL;
  if (B < 1 || B > 65535 || T < 1 || T > (1 << 30) || ld_gen < T || ld_org < T)
    return WN_ERR_BAD_SHAPE;
  if (stoi_mis(gen, 3u) || stoi_mis(org, 3u) || stoi_mis(lengths, 3u) || stoi_mis(window, 3u) ||
      stoi_mis(basis, 3u) || stoi_mis(segments, 3u) || stoi_mis(kept, 3u) ||
      stoi_mis(scratch, 7u) || stoi_mis(stoi_sum, 7u) || stoi_mis(estoi_sum, 7u))
    return WN_ERR_MISALIGNED;
  const long F = stoi_frames_of(T), Fm = F > 0 ? F : 1;
  const long S = F >= STOI_SEG ? F - (STOI_SEG - 1) : 0, Sm = S > 0 ? S : 1;
  StoiArgs a;
  a.gen = gen; a.org = org; a.lengths = lengths; a.window = window; a.basis = basis;
  a.ld_gen = ld_gen; a.ld_org = ld_org;
  a.T = T; a.Fm = (int)Fm; a.Sm = (int)Sm;
  char* p = static_cast<char*>(scratch);
  a.segv = reinterpret_cast<double*>(p);
  p += 16L * B * Sm;
  a.E = reinterpret_cast<float*>(p);
  p += 4L * B * Fm;
  a.kidx = reinterpret_cast<int32_t*>(p);
  p += 4L * B * Fm;
  a.bx = reinterpret_cast<float*>(p);
  p += 4L * B * Fm * STOI_BANDS;
  a.by = reinterpret_cast<float*>(p);
  a.stoi_sum = stoi_sum; a.estoi_sum = estoi_sum; a.segments = segments; a.kept = kept;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(stoi_frames_kernel, dim3((unsigned)B), dim3(256), 0, st, a);
  if (F > 0)
    hipLaunchKernelGGL(stoi_bands_kernel, dim3((unsigned)F, (unsigned)B), dim3(256), 0, st, a);
  if (S > 0)
    hipLaunchKernelGGL(stoi_segments_kernel, dim3((unsigned)((S + 3) / 4), (unsigned)B),
                       dim3(256), 0, st, a);
  hipLaunchKernelGGL(stoi_sum_kernel, dim3((unsigned)B), dim3(256), 0, st, a);
  return wn_check_launch();
}

}  // extern "C"
