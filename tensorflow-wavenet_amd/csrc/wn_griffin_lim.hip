// Griffin-Lim baseline (include/wavenet_griffin_lim.h states every rule and
// summation order; wavenet/griffin_lim.py states them in numpy, tests/gl_ref.py
// restates them in float64): a complex STFT on wn_melspec's frame grid, its
// least-squares inverse, mel -> magnitude inversion, the starting spectrum and
// the fused projection of one Fast Griffin-Lim iteration.
//
// gl_stft_kernel is stft_distance_kernel's shape (wn_spectral.hip) with one
// signal and the phase kept.  One workgroup owns a tile of 32 consecutive
// frames of one clip; the DFT is the fp32 MFMA contraction of the windowed
// frames with the cos | sin basis, bins on the M axis, frames on the N axis.
// The eight waves split the 32-bin chunks (chunk c -> wave c % 8); a wave
// streams its chunk's basis rows through its private LDS ring in pieces of 16
// samples.  The Nyquist bin, whose cos row is (-1)^j, takes the place of bin
// 0's sin row, which is zero.  The samples are read from memory where they are
// used (zeros outside [0, n)).  The epilogue runs on the fragments in
// registers: wn_stft stores (re, -im); wn_gl_project (PROJECT) puts the
// magnitudes A on the phases, adds the momentum step and, with a trace, sums
// the two float64 numbers lanes -> wave -> waves in wave order -> one pair per
// tile; gl_trace_finish_kernel adds a clip's tiles in ascending order.
//
// gl_istft_frames_kernel is the same contraction read the other way: samples
// on the M axis, frames on the N axis, bins on K.  A wave owns chunks of 32
// samples (chunk jc -> wave jc % 8) and walks the n_fft / 64 bin chunks; the
// [32 samples][cos 32 | sin 32] slab of the basis table is one contiguous 8 KiB
// piece, staged in the wave's LDS slab with rows 65 floats apart (the lanes of
// a read walk the rows).  Two accumulators (the cos and the sin half), their
// sum scaled by 2 / n_fft and windowed, go to the scratch; gl_istft_gather_
// kernel adds, per sample, the frames that cover it in ascending order and
// divides by the windows' squares: a gather, no scatter, no atomics.
#include "wn_common.h"

#define GL_TF 32                   // frames per tile
#define GL_WAVES 8
#define GL_KC 16                   // samples per basis piece
#define GL_SLAB (GL_KC * 64)       // floats of a piece: [16][cos 32 | sin 32]
#define GL_RING (GL_WAVES * 2 * GL_SLAB)
#define GL_MAX_FFT 2048
#define GL_ISLAB (32 * 65)         // floats of an inverse slab, rows padded
#define GL_PHASES 1024
#define GL_SEED_XOR 0x6772696666696E4Cull
#define GL_MAX_MELS 128

struct GlsArgs {
  const float* x;
  long ld_x;
  const int32_t* lengths;
  const float* window;
  const float* basis;
  float* out;                      // wn_stft: out; project: c_out
  const float* A;
  const float* t_prev;
  float* t_out;
  double* partials;                // NULL: no trace
  int T, F, n_fft, hop, NC, n_bins, ntiles;
  float alpha;
};

__device__ __forceinline__ double gl_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one (frame, bin) of the projection: reads A and t_prev at `e`, writes t and c
__device__ __forceinline__ void gl_project_bin(const GlsArgs& a, long e, float re,
                                               float im, double& s_err, double& s_a2) {
#pragma clang fp contract(off)
  const float A = a.A[e];
  const float2 tp = reinterpret_cast<const float2*>(a.t_prev)[e];
  const float m2 = re * re + im * im;
  float2 t;
  if (m2 > 1e-30f) {
    const float r = A / sqrtf(m2);
    t.x = re * r;
    t.y = im * r;
  } else {
    t.x = A;
    t.y = 0.f;
  }
  float2 c;
  const float dx = t.x - tp.x, dy = t.y - tp.y;
  const float ex = a.alpha * dx, ey = a.alpha * dy;
  c.x = t.x + ex;
  c.y = t.y + ey;
  reinterpret_cast<float2*>(a.t_out)[e] = t;
  reinterpret_cast<float2*>(a.out)[e] = c;
  const float g = sqrtf(m2) - A;
  s_err += (double)g * (double)g;
  s_a2 += (double)A * (double)A;
}

template <bool PROJECT>
__global__ __launch_bounds__(GL_WAVES * 64) void gl_stft_kernel(GlsArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float gl_lds[];
  float* ring = gl_lds;                       // later: the waves' sums
  float* win = gl_lds + GL_RING;              // [n_fft]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, f0 = blockIdx.x * GL_TF;
  int n = a.lengths ? a.lengths[b] : a.T;
  n = n < 0 ? 0 : (n > a.T ? a.T : n);
  const int nF = (n + a.hop - 1) / a.hop;     // the clip's real frames
  const int nreal = min(GL_TF, nF - f0);
  const int nhere = min(GL_TF, a.F - f0);     // the tile's frames in the tensors
  double* outp = a.partials ? a.partials + ((long)b * a.ntiles + blockIdx.x) * 2 : nullptr;
  const long e0 = ((long)b * a.F + f0) * a.n_bins;   // the tile's first (frame, bin)
  if (nreal <= 0) {                           // (workgroup-uniform)
    const long cnt = (long)nhere * a.n_bins;
    float2 z;
    z.x = 0.f;
    z.y = 0.f;
    for (long q = tid; q < cnt; q += GL_WAVES * 64) {
      reinterpret_cast<float2*>(a.out)[e0 + q] = z;
      if (PROJECT) reinterpret_cast<float2*>(a.t_out)[e0 + q] = z;
    }
    if (PROJECT && outp && tid < 2) outp[tid] = 0.0;
    return;
  }
  const float* cx = a.x + (long)b * a.ld_x;
  const long s0 = (long)f0 * a.hop + a.hop / 2 - a.n_fft / 2;   // the tile's first sample

  for (int j = tid; j < a.n_fft; j += GL_WAVES * 64) win[j] = a.window[j];
  __syncthreads();

  float* myring = ring + wave * 2 * GL_SLAB;
  const int nk = a.n_fft / GL_KC;
  const long gi = s0 + (long)i * a.hop;       // frame i's first sample
  const bool frame_ok = i < nreal, frame_here = i < nhere;
  const long ef = e0 + (long)i * a.n_bins;    // frame i's first bin
  double s_err = 0.0, s_a2 = 0.0;

  const float nyq_cos = h ? -1.f : 1.f;
  for (int c = wave; c < a.NC; c += GL_WAVES) {
    f32x16 re = frag_zero(), im = frag_zero();
    const bool nyq = c == 0 && i == 0;
    const f32x4* src = reinterpret_cast<const f32x4*>(a.basis + (long)c * a.n_fft * 64) + lane;
    f32x4 pf[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) pf[q] = src[q * 64];
    for (int kc = 0; kc < nk; ++kc) {
      float* sl = myring + (kc & 1) * GL_SLAB;
#pragma unroll
      for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(sl + (q * 64 + lane) * 4) = pf[q];
      __builtin_amdgcn_wave_barrier();
      if (kc + 1 < nk) {
#pragma unroll
        for (int q = 0; q < 4; ++q) pf[q] = src[(kc + 1) * 256 + q * 64];
      }
      const int j0 = kc * GL_KC;
#pragma unroll
      for (int s = 0; s < GL_KC / 2; ++s) {
        const int jj = j0 + 2 * s + h;
        const long g = gi + jj;
        float xv = 0.f;
        if (g >= 0 && g < n) xv = cx[g];
        const float w = xv * win[jj];
        const float* row = sl + (2 * s + h) * 64 + i;
        // (chunk 0, row 0 of the sin half: the Nyquist bin's cos, (-1)^j,
        // j's parity being h)
        const float bc = row[0], bs = nyq ? nyq_cos : row[32];
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(bc, w, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(bs, w, im, 0, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();
    }
    // element r of a fragment is [bin 32 c + 8 (r >> 2) + 4 h + (r & 3)][frame i];
    // bin 0's im element holds the Nyquist bin's re
    if (frame_here) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = 32 * c + 8 * (r >> 2) + 4 * h + (r & 3);
        float2 v, vn;
        v.x = frame_ok ? re[r] : 0.f;
        v.y = (frame_ok && k != 0) ? -im[r] : 0.f;
        vn.x = frame_ok ? im[r] : 0.f;        // (used at k == 0 only)
        vn.y = 0.f;
        if (!PROJECT) {
          reinterpret_cast<float2*>(a.out)[ef + k] = v;
          if (k == 0) reinterpret_cast<float2*>(a.out)[ef + a.n_fft / 2] = vn;
        } else if (frame_ok) {
          gl_project_bin(a, ef + k, v.x, v.y, s_err, s_a2);
          if (k == 0) gl_project_bin(a, ef + a.n_fft / 2, vn.x, 0.f, s_err, s_a2);
        } else {
          float2 z;
          z.x = 0.f;
          z.y = 0.f;
          reinterpret_cast<float2*>(a.out)[ef + k] = z;
          reinterpret_cast<float2*>(a.t_out)[ef + k] = z;
          if (k == 0) {
            reinterpret_cast<float2*>(a.out)[ef + a.n_fft / 2] = z;
            reinterpret_cast<float2*>(a.t_out)[ef + a.n_fft / 2] = z;
          }
        }
      }
    }
  }

  if (PROJECT && outp) {
    // lanes -> wave, then the waves in wave order in place of the ring
    s_err = gl_wave_sum(s_err);
    s_a2 = gl_wave_sum(s_a2);
    double* red = reinterpret_cast<double*>(ring);
    __syncthreads();
    if (lane == 0) {
      red[2 * wave] = s_err;
      red[2 * wave + 1] = s_a2;
    }
    __syncthreads();
    if (tid < 2) {
      double t = 0.0;
      for (int w = 0; w < GL_WAVES; ++w) t += red[2 * w + tid];
      outp[tid] = t;
    }
  }
}

__global__ void gl_trace_finish_kernel(const double* __restrict__ partials, int B,
                                       int ntiles, double* __restrict__ trace) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* p = partials + (long)b * ntiles * 2;
  double t0 = 0.0, t1 = 0.0;
  for (int k = 0; k < ntiles; ++k) {
    t0 += p[2 * k];
    t1 += p[2 * k + 1];
  }
  trace[2 * b] = t0;
  trace[2 * b + 1] = t1;
}

// ---------------------------------------------------------------------------
// The inverse: windowed frames into the scratch, then the gather.
// ---------------------------------------------------------------------------
struct GliArgs {
  const float* spec;
  const int32_t* lengths;
  const float* window;
  const float* basis;
  float* scratch;
  int T, F, n_fft, hop, n_bins;
  float scale;
};

__global__ __launch_bounds__(GL_WAVES * 64) void gl_istft_frames_kernel(GliArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float gl_lds[];
  float* slabs = gl_lds;                      // [GL_WAVES][GL_ISLAB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, f0 = blockIdx.x * GL_TF;
  int n = a.lengths ? a.lengths[b] : a.T;
  n = n < 0 ? 0 : (n > a.T ? a.T : n);
  const int nF = (n + a.hop - 1) / a.hop;
  const int nreal = min(GL_TF, nF - f0);
  if (nreal <= 0) return;                     // (workgroup-uniform)
  const bool ok = i < nreal;
  // frame i's spectrum and scratch row (frame f0 of a lane past the clip's
  // last frame: never dereferenced)
  const long fr = (long)b * a.F + f0 + (ok ? i : 0);
  const float2* sp = reinterpret_cast<const float2*>(a.spec) + fr * a.n_bins;
  float* dst = a.scratch + fr * a.n_fft;
  float* sl = slabs + wave * GL_ISLAB;
  const int ncb = a.n_fft / 64;               // bin chunks: bins 0 .. n_fft / 2 - 1
  float half_nyq = 0.f;
  if (ok) half_nyq = 0.5f * sp[a.n_fft / 2].x;
  const float nyq_sign = (i & 1) ? -1.f : 1.f;    // (-1)^j: a chunk starts at an even j

  for (int jc = wave; jc < a.n_fft / 32; jc += GL_WAVES) {
    f32x16 accc = frag_zero(), accs = frag_zero();
    const f32x4* src = reinterpret_cast<const f32x4*>(a.basis + (long)jc * 32 * 64) + lane;
    const long cstep = (long)a.n_fft * 16;    // f32x4s between two bin chunks
    f32x4 pf[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) pf[q] = src[q * 64];
    for (int c = 0; c < ncb; ++c) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int e = (q * 64 + lane) * 4;    // float of the [32][64] slab
        float* d = sl + (e >> 6) * 65 + (e & 63);
        d[0] = pf[q][0];
        d[1] = pf[q][1];
        d[2] = pf[q][2];
        d[3] = pf[q][3];
      }
      __builtin_amdgcn_wave_barrier();
      if (c + 1 < ncb) {
#pragma unroll
        for (int q = 0; q < 8; ++q) pf[q] = src[(c + 1) * cstep + q * 64];
      }
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int kk = 2 * s + h, k = 32 * c + kk;
        float acos_ = sl[i * 65 + kk], asin_ = sl[i * 65 + 32 + kk];
        float2 v;
        v.x = 0.f;
        v.y = 0.f;
        if (ok) v = sp[k];
        float bre = v.x, bim = -v.y;
        if (k == 0) {
          bre = 0.5f * v.x;
          bim = half_nyq;
          asin_ = nyq_sign;
        }
        accc = __builtin_amdgcn_mfma_f32_32x32x2f32(acos_, bre, accc, 0, 0, 0);
        accs = __builtin_amdgcn_mfma_f32_32x32x2f32(asin_, bim, accs, 0, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();
    }
    // element r is [sample 32 jc + 8 (r >> 2) + 4 h + (r & 3)][frame i]
    if (ok) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = 32 * jc + 8 * (r >> 2) + 4 * h + (r & 3);
        const float y = (accc[r] + accs[r]) * a.scale;
        dst[j] = y * a.window[j];
      }
    }
  }
}

__global__ __launch_bounds__(256) void gl_istft_gather_kernel(
    const float* __restrict__ scratch, const int32_t* __restrict__ lengths,
    const float* __restrict__ window, int T, int F, int n_fft, int hop,
    float* __restrict__ x, long ld_x) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  int n = lengths ? lengths[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  float v = 0.f;
  if (t < n) {
    const int nF = (n + hop - 1) / hop;
    // frame f covers t where 0 <= t - (f hop + hop / 2 - n_fft / 2) < n_fft
    const long u = t - hop / 2 + n_fft / 2;   // (>= 0: hop <= n_fft)
    long lo = u - n_fft < 0 ? 0 : (u - n_fft) / hop + 1;
    long hi = u / hop;
    if (hi > nF - 1) hi = nF - 1;
    const float* sc = scratch + (long)b * F * n_fft;
    float num = 0.f, den = 0.f;
    for (long f = lo; f <= hi; ++f) {
      const int j = (int)(u - f * hop);
      const float w = window[j];
      num += sc[f * n_fft + j];
      den += w * w;
    }
    if (den > 1e-8f) v = num / den;
  }
  x[(long)b * ld_x + t] = v;
}

// ---------------------------------------------------------------------------
// Mel inversion and the starting spectrum: plain lanes.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gl_mel_to_magnitude_kernel(
    const float* __restrict__ frames, int F, int n_mels,
    const int32_t* __restrict__ nframes, const float* __restrict__ pinv, int n_bins,
    float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float M[GL_MAX_MELS];
  const int b = blockIdx.y;
  int nf = F;
  if (nframes) {
    nf = nframes[b];
    nf = nf < 0 ? 0 : (nf > F ? F : nf);
  }
  for (int f = blockIdx.x; f < F; f += gridDim.x) {   // (workgroup-uniform)
    float* o = out + ((long)b * F + f) * n_bins;
    if (f >= nf) {
      for (int k = threadIdx.x; k < n_bins; k += 256) o[k] = 0.f;
      continue;
    }
    __syncthreads();                          // (the previous frame's M is read)
    if (threadIdx.x < n_mels)
      M[threadIdx.x] = expf(frames[((long)b * F + f) * n_mels + threadIdx.x]);
    __syncthreads();
    for (int k = threadIdx.x; k < n_bins; k += 256) {
      const float* row = pinv + (long)k * n_mels;
      float p = 0.f;
      for (int m = 0; m < n_mels; ++m) p += row[m] * M[m];
      p = p < 0.f ? 0.f : p;                  // (a NaN passes)
      o[k] = sqrtf(p);
    }
  }
}

__global__ __launch_bounds__(256) void gl_init_kernel(
    const float* __restrict__ A, int F, int n_bins, const int64_t* __restrict__ keys,
    uint64_t seed, int mode, const float* __restrict__ tab, float* __restrict__ c0) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const long cnt = (long)F * n_bins;
  const uint64_t hi = (uint64_t)keys[b] << 40;
  const float2* tb = reinterpret_cast<const float2*>(tab);
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < cnt; e += (long)gridDim.x * 256) {
    const int k = (int)(e % n_bins);
    int p = 0;
    if (mode == 0 && k != 0 && k != n_bins - 1)
      p = (int)(draw_bits(seed ^ GL_SEED_XOR, hi | (uint64_t)e) & (GL_PHASES - 1));
    const float a = A[(long)b * cnt + e];
    const float2 cs = tb[p];
    float2 v;
    v.x = a * cs.x;
    v.y = a * cs.y;
    reinterpret_cast<float2*>(c0)[(long)b * cnt + e] = v;
  }
}

static bool gl_grid_ok(int B, int T, int n_fft, int hop, int n_bins) {
  return n_fft >= 64 && n_fft <= GL_MAX_FFT && n_fft % 64 == 0 && hop >= 1 &&
         hop <= n_fft && n_bins == n_fft / 2 + 1 && B >= 1 && B <= 65535 && T >= 1 &&
         T <= (1 << 30);
}

static inline bool gl_mis(const void* p, unsigned mask) {
  return (reinterpret_cast<uintptr_t>(p) & mask) != 0;
}

// The kernels' dynamic LDS exceeds the 64 KiB a launch gets unasked: the
// largest size a kernel can ask for is allowed once per kernel and device
// (`done`: the kernel's own flags), not once per call.
#define GL_MAX_DEVICES 64
static int gl_allow_lds(const void* kernel, size_t bytes, bool* done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return WN_ERR_LAUNCH;
  if (dev >= 0 && dev < GL_MAX_DEVICES && done[dev]) return WN_OK;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)bytes) != hipSuccess)
    return WN_ERR_LAUNCH;
  if (dev >= 0 && dev < GL_MAX_DEVICES) done[dev] = true;
  return WN_OK;
}

template <bool PROJECT>
static int gl_stft_launch(const GlsArgs& a, int B, hipStream_t s) {
  static bool done[GL_MAX_DEVICES];
  const size_t lds = sizeof(float) * (size_t)(GL_RING + a.n_fft);
  if (gl_allow_lds((const void*)gl_stft_kernel<PROJECT>,
                   sizeof(float) * (size_t)(GL_RING + GL_MAX_FFT), done) != WN_OK)
    return WN_ERR_LAUNCH;
  hipLaunchKernelGGL((gl_stft_kernel<PROJECT>), dim3((unsigned)a.ntiles, (unsigned)B),
                     dim3(GL_WAVES * 64), lds, s, a);
  return wn_check_launch();
}

extern "C" {

int wn_stft(const float* x, long ld_x, int B, int T, const int32_t* lengths,
            const float* window, const float* basis, int n_fft, int hop,
            int n_bins, float* out, void* stream) {
  if (!x || !window || !basis || !out) return WN_ERR_NULL;
  if (!gl_grid_ok(B, T, n_fft, hop, n_bins) || ld_x < T) return WN_ERR_BAD_SHAPE;
  if (!wn_aligned16(basis) || gl_mis(x, 3u) || gl_mis(lengths, 3u) ||
      gl_mis(window, 3u) || gl_mis(out, 7u))
    return WN_ERR_MISALIGNED;
  GlsArgs a = {};
  a.x = x;
  a.ld_x = ld_x;
  a.lengths = lengths;
  a.window = window;
  a.basis = basis;
  a.out = out;
  a.T = T;
  a.F = (T + hop - 1) / hop;
  a.n_fft = n_fft;
  a.hop = hop;
  a.NC = n_fft / 64;              // the Nyquist bin rides in chunk 0
  a.n_bins = n_bins;
  a.ntiles = (a.F + GL_TF - 1) / GL_TF;
  return gl_stft_launch<false>(a, B, (hipStream_t)stream);
}

long wn_istft_scratch_bytes(int B, int T, int n_fft, int hop) {
  if (!gl_grid_ok(B, T, n_fft, hop, n_fft / 2 + 1)) return -1;
  const long F = ((long)T + hop - 1) / hop;
  return (long)sizeof(float) * B * F * n_fft;
}

int wn_istft(const float* spec, int B, int T, const int32_t* lengths,
             const float* window, const float* basis, int n_fft, int hop,
             int n_bins, float* scratch, float* x, long ld_x, void* stream) {
  if (!spec || !window || !basis || !scratch || !x) return WN_ERR_NULL;
  if (!gl_grid_ok(B, T, n_fft, hop, n_bins) || ld_x < T) return WN_ERR_BAD_SHAPE;
  if (!wn_aligned16(basis) || gl_mis(spec, 7u) || gl_mis(lengths, 3u) ||
      gl_mis(window, 3u) || gl_mis(scratch, 3u) || gl_mis(x, 3u))
    return WN_ERR_MISALIGNED;
  GliArgs a;
  a.spec = spec;
  a.lengths = lengths;
  a.window = window;
  a.basis = basis;
  a.scratch = scratch;
  a.T = T;
  a.F = (T + hop - 1) / hop;
  a.n_fft = n_fft;
  a.hop = hop;
  a.n_bins = n_bins;
  a.scale = (float)(2.0 / n_fft);
  const int ntiles = (a.F + GL_TF - 1) / GL_TF;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = sizeof(float) * (size_t)(GL_WAVES * GL_ISLAB);
  static bool done[GL_MAX_DEVICES];
  if (gl_allow_lds((const void*)gl_istft_frames_kernel, lds, done) != WN_OK)
    return WN_ERR_LAUNCH;
  hipLaunchKernelGGL(gl_istft_frames_kernel, dim3((unsigned)ntiles, (unsigned)B),
                     dim3(GL_WAVES * 64), lds, s, a);
  if (wn_check_launch() != WN_OK) return WN_ERR_LAUNCH;
  hipLaunchKernelGGL(gl_istft_gather_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)B),
                     dim3(256), 0, s, scratch, lengths, window, T, a.F, n_fft, hop, x, ld_x);
  return wn_check_launch();
}

int wn_mel_to_magnitude(const float* frames, int B, int F, int n_mels,
                        const int32_t* nframes, const float* pinv, int n_bins,
                        float* out, void* stream) {
  if (!frames || !pinv || !out) return WN_ERR_NULL;
  if (n_mels < 1 || n_mels > GL_MAX_MELS || n_bins < 1 || n_bins > GL_MAX_FFT / 2 + 1 ||
      B < 1 || B > 65535 || F < 1 || (long)B * (long)F > 2147483647L)
    return WN_ERR_BAD_SHAPE;
  if (gl_mis(frames, 3u) || gl_mis(nframes, 3u) || gl_mis(pinv, 3u) || gl_mis(out, 3u))
    return WN_ERR_MISALIGNED;
  const unsigned gx = (unsigned)(F < (1 << 20) ? F : (1 << 20));
  hipLaunchKernelGGL(gl_mel_to_magnitude_kernel, dim3(gx, (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, frames, F, n_mels, nframes, pinv, n_bins, out);
  return wn_check_launch();
}

int wn_gl_init(const float* A, int B, int F, int n_bins, const int64_t* keys,
               uint64_t seed, int mode, const float* tab, float* c0,
               void* stream) {
  if (!A || !keys || !tab || !c0) return WN_ERR_NULL;
  if (n_bins < 33 || n_bins > GL_MAX_FFT / 2 + 1 || (n_bins - 1) % 32 != 0 || B < 1 ||
      B > 65535 || F < 1 || (long)B * (long)F > 2147483647L ||
      (long)F * (long)n_bins >= (1L << 40))   // (the counter's low 40 bits)
    return WN_ERR_BAD_SHAPE;
  if (mode != 0 && mode != 1) return WN_ERR_UNSUPPORTED;
  if (gl_mis(A, 3u) || gl_mis(keys, 7u) || gl_mis(tab, 7u) || gl_mis(c0, 7u))
    return WN_ERR_MISALIGNED;
  const long blocks = ((long)F * n_bins + 255) / 256;
  const unsigned gx = (unsigned)(blocks < (1 << 20) ? blocks : (1 << 20));
  hipLaunchKernelGGL(gl_init_kernel, dim3(gx, (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, A, F, n_bins, keys, seed, mode, tab, c0);
  return wn_check_launch();
}

long wn_gl_project_partials(int B, int T, int hop) {
  if (B < 1 || B > 65535 || T < 1 || T > (1 << 30) || hop < 1) return -1;
  const long F = ((long)T + hop - 1) / hop;
  return 2L * B * ((F + GL_TF - 1) / GL_TF);
}

int wn_gl_project(const float* x, long ld_x, int B, int T, const int32_t* lengths,
                  const float* window, const float* basis, int n_fft, int hop,
                  int n_bins, const float* A, const float* t_prev, float alpha,
                  float* t_out, float* c_out, double* trace, double* partials,
                  void* stream) {
  if (!x || !window || !basis || !A || !t_prev || !t_out || !c_out ||
      (trace != nullptr) != (partials != nullptr))
    return WN_ERR_NULL;
  if (!gl_grid_ok(B, T, n_fft, hop, n_bins) || ld_x < T || !(alpha >= 0.f) ||
      !(alpha < 1.f) || c_out == t_out || c_out == t_prev || c_out == A ||
      t_out == A || t_prev == A)
    return WN_ERR_BAD_SHAPE;
  if (!wn_aligned16(basis) || gl_mis(x, 3u) || gl_mis(lengths, 3u) ||
      gl_mis(window, 3u) || gl_mis(A, 3u) || gl_mis(t_prev, 7u) || gl_mis(t_out, 7u) ||
      gl_mis(c_out, 7u) || gl_mis(trace, 7u) || gl_mis(partials, 7u))
    return WN_ERR_MISALIGNED;
  GlsArgs a = {};
  a.x = x;
  a.ld_x = ld_x;
  a.lengths = lengths;
  a.window = window;
  a.basis = basis;
  a.out = c_out;
  a.A = A;
  a.t_prev = t_prev;
  a.t_out = t_out;
  a.partials = partials;
  a.T = T;
  a.F = (T + hop - 1) / hop;
  a.n_fft = n_fft;
  a.hop = hop;
  a.NC = n_fft / 64;
  a.n_bins = n_bins;
  a.ntiles = (a.F + GL_TF - 1) / GL_TF;
  a.alpha = alpha;
  hipStream_t s = (hipStream_t)stream;
  const int rc = gl_stft_launch<true>(a, B, s);
  if (rc != WN_OK || !trace) return rc;
  hipLaunchKernelGGL(gl_trace_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, s,
                     partials, B, a.ntiles, trace);
  return wn_check_launch();
}

}  // extern "C"
