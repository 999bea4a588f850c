// Synthesis metrics (include/wavenet_spectral.h states both rules and the
// summation orders; wavenet/spectral.py states them in numpy, tests/stft_ref.py
// restates them in float64): the STFT distance of two signals at one
// resolution, and the cepstral distance of two log-mel tensors.
//
// stft_distance_kernel is melspec_kernel's shape (wn_features.hip) with two
// signals and no filterbank.  One workgroup owns a tile of 32 consecutive
// frames of one clip; the DFT is the fp32 MFMA contraction of the windowed
// frames with the cos | sin basis, bins on the M axis, frames on the N axis,
// so a column is a frame.  The eight waves split the 32-bin chunks (chunk c ->
// wave c % 8); a wave streams its chunk's basis rows ONCE through its private
// LDS ring, in pieces of 16 samples, and uses every row for both signals'
// accumulators: re and im of the generated and of the original signal, four
// [32 bins][32 frames] fragments.  The n_fft / 2 bins 0 .. n_fft / 2 - 1 fill
// n_fft / 64 chunks; the Nyquist bin, whose sin row is zero and whose cos row is
// (-1)^j, takes the place of bin 0's sin row, which is zero too, so that it
// does not cost a 33rd chunk of one bin (and a fifth trip for one wave of
// eight).  The epilogue runs on the fragments in
// registers: both power spectra, the two clamped magnitudes, their difference
// and the log distance, each widened to float64 and added to the lane's three
// sums; padding bins and frames behind the clip's last add nothing.  Lanes ->
// wave by the xor butterfly, waves in wave order through LDS, one triple per
// tile; stft_distance_finish_kernel adds a clip's tiles in ascending order.
// No atomics.  A frame's terms depend on its own samples and the tables only,
// a tile's triple on its frames only, so a clip's sums do not depend on the
// batch; a tile behind the clip's last frame adds +0.0.
//
// Both signals' 31 * hop + n_fft samples are staged in LDS (zeros outside
// [0, n)), with one pad float after every `hop` samples at an even hop (odd
// lane stride: 32 banks for the 32 lanes of a read), when they fit beside the
// ring and the window table in 160 KiB; otherwise every sample is read from
// memory where it is used -- the same values, the same arithmetic.
#include "wn_common.h"

#define SPD_TF 32                  // frames per tile
#define SPD_WAVES 8
#define SPD_KC 16                  // samples per basis piece
#define SPD_SLAB (SPD_KC * 64)     // floats of a piece: [16][cos 32 | sin 32]
#define SPD_RING (SPD_WAVES * 2 * SPD_SLAB)
#define SPD_LDS_FLOATS 40960       // 160 KiB
#define SPD_MAX_FFT 2048

struct SpdArgs {
  const float* gen;
  const float* org;
  long ld_gen, ld_org;
  const int32_t* lengths;
  const float* window;
  const float* basis;
  double* partials;
  int T, F, n_fft, hop, NC, pad, nstage, ntiles;
  float floor_;
};

__device__ __forceinline__ double spd_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one (frame, bin)'s terms, added to the lane's sums
__device__ __forceinline__ void spd_terms(float rg, float ig, float ro, float io,
                                          float fl, double& s_num, double& s_den,
                                          double& s_log) {
#pragma clang fp contract(off)
  float pg = rg * rg + ig * ig;
  float po = ro * ro + io * io;
  pg = pg < fl ? fl : pg;                     // (a NaN passes)
  po = po < fl ? fl : po;
  const float mg = sqrtf(pg), mo = sqrtf(po);
  const float d = mo - mg;
  const float l = fabsf(logf(po) - logf(pg)) * 0.5f;
  s_num += (double)d * (double)d;
  s_den += (double)mo * (double)mo;
  s_log += (double)l;
}

// floats one signal's staged samples take (the pad floats and one spare)
static long spd_stage_floats(int n_fft, int hop) {
  const long total = (long)(SPD_TF - 1) * hop + n_fft;
  const int pad = (hop & 1) ? 0 : 1;
  return total + pad * ((total - 1) / hop) + 1;
}

static bool spd_staged(int n_fft, int hop) {
  return SPD_RING + 2L * n_fft + 2 * spd_stage_floats(n_fft, hop) <= SPD_LDS_FLOATS;
}

template <bool STAGE>
__global__ __launch_bounds__(SPD_WAVES * 64) void stft_distance_kernel(SpdArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float spd_lds[];
  float* ring = spd_lds;                      // later: the waves' sums
  float2* tbl = reinterpret_cast<float2*>(spd_lds + SPD_RING);   // [n_fft] {window, slot}
  float* stage_g = spd_lds + SPD_RING + 2 * a.n_fft;
  float* stage_o = stage_g + a.nstage;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, f0 = blockIdx.x * SPD_TF;
  int n = a.lengths ? a.lengths[b] : a.T;
  n = n < 0 ? 0 : (n > a.T ? a.T : n);
  const int nF = (n + a.hop - 1) / a.hop;     // the clip's real frames
  const int nreal = min(SPD_TF, nF - f0);
  double* outp = a.partials + ((long)b * a.ntiles + blockIdx.x) * 3;
  if (nreal <= 0) {                           // (workgroup-uniform)
    if (tid < 3) outp[tid] = 0.0;
    return;
  }
  const float* cg = a.gen + (long)b * a.ld_gen;
  const float* co = a.org + (long)b * a.ld_org;
  const long s0 = (long)f0 * a.hop + a.hop / 2 - a.n_fft / 2;   // the tile's first sample

  for (int j = tid; j < a.n_fft; j += SPD_WAVES * 64) {
    float2 t;
    t.x = a.window[j];
    t.y = __int_as_float(STAGE ? j + a.pad * (j / a.hop) : j);
    tbl[j] = t;
  }
  if (STAGE) {
    const int total = (SPD_TF - 1) * a.hop + a.n_fft;
    for (int r = tid; r < total; r += SPD_WAVES * 64) {
      const long g = s0 + r;
      float vg = 0.f, vo = 0.f;
      if (g >= 0 && g < n) {
        vg = cg[g];
        vo = co[g];
      }
      const int slot = r + a.pad * (r / a.hop);
      stage_g[slot] = vg;
      stage_o[slot] = vo;
    }
  }
  __syncthreads();

  float* myring = ring + wave * 2 * SPD_SLAB;
  const int nk = a.n_fft / SPD_KC;
  const int xoff = i * (a.hop + a.pad);       // frame i's first staged slot
  const long gi = s0 + (long)i * a.hop;       // ... first sample
  const float fl = a.floor_;
  const bool frame_ok = i < nreal;
  double s_num = 0.0, s_den = 0.0, s_log = 0.0;

  const float nyq_cos = h ? -1.f : 1.f;
  for (int c = wave; c < a.NC; c += SPD_WAVES) {
    f32x16 reg = frag_zero(), img = frag_zero(), reo = frag_zero(), imo = frag_zero();
    const bool nyq = c == 0 && i == 0;
    const f32x4* src = reinterpret_cast<const f32x4*>(a.basis + (long)c * a.n_fft * 64) + lane;
    f32x4 pf[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) pf[q] = src[q * 64];
    for (int kc = 0; kc < nk; ++kc) {
      float* sl = myring + (kc & 1) * SPD_SLAB;
#pragma unroll
      for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(sl + (q * 64 + lane) * 4) = pf[q];
      __builtin_amdgcn_wave_barrier();
      if (kc + 1 < nk) {
#pragma unroll
        for (int q = 0; q < 4; ++q) pf[q] = src[(kc + 1) * 256 + q * 64];
      }
      const int j0 = kc * SPD_KC;
#pragma unroll
      for (int s = 0; s < SPD_KC / 2; ++s) {
        const int jj = j0 + 2 * s + h;
        const float2 t = tbl[jj];
        float xg, xo;
        if (STAGE) {
          const int slot = xoff + __float_as_int(t.y);
          xg = stage_g[slot];
          xo = stage_o[slot];
        } else {
          const long g = gi + jj;
          xg = 0.f;
          xo = 0.f;
          if (g >= 0 && g < n) {
            xg = cg[g];
            xo = co[g];
          }
        }
        const float wg = xg * t.x, wo = xo * t.x;
        const float* row = sl + (2 * s + h) * 64 + i;
        // (chunk 0, row 0 of the sin half: the Nyquist bin's cos, (-1)^j,
        // j's parity being h)
        const float bc = row[0], bs = nyq ? nyq_cos : row[32];
        reg = __builtin_amdgcn_mfma_f32_32x32x2f32(bc, wg, reg, 0, 0, 0);
        img = __builtin_amdgcn_mfma_f32_32x32x2f32(bs, wg, img, 0, 0, 0);
        reo = __builtin_amdgcn_mfma_f32_32x32x2f32(bc, wo, reo, 0, 0, 0);
        imo = __builtin_amdgcn_mfma_f32_32x32x2f32(bs, wo, imo, 0, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();
    }
    // element r of a fragment is [bin 32 c + 8 (r >> 2) + 4 h + (r & 3)][frame i];
    // bin 0's im element holds the Nyquist bin's re
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = 32 * c + 8 * (r >> 2) + 4 * h + (r & 3);
      if (frame_ok) {
        float ig = img[r], io = imo[r];
        if (k == 0) {
          ig = 0.f;
          io = 0.f;
        }
        spd_terms(reg[r], ig, reo[r], io, fl, s_num, s_den, s_log);
        if (k == 0) spd_terms(img[r], 0.f, imo[r], 0.f, fl, s_num, s_den, s_log);
      }
    }
  }

  // lanes -> wave, then the waves in wave order in place of the ring
  s_num = spd_wave_sum(s_num);
  s_den = spd_wave_sum(s_den);
  s_log = spd_wave_sum(s_log);
  double* red = reinterpret_cast<double*>(ring);
  __syncthreads();
  if (lane == 0) {
    red[3 * wave] = s_num;
    red[3 * wave + 1] = s_den;
    red[3 * wave + 2] = s_log;
  }
  __syncthreads();
  if (tid < 3) {
    double t = 0.0;
    for (int w = 0; w < SPD_WAVES; ++w) t += red[3 * w + tid];
    outp[tid] = t;
  }
}

__global__ void stft_distance_finish_kernel(const double* __restrict__ partials,
                                            int B, int ntiles,
                                            double* __restrict__ sc_num,
                                            double* __restrict__ sc_den,
                                            double* __restrict__ log_sum) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* p = partials + (long)b * ntiles * 3;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0;
  for (int k = 0; k < ntiles; ++k) {
    t0 += p[3 * k];
    t1 += p[3 * k + 1];
    t2 += p[3 * k + 2];
  }
  sc_num[b] = t0;
  sc_den[b] = t1;
  log_sum[b] = t2;
}

template <bool STAGE>
static int spd_launch(const SpdArgs& a, int B, size_t lds, hipStream_t s) {
  if (hipFuncSetAttribute((const void*)stft_distance_kernel<STAGE>,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return WN_ERR_LAUNCH;
  hipLaunchKernelGGL((stft_distance_kernel<STAGE>), dim3((unsigned)a.ntiles, (unsigned)B),
                     dim3(SPD_WAVES * 64), lds, s, a);
  return wn_check_launch();
}

// ---------------------------------------------------------------------------
// Cepstral distance.  Workgroup (clip, k) owns the frames [k CEP_TF,
// (k + 1) CEP_TF) of its clip, cut at nframes; its four waves take the frames
// f0 + w, f0 + w + 4, ... in ascending order, one frame per trip.  The wave
// puts d[m] = a[m] - b[m] (float32, widened) into its LDS row; lane n < K adds
// e[n] = sum_m dct[n][m] d[m] in float64 from zero, m ascending, every product
// rounded before it is added (no FMA); the frame's s = sum_n e[n]^2 is the xor
// butterfly (32, 16, ... 1) of the lanes' squares (lanes >= K hold zeros);
// r = sqrt(0.5 s) is added to the wave's sum.  The four waves are added in the
// order 0, 1, 2, 3; cepstral_distance_finish_kernel adds a clip's chunks in
// ascending order, from zero.  No atomics; frames at or behind nframes[b] are
// not read.
// ---------------------------------------------------------------------------
#define CEP_TF 64
#define CEP_THREADS 256
#define CEP_MAX_C 512
#define CEP_MAX_K 64

__global__ __launch_bounds__(CEP_THREADS) void cepstral_distance_partials_kernel(
    const float* __restrict__ a, const float* __restrict__ b, int F, int C,
    const int32_t* __restrict__ nframes, const double* __restrict__ dct, int K,
    int nchunk, double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double dl[CEP_THREADS / 64][CEP_MAX_C];
  __shared__ double red[CEP_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long clip = blockIdx.x / nchunk;
  const int f0 = (int)(blockIdx.x - clip * nchunk) * CEP_TF;
  int n = F;
  if (nframes) {
    n = nframes[clip];
    n = n < 0 ? 0 : (n > F ? F : n);
  }
  const int f1 = n < f0 + CEP_TF ? n : f0 + CEP_TF;
  double* d = dl[wave];
  const double* row = dct + (long)(lane < K ? lane : 0) * C;
  double sr = 0.0;
  // (wave-uniform trips: every lane takes part in the butterfly)
  for (int f = f0 + wave; f < f1; f += CEP_THREADS / 64) {
    const long o = (clip * F + f) * C;
    for (int c = lane; c < C; c += 64) d[c] = (double)(a[o + c] - b[o + c]);
    __builtin_amdgcn_wave_barrier();
    double e = 0.0;
    if (lane < K)
      for (int m = 0; m < C; ++m) e += row[m] * d[m];
    __builtin_amdgcn_wave_barrier();          // (the next frame overwrites d)
    sr += sqrt(0.5 * spd_wave_sum(e * e));
  }
  if (lane == 0) red[wave] = sr;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < CEP_THREADS / 64; ++w) t += red[w];
    partials[blockIdx.x] = t;
  }
}

__global__ void cepstral_distance_finish_kernel(const double* __restrict__ partials,
                                                int B, int nchunk,
                                                double* __restrict__ mcd_sum) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* p = partials + (long)b * nchunk;
  double t = 0.0;
  for (int k = 0; k < nchunk; ++k) t += p[k];
  mcd_sum[b] = t;
}

extern "C" {

long wn_stft_distance_partials(int B, int T, int hop) {
  if (B < 1 || B > 65535 || T < 1 || T > (1 << 30) || hop < 1) return -1;
  const long F = ((long)T + hop - 1) / hop;
  return 3L * B * ((F + SPD_TF - 1) / SPD_TF);
}

int wn_stft_distance_staged(int n_fft, int hop) {
  if (n_fft < 64 || n_fft > SPD_MAX_FFT || n_fft % 64 != 0 || hop < 1 || hop > n_fft)
    return 0;
  return spd_staged(n_fft, hop) ? 1 : 0;
}

int wn_stft_distance(const float* gen, long ld_gen, const float* org, long ld_org,
                     int B, int T, const int32_t* lengths, const float* window,
                     const float* basis, int n_fft, int hop, int n_bins,
                     float floor_, double* sc_num, double* sc_den,
                     double* log_sum, double* partials, void* stream) {
  if (!gen || !org || !window || !basis || !sc_num || !sc_den || !log_sum || !partials)
    return WN_ERR_NULL;
  if (n_fft < 64 || n_fft > SPD_MAX_FFT || n_fft % 64 != 0 || hop < 1 ||
      hop > n_fft || n_bins != n_fft / 2 + 1 || !(floor_ > 0.f) ||
      !(floor_ < INFINITY) || B < 1 || B > 65535 || T < 1 || T > (1 << 30) ||
      ld_gen < T || ld_org < T)
    return WN_ERR_BAD_SHAPE;
  if (!wn_aligned16(basis) || (reinterpret_cast<uintptr_t>(gen) & 3u) ||
      (reinterpret_cast<uintptr_t>(org) & 3u) ||
      (reinterpret_cast<uintptr_t>(window) & 3u) ||
      (reinterpret_cast<uintptr_t>(lengths) & 3u) ||
      (reinterpret_cast<uintptr_t>(sc_num) & 7u) ||
      (reinterpret_cast<uintptr_t>(sc_den) & 7u) ||
      (reinterpret_cast<uintptr_t>(log_sum) & 7u) ||
      (reinterpret_cast<uintptr_t>(partials) & 7u))
    return WN_ERR_MISALIGNED;
  SpdArgs a;
  a.gen = gen;
  a.org = org;
  a.ld_gen = ld_gen;
  a.ld_org = ld_org;
  a.lengths = lengths;
  a.window = window;
  a.basis = basis;
  a.partials = partials;
  a.T = T;
  a.F = (T + hop - 1) / hop;
  a.n_fft = n_fft;
  a.hop = hop;
  a.NC = n_fft / 64;              // the Nyquist bin rides in chunk 0
  a.pad = (hop & 1) ? 0 : 1;
  a.ntiles = (a.F + SPD_TF - 1) / SPD_TF;
  a.floor_ = floor_;
  const bool staged = spd_staged(n_fft, hop);
  a.nstage = staged ? (int)spd_stage_floats(n_fft, hop) : 0;
  const size_t lds = sizeof(float) * (size_t)(SPD_RING + 2 * n_fft + 2 * a.nstage);
  hipStream_t s = (hipStream_t)stream;
  const int rc = staged ? spd_launch<true>(a, B, lds, s) : spd_launch<false>(a, B, lds, s);
  if (rc != WN_OK) return rc;
  hipLaunchKernelGGL(stft_distance_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, s,
                     partials, B, a.ntiles, sc_num, sc_den, log_sum);
  return wn_check_launch();
}

long wn_cepstral_distance_partials(int B, int F) {
  if (B < 1 || F < 1 || (long)B * (long)F > 2147483647L) return -1;
  return (long)B * ((F + CEP_TF - 1) / CEP_TF);
}

int wn_cepstral_distance(const float* a, const float* b, int B, int F, int C,
                         const int32_t* nframes, const double* dct, int K,
                         double* mcd_sum, double* partials, void* stream) {
  if (!a || !b || !dct || !mcd_sum || !partials) return WN_ERR_NULL;
  if (C < 1 || C > CEP_MAX_C || K < 1 || K > CEP_MAX_K || K > C - 1 || B < 1 ||
      F < 1 || (long)B * (long)F > 2147483647L)
    return WN_ERR_BAD_SHAPE;
  if ((reinterpret_cast<uintptr_t>(a) & 3u) || (reinterpret_cast<uintptr_t>(b) & 3u) ||
      (reinterpret_cast<uintptr_t>(nframes) & 3u) ||
      (reinterpret_cast<uintptr_t>(dct) & 7u) ||
      (reinterpret_cast<uintptr_t>(mcd_sum) & 7u) ||
      (reinterpret_cast<uintptr_t>(partials) & 7u))
    return WN_ERR_MISALIGNED;
  const int nchunk = (F + CEP_TF - 1) / CEP_TF;
  const unsigned grid = (unsigned)((long)B * nchunk);   // (<= B F <= 2^31 - 1)
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cepstral_distance_partials_kernel, dim3(grid), dim3(CEP_THREADS), 0, s,
                     a, b, F, C, nframes, dct, K, nchunk, partials);
  if (wn_check_launch() != WN_OK) return WN_ERR_LAUNCH;
  hipLaunchKernelGGL(cepstral_distance_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, s,
                     partials, B, nchunk, mcd_sum);
  return wn_check_launch();
}

}  // extern "C"
