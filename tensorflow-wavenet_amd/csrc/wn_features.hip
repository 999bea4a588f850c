// Log-mel front end (wavenet/features.py states the rule; tests/mel_ref.py
// restates it in float64 numpy): frame-rate local-conditioning features from
// the audio itself, aligned to the LC convention -- frame f sits beside the
// samples f * hop .. f * hop + hop - 1 and is centred at f * hop + hop / 2.
//
//   frame[j]  = x[f * hop + hop / 2 - n_fft / 2 + j] * window[j]   (x = 0 outside [0, n))
//   P[k]      = |DFT(frame)[k]|^2,  k = 0 .. n_fft / 2
//   out[f][m] = log(max(sum_k melw[m][k] P[k], floor))
//
// One workgroup owns a tile of 32 consecutive frames of one clip.  The
// 31 * hop + n_fft samples the tile touches are staged into LDS once (zeros
// outside the clip), the DFT is a fp32 MFMA contraction of the windowed
// frames with the cos | sin basis, computed transposed as everywhere in this
// directory (wn_common.h): bins on the M axis, frames on the N axis, so an
// accumulator [32 bins][32 frames] is, after re^2 + im^2, directly the B
// operand of the second contraction with that chunk of the mel filterbank.
// The power spectrum never leaves the registers.
//
// The eight waves split the 32-bin chunks (chunk c -> wave c % 8); a wave
// streams its chunk's basis rows through a wave-private LDS ring in pieces of
// 16 samples, and keeps a [n_mels][32 frames] accumulator over its chunks.
// The waves' accumulators are added in wave order through LDS -- no atomics,
// one summation order per (n_fft, n_mels) -- and the epilogue applies floor
// and log and writes the tile's rows, contiguous in `out`, with 16-byte
// stores.  Every MFMA column is one frame: a frame's bits depend on its own
// samples and the tables only, not on its position in the tile, the batch
// size or the other clips.
//
// LDS banks: lane i of a half-wave reads frame i's sample, hop floats further
// per lane -- one bank for all 32 lanes at an even hop.  The staged samples are
// therefore laid out with one pad float after every `hop` samples when hop is
// even: the lane stride hop + pad is odd and the 32 lanes of a ds_read_b32
// group hit 32 different banks.  A sample's slot is r + pad * (r / hop); the
// window table carries that offset for j beside the window value.
#include "wn_common.h"

#define MEL_TF 32                  // frames per tile
#define MEL_WAVES 8
#define MEL_KC 16                  // samples per basis piece
#define MEL_SLAB (MEL_KC * 64)     // floats of a piece: [16][cos 32 | sin 32]
#define MEL_RING (MEL_WAVES * 2 * MEL_SLAB)
#define MEL_STAGE_MAX 16384        // floats of staged samples (64 KiB)
#define MEL_MAX_FFT 2048
#define MEL_MAX_MELS 128

struct MelArgs {
  const float* audio;
  long ld;
  const int32_t* lengths;
  const float* window;
  const float* basis;
  const float* melw;
  float* out;
  int T, F, n_fft, hop, NC, n_mels, MP, pad;
  float floor_;
};

// STAGE: the tile's samples fit the LDS budget (else they are read from
// memory, the same values); MB = padded mels / 32
template <bool STAGE, int MB>
__global__ __launch_bounds__(MEL_WAVES * 64) void melspec_kernel(MelArgs a) {
  extern __shared__ __attribute__((aligned(16))) float mel_lds[];
  float* ring = mel_lds;                      // later: the waves' sum [32][MP + 4]
  float2* tbl = reinterpret_cast<float2*>(mel_lds + MEL_RING);   // [n_fft] {window, slot}
  float* stage = mel_lds + MEL_RING + 2 * a.n_fft;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, f0 = blockIdx.x * MEL_TF;
  int n = a.lengths ? a.lengths[b] : a.T;
  n = n < 0 ? 0 : (n > a.T ? a.T : n);
  const int nF = (n + a.hop - 1) / a.hop;     // the clip's real frames
  const int rows = min(MEL_TF, a.F - f0);
  const int nreal = max(0, min(rows, nF - f0));
  float* outp = a.out + ((long)b * a.F + f0) * a.n_mels;
  const int ntot = rows * a.n_mels;
  if (nreal == 0) {                           // (workgroup-uniform)
    for (int e = tid; e < ntot; e += MEL_WAVES * 64) outp[e] = 0.f;
    return;
  }
  const float* clip = a.audio + (long)b * a.ld;
  const long s0 = (long)f0 * a.hop + a.hop / 2 - a.n_fft / 2;   // the tile's first sample

  for (int j = tid; j < a.n_fft; j += MEL_WAVES * 64) {
    float2 t;
    t.x = a.window[j];
    t.y = __int_as_float(STAGE ? j + a.pad * (j / a.hop) : j);
    tbl[j] = t;
  }
  if (STAGE) {
    const int total = (MEL_TF - 1) * a.hop + a.n_fft;
    for (int r = tid; r < total; r += MEL_WAVES * 64) {
      const long g = s0 + r;
      float v = 0.f;
      if (g >= 0 && g < n) v = clip[g];
      stage[r + a.pad * (r / a.hop)] = v;
    }
  }
  __syncthreads();

  f32x16 macc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) macc[mb] = frag_zero();
  float* myring = ring + wave * 2 * MEL_SLAB;
  const int nk = a.n_fft / MEL_KC;
  const int xoff = i * (a.hop + a.pad);       // frame i's first staged slot
  const long gi = s0 + (long)i * a.hop;       // ... first sample

  for (int c = wave; c < a.NC; c += MEL_WAVES) {
    f32x16 re = frag_zero(), im = frag_zero();
    const f32x4* src = reinterpret_cast<const f32x4*>(a.basis + (long)c * a.n_fft * 64) + lane;
    f32x4 pf[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) pf[q] = src[q * 64];
    for (int kc = 0; kc < nk; ++kc) {
      float* sl = myring + (kc & 1) * MEL_SLAB;
#pragma unroll
      for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(sl + (q * 64 + lane) * 4) = pf[q];
      __builtin_amdgcn_wave_barrier();
      if (kc + 1 < nk) {
#pragma unroll
        for (int q = 0; q < 4; ++q) pf[q] = src[(kc + 1) * 256 + q * 64];
      }
      const int j0 = kc * MEL_KC;
#pragma unroll
      for (int s = 0; s < MEL_KC / 2; ++s) {
        const int jj = j0 + 2 * s + h;
        const float2 t = tbl[jj];
        float x;
        if (STAGE) {
          x = stage[xoff + __float_as_int(t.y)];
        } else {
          const long g = gi + jj;
          x = 0.f;
          if (g >= 0 && g < n) x = clip[g];
        }
        const float xw = x * t.x;
        const float* row = sl + (2 * s + h) * 64 + i;
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(row[0], xw, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(row[32], xw, im, 0, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();
    }
    // P = re^2 + im^2 is the fragment [bin 8(r>>2) + 4h + (r&3)][frame i]:
    // the B operand of macc[mel][frame] += melw[bin][mel] P[bin][frame]
    const float* mw = a.melw + (long)(32 * c + 4 * h) * a.MP + i;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = __builtin_fmaf(im[r], im[r], re[r] * re[r]);
      const float* mr = mw + (8 * (r >> 2) + (r & 3)) * a.MP;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
        macc[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(mr[32 * mb], p, macc[mb], 0, 0, 0);
    }
  }

  // the waves' sums, added in wave order in place of the ring
  const int ldr = a.MP + 4;
  float* red = ring;
  __syncthreads();
  for (int w = 0; w < MEL_WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4* p = reinterpret_cast<f32x4*>(red + i * ldr + 32 * mb + 8 * q + 4 * h);
          f32x4 v = {macc[mb][4 * q], macc[mb][4 * q + 1], macc[mb][4 * q + 2],
                     macc[mb][4 * q + 3]};
          if (w > 0) v += *p;
          *p = v;
        }
    }
    __syncthreads();
  }

  // floor, log; rows at or behind the clip's last frame are exact zeros
  const float fl = a.floor_;
  if ((a.n_mels & 3) == 0) {
    for (int e = tid * 4; e < ntot; e += MEL_WAVES * 64 * 4) {
      const int f = e / a.n_mels, m = e - f * a.n_mels;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (f < nreal) {
        v = *reinterpret_cast<const f32x4*>(red + f * ldr + m);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = logf(v[k] < fl ? fl : v[k]);
      }
      *reinterpret_cast<f32x4*>(outp + e) = v;
    }
  } else {
    for (int e = tid; e < ntot; e += MEL_WAVES * 64) {
      const int f = e / a.n_mels, m = e - f * a.n_mels;
      float v = 0.f;
      if (f < nreal) {
        v = red[f * ldr + m];
        v = logf(v < fl ? fl : v);
      }
      outp[e] = v;
    }
  }
}

template <bool STAGE>
static int mel_launch(const MelArgs& a, int B, size_t lds, hipStream_t s) {
  const dim3 grid((unsigned)((a.F + MEL_TF - 1) / MEL_TF), (unsigned)B);
#define LAUNCH(MB)                                                              \
  {                                                                             \
    if (hipFuncSetAttribute((const void*)melspec_kernel<STAGE, MB>,             \
                            hipFuncAttributeMaxDynamicSharedMemorySize,         \
                            (int)lds) != hipSuccess)                            \
      return WN_ERR_LAUNCH;                                                     \
    hipLaunchKernelGGL((melspec_kernel<STAGE, MB>), grid, dim3(MEL_WAVES * 64), \
                       lds, s, a);                                              \
  }
  switch (a.MP / 32) {
    case 1: LAUNCH(1) break;
    case 2: LAUNCH(2) break;
    case 3: LAUNCH(3) break;
    default: LAUNCH(4) break;
  }
#undef LAUNCH
  return wn_check_launch();
}

// ---------------------------------------------------------------------------
// Feature normalisation: per-channel statistics of frames and the affine +
// clamp normaliser (wavenet/features.py: FeatureStats, Normalizer;
// tests/featnorm_ref.py restates both).
//
// feature_stats_partials_kernel: FSTAT_PARTS partial sums of x and x * x per
// channel, x widened to float64 first.  The B * F rows are cut into
// FSTAT_PARTS contiguous ranges of per = ceil(B F / FSTAT_PARTS) rows, partial
// k = rows [k per, min(B F, (k + 1) per)) -- a function of (B, F, FSTAT_PARTS)
// only; an empty range gives zeros.  Inside a range the workgroup's 256
// threads form G = 256 / L row groups of L = 2^ceil(log2(ceil(C / V))) lanes
// (at most 256), V = 4 channels per lane where C % 4 == 0 (one 16-byte load),
// else 1.  Row group g adds its rows lo + g, lo + g + G, ... in ascending
// order, the G group sums are added in the order g = 0, 1, ... through LDS.
// feature_stats_finish_kernel adds the partials k = 0, 1, ... in order, from
// zero, and adds that sum to acc.  No atomics: the result is a function of
// the input's bits, (B, F, C), nframes and the previous acc.  Rows at or
// behind nframes[b] are not read.
// ---------------------------------------------------------------------------
#define FSTAT_PARTS 256
#define FSTAT_THREADS 256
#define FNORM_THREADS 256
#define FEAT_MAX_C 512

template <int V>
__global__ __launch_bounds__(FSTAT_THREADS) void feature_stats_partials_kernel(
    const float* __restrict__ fr, long R, int F, int C,
    const int32_t* __restrict__ nframes, long per, int L,
    double* __restrict__ partials) {
  __shared__ double red[2 * V * FSTAT_THREADS];
  const int tid = threadIdx.x;
  const int G = FSTAT_THREADS / L, g = tid / L, lane = tid - g * L;
  const long lo = (long)blockIdx.x * per;
  const long hi = lo + per < R ? lo + per : R;
  double* outp = partials + (long)blockIdx.x * 2 * C;
  // (C > 256 V: L = 256, G = 1, and a lane takes several channel groups)
  // (every thread makes every trip: the barriers below are workgroup-wide)
  for (int cb = 0; cb < C; cb += L * V) {
    const int c0 = cb + lane * V;
    const bool live = c0 < C;
    double s1[V], s2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s1[e] = s2[e] = 0.0;
    for (long r = lo + g; live && r < hi; r += G) {
      const long b = r / F;
      const int f = (int)(r - b * F);
      int n = F;
      if (nframes) {
        n = nframes[b];
        n = n < 0 ? 0 : (n > F ? F : n);
      }
      if (f >= n) continue;
      const float* row = fr + r * C + c0;
      if (V == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const double x = (double)v[e];
          s1[e] += x;
          s2[e] += x * x;
        }
      } else {
        const double x = (double)row[0];
        s1[0] += x;
        s2[0] += x * x;
      }
    }
    __syncthreads();                 // (the previous channel group's reads)
#pragma unroll
    for (int e = 0; e < V; ++e) {
      red[(2 * e) * FSTAT_THREADS + tid] = s1[e];
      red[(2 * e + 1) * FSTAT_THREADS + tid] = s2[e];
    }
    __syncthreads();
    if (g == 0 && live) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        double t1 = 0.0, t2 = 0.0;
        for (int q = 0; q < G; ++q) {
          t1 += red[(2 * e) * FSTAT_THREADS + q * L + lane];
          t2 += red[(2 * e + 1) * FSTAT_THREADS + q * L + lane];
        }
        outp[c0 + e] = t1;
        outp[C + c0 + e] = t2;
      }
    }
  }
}

__global__ void feature_stats_finish_kernel(const double* __restrict__ partials,
                                            int C, double* __restrict__ acc) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;   // [2][C] flat
  if (j >= 2 * C) return;
  double t = 0.0;
  for (int k = 0; k < FSTAT_PARTS; ++k) t += partials[(long)k * 2 * C + j];
  acc[j] += t;
}

// out = clamp((in - shift[c]) * scale[c]) on the real frames, exact zeros on
// the others (which are not read).  One subtraction, one multiplication: no
// FMA can form.  The clamp's comparisons are false for a NaN, which passes.
template <int V>
__global__ __launch_bounds__(FNORM_THREADS) void feature_normalize_kernel(
    const float* in, float* out, long R, int F, int C,
    const int32_t* __restrict__ nframes, const float* __restrict__ shift,
    const float* __restrict__ scale, float lo, float hi) {
#pragma clang fp contract(off)
  const int CV = C / V;
  const long total = R * CV;
  for (long i = (long)blockIdx.x * FNORM_THREADS + threadIdx.x; i < total;
       i += (long)gridDim.x * FNORM_THREADS) {
    const long r = i / CV;
    const int c = (int)(i - r * CV) * V;
    const long b = r / F;
    const int f = (int)(r - b * F);
    int n = F;
    if (nframes) {
      n = nframes[b];
      n = n < 0 ? 0 : (n > F ? F : n);
    }
    const long o = r * C + c;
    if (V == 4) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (f < n) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(in + o);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + c);
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = x[e] - sh[e];
          const float w = d * sc[e];
          v[e] = w < lo ? lo : (w > hi ? hi : w);
        }
      }
      *reinterpret_cast<f32x4*>(out + o) = v;
    } else {
      float v = 0.f;
      if (f < n) {
        const float d = in[o] - shift[c];
        const float w = d * scale[c];
        v = w < lo ? lo : (w > hi ? hi : w);
      }
      out[o] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// Distance of two feature tensors (wavenet/features.py: frame_distance;
// tests/synth_ref.py restates it).  With d = a - b subtracted in float32 and
// widened to float64, per clip over its real frames:
//   abs = sum |d|,  sq = sum d * d,  rms = sum_f sqrt((sum_c d * d) / C)
//
// feature_distance_partials_kernel: workgroup (clip, k) owns the frames
// [k FDIST_TF, (k + 1) FDIST_TF) of its clip, cut at nframes; its four waves
// take the frames f0 + w, f0 + w + 4, ... in ascending order, one frame per
// trip.  Lane i takes the channels V i + 64 V j, j = 0, 1, ... (V = 4 where
// C % 4 == 0: one 16-byte load per input, else 1) and adds |d| and d * d into
// lane sums; the frame's sum over c is the xor butterfly (32, 16, ... 1) of
// the lanes' sums of that frame.  At the end the lane sums go through the
// same butterfly and the four waves are added in the order 0, 1, 2, 3.
// feature_distance_finish_kernel adds a clip's partials k = 0, 1, ... in
// order, from zero.  No atomics: a clip's three numbers are a function of its
// own bits, (F, C) and nframes[b]; an empty chunk adds exact zeros.  Frames at
// or behind nframes[b] are not read.
// ---------------------------------------------------------------------------
#define FDIST_TF 64
#define FDIST_THREADS 256

__device__ __forceinline__ double fdist_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int V>
__global__ __launch_bounds__(FDIST_THREADS) void feature_distance_partials_kernel(
    const float* __restrict__ a, const float* __restrict__ b, int F, int C,
    const int32_t* __restrict__ nframes, int nchunk,
    double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double red[3 * (FDIST_THREADS / 64)];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long clip = blockIdx.x / nchunk;
  const int f0 = (int)(blockIdx.x - clip * nchunk) * FDIST_TF;
  int n = F;
  if (nframes) {
    n = nframes[clip];
    n = n < 0 ? 0 : (n > F ? F : n);
  }
  const int f1 = n < f0 + FDIST_TF ? n : f0 + FDIST_TF;
  double sa = 0.0, ss = 0.0, sr = 0.0;
  // (wave-uniform trips: every lane takes part in the butterfly)
  for (int f = f0 + wave; f < f1; f += FDIST_THREADS / 64) {
    const long o = (clip * F + f) * C;
    double q = 0.0;
    for (int c = lane * V; c < C; c += 64 * V) {
      if (V == 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(a + o + c);
        const f32x4 y = *reinterpret_cast<const f32x4*>(b + o + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double w = (double)(x[e] - y[e]);
          sa += fabs(w);
          q += w * w;
        }
      } else {
        const double w = (double)(a[o + c] - b[o + c]);
        sa += fabs(w);
        q += w * w;
      }
    }
    ss += q;
    sr += sqrt(fdist_wave_sum(q) / (double)C);
  }
  sa = fdist_wave_sum(sa);
  ss = fdist_wave_sum(ss);
  if (lane == 0) {
    red[3 * wave] = sa;
    red[3 * wave + 1] = ss;
    red[3 * wave + 2] = sr;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = 0.0;
    for (int w = 0; w < FDIST_THREADS / 64; ++w) t += red[3 * w + threadIdx.x];
    partials[(long)blockIdx.x * 3 + threadIdx.x] = t;
  }
}

__global__ void feature_distance_finish_kernel(const double* __restrict__ partials,
                                               int B, int nchunk,
                                               double* __restrict__ abs_sum,
                                               double* __restrict__ sq_sum,
                                               double* __restrict__ rms_sum) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* p = partials + (long)b * nchunk * 3;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0;
  for (int k = 0; k < nchunk; ++k) {
    t0 += p[3 * k];
    t1 += p[3 * k + 1];
    t2 += p[3 * k + 2];
  }
  abs_sum[b] = t0;
  sq_sum[b] = t1;
  rms_sum[b] = t2;
}

// ---------------------------------------------------------------------------
// Pre-emphasis and de-emphasis (wavenet/emphasis.py states both rules;
// tests/emph_ref.py restates the recurrence in float64).
//
// preemphasis_kernel: out[t] = in[t] - float32(alpha * in[t - 1]), two
// roundings (emph_mul / emph_sub: the FMA contraction is off), in[-1] = 0; exact zeros at t >= n[b], which are not read.
//
// deemphasis_kernel: y[t] = in[t] + alpha * y[t - 1] as a blocked scan.  One
// workgroup of 256 lanes owns a clip and walks it in chunks of EMPH_CHUNK =
// 256 * EMPH_RUN samples counted from the clip's first sample; `carry`, the y
// in front of the chunk, is a scalar kept across the loop.  In a chunk:
//   1. the samples are staged into LDS (coalesced; zeros behind the clip);
//   2. lane g runs its EMPH_RUN samples sequentially from zero:
//        l[0] = x[0], l[j] = x[j] + alpha * l[j - 1];  b[g] = l[EMPH_RUN - 1];
//   3. the lanes' affine maps y -> alpha^RUN y + b[g] are scanned.  Every map
//      has the same slope, so the scan carries the offsets alone and takes
//      the slopes' products alpha^(RUN k) from a table: s = inclusive scan of
//      b inside the wave by DPP (row shifts 1, 2, 4, 8, then lane 15 / lane 31
//      broadcast to the following rows), the four waves' totals chained in
//      wave order, G[g] = s[g] + alpha^(RUN (lane + 1)) * (y in front of the
//      wave): the y at the end of lane g's run;
//   4. the y in front of lane g's run, X[g] = b[g - 1] + alpha^RUN * G[g - 2]
//      (X[0] = carry, X[1] = b[0] + alpha^RUN * carry): the neighbouring
//      run's samples reach it through ONE more addition, not through the
//      scan's, so that a sample k places back has passed through fewer than
//      2 k + 3 roundings wherever it sits (tests/emph_ref.py: the bound);
//   5. the fix-up y[j] = l[j] + alpha^(j + 1) * X[g], back through LDS; the
//      next chunk's carry is the chunk's last y as it is written, so a clip
//      cut at a multiple of the chunk, with last -> initial, gives the bits
//      of one call.
// The tables alpha^j (j <= RUN) and alpha^(RUN k) (k <= 64) are computed by
// the host in double and rounded once.  No atomics; the order of every
// operation is a function of the sample's position in its clip: a clip's
// bits depend on its samples, alpha and initial[b] alone.  alpha == 0 copies.
// ---------------------------------------------------------------------------
#define EMPH_RUN 16
#define EMPH_THREADS 256
#define EMPH_CHUNK (EMPH_RUN * EMPH_THREADS)
#define EMPH_SLOTS (EMPH_CHUNK + EMPH_THREADS)   // one pad float per run

struct EmphTables {
  float pw[EMPH_RUN + 1];     // alpha^j
  float pl[65];               // alpha^(RUN k)
};

// one rounding each: plain operators with the FMA contraction off (the _rn
// intrinsics inline library code that carries its own contraction flags, and
// the product and the sum were fused: several ulps off the numpy rule)
__device__ __forceinline__ float emph_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float emph_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float emph_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

__global__ __launch_bounds__(256) void preemphasis_kernel(
    const float* __restrict__ in, float* __restrict__ out, long ld_in,
    long ld_out, int B, int T, const int32_t* __restrict__ lengths,
    float alpha) {
#pragma clang fp contract(off)
  const long total = (long)B * T;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (long)gridDim.x * 256) {
    const long b = i / T;
    const int t = (int)(i - b * T);
    int n = T;
    if (lengths) {
      n = lengths[b];
      n = n < 0 ? 0 : (n > T ? T : n);
    }
    float v = 0.f;
    if (t < n) {
      const float* p = in + b * ld_in + t;
      v = p[0];
      if (alpha != 0.f)
        v = emph_sub(v, emph_mul(alpha, t > 0 ? p[-1] : 0.f));
    }
    out[b * ld_out + t] = v;
  }
}

__global__ __launch_bounds__(EMPH_THREADS) void deemphasis_kernel(
    const float* in, float* out, long ld_in, long ld_out, int T,
    const int32_t* __restrict__ lengths, const float* __restrict__ initial,
    float* __restrict__ last, float alpha, EmphTables tb) {
#pragma clang fp contract(off)
  __shared__ float xs[EMPH_SLOTS];
  __shared__ float cy;                      // the chunk's last y
  __shared__ float pw[EMPH_RUN + 1];
  __shared__ float pl[65];
  __shared__ float Bs[EMPH_THREADS], Gs[EMPH_THREADS], wt[EMPH_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long b = blockIdx.x;
  int n = T;
  if (lengths) {
    n = lengths[b];
    n = n < 0 ? 0 : (n > T ? T : n);
  }
  const float* src = in + b * ld_in;
  float* dst = out + b * ld_out;
  float carry = initial ? initial[b] : 0.f;

  if (alpha == 0.f) {                       // the identity, bit for bit
    for (int t = tid; t < n; t += EMPH_THREADS) dst[t] = src[t];
    if (last && tid == 0 && n > 0) last[b] = src[n - 1];
  } else {
    if (tid <= EMPH_RUN) pw[tid] = tb.pw[tid];
    if (tid < 65) pl[tid] = tb.pl[tid];
    for (int c0 = 0; c0 < n; c0 += EMPH_CHUNK) {      // (workgroup-uniform)
      const int m = min(EMPH_CHUNK, n - c0);
      __syncthreads();                      // the previous chunk's stores
#pragma unroll
      for (int k = 0; k < EMPH_RUN; ++k) {
        const int s = tid + k * EMPH_THREADS;
        xs[s + (s >> 4)] = s < m ? src[c0 + s] : 0.f;
      }
      __syncthreads();
      float* mine = xs + tid * (EMPH_RUN + 1);
      float l[EMPH_RUN];
      l[0] = mine[0];
#pragma unroll
      for (int j = 1; j < EMPH_RUN; ++j)
        l[j] = emph_add(mine[j], emph_mul(alpha, l[j - 1]));
      const float bl = l[EMPH_RUN - 1];
      // inclusive scan of the runs' ends over the wave
      float s = bl;
      s = emph_add(s, emph_mul(pl[1], dpp_f32<0x111, 0xf>(0.f, s)));
      s = emph_add(s, emph_mul(pl[2], dpp_f32<0x112, 0xf>(0.f, s)));
      s = emph_add(s, emph_mul(pl[4], dpp_f32<0x114, 0xf>(0.f, s)));
      s = emph_add(s, emph_mul(pl[8], dpp_f32<0x118, 0xf>(0.f, s)));
      s = emph_add(s, emph_mul(pl[(lane & 15) + 1], dpp_f32<0x142, 0xa>(0.f, s)));
      s = emph_add(s, emph_mul(pl[(lane & 31) + 1], dpp_f32<0x143, 0xc>(0.f, s)));
      if (lane == 63) wt[wave] = s;
      __syncthreads();
      float v = carry;                      // the y in front of this wave
      for (int w = 0; w < wave; ++w)
        v = emph_add(wt[w], emph_mul(pl[64], v));
      Bs[tid] = bl;
      Gs[tid] = emph_add(s, emph_mul(pl[lane + 1], v));
      __syncthreads();
      float x = carry;                      // the y in front of this run
      if (tid >= 1)
        x = emph_add(Bs[tid - 1], emph_mul(pl[1], tid >= 2 ? Gs[tid - 2] : carry));
#pragma unroll
      for (int j = 0; j < EMPH_RUN; ++j)
        mine[j] = emph_add(l[j], emph_mul(pw[j + 1], x));
      if (tid == EMPH_THREADS - 1) cy = mine[EMPH_RUN - 1];
      __syncthreads();
      carry = cy;                           // (the y a next piece starts from)
#pragma unroll
      for (int k = 0; k < EMPH_RUN; ++k) {
        const int s2 = tid + k * EMPH_THREADS;
        if (s2 < m) {
          const float y = xs[s2 + (s2 >> 4)];
          dst[c0 + s2] = y;
          if (last && c0 + s2 == n - 1) last[b] = y;
        }
      }
    }
  }
  if (last && n == 0 && tid == 0) last[b] = carry;
  for (int t = n + tid; t < T; t += EMPH_THREADS) dst[t] = 0.f;
}

static int emph_check(const void* in, const void* out, long ld_in, long ld_out,
                      int B, int T, const int32_t* lengths, float alpha) {
  if (!in || !out) return WN_ERR_NULL;
  if (B < 1 || T < 1 || ld_in < T || ld_out < T || !(alpha >= 0.f) ||
      !(alpha < 1.f))
    return WN_ERR_BAD_SHAPE;
  if ((reinterpret_cast<uintptr_t>(in) & 3u) || (reinterpret_cast<uintptr_t>(out) & 3u) ||
      (reinterpret_cast<uintptr_t>(lengths) & 3u))
    return WN_ERR_MISALIGNED;
  return WN_OK;
}

// the shape and alignment rules the entries share (`a`, `b`: the float
// buffers of [B][F][C]; b may be NULL)
static int feat_check(const void* a, const void* b, int B, int F, int C,
                      const int32_t* nframes) {
  if (C < 1 || C > FEAT_MAX_C || B < 1 || F < 1 ||
      (long)B * (long)F > 2147483647L)
    return WN_ERR_BAD_SHAPE;
  const uintptr_t m = (C % 4 == 0) ? 15u : 3u;
  if ((reinterpret_cast<uintptr_t>(a) & m) || (reinterpret_cast<uintptr_t>(b) & m) ||
      (reinterpret_cast<uintptr_t>(nframes) & 3u))
    return WN_ERR_MISALIGNED;
  return WN_OK;
}

extern "C" {

int wn_melspec(const float* audio, long ld, int B, int T, const int32_t* lengths,
               const float* window, const float* basis, const float* melw,
               int n_fft, int hop, int n_bins, int n_mels, float floor_,
               float* out, void* stream) {
  if (!audio || !window || !basis || !melw || !out) return WN_ERR_NULL;
  if (n_fft < 64 || n_fft > MEL_MAX_FFT || n_fft % 64 != 0 || hop < 1 ||
      hop > n_fft || n_bins != n_fft / 2 + 1 || n_mels < 1 ||
      n_mels > MEL_MAX_MELS || !(floor_ > 0.f) || !(floor_ < INFINITY) ||
      B < 1 || B > 65535 || T < 1 || T > (1 << 30) || ld < T)
    return WN_ERR_BAD_SHAPE;
  if (!wn_aligned16(basis) || !wn_aligned16(melw) || !wn_aligned16(out) ||
      (reinterpret_cast<uintptr_t>(audio) & 3u) ||
      (reinterpret_cast<uintptr_t>(window) & 3u) ||
      (reinterpret_cast<uintptr_t>(lengths) & 3u))
    return WN_ERR_MISALIGNED;
  MelArgs a;
  a.audio = audio;
  a.ld = ld;
  a.lengths = lengths;
  a.window = window;
  a.basis = basis;
  a.melw = melw;
  a.out = out;
  a.T = T;
  a.F = (T + hop - 1) / hop;
  a.n_fft = n_fft;
  a.hop = hop;
  a.NC = (n_bins + 31) / 32;
  a.n_mels = n_mels;
  a.MP = (n_mels + 31) / 32 * 32;
  a.pad = (hop & 1) ? 0 : 1;
  a.floor_ = floor_;
  const long total = (long)(MEL_TF - 1) * hop + n_fft;
  const long nstage = total + a.pad * ((total - 1) / hop) + 1;
  const bool staged = nstage <= MEL_STAGE_MAX;
  const size_t lds = sizeof(float) * (size_t)(MEL_RING + 2 * n_fft + (staged ? nstage : 0));
  return staged ? mel_launch<true>(a, B, lds, (hipStream_t)stream)
                : mel_launch<false>(a, B, lds, (hipStream_t)stream);
}

int wn_feature_stats_partials_count(void) { return FSTAT_PARTS; }

int wn_feature_stats(const float* fr, int B, int F, int C, const int32_t* nframes,
                     double* acc, double* partials, void* stream) {
  if (!fr || !acc || !partials) return WN_ERR_NULL;
  const int rc = feat_check(fr, nullptr, B, F, C, nframes);
  if (rc != WN_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(acc) & 7u) || (reinterpret_cast<uintptr_t>(partials) & 7u))
    return WN_ERR_MISALIGNED;
  const long R = (long)B * F;
  const long per = (R + FSTAT_PARTS - 1) / FSTAT_PARTS;
  const int V = (C % 4 == 0) ? 4 : 1;
  int L = 1;
  while (L < (C + V - 1) / V && L < FSTAT_THREADS) L <<= 1;
  hipStream_t s = (hipStream_t)stream;
  if (V == 4)
    hipLaunchKernelGGL(feature_stats_partials_kernel<4>, dim3(FSTAT_PARTS),
                       dim3(FSTAT_THREADS), 0, s, fr, R, F, C, nframes, per, L, partials);
  else
    hipLaunchKernelGGL(feature_stats_partials_kernel<1>, dim3(FSTAT_PARTS),
                       dim3(FSTAT_THREADS), 0, s, fr, R, F, C, nframes, per, L, partials);
  if (wn_check_launch() != WN_OK) return WN_ERR_LAUNCH;
  hipLaunchKernelGGL(feature_stats_finish_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, s,
                     partials, C, acc);
  return wn_check_launch();
}

int wn_feature_normalize(const float* in, float* out, int B, int F, int C,
                         const int32_t* nframes, const float* shift, const float* scale,
                         float lo, float hi, void* stream) {
  if (!in || !out || !shift || !scale) return WN_ERR_NULL;
  int rc = feat_check(in, out, B, F, C, nframes);
  if (rc != WN_OK) return rc;
  if (!(lo <= hi)) return WN_ERR_BAD_SHAPE;    // (lo > hi, or a NaN bound)
  const int V = (C % 4 == 0) ? 4 : 1;
  const uintptr_t m = V == 4 ? 15u : 3u;
  if ((reinterpret_cast<uintptr_t>(shift) & m) || (reinterpret_cast<uintptr_t>(scale) & m))
    return WN_ERR_MISALIGNED;
  const long R = (long)B * F;
  const long total = R * (C / V);
  long blocks = (total + FNORM_THREADS - 1) / FNORM_THREADS;
  if (blocks > 4096) blocks = 4096;
  hipStream_t s = (hipStream_t)stream;
  if (V == 4)
    hipLaunchKernelGGL(feature_normalize_kernel<4>, dim3((unsigned)blocks), dim3(FNORM_THREADS),
                       0, s, in, out, R, F, C, nframes, shift, scale, lo, hi);
  else
    hipLaunchKernelGGL(feature_normalize_kernel<1>, dim3((unsigned)blocks), dim3(FNORM_THREADS),
                       0, s, in, out, R, F, C, nframes, shift, scale, lo, hi);
  return wn_check_launch();
}

long wn_feature_distance_partials(int B, int F) {
  if (B < 1 || F < 1 || (long)B * (long)F > 2147483647L) return -1;
  return 3L * B * ((F + FDIST_TF - 1) / FDIST_TF);
}

int wn_feature_distance(const float* a, const float* b, int B, int F, int C,
                        const int32_t* nframes, double* abs_sum, double* sq_sum,
                        double* rms_sum, double* partials, void* stream) {
  if (!a || !b || !abs_sum || !sq_sum || !rms_sum || !partials) return WN_ERR_NULL;
  const int rc = feat_check(a, b, B, F, C, nframes);
  if (rc != WN_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(abs_sum) & 7u) ||
      (reinterpret_cast<uintptr_t>(sq_sum) & 7u) ||
      (reinterpret_cast<uintptr_t>(rms_sum) & 7u) ||
      (reinterpret_cast<uintptr_t>(partials) & 7u))
    return WN_ERR_MISALIGNED;
  const int nchunk = (F + FDIST_TF - 1) / FDIST_TF;
  const unsigned grid = (unsigned)((long)B * nchunk);   // (<= B F <= 2^31 - 1)
  hipStream_t s = (hipStream_t)stream;
  if (C % 4 == 0)
    hipLaunchKernelGGL(feature_distance_partials_kernel<4>, dim3(grid),
                       dim3(FDIST_THREADS), 0, s, a, b, F, C, nframes, nchunk, partials);
  else
    hipLaunchKernelGGL(feature_distance_partials_kernel<1>, dim3(grid),
                       dim3(FDIST_THREADS), 0, s, a, b, F, C, nframes, nchunk, partials);
  if (wn_check_launch() != WN_OK) return WN_ERR_LAUNCH;
  hipLaunchKernelGGL(feature_distance_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, s,
                     partials, B, nchunk, abs_sum, sq_sum, rms_sum);
  return wn_check_launch();
}

int wn_emphasis_chunk(void) { return EMPH_CHUNK; }

int wn_preemphasis(const float* in, float* out, long ld_in, long ld_out, int B,
                   int T, const int32_t* lengths, float alpha, void* stream) {
  const int rc = emph_check(in, out, ld_in, ld_out, B, T, lengths, alpha);
  if (rc != WN_OK) return rc;
  // a neighbour's input would be overwritten: the buffers must not overlap
  const float* in_end = in + (long)(B - 1) * ld_in + T;
  const float* out_end = out + (long)(B - 1) * ld_out + T;
  if (in < out_end && out < in_end) return WN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(preemphasis_kernel, dim3(grid1d((long)B * T, 256, 4096)),
                     dim3(256), 0, (hipStream_t)stream, in, out, ld_in, ld_out,
                     B, T, lengths, alpha);
  return wn_check_launch();
}

int wn_deemphasis(const float* in, float* out, long ld_in, long ld_out, int B,
                  int T, const int32_t* lengths, const float* initial,
                  float* last, float alpha, void* stream) {
  const int rc = emph_check(in, out, ld_in, ld_out, B, T, lengths, alpha);
  if (rc != WN_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(initial) & 3u) || (reinterpret_cast<uintptr_t>(last) & 3u))
    return WN_ERR_MISALIGNED;
  // out may be in itself; any other overlap would mix two clips
  if (in != out) {
    const float* in_end = in + (long)(B - 1) * ld_in + T;
    const float* out_end = out + (long)(B - 1) * ld_out + T;
    if (in < out_end && out < in_end) return WN_ERR_UNSUPPORTED;
  } else if (ld_in != ld_out) {
    return WN_ERR_UNSUPPORTED;
  }
  EmphTables tb;
  const double a = (double)alpha;
  for (int j = 0; j <= EMPH_RUN; ++j) tb.pw[j] = (float)pow(a, (double)j);
  for (int k = 0; k <= 64; ++k) tb.pl[k] = (float)pow(a, (double)(EMPH_RUN * k));
  hipLaunchKernelGGL(deemphasis_kernel, dim3((unsigned)B), dim3(EMPH_THREADS), 0,
                     (hipStream_t)stream, in, out, ld_in, ld_out, T, lengths,
                     initial, last, alpha, tb);
  return wn_check_launch();
}

}  // extern "C"
