// Mixture-of-logistics output head over 65536 levels (include/wavenet_mol.h
// states every operation): the level rule, the row loss with its gradient in
// place of wn_xent*, held-out scoring on the same row arithmetic, one row's
// parameters and the sampling draw.
#include "wn_common.h"
#include "wn_mol_draw.h"     // MOL_TOP, MOL_MAXK, mol_centre, the two row rules
#include <cmath>

#pragma clang fp contract(off)

#define MOL_TILE 64          // rows of a workgroup's tile: four lanes per row
#define MOL_MAXSTRIDE 100    // floats between a tile's rows in LDS, at most
#define MOL_CLIP_THREADS 1024

extern "C" int wn_xent_partials(long rows);

__device__ __forceinline__ int mol_clip_len(const int32_t* lengths, long b,
                                            int T) {
  return lengths ? min(max(lengths[b], 0), T) : T;
}
__device__ __forceinline__ int mol_clip_start(const int32_t* starts, long b,
                                              int T) {
  return starts ? min(max(starts[b], 0), T) : 0;
}

__device__ __forceinline__ int mol_level(float y) {
  y = fminf(fmaxf(y, -1.f), 1.f);
  float t = y + 1.f;
  t = t * 32767.5f;
  return (int)rintf(t);
}

// ---------------------------------------------------------------------------
// wn_mol_quantize: one lane per sample, grid stride
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mol_quantize_kernel(
    const float* audio, const int32_t* __restrict__ lengths,
    int32_t* __restrict__ levels, float* centres, long N, int T) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N;
       i += (long)gridDim.x * 256) {
    const int t = (int)(i % T);
    int j = 0;
    float c = 0.f;
    if (t < mol_clip_len(lengths, i / T, T)) {   // (behind n[b]: not read)
      j = mol_level(audio[i]);
      c = mol_centre(j);
    }
    levels[i] = j;
    centres[i] = c;
  }
}

// ---------------------------------------------------------------------------
// One component's log-probability of the target bin and its derivatives by mu
// and by beta.  edge: -1 (level 0), +1 (level C - 1), 0 (interior).
// ---------------------------------------------------------------------------
struct MolComp {
  double lp, dmu, dbeta;
};

// float64: the terms below differ by up to twelve orders of magnitude (a
// component e^-14 wide next to the 2 / 65535 bin), and a float32 chain of the
// dozen operations behind one gradient entry loses four to seven ulps
__device__ __forceinline__ MolComp mol_comp(double c, int edge, double mu,
                                            double beta) {
  const double h = 1.0 / 65535.0, h2 = 2.0 / 65535.0;
  const double is = exp(-beta);
  const double d = c - mu;
  const double a = (d + h) * is, b = (d - h) * is;
  const double ea = exp(-fabs(a)), eb = exp(-fabs(b));
  const double spa = fmax(-a, 0.0) + log1p(ea);        // softplus(-a)
  const double spb = fmax(b, 0.0) + log1p(eb);         // softplus(b)
  const double sna = a <= 0.0 ? 1.0 / (1.0 + ea) : ea / (1.0 + ea);
  const double sb = b >= 0.0 ? 1.0 / (1.0 + eb) : eb / (1.0 + eb);
  MolComp o;
  if (edge < 0) {
    o.lp = -spa;
    o.dmu = -(is * sna);
    o.dbeta = -(a * sna);
  } else if (edge > 0) {
    o.lp = -spb;
    o.dmu = is * sb;
    o.dbeta = b * sb;
  } else {
    const double D = h2 * is;
    // log(1 - e^-D); below 1 as log D + log((1 - e^-D) / D), log D = log h2 -
    // beta: finite where e^-beta has underflowed
    const double lt = D >= 1.0 ? log(-expm1(-D))
                               : (log(h2) - beta) +
                                     log(D > 0.0 ? -expm1(-D) / D : 1.0);
    const double gt = D > 0.0 ? D / expm1(D) : 1.0;
    o.lp = (-spa - spb) + lt;
    o.dmu = is * (sb - sna);
    o.dbeta = (b * sb - a * sna) - gt;
  }
  return o;
}

// sums and maxima over a row's four lanes (the same bits in each of them)
__device__ __forceinline__ double quad_sum(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v;
}
__device__ __forceinline__ double quad_max(double v) {
  v = fmax(v, __shfl_xor(v, 1));
  return fmax(v, __shfl_xor(v, 2));
}

// ---------------------------------------------------------------------------
// The rows: a workgroup takes tiles of 64 rows.  A tile's 3 Kp columns come in
// with 16-byte loads, whole rows at a time, and are staged in LDS (rows an odd
// number of 16-byte slots apart, so that the eight rows of a half-wave fall on
// different banks); four lanes share a row, lane s holding the components k =
// 4 i + s.  The gradient is written over the staged row and leaves the same
// way the logits came, so dlogits may be logits.
// SCORE: out[row] = the row's nll (0 without a target), flag[row] = 1 | 0.
// else:  out[blockIdx.x] = the sum of the workgroup's rows.
// ---------------------------------------------------------------------------
template <bool SCORE>
__global__ __launch_bounds__(256) void mol_rows_kernel(
    const float* logits, long ld, const int32_t* __restrict__ levels,
    const int32_t* __restrict__ starts, const int32_t* __restrict__ lengths,
    const float* __restrict__ inv_den, float inv_n, float* dlogits,
    float* __restrict__ out, int32_t* __restrict__ flag, long rows, int T,
    int K, float lsm) {
  __shared__ __attribute__((aligned(16))) float tile[MOL_TILE * MOL_MAXSTRIDE];
  __shared__ double wsum[4];
  const int Kp = (K + 3) & ~3, W4 = 3 * Kp / 4, nk = Kp / 4;
  const int stride = ((W4 + 1) | 1) * 4;
  const int tid = threadIdx.x, r = tid >> 2, s = tid & 3;
  const double inv = (double)(inv_den ? *inv_den : inv_n);
  const long ntiles = (rows + MOL_TILE - 1) / MOL_TILE;
  double lsum = 0.0;
  for (long ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const long row0 = ti * MOL_TILE;
    const int nr = (int)min((long)MOL_TILE, rows - row0);
    for (int c = tid; c < nr * W4; c += 256) {
      const int rr = c / W4, cc = c - rr * W4;
      *reinterpret_cast<f32x4*>(tile + rr * stride + cc * 4) =
          *reinterpret_cast<const f32x4*>(logits + (row0 + rr) * ld + cc * 4);
    }
    __syncthreads();
    const long row = row0 + r;
    float* tr = tile + r * stride;
    bool has = false;
    int j = 0;
    if (r < nr) {
      const int t = (int)(row % T);
      const long b = row / T;
      if (t + 1 < mol_clip_len(lengths, b, T) &&
          t + 1 >= mol_clip_start(starts, b, T)) {
        j = levels[row + 1];
        has = j >= 0 && j <= MOL_TOP;
      }
    }
    float nll = 0.f;
    if (has) {                       // (the same in the row's four lanes)
      const double c = (double)(2 * j - MOL_TOP) / 65535.0;
      const int edge = j == 0 ? -1 : j == MOL_TOP ? 1 : 0;
      double pi[8], w[8], dmu[8], dbe[8];
      double mp = -INFINITY;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = 4 * i + s;
        pi[i] = -INFINITY;
        w[i] = -INFINITY;
        dmu[i] = dbe[i] = 0.0;
        if (k < K) {
          pi[i] = (double)tr[k];
          const float braw = tr[2 * Kp + k];
          const MolComp o = mol_comp(c, edge, (double)tr[Kp + k],
                                     (double)fmaxf(braw, lsm));
          w[i] = o.lp;
          dmu[i] = o.dmu;
          dbe[i] = braw < lsm ? 0.0 : o.dbeta;
          mp = fmax(mp, pi[i]);
        }
      }
      mp = quad_max(mp);
      double sp = 0.0;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (4 * i + s < K) {
          pi[i] = pi[i] - mp;
          sp += exp(pi[i]);
        }
      sp = quad_sum(sp);
      const double lsp = log(sp);
      double mw = -INFINITY;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (4 * i + s < K) {
          w[i] = (pi[i] - lsp) + w[i];
          mw = fmax(mw, w[i]);
        }
      mw = quad_max(mw);
      double sw = 0.0;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (4 * i + s < K) {
          w[i] = exp(w[i] - mw);
          sw += w[i];
        }
      sw = quad_sum(sw);
      nll = (float)-(mw + log(sw));
      if (!SCORE && dlogits) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int k = 4 * i + s;
          if (k < K) {
            const double rk = w[i] / sw, pk = exp(pi[i]) / sp;
            tr[k] = (float)((pk - rk) * inv);
            tr[Kp + k] = (float)(-(rk * dmu[i]) * inv);
            tr[2 * Kp + k] = (float)(-(rk * dbe[i]) * inv);
          } else if (i < nk) {
            tr[k] = tr[Kp + k] = tr[2 * Kp + k] = 0.f;
          }
        }
      }
      // (the float32 row, as wn_mol_score stores it)
      if (!SCORE && s == 0) lsum += (double)nll;
    } else if (!SCORE && dlogits && r < nr) {
      for (int i = 0; i < nk; ++i) {
        const int k = 4 * i + s;
        tr[k] = tr[Kp + k] = tr[2 * Kp + k] = 0.f;
      }
    }
    if (SCORE && r < nr && s == 0) {
      out[row] = nll;
      flag[row] = has ? 1 : 0;
    }
    __syncthreads();
    if (!SCORE && dlogits) {
      for (int c = tid; c < nr * W4; c += 256) {
        const int rr = c / W4, cc = c - rr * W4;
        *reinterpret_cast<f32x4*>(dlogits + (row0 + rr) * ld + cc * 4) =
            *reinterpret_cast<const f32x4*>(tile + rr * stride + cc * 4);
      }
      __syncthreads();
    }
  }
  if (!SCORE) {
    // lanes s = 0 hold their rows' terms, the others +0: one fixed order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) lsum += __shfl_xor(lsum, o);
    if ((tid & 63) == 0) wsum[tid >> 6] = lsum;
    __syncthreads();
    if (tid == 0)
      out[blockIdx.x] = (float)((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
  }
}

// per-clip sums of the scored rows: xent_score_clips_kernel's order (thread i
// sums rows i, i + 1024, ... in float64, a fixed LDS tree finishes)
__global__ __launch_bounds__(MOL_CLIP_THREADS) void mol_score_clips_kernel(
    const float* __restrict__ nll, const int32_t* __restrict__ flag,
    const int32_t* __restrict__ starts, const int32_t* __restrict__ lengths,
    double* __restrict__ clip_nll, int32_t* __restrict__ clip_count, int T) {
  __shared__ double rs[MOL_CLIP_THREADS];
  __shared__ int rc[MOL_CLIP_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = mol_clip_len(lengths, b, T);
  const float* pn = nll + (long)b * T;
  const int32_t* pf = flag + (long)b * T;
  double sum = 0.0;
  int cnt = 0;
  const int t0 = max(mol_clip_start(starts, b, T) - 1, 0);
  for (int t = t0 + tid; t < len - 1; t += MOL_CLIP_THREADS) {
    sum += (double)pn[t];
    cnt += pf[t];
  }
  rs[tid] = sum;
  rc[tid] = cnt;
  __syncthreads();
  for (int k = MOL_CLIP_THREADS / 2; k > 0; k >>= 1) {
    if (tid < k) {
      rs[tid] += rs[tid + k];
      rc[tid] += rc[tid + k];
    }
    __syncthreads();
  }
  if (tid == 0) {
    clip_nll[b] = rs[0];
    clip_count[b] = rc[0];
  }
}

// one row's parameters; lane k < K serves component k (wn_mol_draw.h)
__global__ __launch_bounds__(64) void mol_params_row_kernel(
    const float* __restrict__ row, int K, float lsm, float* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= K) return;
  mol_params_component(row, K, lsm, k, out);
}

// the draw, a lane per row, float64 (wn_mol_draw.h)
__global__ __launch_bounds__(64) void mol_sample_kernel(
    const float* __restrict__ params, const uint64_t* __restrict__ seeds,
    const uint64_t* __restrict__ counters, float temperature,
    int32_t* __restrict__ levels, float* __restrict__ centres, int R, int K) {
  const long r = (long)blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const int j = mol_draw_level(params + r * 3 * K, K, seeds[r], counters[r],
                               temperature);
  levels[r] = j;
  centres[r] = mol_centre(j);
}

static inline bool mol_al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

static int mol_rows_checks(const float* logits, long ld, const float* dlogits,
                           int B, int T, int K, float lsm) {
  if (B <= 0 || T <= 0 || (long)B * T >= (1L << 31)) return WN_ERR_BAD_SHAPE;
  if (K < 1 || K > MOL_MAXK || !(lsm >= -32.f && lsm <= -1.f))
    return WN_ERR_BAD_SHAPE;
  const int Kp = (K + 3) & ~3;
  if (ld < 3 * Kp || (ld & 3)) return WN_ERR_UNSUPPORTED;
  if (!wn_aligned16(logits) || (dlogits && !wn_aligned16(dlogits)))
    return WN_ERR_MISALIGNED;
  return WN_OK;
}

extern "C" {

int wn_mol_quantize(const float* audio, const int32_t* lengths,
                    int32_t* levels_out, float* centres_out, int B, int T,
                    void* stream) {
  if (!audio || !levels_out || !centres_out) return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || (long)B * T >= (1L << 31)) return WN_ERR_BAD_SHAPE;
  if (!mol_al4(audio) || !mol_al4(lengths) || !mol_al4(levels_out) ||
      !mol_al4(centres_out))
    return WN_ERR_MISALIGNED;
  const long N = (long)B * T;
  hipLaunchKernelGGL(mol_quantize_kernel, dim3(grid1d(N, 256)), dim3(256), 0,
                     (hipStream_t)stream, audio, lengths, levels_out,
                     centres_out, N, T);
  return wn_check_launch();
}

int wn_mol_loss(const float* logits, long ld, const int32_t* levels,
                const int32_t* starts, const int32_t* lengths,
                const float* inv_den, float* dlogits, float* loss_partials,
                int B, int T, int K, float log_scale_min, void* stream) {
  if (!logits || !levels || !loss_partials) return WN_ERR_NULL;
  const int code = mol_rows_checks(logits, ld, dlogits, B, T, K, log_scale_min);
  if (code != WN_OK) return code;
  if (!mol_al4(levels) || !mol_al4(starts) || !mol_al4(lengths) ||
      !mol_al4(inv_den) || !mol_al4(loss_partials))
    return WN_ERR_MISALIGNED;
  const long rows = (long)B * T;
  hipLaunchKernelGGL(mol_rows_kernel<false>, dim3(wn_xent_partials(rows)),
                     dim3(256), 0, (hipStream_t)stream, logits, ld, levels,
                     starts, lengths, inv_den, 1.0f / (float)rows, dlogits,
                     loss_partials, (int32_t*)nullptr, rows, T, K,
                     log_scale_min);
  return wn_check_launch();
}

long wn_mol_score_scratch_floats(long rows) {
  return rows > 0 ? 2 * rows : 0;          // flags [rows], row values [rows]
}

int wn_mol_score(const float* logits, long ld, const int32_t* levels,
                 const int32_t* starts, const int32_t* lengths, float* row_nll,
                 double* clip_nll, int32_t* clip_count, float* scratch, int B,
                 int T, int K, float log_scale_min, void* stream) {
  if (!logits || !levels || !clip_nll || !clip_count || !scratch)
    return WN_ERR_NULL;
  const int code = mol_rows_checks(logits, ld, nullptr, B, T, K, log_scale_min);
  if (code != WN_OK) return code;
  if (!mol_al4(levels) || !mol_al4(starts) || !mol_al4(lengths) ||
      !mol_al4(row_nll) || ((uintptr_t)clip_nll & 7) || !mol_al4(clip_count) ||
      !mol_al4(scratch))
    return WN_ERR_MISALIGNED;
  const long rows = (long)B * T;
  int32_t* flag = reinterpret_cast<int32_t*>(scratch);
  float* nll = row_nll ? row_nll : scratch + rows;
  const long ntiles = (rows + MOL_TILE - 1) / MOL_TILE;
  hipLaunchKernelGGL(mol_rows_kernel<true>,
                     dim3((unsigned)(ntiles < 1024 ? ntiles : 1024)), dim3(256),
                     0, (hipStream_t)stream, logits, ld, levels, starts,
                     lengths, (const float*)nullptr, 0.f, (float*)nullptr, nll,
                     flag, rows, T, K, log_scale_min);
  hipLaunchKernelGGL(mol_score_clips_kernel, dim3(B), dim3(MOL_CLIP_THREADS),
                     0, (hipStream_t)stream, nll, flag, starts, lengths,
                     clip_nll, clip_count, T);
  return wn_check_launch();
}

int wn_mol_params_row(const float* logits_row, int K, float log_scale_min,
                      float* out, void* stream) {
  if (!logits_row || !out) return WN_ERR_NULL;
  if (K < 1 || K > MOL_MAXK || !(log_scale_min >= -32.f && log_scale_min <= -1.f))
    return WN_ERR_BAD_SHAPE;
  if (!mol_al4(logits_row) || !mol_al4(out)) return WN_ERR_MISALIGNED;
  hipLaunchKernelGGL(mol_params_row_kernel, dim3(1), dim3(64), 0,
                     (hipStream_t)stream, logits_row, K, log_scale_min, out);
  return wn_check_launch();
}

int wn_mol_sample(const float* params, const uint64_t* seeds,
                  const uint64_t* counters, float temperature,
                  int32_t* levels_out, float* centres_out, int R, int K,
                  void* stream) {
  if (!params || !seeds || !counters || !levels_out || !centres_out)
    return WN_ERR_NULL;
  if (R < 1 || K < 1 || K > MOL_MAXK || !(temperature >= 0.f) ||
      !(temperature <= 3.0e38f))
    return WN_ERR_BAD_SHAPE;
  if (!mol_al4(params) || ((uintptr_t)seeds & 7) || ((uintptr_t)counters & 7) ||
      !mol_al4(levels_out) || !mol_al4(centres_out))
    return WN_ERR_MISALIGNED;
  hipLaunchKernelGGL(mol_sample_kernel, dim3((R + 63) / 64), dim3(64), 0,
                     (hipStream_t)stream, params, seeds, counters, temperature,
                     levels_out, centres_out, R, K);
  return wn_check_launch();
}

}  // extern "C"
