// Device-resident training corpus (wavenet/corpus.py states the rule;
// tests/corpus_ref.py restates it in numpy): the trimmed utterances lie
// concatenated in one device buffer and every training batch is cut from it
// here.  The kernels derive the batch's plan themselves from device-resident
// tables and a few scalars, so a step sends nothing from the host:
//
//   slot  g = g0 + j, j < B;  epoch e = g / P;  item = perm[e - e0][g % P]
//   item  -> (utterance u, piece start); n_u = utt_len[u]
//   'pieces'  start = item_start, n = min(size, n_u - start)   (size 0: n_u)
//   'random'  n = min(size, n_u), start = draw_bits(seed ^ 'crop', g) %
//             (n_u - size + 1) when n_u > size, else 0
//   history H (the _hist entries; 0 elsewhere): h = min(H, start),
//             start' = start - h, n' = n + h: the piece with h samples of its
//             true left context in front; everything below uses (start', n')
//   n is cut to T.
//
// Both kernels are plain copies: a thread owns four consecutive floats of the
// (flat) output and writes them with one 16-byte store; it reads them with one
// 16-byte load where the four lie in one row, inside the slot's data and at a
// source index that is a multiple of four, and with guarded scalar loads
// otherwise (window starts are arbitrary: most rows begin unaligned; a wave's
// scalar loads are still consecutive addresses).  Nothing outside a slot's
// [start, start + n) -- hence nothing outside its utterance -- is read, and
// every output float is written: zeros behind n.  A table entry that points
// outside its table or buffer makes the slot empty (zeros), never a read.
#include "wn_common.h"

#define CORPUS_BLOCK 256
#define CORPUS_CROP_SALT 0x63726f70ull   // 'crop'

struct CorpusPlan {
  const int64_t* utt_off;     // [U] first sample of utterance u in the flat buffer
  const int32_t* utt_len;     // [U]
  const int32_t* item_utt;    // [P]
  const int32_t* item_start;  // [P]
  const int32_t* perm;        // [nE][P]: the orders of epochs e0 .. e0 + nE - 1
  long e0, g0;
  uint64_t seed;
  int U, P, nE, size, random, history;
};

struct CorpusSlot {
  long off;                   // utt_off[u]
  int u, start, n, nu, h;     // n == 0: an empty slot; h: history within n
};

__device__ __forceinline__ CorpusSlot corpus_slot(const CorpusPlan& p, long j, int T, long N) {
  CorpusSlot s = {0, -1, 0, 0, 0, 0};
  const long g = p.g0 + j;
  const long e = g / p.P, er = e - p.e0;
  const int r = (int)(g - e * p.P);
  if (er < 0 || er >= p.nE) return s;
  const int item = p.perm[er * p.P + r];
  if ((unsigned)item >= (unsigned)p.P) return s;
  const int u = p.item_utt[item];
  if ((unsigned)u >= (unsigned)p.U) return s;
  const int nu = p.utt_len[u];
  const long off = p.utt_off[u];
  if (nu <= 0 || off < 0 || off > N - nu) return s;
  int start = 0, n;
  if (p.random) {
    n = min(p.size, nu);
    if (nu > p.size)
      start = (int)(draw_bits(p.seed ^ CORPUS_CROP_SALT, (uint64_t)g) % (uint64_t)(nu - p.size + 1));
  } else {
    start = p.item_start[item];
    if (start < 0 || start >= nu) return s;
    n = nu - start;
    if (p.size > 0) n = min(n, p.size);
  }
  const int h = min(p.history, start);
  s.off = off;
  s.u = u;
  s.start = start - h;
  s.n = min(n + h, T);
  s.nu = nu;
  s.h = min(h, s.n);
  return s;
}

__device__ __forceinline__ void store4(float* out, long idx, long total, const f32x4& v) {
  if (idx + 3 < total) {
    *reinterpret_cast<f32x4*>(out + idx) = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (idx + k < total) out[idx + k] = v[k];
  }
}

// audio [B][T] <- flat
__global__ __launch_bounds__(CORPUS_BLOCK) void corpus_gather_kernel(
    const float* __restrict__ flat, long N, CorpusPlan p, float* __restrict__ out, int B, int T) {
  const long total = (long)B * T;
  for (long idx = 4 * ((long)blockIdx.x * CORPUS_BLOCK + threadIdx.x); idx < total;
       idx += 4L * gridDim.x * CORPUS_BLOCK) {
    long j = idx / T;
    int t = (int)(idx - j * T);
    CorpusSlot s = corpus_slot(p, j, T, N);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const long src = s.off + s.start + t;
    if (t + 3 < s.n && (src & 3) == 0) {          // (n <= T: one row)
      v = *reinterpret_cast<const f32x4*>(flat + src);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (idx + k < total) {
          if (t >= T) {                           // the next row begins
            t = 0;
            s = corpus_slot(p, ++j, T, N);
          }
          if (t < s.n) v[k] = flat[s.off + s.start + t];
          ++t;
        }
      }
    }
    store4(out, idx, total, v);
  }
}

// hist [B] <- h, lens [B] <- n of every slot (wn_corpus_gather_hist)
__global__ __launch_bounds__(CORPUS_BLOCK) void corpus_hist_kernel(
    long N, CorpusPlan p, int32_t* __restrict__ hist, int32_t* __restrict__ lens, int B, int T) {
  const long j = (long)blockIdx.x * CORPUS_BLOCK + threadIdx.x;
  if (j >= B) return;
  const CorpusSlot s = corpus_slot(p, j, T, N);
  hist[j] = s.h;
  lens[j] = s.n;
}

// what a slot reads of its utterance's frames [F][Lc]
struct FrameSlot {
  long base;                  // first frame of the utterance in the flat frames
  int F, lo, hi, start, n;    // window: frames [lo, hi); rows: samples [start, start + n)
};

__device__ __forceinline__ FrameSlot frame_slot(const CorpusPlan& p, const int64_t* fr_off,
                                                const int32_t* fr_len, long NF, int Lc, int hop,
                                                int ctx, long j, int T) {
  FrameSlot f = {0, 0, 0, 0, 0, 0};
  const CorpusSlot s = corpus_slot(p, j, T, INT64_MAX);
  if (s.n <= 0) return f;
  const long base = fr_off[s.u];
  const int F = fr_len[s.u];
  if (F <= 0 || base < 0 || base > NF / Lc - F) return f;
  f.base = base;
  f.F = F;
  f.start = s.start;
  f.n = s.n;
  f.lo = max(0, s.start / hop - ctx);
  f.hi = min(F, (s.start + s.n - 1) / hop + 1 + ctx);
  return f;
}

// the frame row r of the output takes, or -1 for zeros
template <bool ROWS>
__device__ __forceinline__ int frame_of(const FrameSlot& f, int r, int hop) {
  if (ROWS) {
    if (r >= f.n) return -1;
    const int fr = (f.start + r) / hop;
    return fr < f.F ? fr : -1;
  }
  const int fr = f.lo + r;
  return fr < f.hi ? fr : -1;
}

// out [B][R][Lc] <- the utterances' frames; ROWS: R = T, row t = frame
// (start + t) / hop, zeros behind n; else R = Fw, row r = frame f_lo + r
template <bool ROWS>
__global__ __launch_bounds__(CORPUS_BLOCK) void corpus_frames_kernel(
    const float* __restrict__ fr, long NF, const int64_t* __restrict__ fr_off,
    const int32_t* __restrict__ fr_len, CorpusPlan p, int hop, int ctx, int Lc,
    float* __restrict__ out, int B, int R, int T) {
  const long total = (long)B * R * Lc;
  for (long idx = 4 * ((long)blockIdx.x * CORPUS_BLOCK + threadIdx.x); idx < total;
       idx += 4L * gridDim.x * CORPUS_BLOCK) {
    const long q = idx / Lc;
    int c = (int)(idx - q * Lc);
    long j = q / R;
    int r = (int)(q - j * R);
    FrameSlot f = frame_slot(p, fr_off, fr_len, NF, Lc, hop, ctx, j, T);
    int ff = frame_of<ROWS>(f, r, hop);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const long src = (f.base + ff) * Lc + c;
    if (c + 3 < Lc && (ff < 0 || (src & 3) == 0)) {   // one row of the output
      if (ff >= 0) v = *reinterpret_cast<const f32x4*>(fr + src);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (idx + k < total) {
          if (c >= Lc) {                              // the next row begins
            c = 0;
            if (++r >= R) {
              r = 0;
              f = frame_slot(p, fr_off, fr_len, NF, Lc, hop, ctx, ++j, T);
            }
            ff = frame_of<ROWS>(f, r, hop);
          }
          if (ff >= 0) v[k] = fr[(f.base + ff) * Lc + c];
          ++c;
        }
      }
    }
    store4(out, idx, total, v);
  }
}

static int corpus_plan(CorpusPlan& p, const int64_t* utt_off, const int32_t* utt_len, int U,
                       const int32_t* item_utt, const int32_t* item_start, int P,
                       const int32_t* perm, long e0, int nE, long g0, int size, int random,
                       uint64_t seed, int history, int B) {
  if (!utt_off || !utt_len || !item_utt || !item_start || !perm) return WN_ERR_NULL;
  if (U <= 0 || P <= 0 || nE <= 0 || e0 < 0 || g0 < 0 || size < 0 || (random && size < 1) || history < 0 ||
      g0 / P < e0 || (g0 + B - 1) / P >= e0 + nE)
    return WN_ERR_BAD_SHAPE;
  if ((reinterpret_cast<uintptr_t>(utt_off) & 7u) || (reinterpret_cast<uintptr_t>(utt_len) & 3u) ||
      (reinterpret_cast<uintptr_t>(item_utt) & 3u) ||
      (reinterpret_cast<uintptr_t>(item_start) & 3u) || (reinterpret_cast<uintptr_t>(perm) & 3u))
    return WN_ERR_MISALIGNED;
  p.utt_off = utt_off;
  p.utt_len = utt_len;
  p.item_utt = item_utt;
  p.item_start = item_start;
  p.perm = perm;
  p.e0 = e0;
  p.g0 = g0;
  p.seed = seed;
  p.U = U;
  p.P = P;
  p.nE = nE;
  p.size = size;
  p.random = random ? 1 : 0;
  p.history = history;
  return WN_OK;
}

extern "C" {

long wn_corpus_window_frames(int T, int hop, int ctx) {
  if (T < 1 || hop < 1 || ctx < 0) return WN_ERR_BAD_SHAPE;
  return ((long)T + hop - 2) / hop + 1 + 2L * ctx;
}

// hist / lens: both or neither (the plain entry passes neither)
static int corpus_gather(const float* flat, long N, const int64_t* utt_off,
                         const int32_t* utt_len, int U, const int32_t* item_utt,
                         const int32_t* item_start, int P, const int32_t* perm, long e0, int nE,
                         long g0, int size, int random, uint64_t seed, int history, float* audio,
                         int32_t* hist, int32_t* lens, int B, int T, void* stream) {
  if (!flat || !audio) return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || P <= 0 || N <= 0) return WN_ERR_BAD_SHAPE;
  CorpusPlan p;
  const int rc = corpus_plan(p, utt_off, utt_len, U, item_utt, item_start, P, perm, e0, nE, g0,
                             size, random, seed, history, B);
  if (rc != WN_OK) return rc;
  if (!wn_aligned16(flat) || !wn_aligned16(audio) || (reinterpret_cast<uintptr_t>(hist) & 3u) ||
      (reinterpret_cast<uintptr_t>(lens) & 3u))
    return WN_ERR_MISALIGNED;
  const long chunks = ((long)B * T + 3) / 4;
  hipLaunchKernelGGL(corpus_gather_kernel, dim3(grid1d(chunks, CORPUS_BLOCK)),
                     dim3(CORPUS_BLOCK), 0, (hipStream_t)stream, flat, N, p, audio, B, T);
  if (hist)
    hipLaunchKernelGGL(corpus_hist_kernel, dim3(grid1d(B, CORPUS_BLOCK)), dim3(CORPUS_BLOCK), 0,
                       (hipStream_t)stream, N, p, hist, lens, B, T);
  return wn_check_launch();
}

int wn_corpus_gather(const float* flat, long N, const int64_t* utt_off, const int32_t* utt_len,
                     int U, const int32_t* item_utt, const int32_t* item_start, int P,
                     const int32_t* perm, long e0, int nE, long g0, int size, int random,
                     uint64_t seed, float* audio, int B, int T, void* stream) {
  return corpus_gather(flat, N, utt_off, utt_len, U, item_utt, item_start, P, perm, e0, nE, g0,
                       size, random, seed, 0, audio, nullptr, nullptr, B, T, stream);
}

int wn_corpus_gather_hist(const float* flat, long N, const int64_t* utt_off,
                          const int32_t* utt_len, int U, const int32_t* item_utt,
                          const int32_t* item_start, int P, const int32_t* perm, long e0, int nE,
                          long g0, int size, int random, uint64_t seed, int history, float* audio,
                          int32_t* hist, int32_t* lens, int B, int T, void* stream) {
  if (!hist || !lens) return WN_ERR_NULL;
  return corpus_gather(flat, N, utt_off, utt_len, U, item_utt, item_start, P, perm, e0, nE, g0,
                       size, random, seed, history, audio, hist, lens, B, T, stream);
}

int wn_corpus_gather_frames_hist(const float* fr, long NF, const int64_t* fr_off,
                                 const int32_t* fr_len, const int64_t* utt_off,
                                 const int32_t* utt_len, int U, const int32_t* item_utt,
                                 const int32_t* item_start, int P, const int32_t* perm, long e0,
                                 int nE, long g0, int size, int random, uint64_t seed,
                                 int history, int hop, int ctx, int Lc, float* frames, int Fw,
                                 float* rows, int B, int T, void* stream) {
  if (!fr || !fr_off || !fr_len || (!frames && !rows)) return WN_ERR_NULL;
  if (B <= 0 || T <= 0 || P <= 0 || NF <= 0 || hop < 1 || ctx < 0 || Lc < 1 ||
      (frames && Fw < 1))
    return WN_ERR_BAD_SHAPE;
  CorpusPlan p;
  const int rc = corpus_plan(p, utt_off, utt_len, U, item_utt, item_start, P, perm, e0, nE, g0,
                             size, random, seed, history, B);
  if (rc != WN_OK) return rc;
  if (!wn_aligned16(fr) || (frames && !wn_aligned16(frames)) || (rows && !wn_aligned16(rows)) ||
      (reinterpret_cast<uintptr_t>(fr_off) & 7u) || (reinterpret_cast<uintptr_t>(fr_len) & 3u))
    return WN_ERR_MISALIGNED;
  if (frames) {
    const long chunks = ((long)B * Fw * Lc + 3) / 4;
    hipLaunchKernelGGL(corpus_frames_kernel<false>, dim3(grid1d(chunks, CORPUS_BLOCK)),
                       dim3(CORPUS_BLOCK), 0, (hipStream_t)stream, fr, NF, fr_off, fr_len, p, hop,
                       ctx, Lc, frames, B, Fw, T);
  }
  if (rows) {
    const long chunks = ((long)B * T * Lc + 3) / 4;
    hipLaunchKernelGGL(corpus_frames_kernel<true>, dim3(grid1d(chunks, CORPUS_BLOCK)),
                       dim3(CORPUS_BLOCK), 0, (hipStream_t)stream, fr, NF, fr_off, fr_len, p, hop,
                       ctx, Lc, rows, B, T, T);
  }
  return wn_check_launch();
}

int wn_corpus_gather_frames(const float* fr, long NF, const int64_t* fr_off,
                            const int32_t* fr_len, const int64_t* utt_off,
                            const int32_t* utt_len, int U, const int32_t* item_utt,
                            const int32_t* item_start, int P, const int32_t* perm, long e0,
                            int nE, long g0, int size, int random, uint64_t seed, int hop,
                            int ctx, int Lc, float* frames, int Fw, float* rows, int B, int T,
                            void* stream) {
  return wn_corpus_gather_frames_hist(fr, NF, fr_off, fr_len, utt_off, utt_len, U, item_utt,
                                      item_start, P, perm, e0, nE, g0, size, random, seed, 0, hop,
                                      ctx, Lc, frames, Fw, rows, B, T, stream);
}

}  // extern "C"
