// Conditioning frames assembled on the device (include/wavenet_lc_frames.h
// states the rule; wavenet/frontend.py drives it): the mel channels copied or
// normalised into out[b][f][0 .. M), the F0 channel and the voicing flag
// written beside them at out[b][f][c0], out[b][f][c0 + 1], in one launch.
//
// Pitch part: one workgroup of LCF_THREADS lanes per clip (blockIdx.y == 0), a
// lane per frame of a chunk of LCF_CHUNK frames.  The interpolated F0 channel
// needs, for an unvoiced frame, the nearest voiced frame on either side:
//   pass down (mode 1 only): chunks from the last real one to the first, a
//     suffix-min scan of (voiced ? f : none) with the carry of the chunks
//     behind; the index goes, as an int32, into the frame's own voicing slot
//     out[b][f][c0 + 1], which this launch owns and overwrites in the pass up;
//   pass up: chunks from 0, a prefix-max scan of (voiced ? f : -1) with the
//     carry of the chunks in front; the lane that stored a frame's index reads
//     it back (same lane, same address: program order), then writes both
//     channels.
// No atomics, no workspace.  The mel part is a strided copy: 16-byte accesses
// where M, both leading dimensions and the four pointers allow, else scalars.
// A clip's rows are split over gridDim.y workgroups (LCF_ROWS rows each at
// least, LCF_MAX_Y workgroups at most), so a long clip -- or a whole corpus
// passed as one clip without an f0 -- does not run on one compute unit; every
// element is still read and written by exactly one lane.
#include "wn_common.h"

#define LCF_THREADS 1024
#define LCF_CHUNK 1024          // one frame per lane and scan step
#define LCF_WAVES (LCF_THREADS / 64)
#define LCF_MAX_M 512
#define LCF_ROWS 256            // rows of the mel part a workgroup takes at least
#define LCF_MAX_Y 1024          // workgroups per clip at most
#define LCF_NONE 0x7fffffff     // "no voiced frame behind" in the pass down

struct LcfArgs {
  const float* mel;
  long ld_mel;
  int M;
  const float* shift;
  const float* scale;
  float lo, hi;
  const float* f0;
  int mode;
  double fmin, span;
  const int32_t* nframes;
  int F;
  float* out;
  long ld_out;
  int c0;
};

// inclusive max over the lanes t' <= t of the block; *total: over all lanes
__device__ __forceinline__ int lcf_scan_max_up(int x, int t, int* red, int* total) {
  const int lane = t & 63, w = t >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x = max(x, y);
  }
  if (lane == 63) red[w] = x;
  __syncthreads();
  int pre = -1, tot = -1;
#pragma unroll
  for (int i = 0; i < LCF_WAVES; ++i) {
    const int v = red[i];
    if (i < w) pre = max(pre, v);
    tot = max(tot, v);
  }
  __syncthreads();
  *total = tot;
  return max(x, pre);
}

// inclusive min over the lanes t' >= t of the block; *total: over all lanes
__device__ __forceinline__ int lcf_scan_min_down(int x, int t, int* red, int* total) {
  const int lane = t & 63, w = t >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_down(x, o);
    if (lane + o < 64) x = min(x, y);
  }
  if (lane == 0) red[w] = x;
  __syncthreads();
  int post = LCF_NONE, tot = LCF_NONE;
#pragma unroll
  for (int i = 0; i < LCF_WAVES; ++i) {
    const int v = red[i];
    if (i > w) post = min(post, v);
    tot = min(tot, v);
  }
  __syncthreads();
  *total = tot;
  return min(x, post);
}

// min(max(log2(double(f0) / fmin) / span, 0), 1) of a voiced frame
__device__ __forceinline__ double lcf_rel(float f0, double f_lo, double span) {
  const double r = log2((double)f0 / f_lo) / span;
  return r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);
}

__device__ __forceinline__ float lcf_norm(float x, float sh, float sc, float lo, float hi) {
#pragma clang fp contract(off)
  const float d = x - sh;
  const float w = d * sc;
  return w < lo ? lo : (w > hi ? hi : w);
}

// rows [f_lo, f_hi) of one clip: out[f][0 .. M) = norm(mel[f][0 .. M)) on real
// frames, zeros behind them.  V floats per access; four rows in flight per
// lane.  In place (out == mel, equal ld) every element is read and written by
// one lane, the loads of a group of four rows before its stores.
template <int V, bool NORM>
__device__ __forceinline__ void lcf_mel_rows(const LcfArgs& a, const float* melb, float* outb,
                                             int n, int t, long f_lo, long f_hi) {
  typedef float vec __attribute__((ext_vector_type(V)));
  const int MV = a.M / V;
  const int W = MV < LCF_THREADS ? MV : LCF_THREADS;   // lanes across a row
  const int RPI = LCF_THREADS / W;                     // rows per sweep
  const int ro = t / W;
  if (ro >= RPI) return;
  for (int cv = t - ro * W; cv < MV; cv += W) {
    const int c = cv * V;
    vec sh, sc;
    if (NORM) {
      sh = *reinterpret_cast<const vec*>(a.shift + c);
      sc = *reinterpret_cast<const vec*>(a.scale + c);
    }
    for (long f = f_lo + ro; f < f_hi; f += 4L * RPI) {
      vec x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long fk = f + (long)k * RPI;
        if (fk < n) x[k] = *reinterpret_cast<const vec*>(melb + fk * a.ld_mel + c);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long fk = f + (long)k * RPI;
        if (fk >= f_hi) break;
        vec v;
        if (fk < n) {
          v = x[k];
          if (NORM) {
#pragma unroll
            for (int e = 0; e < V; ++e)
              v[e] = lcf_norm(x[k][e], sh[e], sc[e], a.lo, a.hi);
          }
        } else {
          v = 0.f;
        }
        *reinterpret_cast<vec*>(outb + fk * a.ld_out + c) = v;
      }
    }
  }
}

template <int V>
__global__ __launch_bounds__(LCF_THREADS) void lc_frames_kernel(LcfArgs a) {
#pragma clang fp contract(off)
  __shared__ int red[LCF_WAVES];
  const int t = threadIdx.x;
  const long b = blockIdx.x;
  const int F = a.F;
  int n = F;
  if (a.nframes) {
    n = a.nframes[b];
    n = n < 0 ? 0 : (n > F ? F : n);
  }
  float* outb = a.out + b * F * a.ld_out;

  if (a.mel) {
    const float* melb = a.mel + b * F * a.ld_mel;
    const long rows = ((long)F + gridDim.y - 1) / gridDim.y;
    const long f_lo = (long)blockIdx.y * rows;
    const long f_hi = f_lo + rows < F ? f_lo + rows : F;
    if (a.shift) lcf_mel_rows<V, true>(a, melb, outb, n, t, f_lo, f_hi);
    else lcf_mel_rows<V, false>(a, melb, outb, n, t, f_lo, f_hi);
  }
  if (!a.f0 || blockIdx.y != 0) return;

  const float* f0b = a.f0 + b * F;
  float* p0 = outb + a.c0;          // the F0 channel of frame 0
  float* p1 = p0 + 1;               // the voicing flag of frame 0

  if (a.mode == 1 && n > 0) {
    int carry = LCF_NONE;
    for (int base = ((n - 1) / LCF_CHUNK) * LCF_CHUNK; base >= 0; base -= LCF_CHUNK) {
      const int g = base + t;
      const bool real = g < n;
      const bool v = real && f0b[real ? g : 0] > 0.f;
      int tot;
      int nx = lcf_scan_min_down(v ? g : LCF_NONE, t, red, &tot);
      nx = min(nx, carry);
      if (real) *reinterpret_cast<int*>(p1 + (long)g * a.ld_out) = nx == LCF_NONE ? -1 : nx;
      carry = min(carry, tot);
    }
  }

  int carry = -1;
  for (long base = 0; base < F; base += LCF_CHUNK) {
    const long gl = base + t;
    const bool in = gl < F;
    const int g = in ? (int)gl : 0;
    const bool real = in && g < n;
    const float x = real ? f0b[g] : 0.f;
    const bool v = real && x > 0.f;
    int tot;
    int pv = lcf_scan_max_up(v ? g : -1, t, red, &tot);
    pv = max(pv, carry);
    carry = max(carry, tot);
    if (!in) continue;
    float ch0 = 0.f, ch1 = 0.f;
    if (v) {
      ch0 = (float)lcf_rel(x, a.fmin, a.span);
      ch1 = 1.f;
    } else if (real && a.mode == 1) {
      int nx = *reinterpret_cast<const int*>(p1 + (long)g * a.ld_out);
      if (nx <= g || nx >= n) nx = -1;           // (only ever what the pass down stored)
      if (pv >= 0 && nx >= 0) {
        const double ra = lcf_rel(f0b[pv], a.fmin, a.span);
        const double rb = lcf_rel(f0b[nx], a.fmin, a.span);
        const double w = (double)(g - pv) / (double)(nx - pv);
        const double d = rb - ra;
        const double s = d * w;
        ch0 = (float)(ra + s);
      } else if (nx >= 0) {
        ch0 = (float)lcf_rel(f0b[nx], a.fmin, a.span);
      } else if (pv >= 0) {
        ch0 = (float)lcf_rel(f0b[pv], a.fmin, a.span);
      }
    }
    p0[(long)g * a.ld_out] = ch0;
    p1[(long)g * a.ld_out] = ch1;
  }
}

extern "C" {

int wn_lc_frames_chunk(void) { return LCF_CHUNK; }

int wn_lc_frames(const float* mel, long ld_mel, int M, const float* shift, const float* scale,
                 float lo, float hi, const float* f0, int mode, double fmin, double span,
                 const int32_t* nframes, int B, int F, float* out, long ld_out, int c0,
                 void* stream) {
  if (!out || (!mel && !f0) || ((shift == nullptr) != (scale == nullptr))) return WN_ERR_NULL;
  if (B < 1 || B > 65535 || F < 1 || F > (1 << 30) || M < 0 || M > LCF_MAX_M ||
      ld_out < 1 || ld_out > (1L << 20) || ld_out < M)
    return WN_ERR_BAD_SHAPE;
  if (mel && (M < 1 || ld_mel < M || ld_mel > (1L << 20))) return WN_ERR_BAD_SHAPE;
  if (mel && shift && !(lo <= hi)) return WN_ERR_BAD_SHAPE;     // (lo > hi, or a NaN bound)
  if (f0 && (c0 < M || (long)c0 + 2 > ld_out || (mode != 0 && mode != 1) || !(fmin > 0.0) ||
             !(span > 0.0) || !(fmin < 1e300) || !(span < 1e300)))
    return WN_ERR_BAD_SHAPE;
  const void* ptrs[] = {mel, shift, scale, f0, nframes, out};
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) & 3u) return WN_ERR_MISALIGNED;
  LcfArgs a;
  a.mel = mel;
  a.ld_mel = ld_mel;
  a.M = M;
  a.shift = mel ? shift : nullptr;
  a.scale = mel ? scale : nullptr;
  a.lo = lo;
  a.hi = hi;
  a.f0 = f0;
  a.mode = mode;
  a.fmin = fmin;
  a.span = span;
  a.nframes = nframes;
  a.F = F;
  a.out = out;
  a.ld_out = ld_out;
  a.c0 = c0;
  const bool wide = mel && M % 4 == 0 && ld_mel % 4 == 0 && ld_out % 4 == 0 &&
                    wn_aligned16(mel) && wn_aligned16(out) && wn_aligned16(a.shift) &&
                    wn_aligned16(a.scale);
  long ny = mel ? ((long)F + LCF_ROWS - 1) / LCF_ROWS : 1;
  if (ny > LCF_MAX_Y) ny = LCF_MAX_Y;
  const dim3 grid((unsigned)B, (unsigned)ny);
  hipStream_t s = (hipStream_t)stream;
  if (wide)
    hipLaunchKernelGGL(lc_frames_kernel<4>, grid, dim3(LCF_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(lc_frames_kernel<1>, grid, dim3(LCF_THREADS), 0, s, a);
  return wn_check_launch();
}

}  // extern "C"
