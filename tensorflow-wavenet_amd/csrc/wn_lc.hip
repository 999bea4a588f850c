// Local conditioning at frame rate: the learned upsampler (forward, backward)
// and the frame-context convolution in front of it.
#include "wn_common.h"
#include <cmath>

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------
// Learned upsampling of frame-rate local-conditioning features (WaveNet paper
// 2.5).  Layer i (scale s_i) is a transposed convolution over time with
// kernel = stride = s_i and, over the feature axis, a 3-tap kernel with zero
// padding and one scalar bias:
//   out[c] = b_i + W_i[j][0] u[c-1] + W_i[j][1] u[c] + W_i[j][2] u[c+1]
// for output slot j of an input row u.  Timeline position p = off[b] + t takes
// frame p / hop and the slot digits of p % hop, most significant first.  A
// row is computed from its frame, its slot and the weights alone, in one
// fixed order (explicit FMAs): its bits do not depend on the batch, the clip
// length, the offset or the call.
//
// Segment layout (`up`): filters W_i[s_i][3] of all layers back to back, then
// (use_bias) the m biases.  Per launch: frames [B][F][Lc], off[b] int32.
// ---------------------------------------------------------------------------
#define LCUP_MAX_LAYERS 8
#define LCUP_MAX_LC 512
#define LCUP_CPL (LCUP_MAX_LC / 64)          // channels per lane

struct LcUpGeom {
  int m, hop, Lc, use_bias;
  int s[LCUP_MAX_LAYERS];    // scales
  int suf[LCUP_MAX_LAYERS];  // s_{i+1} * ... * s_m (slot digit divisor)
  int fo[LCUP_MAX_LAYERS];   // filter offset of layer i in the segment
  int bo;                    // offset of the biases
};

__device__ __forceinline__ int lcup_slot(const LcUpGeom& g, int i, int j) {
  return (j / g.suf[i]) % g.s[i];
}

// one layer of one row: buf_in / buf_out hold Lc + 2 floats with a zero at
// either end (index c + 1 is channel c)
__device__ __forceinline__ void lcup_layer(const LcUpGeom& g,
                                           const float* __restrict__ up, int i,
                                           int j, const float* bin, float* bout,
                                           int lane) {
  const int slot = lcup_slot(g, i, j);
  const float* w = up + g.fo[i] + 3 * slot;
  const float w0 = w[0], w1 = w[1], w2 = w[2];
  const float b = g.use_bias ? up[g.bo + i] : 0.f;
#pragma unroll
  for (int k = 0; k < LCUP_CPL; ++k) {
    const int c = lane + 64 * k;
    if (c < g.Lc) {
      float a = b;
      a = fmaf(w0, bin[c], a);
      a = fmaf(w1, bin[c + 1], a);
      a = fmaf(w2, bin[c + 2], a);
      bout[c + 1] = a;
    }
  }
}

// the frame row of row r into buf (zero ends); returns the slot index p % hop
__device__ __forceinline__ int lcup_load(const LcUpGeom& g,
                                         const float* __restrict__ frames,
                                         int F, const int32_t* __restrict__ off,
                                         int T, long r, float* buf, int lane) {
  const int b = (int)(r / T), t = (int)(r - (long)b * T);
  const long p = (long)off[b] + t;
  long f = p / g.hop;
  if (f > F - 1) f = F - 1;          // (the host checks coverage; never read past)
  const float* src = frames + ((long)b * F + f) * g.Lc;
#pragma unroll
  for (int k = 0; k < LCUP_CPL; ++k) {
    const int c = lane + 64 * k;
    if (c < g.Lc) buf[c + 1] = src[c];
  }
  if (lane == 0) {
    buf[0] = 0.f;
    buf[g.Lc + 1] = 0.f;
  }
  return (int)(p % g.hop);
}

// forward: one wave per row, four rows per workgroup, ping-pong rows in LDS
__global__ __launch_bounds__(256) void lc_upsample_fwd_kernel(
    LcUpGeom g, const float* __restrict__ frames, int F,
    const int32_t* __restrict__ off, const float* __restrict__ up,
    float* __restrict__ out, int ldo, int T, long N) {
  __shared__ float lds[4][2][LCUP_MAX_LC + 2];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + wv;
  const bool live = r < N;
  float* b0 = lds[wv][0];
  float* b1 = lds[wv][1];
  if (lane == 0) b1[0] = b1[g.Lc + 1] = 0.f;
  const int j = live ? lcup_load(g, frames, F, off, T, r, b0, lane) : 0;
  __syncthreads();
  for (int i = 0; i < g.m; ++i) {
    if (live) lcup_layer(g, up, i, j, (i & 1) ? b1 : b0, (i & 1) ? b0 : b1, lane);
    __syncthreads();
  }
  if (!live) return;
  const float* res = (g.m & 1) ? b1 : b0;
  float* dst = out + r * ldo;
  for (int c = lane; c < ldo; c += 64) dst[c] = c < g.Lc ? res[c + 1] : 0.f;
}

__device__ __forceinline__ float lcup_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// backward: one wave per workgroup owning rows [w * rpw, (w + 1) * rpw).  Per
// row: the layer chain again (every layer's input kept in LDS), then d row
// back through the layers; the (layer, slot, tap) and bias partials add up in
// LDS in row order and go to the workgroup's slab at the end.
// CTX (the frame-context variant): the gradient at the layer-0 input, summed
// in registers in row order over the run of rows that share a frame (a
// segment).  A segment that starts at the workgroup's first row goes to
// dpart[w][0], one that ends at its last row (and does not start at its
// first) to dpart[w][1], every other one straight to dfr[b][f]: no two
// workgroups write the same float.  lc_context_dfix_kernel adds the parts.
template <bool CTX>
__global__ __launch_bounds__(64) void lc_upsample_bwd_kernel(
    LcUpGeom g, const float* __restrict__ frames, int F,
    const int32_t* __restrict__ off, const float* __restrict__ up,
    const float* __restrict__ drows, int ldd, int T, long N, long rpw,
    float* __restrict__ slabs, long slab_stride, int nacc,
    float* __restrict__ dfr, float* __restrict__ dpart) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  const int W = g.Lc + 2;
  float* U = lds;                              // [m + 1][W]
  float* G0 = U + (g.m + 1) * W;               // [2][W]
  float* acc = G0 + 2 * W;                     // [nacc]
  for (int e = lane; e < nacc; e += 64) acc[e] = 0.f;
  for (int e = lane; e < 2 * W; e += 64) G0[e] = 0.f;
  for (int i = 1; i <= g.m; ++i)
    if (lane == 0) U[i * W] = U[i * W + g.Lc + 1] = 0.f;
  __syncthreads();
  const long r0 = (long)blockIdx.x * rpw;
  const long r1 = r0 + rpw < N ? r0 + rpw : N;
  float dacc[LCUP_CPL];
  long seg_key = -1, seg_r = r0;      // (b * F + frame) and first row
  if constexpr (CTX) {
#pragma unroll
    for (int k = 0; k < LCUP_CPL; ++k) dacc[k] = 0.f;
  }
  for (long r = r0; r < r1; ++r) {
    if constexpr (CTX) {
      const int b = (int)(r / T);
      const long key = (long)b * F + ((long)off[b] + (r - (long)b * T)) / g.hop;
      if (key != seg_key) {
        if (seg_key >= 0) {
          // a segment that ended before r1: dpart[w][0] or interior
          float* dst = seg_r == r0
                           ? dpart + (long)blockIdx.x * 2 * g.Lc
                           : dfr + seg_key * g.Lc;
#pragma unroll
          for (int k = 0; k < LCUP_CPL; ++k) {
            const int c = lane + 64 * k;
            if (c < g.Lc) dst[c] = dacc[k];
            dacc[k] = 0.f;
          }
        }
        seg_key = key;
        seg_r = r;
      }
    }
    const int j = lcup_load(g, frames, F, off, T, r, U, lane);
    __syncthreads();
    for (int i = 0; i < g.m; ++i) {
      lcup_layer(g, up, i, j, U + i * W, U + (i + 1) * W, lane);
      __syncthreads();
    }
    float* gc = G0;
    float* gn = G0 + W;
    const float* dr = drows + r * ldd;
#pragma unroll
    for (int k = 0; k < LCUP_CPL; ++k) {
      const int c = lane + 64 * k;
      if (c < g.Lc) gc[c + 1] = dr[c];
    }
    __syncthreads();
    for (int i = g.m - 1; i >= 0; --i) {
      const float* u = U + i * W;
      float p0 = 0.f, p1 = 0.f, p2 = 0.f, pb = 0.f;
#pragma unroll
      for (int k = 0; k < LCUP_CPL; ++k) {
        const int c = lane + 64 * k;
        if (c < g.Lc) {
          const float d = gc[c + 1];
          p0 = fmaf(d, u[c], p0);
          p1 = fmaf(d, u[c + 1], p1);
          p2 = fmaf(d, u[c + 2], p2);
          pb += d;
        }
      }
      p0 = lcup_wave_sum(p0);
      p1 = lcup_wave_sum(p1);
      p2 = lcup_wave_sum(p2);
      pb = lcup_wave_sum(pb);
      const int slot = lcup_slot(g, i, j);
      const int fw = g.fo[i] + 3 * slot;
      if (lane == 0) {
        acc[fw] += p0;
        acc[fw + 1] += p1;
        acc[fw + 2] += p2;
        if (g.use_bias) acc[g.bo + i] += pb;
      }
      if (i > 0) {
        // d u[c] = W0 d out[c + 1] + W1 d out[c] + W2 d out[c - 1]
        const float* w = up + fw;
        const float w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
        for (int k = 0; k < LCUP_CPL; ++k) {
          const int c = lane + 64 * k;
          if (c < g.Lc) {
            float a = w0 * gc[c + 2];
            a = fmaf(w1, gc[c + 1], a);
            a = fmaf(w2, gc[c], a);
            gn[c + 1] = a;
          }
        }
        float* t = gc;
        gc = gn;
        gn = t;
      } else if constexpr (CTX) {
        // the layer-0 input's gradient, the same three taps
        const float* w = up + fw;
        const float w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
        for (int k = 0; k < LCUP_CPL; ++k) {
          const int c = lane + 64 * k;
          if (c < g.Lc) {
            float a = w0 * gc[c + 2];
            a = fmaf(w1, gc[c + 1], a);
            a = fmaf(w2, gc[c], a);
            dacc[k] += a;
          }
        }
      }
      __syncthreads();
    }
  }
  if constexpr (CTX) {
    // the last segment: dpart[w][0] if it is also the first, else [w][1]
    float* dst = dpart + ((long)blockIdx.x * 2 + (seg_r == r0 ? 0 : 1)) * g.Lc;
#pragma unroll
    for (int k = 0; k < LCUP_CPL; ++k) {
      const int c = lane + 64 * k;
      if (seg_key >= 0 && c < g.Lc) dst[c] = dacc[k];
    }
  }
  __syncthreads();
  float* dst = slabs + (long)blockIdx.x * slab_stride;
  for (int e = lane; e < nacc; e += 64) dst[e] = acc[e];
}

// d frames [B][F][Lc] of the frame-context variant: frame f of clip b
// gathers rows [max(0, f hop - o), min(T, (f + 1) hop - o)) of the clip
// (o = off[b] < hop).  A frame inside one workgroup's rows that is neither its
// first nor its last segment was written by that workgroup; the others add
// the workgroups' parts in workgroup order; a frame without rows is zero.
__global__ __launch_bounds__(256) void lc_context_dfix_kernel(
    const int32_t* __restrict__ off, int hop, int Lc, int F, int T, long N,
    long rpw, const float* __restrict__ dpart, float* __restrict__ dfr,
    long total) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % Lc);
  const long bf = e / Lc;
  const int b = (int)(bf / F), f = (int)(bf - (long)b * F);
  const long o = off[b];
  long t0 = (long)f * hop - o, t1 = t0 + hop;
  if (t0 < 0) t0 = 0;
  if (t1 > T) t1 = T;
  if (t0 >= t1) {
    dfr[e] = 0.f;
    return;
  }
  const long ra = (long)b * T + t0, rb = (long)b * T + t1;
  const long wlo = ra / rpw, whi = (rb - 1) / rpw;
  if (wlo == whi) {
    const long s = wlo * rpw, x = s + rpw < N ? s + rpw : N;
    if (ra == s)
      dfr[e] = dpart[(wlo * 2) * Lc + c];
    else if (rb == x)
      dfr[e] = dpart[(wlo * 2 + 1) * Lc + c];
    return;                           // (else: written by the workgroup)
  }
  float a = 0.f;
  for (long w = wlo; w <= whi; ++w)
    a += dpart[(w * 2 + (ra <= w * rpw ? 0 : 1)) * Lc + c];
  dfr[e] = a;
}

// ---------------------------------------------------------------------------
// Frame-context convolution in front of the upsampler: a convolution over
// frames with kernel 2p + 1, Lc -> Lc channels, no bias,
//   ctx[b][f][j] = sum_{k, c} W[k][c][j] x[b][f + k][c]
// on x [B][Fx][Lc], the frames staged with p frames of context either side
// (window frame f + k is clip frame f + k - p; zeros outside the clip) and W
// [2p + 1][Lc][Lc].  The window of output frame f is the contiguous run
// x[b][f] .. x[b][f + 2p], K = (2p + 1) Lc floats, summed in kc order: an
// output's bits depend on its window and W only.
// ---------------------------------------------------------------------------
#define LCCTX_MAX_P 8

// forward: one wave per output frame, lane = channel j (+ 64 k); the window
// value is the same for the whole wave
__global__ __launch_bounds__(256) void lc_context_fwd_kernel(
    const float* __restrict__ x, int Fx, const float* __restrict__ w, int K,
    int Lc, float* __restrict__ ctx, int Fw, long rows) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int b = (int)(r / Fw), f = (int)(r - (long)b * Fw);
  const float* xr = x + ((long)b * Fx + f) * Lc;
  float a[LCUP_CPL];
#pragma unroll
  for (int k = 0; k < LCUP_CPL; ++k) a[k] = 0.f;
  for (int kc = 0; kc < K; ++kc) {
    const float v = xr[kc];
    const float* wr = w + (long)kc * Lc;
#pragma unroll
    for (int k = 0; k < LCUP_CPL; ++k) {
      const int c = lane + 64 * k;
      if (c < Lc) a[k] = fmaf(wr[c], v, a[k]);
    }
  }
  float* dst = ctx + r * Lc;
#pragma unroll
  for (int k = 0; k < LCUP_CPL; ++k) {
    const int c = lane + 64 * k;
    if (c < Lc) dst[c] = a[k];
  }
}

// weight gradient dW[kc][j] = sum_r x[r's window][kc] dctx[r][j]: one wave per
// (kc, slab); slab s sums rows [s rps, (s + 1) rps) of the B * Fw output
// frames in order into slabs[s][kc][j] (wn_reduce_slabs adds the slabs)
__global__ __launch_bounds__(256) void lc_context_wgrad_kernel(
    const float* __restrict__ x, int Fx, const float* __restrict__ d, int Fw,
    int K, int Lc, long rows, long rps, float* __restrict__ slabs,
    long slab_stride) {
  const int lane = threadIdx.x & 63;
  const long kc = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (kc >= K) return;
  const long r0 = (long)blockIdx.y * rps;
  const long r1 = r0 + rps < rows ? r0 + rps : rows;
  float a[LCUP_CPL];
#pragma unroll
  for (int k = 0; k < LCUP_CPL; ++k) a[k] = 0.f;
  for (long r = r0; r < r1; ++r) {
    const int b = (int)(r / Fw), f = (int)(r - (long)b * Fw);
    const float v = x[((long)b * Fx + f) * Lc + kc];
    const float* dr = d + r * Lc;
#pragma unroll
    for (int k = 0; k < LCUP_CPL; ++k) {
      const int c = lane + 64 * k;
      if (c < Lc) a[k] = fmaf(v, dr[c], a[k]);
    }
  }
  float* dst = slabs + (long)blockIdx.y * slab_stride + kc * Lc;
#pragma unroll
  for (int k = 0; k < LCUP_CPL; ++k) {
    const int c = lane + 64 * k;
    if (c < Lc) dst[c] = a[k];
  }
}

static int lcup_geom(const int* scales, int m, int Lc, int use_bias,
                     LcUpGeom* g, int* nacc) {
  if (!scales) return WN_ERR_NULL;
  if (m < 1 || m > LCUP_MAX_LAYERS || Lc < 1 || Lc > LCUP_MAX_LC)
    return WN_ERR_BAD_SHAPE;
  long hop = 1;
  for (int i = 0; i < m; ++i) {
    if (scales[i] < 2) return WN_ERR_BAD_SHAPE;
    hop *= scales[i];
    if (hop > 4096) return WN_ERR_BAD_SHAPE;
  }
  g->m = m;
  g->hop = (int)hop;
  g->Lc = Lc;
  g->use_bias = use_bias ? 1 : 0;
  int fo = 0, suf = 1;
  for (int i = m - 1; i >= 0; --i) {
    g->suf[i] = suf;
    suf *= scales[i];
  }
  for (int i = 0; i < LCUP_MAX_LAYERS; ++i) {
    g->s[i] = i < m ? scales[i] : 1;
    if (i >= m) g->suf[i] = 1;
    g->fo[i] = fo;
    if (i < m) fo += 3 * scales[i];
  }
  g->bo = fo;
  *nacc = fo + (use_bias ? m : 0);
  return WN_OK;
}

extern "C" {

int wn_lc_upsample_floats(const int* scales, int m, int use_bias) {
  LcUpGeom g;
  int n = 0;
  if (lcup_geom(scales, m, 1, use_bias, &g, &n) != WN_OK) return 0;
  return n;
}

int wn_lc_upsample_fwd(const float* frames, int F, const int32_t* off,
                       const float* up, const int* scales, int m, int Lc,
                       int use_bias, float* rows, int ld_rows, int B, int T,
                       void* stream) {
  if (!frames || !off || !up || !rows) return WN_ERR_NULL;
  LcUpGeom g;
  int nacc = 0;
  const int rc = lcup_geom(scales, m, Lc, use_bias, &g, &nacc);
  if (rc != WN_OK) return rc;
  if (F < 1 || B < 1 || T < 1 || ld_rows < Lc) return WN_ERR_BAD_SHAPE;
  const long N = (long)B * T;
  hipLaunchKernelGGL(lc_upsample_fwd_kernel, dim3((unsigned)((N + 3) / 4)),
                     dim3(256), 0, (hipStream_t)stream, g, frames, F, off, up,
                     rows, ld_rows, T, N);
  return wn_check_launch();
}

int wn_lc_upsample_bwd_slabs(long rows, int nacc) {
  if (rows <= 0 || nacc <= 0) return 0;
  long n = (rows + 31) / 32;                   // >= 32 rows per workgroup
  long cap = (16L << 20) / nacc;               // <= 64 MB of slabs
  if (cap < 64) cap = 64;
  if (n > 4096) n = 4096;
  if (n > cap) n = cap;
  return (int)(n < 1 ? 1 : n);
}

int wn_lc_upsample_bwd(const float* frames, int F, const int32_t* off,
                       const float* up, const int* scales, int m, int Lc,
                       int use_bias, const float* drows, int ld_drows, int B,
                       int T, float* slabs, int num_slabs, long slab_stride,
                       void* stream) {
  if (!frames || !off || !up || !drows || !slabs) return WN_ERR_NULL;
  LcUpGeom g;
  int nacc = 0;
  const int rc = lcup_geom(scales, m, Lc, use_bias, &g, &nacc);
  if (rc != WN_OK) return rc;
  if (F < 1 || B < 1 || T < 1 || ld_drows < Lc || num_slabs < 1 ||
      slab_stride < nacc)
    return WN_ERR_BAD_SHAPE;
  const long N = (long)B * T;
  const long rpw = (N + num_slabs - 1) / num_slabs;
  const size_t lds = sizeof(float) * ((size_t)(m + 3) * (Lc + 2) + nacc);
  if (lds > 64 * 1024) return WN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(lc_upsample_bwd_kernel<false>, dim3((unsigned)num_slabs),
                     dim3(64), lds, (hipStream_t)stream, g, frames, F, off, up,
                     drows, ld_drows, T, N, rpw, slabs, slab_stride, nacc,
                     nullptr, nullptr);
  return wn_check_launch();
}

int wn_lc_upsample_bwd_ctx(const float* frames, int F, const int32_t* off,
                           const float* up, const int* scales, int m, int Lc,
                           int use_bias, const float* drows, int ld_drows,
                           int B, int T, float* slabs, int num_slabs,
                           long slab_stride, float* dframes, float* dpart,
                           void* stream) {
  if (!frames || !off || !up || !drows || !slabs || !dframes || !dpart)
    return WN_ERR_NULL;
  LcUpGeom g;
  int nacc = 0;
  const int rc = lcup_geom(scales, m, Lc, use_bias, &g, &nacc);
  if (rc != WN_OK) return rc;
  if (F < 1 || B < 1 || T < 1 || ld_drows < Lc || num_slabs < 1 ||
      slab_stride < nacc)
    return WN_ERR_BAD_SHAPE;
  // every row's frame inside the F frames (offsets < hop on the device)
  if ((long)(T + g.hop - 2) / g.hop + 1 > F) return WN_ERR_BAD_SHAPE;
  const long N = (long)B * T;
  const long rpw = (N + num_slabs - 1) / num_slabs;
  const size_t lds = sizeof(float) * ((size_t)(m + 3) * (Lc + 2) + nacc);
  if (lds > 64 * 1024) return WN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(lc_upsample_bwd_kernel<true>, dim3((unsigned)num_slabs),
                     dim3(64), lds, (hipStream_t)stream, g, frames, F, off, up,
                     drows, ld_drows, T, N, rpw, slabs, slab_stride, nacc,
                     dframes, dpart);
  const long total = (long)B * F * Lc;
  hipLaunchKernelGGL(lc_context_dfix_kernel, dim3((unsigned)((total + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, off, g.hop, Lc, F, T, N,
                     rpw, dpart, dframes, total);
  return wn_check_launch();
}

int wn_lc_context_fwd(const float* x, int Fx, const float* w, int p, int Lc,
                      float* ctx, int Fw, int B, void* stream) {
  if (!x || !w || !ctx) return WN_ERR_NULL;
  if (p < 0 || p > LCCTX_MAX_P || Lc < 1 || Lc > LCUP_MAX_LC || Fw < 1 ||
      B < 1 || Fx < Fw + 2 * p)
    return WN_ERR_BAD_SHAPE;
  const long rows = (long)B * Fw;
  hipLaunchKernelGGL(lc_context_fwd_kernel, dim3((unsigned)((rows + 3) / 4)),
                     dim3(256), 0, (hipStream_t)stream, x, Fx, w,
                     (2 * p + 1) * Lc, Lc, ctx, Fw, rows);
  return wn_check_launch();
}

int wn_lc_context_wgrad_slabs(long rows, int nacc) {
  if (rows <= 0 || nacc <= 0) return 0;
  long n = (rows + 31) / 32;                   // >= 32 frames per slab
  long cap = (16L << 20) / nacc;               // <= 64 MB of slabs
  if (cap < 1) cap = 1;
  if (n > 256) n = 256;
  if (n > cap) n = cap;
  return (int)(n < 1 ? 1 : n);
}

int wn_lc_context_wgrad(const float* x, int Fx, const float* dctx, int Fw,
                        int p, int Lc, int B, float* slabs, int num_slabs,
                        long slab_stride, void* stream) {
  if (!x || !dctx || !slabs) return WN_ERR_NULL;
  if (p < 0 || p > LCCTX_MAX_P || Lc < 1 || Lc > LCUP_MAX_LC || Fw < 1 ||
      B < 1 || Fx < Fw + 2 * p || num_slabs < 1 || num_slabs > 65535)
    return WN_ERR_BAD_SHAPE;
  const int K = (2 * p + 1) * Lc;
  if (slab_stride < (long)K * Lc) return WN_ERR_BAD_SHAPE;
  const long rows = (long)B * Fw;
  const long rps = (rows + num_slabs - 1) / num_slabs;
  hipLaunchKernelGGL(lc_context_wgrad_kernel,
                     dim3((unsigned)((K + 3) / 4), (unsigned)num_slabs),
                     dim3(256), 0, (hipStream_t)stream, x, Fx, dctx, Fw, K, Lc,
                     rows, rps, slabs, slab_stride);
  return wn_check_launch();
}

}  // extern "C"
