// Local conditioning in fast generation: the conditioned-bias ring.
//
// With local conditioning (WaveNet paper 2.5) a layer's filter and gate
// pre-activations gain lc[t] . Wlc, where lc[t] is the feature row beside
// input sample t.  It enters where the filter|gate bias (and the GC term)
// already enter, so the generators read, in place of bias_fg[l][b], row p of
//
//   ring[p % R][l][b][0:64] = bias_fg[l][b] + sum_k lc[b][p][k] * lc_w[k][l][0:64]
//
// which this launch writes for a range of positions p, one chunk of steps
// ahead of the generator (wavenet/fastgen.py).  The sum is ONE fmaf chain per
// element in k order, so a row's bits depend on Lc only: not on B, the
// stream's position, the chunk or the row's place in it.  With all-zero LC a
// row is bias_fg exactly (fmaf(0, w, b) = b), so the generators compute bitwise
// what they compute without LC.
#include "wn_common.h"

#define FGL_PAIRS 16     // (row, stream) pairs per wave
#define FGL_KT 64        // LC channels per LDS tile of lc_w
#define FGL_MAXB 256

struct FgLcBias {
  const float* lc;       // row i of stream b at lc + b * lc_stride + i * Lc
  long lc_stride;
  int Lc;
  const float* lc_w;     // [Lcp][L][64]
  const float* bias;     // [L][nb][64] or null (nb = B with stride 64, 1 with 0)
  int bias_stride;
  int L, B;
  long p0;
  int n_rows;
  float* ring;           // [R][L][nr][64] (nr = B with stride 64, 1 with 0)
  int R, ring_stride;
};

// grid (ceil(n_rows * nr / 64), L), 256 threads: wave w takes 16 (row, stream)
// pairs of layer blockIdx.y, lane = output channel (filter | gate).  Per tile
// of 64 LC channels: lc_w's [64][64] slice and the wave's 16 LC row slices sit
// in LDS, and each k step is one weight read shared by the 16 pairs' chains
// (16 independent fmaf chains per lane; each one still runs k in order).
__global__ __launch_bounds__(256) void fgl_bias_kernel(FgLcBias a) {
  __shared__ float wt[FGL_KT * 64];
  __shared__ __attribute__((aligned(16))) float xs[4][FGL_PAIRS][FGL_KT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = blockIdx.y, L = a.L;
  const int nr = a.ring_stride ? a.B : 1;
  const long npairs = (long)a.n_rows * nr;
  const long pair0 = (long)blockIdx.x * (4 * FGL_PAIRS) + wave * FGL_PAIRS;
  const long blstride = a.bias_stride ? (long)a.B * 64 : 64;
  float acc[FGL_PAIRS];
#pragma unroll
  for (int i = 0; i < FGL_PAIRS; ++i) {
    const long pr = pair0 + i;
    acc[i] = 0.f;
    if (pr < npairs && a.bias) {
      const int b = (int)(pr % nr);
      acc[i] = a.bias[l * blstride + (long)b * a.bias_stride + lane];
    }
  }
  float (*x)[FGL_KT] = xs[wave];
  for (int k0 = 0; k0 < a.Lc; k0 += FGL_KT) {
    const int kn = min(FGL_KT, a.Lc - k0);
    __syncthreads();
    for (int i = tid; i < kn * 64; i += 256)
      wt[i] = a.lc_w[((long)(k0 + (i >> 6)) * L + l) * 64 + (i & 63)];
    for (int j = lane; j < FGL_PAIRS * FGL_KT; j += 64) {
      const int i = j / FGL_KT, k = j % FGL_KT;
      const long pr = pair0 + i;
      float v = 0.f;
      if (pr < npairs && k < kn) {
        const long row = pr / nr, b = pr % nr;
        v = a.lc[b * a.lc_stride + row * a.Lc + k0 + k];
      }
      x[i][k] = v;
    }
    __syncthreads();
    int k = 0;
    for (; k + 4 <= kn; k += 4) {
      const float w0 = wt[k * 64 + lane], w1 = wt[(k + 1) * 64 + lane];
      const float w2 = wt[(k + 2) * 64 + lane], w3 = wt[(k + 3) * 64 + lane];
#pragma unroll
      for (int i = 0; i < FGL_PAIRS; ++i) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(&x[i][k]);
        float c = acc[i];
        c = fmaf(v[0], w0, c);
        c = fmaf(v[1], w1, c);
        c = fmaf(v[2], w2, c);
        c = fmaf(v[3], w3, c);
        acc[i] = c;
      }
    }
    for (; k < kn; ++k) {
      const float w = wt[k * 64 + lane];
#pragma unroll
      for (int i = 0; i < FGL_PAIRS; ++i) acc[i] = fmaf(x[i][k], w, acc[i]);
    }
  }
  const long rl = (long)nr * 64;
#pragma unroll
  for (int i = 0; i < FGL_PAIRS; ++i) {
    const long pr = pair0 + i;
    if (pr < npairs) {
      const long row = pr / nr, b = pr % nr;
      a.ring[((a.p0 + row) % a.R * L + l) * rl + b * 64 + lane] = acc[i];
    }
  }
}

extern "C" {

int wn_fastgen_lc_bias(const float* lc, long lc_stream_stride, int Lc, const float* lc_w, int L,
                       const float* gc_bias_fg, int bias_stream_stride, int B, long p0,
                       int n_rows, float* ring, int R, int ring_stream_stride, void* stream) {
  if (!lc || !lc_w || !ring) return WN_ERR_NULL;
  if (Lc <= 0 || L <= 0 || B <= 0 || n_rows <= 0 || R <= 0 || n_rows > R || p0 < 0 ||
      lc_stream_stride < 0 || (bias_stream_stride != 0 && bias_stream_stride != 64) ||
      (ring_stream_stride != 0 && ring_stream_stride != 64))
    return WN_ERR_BAD_SHAPE;
  // one ring row for all streams only when nothing differs between them
  if (ring_stream_stride == 0 && (lc_stream_stride != 0 || bias_stream_stride != 0))
    return WN_ERR_BAD_SHAPE;
  if (B > FGL_MAXB) return WN_ERR_UNSUPPORTED;
  FgLcBias a;
  a.lc = lc; a.lc_stride = lc_stream_stride; a.Lc = Lc; a.lc_w = lc_w;
  a.bias = gc_bias_fg; a.bias_stride = bias_stream_stride; a.L = L; a.B = B;
  a.p0 = p0; a.n_rows = n_rows; a.ring = ring; a.R = R; a.ring_stride = ring_stream_stride;
  const long npairs = (long)n_rows * (ring_stream_stride ? B : 1);
  const long gx = (npairs + 4 * FGL_PAIRS - 1) / (4 * FGL_PAIRS);
  if (gx > 0x7fffffffL) return WN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(fgl_bias_kernel, dim3((unsigned)gx, L), dim3(256), 0, (hipStream_t)stream,
                     a);
  return wn_check_launch();
}

}  // extern "C"
