// Polyphase sample-rate conversion (include/wavenet_resample.h states the
// rule; wavenet/resample.py's Resampler.reference restates it in numpy float32,
// tests/resample_ref.py in float64).
//
// resample_kernel: a workgroup per RS_TILE outputs of one clip, one output per
// lane.  Output k sits on phase r = (k down + Hh) mod up and walks that phase's
// taps t = LP - 1 .. 0 against the samples jh - t, so all lanes of a wave are at
// the same t and differ in r only.
//
// * The taps are laid out by phase, row r at r * LPS with LPS odd.  A
//   ds_read_b32 is served per 32-lane half over 32 banks: the lanes of a half
//   read the addresses r * LPS + t of at most min(32, up) phases, lanes on one
//   phase read one word (a broadcast), and two phases r1 != r2 share a bank only
//   where (r1 - r2) * LPS = 0 mod 32, that is where r1 - r2 = 0 mod 32 as LPS is
//   odd: no conflict for up <= 32, and for a larger up only between lanes whose
//   phases lie a multiple of 32 apart.  The taps in their natural order would be
//   read at stride `down` across the lanes: gcd(down, 32)-way conflicts, 8-way
//   for 16 kHz -> 10 kHz (5 / 8).
// * TAPS_ALL: up * LPS <= RS_TAB floats, the whole table is staged.  TAPS_ROWS:
//   otherwise, where RS_TILE * LPS <= RS_TAB, the row of every output's phase
//   is staged at lane * LPS (the phases the tile touches; again odd stride).
//   TAPS_MEM: neither fits (a long filter on few phases, 1 / 1000 say): the
//   rows are read from memory.
// * XS: the input span of a tile, at most ((RS_TILE - 1) down + 2 Hh) / up + 2
//   samples, is staged once where that is <= RS_XS floats; lanes then read it at
//   stride down / up: two lanes of a half share a bank with different words only
//   where the span of a half exceeds 32 words (down > up: 2-way at 8 / 5).
//   Otherwise the samples are read from memory.
#include "wn_common.h"

#define RS_TILE 256
#define RS_TAB 12288      // floats of taps in LDS
#define RS_XS 3072        // floats of input in LDS (61 KiB with the taps and the phases)
#define RS_MAX_RATIO 1024
#define RS_MAX_TAPS 65537

enum { TAPS_ALL = 0, TAPS_ROWS = 1, TAPS_MEM = 2 };

struct RsArgs {
  const float* x;
  const float* tab;
  const int32_t* lengths;
  float* out;
  long ld_x, ld_out;
  int T, T_out, up, down, Hh, LP, LPS;
};

__device__ __forceinline__ int rs_len(const int32_t* lengths, int b, int T) {
  int n = T;
  if (lengths) {
    n = lengths[b];
    n = n < 0 ? 0 : (n > T ? T : n);
  }
  return n;
}

template <int TM, bool XS>
__global__ __launch_bounds__(RS_TILE) void resample_kernel(RsArgs a) {
#pragma clang fp contract(off)
  __shared__ float tabs[TM == TAPS_MEM ? 1 : RS_TAB];
  __shared__ float xs[XS ? RS_XS : 1];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long k0 = (long)blockIdx.x * RS_TILE;
  const int n = rs_len(a.lengths, b, a.T);
  const long n_out = ((long)n * a.up + a.down - 1) / a.down;
  const float* x = a.x + (long)b * a.ld_x;
  float* y = a.out + (long)b * a.ld_out;
  const long k = k0 + tid;
  long mm = n_out - k0;                         // real outputs of the tile
  const int m = mm < 0 ? 0 : (mm > RS_TILE ? RS_TILE : (int)mm);
  if (m == 0) {                                 // (workgroup-uniform)
    if (k < a.T_out) y[k] = 0.f;
    return;
  }
  const int up = a.up, Hh = a.Hh, LPS = a.LPS;
  // this lane's output: phase, newest sample, taps
  const long c = k * a.down + Hh;
  const int jh = (int)(c / up);
  const int r = (int)(c - (long)jh * up);
  int t_hi = (2 * Hh - r) / up;                 // r + t up <= 2 Hh
  t_hi = t_hi < jh ? t_hi : jh;                 // jh - t >= 0
  int t_lo = jh - n + 1;                        // jh - t < n
  t_lo = t_lo < 0 ? 0 : t_lo;
  // the samples the tile reads: j_lo .. j_hi, all below n
  int j_lo = 0;
  if (XS) {
    const long lo = k0 * a.down - Hh;           // j >= ceil(lo / up)
    j_lo = lo <= 0 ? 0 : (int)((lo + up - 1) / up);
    const long hi = ((k0 + m - 1) * a.down + Hh) / up;
    const int j_hi = hi < n - 1 ? (int)hi : n - 1;
    int span = j_hi - j_lo + 1;
    span = span > RS_XS ? RS_XS : span;         // (the host chose XS so that it fits)
    for (int i = tid; i < span; i += RS_TILE) xs[i] = x[j_lo + i];
  }
  if (TM == TAPS_ALL) {
    const int words = up * LPS;                 // <= RS_TAB (the host's choice)
    for (int i = tid; i < words; i += RS_TILE) tabs[i] = a.tab[i];
  } else if (TM == TAPS_ROWS) {
    __shared__ int rs[RS_TILE];
    rs[tid] = r;
    __syncthreads();
    const int words = m * LPS;                  // <= RS_TILE * LPS <= RS_TAB
    for (int i = tid; i < words; i += RS_TILE) {
      const int lo = i / LPS, t = i - lo * LPS;
      tabs[i] = a.tab[(long)rs[lo] * LPS + t];
    }
  }
  __syncthreads();
  float acc = 0.f;
  if (tid < m) {
    const float* hg = a.tab + (long)r * LPS;
    const float* hl = tabs + (TM == TAPS_ALL ? r : tid) * LPS;
    for (int t = a.LP - 1; t >= 0; --t) {       // (the same t in every lane)
      if (t <= t_hi && t >= t_lo) {
        const float h = TM == TAPS_MEM ? hg[t] : hl[t];
        const float v = XS ? xs[jh - t - j_lo] : x[jh - t];
        acc = acc + h * v;
      }
    }
  }
  if (k < a.T_out) y[k] = acc;                  // (+0 behind n_out)
}

__global__ __launch_bounds__(256) void resample_copy_kernel(RsArgs a) {
  const int b = blockIdx.y;
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  const int n = rs_len(a.lengths, b, a.T);
  if (k < a.T_out) a.out[(long)b * a.ld_out + k] = k < n ? a.x[(long)b * a.ld_x + k] : 0.f;
}

static inline bool rs_mis(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 3u) != 0;
}

static int rs_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

extern "C" {

int wn_resample_tile(void) { return RS_TILE; }

int wn_resample(const float* x, long ld_x, const int32_t* lengths, int B, int T,
                int up, int down, int Hh, const float* tab, float* out,
                long ld_out, void* stream) {
  if (!x || !tab || !out) return WN_ERR_NULL;
  if (up < 1 || up > RS_MAX_RATIO || down < 1 || down > RS_MAX_RATIO || Hh < 0 ||
      2L * Hh + 1 > RS_MAX_TAPS || B < 1 || B > 65535 || T < 1 || T > (1 << 30) ||
      rs_gcd(up, down) != 1)
    return WN_ERR_BAD_SHAPE;
  const long T_out = ((long)T * up + down - 1) / down;
  if (T_out > (1L << 30) || ld_x < T || ld_out < T_out) return WN_ERR_BAD_SHAPE;
  if (rs_mis(x) || rs_mis(lengths) || rs_mis(tab) || rs_mis(out)) return WN_ERR_MISALIGNED;
  {
    const uintptr_t lo_x = reinterpret_cast<uintptr_t>(x), lo_y = reinterpret_cast<uintptr_t>(out);
    const uintptr_t hi_x = lo_x + 4u * (uintptr_t)((long)(B - 1) * ld_x + T);
    const uintptr_t hi_y = lo_y + 4u * (uintptr_t)((long)(B - 1) * ld_out + T_out);
    if (lo_x < hi_y && lo_y < hi_x) return WN_ERR_BAD_SHAPE;
  }
  RsArgs a;
  a.x = x; a.tab = tab; a.lengths = lengths; a.out = out;
  a.ld_x = ld_x; a.ld_out = ld_out;
  a.T = T; a.T_out = (int)T_out; a.up = up; a.down = down; a.Hh = Hh;
  a.LP = (2 * Hh + up) / up;
  a.LPS = a.LP | 1;
  const dim3 grid((unsigned)((T_out + RS_TILE - 1) / RS_TILE), (unsigned)B);
  if (up == down) {                             // 1 / 1
    hipLaunchKernelGGL(resample_copy_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    return wn_check_launch();
  }
  const bool xs = ((long)(RS_TILE - 1) * down + 2L * Hh) / up + 2 <= RS_XS;
  // (TAPS_ROWS means up > RS_TAB / LPS with LPS <= RS_TAB / RS_TILE: at up <=
  // 1024 a ratio down / up below 4, whose span always fits; should the limits
  // ever change, such a shape reads both from memory)
  const int tm = (long)up * a.LPS <= RS_TAB ? TAPS_ALL
               : ((long)RS_TILE * a.LPS <= RS_TAB && xs) ? TAPS_ROWS : TAPS_MEM;
  void (*kern)(RsArgs);
  if (tm == TAPS_ALL)
    kern = xs ? resample_kernel<TAPS_ALL, true> : resample_kernel<TAPS_ALL, false>;
  else if (tm == TAPS_ROWS)
    kern = resample_kernel<TAPS_ROWS, true>;
  else
    kern = xs ? resample_kernel<TAPS_MEM, true> : resample_kernel<TAPS_MEM, false>;
  hipLaunchKernelGGL(kern, grid, dim3(RS_TILE), 0, (hipStream_t)stream, a);
  return wn_check_launch();
}

}  // extern "C"
