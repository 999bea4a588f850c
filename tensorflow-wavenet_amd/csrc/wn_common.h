// Shared device helpers for the gfx950 (CDNA4 / MI355X) WaveNet kernels.
//
// Conventions used by every MFMA kernel in this directory
// -------------------------------------------------------
// * Activations live in HBM as "planes": [rows][32] fp32, rows = B*T, one
//   128-byte line per audio sample (reference layout [B,T,C] with C padded to
//   32; wavenet/model.py keeps residual/dilation channels innermost too).
// * A "fragment" is a 32(time) x 32(channel) tile held by one 64-lane wave in
//   16 VGPRs per lane.  Lane l = (j = l & 31, h = l >> 5) owns time row j and
//   the 16 channels  c(r,h) = 8*(r>>2) + 4*h + (r&3),  r = 0..15.
//   This is exactly the C/D layout of v_mfma_f32_32x32x2_f32 when the product
//   is computed transposed (channels on the M axis, time on the N axis):
//       OUT^T[ch, time] += W^T[ch, k] * X^T[k, time]
//   so an accumulator IS a fragment: it feeds the next MFMA as the B operand
//   with no lane movement and no LDS round trip, and it is loaded/stored with
//   four 16-byte accesses per lane (channels 8q+4h .. 8q+4h+3, q = 0..3).
// * Weights are the A operand, read from LDS in the reference's own
//   [k][n] (Cin-major, Cout contiguous) order: lane (i, h) reads
//   W[c(r,h)][n0 + i] -> 32 consecutive floats per half-wave, conflict-free.
// * fp32 in / fp32 accumulate MFMA is bit-for-bit an fmaf chain, so parity
//   with the fp32 CPU oracle is limited only by summation order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define WN_OK 0
#define WN_ERR_BAD_SHAPE (-1)
#define WN_ERR_UNSUPPORTED (-2)
#define WN_ERR_MISALIGNED (-3)
#define WN_ERR_LAUNCH (-4)
#define WN_ERR_NULL (-5)
// (variant word of the stack launches: see include/wavenet_hip.h)

#define WN_CH 32  // padded residual/dilation channel count of every plane

// Layer parameter block (floats), contiguous per layer in the flat buffer:
//   Wf[2][32][32] Wg[2][32][32] Wd[32][32] bf[32] bg[32] bd[32]
//   (+ Wgc_filter[G][32] Wgc_gate[G][32] when globally conditioned)
#define LAYER_W_FLOATS (5 * 1024)
#define LAYER_OFF_BF 5120
#define LAYER_OFF_BG 5152
#define LAYER_OFF_BD 5184
#define LAYER_BLOCK_FLOATS (LAYER_W_FLOATS + 96)
#define LAYER_OFF_GC LAYER_BLOCK_FLOATS

static inline int wn_check_launch() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? WN_OK : WN_ERR_LAUNCH;
}

// Compute units of the CURRENT device.  Queried on every call (the HIP
// runtime answers from its own device table; no mutable global here, see the
// threading contract in include/wavenet_hip.h).
static inline int wn_device_cus() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) !=
          hipSuccess || n <= 0)
    n = 256;
  return n;
}

static inline bool wn_aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// workgroups of a grid-stride launch over n elements
static inline int grid1d(long n, int block, int cap = 2048) {
  long g = (n + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

#ifdef __HIPCC__

__device__ __forceinline__ f32x16 frag_zero() {
  f32x16 f;
#pragma unroll
  for (int r = 0; r < 16; ++r) f[r] = 0.f;
  return f;
}

// Load the fragment of plane rows [row0, row0+32) ; `rowp` already points at
// this lane's row (row0 + j), `h` = lane >> 5.  valid=false gives zeros (rows
// before the clip start / past its end: the causal zero padding of
// wavenet/ops.py:50-51).
__device__ __forceinline__ f32x16 frag_load(const float* __restrict__ rowp,
                                            int h, bool valid) {
  f32x16 f;
  const f32x4* p = reinterpret_cast<const f32x4*>(rowp + 4 * h);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (valid) v = p[2 * q];
    f[4 * q + 0] = v[0];
    f[4 * q + 1] = v[1];
    f[4 * q + 2] = v[2];
    f[4 * q + 3] = v[3];
  }
  return f;
}

__device__ __forceinline__ void frag_store(float* __restrict__ rowp, int h,
                                           bool valid, const f32x16& f) {
  if (!valid) return;
  f32x4* p = reinterpret_cast<f32x4*>(rowp + 4 * h);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x4 v = {f[4 * q + 0], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]};
    p[2 * q] = v;
  }
}

// ---------------------------------------------------------------------------
// Coalesced plane I/O through a wave-private LDS tile.
// A fragment access touches 32 rows x 32 B per instruction; HBM/L2 like whole
// 128-byte lines better (measured: 3.6 -> see DESIGN.md).  So global memory is
// always accessed "row-contiguous" (lane l <-> row 8c + (l>>3), 16-byte chunk
// l&7: one instruction = 8 full rows = 1 KiB contiguous) and the 32x32 tile is
// turned into fragment layout through LDS.  Tile layout: [row][32 floats],
// chunk c of row r stored at chunk c ^ (r & 7): conflict-free for the
// row-contiguous side, 2-way for the fragment side.  A wave's DS operations
// execute in order, so no barrier is needed between the two sides.
// ---------------------------------------------------------------------------
struct RowRegs {
  f32x4 v[4];
};

// rows [lo, hi) of the 32-row tile are real, the others read as zero
__device__ __forceinline__ RowRegs rows_load(const float* __restrict__ tile0,
                                             int lane, int lo, int hi) {
  RowRegs R;
  const float* p = tile0 + (long)(lane >> 3) * 32 + (lane & 7) * 4;
  if (lo <= 0 && hi >= 32) {  // wave-uniform: whole tile real -> no predicates
#pragma unroll
    for (int c = 0; c < 4; ++c)
      R.v[c] = *reinterpret_cast<const f32x4*>(p + c * 256);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int r = 8 * c + (lane >> 3);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r >= lo && r < hi) v = *reinterpret_cast<const f32x4*>(p + c * 256);
      R.v[c] = v;
    }
  }
  return R;
}

// address-space-qualified pointers of __builtin_amdgcn_global_load_lds
typedef const __attribute__((address_space(1))) void* wn_gptr_t;
typedef __attribute__((address_space(3))) void* wn_lptr_t;

// LDS-DMA of one [32][32] fp32 tile (global rows 128 B apart) into the
// swizzled LDS tile layout of rows_to_lds, without staging registers: one
// wave-instruction writes 1 KiB of LDS linearly (lane l -> base + 16 l = row
// l >> 3, slot l & 7), so the swizzle is applied to the per-lane SOURCE chunk:
// slot s of row r holds global chunk s ^ (r & 7).  Rows outside [lo, hi) read
// as zero: the tile is zero-filled by ds_write first and the DMA of those rows
// is masked off.  `lds_tile` must be wave-uniform.  Completion: vmcnt.
// AUX: cache policy of the loads (16 = sc1, device scope: see wn_stack.hip).
template <int AUX = 0>
__device__ __forceinline__ void tile_dma(float* lds_tile,
                                         const float* __restrict__ tile0,
                                         int lane, int lo, int hi) {
  const int rr = lane >> 3;
  const float* src = tile0 + (long)rr * 32 + (((lane & 7) ^ (rr & 7)) << 2);
  if (lo <= 0 && hi >= 32) {  // wave-uniform: whole tile real
#pragma unroll
    for (int c = 0; c < 4; ++c)
      __builtin_amdgcn_global_load_lds((wn_gptr_t)(src + c * 256),
                                       (wn_lptr_t)(lds_tile + c * 256), 16, 0, AUX);
  } else {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *reinterpret_cast<f32x4*>(lds_tile + c * 256 + lane * 4) = zero;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int r = 8 * c + rr;
      if (r >= lo && r < hi)
        __builtin_amdgcn_global_load_lds((wn_gptr_t)(src + c * 256),
                                         (wn_lptr_t)(lds_tile + c * 256), 16, 0, AUX);
    }
  }
}

__device__ __forceinline__ void rows_store(float* __restrict__ tile0, int lane,
                                           int hi, const RowRegs& R) {
  float* p = tile0 + (long)(lane >> 3) * 32 + (lane & 7) * 4;
  if (hi >= 32) {
#pragma unroll
    for (int c = 0; c < 4; ++c) *reinterpret_cast<f32x4*>(p + c * 256) = R.v[c];
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int r = 8 * c + (lane >> 3);
      if (r < hi) *reinterpret_cast<f32x4*>(p + c * 256) = R.v[c];
    }
  }
}

__device__ __forceinline__ void rows_to_lds(float* tile, int lane,
                                            const RowRegs& R) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int r = 8 * c + (lane >> 3);
    *reinterpret_cast<f32x4*>(tile + r * 32 + (((lane & 7) ^ (r & 7)) << 2)) =
        R.v[c];
  }
}

__device__ __forceinline__ RowRegs rows_from_lds(const float* tile, int lane) {
  RowRegs R;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int r = 8 * c + (lane >> 3);
    R.v[c] = *reinterpret_cast<const f32x4*>(
        tile + r * 32 + (((lane & 7) ^ (r & 7)) << 2));
  }
  return R;
}

__device__ __forceinline__ f32x16 frag_from_lds(const float* tile, int j,
                                                int h) {
  f32x16 f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(
        tile + j * 32 + (((2 * q + h) ^ (j & 7)) << 2));
    f[4 * q + 0] = v[0];
    f[4 * q + 1] = v[1];
    f[4 * q + 2] = v[2];
    f[4 * q + 3] = v[3];
  }
  return f;
}

__device__ __forceinline__ void frag_to_lds(float* tile, int j, int h,
                                            const f32x16& f) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x4 v = {f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]};
    *reinterpret_cast<f32x4*>(tile + j * 32 + (((2 * q + h) ^ (j & 7)) << 2)) = v;
  }
}

// element [row][ch] of a swizzled tile (transposed, channel-on-lane reads)
__device__ __forceinline__ float tile_elem(const float* tile, int row, int ch) {
  return tile[row * 32 + (((ch >> 2) ^ (row & 7)) << 2) + (ch & 3)];
}

// Per-channel vector (bias) from LDS/global as a fragment (same value for
// every time row).
__device__ __forceinline__ f32x16 frag_bcast(const float* __restrict__ vec,
                                             int h) {
  f32x16 f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) f[4 * q + e] = vec[8 * q + 4 * h + e];
  }
  return f;
}

// acc^T[n0+i, time] += sum_k W[k][n0+i] * frag[time, k]   (k over 32 channels)
// wl: LDS, row-major [32][ldw] with the contraction index k as the row.
// `wl_lane` must already be  wl + n0 + i + 4*h*ldw  (per-lane base), so the
// 16 reads are base + compile-time offsets.
template <int LDW>
__device__ __forceinline__ void mma32(f32x16& acc, const f32x16& frag,
                                      const float* wl_lane) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float a = wl_lane[(8 * (r >> 2) + (r & 3)) * LDW];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, frag[r], acc, 0, 0, 0);
  }
}

__device__ __forceinline__ float wn_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.f + __expf(-x));
}
__device__ __forceinline__ float wn_tanh(float x) {
  // 1 - 2/(e^{2x}+1); saturates correctly at +-inf of the exp.
  return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * x));
}

// Backward of a residual block without pre-activation-gradient planes
// (layer_bwd2d_kernel in wn_layer.hip, stack_bwd_kernel in wn_stack.hip):
// transposed weight image per layer, 5 x [cout][33] + padding = 21 KiB
#define B2_WIMG 5376

// (da_f, da_g) fragments from dz, z, sigmoid fragments; tanh = z / sigmoid
__device__ __forceinline__ void gate_grad(const f32x16& dz, const f32x16& zz,
                                          const f32x16& ss, f32x16& df,
                                          f32x16& dg) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    // seven vector instructions per element (add, rcp, mul, fma, mul, fma,
    // mul): on gfx950 the f32 MFMA and the vector ALU are one resource, so
    // every instruction here is matrix-pipe time (tools/ubench/mfma_valu.hip).
    // A sigmoid that underflowed to 0 must not turn 0 * inf into NaN: + 1e-30
    // (no change to any sigmoid above 1e-22; fmaxf compiles to TWO v_max, the
    // first one canonicalising its operand).
    const float sgm = ss[r];
    const float th = zz[r] * __builtin_amdgcn_rcpf(sgm + 1e-30f);
    df[r] = dz[r] * __builtin_fmaf(-zz[r], th, sgm);      // dz * sig * (1 - tanh^2)
    dg[r] = dz[r] * __builtin_fmaf(-zz[r], sgm, zz[r]);   // dz * tanh * sig * (1 - sig)
  }
}

// ---------------------------------------------------------------------------
// The sampling draw of fast generation (generate.py:229-240), one copy for
// every draw site (tests/draw_ref.py restates it in float64 numpy):
//   p    = float32(softmax_f64(logits))            the probabilities returned
//   w_q  = exp(log(p_q) / tau - max)               w = p at tau == 1; 0 at p == 0
//   w_q  = 0 for the codes top-k / top-p drop      (wave_trunc_cut; off: none)
//   u    = uniform(seed, counter) * sum(w)         counter-based, no state
//   code = the inverse CDF of w at u
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the draw's uniform in [0, 1): the top 53 bits of splitmix64(seed ^ splitmix64(counter))
// (also in halves, for a caller that hashes before its logits are ready)
__device__ __forceinline__ uint64_t draw_bits(uint64_t seed, uint64_t counter) {
  return splitmix64(seed ^ splitmix64(counter));
}
__device__ __forceinline__ double draw_unit(uint64_t bits) {
  return (double)(bits >> 11) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ double draw_uniform(uint64_t seed, uint64_t counter) {
  return draw_unit(draw_bits(seed, counter));
}

// the weight exponent log(p) / tau; p == 0 (float32 underflow) gets -inf, so
// weight exactly 0 at any tau, as np.log(0) gives it in the reference
__device__ __forceinline__ double draw_log_weight(double p, double tau) {
  return p > 0.0 ? log(p) / tau : -INFINITY;
}

// ---- wave-wide reductions by DPP (row shifts inside the four 16-lane rows,
// then lane 15 / lane 31 broadcast to the following rows): an inclusive scan in
// six VALU steps, the total in lane 63 -- no LDS round trip per step as with
// ds_bpermute shuffles.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f32(float old, float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(x), CTRL,
                                                    ROW_MASK, 0xf, false));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double old, double x) {
  const long long o = __double_as_longlong(old), v = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_update_dpp((int)o, (int)v, CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(v >> 32), CTRL, ROW_MASK, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double readlane_f64(double x, int l) {
  const long long v = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readlane((int)v, l), hi = __builtin_amdgcn_readlane((int)(v >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// max over the wave, the same value in every lane
__device__ __forceinline__ float wave_max_f32(float x) {
  x = fmaxf(x, dpp_f32<0x111, 0xf>(x, x));   // row_shr:1
  x = fmaxf(x, dpp_f32<0x112, 0xf>(x, x));
  x = fmaxf(x, dpp_f32<0x114, 0xf>(x, x));
  x = fmaxf(x, dpp_f32<0x118, 0xf>(x, x));
  x = fmaxf(x, dpp_f32<0x142, 0xa>(x, x));   // row_bcast:15 -> rows 1, 3
  x = fmaxf(x, dpp_f32<0x143, 0xc>(x, x));   // row_bcast:31 -> rows 2, 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
__device__ __forceinline__ double wave_max_f64(double x) {
  x = fmax(x, dpp_f64<0x111, 0xf>(x, x));
  x = fmax(x, dpp_f64<0x112, 0xf>(x, x));
  x = fmax(x, dpp_f64<0x114, 0xf>(x, x));
  x = fmax(x, dpp_f64<0x118, 0xf>(x, x));
  x = fmax(x, dpp_f64<0x142, 0xa>(x, x));
  x = fmax(x, dpp_f64<0x143, 0xc>(x, x));
  return readlane_f64(x, 63);
}
// inclusive prefix sum over the lanes (lane 63: the wave's sum)
__device__ __forceinline__ double wave_scan_f64(double x) {
  x += dpp_f64<0x111, 0xf>(0.0, x);
  x += dpp_f64<0x112, 0xf>(0.0, x);
  x += dpp_f64<0x114, 0xf>(0.0, x);
  x += dpp_f64<0x118, 0xf>(0.0, x);
  x += dpp_f64<0x142, 0xa>(0.0, x);
  x += dpp_f64<0x143, 0xc>(0.0, x);
  return x;
}

// float64 softmax (model.py:620-621) by one wave of the Q logits in pd.
// Leaves the float32-rounded probabilities, the ones generate.py sees, in pd
// as doubles and stores them to po unless it is null.  Each exp is evaluated
// once and kept in pd.
__device__ __forceinline__ void wave_softmax_f64(double* pd, int Q, int lane, float* po) {
  double m = -1e300;
  for (int q = lane; q < Q; q += 64) m = fmax(m, pd[q]);
  for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  double se = 0.0;
  for (int q = lane; q < Q; q += 64) {
    const double e = exp(pd[q] - m);
    pd[q] = e;
    se += e;
  }
  for (int o = 32; o >= 1; o >>= 1) se += __shfl_xor(se, o);
  for (int q = lane; q < Q; q += 64) {
    const float p32 = (float)(pd[q] / se);
    if (po) po[q] = p32;
    pd[q] = (double)p32;
  }
}

// ---------------------------------------------------------------------------
// Top-k / nucleus (top-p) truncation of the draw (tests/trunc_ref.py restates
// it in float64 numpy; wavenet/sampling.py is the host's copy).  It acts on
// the tempered weights w, between the temperature and the inverse CDF:
//   top-k    keep the codes with w >= the top_k-th largest w (a tie at the cut
//            keeps its whole tie group); 0 or >= Q: off
//   nucleus  of what top-k kept, with total = sum(w): the smallest set
//            {w >= c} whose mass is >= (double)top_p * total; 0 or >= 1: off
// Dropped codes get weight exactly 0, so the inverse CDF never returns them.
// The rule selects on the float32 probabilities; w is a strictly increasing
// function of p (equal p give equal w), so the sets are the same.  Both are
// "the largest cut c with f({w >= c}) >= bound" for a monotone f (a count, a
// float64 mass added in one fixed order), found by bisection over the weights'
// bit patterns: non-negative doubles order as unsigned integers.  At tau == 1
// the weights are float32 values, whose low 29 mantissa bits are 0: the keys
// are shifted by `sh` = 29 then and the search takes half the probes.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool draw_trunc_on(int top_k, float top_p) {
  return top_k > 0 || (top_p > 0.f && top_p < 1.f);
}
__device__ __forceinline__ int draw_key_shift(float temperature) {
  return temperature == 1.0f ? 29 : 0;
}
__device__ __forceinline__ uint64_t draw_key(double w, int sh) {
  return (uint64_t)__double_as_longlong(w) >> sh;
}

// The cut of the Q weights w (LDS, read only) by one whole wave: keep code q
// iff draw_key(w[q], sh) >= the returned key (the same value in every lane).
// Lane l adds its weights q = l, l + 64, ... in ascending order, the lanes'
// sums are added by wave_scan_f64: every probe's mass is summed the same way.
__device__ __forceinline__ uint64_t wave_trunc_cut(const double* w, int Q, int lane, int top_k,
                                                   float top_p, int sh) {
  double mx = 0.0, nmn = -INFINITY;
  for (int q = lane; q < Q; q += 64) {
    mx = fmax(mx, w[q]);
    nmn = fmax(nmn, -w[q]);
  }
  uint64_t lo = draw_key(-wave_max_f64(nmn), sh);      // every code is >= lo
  const uint64_t hi = draw_key(wave_max_f64(mx), sh);
  if (top_k > 0 && top_k < Q) {
    uint64_t b = hi;
    while (lo < b) {                                   // count(key >= lo) >= top_k holds
      const uint64_t mid = lo + ((b - lo + 1) >> 1);
      int n = 0;
      for (int q0 = 0; q0 < Q; q0 += 64) {             // (wave-uniform trip count)
        const int q = q0 + lane;
        n += __popcll(__builtin_amdgcn_ballot_w64(q < Q && draw_key(w[q < Q ? q : 0], sh) >= mid));
      }
      if (n >= top_k) lo = mid; else b = mid - 1;
    }
  }
  if (top_p > 0.f && top_p < 1.f) {
    auto mass = [&](uint64_t c) {
      double s = 0.0;
      for (int q = lane; q < Q; q += 64) {
        const double v = w[q];
        s += draw_key(v, sh) >= c ? v : 0.0;
      }
      return readlane_f64(wave_scan_f64(s), 63);
    };
    const double bound = (double)top_p * mass(lo);     // of what top-k kept
    uint64_t b = hi;
    while (lo < b) {                                   // mass(key >= lo) >= bound holds
      const uint64_t mid = lo + ((b - lo + 1) >> 1);
      if (mass(mid) >= bound) lo = mid; else b = mid - 1;
    }
  }
  return lo;
}

// The draw by one wave from the probabilities wave_softmax_f64 left in pd
// (overwritten with the weights): temperature, the truncation above (top_k =
// 0, top_p = 0: none), then the inverse CDF over per-lane contiguous segments
// (segment sums -> prefix sum -> pick) with the uniform of (seed, counter).
// Returns the code in every lane.
__device__ __forceinline__ int wave_draw_f64(double* pd, int Q, int lane, float temperature,
                                             int top_k, float top_p, uint64_t seed,
                                             uint64_t counter) {
  if (temperature != 1.0f) {
    const double tau = (double)temperature;
    double mx = -1e300;
    for (int q = lane; q < Q; q += 64) {
      const double lp = draw_log_weight(pd[q], tau);
      pd[q] = lp;
      mx = fmax(mx, lp);
    }
    for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    for (int q = lane; q < Q; q += 64) pd[q] = exp(pd[q] - mx);
  }
  if (draw_trunc_on(top_k, top_p)) {
    const int sh = draw_key_shift(temperature);
    const uint64_t cut = wave_trunc_cut(pd, Q, lane, top_k, top_p, sh);
    for (int q = lane; q < Q; q += 64)
      if (draw_key(pd[q], sh) < cut) pd[q] = 0.0;
  }
  __builtin_amdgcn_wave_barrier();
  const int per = (Q + 63) / 64;
  const int q0 = lane * per, q1 = min(Q, q0 + per);
  double seg = 0.0;
  for (int q = q0; q < q1; ++q) seg += pd[q];
  double incl = seg;
  for (int o = 1; o < 64; o <<= 1) {
    const double v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  const double total = __shfl(incl, 63);
  const double u = draw_uniform(seed, counter) * total;
  // (the neighbour's inclusive sum, not incl - seg: the lanes' intervals
  // then tile [0, total) exactly -- no gap a draw could fall into)
  const double up = __shfl_up(incl, 1);
  const double excl = lane == 0 ? 0.0 : up;
  int pick = -1;
  if (u >= excl && u < incl) {
    double c = excl;
    pick = q1 - 1;
    for (int q = q0; q < q1; ++q) {
      c += pd[q];
      if (u < c) { pick = q; break; }
      if (pd[q] > 0.0) pick = q;   // (u past the rounded walk: the last code of weight > 0)
    }
  }
  // exactly one lane holds the pick (u < total); fall back to Q - 1
  int best = pick;
  for (int o = 32; o >= 1; o >>= 1) best = max(best, __shfl_xor(best, o));
  return best < 0 ? Q - 1 : best;
}

#endif  // __HIPCC__
