// Pitch path (include/wavenet_pitch_path.h states the rule; wavenet/pitch.py's
// PitchPath.reference restates it in numpy float32, tests/pitch_path_ref.py in
// float64): a Viterbi path over the frames of a clip through the lag
// candidates of the tracker's c' rows.  Strictly serial in the frame index, so
// one workgroup walks one clip and what counts is the time per frame.
//
// A lane owns PATH_PER = 4 consecutive states in registers; WAVES = 1 serves
// N <= 256 states, WAVES = 4 the rest.  Per frame:
//   1. the next frame's c' values and tracker lag are loaded (used after 3.)
//   2. A = V - p upwards, Bk = V + p downwards, min V: the lane folds its four
//      states, the wave scans by DPP row shifts (path_scan_up / _down: no LDS
//      round trip per step), the waves' totals cross through LDS (slots scan_v
//      / scan_i) behind ONE barrier
//   3. nV, nU and the predecessors (int16, to the workspace)
//   4. m = min(min nV, nU) through LDS (slot norm) behind a second barrier
// Every index that is ever stored or used as an address is a state's own
// index clamped to [0, N - 1], or N: see the header.
#include "wn_common.h"

#define PATH_PER 4
#define PATH_MAX_TAU 1024
#define PATH_MAX_F (1 << 20)

struct PathArgs {
  const float* cmnd;
  const int32_t* lag_in;
  const int32_t* nframes;
  const float* pen;
  const float* bias;
  int16_t* pred;
  float* f0;
  float* aper;
  int32_t* lag;
  double* cost;
  int F, tau_min, tau_max;
  float sw, unv, sr;
};

struct MinIdx {
  float v;
  int i;
};

// `l` covers lower indices than `r`: the smaller value, the left one at a tie
// (and whenever the comparison is unordered)
__device__ __forceinline__ MinIdx path_op(MinIdx l, MinIdx r) { return r.v < l.v ? r : l; }

__device__ __forceinline__ MinIdx path_shfl_up(MinIdx x, int o) {
  MinIdx y = {__shfl_up(x.v, o, 64), __shfl_up(x.i, o, 64)};
  return y;
}
__device__ __forceinline__ MinIdx path_shfl_down(MinIdx x, int o) {
  MinIdx y = {__shfl_down(x.v, o, 64), __shfl_down(x.i, o, 64)};
  return y;
}

// x as the DPP pattern CTRL moves it; a lane without a source lane (or in a
// row outside ROW_MASK) reads itself, and path_op(x, x) is x
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ MinIdx path_dpp(MinIdx x) {
  MinIdx y = {dpp_f32<CTRL, ROW_MASK>(x.v, x.v),
              __builtin_amdgcn_update_dpp(x.i, x.i, CTRL, ROW_MASK, 0xf, false)};
  return y;
}
__device__ __forceinline__ MinIdx path_readlane(MinIdx x, int l) {
  MinIdx y = {__int_as_float(__builtin_amdgcn_readlane(__float_as_int(x.v), l)),
              __builtin_amdgcn_readlane(x.i, l)};
  return y;
}

// inclusive scan towards the higher lanes (lane 63: the wave's total): row
// shifts right inside the four 16-lane rows, then lane 15 / lane 31 broadcast
// to the following rows -- the source is always the lower lanes, the left
// operand
__device__ __forceinline__ MinIdx path_scan_up(MinIdx x) {
  x = path_op(path_dpp<0x111, 0xf>(x), x);    // row_shr:1
  x = path_op(path_dpp<0x112, 0xf>(x), x);
  x = path_op(path_dpp<0x114, 0xf>(x), x);
  x = path_op(path_dpp<0x118, 0xf>(x), x);
  x = path_op(path_dpp<0x142, 0xa>(x), x);    // row_bcast:15 -> rows 1, 3
  x = path_op(path_dpp<0x143, 0xc>(x), x);    // row_bcast:31 -> rows 2, 3
  return x;
}

// the mirrored scan (lane 0: the wave's total): row shifts left, then the
// totals of the rows above from lanes 16 / 48 and of the upper half from lane
// 32 (there is no broadcast towards the lower rows)
__device__ __forceinline__ MinIdx path_scan_down(MinIdx x, int lane) {
  x = path_op(x, path_dpp<0x101, 0xf>(x));    // row_shl:1
  x = path_op(x, path_dpp<0x102, 0xf>(x));
  x = path_op(x, path_dpp<0x104, 0xf>(x));
  x = path_op(x, path_dpp<0x108, 0xf>(x));
  const MinIdx r1 = path_readlane(x, 16), r3 = path_readlane(x, 48);
  if ((lane >> 4) == 0) x = path_op(x, r1);
  if ((lane >> 4) == 2) x = path_op(x, r3);
  const MinIdx up = path_readlane(x, 32);
  if (lane < 32) x = path_op(x, up);
  return x;
}

// min over the wave, the same value in every lane
__device__ __forceinline__ float path_wave_min(float x) {
  float y;
  y = dpp_f32<0x111, 0xf>(x, x); x = y < x ? y : x;
  y = dpp_f32<0x112, 0xf>(x, x); x = y < x ? y : x;
  y = dpp_f32<0x114, 0xf>(x, x); x = y < x ? y : x;
  y = dpp_f32<0x118, 0xf>(x, x); x = y < x ? y : x;
  y = dpp_f32<0x142, 0xa>(x, x); x = y < x ? y : x;
  y = dpp_f32<0x143, 0xc>(x, x); x = y < x ? y : x;
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void pitch_path_kernel(PathArgs a) {
#pragma clang fp contract(off)
  constexpr int THREADS = 64 * WAVES;
  __shared__ float scan_v[3][4];
  __shared__ int scan_i[3][4];
  __shared__ float norm[4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int F = a.F, tmin = a.tau_min, N = a.tau_max - a.tau_min;
  const int R = a.tau_max + 1;                  // a c' row
  int Fb = a.nframes ? a.nframes[b] : F;
  Fb = Fb < 0 ? 0 : (Fb > F ? F : Fb);
  const float* crow0 = a.cmnd + (long)b * F * R;
  const int32_t* lin = a.lag_in + (long)b * F;
  int16_t* prow0 = a.pred + (long)b * F * (N + 1);
  float* f0 = a.f0 + (long)b * F;
  float* aper = a.aper + (long)b * F;
  int32_t* lag = a.lag + (long)b * F;

  for (int f = Fb + tid; f < F; f += THREADS) {
    f0[f] = 0.f;
    aper[f] = 0.f;
    lag[f] = 0;
  }
  if (Fb == 0) {                                // (workgroup-uniform)
    if (tid == 0) a.cost[b] = 0.0;
    return;
  }

  // this lane's states: s, real or not, and the in-range index that stands
  // for it everywhere (N - 1 behind the last state)
  bool ok[PATH_PER];
  int sc[PATH_PER];
  float p[PATH_PER], bs[PATH_PER];
#pragma unroll
  for (int j = 0; j < PATH_PER; ++j) {
    const int s = PATH_PER * tid + j;
    ok[j] = s < N;
    sc[j] = ok[j] ? s : N - 1;
    p[j] = a.pen[tmin + sc[j]];
    bs[j] = a.bias[tmin + sc[j]];
  }

  float V[PATH_PER], U;
  double cost = 0.0;

  // m = min(min V, U); V -= m; U -= m; cost += m
  auto normalise = [&]() {
    float mn = V[0];
#pragma unroll
    for (int j = 1; j < PATH_PER; ++j) mn = V[j] < mn ? V[j] : mn;
    mn = path_wave_min(mn);
    if (lane == 0) norm[wave] = mn;
    __syncthreads();
    float m = norm[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
      const float y = norm[w];
      m = y < m ? y : m;
    }
    m = U < m ? U : m;
#pragma unroll
    for (int j = 0; j < PATH_PER; ++j) V[j] = V[j] - m;
    U = U - m;
    cost += (double)m;
  };

  // ---- frame 0
  {
    const float* cr = crow0 + tmin;
#pragma unroll
    for (int j = 0; j < PATH_PER; ++j) V[j] = ok[j] ? cr[sc[j]] + bs[j] : INFINITY;
    U = lin[0] == 0 ? 0.f : a.unv;
  }
  normalise();

  int last = N;
  for (int f = 1;; ++f) {
    // ---- 1. the next frame's inputs, ahead of the scans
    float c[PATH_PER] = {0.f, 0.f, 0.f, 0.f};
    int lg = 0;
    if (f < Fb) {                               // (workgroup-uniform)
      const float* cr = crow0 + (long)f * R + tmin;
#pragma unroll
      for (int j = 0; j < PATH_PER; ++j) c[j] = cr[sc[j]];
      lg = lin[f];
    }

    // ---- 2. the one-sided minima and min V
    MinIdx pa[PATH_PER], sb[PATH_PER], mv;
    pa[0].v = V[0] - p[0];
    pa[0].i = sc[0];
    mv.v = V[0];
    mv.i = sc[0];
#pragma unroll
    for (int j = 1; j < PATH_PER; ++j) {
      const MinIdx x = {V[j] - p[j], sc[j]}, y = {V[j], sc[j]};
      pa[j] = path_op(pa[j - 1], x);
      mv = path_op(mv, y);
    }
    sb[PATH_PER - 1].v = V[PATH_PER - 1] + p[PATH_PER - 1];
    sb[PATH_PER - 1].i = sc[PATH_PER - 1];
#pragma unroll
    for (int j = PATH_PER - 2; j >= 0; --j) {
      const MinIdx x = {V[j] + p[j], sc[j]};
      sb[j] = path_op(x, sb[j + 1]);
    }
    const MinIdx wa = path_scan_up(pa[PATH_PER - 1]);
    const MinIdx wb = path_scan_down(sb[0], lane);
    mv = path_readlane(path_scan_up(mv), 63);
    if (lane == 63) {
      scan_v[0][wave] = wa.v;
      scan_i[0][wave] = wa.i;
    }
    if (lane == 0) {
      scan_v[1][wave] = wb.v;
      scan_i[1][wave] = wb.i;
      scan_v[2][wave] = mv.v;
      scan_i[2][wave] = mv.i;
    }
    // what lies below / above this lane inside its wave
    MinIdx xa = path_shfl_up(wa, 1), xb = path_shfl_down(wb, 1);
    bool ha = lane > 0, hb = lane < 63;
    __syncthreads();
#pragma unroll
    for (int w = WAVES - 1; w >= 0; --w)
      if (w < wave) {
        const MinIdx t = {scan_v[0][w], scan_i[0][w]};
        xa = ha ? path_op(t, xa) : t;
        ha = true;
      }
#pragma unroll
    for (int w = 0; w < WAVES; ++w)
      if (w > wave) {
        const MinIdx t = {scan_v[1][w], scan_i[1][w]};
        xb = hb ? path_op(xb, t) : t;
        hb = true;
      }
    MinIdx km = {scan_v[2][0], scan_i[2][0]};
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
      const MinIdx t = {scan_v[2][w], scan_i[2][w]};
      km = path_op(km, t);
    }

    if (f == Fb) {                              // (workgroup-uniform) the end
      last = U <= km.v ? N : km.i;
      break;
    }

    // ---- 3. the frame's costs and predecessors
    int16_t* prow = prow0 + (long)f * (N + 1);
    const float fu = U + a.sw;
#pragma unroll
    for (int j = 0; j < PATH_PER; ++j) {
      const MinIdx ma = ha ? path_op(xa, pa[j]) : pa[j];
      const MinIdx mb = hb ? path_op(sb[j], xb) : sb[j];
      const float L = ma.v + p[j], Rr = mb.v - p[j];
      const bool left = L <= Rr;
      const float vv = left ? L : Rr;
      const int pvoiced = left ? ma.i : mb.i;
      const bool voiced = vv <= fu;
      const float pv = voiced ? vv : fu;
      const float loc = c[j] + bs[j];
      V[j] = ok[j] ? pv + loc : INFINITY;
      if (ok[j]) prow[sc[j]] = (int16_t)(voiced ? pvoiced : N);
    }
    {
      const float fv = km.v + a.sw;
      const float lu = lg == 0 ? 0.f : a.unv;
      const bool stay = U <= fv;
      if (tid == 0) prow[N] = (int16_t)(stay ? N : km.i);
      U = (stay ? U : fv) + lu;
    }

    // ---- 4.
    normalise();
  }

  // ---- the walk back (lane 0), then f0 and aper by all lanes
  __syncthreads();
  if (tid == 0) {
    int st = last;
    for (int f = Fb - 1; f >= 0; --f) {
      lag[f] = st < N ? tmin + st : 0;
      if (f > 0) {
        const int pr = prow0[(long)f * (N + 1) + st];
        st = pr < 0 ? 0 : (pr > N ? N : pr);
      }
    }
    a.cost[b] = cost;
  }
  __syncthreads();
  for (int f = tid; f < Fb; f += THREADS) {
    const int tau = lag[f];
    float fo = 0.f, ap = 1.f;
    if (tau >= tmin && tau < a.tau_max) {       // (0: unvoiced)
      const float* cr = crow0 + (long)f * R;
      const float ca = cr[tau - 1], cb = cr[tau], cg = cr[tau + 1];
      const float den = (ca - 2.f * cb) + cg;
      float delta = 0.f;
      if (den > 0.f) {
        delta = 0.5f * (ca - cg) / den;
        delta = delta < -0.5f ? -0.5f : (delta > 0.5f ? 0.5f : delta);
      }
      fo = a.sr / ((float)tau + delta);
      ap = cb;
    }
    f0[f] = fo;
    aper[f] = ap;
  }
}

static bool path_shape_ok(int B, int F, int tau_min, int tau_max) {
  return B >= 1 && B <= 65535 && F >= 1 && F <= PATH_MAX_F && tau_min >= 2 &&
         tau_max <= PATH_MAX_TAU && tau_min + 2 <= tau_max;
}

extern "C" {

long wn_pitch_path_workspace_bytes(int B, int F, int tau_min, int tau_max) {
  if (!path_shape_ok(B, F, tau_min, tau_max)) return -1;
  return 2L * B * F * (tau_max - tau_min + 1);
}

int wn_pitch_path(const float* cmnd, const int32_t* lag_in,
                  const int32_t* nframes, int B, int F, int tau_min,
                  int tau_max, const float* pen, const float* bias,
                  float switch_cost, float unvoiced_cost, float sample_rate,
                  void* workspace, float* f0, float* aper, int32_t* lag,
                  double* cost, void* stream) {
  if (!cmnd || !lag_in || !pen || !bias || !workspace || !f0 || !aper ||
      !lag || !cost)
    return WN_ERR_NULL;
  if (!path_shape_ok(B, F, tau_min, tau_max)) return WN_ERR_BAD_SHAPE;
  if ((reinterpret_cast<uintptr_t>(cmnd) & 3u) ||
      (reinterpret_cast<uintptr_t>(lag_in) & 3u) ||
      (reinterpret_cast<uintptr_t>(nframes) & 3u) ||
      (reinterpret_cast<uintptr_t>(pen) & 3u) ||
      (reinterpret_cast<uintptr_t>(bias) & 3u) ||
      (reinterpret_cast<uintptr_t>(workspace) & 1u) ||
      (reinterpret_cast<uintptr_t>(f0) & 3u) ||
      (reinterpret_cast<uintptr_t>(aper) & 3u) ||
      (reinterpret_cast<uintptr_t>(lag) & 3u) ||
      (reinterpret_cast<uintptr_t>(cost) & 7u))
    return WN_ERR_MISALIGNED;
  PathArgs a;
  a.cmnd = cmnd;
  a.lag_in = lag_in;
  a.nframes = nframes;
  a.pen = pen;
  a.bias = bias;
  a.pred = static_cast<int16_t*>(workspace);
  a.f0 = f0;
  a.aper = aper;
  a.lag = lag;
  a.cost = cost;
  a.F = F;
  a.tau_min = tau_min;
  a.tau_max = tau_max;
  a.sw = switch_cost;
  a.unv = unvoiced_cost;
  a.sr = sample_rate;
  if (tau_max - tau_min <= 64 * PATH_PER)
    hipLaunchKernelGGL(pitch_path_kernel<1>, dim3((unsigned)B), dim3(64), 0,
                       (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(pitch_path_kernel<4>, dim3((unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, a);
  return wn_check_launch();
}

}  // extern "C"
