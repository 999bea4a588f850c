// Batched fast generation: B independent streams stepped in lock step
// (WaveNetModel.generate_batch).  The batched counterpart of the step kernels
// of wn_fastgen.hip (wn_fastgen_step): the reference's generator is batch
// shaped (every FIFO queue holds (batch_size, channels) rows, model.py:450-485),
// and with B streams each layer of the serial chain becomes a [B, 32] x [32, 64]
// product, so the streams sit on the rows of v_mfma_f32_16x16x4_f32.
//
// One step, five launches (no in-launch waits, no cooperative launch):
//   fgb_draw_kernel     B waves     : the PREVIOUS step's float64 softmax,
//                                     temperature and inverse-CDF draw, one
//                                     wave per stream (when one is pending)
//   fgb_chain_kernel    Bp/32 WGs   : the L layers for a group of 32 streams
//                                     (4 waves, one 16 x 16 output tile each)
//   fgb_skip_kernel     many WGs    : h1 = relu(z_all . Ws + bsum), and the
//                                     NEXT step's past-tap pre-activations of
//                                     every (layer, group)
//   fgb_post1_kernel                : h2 = relu(h1 . W1 + b1)
//   fgb_logits_kernel               : logits = h2 . W2 + b2 (a draw pending)
// wn_fastgen_batch_finish draws for the last step of a sequence.
//
// Batch invariance: a row's arithmetic never depends on B or on the stream's
// position.  The MFMA tiles have a fixed height (zero-filled rows past B), an
// f32 MFMA is an fmaf chain per output element whatever its row, and every
// K split is a function of the model shape only.  Stream b therefore gives
// bitwise the same probabilities and codes alone or inside any batch.
//
// State: ring row [sum(d)][Bp][32] (all streams share one cursor), so a
// layer's past tap is one contiguous read for a whole group.
//
// Restarts (bulk synthesis refills a finished stream's slot): the counter
// rule of the draw is counter = step; the origin rule of the _q entries is
// counter = step - origin[b].  fgb_restart_kernel zeroes a stream's ring
// columns, clears its previous code and sets its origin to the current step,
// after which the stream is bit for bit a fresh one; the ring position stays
// the shared cursors[0] % d.  fgb_lc_rows_kernel gathers the LC rows of a
// segment for streams that hold different items.
//
// The two ends are replaceable (wn_fastgen_batch.h): the chain kernel's input
// stage is a template parameter, one-hot codes (two gathered rows of the
// causal filter) or levels (a mixture-of-logistics model's scalar input: the
// K0 taps of the causal filter over a 64-slot history of each stream's
// levels, staged through LDS), and wn_fastgen_mol.hip puts the mixture draw
// where fgb_draw_kernel stands.  Everything between them -- rings, past-tap
// pre-activations, LC ring, skip / post GEMMs -- is the same launch for both.
#include "wn_fastgen_batch.h"
#include "wn_mol_draw.h"   // mol_centre, MOL_TOP

// 16 x 16 x 4 f32 MFMA.  Lane l: A[l & 15][k = l >> 4], B[k = l >> 4][l & 15];
// C/D: column l & 15, rows 4 (l >> 4) + r.
__device__ __forceinline__ f32x4 fgb_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------- the draw
// The draw of wn_common.h for stream b: its own rows and seed, counter = the
// step that produced the logits (the counter rule of tests/draw_ref.py).  One
// wave; pd: FGB_MAXQ doubles of LDS owned by it.  ORIGIN (the _q entries): the
// counter is the stream's own step, step - origin[b], so that a stream
// restarted at step T0 (wn_fastgen_batch_restart) draws as a fresh one does.
template <bool ORIGIN>
__device__ void fgb_draw_wave(const FgBatch& g, double* pd, int lane, int b, int step) {
  const int Q = g.Q;
  const float* lg = g.logits + (long)b * Q;
  const int local = step - g.ctl[FGB_CTL_BASE];
  const int proba_every = g.ctl[FGB_CTL_PEVERY] > 0 ? g.ctl[FGB_CTL_PEVERY] : 1;
  for (int q = lane; q < Q; q += 64) pd[q] = (double)lg[q];
  __builtin_amdgcn_wave_barrier();
  const bool want_p = g.proba_out && (local % proba_every == 0);
  wave_softmax_f64(pd, Q, lane,
                   want_p ? g.proba_out + ((long)b * g.ctl[FGB_CTL_LDP] + local / proba_every) * Q
                          : nullptr);
  if (local + 1 < g.ctl[FGB_CTL_NGIVEN]) return;   // still inside the given samples
  const int code = wave_draw_f64(pd, Q, lane, __int_as_float(g.ctl[FGB_CTL_TEMP]),
                                 g.ctl[FGB_CTL_TOPK], __int_as_float(g.ctl[FGB_CTL_TOPP]),
                                 g.seeds[b],
                                 ORIGIN ? (uint64_t)(step - g.origin[b]) : (uint64_t)step);
  if (lane == 0) g.samples[(long)b * g.ctl[FGB_CTL_LDS] + local + 1] = code;
}

// one wave per stream; reads the cursors, writes none (the chain kernel that
// follows clears the pending flag, wn_fastgen_batch_finish a memset)
__global__ __launch_bounds__(256) void fgb_draw_kernel(FgBatch g) {
  __shared__ double pd[4][FGB_MAXQ];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + w;
  if (!g.cursors[1] || b >= g.B) return;
  fgb_draw_wave<false>(g, pd[w], lane, b, g.cursors[0] - 1);
}

__global__ __launch_bounds__(256) void fgb_draw_q_kernel(FgBatch g) {
  __shared__ double pd[4][FGB_MAXQ];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + w;
  if (!g.cursors[1] || b >= g.B) return;
  fgb_draw_wave<true>(g, pd[w], lane, b, g.cursors[0] - 1);
}

// ------------------------------------------------------------- the restart
// A flagged stream becomes a fresh one: its 32 floats of every ring row are
// zeroed (a FIFO of zeros is the same wherever its head sits, so the shared
// ring position needs no reset), prev = -1, origin = the step the queues are
// at.  Workgroup (x, y): the streams 32 y .. 32 y + 31, ring rows x, x +
// gridDim.x, ...; a thread: one float4 of one stream.  prev or hist (levels
// input: the stream's 64 history slots become -1, eight a thread) is null.
__global__ __launch_bounds__(256) void fgb_restart_kernel(
    float* state, const int32_t* dil, int L, int B, int Bp, const int32_t* cursors,
    int32_t* prev, int32_t* hist, int32_t* origin, const int32_t* flags) {
  const int tid = threadIdx.x;
  const int b = blockIdx.y * FGB_TILE + (tid >> 3);
  const bool on = b < B && flags[b] != 0;
  int rows = 0;
  for (int l = 0; l < L; ++l) rows += dil[l];
  if (on) {
    const float4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int r = blockIdx.x; r < rows; r += gridDim.x)
      *reinterpret_cast<float4*>(state + ((long)r * Bp + b) * 32 + (tid & 7) * 4) = zero;
    if (blockIdx.x == 0 && hist) {
#pragma unroll
      for (int i = 0; i < FGB_HIST / 8; ++i) hist[b * FGB_HIST + (tid & 7) * 8 + i] = -1;
    }
    if (blockIdx.x == 0 && (tid & 7) == 0) {
      if (prev) prev[b] = -1;
      origin[b] = cursors[0];
    }
  }
}

// ------------------------------------------------- a segment's LC rows
// out[b][j] = row t - 1 of stream b's item for its own step t = pos0 + j -
// origin_b in [1, m_b], zeros elsewhere.  table [B][3] (int64): the address
// of the item's rows [m_b][Lc] (0: none), origin_b, m_b.
__global__ __launch_bounds__(256) void fgb_lc_rows_kernel(const long long* table, int B, int n,
                                                          int Lc, long pos0, float* out) {
  const long total = (long)B * n * Lc;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % Lc);
    const long bj = i / Lc;
    const int j = (int)(bj % n), b = (int)(bj / n);
    const float* src = reinterpret_cast<const float*>(table[3 * b]);
    const long t = pos0 + j - table[3 * b + 1];
    float v = 0.f;
    if (src && t >= 1 && t <= table[3 * b + 2]) v = src[(t - 1) * Lc + c];
    out[i] = v;
  }
}

// ---------------------------------------------------------------- the chain
// Workgroup = 32 streams, 4 waves; wave w owns output tile (rows 16 (w & 1),
// columns 16 (w >> 1)) of the filter, the gate (same rows / columns, so
// tanh . sigmoid stays in the lane) and the dense output.  x and z pass
// between the waves through LDS (two barriers a layer).  Each layer's
// B operands, dense bias and past-tap pre-activations are loaded into
// registers two layers ahead (they do not depend on the chain).
struct FgbLW {
  float f[8], gt[8], d[8];   // Wf[1], Wg[1], Wd: B[k = 4 s + kk][col]
  float pf[4], pg[4];        // pre[l][row][col], pre[l][row][32 + col]
  float bd;
};

// LEVELS (the input stage): false, one-hot codes, x = W[0][prev] + W[1][code];
// true, levels: the rule of scalar_causal_fwd_kernel (wn_misc.hip) on the
// stream's history ring,
//   x[col] = sum_k W[k][col] c(hist[(T - s_k) & 63]),
//   s_k = (K0 - 1 - k) + (K0 - 1) / 2, c = mol_centre,
// taps k ascending from +0, one fmaf each; a slot that holds no level in
// 0 .. 65535 is skipped (the zero padding of training).  Slot T & 63 gets the
// level this step consumes.  The group's 32 x 64 slots, as centres, and the
// K0 x 32 filter are staged through LDS (rows 65 words apart: the four rows a
// wave reads fall on different banks).
#define FGB_HLD (FGB_HIST + 1)
#define FGB_EMPTY 2.f    // (centres lie in [-1, 1])

template <bool LEVELS>
__global__ __launch_bounds__(256) void fgb_chain_kernel(FgBatch g) {
  __shared__ float xs[FGB_TILE * FGB_XLD];
  __shared__ float zs[FGB_TILE * FGB_XLD];
  __shared__ int roff_s[FGB_MAXL], pos_s[FGB_MAXL];
  __shared__ float hs[LEVELS ? FGB_TILE * FGB_HLD : 1];   // centres; FGB_EMPTY: no level
  __shared__ int cur_s[LEVELS ? FGB_TILE : 1];            // the level this step consumes
  __shared__ float wcs[LEVELS ? FGB_MAXK0 * 32 : 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int rb = w & 1, cb = w >> 1;
  const int ci = lane & 15, kk = lane >> 4;
  const int col = cb * 16 + ci;            // this lane's output channel
  const int arow = rb * 16 + ci;           // this lane's A-operand row
  const int row0 = rb * 16 + kk * 4;       // first of its four output rows
  const int b0 = blockIdx.x * FGB_TILE;
  const int L = g.L, Q = g.Q, Bp = g.Bp, KZ = g.L * 32;
  const int T = g.cursors[0];
  const int local = T - g.ctl[FGB_CTL_BASE];
  const long lds = g.ctl[FGB_CTL_LDS];

  auto load = [&](FgbLW& W, int l) {
    if (l < L) {
      const float* blk = g.layer0 + (long)l * g.layer_stride;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int k = 4 * s + kk;
        W.f[s] = blk[1 * 1024 + k * 32 + col];
        W.gt[s] = blk[3 * 1024 + k * 32 + col];
        W.d[s] = blk[4 * 1024 + k * 32 + col];
      }
      const float* pr = g.pre + ((long)l * Bp + b0 + row0) * 64 + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        W.pf[r] = pr[r * 64];
        W.pg[r] = pr[r * 64 + 32];
      }
      W.bd = g.use_dense_bias ? blk[LAYER_OFF_BD + col] : 0.f;
    }
  };
  FgbLW wa, wb;
  load(wa, 0);
  load(wb, 1);

  if (w == 0) {   // ring offsets = exclusive prefix sum of the dilations
    const int dl = lane < L ? g.dil[lane] : 0;
    int incl = dl;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane < L) {
      roff_s[lane] = incl - dl;
      pos_s[lane] = T % dl;
    }
  }
  float x[4];
  int code[4];
  const int slot = T & (FGB_HIST - 1);
  if constexpr (LEVELS) {
    // causal layer on levels.  Staging: a stream's 64 slots, the one of this
    // step already holding the level it consumes; rows past B hold nothing
    const int K0 = g.K0;
    for (int i = tid; i < FGB_TILE * FGB_HIST; i += 256) {
      const int r = i >> 6, sl = i & (FGB_HIST - 1);
      const int b = b0 + r;
      int v = -1;
      if (b < g.B)
        v = sl == slot ? g.samples[b * lds + local] : g.hist[(long)b * FGB_HIST + sl];
      // (one conversion a slot here, not one a tap and lane below)
      hs[r * FGB_HLD + sl] = v >= 0 && v <= MOL_TOP ? mol_centre(v) : FGB_EMPTY;
      if (sl == slot) cur_s[r] = v;
    }
    for (int i = tid; i < K0 * 32; i += 256) wcs[i] = g.causal[i];
    __syncthreads();
    const int extra = (K0 - 1) / 2;
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = 0.f;
    const float* h = hs + row0 * FGB_HLD;
#pragma unroll 4
    for (int k = 0; k < K0; ++k) {
      const int sl = (T - ((K0 - 1 - k) + extra)) & (FGB_HIST - 1);
      const float wk = wcs[k * 32 + col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float c = h[r * FGB_HLD + sl];
        if (c <= 1.f) x[r] = fmaf(wk, c, x[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      code[r] = cur_s[row0 + r];
      xs[(row0 + r) * FGB_XLD + col] = x[r];
    }
  } else {
    // causal layer (filter width 2): x = W[0][prev] + W[1][code]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + row0 + r;
      int c = -1, p = -1;
      if (b < g.B) {
        c = g.samples[b * lds + local];
        p = g.prev[b];
      }
      float v = 0.f;
      if (p >= 0 && p < Q) v = g.causal[(long)p * 32 + col];
      if (c >= 0 && c < Q) v += g.causal[((long)Q + c) * 32 + col];
      x[r] = v;
      code[r] = c;
      xs[(row0 + r) * FGB_XLD + col] = v;
    }
  }
  __syncthreads();
  // (every wave has read prev[] / staged hist[] for its rows)
  if (cb == 0 && ci == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (b0 + row0 + r < g.B) {
        if constexpr (LEVELS)
          g.hist[(long)(b0 + row0 + r) * FGB_HIST + slot] = code[r];
        else
          g.prev[b0 + row0 + r] = code[r];
      }
  }
  if (blockIdx.x == 0 && tid == 0) g.cursors[1] = 0;   // the draw has run

  auto body = [&](int l, const FgbLW& W) {
    // enqueue x_l[T]
    float* ring = g.state + ((long)(roff_s[l] + pos_s[l]) * Bp + b0 + row0) * 32 + col;
#pragma unroll
    for (int r = 0; r < 4; ++r) ring[r * 32] = x[r];
    f32x4 af = {W.pf[0], W.pf[1], W.pf[2], W.pf[3]};
    f32x4 ag = {W.pg[0], W.pg[1], W.pg[2], W.pg[3]};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const float a = xs[arow * FGB_XLD + 4 * s + kk];
      af = fgb_mfma(a, W.f[s], af);
      ag = fgb_mfma(a, W.gt[s], ag);
    }
    float* zo = g.z_all + (long)(b0 + row0) * KZ + l * 32 + col;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // tanh(a) = 2 sigmoid(2 a) - 1, as the single-stream chain
      const float th = fmaf(2.f, wn_sigmoid(2.f * af[r]), -1.f);
      const float z = th * wn_sigmoid(ag[r]);
      zo[(long)r * KZ] = z;
      zs[(row0 + r) * FGB_XLD + col] = z;
    }
    __syncthreads();
    if (l + 1 < L) {
      f32x4 ad = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 8; ++s)
        ad = fgb_mfma(zs[arow * FGB_XLD + 4 * s + kk], W.d[s], ad);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        x[r] += W.bd + ad[r];
        xs[(row0 + r) * FGB_XLD + col] = x[r];
      }
    }
    __syncthreads();
  };
  for (int l = 0; l < L; l += 2) {
    body(l, wa);
    load(wa, l + 2);
    if (l + 1 < L) {
      body(l + 1, wb);
      load(wb, l + 3);
    }
  }
}

// ---------------------------------------------------------------- the tail
// out[m][n] = act(sum_k A[m][k] W[k][n] + bias[n]) for one 16 x 16 tile:
// the four waves take fixed K quarters, each lane group kk one sixteenth of
// K (a function of K only), and the quarters are summed in a fixed order.
struct FgbGemm {
  const float* A;
  long lda;
  int K;
  const float* W;
  long ldw;
  int N;
  const float* bias;
  int relu;
  float* out;
  long ldo;
};

__device__ __forceinline__ void fgb_gemm_tile(const FgbGemm& p, int nt, int mt,
                                              float (*red)[256]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ci = lane & 15, kk = lane >> 4;
  const int Kc = (p.K + 15) / 16;
  const int k0 = (w * 4 + kk) * Kc;
  const int jc = min(nt * 16 + ci, p.N - 1);   // (columns past N: not stored)
  const float* ap = p.A + (long)(mt * 16 + ci) * p.lda;
  const float* wp = p.W + jc;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int s = 0; s < Kc; ++s) {
    const int k = k0 + s;
    const int kc = min(k, p.K - 1);
    float a = ap[kc];
    const float bw = wp[(long)kc * p.ldw];
    if (k >= p.K) a = 0.f;
    acc = fgb_mfma(a, bw, acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[w][(kk * 4 + r) * 16 + ci] = acc[r];
  __syncthreads();
  const int row = tid >> 4, j = nt * 16 + (tid & 15);
  if (j < p.N) {
    float v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    if (p.bias) v += p.bias[j];
    if (p.relu) v = fmaxf(v, 0.f);
    p.out[(long)(mt * 16 + row) * p.ldo + j] = v;
  }
}

// pre[l][b][0:32 | 32:64] = x_l[t' - d_l] (Wf[0] | Wg[0]) + bias_fg[l][b] for
// the step t' = cursors[0] + ahead, group gi (rows past B: 0).  Wave w:
// rows 16 (w & 1), filter (w < 2) or gate half, two 16-column tiles.
// LC: the bias of stream b is row tpos of the conditioned-bias ring
// [R][L][nb][64] (wn_fastgen_lc_bias; nb = B with stream stride 64, 1 with 0).
template <bool LC>
__device__ __forceinline__ void fgb_pre_tile(const FgBatch& g, const FgbLc& lc, int l, int gi,
                                             int ahead) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int rb = w & 1, half = w >> 1;
  const int ci = lane & 15, kk = lane >> 4;
  int roff = 0;
  for (int i = 0; i < l; ++i) roff += g.dil[i];
  const int d = g.dil[l];
  const int tpos = g.cursors[0] + ahead;
  const float* xr = g.state + ((long)(roff + tpos % d) * g.Bp + gi * FGB_TILE + rb * 16 + ci) * 32;
  const float* wt = g.layer0 + (long)l * g.layer_stride + half * 2048;   // Wf[0] / Wg[0]
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int k = 4 * s + kk;
    const float a = xr[k];
    a0 = fgb_mfma(a, wt[k * 32 + ci], a0);
    a1 = fgb_mfma(a, wt[k * 32 + 16 + ci], a1);
  }
  const long lstride = g.bias_stride ? (long)g.B * 64 : 64;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = gi * FGB_TILE + rb * 16 + kk * 4 + r;
    float* out = g.pre + ((long)l * g.Bp + b) * 64 + half * 32;
    float v0 = 0.f, v1 = 0.f;
    if (b < g.B) {
      float c0 = 0.f, c1 = 0.f;
      if (LC) {
        const long rl = lc.stride ? (long)g.B * 64 : 64;
        const float* bb = lc.ring + ((long)(tpos % lc.R) * g.L + l) * rl + (long)b * lc.stride +
                          half * 32;
        c0 = bb[ci];
        c1 = bb[16 + ci];
      } else if (g.bias_fg) {
        const float* bb = g.bias_fg + l * lstride + (long)b * g.bias_stride + half * 32;
        c0 = bb[ci];
        c1 = bb[16 + ci];
      }
      v0 = c0 + a0[r];
      v1 = c1 + a1[r];
    }
    out[ci] = v0;
    out[16 + ci] = v1;
  }
}

__global__ __launch_bounds__(256) void fgb_pre_kernel(FgBatch g, int ahead) {
  const FgbLc none = {nullptr, 0, 0};
  fgb_pre_tile<false>(g, none, blockIdx.x / (g.Bp / FGB_TILE), blockIdx.x % (g.Bp / FGB_TILE),
                      ahead);
}

__global__ __launch_bounds__(256) void fgb_pre_lc_kernel(FgBatch g, FgbLc lc, int ahead) {
  fgb_pre_tile<true>(g, lc, blockIdx.x / (g.Bp / FGB_TILE), blockIdx.x % (g.Bp / FGB_TILE),
                     ahead);
}

__host__ __device__ __forceinline__ int fgb_ntiles(int n) { return (n + 15) / 16; }

// h1 = relu(z_all . Ws + bsum), then L x Bp/32 more workgroups: the next
// step's pre-activations
template <bool LC>
__device__ __forceinline__ void fgb_skip_body(const FgBatch& g, const FgbLc& lc) {
  __shared__ float red[4][256];
  const int nt = fgb_ntiles(g.S), nskip = nt * (g.Bp / 16);
  const int bid = blockIdx.x;
  if (bid >= nskip) {                       // workgroup-uniform
    const int r = bid - nskip, ng = g.Bp / FGB_TILE;
    fgb_pre_tile<LC>(g, lc, r / ng, r % ng, 1);
    return;
  }
  FgbGemm p = {g.z_all, (long)g.L * 32, g.L * 32, g.skip_w, g.S, g.S, g.skip_bsum, 1, g.h1, g.S};
  fgb_gemm_tile(p, bid % nt, bid / nt, red);
}

__global__ __launch_bounds__(256) void fgb_skip_kernel(FgBatch g) {
  const FgbLc none = {nullptr, 0, 0};
  fgb_skip_body<false>(g, none);
}

__global__ __launch_bounds__(256) void fgb_skip_lc_kernel(FgBatch g, FgbLc lc) {
  fgb_skip_body<true>(g, lc);
}

__global__ __launch_bounds__(256) void fgb_post1_kernel(FgBatch g) {
  __shared__ float red[4][256];
  const int nt = fgb_ntiles(g.S);
  FgbGemm p = {g.h1, g.S, g.S, g.post1_w, g.S, g.S, g.post1_b, 1, g.h2, g.S};
  fgb_gemm_tile(p, blockIdx.x % nt, blockIdx.x / nt, red);
}

__global__ __launch_bounds__(256) void fgb_logits_kernel(FgBatch g) {
  __shared__ float red[4][256];
  const int nt = fgb_ntiles(g.Q);
  FgbGemm p = {g.h2, g.S, g.S, g.post2_w, g.Q, g.Q, g.post2_b, 0, g.logits, g.Q};
  fgb_gemm_tile(p, blockIdx.x % nt, blockIdx.x / nt, red);
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // (no other workgroup reads them)
    g.cursors[0] += 1;
    g.cursors[1] = 1;                           // a draw is pending
  }
}

// ------------------------------------------------------------------- C ABI
int fgb_rows(int B) { return (B + FGB_TILE - 1) / FGB_TILE * FGB_TILE; }

int fgb_check_batch(int B) {
  if (B <= 0) return WN_ERR_BAD_SHAPE;
  if (B > FGB_MAXB) return WN_ERR_UNSUPPORTED;
  return WN_OK;
}

// null: no local conditioning; else the ring must be set and its shape sane
int fgb_check_lc(const FgbLc* lc) {
  if (!lc) return WN_OK;
  if (!lc->ring) return WN_ERR_NULL;
  if (lc->R < 1 || (lc->stride != 0 && lc->stride != 64)) return WN_ERR_BAD_SHAPE;
  return WN_OK;
}

void fgb_launch_chain_levels(const FgBatch& g, hipStream_t s) {
  hipLaunchKernelGGL(fgb_chain_kernel<true>, dim3(g.Bp / FGB_TILE), dim3(256), 0, s, g);
}

// skip sum + next pre-activations, post1, logits
void fgb_launch_tail(const FgBatch& g, const FgbLc* lc, FgbStage stage, hipStream_t s) {
  const int mt = g.Bp / 16, ng = g.Bp / FGB_TILE;
  if (stage == FGB_STAGE_SKIP) {
    if (lc)
      hipLaunchKernelGGL(fgb_skip_lc_kernel, dim3(fgb_ntiles(g.S) * mt + g.L * ng), dim3(256),
                         0, s, g, *lc);
    else
      hipLaunchKernelGGL(fgb_skip_kernel, dim3(fgb_ntiles(g.S) * mt + g.L * ng), dim3(256), 0,
                         s, g);
  } else if (stage == FGB_STAGE_POST1) {
    hipLaunchKernelGGL(fgb_post1_kernel, dim3(fgb_ntiles(g.S) * mt), dim3(256), 0, s, g);
  } else {
    hipLaunchKernelGGL(fgb_logits_kernel, dim3(fgb_ntiles(g.Q) * mt), dim3(256), 0, s, g);
  }
}

void fgb_launch_restart(float* state, const int32_t* dil, int L, int B,
                        const int32_t* cursors, int32_t* prev, int32_t* hist,
                        int32_t* origin, const int32_t* flags, hipStream_t s) {
  const int Bp = fgb_rows(B);
  hipLaunchKernelGGL(fgb_restart_kernel, dim3(128, Bp / FGB_TILE), dim3(256), 0, s, state, dil,
                     L, B, Bp, cursors, prev, hist, origin, flags);
}

extern "C" {

int wn_fastgen_batch_rows(int B) {
  const int rc = fgb_check_batch(B);
  return rc != WN_OK ? rc : fgb_rows(B);
}

long wn_fastgen_batch_state_floats(const int32_t* dilations_host, int L, int B) {
  if (!dilations_host) return WN_ERR_NULL;
  if (L <= 0) return WN_ERR_BAD_SHAPE;
  if (L > FGB_MAXL) return WN_ERR_UNSUPPORTED;
  const int rc = fgb_check_batch(B);
  if (rc != WN_OK) return rc;
  long n = 0;
  for (int l = 0; l < L; ++l) {
    if (dilations_host[l] <= 0) return WN_ERR_BAD_SHAPE;
    n += dilations_host[l];
  }
  return n * fgb_rows(B) * 32;
}

int wn_fastgen_batch_init(float* state, long state_floats, int32_t* cursors, int32_t* prev,
                          int B, void* stream) {
  if (!state || !cursors || !prev) return WN_ERR_NULL;
  const int rc = fgb_check_batch(B);
  if (rc != WN_OK) return rc;
  if (state_floats <= 0) return WN_ERR_BAD_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(state, 0, state_floats * sizeof(float), s) != hipSuccess ||
      hipMemsetD32Async((hipDeviceptr_t)cursors, 0, 4, s) != hipSuccess ||
      hipMemsetD32Async((hipDeviceptr_t)prev, -1, fgb_rows(B), s) != hipSuccess)
    return WN_ERR_LAUNCH;
  return WN_OK;
}

}  // extern "C"

int fgb_pre(const FgbLc* lc, const float* layer0, long layer_stride,
                   const float* gc_bias_fg, int bias_stream_stride,
                   const int32_t* dilations_dev, int L, int B, const float* state,
                   const int32_t* cursors, float* pre, void* stream) {
  if (!layer0 || !dilations_dev || !state || !cursors || !pre) return WN_ERR_NULL;
  const int lrc = fgb_check_lc(lc);
  if (lrc != WN_OK) return lrc;
  if (L <= 0 || (bias_stream_stride != 0 && bias_stream_stride != 64)) return WN_ERR_BAD_SHAPE;
  if (L > FGB_MAXL) return WN_ERR_UNSUPPORTED;
  const int rc = fgb_check_batch(B);
  if (rc != WN_OK) return rc;
  FgBatch g = {};
  g.layer0 = layer0; g.layer_stride = layer_stride; g.bias_fg = gc_bias_fg;
  g.bias_stride = bias_stream_stride; g.dil = dilations_dev; g.L = L; g.B = B;
  g.Bp = fgb_rows(B); g.state = const_cast<float*>(state);
  g.cursors = const_cast<int32_t*>(cursors); g.pre = pre;
  if (lc)
    hipLaunchKernelGGL(fgb_pre_lc_kernel, dim3(L * (g.Bp / FGB_TILE)), dim3(256), 0,
                       (hipStream_t)stream, g, *lc, 0);
  else
    hipLaunchKernelGGL(fgb_pre_kernel, dim3(L * (g.Bp / FGB_TILE)), dim3(256), 0,
                       (hipStream_t)stream, g, 0);
  return wn_check_launch();
}

extern "C" {

int wn_fastgen_batch_pre(const float* layer0, long layer_stride, const float* gc_bias_fg,
                         int bias_stream_stride, const int32_t* dilations_dev, int L, int B,
                         const float* state, const int32_t* cursors, float* pre,
                         void* stream) {
  return fgb_pre(nullptr, layer0, layer_stride, gc_bias_fg, bias_stream_stride, dilations_dev,
                 L, B, state, cursors, pre, stream);
}

int wn_fastgen_batch_pre_lc(const float* layer0, long layer_stride, const float* gc_bias_fg,
                            int bias_stream_stride, const int32_t* dilations_dev, int L, int B,
                            const float* state, const int32_t* cursors, float* pre,
                            const float* lc_ring, int lc_R, int lc_stride, void* stream) {
  const FgbLc lc = {lc_ring, lc_R, lc_stride};
  return fgb_pre(&lc, layer0, layer_stride, gc_bias_fg, bias_stream_stride, dilations_dev, L, B,
                 state, cursors, pre, stream);
}

// Enqueue the stages [first, last) of one step: 0 draw, 1 chain, 2 skip sum +
// next pre-activations, 3 post1, 4 logits (wn_fastgen_batch_step: all five;
// single stages let a caller time each launch between its own events).
static int fgb_stages(const FgbLc* lc, const int32_t* origins, int first, int last,
                      const float* params_causal,
                            const float* layer0, long layer_stride, const float* skip_w,
                            const float* skip_bsum, const float* post1_w,
                            const float* post1_b, const float* post2_w, const float* post2_b,
                            const float* gc_bias_fg, int bias_stream_stride,
                            const int32_t* dilations_dev, int L, int S, int Q, int B,
                            float* state, int32_t* cursors, int32_t* prev,
                            int32_t* samples_io, const int32_t* ctl, const uint64_t* seeds,
                            float* proba_out, int use_biases, float* pre, float* z_all,
                            float* h1, float* h2, float* logits, void* stream) {
  if (!params_causal || !layer0 || !skip_w || !post1_w || !post2_w || !dilations_dev ||
      !state || !cursors || !prev || !samples_io || !ctl || !seeds || !pre || !z_all ||
      !h1 || !h2 || !logits)
    return WN_ERR_NULL;
  if (L <= 0 || S <= 0 || Q <= 0 || (bias_stream_stride != 0 && bias_stream_stride != 64) ||
      first < 0 || last > 5 || first >= last)
    return WN_ERR_BAD_SHAPE;
  const int lrc = fgb_check_lc(lc);
  if (lrc != WN_OK) return lrc;
  if (S > FGB_MAXS || Q > FGB_MAXQ || L > FGB_MAXL) return WN_ERR_UNSUPPORTED;
  const int rc = fgb_check_batch(B);
  if (rc != WN_OK) return rc;
  FgBatch g = {};
  g.causal = params_causal; g.layer0 = layer0; g.layer_stride = layer_stride;
  g.skip_w = skip_w; g.skip_bsum = skip_bsum; g.post1_w = post1_w; g.post1_b = post1_b;
  g.post2_w = post2_w; g.post2_b = post2_b; g.bias_fg = gc_bias_fg;
  g.bias_stride = bias_stream_stride; g.dil = dilations_dev;
  g.L = L; g.S = S; g.Q = Q; g.B = B; g.Bp = fgb_rows(B);
  g.state = state; g.cursors = cursors; g.prev = prev; g.samples = samples_io;
  g.ctl = ctl; g.seeds = seeds; g.proba_out = proba_out; g.use_dense_bias = use_biases;
  g.pre = pre; g.z_all = z_all; g.h1 = h1; g.h2 = h2; g.logits = logits;
  g.origin = origins;
  hipStream_t s = (hipStream_t)stream;
  const int ng = g.Bp / FGB_TILE;
  for (int stage = first; stage < last; ++stage) {
    switch (stage) {
      case 0:
        if (origins)
          hipLaunchKernelGGL(fgb_draw_q_kernel, dim3((B + 3) / 4), dim3(256), 0, s, g);
        else
          hipLaunchKernelGGL(fgb_draw_kernel, dim3((B + 3) / 4), dim3(256), 0, s, g);
        break;
      case 1:
        hipLaunchKernelGGL(fgb_chain_kernel<false>, dim3(ng), dim3(256), 0, s, g);
        break;
      default:
        fgb_launch_tail(g, lc, (FgbStage)stage, s);
        break;
    }
  }
  return wn_check_launch();
}

int wn_fastgen_batch_stages(int first, int last, const float* params_causal,
                            const float* layer0, long layer_stride, const float* skip_w,
                            const float* skip_bsum, const float* post1_w,
                            const float* post1_b, const float* post2_w, const float* post2_b,
                            const float* gc_bias_fg, int bias_stream_stride,
                            const int32_t* dilations_dev, int L, int S, int Q, int B,
                            float* state, int32_t* cursors, int32_t* prev,
                            int32_t* samples_io, const int32_t* ctl, const uint64_t* seeds,
                            float* proba_out, int use_biases, float* pre, float* z_all,
                            float* h1, float* h2, float* logits, void* stream) {
  return fgb_stages(nullptr, nullptr, first, last, params_causal, layer0, layer_stride, skip_w, skip_bsum,
                    post1_w, post1_b, post2_w, post2_b, gc_bias_fg, bias_stream_stride,
                    dilations_dev, L, S, Q, B, state, cursors, prev, samples_io, ctl, seeds,
                    proba_out, use_biases, pre, z_all, h1, h2, logits, stream);
}

int wn_fastgen_batch_step_lc(const float* params_causal, const float* layer0, long layer_stride,
                             const float* skip_w, const float* skip_bsum, const float* post1_w,
                             const float* post1_b, const float* post2_w, const float* post2_b,
                             const float* gc_bias_fg, int bias_stream_stride,
                             const int32_t* dilations_dev, int L, int S, int Q, int B,
                             float* state, int32_t* cursors, int32_t* prev, int32_t* samples_io,
                             const int32_t* ctl, const uint64_t* seeds, float* proba_out,
                             int use_biases, float* pre, float* z_all, float* h1, float* h2,
                             float* logits, const float* lc_ring, int lc_R, int lc_stride,
                             void* stream) {
  const FgbLc lc = {lc_ring, lc_R, lc_stride};
  return fgb_stages(&lc, nullptr, 0, 5, params_causal, layer0, layer_stride, skip_w, skip_bsum, post1_w,
                    post1_b, post2_w, post2_b, gc_bias_fg, bias_stream_stride, dilations_dev, L,
                    S, Q, B, state, cursors, prev, samples_io, ctl, seeds, proba_out, use_biases,
                    pre, z_all, h1, h2, logits, stream);
}

int wn_fastgen_batch_step(const float* params_causal, const float* layer0, long layer_stride,
                          const float* skip_w, const float* skip_bsum, const float* post1_w,
                          const float* post1_b, const float* post2_w, const float* post2_b,
                          const float* gc_bias_fg, int bias_stream_stride,
                          const int32_t* dilations_dev, int L, int S, int Q, int B,
                          float* state, int32_t* cursors, int32_t* prev, int32_t* samples_io,
                          const int32_t* ctl, const uint64_t* seeds, float* proba_out,
                          int use_biases, float* pre, float* z_all, float* h1, float* h2,
                          float* logits, void* stream) {
  return fgb_stages(nullptr, nullptr, 0, 5, params_causal, layer0, layer_stride, skip_w, skip_bsum,
                                 post1_w, post1_b, post2_w, post2_b, gc_bias_fg,
                                 bias_stream_stride, dilations_dev, L, S, Q, B, state, cursors,
                                 prev, samples_io, ctl, seeds, proba_out, use_biases, pre, z_all,
                                 h1, h2, logits, stream);
}

static int fgb_finish(const int32_t* origins, int Q, int B, int32_t* cursors,
                      int32_t* samples_io, const int32_t* ctl, const uint64_t* seeds,
                      float* proba_out, const float* logits, void* stream) {
  if (!cursors || !samples_io || !ctl || !seeds || !logits) return WN_ERR_NULL;
  if (Q <= 0) return WN_ERR_BAD_SHAPE;
  if (Q > FGB_MAXQ) return WN_ERR_UNSUPPORTED;
  const int rc = fgb_check_batch(B);
  if (rc != WN_OK) return rc;
  FgBatch g = {};
  g.Q = Q; g.B = B; g.Bp = fgb_rows(B); g.cursors = cursors; g.samples = samples_io;
  g.ctl = ctl; g.seeds = seeds; g.proba_out = proba_out; g.logits = const_cast<float*>(logits);
  g.origin = origins;
  hipStream_t s = (hipStream_t)stream;
  if (origins)
    hipLaunchKernelGGL(fgb_draw_q_kernel, dim3((B + 3) / 4), dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL(fgb_draw_kernel, dim3((B + 3) / 4), dim3(256), 0, s, g);
  if (wn_check_launch() != WN_OK) return WN_ERR_LAUNCH;
  if (hipMemsetD32Async((hipDeviceptr_t)(cursors + 1), 0, 1, s) != hipSuccess)
    return WN_ERR_LAUNCH;
  return WN_OK;
}

int wn_fastgen_batch_finish(int Q, int B, int32_t* cursors, int32_t* samples_io,
                            const int32_t* ctl, const uint64_t* seeds, float* proba_out,
                            const float* logits, void* stream) {
  return fgb_finish(nullptr, Q, B, cursors, samples_io, ctl, seeds, proba_out, logits, stream);
}

// ---- the _q entries: the same launches with the draw counted from each
// stream's own origin (streams restarted by wn_fastgen_batch_restart)
int wn_fastgen_batch_step_q(const float* params_causal, const float* layer0, long layer_stride,
                            const float* skip_w, const float* skip_bsum, const float* post1_w,
                            const float* post1_b, const float* post2_w, const float* post2_b,
                            const float* gc_bias_fg, int bias_stream_stride,
                            const int32_t* dilations_dev, int L, int S, int Q, int B,
                            float* state, int32_t* cursors, int32_t* prev, int32_t* samples_io,
                            const int32_t* ctl, const uint64_t* seeds, float* proba_out,
                            int use_biases, float* pre, float* z_all, float* h1, float* h2,
                            float* logits, const int32_t* origins, void* stream) {
  if (!origins) return WN_ERR_NULL;
  return fgb_stages(nullptr, origins, 0, 5, params_causal, layer0, layer_stride, skip_w,
                    skip_bsum, post1_w, post1_b, post2_w, post2_b, gc_bias_fg,
                    bias_stream_stride, dilations_dev, L, S, Q, B, state, cursors, prev,
                    samples_io, ctl, seeds, proba_out, use_biases, pre, z_all, h1, h2, logits,
                    stream);
}

int wn_fastgen_batch_step_lc_q(const float* params_causal, const float* layer0,
                               long layer_stride, const float* skip_w, const float* skip_bsum,
                               const float* post1_w, const float* post1_b, const float* post2_w,
                               const float* post2_b, const float* gc_bias_fg,
                               int bias_stream_stride, const int32_t* dilations_dev, int L,
                               int S, int Q, int B, float* state, int32_t* cursors,
                               int32_t* prev, int32_t* samples_io, const int32_t* ctl,
                               const uint64_t* seeds, float* proba_out, int use_biases,
                               float* pre, float* z_all, float* h1, float* h2, float* logits,
                               const float* lc_ring, int lc_R, int lc_stride,
                               const int32_t* origins, void* stream) {
  if (!origins) return WN_ERR_NULL;
  const FgbLc lc = {lc_ring, lc_R, lc_stride};
  return fgb_stages(&lc, origins, 0, 5, params_causal, layer0, layer_stride, skip_w, skip_bsum,
                    post1_w, post1_b, post2_w, post2_b, gc_bias_fg, bias_stream_stride,
                    dilations_dev, L, S, Q, B, state, cursors, prev, samples_io, ctl, seeds,
                    proba_out, use_biases, pre, z_all, h1, h2, logits, stream);
}

int wn_fastgen_batch_finish_q(int Q, int B, int32_t* cursors, int32_t* samples_io,
                              const int32_t* ctl, const uint64_t* seeds, float* proba_out,
                              const float* logits, const int32_t* origins, void* stream) {
  if (!origins) return WN_ERR_NULL;
  return fgb_finish(origins, Q, B, cursors, samples_io, ctl, seeds, proba_out, logits, stream);
}

int wn_fastgen_batch_restart(float* state, const int32_t* dilations_dev, int L, int B,
                             const int32_t* cursors, int32_t* prev, int32_t* origins,
                             const int32_t* flags, void* stream) {
  if (!state || !dilations_dev || !cursors || !prev || !origins || !flags) return WN_ERR_NULL;
  if (L <= 0) return WN_ERR_BAD_SHAPE;
  if (L > FGB_MAXL) return WN_ERR_UNSUPPORTED;
  const int rc = fgb_check_batch(B);
  if (rc != WN_OK) return rc;
  fgb_launch_restart(state, dilations_dev, L, B, cursors, prev, nullptr, origins, flags,
                     (hipStream_t)stream);
  return wn_check_launch();
}

int wn_fastgen_batch_lc_rows(const int64_t* table, int B, int n, int Lc, long pos0, float* out,
                             void* stream) {
  if (!table || !out) return WN_ERR_NULL;
  if (n <= 0 || Lc <= 0 || pos0 < 0) return WN_ERR_BAD_SHAPE;
  const int rc = fgb_check_batch(B);
  if (rc != WN_OK) return rc;
  const long total = (long)B * n * Lc;
  const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(fgb_lc_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(table), B, n, Lc, pos0, out);
  return wn_check_launch();
}

}  // extern "C"
