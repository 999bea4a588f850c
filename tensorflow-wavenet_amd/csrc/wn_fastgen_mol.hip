// Batched fast generation for mixture-of-logistics models
// (include/wavenet_fastgen_mol.h, WaveNetModel.generate_mixture_batch): the
// batched generator of wn_fastgen_batch.hip with its two ends replaced.  One
// step, five launches:
//   fgm_draw_kernel          : the PREVIOUS step's parameters (log-softmax in
//                              float64, mu, clamped beta) and its draw, one
//                              wave per stream (when one is pending)
//   fgb_chain_kernel<levels> : the causal layer over the stream's history of
//                              levels, then the L layers
//   fgb_skip / post1 / logits: as they are, with Q = 3 Kp columns
// The parameters and the draw are the bodies of wn_mol_params_row and
// wn_mol_sample (wn_mol_draw.h): one statement of each rule.
#include "wn_fastgen_batch.h"
#include "wn_mol_draw.h"

// Stream b's pending row: lane k < K computes component k's parameters into
// the wave's LDS row pr [3][K]; every proba_every-th step the row goes to
// params_out; lane 0 draws.  counter = the step that produced the logits,
// counted from the stream's origin where there is one.
__global__ __launch_bounds__(256) void fgm_draw_kernel(FgBatch g) {
  __shared__ float prs[4][3 * MOL_MAXK];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + w;
  if (!g.cursors[1] || b >= g.B) return;
  const int K = g.K, step = g.cursors[0] - 1;
  float* pr = prs[w];
  const int local = step - g.ctl[FGB_CTL_BASE];
  const int every = g.ctl[FGB_CTL_PEVERY] > 0 ? g.ctl[FGB_CTL_PEVERY] : 1;
  if (lane < K) mol_params_component(g.logits + (long)b * g.Q, K, g.lsm, lane, pr);
  __builtin_amdgcn_wave_barrier();
  if (g.proba_out && local % every == 0) {
    float* out = g.proba_out + ((long)b * g.ctl[FGB_CTL_LDP] + local / every) * 3 * K;
    for (int i = lane; i < 3 * K; i += 64) out[i] = pr[i];
  }
  if (local + 1 < g.ctl[FGB_CTL_NGIVEN]) return;   // still inside the given samples
  if (lane == 0) {
    const uint64_t ctr = g.origin ? (uint64_t)(step - g.origin[b]) : (uint64_t)step;
    g.samples[(long)b * g.ctl[FGB_CTL_LDS] + local + 1] =
        mol_draw_level(pr, K, g.seeds[b], ctr, __int_as_float(g.ctl[FGB_CTL_TEMP]));
  }
}

static inline bool fgm_al(const void* p, unsigned a) {
  return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0;
}

static int fgm_check_head(int K, float lsm) {
  if (K < 1 || K > MOL_MAXK || !(lsm >= -32.f && lsm <= -1.f)) return WN_ERR_BAD_SHAPE;
  return WN_OK;
}

extern "C" {

int wn_fastgen_mol_init(float* state, long state_floats, int32_t* cursors, int32_t* hist,
                        int B, void* stream) {
  if (!state || !cursors || !hist) return WN_ERR_NULL;
  const int rc = fgb_check_batch(B);
  if (rc != WN_OK) return rc;
  if (state_floats <= 0) return WN_ERR_BAD_SHAPE;
  if (!wn_aligned16(state) || !fgm_al(cursors, 4) || !fgm_al(hist, 4)) return WN_ERR_MISALIGNED;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(state, 0, state_floats * sizeof(float), s) != hipSuccess ||
      hipMemsetD32Async((hipDeviceptr_t)cursors, 0, 4, s) != hipSuccess ||
      hipMemsetD32Async((hipDeviceptr_t)hist, -1, (size_t)fgb_rows(B) * FGB_HIST, s) !=
          hipSuccess)
    return WN_ERR_LAUNCH;
  return WN_OK;
}

int wn_fastgen_mol_pre(const float* layer0, long layer_stride, const float* gc_bias_fg,
                       int bias_stream_stride, const int32_t* dilations_dev, int L, int B,
                       const float* state, const int32_t* cursors, float* pre,
                       const float* lc_ring, int lc_R, int lc_stride, void* stream) {
  if (!fgm_al(layer0, 4) || !fgm_al(gc_bias_fg, 4) || !fgm_al(dilations_dev, 4) ||
      !fgm_al(state, 4) || !fgm_al(cursors, 4) || !fgm_al(pre, 4) || !fgm_al(lc_ring, 4))
    return WN_ERR_MISALIGNED;
  const FgbLc lc = {lc_ring, lc_R, lc_stride};
  return fgb_pre(lc_ring ? &lc : nullptr, layer0, layer_stride, gc_bias_fg, bias_stream_stride,
                 dilations_dev, L, B, state, cursors, pre, stream);
}

int wn_fastgen_mol_step(const float* params_causal, int K0, const float* layer0,
                        long layer_stride, const float* skip_w, const float* skip_bsum,
                        const float* post1_w, const float* post1_b, const float* post2_w,
                        const float* post2_b, const float* gc_bias_fg, int bias_stream_stride,
                        const int32_t* dilations_dev, int L, int S, int K, int B, float* state,
                        int32_t* cursors, int32_t* hist, int32_t* samples_io,
                        const int32_t* ctl, const uint64_t* seeds, float* params_out,
                        int use_biases, float log_scale_min, float* pre, float* z_all,
                        float* h1, float* h2, float* logits, const float* lc_ring, int lc_R,
                        int lc_stride, const int32_t* origins, void* stream) {
  if (!params_causal || !layer0 || !skip_w || !post1_w || !post2_w || !dilations_dev ||
      !state || !cursors || !hist || !samples_io || !ctl || !seeds || !pre || !z_all || !h1 ||
      !h2 || !logits)
    return WN_ERR_NULL;
  if (L <= 0 || S <= 0 || (bias_stream_stride != 0 && bias_stream_stride != 64))
    return WN_ERR_BAD_SHAPE;
  if (K0 < 1 || K0 > FGB_MAXK0) return WN_ERR_BAD_SHAPE;
  int rc = fgm_check_head(K, log_scale_min);
  if (rc != WN_OK) return rc;
  const FgbLc lcv = {lc_ring, lc_R, lc_stride};
  const FgbLc* lc = lc_ring ? &lcv : nullptr;
  rc = fgb_check_lc(lc);
  if (rc != WN_OK) return rc;
  if (S > FGB_MAXS || L > FGB_MAXL) return WN_ERR_UNSUPPORTED;
  rc = fgb_check_batch(B);
  if (rc != WN_OK) return rc;
  const void* words[] = {params_causal, layer0, skip_w, skip_bsum, post1_w, post1_b, post2_w,
                         post2_b, gc_bias_fg, dilations_dev, state, cursors, hist, samples_io,
                         ctl, params_out, pre, z_all, h1, h2, logits, lc_ring, origins};
  for (const void* p : words)
    if (!fgm_al(p, 4)) return WN_ERR_MISALIGNED;
  if (!fgm_al(seeds, 8)) return WN_ERR_MISALIGNED;
  FgBatch g = {};
  g.causal = params_causal; g.layer0 = layer0; g.layer_stride = layer_stride;
  g.skip_w = skip_w; g.skip_bsum = skip_bsum; g.post1_w = post1_w; g.post1_b = post1_b;
  g.post2_w = post2_w; g.post2_b = post2_b; g.bias_fg = gc_bias_fg;
  g.bias_stride = bias_stream_stride; g.dil = dilations_dev;
  g.L = L; g.S = S; g.Q = 3 * ((K + 3) & ~3); g.B = B; g.Bp = fgb_rows(B);
  g.state = state; g.cursors = cursors; g.samples = samples_io;
  g.ctl = ctl; g.seeds = seeds; g.proba_out = params_out; g.use_dense_bias = use_biases;
  g.pre = pre; g.z_all = z_all; g.h1 = h1; g.h2 = h2; g.logits = logits;
  g.origin = origins; g.hist = hist; g.K0 = K0; g.K = K; g.lsm = log_scale_min;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fgm_draw_kernel, dim3((B + 3) / 4), dim3(256), 0, s, g);
  fgb_launch_chain_levels(g, s);
  fgb_launch_tail(g, lc, FGB_STAGE_SKIP, s);
  fgb_launch_tail(g, lc, FGB_STAGE_POST1, s);
  fgb_launch_tail(g, lc, FGB_STAGE_LOGITS, s);
  return wn_check_launch();
}

int wn_fastgen_mol_finish(int K, float log_scale_min, int B, int32_t* cursors,
                          int32_t* samples_io, const int32_t* ctl, const uint64_t* seeds,
                          float* params_out, const float* logits, const int32_t* origins,
                          void* stream) {
  if (!cursors || !samples_io || !ctl || !seeds || !logits) return WN_ERR_NULL;
  int rc = fgm_check_head(K, log_scale_min);
  if (rc != WN_OK) return rc;
  rc = fgb_check_batch(B);
  if (rc != WN_OK) return rc;
  if (!fgm_al(cursors, 4) || !fgm_al(samples_io, 4) || !fgm_al(ctl, 4) || !fgm_al(seeds, 8) ||
      !fgm_al(params_out, 4) || !fgm_al(logits, 4) || !fgm_al(origins, 4))
    return WN_ERR_MISALIGNED;
  FgBatch g = {};
  g.Q = 3 * ((K + 3) & ~3); g.B = B; g.Bp = fgb_rows(B); g.cursors = cursors;
  g.samples = samples_io; g.ctl = ctl; g.seeds = seeds; g.proba_out = params_out;
  g.logits = const_cast<float*>(logits); g.origin = origins; g.K = K; g.lsm = log_scale_min;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fgm_draw_kernel, dim3((B + 3) / 4), dim3(256), 0, s, g);
  if (wn_check_launch() != WN_OK) return WN_ERR_LAUNCH;
  if (hipMemsetD32Async((hipDeviceptr_t)(cursors + 1), 0, 1, s) != hipSuccess)
    return WN_ERR_LAUNCH;
  return WN_OK;
}

int wn_fastgen_mol_restart(float* state, const int32_t* dilations_dev, int L, int B,
                           const int32_t* cursors, int32_t* hist, int32_t* origins,
                           const int32_t* flags, void* stream) {
  if (!state || !dilations_dev || !cursors || !hist || !origins || !flags) return WN_ERR_NULL;
  if (L <= 0) return WN_ERR_BAD_SHAPE;
  if (L > FGB_MAXL) return WN_ERR_UNSUPPORTED;
  const int rc = fgb_check_batch(B);
  if (rc != WN_OK) return rc;
  if (!wn_aligned16(state) || !fgm_al(dilations_dev, 4) || !fgm_al(cursors, 4) ||
      !fgm_al(hist, 4) || !fgm_al(origins, 4) || !fgm_al(flags, 4))
    return WN_ERR_MISALIGNED;
  fgb_launch_restart(state, dilations_dev, L, B, cursors, nullptr, hist, origins, flags,
                     (hipStream_t)stream);
  return wn_check_launch();
}

}  // extern "C"
