// The batched generator's argument block and the launches that do not care
// what the first and last layers are (wn_fastgen_batch.hip), for the file
// that puts other ends on them (wn_fastgen_mol.hip: levels in, a mixture
// draw out).
#pragma once
#include "wn_common.h"

#define FGB_MAXB 256
#define FGB_TILE 32      // streams per chain workgroup
#define FGB_MAXL 64
#define FGB_MAXS 512
#define FGB_MAXQ 512
#define FGB_XLD 33       // LDS row stride of the chain's x / z tiles
#define FGB_HIST 64      // slots of a stream's level history (levels input)
#define FGB_MAXK0 32     // taps of the causal layer on levels, at most

// ctl: int32[8] per call (device memory, so that a captured graph serves
// every call): base (cursors[0] when the call started), n_given, proba_every,
// temperature (float bits), row stride of samples_io, rows per stream of
// proba_out, top-k and top-p (float bits) of the draw (0: off)
#define FGB_CTL_BASE 0
#define FGB_CTL_NGIVEN 1
#define FGB_CTL_PEVERY 2
#define FGB_CTL_TEMP 3
#define FGB_CTL_LDS 4
#define FGB_CTL_LDP 5
#define FGB_CTL_TOPK 6
#define FGB_CTL_TOPP 7

struct FgBatch {
  const float* causal;     // [2][Q][32]; levels input: [K0][32]
  const float* layer0;     // layer blocks
  long layer_stride;
  const float* skip_w;     // [L * 32][S]
  const float* skip_bsum;  // [S] or null
  const float* post1_w;    // [S][S]
  const float* post1_b;    // [S] or null
  const float* post2_w;    // [S][Q]
  const float* post2_b;    // [Q] or null
  const float* bias_fg;    // [L][nb][64] or null; nb = B (stride 64) or 1 (stride 0)
  int bias_stride;
  const int32_t* dil;
  int L, S, Q, B, Bp;
  float* state;            // [sum(d)][Bp][32]
  int32_t* cursors;        // [0] steps pushed, [1] draw pending
  int32_t* prev;           // [Bp] code consumed one step back (-1: none)
  int32_t* samples;        // [B][ctl[LDS]], indexed by cursors[0] - ctl[BASE]
  const int32_t* ctl;
  const uint64_t* seeds;   // [B]
  float* proba_out;        // [B][ctl[LDP]][Q] or null (mixture: [..][3][K])
  int use_dense_bias;
  float* pre;              // [L][Bp][64]
  float* z_all;            // [Bp][L * 32]
  float* h1;               // [Bp][S]
  float* h2;               // [Bp][S]
  float* logits;           // [Bp][Q]
  const int32_t* origin;   // [Bp] step at which stream b (re)started, or null (all 0)
  // levels input (the mixture head): slot T & 63 of a stream's row holds the
  // level consumed at step T (-1: none); K0 taps; K components, beta's floor
  int32_t* hist;           // [Bp][FGB_HIST]
  int K0, K;
  float lsm;
};

// the conditioned-bias ring [R][L][nb][64] (wn_fastgen_lc_bias; nb = B with
// stream stride 64, 1 with 0)
struct FgbLc {
  const float* ring;
  int R, stride;
};

// (internal to the library: not part of the C ABI of include/)
#pragma GCC visibility push(hidden)
enum FgbStage { FGB_STAGE_SKIP = 2, FGB_STAGE_POST1 = 3, FGB_STAGE_LOGITS = 4 };

int fgb_rows(int B);
int fgb_check_batch(int B);
// null: no local conditioning; else the ring must be set and its shape sane
int fgb_check_lc(const FgbLc* lc);
int fgb_pre(const FgbLc* lc, const float* layer0, long layer_stride,
            const float* gc_bias_fg, int bias_stream_stride,
            const int32_t* dilations_dev, int L, int B, const float* state,
            const int32_t* cursors, float* pre, void* stream);
// the chain on levels (g.hist, g.K0), and the stages behind it as they are
void fgb_launch_chain_levels(const FgBatch& g, hipStream_t s);
void fgb_launch_tail(const FgBatch& g, const FgbLc* lc, FgbStage stage, hipStream_t s);
// flagged streams: ring columns zeroed, origin = cursors[0], prev = -1 (when
// given), history slots = -1 (when given)
void fgb_launch_restart(float* state, const int32_t* dil, int L, int B,
                        const int32_t* cursors, int32_t* prev, int32_t* hist,
                        int32_t* origin, const int32_t* flags, hipStream_t s);
#pragma GCC visibility pop
