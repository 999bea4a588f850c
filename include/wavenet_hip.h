/* wavenet_hip.h -- C ABI of libwavenet_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary of the reference (jyegerlehner/tensorflow-wavenet) is
 * its Python class API (wavenet/__init__.py:1-4); it has no FFI of its own.
 * This C ABI is the new, internal boundary under the Python host
 * (tensorflow-wavenet_amd/wavenet): each entry point names the reference
 * code it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Contract (all entry points)
 *   - plain C: raw device pointers + explicit sizes, no torch / C++ types;
 *   - every buffer is allocated and owned by the caller; the library never
 *     allocates, frees or retains a pointer past return;
 *   - asynchronous on the caller's `stream` (a hipStream_t passed as void*),
 *     no internal synchronisation, no mutable globals: re-entrant, safe for
 *     one process per GPU and for several streams;
 *   - returns WN_OK (0) or a negative WN_ERR_* code; no C++ exception
 *     crosses the boundary;
 *   - activation "planes" are [rows][32] fp32 with rows = B*T (reference
 *     layout [B,T,C], channels innermost, residual/dilation channels zero-
 *     padded to 32); weights keep the reference's [K][Cin][Cout] order.
 *   - device pointers and leading dimensions must be 16-byte aligned.
 */
#ifndef WAVENET_HIP_H_
#define WAVENET_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WN_OK 0
#define WN_ERR_BAD_SHAPE (-1)
#define WN_ERR_UNSUPPORTED (-2)
#define WN_ERR_MISALIGNED (-3)
#define WN_ERR_LAUNCH (-4)
#define WN_ERR_NULL (-5)

int wn_version(void);
const char* wn_error_string(int code);

/* ---- mu-law companding: wavenet/ops.py:65-73 (encode), :76-85 (decode) ---
 * Host: build the Q-1 float32 decision thresholds / the Q-entry decode table
 * of the float32 chain (host memory).  Device: bit-exact encode by threshold
 * search, decode by table lookup. */
int wn_mu_law_thresholds_host(int Q, float* thr_out);
int wn_mu_law_decode_table_host(int Q, float* lut_out);
int wn_mu_law_encode(const float* audio, int32_t* codes, long n,
                     const float* thr_dev, int Q, void* stream);
int wn_mu_law_decode(const int32_t* codes, float* audio, long n,
                     const float* lut_dev, int Q, void* stream);

/* ---- input noise (csrc/wn_misc.hip; wavenet/input_noise.py): perturbed
 * copies of the codes for the network to read while the loss keeps the clean
 * codes as targets.  codes / codes_in: int32 [B][T]; keys: device int64 [B],
 * clip b's key k[b], 0 <= k[b] < 2^40; lengths: device int32 [B] (clamped to
 * [0, T] by the kernel) or NULL (n[b] = T).  keys and lengths are read when
 * the kernel runs.  With w = width, for position t < 2^24 of clip b:
 *
 *   c    = (k[b] << 24) | t
 *   bits = draw_bits(seed ^ 0x6e6f697365, c)
 *        = splitmix64((seed ^ 0x6e6f697365) ^ splitmix64(c))
 *   hit  = (bits & 0xFFFFFF) < thresh
 *   d    = ((bits >> 24) & 0xFFFFF) % (w + 1) - ((bits >> 44) & 0xFFFFF) % (w + 1)
 *   codes_in[b][t] = clamp(codes[b][t] + d, 0, Q - 1)
 *                        where hit, t < n[b] and 0 <= codes[b][t] < Q,
 *                    codes[b][t] otherwise (padding, out-of-range codes,
 *                        thresh == 0)
 *
 * (d is triangular on [-w, w]; thresh = int(prob * 2^24), 2^24 hits every
 * position.)  Integer arithmetic only: a pure function of (seed, k[b], t) and
 * the code, not of B, T, the clip's place in the batch or the launch.
 *
 * wn_code_noise applies the rule to given codes (codes_in may be codes
 * itself).  wn_mu_law_encode_noisy makes one pass over the audio [B][T] and
 * writes the clean codes -- the bits of wn_mu_law_encode, by the same
 * threshold search (thr_dev: its Q - 1 thresholds) -- and the perturbed ones
 * (codes_in == codes: WN_ERR_UNSUPPORTED).
 *
 * One grid row per clip, four consecutive positions per thread, moved with
 * 16-byte accesses where the clip's rows of every array start 16-byte aligned
 * (with T % 4 != 0 only clip 0's do) and one by one otherwise; no LDS, no
 * atomics.  NULL (but lengths): WN_ERR_NULL; B, T <= 0, T > 2^24, Q < 2,
 * width < 1 or > 4095, thresh < 0 or > 2^24: WN_ERR_BAD_SHAPE; keys not
 * 8-byte, any other pointer not 4-byte aligned: WN_ERR_MISALIGNED.  All checks
 * come before any launch. */
int wn_code_noise(const int32_t* codes, int32_t* codes_in, const int64_t* keys,
                  const int32_t* lengths, int B, int T, int Q, uint64_t seed,
                  int thresh, int width, void* stream);
int wn_mu_law_encode_noisy(const float* audio, int32_t* codes,
                           int32_t* codes_in, const int64_t* keys,
                           const int32_t* lengths, int B, int T,
                           const float* thr_dev, int Q, uint64_t seed,
                           int thresh, int width, void* stream);

/* ---- causal layer on one-hot input as a gather: wavenet/model.py:227-234
 * (_create_causal_layer) + :518-531 (_one_hot).  Wc is [K][Q][ldw] (the
 * 32 channels of one block start at Wc; ldw = padded channel count, 32 for
 * <= 32 residual channels), K = filter_width taps at shifts (K-1-k) + (K-1)/2;
 * x0 is the [B*T][32] plane of that block. */
int wn_causal_gather(const int32_t* q, const float* Wc, float* x0, int B,
                     int T, int Q, int K, int ldw, void* stream);

/* ---- causal layer on scalar input (scalar_input=True): wavenet/model.py:
 * 143-153, 227-234, 646-648; W is [K0][ldw] (ldw = padded channel count; for
 * more than 32 channels one call per 32-wide block with W + 32 * block and
 * that block's plane), K0 = initial_filter_width (any).
 * The wgrad writes [splits][K0*32] slabs for wn_reduce_slabs (per block). */
int wn_scalar_causal_fwd(const float* audio, const float* W, int ldw, float* x0,
                         int B, int T, int K0, void* stream);
int wn_scalar_causal_wgrad(const float* audio, const float* dx0, float* slabs,
                           int splits, int B, int T, int K0, void* stream);
/* one-hot causal layer, filter width 2: dWc[tap][v][32] as per-wave slabs
 * [num_slabs][2][Q][32] (reduce with wn_reduce_slabs, slab stride 2*Q*32);
 * Q <= 256, num_slabs = wn_causal_wgrad_slabs(B*T) */
int wn_causal_wgrad_slabs(long rows);
int wn_causal_wgrad(const int32_t* q, const float* dx0, float* slabs,
                    int num_slabs, int B, int T, int Q, void* stream);

/* ---- fused residual block: wavenet/model.py:236-330
 * (_create_dilation_layer) incl. both causal_conv calls, ops.py:46-62.
 * wblock = Wf[2][32][32] Wg[2][32][32] Wd[32][32] bf[32] bg[32] bd[32].
 * bias_fg: [B or 1][64] per-clip (bias + global-conditioning) or NULL. */
/* save_ts: 0 = nothing kept for backward (inference); 1 = tanh and sigmoid
 * planes (th, sg; the generic-tap *_k / channel-block *_blk kernels); 2 = the
 * sigmoid plane only (sg; th may be NULL) for wn_layer_bwd2, which recovers
 * tanh = z / sigmoid. */
int wn_layer_fwd(const float* x, float* x_out, float* z, float* th, float* sg,
                 const float* wblock, const float* bias_fg,
                 int bias_clip_stride, int B, int T, int dilation,
                 int has_dense, int save_ts, void* stream);
/* floats of a per-workgroup weight-gradient slab (layout = wblock) */
int wn_layer_wgrad_slab_floats(void);

/* generic filter width K >= 2 (off-default; the K = 2 kernels above are the
 * tuned path): block = Wf[K][32][32] Wg[K][32][32] Wd[32][32] bf bg bd,
 * tap k reads x[t - (K-1-k + (K-1)/2) * dilation] (ops.py:46-62). */
int wn_layer_fwd_k(const float* x, float* x_out, float* z, float* th,
                   float* sg, const float* wblock, const float* bias_fg,
                   int bias_clip_stride, int B, int T, int dilation, int K,
                   int has_dense, int save_ts, void* stream);
int wn_layer_bwd_k(const float* daf_cur, const float* dag_cur,
                   const float* dxin, float* dx_out, const float* wblock_b,
                   const float* dZ, const float* th, const float* sg,
                   const float* wblock_a, float* daf_next, float* dag_next,
                   int B, int T, int dilation, int K, int do_b, int do_a, int blocks, long blk_stride,
                   void* stream);
/* (k0 / Ktot: the K taps k0 .. k0 + K - 1 of a filter of Ktot taps; slab
 * layout [(2K+1) * 1024 + 96]: Wf taps, Wg taps, Wd, bf | bg | bd.  CB > 1: all
 * CB x CB (input block a, output block b) pairs of a channel-block layer in one
 * launch -- x / z are the first input plane, daf / dag / dxin the first output
 * plane, planes plane_stride floats apart, slabs [pair = a * CB + b][num_slabs]) */
int wn_layer_wgrad_k(const float* x, const float* daf, const float* dag,
                     const float* z, const float* dxin, float* slabs,
                     int num_slabs, int B, int T, int dilation, int K, int k0,
                     int Ktot, int CB, long plane_stride, void* stream);

/* out planes = addend planes + in planes * W (+ bias): the 1x1 residual conv
 * x_{l+1} = x_l + z_l Wd (+ bd) of wavenet/model.py:294-300, 330 for the
 * channel-block models (C = 32, 64, 96 or 128 padded channels = C / 32 planes of
 * [rows][32]) and its data gradient dz = dZ + dx_{l+1} Wd^T, as one streaming
 * launch per layer (a wave per 32-row tile) instead of a K = N = C plane-mode
 * wn_gemm_nn.  W [C][C] row-major ([Cin][Cout]); bias [C] or NULL; addend in
 * the planes' layout or NULL.  Other widths: WN_ERR_UNSUPPORTED (use wn_gemm_nn). */
int wn_dense_planes(const float* in, long in_plane_stride, const float* W,
                    const float* bias, const float* addend, long add_plane_stride,
                    float* out, long out_plane_stride, long rows, int C,
                    void* stream);
/* The backward's dz = dZ + dx_{l+1} Wd^T (wn_dense_planes with addend = dZ) and
 * the gate gradients of autodiff of wavenet/model.py:264-282 in one launch:
 * daf = dz s (1 - t^2), dag = dz s t (1 - s) with the saved tanh / sigmoid
 * planes th / sg; dz itself is not stored.  Bitwise the planes the two launches
 * (wn_dense_planes, then wn_layer_bwd_k with do_a only) give. */
int wn_dense_planes_gate(const float* in, long in_plane_stride, const float* W,
                         const float* addend, long add_plane_stride, const float* th,
                         const float* sg, long ts_plane_stride, float* daf, float* dag,
                         long da_plane_stride, long rows, int C, void* stream);

/* more than 32 residual / dilation channels: channels are cut into 32-wide
 * blocks, each block of an activation is its own [B*T][32] plane, and one
 * launch computes ONE output block from all input blocks (weights in the
 * reference's [K][Cin][Cout] layout, row stride ldw = padded channel count).
 * fwd: z / tanh / sigmoid planes of dilation block jb; wf / wg point at column
 * 32 jb of Wf / Wg; x is input block 0, block i at x + i * in_plane_stride.
 * bwd: dx plane of residual block rb from the da planes of all dilation
 * blocks; wf / wg point at row 32 rb; tap_stride = floats between taps.
 * K * blocks <= 8 PER CALL; wider layers run in chunks of blocks: fwd with
 * in_blocks = the chunk, x / wf / wg offset to its first block, tap_rows = the
 * rows between two taps of the weight matrix (the padded channel count), the
 * partial pre-activations handed from pre_out (planes af | ag, pre_plane_stride
 * apart; no gate, z / th / sg untouched) to the next call's pre_in (which
 * replaces the bias); bwd with da_blocks = the chunk and dxin = the previous
 * chunk's dx_out.  The 1x1 convs of such a layer are wn_gemm_nn calls in
 * plane mode; its weight gradients come from wn_layer_wgrad_k per block pair.
 * K / k0 / Ktot: the call covers taps k0 .. k0 + K - 1 of a filter of Ktot
 * taps (K * blocks <= 8 per call: wide layers run in chunks of blocks, filter
 * widths above 8 in groups of taps, chained through pre_in / pre_out and
 * dxin / dx_out).  out_blocks / dx_blocks > 1: that many consecutive output
 * (residual) blocks in one launch -- planes out_plane_stride (dx_plane_stride)
 * floats apart, weight columns (rows) and bias entries 32 further per block,
 * partial pre-activation planes [block][af | ag]. */
int wn_layer_fwd_blk(const float* x, long in_plane_stride, int in_blocks,
                     float* z, float* th, float* sg, const float* wf,
                     const float* wg, int ldw, const float* bias_f,
                     const float* bias_g, int bias_clip_stride, int B, int T,
                     int dilation, int K, int save_ts, int tap_rows,
                     const float* pre_in, float* pre_out, long pre_plane_stride,
                     int k0, int Ktot, int out_blocks, long out_plane_stride,
                     void* stream);
int wn_layer_bwd_blk(const float* daf, const float* dag, long da_plane_stride,
                     int da_blocks, const float* dxin, float* dx_out,
                     const float* wf, const float* wg, int ldw, long tap_stride,
                     int B, int T, int dilation, int K, int k0, int Ktot,
                     int dx_blocks, long dx_plane_stride, void* stream);

/* default backward of one block (TF autodiff of model.py:236-330), no
 * pre-activation-gradient planes in HBM: every tile recomputes da for its
 * rows t and t+d from dZ_l, dx_{l+1}, z_l and the sigmoid plane, so the only
 * plane written is dx_l (768 B of HBM traffic per sample and layer instead of
 * 1408 B).  dxin == NULL for the last layer (its dense output is unused,
 * model.py:294-300).  slabs: [wn_layer_bwd2_slabs(B, T)][wblock layout] weight
 * gradients of layer l; tile_colsum (optional): [B * ceil(T/32)][64] per-tile
 * column sums of da_f | da_g, reduced per clip for the global-conditioning
 * gradients. */
int wn_layer_bwd2_slabs(int B, int T);
/* wimg: this layer's image out of wn_layer_bwd2_pack (the five matrices
 * transposed with row stride 33, wn_layer_bwd2_wimg_floats() floats per layer,
 * L images back to back; rebuilt once per step), which the kernel pulls into
 * LDS by LDS-DMA; wblock is the plain layer block (A/B kernel variants). */
int wn_layer_bwd2_wimg_floats(void);
int wn_layer_bwd2_pack(const float* layer0, long layer_stride, float* wimg,
                       int L, void* stream);
int wn_layer_bwd2(const float* x, const float* z, const float* sg,
                  const float* dZ, const float* dxin, float* dx_out,
                  const float* wblock, const float* wimg, float* slabs,
                  float* tile_colsum, int B, int T, int dilation,
                  void* stream);

/* ---- the whole residual stack in ONE persistent launch (csrc/wn_stack.hip):
 * replaces the per-layer loop of WaveNetModel._create_network
 * (wavenet/model.py:417-428 over _create_dilation_layer, model.py:236-330) and
 * its gradient; same arithmetic per 32-row tile as wn_layer_fwd / wn_layer_bwd2.
 * A workgroup keeps a group of consecutive tiles for all L layers; the tile's
 * own rows stay in registers (forward), the dilated tap of another tile is
 * handed over through memory: sc1 stores, one flag per (layer, tile), sc1
 * loads.  No grid barrier; groups are handed out by an atomic ticket in
 * dependency order, so the launch completes whatever the residency.
 *   X, Z, SG, dZ     : [L][B*T][32] planes, layer-major (X[0] = causal layer
 *                      output; forward writes X[1..L-1], Z, SG; backward reads
 *                      X, Z, SG, dZ)
 *   DX, dx_layer_stride : the backward writes, at DX + l * dx_layer_stride
 *                      floats, dL/dx_0 for l = 0 and for l > 0 dL/dx_l WITHOUT the
 *                      anti-causal tap's term, which is Q[l] at the rows d_l
 *                      later.  dx_layer_stride = B*T*32 keeps every layer's
 *                      plane ([L][B*T][32]); 0: ONE [B*T][32] plane rewritten in
 *                      place from layer to layer (a tile's own rows have no
 *                      other reader; they stay in the L2 / Infinity Cache
 *                      instead of travelling to HBM and back every layer)
 *   Q                : an [L][B*T][32] scratch: a tile publishes q_l[s] =
 *                      da_l[s] W[0]^T, what its rows contribute to the rows d
 *                      earlier (the "push" formulation; every tile re-deriving
 *                      da at the rows d later cost more bytes and MFMAs)
 *   wimg             : [L][wn_stack_wimg_floats()] weight images out of
 *                      wn_stack_pack (rows of 36 floats so that four MFMA
 *                      operands are one 16-byte LDS read; forward: the five
 *                      matrices transposed + the dense bias, backward: as they
 *                      are; rebuilt whenever the parameters changed), pulled
 *                      into LDS by LDS-DMA.  Forward and backward take their
 *                      own image.
 *   bias             : [L][B or 1][64] filter|gate bias (+gc) of wn_gc_bias, or NULL
 *   dilations        : [L] int32, DEVICE memory
 *   flags            : wn_stack_flag_count(B, T, L) uint32, zero before first use
 *   ctl              : 4 uint32 {0, 0, 1, 0} before first use: {group ticket,
 *                      workgroups done, epoch, error}; the kernel re-arms the
 *                      first three.  ctl[3] != 0 after a launch: a bounded flag
 *                      wait (2 s) expired -- results are invalid
 *   poison           : NULL, or one float (0 before first use) that is set to
 *                      NaN in that case: summed into the loss reduction it
 *                      makes the failure loud without a host synchronisation
 *   forward and backward use SEPARATE flags / ctl buffers.
 *   slabs            : [L][slab_layer_stride floats], slab g of layer l at
 *                      l * slab_layer_stride + g * 5216, g < wn_stack_bwd_slabs(B, T, variant)
 *   tilesum          : as wn_layer_bwd2 ([L][tiles][64] or NULL), tiles =
 *                      B * ceil(T / wn_stack_tile_rows(B, T, variant))
 * Tile height: 32 rows; 16 for small batches (wn_stack_tile_rows: at most four
 * 32-row tiles per CU -- the launches are then bound by one wave's dependent
 * path through a layer, and a 16-row tile on v_mfma_f32_16x16x4_f32 halves
 * that path).  Both launches of a shape use the same height; it sets the slab count
 * (wn_stack_bwd_slabs) and the tilesum layout.  The 16-row results agree with
 * the 32-row ones to rounding (another summation grouping), not bitwise.
 *   variant          : 0 = the library's choice for the shape (what every
 *                      production caller passes), or a word built with
 *                      WN_STACK_VARIANT for A/B runs and tests.  The same word
 *                      goes to wn_stack_tile_rows / wn_stack_bwd_slabs /
 *                      wn_stack_fwd / wn_stack_bwd of one step: behaviour is a
 *                      function of the arguments only (no process environment
 *                      is read anywhere in the library).
 * L <= 256. */
/* rows: 0 (auto), 16 or 32 rows per tile; waves: 0 (auto) or waves per
 * workgroup (16-row launches: 4 / 8; 32-row backward: 1 / 2 / 4 / 8; the 32-row
 * forward ignores it) */
#define WN_STACK_VARIANT(rows, waves) (((rows) & 0x3f) | (((waves) & 0xf) << 8))
long wn_stack_flag_count(int B, int T, int L);
int wn_stack_tile_rows(int B, int T, int variant);
int wn_stack_wimg_floats(void);
int wn_stack_pack(const float* layer0, long layer_stride, float* wimg_fwd,
                  float* wimg_bwd, int L, void* stream);
int wn_stack_fwd(float* X, float* Z, float* SG, const float* wimg,
                 const float* bias, long bias_layer_stride,
                 int bias_clip_stride, const int* dilations, unsigned* flags,
                 unsigned* ctl, float* poison, int L, int B, int T, int save_sg,
                 int variant, void* stream);
/* Small batches (wn_stack_fwd_skip_ok: the 16-row launch with one tile per
 * SIMD, 512 skip channels): wn_stack_fwd that ALSO computes the skip sum,
 *   h1[B*T][512] = relu(sum_l z_l Ws_l + skip_bsum)
 * (model.py:505-509: what wn_gemm_nn over the Z planes computes afterwards) in
 * the same launch -- a partner wave per tile takes the tile's z of every layer
 * through LDS while the chain wave goes on; the launch's matrix pipe is three
 * quarters idle otherwise.  skip_img: wn_stack_skip_img_floats(L) floats written
 * by wn_stack_skip_pack from skip_w [L * 32][512] (a function of the weights
 * only; the Python host repacks it on every forward call);
 * skip_bsum: [512] or NULL.  Same sums as the GEMM up to the order of additions. */
int wn_stack_fwd_skip_ok(int B, int T, int S, int variant);
long wn_stack_skip_img_floats(int L);
int wn_stack_skip_pack(const float* skip_w, int L, float* img, void* stream);
int wn_stack_fwd_skip(float* X, float* Z, float* SG, const float* wimg,
                      const float* bias, long bias_layer_stride,
                      int bias_clip_stride, const int* dilations, unsigned* flags,
                      unsigned* ctl, float* poison, int L, int B, int T, int save_sg,
                      int variant, const float* skip_img, const float* skip_bsum,
                      float* h1, void* stream);
/* Local conditioning: wn_stack_fwd where row r of layer l ALSO adds its own
 * filter | gate addend lc_add[r * lc_row_stride + l * 64 .. + 63] (lc_add =
 * lc rows x the LC weights of all layers, one GEMM per pass) to the
 * pre-activations; r = b * T + t.  lc_row_stride >= 64 L, a multiple of 4;
 * lc_add 16-byte aligned.  32-row tiles only: a variant word that resolves to
 * 16 rows (wn_stack_tile_rows) is WN_ERR_UNSUPPORTED. */
int wn_stack_fwd_lc(float* X, float* Z, float* SG, const float* wimg,
                    const float* bias, long bias_layer_stride,
                    int bias_clip_stride, const int* dilations, unsigned* flags,
                    unsigned* ctl, float* poison, int L, int B, int T, int save_sg,
                    int variant, const float* lc_add, long lc_row_stride,
                    void* stream);
int wn_stack_bwd_slabs(int B, int T, int variant);
/* Launch-shape queries (no device needed: 256 CUs are assumed without one).
 * wn_stack_fwd_waves: waves (= tiles) per workgroup wn_stack_fwd / _fwd_lc
 * launch for the shape and variant word.  wn_stack_bwd_waves: waves per
 * workgroup of wn_stack_bwd / _bwd_lc, and its tiles per wave and layer in
 * *tiles_per_wave.  Both answer for the tile height wn_stack_tile_rows picks;
 * B or T <= 0 is WN_ERR_BAD_SHAPE, a NULL tiles_per_wave WN_ERR_NULL. */
int wn_stack_fwd_waves(int B, int T, int variant);
int wn_stack_bwd_waves(int B, int T, int variant, int* tiles_per_wave);
int wn_stack_bwd(const float* X, const float* Z, const float* SG,
                 const float* dZ, float* DX, long dx_layer_stride, float* Q,
                 const float* wimg, float* slabs,
                 long slab_layer_stride, float* tilesum, const int* dilations,
                 unsigned* flags, unsigned* ctl, float* poison, int L, int B,
                 int T, int variant, void* stream);
/* Local conditioning: wn_stack_bwd that ALSO stores the pre-activation
 * gradients da_f | da_g of row r and layer l at lc_da[r * lc_row_stride + l * 64
 * .. + 63] (same layout and constraints as wn_stack_fwd_lc's lc_add); the LC
 * weight gradients are lc^T da (wn_gemm_tn).  32-row tiles only. */
int wn_stack_bwd_lc(const float* X, const float* Z, const float* SG,
                    const float* dZ, float* DX, long dx_layer_stride, float* Q,
                    const float* wimg, float* slabs,
                    long slab_layer_stride, float* tilesum, const int* dilations,
                    unsigned* flags, unsigned* ctl, float* poison, int L, int B,
                    int T, int variant, float* lc_da, long lc_row_stride,
                    void* stream);

/* ---- fp32 MFMA GEMMs: the skip sum + post-processing of
 * wavenet/model.py:303-305, 430-440 (_create_network) and their gradients.
 * C = epi(A W): + bias, relu, * (mask > 0), + addend.  A dense [M][lda] or
 * a_planes planes of [M][32]; C dense [M][ldc] or c_planes planes of [M][32]
 * (c_plane_stride floats apart); an addend passed with ld_add == 0 is in C's
 * plane layout (needs c_planes > 0): the 1x1 residual conv of the
 * channel-block models, x_{l+1} planes = x_l planes + z_l Wd.  The epilogue
 * reaches the 32 rows of a wave's half tile through 32-bit byte offsets: ldc
 * (dense C, or any Cpre), ld_mask and ld_add beyond (31 ld + 64) * 4 < 2^31
 * (17 318 412 floats at most), a c_plane_stride of 2^29 - 1024 floats or
 * more, or a negative one of these, is WN_ERR_UNSUPPORTED before any launch. */
int wn_gemm_nn(const float* A, long lda, int a_planes, long a_plane_stride,
               const float* W, int ldw, const float* bias, const float* mask,
               long ld_mask, const float* addend, long ld_add, float* C,
               long ldc, int c_planes, long c_plane_stride, float* Cpre,
               long M, int N, int K, int relu, void* stream);

/* opt-in: same contraction with fp32 accuracy rebuilt from bf16 matrix
 * instructions (every operand split exactly into three bf16 pieces, nprod =
 * 3 / 6 / 9 piece products; 6 is as accurate as the fp32 MFMA path).
 * w_scratch: wn_gemm_split_w_bytes(K, N) bytes, caller-owned.  Not used unless
 * the host asks for it (WaveNetModel.gemm_mode). */
long wn_gemm_split_w_bytes(int K, int N);
int wn_gemm_nn_split(const float* A, long lda, int a_planes,
                     long a_plane_stride, const float* W, int ldw,
                     const float* bias, const float* mask, long ld_mask,
                     const float* addend, long ld_add, float* C, long ldc,
                     int c_planes, long c_plane_stride, float* Cpre, long M,
                     int N, int K, int relu, void* w_scratch, int nprod,
                     void* stream);
/* floats per slab of wn_gemm_tn: the Mw x Nw matrix and
 * wn_gemm_tn_tail_rows(Mw, Nw) rows of column sums behind it */
long wn_gemm_tn_slab_floats(int Mw, int Nw);
int wn_gemm_tn_tail_rows(int Mw, int Nw);
/* recommended `splits` for wn_gemm_tn (grid = one resident wave of
 * workgroups); kind: 0 dense A, 1 one-hot A, 2 wn_gemm_tn_split */
int wn_gemm_tn_splits(long rows, int Mw, int Nw, int kind);
/* opt-in split-bf16 variant of wn_gemm_tn (see wn_gemm_nn_split); dense or
 * plane A, rows % 16 == 0 */
int wn_gemm_tn_split(const float* A, long lda, int a_planes,
                     long a_plane_stride, const float* G, long ldg,
                     float* slabs, int splits, long rows, int Mw, int Nw,
                     int want_colsum, int nprod, void* stream);
/* want_colsum: 0 none; 1 the column sums of G (the bias gradient) in the first
 * tail row of every slab; 2 ("spread", shapes with wn_gemm_tn_tail_rows > 1
 * only): every tile row of a split sums its share of the rows into its own
 * tail row -- no workgroup carries all the extra adds, none falls behind and
 * re-fetches its chunks -- and wn_reduce_slabs_mt(tail_rows) adds the rows up */
int wn_gemm_tn(const float* A, long lda, int a_planes, long a_plane_stride,
               const int32_t* codes, int shift, int T, const float* G,
               long ldg, float* slabs, int splits, long rows, int Mw, int Nw,
               int want_colsum, void* stream);
int wn_reduce_slabs(const float* slabs, int num_slabs, long slab_stride,
                    int batch, long in_batch_stride, long offset, long n,
                    float* dst, long out_batch_stride, int replicate,
                    long rep_stride, void* stream);
/* the slabs of one wn_gemm_tn in ONE launch: elements [0, n_main) of every
 * slab (the matrix) -> dst_main, the n_tail elements behind them (column sums
 * = bias gradient; tail_rows partial rows of n_tail each, summed) -> dst_tail,
 * `replicate` copies rep_stride floats apart.
 * All counts / strides multiples of 4 floats, pointers 16-byte aligned. */
int wn_reduce_slabs_mt(const float* slabs, int num_slabs, long slab_stride,
                       long n_main, float* dst_main, long n_tail, float* dst_tail,
                       int replicate, long rep_stride, int tail_rows, void* stream);
/* channel-block models (more than 32 residual / dilation channels,
 * model.py:46-60 puts no limit on them): the wn_layer_wgrad_k slabs of the
 * CB x CB block pairs of one layer, slabs[pair = a * CB + b][num_slabs]
 * [(2K+1)*1024 + 96], summed in a fixed order and written into the layer's
 * gradient block (Wf [K][C][C], Wg, Wd [C][C] at 0; bf | bg | bd [C] each at
 * off_bias, from the pairs with a == 0).  The slabs hold taps tap0 .. tap0 +
 * K - 1 of a filter of Ktot taps (filter widths above 8 run in tap groups). */
int wn_reduce_pair_slabs(const float* slabs, int num_slabs, int CB, int K,
                         int has_dense, int use_bias, float* layer_grad, int C,
                         long off_bias, int tap0, int Ktot, void* stream);
int wn_transpose(const float* in, int rows, int cols, long in_ld, float* out,
                 long out_ld, void* stream);

/* ---- loss: wavenet/model.py:654-666 (shifted one-hot softmax xent, mean),
 * forward + TF-compatible backward; predict softmax in float64
 * (model.py:584-585, 620-621) */
int wn_xent_partials(long rows);
int wn_xent(const float* logits, long ld, const int32_t* q, float* dlogits,
            float* loss_partials, int B, int T, int Q, int tf_quirk,
            void* stream);
/* wn_xent for a batch of right-padded clips: lengths [B] (device int32, the
 * real samples of every clip, clamped to [0, T] by the kernel; the host
 * checks 1 <= lengths[b] <= T) and inv_den (device float, 1 / denominator:
 * 1 / sum(lengths) for the masked mean).  Clip b is treated as a clip of
 * T = lengths[b] fed alone; rows t >= lengths[b] add nothing to the loss and
 * get dlogits rows of exact zeros.  Both are READ FROM DEVICE MEMORY when the
 * kernel runs, so a recorded launch replays with the values staged for this
 * call.  Same partials as wn_xent; lengths[b] = T for every clip and
 * *inv_den = 1.0f / (float)(B*T) give wn_xent's results bit for bit.
 * lengths and inv_den 4-byte aligned, else WN_ERR_MISALIGNED. */
int wn_xent_masked(const float* logits, long ld, const int32_t* q,
                   const int32_t* lengths, const float* inv_den,
                   float* dlogits, float* loss_partials, int B, int T, int Q,
                   int tf_quirk, void* stream);
/* wn_xent_masked for clips with leading history: starts [B] (device int32,
 * clamped to [0, T] by the kernel; the host checks 0 <= starts[b] <=
 * lengths[b]) samples at the head of clip b are fed to the network but
 * predicted by nobody.  Row t has a target iff starts[b] <= t + 1 <
 * lengths[b]; rows with t + 1 < starts[b] add nothing to the loss and get
 * dlogits rows of exact zeros, without an exponential being evaluated, like
 * padding; row lengths[b] - 1 stays the label-less last row.  starts is read
 * from device memory when the kernel runs, like lengths and inv_den.  Same
 * partials as wn_xent_masked; starts all zero gives its results bit for bit.
 * Errors as wn_xent_masked (starts: NULL -5, 4-byte alignment -3), all
 * before any launch. */
int wn_xent_window(const float* logits, long ld, const int32_t* q,
                   const int32_t* starts, const int32_t* lengths,
                   const float* inv_den, float* dlogits, float* loss_partials,
                   int B, int T, int Q, int tf_quirk, void* stream);
/* Scoring of held-out data (WaveNetModel.score): the inputs of wn_xent_masked
 * (lengths may be NULL: every clip has T rows), forward only.
 *   row_nll      float [B*T], may be NULL: logsumexp(logits[b,t,:Q]) -
 *                logits[b,t,q[b,t+1]] where row (b, t) has a target -- t + 1 <
 *                len_b (lengths[b] clamped to [0, T]) and 0 <= q[b,t+1] < Q,
 *                the loss kernels' rule -- and 0.0 elsewhere (the label-less
 *                last row, padding: no exponential is evaluated there);
 *   clip_nll     double [B]: the sum of clip b's row_nll values in float64;
 *   clip_count   int32 [B]: its rows with a target;
 *   clip_correct int32 [B]: those whose arg-max over [0, Q) is the target
 *                (the lowest index wins a tie; a row containing NaN is never
 *                correct, and its NaN reaches clip_nll).
 * The row arithmetic is wn_xent's (float32); columns >= Q are not read.  The
 * per-clip sums have a fixed order (no atomics): a function of the rows and
 * len_b alone, the same bits with and without row_nll.  lengths is read from
 * device memory when the kernels run.  scratch: wn_xent_score_scratch_floats(
 * B*T) floats, caller-owned.  Errors as wn_xent (NULL -5, shape -1, Q % 4 or
 * ld % 4 -2, alignment -3: logits 16 bytes, clip_nll 8, the others 4), all
 * before any launch. */
long wn_xent_score_scratch_floats(long rows);
int wn_xent_score(const float* logits, long ld, const int32_t* q,
                  const int32_t* lengths, float* row_nll, double* clip_nll,
                  int32_t* clip_count, int32_t* clip_correct, float* scratch,
                  int B, int T, int Q, void* stream);
/* wn_xent_score with wn_xent_window's starts (may be NULL: no history): rows
 * with t + 1 < starts[b] have no target either (row_nll 0.0, nothing
 * evaluated), clip_count[b] = len_b - max(starts[b], 1) for codes in range,
 * and the per-clip sums run over rows max(starts[b] - 1, 0) .. len_b - 2 in
 * the same fixed order.  starts NULL or all zero gives wn_xent_score's bits.
 * starts 4-byte aligned, else WN_ERR_MISALIGNED. */
int wn_xent_score_window(const float* logits, long ld, const int32_t* q,
                         const int32_t* starts, const int32_t* lengths,
                         float* row_nll, double* clip_nll, int32_t* clip_count,
                         int32_t* clip_correct, float* scratch, int B, int T,
                         int Q, void* stream);
int wn_softmax64_row(const float* logits_row, int Q, float* proba,
                     void* stream);

/* ---- optimizers with TensorFlow-0.10 update rules: wavenet/ops.py:6-24 */
int wn_adam(float* p, const float* g, float* m, float* v, long n, float lr_t,
            float beta1, float beta2, float eps, float grad_scale, float l2,
            const float* l2_mask, void* stream);
int wn_momentum(float* p, const float* g, float* acc, long n, float lr,
                float momentum, float grad_scale, float l2,
                const float* l2_mask, void* stream);
int wn_rmsprop(float* p, const float* g, float* ms, float* mom, long n,
               float lr, float decay, float momentum, float eps,
               float grad_scale, float l2, const float* l2_mask,
               void* stream);
/* ---- global-norm gradient clipping (tf.clip_by_global_norm) and an
 * exponential moving average of the weights (tf.train.
 * ExponentialMovingAverage, no num_updates warm-up) inside the update.
 *
 * wn_grad_norm_partials writes wn_grad_norm_partials_count() (a constant)
 * float64 sums of g[i]^2: partial k covers a contiguous range that depends on
 * (n, count) only and is summed in a fixed order, no atomics -- the partials
 * are a function of the bucket's bits and n, not of the device.  g 16-byte,
 * partials 8-byte aligned, else WN_ERR_MISALIGNED.
 *
 * wn_*_clip: the update of wn_adam / wn_momentum / wn_rmsprop with
 *   partials, nparts : the partials above (nparts == the count, else
 *                      WN_ERR_BAD_SHAPE); NULL: no clipping
 *   clip_norm        : positive and finite (else WN_ERR_BAD_SHAPE).  Every
 *                      workgroup sums the partials in the same order in
 *                      float64; norm = grad_scale * sqrt(sum), factor =
 *                      clip_norm / max(norm, clip_norm), both float64; the
 *                      gradient is scaled by grad_scale * (float)factor.
 *                      norm <= clip_norm: factor is exactly 1 and the update
 *                      is the plain entry point's bit for bit.  A non-finite
 *                      norm gives a NaN factor, hence NaN parameters.
 *   ema, ema_decay   : shadow weights [n], s -= (1 - decay) * (s - p_new) in
 *                      float32 in the same pass; decay in [0, 1) (else
 *                      WN_ERR_BAD_SHAPE); NULL: no EMA
 *   norm_out         : one float, the norm before clipping (written only with
 *                      partials); may be NULL. */
int wn_grad_norm_partials_count(void);
int wn_grad_norm_partials(const float* g, long n, double* partials,
                          void* stream);
int wn_adam_clip(float* p, const float* g, float* m, float* v, long n,
                 float lr_t, float beta1, float beta2, float eps,
                 float grad_scale, float l2, const float* l2_mask,
                 const double* partials, int nparts, float clip_norm,
                 float* ema, float ema_decay, float* norm_out, void* stream);
int wn_momentum_clip(float* p, const float* g, float* acc, long n, float lr,
                     float momentum, float grad_scale, float l2,
                     const float* l2_mask, const double* partials, int nparts,
                     float clip_norm, float* ema, float ema_decay,
                     float* norm_out, void* stream);
int wn_rmsprop_clip(float* p, const float* g, float* ms, float* mom, long n,
                    float lr, float decay, float momentum, float eps,
                    float grad_scale, float l2, const float* l2_mask,
                    const double* partials, int nparts, float clip_norm,
                    float* ema, float ema_decay, float* norm_out,
                    void* stream);
int wn_l2_partials_count(void);
int wn_l2_partials(const float* p, long n, const float* mask, float* partials,
                   void* stream);

/* ---- global conditioning: wavenet/model.py:272-284, 533-562.  ch = padded
 * dilation channel count (32, or 64 with two channel blocks): out is
 * [L][B][2 ch] = filter | gate bias (+ embedding * Wgc), dsum likewise. */
int wn_gc_bias(const float* layer0, long layer_stride, long off_bias,
               long off_gc, int G, const float* emb, int card,
               const int32_t* ids, float* out, int L, int B, int ch,
               void* stream);
int wn_colsum_clip_chunks(int T);
int wn_colsum_clip(const float* plane0, const float* plane1, int B, int T,
                   float* part, float* out, void* stream);
int wn_gc_grad(const float* layer0, long layer_stride, long off_gc, int G,
               const float* emb, int card, const int32_t* ids,
               const float* dsum, int L, int B, float* glayer0, float* gemb,
               float* scratch /* L * B * G floats */, int ch, void* stream);

/* ---- thin exported ops of wavenet/__init__.py:1-4 (arbitrary shapes):
 * causal_conv ops.py:46-62, time_to_batch :27-34, batch_to_time :37-43 */
int wn_causal_conv(const float* x, const float* w, float* y, int B, int T,
                   int Cin, int Cout, int K, int dilation, void* stream);
int wn_time_to_batch(const float* in, float* out, int B, int T, int C,
                     int dilation, void* stream);
int wn_batch_to_time(const float* in, float* out, int B_out, int U, int C,
                     int dilation, void* stream);

/* ---- diagnostics: register-only fp32 MFMA loop (clock-limited ceiling) */
int wn_diag_mfma_peak(float* out, int blocks, int iters, void* stream);

/* ---- utilities */
int wn_axpy(float* y, const float* x, float a, const float* mask, long n,
            void* stream);
int wn_fill(float* p, long n, float value, void* stream);
int wn_sum_rows(const float* in, int rows, int n, float* out, void* stream);

/* ---- fast generation: wavenet/model.py:332-387, 444-516, 592-626
 * (_create_generator / predict_proba_incremental) and the host loop of
 * generate.py:213-241, as ONE persistent kernel with the FIFO state on the
 * device and on-device sampling. */
long wn_fastgen_state_floats(const int32_t* dilations_host, int L);
int wn_fastgen_init(float* state, long state_floats, int32_t* cursors, int L,
                    void* stream);   /* cursors: int32[>= 3] */
/* samples_io holds n_steps + 1 codes; the first n_given are inputs (seed /
 * priming, generate.py:195-210), the rest are drawn on the device.  Step i
 * consumes samples_io[i]; proba_out (optional) receives the next-sample
 * distribution of every proba_every-th step.  push = 0 (n_steps must be 1)
 * evaluates a step without advancing the queues (the reference's proba op run
 * without net.push_ops, test/test_generation.py:66-68). */
int wn_fastgen_run(const float* params_causal, const float* layer0,
                   long layer_stride, const float* skip_w,
                   const float* skip_bsum, const float* post1_w,
                   const float* post1_b, const float* post2_w,
                   const float* post2_b, const float* gc_bias_fg,
                   const int32_t* dilations_dev, int L, int S, int Q,
                   float* state, int32_t* cursors, int32_t* samples_io,
                   int n_given, int n_steps, float temperature, uint64_t seed,
                   float* proba_out, int proba_every, int use_biases,
                   int push, void* stream);

/* The same generator for C = 32 * blocks > 32 padded residual / dilation
 * channels (the reference's generator has no width limit, model.py:444-516):
 * layer blocks Wf[2][C][C] Wg[2][C][C] Wd[C][C] bf[C] bg[C] bd[C], causal
 * [2][Q][C], skip [L][C][S], gc_bias_fg [L][2 C], queue entries of C floats
 * (state_floats = sum(dilations) * C).  C <= 1024, S <= 4096, Q <= 4096,
 * L <= 1024 and 8 Q + 4 (5 C + 2 S + 3 L) <= 150 KB of LDS; C = 32 is accepted
 * too (the host uses this entry for 32-channel models beyond the S / Q <= 512,
 * L <= 64 of wn_fastgen_run / wn_fastgen_step).  One persistent workgroup,
 * correctness first -- except with `coop` scratch (S <= 512 a multiple of 16,
 * Q <= 512): a COOPERATIVE launch,
 * workgroup 0 runs the layers and the draw, 2 S / 16 + Q / 16 more workgroups the
 * skip sum and the post-processing mat-vecs (hand-over words in `coop`; the
 * same samples up to the rounding of the skip sum's order).  It is launched
 * with hipLaunchCooperativeKernel (residency is the runtime's promise) behind
 * the library's own occupancy check; refused, or with coop = NULL, the single
 * workgroup runs.
 * coop: NULL, or wn_fastgen_wide_coop_bytes(L, C, S, Q) bytes (16-byte aligned,
 * zeroed by the call).  After a cooperative run ((unsigned*)coop)[12] != 0
 * means a hand-over wait expired (2 s): that run's samples are not valid. */
long wn_fastgen_wide_coop_bytes(int L, int C, int S, int Q);
int wn_fastgen_run_wide(const float* params_causal, const float* layer0,
                        long layer_stride, const float* skip_w,
                        const float* skip_bsum, const float* post1_w,
                        const float* post1_b, const float* post2_w,
                        const float* post2_b, const float* gc_bias_fg,
                        const int32_t* dilations_dev, int L, int C, int S, int Q,
                        float* state, int32_t* cursors, int32_t* samples_io,
                        int n_given, int n_steps, float temperature,
                        uint64_t seed, float* proba_out, int proba_every,
                        int use_biases, int push, void* coop, void* stream);

/* Multi-CU variant: enqueues ONE generation step as four kernels (chain on
 * one CU, current tap only, preceded by the previous step's float64 softmax +
 * draw; skip sum + the NEXT step's past-tap pre-activations, conv1 and conv2
 * on S/16 / Q/16 CUs).  Everything step- or call-dependent lives in device memory
 * (cursors, ctl), so the host captures a few hundred calls into a hipGraph
 * ONCE and replays it for every generate() call.
 * ctl: int32[8] = {base (cursors[0] when the call started), n_given,
 * proba_every, temperature (float bits), seed lo, seed hi, top_k, top_p
 * (float bits)}; top_k / top_p: the truncated draw of wn_fastgen_run_trunc
 * below, 0 = off.
 * pre: float[L][64], maintained by the step kernels; wn_fastgen_pre fills it
 * for the step the queues are at (call once before a sequence of steps). */
int wn_fastgen_step(const float* params_causal, const float* layer0,
                    long layer_stride, const float* skip_w,
                    const float* skip_bsum, const float* post1_w,
                    const float* post1_b, const float* post2_w,
                    const float* post2_b, const float* gc_bias_fg,
                    const int32_t* dilations_dev, int L, int S, int Q,
                    float* state, int32_t* cursors, int32_t* samples_io,
                    const int32_t* ctl, float* proba_out, int use_biases,
                    const float* cw_img, float* pre, float* z_all, float* h1,
                    float* h2, float* logits, void* stream);
/* cursors is int32[4] for the step path: {steps done, previous code, draw
 * pending, 0}.  A step's softmax / draw / cursor update runs at the start of
 * the NEXT step's chain kernel; wn_fastgen_finish does it for the last step
 * of a sequence (no-op when nothing is pending). */
int wn_fastgen_finish(int Q, int32_t* cursors, int32_t* samples_io,
                      const int32_t* ctl, float* proba_out, const float* logits,
                      void* stream);

/* ONE persistent multi-CU launch for n_steps samples (csrc/wn_fastgen.hip,
 * fg_persist_kernel): the same inputs, state and results as n_steps x
 * wn_fastgen_step + wn_fastgen_finish, without a kernel boundary per stage and
 * with every workgroup's weights resident for the run (chain segments of ~10
 * layers in LDS, skip / post-processing slices in LDS; the stages hand over
 * through sc1 payloads + relaxed agent-scope flags).  cursors[2] must be 0 on
 * entry.  sync: 16 uint32 (zeroed by the call; sync[12] != 0 afterwards = a
 * bounded wait expired, results invalid); ll: wn_fastgen_persist_ll_words(L, S,
 * Q) 8-byte hand-over words (payload + step in one store; zeroed by the call).
 * Needs all wn_fastgen_persist_workgroups(L, S, Q) workgroups resident at once:
 * checked against hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs for the
 * launch configuration, then launched with hipLaunchCooperativeKernel, which
 * makes residency the runtime's promise -- else WN_ERR_UNSUPPORTED, returned
 * before any generator state is written: use wn_fastgen_step.  Should a
 * hand-over wait expire all the same (2 s), it surfaces as sync[12] -- the
 * caller restores its own snapshot of state / cursors / pre and takes the step
 * kernels.  The chain's workgroups (draw, segments) take the blocks 0, 8, 16,
 * ... (one XCD: a hand-over word is 0.15 us faster inside an XCD). */
int wn_fastgen_persist_workgroups(int L, int S, int Q);
/* role (0 .. total - 1: chain segments, skip, post1, logits, draw) of workgroup
 * `block` of the launch: the chain's roles on the blocks 0, 8, 16, ... (host-side
 * mirror of the kernel's mapping, for tests) */
int wn_fastgen_persist_role(int block, int total, int nseg);
long wn_fastgen_persist_ll_words(int L, int S, int Q);
int wn_fastgen_persist(const float* params_causal, const float* layer0,
                       long layer_stride, const float* skip_w,
                       const float* skip_bsum, const float* post1_w,
                       const float* post1_b, const float* post2_w,
                       const float* post2_b, const float* gc_bias_fg,
                       const int32_t* dilations_dev, int L, int S, int Q,
                       float* state, int32_t* cursors, int32_t* samples_io,
                       const int32_t* ctl, float* proba_out, int use_biases,
                       const float* cw_img, float* pre, float* z_all, float* h1,
                       float* h2, float* logits, unsigned* sync,
                       unsigned long long* ll, int n_steps, void* stream);
int wn_fastgen_pre(const float* layer0, long layer_stride,
                   const float* gc_bias_fg, const int32_t* dilations_dev,
                   int L, const float* state, const int32_t* cursors,
                   float* pre, void* stream);
/* cw_img [L][3072]: Wf[1] | Wg[1] | Wd of every layer, transposed + swizzled
 * for the chain's LDS ring */
int wn_fastgen_pack(const float* layer0, long layer_stride, float* img, int L,
                    void* stream);

/* ---- batched fast generation (csrc/wn_fastgen_batch.hip): 1 <= B <= 256
 * independent streams stepped in lock step, the streams on the MFMA rows of
 * the chain (32 per workgroup).  Shapes of wn_fastgen_step: C = 32, S <= 512,
 * Q <= 512, L <= 64.  Rows are padded to Bp = wn_fastgen_batch_rows(B) (a
 * multiple of 32); a stream's results do not depend on B or on its position.
 * Buffers: state float[wn_fastgen_batch_state_floats] (ring rows [sum d][Bp][32]),
 * cursors int32[4] ({steps pushed, draw pending, 0, 0}), prev int32[Bp] (code
 * consumed one step back), pre float[L][Bp][64], z_all float[Bp][L * 32],
 * h1 / h2 float[Bp][S], logits float[Bp][Q], seeds uint64[B].
 * gc_bias_fg: [L][B][64] with bias_stream_stride 64 (per-stream GC bias), or
 * [L][1][64] with 0, or NULL.
 * samples_io int32[B][ctl[4]]: stream b's step i consumes samples_io[b][i]
 * (cursors[0] - ctl[0] = i); proba_out (optional) float[B][ctl[5]][Q].
 * ctl: int32[8] = {base (cursors[0] when the call started), n_given,
 * proba_every, temperature (float bits), samples row stride, proba rows per
 * stream, top_k, top_p (float bits)} (the truncated draw of
 * wn_fastgen_run_trunc, one setting for all streams; 0 = off).
 * The draw of stream b takes seeds[b] and the counter rule of
 * the single-stream generator.  A step's draw runs at the start of the NEXT
 * step; wn_fastgen_batch_finish draws for the last one (no-op when none is
 * pending).  wn_fastgen_batch_pre fills pre for the step the queues are at
 * (call once before a sequence of steps). */
int wn_fastgen_batch_rows(int B);
long wn_fastgen_batch_state_floats(const int32_t* dilations_host, int L, int B);
int wn_fastgen_batch_init(float* state, long state_floats, int32_t* cursors,
                          int32_t* prev, int B, void* stream);
int wn_fastgen_batch_pre(const float* layer0, long layer_stride,
                         const float* gc_bias_fg, int bias_stream_stride,
                         const int32_t* dilations_dev, int L, int B,
                         const float* state, const int32_t* cursors, float* pre,
                         void* stream);
int wn_fastgen_batch_step(const float* params_causal, const float* layer0,
                          long layer_stride, const float* skip_w,
                          const float* skip_bsum, const float* post1_w,
                          const float* post1_b, const float* post2_w,
                          const float* post2_b, const float* gc_bias_fg,
                          int bias_stream_stride, const int32_t* dilations_dev,
                          int L, int S, int Q, int B, float* state,
                          int32_t* cursors, int32_t* prev, int32_t* samples_io,
                          const int32_t* ctl, const uint64_t* seeds,
                          float* proba_out, int use_biases, float* pre,
                          float* z_all, float* h1, float* h2, float* logits,
                          void* stream);
/* The stages [first, last) of one step (0 draw, 1 chain, 2 skip sum + next
 * pre-activations, 3 post1, 4 logits; wn_fastgen_batch_step = 0 .. 5), same
 * arguments: for timing each launch between the caller's own events. */
int wn_fastgen_batch_stages(int first, int last, const float* params_causal,
                            const float* layer0, long layer_stride,
                            const float* skip_w, const float* skip_bsum,
                            const float* post1_w, const float* post1_b,
                            const float* post2_w, const float* post2_b,
                            const float* gc_bias_fg, int bias_stream_stride,
                            const int32_t* dilations_dev, int L, int S, int Q,
                            int B, float* state, int32_t* cursors, int32_t* prev,
                            int32_t* samples_io, const int32_t* ctl,
                            const uint64_t* seeds, float* proba_out,
                            int use_biases, float* pre, float* z_all, float* h1,
                            float* h2, float* logits, void* stream);
int wn_fastgen_batch_finish(int Q, int B, int32_t* cursors, int32_t* samples_io,
                            const int32_t* ctl, const uint64_t* seeds,
                            float* proba_out, const float* logits, void* stream);
/* Restarting single streams (bulk synthesis refills the slot of a finished
 * utterance).  The counter rule above draws with counter = step; the origin
 * rule: with origins int32[Bp] the counter of stream b is step - origins[b],
 * so a stream restarted at step T0 draws as a fresh stream does from step 0.
 * The _q entries are wn_fastgen_batch_step / _step_lc / _finish with the
 * origin rule (origins in front of the stream; NULL: WN_ERR_NULL); nothing
 * else in a step knows about origins, the ring position stays cursors[0] % d.
 * wn_fastgen_batch_restart, one launch: for every stream b < B with
 * flags[b] != 0 (flags int32[Bp] on the device) the 32 floats of b in every
 * ring row become zeros, prev[b] = -1 and origins[b] = cursors[0] (read on
 * the device); no word of another stream is written.  Valid only with no
 * draw pending (cursors[1] == 0: after wn_fastgen_batch_finish[_q]) and
 * before the wn_fastgen_batch_pre[_lc] of the next sequence of steps. */
int wn_fastgen_batch_step_q(const float* params_causal, const float* layer0,
                            long layer_stride, const float* skip_w,
                            const float* skip_bsum, const float* post1_w,
                            const float* post1_b, const float* post2_w,
                            const float* post2_b, const float* gc_bias_fg,
                            int bias_stream_stride, const int32_t* dilations_dev,
                            int L, int S, int Q, int B, float* state,
                            int32_t* cursors, int32_t* prev, int32_t* samples_io,
                            const int32_t* ctl, const uint64_t* seeds,
                            float* proba_out, int use_biases, float* pre,
                            float* z_all, float* h1, float* h2, float* logits,
                            const int32_t* origins, void* stream);
int wn_fastgen_batch_finish_q(int Q, int B, int32_t* cursors, int32_t* samples_io,
                              const int32_t* ctl, const uint64_t* seeds,
                              float* proba_out, const float* logits,
                              const int32_t* origins, void* stream);
int wn_fastgen_batch_restart(float* state, const int32_t* dilations_dev, int L,
                             int B, const int32_t* cursors, int32_t* prev,
                             int32_t* origins, const int32_t* flags,
                             void* stream);
/* The LC rows of n lock-step steps from position pos0 for B streams holding
 * different items: out float[B][n][Lc].  table int64[B][3] on the device:
 * {address of the item's rows float[m_b][Lc] (0: no item), the stream's
 * origin, m_b}.  With t = pos0 + j - origin_b: out[b][j] = rows_b[t - 1] for
 * 1 <= t <= m_b, exact zeros elsewhere; nothing at or behind row m_b is read. */
int wn_fastgen_batch_lc_rows(const int64_t* table, int B, int n, int Lc,
                             long pos0, float* out, void* stream);

/* ---- local conditioning in fast generation (csrc/wn_fastgen_lc.hip).
 * The conditioned-bias ring: for positions p = p0 .. p0 + n_rows - 1 and every
 * stream b,
 *   ring[p % R][l][b][0:64] = gc_bias_fg[l][b] + sum_k lc[b][p - p0][k] lc_w[k][l][0:64]
 * (lc row i of stream b at lc + b * lc_stream_stride + i * Lc; lc_w the
 * model's [Lcp][L][64] segment; gc_bias_fg as wn_fastgen_batch_pre's, or NULL).
 * The sum is one fmaf chain in k order: a row's bits depend on Lc only.
 * ring_stream_stride 64: ring [R][L][B][64]; 0: [R][L][1][64], one row for
 * all streams (then lc_stream_stride and bias_stream_stride must be 0).
 * n_rows <= R, 1 <= B <= 256. */
int wn_fastgen_lc_bias(const float* lc, long lc_stream_stride, int Lc,
                       const float* lc_w, int L, const float* gc_bias_fg,
                       int bias_stream_stride, int B, long p0, int n_rows,
                       float* ring, int R, int ring_stream_stride, void* stream);
/* The _lc variants take the arguments of their entry point plus the ring
 * (lc_ring, its rows lc_R, its stream stride lc_stride: 0 or 64) and read the
 * filter|gate bias of step p from ring row p % lc_R in place of gc_bias_fg
 * (which they still accept and do not read).  Step p is the step that
 * consumes the input at position p (cursors[0] = p when it starts): its row
 * holds the LC row beside that input.  Everything else is the plain entry
 * point's: the draw, the chain, the skip sum and the post-processing. */
int wn_fastgen_run_lc(const float* params_causal, const float* layer0,
                      long layer_stride, const float* skip_w,
                      const float* skip_bsum, const float* post1_w,
                      const float* post1_b, const float* post2_w,
                      const float* post2_b, const float* gc_bias_fg,
                      const int32_t* dilations_dev, int L, int S, int Q,
                      float* state, int32_t* cursors, int32_t* samples_io,
                      int n_given, int n_steps, float temperature,
                      uint64_t seed, float* proba_out, int proba_every,
                      int use_biases, int push, const float* lc_ring, int lc_R,
                      int lc_stride, void* stream);

/* ---- top-k / nucleus (top-p) truncation of the draw.  Between the
 * temperature and the inverse CDF the draw keeps, of the float32
 * probabilities p it returns in proba_out (which stay untruncated):
 *   top_k  the codes with p >= the top_k-th largest p (a tie at the cut keeps
 *          its whole tie group); 0 or >= Q: every code
 *   top_p  then, with w the tempered weights of what top_k kept: the smallest
 *          set {p >= c} whose float64 w-mass is >= (double)top_p * sum(w);
 *          0 or 1: every code
 * and gives every other code weight exactly 0, so it is never drawn; the
 * uniform and its counter rule are unchanged.  0 <= top_k, 0 <= top_p <= 1.
 * The step, persistent and batched entry points read both from ctl words 6, 7;
 * the entries with a scalar temperature have the counterparts below: the
 * arguments of their entry point with top_k, top_p in front of the stream.
 * top_k = 0, top_p = 0 is the plain entry point, bit for bit. */
int wn_fastgen_run_trunc(const float* params_causal, const float* layer0,
                         long layer_stride, const float* skip_w,
                         const float* skip_bsum, const float* post1_w,
                         const float* post1_b, const float* post2_w,
                         const float* post2_b, const float* gc_bias_fg,
                         const int32_t* dilations_dev, int L, int S, int Q,
                         float* state, int32_t* cursors, int32_t* samples_io,
                         int n_given, int n_steps, float temperature,
                         uint64_t seed, float* proba_out, int proba_every,
                         int use_biases, int push, int top_k, float top_p,
                         void* stream);
int wn_fastgen_run_wide_trunc(const float* params_causal, const float* layer0,
                              long layer_stride, const float* skip_w,
                              const float* skip_bsum, const float* post1_w,
                              const float* post1_b, const float* post2_w,
                              const float* post2_b, const float* gc_bias_fg,
                              const int32_t* dilations_dev, int L, int C, int S,
                              int Q, float* state, int32_t* cursors,
                              int32_t* samples_io, int n_given, int n_steps,
                              float temperature, uint64_t seed, float* proba_out,
                              int proba_every, int use_biases, int push,
                              void* coop, int top_k, float top_p, void* stream);
int wn_fastgen_run_lc_trunc(const float* params_causal, const float* layer0,
                            long layer_stride, const float* skip_w,
                            const float* skip_bsum, const float* post1_w,
                            const float* post1_b, const float* post2_w,
                            const float* post2_b, const float* gc_bias_fg,
                            const int32_t* dilations_dev, int L, int S, int Q,
                            float* state, int32_t* cursors, int32_t* samples_io,
                            int n_given, int n_steps, float temperature,
                            uint64_t seed, float* proba_out, int proba_every,
                            int use_biases, int push, const float* lc_ring,
                            int lc_R, int lc_stride, int top_k, float top_p,
                            void* stream);
int wn_fastgen_pre_lc(const float* layer0, long layer_stride,
                      const float* gc_bias_fg, const int32_t* dilations_dev,
                      int L, const float* state, const int32_t* cursors,
                      float* pre, const float* lc_ring, int lc_R, int lc_stride,
                      void* stream);
int wn_fastgen_step_lc(const float* params_causal, const float* layer0,
                       long layer_stride, const float* skip_w,
                       const float* skip_bsum, const float* post1_w,
                       const float* post1_b, const float* post2_w,
                       const float* post2_b, const float* gc_bias_fg,
                       const int32_t* dilations_dev, int L, int S, int Q,
                       float* state, int32_t* cursors, int32_t* samples_io,
                       const int32_t* ctl, float* proba_out, int use_biases,
                       const float* cw_img, float* pre, float* z_all, float* h1,
                       float* h2, float* logits, const float* lc_ring, int lc_R,
                       int lc_stride, void* stream);
int wn_fastgen_persist_lc(const float* params_causal, const float* layer0,
                          long layer_stride, const float* skip_w,
                          const float* skip_bsum, const float* post1_w,
                          const float* post1_b, const float* post2_w,
                          const float* post2_b, const float* gc_bias_fg,
                          const int32_t* dilations_dev, int L, int S, int Q,
                          float* state, int32_t* cursors, int32_t* samples_io,
                          const int32_t* ctl, float* proba_out, int use_biases,
                          const float* cw_img, float* pre, float* z_all,
                          float* h1, float* h2, float* logits, unsigned* sync,
                          unsigned long long* ll, int n_steps,
                          const float* lc_ring, int lc_R, int lc_stride,
                          void* stream);
int wn_fastgen_batch_pre_lc(const float* layer0, long layer_stride,
                            const float* gc_bias_fg, int bias_stream_stride,
                            const int32_t* dilations_dev, int L, int B,
                            const float* state, const int32_t* cursors,
                            float* pre, const float* lc_ring, int lc_R,
                            int lc_stride, void* stream);
int wn_fastgen_batch_step_lc(const float* params_causal, const float* layer0,
                             long layer_stride, const float* skip_w,
                             const float* skip_bsum, const float* post1_w,
                             const float* post1_b, const float* post2_w,
                             const float* post2_b, const float* gc_bias_fg,
                             int bias_stream_stride,
                             const int32_t* dilations_dev, int L, int S, int Q,
                             int B, float* state, int32_t* cursors,
                             int32_t* prev, int32_t* samples_io,
                             const int32_t* ctl, const uint64_t* seeds,
                             float* proba_out, int use_biases, float* pre,
                             float* z_all, float* h1, float* h2, float* logits,
                             const float* lc_ring, int lc_R, int lc_stride,
                             void* stream);
int wn_fastgen_batch_step_lc_q(const float* params_causal, const float* layer0,
                               long layer_stride, const float* skip_w,
                               const float* skip_bsum, const float* post1_w,
                               const float* post1_b, const float* post2_w,
                               const float* post2_b, const float* gc_bias_fg,
                               int bias_stream_stride,
                               const int32_t* dilations_dev, int L, int S, int Q,
                               int B, float* state, int32_t* cursors,
                               int32_t* prev, int32_t* samples_io,
                               const int32_t* ctl, const uint64_t* seeds,
                               float* proba_out, int use_biases, float* pre,
                               float* z_all, float* h1, float* h2, float* logits,
                               const float* lc_ring, int lc_R, int lc_stride,
                               const int32_t* origins, void* stream);

/* ---- learned upsampling of frame-rate local-conditioning features
 * (csrc/wn_lc.hip).  scales: host array of m (1..8) ints >= 2, hop = their
 * product <= 4096.  `up`: the model's lc_up segment, the filters W_i[s_i][3] of
 * all layers back to back, then (use_bias) the m biases;
 * wn_lc_upsample_floats(scales, m, use_bias) floats (0 for bad scales).
 * Layer i maps an input row u to output slot j of s_i:
 *   out[c] = b_i + W_i[j][0] u[c-1] + W_i[j][1] u[c] + W_i[j][2] u[c+1]
 * (u[-1] = u[Lc] = 0).  Row r = b * T + t gets frame p / hop of clip b,
 * p = off[b] + t, through the slot digits of p % hop (most significant
 * first).  frames [B][F][Lc]; off int32 [B] on the device; 1 <= Lc <= 512.
 * fwd writes rows[r * ld_rows + 0 .. ld_rows - 1], zeros from column Lc on.
 * bwd: every workgroup owns a fixed range of rows and writes the
 * (layer, slot, tap) and bias partials of d rows [N][ld_drows] into its slab
 * (slab_stride >= wn_lc_upsample_floats floats, same layout as `up`); sum
 * them with wn_reduce_slabs.  num_slabs = wn_lc_upsample_bwd_slabs(B * T,
 * floats).  No atomics: the result depends on B * T and the inputs only. */
int wn_lc_upsample_floats(const int* scales, int m, int use_bias);
int wn_lc_upsample_fwd(const float* frames, int F, const int32_t* off,
                       const float* up, const int* scales, int m, int Lc,
                       int use_bias, float* rows, int ld_rows, int B, int T,
                       void* stream);
int wn_lc_upsample_bwd_slabs(long rows, int nacc);
int wn_lc_upsample_bwd(const float* frames, int F, const int32_t* off,
                       const float* up, const int* scales, int m, int Lc,
                       int use_bias, const float* drows, int ld_drows, int B,
                       int T, float* slabs, int num_slabs, long slab_stride,
                       void* stream);
/* bwd_ctx: wn_lc_upsample_bwd (the same slabs, bitwise) that also writes the
 * gradient at the upsampler's input, dframes [B][F][Lc]: per frame the sum
 * over its rows of the layer-0 input's gradient (its three taps).  Needs
 * every row's frame inside F ((T + hop - 2) / hop + 1 <= F, off[b] < hop).
 * dpart: num_slabs * 2 * Lc floats of per-workgroup parts (frames shared
 * between workgroups), added in workgroup order by a second launch; a frame
 * without rows gets zero.  No atomics. */
int wn_lc_upsample_bwd_ctx(const float* frames, int F, const int32_t* off,
                           const float* up, const int* scales, int m, int Lc,
                           int use_bias, const float* drows, int ld_drows,
                           int B, int T, float* slabs, int num_slabs,
                           long slab_stride, float* dframes, float* dpart,
                           void* stream);

/* ---- frame-context convolution in front of the upsampler (csrc/wn_lc.hip).
 * 0 <= p <= 8, 1 <= Lc <= 512; w [2p + 1][Lc][Lc] ([K][Cin][Cout]), no bias.
 * x [B][Fx][Lc]: frames staged with p frames of context either side, Fx >=
 * Fw + 2p.  fwd: ctx[b][f][j] = sum_{k, c} w[k][c][j] x[b][f + k][c] for
 * f < Fw, ctx [B][Fw][Lc]; an output's bits depend on x[b][f .. f + 2p] and w
 * only.  wgrad: dw[k][c][j] = sum_{b, f < Fw} x[b][f + k][c] dctx[b][f][j]:
 * slab s sums a fixed range of the B * Fw frames, [(2p + 1) Lc][Lc] floats
 * per slab (slab_stride >= that); sum them with wn_reduce_slabs.
 * num_slabs = wn_lc_context_wgrad_slabs(B * Fw, (2p + 1) * Lc * Lc). */
int wn_lc_context_fwd(const float* x, int Fx, const float* w, int p, int Lc,
                      float* ctx, int Fw, int B, void* stream);
int wn_lc_context_wgrad_slabs(long rows, int nacc);
int wn_lc_context_wgrad(const float* x, int Fx, const float* dctx, int Fw,
                        int p, int Lc, int B, float* slabs, int num_slabs,
                        long slab_stride, void* stream);

/* ---- log-mel front end (csrc/wn_features.hip): frame-rate local-conditioning
 * features from the audio, on the LC alignment -- frame f sits beside samples
 * f * hop .. f * hop + hop - 1 and is centred at c = f * hop + hop / 2:
 *   frame[j]  = x[c - n_fft / 2 + j] * window[j], j < n_fft; x = 0 outside [0, n[b])
 *   P[k]      = |DFT(frame)[k]|^2, k < n_bins = n_fft / 2 + 1
 *   out[f][m] = log(max(sum_k melw[m][k] P[k], floor))        (natural log)
 * audio float [B][ld] (ld >= T); lengths: device int32 [B] (n[b], clamped to
 * [0, T] by the kernel, read when it runs) or NULL (n[b] = T); out float
 * [B][F][n_mels], F = ceil(T / hop); frames f >= ceil(n[b] / hop) are written
 * as exact zeros.  Nothing at or behind n[b] is read.  The tables (device
 * float32, built by the host in float64: wavenet/features.py), NC =
 * ceil(n_bins / 32), MP = n_mels rounded up to 32:
 *   window [n_fft]
 *   basis  [NC][n_fft][64]: row j of chunk c holds cos(2 pi j k / n_fft) for
 *          the bins k = 32 c .. 32 c + 31, then sin(...) for the same bins;
 *          zeros for k >= n_bins
 *   melw   [32 NC][MP]: melw[k][m], the filterbank transposed, zero padded
 * n_fft a multiple of 64 in [64, 2048], 1 <= hop <= n_fft, 1 <= n_mels <= 128,
 * floor > 0, 1 <= B <= 65535, 1 <= T <= 2^30 (else WN_ERR_BAD_SHAPE); basis,
 * melw, out 16-byte, the others 4-byte aligned (else WN_ERR_MISALIGNED).  No
 * atomics, one summation order: a frame's bits depend on its own n_fft
 * samples and the tables only -- not on B, the other clips or its position.
 * One workgroup computes 32 consecutive frames.  The 31 hop + n_fft samples
 * they touch are staged on chip -- with one pad float after every `hop` of
 * them where hop is even -- when
 *   31 hop + n_fft + (hop even ? (31 hop + n_fft - 1) / hop : 0) + 1 <= 16384
 * floats; otherwise every sample is read from memory where it is used: the
 * same arithmetic, the same bits.  The launch asks for 64 KiB + 8 n_fft bytes
 * + the staged floats of dynamic LDS: 147296 bytes at most (n_fft 2048, hop
 * 460), 147280 at the largest odd hop (461). */
int wn_melspec(const float* audio, long ld, int B, int T, const int32_t* lengths,
               const float* window, const float* basis, const float* melw,
               int n_fft, int hop, int n_bins, int n_mels, float floor_,
               float* out, void* stream);

/* ---- feature normalisation (csrc/wn_features.hip; wavenet/features.py:
 * FeatureStats, Normalizer).  fr / in / out float32 [B][F][C]; nframes: device
 * int32 [B] (clip b has nframes[b] real frames, clamped to [0, F] by the
 * kernel, read when it runs) or NULL (all F frames are real).  Frames at or
 * behind nframes[b] are never read.
 *
 * wn_feature_stats ACCUMULATES INTO acc, float64 [2][C], over the real frames:
 *   acc[0][c] += sum x,   acc[1][c] += sum x * x     (x widened to float64)
 * partials: scratch of wn_feature_stats_partials_count() * 2 * C doubles (the
 * count is a constant).  The summation order, fixed: partial k sums the rows
 * [k per, min(B F, (k + 1) per)) of the B F rows, per = ceil(B F / count) -- a
 * function of (B, F, count) only.  Inside it the rows are dealt to G = 256 / L
 * row groups, L = the power of two next at or above ceil(C / V), at most 256,
 * V = 4 where C % 4 == 0 else 1; group g adds its rows lo + g, lo + g + G, ...
 * in ascending order, then the groups are added in the order g = 0, 1, ...;
 * at last the partials are added in the order k = 0, 1, ... starting from
 * zero, and that sum is added to acc.  No atomics: the result is a function of
 * the input's bits, (B, F, C), nframes and the previous acc, not of the device
 * or the launch.  The frame count is the host's sum of nframes.
 *
 * wn_feature_normalize: a real frame gets, in float32,
 *   v = (x - shift[c]) * scale[c]      (one subtraction, one multiplication)
 *   out = v < lo ? lo : (v > hi ? hi : v)                 (a NaN stays a NaN)
 * lo = -INFINITY, hi = +INFINITY: no clamp.  Frames f >= nframes[b] are
 * written as exact zeros whatever `in` held (wn_melspec's padding).  out may
 * be in.  16-byte loads and stores where C % 4 == 0, else a scalar path.
 *
 * 1 <= C <= 512, B, F >= 1, B * F <= 2^31 - 1, lo <= hi (else
 * WN_ERR_BAD_SHAPE); fr, in, out (and shift, scale) 16-byte aligned when
 * C % 4 == 0, else 4-byte; nframes 4-byte; acc, partials 8-byte (else
 * WN_ERR_MISALIGNED).  All checks come before any launch. */
int wn_feature_stats_partials_count(void);
int wn_feature_stats(const float* fr, int B, int F, int C, const int32_t* nframes,
                     double* acc, double* partials, void* stream);
int wn_feature_normalize(const float* in, float* out, int B, int F, int C,
                         const int32_t* nframes, const float* shift,
                         const float* scale, float lo, float hi, void* stream);

/* ---- distance of two feature tensors (csrc/wn_features.hip; wavenet/
 * features.py: frame_distance).  a, b float32 [B][F][C]; nframes as above
 * (frames at or behind nframes[b] are never read).  With d = a - b subtracted
 * in float32 and widened to float64, outputs float64 [B] each:
 *   abs_sum[b] = sum_{f,c} |d|
 *   sq_sum[b]  = sum_{f,c} d * d
 *   rms_sum[b] = sum_f sqrt((sum_c d * d) / C)          (float64 square root)
 * partials: scratch of wn_feature_distance_partials(B, F) doubles (3 per clip
 * and chunk of 64 frames; -1: bad arguments; needs no device).  The summation
 * order, fixed: the workgroup of chunk k of a clip gives its four waves the
 * frames 64 k + w, 64 k + w + 4, ... below nframes[b], in ascending order;
 * lane i of a wave adds the channels V i + 64 V j, j = 0, 1, ... (V = 4 where
 * C % 4 == 0, one 16-byte load per input, else 1) into its own sums; a
 * frame's sum over c is the xor butterfly (32, 16, ..., 1) of the lanes' sums
 * of that frame; the lanes' sums over the wave's frames go through the same
 * butterfly, the waves are added in the order 0, 1, 2, 3, the chunks in the
 * order k = 0, 1, ..., from zero.  No atomics: clip b's numbers are a function
 * of that clip's bits, (F, C) and nframes[b] -- not of B, the clip's position
 * or the other clips.  Equal inputs give exact zeros.
 *
 * 1 <= C <= 512, B, F >= 1, B * F <= 2^31 - 1 (else WN_ERR_BAD_SHAPE); a, b
 * 16-byte aligned when C % 4 == 0, else 4-byte; nframes 4-byte; the outputs
 * and partials 8-byte (else WN_ERR_MISALIGNED).  All checks come before any
 * launch. */
long wn_feature_distance_partials(int B, int F);
int wn_feature_distance(const float* a, const float* b, int B, int F, int C,
                        const int32_t* nframes, double* abs_sum, double* sq_sum,
                        double* rms_sum, double* partials, void* stream);

/* ---- pre-emphasis and de-emphasis (csrc/wn_features.hip; wavenet/
 * emphasis.py).  in / out: float32, clip b at in + b * ld_in / out + b * ld_out,
 * T samples each; lengths: device int32 [B] (clip b has lengths[b] real
 * samples, clamped to [0, T] by the kernel, read when it runs) or NULL (all T
 * are real).  Positions at or behind lengths[b] are never read and are
 * written as exact zeros.  alpha == 0 copies the real samples bit for bit.
 *
 * wn_preemphasis: out[b][t] = in[b][t] - float32(alpha * in[b][t - 1]) with
 * in[b][-1] = 0: one multiplication, one subtraction, two roundings, no FMA.
 * out must not overlap in (WN_ERR_UNSUPPORTED).
 *
 * wn_deemphasis: y[b][t] = in[b][t] + alpha * y[b][t - 1], y[b][-1] =
 * initial[b] (NULL: 0), as a blocked scan: one workgroup per clip walks it in
 * chunks of wn_emphasis_chunk() samples counted from the clip's first sample,
 * each lane runs 16 samples sequentially, the lanes' runs are joined by a
 * wave- and workgroup-level scan with the powers of alpha (computed in double,
 * rounded once) and the chunk's carry is kept in a register.  last (NULL: not
 * wanted): last[b] = y[b][lengths[b] - 1].  out may be in itself (with ld_out
 * == ld_in); any other overlap is WN_ERR_UNSUPPORTED.  No atomics: clip b's
 * output bits are a function of its own real samples, alpha and initial[b] --
 * not of B, T, the leading dimensions or the other clips.  Cutting a clip at
 * a multiple of wn_emphasis_chunk() and passing last as the next piece's
 * initial gives the bits of one call.
 *
 * B, T >= 1, ld_in, ld_out >= T, 0 <= alpha < 1 (else WN_ERR_BAD_SHAPE); every
 * pointer 4-byte aligned (else WN_ERR_MISALIGNED).  All checks come before
 * any launch; wn_emphasis_chunk needs no device. */
int wn_emphasis_chunk(void);
int wn_preemphasis(const float* in, float* out, long ld_in, long ld_out, int B,
                   int T, const int32_t* lengths, float alpha, void* stream);
int wn_deemphasis(const float* in, float* out, long ld_in, long ld_out, int B,
                  int T, const int32_t* lengths, const float* initial,
                  float* last, float alpha, void* stream);

/* ---- device-resident training corpus (csrc/wn_corpus.hip; the rule:
 * wavenet/corpus.py).  The trimmed utterances lie in one device buffer `flat`
 * [N] float32; utterance u is flat[utt_off[u] .. + utt_len[u]).  A batch is
 * cut by the kernel, which derives its plan from device tables and scalars
 * (the "plan" arguments, the same for both entries):
 *   utt_off int64 [U], utt_len int32 [U]
 *   item_utt, item_start int32 [P]: item i is a piece of utterance item_utt[i]
 *          that begins at item_start[i]
 *   perm int32 [nE][P]: the item orders of the epochs e0 .. e0 + nE - 1
 *   g0 = step * B: slot j < B is the global slot g = g0 + j of epoch g / P and
 *          takes the item perm[g / P - e0][g % P]; the epochs g0 / P ..
 *          (g0 + B - 1) / P must lie in [e0, e0 + nE) (else WN_ERR_BAD_SHAPE)
 *   size, random, seed: random == 0: n = utt_len - item_start, cut to `size`
 *          when size > 0; random != 0 (size >= 1): n = min(size, utt_len) and
 *          start = draw_bits(seed ^ 0x63726f70, g) % (utt_len - size + 1) when
 *          utt_len > size, else 0 (draw_bits: splitmix64(seed ^ splitmix64(c)))
 *   n is cut to T.
 * wn_corpus_gather: audio [B][T] float32, slot j = flat[utt_off + start .. + n)
 * and exact zeros behind n, whatever audio held.  Nothing outside
 * [utt_off + start, utt_off + start + n) is read; a table entry that points
 * outside its table or outside [0, N) makes its slot all zeros.
 * wn_corpus_gather_frames: the utterances' frame-rate features fr [NF] float32,
 * utterance u's frames [fr_len[u]][Lc] from frame fr_off[u] (int64 [U]) on,
 * frame f beside samples f * hop .. f * hop + hop - 1.  Either output may be
 * NULL, not both:
 *   frames [B][Fw][Lc]: row r = frame f_lo + r while that is < f_hi, else
 *          zeros; f_lo = max(0, start / hop - ctx), f_hi = min(fr_len,
 *          (start + n - 1) / hop + 1 + ctx).  Fw >= wn_corpus_window_frames
 *          (T, hop, ctx) = (T + hop - 2) / hop + 1 + 2 ctx covers every start.
 *   rows [B][T][Lc]: row t = frame (start + t) / hop, zeros for t >= n.
 * B, T, P, U, nE, N, NF >= 1, hop >= 1, ctx >= 0, Lc >= 1 (else
 * WN_ERR_BAD_SHAPE); flat, fr and the outputs 16-byte aligned, int64 tables
 * 8-byte, int32 tables 4-byte (else WN_ERR_MISALIGNED).  All checks come
 * before any launch; wn_corpus_window_frames needs no device (-1: bad
 * arguments).  Plain 16-byte stores; 16-byte loads where the source index
 * allows, scalar loads elsewhere; no atomics. */
long wn_corpus_window_frames(int T, int hop, int ctx);
int wn_corpus_gather(const float* flat, long N, const int64_t* utt_off,
                     const int32_t* utt_len, int U, const int32_t* item_utt,
                     const int32_t* item_start, int P, const int32_t* perm,
                     long e0, int nE, long g0, int size, int random,
                     uint64_t seed, float* audio, int B, int T, void* stream);
int wn_corpus_gather_frames(const float* fr, long NF, const int64_t* fr_off,
                            const int32_t* fr_len, const int64_t* utt_off,
                            const int32_t* utt_len, int U,
                            const int32_t* item_utt, const int32_t* item_start,
                            int P, const int32_t* perm, long e0, int nE,
                            long g0, int size, int random, uint64_t seed,
                            int hop, int ctx, int Lc, float* frames, int Fw,
                            float* rows, int B, int T, void* stream);
/* The two gathers with one more plan scalar, history >= 0 (else
 * WN_ERR_BAD_SHAPE): every slot brings up to `history` samples of its true
 * left context.  After start and n are derived as above, h = min(history,
 * start), start' = start - h, n' = n + h, n' is cut to T, and everything
 * said above holds with (start', n') for (start, n): the audio, the zeros
 * behind n', f_lo / f_hi / rows, the out-of-table rule.
 * wn_corpus_gather_hist also writes hist int32 [B] (h, cut to n') and lens
 * int32 [B] (n'; 0 for an empty slot) to device memory (both required, 4-byte
 * aligned), for a loss that reads them without a host round trip.
 * history == 0 gives the existing entries' output bits. */
int wn_corpus_gather_hist(const float* flat, long N, const int64_t* utt_off,
                          const int32_t* utt_len, int U,
                          const int32_t* item_utt, const int32_t* item_start,
                          int P, const int32_t* perm, long e0, int nE, long g0,
                          int size, int random, uint64_t seed, int history,
                          float* audio, int32_t* hist, int32_t* lens, int B,
                          int T, void* stream);
int wn_corpus_gather_frames_hist(const float* fr, long NF,
                                 const int64_t* fr_off, const int32_t* fr_len,
                                 const int64_t* utt_off,
                                 const int32_t* utt_len, int U,
                                 const int32_t* item_utt,
                                 const int32_t* item_start, int P,
                                 const int32_t* perm, long e0, int nE, long g0,
                                 int size, int random, uint64_t seed,
                                 int history, int hop, int ctx, int Lc,
                                 float* frames, int Fw, float* rows, int B,
                                 int T, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WAVENET_HIP_H_ */
