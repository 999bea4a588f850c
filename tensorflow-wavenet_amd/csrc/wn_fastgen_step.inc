// Bodies of fg_skip_kernel and fg_persist_kernel (FG_LC 0) and of their
// local-conditioning variants fg_skip_lc_kernel / fg_persist_lc_kernel (FG_LC 1),
// included twice by wn_fastgen.hip (FG_PART selects the kernel): the LC
// variants differ in the filter|gate bias of the next step's past-tap
// pre-activations only, and the plain kernels are compiled from the same text
// as before they had one.
#if FG_PART == 0
#if FG_LC
__global__ __launch_bounds__(256) void fg_skip_lc_kernel(FgStepLc lc_arg) {
  const FgStep& g = lc_arg.g;
#else
__global__ __launch_bounds__(256) void fg_skip_kernel(FgStep g) {
#endif
  __shared__ float zs[FG_MAXL * 32];
  __shared__ float red[FGM_PARTS][FGM_OUTS];
  const int nskip = (g.S + FGM_OUTS - 1) / FGM_OUTS;
  if ((int)blockIdx.x >= nskip) {        // workgroup-uniform
#if FG_LC
    fg_pre_layer<true>(g, lc_arg.ring, lc_arg.R, blockIdx.x - nskip, 1, zs);
#else
    fg_pre_layer<false>(g, nullptr, 0, blockIdx.x - nskip, 1, zs);
#endif
    return;
  }
  const int tid = threadIdx.x, o = tid & (FGM_OUTS - 1), part = tid / FGM_OUTS;
  const int s = blockIdx.x * FGM_OUTS + o;
  const int KK = g.L * 32;
  for (int i = tid; i < KK; i += 256) zs[i] = g.z_all[i];
  __syncthreads();
  red[part][o] = s < g.S ? fg_mv_partial<50>(zs, KK, g.skip_w, g.S, s, part) : 0.f;
  __syncthreads();
  if (part == 0 && s < g.S)
    g.h1[s] = fmaxf((g.skip_bsum ? g.skip_bsum[s] : 0.f) + fg_mv_reduce(red, o), 0.f);
}
#else
#if FG_LC
__global__ __launch_bounds__(FGP_THREADS) void fg_persist_lc_kernel(FgPersistLc lc_arg) {
  const FgPersist& a = lc_arg.a;
#else
__global__ __launch_bounds__(FGP_THREADS) void fg_persist_kernel(FgPersist a) {
#endif
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const FgStep& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = g.L, S = g.S, Q = g.Q, nseg = a.nseg, n_steps = a.n_steps;
  const int nsk = (S + 15) / 16, nlg = (Q + 15) / 16;
  const int base = g.ctl[FGCTL_BASE];
  unsigned* sync = a.sync;
  // hand-over words: z [L][32] | h1 [S] | h2 [S] | logits [Q] | x [nseg][32] | x0 [32]
  fgp_ll_t* zll = a.ll;
  fgp_ll_t* h1ll = zll + L * 32;
  fgp_ll_t* h2ll = h1ll + S;
  fgp_ll_t* lgll = h2ll + S;
  fgp_ll_t* xll = lgll + Q;
  fgp_ll_t* x0ll = xll + FGP_MAXSEG * 32;            // [32] the causal layer's output for the next step
  bool dead = false;
  // Role of this workgroup.  Workgroups go to the eight XCDs round-robin
  // (blockIdx % 8) and a hand-over word between two workgroups of ONE XCD costs
  // 0.59 - 0.64 us, between two XCDs 0.76 (tools/ubench/ll_hop.hip): the serial
  // chain's hand-overs -- draw -> segment 0 -> ... -> last segment -- stay on
  // one XCD: those nseg + 1 roles take the blocks 0, 8, 16, ..., the mat-vec
  // roles (skip | post1 | logits) the rest in order.  Roles are numbered
  // chain segments, skip, post1, logits, draw.
  int role = fgp_role_of_block((int)blockIdx.x, (int)gridDim.x, nseg);
#ifdef FGP_STAMPS
#define PSTAMP(slot) if (a.dbg && (tid & 63) == 0) a.dbg[(size_t)(slot)] = __builtin_amdgcn_s_memrealtime()
#else
#define PSTAMP(slot)
#endif

  if (role < nseg) {
    // ------------------------------------------------------------ chain segment
    const int seg = role;
    const int l0 = __builtin_amdgcn_readfirstlane((int)((long)seg * L / nseg));
    const int l1 = (int)((long)(seg + 1) * L / nseg);
    const int nl = __builtin_amdgcn_readfirstlane(l1 - l0);
    float* wres = lds;                                 // [nl][FGP_BLK]: weights | {pre, row, bd, -}
    int* meta = reinterpret_cast<int*>(wres + (size_t)nl * FGP_BLK);   // [nl] ring offset (rows), [nl] dilation
    int* flags = meta + 2 * FGP_SEGL;                  // [0] pre ready for step, [1] chain done with step
    // resident weights in LANE order: chunk c of the chain lane's row at float4
    // [c][lane] (filter | gate rows: c < 8; dense rows: [8 + cc][lane], lane =
    // 32 (c >> 2) + n), so a layer's reads are one lane address plus
    // immediates and conflict-free (the ring-slot image is [matrix][n][chunk ^ (n & 7)])
    for (int i = tid; i < nl * FGC_CW / 4; i += FGP_THREADS) {
      const int ll = i / (FGC_CW / 4), q = i % (FGC_CW / 4);
      const int m = q >> 8, n = (q >> 3) & 31, c = (q & 7) ^ (n & 7);
      const int dst = m < 2 ? c * 64 + m * 32 + n : 512 + (c & 3) * 64 + (c >> 2) * 32 + n;
      reinterpret_cast<f32x4*>(wres)[ll * (FGP_BLK / 4) + dst] =
          reinterpret_cast<const f32x4*>(g.cw_img + (size_t)l0 * FGC_CW)[i];
    }
    if (tid < nl) {
      int ro = 0;
      for (int q = 0; q < l0 + tid; ++q) ro += g.dil[q];
      meta[tid] = ro;
      meta[FGP_SEGL + tid] = g.dil[l0 + tid];
    }
    __syncthreads();
    for (int i = tid; i < nl * 64; i += FGP_THREADS) {
      const int ll = i >> 6, ln = i & 63;
      f32x4 ms;
      ms[0] = g.pre[(size_t)l0 * 64 + i];
      ms[1] = __int_as_float((meta[ll] + base % meta[FGP_SEGL + ll]) * 32);
      ms[2] = g.use_dense_bias
                  ? g.layer0[(size_t)(l0 + ll) * g.layer_stride + LAYER_OFF_BD + (ln & 31)] : 0.f;
      ms[3] = 0.f;
      reinterpret_cast<f32x4*>(wres)[ll * (FGP_BLK / 4) + 768 + ln] = ms;
    }
    if (tid == 0) { flags[0] = 1; flags[1] = 0; flags[2] = 0; flags[3] = 0; }
    __syncthreads();
    const int nn = lane & 31;
    if (wave == 0) {
      // ---- the serial chain of this segment (no workgroup barrier, weights
      // resident): fgp_chain_layers
      const int prev_code = g.cursors[1];
      fgp_ll_t* zrow = zll + l0 * 32 + nn;
      fgp_ll_t* xo = seg + 1 < nseg ? xll + seg * 32 : nullptr;
      for (int i = 0; i < n_steps; ++i) {
        const unsigned step = (unsigned)(i + 1);
        // this step's past-tap pre-activations are in LDS (helper waves): the
        // first layer's operands are requested before x is waited for
        while (!dead && __hip_atomic_load(flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < i + 1)
          __builtin_amdgcn_s_sleep(1);
        FgpLW wa;
        fgp_lw_load(wa, wres, 0, lane);
        float x = 0.f;
        if (seg == 0) {
          // (x lives in EVERY lane: channel lane & 31)
          if (i > 0) {
            // the draw workgroup's x0 of this step (fg_draw_wg256)
            x = fgp_get(x0ll + nn, (unsigned)i, sync, dead);
          } else {
            const int code = g.samples[0];
            float v = 0.f;
            if (prev_code >= 0 && prev_code < Q) v = g.causal[(long)prev_code * 32 + nn];
            if (code >= 0 && code < Q) v += g.causal[((long)Q + code) * 32 + nn];
            x = v;
          }
          PSTAMP(i * 16 + 0);
        } else {
          x = fgp_get(xll + (seg - 1) * 32 + nn, step, sync, dead);
        }
        PSTAMP(i * 16 + 1 + seg);
        if (nl == 10) x = fgp_chain_layers<10>(x, wres, wa, nl, l0, L, g.state, zrow, xo, step, lane);
        else x = fgp_chain_layers<0>(x, wres, wa, nl, l0, L, g.state, zrow, xo, step, lane);
        PSTAMP(i * 16 + 6 + seg);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0)
          __hip_atomic_store(flags + 1, i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    } else {
      // ---- helper waves: the NEXT step's past-tap pre-activations of this
      // segment's layers (model.py:335-338, the `state` half of the conv):
      // pre[l][n] = bias_fg[l][n] + sum_k x_l[t + 1 - d_l][k] * W[0][k][n],
      // one wave per layer, lane = output n (filter | gate); the queue entry
      // is read with device-scope loads after the chain wave's flag (its
      // write-through stores were acknowledged before it set the flag)
      const int hw = wave - 1;                          // 0..3
      for (int i = 0; i + 1 < n_steps; ++i) {
        while (!dead && __hip_atomic_load(flags + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < i + 1) {
          __builtin_amdgcn_s_sleep(4);
          if (__hip_atomic_load(sync + FGP_ERR, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) dead = true;
        }
        const int tpos = base + i + 1;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int ll = hw; ll < nl; ll += 4) {
          const int l = l0 + ll, d = meta[FGP_SEGL + ll];
          const float xv = lane < 32 ? fgp_ld(g.state + ((long)meta[ll] + tpos % d) * 32 + lane) : 0.f;
          const float* W = g.layer0 + (long)l * g.layer_stride + (lane < 32 ? 0 : 2 * 1024) + (lane & 31);
          float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            p0 = fmaf(__shfl(xv, k), W[k * 32], p0);
            p1 = fmaf(__shfl(xv, 8 + k), W[(8 + k) * 32], p1);
            p2 = fmaf(__shfl(xv, 16 + k), W[(16 + k) * 32], p2);
            p3 = fmaf(__shfl(xv, 24 + k), W[(24 + k) * 32], p3);
          }
#if FG_LC
          const float bias = lc_arg.ring[((long)(tpos % lc_arg.R) * L + l) * 64 + lane];
          acc[(ll - hw) >> 2] = bias + ((p0 + p1) + (p2 + p3));
#else
          acc[(ll - hw) >> 2] = (g.bias_fg ? g.bias_fg[l * 64 + lane] : 0.f) + ((p0 + p1) + (p2 + p3));
#endif
        }
        // (the chain wave is past this segment's layers of step i: the
        // {pre, row} words of the layers' blocks are free)
        for (int ll = hw; ll < nl; ll += 4) {
          float* ms = wres + (size_t)ll * FGP_BLK + 3072 + lane * 4;
          ms[0] = acc[(ll - hw) >> 2];
          ms[1] = __int_as_float((meta[ll] + tpos % meta[FGP_SEGL + ll]) * 32);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // four helper waves: the last one to finish raises the step
        if (lane == 0) {
          const int old = __hip_atomic_fetch_add(flags + 2, 1, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP);
          if (old == 3) {
            __hip_atomic_store(flags + 2, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_store(flags, i + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        }
      }
    }
    return;
  }
  role -= nseg;
  if (tid >= 256) return;          // the tail roles are 256-thread workgroups
  float* in_s = lds;               // staged input vector
  const int o = tid & 15, part = tid >> 4;
  if (role < nsk) {
    // ------------------------------------------------------------------- skip
    const int KK = L * 32, col0 = role * 16;
    float* w_s = lds + ((KK + 3) & ~3);               // [KK][16]
    float* red = w_s + (size_t)KK * 16;               // [16][16]
    for (int i = tid; i < KK * 16; i += 256) {
      const int k = i >> 4, c = i & 15;
      w_s[i] = col0 + c < S ? g.skip_w[(size_t)k * S + col0 + c] : 0.f;
    }
    __syncthreads();
    for (int i = 0; i < n_steps; ++i) {
      const unsigned step = (unsigned)(i + 1);
      float accv = 0.f;
      for (int sg = 0; sg < nseg; ++sg) {
        const int l0 = (int)((long)sg * L / nseg), l1 = (int)((long)(sg + 1) * L / nseg);
        const int n = (l1 - l0) * 32;
        fgp_get2(in_s + l0 * 32, zll + l0 * 32, tid, n, step, sync, dead);
        __syncthreads();
        accv += fgp_mv16(in_s + l0 * 32, w_s + (size_t)l0 * 32 * 16, n, o, part, 16);
      }
      red[part * 16 + o] = accv;
      __syncthreads();
      if (part == 0) {
        float t = 0.f;
#pragma unroll
        for (int p = 0; p < 16; ++p) t += red[p * 16 + o];
        if (col0 + o < S)
          fgp_put(h1ll + col0 + o, fmaxf((g.skip_bsum ? g.skip_bsum[col0 + o] : 0.f) + t, 0.f), step);
      }
      if (role == 0) { PSTAMP(i * 16 + 11); }
      __syncthreads();             // (red is rewritten in the next step)
    }
    return;
  }
  role -= nsk;
  if (role < nsk + nlg) {
    // ------------------------------------------------------- post1 / logits
    const bool lg = role >= nsk;
    fgp_post_role(lg ? g.post2_w : g.post1_w, lg ? g.post2_b : g.post1_b,
                  (lg ? role - nsk : role) * 16, lg ? Q : S, S, lg, lg ? h2ll : h1ll,
                  lg ? lgll : h2ll, n_steps, lds, sync, dead, tid,
                  a.dbg && role == 0 ? a.dbg + 12 : (a.dbg && role == nsk ? a.dbg + 13 : nullptr));
    return;
  }
  // ---------------------------------------------------------------------- draw
  // (256 threads: one logit per thread for Q <= 256)
  float* lgs = lds;                                             // [Q] the step's logits
  double* dpart = reinterpret_cast<double*>(lds + ((Q + 3) & ~3));  // 16 doubles: per-wave partials
  int* nxt = reinterpret_cast<int*>(dpart + 16);                 // [2] the code drawn at step parity
  float* ctab = reinterpret_cast<float*>(nxt + 8);               // [2][Q][32] the causal layer's filter
  double* wts = reinterpret_cast<double*>(ctab + 2 * Q * 32);    // [Q] the truncating draw's weights
  for (int i = tid; i < 2 * Q * 32; i += 256) ctab[i] = g.causal[i];
  const FgDrawCtl dc = fg_draw_ctl(g);
  __syncthreads();
  for (int i = 0; i < n_steps; ++i) {
    const unsigned step = (unsigned)(i + 1);
    fgp_get2(lgs, lgll, tid, Q, step, sync, dead);
    PSTAMP(i * 16 + 14);
    __syncthreads();
    // the code this step consumes (drawn / given one step ago: written behind
    // the previous step's last barrier, read behind this one)
    const int cur_code = i == 0 ? g.samples[0] : nxt[i & 1];
    // (dpart[] is rewritten a step later only after this barrier, which every
    // wave reaches after its last read of the step before)
    // the drawing thread publishes the code of step i + 1 for segment 0
    if (Q <= 256) fg_draw_wg256<1>(g, dc, lgs, dpart, wts, nxt, x0ll, ctab, cur_code, step, i + 1 < n_steps, tid, base + i);
    else fg_draw_wg256<2>(g, dc, lgs, dpart, wts, nxt, x0ll, ctab, cur_code, step, i + 1 < n_steps, tid, base + i);
    PSTAMP(i * 16 + 15);
  }
  __syncthreads();
  // the code the last step consumed (this CU's L1 may hold an older copy of the
  // samples line: the draws were kept in LDS)
  const int cur_code = n_steps >= 2 ? nxt[(n_steps - 1) & 1] : g.samples[0];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // cursors as wn_fastgen_finish leaves them: {steps done, the last code consumed, nothing pending}
  if (tid == 0) {
    g.cursors[0] = base + n_steps;
    g.cursors[1] = cur_code;
    g.cursors[2] = 0;
  }
#undef PSTAMP
}
#endif
