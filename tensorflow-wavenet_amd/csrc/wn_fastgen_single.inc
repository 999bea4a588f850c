// Body of fastgen_kernel (FG_LC 0) and fastgen_lc_kernel (FG_LC 1), included
// twice by wn_fastgen.hip: the LC variant differs in the filter|gate bias only,
// and fastgen_kernel is compiled from the same text as before it had one.
#if FG_LC
__global__ __launch_bounds__(FG_THREADS, 1) void fastgen_lc_kernel(FastGenLc lc_arg) {
  const FastGen& g = lc_arg.g;
#else
__global__ __launch_bounds__(FG_THREADS, 1) void fastgen_kernel(FastGen g) {
#endif
  __shared__ __attribute__((aligned(16))) float wring[2][FG_CW];
  __shared__ float zbuf[2][32];
  __shared__ float hbuf[FG_MAXS];     // relu(total)
  __shared__ float h2buf[FG_MAXS];    // relu(conv1)
  __shared__ float part[FG_MAXS];     // post2 partial sums
  __shared__ double pd[FG_MAXQ];
  __shared__ int s_code;
  __shared__ int pos[FG_MAXL];        // ring cursor of every layer
  __shared__ int sdil[FG_MAXL], roff[FG_MAXL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = g.S, Q = g.Q, L = g.L;
  const int st = tid - 64;            // loader-thread index 0..191 (waves 1..3)

  const int steps_done = g.cursors[0];
  int prev_code = g.cursors[1];
  if (tid == 0) s_code = g.samples[0];
  for (int l = tid; l < L; l += FG_THREADS) {
    sdil[l] = g.dil[l];
    pos[l] = steps_done % g.dil[l];
  }
  __syncthreads();
  if (tid == 0) {
    int off = 0;
    for (int l = 0; l < L; ++l) { roff[l] = off; off += sdil[l]; }
  }
  __syncthreads();

  for (int step = 0; step < g.n_steps; ++step) {
    const int code = s_code;
    const long tpos = (long)steps_done + step;
    // ---------------- loaders: chain-weight ring + skip columns ------------
    f32x4 cw[FG_LDR];
    auto cw_load = [&](int l) {        // global -> registers
      const f32x4* src = reinterpret_cast<const f32x4*>(
          g.layer0 + (long)l * g.layer_stride);
#pragma unroll
      for (int k = 0; k < FG_LDR; ++k) {
        const int i4 = st + FG_SKT * k;
        if (i4 < FG_CW4) cw[k] = src[i4];
      }
    };
    auto cw_store = [&](int buf) {     // registers -> LDS ring
      f32x4* dst = reinterpret_cast<f32x4*>(wring[buf]);
#pragma unroll
      for (int k = 0; k < FG_LDR; ++k) {
        const int i4 = st + FG_SKT * k;
        if (i4 < FG_CW4) dst[i4] = cw[k];
      }
    };
    float acc[FG_SKO], sw[FG_SKO][32];
    bool son[FG_SKO];
#pragma unroll
    for (int o = 0; o < FG_SKO; ++o) {
      acc[o] = 0.f;
      son[o] = wave >= 1 && st + FG_SKT * o < S;
    }
    auto skip_load = [&](int l) {
      const float* ws = g.skip_w + (long)l * 32 * S + st;
#pragma unroll
      for (int o = 0; o < FG_SKO; ++o)
        if (son[o]) {
#pragma unroll
          for (int k = 0; k < 32; ++k) sw[o][k] = ws[(long)k * S + FG_SKT * o];
        }
    };
    auto skip_fma = [&](const float* zl) {
#pragma unroll
      for (int o = 0; o < FG_SKO; ++o)
        if (son[o]) {
#pragma unroll
          for (int k = 0; k < 32; ++k) acc[o] = fmaf(zl[k], sw[o][k], acc[o]);
        }
    };
    // ---------------- chain state (wave 0) ---------------------------------
    float x = 0.f;                     // residual stream on lanes < 32
    float stv = 0.f, bias = 0.f, bdv = 0.f;  // prefetched for the coming layer
    auto chain_prefetch = [&](int l) {
#if FG_LC
      bias = lc_arg.ring[((tpos % lc_arg.R) * L + l) * 64 + lane];
#else
      bias = g.bias_fg ? g.bias_fg[l * 64 + lane] : 0.f;
#endif
      bdv = g.use_dense_bias
                ? g.layer0[(long)l * g.layer_stride + LAYER_OFF_BD + (lane & 31)]
                : 0.f;
      stv = lane < 32 ? g.state[((long)roff[l] + pos[l]) * 32 + lane] : 0.f;
    };
    // prologue: layer 0 weights into ring[0]
    if (wave >= 1) {
      cw_load(0);
      cw_store(0);
      if (L > 1) cw_load(1);
      skip_load(0);
    } else {
      chain_prefetch(0);
      if (lane < 32) {
        float v = 0.f;
        if (prev_code >= 0 && prev_code < Q) v = g.causal[(long)prev_code * 32 + lane];
        if (code >= 0 && code < Q) v += g.causal[((long)Q + code) * 32 + lane];
        x = v;
      }
    }
    __syncthreads();
    for (int l = 0; l <= L; ++l) {
      if (wave == 0) {
        if (l < L) {
          const float* wl = wring[l & 1];
          const float cur_st = stv, cur_bias = bias, cur_bd = bdv;
          if (g.push && lane < 32)       // enqueue x_l[t] (after the dequeue)
            g.state[((long)roff[l] + pos[l]) * 32 + lane] = x;
          if (l + 1 < L) chain_prefetch(l + 1);
          const float* wcol = wl + (lane < 32 ? 0 : 2048) + (lane & 31);
          float a = cur_bias;
#pragma unroll
          for (int k = 0; k < 32; ++k) {
            a = fmaf(readlane_f(cur_st, k), wcol[k * 32], a);      // W[0]
            a = fmaf(readlane_f(x, k), wcol[1024 + k * 32], a);    // W[1]
          }
          const float gate = __shfl(a, (lane & 31) + 32);
          const float z = wn_tanh(a) * wn_sigmoid(gate);  // valid on lanes < 32
          if (lane < 32) zbuf[l & 1][lane] = z;
          if (l + 1 < L) {
            float dsum = cur_bd;
            const float* wd = wl + 4096 + (lane & 31);
#pragma unroll
            for (int k = 0; k < 32; ++k) dsum = fmaf(readlane_f(z, k), wd[k * 32], dsum);
            if (lane < 32) x += dsum;
          }
        }
      } else {
        // ring slot (l+1)&1 was last read in iteration l-1: free to refill
        if (l + 1 < L) cw_store((l + 1) & 1);
        if (l + 2 < L) cw_load(l + 2);
        if (l >= 1) skip_fma(zbuf[(l - 1) & 1]);
        if (l >= 1 && l < L) skip_load(l);
      }
      // raw barrier: only LDS traffic is drained.  __syncthreads() would also
      // wait vmcnt(0), i.e. for the weight loads just issued for the NEXT
      // layers -- exposing a full L2 / Infinity-Cache round trip per layer.
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    // advance the ring cursors (after every wave is done with this step)
    if (g.push) {
      for (int l = tid; l < L; l += FG_THREADS) {
        const int p = pos[l] + 1;
        pos[l] = p == sdil[l] ? 0 : p;
      }
    }
    // ---------------- post-processing (model.py:505-514) -------------------
    if (wave >= 1) {
#pragma unroll
      for (int o = 0; o < FG_SKO; ++o)
        if (son[o]) {
          const int sc = st + FG_SKT * o;
          hbuf[sc] = fmaxf(acc[o] + (g.skip_bsum ? g.skip_bsum[sc] : 0.f), 0.f);
        }
    }
    __syncthreads();
    if (wave >= 1) {
      for (int s = st; s < S; s += FG_SKT) {
        float c0 = g.post1_b ? g.post1_b[s] : 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
        const float* w = g.post1_w + s;
        int k = 0;
        for (; k + 64 <= S; k += 64) {
          float wv[64];
#pragma unroll
          for (int u = 0; u < 64; ++u) wv[u] = w[(long)(k + u) * S];
#pragma unroll
          for (int u = 0; u < 64; u += 4) {
            c0 = fmaf(hbuf[k + u], wv[u], c0);
            c1 = fmaf(hbuf[k + u + 1], wv[u + 1], c1);
            c2 = fmaf(hbuf[k + u + 2], wv[u + 2], c2);
            c3 = fmaf(hbuf[k + u + 3], wv[u + 3], c3);
          }
        }
        for (; k < S; ++k) c0 = fmaf(hbuf[k], w[(long)k * S], c0);
        h2buf[s] = fmaxf((c0 + c1) + (c2 + c3), 0.f);
      }
    }
    __syncthreads();
    // logits: thread (q, part) sums a k-range; parts = 192 / Q
    {
      int parts = FG_SKT / Q;
      if (parts < 1) parts = 1;
      if (wave >= 1) {
        for (int o = st; o < Q * parts; o += FG_SKT) {
          const int q = o % Q, p = o / Q;
          const int k0 = (int)((long)S * p / parts), k1 = (int)((long)S * (p + 1) / parts);
          float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
          const float* w = g.post2_w + q;
          int k = k0;
          for (; k + 64 <= k1; k += 64) {
            float wv[64];
#pragma unroll
            for (int u = 0; u < 64; ++u) wv[u] = w[(long)(k + u) * Q];
#pragma unroll
            for (int u = 0; u < 64; u += 4) {
              c0 = fmaf(h2buf[k + u], wv[u], c0);
              c1 = fmaf(h2buf[k + u + 1], wv[u + 1], c1);
              c2 = fmaf(h2buf[k + u + 2], wv[u + 2], c2);
              c3 = fmaf(h2buf[k + u + 3], wv[u + 3], c3);
            }
          }
          for (; k < k1; ++k) c0 = fmaf(h2buf[k], w[(long)k * Q], c0);
          part[o] = (c0 + c1) + (c2 + c3);
        }
      }
      __syncthreads();
      for (int q = tid; q < Q; q += FG_THREADS) {
        float c = g.post2_b ? g.post2_b[q] : 0.f;
        for (int p = 0; p < parts; ++p) c += part[p * Q + q];
        pd[q] = (double)c;
      }
      __syncthreads();
    }
    // softmax in float64, optional temperature, draw (wn_common.h)
    if (wave == 0) {
      const bool want_p = g.proba_out && (step % g.proba_every == 0);
      wave_softmax_f64(pd, Q, lane, want_p ? g.proba_out + (long)(step / g.proba_every) * Q : nullptr);
    }
    __syncthreads();
    if (step + 1 >= g.n_given) {
      if (wave == 0) {
        const int best = wave_draw_f64(pd, Q, lane, g.temperature, g.top_k, g.top_p, g.seed, (uint64_t)tpos);
        if (lane == 0) {
          g.samples[step + 1] = best;
          s_code = best;
        }
      }
    } else if (tid == 0) {
      s_code = g.samples[step + 1];
    }
    prev_code = code;
    __syncthreads();
  }
  if (tid == 0 && g.push) {
    g.cursors[0] = steps_done + g.n_steps;
    g.cursors[1] = prev_code;
  }
}
