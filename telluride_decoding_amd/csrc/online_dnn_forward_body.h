    // The forward of one pass of a fully connected regressor: the layer-1 driver and the later-layers loop of
    // dnn_online_push_kernel (online_dnn.hip) and dnn_calib_push_kernel (online_dnn_calib.hip), stated once.  This is
    // a FRAGMENT of a kernel body, not a header: no include guard, no declarations of its own at file scope; each
    // kernel pulls it in with #include inside its pass loop, where the text stood.  A fragment and not a function
    // because, called as a __device__ __forceinline__ function, it changes dnn_online_push_kernel's register
    // allocation around layer 1 -- what a helper call cost there is DESIGN.md section 36 (4 to 5 %), the counts
    // that moved for this block are in section 47 -- while included as text that kernel compiles to the same code.
    //
    // It expects in scope:
    //   t                   the DnnNet (by reference), and derived from it  nl = t.nl, w1 = t.w[1], w1q = t.nj / 4,
    //                       nj = t.nj, ks = t.ks, lda_s = t.lda, k_all = t.w[0], chunk_floats = t.g ks nj
    //   prm, vec            the session's packed parameters; whether W1 takes 16-byte loads
    //   small               the staged small parameters (b1, W2, b2, ...), indexed by parameter offset
    //   tid                 threadIdx.x of kThreads
    //   c, pre, post, tl    the channels and the context, tl = pre + post rows of EEG tail
    //   ldr, pass           the staged rows' stride (row_stride(c)); the frames a pass holds at most
    //   a, nf               this pass emits the frames [a, a + nf)
    //   p, p0, p1           the kernel's params (p.eeg_ld, p.env_ld); this push is rows [p0, p1)
    //   eeg, env            the session's pushed rows;  tail, etail  its EEG and envelope tails in the state
    //   ws_s, rows_s, env_s, pred_s, act_s   the kernel's LDS areas (online_dnn_common.h's lds_bytes)
    // It stages the pass's rows and envelopes (rows_s, env_s) and leaves the pass's predictions in pred_s [nf],
    // behind a barrier.
    float4 regs[kLoads];
    chunk_load(prm, t, 0, vec, tid, regs);
    // ---- stage the EEG rows a - pre .. a + nf - 1 + post and the envelope rows a .. a + nf - 1
    stage_rows<kThreads>(rows_s, ldr, tail, tl, eeg, p.eeg_ld, c, a - pre, nf + tl, p0, p1);
    stage_env<kThreads>(env_s, etail, post, env, p.env_ld, a, nf, p0);
    chunk_store(ws_s, t, 0, tid, regs);
    __syncthreads();
    // ---- layer 1: thread = (frame f, column lane cg), frame-fastest; the thread owns the column groups cg,
    // cg + cl, ... (4 columns each, cl = kThreads / nf lanes), which share the frame's x.  Per slice a chain of
    // fused multiply-adds from 0.f over the slice's rows, added to the accumulators in slice order.
    const int cl = kThreads / nf, ng = (w1q + cl - 1) / cl;         // (nf <= 64, w1q <= 16: ng <= kPairs)
    const int pf = tid % nf, cg = tid / nf;
    const bool busy = cg < cl && cg * ng < w1q;
    // the thread's groups are cg ng .. cg ng + ng - 1; it reads the ng ADJACENT groups from jb on (one address and
    // constant offsets per row of W1), moved back where they would pass the last group: a group in front of its
    // own repeats a neighbour's sums and is dropped
    const int jb = busy ? (cg * ng < w1q - ng ? cg * ng : w1q - ng) : 0;
    bool own[kPairs];
    float z1[kPairs][4];
#pragma unroll
    for (int o = 0; o < kPairs; ++o) {
      own[o] = busy && o < ng && jb + o >= cg * ng;
      z1[o][0] = z1[o][1] = z1[o][2] = z1[o][3] = 0.f;
    }
    int lag0 = 0, ch0 = 0;                                          // the slice's first row is (lag0, ch0)
    for (int ci = 0; ci < t.nchunks; ++ci) {
      if (ci + 1 < t.nchunks) chunk_load(prm, t, ci + 1, vec, tid, regs);
      const float* buf = ws_s + (ci & 1) * chunk_floats;
      const int sl_end = (ci + 1) * t.g < t.nslices ? (ci + 1) * t.g : t.nslices;
      for (int sl = ci * t.g; sl < sl_end; ++sl) {
        const int kbase = sl * ks;
        const int ksl = k_all - kbase < ks ? k_all - kbase : ks;
        if (busy) {
          const float* xp = rows_s + (pf + lag0) * ldr + ch0;
          const float* wrow = buf + (size_t)(sl - ci * t.g) * ks * nj + 4 * jb;
          if (ng == 1) slice_fma<1>(xp, wrow, nj, ksl, ch0, c, ldr, z1);
          else if (ng == 2) slice_fma<2>(xp, wrow, nj, ksl, ch0, c, ldr, z1);
          else if (ng == 3) slice_fma<3>(xp, wrow, nj, ksl, ch0, c, ldr, z1);
          else slice_fma<4>(xp, wrow, nj, ksl, ch0, c, ldr, z1);
        }
        ch0 += ksl;
        while (ch0 >= c) { ch0 -= c; ++lag0; }
      }
      if (ci + 1 < t.nchunks) chunk_store(ws_s + ((ci + 1) & 1) * chunk_floats, t, ci + 1, tid, regs);
      __syncthreads();
    }
    // z1 = the partials + b1; ReLU when a layer follows, else (no hidden layer: w1 = 1) the prediction itself
#pragma unroll
    for (int o = 0; o < kPairs; ++o) {
      if (!own[o]) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 4 * (jb + o) + q;
        if (j >= w1) continue;
        const float z = z1[o][q] + small[t.off_b[0] + j];
        if (nl > 1) act_s[pf * lda_s + j] = z <= 0.f ? 0.f : z;
        else pred_s[pf] = z;
      }
    }
    __syncthreads();
    // ---- the later layers: (frame, unit) pairs over the workgroup, frame-fastest; the last layer's one unit is
    // the prediction
    for (int l = 2; l <= nl; ++l) {
      const int wi = t.w[l - 1], wo = t.w[l];
      const float* W = small + t.off_w[l - 1];
      const float* b = small + t.off_b[l - 1];
      const float* in = act_s + (size_t)(l & 1) * pass * lda_s;
      float* outp = act_s + (size_t)((l + 1) & 1) * pass * lda_s;
      for (int pr = tid; pr < nf * wo; pr += kThreads) {
        const int o = pr / nf, f = pr - o * nf;
        const float* xin = in + f * lda_s;
        float sum = 0.f;
        for (int i = 0; i < wi; ++i) sum = fmaf(xin[i], W[i * wo + o], sum);
        sum += b[o];
        if (l < nl) outp[f * lda_s + o] = sum <= 0.f ? 0.f : sum;
        else pred_s[f] = sum;
      }
      __syncthreads();
    }
