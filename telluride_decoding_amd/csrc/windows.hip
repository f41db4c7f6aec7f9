// Window half of the decode side: windowed correlation sums, per-window scores,
// class moments, the attended-speaker decisions and the fused decode.  The prediction is decode.hip.
#include "decode_common.h"

namespace {

// ---------------------------------------------------------------- window sums
struct WinDesc {
  long long row0;   // global first row of the window
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One workgroup per window; 5 float64 sums per column, fixed reduction tree
// (bitwise reproducible).
__global__ __launch_bounds__(kThreads) void window_sums_kernel(
    const float* __restrict__ a, long long lda, const float* __restrict__ b, long long ldb,
    int cols, const long long* __restrict__ win_row0, int width, double* __restrict__ out) {
  __shared__ double red[4][5];
  const long long r0 = win_row0[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int col = 0; col < cols; ++col) {
    double s[5] = {0, 0, 0, 0, 0};
    for (int r = tid; r < width; r += kThreads) {
      const double av = (double)a[(r0 + r) * lda + col];
      const double bv = (double)b[(r0 + r) * ldb + col];
      s[0] += av; s[1] += bv; s[2] += av * av; s[3] += bv * bv; s[4] += av * bv;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double v = wave_sum(s[k]);
      if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid < 5)
      out[((long long)blockIdx.x * cols + col) * 5 + tid] =
          (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    __syncthreads();
  }
}

// Short windows that share no whole blocks (the reference harness' W = 10 frames every 5,
// infer.py:376-378: hundreds of thousands of windows of a few frames): one THREAD per window
// and column, frames summed in ascending order; the window's first row comes from the per-trial
// descriptor (first = first window of the trial), so nothing per window is uploaded.  (One
// 256-thread workgroup per window and a host-built table of 240 k start rows took 0.63 ms per
// stream at C4.)
__global__ void window_sums_short_kernel(const float* __restrict__ a, long long lda,
                                         const float* __restrict__ b, long long ldb, int cols,
                                         const FileDesc* __restrict__ trials, int n_trials,
                                         long long n_win, int width, int hop,
                                         double* __restrict__ out) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= n_win * cols) return;
  const long long w = i / cols;
  const int col = (int)(i % cols);
  const FileDesc tr = trials[find_file(trials, n_trials, w)];
  const long long r0 = tr.row0 + (w - tr.first) * hop;
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  for (int r = 0; r < width; ++r) {
    const double av = (double)a[(r0 + r) * lda + col];
    const double bv = (double)b[(r0 + r) * ldb + col];
    s0 += av; s1 += bv; s2 += av * av; s3 += bv * bv; s4 += av * bv;
  }
  double* o = out + i * 5;
  o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3; o[4] = s4;
}

// ---- two-stage window sums: block partials, then windows from blocks ---------
// Overlapping windows share frames (width / hop = 10 at C4): with g = gcd(width,
// hop) every window is a run of width / g whole blocks of g frames, so the frames
// are read ONCE into per-block float64 partial sums and a window is the sum of its
// blocks in ascending order.  A block belongs to 16 lanes (4 blocks per wave): lane-
// strided accumulation, then a fixed 4-step shuffle tree -- bitwise reproducible, and the
// same order in both kernels below (the fused decode is tested bit-for-bit against the
// unfused chain).  One wave per block spent most of its time in 6-step float64 shuffle
// trees for 2 rounds of loads (22 us at C4; 16 lanes per block: 8 us).
constexpr int kBlockLanes = 16;

// The tree v += v[lane ^ 8], ^ 4, ^ 2, ^ 1 within each group of 16 lanes, every lane ending with the
// total -- as DPP row rotations instead of ds_bpermute shuffles: after the ^ 8 step the values repeat
// every 8 lanes, so lane (i + 4) mod 16 holds what lane i ^ 4 holds, and so on down: the same operand
// pairs, the same bits, no LDS crossbar (40 ds_bpermute per pass of blocks made the per-trial kernel
// LDS-bound at short blocks: 50 us at W = 10 / hop 5).
template <int kCtrl>
__device__ __forceinline__ double dpp_row_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kCtrl, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kCtrl, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double group16_sum(double v) {
  static_assert(kBlockLanes == 16, "a DPP row is 16 lanes");
  v += dpp_row_f64<0x128>(v);     // row_ror:8
  v += dpp_row_f64<0x124>(v);     // row_ror:4
  v += dpp_row_f64<0x122>(v);     // row_ror:2
  v += dpp_row_f64<0x121>(v);     // row_ror:1
  return v;
}

__global__ __launch_bounds__(kThreads) void block_sums_kernel(
    const float* __restrict__ a, long long lda, const float* __restrict__ b, long long ldb,
    int cols, int b_cols, const FileDesc* __restrict__ trials, int n_trials, long long n_blocks,
    int g, double* __restrict__ out) {
  const int sub = threadIdx.x & (kBlockLanes - 1);
  const long long blk = blockIdx.x * (long long)(kThreads / kBlockLanes) + threadIdx.x / kBlockLanes;
  const bool live = blk < n_blocks;                 // dead groups stay for the shuffles
  const long long bq = live ? blk : n_blocks - 1;
  const FileDesc tr = trials[find_file(trials, n_trials, bq)];
  const long long r0 = tr.row0 + (bq - tr.first) * g;
  // (blockIdx.y deals the columns out: 20 models x 31 blocks of a held-out recording were 8
  // workgroups walking 20 columns each, 69 us)
  for (int col = blockIdx.y; col < cols; col += gridDim.y) {
    const int bc = col % b_cols;
    double s[5] = {0, 0, 0, 0, 0};
    for (int r = sub; r < g; r += kBlockLanes) {
      const double av = (double)a[(r0 + r) * lda + col];
      const double bv = (double)b[(r0 + r) * ldb + bc];
      s[0] += av; s[1] += bv; s[2] += av * av; s[3] += bv * bv; s[4] += av * bv;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double v = group16_sum(s[k]);
      if (sub == 0 && live) out[(blk * cols + col) * 5 + k] = v;
    }
  }
}

// Many columns (the 20 lambdas of a sweep's held-out evaluation, regression.py:197-214): a lane is a COLUMN,
// a wave step reads 64 / cols whole rows of both arrays -- contiguous -- where the kernel above gives every
// column a pass of its own over lines it shares with the other columns (20 columns: 20 x the L2 traffic,
// 290 us for 1e6 rows).  One wave per block, its row phases summed through LDS in a fixed order.
__global__ __launch_bounds__(kThreads) void block_sums_cols_kernel(
    const float* __restrict__ a, long long lda, const float* __restrict__ b, long long ldb,
    int cols, int b_cols, const FileDesc* __restrict__ trials, int n_trials, long long n_blocks,
    int g, double* __restrict__ out) {
  __shared__ double part[kThreads / 64][64][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long blk = blockIdx.x * (long long)(kThreads / 64) + wave;
  if (blk >= n_blocks) return;                          // (wave-uniform; no workgroup barrier below)
  const FileDesc tr = trials[find_file(trials, n_trials, blk)];
  const long long r0 = tr.row0 + (blk - tr.first) * g;
  const int per = 64 / cols;                            // rows per wave step (cols <= 64)
  const int col = lane % cols, rs = lane / cols;
  const int bc = col % b_cols;                          // (b may have fewer columns: cycled, like block_sums_kernel)
  double s[5] = {0, 0, 0, 0, 0};
  if (rs < per) {
    int r = rs;
    for (; r + 3 * per < g; r += 4 * per) {             // four loads of each array in flight
      float av[4], bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        av[q] = a[(r0 + r + q * per) * lda + col];
        bv[q] = b[(r0 + r + q * per) * ldb + bc];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double x = (double)av[q], y = (double)bv[q];
        s[0] += x; s[1] += y; s[2] += x * x; s[3] += y * y; s[4] += x * y;
      }
    }
    for (; r < g; r += per) {
      const double x = (double)a[(r0 + r) * lda + col], y = (double)b[(r0 + r) * ldb + bc];
      s[0] += x; s[1] += y; s[2] += x * x; s[3] += y * y; s[4] += x * y;
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) part[wave][lane][k] = s[k];
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);                   // lgkmcnt(0): the wave's own LDS writes
  if (rs == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      double v = s[k];
      for (int q = 1; q < per; ++q) v += part[wave][q * cols + col][k];
      out[(blk * cols + col) * 5 + k] = v;
    }
  }
}

// The fused decode's shape: two truth columns (the speakers' envelopes) against ONE shared
// prediction column -- every frame is loaded once and 8 sums instead of 10 go through the tree.
__global__ __launch_bounds__(kThreads) void block_sums_pair_kernel(
    const float* __restrict__ a, long long lda, const float* __restrict__ b,
    const FileDesc* __restrict__ trials, int n_trials, long long n_blocks, int g,
    double* __restrict__ out) {
  const int sub = threadIdx.x & (kBlockLanes - 1);
  const long long blk = blockIdx.x * (long long)(kThreads / kBlockLanes) + threadIdx.x / kBlockLanes;
  const bool live = blk < n_blocks;
  const long long bq = live ? blk : n_blocks - 1;
  const FileDesc tr = trials[find_file(trials, n_trials, bq)];
  const long long r0 = tr.row0 + (bq - tr.first) * g;
  double sa0 = 0, sa1 = 0, sb = 0, qa0 = 0, qa1 = 0, qb = 0, p0 = 0, p1 = 0;
  for (int r = sub; r < g; r += kBlockLanes) {
    const double a0 = (double)a[(r0 + r) * lda], a1 = (double)a[(r0 + r) * lda + 1];
    const double bv = (double)b[r0 + r];
    sa0 += a0; sa1 += a1; sb += bv;
    qa0 += a0 * a0; qa1 += a1 * a1; qb += bv * bv;
    p0 += a0 * bv; p1 += a1 * bv;
  }
  sa0 = group16_sum(sa0); sa1 = group16_sum(sa1); sb = group16_sum(sb);
  qa0 = group16_sum(qa0); qa1 = group16_sum(qa1); qb = group16_sum(qb);
  p0 = group16_sum(p0); p1 = group16_sum(p1);
  if (sub == 0 && live) {
    double* o = out + blk * 10;
    o[0] = sa0; o[1] = sb; o[2] = qa0; o[3] = qb; o[4] = p0;
    o[5] = sa1; o[6] = sb; o[7] = qa1; o[8] = qb; o[9] = p1;
  }
}

// Window w of trial t (FileDesc: first = first WINDOW of the trial, out0 = first
// BLOCK of the trial) starts at block out0 + (w - first) * blocks_per_hop.
__device__ __forceinline__ long long window_first_block(const FileDesc* __restrict__ trials,
                                                        int n_trials, long long w,
                                                        int blocks_per_hop) {
  const FileDesc tr = trials[find_file(trials, n_trials, w)];
  return tr.out0 + (w - tr.first) * blocks_per_hop;
}

__global__ void window_from_blocks_kernel(const double* __restrict__ bsums,
                                          const FileDesc* __restrict__ trials, int n_trials,
                                          long long n_win, int cols, int blocks_per_win,
                                          int blocks_per_hop, double* __restrict__ out) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= n_win * cols * 5) return;
  const long long w = i / (cols * 5);
  const int ck = (int)(i % (cols * 5));
  const double* p = bsums + window_first_block(trials, n_trials, w, blocks_per_hop) * cols * 5 + ck;
  double s = 0.0;
  for (int j = 0; j < blocks_per_win; ++j) s += p[(long long)j * cols * 5];
  out[i] = s;
}

// The same for long windows (whole-recording statistics: thousands of blocks per window): one
// wave per output, lane-strided partial sums and a fixed shuffle tree instead of one thread
// walking all the blocks (0.56 ms for a 1.2 M-frame window).
__global__ __launch_bounds__(256) void window_from_blocks_wide_kernel(
    const double* __restrict__ bsums, const FileDesc* __restrict__ trials, int n_trials,
    long long n_win, int cols, int blocks_per_win, int blocks_per_hop, double* __restrict__ out) {
  const long long i = blockIdx.x * 4LL + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n_win * cols * 5) return;
  const long long w = i / (cols * 5);
  const int ck = (int)(i % (cols * 5));
  const double* p = bsums + window_first_block(trials, n_trials, w, blocks_per_hop) * cols * 5 + ck;
  double s = 0.0;
  for (int j = lane; j < blocks_per_win; j += 64) s += p[(long long)j * cols * 5];
  s = wave_sum(s);
  if (lane == 0) out[i] = s;
}

// Fused tail of the two-speaker decode: window sums from block partials (column
// spk = envelope of speaker spk vs the shared prediction), global-statistics
// correlation score per speaker (infer_decoder.py:326-328 averaged over the
// window, infer.py:263-265) and the winner-take-all decision
// (attention_decoder.py:128-134: strict >).
struct FusedCorr {
  double mean_a[2], mean_b[2], power[2];
};

__global__ void decode_finalize_kernel(const double* __restrict__ bsums,
                                       const FileDesc* __restrict__ trials, int n_trials,
                                       long long n_win, int blocks_per_win, int blocks_per_hop,
                                       int width, FusedCorr fc,
                                       double* __restrict__ scores,
                                       unsigned char* __restrict__ decisions) {
  const long long w = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (w >= n_win) return;
  const double n = (double)width;
  const long long blk0 = window_first_block(trials, n_trials, w, blocks_per_hop);
  double sc[2];
#pragma unroll
  for (int spk = 0; spk < 2; ++spk) {
    const double* p = bsums + (blk0 * 2 + spk) * 5;
    double sa = 0.0, sb = 0.0, sab = 0.0;
    for (int j = 0; j < blocks_per_win; ++j) {
      sa += p[(long long)j * 10 + 0];
      sb += p[(long long)j * 10 + 1];
      sab += p[(long long)j * 10 + 4];
    }
    const double num = sab - fc.mean_a[spk] * sb - fc.mean_b[spk] * sa +
                       n * fc.mean_a[spk] * fc.mean_b[spk];
    sc[spk] = num / (fc.power[spk] * n);
  }
  scores[w * 2 + 0] = sc[0];
  scores[w * 2 + 1] = sc[1];
  decisions[w] = sc[0] > sc[1] ? 1 : 0;
}

// The same tail when every trial is short enough for ONE workgroup (C4: 200 trials of 6000
// frames): windows never span trials, so a workgroup forms its trial's block sums in LDS -- 64
// groups of 16 lanes, the arithmetic and summation order of block_sums_pair_kernel -- and then
// its windows, scores and decisions from them (order of decode_finalize_kernel): one launch
// instead of two latency-bound ones and no round trip of the block sums through HBM (10 + 8 us
// and a gap at C4 -> 6 us).  Bit-identical to the two-kernel path.
// Descriptor: row0 = first frame of the trial, nrows = its blocks, out0 = its windows,
// first = index of its first window.
constexpr int kTrialThreads = 1024;
constexpr int kTrialBlocksMax = 1536;    // 5 float64 per block in LDS: 60 KB

__global__ __launch_bounds__(kTrialThreads) void decode_trial_kernel(
    const float* __restrict__ a, long long lda, const float* __restrict__ b,
    const FileDesc* __restrict__ trials, int g, int blocks_per_win, int blocks_per_hop, int width,
    FusedCorr fc, double* __restrict__ scores, unsigned char* __restrict__ decisions,
    long long u_stride, FileDesc u0) {
  extern __shared__ double tb_sums[];     // [block][5]: sum a0, sum a1, sum b, sum a0 b, sum a1 b
  // (u_stride > 0: trials of one length, one after the other -- trial t's descriptor follows from
  // trial 0's, a kernel argument: no table read per workgroup in front of everything else)
  FileDesc tr;
  if (u_stride > 0) {
    tr = u0;
    tr.row0 += blockIdx.x * u_stride;
    tr.first = blockIdx.x * tr.out0;
  } else {
    tr = trials[blockIdx.x];
  }
  const int n_blocks = (int)tr.nrows, n_win = (int)tr.out0;
  const int sub = threadIdx.x & (kBlockLanes - 1), grp = threadIdx.x / kBlockLanes;
  constexpr int kGroups = kTrialThreads / kBlockLanes;
  // Short blocks (a row per lane at most: windows of a few frames, e.g. W = 10 / hop 5 -> 1200 blocks
  // of 5 frames per minute): eight passes of blocks at a time, their loads issued together -- one
  // memory latency per eight passes instead of one per pass.  The same sums in the same order.
  int base0 = 0;
  if (g <= kBlockLanes) {
    for (; base0 + 8 * kGroups <= n_blocks + 7 * kGroups && base0 < n_blocks; base0 += 8 * kGroups) {
      float va0[8], va1[8], vb[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int blk = base0 + u * kGroups + grp;
        const long long rr = tr.row0 + (long long)(blk < n_blocks ? blk : n_blocks - 1) * g + (sub < g ? sub : 0);
        va0[u] = a[rr * lda]; va1[u] = a[rr * lda + 1]; vb[u] = b[rr];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int blk = base0 + u * kGroups + grp;
        const bool live = blk < n_blocks;
        double sa0 = 0, sa1 = 0, sb = 0, p0 = 0, p1 = 0;
        if (sub < g) {
          const double a0 = (double)va0[u], a1 = (double)va1[u], bv = (double)vb[u];
          sa0 += a0; sa1 += a1; sb += bv;
          p0 += a0 * bv; p1 += a1 * bv;
        }
        sa0 = group16_sum(sa0); sa1 = group16_sum(sa1); sb = group16_sum(sb);
        p0 = group16_sum(p0); p1 = group16_sum(p1);
        if (sub == 0 && live) {
          double* o = tb_sums + blk * 5;
          o[0] = sa0; o[1] = sa1; o[2] = sb; o[3] = p0; o[4] = p1;
        }
      }
    }
  }
  for (int base = base0; base < n_blocks; base += kGroups) {
    const int blk = base + grp;
    const bool live = blk < n_blocks;               // dead groups stay for the shuffles
    const long long r0 = tr.row0 + (long long)(live ? blk : n_blocks - 1) * g;
    double sa0 = 0, sa1 = 0, sb = 0, p0 = 0, p1 = 0;
    // eight rows per lane at a time, every load issued before the first sum (a rolled loop waits out one
    // memory latency per row: 7 in a row at g = 100, most of this kernel's 9 us); same order of sums
    for (int rb = sub; rb < g; rb += 8 * kBlockLanes) {
      float va0[8], va1[8], vb[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int r = rb + i * kBlockLanes;
        const long long rr = r0 + (r < g ? r : sub);
        va0[i] = a[rr * lda]; va1[i] = a[rr * lda + 1]; vb[i] = b[rr];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (rb + i * kBlockLanes < g) {
          const double a0 = (double)va0[i], a1 = (double)va1[i], bv = (double)vb[i];
          sa0 += a0; sa1 += a1; sb += bv;
          p0 += a0 * bv; p1 += a1 * bv;
        }
      }
    }
    sa0 = group16_sum(sa0); sa1 = group16_sum(sa1); sb = group16_sum(sb);
    p0 = group16_sum(p0); p1 = group16_sum(p1);
    if (sub == 0 && live) {
      double* o = tb_sums + blk * 5;
      o[0] = sa0; o[1] = sa1; o[2] = sb; o[3] = p0; o[4] = p1;
    }
  }
  __syncthreads();
  const double n = (double)width;
  for (int w = threadIdx.x; w < n_win; w += kTrialThreads) {
    const double* p = tb_sums + (size_t)w * blocks_per_hop * 5;
    double sc[2];
#pragma unroll
    for (int spk = 0; spk < 2; ++spk) {
      double sa = 0.0, sb = 0.0, sab = 0.0;
      for (int j = 0; j < blocks_per_win; ++j) {
        sa += p[j * 5 + spk];
        sb += p[j * 5 + 2];
        sab += p[j * 5 + 3 + spk];
      }
      const double num = sab - fc.mean_a[spk] * sb - fc.mean_b[spk] * sa +
                         n * fc.mean_a[spk] * fc.mean_b[spk];
      sc[spk] = num / (fc.power[spk] * n);
    }
    const long long wi = tr.first + w;
    scores[wi * 2 + 0] = sc[0];
    scores[wi * 2 + 1] = sc[1];
    decisions[wi] = sc[0] > sc[1] ? 1 : 0;
  }
}

__global__ __launch_bounds__(kThreads) void window_means_kernel(
    const double* __restrict__ v, const long long* __restrict__ win_row0, int width,
    double* __restrict__ out) {
  __shared__ double red[4];
  const long long r0 = win_row0[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s = 0.0;
  for (int r = tid; r < width; r += kThreads) s += v[r0 + r];
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) out[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) / (double)width;
}

// Per-column statistics live in a device table (td_table_upload: cached by content), so the
// number of columns is unlimited (the reference has no limit either, brain_model.py:34-79).
struct ScoreParams {
  const double* mean_a; const double* mean_b; const double* power; const double* lda_w;  // [cols]
  double lda_slope, lda_intercept;
};

// "Constant column" test of the Pearson zero rule (brain_model.py:72-79: all zeros if the
// centred sum of squares of ANY column is <= 0).  The reference centres in float32, where a
// constant column gives exactly 0; from raw float64 sums the same column leaves a rounding
// residue of either sign, so anything within 32 eps of the raw sum of squares counts as zero.
__device__ __forceinline__ bool no_variance(double var, double sum_sq) {
  return var <= 32.0 * 2.220446049250313e-16 * sum_sq;
}

// mode 0: mean over the window of (a-ma)(b-mb)/power per column, reduced across
// columns; mode 1: per-window Pearson per column with the reference's "any
// constant column zeroes everything" rule (brain_model.py:72-79).
__global__ void window_scores_kernel(const double* __restrict__ sums, long long n_win, int cols,
                                     int width, int mode, int reduction, int group,
                                     ScoreParams sp, double* __restrict__ scores) {
  const long long w = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (w >= n_win) return;
  const double* s = sums + w * cols * 5;
  const double n = (double)width;
  if (mode == 0) {
    double acc = 0.0;
    const int c_lo = reduction == 1 ? 1 : 0;
    const int c_hi = reduction == 2 ? cols : c_lo + 1;
    for (int c = c_lo; c < c_hi; ++c) {
      const double sa = s[c * 5 + 0], sb = s[c * 5 + 1], sab = s[c * 5 + 4];
      // sum (a-ma)(b-mb) = sab - ma*sb - mb*sa + n*ma*mb
      const double num = sab - sp.mean_a[c] * sb - sp.mean_b[c] * sa + n * sp.mean_a[c] * sp.mean_b[c];
      acc += num / (sp.power[c] * n);
    }
    scores[w] = acc / (double)(c_hi - c_lo);
  } else {
    // the zero rule is per MODEL: columns [g0, g0 + group) are the outputs of one model (one
    // pearson_correlation call in the reference); group == cols is a single model
    for (int g0 = 0; g0 < cols; g0 += group) {
      const int g1 = min(g0 + group, cols);
      bool zero = false;
      for (int c = g0; c < g1; ++c) {
        const double sa = s[c * 5 + 0], sb = s[c * 5 + 1];
        zero = zero || no_variance(s[c * 5 + 2] - sa * sa / n, s[c * 5 + 2]) ||
               no_variance(s[c * 5 + 3] - sb * sb / n, s[c * 5 + 3]);
      }
      for (int c = g0; c < g1; ++c) {
        const double sa = s[c * 5 + 0], sb = s[c * 5 + 1];
        const double va = s[c * 5 + 2] - sa * sa / n, vb = s[c * 5 + 3] - sb * sb / n;
        const double cov = s[c * 5 + 4] - sa * sb / n;
        scores[w * cols + c] = zero ? 0.0 : cov / (sqrt(va) * sqrt(vb));
      }
    }
  }
}

// Per-frame reduced score (Decoder.infer_one, infer_decoder.py:439-455), formed
// in float64 from the float32 inputs (the reference rounds each step to float32;
// this is the same value to ~1e-7 relative).
__global__ void frame_scores_kernel(const float* __restrict__ a, long long lda,
                                    const float* __restrict__ b, long long ldb, int cols,
                                    long long rows, int reduction, ScoreParams sp,
                                    double* __restrict__ out) {
  for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < rows;
       r += (long long)gridDim.x * blockDim.x) {
    double acc = 0.0;
    if (reduction == 5) {   // 'all': every column, out is [rows, cols]
      for (int c = 0; c < cols; ++c)
        out[r * cols + c] = ((double)a[r * lda + c] - sp.mean_a[c]) *
                            ((double)b[r * ldb + c] - sp.mean_b[c]) / sp.power[c];
      continue;
    }
    if (reduction == 0 || reduction == 1) {
      const int c = reduction;
      acc = ((double)a[r * lda + c] - sp.mean_a[c]) * ((double)b[r * ldb + c] - sp.mean_b[c]) /
            sp.power[c];
    } else {
      for (int c = 0; c < cols; ++c) {
        const double v = ((double)a[r * lda + c] - sp.mean_a[c]) *
                         ((double)b[r * ldb + c] - sp.mean_b[c]) / sp.power[c];
        if (reduction == 2) acc += v;
        else if (reduction == 3) acc += (v > 0.0 ? v * v : (v < 0.0 ? -v * v : 0.0));
        else acc += v * sp.lda_w[c];
      }
      if (reduction == 2 || reduction == 3) acc /= (double)cols;
      else acc = sp.lda_slope * acc + sp.lda_intercept;
    }
    out[r] = acc;
  }
}

// ---------------------------------------------------------------- windowed class moments
// Decoder.train with a window (infer_decoder.py:330-400, average_data :748-783): the per-frame value
// of frame_scores_kernel's 'all' branch, its means over consecutive windows of `width` frames, and
// the moments [[M^T M, sum m], [sum m^T, n_win]] of those means that the LDA's scatter matrices are
// made of -- the frames are read once and nothing per frame is written.
// A lane is a COLUMN (block_sums_cols_kernel's layout): lane = rs * cols + col reads rows rs,
// rs + per, ... of its window (per = 64 / cols rows per wave step, contiguous when the stream is
// dense) and sums them in that order; the per row phases of a column are then summed in ascending
// order through LDS.  A wave owns win_per_wave consecutive windows and adds m_i m_j of each, in window
// order, to its own (cols + 1)^2 tile in LDS; the four tiles of a workgroup are summed pairwise in a
// fixed order into the workgroup's partial.  Which wave sees which window follows from (rows, width)
// alone, and nothing is atomic: the same bits on every call, whatever the CU count.
constexpr int kWcmMaxCols = 32;
constexpr int kWcmEntMax = (kWcmMaxCols + 1) * (kWcmMaxCols + 1);
constexpr int kWcmWaves = kThreads / 64;
constexpr int kWcmMinWinPerWave = 4;
constexpr int kWcmMaxGroups = 1024;     // partials: at most 1024 x 33^2 float64 (8.9 MB of scratch)

__global__ __launch_bounds__(kThreads) void window_class_moments_kernel(
    const float* __restrict__ a, long long lda, const float* __restrict__ b, long long ldb, int cols,
    long long n_win, int width, int win_per_wave, ScoreParams sp, double* __restrict__ means,
    double* __restrict__ partials) {
  __shared__ double tile[kWcmWaves][kWcmEntMax];
  __shared__ double part[kWcmWaves][64];
  __shared__ double mvec[kWcmWaves][kWcmMaxCols + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n1 = cols + 1, n_ent = n1 * n1;
  for (int e = lane; e < n_ent; e += 64) tile[wave][e] = 0.0;
  const int per = 64 / cols;                              // rows per wave step (cols <= 32: >= 2)
  const int col = lane % cols, rs = lane / cols;
  const bool reads = rs < per;
  const double ma = sp.mean_a[col], mb = sp.mean_b[col], pw = sp.power[col];
  const long long w0 = ((long long)blockIdx.x * kWcmWaves + wave) * win_per_wave;
  // (every wave of the workgroup walks win_per_wave steps, past the last window too: the
  // workgroup barriers below are met by all of them)
  for (int it = 0; it < win_per_wave; ++it) {
    const long long w = w0 + it;
    const bool live = w < n_win;                          // wave-uniform
    double s = 0.0;
    if (live && reads) {
      const long long r0 = w * width;
      int r = rs;
      for (; r + 3 * (long long)per < width; r += 4 * per) {   // four loads of each array in flight
        float av[4], bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          av[q] = a[(r0 + r + q * per) * lda + col];
          bv[q] = b[(r0 + r + q * per) * ldb + col];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) s += ((double)av[q] - ma) * ((double)bv[q] - mb) / pw;
      }
      for (; r < width; r += per)
        s += ((double)a[(r0 + r) * lda + col] - ma) * ((double)b[(r0 + r) * ldb + col] - mb) / pw;
    }
    part[wave][lane] = s;
    __syncthreads();
    if (lane <= cols) {
      double m = 1.0;                                     // lane == cols: the count's column
      if (lane < cols) {
        m = part[wave][lane];
        for (int q = 1; q < per; ++q) m += part[wave][q * cols + lane];
        m /= (double)width;
        if (live && means) means[w * cols + lane] = m;
      }
      mvec[wave][lane] = live ? m : 0.0;
    }
    __syncthreads();
    if (live)
      for (int e = lane; e < n_ent; e += 64) tile[wave][e] += mvec[wave][e / n1] * mvec[wave][e % n1];
  }
  __syncthreads();
  static_assert(kWcmWaves == 4, "the pairwise sum below is written for four waves");
  for (int e = tid; e < n_ent; e += kThreads)
    partials[(long long)blockIdx.x * n_ent + e] = (tile[0][e] + tile[1][e]) + (tile[2][e] + tile[3][e]);
}

// moments[e] = the workgroups' partials in workgroup order (none: zeros).
__global__ void window_class_moments_finish_kernel(const double* __restrict__ partials, int n_groups,
                                                   int n_ent, double* __restrict__ moments) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_ent) return;
  double s = 0.0;
  for (int g = 0; g < n_groups; ++g) s += partials[(long long)g * n_ent + e];
  moments[e] = s;
}

// ---------------------------------------------------------------- decisions
__global__ void decide_wta_kernel(const double* __restrict__ s1, const double* __restrict__ s2,
                                  long long n, unsigned char* __restrict__ out) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    out[i] = s1[i] > s2[i] ? 1 : 0;
}

// One lane per trial: a sequential +-0.1 scan clipped to [0.1, 0.9]
// (attention_decoder.py:169-173), float64 like the Python floats there.
__global__ void decide_step_kernel(const double* __restrict__ s1, const double* __restrict__ s2,
                                   const long long* __restrict__ win_off, int n_trials,
                                   unsigned char* __restrict__ out, double* __restrict__ state) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_trials) return;
  double st = state[t];
  for (long long i = win_off[t]; i < win_off[t + 1]; ++i) {
    if (s1[i] > s2[i]) st = fmin(0.9, st + 0.1);
    else st = fmax(0.1, st - 0.1);
    out[i] = st > 0.5 ? 1 : 0;
  }
  state[t] = st;
}

// ---------------------------------------------------------------- state-space decoder
// attention_decoder.StateSpaceAttentionDecoder.attention (attention_decoder.py:
// 329-451), one lane per trial, sequential over the trial's windows.
constexpr int kMaxKw = 32;

struct SsdParams {
  int outer_iter, inner_iter, newton_iter, k_f, k_b;
  double offset;
  int tuned;
  double rho_d[2], mu_d[2];
};

// np.sum order for a short vector: NumPy's pairwise routine keeps 8 running
// sums for n >= 8, combines them as a balanced tree and then adds the tail.
__device__ double np_sum(const double* a, int n) {
  if (n < 8) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += a[i];
    return s;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

// Decoder state that survives from one window to the next (attention_decoder.py: mu_d, rho_d,
// z_k_k, the smoothed tails, the last k_w correlations, the call count), for callers that feed
// windows as they arrive: kSsdState doubles per trial, all zeros = a fresh decoder.
constexpr int kSsdState = 8 * (kMaxKw + 1) + 8;

__global__ void ssd_kernel(const double* __restrict__ s1, const double* __restrict__ s2,
                           const long long* __restrict__ win_off, int n_trials, SsdParams sp,
                           double* __restrict__ out, double* __restrict__ state) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_trials) return;
  const int kw = sp.k_f + sp.k_b + 1;
  const double c0 = 1.96;
  const double mean_p = 0.2, var_p = 5.0;
  const double a_0 = 2 + mean_p * mean_p / var_p;
  const double b_0 = mean_p * (a_0 - 1);
  const double alpha_0[2] = {6.4113e+02, 4.0434e+03};
  const double beta_0[2] = {3.7581e+02, 6.2791e+03};
  double mu_0[2] = {-0.3994, -1.5103};
  double rho_d[2] = {1.7060, 0.64395};
  double mu_d[2] = {-0.3994, -1.5103};
  if (sp.tuned) {
    rho_d[0] = sp.rho_d[0]; rho_d[1] = sp.rho_d[1];
    mu_d[0] = sp.mu_d[0]; mu_d[1] = sp.mu_d[1];
    mu_0[0] = sp.mu_d[0]; mu_0[1] = sp.mu_d[1];
  }
  const double lam = 1.0;
  double r1h[kMaxKw], r2h[kMaxKw];           // last kw |r + offset|
  double z_last[kMaxKw], eta_last[kMaxKw];   // z_smoothed[-kw:], eta_smoothed[-kw:]
  double z_kk[kMaxKw + 1], s_kk[kMaxKw + 1], z_pred[kMaxKw + 1], s_pred[kMaxKw + 1];
  double z_cap[kMaxKw + 1], s_cap[kMaxKw + 1], sm[kMaxKw];
  double l1[kMaxKw], l2[kMaxKw], ep[kMaxKw], tmp[kMaxKw], eta[kMaxKw];
  for (int i = 0; i < kw; ++i) { z_last[i] = 0.0; eta_last[i] = 0.3; r1h[i] = r2h[i] = 0.0; }
  for (int i = 0; i <= kw; ++i) z_kk[i] = s_kk[i] = z_pred[i] = s_pred[i] = z_cap[i] = s_cap[i] = 0.0;
  for (int i = 0; i < kw; ++i) sm[i] = 0.0;
  int calls = 0;
  double* st = state ? state + (size_t)t * kSsdState : nullptr;
  constexpr int kA = kMaxKw + 1;
  if (st && st[8 * kA] > 0.0) {            // a decoder that has seen windows: pick it up
    for (int i = 0; i < kw; ++i) {
      r1h[i] = st[0 * kA + i]; r2h[i] = st[1 * kA + i];
      z_last[i] = st[2 * kA + i]; eta_last[i] = st[3 * kA + i];
    }
    for (int i = 0; i <= kw; ++i) {
      z_kk[i] = st[4 * kA + i]; s_kk[i] = st[5 * kA + i];
      z_cap[i] = st[6 * kA + i]; s_cap[i] = st[7 * kA + i];
    }
    calls = (int)st[8 * kA];
    rho_d[0] = st[8 * kA + 1]; rho_d[1] = st[8 * kA + 2];
    mu_d[0] = st[8 * kA + 3]; mu_d[1] = st[8 * kA + 4];
  }
  for (long long w = win_off[t]; w < win_off[t + 1]; ++w) {
    ++calls;
    for (int i = 0; i + 1 < kw; ++i) { r1h[i] = r1h[i + 1]; r2h[i] = r2h[i + 1]; }
    r1h[kw - 1] = fabs(s1[w] + sp.offset);
    r2h[kw - 1] = fabs(s2[w] + sp.offset);
    if (calls < kw) {
      out[w * 3 + 0] = 0.5; out[w * 3 + 1] = 0.5; out[w * 3 + 2] = 0.5;
      continue;
    }
    for (int i = 0; i < kw; ++i) { l1[i] = log(r1h[i]); l2[i] = log(r2h[i]); eta[i] = eta_last[i]; }
    const double* z = z_last;   // first outer iteration; afterwards z_cap + 1
    for (int it = 0; it < sp.outer_iter; ++it) {
      for (int i = 0; i < kw; ++i) {
        const double d10 = l1[i] - mu_d[0], d11 = l1[i] - mu_d[1];
        const double d21 = l2[i] - mu_d[1], d20 = l2[i] - mu_d[0];
        const double p11 = (1.0 / r1h[i]) * sqrt(rho_d[0]) * exp(-0.5 * rho_d[0] * (d10 * d10));
        const double p12 = (1.0 / r1h[i]) * sqrt(rho_d[1]) * exp(-0.5 * rho_d[1] * (d11 * d11));
        const double p21 = (1.0 / r2h[i]) * sqrt(rho_d[1]) * exp(-0.5 * rho_d[1] * (d21 * d21));
        const double p22 = (1.0 / r2h[i]) * sqrt(rho_d[0]) * exp(-0.5 * rho_d[0] * (d20 * d20));
        const double p = 1.0 / (1.0 + exp(-z[i]));
        ep[i] = (p * p11 * p21) / (p * p11 * p21 + (1.0 - p) * p12 * p22);
      }
      for (int i = 0; i < kw; ++i) tmp[i] = ep[i] * l1[i] + (1.0 - ep[i]) * l2[i];
      mu_d[0] = (np_sum(tmp, kw) + kw * mu_0[0]) / (2.0 * kw);
      for (int i = 0; i < kw; ++i) tmp[i] = ep[i] * l2[i] + (1.0 - ep[i]) * l1[i];
      mu_d[1] = (np_sum(tmp, kw) + kw * mu_0[1]) / (2.0 * kw);
      for (int i = 0; i < kw; ++i) {
        const double u = l1[i] - mu_d[0], v = l2[i] - mu_d[0];
        tmp[i] = ep[i] * (u * u) + (1.0 - ep[i]) * (v * v);
      }
      {
        const double dm = mu_d[0] - mu_0[0];
        rho_d[0] = (2.0 * kw * alpha_0[0]) / (np_sum(tmp, kw) + kw * (2.0 * beta_0[0] + dm * dm));
      }
      for (int i = 0; i < kw; ++i) {
        const double u = l2[i] - mu_d[1], v = l1[i] - mu_d[1];
        tmp[i] = ep[i] * (u * u) + (1.0 - ep[i]) * (v * v);
      }
      {
        const double dm = mu_d[1] - mu_0[1];
        rho_d[1] = (2.0 * kw * alpha_0[1]) / (np_sum(tmp, kw) + kw * (2.0 * beta_0[1] + dm * dm));
      }
      for (int in = 0; in < sp.inner_iter; ++in) {
        for (int k = 1; k <= kw; ++k) {
          z_pred[k] = lam * z_kk[k - 1];
          s_pred[k] = lam * lam * s_kk[k - 1] + eta[k - 1];
          for (int nt = 0; nt < sp.newton_iter; ++nt) {
            const double ez = exp(z_kk[k]);
            z_kk[k] = z_kk[k] - (z_kk[k] - z_pred[k] - s_pred[k] * (ep[k - 1] - ez / (1 + ez))) /
                                    (1 + s_pred[k] * ez / ((1 + ez) * (1 + ez)));
          }
          const double ez = exp(z_kk[k]);
          s_kk[k] = 1.0 / (1.0 / s_pred[k] + ez / ((1 + ez) * (1 + ez)));
        }
        z_cap[kw] = z_kk[kw];
        s_cap[kw] = s_kk[kw];
        for (int k = 0; k < kw; ++k) {   // ascending, as in the reference (:423-430)
          sm[k] = s_kk[k] * lam / s_pred[k + 1];
          z_cap[k] = z_kk[k] + sm[k] * (z_cap[k + 1] - z_pred[k + 1]);
          s_cap[k] = s_kk[k] + sm[k] * sm[k] * (s_cap[k + 1] - s_pred[k + 1]);
        }
        z_kk[0] = z_cap[0];
        s_kk[0] = s_cap[0];
        for (int i = 0; i < kw; ++i) {
          const double dz = z_cap[i + 1] - z_cap[i];
          eta[i] = (dz * dz + s_cap[i + 1] + s_cap[i] - 2.0 * s_cap[i + 1] * sm[i] + 2 * b_0) /
                   (1 + 2 * (a_0 + 1));
        }
      }
      z = z_cap + 1;
    }
    for (int i = 0; i < kw; ++i) { z_last[i] = z_cap[i + 1]; eta_last[i] = eta[i]; }
    z_kk[0] = z_cap[1];
    const double zd = z_last[kw - 1 - sp.k_f], ed = eta_last[kw - 1 - sp.k_f];
    out[w * 3 + 0] = 1.0 / (1 + exp(-zd));
    out[w * 3 + 1] = 1.0 / (1 + exp(-zd - c0 * sqrt(ed)));
    out[w * 3 + 2] = 1.0 / (1 + exp(-zd + c0 * sqrt(ed)));
  }
  if (st) {
    for (int i = 0; i < kw; ++i) {
      st[0 * kA + i] = r1h[i]; st[1 * kA + i] = r2h[i];
      st[2 * kA + i] = z_last[i]; st[3 * kA + i] = eta_last[i];
    }
    for (int i = 0; i <= kw; ++i) {
      st[4 * kA + i] = z_kk[i]; st[5 * kA + i] = s_kk[i];
      st[6 * kA + i] = z_cap[i]; st[7 * kA + i] = s_cap[i];
    }
    st[8 * kA] = (double)calls;
    st[8 * kA + 1] = rho_d[0]; st[8 * kA + 2] = rho_d[1];
    st[8 * kA + 3] = mu_d[0]; st[8 * kA + 4] = mu_d[1];
  }
}

// ---------------------------------------------------------------- helpers
// Full windows of `width` frames, `hop` apart, in a trial of n frames.
int64_t windows_of(int64_t n, int width, int hop) { return n >= width ? (n - width) / hop + 1 : 0; }

// The first frame of every full window, trial after trial.
std::vector<long long> build_windows(const int64_t* trial_offsets, int num_trials, int width, int hop) {
  std::vector<long long> row0;
  for (int t = 0; t < num_trials; ++t) {
    const int64_t tw = windows_of(trial_offsets[t + 1] - trial_offsets[t], width, hop);
    for (int64_t i = 0; i < tw; ++i) row0.push_back(trial_offsets[t] + i * hop);
  }
  return row0;
}

int64_t gcd64(int64_t a, int64_t b) {
  while (b) { const int64_t t = a % b; a = b; b = t; }
  return a;
}

// Block size for the two-stage window sums: a divisor of gcd(width, hop) -- the largest one
// <= 256 (a block is summed by 16 lanes: <= 16 frames per lane, and non-overlapping windows,
// e.g. minibatch metrics with hop = width = 1000, still give thousands of blocks to spread over
// the chip), else the largest <= 4096 -- or 0 if the only usable divisors are tiny / the
// windows would span too many blocks (then the one-workgroup-per-window kernel is used).
int window_block_size(int width, int hop) {
  const int64_t g = gcd64(width, hop);
  int best = 0;
  for (int64_t dv = g < 256 ? g : 256; dv >= 32; --dv)
    if (g % dv == 0) { best = (int)dv; break; }
  if (best == 0)
    for (int64_t dv = g < 4096 ? g : 4096; dv >= 32; --dv)
      if (g % dv == 0) { best = (int)dv; break; }
  if (best == 0 || width / best > (1 << 16)) return 0;   // (a window sums its blocks serially)
  return best;
}

// Per-trial descriptors of the window kernels: `first` counts the windows ahead of a trial (out0 = 0: the
// table of window_sums_short_kernel, which reads its windows from the frames).  Returns the window count.
int64_t build_window_table(const int64_t* trial_offsets, int num_trials, int width, int hop, std::vector<FileDesc>* win_tab) {
  win_tab->resize(num_trials);
  int64_t nw = 0;
  for (int t = 0; t < num_trials; ++t) {
    FileDesc& w = (*win_tab)[t];
    w.row0 = trial_offsets[t]; w.nrows = trial_offsets[t + 1] - trial_offsets[t]; w.out0 = 0; w.first = nw;
    nw += windows_of(w.nrows, width, hop);
  }
  return nw;
}

// Per-trial descriptors for the block and window kernels (blocks of g frames of
// every trial that has at least one full window): a window table whose out0 is the trial's first block.
void build_block_tables(const int64_t* trial_offsets, int num_trials, int width, int hop, int g,
                        std::vector<FileDesc>* blk_tab, std::vector<FileDesc>* win_tab, int64_t* n_blocks, int64_t* n_windows) {
  *n_windows = build_window_table(trial_offsets, num_trials, width, hop, win_tab);
  blk_tab->resize(num_trials);
  int64_t nb = 0;
  for (int t = 0; t < num_trials; ++t) {
    FileDesc& b = (*blk_tab)[t];
    b.row0 = trial_offsets[t]; b.nrows = (*win_tab)[t].nrows; b.out0 = trial_offsets[t]; b.first = nb;
    (*win_tab)[t].out0 = nb;
    const int64_t tw = windows_of(b.nrows, width, hop);
    if (tw > 0) nb += ((tw - 1) * hop + width) / g;
  }
  *n_blocks = nb;
}

// The items (blocks, windows) of trial t in one of those tables: `first` runs up to `total`.
int64_t items_of(const std::vector<FileDesc>& tab, int t, int64_t total) {
  return (t + 1 < (int)tab.size() ? tab[t + 1].first : total) - tab[t].first;
}

// The num_trials + 1 window offsets as the kernels' long long, at the head of a td_scratch block of `bytes`.
int upload_window_offsets(td_handle* h, const int64_t* window_offsets_host, int num_trials, size_t bytes, void** scratch) {
  TD_TRY(td_scratch(h, bytes, scratch));
  std::vector<long long> off(window_offsets_host, window_offsets_host + num_trials + 1);
  return td_upload_async(h, off.data(), sizeof(long long) * off.size(), *scratch);
}

int fill_score_params(td_handle* h, ScoreParams* sp, int cols, const double* mean_a,
                      const double* mean_b, const double* power, const double* lda_w,
                      double slope, double intercept) {
  TD_REQUIRE(h, cols >= 1, "cols must be >= 1, not %d", cols);
  std::vector<double> t((size_t)4 * cols);
  for (int c = 0; c < cols; ++c) {
    t[c] = mean_a ? mean_a[c] : 0.0;
    t[cols + c] = mean_b ? mean_b[c] : 0.0;
    t[2 * cols + c] = power ? power[c] : 1.0;
    t[3 * cols + c] = lda_w ? lda_w[c] : 0.0;
  }
  const void* dev = nullptr;
  TD_TRY(td_table_upload(h, t.data(), sizeof(double) * t.size(), &dev));
  const double* d = reinterpret_cast<const double*>(dev);
  sp->mean_a = d; sp->mean_b = d + cols; sp->power = d + 2 * cols; sp->lda_w = d + 3 * cols;
  sp->lda_slope = slope;
  sp->lda_intercept = intercept;
  return TD_OK;
}

}  // namespace

extern "C" {

int td_window_count(const int64_t* trial_offsets_host, int num_trials, int width, int hop,
                    int64_t* window_offsets_host, int64_t* total_windows) {
  if (!trial_offsets_host || num_trials < 0 || width <= 0 || hop <= 0)
    return td_fail(nullptr, TD_ERR_INVALID, "td_window_count: bad argument");
  // (closed form: the windows themselves are not listed here -- a quarter of a million of them at
  // W = 10 / hop 5 made this call 140 us of host time in front of every decode)
  int64_t count = 0;
  for (int t = 0; t < num_trials; ++t) {
    if (window_offsets_host) window_offsets_host[t] = count;
    count += windows_of(trial_offsets_host[t + 1] - trial_offsets_host[t], width, hop);
  }
  if (window_offsets_host) window_offsets_host[num_trials] = count;
  if (total_windows) *total_windows = count;
  return TD_OK;
}

int td_window_sums(td_handle* h, const float* a_dev, int64_t lda, const float* b_dev, int64_t ldb,
                   int cols, const int64_t* trial_offsets_host, int num_trials, int width, int hop,
                   double* out_dev) {
  return td_window_sums_cycled(h, a_dev, lda, b_dev, ldb, cols, cols, trial_offsets_host, num_trials, width, hop,
                               out_dev);
}

int td_window_sums_cycled(td_handle* h, const float* a_dev, int64_t lda, const float* b_dev, int64_t ldb,
                          int cols, int b_cols, const int64_t* trial_offsets_host, int num_trials, int width,
                          int hop, double* out_dev) {
  if (!h || !a_dev || !b_dev || !trial_offsets_host || !out_dev)
    return td_fail(h, TD_ERR_INVALID, "td_window_sums: NULL argument");
  TD_REQUIRE(h, cols > 0 && width > 0 && hop > 0, "td_window_sums: bad sizes");
  TD_REQUIRE(h, b_cols > 0 && b_cols <= cols && cols % b_cols == 0, "td_window_sums_cycled: b_cols must divide cols");
  const int g = window_block_size(width, hop);
  TD_REQUIRE(h, b_cols == cols || g > 0,
             "td_window_sums_cycled: windows without a common block of >= 32 frames take b with all its columns");
  if (g > 0) {
    // shared frames are read once: block partials, then windows from blocks
    std::vector<FileDesc> blk_tab, win_tab;
    int64_t n_blocks = 0, n_win = 0;
    build_block_tables(trial_offsets_host, num_trials, width, hop, g, &blk_tab, &win_tab, &n_blocks,
                       &n_win);
    if (n_win == 0) return TD_OK;
    const size_t tb = td_round_up(sizeof(FileDesc) * num_trials, 256);
    void* scratch = nullptr;
    TD_TRY(td_scratch(h, 2 * tb + sizeof(double) * n_blocks * cols * 5, &scratch));
    FileDesc* d_blk = reinterpret_cast<FileDesc*>(scratch);
    FileDesc* d_win = reinterpret_cast<FileDesc*>(reinterpret_cast<char*>(scratch) + tb);
    double* bsums = reinterpret_cast<double*>(reinterpret_cast<char*>(scratch) + 2 * tb);
    TD_TRY(td_upload_async(h, blk_tab.data(), sizeof(FileDesc) * num_trials, d_blk));
    TD_TRY(td_upload_async(h, win_tab.data(), sizeof(FileDesc) * num_trials, d_win));
    if (cols >= 8 && cols <= 64)
      hipLaunchKernelGGL(block_sums_cols_kernel, dim3((unsigned)td_ceil_div(n_blocks, kThreads / 64)), dim3(kThreads), 0,
                         h->stream, a_dev, (long long)lda, b_dev, (long long)ldb, cols, b_cols, d_blk, num_trials,
                         (long long)n_blocks, g, bsums);
    else
    hipLaunchKernelGGL(block_sums_kernel,
                       dim3((unsigned)td_ceil_div(n_blocks, kThreads / kBlockLanes), (unsigned)(cols < 64 ? cols : 64)),
                       dim3(kThreads), 0, h->stream, a_dev, (long long)lda, b_dev, (long long)ldb,
                       cols, b_cols, d_blk, num_trials, (long long)n_blocks, g, bsums);
    const long long outs = (long long)n_win * cols * 5;
    if (width / g > 64)
      hipLaunchKernelGGL(window_from_blocks_wide_kernel, dim3((unsigned)td_ceil_div(outs, 4)),
                         dim3(256), 0, h->stream, bsums, d_win, num_trials, (long long)n_win, cols,
                         width / g, hop / g, out_dev);
    else
      hipLaunchKernelGGL(window_from_blocks_kernel, dim3((unsigned)td_ceil_div(outs, 256)), dim3(256),
                         0, h->stream, bsums, d_win, num_trials, (long long)n_win, cols, width / g,
                         hop / g, out_dev);
    TD_HIP(h, hipGetLastError());
    return TD_OK;
  }
  if (width <= 256) {
    std::vector<FileDesc> win_tab;
    const int64_t nw = build_window_table(trial_offsets_host, num_trials, width, hop, &win_tab);
    if (nw == 0) return TD_OK;
    const void* tab = nullptr;
    TD_TRY(td_table_upload(h, win_tab.data(), sizeof(FileDesc) * num_trials, &tab));
    hipLaunchKernelGGL(window_sums_short_kernel, dim3((unsigned)td_ceil_div(nw * cols, 256)),
                       dim3(256), 0, h->stream, a_dev, (long long)lda, b_dev, (long long)ldb, cols,
                       reinterpret_cast<const FileDesc*>(tab), num_trials, nw, width, hop, out_dev);
    TD_HIP(h, hipGetLastError());
    return TD_OK;
  }
  const std::vector<long long> row0 = build_windows(trial_offsets_host, num_trials, width, hop);
  if (row0.empty()) return TD_OK;
  void* scratch = nullptr;
  TD_TRY(td_scratch(h, row0.size() * sizeof(long long), &scratch));
  TD_TRY(td_upload_async(h, row0.data(), row0.size() * sizeof(long long), scratch));
  hipLaunchKernelGGL(window_sums_kernel, dim3((unsigned)row0.size()), dim3(kThreads), 0, h->stream,
                     a_dev, (long long)lda, b_dev, (long long)ldb, cols,
                     reinterpret_cast<const long long*>(scratch), width, out_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_window_means(td_handle* h, const double* v_dev, const int64_t* trial_offsets_host,
                    int num_trials, int width, int hop, double* out_dev) {
  if (!h || !v_dev || !trial_offsets_host || !out_dev)
    return td_fail(h, TD_ERR_INVALID, "td_window_means: NULL argument");
  TD_REQUIRE(h, width > 0 && hop > 0, "td_window_means: bad sizes");
  const std::vector<long long> row0 = build_windows(trial_offsets_host, num_trials, width, hop);
  if (row0.empty()) return TD_OK;
  void* scratch = nullptr;
  TD_TRY(td_scratch(h, row0.size() * sizeof(long long), &scratch));
  TD_TRY(td_upload_async(h, row0.data(), row0.size() * sizeof(long long), scratch));
  hipLaunchKernelGGL(window_means_kernel, dim3((unsigned)row0.size()), dim3(kThreads), 0,
                     h->stream, v_dev, reinterpret_cast<const long long*>(scratch), width, out_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_window_scores(td_handle* h, const double* sums_dev, int64_t total_windows, int cols,
                     int width, int mode, int reduction, const double* mean_a_host,
                     const double* mean_b_host, const double* power_host, double* scores_dev) {
  if (!h || !sums_dev || !scores_dev) return td_fail(h, TD_ERR_INVALID, "td_window_scores: NULL");
  TD_REQUIRE(h, mode == 0 || mode == 1, "td_window_scores: mode must be 0 or 1");
  TD_REQUIRE(h, mode == 1 || (reduction >= 0 && reduction <= 2),
             "Unknown reduction technique: %d", reduction);
  TD_REQUIRE(h, mode == 1 || reduction != 1 || cols >= 2, "reduction 'second' needs >= 2 columns");
  ScoreParams sp = {nullptr, nullptr, nullptr, nullptr, 1.0, 0.0};
  if (mode == 0)      // (the Pearson mode uses no per-column statistics)
    TD_TRY(fill_score_params(h, &sp, cols, mean_a_host, mean_b_host, power_host, nullptr, 1.0, 0.0));
  if (total_windows <= 0) return TD_OK;
  hipLaunchKernelGGL(window_scores_kernel, dim3((unsigned)td_ceil_div(total_windows, 256)),
                     dim3(256), 0, h->stream, sums_dev, (long long)total_windows, cols, width, mode,
                     reduction, cols, sp, scores_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_window_pearson(td_handle* h, const double* sums_dev, int64_t total_windows, int cols,
                      int group, int width, double* scores_dev) {
  if (!h || !sums_dev || !scores_dev) return td_fail(h, TD_ERR_INVALID, "td_window_pearson: NULL");
  TD_REQUIRE(h, cols >= 1 && group >= 1 && cols % group == 0,
             "td_window_pearson: %d columns are not whole groups of %d", cols, group);
  if (total_windows <= 0) return TD_OK;
  ScoreParams sp = {nullptr, nullptr, nullptr, nullptr, 1.0, 0.0};
  hipLaunchKernelGGL(window_scores_kernel, dim3((unsigned)td_ceil_div(total_windows, 256)),
                     dim3(256), 0, h->stream, sums_dev, (long long)total_windows, cols, width, 1,
                     0, group, sp, scores_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_frame_scores(td_handle* h, const float* a_dev, int64_t lda, const float* b_dev, int64_t ldb,
                    int cols, int64_t rows, int reduction, const double* mean_a_host,
                    const double* mean_b_host, const double* power_host,
                    const double* lda_w_host, double lda_slope, double lda_intercept,
                    double* out_dev) {
  if (!h || !a_dev || !b_dev || !out_dev) return td_fail(h, TD_ERR_INVALID, "td_frame_scores: NULL");
  TD_REQUIRE(h, reduction >= 0 && reduction <= 5, "Unknown reduction technique: %d", reduction);
  TD_REQUIRE(h, reduction != 1 || cols >= 2, "reduction 'second' needs >= 2 columns");
  TD_REQUIRE(h, reduction != 4 || lda_w_host, "lda reduction needs its weights");
  ScoreParams sp;
  TD_TRY(fill_score_params(h, &sp, cols, mean_a_host, mean_b_host, power_host, lda_w_host,
                           lda_slope, lda_intercept));
  if (rows <= 0) return TD_OK;
  long long blocks = td_ceil_div(rows, 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(frame_scores_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, a_dev,
                     (long long)lda, b_dev, (long long)ldb, cols, (long long)rows, reduction, sp,
                     out_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_window_class_moments(td_handle* h, const float* a_dev, int64_t lda, const float* b_dev,
                            int64_t ldb, int cols, int64_t rows, int width,
                            const double* mean_a_host, const double* mean_b_host,
                            const double* power_host, double* means_dev, double* moments_dev) {
  if (!h || !a_dev || !b_dev || !moments_dev)
    return td_fail(h, TD_ERR_INVALID, "td_window_class_moments: NULL argument");
  TD_REQUIRE(h, cols >= 1 && cols <= kWcmMaxCols,
             "td_window_class_moments: 1 to %d columns, not %d", kWcmMaxCols, cols);
  TD_REQUIRE(h, width >= 2, "td_window_class_moments: window of %d frames (at least 2)", width);
  TD_REQUIRE(h, rows >= 0 && lda >= cols && ldb >= cols, "td_window_class_moments: bad sizes");
  ScoreParams sp;
  TD_TRY(fill_score_params(h, &sp, cols, mean_a_host, mean_b_host, power_host, nullptr, 1.0, 0.0));
  const int n_ent = (cols + 1) * (cols + 1);
  const int64_t n_win = rows / width;
  // the grid follows from (rows, width) alone
  int64_t wpw = td_ceil_div(n_win, (int64_t)kWcmWaves * kWcmMaxGroups);
  if (wpw < kWcmMinWinPerWave) wpw = kWcmMinWinPerWave;
  const int64_t groups = td_ceil_div(n_win, wpw * kWcmWaves);
  TD_REQUIRE(h, wpw <= 0x7fffffff, "td_window_class_moments: too many windows");
  double* partials = nullptr;
  if (groups > 0) {
    void* scratch = nullptr;
    TD_TRY(td_scratch(h, (size_t)groups * n_ent * sizeof(double), &scratch));
    partials = reinterpret_cast<double*>(scratch);
    hipLaunchKernelGGL(window_class_moments_kernel, dim3((unsigned)groups), dim3(kThreads), 0,
                       h->stream, a_dev, (long long)lda, b_dev, (long long)ldb, cols,
                       (long long)n_win, width, (int)wpw, sp, means_dev, partials);
    TD_HIP(h, hipGetLastError());
  }
  hipLaunchKernelGGL(window_class_moments_finish_kernel, dim3((unsigned)td_ceil_div(n_ent, 256)),
                     dim3(256), 0, h->stream, partials, (int)groups, n_ent, moments_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_decide_wta(td_handle* h, const double* s1_dev, const double* s2_dev, int64_t n,
                  uint8_t* out_dev) {
  if (!h || !s1_dev || !s2_dev || !out_dev) return td_fail(h, TD_ERR_INVALID, "td_decide_wta: NULL");
  if (n <= 0) return TD_OK;
  long long blocks = td_ceil_div(n, 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(decide_wta_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, s1_dev,
                     s2_dev, (long long)n, out_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_decide_step(td_handle* h, const double* s1_dev, const double* s2_dev,
                   const int64_t* window_offsets_host, int num_trials, uint8_t* out_dev,
                   double* state_inout_host) {
  if (!h || !s1_dev || !s2_dev || !window_offsets_host || !out_dev)
    return td_fail(h, TD_ERR_INVALID, "td_decide_step: NULL");
  if (num_trials <= 0) return TD_OK;
  const size_t off_bytes = td_round_up(sizeof(long long) * (num_trials + 1), 256);
  void* scratch = nullptr;
  TD_TRY(upload_window_offsets(h, window_offsets_host, num_trials, off_bytes + sizeof(double) * num_trials,
                               &scratch));
  std::vector<double> st(num_trials, 0.5);
  if (state_inout_host) st.assign(state_inout_host, state_inout_host + num_trials);
  double* dstate = reinterpret_cast<double*>(reinterpret_cast<char*>(scratch) + off_bytes);
  TD_TRY(td_upload_async(h, st.data(), sizeof(double) * st.size(), dstate));
  hipLaunchKernelGGL(decide_step_kernel, dim3((unsigned)td_ceil_div(num_trials, 64)), dim3(64), 0,
                     h->stream, s1_dev, s2_dev, reinterpret_cast<const long long*>(scratch),
                     num_trials, out_dev, dstate);
  TD_HIP(h, hipGetLastError());
  if (state_inout_host) {
    TD_HIP(h, hipMemcpyAsync(state_inout_host, dstate, sizeof(double) * num_trials,
                             hipMemcpyDeviceToHost, h->stream));
    TD_HIP(h, hipStreamSynchronize(h->stream));
  }
  return TD_OK;
}

int td_ssd_state_doubles(void) { return kSsdState; }

int td_decode_ssd(td_handle* h, const double* s1_dev, const double* s2_dev,
                  const int64_t* window_offsets_host, int num_trials, const double* params_host,
                  const double* prior_host, double* out_dev) {
  return td_decode_ssd_stream(h, s1_dev, s2_dev, window_offsets_host, num_trials, params_host,
                              prior_host, nullptr, out_dev);
}

int td_decode_ssd_stream(td_handle* h, const double* s1_dev, const double* s2_dev,
                         const int64_t* window_offsets_host, int num_trials,
                         const double* params_host, const double* prior_host, double* state_dev,
                         double* out_dev) {
  if (!h || !s1_dev || !s2_dev || !window_offsets_host || !params_host || !out_dev)
    return td_fail(h, TD_ERR_INVALID, "td_decode_ssd: NULL");
  SsdParams sp;
  sp.outer_iter = (int)params_host[0];
  sp.inner_iter = (int)params_host[1];
  sp.newton_iter = (int)params_host[2];
  sp.k_f = (int)params_host[3];
  sp.k_b = (int)params_host[4];
  sp.offset = params_host[5];
  sp.tuned = params_host[6] != 0.0 ? 1 : 0;
  TD_REQUIRE(h, sp.k_f >= 0 && sp.k_b >= 0 && sp.k_f + sp.k_b + 1 <= kMaxKw,
             "state-space window k_f + k_b + 1 must be <= %d", kMaxKw);
  TD_REQUIRE(h, !sp.tuned || prior_host, "tuned priors requested but not given");
  for (int i = 0; i < 2; ++i) {
    sp.rho_d[i] = sp.tuned ? prior_host[i] : 0.0;
    sp.mu_d[i] = sp.tuned ? prior_host[2 + i] : 0.0;
  }
  if (num_trials <= 0) return TD_OK;
  void* scratch = nullptr;
  TD_TRY(upload_window_offsets(h, window_offsets_host, num_trials, sizeof(long long) * (num_trials + 1), &scratch));
  // (a decoder that carries state is a step of an online session: td_profile_read counts its launch)
  if (state_dev) TD_TRY(td_profile_mark(h, true, 0.0));
  hipLaunchKernelGGL(ssd_kernel, dim3((unsigned)td_ceil_div(num_trials, 64)), dim3(64), 0,
                     h->stream, s1_dev, s2_dev, reinterpret_cast<const long long*>(scratch),
                     num_trials, sp, out_dev, state_dev);
  TD_HIP(h, hipGetLastError());
  if (state_dev) TD_TRY(td_profile_mark(h, false, 0.0));
  return TD_OK;
}

int td_decode_fused(td_handle* h, const float* eeg_dev, int64_t ldx, int c, int pre, int post,
                    const float* w_dev, const float* b_dev, const float* env_dev, int64_t ldenv,
                    const int64_t* trial_offsets_host, int num_trials, int width, int hop,
                    const double* corr_host, double* scores_dev, uint8_t* decisions_dev) {
  if (!h || !eeg_dev || !w_dev || !env_dev || !trial_offsets_host || !corr_host || !scores_dev ||
      !decisions_dev)
    return td_fail(h, TD_ERR_INVALID, "td_decode_fused: NULL argument");
  TD_REQUIRE(h, num_trials > 0 && width > 0 && hop > 0, "td_decode_fused: bad sizes");
  TD_REQUIRE(h, ldenv >= 2, "td_decode_fused: the envelope stream needs two columns");
  const int64_t rows = trial_offsets_host[num_trials];
  int g = window_block_size(width, hop);
  if (g == 0 && num_trials >= 16) {
    // Short windows (W = 10 / hop 5 of the reference harness: gcd < 32): the per-trial tail kernel
    // does not care how small a block is as long as a trial's blocks fit its LDS table -- blocks of
    // gcd(W, hop) frames then, instead of the unfused chain below, whose per-window tables (240 000
    // entries at C4) are built on the host three times per call (0.3 -> 0.7 ms a call against 0.09)
    const int64_t gg = gcd64(width, hop);
    bool fits = width / gg <= 64;
    for (int t = 0; t < num_trials && fits; ++t) {
      const int64_t tw = windows_of(trial_offsets_host[t + 1] - trial_offsets_host[t], width, hop);
      if (tw > 0 && ((tw - 1) * hop + width) / gg > kTrialBlocksMax) fits = false;
    }
    if (fits) g = (int)gg;
  }
  if (g == 0) {
    // windows that do not share whole blocks (gcd(width, hop) < 32): unfused chain
    const std::vector<long long> row0 = build_windows(trial_offsets_host, num_trials, width, hop);
    const int64_t nw = (int64_t)row0.size();
    // (predictions and sums in the solver-workspace arena: the window kernels use td_scratch
    // themselves; no allocation, nothing waits for the device)
    float* pred = nullptr;
    const size_t bytes = td_round_up(sizeof(float) * rows, 256) +
                         sizeof(double) * (size_t)nw * (10 + 2) + 256;
    TD_TRY(td_workspace(h, bytes, reinterpret_cast<void**>(&pred)));
    double* sums = reinterpret_cast<double*>(reinterpret_cast<char*>(pred) +
                                             td_round_up(sizeof(float) * rows, 256));
    double* s1 = sums + (size_t)nw * 10;
    double* s2 = s1 + nw;
    int rc = td_launch_fir(h, eeg_dev, ldx, trial_offsets_host, num_trials, c, pre, post, w_dev, b_dev,
                           1, pred, 1);
    for (int spk = 0; spk < 2 && rc == TD_OK && nw > 0; ++spk) {
      rc = td_window_sums(h, env_dev + spk, ldenv, pred, 1, 1, trial_offsets_host, num_trials, width,
                          hop, sums + (size_t)spk * nw * 5);
      if (rc == TD_OK)
        rc = td_window_scores(h, sums + (size_t)spk * nw * 5, nw, 1, width, 0, 0,
                              corr_host + 3 * spk, corr_host + 3 * spk + 1, corr_host + 3 * spk + 2,
                              spk == 0 ? s1 : s2);
    }
    if (rc == TD_OK && nw > 0) {
      rc = td_decide_wta(h, s1, s2, nw, decisions_dev);
      hipMemcpy2DAsync(scores_dev, 2 * sizeof(double), s1, sizeof(double), sizeof(double), nw,
                       hipMemcpyDeviceToDevice, h->stream);
      hipMemcpy2DAsync(scores_dev + 1, 2 * sizeof(double), s2, sizeof(double), sizeof(double), nw,
                       hipMemcpyDeviceToDevice, h->stream);
    }
    return rc;
  }
  // Three launches, one scratch block, per-trial descriptors from the table cache (uploaded
  // only when the trial layout changes), no allocation and no host synchronisation:
  //   FIR prediction (matrix cores) -> block partial sums of (envelope_spk, prediction)
  //   -> window scores of both speakers + winner-take-all.
  std::vector<FileDesc> tabs, win_tab;
  int64_t n_blocks = 0, nwin = 0;
  build_block_tables(trial_offsets_host, num_trials, width, hop, g, &tabs, &win_tab, &n_blocks,
                     &nwin);
  FusedCorr fc;
  for (int spk = 0; spk < 2; ++spk) {
    fc.mean_a[spk] = corr_host[3 * spk];
    fc.mean_b[spk] = corr_host[3 * spk + 1];
    fc.power[spk] = corr_host[3 * spk + 2];
  }
  // many short trials: one workgroup per trial does block sums, windows and decisions
  int64_t max_tb = 0;
  for (int t = 0; t < num_trials; ++t) {
    const int64_t tb = items_of(tabs, t, n_blocks);
    if (tb > max_tb) max_tb = tb;
  }
  if (nwin > 0 && num_trials >= 16 && max_tb <= kTrialBlocksMax) {
    std::vector<FileDesc> tt(num_trials);
    for (int t = 0; t < num_trials; ++t) {
      tt[t].row0 = trial_offsets_host[t];
      tt[t].nrows = items_of(tabs, t, n_blocks);
      tt[t].out0 = items_of(win_tab, t, nwin);
      tt[t].first = win_tab[t].first;
    }
    int64_t tt_stride = num_trials > 1 ? tt[1].row0 - tt[0].row0 : 0;
    for (int t = 1; t < num_trials && tt_stride > 0; ++t)
      if (tt[t].row0 - tt[t - 1].row0 != tt_stride || tt[t].nrows != tt[0].nrows || tt[t].out0 != tt[0].out0 ||
          tt[t].first != t * tt[0].out0)
        tt_stride = 0;
    const size_t s_pred1 = td_round_up(sizeof(float) * rows, 256);
    void* scratch1 = nullptr;
    TD_TRY(td_scratch(h, s_pred1, &scratch1));
    float* pred1 = reinterpret_cast<float*>(scratch1);
    const void* tt_dev = nullptr;
    TD_TRY(td_table_upload(h, tt.data(), sizeof(FileDesc) * tt.size(), &tt_dev));
    TD_TRY(td_launch_fir(h, eeg_dev, ldx, trial_offsets_host, num_trials, c, pre, post, w_dev, b_dev, 1,
                         pred1, 1, 0));
    hipLaunchKernelGGL(decode_trial_kernel, dim3((unsigned)num_trials), dim3(kTrialThreads),
                       sizeof(double) * 5 * (size_t)max_tb, h->stream, env_dev, (long long)ldenv,
                       pred1, reinterpret_cast<const FileDesc*>(tt_dev), g, width / g, hop / g, width,
                       fc, scores_dev, decisions_dev, (long long)tt_stride, tt[0]);
    TD_HIP(h, hipGetLastError());
    return TD_OK;
  }
  tabs.insert(tabs.end(), win_tab.begin(), win_tab.end());
  const size_t s_pred = td_round_up(sizeof(float) * rows, 256);
  void* scratch = nullptr;
  TD_TRY(td_scratch(h, s_pred + sizeof(double) * n_blocks * 10 + 256, &scratch));
  char* base = reinterpret_cast<char*>(scratch);
  float* pred = reinterpret_cast<float*>(base);
  double* bsums = reinterpret_cast<double*>(base + s_pred);
  // both descriptor tables first, so that no copy sits between the kernels
  const void* tab_dev = nullptr;
  if (nwin > 0) TD_TRY(td_table_upload(h, tabs.data(), sizeof(FileDesc) * tabs.size(), &tab_dev));
  const FileDesc* d_blk = reinterpret_cast<const FileDesc*>(tab_dev);
  const FileDesc* d_win = d_blk + num_trials;
  TD_TRY(td_launch_fir(h, eeg_dev, ldx, trial_offsets_host, num_trials, c, pre, post, w_dev, b_dev, 1,
                       pred, 1, 0));
  if (nwin == 0) return TD_OK;
  // a = envelope of speaker spk (the "truth" stream), b = the shared prediction
  hipLaunchKernelGGL(block_sums_pair_kernel,
                     dim3((unsigned)td_ceil_div(n_blocks, kThreads / kBlockLanes)), dim3(kThreads), 0,
                     h->stream, env_dev, (long long)ldenv, pred, d_blk, num_trials,
                     (long long)n_blocks, g, bsums);
  hipLaunchKernelGGL(decode_finalize_kernel, dim3((unsigned)td_ceil_div(nwin, 256)), dim3(256), 0,
                     h->stream, bsums, d_win, num_trials, (long long)nwin, width / g, hop / g, width,
                     fc, scores_dev, decisions_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

}  // extern "C"
