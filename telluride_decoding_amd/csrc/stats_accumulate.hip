// The accumulate of the statistics (stats_common.h): what a call sums per file, the routes that turn it into
// matrix kernels, and the ONE finalize launch that does everything around them.
#include "stats_common.h"

namespace {

struct WinJob {
  long long row0, valid, nprime;  // stream rows of this file; rows used
  int head, tail;                 // which boundary windows this call owns (else they stay zero:
                                  // another rank holds that end of the recording)
};

__global__ void gather_windows_kernel(const float* __restrict__ x, long long ld, int c, int hw,
                                      const WinJob* __restrict__ jobs, float* __restrict__ win,
                                      long long first_slot) {
  const WinJob j = jobs[blockIdx.x];
  const int which = blockIdx.y;  // 0 head, 1 tail
  float* dst = win + ((first_slot + blockIdx.x) * 2 + which) * (long long)(2 * hw) * c;
  const long long base = which == 0 ? -hw : j.nprime - hw;
  const bool own = which == 0 ? j.head != 0 : j.tail != 0;
  for (int idx = threadIdx.x; idx < 2 * hw * c; idx += blockDim.x) {
    const int r = idx / c, col = idx % c;
    const long long u = base + r;
    dst[idx] = (own && u >= 0 && u < j.valid) ? x[(j.row0 + u) * ld + col] : 0.f;
  }
}

// The all-ones row of [y | 1]^T x~ (the bias moments, lagged column sums of x) for the files
// just added, from their column sums over the rows that enter the fit and their boundary
// windows (x~ zero-extended outside the file):
//   sum_{t=0}^{N'-1} x~[t+e] = colsum[0,N') - sum_{v<e} x[v] + sum_{v=N'}^{N'+e-1} x~[v]   (e > 0)
//                            = colsum[0,N') - sum_{v=N'+e}^{N'-1} x[v]                     (e < 0)
// g is [l][rows][c]; the ones row is row `row`.
// Two launches: (file, lag, channel) contributions in parallel, then a fixed-order sum over
// the files.
__global__ void ones_contrib_kernel(int c, int l, int e_min, const double* __restrict__ colsum_seg,
                                    const float* __restrict__ win, int hw, long long first_slot,
                                    double* __restrict__ contrib) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= l * c) return;
  const int f = blockIdx.y;
  const int k = idx / c, j = idx % c;
  const int e = e_min + k;
  double v = colsum_seg[(size_t)f * c + j];
  const float* head = win + ((first_slot + f) * 2 + 0) * (long long)(2 * hw) * c;
  const float* tail = win + ((first_slot + f) * 2 + 1) * (long long)(2 * hw) * c;
  for (int m = 0; m < e; ++m)
    v += (double)tail[(long long)(m + hw) * c + j] - (double)head[(long long)(m + hw) * c + j];
  for (int m = e; m < 0; ++m) v -= (double)tail[(long long)(m + hw) * c + j];
  contrib[(size_t)f * l * c + idx] = v;
}

// g is [l][rows][c]; the ones row is row `row`.
__global__ void ones_rows_kernel(double* __restrict__ g, int rows, int row, int c, int l,
                                 const double* __restrict__ contrib, int n_files) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= l * c) return;
  const int k = idx / c, j = idx % c;
  double s = 0.0;
  for (int f = 0; f < n_files; ++f) s += contrib[(size_t)f * l * c + idx];
  g[((long long)k * rows + row) * c + j] += s;
}

// Launches both; `contrib` is caller-provided device memory of n_files * l * c doubles.
inline void launch_ones_rows(td_handle* h, double* g, int rows, int row, int c, int l, int e_min,
                             const double* colsum_seg, const float* win, int hw, long long first_slot,
                             int n_files, double* contrib) {
  const unsigned bx = (unsigned)td_ceil_div((int64_t)l * c, 256);
  hipLaunchKernelGGL(ones_contrib_kernel, dim3(bx, (unsigned)n_files), dim3(256), 0, h->stream, c, l,
                     e_min, colsum_seg, win, hw, first_slot, contrib);
  hipLaunchKernelGGL(ones_rows_kernel, dim3(bx), dim3(256), 0, h->stream, g, rows, row, c, l, contrib,
                     n_files);
}

// ---- one finalize launch per accumulate call -----------------------------------------------
// Everything an accumulate call does around its matrix kernels -- the float64 reductions of
// their partial slabs (with the lag-0 mirror), the column sums of y, the bias moments (the
// all-ones row of [y | 1]^T x~), the boundary windows and the frame count -- used to be a dozen
// launches of a few microseconds each with a launch gap in front of every one: ~75 us per call
// that do not shrink with the time range a rank holds, i.e. the strong-scaling ceiling of the
// accumulate (5.4x on 8 GPUs).  They are independent of each other once the matrix kernels have
// written their slabs, so they are ONE launch: workgroups take jobs by blockIdx range.  With
// `fresh` statistics (td_stats_reset pending) every job overwrites instead of adding and the
// memset of the reset goes away too.
constexpr int kFinThreads = 1024;
constexpr int kFinVecPhases = 8;    // slab phases of the float4 reduction (fin_reduce4)
constexpr int kFinMaxReduce = 5;      // F'xx + up to 4 target columns

struct FinalizeParams {
  LagReduceJob red[kFinMaxReduce];
  int red_q[kFinMaxReduce];           // slab phases per output: 4 (256 outputs per workgroup) or 16 (64)
  int red_block0[kFinMaxReduce + 1];  // first workgroup of each reduction
  int n_red;
  // column sums of y: sy[i] (+)= sum_w ysum[i][w]     (one workgroup per target column)
  const double* ysum[4];
  int ys_cols, ys_n_work, ys_accumulate;
  double* sy;
  // the all-ones row (bias moments) of gxo [l][rows][c], one workgroup per lag
  int ones_l;                         // 0 = none
  const double* csum;                 // [n_work][cs_pad] per-slab column sums of x over the rows summed
  int cs_n_work, cs_pad;
  const float* x;                     // the stream itself: the file ends are read in place
  long long ldx;
  const WinJob* jobs;
  int n_files, c, e_min, rows, row, ones_accumulate;
  double* gxo;
  // boundary windows of the new files (two workgroups per file)
  float* win;                         // null = none
  int hw;
  long long first_slot;
  // ... and of the second view (CCA): its own stream, rows and channel count
  float* win2;
  const float* x2;
  long long ldx2;
  const WinJob* jobs2;
  int c2;
  // the Gram reduction of the one-pass CCA accumulate (64 outputs x 16 slab phases per workgroup)
  GramReduceJob gram;
  int b_win2, b_gram, n_blocks;
  // frame count
  double* n_dst;
  double n_value;
  unsigned* zero_tab;                 // the channel-maximum table of the NEXT call (float16 kernel), or null
  int b_ysum, b_ones, b_win;          // first workgroup of each job kind
};

__device__ __forceinline__ void fin_reduce(const LagReduceJob& jb, int q_phases, int block,
                                           double* part) {
  const int outs_per = kFinThreads / q_phases;
  const int ol = threadIdx.x % outs_per, q = threadIdx.x / outs_per;
  const long long total = (long long)jb.e_count * jb.ca_eff * jb.cb;
  // (slabs of the virtual-image kernel: td_virt_offset says where an output's sums are)
  const size_t slab = jb.vmap ? (size_t)jb.slab_elems : (size_t)jb.e_pad * jb.ca_pad * jb.cb_pad;
  const long long o = (long long)block * outs_per + ol;
  double s = 0.0;
  int j = 0, i = 0, e = 0;
  if (o < total) {
    j = (int)(o % jb.cb);
    i = (int)((o / jb.cb) % jb.ca_eff);
    e = (int)(o / ((long long)jb.cb * jb.ca_eff));
    // a symmetric lag-0 block takes the sums of its upper triangle on both sides
    const bool flip = jb.mirror && e == 0 && i > j;
    const int is = flip ? j : i, js = flip ? i : j;
    const size_t off = jb.vmap ? (size_t)td_virt_offset(jb.vmap, e, is, js)
                               : ((size_t)e * jb.ca_pad + is) * jb.cb_pad + js;
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};       // eight loads in flight
    int w = q;
    if (jb.is_f64) {
      const double* src = reinterpret_cast<const double*>(jb.partial) + off;
      for (; w + 7 * q_phases < jb.n_work; w += 8 * q_phases) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = src[(size_t)(w + k * q_phases) * slab];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] += v[k];
      }
      for (; w < jb.n_work; w += q_phases) a[0] += src[(size_t)w * slab];
    } else {
      const float* src = reinterpret_cast<const float*>(jb.partial) + off;
      for (; w + 7 * q_phases < jb.n_work; w += 8 * q_phases) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = src[(size_t)(w + k * q_phases) * slab];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] += (double)v[k];
      }
      for (; w < jb.n_work; w += q_phases) a[0] += (double)src[(size_t)w * slab];
    }
    const double s0 = a[0] + a[4], s1 = a[1] + a[5], s2 = a[2] + a[6], s3 = a[3] + a[7];
    s = (s0 + s1) + (s2 + s3);
  }
  part[q * outs_per + ol] = s;
  __syncthreads();
  if (q == 0 && o < total) {
    double t = 0.0;
    for (int k = 0; k < q_phases; ++k) t += part[k * outs_per + ol];
    // float16 kernel: the sums carry the two channels' power-of-two scales
    if (jb.scale_a) {
      t = ldexp(t, -(td_f16_scale_exp(jb.scale_a[i]) + td_f16_scale_exp(jb.scale_b[j])));
      // an infinity or a NaN in either channel: what float32 arithmetic would have made of it
      if (td_chan_not_finite(jb.scale_a[i]) || td_chan_not_finite(jb.scale_b[j])) t = __builtin_nan("");
    }
    double* dst = jb.g + ((long long)e * jb.ca_dst + i) * jb.ldg + j;
    *dst = jb.accumulate ? *dst + t : t;
  }
}

// The same for float32 slabs whose rows are whole float4s: a thread sums FOUR consecutive outputs
// (16-byte loads: 64 KB in flight per CU instead of 16) in q_phases = 8 slab phases, 512 outputs
// per workgroup.  The lag-0 mirror needs no transposed reads here: the thread that holds (i, j),
// j > i, of a symmetric block also writes (j, i), and the lower half's own sums are dropped.
__device__ __forceinline__ void fin_reduce4(const LagReduceJob& jb, int block, double* part) {
  constexpr int Q = kFinVecPhases, kGroups = kFinThreads / Q;       // groups of 4 outputs
  const int ol = threadIdx.x % kGroups, q = threadIdx.x / kGroups;
  const long long total = (long long)jb.e_count * jb.ca_eff * jb.cb;
  const size_t slab = (size_t)jb.e_pad * jb.ca_pad * jb.cb_pad;
  const long long o = ((long long)block * kGroups + ol) * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int j = 0, i = 0, e = 0;
  if (o < total) {
    j = (int)(o % jb.cb);
    i = (int)((o / jb.cb) % jb.ca_eff);
    e = (int)(o / ((long long)jb.cb * jb.ca_eff));
    const float* src = reinterpret_cast<const float*>(jb.partial) + ((size_t)e * jb.ca_pad + i) * jb.cb_pad + j;
    double a[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int k = 0; k < 4; ++k) a[c][k] = 0.0;
    int w = q;
    for (; w + 3 * Q < jb.n_work; w += 4 * Q) {
      float4 v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = *reinterpret_cast<const float4*>(src + (size_t)(w + c * Q) * slab);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        a[c][0] += (double)v[c].x; a[c][1] += (double)v[c].y; a[c][2] += (double)v[c].z; a[c][3] += (double)v[c].w;
      }
    }
    for (; w < jb.n_work; w += Q) {
      const float4 v = *reinterpret_cast<const float4*>(src + (size_t)w * slab);
      a[0][0] += (double)v.x; a[0][1] += (double)v.y; a[0][2] += (double)v.z; a[0][3] += (double)v.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = (a[0][k] + a[1][k]) + (a[2][k] + a[3][k]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) part[(q * kGroups + ol) * 4 + k] = s[k];
  __syncthreads();
  if (q == 0 && o < total) {
    const bool sym = jb.mirror && e == 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double t = 0.0;
#pragma unroll
      for (int ph = 0; ph < Q; ++ph) t += part[(ph * kGroups + ol) * 4 + k];
      const int jj = j + k;
      if (jb.scale_a) {
        t = ldexp(t, -(td_f16_scale_exp(jb.scale_a[i]) + td_f16_scale_exp(jb.scale_b[jj])));
        if (td_chan_not_finite(jb.scale_a[i]) || td_chan_not_finite(jb.scale_b[jj])) t = __builtin_nan("");
      }
      if (sym && jj < i) continue;                     // written by the holder of (jj, i)
      double* dst = jb.g + ((long long)e * jb.ca_dst + i) * jb.ldg + jj;
      *dst = jb.accumulate ? *dst + t : t;
      if (sym && jj > i) {
        double* low = jb.g + ((long long)e * jb.ca_dst + jj) * jb.ldg + i;
        *low = jb.accumulate ? *low + t : t;
      }
    }
  }
}

// x~[u] of a file for the bias moments: zero outside the file and at an end another rank owns
__device__ __forceinline__ double fin_edge(const FinalizeParams& p, const WinJob& jw, long long u,
                                           bool own, int col) {
  return (own && u >= 0 && u < jw.valid) ? (double)p.x[(jw.row0 + u) * p.ldx + col] : 0.0;
}

// gram_reduce_kernel (lagcov.hip) as a finalize job: block t of the partial slabs is the t-th pair
// (gi <= gj) of 16-column groups of z = [x | x2 | 1]; element (i, j) goes to both triangles.
__device__ __forceinline__ void fin_gram(const GramReduceJob& jb, int block, double* part) {
  const int ol = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int o = block * 64 + ol;
  const size_t stride = (size_t)jb.n_groups * (jb.n_groups + 1) / 2 * 256;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  int wk = q;
  for (; wk + 48 < jb.n_slabs; wk += 64) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] += (double)jb.partial[(size_t)(wk + 16 * k) * stride + o];
  }
  for (; wk < jb.n_slabs; wk += 16) a[0] += (double)jb.partial[(size_t)wk * stride + o];
  part[q * 64 + ol] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (q != 0) return;
  double v = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) v += part[k * 64 + ol];
  int t = o >> 8, gi = 0;
  while (t >= jb.n_groups - gi) { t -= jb.n_groups - gi; ++gi; }
  const int gj = gi + t;
  const int i = gi * 16 + ((o >> 4) & 15), j = gj * 16 + (o & 15);   // columns of z
  const int ones = 16 * jb.n_groups - 1;
  if (i > j) return;                                 // diagonal blocks hold both triangles
  auto put = [&](double* dst) { *dst = jb.accumulate ? *dst + v : v; };
  if (j < 64) {                                      // x^T x
    if (j < jb.c1) {
      put(jb.fxx + (size_t)i * jb.c1 + j);
      if (i != j) put(jb.fxx + (size_t)j * jb.c1 + i);
    }
  } else if (i < 64) {                               // x^T [x2 | 1]
    if (i < jb.c1) {
      if (j - 64 < jb.c2) put(jb.gxy + (size_t)i * jb.c2 + (j - 64));
      else if (j == ones) put(jb.sx + i);
    }
  } else {                                           // [x2 | 1]^T [x2 | 1]
    const int aa = i - 64, bb = j - 64;
    if (bb < jb.c2) {
      put(jb.fyy + (size_t)aa * jb.c2 + bb);
      if (aa != bb) put(jb.fyy + (size_t)bb * jb.c2 + aa);
    } else if (j == ones && aa < jb.c2) {
      put(jb.sx2 + aa);
    }
  }
}

__device__ __forceinline__ void stats_finalize_body(const FinalizeParams& p, const int b, double* part) {
  const int tid = threadIdx.x;
  if (b == 0 && tid == 0 && p.n_dst) *p.n_dst = p.n_value;
  if (b == 0 && p.zero_tab)
    for (int i = tid; i < kChanTab; i += kFinThreads) p.zero_tab[i] = 0u;
  if (b < p.b_ysum) {                                   // ---- slab reductions
    int r = 0;
    while (r + 1 < p.n_red && b >= p.red_block0[r + 1]) ++r;
    if (p.red_q[r] == 0) fin_reduce4(p.red[r], b - p.red_block0[r], part);     // (0 = the float4 form)
    else fin_reduce(p.red[r], p.red_q[r], b - p.red_block0[r], part);
    return;
  }
  if (b < p.b_ones) {                                   // ---- column sum of one target column
    const int i = b - p.b_ysum;
    double s = 0.0;
    for (int w = tid; w < p.ys_n_work; w += kFinThreads) s += p.ysum[i][w];
    part[tid] = s;
    __syncthreads();
    for (int off = kFinThreads / 2; off > 0; off >>= 1) {
      if (tid < off) part[tid] += part[tid + off];
      __syncthreads();
    }
    if (tid == 0) p.sy[i] = p.ys_accumulate ? p.sy[i] + part[0] : part[0];
    return;
  }
  if (b < p.b_win) {                                    // ---- bias moments of one lag
    // sum_f sum_{t < N'_f} x~_f[t + e] = (column sum of every row summed) + sum_f corr_f(e):
    //   e > 0: corr = - sum_{v < e} x~[v] + sum_{v = N'}^{N' + e - 1} x~[v]
    //   e < 0: corr = - sum_{v = N' + e}^{N' - 1} x~[v]
    const int k = b - p.b_ones, e = p.e_min + k;
    const int j = tid & 63, q = tid >> 6;               // 16 phases; c <= 64
    double s = 0.0;
    if (j < p.c) {
      double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // eight loads in flight
      int w = q;
      for (; w + 7 * 16 < p.cs_n_work; w += 8 * 16) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p.csum[(size_t)(w + 16 * k) * p.cs_pad + j];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] += v[k];
      }
      for (; w < p.cs_n_work; w += 16) a[0] += p.csum[(size_t)w * p.cs_pad + j];
      s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
      if (p.n_files >= 32) {
        // many recordings: a phase per recording, the (<= 2 x 31) edge rows of one in sequence
        for (int f = q; f < p.n_files; f += 16) {
          const WinJob jw = p.jobs[f];
          double v = 0.0;
          for (int m = 0; m < e; ++m)
            v += fin_edge(p, jw, jw.nprime + m, jw.tail != 0, j) - fin_edge(p, jw, m, jw.head != 0, j);
          for (int m = e; m < 0; ++m) v -= fin_edge(p, jw, jw.nprime + m, jw.tail != 0, j);
          s += v;
        }
      } else {
        // few recordings (a C2 call has 10, a rank's share of a strong-scaled job 2): the phases split
        // the edge ROWS -- with a phase per recording one thread walked 62 dependent loads while 14 of
        // the 16 phases idled, and this job (~20 us) was the long pole of the finalize launch of a
        // short call (22 us at a 1/8 share, whose slab reduction needs 8)
        for (int f = 0; f < p.n_files; ++f) {
          const WinJob jw = p.jobs[f];
          double v = 0.0;
          for (int m = q; m < e; m += 16)
            v += fin_edge(p, jw, jw.nprime + m, jw.tail != 0, j) - fin_edge(p, jw, m, jw.head != 0, j);
          for (int m = e + q; m < 0; m += 16) v -= fin_edge(p, jw, jw.nprime + m, jw.tail != 0, j);
          s += v;
        }
      }
    }
    part[q * 64 + j] = s;
    __syncthreads();
    if (q == 0 && j < p.c) {
      double t = 0.0;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) t += part[kk * 64 + j];
      double* dst = p.gxo + ((long long)k * p.rows + p.row) * p.c + j;
      *dst = p.ones_accumulate ? *dst + t : t;
    }
    return;
  }
  if (b >= p.b_gram && p.n_blocks) {                    // ---- one-pass CCA: the Gram reduction
    fin_gram(p.gram, b - p.b_gram, part);
    return;
  }
  const bool second = p.win2 && b >= p.b_win2;          // ---- boundary windows of one file end
  float* win = second ? p.win2 : p.win;
  if (win) {
    const int rel = b - (second ? p.b_win2 : p.b_win);
    const int f = rel >> 1, which = rel & 1;
    const WinJob jw = second ? p.jobs2[f] : p.jobs[f];
    const float* src = second ? p.x2 : p.x;
    const long long ld = second ? p.ldx2 : p.ldx;
    const int c = second ? p.c2 : p.c;
    float* dst = win + ((p.first_slot + f) * 2 + which) * (long long)(2 * p.hw) * c;
    const long long base = which == 0 ? -p.hw : jw.nprime - p.hw;
    const bool own = which == 0 ? jw.head != 0 : jw.tail != 0;
    for (int idx = tid; idx < 2 * p.hw * c; idx += kFinThreads) {
      const int r = idx / c, col = idx % c;
      const long long u = base + r;
      dst[idx] = (own && u >= 0 && u < jw.valid) ? src[(jw.row0 + u) * ld + col] : 0.f;
    }
  }
}

__global__ __launch_bounds__(kFinThreads) void stats_finalize_kernel(FinalizeParams p) {
  __shared__ double part[4 * kFinThreads];
  stats_finalize_body(p, blockIdx.x, part);
}

// Several finalize launches in one (td_stats_accumulate_each: one parameter block per recording): workgroup b
// belongs to the block whose range [first[i], first[i + 1]) holds it.
__global__ __launch_bounds__(kFinThreads) void stats_finalize_multi_kernel(const FinalizeParams* __restrict__ params,
                                                                          const int* __restrict__ first, int n) {
  __shared__ double part[4 * kFinThreads];
  __shared__ __attribute__((aligned(16))) int sp_raw[(sizeof(FinalizeParams) + sizeof(int) - 1) / sizeof(int)];
  const int b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= b) lo = mid; else hi = mid - 1;
  }
  // (the block through LDS: every thread reads its fields from there, not from a per-thread copy)
  const int words = (int)(sizeof(FinalizeParams) / sizeof(int));
  const int* src = reinterpret_cast<const int*>(params + lo);
  for (int i = threadIdx.x; i < words; i += kFinThreads) sp_raw[i] = src[i];
  __syncthreads();
  stats_finalize_body(*reinterpret_cast<const FinalizeParams*>(sp_raw), b - first[lo], part);
}

// The description of one finalize launch, filled in the order of its workgroup ranges:
// [reductions | sum y per target column | ones row per lag | windows of x | windows of x2 | Gram reduction].
struct FinalizeBuilder {
  FinalizeParams fp;
  int blocks = 0;
  FinalizeBuilder() { memset(&fp, 0, sizeof(fp)); }

  // the stream whose file ends the ones rows and the windows read, and its file table on the device
  void files(const WinJob* jobs_dev, const float* x, int64_t ldx, int c, int n_files, int hw) {
    fp.jobs = jobs_dev;
    fp.x = x; fp.ldx = ldx; fp.c = c; fp.n_files = n_files; fp.hw = hw;
  }
  void add_reduce(const LagReduceJob& job) {
    const long long outs = (long long)job.e_count * job.ca_eff * job.cb;
    const bool vec = !job.is_f64 && !job.vmap && outs >= 32768 && job.cb % 4 == 0 && job.cb_pad % 4 == 0 &&
                     (reinterpret_cast<uintptr_t>(job.partial) & 15) == 0;
    // (16 slab phases x 64 outputs per workgroup for small jobs -- and for virtual-image slabs up to 32 x 32 x 32,
    // whose reduction was the long pole of the 32-channel call: 35 us with 4 phases)
    const int q = vec ? 0 : (outs < 32768 || (job.vmap && outs <= 65536)) ? 16 : 4;
    fp.red[fp.n_red] = job;
    fp.red_q[fp.n_red] = q;
    fp.red_block0[fp.n_red] = blocks;
    blocks += (int)td_ceil_div(outs, vec ? 4 * (kFinThreads / kFinVecPhases) : kFinThreads / q);
    fp.red_block0[++fp.n_red] = blocks;
    fp.b_ysum = fp.b_ones = fp.b_win = blocks;
  }
  // sum y and the ones rows of gxo from the slabs [t0, t1) of a targets launch (after the last reduction)
  void add_targets(const td_stats* s, const TargetsOutputs& to, int t0, int t1, bool accumulate) {
    for (int i = 0; i < s->d; ++i) fp.ysum[i] = to.ysum[i] + t0;
    fp.ys_n_work = t1 - t0;
    fp.ys_cols = s->d; fp.ys_accumulate = accumulate ? 1 : 0;
    fp.sy = s->g + s->off_sy;
    blocks += s->d;
    fp.b_ones = blocks;
    fp.ones_l = s->l1;
    fp.csum = to.csum + (size_t)t0 * to.cb_pad; fp.cs_n_work = t1 - t0; fp.cs_pad = to.cb_pad;
    fp.e_min = -s->pre1; fp.rows = s->d + 1; fp.row = s->d; fp.ones_accumulate = accumulate ? 1 : 0;
    fp.gxo = s->g + s->off_gxo;
    blocks += s->l1;
    fp.b_win = blocks;
  }
  // the boundary windows of the new files of files() (after the targets)
  void add_windows(float* win, int64_t first_slot) {
    fp.win = win; fp.first_slot = first_slot;
    blocks += 2 * fp.n_files;
  }
  // ... of the second view, and the Gram reduction td_gram left in fp.gram (the one-pass CCA accumulate)
  void add_second_view(const WinJob* jobs2_dev, const float* x2, int64_t ldx2, int c2, float* win2) {
    fp.jobs2 = jobs2_dev;
    fp.x2 = x2; fp.ldx2 = ldx2; fp.c2 = c2; fp.win2 = win2;
    fp.b_win2 = blocks;
    blocks += 2 * fp.n_files;
    fp.b_gram = blocks;
    const int pairs = fp.gram.n_groups * (fp.gram.n_groups + 1) / 2;
    blocks += pairs * 256 / 64;
    fp.n_blocks = blocks;
  }
  void set_count(const td_stats* s, double frames) {     // (n travels in the all-reduce)
    fp.n_dst = s->g + s->off_n;
    fp.n_value = frames;
  }
};

int launch_finalize(td_handle* h, const FinalizeParams& fp, int blocks) {
  hipLaunchKernelGGL(stats_finalize_kernel, dim3((unsigned)blocks), dim3(kFinThreads), 0, h->stream, fp);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

// What one accumulate call sums, per file: the rows of the four products, the window jobs of both views,
// the rows that enter the sums and whether the file is summed whole (td_stats::whole_files).
struct FileRows {
  std::vector<LagSeg> sxx, syx, syy, sxy;   // A = B = x | A = y, B = x | A = B = x2 | A = x, B = x2
  std::vector<WinJob> j1, j2;
  std::vector<int64_t> frames;
  std::vector<char> whole;
  int64_t new_frames = 0;
};

// all_whole (may be null) is cleared at the first file that is not summed whole.
int file_rows(td_handle* h, const int64_t* file_offsets_host, int num_files, int input_offset,
              const int64_t* rows_used_host, const int64_t* range_begin_host, const int64_t* range_end_host,
              const int* edge_flags_host, bool* all_whole, FileRows* out) {
  const int64_t dx = input_offset > 0 ? input_offset : 0;    // rows dropped from x
  const int64_t dy = input_offset < 0 ? -input_offset : 0;   // rows dropped from x2 and y
  out->j1.resize(num_files); out->j2.resize(num_files);
  out->frames.resize(num_files); out->whole.resize(num_files);
  for (int f = 0; f < num_files; ++f) {
    const int64_t r0 = file_offsets_host[f], r1 = file_offsets_host[f + 1];
    TD_REQUIRE(h, r1 >= r0, "file_offsets must be non-decreasing");
    const int64_t nf = r1 - r0;
    const int64_t vx = nf - dx > 0 ? nf - dx : 0;
    const int64_t vy = nf - dy > 0 ? nf - dy : 0;
    // zip() of the four streams truncates to the shortest; the attention stream
    // is never shifted (brain_data.py:466-483).
    int64_t nz = vx < vy ? vx : vy;
    if (nf < nz) nz = nf;
    int64_t np = nz;
    if (rows_used_host) {
      TD_REQUIRE(h, rows_used_host[f] >= 0 && rows_used_host[f] <= nz,
                 "rows_used[%d] = %lld outside [0, %lld]", f, (long long)rows_used_host[f],
                 (long long)nz);
      np = rows_used_host[f];
    }
    // the rows [ub, ue) of the file that THIS call sums (all of [0, N') by default): the sums
    // are additive over disjoint row ranges, so ranks can share one long recording
    int64_t ub = 0, ue = np;
    if (range_begin_host) {
      ub = range_begin_host[f]; ue = range_end_host[f];
      TD_REQUIRE(h, ub >= 0 && ub <= ue && ue <= np, "range [%lld, %lld) of file %d outside [0, %lld]",
                 (long long)ub, (long long)ue, f, (long long)np);
    }
    out->frames[f] = ue - ub;
    out->new_frames += ue - ub;
    LagSeg a;
    a.a_row0 = r0 + dx; a.a_valid = vx; a.b_row0 = r0 + dx; a.b_valid = vx;
    a.u_begin = ub; a.u_end = ue;
    out->sxx.push_back(a);
    LagSeg b;   // A = y stream, B = x
    b.a_row0 = r0 + dy; b.a_valid = vy; b.b_row0 = r0 + dx; b.b_valid = vx;
    b.u_begin = ub; b.u_end = ue;
    out->syx.push_back(b);
    LagSeg c;   // A = B = x2
    c.a_row0 = r0 + dy; c.a_valid = vy; c.b_row0 = r0 + dy; c.b_valid = vy;
    c.u_begin = ub; c.u_end = ue;
    out->syy.push_back(c);
    LagSeg e;   // A = x, B = x2
    e.a_row0 = r0 + dx; e.a_valid = vx; e.b_row0 = r0 + dy; e.b_valid = vy;
    e.u_begin = ub; e.u_end = ue;
    out->sxy.push_back(e);
    const int flags = edge_flags_host ? edge_flags_host[f] : 3;
    out->whole[f] = (ub == 0 && ue == np && np == vx && flags == 3) ? 1 : 0;
    if (all_whole && !out->whole[f]) *all_whole = false;
    WinJob& w1 = out->j1[f];
    w1.row0 = r0 + dx; w1.valid = vx; w1.nprime = np;
    w1.head = flags & 1; w1.tail = flags & 2;
    WinJob& w2 = out->j2[f];
    w2.row0 = r0 + dy; w2.valid = vy; w2.nprime = np;
    w2.head = flags & 1; w2.tail = flags & 2;
  }
  return TD_OK;
}

// A device block the statistics own (dscratch, djobs: what a deferred finalize reads).  Too small for `need`
// bytes: the device is drained (kernels of other streams may still read the old block) and a block of `grown`
// bytes replaces it.
int grow_owned_block(td_handle* h, void** block, size_t* bytes, size_t need, size_t grown) {
  if (need <= *bytes) return TD_OK;
  if (*block) { TD_HIP(h, hipDeviceSynchronize()); TD_HIP(h, hipFree(*block)); }
  *block = nullptr; *bytes = 0;
  TD_HIP(h, hipMalloc(block, grown));
  *bytes = grown;
  return TD_OK;
}

}  // namespace

extern "C" {

int td_stats_accumulate(td_handle* h, td_stats* s, const float* x_dev, int64_t ldx,
                        const float* x2_dev, int64_t ldx2, const float* y_dev, int64_t ldy,
                        const int64_t* file_offsets_host, int num_files, int input_offset,
                        const int64_t* rows_used_host) {
  return td_stats_accumulate_parts(h, s, x_dev, ldx, x2_dev, ldx2, y_dev, ldy, file_offsets_host,
                                   num_files, input_offset, rows_used_host,
                                   TD_ACC_MAIN | TD_ACC_TARGETS);
}

int td_stats_accumulate_parts(td_handle* h, td_stats* s, const float* x_dev, int64_t ldx,
                              const float* x2_dev, int64_t ldx2, const float* y_dev, int64_t ldy,
                              const int64_t* file_offsets_host, int num_files, int input_offset,
                              const int64_t* rows_used_host, int parts) {
  return td_stats_accumulate_ranges(h, s, x_dev, ldx, x2_dev, ldx2, y_dev, ldy, file_offsets_host,
                                    num_files, input_offset, rows_used_host, nullptr, nullptr,
                                    nullptr, parts);
}

// Auto-covariance G[e] = x~^T shift_e(x~), e = 0 .. l-1, accumulated into g [l][c][c].  Up to
// 64 channels it is one td_lagcov call (the split kernel, float16 form).
//
// 65 .. 128 channels (the codelab's 69): the fast kernel wants ONE 64-channel tile with 16-byte
// rows on both sides of the product, and 69 floats per row are neither.  The channels are cut
// into tiles of 32; every unordered PAIR of tiles (i < j) is gathered into a dense [rows][64]
// copy (tile i | tile j, zeros past channel c) and goes through the split kernel as a 64-channel
// stream of its own: its lag matrices hold the blocks (i,i) (i,j) (j,i) (j,j), which are added
// into g where they belong -- a diagonal block from one pass only.  3 passes for <= 96 channels,
// 6 for <= 128, each at the speed of the aligned 64-channel case; the copies cost a read and a
// write of the input per pass.  (Before: two diagonal 64-channel blocks on the unaligned bf16x3
// path and two off-diagonal ones on the float32 matrix kernel with A and B at different
// channels of the same rows -- 1.15 ms of the codelab accumulate's 2.0; it remains the fallback,
// lagcov_auto_blocks.)
// (Inside extern "C": the two kernels keep the unmangled symbols they have always had.)
namespace {
// out[r][k] = x[row_lo + r][32 (k < 32 ? ti : tj) + (k & 31)], zero past channel c; the largest
// magnitude of every column of the copy goes into tab (the float16 kernel's channel scales:
// chan_max_kernel's table, lag_util.hip)
__global__ __launch_bounds__(256) void gather_tile_pair_kernel(const float* __restrict__ x, long long ldx,
                                                               int c, long long row_lo, long long rows,
                                                               int ti, int tj, float* __restrict__ out,
                                                               unsigned* __restrict__ tab) {
  __shared__ unsigned red[4][64];
  const int k = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int ch = 32 * (k < 32 ? ti : tj) + (k & 31);
  const bool ok = ch < c;
  unsigned m = 0u;
  long long r = blockIdx.x * 4LL + rg;
  const long long stride = 4LL * gridDim.x;
  for (; r + 3 * stride < rows; r += 4 * stride) {       // four rows in flight per thread
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = ok ? x[(row_lo + r + q * stride) * ldx + ch] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      out[(r + q * stride) * 64 + k] = v[q];
      m = max(m, __float_as_uint(v[q]) & 0x7fffffffu);
    }
  }
  for (; r < rows; r += stride) {
    const float v = ok ? x[(row_lo + r) * ldx + ch] : 0.f;
    out[r * 64 + k] = v;
    m = max(m, __float_as_uint(v) & 0x7fffffffu);
  }
  if (!tab) return;
  red[rg][k] = m;
  __syncthreads();
  if (rg == 0) {
    m = max(max(red[0][k], red[1][k]), max(red[2][k], red[3][k]));
    if (m) atomicMax(tab + (blockIdx.x % kChanShards) * 128 + k, m);
  }
}

// g [l][c][c] += the blocks of tmp [l][64][64] (a pass over tiles ti | tj); diag bit 0 / 1: the
// pass owns the diagonal block of ti / tj
__global__ __launch_bounds__(256) void scatter_tile_pair_kernel(const double* __restrict__ tmp, int l, int c,
                                                                int ti, int tj, int diag,
                                                                double* __restrict__ g) {
  const long long total = (long long)l * 64 * 64;
  for (long long o = blockIdx.x * 256LL + threadIdx.x; o < total; o += 256LL * gridDim.x) {
    const int j = (int)(o & 63), i = (int)((o >> 6) & 63), e = (int)(o >> 12);
    const int bi = i >> 5, bj = j >> 5;
    if (bi == bj && !((diag >> bi) & 1)) continue;
    const int ci = 32 * (bi ? tj : ti) + (i & 31), cj = 32 * (bj ? tj : ti) + (j & 31);
    if (ci >= c || cj >= c) continue;
    g[((long long)e * c + ci) * c + cj] += tmp[o];
  }
}

int lagcov_auto_blocks(td_handle* h, const float* x, int64_t ldx, int c, const std::vector<LagSeg>& segs,
                       int l, double* g) {
  const int c1 = c - 64;
  TD_TRY(td_lagcov(h, x, ldx, 64, false, x, ldx, 64, segs, 0, l, g, true, c, c));
  TD_TRY(td_lagcov(h, x + 64, ldx, c1, false, x + 64, ldx, c1, segs, 0, l, g + (size_t)64 * c + 64, true,
                   c, c));
  TD_TRY(td_lagcov(h, x, ldx, 64, false, x + 64, ldx, c1, segs, 0, l, g + 64, true, c, c));
  TD_TRY(td_lagcov(h, x + 64, ldx, c1, false, x, ldx, 64, segs, 0, l, g + (size_t)64 * c, true, c, c));
  // (the lag-0 matrix is promised exactly symmetric: its two off-diagonal blocks come from two
  // launches)
  return td_mirror_upper(h, g, c, c);
}

int lagcov_auto(td_handle* h, const float* x, int64_t ldx, int c, const std::vector<LagSeg>& segs,
                int l, double* g) {
  {
    // 9 .. 32 and 65 .. 128 channels, <= 64 lags: the float16 kernel on virtual images, no copies
    // (lagcov.hip)
    bool handled = false;
    TD_TRY(td_lagcov_virt(h, x, ldx, c, segs, l, g, true, &handled));
    if (handled) return TD_OK;
  }
  if (c <= 64 || c > 128)
    return td_lagcov(h, x, ldx, c, false, x, ldx, c, segs, 0, l, g, true, 0, 0, false, true);
  long long lo = 0, hi = 0;
  bool any = false, same = true;
  for (const LagSeg& sg : segs) {
    if (sg.a_row0 != sg.b_row0 || sg.a_valid != sg.b_valid) same = false;
    if (sg.a_valid <= 0) continue;
    if (!any || sg.a_row0 < lo) lo = sg.a_row0;
    if (!any || sg.a_row0 + sg.a_valid > hi) hi = sg.a_row0 + sg.a_valid;
    any = true;
  }
  // (more than 64 lags: not the split kernel's case; > 2^33 bytes of copy: the caller's arrays
  // of that size are cut into calls anyway)
  if (!any || !same || l > 64 || (hi - lo) > (1LL << 25)) return lagcov_auto_blocks(h, x, ldx, c, segs, l, g);
  const long long rows = hi - lo;
  std::vector<LagSeg> rel(segs);
  for (LagSeg& sg : rel) { sg.a_row0 -= lo; sg.b_row0 -= lo; }
  void* copy = nullptr;
  void* tmp = nullptr;
  TD_TRY(td_alloc_async(h, sizeof(float) * 64 * (size_t)rows, &copy));
  int rc = td_alloc_async(h, sizeof(double) * (size_t)l * 64 * 64, &tmp);
  if (rc != TD_OK) { td_free_async(h, copy, true); return rc; }
  const int nt = (c + 31) / 32;
  const unsigned gb = (unsigned)(td_ceil_div(rows, 16) > 2048 ? 2048 : td_ceil_div(rows, 16));
  for (int ti = 0; ti < nt && rc == TD_OK; ++ti)
    for (int tj = ti + 1; tj < nt && rc == TD_OK; ++tj) {
      const int diag = (tj == ti + 1 ? 1 : 0) | (ti == nt - 2 && tj == nt - 1 ? 2 : 0);
      // (the copy's channel maxima ride along: a table the float32 / bf16x3 forms simply ignore)
      unsigned* tab = nullptr;
      rc = td_chan_tab_scratch(h, &tab);
      if (rc != TD_OK) break;
      hipLaunchKernelGGL(gather_tile_pair_kernel, dim3(gb), dim3(256), 0, h->stream, x, (long long)ldx, c,
                         lo, rows, ti, tj, reinterpret_cast<float*>(copy), tab);
      const float* xc = reinterpret_cast<const float*>(copy);
      rc = td_lagcov(h, xc, 64, 64, false, xc, 64, 64, rel, 0, l, reinterpret_cast<double*>(tmp), false,
                     0, 0, false, true, tab);
      if (rc != TD_OK) break;
      hipLaunchKernelGGL(scatter_tile_pair_kernel, dim3((unsigned)td_ceil_div((long long)l * 4096, 256)),
                         dim3(256), 0, h->stream, reinterpret_cast<const double*>(tmp), l, c, ti, tj, diag,
                         g);
    }
  td_free_async(h, copy, true);
  td_free_async(h, tmp, true);
  TD_TRY(rc);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}
}  // namespace

}  // extern "C"

namespace {
// Regression statistics (stats_fusable): the matrix kernels of the call run out of ONE scratch
// block and ONE finalize launch does everything else (stats_finalize_kernel).  A call is
//   MAIN    : lagcov kernel (F'xx slabs)                      + finalize {reduce + mirror, windows, n}
//   TARGETS : one targets kernel per column (y^T x~, sums)    + finalize {reduces, sum y, bias row}
//   both    : the kernels of both                             + ONE finalize with all of it
// -- 3 launches for the C2 fit where there were 12 -- and fresh statistics are overwritten, so
// td_stats_reset queues nothing.
int accumulate_fused(td_handle* h, td_stats* s, const float* x_dev, int64_t ldx, const float* y_dev,
                     int64_t ldy, const std::vector<LagSeg>& sxx, const std::vector<LagSeg>& syx,
                     const std::vector<WinJob>& j1, int num_files, int64_t new_frames,
                     int64_t first_slot, bool do_main, bool do_targets, bool tgt_first, bool defer) {
  LagcovPlan mp;
  TargetsPlan tp;
  VirtPlan vp;                   // <= 32 channels: the float16 kernel on virtual images (lagcov.hip)
  Narrow16Plan np16;             // <= 16 channels: matrix + targets in one streaming kernel (lag_narrow16.hip)
  if (h->narrow16) TD_TRY(td_narrow16_plan(h, s->c1, s->d, s->pre1, s->l1, ldx, ldy, syx, &np16));
  const bool n16 = np16.ok;
  if (do_main && n16) TD_TRY(ensure_window_capacity(h, s, s->n_files + num_files));
  if (do_main && !n16) {
    TD_TRY(ensure_window_capacity(h, s, s->n_files + num_files));
    TD_TRY(td_lagcov_virt_plan(h, x_dev, ldx, s->c1, sxx, s->l1, &vp));
    mp.allow_f16 = true;         // the finalize launch divides the channel scales out
    if (!vp.ok) TD_TRY(td_lagcov_plan(h, x_dev, ldx, s->c1, false, x_dev, ldx, s->c1, sxx, 0, s->l1, &mp));
  }
  const bool virt = do_main && !n16 && vp.ok;
  // 3 launches and two reads of x: targets kernel (yT x~, column sums, channel maxima) -> lag kernel
  // -> finalize.  (A folded form once carried one target column inside the float16 lag kernel behind
  // a streaming pre-pass for the maxima and column sums.  Measured at C2, the targets cost the lag
  // kernel 42 us, 6 %, plus the 49 us pre-pass; as a pass of their own -- which is HBM-bound, has
  // the matrix pipe to spare and measures the channel maxima on the way -- they cost 62 us in all.
  // The folded form was removed.)
  if (do_targets && !n16) {
    TD_TRY(td_lagcov_targets_plan(h, y_dev, ldy, s->d, x_dev, ldx, s->c1, syx, -s->pre1, s->l1, &tp));
    TD_REQUIRE(h, tp.handled && tp.n_work > 0, "accumulate_fused: the targets kernel refused the shape");
  }
  const size_t main_bytes = n16 ? np16.scratch_bytes : virt ? vp.scratch_bytes
                            : do_main ? mp.scratch_bytes : 0;
  // TD_ACC_DEFER: the finalize launch is left to td_stats_complete (another stream, later): what it reads
  // then -- the partial slabs, the file table, the channel scales -- lives in blocks the statistics own,
  // not in the handle's scratch, which the next call of this stream overwrites.
  const bool deferred = defer && do_main && !virt;
  const size_t scratch_bytes = main_bytes + (do_targets && !n16 ? tp.scratch_bytes : 0);
  void* scratch = nullptr;
  if (deferred) {
    TD_TRY(grow_owned_block(h, &s->dscratch, &s->dscratch_bytes, scratch_bytes, scratch_bytes + scratch_bytes / 8));
    scratch = s->dscratch;
  } else {
    TD_TRY(td_scratch(h, scratch_bytes, &scratch));
  }
  char* base = reinterpret_cast<char*>(scratch);
  FinalizeBuilder fin;
  FinalizeParams& fp = fin.fp;
  const void* jobs_dev = nullptr;
  if (deferred) {
    const size_t jb = sizeof(WinJob) * num_files;
    if (jb > s->djobs_bytes) s->djobs_host.clear();
    TD_TRY(grow_owned_block(h, &s->djobs, &s->djobs_bytes, jb, jb * 2 < 4096 ? 4096 : jb * 2));
    // (uploaded only when it differs from what the block holds: a pipeline's fits usually share their file table,
    // and the copy would sit between the matrix kernel of one fit and the targets kernel of the next)
    if (s->djobs_host.size() != jb || memcmp(s->djobs_host.data(), j1.data(), jb) != 0) {
      s->djobs_host.clear();
      TD_TRY(td_upload_async(h, j1.data(), jb, s->djobs));
      s->djobs_host.assign(reinterpret_cast<const char*>(j1.data()), reinterpret_cast<const char*>(j1.data()) + jb);
    }
    jobs_dev = s->djobs;
  } else {
    TD_TRY(td_table_upload(h, j1.data(), sizeof(WinJob) * num_files, &jobs_dev));
  }
  fin.files(reinterpret_cast<const WinJob*>(jobs_dev), x_dev, ldx, s->c1, num_files, s->hw);
  TargetsOutputs to;
  // The targets kernels run first: they stream every row the lag kernel will touch, so the first
  // of them also measures the channel maxima the float16 lag kernel scales by (no pre-context:
  // with one the lag kernel reaches further past a range's end than the targets do, and it
  // measures for itself: chan_max_kernel).
  LagReduceJob job16;
  if (n16) {
    // one launch for whichever parts this call carries (the same sums whether they come together or apart)
    to.maxtab = nullptr;
    TD_TRY(td_narrow16_launch(h, &np16, x_dev, ldx, y_dev, ldy, base, do_main, do_targets, s->g + s->off_fxx,
                              !s->fresh_main, s->g + s->off_gxo, !s->fresh_tgt, &job16, &to));
  }
  if (do_targets && !n16) {
    to.maxtab = nullptr;
    if (do_main && (mp.f16 || virt) && s->pre1 == 0) {
      TD_TRY(td_chan_tab(h, &to.maxtab));
      mp.tab = to.maxtab;
    } else if (!do_main && tgt_first && s->pre1 == 0 && h->acc_mode == TD_ACC_F16X2) {
      // ahead of the MAIN call (which may run on another handle): the maxima go into the statistics'
      // own table, zeroed here in stream order
      if (!s->chan_tab) {
        void* p = nullptr;
        TD_TRY(td_alloc_async(h, sizeof(unsigned) * kChanTab, &p));
        s->chan_tab = reinterpret_cast<unsigned*>(p);
      }
      TD_HIP(h, hipMemsetAsync(s->chan_tab, 0, sizeof(unsigned) * kChanTab, h->stream));
      to.maxtab = s->chan_tab;
      s->tab_ready = true;
    }
    TD_TRY(td_lagcov_targets_launch(h, &tp, base + main_bytes, s->g + s->off_gxo, !s->fresh_tgt, &to));
  }
  if (do_main) {
    LagReduceJob job;
    // (the maxima a TARGETS_FIRST call of these files left in the statistics: no pre-pass here)
    const bool ahead = !do_targets && s->tab_ready && (mp.f16 || virt) && s->pre1 == 0;
    if (ahead) mp.tab = s->chan_tab;
    s->tab_ready = false;
    bool own_tab = false;
    if (n16) {
      job = job16;
    } else if (virt) {
      unsigned* tab = mp.tab;
      if (!tab) {
        // nobody measured the channel maxima on the way (a pre-context, a MAIN-only call): a pass of
        // its own over the rows of the array that hold this call's recordings
        TD_TRY(td_chan_tab_scratch(h, &tab));
        TD_TRY(td_chan_max_works(h, x_dev, ldx, s->c1, vp.works, tab));
        own_tab = true;
      }
      TD_TRY(td_lagcov_virt_launch(h, &vp, x_dev, ldx, base, tab, s->g + s->off_fxx, !s->fresh_main, &job));
    } else {
      if (deferred && mp.f16 && !ahead) {
        // (the finalize will run on another stream, later: the lag kernel leaves the channel scales in a block
        // of the statistics and zeroes the next call's channel table itself)
        if (!s->dscale) TD_HIP(h, hipMalloc(reinterpret_cast<void**>(&s->dscale), sizeof(unsigned) * 128));
        mp.scale_out = s->dscale;
        mp.zero_tab = h->chan_max + kChanTab * ((h->chan_phase + 1) & 1);
      }
      TD_TRY(td_lagcov_launch(h, &mp, base, s->g + s->off_fxx, !s->fresh_main, 0, 0, &job));
    }
    if (mp.scale_out && job.scale_a) job.scale_a = job.scale_b = mp.scale_out;
    fin.add_reduce(job);
    if ((mp.f16 || (virt && !own_tab)) && !ahead) {      // this call used table chan_phase & 1: clear the other for the next
      ++h->chan_phase;
      fp.zero_tab = mp.zero_tab ? nullptr : h->chan_max + kChanTab * (h->chan_phase & 1);
    }
    s->n_files += num_files;
    s->frames += new_frames;
    fin.set_count(s, (double)s->frames);
    s->fresh_main = false;
  }
  if (do_targets) {
    for (int i = 0; i < s->d; ++i) fin.add_reduce(to.jobs[i]);
    fin.add_targets(s, to, 0, to.n_work, !s->fresh_tgt);
    s->fresh_tgt = false;
  }
  if (do_main) fin.add_windows(s->win1, first_slot);
  const int blocks = fin.blocks;
  if (deferred) {
    // A finalize that would read or zero the HANDLE's channel table cannot wait for another stream (the next call
    // of this one overwrites the table): it is queued here, in the call, like an undeferred one -- the counters
    // above already describe a finished call either way.
    bool can_wait = !fp.zero_tab;
    for (int r = 0; r < fp.n_red; ++r)
      if (fp.red[r].scale_a && fp.red[r].scale_a != s->dscale &&
          !(s->chan_tab && fp.red[r].scale_a == s->chan_tab + kChanShards * 128))
        can_wait = false;
    if (can_wait) {
      s->pend_params.assign(reinterpret_cast<const char*>(&fp), reinterpret_cast<const char*>(&fp) + sizeof(fp));
      s->pend_blocks = blocks;
      s->pending = true;
      return TD_OK;
    }
  }
  return launch_finalize(h, fp, blocks);
}

// One accumulate over SEVERAL recordings that leaves every recording's statistics in an object of its own
// (the per-recording statistics of a leave-one-out sweep, regression.py:151-242: 32 calls of three small
// launches each were 2 of the 11.5 ms of a C5 sweep): ONE targets launch and ONE matrix launch over all the
// recordings -- the work items of the matrix kernel each belong to one recording and keep a partial slab of
// their own (no chains across items) -- and one finalize launch per recording over ITS slabs, target sums,
// boundary windows and frame count.  each[f]: freshly reset regression statistics of one layout, 33..64
// channels (the plain float16 / bfloat16 / float32 matrix kernels).  *handled = 0: not this shape, nothing
// was queued -- the caller accumulates recording by recording.
int accumulate_each(td_handle* h, td_stats* const* each, const float* x_dev, int64_t ldx, const float* y_dev,
                    int64_t ldy, const std::vector<LagSeg>& sxx, const std::vector<LagSeg>& syx,
                    const std::vector<WinJob>& j1, int num_files, const std::vector<int64_t>& frames,
                    const std::vector<char>& whole, int* handled) {
  *handled = 0;
  td_stats* s0 = each[0];
  for (int f = 0; f < num_files; ++f) {
    td_stats* s = each[f];
    if (!stats_fusable(s) || s->c1 != s0->c1 || s->pre1 != s0->pre1 || s->l1 != s0->l1 || s->d != s0->d ||
        s->n_files != 0 || s->frames != 0 || s->pending || frames[f] <= 0) {   // (empty: every sum is overwritten)
      *handled = -1;
      return TD_OK;
    }
    for (int g = 0; g < f; ++g)
      if (each[g] == s) { *handled = -2; return TD_OK; }
  }
  Narrow16Plan np16;
  if (h->narrow16) TD_TRY(td_narrow16_plan(h, s0->c1, s0->d, s0->pre1, s0->l1, ldx, ldy, syx, &np16));
  if (np16.ok) { *handled = -3; return TD_OK; }
  VirtPlan vp;
  TD_TRY(td_lagcov_virt_plan(h, x_dev, ldx, s0->c1, sxx, s0->l1, &vp));
  if (vp.ok) { *handled = -4; return TD_OK; }
  LagcovPlan mp;
  mp.allow_f16 = true;
  mp.no_chains = true;           // a partial slab per work item: the items of a recording are summed on their own
  TD_TRY(td_lagcov_plan(h, x_dev, ldx, s0->c1, false, x_dev, ldx, s0->c1, sxx, 0, s0->l1, &mp));
  TargetsPlan tp;
  TD_TRY(td_lagcov_targets_plan(h, y_dev, ldy, s0->d, x_dev, ldx, s0->c1, syx, -s0->pre1, s0->l1, &tp));
  if (!tp.handled || tp.n_work <= 0 || (int)mp.work_seg.size() != (int)mp.works.size()) { *handled = -5; return TD_OK; }
  *handled = 1;
  for (int f = 0; f < num_files; ++f) TD_TRY(ensure_window_capacity(h, each[f], 1));
  const size_t main_bytes = mp.scratch_bytes;
  // (behind the kernels' scratch: the recordings' finalize parameter blocks and their first workgroups)
  const size_t kern_bytes = td_round_up(main_bytes + tp.scratch_bytes, 256);
  const size_t pb = td_round_up(sizeof(FinalizeParams) * (size_t)num_files, 256);
  void* scratch = nullptr;
  TD_TRY(td_scratch(h, kern_bytes + pb + sizeof(int) * ((size_t)num_files + 1), &scratch));
  char* base = reinterpret_cast<char*>(scratch);
  const void* jobs_dev = nullptr;
  TD_TRY(td_table_upload(h, j1.data(), sizeof(WinJob) * num_files, &jobs_dev));
  TargetsOutputs to;
  to.maxtab = nullptr;
  if ((mp.f16) && s0->pre1 == 0) {
    TD_TRY(td_chan_tab(h, &to.maxtab));
    mp.tab = to.maxtab;
  }
  TD_TRY(td_lagcov_targets_launch(h, &tp, base + main_bytes, s0->g + s0->off_gxo, false, &to));
  LagReduceJob job;
  TD_TRY(td_lagcov_launch(h, &mp, base, s0->g + s0->off_fxx, false, 0, 0, &job));
  TD_REQUIRE(h, job.n_work == (int)mp.works.size() && !job.vmap, "accumulate_each: the matrix kernel merged work items");
  bool zero_next = false;
  if (mp.f16) { ++h->chan_phase; zero_next = true; }
  // first work item of every recording (the items are in recording order)
  std::vector<int> w0((size_t)num_files + 1, (int)mp.works.size());
  for (int i = (int)mp.works.size() - 1; i >= 0; --i) w0[mp.work_seg[i]] = i;
  for (int f = num_files - 1; f >= 0; --f) if (w0[f] > w0[f + 1]) w0[f] = w0[f + 1];
  const size_t slab = (size_t)job.e_pad * job.ca_pad * job.cb_pad;
  // the recordings' finalize launches as ONE (34 launches of ~8 us each were a quarter of the call at C5)
  std::vector<FinalizeParams> all_fp((size_t)num_files);
  std::vector<int> first_block((size_t)num_files + 1, 0);
  for (int f = 0; f < num_files; ++f) {
    td_stats* s = each[f];
    FinalizeBuilder fin;      // (no reduction here reads virtual-image slabs: add_reduce's rule is the plain one)
    LagReduceJob jf = job;
    jf.partial = (job.is_f64 ? reinterpret_cast<const char*>(job.partial) + sizeof(double) * slab * w0[f]
                             : reinterpret_cast<const char*>(job.partial) + sizeof(float) * slab * w0[f]);
    jf.n_work = w0[f + 1] - w0[f];
    jf.g = s->g + s->off_fxx; jf.accumulate = 0;
    fin.add_reduce(jf);
    const int t0 = tp.seg_work0[f], t1 = tp.seg_work0[f + 1];
    for (int i = 0; i < s->d; ++i) {
      LagReduceJob jt = to.jobs[i];
      const size_t tslab = (size_t)jt.e_pad * jt.ca_pad * jt.cb_pad;
      jt.partial = reinterpret_cast<const char*>(jt.partial) + (jt.is_f64 ? sizeof(double) : sizeof(float)) * tslab * t0;
      jt.n_work = t1 - t0;
      jt.g = s->g + s->off_gxo + (jt.g - (s0->g + s0->off_gxo));     // the same row of THIS recording's [l][d + 1][c]
      jt.accumulate = 0;
      fin.add_reduce(jt);
    }
    fin.files(reinterpret_cast<const WinJob*>(jobs_dev) + f, x_dev, ldx, s->c1, 1, s->hw);
    fin.add_targets(s, to, t0, t1, false);
    fin.add_windows(s->win1, 0);
    fin.set_count(s, (double)frames[f]);
    if (zero_next && f == num_files - 1) fin.fp.zero_tab = h->chan_max + kChanTab * (h->chan_phase & 1);
    all_fp[f] = fin.fp;
    first_block[f + 1] = first_block[f] + fin.blocks;
    s->n_files = 1; s->frames = frames[f]; s->fresh_main = false; s->fresh_tgt = false;
    s->tab_ready = false;
    if (!whole[f]) s->whole_files = false;
  }
  {
    static_assert(sizeof(FinalizeParams) % sizeof(int) == 0, "FinalizeParams is copied word by word");
    void* blk = base + kern_bytes;
    TD_TRY(td_upload_async(h, all_fp.data(), sizeof(FinalizeParams) * (size_t)num_files, blk));
    TD_TRY(td_upload_async(h, first_block.data(), sizeof(int) * ((size_t)num_files + 1), reinterpret_cast<char*>(blk) + pb));
    hipLaunchKernelGGL(stats_finalize_multi_kernel, dim3((unsigned)first_block[num_files]), dim3(kFinThreads), 0, h->stream,
                       reinterpret_cast<const FinalizeParams*>(blk),
                       reinterpret_cast<const int*>(reinterpret_cast<char*>(blk) + pb), num_files);
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

// ---- the routes of statistics that are not fusable (or of a call without rows) -----------------------
// One td_stats_accumulate_ranges call after validation.
struct AccCall {
  td_handle* h;
  td_stats* s;
  const float *x, *x2, *y;
  int64_t ldx, ldx2, ldy;
  int num_files;
  int64_t first_slot;            // window slot of the first file of the call
  bool do_main, do_targets;
  FileRows rows;
};

// CCA without context: the Gram kernel + ONE finalize launch (its float64 reduction, the
// boundary windows of both views, the frame count) -- 2 launches for what was reset +
// 2 window gathers + Gram + reduction + an upload of the count.
int accumulate_gram(const AccCall& a, bool gram_fresh) {
  td_handle* h = a.h;
  td_stats* s = a.s;
  TD_TRY(ensure_window_capacity(h, s, s->n_files + a.num_files));
  FinalizeBuilder fin;
  bool handled = false;
  TD_TRY(td_gram(h, a.x, a.ldx, s->c1, a.x2, a.ldx2, s->c2, a.rows.sxy, s->g + s->off_fxx,
                 s->g + s->off_fyy, s->g + s->off_gxy, s->g + s->off_gxo, s->g + s->off_gyo,
                 &handled, !gram_fresh, nullptr, 0.0, &fin.fp.gram));
  TD_REQUIRE(h, handled, "td_gram refused a shape the one-pass test accepted");
  const size_t bytes = sizeof(WinJob) * a.num_files;
  const void* d1 = nullptr;
  const void* d2 = nullptr;
  TD_TRY(td_table_upload(h, a.rows.j1.data(), bytes, &d1));
  TD_TRY(td_table_upload(h, a.rows.j2.data(), bytes, &d2));
  // block ranges: [windows of x | windows of x2 | Gram reduction]; no reductions / bias jobs
  fin.files(reinterpret_cast<const WinJob*>(d1), a.x, a.ldx, s->c1, a.num_files, s->hw);
  fin.add_windows(s->win1, a.first_slot);
  fin.add_second_view(reinterpret_cast<const WinJob*>(d2), a.x2, a.ldx2, s->c2, s->win2);
  s->n_files += a.num_files;
  s->frames += a.rows.new_frames;
  fin.set_count(s, (double)s->frames);
  s->fresh_main = s->fresh_tgt = false;
  return launch_finalize(h, fin.fp, fin.blocks);
}

// segs of a product A^T shift_e(B), e <= e_max, as segments of the product with the operands swapped --
// sum_s b[s] a~[s - e] -- with the wide operand (the old A) restricted to the rows that are summed.  For
// ranges that start at a recording's first row.
std::vector<LagSeg> swapped_segments(const std::vector<LagSeg>& segs, int e_max) {
  std::vector<LagSeg> sw(segs.size());
  for (size_t f = 0; f < segs.size(); ++f) {
    const LagSeg& sg = segs[f];
    LagSeg& o = sw[f];
    o.a_row0 = sg.b_row0; o.a_valid = sg.b_valid;
    o.b_row0 = sg.a_row0;
    o.b_valid = sg.a_valid < sg.u_end ? sg.a_valid : sg.u_end;      // only the rows that are summed
    if (o.b_valid < 0) o.b_valid = 0;
    o.u_begin = 0;
    o.u_end = sg.u_end + e_max < sg.b_valid ? sg.u_end + e_max : sg.b_valid;
    if (o.u_end < 0 || sg.u_end <= 0) o.u_end = 0;
  }
  return sw;
}

// dst [e_count][ca_dst][cb] += what `run` accumulates into a zeroed temporary [e_count][cb][ca] (a product
// with the operands swapped), with the lag order reversed and every block transposed.
template <class Run>
int add_swapped_product(td_handle* h, int e_count, int ca, int cb, double* dst, int ca_dst, Run run) {
  void* tmp = nullptr;
  const size_t tmp_bytes = sizeof(double) * (size_t)e_count * ca * cb;
  TD_TRY(td_alloc_async(h, tmp_bytes, &tmp));
  TD_HIP(h, hipMemsetAsync(tmp, 0, tmp_bytes, h->stream));
  int rc = run(reinterpret_cast<double*>(tmp));
  if (rc == TD_OK) rc = td_add_reversed_transposed(h, reinterpret_cast<const double*>(tmp), e_count, ca, cb, dst, ca_dst);
  td_free_async(h, tmp, true);
  return rc;
}

// Cross-covariance [e][c1][c2].  A narrow second view (an envelope: c2 <= 8) against a wide
// first one would run as padded 64 x 64 tiles of the matrix kernel (the codelab's 69 x 1
// channels, 67 lags: 1.1 ms of a 2.7 ms accumulate for 69 numbers per lag): with the
// operands swapped -- sum_s x2[s] x~[s - e] -- the narrow view is the skinny operand of the
// LDS-tiled kernel, the wide one is restricted to the rows that are summed, and the result
// is added back transposed with the lags reversed.  (Ranges that do not start at a
// recording's first row keep the direct form.)
int cross_covariance(const AccCall& a, bool column) {
  td_handle* h = a.h;
  td_stats* s = a.s;
  const int e_min_xy = -(s->post1 + s->pre2), e_cnt_xy = s->l1 + s->l2 - 1;
  bool swap = s->c2 <= 8 && s->c1 > 8;
  for (const LagSeg& sg : a.rows.sxy) if (sg.u_begin != 0) swap = false;
  if (!swap)
    return td_lagcov(h, a.x, a.ldx, s->c1, false, a.x2, a.ldx2, s->c2, a.rows.sxy, e_min_xy, e_cnt_xy,
                     s->g + s->off_gxy, true);
  const int e_max_xy = e_min_xy + e_cnt_xy - 1;
  const std::vector<LagSeg> sw = swapped_segments(a.rows.sxy, e_max_xy);
  return add_swapped_product(h, e_cnt_xy, s->c1, s->c2, s->g + s->off_gxy, 0, [&](double* tmp) {
    return column ? td_lagcov_column(h, a.x2, a.ldx2, a.x, a.ldx, s->c1, sw, -e_max_xy, e_cnt_xy, tmp)
                  : td_lagcov(h, a.x2, a.ldx2, s->c2, false, a.x, a.ldx, s->c1, sw, -e_max_xy, e_cnt_xy, tmp, true,
                              0, 0, true);
  });
}

// MAIN of the general ladder: the boundary windows of the new files, F'xx (and the auto / cross moments of a
// second view), the counters.
int accumulate_main(const AccCall& a, bool one_pass, bool gram_fresh) {
  td_handle* h = a.h;
  td_stats* s = a.s;
  const int64_t new_frames = a.rows.new_frames;
  // Boundary windows of the new files (also feed the all-ones rows of accumulate_targets).
  TD_TRY(ensure_window_capacity(h, s, s->n_files + a.num_files));
  {
    const size_t bytes = sizeof(WinJob) * a.num_files;
    const void* d1 = nullptr;
    const void* d2 = nullptr;
    TD_TRY(td_table_upload(h, a.rows.j1.data(), bytes, &d1));
    hipLaunchKernelGGL(gather_windows_kernel, dim3((unsigned)a.num_files, 2), dim3(256), 0,
                       h->stream, a.x, (long long)a.ldx, s->c1, s->hw,
                       reinterpret_cast<const WinJob*>(d1), s->win1, (long long)a.first_slot);
    if (s->c2) {
      TD_TRY(td_table_upload(h, a.rows.j2.data(), bytes, &d2));
      hipLaunchKernelGGL(gather_windows_kernel, dim3((unsigned)a.num_files, 2), dim3(256), 0,
                         h->stream, a.x2, (long long)a.ldx2, s->c2, s->hw,
                         reinterpret_cast<const WinJob*>(d2), s->win2, (long long)a.first_slot);
    }
    TD_HIP(h, hipGetLastError());
  }
  // F'xx: lagged auto-covariance of x (the MFMA kernel), and the CCA auto / cross moments.
  if (one_pass) {
    bool handled = false;
    TD_TRY(td_gram(h, a.x, a.ldx, s->c1, a.x2, a.ldx2, s->c2, a.rows.sxy, s->g + s->off_fxx,
                   s->g + s->off_fyy, s->g + s->off_gxy, s->g + s->off_gxo, s->g + s->off_gyo,
                   &handled, !gram_fresh, s->g + s->off_n, (double)(s->frames + new_frames)));
    TD_REQUIRE(h, handled, "td_gram refused a shape the one-pass test accepted");
    if (gram_fresh) s->fresh_main = s->fresh_tgt = false;
  } else {
    TD_TRY(lagcov_auto(h, a.x, a.ldx, s->c1, a.rows.sxx, s->l1, s->g + s->off_fxx));
  }
  if (s->c2 && !one_pass) {
    // (a one-column view -- an envelope -- is a "target column" against itself / against x: the
    // matrix-core targets kernel in windows of 32 lags, td_lagcov_column, instead of a padded
    // 64-channel tile for its auto-covariance (0.14 ms at the codelab's shape) and the skinny
    // VALU kernel for the cross-covariance (0.28 ms))
    const bool column = s->c2 == 1;
    if (column)
      TD_TRY(td_lagcov_column(h, a.x2, a.ldx2, a.x2, a.ldx2, 1, a.rows.syy, 0, s->l2, s->g + s->off_fyy));
    else
      TD_TRY(td_lagcov(h, a.x2, a.ldx2, s->c2, false, a.x2, a.ldx2, s->c2, a.rows.syy, 0, s->l2,
                       s->g + s->off_fyy, true, 0, 0, false, true));
    TD_TRY(cross_covariance(a, column));
  }
  s->n_files += a.num_files;
  s->frames += new_frames;
  // keep n on the device too (it travels in the all-reduce); the one-pass Gram reduction
  // has written it already
  const double nd = (double)s->frames;
  if (!one_pass || new_frames == 0) TD_TRY(td_upload_async(h, &nd, sizeof(double), s->g + s->off_n));
  return TD_OK;
}

// Where the ones rows of a TARGETS call come from: per-file column sums of a view over the rows summed
// (left by a targets call that handled the shape) and the room for the files' contributions.  They live in
// the solver workspace arena (td_scratch is used by the kernels' own tables and partial slabs).
struct OnesWork {
  double* colsum_seg;
  double* contrib;
};

// The all-ones row of gxo (second = false) or gyo (the second view) after a targets call that handled the shape.
int ones_rows_after_targets(const AccCall& a, const OnesWork& w, bool second) {
  const td_stats* s = a.s;
  if (second)
    launch_ones_rows(a.h, s->g + s->off_gyo, 1, 0, s->c2, s->l2, -s->pre2, w.colsum_seg, s->win2, s->hw,
                     (long long)a.first_slot, a.num_files, w.contrib);
  else
    launch_ones_rows(a.h, s->g + s->off_gxo, s->d + 1, s->d, s->c1, s->l1, -s->pre1, w.colsum_seg, s->win1, s->hw,
                     (long long)a.first_slot, a.num_files, w.contrib);
  TD_HIP(a.h, hipGetLastError());
  return TD_OK;
}

// More than four target columns (the fused path and one td_lagcov_targets call take up to four):
//  * a narrow x (<= 8 channels: a forward model, the targets are the EEG channels) -- the
//    product with the operands swapped, sum_v x[v] y[v - e]: x is the skinny operand of the
//    LDS-tiled VALU kernel, y restricted to the rows that are summed is the wide one, and the
//    result is added back transposed with the lags reversed (as the cross-covariance of a
//    lagged CCA above);
//  * otherwise, up to 32 lags and 16 columns: the matrix-core targets kernel, four columns a call.
// Both take the all-ones row from the column sums of x and sum y on its own.  (Before: the
// general float32 matrix kernel on [y | 1] padded to 128 rows -- 3.4 ms per 1e6 samples for
// 8 features x 32 lags against 64 targets, 1.3 ms for 64 channels against 8 targets -- and a
// column sum that read the targets once per column.)  *done = false: neither form, nothing was queued.
int targets_many_columns(const AccCall& a, const OnesWork& w, bool* done) {
  td_handle* h = a.h;
  td_stats* s = a.s;
  const std::vector<LagSeg>& syx = a.rows.syx;
  *done = false;
  bool from_start = true;
  for (const LagSeg& sg : syx) if (sg.u_begin != 0) from_start = false;
  const int e_min = -s->pre1, e_max = s->post1;
  bool handled = false;
  if (s->c1 <= 8 && from_start) {
    const std::vector<LagSeg> sw = swapped_segments(syx, e_max);          // a = y, b = x
    // tmp [e'][c1][d] -> gxo [e][d + 1][c1] rows < d (e' runs backwards)
    TD_TRY(add_swapped_product(h, s->l1, s->d, s->c1, s->g + s->off_gxo, s->d + 1, [&](double* tmp) {
      return td_lagcov(h, a.x, a.ldx, s->c1, false, a.y, a.ldy, s->d, sw, -e_max, s->l1, tmp, true, 0, 0, true);
    }));
    // the all-ones row from the column sums of x (the d = 0 form of the targets path), sum y
    TD_TRY(td_lagcov_targets(h, nullptr, 0, 0, a.x, a.ldx, s->c1, syx, e_min, s->l1,
                             s->g + s->off_gxo, nullptr, w.colsum_seg, &handled, s->d + 1));
    if (handled) {
      TD_TRY(ones_rows_after_targets(a, w, false));
    } else {
      // (column sums alone with more than 31 past lags: the all-ones column on the skinny kernel)
      TD_TRY(td_lagcov(h, nullptr, 0, 0, true, a.x, a.ldx, s->c1, syx, e_min, s->l1,
                       s->g + s->off_gxo + (size_t)s->d * s->c1, true, s->c1, s->d + 1));
    }
    TD_TRY(td_colsum(h, a.y, a.ldy, s->d, syx, s->g + s->off_sy, true));
    *done = true;
  } else if (s->d <= 16 && s->l1 <= 32 && e_min <= 0 && e_max >= 0) {
    for (int c0 = 0; c0 < s->d; c0 += 4) {
      const int dc = s->d - c0 < 4 ? s->d - c0 : 4;
      TD_TRY(td_lagcov_targets(h, a.y + c0, a.ldy, dc, a.x, a.ldx, s->c1, syx, e_min, s->l1,
                               s->g + s->off_gxo + (size_t)c0 * s->c1, s->g + s->off_sy + c0, w.colsum_seg,
                               &handled, s->d + 1));
      TD_REQUIRE(h, handled, "accumulate: the targets kernel refused a column slice");
    }
    TD_TRY(ones_rows_after_targets(a, w, false));
    *done = true;
  }
  return TD_OK;
}

// 33+ lags (the codelab's 37) of up to four columns: the window of 32 lags around lag 0 on the matrix-core
// targets kernel (with the column sums the bias row needs), the lags outside it column by column in
// windows of 32 (td_lagcov_column).  (Before: the LDS-tiled VALU kernel on [y | 1], 0.6 ms of
// the codelab shape's 2.7.)
int targets_many_lags(const AccCall& a, const OnesWork& w, bool* handled) {
  td_handle* h = a.h;
  td_stats* s = a.s;
  const std::vector<LagSeg>& syx = a.rows.syx;
  const int e_min = -s->pre1;
  const int e_lo = e_min < -31 ? -31 : e_min;
  const int here = e_min + s->l1 - e_lo < 256 ? e_min + s->l1 - e_lo : 256;   // windows of one launch
  const size_t lag_stride = (size_t)(s->d + 1) * s->c1;
  TD_TRY(td_lagcov_targets(h, a.y, a.ldy, s->d, a.x, a.ldx, s->c1, syx, e_lo, here,
                           s->g + s->off_gxo + (size_t)(e_lo - e_min) * lag_stride, s->g + s->off_sy,
                           w.colsum_seg, handled));
  TD_REQUIRE(h, *handled, "accumulate: the targets kernel refused the windows from lag 0 on");
  const int before = e_lo - e_min, after = e_min + s->l1 - (e_lo + here);
  for (int i = 0; i < s->d; ++i) {
    if (before > 0)
      TD_TRY(td_lagcov_column(h, a.y + i, a.ldy, a.x, a.ldx, s->c1, syx, e_min, before,
                              s->g + s->off_gxo + (size_t)i * s->c1, s->d + 1));
    if (after > 0)
      TD_TRY(td_lagcov_column(h, a.y + i, a.ldy, a.x, a.ldx, s->c1, syx, e_lo + here, after,
                              s->g + s->off_gxo + (size_t)(before + here) * lag_stride + (size_t)i * s->c1,
                              s->d + 1));
  }
  return TD_OK;
}

// TARGETS of the general ladder: [y | 1]^T x~ for every signed lag (Xty and the lagged column sums), and the
// ones rows of a second view.
int accumulate_targets(const AccCall& a) {
  td_handle* h = a.h;
  td_stats* s = a.s;
  const std::vector<LagSeg>& syx = a.rows.syx;
  void* ws = nullptr;
  const int cmax = s->c1 > s->c2 ? s->c1 : s->c2;
  const int lmax = s->l1 > s->l2 ? s->l1 : s->l2;
  TD_TRY(td_workspace(h, sizeof(double) * (size_t)a.num_files * cmax * (1 + lmax), &ws));
  OnesWork w;
  w.colsum_seg = reinterpret_cast<double*>(ws);
  w.contrib = w.colsum_seg + (size_t)a.num_files * cmax;
  bool handled = false, wide_done = false;
  if (s->d > 4) TD_TRY(targets_many_columns(a, w, &wide_done));
  if (!wide_done) {
    if (s->d >= 1 && s->d <= 4 && s->l1 > 32)
      TD_TRY(targets_many_lags(a, w, &handled));
    else
      TD_TRY(td_lagcov_targets(h, a.y, a.ldy, s->d, a.x, a.ldx, s->c1, syx, -s->pre1, s->l1,
                               s->g + s->off_gxo, s->d ? s->g + s->off_sy : nullptr, w.colsum_seg,
                               &handled));
    if (handled) {
      TD_TRY(ones_rows_after_targets(a, w, false));
    } else {
      TD_TRY(td_lagcov(h, a.y, a.ldy, s->d, true, a.x, a.ldx, s->c1, syx, -s->pre1, s->l1,
                       s->g + s->off_gxo, true));
      if (s->d) TD_TRY(td_colsum(h, a.y, a.ldy, s->d, syx, s->g + s->off_sy, true));
    }
  }
  if (s->c2) {
    TD_TRY(td_lagcov_targets(h, nullptr, 0, 0, a.x2, a.ldx2, s->c2, a.rows.syy, -s->pre2, s->l2,
                             s->g + s->off_gyo, nullptr, w.colsum_seg, &handled));
    if (handled) {
      TD_TRY(ones_rows_after_targets(a, w, true));
    } else {
      TD_TRY(td_lagcov(h, nullptr, 0, 0, true, a.x2, a.ldx2, s->c2, a.rows.syy, -s->pre2, s->l2,
                       s->g + s->off_gyo, true));
    }
  }
  return TD_OK;
}
}  // namespace

int td_stats_settle(td_handle* h, td_stats* s) {
  if (!s || !s->pending) return TD_OK;
  if (!h) return td_fail(h, TD_ERR_INVALID, "td_stats_complete: NULL handle");
  FinalizeParams fp;
  memcpy(&fp, s->pend_params.data(), sizeof(fp));
  TD_TRY(launch_finalize(h, fp, s->pend_blocks));
  s->pending = false;
  return TD_OK;
}

extern "C" {

int td_stats_complete(td_handle* h, td_stats* s) {
  if (!h || !s) return td_fail(h, TD_ERR_INVALID, "td_stats_complete: NULL argument");
  return td_stats_settle(h, s);
}

int td_stats_accumulate_each(td_handle* h, td_stats* const* each, const float* x_dev, int64_t ldx,
                             const float* y_dev, int64_t ldy, const int64_t* file_offsets_host, int num_files,
                             int input_offset, const int64_t* rows_used_host, int* handled) {
  if (!h || !each || !handled) return td_fail(h, TD_ERR_INVALID, "td_stats_accumulate_each: NULL argument");
  *handled = 0;
  TD_REQUIRE(h, x_dev && y_dev && file_offsets_host && num_files > 0, "td_stats_accumulate_each: NULL input");
  for (int f = 0; f < num_files; ++f) {
    TD_REQUIRE(h, each[f], "td_stats_accumulate_each: NULL statistics");
    TD_TRY(td_stats_settle(h, each[f]));
  }
  TD_REQUIRE(h, ldx >= each[0]->c1 && ldy >= each[0]->d, "td_stats_accumulate_each: row pitch below the column count");
  FileRows rows;
  TD_TRY(file_rows(h, file_offsets_host, num_files, input_offset, rows_used_host, nullptr, nullptr, nullptr, nullptr,
                   &rows));
  return accumulate_each(h, each, x_dev, ldx, y_dev, ldy, rows.sxx, rows.syx, rows.j1, num_files, rows.frames,
                         rows.whole, handled);
}

int td_stats_accumulate_ranges(td_handle* h, td_stats* s, const float* x_dev, int64_t ldx,
                               const float* x2_dev, int64_t ldx2, const float* y_dev, int64_t ldy,
                               const int64_t* file_offsets_host, int num_files, int input_offset,
                               const int64_t* rows_used_host, const int64_t* range_begin_host,
                               const int64_t* range_end_host, const int* edge_flags_host,
                               int parts) {
  if (!h || !s) return td_fail(h, TD_ERR_INVALID, "td_stats_accumulate: NULL argument");
  TD_REQUIRE(h, (range_begin_host == nullptr) == (range_end_host == nullptr),
             "td_stats_accumulate_ranges: give both range arrays or neither");
  TD_REQUIRE(h, !range_begin_host || input_offset == 0,
             "td_stats_accumulate_ranges: time ranges need input_offset = 0");
  const bool defer = (parts & TD_ACC_DEFER) != 0;
  parts &= ~TD_ACC_DEFER;
  TD_REQUIRE(h, (parts >= 1 && parts <= 3) || parts == (TD_ACC_TARGETS | TD_ACC_TARGETS_FIRST),
             "td_stats_accumulate_parts: parts must be 1, 2, 3 or TD_ACC_TARGETS | TD_ACC_TARGETS_FIRST");
  TD_REQUIRE(h, !defer || parts == 3 || parts == TD_ACC_MAIN,
             "td_stats_accumulate_parts: TD_ACC_DEFER goes with TD_ACC_MAIN (| TD_ACC_TARGETS)");
  TD_TRY(td_stats_settle(h, s));          // (a finalize still pending from the call before)
  AccCall a;
  a.h = h; a.s = s;
  a.x = x_dev; a.ldx = ldx; a.x2 = x2_dev; a.ldx2 = ldx2; a.y = y_dev; a.ldy = ldy;
  a.num_files = num_files;
  a.do_main = (parts & TD_ACC_MAIN) != 0; a.do_targets = (parts & TD_ACC_TARGETS) != 0;
  const bool tgt_first = (parts & TD_ACC_TARGETS_FIRST) != 0;
  TD_REQUIRE(h, !tgt_first || stats_fusable(s),
             "td_stats_accumulate_parts: TARGETS_FIRST is for regression statistics (targets, no second input)");
  TD_REQUIRE(h, x_dev && file_offsets_host && num_files >= 0, "td_stats_accumulate: NULL input");
  TD_REQUIRE(h, ldx >= s->c1, "ldx (%lld) < channels (%d)", (long long)ldx, s->c1);
  TD_REQUIRE(h, !s->c2 || (x2_dev && ldx2 >= s->c2), "input_2 missing or ldx2 too small");
  TD_REQUIRE(h, !s->d || (y_dev && ldy >= s->d), "y missing or ldy too small");
  if (num_files == 0) return TD_OK;

  TD_TRY(file_rows(h, file_offsets_host, num_files, input_offset, rows_used_host, range_begin_host, range_end_host,
                   edge_flags_host, a.do_main ? &s->whole_files : nullptr, &a.rows));
  const int64_t new_frames = a.rows.new_frames;
  // window slot of the first new file: MAIN appends the files, a TARGETS-only call comes
  // after the MAIN call of the same files
  a.first_slot = (a.do_main || tgt_first) ? s->n_files : s->n_files - num_files;
  TD_REQUIRE(h, a.first_slot >= 0, "td_stats_accumulate_parts: TARGETS before MAIN (say TD_ACC_TARGETS_FIRST)");

  if (stats_fusable(s) && new_frames > 0)
    return accumulate_fused(h, s, x_dev, ldx, y_dev, ldy, a.rows.sxx, a.rows.syx, a.rows.j1, num_files, new_frames,
                            a.first_slot, a.do_main, a.do_targets, tgt_first, defer);
  TD_REQUIRE(h, !tgt_first, "td_stats_accumulate_parts: TARGETS_FIRST needs the fused accumulate path");
  // CCA without context on either input: every moment is one Gram matrix of [x | x2 | 1]
  // (td_gram), done by MAIN; TARGETS then has nothing left to add.
  const bool one_pass = stats_one_pass(s);
  // (the one-pass Gram reduction overwrites fresh statistics itself)
  const bool gram_fresh = one_pass && a.do_main && s->fresh_main && s->fresh_tgt && new_frames > 0;
  if (!gram_fresh) TD_TRY(stats_materialize(h, s));

  if (one_pass && a.do_main && new_frames > 0) return accumulate_gram(a, gram_fresh);
  if (a.do_main) TD_TRY(accumulate_main(a, one_pass, gram_fresh));
  if (a.do_targets && !one_pass) TD_TRY(accumulate_targets(a));
  return TD_OK;
}

}  // extern "C"
