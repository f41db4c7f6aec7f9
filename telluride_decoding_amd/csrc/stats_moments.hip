// The expansion of the compact statistics into the dense moment matrices the reference accumulates
// literally (stats_common.h: the identity; td_stats_moments, td_stats_moments_ld), and the dense moments of
// every fold of a leave-one-out sweep from the total's (td_stats_loso_moments).
#include "stats_common.h"

namespace {

// Expansion in two phases (both fill the chip, neither depends on the number of
// files beyond phase 1's short loop):
//   1. edge_outer_kernel: D[s][e] = the edge correction that lag step s adds,
//      summed over files in fixed order (|files| * 2 rank-1 updates of a 64x64
//      tile per workgroup);
//   2. expand_kernel: one workgroup per (e, 32x32 sub-tile) walks the lag
//      diagonal a = 1..posta and a = -1..-prea with a running sum of D and
//      writes the dense blocks (the mirrored block through an LDS transpose, so
//      both stores are coalesced).
// (v1 walked the diagonal inside 32 workgroups with the file loop inside: 0.5 ms
// at C2 with 10 files, 8.7 ms with 200; v2 recomputed the prefix per lag in
// float64 VALU: 0.23 / 4.2 ms.)
struct ExpandParams {
  const double* g;   // [e_count][ca][cb]
  int e_min, e_count;
  int ca, prea, posta;
  int cb, preb, postb;
  const float* wina;  // [files][2][2hw][ca]
  const float* winb;  // [files][2][2hw][cb]
  int hw;
  long long n_files;
  double* m;          // dense output
  long long ldm;
  int symmetric;      // A == B: only e >= 0 is given; mirror into the lower part
  double* dstep;      // [prea + posta][e_count][ca][cb]
  int n_tj;           // column tiles (64 wide in phase 1, 32 wide in phase 2)
};

// step s < posta:  a = s + 1 adds  -P[s][e] (head)  +P[N'+s][e] (tail)
// step s >= posta: a = -(s - posta + 1) adds  -P[N'+a][e] (tail)
__global__ __launch_bounds__(256) void edge_outer_kernel(ExpandParams p) {
  const int s = blockIdx.x;
  const int e = p.e_min + blockIdx.y;
  const int ti = blockIdx.z / p.n_tj, tj = blockIdx.z % p.n_tj;
  const int i0 = ti * 64 + (threadIdx.x >> 4) * 4;
  const int j0 = tj * 64 + (threadIdx.x & 15) * 4;
  const long long wa = (long long)2 * p.hw * p.ca, wb = (long long)2 * p.hw * p.cb;
  double v[4][4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) v[ii][jj] = 0.0;

  // (the window rows of 32 recordings at a time through LDS, fetched by the whole workgroup at once: as a loop of
  // two dependent global loads per recording and thread this kernel took 47 us for the 31 recordings of a
  // LOSO fold; the terms are added in the same order as before)
  __shared__ float sa[32][64], sb[32][64];
  const int la = (threadIdx.x >> 4) * 4, lb = (threadIdx.x & 15) * 4;
  auto add_outer = [&](int which, int ra, int rb, double sign) {
    if (ra < 0 || ra >= 2 * p.hw || rb < 0 || rb >= 2 * p.hw) return;       // (uniform)
    const float* pa = p.wina + (long long)which * wa + (long long)ra * p.ca;
    const float* pb = p.winb + (long long)which * wb + (long long)rb * p.cb;
    for (long long f0 = 0; f0 < p.n_files; f0 += 32) {
      const int nf = p.n_files - f0 < 32 ? (int)(p.n_files - f0) : 32;
      __syncthreads();
      for (int idx = threadIdx.x; idx < nf * 64; idx += 256) {
        const int f = idx >> 6, c = idx & 63;
        const int ia = ti * 64 + c, ib = tj * 64 + c;
        sa[f][c] = ia < p.ca ? pa[(f0 + f) * 2 * wa + ia] : 0.f;
        sb[f][c] = ib < p.cb ? pb[(f0 + f) * 2 * wb + ib] : 0.f;
      }
      __syncthreads();
      for (int f = 0; f < nf; ++f) {
        double av[4], bv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { av[k] = (double)sa[f][la + k]; bv[k] = (double)sb[f][lb + k]; }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) v[ii][jj] += sign * av[ii] * bv[jj];
      }
    }
  };
  if (s < p.posta) {
    add_outer(0, s + p.hw, s + e + p.hw, -1.0);
    add_outer(1, s + p.hw, s + e + p.hw, +1.0);
  } else {
    const int aa = -(s - p.posta + 1);
    add_outer(1, aa + p.hw, aa + e + p.hw, -1.0);
  }
  double* d = p.dstep + ((long long)s * p.e_count + blockIdx.y) * p.ca * p.cb;
#pragma unroll
  for (int ii = 0; ii < 4; ++ii)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int i = i0 + ii, j = j0 + jj;
      if (i < p.ca && j < p.cb) d[(long long)i * p.cb + j] = v[ii][jj];
    }
}

constexpr int kExpandSeg = 8;
constexpr int kExpandFusedFiles = 2;   // up to this many files: no edge_outer_kernel pass

__global__ __launch_bounds__(256) void expand_kernel(ExpandParams p) {
  __shared__ double tr[32][33];
  const int e = p.e_min + blockIdx.x;
  const int ti = blockIdx.y / p.n_tj, tj = blockIdx.y % p.n_tj;
  const int ri = threadIdx.x >> 3, cj = (threadIdx.x & 7) * 4;   // 32 rows x 8 column quads
  const int i = ti * 32 + ri, j0 = tj * 32 + cj;
  const long long tile = (long long)p.ca * p.cb;
  const double* g = p.g + (long long)(e - p.e_min) * tile;
  const bool row_ok = i < p.ca;

  double base[4], v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    base[q] = (row_ok && j0 + q < p.cb) ? g[(long long)i * p.cb + j0 + q] : 0.0;

  auto emit = [&](int a) {
    const int la = a + p.prea, lb = a + e + p.preb;
    if (lb < 0 || lb >= p.preb + 1 + p.postb) return;   // uniform per workgroup
    const long long r = (long long)la * p.ca + i;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (row_ok && j0 + q < p.cb) p.m[r * p.ldm + (long long)lb * p.cb + j0 + q] = v[q];
    if (p.symmetric && e != 0) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) tr[cj + q][ri] = v[q];
      __syncthreads();
      // thread (ri, cj) now writes mirrored row j = tj*32 + ri, columns i = ti*32 + cj + q
      const int jm = tj * 32 + ri;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int im = ti * 32 + cj + q;
        if (jm < p.cb && im < p.ca)
          p.m[((long long)lb * p.cb + jm) * p.ldm + (long long)la * p.ca + im] = tr[ri][cj + q];
      }
    }
  };
  // D[s][e] of step s for this thread's four elements, formed on the spot when phase 1 was skipped
  // (few files: its 32 MB of step tiles cost more to write and read back than these 2 |files| products
  // per element and step) -- the same terms in the same order as edge_outer_kernel, so the same bits.
  const long long wa = (long long)2 * p.hw * p.ca, wb = (long long)2 * p.hw * p.cb;
  auto outer4 = [&](int which, int ra, int rb, double sign, double (&d)[4]) {
    if (ra < 0 || ra >= 2 * p.hw || rb < 0 || rb >= 2 * p.hw) return;
    const float* pa = p.wina + (long long)which * wa + (long long)ra * p.ca;
    const float* pb = p.winb + (long long)which * wb + (long long)rb * p.cb;
    for (long long f = 0; f < p.n_files; ++f) {
      const double av = row_ok ? (double)pa[f * 2 * wa + i] : 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double bv = j0 + q < p.cb ? (double)pb[f * 2 * wb + j0 + q] : 0.0;
        d[q] += sign * av * bv;
      }
    }
  };
  auto add_step = [&](int s) {
    if (p.dstep) {
      const double* d = p.dstep + ((long long)s * p.e_count + blockIdx.x) * tile;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (row_ok && j0 + q < p.cb) v[q] += d[(long long)i * p.cb + j0 + q];
      return;
    }
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    if (s < p.posta) {
      outer4(0, s + p.hw, s + e + p.hw, -1.0, d);
      outer4(1, s + p.hw, s + e + p.hw, +1.0, d);
    } else {
      const int aa = -(s - p.posta + 1);
      outer4(1, aa + p.hw, aa + e + p.hw, -1.0, d);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] += d[q];
  };

  // The lag diagonal is walked in segments of kExpandSeg steps, one workgroup (blockIdx.z) each:
  // steps 0 .. posta - 1 are a = 1 .. posta, steps posta .. posta + prea - 1 are a = -1 .. -prea;
  // the running sum at a segment's first step is the prefix of D over the steps of its side
  // before it (a few independent loads).  (One workgroup walking all 31 steps of C2, a load, an
  // add and a barrier-fenced transposing store per step, was a 40 us serial chain per launch.)
  const int n_steps = p.posta + p.prea;
  const int s0 = (int)blockIdx.z * kExpandSeg;
  const int s1 = s0 + kExpandSeg < n_steps ? s0 + kExpandSeg : n_steps;
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = base[q];
  if (blockIdx.z == 0) emit(0);
  if (s0 < s1) {
    const int side0 = s0 < p.posta ? 0 : p.posta;      // first step of the side s0 is on
    for (int sp = side0; sp < s0; ++sp) add_step(sp);
    for (int st = s0; st < s1; ++st) {
      if (st == p.posta) {                             // the negative side starts from the base again
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = base[q];
      }
      add_step(st);
      emit(st < p.posta ? st + 1 : -(st - p.posta + 1));
    }
  }
}

// Fills the bias row/column of XtX and the whole XtY from gxo / sy / n.
__global__ void bias_fill_kernel(const double* __restrict__ gxo, const double* __restrict__ sy,
                                 const double* __restrict__ n, int l1, int c1, int d,
                                 double* __restrict__ xtx, long long ld, double* __restrict__ xty) {
  const int k1 = l1 * c1;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < k1) {
    const int l = idx / c1, c = idx % c1;
    const double* row = gxo + (long long)l * (d + 1) * c1;
    if (xtx) {
      const double s = row[(long long)d * c1 + c];   // ones row of A = [y | 1]
      xtx[(long long)idx * ld + k1] = s;
      xtx[(long long)k1 * ld + idx] = s;
    }
    if (xty)
      for (int dd = 0; dd < d; ++dd) xty[(long long)idx * d + dd] = row[(long long)dd * c1 + c];
  } else if (idx == k1) {
    if (xtx) xtx[(long long)k1 * ld + k1] = n[0];
    if (xty)
      for (int dd = 0; dd < d; ++dd) xty[(long long)k1 * d + dd] = sy[dd];
  }
}

// ---- the dense moments of every fold of a leave-one-out sweep in ONE launch (round 6) -----------------
// The moments are linear in the recordings: a fold's training statistics are the total's plus a few signed
// terms (minus the held-out recording; a fold whose minibatch stream drops a remainder: minus the last
// training recording, plus the same recording accumulated without its tail), each term the statistics of one
// or two recordings.  So M_fold = M_total + sum_t sign_t (T(G_t) + E_t): the total's dense matrix -- which the
// sweep solver expands anyway, for its preconditioner -- read once per fold and the terms' Toeplitz blocks and
// edge products formed on the spot, like expand_kernel does for a statistic of one or two recordings.  Replaces,
// per fold, a 31-member combine (16 MB of statistics summed), its window copy, an edge_outer pass over 31
// recordings (32 MB of step tiles) and an expansion: 33 x 5 launches and 2.7 of the 15.5 ms of a C5 sweep.
constexpr int kLosoMaxTerms = 4;
struct LosoTermDev {
  const double* g;      // the term's lagged auto-covariance blocks [l][c][c]
  const float* win;     // its boundary windows [files][2][2 hw][c]
  const double* gxo;    // [l][d + 1][c]
  const double* sy;     // [d]
  const double* n;      // [1]
  long long n_files;
  double sign;
};
struct LosoFoldDev {
  int n_terms, pad;
  LosoTermDev t[kLosoMaxTerms];
};
struct LosoExpandParams {
  const double* mt;     // dense moments of the total, row stride ldm
  const LosoFoldDev* folds;
  int c, pre, post, l, hw, segs;
  double* out;          // [folds][n][ldm]
  long long ldm, fold_stride;
};

__global__ __launch_bounds__(256) void loso_expand_kernel(LosoExpandParams p) {
  __shared__ double tr[32][33];
  // (the fold is the fastest index: the workgroups that run together read the same tile of the total's matrix)
  const int fold = blockIdx.x;
  const int n_tj = (p.c + 31) / 32;
  const int ti = blockIdx.y / n_tj, tj = blockIdx.y % n_tj;
  const int seg = blockIdx.z % p.segs, e = blockIdx.z / p.segs;
  const LosoFoldDev& fd = p.folds[fold];
  double* out = p.out + (long long)fold * p.fold_stride;
  const int ri = threadIdx.x >> 3, cj = (threadIdx.x & 7) * 4;   // 32 rows x 8 column quads
  const int i = ti * 32 + ri, j0 = tj * 32 + cj;
  const long long tile = (long long)p.c * p.c;
  const bool row_ok = i < p.c;
  const long long wsz = (long long)2 * p.hw * p.c;

  double base[4] = {0.0, 0.0, 0.0, 0.0}, v[4];
  for (int t = 0; t < fd.n_terms; ++t) {
    const double* g = fd.t[t].g + (long long)e * tile;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (row_ok && j0 + q < p.c) base[q] += fd.t[t].sign * g[(long long)i * p.c + j0 + q];
  }
  auto emit = [&](int a) {
    const int la = a + p.pre, lb = a + e + p.pre;
    if (lb < 0 || lb >= p.l) return;                    // uniform per workgroup
    const long long r = (long long)la * p.c + i;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (row_ok && j0 + q < p.c) {
        const long long at = r * p.ldm + (long long)lb * p.c + j0 + q;
        out[at] = p.mt[at] + v[q];
      }
    if (e != 0) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) tr[cj + q][ri] = v[q];
      __syncthreads();
      const int jm = tj * 32 + ri;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int im = ti * 32 + cj + q;
        if (jm < p.c && im < p.c) {
          const long long at = ((long long)lb * p.c + jm) * p.ldm + (long long)la * p.c + im;
          out[at] = p.mt[at] + tr[ri][cj + q];
        }
      }
    }
  };
  auto outer4 = [&](const LosoTermDev& tm, int which, int ra, int rb, double sign, double (&d)[4]) {
    if (ra < 0 || ra >= 2 * p.hw || rb < 0 || rb >= 2 * p.hw) return;
    const float* pa = tm.win + (long long)which * wsz + (long long)ra * p.c;
    const float* pb = tm.win + (long long)which * wsz + (long long)rb * p.c;
    for (long long f = 0; f < tm.n_files; ++f) {
      const double av = row_ok ? (double)pa[f * 2 * wsz + i] : 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double bv = j0 + q < p.c ? (double)pb[f * 2 * wsz + j0 + q] : 0.0;
        d[q] += sign * av * bv;
      }
    }
  };
  auto add_step = [&](int s) {
    for (int t = 0; t < fd.n_terms; ++t) {
      double d[4] = {0.0, 0.0, 0.0, 0.0};
      if (s < p.post) {
        outer4(fd.t[t], 0, s + p.hw, s + e + p.hw, -1.0, d);
        outer4(fd.t[t], 1, s + p.hw, s + e + p.hw, +1.0, d);
      } else {
        const int aa = -(s - p.post + 1);
        outer4(fd.t[t], 1, aa + p.hw, aa + e + p.hw, -1.0, d);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] += fd.t[t].sign * d[q];
    }
  };
  const int n_steps = p.post + p.pre;
  const int s0 = p.segs == 1 ? 0 : seg * kExpandSeg;
  const int s1 = p.segs == 1 ? n_steps : (s0 + kExpandSeg < n_steps ? s0 + kExpandSeg : n_steps);
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = base[q];
  if (seg == 0) emit(0);
  if (s0 < s1) {
    const int side0 = s0 < p.post ? 0 : p.post;
    for (int sp = side0; sp < s0; ++sp) add_step(sp);
    for (int st = s0; st < s1; ++st) {
      if (st == p.post) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = base[q];
      }
      add_step(st);
      emit(st < p.post ? st + 1 : -(st - p.post + 1));
    }
  }
}

// the bias row / column of every fold's XtX and its whole XtY: the total's plus the signed terms'
struct LosoBiasParams {
  const double* gxo; const double* sy; const double* n;      // the total's
  const LosoFoldDev* folds;
  int l, c, d;
  double* out; long long ldm, fold_stride;
  double* xty; long long xty_stride;
};
__global__ void loso_bias_kernel(LosoBiasParams p) {
  const int k1 = p.l * p.c;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int fold = blockIdx.y;
  if (idx > k1) return;
  const LosoFoldDev& fd = p.folds[fold];
  double* xtx = p.out + (long long)fold * p.fold_stride;
  double* xty = p.xty + (long long)fold * p.xty_stride;
  auto value = [&](const double* gxo, const double* sy, const double* n, int dd) -> double {
    // dd < d: column dd of XtY; dd == d: the bias entry of XtX
    if (idx < k1) {
      const int l = idx / p.c, c = idx % p.c;
      return gxo[((long long)l * (p.d + 1) + dd) * p.c + c];
    }
    return dd < p.d ? sy[dd] : n[0];
  };
  for (int dd = 0; dd <= p.d; ++dd) {
    double s = value(p.gxo, p.sy, p.n, dd);
    for (int t = 0; t < fd.n_terms; ++t) s += fd.t[t].sign * value(fd.t[t].gxo, fd.t[t].sy, fd.t[t].n, dd);
    if (dd < p.d) {
      xty[(long long)idx * p.d + dd] = s;
    } else {
      xtx[(long long)idx * p.ldm + k1] = s;
      xtx[(long long)k1 * p.ldm + idx] = s;
    }
  }
}

int expand_block(td_handle* h, const double* g, int e_min, int e_count, int ca, int prea,
                 int posta, int cb, int preb, int postb, const float* wina, const float* winb,
                 int hw, int64_t n_files, double* m, int64_t ldm, bool symmetric) {
  ExpandParams p;
  p.g = g; p.e_min = e_min; p.e_count = e_count;
  p.ca = ca; p.prea = prea; p.posta = posta;
  p.cb = cb; p.preb = preb; p.postb = postb;
  p.wina = wina; p.winb = winb; p.hw = hw; p.n_files = n_files;
  p.m = m; p.ldm = ldm; p.symmetric = symmetric ? 1 : 0;
  const int n_steps = prea + posta;
  p.dstep = nullptr;
  // (one or two files -- the per-recording statistics of a leave-one-out sweep, a single-recording fit:
  // the expansion forms its edge terms itself, see expand_kernel)
  if (n_steps > 0 && n_files > kExpandFusedFiles) {
    void* scratch = nullptr;
    TD_TRY(td_scratch(h, sizeof(double) * (size_t)n_steps * e_count * ca * cb, &scratch));
    p.dstep = reinterpret_cast<double*>(scratch);
    p.n_tj = (int)td_ceil_div(cb, 64);
    dim3 grid1((unsigned)n_steps, (unsigned)e_count, (unsigned)(td_ceil_div(ca, 64) * p.n_tj));
    hipLaunchKernelGGL(edge_outer_kernel, grid1, dim3(256), 0, h->stream, p);
  }
  p.n_tj = (int)td_ceil_div(cb, 32);
  const int segs = n_steps > 0 ? (int)td_ceil_div(n_steps, kExpandSeg) : 1;
  dim3 grid((unsigned)e_count, (unsigned)(td_ceil_div(ca, 32) * p.n_tj), (unsigned)segs);
  hipLaunchKernelGGL(expand_kernel, grid, dim3(256), 0, h->stream, p);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

}  // namespace

extern "C" {

int td_stats_moments(td_handle* h, td_stats* s, double* xtx_dev, double* xty_dev,
                     double* x2tx2_dev, double* xtx2_dev, double* sum_x2_dev) {
  return td_stats_moments_ld(h, s, xtx_dev, s ? s->k1 + 1 : 0, xty_dev, x2tx2_dev, xtx2_dev, sum_x2_dev);
}

}  // extern "C"

// The same with the rows of XtX `ld_xtx` numbers apart (the solvers ask for their padded stride,
// a multiple of 64: with the dense stride n = 2049 every 256-byte piece of a row straddles cache
// lines and the 34 MB of the C2 matrix took 42 us to write).
int td_stats_moments_ld(td_handle* h, td_stats* s, double* xtx_dev, int64_t ld_xtx, double* xty_dev,
                        double* x2tx2_dev, double* xtx2_dev, double* sum_x2_dev) {
  if (!h || !s) return td_fail(h, TD_ERR_INVALID, "td_stats_moments: NULL argument");
  TD_TRY(stats_materialize(h, s));
  if (xtx_dev)
    TD_TRY(expand_block(h, s->g + s->off_fxx, 0, s->l1, s->c1, s->pre1, s->post1, s->c1, s->pre1,
                        s->post1, s->win1, s->win1, s->hw, s->n_files, xtx_dev, ld_xtx, true));
  if (xtx_dev || xty_dev) {
    hipLaunchKernelGGL(bias_fill_kernel, dim3((unsigned)td_ceil_div(s->k1 + 1, 256)), dim3(256), 0,
                       h->stream, s->g + s->off_gxo, s->g + s->off_sy, s->g + s->off_n, s->l1,
                       s->c1, s->d, xtx_dev, (long long)ld_xtx, s->d ? xty_dev : nullptr);
    TD_HIP(h, hipGetLastError());
  }
  if (s->c2) {
    if (x2tx2_dev)
      TD_TRY(expand_block(h, s->g + s->off_fyy, 0, s->l2, s->c2, s->pre2, s->post2, s->c2, s->pre2,
                          s->post2, s->win2, s->win2, s->hw, s->n_files, x2tx2_dev, s->k2, true));
    if (xtx2_dev)
      TD_TRY(expand_block(h, s->g + s->off_gxy, -(s->post1 + s->pre2), s->l1 + s->l2 - 1, s->c1,
                          s->pre1, s->post1, s->c2, s->pre2, s->post2, s->win1, s->win2, s->hw,
                          s->n_files, xtx2_dev, s->k2, false));
    if (sum_x2_dev)
      TD_HIP(h, hipMemcpyAsync(sum_x2_dev, s->g + s->off_gyo, sizeof(double) * s->k2,
                               hipMemcpyDeviceToDevice, h->stream));
  }
  return TD_OK;
}

// Dense moments of the folds of a leave-one-out sweep (td_ridge_solve_loso_terms): fold f = total +
// sum_{t in [term_begin[f], term_begin[f + 1])} signs[t] terms[t].  mt: the total's dense XtX (row stride ld), already
// expanded; out [n_folds][n][ld] receives the folds' XtX, xty_out [n_folds][n][d] their XtY.  Regression
// statistics without a second view; every fold at most kLosoMaxTerms terms.
int td_stats_loso_moments(td_handle* h, td_stats* total, td_stats* const* terms, const int* term_begin,
                          const double* signs, int n_folds, const double* mt, int64_t ld, double* out,
                          double* xty_out) {
  TD_REQUIRE(h, total && terms && term_begin && signs && mt && out && xty_out, "td_stats_loso_moments: NULL argument");
  TD_REQUIRE(h, total->c2 == 0 && total->d >= 1, "td_stats_loso_moments: regression statistics only");
  TD_TRY(stats_materialize(h, total));
  std::vector<LosoFoldDev> folds((size_t)n_folds);
  for (int f = 0; f < n_folds; ++f) {
    const int nt = term_begin[f + 1] - term_begin[f];
    TD_REQUIRE(h, nt >= 0 && nt <= kLosoMaxTerms, "td_stats_loso_moments: a fold has %d terms (at most %d)", nt,
               kLosoMaxTerms);
    memset(&folds[f], 0, sizeof(LosoFoldDev));
    folds[f].n_terms = nt;
    for (int t = 0; t < nt; ++t) {
      td_stats* s = terms[term_begin[f] + t];
      TD_REQUIRE(h, s, "td_stats_loso_moments: NULL statistics");
      TD_REQUIRE(h, s->c1 == total->c1 && s->l1 == total->l1 && s->pre1 == total->pre1 && s->d == total->d &&
                 s->c2 == 0 && s->hw == total->hw, "td_stats_loso_moments: layouts differ");
      TD_TRY(stats_materialize(h, s));
      LosoTermDev& td = folds[f].t[t];
      td.g = s->g + s->off_fxx; td.win = s->win1; td.gxo = s->g + s->off_gxo; td.sy = s->g + s->off_sy;
      td.n = s->g + s->off_n; td.n_files = s->n_files; td.sign = signs[term_begin[f] + t];
    }
  }
  const void* folds_dev = nullptr;
  TD_TRY(td_table_upload(h, folds.data(), folds.size() * sizeof(LosoFoldDev), &folds_dev));
  const int n = total->k1 + 1;
  LosoExpandParams p;
  p.mt = mt; p.folds = reinterpret_cast<const LosoFoldDev*>(folds_dev);
  p.c = total->c1; p.pre = total->pre1; p.post = total->post1; p.l = total->l1; p.hw = total->hw;
  const int n_steps = total->pre1 + total->post1;
  const int tiles = (int)(td_ceil_div(p.c, 32) * td_ceil_div(p.c, 32));
  // (a workgroup walks its lag diagonal from the start -- a segment that starts later first repeats the steps in
  //  front of it: segments only when the folds alone do not fill the chip)
  p.segs = n_steps > 0 && (long long)n_folds * tiles * p.l < 2048 ? (int)td_ceil_div(n_steps, kExpandSeg) : 1;
  p.out = out; p.ldm = ld; p.fold_stride = (long long)n * ld;
  TD_REQUIRE(h, (long long)p.segs * p.l < 65536, "td_stats_loso_moments: too many lags");
  hipLaunchKernelGGL(loso_expand_kernel, dim3((unsigned)n_folds, (unsigned)tiles, (unsigned)(p.segs * p.l)), dim3(256),
                     0, h->stream, p);
  LosoBiasParams b;
  b.gxo = total->g + total->off_gxo; b.sy = total->g + total->off_sy; b.n = total->g + total->off_n;
  b.folds = p.folds; b.l = total->l1; b.c = total->c1; b.d = total->d;
  b.out = out; b.ldm = ld; b.fold_stride = p.fold_stride; b.xty = xty_out; b.xty_stride = (long long)n * total->d;
  hipLaunchKernelGGL(loso_bias_kernel, dim3((unsigned)td_ceil_div(n, 256), (unsigned)n_folds), dim3(256), 0, h->stream, b);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}
