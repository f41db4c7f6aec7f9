// The online CCA fit (td_ccafit_online_*): the exact float64 moments of BOTH lagged views of a CCA model -- the EEG
// and the attended speaker's feature block -- for rows that arrive in pushes of any length, as the online family does
// everything else: the state on the device, ONE launch per push for a bank of sessions, and any cut of a recording
// gives the bytes of one push.  td_ccafit_online_solve turns the moments into rotations on the device through the
// dense stage td_cca_solve runs (eig.hip: td_cca_dense), plus the fitted stretch's statistics in closed form.
//
// Views.  View 1 is the EEG: c1 channels, context (pre1, post1), k1 = c1 (pre1 + 1 + post1).  View 2 is the feature
// block: c2 columns, context (pre2, post2), k2 = c2 (pre2 + 1 + post2).  The joint vector of frame t is
// u = [x~_t | y~_t | 1], n = k1 + k2 + 1, each half oracle/lag.py's row t of its view: v[l c + ch] =
// x[t + l - pre][ch], zero outside the recording.  Frames run post = max(post1, post2) rows behind the input, as
// td_cca_online_push has it: emitted = max(0, pushed - post); a push that carries flush emits the rest, as if `post`
// zero rows followed in both views.
//
// The sum.  For every newly emitted frame, in frame order, M = M g + u u^T in float64.  The inputs are float32, so a
// product is exact; with g == 1 an element takes ONE rounding per frame (a fused multiply-add of the widened values),
// with g < 1 two, round(round(acc g) + p), written so that nothing fuses them (see step()).  The order is a
// function of the frame index alone, so NumPy's M * g + np.outer(u, u) in frame order is a bit-exact twin.
// M[n - 1][n - 1] is the frame count (g == 1) or the effective count.
//
// The launch.  grid (upper-triangular 64 x 64 tiles of M + one tail workgroup, sessions), 256 threads; a thread owns
// a 4 x 4 block of accumulators, rows ty + 16 p and columns tx + 16 q of its tile, so that the 8-byte LDS reads of a
// half wave are 16 consecutive doubles (or one address): no bank conflict.  A workgroup stages the two 64-wide slices
// of the joint vectors of a pass of kPass frames into LDS as float64, then every thread walks the pass in frame
// order.  The staging is what differs from online_fit.hip: a joint column belongs to view 1, to view 2 or is the ones
// column, and each view has its own (c, pre), tail length pre_v + post, source pointer and leading dimension; a
// thread resolves its column to a Column {source, tail, lag - pre, channel} ONCE per launch, so a slice may straddle
// the view boundary and the ones column may sit alone in the last tile.  Only tiles with tj >= ti are computed and
// stored (a diagonal tile whole); the lower tiles stay zero and td_ccafit_online_moments mirrors.
//
// The state.  M [n^2] float64, then TWO tail copies of {EEG [pre1 + post][c1], features [pre2 + post][c2]} float32:
// slot j of a view's tail holds row pushed - (pre_v + post) + j, zero before row 0, so all zeros = fresh.  A launch
// reads copy (pushes_before & 1) and the tail workgroup writes every slot of the other one.  The host counts the
// pushes with n > 0; a push without rows writes no tail.  No workgroup reads what another writes, no atomics, vector
// stores only.
//
// What this file shares with online_fit.hip -- step(), view_row(), the tiling and a thread's accumulators, the checks
// of a push -- is online_fit_common.h.  Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are in DESIGN.md
// section 39.
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

#include "online_fit_common.h"

namespace {

constexpr int kMaxChannels = TD_ONLINE_CCAFIT_MAX_CHANNELS;
constexpr int kMaxFeatures = TD_ONLINE_CCAFIT_MAX_FEATURES;
constexpr int kMaxLags = TD_ONLINE_CCAFIT_MAX_LAGS;
constexpr int kMaxK = TD_ONLINE_CCAFIT_MAX_K;
constexpr int kMaxDims = TD_ONLINE_CCAFIT_MAX_DIMS;

struct CcaFitShape {
  int c1, pre1, post1, c2, pre2, post2;
  int post, k1, k2, n, tiles;                  // post = max(post1, post2), n = k1 + k2 + 1, tiles = ceil(n / 64)
  int tl1, tl2;                                // tail rows: pre_v + post
  long long off_tail, tail_floats, off_ftail;  // (floats) the first tail copy, one copy's length, the feature tail in a copy
  long long bytes;
};

struct CcaFitParams {
  const float* eeg; long long ld_e, ss_e;
  const float* feat; long long ld_f, ss_f;
  long long n, frames_before, e0;
  long long emitted;
  int work_tiles, live;
  double g;
  char* state; long long state_ss;             // (bytes)
  CcaFitShape s;
};

int ccafit_shape(td_handle* h, const char* who, int c1, int pre1, int post1, int c2, int pre2, int post2,
                 CcaFitShape* s) {
  TD_REQUIRE(h, c1 >= 1 && c1 <= kMaxChannels, "%s: %d channels (1 .. %d)", who, c1, kMaxChannels);
  TD_REQUIRE(h, c2 >= 1 && c2 <= kMaxFeatures, "%s: %d features (1 .. %d)", who, c2, kMaxFeatures);
  TD_REQUIRE(h, pre1 >= 0 && post1 >= 0 && pre1 + 1 + post1 <= kMaxLags,
             "%s: an EEG context of %d + 1 + %d lags (1 .. %d)", who, pre1, post1, kMaxLags);
  TD_REQUIRE(h, pre2 >= 0 && post2 >= 0 && pre2 + 1 + post2 <= kMaxLags,
             "%s: a feature context of %d + 1 + %d lags (1 .. %d)", who, pre2, post2, kMaxLags);
  const int k1 = (pre1 + 1 + post1) * c1, k2 = (pre2 + 1 + post2) * c2;
  TD_REQUIRE(h, k1 + k2 <= kMaxK, "%s: %d + %d = %d lagged inputs in the two views (at most %d)", who, k1, k2,
             k1 + k2, kMaxK);
  s->c1 = c1; s->pre1 = pre1; s->post1 = post1; s->c2 = c2; s->pre2 = pre2; s->post2 = post2;
  s->post = std::max(post1, post2);
  s->k1 = k1; s->k2 = k2; s->n = k1 + k2 + 1;
  s->tiles = tiles_of(s->n);
  s->tl1 = pre1 + s->post; s->tl2 = pre2 + s->post;
  s->off_tail = 2LL * s->n * s->n;
  s->off_ftail = (long long)s->tl1 * c1;
  s->tail_floats = s->off_ftail + (long long)s->tl2 * c2;
  s->bytes = td_round_up(4 * (s->off_tail + 2 * s->tail_floats), 8);
  return TD_OK;
}

// What a thread stages: joint column -> the rows of one channel of one view, the ones column, or nothing.
struct Column {
  const float* src;       // the push's rows of the view (this session)
  const float* tail;      // the live tail of the view
  long long ld;
  int c, tl, shift, ch;   // the view's channels and tail rows; lag - pre; the channel
  double fixed;           // kind != 0: the value (1 for the ones column, 0 beyond it)
  int kind;               // 0: data
};

__device__ __forceinline__ Column resolve(const CcaFitShape& sh, int kk, const float* eeg, long long ld_e,
                                          const float* feat, long long ld_f, const float* tail1,
                                          const float* tail2) {
  Column col;
  col.kind = 1;
  col.fixed = kk == sh.k1 + sh.k2 ? 1.0 : 0.0;
  col.src = eeg; col.tail = tail1; col.ld = ld_e; col.c = sh.c1; col.tl = sh.tl1; col.shift = 0; col.ch = 0;
  if (kk < sh.k1) {
    const int lag = kk / sh.c1;
    col.kind = 0; col.shift = lag - sh.pre1; col.ch = kk - lag * sh.c1;
  } else if (kk < sh.k1 + sh.k2) {
    const int kq = kk - sh.k1, lag = kq / sh.c2;
    col.kind = 0; col.src = feat; col.tail = tail2; col.ld = ld_f; col.c = sh.c2; col.tl = sh.tl2;
    col.shift = lag - sh.pre2; col.ch = kq - lag * sh.c2;
  }
  return col;
}

// grid (work tiles + the tail workgroup, sessions)
template <bool kForget>
__global__ void __launch_bounds__(kThreads) online_ccafit_kernel(CcaFitParams p) {
  __shared__ double vi[kPass][kTile];
  __shared__ double vj[kPass][kTile];
  const CcaFitShape& sh = p.s;
  const int s = blockIdx.y, tid = threadIdx.x;
  char* block = p.state + (long long)s * p.state_ss;
  double* M = reinterpret_cast<double*>(block);
  float* copies = reinterpret_cast<float*>(block) + sh.off_tail;
  const float* tail1 = copies + (long long)p.live * sh.tail_floats;
  const float* tail2 = tail1 + sh.off_ftail;
  const float* eeg = p.eeg + (long long)s * p.ss_e;
  const float* feat = p.feat + (long long)s * p.ss_f;
  const long long before = p.frames_before, after = p.frames_before + p.n;

  if ((int)blockIdx.x >= p.work_tiles) {
    // ---- the next tail copy: slot j of view v <- row after - (pre_v + post) + j
    float* next = copies + (long long)(1 - p.live) * sh.tail_floats;
    const int e_total = sh.tl1 * sh.c1, f_total = sh.tl2 * sh.c2;
    for (int e = tid; e < e_total; e += kThreads) {
      const int j = e / sh.c1, ch = e - j * sh.c1;
      next[e] = view_row(eeg, p.ld_e, tail1, sh.c1, sh.tl1, ch, after - sh.tl1 + j, before, after);
    }
    for (int e = tid; e < f_total; e += kThreads) {
      const int j = e / sh.c2, ch = e - j * sh.c2;
      next[sh.off_ftail + e] = view_row(feat, p.ld_f, tail2, sh.c2, sh.tl2, ch, after - sh.tl2 + j, before, after);
    }
    return;
  }

  // ---- which tile (ti, tj), tj >= ti
  int rem = (int)blockIdx.x, ti = 0;
  while (rem >= sh.tiles - ti) { rem -= sh.tiles - ti; ++ti; }
  const int tj = ti + rem;

  // ---- what this thread stages: column `col` of slice `half` (0: vi, 1: vj) of frames fr0, fr0 + 2, ..
  const int col = tid & 63, half = (tid >> 6) & 1, fr0 = tid >> 7;
  const Column cl = resolve(sh, (half == 0 ? ti : tj) * kTile + col, eeg, p.ld_e, feat, p.ld_f, tail1, tail2);

  // ---- the accumulators: rows ty + 16 a, columns tx + 16 b
  const int tx = tid & 15, ty = tid >> 4;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = ti * kTile + ty + 16 * a;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = tj * kTile + tx + 16 * b;
      acc[a][b] = (i < sh.n && j < sh.n) ? M[(long long)i * sh.n + j] : 0.0;
    }
  }

  const double g = p.g;
  for (long long f0 = 0; f0 < p.emitted; f0 += kPass) {
    const int np = p.emitted - f0 < kPass ? (int)(p.emitted - f0) : kPass;
    __syncthreads();                                         // (the pass before has been read)
    for (int q = fr0; q < np; q += 2) {
      double v = cl.fixed;
      if (cl.kind == 0)
        v = (double)view_row(cl.src, cl.ld, cl.tail, cl.c, cl.tl, cl.ch, p.e0 + f0 + q + cl.shift, before, after);
      if (half == 0) vi[q][col] = v;
      else vj[q][col] = v;
    }
    __syncthreads();
    for (int q = 0; q < np; ++q) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = vi[q][ty + 16 * u];
        b[u] = vj[q][tx + 16 * u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int w = 0; w < 4; ++w) acc[u][w] = step<kForget>(acc[u][w], a[u], b[w], g);
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = ti * kTile + ty + 16 * a;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = tj * kTile + tx + 16 * b;
      if (i < sh.n && j < sh.n) M[(long long)i * sh.n + j] = acc[a][b];
    }
  }
}

// grid (blocks, sessions): xtx [S][k1 + 1][k1 + 1] (the ones row and column last), x2tx2 [S][k2][k2],
// xtx2 [S][k1][k2], sum2 [S][k2]; any may be null
__global__ void __launch_bounds__(kThreads) online_ccafit_moments_kernel(const char* state, long long state_ss,
                                                                         CcaFitShape sh, double* xtx, double* x2tx2,
                                                                         double* xtx2, double* sum2) {
  const int s = blockIdx.y;
  const double* M = reinterpret_cast<const double*>(state + (long long)s * state_ss);
  const int n = sh.n, k1 = sh.k1, k2 = sh.k2, n1 = k1 + 1;
  const long long e_xx = (long long)n1 * n1, e_yy = (long long)k2 * k2, e_xy = (long long)k1 * k2;
  const long long total = e_xx + e_yy + e_xy + k2;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
    if (e < e_xx) {
      const int i = (int)(e / n1), j = (int)(e % n1);
      if (xtx) xtx[(long long)s * e_xx + e] = sym_at(M, n, i < k1 ? i : n - 1, j < k1 ? j : n - 1);
    } else if (e < e_xx + e_yy) {
      const long long r = e - e_xx;
      if (x2tx2) x2tx2[(long long)s * e_yy + r] = sym_at(M, n, k1 + (int)(r / k2), k1 + (int)(r % k2));
    } else if (e < e_xx + e_yy + e_xy) {
      const long long r = e - e_xx - e_yy;
      if (xtx2) xtx2[(long long)s * e_xy + r] = sym_at(M, n, (int)(r / k2), k1 + (int)(r % k2));
    } else {
      const long long r = e - e_xx - e_yy - e_xy;
      if (sum2) sum2[(long long)s * k2 + r] = sym_at(M, n, k1 + (int)r, n - 1);
    }
  }
}

// One view's part of the fitted stretch's statistics for column d of the float32 model: with m = sums / count,
//   mean = sum_i (m[i] - mu[i]) R[i][d],    q = R[:, d]^T (S / count - m m^T) R[:, d] = r^T S r / count - (m^T r)^2,
// every sum in float64 in a fixed order.  The column r = R[:, d] is widened into LDS once (r_s), so that the walk
// over S reads one coalesced row segment per step: a wave per row, a lane per column in four partial sums, the
// lanes' and the waves' sums combined in order.  Thread 0 holds the values.
__device__ __forceinline__ void view_statistics(const double* S, int ld, const double* sums, int k, double count,
                                                const float* mu, const float* R, int dim, int d, double* r_s,
                                                double* part, double* mean_out, double* q_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();                                           // (r_s and part of the view before have been read)
  for (int i = tid; i < k; i += kThreads) r_s[i] = (double)R[(long long)i * dim + d];
  __syncthreads();
  double rsr = 0.0, mr = 0.0, dm = 0.0;
  for (int i = wave; i < k; i += kThreads / 64) {
    const double* row = S + (long long)i * ld;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int j = lane;
    for (; j + 192 < k; j += 256) {
      a0 = fma(row[j], r_s[j], a0);
      a1 = fma(row[j + 64], r_s[j + 64], a1);
      a2 = fma(row[j + 128], r_s[j + 128], a2);
      a3 = fma(row[j + 192], r_s[j + 192], a3);
    }
    if (j < k) a0 = fma(row[j], r_s[j], a0);
    if (j + 64 < k) a1 = fma(row[j + 64], r_s[j + 64], a1);
    if (j + 128 < k) a2 = fma(row[j + 128], r_s[j + 128], a2);
    rsr = fma(r_s[i], (a0 + a1) + (a2 + a3), rsr);
  }
  for (int i = tid; i < k; i += kThreads) {
    const double mi = sums[i] / count;
    mr = fma(mi, r_s[i], mr);
    dm = fma(mi - (double)mu[i], r_s[i], dm);
  }
  rsr = wave_sum(rsr); mr = wave_sum(mr); dm = wave_sum(dm);
  if (lane == 0) { part[wave] = rsr; part[4 + wave] = mr; part[8 + wave] = dm; }
  __syncthreads();
  if (tid == 0) {
    const double a = (part[0] + part[1]) + (part[2] + part[3]);
    const double b = (part[4] + part[5]) + (part[6] + part[7]);
    *mean_out = (part[8] + part[9]) + (part[10] + part[11]);
    *q_out = a / count - b * b;
  }
}

// grid (dim): corr [3][dim] = {mean_a, mean_b, power} of one (session, lambda), from the dense moments the solve
// left in the workspace and the float32 model it returned.  (A workgroup takes both views of its column: the power
// is the square root of the PRODUCT of the two quadratic forms, and no workgroup reads what another writes.)
__global__ void __launch_bounds__(kThreads) online_ccafit_corr_kernel(const double* xtx, const double* x2tx2,
                                                                      const double* sum2, int k1, int k2,
                                                                      const float* mean_x, const float* rot_x,
                                                                      const float* mean_y, const float* rot_y,
                                                                      int dim, double* corr) {
  __shared__ double r_s[kMaxK];                              // 16 KiB: a view has at most kMaxK - 1 columns
  __shared__ double part[12];
  const int d = blockIdx.x, n1 = k1 + 1;
  const double count = xtx[(long long)k1 * n1 + k1];
  double mean_a = 0.0, mean_b = 0.0, qx = 0.0, qy = 0.0;
  view_statistics(xtx, n1, xtx + (long long)k1 * n1, k1, count, mean_x, rot_x, dim, d, r_s, part, &mean_a, &qx);
  view_statistics(x2tx2, k2, sum2, k2, count, mean_y, rot_y, dim, d, r_s, part, &mean_b, &qy);
  if (threadIdx.x == 0) {
    corr[d] = mean_a;
    corr[dim + d] = mean_b;
    corr[2 * dim + d] = sqrt(qx * qy);
  }
}

int launch_moments(td_handle* h, int num_sessions, const char* state, long long stride, const CcaFitShape& sh,
                   double* xtx, double* x2tx2, double* xtx2, double* sum2) {
  const long long per = (long long)(sh.k1 + 1) * (sh.k1 + 1) + (long long)sh.k2 * (sh.k1 + sh.k2 + 1);
  hipLaunchKernelGGL(online_ccafit_moments_kernel, dim3(blocks_for(per), (unsigned)num_sessions), dim3(kThreads), 0,
                     h->stream, state, stride, sh, xtx, x2tx2, xtx2, sum2);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

}  // namespace

extern "C" {

int td_ccafit_online_state_bytes(int c1, int pre1, int post1, int c2, int pre2, int post2, int64_t* bytes) {
  if (!bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_ccafit_online_state_bytes: NULL argument");
  CcaFitShape sh;
  TD_TRY(ccafit_shape(nullptr, "td_ccafit_online_state_bytes", c1, pre1, post1, c2, pre2, post2, &sh));
  *bytes = sh.bytes;
  return TD_OK;
}

int td_ccafit_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t ld_eeg,
                          int64_t eeg_session_stride, const float* feat_dev, int64_t ld_feat,
                          int64_t feat_session_stride, int64_t n, int c1, int pre1, int post1, int c2, int pre2,
                          int post2, int64_t frames_before, int64_t pushes_before, int flush, double forget,
                          void* state_dev, int64_t state_session_stride) {
  const char* who = "td_ccafit_online_push";
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "%s: handle is NULL", who);
  CcaFitShape sh;
  TD_TRY(ccafit_shape(h, who, c1, pre1, post1, c2, pre2, post2, &sh));
  TD_TRY(check_fit_push(h, who, num_sessions, eeg_dev, ld_eeg, eeg_session_stride, c1, feat_dev, ld_feat,
                        feat_session_stride, c2, "features", n, frames_before, pushes_before, forget, state_dev,
                        state_session_stride, sh.bytes));
  const OnlinePlan pl = plan_push(frames_before, n, sh.post, 1, 1, flush);
  const long long emitted = pl.emitted_after - pl.emitted_before;
  if (n == 0 && emitted == 0) return TD_OK;

  CcaFitParams p;
  memset(&p, 0, sizeof(p));
  p.eeg = eeg_dev; p.ld_e = ld_eeg; p.ss_e = num_sessions > 1 ? eeg_session_stride : 0;
  p.feat = feat_dev; p.ld_f = ld_feat; p.ss_f = num_sessions > 1 ? feat_session_stride : 0;
  p.n = n; p.frames_before = frames_before; p.e0 = pl.emitted_before; p.emitted = emitted;
  p.work_tiles = emitted > 0 ? upper_tiles(sh.tiles) : 0;
  p.live = (int)(pushes_before & 1);
  p.g = forget;
  p.state = reinterpret_cast<char*>(state_dev); p.state_ss = state_session_stride;
  p.s = sh;
  const dim3 grid((unsigned)(p.work_tiles + (n > 0 ? 1 : 0)), (unsigned)num_sessions);
  TD_TRY(td_profile_mark(h, true, (double)n * num_sessions));
  if (forget < 1.0) hipLaunchKernelGGL(online_ccafit_kernel<true>, grid, dim3(kThreads), 0, h->stream, p);
  else hipLaunchKernelGGL(online_ccafit_kernel<false>, grid, dim3(kThreads), 0, h->stream, p);
  TD_HIP(h, hipGetLastError());
  TD_TRY(td_profile_mark(h, false, 0.0));
  return TD_OK;
}

int td_ccafit_online_moments(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride,
                             int c1, int pre1, int post1, int c2, int pre2, int post2, double* xtx_dev,
                             double* x2tx2_dev, double* xtx2_dev, double* sum2_dev) {
  const char* who = "td_ccafit_online_moments";
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "%s: handle is NULL", who);
  CcaFitShape sh;
  TD_TRY(ccafit_shape(h, who, c1, pre1, post1, c2, pre2, post2, &sh));
  TD_TRY(check_state(h, who, num_sessions, state_dev, state_session_stride, sh.bytes));
  if (!xtx_dev && !x2tx2_dev && !xtx2_dev && !sum2_dev) return td_fail(h, TD_ERR_INVALID, "%s: NULL argument", who);
  return launch_moments(h, num_sessions, reinterpret_cast<const char*>(state_dev), state_session_stride, sh, xtx_dev,
                        x2tx2_dev, xtx2_dev, sum2_dev);
}

int td_ccafit_online_solve(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride,
                           int c1, int pre1, int post1, int c2, int pre2, int post2, int64_t frames_emitted,
                           const double* lambdas_host, int n_lambda, int dim, double eps_eig, float* rot_x_dev,
                           float* rot_y_dev, float* mean_x_dev, float* mean_y_dev, float* e_dev, double* corr_dev,
                           int* info_host) {
  const char* who = "td_ccafit_online_solve";
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "%s: handle is NULL", who);
  CcaFitShape sh;
  TD_TRY(ccafit_shape(h, who, c1, pre1, post1, c2, pre2, post2, &sh));
  TD_TRY(check_state(h, who, num_sessions, state_dev, state_session_stride, sh.bytes));
  if (!lambdas_host || !rot_x_dev || !rot_y_dev || !mean_x_dev || !mean_y_dev || !e_dev || !corr_dev)
    return td_fail(h, TD_ERR_INVALID, "%s: NULL argument", who);
  TD_REQUIRE(h, n_lambda >= 1, "%s: %d lambdas (at least 1)", who, n_lambda);
  for (int i = 0; i < n_lambda; ++i)
    TD_REQUIRE(h, lambdas_host[i] >= 0.0 && std::isfinite(lambdas_host[i]), "%s: lambda %d is %g (finite, >= 0)", who,
               i, lambdas_host[i]);
  const int k1 = sh.k1, k2 = sh.k2;
  TD_REQUIRE(h, dim >= 1 && dim <= std::min(kMaxDims, std::min(k1, k2)), "%s: dim must be in [1, %d], not %d", who,
             std::min(kMaxDims, std::min(k1, k2)), dim);
  if (frames_emitted < 2)
    return td_fail(h, TD_ERR_STATE, "%s: %lld frames counted (the covariance needs at least 2)", who,
                   (long long)frames_emitted);
  // The count the covariances divide by is the state's own M[n - 1][n - 1] (the frame count, or the effective count
  // under forgetting), read once per session; denom = count - 1 is the reference's for one minibatch of all frames.
  for (int s = 0; s < num_sessions; ++s) {
    const char* block = reinterpret_cast<const char*>(state_dev) + (long long)s * state_session_stride;
    double count = 0.0;
    TD_HIP(h, hipMemcpyAsync(&count, reinterpret_cast<const double*>(block) + (long long)sh.n * sh.n - 1,
                             sizeof(double), hipMemcpyDeviceToHost, h->stream));
    TD_HIP(h, hipStreamSynchronize(h->stream));
    if (!(count > 1.0))
      return td_fail(h, TD_ERR_STATE, "%s: session %d has an effective count of %g frames (more than 1)", who, s,
                     count);
    for (int li = 0; li < n_lambda; ++li) {
      const long long sl = (long long)s * n_lambda + li;
      float* rot_x = rot_x_dev + sl * k1 * dim;
      float* rot_y = rot_y_dev + sl * k2 * dim;
      float* mean_x = mean_x_dev + (long long)s * k1;
      float* mean_y = mean_y_dev + (long long)s * k2;
      td_cca_ws w;
      TD_TRY(td_cca_workspace(h, k1, k2, dim, &w));
      TD_TRY(launch_moments(h, 1, block, state_session_stride, sh, w.xtx, w.x2tx2, w.xtx2, w.sum2));
      TD_TRY(td_cca_dense(h, k1, k2, count, w.xtx, k1 + 1, w.x2tx2, w.xtx2, w.xtx + (size_t)k1 * (k1 + 1), w.sum2,
                          nullptr, count - 1.0, lambdas_host[li], eps_eig, dim, rot_x, rot_y, mean_x, mean_y,
                          e_dev + sl * dim, info_host ? info_host + 4 * sl : nullptr));
      hipLaunchKernelGGL(online_ccafit_corr_kernel, dim3((unsigned)dim), dim3(kThreads), 0, h->stream, w.xtx, w.x2tx2,
                         w.sum2, k1, k2, mean_x, rot_x, mean_y, rot_y, dim, corr_dev + sl * 3 * dim);
      TD_HIP(h, hipGetLastError());
    }
  }
  TD_HIP(h, hipStreamSynchronize(h->stream));
  return TD_OK;
}

}  // extern "C"
