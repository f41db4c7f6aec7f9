// The online ridge fit (td_fit_online_*): the exact moments of the lagged regression -- [x~ | 1]^T [x~ | 1] and
// [x~ | 1]^T y in float64 -- for (eeg, target) rows that arrive in pushes of any length, as the online family does
// everything else: the state on the device, ONE launch per push for a bank of sessions, and any cut of a recording
// gives the bytes of one push.  td_fit_online_solve turns the moments into ridge weights on the device.
//
// Frames.  The lagged vector v of frame t is oracle/lag.py's row t: v[l c + ch] = x[t + l - pre][ch], zero outside
// the recording, and v[K] = 1 (the reference's ones column, brain_model.py:434-436).  Frames are emitted `post` rows
// late as td_online_push emits them: after `pushed` rows emitted = max(0, pushed - post); a push that carries flush
// emits the rest, `post` zero rows behind the end.
//
// The sum.  For every newly emitted frame, in frame order, A[i][j] = A[i][j] g + v[i] v[j] and
// B[i][o] = B[i][o] g + v[i] y[t][o] in float64.  The inputs are float32, so a product is exact; with g == 1 an
// element takes ONE rounding per frame (a fused multiply-add of the widened values), with g < 1 two,
// round(round(acc g) + p), written so that nothing fuses them (see step()).  The order is a function
// of the frame index alone -- not of the cut, not of a pass -- so NumPy's A * g + np.outer(v, v) in frame order is a
// bit-exact twin.
//
// The launch.  grid (upper-triangular 64 x 64 tiles of A + the 64-row tiles of B + one tail workgroup, sessions),
// 256 threads; a thread owns a 4 x 4 block of accumulators, rows ty + 16 p and columns tx + 16 q of its tile, so
// that the 8-byte LDS reads of a half wave are 16 consecutive doubles (or one address): no bank conflict.  A
// workgroup stages the two 64-wide slices of the lagged vectors of a pass of kPass frames into LDS as float64 --
// from the tail, the push or zeros -- then every thread walks the pass in frame order.  Only tiles with tj >= ti
// are computed and stored (a diagonal tile whole: its two triangles hold the same bits); the lower tiles of the
// state stay zero and td_fit_online_moments mirrors.
//
// The state.  A [(K + 1)^2] float64, B [(K + 1) d] float64, then TWO tail copies of {EEG [pre + post][c], target
// [post][d]} float32: slot j of a copy holds row pushed - (pre + post) + j (target: pushed - post + j), zero before
// row 0, so all zeros = fresh.  A session is many workgroups, and the rows a push retires from the tail are rows
// other workgroups still read: a launch reads copy (pushes_before & 1) and the tail workgroup writes every slot of
// the other one.  The host counts the pushes with n > 0; a push without rows writes no tail.  No workgroup reads
// what another writes, no atomics, vector stores only.
//
// What this file shares with online_cca_fit.hip -- step(), view_row(), the tiling and a thread's accumulators, the
// checks of a push -- is online_fit_common.h.  Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are in
// DESIGN.md section 34.
#include <cmath>

#pragma clang fp contract(off)

#include "online_fit_common.h"

namespace {

constexpr int kMaxChannels = TD_ONLINE_FIT_MAX_CHANNELS;
constexpr int kMaxLags = TD_ONLINE_FIT_MAX_LAGS;
constexpr int kMaxK = TD_ONLINE_FIT_MAX_K;
constexpr int kMaxOutputs = TD_ONLINE_FIT_MAX_OUTPUTS;

struct FitShape {
  int c, pre, post, d, k, n1, tiles;           // n1 = K + 1, tiles = ceil(n1 / 64)
  long long off_b;                             // (doubles) B behind A
  long long off_tail, tail_floats, off_ttail;  // (floats) the first tail copy, one copy's length, the target tail in a copy
  long long bytes;
};

struct FitParams {
  const float* eeg; long long ld_e, ss_e;
  const float* tgt; long long ld_t, ss_t;
  long long n, frames_before, e0;
  long long emitted;
  int a_tiles, work_tiles, live;
  double g;
  char* state; long long state_ss;             // (bytes)
  FitShape s;
};

int fit_shape(td_handle* h, const char* who, int c, int pre, int post, int d, FitShape* s) {
  TD_REQUIRE(h, c >= 1 && c <= kMaxChannels, "%s: %d channels (1 .. %d)", who, c, kMaxChannels);
  TD_REQUIRE(h, pre >= 0 && post >= 0 && pre + 1 + post <= kMaxLags, "%s: a context of %d + 1 + %d lags (1 .. %d)",
             who, pre, post, kMaxLags);
  const int k = (pre + 1 + post) * c;
  TD_REQUIRE(h, k <= kMaxK, "%s: %d lags x %d channels = %d lagged inputs (at most %d)", who, pre + 1 + post, c, k,
             kMaxK);
  TD_REQUIRE(h, d >= 1 && d <= kMaxOutputs, "%s: %d outputs (1 .. %d)", who, d, kMaxOutputs);
  s->c = c; s->pre = pre; s->post = post; s->d = d; s->k = k; s->n1 = k + 1;
  s->tiles = tiles_of(k + 1);
  s->off_b = (long long)s->n1 * s->n1;
  s->off_tail = 2 * (s->off_b + (long long)s->n1 * d);
  s->off_ttail = (long long)(pre + post) * c;
  s->tail_floats = s->off_ttail + (long long)post * d;
  s->bytes = td_round_up(4 * (s->off_tail + 2 * s->tail_floats), 8);
  return TD_OK;
}

// grid (work tiles + the tail workgroup, sessions)
template <bool kForget>
__global__ void __launch_bounds__(kThreads) online_fit_kernel(FitParams p) {
  __shared__ double vi[kPass][kTile];
  __shared__ double vj[kPass][kTile];
  const FitShape& sh = p.s;
  const int s = blockIdx.y, tid = threadIdx.x;
  const int c = sh.c, d = sh.d, tl = sh.pre + sh.post;
  char* block = p.state + (long long)s * p.state_ss;
  double* A = reinterpret_cast<double*>(block);
  double* B = A + sh.off_b;
  float* copies = reinterpret_cast<float*>(block) + sh.off_tail;
  const float* tail = copies + (long long)p.live * sh.tail_floats;
  const float* ttail = tail + sh.off_ttail;
  const float* eeg = p.eeg + (long long)s * p.ss_e;
  const float* tgt = p.tgt + (long long)s * p.ss_t;
  const long long before = p.frames_before, after = p.frames_before + p.n;

  if ((int)blockIdx.x >= p.work_tiles) {
    // ---- the next tail copy: EEG slot j <- row after - (pre + post) + j, target slot j <- row after - post + j
    float* next = copies + (long long)(1 - p.live) * sh.tail_floats;
    const int e_total = tl * c, t_total = sh.post * d;
    for (int e = tid; e < e_total; e += kThreads) {
      const int j = e / c, ch = e - j * c;
      const long long r = after - tl + j;
      float v = 0.0f;
      if (r >= before) v = eeg[(r - before) * p.ld_e + ch];
      else if (r >= 0) v = tail[(r - (before - tl)) * c + ch];
      next[e] = v;
    }
    for (int e = tid; e < t_total; e += kThreads) {
      const int j = e / d, o = e - j * d;
      const long long r = after - sh.post + j;
      float v = 0.0f;
      if (r >= before) v = tgt[(r - before) * p.ld_t + o];
      else if (r >= 0) v = ttail[(r - (before - sh.post)) * d + o];
      next[sh.off_ttail + e] = v;
    }
    return;
  }

  // ---- which tile: A (ti, tj), tj >= ti, or B rows of tile ti
  const bool is_b = (int)blockIdx.x >= p.a_tiles;
  int ti, tj = 0;
  if (is_b) {
    ti = (int)blockIdx.x - p.a_tiles;
  } else {
    int rem = (int)blockIdx.x;
    ti = 0;
    while (rem >= sh.tiles - ti) { rem -= sh.tiles - ti; ++ti; }
    tj = ti + rem;
  }

  // ---- what this thread stages: column `col` of slice `half` (0: vi, 1: vj / the targets) of frames fr0, fr0 + 2, ..
  const int col = tid & 63, half = (tid >> 6) & 1, fr0 = tid >> 7;
  const bool stage_y = is_b && half == 1;
  const int kk = (half == 0 ? ti : tj) * kTile + col;       // the lagged input (unused for the targets)
  const int lag = kk < sh.k ? kk / c : 0;
  const int ch = kk < sh.k ? kk - lag * c : 0;
  const double fixed = kk == sh.k ? 1.0 : 0.0;               // the ones column, zero beyond it

  // ---- the accumulators
  const int tx = tid & 15, ty = tid >> 4;                    // A: rows ty + 16 p, columns tx + 16 q
  const int brow = tid & 63, bo = tid >> 6;                  // B: row brow, outputs bo and bo + 4
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  if (is_b) {
    const int i = ti * kTile + brow;
    if (i < sh.n1) {
      if (bo < d) acc[0][0] = B[(long long)i * d + bo];
      if (bo + 4 < d) acc[0][1] = B[(long long)i * d + bo + 4];
    }
  } else {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int i = ti * kTile + ty + 16 * a;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int j = tj * kTile + tx + 16 * b;
        if (i < sh.n1 && j < sh.n1) acc[a][b] = A[(long long)i * sh.n1 + j];
      }
    }
  }

  const double g = p.g;
  for (long long f0 = 0; f0 < p.emitted; f0 += kPass) {
    const int np = p.emitted - f0 < kPass ? (int)(p.emitted - f0) : kPass;
    __syncthreads();                                         // (the pass before has been read)
    for (int q = fr0; q < np; q += 2) {
      const long long f = p.e0 + f0 + q;
      double v;
      if (stage_y) {
        v = 0.0;
        if (col < d) {
          if (f >= before) v = (double)tgt[(f - before) * p.ld_t + col];
          else if (f >= before - sh.post) v = (double)ttail[(f - (before - sh.post)) * d + col];
        }
      } else if (kk >= sh.k) {
        v = fixed;
      } else {
        const long long r = f + lag - sh.pre;
        v = 0.0;
        if (r >= after || r < 0) v = 0.0;                    // behind a flushed end, before the recording
        else if (r >= before) v = (double)eeg[(r - before) * p.ld_e + ch];
        else if (r >= before - tl) v = (double)tail[(r - (before - tl)) * c + ch];
      }
      if (half == 0) vi[q][col] = v;
      else vj[q][col] = v;
    }
    __syncthreads();
    if (is_b) {
      for (int q = 0; q < np; ++q) {
        const double a = vi[q][brow];
        acc[0][0] = step<kForget>(acc[0][0], a, vj[q][bo], g);
        acc[0][1] = step<kForget>(acc[0][1], a, vj[q][bo + 4], g);
      }
    } else {
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
  }

  if (is_b) {
    const int i = ti * kTile + brow;
    if (i < sh.n1) {
      if (bo < d) B[(long long)i * d + bo] = acc[0][0];
      if (bo + 4 < d) B[(long long)i * d + bo + 4] = acc[0][1];
    }
  } else {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int i = ti * kTile + ty + 16 * a;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int j = tj * kTile + tx + 16 * b;
        if (i < sh.n1 && j < sh.n1) A[(long long)i * sh.n1 + j] = acc[a][b];
      }
    }
  }
}

// grid (blocks, sessions): xtx [S][n1][n1], xty [S][n1][d]
__global__ void __launch_bounds__(kThreads) online_fit_moments_kernel(const char* state, long long state_ss,
                                                                      FitShape sh, double* xtx, double* xty) {
  const int s = blockIdx.y;
  const double* A = reinterpret_cast<const double*>(state + (long long)s * state_ss);
  const double* B = A + sh.off_b;
  const long long nn = (long long)sh.n1 * sh.n1, nd = (long long)sh.n1 * sh.d;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < nn + nd; e += (long long)gridDim.x * kThreads) {
    if (e < nn) {
      if (xtx) xtx[(long long)s * nn + e] = sym_at(A, sh.n1, (int)(e / sh.n1), (int)(e % sh.n1));
    } else if (xty) {
      xty[(long long)s * nd + (e - nn)] = B[e - nn];
    }
  }
}

// grid (blocks, sessions x lambdas): a [S nl][n1][n1] = A_sym / A[K][K] + lambda I, rhs [S nl][n1][d] = B / A[K][K]
__global__ void __launch_bounds__(kThreads) online_fit_systems_kernel(const char* state, long long state_ss,
                                                                      FitShape sh, const double* lams, int n_lambda,
                                                                      double* a, double* rhs) {
  const int sys = blockIdx.y, s = sys / n_lambda, li = sys - s * n_lambda;
  const double* A = reinterpret_cast<const double*>(state + (long long)s * state_ss);
  const double* B = A + sh.off_b;
  const long long nn = (long long)sh.n1 * sh.n1, nd = (long long)sh.n1 * sh.d;
  const double count = A[nn - 1], lam = lams[li];
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < nn + nd; e += (long long)gridDim.x * kThreads) {
    if (e < nn) {
      const int i = (int)(e / sh.n1), j = (int)(e % sh.n1);
      const double v = sym_at(A, sh.n1, i, j) / count;
      a[(long long)sys * nn + e] = i == j ? v + lam : v;
    } else {
      rhs[(long long)sys * nd + (e - nn)] = B[e - nn] / count;
    }
  }
}

// sol [S nl][n1][d] -> W [S nl][K][d], b [S nl][d] float32
__global__ void __launch_bounds__(kThreads) online_fit_emit_kernel(const double* sol, int k, int d, float* w, float* b) {
  const int sys = blockIdx.y;
  const long long nd = (long long)(k + 1) * d;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < nd; e += (long long)gridDim.x * kThreads) {
    const float v = (float)sol[(long long)sys * nd + e];
    if (e < (long long)k * d) w[(long long)sys * k * d + e] = v;
    else b[(long long)sys * d + (e - (long long)k * d)] = v;
  }
}

}  // namespace

extern "C" {

int td_fit_online_state_bytes(int c, int pre, int post, int d, int64_t* bytes) {
  if (!bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_fit_online_state_bytes: NULL argument");
  FitShape sh;
  TD_TRY(fit_shape(nullptr, "td_fit_online_state_bytes", c, pre, post, d, &sh));
  *bytes = sh.bytes;
  return TD_OK;
}

int td_fit_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t ld_eeg,
                       int64_t eeg_session_stride, const float* target_dev, int64_t ld_target,
                       int64_t target_session_stride, int64_t n, int c, int pre, int post, int d,
                       int64_t frames_before, int64_t pushes_before, int flush, double forget, void* state_dev,
                       int64_t state_session_stride) {
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_fit_online_push: handle is NULL");
  FitShape sh;
  TD_TRY(fit_shape(h, "td_fit_online_push", c, pre, post, d, &sh));
  TD_TRY(check_fit_push(h, "td_fit_online_push", num_sessions, eeg_dev, ld_eeg, eeg_session_stride, c, target_dev,
                        ld_target, target_session_stride, d, "outputs", n, frames_before, pushes_before, forget,
                        state_dev, state_session_stride, sh.bytes));
  const OnlinePlan pl = plan_push(frames_before, n, post, 1, 1, flush);
  const long long emitted = pl.emitted_after - pl.emitted_before;
  if (n == 0 && emitted == 0) return TD_OK;

  FitParams p;
  memset(&p, 0, sizeof(p));
  p.eeg = eeg_dev; p.ld_e = ld_eeg; p.ss_e = num_sessions > 1 ? eeg_session_stride : 0;
  p.tgt = target_dev; p.ld_t = ld_target; p.ss_t = num_sessions > 1 ? target_session_stride : 0;
  p.n = n; p.frames_before = frames_before; p.e0 = pl.emitted_before; p.emitted = emitted;
  p.a_tiles = upper_tiles(sh.tiles);
  p.work_tiles = emitted > 0 ? p.a_tiles + sh.tiles : 0;
  p.live = (int)(pushes_before & 1);
  p.g = forget;
  p.state = reinterpret_cast<char*>(state_dev); p.state_ss = state_session_stride;
  p.s = sh;
  const dim3 grid((unsigned)(p.work_tiles + (n > 0 ? 1 : 0)), (unsigned)num_sessions);
  TD_TRY(td_profile_mark(h, true, (double)n * num_sessions));
  if (forget < 1.0) hipLaunchKernelGGL(online_fit_kernel<true>, grid, dim3(kThreads), 0, h->stream, p);
  else hipLaunchKernelGGL(online_fit_kernel<false>, grid, dim3(kThreads), 0, h->stream, p);
  TD_HIP(h, hipGetLastError());
  TD_TRY(td_profile_mark(h, false, 0.0));
  return TD_OK;
}

int td_fit_online_moments(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride, int c,
                          int pre, int post, int d, double* xtx_dev, double* xty_dev) {
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_fit_online_moments: handle is NULL");
  FitShape sh;
  TD_TRY(fit_shape(h, "td_fit_online_moments", c, pre, post, d, &sh));
  TD_TRY(check_state(h, "td_fit_online_moments", num_sessions, state_dev, state_session_stride, sh.bytes));
  if (!xtx_dev && !xty_dev) return td_fail(h, TD_ERR_INVALID, "td_fit_online_moments: NULL argument");
  const long long per = (long long)sh.n1 * (sh.n1 + d);
  hipLaunchKernelGGL(online_fit_moments_kernel, dim3(blocks_for(per), (unsigned)num_sessions), dim3(kThreads), 0,
                     h->stream, reinterpret_cast<const char*>(state_dev), (long long)state_session_stride, sh,
                     xtx_dev, xty_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_fit_online_solve(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride, int c,
                        int pre, int post, int d, int64_t frames_emitted, const double* lambdas_host, int n_lambda,
                        float* w_dev, float* b_dev) {
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_fit_online_solve: handle is NULL");
  FitShape sh;
  TD_TRY(fit_shape(h, "td_fit_online_solve", c, pre, post, d, &sh));
  TD_TRY(check_state(h, "td_fit_online_solve", num_sessions, state_dev, state_session_stride, sh.bytes));
  if (!lambdas_host || !w_dev || !b_dev) return td_fail(h, TD_ERR_INVALID, "td_fit_online_solve: NULL argument");
  TD_REQUIRE(h, n_lambda >= 1 && (long long)n_lambda * num_sessions <= 65535,
             "td_fit_online_solve: %d lambdas for %d sessions (1 .. 65535 systems)", n_lambda, num_sessions);
  for (int i = 0; i < n_lambda; ++i)
    TD_REQUIRE(h, std::isfinite(lambdas_host[i]), "td_fit_online_solve: lambda %d is %g (finite)", i, lambdas_host[i]);
  if (frames_emitted <= 0)
    return td_fail(h, TD_ERR_STATE, "td_fit_online_solve: no frame emitted yet (the moments are empty)");
  const int systems = n_lambda * num_sessions;
  const long long nn = (long long)sh.n1 * sh.n1, nd = (long long)sh.n1 * d;
  const long long lam_bytes = td_round_up(8LL * n_lambda, 256);
  const long long bytes = lam_bytes + 8LL * systems * (nn + nd);
  if (bytes > TD_ONLINE_FIT_MAX_SOLVE_BYTES)
    return td_fail(h, TD_ERR_NOMEM,
                   "td_fit_online_solve: %d systems of %d unknowns need %lld bytes of dense systems (at most %lld): "
                   "solve fewer sessions or lambdas per call", systems, sh.n1, bytes,
                   (long long)TD_ONLINE_FIT_MAX_SOLVE_BYTES);
  // (td_spd_solve pads the systems into the handle's solver workspace and solves them there; what it reads and
  // leaves the solutions in is the handle's other arena)
  void* base = nullptr;
  TD_TRY(td_scratch(h, (size_t)bytes, &base));
  double* lams = reinterpret_cast<double*>(base);
  double* a = reinterpret_cast<double*>(reinterpret_cast<char*>(base) + lam_bytes);
  double* rhs = a + (long long)systems * nn;
  TD_TRY(td_upload_async(h, lambdas_host, sizeof(double) * n_lambda, lams));
  hipLaunchKernelGGL(online_fit_systems_kernel, dim3(blocks_for(nn + nd), (unsigned)systems), dim3(kThreads), 0,
                     h->stream, reinterpret_cast<const char*>(state_dev), (long long)state_session_stride, sh, lams,
                     n_lambda, a, rhs);
  TD_HIP(h, hipGetLastError());
  TD_TRY(td_spd_solve(h, a, rhs, sh.n1, d, systems));         // (TD_ERR_SINGULAR: not positive definite)
  hipLaunchKernelGGL(online_fit_emit_kernel, dim3(blocks_for(nd), (unsigned)systems), dim3(kThreads), 0, h->stream,
                     rhs, sh.k, d, w_dev, b_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

}  // extern "C"
