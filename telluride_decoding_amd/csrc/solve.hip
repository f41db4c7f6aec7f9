// A3 -- ridge solve: the routes.  td_ridge_solve / _async / _multi pick between the one-launch conjugate
// gradients of cg.hip (on the compact statistics or on the dense moments) and the batched float64
// factorisation of chol.hip, which also owns the "Singular matrix" report; targets wider than the batched
// solver carries go through the td_chol_* helpers one lambda at a time.
//
// Reference: brain_model.calculate_linear_regressor_parameters_from_dataset,
// brain_model.py:447-455 (normalise by n, add lambda to EVERY diagonal entry incl.
// the bias) and :477 (np.linalg.solve -- a general LU in the input dtype).  The
// regularised matrix is symmetric positive definite, so Cholesky in float64 gives
// the same solution to well below the reference's own float32 rounding noise.
#include "solve_common.h"

namespace {

using namespace td_tile64;   // NB

// td_ridge_solve: when the one-launch conjugate-gradient solve (cg.hip) is tried first
// (measured, tools/time_cg.py at 64 channels x 2..32 lags: one system 0.12 / 0.16 / 0.19 / 0.35 ms at
// n = 129 / 513 / 769 / 2049 against 0.20 / 0.39 / 0.51 / 1.15 for the factorisation; the systems run one
// after another, the batched factorisation shares its chain: two systems win from n = 129 by little and
// from 257 clearly, four only from n = 513 -- 0.40 against 0.47)
constexpr int kCgAutoSystems = 4;     // (lambda, output) systems at most
constexpr int kCgAutoMinN1 = 128;     // smallest n for one system,
constexpr int kCgAutoMinN2 = 192;     // two,
constexpr int kCgAutoMinN4 = 512;     // three or four
constexpr int kCgMaxIter = 400;
constexpr int kCgAutoMaxIter = 160;   // the automatic route gives up early (the factorisation follows)
constexpr double kCgTol = 1e-12;      // relative residual, as td_ridge_solve_loso

__global__ void ridge_emit_kernel(const double* __restrict__ sol, int k1, int d, int np, int batch,
                                  float* __restrict__ w, float* __restrict__ bias) {
  const long long total = (long long)batch * (k1 + 1) * d;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(i % d);
    const int r = (int)((i / d) % (k1 + 1));
    const int b = (int)(i / ((long long)d * (k1 + 1)));
    const float v = (float)sol[((size_t)b * kMaxRhs + q) * np + r];
    if (r < k1) w[((size_t)b * k1 + r) * d + q] = v;
    else bias[(size_t)b * d + q] = v;
  }
}

// The ring of asynchronous result flags (td_ridge_solve_async / _multi): slot = the next of
// kAsyncFlags pinned host ints + device ints.  A slot is handed out again only when the copy that
// filled it last has COMPLETED (an event per slot): with more than kAsyncFlags solves outstanding the
// new call would overwrite a flag the caller cannot have read yet -- TD_ERR_STATE instead of a
// silently stale (or clobbered) flag.
int async_slot_acquire(td_handle* h, int* slot_out) {
  if (!h->dev_flags) {
    TD_HIP(h, hipMalloc(reinterpret_cast<void**>(&h->dev_flags), sizeof(int) * td_handle::kAsyncFlags));
    TD_HIP(h, hipHostMalloc(reinterpret_cast<void**>(&h->host_flags), sizeof(int) * td_handle::kAsyncFlags,
                            hipHostMallocDefault));
  }
  const int slot = h->async_next;
  if (h->async_events[slot]) {
    const hipError_t q = hipEventQuery(h->async_events[slot]);
    if (q == hipErrorNotReady)
      return td_fail(h, TD_ERR_STATE,
                     "asynchronous solve: the ring of %d result flags is full (the solve that owns the oldest "
                     "slot has not finished): wait for an earlier solve and read its flag first",
                     td_handle::kAsyncFlags);
    if (q != hipSuccess) return td_fail(h, TD_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
  }
  h->async_next = (h->async_next + 1) % td_handle::kAsyncFlags;
  *slot_out = slot;
  return TD_OK;
}

// ... and the copy of slot's device flag to its host int, with the event that frees the slot
int async_slot_publish(td_handle* h, int slot, bool copy_from_device) {
  if (copy_from_device)
    TD_HIP(h, hipMemcpyAsync(h->host_flags + slot, h->dev_flags + slot, sizeof(int), hipMemcpyDeviceToHost,
                             h->stream));
  if (!h->async_events[slot]) TD_HIP(h, hipEventCreateWithFlags(&h->async_events[slot], hipEventDisableTiming));
  TD_HIP(h, hipEventRecord(h->async_events[slot], h->stream));
  return TD_OK;
}

// ---- ridge solve with more than kMaxRhs outputs (a forward model: D = EEG channels) --------------
// The batched solver carries at most kMaxRhs right-hand-side rows per system (they ride in its
// panel and update kernels).  Wider targets go through the Cholesky helpers of chol.hip, one lambda at
// a time: factor cov + lambda I with up to 64 columns of cov_xy riding along (forward
// substitution), backward substitution 8 rows at a time; more than 64 outputs factor again per
// 64 columns.  Same arithmetic (float64 Cholesky), same failure (TD_ERR_SINGULAR), synchronous.
// out [nb][n]: column c0 + q of xty [n][d], scaled
__global__ void xty_rows_kernel(const double* __restrict__ xty, int n, int d, int c0, int nb, double inv,
                                double* __restrict__ out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nb * n; i += gridDim.x * blockDim.x)
    out[i] = xty[(size_t)(i % n) * d + c0 + i / n] * inv;
}

// sol [nb][n] (row q = output c0 + q; entry k1 = the bias) -> W [k1][d], b [d]
__global__ void ridge_emit_rows_kernel(const double* __restrict__ sol, int k1, int d, int c0, int nb,
                                       float* __restrict__ w, float* __restrict__ bias) {
  const int n = k1 + 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nb * n; i += gridDim.x * blockDim.x) {
    const int q = i / n, r = i % n;
    const float v = (float)sol[i];
    if (r < k1) w[(size_t)r * d + c0 + q] = v;
    else bias[c0 + q] = v;
  }
}

int ridge_solve_wide(td_handle* h, td_stats* s, const double* lambdas_host, int n_lambda, float* w_dev,
                     float* b_dev) {
  int k1 = 0, d = 0;
  int64_t frames = 0;
  td_stats_layout(s, &k1, &d, &frames);
  const int n = k1 + 1;
  const size_t off_xty = (size_t)n * n, off_bt = off_xty + (size_t)n * d, off_z = off_bt + (size_t)64 * n,
               off_sol = off_z + (size_t)64 * n, off_ws = off_sol + (size_t)64 * n;
  void* base = nullptr;
  TD_TRY(td_workspace(h, sizeof(double) * off_ws + td_chol_ws_bytes(n) + 256, &base));
  double* xtx = reinterpret_cast<double*>(base);
  double* xty = xtx + off_xty;
  double* bt = xtx + off_bt;
  double* z = xtx + off_z;
  double* sol = xtx + off_sol;
  void* cws = reinterpret_cast<char*>(base) + td_round_up((int64_t)(sizeof(double) * off_ws), 256);
  TD_TRY(td_stats_moments_ld(h, s, xtx, n, xty, nullptr, nullptr, nullptr));
  const double inv = 1.0 / (double)frames;
  for (int li = 0; li < n_lambda; ++li) {
    float* w_l = w_dev + (size_t)li * k1 * d;
    float* b_l = b_dev + (size_t)li * d;
    for (int c0 = 0; c0 < d; c0 += 64) {
      const int nb = d - c0 < 64 ? d - c0 : 64;
      hipLaunchKernelGGL(xty_rows_kernel, dim3(64), dim3(256), 0, h->stream, xty, n, d, c0, nb, inv, bt);
      td_chol_state st;
      TD_TRY(td_chol_factor(h, cws, xtx, n, bt, nb, &st, lambdas_host[li], inv));
      unpad_rows(h, st.rt, nb, n, st.np, z, 64);
      TD_TRY(td_chol_back(h, &st, z, nb, sol));
      hipLaunchKernelGGL(ridge_emit_rows_kernel, dim3(64), dim3(256), 0, h->stream, sol, k1, d, c0, nb,
                         w_l, b_l);
    }
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

// ---- the batched factorisation's workspace and systems -------------------------------------------------------
// The handle's workspace (grow-only) for `batch` systems from dense moments: [xtx n * np][xty n * d][SolveWs];
// the moments have the padded row stride np (aligned rows: td_stats_moments_ld).
struct RidgeWs {
  double* xtx; double* xty;
  SolveWs w;
};

int ridge_workspace(td_handle* h, int n, int np, int d, int batch, RidgeWs* out) {
  const size_t nn = (size_t)n * np;
  const size_t head = td_round_up((int64_t)(sizeof(double) * (nn + (size_t)n * d)), 256);
  void* base = nullptr;
  TD_TRY(td_workspace(h, head + carve(nullptr, np, batch).bytes, &base));
  out->xtx = reinterpret_cast<double*>(base);
  out->xty = out->xtx + nn;
  out->w = carve(reinterpret_cast<char*>(base) + head, np, batch);
  return TD_OK;
}

// cov = M / frames + lambda I for each lambda (the same xtx for the n_lambda systems: stride 0) and rhs = xty / frames,
// as systems first .. first + n_lambda - 1 of the batch
void pad_ridge_systems(td_handle* h, const RidgeWs& ws, int n, int np, int d, int64_t frames, int n_lambda,
                       size_t first) {
  pad_systems(h, ws.xtx, 0LL, np, n, np, 1.0 / (double)frames, ws.w.lams, ws.w.a + first * np * np, n_lambda,
              ws.xty, 0LL, d, ws.w.rt + first * kMaxRhs * np);
}

// ---- conjugate gradients in front of the factorisation -------------------------------------------------------
// What both attempts of a solve ask of the handle and of the lambdas.
struct CgAsk {
  bool allowed;        // not td_set_solver(TD_SOLVER_CHOLESKY), and every lambda is positive
  bool by_choice;      // td_set_solver(TD_SOLVER_CG): 400 iterations, 10 tol; else automatic -- at most ~3x the
                       // iterations of a well-conditioned system of this kind (C2: 55), the answer's TRUE residual
                       // within 2 tol
  int cus;             // CUs the handle's stream runs on
  int resident_rows;   // td_cg_rows: rows per workgroup of the LDS-resident solve on those CUs, 0 = does not fit
  int max_iter() const { return by_choice ? kCgMaxIter : kCgAutoMaxIter; }
  double accept() const { return by_choice ? 100.0 : 4.0; }
};

// (lambda = 0 leaves a matrix that may be exactly singular -- a duplicated channel -- on which conjugate
// gradients happily converges to SOME solution of the consistent system where np.linalg.solve
// (brain_model.py:477) and the factorisation report "Singular matrix": only lambda > 0 goes that way)
bool all_positive(const double* lambdas_host, int n_lambda) {
  bool positive = true;
  for (int i = 0; i < n_lambda; ++i) positive = positive && lambdas_host[i] > 0.0;
  return positive;
}

// The device block {status, iterations} a conjugate-gradient launch reports in: allocated when an attempt is about
// to be made ...
int cg_status_block(td_handle* h) {
  if (!h->cg_status) TD_HIP(h, hipMalloc(reinterpret_cast<void**>(&h->cg_status), sizeof(int) * 16));
  return TD_OK;
}

// ... and read back behind it (waits for the stream) into the handle's report.  Anything but "converged, true
// residual checked" leaves the solve to the factorisation.
int cg_status_read(td_handle* h, bool* converged) {
  int st[2] = {0, 0};
  TD_HIP(h, hipMemcpyAsync(st, h->cg_status, sizeof(int) * 2, hipMemcpyDeviceToHost, h->stream));
  TD_HIP(h, hipStreamSynchronize(h->stream));
  h->last_iterations = st[1]; h->last_cg_status = st[0];
  *converged = st[0] == 0;
  if (*converged) h->last_solver = TD_SOLVER_CG;
  return TD_OK;
}

// Conjugate gradients on the COMPACT statistics (cg.hip: one workgroup per channel, no dense matrix,
// no expansion): the route of a handle whose CUs cannot hold the dense matrix in LDS (the solve
// partition of a pipelined fit) and of asynchronous solves that asked for it (td_set_option
// "async_cg"): an asynchronous caller finds 2 in its flag when the solver gave up (not converged,
// ill-conditioned for the promise, aborted) and solves again with the factorisation.
// *done: nothing is left to do -- converged, or queued for an asynchronous caller, whom nothing waits for (the flag
// says how it went).
int try_compact_cg(td_handle* h, td_stats* s, const CgAsk& ask, int n, int d, const double* lams_dev,
                   const double* lambdas_host, int n_lambda, float* w_dev, float* b_dev, int* flag_dev, bool* done) {
  *done = false;
  const bool want = ask.allowed && n_lambda * d <= kCgAutoSystems &&
                    (flag_dev ? h->async_cg != 0 : (ask.resident_rows == 0 && n >= kCgAutoMinN1));
  StatsCompact sc;
  sc.ok = false;
  if (want) TD_TRY(td_stats_compact(s, &sc));
  if (!want || !sc.ok) return TD_OK;
  TD_TRY(cg_status_block(h));
  const int rc = td_cg_solve_compact(h, sc, lams_dev, lambdas_host, n_lambda, ask.max_iter(), kCgTol, ask.accept(),
                                     w_dev, b_dev, h->cg_status, flag_dev);
  if (rc == TD_CG_NOT_RESIDENT) return TD_OK;
  if (rc != TD_OK) return rc;
  if (flag_dev) {
    h->last_solver = TD_SOLVER_CG;
    *done = true;
    return TD_OK;
  }
  return cg_status_read(h, done);
}

// A few large systems, synchronous caller, the whole matrix fits the LDS of the CUs this handle runs
// on: conjugate gradients in ONE launch (cg.hip) instead of the ~100 launches of the factorisation.
// The AUTOMATIC route answers for np.linalg.solve (brain_model.py:477), so it is taken only where a
// residual bound is a weight bound: a true relative residual of 2e-12 leaves the weights within
// cond(A) x 2e-12 of the factorisation's, and cond(A) <= trace(cov) / lambda + 1 -- with
// lambda >= 1e-6 trace(cov) that is 2e-6, inside the 1e-5 the fit promises.  The kernel sums the trace
// itself (one exchange in front of the first system) and reports status 4 for a smaller lambda (low-pass
// EEG with a tiny ridge): the factorisation follows; td_set_solver(TD_SOLVER_CG) remains the explicit choice.
int try_dense_cg(td_handle* h, const CgAsk& ask, const RidgeWs& ws, int n, int np, int d, double inv, int n_lambda,
                 float* w_dev, float* b_dev, int* flag_dev, bool* done) {
  *done = false;
  const int systems = n_lambda * d;
  const bool cg_auto = systems <= kCgAutoSystems &&
                       n >= (systems == 1 ? kCgAutoMinN1 : systems == 2 ? kCgAutoMinN2 : kCgAutoMinN4);
  if (flag_dev || !ask.allowed || !(cg_auto || ask.by_choice) || n < 3 || ask.resident_rows <= 0) return TD_OK;
  TD_TRY(cg_status_block(h));
  const int rc = td_cg_solve_dense(h, ws.xtx, n, np, ws.xty, d, inv, ws.w.lams, n_lambda, ask.cus, ask.max_iter(),
                                   kCgTol, w_dev, b_dev, h->cg_status, ask.accept(), !ask.by_choice);
  if (rc == TD_CG_NOT_RESIDENT) {
    h->last_cg_status = 3;
    return TD_OK;
  }
  if (rc != TD_OK) return rc;
  return cg_status_read(h, done);
}

// flag_dev == NULL: synchronous (the status reports a singular system); else the caller's device
// int receives 0 / 1 in stream order and nothing waits for the device.
int ridge_solve_impl(td_handle* h, td_stats* s, const double* lambdas_host, int n_lambda, float* w_dev,
                     float* b_dev, int* flag_dev) {
  if (!h || !s || !lambdas_host || !w_dev || !b_dev)
    return td_fail(h, TD_ERR_INVALID, "td_ridge_solve: NULL argument");
  // the handle's report of this solve, reset in front of every branch (td_last_solve_info must not report the
  // PREVIOUS solve after a wide one)
  h->last_cg_kernel = TD_CG_KERNEL_NONE; h->last_cg_param = 0; h->last_cg_wgs = 0;
  h->last_solver = TD_SOLVER_CHOLESKY; h->last_iterations = 0; h->last_cg_status = 0;
  int k1 = 0, d = 0;
  int64_t frames = 0;
  td_stats_layout(s, &k1, &d, &frames);
  TD_REQUIRE(h, n_lambda > 0, "td_ridge_solve: need at least one lambda");
  TD_REQUIRE(h, d > 0, "td_ridge_solve: statistics were created without a target (d = 0)");
  if (frames <= 0) return td_fail(h, TD_ERR_STATE, "td_ridge_solve: no data accumulated");
  TD_TRY(td_stats_settle(h, s));          // (a finalize launch left pending: TD_ACC_DEFER)
  if (d > kMaxRhs) {
    // wide targets: synchronous; an asynchronous caller gets its flag written behind the solve
    const int rc = ridge_solve_wide(h, s, lambdas_host, n_lambda, w_dev, b_dev);
    if (!flag_dev || (rc != TD_OK && rc != TD_ERR_SINGULAR)) return rc;
    const int flag = rc == TD_ERR_SINGULAR ? 1 : 0;
    return td_upload_async(h, &flag, sizeof(int), flag_dev);
  }
  const int n = k1 + 1;
  const int np = (int)td_round_up(n, NB);
  RidgeWs ws;
  TD_TRY(ridge_workspace(h, n, np, d, n_lambda, &ws));
  TD_TRY(td_upload_async(h, lambdas_host, sizeof(double) * n_lambda, ws.w.lams));
  CgAsk ask;
  ask.allowed = h->solver_mode != TD_SOLVER_CHOLESKY && all_positive(lambdas_host, n_lambda);
  ask.by_choice = h->solver_mode == TD_SOLVER_CG;
  ask.cus = h->cu_count > 0 ? h->cu_count : 256;
  ask.resident_rows = td_cg_rows(n - 1, ask.cus);
  bool done = false;
  // (the compact attempt needs no dense moments: it comes before their expansion)
  TD_TRY(try_compact_cg(h, s, ask, n, d, ws.w.lams, lambdas_host, n_lambda, w_dev, b_dev, flag_dev, &done));
  if (done) return TD_OK;
  TD_TRY(td_stats_moments_ld(h, s, ws.xtx, np, ws.xty, nullptr, nullptr, nullptr));
  TD_TRY(try_dense_cg(h, ask, ws, n, np, d, 1.0 / (double)frames, n_lambda, w_dev, b_dev, flag_dev, &done));
  if (done) return TD_OK;
  // the factorisation, which also owns the "Singular matrix" report
  pad_ridge_systems(h, ws, n, np, d, frames, n_lambda, 0);
  TD_TRY(spd_solve_padded(h, ws.w.a, ws.w.rt, ws.w.sol, ws.w.linv, ws.w.tol, np, n, d, n_lambda, flag_dev));
  hipLaunchKernelGGL(ridge_emit_kernel, dim3(256), dim3(256), 0, h->stream, ws.w.sol, k1, d, np,
                     n_lambda, w_dev, b_dev);
  TD_HIP(h, hipGetLastError());
  return flag_dev ? TD_OK : spd_check_flag(h);
}

}  // namespace

int stats_layouts_agree(td_handle* h, td_stats* const* stats, int count, int k1, int d, const char* who,
                        const char* empty, int64_t* frames_out) {
  for (int i = 0; i < count; ++i) {
    int ki = 0, di = 0;
    int64_t fi = 0;
    TD_REQUIRE(h, stats[i], "%s: NULL statistics", who);
    td_stats_layout(stats[i], &ki, &di, &fi);
    TD_REQUIRE(h, ki == k1 && di == d, "%s: layouts differ", who);
    if (empty && fi <= 0) return td_fail(h, TD_ERR_STATE, "%s", empty);
    if (frames_out) frames_out[i] = fi;
  }
  return TD_OK;
}

extern "C" {

int td_ridge_solve(td_handle* h, td_stats* s, const double* lambdas_host, int n_lambda,
                   float* w_dev, float* b_dev) {
  return ridge_solve_impl(h, s, lambdas_host, n_lambda, w_dev, b_dev, nullptr);
}

// Several statistics x several lambdas in ONE batched factorisation (the folds of a
// leave-one-out sweep, regression.py:151-242): the blocked Cholesky is a chain of ~100 small
// launches per solve whose late block steps cannot fill the chip with 20 systems; with
// n_stats * n_lambda systems per launch the same chain serves them all.
int td_ridge_solve_multi(td_handle* h, td_stats* const* stats, int n_stats,
                         const double* lambdas_host, int n_lambda, float* w_dev, float* b_dev,
                         const int** singular_flag_host) {
  if (!h || !stats || !lambdas_host || !w_dev || !b_dev)
    return td_fail(h, TD_ERR_INVALID, "td_ridge_solve_multi: NULL argument");
  TD_REQUIRE(h, n_stats > 0 && n_lambda > 0, "td_ridge_solve_multi: empty batch");
  int k1 = 0, d = 0;
  int64_t frames0 = 0;
  td_stats_layout(stats[0], &k1, &d, &frames0);
  TD_REQUIRE(h, d > 0, "td_ridge_solve_multi: statistics were created without a target (d = 0)");
  std::vector<int64_t> frames((size_t)n_stats);
  TD_TRY(stats_layouts_agree(h, stats, n_stats, k1, d, "td_ridge_solve_multi",
                             "td_ridge_solve_multi: no data accumulated", frames.data()));
  if (d > kMaxRhs) {
    // wide targets: one statistics object at a time (ridge_solve_wide), synchronous
    int singular = 0;
    for (int i = 0; i < n_stats; ++i) {
      const int rc = ridge_solve_wide(h, stats[i], lambdas_host, n_lambda,
                                      w_dev + (size_t)i * n_lambda * k1 * d, b_dev + (size_t)i * n_lambda * d);
      if (rc == TD_ERR_SINGULAR) singular = 1;
      else if (rc != TD_OK) return rc;
    }
    if (!singular_flag_host)
      return singular ? td_fail(h, TD_ERR_SINGULAR, "Singular matrix: covariance is not positive definite")
                      : TD_OK;
    int slot = 0;
    TD_TRY(async_slot_acquire(h, &slot));
    h->host_flags[slot] = singular;       // (everything above has finished: the solves are synchronous)
    TD_TRY(async_slot_publish(h, slot, false));
    *singular_flag_host = h->host_flags + slot;
    return TD_OK;
  }
  const int n = k1 + 1;
  const int np = (int)td_round_up(n, NB);
  const int batch = n_stats * n_lambda;
  RidgeWs ws;
  TD_TRY(ridge_workspace(h, n, np, d, batch, &ws));
  TD_TRY(td_upload_async(h, lambdas_host, sizeof(double) * n_lambda, ws.w.lams));
  for (int i = 0; i < n_stats; ++i) {
    TD_TRY(td_stats_moments_ld(h, stats[i], ws.xtx, np, ws.xty, nullptr, nullptr, nullptr));
    pad_ridge_systems(h, ws, n, np, d, frames[i], n_lambda, (size_t)i * n_lambda);
  }
  int* flag_dev = nullptr;
  int slot = 0;
  if (singular_flag_host) {
    *singular_flag_host = nullptr;
    TD_TRY(async_slot_acquire(h, &slot));
    flag_dev = h->dev_flags + slot;
  }
  TD_TRY(spd_solve_padded(h, ws.w.a, ws.w.rt, ws.w.sol, ws.w.linv, ws.w.tol, np, n, d, batch, flag_dev));
  hipLaunchKernelGGL(ridge_emit_kernel, dim3(256), dim3(256), 0, h->stream, ws.w.sol, k1, d, np, batch,
                     w_dev, b_dev);
  TD_HIP(h, hipGetLastError());
  if (!singular_flag_host) return spd_check_flag(h);
  TD_TRY(async_slot_publish(h, slot, true));
  *singular_flag_host = h->host_flags + slot;
  return TD_OK;
}

int td_ridge_solve_async(td_handle* h, td_stats* s, const double* lambdas_host, int n_lambda,
                         float* w_dev, float* b_dev, const int** singular_flag_host) {
  if (!h || !singular_flag_host)
    return td_fail(h, TD_ERR_INVALID, "td_ridge_solve_async: NULL argument");
  *singular_flag_host = nullptr;
  int slot = 0;
  TD_TRY(async_slot_acquire(h, &slot));
  TD_TRY(ridge_solve_impl(h, s, lambdas_host, n_lambda, w_dev, b_dev, h->dev_flags + slot));
  TD_TRY(async_slot_publish(h, slot, true));
  *singular_flag_host = h->host_flags + slot;
  return TD_OK;
}

}  // extern "C"
