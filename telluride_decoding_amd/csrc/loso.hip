// A3 -- the leave-one-out sweep of the ridge solve: every (fold, lambda) system by conjugate gradients,
// preconditioned with the factorisation of chol.hip, which also applies it (td_ridge_solve_loso,
// td_ridge_solve_loso_terms).
#include "solve_common.h"

namespace {

using namespace td_tile64;   // NB

// ---- the (fold x lambda) systems of a leave-one-out sweep by preconditioned CG ------------------
// regression.jackknife_over_regularizations (regression.py:326-420) solves F x Lambda ridge
// systems whose matrices differ little: fold f's is A_f + lambda I with A_f = M_f / n_f, M_f the
// moments of all recordings but one -- within 1 / F of P = M_total / N.  So ONE Cholesky factor
// per lambda, of P + lambda I (Lambda factorisations instead of F x Lambda), preconditions a
// conjugate-gradient solve of every fold's system with that lambda: the preconditioned spectrum
// sits in a narrow band below 1 + 1 / (F - 1) when the recordings are alike, and CG reaches
// float64 accuracy in a handful of iterations.  An iteration is
//   q = A_f p        one pass over the F dense matrices (a [Lambda d x n] x [n x n] product per fold
//                    on the float64 MFMA: every matrix byte read once for all lambdas),
//   z = (P + lambda I)^-1 r   two blocked triangular substitutions with F d right-hand sides each,
//   a few row-wise dot products / axpys.
// At C5 (32 folds x 20 lambdas, n = 2049): 20 factorisations + ~10 iterations instead of 640
// factorisations.  Convergence is checked (relative residual of every system); the caller
// falls back to the direct batched solve if it is not reached.
//
// Vectors are ROWS of np doubles in the order [lambda][output q][fold]: the rows of a lambda are
// contiguous (the triangular solves), the rows of a fold a constant stride apart (the products).
//
// The product (loso_matvec_kernel) and the substitutions (loso_binv_kernel, loso_big_solve_kernel,
// loso_big_update_kernel) are in chol.hip, which says why; here are the row-wise kernels and the host.

// Row-wise pieces of the CG iteration.  One workgroup per row.
//   stage 0 (start):  x = 0 ; r = b ; bb = b . b
//   stage 1:          rz = r . z ; p = z                        (first direction)
//   stage 2:          alpha = rz / (p . q) ; x += alpha p ; r -= alpha q
//   stage 3:          rz' = r . z ; beta = rz' / rz ; p = z + beta p ; rz = rz'
//   stage 4 (end):    flag |= (r . r > tol^2 bb)
struct LosoVec {
  double *x, *r, *z, *p, *q;
  const double* b;
  double *rz, *bb;
  int np, stage;
  double tol2;
  int* flag;
};

__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(256) void loso_vec_kernel(LosoVec v) {
  __shared__ double red[256];
  const long long row = blockIdx.x;
  const long long o = row * v.np;
  const int tid = threadIdx.x;
  if (v.stage == 0) {
    double s = 0.0;
    for (int i = tid; i < v.np; i += 256) {
      const double bi = v.b[o + i];
      v.x[o + i] = 0.0; v.r[o + i] = bi; s += bi * bi;
    }
    s = block_sum(s, red);
    if (tid == 0) v.bb[row] = s;
  } else if (v.stage == 1) {
    double s = 0.0;
    for (int i = tid; i < v.np; i += 256) { const double zi = v.z[o + i]; s += v.r[o + i] * zi; v.p[o + i] = zi; }
    s = block_sum(s, red);
    if (tid == 0) v.rz[row] = s;
  } else if (v.stage == 2) {
    double s = 0.0;
    for (int i = tid; i < v.np; i += 256) s += v.p[o + i] * v.q[o + i];
    s = block_sum(s, red);
    // (a converged or empty system: p . q = 0 -> leave it alone)
    const double alpha = s > 0.0 ? v.rz[row] / s : 0.0;
    for (int i = tid; i < v.np; i += 256) { v.x[o + i] += alpha * v.p[o + i]; v.r[o + i] -= alpha * v.q[o + i]; }
  } else if (v.stage == 3) {
    double s = 0.0;
    for (int i = tid; i < v.np; i += 256) s += v.r[o + i] * v.z[o + i];
    s = block_sum(s, red);
    const double old = v.rz[row];
    const double beta = old > 0.0 ? s / old : 0.0;
    for (int i = tid; i < v.np; i += 256) v.p[o + i] = v.z[o + i] + beta * v.p[o + i];
    __syncthreads();
    if (tid == 0) v.rz[row] = s;
  } else {
    double s = 0.0;
    for (int i = tid; i < v.np; i += 256) s += v.r[o + i] * v.r[o + i];
    s = block_sum(s, red);
    if (tid == 0 && !(s <= v.tol2 * v.bb[row])) atomicExch(v.flag, 1);
  }
}

// b rows [lambda][q][fold][np] = xty_f[:, q] / n_f (the same for every lambda), zero padded
__global__ void loso_rhs_kernel(const double* __restrict__ xty, const double* __restrict__ inv_n, int n,
                                int d, int np, int folds, int n_lambda, double* __restrict__ b) {
  const long long total = (long long)n_lambda * d * folds * np;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % np);
    const long long row = i / np;
    const int f = (int)(row % folds);
    const int q = (int)((row / folds) % d);
    b[i] = c < n ? xty[((size_t)f * n + c) * d + q] * inv_n[f] : 0.0;
  }
}

// w [fold][lambda][k1][d], bias [fold][lambda][d] (float32) from the solution rows
// (k_major: w [fold][k1][lambda][d] -- the models of a fold as the OUTPUT COLUMNS of one filter, what
//  td_predict_fir_per_file takes)
__global__ void loso_emit_kernel(const double* __restrict__ x, int k1, int d, int np, int folds,
                                 int n_lambda, float* __restrict__ w, float* __restrict__ bias, int k_major) {
  const long long total = (long long)folds * n_lambda * (k1 + 1) * d;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(i % d);
    const int r = (int)((i / d) % (k1 + 1));
    const int lam = (int)((i / ((long long)d * (k1 + 1))) % n_lambda);
    const int f = (int)(i / ((long long)d * (k1 + 1) * n_lambda));
    const float v = (float)x[(((long long)lam * d + q) * folds + f) * np + r];
    const long long sys = (long long)f * n_lambda + lam;
    if (r < k1) w[k_major ? (((size_t)f * k1 + r) * n_lambda + lam) * d + q : ((size_t)sys * k1 + r) * d + q] = v;
    else bias[(size_t)sys * d + q] = v;
  }
}

// ---- the host side, step by step ---------------------------------------------------------------------------
// The sizes of a sweep.
struct LosoDims {
  int k1, d, n, np, nblk, nbig;      // unknowns n = k1 + 1, padded np = nblk 64-blocks = nbig steps of kBig of them
  int n_folds, n_lambda, rows_per_lambda;
  long long rows;                    // n_lambda * d * n_folds vectors
  size_t nn;                         // a fold's dense moments: n rows with the padded stride (td_stats_moments_ld)
};

LosoDims loso_dims(int k1, int d, int n_folds, int n_lambda) {
  LosoDims s;
  s.k1 = k1; s.d = d; s.n = k1 + 1; s.np = (int)td_round_up(s.n, NB); s.nblk = s.np / NB;
  s.nbig = (int)td_ceil_div(s.nblk, kBig);
  s.n_folds = n_folds; s.n_lambda = n_lambda; s.rows_per_lambda = d * n_folds;
  s.rows = (long long)n_lambda * d * n_folds;
  s.nn = (size_t)s.n * s.np;
  return s;
}

// workspace layout of a sweep: every piece rounded up to 256 bytes
struct LosoWs {
  double *af, *xty, *mt, *invn, *lams;       // the folds' moments and right-hand sides, the total's, 1 / frames, lambdas
  double *pa, *linv, *tolv, *rt, *sol;       // the preconditioners' systems as chol_factor_forward takes them
  double *x, *r, *z, *p, *q, *b, *v, *y, *spare;   // the vectors, `rows` rows of np each
  double *rz, *bb;                           // per row
  double* xinv;                              // the inverses of the 256-blocks
  size_t bytes;
};

LosoWs carve(void* base, const LosoDims& s) {
  LosoWs w;
  char* p = reinterpret_cast<char*>(base);
  auto take = [&](size_t count) {
    double* q = reinterpret_cast<double*>(p);
    p += td_round_up((int64_t)(sizeof(double) * count), 256);
    return q;
  };
  w.af = take(s.nn * s.n_folds); w.xty = take((size_t)s.n * s.d * s.n_folds); w.mt = take(s.nn);
  w.invn = take(s.n_folds); w.lams = take(s.n_lambda);
  w.pa = take((size_t)s.n_lambda * s.np * s.np); w.linv = take((size_t)s.n_lambda * s.nblk * NB * NB);
  w.tolv = take(td_round_up(s.n_lambda, 32)); w.rt = take((size_t)s.n_lambda * kMaxRhs * s.np);
  w.sol = take((size_t)s.n_lambda * kMaxRhs * s.np);
  for (double** vec : {&w.x, &w.r, &w.z, &w.p, &w.q, &w.b, &w.v, &w.y, &w.spare}) *vec = take((size_t)s.rows * s.np);
  w.rz = take(s.rows); w.bb = take(s.rows);
  w.xinv = take((size_t)s.n_lambda * s.nbig * 16 * NB * NB);
  w.bytes = (size_t)(p - reinterpret_cast<char*>(base));
  return w;
}

// Fold counts and validation: inv_n[f] = 1 / frames of fold f.  folds != NULL: the folds' training statistics;
// else fold f = total + sum of signs[t] * terms[t] over t in [term_begin[f], term_begin[f + 1]).
int loso_inv_frames(td_handle* h, td_stats* const* folds, td_stats* const* terms, const int* term_begin,
                    const double* signs, int n_folds, int k1, int d, int64_t frames_total,
                    std::vector<double>* inv_n) {
  inv_n->resize((size_t)n_folds);
  if (folds) {
    std::vector<int64_t> frames((size_t)n_folds);
    TD_TRY(stats_layouts_agree(h, folds, n_folds, k1, d, "td_ridge_solve_loso",
                               "td_ridge_solve_loso: a fold has no data", frames.data()));
    for (int f = 0; f < n_folds; ++f) (*inv_n)[f] = 1.0 / (double)frames[f];
    return TD_OK;
  }
  for (int f = 0; f < n_folds; ++f) {
    double frames = (double)frames_total;
    TD_REQUIRE(h, term_begin[f + 1] >= term_begin[f], "td_ridge_solve_loso_terms: term_begin must not decrease");
    for (int t = term_begin[f]; t < term_begin[f + 1]; ++t) {
      int64_t ft = 0;
      TD_TRY(stats_layouts_agree(h, terms + t, 1, k1, d, "td_ridge_solve_loso_terms", nullptr, &ft));
      TD_REQUIRE(h, signs[t] == 1.0 || signs[t] == -1.0, "td_ridge_solve_loso_terms: a sign is +1 or -1");
      frames += signs[t] * (double)ft;
    }
    const int64_t ff = (int64_t)frames;
    if (ff <= 0) return td_fail(h, TD_ERR_STATE, "td_ridge_solve_loso: a fold has no data");
    (*inv_n)[f] = 1.0 / (double)ff;
  }
  return TD_OK;
}

// The preconditioners: Cholesky factors of M_total / N + lambda I (no right-hand sides: one zero row rides
// along) and the inverses of their 256-blocks.  Leaves the total's dense moments in w.mt.
int loso_preconditioner(td_handle* h, td_stats* total, int64_t frames_total, const LosoDims& s, const LosoWs& w) {
  TD_TRY(td_stats_moments_ld(h, total, w.mt, s.np, nullptr, nullptr, nullptr, nullptr));
  pad_systems(h, w.mt, 0LL, s.np, s.n, s.np, 1.0 / (double)frames_total, w.lams, w.pa, s.n_lambda);
  TD_HIP(h, hipMemsetAsync(w.rt, 0, sizeof(double) * (size_t)s.n_lambda * kMaxRhs * s.np, h->stream));
  TD_TRY(chol_factor_forward(h, w.pa, w.rt, w.sol, w.linv, w.tolv, s.np, 1, s.n_lambda, nullptr, kMaxRhs, s.n));
  chol_big_inverses(h, w.pa, w.linv, w.xinv, s.np, s.n_lambda);
  return TD_OK;
}

// The folds' dense moments and the right-hand-side rows b.
int loso_fold_systems(td_handle* h, td_stats* total, td_stats* const* folds, td_stats* const* terms,
                      const int* term_begin, const double* signs, const LosoDims& s, const LosoWs& w) {
  if (folds) {
    for (int f = 0; f < s.n_folds; ++f)
      TD_TRY(td_stats_moments_ld(h, folds[f], w.af + (size_t)f * s.nn, s.np, w.xty + (size_t)f * s.n * s.d, nullptr,
                                 nullptr, nullptr));
  } else {
    // ONE launch for every fold: the total's dense matrix (w.mt, the preconditioner's) plus the folds' few signed terms
    TD_TRY(td_stats_loso_moments(h, total, terms, term_begin, signs, s.n_folds, w.mt, s.np, w.af, w.xty));
  }
  hipLaunchKernelGGL(loso_rhs_kernel, dim3(1024), dim3(256), 0, h->stream, w.xty, w.invn, s.n, s.d, s.np, s.n_folds,
                     s.n_lambda, w.b);
  return TD_OK;
}

// z = (P + lambda I)^-1 r with the factors (chol.hip: v = r in, y between the two directions)
int loso_precondition(td_handle* h, const LosoDims& s, const LosoWs& w) {
  TD_HIP(h, hipMemcpyAsync(w.v, w.r, sizeof(double) * (size_t)s.rows * s.np, hipMemcpyDeviceToDevice, h->stream));
  chol_big_substitute(h, w.pa, w.xinv, s.np, s.n_lambda, s.rows_per_lambda, w.v, w.y, w.z);
  return TD_OK;
}

// The iteration.  *flag: 0 every system reached tol, 1 not within max_iter, 2 the preconditioner's factorisation
// failed; *iterations: how many were run.
// Convergence is looked at after iteration 3 and after every later one (a device-to-host read
// of one int: ~30 us against the ~1.9 ms of an iteration at C5, where systems alike enough
// for this solver are done in 4 to 6).
int loso_iterate(td_handle* h, const LosoDims& s, const LosoWs& w, int max_iter, double tol, int* iterations,
                 int* flag_out) {
  LosoVec lv;
  lv.x = w.x; lv.r = w.r; lv.z = w.z; lv.p = w.p; lv.q = w.q; lv.b = w.b; lv.rz = w.rz; lv.bb = w.bb; lv.np = s.np;
  lv.tol2 = tol * tol; lv.flag = h->dev_flag;
  auto vec_stage = [&](int stage) {
    lv.stage = stage;
    hipLaunchKernelGGL(loso_vec_kernel, dim3((unsigned)s.rows), dim3(256), 0, h->stream, lv);
  };
  vec_stage(0);
  TD_TRY(loso_precondition(h, s, w));
  vec_stage(1);
  int it = 0, flag = 1;
  while (it < max_iter) {
    const int first = 3 < max_iter ? 3 : max_iter;
    const int upto = it < first ? first : it + 1;
    for (; it < upto; ++it) {
      loso_matvec(h, w.af, w.p, w.q, w.invn, w.lams, s.n, s.np, s.n_folds, s.n_lambda, s.d);
      vec_stage(2);
      TD_TRY(loso_precondition(h, s, w));
      vec_stage(3);
    }
    // (the flag also carries "preconditioner not positive definite" from the factorisation)
    int pd_flag = 0;
    TD_HIP(h, hipMemcpyAsync(&pd_flag, h->dev_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    TD_HIP(h, hipStreamSynchronize(h->stream));
    if (pd_flag) { flag = 2; break; }          // 2: the preconditioner's factorisation failed
    vec_stage(4);
    TD_HIP(h, hipMemcpyAsync(&flag, h->dev_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    TD_HIP(h, hipStreamSynchronize(h->stream));
    if (!flag) break;
    if (it < max_iter) TD_HIP(h, hipMemsetAsync(h->dev_flag, 0, sizeof(int), h->stream));
  }
  *iterations = it;
  *flag_out = flag;
  return TD_OK;
}

// The (fold x lambda) systems of a leave-one-out sweep by preconditioned conjugate gradients
// (kernels and rationale above: loso_matvec_kernel).  Synchronous; *status_host = 0 when every
// system reached the relative residual `tol`, 1 when the preconditioner was not positive
// definite or some system did not converge in max_iter iterations (the outputs are then not to
// be used: the caller falls back to td_ridge_solve_multi).
// folds != NULL: the folds' training statistics; else fold f = total + sum of signs[t] * terms[t] over
// t in [term_begin[f], term_begin[f + 1]).
int ridge_solve_loso_impl(td_handle* h, td_stats* total, td_stats* const* folds, td_stats* const* terms,
                          const int* term_begin, const double* signs, int n_folds, const double* lambdas_host,
                          int n_lambda, int max_iter, double tol, float* w_dev, float* b_dev, int* status_host,
                          int* iterations_host, int w_k_major) {
  if (!h || !total || (!folds && !(terms && term_begin && signs)) || !lambdas_host || !w_dev || !b_dev || !status_host)
    return td_fail(h, TD_ERR_INVALID, "td_ridge_solve_loso: NULL argument");
  TD_REQUIRE(h, n_folds > 0 && n_lambda > 0 && max_iter > 0 && tol > 0.0, "td_ridge_solve_loso: bad sizes");
  int k1 = 0, d = 0;
  int64_t frames_total = 0;
  td_stats_layout(total, &k1, &d, &frames_total);
  TD_REQUIRE(h, d > 0 && d <= kMaxRhs, "td_ridge_solve_loso: outputs per solve must be in [1, %d]", kMaxRhs);
  if (frames_total <= 0) return td_fail(h, TD_ERR_STATE, "td_ridge_solve_loso: no data accumulated");
  std::vector<double> inv_n;
  TD_TRY(loso_inv_frames(h, folds, terms, term_begin, signs, n_folds, k1, d, frames_total, &inv_n));
  const LosoDims s = loso_dims(k1, d, n_folds, n_lambda);
  void* base = nullptr;
  TD_TRY(td_workspace(h, carve(nullptr, s).bytes, &base));
  const LosoWs w = carve(base, s);
  TD_TRY(td_upload_async(h, lambdas_host, sizeof(double) * n_lambda, w.lams));
  TD_TRY(td_upload_async(h, inv_n.data(), sizeof(double) * n_folds, w.invn));
  TD_TRY(loso_preconditioner(h, total, frames_total, s, w));
  TD_TRY(loso_fold_systems(h, total, folds, terms, term_begin, signs, s, w));
  int it = 0, flag = 1;
  TD_TRY(loso_iterate(h, s, w, max_iter, tol, &it, &flag));
  hipLaunchKernelGGL(loso_emit_kernel, dim3(1024), dim3(256), 0, h->stream, w.x, k1, d, s.np, n_folds, n_lambda,
                     w_dev, b_dev, w_k_major);
  TD_HIP(h, hipGetLastError());
  *status_host = flag == 2 ? 2 : flag ? 1 : 0;      // 0 converged, 1 not converged in max_iter, 2 not positive definite
  if (iterations_host) *iterations_host = it;
  return TD_OK;
}

}  // namespace

extern "C" {

int td_ridge_solve_loso(td_handle* h, td_stats* total, td_stats* const* folds, int n_folds,
                        const double* lambdas_host, int n_lambda, int max_iter, double tol,
                        float* w_dev, float* b_dev, int* status_host, int* iterations_host) {
  if (!folds) return td_fail(h, TD_ERR_INVALID, "td_ridge_solve_loso: NULL argument");
  return ridge_solve_loso_impl(h, total, folds, nullptr, nullptr, nullptr, n_folds, lambdas_host, n_lambda, max_iter,
                               tol, w_dev, b_dev, status_host, iterations_host, 0);
}

int td_ridge_solve_loso_terms(td_handle* h, td_stats* total, td_stats* const* terms, const int* term_begin,
                              const double* signs, int n_folds, const double* lambdas_host, int n_lambda,
                              int max_iter, double tol, int w_k_major, float* w_dev, float* b_dev,
                              int* status_host, int* iterations_host) {
  if (!terms || !term_begin || !signs) return td_fail(h, TD_ERR_INVALID, "td_ridge_solve_loso_terms: NULL argument");
  return ridge_solve_loso_impl(h, total, nullptr, terms, term_begin, signs, n_folds, lambdas_host, n_lambda, max_iter,
                               tol, w_dev, b_dev, status_host, iterations_host, w_k_major ? 1 : 0);
}

}  // extern "C"

