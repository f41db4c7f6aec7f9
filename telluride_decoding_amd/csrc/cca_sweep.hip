// CCA dense stage of a leave-one-file-out x regularisation sweep (regression.jackknife_over_regularizations
// with model='cca'; reference regression.py:326-420 over cca.calculate_cca_parameters_from_dataset, cca.py:337-367).
//
// Every (fold, lambda) pair is one CCA model.  A fold's training statistics are the total's plus a few signed
// terms (minus the held-out recording, minus / plus the last training recordings when batching drops a remainder),
// so the dense moments of the total and of every DISTINCT term are expanded once and
//   C_xx = S_xx / denom - m_x^T m_x + lambda I,  C_yy likewise,  C_xy = S_xy / denom - m_x^T m_y,  m = sum / frames
// are formed from them per fold.  The reference whitens both sides by eigen-decomposition and takes
// svd(K11 C_xy K22); when no eigenvalue of C_xx is dropped any whitening of the x side gives the same canonical
// directions, so with C_xx = L L^T and W = L^-1 C_xy (the forward substitution that rides along the batched
// float64 factorisation of chol.hip):
//   K   = C_yy^-1/2               (K2 x K2 Jacobi eigen-decomposition, eigenvalues <= eps_eig dropped)
//   B   = K (W^T W) K             (= K C_xy^T C_xx^-1 C_xy K, symmetric K2 x K2) = V diag(sigma^2) V^T
//   e   = sigma (descending),  rot_y = K V[:, :dim],  rot_x = L^-T (W rot_y diag(1 / sigma))
// -- no K1-sized eigen-decomposition, one factorisation per (fold, lambda), a backward substitution with `dim`
// right-hand sides.  Everything K2-sized (K2 <= 64) of one pair lives in the LDS of one workgroup, in float64.
// A pair whose C_xx has no Cholesky factor, whose C_yy loses an eigenvalue or whose sigma_dim <= 1e-6 sigma_1
// gets status 1: the caller refits it the long way.
#include <algorithm>

#include "stats_common.h"
#include "td_common.h"

namespace {

constexpr int NB = 64;
constexpr int LS = 65;              // row stride of the tail's 64 x 64 LDS matrices
constexpr int kMaxTerms = 4;
constexpr int kMaxSweeps = 30;
constexpr double kRotTol = 1e-15;   // as eig.hip: rotate while |a_pq| > kRotTol sqrt|a_pp a_qq|
constexpr int kTailDoubles = 4 * NB * LS + 5 * NB;
constexpr size_t kChunkBytes = (size_t)3 << 29;   // padded systems of one batched factorisation, at most
constexpr int kChunkSystems = 160;                // (as regression.MAX_SYSTEMS_PER_SOLVE)

struct FoldDesc {
  int term[kMaxTerms];        // which expanded moments (0 = the total's)
  double sign[kMaxTerms];
  int n_terms, pad;
  double inv_denom, inv_frames;
};

// the expanded moments of one statistics object: [xtx (k1 + 1)^2 | x2tx2 k2^2 | xtx2 k1 k2 | sum_x2 k2]
struct Moments {
  const double* base;
  long long stride;           // doubles per statistics object
  int k1, k2;
  __device__ __forceinline__ double at(const FoldDesc& d, long long off) const {
    double s = base[off];
    for (int t = 0; t < d.n_terms; ++t) s += d.sign[t] * base[(long long)d.term[t] * stride + off];
    return s;
  }
  __device__ __forceinline__ long long o_s1() const { return (long long)k1 * (k1 + 1); }
  __device__ __forceinline__ long long o_yy() const { return (long long)(k1 + 1) * (k1 + 1); }
  __device__ __forceinline__ long long o_xy() const { return o_yy() + (long long)k2 * k2; }
  __device__ __forceinline__ long long o_s2() const { return o_xy() + (long long)k1 * k2; }
};

// ---- C_xx + lambda I of a chunk of folds, identity padded, into the factorisation's system buffer ----------------
// Workgroup = one 64 x 64 tile on or below the diagonal of one fold: the moments are read once for all lambdas.
__global__ __launch_bounds__(256) void cca_cov_kernel(Moments M, const FoldDesc* __restrict__ folds,
                                                      const double* __restrict__ lams, int n_lambda, int np,
                                                      double* __restrict__ a) {
  __shared__ double mr[NB], mc[NB];
  const int f = blockIdx.y, tid = threadIdx.x, k1 = M.k1, n1 = M.k1 + 1;
  int bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= (int)blockIdx.x) ++bi;
  const int bj = (int)blockIdx.x - bi * (bi + 1) / 2;
  const FoldDesc d = folds[f];
  if (tid < 2 * NB) {
    const int idx = (tid < NB ? bi : bj) * NB + (tid & 63);
    const double m = idx < k1 ? M.at(d, M.o_s1() + idx) * d.inv_frames : 0.0;
    (tid < NB ? mr : mc)[tid & 63] = m;
  }
  __syncthreads();
  const int c = bj * NB + (tid & 63);
  for (int i = 0; i < 16; ++i) {
    const int rl = (tid >> 6) + 4 * i, r = bi * NB + rl;
    const bool in = r < k1 && c < k1;
    double v = 0.0;
    if (in) v = M.at(d, (long long)r * n1 + c) * d.inv_denom - mr[rl] * mc[tid & 63];
    for (int l = 0; l < n_lambda; ++l) {
      double* dst = a + ((size_t)(f * n_lambda + l) * np + r) * np + c;
      *dst = in ? (r == c ? v + lams[l] : v) : (r == c ? 1.0 : 0.0);
    }
  }
}

// ---- C_xy^T as right-hand-side rows (for every lambda of the fold), C_yy, the means -------------------------------
struct RhsParams {
  Moments M;
  const FoldDesc* folds;
  int n_lambda, np, rt_rows, fold0;
  double* rt;        // [folds * n_lambda][rt_rows][np]
  double* cyy;       // [folds][k2][k2] (without lambda)
  double* mx;        // [folds][k1]
  double* my;        // [folds][k2]
  float* mean_x;     // outputs [F][k1], [F][k2]
  float* mean_y;
};

__global__ __launch_bounds__(256) void cca_rhs_kernel(RhsParams P) {
  const int f = blockIdx.y, k1 = P.M.k1, k2 = P.M.k2;
  const FoldDesc d = P.folds[f];
  const int t0 = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  for (int i = t0; i < k2 * P.np; i += step) {
    const int q = i / P.np, r = i % P.np;
    double v = 0.0;
    if (r < k1)
      v = P.M.at(d, P.M.o_xy() + (long long)r * k2 + q) * d.inv_denom -
          (P.M.at(d, P.M.o_s1() + r) * d.inv_frames) * (P.M.at(d, P.M.o_s2() + q) * d.inv_frames);
    for (int l = 0; l < P.n_lambda; ++l) P.rt[((size_t)(f * P.n_lambda + l) * P.rt_rows + q) * P.np + r] = v;
  }
  for (int i = t0; i < k2 * k2; i += step) {
    const int q = i / k2, j = i % k2;
    P.cyy[(size_t)f * k2 * k2 + i] =
        P.M.at(d, P.M.o_yy() + i) * d.inv_denom -
        (P.M.at(d, P.M.o_s2() + q) * d.inv_frames) * (P.M.at(d, P.M.o_s2() + j) * d.inv_frames);
  }
  for (int i = t0; i < k1; i += step) {
    const double m = P.M.at(d, P.M.o_s1() + i) * d.inv_frames;
    P.mx[(size_t)f * k1 + i] = m;
    P.mean_x[(size_t)(P.fold0 + f) * k1 + i] = (float)m;
  }
  for (int i = t0; i < k2; i += step) {
    const double m = P.M.at(d, P.M.o_s2() + i) * d.inv_frames;
    P.my[(size_t)f * k2 + i] = m;
    P.mean_y[(size_t)(P.fold0 + f) * k2 + i] = (float)m;
  }
}

// ---- in-LDS pieces of the tail -------------------------------------------------------------------------------------
// round-robin pairing (as eig.hip): `players` even, round in [0, players - 1), pair k -> p < q
__device__ __forceinline__ void rr_pair(int players, int round, int k, int* p, int* q) {
  const int m = players - 1;
  int a, b;
  if (k == 0) { a = round; b = m; }
  else {
    a = round + k; a = a >= m ? a - m : a;
    b = round + m - k; b = b >= m ? b - m : b;
  }
  *p = a < b ? a : b;
  *q = a < b ? b : a;
}

// Jacobi rotation that annihilates a_pq: t = b / (d + sign(d) hypot(d, b)), d = a_qq - a_pp, b = 2 a_pq
__device__ __forceinline__ bool jacobi_rotation(double app, double aqq, double apq, double* c, double* s) {
  *c = 1.0; *s = 0.0;
  const double mag2 = apq * apq;
  if (!(mag2 > 1e-290 && mag2 > (kRotTol * kRotTol) * fabs(app * aqq))) return false;
  const double d = aqq - app, b = 2.0 * apq;
  const double t = b / (d + copysign(sqrt(d * d + b * b), d));
  const double cc = 1.0 / sqrt(1.0 + t * t);
  *c = cc; *s = t * cc;
  return true;
}

// Cyclic Jacobi of the symmetric S [n][LS] (n <= 64) by one workgroup of 256 threads: S ends diagonal (the
// eigenvalues), V [n][LS] holds the eigenvectors as columns.  cs: 2 x 32 doubles; flag: one int.
__device__ void jacobi_lds(double* S, double* V, double* cs, int* flag, int n, int tid) {
  for (int idx = tid; idx < n * n; idx += 256) V[(idx / n) * LS + idx % n] = (idx / n == idx % n) ? 1.0 : 0.0;
  __syncthreads();
  if (n < 2) return;
  const int players = (n + 1) & ~1, pairs = players >> 1;
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    if (tid == 0) *flag = 0;
    __syncthreads();
    for (int round = 0; round < players - 1; ++round) {
      int p = 0, q = 0;
      bool rotated = false;
      if (tid < pairs) {
        rr_pair(players, round, tid, &p, &q);
        double c = 1.0, s = 0.0;
        if (q < n) rotated = jacobi_rotation(S[p * LS + p], S[q * LS + q], S[p * LS + q], &c, &s);
        if (rotated) *flag = 1;
        cs[2 * tid] = c; cs[2 * tid + 1] = s;
      }
      __syncthreads();
      for (int idx = tid; idx < n * pairs; idx += 256) {       // S <- S R, V <- V R (columns p, q of every row)
        const int k = idx % pairs, i = idx / pairs;
        int pp, qq;
        rr_pair(players, round, k, &pp, &qq);
        const double c = cs[2 * k], s = cs[2 * k + 1];
        if (qq < n && s != 0.0) {
          const double a = S[i * LS + pp], b = S[i * LS + qq];
          S[i * LS + pp] = c * a - s * b; S[i * LS + qq] = s * a + c * b;
          const double va = V[i * LS + pp], vb = V[i * LS + qq];
          V[i * LS + pp] = c * va - s * vb; V[i * LS + qq] = s * va + c * vb;
        }
      }
      __syncthreads();
      for (int idx = tid; idx < n * pairs; idx += 256) {       // S <- R^T S (rows p, q of every column)
        const int k = idx / n, j = idx % n;
        int pp, qq;
        rr_pair(players, round, k, &pp, &qq);
        const double c = cs[2 * k], s = cs[2 * k + 1];
        if (qq < n && s != 0.0) {
          const double a = S[pp * LS + j], b = S[qq * LS + j];
          S[pp * LS + j] = c * a - s * b; S[qq * LS + j] = s * a + c * b;
        }
      }
      __syncthreads();
      if (rotated) { S[p * LS + q] = 0.0; S[q * LS + p] = 0.0; }   // (what the rotation annihilates, exactly)
    }
    __syncthreads();
    const int any = *flag;
    __syncthreads();
    if (!any) break;
  }
}

// out [n][LS] = a b (tb = false) or a b^T (tb = true), all n x n in LDS
__device__ __forceinline__ void mm_lds(double* out, const double* a, const double* b, int n, bool tb, int tid) {
  for (int idx = tid; idx < n * n; idx += 256) {
    const int i = idx / n, j = idx % n;
    double s = 0.0;
    if (tb) for (int m = 0; m < n; ++m) s += a[i * LS + m] * b[j * LS + m];
    else    for (int m = 0; m < n; ++m) s += a[i * LS + m] * b[m * LS + j];
    out[i * LS + j] = s;
  }
}

struct TailParams {
  int k1, k2, np, rt_rows, ut_rows, n_lambda, dim, fold0;
  double eps;
  const double* lams;
  const double* a;        // [batch][np][np]: L (lower triangle)
  const double* tol;      // [batch]
  const double* rt;       // [batch][rt_rows][np]: W^T = (L^-1 C_xy)^T
  const double* cyy;      // [folds][k2][k2]
  const double* my;       // [folds][k2]
  double* ut;             // [batch][ut_rows][np]: (W rot_y / sigma)^T, the right-hand sides of the backward pass
  float* rot_y;           // [F][k2][n_lambda * dim]
  float* bias_y;          // [F][n_lambda * dim]
  float* e;               // [F][n_lambda][dim]
  int* status;            // [F][n_lambda]
};

// One workgroup per (fold, lambda); consecutive workgroups share a fold's C_yy.
__global__ __launch_bounds__(256) void cca_tail_kernel(TailParams P) {
  extern __shared__ double lds[];
  double* A = lds;                 // C_yy -> M -> B
  double* Bm = A + NB * LS;        // eigenvectors
  double* Cm = Bm + NB * LS;       // scratch / staging
  double* Dm = Cm + NB * LS;       // K = C_yy^-1/2
  double* vals = Dm + NB * LS;     // [64]
  double* cs = vals + NB;          // [64]
  double* sig = cs + NB;           // [64] sorted sigma
  double* red = sig + NB;          // [64]
  int* order = reinterpret_cast<int*>(red + NB);   // [64] + flag + bad  (128 ints of room)
  int* flag = order + NB;
  int* bad = flag + 1;
  const int tid = threadIdx.x, sys = blockIdx.x, f = sys / P.n_lambda, l = sys % P.n_lambda;
  const int k1 = P.k1, k2 = P.k2, np = P.np, dim = P.dim;
  const double lam = P.lams[l];
  if (tid == 0) *bad = 0;
  if (tid < NB) { order[tid] = 0; sig[tid] = 0.0; }
  // 1. K = C_yy^-1/2
  for (int idx = tid; idx < k2 * k2; idx += 256) {
    const int i = idx / k2, j = idx % k2;
    A[i * LS + j] = P.cyy[(size_t)f * k2 * k2 + idx] + (i == j ? lam : 0.0);
  }
  __syncthreads();
  jacobi_lds(A, Bm, cs, flag, k2, tid);
  if (tid < k2) {
    const double v = A[tid * LS + tid];
    const bool keep = v > P.eps;
    if (!keep) *bad = 1;                                  // (NaN too)
    vals[tid] = keep ? 1.0 / sqrt(sqrt(v)) : 0.0;
  }
  __syncthreads();
  for (int idx = tid; idx < k2 * k2; idx += 256) {
    const int i = idx / k2, j = idx % k2;
    Cm[i * LS + j] = Bm[i * LS + j] * vals[j];
  }
  __syncthreads();
  mm_lds(Dm, Cm, Cm, k2, true, tid);
  // the smallest pivot of this system's factorisation: L_ii^2 against the tolerance the factorisation used
  {
    const double* ab = P.a + (size_t)sys * np * np;
    double pm = 1e300;
    for (int i = tid; i < k1; i += 256) {
      const double lii = ab[(size_t)i * np + i];
      pm = lii > 0.0 ? fmin(pm, lii * lii) : -1.0;        // (a NaN pivot is not positive either)
      if (!(lii > 0.0)) break;
    }
    for (int off = 32; off > 0; off >>= 1) pm = fmin(pm, __shfl_xor(pm, off));
    if ((tid & 63) == 0) red[tid >> 6] = pm;
  }
  __syncthreads();
  if (tid == 0) {
    const double pm = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    if (!(pm > P.tol[sys])) *bad = 1;
  }
  // 2. M = W^T W: the rows of rt (q < k2), 64 columns at a time through Cm; thread (ti, tj) owns M[ti + 16 a][tj + 16 b]
  const double* w = P.rt + (size_t)sys * P.rt_rows * np;
  const int ti = tid >> 4, tj = tid & 15;
  double acc[4][4];
  for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  for (int c0 = 0; c0 < np; c0 += NB) {
    __syncthreads();
    for (int idx = tid; idx < NB * NB; idx += 256) {
      const int q = idx >> 6, c = idx & 63;
      Cm[q * LS + c] = (q < k2 && c0 + c < k1) ? w[(size_t)q * np + c0 + c] : 0.0;
    }
    __syncthreads();
    for (int c = 0; c < NB; ++c) {
      double x[4], y[4];
      for (int a = 0; a < 4; ++a) { x[a] = Cm[(ti + 16 * a) * LS + c]; y[a] = Cm[(tj + 16 * a) * LS + c]; }
      for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) acc[a][b] += x[a] * y[b];
    }
  }
  __syncthreads();
  for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) A[(ti + 16 * a) * LS + tj + 16 * b] = acc[a][b];
  __syncthreads();
  // 3. B = K M K, symmetrised
  mm_lds(Cm, A, Dm, k2, false, tid);
  __syncthreads();
  mm_lds(Bm, Dm, Cm, k2, false, tid);
  __syncthreads();
  for (int idx = tid; idx < k2 * k2; idx += 256) {
    const int i = idx / k2, j = idx % k2;
    A[i * LS + j] = 0.5 * (Bm[i * LS + j] + Bm[j * LS + i]);
  }
  __syncthreads();
  // 4. B = V diag(sigma^2) V^T
  jacobi_lds(A, Bm, cs, flag, k2, tid);
  if (tid < k2) vals[tid] = A[tid * LS + tid];
  __syncthreads();
  // 5. the `dim` largest, descending (ties: the lower index first)
  if (tid < k2) {
    const double v = vals[tid];
    int rank = 0;
    for (int j = 0; j < k2; ++j) rank += (vals[j] > v || (vals[j] == v && j < tid)) ? 1 : 0;
    if (!(v == v)) { rank = k2 - 1; *bad = 1; }
    if (rank < dim) { order[rank] = tid; sig[rank] = sqrt(fmax(v, 0.0)); }
  }
  __syncthreads();
  if (tid == 0 && !(sig[dim - 1] > 1e-6 * sig[0])) *bad = 1;
  // 6. rot_y = K V[:, order], G = rot_y / sigma (into Cm [k2][dim])
  for (int idx = tid; idx < k2 * dim; idx += 256) {
    const int q = idx / dim, i = idx % dim, col = order[i];
    double s = 0.0;
    for (int m = 0; m < k2; ++m) s += Dm[q * LS + m] * Bm[m * LS + col];
    A[q * LS + i] = s;                                   // rot_y
    Cm[q * LS + i] = sig[i] > 0.0 ? s / sig[i] : 0.0;    // G
  }
  __syncthreads();
  const int F_ = P.fold0 + f, cols = P.n_lambda * dim;
  for (int idx = tid; idx < k2 * dim; idx += 256) {
    const int q = idx / dim, i = idx % dim;
    P.rot_y[((size_t)F_ * k2 + q) * cols + l * dim + i] = (float)A[q * LS + i];
  }
  if (tid < dim) {
    double b = 0.0;
    for (int q = 0; q < k2; ++q) b -= P.my[(size_t)f * k2 + q] * A[q * LS + tid];
    P.bias_y[(size_t)F_ * cols + l * dim + tid] = (float)b;
    P.e[((size_t)F_ * P.n_lambda + l) * dim + tid] = (float)sig[tid];
  }
  if (tid == 0) P.status[(size_t)F_ * P.n_lambda + l] = *bad;
  // 7. ut[i][r] = sum_q G[q][i] W^T[q][r]: the right-hand sides of rot_x = L^-T (W G), eight at a time
  double* ut = P.ut + (size_t)sys * P.ut_rows * np;
  for (int i0 = 0; i0 < P.ut_rows; i0 += 8) {
    for (int r = tid; r < np; r += 256) {
      double u[8];
      for (int i = 0; i < 8; ++i) u[i] = 0.0;
      if (r < k1) {
        for (int q = 0; q < k2; ++q) {
          const double wv = w[(size_t)q * np + r];
          for (int i = 0; i < 8; ++i) u[i] += (i0 + i < dim ? Cm[q * LS + i0 + i] : 0.0) * wv;
        }
      }
      for (int i = 0; i < 8; ++i) ut[(size_t)(i0 + i) * np + r] = u[i];
    }
  }
}

// rot_x [F][k1][n_lambda * dim] and bias_x = -mean_x rot_x from the backward pass's rows
__global__ __launch_bounds__(256) void cca_emit_kernel(const double* __restrict__ sol, const double* __restrict__ mx,
                                                       int k1, int np, int ut_rows, int n_lambda, int dim, int fold0,
                                                       float* __restrict__ rot_x, float* __restrict__ bias_x) {
  __shared__ double red[4];
  const int sys = blockIdx.x, f = sys / n_lambda, l = sys % n_lambda, tid = threadIdx.x;
  const int cols = n_lambda * dim;
  const double* s = sol + (size_t)sys * ut_rows * np;
  for (int i = 0; i < dim; ++i) {
    double b = 0.0;
    for (int r = tid; r < k1; r += 256) {
      const double v = s[(size_t)i * np + r];
      rot_x[((size_t)(fold0 + f) * k1 + r) * cols + l * dim + i] = (float)v;
      b -= mx[(size_t)f * k1 + r] * v;
    }
    for (int off = 32; off > 0; off >>= 1) b += __shfl_xor(b, off);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) bias_x[(size_t)(fold0 + f) * cols + l * dim + i] = (float)((red[0] + red[1]) + (red[2] + red[3]));
  }
}

struct Carver {
  char* p;
  explicit Carver(void* base) : p(reinterpret_cast<char*>(base)) {}
  template <typename T>
  T* take(size_t count) {
    T* r = reinterpret_cast<T*>(p);
    p += td_round_up((int64_t)(sizeof(T) * count), 256);
    return r;
  }
};

}  // namespace

extern "C" {

int td_cca_solve_loso_terms(td_handle* h, td_stats* total, td_stats* const* terms, const int* term_begin,
                            const double* signs, int n_folds, const int64_t* fold_batches, int batch_size,
                            const double* lambdas_host, int n_lambda, int dim, double eps_eig, float* rot_x_dev,
                            float* rot_y_dev, float* mean_x_dev, float* mean_y_dev, float* bias_x_dev,
                            float* bias_y_dev, float* e_dev, int* status_dev) {
  if (!h || !total || !term_begin || !fold_batches || !lambdas_host || !rot_x_dev || !rot_y_dev || !mean_x_dev ||
      !mean_y_dev || !bias_x_dev || !bias_y_dev || !e_dev || !status_dev)
    return td_fail(h, TD_ERR_INVALID, "td_cca_solve_loso_terms: NULL argument");
  int k1 = 0, k2 = 0;
  int64_t frames_total = 0;
  td_stats_dims(total, &k1, &k2, &frames_total);
  TD_REQUIRE(h, k2 > 0, "td_cca_solve_loso_terms: statistics were created without input_2");
  TD_REQUIRE(h, k2 <= NB, "td_cca_solve_loso_terms: input_2 is %d columns wide, at most %d", k2, NB);
  TD_REQUIRE(h, n_folds > 0 && n_lambda > 0 && batch_size > 0, "td_cca_solve_loso_terms: empty sweep");
  TD_REQUIRE(h, dim > 0 && dim <= std::min(k1, k2), "td_cca_solve_loso_terms: dim must be in [1, %d], not %d",
             std::min(k1, k2), dim);
  TD_REQUIRE(h, (long long)n_lambda * dim <= 4096, "td_cca_solve_loso_terms: %d x %d output columns", n_lambda, dim);
  const int n_terms = term_begin[n_folds];
  TD_REQUIRE(h, n_terms == 0 || (terms && signs), "td_cca_solve_loso_terms: NULL terms");
  for (int li = 0; li < n_lambda; ++li)
    TD_REQUIRE(h, lambdas_host[li] >= 0.0, "regularization lambda must be >= 0");
  // the distinct statistics objects: 0 = the total, then the terms in order of first appearance
  std::vector<td_stats*> distinct{total};
  std::vector<FoldDesc> descs((size_t)n_folds);
  for (int f = 0; f < n_folds; ++f) {
    FoldDesc& d = descs[f];
    memset(&d, 0, sizeof(d));
    const int nt = term_begin[f + 1] - term_begin[f];
    TD_REQUIRE(h, nt >= 0 && nt <= kMaxTerms, "td_cca_solve_loso_terms: fold %d has %d terms, at most %d", f, nt,
               kMaxTerms);
    int64_t frames = frames_total;
    for (int t = 0; t < nt; ++t) {
      td_stats* s = terms[term_begin[f] + t];
      const double sg = signs[term_begin[f] + t];
      TD_REQUIRE(h, s && (sg == 1.0 || sg == -1.0), "td_cca_solve_loso_terms: a term's sign is +1 or -1");
      int tk1 = 0, tk2 = 0;
      int64_t tf = 0;
      td_stats_dims(s, &tk1, &tk2, &tf);
      TD_REQUIRE(h, tk1 == k1 && tk2 == k2, "td_cca_solve_loso_terms: a term's layout differs from the total's");
      frames += sg > 0 ? tf : -tf;
      size_t idx = 0;
      while (idx < distinct.size() && distinct[idx] != s) ++idx;
      if (idx == distinct.size()) distinct.push_back(s);
      d.term[t] = (int)idx;
      d.sign[t] = sg;
    }
    d.n_terms = nt;
    TD_REQUIRE(h, frames == fold_batches[f] * (int64_t)batch_size && frames > 1,
               "td_cca_solve_loso_terms: fold %d holds %lld frames, not %lld minibatches of %d", f, (long long)frames,
               (long long)fold_batches[f], batch_size);
    d.inv_frames = 1.0 / (double)frames;
    d.inv_denom = 1.0 / (double)(frames - 1);
  }
  const int np = (int)td_round_up(k1, NB), nblk = np / NB;
  const int rt_rows = (int)td_round_up(k2, 8), ut_rows = (int)td_round_up(dim, 8);
  const size_t n1 = (size_t)k1 + 1;
  const size_t msz = (size_t)td_round_up((int64_t)(n1 * n1 + (size_t)k2 * k2 + (size_t)k1 * k2 + k2), 32);
  // folds per batched factorisation: by bytes and by count, at least one
  const size_t per_sys = sizeof(double) * ((size_t)np * np + (size_t)(rt_rows + 2 * ut_rows) * np + (size_t)nblk * NB * NB);
  int chunk = (int)std::min<size_t>((size_t)n_folds, std::min<size_t>(kChunkBytes / (per_sys * n_lambda),
                                                                       (size_t)(kChunkSystems / n_lambda)));
  if (chunk < 1) chunk = 1;
  const int batch_max = chunk * n_lambda;
  struct Ws {
    double *mom, *lams, *a, *rt, *ut, *sol, *linv, *tol, *cyy, *mx, *my;
    FoldDesc* folds;
  } w;
  auto carve = [&](void* base) {
    Carver cv(base);
    w.mom = cv.take<double>(msz * distinct.size());
    w.lams = cv.take<double>(n_lambda);
    w.folds = cv.take<FoldDesc>(n_folds);
    w.a = cv.take<double>((size_t)batch_max * np * np);
    w.rt = cv.take<double>((size_t)batch_max * rt_rows * np);
    w.ut = cv.take<double>((size_t)batch_max * ut_rows * np);
    w.sol = cv.take<double>((size_t)batch_max * ut_rows * np);
    w.linv = cv.take<double>((size_t)batch_max * nblk * NB * NB);
    w.tol = cv.take<double>(td_round_up(batch_max, 32));
    w.cyy = cv.take<double>((size_t)chunk * k2 * k2);
    w.mx = cv.take<double>((size_t)chunk * k1);
    w.my = cv.take<double>((size_t)chunk * k2);
    return (size_t)(cv.p - reinterpret_cast<char*>(base));
  };
  void* base = nullptr;
  TD_TRY(td_workspace(h, carve(nullptr), &base));
  carve(base);
  for (size_t m = 0; m < distinct.size(); ++m) {
    double* mo = w.mom + m * msz;
    TD_TRY(td_stats_moments_ld(h, distinct[m], mo, (int64_t)n1, nullptr, mo + n1 * n1, mo + n1 * n1 + (size_t)k2 * k2,
                               mo + n1 * n1 + (size_t)k2 * k2 + (size_t)k1 * k2));
  }
  TD_TRY(td_upload_async(h, lambdas_host, sizeof(double) * n_lambda, w.lams));
  TD_TRY(td_upload_async(h, descs.data(), sizeof(FoldDesc) * descs.size(), w.folds));
  if (!h->lds_opt_cca_tail) {
    TD_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&cca_tail_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * kTailDoubles)));
    h->lds_opt_cca_tail = true;
  }
  Moments M;
  M.base = w.mom; M.stride = (long long)msz; M.k1 = k1; M.k2 = k2;
  const unsigned tiles = (unsigned)(nblk * (nblk + 1) / 2);
  for (int f0 = 0; f0 < n_folds; f0 += chunk) {
    const int nf = std::min(chunk, n_folds - f0), batch = nf * n_lambda;
    hipLaunchKernelGGL(cca_cov_kernel, dim3(tiles, (unsigned)nf), dim3(256), 0, h->stream, M, w.folds + f0, w.lams,
                       n_lambda, np, w.a);
    RhsParams R;
    R.M = M; R.folds = w.folds + f0; R.n_lambda = n_lambda; R.np = np; R.rt_rows = rt_rows; R.fold0 = f0;
    R.rt = w.rt; R.cyy = w.cyy; R.mx = w.mx; R.my = w.my; R.mean_x = mean_x_dev; R.mean_y = mean_y_dev;
    hipLaunchKernelGGL(cca_rhs_kernel, dim3((unsigned)std::min<int64_t>(64, td_ceil_div((int64_t)k2 * np, 256)),
                                            (unsigned)nf), dim3(256), 0, h->stream, R);
    TD_HIP(h, hipGetLastError());
    TD_TRY(td_chol_batch_forward(h, w.a, w.rt, w.linv, w.tol, np, k1, k2, batch, rt_rows));
    TailParams T;
    T.k1 = k1; T.k2 = k2; T.np = np; T.rt_rows = rt_rows; T.ut_rows = ut_rows; T.n_lambda = n_lambda; T.dim = dim;
    T.fold0 = f0; T.eps = eps_eig; T.lams = w.lams; T.a = w.a; T.tol = w.tol; T.rt = w.rt; T.cyy = w.cyy; T.my = w.my;
    T.ut = w.ut; T.rot_y = rot_y_dev; T.bias_y = bias_y_dev; T.e = e_dev; T.status = status_dev;
    hipLaunchKernelGGL(cca_tail_kernel, dim3((unsigned)batch), dim3(256), sizeof(double) * kTailDoubles, h->stream, T);
    TD_HIP(h, hipGetLastError());
    for (int i0 = 0; i0 < dim; i0 += 8)
      TD_TRY(td_chol_batch_backward(h, w.a, w.ut + (size_t)i0 * np, w.sol + (size_t)i0 * np, w.linv, np,
                                    std::min(8, dim - i0), batch, ut_rows));
    hipLaunchKernelGGL(cca_emit_kernel, dim3((unsigned)batch), dim3(256), 0, h->stream, w.sol, w.mx, k1, np, ut_rows,
                       n_lambda, dim, f0, rot_x_dev, bias_x_dev);
    TD_HIP(h, hipGetLastError());
  }
  return TD_OK;
}

}  // extern "C"
