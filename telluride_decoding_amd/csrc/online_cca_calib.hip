// Online calibration of a CCA model (td_ccacalib_online_*): what infer_decoder.Decoder.train(data0, data1,
// window_size = W) takes from a labelled stretch with a CCADecoder -- per dim the statistics {mean_a, mean_b, power} of
// ONE correlator fed both classes, the scaled LDA over the `dims` columns between the window means of the unattended
// (class 0) and the attended (class 1) correlations, d' -- for (eeg, attended features, unattended features) rows that
// arrive in pushes of any length, with the bank's CURRENT model.  online_calib.hip's scheme, one column per dim: a bank
// of sessions, one workgroup each, the state on the device, ONE launch per push, the host counts the frames, a block
// of zeros is a fresh session, no atomics, vector stores only.
//
// One pass is enough, column by column: with a the EEG view's projection and b a speaker's, the window mean of
// (a_d - mean_a_d)(b_d - mean_b_d) / power_d is affine in the window's sums of a_d b_d, a_d and b_d,
//   m_d = (sum a_d b_d - mean_b_d sum a_d - mean_a_d sum b_d + W mean_a_d mean_b_d) / (W power_d),
// so the state keeps in float64, with D = dims and none of it a function of the final statistics, T(D) = 9 D^2 + 20 D
// sums (include/td_hotpath.h has the layout): the correlator's 6 D sums, per class the sum over the completed windows
// of z = (sum a b [D] | sum a [D] | sum b [D]) and the upper triangle of the sum of z z^T, and the open window's 5 D
// running sums; then the float32 tails as td_cca_online_push carries them.
//
// And no eigenproblem: scaled LDA on two classes uses the leading eigenvector of inv(Sw) Sb alone, Sb has rank one, so
// that vector is Sw^-1 (mu_1 - mu_0) up to scale and sign, and slope and intercept remove both.  The finish is one
// Cholesky solve of at most 16 x 16.
//
// The projections are td_cca_online_push's, bit for bit: online_cca_common.h's project_row, whose bits do not depend
// on this file's contraction mode.  A pass of frames leaves {a | b1 | b0} in LDS as the float32 values they are; the
// walk widens them where it reads them (the widening is exact, so it is the float64 copy of the frame).
//
// The walk, in frame order.  The 11 D per-frame sums have one owning lane each (the first 11 D threads): a lane keeps
// its sum in a register across the passes of a launch; a per-frame term is a product of two widened float32 values, or
// one of them alone: exact in float64.  A lane of the open window that sees a frame complete a window leaves its sum
// in LDS, win_s [window of the pass][5 D], and returns to zero.  Behind a barrier all 1024 threads share the 9 D^2 +
// 9 D class entries (three each at D = 16): a thread walks the pass's completed windows in order and gives its entry
// acc + z_i (a class's sum) or acc + z_i z_j UNFUSED (its Gram: the product rounds, then the add -- this file is
// compiled with fp contract(off), as online_calib.hip is).  An entry has the same thread in every pass, which reads
// what it stored.  So acc += float64(x) * float64(y) per frame, zsum + z and gram + np.outer(z, z) per window in NumPy
// are a bit-exact twin, and any cut of a recording gives the same state bytes.
//
// LDS: the walk's lanes d = 0 .. D - 1 of a sum read D consecutive words of a frame's 3 D (distinct banks; lanes of
// different sums that read the same word broadcast); the projection's streams are online_cca.hip's.
//
// The finish is a workgroup of 256 threads per session -- a thread per entry of the 16 x 16 scatter -- with the
// right-looking Cholesky's three barriers per column.  Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are
// in DESIGN.md section 42.
#include <cmath>

#include "online_cca_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 1024;     // 16 waves: td_cca_online_push's, a pass of 64 frames is 192 projections
constexpr int kWaves = kThreads / 64;
constexpr int kFinThreads = 256;   // a thread per entry of the dims x dims scatter
constexpr int kMaxC1 = 128, kMaxC2 = 32, kMaxLags = 64, kMaxDims = 16;   // td_cca_online_push's limits
constexpr int kPass = 64;          // emitted frames per pass of a workgroup; halved until the LDS budget holds
constexpr long long kLdsBudget = TD_CCA_ONLINE_LDS_BYTES;

// ---- the head: [0, 6 D) the correlator | class 0 | class 1 | the open window [5 D]
__host__ __device__ inline int class_entries(int dims) { return 3 * dims + 3 * dims * (3 * dims + 1) / 2; }
__host__ __device__ inline int head_sums(int dims) { return 9 * dims * dims + 20 * dims; }
__host__ __device__ inline int open_offset(int dims) { return 6 * dims + 2 * class_entries(dims); }
constexpr int kClassPerThread = (9 * kMaxDims * kMaxDims + 9 * kMaxDims + kThreads - 1) / kThreads;

__host__ __device__ inline long long head_end(int dims) { return 8LL * head_sums(dims); }
__host__ __device__ inline long long feat_tail_offset(int c1, int pre1, int post, int dims) {
  return tail_end(head_end(dims), c1, pre1 + post);
}
__host__ __device__ inline long long block_bytes(int c1, int pre1, int c2, int pre2, int post, int dims) {
  return tails_bytes(head_end(dims), c1, pre1 + post, 2LL * c2 * (pre2 + post));
}

// LDS of a launch: 8 (5 dims pass) for the windows a pass completes, then float32: both means (k1 + k2), both
// rotations (dims (k1 + k2)), the staged rows (R1 c1 + 2 R2 c2) and the pass's projections (3 dims pass).
__host__ __device__ inline long long lds_bytes(int c1, int pre1, int post1, int c2, int pre2, int post2, int dims,
                                               int pass) {
  const int post = delay_of(post1, post2);
  const long long k1 = (long long)c1 * (pre1 + 1 + post1), k2 = (long long)c2 * (pre2 + 1 + post2);
  const long long r1 = stage_rows(pass, pre1, post1, post), r2 = stage_rows(pass, pre2, post2, post);
  return 40LL * dims * pass + 4LL * ((dims + 1) * (k1 + k2) + r1 * c1 + 2 * r2 * c2 + 3LL * dims * pass);
}

// The largest pass (kPass halved, at least 1, no more than the frames to emit) whose LDS fits; 0: none does.
int pass_of(int c1, int pre1, int post1, int c2, int pre2, int post2, int dims, long long emitted_now) {
  int pass = emitted_now < kPass ? (emitted_now > 1 ? (int)emitted_now : 1) : kPass;
  while (pass > 1 && lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, pass) > kLdsBudget) pass = (pass + 1) / 2;
  return lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, pass) <= kLdsBudget ? pass : 0;
}

struct CcaCalibParams {
  const float* eeg; long long eeg_ld, eeg_ss;
  const float* feat[2]; long long feat_ld, feat_ss;   // attended, unattended
  const float *mean_x, *rot_x, *mean_y, *rot_y; long long model_ss;   // 0 or 1 (models)
  long long n, p0;               // rows of this push, rows pushed before it
  long long e0, e1;              // frames emitted before / after
  int c1, pre1, post1, c2, pre2, post2, dims, width, pass;
  unsigned char* state; long long state_ss;
};

// The column of the open window's sums (sum a | sum b1 | sum a b1 | sum b0 | sum a b0) that holds component i of a
// class's z = (sum a b | sum a | sum b): class 1 pairs a with b1, class 0 with b0.
__device__ __forceinline__ int z_column(int cls, int i, int dims) {
  const int blk = i / dims, d = i - blk * dims;
  if (blk == 0) return (cls ? 2 : 4) * dims + d;
  if (blk == 1) return d;
  return (cls ? 1 : 3) * dims + d;
}

enum : int { kPlain = 0, kOpenSum = 1, kIdle = 2 };

__global__ __launch_bounds__(kThreads) void online_ccacalib_push_kernel(CcaCalibParams p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x;
  const int c1 = p.c1, pre1 = p.pre1, post1 = p.post1, c2 = p.c2, pre2 = p.pre2, post2 = p.post2;
  const int dims = p.dims, width = p.width, pass = p.pass;
  const int post = delay_of(post1, post2);
  const int k1 = c1 * (pre1 + 1 + post1), k2 = c2 * (pre2 + 1 + post2);
  const int t1 = pre1 + post, t2 = pre2 + post;                 // rows of the tails
  const int r1 = stage_rows(pass, pre1, post1, post), r2 = stage_rows(pass, pre2, post2, post);
  double* win_s = lds;                                          // [pass][5 dims] the windows a pass completes
  float* mean1_s = reinterpret_cast<float*>(win_s + (size_t)5 * dims * pass);   // [k1]
  float* mean2_s = mean1_s + k1;                                // [k2]
  float* rot1_s = mean2_s + k2;                                 // [dims][k1]
  float* rot2_s = rot1_s + (size_t)dims * k1;                   // [dims][k2]
  float* rows1_s = rot2_s + (size_t)dims * k2;                  // [r1][c1] the pass's EEG rows
  float* rows2_s = rows1_s + (size_t)r1 * c1;                   // [2][r2][c2] the pass's feature rows
  float* proj_s = rows2_s + 2 * (size_t)r2 * c2;                // [pass][3 dims] a | b1 | b0

  unsigned char* st = p.state + (long long)s * p.state_ss;
  double* head = reinterpret_cast<double*>(st);                                             // [head_sums(dims)]
  float* tail1 = reinterpret_cast<float*>(st + head_end(dims));                     // [t1][c1]
  float* tail2 = reinterpret_cast<float*>(st + feat_tail_offset(c1, pre1, post, dims));    // [2][t2][c2]
  const float* eeg = p.eeg + (long long)s * p.eeg_ss;
  const float* feat[2] = {p.feat[0] + (long long)s * p.feat_ss, p.feat[1] + (long long)s * p.feat_ss};
  const long long ms = (long long)s * p.model_ss;
  const long long p0 = p.p0, p1 = p.p0 + p.n;

  stage_model<kThreads>(mean1_s, mean2_s, rot1_s, rot2_s, p.mean_x + ms * k1, p.rot_x + ms * k1 * dims,
                        p.mean_y + ms * k2, p.rot_y + ms * k2 * dims, k1, k2, dims);

  // ---- the walk's lanes: thread t < 6 dims owns the correlator's sum t, the next 5 dims threads the open window's
  const int n_class = class_entries(dims), open0 = open_offset(dims);
  int role = kIdle, f0 = 0, f1 = -1, mine = 0;                  // the term is v[f0] v[f1], or v[f0] alone
  double acc = 0.0;
  if (tid < 11 * dims) {
    const int j = tid / dims, d = tid - j * dims;
    if (j < 6) {                                                // sum a, a^2, b1, b1^2, b0, b0^2
      role = kPlain;
      mine = tid;
      f0 = (j >> 1) * dims + d;
      f1 = (j & 1) ? f0 : -1;
    } else {                                                    // sum a, b1, a b1, b0, a b0
      role = kOpenSum;
      const int q = j - 6;
      mine = open0 + (tid - 6 * dims);
      f0 = (q == 0 ? 0 : (q <= 2 ? 1 : 2)) * dims + d;
      f1 = (q == 2 || q == 4) ? d : -1;
    }
    acc = head[mine];
  }
  // ---- the class entries: thread t owns entries t, t + 1024, ... of the 2 n_class behind the correlator's sums
  int zi[kClassPerThread], zj[kClassPerThread];                 // win_s columns; zj < 0: a class's sum z, zi < 0: none
#pragma unroll
  for (int u = 0; u < kClassPerThread; ++u) {
    const int e = tid + u * kThreads;
    zi[u] = zj[u] = -1;
    if (e < 2 * n_class) {
      const int cls = e / n_class, r = e - cls * n_class;
      if (r < 3 * dims) {
        zi[u] = z_column(cls, r, dims);
      } else {
        int g = r - 3 * dims, i = 0;                            // row-major upper triangle of [3 dims][3 dims]
        while (g >= 3 * dims - i) { g -= 3 * dims - i; ++i; }
        zi[u] = z_column(cls, i, dims);
        zj[u] = z_column(cls, i + g, dims);
      }
    }
  }

  for (long long a = p.e0; a < p.e1; a += pass) {
    const int nf = (int)(p.e1 - a < pass ? p.e1 - a : pass);     // frames [a, a + nf) of this pass
    // ---- stage the EEG rows a - pre1 .. a + nf - 1 + post1 and each class's feature rows a - pre2 ..
    // a + nf - 1 + post2
    stage_rows<kThreads>(rows1_s, c1, tail1, t1, eeg, p.eeg_ld, c1, a - pre1, nf + pre1 + post1, p0, p1);
    stage_feat<kThreads>(rows2_s, r2, tail2, t2, feat, p.feat_ld, c2, a - pre2, nf + pre2 + post2, p0, p1);
    __syncthreads();
    // ---- projections, td_cca_online_push's: a wave per (frame, view)
    for (int t = wave; t < 3 * nf; t += kWaves) {
      const int f = t / 3, part = t - 3 * f;
      float* out = proj_s + (size_t)f * 3 * dims + part * dims;
      if (part == 0) project_row(rows1_s + (size_t)f * c1, mean1_s, rot1_s, k1, dims, lane, out);
      else project_row(rows2_s + ((size_t)(part - 1) * r2 + f) * c2, mean2_s, rot2_s, k2, dims, lane, out);
    }
    __syncthreads();
    // ---- the walk: every per-frame sum advances by this pass's frames in frame order
    const int n_done = (int)((a + nf) / width - a / width);      // windows this pass completes
    if (role != kIdle) {
      int pos = (int)(a % width), done = 0;                      // frames of the open window before frame a
      for (int f = 0; f < nf; ++f) {
        const float* v = proj_s + (size_t)f * 3 * dims;
        double term = (double)v[f0];
        if (f1 >= 0) term = term * (double)v[f1];                // exact
        acc = acc + term;
        if (++pos == width) {
          pos = 0;
          if (role == kOpenSum) {
            win_s[(size_t)done * 5 * dims + (mine - open0)] = acc;
            acc = 0.0;
          }
          ++done;
        }
      }
    }
    __syncthreads();
    // ---- the windows this pass completed, in order: a class's sum z takes z_i, its Gram z_i z_j
    if (n_done > 0) {
#pragma unroll
      for (int u = 0; u < kClassPerThread; ++u) {
        if (zi[u] < 0) continue;
        double* at = head + 6 * dims + tid + u * kThreads;
        double g = *at;
        for (int w = 0; w < n_done; ++w) {
          const double* z = win_s + (size_t)w * 5 * dims;
          if (zj[u] < 0) {
            g = g + z[zi[u]];
          } else {
            const double zz = z[zi[u]] * z[zj[u]];               // rounded, then the add rounds: G + z_i z_j unfused
            g = g + zz;
          }
        }
        *at = g;
      }
    }
    // (the next pass stores win_s and proj_s behind its two barriers)
  }

  // ---- the tails for the next push: the last pre1 + post EEG rows and the last pre2 + post feature rows
  __syncthreads();
  const long long n = p.n;
  tail_park<kThreads>(rows1_s, tail1, t1, c1, n);
  feat_tail_park<kThreads>(rows2_s, r2, tail2, t2, c2, n);
  __syncthreads();
  tail_store<kThreads>(tail1, rows1_s, t1, c1, eeg, p.eeg_ld, n);
  feat_tail_store<kThreads>(tail2, rows2_s, r2, t2, c2, feat, p.feat_ld, n);
  if (role != kIdle && p.e1 > p.e0) head[mine] = acc;
}

// Entry (r, c) of a symmetric matrix kept as its row-major upper triangle of side n.
__device__ __forceinline__ double upper_at(const double* g, int n, int r, int c) {
  const int lo = r < c ? r : c, hi = r < c ? c : r;
  return g[lo * n - lo * (lo - 1) / 2 + (hi - lo)];
}

// grid (S), a workgroup per session, float64.  Every barrier is reached by every thread: a session that fails a test
// goes on with what it has (NaN or infinity at worst) and thread 0 sorts it out at the end.
__global__ __launch_bounds__(kFinThreads) void online_ccacalib_finish_kernel(const unsigned char* state,
                                                                             long long state_ss, int dims,
                                                                             long long frames, int width, double* corr,
                                                                             double* lda, double* dprime,
                                                                             int* status) {
  __shared__ double mean_a[kMaxDims], mean_b[kMaxDims], power[kMaxDims], c0[kMaxDims];
  __shared__ double cz_s[2][kMaxDims], mu_s[2][kMaxDims];       // C sum z and the class means
  __shared__ double sc_s[2][kMaxDims * kMaxDims];               // the classes' scatters S_0, S_1
  __shared__ double l_s[kMaxDims * kMaxDims];                   // Sw, then its Cholesky factor in the lower triangle
  __shared__ double v_s[kMaxDims], w_s[kMaxDims], sw_s[2][kMaxDims], norm_s;
  __shared__ int bad_power, bad_pivot;
  const int tid = threadIdx.x, s = blockIdx.x, D = dims;
  const double* q = reinterpret_cast<const double*>(state + (long long)s * state_ss);
  const int n_class = class_entries(D);
  const double count = 2.0 * (double)frames, n_win = (double)(frames / width);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (tid == 0) bad_power = bad_pivot = 0;
  __syncthreads();
  // ---- the correlator after train's add(data0) then add(data1): class 0 = (a, b0) first, then class 1 = (a, b1)
  if (tid < D) {
    const int d = tid;
    const double sum_x = q[d] + q[d], sum_x2 = q[D + d] + q[D + d];
    const double sum_y = q[4 * D + d] + q[2 * D + d], sum_y2 = q[5 * D + d] + q[3 * D + d];
    const double ma = sum_x / count, mb = sum_y / count;
    const double pw = sqrt((sum_x2 - sum_x * sum_x / count) * (sum_y2 - sum_y * sum_y / count)) / count;
    mean_a[d] = ma; mean_b[d] = mb; power[d] = pw; c0[d] = ma * mb / pw;
    if (!(pw > 0.0) || isinf(pw)) bad_power = 1;
  }
  __syncthreads();
  // ---- per class: C sum z and the mean
  if (tid < 2 * D) {
    const int cls = tid / D, d = tid - cls * D;
    const double* z = q + 6 * D + cls * n_class;
    const double sc = 1.0 / ((double)width * power[d]);
    const double cz = (sc * z[d] + (-mean_b[d] * sc) * z[D + d]) + (-mean_a[d] * sc) * z[2 * D + d];
    cz_s[cls][d] = cz;
    mu_s[cls][d] = (cz + n_win * c0[d]) / n_win;
  }
  __syncthreads();
  // ---- per class: S = C G C^T + cz c0^T + c0 cz^T + n c0 c0^T - n mu mu^T, a thread per entry; Sw = S_0 + S_1
  if (tid < D * D) {
    const int d = tid / D, e = tid - d * D;
    const double sd = 1.0 / ((double)width * power[d]), se = 1.0 / ((double)width * power[e]);
    const double cd[3] = {sd, -mean_b[d] * sd, -mean_a[d] * sd}, ce[3] = {se, -mean_b[e] * se, -mean_a[e] * se};
    double sw = 0.0;
#pragma unroll
    for (int cls = 0; cls < 2; ++cls) {
      const double* g = q + 6 * D + cls * n_class + 3 * D;
      double m = 0.0;
#pragma unroll
      for (int pi = 0; pi < 3; ++pi)
#pragma unroll
        for (int qi = 0; qi < 3; ++qi) m = m + (cd[pi] * ce[qi]) * upper_at(g, 3 * D, pi * D + d, qi * D + e);
      const double smm = ((m + cz_s[cls][d] * c0[e]) + c0[d] * cz_s[cls][e]) + n_win * c0[d] * c0[e];
      const double sv = smm - n_win * mu_s[cls][d] * mu_s[cls][e];
      sc_s[cls][tid] = sv;
      sw = sw + sv;
    }
    l_s[tid] = sw;
  }
  if (tid < D) v_s[tid] = mu_s[1][tid] - mu_s[0][tid];
  __syncthreads();
  // ---- Sw = L L^T, right-looking: the pivot, the column, the update of what lies right of it
  for (int k = 0; k < D; ++k) {
    if (tid == 0) {
      const double piv = l_s[k * D + k];
      if (!(piv > 0.0) || isinf(piv)) bad_pivot = 1;
      l_s[k * D + k] = sqrt(piv);
    }
    __syncthreads();
    if (tid > k && tid < D) l_s[tid * D + k] = l_s[tid * D + k] / l_s[k * D + k];
    __syncthreads();
    if (tid < D * D) {
      const int i = tid / D, j = tid - i * D;
      if (j > k && i >= j) l_s[tid] = l_s[tid] - l_s[i * D + k] * l_s[j * D + k];
    }
    __syncthreads();
  }
  // ---- v = Sw^-1 (mu_1 - mu_0): L y = mu_1 - mu_0, then L^T v = y
  for (int k = 0; k < D; ++k) {
    if (tid == 0) v_s[k] = v_s[k] / l_s[k * D + k];
    __syncthreads();
    if (tid > k && tid < D) v_s[tid] = v_s[tid] - l_s[tid * D + k] * v_s[k];
    __syncthreads();
  }
  for (int k = D - 1; k >= 0; --k) {
    if (tid == 0) v_s[k] = v_s[k] / l_s[k * D + k];
    __syncthreads();
    if (tid < k) v_s[tid] = v_s[tid] - l_s[k * D + tid] * v_s[k];
    __syncthreads();
  }
  if (tid == 0) {
    double nn = 0.0;
    for (int d = 0; d < D; ++d) nn = nn + v_s[d] * v_s[d];
    norm_s = sqrt(nn);
  }
  __syncthreads();
  if (tid < D) w_s[tid] = D == 1 ? 1.0 : v_s[tid] / norm_s;     // (the reference's w at one column is [1])
  __syncthreads();
  if (tid < 2 * D) {                                            // S_c w
    const int cls = tid / D, d = tid - cls * D;
    double t = 0.0;
    for (int e = 0; e < D; ++e) t = t + sc_s[cls][d * D + e] * w_s[e];
    sw_s[cls][d] = t;
  }
  __syncthreads();
  int st = TD_CALIB_OK;
  if (n_win < 1.0) st = TD_CALIB_NO_WINDOW;
  else if (bad_power) st = TD_CALIB_NO_POWER;
  else if (bad_pivot || 2.0 * n_win < (double)D + 2.0) st = TD_CALIB_NOT_POSITIVE;   // (rank <= 2 n_win - 2)
  const bool have_stats = st != TD_CALIB_NO_WINDOW && st != TD_CALIB_NO_POWER;
  if (tid < D) {
    double* cr = corr + 6LL * D * s;
    for (int spk = 0; spk < 2; ++spk) {
      cr[(3 * spk) * D + tid] = have_stats ? mean_a[tid] : nan;
      cr[(3 * spk + 1) * D + tid] = have_stats ? mean_b[tid] : nan;
      cr[(3 * spk + 2) * D + tid] = have_stats ? power[tid] : nan;
    }
  }
  if (tid == 0) {
    double along = 0.0, at0 = 0.0, spread = 0.0;
    for (int d = 0; d < D; ++d) {
      along = along + (mu_s[1][d] - mu_s[0][d]) * w_s[d];
      at0 = at0 + mu_s[0][d] * w_s[d];
      spread = spread + (w_s[d] * sw_s[0][d] + w_s[d] * sw_s[1][d]);
    }
    if (st == TD_CALIB_OK && (along == 0.0 || isnan(along))) st = TD_CALIB_SAME_MEANS;   // equal, or not a number
    const bool ok = st == TD_CALIB_OK;
    const double slope = 1.0 / along;
    double* out = lda + (long long)(D + 2) * s;
    for (int d = 0; d < D; ++d) out[d] = ok ? w_s[d] : nan;
    out[D] = ok ? slope : nan;
    out[D + 1] = ok ? -slope * at0 : nan;
    dprime[s] = ok ? fabs(along) / sqrt(spread / (2.0 * n_win)) : nan;
    status[s] = st;
  }
}

// The shape checks td_ccacalib_online_state_bytes, td_ccacalib_online_lds_bytes and td_ccacalib_online_push share.
int check_shape(td_handle* h, const char* who, int c1, int pre1, int post1, int c2, int pre2, int post2, int dims,
                int width) {
  TD_TRY(check_cca_views(h, who, c1, pre1, post1, c2, pre2, post2, dims, width, kMaxC1, kMaxC2, kMaxLags, kMaxDims));
  const long long need = lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, 1);
  TD_REQUIRE(h, need <= kLdsBudget,
             "%s: the rotations of %d x %d and %d x %d lags in %d dims and a pass of one frame take %lld bytes of "
             "LDS (budget %lld bytes)", who, c1, pre1 + 1 + post1, c2, pre2 + 1 + post2, dims, need, kLdsBudget);
  return TD_OK;
}

}  // namespace

extern "C" {

int td_ccacalib_online_state_bytes(int c1, int pre1, int post1, int c2, int pre2, int post2, int dims,
                                   int64_t* bytes) {
  if (!bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_ccacalib_online_state_bytes: NULL argument");
  TD_TRY(check_shape(nullptr, "td_ccacalib_online_state_bytes", c1, pre1, post1, c2, pre2, post2, dims, 1));
  *bytes = block_bytes(c1, pre1, c2, pre2, delay_of(post1, post2), dims);
  return TD_OK;
}

int td_ccacalib_online_lds_bytes(int c1, int pre1, int post1, int c2, int pre2, int post2, int dims,
                                 int64_t emitted, int* pass, int64_t* bytes) {
  if (!pass || !bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_ccacalib_online_lds_bytes: NULL argument");
  TD_TRY(check_shape(nullptr, "td_ccacalib_online_lds_bytes", c1, pre1, post1, c2, pre2, post2, dims, 1));
  TD_REQUIRE(nullptr, emitted >= 0, "td_ccacalib_online_lds_bytes: %lld frames", (long long)emitted);
  *pass = pass_of(c1, pre1, post1, c2, pre2, post2, dims, emitted);
  *bytes = lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, *pass);
  return TD_OK;
}

int td_ccacalib_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t eeg_ld,
                            int64_t eeg_session_stride, const float* att_dev, const float* unatt_dev,
                            int64_t feat_ld, int64_t feat_session_stride, int64_t n, int c1, int pre1, int post1,
                            int c2, int pre2, int post2, int dims, const float* mean_x_dev, const float* rot_x_dev,
                            const float* mean_y_dev, const float* rot_y_dev, int64_t model_session_stride, int width,
                            int64_t frames_before, int flush, void* state_dev, int64_t state_session_stride) {
  const char* who = "td_ccacalib_online_push";
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_ccacalib_online_push: handle is NULL");
  TD_TRY(check_shape(h, who, c1, pre1, post1, c2, pre2, post2, dims, width));
  TD_REQUIRE(h, n >= 0 && n <= TD_ONLINE_MAX_PUSH, "%s: %lld rows in one push (0 .. %d)", who, (long long)n,
             TD_ONLINE_MAX_PUSH);
  TD_REQUIRE(h, frames_before >= 0, "%s: %lld frames before", who, (long long)frames_before);
  const int post = delay_of(post1, post2);
  TD_TRY(check_state(h, who, num_sessions, state_dev, state_session_stride,
                     block_bytes(c1, pre1, c2, pre2, post, dims)));
  if (!mean_x_dev || !rot_x_dev || !mean_y_dev || !rot_y_dev || (n > 0 && (!eeg_dev || !att_dev || !unatt_dev)))
    return td_fail(h, TD_ERR_INVALID, "%s: NULL argument", who);
  if (n > 0)
    TD_TRY(check_push_strides(h, who, num_sessions, eeg_ld, eeg_session_stride, c1, feat_ld, feat_session_stride, c2,
                              "features"));
  TD_REQUIRE(h, model_session_stride == 0 || model_session_stride == 1,
             "%s: a model stride of %lld models (0 = one model, 1 = one per session)", who,
             (long long)model_session_stride);
  if (n == 0 && !flush) return TD_OK;
  const OnlinePlan pl = plan_push(frames_before, n, post, width, width, flush);   // (its windows: hop = width)
  CcaCalibParams p;
  p.eeg = eeg_dev; p.eeg_ld = eeg_ld; p.eeg_ss = num_sessions > 1 ? eeg_session_stride : 0;
  p.feat[0] = att_dev; p.feat[1] = unatt_dev; p.feat_ld = feat_ld;
  p.feat_ss = num_sessions > 1 ? feat_session_stride : 0;
  p.mean_x = mean_x_dev; p.rot_x = rot_x_dev; p.mean_y = mean_y_dev; p.rot_y = rot_y_dev;
  p.model_ss = model_session_stride;
  p.n = n; p.p0 = frames_before; p.e0 = pl.emitted_before; p.e1 = pl.emitted_after;
  p.c1 = c1; p.pre1 = pre1; p.post1 = post1; p.c2 = c2; p.pre2 = pre2; p.post2 = post2; p.dims = dims;
  p.width = width;
  p.pass = pass_of(c1, pre1, post1, c2, pre2, post2, dims, p.e1 - p.e0);   // (>= 1: check_shape)
  p.state = reinterpret_cast<unsigned char*>(state_dev); p.state_ss = state_session_stride;
  return launch_push(h, &h->lds_opt_online_ccacalib, online_ccacalib_push_kernel, num_sessions, kThreads, kLdsBudget,
                     lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, p.pass), (double)n * num_sessions, p);
}

int td_ccacalib_online_sums(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride,
                            int dims, double* out_dev) {
  const char* who = "td_ccacalib_online_sums";
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_ccacalib_online_sums: handle is NULL");
  TD_REQUIRE(h, dims >= 1 && dims <= kMaxDims, "%s: %d dims (1 .. %d)", who, dims, kMaxDims);
  TD_TRY(check_state(h, who, num_sessions, state_dev, state_session_stride, 8LL * head_sums(dims)));
  if (!out_dev) return td_fail(h, TD_ERR_INVALID, "%s: NULL argument", who);
  return launch_head_sums(h, num_sessions, state_dev, state_session_stride, head_sums(dims), out_dev);
}

int td_ccacalib_online_finish(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride,
                              int dims, int64_t frames_emitted, int width, double* corr_dev, double* lda_dev,
                              double* dprime_dev, int32_t* status_dev) {
  const char* who = "td_ccacalib_online_finish";
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_ccacalib_online_finish: handle is NULL");
  TD_REQUIRE(h, dims >= 1 && dims <= kMaxDims, "%s: %d dims (1 .. %d)", who, dims, kMaxDims);
  TD_TRY(check_state(h, who, num_sessions, state_dev, state_session_stride, 8LL * head_sums(dims)));
  TD_REQUIRE(h, width >= 1 && width <= TD_ONLINE_MAX_WIDTH, "%s: window of %d frames (1 .. %d)", who, width,
             TD_ONLINE_MAX_WIDTH);
  TD_REQUIRE(h, frames_emitted >= 0, "%s: %lld frames emitted", who, (long long)frames_emitted);
  if (!corr_dev || !lda_dev || !dprime_dev || !status_dev) return td_fail(h, TD_ERR_INVALID, "%s: NULL argument", who);
  TD_TRY(td_profile_mark(h, true, (double)num_sessions));
  hipLaunchKernelGGL(online_ccacalib_finish_kernel, dim3((unsigned)num_sessions), dim3(kFinThreads), 0, h->stream,
                     reinterpret_cast<const unsigned char*>(state_dev), (long long)state_session_stride, dims,
                     (long long)frames_emitted, width, corr_dev, lda_dev, dprime_dev, status_dev);
  TD_HIP(h, hipGetLastError());
  TD_TRY(td_profile_mark(h, false, 0.0));
  return TD_OK;
}

}  // extern "C"
