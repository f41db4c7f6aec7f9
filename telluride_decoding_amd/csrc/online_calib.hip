// Online calibration (td_calib_online_*): what infer_decoder.Decoder.train(data0, data1, window_size = W) takes from a
// labelled stretch -- the correlator's statistics {mean_truth, mean_pred, power}, the scaled LDA between the window
// means of the unattended (class 0) and the attended (class 1) correlations, d' -- for (eeg, attended envelope,
// unattended envelope) rows that arrive in pushes of any length, with the bank's CURRENT weights.  As the online family
// does everything else: a bank of sessions, one workgroup of 256 threads each, the state on the device, ONE launch per
// push, the host counts the frames, a block of zeros is a fresh session, no atomics, vector stores only.
//
// One pass is enough.  train needs two because the per-frame correlation (x - mean_x)(p - mean_y) / power (x the
// truth, p the prediction) takes the FINAL statistics; but a window mean of it is affine in three per-window sums,
//   m_w = (sum x p - mean_y sum x - mean_x sum p + W mean_x mean_y) / (W power),
// so the state keeps, in float64, none of them a function of the final statistics, online_calib_common.h's 29 sums
// (the layout is there: the correlator's six, per class sum_w z and the upper triangle of sum_w z z^T with
// z = (sum x p, sum x, sum p), the open window's five), then the EEG tail [pre + post][c] and the envelope tail [post][2] in float32, as td_online_push's block carries
// them, rounded up to 8 bytes.  Windows are infer_decoder.average_data's: consecutive, hop = width, the tail dropped.
//
// The prediction of an emitted frame is the float32 value td_online_push returns in `pred`: the same function
// (online_common.h's fir_predict, whose bits do not depend on this file's contraction mode).
//
// The sums advance in frame order, one lane per state double: online_calib_common.h's walk, which
// online_dnn_calib.hip shares -- the head's layout, the lanes' roles, the Gram's G + z_i z_j UNFUSED under that
// header's fp contract(off) (this file switches it off too, as online_fit.hip does and for its reason).  So
// acc += float64(x) * float64(p) and G + np.outer(z, z) in NumPy are a bit-exact twin, and any cut of a recording
// gives the same state bytes.  The serial walk is intended: pushes are tens to hundreds of frames and the prediction
// dominates.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are in DESIGN.md section 35.
#include <cmath>

#include "online_calib_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxChannels = TD_CALIB_ONLINE_MAX_CHANNELS, kMaxLags = TD_CALIB_ONLINE_MAX_LAGS;
constexpr int kPass = 64;       // emitted frames per pass of a workgroup (fewer for a short push: less LDS)

struct CalibParams {
  const float* eeg; long long eeg_ld, eeg_ss;
  const float* env; long long env_ld, env_ss;
  const float* w; long long w_ss;
  const float* b; long long b_ss;
  long long n, p0;               // rows of this push, rows pushed before it
  long long e0, e1;              // frames emitted before / after
  int c, pre, post, width, pass;
  unsigned char* state; long long state_ss;
};

__global__ __launch_bounds__(kThreads) void online_calib_push_kernel(CalibParams p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x;
  const int c = p.c, pre = p.pre, post = p.post, width = p.width;
  const int tl = pre + post, nl = tl + 1, k_all = nl * c, pass = p.pass;
  double* val_s = lds;                                       // [pass][4] a frame's {1, p, a, u}
  float* w_s = reinterpret_cast<float*>(val_s + 4 * pass);   // [nl c] the weights
  float* rows_s = w_s + k_all;                               // [pass + tl][c] the pass's EEG rows
  float* env_s = rows_s + (size_t)(pass + tl) * c;           // [max(pass, post)][2]

  unsigned char* st = p.state + (long long)s * p.state_ss;
  double* sums = reinterpret_cast<double*>(st);                                    // [kSums]
  float* tail = reinterpret_cast<float*>(st + state_eeg_offset());                 // [tl][c]
  float* etail = reinterpret_cast<float*>(st + state_env_offset(c, pre, post));    // [post][2]
  const float* eeg = p.eeg + (long long)s * p.eeg_ss;
  const float* env = p.env + (long long)s * p.env_ss;
  const float* w = p.w + (long long)s * p.w_ss;
  const float bias = p.b[(long long)s * p.b_ss];
  const long long p0 = p.p0, p1 = p.p0 + p.n;

  for (int k = tid; k < k_all; k += kThreads) w_s[k] = w[k];

  WalkLane wl = walk_lane(sums, tid);                        // lane t owns state double t

  for (long long a = p.e0; a < p.e1; a += pass) {
    const int nf = (int)(p.e1 - a < pass ? p.e1 - a : pass);     // frames [a, a + nf) of this pass
    // ---- stage the EEG rows a - pre .. a + nf - 1 + post and the envelope rows a .. a + nf - 1
    stage_rows<kThreads>(rows_s, c, tail, tl, eeg, p.eeg_ld, c, a - pre, nf + tl, p0, p1);
    stage_env<kThreads>(env_s, etail, post, env, p.env_ld, a, nf, p0);
    __syncthreads();
    // ---- predictions, td_online_push's: a wave per frame
    for (int f = wave; f < nf; f += kWaves) {
      const float pr = fir_predict(w_s, rows_s + f * c, k_all, bias);
      if (lane == 0) {
        val_s[4 * f] = 1.0;
        val_s[4 * f + 1] = (double)pr;
        val_s[4 * f + 2] = (double)env_s[2 * f];
        val_s[4 * f + 3] = (double)env_s[2 * f + 1];
      }
    }
    __syncthreads();
    // ---- the walk: every sum advances by this pass's frames in frame order
    walk_advance(wl, val_s, (int)(a % width), nf, width);
    __syncthreads();
  }

  // ---- the tails for the next push: the last pre + post EEG rows and the last post envelope rows
  __syncthreads();
  tail_park<kThreads>(rows_s, tail, tl, c, p.n);
  env_tail_park<kThreads>(env_s, etail, post, p.n);
  __syncthreads();
  tail_store<kThreads>(tail, rows_s, tl, c, eeg, p.eeg_ld, p.n);
  env_tail_store<kThreads>(etail, env_s, post, env, p.env_ld, p.n);
  // (every lane read the open sums it copies before the first pass; the barriers since then order these stores
  // behind those loads)
  if (wl.role != kIdle && p.e1 > p.e0) sums[tid] = wl.acc;
}

size_t lds_bytes(int c, int nl, int post, int pass) {
  const size_t env_rows = pass > post ? pass : post;
  return sizeof(double) * 4 * pass + sizeof(float) * ((size_t)nl * c + (size_t)(pass + nl - 1) * c + 2 * env_rows);
}

// One class's window-mean moments from its sums: {sum_w m, sum_w m^2} with m = c . z + c0.
__device__ __forceinline__ void class_moments(const double* q, const double* cv, double c0, double n_win, double* sm,
                                              double* sm2) {
  const double cz = (cv[0] * q[0] + cv[1] * q[1]) + cv[2] * q[2];
  const double* g = q + 3;                                   // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
  const double quad = ((g[0] * cv[0] * cv[0] + g[3] * cv[1] * cv[1]) + g[5] * cv[2] * cv[2]) +
                      2.0 * ((g[1] * cv[0] * cv[1] + g[2] * cv[0] * cv[2]) + g[4] * cv[1] * cv[2]);
  *sm = cz + n_win * c0;
  *sm2 = (quad + 2.0 * c0 * cz) + n_win * c0 * c0;
}

// grid (ceil(S / 256)): a thread per session, float64
__global__ __launch_bounds__(kThreads) void online_calib_finish_kernel(const unsigned char* state, long long state_ss,
                                                                       int num_sessions, long long frames, int width,
                                                                       double* corr, double* lda, double* dprime,
                                                                       int* status) {
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= num_sessions) return;
  const double* q = reinterpret_cast<const double*>(state + (long long)s * state_ss);
  // the correlator after train's add(data0) then add(data1): class 0 = (u, p) first, then class 1 = (a, p)
  const double count = 2.0 * (double)frames;
  const double sum_x = q[4] + q[2], sum_x2 = q[5] + q[3], sum_y = q[0] + q[0], sum_y2 = q[1] + q[1];
  const double mean_x = sum_x / count, mean_y = sum_y / count;
  const double power = sqrt((sum_x2 - sum_x * sum_x / count) * (sum_y2 - sum_y * sum_y / count)) / count;
  const double n_win = (double)(frames / width);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  int st = TD_CALIB_OK;
  double slope = nan, icpt = nan, dp = nan;
  if (n_win < 1.0) {
    st = TD_CALIB_NO_WINDOW;
  } else if (!(power > 0.0) || isinf(power)) {
    st = TD_CALIB_NO_POWER;
  } else {
    const double scale = 1.0 / ((double)width * power);
    const double cv[3] = {scale, -mean_y * scale, -mean_x * scale};
    const double c0 = mean_x * mean_y / power;
    double sm0, sq0, sm1, sq1;
    class_moments(q + 6, cv, c0, n_win, &sm0, &sq0);
    class_moments(q + 15, cv, c0, n_win, &sm1, &sq1);
    const double m0 = sm0 / n_win, m1 = sm1 / n_win;
    const double v0 = sq0 / n_win - m0 * m0, v1 = sq1 / n_win - m1 * m1;
    if (m0 == m1 || isnan(m0) || isnan(m1)) {                // equal, or not a number
      st = TD_CALIB_SAME_MEANS;
    } else {
      slope = 1.0 / (m1 - m0);
      icpt = -slope * m0;
      dp = fabs(m1 - m0) / sqrt((v0 + v1) / 2.0);
    }
  }
  const bool have_stats = st == TD_CALIB_OK || st == TD_CALIB_SAME_MEANS;
  double* cr = corr + 6LL * s;
  for (int spk = 0; spk < 2; ++spk) {
    cr[3 * spk] = have_stats ? mean_x : nan;
    cr[3 * spk + 1] = have_stats ? mean_y : nan;
    cr[3 * spk + 2] = have_stats ? power : nan;
  }
  lda[3LL * s] = 1.0;
  lda[3LL * s + 1] = slope;
  lda[3LL * s + 2] = icpt;
  dprime[s] = dp;
  status[s] = st;
}

int check_shape(td_handle* h, const char* who, int c, int pre, int post) {
  TD_REQUIRE(h, c >= 1 && c <= kMaxChannels, "%s: %d channels (1 .. %d)", who, c, kMaxChannels);
  TD_REQUIRE(h, pre >= 0 && post >= 0 && pre + 1 + post <= kMaxLags,
             "%s: a context of %d + 1 + %d lags (1 .. %d)", who, pre, post, kMaxLags);
  return TD_OK;
}

}  // namespace

extern "C" {

int td_calib_online_state_bytes(int c, int pre, int post, int64_t* bytes) {
  if (!bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_calib_online_state_bytes: NULL argument");
  TD_TRY(check_shape(nullptr, "td_calib_online_state_bytes", c, pre, post));
  *bytes = state_bytes(c, pre, post);
  return TD_OK;
}

int td_calib_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t eeg_ld,
                         int64_t eeg_session_stride, const float* env_dev, int64_t env_ld,
                         int64_t env_session_stride, const float* w_dev, int64_t w_session_stride,
                         const float* b_dev, int64_t b_session_stride, int64_t n, int64_t frames_before, int c,
                         int pre, int post, int width, int flush, void* state_dev, int64_t state_session_stride) {
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_calib_online_push: handle is NULL");
  TD_TRY(check_shape(h, "td_calib_online_push", c, pre, post));
  TD_TRY(check_calib_push(h, "td_calib_online_push", width, n, frames_before, num_sessions, state_dev,
                          state_session_stride, c, pre, post));
  if (!w_dev || !b_dev || (n > 0 && (!eeg_dev || !env_dev)))
    return td_fail(h, TD_ERR_INVALID, "td_calib_online_push: NULL argument");
  if (n > 0)
    TD_TRY(check_push_strides(h, "td_calib_online_push", num_sessions, eeg_ld, eeg_session_stride, c, env_ld,
                              env_session_stride, 2, "envelopes"));
  const int nl = pre + 1 + post;
  TD_TRY(check_fir_strides(h, "td_calib_online_push", w_session_stride, b_session_stride, nl * c));
  if (n == 0 && !flush) return TD_OK;
  const OnlinePlan pl = plan_push(frames_before, n, post, width, width, flush);   // (its windows: hop = width)
  CalibParams p;
  p.eeg = eeg_dev; p.eeg_ld = eeg_ld; p.eeg_ss = num_sessions > 1 ? eeg_session_stride : 0;
  p.env = env_dev; p.env_ld = env_ld; p.env_ss = num_sessions > 1 ? env_session_stride : 0;
  p.w = w_dev; p.w_ss = w_session_stride; p.b = b_dev; p.b_ss = b_session_stride;
  p.n = n; p.p0 = frames_before;
  p.e0 = pl.emitted_before; p.e1 = pl.emitted_after;
  p.c = c; p.pre = pre; p.post = post; p.width = width;
  const long long emitted_now = p.e1 - p.e0;
  p.pass = emitted_now < kPass ? (emitted_now > 1 ? (int)emitted_now : 1) : kPass;
  p.state = reinterpret_cast<unsigned char*>(state_dev); p.state_ss = state_session_stride;
  return launch_push(h, &h->lds_opt_online_calib, online_calib_push_kernel, num_sessions, kThreads,
                     lds_bytes(kMaxChannels, kMaxLags, kMaxLags - 1, kPass), lds_bytes(c, nl, post, p.pass),
                     (double)n * num_sessions, p);
}

int td_calib_online_sums(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride,
                         double* out_dev) {
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_calib_online_sums: handle is NULL");
  TD_TRY(check_state(h, "td_calib_online_sums", num_sessions, state_dev, state_session_stride, 8LL * kSums));
  if (!out_dev) return td_fail(h, TD_ERR_INVALID, "td_calib_online_sums: NULL argument");
  return launch_head_sums(h, num_sessions, state_dev, state_session_stride, kSums, out_dev);
}

int td_calib_online_finish(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride,
                           int64_t frames_emitted, int width, double* corr_dev, double* lda_dev, double* dprime_dev,
                           int32_t* status_dev) {
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_calib_online_finish: handle is NULL");
  TD_TRY(check_state(h, "td_calib_online_finish", num_sessions, state_dev, state_session_stride, 8LL * kSums));
  TD_REQUIRE(h, width >= 1 && width <= TD_ONLINE_MAX_WIDTH, "td_calib_online_finish: window of %d frames (1 .. %d)",
             width, TD_ONLINE_MAX_WIDTH);
  TD_REQUIRE(h, frames_emitted >= 0, "td_calib_online_finish: %lld frames emitted", (long long)frames_emitted);
  if (!corr_dev || !lda_dev || !dprime_dev || !status_dev)
    return td_fail(h, TD_ERR_INVALID, "td_calib_online_finish: NULL argument");
  TD_TRY(td_profile_mark(h, true, (double)num_sessions));
  hipLaunchKernelGGL(online_calib_finish_kernel, dim3((unsigned)td_ceil_div(num_sessions, kThreads)), dim3(kThreads),
                     0, h->stream, reinterpret_cast<const unsigned char*>(state_dev),
                     (long long)state_session_stride, num_sessions, (long long)frames_emitted, width, corr_dev,
                     lda_dev, dprime_dev, status_dev);
  TD_HIP(h, hipGetLastError());
  TD_TRY(td_profile_mark(h, false, 0.0));
  return TD_OK;
}

}  // extern "C"
