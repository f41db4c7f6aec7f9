// Online attention decode with a CCA model (td_cca_online_*): online.hip's session -- state on the device, one
// workgroup per listener, ONE launch per push -- with BrainModelCCA in front of the correlator instead of the FIR
// prediction.  Per emitted frame t the EEG view's lagged row is centred and rotated once,
//   a[d] = sum_k (x~_t[k] - mean_x[k]) rot_x[k][d],
// each speaker's lagged feature row likewise, b_s[d] = sum_k (y~_{s,t}[k] - mean_y[k]) rot_y[k][d], and from
// the projections on everything is what the existing kernels compute: frame_scores_kernel's expression over the
// `dims` columns, window_means_kernel's sum, decide_wta_kernel's / decide_step_kernel's decisions (windows.hip),
// online.hip's ring.
//
// Any cut of a recording into pushes gives the bits of one push: a projection is a float32 sum whose order
// depends on (lag, channel, d) alone -- lane q of a wave takes the terms k = q, q + 64, ... into four
// accumulators in turn, ((a0 + a1) + (a2 + a3)), then the 64-lane tree -- and the centring is one float32
// subtraction in front of each fused multiply-add (the reference's (x - mean) @ rot; no bias folding).
//
// The rotations live in LDS transposed, rot_s[d][k]: the 64 lanes of a wave read 64 consecutive words of one
// column, the same addresses modulo nothing -- no bank conflict whatever k1 is -- and the lagged row of a frame is
// contiguous in the staged rows (row f + l at (f + l) c + ch = f c + k), so x~, the mean and the rotation column
// are three unit-stride LDS streams.  No atomics, vector stores only.  The projection, the model's and the feature
// blocks' staging and the feature tails are online_cca_common.h's, shared with online_cca_calib.hip.
#include "online_cca_common.h"

namespace {

constexpr int kThreads = 1024;     // 16 waves: a pass of 64 frames is 192 (frame, view) projections
constexpr int kWaves = kThreads / 64;
constexpr int kWinThreads = 256;   // window_means_kernel's workgroup: a window mean keeps ITS order
constexpr int kMaxC1 = 128, kMaxC2 = 32, kMaxLags = 64, kMaxDims = 16;   // (kFirMaxD columns)
constexpr int kPass = 64;          // emitted frames per pass of a workgroup; halved until the LDS budget holds
constexpr long long kLdsBudget = TD_CCA_ONLINE_LDS_BYTES;

// One session's state block: [stepped state f64][ring f64 [2][width]][EEG tail f32 [pre1 + post][c1]]
// [feature tail f32 [2][pre2 + post][c2]], rounded up to 8 bytes; post = max(post1, post2).
__host__ __device__ inline long long state_feat_offset(int c1, int pre1, int post, int width) {
  return tail_end(state_eeg_offset(width), c1, pre1 + post);
}
__host__ __device__ inline long long state_bytes(int c1, int pre1, int c2, int pre2, int post, int width) {
  return tails_bytes(state_eeg_offset(width), c1, pre1 + post, 2LL * c2 * (pre2 + post));
}

// LDS of a launch: 8 (4 pass) for the pass's per-frame scores and window means, then float32: both means
// (k1 + k2), both rotations (dims (k1 + k2)), the staged rows (R1 c1 + 2 R2 c2) and the pass's projections
// (3 dims pass).
__host__ __device__ inline long long lds_bytes(int c1, int pre1, int post1, int c2, int pre2, int post2, int dims,
                                               int pass) {
  const int post = delay_of(post1, post2);
  const long long k1 = (long long)c1 * (pre1 + 1 + post1), k2 = (long long)c2 * (pre2 + 1 + post2);
  const long long r1 = stage_rows(pass, pre1, post1, post), r2 = stage_rows(pass, pre2, post2, post);
  return 32LL * pass + 4LL * ((dims + 1) * (k1 + k2) + r1 * c1 + 2 * r2 * c2 + 3LL * dims * pass);
}

// The largest pass (kPass halved, at least 1, no more than the frames to emit) whose LDS fits; 0: none does.
int pass_of(int c1, int pre1, int post1, int c2, int pre2, int post2, int dims, long long emitted_now) {
  int pass = emitted_now < kPass ? (emitted_now > 1 ? (int)emitted_now : 1) : kPass;
  while (pass > 1 && lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, pass) > kLdsBudget) pass = (pass + 1) / 2;
  return lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, pass) <= kLdsBudget ? pass : 0;
}

struct CcaOnlineParams {
  const float* eeg; long long eeg_ld, eeg_ss;
  const float* feat[2]; long long feat_ld, feat_ss;
  const float *mean_x, *rot_x, *mean_y, *rot_y; long long model_ss;   // 0 or 1 (models)
  const double* corr;            // [S][2][3][dims]
  const double* lda;             // [S][dims + 2] or null
  long long n, p0;               // rows of this push, rows pushed before it
  long long e0, e1;              // frames emitted before / after
  long long w0, n_win;           // first new window, new windows
  int c1, pre1, post1, c2, pre2, post2, dims, reduction, width, hop, decoder, pass;
  unsigned char* state; long long state_ss;
  double* scores; unsigned char* decisions; float* proj; double* frame;
};

// frame_scores_kernel's value (windows.hip) of one row: a = the EEG view's projection, b = a speaker's.  That
// kernel's operations one for one -- the column's value v, a plain add of v, of +-v v or of the PRODUCT v lda_w
// into a sum that starts at 0.0, then the division by the column count or ONE fused slope acc + intercept --
// with contraction switched off so that no other pair of them fuses here.
__device__ __forceinline__ double frame_score(const float* a, const float* b, const double* cr, int dims,
                                              int reduction, const double* lda) {
#pragma clang fp contract(off)
  if (reduction == 0 || reduction == 1) {
    const int c = reduction;
    return ((double)a[c] - cr[c]) * ((double)b[c] - cr[dims + c]) / cr[2 * dims + c];
  }
  double acc = 0.0;
  for (int c = 0; c < dims; ++c) {
    const double v = ((double)a[c] - cr[c]) * ((double)b[c] - cr[dims + c]) / cr[2 * dims + c];
    double term;
    if (reduction == 2) term = v;
    else if (reduction == 3) term = (v > 0.0 ? v * v : (v < 0.0 ? -v * v : 0.0));
    else term = v * lda[c];
    acc = acc + term;
  }
  if (reduction == 4) return fma(lda[dims], acc, lda[dims + 1]);
  return acc / (double)dims;
}

__global__ __launch_bounds__(kThreads) void cca_online_push_kernel(CcaOnlineParams p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x;
  const int c1 = p.c1, pre1 = p.pre1, post1 = p.post1, c2 = p.c2, pre2 = p.pre2, post2 = p.post2;
  const int dims = p.dims, width = p.width, hop = p.hop, pass = p.pass;
  const int post = delay_of(post1, post2);
  const int k1 = c1 * (pre1 + 1 + post1), k2 = c2 * (pre2 + 1 + post2);
  const int t1 = pre1 + post, t2 = pre2 + post;                 // rows of the tails
  const int r1 = stage_rows(pass, pre1, post1, post), r2 = stage_rows(pass, pre2, post2, post);
  double* sc_s = lds;                                           // [2][pass] the pass's per-frame scores
  double* wm_s = sc_s + 2 * pass;                               // [2][pass] the pass's window means
  float* mean1_s = reinterpret_cast<float*>(wm_s + 2 * pass);   // [k1]
  float* mean2_s = mean1_s + k1;                                // [k2]
  float* rot1_s = mean2_s + k2;                                 // [dims][k1]
  float* rot2_s = rot1_s + (size_t)dims * k1;                   // [dims][k2]
  float* rows1_s = rot2_s + (size_t)dims * k2;                  // [r1][c1] the pass's EEG rows
  float* rows2_s = rows1_s + (size_t)r1 * c1;                   // [2][r2][c2] the pass's feature rows
  float* proj_s = rows2_s + 2 * (size_t)r2 * c2;                // [pass][3 dims] a | b1 | b2

  unsigned char* st = p.state + (long long)s * p.state_ss;
  double* step_p = reinterpret_cast<double*>(st);
  double* ring = reinterpret_cast<double*>(st + state_ring_offset());                      // [2][width]
  float* tail1 = reinterpret_cast<float*>(st + state_eeg_offset(width));                   // [t1][c1]
  float* tail2 = reinterpret_cast<float*>(st + state_feat_offset(c1, pre1, post, width));  // [2][t2][c2]
  const float* eeg = p.eeg + (long long)s * p.eeg_ss;
  const float* feat[2] = {p.feat[0] + (long long)s * p.feat_ss, p.feat[1] + (long long)s * p.feat_ss};
  const long long ms = (long long)s * p.model_ss;
  const float* mean_x = p.mean_x + ms * k1;
  const float* rot_x = p.rot_x + ms * k1 * dims;
  const float* mean_y = p.mean_y + ms * k2;
  const float* rot_y = p.rot_y + ms * k2 * dims;
  const double* cr = p.corr + (long long)s * 6 * dims;
  const double* lda = p.lda ? p.lda + (long long)s * (dims + 2) : nullptr;
  const long long p0 = p.p0, p1 = p.p0 + p.n;
  const long long emitted_now = p.e1 - p.e0;

  // ---- the model: the means as they are, the rotations transposed (global [k][dims] -> LDS [dims][k])
  stage_model<kThreads>(mean1_s, mean2_s, rot1_s, rot2_s, mean_x, rot_x, mean_y, rot_y, k1, k2, dims);
  double step = load_step(step_p, p.decoder);

  for (long long a = p.e0; a < p.e1; a += pass) {
    const int nf = (int)(p.e1 - a < pass ? p.e1 - a : pass);     // frames [a, a + nf) of this pass
    // ---- stage the EEG rows a - pre1 .. a + nf - 1 + post1 and each speaker's feature rows a - pre2 ..
    // a + nf - 1 + post2: from the tails (rows before this push), from the push, zeros before the recording
    // and behind a flushed end
    stage_rows<kThreads>(rows1_s, c1, tail1, t1, eeg, p.eeg_ld, c1, a - pre1, nf + pre1 + post1, p0, p1);
    stage_feat<kThreads>(rows2_s, r2, tail2, t2, feat, p.feat_ld, c2, a - pre2, nf + pre2 + post2, p0, p1);
    __syncthreads();
    // ---- projections: a wave per (frame, view): the EEG view once, then each speaker's features
    for (int t = wave; t < 3 * nf; t += kWaves) {
      const int f = t / 3, part = t - 3 * f;
      float* out = proj_s + (size_t)f * 3 * dims + part * dims;
      if (part == 0) project_row(rows1_s + (size_t)f * c1, mean1_s, rot1_s, k1, dims, lane, out);
      else project_row(rows2_s + ((size_t)(part - 1) * r2 + f) * c2, mean2_s, rot2_s, k2, dims, lane, out);
    }
    __syncthreads();
    // ---- per-frame scores of both speakers
    for (int i = tid; i < 2 * nf; i += kThreads) {
      const int spk = i / nf, f = i - spk * nf;
      const float* pa = proj_s + (size_t)f * 3 * dims;
      const double v = frame_score(pa, pa + (1 + spk) * dims, cr + 3 * spk * dims, dims, p.reduction, lda);
      sc_s[spk * pass + f] = v;
      const long long at = (long long)s * emitted_now + (a - p.e0) + f;
      if (p.frame) p.frame[(long long)spk * gridDim.x * emitted_now + at] = v;
    }
    if (p.proj) {
      float* dst = p.proj + ((long long)s * emitted_now + (a - p.e0)) * 3 * dims;
      for (int i = tid; i < nf * 3 * dims; i += kThreads) dst[i] = proj_s[i];
    }
    __syncthreads();
    // ---- the windows that end in (a, a + nf], their decisions, the ring, then the next pass
    window_block<kThreads, kWinThreads>(sc_s, wm_s, ring, pass, a, nf, width, hop, p.decoder, step, p.w0, p.n_win,
                                        p.scores, p.decisions);
  }

  // ---- the tails for the next push: the last pre1 + post EEG rows and the last pre2 + post feature rows of
  // (old tail, this push).  A push shorter than a tail shifts it: the rows that stay go through LDS.
  __syncthreads();
  const long long n = p.n;
  tail_park<kThreads>(rows1_s, tail1, t1, c1, n);
  feat_tail_park<kThreads>(rows2_s, r2, tail2, t2, c2, n);
  __syncthreads();
  tail_store<kThreads>(tail1, rows1_s, t1, c1, eeg, p.eeg_ld, n);
  feat_tail_store<kThreads>(tail2, rows2_s, r2, t2, c2, feat, p.feat_ld, n);
  store_step(step_p, p.decoder, step);
}

// The shape checks td_cca_online_state_bytes, td_cca_online_lds_bytes and td_cca_online_push share.
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

int td_cca_online_state_bytes(int c1, int pre1, int post1, int c2, int pre2, int post2, int width,
                              int64_t* bytes) {
  if (!bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_cca_online_state_bytes: NULL argument");
  // (the state does not depend on dims: the LDS budget is checked for the least a model can have, one)
  TD_TRY(check_shape(nullptr, "td_cca_online_state_bytes", c1, pre1, post1, c2, pre2, post2, 1, width));
  *bytes = state_bytes(c1, pre1, c2, pre2, delay_of(post1, post2), width);
  return TD_OK;
}

int td_cca_online_lds_bytes(int c1, int pre1, int post1, int c2, int pre2, int post2, int dims,
                            int64_t emitted, int* pass, int64_t* bytes) {
  if (!pass || !bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_cca_online_lds_bytes: NULL argument");
  TD_TRY(check_shape(nullptr, "td_cca_online_lds_bytes", c1, pre1, post1, c2, pre2, post2, dims, 1));
  TD_REQUIRE(nullptr, emitted >= 0, "td_cca_online_lds_bytes: %lld frames", (long long)emitted);
  *pass = pass_of(c1, pre1, post1, c2, pre2, post2, dims, emitted);
  *bytes = lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, *pass);
  return TD_OK;
}

int td_cca_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t eeg_ld,
                       int64_t eeg_session_stride, const float* feat1_dev, const float* feat2_dev,
                       int64_t feat_ld, int64_t feat_session_stride, int64_t n, int c1, int pre1, int post1,
                       int c2, int pre2, int post2, int dims, const float* mean_x_dev, const float* rot_x_dev,
                       const float* mean_y_dev, const float* rot_y_dev, int64_t model_session_stride,
                       const double* corr_dev, int reduction, const double* lda_dev, int width, int hop,
                       int decoder, int64_t frames_before, int flush, void* state_dev,
                       int64_t state_session_stride, double* scores_dev, uint8_t* decisions_dev,
                       float* proj_dev, double* frame_dev) {
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_cca_online_push: handle is NULL");
  TD_REQUIRE(h, num_sessions >= 1, "td_cca_online_push: %d sessions", num_sessions);
  TD_TRY(check_shape(h, "td_cca_online_push", c1, pre1, post1, c2, pre2, post2, dims, width));
  TD_TRY(check_push_args(h, "td_cca_online_push", n, width, hop, reduction, dims, lda_dev, decoder, frames_before));
  if (!mean_x_dev || !rot_x_dev || !mean_y_dev || !rot_y_dev || !corr_dev || !state_dev || !scores_dev ||
      !decisions_dev || (n > 0 && (!eeg_dev || !feat1_dev || !feat2_dev)))
    return td_fail(h, TD_ERR_INVALID, "td_cca_online_push: NULL argument");
  TD_TRY(check_push_strides(h, "td_cca_online_push", num_sessions, eeg_ld, eeg_session_stride, c1, feat_ld,
                            feat_session_stride, c2, "features"));
  TD_REQUIRE(h, model_session_stride == 0 || model_session_stride == 1,
             "td_cca_online_push: a model stride of %lld models (0 = one model, 1 = one per session)",
             (long long)model_session_stride);
  const int post = delay_of(post1, post2);
  TD_TRY(check_state_stride(h, "td_cca_online_push", state_session_stride,
                            state_bytes(c1, pre1, c2, pre2, post, width)));
  if (n == 0 && !flush) return TD_OK;
  const OnlinePlan pl = plan_push(frames_before, n, post, width, hop, flush);
  const long long e0 = pl.emitted_before, e1 = pl.emitted_after, w0 = pl.first_window, n_win = pl.new_windows;
  CcaOnlineParams p;
  p.eeg = eeg_dev; p.eeg_ld = eeg_ld; p.eeg_ss = num_sessions > 1 ? eeg_session_stride : 0;
  p.feat[0] = feat1_dev; p.feat[1] = feat2_dev; p.feat_ld = feat_ld;
  p.feat_ss = num_sessions > 1 ? feat_session_stride : 0;
  p.mean_x = mean_x_dev; p.rot_x = rot_x_dev; p.mean_y = mean_y_dev; p.rot_y = rot_y_dev;
  p.model_ss = model_session_stride;
  p.corr = corr_dev; p.lda = reduction == 4 ? lda_dev : nullptr;
  p.n = n; p.p0 = frames_before; p.e0 = e0; p.e1 = e1; p.w0 = w0; p.n_win = n_win;
  p.c1 = c1; p.pre1 = pre1; p.post1 = post1; p.c2 = c2; p.pre2 = pre2; p.post2 = post2; p.dims = dims;
  p.reduction = reduction; p.width = width; p.hop = hop; p.decoder = decoder;
  p.pass = pass_of(c1, pre1, post1, c2, pre2, post2, dims, e1 - e0);     // (>= 1: check_shape)
  p.state = reinterpret_cast<unsigned char*>(state_dev); p.state_ss = state_session_stride;
  p.scores = scores_dev; p.decisions = decisions_dev; p.proj = proj_dev; p.frame = frame_dev;
  return launch_push(h, &h->lds_opt_online_cca, cca_online_push_kernel, num_sessions, kThreads, kLdsBudget,
                     lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, p.pass), (double)n * num_sessions, p);
}

}  // extern "C"
