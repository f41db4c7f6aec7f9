// Online attention decode (td_online_*): the chain of td_decode_fused -- FIR prediction, global-statistics
// correlation against two envelopes, window means, decision -- for EEG that arrives in chunks.  A bank of
// independent sessions, one workgroup each; everything a session carries from push to push (the last
// pre + post EEG rows, the last post envelope rows, a ring of the last `width` per-frame scores, the
// stepped decoder's state) lives in its state block on the device, and ONE launch advances the bank by a
// push.  The host counts the frames; the block holds data only.
//
// Any cut of a recording into pushes gives the bits of one push: the prediction's float32 sum has an order
// that depends on (lag, channel) alone, the per-frame score is frame_scores_kernel's expression, a window
// mean is window_means_kernel's sum (256 threads stride the window, 64-lane wave sums, ((w0 + w1) +
// (w2 + w3)) / width) and the decisions are decide_wta_kernel's / decide_step_kernel's operations
// (windows.hip).  No atomics.
#include "online_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxChannels = 128, kMaxLags = 64;
constexpr int kPass = 64;       // emitted frames per pass of a workgroup (fewer for a short push: less LDS)

// One session's state block (online_common.h): [stepped state f64][ring f64 [2][width]][EEG tail f32 [pre + post][c]]
// [envelope tail f32 [post][2]], rounded up to 8 bytes.

struct OnlineParams {
  const float* eeg; long long eeg_ld, eeg_ss;
  const float* env; long long env_ld, env_ss;
  const float* w; long long w_ss;
  const float* b; long long b_ss;
  const double* corr;            // [S][2][3]
  const double* lda;             // [S][3] or null
  long long n, p0;               // rows of this push, rows pushed before it
  long long e0, e1;              // frames emitted before / after
  long long w0, n_win;           // first new window, new windows
  int c, pre, post, reduction, width, hop, decoder, pass;
  unsigned char* state; long long state_ss;
  double* scores; unsigned char* decisions; float* pred; double* frame;
};

__global__ __launch_bounds__(kThreads) void online_push_kernel(OnlineParams p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x;
  const int c = p.c, pre = p.pre, post = p.post, width = p.width, hop = p.hop;
  const int tl = pre + post, nl = tl + 1, k_all = nl * c, pass = p.pass;
  double* sc_s = lds;                                        // [2][pass] the pass's per-frame scores
  double* wm_s = sc_s + 2 * pass;                            // [2][pass] the pass's window means
  float* w_s = reinterpret_cast<float*>(wm_s + 2 * pass);    // [nl c] the weights
  float* rows_s = w_s + k_all;                               // [pass + tl][c] the pass's EEG rows
  float* env_s = rows_s + (size_t)(pass + tl) * c;           // [max(pass, post)][2]
  float* pred_s = env_s + 2 * (pass > post ? pass : post);   // [pass]

  unsigned char* st = p.state + (long long)s * p.state_ss;
  double* step_p = reinterpret_cast<double*>(st);
  double* ring = reinterpret_cast<double*>(st + state_ring_offset());             // [2][width]
  float* tail = reinterpret_cast<float*>(st + state_eeg_offset(width));           // [tl][c]
  float* etail = reinterpret_cast<float*>(st + state_env_offset(c, pre, post, width));   // [post][2]
  const float* eeg = p.eeg + (long long)s * p.eeg_ss;
  const float* env = p.env + (long long)s * p.env_ss;
  const float* w = p.w + (long long)s * p.w_ss;
  const float bias = p.b[(long long)s * p.b_ss];
  const double* cr = p.corr + (long long)s * 6;
  const double lda_w = p.lda ? p.lda[s * 3LL] : 0.0, lda_slope = p.lda ? p.lda[s * 3LL + 1] : 1.0,
               lda_icpt = p.lda ? p.lda[s * 3LL + 2] : 0.0;
  const long long p0 = p.p0, p1 = p.p0 + p.n;
  const long long emitted_now = p.e1 - p.e0;

  for (int k = tid; k < k_all; k += kThreads) w_s[k] = w[k];
  double step = load_step(step_p, p.decoder);

  for (long long a = p.e0; a < p.e1; a += pass) {
    const int nf = (int)(p.e1 - a < pass ? p.e1 - a : pass);     // frames [a, a + nf) of this pass
    // ---- stage the EEG rows a - pre .. a + nf - 1 + post and the envelope rows a .. a + nf - 1
    stage_rows<kThreads>(rows_s, c, tail, tl, eeg, p.eeg_ld, c, a - pre, nf + tl, p0, p1);
    stage_env<kThreads>(env_s, etail, post, env, p.env_ld, a, nf, p0);
    __syncthreads();
    // ---- predictions: a wave per frame
    for (int f = wave; f < nf; f += kWaves) {
      const float pr = fir_predict(w_s, rows_s + f * c, k_all, bias);
      if (lane == 0) pred_s[f] = pr;
    }
    __syncthreads();
    // ---- per-frame scores of both speakers
    for (int i = tid; i < 2 * nf; i += kThreads) {
      const int spk = i / nf, f = i - spk * nf;
      const float pr = pred_s[f];
      const double v = frame_score(env_s[2 * f + spk], pr, cr[3 * spk], cr[3 * spk + 1], cr[3 * spk + 2],
                                   p.reduction, lda_w, lda_slope, lda_icpt);
      sc_s[spk * pass + f] = v;
      const long long at = (long long)s * emitted_now + (a - p.e0) + f;
      if (p.frame) p.frame[(long long)spk * gridDim.x * emitted_now + at] = v;
      if (p.pred && spk == 0) p.pred[at] = pr;
    }
    __syncthreads();
    // ---- the windows that end in (a, a + nf], their decisions, the ring, then the next pass
    window_block<kThreads, kThreads>(sc_s, wm_s, ring, pass, a, nf, width, hop, p.decoder, step, p.w0, p.n_win,
                                     p.scores, p.decisions);
  }

  // ---- the tails for the next push: the last pre + post EEG rows and the last post envelope rows
  __syncthreads();
  tail_park<kThreads>(rows_s, tail, tl, c, p.n);
  env_tail_park<kThreads>(env_s, etail, post, p.n);
  __syncthreads();
  tail_store<kThreads>(tail, rows_s, tl, c, eeg, p.eeg_ld, p.n);
  env_tail_store<kThreads>(etail, env_s, post, env, p.env_ld, p.n);
  store_step(step_p, p.decoder, step);
}

size_t lds_bytes(int c, int nl, int post, int pass) {
  const size_t env_rows = pass > post ? pass : post;
  return sizeof(double) * 4 * pass +
         sizeof(float) * ((size_t)nl * c + (size_t)(pass + nl - 1) * c + 2 * env_rows + (size_t)pass);
}

}  // namespace

extern "C" {

int td_online_state_bytes(int c, int pre, int post, int width, int64_t* bytes) {
  if (!bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_online_state_bytes: NULL argument");
  TD_TRY(check_context(nullptr, "td_online_state_bytes", c, pre, post, kMaxChannels, kMaxLags));
  TD_REQUIRE(nullptr, width >= 1 && width <= TD_ONLINE_MAX_WIDTH,
             "td_online_state_bytes: window of %d frames (1 .. %d)", width, TD_ONLINE_MAX_WIDTH);
  *bytes = state_bytes(c, pre, post, width);
  return TD_OK;
}

int td_online_plan(int64_t frames_before, int64_t n, int post, int width, int hop, int flush,
                   int64_t* emitted_before, int64_t* emitted_after, int64_t* first_window,
                   int64_t* new_windows) {
  TD_REQUIRE(nullptr, frames_before >= 0 && n >= 0 && post >= 0 && width >= 1 && hop >= 1,
             "td_online_plan: %lld frames before, %lld frames, post %d, windows of %d every %d",
             (long long)frames_before, (long long)n, post, width, hop);
  const OnlinePlan pl = plan_push(frames_before, n, post, width, hop, flush);
  if (emitted_before) *emitted_before = pl.emitted_before;
  if (emitted_after) *emitted_after = pl.emitted_after;
  if (first_window) *first_window = pl.first_window;
  if (new_windows) *new_windows = pl.new_windows;
  return TD_OK;
}

int td_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t eeg_ld,
                   int64_t eeg_session_stride, const float* env_dev, int64_t env_ld,
                   int64_t env_session_stride, int64_t n, int c, int pre, int post,
                   const float* w_dev, int64_t w_session_stride, const float* b_dev,
                   int64_t b_session_stride, const double* corr_dev, int reduction,
                   const double* lda_dev, int width, int hop, int decoder, int64_t frames_before,
                   int flush, void* state_dev, int64_t state_session_stride, double* scores_dev,
                   uint8_t* decisions_dev, float* pred_dev, double* frame_dev) {
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_online_push: handle is NULL");
  TD_REQUIRE(h, num_sessions >= 1, "td_online_push: %d sessions", num_sessions);
  TD_TRY(check_context(h, "td_online_push", c, pre, post, kMaxChannels, kMaxLags));
  TD_TRY(check_push_args(h, "td_online_push", n, width, hop, reduction, 0, lda_dev, decoder, frames_before));
  if (!w_dev || !b_dev || !corr_dev || !state_dev || !scores_dev || !decisions_dev || (n > 0 && (!eeg_dev || !env_dev)))
    return td_fail(h, TD_ERR_INVALID, "td_online_push: NULL argument");
  TD_TRY(check_push_strides(h, "td_online_push", num_sessions, eeg_ld, eeg_session_stride, c, env_ld,
                            env_session_stride, 2, "envelopes"));
  const int nl = pre + 1 + post;
  TD_TRY(check_fir_strides(h, "td_online_push", w_session_stride, b_session_stride, nl * c));
  TD_TRY(check_state_stride(h, "td_online_push", state_session_stride, state_bytes(c, pre, post, width)));
  if (n == 0 && !flush) return TD_OK;
  const OnlinePlan pl = plan_push(frames_before, n, post, width, hop, flush);
  OnlineParams p;
  p.eeg = eeg_dev; p.eeg_ld = eeg_ld; p.eeg_ss = num_sessions > 1 ? eeg_session_stride : 0;
  p.env = env_dev; p.env_ld = env_ld; p.env_ss = num_sessions > 1 ? env_session_stride : 0;
  p.w = w_dev; p.w_ss = w_session_stride; p.b = b_dev; p.b_ss = b_session_stride;
  p.corr = corr_dev; p.lda = reduction == 4 ? lda_dev : nullptr;
  p.n = n; p.p0 = frames_before; p.e0 = pl.emitted_before; p.e1 = pl.emitted_after;
  p.w0 = pl.first_window; p.n_win = pl.new_windows;
  p.c = c; p.pre = pre; p.post = post; p.reduction = reduction; p.width = width; p.hop = hop; p.decoder = decoder;
  const long long emitted_now = pl.emitted_after - pl.emitted_before;
  p.pass = emitted_now < kPass ? (emitted_now > 1 ? (int)emitted_now : 1) : kPass;
  p.state = reinterpret_cast<unsigned char*>(state_dev); p.state_ss = state_session_stride;
  p.scores = scores_dev; p.decisions = decisions_dev; p.pred = pred_dev; p.frame = frame_dev;
  return launch_push(h, &h->lds_opt_online, online_push_kernel, num_sessions, kThreads,
                     lds_bytes(kMaxChannels, kMaxLags, kMaxLags - 1, kPass), lds_bytes(c, nl, post, p.pass),
                     (double)n * num_sessions, p);
}

}  // extern "C"
