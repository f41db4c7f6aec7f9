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
#include "td_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxChannels = 128, kMaxLags = 64;
constexpr int kPass = 64;       // emitted frames per pass of a workgroup (fewer for a short push: less LDS)

// One session's state block: [stepped state f64][ring f64 [2][width]][EEG tail f32 [pre + post][c]]
// [envelope tail f32 [post][2]], rounded up to 8 bytes.
__host__ __device__ inline long long state_ring_offset() { return 8; }
__host__ __device__ inline long long state_eeg_offset(int width) { return 8 + 16LL * width; }
__host__ __device__ inline long long state_env_offset(int c, int pre, int post, int width) {
  return state_eeg_offset(width) + 4LL * c * (pre + post);
}
__host__ __device__ inline long long state_bytes(int c, int pre, int post, int width) {
  return (state_env_offset(c, pre, post, width) + 8LL * post + 7) / 8 * 8;
}

long long windows_of(long long frames, int width, int hop) {      // td_window_count of one trial
  return frames >= width ? (frames - width) / hop + 1 : 0;
}

struct OnlinePlan {
  long long emitted_before, emitted_after, first_window, new_windows;
};

OnlinePlan plan_push(long long frames_before, long long n, int post, int width, int hop, int flush) {
  OnlinePlan pl;
  const long long pushed = frames_before + n;
  pl.emitted_before = frames_before > post ? frames_before - post : 0;
  pl.emitted_after = flush ? pushed : (pushed > post ? pushed - post : 0);
  pl.first_window = windows_of(pl.emitted_before, width, hop);
  pl.new_windows = windows_of(pl.emitted_after, width, hop) - pl.first_window;
  return pl;
}

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

// (windows.hip's wave_sum: the same shuffle tree, the same bits)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// frame_scores_kernel's value for ONE column (windows.hip): a = the truth, b = the prediction.  The sums
// over the columns start from 0.0 there, so they do here; the lda map is that kernel's one fused
// multiply-add (slope * acc + intercept, contracted).
__device__ __forceinline__ double frame_score(float truth, float pred, double mean_a, double mean_b,
                                              double power, int reduction, double lda_w,
                                              double lda_slope, double lda_intercept) {
  const double v = ((double)truth - mean_a) * ((double)pred - mean_b) / power;
  if (reduction == 0) return v;
  double acc = 0.0;
  if (reduction == 2) {
    acc += v;
  } else if (reduction == 3) {
    acc += (v > 0.0 ? v * v : (v < 0.0 ? -v * v : 0.0));
  } else {
    acc += v * lda_w;
    acc = fma(lda_slope, acc, lda_intercept);
  }
  return acc;
}

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
  double step = 0.5;
  if (tid == 0 && p.decoder == 1) {
    const double stored = *step_p;
    step = stored == 0.0 ? 0.5 : stored;
  }

  for (long long a = p.e0; a < p.e1; a += pass) {
    const int nf = (int)(p.e1 - a < pass ? p.e1 - a : pass);     // frames [a, a + nf) of this pass
    // ---- stage the EEG rows a - pre .. a + nf - 1 + post and the envelope rows a .. a + nf - 1: from the
    // tails (rows before this push), from the push, zeros before the recording and behind a flushed end
    const int n_rows = nf + tl;
    for (int rr = wave; rr < n_rows; rr += kWaves) {
      const long long row = a - pre + rr;
      for (int ch = lane; ch < c; ch += 64) {
        float v = 0.f;
        if (row >= 0 && row < p0) v = tail[(row - (p0 - tl)) * c + ch];
        else if (row >= p0 && row < p1) v = eeg[(row - p0) * p.eeg_ld + ch];
        rows_s[rr * c + ch] = v;
      }
    }
    for (int i = tid; i < 2 * nf; i += kThreads) {
      const long long row = a + (i >> 1);
      env_s[i] = row < p0 ? etail[(row - (p0 - post)) * 2 + (i & 1)] : env[(row - p0) * p.env_ld + (i & 1)];
    }
    __syncthreads();
    // ---- predictions: a wave per frame; lane q takes the terms k = q, q + 64, ... of the (lag, channel)
    // sum into four accumulators in turn, ((a0 + a1) + (a2 + a3)), then the 64-lane tree, then the bias
    for (int f = wave; f < nf; f += kWaves) {
      const float* xr = rows_s + f * c;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int k = lane;
      for (; k + 192 < k_all; k += 256) {
        a0 = fmaf(w_s[k], xr[k], a0);
        a1 = fmaf(w_s[k + 64], xr[k + 64], a1);
        a2 = fmaf(w_s[k + 128], xr[k + 128], a2);
        a3 = fmaf(w_s[k + 192], xr[k + 192], a3);
      }
      if (k < k_all) a0 = fmaf(w_s[k], xr[k], a0);
      if (k + 64 < k_all) a1 = fmaf(w_s[k + 64], xr[k + 64], a1);
      if (k + 128 < k_all) a2 = fmaf(w_s[k + 128], xr[k + 128], a2);
      const float total = wave_sum_f32((a0 + a1) + (a2 + a3));
      if (lane == 0) pred_s[f] = total + bias;
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
    // ---- the windows that end in (a, a + nf]: window wi = frames [wi hop, wi hop + width).  A WAVE forms a
    // window's mean with window_means_kernel's operations: lane q stands in for the threads q, q + 64,
    // q + 128, q + 192 of that kernel's workgroup (four partial sums, four wave sums).  Frames before
    // `a` come from the ring, which holds the `width` frames before `a` until this pass has stored its own.
    const long long end_lo = a + 1 > width ? a + 1 : width;      // the first window end in reach
    const long long wi_lo = (end_lo - width + hop - 1) / hop;
    const long long wi_hi = a + nf >= width ? (a + nf - width) / hop + 1 : 0;   // one past the last
    const int nw = wi_hi > wi_lo ? (int)(wi_hi - wi_lo) : 0;
    for (int j = wave; j < nw; j += kWaves) {
      const long long r0 = (wi_lo + j) * hop;
      const int slot0 = (int)(r0 % width);                       // ring slot of the window's first frame
#pragma unroll
      for (int spk = 0; spk < 2; ++spk) {
        double part[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          double acc = 0.0;
          for (int r = 64 * q + lane; r < width; r += kThreads) {
            const long long fr = r0 + r;
            const int slot = slot0 + r - (slot0 + r >= width ? width : 0);
            acc += fr >= a ? sc_s[spk * pass + (int)(fr - a)] : ring[(long long)spk * width + slot];
          }
          part[q] = wave_sum(acc);
        }
        if (lane == 0) {
          const double m = ((part[0] + part[1]) + (part[2] + part[3])) / (double)width;
          wm_s[spk * pass + j] = m;
          p.scores[((long long)spk * gridDim.x + s) * p.n_win + (wi_lo + j - p.w0)] = m;
        }
      }
    }
    __syncthreads();
    // ---- decisions (decide_wta_kernel / decide_step_kernel), the ring, then the next pass
    unsigned char* dec = p.decisions + (long long)s * p.n_win + (wi_lo - p.w0);
    if (p.decoder == 1) {
      if (tid == 0) {
        for (int j = 0; j < nw; ++j) {
          if (wm_s[j] > wm_s[pass + j]) step = fmin(0.9, step + 0.1);
          else step = fmax(0.1, step - 0.1);
          dec[j] = step > 0.5 ? 1 : 0;
        }
      }
    } else {
      for (int j = tid; j < nw; j += kThreads)
        dec[j] = p.decoder == 0 ? (wm_s[j] > wm_s[pass + j] ? 1 : 0) : 0;
    }
    // (a pass longer than the ring: only its last `width` frames, one per slot)
    const int slot_a = (int)(a % width);
    for (int i = tid; i < 2 * nf; i += kThreads) {
      const int spk = i / nf, f = i - spk * nf;
      if (nf - f <= width) ring[(long long)spk * width + (slot_a + f) % width] = sc_s[spk * pass + f];
    }
    __threadfence_block();
    __syncthreads();
  }

  // ---- the tails for the next push: the last pre + post EEG rows and the last post envelope rows of
  // (old tail, this push).  A push shorter than a tail shifts it: the rows that stay go through LDS.
  __syncthreads();
  const long long n = p.n;
  const int keep = n < tl ? (int)(tl - n) : 0;                   // old EEG rows that stay
  for (int i = tid; i < keep * c; i += kThreads) rows_s[i] = tail[(tl - keep) * c + i];
  const int ekeep = n < post ? (int)(post - n) : 0;
  for (int i = tid; i < ekeep * 2; i += kThreads) env_s[i] = etail[(post - ekeep) * 2 + i];
  __syncthreads();
  for (int rr = wave; rr < tl; rr += kWaves)
    for (int ch = lane; ch < c; ch += 64)
      tail[rr * c + ch] = rr < keep ? rows_s[rr * c + ch] : eeg[(n - (tl - rr)) * p.eeg_ld + ch];
  for (int i = tid; i < post * 2; i += kThreads) {
    const int rr = i >> 1;
    etail[i] = rr < ekeep ? env_s[i] : env[(n - (post - rr)) * p.env_ld + (i & 1)];
  }
  if (tid == 0 && p.decoder == 1) *step_p = step;
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
  TD_REQUIRE(nullptr, c >= 1 && c <= kMaxChannels, "td_online_state_bytes: %d channels (1 .. %d)", c, kMaxChannels);
  TD_REQUIRE(nullptr, pre >= 0 && post >= 0 && pre + 1 + post <= kMaxLags,
             "td_online_state_bytes: context of %d + 1 + %d frames (at most %d lags)", pre, post, kMaxLags);
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
  TD_REQUIRE(h, c >= 1 && c <= kMaxChannels, "td_online_push: %d channels (1 .. %d)", c, kMaxChannels);
  TD_REQUIRE(h, pre >= 0 && post >= 0 && pre + 1 + post <= kMaxLags,
             "td_online_push: context of %d + 1 + %d frames (at most %d lags)", pre, post, kMaxLags);
  TD_REQUIRE(h, n >= 0 && n <= TD_ONLINE_MAX_PUSH, "td_online_push: %lld frames in one push (0 .. %d)",
             (long long)n, TD_ONLINE_MAX_PUSH);
  TD_REQUIRE(h, width >= 1 && width <= TD_ONLINE_MAX_WIDTH, "td_online_push: window of %d frames (1 .. %d)",
             width, TD_ONLINE_MAX_WIDTH);
  TD_REQUIRE(h, hop >= 1, "td_online_push: window step of %d frames", hop);
  TD_REQUIRE(h, reduction == 0 || reduction == 2 || reduction == 3 || reduction == 4,
             "td_online_push: reduction %d (0 first, 2 mean, 3 mean-squared, 4 lda)", reduction);
  TD_REQUIRE(h, reduction != 4 || lda_dev, "td_online_push: the lda reduction needs lda_dev");
  TD_REQUIRE(h, decoder >= 0 && decoder <= 2, "td_online_push: decoder %d (0 winner-take-all, 1 stepped, 2 none)",
             decoder);
  TD_REQUIRE(h, frames_before >= 0, "td_online_push: %lld frames before", (long long)frames_before);
  if (!w_dev || !b_dev || !corr_dev || !state_dev || !scores_dev || !decisions_dev || (n > 0 && (!eeg_dev || !env_dev)))
    return td_fail(h, TD_ERR_INVALID, "td_online_push: NULL argument");
  TD_REQUIRE(h, eeg_ld >= c && env_ld >= 2, "td_online_push: a row stride below a row (%lld for %d channels, %lld for 2 envelopes)",
             (long long)eeg_ld, c, (long long)env_ld);
  TD_REQUIRE(h, num_sessions == 1 || (eeg_session_stride >= c && env_session_stride >= 2),
             "td_online_push: a session stride below a row");
  const int nl = pre + 1 + post;
  TD_REQUIRE(h, w_session_stride == 0 || w_session_stride >= (int64_t)nl * c,
             "td_online_push: a weight stride of %lld for %d weights (0 = one model)", (long long)w_session_stride, nl * c);
  TD_REQUIRE(h, b_session_stride == 0 || b_session_stride >= 1, "td_online_push: a bias stride of %lld",
             (long long)b_session_stride);
  const long long sbytes = state_bytes(c, pre, post, width);
  TD_REQUIRE(h, state_session_stride >= sbytes && state_session_stride % 8 == 0,
             "td_online_push: a state stride of %lld bytes (a multiple of 8, at least %lld)",
             (long long)state_session_stride, sbytes);
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
  if (!h->lds_opt_online) {
    TD_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&online_push_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes(kMaxChannels, kMaxLags, kMaxLags - 1, kPass)));
    h->lds_opt_online = true;
  }
  TD_TRY(td_profile_mark(h, true, (double)n * num_sessions));
  hipLaunchKernelGGL(online_push_kernel, dim3((unsigned)num_sessions), dim3(kThreads), lds_bytes(c, nl, post, p.pass),
                     h->stream, p);
  TD_HIP(h, hipGetLastError());
  TD_TRY(td_profile_mark(h, false, 0.0));
  return TD_OK;
}

}  // extern "C"
