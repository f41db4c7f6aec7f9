// Online attention decode with a fully connected regressor (td_fc_online_*): online.hip's session -- state on the
// device, one workgroup per listener, ONE launch per push -- with brain_model.BrainModelDNN in front of the
// correlator instead of the FIR prediction.  The state block is online.hip's (td_online_state_bytes, td_online_plan
// serve as they are), and everything around the prediction is online_common.h's, as in online_push_kernel: the
// staging, frame_scores_kernel's expression, the ring, window_means_kernel's sum (256 threads stride the window,
// 64-lane wave sums, ((w0 + w1) + (w2 + w3)) / width), decide_wta_kernel's / decide_step_kernel's decisions
// (windows.hip), the tail update.
//
// The prediction of an emitted frame has td_mlp_forward's bits (mlp.hip).  Only the order within each sum is the
// contract:
//   slice partial  fmaf(x, w, s) from 0.f over the slice's rows of W1 in order; ks = min(64, round_up(ceil(K / 64), 4))
//                  rows a slice (mlp_check_and_plan's rule);
//   z1[j]          (0.f + the slice partials added in slice order) + b1[j];
//   ReLU           s <= 0.f ? 0.f : s, only when a layer follows;
//   later layers   an fmaf chain over the inputs in order from 0.f, then + b, then ReLU except on the last.
// Every sum belongs to one frame, so no sum depends on where a frame falls in a push: any cut of a recording into
// pushes gives the bits of one push.  No atomics, vector stores only.
//
// The mapping of sums to threads is this file's own.  A thread owns one frame and up to four groups of 4 columns of
// W1 -- one read of x feeds up to 16 fused multiply-adds -- and keeps their accumulators in registers across the
// slices; the threads of a pass of nf frames are laid frame-fastest over the workgroup (thread = frame + nf x column
// lane), so a push of 10 frames into 64 units is 160 busy threads, and the lanes of a wave read few distinct rows of
// W1 (broadcast) and distinct frames.  W1 (up to 2 MB) never fits in LDS: it is
// streamed in chunks of whole slices (at most 4096 floats), global -> registers -> LDS, double-buffered -- the
// loads of chunk i + 1 are in flight while chunk i is multiplied, one barrier a chunk -- with 16-byte loads along
// W1's rows when the layer's width is a multiple of 4 (the chunk is then one contiguous span).  The staged EEG rows
// hold every frame's lagged vector as the span that starts at its first row; their row stride is odd (c | 1), so
// the frames of a half-wave sit on 32 different banks.  The small parameters (b1, W2, b2, ...) are staged once per
// launch; the activations of a pass live in two LDS buffers with an odd row stride.
//
// The network's shape, the LDS of a launch, the shape checks and layer 1's device functions (chunk_load, chunk_store,
// slice_fma) are online_dnn_common.h's, and the forward of a pass -- the layer-1 driver and the later-layers loop --
// is the text of online_dnn_forward_body.h, both shared with online_dnn_calib.hip; this kernel's code is what it was
// with them in this file (DESIGN.md sections 45 and 47).
#include "online_dnn_common.h"

namespace {

constexpr int kWaves = kThreads / 64;

struct DnnOnlineParams {
  const float* eeg; long long eeg_ld, eeg_ss;
  const float* env; long long env_ld, env_ss;
  const float* params; long long params_ss;
  const double* corr;            // [S][2][3]
  const double* lda;             // [S][3] or null
  long long n, p0;               // rows of this push, rows pushed before it
  long long e0, e1;              // frames emitted before / after
  long long w0, n_win;           // first new window, new windows
  int c, pre, post, reduction, width, hop, decoder, pass;
  DnnNet net;
  unsigned char* state; long long state_ss;
  double* scores; unsigned char* decisions; float* pred; double* frame;
};

__global__ __launch_bounds__(kThreads) void dnn_online_push_kernel(DnnOnlineParams p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x;
  const int c = p.c, pre = p.pre, post = p.post, width = p.width, hop = p.hop;
  const int tl = pre + post, pass = p.pass, ldr = row_stride(c);
  const DnnNet& t = p.net;
  const int nl = t.nl, w1 = t.w[1], w1q = t.nj / 4, nj = t.nj, ks = t.ks, lda_s = t.lda, k_all = t.w[0];
  const int chunk_floats = t.g * ks * nj;
  double* sc_s = lds;                                        // [2][pass] the pass's per-frame scores
  double* wm_s = sc_s + 2 * pass;                            // [2][pass] the pass's window means
  float* ws_s = reinterpret_cast<float*>(wm_s + 2 * pass);   // [2][chunk_floats] chunks of W1 (16-byte aligned)
  float* sm_s = ws_s + 2 * chunk_floats;                     // [n_small] b1, W2, b2, ...
  float* rows_s = sm_s + (t.n_small + 3) / 4 * 4;            // [pass + tl][ldr] the pass's EEG rows
  float* env_s = rows_s + (size_t)(pass + tl) * ldr;         // [max(pass, post)][2]
  float* pred_s = env_s + 2 * (pass > post ? pass : post);   // [pass]
  float* act_s = pred_s + pass;                              // [2][pass][lda_s] activations, in turn

  unsigned char* st = p.state + (long long)s * p.state_ss;
  double* step_p = reinterpret_cast<double*>(st);
  double* ring = reinterpret_cast<double*>(st + state_ring_offset());             // [2][width]
  float* tail = reinterpret_cast<float*>(st + state_eeg_offset(width));           // [tl][c]
  float* etail = reinterpret_cast<float*>(st + state_env_offset(c, pre, post, width));   // [post][2]
  const float* eeg = p.eeg + (long long)s * p.eeg_ss;
  const float* env = p.env + (long long)s * p.env_ss;
  const float* prm = p.params + (long long)s * p.params_ss;
  const bool vec = (w1 & 3) == 0 && (reinterpret_cast<size_t>(prm) & 15) == 0;
  const double* cr = p.corr + (long long)s * 6;
  const double lda_w = p.lda ? p.lda[s * 3LL] : 0.0, lda_slope = p.lda ? p.lda[s * 3LL + 1] : 1.0,
               lda_icpt = p.lda ? p.lda[s * 3LL + 2] : 0.0;
  const long long p0 = p.p0, p1 = p.p0 + p.n;
  const long long emitted_now = p.e1 - p.e0;

  for (int i = tid; i < t.n_small; i += kThreads) sm_s[i] = prm[t.small0 + i];
  const float* small = sm_s - t.small0;                      // indexed by parameter offset
  double step = load_step(step_p, p.decoder);

  for (long long a = p.e0; a < p.e1; a += pass) {
    const int nf = (int)(p.e1 - a < pass ? p.e1 - a : pass);     // frames [a, a + nf) of this pass
    // ---- the forward: stage the pass's rows, layer 1 over the streamed W1, the later layers; the predictions in
    // pred_s behind a barrier
#include "online_dnn_forward_body.h"
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
    // ---- the windows that end in (a, a + nf]: online_common.h's window_block<kThreads, kThreads>, line for line,
    // written out here.  Called as the helper, this kernel's register allocation around layer 1 changed and a push
    // of 100 frames took 4 to 5 % longer on the MI355X; the other three kernels call it.
    // A change to that block is a change to this one.
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
          double sum = 0.0;
          for (int r = 64 * q + lane; r < width; r += kThreads) {
            const long long fr = r0 + r;
            const int slot = slot0 + r - (slot0 + r >= width ? width : 0);
            sum += fr >= a ? sc_s[spk * pass + (int)(fr - a)] : ring[(long long)spk * width + slot];
          }
          part[q] = wave_sum(sum);
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

  // ---- the tails for the next push: the last pre + post EEG rows and the last post envelope rows
  __syncthreads();
  tail_park<kThreads>(rows_s, tail, tl, c, p.n);
  env_tail_park<kThreads>(env_s, etail, post, p.n);
  __syncthreads();
  tail_store<kThreads>(tail, rows_s, tl, c, eeg, p.eeg_ld, p.n);
  env_tail_store<kThreads>(etail, env_s, post, env, p.env_ld, p.n);
  store_step(step_p, p.decoder, step);
}

}  // namespace

extern "C" {

int td_fc_online_lds_bytes(int c, int pre, int post, int num_hidden, const int* hidden_host, int64_t emitted,
                            int* pass, int64_t* bytes) {
  return lds_query("td_fc_online_lds_bytes", c, pre, post, num_hidden, hidden_host, emitted, pass, bytes);
}

int td_fc_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t eeg_ld,
                       int64_t eeg_session_stride, const float* env_dev, int64_t env_ld,
                       int64_t env_session_stride, int64_t n, int c, int pre, int post, const int* hidden_host,
                       int num_hidden, const float* params_dev, int64_t params_session_stride,
                       const double* corr_dev, int reduction, const double* lda_dev, int width, int hop,
                       int decoder, int64_t frames_before, int flush, void* state_dev,
                       int64_t state_session_stride, double* scores_dev, uint8_t* decisions_dev, float* pred_dev,
                       double* frame_dev) {
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_fc_online_push: handle is NULL");
  TD_REQUIRE(h, num_sessions >= 1, "td_fc_online_push: %d sessions", num_sessions);
  TD_TRY(check_shape(h, "td_fc_online_push", c, pre, post, num_hidden, hidden_host));
  TD_TRY(check_push_args(h, "td_fc_online_push", n, width, hop, reduction, 0, lda_dev, decoder, frames_before));
  if (!params_dev || !corr_dev || !state_dev || !scores_dev || !decisions_dev || (n > 0 && (!eeg_dev || !env_dev)))
    return td_fail(h, TD_ERR_INVALID, "td_fc_online_push: NULL argument");
  TD_TRY(check_push_strides(h, "td_fc_online_push", num_sessions, eeg_ld, eeg_session_stride, c, env_ld,
                            env_session_stride, 2, "envelopes"));
  const DnnNet t = net_of(c, pre, post, hidden_host, num_hidden);
  TD_REQUIRE(h, params_session_stride == 0 || params_session_stride >= t.n_params,
             "td_fc_online_push: a parameter stride of %lld for %d parameters (0 = one model)",
             (long long)params_session_stride, t.n_params);
  TD_TRY(check_state_stride(h, "td_fc_online_push", state_session_stride, state_bytes(c, pre, post, width)));
  if (n == 0 && !flush) return TD_OK;
  const OnlinePlan pl = plan_push(frames_before, n, post, width, hop, flush);
  const long long e0 = pl.emitted_before, e1 = pl.emitted_after, w0 = pl.first_window, n_win = pl.new_windows;
  DnnOnlineParams p;
  p.eeg = eeg_dev; p.eeg_ld = eeg_ld; p.eeg_ss = num_sessions > 1 ? eeg_session_stride : 0;
  p.env = env_dev; p.env_ld = env_ld; p.env_ss = num_sessions > 1 ? env_session_stride : 0;
  p.params = params_dev; p.params_ss = params_session_stride;
  p.corr = corr_dev; p.lda = reduction == 4 ? lda_dev : nullptr;
  p.n = n; p.p0 = frames_before; p.e0 = e0; p.e1 = e1; p.w0 = w0; p.n_win = n_win;
  p.c = c; p.pre = pre; p.post = post; p.reduction = reduction; p.width = width; p.hop = hop; p.decoder = decoder;
  p.pass = pass_of(t, c, pre, post, e1 - e0);     // (>= 1: check_shape)
  p.net = t;
  p.state = reinterpret_cast<unsigned char*>(state_dev); p.state_ss = state_session_stride;
  p.scores = scores_dev; p.decisions = decisions_dev; p.pred = pred_dev; p.frame = frame_dev;
  return launch_push(h, &h->lds_opt_online_dnn, dnn_online_push_kernel, num_sessions, kThreads, kLdsBudget,
                     lds_bytes(t, c, pre, post, p.pass), (double)n * num_sessions, p);
}

}  // extern "C"
