// Online calibration of a DNN decoder bank (td_fccalib_online_*): online_calib.hip's sums -- what
// infer_decoder.Decoder.train(data0, data1, window_size = W) takes from a labelled stretch: the correlator's
// statistics, the scaled LDA between the window means of the unattended (class 0) and the attended (class 1)
// correlations, d' -- with the bank's fully connected regressor in front of them instead of the FIR prediction.  A bank
// of sessions, one workgroup of 256 threads each, the state on the device, ONE launch per push, the host counts the
// frames, a block of zeros is a fresh session, no atomics, vector stores only.
//
// The state block is td_calib_online_push's byte for byte -- online_calib_common.h's head of TD_CALIB_ONLINE_SUMS
// float64 sums, then the EEG tail [pre + post][c] and the envelope tail [post][2] in float32, rounded up to 8 -- so
// td_calib_online_sums and td_calib_online_finish, which read the head alone, serve it as they are.
//
// The prediction of an emitted frame is the float32 value td_fc_online_push returns in `pred`, which has
// td_mlp_forward's bits: the forward of a pass is online_dnn_forward_body.h, the text dnn_online_push_kernel includes
// too, over online_dnn_common.h's layer-1 functions.  Behind the forward the walk is online_calib_common.h's, the one
// online_calib_push_kernel calls: a frame's {1, p, a, u} sits in LDS as float64, lane t of the first wave owns state
// double t and advances it in frame order, the Gram takes G + z_i z_j UNFUSED -- that header's fp contract(off), and
// this file's own, as in online_calib.hip; the prediction's fused multiply-adds are explicit
// fmaf calls, which the pragma does not touch.  So acc += float64(x) * float64(p) and G + np.outer(z, z) in NumPy
// are a bit-exact twin, and any cut of a recording into pushes gives the same state bytes.
//
// LDS of a launch is online_dnn.hip's, byte for byte (lds_bytes): the 8 (4 pass) bytes that hold the scores and the
// window means there hold {1, p, a, u} here.  Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are in
// DESIGN.md sections 45 and 47.
#include "online_dnn_common.h"
#include "online_calib_common.h"

#pragma clang fp contract(off)

namespace {

struct DnnCalibParams {
  const float* eeg; long long eeg_ld, eeg_ss;
  const float* env; long long env_ld, env_ss;
  const float* params; long long params_ss;
  long long n, p0;               // rows of this push, rows pushed before it
  long long e0, e1;              // frames emitted before / after
  int c, pre, post, width, pass;
  DnnNet net;
  unsigned char* state; long long state_ss;
};

__global__ __launch_bounds__(kThreads) void dnn_calib_push_kernel(DnnCalibParams p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int s = blockIdx.x;
  const int c = p.c, pre = p.pre, post = p.post, width = p.width;
  const int tl = pre + post, pass = p.pass, ldr = row_stride(c);
  const DnnNet& t = p.net;
  const int nl = t.nl, w1 = t.w[1], w1q = t.nj / 4, nj = t.nj, ks = t.ks, lda_s = t.lda, k_all = t.w[0];
  const int chunk_floats = t.g * ks * nj;
  double* val_s = lds;                                       // [pass][4] a frame's {1, p, a, u}
  float* ws_s = reinterpret_cast<float*>(val_s + 4 * pass);  // [2][chunk_floats] chunks of W1 (16-byte aligned)
  float* sm_s = ws_s + 2 * chunk_floats;                     // [n_small] b1, W2, b2, ...
  float* rows_s = sm_s + (t.n_small + 3) / 4 * 4;            // [pass + tl][ldr] the pass's EEG rows
  float* env_s = rows_s + (size_t)(pass + tl) * ldr;         // [max(pass, post)][2]
  float* pred_s = env_s + 2 * (pass > post ? pass : post);   // [pass]
  float* act_s = pred_s + pass;                              // [2][pass][lda_s] activations, in turn

  unsigned char* st = p.state + (long long)s * p.state_ss;
  double* sums = reinterpret_cast<double*>(st);                                    // [kSums]
  float* tail = reinterpret_cast<float*>(st + state_eeg_offset());                 // [tl][c]
  float* etail = reinterpret_cast<float*>(st + state_env_offset(c, pre, post));    // [post][2]
  const float* eeg = p.eeg + (long long)s * p.eeg_ss;
  const float* env = p.env + (long long)s * p.env_ss;
  const float* prm = p.params + (long long)s * p.params_ss;
  const bool vec = (w1 & 3) == 0 && (reinterpret_cast<size_t>(prm) & 15) == 0;
  const long long p0 = p.p0, p1 = p.p0 + p.n;

  for (int i = tid; i < t.n_small; i += kThreads) sm_s[i] = prm[t.small0 + i];
  const float* small = sm_s - t.small0;                      // indexed by parameter offset

  WalkLane wl = walk_lane(sums, tid);                        // lane t owns state double t

  for (long long a = p.e0; a < p.e1; a += pass) {
    const int nf = (int)(p.e1 - a < pass ? p.e1 - a : pass);     // frames [a, a + nf) of this pass
    // ---- the forward: stage the pass's rows, layer 1 over the streamed W1, the later layers; the predictions in
    // pred_s behind a barrier
#include "online_dnn_forward_body.h"
    // ---- a frame's {1, p, a, u}, widened
    for (int f = tid; f < nf; f += kThreads) {
      val_s[4 * f] = 1.0;
      val_s[4 * f + 1] = (double)pred_s[f];
      val_s[4 * f + 2] = (double)env_s[2 * f];
      val_s[4 * f + 3] = (double)env_s[2 * f + 1];
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

}  // namespace

extern "C" {

int td_fccalib_online_state_bytes(int c, int pre, int post, int64_t* bytes) {
  if (!bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_fccalib_online_state_bytes: NULL argument");
  TD_TRY(check_context(nullptr, "td_fccalib_online_state_bytes", c, pre, post, kMaxChannels, kMaxLags));
  *bytes = state_bytes(c, pre, post);
  return TD_OK;
}

int td_fccalib_online_lds_bytes(int c, int pre, int post, int num_hidden, const int* hidden_host, int64_t emitted,
                                int* pass, int64_t* bytes) {
  return lds_query("td_fccalib_online_lds_bytes", c, pre, post, num_hidden, hidden_host, emitted, pass, bytes);
}

int td_fccalib_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t eeg_ld,
                           int64_t eeg_session_stride, const float* env_dev, int64_t env_ld,
                           int64_t env_session_stride, int64_t n, int64_t frames_before, int c, int pre, int post,
                           const int* hidden_host, int num_hidden, const float* params_dev,
                           int64_t params_session_stride, int width, int flush, void* state_dev,
                           int64_t state_session_stride) {
  const char* who = "td_fccalib_online_push";
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "%s: handle is NULL", who);
  TD_TRY(check_shape(h, who, c, pre, post, num_hidden, hidden_host));
  TD_TRY(check_calib_push(h, who, width, n, frames_before, num_sessions, state_dev, state_session_stride, c, pre,
                          post));
  if (!params_dev || (n > 0 && (!eeg_dev || !env_dev))) return td_fail(h, TD_ERR_INVALID, "%s: NULL argument", who);
  if (n > 0)
    TD_TRY(check_push_strides(h, who, num_sessions, eeg_ld, eeg_session_stride, c, env_ld, env_session_stride, 2,
                              "envelopes"));
  const DnnNet t = net_of(c, pre, post, hidden_host, num_hidden);
  TD_REQUIRE(h, params_session_stride == 0 || params_session_stride >= t.n_params,
             "%s: a parameter stride of %lld for %d parameters (0 = one model)", who,
             (long long)params_session_stride, t.n_params);
  if (n == 0 && !flush) return TD_OK;
  const OnlinePlan pl = plan_push(frames_before, n, post, width, width, flush);   // (its windows: hop = width)
  DnnCalibParams p;
  p.eeg = eeg_dev; p.eeg_ld = eeg_ld; p.eeg_ss = num_sessions > 1 ? eeg_session_stride : 0;
  p.env = env_dev; p.env_ld = env_ld; p.env_ss = num_sessions > 1 ? env_session_stride : 0;
  p.params = params_dev; p.params_ss = params_session_stride;
  p.n = n; p.p0 = frames_before;
  p.e0 = pl.emitted_before; p.e1 = pl.emitted_after;
  p.c = c; p.pre = pre; p.post = post; p.width = width;
  p.pass = pass_of(t, c, pre, post, p.e1 - p.e0);     // (>= 1: check_shape)
  p.net = t;
  p.state = reinterpret_cast<unsigned char*>(state_dev); p.state_ss = state_session_stride;
  return launch_push(h, &h->lds_opt_online_dnn_calib, dnn_calib_push_kernel, num_sessions, kThreads, kLdsBudget,
                     lds_bytes(t, c, pre, post, p.pass), (double)n * num_sessions, p);
}

}  // extern "C"
