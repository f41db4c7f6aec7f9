// What the online push kernels share (online.hip, online_cca.hip, online_calib.hip, through online_dnn_common.h
// online_dnn.hip and online_dnn_calib.hip and, through online_cca_common.h, online_cca_calib.hip): the state block's layout, the plan of a push, and the blocks of a push
// kernel that every session repeats -- stage, (predict: each file's own, the FIR prediction here for the two files
// that use it), score, windows, tails -- and, on the host, the launch tail of a push entry point and the read-out of a
// calibration state's float64 head.  What the two envelope calibrations share beyond this is online_calib_common.h.
// The host interface is td_common.h.  online_fit.hip and online_cca_fit.hip
// take, through online_fit_common.h, the plan of a push, the wave sum and the host checks of the strides and the
// state; their moments and double-buffered tails are their own.  online_pre.hip and online_audio.hip carry other
// state and do not use this.
//
// Every block here is under the family's promise: any cut of a recording into pushes gives the bytes of one push.
// The calibration and the fit files include this under a file-level `#pragma clang fp contract(off)`, the other
// files under the default (on), so nothing here may depend on the contraction mode at the include point: where
// a fused operation is the contract it is an explicit fmaf / fma, and nowhere else does a product feed an add or a
// subtract in one expression (no bare a * b + c).  Keep it so when adding to this file.
#pragma once
#include "td_common.h"

namespace {

// ---- state layout.  A session's block is [head][EEG tail f32 [rows][c]][a second tail, f32], rounded up to 8
// bytes.  The decoders' head is [stepped state f64][ring f64 [2][width]]; calibration's is its sums.  The second
// tail is the envelope tail [post][2], or the CCA feature tail [2][pre2 + post][c2].
__host__ __device__ inline long long tail_end(long long head, int c, int rows) { return head + 4LL * c * rows; }
__host__ __device__ inline long long tails_bytes(long long head, int c, int rows, long long second_floats) {
  return (tail_end(head, c, rows) + 4LL * second_floats + 7) / 8 * 8;
}
__host__ __device__ inline long long state_ring_offset() { return 8; }
__host__ __device__ inline long long state_eeg_offset(int width) { return 8 + 16LL * width; }   // the decoders' head
// The linear and the DNN decoder: the envelope tail behind pre + post EEG rows.
__host__ __device__ inline long long state_env_offset(int c, int pre, int post, int width) {
  return tail_end(state_eeg_offset(width), c, pre + post);
}
__host__ __device__ inline long long state_bytes(int c, int pre, int post, int width) {
  return tails_bytes(state_eeg_offset(width), c, pre + post, 2LL * post);
}

// ---- the plan of a push: host arithmetic (td_online_plan exports it)
inline long long windows_of(long long frames, int width, int hop) {      // td_window_count of one trial
  return frames >= width ? (frames - width) / hop + 1 : 0;
}

struct OnlinePlan {
  long long emitted_before, emitted_after, first_window, new_windows;
};

inline OnlinePlan plan_push(long long frames_before, long long n, int post, int width, int hop, int flush) {
  OnlinePlan pl;
  const long long pushed = frames_before + n;
  pl.emitted_before = frames_before > post ? frames_before - post : 0;
  pl.emitted_after = flush ? pushed : (pushed > post ? pushed - post : 0);
  pl.first_window = windows_of(pl.emitted_before, width, hop);
  pl.new_windows = windows_of(pl.emitted_after, width, hop) - pl.first_window;
  return pl;
}

// ---- wave sums (windows.hip's wave_sum: the same shuffle tree, the same bits)
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

// frame_scores_kernel's value for ONE column (windows.hip): a = the truth, b = the prediction.  The sums over the
// columns start from 0.0 there, so they do here; that kernel's v lda_w + 0.0 and slope acc + intercept are one
// fused multiply-add each.
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
    acc = fma(v, lda_w, acc);
    acc = fma(lda_slope, acc, lda_intercept);
  }
  return acc;
}

// ---- the stepped decoder's state: thread 0 carries it through the launch (a stored 0.0 is a fresh session)
__device__ __forceinline__ double load_step(const double* step_p, int decoder) {
  double step = 0.5;
  if (threadIdx.x == 0 && decoder == 1) {
    const double stored = *step_p;
    step = stored == 0.0 ? 0.5 : stored;
  }
  return step;
}

__device__ __forceinline__ void store_step(double* step_p, int decoder, double step) {
  if (threadIdx.x == 0 && decoder == 1) *step_p = step;
}

// ---- staging.  Rows first .. first + n_rows - 1 of the recording into rows_s (row stride ldr): from the tail (the
// tail_rows rows before this push, which is rows [p0, p1)), from the push, zeros before the recording and behind a
// flushed end.  A wave per row.
template <int NT>
__device__ __forceinline__ void stage_rows(float* rows_s, int ldr, const float* tail, int tail_rows, const float* src,
                                           long long src_ld, int c, long long first, int n_rows, long long p0,
                                           long long p1) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int rr = wave; rr < n_rows; rr += NT / 64) {
    const long long row = first + rr;
    for (int ch = lane; ch < c; ch += 64) {
      float v = 0.f;
      if (row >= 0 && row < p0) v = tail[(row - (p0 - tail_rows)) * c + ch];
      else if (row >= p0 && row < p1) v = src[(row - p0) * src_ld + ch];
      rows_s[rr * ldr + ch] = v;
    }
  }
}

// The envelope rows a .. a + nf - 1 ([n][2]) into env_s: from the tail of `post` rows or from the push (an emitted
// frame's envelope row always exists).
template <int NT>
__device__ __forceinline__ void stage_env(float* env_s, const float* etail, int post, const float* env,
                                          long long env_ld, long long a, int nf, long long p0) {
  for (int i = threadIdx.x; i < 2 * nf; i += NT) {
    const long long row = a + (i >> 1);
    env_s[i] = row < p0 ? etail[(row - (p0 - post)) * 2 + (i & 1)] : env[(row - p0) * env_ld + (i & 1)];
  }
}

// ---- the FIR prediction of one frame by one wave: lane q takes the terms k = q, q + 64, ... of the (lag, channel)
// sum into four accumulators in turn, ((a0 + a1) + (a2 + a3)), then the 64-lane tree, then the bias.  Lane 0 holds
// the value.
__device__ __forceinline__ float fir_predict(const float* w_s, const float* xr, int k_all, float bias) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int k = threadIdx.x & 63;
  for (; k + 192 < k_all; k += 256) {
    a0 = fmaf(w_s[k], xr[k], a0);
    a1 = fmaf(w_s[k + 64], xr[k + 64], a1);
    a2 = fmaf(w_s[k + 128], xr[k + 128], a2);
    a3 = fmaf(w_s[k + 192], xr[k + 192], a3);
  }
  if (k < k_all) a0 = fmaf(w_s[k], xr[k], a0);
  if (k + 64 < k_all) a1 = fmaf(w_s[k + 64], xr[k + 64], a1);
  if (k + 128 < k_all) a2 = fmaf(w_s[k + 128], xr[k + 128], a2);
  return wave_sum_f32((a0 + a1) + (a2 + a3)) + bias;
}

// ---- the window block of a pass: frames [a, a + nf) with their scores in sc_s [2][pass]; call it behind the barrier
// that follows their stores.  The windows that end in (a, a + nf]: window wi = frames [wi hop, wi hop + width).  A
// WAVE forms a window's mean with window_means_kernel's operations: lane q stands in for the threads q, q + 64, ...
// of that kernel's workgroup of NW = 256 threads (four partial sums, four wave sums), whatever this workgroup's own
// NT is.  Frames before `a` come from the ring, which holds the `width` frames before `a` until this pass has stored
// its own.  Then the scores store, the decisions (decide_wta_kernel / decide_step_kernel), the ring update, the
// fence and the barrier in front of the next pass.
template <int NT, int NW>
__device__ __forceinline__ void window_block(const double* sc_s, double* wm_s, double* ring, int pass, long long a,
                                             int nf, int width, int hop, int decoder, double& step, long long w0,
                                             long long n_win, double* scores, unsigned char* decisions) {
  static_assert(NW == 256, "a window mean keeps window_means_kernel's order: four wave sums");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x;
  const long long end_lo = a + 1 > width ? a + 1 : width;      // the first window end in reach
  const long long wi_lo = (end_lo - width + hop - 1) / hop;
  const long long wi_hi = a + nf >= width ? (a + nf - width) / hop + 1 : 0;   // one past the last
  const int nw = wi_hi > wi_lo ? (int)(wi_hi - wi_lo) : 0;
  for (int j = wave; j < nw; j += NT / 64) {
    const long long r0 = (wi_lo + j) * hop;
    const int slot0 = (int)(r0 % width);                       // ring slot of the window's first frame
#pragma unroll
    for (int spk = 0; spk < 2; ++spk) {
      double part[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double acc = 0.0;
        for (int r = 64 * q + lane; r < width; r += NW) {
          const long long fr = r0 + r;
          const int slot = slot0 + r - (slot0 + r >= width ? width : 0);
          acc += fr >= a ? sc_s[spk * pass + (int)(fr - a)] : ring[(long long)spk * width + slot];
        }
        part[q] = wave_sum(acc);
      }
      if (lane == 0) {
        const double m = ((part[0] + part[1]) + (part[2] + part[3])) / (double)width;
        wm_s[spk * pass + j] = m;
        scores[((long long)spk * gridDim.x + s) * n_win + (wi_lo + j - w0)] = m;
      }
    }
  }
  __syncthreads();
  unsigned char* dec = decisions + (long long)s * n_win + (wi_lo - w0);
  if (decoder == 1) {
    if (tid == 0) {
      for (int j = 0; j < nw; ++j) {
        if (wm_s[j] > wm_s[pass + j]) step = fmin(0.9, step + 0.1);
        else step = fmax(0.1, step - 0.1);
        dec[j] = step > 0.5 ? 1 : 0;
      }
    }
  } else {
    for (int j = tid; j < nw; j += NT)
      dec[j] = decoder == 0 ? (wm_s[j] > wm_s[pass + j] ? 1 : 0) : 0;
  }
  // (a pass longer than the ring: only its last `width` frames, one per slot)
  const int slot_a = (int)(a % width);
  for (int i = tid; i < 2 * nf; i += NT) {
    const int spk = i / nf, f = i - spk * nf;
    if (nf - f <= width) ring[(long long)spk * width + (slot_a + f) % width] = sc_s[spk * pass + f];
  }
  __threadfence_block();
  __syncthreads();
}

// ---- the tails for the next push: the last `rows` rows of (old tail, this push of n rows).  A push shorter than a
// tail shifts it: the rows that stay go through LDS -- tail_park, a barrier, tail_store.
template <int NT>
__device__ __forceinline__ void tail_park(float* park_s, const float* tail, int rows, int c, long long n) {
  const int keep = n < rows ? (int)(rows - n) : 0;               // old rows that stay
  for (int i = threadIdx.x; i < keep * c; i += NT) park_s[i] = tail[(rows - keep) * c + i];
}

template <int NT>
__device__ __forceinline__ void tail_store(float* tail, const float* park_s, int rows, int c, const float* src,
                                           long long src_ld, long long n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int keep = n < rows ? (int)(rows - n) : 0;
  for (int rr = wave; rr < rows; rr += NT / 64)
    for (int ch = lane; ch < c; ch += 64)
      tail[rr * c + ch] = rr < keep ? park_s[rr * c + ch] : src[(n - (rows - rr)) * src_ld + ch];
}

// The envelope tail [post][2], a thread per float.
template <int NT>
__device__ __forceinline__ void env_tail_park(float* park_s, const float* etail, int post, long long n) {
  const int ekeep = n < post ? (int)(post - n) : 0;
  for (int i = threadIdx.x; i < ekeep * 2; i += NT) park_s[i] = etail[(post - ekeep) * 2 + i];
}

template <int NT>
__device__ __forceinline__ void env_tail_store(float* etail, const float* park_s, int post, const float* env,
                                               long long env_ld, long long n) {
  const int ekeep = n < post ? (int)(post - n) : 0;
  for (int i = threadIdx.x; i < post * 2; i += NT) {
    const int rr = i >> 1;
    etail[i] = rr < ekeep ? park_s[i] : env[(n - (post - rr)) * env_ld + (i & 1)];
  }
}

// ---- a calibration state's float64 head, copied out.  grid (ceil(S sums / NT)): out [S][sums].  (A template, so
// that only the files that launch it hold a copy: a plain kernel here is emitted into every including file.)
template <int NT>
__global__ __launch_bounds__(NT) void online_head_sums_kernel(const unsigned char* state, long long state_ss,
                                                              int num_sessions, int sums, double* out) {
  const long long e = (long long)blockIdx.x * NT + threadIdx.x;
  if (e >= (long long)num_sessions * sums) return;
  const int s = (int)(e / sums), j = (int)(e - (long long)s * sums);
  out[e] = reinterpret_cast<const double*>(state + (long long)s * state_ss)[j];
}

template <int NT = 256>
inline int launch_head_sums(td_handle* h, int num_sessions, const void* state_dev, long long state_ss, int sums,
                            double* out_dev) {
  const unsigned blocks = (unsigned)td_ceil_div((long long)num_sessions * sums, NT);
  hipLaunchKernelGGL(online_head_sums_kernel<NT>, dim3(blocks), dim3(NT), 0, h->stream,
                     reinterpret_cast<const unsigned char*>(state_dev), state_ss, num_sessions, sums, out_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

// ---- the launch tail of a push entry point: the kernel's dynamic LDS cap raised once per handle (`raised` is the
// handle's flag for this kernel), then the profile mark, the launch of `grid` workgroups of `block` threads with
// `lds` bytes, its error, the profile mark.
template <typename Params>
inline int launch_push(td_handle* h, bool* raised, void (*kernel)(Params), int grid, int block, long long lds_cap,
                       long long lds, double work, const Params& p) {
  if (!*raised) {
    TD_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_cap));
    *raised = true;
  }
  TD_TRY(td_profile_mark(h, true, work));
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3((unsigned)block), (size_t)lds, h->stream, p);
  TD_HIP(h, hipGetLastError());
  TD_TRY(td_profile_mark(h, false, 0.0));
  return TD_OK;
}

// ---- host checks.  `who` is the entry point's name; each file calls these where its own checks stood, so the
// first message of a call with several bad arguments stays what it was.
inline int check_context(td_handle* h, const char* who, int c, int pre, int post, int max_channels, int max_lags) {
  TD_REQUIRE(h, c >= 1 && c <= max_channels, "%s: %d channels (1 .. %d)", who, c, max_channels);
  TD_REQUIRE(h, pre >= 0 && post >= 0 && pre + 1 + post <= max_lags,
             "%s: context of %d + 1 + %d frames (at most %d lags)", who, pre, post, max_lags);
  return TD_OK;
}

// The decoders' push: dims = 0 for one prediction column (no reduction 1), else the CCA model's columns.
inline int check_push_args(td_handle* h, const char* who, long long n, int width, int hop, int reduction, int dims,
                           const double* lda_dev, int decoder, long long frames_before) {
  TD_REQUIRE(h, n >= 0 && n <= TD_ONLINE_MAX_PUSH, "%s: %lld frames in one push (0 .. %d)", who, n,
             TD_ONLINE_MAX_PUSH);
  TD_REQUIRE(h, width >= 1 && width <= TD_ONLINE_MAX_WIDTH, "%s: window of %d frames (1 .. %d)", who, width,
             TD_ONLINE_MAX_WIDTH);
  TD_REQUIRE(h, hop >= 1, "%s: window step of %d frames", who, hop);
  if (dims == 0) {
    TD_REQUIRE(h, reduction == 0 || reduction == 2 || reduction == 3 || reduction == 4,
               "%s: reduction %d (0 first, 2 mean, 3 mean-squared, 4 lda)", who, reduction);
  } else {
    TD_REQUIRE(h, reduction >= 0 && reduction <= 4,
               "%s: reduction %d (0 first, 1 second, 2 mean, 3 mean-squared, 4 lda)", who, reduction);
    TD_REQUIRE(h, reduction != 1 || dims >= 2, "%s: reduction 1 (second) needs at least 2 dims", who);
  }
  TD_REQUIRE(h, reduction != 4 || lda_dev, "%s: the lda reduction needs lda_dev", who);
  TD_REQUIRE(h, decoder >= 0 && decoder <= 2, "%s: decoder %d (0 winner-take-all, 1 stepped, 2 none)", who, decoder);
  TD_REQUIRE(h, frames_before >= 0, "%s: %lld frames before", who, frames_before);
  return TD_OK;
}

// The row and session strides of the EEG and of what is pushed beside it (c2 `what` per row).
inline int check_push_strides(td_handle* h, const char* who, int num_sessions, long long eeg_ld, long long eeg_ss,
                              int c, long long side_ld, long long side_ss, int c2, const char* what) {
  TD_REQUIRE(h, eeg_ld >= c && side_ld >= c2, "%s: a row stride below a row (%lld for %d channels, %lld for %d %s)",
             who, eeg_ld, c, side_ld, c2, what);
  TD_REQUIRE(h, num_sessions == 1 || (eeg_ss >= c && side_ss >= c2), "%s: a session stride below a row", who);
  return TD_OK;
}

// The FIR model's strides: k weights and one bias per session, or one model for all.
inline int check_fir_strides(td_handle* h, const char* who, long long w_ss, long long b_ss, int k) {
  TD_REQUIRE(h, w_ss == 0 || w_ss >= k, "%s: a weight stride of %lld for %d weights (0 = one model)", who, w_ss, k);
  TD_REQUIRE(h, b_ss == 0 || b_ss >= 1, "%s: a bias stride of %lld", who, b_ss);
  return TD_OK;
}

inline int check_state_stride(td_handle* h, const char* who, long long stride, long long need) {
  TD_REQUIRE(h, stride >= need && stride % 8 == 0, "%s: a state stride of %lld bytes (a multiple of 8, at least %lld)",
             who, stride, need);
  return TD_OK;
}

// A bank's state as the training stages take it (the fits and the calibrations): the session count, the pointer,
// the stride against the `need` bytes of one block.
inline int check_state(td_handle* h, const char* who, int num_sessions, const void* state_dev, long long stride,
                       long long need) {
  TD_REQUIRE(h, num_sessions >= 1 && num_sessions <= 65535, "%s: %d sessions (1 .. 65535)", who, num_sessions);
  if (!state_dev) return td_fail(h, TD_ERR_INVALID, "%s: NULL argument", who);
  TD_TRY(check_state_stride(h, who, stride, need));
  return TD_OK;
}

}  // namespace
