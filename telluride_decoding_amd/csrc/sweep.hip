// The window-size sweep of infer.run_reduction_test (reference infer.py:376-407) in one launch set:
// the window means of both speakers' per-frame scores and of the attention labels for EVERY window
// size, then per size the end of the first same-label stretch, the decisions and the count of
// correct windows.  The per-size route (td_window_means x3 + td_decide_* per size, each behind an
// upload and in front of a copy back) stays; this file repeats its arithmetic operation for
// operation, so the two agree bit for bit (tests/test_gpu_infer_sweep.py).
#include "td_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSizes = 16;
constexpr int kStepWords = 256;   // 64-window words per pass of the stepped decoder's walk

// The sweep's window sizes, passed by value: nothing is uploaded in front of the launches.
struct SweepSizes {
  int n;
  int width[kMaxSizes], hop[kMaxSizes];
  long long n_win[kMaxSizes];    // full windows of this size (td_window_count of one trial)
  long long first[kMaxSizes];    // index of its first window in the concatenated outputs
  long long total;
};

// (windows.hip's wave_sum: the same shuffle tree, the same bits)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One workgroup per (signal, size, window): signal 0 / 1 = the speakers' scores [frames, cols], 2 =
// the labels [frames].  Per column the mean is window_means_kernel's: threads stride the window, a
// 64-lane wave sum, ((w0 + w1) + (w2 + w3)) / width; the columns' means are then added in column
// order and scaled by the float64 reciprocal of cols -- infer._window_means_host's `acc / cols`, a
// device tensor divided by a host scalar, which the tensor library evaluates as acc * (1.0 / cols).
// (np.mean over all entries of the window, one rounding further away than a true division.)
__global__ __launch_bounds__(kThreads) void sweep_means_kernel(
    const double* __restrict__ s1, long long ld1, const double* __restrict__ s2, long long ld2,
    int cols, const double* __restrict__ labels, SweepSizes sz, double* __restrict__ means) {
  __shared__ double red[4];
  const long long b = blockIdx.x;
  const int sig = (int)(b / sz.total);
  const long long w = b - sig * sz.total;
  int k = 0;
  while (k + 1 < sz.n && w >= sz.first[k + 1]) ++k;
  const int width = sz.width[k];
  const long long r0 = (w - sz.first[k]) * sz.hop[k];
  const double* v = sig == 0 ? s1 : sig == 1 ? s2 : labels;
  const long long ld = sig == 0 ? ld1 : sig == 1 ? ld2 : 1;
  const int nc = sig == 2 ? 1 : cols;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double acc = 0.0;
  for (int c = 0; c < nc; ++c) {
    double s = 0.0;
    for (int r = tid; r < width; r += kThreads) s += v[(r0 + r) * ld + c];
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0) {
      const double m = ((red[0] + red[1]) + (red[2] + red[3])) / (double)width;
      acc = c == 0 ? m : acc + m;
    }
    __syncthreads();
  }
  if (tid == 0) means[b] = nc > 1 ? acc * (1.0 / (double)nc) : acc;
}

// One workgroup per size, after the means: end_first_section = the first window whose label mean's
// truth value differs from window 0's (infer.find_first_segment; 0 if none), the decisions --
// decoder 0: s1 > s2, strict (decide_wta_kernel); 1: one lane walks the windows with the float64
// operations of decide_step_kernel from a state of 0.5; 2: none -- and correct = the windows with
// decision xor (label mean != 0) (infer.fraction_correct's numerator).  Integer reductions only.
__global__ __launch_bounds__(kThreads) void sweep_decide_kernel(
    const double* __restrict__ means, SweepSizes sz, int decoder,
    unsigned char* __restrict__ decisions, long long* __restrict__ summary) {
  __shared__ long long red_end[kThreads];
  __shared__ long long red_ok[kThreads];
  const int k = blockIdx.x, tid = threadIdx.x;
  const long long n = sz.n_win[k];
  if (n == 0) {                       // (uniform over the workgroup)
    if (tid == 0) { summary[2 * k] = 0; summary[2 * k + 1] = 0; }
    return;
  }
  const double* m1 = means + sz.first[k];
  const double* m2 = means + sz.total + sz.first[k];
  const double* ml = means + 2 * sz.total + sz.first[k];
  unsigned char* dec = decisions + sz.first[k];
  const bool lab0 = ml[0] != 0.0;
  long long end = n, ok = 0;
  for (long long i = tid; i < n; i += kThreads) {
    const bool lab = ml[i] != 0.0;
    if (lab != lab0 && i < end) end = i;
    if (decoder == 0) {
      const bool d = m1[i] > m2[i];
      dec[i] = d ? 1 : 0;
      ok += (d != lab) ? 1 : 0;
    } else if (decoder == 2) {
      dec[i] = 0;
    }
  }
  if (decoder == 1) {
    // The stepped decoder is sequential in time: ONE lane walks the windows, with decide_step_kernel's
    // float64 operations.  What it walks over is prepared by everyone: per pass of kStepWords * 64 windows
    // the waves turn the comparisons s1 > s2 and the labels into 64-bit words (a ballot per 64 windows),
    // the lane steps through the bits in registers and leaves the decisions as words, and everyone writes
    // them out as bytes.  (The lane reading two means and writing a byte per window itself took 2.1 ms for
    // the 12 000 windows of size 10 in 60 000 frames: one memory latency per window.)
    __shared__ unsigned long long cmp_w[kStepWords], lab_w[kStepWords], dec_w[kStepWords];
    const int lane = tid & 63, wave = tid >> 6;
    double st = 0.5;
    for (long long base = 0; base < n; base += kStepWords * 64LL) {
      const long long left = n - base;
      const int words = left >= kStepWords * 64LL ? kStepWords : (int)((left + 63) / 64);
      for (int wd = wave; wd < words; wd += kThreads / 64) {         // (uniform over a wave)
        const long long i = base + 64LL * wd + lane;
        const bool in = i < n;
        const unsigned long long cb = __ballot(in && m1[in ? i : 0] > m2[in ? i : 0]);
        const unsigned long long lb = __ballot(in && ml[in ? i : 0] != 0.0);
        if (lane == 0) { cmp_w[wd] = cb; lab_w[wd] = lb; }
      }
      __syncthreads();
      if (tid == 0) {
        for (int wd = 0; wd < words; ++wd) {
          const unsigned long long cb = cmp_w[wd];
          const long long rest = left - 64LL * wd;
          const int count = rest < 64 ? (int)rest : 64;
          unsigned long long db = 0;
          for (int bit = 0; bit < count; ++bit) {
            if ((cb >> bit) & 1) st = fmin(0.9, st + 0.1);
            else st = fmax(0.1, st - 0.1);
            db |= (unsigned long long)(st > 0.5 ? 1 : 0) << bit;
          }
          dec_w[wd] = db;
          const unsigned long long valid = count == 64 ? ~0ULL : ((1ULL << count) - 1);
          ok += __popcll((db ^ lab_w[wd]) & valid);
        }
      }
      __syncthreads();
      const long long stop = left < words * 64LL ? left : words * 64LL;
      for (long long j = tid; j < stop; j += kThreads) dec[base + j] = (dec_w[j >> 6] >> (j & 63)) & 1;
      __syncthreads();                                                // (the words are rewritten next pass)
    }
  }
  red_end[tid] = end;
  red_ok[tid] = ok;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      red_end[tid] = red_end[tid + off] < red_end[tid] ? red_end[tid + off] : red_end[tid];
      red_ok[tid] += red_ok[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    summary[2 * k] = red_end[0] < n ? red_end[0] : 0;
    summary[2 * k + 1] = red_ok[0];
  }
}

}  // namespace

int td_attention_sweep(td_handle* h, const double* s1_dev, int64_t ld1, const double* s2_dev,
                       int64_t ld2, int cols, const double* labels_dev, int64_t frames,
                       const int* sizes_host, int num_sizes, int decoder, double* means_dev,
                       uint8_t* decisions_dev, int64_t* summary_dev) {
  if (!h || !s1_dev || !s2_dev || !labels_dev || !sizes_host || !means_dev || !decisions_dev ||
      !summary_dev)
    return td_fail(h, TD_ERR_INVALID, "td_attention_sweep: NULL argument");
  TD_REQUIRE(h, num_sizes >= 1 && num_sizes <= kMaxSizes,
             "td_attention_sweep: 1 to %d window sizes, not %d", kMaxSizes, num_sizes);
  TD_REQUIRE(h, cols >= 1, "td_attention_sweep: %d columns", cols);
  TD_REQUIRE(h, ld1 >= cols && ld2 >= cols,
             "td_attention_sweep: a row stride below the %d columns", cols);
  TD_REQUIRE(h, frames >= 0, "td_attention_sweep: %lld frames", (long long)frames);
  TD_REQUIRE(h, decoder >= 0 && decoder <= 2,
             "td_attention_sweep: decoder %d (0 winner-take-all, 1 stepped, 2 none)", decoder);
  SweepSizes sz;
  memset(&sz, 0, sizeof(sz));
  sz.n = num_sizes;
  for (int k = 0; k < num_sizes; ++k) {
    const int width = sizes_host[2 * k], hop = sizes_host[2 * k + 1];
    TD_REQUIRE(h, width >= 1 && hop >= 1, "td_attention_sweep: window %d of %d frames every %d", k,
               width, hop);
    sz.width[k] = width;
    sz.hop[k] = hop;
    sz.first[k] = sz.total;
    sz.n_win[k] = frames >= width ? (frames - width) / hop + 1 : 0;    // td_window_count
    sz.total += sz.n_win[k];
  }
  TD_REQUIRE(h, 3 * sz.total <= 0x7fffffffLL, "td_attention_sweep: too many windows");
  if (sz.total > 0) {
    hipLaunchKernelGGL(sweep_means_kernel, dim3((unsigned)(3 * sz.total)), dim3(kThreads), 0,
                       h->stream, s1_dev, (long long)ld1, s2_dev, (long long)ld2, cols, labels_dev,
                       sz, means_dev);
    TD_HIP(h, hipGetLastError());
  }
  hipLaunchKernelGGL(sweep_decide_kernel, dim3((unsigned)num_sizes), dim3(kThreads), 0, h->stream,
                     means_dev, sz, decoder, decisions_dev,
                     reinterpret_cast<long long*>(summary_dev));
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}
