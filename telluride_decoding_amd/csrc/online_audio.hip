// The online audio front end (td_audio_online_*): audio.hip's intensity envelope -- the windowed mean of
// float32(x)^2 in float64, then sqrt and ** exponent -- for audio rows that arrive in pushes of any length, as the
// online family does everything else: the state on the device, ONE launch per push for a bank of sessions, and any
// cut of a recording gives the bytes of one push.  The frames are those of AudioFeatures.compute_intensity on the
// WHOLE recording (a fresh object): the batch call restarts its window centres on every call, this one does not.
//
// Frames.  With N rows pushed so far, F(N) = rint(N / fs_in * fs_out), hw = 0.5 window / fs_out and, for frame i,
// t = i / fs_out, a_i = rint(fs_in (t - hw)), u_i = rint(fs_in (t + hw)) (float64 in the reference's order, half
// even: window_of of audio.hip), frame i is emitted by the first push after which u_i <= N and i < F(N); a flush
// emits every frame i < F(N) still missing, its window clamped at N.  The host says which frames a push emits
// (td_audio_online_plan) and every wave computes its frame's window itself: no index array is uploaded.
//
// The sum.  A wave owns one (session, frame).  Lane l adds the rows a + l + 64 k of its span in increasing k, in
// float64, one accumulator per channel; then the fixed xor butterfly (32, 16, .. 1) per channel.  That order is a
// function of (a_i, u_i) and the data alone -- not of the cut, not of an address -- so the bits are too.
//
// The state.  A frame reaches back before its push: the squares (float32) of the last K rows pushed are carried,
// slot j of a tail copy holding row N - K + j (rows before row 0 read as zero, so all zeros = fresh and the copy is a
// function of the rows pushed whatever the cut).  K = ceil((window / 2 + max(window / 2, 0.5)) fs_in / fs_out) + 2
// bounds N - max(0, a_e) for the first frame e not yet emitted (tests/test_cpu_online_audio.py checks it by brute
// force; the push checks it again before it launches).  The rows a push retires from the tail are rows other
// workgroups of the same launch still read, so the state block holds TWO tail copies: a launch reads copy `live` and
// the workgroups behind the frames' write all K slots of the other one.  The host flips `live` after every push
// with n > 0; a push without rows (a flush on its own) writes nothing and flips nothing.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are in DESIGN.md section 31.
#include <cmath>

#include "td_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;          // frames per workgroup
constexpr int kMaxChannels = TD_AUDIO_ONLINE_MAX_CHANNELS;
constexpr int kTailBlocks = 32;                // workgroups per session that write the next tail copy (at most)

struct AudioParams {
  const void* x; long long ldx, x_ss;
  long long n, rows_before;
  long long e0;                   // the first frame this push emits
  int emitted, c, k_rows, post_blocks;   // post_blocks: the frame workgroups (blockIdx.x below it)
  double fs_in, fs_out, hw, expo;
  const float* tail_in; float* tail_out; long long state_ss;   // (elements of float)
  float* out32; double* out64; long long ldout, out_ss;
  long long* win;
};

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }

// numpy's scalar-power fast paths (1, 2, 0.5, 0, -1), pow otherwise (audio.hip's pow_e)
__device__ __forceinline__ double pow_e(double v, double e) {
  if (e == 1.0) return v;
  if (e == 2.0) return v * v;
  if (e == 0.5) return sqrt(v);
  if (e == 0.0) return 1.0;
  if (e == -1.0) return 1.0 / v;
  return pow(v, e);
}

// float32(x)^2, squared in float32 as numpy does (audio.hip's feature<true>)
template <typename T>
__device__ __forceinline__ float square32(T v) {
  const float f = (float)v;
  return f * f;
}

// The reference's window of frame i, float64 in its order of operations (audio.hip's window_of, tau = 0).
__host__ __device__ inline void window_raw(long long i, double fs_in, double fs_out, double hw, long long& a,
                                           long long& u) {
  const double t = (double)i / fs_out;
  a = (long long)rint(fs_in * (t - hw));
  u = (long long)rint(fs_in * (t + hw));
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double finish(double sum, long long cnt, double expo) {
  if (cnt <= 0) return qnan();        // np.mean of an empty slice
  return pow_e(sqrt(sum / (double)cnt), expo);
}

// grid (frame workgroups + tail workgroups, sessions)
template <typename T>
__global__ void __launch_bounds__(kThreads) audio_online_kernel(AudioParams p) {
  const int s = blockIdx.y, c = p.c;
  const T* x = reinterpret_cast<const T*>(p.x) + (long long)s * p.x_ss;
  const float* tail = p.tail_in + (long long)s * p.state_ss;
  const long long before = p.rows_before, n_all = p.rows_before + p.n;
  const long long base = before - p.k_rows;                 // the row of the tail's slot 0 (may be negative)

  if ((int)blockIdx.x >= p.post_blocks) {
    // ---- the next tail copy: slot j <- the square of row n_all - K + j
    float* next = p.tail_out + (long long)s * p.state_ss;
    const long long total = (long long)p.k_rows * c;
    const long long first = n_all - p.k_rows;
    for (long long e = (long long)(blockIdx.x - p.post_blocks) * kThreads + threadIdx.x; e < total;
         e += (long long)(gridDim.x - p.post_blocks) * kThreads) {
      const long long j = e / c;
      const int ch = (int)(e - j * c);
      const long long r = first + j;
      float v = 0.0f;
      if (r >= before) v = square32(x[(r - before) * p.ldx + ch]);
      else if (r >= 0) v = tail[(r - base) * c + ch];
      next[e] = v;
    }
    return;
  }

  const int f = blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (f >= p.emitted) return;
  long long t1, t2;
  window_raw(p.e0 + f, p.fs_in, p.fs_out, p.hw, t1, t2);
  t1 = t1 < 0 ? 0 : t1;
  t2 = t2 > n_all ? n_all : t2;                             // (only a flushed frame's window reaches past the rows)
  double acc[kMaxChannels];
#pragma unroll
  for (int ch = 0; ch < kMaxChannels; ++ch) acc[ch] = 0.0;
  for (long long r = t1 + lane; r < t2; r += 64) {
    if (r >= before) {
      const T* row = x + (r - before) * p.ldx;
#pragma unroll
      for (int ch = 0; ch < kMaxChannels; ++ch)
        if (ch < c) acc[ch] += (double)square32(row[ch]);
    } else {
      const float* row = tail + (r - base) * c;
#pragma unroll
      for (int ch = 0; ch < kMaxChannels; ++ch)
        if (ch < c) acc[ch] += (double)row[ch];
    }
  }
  double mine = 0.0;
#pragma unroll
  for (int ch = 0; ch < kMaxChannels; ++ch) {
    if (ch < c) {
      const double tot = wave_sum(acc[ch]);
      if (lane == ch) mine = tot;
    }
  }
  if (lane < c) {
    const double v = finish(mine, t2 - t1, p.expo);
    const long long at = (long long)s * p.out_ss + (long long)f * p.ldout + lane;
    if (p.out64) p.out64[at] = v;
    if (p.out32) p.out32[at] = (float)v;
  }
  if (p.win && s == 0 && lane == 0) {
    p.win[2 * (long long)f] = t1;
    p.win[2 * (long long)f + 1] = t2;
  }
}

struct Rates {
  double fs_in, fs_out, window, hw;
  long long k_rows;
};

// F(N): the frames of a recording of N rows
long long frames_of(const Rates& r, long long n) { return (long long)rint((double)n / r.fs_in * r.fs_out); }

long long upper_of(const Rates& r, long long i) {
  long long a, u;
  window_raw(i, r.fs_in, r.fs_out, r.hw, a, u);
  return u;
}

// G(N): the frames i with u_i <= N (u is non-decreasing in i)
long long frames_in_reach(const Rates& r, long long n) {
  long long g = (long long)(((double)n / r.fs_in - r.hw) * r.fs_out);
  if (g < 0) g = 0;
  while (g > 0 && upper_of(r, g - 1) > n) --g;
  while (upper_of(r, g) <= n) ++g;
  return g;
}

struct PushPlan {
  long long e0, e1, held;
};

void plan_push(const Rates& r, long long rows_before, long long n, int flush, PushPlan* p) {
  const long long n1 = rows_before + n;
  const long long g0 = frames_in_reach(r, rows_before), f0 = frames_of(r, rows_before);
  const long long g1 = frames_in_reach(r, n1), f1 = frames_of(r, n1);
  p->e0 = g0 < f0 ? g0 : f0;
  p->e1 = flush ? f1 : (g1 < f1 ? g1 : f1);
  if (p->e1 < p->e0) p->e1 = p->e0;
  p->held = f1 - p->e1;
}

int check_rates(td_handle* h, const char* who, double fs_in, double fs_out, double window, Rates* r) {
  TD_REQUIRE(h, fs_in > 0.0 && fs_out > 0.0 && std::isfinite(fs_in) && std::isfinite(fs_out),
             "%s: rates of %g and %g Hz (positive and finite)", who, fs_in, fs_out);
  TD_REQUIRE(h, window > 0.0 && std::isfinite(window), "%s: a window of %g frames (positive and finite)", who, window);
  TD_REQUIRE(h, fs_out < fs_in || window > 1.0,
             "%s: %g -> %g Hz with a window of %g is the reference's pass-through (fs_out >= fs_in and window <= 1): "
             "there is nothing to compute", who, fs_in, fs_out, window);
  r->fs_in = fs_in;
  r->fs_out = fs_out;
  r->window = window;
  r->hw = 0.5 * window / fs_out;
  const double half = 0.5 * window;
  const double k = std::ceil((half + (half > 0.5 ? half : 0.5)) * fs_in / fs_out) + 2.0;
  TD_REQUIRE(h, k <= (double)TD_AUDIO_ONLINE_MAX_TAIL,
             "%s: %g -> %g Hz with a window of %g carries %.0f rows (at most %d)", who, fs_in, fs_out, window, k,
             TD_AUDIO_ONLINE_MAX_TAIL);
  r->k_rows = (long long)k;
  return TD_OK;
}

long long state_bytes(int c, long long k_rows) { return 2LL * 4LL * k_rows * c; }

}  // namespace

extern "C" {

int td_audio_online_plan(int64_t rows_before, int64_t n, double fs_in, double fs_out, double window, int flush,
                         int64_t* frames_before, int64_t* frames_after, int64_t* held, int64_t* tail_rows) {
  if (!frames_before || !frames_after || !held || !tail_rows)
    return td_fail(nullptr, TD_ERR_INVALID, "td_audio_online_plan: NULL argument");
  Rates r;
  TD_TRY(check_rates(nullptr, "td_audio_online_plan", fs_in, fs_out, window, &r));
  TD_REQUIRE(nullptr, rows_before >= 0 && n >= 0, "td_audio_online_plan: %lld rows behind %lld", (long long)n,
             (long long)rows_before);
  PushPlan p;
  plan_push(r, rows_before, n, flush, &p);
  *frames_before = p.e0;
  *frames_after = p.e1;
  *held = p.held;
  *tail_rows = r.k_rows;
  return TD_OK;
}

int td_audio_online_state_bytes(int c, int64_t tail_rows, int64_t* bytes) {
  if (!bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_audio_online_state_bytes: NULL argument");
  TD_REQUIRE(nullptr, c >= 1 && c <= kMaxChannels, "td_audio_online_state_bytes: %d channels (1 .. %d)", c,
             kMaxChannels);
  TD_REQUIRE(nullptr, tail_rows >= 1 && tail_rows <= TD_AUDIO_ONLINE_MAX_TAIL,
             "td_audio_online_state_bytes: %lld carried rows (1 .. %d)", (long long)tail_rows, TD_AUDIO_ONLINE_MAX_TAIL);
  *bytes = state_bytes(c, tail_rows);
  return TD_OK;
}

int td_audio_online_push(td_handle* h, int num_sessions, const void* x_dev, int x_type, int64_t ldx,
                         int64_t x_session_stride, int64_t n, int c, int64_t rows_before, int flush, double fs_in,
                         double fs_out, double window, double exponent, void* state_dev,
                         int64_t state_session_stride, int live, float* out32_dev, double* out64_dev, int64_t ldout,
                         int64_t out_session_stride, int64_t* windows_dev) {
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_audio_online_push: handle is NULL");
  TD_REQUIRE(h, num_sessions >= 1 && num_sessions <= 65535, "td_audio_online_push: %d sessions (1 .. 65535)",
             num_sessions);
  TD_REQUIRE(h, c >= 1 && c <= kMaxChannels, "td_audio_online_push: %d channels (1 .. %d)", c, kMaxChannels);
  TD_REQUIRE(h, x_type == TD_AUDIO_X_I16 || x_type == TD_AUDIO_X_F32 || x_type == TD_AUDIO_X_F64,
             "td_audio_online_push: an input type of %d (0 int16, 1 float32, 2 float64)", x_type);
  Rates r;
  TD_TRY(check_rates(h, "td_audio_online_push", fs_in, fs_out, window, &r));
  TD_REQUIRE(h, n >= 0 && n <= TD_ONLINE_MAX_PUSH, "td_audio_online_push: %lld rows in one push (0 .. %d)",
             (long long)n, TD_ONLINE_MAX_PUSH);
  TD_REQUIRE(h, rows_before >= 0, "td_audio_online_push: %lld rows before", (long long)rows_before);
  TD_REQUIRE(h, live == 0 || live == 1, "td_audio_online_push: live tail copy %d (0 or 1)", live);
  if (!state_dev || (!out32_dev && !out64_dev) || (n > 0 && !x_dev))
    return td_fail(h, TD_ERR_INVALID, "td_audio_online_push: NULL argument");
  TD_REQUIRE(h, ldx >= c && ldout >= c,
             "td_audio_online_push: a row stride below a row (%lld in, %lld out for %d channels)", (long long)ldx,
             (long long)ldout, c);
  TD_REQUIRE(h, num_sessions == 1 || (x_session_stride >= c && out_session_stride >= c),
             "td_audio_online_push: a session stride below a row");
  const long long sbytes = state_bytes(c, r.k_rows);
  TD_REQUIRE(h, state_session_stride >= sbytes && state_session_stride % 8 == 0,
             "td_audio_online_push: a state stride of %lld bytes (a multiple of 8, at least %lld)",
             (long long)state_session_stride, sbytes);
  PushPlan pl;
  plan_push(r, rows_before, n, flush, &pl);
  const long long emitted = pl.e1 - pl.e0;
  TD_REQUIRE(h, emitted <= TD_ONLINE_MAX_PUSH, "td_audio_online_push: %lld frames from one push (0 .. %d)", emitted,
             TD_ONLINE_MAX_PUSH);
  if (emitted > 0) {                               // (the bound on K, checked where it matters: no read before the tail)
    long long a, u;
    window_raw(pl.e0, r.fs_in, r.fs_out, r.hw, a, u);
    TD_REQUIRE(h, (a < 0 ? 0 : a) >= rows_before - r.k_rows,
               "td_audio_online_push: frame %lld reaches back to row %lld, behind the %lld carried rows", pl.e0, a,
               r.k_rows);
  }
  if (n == 0 && emitted == 0) return TD_OK;

  AudioParams p;
  memset(&p, 0, sizeof(p));
  p.x = x_dev; p.ldx = ldx; p.x_ss = num_sessions > 1 ? x_session_stride : 0;
  p.n = n; p.rows_before = rows_before; p.e0 = pl.e0; p.emitted = (int)emitted; p.c = c; p.k_rows = (int)r.k_rows;
  p.fs_in = r.fs_in; p.fs_out = r.fs_out; p.hw = r.hw; p.expo = exponent;
  float* copies = reinterpret_cast<float*>(state_dev);
  p.tail_in = copies + (long long)live * r.k_rows * c;
  p.tail_out = copies + (long long)(1 - live) * r.k_rows * c;
  p.state_ss = state_session_stride / 4;
  p.out32 = out32_dev; p.out64 = out64_dev; p.ldout = ldout; p.out_ss = num_sessions > 1 ? out_session_stride : 0;
  p.win = reinterpret_cast<long long*>(windows_dev);
  p.post_blocks = (int)td_ceil_div(emitted, kWaves);
  long long tail_blocks = 0;
  if (n > 0) {
    tail_blocks = td_ceil_div(r.k_rows * c, kThreads);
    if (tail_blocks > kTailBlocks) tail_blocks = kTailBlocks;
  }
  const dim3 grid((unsigned)(p.post_blocks + tail_blocks), (unsigned)num_sessions);
  TD_TRY(td_profile_mark(h, true, (double)n * num_sessions));
  if (x_type == TD_AUDIO_X_I16) hipLaunchKernelGGL(audio_online_kernel<short>, grid, dim3(kThreads), 0, h->stream, p);
  else if (x_type == TD_AUDIO_X_F32) hipLaunchKernelGGL(audio_online_kernel<float>, grid, dim3(kThreads), 0, h->stream, p);
  else hipLaunchKernelGGL(audio_online_kernel<double>, grid, dim3(kThreads), 0, h->stream, p);
  TD_HIP(h, hipGetLastError());
  TD_TRY(td_profile_mark(h, false, 0.0));
  return TD_OK;
}

}  // extern "C"
