// audio.hip -- the audio features of the reference's preprocess.AudioFeatures (preprocess.py:589-755) on the
// device: the windowed-mean intensity envelope (audio_resample / compute_intensity) and the auditory
// spectrogram (compute_spectrogram).
//
// Intensity.  Row i of the output is the mean over rows [t1_i, t2_i) of the virtual concatenation
// [buffer ; f(x)], f(x) = float32(x)^2 (squared in float32, as numpy does) or x itself; the sum runs in
// float64 and sqrt / ** exponent are fused into the store.  The window bounds are computed here, in float64
// and in the reference's order of operations (rint is Python's half-even round).  One wave reduces one output
// frame's contiguous span straight from global memory with 16-B loads (1, 2 or 4 contiguous channels; any
// other layout takes a lane-per-channel form); overlapping spans (window > 1) are re-read from L2.
//
// Spectrogram.  scipy's STFT of the pre-emphasised wave restated as a matrix product on the float64 matrix
// cores: A [T, seg] holds the frames (pre-emphasis and the boundary padding applied while a run of 64
// overlapping frames is staged in LDS), B [seg, K] the cos / sin table with the Hamming window and scipy's
// 1 / sum(window) folded in, built on the host with the angle reduced exactly as (k n) mod nfft and kept on
// the device per (seg, nfft).  |A B|^2 goes to a float64 [K, T] buffer; a second kernel applies the
// smoothing FIR along k and then along t and leaves per-block max / min; a third compresses and scales.
// The maximum of the compressed spectrum is f(max P) with the increasing f(p) = (off + p)^(1/4) - off^(1/4)
// (NaN when any off + p < 0, which the minimum decides), so no fourth pass is needed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "td_common.h"
#include "td_hotpath.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }

// numpy's scalar-power fast paths (1, 2, 0.5, 0, -1), pow otherwise
__device__ __forceinline__ double pow_e(double v, double e) {
  if (e == 1.0) return v;
  if (e == 2.0) return v * v;
  if (e == 0.5) return sqrt(v);
  if (e == 0.0) return 1.0;
  if (e == -1.0) return 1.0 / v;
  return pow(v, e);
}

__device__ __forceinline__ float pow_ef(float v, float e) {
  if (e == 1.0f) return v;
  if (e == 2.0f) return v * v;
  if (e == 0.5f) return sqrtf(v);
  if (e == 0.0f) return 1.0f;
  if (e == -1.0f) return 1.0f / v;
  return powf(v, e);
}

template <bool SQ, typename T>
__device__ __forceinline__ double feature(T v) {
  if (SQ) {
#pragma clang fp contract(off)
    const float f = (float)v;
    return (double)(f * f);
  }
  return (double)v;
}

// The reference's window of output row i (preprocess.py:657-661), float64 in its order of operations.
__device__ __forceinline__ void window_of(long long i, double fs_in, double fs_out, double hw, long long tau,
                                          long long frames_in, long long& t1, long long& t2) {
#pragma clang fp contract(off)
  const double t = (double)i / fs_out;
  t1 = (long long)rint(fs_in * (t - hw)) + tau;
  t2 = (long long)rint(fs_in * (t + hw)) + tau;
  t1 = t1 < 0 ? 0 : t1;
  t2 = t2 > frames_in ? frames_in : t2;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double finish(double sum, long long cnt, int post, double expo) {
  if (cnt <= 0) return qnan();        // np.mean of an empty slice
  double v = sum / (double)cnt;
  if (post) v = pow_e(sqrt(v), expo);
  return v;
}

// C in {1, 2, 4}, x contiguous (ldx == C) and 16-B aligned: one wave per output row.  Element e of the flat
// span has channel e % C; a lane's scalar elements all sit at lane + 64 j from a multiple of C (channel
// lane % C), and element p of an aligned 4-element group has channel p % C.
template <int C, bool SQ, typename T>
__global__ void __launch_bounds__(kThreads)
intensity_vec_kernel(const double* __restrict__ buf, long long nb, const T* __restrict__ x, long long nx,
                     long long m, double fs_in, double fs_out, double hw, int post, double expo,
                     double* __restrict__ out, long long* __restrict__ win) {
  const long long i = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= m) return;
  long long t1, t2;
  window_of(i, fs_in, fs_out, hw, nb, nb + nx, t1, t2);
  double s = 0.0, v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  if (t1 < t2) {
    const long long be = t2 < nb ? t2 : nb;            // buffer rows [t1, be)
    for (long long e = t1 * C + lane; e < be * C; e += 64) s += buf[e];
    const long long x1 = (t1 > nb ? t1 : nb) - nb, x2 = t2 - nb;   // rows of x
    if (x2 > x1) {
      const long long e1 = x1 * C, e2 = x2 * C;
      const long long a = (e1 + 3) & ~3LL, b = e2 & ~3LL;
      if (a >= b) {
        for (long long e = e1 + lane; e < e2; e += 64) s += feature<SQ>(x[e]);
      } else {
        if (lane < a - e1) s += feature<SQ>(x[e1 + lane]);
        if (lane < e2 - b) s += feature<SQ>(x[b + lane]);
#pragma unroll 4
        for (long long j = (a >> 2) + lane; j < (b >> 2); j += 64) {
          if constexpr (sizeof(T) == 4) {
            const float4 q = *reinterpret_cast<const float4*>(x + 4 * j);
            v0 += feature<SQ>(q.x); v1 += feature<SQ>(q.y); v2 += feature<SQ>(q.z); v3 += feature<SQ>(q.w);
          } else {
            const double2 q0 = *reinterpret_cast<const double2*>(x + 4 * j);
            const double2 q1 = *reinterpret_cast<const double2*>(x + 4 * j + 2);
            v0 += feature<SQ>(q0.x); v1 += feature<SQ>(q0.y); v2 += feature<SQ>(q1.x); v3 += feature<SQ>(q1.y);
          }
        }
      }
    }
  }
  const long long cnt = t2 - t1;
  if (C == 1) {
    const double tot = wave_sum(s + ((v0 + v1) + (v2 + v3)));
    if (lane == 0) out[i] = finish(tot, cnt, post, expo);
  } else if (C == 2) {
    const double c0 = wave_sum((lane & 1 ? 0.0 : s) + v0 + v2);
    const double c1 = wave_sum((lane & 1 ? s : 0.0) + v1 + v3);
    if (lane == 0) { out[2 * i] = finish(c0, cnt, post, expo); out[2 * i + 1] = finish(c1, cnt, post, expo); }
  } else {
    const int ch = lane & 3;
    const double c0 = wave_sum((ch == 0 ? s : 0.0) + v0);
    const double c1 = wave_sum((ch == 1 ? s : 0.0) + v1);
    const double c2 = wave_sum((ch == 2 ? s : 0.0) + v2);
    const double c3 = wave_sum((ch == 3 ? s : 0.0) + v3);
    if (lane < 4) {
      const double c = lane == 0 ? c0 : lane == 1 ? c1 : lane == 2 ? c2 : c3;
      out[4 * i + lane] = finish(c, cnt, post, expo);
    }
  }
  if (win && lane == 0) { win[2 * i] = t1; win[2 * i + 1] = t2; }
}

// Any channel count and row stride: one wave per output row, a lane per channel, rows in order.
template <bool SQ, typename T>
__global__ void __launch_bounds__(kThreads)
intensity_any_kernel(const double* __restrict__ buf, long long nb, const T* __restrict__ x, long long ldx,
                     long long nx, int c_count, long long m, double fs_in, double fs_out, double hw, int post,
                     double expo, double* __restrict__ out, long long* __restrict__ win) {
  const long long i = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= m) return;
  long long t1, t2;
  window_of(i, fs_in, fs_out, hw, nb, nb + nx, t1, t2);
  for (int c = lane; c < c_count; c += 64) {
    double s = 0.0;
    for (long long r = t1; r < t2; ++r)
      s += r < nb ? buf[r * c_count + c] : feature<SQ>(x[(r - nb) * ldx + c]);
    out[i * c_count + c] = finish(s, t2 - t1, post, expo);
  }
  if (win && lane == 0) { win[2 * i] = t1; win[2 * i + 1] = t2; }
}

// Rows [r0, r1) of [buffer ; f(x)], as float32 (sqrt and ** exponent in float32) or float64.
template <bool SQ, typename T>
__global__ void __launch_bounds__(kThreads)
passthrough_kernel(const double* __restrict__ buf, long long nb, const T* __restrict__ x, long long ldx,
                   int c_count, long long r0, long long total, int post, double expo, float* __restrict__ o32,
                   double* __restrict__ o64) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= total) return;
  const long long r = r0 + g / c_count;
  const int c = (int)(g % c_count);
  const double v = r < nb ? buf[r * c_count + c] : feature<SQ>(x[(r - nb) * ldx + c]);
  if (o32) {
    float f = (float)v;
    if (post) f = pow_ef(sqrtf(f), (float)expo);
    o32[g] = f;
  } else if (post == 2) {   // float32 data whose ** exponent numpy promotes: sqrt in float32, the power in float64
    o64[g] = pow_e((double)sqrtf((float)v), expo);
  } else {
    o64[g] = post ? pow_e(sqrt(v), expo) : v;
  }
}

// ---------------------------------------------------------------------------------------------------------
// Spectrogram
constexpr int kMaxSeg = 1024;
constexpr int kMaxNfft = 4096;
constexpr int kMaxTaps = 16;
constexpr int kFrames = 64;        // frames per workgroup of the DFT (4 MFMA row tiles)
constexpr int kNc = 64;            // samples per LDS stage of the DFT
constexpr int kLs = kNc + 2;       // LDS row stride in doubles (conflict-free operand reads)
constexpr int kFirK = 16, kFirT = 64;

// The pre-emphasised, boundary-padded signal at padded position p (scipy's zero extension of seg // 2 at each
// end, then the zero tail of `padded`): pe[0] = w[0], pe[i] = w[i] - 0.95 w[i-1] in float64 (lfilter).
__device__ __forceinline__ double padded_pe(const float* __restrict__ w, long long n, long long pad, long long p) {
#pragma clang fp contract(off)
  const long long i = p - pad;
  if (i < 0 || i >= n) return 0.0;
  const double cur = (double)w[i];
  return i == 0 ? cur : cur + (-0.95 * (double)w[i - 1]);
}

// grid (frame blocks, groups of 4 k tiles); wave w of group g owns k tile 4 g + w (16 bins).  B is [segp][kp]
// cos then [segp][kp] sin.  power [K, T].
__global__ void __launch_bounds__(kThreads)
spec_dft_kernel(const float* __restrict__ w, long long n, long long pad, int seg, int segp, int hop, long long frames,
                const double* __restrict__ bcos, int kp, int k_bins, double* __restrict__ power) {
  __shared__ double as[kFrames * kLs];
  const double* bsin = bcos + (long long)segp * kp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
  const long long t0 = (long long)blockIdx.x * kFrames;
  const int ktile = blockIdx.y * kWaves + wave;
  const bool active = ktile * 16 < kp;
  f64x4 re[4], im[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) { re[mt] = f64x4{0, 0, 0, 0}; im[mt] = f64x4{0, 0, 0, 0}; }
  for (int n0 = 0; n0 < segp; n0 += kNc) {
    for (int e = threadIdx.x; e < kFrames * kNc; e += kThreads) {
      const int tt = e / kNc, nn = e - tt * kNc;
      const long long t = t0 + tt;
      const int s = n0 + nn;
      as[tt * kLs + nn] = (t < frames && s < seg) ? padded_pe(w, n, pad, t * hop + s) : 0.0;
    }
    __syncthreads();
    if (active) {
      const double* bc = bcos + (long long)n0 * kp + ktile * 16 + li;
      const double* bs = bsin + (long long)n0 * kp + ktile * 16 + li;
#pragma unroll 4
      for (int q = 0; q < kNc / 4; ++q) {
        const int kk = 4 * q + lk;
        const double b0 = bc[(long long)kk * kp], b1 = bs[(long long)kk * kp];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          const double a = as[(16 * mt + li) * kLs + kk];
          re[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, re[mt], 0, 0, 0);
          im[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, im[mt], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  if (!active) return;
  const int k = ktile * 16 + li;                  // C/D map: col = lane & 15, row = (lane >> 4) + 4 reg
  if (k >= k_bins) return;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long t = t0 + 16 * mt + lk + 4 * r;
      if (t < frames) power[(long long)k * frames + t] = re[mt][r] * re[mt][r] + im[mt][r] * im[mt][r];
    }
}

struct Taps {
  double h[kMaxTaps];
};

__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double nan_min(double a, double b) { return (a < b || a != a) ? a : b; }

// The causal FIR (lfilter(h, [1]), zero initial state) along k, then along t, over a 16 x 64 tile with its
// (taps - 1) halo; out [K, T], part[block] = (max, min) of the tile.
__global__ void __launch_bounds__(kThreads)
spec_fir_kernel(const double* __restrict__ power, int k_bins, long long frames, Taps tp, int nt,
                double* __restrict__ out, double* __restrict__ part) {
  constexpr int kH = kMaxTaps - 1;
  __shared__ double ps[(kFirK + kH) * (kFirT + kH)];
  __shared__ double qs[kFirK * (kFirT + kH)];
  __shared__ double red[2 * kWaves];
  const int hl = nt - 1;
  const int pw = kFirT + hl;                       // tile width with halo
  const int k0 = blockIdx.y * kFirK;
  const long long t0 = (long long)blockIdx.x * kFirT;
  for (int e = threadIdx.x; e < (kFirK + hl) * pw; e += kThreads) {
    const int kk = e / pw, tt = e - kk * pw;
    const int k = k0 - hl + kk;
    const long long t = t0 - hl + tt;
    ps[e] = (k >= 0 && k < k_bins && t >= 0 && t < frames) ? power[(long long)k * frames + t] : 0.0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kFirK * pw; e += kThreads) {     // along k
    const int kk = e / pw, tt = e - kk * pw;
    double acc = tp.h[hl] * ps[kk * pw + tt];
    for (int j = hl - 1; j >= 0; --j) acc = tp.h[j] * ps[(kk + hl - j) * pw + tt] + acc;
    qs[e] = acc;
  }
  __syncthreads();
  double mx = -INFINITY, mn = INFINITY;
  for (int e = threadIdx.x; e < kFirK * kFirT; e += kThreads) {  // along t
    const int kk = e / kFirT, tt = e - kk * kFirT;
    const int k = k0 + kk;
    const long long t = t0 + tt;
    if (k >= k_bins || t >= frames) continue;
    const double* q = qs + kk * pw + tt;
    double acc = tp.h[hl] * q[0];
    for (int j = hl - 1; j >= 0; --j) acc = tp.h[j] * q[hl - j] + acc;
    out[(long long)k * frames + t] = acc;
    mx = nan_max(mx, acc);
    mn = nan_min(mn, acc);
  }
  for (int o = 32; o >= 1; o >>= 1) {
    mx = nan_max(mx, __shfl_xor(mx, o, 64));
    mn = nan_min(mn, __shfl_xor(mn, o, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[2 * wave] = mx; red[2 * wave + 1] = mn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < kWaves; ++v) { mx = nan_max(mx, red[2 * v]); mn = nan_min(mn, red[2 * v + 1]); }
    const long long b = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    part[2 * b] = mx;
    part[2 * b + 1] = mn;
  }
}

// One workgroup: the (max, min) over every block -> scale[0] = off = 1e-4 max, scale[1] = off^(1/4),
// scale[2] = 255 / max S.
__global__ void __launch_bounds__(kThreads)
spec_scale_kernel(const double* __restrict__ part, long long blocks, double* __restrict__ scale) {
  __shared__ double red[2 * kWaves];
  double mx = -INFINITY, mn = INFINITY;
  for (long long b = threadIdx.x; b < blocks; b += kThreads) {
    mx = nan_max(mx, part[2 * b]);
    mn = nan_min(mn, part[2 * b + 1]);
  }
  for (int o = 32; o >= 1; o >>= 1) {
    mx = nan_max(mx, __shfl_xor(mx, o, 64));
    mn = nan_min(mn, __shfl_xor(mn, o, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[2 * wave] = mx; red[2 * wave + 1] = mn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < kWaves; ++v) { mx = nan_max(mx, red[2 * v]); mn = nan_min(mn, red[2 * v + 1]); }
    const double off = 0.0001 * mx;
    const double off4 = pow(off, 0.25);
    const double smax = pow(off + mx, 0.25) - off4;
    const double smin = pow(off + mn, 0.25) - off4;
    scale[0] = off;
    scale[1] = off4;
    scale[2] = 255.0 / (smin != smin ? qnan() : smax);
  }
}

__global__ void __launch_bounds__(kThreads)
spec_compress_kernel(double* __restrict__ out, long long total, const double* __restrict__ scale) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= total) return;
  out[g] = scale[2] * (pow(scale[0] + out[g], 0.25) - scale[1]);
}

// The B table per (device, seg, nfft), built once and kept for the life of the process.
struct DftTable {
  double* dev = nullptr;
  int segp = 0, kp = 0;
};

int dft_table(td_handle* h, int seg, int nfft, DftTable* out) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int>, DftTable> cache;
  int dev = 0;
  TD_HIP(h, hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_tuple(dev, seg, nfft);
  auto it = cache.find(key);
  if (it != cache.end()) {
    *out = it->second;
    return TD_OK;
  }
  DftTable t;
  const int k_bins = nfft / 2 + 1;
  t.kp = (int)td_round_up(k_bins, 16);
  t.segp = (int)td_round_up(seg, kNc);
  const long double two_pi = 6.283185307179586476925286766559L;
  std::vector<double> cs(nfft), sn(nfft), win(seg);
  for (int m = 0; m < nfft; ++m) {
    cs[m] = (double)cosl(two_pi * m / nfft);
    sn[m] = (double)-sinl(two_pi * m / nfft);
  }
  double wsum = 0.0;
  for (int i = 0; i < seg; ++i) {   // periodic Hamming (scipy.signal.get_window('hamming', seg))
    win[i] = 0.54 - 0.46 * (double)cosl(two_pi * i / seg);
    wsum += win[i];
  }
  std::vector<double> host((size_t)2 * t.segp * t.kp, 0.0);
  double* hc = host.data();
  double* hs = hc + (size_t)t.segp * t.kp;
  for (int i = 0; i < seg; ++i) {
    const double wi = win[i] / wsum;   // scipy's 'spectrum' scaling, 1 / sum(window)
    for (int k = 0; k < k_bins; ++k) {
      const int m = (int)(((long long)k * i) % nfft);
      hc[(size_t)i * t.kp + k] = wi * cs[m];
      hs[(size_t)i * t.kp + k] = wi * sn[m];
    }
  }
  TD_HIP(h, hipMalloc(&t.dev, host.size() * sizeof(double)));
  TD_HIP(h, hipMemcpy(t.dev, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
  cache[key] = t;
  *out = t;
  return TD_OK;
}

template <bool SQ, typename T>
void launch_intensity(td_handle* h, const double* buf, long long nb, const T* x, long long ldx, long long n, int c,
                      long long m, double fs_in, double fs_out, double hw, int post, double expo, double* out,
                      long long* win) {
  const dim3 grid((unsigned)td_ceil_div(m, kWaves));
  const bool vec = ldx == c && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  if (vec && c == 1)
    hipLaunchKernelGGL((intensity_vec_kernel<1, SQ, T>), grid, dim3(kThreads), 0, h->stream, buf, nb, x, n, m, fs_in,
                       fs_out, hw, post, expo, out, win);
  else if (vec && c == 2)
    hipLaunchKernelGGL((intensity_vec_kernel<2, SQ, T>), grid, dim3(kThreads), 0, h->stream, buf, nb, x, n, m, fs_in,
                       fs_out, hw, post, expo, out, win);
  else if (vec && c == 4)
    hipLaunchKernelGGL((intensity_vec_kernel<4, SQ, T>), grid, dim3(kThreads), 0, h->stream, buf, nb, x, n, m, fs_in,
                       fs_out, hw, post, expo, out, win);
  else
    hipLaunchKernelGGL((intensity_any_kernel<SQ, T>), grid, dim3(kThreads), 0, h->stream, buf, nb, x, ldx, n, c, m,
                       fs_in, fs_out, hw, post, expo, out, win);
}

template <bool SQ, typename T>
void launch_passthrough(td_handle* h, const double* buf, long long nb, const T* x, long long ldx, int c, long long r0,
                        long long total, int post, double expo, float* o32, double* o64) {
  hipLaunchKernelGGL((passthrough_kernel<SQ, T>), dim3((unsigned)td_ceil_div(total, kThreads)), dim3(kThreads), 0,
                     h->stream, buf, nb, x, ldx, c, r0, total, post, expo, o32, o64);
}

}  // namespace

extern "C" {

int td_audio_intensity(td_handle* h, const double* buf_dev, int64_t buf_rows, const void* x_dev, int x_is_f64,
                       int64_t ldx, int64_t n, int c, int square, int64_t rows_out, double fs_in, double fs_out,
                       double half_window, int post, double exponent, double* out_dev, int64_t* windows_dev) {
  if (!h || (!x_dev && n > 0) || (!buf_dev && buf_rows > 0) || (!out_dev && rows_out > 0))
    return td_fail(h, TD_ERR_INVALID, "td_audio_intensity: NULL argument");
  TD_REQUIRE(h, c >= 1 && n >= 0 && buf_rows >= 0 && rows_out >= 0 && ldx >= c, "td_audio_intensity: bad sizes");
  TD_REQUIRE(h, fs_in > 0 && fs_out > 0 && half_window > 0, "td_audio_intensity: bad rates");
  if (rows_out == 0) return TD_OK;
  long long* win = reinterpret_cast<long long*>(windows_dev);
  if (x_is_f64) {
    const double* x = static_cast<const double*>(x_dev);
    if (square) launch_intensity<true>(h, buf_dev, buf_rows, x, ldx, n, c, rows_out, fs_in, fs_out, half_window, post,
                                       exponent, out_dev, win);
    else launch_intensity<false>(h, buf_dev, buf_rows, x, ldx, n, c, rows_out, fs_in, fs_out, half_window, post,
                                 exponent, out_dev, win);
  } else {
    const float* x = static_cast<const float*>(x_dev);
    if (square) launch_intensity<true>(h, buf_dev, buf_rows, x, ldx, n, c, rows_out, fs_in, fs_out, half_window, post,
                                       exponent, out_dev, win);
    else launch_intensity<false>(h, buf_dev, buf_rows, x, ldx, n, c, rows_out, fs_in, fs_out, half_window, post,
                                 exponent, out_dev, win);
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_audio_passthrough(td_handle* h, const double* buf_dev, int64_t buf_rows, const void* x_dev, int x_is_f64,
                         int64_t ldx, int64_t n, int c, int square, int64_t row_begin, int64_t row_end, int post,
                         double exponent, float* out32_dev, double* out64_dev) {
  if (!h || (!x_dev && n > 0) || (!buf_dev && buf_rows > 0) || (!out32_dev == !out64_dev))
    return td_fail(h, TD_ERR_INVALID, "td_audio_passthrough: NULL argument (or both outputs)");
  TD_REQUIRE(h, c >= 1 && n >= 0 && buf_rows >= 0 && ldx >= c, "td_audio_passthrough: bad sizes");
  TD_REQUIRE(h, 0 <= row_begin && row_begin <= row_end && row_end <= buf_rows + n,
             "td_audio_passthrough: rows [%lld, %lld) outside [0, %lld)", (long long)row_begin, (long long)row_end,
             (long long)(buf_rows + n));
  const long long total = (row_end - row_begin) * (long long)c;
  if (total == 0) return TD_OK;
  if (x_is_f64) {
    const double* x = static_cast<const double*>(x_dev);
    if (square) launch_passthrough<true>(h, buf_dev, buf_rows, x, ldx, c, row_begin, total, post, exponent, out32_dev,
                                         out64_dev);
    else launch_passthrough<false>(h, buf_dev, buf_rows, x, ldx, c, row_begin, total, post, exponent, out32_dev,
                                   out64_dev);
  } else {
    const float* x = static_cast<const float*>(x_dev);
    if (square) launch_passthrough<true>(h, buf_dev, buf_rows, x, ldx, c, row_begin, total, post, exponent, out32_dev,
                                         out64_dev);
    else launch_passthrough<false>(h, buf_dev, buf_rows, x, ldx, c, row_begin, total, post, exponent, out32_dev,
                                   out64_dev);
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_audio_spectrogram(td_handle* h, const float* wave_dev, int64_t n, int seg, int hop, int nfft,
                         const double* taps_host, int num_taps, int64_t frames, double* out_dev) {
  if (!h || !wave_dev || !taps_host || !out_dev) return td_fail(h, TD_ERR_INVALID, "td_audio_spectrogram: NULL argument");
  TD_REQUIRE(h, seg >= 1 && seg <= kMaxSeg, "td_audio_spectrogram: segment length %d outside [1, %d]", seg, kMaxSeg);
  TD_REQUIRE(h, nfft >= seg && nfft <= kMaxNfft, "td_audio_spectrogram: nfft %d outside [segment, %d]", nfft, kMaxNfft);
  TD_REQUIRE(h, num_taps >= 1 && num_taps <= kMaxTaps, "td_audio_spectrogram: %d smoothing taps outside [1, %d]",
             num_taps, kMaxTaps);
  TD_REQUIRE(h, hop >= 1 && hop <= seg && n >= seg, "td_audio_spectrogram: bad hop / length");
  TD_REQUIRE(h, frames >= 1, "td_audio_spectrogram: no frames");   // (positions past the wave read as zeros)
  const long long pad = seg / 2;
  DftTable tab;
  TD_TRY(dft_table(h, seg, nfft, &tab));
  const int k_bins = nfft / 2 + 1;
  const long long fir_bt = td_ceil_div(frames, kFirT), fir_bk = td_ceil_div(k_bins, kFirK);
  const long long cells = (long long)k_bins * frames;
  void* scratch = nullptr;
  TD_TRY(td_scratch(h, (size_t)(cells + 2 * fir_bt * fir_bk + 4) * sizeof(double), &scratch));
  double* power = static_cast<double*>(scratch);
  double* part = power + cells;
  double* scale = part + 2 * fir_bt * fir_bk;
  const int ktiles = tab.kp / 16;
  hipLaunchKernelGGL(spec_dft_kernel, dim3((unsigned)td_ceil_div(frames, kFrames), (unsigned)td_ceil_div(ktiles, kWaves)),
                     dim3(kThreads), 0, h->stream, wave_dev, (long long)n, pad, seg, tab.segp, hop, (long long)frames,
                     tab.dev, tab.kp, k_bins, power);
  Taps tp{};
  for (int j = 0; j < num_taps; ++j) tp.h[j] = taps_host[j];
  hipLaunchKernelGGL(spec_fir_kernel, dim3((unsigned)fir_bt, (unsigned)fir_bk), dim3(kThreads), 0, h->stream, power,
                     k_bins, (long long)frames, tp, num_taps, out_dev, part);
  hipLaunchKernelGGL(spec_scale_kernel, dim3(1), dim3(kThreads), 0, h->stream, part, fir_bt * fir_bk, scale);
  hipLaunchKernelGGL(spec_compress_kernel, dim3((unsigned)td_ceil_div(cells, kThreads)), dim3(kThreads), 0, h->stream,
                     out_dev, cells, scale);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

}  // extern "C"
