// preprocess.hip -- the signal conditioning of the reference's preprocess.Preprocessor
// (preprocess.py:54-587) on the device: a state-carrying cascade of second-order IIR sections
// (scipy.signal.sosfilt in float64, preprocess.py:293-352) with the nearest-neighbour resample fused
// into its store (:376-389), re-referencing by groups + channel selection (:417-443) in one pass, a
// float64 mean (:445-461), and normalisation + temporal context (:463-527) in one pass.
//
// The filter.  Per channel the cascade of S sections (direct form II transposed, scipy's update
// order) is a linear recurrence in its D = 2S state: s' = A s + B x.  A time chunk of L samples run
// from a zero state ends at e_k; its true start state then follows from an affine scan with the
// constant matrix P = A^L:  start(k) = P start(k-1) + e_(k-1),  start(0) = the file's initial state.
//   1. sos_chunk_end_kernel: every (chunk, channel) lane filters its chunk from zero; keeps only e_k.
//   2. the scan, hierarchical: lanes over (block of G chunks, channel) scan their block serially
//      (sos_scan_local_kernel), the block totals are scanned the same way with P^G (recursively), and
//      sos_scan_fix_kernel adds P^(j+1) x (state before the block) to the j-th item of every block.
//   3. sos_chunk_out_kernel: every lane re-runs its chunk from its true start state and stores the
//      output rows the resample keeps (all rows without one); the last chunk leaves the final state.
// Lanes go over (chunk, channel) pairs with the channel fastest: a row of 64 channels is one
// coalesced 256-B (float32) load, and one channel (an audio envelope) still fills whole waves with
// chunks.
// The scan is compensated.  P is strongly non-normal for a narrow high-pass (poles near z = 1: ||P^j|| up to
// 1e37 at 16 + 16 sections), and a plain float64 scan left outputs ~1e-8 of max|x| away from the sequential
// filter at fixed positions in the blocks.  So the host builds P^j in long double and
// stores each as an unevaluated sum hi + lo of two doubles, every scan item is such a pair, and the scan
// kernels carry P acc + e in double-double arithmetic (error-free products and sums).  The two passes over
// x stay in plain float64: each chunk's start state is rounded once to the nearest double.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "td_common.h"
#include "td_hotpath.h"

namespace {

constexpr int kMaxSections = 16;
constexpr int kScanGroup = 64;        // G: chunks per block of the hierarchical scan
constexpr int kThreads = 256;

// b0 b1 b2 a1 a2 per section (a0 = 1), passed by value: uniform across lanes (scalar loads)
struct SosCoef {
  double c[kMaxSections][5];
  double zi[kMaxSections][2];
};

template <int S>
__device__ __forceinline__ double sos_step(const SosCoef& k, double (&z)[2 * S], double x) {
#pragma unroll
  for (int i = 0; i < S; ++i) {   // scipy _sosfilt: y = b0 x + z0; z0 = b1 x - a1 y + z1; z1 = b2 x - a2 y
    const double y = k.c[i][0] * x + z[2 * i];
    z[2 * i] = k.c[i][1] * x - k.c[i][3] * y + z[2 * i + 1];
    z[2 * i + 1] = k.c[i][2] * x - k.c[i][4] * y;
    x = y;
  }
  return x;
}

template <typename T>
__device__ __forceinline__ double load_x(const T* x, long long ldx, long long row, int c) {
  return (double)x[row * ldx + c];
}

// Item k of a scan buffer: D x C doubles, [j][c] -- the [S, 2, C] layout of scipy's zi -- holding the high
// parts of the double-double values; their low parts sit `lo` doubles further on.
template <int S, typename T>
__global__ void __launch_bounds__(kThreads)
sos_chunk_end_kernel(const T* __restrict__ x, long long ldx, int c_count, int chunk, long long lanes,
                     SosCoef k, double* __restrict__ items, long long lo) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= lanes) return;
  const long long ck = g / c_count;
  const int c = (int)(g - ck * c_count);
  double z[2 * S];
#pragma unroll
  for (int j = 0; j < 2 * S; ++j) z[j] = 0.0;
  const long long t0 = ck * chunk;
  for (int t = 0; t < chunk; ++t) sos_step<S>(k, z, load_x(x, ldx, t0 + t, c));
  double* dst = items + (ck + 1) * (2 * S) * (long long)c_count + c;   // item k+1 holds e_k
#pragma unroll
  for (int j = 0; j < 2 * S; ++j) {
    dst[(long long)j * c_count] = z[j];
    dst[(long long)j * c_count + lo] = 0.0;
  }
}

// Item 0: the file's initial state.  reset: sections [0, split) from x[0] * zi, sections [split, S)
// from y0 * zi where y0 is the first output of sections [0, split) (the low-pass is reset from the
// high-pass OUTPUT's first row, preprocess.py:293-352).  Otherwise the carried state [S, 2, C].
template <int S, typename T>
__global__ void __launch_bounds__(kThreads)
sos_init_kernel(const T* __restrict__ x, int c_count, SosCoef k, int split, int reset,
                const double* __restrict__ state, double* __restrict__ item0, long long lo) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= c_count) return;
  for (int j = 0; j < 2 * S; ++j) item0[(long long)j * c_count + c + lo] = 0.0;
  if (!reset) {
    for (int j = 0; j < 2 * S; ++j) item0[(long long)j * c_count + c] = state[(long long)j * c_count + c];
    return;
  }
  const double x0 = (double)x[c];
  double y0 = x0;
  for (int i = 0; i < split; ++i)       // one step of the first stage from its reset state
    y0 = k.c[i][0] * y0 + x0 * k.zi[i][0];
  for (int i = 0; i < S; ++i) {
    const double v = i < split ? x0 : y0;
    item0[(long long)(2 * i) * c_count + c] = v * k.zi[i][0];
    item0[(long long)(2 * i + 1) * c_count + c] = v * k.zi[i][1];
  }
}

// ---- double-double arithmetic (value = hi + lo, |lo| <= ulp(hi) / 2) --------------------------------
// Contraction stays off here: a product fused into a neighbouring sum would break the error-free terms.
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
#pragma clang fp contract(off)
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// (h, l) += (ph, pl) x (vh, vl): the product ph vh exact (fma), the cross terms and the sum's error into l.
__device__ __forceinline__ void dd_mac(double& h, double& l, double ph, double pl, double vh, double vl) {
#pragma clang fp contract(off)
  const double m = ph * vh;
  const double me = __builtin_fma(ph, vh, -m);
  double s, e;
  two_sum(h, m, s, e);
  h = s;
  l += e + (me + __builtin_fma(ph, vl, pl * vh));
}

__device__ __forceinline__ void dd_norm(double& h, double& l) {
#pragma clang fp contract(off)
  const double s = h + l;
  l = l - (s - h);
  h = s;
}

// acc += P v in double-double; P row-major D x D, its low parts pl_off doubles after its high parts.
template <int S>
__device__ __forceinline__ void matvec_add_dd(const double* __restrict__ p, long long pl_off,
                                              const double (&vh)[2 * S], const double (&vl)[2 * S],
                                              double (&ah)[2 * S], double (&al)[2 * S]) {
#pragma unroll
  for (int r = 0; r < 2 * S; ++r) {
    double h = ah[r], l = al[r];
#pragma unroll
    for (int q = 0; q < 2 * S; ++q) dd_mac(h, l, p[r * 2 * S + q], p[r * 2 * S + q + pl_off], vh[q], vl[q]);
    dd_norm(h, l);
    ah[r] = h;
    al[r] = l;
  }
}

// Lanes over (block b, channel): items [bG, bG + G) become inclusive prefixes out_k = P out_(k-1) + v_k
// within the block; tot[b] (if given) receives the block's last prefix.  Items, tot: low parts lo doubles
// on; p: P^1 of this level, low parts pl_off doubles on.
template <int S>
__global__ void __launch_bounds__(kThreads)
sos_scan_local_kernel(double* __restrict__ items, long long lo, long long n_items, int c_count, long long lanes,
                      const double* __restrict__ p, long long pl_off, double* __restrict__ tot) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= lanes) return;
  const long long b = g / c_count;
  const int c = (int)(g - b * c_count);
  constexpr int D = 2 * S;
  const long long k0 = b * kScanGroup;
  const long long k1 = k0 + kScanGroup < n_items ? k0 + kScanGroup : n_items;
  double ah[D], al[D];
  const double* it = items + k0 * D * (long long)c_count + c;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    ah[j] = it[(long long)j * c_count];
    al[j] = it[(long long)j * c_count + lo];
  }
  for (long long kk = k0 + 1; kk < k1; ++kk) {
    double* cur = items + kk * D * (long long)c_count + c;
    double nh[D], nl[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      nh[j] = cur[(long long)j * c_count];
      nl[j] = cur[(long long)j * c_count + lo];
    }
    matvec_add_dd<S>(p, pl_off, ah, al, nh, nl);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      ah[j] = nh[j];
      al[j] = nl[j];
      cur[(long long)j * c_count] = nh[j];
      cur[(long long)j * c_count + lo] = nl[j];
    }
  }
  if (tot) {
    double* dst = tot + b * D * (long long)c_count + c;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      dst[(long long)j * c_count] = ah[j];
      dst[(long long)j * c_count + lo] = al[j];
    }
  }
}

// Lanes over (item k >= G, channel): item k += P^(j+1) tot[b-1], b = k / G, j = k % G, where tot holds the
// block totals after their own (inclusive) scan: the true prefix at the end of block b-1.
template <int S>
__global__ void __launch_bounds__(kThreads)
sos_scan_fix_kernel(double* __restrict__ items, long long lo, long long n_items, int c_count, long long lanes,
                    const double* __restrict__ ppow, long long pl_off, const double* __restrict__ tot) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= lanes) return;
  constexpr int D = 2 * S;
  const long long kk = kScanGroup + g / c_count;
  const int c = (int)(g % c_count);
  const long long b = kk / kScanGroup;
  const int j = (int)(kk - b * kScanGroup);
  const double* prev = tot + (b - 1) * D * (long long)c_count + c;
  double vh[D], vl[D], ah[D], al[D];
  double* cur = items + kk * D * (long long)c_count + c;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    vh[q] = prev[(long long)q * c_count];
    vl[q] = prev[(long long)q * c_count + lo];
    ah[q] = cur[(long long)q * c_count];
    al[q] = cur[(long long)q * c_count + lo];
  }
  matvec_add_dd<S>(ppow + (long long)j * D * D, pl_off, vh, vl, ah, al);
#pragma unroll
  for (int q = 0; q < D; ++q) {
    cur[(long long)q * c_count] = ah[q];
    cur[(long long)q * c_count + lo] = al[q];
  }
}

__device__ __forceinline__ long long lower_bound_rows(const long long* rows, long long m, long long t) {
  long long lo = 0, hi = m;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (rows[mid] < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Lanes over (chunk, channel): the chunk from its true start state; output row i of the file is
// input row rows[i] (rows nondecreasing; nullptr: every row).  final_state: the last chunk's end.
template <int S, typename T>
__global__ void __launch_bounds__(kThreads)
sos_chunk_out_kernel(const T* __restrict__ x, long long ldx, int c_count, long long n, int chunk,
                     long long lanes, SosCoef k, const double* __restrict__ items, long long lo,
                     const long long* __restrict__ rows, long long m, double* __restrict__ y, long long ldy,
                     double* __restrict__ final_state) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= lanes) return;
  const long long ck = g / c_count;
  const int c = (int)(g - ck * c_count);
  double z[2 * S];
  const double* it = items + ck * (2 * S) * (long long)c_count + c;
#pragma unroll
  for (int j = 0; j < 2 * S; ++j) z[j] = it[(long long)j * c_count] + it[(long long)j * c_count + lo];
  const long long t0 = ck * chunk;
  const long long t1 = t0 + chunk < n ? t0 + chunk : n;
  if (rows) {
    long long i = lower_bound_rows(rows, m, t0);
    long long next = i < m ? rows[i] : n;
    for (long long t = t0; t < t1; ++t) {
      const double v = sos_step<S>(k, z, load_x(x, ldx, t, c));
      while (next == t) {           // (upsampling repeats a row)
        y[i * ldy + c] = v;
        ++i;
        next = i < m ? rows[i] : n;
      }
    }
  } else {
    for (long long t = t0; t < t1; ++t) y[t * ldy + c] = sos_step<S>(k, z, load_x(x, ldx, t, c));
  }
  if (final_state && t1 == n) {
#pragma unroll
    for (int j = 0; j < 2 * S; ++j) final_state[(long long)j * c_count + c] = z[j];
  }
}

// ---- host: the cascade's state-transition matrix and its powers ----------------------------------
// (long double: the x86-64 host's 64-bit significand, 11 bits past a double's)
using ldouble = long double;

void step_host(const double* sos, int s_count, ldouble* z, ldouble x) {
  for (int i = 0; i < s_count; ++i) {
    const double* c = sos + 6 * i;
    const ldouble y = c[0] * x + z[2 * i];
    z[2 * i] = c[1] * x - c[4] * y + z[2 * i + 1];
    z[2 * i + 1] = c[2] * x - c[5] * y;
    x = y;
  }
}

void matmul(const std::vector<ldouble>& a, const std::vector<ldouble>& b, int d, std::vector<ldouble>* out) {
  std::vector<ldouble> r((size_t)d * d, 0.0L);
  for (int i = 0; i < d; ++i)
    for (int q = 0; q < d; ++q) {
      const ldouble aiq = a[(size_t)i * d + q];
      if (aiq == 0.0L) continue;
      for (int j = 0; j < d; ++j) r[(size_t)i * d + j] += aiq * b[(size_t)q * d + j];
    }
  *out = std::move(r);
}

std::vector<ldouble> mat_pow(const std::vector<ldouble>& a, int d, long long e) {
  std::vector<ldouble> r((size_t)d * d, 0.0L), base = a;
  for (int i = 0; i < d; ++i) r[(size_t)i * d + i] = 1.0L;
  while (e > 0) {
    if (e & 1) matmul(r, base, d, &r);
    e >>= 1;
    if (e) matmul(base, base, d, &base);
  }
  return r;
}

// The scan's tables for one cascade, chunk length and depth: level l's P_l^1 .. P_l^G (P_0 = A^chunk,
// P_(l+1) = P_l^G), row-major D x D each, all high parts, then all low parts.  A stream of calls with one
// Preprocessor asks for the same tables every time, so the last set built on this thread is kept.
const std::vector<double>& scan_tables(const double* sos, int s_count, int chunk, int n_levels) {
  thread_local std::vector<double> key, tables;
  std::vector<double> want(sos, sos + 6 * s_count);
  want.push_back(chunk);
  want.push_back(n_levels);
  if (want == key) return tables;
  const int d = 2 * s_count;
  std::vector<ldouble> a((size_t)d * d);       // the one-sample transition (x = 0)
  for (int q = 0; q < d; ++q) {
    std::vector<ldouble> z(d, 0.0L);
    z[q] = 1.0L;
    step_host(sos, s_count, z.data(), 0.0L);
    for (int r = 0; r < d; ++r) a[(size_t)r * d + q] = z[r];
  }
  std::vector<ldouble> full;
  std::vector<ldouble> p = mat_pow(a, d, chunk);
  for (int l = 0; l < n_levels; ++l) {
    std::vector<ldouble> pj = p;
    for (int j = 0; j < kScanGroup; ++j) {      // P^1 .. P^G
      full.insert(full.end(), pj.begin(), pj.end());
      if (j + 1 < kScanGroup) matmul(pj, p, d, &pj);
    }
    p = pj;
  }
  tables.resize(2 * full.size());
  for (size_t i = 0; i < full.size(); ++i) {
    const double hi = (double)full[i];
    tables[i] = hi;
    tables[full.size() + i] = (double)(full[i] - (ldouble)hi);
  }
  key = std::move(want);
  return tables;
}

// chunk length: enough (chunk, channel) lanes to fill the chip several times over, long chunks otherwise
int sos_chunk(int64_t n_total, int c) {
  int chunk = 256;
  while (chunk > 16 && (n_total / chunk) * (int64_t)c < (int64_t)64 * 1024) chunk >>= 1;
  return chunk;
}

struct ScanLevel {
  long long n_items;     // items scanned at this level
  size_t items_off;      // doubles, in the work buffer (level 0: the chunk items)
  size_t pow_off;        // P_l^1 .. P_l^G
};

template <int S, typename T>
int sos_filter_t(td_handle* h, const T* x, int64_t ldx, int c, const int64_t* offs, int num_files,
                 const double* sos, int split, const double* zi, int reset, double* state,
                 const int64_t* out_rows_dev, const int64_t* out_offs, double* y, int64_t ldy) {
  constexpr int D = 2 * S;
  SosCoef k;
  std::memset(&k, 0, sizeof(k));
  for (int i = 0; i < S; ++i) {
    for (int j = 0; j < 3; ++j) k.c[i][j] = sos[6 * i + j];
    k.c[i][3] = sos[6 * i + 4];
    k.c[i][4] = sos[6 * i + 5];
    k.zi[i][0] = zi[2 * i];
    k.zi[i][1] = zi[2 * i + 1];
  }
  int64_t n_max = 0, n_total = 0;
  for (int f = 0; f < num_files; ++f) {
    const int64_t n = offs[f + 1] - offs[f];
    TD_REQUIRE(h, n >= 1, "td_sos_filter: file %d has no rows (the filter reset reads its first row)", f);
    n_max = std::max(n_max, n);
    n_total += n;
  }
  const int chunk = sos_chunk(n_total, c);
  // the levels of the scan (items are double-double: high parts in [0, work), low parts in [work, 2 work))
  std::vector<ScanLevel> levels;
  const long long n_chunks_max = (n_max + chunk - 1) / chunk;
  size_t work = 0;
  for (long long n = n_chunks_max;; n = (n + kScanGroup - 1) / kScanGroup) {
    levels.push_back({n, work, 0});
    work += (size_t)n * D * c;
    if (n <= kScanGroup) break;
  }
  const std::vector<double>& tables = scan_tables(sos, S, chunk, (int)levels.size());
  const long long tab_lo = (long long)(tables.size() / 2);
  for (size_t l = 0; l < levels.size(); ++l) levels[l].pow_off = l * kScanGroup * D * D;
  const long long lo = (long long)work;
  void* scratch = nullptr;
  TD_TRY(td_scratch(h, (2 * work + tables.size()) * sizeof(double), &scratch));
  double* wbuf = reinterpret_cast<double*>(scratch);
  double* tab = wbuf + 2 * work;
  TD_TRY(td_upload_async(h, tables.data(), tables.size() * sizeof(double), tab));
  for (int f = 0; f < num_files; ++f) {
    const int64_t n = offs[f + 1] - offs[f];
    const T* xf = x + offs[f] * ldx;
    const long long nch = (n + chunk - 1) / chunk;
    double* items = wbuf;
    hipLaunchKernelGGL((sos_init_kernel<S, T>), dim3((unsigned)td_ceil_div(c, kThreads)), dim3(kThreads), 0,
                       h->stream, xf, c, k, split, (f > 0 || reset) ? 1 : 0, state, items, lo);
    if (nch > 1) {
      const long long lanes = (nch - 1) * c;
      hipLaunchKernelGGL((sos_chunk_end_kernel<S, T>), dim3((unsigned)td_ceil_div(lanes, kThreads)),
                         dim3(kThreads), 0, h->stream, xf, (long long)ldx, c, chunk, lanes, k, items, lo);
      // upward: scan every level's blocks, handing the block totals to the next level
      long long n_items = nch;
      int depth = 0;
      std::vector<long long> n_at;
      for (;; ++depth) {
        n_at.push_back(n_items);
        double* it = wbuf + levels[depth].items_off;
        const long long nb = (n_items + kScanGroup - 1) / kScanGroup;
        double* tot = nb > 1 ? wbuf + levels[depth + 1].items_off : nullptr;
        const long long lanes_l = nb * c;
        hipLaunchKernelGGL((sos_scan_local_kernel<S>), dim3((unsigned)td_ceil_div(lanes_l, kThreads)),
                           dim3(kThreads), 0, h->stream, it, lo, n_items, c, lanes_l,
                           tab + levels[depth].pow_off, tab_lo, tot);
        if (nb == 1) break;
        n_items = nb;
      }
      // downward: fold each level's scanned totals into the items below it
      for (int l = depth - 1; l >= 0; --l) {
        const long long lanes_f = (n_at[l] - kScanGroup) * c;
        hipLaunchKernelGGL((sos_scan_fix_kernel<S>), dim3((unsigned)td_ceil_div(lanes_f, kThreads)),
                           dim3(kThreads), 0, h->stream, wbuf + levels[l].items_off, lo, n_at[l], c,
                           lanes_f, tab + levels[l].pow_off, tab_lo, wbuf + levels[l + 1].items_off);
      }
    }
    const long long lanes = nch * c;
    const long long* rows = out_rows_dev ? reinterpret_cast<const long long*>(out_rows_dev) + out_offs[f] : nullptr;
    const long long m = out_rows_dev ? out_offs[f + 1] - out_offs[f] : n;
    double* yf = y + (out_rows_dev ? out_offs[f] : offs[f]) * ldy;
    hipLaunchKernelGGL((sos_chunk_out_kernel<S, T>), dim3((unsigned)td_ceil_div(lanes, kThreads)), dim3(kThreads), 0,
                       h->stream, xf, (long long)ldx, c, (long long)n, chunk, lanes, k, items, lo, rows, m, yf,
                       (long long)ldy, f == num_files - 1 ? state : nullptr);
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

template <typename T>
int sos_filter_dispatch(td_handle* h, const T* x, int64_t ldx, int c, const int64_t* offs, int nf,
                        const double* sos, int s_count, int split, const double* zi, int reset, double* state,
                        const int64_t* rows, const int64_t* out_offs, double* y, int64_t ldy) {
  switch (s_count) {
#define TD_SOS_CASE(S_)                                                                                 \
  case S_:                                                                                              \
    return sos_filter_t<S_, T>(h, x, ldx, c, offs, nf, sos, split, zi, reset, state, rows, out_offs, y, \
                               ldy);
    TD_SOS_CASE(1) TD_SOS_CASE(2) TD_SOS_CASE(3) TD_SOS_CASE(4) TD_SOS_CASE(5) TD_SOS_CASE(6)
    TD_SOS_CASE(7) TD_SOS_CASE(8) TD_SOS_CASE(9) TD_SOS_CASE(10) TD_SOS_CASE(11) TD_SOS_CASE(12)
    TD_SOS_CASE(13) TD_SOS_CASE(14) TD_SOS_CASE(15) TD_SOS_CASE(16)
#undef TD_SOS_CASE
    default:
      return td_fail(h, TD_ERR_INVALID, "td_sos_filter: %d sections (1..%d)", s_count, kMaxSections);
  }
}

// ---- re-reference + channel selection, mean, normalisation + context -----------------------------
template <typename T>
__global__ void __launch_bounds__(kThreads)
group_means_kernel(const T* __restrict__ x, long long ldx, const long long* __restrict__ rows, long long m,
                   int n_groups, const int* __restrict__ ref_ptr, const int* __restrict__ ref_idx,
                   double* __restrict__ means) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= m * n_groups) return;
  const long long r = g / n_groups;
  const int grp = (int)(g - r * n_groups);
  const long long row = rows ? rows[r] : r;
  const T* xr = x + row * ldx;
  double s = 0.0;
  const int b = ref_ptr[grp], e = ref_ptr[grp + 1];
  for (int i = b; i < e; ++i) s += (double)xr[ref_idx[i]];
  means[g] = s / (double)(e - b);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
reref_select_kernel(const T* __restrict__ x, long long ldx, const long long* __restrict__ rows, long long m,
                    int cs, const int* __restrict__ sel, int n_groups, const int* __restrict__ memb_ptr,
                    const int* __restrict__ memb_idx, const double* __restrict__ means, double* __restrict__ z,
                    long long ldz) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= m * cs) return;
  const long long r = g / cs;
  const int j = (int)(g - r * cs);
  const int ch = sel[j];
  const long long row = rows ? rows[r] : r;
  double v = (double)x[row * ldx + ch];
  if (n_groups) {
    const double* mr = means + r * n_groups;
    for (int i = memb_ptr[ch]; i < memb_ptr[ch + 1]; ++i) v -= mr[memb_idx[i]];   // group order
  }
  z[r * ldz + j] = v;
}

__global__ void __launch_bounds__(kThreads)
sum_partials_kernel(const double* __restrict__ z, long long ldz, long long m, int cs, double* __restrict__ part) {
  __shared__ double red[kThreads];
  const long long total = m * cs;
  double s = 0.0;
  for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < total;
       g += (long long)gridDim.x * kThreads) {
    const long long r = g / cs;
    s += z[r * ldz + (g - r * cs)];
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(kThreads)
sum_final_kernel(const double* __restrict__ part, int n, double inv_count, double* __restrict__ out) {
  __shared__ double red[kThreads];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0] * inv_count;
}

// Row t of [context state ; normalised z]
__device__ __forceinline__ double ctx_value(const double* state, long long state_rows, const double* z,
                                            long long ldz, int cs, long long t, int j, double mean,
                                            double std_dev) {
  if (t < state_rows) return state[t * cs + j];
  return (z[(t - state_rows) * ldz + j] - mean) / std_dev;
}

__global__ void __launch_bounds__(kThreads)
context_out_kernel(const double* __restrict__ z, long long ldz, int cs, const double* __restrict__ state,
                   long long state_rows, int width_blocks, long long rows_out, double mean, double std_dev,
                   float* __restrict__ out32, double* __restrict__ out64, long long ldout) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long w = (long long)width_blocks * cs;
  if (g >= rows_out * w) return;
  const long long r = g / w;
  const int q = (int)(g - r * w);
  const int b = q / cs, j = q - b * cs;
  const double v = ctx_value(state, state_rows, z, ldz, cs, r + b, j, mean, std_dev);
  if (out64) out64[r * ldout + q] = v;
  if (out32) out32[r * ldout + q] = (float)v;
}

__global__ void __launch_bounds__(kThreads)
context_state_kernel(const double* __restrict__ z, long long ldz, int cs, const double* __restrict__ state,
                     long long state_rows, long long first, long long keep, double mean, double std_dev,
                     double* __restrict__ state_out) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= keep * cs) return;
  const long long u = g / cs;
  const int j = (int)(g - u * cs);
  state_out[g] = ctx_value(state, state_rows, z, ldz, cs, first + u, j, mean, std_dev);
}

}  // namespace

extern "C" {

int td_sos_filter_plan(int64_t n_total, int64_t n_max, int c, int* chunk, int* levels) {
  if (n_total < 1 || n_max < 1 || n_max > n_total || c < 1 || !chunk || !levels) return TD_ERR_INVALID;
  *chunk = sos_chunk(n_total, c);
  *levels = 1;
  for (long long n = (n_max + *chunk - 1) / *chunk; n > kScanGroup; n = (n + kScanGroup - 1) / kScanGroup)
    ++*levels;
  return TD_OK;
}

int td_sos_filter(td_handle* h, const void* x_dev, int x_is_f64, int64_t ldx, int c,
                  const int64_t* file_offsets_host, int num_files, const double* sos_host, int num_sections,
                  int stage_split, const double* zi_host, int reset, double* state_dev,
                  const int64_t* out_rows_dev, const int64_t* out_offsets_host, double* y_dev, int64_t ldy) {
  if (!h || !x_dev || !file_offsets_host || !sos_host || !zi_host || !state_dev || !y_dev)
    return td_fail(h, TD_ERR_INVALID, "td_sos_filter: NULL argument");
  TD_REQUIRE(h, c >= 1 && num_files >= 1 && ldx >= c && ldy >= c, "td_sos_filter: bad sizes");
  TD_REQUIRE(h, num_sections >= 1 && num_sections <= kMaxSections, "td_sos_filter: %d sections (1..%d)",
             num_sections, kMaxSections);
  TD_REQUIRE(h, stage_split >= 0 && stage_split <= num_sections, "td_sos_filter: bad stage split");
  TD_REQUIRE(h, !out_rows_dev || out_offsets_host, "td_sos_filter: out_rows without out_offsets");
  for (int i = 0; i < num_sections; ++i)
    TD_REQUIRE(h, sos_host[6 * i + 3] == 1.0, "td_sos_filter: section %d is not normalised (a0 != 1)", i);
  if (x_is_f64)
    return sos_filter_dispatch(h, reinterpret_cast<const double*>(x_dev), ldx, c, file_offsets_host, num_files,
                               sos_host, num_sections, stage_split, zi_host, reset, state_dev, out_rows_dev,
                               out_offsets_host, y_dev, ldy);
  return sos_filter_dispatch(h, reinterpret_cast<const float*>(x_dev), ldx, c, file_offsets_host, num_files,
                             sos_host, num_sections, stage_split, zi_host, reset, state_dev, out_rows_dev,
                             out_offsets_host, y_dev, ldy);
}

int td_reref_select(td_handle* h, const void* x_dev, int x_is_f64, int64_t ldx, int c, const int64_t* rows_dev,
                    int64_t m, int num_groups, const int* ref_ptr_host, const int* ref_idx_host,
                    const int* chan_ptr_host, const int* chan_idx_host, const int* sel_host, int cs,
                    double* z_dev, int64_t ldz) {
  if (!h || !x_dev || !z_dev) return td_fail(h, TD_ERR_INVALID, "td_reref_select: NULL argument");
  TD_REQUIRE(h, c >= 1 && cs >= 1 && m >= 0 && ldx >= c && ldz >= cs && num_groups >= 0,
             "td_reref_select: bad sizes");
  TD_REQUIRE(h, num_groups == 0 || (ref_ptr_host && ref_idx_host && chan_ptr_host && chan_idx_host),
             "td_reref_select: groups without their tables");
  std::vector<int> sel(cs);
  for (int j = 0; j < cs; ++j) {
    sel[j] = sel_host ? sel_host[j] : j;
    TD_REQUIRE(h, sel[j] >= 0 && sel[j] < c, "td_reref_select: channel %d of %d", sel[j], c);
  }
  // per input channel, the groups that re-reference it, in group order (a channel listed twice in ONE group
  // is re-referenced once: numpy's fancy-index update)
  std::vector<int> memb_ptr(c + 1, 0), memb_idx;
  std::vector<int> ref_ptr, ref_idx;
  if (num_groups) {
    std::vector<std::vector<int>> per(c);
    for (int g = 0; g < num_groups; ++g) {
      TD_REQUIRE(h, ref_ptr_host[g + 1] > ref_ptr_host[g], "td_reref_select: group %d has no reference channel",
                 g);
      for (int i = ref_ptr_host[g]; i < ref_ptr_host[g + 1]; ++i)
        TD_REQUIRE(h, ref_idx_host[i] >= 0 && ref_idx_host[i] < c, "td_reref_select: reference channel %d of %d",
                   ref_idx_host[i], c);
      for (int i = chan_ptr_host[g]; i < chan_ptr_host[g + 1]; ++i) {
        const int ch = chan_idx_host[i];
        TD_REQUIRE(h, ch >= 0 && ch < c, "td_reref_select: channel %d of %d", ch, c);
        if (per[ch].empty() || per[ch].back() != g) per[ch].push_back(g);
      }
    }
    for (int ch = 0; ch < c; ++ch) {
      memb_ptr[ch + 1] = memb_ptr[ch] + (int)per[ch].size();
      memb_idx.insert(memb_idx.end(), per[ch].begin(), per[ch].end());
    }
    ref_ptr.assign(ref_ptr_host, ref_ptr_host + num_groups + 1);
    ref_idx.assign(ref_idx_host + ref_ptr[0], ref_idx_host + ref_ptr[num_groups]);
    for (int& v : ref_ptr) v -= ref_ptr_host[0];
  }
  if (m == 0) return TD_OK;
  if (memb_idx.empty()) memb_idx.push_back(0);
  if (ref_idx.empty()) { ref_ptr.assign(1, 0); ref_idx.push_back(0); }
  // one table: sel | memb_ptr | memb_idx | ref_ptr | ref_idx
  std::vector<int> tabv;
  tabv.insert(tabv.end(), sel.begin(), sel.end());
  const size_t o_mp = tabv.size();
  tabv.insert(tabv.end(), memb_ptr.begin(), memb_ptr.end());
  const size_t o_mi = tabv.size();
  tabv.insert(tabv.end(), memb_idx.begin(), memb_idx.end());
  const size_t o_rp = tabv.size();
  tabv.insert(tabv.end(), ref_ptr.begin(), ref_ptr.end());
  const size_t o_ri = tabv.size();
  tabv.insert(tabv.end(), ref_idx.begin(), ref_idx.end());
  const void* tab_dev = nullptr;
  TD_TRY(td_table_upload(h, tabv.data(), tabv.size() * sizeof(int), &tab_dev));
  const int* t = reinterpret_cast<const int*>(tab_dev);
  double* means = nullptr;
  const long long* rows = reinterpret_cast<const long long*>(rows_dev);
  if (num_groups) {
    void* scratch = nullptr;
    TD_TRY(td_scratch(h, (size_t)m * num_groups * sizeof(double), &scratch));
    means = reinterpret_cast<double*>(scratch);
    const long long lanes = m * num_groups;
    if (x_is_f64)
      hipLaunchKernelGGL(group_means_kernel<double>, dim3((unsigned)td_ceil_div(lanes, kThreads)), dim3(kThreads), 0,
                         h->stream, reinterpret_cast<const double*>(x_dev), (long long)ldx, rows, (long long)m,
                         num_groups, t + o_rp, t + o_ri, means);
    else
      hipLaunchKernelGGL(group_means_kernel<float>, dim3((unsigned)td_ceil_div(lanes, kThreads)), dim3(kThreads), 0,
                         h->stream, reinterpret_cast<const float*>(x_dev), (long long)ldx, rows, (long long)m,
                         num_groups, t + o_rp, t + o_ri, means);
  }
  const long long lanes = m * cs;
  if (x_is_f64)
    hipLaunchKernelGGL(reref_select_kernel<double>, dim3((unsigned)td_ceil_div(lanes, kThreads)), dim3(kThreads), 0,
                       h->stream, reinterpret_cast<const double*>(x_dev), (long long)ldx, rows, (long long)m, cs, t,
                       num_groups, t + o_mp, t + o_mi, means, z_dev, (long long)ldz);
  else
    hipLaunchKernelGGL(reref_select_kernel<float>, dim3((unsigned)td_ceil_div(lanes, kThreads)), dim3(kThreads), 0,
                       h->stream, reinterpret_cast<const float*>(x_dev), (long long)ldx, rows, (long long)m, cs, t,
                       num_groups, t + o_mp, t + o_mi, means, z_dev, (long long)ldz);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_mean_f64(td_handle* h, const double* z_dev, int64_t m, int cs, int64_t ldz, double* mean_dev) {
  if (!h || !z_dev || !mean_dev) return td_fail(h, TD_ERR_INVALID, "td_mean_f64: NULL argument");
  TD_REQUIRE(h, m >= 1 && cs >= 1 && ldz >= cs, "td_mean_f64: bad sizes");
  const long long total = m * cs;
  const int blocks = (int)std::min<long long>(1024, td_ceil_div(total, kThreads));
  void* scratch = nullptr;
  TD_TRY(td_scratch(h, (size_t)blocks * sizeof(double), &scratch));
  double* part = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(sum_partials_kernel, dim3(blocks), dim3(kThreads), 0, h->stream, z_dev, (long long)ldz,
                     (long long)m, cs, part);
  hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(kThreads), 0, h->stream, part, blocks, 1.0 / (double)total,
                     mean_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_context_out(td_handle* h, const double* z_dev, int64_t m, int cs, int64_t ldz, const double* state_dev,
                   int64_t state_rows, int pre, int post, double mean, double std_dev, float* out32_dev,
                   double* out64_dev, int64_t ldout, double* state_out_dev) {
  if (!h || (!z_dev && m > 0) || (!out32_dev && !out64_dev))
    return td_fail(h, TD_ERR_INVALID, "td_context_out: NULL argument");
  TD_REQUIRE(h, cs >= 1 && m >= 0 && pre >= 0 && post >= 0 && state_rows >= 0 && ldz >= cs,
             "td_context_out: bad sizes");
  TD_REQUIRE(h, state_rows == 0 || state_dev, "td_context_out: state rows without a state");
  const int width_blocks = pre + post + 1;
  TD_REQUIRE(h, ldout >= (int64_t)width_blocks * cs, "td_context_out: output row stride %lld < %lld",
             (long long)ldout, (long long)width_blocks * cs);
  const long long cat = state_rows + m;
  const long long rows_out = cat - pre - post;
  TD_REQUIRE(h, rows_out >= 0, "td_context_out: %lld rows cannot hold %d + %d rows of context", cat, pre, post);
  const long long keep = std::min<long long>(cat, pre + post);
  TD_REQUIRE(h, keep == 0 || state_out_dev, "td_context_out: context without a state to carry");
  TD_REQUIRE(h, state_out_dev != state_dev || keep == 0, "td_context_out: the new state may not alias the old");
  const long long outs = rows_out * width_blocks * cs;
  if (outs > 0)
    hipLaunchKernelGGL(context_out_kernel, dim3((unsigned)td_ceil_div(outs, kThreads)), dim3(kThreads), 0,
                       h->stream, z_dev, (long long)ldz, cs, state_dev, (long long)state_rows, width_blocks, rows_out,
                       mean, std_dev, out32_dev, out64_dev, (long long)ldout);
  if (keep > 0)
    hipLaunchKernelGGL(context_state_kernel, dim3((unsigned)td_ceil_div(keep * cs, kThreads)), dim3(kThreads), 0,
                       h->stream, z_dev, (long long)ldz, cs, state_dev, (long long)state_rows, cat - keep, keep, mean,
                       std_dev, state_out_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

}  // extern "C"
