// Small passes beside the lag kernels: channel maxima (the float16 kernels' scales), float64 column sums,
// the bf16 matrix-pipe probe (split from lagcov.hip; td_common.h declares the entry points).
#include <cstdlib>
#include <cstring>

#include "lag_common.h"

namespace {

typedef td_u32x4 u32x4;

// Largest magnitude of every channel over the rows [row0, row1) of a time x channel array, as
// float bits (non-negative floats order like unsigned integers; a NaN is "larger" than
// everything) atomically maxed into tab[channel]: the scales of the float16 kernel above.
// Order-independent, so the result is reproducible.  tab holds zeros before the call.
__global__ __launch_bounds__(256) void chan_max_kernel(const float* __restrict__ x, long long ld,
                                                       int c, long long row0, long long row1,
                                                       unsigned* __restrict__ tab, int vec4) {
  __shared__ unsigned red[16][64];
  const int tid = threadIdx.x, c4 = (tid & 15) * 4, rl = tid >> 4;
  unsigned m[4] = {0u, 0u, 0u, 0u};
  const long long stride = (long long)gridDim.x * 16;
  if (vec4) {
    if (c4 < c) {
      // four rows in flight per thread
      long long r = row0 + (long long)blockIdx.x * 16 + rl;
      for (; r + 3 * stride < row1; r += 4 * stride) {
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const float4*>(x + (r + k * stride) * ld + c4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          m[0] = max(m[0], __float_as_uint(v[k].x) & 0x7fffffffu);
          m[1] = max(m[1], __float_as_uint(v[k].y) & 0x7fffffffu);
          m[2] = max(m[2], __float_as_uint(v[k].z) & 0x7fffffffu);
          m[3] = max(m[3], __float_as_uint(v[k].w) & 0x7fffffffu);
        }
      }
      for (; r < row1; r += stride) {
        const float4 v = *reinterpret_cast<const float4*>(x + r * ld + c4);
        m[0] = max(m[0], __float_as_uint(v.x) & 0x7fffffffu);
        m[1] = max(m[1], __float_as_uint(v.y) & 0x7fffffffu);
        m[2] = max(m[2], __float_as_uint(v.z) & 0x7fffffffu);
        m[3] = max(m[3], __float_as_uint(v.w) & 0x7fffffffu);
      }
    }
  } else {
    for (long long r = row0 + (long long)blockIdx.x * 16 + rl; r < row1; r += stride)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (c4 + q < c) m[q] = max(m[q], __float_as_uint(x[r * ld + c4 + q]) & 0x7fffffffu);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[rl][c4 + q] = m[q];
  __syncthreads();
  if (tid < 64) {
    unsigned t = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) t = max(t, red[k][tid]);
    if (tid < c && t) atomicMax(tab + (blockIdx.x % kChanShards) * 128 + tid, t);
  }
}

// The same for up to 128 channels in one pass (the virtual-image kernel's 65..128-channel inputs): 32
// threads per row, 8 rows per step, four steps in flight.
__global__ __launch_bounds__(256) void chan_max_wide_kernel(const float* __restrict__ x, long long ld, int c,
                                                            long long row0, long long row1,
                                                            unsigned* __restrict__ tab, int vec4) {
  __shared__ unsigned red[8][128];
  const int tid = threadIdx.x, c4 = (tid & 31) * 4, rl = tid >> 5;
  unsigned m[4] = {0u, 0u, 0u, 0u};
  const long long stride = (long long)gridDim.x * 8;
  long long r = row0 + (long long)blockIdx.x * 8 + rl;
  if (vec4) {
    if (c4 < c) {
      for (; r + 3 * stride < row1; r += 4 * stride) {
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const float4*>(x + (r + k * stride) * ld + c4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          m[0] = max(m[0], __float_as_uint(v[k].x) & 0x7fffffffu);
          m[1] = max(m[1], __float_as_uint(v[k].y) & 0x7fffffffu);
          m[2] = max(m[2], __float_as_uint(v[k].z) & 0x7fffffffu);
          m[3] = max(m[3], __float_as_uint(v[k].w) & 0x7fffffffu);
        }
      }
      for (; r < row1; r += stride) {
        const float4 v = *reinterpret_cast<const float4*>(x + r * ld + c4);
        m[0] = max(m[0], __float_as_uint(v.x) & 0x7fffffffu);
        m[1] = max(m[1], __float_as_uint(v.y) & 0x7fffffffu);
        m[2] = max(m[2], __float_as_uint(v.z) & 0x7fffffffu);
        m[3] = max(m[3], __float_as_uint(v.w) & 0x7fffffffu);
      }
    }
  } else {
    // unaligned rows: a thread is ONE channel (whole rows per load instruction), two rows per step of
    // the workgroup, four steps in flight
    const int ch = tid & 127, rh = tid >> 7;
    unsigned mm = 0u;
    const long long st2 = (long long)gridDim.x * 2;
    long long rr = row0 + (long long)blockIdx.x * 2 + rh;
    if (ch < c) {
      for (; rr + 3 * st2 < row1; rr += 4 * st2) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = x[(rr + k * st2) * ld + ch];
#pragma unroll
        for (int k = 0; k < 4; ++k) mm = max(mm, __float_as_uint(v[k]) & 0x7fffffffu);
      }
      for (; rr < row1; rr += st2) mm = max(mm, __float_as_uint(x[rr * ld + ch]) & 0x7fffffffu);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) red[k][ch] = 0u;       // (both row halves write: combine below)
    __syncthreads();
    atomicMax(&red[0][ch], mm);
    __syncthreads();
    if (tid < 128 && tid < c && red[0][tid]) atomicMax(tab + (blockIdx.x % kChanShards) * 128 + tid, red[0][tid]);
    return;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[rl][c4 + q] = m[q];
  __syncthreads();
  if (tid < 128) {
    unsigned t = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) t = max(t, red[k][tid]);
    if (tid < c && t) atomicMax(tab + (blockIdx.x % kChanShards) * 128 + tid, t);
  }
}

// ---- measurement aid: what the bf16 matrix pipe sustains (td_probe_bf16_mfma) ----------------
// A bare loop of the MFMA lagcov_split_kernel issues, in its six-product order, operands in
// registers, no memory and no LDS: the rate the chip holds under that load for ~1 ms.  With
// all-zero operands it runs at ~0.9 of the nominal peak, with operands shaped like the three
// pieces of a float32 split at 0.66-0.70: the power / clock ceiling the accumulate is measured
// against (bench.py reports both next to its roofline).
__global__ __launch_bounds__(256) void bf16_mfma_probe_kernel(const unsigned* __restrict__ ops,
                                                              float* __restrict__ out, int iters) {
  u32x4 a[3], b[3];
#pragma unroll
  for (int pc = 0; pc < 3; ++pc) {
    a[pc] = *reinterpret_cast<const u32x4*>(ops + (pc * 256 + threadIdx.x) * 4);
    b[pc] = *reinterpret_cast<const u32x4*>(ops + ((3 + pc) * 256 + threadIdx.x) * 4);
  }
  f32x16 acc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
  constexpr int pa[6] = {2, 0, 1, 1, 0, 0}, pb[6] = {0, 2, 1, 0, 1, 0};
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = td_mfma_bf16(a[pa[t]], b[pb[t]], acc[k]);
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += acc[k][r];
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

// ---- float64 column sums (sum of y over the rows that enter the fit) --------
__global__ __launch_bounds__(kThreads) void colsum_kernel(const float* __restrict__ a, long long lda, int ca,
                                                          const LagWork* __restrict__ works, int n_work,
                                                          double* __restrict__ partial) {
  // block b handles work item b.  Thread = (column cl of a tile of cp <= 64 columns, row phase rp):
  // cp = the column count rounded up to a power of two, so that narrow inputs spread their rows
  // over the lanes (one column: 256 row phases) and wide ones read whole rows: coalesced either
  // way.  (The first version took one column per pass -- every pass read every row's cache line
  // for 4 bytes: 1.1 ms for the 64 targets of a forward model.)
  __shared__ double red[kThreads];
  const LagWork w = works[blockIdx.x];
  const int tid = threadIdx.x;
  int cp = 1;
  while (cp < ca && cp < 64) cp <<= 1;
  const int cl = tid & (cp - 1), rp = tid / cp, n_rp = kThreads / cp;
  for (int c0 = 0; c0 < ca; c0 += cp) {
    const int c = c0 + cl;
    double s0 = 0.0, s1 = 0.0;
    if (c < ca) {
      long long u = w.u_begin + rp;
      for (; u + n_rp < w.u_end; u += 2 * n_rp) {
        const bool ok0 = u >= 0 && u < w.a_valid, ok1 = u + n_rp >= 0 && u + n_rp < w.a_valid;
        const float v0 = ok0 ? a[(w.a_row0 + u) * lda + c] : 0.f;
        const float v1 = ok1 ? a[(w.a_row0 + u + n_rp) * lda + c] : 0.f;
        s0 += (double)v0; s1 += (double)v1;
      }
      for (; u < w.u_end; u += n_rp)
        if (u >= 0 && u < w.a_valid) s0 += (double)a[(w.a_row0 + u) * lda + c];
    }
    red[tid] = s0 + s1;
    __syncthreads();
    // fixed order: halve the row phases until one is left
    for (int off = n_rp / 2; off > 0; off >>= 1) {
      if (rp < off) red[tid] += red[tid + off * cp];
      __syncthreads();
    }
    if (rp == 0 && c < ca) partial[(size_t)blockIdx.x * ca + c] = red[tid];
    __syncthreads();
  }
}

// out[c] (+)= sum over the work items; 16 phases x 64 columns per workgroup, fixed order
__global__ __launch_bounds__(1024) void colsum_reduce_kernel(const double* __restrict__ partial, int n_work,
                                                             int ca, double* __restrict__ out, int accumulate) {
  __shared__ double part[16][64];
  const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double s0 = 0.0, s1 = 0.0;
  if (c < ca) {
    int w = q;
    for (; w + 16 < n_work; w += 32) {
      s0 += partial[(size_t)w * ca + c];
      s1 += partial[(size_t)(w + 16) * ca + c];
    }
    if (w < n_work) s0 += partial[(size_t)w * ca + c];
  }
  part[q][cl] = s0 + s1;
  __syncthreads();
  if (q == 0 && c < ca) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += part[k][cl];
    out[c] = accumulate ? out[c] + t : t;
  }
}

}  // namespace

int td_chan_max(td_handle* h, const float* x, int64_t ldx, int c, long long row0, long long row1, unsigned* tab) {
  TD_REQUIRE(h, c >= 1 && c <= 128, "td_chan_max: 1 .. 128 channels");
  const bool al = (ldx % 4 == 0) && (c % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
  if (c <= 64) {
    const long long blocks = td_ceil_div(row1 - row0, 16 * 8);       // >= 8 rows per thread
    hipLaunchKernelGGL(chan_max_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks)),
                       dim3(256), 0, h->stream, x, (long long)ldx, c, row0, row1, tab, al ? 1 : 0);
  } else {
    const long long blocks = td_ceil_div(row1 - row0, (al ? 8 : 2) * 8);
    hipLaunchKernelGGL(chan_max_wide_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks)),
                       dim3(256), 0, h->stream, x, (long long)ldx, c, row0, row1, tab, al ? 1 : 0);
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

// ... over the rows of the array that hold the recordings of a work list (a superset of what its kernel reads)
int td_chan_max_works(td_handle* h, const float* x, int64_t ldx, int c, const std::vector<LagWork>& works,
                      unsigned* tab) {
  long long lo = works[0].a_row0, hi = lo;
  for (const LagWork& wk : works) {
    lo = wk.a_row0 < lo ? wk.a_row0 : lo;
    hi = wk.a_row0 + wk.a_valid > hi ? wk.a_row0 + wk.a_valid : hi;
  }
  return td_chan_max(h, x, ldx, c, lo, hi, tab);
}

int td_colsum(td_handle* h, const float* a, int64_t lda, int ca, const std::vector<LagSeg>& segs,
              double* out_dev, bool accumulate) {
  if (ca <= 0) return TD_OK;
  std::vector<LagWork> works = split_work(segs, 1 << 10);
  if (works.empty()) {
    if (!accumulate) TD_HIP(h, hipMemsetAsync(out_dev, 0, sizeof(double) * ca, h->stream));
    return TD_OK;
  }
  const size_t table_bytes = td_round_up(works.size() * sizeof(LagWork), 256);
  void* scratch = nullptr;
  TD_TRY(td_scratch(h, table_bytes + works.size() * ca * sizeof(double), &scratch));
  TD_TRY(td_upload_async(h, works.data(), works.size() * sizeof(LagWork), scratch));
  double* partial = reinterpret_cast<double*>(reinterpret_cast<char*>(scratch) + table_bytes);
  hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)works.size()), dim3(kThreads), 0, h->stream,
                     a, (long long)lda, ca, reinterpret_cast<const LagWork*>(scratch),
                     (int)works.size(), partial);
  hipLaunchKernelGGL(colsum_reduce_kernel, dim3((unsigned)td_ceil_div(ca, 64)), dim3(1024), 0,
                     h->stream, partial, (int)works.size(), ca, out_dev, accumulate ? 1 : 0);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

// Sustained rate of the bf16 matrix pipe (see bf16_mfma_probe_kernel): split_shaped = 0 runs
// all-zero operands, 1 random operands with the magnitudes of float32 split pieces.  Blocking.
extern "C" int td_probe_bf16_mfma(td_handle* h, int split_shaped, double* tflops) {
  if (!h || !tflops) return td_fail(h, TD_ERR_INVALID, "td_probe_bf16_mfma: NULL argument");
  const int cus = h->cu_count > 0 ? h->cu_count : 256;
  const int grid = 2 * cus, iters = 800;            // two waves per SIMD, ~1 ms
  std::vector<unsigned> host(6 * 256 * 4, 0u);
  if (split_shaped) {
    unsigned state = 12345u;
    auto rnd = [&]() {                              // sum of 12 uniforms - 6: ~N(0, 1)
      float u = 0.f;
      for (int k = 0; k < 12; ++k) { state = state * 1664525u + 1013904223u; u += (state >> 8) * (1.f / 16777216.f); }
      return u - 6.f;
    };
    auto bf = [](float x) { unsigned u; memcpy(&u, &x, 4); return (u + 0x8000u) >> 16; };
    for (int pc = 0; pc < 6; ++pc) {
      const float scale = pc % 3 == 0 ? 1.f : pc % 3 == 1 ? 1.f / 512 : 1.f / 262144;
      for (int i = 0; i < 256 * 4; ++i) host[pc * 1024 + i] = bf(rnd() * scale) | (bf(rnd() * scale) << 16);
    }
  }
  void* scratch = nullptr;
  TD_TRY(td_scratch(h, sizeof(unsigned) * host.size() + sizeof(float) * 256 * (size_t)grid, &scratch));
  unsigned* ops = reinterpret_cast<unsigned*>(scratch);
  float* out = reinterpret_cast<float*>(ops + host.size());
  TD_HIP(h, hipMemcpyAsync(ops, host.data(), sizeof(unsigned) * host.size(), hipMemcpyHostToDevice, h->stream));
  TD_HIP(h, hipStreamSynchronize(h->stream));
  float ms = 0.f;
  for (int rep = 0; rep < 3; ++rep) {
    TD_HIP(h, hipEventRecord(h->ev_start, h->stream));
    hipLaunchKernelGGL(bf16_mfma_probe_kernel, dim3((unsigned)grid), dim3(256), 0, h->stream, ops, out, iters);
    TD_HIP(h, hipEventRecord(h->ev_stop, h->stream));
    TD_HIP(h, hipEventSynchronize(h->ev_stop));
    TD_HIP(h, hipEventElapsedTime(&ms, h->ev_start, h->ev_stop));
  }
  const double mfma = (double)iters * 24 * grid * 4;
  *tflops = mfma * 32768.0 / (ms * 1e-3) / 1e12;
  return TD_OK;
}
