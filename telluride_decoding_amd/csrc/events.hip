// Events of a trigger channel that is resident on the device (BrainTrial.find_status_trigger_times): an ordered
// compaction of the code changes, so that only the events come back to the host.
//
//   code[i] = (int)v[i * stride] & mask      truncation toward zero; the inputs are finite, |v| < 2^31
//   event at i: code[i] != code[i - 1] and code[i] != 0, with code[-1] = 0
//   at[k], code[k]: the k-th event in increasing order of i
//
// Three launches, none of whose workgroups waits for another, and no atomic anywhere:
//   td_code_onsets_count   onsets_count_kernel: workgroup g counts the events of chunk g (kChunk samples) into
//                          offsets[g]; onsets_scan_kernel: ONE workgroup turns the counts into their exclusive
//                          prefix sums in place, 256 at a time with a running carry, and leaves the total in
//                          offsets[groups].  The host reads those 8 bytes and allocates exactly.
//   td_code_onsets_fill    onsets_fill_kernel: workgroup g finds its events again and writes event offsets[g] + rank;
//                          the rank within the chunk comes from ballots: a thread takes samples tid, tid + 256, ...
//                          of the chunk, so pass j of wave w holds 64 consecutive samples, its events are ranked by
//                          the popcount of the ballot below the lane, and the (pass, wave) counts are summed in
//                          order through LDS.
// The sample before a chunk's first one belongs to the neighbouring workgroup: like every predecessor it is read
// from global memory (a second load per sample, of a neighbouring address that is in the cache; the signal itself,
// 8 bytes a sample, is read once by the count and once by the fill).  The input needs 8-byte alignment only, and a
// stride in elements: a column of a [frames, w] matrix that fix_offset has sliced is read where it lies.
//
// The sample index is 64-bit; a sample's place in its chunk and an event's rank in it (<= kChunk) are 32-bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "td_common.h"
#include "td_hotpath.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPasses = 8;
constexpr int kChunk = kThreads * kPasses;   // samples per workgroup

struct OnsetParams {
  const double* v;
  long long n, stride;
  int mask;
};

__device__ __forceinline__ int onset_code(const OnsetParams& p, long long i) {
  return (int)p.v[i * p.stride] & p.mask;
}

// The code of sample i where it is an event, else 0 (an event's code is never 0).
__device__ __forceinline__ int onset_at(const OnsetParams& p, long long i) {
  const int code = onset_code(p, i);
  const int prev = i > 0 ? onset_code(p, i - 1) : 0;
  return code != prev ? code : 0;
}

__global__ __launch_bounds__(kThreads) void onsets_count_kernel(OnsetParams p, long long* offsets) {
  __shared__ int wave_count[kWaves];
  const int tid = threadIdx.x;
  const long long base = (long long)blockIdx.x * kChunk;
  int count = 0;                                                 // (the same in every lane of a wave)
  for (int j = 0; j < kPasses; ++j) {
    const long long i = base + j * kThreads + tid;
    const bool event = i < p.n && onset_at(p, i) != 0;
    count += __popcll(__ballot(event));
  }
  if ((tid & 63) == 0) wave_count[tid >> 6] = count;
  __syncthreads();
  if (tid == 0) {
    int sum = 0;
    for (int w = 0; w < kWaves; ++w) sum += wave_count[w];
    offsets[blockIdx.x] = sum;
  }
}

// offsets[0 .. groups) counts -> exclusive prefix sums, offsets[groups] = the total.  One workgroup.
__global__ __launch_bounds__(kThreads) void onsets_scan_kernel(long long* offsets, long long groups) {
  __shared__ long long wave_sum[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long carry = 0;
  for (long long t0 = 0; t0 < groups; t0 += kThreads) {
    const long long t = t0 + tid;
    const long long own = t < groups ? offsets[t] : 0;
    long long incl = own;                                        // inclusive scan within the wave
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    long long before = carry, all = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) before += wave_sum[w];
      all += wave_sum[w];
    }
    if (t < groups) offsets[t] = before + incl - own;
    carry += all;
    __syncthreads();                                             // wave_sum is written again in the next round
  }
  if (tid == 0) offsets[groups] = carry;
}

__global__ __launch_bounds__(kThreads) void onsets_fill_kernel(OnsetParams p, const long long* offsets,
                                                               long long capacity, long long* at, int* codes) {
  __shared__ int part[kPasses][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long base = (long long)blockIdx.x * kChunk;
  int code[kPasses], rank[kPasses];
#pragma unroll
  for (int j = 0; j < kPasses; ++j) {
    const long long i = base + j * kThreads + tid;
    code[j] = i < p.n ? onset_at(p, i) : 0;
    const unsigned long long votes = __ballot(code[j] != 0);
    rank[j] = __popcll(votes & ((1ull << lane) - 1ull));
    if (lane == 0) part[j][wave] = __popcll(votes);
  }
  __syncthreads();
  const long long first = offsets[blockIdx.x];
  int before = 0;                                                // events of the chunk in the (pass, wave)s before this one
#pragma unroll
  for (int j = 0; j < kPasses; ++j) {
    for (int w = 0; w < kWaves; ++w) {
      if (w == wave && code[j] != 0) {
        const long long k = first + before + rank[j];
        if (k < capacity) {
          at[k] = base + j * kThreads + tid;
          codes[k] = code[j];
        }
      }
      before += part[j][w];
    }
  }
}

int onsets_check(td_handle* h, const char* who, const double* v, int64_t n, int64_t stride, int mask) {
  TD_REQUIRE(h, n >= 0 && (n == 0 || v), "%s: NULL signal or a negative length", who);
  TD_REQUIRE(h, stride >= 1 || n <= 1, "%s: a stride of %lld elements", who, (long long)stride);
  TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(v) & 7) == 0, "%s: the signal must be 8-byte aligned", who);
  TD_REQUIRE(h, mask > 0 && mask <= 0xffffff, "%s: a mask of 0x%x is outside 1 .. 0xffffff", who, (unsigned)mask);
  TD_REQUIRE(h, td_ceil_div(n, kChunk) <= 0x7fffffffll, "%s: too many samples for one launch", who);
  return TD_OK;
}

}  // namespace

extern "C" {

int td_code_onsets_plan(int64_t n, int* chunk, int64_t* groups) {
  if (n < 0 || !chunk || !groups) return TD_ERR_INVALID;
  *chunk = kChunk;
  *groups = td_ceil_div(n, kChunk);
  return TD_OK;
}

int td_code_onsets_count(td_handle* h, const double* signal_dev, int64_t n, int64_t stride, int mask,
                         int64_t* offsets_dev) {
  if (!h || !offsets_dev) return td_fail(h, TD_ERR_INVALID, "td_code_onsets_count: NULL argument");
  TD_TRY(onsets_check(h, "td_code_onsets_count", signal_dev, n, stride, mask));
  TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(offsets_dev) & 7) == 0, "td_code_onsets_count: misaligned offsets");
  const long long groups = td_ceil_div(n, kChunk);
  OnsetParams p{signal_dev, n, stride, mask};
  long long* offsets = reinterpret_cast<long long*>(offsets_dev);
  if (groups > 0)
    hipLaunchKernelGGL(onsets_count_kernel, dim3((unsigned)groups), dim3(kThreads), 0, h->stream, p, offsets);
  hipLaunchKernelGGL(onsets_scan_kernel, dim3(1), dim3(kThreads), 0, h->stream, offsets, groups);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_code_onsets_fill(td_handle* h, const double* signal_dev, int64_t n, int64_t stride, int mask,
                        const int64_t* offsets_dev, int64_t capacity, int64_t* at_dev, int32_t* code_dev) {
  if (!h || !offsets_dev) return td_fail(h, TD_ERR_INVALID, "td_code_onsets_fill: NULL argument");
  TD_TRY(onsets_check(h, "td_code_onsets_fill", signal_dev, n, stride, mask));
  TD_REQUIRE(h, capacity >= 0 && (capacity == 0 || (at_dev && code_dev)),
             "td_code_onsets_fill: NULL outputs or a negative capacity");
  TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(at_dev) & 7) == 0 && (reinterpret_cast<uintptr_t>(code_dev) & 3) == 0 &&
             (reinterpret_cast<uintptr_t>(offsets_dev) & 7) == 0, "td_code_onsets_fill: misaligned outputs or offsets");
  const long long groups = td_ceil_div(n, kChunk);
  if (groups == 0 || capacity == 0) return TD_OK;
  OnsetParams p{signal_dev, n, stride, mask};
  hipLaunchKernelGGL(onsets_fill_kernel, dim3((unsigned)groups), dim3(kThreads), 0, h->stream, p,
                     reinterpret_cast<const long long*>(offsets_dev), (long long)capacity,
                     reinterpret_cast<long long*>(at_dev), code_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

}  // extern "C"
