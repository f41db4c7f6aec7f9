// What the two kernels that project with a CCA model share (online_cca.hip's td_cca_online_push and
// online_cca_calib.hip's td_ccacalib_online_push): the projection of one lagged row by one wave, and the staging and
// the tail of the two speakers' feature blocks.  Both files get the SAME projection bits from here: online_cca.hip
// includes this under the default contraction mode, online_cca_calib.hip under a file-level `#pragma clang fp
// contract(off)`, so -- online_common.h's rule -- the fused operation is an explicit fmaf and nowhere does a product
// feed an add or a subtract in one expression.
#pragma once
#include "online_common.h"

namespace {

constexpr int kDimBlock = 4;       // columns a wave accumulates at once (4 x 4 accumulators)

// Frames run max(post1, post2) rows behind the input.
__host__ __device__ inline int delay_of(int post1, int post2) { return post1 > post2 ? post1 : post2; }

// Rows of the staging areas: a pass reads nf + pre + post_v rows of a view; the tail shift at the end of a
// push parks up to pre + post rows there.
__host__ __device__ inline int stage_rows(int pass, int pre, int post_v, int post) {
  const int a = pass + pre + post_v, b = pre + post;
  return a > b ? a : b;
}

// One view's projection of one frame by one wave: out[d] = sum_k (xr[k] - mean[k]) rot[d K + k], kDimBlock
// columns at a time (a column past dims - 1 repeats the last one and is dropped).
__device__ __forceinline__ void project_row(const float* xr, const float* mean, const float* rot, int K, int dims,
                                            int lane, float* out) {
  for (int d0 = 0; d0 < dims; d0 += kDimBlock) {
    const float* r[kDimBlock];
#pragma unroll
    for (int i = 0; i < kDimBlock; ++i) r[i] = rot + (size_t)(d0 + i < dims ? d0 + i : dims - 1) * K;
    float acc[kDimBlock][4];
#pragma unroll
    for (int i = 0; i < kDimBlock; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    int k = lane;
    for (; k + 192 < K; k += 256) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xc = xr[k + 64 * j] - mean[k + 64 * j];
#pragma unroll
        for (int i = 0; i < kDimBlock; ++i) acc[i][j] = fmaf(xc, r[i][k + 64 * j], acc[i][j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (k + 64 * j < K) {
        const float xc = xr[k + 64 * j] - mean[k + 64 * j];
#pragma unroll
        for (int i = 0; i < kDimBlock; ++i) acc[i][j] = fmaf(xc, r[i][k + 64 * j], acc[i][j]);
      }
    }
#pragma unroll
    for (int i = 0; i < kDimBlock; ++i) {
      const float total = wave_sum_f32((acc[i][0] + acc[i][1]) + (acc[i][2] + acc[i][3]));
      if (lane == 0 && d0 + i < dims) out[d0 + i] = total;
    }
  }
}

// ---- the model into LDS: the means as they are, the rotations transposed (global [k][dims] -> LDS [dims][k])
template <int NT>
__device__ __forceinline__ void stage_model(float* mean1_s, float* mean2_s, float* rot1_s, float* rot2_s,
                                            const float* mean_x, const float* rot_x, const float* mean_y,
                                            const float* rot_y, int k1, int k2, int dims) {
  const int tid = threadIdx.x;
  for (int k = tid; k < k1; k += NT) mean1_s[k] = mean_x[k];
  for (int k = tid; k < k2; k += NT) mean2_s[k] = mean_y[k];
  for (int i = tid; i < k1 * dims; i += NT) {
    const int k = i / dims, d = i - k * dims;
    rot1_s[d * k1 + k] = rot_x[i];
  }
  for (int i = tid; i < k2 * dims; i += NT) {
    const int k = i / dims, d = i - k * dims;
    rot2_s[d * k2 + k] = rot_y[i];
  }
}

// ---- each speaker's feature rows first .. first + n_rows - 1 into rows2_s [2][r2][c2]: from the tails [2][t2][c2]
// (the rows before this push, which is rows [p0, p1)), from the push, zeros before the recording and behind a
// flushed end
template <int NT>
__device__ __forceinline__ void stage_feat(float* rows2_s, int r2, const float* tail2, int t2,
                                           const float* const* feat, long long feat_ld, int c2, long long first,
                                           int n_rows2, long long p0, long long p1) {
  for (int i = threadIdx.x; i < 2 * n_rows2 * c2; i += NT) {
    const int spk = i / (n_rows2 * c2), rem = i - spk * (n_rows2 * c2);
    const int rr = rem / c2, ch = rem - rr * c2;
    const long long row = first + rr;
    float v = 0.f;
    if (row >= 0 && row < p0) v = tail2[((long long)spk * t2 + (row - (p0 - t2))) * c2 + ch];
    else if (row >= p0 && row < p1) v = feat[spk][(row - p0) * feat_ld + ch];
    rows2_s[((size_t)spk * r2 + rr) * c2 + ch] = v;
  }
}

// ---- the feature tails for the next push: the last t2 rows of (old tail, this push of n rows) of each speaker.  A
// push shorter than the tail shifts it: the rows that stay go through LDS -- feat_tail_park, a barrier,
// feat_tail_store.
template <int NT>
__device__ __forceinline__ void feat_tail_park(float* rows2_s, int r2, const float* tail2, int t2, int c2,
                                               long long n) {
  const int keep2 = n < t2 ? (int)(t2 - n) : 0;
  for (int i = threadIdx.x; i < 2 * keep2 * c2; i += NT) {
    const int spk = i / (keep2 * c2), rem = i - spk * (keep2 * c2);
    rows2_s[(size_t)spk * r2 * c2 + rem] = tail2[((long long)spk * t2 + (t2 - keep2)) * c2 + rem];
  }
}

template <int NT>
__device__ __forceinline__ void feat_tail_store(float* tail2, const float* rows2_s, int r2, int t2, int c2,
                                                const float* const* feat, long long feat_ld, long long n) {
  const int keep2 = n < t2 ? (int)(t2 - n) : 0;
  for (int i = threadIdx.x; i < 2 * t2 * c2; i += NT) {
    const int spk = i / (t2 * c2), rem = i - spk * (t2 * c2);
    const int rr = rem / c2, ch = rem - rr * c2;
    tail2[i] = rr < keep2 ? rows2_s[(size_t)spk * r2 * c2 + rem] : feat[spk][(n - (t2 - rr)) * feat_ld + ch];
  }
}

// ---- the shape checks the two families share (`who` is the entry point's name): everything but the LDS budget,
// which depends on what else a kernel keeps there.
inline int check_cca_views(td_handle* h, const char* who, int c1, int pre1, int post1, int c2, int pre2, int post2,
                           int dims, int width, int max_c1, int max_c2, int max_lags, int max_dims) {
  TD_REQUIRE(h, c1 >= 1 && c1 <= max_c1, "%s: %d EEG channels (1 .. %d)", who, c1, max_c1);
  TD_REQUIRE(h, pre1 >= 0 && post1 >= 0 && pre1 + 1 + post1 <= max_lags,
             "%s: EEG context of %d + 1 + %d frames (at most %d lags)", who, pre1, post1, max_lags);
  TD_REQUIRE(h, c2 >= 1 && c2 <= max_c2, "%s: %d feature channels (1 .. %d)", who, c2, max_c2);
  TD_REQUIRE(h, pre2 >= 0 && post2 >= 0 && pre2 + 1 + post2 <= max_lags,
             "%s: feature context of %d + 1 + %d frames (at most %d lags)", who, pre2, post2, max_lags);
  TD_REQUIRE(h, dims >= 1 && dims <= max_dims, "%s: %d dims (1 .. %d)", who, dims, max_dims);
  TD_REQUIRE(h, width >= 1 && width <= TD_ONLINE_MAX_WIDTH, "%s: window of %d frames (1 .. %d)", who, width,
             TD_ONLINE_MAX_WIDTH);
  return TD_OK;
}

}  // namespace
