// What the two online kernels that run a fully connected regressor share (online_dnn.hip: td_fc_online_*;
// online_dnn_calib.hip: td_fccalib_online_*): the network's shape and how W1 is cut, the LDS of a launch and the pass
// that fits it, the shape checks and the LDS query, and the three device functions of layer 1 -- a chunk of W1 from
// global into registers, from registers into LDS, one slice of W1 for one frame's columns.  The layer-1 driver and
// the later layers are no function (DESIGN.md sections 36 and 47: a helper call there changed
// dnn_online_push_kernel's register allocation): they are the text of online_dnn_forward_body.h, which each kernel
// includes inside its pass loop.
//
// The prediction has td_mlp_forward's bits whatever the including file's contraction mode: every fused operation
// here is an explicit fmaf and no product feeds an add in one expression (online_common.h's rule).
#pragma once
#include "online_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxChannels = 128, kMaxLags = 64, kMaxK = 8192;
constexpr int kMaxHidden = 4, kMaxWidth = 64, kMaxKs = 64;
constexpr int kPass = 64;                              // emitted frames per pass; halved until the LDS budget holds
constexpr int kChunkFloats = kMaxKs * kMaxWidth;       // a staged chunk of W1: whole slices, at most this much
constexpr int kLoads = kChunkFloats / 4 / kThreads;    // float4 a thread carries from global to LDS per chunk
constexpr int kPairs = kPass * (kMaxWidth / 4) / kThreads;   // (frame, 4 columns) pairs a thread owns
constexpr long long kLdsBudget = TD_FC_ONLINE_LDS_BYTES;

// The network's shape and how W1 is cut: host arithmetic, passed to the kernel by value.
struct DnnNet {
  int nl;                          // layers (hidden + 1)
  int w[kMaxHidden + 2];           // w[0] = K, w[1 .. nl - 1] hidden, w[nl] = 1
  int off_w[kMaxHidden + 1], off_b[kMaxHidden + 1];   // offsets into the packed parameters
  int n_params, small0, n_small;   // everything behind W1 starts at small0
  int ks, nslices;                 // rows per slice of W1, slices
  int nj;                          // w[1] rounded up to 4: the row stride of a staged chunk
  int g, nchunks;                  // slices per staged chunk, chunks
  int lda;                         // row stride of the staged activations (odd)
};

DnnNet net_of(int c, int pre, int post, const int* hidden, int num_hidden) {
  DnnNet t;
  memset(&t, 0, sizeof(t));
  t.nl = num_hidden + 1;
  t.w[0] = c * (pre + 1 + post);
  int maxw = 1;
  for (int i = 0; i < num_hidden; ++i) {
    t.w[i + 1] = hidden[i];
    maxw = hidden[i] > maxw ? hidden[i] : maxw;
  }
  t.w[t.nl] = 1;
  int at = 0;
  for (int l = 1; l <= t.nl; ++l) {
    t.off_w[l - 1] = at; at += t.w[l - 1] * t.w[l];
    t.off_b[l - 1] = at; at += t.w[l];
  }
  t.n_params = at;
  t.small0 = t.w[0] * t.w[1];
  t.n_small = at - t.small0;
  t.ks = (int)td_round_up(td_ceil_div(t.w[0], 64), 4);
  t.ks = t.ks > kMaxKs ? kMaxKs : t.ks;
  t.nslices = (int)td_ceil_div(t.w[0], t.ks);
  t.nj = (int)td_round_up(t.w[1], 4);
  t.g = kChunkFloats / (t.ks * t.nj);
  t.g = t.g > t.nslices ? t.nslices : t.g;
  t.nchunks = (int)td_ceil_div(t.nslices, t.g);
  t.lda = maxw | 1;
  return t;
}

__host__ __device__ inline int row_stride(int c) { return c | 1; }

// LDS of a launch: 8 (4 pass) for what a pass keeps per frame in float64 (the decoder: both speakers' scores and
// window means; the calibration: {1, p, a, u}), then float32: two chunks of W1, the small parameters (rounded up to
// 4), the staged rows, the envelopes, the predictions, two activation buffers.
long long lds_bytes(const DnnNet& t, int c, int pre, int post, int pass) {
  const long long env_rows = pass > post ? pass : post;
  return 32LL * pass + 4LL * (2LL * t.g * t.ks * t.nj + td_round_up(t.n_small, 4) +
                              (long long)(pass + pre + post) * row_stride(c) + 2 * env_rows + pass +
                              2LL * pass * t.lda);
}

// The largest pass (kPass halved, at least 1, no more than the frames to emit) whose LDS fits; 0: none does.
int pass_of(const DnnNet& t, int c, int pre, int post, long long emitted_now) {
  int pass = emitted_now < kPass ? (emitted_now > 1 ? (int)emitted_now : 1) : kPass;
  while (pass > 1 && lds_bytes(t, c, pre, post, pass) > kLdsBudget) pass = (pass + 1) / 2;
  return lds_bytes(t, c, pre, post, pass) <= kLdsBudget ? pass : 0;
}

// Chunk ci of W1 (rows [ci g ks, ...) as [rows][nj], columns past w1 - 1 repeating it) from global into registers: float4
// number tid + i kThreads of the chunk.  vec: w1 is a multiple of 4 and W1 is 16-byte aligned -- the chunk is one
// contiguous span of W1.
__device__ __forceinline__ void chunk_load(const float* __restrict__ w1p, const DnnNet& t, int ci, bool vec, int tid,
                                           float4 (&regs)[kLoads]) {
  const int k0 = ci * t.g * t.ks, w1 = t.w[1], nj = t.nj;
  const int rows = t.w[0] - k0 < t.g * t.ks ? t.w[0] - k0 : t.g * t.ks;
  const int n4 = rows * nj / 4;
  const float* base = w1p + (long long)k0 * w1;
  // (no branch around a load: an index past the chunk reads the chunk's last element and is dropped by
  // chunk_store -- the loads of a chunk then issue back to back, with no wait between them)
  if (vec) {
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int i4 = tid + i * kThreads;
      regs[i] = reinterpret_cast<const float4*>(base)[i4 < n4 ? i4 : n4 - 1];
    }
  } else {
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int i4 = tid + i * kThreads;
      const int e = (i4 < n4 ? i4 : n4 - 1) * 4, kk = e / nj, j = e - kk * nj;
      const float* src = base + (long long)kk * w1;
      const float v0 = src[j < w1 ? j : w1 - 1], v1 = src[j + 1 < w1 ? j + 1 : w1 - 1];
      const float v2 = src[j + 2 < w1 ? j + 2 : w1 - 1], v3 = src[j + 3 < w1 ? j + 3 : w1 - 1];
      regs[i] = make_float4(v0, v1, v2, v3);       // (a column past w1 - 1 repeats the last one: its sums are dropped)
    }
  }
}

__device__ __forceinline__ void chunk_store(float* buf, const DnnNet& t, int ci, int tid, const float4 (&regs)[kLoads]) {
  const int k0 = ci * t.g * t.ks;
  const int rows = t.w[0] - k0 < t.g * t.ks ? t.w[0] - k0 : t.g * t.ks;
  const int n4 = rows * t.nj / 4;
#pragma unroll
  for (int i = 0; i < kLoads; ++i) {
    const int i4 = tid + i * kThreads;
    if (i4 < n4) reinterpret_cast<float4*>(buf)[i4] = regs[i];
  }
}

// One slice of W1 for one frame and NG adjacent groups of 4 columns: per column a chain of fused multiply-adds from
// 0.f over the slice's ksl rows in order, then added to the accumulators.  xp: the frame's staged x at the slice's
// first row, which is channel ch0 of its lag; the rows of a lag are contiguous, the lags ldr apart.  wrow: the
// thread's first column in the slice's first row of the staged chunk, the rows nj floats apart.
template <int NG>
__device__ __forceinline__ void slice_fma(const float* xp, const float* wrow, int nj, int ksl, int ch0, int c, int ldr,
                                          float (&acc)[kPairs][4]) {
  float s[NG][4];
#pragma unroll
  for (int g = 0; g < NG; ++g) s[g][0] = s[g][1] = s[g][2] = s[g][3] = 0.f;
  int kk = 0, ch = ch0;
  while (kk < ksl) {
    const int run = c - ch < ksl - kk ? c - ch : ksl - kk;       // rows left in this lag, or in the slice
    // UN rows at a time: their reads are issued together, in front of their multiply-adds (one trip to LDS per UN
    // rows, not per row); the rows of each column's chain stay in order
    constexpr int UN = NG == 1 ? 8 : NG == 2 ? 6 : 4;
    int i = 0;
    for (; i + UN <= run; i += UN) {
      float xv[UN];
      float4 wv[UN][NG];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        xv[u] = xp[i + u];
#pragma unroll
        for (int g = 0; g < NG; ++g) wv[u][g] = reinterpret_cast<const float4*>(wrow + (i + u) * nj)[g];
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          s[g][0] = fmaf(xv[u], wv[u][g].x, s[g][0]); s[g][1] = fmaf(xv[u], wv[u][g].y, s[g][1]);
          s[g][2] = fmaf(xv[u], wv[u][g].z, s[g][2]); s[g][3] = fmaf(xv[u], wv[u][g].w, s[g][3]);
        }
      }
    }
    for (; i < run; ++i) {
      const float x1 = xp[i];
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const float4 w1v = reinterpret_cast<const float4*>(wrow + i * nj)[g];
        s[g][0] = fmaf(x1, w1v.x, s[g][0]); s[g][1] = fmaf(x1, w1v.y, s[g][1]);
        s[g][2] = fmaf(x1, w1v.z, s[g][2]); s[g][3] = fmaf(x1, w1v.w, s[g][3]);
      }
    }
    kk += run;
    xp += run + (ldr - c);
    wrow += run * nj;
    ch = 0;
  }
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    acc[g][0] += s[g][0]; acc[g][1] += s[g][1]; acc[g][2] += s[g][2]; acc[g][3] += s[g][3];
  }
}

// The shape checks the entry points of both families share: the intersection of td_online_push's limits and
// td_mlp_forward's, and the LDS of a pass of one frame against the budget.
int check_shape(td_handle* h, const char* who, int c, int pre, int post, int num_hidden, const int* hidden) {
  TD_TRY(check_context(h, who, c, pre, post, kMaxChannels, kMaxLags));
  TD_REQUIRE(h, (long long)c * (pre + 1 + post) <= kMaxK, "%s: %d lagged inputs (at most %d)", who,
             c * (pre + 1 + post), kMaxK);
  TD_REQUIRE(h, num_hidden >= 0 && num_hidden <= kMaxHidden, "%s: %d hidden layers (at most %d)", who, num_hidden,
             kMaxHidden);
  TD_REQUIRE(h, num_hidden == 0 || hidden, "%s: NULL hidden widths", who);
  for (int i = 0; i < num_hidden; ++i)
    TD_REQUIRE(h, hidden[i] >= 1 && hidden[i] <= kMaxWidth, "%s: hidden layer of %d units (1 .. %d)", who, hidden[i],
               kMaxWidth);
  const DnnNet t = net_of(c, pre, post, hidden, num_hidden);
  const long long need = lds_bytes(t, c, pre, post, 1);
  TD_REQUIRE(h, need <= kLdsBudget,
             "%s: two chunks of W1, the small layers' %d parameters and a pass of one frame of %d x %d lags take %lld "
             "bytes of LDS (budget %lld bytes)", who, t.n_small, c, pre + 1 + post, need, kLdsBudget);
  return TD_OK;
}

// The LDS query of both families (td_fc_online_lds_bytes, td_fccalib_online_lds_bytes): the pass and the bytes of a
// launch that emits `emitted` frames.
int lds_query(const char* who, int c, int pre, int post, int num_hidden, const int* hidden, long long emitted,
              int* pass, int64_t* bytes) {
  if (!pass || !bytes) return td_fail(nullptr, TD_ERR_INVALID, "%s: NULL argument", who);
  TD_TRY(check_shape(nullptr, who, c, pre, post, num_hidden, hidden));
  TD_REQUIRE(nullptr, emitted >= 0, "%s: %lld frames", who, emitted);
  const DnnNet t = net_of(c, pre, post, hidden, num_hidden);
  *pass = pass_of(t, c, pre, post, emitted);
  *bytes = lds_bytes(t, c, pre, post, *pass);
  return TD_OK;
}

}  // namespace
