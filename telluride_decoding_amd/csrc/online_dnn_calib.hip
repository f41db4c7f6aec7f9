// Online calibration of a DNN decoder bank (td_fccalib_online_*): online_calib.hip's sums -- what
// infer_decoder.Decoder.train(data0, data1, window_size = W) takes from a labelled stretch: the correlator's
// statistics, the scaled LDA between the window means of the unattended (class 0) and the attended (class 1)
// correlations, d' -- with the bank's fully connected regressor in front of them instead of the FIR prediction.  A bank
// of sessions, one workgroup of 256 threads each, the state on the device, ONE launch per push, the host counts the
// frames, a block of zeros is a fresh session, no atomics, vector stores only.
//
// The state block is td_calib_online_push's byte for byte -- TD_CALIB_ONLINE_SUMS float64 sums in its order, then the
// EEG tail [pre + post][c] and the envelope tail [post][2] in float32, rounded up to 8 -- so td_calib_online_sums and
// td_calib_online_finish, which read the head alone, serve it as they are.
//
// The prediction of an emitted frame is the float32 value td_fc_online_push returns in `pred`, which has
// td_mlp_forward's bits: online_dnn_common.h's layer-1 functions under the driver and the later-layers loop of
// dnn_online_push_kernel, restated below.  Behind the forward the walk is online_calib_push_kernel's: a frame's
// {1, p, a, u} sits in LDS as float64, lane t of the first wave owns state double t and advances it in frame order,
// the Gram takes G + z_i z_j UNFUSED -- hence the file-level fp contract(off), as in online_calib.hip (DESIGN.md
// section 34); the prediction's fused multiply-adds are explicit fmaf calls, which the pragma does not touch.  So
// acc += float64(x) * float64(p) and G + np.outer(z, z) in NumPy are a bit-exact twin, and any cut of a recording
// into pushes gives the same state bytes.
//
// LDS of a launch is online_dnn.hip's, byte for byte (lds_bytes): the 8 (4 pass) bytes that hold the scores and the
// window means there hold {1, p, a, u} here.  Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are in
// DESIGN.md section 45.
#include "online_dnn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSums = TD_CALIB_ONLINE_SUMS;
constexpr int kOpen = 24;       // the first of the open window's five sums

// (online_calib.hip's block: online_common.h's tails behind a head of kSums doubles)
__host__ __device__ inline long long state_eeg_offset() { return 8LL * kSums; }
__host__ __device__ inline long long state_env_offset(int c, int pre, int post) {
  return tail_end(state_eeg_offset(), c, pre + post);
}
__host__ __device__ inline long long state_bytes(int c, int pre, int post) {
  return tails_bytes(state_eeg_offset(), c, pre + post, 2LL * post);
}

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

// What a lane of the walk does with its state double (online_calib.hip's roles).  A frame's values sit in LDS as
// {1, p, a, u}; a term is the product of two of them (f0, f1: indices into that quadruple).
enum : int { kPlain = 0, kOpenSum = 1, kClassSum = 2, kClassGram = 3, kIdle = 4 };

// component `comp` of z = (sum x p, sum x, sum p) for the truth at index `truth` (2: a, 3: u): its two factors and the
// open-window sum that holds its running value
__device__ __forceinline__ void z_component(int truth, int comp, int* f0, int* f1, int* open) {
  if (comp == 0) { *f0 = truth; *f1 = 1; *open = kOpen + (truth == 2 ? 2 : 4); }
  else if (comp == 1) { *f0 = truth; *f1 = 0; *open = kOpen + (truth == 2 ? 1 : 3); }
  else { *f0 = 1; *f1 = 0; *open = kOpen; }
}

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

  // ---- the walk's lanes: lane t owns state double t (online_calib_push_kernel's assignment)
  int role = kIdle, f0 = 0, f1 = 0, g0 = 0, g1 = 0;
  double acc = 0.0, r1 = 0.0, r2 = 0.0;
  if (tid < kSums) {
    acc = sums[tid];
    if (tid < 6) {                                           // sum p, p^2, a, a^2, u, u^2
      role = kPlain;
      f0 = 1 + (tid >> 1);
      f1 = (tid & 1) ? f0 : 0;
    } else if (tid >= kOpen) {                               // sum p, a, a p, u, u p
      role = kOpenSum;
      const int j = tid - kOpen;
      f0 = j == 0 ? 1 : (j <= 2 ? 2 : 3);
      f1 = (j == 2 || j == 4) ? 1 : 0;
    } else {
      const int cls = (tid - 6) / 9, j = (tid - 6) - 9 * cls;
      const int truth = cls == 1 ? 2 : 3;
      int open = 0;
      if (j < 3) {
        role = kClassSum;
        z_component(truth, j, &f0, &f1, &open);
        r1 = sums[open];
      } else {
        role = kClassGram;
        const int e = j - 3;                                 // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
        const int zi = e < 3 ? 0 : (e < 5 ? 1 : 2), zj = e < 3 ? e : (e < 5 ? e - 2 : 2);
        z_component(truth, zi, &f0, &f1, &open);
        r1 = sums[open];
        z_component(truth, zj, &g0, &g1, &open);
        r2 = sums[open];
      }
    }
  }

  for (long long a = p.e0; a < p.e1; a += pass) {
    const int nf = (int)(p.e1 - a < pass ? p.e1 - a : pass);     // frames [a, a + nf) of this pass
    // ---- the forward: dnn_online_push_kernel's layer-1 driver and later-layers loop, line for line, written out
    // here.  They sit inline in that kernel's body because a helper call there changed its register allocation
    // (DESIGN.md section 36), so there is no function to share; tests/test_gpu_online_dnn_calib.py pins this copy's
    // bits to td_fc_online_push's `pred`.  A change to that block is a change to this one.
    float4 regs[kLoads];
    chunk_load(prm, t, 0, vec, tid, regs);
    // ---- stage the EEG rows a - pre .. a + nf - 1 + post and the envelope rows a .. a + nf - 1
    stage_rows<kThreads>(rows_s, ldr, tail, tl, eeg, p.eeg_ld, c, a - pre, nf + tl, p0, p1);
    stage_env<kThreads>(env_s, etail, post, env, p.env_ld, a, nf, p0);
    chunk_store(ws_s, t, 0, tid, regs);
    __syncthreads();
    // ---- layer 1: thread = (frame f, column lane cg), frame-fastest; the thread owns the column groups cg,
    // cg + cl, ... (4 columns each, cl = kThreads / nf lanes), which share the frame's x.  Per slice a chain of
    // fused multiply-adds from 0.f over the slice's rows, added to the accumulators in slice order.
    const int cl = kThreads / nf, ng = (w1q + cl - 1) / cl;         // (nf <= 64, w1q <= 16: ng <= kPairs)
    const int pf = tid % nf, cg = tid / nf;
    const bool busy = cg < cl && cg * ng < w1q;
    // the thread's groups are cg ng .. cg ng + ng - 1; it reads the ng ADJACENT groups from jb on, moved back where
    // they would pass the last group: a group in front of its own repeats a neighbour's sums and is dropped
    const int jb = busy ? (cg * ng < w1q - ng ? cg * ng : w1q - ng) : 0;
    bool own[kPairs];
    float l1[kPairs][4];
#pragma unroll
    for (int o = 0; o < kPairs; ++o) {
      own[o] = busy && o < ng && jb + o >= cg * ng;
      l1[o][0] = l1[o][1] = l1[o][2] = l1[o][3] = 0.f;
    }
    int lag0 = 0, ch0 = 0;                                          // the slice's first row is (lag0, ch0)
    for (int ci = 0; ci < t.nchunks; ++ci) {
      if (ci + 1 < t.nchunks) chunk_load(prm, t, ci + 1, vec, tid, regs);
      const float* buf = ws_s + (ci & 1) * chunk_floats;
      const int sl_end = (ci + 1) * t.g < t.nslices ? (ci + 1) * t.g : t.nslices;
      for (int sl = ci * t.g; sl < sl_end; ++sl) {
        const int kbase = sl * ks;
        const int ksl = k_all - kbase < ks ? k_all - kbase : ks;
        if (busy) {
          const float* xp = rows_s + (pf + lag0) * ldr + ch0;
          const float* wrow = buf + (size_t)(sl - ci * t.g) * ks * nj + 4 * jb;
          if (ng == 1) slice_fma<1>(xp, wrow, nj, ksl, ch0, c, ldr, l1);
          else if (ng == 2) slice_fma<2>(xp, wrow, nj, ksl, ch0, c, ldr, l1);
          else if (ng == 3) slice_fma<3>(xp, wrow, nj, ksl, ch0, c, ldr, l1);
          else slice_fma<4>(xp, wrow, nj, ksl, ch0, c, ldr, l1);
        }
        ch0 += ksl;
        while (ch0 >= c) { ch0 -= c; ++lag0; }
      }
      if (ci + 1 < t.nchunks) chunk_store(ws_s + ((ci + 1) & 1) * chunk_floats, t, ci + 1, tid, regs);
      __syncthreads();
    }
    // z1 = the partials + b1; ReLU when a layer follows, else (no hidden layer: w1 = 1) the prediction itself
#pragma unroll
    for (int o = 0; o < kPairs; ++o) {
      if (!own[o]) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 4 * (jb + o) + q;
        if (j >= w1) continue;
        const float z = l1[o][q] + small[t.off_b[0] + j];
        if (nl > 1) act_s[pf * lda_s + j] = z <= 0.f ? 0.f : z;
        else pred_s[pf] = z;
      }
    }
    __syncthreads();
    // ---- the later layers: (frame, unit) pairs over the workgroup, frame-fastest; the last layer's one unit is
    // the prediction
    for (int l = 2; l <= nl; ++l) {
      const int wi = t.w[l - 1], wo = t.w[l];
      const float* W = small + t.off_w[l - 1];
      const float* b = small + t.off_b[l - 1];
      const float* in = act_s + (size_t)(l & 1) * pass * lda_s;
      float* outp = act_s + (size_t)((l + 1) & 1) * pass * lda_s;
      for (int pr = tid; pr < nf * wo; pr += kThreads) {
        const int o = pr / nf, f = pr - o * nf;
        const float* xin = in + f * lda_s;
        float sum = 0.f;
        for (int i = 0; i < wi; ++i) sum = fmaf(xin[i], W[i * wo + o], sum);
        sum += b[o];
        if (l < nl) outp[f * lda_s + o] = sum <= 0.f ? 0.f : sum;
        else pred_s[f] = sum;
      }
      __syncthreads();
    }
    // ---- a frame's {1, p, a, u}, widened
    for (int f = tid; f < nf; f += kThreads) {
      val_s[4 * f] = 1.0;
      val_s[4 * f + 1] = (double)pred_s[f];
      val_s[4 * f + 2] = (double)env_s[2 * f];
      val_s[4 * f + 3] = (double)env_s[2 * f + 1];
    }
    __syncthreads();
    // ---- the walk (online_calib_push_kernel's): every sum advances by this pass's frames in frame order
    if (role != kIdle) {
      int pos = (int)(a % width);                            // frames of the open window before frame a
      for (int f = 0; f < nf; ++f) {
        const double* v = val_s + 4 * f;
        const double t1 = v[f0] * v[f1];                     // exact
        const bool done = ++pos == width;
        if (done) pos = 0;
        if (role == kPlain) {
          acc = acc + t1;
        } else if (role == kOpenSum) {
          acc = acc + t1;
          if (done) acc = 0.0;
        } else if (role == kClassSum) {
          r1 = r1 + t1;
          if (done) { acc = acc + r1; r1 = 0.0; }
        } else {
          const double t2 = v[g0] * v[g1];
          r1 = r1 + t1;
          r2 = r2 + t2;
          if (done) {
            const double zz = r1 * r2;                       // rounded, then the add rounds: G + z_i z_j unfused
            acc = acc + zz;
            r1 = 0.0;
            r2 = 0.0;
          }
        }
      }
    }
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
  if (role != kIdle && p.e1 > p.e0) sums[tid] = acc;
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
  if (!pass || !bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_fccalib_online_lds_bytes: NULL argument");
  TD_TRY(check_shape(nullptr, "td_fccalib_online_lds_bytes", c, pre, post, num_hidden, hidden_host));
  TD_REQUIRE(nullptr, emitted >= 0, "td_fccalib_online_lds_bytes: %lld frames", (long long)emitted);
  const DnnNet t = net_of(c, pre, post, hidden_host, num_hidden);
  *pass = pass_of(t, c, pre, post, emitted);
  *bytes = lds_bytes(t, c, pre, post, *pass);
  return TD_OK;
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
  TD_REQUIRE(h, width >= 1 && width <= TD_ONLINE_MAX_WIDTH, "%s: window of %d frames (1 .. %d)", who, width,
             TD_ONLINE_MAX_WIDTH);
  TD_REQUIRE(h, n >= 0 && n <= TD_ONLINE_MAX_PUSH, "%s: %lld rows in one push (0 .. %d)", who, (long long)n,
             TD_ONLINE_MAX_PUSH);
  TD_REQUIRE(h, frames_before >= 0, "%s: %lld frames before", who, (long long)frames_before);
  TD_TRY(check_state(h, who, num_sessions, state_dev, state_session_stride, state_bytes(c, pre, post)));
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
  if (!h->lds_opt_online_dnn_calib) {
    TD_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&dnn_calib_push_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
    h->lds_opt_online_dnn_calib = true;
  }
  TD_TRY(td_profile_mark(h, true, (double)n * num_sessions));
  hipLaunchKernelGGL(dnn_calib_push_kernel, dim3((unsigned)num_sessions), dim3(kThreads),
                     (size_t)lds_bytes(t, c, pre, post, p.pass), h->stream, p);
  TD_HIP(h, hipGetLastError());
  TD_TRY(td_profile_mark(h, false, 0.0));
  return TD_OK;
}

}  // extern "C"
