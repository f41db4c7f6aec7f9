// What the two envelope calibrations share (online_calib.hip: td_calib_online_*, the FIR prediction in front;
// online_dnn_calib.hip: td_fccalib_online_*, a fully connected regressor in front): the state block's head of 29
// float64 sums, the walk that advances them in frame order, and the opening checks of the two push entry points.
// Both kernels are under the family's hardest promise -- any cut of a recording into pushes gives the same state
// bytes, bit for bit those of the NumPy twin -- and this is the one statement of the arithmetic that keeps it.
// online_cca_calib.hip's dims-wide walk is another algorithm (per-window hand-off through LDS) and does not use this.
#pragma once
#include "online_common.h"

// The walk's Gram update is G + z_i z_j UNFUSED: the product rounds, then the add rounds, as np.outer then + do.  A
// function is compiled under the contraction mode in force where it is DEFINED, not where it is called: without this
// line the functions below contract under the default even when the including file switches contraction off after its
// includes (measured: v_mul_f64 9 -> 3, v_add_f64 18 -> 12, v_fma_f64 and v_fmac_f64 0 -> 3 each in
// online_calib_push_kernel), and the twin breaks silently.  The pragma stands at file scope, so
// it runs on into the includer: do not include this header from a file that relies on the default contraction behind
// the include point.  Both includers switch it off themselves, and what they take from online_common.h and
// online_dnn_common.h (included in front of this) fuses by explicit fmaf only.
#pragma clang fp contract(off)

namespace {

// ---- the state block: online_common.h's tails behind a head of kSums doubles
//   [0, 6)    the correlator's sums over every emitted frame: sum p, sum p^2, sum a, sum a^2, sum u, sum u^2
//   [6, 15)   class 0 (truth u) over the windows completed so far: sum_w z [3], then the upper triangle of
//             sum_w z z^T in the order (0,0) (0,1) (0,2) (1,1) (1,2) (2,2), with z = (sum x p, sum x, sum p)
//   [15, 24)  class 1 (truth a), the same
//   [24, 29)  the open window's running sums: sum p, sum a, sum a p, sum u, sum u p
constexpr int kSums = TD_CALIB_ONLINE_SUMS;
constexpr int kOpen = 24;       // the first of the open window's five sums

__host__ __device__ inline long long state_eeg_offset() { return 8LL * kSums; }
__host__ __device__ inline long long state_env_offset(int c, int pre, int post) {
  return tail_end(state_eeg_offset(), c, pre + post);
}
__host__ __device__ inline long long state_bytes(int c, int pre, int post) {
  return tails_bytes(state_eeg_offset(), c, pre + post, 2LL * post);
}

// ---- the walk.  The 29 sums are independent, so lane t of the first wave owns state double t and walks a pass's
// frames from LDS, where a frame's values sit as float64 {1, p, a, u}; a lane of a class sum keeps its own copy of
// the one or two open-window sums it needs (the same additions in the same order: the same bits as the open
// window's lanes).  A per-frame term is the product of two of the quadruple (f0, f1: indices into it) -- two widened
// float32 values, or one and 1.0: exact in float64.
enum : int { kPlain = 0, kOpenSum = 1, kClassSum = 2, kClassGram = 3, kIdle = 4 };

struct WalkLane {
  int role, f0, f1, g0, g1;      // what the lane does; its term's factors; a Gram lane's second term's
  double acc, r1, r2;            // the state double; the lane's copies of the open-window sums
};

// component `comp` of z = (sum x p, sum x, sum p) for the truth at index `truth` (2: a, 3: u): its two factors and the
// open-window sum that holds its running value
__device__ __forceinline__ void z_component(int truth, int comp, int* f0, int* f1, int* open) {
  if (comp == 0) { *f0 = truth; *f1 = 1; *open = kOpen + (truth == 2 ? 2 : 4); }
  else if (comp == 1) { *f0 = truth; *f1 = 0; *open = kOpen + (truth == 2 ? 1 : 3); }
  else { *f0 = 1; *f1 = 0; *open = kOpen; }
}

// Lane tid's part of the walk, from the state's sums as the last push left them (idle from tid = kSums on).
__device__ __forceinline__ WalkLane walk_lane(const double* sums, int tid) {
  WalkLane w = {kIdle, 0, 0, 0, 0, 0.0, 0.0, 0.0};
  if (tid < kSums) {
    w.acc = sums[tid];
    if (tid < 6) {                                           // sum p, p^2, a, a^2, u, u^2
      w.role = kPlain;
      w.f0 = 1 + (tid >> 1);
      w.f1 = (tid & 1) ? w.f0 : 0;
    } else if (tid >= kOpen) {                               // sum p, a, a p, u, u p
      w.role = kOpenSum;
      const int j = tid - kOpen;
      w.f0 = j == 0 ? 1 : (j <= 2 ? 2 : 3);
      w.f1 = (j == 2 || j == 4) ? 1 : 0;
    } else {
      const int cls = (tid - 6) / 9, j = (tid - 6) - 9 * cls;
      const int truth = cls == 1 ? 2 : 3;
      int open = 0;
      if (j < 3) {
        w.role = kClassSum;
        z_component(truth, j, &w.f0, &w.f1, &open);
        w.r1 = sums[open];
      } else {
        w.role = kClassGram;
        const int e = j - 3;                                 // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
        const int zi = e < 3 ? 0 : (e < 5 ? 1 : 2), zj = e < 3 ? e : (e < 5 ? e - 2 : 2);
        z_component(truth, zi, &w.f0, &w.f1, &open);
        w.r1 = sums[open];
        z_component(truth, zj, &w.g0, &w.g1, &open);
        w.r2 = sums[open];
      }
    }
  }
  return w;
}

// The lane's sum advanced by the frames [a, a + nf) of a pass, in frame order, from val_s [pass][4]; pos = a % width,
// the frames of the open window before frame a.  When a frame completes a window the class's sum z takes plain
// adds, its Gram G + z_i z_j unfused, and the open-window sums return to zero.  Call it behind the barrier that
// follows the stores of val_s.
__device__ __forceinline__ void walk_advance(WalkLane& w, const double* val_s, int pos, int nf, int width) {
  // (the loop runs on locals: on the struct's members the compiler copied one add onto two arms of a branch --
  // v_add_f64 18 -> 20 in online_calib_push_kernel, the same work per frame -- and the counts would not be the parent's)
  const int role = w.role, f0 = w.f0, f1 = w.f1, g0 = w.g0, g1 = w.g1;
  double acc = w.acc, r1 = w.r1, r2 = w.r2;
  if (role != kIdle) {
    for (int f = 0; f < nf; ++f) {
      const double* v = val_s + 4 * f;
      const double t1 = v[f0] * v[f1];                       // exact
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
          const double zz = r1 * r2;                         // rounded, then the add rounds: G + z_i z_j unfused
          acc = acc + zz;
          r1 = 0.0;
          r2 = 0.0;
        }
      }
    }
  }
  w.acc = acc; w.r1 = r1; w.r2 = r2;
}

// ---- the opening checks of the two push entry points behind their own shape check: the window, the rows of a push,
// the frames before it, the bank's state against state_bytes.
inline int check_calib_push(td_handle* h, const char* who, int width, long long n, long long frames_before,
                            int num_sessions, const void* state_dev, long long state_ss, int c, int pre, int post) {
  TD_REQUIRE(h, width >= 1 && width <= TD_ONLINE_MAX_WIDTH, "%s: window of %d frames (1 .. %d)", who, width,
             TD_ONLINE_MAX_WIDTH);
  TD_REQUIRE(h, n >= 0 && n <= TD_ONLINE_MAX_PUSH, "%s: %lld rows in one push (0 .. %d)", who, n, TD_ONLINE_MAX_PUSH);
  TD_REQUIRE(h, frames_before >= 0, "%s: %lld frames before", who, frames_before);
  TD_TRY(check_state(h, who, num_sessions, state_dev, state_ss, state_bytes(c, pre, post)));
  return TD_OK;
}

}  // namespace
