// What the two online moment kernels share (online_fit.hip: A = sum v v^T and B = sum v y^T of the ridge fit;
// online_cca_fit.hip: M = sum u u^T of the two views of a CCA fit): the launch's constants, the rounding of one
// accumulator step, the rule for a row of a view, the upper-triangular 64 x 64 tiling of a symmetric matrix as the
// host counts it and as the moments kernels read it, and the checks of a push.  The emitted range of a push, the
// stride checks, the state check and the wave sum are online_common.h's (plan_push, check_push_strides, check_state,
// wave_sum), as for every online push.
//
// Both files include this under a file-level `#pragma clang fp contract(off)`, but nothing here may depend on the
// contraction mode at the include point, the rule online_common.h states for itself: step, the one place where a
// product feeds an add, turns contraction off in its own body, and nowhere else is there a bare a * b + c.  Keep it
// so when adding to this file.
#pragma once
#include "online_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;
constexpr int kPass = 32;                      // frames staged per pass: 2 x 32 x 64 x 8 = 32 KiB of LDS

// acc <- acc g + a b: with g == 1 ONE rounding (a fused multiply-add of the widened float32 values, whose product is
// exact), with g < 1 two, round(round(acc g) + p).  The unfused form is written with plain operators under an
// `fp contract(off)` of its own: the toolchain's __dmul_rn / __dadd_rn are `x * y` / `x + y` in a header compiled
// with the default contraction, so inlined they may be fused again -- into fma(acc, g, a b), ONE rounding (seen on
// the ridge fit's B tiles).
template <bool kForget>
__device__ __forceinline__ double step(double acc, double a, double b, double g) {
#pragma clang fp contract(off)
  if (kForget) {
    const double scaled = acc * g;             // rounded
    const double p = a * b;                    // exact: float32 x float32
    return scaled + p;                         // rounded
  }
  return __fma_rn(a, b, acc);
}

// Row r of a view for a launch that has `before` rows behind it and `after` with its own: the push, the tail (slot j
// = row before - tl + j), zero before the recording and behind a flushed end.  (An emitted frame never reaches below
// the tail: f >= before - post, so r >= before - post - pre_v.)
__device__ __forceinline__ float view_row(const float* src, long long ld, const float* tail, int c, int tl, int ch,
                                          long long r, long long before, long long after) {
  if (r >= after || r < 0) return 0.0f;
  if (r >= before) return src[(r - before) * ld + ch];
  if (r >= before - tl) return tail[(r - (before - tl)) * c + ch];
  return 0.0f;
}

// ---- the tiling.  Only the tiles (ti, tj) with tj >= ti of an n x n symmetric matrix are computed and stored (a
// diagonal tile whole: its two triangles hold the same bits); the lower tiles of the state stay zero.
inline int tiles_of(int n) { return (n + kTile - 1) / kTile; }
inline int upper_tiles(int tiles) { return tiles * (tiles + 1) / 2; }

// The matrix as stored (upper tiles only) read as the symmetric matrix it stands for
__device__ __forceinline__ double sym_at(const double* M, int n, int i, int j) {
  return (i / kTile <= j / kTile) ? M[(long long)i * n + j] : M[(long long)j * n + i];
}

// (A thread's 4 x 4 accumulators of a tile -- their load, the walk of a pass, their store -- the tile decode and, in
// online_fit.hip, the three row rules that view_row restates stay written out in the two kernels: as calls of inlined
// functions each of them moved the kernels' code -- branch layout, 64-bit address arithmetic, an unrolled copy -- and
// the kernels are to stay the code they were.)

// ---- host arithmetic
inline unsigned blocks_for(long long elements) {
  const long long b = td_ceil_div(elements, kThreads * 4);
  return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

// What td_fit_online_push and td_ccafit_online_push refuse in the same words behind their shape checks, in the
// order they stood in: the rows of a push, the forgetting factor, the counters, the state, the pointers, the strides
// (`what`: what the second stream's columns are called).
inline int check_fit_push(td_handle* h, const char* who, int num_sessions, const float* eeg_dev, long long ld_eeg,
                          long long eeg_ss, int c, const float* side_dev, long long ld_side, long long side_ss, int c2,
                          const char* what, long long n, long long frames_before, long long pushes_before,
                          double forget, const void* state_dev, long long stride, long long state_bytes) {
  TD_REQUIRE(h, n >= 0 && n <= TD_ONLINE_MAX_PUSH, "%s: %lld rows in one push (0 .. %d)", who, n, TD_ONLINE_MAX_PUSH);
  TD_REQUIRE(h, forget > 0.0 && forget <= 1.0, "%s: a forgetting factor of %g (0 < g <= 1)", who, forget);
  TD_REQUIRE(h, frames_before >= 0 && pushes_before >= 0, "%s: %lld frames and %lld pushes before", who,
             frames_before, pushes_before);
  TD_TRY(check_state(h, who, num_sessions, state_dev, stride, state_bytes));
  if (n > 0 && (!eeg_dev || !side_dev)) return td_fail(h, TD_ERR_INVALID, "%s: NULL argument", who);
  if (n > 0) TD_TRY(check_push_strides(h, who, num_sessions, ld_eeg, eeg_ss, c, ld_side, side_ss, c2, what));
  return TD_OK;
}

}  // namespace
