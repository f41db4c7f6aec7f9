// What the lag kernels' files share (lagcov.hip, lag_narrow16.hip, lag_targets.hip, lag_util.hip); the host
// interface of all of them is td_common.h.
#pragma once
#include "td_common.h"

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kThreads = 256;
}  // namespace

// Splits segments into slabs of at most `slab` samples (lagcov.hip).
std::vector<LagWork> split_work(const std::vector<LagSeg>& segs, long long slab);
