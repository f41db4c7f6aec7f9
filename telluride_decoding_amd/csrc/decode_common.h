// What the decode side's two files share (decode.hip, windows.hip); the host interface of both is td_common.h.
#pragma once
#include <cstdlib>

#include "td_common.h"

namespace {

constexpr int kThreads = 256;

// Per-file descriptor: the host uploads one of these per file / trial (not per
// strip, block or window); kernels find their file with a binary search on
// `first`, the running count of work items (strips, blocks) before the file.
struct FileDesc {
  long long row0;   // global first INPUT row of the file's (offset-shifted) stream
  long long nrows;  // rows in that stream
  long long out0;   // global OUTPUT row of stream frame 0
  long long first;  // index of the file's first work item
};

// Largest f in [0, n) with files[f].first <= idx (files with no items share their
// successor's `first` and are skipped).
__device__ __forceinline__ int find_file(const FileDesc* __restrict__ files, int n, long long idx) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (files[mid].first <= idx) lo = mid; else hi = mid - 1;
  }
  return lo;
}

}  // namespace

// The FIR prediction on whichever kernel fits the shape (decode.hip).   `shift` leading rows of every file are
// dropped before context is added; w_file_stride / b_file_stride (floats): every file under weights of its own.
int td_launch_fir(td_handle* h, const float* x, int64_t ldx, const int64_t* offs, int num_files,
                  int c, int pre, int post, const float* w, const float* bias, int d, float* out,
                  int64_t ldout, int64_t shift = 0, int64_t w_file_stride = 0, int64_t b_file_stride = 0);
