// The statistics between objects, ranks and processes: the sum of several objects (td_stats_combine) and
// the flat float64 form an all-reduce carries (td_stats_packed_len / _pack / _unpack*).
#include "stats_common.h"

namespace {

__global__ void f2d_kernel(double* __restrict__ dst, const float* __restrict__ src, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    dst[i] = (double)src[i];
}

__global__ void d2f_kernel(float* __restrict__ dst, const double* __restrict__ src, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    dst[i] = (float)src[i];
}

inline int blocks_for(long long n) {
  long long b = td_ceil_div(n, 256);
  return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

}  // namespace

extern "C" {

// dst = sum of srcs: ONE launch for the additive block (an n-way sum through a table of source
// pointers, summed in source order like a chain of axpy) and one per boundary-window array (a
// gather of the sources' per-file windows, in source order).  (One axpy + one or two copies
// per source cost the leave-one-out sweep of 32 recordings ~4000 launches: 6 ms of device time
// and 13 ms of gaps while the host queued them.)
struct CombineSrc {
  const double* g;
  const float* win1;
  const float* win2;
  long long first_file, n_files;    // slot of the source's first file in dst
};

__global__ void combine_sum_kernel(const CombineSrc* __restrict__ srcs, int n, long long len,
                                   double* __restrict__ dst) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < len;
       i += (long long)gridDim.x * blockDim.x) {
    double v = 0.0;
    for (int k = 0; k < n; ++k) v += srcs[k].g[i];
    dst[i] = v;
  }
}

// blockIdx.y = source; per = floats of one file's windows
__global__ void combine_windows_kernel(const CombineSrc* __restrict__ srcs, long long per,
                                       int which, float* __restrict__ dst) {
  const CombineSrc s = srcs[blockIdx.y];
  const float* src = which == 0 ? s.win1 : s.win2;
  const long long len = per * s.n_files;
  float* d = dst + per * s.first_file;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < len;
       i += (long long)gridDim.x * blockDim.x)
    d[i] = src[i];
}

int td_stats_combine(td_handle* h, td_stats* dst, td_stats* const* srcs, int n) {
  if (!h || !dst || (n > 0 && !srcs)) return td_fail(h, TD_ERR_INVALID, "td_stats_combine: NULL");
  TD_TRY(td_stats_reset(h, dst));
  if (n == 0) return stats_materialize(h, dst);
  int64_t files = 0;
  for (int i = 0; i < n; ++i) {
    const td_stats* s = srcs[i];
    TD_REQUIRE(h, s && s != dst && s->g_len == dst->g_len && s->c1 == dst->c1 && s->c2 == dst->c2 &&
                      s->l1 == dst->l1 && s->l2 == dst->l2 && s->d == dst->d &&
                      s->pre1 == dst->pre1 && s->pre2 == dst->pre2,
               "td_stats_combine: layouts differ");
    files += s->n_files;
  }
  for (int i = 0; i < n; ++i) TD_TRY(stats_materialize(h, srcs[i]));
  dst->fresh_main = dst->fresh_tgt = false;    // combine_sum_kernel writes every number of dst->g
  TD_TRY(ensure_window_capacity(h, dst, files));
  std::vector<CombineSrc> table((size_t)n);
  int64_t frames = 0, slot = 0, max_files = 0;
  for (int i = 0; i < n; ++i) {
    const td_stats* s = srcs[i];
    table[i] = CombineSrc{s->g, s->win1, s->win2, (long long)slot, (long long)s->n_files};
    slot += s->n_files;
    frames += s->frames;
    max_files = s->n_files > max_files ? s->n_files : max_files;
  }
  const void* table_dev = nullptr;
  TD_TRY(td_table_upload(h, table.data(), sizeof(CombineSrc) * table.size(), &table_dev));
  const CombineSrc* tp = reinterpret_cast<const CombineSrc*>(table_dev);
  hipLaunchKernelGGL(combine_sum_kernel, dim3(blocks_for(dst->g_len)), dim3(256), 0, h->stream, tp, n,
                     (long long)dst->g_len, dst->g);
  if (max_files > 0) {
    const long long per1 = stats_window_floats(dst, dst->c1);
    const long long per2 = stats_window_floats(dst, dst->c2);
    const unsigned bx = (unsigned)td_ceil_div(per1 * max_files, 256);
    hipLaunchKernelGGL(combine_windows_kernel, dim3(bx < 64 ? bx : 64, (unsigned)n), dim3(256), 0,
                       h->stream, tp, per1, 0, dst->win1);
    if (dst->c2) {
      const unsigned bx2 = (unsigned)td_ceil_div(per2 * max_files, 256);
      hipLaunchKernelGGL(combine_windows_kernel, dim3(bx2 < 64 ? bx2 : 64, (unsigned)n), dim3(256),
                         0, h->stream, tp, per2, 1, dst->win2);
    }
  }
  dst->n_files = files;
  dst->frames = frames;
  dst->whole_files = false;
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_stats_packed_len(td_handle* h, const td_stats* s, int64_t total_file_slots,
                        int64_t* num_doubles) {
  if (!s || !num_doubles) return td_fail(h, TD_ERR_INVALID, "td_stats_packed_len: NULL");
  const int64_t per = stats_window_floats(s, s->c1 + s->c2);
  *num_doubles = s->g_len + per * total_file_slots;
  return TD_OK;
}

int td_stats_pack(td_handle* h, const td_stats* s, double* buf_dev, int64_t total_file_slots,
                  int64_t file_slot) {
  if (!h || !s || !buf_dev) return td_fail(h, TD_ERR_INVALID, "td_stats_pack: NULL");
  TD_TRY(stats_materialize(h, const_cast<td_stats*>(s)));
  TD_REQUIRE(h, file_slot >= 0 && file_slot + s->n_files <= total_file_slots,
             "td_stats_pack: files [%lld, %lld) do not fit %lld slots", (long long)file_slot,
             (long long)(file_slot + s->n_files), (long long)total_file_slots);
  int64_t len = 0;
  td_stats_packed_len(h, s, total_file_slots, &len);
  TD_HIP(h, hipMemsetAsync(buf_dev, 0, sizeof(double) * len, h->stream));
  TD_HIP(h, hipMemcpyAsync(buf_dev, s->g, sizeof(double) * s->g_len, hipMemcpyDeviceToDevice,
                           h->stream));
  const int64_t per1 = stats_window_floats(s, s->c1), per2 = stats_window_floats(s, s->c2);
  double* w1 = buf_dev + s->g_len;
  double* w2 = w1 + per1 * total_file_slots;
  if (s->n_files) {
    hipLaunchKernelGGL(f2d_kernel, dim3(blocks_for(per1 * s->n_files)), dim3(256), 0, h->stream,
                       w1 + per1 * file_slot, s->win1, (long long)(per1 * s->n_files));
    if (s->c2)
      hipLaunchKernelGGL(f2d_kernel, dim3(blocks_for(per2 * s->n_files)), dim3(256), 0, h->stream,
                         w2 + per2 * file_slot, s->win2, (long long)(per2 * s->n_files));
    TD_HIP(h, hipGetLastError());
  }
  return TD_OK;
}

int td_stats_unpack_known(td_handle* h, td_stats* s, const double* buf_dev, int64_t total_file_slots,
                          int64_t total_frames) {
  if (!h || !s || !buf_dev) return td_fail(h, TD_ERR_INVALID, "td_stats_unpack: NULL");
  s->fresh_main = s->fresh_tgt = false;        // every number of g is overwritten below
  TD_TRY(ensure_window_capacity(h, s, total_file_slots));
  TD_HIP(h, hipMemcpyAsync(s->g, buf_dev, sizeof(double) * s->g_len, hipMemcpyDeviceToDevice,
                           h->stream));
  const int64_t per1 = stats_window_floats(s, s->c1), per2 = stats_window_floats(s, s->c2);
  const double* w1 = buf_dev + s->g_len;
  const double* w2 = w1 + per1 * total_file_slots;
  if (total_file_slots) {
    hipLaunchKernelGGL(d2f_kernel, dim3(blocks_for(per1 * total_file_slots)), dim3(256), 0,
                       h->stream, s->win1, w1, (long long)(per1 * total_file_slots));
    if (s->c2)
      hipLaunchKernelGGL(d2f_kernel, dim3(blocks_for(per2 * total_file_slots)), dim3(256), 0,
                         h->stream, s->win2, w2, (long long)(per2 * total_file_slots));
    TD_HIP(h, hipGetLastError());
  }
  s->n_files = total_file_slots;
  s->whole_files = false;
  if (total_frames >= 0) {
    s->frames = total_frames;
  } else {
    double nd = 0.0;
    TD_HIP(h, hipMemcpyAsync(&nd, s->g + s->off_n, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    TD_HIP(h, hipStreamSynchronize(h->stream));
    s->frames = (int64_t)(nd + 0.5);
  }
  return TD_OK;
}

int td_stats_unpack(td_handle* h, td_stats* s, const double* buf_dev, int64_t total_file_slots) {
  return td_stats_unpack_known(h, s, buf_dev, total_file_slots, -1);
}

}  // extern "C"
