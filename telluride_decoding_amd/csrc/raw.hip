// Raw recordings (ingest_brainvision.py, ingest_edf.py): one uploaded file image becomes a channel-major matrix, and
// the chosen channels become the [frames, width] float32 feature 'eeg' (BrainTrial.assemble_brain_data).
//
//   td_raw_decode        out[s, r n + i] = f(sample i of signal s in data record r).  A record is record_bytes
//                        bytes; signal s holds n consecutive samples at its own byte offset in it.  That one
//                        description is BrainVision MULTIPLEXED (n = 1, a record is a frame), BrainVision
//                        VECTORIZED (one record, n = frames) and EDF (n samples per data record).  Samples are
//                        little-endian int16 or float32.  f is one float32 multiply (arith 0) or the float64
//                        scale * (offset + x) (arith 1), each operation rounded once: numpy's bits.
//     direct route       consecutive lanes take consecutive output samples of one signal: coalesced stores, loads in
//                        runs of n samples.  Correct for every n.
//     transposing route  (td_raw_route: n * sample size < 64 bytes and a tile of records fits the staging area)
//                        a workgroup copies `tile` consecutive records -- one contiguous byte range of the file --
//                        into LDS with 16-byte loads and turns them there.  Every record starts a row of an odd
//                        number of dwords, so the lanes that then read one signal of consecutive records fall on
//                        distinct banks; on the way in a lane writes the four dwords of its 16 bytes in an order
//                        rotated by lane / 8, so that the lanes 8 apart, whose chunks are 32 dwords apart, do not
//                        meet on a bank either.
//   td_columns_assemble  up to 1024 [frames, w_k] float32 / float64 sources side by side as one float32 matrix in
//                        one launch.  All w_k == 1 (rows of the decode's matrix) and >= 16 of them: a 64 x 64
//                        tiled transpose through LDS (padded rows), loads along frames, stores along columns.
//                        Otherwise one lane per output element.
//
// Every byte and element index is 64-bit; what is 32-bit is bounded by a tile (<= 48 KB, <= 128 records of < 32
// samples, <= 1024 signals).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "td_common.h"
#include "td_hotpath.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSignals = 1024;
constexpr int kStageBytes = 48 * 1024;   // LDS bytes of staged records per workgroup
constexpr int kRunBytes = 64;            // the direct route's loads come in runs of n * w bytes: shorter ones transpose
constexpr int kMaxTile = 128, kMinTile = 16;
constexpr int kMaxSources = 1024;
constexpr int kMaxColumns = 65536;
constexpr int kTransposeSources = 16;    // fewer width-1 sources than this: one lane per output element

struct RawSignal {
  long long off;       // bytes from the start of a record
  double scale, add;
};
struct RawParams {
  const uint8_t* image;
  long long data_offset, records, record_bytes;
  int n, num;
  const RawSignal* sig;
  void* out;
  long long ld_out;
};

template <int W>
__device__ __forceinline__ float raw_value(const uint8_t* p) {
  if (W == 2) return (float)*reinterpret_cast<const short*>(p);      // (exact)
  return *reinterpret_cast<const float*>(p);
}

// One rounding per operation, no contraction: numpy's float32 x * float32(scale), float64 scale * (offset + x).
template <int W, int ARITH>
__device__ __forceinline__ void raw_store(void* out, long long at, const uint8_t* src, const RawSignal& S) {
  const float x = raw_value<W>(src);
  if (ARITH == 0)
    static_cast<float*>(out)[at] = __fmul_rn(x, (float)S.scale);
  else
    static_cast<double*>(out)[at] = __dmul_rn(S.scale, __dadd_rn(S.add, (double)x));
}

template <int W, int ARITH>
__global__ __launch_bounds__(kThreads) void raw_direct_kernel(RawParams p) {
  const int s = blockIdx.y;
  const RawSignal S = p.sig[s];
  const long long total = p.records * p.n;
  const bool small = total < (1ll << 32);                       // (a 64-bit division is several times the work)
  const uint8_t* base = p.image + p.data_offset + S.off;
  const long long row = (long long)s * p.ld_out;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const long long r = small ? (long long)((unsigned)i / (unsigned)p.n) : i / p.n;
    const long long k = i - r * p.n;
    raw_store<W, ARITH>(p.out, row + i, base + r * p.record_bytes + k * W, S);
  }
}

__device__ __forceinline__ uint32_t pick4(const uint4& v, int j) {
  return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w));
}

// Byte `rel` of the tile (a multiple of W) -> its place in the padded rows.
__device__ __forceinline__ int stage_at(int rel, int record_bytes, int rowpad) {
  const int r = (int)((unsigned)rel / (unsigned)record_bytes);
  return r * rowpad + (rel - r * record_bytes);
}

template <int W, int ARITH>
__global__ __launch_bounds__(kThreads) void raw_transpose_kernel(RawParams p, int tile, int rowpad) {
  extern __shared__ uint4 raw_smem4[];
  uint8_t* stage = reinterpret_cast<uint8_t*>(raw_smem4);
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * tile;
  const int nrec = (int)(p.records - r0 < tile ? p.records - r0 : tile);
  const int B = (int)p.record_bytes;                            // (<= kStageBytes on this route)
  const long long begin = p.data_offset + r0 * p.record_bytes;  // bytes of the image, multiples of W
  const long long end = begin + (long long)nrec * B;            // <= data_offset + records * record_bytes
  const long long begin16 = begin & ~15ll;
  const int chunks = (int)((end - begin16 + 15) >> 4);

  for (int q = tid; q < chunks; q += kThreads) {
    const long long a = begin16 + 16ll * q;
    if (a >= begin && a + 16 <= end) {
      const uint4 v = *reinterpret_cast<const uint4*>(p.image + a);
      const int rel = (int)(a - begin);
      if (W == 4) {
        const int rot = (tid >> 3) & 3;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int j = (jj + rot) & 3;
          *reinterpret_cast<uint32_t*>(stage + stage_at(rel + 4 * j, B, rowpad)) = pick4(v, j);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t d = pick4(v, j);
          *reinterpret_cast<uint16_t*>(stage + stage_at(rel + 4 * j, B, rowpad)) = (uint16_t)d;
          *reinterpret_cast<uint16_t*>(stage + stage_at(rel + 4 * j + 2, B, rowpad)) = (uint16_t)(d >> 16);
        }
      }
    } else {
      // the tile's first and last 16 bytes of the file: only the samples that are the tile's own
      for (int e = 0; e < 16 / W; ++e) {
        const long long b = a + e * W;
        if (b < begin || b >= end) continue;
        const int at = stage_at((int)(b - begin), B, rowpad);
        if (W == 4) *reinterpret_cast<uint32_t*>(stage + at) = *reinterpret_cast<const uint32_t*>(p.image + b);
        else *reinterpret_cast<uint16_t*>(stage + at) = *reinterpret_cast<const uint16_t*>(p.image + b);
      }
    }
  }
  __syncthreads();

  // consecutive lanes, consecutive samples of one signal: r * rowpad has an odd dword stride
  const int n = p.n;
  const int per = nrec * n;
  const int total = per * p.num;
  const long long col0 = r0 * n;
  for (int idx = tid; idx < total; idx += kThreads) {
    const int s = (int)((unsigned)idx / (unsigned)per);
    const int j = idx - s * per;
    const int r = n == 1 ? j : (int)((unsigned)j / (unsigned)n);
    const int k = j - r * n;
    const RawSignal S = p.sig[s];
    raw_store<W, ARITH>(p.out, (long long)s * p.ld_out + col0 + j, stage + r * rowpad + (int)S.off + k * W, S);
  }
}

// A record's row in the staging area: whole dwords, an odd number of them.
int raw_rowpad(long long record_bytes) {
  long long dwords = (record_bytes + 3) / 4;
  if ((dwords & 1) == 0) ++dwords;
  return (int)(4 * dwords);
}

// Records per workgroup of the transposing route, 0: the direct route.
int raw_tile(int n, int w, long long record_bytes) {
  if ((long long)n * w >= kRunBytes || record_bytes > kStageBytes / kMinTile) return 0;
  const int rowpad = raw_rowpad(record_bytes);
  int t = kMaxTile;
  while (t >= kMinTile && (long long)t * rowpad > kStageBytes) t >>= 1;
  return t >= kMinTile ? t : 0;
}

template <int W, int ARITH>
void raw_launch(td_handle* h, const RawParams& p, int tile) {
  if (tile > 0) {
    const int rowpad = raw_rowpad(p.record_bytes);
    hipLaunchKernelGGL((raw_transpose_kernel<W, ARITH>), dim3((unsigned)td_ceil_div(p.records, tile)), dim3(kThreads),
                       (size_t)tile * rowpad, h->stream, p, tile, rowpad);
  } else {
    long long blocks = td_ceil_div(p.records * p.n, kThreads);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL((raw_direct_kernel<W, ARITH>), dim3((unsigned)blocks, (unsigned)p.num), dim3(kThreads), 0,
                       h->stream, p);
  }
}

// ---------------------------------------------------------------- columns
struct ColSource {
  const void* ptr;
  long long ld;        // elements between rows
  int width, col0;     // columns; the first of them in the output
  int is_f64, pad;
};
struct ColParams {
  const ColSource* src;
  const int* col_src;  // output column -> source
  int num, total_w;
  long long frames;
  uint32_t* out;       // float32 bits
  long long ld_out;
};

__device__ __forceinline__ uint32_t col_bits(const ColSource& S, long long f, int e) {
  const long long at = f * S.ld + e;
  return S.is_f64 ? td_f64_to_f32_bits(static_cast<const uint64_t*>(S.ptr)[at]) : static_cast<const uint32_t*>(S.ptr)[at];
}

// Every source one column: tile [64 sources][64 frames], rows padded by one dword.
__global__ __launch_bounds__(kThreads) void columns_transpose_kernel(ColParams p) {
  __shared__ uint32_t tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long long f0 = (long long)blockIdx.x * 64;
  const int k0 = blockIdx.y * 64;
  for (int kk = ty; kk < 64; kk += 4) {
    const int k = k0 + kk;
    if (k < p.num && f0 + tx < p.frames) tile[kk][tx] = col_bits(p.src[k], f0 + tx, 0);
  }
  __syncthreads();
  for (int ff = ty; ff < 64; ff += 4) {
    const long long f = f0 + ff;
    if (f < p.frames && k0 + tx < p.num) p.out[f * p.ld_out + k0 + tx] = tile[tx][ff];
  }
}

__global__ __launch_bounds__(kThreads) void columns_gather_kernel(ColParams p) {
  const long long total = p.frames * p.total_w;
  const bool small = total < (1ll << 32);
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const long long f = small ? (long long)((unsigned)i / (unsigned)p.total_w) : i / p.total_w;
    const int j = (int)(i - f * p.total_w);
    const ColSource S = p.src[p.col_src[j]];
    p.out[f * p.ld_out + j] = col_bits(S, f, j - S.col0);
  }
}

bool columns_transposed(int num_sources, int max_width) { return max_width == 1 && num_sources >= kTransposeSources; }

}  // namespace

extern "C" {

int td_raw_route(int samples_per_record, int sample_bytes, int64_t record_bytes, int* transposed, int* tile_records) {
  if (samples_per_record < 1 || (sample_bytes != 2 && sample_bytes != 4) || !transposed || !tile_records ||
      record_bytes < (int64_t)samples_per_record * sample_bytes || record_bytes % sample_bytes)
    return TD_ERR_INVALID;
  *tile_records = raw_tile(samples_per_record, sample_bytes, record_bytes);
  *transposed = *tile_records > 0 ? 1 : 0;
  return TD_OK;
}

int td_raw_decode(td_handle* h, const uint8_t* image_dev, int64_t image_bytes, int64_t data_offset, int64_t records,
                  int64_t record_bytes, int samples_per_record, int sample_kind, int num_signals,
                  const int64_t* signal_offset_host, const double* scale_host, const double* offset_host, int arith,
                  void* out_dev, int64_t ld_out) {
  if (!h || !image_dev || !signal_offset_host || !scale_host || !offset_host || !out_dev)
    return td_fail(h, TD_ERR_INVALID, "td_raw_decode: NULL argument");
  TD_REQUIRE(h, sample_kind == TD_RAW_INT16 || sample_kind == TD_RAW_FLOAT32, "td_raw_decode: sample kind %d is neither "
             "int16 (%d) nor float32 (%d)", sample_kind, TD_RAW_INT16, TD_RAW_FLOAT32);
  TD_REQUIRE(h, arith == 0 || arith == 1, "td_raw_decode: arith %d is neither 0 nor 1", arith);
  const int w = sample_kind == TD_RAW_INT16 ? 2 : 4;
  const int n = samples_per_record;
  TD_REQUIRE(h, n >= 1 && records >= 0 && record_bytes >= 1 && image_bytes >= 0 && data_offset >= 0,
             "td_raw_decode: bad sizes");
  TD_REQUIRE(h, num_signals >= 1 && num_signals <= kMaxSignals, "td_raw_decode: 1 .. %d signals, not %d", kMaxSignals,
             num_signals);
  TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(image_dev) & 15) == 0, "td_raw_decode: the image must be 16-byte aligned");
  TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(out_dev) & (arith ? 7 : 3)) == 0, "td_raw_decode: misaligned output");
  TD_REQUIRE(h, data_offset % w == 0 && record_bytes % w == 0,
             "td_raw_decode: data offset %lld and record size %lld must be multiples of the sample size %d",
             (long long)data_offset, (long long)record_bytes, w);
  TD_REQUIRE(h, data_offset <= image_bytes && records <= (image_bytes - data_offset) / record_bytes,
             "td_raw_decode: %lld records of %lld bytes from byte %lld do not fit an image of %lld bytes",
             (long long)records, (long long)record_bytes, (long long)data_offset, (long long)image_bytes);
  TD_REQUIRE(h, (long long)n * w <= record_bytes && ld_out >= records * n,
             "td_raw_decode: row stride %lld below %lld records of %d samples (or a record smaller than one signal)",
             (long long)ld_out, (long long)records, n);
  std::vector<RawSignal> sig(num_signals);
  for (int s = 0; s < num_signals; ++s) {
    const long long off = signal_offset_host[s];
    TD_REQUIRE(h, off >= 0 && off % w == 0 && off + (long long)n * w <= record_bytes,
               "td_raw_decode: signal %d: bytes [%lld, +%lld) are outside the record of %lld bytes or not aligned to %d",
               s, off, (long long)n * w, (long long)record_bytes, w);
    TD_REQUIRE(h, arith == 1 || offset_host[s] == 0.0, "td_raw_decode: signal %d: arith 0 takes no offset", s);
    sig[s].off = off;
    sig[s].scale = scale_host[s];
    sig[s].add = offset_host[s];
  }
  if (records == 0) return TD_OK;
  const int tile = raw_tile(n, w, record_bytes);
  TD_REQUIRE(h, td_ceil_div(records, tile > 0 ? tile : 1) <= 0x7fffffffll || tile == 0,
             "td_raw_decode: too many records for one launch");
  const void* sig_dev = nullptr;
  TD_TRY(td_table_upload(h, sig.data(), sig.size() * sizeof(RawSignal), &sig_dev));
  RawParams p;
  p.image = image_dev;
  p.data_offset = data_offset;
  p.records = records;
  p.record_bytes = record_bytes;
  p.n = n;
  p.num = num_signals;
  p.sig = static_cast<const RawSignal*>(sig_dev);
  p.out = out_dev;
  p.ld_out = ld_out;
  if (w == 2 && arith == 0) raw_launch<2, 0>(h, p, tile);
  else if (w == 2) raw_launch<2, 1>(h, p, tile);
  else if (arith == 0) raw_launch<4, 0>(h, p, tile);
  else raw_launch<4, 1>(h, p, tile);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_columns_route(int num_sources, int max_width, int* transposed) {
  if (num_sources < 1 || num_sources > kMaxSources || max_width < 1 || !transposed) return TD_ERR_INVALID;
  *transposed = columns_transposed(num_sources, max_width) ? 1 : 0;
  return TD_OK;
}

int td_columns_assemble(td_handle* h, int num_sources, const void* const* src_dev, const int64_t* ld_host,
                        const int* width_host, const int* is_f64_host, int64_t frames, float* out_dev, int64_t ld_out) {
  if (!h || !src_dev || !ld_host || !width_host || !is_f64_host || (!out_dev && frames > 0))
    return td_fail(h, TD_ERR_INVALID, "td_columns_assemble: NULL argument");
  TD_REQUIRE(h, num_sources >= 1 && num_sources <= kMaxSources, "td_columns_assemble: 1 .. %d sources, not %d",
             kMaxSources, num_sources);
  TD_REQUIRE(h, frames >= 0, "td_columns_assemble: bad sizes");
  TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(out_dev) & 3) == 0, "td_columns_assemble: misaligned output");
  // one table: the sources, then the source of every output column
  std::vector<ColSource> src(num_sources);
  long long total_w = 0;
  int max_width = 1;
  for (int k = 0; k < num_sources; ++k) {
    const int f64 = is_f64_host[k] ? 1 : 0;
    TD_REQUIRE(h, width_host[k] >= 1 && (frames <= 1 || ld_host[k] >= width_host[k]) && (src_dev[k] || frames == 0),
               "td_columns_assemble: source %d: bad pointer, width or row stride", k);
    TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(src_dev[k]) & (f64 ? 7 : 3)) == 0,
               "td_columns_assemble: source %d: misaligned", k);
    src[k].ptr = src_dev[k];
    src[k].ld = ld_host[k];
    src[k].width = width_host[k];
    src[k].col0 = (int)total_w;
    src[k].is_f64 = f64;
    src[k].pad = 0;
    total_w += width_host[k];
    if (width_host[k] > max_width) max_width = width_host[k];
    TD_REQUIRE(h, total_w <= kMaxColumns, "td_columns_assemble: more than %d columns", kMaxColumns);
  }
  TD_REQUIRE(h, ld_out >= total_w, "td_columns_assemble: row stride %lld below the %lld columns", (long long)ld_out,
             total_w);
  if (frames == 0) return TD_OK;
  const size_t src_bytes = src.size() * sizeof(ColSource);
  std::vector<char> tab(src_bytes + (size_t)total_w * sizeof(int));
  memcpy(tab.data(), src.data(), src_bytes);
  int* col_src = reinterpret_cast<int*>(tab.data() + src_bytes);
  for (int k = 0; k < num_sources; ++k)
    for (int e = 0; e < src[k].width; ++e) col_src[src[k].col0 + e] = k;
  const void* tab_dev = nullptr;
  TD_TRY(td_table_upload(h, tab.data(), tab.size(), &tab_dev));
  ColParams p;
  p.src = static_cast<const ColSource*>(tab_dev);
  p.col_src = reinterpret_cast<const int*>(static_cast<const char*>(tab_dev) + src_bytes);
  p.num = num_sources;
  p.total_w = (int)total_w;
  p.frames = frames;
  p.out = reinterpret_cast<uint32_t*>(out_dev);
  p.ld_out = ld_out;
  if (columns_transposed(num_sources, max_width)) {
    TD_REQUIRE(h, td_ceil_div(frames, 64) <= 0x7fffffffll, "td_columns_assemble: too many frames for one launch");
    hipLaunchKernelGGL(columns_transpose_kernel, dim3((unsigned)td_ceil_div(frames, 64), (unsigned)td_ceil_div(num_sources, 64)),
                       dim3(kThreads), 0, h->stream, p);
  } else {
    long long blocks = td_ceil_div(frames * total_w, kThreads);
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(columns_gather_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, h->stream, p);
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

}  // extern "C"
