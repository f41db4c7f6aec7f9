// BioSemi BDF (ingest_bdf.py): 24-bit little-endian two's-complement samples at any byte alignment.
//
//   td_raw24_decode   out[s, r n + i] = scale[s] * (offset[s] + double(x)), x the sign-extended sample
//                     b0 | b1 << 8 | b2 << 16 at byte data_offset + r record_bytes + signal_offset[s] + 3 i of the
//                     image.  td_raw_decode's description of a file (records of record_bytes bytes, signal s n
//                     consecutive samples from its own byte offset), without its alignment conditions: 3 divides
//                     nothing here, so no load of a sample is aligned and none is attempted.
//
// One route, correct for every n >= 1.  A run is the 3 n contiguous bytes of one signal in one record; a lane takes a
// quad, 4 consecutive samples of a run (the run's last quad may hold fewer): 12 bytes at any alignment, which lie in
// at most 4 aligned dwords.  The lane loads those dwords (only the ones that hold a byte of its own samples: a dword
// may start before the run, inside the image, never at or past image_bytes -- the image's last partial dword is read
// byte by byte), shifts the 16 bytes down by the run's misalignment with three v_alignbyte_b32, cuts the four samples
// out with two more, and stores 32 bytes: two 16-byte stores where the first sample's place in the row is 16-byte
// aligned, else 8 + 16 + 8.  Consecutive lanes take consecutive quads of a run, so a wave stores 2 KB contiguous.
// 12 q is a multiple of 4, so the misalignment is the same for every quad of a run.
//
// Every byte offset into the image, the record index, the quad index over all records and the output index are
// 64-bit; what is 32-bit is a byte's place within a lane's 16 bytes, a sample's place within its quad and the signal
// (<= 1024).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "td_common.h"
#include "td_hotpath.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSignals = 1024;
constexpr int kQuad = 4;                 // samples per lane

struct Raw24Signal {
  long long off;       // bytes from the start of a record
  double scale, add;
};
struct Raw24Params {
  const uint8_t* image;
  long long image_bytes, data_offset, records, record_bytes;
  int n, num;
  const Raw24Signal* sig;
  double* out;
  long long ld_out;
};

// The aligned dword at byte a of the image (a < image_bytes); the bytes at or past image_bytes read as 0.
__device__ __forceinline__ uint32_t raw24_dword(const uint8_t* image, long long a, long long image_bytes) {
  if (a + 4 <= image_bytes) return *reinterpret_cast<const uint32_t*>(image + a);
  uint32_t d = 0;
  for (int k = 0; k < 3; ++k)
    if (a + k < image_bytes) d |= (uint32_t)image[a + k] << (8 * k);
  return d;
}

__device__ __forceinline__ double raw24_value(uint32_t low24, const Raw24Signal& S) {
  const int x = (int)(low24 << 8) >> 8;                         // sign extension of bit 23
  return __dmul_rn(S.scale, __dadd_rn(S.add, (double)x));       // one rounding each, no contraction: numpy's bits
}

__global__ __launch_bounds__(kThreads) void raw24_kernel(Raw24Params p) {
  const int s = blockIdx.y;
  const Raw24Signal S = p.sig[s];
  const long long quads = ((long long)p.n + kQuad - 1) / kQuad;  // per run
  const long long total = p.records * quads;
  const bool small = total < (1ll << 32);                       // (a 64-bit division is several times the work)
  const long long first = p.data_offset + S.off;
  double* row = p.out + (long long)s * p.ld_out;
  for (long long idx = (long long)blockIdx.x * kThreads + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * kThreads) {
    const long long r = small ? (long long)((unsigned)idx / (unsigned)quads) : idx / quads;
    const int i0 = (int)(idx - r * quads) * kQuad;              // the quad's first sample in the run (< n)
    const int cnt = p.n - i0 < kQuad ? p.n - i0 : kQuad;
    const long long b = first + r * p.record_bytes + 3ll * i0;  // the quad's first byte
    const long long a0 = b & ~3ll;
    const int sh = (int)(b & 3);
    const int used = sh + 3 * cnt;                              // bytes from a0 to the end of the quad's samples (<= 15)
    uint32_t d0 = raw24_dword(p.image, a0, p.image_bytes), d1 = 0, d2 = 0, d3 = 0;
    if (used > 4) d1 = raw24_dword(p.image, a0 + 4, p.image_bytes);
    if (used > 8) d2 = raw24_dword(p.image, a0 + 8, p.image_bytes);
    if (used > 12) d3 = raw24_dword(p.image, a0 + 12, p.image_bytes);
    // the 12 bytes of the quad, from bit 0 of e0
    const uint32_t e0 = __builtin_amdgcn_alignbyte(d1, d0, sh);
    const uint32_t e1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
    const uint32_t e2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
    const double v0 = raw24_value(e0, S);
    const double v1 = raw24_value(__builtin_amdgcn_alignbyte(e1, e0, 3), S);
    const double v2 = raw24_value(__builtin_amdgcn_alignbyte(e2, e1, 2), S);
    const double v3 = raw24_value(e2 >> 8, S);
    double* dst = row + r * p.n + i0;
    if (cnt == kQuad) {
      if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<double2*>(dst) = make_double2(v0, v1);
        *reinterpret_cast<double2*>(dst + 2) = make_double2(v2, v3);
      } else {
        dst[0] = v0;
        *reinterpret_cast<double2*>(dst + 1) = make_double2(v1, v2);
        dst[3] = v3;
      }
    } else {
      dst[0] = v0;
      if (cnt > 1) dst[1] = v1;
      if (cnt > 2) dst[2] = v2;
    }
  }
}

}  // namespace

extern "C" {

int td_raw24_decode(td_handle* h, const uint8_t* image_dev, int64_t image_bytes, int64_t data_offset, int64_t records,
                    int64_t record_bytes, int samples_per_record, int num_signals, const int64_t* signal_offset_host,
                    const double* scale_host, const double* offset_host, double* out_dev, int64_t ld_out) {
  if (!h || !image_dev || !signal_offset_host || !scale_host || !offset_host || !out_dev)
    return td_fail(h, TD_ERR_INVALID, "td_raw24_decode: NULL argument");
  const int n = samples_per_record;
  TD_REQUIRE(h, n >= 1 && records >= 0 && record_bytes >= 1 && image_bytes >= 0 && data_offset >= 0,
             "td_raw24_decode: bad sizes");
  TD_REQUIRE(h, num_signals >= 1 && num_signals <= kMaxSignals, "td_raw24_decode: 1 .. %d signals, not %d", kMaxSignals,
             num_signals);
  TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(image_dev) & 15) == 0, "td_raw24_decode: the image must be 16-byte aligned");
  TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(out_dev) & 7) == 0, "td_raw24_decode: misaligned output");
  TD_REQUIRE(h, data_offset <= image_bytes && records <= (image_bytes - data_offset) / record_bytes,
             "td_raw24_decode: %lld records of %lld bytes from byte %lld do not fit an image of %lld bytes",
             (long long)records, (long long)record_bytes, (long long)data_offset, (long long)image_bytes);
  TD_REQUIRE(h, 3ll * n <= record_bytes && ld_out >= records * n,
             "td_raw24_decode: row stride %lld below %lld records of %d samples (or a record smaller than one signal)",
             (long long)ld_out, (long long)records, n);
  std::vector<Raw24Signal> sig(num_signals);
  for (int s = 0; s < num_signals; ++s) {
    const long long off = signal_offset_host[s];
    TD_REQUIRE(h, off >= 0 && off + 3ll * n <= record_bytes,
               "td_raw24_decode: signal %d: bytes [%lld, +%lld) are outside the record of %lld bytes", s, off, 3ll * n,
               (long long)record_bytes);
    sig[s].off = off;
    sig[s].scale = scale_host[s];
    sig[s].add = offset_host[s];
  }
  if (records == 0) return TD_OK;
  const void* sig_dev = nullptr;
  TD_TRY(td_table_upload(h, sig.data(), sig.size() * sizeof(Raw24Signal), &sig_dev));
  Raw24Params p;
  p.image = image_dev;
  p.image_bytes = image_bytes;
  p.data_offset = data_offset;
  p.records = records;
  p.record_bytes = record_bytes;
  p.n = n;
  p.num = num_signals;
  p.sig = static_cast<const Raw24Signal*>(sig_dev);
  p.out = out_dev;
  p.ld_out = ld_out;
  long long blocks = td_ceil_div(records * td_ceil_div(n, kQuad), kThreads);
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(raw24_kernel, dim3((unsigned)blocks, (unsigned)num_signals), dim3(kThreads), 0, h->stream, p);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

}  // extern "C"
