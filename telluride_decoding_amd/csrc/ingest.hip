// Ingestion (ingest.py): the joint moments of a list of trials, the z-score, and the TFRecord file image of one
// trial, built on the device from device-resident features.
//
//   td_ingest_moments    two passes in float64 over a pointer table of trials: column sums -> means, then the
//                        sums of centred squares against those means (never the one-pass sum of squares, which
//                        cancels on data with a DC offset).  Four launches whatever the number of trials.
//   td_ingest_normalize  (a - mean) / std with numpy's result types; the subtraction and the division are the
//                        correctly rounded IEEE operations (no reciprocal, no fast-math on the build line).
//   td_tfrecord_encode   frames x stride bytes of TFRecord file, one tf.train.Example per frame.  Every record of
//                        a trial is the same bytes outside its float payloads and its data CRC, so the host hands
//                        over ONE record template and the payload byte offsets (arbitrary: nothing in a record is
//                        4-byte aligned).  Staged route: a workgroup builds `group` records in LDS -- template
//                        words, payload bytes, masked CRC-32C -- and stores the group's byte range, which starts
//                        16-byte aligned because group * stride is a multiple of 16, with 16-byte stores.  Large
//                        route (a record that does not fit the staging area, td_tfrecord_route): one workgroup
//                        per record composes aligned words straight from the inputs.
//
// CRC-32C of a record: `lanes` lanes each run the byte-table CRC over their piece (the first piece from the
// initial register 0xffffffff, the others from 0); the register is linear over GF(2) in (state, data), so
// state(A | B) = advance_|B|(state(A)) ^ state_from_0(B), and advance by a fixed number of zero bytes is four table
// look-ups.  All pieces but the first have the same length, so one advance table serves a launch.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "td_common.h"
#include "td_hotpath.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxFeatures = 16;
constexpr int kStageBytes = 48 * 1024;       // LDS bytes of staged records per workgroup
constexpr int kTabWords = 256 + 4 * 256;     // CRC byte table, then the advance table
constexpr unsigned kMaskDelta = 0xa282ead8u;

// ---------------------------------------------------------------- encoder
struct EncFeature {
  const void* ptr;
  long long ld;       // elements between rows
  int width, offset;  // floats per row; byte offset of the payload in the record (12 = first data byte)
  int is_f64, reversed;
};
struct EncParams {
  EncFeature f[kMaxFeatures];
  int num, stride;
  long long frames;
};

__device__ __forceinline__ uint32_t load_bits(const EncFeature& F, long long frames, long long row, int e) {
  if (F.reversed) row = frames - 1 - row;
  const long long at = row * F.ld + e;
  return F.is_f64 ? td_f64_to_f32_bits(static_cast<const uint64_t*>(F.ptr)[at]) : static_cast<const uint32_t*>(F.ptr)[at];
}

__device__ __forceinline__ uint32_t crc_advance(const uint32_t* adv, uint32_t c) {
  return adv[c & 0xff] ^ adv[256 + ((c >> 8) & 0xff)] ^ adv[512 + ((c >> 16) & 0xff)] ^ adv[768 + (c >> 24)];
}

__device__ __forceinline__ uint32_t crc_mask(uint32_t reg) {
  const uint32_t crc = ~reg;
  return ((crc >> 15) | (crc << 17)) + kMaskDelta;
}

// tabs: kTabWords of tables, then the template repeated four times as `stride` words (word w of the file is
// word w % stride of it, because 4 * stride bytes is a whole number of records).
__global__ __launch_bounds__(kThreads) void encode_staged_kernel(EncParams p, const uint32_t* __restrict__ tabs,
                                                                 int group, int lanes, int piece,
                                                                 uint8_t* __restrict__ out) {
  extern __shared__ uint4 smem4[];
  uint32_t* crc_tab = reinterpret_cast<uint32_t*>(smem4);
  uint32_t* adv = crc_tab + 256;
  uint32_t* part = crc_tab + kTabWords;                         // [kThreads]
  uint32_t* stage32 = part + kThreads;                          // byte offset 6144: 16-byte aligned
  uint8_t* stage = reinterpret_cast<uint8_t*>(stage32);
  const int tid = threadIdx.x;
  const int stride = p.stride;
  const long long r0 = (long long)blockIdx.x * group;
  const int nrec = (int)(p.frames - r0 < group ? p.frames - r0 : group);
  const int nbytes = nrec * stride;
  const uint32_t* tmpl4 = tabs + kTabWords;

  for (int i = tid; i < kTabWords; i += kThreads) crc_tab[i] = tabs[i];
  const int nwords = (nbytes + 3) >> 2;                         // <= group * stride / 4 (a multiple of 16 bytes)
  const unsigned w0 = (unsigned)((((unsigned long long)r0 * (unsigned)stride) >> 2) % (unsigned)stride);
  for (int w = tid; w < nwords; w += kThreads) stage32[w] = tmpl4[(w0 + (unsigned)w) % (unsigned)stride];
  __syncthreads();

  for (int f = 0; f < p.num; ++f) {
    const EncFeature& F = p.f[f];
    const int total = nrec * F.width;
    for (int idx = tid; idx < total; idx += kThreads) {
      const int r = idx / F.width, e = idx - r * F.width;
      const uint32_t bits = load_bits(F, p.frames, r0 + r, e);
      uint8_t* d = stage + r * stride + F.offset + 4 * e;
      d[0] = (uint8_t)bits; d[1] = (uint8_t)(bits >> 8); d[2] = (uint8_t)(bits >> 16); d[3] = (uint8_t)(bits >> 24);
    }
  }
  __syncthreads();

  const int rec = tid / lanes, k = tid - rec * lanes;
  const int len = stride - 16;
  if (rec < nrec) {
    const int first = len - (lanes - 1) * piece;
    const int begin = k == 0 ? 0 : first + (k - 1) * piece;
    const int n = k == 0 ? first : piece;
    const uint8_t* src = stage + rec * stride + 12 + begin;
    uint32_t c = k == 0 ? 0xffffffffu : 0u;
    for (int i = 0; i < n; ++i) c = crc_tab[(c ^ src[i]) & 0xff] ^ (c >> 8);
    part[tid] = c;
  }
  __syncthreads();
  if (rec < nrec && k == 0) {
    uint32_t c = part[tid];
    for (int j = 1; j < lanes; ++j) c = crc_advance(adv, c) ^ part[tid + j];
    const uint32_t v = crc_mask(c);
    uint8_t* d = stage + rec * stride + stride - 4;
    d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); d[2] = (uint8_t)(v >> 16); d[3] = (uint8_t)(v >> 24);
  }
  __syncthreads();

  uint8_t* g = out + r0 * stride;                               // 16-byte aligned: group * stride % 16 == 0
  const int n16 = nbytes >> 4;
  for (int i = tid; i < n16; i += kThreads) reinterpret_cast<uint4*>(g)[i] = smem4[(6144 >> 4) + i];
  for (int b = (n16 << 4) + tid; b < nbytes; b += kThreads) g[b] = stage[b];
}

__device__ __forceinline__ uint8_t record_byte(const EncParams& p, const uint8_t* tmpl, long long r, int b) {
  for (int f = 0; f < p.num; ++f) {
    const unsigned d = (unsigned)(b - p.f[f].offset);
    if (d < 4u * (unsigned)p.f[f].width) return (uint8_t)(load_bits(p.f[f], p.frames, r, (int)(d >> 2)) >> (8 * (d & 3)));
  }
  return tmpl[b];
}

// One workgroup per record; tmpl: the record template's `stride` bytes (after the tables and the word template).
__global__ __launch_bounds__(kThreads) void encode_large_kernel(EncParams p, const uint32_t* __restrict__ tabs,
                                                                int piece, uint8_t* __restrict__ out) {
  __shared__ uint32_t crc_tab[kTabWords];
  __shared__ uint32_t part[kThreads];
  const uint32_t* adv = crc_tab + 256;
  const int tid = threadIdx.x;
  const int stride = p.stride;
  const long long r = blockIdx.x;
  const uint8_t* tmpl = reinterpret_cast<const uint8_t*>(tabs + kTabWords + stride);
  for (int i = tid; i < kTabWords; i += kThreads) crc_tab[i] = tabs[i];

  // bytes [0, stride - 4) of the record: whole aligned words of the file, single bytes at both ends
  const long long base = r * stride, end = base + stride - 4;
  long long a0 = (base + 3) & ~3ll;
  if (a0 > end) a0 = end;
  const int head = (int)(a0 - base);
  const int nw = (int)((end - a0) >> 2);
  if (tid < head) out[base + tid] = record_byte(p, tmpl, r, tid);
  for (int w = tid; w < nw; w += kThreads) {
    const int b = head + 4 * w;
    const uint32_t v = (uint32_t)record_byte(p, tmpl, r, b) | ((uint32_t)record_byte(p, tmpl, r, b + 1) << 8) |
                       ((uint32_t)record_byte(p, tmpl, r, b + 2) << 16) | ((uint32_t)record_byte(p, tmpl, r, b + 3) << 24);
    *reinterpret_cast<uint32_t*>(out + a0 + 4ll * w) = v;
  }
  const int tail0 = head + 4 * nw;
  if (tail0 + tid < stride - 4) out[base + tail0 + tid] = record_byte(p, tmpl, r, tail0 + tid);

  const int len = stride - 16;
  const int first = len - (kThreads - 1) * piece;
  const int begin = tid == 0 ? 0 : first + (tid - 1) * piece;
  const int n = tid == 0 ? first : piece;
  uint32_t c = tid == 0 ? 0xffffffffu : 0u;
  __syncthreads();                                              // the tables
  for (int i = 0; i < n; ++i) c = crc_tab[(c ^ record_byte(p, tmpl, r, 12 + begin + i)) & 0xff] ^ (c >> 8);
  part[tid] = c;
  __syncthreads();
  if (tid == 0) {
    for (int j = 1; j < kThreads; ++j) c = crc_advance(adv, c) ^ part[j];
    const uint32_t v = crc_mask(c);
    uint8_t* d = out + base + stride - 4;
    d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); d[2] = (uint8_t)(v >> 16); d[3] = (uint8_t)(v >> 24);
  }
}

// ---------------------------------------------------------------- encoder: host side
struct CrcTables {
  uint32_t byte_tab[256];
  std::mutex mu;
  std::map<int, std::vector<uint32_t>> advance;     // piece length -> [4][256]
  CrcTables() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82f63b78u : c >> 1;
      byte_tab[i] = c;
    }
  }
  // advance[j][b]: the register (b << 8 j) after `n` zero bytes
  const std::vector<uint32_t>& advance_by(int n) {
    std::lock_guard<std::mutex> lock(mu);
    auto it = advance.find(n);
    if (it != advance.end()) return it->second;
    uint32_t basis[32];
    for (int bit = 0; bit < 32; ++bit) {
      uint32_t c = 1u << bit;
      for (int i = 0; i < n; ++i) c = byte_tab[c & 0xff] ^ (c >> 8);
      basis[bit] = c;
    }
    std::vector<uint32_t> tab(1024);
    for (int j = 0; j < 4; ++j)
      for (int b = 0; b < 256; ++b) {
        uint32_t c = 0;
        for (int k = 0; k < 8; ++k)
          if (b & (1 << k)) c ^= basis[8 * j + k];
        tab[256 * j + b] = c;
      }
    return advance.emplace(n, std::move(tab)).first->second;
  }
};

CrcTables& crc_tables() {
  static CrcTables t;
  return t;
}

int gcd16(int stride) {
  int g = 16;
  while (stride % g) g >>= 1;
  return g;
}

// The route of a record of `stride` bytes: records per workgroup (0: the large route) and lanes per record's CRC.
void encode_route(int stride, int* group, int* lanes) {
  const int gmin = 16 / gcd16(stride);
  if ((long long)gmin * stride > kStageBytes) {
    *group = 0;
    *lanes = kThreads;
    return;
  }
  int g = (kStageBytes / stride) / gmin * gmin;
  // at most 64 records a workgroup (gmin divides 16): at least four lanes then share a record's CRC, whose
  // byte loop is a chain of dependent LDS look-ups and the longest phase of the kernel
  if (g > kThreads / 4) g = kThreads / 4;
  int l = 1;
  while (l * 2 * g <= kThreads) l *= 2;
  // fewer records with twice the lanes each when that keeps more of the workgroup busy in the CRC pass
  // (1200-byte records: 40 x 4 lanes = 160 threads, or 32 x 8 = 256)
  const int g2 = (kThreads / (2 * l)) / gmin * gmin;
  if (g2 >= gmin && g2 * 2 * l > g * l) {
    g = g2;
    l *= 2;
  }
  *group = g;
  *lanes = l;
}

// ---------------------------------------------------------------- decoder
// The encoder's mirror: one pass over a file image checks every record's skeleton against the template under a
// byte mask, its data CRC, and scatters the float payloads into the caller's tensors.  Failures meet in one
// 64-bit word by atomicMin over (record << 2 | kind): a minimum does not depend on the order of its operands, so
// the status is the same on every call.  Skeleton (1) sorts below CRC (2) at the same record.
constexpr unsigned kBadSkeleton = 1u, kBadCrc = 2u;
constexpr unsigned kNoneBad = 0xffffffffu;
constexpr int kDecStageOffset = 6144 + 16;   // tables, the partial registers, the workgroup's lowest failure

struct DecOutput {
  float* dst;         // row 0 of the file, column `col` already added
  long long ld;       // elements between rows
  int offset, count;  // byte offset of the payload in the record; floats per row
};
struct DecParams {
  DecOutput o[kMaxFeatures];
  int num, stride;
  long long frames;
};

// The 32 bits at byte `at` of a word array (any alignment): two aligned words, funnel-shifted.  Reads word
// (at >> 2) + 1 only when `at` is not a multiple of 4.
template <typename Words>
__device__ __forceinline__ uint32_t bits_at(Words words, long long at) {
  const long long w = at >> 2;
  const unsigned sh = 8u * (unsigned)(at & 3);
  const uint32_t lo = words[w];
  if (sh == 0) return lo;
  return (lo >> sh) | (words[w + 1] << (32u - sh));
}

__device__ __forceinline__ void report_bad(unsigned long long* status, long long record, unsigned kind) {
  atomicMin(status, ((unsigned long long)record << 2) | kind);
}

// tabs: kTabWords of tables, the template four times over as `stride` words, the mask likewise.
__global__ __launch_bounds__(kThreads) void decode_staged_kernel(DecParams p, const uint32_t* __restrict__ tabs,
                                                                 int group, int lanes, int piece,
                                                                 const uint8_t* __restrict__ image,
                                                                 unsigned long long* __restrict__ status) {
  extern __shared__ uint4 smem4[];
  uint32_t* crc_tab = reinterpret_cast<uint32_t*>(smem4);
  const uint32_t* adv = crc_tab + 256;
  uint32_t* part = crc_tab + kTabWords;                         // [kThreads]
  unsigned* bad = part + kThreads;                              // (local record << 2 | kind) of the lowest failure
  uint32_t* stage32 = crc_tab + (kDecStageOffset >> 2);
  const uint8_t* stage = reinterpret_cast<const uint8_t*>(stage32);
  const int tid = threadIdx.x;
  const int stride = p.stride;
  const long long r0 = (long long)blockIdx.x * group;
  const int nrec = (int)(p.frames - r0 < group ? p.frames - r0 : group);
  const int nbytes = nrec * stride;
  const uint32_t* tmpl4 = tabs + kTabWords;
  const uint32_t* mask4 = tmpl4 + stride;

  for (int i = tid; i < kTabWords; i += kThreads) crc_tab[i] = tabs[i];
  if (tid == 0) *bad = kNoneBad;
  const uint8_t* g = image + r0 * stride;                       // 16-byte aligned: group * stride % 16 == 0
  const int n16 = nbytes >> 4;
  for (int i = tid; i < n16; i += kThreads) smem4[(kDecStageOffset >> 4) + i] = reinterpret_cast<const uint4*>(g)[i];
  // the tail of the file's last group, as whole words of zero-padded bytes (nothing past the image is read)
  for (int w = (n16 << 2) + tid; 4 * w < nbytes; w += kThreads) {
    uint32_t v = 0;
    for (int j = 0; j < 4 && 4 * w + j < nbytes; ++j) v |= (uint32_t)g[4 * w + j] << (8 * j);
    stage32[w] = v;
  }
  __syncthreads();

  // skeleton: word w of the group is word (w0 + w) mod stride of the repeated template
  const int nwords = (nbytes + 3) >> 2;
  const unsigned w0 = (unsigned)((((unsigned long long)r0 * (unsigned)stride) >> 2) % (unsigned)stride);
  for (int w = tid; w < nwords; w += kThreads) {
    const unsigned t = (w0 + (unsigned)w) % (unsigned)stride;
    uint32_t diff = (stage32[w] ^ tmpl4[t]) & mask4[t];
    if (4 * w + 4 > nbytes) diff &= 0xffffffffu >> (8 * (4 * w + 4 - nbytes));
    for (int j = 0; diff; ++j, diff >>= 8)                      // (a word may straddle two records)
      if (diff & 0xff) atomicMin(bad, ((unsigned)((4 * w + j) / stride) << 2) | kBadSkeleton);
  }

  // data CRC: the encoder's split
  const int rec = tid / lanes, k = tid - rec * lanes;
  const int len = stride - 16;
  if (rec < nrec) {
    const int first = len - (lanes - 1) * piece;
    const int begin = k == 0 ? 0 : first + (k - 1) * piece;
    const int n = k == 0 ? first : piece;
    const uint8_t* src = stage + rec * stride + 12 + begin;
    uint32_t c = k == 0 ? 0xffffffffu : 0u;
    for (int i = 0; i < n; ++i) c = crc_tab[(c ^ src[i]) & 0xff] ^ (c >> 8);
    part[tid] = c;
  }
  __syncthreads();
  if (rec < nrec && k == 0) {
    uint32_t c = part[tid];
    for (int j = 1; j < lanes; ++j) c = crc_advance(adv, c) ^ part[tid + j];
    if (crc_mask(c) != bits_at(stage32, (long long)rec * stride + stride - 4))
      atomicMin(bad, ((unsigned)rec << 2) | kBadCrc);
  }

  // payloads: consecutive lanes, consecutive floats of the group's rows
  for (int f = 0; f < p.num; ++f) {
    const DecOutput& O = p.o[f];
    const int total = nrec * O.count;
    for (int idx = tid; idx < total; idx += kThreads) {
      const int r = idx / O.count, e = idx - r * O.count;
      const uint32_t bits = bits_at(stage32, (long long)r * stride + O.offset + 4 * e);
      reinterpret_cast<uint32_t*>(O.dst)[(r0 + r) * O.ld + e] = bits;
    }
  }
  __syncthreads();
  if (tid == 0 && *bad != kNoneBad) report_bad(status, r0 + (*bad >> 2), *bad & 3u);
}

// CRC register after the n bytes at image + at: single bytes up to a word boundary, aligned words, single bytes.
__device__ __forceinline__ uint32_t crc_span(const uint32_t* crc_tab, const uint8_t* __restrict__ image, long long at,
                                             int n, uint32_t c) {
  int i = 0;
  for (; i < n && ((at + i) & 3); ++i) c = crc_tab[(c ^ image[at + i]) & 0xff] ^ (c >> 8);
  const uint32_t* words = reinterpret_cast<const uint32_t*>(image + at + i);
  for (int w = 0; i + 4 <= n; ++w, i += 4) {
    uint32_t v = words[w];
    for (int j = 0; j < 4; ++j, v >>= 8) c = crc_tab[(c ^ v) & 0xff] ^ (c >> 8);
  }
  for (; i < n; ++i) c = crc_tab[(c ^ image[at + i]) & 0xff] ^ (c >> 8);
  return c;
}

// One workgroup per record, aligned words straight from the image.
__global__ __launch_bounds__(kThreads) void decode_large_kernel(DecParams p, const uint32_t* __restrict__ tabs,
                                                                int piece, const uint8_t* __restrict__ image,
                                                                unsigned long long* __restrict__ status) {
  __shared__ uint32_t crc_tab[kTabWords];
  __shared__ uint32_t part[kThreads];
  __shared__ unsigned bad;
  const uint32_t* adv = crc_tab + 256;
  const int tid = threadIdx.x;
  const int stride = p.stride;
  const long long r = blockIdx.x;
  const uint32_t* tmpl4 = tabs + kTabWords;
  const uint32_t* mask4 = tmpl4 + stride;
  const uint8_t* tmpl = reinterpret_cast<const uint8_t*>(tmpl4);     // (the first of the four copies)
  const uint8_t* mask = reinterpret_cast<const uint8_t*>(mask4);
  const uint32_t* image32 = reinterpret_cast<const uint32_t*>(image);
  for (int i = tid; i < kTabWords; i += kThreads) crc_tab[i] = tabs[i];
  if (tid == 0) bad = kNoneBad;
  __syncthreads();

  // skeleton: the record's whole aligned words of the file, single bytes at both ends
  const long long base = r * stride, end = base + stride;
  const long long a0 = (base + 3) & ~3ll;                       // (< end: stride >= 17)
  const int head = (int)(a0 - base);
  const int nw = (int)((end - a0) >> 2);
  const unsigned t0 = (unsigned)((unsigned long long)(a0 >> 2) % (unsigned)stride);
  bool differs = false;
  if (tid < head) differs = ((image[base + tid] ^ tmpl[tid]) & mask[tid]) != 0;
  for (int w = tid; w < nw; w += kThreads) {
    const unsigned t = (t0 + (unsigned)w) % (unsigned)stride;
    differs |= ((image32[(a0 >> 2) + w] ^ tmpl4[t]) & mask4[t]) != 0;
  }
  const int tail0 = head + 4 * nw;
  if (tail0 + tid < stride) differs |= ((image[base + tail0 + tid] ^ tmpl[tail0 + tid]) & mask[tail0 + tid]) != 0;
  if (differs) atomicMin(&bad, kBadSkeleton);

  const int len = stride - 16;
  const int first = len - (kThreads - 1) * piece;
  const int begin = tid == 0 ? 0 : first + (tid - 1) * piece;
  part[tid] = crc_span(crc_tab, image, base + 12 + begin, tid == 0 ? first : piece, tid == 0 ? 0xffffffffu : 0u);
  __syncthreads();
  if (tid == 0) {
    uint32_t c = part[0];
    for (int j = 1; j < kThreads; ++j) c = crc_advance(adv, c) ^ part[j];
    uint32_t stored = 0;
    for (int j = 0; j < 4; ++j) stored |= (uint32_t)image[end - 4 + j] << (8 * j);
    if (crc_mask(c) != stored) atomicMin(&bad, kBadCrc);
  }

  for (int f = 0; f < p.num; ++f) {
    const DecOutput& O = p.o[f];
    uint32_t* dst = reinterpret_cast<uint32_t*>(O.dst) + r * O.ld;
    for (int e = tid; e < O.count; e += kThreads) dst[e] = bits_at(image32, base + O.offset + 4ll * e);
  }
  __syncthreads();
  if (tid == 0 && bad != kNoneBad) report_bad(status, r, bad);
}

// The decoder's table for records of `stride` bytes whose CRC pieces are `piece` bytes: the CRC byte table, the
// advance table, then the template and the mask, each four times over as `stride` words.  Host only.
void decode_table(const uint8_t* template_host, const uint8_t* mask_host, int stride, int piece,
                  std::vector<uint32_t>* tab) {
  tab->assign((size_t)kTabWords + 2 * (size_t)stride, 0u);
  CrcTables& ct = crc_tables();
  memcpy(tab->data(), ct.byte_tab, sizeof(ct.byte_tab));
  memcpy(tab->data() + 256, ct.advance_by(piece).data(), 1024 * sizeof(uint32_t));
  uint8_t* t4 = reinterpret_cast<uint8_t*>(tab->data() + kTabWords);
  uint8_t* m4 = t4 + 4 * (size_t)stride;
  for (int k = 0; k < 4; ++k) {
    memcpy(t4 + (size_t)k * stride, template_host, stride);
    for (int b = 0; b < stride; ++b) m4[(size_t)k * stride + b] = mask_host[b] ? 0xff : 0x00;
  }
}

// ---------------------------------------------------------------- moments
struct MomTrial {
  const void* ptr;
  long long rows, ld, chunk0;     // chunk0: the first chunk of this trial in the launch
  int is_f64, pad;
};

// Tree sum over the row slots (tid / wt) of s[kThreads]; the totals end in s[0 .. wt).
__device__ __forceinline__ void reduce_slots(double* s, int tid, int wt, int slots) {
  int top = 1;
  while (top < slots) top <<= 1;
  const int ro = tid / wt;
  for (int h = top >> 1; h >= 1; h >>= 1) {
    __syncthreads();
    if (ro < h && ro + h < slots) s[tid] += s[tid + h * wt];
  }
  __syncthreads();
}

// second == 0: partial[chunk][col] = the column sums of the chunk's rows.  second != 0: partial[chunk][col] = the
// sums of (x - mean of the column)^2 and partial[chunk][width + col] of (x - mean of everything)^2, the means read
// from stats (td_ingest_moments' out layout).
__global__ __launch_bounds__(kThreads) void moments_chunk_kernel(const MomTrial* __restrict__ tab, int num, int width,
                                                                 int chunk_rows, int second,
                                                                 const double* __restrict__ stats,
                                                                 double* __restrict__ partial) {
  __shared__ double s1[kThreads];
  __shared__ double s2[kThreads];
  const int tid = threadIdx.x;
  const long long chunk = blockIdx.x;
  int lo = 0, hi = num - 1;
  while (lo < hi) {                                             // the last trial with chunk0 <= chunk
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
  }
  const MomTrial t = tab[lo];
  const long long rb = (chunk - t.chunk0) * chunk_rows;
  const long long re = rb + chunk_rows < t.rows ? rb + chunk_rows : t.rows;
  const double mean_all = second ? stats[0] : 0.0;
  const int pw = second ? 2 * width : width;
  for (int c0 = 0; c0 < width; c0 += kThreads) {
    const int wt = width - c0 < kThreads ? width - c0 : kThreads;
    const int slots = kThreads / wt;
    const int ro = tid / wt, col = c0 + tid - ro * wt;
    double a1 = 0.0, a2 = 0.0;
    if (ro < slots) {
      const double mean_col = second ? stats[2 + col] : 0.0;
      // (four rows in flight per thread with separate accumulators measured slower: 1.5 ms against 1.1 ms at
      // 40 trials x 1e5 x 64)
      for (long long row = rb + ro; row < re; row += slots) {
        const long long at = row * t.ld + col;
        const double x = t.is_f64 ? static_cast<const double*>(t.ptr)[at] : (double)static_cast<const float*>(t.ptr)[at];
        if (second) {
          const double d1 = x - mean_col, d2 = x - mean_all;
          a1 += d1 * d1;
          a2 += d2 * d2;
        } else {
          a1 += x;
        }
      }
    }
    __syncthreads();                                            // (the previous tile's totals were read)
    s1[tid] = a1;
    reduce_slots(s1, tid, wt, slots);
    if (second) {
      s2[tid] = a2;
      reduce_slots(s2, tid, wt, slots);
    }
    if (tid < wt) {
      partial[chunk * pw + c0 + tid] = s1[tid];
      if (second) partial[chunk * pw + width + c0 + tid] = s2[tid];
    }
  }
}

// One workgroup.  second == 0: out[2 + col] = mean of the column, out[0] = mean of everything.  second != 0:
// out[2 + width + col] = std of the column, out[1] = std of everything.  The chunks are summed in a fixed order.
__global__ __launch_bounds__(kThreads) void moments_finish_kernel(const double* __restrict__ partial, long long chunks,
                                                                  int width, int second, double rows_total,
                                                                  double* __restrict__ out, double* __restrict__ colsum) {
  __shared__ double s1[kThreads];
  const int tid = threadIdx.x;
  const int pw = second ? 2 * width : width;
  const int which = second ? 2 : 1;
  for (int w = 0; w < which; ++w) {
    for (int c0 = 0; c0 < width; c0 += kThreads) {
      const int wt = width - c0 < kThreads ? width - c0 : kThreads;
      const int slots = kThreads / wt;
      const int ro = tid / wt, col = c0 + tid - ro * wt;
      double a = 0.0;
      if (ro < slots)
        for (long long ch = ro; ch < chunks; ch += slots) a += partial[ch * pw + w * width + col];
      __syncthreads();
      s1[tid] = a;
      reduce_slots(s1, tid, wt, slots);
      if (tid < wt) {
        if (!second) { out[2 + c0 + tid] = s1[tid] / rows_total; colsum[c0 + tid] = s1[tid]; }
        else if (w == 0) out[2 + width + c0 + tid] = sqrt(s1[tid] / rows_total);
        else colsum[c0 + tid] = s1[tid];
      }
    }
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    double a = 0.0;
    for (int c = 0; c < width; ++c) a += colsum[c];
    const double count = rows_total * (double)width;
    if (!second) out[0] = a / count; else out[1] = sqrt(a / count);
  }
}

// ---------------------------------------------------------------- normalise
template <typename TIn, typename TSub, typename TOut>
__global__ __launch_bounds__(kThreads) void normalize_kernel(const TIn* __restrict__ a, long long lda, long long rows,
                                                             int width, const double* __restrict__ mean,
                                                             const double* __restrict__ sd, int per_column, int divide,
                                                             TOut* __restrict__ out, long long ldo) {
  const long long total = rows * width;
  const bool small = total < (1ll << 32);                       // (a 64-bit division is several times the work)
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const long long r = small ? (long long)((unsigned)i / (unsigned)width) : i / width;
    const int c = (int)(i - r * width);
    const int k = per_column ? c : 0;
    const TSub centred = (TSub)a[r * lda + c] - (TSub)mean[k];
    TOut v = (TOut)centred;
    if (divide) v = v / (TOut)sd[k];
    out[r * ldo + c] = v;
  }
}

template <typename TIn, typename TSub, typename TOut>
void launch_normalize(td_handle* h, const void* a, long long lda, long long rows, int width, const double* mean,
                      const double* sd, int per_column, int divide, void* out, long long ldo) {
  const long long total = rows * width;
  long long blocks = td_ceil_div(total, kThreads);
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL((normalize_kernel<TIn, TSub, TOut>), dim3((unsigned)blocks), dim3(kThreads), 0, h->stream,
                     static_cast<const TIn*>(a), lda, rows, width, mean, sd, per_column, divide,
                     static_cast<TOut*>(out), ldo);
}

}  // namespace

extern "C" {

int td_tfrecord_route(int stride, int* staged, int* group, int* lanes) {
  if (stride < 17 || !staged || !group || !lanes) return TD_ERR_INVALID;
  encode_route(stride, group, lanes);
  *staged = *group > 0 ? 1 : 0;
  return TD_OK;
}

int td_tfrecord_encode(td_handle* h, const uint8_t* template_host, int stride, int num_features,
                       const void* const* feature_dev, const int64_t* ld_host, const int* width_host,
                       const int* offset_host, const int* is_f64_host, const int* reversed_host, int64_t frames,
                       uint8_t* out_dev) {
  if (!h || !template_host || !feature_dev || !ld_host || !width_host || !offset_host || !is_f64_host ||
      !reversed_host || (!out_dev && frames > 0))
    return td_fail(h, TD_ERR_INVALID, "td_tfrecord_encode: NULL argument");
  TD_REQUIRE(h, stride >= 17 && stride <= (1 << 28) && frames >= 0, "td_tfrecord_encode: bad sizes");
  TD_REQUIRE(h, num_features >= 1 && num_features <= kMaxFeatures, "td_tfrecord_encode: 1 .. %d features, not %d",
             kMaxFeatures, num_features);
  TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(out_dev) & 15) == 0, "td_tfrecord_encode: the image must be 16-byte aligned");
  uint64_t length = 0;
  memcpy(&length, template_host, 8);
  TD_REQUIRE(h, length + 16 == (uint64_t)stride, "td_tfrecord_encode: the template's length field is not stride - 16");
  EncParams p;
  memset(&p, 0, sizeof(p));
  p.num = num_features;
  p.stride = stride;
  p.frames = frames;
  for (int f = 0; f < num_features; ++f) {
    TD_REQUIRE(h, feature_dev[f] && width_host[f] >= 1 && ld_host[f] >= width_host[f],
               "td_tfrecord_encode: feature %d: bad pointer, width or row stride", f);
    TD_REQUIRE(h, offset_host[f] >= 12 && (long long)offset_host[f] + 4ll * width_host[f] <= stride - 4,
               "td_tfrecord_encode: feature %d: payload [%d, +%lld) outside the record's data", f, offset_host[f],
               4ll * width_host[f]);
    p.f[f].ptr = feature_dev[f];
    p.f[f].ld = ld_host[f];
    p.f[f].width = width_host[f];
    p.f[f].offset = offset_host[f];
    p.f[f].is_f64 = is_f64_host[f] ? 1 : 0;
    p.f[f].reversed = reversed_host[f] ? 1 : 0;
  }
  if (frames == 0) return TD_OK;
  int group = 0, lanes = 0;
  encode_route(stride, &group, &lanes);
  const int piece = (stride - 16) / lanes;
  // one table: CRC byte table | advance table | the template as words, four times over | the template's bytes
  std::vector<uint32_t> tab(kTabWords + stride + (stride + 3) / 4, 0u);
  CrcTables& ct = crc_tables();
  memcpy(tab.data(), ct.byte_tab, sizeof(ct.byte_tab));
  memcpy(tab.data() + 256, ct.advance_by(piece).data(), 1024 * sizeof(uint32_t));
  uint8_t* t4 = reinterpret_cast<uint8_t*>(tab.data() + kTabWords);
  for (int k = 0; k < 5; ++k) memcpy(t4 + (size_t)k * stride, template_host, stride);
  const void* tab_dev = nullptr;
  TD_TRY(td_table_upload(h, tab.data(), tab.size() * sizeof(uint32_t), &tab_dev));
  const uint32_t* tabs = static_cast<const uint32_t*>(tab_dev);
  if (group > 0) {
    const size_t lds = 6144 + (size_t)group * stride;
    hipLaunchKernelGGL(encode_staged_kernel, dim3((unsigned)td_ceil_div(frames, group)), dim3(kThreads), lds, h->stream,
                       p, tabs, group, lanes, piece, out_dev);
  } else {
    TD_REQUIRE(h, frames <= 0x7fffffffll, "td_tfrecord_encode: too many records for the large route");
    hipLaunchKernelGGL(encode_large_kernel, dim3((unsigned)frames), dim3(kThreads), 0, h->stream, p, tabs, piece, out_dev);
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_tfrecord_decode(td_handle* h, const uint8_t* image_dev, int stride, int64_t frames,
                       const uint8_t* template_host, const uint8_t* mask_host, int num_outputs,
                       const int* offset_host, const int* count_host, void* const* dst_dev, const int64_t* ld_host,
                       const int* col_host, int64_t* status_dev) {
  if (!h || !template_host || !mask_host || !status_dev || (!image_dev && frames > 0) ||
      (num_outputs > 0 && (!offset_host || !count_host || !dst_dev || !ld_host || !col_host)))
    return td_fail(h, TD_ERR_INVALID, "td_tfrecord_decode: NULL argument");
  TD_REQUIRE(h, stride >= 17 && stride <= (1 << 28) && frames >= 0, "td_tfrecord_decode: bad sizes");
  TD_REQUIRE(h, num_outputs >= 0 && num_outputs <= kMaxFeatures, "td_tfrecord_decode: 0 .. %d outputs, not %d",
             kMaxFeatures, num_outputs);
  TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(image_dev) & 15) == 0, "td_tfrecord_decode: the image must be 16-byte aligned");
  TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(status_dev) & 7) == 0, "td_tfrecord_decode: the status must be 8-byte aligned");
  uint64_t length = 0;
  memcpy(&length, template_host, 8);
  TD_REQUIRE(h, length + 16 == (uint64_t)stride, "td_tfrecord_decode: the template's length field is not stride - 16");
  DecParams p;
  memset(&p, 0, sizeof(p));
  p.num = num_outputs;
  p.stride = stride;
  p.frames = frames;
  for (int f = 0; f < num_outputs; ++f) {
    TD_REQUIRE(h, count_host[f] >= 1 && offset_host[f] >= 12 && (long long)offset_host[f] + 4ll * count_host[f] <= stride - 4,
               "td_tfrecord_decode: output %d: payload [%d, +%lld) outside the record's data", f, offset_host[f],
               4ll * count_host[f]);
    TD_REQUIRE(h, col_host[f] >= 0 && ld_host[f] >= (long long)col_host[f] + count_host[f],
               "td_tfrecord_decode: output %d: row stride %lld below column %d + %d floats", f, (long long)ld_host[f],
               col_host[f], count_host[f]);
    TD_REQUIRE(h, dst_dev[f] || frames == 0, "td_tfrecord_decode: output %d: NULL destination", f);
    TD_REQUIRE(h, (reinterpret_cast<uintptr_t>(dst_dev[f]) & 3) == 0, "td_tfrecord_decode: output %d: misaligned destination", f);
    p.o[f].dst = static_cast<float*>(dst_dev[f]) + col_host[f];
    p.o[f].ld = ld_host[f];
    p.o[f].offset = offset_host[f];
    p.o[f].count = count_host[f];
  }
  int group = 0, lanes = 0;
  encode_route(stride, &group, &lanes);
  TD_REQUIRE(h, group > 0 || frames <= 0x7fffffffll, "td_tfrecord_decode: too many records for the large route");
  if (frames == 0) return TD_OK;
  const int piece = (stride - 16) / lanes;
  std::vector<uint32_t> tab;
  decode_table(template_host, mask_host, stride, piece, &tab);
  const void* tab_dev = nullptr;
  TD_TRY(td_table_upload(h, tab.data(), tab.size() * sizeof(uint32_t), &tab_dev));
  const uint32_t* tabs = static_cast<const uint32_t*>(tab_dev);
  unsigned long long* status = reinterpret_cast<unsigned long long*>(status_dev);
  TD_HIP(h, hipMemsetAsync(status, 0xff, sizeof(*status), h->stream));     // -1: all clear
  if (group > 0) {
    const size_t lds = kDecStageOffset + (size_t)group * stride;
    hipLaunchKernelGGL(decode_staged_kernel, dim3((unsigned)td_ceil_div(frames, group)), dim3(kThreads), lds, h->stream,
                       p, tabs, group, lanes, piece, image_dev, status);
  } else {
    hipLaunchKernelGGL(decode_large_kernel, dim3((unsigned)frames), dim3(kThreads), 0, h->stream, p, tabs, piece,
                       image_dev, status);
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_ingest_moments(td_handle* h, const void* const* data_dev, const int64_t* rows_host, const int64_t* ld_host,
                      const int* is_f64_host, int num, int width, double* out_dev) {
  if (!h || !data_dev || !rows_host || !ld_host || !is_f64_host || !out_dev)
    return td_fail(h, TD_ERR_INVALID, "td_ingest_moments: NULL argument");
  TD_REQUIRE(h, num >= 1 && width >= 1, "td_ingest_moments: bad sizes");
  // rows per chunk: ~512 steps of a workgroup's row slots
  const int slots = width < kThreads ? kThreads / width : 1;
  const int chunk_rows = 512 * slots;
  std::vector<MomTrial> tab(num);
  long long chunks = 0, rows_total = 0;
  for (int t = 0; t < num; ++t) {
    TD_REQUIRE(h, rows_host[t] >= 0 && (rows_host[t] == 0 || (data_dev[t] && ld_host[t] >= width)),
               "td_ingest_moments: array %d: bad pointer, rows or row stride", t);
    tab[t].ptr = data_dev[t];
    tab[t].rows = rows_host[t];
    tab[t].ld = ld_host[t];
    tab[t].chunk0 = chunks;
    tab[t].is_f64 = is_f64_host[t] ? 1 : 0;
    tab[t].pad = 0;
    chunks += td_ceil_div(rows_host[t], chunk_rows);
    rows_total += rows_host[t];
  }
  TD_REQUIRE(h, rows_total > 0 && chunks <= 0x7fffffffll, "td_ingest_moments: no rows (or too many)");
  const void* tab_dev = nullptr;
  TD_TRY(td_table_upload(h, tab.data(), tab.size() * sizeof(MomTrial), &tab_dev));
  void* scratch = nullptr;
  TD_TRY(td_scratch(h, ((size_t)chunks * 2 * width + width) * sizeof(double), &scratch));
  double* partial = static_cast<double*>(scratch);
  double* colsum = partial + (size_t)chunks * 2 * width;
  const MomTrial* trials = static_cast<const MomTrial*>(tab_dev);
  for (int second = 0; second < 2; ++second) {
    hipLaunchKernelGGL(moments_chunk_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, h->stream, trials, num, width,
                       chunk_rows, second, out_dev, partial);
    hipLaunchKernelGGL(moments_finish_kernel, dim3(1), dim3(kThreads), 0, h->stream, partial, chunks, width, second,
                       (double)rows_total, out_dev, colsum);
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_ingest_normalize(td_handle* h, const void* a_dev, int a_is_f64, int64_t lda, int64_t rows, int width,
                        const double* mean_host, const double* std_host, int per_column, int sub_f64, int out_f64,
                        int divide, void* out_dev, int64_t ldout) {
  if (!h || !mean_host || !std_host || (rows > 0 && (!a_dev || !out_dev)))
    return td_fail(h, TD_ERR_INVALID, "td_ingest_normalize: NULL argument");
  TD_REQUIRE(h, rows >= 0 && width >= 1 && lda >= width && ldout >= width, "td_ingest_normalize: bad sizes");
  TD_REQUIRE(h, (!a_is_f64 || sub_f64) && (!sub_f64 || out_f64),
             "td_ingest_normalize: the arithmetic may not be narrower than its operand");
  if (rows == 0) return TD_OK;
  const int n = per_column ? width : 1;
  std::vector<double> stat(2 * (size_t)n);
  memcpy(stat.data(), mean_host, n * sizeof(double));
  memcpy(stat.data() + n, std_host, n * sizeof(double));
  const void* stat_dev = nullptr;
  TD_TRY(td_table_upload(h, stat.data(), stat.size() * sizeof(double), &stat_dev));
  const double* mean = static_cast<const double*>(stat_dev);
  const double* sd = mean + n;
  if (a_is_f64)
    launch_normalize<double, double, double>(h, a_dev, lda, rows, width, mean, sd, per_column, divide, out_dev, ldout);
  else if (sub_f64)
    launch_normalize<float, double, double>(h, a_dev, lda, rows, width, mean, sd, per_column, divide, out_dev, ldout);
  else if (out_f64)
    launch_normalize<float, float, double>(h, a_dev, lda, rows, width, mean, sd, per_column, divide, out_dev, ldout);
  else
    launch_normalize<float, float, float>(h, a_dev, lda, rows, width, mean, sd, per_column, divide, out_dev, ldout);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

}  // extern "C"
