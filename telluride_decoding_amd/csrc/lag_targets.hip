// The regression-targets pass of the lagged covariance, [y]^T x~ per signed lag, with the column sums of x
// and y (split from lagcov.hip; td_common.h declares the entry points).
#include <cstdlib>
#include <cstring>

#include "lag_common.h"

namespace {

// ---- regression targets: [y]^T x~ per signed lag, lane = channel -----------------------
//   G[e - e_min][i][j] = sum_{u in [us, ue)} Y~[u][i] * X~[u + e][j]      (i < NI target columns)
// One WAVE streams the rows v = us + e_min .. of its strip of X (one coalesced 256-byte load
// per row: lane j gets x[v][j]) and keeps E running sums per target in registers: row v adds
// x[v][j] * y[v - e] to the sum of every lag e.  The y values are the same for all lanes: the
// strip's targets sit in a wave-private LDS line (broadcast reads) and move through a ring of
// E registers whose slot indices are compile-time constants in the unrolled body.  Rows of Y
// outside [us, ue) are zero, which handles every strip and file edge.  The kernel also
// returns the plain column sums of X over [us, ue) and of Y: the all-ones row of [y | 1]^T x~
// (the bias moments) follows from those and the per-file boundary windows (stats_accumulate.hip) instead
// of a second set of FMAs.  f32 FMA chains of at most kWaveStrip rows, summed in float64 by
// the reduction kernels.
// (The first version was an LDS-tiled workgroup kernel whose FMAs each read an operand from
// LDS: 233 us at C2 for 8 GFLOP.)
constexpr int kWaveStrip = 512;

template <int E, int NI>
__global__ __launch_bounds__(kThreads) void lagcov_wave_kernel(LagParams p, double* __restrict__ part64,
                                                              double* __restrict__ csum,
                                                              double* __restrict__ ysum) {
  // rows of load prefetch: a row is one 256-byte load, HBM latency ~2 us -- with 8 rows in
  // flight per wave the kernel was latency-bound at 0.85 TB/s
  constexpr int P = 32;
  constexpr int NY = NI > 0 ? NI : 1;
  constexpr int kRowsMax = ((kWaveStrip + 2 * E - 2) / E) * E;   // whole bodies
  __shared__ float ylds[kThreads / 64][kRowsMax * NY];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  long long id = blockIdx.x * (long long)(kThreads / 64) + wave;
  if (id >= (long long)p.n_work * p.n_cbt) return;
  const int cbt = (int)(id % p.n_cbt);
  const int wi = (int)(id / p.n_cbt);
  const LagWork w = p.works[wi];
  const int len = (int)(w.u_end - w.u_begin);
  const int n_body = (len + E - 1 + E - 1) / E;      // rows streamed: len + E - 1, whole bodies
  float* ya = ylds[wave];

  // targets of the strip, zero outside [u_begin, u_end) and beyond the stream
  if (NI > 0) {
    for (int t = lane; t < n_body * E; t += 64) {
      const long long u = w.u_begin + t;
      const bool ok = t < len && u >= 0 && u < w.a_valid;
#pragma unroll
      for (int i = 0; i < NI; ++i)
        ya[t * NY + i] = (ok && i < p.ca) ? p.a[(w.a_row0 + (ok ? u : 0)) * p.lda + (i < p.ca ? i : 0)] : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    if (cbt == 0 && ysum) {
      // column sums of Y over the strip (float64), lane-strided + shuffle tree
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        double sy = 0.0;
        for (int t = lane; t < len; t += 64) sy += (double)ya[t * NY + i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sy += __shfl_down(sy, off, 64);
        if (lane == 0) ysum[(size_t)wi * NI + i] = sy;
      }
    }
  }

  const int cg = cbt * 64 + lane;
  const bool ch_ok = cg < p.cb;
  const int voff = ch_ok ? cg : cbt * 64;
  const long long vs = w.u_begin + p.e_min;           // first streamed row
  // Loads are unconditional (row index clamped into the stream) and the row's validity is
  // applied as a 0/1 factor when the value is USED: a select on the loaded value makes hipcc
  // branch around the load and wait for it on the spot (vmcnt(0) after every load: no
  // prefetch at all, 0.8 TB/s).
  auto load_row = [&](long long v) -> float {
    long long vc = v < w.b_valid ? v : w.b_valid - 1;
    vc = vc < 0 ? 0 : vc;
    const float* rowp = p.b + (w.b_row0 + vc) * p.ldb;    // wave-uniform base
    return rowp[voff];
  };
  auto row_mask = [&](long long v) -> float { return (v >= 0 && v < w.b_valid) ? 1.f : 0.f; };
  // f32 FMA chains of one body (E rows), flushed into float64 sums after every body: the
  // targets correlate with x, so the running sums drift away from zero and a long f32 chain
  // loses ~1e-7 relative (which the ridge solve amplifies)
  float acc[E][NY], ring[E][NY];
  double acc64[E][NY];
#pragma unroll
  for (int k = 0; k < E; ++k)
#pragma unroll
    for (int i = 0; i < NY; ++i) { acc[k][i] = 0.f; ring[k][i] = 0.f; acc64[k][i] = 0.0; }
  double cs = 0.0;   // column sum of x over [u_begin, u_end): float64 (it feeds the bias moments)
  float xr[P];
#pragma unroll
  for (int k = 0; k < P; ++k) xr[k] = load_row(vs + k);
  const int t_lo = -p.e_min, t_hi = len - p.e_min;    // rows of [u_begin, u_end) in stream time

  for (int b = 0; b < n_body; ++b) {
    const int tb = b * E;
#pragma unroll
    for (int s = 0; s < E; ++s) {
      const float xv = xr[s % P] * row_mask(vs + tb + s);
      xr[s % P] = load_row(vs + tb + s + P);
      const int t = tb + s;
      cs += (t >= t_lo && t < t_hi) ? (double)xv : 0.0;
      if (NI > 0) {
#pragma unroll
        for (int i = 0; i < NI; ++i) ring[s][i] = ya[t * NY + i];
        // lag e_min + k pairs row v with the target k rows back: ring slot (s - k) mod E
#pragma unroll
        for (int k = 0; k < E; ++k)
#pragma unroll
          for (int i = 0; i < NI; ++i)
            acc[k][i] = fmaf(xv, ring[(s - k) & (E - 1)][i], acc[k][i]);
      }
    }
    if (NI > 0) {
#pragma unroll
      for (int k = 0; k < E; ++k)
#pragma unroll
        for (int i = 0; i < NI; ++i) { acc64[k][i] += (double)acc[k][i]; acc[k][i] = 0.f; }
    }
  }
  if (ch_ok || true) {
    if (NI > 0) {
      double* slab = part64 + (size_t)wi * p.e_pad * p.ca_pad * p.cb_pad;
#pragma unroll
      for (int k = 0; k < E; ++k)
        if (k < p.e_count) {
#pragma unroll
          for (int i = 0; i < NI; ++i)
            slab[((size_t)k * p.ca_pad + i) * p.cb_pad + cbt * 64 + lane] = acc64[k][i];
        }
    }
    csum[(size_t)wi * p.cb_pad + cbt * 64 + lane] = cs;
  }
}

// Column sums alone (no targets) of a NARROW stream, cb <= 32: lagcov_wave_kernel<32, 0> gives a lane to a channel
// and a load instruction to a row -- 4 useful bytes per instruction for one channel, 74 us for a 4 MB signal.
// Here a lane is (row of a group, channel): 64 / cbp rows per instruction (cbp = cb rounded up to a power of two),
// float64 sums, the rows of a group met by shuffles.  Same work items, same output slots.
__global__ __launch_bounds__(kThreads) void colsum_rows_kernel(LagParams p, double* __restrict__ csum, int cbp) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long wi = blockIdx.x * (long long)(kThreads / 64) + wave;
  if (wi >= p.n_work) return;
  const LagWork w = p.works[wi];
  const int per = 64 / cbp, c = lane % cbp, rs = lane / cbp;
  const bool ch_ok = c < p.cb;
  // the rows [u_begin, u_end) that exist
  const long long lo = w.u_begin > 0 ? w.u_begin : 0, hi = w.u_end < w.b_valid ? w.u_end : w.b_valid;
  const float* base = p.b + w.b_row0 * p.ldb + (ch_ok ? c : 0);
  double cs = 0.0;
  constexpr int kInFlight = 8;
  for (long long u0 = lo + rs; u0 < hi; u0 += (long long)per * kInFlight) {
    float v[kInFlight];
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) {
      const long long u = u0 + (long long)per * k;
      v[k] = u < hi ? base[u * p.ldb] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) cs += (double)v[k];
  }
  for (int off = cbp; off < 64; off <<= 1) cs += __shfl_xor(cs, off, 64);
  // (slot of channel c; the other lanes of the item's 64 slots hold zero)
  csum[(size_t)wi * p.cb_pad + lane] = (lane < cbp && ch_ok) ? cs : 0.0;
}

// The same moments on the matrix cores (one target column, at most 32 lags).  As a product,
// G[m][j] = sum_v A[m][v] B[v][j] with A[m][v] = y[v - e_min - m] (a Toeplitz matrix of the
// strip's targets, zero outside [u_begin, u_end)) and B[v][j] = x~[v][j]: M = lag, K = time,
// N = channel.  The B operand of v_mfma_f32_32x32x2_f32 wants lane (n = lane & 31, k = lane >> 5)
// to hold B[2 kk + k][n]: with n -> channels 2n (tile 0) and 2n + 1 (tile 1) that is ONE
// coalesced float2 load per lane straight from global memory -- two 256-byte rows per wave
// instruction, no LDS for x at all -- and the A operand is one broadcast-friendly LDS read of the
// staged targets.  The lane-per-channel kernel above spends 32 FMAs per row and lane (VALU-bound,
// 123 us at C2); here a row costs one MFMA per 32 channels and the kernel runs at the speed of
// its loads.  The sums drift (y correlates with x), so the MFMA accumulators are 32-row chains
// flushed into float64 sums (64 VGPRs).  The pipelined loop does only the bodies that need no
// masks and no address clamping (all but the first / last one or two of a strip); the others
// follow in a plain load-then-multiply tail.  (With both forms inside one unrolled loop the
// register allocation of the rare form cost the common one its float64 accumulators.)
constexpr int kTgtPrefetch = 16;     // steps (row pairs) of x in flight per wave
constexpr int kTgtBody = 16;         // steps per flush (= the prefetch ring: static slots)
constexpr int kTgtStrip = 4 * kWaveStrip;   // rows of one WORKGROUP's strip
constexpr int kTgtStripMin = 512;    // ... and the shortest the planner cuts (a short call: more, shorter strips)

// Geometry of a wave's share of a strip, the same in both kernels.
struct TgtStrip {
  const float* strip;   // first valid streamed row of x
  int len, n_body;      // targets in the strip; 32-row bodies of streamed rows
  int r_lo, r_hi;       // stream rows of the first / last valid row of x (clamped)
  long long last;       // stream row of the last valid row (may be < 0 or huge)
  int t_lo, t_hi;       // stream rows of [u_begin, u_end)
  int ldb32;
};

__device__ __forceinline__ TgtStrip tgt_strip(const LagParams& p, const LagWork& w) {
  constexpr int E = 32, kRowsBody = 2 * kTgtBody;
  TgtStrip t;
  t.len = (int)(w.u_end - w.u_begin);
  t.n_body = (t.len + E - 1 + kRowsBody - 1) / kRowsBody;
  const long long vs = w.u_begin + p.e_min;           // first streamed row
  const long long v_first = vs < 0 ? 0 : (vs < w.b_valid ? vs : (w.b_valid > 0 ? w.b_valid - 1 : 0));
  t.strip = p.b + (w.b_row0 + v_first) * p.ldb;
  t.r_lo = (int)(v_first - vs);
  t.last = w.b_valid - 1 - vs;
  t.r_hi = t.last < t.r_lo ? t.r_lo : (t.last > (1 << 20) ? (1 << 20) : (int)t.last);
  t.t_lo = -p.e_min;
  t.t_hi = t.len - p.e_min;
  t.ldb32 = (int)p.ldb;
  return t;
}

// Body b (rows [32 b, 32 b + 32)) and the body the wave prefetches under it (4 bodies on) lie
// wholly inside the file and inside [u_begin, u_end): no masks, no clamping.
__device__ __forceinline__ bool tgt_body_fast(const TgtStrip& t, int b) {
  const int first = b * 2 * kTgtBody, end = first + 2 * kTgtBody;
  return first >= t.r_lo && (long long)(end + 8 * kTgtBody - 1) <= t.last && first >= t.t_lo &&
         end <= t.t_hi;
}

// Targets of the strip behind kPad zeros (lag m pairs stream row r with target r - m), zero
// outside [u_begin, u_end) and beyond the stream.
__device__ __forceinline__ void tgt_stage_targets(const LagParams& p, const LagWork& w, int len,
                                                  int n_body, int kPad, float* ya, int tid) {
  for (int t = tid; t < kPad + n_body * 2 * kTgtBody; t += kThreads) {
    const int tt = t - kPad;
    const long long u = w.u_begin + tt;
    const bool ok = tt >= 0 && tt < len && u >= 0 && u < w.a_valid;
    ya[t] = ok ? p.a[(w.a_row0 + (ok ? u : 0)) * p.lda] : 0.f;
  }
}

// What both targets kernels end with: the channel maxima into the table, the four waves' float64
// sums into wave 0 (LDS, fixed order), the strip's slab and column sums stored.  e_lo: first lag
// of the window (0 without windows).
template <bool kHalf>
__device__ __forceinline__ void tgt_combine_store(const LagParams& p, double* __restrict__ part64,
                                                  double* csum, unsigned* maxtab,
                                                  double (&comb)[3][16][64], int slab_i, int e_lo, int c0,
                                                  bool ok0, bool ok1, double (&big0)[16],
                                                  double (&big1)[16], double cs0, double cs1, float mx0,
                                                  float mx1) {
  const int lane = threadIdx.x & 63, g = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the two row parities of a channel sit in lanes n and n + 32
  cs0 += __shfl_xor(cs0, 32, 64);
  cs1 += __shfl_xor(cs1, 32, 64);
  mx0 = fmaxf(mx0, __shfl_xor(mx0, 32, 64));
  mx1 = fmaxf(mx1, __shfl_xor(mx1, 32, 64));
  // (per WAVE here: four of them max into the row of their workgroup's shard)
  if (maxtab && g == 0) {
    unsigned* row = maxtab + (blockIdx.x % kChanShards) * 128;
    if (ok0 && mx0 > 0.f) atomicMax(row + c0, __float_as_uint(mx0));
    if (ok1 && mx1 > 0.f) atomicMax(row + c0 + 1, __float_as_uint(mx1));
  }
  // the four waves' sums -> wave 0 (fixed order), 16 registers at a time: big0, big1, column sums
#pragma unroll
  for (int round = 0; round < 3; ++round) {
    if (kHalf && round == 1) continue;
    __syncthreads();
    if (wave > 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        comb[wave - 1][r][lane] = round == 0 ? big0[r] : round == 1 ? big1[r] : (r == 0 ? cs0 : r == 1 ? cs1 : 0.0);
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const double others = comb[0][r][lane] + (comb[1][r][lane] + comb[2][r][lane]);
        if (round == 0) big0[r] += others;
        else if (round == 1) big1[r] += others;
        else if (r == 0) cs0 += others;
        else if (r == 1) cs1 += others;
      }
    }
  }
  if (wave != 0) return;
  // C/D map: col = lane & 31 (channel pair n), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (lag)
  double* slab = part64 + (size_t)slab_i * p.e_pad * p.ca_pad * p.cb_pad;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int k = e_lo + (r & 3) + 8 * (r >> 2) + 4 * g;
    if (k < p.e_count) {
      slab[(size_t)k * p.ca_pad * p.cb_pad + c0] = big0[r];
      if (!kHalf) slab[(size_t)k * p.ca_pad * p.cb_pad + c0 + 1] = big1[r];
    }
  }
  if (g == 0 && csum) {
    csum[(size_t)slab_i * p.cb_pad + c0] = cs0;
    if (!kHalf) csum[(size_t)slab_i * p.cb_pad + c0 + 1] = cs1;
  }
}

// The four waves of a workgroup share one strip of up to kTgtStrip rows and take its 32-row
// bodies in turn (wave w: bodies w, w + 4, ...); every wave owns a private slab (index
// 4 * strip + wave), so nothing is combined across waves here.
//
// The kernel streams every row of x the accumulate touches (the rows past a range's end too), so
// it also measures the largest magnitude of every channel for the float16 lag kernel that runs
// next (maxtab: atomic max of float bits, td_f16_scale_exp) -- the pre-pass that kernel needs
// costs nothing here.  The four waves' sums meet in LDS (fixed order): one slab per strip.
// kHalf (<= 32 channels): a lane holds ONE channel and the second matrix instruction of a step, its
// accumulators and its float64 sums are not there (half the matrix work of the 64-channel form).
template <bool kVec2, bool kHalf = false>
__global__ __launch_bounds__(kThreads) void lagcov_targets_mfma_kernel(LagParams p,
                                                                       double* __restrict__ part64,
                                                                       double* csum, double* ysum,
                                                                       unsigned* maxtab) {
  constexpr int E = 32, P = kTgtPrefetch, kPad = 32, kRowsBody = 2 * kTgtBody;
  constexpr int kBodiesMax = (kTgtStrip + E - 1 + kRowsBody - 1) / kRowsBody;
  __shared__ float ya[kPad + kBodiesMax * kRowsBody];
  __shared__ double comb[3][16][64];                   // waves 1-3 -> wave 0, 16 registers at a time
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // Work item = (strip, 64-channel tile); td_lagcov_column adds windows of 32 lags (p.n_groups of
  // them: lags e_min + 32 win ..; otherwise one).  The windows of an item read the same rows of x:
  // they are dealt to ONE XCD, next to each other in dispatch order (workgroup g runs on XCD g % 8),
  // so that the second and third read hit its L2 -- with the windows in blockIdx.y a strip's
  // windows ran a whole grid apart and x came from HBM once per window.
  // A strip's slab holds all its windows; the column sums are window 0's business.
  const int n_win = p.n_groups;
  const int slot = (int)(blockIdx.x >> 3);
  const int item = (slot / n_win) * 8 + (int)(blockIdx.x & 7);
  if (item >= p.n_work * p.n_cbt) return;              // (the grid is padded to whole XCD rounds)
  const int cbt = item % p.n_cbt;
  const int wi = item / p.n_cbt;                       // strip = slab
  const LagWork w = p.works[wi];
  const int e_lo = 32 * (slot % n_win);
  p.e_min += e_lo;
  if (e_lo) { csum = nullptr; ysum = nullptr; maxtab = nullptr; }
  const TgtStrip ts = tgt_strip(p, w);
  const int slab_i = wi;
  tgt_stage_targets(p, w, ts.len, ts.n_body, kPad, ya, tid);
  __syncthreads();
  if (cbt == 0 && ysum && wave == 0) {
    // the strip's column sum of y
    double sy = 0.0;
    for (int t = lane; t < ts.len; t += 64) sy += (double)ya[kPad + t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sy += __shfl_down(sy, off, 64);
    if (lane == 0) ysum[slab_i] = sy;
  }

  const int n = lane & 31, g = lane >> 5;
  const int c0 = kHalf ? cbt * 64 + n : cbt * 64 + 2 * n;   // this lane's channels: c0 (tile 0), c0 + 1
  const bool ok0 = c0 < p.cb, ok1 = !kHalf && c0 + 1 < p.cb;
  const int off0 = ok0 ? c0 : 0, off1 = ok1 ? c0 + 1 : off0;
  // this wave's fast bodies: b0, b0 + 4, ... (fast bodies are a contiguous run of the strip)
  int b0 = wave, nb = 0;
  while (b0 < ts.n_body && !tgt_body_fast(ts, b0)) b0 += 4;
  for (int b = b0; b < ts.n_body && tgt_body_fast(ts, b); b += 4) ++nb;

  f32x16 acc0, acc1;
  double big0[16], big1[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; big0[r] = 0.0; big1[r] = 0.0; }
  double cs0 = 0.0, cs1 = 0.0;        // column sums of x over [u_begin, u_end)
  float mx0 = 0.f, mx1 = 0.f;         // largest magnitudes of the two channels (every row streamed)
  const float* yp = ya + kPad + g - n;                // A operand of step kk: yp[2 kk]
  if (nb > 0) {
    float xr[P][2];
    auto load_step = [&](const float* bp, int s, float& x0, float& x1) {
      if (kHalf) {
        x0 = bp[s * 2 * ts.ldb32]; x1 = 0.f;
      } else if (kVec2) {
        const float2 v = *reinterpret_cast<const float2*>(bp + s * 2 * ts.ldb32);
        x0 = v.x; x1 = v.y;
      } else {
        x0 = bp[s * 2 * ts.ldb32]; x1 = bp[s * 2 * ts.ldb32 + off1 - off0];
      }
    };
    {
      const float* bp = ts.strip + (b0 * kRowsBody + g - ts.r_lo) * ts.ldb32 + off0;
#pragma unroll
      for (int k = 0; k < P; ++k) load_step(bp, k, xr[k][0], xr[k][1]);
    }
    for (int it = 0; it < nb; ++it) {
      const int b = b0 + 4 * it;
      // the wave's next body (always readable: tgt_body_fast covers it)
      const float* bp = ts.strip + ((b + 4) * kRowsBody + g - ts.r_lo) * ts.ldb32 + off0;
      float c0s = 0.f, c1s = 0.f;
#pragma unroll
      for (int s = 0; s < kTgtBody; ++s) {
        const float x0 = xr[s % P][0], x1 = xr[s % P][1];
        c0s += x0; c1s += x1;
        mx0 = fmaxf(mx0, fabsf(x0)); mx1 = fmaxf(mx1, fabsf(x1));
        const float a = yp[(b * kTgtBody + s) * 2];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x0, acc0, 0, 0, 0);
        if (!kHalf) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x1, acc1, 0, 0, 0);
        // the slot is free once the MFMAs have read it: refill it for the wave's next body
        load_step(bp, s, xr[s % P][0], xr[s % P][1]);
      }
      cs0 += (double)c0s;
      cs1 += (double)c1s;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        big0[r] += (double)acc0[r]; acc0[r] = 0.f;
        if (!kHalf) { big1[r] += (double)acc1[r]; acc1[r] = 0.f; }
      }
    }
  }
  // The bodies left out above (first / last of a strip: rows outside the file or outside
  // [u_begin, u_end), or a prefetch that would run past the file): clamped loads, 0/1 masks,
  // all loads of a body first and then its MFMAs -- a few percent of the rows.
  for (int b = wave; b < ts.n_body; b += 4) {
    if (tgt_body_fast(ts, b)) continue;
    float c0s = 0.f, c1s = 0.f;
    float xe[kTgtBody][2];
#pragma unroll
    for (int s = 0; s < kTgtBody; ++s) {
      const int r = (b * kTgtBody + s) * 2 + g;
      const int rc = min(max(r, ts.r_lo), ts.r_hi) - ts.r_lo;
      const float* rowp = ts.strip + rc * ts.ldb32;
      if (kHalf) {
        xe[s][0] = rowp[off0]; xe[s][1] = 0.f;
      } else if (kVec2) {
        const float2 v = *reinterpret_cast<const float2*>(rowp + off0);
        xe[s][0] = v.x; xe[s][1] = v.y;
      } else {
        xe[s][0] = rowp[off0]; xe[s][1] = rowp[off1];
      }
    }
#pragma unroll
    for (int s = 0; s < kTgtBody; ++s) {
      const int r = (b * kTgtBody + s) * 2 + g;
      const float m = (r >= ts.r_lo && (long long)r <= ts.last) ? 1.f : 0.f;
      const float x0 = xe[s][0] * m, x1 = xe[s][1] * m;
      mx0 = fmaxf(mx0, fabsf(x0)); mx1 = fmaxf(mx1, fabsf(x1));
      const float in = (r >= ts.t_lo && r < ts.t_hi) ? 1.f : 0.f;
      c0s = fmaf(in, x0, c0s); c1s = fmaf(in, x1, c1s);
      const float a = yp[(b * kTgtBody + s) * 2];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x0, acc0, 0, 0, 0);
      if (!kHalf) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x1, acc1, 0, 0, 0);
    }
    cs0 += (double)c0s;
    cs1 += (double)c1s;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      big0[r] += (double)acc0[r]; acc0[r] = 0.f;
      if (!kHalf) { big1[r] += (double)acc1[r]; acc1[r] = 0.f; }
    }
  }
  tgt_combine_store<kHalf>(p, part64, csum, maxtab, comb, slab_i, e_lo, c0, ok0, ok1, big0, big1, cs0, cs1,
                           mx0, mx1);
}

// The 64-channel form on the float16 matrix pipe.  The float32 instruction of the kernel above takes
// 128 matrix cycles for a pair of rows (two v_mfma_f32_32x32x2_f32): a CU cannot stream more than 16
// bytes a cycle through it, and with the float64 flush it ran at 0.42 of that.  Here a body (32 rows
// x 64 channels) is 12 v_mfma_f32_32x32x16_f16 (384 cycles against 2048): x and y as two float16
// pieces each, three products (l h', h l', h h'; td_split2_f16).
//
// Scales.  The B operand gives a lane 8 rows of ONE channel and the result gives it the 16 lags of
// that same channel, so the scale of x is private to the lane: a power of two per (body, channel)
// that puts the body's largest magnitude into [2^14, 2^15), taken from the lane's 16 values and its
// partner's (lane ^ 32).  No maximum over the whole stream is needed -- which is why this kernel can
// measure the channel maxima and use the float16 pipe in the same pass.  y: one power of two per
// strip, found while the strip is staged.  Both are divided out exactly when a body's 32-row chain
// is added to the float64 sums.  A body whose channel holds a NaN or an infinity (or a strip whose
// targets do) takes the factor NaN: the pieces are clamped and would lose it.
//
// Rows.  K index 8 g + i of k-step ks is stream row 32 b + 2 (8 ks + i) + g (g = lane >> 5): any
// pairing of K with rows is right as long as A uses the same one, and this one makes a lane's 16
// loads of a body the loads of the float32 kernel -- two whole 256-byte rows per wave instruction,
// the same float32 partial column sums in the same order (csum, ysum and maxtab are bit-identical
// to that kernel's).  The A operand is then 8 targets at stride 2 from y[row - lag]: the staged
// pieces are kept de-interleaved by parity and, for each parity, at the two half-word alignments, so
// that every lane reads its 8 float16 as four aligned words from an image that is fixed per lane.
constexpr int kTgtBodiesMax = (kTgtStrip + 31 + 31) / 32;
constexpr int kTgtImage = (32 + kTgtBodiesMax * 32) / 2 + 8;     // float16 per image of the targets

// k with max 2^k in [2^14, 2^15); 0 for nothing seen and for a NaN / infinity.  (td_f16_scale_exp
// stops at 2^126 because its scale is a float factor; this one is applied by v_ldexp_f32 and follows
// a denormal maximum all the way.)
__device__ __forceinline__ int tgt_scale_exp(unsigned max_bits) {
  if (max_bits == 0 || td_chan_not_finite(max_bits)) return 0;
  return 15 - __builtin_amdgcn_frexp_expf(__uint_as_float(max_bits));
}

// td_split2_f16 without its clamp (the body's own scale keeps every finite value below 2^15; what
// is not finite poisons the body through its factor) and with the residual as ONE mixed-precision
// fma per value (v_fma_mix_f32 reads the float16 piece in place).
__device__ __forceinline__ void tgt_split2(float x0, float x1, unsigned& h, unsigned& l) {
  h = td_pack_f16(x0, x1);
  const td_f16x2 hv = __builtin_bit_cast(td_f16x2, h);
  l = td_pack_f16(__builtin_fmaf((float)hv[0], -1.f, x0), __builtin_fmaf((float)hv[1], -1.f, x1));
}

// One body: x[s][t] = row 2 s + g of channel tile t (masked already), mb0 / mb1 = the float bits of
// the largest magnitude among this lane's 16 values of either tile.  refill(s) is called when step
// s's registers are free (the fast loop loads the wave's next body into them).
template <class Refill>
__device__ __forceinline__ void tgt_split_body(float (&x)[kTgtBody][2], unsigned mb0, unsigned mb1,
                                               const unsigned* ah, const unsigned* al, int ky, bool y_bad,
                                               double (&big0)[16], double (&big1)[16], Refill refill) {
  mb0 = max(mb0, (unsigned)__shfl_xor((int)mb0, 32, 64));
  mb1 = max(mb1, (unsigned)__shfl_xor((int)mb1, 32, 64));
  const int k0 = tgt_scale_exp(mb0), k1 = tgt_scale_exp(mb1);
  td_u32x4 h0[2], l0[2], h1[2], l1[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = 8 * ks + 2 * j;
      unsigned h, l;
      tgt_split2(ldexpf(x[s][0], k0), ldexpf(x[s + 1][0], k0), h, l);
      h0[ks][j] = h; l0[ks][j] = l;
      tgt_split2(ldexpf(x[s][1], k1), ldexpf(x[s + 1][1], k1), h, l);
      h1[ks][j] = h; l1[ks][j] = l;
      refill(s);
      refill(s + 1);
    }
  __builtin_amdgcn_sched_barrier(0);    // (the refills stay above the matrix instructions and the flush)
  td_f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const td_u32x4 yh = {ah[4 * ks], ah[4 * ks + 1], ah[4 * ks + 2], ah[4 * ks + 3]};
    const td_u32x4 yl = {al[4 * ks], al[4 * ks + 1], al[4 * ks + 2], al[4 * ks + 3]};
    acc0 = td_mfma_f16(yl, h0[ks], acc0);
    acc1 = td_mfma_f16(yl, h1[ks], acc1);
    acc0 = td_mfma_f16(yh, l0[ks], acc0);
    acc1 = td_mfma_f16(yh, l1[ks], acc1);
    acc0 = td_mfma_f16(yh, h0[ks], acc0);
    acc1 = td_mfma_f16(yh, h1[ks], acc1);
  }
  // 2^-(k_x + k_y) as a float64 (|k_x + k_y| <= 328), or NaN
  const double nan = __hiloint2double(0x7ff80000, 0);
  const double f0 = (y_bad || td_chan_not_finite(mb0)) ? nan : __hiloint2double((1023 - k0 - ky) << 20, 0);
  const double f1 = (y_bad || td_chan_not_finite(mb1)) ? nan : __hiloint2double((1023 - k1 - ky) << 20, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    big0[r] = fma((double)acc0[r], f0, big0[r]);
    big1[r] = fma((double)acc1[r], f1, big1[r]);
  }
}

__global__ __launch_bounds__(kThreads, 2) void lagcov_targets_split_kernel(LagParams p,
                                                                           double* __restrict__ part64,
                                                                           double* csum, double* ysum,
                                                                           unsigned* maxtab) {
  constexpr int kPad = 32, kRowsBody = 2 * kTgtBody;
  __shared__ float ya[kPad + kTgtBodiesMax * kRowsBody];
  __shared__ __attribute__((aligned(16))) _Float16 yimg[2][2][2][kTgtImage];   // [piece h, l][parity of the target][alignment]
  __shared__ double comb[3][16][64];
  __shared__ unsigned ymax_w[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // work item = (strip, 64-channel tile), one window of lags
  const int item = (int)blockIdx.x;
  if (item >= p.n_work * p.n_cbt) return;              // (the grid is padded to whole XCD rounds)
  const int cbt = item % p.n_cbt;
  const int wi = item / p.n_cbt;                       // strip = slab
  const LagWork w = p.works[wi];
  const TgtStrip ts = tgt_strip(p, w);
  const int n = lane & 31, g = lane >> 5;
  const int c0 = cbt * 64 + 2 * n;                     // this lane's channels: c0 (tile 0), c0 + 1
  const bool ok0 = c0 < p.cb, ok1 = c0 + 1 < p.cb;
  const int off0 = ok0 ? c0 : 0;
  // A operand of (body b, k-step ks): targets y[32 b + 16 ks + 2 i + g - n], i < 8 = D[q][j + i] with
  // kPad + 32 b + 16 ks + g - n = 2 j + q: words 8 b + 4 ks + 8 + ((g - n) >> 2) .. + 3 of the image
  // (q, j & 1) -- the image and the offset are the lane's own
  const int dg = g - n;
  const unsigned* ah = reinterpret_cast<const unsigned*>(&yimg[0][dg & 1][(dg >> 1) & 1][0]) + 8 + (dg >> 2);
  const unsigned* al = reinterpret_cast<const unsigned*>(&yimg[1][dg & 1][(dg >> 1) & 1][0]) + 8 + (dg >> 2);
  // this wave's fast bodies: b0, b0 + 4, ... (fast bodies are a contiguous run of the strip)
  int b0 = wave, nb = 0;
  while (b0 < ts.n_body && !tgt_body_fast(ts, b0)) b0 += 4;
  for (int b = b0; b < ts.n_body && tgt_body_fast(ts, b); b += 4) ++nb;

  // x through a buffer descriptor: one per-lane offset and a scalar one per load (no 64-bit address
  // arithmetic in the loop), and a load the compiler does not merge with the prologue's -- given
  // plain pointers it turns "loaded at the end of a pass, used at the start of the next" into ONE
  // load at the top of the loop, waited for on the spot: nothing in flight under the arithmetic.
  // (The float32 kernel's ring gets the same treatment; its refills fly for a third of a pass.)
  const long long rows_here = ts.last - ts.r_lo + 1;   // valid rows from ts.strip on
  const long long rows_need = (long long)ts.n_body * kRowsBody;   // (fast bodies lie below n_body)
  const unsigned buf_bytes =      // (no fast body: an empty descriptor, nothing is loaded)
      nb > 0 ? (unsigned)(((rows_here < rows_need ? rows_here : rows_need) - 1) * ts.ldb32 + p.cb) * 4u : 0u;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ts.strip), 0, buf_bytes, 0x00020000);
  const unsigned voff = (unsigned)(g * ts.ldb32 + off0) * 4u;
  // Two register images of a body, used in turn: while one is multiplied the other (the wave's next
  // body) is on its way, and the first is refilled -- with the wave's next body but one -- as soon
  // as its values are split.  A wave keeps 8 .. 16 KB in flight all the time; with one image the
  // loads flew only under the matrix instructions and the flush, and the launch took the same time
  // on 192 and on 256 CUs.  (A refill past the wave's last fast body loads that body again: every
  // address stays inside the strip, the descriptor's range check is never what keeps a load in.)
  float xa[kTgtBody][2], xb[kTgtBody][2];
  auto load_step = [&](float (&xr)[kTgtBody][2], unsigned body_off, int s) {
    const td_f32x2 v = __builtin_bit_cast(
        td_f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, body_off + (unsigned)(s * 2 * ts.ldb32) * 4u, 0));
    xr[s][0] = v[0]; xr[s][1] = v[1];
  };
  const int b_last = b0 + 4 * (nb - 1);
  auto body_off = [&](int b) { return (unsigned)(((b < b_last ? b : b_last) * kRowsBody - ts.r_lo) * ts.ldb32) * 4u; };
  // the first two bodies start their way here, under the staging of the targets
  if (nb > 0) {
    const unsigned bo0 = body_off(b0), bo1 = body_off(b0 + 4);
#pragma unroll
    for (int s = 0; s < kTgtBody; ++s) load_step(xa, bo0, s);
#pragma unroll
    for (int s = 0; s < kTgtBody; ++s) load_step(xb, bo1, s);
  }
  const int n_y = kPad + ts.n_body * kRowsBody;
  tgt_stage_targets(p, w, ts.len, ts.n_body, kPad, ya, tid);
  __syncthreads();
  {
    unsigned ym = 0u;
    for (int t = tid; t < n_y; t += kThreads) ym = max(ym, __float_as_uint(ya[t]) & 0x7fffffffu);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ym = max(ym, (unsigned)__shfl_xor((int)ym, off, 64));
    if (lane == 0) ymax_w[wave] = ym;
  }
  if (cbt == 0 && ysum && wave == 0) {
    // the strip's column sum of y
    double sy = 0.0;
    for (int t = lane; t < ts.len; t += 64) sy += (double)ya[kPad + t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sy += __shfl_down(sy, off, 64);
    if (lane == 0) ysum[wi] = sy;
  }
  __syncthreads();
  const unsigned ymax = max(max(ymax_w[0], ymax_w[1]), max(ymax_w[2], ymax_w[3]));
  const bool y_bad = td_chan_not_finite(ymax);
  const int ky = tgt_scale_exp(ymax);
  // images: D[q][t] = y[2 t + q]; alignment 0 holds D[q][t] at t, alignment 1 holds D[q][t + 1]
  for (int t = tid; t < n_y / 2; t += kThreads) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float v = ldexpf(ya[2 * t + q], ky);
      const _Float16 hv = (_Float16)v;
      const _Float16 lv = (_Float16)(v - (float)hv);
      yimg[0][q][0][t] = hv;
      yimg[1][q][0][t] = lv;
      if (t > 0) { yimg[0][q][1][t - 1] = hv; yimg[1][q][1][t - 1] = lv; }
    }
  }
  __syncthreads();

  double big0[16], big1[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { big0[r] = 0.0; big1[r] = 0.0; }
  double cs0 = 0.0, cs1 = 0.0;        // column sums of x over [u_begin, u_end)
  float mx0 = 0.f, mx1 = 0.f;         // largest magnitudes of the two channels (every row streamed)
  if (nb > 0) {
    // body b from image xr, which then receives body b + 8
    auto pass = [&](float (&xr)[kTgtBody][2], int b) {
      const unsigned bo = body_off(b + 8);
      float c0s = 0.f, c1s = 0.f, m0 = 0.f, m1 = 0.f;
#pragma unroll
      for (int s = 0; s < kTgtBody; ++s) {
        c0s += xr[s][0]; c1s += xr[s][1];
        m0 = fmaxf(m0, fabsf(xr[s][0])); m1 = fmaxf(m1, fabsf(xr[s][1]));
      }
      cs0 += (double)c0s;
      cs1 += (double)c1s;
      mx0 = fmaxf(mx0, m0); mx1 = fmaxf(mx1, m1);
      // fmaxf passes over a NaN, the sum does not: a finite sum of the lane's 16 values says that all of
      // them were finite.  (A sum of finite values that overflows poisons the body too -- the channel's
      // column sum is then infinite in either kernel.  No branch here: with one in the loop the
      // compiler sinks the refills below it, next to their use, and nothing is prefetched.)
      const unsigned mb0 = fabsf(c0s) <= 3.402823466e38f ? __float_as_uint(m0) : 0x7fc00000u;
      const unsigned mb1 = fabsf(c1s) <= 3.402823466e38f ? __float_as_uint(m1) : 0x7fc00000u;
      tgt_split_body(xr, mb0, mb1, ah + 8 * b, al + 8 * b, ky, y_bad, big0, big1,
                     [&](int s) { load_step(xr, bo, s); });
    };
    // (whole pairs in the loop, an odd body behind it: with "if (it + 1 < nb)" around the second pass
    // the compiler's wait for the first image also waits for the refills of the second)
    for (int it = 0; it + 1 < nb; it += 2) {
      pass(xa, b0 + 4 * it);
      pass(xb, b0 + 4 * it + 4);
    }
    if (nb & 1) pass(xa, b0 + 4 * (nb - 1));
  }
  // The bodies left out above (first / last of a strip: rows outside the file or outside
  // [u_begin, u_end), or a prefetch that would run past the file): clamped loads, the rows that do
  // not exist set to zero, the same arithmetic.
  for (int b = wave; b < ts.n_body; b += 4) {
    if (tgt_body_fast(ts, b)) continue;
    float xe[kTgtBody][2];
#pragma unroll
    for (int s = 0; s < kTgtBody; ++s) {
      const int r = (b * kTgtBody + s) * 2 + g;
      const int rc = min(max(r, ts.r_lo), ts.r_hi) - ts.r_lo;
      const float2 v = *reinterpret_cast<const float2*>(ts.strip + rc * ts.ldb32 + off0);
      xe[s][0] = v.x; xe[s][1] = v.y;
    }
    float c0s = 0.f, c1s = 0.f;
    unsigned mb0 = 0u, mb1 = 0u;
#pragma unroll
    for (int s = 0; s < kTgtBody; ++s) {
      const int r = (b * kTgtBody + s) * 2 + g;
      const bool there = r >= ts.r_lo && (long long)r <= ts.last;
      xe[s][0] = there ? xe[s][0] : 0.f;
      xe[s][1] = there ? xe[s][1] : 0.f;
      mx0 = fmaxf(mx0, fabsf(xe[s][0])); mx1 = fmaxf(mx1, fabsf(xe[s][1]));
      mb0 = max(mb0, __float_as_uint(xe[s][0]) & 0x7fffffffu);
      mb1 = max(mb1, __float_as_uint(xe[s][1]) & 0x7fffffffu);
      const float in = (r >= ts.t_lo && r < ts.t_hi) ? 1.f : 0.f;
      c0s = fmaf(in, xe[s][0], c0s); c1s = fmaf(in, xe[s][1], c1s);
    }
    cs0 += (double)c0s;
    cs1 += (double)c1s;
    tgt_split_body(xe, mb0, mb1, ah + 8 * b, al + 8 * b, ky, y_bad, big0, big1, [](int) {});
  }
  tgt_combine_store<false>(p, part64, csum, maxtab, comb, wi, 0, c0, ok0, ok1, big0, big1, cs0, cs1, mx0, mx1);
}

// per-file float64 column sums from the per-strip float32 ones: out[f][j] (+)= sum over the
// strips of file f
// (one workgroup of 1024 threads per file and 64-channel tile: 16 strip-strided partial sums
// per channel, combined in a fixed order)
__global__ __launch_bounds__(1024) void colsum_file_reduce_kernel(
    const double* __restrict__ csum, int cb_pad, int cb, const int* __restrict__ file_work0,
    double* __restrict__ out) {
  __shared__ double part[16][64];
  const int f = blockIdx.x, j = blockIdx.y * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  double s0 = 0.0, s1 = 0.0;
  if (j < cb) {
    int wk = file_work0[f] + q;
    const int end = file_work0[f + 1];
    for (; wk + 16 < end; wk += 32) {
      s0 += csum[(size_t)wk * cb_pad + j];
      s1 += csum[(size_t)(wk + 16) * cb_pad + j];
    }
    if (wk < end) s0 += csum[(size_t)wk * cb_pad + j];
  }
  part[q][threadIdx.x & 63] = s0 + s1;
  __syncthreads();
  if (q == 0 && j < cb) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += part[k][threadIdx.x];
    out[(size_t)f * cb + j] = t;
  }
}

// sy[i] (+)= sum over strips; one workgroup per target column
__global__ __launch_bounds__(256) void ysum_reduce_kernel(const double* __restrict__ ysum, int n_work,
                                                          int ni, double* __restrict__ sy,
                                                          int accumulate) {
  __shared__ double red[256];
  const int i = blockIdx.x;
  double s = 0.0;
  for (int wk = threadIdx.x; wk < n_work; wk += 256) s += ysum[(size_t)wk * ni + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) sy[i] = accumulate ? sy[i] + red[0] : red[0];
}

}  // namespace

// Targets path (see lagcov_wave_kernel).  g_dev is [e_count][d + 1][cb]: rows i < d receive
// y_i^T x~ (accumulated), row d (the all-ones row) is left to the caller, who gets the
// per-segment column sums of B over [u_begin, u_end) in colsum_seg_dev [n_segs][cb]
// (overwritten) and, if sy_dev, the accumulated column sums of Y.  Returns TD_ERR_STATE-free
// false in *handled when the shape needs the generic kernel (targets with more than 32 lags,
// more than 4 targets, column sums alone with more than 31 past lags).
int td_lagcov_targets_plan(td_handle* h, const float* y, int64_t ldy, int d, const float* b,
                           int64_t ldb, int cb, const std::vector<LagSeg>& segs, int e_min,
                           int e_count, TargetsPlan* plan, bool any_lag_window) {
  plan->handled = false;
  plan->scratch_bytes = 0;
  plan->works.clear();
  plan->seg_work0.clear();
  if (any_lag_window) {
    // td_lagcov_column: a window of lags that need not contain lag 0.  The products are right for
    // any window (targets are zero outside their rows, the stream is masked by its own validity);
    // the column sums the kernel leaves are not (they assume the rows [u_begin, u_end) lie inside
    // what a strip streams) and the caller must not use them.
    if (d != 1 || e_count > 32 * 8) return TD_OK;
  } else {
    if (d > 4 || e_min > 0 || e_min + e_count - 1 < 0) return TD_OK;
    // with targets at most 32 lags; without (column sums only: the lag count plays no part) the
    // wave kernel streams a strip from row u_begin + e_min on and covers it when e_min >= -31
    // (more lags with targets: windows of 32, the kernel's p.n_groups -- window 0, which holds lag 0
    // and starts at most 31 lags back, leaves the column sums)
    if (d > 0 ? (e_count > 32 * 8 || (e_count > 32 && e_min < -31)) : -e_min > 31) return TD_OK;
  }
  plan->handled = true;
  plan->lag_window = any_lag_window;
  const int n_segs = (int)segs.size();
  plan->d = d; plan->cb = cb; plan->e_count = e_count; plan->n_segs = n_segs;
  // Strips.  Without targets (column sums only: lagcov_wave_kernel) a strip is kWaveStrip rows
  // and one wave; with targets (lagcov_targets_mfma_kernel) a strip is kTgtStrip rows and one
  // WORKGROUP whose four waves each fill their own slab.  Every segment gets at least one
  // (possibly empty) strip so that the per-segment column sums are defined.  seg_work0 counts
  // slabs.
  const int ni = d > 0 ? 1 : 0;     // one target column per launch
  const int slabs_per_strip = 1;
  // strips of the targets kernel: <= kTgtStrip rows, shorter when the call is short, so that
  // there are ~4 workgroups per CU (a rank's 1/8 share of the C2 job ran on 61 workgroups)
  long long total = 0;
  for (const LagSeg& sg : segs) total += sg.u_end > sg.u_begin ? sg.u_end - sg.u_begin : 0;
  const int cus = h->cu_count > 0 ? h->cu_count : 256;
  long long t_strip = td_round_up(td_ceil_div(total > 0 ? total : 1, 4 * cus), 32);
  t_strip = t_strip < kTgtStripMin ? kTgtStripMin : (t_strip > kTgtStrip ? kTgtStrip : t_strip);
  // ... and really no more than 4 per CU: every recording ends in a short strip of its own, which put the C2
  // call on 192 CUs at 770 workgroups for 768 places -- the float16 kernel, two workgroups on a CU at a time,
  // ran a third round for the last two
  const long long n_tiles = td_ceil_div(cb, 64);
  auto strips_at = [&](long long t) {
    long long k = 0;
    for (const LagSeg& sg : segs) k += sg.u_end > sg.u_begin ? td_ceil_div(sg.u_end - sg.u_begin, t) : 1;
    return k;
  };
  while (t_strip < kTgtStrip && strips_at(t_strip) * n_tiles > 4LL * cus) t_strip += 32;
  // strips of the column-sum kernel (one WAVE each): <= kWaveStrip rows, shorter when the call is
  // short, down to 128 (a strip streams 31 .. 62 rows more than it sums) -- 200k rows in strips of
  // 512 were 391 waves on 1024 SIMDs: 52 us for a 55 MB read
  long long w_strip = td_round_up(td_ceil_div(total > 0 ? total : 1, 8 * cus), 32);
  w_strip = w_strip < 128 ? 128 : (w_strip > kWaveStrip ? kWaveStrip : w_strip);
  plan->seg_work0.assign(n_segs + 1, 0);
  for (int f = 0; f < n_segs; ++f) {
    plan->seg_work0[f] = (int)plan->works.size() * slabs_per_strip;
    std::vector<LagSeg> one(1, segs[f]);
    std::vector<LagWork> ws = split_work(one, ni > 0 ? t_strip : w_strip);
    plan->works.insert(plan->works.end(), ws.begin(), ws.end());
  }
  plan->seg_work0[n_segs] = (int)plan->works.size() * slabs_per_strip;
  plan->n_strips = (int)plan->works.size();
  plan->n_work = plan->n_strips * slabs_per_strip;     // slabs
  LagParams& p = plan->p;
  p.a = y; p.b = b; p.lda = ldy; p.ldb = ldb; p.ca = d; p.cb = cb; p.a_ones = 0;
  p.e_min = e_min; p.e_count = e_count;
  p.n_groups = 1; p.n_cat = 1; p.n_cbt = (int)td_ceil_div(cb, 64);
  p.e_pad = e_count; p.ca_pad = ni > 0 ? ni : 1; p.cb_pad = p.n_cbt * 64;
  p.n_work = plan->n_work;
  p.lag_g = 8; p.lag_lg = 3; p.partial = nullptr; p.works = nullptr;
  const size_t slab_elems = ni > 0 ? (size_t)p.e_pad * p.ca_pad * p.cb_pad : 0;
  plan->part_bytes = td_round_up(slab_elems * plan->n_work * sizeof(double), 256);
  plan->cs_bytes = td_round_up((size_t)plan->n_work * p.cb_pad * sizeof(double), 256);
  plan->ys_bytes = td_round_up((size_t)plan->n_work * sizeof(double), 256);
  const int cols = d > 0 ? d : 1;
  plan->scratch_bytes = plan->cs_bytes + cols * (plan->part_bytes + plan->ys_bytes);
  return TD_OK;
}

int td_lagcov_targets_launch(td_handle* h, TargetsPlan* plan, void* scratch, double* g_dev,
                             bool accumulate, TargetsOutputs* out) {
  LagParams p = plan->p;
  const int d = plan->d, cb = plan->cb, e_count = plan->e_count, n_work = plan->n_work;
  char* base = reinterpret_cast<char*>(scratch);
  double* csum = reinterpret_cast<double*>(base);
  out->csum = csum; out->n_work = n_work; out->cb_pad = p.cb_pad;
  for (int i = 0; i < 4; ++i) out->ysum[i] = nullptr;
  if (n_work == 0) return TD_OK;
  const void* works_dev = nullptr;
  TD_TRY(td_table_upload(h, plan->works.data(), plan->works.size() * sizeof(LagWork), &works_dev));
  p.works = reinterpret_cast<const LagWork*>(works_dev);
  const int cols = d > 0 ? d : 1;
  if (d == 0) {
    double* ysum = reinterpret_cast<double*>(base + plan->cs_bytes + plan->part_bytes);
    const unsigned blocks = (unsigned)td_ceil_div((int64_t)n_work * p.n_cbt, kThreads / 64);
    if (cb <= 32) {
      int cbp = 1;
      while (cbp < cb) cbp <<= 1;
      hipLaunchKernelGGL(colsum_rows_kernel, dim3(blocks), dim3(kThreads), 0, h->stream, p, csum, cbp);
    } else {
      hipLaunchKernelGGL((lagcov_wave_kernel<32, 0>), dim3(blocks), dim3(kThreads), 0, h->stream, p,
                         nullptr, csum, ysum);
    }
  } else {
    const float* y = p.a;
    const bool vec2 = (p.ldb % 2 == 0) && (cb % 2 == 0) && ((reinterpret_cast<uintptr_t>(p.b) & 7) == 0);
    // (td_lagcov_column: several windows of 32 lags per work item, see the kernel)
    const int n_win = (int)td_ceil_div(e_count, 32);
    p.n_groups = n_win;
    const dim3 grid((unsigned)(td_ceil_div((int64_t)plan->n_strips * p.n_cbt, 8) * 8 * n_win));
    for (int i = 0; i < cols; ++i) {
      // target column i: A = y + i (one column), output row i of every lag
      LagParams pi = p;
      pi.a = y + i;
      pi.ca = 1;
      char* col = base + plan->cs_bytes + (size_t)i * (plan->part_bytes + plan->ys_bytes);
      double* part64 = reinterpret_cast<double*>(col);
      double* ysum = reinterpret_cast<double*>(col + plan->part_bytes);
      unsigned* maxtab = i == 0 ? out->maxtab : nullptr;        // (one column's pass is enough)
      if (h->targets_f16 && !plan->lag_window && cb > 32 && vec2 && n_win == 1)
        hipLaunchKernelGGL(lagcov_targets_split_kernel, grid, dim3(kThreads), 0, h->stream, pi, part64, csum,
                           ysum, maxtab);
      else if (cb <= 32)
        hipLaunchKernelGGL((lagcov_targets_mfma_kernel<false, true>), grid, dim3(kThreads), 0, h->stream,
                           pi, part64, csum, ysum, maxtab);
      else if (vec2)
        hipLaunchKernelGGL((lagcov_targets_mfma_kernel<true>), grid, dim3(kThreads), 0, h->stream,
                           pi, part64, csum, ysum, maxtab);
      else
        hipLaunchKernelGGL((lagcov_targets_mfma_kernel<false>), grid, dim3(kThreads), 0, h->stream,
                           pi, part64, csum, ysum, maxtab);
      LagReduceJob& job = out->jobs[i];
      job = LagReduceJob{};
      job.partial = part64; job.is_f64 = 1;
      job.n_work = n_work; job.e_pad = p.e_pad; job.ca_pad = p.ca_pad; job.cb_pad = p.cb_pad;
      job.e_count = e_count; job.ca_eff = 1; job.cb = cb;
      job.g = g_dev + (size_t)i * cb; job.accumulate = accumulate ? 1 : 0; job.ca_dst = d + 1;
      job.ldg = cb; job.mirror = 0;
      out->ysum[i] = ysum;
    }
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_lagcov_targets(td_handle* h, const float* y, int64_t ldy, int d, const float* b, int64_t ldb,
                      int cb, const std::vector<LagSeg>& segs, int e_min, int e_count,
                      double* g_dev, double* sy_dev, double* colsum_seg_dev, bool* handled, int rows_dst) {
  // (rows_dst: rows per lag of g_dev when the d columns are a slice of more targets; 0 = d + 1)
  if (rows_dst <= 0) rows_dst = d + 1;
  TargetsPlan plan;
  TD_TRY(td_lagcov_targets_plan(h, y, ldy, d, b, ldb, cb, segs, e_min, e_count, &plan));
  *handled = plan.handled;
  if (!plan.handled || segs.empty()) return TD_OK;
  const int n_segs = plan.n_segs;
  if (plan.n_work == 0) {
    TD_HIP(h, hipMemsetAsync(colsum_seg_dev, 0, sizeof(double) * n_segs * cb, h->stream));
    return TD_OK;
  }
  void* scratch = nullptr;
  TD_TRY(td_scratch(h, plan.scratch_bytes, &scratch));
  TargetsOutputs out;
  out.maxtab = nullptr;
  TD_TRY(td_lagcov_targets_launch(h, &plan, scratch, g_dev, true, &out));
  for (int i = 0; i < d; ++i) {
    LagReduceJob job = out.jobs[i];
    job.ca_dst = rows_dst;       // (the launch described a dense [e][d + 1][cb]; the rest is as it set it)
    TD_TRY(td_lagcov_reduce(h, job));
    if (sy_dev)
      hipLaunchKernelGGL(ysum_reduce_kernel, dim3(1), dim3(256), 0, h->stream, out.ysum[i], job.n_work,
                         1, sy_dev + i, 1);
  }
  const void* seg_dev = nullptr;
  TD_TRY(td_table_upload(h, plan.seg_work0.data(), (n_segs + 1) * sizeof(int), &seg_dev));
  hipLaunchKernelGGL(colsum_file_reduce_kernel, dim3((unsigned)n_segs, (unsigned)plan.p.n_cbt),
                     dim3(1024), 0, h->stream, out.csum, plan.p.cb_pad, cb,
                     reinterpret_cast<const int*>(seg_dev), colsum_seg_dev);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int td_lagcov_column(td_handle* h, const float* y, int64_t ldy, const float* b, int64_t ldb, int cb,
                     const std::vector<LagSeg>& segs, int e_min, int e_count, double* g_dev, int rows_dst) {
  // (rows_dst: rows of cb numbers per lag of g_dev when the column is one of several targets)
  if (rows_dst <= 0) rows_dst = 1;
  if (segs.empty()) return TD_OK;
  for (int k0 = 0; k0 < e_count; k0 += 32 * 8) {       // (one launch covers 8 windows = 256 lags)
    const int cnt = e_count - k0 < 32 * 8 ? e_count - k0 : 32 * 8;
    TargetsPlan plan;
    TD_TRY(td_lagcov_targets_plan(h, y, ldy, 1, b, ldb, cb, segs, e_min + k0, cnt, &plan, true));
    TD_REQUIRE(h, plan.handled, "lagcov_column: the targets kernel refused the shape");
    if (plan.n_work == 0) continue;
    void* scratch = nullptr;
    TD_TRY(td_scratch(h, plan.scratch_bytes, &scratch));
    TargetsOutputs out;
    out.maxtab = nullptr;
    double* dst = g_dev + (size_t)k0 * cb * rows_dst;
    TD_TRY(td_lagcov_targets_launch(h, &plan, scratch, dst, true, &out));
    LagReduceJob job = out.jobs[0];
    job.ca_dst = rows_dst;
    TD_TRY(td_lagcov_reduce(h, job));
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}
