// The online EEG front end (td_frontend_*): preprocess.hip's chain -- the cascade of second-order sections, the
// nearest-neighbour resample, re-referencing by groups, channel selection, normalisation, the float32 cast -- for raw
// rows that arrive in pushes of any length, as the online family does everything else: the state on the device, one
// workgroup per session, ONE launch per push, and any cut of a recording gives the bytes of one push.
//
// The filter.  A lane owns one channel of its session and keeps the cascade's 2 S state doubles in registers (the
// kernel is compiled per section count, as preprocess.hip's are).  It walks the push's rows in order -- there is no
// chunk scan, so where a push ends cannot matter -- with every fused multiply-add written out, in this order:
//     y  = fma(b0, x, z0)
//     z0 = fma(-a1, y, fma(b1, x, z1))
//     z1 = fma(-a2, y, b2 * x)
//     x  = y
// Contraction is off for the whole file: the bits do not depend on what the compiler would choose to fuse.  The loads
// of a row are one coalesced line across the lanes and do not depend on the recurrence: they are issued four rows
// ahead of the steps that use them.  Reset (rows_before == 0): sections [0, split) start from x[0] * zi, sections
// [split, S) from y0 * zi with y0 the output that the first stage's step itself produces on row 0.
//
// The resample.  Output frame j reads row r_j = rint((j * (1.0 / fs_out)) * fs_in); the host says which frames a
// push emits (td_frontend_plan) and every lane computes their rows itself.  A row before this push is the held
// frame's (it was pushed, F(N) did not count its frame yet: only when downsampling) or the last one (a flush clamps
// to it: only when upsampling): both filtered rows are part of the state.  The held slot always carries the row of
// the last frame in reach, whether it waits or not, so the state is a function of the rows pushed, not of the cut.
//
// Behind the resample.  The filtered rows of a pass of frames go to an LDS tile [pass][c] in float64; then all
// threads of the workgroup restate group_means_kernel, reref_select_kernel and context_out_kernel (pre = post = 0)
// operation for operation -- a group's mean is the sequential sum over its reference channels in list order divided
// by their count, the subtractions go in group order from the values before any group was subtracted, then the
// selection, (v - mean) / std, the (float) cast -- and store coalesced.  LDS: 8 pass (c + groups) bytes.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are in DESIGN.md section 30.  The sections are NOT split
// over lanes: one lane runs the whole cascade of its channel (section 30 says where a push's time goes).
#include <cmath>

#include "td_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxSections = 16;
constexpr int kMaxChannels = 128;
constexpr int kThreads = 128;                 // a lane per channel; all of them behind the resample
constexpr int kPass = 64;                     // emitted frames per pass; halved until the LDS budget holds
constexpr int kAhead = 4;                     // rows whose loads are issued in front of their steps
constexpr long long kLdsBudget = TD_FRONTEND_LDS_BYTES;

// b0 b1 b2 a1 a2 per section (a0 = 1) and the stage's sosfilt_zi, by value: uniform across lanes (scalar loads)
struct SosCoef {
  double c[kMaxSections][5];
  double zi[kMaxSections][2];
};

struct FrontParams {
  const void* x; long long ldx, x_ss;
  long long n, rows_before;       // rows of this push, rows pushed before it
  long long e0;                   // the first frame this push emits
  int emitted;                    // frames this push emits
  int c, cs, split, reset, same_rate, n_groups, pass;
  double fs_in, delta_out;        // delta_out = 1.0 / fs_out
  // The held row of the state is the filtered row of frame G(N) - 1, the last frame whose row has been pushed (a
  // function of N alone, so any cut leaves the same bytes).  held_src: that row when this push brought it, -1: the
  // slot stays; held_frame: the frame, which this push may emit itself.
  long long held_src, held_frame;
  const int* tab; int o_mp, o_mi, o_rp, o_ri;   // sel | memb_ptr | memb_idx | ref_ptr | ref_idx (td_reref_select's)
  const double* mean; const double* std_dev; long long stat_ss;
  unsigned char* state; long long state_ss;
  float* out32; double* out64; long long ldout, out_ss;
  SosCoef k;
};

long long state_bytes(int c, int s_count) { return 8LL * (2 * s_count + 2) * c; }

long long lds_bytes(int c, int n_groups, int pass) { return 8LL * pass * (c + n_groups); }

int pass_of(int c, int n_groups, long long emitted) {
  int pass = emitted < kPass ? (emitted > 1 ? (int)emitted : 1) : kPass;
  while (pass > 1 && lds_bytes(c, n_groups, pass) > kLdsBudget) pass = (pass + 1) / 2;
  return pass;
}

// ---- the resample plan (host): the reference's float64 products in its order (preprocess.resample_indices)
struct Rates {
  double fs_in, fs_out, delta_out;
  bool same;
};

__host__ __device__ inline long long frame_row(long long j, double delta_out, double fs_in, bool same) {
  return same ? j : (long long)rint(((double)j * delta_out) * fs_in);
}

// F(N): the frames of a recording of N rows
long long frames_of(const Rates& r, long long n) {
  return r.same ? n : (long long)rint((double)n / r.fs_in * r.fs_out);
}

// G(N): the frames whose row is among the first N
long long frames_in_reach(const Rates& r, long long n) {
  if (n <= 0) return 0;
  if (r.same) return n;
  long long g = (long long)((double)n / r.fs_in * r.fs_out);
  if (g < 0) g = 0;
  while (g > 0 && frame_row(g - 1, r.delta_out, r.fs_in, false) > n - 1) --g;
  while (frame_row(g, r.delta_out, r.fs_in, false) <= n - 1) ++g;
  return g;
}

struct PushPlan {
  long long e0, e1, held, held_src, held_frame;
};

// false: more than one frame would be held back (no pair of rates is known to do that; the state carries one row).
bool plan_push(const Rates& r, long long rows_before, long long n, int flush, PushPlan* p) {
  const long long n1 = rows_before + n;
  const long long g0 = frames_in_reach(r, rows_before), f0 = frames_of(r, rows_before);
  const long long g1 = frames_in_reach(r, n1), f1 = frames_of(r, n1);
  p->e0 = g0 < f0 ? g0 : f0;
  p->e1 = flush ? f1 : (g1 < f1 ? g1 : f1);
  if (p->e1 < p->e0) p->e1 = p->e0;
  p->held = g1 > p->e1 ? g1 - p->e1 : 0;
  p->held_src = -1;
  p->held_frame = g1 - 1;
  if (g0 - p->e0 > 1 || (!flush && p->held > 1)) return false;
  if (n > 0) {                                 // (g1 >= 1: row 0 is frame 0's)
    const long long row = frame_row(g1 - 1, r.delta_out, r.fs_in, r.same);
    if (row >= rows_before) p->held_src = row - rows_before;
  }
  return true;
}

template <typename T>
__device__ __forceinline__ double load_x(const T* x, long long ldx, long long row, int c) {
  return (double)x[row * ldx + c];
}

// One row through the cascade.  kc: b0 b1 b2 -a1 -a2 per section, in the lane's registers.
template <int S>
__device__ __forceinline__ double sos_step(const double (&kc)[5 * S + 1], double (&z)[2 * S + 1], double x) {
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const double y = fma(kc[5 * i], x, z[2 * i]);
    z[2 * i] = fma(kc[5 * i + 3], y, fma(kc[5 * i + 1], x, z[2 * i + 1]));
    z[2 * i + 1] = fma(kc[5 * i + 4], y, kc[5 * i + 2] * x);
    x = y;
  }
  return x;
}

// Row 0 of a recording: each stage starts from zi x (the stage's input on this row), then takes its step.
template <int S>
__device__ __forceinline__ double sos_first(const SosCoef& k, const double (&kc)[5 * S + 1], int split,
                                            double (&z)[2 * S + 1], double x) {
  double base = x;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    if (i == split) base = x;                 // the second stage's input: the first stage's output on this row
    z[2 * i] = base * k.zi[i][0];
    z[2 * i + 1] = base * k.zi[i][1];
    const double y = fma(kc[5 * i], x, z[2 * i]);
    z[2 * i] = fma(kc[5 * i + 3], y, fma(kc[5 * i + 1], x, z[2 * i + 1]));
    z[2 * i + 1] = fma(kc[5 * i + 4], y, kc[5 * i + 2] * x);
    x = y;
  }
  return x;
}

template <int S, typename T>
__global__ void __launch_bounds__(kThreads) frontend_push_kernel(FrontParams p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, s = blockIdx.x;
  const int c = p.c, cs = p.cs, pass = p.pass, ng = p.n_groups;
  double* tile = lds;                          // [pass][c] filtered rows of the pass's frames
  double* means = lds + (size_t)pass * c;      // [pass][ng]
  const T* x = reinterpret_cast<const T*>(p.x) + (long long)s * p.x_ss;
  double* st = reinterpret_cast<double*>(p.state + (long long)s * p.state_ss);
  double* held_p = st + (long long)2 * S * c;
  double* last_p = held_p + c;
  const double mean = p.mean[(long long)s * p.stat_ss], std_dev = p.std_dev[(long long)s * p.stat_ss];
  const bool active = tid < c;
  const long long n = p.n, n_all = p.rows_before + p.n;

  // The coefficients arrive by value, uniform across the lanes: left to itself the compiler keeps them in scalar
  // registers, of which a cascade of more than a few sections has too few (they would be spilled and fetched back
  // lane by lane inside the recurrence).  The empty statement pins each one in a vector register of the lane.
  double kc[5 * S + 1];
#pragma unroll
  for (int i = 0; i < S; ++i) {
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      double v = j < 3 ? p.k.c[i][j] : -p.k.c[i][j];
      asm volatile("" : "+v"(v));
      kc[5 * i + j] = v;
    }
  }
  double z[2 * S + 1];
  double cur = 0.0;                            // the filtered value of row t - 1
  double held_v = 0.0;
  const bool held_in_loop = p.held_src >= 0 && p.held_frame >= p.e0 && p.held_frame < p.e0 + p.emitted;
  long long t = 0;                             // rows of this push the lane has taken
  if (active) {
    if (p.reset) {
      cur = sos_first<S>(p.k, kc, p.split, z, load_x(x, p.ldx, 0, tid));
      t = 1;
    } else {
#pragma unroll
      for (int j = 0; j < 2 * S; ++j) z[j] = st[(long long)j * c + tid];
    }
  }
  // the lane's rows up to (not including) t_end
  auto advance = [&](long long t_end) {
    while (t + kAhead <= t_end) {
      double xv[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) xv[u] = load_x(x, p.ldx, t + u, tid);
#pragma unroll
      for (int u = 0; u < kAhead; ++u) cur = sos_step<S>(kc, z, xv[u]);
      t += kAhead;
    }
    for (; t < t_end; ++t) cur = sos_step<S>(kc, z, load_x(x, p.ldx, t, tid));
  };

  for (int a = 0; a < p.emitted; a += pass) {
    const int nf = p.emitted - a < pass ? p.emitted - a : pass;
    if (active) {
      for (int f = 0; f < nf; ++f) {
        long long row = frame_row(p.e0 + a + f, p.delta_out, p.fs_in, p.same_rate != 0);
        row = (row < n_all - 1 ? row : n_all - 1) - p.rows_before;     // (a flush clamps to the last row)
        double v;
        if (row >= 0) {
          advance(row + 1);
          v = cur;
        } else {
          v = row == -1 ? last_p[tid] : held_p[tid];
        }
        tile[f * c + tid] = v;
        if (held_in_loop && p.e0 + a + f == p.held_frame) held_v = v;
      }
    }
    __syncthreads();
    // ---- group_means_kernel: the sequential sum over the reference channels, divided by their count
    if (ng) {
      const int* ref_ptr = p.tab + p.o_rp;
      const int* ref_idx = p.tab + p.o_ri;
      for (int i = tid; i < nf * ng; i += kThreads) {
        const int f = i / ng, grp = i - f * ng;
        const double* xr = tile + f * c;
        double sum = 0.0;
        const int b = ref_ptr[grp], e = ref_ptr[grp + 1];
        for (int q = b; q < e; ++q) sum += xr[ref_idx[q]];
        means[i] = sum / (double)(e - b);
      }
      __syncthreads();
    }
    // ---- reref_select_kernel, then context_out_kernel's (z - mean) / std and its cast
    {
      const int* sel = p.tab;
      const int* memb_ptr = p.tab + p.o_mp;
      const int* memb_idx = p.tab + p.o_mi;
      for (int i = tid; i < nf * cs; i += kThreads) {
        const int f = i / cs, j = i - f * cs;
        const int ch = sel[j];
        double v = tile[f * c + ch];
        if (ng) {
          const double* mr = means + f * ng;
          for (int q = memb_ptr[ch]; q < memb_ptr[ch + 1]; ++q) v -= mr[memb_idx[q]];   // group order
        }
        v = (v - mean) / std_dev;
        const long long at = (long long)s * p.out_ss + (long long)(a + f) * p.ldout + j;
        if (p.out64) p.out64[at] = v;
        if (p.out32) p.out32[at] = (float)v;
      }
    }
    __syncthreads();
  }

  // ---- the rest of the push, and the state for the next one
  if (active) {
    if (p.held_src >= 0 && !held_in_loop) {    // (not emitted yet: no emitted frame's row lies behind its row)
      advance(p.held_src + 1);
      held_v = cur;
    }
    if (p.held_src >= 0) held_p[tid] = held_v;
    advance(n);
    if (n > 0) {
#pragma unroll
      for (int j = 0; j < 2 * S; ++j) st[(long long)j * c + tid] = z[j];
      last_p[tid] = cur;
    }
  }
}

template <typename T>
void launch(td_handle* h, int s_count, int sessions, size_t lds, const FrontParams& p) {
  switch (s_count) {
#define TD_FRONT_CASE(S_)                                                                                    \
  case S_:                                                                                                   \
    hipLaunchKernelGGL((frontend_push_kernel<S_, T>), dim3((unsigned)sessions), dim3(kThreads), lds, h->stream, p); \
    break;
    TD_FRONT_CASE(0) TD_FRONT_CASE(1) TD_FRONT_CASE(2) TD_FRONT_CASE(3) TD_FRONT_CASE(4) TD_FRONT_CASE(5)
    TD_FRONT_CASE(6) TD_FRONT_CASE(7) TD_FRONT_CASE(8) TD_FRONT_CASE(9) TD_FRONT_CASE(10) TD_FRONT_CASE(11)
    TD_FRONT_CASE(12) TD_FRONT_CASE(13) TD_FRONT_CASE(14) TD_FRONT_CASE(15) TD_FRONT_CASE(16)
#undef TD_FRONT_CASE
  }
}

int check_rates(td_handle* h, const char* who, double fs_in, double fs_out, Rates* r) {
  TD_REQUIRE(h, fs_in > 0.0 && fs_out > 0.0 && std::isfinite(fs_in) && std::isfinite(fs_out),
             "%s: rates of %g and %g Hz (positive and finite)", who, fs_in, fs_out);
  r->fs_in = fs_in;
  r->fs_out = fs_out;
  r->delta_out = 1.0 / fs_out;
  r->same = fs_in == fs_out;
  return TD_OK;
}

}  // namespace

extern "C" {

int td_frontend_state_bytes(int c, int num_sections, int64_t* bytes) {
  if (!bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_frontend_state_bytes: NULL argument");
  TD_REQUIRE(nullptr, c >= 1 && c <= kMaxChannels, "td_frontend_state_bytes: %d channels (1 .. %d)", c, kMaxChannels);
  TD_REQUIRE(nullptr, num_sections >= 0 && num_sections <= kMaxSections,
             "td_frontend_state_bytes: %d sections (0 .. %d)", num_sections, kMaxSections);
  *bytes = state_bytes(c, num_sections);
  return TD_OK;
}

int td_frontend_plan(int64_t rows_before, int64_t n, double fs_in, double fs_out, int flush,
                     int64_t* frames_before, int64_t* frames_after, int64_t* held) {
  if (!frames_before || !frames_after || !held)
    return td_fail(nullptr, TD_ERR_INVALID, "td_frontend_plan: NULL argument");
  Rates r;
  TD_TRY(check_rates(nullptr, "td_frontend_plan", fs_in, fs_out, &r));
  TD_REQUIRE(nullptr, rows_before >= 0 && n >= 0, "td_frontend_plan: %lld rows behind %lld", (long long)n,
             (long long)rows_before);
  PushPlan p;
  TD_REQUIRE(nullptr, plan_push(r, rows_before, n, flush, &p),
             "td_frontend_plan: %g -> %g Hz holds more than one frame back at row %lld", fs_in, fs_out,
             (long long)(rows_before + n));
  *frames_before = p.e0;
  *frames_after = p.e1;
  *held = p.held;
  return TD_OK;
}

int td_frontend_lds_bytes(int c, int num_groups, int64_t emitted, int* pass, int64_t* bytes) {
  if (!pass || !bytes) return td_fail(nullptr, TD_ERR_INVALID, "td_frontend_lds_bytes: NULL argument");
  TD_REQUIRE(nullptr, c >= 1 && c <= kMaxChannels, "td_frontend_lds_bytes: %d channels (1 .. %d)", c, kMaxChannels);
  TD_REQUIRE(nullptr, num_groups >= 0 && num_groups <= TD_FRONTEND_MAX_GROUPS,
             "td_frontend_lds_bytes: %d groups (0 .. %d)", num_groups, TD_FRONTEND_MAX_GROUPS);
  TD_REQUIRE(nullptr, emitted >= 0, "td_frontend_lds_bytes: %lld frames", (long long)emitted);
  *pass = pass_of(c, num_groups, emitted);
  *bytes = lds_bytes(c, num_groups, *pass);
  return TD_OK;
}

int td_frontend_push(td_handle* h, int num_sessions, const void* x_dev, int x_is_f64, int64_t ldx,
                     int64_t x_session_stride, int64_t n, int c, const double* sos_host, int num_sections,
                     int stage_split, const double* zi_host, double fs_in, double fs_out, int num_groups,
                     const int* ref_ptr_host, const int* ref_idx_host, const int* chan_ptr_host,
                     const int* chan_idx_host, const int* sel_host, int cs, const double* mean_dev,
                     const double* std_dev, int64_t stat_session_stride, int64_t rows_before, int flush,
                     void* state_dev, int64_t state_session_stride, float* out32_dev, double* out64_dev,
                     int64_t ldout, int64_t out_session_stride) {
  if (!h) return td_fail(nullptr, TD_ERR_INVALID, "td_frontend_push: handle is NULL");
  TD_REQUIRE(h, num_sessions >= 1, "td_frontend_push: %d sessions", num_sessions);
  TD_REQUIRE(h, c >= 1 && c <= kMaxChannels, "td_frontend_push: %d channels (1 .. %d)", c, kMaxChannels);
  TD_REQUIRE(h, cs >= 1 && cs <= kMaxChannels, "td_frontend_push: %d selected channels (1 .. %d)", cs, kMaxChannels);
  TD_REQUIRE(h, num_sections >= 0 && num_sections <= kMaxSections, "td_frontend_push: %d sections (0 .. %d)",
             num_sections, kMaxSections);
  TD_REQUIRE(h, num_sections == 0 || (sos_host && zi_host), "td_frontend_push: sections without sos_host / zi_host");
  TD_REQUIRE(h, stage_split >= 0 && stage_split <= num_sections, "td_frontend_push: a stage split of %d in %d sections",
             stage_split, num_sections);
  for (int i = 0; i < num_sections; ++i)
    TD_REQUIRE(h, sos_host[6 * i + 3] == 1.0, "td_frontend_push: section %d is not normalised (a0 != 1)", i);
  Rates r;
  TD_TRY(check_rates(h, "td_frontend_push", fs_in, fs_out, &r));
  TD_REQUIRE(h, n >= 0 && n <= TD_ONLINE_MAX_PUSH, "td_frontend_push: %lld rows in one push (0 .. %d)", (long long)n,
             TD_ONLINE_MAX_PUSH);
  TD_REQUIRE(h, rows_before >= 0, "td_frontend_push: %lld rows before", (long long)rows_before);
  TD_REQUIRE(h, num_groups >= 0 && num_groups <= TD_FRONTEND_MAX_GROUPS, "td_frontend_push: %d groups (0 .. %d)",
             num_groups, TD_FRONTEND_MAX_GROUPS);
  TD_REQUIRE(h, num_groups == 0 || (ref_ptr_host && ref_idx_host && chan_ptr_host && chan_idx_host),
             "td_frontend_push: groups without their tables");
  if (!mean_dev || !std_dev || !state_dev || (!out32_dev && !out64_dev) || (n > 0 && !x_dev))
    return td_fail(h, TD_ERR_INVALID, "td_frontend_push: NULL argument");
  TD_REQUIRE(h, ldx >= c && ldout >= cs,
             "td_frontend_push: a row stride below a row (%lld for %d channels in, %lld for %d out)", (long long)ldx, c,
             (long long)ldout, cs);
  TD_REQUIRE(h, num_sessions == 1 || (x_session_stride >= c && out_session_stride >= cs),
             "td_frontend_push: a session stride below a row");
  TD_REQUIRE(h, stat_session_stride >= 0, "td_frontend_push: a mean / std stride of %lld (0 = shared)",
             (long long)stat_session_stride);
  const long long sbytes = state_bytes(c, num_sections);
  TD_REQUIRE(h, state_session_stride >= sbytes && state_session_stride % 8 == 0,
             "td_frontend_push: a state stride of %lld bytes (a multiple of 8, at least %lld)",
             (long long)state_session_stride, sbytes);
  // the tables of td_reref_select: sel | memb_ptr | memb_idx | ref_ptr | ref_idx
  std::vector<int> tabv(cs);
  for (int j = 0; j < cs; ++j) {
    tabv[j] = sel_host ? sel_host[j] : j;
    TD_REQUIRE(h, tabv[j] >= 0 && tabv[j] < c, "td_frontend_push: selected channel %d of %d", tabv[j], c);
  }
  std::vector<int> memb_ptr(c + 1, 0), memb_idx, ref_ptr(1, 0), ref_idx;
  if (num_groups) {
    std::vector<std::vector<int>> per(c);
    for (int g = 0; g < num_groups; ++g) {
      TD_REQUIRE(h, ref_ptr_host[g + 1] > ref_ptr_host[g], "td_frontend_push: group %d has no reference channel", g);
      for (int i = ref_ptr_host[g]; i < ref_ptr_host[g + 1]; ++i) {
        TD_REQUIRE(h, ref_idx_host[i] >= 0 && ref_idx_host[i] < c, "td_frontend_push: reference channel %d of %d",
                   ref_idx_host[i], c);
        ref_idx.push_back(ref_idx_host[i]);
      }
      ref_ptr.push_back((int)ref_idx.size());
      TD_REQUIRE(h, chan_ptr_host[g + 1] >= chan_ptr_host[g], "td_frontend_push: group %d's channel list runs backwards",
                 g);
      for (int i = chan_ptr_host[g]; i < chan_ptr_host[g + 1]; ++i) {
        const int ch = chan_idx_host[i];
        TD_REQUIRE(h, ch >= 0 && ch < c, "td_frontend_push: re-referenced channel %d of %d", ch, c);
        if (per[ch].empty() || per[ch].back() != g) per[ch].push_back(g);
      }
    }
    for (int ch = 0; ch < c; ++ch) {
      memb_ptr[ch + 1] = memb_ptr[ch] + (int)per[ch].size();
      memb_idx.insert(memb_idx.end(), per[ch].begin(), per[ch].end());
    }
  }
  if (memb_idx.empty()) memb_idx.push_back(0);
  if (ref_idx.empty()) ref_idx.push_back(0);
  PushPlan pl;
  TD_REQUIRE(h, plan_push(r, rows_before, n, flush, &pl),
             "td_frontend_push: %g -> %g Hz holds more than one frame back at row %lld", fs_in, fs_out,
             (long long)(rows_before + n));
  const long long emitted = pl.e1 - pl.e0;
  TD_REQUIRE(h, emitted <= TD_ONLINE_MAX_PUSH, "td_frontend_push: %lld frames from one push (0 .. %d)", emitted,
             TD_ONLINE_MAX_PUSH);
  if (n == 0 && emitted == 0) return TD_OK;

  FrontParams p;
  memset(&p, 0, sizeof(p));
  p.o_mp = (int)tabv.size();
  tabv.insert(tabv.end(), memb_ptr.begin(), memb_ptr.end());
  p.o_mi = (int)tabv.size();
  tabv.insert(tabv.end(), memb_idx.begin(), memb_idx.end());
  p.o_rp = (int)tabv.size();
  tabv.insert(tabv.end(), ref_ptr.begin(), ref_ptr.end());
  p.o_ri = (int)tabv.size();
  tabv.insert(tabv.end(), ref_idx.begin(), ref_idx.end());
  const void* tab_dev = nullptr;
  TD_TRY(td_table_upload(h, tabv.data(), tabv.size() * sizeof(int), &tab_dev));
  p.tab = reinterpret_cast<const int*>(tab_dev);
  p.x = x_dev; p.ldx = ldx; p.x_ss = num_sessions > 1 ? x_session_stride : 0;
  p.n = n; p.rows_before = rows_before; p.e0 = pl.e0; p.emitted = (int)emitted;
  p.c = c; p.cs = cs; p.split = stage_split; p.reset = rows_before == 0 ? 1 : 0; p.same_rate = r.same ? 1 : 0;
  p.n_groups = num_groups; p.pass = pass_of(c, num_groups, emitted);
  p.fs_in = r.fs_in; p.delta_out = r.delta_out; p.held_src = pl.held_src; p.held_frame = pl.held_frame;
  p.mean = mean_dev; p.std_dev = std_dev; p.stat_ss = stat_session_stride;
  p.state = reinterpret_cast<unsigned char*>(state_dev); p.state_ss = state_session_stride;
  p.out32 = out32_dev; p.out64 = out64_dev; p.ldout = ldout; p.out_ss = num_sessions > 1 ? out_session_stride : 0;
  for (int i = 0; i < num_sections; ++i) {
    for (int j = 0; j < 3; ++j) p.k.c[i][j] = sos_host[6 * i + j];
    p.k.c[i][3] = sos_host[6 * i + 4];
    p.k.c[i][4] = sos_host[6 * i + 5];
    p.k.zi[i][0] = zi_host[2 * i];
    p.k.zi[i][1] = zi_host[2 * i + 1];
  }
  const size_t lds = (size_t)lds_bytes(c, num_groups, p.pass);
  TD_TRY(td_profile_mark(h, true, (double)n * num_sessions));
  if (x_is_f64) launch<double>(h, num_sections, num_sessions, lds, p);
  else launch<float>(h, num_sections, num_sessions, lds, p);
  TD_HIP(h, hipGetLastError());
  TD_TRY(td_profile_mark(h, false, 0.0));
  return TD_OK;
}

}  // extern "C"
