// Fully connected regressor (brain_model.BrainModelDNN; reference brain_model.py:486-549): training by
// RMSprop, its gradients and inference, on the lagged view of the raw recordings -- the lag matrix is never
// built.  Entry points td_mlp_train / td_mlp_grad / td_mlp_forward (include/td_hotpath.h).
// The match-mismatch classifier (brain_model.BrainModelClassifier; reference :554-620) is the same kernels with
// a second lagged view (x2) concatenated behind the first, a sigmoid output with binary cross-entropy, and Adam:
// td_mlpc_train / td_mlpc_grad / td_mlpc_forward.  The flags below only select: neither family's arithmetic or
// reduction order depends on the other's being there.
// The regressor also trains on the Pearson correlation loss (td_mlp_train_loss / td_mlp_grad_loss, loss 1):
// L = -(1 / B) sum_o r_o over the step's B rows.  dL/dp of a row needs the step's moments of every output
// column, so the head runs as two launches (below).
//
// A training step is three launches, queued from C without a host round trip:
//   slab  one workgroup per slice of W1's rows (K = lags x channels, <= 64 rows a slice): first the update of
//         the PREVIOUS step -- dW1 of the slice = X~^T dZ1 over that step's rows, then RMSprop on the slice --
//         then the partial first-layer pre-activations of THIS step's rows over the slice, zpart[slice][j][r].
//         Extra workgroups reduce the previous step's partial gradients of the small layers (b1, W2, b2, ...)
//         in a fixed order, apply RMSprop to them, and reduce its six loss sums.
//   z1    thread per (unit, row): z1 = the slices' partials summed in slice order, + b1;
//   head  one workgroup per 64 rows: the small layers (their parameters staged in LDS), the loss sums, the
//         backward pass; dZ1 of its rows and its rows' partial gradients of the small layers.
// Where each row of a step reads (file, frame, target row: through the shuffle) comes from a table built once
// per epoch (mlp_rows_kernel).
// Every reduction runs in a fixed order and there are no atomics: two runs are bitwise identical.  A step's
// update is applied by the next step's slab launch, so every layer is updated after the full backward pass
// (Keras); one slab launch after the last step applies the last update.
// With the Pearson loss the head is two launches of the same kernel (four launches a step):
//   head<1>  the forward of its 64 rows, the six history sums, and the workgroup's five float64 raw moments
//            (sum p, y, p^2, y^2, p y) of every output column over its valid rows, rows in order;
//   head<2>  every workgroup sums the <= 32 partial moments in workgroup order, forms r_o and the two
//            coefficients of dL/dp per column in float64, recomputes its rows' forward (the same code on the
//            same inputs: the same bits) and runs the backward pass.  No workgroup waits for another.
//
// Host side (from struct MlpPlan on): every exported entry point packs its arguments into one MlpCall and calls
// mlp_train, mlp_grad or mlp_forward; each of those checks the call (mlp_check_and_plan first, then its own
// arguments, in the order a caller observes), lays out the scratch and queues the launches.
//
// td_dnn_train_many trains many regressors of one architecture on the same recordings at once (the folds of a
// jackknife, a few learning rates): the same three (four) launches per step with the models in blockIdx.y.  The
// kernels' bodies are __device__ functions of (the arguments, the launch's step); a single fit's kernels pass
// their own kernel argument, the batched ones (mlp_*_many_kernel) the model's entry of a device table and a step
// derived from the launch index.  Models share nothing but x and y, so each comes out as its own single fit.
// td_clf_train_many is the same for classifiers: Adam with every model's own settings, lr_t of every update from a
// host-computed table (ManyModel::lr_t), or, with the update off, the scoring of many models in one chain.
#include "td_common.h"

#include <cmath>

namespace {

constexpr int kMlpMaxHidden = 4, kMlpMaxWidth = 64, kMlpMaxD = 8, kMlpMaxB = 2048;
constexpr int kMlpMaxK = 8192, kMlpMaxC = 128, kMlpMaxLags = 64;
constexpr int kSlabThreads = 256;
constexpr int kSlabMaxKs = 64;          // W1 rows per slab workgroup
constexpr int kSlabRowChunk = 64;       // rows staged per pass of the update phase
constexpr int kDzLd = kMlpMaxWidth + 4; // row stride of the staged dZ1 (float4 reads, rows on shifted banks)
constexpr int kHeadRows = 64;           // rows (one per thread) per head workgroup
constexpr int kFwdChunk = 4096;         // rows per step of td_mlp_forward
// LDS of the head kernel at the largest shape: activations of 4 x 64 + 8 units, two dZ buffers, the targets, the
// small parameters (b1, three 64 x 64 layers, the 64 x 8 output layer): 154 KB
constexpr int kHeadMaxLds = 4 * ((4 * kMlpMaxWidth + kMlpMaxD) * kHeadRows + 2 * kMlpMaxWidth * kHeadRows +
                                 kMlpMaxD * kHeadRows + kMlpMaxWidth + 3 * (kMlpMaxWidth + 1) * kMlpMaxWidth +
                                 (kMlpMaxWidth + 1) * kMlpMaxD);

struct MlpGeom {
  const float* x;
  long long ldx;
  const float* y;
  long long ldy;
  const long long* file_offs;     // [nf + 1] rows of x / y
  const long long* stream_offs;   // [nf + 1] rows of the zipped, batched stream (training)
  int nf;
  int c, pre, lags, k;
  int dx, dy;                     // leading rows dropped of x / of y in every file (input_offset)
  int nl;                         // dense layers (hidden + 1)
  int w[kMlpMaxHidden + 2];       // widths: w[0] = k, ..., w[nl] = d
  int off_w[kMlpMaxHidden + 1];   // offsets of W_l, b_l in the packed parameters
  int off_b[kMlpMaxHidden + 1];
  int n_params, small0, n_small;  // small parameters: everything after W1
  long long n_rows;               // rows of the stream (training) / of x (inference)
  int batch;                      // rows per step
  int fwd;                        // 1: row i of chunk s is output row s * batch + i (inference)
  int shuffle;
  unsigned seed_lo, seed_hi;
  // the second view (classifier): inputs k >= k1 are x2~[yrow + l - pre2, ch], l = (k - k1) / c2, zero outside
  // the file's rows that survive the offset.  The regressor has k1 = k and never looks at it.
  const float* x2;
  long long ldx2;
  int c2, pre2, k1;
  int dxy;                        // dy - dx: x2's first row of a file = (x's first row) + dxy
  int bce;                        // 1: sigmoid output, binary cross-entropy (0: linear output, mse)
  int pearson;                    // 1: linear output, the Pearson correlation loss (regressor only)
};

// Where slot i of a pass reads: x rows [base, base + lags) clipped to [lo, hi), target row yrow (32-bit: the
// tables are built once per epoch by mlp_rows_kernel, so the step kernels read one 16-B entry per row)
typedef int4 RowEntry;

// ---- the shuffle: a 4-round Feistel bijection on [0, 4^half), cycle-walked into [0, n) ----------------
__device__ __forceinline__ unsigned mlp_mix32(unsigned z) {
  z ^= z >> 16; z *= 0x7feb352dU; z ^= z >> 15; z *= 0x846ca68bU; z ^= z >> 16;
  return z;
}

__device__ __forceinline__ long long mlp_permute(long long i, long long n, int epoch, unsigned seed_lo,
                                                 unsigned seed_hi) {
  int bits = 2;
  while ((1LL << bits) < n) bits += 2;
  const int half = bits / 2;
  const unsigned mask = (1u << half) - 1u;
  unsigned key[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    key[r] = mlp_mix32(seed_lo ^ mlp_mix32(seed_hi ^ mlp_mix32((unsigned)epoch * 4u + (unsigned)r)));
  unsigned v = (unsigned)i;
  do {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned left = v >> half, right = v & mask;
      v = (right << half) | (left ^ (mlp_mix32(right ^ key[r]) & mask));
    }
  } while ((long long)v >= n);
  return (long long)v;
}

struct RowInfo {
  long long base, lo, hi, yrow;
};

// slot = step * batch + row of the step: where its lagged input and its target are
__device__ __forceinline__ RowInfo mlp_row_search(const MlpGeom& g, long long slot, int epoch) {
  const long long* offs = g.fwd ? g.file_offs : g.stream_offs;
  long long q = slot;
  if (!g.fwd && g.shuffle) q = mlp_permute(slot, g.n_rows, epoch, g.seed_lo, g.seed_hi);
  int lo = 0, hi = g.nf;     // the last file f with offs[f] <= q
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offs[mid] <= q) lo = mid; else hi = mid;
  }
  const long long t = q - offs[lo];
  RowInfo ri;
  ri.lo = g.file_offs[lo] + g.dx;
  ri.hi = g.file_offs[lo + 1];
  ri.base = ri.lo + t - g.pre;
  ri.yrow = g.file_offs[lo] + g.dy + t;
  return ri;
}

__device__ __forceinline__ RowInfo mlp_row(const RowEntry* tab, long long slot) {
  const RowEntry e = tab[slot];
  RowInfo ri;
  ri.base = e.x; ri.lo = e.y; ri.hi = e.z; ri.yrow = e.w;
  return ri;
}

// the row table of one epoch (or of every output row, inference)
__global__ void mlp_rows_kernel(MlpGeom g, int epoch, RowEntry* tab) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < g.n_rows; i += (long long)gridDim.x * blockDim.x) {
    const RowInfo ri = mlp_row_search(g, i, epoch);
    tab[i] = make_int4((int)ri.base, (int)ri.lo, (int)ri.hi, (int)ri.yrow);
  }
}

// lagged input k = l * c + ch of a row: x~[t + l - pre, ch], zero outside the file; k >= k1: the second view
__device__ __forceinline__ float mlp_xt(const MlpGeom& g, const RowInfo& ri, int k) {
  if (k >= g.k1) {
    const int k2 = k - g.k1, l = k2 / g.c2, ch = k2 - l * g.c2;
    const long long row = ri.yrow - g.pre2 + l;
    return (row >= ri.lo + g.dxy && row < ri.hi) ? g.x2[row * g.ldx2 + ch] : 0.f;
  }
  const int l = k / g.c, ch = k - l * g.c;
  const long long row = ri.base + l;
  return (row >= ri.lo && row < ri.hi) ? g.x[row * g.ldx + ch] : 0.f;
}

enum { kUpdRmsprop = 0, kUpdAdam = 1, kUpdNone = 2 };

// What changes from one slab launch of a call to the next.  The host loop of a single fit sets it in SlabArgs::at;
// the batched kernels derive it per model from the launch index (mlp_many_step).
struct SlabStep {
  double* stats_out;      // six sums of the previous step (may be null); Pearson: seven, the last one L
  const RowEntry* prev_rows;   // row tables of the previous / current step's epoch
  const RowEntry* cur_rows;
  int prev_epoch, prev_step;   // -1: no update
  int cur_epoch, cur_step;     // -1: no forward
  float lr;                    // the update's learning rate: RMSprop's lr; Adam's lr_t of this very update
};

struct SlabArgs {
  MlpGeom g;
  float* params;
  float* state;
  float* grad_out;        // non-null: the previous step's gradient is written here instead of applied
  float* zpart;           // [nslices][w1][batch]
  const float* dz1;       // [w1][batch] of the previous step
  const float* gpart;     // [n_head][n_small]
  const double* spart;    // [n_head][6]
  const double* lstat;    // Pearson: the previous step's loss L (written by head<2>)
  SlabStep at;
  int ks, nslices, n_head;
  float rho, eps;              // RMSprop; Adam: rho = beta_1 (the learning rate is the step's: SlabStep::lr)
  float beta2, omb1, omb2;     // Adam: beta_2, 1 - beta_1, 1 - beta_2 (each rounded once from double)
  int update;                  // kUpdRmsprop / kUpdAdam (state = m [P], then v [P]) / kUpdNone (the sums only)
};

__device__ __forceinline__ int mlp_rows_in_step(const MlpGeom& g, int step) {
  const long long left = g.n_rows - (long long)step * g.batch;
  return (int)(left < g.batch ? left : g.batch);
}

// Keras RMSprop without momentum: v = rho v + (1 - rho) g^2, w -= lr g / (sqrt(v) + eps); returns the new w
__device__ __forceinline__ float mlp_rmsprop(float* p, float* v, float grad, float lr, float rho, float eps) {
  // (the roundings spelled out -- rho v rounded, then one fused multiply-add -- so that every kernel this is
  // inlined into computes the same bits; left to the compiler, which of the two products it fuses varies)
  const float vn = fmaf(1.f - rho, grad * grad, rho * *v);
  const float pn = *p - lr * grad / (sqrtf(vn) + eps);
  *v = vn;
  *p = pn;
  return pn;
}

// Keras Adam without amsgrad: m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, w -= lr_t m / (sqrt(v) + eps)
__device__ __forceinline__ float mlp_adam(float* p, float* m, float* v, float grad, const SlabArgs& a, float lr_t) {
  // (the roundings spelled out, as in mlp_rmsprop: b1 m and b2 v rounded, the other product of each sum fused,
  // lr_t m rounded before the division and the subtraction -- the form the compiler's contraction had given the
  // single-model kernels, so that a single fit keeps its bits and the batched kernels compute the same)
  const float mn = fmaf(a.omb1, grad, a.rho * *m);
  const float vn = fmaf(a.omb2, grad * grad, a.beta2 * *v);
  const float pn = *p - (lr_t * mn) / (sqrtf(vn) + a.eps);
  *m = mn;
  *v = vn;
  *p = pn;
  return pn;
}

// the update rule of the call on parameter `at`; returns the new value
__device__ __forceinline__ float mlp_apply(const SlabArgs& a, const SlabStep& st, long long at, float grad) {
  if (a.update == kUpdAdam)
    return mlp_adam(&a.params[at], &a.state[at], &a.state[a.g.n_params + at], grad, a, st.lr);
  return mlp_rmsprop(&a.params[at], &a.state[at], grad, st.lr, a.rho, a.eps);
}

constexpr int kW1Groups = kSlabMaxKs * kMlpMaxWidth / 4 / kSlabThreads;   // (row, 4 columns) groups per thread

// dW1 of the rows [k0, k0 + ksl) over the rows of the previous step: thread group (kk, 4 columns); rows summed
// in order within chunks of 64, the chunks in order
__device__ void mlp_w1_grad(const SlabArgs& a, const SlabStep& st, int k0, int ksl, float (*acc)[4], RowInfo* ri,
                            float (*xs)[kSlabMaxKs + 1], float (*dzs)[kDzLd]) {
  const MlpGeom& g = a.g;
  const int w1 = g.w[1], w1q = (w1 + 3) / 4, tid = threadIdx.x;
  const int rows = mlp_rows_in_step(g, st.prev_step);
  const int n_groups = ksl * w1q;
  for (int r0 = 0; r0 < rows; r0 += kSlabRowChunk) {
    const int nr = rows - r0 < kSlabRowChunk ? rows - r0 : kSlabRowChunk;
    __syncthreads();
    if (tid < nr) ri[tid] = mlp_row(st.prev_rows, (long long)st.prev_step * g.batch + r0 + tid);
    for (int i = tid; i < nr * w1q * 4; i += kSlabThreads) {
      const int j = i / nr, r = i - j * nr;
      dzs[r][j] = j < w1 ? a.dz1[(long long)j * g.batch + r0 + r] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < nr * ksl; i += kSlabThreads) {
      const int r = i / ksl, kk = i - r * ksl;
      xs[r][kk] = mlp_xt(g, ri[r], k0 + kk);
    }
    __syncthreads();
#pragma unroll
    for (int o = 0; o < kW1Groups; ++o) {
      const int grp = tid + o * kSlabThreads;
      if (grp < n_groups) {
        const int kk = grp / w1q, j0 = (grp - kk * w1q) * 4;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int r = 0; r < nr; ++r) {
          const float xv = xs[r][kk];
          const float4 dv = *reinterpret_cast<const float4*>(&dzs[r][j0]);
          s0 = fmaf(xv, dv.x, s0); s1 = fmaf(xv, dv.y, s1); s2 = fmaf(xv, dv.z, s2); s3 = fmaf(xv, dv.w, s3);
        }
        acc[o][0] += s0; acc[o][1] += s1; acc[o][2] += s2; acc[o][3] += s3;
      }
    }
  }
}

// The slab launch of one model: `a` is the launch's kernel argument (a single fit) or the model's entry of the
// device table (the batched kernels); `st` says which steps this launch updates and runs forward.
template <int NJ>
__device__ __forceinline__ void mlp_slab_body(const SlabArgs& a, const SlabStep& st) {
  __shared__ RowInfo ri[kSlabRowChunk];
  __shared__ float xs[kSlabRowChunk][kSlabMaxKs + 1];   // (+1: the forward reads a column, rows on other banks)
  __shared__ __attribute__((aligned(16))) float dzs[kSlabRowChunk][kDzLd];
  __shared__ __attribute__((aligned(16))) float ws[kSlabMaxKs][NJ];
  const MlpGeom& g = a.g;
  const int tid = threadIdx.x, w1 = g.w[1];
  const int wg = blockIdx.x;
  if (wg >= a.nslices) {
    // the small layers' update and the loss sums of the previous step
    if (st.prev_step < 0) return;
    const int p = (wg - a.nslices) * kSlabThreads + tid;
    if (p < g.n_small && a.update != kUpdNone) {
      float s = 0.f;
      for (int hw = 0; hw < a.n_head; ++hw) s += a.gpart[(long long)hw * g.n_small + p];
      if (a.grad_out) a.grad_out[g.small0 + p] = s;
      else mlp_apply(a, st, g.small0 + p, s);
    }
    if (wg == a.nslices && tid < 6 && st.stats_out) {
      double s = 0.0;
      for (int hw = 0; hw < a.n_head; ++hw) s += a.spart[hw * 6 + tid];
      st.stats_out[tid] = s;
    }
    if (wg == a.nslices && tid == 6 && st.stats_out && g.pearson) st.stats_out[6] = a.lstat[0];
    return;
  }
  const int k0 = wg * a.ks;
  const int ksl = g.k - k0 < a.ks ? g.k - k0 : a.ks;
  float* w1p = a.params;   // W1 [k][w1]
  const bool fwd = st.cur_step >= 0;
  // the slice of W1 the forward multiplies by, zero-padded to NJ columns; the update below refreshes it
  if (fwd)
    for (int i = tid; i < kSlabMaxKs * NJ; i += kSlabThreads) {
      const int kk = i / NJ, j = i - kk * NJ;
      ws[kk][j] = (kk < ksl && j < w1) ? w1p[(long long)(k0 + kk) * w1 + j] : 0.f;
    }
  if (st.prev_step >= 0 && a.update != kUpdNone) {
    float acc[kW1Groups][4];
#pragma unroll
    for (int o = 0; o < kW1Groups; ++o) acc[o][0] = acc[o][1] = acc[o][2] = acc[o][3] = 0.f;
    mlp_w1_grad(a, st, k0, ksl, acc, ri, xs, dzs);
    const int w1q = (w1 + 3) / 4;
#pragma unroll
    for (int o = 0; o < kW1Groups; ++o) {
      const int grp = tid + o * kSlabThreads;
      if (grp < ksl * w1q) {
        const int kk = grp / w1q, j0 = (grp - kk * w1q) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (j0 + q < w1) {
            const long long at = (long long)(k0 + kk) * w1 + j0 + q;
            if (a.grad_out) {
              a.grad_out[at] = acc[o][q];
            } else {
              const float nw = mlp_apply(a, st, at, acc[o][q]);
              if (fwd) ws[kk][j0 + q] = nw;
            }
          }
        }
      }
    }
  }
  if (!fwd) return;
  // partial z1 of this step's rows over the slice: chunks of 64 rows staged in LDS, thread = (row, 4 columns)
  const int rows = mlp_rows_in_step(g, st.cur_step);
  constexpr int kQ = NJ / 4;
  for (int r0 = 0; r0 < rows; r0 += kSlabRowChunk) {
    const int nr = rows - r0 < kSlabRowChunk ? rows - r0 : kSlabRowChunk;
    __syncthreads();
    if (tid < nr) ri[tid] = mlp_row(st.cur_rows, (long long)st.cur_step * g.batch + r0 + tid);
    __syncthreads();
    for (int i = tid; i < nr * ksl; i += kSlabThreads) {
      const int r = i / ksl, kk = i - r * ksl;
      xs[r][kk] = mlp_xt(g, ri[r], k0 + kk);
    }
    __syncthreads();
    for (int t = tid; t < kSlabRowChunk * kQ; t += kSlabThreads) {
      const int r = t % kSlabRowChunk, j0 = (t / kSlabRowChunk) * 4;
      if (r >= nr || j0 >= w1) continue;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
      for (int kk = 0; kk < ksl; ++kk) {
        const float xv = xs[r][kk];
        const float4 wv = *reinterpret_cast<const float4*>(&ws[kk][j0]);
        s0 = fmaf(xv, wv.x, s0); s1 = fmaf(xv, wv.y, s1); s2 = fmaf(xv, wv.z, s2); s3 = fmaf(xv, wv.w, s3);
      }
      float* zp = a.zpart + ((long long)wg * w1 + j0) * g.batch + r0 + r;
      zp[0] = s0;
      if (j0 + 1 < w1) zp[g.batch] = s1;
      if (j0 + 2 < w1) zp[2 * (long long)g.batch] = s2;
      if (j0 + 3 < w1) zp[3 * (long long)g.batch] = s3;
    }
  }
}

template <int NJ>
__global__ __launch_bounds__(kSlabThreads) void mlp_slab_kernel(SlabArgs a) {
  mlp_slab_body<NJ>(a, a.at);
}

// z1 = sum of the slices' partials in slice order, + b1: thread per (unit, row)
__device__ __forceinline__ void mlp_z1_body(const float* __restrict__ zpart, int nslices, int w1, int batch, int rows,
                                            const float* __restrict__ b1, float* __restrict__ z1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= w1 * batch) return;
  const int j = i / batch, r = i - j * batch;
  if (r >= rows) return;
  const float* zp = zpart + i;
  const long long stride = (long long)w1 * batch;
  float s = 0.f;
#pragma unroll 8
  for (int sl = 0; sl < nslices; ++sl) s += zp[sl * stride];
  z1[i] = s + b1[j];
}

__global__ __launch_bounds__(256) void mlp_z1_kernel(const float* __restrict__ zpart, int nslices, int w1, int batch,
                                                     int rows, const float* __restrict__ b1, float* __restrict__ z1) {
  mlp_z1_body(zpart, nslices, w1, batch, rows, b1, z1);
}

// What changes from one head launch of a call to the next (as SlabStep).
struct HeadStep {
  const RowEntry* rows_tab;
  int epoch, step;
};

struct HeadArgs {
  MlpGeom g;
  const float* params;
  const float* zpart;
  int nslices;
  HeadStep at;
  int backward;
  float* dz1;       // [w1][batch]
  float* gpart;     // [n_head][n_small]
  double* spart;    // [n_head][6]
  double* mpart;    // Pearson: [n_head][d][5] raw moments of the workgroups' valid rows
  double* lstat;    // Pearson: the step's loss
  float* out;       // inference: [rows, d] (row stride ldout)
  long long ldout;
  const float* z1;  // [w1][batch]: b1 + the slices' partials (mlp_z1_kernel)
  int act_off[kMlpMaxHidden + 2];   // LDS offsets of the activations of layer l = 1 .. nl ([w_l][64])
  int act_floats;
  int maxw;
};

// the classifier's output: sigma(z), and the binary cross-entropy of a logit in its stable form
__device__ __forceinline__ float mlp_sigmoid(float z) {
  const float e = expf(-fabsf(z));
  return z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

__device__ __forceinline__ float mlp_bce(float z, float y) {
  return fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z)));
}

// z1 = b1 + partials, the small layers, the loss sums and the backward pass of 64 rows.
// PP 0: all of it in one launch (mse, bce).  The Pearson loss: PP 1 = forward, sums and the partial moments;
// PP 2 = forward again, the moments' reduction, dL/dp and the backward pass.
// (`a`, `st`: as mlp_slab_body)
template <int PP>
__device__ __forceinline__ void mlp_head_body(const HeadArgs& a, const HeadStep& st) {
  extern __shared__ float lds[];
  const MlpGeom& g = a.g;
  const int tid = threadIdx.x, nl = g.nl, d = g.w[nl];
  float* act = lds;
  float* dzb = lds + a.act_floats;                    // [2][maxw][64]
  float* yb = dzb + 2 * a.maxw * kHeadRows;           // [d][64]
  float* wsm = yb + d * kHeadRows;                    // the small parameters (b1, W2, b2, ...)
  for (int i = tid; i < g.n_small; i += kHeadRows) wsm[i] = a.params[g.small0 + i];
  const float* prm = wsm - g.small0;                  // indexed by parameter offset
  __syncthreads();
  const int rows = mlp_rows_in_step(g, st.step);
  const int r = blockIdx.x * kHeadRows + tid;
  const bool valid = r < rows;
  long long yrow = 0;
  if (valid && !a.out) yrow = mlp_row(st.rows_tab, (long long)st.step * g.batch + r).yrow;
  // layer 1: b1 + the slices' partial sums (mlp_z1_kernel)
  {
    const int w1 = g.w[1];
    float* a1 = act + a.act_off[1];
    for (int j = 0; j < w1; ++j) {
      const float s = valid ? a.z1[(long long)j * g.batch + r] : prm[g.off_b[0] + j];
      a1[j * kHeadRows + tid] = (nl > 1 && s <= 0.f) ? 0.f : s;
    }
  }
  for (int l = 2; l <= nl; ++l) {
    const int wi = g.w[l - 1], wo = g.w[l];
    const float* W = prm + g.off_w[l - 1];
    const float* b = prm + g.off_b[l - 1];
    const float* in = act + a.act_off[l - 1];
    float* outp = act + a.act_off[l];
    for (int o = 0; o < wo; ++o) {
      float s = 0.f;
      for (int i = 0; i < wi; ++i) s = fmaf(in[i * kHeadRows + tid], W[i * wo + o], s);
      s += b[o];
      outp[o * kHeadRows + tid] = (l < nl && s <= 0.f) ? 0.f : s;
    }
  }
  const float* p = act + a.act_off[nl];
  if (a.out) {
    if (valid)
      for (int o = 0; o < d; ++o) {
        const float pv = p[o * kHeadRows + tid];
        a.out[((long long)st.step * g.batch + r) * a.ldout + o] = g.bce ? mlp_sigmoid(pv) : pv;
      }
    return;
  }
  for (int o = 0; o < d; ++o) yb[o * kHeadRows + tid] = valid ? g.y[yrow * g.ldy + o] : 0.f;
  // classifier: p holds the logits; every row's entry losses go to the second dZ buffer (free until the
  // backward pass, which starts behind a barrier)
  float* lossb = dzb + a.maxw * kHeadRows;
  if (g.bce)
    for (int o = 0; o < d; ++o)
      lossb[o * kHeadRows + tid] = valid ? mlp_bce(p[o * kHeadRows + tid], yb[o * kHeadRows + tid]) : 0.f;
  __syncthreads();
  // the six loss sums of these rows in float64, rows in order: sum p, y, p^2, y^2, p y of output column 0 and
  // sum (p - y)^2 over every column
  // (classifier: slot 0 = the number of entries with (z > 0) == (y > 0.5), slot 5 = the sum of the entry
  // losses, slots 1 - 4 = 0; rows in order, outputs in order within a row)
  if constexpr (PP == 2) {
    // (written by the first pass)
  } else if (tid < 6 && g.bce) {
    double s = 0.0;
    const int left = rows - blockIdx.x * kHeadRows;
    const int n = left < kHeadRows ? left : kHeadRows;
    if (tid == 0 || tid == 5)
      for (int rr = 0; rr < n; ++rr)
        for (int o = 0; o < d; ++o) {
          if (tid == 5) s += (double)lossb[o * kHeadRows + rr];
          else if ((p[o * kHeadRows + rr] > 0.f) == (yb[o * kHeadRows + rr] > 0.5f)) s += 1.0;
        }
    a.spart[blockIdx.x * 6 + tid] = s;
  } else if (tid < 6) {
    double s = 0.0;
    const int left = rows - blockIdx.x * kHeadRows;
    const int n = left < kHeadRows ? left : kHeadRows;
    for (int rr = 0; rr < n; ++rr) {
      const double pv = p[rr], yv = yb[rr];
      if (tid == 0) s += pv;
      else if (tid == 1) s += yv;
      else if (tid == 2) s += pv * pv;
      else if (tid == 3) s += yv * yv;
      else if (tid == 4) s += pv * yv;
      else
        for (int o = 0; o < d; ++o) {
          const double e = (double)p[o * kHeadRows + rr] - (double)yb[o * kHeadRows + rr];
          s += e * e;
        }
    }
    a.spart[blockIdx.x * 6 + tid] = s;
  }
  if constexpr (PP == 1) {
    // the raw moments of every output column over this workgroup's valid rows (none: zeros), rows in order
    if (tid < 5 * d) {
      const int o = tid / 5, q = tid - o * 5;
      const int left = rows - blockIdx.x * kHeadRows;
      const int n = left < kHeadRows ? left : kHeadRows;
      double s = 0.0;
      for (int rr = 0; rr < n; ++rr) {
        const double pv = p[o * kHeadRows + rr], yv = yb[o * kHeadRows + rr];
        s += q == 0 ? pv : q == 1 ? yv : q == 2 ? pv * pv : q == 3 ? yv * yv : pv * yv;
      }
      a.mpart[((long long)blockIdx.x * d + o) * 5 + q] = s;
    }
    return;
  }
  if (!a.backward) return;
  float* gp = a.gpart + (long long)blockIdx.x * g.n_small - g.small0;   // indexed by parameter offset
  // dL/dp of Keras 'mse' (the mean over rows x outputs): 2 (p - y) / (rows d)
  // (classifier: dL/dz of the mean binary cross-entropy through the sigmoid: (sigma(z) - y) / (rows d))
  const float scale = (g.bce ? 1.f : 2.f) / ((float)rows * (float)d);
  int cur = 0;
  if constexpr (PP == 2) {
    // L = -(1 / B) sum_o r_o with r_o = Spy / sqrt(Spp Syy) of the step's B rows, so
    // dL/dp[i, o] = -(1 / B) ((y - mean y) / sqrt(Spp Syy) - r_o (p - mean p) / Spp): the coefficients in
    // float64 from the step's raw moments (the workgroups' partials summed in workgroup order), each entry
    // formed in float64 from the float32 p and y and rounded once.  A column that is constant within the step
    // (Spp or Syy within 32 eps of its raw sum of squares: the zero rule of pearson_correlation) has r_o = 0
    // and a zero dZ column.
    __shared__ double mom[kMlpMaxD * 5];
    __shared__ double coef[kMlpMaxD][5];   // mean p, mean y, the coefficients of (y - mean y) and (p - mean p), r
    if (tid < 5 * d) {
      double s = 0.0;
      for (int hw = 0; hw < (int)gridDim.x; ++hw) s += a.mpart[(long long)hw * 5 * d + tid];
      mom[tid] = s;
    }
    __syncthreads();
    if (tid < d) {
      const double* m = mom + 5 * tid;
      const double n = (double)rows;
      const double spp = m[2] - m[0] * m[0] / n, syy = m[3] - m[1] * m[1] / n, spy = m[4] - m[0] * m[1] / n;
      const double tiny = 32.0 * 2.220446049250313e-16;
      double r = 0.0, cy = 0.0, cp = 0.0;
      if (!(spp <= tiny * m[2] || syy <= tiny * m[3])) {
        const double q = sqrt(spp * syy);
        r = spy / q;
        cy = -1.0 / (n * q);
        cp = r / (n * spp);
      }
      coef[tid][0] = m[0] / n; coef[tid][1] = m[1] / n; coef[tid][2] = cy; coef[tid][3] = cp; coef[tid][4] = r;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) {
      double s = 0.0;
      for (int o = 0; o < d; ++o) s += coef[o][4];
      a.lstat[0] = -s / (double)rows;
    }
    for (int o = 0; o < d; ++o) {
      const double pm = (double)p[o * kHeadRows + tid] - coef[o][0];
      const double ym = (double)yb[o * kHeadRows + tid] - coef[o][1];
      dzb[o * kHeadRows + tid] = valid ? (float)(coef[o][2] * ym + coef[o][3] * pm) : 0.f;
    }
  } else {
    for (int o = 0; o < d; ++o) {
      const float pv = g.bce ? mlp_sigmoid(p[o * kHeadRows + tid]) : p[o * kHeadRows + tid];
      dzb[o * kHeadRows + tid] = valid ? (pv - yb[o * kHeadRows + tid]) * scale : 0.f;
    }
  }
  for (int l = nl; l >= 1; --l) {
    __syncthreads();
    const int wo = g.w[l];
    const float* dz = dzb + cur * a.maxw * kHeadRows;
    // bias gradient: the sum over the 64 rows, in order
    for (int o = tid; o < wo; o += kHeadRows) {
      float s = 0.f;
      for (int rr = 0; rr < kHeadRows; ++rr) s += dz[o * kHeadRows + rr];
      // (the correlation does not change with a shift of p: the output bias' gradient is identically zero,
      // and is written as such rather than as the rounding residue of the sum)
      if constexpr (PP == 2) gp[g.off_b[l - 1] + o] = l == nl ? 0.f : s;
      else gp[g.off_b[l - 1] + o] = s;
    }
    if (l == 1) {
      if (valid)
        for (int j = 0; j < wo; ++j) a.dz1[(long long)j * g.batch + r] = dz[j * kHeadRows + tid];
      break;
    }
    const int wi = g.w[l - 1];
    const float* in = act + a.act_off[l - 1];
    for (int idx = tid; idx < wi * wo; idx += kHeadRows) {
      const int i = idx / wo, o = idx - i * wo;
      float s = 0.f;
      for (int rr = 0; rr < kHeadRows; ++rr) s = fmaf(in[i * kHeadRows + rr], dz[o * kHeadRows + rr], s);
      gp[g.off_w[l - 1] + idx] = s;
    }
    // dA_{l-1} = dZ_l W_l^T through the ReLU (ReLU'(0) = 0: the activation is 0 exactly where z <= 0)
    const float* W = prm + g.off_w[l - 1];
    float* dn = dzb + (cur ^ 1) * a.maxw * kHeadRows;
    for (int i = 0; i < wi; ++i) {
      float s = 0.f;
      for (int o = 0; o < wo; ++o) s = fmaf(W[i * wo + o], dz[o * kHeadRows + tid], s);
      dn[i * kHeadRows + tid] = in[i * kHeadRows + tid] > 0.f ? s : 0.f;
    }
    cur ^= 1;
  }
}

template <int PP>
__global__ __launch_bounds__(kHeadRows) void mlp_head_kernel(HeadArgs a) {
  mlp_head_body<PP>(a, a.at);
}

// ---- many models in one launch (td_dnn_train_many, td_clf_train_many): blockIdx.y = model --------------------------------------
// A model's entry of the device table: the arguments its own launches of a single fit would carry (their `at`
// is not read), and what derives `at` from the launch index.  Models share x, y and the architecture; each has
// its own stream (stream_offs, n_rows), parameters, state, scratch, optimizer settings and row tables.
struct ManyModel {
  SlabArgs slab;
  HeadArgs head;
  RowEntry* rows[2];      // row tables of even / odd epochs (in order: rows[0] serves every epoch)
  const float* lr_t;      // Adam: [total] the learning rate of every update of the call, from the host (else null)
  float lr;               // RMSprop: the learning rate of every update
  double* stats;          // [epochs][max_steps][nstat]
  int steps, total;       // steps per epoch of this model; epochs x steps
  int max_steps, nstat;
};

// Round t of the call runs this model's step t (epoch t / steps, step t % steps, while t < total) forward and
// applies the update of its step t - 1, exactly the pair a single fit's launch t carries.  False: nothing to do
// (a model with fewer steps than the call's longest has finished).
__device__ __forceinline__ bool mlp_many_step(const ManyModel& m, int t, SlabStep* st) {
  const bool cur = t < m.total, prev = t >= 1 && t - 1 < m.total;
  if (!cur && !prev) return false;
  const int shuffle = m.slab.g.shuffle;
  st->cur_epoch = st->cur_step = st->prev_epoch = st->prev_step = -1;
  st->stats_out = nullptr;
  st->lr = 0.f;
  st->prev_rows = st->cur_rows = m.rows[0];
  if (cur) {
    st->cur_epoch = t / m.steps;
    st->cur_step = t - st->cur_epoch * m.steps;
    if (shuffle) st->cur_rows = m.rows[st->cur_epoch & 1];
  }
  if (prev) {
    st->prev_epoch = (t - 1) / m.steps;
    st->prev_step = t - 1 - st->prev_epoch * m.steps;
    if (shuffle) st->prev_rows = m.rows[st->prev_epoch & 1];
    st->stats_out = m.stats + (long long)m.nstat * ((long long)st->prev_epoch * m.max_steps + st->prev_step);
    st->lr = m.lr_t ? m.lr_t[t - 1] : m.lr;
  }
  return true;
}

template <int NJ>
__global__ __launch_bounds__(kSlabThreads) void mlp_slab_many_kernel(const ManyModel* __restrict__ tab, int t) {
  const ManyModel& m = tab[blockIdx.y];
  SlabStep st;
  if (!mlp_many_step(m, t, &st)) return;
  mlp_slab_body<NJ>(m.slab, st);
}

__global__ __launch_bounds__(256) void mlp_z1_many_kernel(const ManyModel* __restrict__ tab, int t) {
  const ManyModel& m = tab[blockIdx.y];
  if (t >= m.total) return;
  const MlpGeom& g = m.head.g;
  const int step = t % m.steps;
  mlp_z1_body(m.head.zpart, m.head.nslices, g.w[1], g.batch, mlp_rows_in_step(g, step), m.head.params + g.off_b[0],
              const_cast<float*>(m.head.z1));
}

template <int PP>
__global__ __launch_bounds__(kHeadRows) void mlp_head_many_kernel(const ManyModel* __restrict__ tab, int t) {
  const ManyModel& m = tab[blockIdx.y];
  if (t >= m.total) return;
  HeadStep st;
  st.epoch = t / m.steps;
  st.step = t - st.epoch * m.steps;
  st.rows_tab = m.rows[m.head.g.shuffle ? st.epoch & 1 : 0];
  mlp_head_body<PP>(m.head, st);
}

struct MlpPlan {
  MlpGeom g;
  int ks = 0, nslices = 0, n_small_wg = 0, n_head = 0, nj = 0;
  size_t head_lds = 0;
  int act_off[kMlpMaxHidden + 2] = {};
  int act_floats = 0, maxw = 0;
};

// What a caller passes, as the prototypes of include/td_hotpath.h name it.  Every exported entry point fills one
// and calls mlp_train / mlp_grad / mlp_forward.
struct MlpView {
  const float* x;
  int64_t ldx;
  int c, pre, post;
};

struct MlpCall {
  MlpView v1, v2;                 // v2.x == nullptr: no second view
  const int64_t* file_offsets;    // host
  int num_files, input_offset;
  const int64_t* rows_used;       // host, or nullptr
  const float* y;
  int64_t ldy;
  int d;
  const int* hidden;              // host
  int num_hidden;
  int batch_rows;
  int loss;                       // 0 = mse, 1 = the Pearson correlation loss
  bool classifier;                // td_mlpc_*: the second view is required; sigmoid output, binary cross-entropy
};

// An entry point's arguments as an MlpCall, group by group in the struct's order: the first view, the second ({}: a
// regressor has none), the files, the targets, the network, the step, the loss and the family.
MlpCall mlp_call(const MlpView& v1, const MlpView& v2, const int64_t* offsets, int num_files, int input_offset,
                 const int64_t* rows_used, const float* y, int64_t ldy, int d, const int* hidden, int num_hidden,
                 int batch_rows, int loss, bool classifier) {
  return {v1, v2, offsets, num_files, input_offset, rows_used, y, ldy, d, hidden, num_hidden, batch_rows, loss,
          classifier};
}

int mlp_check_and_plan(td_handle* h, const char* fn, const MlpCall& a, MlpPlan* plan) {
  const MlpView &v1 = a.v1, &v2 = a.v2;
  const int64_t* offs = a.file_offsets;
  const int nf = a.num_files, c = v1.c, d = a.d, num_hidden = a.num_hidden, batch = a.batch_rows;
  if (!h) return td_fail(h, TD_ERR_INVALID, "%s: NULL handle", fn);
  TD_REQUIRE(h, v1.x && offs && nf >= 1, "%s: NULL argument or no files", fn);
  TD_REQUIRE(h, c >= 1 && v1.pre >= 0 && v1.post >= 0, "%s: bad sizes", fn);
  const int64_t lags = (int64_t)v1.pre + 1 + v1.post;
  TD_REQUIRE(h, lags <= kMlpMaxLags, "%s: pre + 1 + post = %lld exceeds %d", fn, (long long)lags, kMlpMaxLags);
  TD_REQUIRE(h, c <= kMlpMaxC || lags == 1, "%s: %d channels exceed %d (only context-free input may be wider)", fn,
             c, kMlpMaxC);
  TD_REQUIRE(h, c * lags <= kMlpMaxK, "%s: %lld lagged inputs exceed %d", fn, (long long)(c * lags), kMlpMaxK);
  TD_REQUIRE(h, v1.ldx >= c, "%s: leading dimension of x too small", fn);
  int64_t k2 = 0;
  if (a.classifier) {
    TD_REQUIRE(h, v2.x, "%s: NULL second input", fn);
    TD_REQUIRE(h, v2.c >= 1 && v2.pre >= 0 && v2.post >= 0, "%s: bad sizes of the second input", fn);
    const int64_t lags2 = (int64_t)v2.pre + 1 + v2.post;
    TD_REQUIRE(h, lags2 <= kMlpMaxLags, "%s: pre2 + 1 + post2 = %lld exceeds %d", fn, (long long)lags2, kMlpMaxLags);
    TD_REQUIRE(h, v2.c <= kMlpMaxC || lags2 == 1,
               "%s: %d channels of the second input exceed %d (only context-free input may be wider)", fn, v2.c,
               kMlpMaxC);
    k2 = v2.c * lags2;
    TD_REQUIRE(h, k2 <= kMlpMaxK && c * lags + k2 <= kMlpMaxK, "%s: %lld lagged inputs of both views exceed %d", fn,
               (long long)(c * lags + k2), kMlpMaxK);
    TD_REQUIRE(h, v2.ldx >= v2.c, "%s: leading dimension of x2 too small", fn);
  }
  TD_REQUIRE(h, num_hidden >= 0 && num_hidden <= kMlpMaxHidden, "%s: %d hidden layers (at most %d)", fn, num_hidden,
             kMlpMaxHidden);
  TD_REQUIRE(h, num_hidden == 0 || a.hidden, "%s: NULL hidden widths", fn);
  for (int i = 0; i < num_hidden; ++i)
    TD_REQUIRE(h, a.hidden[i] >= 1 && a.hidden[i] <= kMlpMaxWidth, "%s: hidden layer of %d units (1 .. %d)", fn,
               a.hidden[i], kMlpMaxWidth);
  TD_REQUIRE(h, d >= 1 && d <= kMlpMaxD, "%s: %d outputs (1 .. %d)", fn, d, kMlpMaxD);
  TD_REQUIRE(h, batch >= 1 && batch <= kFwdChunk, "%s: batch of %d rows", fn, batch);
  TD_REQUIRE(h, offs[0] == 0, "%s: file offsets must start at 0", fn);
  for (int f = 0; f < nf; ++f) TD_REQUIRE(h, offs[f + 1] >= offs[f], "%s: file offsets decrease", fn);
  TD_REQUIRE(h, offs[nf] < (1LL << 31), "%s: more than 2^31 rows", fn);
  TD_REQUIRE(h, a.loss == 0 || a.loss == 1, "%s: loss %d (0 = mse, 1 = Pearson)", fn, a.loss);
  MlpGeom& g = plan->g;
  memset(&g, 0, sizeof(g));
  g.x = v1.x; g.ldx = v1.ldx; g.nf = nf;
  g.c = c; g.pre = v1.pre; g.lags = (int)lags; g.k = (int)(c * lags + k2);
  g.k1 = (int)(c * lags);
  g.c2 = 1;
  if (a.classifier) {
    g.x2 = v2.x; g.ldx2 = v2.ldx; g.c2 = v2.c; g.pre2 = v2.pre;
    g.bce = 1;
  }
  g.pearson = a.loss;
  g.dx = a.input_offset > 0 ? a.input_offset : 0;
  g.dy = a.input_offset < 0 ? -a.input_offset : 0;
  g.dxy = g.dy - g.dx;
  g.nl = num_hidden + 1;
  g.w[0] = g.k;
  for (int i = 0; i < num_hidden; ++i) g.w[i + 1] = a.hidden[i];
  g.w[g.nl] = d;
  int at = 0;
  for (int l = 1; l <= g.nl; ++l) {
    g.off_w[l - 1] = at; at += g.w[l - 1] * g.w[l];
    g.off_b[l - 1] = at; at += g.w[l];
  }
  g.n_params = at;
  g.small0 = g.k * g.w[1];
  g.n_small = at - g.small0;
  g.batch = batch;
  plan->ks = (int)td_round_up(td_ceil_div(g.k, 64), 4);
  plan->ks = plan->ks > kSlabMaxKs ? kSlabMaxKs : plan->ks;
  plan->nslices = (int)td_ceil_div(g.k, plan->ks);
  plan->n_small_wg = (int)td_ceil_div(g.n_small, kSlabThreads);
  plan->n_head = (int)td_ceil_div(batch, kHeadRows);
  const int w1 = g.w[1];
  plan->nj = w1 <= 4 ? 4 : w1 <= 8 ? 8 : w1 <= 16 ? 16 : w1 <= 24 ? 24 : w1 <= 32 ? 32 : w1 <= 48 ? 48 : 64;
  int maxw = 0, off = 0;
  for (int l = 1; l <= g.nl; ++l) {
    plan->act_off[l] = off;
    off += g.w[l] * kHeadRows;
    maxw = g.w[l] > maxw ? g.w[l] : maxw;
  }
  plan->act_floats = off;
  plan->maxw = maxw;
  plan->head_lds = sizeof(float) * ((size_t)off + 2 * (size_t)maxw * kHeadRows + (size_t)d * kHeadRows + g.n_small);
  return TD_OK;
}

// The instantiations of the two kernel families as the host picks them, each table next to its launcher -- a single
// fit's launches (One), and the many-model launches with the models in blockIdx.y (Many): the slab kernel whose tile
// holds plan.nj first-layer units (kSlabNj), and the head kernel of a pass (0: mse and cross-entropy; 1, 2: Pearson).
constexpr int kSlabNj[7] = {4, 8, 16, 24, 32, 48, 64};
constexpr void (*kSlabOne[7])(SlabArgs) = {
    mlp_slab_kernel<4>,  mlp_slab_kernel<8>,  mlp_slab_kernel<16>, mlp_slab_kernel<24>,
    mlp_slab_kernel<32>, mlp_slab_kernel<48>, mlp_slab_kernel<64>};

template <typename K, typename... Args>
int mlp_launch_slab_of(td_handle* h, const MlpPlan& plan, K* const (&family)[7], dim3 grid, const Args&... args) {
  // (the search stops in front of the last entry: an nj that is none of the first six takes the widest kernel, 64)
  const int i = (int)(std::find(kSlabNj, kSlabNj + 6, plan.nj) - kSlabNj);
  hipLaunchKernelGGL(family[i], grid, dim3(kSlabThreads), 0, h->stream, args...);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

int mlp_launch_slab(td_handle* h, const MlpPlan& plan, const SlabArgs& a, bool with_small) {
  return mlp_launch_slab_of(h, plan, kSlabOne, dim3(plan.nslices + (with_small ? plan.n_small_wg : 0)), a);
}

int mlp_launch_head(td_handle* h, const MlpPlan& plan, const HeadArgs& a) {
  const MlpGeom& g = a.g;
  const int rows = (int)std::min<long long>(g.batch, g.n_rows - (long long)a.at.step * g.batch);
  hipLaunchKernelGGL(mlp_z1_kernel, dim3((unsigned)td_ceil_div((int64_t)g.w[1] * g.batch, 256)), dim3(256), 0,
                     h->stream, a.zpart, plan.nslices, g.w[1], g.batch, rows, a.params + g.off_b[0],
                     const_cast<float*>(a.z1));
  if (g.pearson && !a.out) {
    hipLaunchKernelGGL(mlp_head_kernel<1>, dim3(plan.n_head), dim3(kHeadRows), plan.head_lds, h->stream, a);
    if (a.backward)
      hipLaunchKernelGGL(mlp_head_kernel<2>, dim3(plan.n_head), dim3(kHeadRows), plan.head_lds, h->stream, a);
  } else {
    hipLaunchKernelGGL(mlp_head_kernel<0>, dim3(plan.n_head), dim3(kHeadRows), plan.head_lds, h->stream, a);
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

constexpr void (*kHeadOne[3])(HeadArgs) = {mlp_head_kernel<0>, mlp_head_kernel<1>, mlp_head_kernel<2>};

// lets the first `passes` head kernels of a family take kHeadMaxLds of dynamic LDS
template <typename K>
int mlp_raise_head_lds(td_handle* h, K* const (&family)[3], int passes) {
  for (int pp = 0; pp < passes; ++pp)
    TD_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void*>(family[pp]), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  kHeadMaxLds));
  return TD_OK;
}

// Device scratch of a call: working copies of the parameters and optimizer state, the exchange buffers
// between the launches and the offset tables.
struct MlpWork {
  float *params, *state, *zpart, *dz1, *gpart, *z1;
  RowEntry* rows[2];        // row tables of even / odd epochs
  double *spart, *mpart, *lstat;   // (mpart, lstat: the Pearson loss)
  long long *file_offs, *stream_offs;
};

int mlp_work(td_handle* h, const MlpPlan& plan, int nf, MlpWork* w) {
  const MlpGeom& g = plan.g;
  const size_t n_par = td_round_up(g.n_params, 64);
  const size_t n_z = td_round_up((int64_t)plan.nslices * g.w[1] * g.batch, 64);
  const size_t n_dz = td_round_up((int64_t)g.w[1] * g.batch, 64);
  const size_t n_gp = td_round_up((int64_t)plan.n_head * g.n_small, 64);
  const size_t n_sp = td_round_up((int64_t)plan.n_head * 6, 32);
  const size_t n_mp = td_round_up((int64_t)plan.n_head * 5 * kMlpMaxD, 32);
  const size_t n_off = td_round_up((int64_t)nf + 1, 32);
  const size_t n_tab = td_round_up(g.n_rows, 64);
  const size_t n_st = td_round_up(2 * (int64_t)g.n_params, 64);   // Adam keeps two accumulators per parameter
  const size_t bytes = 4 * (n_par + n_st + n_z + 2 * n_dz + n_gp) + 8 * (n_sp + n_mp + 32 + 2 * n_off) + 2 * 16 * n_tab;
  void* base = nullptr;
  TD_TRY(td_scratch(h, bytes, &base));
  char* p = static_cast<char*>(base);
  w->rows[0] = reinterpret_cast<RowEntry*>(p); p += 16 * n_tab;
  w->rows[1] = reinterpret_cast<RowEntry*>(p); p += 16 * n_tab;
  w->spart = reinterpret_cast<double*>(p); p += 8 * n_sp;
  w->mpart = reinterpret_cast<double*>(p); p += 8 * n_mp;
  w->lstat = reinterpret_cast<double*>(p); p += 8 * 32;
  w->file_offs = reinterpret_cast<long long*>(p); p += 8 * n_off;
  w->stream_offs = reinterpret_cast<long long*>(p); p += 8 * n_off;
  w->params = reinterpret_cast<float*>(p); p += 4 * n_par;
  w->state = reinterpret_cast<float*>(p); p += 4 * n_st;
  w->zpart = reinterpret_cast<float*>(p); p += 4 * n_z;
  w->dz1 = reinterpret_cast<float*>(p); p += 4 * n_dz;
  w->z1 = reinterpret_cast<float*>(p); p += 4 * n_dz;
  w->gpart = reinterpret_cast<float*>(p);
  return TD_OK;
}

// the stream's rows per file (rows_used, else the zipped lengths) as offsets
int mlp_stream_offsets(td_handle* h, const char* fn, const MlpCall& a, std::vector<long long>* so) {
  const int64_t off = a.input_offset < 0 ? -(int64_t)a.input_offset : a.input_offset;
  so->assign(a.num_files + 1, 0);
  for (int f = 0; f < a.num_files; ++f) {
    const int64_t n = a.file_offsets[f + 1] - a.file_offsets[f];
    const int64_t z = n - off > 0 ? n - off : 0;
    int64_t u = z;
    if (a.rows_used) {
      TD_REQUIRE(h, a.rows_used[f] >= 0 && a.rows_used[f] <= z, "%s: rows_used[%d] = %lld, the file has %lld rows",
                 fn, f, (long long)a.rows_used[f], (long long)z);
      u = a.rows_used[f];
    }
    (*so)[f + 1] = (*so)[f] + u;
  }
  return TD_OK;
}

int mlp_setup(td_handle* h, MlpPlan* plan, const MlpCall& a, const std::vector<long long>& so, MlpWork* w) {
  const int nf = a.num_files;
  TD_TRY(mlp_work(h, *plan, nf, w));
  TD_TRY(td_upload_async(h, a.file_offsets, sizeof(long long) * (nf + 1), w->file_offs));
  if (!so.empty()) TD_TRY(td_upload_async(h, so.data(), sizeof(long long) * (nf + 1), w->stream_offs));
  plan->g.file_offs = w->file_offs;
  plan->g.stream_offs = so.empty() ? w->file_offs : w->stream_offs;
  return mlp_raise_head_lds(h, kHeadOne, plan->g.pearson ? 3 : 1);
}

void mlp_fill(const MlpPlan& plan, const MlpWork& w, SlabArgs* sa, HeadArgs* ha) {
  memset(sa, 0, sizeof(*sa));
  memset(ha, 0, sizeof(*ha));
  sa->g = plan.g;
  sa->params = w.params; sa->state = w.state;
  sa->zpart = w.zpart; sa->dz1 = w.dz1; sa->gpart = w.gpart; sa->spart = w.spart; sa->lstat = w.lstat;
  sa->ks = plan.ks; sa->nslices = plan.nslices; sa->n_head = plan.n_head;
  sa->at.prev_epoch = sa->at.prev_step = sa->at.cur_epoch = sa->at.cur_step = -1;
  ha->g = plan.g;
  ha->params = w.params; ha->zpart = w.zpart; ha->nslices = plan.nslices;
  ha->dz1 = w.dz1; ha->gpart = w.gpart; ha->spart = w.spart; ha->mpart = w.mpart; ha->lstat = w.lstat;
  for (int l = 0; l < kMlpMaxHidden + 2; ++l) ha->act_off[l] = plan.act_off[l];
  ha->act_floats = plan.act_floats; ha->maxw = plan.maxw;
  ha->z1 = w.z1;
  ha->backward = 1;
  sa->at.prev_rows = sa->at.cur_rows = ha->at.rows_tab = w.rows[0];
}

// the row table of `epoch` into tab (queued)
int mlp_launch_rows(td_handle* h, const MlpGeom& g, int epoch, RowEntry* tab) {
  const long long blocks = std::min<long long>(td_ceil_div(g.n_rows, 256), 4096);
  hipLaunchKernelGGL(mlp_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, g, epoch, tab);
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

// The optimizer of a training call.  RMSprop: lr, b1 = rho, eps.  Adam: lr_t of update t = step0 + 1, ... is
// computed here in double and rounded once, as are 1 - beta_1 and 1 - beta_2.
struct MlpOpt {
  int update;
  double lr, b1, b2, eps;
  int64_t step0;
};

// Adam's lr_t of update `index` of a call (t = step0 + index + 1): double arithmetic, rounded once.  The one
// expression both mlp_train (per launch) and mlp_train_many (its per-model table) use.
float mlp_adam_lr(const MlpOpt& opt, int64_t index) {
  const double t = (double)(opt.step0 + index + 1);
  return (float)(opt.lr * std::sqrt(1.0 - std::pow(opt.b2, t)) / (1.0 - std::pow(opt.b1, t)));
}

// The checks of a training call's settings; model >= 0 names the model of a many-model call in the message.
int mlp_check_opt(td_handle* h, const char* fn, const MlpOpt& opt, int model) {
  char who[24] = "";
  if (model >= 0) snprintf(who, sizeof(who), "model %d: ", model);
  TD_REQUIRE(h, std::isfinite(opt.lr) && std::isfinite(opt.b1) && std::isfinite(opt.b2) && std::isfinite(opt.eps),
             "%s: %snon-finite optimizer setting", fn, who);
  if (opt.update == kUpdAdam)
    TD_REQUIRE(h, opt.b1 >= 0.0 && opt.b1 < 1.0 && opt.b2 >= 0.0 && opt.b2 < 1.0 && opt.step0 >= 0,
               "%s: %sAdam needs 0 <= beta < 1 and step0 >= 0", fn, who);
  return TD_OK;
}

// the update rule and every setting of it but the learning rate (a launch's or a model's own), as the kernels read them
void mlp_set_opt(SlabArgs* sa, const MlpOpt& opt) {
  sa->update = opt.update;
  sa->rho = (float)opt.b1; sa->eps = (float)opt.eps;
  sa->beta2 = (float)opt.b2; sa->omb1 = (float)(1.0 - opt.b1); sa->omb2 = (float)(1.0 - opt.b2);
}

// the visiting order of a stream: seed < 0 in order, else the Feistel bijection of (seed, epoch)
void mlp_set_seed(MlpGeom* g, int64_t seed) {
  g->shuffle = seed >= 0;
  g->seed_lo = (unsigned)((uint64_t)seed & 0xffffffffu);
  g->seed_hi = (unsigned)((uint64_t)seed >> 32);
}

void mlp_set_update(SlabArgs* sa, const MlpOpt& opt, int64_t index) {
  if (opt.update != kUpdAdam) return;
  sa->at.lr = mlp_adam_lr(opt, index);
}

// Checks the call, then queues every launch of it.
int mlp_train(td_handle* h, const char* fn, const MlpCall& a, int epochs, float* params_dev, float* state_dev,
              const MlpOpt& opt, int64_t shuffle_seed, double* stats_dev) {
  MlpPlan plan;
  TD_TRY(mlp_check_and_plan(h, fn, a, &plan));
  const int batch_rows = a.batch_rows;
  const bool update = opt.update != kUpdNone;
  TD_REQUIRE(h, batch_rows <= kMlpMaxB, "%s: batch of %d rows exceeds %d", fn, batch_rows, kMlpMaxB);
  TD_REQUIRE(h, a.y && params_dev && (state_dev || !update) && a.ldy >= a.d, "%s: NULL argument or ldy too small",
             fn);
  TD_REQUIRE(h, epochs >= 0, "%s: negative epoch count", fn);
  TD_TRY(mlp_check_opt(h, fn, opt, -1));
  std::vector<long long> so;
  TD_TRY(mlp_stream_offsets(h, fn, a, &so));
  const long long n_rows = so[a.num_files];
  TD_REQUIRE(h, n_rows >= 1, "%s: no rows to train on", fn);
  const int steps = (int)td_ceil_div(n_rows, batch_rows);
  TD_REQUIRE(h, epochs == 0 || stats_dev, "%s: NULL stats buffer", fn);
  if (epochs == 0) return TD_OK;
  plan.g.y = a.y; plan.g.ldy = a.ldy;
  plan.g.n_rows = n_rows;
  mlp_set_seed(&plan.g, shuffle_seed);
  MlpWork w;
  TD_TRY(mlp_setup(h, &plan, a, so, &w));
  // work on copies: the caller's parameters change only when every launch has been queued
  const size_t pbytes = sizeof(float) * plan.g.n_params;
  const size_t sbytes = opt.update == kUpdAdam ? 2 * pbytes : pbytes;
  TD_HIP(h, hipMemcpyAsync(w.params, params_dev, pbytes, hipMemcpyDeviceToDevice, h->stream));
  if (update) TD_HIP(h, hipMemcpyAsync(w.state, state_dev, sbytes, hipMemcpyDeviceToDevice, h->stream));
  SlabArgs sa;
  HeadArgs ha;
  mlp_fill(plan, w, &sa, &ha);
  mlp_set_opt(&sa, opt);
  sa.at.lr = (float)opt.lr;
  ha.backward = update;
  const int nstat = plan.g.pearson ? 7 : 6;
  int pe = -1, ps = -1;
  for (int e = 0; e < epochs; ++e) {
    // in order, one table serves every epoch; shuffled, epochs alternate between two (the first step of
    // epoch e still updates with the last rows of epoch e - 1)
    RowEntry* tab = plan.g.shuffle ? w.rows[e & 1] : w.rows[0];
    if (e == 0 || plan.g.shuffle) TD_TRY(mlp_launch_rows(h, plan.g, e, tab));
    sa.at.prev_rows = sa.at.cur_rows;
    sa.at.cur_rows = ha.at.rows_tab = tab;
    for (int s = 0; s < steps; ++s) {
      if (s == 1) sa.at.prev_rows = tab;
      sa.at.prev_epoch = pe; sa.at.prev_step = ps; sa.at.cur_epoch = e; sa.at.cur_step = s;
      sa.at.stats_out = ps >= 0 ? stats_dev + nstat * ((long long)pe * steps + ps) : nullptr;
      if (ps >= 0) mlp_set_update(&sa, opt, (int64_t)pe * steps + ps);
      TD_TRY(mlp_launch_slab(h, plan, sa, ps >= 0));
      ha.at.epoch = e; ha.at.step = s;
      TD_TRY(mlp_launch_head(h, plan, ha));
      pe = e; ps = s;
    }
  }
  sa.at.prev_epoch = pe; sa.at.prev_step = ps; sa.at.cur_epoch = sa.at.cur_step = -1;
  sa.at.prev_rows = sa.at.cur_rows;
  sa.at.stats_out = stats_dev + nstat * ((long long)pe * steps + ps);
  mlp_set_update(&sa, opt, (int64_t)pe * steps + ps);
  TD_TRY(mlp_launch_slab(h, plan, sa, true));
  if (update) {
    TD_HIP(h, hipMemcpyAsync(params_dev, w.params, pbytes, hipMemcpyDeviceToDevice, h->stream));
    TD_HIP(h, hipMemcpyAsync(state_dev, w.state, sbytes, hipMemcpyDeviceToDevice, h->stream));
  }
  return TD_OK;
}

int mlp_grad(td_handle* h, const char* fn, const MlpCall& a, int batch_index, const float* params_dev,
             float* grad_dev, double* stats_dev) {
  MlpPlan plan;
  TD_TRY(mlp_check_and_plan(h, fn, a, &plan));
  TD_REQUIRE(h, a.batch_rows <= kMlpMaxB, "%s: batch of %d rows exceeds %d", fn, a.batch_rows, kMlpMaxB);
  TD_REQUIRE(h, a.y && params_dev && grad_dev && stats_dev && a.ldy >= a.d, "%s: NULL argument or ldy too small",
             fn);
  std::vector<long long> so;
  TD_TRY(mlp_stream_offsets(h, fn, a, &so));
  const long long n_rows = so[a.num_files];
  TD_REQUIRE(h, batch_index >= 0 && (long long)batch_index * a.batch_rows < n_rows,
             "%s: minibatch %d is outside the stream's %lld rows", fn, batch_index, n_rows);
  plan.g.y = a.y; plan.g.ldy = a.ldy;
  plan.g.n_rows = n_rows;
  MlpWork w;
  TD_TRY(mlp_setup(h, &plan, a, so, &w));
  TD_HIP(h, hipMemcpyAsync(w.params, params_dev, sizeof(float) * plan.g.n_params, hipMemcpyDeviceToDevice,
                           h->stream));
  SlabArgs sa;
  HeadArgs ha;
  mlp_fill(plan, w, &sa, &ha);
  // the training step's launches: forward, head, and the update launch writing the gradient instead
  TD_TRY(mlp_launch_rows(h, plan.g, 0, w.rows[0]));
  sa.at.cur_epoch = 0; sa.at.cur_step = batch_index;
  TD_TRY(mlp_launch_slab(h, plan, sa, false));
  ha.at.epoch = 0; ha.at.step = batch_index;
  TD_TRY(mlp_launch_head(h, plan, ha));
  sa.at.cur_epoch = sa.at.cur_step = -1;
  sa.at.prev_epoch = 0; sa.at.prev_step = batch_index;
  sa.grad_out = grad_dev;
  sa.at.stats_out = stats_dev;
  TD_TRY(mlp_launch_slab(h, plan, sa, true));
  return TD_OK;
}

// (a.batch_rows: the rows of a chunk, kFwdChunk)
int mlp_forward(td_handle* h, const char* fn, const MlpCall& a, const float* params_dev, float* out_dev,
                int64_t ldout) {
  MlpPlan plan;
  TD_TRY(mlp_check_and_plan(h, fn, a, &plan));
  TD_REQUIRE(h, params_dev && out_dev && ldout >= a.d, "%s: NULL argument or ldout too small", fn);
  const long long n_rows = a.file_offsets[a.num_files];
  if (n_rows == 0) return TD_OK;
  // every row of x: output row file_offsets[f] + t is frame t of file f (as td_predict_fir)
  plan.g.fwd = 1;
  plan.g.n_rows = n_rows;
  MlpWork w;
  TD_TRY(mlp_setup(h, &plan, a, std::vector<long long>(), &w));
  SlabArgs sa;
  HeadArgs ha;
  mlp_fill(plan, w, &sa, &ha);
  sa.params = const_cast<float*>(params_dev);   // read only: no update phase
  ha.params = params_dev;
  ha.out = out_dev; ha.ldout = ldout; ha.backward = 0;
  TD_TRY(mlp_launch_rows(h, plan.g, 0, w.rows[0]));
  const int chunks = (int)td_ceil_div(n_rows, kFwdChunk);
  for (int s = 0; s < chunks; ++s) {
    sa.at.cur_epoch = 0; sa.at.cur_step = s;
    TD_TRY(mlp_launch_slab(h, plan, sa, false));
    ha.at.epoch = 0; ha.at.step = s;
    TD_TRY(mlp_launch_head(h, plan, ha));
  }
  return TD_OK;
}

// ---- td_dnn_train_many, td_clf_train_many ---------------------------------------------------------------------
struct ManyCall {
  int num_models;
  const int64_t* rows_used;        // host [num_models][num_files]
  float* const* params;            // host [num_models] device pointers
  float* const* state;             // (score only: may be null, as may its entries)
  const MlpOpt* opt;               // host [num_models]: one update rule for all, every model its own settings
  const int64_t* shuffle_seed;     // host [num_models], < 0: in order (score only: not read)
};

// The per-model settings of a many-model call: model m's from the arrays of an entry point (lr null: all zero, the
// call only scores; b2 / step0 null: the rule has none), and one entry even without models, so that opt[0] names
// the rule.
template <typename T>
std::vector<MlpOpt> mlp_opts(int rule, int num_models, const T* lr, const T* b1, const T* b2, const T* eps,
                             const int64_t* step0) {
  std::vector<MlpOpt> opt(std::max(num_models, 1), {rule, 0.0, 0.0, 0.0, 0.0, 0});
  for (int m = 0; lr && m < num_models; ++m)
    opt[m] = {rule, lr[m], b1[m], b2 ? b2[m] : 0.0, eps[m], step0 ? step0[m] : 0};
  return opt;
}

// a call's scratch, sized on a first pass (base null) and handed out on a second
struct MlpBump {
  char* base;
  size_t at;
  template <typename T>
  T* take(size_t n) {
    at = td_round_up(at, 256);
    T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
    at += n * sizeof(T);
    return p;
  }
};

constexpr void (*kSlabMany[7])(const ManyModel*, int) = {
    mlp_slab_many_kernel<4>,  mlp_slab_many_kernel<8>,  mlp_slab_many_kernel<16>, mlp_slab_many_kernel<24>,
    mlp_slab_many_kernel<32>, mlp_slab_many_kernel<48>, mlp_slab_many_kernel<64>};

int mlp_launch_head_many(td_handle* h, const MlpPlan& plan, int num_models, const ManyModel* tab, int t) {
  const MlpGeom& g = plan.g;
  hipLaunchKernelGGL(mlp_z1_many_kernel, dim3((unsigned)td_ceil_div((int64_t)g.w[1] * g.batch, 256), num_models),
                     dim3(256), 0, h->stream, tab, t);
  const dim3 grid(plan.n_head, num_models), block(kHeadRows);
  if (g.pearson) {
    hipLaunchKernelGGL(mlp_head_many_kernel<1>, grid, block, plan.head_lds, h->stream, tab, t);
    hipLaunchKernelGGL(mlp_head_many_kernel<2>, grid, block, plan.head_lds, h->stream, tab, t);
  } else {
    hipLaunchKernelGGL(mlp_head_many_kernel<0>, grid, block, plan.head_lds, h->stream, tab, t);
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

constexpr void (*kHeadMany[3])(const ManyModel*, int) = {mlp_head_many_kernel<0>, mlp_head_many_kernel<1>,
                                                         mlp_head_many_kernel<2>};

// mlp_train for num_models models at once (regressors on RMSprop, classifiers on Adam or scored only, kUpdNone):
// every check of every model first, then working copies, the rounds of launches (round t = launch t of every
// model's own fit, models in blockIdx.y) and the commit.
int mlp_train_many(td_handle* h, const char* fn, const MlpCall& a, int epochs, const ManyCall& mc, double* stats_dev) {
  MlpPlan plan;
  TD_TRY(mlp_check_and_plan(h, fn, a, &plan));
  const int nm = mc.num_models, nf = a.num_files, batch_rows = a.batch_rows;
  TD_REQUIRE(h, batch_rows <= kMlpMaxB, "%s: batch of %d rows exceeds %d", fn, batch_rows, kMlpMaxB);
  TD_REQUIRE(h, nm >= 1 && nm <= TD_DNN_MANY_MAX_MODELS, "%s: %d models (1 .. %d a call)", fn, nm,
             TD_DNN_MANY_MAX_MODELS);
  const int rule = mc.opt ? mc.opt[0].update : kUpdNone;
  const bool update = rule != kUpdNone, adam = rule == kUpdAdam;
  TD_REQUIRE(h, a.y && a.ldy >= a.d && mc.rows_used && mc.params && (mc.state || !update) && mc.opt &&
                    (mc.shuffle_seed || !update), "%s: NULL argument or ldy too small", fn);
  TD_REQUIRE(h, epochs >= 0, "%s: negative epoch count", fn);
  TD_REQUIRE(h, update || epochs == 1, "%s: scoring is one pass (epochs = 1), not %d", fn, epochs);
  std::vector<std::vector<long long>> so(nm);
  int max_steps = 0;
  long long max_total = 0;
  for (int m = 0; m < nm; ++m) {
    TD_REQUIRE(h, mc.params[m] && (!update || mc.state[m]), "%s: model %d: NULL parameters or state", fn, m);
    // (scoring writes to no model, so two entries may score one model on different files)
    for (int j = 0; update && j < m; ++j)
      TD_REQUIRE(h, mc.params[j] != mc.params[m] && mc.state[j] != mc.state[m],
                 "%s: models %d and %d share their parameters or state", fn, j, m);
    TD_TRY(mlp_check_opt(h, fn, mc.opt[m], m));
    MlpCall am = a;
    am.rows_used = mc.rows_used + (size_t)m * nf;
    TD_TRY(mlp_stream_offsets(h, fn, am, &so[m]));
    const long long n_rows = so[m][nf];
    TD_REQUIRE(h, n_rows >= 1, "%s: model %d: no rows to train on", fn, m);
    const long long steps = td_ceil_div(n_rows, batch_rows);
    TD_REQUIRE(h, (long long)epochs * steps < (1LL << 31) - 1, "%s: model %d: %lld launches", fn, m,
               (long long)epochs * steps);
    max_steps = std::max<int>(max_steps, (int)steps);
    max_total = std::max<long long>(max_total, (long long)epochs * steps);
  }
  TD_REQUIRE(h, epochs == 0 || stats_dev, "%s: NULL stats buffer", fn);
  if (epochs == 0) return TD_OK;
  MlpGeom& g = plan.g;
  g.y = a.y; g.ldy = a.ldy;
  const int nstat = g.pearson ? 7 : 6;
  const size_t n_off = nf + 1;
  const auto seed_of = [&](int m) -> int64_t { return update ? mc.shuffle_seed[m] : -1; };
  // Adam: lr_t of every update of the call, model after model (model m's at lr_at[m])
  std::vector<size_t> lr_at(nm + 1, 0);
  for (int m = 0; adam && m < nm; ++m)
    lr_at[m + 1] = lr_at[m] + (size_t)(epochs * td_ceil_div(so[m][nf], batch_rows));
  // the scratch: the table, the offsets, then every model's own block
  std::vector<MlpWork> work(nm);
  float* lr_dev = nullptr;
  long long* so_dev = nullptr;
  ManyModel* tab_dev = nullptr;
  MlpBump bump = {nullptr, 0};
  for (int pass = 0; pass < 2; ++pass) {
    if (pass) {
      void* base = nullptr;
      TD_TRY(td_scratch(h, bump.at, &base));
      bump = {static_cast<char*>(base), 0};
    }
    tab_dev = bump.take<ManyModel>(nm);
    so_dev = bump.take<long long>((size_t)(nm + 1) * n_off);     // the file offsets, then every model's stream
    lr_dev = bump.take<float>(lr_at[nm]);
    for (int m = 0; m < nm; ++m) {
      MlpWork& w = work[m];
      const long long n_rows = so[m][nf];
      w.rows[0] = bump.take<RowEntry>(n_rows);
      w.rows[1] = seed_of(m) >= 0 ? bump.take<RowEntry>(n_rows) : w.rows[0];
      w.spart = bump.take<double>((size_t)plan.n_head * 6);
      w.mpart = bump.take<double>((size_t)plan.n_head * 5 * kMlpMaxD);
      w.lstat = bump.take<double>(1);
      w.params = bump.take<float>(g.n_params);
      w.state = bump.take<float>(adam ? 2 * (size_t)g.n_params : g.n_params);   // Adam: m, then v
      w.zpart = bump.take<float>((size_t)plan.nslices * g.w[1] * g.batch);
      w.dz1 = bump.take<float>((size_t)g.w[1] * g.batch);
      w.z1 = bump.take<float>((size_t)g.w[1] * g.batch);
      w.gpart = bump.take<float>((size_t)plan.n_head * g.n_small);
      w.file_offs = so_dev;
      w.stream_offs = so_dev + (size_t)(m + 1) * n_off;
    }
  }
  std::vector<long long> so_host((size_t)(nm + 1) * n_off);
  for (size_t f = 0; f < n_off; ++f) so_host[f] = a.file_offsets[f];
  for (int m = 0; m < nm; ++m) std::copy(so[m].begin(), so[m].end(), so_host.begin() + (size_t)(m + 1) * n_off);
  std::vector<ManyModel> tab(nm);
  for (int m = 0; m < nm; ++m) {
    const MlpWork& w = work[m];
    MlpPlan pm = plan;
    pm.g.file_offs = w.file_offs; pm.g.stream_offs = w.stream_offs;
    pm.g.n_rows = so[m][nf];
    mlp_set_seed(&pm.g, seed_of(m));
    ManyModel& t = tab[m];
    memset(&t, 0, sizeof(t));
    mlp_fill(pm, w, &t.slab, &t.head);
    mlp_set_opt(&t.slab, mc.opt[m]);
    t.head.backward = update;
    t.lr = (float)mc.opt[m].lr; t.lr_t = adam ? lr_dev + lr_at[m] : nullptr;
    t.rows[0] = w.rows[0]; t.rows[1] = w.rows[1];
    t.steps = (int)td_ceil_div(pm.g.n_rows, batch_rows);
    t.total = epochs * t.steps;
    t.max_steps = max_steps; t.nstat = nstat;
    t.stats = stats_dev + (size_t)m * epochs * max_steps * nstat;
  }
  TD_TRY(td_upload_async(h, so_host.data(), sizeof(long long) * so_host.size(), so_dev));
  TD_TRY(td_upload_async(h, tab.data(), sizeof(ManyModel) * nm, tab_dev));
  if (adam) {
    // lr_t of update k of model m, k = 0 .. total_m - 1: mlp_train's own expression on the host (the device's pow
    // is not the host's), read by the update of step k
    std::vector<float> lr_t(lr_at[nm]);
    for (int m = 0; m < nm; ++m)
      for (int k = 0; k < tab[m].total; ++k) lr_t[lr_at[m] + k] = mlp_adam_lr(mc.opt[m], k);
    TD_TRY(td_upload_async(h, lr_t.data(), sizeof(float) * lr_t.size(), lr_dev));
  }
  TD_TRY(mlp_raise_head_lds(h, kHeadMany, 3));
  // work on copies: the callers' parameters change only when every launch has been queued
  const size_t pbytes = sizeof(float) * g.n_params, sbytes = adam ? 2 * pbytes : pbytes;
  for (int m = 0; m < nm; ++m) {
    TD_HIP(h, hipMemcpyAsync(work[m].params, mc.params[m], pbytes, hipMemcpyDeviceToDevice, h->stream));
    if (update) TD_HIP(h, hipMemcpyAsync(work[m].state, mc.state[m], sbytes, hipMemcpyDeviceToDevice, h->stream));
    if (!tab[m].slab.g.shuffle) TD_TRY(mlp_launch_rows(h, tab[m].slab.g, 0, work[m].rows[0]));
  }
  for (long long t = 0; t <= max_total; ++t) {
    // shuffled: the table of a model's epoch e, in front of the round that starts it (its other table still
    // serves the update of the last step of epoch e - 1)
    for (int m = 0; m < nm; ++m)
      if (tab[m].slab.g.shuffle && t < tab[m].total && t % tab[m].steps == 0) {
        const int e = (int)(t / tab[m].steps);
        TD_TRY(mlp_launch_rows(h, tab[m].slab.g, e, work[m].rows[e & 1]));
      }
    TD_TRY(mlp_launch_slab_of(h, plan, kSlabMany, dim3(plan.nslices + plan.n_small_wg, nm), tab_dev, (int)t));
    if (t < max_total) TD_TRY(mlp_launch_head_many(h, plan, nm, tab_dev, (int)t));
  }
  for (int m = 0; update && m < nm; ++m) {
    TD_HIP(h, hipMemcpyAsync(mc.params[m], work[m].params, pbytes, hipMemcpyDeviceToDevice, h->stream));
    TD_HIP(h, hipMemcpyAsync(mc.state[m], work[m].state, sbytes, hipMemcpyDeviceToDevice, h->stream));
  }
  return TD_OK;
}

}  // namespace

// The exported entry points: each packs its arguments with mlp_call and passes its own name for the messages.
int td_mlp_train(td_handle* h, const float* x_dev, int64_t ldx, const int64_t* file_offsets_host, int num_files,
                 int c, int pre, int post, int input_offset, const int64_t* rows_used_host, const float* y_dev,
                 int64_t ldy, int d, const int* hidden_host, int num_hidden, int batch_rows, int epochs,
                 float* params_dev, float* state_dev, float lr, float rho, float eps, int64_t shuffle_seed,
                 double* stats_dev) {
  const MlpCall a = mlp_call({x_dev, ldx, c, pre, post}, {}, file_offsets_host, num_files, input_offset,
                             rows_used_host, y_dev, ldy, d, hidden_host, num_hidden, batch_rows, 0, false);
  return mlp_train(h, "td_mlp_train", a, epochs, params_dev, state_dev, {kUpdRmsprop, lr, rho, 0.0, eps, 0},
                   shuffle_seed, stats_dev);
}

int td_mlp_train_loss(td_handle* h, const float* x_dev, int64_t ldx, const int64_t* file_offsets_host,
                      int num_files, int c, int pre, int post, int input_offset, const int64_t* rows_used_host,
                      const float* y_dev, int64_t ldy, int d, const int* hidden_host, int num_hidden,
                      int batch_rows, int epochs, float* params_dev, float* state_dev, float lr, float rho,
                      float eps, int64_t shuffle_seed, double* stats_dev, int loss) {
  const MlpCall a = mlp_call({x_dev, ldx, c, pre, post}, {}, file_offsets_host, num_files, input_offset,
                             rows_used_host, y_dev, ldy, d, hidden_host, num_hidden, batch_rows, loss, false);
  return mlp_train(h, "td_mlp_train_loss", a, epochs, params_dev, state_dev, {kUpdRmsprop, lr, rho, 0.0, eps, 0},
                   shuffle_seed, stats_dev);
}

int td_mlp_grad(td_handle* h, const float* x_dev, int64_t ldx, const int64_t* file_offsets_host, int num_files,
                int c, int pre, int post, int input_offset, const int64_t* rows_used_host, const float* y_dev,
                int64_t ldy, int d, const int* hidden_host, int num_hidden, int batch_rows, int batch_index,
                const float* params_dev, float* grad_dev, double* stats_dev) {
  const MlpCall a = mlp_call({x_dev, ldx, c, pre, post}, {}, file_offsets_host, num_files, input_offset,
                             rows_used_host, y_dev, ldy, d, hidden_host, num_hidden, batch_rows, 0, false);
  return mlp_grad(h, "td_mlp_grad", a, batch_index, params_dev, grad_dev, stats_dev);
}

int td_mlp_grad_loss(td_handle* h, const float* x_dev, int64_t ldx, const int64_t* file_offsets_host,
                     int num_files, int c, int pre, int post, int input_offset, const int64_t* rows_used_host,
                     const float* y_dev, int64_t ldy, int d, const int* hidden_host, int num_hidden, int batch_rows,
                     int batch_index, const float* params_dev, float* grad_dev, double* stats_dev, int loss) {
  const MlpCall a = mlp_call({x_dev, ldx, c, pre, post}, {}, file_offsets_host, num_files, input_offset,
                             rows_used_host, y_dev, ldy, d, hidden_host, num_hidden, batch_rows, loss, false);
  return mlp_grad(h, "td_mlp_grad_loss", a, batch_index, params_dev, grad_dev, stats_dev);
}

int td_mlp_forward(td_handle* h, const float* x_dev, int64_t ldx, const int64_t* file_offsets_host, int num_files,
                   int c, int pre, int post, int input_offset, int d, const int* hidden_host, int num_hidden,
                   const float* params_dev, float* out_dev, int64_t ldout) {
  const MlpCall a = mlp_call({x_dev, ldx, c, pre, post}, {}, file_offsets_host, num_files, input_offset, nullptr,
                             nullptr, 0, d, hidden_host, num_hidden, kFwdChunk, 0, false);
  return mlp_forward(h, "td_mlp_forward", a, params_dev, out_dev, ldout);
}

int td_mlpc_train(td_handle* h, const float* x_dev, int64_t ldx, const float* x2_dev, int64_t ldx2,
                  const int64_t* file_offsets_host, int num_files, int c, int pre, int post, int c2, int pre2,
                  int post2, int input_offset, const int64_t* rows_used_host, const float* y_dev, int64_t ldy, int d,
                  const int* hidden_host, int num_hidden, int batch_rows, int epochs, float* params_dev,
                  float* state_dev, double lr, double beta1, double beta2, double eps, int64_t step0, int update,
                  int64_t shuffle_seed, double* stats_dev) {
  const MlpCall a = mlp_call({x_dev, ldx, c, pre, post}, {x2_dev, ldx2, c2, pre2, post2}, file_offsets_host,
                             num_files, input_offset, rows_used_host, y_dev, ldy, d, hidden_host, num_hidden,
                             batch_rows, 0, true);
  return mlp_train(h, "td_mlpc_train", a, epochs, params_dev, state_dev,
                   {update ? kUpdAdam : kUpdNone, lr, beta1, beta2, eps, step0}, shuffle_seed, stats_dev);
}

int td_mlpc_grad(td_handle* h, const float* x_dev, int64_t ldx, const float* x2_dev, int64_t ldx2,
                 const int64_t* file_offsets_host, int num_files, int c, int pre, int post, int c2, int pre2,
                 int post2, int input_offset, const int64_t* rows_used_host, const float* y_dev, int64_t ldy, int d,
                 const int* hidden_host, int num_hidden, int batch_rows, int batch_index, const float* params_dev,
                 float* grad_dev, double* stats_dev) {
  const MlpCall a = mlp_call({x_dev, ldx, c, pre, post}, {x2_dev, ldx2, c2, pre2, post2}, file_offsets_host,
                             num_files, input_offset, rows_used_host, y_dev, ldy, d, hidden_host, num_hidden,
                             batch_rows, 0, true);
  return mlp_grad(h, "td_mlpc_grad", a, batch_index, params_dev, grad_dev, stats_dev);
}

int td_mlpc_forward(td_handle* h, const float* x_dev, int64_t ldx, const float* x2_dev, int64_t ldx2,
                    const int64_t* file_offsets_host, int num_files, int c, int pre, int post, int c2, int pre2,
                    int post2, int input_offset, int d, const int* hidden_host, int num_hidden,
                    const float* params_dev, float* out_dev, int64_t ldout) {
  const MlpCall a = mlp_call({x_dev, ldx, c, pre, post}, {x2_dev, ldx2, c2, pre2, post2}, file_offsets_host,
                             num_files, input_offset, nullptr, nullptr, 0, d, hidden_host, num_hidden, kFwdChunk, 0,
                             true);
  return mlp_forward(h, "td_mlpc_forward", a, params_dev, out_dev, ldout);
}

int td_dnn_train_many(td_handle* h, const float* x_dev, int64_t ldx, const int64_t* file_offsets_host, int num_files,
                      int c, int pre, int post, int input_offset, const float* y_dev, int64_t ldy, int d,
                      const int* hidden_host, int num_hidden, int batch_rows, int epochs, int loss, int num_models,
                      const int64_t* rows_used_host, float* const* params_dev_host, float* const* state_dev_host,
                      const float* lr_host, const float* rho_host, const float* eps_host,
                      const int64_t* shuffle_seed_host, double* stats_dev) {
  const MlpCall a = mlp_call({x_dev, ldx, c, pre, post}, {}, file_offsets_host, num_files, input_offset, nullptr,
                             y_dev, ldy, d, hidden_host, num_hidden, batch_rows, loss, false);
  const char* fn = "td_dnn_train_many";
  TD_REQUIRE(h, lr_host && rho_host && eps_host && num_models <= TD_DNN_MANY_MAX_MODELS,
             "%s: NULL argument or more than %d models", fn, TD_DNN_MANY_MAX_MODELS);
  const std::vector<MlpOpt> opt = mlp_opts<float>(kUpdRmsprop, num_models, lr_host, rho_host, nullptr, eps_host,
                                                  nullptr);
  const ManyCall mc = {num_models, rows_used_host, params_dev_host, state_dev_host, opt.data(), shuffle_seed_host};
  return mlp_train_many(h, fn, a, epochs, mc, stats_dev);
}

int td_clf_train_many(td_handle* h, const float* x_dev, int64_t ldx, const float* x2_dev, int64_t ldx2,
                      const int64_t* file_offsets_host, int num_files, int c, int pre, int post, int c2, int pre2,
                      int post2, int input_offset, const float* y_dev, int64_t ldy, int d, const int* hidden_host,
                      int num_hidden, int batch_rows, int epochs, int update, int num_models,
                      const int64_t* rows_used_host, float* const* params_dev_host, float* const* state_dev_host,
                      const double* lr_host, const double* beta1_host, const double* beta2_host,
                      const double* eps_host, const int64_t* step0_host, const int64_t* shuffle_seed_host,
                      double* stats_dev) {
  const MlpCall a = mlp_call({x_dev, ldx, c, pre, post}, {x2_dev, ldx2, c2, pre2, post2}, file_offsets_host,
                             num_files, input_offset, nullptr, y_dev, ldy, d, hidden_host, num_hidden, batch_rows, 0,
                             true);
  const char* fn = "td_clf_train_many";
  TD_REQUIRE(h, num_models <= TD_DNN_MANY_MAX_MODELS, "%s: more than %d models", fn, TD_DNN_MANY_MAX_MODELS);
  TD_REQUIRE(h, !update || (lr_host && beta1_host && beta2_host && eps_host && step0_host), "%s: NULL argument", fn);
  // score only: the optimizer's arrays are not read
  const std::vector<MlpOpt> opt = mlp_opts<double>(update ? kUpdAdam : kUpdNone, num_models, update ? lr_host : nullptr,
                                                   beta1_host, beta2_host, eps_host, step0_host);
  const ManyCall mc = {num_models, rows_used_host, params_dev_host, state_dev_host, opt.data(), shuffle_seed_host};
  return mlp_train_many(h, fn, a, epochs, mc, stats_dev);
}
