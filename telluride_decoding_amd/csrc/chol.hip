// A3 -- ridge solve.  Float64 blocked Cholesky + forward/backward substitution
// on the device, batched over regularisation values: the factorisation, the padded batch of systems
// it works on, td_spd_solve and the td_chol_* interface of eig.hip and cca_sweep.hip.  The ridge routes
// that call it are in solve.hip, the leave-one-out sweep it preconditions in loso.hip.
//
// Reference: brain_model.calculate_linear_regressor_parameters_from_dataset,
// brain_model.py:447-455 (normalise by n, add lambda to EVERY diagonal entry incl.
// the bias) and :477 (np.linalg.solve -- a general LU in the input dtype).  The
// regularised matrix is symmetric positive definite, so Cholesky in float64 gives
// the same solution to well below the reference's own float32 rounding noise.
//
// Structure (right-looking, 64-wide block columns, row-major lower triangle, the
// matrix padded with an identity to a multiple of 64 so that every tile is full and
// 16-byte aligned):
//   diag    : L_kk and L_kk^-1 of one 64x64 block in ONE sweep of 64 column steps --
//             the elimination is applied to the augmented tile [A_kk | I], whose right
//             half ends as L_kk^-1 (register-resident 4x4 sub-tiles, one barrier per step)
//   panel   : X_i = A_ik L_kk^-T as a 64x64x64 GEMM on the float64 matrix cores
//             (v_mfma_f64_16x16x4_f64) -- the triangular solve became a product
//   update  : A_ij -= X_i X_j^T, same GEMM; the workgroup that owns tile (k+1, k+1) goes
//             on to factor it (look-ahead), so the diag sweep of the NEXT step overlaps
//             the trailing update of this one
//   back    : w_k = L_kk^-T z_k, z_m -= L_km^T w_k (m < k), one small launch per block
// The right-hand sides ride along as `nrhs` extra matrix ROWS (rt = B^T, [nrhs][n]):
// panel and update then perform the forward substitution z = L^-1 b for free.
// Small dense, latency-bound: reported as time, not against a roofline.
// (v1 solved the panel by 64-step substitution in every workgroup and ran the update
// on LDS-fed VALU FMAs: 56 + 24 + 22 us per block step, 3.3 ms at n = 2049.)
#include "solve_common.h"

namespace {

using namespace td_tile64;   // NB, LS, f64x4, f64x2, factor_inv_tile and its helpers, tile_to_lds / _regs

constexpr int kOuterCols = 4;  // block columns per outer block of the factorisation (<= 4)

struct CholParams {
  double* a;        // [batch][n][n]   n = nblk * 64 (identity padded); lower triangle in, L out
  double* rt;       // [batch][kMaxRhs][n]  B^T in (rows >= nrhs zero), z^T out
  double* linv;     // [batch][nblk][64][64]  L_kk^-1 (lower triangular, zeros above)
  double* sol;      // [batch][kMaxRhs][n]  w^T out of the backward pass
  int n, nrhs, nblk, k;
  int kf;           // update: first block column of the panels X that are applied
  int jlo;          // update: first block column that is updated
  int col_mode;     // update: 1 = block column jlo only (left-looking step inside an outer block)
  int workers, batch;  // update: workgroups per system; systems
  int rt_rows;         // rows of rt / sol per system (kMaxRhs for the ridge solves; up to 64 for
                       // the forward-only right-hand sides of the CCA whitening)
  int* flag;        // set to 1 when a pivot is not positive
  const double* tol; // [batch] pivots at or below this are "not positive" (64 n eps max diag):
                     // an exactly singular matrix leaves a pivot of +-rounding noise, which
                     // LAPACK's exact-zero test (np.linalg.solve -> "Singular matrix") catches
                     // only because LU happens to cancel exactly there
};

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// C (64x64) = As . Bs^T on the float64 matrix cores; 4 waves, wave w owns the 32x32
// quadrant (w >> 1, w & 1) as 2x2 tiles of v_mfma_f64_16x16x4_f64.  Operand lane map:
// A[i = lane & 15][k = lane >> 4]; C/D: col = lane & 15, row = (lane >> 4) + 4 * reg.
template <bool kAccumulate = false>
__device__ __forceinline__ void gemm_nt_64(const double* __restrict__ as,
                                           const double* __restrict__ bs, int wave, int lane,
                                           f64x4 (&acc)[2][2]) {
  const int li = lane & 15, lk = lane >> 4;
  const double* ap = as + ((wave >> 1) * 32 + li) * LS + lk;
  const double* bp = bs + ((wave & 1) * 32 + li) * LS + lk;
  if (!kAccumulate) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[m][n][r] = 0.0;
  }
  // (fully unrolled: with a rolled loop hipcc keeps the accumulators in VGPRs across the back
  // edge and copies all 32 of them to AGPRs and back around every 16 MFMAs -- 4 of the 8 VALU
  // instructions per MFMA that PMC counted in the batched update)
  // Software-pipelined by hand, two k-steps (8 MFMAs = 512 cycles) per stage: the LDS operands
  // of stage g + 1 are requested before the MFMAs of stage g issue.  (Left to itself hipcc
  // issued a stage's reads right behind the previous stage's last MFMAs and waited for them:
  // an LDS round trip per 8 MFMAs with the matrix pipe idle.)
  double a0[2][2], a1[2][2], b0[2][2], b1[2][2];
  auto ld = [&](int g, int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = 4 * (2 * g + h);
      a0[buf][h] = ap[k]; a1[buf][h] = ap[16 * LS + k];
      b0[buf][h] = bp[k]; b1[buf][h] = bp[16 * LS + k];
    }
  };
  ld(0, 0);
#pragma unroll
  for (int g = 0; g < NB / 8; ++g) {
    const int buf = g & 1;
    if (g + 1 < NB / 8) ld(g + 1, buf ^ 1);
    __builtin_amdgcn_sched_barrier(0);        // (hipcc otherwise sinks the reads to their first use)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[buf][h], b0[buf][h], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[buf][h], b1[buf][h], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[buf][h], b0[buf][h], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[buf][h], b1[buf][h], acc[1][1], 0, 0, 0);
    }
  }
}

// (row, col) of accumulator element acc[m][n][r] inside the 64x64 tile
__device__ __forceinline__ int acc_row(int wave, int lane, int m, int r) {
  return (wave >> 1) * 32 + 16 * m + (lane >> 4) + 4 * r;
}
__device__ __forceinline__ int acc_col(int wave, int lane, int n) {
  return (wave & 1) * 32 + 16 * n + (lane & 15);
}

// Global address of accumulator element acc[m][nn][r] of a full 64x64 tile at `tile` (row
// stride n doubles): wave-uniform part + one per-lane 32-bit byte offset.
__device__ __forceinline__ unsigned acc_lane_off(int lane, int n) {
  return (unsigned)(((lane >> 4) * n + (lane & 15)) * 8);
}
__device__ __forceinline__ char* acc_base(double* tile, int wave, int n, int m, int nn, int r) {
  return reinterpret_cast<char*>(tile) +
         ((size_t)((wave >> 1) * 32 + 16 * m + 4 * r) * n + (wave & 1) * 32 + 16 * nn) * 8;
}

// Factors the tile held in `at` (LDS) and publishes L_kk (the global tile: lower part, zeros
// above) and L_kk^-1.
__device__ __forceinline__ void factor_and_publish(const CholParams& p, int sys, int kb, double* a_b,
                                                   double* at, double* wt, double* sc, int tid) {
  factor_inv_tile(at, wt, sc, tid, p.flag, p.tol[sys]);
  double* g = a_b + (size_t)kb * NB * p.n + (size_t)kb * NB;
  double* li = p.linv + ((size_t)sys * p.nblk + kb) * NB * NB;
  const int c = tid & 63, r0 = tid >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = r0 + 4 * i;
    g[(size_t)r * p.n + c] = (c <= r) ? at[r * LS + c] : 0.0;
    li[r * NB + c] = wt[r * LS + c];
  }
}

// First diagonal block (the later ones are factored by the update kernel).

__global__ __launch_bounds__(256) void chol_diag_kernel(CholParams p) {
  __shared__ double at[NB * LS];
  __shared__ double wt[NB * LS];
  __shared__ double sc[kFactorScratch];
  double* a_b = p.a + (size_t)blockIdx.y * p.n * p.n;
  tile_to_lds(at, a_b + (size_t)p.k * NB * p.n + (size_t)p.k * NB, p.n, NB, threadIdx.x);
  __syncthreads();
  factor_and_publish(p, blockIdx.y, p.k, a_b, at, wt, sc, threadIdx.x);
}

// Update A_ij -= sum_{q < KW} X_i^(kf+q) X_j^(kf+q)^T  (X^(c) = block column c of the panels,
// already in place), for the right-hand-side row too.  Two tile sets:
//   trailing (col_mode 0): jlo <= j <= i < nblk -- the part of the matrix right of an outer
//     block of KW columns takes the rank-64*KW update in ONE pass: a tile of C is read and
//     written once per KW block columns instead of once per block column.  The batched solve
//     of a leave-one-out sweep (hundreds of systems) is bound by exactly that traffic: with
//     rank-64 updates it moved ~80 KB per 64^3 tile product and ran at 4 TB/s with the matrix
//     cores 45% busy.
//   column (col_mode 1): j = jlo only -- the left-looking step inside an outer block: block
//     column jlo receives the updates of the KW columns before it just before its own panel.
// Workgroup 0 owns tile 0 = (jlo, jlo), which is final after this update, and goes on to
// factor it (look-ahead: the serial chain of the solve).  The other workgroups each walk a
// strided list of tiles with the next operands AND the old values of the output tile
// prefetched into registers under the current GEMM, so a tile costs about its MFMAs per wave
// instead of a load-GEMM-store round trip.
struct UpdTile {
  double* rows_i;      // block row i (or the right-hand-side rows)
  const double* rows_j;
  int rows_valid, bi, bj;   // bi = nblk for the right-hand-side rows
};

__device__ __forceinline__ UpdTile upd_tile(const CholParams& p, int sys, double* a_b, int t, int n_tri) {
  int bi, bj;
  if (p.col_mode) {            // n_tri = block rows jlo .. nblk-1; then the right-hand-side row
    bi = t < n_tri ? p.jlo + t : p.nblk;
    bj = p.jlo;
  } else if (t < n_tri) {
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    bi = p.jlo + ti;
    bj = p.jlo + (t - ti * (ti + 1) / 2);
  } else {
    bi = p.nblk;
    bj = p.jlo + (t - n_tri);
  }
  UpdTile u;
  if (bi == p.nblk) {
    u.rows_i = p.rt + (size_t)sys * p.rt_rows * p.n;
    u.rows_valid = p.nrhs;
  } else {
    u.rows_i = a_b + (size_t)bi * NB * p.n;
    u.rows_valid = NB;
  }
  u.rows_j = a_b + (size_t)bj * NB * p.n;
  u.bi = bi;
  u.bj = bj;
  return u;
}

// Panel: block rows i = k+1 .. nblk-1 and the virtual right-hand-side row (the last index):
// X = A_ik L_kk^-T.  A workgroup keeps L_kk^-1 in LDS and walks kPanelTiles row tiles with the
// next tile's rows prefetched into registers under the current GEMM (one tile per workgroup,
// load - barrier - GEMM - store, took 2.1 ms of a 16.8 ms batch of 160 solves for 10% of the
// arithmetic).
// (A single system keeps one tile per workgroup: its launches are latency chains.)
constexpr int kPanelTiles = 3;

__global__ __launch_bounds__(256) void chol_panel_kernel(CholParams p, int tiles_per_wg) {
  __shared__ double as[NB * LS];
  __shared__ double bs[NB * LS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = p.n, k0 = p.k * NB;
  double* a_b = p.a + (size_t)blockIdx.y * n * n;
  const int total = p.nblk - p.k;                  // row tiles below the diagonal + the rhs rows
  const int first = blockIdx.x * tiles_per_wg;
  const int end = first + tiles_per_wg < total ? first + tiles_per_wg : total;
  auto rows_of = [&](int t, int& rows_valid) -> double* {
    const int bi = p.k + 1 + t;
    if (bi == p.nblk) {
      rows_valid = p.nrhs;
      return p.rt + (size_t)blockIdx.y * p.rt_rows * n + k0;
    }
    rows_valid = NB;
    return a_b + (size_t)bi * NB * n + k0;
  };
  f64x2 ra[8];
  int valid = NB;
  double* rows = rows_of(first, valid);
  tile_to_regs(ra, rows, n, valid, tid);
  tile_to_lds(bs, p.linv + ((size_t)blockIdx.y * p.nblk + p.k) * NB * NB, NB, NB, tid);
  for (int t = first; t < end; ++t) {
    regs_to_lds(as, ra, tid);
    __syncthreads();
    int valid_next = NB;
    double* rows_next = rows;
    if (t + 1 < end) {
      rows_next = rows_of(t + 1, valid_next);
      tile_to_regs(ra, rows_next, n, valid_next, tid);
    }
    f64x4 acc[2][2];
    gemm_nt_64(as, bs, wave, lane, acc);
    if (valid == NB) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            *reinterpret_cast<double*>(acc_base(rows, wave, n, m, nn, r) + acc_lane_off(lane, n)) =
                acc[m][nn][r];
    } else {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = acc_row(wave, lane, m, r), col = acc_col(wave, lane, nn);
            if (row < valid) rows[(size_t)row * n + col] = acc[m][nn][r];
          }
    }
    if (t + 1 < end) __syncthreads();             // `as` is free for the next tile
    rows = rows_next;
    valid = valid_next;
  }
}

template <int KW>
__global__ __launch_bounds__(256, 2) void chol_update_kernel(CholParams p, int n_tri, int n_tiles) {
  __shared__ double xi[NB * LS];
  __shared__ double xj[NB * LS];
  __shared__ double sc[kFactorScratch];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = p.n, k0 = p.kf * NB;
  // One-dimensional grid, XCD-aware: workgroup L runs on XCD L mod 8 (round-robin dispatch),
  // so system s = 8 * (slot / workers) + L mod 8 keeps ALL its workgroups on one XCD, next to
  // each other in dispatch order: the panels X of a system (up to 4 MB for 4 block columns)
  // are then fetched into ONE L2 and shared by its tiles.  (Dealt across the 8 XCDs, every
  // tile product of a 160-system batch pulled its 256 KB of operands from beyond the L2 and the
  // update ran at the speed of that traffic: 6 TB/s, matrix cores half idle.)
  // (Fewer than 8 systems: plain order, a system spreads over the whole chip.)
  const int workers = p.workers;
  const bool by_xcd = p.batch >= 8;
  const int slot = by_xcd ? blockIdx.x >> 3 : blockIdx.x;
  const int sys = by_xcd ? (slot / workers) * 8 + (blockIdx.x & 7) : slot / workers;
  const int wk = slot % workers;
  if (sys >= p.batch) return;
  double* a_b = p.a + (size_t)sys * n * n;

  if (wk == 0) {
    // ---- tile (jlo, jlo): update, then factor it on chip --------------------------------
    const UpdTile u = upd_tile(p, sys, a_b, 0, n_tri);
    // every load of the chain is issued up front: the KW operand tiles (tile 0 is on the
    // diagonal: X_i == X_j) and the old values of the tile
    // (two operand tiles in flight: a third would cost the kernel its second wave per SIMD)
    constexpr int kInFlight = KW < 2 ? KW : 2;
    f64x2 rq[kInFlight][8];
#pragma unroll
    for (int q = 0; q < kInFlight; ++q) tile_to_regs(rq[q], u.rows_i + k0 + q * NB, n, NB, tid);
    const double* src = u.rows_i + (size_t)u.bj * NB;
    double cold[2][2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          cold[m][nn][r] = *reinterpret_cast<const double*>(
              acc_base(const_cast<double*>(src), wave, n, m, nn, r) + acc_lane_off(lane, n));
    f64x4 acc[2][2];
#pragma unroll
    for (int q = 0; q < KW; ++q) {
      double* xq = (q & 1) ? xj : xi;             // alternate tiles: one barrier per round
      regs_to_lds(xq, rq[q % kInFlight], tid);
      if (q + kInFlight < KW)
        tile_to_regs(rq[q % kInFlight], u.rows_i + k0 + (q + kInFlight) * NB, n, NB, tid);
      __syncthreads();
      if (q == 0) gemm_nt_64<false>(xq, xq, wave, lane, acc);
      else        gemm_nt_64<true>(xq, xq, wave, lane, acc);
    }
    __syncthreads();                  // every wave is done reading xi / xj before they are reused
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = acc_row(wave, lane, m, r), col = acc_col(wave, lane, nn);
          xi[row * LS + col] = cold[m][nn][r] - acc[m][nn][r];
        }
    __syncthreads();
    factor_and_publish(p, sys, p.jlo, a_b, xi, xj, sc, tid);
    return;
  }

  // ---- bulk: tiles 1 + (blockIdx.x - 1), stride gridDim.x - 1 ------------------------------
  // Matrix tiles are addressed through a buffer descriptor of this system's matrix: SGPR tile
  // offset + ONE per-lane VGPR offset for every load and store (with flat addresses hipcc kept
  // a 64-bit VGPR pair per load -- 96 VGPRs of addresses -- and the kernel had no registers
  // left to prefetch the LDS operands of the MFMAs).  The right-hand-side rows (another
  // buffer, fewer than 64 rows) keep the pointer path.
  const int stride = workers - 1;
  int t = wk;
  if (t >= n_tiles) return;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(a_b, 0, n * n * 8, 0x00020000);
  const unsigned voff_t = (unsigned)(((tid >> 5) * n + (tid & 31) * 2) * 8);
  const unsigned voff_c = acc_lane_off(lane, n);
  auto load_tile = [&](f64x2 (&v)[8], int brow, int q) {
    const unsigned s0 = (unsigned)((brow * NB * n + (p.kf + q) * NB) * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      v[i] = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(
                                           rs, voff_t, s0 + (unsigned)(8 * i * n * 8), 0));
  };
  auto c_off = [&](const UpdTile& u, int m, int nn, int r) -> unsigned {
    return (unsigned)(((u.bi * NB + (wave >> 1) * 32 + 16 * m + 4 * r) * n + u.bj * NB +
                       (wave & 1) * 32 + 16 * nn) * 8);
  };
  auto load_operands = [&](const UpdTile& u, int q, f64x2 (&va)[8], f64x2 (&vb)[8]) {
    // (a matrix tile goes through the matrix's buffer descriptor; the right-hand-side rows live
    // in another buffer -- also when there are exactly 64 of them)
    if (u.bi != p.nblk) load_tile(va, u.bi, q);
    else tile_to_regs(va, u.rows_i + (p.kf + q) * NB, n, u.rows_valid, tid);
    load_tile(vb, u.bj, q);
  };
  f64x2 ra[8], rb[8];
  UpdTile cur = upd_tile(p, sys, a_b, t, n_tri);
  load_operands(cur, 0, ra, rb);
  while (true) {
    const int tn = t + stride;
    const bool more = tn < n_tiles;
    UpdTile nxt = cur;
    if (more) nxt = upd_tile(p, sys, a_b, tn, n_tri);
    double* dst = cur.rows_i + (size_t)cur.bj * NB;
    const bool full = cur.bi != p.nblk;             // every tile but the right-hand-side rows
    f64x4 acc[2][2];
    double cold[2][2][4];
#pragma unroll
    for (int q = 0; q < KW; ++q) {
      regs_to_lds(xi, ra, tid);
      regs_to_lds(xj, rb, tid);
      __syncthreads();
      // loads that fly under the GEMM: the next operands (the next 64 columns of this tile's
      // panels, or the first of the next tile) and, in the last round, the old output values
      if (q + 1 < KW) {
        load_operands(cur, q + 1, ra, rb);
      } else {
        if (full) {
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int nn = 0; nn < 2; ++nn)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                cold[m][nn][r] = __builtin_bit_cast(
                    double, __builtin_amdgcn_raw_buffer_load_b64(rs, voff_c, c_off(cur, m, nn, r), 0));
        } else {
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int nn = 0; nn < 2; ++nn)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = acc_row(wave, lane, m, r), col = acc_col(wave, lane, nn);
                const int rc = row < cur.rows_valid ? row : 0;
                cold[m][nn][r] = dst[(unsigned)(rc * n + col)];
              }
        }
        if (more) load_operands(nxt, 0, ra, rb);
      }
      if (q == 0) gemm_nt_64<false>(xi, xj, wave, lane, acc);
      else        gemm_nt_64<true>(xi, xj, wave, lane, acc);
      if (q + 1 < KW) __syncthreads();      // LDS operands are free for the next round
    }
    if (full) {
      // (one branch for the tile instead of one exec-masked block per store)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            __builtin_amdgcn_raw_buffer_store_b64(
                __builtin_bit_cast(u32x2, cold[m][nn][r] - acc[m][nn][r]), rs, voff_c,
                c_off(cur, m, nn, r), 0);
    } else {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = acc_row(wave, lane, m, r), col = acc_col(wave, lane, nn);
            if (row < cur.rows_valid) dst[(unsigned)(row * n + col)] = cold[m][nn][r] - acc[m][nn][r];
          }
    }
    if (!more) break;
    __syncthreads();                  // LDS operands are free for the next tile
    cur = nxt;
    t = tn;
  }
}

// Backward substitution step for block k (descending): every workgroup forms
// w_k = L_kk^-T z_k from the stored inverse; workgroup m < k applies z_m -= L_km^T w_k, the
// last workgroup (m == k) publishes w_k to `sol` (z_k itself is still being read by the
// others).  Thread (c, g) = (tid & 63, tid >> 6) sums 16 of the 64 terms of column c.
__global__ __launch_bounds__(256) void chol_back_kernel(CholParams p) {
  __shared__ double zs[kMaxRhs][NB];
  __shared__ double ws[kMaxRhs][NB];
  __shared__ double part[4][NB];
  const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
  const int n = p.n, k0 = p.k * NB;
  const double* a_b = p.a + (size_t)blockIdx.y * n * n;
  double* rt = p.rt + (size_t)blockIdx.y * p.rt_rows * n;
  const double* li = p.linv + ((size_t)blockIdx.y * p.nblk + p.k) * NB * NB;
  for (int idx = tid; idx < p.nrhs * NB; idx += 256) zs[idx >> 6][idx & 63] = rt[(size_t)(idx >> 6) * n + k0 + (idx & 63)];
  __syncthreads();
  // w[c] = sum_r Linv[r][c] * z[r]
  double lcol[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) lcol[i] = li[(g + 4 * i) * NB + c];
  for (int q = 0; q < p.nrhs; ++q) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += lcol[i] * zs[q][g + 4 * i];
    part[g][c] = s;
    __syncthreads();
    if (g == 0) ws[q][c] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
    __syncthreads();
  }
  const int m = blockIdx.x;
  if (m == p.k) {
    double* sol = p.sol + (size_t)blockIdx.y * p.rt_rows * n;
    for (int idx = tid; idx < p.nrhs * NB; idx += 256) sol[(size_t)(idx >> 6) * n + k0 + (idx & 63)] = ws[idx >> 6][idx & 63];
    return;
  }
  const int m0 = m * NB;
#pragma unroll
  for (int i = 0; i < 16; ++i) lcol[i] = a_b[(size_t)(k0 + g + 4 * i) * n + m0 + c];   // L[k-block][m-block]
  for (int q = 0; q < p.nrhs; ++q) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += lcol[i] * ws[q][g + 4 * i];
    part[g][c] = s;
    __syncthreads();
    if (g == 0) rt[(size_t)q * n + m0 + c] -= (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
    __syncthreads();
  }
}

// tol[b] = 64 n eps max_{i < n_real} a[i][i]; the identity padding (rows n_real .. n - 1, decoupled
// from the system) takes that maximum as its diagonal, so that its pivots sit on the system's own
// scale: with a fixed 1.0 a system whose diagonal is ~1e13 or more (a huge ridge lambda) had its
// PADDING reported as "not positive definite", and a tiny one had its tolerance set by the padding.
__global__ __launch_bounds__(256) void diag_tol_kernel(double* __restrict__ a, int n, int n_real,
                                                       double* __restrict__ tol) {
  __shared__ double red[256];
  double* ab = a + (size_t)blockIdx.x * n * n;
  double m = 0.0;
  for (int i = threadIdx.x; i < n_real; i += 256) m = fmax(m, fabs(ab[(size_t)i * n + i]));
  red[threadIdx.x] = m;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  if (threadIdx.x == 0) tol[blockIdx.x] = 64.0 * n_real * 2.220446049250313e-16 * red[0];
  const double top = red[0] > 0.0 ? red[0] : 1.0;
  for (int i = n_real + threadIdx.x; i < n; i += 256) ab[(size_t)i * n + i] = top;
}

// What every launch of a solve is told: the buffers and sizes, block step 0, one worker, no flag and no
// tolerances (the backward pass needs neither).  Every field is assigned.
CholParams chol_params(double* a_dev, double* rt_dev, double* sol_dev, double* linv_dev, int n, int nrhs,
                       int batch, int rt_rows) {
  CholParams p;
  p.a = a_dev; p.rt = rt_dev; p.linv = linv_dev; p.sol = sol_dev; p.tol = nullptr;
  p.n = n; p.nrhs = nrhs; p.nblk = n / NB; p.flag = nullptr;
  p.k = 0; p.kf = 0; p.jlo = 0; p.col_mode = 0; p.workers = 1; p.batch = batch;
  p.rt_rows = rt_rows;
  return p;
}

}  // namespace

// Core: a [batch][n][n] (n a multiple of 64), rt [batch][kMaxRhs][n]; solution in sol.
// Factorisation with the forward substitution of the right-hand-side rows (rt: B^T in, z^T =
// (L^-1 B)^T out); L and the inverses of its diagonal blocks stay in a_dev / linv_dev.
int chol_factor_forward(td_handle* h, double* a_dev, double* rt_dev, double* sol_dev,
                        double* linv_dev, double* tol_dev, int n, int nrhs, int batch,
                        int* flag_dev, int rt_rows, int n_real) {
  // (the update kernel addresses a system through a 32-bit buffer descriptor: n * n * 8 bytes)
  TD_REQUIRE(h, n <= 16320, "cholesky: systems of more than 16320 unknowns are not supported (n = %d)", n);
  if (!flag_dev) flag_dev = h->dev_flag;      // (a caller's flag outlives the next solve)
  TD_HIP(h, hipMemsetAsync(flag_dev, 0, sizeof(int), h->stream));
  hipLaunchKernelGGL(diag_tol_kernel, dim3((unsigned)batch), dim3(256), 0, h->stream, a_dev, n,
                     n_real, tol_dev);
  const int nblk = n / NB;
  CholParams p = chol_params(a_dev, rt_dev, sol_dev, linv_dev, n, nrhs, batch, rt_rows);
  p.tol = tol_dev; p.flag = flag_dev;
  hipLaunchKernelGGL(chol_diag_kernel, dim3(1, (unsigned)batch), dim3(256), 0, h->stream, p);
  // Outer blocks of `ow` block columns: left-looking inside (column c first takes the updates
  // of the columns of its outer block before it, then its panel), right-looking outside (the
  // trailing matrix takes the rank-64*ow update once per outer block).
  // A single system is bound by the chain of launches, not by traffic: there the left-looking
  // column steps (whose tiles run KW GEMMs in sequence) only lengthen the chain
  // (n = 2049: 1.10 ms with 1 column per outer block, 1.28 ms with 4; 160 systems: 21.6 -> 16.8 ms).
  const int ow = batch <= 2 ? 1 : kOuterCols;
  const int panel_tiles = batch <= 2 ? 1 : kPanelTiles;
  auto launch_update = [&](int kf, int kw, int jlo, int col_mode) {
    const int rem = nblk - jlo;                  // block rows jlo .. nblk-1
    const int tri = col_mode ? rem : rem * (rem + 1) / 2;
    const int n_tiles = col_mode ? rem + 1 : tri + rem;
    // workgroup 0 = look-ahead tile; the bulk gets at most ~3 tiles per workgroup
    int bulk_wgs = (n_tiles - 1 + 2) / 3;
    if (bulk_wgs > n_tiles - 1) bulk_wgs = n_tiles - 1;
    if (bulk_wgs < 1) bulk_wgs = 1;
    p.kf = kf; p.jlo = jlo; p.col_mode = col_mode;
    p.workers = 1 + bulk_wgs; p.batch = batch;
    const dim3 grid((unsigned)((1 + bulk_wgs) * (batch >= 8 ? (int)td_round_up(batch, 8) : batch)));
    switch (kw) {
      case 1: hipLaunchKernelGGL(chol_update_kernel<1>, grid, dim3(256), 0, h->stream, p, tri, n_tiles); break;
      case 2: hipLaunchKernelGGL(chol_update_kernel<2>, grid, dim3(256), 0, h->stream, p, tri, n_tiles); break;
      case 3: hipLaunchKernelGGL(chol_update_kernel<3>, grid, dim3(256), 0, h->stream, p, tri, n_tiles); break;
      default: hipLaunchKernelGGL(chol_update_kernel<4>, grid, dim3(256), 0, h->stream, p, tri, n_tiles); break;
    }
  };
  for (int kb = 0; kb < nblk; kb += ow) {
    const int cols = nblk - kb < ow ? nblk - kb : ow;
    for (int q = 0; q < cols; ++q) {
      const int c = kb + q;
      if (q > 0) launch_update(kb, q, c, 1);       // ... which also factors tile (c, c)
      p.k = c;
      // block rows c+1 .. nblk-1 and the right-hand-side row
      hipLaunchKernelGGL(chol_panel_kernel,
                         dim3((unsigned)((nblk - c + panel_tiles - 1) / panel_tiles), (unsigned)batch),
                         dim3(256), 0, h->stream, p, panel_tiles);
    }
    if (kb + ow < nblk) launch_update(kb, ow, kb + ow, 0);   // ... factors (kb + ow, kb + ow)
  }
  if (hipGetLastError() != hipSuccess) return td_fail(h, TD_ERR_HIP, "cholesky launch failed");
  return TD_OK;
}

// Backward substitution w^T = (L^-T z)^T of the rows in rt_dev (at most kMaxRhs per system)
// into sol_dev, with the factors chol_factor_forward left behind.
static int chol_backward(td_handle* h, double* a_dev, double* rt_dev, double* sol_dev, double* linv_dev,
                         int n, int nrhs, int batch, int rt_rows) {
  CholParams p = chol_params(a_dev, rt_dev, sol_dev, linv_dev, n, nrhs, batch, rt_rows);
  for (int k = p.nblk - 1; k >= 0; --k) {
    p.k = k;
    hipLaunchKernelGGL(chol_back_kernel, dim3((unsigned)(k + 1), (unsigned)batch), dim3(256), 0,
                       h->stream, p);
  }
  if (hipGetLastError() != hipSuccess) return td_fail(h, TD_ERR_HIP, "cholesky launch failed");
  return TD_OK;
}

int spd_solve_padded(td_handle* h, double* a_dev, double* rt_dev, double* sol_dev,
                     double* linv_dev, double* tol_dev, int n, int n_real, int nrhs, int batch,
                     int* flag_dev) {
  TD_TRY(chol_factor_forward(h, a_dev, rt_dev, sol_dev, linv_dev, tol_dev, n, nrhs, batch, flag_dev,
                             kMaxRhs, n_real));
  return chol_backward(h, a_dev, rt_dev, sol_dev, linv_dev, n, nrhs, batch, kMaxRhs);
}

int spd_check_flag(td_handle* h) {
  int flag = 0;
  TD_HIP(h, hipMemcpyAsync(&flag, h->dev_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  TD_HIP(h, hipStreamSynchronize(h->stream));
  if (flag)
    return td_fail(h, TD_ERR_SINGULAR, "Singular matrix: covariance is not positive definite");
  return TD_OK;
}

namespace {

// ---- padding / unpadding --------------------------------------------------------------
// dst [batch][np][np] = src [batch][n][n] * scale + lambda_b * I, identity beyond n -- the 64x64
// tiles on and below the diagonal only: the factorisation never touches the others, and this
// copy is pure HBM traffic (33 MB per system at n = 2049: 2.1 ms for the 160 systems of one
// batch of a leave-one-out sweep when the whole square was written).  Workgroup = one tile.
__global__ __launch_bounds__(256) void pad_matrix_kernel(const double* __restrict__ src,
                                                         long long src_batch_stride, int src_ld, int n,
                                                         int np, double scale,
                                                         const double* __restrict__ lambdas,
                                                         double* __restrict__ dst) {
  const int b = blockIdx.y;
  int bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= (int)blockIdx.x) ++bi;
  const int bj = (int)blockIdx.x - bi * (bi + 1) / 2;
  const double lam = lambdas ? lambdas[b] : 0.0;
  const double* s = src + (size_t)b * src_batch_stride;
  double* d = dst + (size_t)b * np * np;
  const int c = bj * NB + (threadIdx.x & 63);
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int r = bi * NB + (threadIdx.x >> 6) + 4 * i;
    double v = (r == c) ? 1.0 : 0.0;
    if (r < n && c < n) v = s[(size_t)r * src_ld + c] * scale + (r == c ? lam : 0.0);
    d[(size_t)r * np + c] = v;
  }
}

// rt [batch][kMaxRhs][np] = scale * rhs^T (rhs [batch][n][nrhs]), zero padded.
__global__ void pad_rhs_kernel(const double* __restrict__ rhs, long long rhs_batch_stride, int n,
                               int nrhs, int np, double scale, double* __restrict__ rt) {
  const int b = blockIdx.y;
  const double* s = rhs + (size_t)b * rhs_batch_stride;
  double* d = rt + (size_t)b * kMaxRhs * np;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kMaxRhs * np; i += gridDim.x * blockDim.x) {
    const int q = i / np, r = i % np;
    d[i] = (q < nrhs && r < n) ? s[(size_t)r * nrhs + q] * scale : 0.0;
  }
}

// rhs [batch][n][nrhs] = sol^T
__global__ void unpad_sol_kernel(const double* __restrict__ sol, int n, int nrhs, int np,
                                 double* __restrict__ rhs) {
  const int b = blockIdx.y;
  const double* s = sol + (size_t)b * kMaxRhs * np;
  double* d = rhs + (size_t)b * n * nrhs;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n * nrhs; i += gridDim.x * blockDim.x) {
    const int r = i / nrhs, q = i % nrhs;
    d[i] = s[(size_t)q * np + r];
  }
}

// rows [nb][n] -> padded rows [rows][np] (zero beyond nb / n); and back
__global__ void pad_rows_kernel(const double* __restrict__ src, int nb, int n, int rows, int np,
                                double* __restrict__ dst) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * np; i += gridDim.x * blockDim.x) {
    const int q = i / np, r = i % np;
    dst[i] = (q < nb && r < n) ? src[(size_t)q * n + r] : 0.0;
  }
}

__global__ void unpad_rows_kernel(const double* __restrict__ src, int nb, int n, int np,
                                  double* __restrict__ dst) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nb * n; i += gridDim.x * blockDim.x)
    dst[i] = src[(size_t)(i / n) * np + (i % n)];
}

}  // namespace

SolveWs carve(void* base, int np, int batch) {
  SolveWs w;
  char* p = reinterpret_cast<char*>(base);
  const size_t nblk = np / NB;
  w.a = reinterpret_cast<double*>(p);    p += sizeof(double) * (size_t)batch * np * np;
  w.rt = reinterpret_cast<double*>(p);   p += sizeof(double) * (size_t)batch * kMaxRhs * np;
  w.sol = reinterpret_cast<double*>(p);  p += sizeof(double) * (size_t)batch * kMaxRhs * np;
  w.linv = reinterpret_cast<double*>(p); p += sizeof(double) * (size_t)batch * nblk * NB * NB;
  w.lams = reinterpret_cast<double*>(p); p += sizeof(double) * td_round_up(batch, 32);
  w.tol = reinterpret_cast<double*>(p);  p += sizeof(double) * td_round_up(batch, 32);
  w.bytes = (size_t)(p - reinterpret_cast<char*>(base));
  return w;
}

void pad_systems(td_handle* h, const double* src, long long src_batch_stride, int src_ld, int n, int np,
                 double scale, const double* lambdas, double* a_dst, int batch, const double* rhs,
                 long long rhs_batch_stride, int nrhs, double* rt_dst) {
  const int nblk = np / NB;
  hipLaunchKernelGGL(pad_matrix_kernel, dim3((unsigned)(nblk * (nblk + 1) / 2), (unsigned)batch), dim3(256), 0,
                     h->stream, src, src_batch_stride, src_ld, n, np, scale, lambdas, a_dst);
  if (rhs)
    hipLaunchKernelGGL(pad_rhs_kernel, dim3(16, (unsigned)batch), dim3(256), 0, h->stream, rhs, rhs_batch_stride,
                       n, nrhs, np, scale, rt_dst);
}

void unpad_rows(td_handle* h, const double* src, int nb, int n, int np, double* dst, int blocks) {
  hipLaunchKernelGGL(unpad_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, src, nb, n, np, dst);
}

namespace {

// ---- the tile kernels of the leave-one-out sweep (loso.hip has the method, the row-wise kernels and the host) ----
// They share the force-inlined tile helpers of td_tile64.h with the factorisation's kernels and with each other, and
// what hipcc emits for a kernel depends on the other callers of a helper in its translation unit (constants that
// every caller passes are propagated into it before it is inlined): loso_big_update_kernel compiles to the same
// code only next to a caller of tile_to_regs whose row count is not a constant (chol_panel_kernel), and
// loso_matvec_kernel only next to the other callers of gemm_32x64.  So they live here, each launched through one
// host function (tools/isa_diff.py shows the difference when one is moved out).
struct LosoMatvec {
  const double* a;        // [folds][n][np] dense moments (symmetric; rows np numbers apart)
  const double* p;        // rows
  double* q;              // rows
  const double* inv_n;    // [folds] 1 / frames of the fold
  const double* lams;     // [n_lambda]
  int n, np, folds, n_lambda, d;
};

// q_row = inv_n[f] * (p_row . A_f) + lambda * p_row for the rows (lambda, q) of fold f.
// grid: (np / 64 column tiles, folds, ceil(n_lambda * d / 32))
// The pass is HBM traffic (every A_f byte once: 1.07 GB at C5): the next 64 x 64 tile of A_f and
// the next 32 x 64 piece of the rows are fetched into registers while the matrix cores work on
// the current ones (load - barrier - product - barrier without that: 0.79 ms, 1.4 TB/s).
__global__ __launch_bounds__(256) void loso_matvec_kernel(LosoMatvec m) {
  __shared__ double as[kLosoRows * LS];
  __shared__ double bs[NB * LS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ct = blockIdx.x, f = blockIdx.y, chunk = blockIdx.z;
  const int rows_f = m.n_lambda * m.d;                 // rows of this fold: index j = lambda * d + q
  const int j0 = chunk * kLosoRows;
  const int rows_valid = rows_f - j0 < kLosoRows ? rows_f - j0 : kLosoRows;
  const long long row_stride = (long long)m.folds * m.np;        // between rows j and j + 1 of a fold
  const double* pf = m.p + ((long long)j0 * m.folds + f) * m.np;
  const double* af = m.a + (size_t)f * m.n * m.np;     // rows np numbers apart (aligned)
  const int c0 = ct * NB;
  const int cols_valid = m.n - c0 < NB ? m.n - c0 : NB;
  f64x4 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = 0.0;
  // thread (c = tid & 63, r0 = tid >> 6): rows r0 + 4 i of the A tile (16), rows r0 + 4 i of the
  // row piece (8); a wave instruction reads one 512-byte row of the tile
  const int c = tid & 63, r0 = tid >> 6;
  double ta[16], tp[8];
  auto fetch = [&](int kt) {
    const int k0 = kt * NB;
    const int k_valid = m.n - k0 < NB ? (m.n - k0 > 0 ? m.n - k0 : 0) : NB;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = r0 + 4 * i;
      ta[i] = (r < k_valid && c < cols_valid) ? af[(size_t)(k0 + r) * m.np + c0 + c] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + 4 * i;
      tp[i] = (r < rows_valid && c < k_valid) ? pf[(long long)r * row_stride + k0 + c] : 0.0;
    }
  };
  const int n_kt = m.np / NB;
  fetch(0);
  for (int kt = 0; kt < n_kt; ++kt) {
#pragma unroll
    for (int i = 0; i < 16; ++i) bs[(r0 + 4 * i) * LS + c] = ta[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) as[(r0 + 4 * i) * LS + c] = tp[i];
    __syncthreads();
    if (kt + 1 < n_kt) fetch(kt + 1);
    gemm_32x64<false>(as, bs, wave, lane, acc);
    __syncthreads();
  }
  // C/D map: col = lane & 15, row = (lane >> 4) + 4 reg
  const int col = c0 + 16 * wave + (lane & 15);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * t + (lane >> 4) + 4 * r;
      if (row < rows_valid) {
        const int j = j0 + row;
        const long long off = ((long long)j * m.folds + f) * m.np + col;
        const double lam = m.lams[j / m.d];
        m.q[off] = col < m.n ? acc[t][r] * m.inv_n[f] + lam * m.p[off] : 0.0;
      }
    }
}

// ---- the substitutions of the preconditioner, in steps of FOUR block columns (256 unknowns) -----
// In steps of one 64-block a substitution was a chain of 33 dependent launches (n = 2049), ~17 us
// each whatever they computed: 1.1 ms per application of the preconditioner, 8 of the C5 sweep's
// 24 ms (that form has been removed).  With the
// inverse of every 256 x 256 diagonal block of L at hand (four 64-blocks: X_ii = Linv_ii,
// X_ij = -Linv_ii sum_{j <= p < i} L_ip X_pj, built once per factorisation: loso_binv_kernel) a
// step solves 256 unknowns at a time -- one launch for the solved block (a sum of <= 4 products
// per 64-column tile), one for the updates of the tiles beyond (4 products each) -- and the chain
// is 9 x 2 launches per direction.
struct LosoBig {
  const double* l;        // [n_lambda][np][np]
  const double* xinv;     // [n_lambda][nbig][4][4][64][64] inverses of the 256-blocks (lower tiles)
  double* v;              // rows, updated in place
  double* out;            // rows: the solved blocks
  int np, nblk, nbig, kb, m, rows_per_lambda;     // kb: big block; m: its 64-blocks (<= 4)
};

__device__ __forceinline__ void rows_to_regs(double (&r)[8], const double* __restrict__ g, long long ld,
                                             int rows_valid, int tid) {
  // thread (c = tid & 63, r0 = tid >> 6): rows r0 + 4 i of a 32 x 64 piece
  const int c = tid & 63, r0 = tid >> 6;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = r0 + 4 * i;
    r[i] = row < rows_valid ? g[(long long)row * ld + c] : 0.0;
  }
}
__device__ __forceinline__ void rows_regs_to_lds(double* lds, const double (&r)[8], int tid) {
  const int c = tid & 63, r0 = tid >> 6;
#pragma unroll
  for (int i = 0; i < 8; ++i) lds[(r0 + 4 * i) * LS + c] = r[i];
}

// X = (L_KK)^-1 of one 256-block, block column j of it per workgroup.  grid: (nbig, n_lambda, 4)
__global__ __launch_bounds__(256) void loso_binv_kernel(const double* __restrict__ l,
                                                        const double* __restrict__ linv,
                                                        double* __restrict__ xinv, int np, int nblk, int nbig) {
  __shared__ double as[NB * LS];
  __shared__ double bs[NB * LS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kb = blockIdx.x, lam = blockIdx.y, j = blockIdx.z;
  const int m = nblk - kBig * kb < kBig ? nblk - kBig * kb : kBig;
  if (j >= m) return;
  const double* lmat = l + (size_t)lam * np * np;
  const double* li = linv + ((size_t)lam * nblk + (size_t)kBig * kb) * NB * NB;
  double* x = xinv + ((size_t)lam * nbig + kb) * 16 * NB * NB;          // tile (r, c) at (4 r + c) * 4096
  const int col = 16 * wave + (lane & 15);
  // X_jj = Linv_jj
  for (int idx = tid; idx < NB * NB; idx += 256) x[(size_t)(4 * j + j) * NB * NB + idx] = li[(size_t)j * NB * NB + idx];
  for (int i = j + 1; i < m; ++i) {
    __syncthreads();                                   // (X tiles written above are read below)
    f64x4 acc[2][2];                                   // [row half][16-row tile] of the 64 x 64 sum
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[hf][t][r] = 0.0;
    for (int p = j; p < i; ++p) {
      // A = L[4 kb + i][4 kb + p], B = X_pj
      tile_to_lds(as, lmat + (size_t)(kBig * kb + i) * NB * np + (size_t)(kBig * kb + p) * NB, np, NB, tid);
      tile_to_lds(bs, x + (size_t)(4 * p + j) * NB * NB, NB, NB, tid);
      __syncthreads();
      gemm_32x64<false>(as, bs, wave, lane, acc[0]);
      gemm_32x64<false>(as + 32 * LS, bs, wave, lane, acc[1]);
      __syncthreads();
    }
    // the sum -> LDS (as B), times -Linv_ii from the left
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) bs[(32 * hf + 16 * t + (lane >> 4) + 4 * r) * LS + col] = acc[hf][t][r];
    tile_to_lds(as, li + (size_t)i * NB * NB, NB, NB, tid);
    __syncthreads();
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[hf][t][r] = 0.0;
    gemm_32x64<false>(as, bs, wave, lane, acc[0]);
    gemm_32x64<false>(as + 32 * LS, bs, wave, lane, acc[1]);
    double* xt = x + (size_t)(4 * i + j) * NB * NB;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) xt[(32 * hf + 16 * t + (lane >> 4) + 4 * r) * NB + col] = -acc[hf][t][r];
    __threadfence_block();
  }
}

// The solved 256-block: tile c of it = sum over p of (rows of block 4 kb + p) x (a tile of X).
//   forward:  y_c = sum_{p <= c} b_p X_cp^T          backward: w_c = sum_{p >= c} y_p X_pc
// grid: (m, n_lambda, row chunks)
template <bool kBack>
__global__ __launch_bounds__(256) void loso_big_solve_kernel(LosoBig t) {
  __shared__ double as[kLosoRows * LS];
  __shared__ double bs[NB * LS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.x, lam = blockIdx.y, chunk = blockIdx.z;
  const int r0 = chunk * kLosoRows;
  const int rows_valid = t.rows_per_lambda - r0 < kLosoRows ? t.rows_per_lambda - r0 : kLosoRows;
  const double* vrows = t.v + ((long long)lam * t.rows_per_lambda + r0) * t.np + (size_t)kBig * t.kb * NB;
  double* orows = t.out + ((long long)lam * t.rows_per_lambda + r0) * t.np + (size_t)kBig * t.kb * NB;
  const double* x = t.xinv + ((size_t)lam * t.nbig + t.kb) * 16 * NB * NB;
  const int p_lo = kBack ? c : 0, p_hi = kBack ? t.m - 1 : c;
  auto xtile = [&](int p) { return x + (size_t)(kBack ? 4 * p + c : 4 * c + p) * NB * NB; };
  f64x4 acc[2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[s][r] = 0.0;
  double ra[8];
  f64x2 rt[8];
  rows_to_regs(ra, vrows + (size_t)p_lo * NB, t.np, rows_valid, tid);
  tile_to_regs(rt, xtile(p_lo), NB, NB, tid);
  for (int p = p_lo; p <= p_hi; ++p) {
    rows_regs_to_lds(as, ra, tid);
    regs_to_lds(bs, rt, tid);
    __syncthreads();
    if (p < p_hi) {
      rows_to_regs(ra, vrows + (size_t)(p + 1) * NB, t.np, rows_valid, tid);
      tile_to_regs(rt, xtile(p + 1), NB, NB, tid);
    }
    gemm_32x64<!kBack>(as, bs, wave, lane, acc);       // forward: . X_cp^T ; backward: . X_pc
    __syncthreads();
  }
  const int ccol = 16 * wave + (lane & 15);
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * s + (lane >> 4) + 4 * r;
      if (row < rows_valid) orows[(long long)row * t.np + (size_t)c * NB + ccol] = acc[s][r];
    }
}

// The tiles beyond take the solved 256-block's update.
//   forward (tile i > the block):   b_i -= sum_p y_p L[i][4 kb + p]^T
//   backward (tile mm < the block): y_mm -= sum_p w_p L[4 kb + p][mm]
// grid: (tiles to update, n_lambda, row chunks)
template <bool kBack>
__global__ __launch_bounds__(256) void loso_big_update_kernel(LosoBig t) {
  __shared__ double as[kLosoRows * LS];
  __shared__ double bs[NB * LS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lam = blockIdx.y, chunk = blockIdx.z;
  const int bi = kBack ? (int)blockIdx.x : kBig * t.kb + t.m + (int)blockIdx.x;
  const int r0 = chunk * kLosoRows;
  const int rows_valid = t.rows_per_lambda - r0 < kLosoRows ? t.rows_per_lambda - r0 : kLosoRows;
  double* vrows = t.v + ((long long)lam * t.rows_per_lambda + r0) * t.np;
  const double* srows = t.out + ((long long)lam * t.rows_per_lambda + r0) * t.np + (size_t)kBig * t.kb * NB;
  const double* lmat = t.l + (size_t)lam * t.np * t.np;
  auto ltile = [&](int p) {
    const int kk = kBig * t.kb + p;
    return kBack ? lmat + (size_t)kk * NB * t.np + (size_t)bi * NB : lmat + (size_t)bi * NB * t.np + (size_t)kk * NB;
  };
  f64x4 acc[2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[s][r] = 0.0;
  double ra[8];
  f64x2 rt[8];
  rows_to_regs(ra, srows, t.np, rows_valid, tid);
  tile_to_regs(rt, ltile(0), t.np, NB, tid);
  for (int p = 0; p < t.m; ++p) {
    rows_regs_to_lds(as, ra, tid);
    regs_to_lds(bs, rt, tid);
    __syncthreads();
    if (p + 1 < t.m) {
      rows_to_regs(ra, srows + (size_t)(p + 1) * NB, t.np, rows_valid, tid);
      tile_to_regs(rt, ltile(p + 1), t.np, NB, tid);
    }
    gemm_32x64<!kBack>(as, bs, wave, lane, acc);
    __syncthreads();
  }
  const int ccol = 16 * wave + (lane & 15);
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * s + (lane >> 4) + 4 * r;
      if (row < rows_valid) vrows[(long long)row * t.np + (size_t)bi * NB + ccol] -= acc[s][r];
    }
}

}  // namespace

void loso_matvec(td_handle* h, const double* a, const double* p, double* q, const double* inv_n,
                 const double* lams, int n, int np, int folds, int n_lambda, int d) {
  LosoMatvec mv;
  mv.a = a; mv.p = p; mv.q = q; mv.inv_n = inv_n; mv.lams = lams;
  mv.n = n; mv.np = np; mv.folds = folds; mv.n_lambda = n_lambda; mv.d = d;
  const dim3 grid((unsigned)(np / NB), (unsigned)folds, (unsigned)td_ceil_div(n_lambda * d, kLosoRows));
  hipLaunchKernelGGL(loso_matvec_kernel, grid, dim3(256), 0, h->stream, mv);
}

void chol_big_inverses(td_handle* h, const double* l, const double* linv, double* xinv, int np, int n_lambda) {
  const int nblk = np / NB, nbig = (int)td_ceil_div(nblk, kBig);
  hipLaunchKernelGGL(loso_binv_kernel, dim3((unsigned)nbig, (unsigned)n_lambda, kBig), dim3(256), 0, h->stream, l,
                     linv, xinv, np, nblk, nbig);
}

void chol_big_substitute(td_handle* h, const double* l, const double* xinv, int np, int n_lambda,
                         int rows_per_lambda, double* v, double* y, double* z) {
  const int nblk = np / NB, nbig = (int)td_ceil_div(nblk, kBig);
  const unsigned chunks = (unsigned)td_ceil_div(rows_per_lambda, kLosoRows);
  auto big_m = [&](int kb) { return nblk - kBig * kb < kBig ? nblk - kBig * kb : kBig; };   // 64-blocks of step kb
  LosoBig b;
  b.l = l; b.xinv = xinv; b.np = np; b.nblk = nblk; b.nbig = nbig; b.rows_per_lambda = rows_per_lambda;
  b.v = v; b.out = y;
  for (int kb = 0; kb < nbig; ++kb) {
    b.kb = kb; b.m = big_m(kb);
    hipLaunchKernelGGL(loso_big_solve_kernel<false>, dim3((unsigned)b.m, (unsigned)n_lambda, chunks), dim3(256), 0,
                       h->stream, b);
    const int beyond = nblk - kBig * kb - b.m;
    if (beyond > 0)
      hipLaunchKernelGGL(loso_big_update_kernel<false>, dim3((unsigned)beyond, (unsigned)n_lambda, chunks),
                         dim3(256), 0, h->stream, b);
  }
  b.v = y; b.out = z;
  for (int kb = nbig - 1; kb >= 0; --kb) {
    b.kb = kb; b.m = big_m(kb);
    hipLaunchKernelGGL(loso_big_solve_kernel<true>, dim3((unsigned)b.m, (unsigned)n_lambda, chunks), dim3(256), 0,
                       h->stream, b);
    if (kb > 0)
      hipLaunchKernelGGL(loso_big_update_kernel<true>, dim3((unsigned)(kBig * kb), (unsigned)n_lambda, chunks),
                         dim3(256), 0, h->stream, b);
  }
}

// ---- Cholesky whitening for the CCA dense stage (eig.hip: td_cca_solve) -------------------------
// C = L L^T of one n x n system with up to 64 forward right-hand sides given as ROWS (bt [nb][n] =
// B^T): afterwards st->rt holds (L^-1 B)^T as rows of length st->np, and td_chol_back applies
// L^-T to further rows (8 at a time).  `ws` is caller memory of td_chol_ws_bytes(n) bytes.
size_t td_chol_ws_bytes(int n) {
  const size_t np = (size_t)td_round_up(n, NB), nblk = np / NB;
  return sizeof(double) * (np * np + 64 * np + 2 * kMaxRhs * np + nblk * NB * NB + 64) + 1024;
}

__global__ void diag_add_kernel(double* __restrict__ a, int np, int n, double v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[(size_t)i * np + i] += v;
}

// Factors scale * C + diag_shift I (the inertia test of td_cca_solve uses a negative shift; the wide
// ridge solve of solve.hip scale = 1 / frames and shift = lambda).
int td_chol_factor(td_handle* h, void* ws, const double* c_dev, int n, const double* bt_dev, int nb,
                   td_chol_state* st, double diag_shift, double scale) {
  TD_REQUIRE(h, n > 0 && nb >= 0 && nb <= 64, "td_chol_factor: bad sizes");
  const int np = (int)td_round_up(n, NB);
  char* p = reinterpret_cast<char*>(ws);
  st->n = n; st->np = np;
  st->a = reinterpret_cast<double*>(p);     p += sizeof(double) * (size_t)np * np;
  st->rt = reinterpret_cast<double*>(p);    p += sizeof(double) * (size_t)64 * np;
  st->rt8 = reinterpret_cast<double*>(p);   p += sizeof(double) * (size_t)kMaxRhs * np;
  st->sol = reinterpret_cast<double*>(p);   p += sizeof(double) * (size_t)kMaxRhs * np;
  st->linv = reinterpret_cast<double*>(p);  p += sizeof(double) * (size_t)(np / NB) * NB * NB;
  st->tol = reinterpret_cast<double*>(p);
  pad_systems(h, c_dev, 0LL, n, n, np, scale, nullptr, st->a, 1);
  if (diag_shift != 0.0)
    hipLaunchKernelGGL(diag_add_kernel, dim3((unsigned)td_ceil_div(n, 256)), dim3(256), 0, h->stream, st->a,
                       np, n, diag_shift);
  hipLaunchKernelGGL(pad_rows_kernel, dim3(64), dim3(256), 0, h->stream, bt_dev, nb, n, 64, np, st->rt);
  TD_TRY(chol_factor_forward(h, st->a, st->rt, st->sol, st->linv, st->tol, np, nb > 0 ? nb : 1, 1,
                             nullptr, 64, n));
  return spd_check_flag(h);            // TD_ERR_SINGULAR: not positive definite (blocking)
}

int td_chol_back(td_handle* h, const td_chol_state* st, const double* ut_dev, int nu, double* xt_dev) {
  for (int q0 = 0; q0 < nu; q0 += kMaxRhs) {
    const int nq = nu - q0 < kMaxRhs ? nu - q0 : kMaxRhs;
    hipLaunchKernelGGL(pad_rows_kernel, dim3(16), dim3(256), 0, h->stream, ut_dev + (size_t)q0 * st->n,
                       nq, st->n, kMaxRhs, st->np, st->rt8);
    TD_TRY(chol_backward(h, st->a, st->rt8, st->sol, st->linv, st->np, nq, 1, kMaxRhs));
    unpad_rows(h, st->sol, nq, st->n, st->np, xt_dev + (size_t)q0 * st->n, 16);
  }
  TD_HIP(h, hipGetLastError());
  return TD_OK;
}

// The batched factorisation and the backward substitution for callers that fill the padded buffers
// themselves (cca_sweep.hip): a [batch][np][np], rt / sol [batch][rt_rows][np], linv [batch][np / 64][64][64],
// tol [batch].  Up to 64 right-hand-side rows ride along the factorisation; the backward pass takes at most 8.
// A non-positive pivot sets the handle's flag only: the caller looks at each system's own pivots.
int td_chol_batch_forward(td_handle* h, double* a_dev, double* rt_dev, double* linv_dev, double* tol_dev, int np,
                          int n_real, int nrhs, int batch, int rt_rows) {
  TD_REQUIRE(h, np % NB == 0 && nrhs > 0 && nrhs <= 64 && nrhs <= rt_rows && batch > 0, "td_chol_batch_forward: bad sizes");
  return chol_factor_forward(h, a_dev, rt_dev, nullptr, linv_dev, tol_dev, np, nrhs, batch, nullptr, rt_rows, n_real);
}

int td_chol_batch_backward(td_handle* h, double* a_dev, double* rt_dev, double* sol_dev, double* linv_dev, int np,
                           int nrhs, int batch, int rt_rows) {
  TD_REQUIRE(h, np % NB == 0 && nrhs > 0 && nrhs <= kMaxRhs && nrhs <= rt_rows && batch > 0,
             "td_chol_batch_backward: bad sizes");
  return chol_backward(h, a_dev, rt_dev, sol_dev, linv_dev, np, nrhs, batch, rt_rows);
}

extern "C" {

int td_spd_solve(td_handle* h, double* a_dev, double* rhs_dev, int n, int nrhs, int batch) {
  if (!h || !a_dev || !rhs_dev) return td_fail(h, TD_ERR_INVALID, "td_spd_solve: NULL argument");
  TD_REQUIRE(h, n > 0 && batch > 0, "td_spd_solve: empty problem");
  TD_REQUIRE(h, nrhs > 0 && nrhs <= kMaxRhs, "td_spd_solve: nrhs must be in [1, %d], not %d",
             kMaxRhs, nrhs);
  const int np = (int)td_round_up(n, NB);
  void* base = nullptr;
  TD_TRY(td_workspace(h, carve(nullptr, np, batch).bytes, &base));
  const SolveWs w = carve(base, np, batch);
  pad_systems(h, a_dev, (long long)n * n, n, n, np, 1.0, nullptr, w.a, batch, rhs_dev, (long long)n * nrhs, nrhs,
              w.rt);
  TD_TRY(spd_solve_padded(h, w.a, w.rt, w.sol, w.linv, w.tol, np, n, nrhs, batch));
  hipLaunchKernelGGL(unpad_sol_kernel, dim3(16, (unsigned)batch), dim3(256), 0, h->stream, w.sol, n,
                     nrhs, np, rhs_dev);
  TD_HIP(h, hipGetLastError());
  return spd_check_flag(h);
}

}  // extern "C"
