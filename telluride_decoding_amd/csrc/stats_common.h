// The statistics object and what its four files share:
//   stats.hip             the object's life cycle, its layout as the solvers see it
//   stats_accumulate.hip  the accumulate routes and the finalize launch
//   stats_moments.hip     the expansion into dense moments
//   stats_exchange.hip    combine / pack / unpack
//
// Device-resident sufficient statistics of lagged regression / CCA inputs
// (SURVEY.md 8a rows A1+A2, A4's accumulate) and their expansion into the dense
// moment matrices the reference accumulates literally.
//
// Identity used (x~ = stream zero-extended outside its file; a = l - pre the
// signed lag of lagged column block l; N' = rows of the file that enter the
// sums, N' <= file length because of batch(drop_remainder) / input_offset):
//
//   M[(la,i),(lb,j)] = sum_{t=0}^{N'-1} A~[t+a][i] B~[t+b][j]
//                    = G'[e][i][j] + corr(a, e)[i][j],          e = b - a,
//   G'[e]      = sum_{u=0}^{N'-1} A~[u]^T B~[u+e]               (lagcov.hip)
//   corr(a>0)  = - sum_{u=0}^{a-1} P[u][e] + sum_{u=N'}^{N'+a-1} P[u][e]
//   corr(a<0)  = - sum_{u=N'+a}^{N'-1} P[u][e],   P[u][e] = A~[u]^T B~[u+e].
//
// The corrections only touch <= max(pre, post) samples at each end of each
// file; those samples are kept in small per-file "boundary windows", so the
// statistics stay compact (C x C x L instead of (C L)^2) and additive over
// files, ranks and subjects.
#pragma once
#include <vector>

#include "td_common.h"

struct td_stats {
  int c1 = 0, pre1 = 0, post1 = 0, c2 = 0, pre2 = 0, post2 = 0, d = 0;
  int l1 = 0, l2 = 0, k1 = 0, k2 = 0, hw = 0;  // hw: half width of a boundary window
  // One device block of doubles, in this order (offsets below):
  //   fxx [l1][c1][c1]            e = 0..l1-1            (A = B = x)
  //   gxo [l1][d+1][c1]           e = -pre1..post1       (A = [y | 1], B = x)
  //   sy  [d]  and  n [1]         sum of y rows, frame count
  //   fyy [l2][c2][c2]            e = 0..l2-1            (A = B = x2)
  //   gxy [l1+l2-1][c1][c2]       e = -(post1+pre2)..(pre1+post2)   (A = x, B = x2)
  //   gyo [l2][1][c2]             e = -pre2..post2       (A = [1], B = x2)
  double* g = nullptr;
  int64_t off_fxx = 0, off_gxo = 0, off_sy = 0, off_n = 0, off_fyy = 0, off_gxy = 0,
          off_gyo = 0, g_len = 0;
  // Boundary windows, float32: [file][2 (head, tail)][2*hw][c].  Head row r holds
  // x~[r - hw]; tail row r holds x~[N' + r - hw].
  float* win1 = nullptr;
  float* win2 = nullptr;
  int64_t n_files = 0, cap_files = 0;
  int64_t frames = 0;
  // Every file so far was summed whole -- rows [0, N') with N' = the rows that exist, both ends owned:
  // its tail window holds zeros from row hw on and the moment matrix is block-Toeplitz but for the
  // HEAD windows (td_stats_compact: the solver that works on the compact statistics).  False after a
  // dropped remainder, a time range, an input offset that leaves rows behind the sums, an unpack or a
  // combine (conservative: their sources are not inspected).
  bool whole_files = true;
  // A reset that has not been written yet (regression statistics only, see stats_fusable): the
  // next accumulate call's finalize launch OVERWRITES its half of `g` instead of adding to it --
  // `fresh_main` covers fxx and n, `fresh_tgt` gxo and sy -- and no memset is queued.  Every
  // other reader of `g` calls stats_materialize first.
  bool fresh_main = false, fresh_tgt = false;
  // Channel maxima measured by a TARGETS call that runs AHEAD of the MAIN call of the same files
  // (TD_ACC_TARGETS_FIRST: pipelined fits take the HBM-bound targets pass off the stream the matrix
  // kernel runs on): the float16 lag kernel of that MAIN call scales by them, from whichever handle.
  unsigned* chan_tab = nullptr;
  bool tab_ready = false;
  // A finalize launch left pending by an accumulate call with TD_ACC_DEFER (td_stats_complete queues it):
  // its parameter block and its grid; the partial slabs, the file table and the
  // channel scales it reads live in blocks this object owns (the handle's scratch belongs to the next call).
  bool pending = false;
  std::vector<char> pend_params;
  int pend_blocks = 0;
  void* dscratch = nullptr;
  size_t dscratch_bytes = 0;
  void* djobs = nullptr;
  size_t djobs_bytes = 0;
  std::vector<char> djobs_host;   // what djobs holds (uploads of an unchanged table are skipped)
  unsigned* dscale = nullptr;     // [128] the float16 kernel's combined channel-maximum row of that call
};

// The shape whose accumulate runs as matrix kernels + ONE finalize launch (accumulate_fused):
// regression statistics (no second view), up to 64 channels and 32 lags, 1..4 target columns.
inline bool stats_fusable(const td_stats* s) {
  return s->c2 == 0 && s->d >= 1 && s->d <= 4 && s->c1 <= 64 && s->l1 <= 32;
}

// CCA without context on either input and without targets: every moment is one Gram matrix of
// [x | x2 | 1] (td_gram), whose reduction can overwrite fresh statistics as well.
inline bool stats_one_pass(const td_stats* s) {
  return s->c2 > 0 && s->d == 0 && s->l1 == 1 && s->l2 == 1 && s->c1 <= 64 && s->c2 <= 31;
}

// Floats of one file's boundary windows of a view of c channels: [2 (head, tail)][2 hw][c].
inline int64_t stats_window_floats(const td_stats* s, int c) { return (int64_t)2 * 2 * s->hw * c; }

// stats.hip.  Writes a pending reset (see td_stats::fresh_*): the part of `g` nobody has overwritten yet is
// zeroed on the handle's stream.  main = [0, off_gxo) + [off_n, g_len), targets = [off_gxo, off_n).
int stats_materialize(td_handle* h, td_stats* s);
// Room for the boundary windows of `need` files (the windows held so far are kept).
int ensure_window_capacity(td_handle* h, td_stats* s, int64_t need);

// The layout as the solvers see it (solve.hip, loso.hip, eig.hip, cca_sweep.hip).
int td_stats_layout(const td_stats* s, int* k1, int* d, int64_t* frames);
int td_stats_dims(const td_stats* s, int* k1, int* k2, int64_t* frames);
int td_stats_cca_direct(td_handle* h, td_stats* s, const double** xx, const double** yy, const double** xy,
                        const double** sum1, const double** sum2, int* ok);
