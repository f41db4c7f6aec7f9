// Host functions of the solvers that cross their files: chol.hip (the blocked float64 Cholesky and the padded
// batch of systems it works on), solve.hip (the ridge routes) and loso.hip (the leave-one-out sweep).  Internal to
// the library, not part of its interface (include/td_hotpath.h); eig.hip and cca_sweep.hip reach the factorisation
// through the td_chol_* functions of td_common.h.
#ifndef TD_SOLVE_COMMON_H_
#define TD_SOLVE_COMMON_H_

#include "stats_common.h"
#include "td_common.h"
#include "td_tile64.h"

constexpr int kMaxRhs = 8;      // right-hand-side rows a system carries through the batched solver
constexpr int kLosoRows = 32;   // leave-one-out sweep: right-hand-side rows per workgroup
constexpr int kBig = 4;         // ... and 64-blocks per step of the preconditioner's substitutions (chol.hip)

// ---- chol.hip ----------------------------------------------------------------------------------------------------
// workspace layout for a batch of padded systems
struct SolveWs {
  double* a; double* rt; double* sol; double* linv; double* lams; double* tol;
  size_t bytes;
};
SolveWs carve(void* base, int np, int batch);

// The padded batch of systems from dense moments: a_dst [batch][np][np] = src_b * scale + lambdas[b] I (identity
// beyond n; lambdas may be null; src_b = src + b * src_batch_stride, rows src_ld apart -- stride 0: one matrix for
// the whole batch) and, with rhs, rt_dst [batch][kMaxRhs][np] = scale * rhs_b^T (rhs_b [n][nrhs]), zero padded.
// Launches only: the caller looks at hipGetLastError behind its own launches.
void pad_systems(td_handle* h, const double* src, long long src_batch_stride, int src_ld, int n, int np,
                 double scale, const double* lambdas, double* a_dst, int batch, const double* rhs = nullptr,
                 long long rhs_batch_stride = 0, int nrhs = 0, double* rt_dst = nullptr);
// dst [nb][n] = the first n numbers of the rows of src [nb][np], on `blocks` workgroups
void unpad_rows(td_handle* h, const double* src, int nb, int n, int np, double* dst, int blocks);

// Factorisation with the forward substitution of the right-hand-side rows; see chol.hip.
int chol_factor_forward(td_handle* h, double* a_dev, double* rt_dev, double* sol_dev, double* linv_dev,
                        double* tol_dev, int n, int nrhs, int batch, int* flag_dev, int rt_rows, int n_real);
// ... and the backward substitution behind it, for systems with kMaxRhs right-hand-side rows.  flag_dev: null =
// the handle's flag (spd_check_flag reads it), else the caller's device int.
int spd_solve_padded(td_handle* h, double* a_dev, double* rt_dev, double* sol_dev, double* linv_dev,
                     double* tol_dev, int n, int n_real, int nrhs, int batch, int* flag_dev = nullptr);
// Waits for the stream; TD_ERR_SINGULAR ("Singular matrix") when the handle's flag is set.
int spd_check_flag(td_handle* h);

// The tile kernels of the leave-one-out sweep (loso.hip), which live with the factorisation's (see chol.hip).
// q_row = inv_n[f] * (p_row . A_f) + lambda * p_row for the rows [lambda][output][fold] of np numbers; a
// [folds][n][np] the folds' dense moments.
void loso_matvec(td_handle* h, const double* a, const double* p, double* q, const double* inv_n,
                 const double* lams, int n, int np, int folds, int n_lambda, int d);
// The factors as a preconditioner of many rows, in steps of kBig 64-blocks.  l
// [n_lambda][np][np] and linv are what chol_factor_forward left; xinv [n_lambda][ceil(np / 64 / kBig)][16][64][64]
// receives the inverses of the 256-blocks (once per factorisation).
void chol_big_inverses(td_handle* h, const double* l, const double* linv, double* xinv, int np, int n_lambda);
// z = (L L^T)^-1 v for rows_per_lambda rows of np numbers per lambda: forward from v (overwritten) into y, backward
// from y (overwritten) into z.
void chol_big_substitute(td_handle* h, const double* l, const double* xinv, int np, int n_lambda,
                         int rows_per_lambda, double* v, double* y, double* z);

// ---- solve.hip ---------------------------------------------------------------------------------------------------
// Every statistics object of stats[0 .. count) is there and has the layout (k1, d); with `empty`, every one holds
// data too (`empty` is then the TD_ERR_STATE message, complete).  `who` starts the other messages ("<who>: NULL
// statistics", "<who>: layouts differ"); per object the checks run in that order.  frames_out (may be null)
// receives each object's frame count.
int stats_layouts_agree(td_handle* h, td_stats* const* stats, int count, int k1, int d, const char* who,
                        const char* empty, int64_t* frames_out);

#endif  // TD_SOLVE_COMMON_H_
