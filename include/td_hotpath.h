/*
 * td_hotpath.h -- C-ABI of the MI355X-native linear auditory-attention-decoding
 * hot path (ridge TRF fit, CCA moments/transform, windowed correlation,
 * attended-speaker decision).
 *
 * The reference (google/telluride_decoding v2.1.6) is pure Python and has no
 * FFI of its own: the boundary is the Python call
 * surface of the functions cited next to each entry point below.  This header
 * is what a ctypes (or cgo / JNI) binding of that surface binds; see
 * INTEGRATION.md for the binding a reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - Every function returns TD_OK (0) or a negative td_status; the message is
 *     available from td_last_error().  No exceptions cross the ABI.
 *   - Pointers named *_dev are DEVICE addresses (hipMalloc / td_malloc / a
 *     torch tensor's data_ptr()).  Pointers named *_host are host addresses.
 *   - All matrices are row-major, time x feature ("num_frames x num_channels",
 *     reference result_store.py:43-44, infer_decoder.py:296-297); `ld*` is the
 *     row stride in ELEMENTS.
 *   - Several recordings ("files", "trials") are passed concatenated along
 *     time with a host array file_offsets[F+1] of row offsets; temporal
 *     context never crosses a file boundary (reference brain_data.py:722-724).
 *   - All work is stream-ordered on the handle's stream (td_set_stream adopts an
 *     external hipStream_t, e.g. torch's current stream).  One handle per host
 *     thread and GPU; handles are not thread-safe (the reference objects are
 *     not either: SURVEY.md 8b "Threading").
 */
#ifndef TD_HOTPATH_H_
#define TD_HOTPATH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum td_status {
  TD_OK = 0,
  TD_ERR_INVALID = -1,   /* bad argument (Python side raises ValueError/TypeError) */
  TD_ERR_HIP = -2,       /* a HIP runtime call failed */
  TD_ERR_SINGULAR = -3,  /* matrix not positive definite (numpy: LinAlgError)  */
  TD_ERR_NOMEM = -4,
  TD_ERR_STATE = -5      /* call sequence error (e.g. solve before accumulate)  */
} td_status;

typedef struct td_handle td_handle; /* owns stream, workspace, error string */
typedef struct td_stats td_stats;   /* device-resident sufficient statistics */

/* ------------------------------------------------------------------ lifecycle */
int td_version(void);
int td_device_count(int* count);
int td_create(int device_id, td_handle** out);
int td_destroy(td_handle* h);
const char* td_last_error(const td_handle* h); /* h may be NULL: last global */
/* A new handle queues work on a private non-blocking stream.  td_set_stream adopts
 * an external hipStream_t instead (NULL = HIP's default stream, which is what
 * torch.cuda.current_stream().cuda_stream is unless the caller changed it);
 * td_use_own_stream goes back to the private one. */
int td_set_stream(td_handle* h, void* hip_stream);
int td_use_own_stream(td_handle* h);
/* A HIP stream restricted to CUs [cu_first, cu_first + cu_count) of the device
 * (hipExtStreamCreateWithCUMask), for running the latency-bound solve stage beside the
 * throughput-bound accumulate stage of the next fit (pipeline.FitPipeline): a grid
 * that fills every CU otherwise starves the other stream until it has drained.  The
 * reference has no counterpart (single Python thread, regression.py:151-242 refits
 * serially).  *stream_out is a hipStream_t; free it with td_stream_destroy. */
int td_stream_create_masked(int device_id, int cu_first, int cu_count, void** stream_out);
int td_stream_destroy(void* hip_stream);
/* Tells the handle how many CUs its (adopted, CU-masked) stream runs on: the accumulate plans
 * its work items to fill whole rounds of them.  Default: every CU of the device.  No reference
 * counterpart. */
int td_set_cu_count(td_handle* h, int cu_count);
/* How the lagged-covariance kernel multiplies float32 numbers (same-stream shapes of 33..64
 * channels; everything else is float32 MFMA).  The reference multiplies in float32
 * (brain_model.py:437, np.matmul); all three modes are closer to exact arithmetic than that:
 *   TD_ACC_F16X2  (default) two float16 pieces per number, per-channel power-of-two scales, three
 *                 products on the float16 matrix pipe: sums of squares come out ~5e-8 low (the
 *                 pipe truncates 22-bit products when it aligns them), everything else zero-mean;
 *   TD_ACC_BF16X3 three bfloat16 pieces, six products: exact to 2^-27 per product, 1.6x the time;
 *   TD_ACC_F32    the float32 matrix instruction: 3x the time. */
enum { TD_ACC_F16X2 = 0, TD_ACC_BF16X3 = 1, TD_ACC_F32 = 2 };
int td_set_accumulate_mode(td_handle* h, int mode);
int td_synchronize(td_handle* h);

/* Device memory helpers for callers that do not bring their own allocator. */
int td_malloc(td_handle* h, size_t bytes, void** dev_ptr);
int td_free(td_handle* h, void* dev_ptr);
int td_memcpy_h2d(td_handle* h, void* dst_dev, const void* src_host, size_t bytes);
int td_memcpy_d2h(td_handle* h, void* dst_host, const void* src_dev, size_t bytes);
int td_memset(td_handle* h, void* dst_dev, int value, size_t bytes);

/* hipEvent timing on the handle's stream (bench.py's roofline leg). */
int td_timer_start(td_handle* h);
int td_timer_stop(td_handle* h, float* elapsed_ms); /* synchronises the stop event */
/* Per-launch hipEvent timing of the DOMINANT kernel (the lagged-covariance MFMA
 * accumulate): while enabled every launch is bracketed by two events on the
 * handle's stream; td_profile_read synchronises, returns the number of launches,
 * their summed duration and the samples they covered, and resets the counters. */
int td_profile_enable(td_handle* h, int on);
int td_profile_read(td_handle* h, int64_t* launches, double* total_ms, double* samples);
/* Measurement aid: the rate (TFLOP/s) a bare register-only loop of v_mfma_f32_32x32x16_bf16
 * sustains on the handle's CUs for ~1 ms -- the practical ceiling of the bf16x3 accumulate, which
 * is power-bound.  split_shaped = 0: all-zero operands; 1: random operands with the magnitudes
 * of the three bf16 pieces of a float32.  Blocking.  No reference counterpart. */
int td_probe_bf16_mfma(td_handle* h, int split_shaped, double* tflops);

/* ------------------------------------------------------------------ A1 + A2
 * Sufficient statistics of lagged regression / CCA inputs WITHOUT building the
 * lag matrix.  Replaces, per file, the context builder
 *   brain_data.BrainData.add_temporal_context (brain_data.py:425-483)
 * and the accumulate loops of
 *   brain_model.calculate_linear_regressor_parameters_from_dataset
 *       (brain_model.py:422-446: sum_xtx, sum_x, sum_xty, num_samples) and
 *   cca.calculate_cca_parameters_from_dataset (cca.py:304-332: cov_xx, cov_yy,
 *       cov_xy, sum_x, sum_y, total_frames).
 *
 * Feature layout (the numerical contract): lagged column l*C + c of input_1
 * holds x~[t + l - pre, c], x~ zero outside the file (brain_data.py:448-454).
 *
 *   c1,pre1,post1 : input_1 ("x", EEG) channels and context
 *   c2,pre2,post2 : input_2 (CCA second view); c2 = 0 when unused
 *   d             : width of the regression target y; d = 0 when unused
 */
int td_stats_create(td_handle* h, int c1, int pre1, int post1, int c2, int pre2,
                    int post2, int d, td_stats** out);
/* Stream-ordered and non-blocking: the memory returns to the device's pool after the work
 * queued so far on h's stream and on the streams of the process's other handles. */
int td_stats_destroy(td_handle* h, td_stats* s);
int td_stats_reset(td_handle* h, td_stats* s);

/* Adds F files.  x_dev[rows, c1] (ld ldx), x2_dev[rows, c2] or NULL,
 * y_dev[rows, d] or NULL; rows = file_offsets_host[F].
 * input_offset > 0 drops that many leading rows of x, < 0 of x2 and y
 * (brain_data.py:466-475).  rows_used_host[F] (may be NULL = all) gives, per
 * file, how many rows of the zipped streams enter the sums: the caller uses it
 * to reproduce batch(drop_remainder=True) (brain_data.py:369-370), which drops
 * the tail of the LAST file only. */
int td_stats_accumulate(td_handle* h, td_stats* s, const float* x_dev, int64_t ldx,
                        const float* x2_dev, int64_t ldx2, const float* y_dev,
                        int64_t ldy, const int64_t* file_offsets_host, int num_files,
                        int input_offset, const int64_t* rows_used_host);
/* The same in two independently schedulable parts, for callers that pipeline fits on two
 * streams (pipeline.FitPipeline): TD_ACC_MAIN = boundary windows, the lagged auto- and
 * cross-covariances (the matrix-core kernel) and the frame / file counters;
 * TD_ACC_TARGETS = [y | 1]^T x~ (Xty, the bias moments, sum y) and the lagged column sums of
 * input_2.  Both parts of a call take identical arguments; TARGETS must be ordered after
 * MAIN of the same files (it reads their boundary windows).  parts = 3 is
 * td_stats_accumulate.
 * TD_ACC_TARGETS | TD_ACC_TARGETS_FIRST (regression statistics): the targets part AHEAD of the MAIN
 * call of the same files, possibly on another handle / stream -- it streams every row the matrix
 * kernel will read (HBM-bound, ~65 us at C2) and also measures the channel maxima the float16
 * accumulate scales by, leaving them in the statistics object; the MAIN call that follows (ordered
 * after it by the caller: an event) then starts its matrix kernel at once.  A pipeline runs
 * targets(i + 1) beside the matrix kernel of fit i this way (pipeline.FitPipeline). */
#define TD_ACC_MAIN 1
#define TD_ACC_TARGETS 2
#define TD_ACC_TARGETS_FIRST 4
/* parts = TD_ACC_MAIN [| TD_ACC_TARGETS] | TD_ACC_DEFER (regression statistics): the call queues its
 * matrix and targets kernels and leaves the FINALIZE launch -- the float64 reduction of their partial sums
 * into the statistics, the boundary windows, the bias moments: ~35 us of a 0.85 ms C2 fit, the last link of
 * the accumulate stream's chain -- pending.  td_stats_complete(h2, s) queues it on h2's stream, which the
 * caller has ordered behind this call (an event: as for every use of s from another stream), so a pipeline
 * hands it to the stream that solves the fit and the accumulate stream starts the next fit's kernels at
 * once (pipeline.FitPipeline: 0.86 -> 0.84 ms per pipelined C2 fit).  Until the completion has run the
 * caller keeps x / y in place (the finalize reads the recordings' ends) and does not accumulate into s
 * again from another stream; every other entry point that reads or changes s completes a pending
 * finalize on its own handle's stream first, so forgetting the call costs overlap, not correctness.
 * Shapes the deferral does not cover finalize inside the call as without the flag. */
#define TD_ACC_DEFER 8
int td_stats_complete(td_handle* h, td_stats* s);
int td_stats_accumulate_parts(td_handle* h, td_stats* s, const float* x_dev, int64_t ldx,
                              const float* x2_dev, int64_t ldx2, const float* y_dev,
                              int64_t ldy, const int64_t* file_offsets_host, int num_files,
                              int input_offset, const int64_t* rows_used_host, int parts);

/* The per-recording statistics of a leave-one-out sweep in one call (regression.jackknife_one_model,
 * regression.py:151-242, refits on all files but one: every recording's statistics are needed on their own):
 * the files of x / y as in td_stats_accumulate, but file f is summed into each[f] -- freshly created or reset
 * regression statistics of one layout -- by ONE targets launch and ONE matrix launch over all the recordings
 * and ONE finalize launch over all of them.  (The float16 matrix kernel scales a channel by its largest magnitude
 * over ALL the recordings of the call: a recording whose amplitude is below 2^-9 of the largest one's loses low
 * bits of its second piece -- 3 bits at a ratio of 1e-6; accumulate such recordings on their own.)
 * *handled = 0: a shape this form does not take (<= 32 or > 64
 * channels, statistics that already hold data); nothing was queued, call td_stats_accumulate per file. */
int td_stats_accumulate_each(td_handle* h, td_stats* const* each, const float* x_dev, int64_t ldx,
                             const float* y_dev, int64_t ldy, const int64_t* file_offsets_host, int num_files,
                             int input_offset, const int64_t* rows_used_host, int* handled);

/* The same for callers that share ONE long recording between ranks by time range
 * (third unit): the moments are sums over rows, so a call may sum only the rows
 * [range_begin[f], range_end[f]) of file f's zipped stream.  A "file" here is the piece of the
 * recording the caller holds: its range plus a read-only halo of pre + post rows on either
 * side (clipped at the true ends), so that x~[u + lag] is real data at an interior cut and zero
 * only beyond a true end of the recording (brain_data.py:448-454).  edge_flags[f]: bit 0 =
 * the piece starts at the recording's first row, bit 1 = it ends at its last row -- only that
 * piece contributes the head / tail boundary window (the edge corrections of the dense
 * moments and the bias moments are linear in them, so the sum over ranks is exact).
 * rows_used[f] counts rows of the PIECE (the tail piece applies drop_remainder).  Ranks map a
 * shared recording to the same boundary slot of the packed all-reduce buffer.  NULL ranges =
 * whole files, NULL flags = both ends: td_stats_accumulate_parts.  input_offset must be 0. */
int td_stats_accumulate_ranges(td_handle* h, td_stats* s, const float* x_dev, int64_t ldx,
                               const float* x2_dev, int64_t ldx2, const float* y_dev,
                               int64_t ldy, const int64_t* file_offsets_host, int num_files,
                               int input_offset, const int64_t* rows_used_host,
                               const int64_t* range_begin_host, const int64_t* range_end_host,
                               const int* edge_flags_host, int parts);

/* Frames summed so far (num_samples / total_frames) and number of files. */
int td_stats_counts(td_handle* h, const td_stats* s, int64_t* frames, int64_t* files);

/* Additive algebra for sharding and leave-one-out sweeps
 * (regression.py:151-242): dst = sum_i srcs[i].  All must share one layout. */
int td_stats_combine(td_handle* h, td_stats* dst, td_stats* const* srcs, int n);

/* Packed form for ONE all-reduce(sum) over ranks: doubles.  Every rank packs
 * its own statistics; file-boundary samples go to the slot range
 * [file_slot, file_slot + own files) of total_file_slots so that the sum over
 * ranks is the concatenation. */
int td_stats_packed_len(td_handle* h, const td_stats* s, int64_t total_file_slots,
                        int64_t* num_doubles);
int td_stats_pack(td_handle* h, const td_stats* s, double* buf_dev,
                  int64_t total_file_slots, int64_t file_slot);
int td_stats_unpack(td_handle* h, td_stats* s, const double* buf_dev,
                    int64_t total_file_slots);
/* The same without the device-to-host read of the frame count (which synchronises the
 * stream): the caller states the total number of frames of all ranks. */
int td_stats_unpack_known(td_handle* h, td_stats* s, const double* buf_dev,
                          int64_t total_file_slots, int64_t total_frames);

/* The exchange step of a multi-GPU fit (SURVEY.md 8e, 8b(3) "stats_allreduce(handle, rccl_comm)"):
 * pack -> ONE ncclAllReduce(sum, float64) over `rccl_comm` (an ncclComm_t) -> unpack, all
 * queued on the handle's stream; nothing waits on the host when total_frames (the frames of all
 * ranks; < 0: read back from the reduced buffer) is given.  Afterwards every rank holds the
 * statistics of all recordings.  total_file_slots / file_slot as in td_stats_pack.  The
 * reference has no counterpart: it fans out OS processes per (lambda, held-out file) and refits
 * from scratch (doc/DecodingCodelab.md:354-381, regression.py:381-409).
 * RCCL is bound at run time (dlopen; TD_RCCL_LIB overrides the path; inside a PyTorch process
 * the librccl PyTorch mapped is used), so a binding needs no torch and a single-GPU user no RCCL. */
int td_stats_allreduce(td_handle* h, td_stats* s, void* rccl_comm, int64_t total_file_slots,
                       int64_t file_slot, int64_t total_frames);
/* In-place all-reduce(sum) of a float64 device buffer on the handle's stream (the per-recording
 * statistics table of the leave-one-out sweep, regression.py:326-420). */
int td_allreduce_f64(td_handle* h, double* buf_dev, int64_t count, void* rccl_comm);
/* Communicator plumbing for callers that have no ncclComm_t of their own: rank 0 makes a
 * 128-byte id (ncclGetUniqueId), hands it to the other ranks by any means, then every rank
 * creates its communicator on the handle's device (ncclCommInitRank; collective). */
/* TD_OK when librccl can be bound in this process (dlopen + the six symbols; no RCCL call is made --
 * ncclGetUniqueId would start a bootstrap thread and socket), TD_ERR_STATE with the reason otherwise. */
int td_rccl_available(td_handle* h);
int td_rccl_unique_id(td_handle* h, void* id_out_128);
int td_rccl_comm_create(td_handle* h, int num_ranks, int rank, const void* id_128, void** comm_out);
int td_rccl_comm_count(td_handle* h, void* comm, int* num_ranks);
int td_rccl_comm_destroy(td_handle* h, void* comm);

/* Dense moment matrices (float64, device), expanded from the compact lag
 * statistics with exact file-edge corrections.  k1 = c1*(pre1+1+post1),
 * k2 = c2*(pre2+1+post2).
 *   xtx_dev [(k1+1) x (k1+1)] : sum_xtx incl. the trailing ones column
 *                               (brain_model.py:434-437)
 *   xty_dev [(k1+1) x d]      : sum_xty (brain_model.py:439)
 *   x2tx2_dev [k2 x k2], xtx2_dev [k1 x k2], sum_x2_dev [k2] : cca.py:325-329
 * Any output pointer may be NULL. */
int td_stats_moments(td_handle* h, td_stats* s, double* xtx_dev, double* xty_dev,
                     double* x2tx2_dev, double* xtx2_dev, double* sum_x2_dev);

/* ------------------------------------------------------------------ A3
 * Ridge solve for a batch of lambdas: cov_x = XtX/n + lambda*I over ALL k1+1
 * diagonal entries incl. the bias (brain_model.py:447-455), then
 * solve(cov_x, cov_xy) (:477).  Float64 Cholesky on the device.
 *   w_dev [n_lambda, k1, d] float32, b_dev [n_lambda, d] float32.
 * Any number of outputs d (up to 8 ride in the batched factorisation; wider targets -- a forward
 * model whose targets are the EEG channels -- are solved one lambda at a time, 64 columns per
 * factorisation).  TD_ERR_SINGULAR when cov_x is not positive definite. */
int td_ridge_solve(td_handle* h, td_stats* s, const double* lambdas_host, int n_lambda,
                   float* w_dev, float* b_dev);
/* How td_ridge_solve solves (brain_model.py:477 is one dense np.linalg.solve):
 *   TD_SOLVER_AUTO (default) a synchronous call with at most 4 (lambda, output) systems of
 *                  n >= 128 / 192 / 512 (one / two / three or four systems: where one launch measures faster than the
 *                  factorisation's chain), every lambda >= 1e-6 trace(cov_x) (condition number <= 1e6: the answer
 *                  stands in for np.linalg.solve, and a residual bound must be a weight bound) runs conjugate
 *                  gradients in ONE persistent launch: with the dense matrix resident in the LDS of the CUs the
 *                  handle runs on when it fits (td_set_cu_count; n = 2049 on the 256 CUs of an MI355X does), else
 *                  -- statistics whose files were summed whole, no pre-context -- on the compact statistics, one
 *                  workgroup per channel (64 CUs suffice).  The blocked Cholesky follows only when that does not
 *                  converge in 160 iterations to a relative residual of 1e-12 (the TRUE residual checked within
 *                  2e-12), meets a non-positive curvature, cannot have all its workgroups resident (asked of the
 *                  runtime BEFORE the launch) or aborts itself (a wait longer than 20 ms: another process's
 *                  persistent grid); everything else takes the Cholesky directly;
 *   TD_SOLVER_CHOLESKY       always the blocked float64 Cholesky (~100 launches per system);
 *   TD_SOLVER_CG             conjugate gradients first for any system count / size that fits (lambda > 0; 400
 *                            iterations, true residual within 1e-11, no conditioning gate for the resident kernel).
 * td_last_solve_info: what the last td_ridge_solve on this handle did -- solver (TD_SOLVER_CHOLESKY or
 * TD_SOLVER_CG), iterations of the slowest system, and the conjugate-gradient status (0 converged,
 * 2 not converged / not positive definite, 3 aborted, 4 not attempted: lambda below 1e-6 trace) when it was
 * tried.  Any pointer may be NULL. */
enum { TD_SOLVER_AUTO = 0, TD_SOLVER_CHOLESKY = 1, TD_SOLVER_CG = 2 };
int td_set_solver(td_handle* h, int mode);
/* Named options of a handle (the library reads no TD_* environment variable except TD_RCCL_LIB):
 *   "cca_whitening"   0 (default) td_cca_solve whitens the large side by its Cholesky factor when the
 *                     inertia certificate allows; 1 = always the eigen-decomposition the reference calls
 *                     (cca.py:345-360);
 *   "cca_fused"       1 (default): td_cca_solve runs the dense stage of a small problem (K1 <= 64, K2 <= 16,
 *                     K2 <= K1) as ONE launch of one workgroup; 0: the chain of launches (A/B runs);
 *   "reserve_workspace"  value = bytes: the handle's workspace arena (dense moments, factors, the folds of a
 *                     leave-one-out sweep: 1.9 GB at C5) is grown to that size NOW -- a hipMalloc of 2 GB takes
 *                     ~55 ms and otherwise lands in the first call that needs it.  The arena never shrinks;
 *   "cg_limit_ticks"  the conjugate-gradient kernel's wait limit per launch in 10 ns ticks (< 0: the
 *                     default, 20 ms; 0: every workgroup gives up at its first empty poll -- the abort /
 *                     drain / Cholesky-fallback route, for tests).
 *   "async_cg"        1: td_ridge_solve_async may solve by conjugate gradients on the compact statistics
 *                     (one launch of one workgroup per channel: fits a 64-CU partition); its flag is
 *                     then 2 when the solver gave up -- the caller solves again (td_ridge_solve) -- as
 *                     well as 0 / 1.  0 (default): the factorisation, flags 0 / 1 only.
 *   "narrow16"        1 (default): regression statistics of <= 16 channels x <= 16 lags are accumulated by
 *                     the one-kernel streaming form (float32 products); 0: the tiled kernels (A/B runs).
 *   "targets_f16"     1 (default): y^T x~ of 33 .. 64 channels per tile (rows of whole 8-byte pairs, <= 32 lags)
 *                     is multiplied as two float16 pieces under per-body scales (lagcov_targets_split_kernel);
 *                     0: the float32 matrix instruction (lagcov_targets_mfma_kernel; A/B runs).
 * Unknown names are TD_ERR_INVALID. */
int td_set_option(td_handle* h, const char* name, int64_t value);
/* Bytes of device memory the handle's kernel scratch arena holds now (it grows to the largest request
 * x 1.25 and never shrinks; the workspace arena of "reserve_workspace" is separate). */
int td_scratch_bytes(td_handle* h, int64_t* bytes);
int td_last_solve_info(td_handle* h, int* solver, int* iterations, int* cg_status);
/* Which conjugate-gradient kernel the last td_ridge_solve / td_ridge_solve_async on this handle LAUNCHED
 * (recorded at the point of launch, cleared at the start of every ridge solve; a launch that then gave up
 * -- td_last_solve_info says 'cholesky' -- is still reported): *kernel TD_CG_KERNEL_NONE / _RESIDENT (dense
 * matrix in LDS) / _COMPACT (compact statistics), *param the rows per workgroup R = 1..8 of the resident
 * kernel or the channels per workgroup 1 / 2 of the compact one (0 for none), *workgroups the grid.  Any
 * pointer may be NULL.  No reference counterpart. */
enum { TD_CG_KERNEL_NONE = 0, TD_CG_KERNEL_RESIDENT = 1, TD_CG_KERNEL_COMPACT = 2 };
int td_last_cg_plan(td_handle* h, int* kernel, int* param, int* workgroups);
/* The same without waiting for the device.  *singular_flag_host points at a pinned host int
 * owned by the handle (a ring of 8: read it before the 8th later call; a call that would reuse a
 * slot whose solve has not finished yet -- more than 8 solves outstanding, nobody can have read
 * that flag -- returns TD_ERR_STATE instead of overwriting it) that becomes 0, or 1 if
 * some cov_x was not positive definite (w_dev / b_dev are then meaningless), or -- only with
 * td_set_option(h, "async_cg", 1) -- 2 if the conjugate-gradient solver gave up, once the work queued
 * by this call has completed -- wait for an event recorded after the call, then read it.  For
 * callers that pipeline fits: a host that waits for every solve cannot queue the next fit's
 * work in time (pipeline.FitPipeline). */
int td_ridge_solve_async(td_handle* h, td_stats* s, const double* lambdas_host, int n_lambda,
                         float* w_dev, float* b_dev, const int** singular_flag_host);

/* Several statistics x several lambdas in one batched factorisation: the folds of a
 * leave-one-file-out sweep (regression.jackknife_one_model / jackknife_over_regularizations,
 * regression.py:151-242, 326-420, refit per (lambda, fold)).  stats_host[n_stats] share one
 * layout.  w_dev [n_stats, n_lambda, k1, d], b_dev [n_stats, n_lambda, d] float32.
 * singular_flag_host NULL: synchronous, TD_ERR_SINGULAR if any system is not positive definite;
 * else as td_ridge_solve_async (one flag for the whole batch). */
int td_ridge_solve_multi(td_handle* h, td_stats* const* stats_host, int n_stats,
                         const double* lambdas_host, int n_lambda, float* w_dev, float* b_dev,
                         const int** singular_flag_host);

/* The same systems for a leave-one-out sweep (regression.jackknife_over_regularizations,
 * regression.py:326-420: fold f = every recording but f, all lambdas) WITHOUT factoring each of
 * them: one Cholesky factor per lambda of the TOTAL covariance + lambda I preconditions a
 * conjugate-gradient solve of every fold's system (the folds' matrices differ from the total's
 * by 1 / folds), all systems in lock step: a [lambda x n] . [n x n] product per fold on the float64
 * MFMA and two blocked triangular substitutions per iteration.  total = statistics of all
 * recordings, folds[f] = training statistics of fold f.  Synchronous.  *status_host = 0: every
 * system converged to the relative residual `tol` (outputs as td_ridge_solve_multi);
 * 1: max_iter iterations were not enough; 2: the preconditioner (total covariance + lambda I) is not
 * positive definite -- in both cases use td_ridge_solve_multi.  iterations_host (may be NULL)
 * receives the iteration count. */
int td_ridge_solve_loso(td_handle* h, td_stats* total, td_stats* const* folds, int n_folds,
                        const double* lambdas_host, int n_lambda, int max_iter, double tol,
                        float* w_dev, float* b_dev, int* status_host, int* iterations_host);

/* The same sweep with the folds given as what they ARE (regression.py:326-420: fold f = every recording but
 * f): fold f = total + sum over t in [term_begin[f], term_begin[f + 1]) of signs[t] * terms[t], signs +1 / -1,
 * at most 4 terms a fold -- minus the held-out recording's statistics; for a fold whose minibatch stream
 * drops a remainder (brain_data.py:369-370) minus the last training recording's and plus the same recording
 * accumulated without its tail.  The statistics are linear in the recordings, so no fold's training
 * statistics are ever summed and the dense moments of ALL folds come from the total's (expanded once, for the
 * preconditioner) in one launch.  term_begin [n_folds + 1].  w_k_major = 1: w_dev is [n_folds][k1][n_lambda][d] --
 * a fold's models as the output columns of ONE filter, the layout td_predict_fir_per_file takes for the held-out
 * evaluation (regression.py:197-214) -- instead of [n_folds][n_lambda][k1][d]; everything else as td_ridge_solve_loso. */
int td_ridge_solve_loso_terms(td_handle* h, td_stats* total, td_stats* const* terms, const int* term_begin,
                              const double* signs, int n_folds, const double* lambdas_host, int n_lambda,
                              int max_iter, double tol, int w_k_major, float* w_dev, float* b_dev,
                              int* status_host, int* iterations_host);

/* The CCA dense stage of a leave-one-file-out x regularisation sweep (regression.py:326-420 over
 * cca.calculate_cca_parameters_from_dataset, cca.py:337-367): one CCA model per (fold, lambda), the folds given as
 * td_ridge_solve_loso_terms takes them (fold f = total + signed terms, at most 4).  fold_batches[f] minibatches of
 * batch_size frames make fold f's training stream: means over fold_batches[f] * batch_size frames (which the fold's
 * statistics must hold), covariances S / (frames - 1) - mean^T mean, + lambda I on BOTH auto-covariances.  The x side
 * is whitened by its Cholesky factor (valid when no eigenvalue of cov_xx is dropped), the other side (k2 <= 64) by
 * the reference's eigen route in one workgroup per pair; no k1-sized eigen-decomposition.  Outputs, float32 on the
 * device: rot_x [n_folds][k1][n_lambda * dim] and rot_y [n_folds][k2][n_lambda * dim] (k-major: a fold's models are
 * the output columns of one filter, what td_predict_fir takes), mean_x [n_folds][k1], mean_y [n_folds][k2], bias_x /
 * bias_y [n_folds][n_lambda * dim] = -mean . rot, e [n_folds][n_lambda][dim] (the canonical correlations,
 * descending); status_dev int32 [n_folds][n_lambda]: 0 solved, 1 = cov_xx + lambda I has no Cholesky factor, an
 * eigenvalue of cov_yy + lambda I is <= eps_eig, or sigma_dim <= 1e-6 sigma_1 -- that pair's outputs are not to be
 * used (td_cca_solve on the fold's summed statistics decides).  Queued on the handle's stream, no wait.
 * TD_ERR_INVALID: k2 > 64, more than 4 terms in a fold, dim outside [1, min(k1, k2)]. */
int td_cca_solve_loso_terms(td_handle* h, td_stats* total, td_stats* const* terms, const int* term_begin,
                            const double* signs, int n_folds, const int64_t* fold_batches, int batch_size,
                            const double* lambdas_host, int n_lambda, int dim, double eps_eig, float* rot_x_dev,
                            float* rot_y_dev, float* mean_x_dev, float* mean_y_dev, float* bias_x_dev,
                            float* bias_y_dev, float* e_dev, int* status_dev);

/* Generic SPD solve used by the above and by the shrinkage branch
 * (brain_model.py:456-477): a_dev [batch, n, n] float64 (destroyed),
 * rhs_dev [batch, n, nrhs] float64 (overwritten with the solution). */
int td_spd_solve(td_handle* h, double* a_dev, double* rhs_dev, int n, int nrhs, int batch);

/* General square solve (np.linalg.solve, brain_model.py:477) for the one branch whose matrix
 * may be indefinite: a negative Ledoit-Wolf shrinkage.  Float64 LU with partial pivoting on
 * the device; a_dev [n, n] is destroyed, rhs_dev [n, nrhs] is overwritten with the solution.
 * TD_ERR_SINGULAR on a zero pivot column.  n <= 16320 (as the Cholesky solves). */
int td_general_solve(td_handle* h, double* a_dev, double* rhs_dev, int n, int nrhs);

/* Ledoit-Wolf moment of the automatic-shrinkage branch (lamb == -1, use_ridge False):
 * np.sum(sum_x2tx2) of brain_model.py:440-443, i.e. the sum over all lagged rows r of
 * (sum_k (X[r,k] - mean_b[k])^2)^2 with mean_b the running column mean after the minibatch
 * that holds r (:441).  The stream is the files' lagged rows (context pre/post, the
 * input_offset / rows_used conventions of td_stats_accumulate) cut into minibatches of
 * batch_rows; a shorter last minibatch is allowed.  result_dev: one float64 on the device,
 * overwritten. */
int td_shrinkage_moment(td_handle* h, const float* x_dev, int64_t ldx, int c, int pre, int post,
                        const int64_t* file_offsets_host, int num_files, int input_offset,
                        const int64_t* rows_used_host, int64_t batch_rows, double* result_dev);

/* The shrinkage algebra of brain_model.py:449-476 on the device.  s_dev [n rows, row stride ld]: float64 moment
 * sums (td_stats_moments: with use_offset n = K + 1 includes the ones row and column), sum_row_dev [n]: the column-sum
 * row of the moments (the ones row), frames: rows summed.  With zc = S - m^T m, m = sum_row / frames ("sum minus mean
 * outer", sic, :450): out_host[0] = trace(zc), out_host[1] = sum(zc^2) -- from which mu = trace / n,
 * delta = (sum(zc^2) - 2 mu trace + n mu^2) / n and beta_ (:457-462) are scalars.  Synchronous. */
int td_shrinkage_terms(td_handle* h, const double* s_dev, int64_t ld, int n, const double* sum_row_dev, double frames,
                       double* out_host);
/* out = scale * S + diag * I (:463-465 with scale = (1 - shrinkage) / frames, diag = shrinkage * mu; a ridge with
 * scale = 1 / frames, diag = lambda): out64_dev [n, n] float64 for the solver and / or out32_dev [n, n] float32 (what
 * the reference returns as cov_x); either may be NULL.  Queued on the handle's stream. */
int td_shrunk_covariance(td_handle* h, const double* s_dev, int64_t ld, int n, double scale, double diag,
                         double* out64_dev, float* out32_dev);

/* ------------------------------------------------------------------ A3' / A4 forward
 * Linear model forward X.W + b on the lagged view of x, never materialised
 * (Keras Dense in brain_model.py:335-341, 376).  out_dev [rows, d] float32. */
int td_predict_fir(td_handle* h, const float* x_dev, int64_t ldx,
                   const int64_t* file_offsets_host, int num_files, int c, int pre,
                   int post, int input_offset, const float* w_dev, const float* b_dev,
                   int d, float* out_dev, int64_t ldout);
/* input_offset > 0 drops that many leading rows of every file of x BEFORE the
 * context is added (brain_data.py:466-475).  Output row file_offsets[f] + t is
 * frame t of the zipped streams of file f.
 * Arithmetic: float32 products accumulated in float32.  With td_set_accumulate_mode(TD_ACC_F32) the
 * products are exact float32 ones (v_mfma_f32_32x32x2_f32); otherwise every sample and weight enters as
 * two float16 pieces under a power-of-two scale of its row (22 significant bits; one output, <= 64
 * channels, <= 32 lags: fir_stream_kernel) or three bf16 pieces (the other shapes): within 4e-7 of the
 * sum of the terms' magnitudes against float64 either way (tests/test_gpu_decode.py).  A non-finite
 * sample makes exactly the outputs whose lag window holds it non-finite. */

/* The same forward with EVERY FILE UNDER ITS OWN MODEL: w_dev [num_files, K, d], b_dev
 * [num_files, d] (may be NULL).  This is the evaluation half of the leave-one-out sweep
 * (regression.jackknife_one_model, regression.py:197-214: the model fitted without recording f
 * predicts recording f; with the lambdas of a sweep as the d output columns) as ONE launch over
 * all held-out recordings instead of one per fold. */
int td_predict_fir_per_file(td_handle* h, const float* x_dev, int64_t ldx,
                            const int64_t* file_offsets_host, int num_files, int c, int pre,
                            int post, int input_offset, const float* w_dev, const float* b_dev,
                            int d, float* out_dev, int64_t ldout);

/* CCA transform [(x - mean1).rot1 | (x2 - mean2).rot2] on lagged views
 * (cca.BrainCcaLayer.call, cca.py:150-161).  out_dev [rows, 2*dims]. */
int td_cca_transform(td_handle* h, const float* x_dev, int64_t ldx, int c1, int pre1,
                     int post1, const float* x2_dev, int64_t ldx2, int c2, int pre2,
                     int post2, const int64_t* file_offsets_host, int num_files,
                     int input_offset, const float* mean1_dev, const float* rot1_dev,
                     const float* mean2_dev, const float* rot2_dev, int dims,
                     float* out_dev, int64_t ldout);

/* ------------------------------------------------------------------ A4 dense stage
 * CCA rotations from the accumulated moments, entirely on the device in float64
 * (cca.calculate_cca_parameters_from_dataset, cca.py:337-367): means, the reference's
 * covariance normalisation  cov = S / denom - mean^T mean  with
 * denom = num_mini_batches * n_row - 1 (:339-343, n_row = rows of the LAST minibatch),
 * + regularization * I on both auto-covariances, symmetric eigen-decompositions
 * (np.linalg.eig at :345-346), eigenvalues <= eps_eig dropped (:349-355), whitening
 * K11 / K22 (:357-360), svd(K11 cov_xy K22) (:361-363) and the rotations (:365-367).
 *   rot_x_dev [k1, dim], rot_y_dev [k2, dim], mean_x_dev [k1], mean_y_dev [k2], e_dev [dim]:
 *   float32 on the device, the dtype the reference returns for float32 inputs.
 *   dim <= min(k1, k2) (the caller clips, as the reference's slicing does).
 *   info_host (may be NULL, else int[4]) receives the Jacobi sweep counts {eig xx, eig yy, svd}
 *   and in [3] which sides were whitened by a Cholesky factor instead of the eigen-decomposition
 *   (any whitening gives the same canonical directions when no eigenvalue is dropped): bit 0 the
 *   x side, bit 1 the other side (17 .. 64 columns); bit 2: the whole stage ran as ONE launch (K1 <= 64,
 *   K2 <= 16, K2 <= K1 and a Cholesky factor exists; td_set_option "cca_fused").
 * Singular vectors are defined up to a joint sign of (rot_x[:, i], rot_y[:, i]). */
int td_cca_solve(td_handle* h, td_stats* s, double denom, double regularization, double eps_eig,
                 int dim, float* rot_x_dev, float* rot_y_dev, float* mean_x_dev, float* mean_y_dev,
                 float* e_dev, int* info_host);

/* The two float64 decompositions td_cca_solve is built from, for callers that bring their
 * own covariance matrices (np.linalg.eig on a symmetric matrix, np.linalg.svd).
 * td_sym_eigh: a_dev [n, n] symmetric (left untouched) -> vals_dev [n] (unsorted, as
 * np.linalg.eig leaves them), vecs_dev [n, n] with the eigenvectors as columns.  Cyclic Jacobi
 * (n <= 64: one workgroup in LDS; larger: block Jacobi with MFMA updates); *sweeps (may be
 * NULL) = outer sweeps used.
 * td_jacobi_svd: t_dev [m, n] -> the dim largest singular values s_dev [dim] (descending) with
 * u_dev [dim, m] and v_dev [dim, n] (singular vectors as ROWS), one-sided Jacobi. */
int td_sym_eigh(td_handle* h, const double* a_dev, int n, double* vals_dev, double* vecs_dev,
                int* sweeps);
int td_jacobi_svd(td_handle* h, const double* t_dev, int m, int n, int dim, double* u_dev,
                  double* s_dev, double* v_dev, int* sweeps);

/* ------------------------------------------------------------------ A5 / A6 / A7
 * Five running sums per window and column, in float64:
 *   out_dev[w][col] = {sum a, sum b, sum a^2, sum b^2, sum a*b}
 * over frames [k*hop, k*hop + width) of each trial, full windows only
 * (result_store.py:253-271; step = width//2 in infer_decoder.py:498-499).
 * Both correlation flavours derive from them: per-window Pearson
 * (brain_model.pearson_correlation, brain_model.py:34-79) and the
 * global-statistics score of Decoder.compute_correlation
 * (infer_decoder.py:312-328) averaged per window (infer.py:263-265).
 * window_offsets_host[T+1] (output) receives the first window index of each
 * trial; the caller sizes out_dev with td_window_count. */
int td_window_count(const int64_t* trial_offsets_host, int num_trials, int width, int hop,
                    int64_t* window_offsets_host, int64_t* total_windows);
int td_window_sums(td_handle* h, const float* a_dev, int64_t lda, const float* b_dev,
                   int64_t ldb, int cols, const int64_t* trial_offsets_host,
                   int num_trials, int width, int hop, double* out_dev);
/* The same with b holding b_cols <= cols columns, column j of a paired with column j % b_cols of b: the
 * predictions of several models (regression.jackknife_one_model: the lambdas of a sweep as output columns)
 * against ONE truth, without a tiled copy of the truth.  b_cols divides cols; windows and hops that share a
 * block of >= 32 frames (else TD_ERR_INVALID: tile b and call td_window_sums). */
int td_window_sums_cycled(td_handle* h, const float* a_dev, int64_t lda, const float* b_dev,
                          int64_t ldb, int cols, int b_cols, const int64_t* trial_offsets_host,
                          int num_trials, int width, int hop, double* out_dev);

/* Per-window scores from the five sums.
 *   mode 0: global-statistics correlation mean over the window of
 *           (a-mean_a)(b-mean_b)/power (infer_decoder.py:327-328), then the
 *           column reduction `reduction` (0 first, 1 second, 2 mean) of
 *           infer_decoder.py:441-446.  (mean-squared / lda need per-frame values: use
 *           td_frame_scores.)
 *   mode 1: per-window Pearson r (brain_model.py:62-79), incl. the
 *           "any constant column zeroes every column" rule.
 * scores_dev [total_windows] (mode 0) or [total_windows, cols] (mode 1). */
int td_window_scores(td_handle* h, const double* sums_dev, int64_t total_windows,
                     int cols, int width, int mode, int reduction,
                     const double* mean_a_host, const double* mean_b_host,
                     const double* power_host, double* scores_dev);

/* Per-window Pearson r of SEVERAL models at once: the columns are `cols / group` models of
 * `group` outputs each (e.g. the weight vectors of every lambda of a jackknife fold, evaluated
 * by one prediction pass; regression.py:197-214 evaluates them one by one).  The reference's
 * zero rule (brain_model.py:72-79: a constant column zeroes the whole result of THAT
 * pearson_correlation call) is applied per model: over its `group` columns only.
 * td_window_scores(mode 1) is the case group == cols.  scores_dev [total_windows, cols]. */
int td_window_pearson(td_handle* h, const double* sums_dev, int64_t total_windows, int cols,
                      int group, int width, double* scores_dev);

/* Per-frame reduced correlation score (Decoder.infer_one, infer_decoder.py:439-455)
 * for reductions that are not linear in the window sums.
 *   reduction: 0 first, 1 second, 2 mean, 3 mean-squared, 4 lda (affine map
 *   lda_w_host[cols], slope, intercept of scaled_lda.py:344-355), 5 all.
 * out_dev [rows] float64 ([rows, cols] for 'all'). */
int td_frame_scores(td_handle* h, const float* a_dev, int64_t lda, const float* b_dev,
                    int64_t ldb, int cols, int64_t rows, int reduction,
                    const double* mean_a_host, const double* mean_b_host,
                    const double* power_host, const double* lda_w_host, double lda_slope,
                    double lda_intercept, double* out_dev);

/* Window means of a float64 per-frame signal (infer.regress_and_correlate,
 * infer.py:261-266; infer_decoder.average_data :748-783 when hop == width). */
int td_window_means(td_handle* h, const double* v_dev, const int64_t* trial_offsets_host,
                    int num_trials, int width, int hop, double* out_dev);

/* Decoder.train with a window (infer_decoder.py:330-400): the per-frame value of
 * td_frame_scores' reduction 5, v = ((double)a - mean_a[c]) ((double)b - mean_b[c]) / power[c], its means
 * m[w][c] over the non-overlapping windows [w width, (w + 1) width) of the whole stream (average_data,
 * :748-783: the tail of rows % width frames is dropped, n_win = rows / width) and the moments of those
 * means, [[M^T M, sum_w m], [sum_w m^T, n_win]] row-major float64 -- what the LDA's scatter matrices are
 * made of -- in one pass over a and b and one finishing launch.
 *   means_dev   [n_win, cols] float64, or NULL when only the moments are wanted
 *   moments_dev [(cols + 1) (cols + 1)] float64; all zero when n_win == 0 (not an error)
 * All arithmetic is float64 in a fixed order without atomics, and the grid follows from (rows, width)
 * alone: two calls give the same bits.  TD_ERR_INVALID: cols outside [1, 32], width < 2, lda or
 * ldb < cols. */
int td_window_class_moments(td_handle* h, const float* a_dev, int64_t lda, const float* b_dev, int64_t ldb,
                            int cols, int64_t rows, int width,
                            const double* mean_a_host, const double* mean_b_host, const double* power_host,
                            double* means_dev, double* moments_dev);

/* ------------------------------------------------------------------ A8 / A9
 * Winner-take-all: out[i] = s1[i] > s2[i] (strict; ties -> speaker 2)
 * (attention_decoder.AttentionDecoder.attention, attention_decoder.py:128-134). */
int td_decide_wta(td_handle* h, const double* s1_dev, const double* s2_dev, int64_t n,
                  uint8_t* out_dev);
/* Stepped decoder with hysteresis, one state per trial starting at 0.5
 * (attention_decoder.StepAttentionDecoder, attention_decoder.py:141-173).
 * state_inout_host[T] may be NULL (fresh 0.5). */
int td_decide_step(td_handle* h, const double* s1_dev, const double* s2_dev,
                   const int64_t* window_offsets_host, int num_trials, uint8_t* out_dev,
                   double* state_inout_host);

/* State-space decoder, batched over independent trials
 * (attention_decoder.StateSpaceAttentionDecoder.attention,
 * attention_decoder.py:329-451).  params_host[8] =
 * {outer_iter, inner_iter, newton_iter, forward_lag, backward_lag, offset,
 *  tuned(0/1), reserved}; prior_host[4] = {rho_att, rho_unatt, mu_att, mu_unatt}
 * (tune_log_normal_priors, :277-327) used when tuned = 1.
 * out_dev [total_windows, 3] = (p, lower, upper). */
int td_decode_ssd(td_handle* h, const double* s1_dev, const double* s2_dev,
                  const int64_t* window_offsets_host, int num_trials,
                  const double* params_host, const double* prior_host, double* out_dev);
/* The same decoder fed as the windows arrive (the reference's object is stateful:
 * attention_decoder.py:329-451 keeps mu_d, rho_d, z_k_k, the smoothed tails and the last
 * k_w correlations between calls): state_dev [num_trials, td_ssd_state_doubles()] float64 on the
 * device, all zeros for a fresh decoder, is read before the trial's windows of this call and
 * written after them -- any split of a trial's windows over calls gives the outputs of one call.
 * state_dev NULL = td_decode_ssd.  (With td_profile_enable, a call that carries state counts as one launch.) */
int td_ssd_state_doubles(void);
int td_decode_ssd_stream(td_handle* h, const double* s1_dev, const double* s2_dev,
                         const int64_t* window_offsets_host, int num_trials,
                         const double* params_host, const double* prior_host, double* state_dev,
                         double* out_dev);

/* The whole window-size sweep of infer.run_reduction_test (infer.py:376-407) in two launches.
 *   s1_dev / s2_dev  per-frame scores of speaker 1 / 2, float64 [frames, cols], row strides ld1 / ld2
 *                    (td_frame_scores' output; cols > 1 only for reduction 'all')
 *   labels_dev       attention labels, float64 [frames]
 *   sizes_host       num_sizes (1..16) pairs {width, hop}
 *   decoder          0 winner-take-all, 1 stepped, 2 none (decisions 0, correct 0: the caller decides
 *                    from the means, e.g. with td_decode_ssd)
 * Size k has n_k = td_window_count(frames, width_k, hop_k) full windows; the outputs hold the sizes one
 * after the other, total_windows = sum n_k:
 *   means_dev     [3][total_windows] float64: window means of s1, s2 and the labels.  Each is bit for
 *                 bit td_window_means of the column (several columns: their means added in column order
 *                 and multiplied by the float64 1.0 / cols, as infer._window_means_host combines them).
 *   decisions_dev [total_windows] u8: td_decide_wta / td_decide_step (one trial per size, state 0.5)
 *   summary_dev   [num_sizes][2] int64: {end_first_section = first window whose label mean's truth
 *                 value differs from window 0's, 0 if none; correct = windows with decision xor
 *                 (label mean != 0)}.  A size without a full window has {0, 0}.
 * Fixed-order float64 and integer reductions, no atomics: two calls give the same bits.
 * TD_ERR_INVALID, before anything is queued: a NULL argument, num_sizes outside 1..16, width < 1,
 * hop < 1, cols < 1, ld1 or ld2 < cols, frames < 0, decoder outside 0..2. */
int td_attention_sweep(td_handle* h, const double* s1_dev, int64_t ld1, const double* s2_dev,
                       int64_t ld2, int cols, const double* labels_dev, int64_t frames,
                       const int* sizes_host, int num_sizes, int decoder, double* means_dev,
                       uint8_t* decisions_dev, int64_t* summary_dev);

/* ------------------------------------------------------------------ fused decode
 * Raw EEG -> decisions in one pass: FIR predict, global-statistics correlation
 * against two candidate envelopes, window means, winner-take-all.  Equivalent to
 * infer.run_reduction_test's inner loop (infer.py:376-407) with reduction
 * 'first' and decoder 'wta'.  env_dev [rows, 2].  corr_host[6] =
 * {mean_truth, mean_pred, power} for speaker 1 then speaker 2.
 * scores_dev [total_windows, 2] float64, decisions_dev [total_windows] u8. */
int td_decode_fused(td_handle* h, const float* eeg_dev, int64_t ldx, int c, int pre,
                    int post, const float* w_dev, const float* b_dev,
                    const float* env_dev, int64_t ldenv,
                    const int64_t* trial_offsets_host, int num_trials, int width,
                    int hop, const double* corr_host, double* scores_dev,
                    uint8_t* decisions_dev);

/* ------------------------------------------------------------------ online decode
 * td_decode_fused's chain for EEG that arrives in chunks (the reference's streaming shape:
 * Preprocessor.process(..., reset=False), Decoder.infer_one per minibatch, the stateful attention
 * decoders): `num_sessions` independent listeners, one state block each on the device, advanced by ONE
 * launch per push (one workgroup per session).  However a recording is cut into pushes, the outputs and
 * the final state are those of one push of the whole recording, bit for bit.
 *
 * The prediction of frame t needs the EEG rows up to t + post, so frames are emitted `post` frames late:
 * after `pushed` frames, emitted = max(0, pushed - post), or pushed once the recording was flushed; the
 * full windows of the emitted frames are windows(emitted) = td_window_count of one trial of that length.
 *
 * td_online_state_bytes: the size of one session's state block (a multiple of 8).  All zeros = a fresh
 * session.  It holds the last pre + post EEG rows, the last post envelope rows, a ring of the last
 * `width` per-frame scores of both speakers and the stepped decoder's float64 state (0 = fresh = 0.5) --
 * data only: the HOST counts the frames (frames_before) and is authoritative.
 *
 * td_online_plan (host, integers): what a push of n frames behind frames_before pushed ones emits.
 *   emitted_before / emitted_after  frames emitted before / after the push (flush != 0: all of them)
 *   first_window, new_windows       the push's windows are [first_window, first_window + new_windows)
 *
 * td_online_push: the sessions' next n frames.
 *   eeg_dev   [S][n][c] float32, row stride eeg_ld, session stride eeg_session_stride (elements)
 *   env_dev   [S][n][2] float32 (speaker 1, speaker 2), strides env_ld / env_session_stride
 *   n >= 0    (n == 0 and flush == 0: nothing is queued; the input pointers may then be NULL)
 *   w_dev     [(pre + 1 + post) c] float32 in the lag layout of td_predict_fir (row l c + ch multiplies
 *             x[t + l - pre][ch]), session stride w_session_stride; b_dev one bias per session, stride
 *             b_session_stride.  A session stride of 0 = one model for all sessions.
 *   corr_dev  [S][2][3] float64 {mean_truth, mean_pred, power} of speaker 1 then 2 (td_decode_fused's corr_host)
 *   reduction td_frame_scores' codes for ONE column: 0 first, 2 mean, 3 mean-squared, 4 lda with
 *             lda_dev [S][3] float64 {lda_w, slope, intercept} (NULL for the other reductions)
 *   width >= 1, hop >= 1; decoder 0 winner-take-all, 1 stepped, 2 none (decisions 0)
 *   frames_before  frames pushed so far (every session of a bank has seen the same number)
 *   flush     after these n rows behave as if `post` zero rows followed -- the end of the recording, the
 *             zero padding of td_predict_fir; the state is then good for nothing but td_memset
 *   state_dev, state_session_stride (BYTES, a multiple of 8, >= td_online_state_bytes)
 * Outputs, sized by td_online_plan:
 *   scores_dev    [2][S][new_windows] float64 (planar: a plane goes straight into td_decode_ssd_stream)
 *   decisions_dev [S][new_windows] u8
 *   pred_dev      [S][emitted_after - emitted_before] float32, or NULL: the predictions
 *   frame_dev     [2][S][emitted_after - emitted_before] float64, or NULL: the per-frame scores
 * Arithmetic: the prediction is a float32 sum whose order depends on (lag, channel) alone -- never on
 * where a frame falls in a push -- with the rows before the recording read as the zeros of a fresh state;
 * the per-frame score, the window mean and the decisions are td_frame_scores', td_window_means',
 * td_decide_wta's / td_decide_step's operation for operation.  No atomics: two runs give the same bits.
 * TD_ERR_INVALID, before anything is queued: a NULL required pointer, num_sessions < 1, c outside
 * 1..128, pre or post < 0, pre + 1 + post > 64, n outside 0..TD_ONLINE_MAX_PUSH, width outside
 * 1..TD_ONLINE_MAX_WIDTH, hop < 1, reduction not one of 0 / 2 / 3 / 4 (4 without lda_dev), decoder outside
 * 0..2, frames_before < 0, eeg_ld < c, env_ld < 2, a session stride of the inputs below one row (more
 * than one session), a model stride that is neither 0 nor a whole model, a state stride below the state
 * block or not a multiple of 8.
 * With td_profile_enable the launch is bracketed like the accumulate's dominant kernel (so is the
 * launch of td_decode_ssd_stream when it carries state): td_profile_read counts launches per push. */
#define TD_ONLINE_MAX_WIDTH 65536
#define TD_ONLINE_MAX_PUSH 1048576
int td_online_state_bytes(int c, int pre, int post, int width, int64_t* bytes);
int td_online_plan(int64_t frames_before, int64_t n, int post, int width, int hop, int flush,
                   int64_t* emitted_before, int64_t* emitted_after, int64_t* first_window,
                   int64_t* new_windows);
int td_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t eeg_ld,
                   int64_t eeg_session_stride, const float* env_dev, int64_t env_ld,
                   int64_t env_session_stride, int64_t n, int c, int pre, int post,
                   const float* w_dev, int64_t w_session_stride, const float* b_dev,
                   int64_t b_session_stride, const double* corr_dev, int reduction,
                   const double* lda_dev, int width, int hop, int decoder, int64_t frames_before,
                   int flush, void* state_dev, int64_t state_session_stride, double* scores_dev,
                   uint8_t* decisions_dev, float* pred_dev, double* frame_dev);

/* ------------------------------------------------------------------ online decode, CCA model
 * The session of td_online_push with a CCA model (cca.BrainModelCCA behind infer_decoder.CCADecoder) in front
 * of the correlator: ONE launch per push, one workgroup per session, the state on the device, and however a
 * recording is cut into pushes the outputs and the final state are those of one push, bit for bit.
 *
 * View 1 is the EEG, c1 channels with context pre1 / post1, k1 = c1 (pre1 + 1 + post1); view 2 is one block of
 * c2 audio features per speaker with context pre2 / post2, k2 = c2 (pre2 + 1 + post2).  Frames are emitted
 * post = max(post1, post2) frames late: td_online_plan with that post says what a push emits.  Per emitted
 * frame t
 *   a[d]   = sum_k (x~_t[k]     - mean_x[k]) rot_x[k][d]      (once, shared by both speakers)
 *   b_s[d] = sum_k (y~_{s,t}[k] - mean_y[k]) rot_y[k][d]      (speaker s = 1, 2)
 * in float32: one subtraction in front of each fused multiply-add (BrainCcaLayer.call's (x - mean) @ rot), in
 * an order that depends on (lag, channel, d) alone -- lane q of a wave takes the terms k = q, q + 64, ... into
 * four accumulators in turn, ((a0 + a1) + (a2 + a3)), then the 64-lane tree.  From the projections on it is
 * td_frame_scores(a, b_s) over the dims columns, td_window_means, td_decide_wta / td_decide_step, operation for
 * operation, and td_online_push's ring.
 *
 * td_cca_online_state_bytes: one session's state block (a multiple of 8; all zeros = fresh):
 *   8                          the stepped decoder's float64 state (0 = fresh = 0.5)
 *   16 width                   the ring of the last `width` per-frame scores, float64 [2][width]
 *   4 c1 (pre1 + post)         the last pre1 + post EEG rows
 *   8 c2 (pre2 + post)         the last pre2 + post feature rows of each speaker, [2][pre2 + post][c2]
 * Data only: the host counts the frames.
 *
 * td_cca_online_lds_bytes: the LDS of a launch that emits `emitted` frames and the frames per pass it takes:
 *   bytes(pass) = 32 pass + 4 ((dims + 1) (k1 + k2) + R1 c1 + 2 R2 c2 + 3 dims pass),
 *   R1 = max(pass + pre1 + post1, pre1 + post), R2 = max(pass + pre2 + post2, pre2 + post)
 * (scores and window means of a pass; the means and the rotations, transposed; the staged rows; the pass's
 * projections).  pass = min(64, max(emitted, 1)), halved (rounding up) while bytes(pass) exceeds
 * TD_CCA_ONLINE_LDS_BYTES; a shape whose bytes(1) exceeds it is refused by all three entry points
 * (td_cca_online_state_bytes checks dims = 1, the least a model can have).
 *
 * td_cca_online_push: the sessions' next n frames.
 *   eeg_dev    [S][n][c1] float32, row stride eeg_ld, session stride eeg_session_stride (elements)
 *   feat1_dev, feat2_dev  [S][n][c2] float32 each (speaker 1, speaker 2), strides feat_ld / feat_session_stride
 *   mean_x_dev [k1], rot_x_dev [k1][dims], mean_y_dev [k2], rot_y_dev [k2][dims] float32 in the lag layout of
 *              td_cca_transform (row l c + ch belongs to x[t + l - pre][ch]); model_session_stride 0 = one
 *              model for all sessions, 1 = the four arrays hold one model per session, one after the other
 *   corr_dev   [S][2][3][dims] float64 {mean_a, mean_b, power} of speaker 1 then 2
 *   reduction  td_frame_scores' codes: 0 first, 1 second (dims >= 2), 2 mean, 3 mean-squared, 4 lda with
 *              lda_dev [S][dims + 2] float64 {weights, slope, intercept} (NULL for the other reductions)
 *   width, hop, decoder, frames_before, flush, state_dev, state_session_stride: as td_online_push; a flush
 *              behaves as if `post` zero rows followed in both views
 * Outputs, sized by td_online_plan(..., post = max(post1, post2), ...):
 *   scores_dev    [2][S][new_windows] float64, decisions_dev [S][new_windows] u8
 *   proj_dev      [S][emitted][3 dims] float32 (a | b_1 | b_2), or NULL
 *   frame_dev     [2][S][emitted] float64, or NULL: the per-frame scores
 * No atomics: two runs give the same bits.  TD_ERR_INVALID, before anything is queued and with the state
 * untouched: a NULL required pointer, num_sessions < 1, c1 outside 1..128, c2 outside 1..32, a negative context,
 * more than 64 lags in a view, dims outside 1..16, a shape over the LDS budget, n outside 0..TD_ONLINE_MAX_PUSH,
 * width outside 1..TD_ONLINE_MAX_WIDTH, hop < 1, reduction outside 0..4 (1 with dims 1, 4 without lda_dev),
 * decoder outside 0..2, frames_before < 0, eeg_ld < c1, feat_ld < c2, a session stride of the inputs below
 * one row (more than one session), a model stride other than 0 or 1, a state stride below the state block or
 * not a multiple of 8.  With td_profile_enable the launch is bracketed as td_online_push's is. */
#define TD_CCA_ONLINE_LDS_BYTES 163840
int td_cca_online_state_bytes(int c1, int pre1, int post1, int c2, int pre2, int post2, int width,
                              int64_t* bytes);
int td_cca_online_lds_bytes(int c1, int pre1, int post1, int c2, int pre2, int post2, int dims,
                            int64_t emitted, int* pass, int64_t* bytes);
int td_cca_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t eeg_ld,
                       int64_t eeg_session_stride, const float* feat1_dev, const float* feat2_dev,
                       int64_t feat_ld, int64_t feat_session_stride, int64_t n, int c1, int pre1, int post1,
                       int c2, int pre2, int post2, int dims, const float* mean_x_dev, const float* rot_x_dev,
                       const float* mean_y_dev, const float* rot_y_dev, int64_t model_session_stride,
                       const double* corr_dev, int reduction, const double* lda_dev, int width, int hop,
                       int decoder, int64_t frames_before, int flush, void* state_dev,
                       int64_t state_session_stride, double* scores_dev, uint8_t* decisions_dev,
                       float* proj_dev, double* frame_dev);

/* ------------------------------------------------------------------ online decode, fully connected regressor
 * The session of td_online_push with a fully connected regressor (brain_model.BrainModelDNN behind
 * infer_decoder.LinearRegressionDecoder) in front of the correlator: ONE launch per push, one workgroup per
 * session, and however a recording is cut into pushes the outputs and the final state are those of one push, bit
 * for bit.  The state block is td_online_push's (td_online_state_bytes; td_online_plan says what a push emits), and
 * so is everything behind the prediction: td_frame_scores' expression for one column, the ring, td_window_means'
 * sum, td_decide_wta's / td_decide_step's decisions, the tail update.  (td_fc_: "fully connected".  The td_online_*,
 * td_mlp_* and td_dnn_* families are each checked as a closed set against their bindings, so this one has its own.)
 *
 * The prediction of an emitted frame t is td_mlp_forward's, bit for bit (one output, input_offset 0).  The model is
 * td_mlp_*'s packed parameter buffer [W1 (K x h1), b1, W2, b2, ..., WL, bL], K = c (pre + 1 + post); the input is
 * x~[k], k = lag c + channel, of the rows t - pre .. t + post, zero before the recording and, after a flush, past
 * its end.  With ks = min(64, round_up(ceil(K / 64), 4)) rows of W1 a slice:
 *   a slice partial   fmaf(x, w, s) from 0.f over the slice's rows in order
 *   z1[j]             (0.f + the slice partials added in slice order) + b1[j]
 *   ReLU              s <= 0.f ? 0.f : s, only when a layer follows
 *   a later layer     an fmaf chain over its inputs in order from 0.f, then + b, then ReLU except on the last.
 * W1 is streamed through LDS in chunks of whole slices (at most 4096 floats, double-buffered, 16-byte loads when
 * h1 is a multiple of 4 and the model is 16-byte aligned); the small parameters are staged once per launch.
 *
 * td_fc_online_lds_bytes: the LDS of a launch that emits `emitted` frames and the frames per pass it takes:
 *   bytes(pass) = 32 pass + 4 (2 chunk + round_up(n_small, 4) + (pass + pre + post) (c | 1) + 2 max(pass, post)
 *                              + pass + 2 pass lda),
 *   chunk = g ks round_up(h1, 4), g = min(slices, floor(4096 / (ks round_up(h1, 4)))), n_small = the parameters
 *   behind W1, lda = (the widest hidden layer, 1 without one) | 1
 * (scores and window means of a pass; two chunks of W1; the small parameters; the staged rows on an odd stride; the
 * envelopes; the predictions; two activation buffers).  pass = min(64, max(emitted, 1)), halved (rounding up) while
 * bytes(pass) exceeds TD_FC_ONLINE_LDS_BYTES; a shape whose bytes(1) exceeds it is refused by both entry points.
 *
 * td_fc_online_push: the sessions' next n frames.
 *   eeg_dev, env_dev, n, c, pre, post, corr_dev, reduction, lda_dev, width, hop, decoder, frames_before, flush,
 *   state_dev, state_session_stride and the four outputs: as td_online_push
 *   hidden_host [num_hidden] the hidden layers' units (NULL with num_hidden 0: z1 is the prediction, no ReLU)
 *   params_dev  the packed parameters, session stride params_session_stride (elements; 0 = one model for all)
 * No atomics: two runs give the same bits.  TD_ERR_INVALID, before anything is queued and with the state
 * untouched: what td_online_push refuses, and num_hidden outside 0..4, NULL hidden_host with num_hidden > 0, a
 * hidden layer outside 1..64 units, K > 8192, a shape over the LDS budget, NULL params_dev, a parameter stride that
 * is neither 0 nor a whole model.  With td_profile_enable the launch is bracketed as td_online_push's is. */
#define TD_FC_ONLINE_LDS_BYTES 163840
int td_fc_online_lds_bytes(int c, int pre, int post, int num_hidden, const int* hidden_host, int64_t emitted,
                            int* pass, int64_t* bytes);
int td_fc_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t eeg_ld,
                       int64_t eeg_session_stride, const float* env_dev, int64_t env_ld,
                       int64_t env_session_stride, int64_t n, int c, int pre, int post, const int* hidden_host,
                       int num_hidden, const float* params_dev, int64_t params_session_stride,
                       const double* corr_dev, int reduction, const double* lda_dev, int width, int hop,
                       int decoder, int64_t frames_before, int flush, void* state_dev,
                       int64_t state_session_stride, double* scores_dev, uint8_t* decisions_dev, float* pred_dev,
                       double* frame_dev);

/* ------------------------------------------------------------------ preprocessing
 * preprocess.Preprocessor (preprocess.py:54-587): the signal conditioning before the fits.
 *
 * td_sos_filter: a cascade of num_sections <= 16 second-order sections (scipy.signal.sosfilt,
 * direct form II transposed, a0 = 1; float64 arithmetic whatever the input) over x [N, c] (float32,
 * or float64 when x_is_f64), files concatenated along time (file_offsets_host[F+1]).  sos_host
 * [S][6]; zi_host [S][2] the sosfilt_zi of each STAGE (sections [0, stage_split) and
 * [stage_split, S) -- the high-pass and the low-pass -- each designed on its own).
 * state_dev [S, 2, c] float64 is the carried filter state (scipy's zi layout): read when reset == 0
 * for the first file, written with the final state of the last file.  A reset (reset != 0 for the
 * first file, always for the later ones) starts the first stage from zi * x[first row] and the second
 * from zi * (the first stage's output at that row), preprocess.py:293-352.
 * out_rows_dev (device, int64, may be NULL): the file-local input rows to store, nondecreasing, file f's
 * at [out_offsets_host[f], out_offsets_host[f+1]) -- the nearest-neighbour resample
 * (preprocess.py:376-389) fused into the store; y_dev row out_offsets[f] + i.  NULL: every row,
 * y_dev row file_offsets[f] + t.  y_dev float64, row stride ldy. */
int td_sos_filter(td_handle* h, const void* x_dev, int x_is_f64, int64_t ldx, int c,
                  const int64_t* file_offsets_host, int num_files, const double* sos_host, int num_sections,
                  int stage_split, const double* zi_host, int reset, double* state_dev,
                  const int64_t* out_rows_dev, const int64_t* out_offsets_host, double* y_dev, int64_t ldy);
/* The plan td_sos_filter follows for files of n_total rows in all, the longest n_max, over c channels:
 * the time-chunk length each (chunk, channel) lane filters, and the number of levels of the chunk
 * scan (blocks of 64 chunks per level).  Read-only; no handle. */
int td_sos_filter_plan(int64_t n_total, int64_t n_max, int c, int* chunk, int* levels);
/* Re-referencing by groups and channel selection in one pass (preprocess.py:417-443): row r of
 * z_dev [m, cs] float64 is row rows_dev[r] of x (rows_dev NULL: row r), every channel of group g
 * (chan_idx_host[chan_ptr_host[g] .. chan_ptr_host[g+1]]) minus the mean of that row's reference
 * channels (ref_idx_host[ref_ptr_host[g] ..]) taken BEFORE any group is subtracted, groups in order;
 * then output column j = channel sel_host[j] (NULL: j). */
int td_reref_select(td_handle* h, const void* x_dev, int x_is_f64, int64_t ldx, int c, const int64_t* rows_dev,
                    int64_t m, int num_groups, const int* ref_ptr_host, const int* ref_idx_host,
                    const int* chan_ptr_host, const int* chan_idx_host, const int* sel_host, int cs,
                    double* z_dev, int64_t ldz);
/* The float64 mean of all m x cs entries of z (np.mean, preprocess.py:445-455) into mean_dev[0]. */
int td_mean_f64(td_handle* h, const double* z_dev, int64_t m, int cs, int64_t ldz, double* mean_dev);
/* Normalisation and temporal context in one pass (preprocess.py:463-527): the rows
 * [state ; (z - mean) / std_dev] (state_dev [state_rows, cs], already normalised) become
 * state_rows + m - pre - post output rows of (pre + post + 1) * cs columns, block b of row r = row
 * r + b; written as float32 (out32_dev) and / or float64 (out64_dev), row stride ldout.  The last
 * min(state_rows + m, pre + post) rows go to state_out_dev (not aliasing state_dev). */
int td_context_out(td_handle* h, const double* z_dev, int64_t m, int cs, int64_t ldz, const double* state_dev,
                   int64_t state_rows, int pre, int post, double mean, double std_dev, float* out32_dev,
                   double* out64_dev, int64_t ldout, double* state_out_dev);

/* ------------------------------------------------------------------ online front end
 * The chain above for raw EEG that arrives in chunks of ANY length, in front of td_online_push: `num_sessions`
 * independent listeners configured by one Preprocessor's parameters, one state block each on the device, advanced
 * by ONE launch per push (one workgroup per session).  The steps keep their order: high-pass sections, low-pass
 * sections, nearest-neighbour resample, re-reference by groups, channel selection, (v - mean) / std, float32.
 * However a recording is cut into pushes, the concatenated output and the final state are those of one push of the
 * whole recording, bit for bit, and the output has exactly the rows of Preprocessor.process(whole, reset=True).
 * (The td_online_*, td_cca_online_* and td_fc_online_* families are checked as closed sets: this one has its own.)
 *
 * The filter is scipy's sosfilt recurrence (direct form II transposed, a0 = 1) in float64, strictly sequential in
 * time per (session, channel) -- no chunk scan, so the cut cannot matter -- with every fused multiply-add written
 * out (contraction is off in that file, the compiler chooses nothing).  Per section, in section order:
 *     y  = fma(b0, x, z0)
 *     z0 = fma(-a1, y, fma(b1, x, z1))
 *     z1 = fma(-a2, y, b2 * x)
 *     x  = y
 * Reset (rows_before == 0): sections [0, stage_split) start from x[0] * zi; sections [stage_split, S) from y0 * zi,
 * y0 being the output the first stage's step itself produces on row 0 (the reference's lowpass_filter_reset on the
 * high-pass output).  Either stage may be absent; num_sections == 0 is no filter.
 *
 * The resample over any cut.  Output frame j reads input row r_j = rint((j * (1.0 / fs_out)) * fs_in) and, with
 * F(N) = rint(N / fs_in * fs_out), is emitted by the first push after which both r_j <= N - 1 and j < F(N) hold
 * (N rows pushed so far); a flush then emits the frames j < F(N) not yet emitted at row min(N - 1, r_j).  These are
 * the reference's float64 products in its order (preprocess.resample_indices), so the rows over any cut are those
 * of resample_indices(N, fs_in, fs_out).  At most one frame is ever held back (only when downsampling: its row was
 * pushed, F does not count it yet); only upsampling clamps at a flush.  fs_in == fs_out: every row is a frame.  The
 * kernel computes r_j itself from (first frame, count): no index array is uploaded.
 *
 * Behind the resample it is td_reref_select and td_context_out (pre = post = 0) operation for operation: a group's
 * mean is the sequential float64 sum over its reference channels in list order divided by their count, the
 * subtractions go in group order from the values before any group was subtracted (a channel listed twice in ONE
 * group is subtracted once), then the selection, (v - mean) / std and a (float) cast.  None of these can
 * contract: with no filter the output is Preprocessor.process's byte for byte.
 *
 * td_frontend_state_bytes: one session's state block, 8 (2 num_sections + 2) c bytes: the filter state
 * [num_sections][2][c] float64 in scipy's zi layout (Preprocessor.filter_state's), then the held row [c] (the
 * filtered row of the last frame whose row has been pushed: the one a held frame waits with) and the last filtered
 * row [c].  All zeros = fresh.  Data only: the HOST counts the rows (rows_before) and
 * is authoritative.
 *
 * td_frontend_plan (host only): what a push of n rows behind rows_before pushed ones emits.
 *   frames_before / frames_after   frames emitted before / after the push (flush != 0: F(rows_before + n))
 *   held   frames whose row has been pushed but that are not emitted after the push (0 or 1; after a flush: dropped)
 *
 * td_frontend_lds_bytes: the LDS of a launch over c channels and num_groups groups that emits `emitted` frames,
 * and the frames per pass:  bytes(pass) = 8 pass (c + num_groups)  (a tile [pass][c] of filtered rows and the
 * pass's group means, float64);  pass = min(64, max(emitted, 1)), halved (rounding up) while bytes(pass) exceeds
 * TD_FRONTEND_LDS_BYTES.
 *
 * td_frontend_push: the sessions' next n raw rows.
 *   x_dev     [S][n][c] float32 (float64 when x_is_f64), row stride ldx, session stride x_session_stride (elements)
 *   n >= 0    (n == 0 and flush == 0: nothing is queued; so is a flush that has no row to add and no frame to emit)
 *   sos_host  [num_sections][6], zi_host [num_sections][2], stage_split: as td_sos_filter (NULL with no section);
 *             they travel to the kernel by value
 *   fs_in, fs_out  > 0
 *   num_groups (0 .. TD_FRONTEND_MAX_GROUPS), ref_ptr_host, ref_idx_host, chan_ptr_host, chan_idx_host, sel_host
 *             (NULL: channel j), cs: as td_reref_select; the tables go to the device through the handle's
 *             content-addressed table cache, so a steady push uploads nothing
 *   mean_dev, std_dev  float64, one per session stat_session_stride elements apart (0 = shared by all sessions)
 *   rows_before  rows pushed so far (0 = the filter resets on this push's first row)
 *   flush     the end of the recording; the state is then good for nothing but td_memset
 *   state_dev, state_session_stride (BYTES, a multiple of 8, >= td_frontend_state_bytes)
 *   out32_dev / out64_dev  [S][frames_after - frames_before][cs] float32 / float64 (either may be NULL, not both),
 *             row stride ldout, session stride out_session_stride (elements)
 * No atomics, vector stores only: two runs give the same bits.  TD_ERR_INVALID, before anything is queued and with
 * the state untouched: a NULL required pointer, num_sessions < 1, c or cs outside 1..128, num_sections outside
 * 0..16, a section with a0 != 1, stage_split outside 0..num_sections, a rate that is not positive and finite, n or
 * the emitted count outside 0..TD_ONLINE_MAX_PUSH, rows_before < 0, num_groups outside 0..TD_FRONTEND_MAX_GROUPS,
 * a group without reference channels, a selected or group channel outside the row, ldx < c, ldout < cs, a session
 * stride of x or the outputs below one row (more than one session), a negative stat stride, a state stride below
 * the state block or not a multiple of 8.  With td_profile_enable the launch is bracketed as td_online_push's is. */
#define TD_FRONTEND_MAX_GROUPS 32
#define TD_FRONTEND_LDS_BYTES 49152
int td_frontend_state_bytes(int c, int num_sections, int64_t* bytes);
int td_frontend_plan(int64_t rows_before, int64_t n, double fs_in, double fs_out, int flush,
                     int64_t* frames_before, int64_t* frames_after, int64_t* held);
int td_frontend_lds_bytes(int c, int num_groups, int64_t emitted, int* pass, int64_t* bytes);
int td_frontend_push(td_handle* h, int num_sessions, const void* x_dev, int x_is_f64, int64_t ldx,
                     int64_t x_session_stride, int64_t n, int c, const double* sos_host, int num_sections,
                     int stage_split, const double* zi_host, double fs_in, double fs_out, int num_groups,
                     const int* ref_ptr_host, const int* ref_idx_host, const int* chan_ptr_host,
                     const int* chan_idx_host, const int* sel_host, int cs, const double* mean_dev,
                     const double* std_dev, int64_t stat_session_stride, int64_t rows_before, int flush,
                     void* state_dev, int64_t state_session_stride, float* out32_dev, double* out64_dev,
                     int64_t ldout, int64_t out_session_stride);

/* ------------------------------------------------------------------ audio features
 * preprocess.AudioFeatures (preprocess.py:589-755): the intensity envelope and the auditory spectrogram.
 *
 * td_audio_intensity: the windowed mean of audio_resample (preprocess.py:619-686) over the virtual rows
 * [buf ; f(x)], tau = buf_rows, frames_in = buf_rows + n.  buf_dev [buf_rows, c] float64 (the carried buffer,
 * contiguous); x_dev [n, c] float32 (float64 when x_is_f64), row stride ldx; f(x) = float32(x)^2 (squared in
 * float32) when square != 0, else x.  Output row i < rows_out of out_dev [rows_out, c] float64 (contiguous) is
 * the float64 mean over rows [t1, t2), t = i / fs_out, t1 = max(0, rint(fs_in (t - half_window)) + tau),
 * t2 = min(frames_in, rint(fs_in (t + half_window)) + tau) in float64 in that order; NaN when t1 >= t2.
 * post != 0: sqrt, then ** exponent (numpy's fast paths for 1, 2, 0.5, 0, -1).  windows_dev (may be NULL):
 * [rows_out, 2] int64 receives (t1, t2). */
int td_audio_intensity(td_handle* h, const double* buf_dev, int64_t buf_rows, const void* x_dev, int x_is_f64,
                       int64_t ldx, int64_t n, int c, int square, int64_t rows_out, double fs_in, double fs_out,
                       double half_window, int post, double exponent, double* out_dev, int64_t* windows_dev);
/* Rows [row_begin, row_end) of the same [buf ; f(x)] (the pass-through of audio_resample and the new
 * buffer), contiguous, into exactly one of out32_dev (rounded to float32; sqrt and ** exponent in float32
 * when post != 0) or out64_dev (float64; post 1: sqrt and ** exponent in float64, post 2: the sqrt in
 * float32 and ** exponent in float64 -- numpy's promotion of a float32 array to a float64 exponent). */
int td_audio_passthrough(td_handle* h, const double* buf_dev, int64_t buf_rows, const void* x_dev, int x_is_f64,
                         int64_t ldx, int64_t n, int c, int square, int64_t row_begin, int64_t row_end, int post,
                         double exponent, float* out32_dev, double* out64_dev);
/* compute_spectrogram (preprocess.py:712-755) of wave_dev [n] float32: scipy.signal.stft of the
 * pre-emphasised wave (lfilter([1, -0.95])), periodic Hamming window of seg samples, hop, nfft-point
 * one-sided DFT, seg // 2 zeros of boundary padding, `frames` frames; the power smoothed by the causal FIR
 * taps_host[num_taps] along frequency then time, compressed to (off + P)^(1/4) - off^(1/4) with
 * off = 1e-4 max P and scaled to 255 / max.  out_dev [nfft / 2 + 1, frames] float64.  Limits: seg <= 1024,
 * seg <= nfft <= 4096, num_taps <= 16, n >= seg. */
int td_audio_spectrogram(td_handle* h, const float* wave_dev, int64_t n, int seg, int hop, int nfft,
                         const double* taps_host, int num_taps, int64_t frames, double* out_dev);

/* ------------------------------------------------------------------ online audio front end
 * The intensity envelope above for audio that arrives in chunks of ANY length, in front of td_online_push's env1 /
 * env2: `num_sessions` independent listeners configured by one AudioFeatures' parameters (fs_in, fs_out, window,
 * exponent), one state block each on the device, advanced by ONE launch per push.  However a recording is cut into
 * pushes, the concatenated output and the live state are those of one push of the whole recording, bit for bit, and
 * the frames are those of AudioFeatures(...).compute_intensity(whole) on a fresh object: the same windows, the same
 * count.  (td_audio_intensity restarts its window centres on every call; this family does not.)  The auditory
 * spectrogram has no such form: it is scaled by the maximum over the whole recording.
 *
 * Frames.  With N rows pushed so far, F(N) = rint(N / fs_in * fs_out), hw = 0.5 window / fs_out and, for frame i,
 * t = i / fs_out, a_i = rint(fs_in (t - hw)), u_i = rint(fs_in (t + hw)) -- float64 in the reference's order, half
 * even --, frame i is emitted by the first push after which u_i <= N and i < F(N).  A flush emits every frame
 * i < F(N) still missing.  Frame i is sqrt(mean) ** exponent (numpy's fast paths for 1, 2, 0.5, 0, -1) of the
 * float64 mean of float32(x)^2 -- squared in float32 -- over rows [max(0, a_i), min(N at emission, u_i)); an empty
 * window gives NaN.  The sum: lane l of a wave adds rows max(0, a_i) + l + 64 k in increasing k, then the xor
 * butterfly 32, 16, .. 1 -- a function of the window and the data, not of the cut or of an address.
 *
 * State.  The float32 squares of the last K rows pushed, K = ceil((window / 2 + max(window / 2, 0.5)) fs_in /
 * fs_out) + 2 (td_audio_online_plan's tail_rows; it bounds what the first frame not yet emitted reaches back).  A
 * tail copy is [K][c] float32, slot j holding row N - K + j, rows before row 0 zero: all zeros = fresh, and a copy
 * is a function of the rows pushed alone.  The block holds TWO copies (td_audio_online_state_bytes = 8 K c): a
 * launch reads copy `live` and writes every slot of the other one, so no workgroup reads what another writes.  The
 * HOST flips `live` after every push with n > 0 and counts the rows; a push with n == 0 writes no state.
 *
 * td_audio_online_plan (host only): what a push of n rows behind rows_before pushed ones emits.
 *   frames_before / frames_after   frames emitted before / after the push (flush != 0: F(rows_before + n))
 *   held       F(rows_before + n) - frames_after
 *   tail_rows  K
 *
 * td_audio_online_push: the sessions' next n rows.
 *   x_dev     [S][n][c] int16 / float32 / float64 (x_type TD_AUDIO_X_I16 / _F32 / _F64), row stride ldx, session
 *             stride x_session_stride (elements); the online object never transposes
 *   n >= 0    (n == 0 with no frame to emit: nothing is queued)
 *   state_dev, state_session_stride (BYTES, a multiple of 8, >= td_audio_online_state_bytes), live (0 or 1)
 *   out32_dev / out64_dev  [S][frames_after - frames_before][c] float32 / float64 (either may be NULL, not both),
 *             row stride ldout, session stride out_session_stride (elements); out32 is the float64 value rounded once
 *   windows_dev  NULL or [frames_after - frames_before][2] int64: the clamped window of every emitted frame
 * No atomics, vector stores only: two runs give the same bits.  TD_ERR_INVALID, before anything is queued and with
 * the state untouched: a NULL required pointer, num_sessions outside 1..65535, c outside
 * 1..TD_AUDIO_ONLINE_MAX_CHANNELS, an unknown x_type, a rate or window that is not positive and finite, the
 * reference's pass-through case (fs_out >= fs_in and window <= 1: it returns its input, there is nothing to
 * compute), K above TD_AUDIO_ONLINE_MAX_TAIL (which admits 48 kHz -> 64 Hz at window 8: K = 6002), n or the
 * emitted count outside 0..TD_ONLINE_MAX_PUSH, rows_before < 0, live outside 0..1, ldx or ldout < c, a session
 * stride of x or the outputs below one row (more than one session), a state stride below the state block or not
 * a multiple of 8.  With td_profile_enable the launch is bracketed as td_online_push's is. */
#define TD_AUDIO_ONLINE_MAX_CHANNELS 8
#define TD_AUDIO_ONLINE_MAX_TAIL 8192
#define TD_AUDIO_X_I16 0
#define TD_AUDIO_X_F32 1
#define TD_AUDIO_X_F64 2
int td_audio_online_plan(int64_t rows_before, int64_t n, double fs_in, double fs_out, double window, int flush,
                         int64_t* frames_before, int64_t* frames_after, int64_t* held, int64_t* tail_rows);
int td_audio_online_state_bytes(int c, int64_t tail_rows, int64_t* bytes);
int td_audio_online_push(td_handle* h, int num_sessions, const void* x_dev, int x_type, int64_t ldx,
                         int64_t x_session_stride, int64_t n, int c, int64_t rows_before, int flush, double fs_in,
                         double fs_out, double window, double exponent, void* state_dev,
                         int64_t state_session_stride, int live, float* out32_dev, double* out64_dev, int64_t ldout,
                         int64_t out_session_stride, int64_t* windows_dev);

/* ------------------------------------------------------------------ online ridge fit
 * The training stage of the online chain: the exact moments of the lagged regression for (eeg, target) rows that
 * arrive in pushes of any length -- `num_sessions` independent sessions, one state block each on the device, advanced
 * by ONE launch per push -- and ridge weights from them on demand.  However a recording is cut into pushes, the state
 * is that of one push of the whole recording, bit for bit.
 *
 * Frames.  c channels, context (pre, post), lags = pre + 1 + post, K = lags c, d outputs.  The lagged vector v of
 * frame t has v[l c + ch] = x[t + l - pre][ch], zero outside the recording, and v[K] = 1 (the reference's ones
 * column, brain_model.py:434-436).  Frames are emitted `post` rows late, as td_online_push emits them: after
 * `pushed` rows, emitted = max(0, pushed - post); a push that carries flush emits the rest with `post` zero rows
 * behind the end.
 *
 * The sum.  For every newly emitted frame, in frame order, with the forgetting factor g = forget:
 *   A[i][j] = A[i][j] g + v[i] v[j]     (K + 1) x (K + 1) float64
 *   B[i][o] = B[i][o] g + v[i] y[t][o]  (K + 1) x d       float64
 * The inputs are float32, so a product is exact.  g == 1: one rounding per frame and element (acc + p).  g < 1: two,
 * round(round(acc g) + p).  The order is a function of the frame index alone, so NumPy's A * g + np.outer(v, v) in
 * frame order gives the same bits.  A[K][K] is the frame count (g == 1) or the effective count (g < 1).
 *
 * State (td_fit_online_state_bytes; all zeros = a fresh session): A as a full square of float64 of which the launch
 * computes and stores the 64 x 64 tiles (ti, tj) with tj >= ti only (a diagonal tile whole) -- the lower tiles stay
 * zero, td_fit_online_moments mirrors --, B, then TWO tail copies of {EEG [pre + post][c], target [post][d]} float32,
 * slot j holding row pushed - (pre + post) + j (target: pushed - post + j), zero before row 0.  A launch reads copy
 * (pushes_before & 1) and one workgroup per session writes every slot of the other one; pushes_before counts the
 * pushes with n > 0 (the HOST counts frames and pushes; a push without rows writes no tail).
 *
 * td_fit_online_push: the sessions' next n rows.
 *   eeg_dev     [S][n][c] float32, row stride ld_eeg, session stride eeg_session_stride (elements)
 *   target_dev  [S][n][d] float32, row stride ld_target, session stride target_session_stride (elements)
 *   n >= 0      (n == 0 with no frame to emit: nothing is queued); a push that emits nothing still rolls the tails
 *   frames_before   rows pushed so far;  flush != 0: the recording ends behind this push
 *   state_dev, state_session_stride (BYTES, a multiple of 8, >= td_fit_online_state_bytes)
 * grid: sessions x (upper-triangular tiles of A + the 64-row tiles of B + the tail workgroup), 256 threads, a 4 x 4
 * block of float64 accumulators per thread.  No workgroup reads what another writes, no atomics, vector stores only:
 * two runs give the same bits.  With td_profile_enable the launch is bracketed as td_online_push's is.
 *
 * td_fit_online_moments: xtx_dev [S][K + 1][K + 1] and xty_dev [S][K + 1][d] float64 (either may be NULL, not both),
 * mirrored and dense, in the layout of td_stats_moments (the ones row / column last).
 *
 * td_fit_online_solve: ridge weights for every (session, lambda): the systems A_sym / A[K][K] + lambda I (the
 * reference's cov_x, lambda on the bias entry too: brain_model.py:447-455) and B / A[K][K] are built in one launch,
 * td_spd_solve solves them (batched float64 Cholesky in the handle's solver workspace), one more launch writes
 * w_dev [S][n_lambda][K][d] and b_dev [S][n_lambda][d] float32.  frames_emitted: the host's count of emitted frames.
 * Synchronous.  TD_ERR_STATE: no frame emitted yet (never a division by zero).  TD_ERR_NOMEM: the dense systems need
 * more than TD_ONLINE_FIT_MAX_SOLVE_BYTES.  TD_ERR_SINGULAR: a system is not positive definite, as td_ridge_solve.
 *
 * TD_ERR_INVALID, before anything is queued and with the state untouched: a NULL required pointer, num_sessions
 * outside 1..65535, c outside 1..TD_ONLINE_FIT_MAX_CHANNELS, pre or post < 0, more than TD_ONLINE_FIT_MAX_LAGS lags,
 * K above TD_ONLINE_FIT_MAX_K, d outside 1..TD_ONLINE_FIT_MAX_OUTPUTS, n outside 0..TD_ONLINE_MAX_PUSH, forget
 * outside (0, 1], frames_before or pushes_before < 0, a row or session stride below a row, a state stride below
 * the state block or not a multiple of 8, n_lambda < 1 or more than 65535 systems, a lambda that is not finite. */
#define TD_ONLINE_FIT_MAX_CHANNELS 128
#define TD_ONLINE_FIT_MAX_LAGS 64
#define TD_ONLINE_FIT_MAX_K 2048
#define TD_ONLINE_FIT_MAX_OUTPUTS 8
#define TD_ONLINE_FIT_MAX_SOLVE_BYTES (4LL << 30)
int td_fit_online_state_bytes(int c, int pre, int post, int d, int64_t* bytes);
int td_fit_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t ld_eeg,
                       int64_t eeg_session_stride, const float* target_dev, int64_t ld_target,
                       int64_t target_session_stride, int64_t n, int c, int pre, int post, int d,
                       int64_t frames_before, int64_t pushes_before, int flush, double forget, void* state_dev,
                       int64_t state_session_stride);
int td_fit_online_moments(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride, int c,
                          int pre, int post, int d, double* xtx_dev, double* xty_dev);
int td_fit_online_solve(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride, int c,
                        int pre, int post, int d, int64_t frames_emitted, const double* lambdas_host, int n_lambda,
                        float* w_dev, float* b_dev);

/* ------------------------------------------------------------------ online CCA fit
 * The training stage of the online CCA decoder (td_cca_online_push): the exact float64 moments of BOTH lagged views
 * for rows that arrive in pushes of any length -- ONE launch per push for `num_sessions` sessions, one state block
 * each on the device -- and rotations from them on demand, through the dense stage td_cca_solve runs.  However a
 * recording is cut into pushes, the state is that of one push of the whole recording, bit for bit.  (The prefix is
 * td_ccafit_online_: td_cca_online_* is the decoder's closed set.)
 *
 * Views.  View 1 is the EEG: c1 channels, context (pre1, post1), k1 = c1 (pre1 + 1 + post1).  View 2 is the attended
 * speaker's feature block: c2 columns, context (pre2, post2), k2 = c2 (pre2 + 1 + post2).  The joint vector of frame
 * t is u = [x~_t | y~_t | 1], n = k1 + k2 + 1; each half is the lagged row t of its view, lag-major, channel-minor,
 * v[l c + ch] = x[t + l - pre][ch], zero outside the recording.  Frames run post = max(post1, post2) rows behind the
 * input, as td_cca_online_push has it: emitted = max(0, pushed - post); a push that carries flush emits the rest, as
 * if `post` zero rows followed in both views.
 *
 * The sum.  For every newly emitted frame, in frame order, with the forgetting factor g = forget:
 *   M = M g + u u^T     n x n float64
 * The inputs are float32, so a product is exact.  g == 1: one rounding per frame and element (the fused multiply-add
 * of the widened values).  g < 1: two, round(round(acc g) + p).  The order is a function of the frame index alone, so
 * NumPy's M * g + np.outer(u, u) in frame order gives the same bits.  M[n - 1][n - 1] is the frame count (g == 1) or
 * the effective count (g < 1).
 *
 * State (td_ccafit_online_state_bytes, rounded up to 8; all zeros = a fresh session): M as a full square of float64
 * of which the launch computes and stores the 64 x 64 tiles (ti, tj) with tj >= ti only (a diagonal tile whole) -- the
 * lower tiles stay zero, td_ccafit_online_moments mirrors --, then TWO tail copies of {EEG [pre1 + post][c1],
 * features [pre2 + post][c2]} float32, slot j of a view's tail holding row pushed - (pre_v + post) + j, zero before
 * row 0.  A launch reads copy (pushes_before & 1) and one workgroup per session writes every slot of the other one;
 * pushes_before counts the pushes with n > 0 (the HOST counts frames and pushes; a push without rows writes no tail).
 *
 * td_ccafit_online_push: the sessions' next n rows.
 *   eeg_dev   [S][n][c1] float32, row stride ld_eeg, session stride eeg_session_stride (elements)
 *   feat_dev  [S][n][c2] float32, row stride ld_feat, session stride feat_session_stride (elements)
 *   n >= 0    (n == 0 with no frame to emit: nothing is queued); a push that emits nothing still rolls the tails
 *   frames_before   rows pushed so far;  flush != 0: the recording ends behind this push
 *   state_dev, state_session_stride (BYTES, a multiple of 8, >= td_ccafit_online_state_bytes)
 * grid: sessions x (upper-triangular tiles of M + the tail workgroup), 256 threads, a 4 x 4 block of float64
 * accumulators per thread.  No workgroup reads what another writes, no atomics, vector stores only: two runs give the
 * same bits.  With td_profile_enable the launch is bracketed as td_online_push's is.
 *
 * td_ccafit_online_moments: one launch fills xtx_dev [S][k1 + 1][k1 + 1] (the ones row and column last, the layout of
 * td_stats_moments), x2tx2_dev [S][k2][k2], xtx2_dev [S][k1][k2] and sum2_dev [S][k2], float64, dense and mirrored
 * (any may be NULL, not all).
 *
 * td_ccafit_online_solve: the reference's CCA model (cca.py:337-343) of one minibatch that holds all counted frames,
 * for every (session, lambda): means = sums / count, denom = count - 1, cov = S / denom - mean^T mean, + lambda I on
 * both auto-covariances, eps_eig filtering, whitening, SVD, rotations -- td_cca_solve's dense stage, called once per
 * (session, lambda) on the moments one launch expands into the handle's workspace; count = M[n - 1][n - 1].
 *   rot_x_dev [S][n_lambda][k1][dim], rot_y_dev [S][n_lambda][k2][dim], mean_x_dev [S][k1], mean_y_dev [S][k2],
 *   e_dev [S][n_lambda][dim] float32; corr_dev [S][n_lambda][3][dim] float64; info_host [S][n_lambda][4] (may be
 *   NULL) as td_cca_solve's.
 * corr is the fitted stretch's statistics in closed form from the same moments, for the float32 model returned: with
 * m = sums / count and C = S / count - m m^T,  mean_a[d] = (m_x - mean_x) . rot_x[:, d], mean_b likewise,
 * power[d] = sqrt((rot_x[:, d]^T C_xx rot_x[:, d]) (rot_y[:, d]^T C_yy rot_y[:, d])): one more launch per pair.
 * frames_emitted: the host's count of emitted frames.  Synchronous (per pair, as td_cca_solve).  TD_ERR_STATE: fewer
 * than 2 frames counted, or an effective count <= 1 (never a division by zero).
 *
 * TD_ERR_INVALID, before anything is queued and with the state untouched: a NULL required pointer, num_sessions
 * outside 1..65535, c1 outside 1..TD_ONLINE_CCAFIT_MAX_CHANNELS, c2 outside 1..TD_ONLINE_CCAFIT_MAX_FEATURES, a
 * context < 0, more than TD_ONLINE_CCAFIT_MAX_LAGS lags in a view, k1 + k2 above TD_ONLINE_CCAFIT_MAX_K, n outside
 * 0..TD_ONLINE_MAX_PUSH, forget outside (0, 1], frames_before or pushes_before < 0, a row or session stride below a
 * row, a state stride below the state block or not a multiple of 8, n_lambda < 1, a lambda < 0 or not finite, dim
 * outside 1..min(TD_ONLINE_CCAFIT_MAX_DIMS, k1, k2). */
#define TD_ONLINE_CCAFIT_MAX_CHANNELS 128
#define TD_ONLINE_CCAFIT_MAX_FEATURES 32
#define TD_ONLINE_CCAFIT_MAX_LAGS 64
#define TD_ONLINE_CCAFIT_MAX_K 2048
#define TD_ONLINE_CCAFIT_MAX_DIMS 16
int td_ccafit_online_state_bytes(int c1, int pre1, int post1, int c2, int pre2, int post2, int64_t* bytes);
int td_ccafit_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t ld_eeg,
                          int64_t eeg_session_stride, const float* feat_dev, int64_t ld_feat,
                          int64_t feat_session_stride, int64_t n, int c1, int pre1, int post1, int c2, int pre2,
                          int post2, int64_t frames_before, int64_t pushes_before, int flush, double forget,
                          void* state_dev, int64_t state_session_stride);
int td_ccafit_online_moments(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride,
                             int c1, int pre1, int post1, int c2, int pre2, int post2, double* xtx_dev,
                             double* x2tx2_dev, double* xtx2_dev, double* sum2_dev);
int td_ccafit_online_solve(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride,
                           int c1, int pre1, int post1, int c2, int pre2, int post2, int64_t frames_emitted,
                           const double* lambdas_host, int n_lambda, int dim, double eps_eig, float* rot_x_dev,
                           float* rot_y_dev, float* mean_x_dev, float* mean_y_dev, float* e_dev, double* corr_dev,
                           int* info_host);

/* ------------------------------------------------------------------ online calibration
 * The stage behind the online ridge fit: what infer_decoder.Decoder.train(data0, data1, window_size = W) takes from
 * a labelled stretch -- the correlation statistics {mean_truth, mean_pred, power}, the scaled LDA between the window
 * means of the unattended (class 0) and the attended (class 1) correlations, d' -- for (eeg, attended envelope,
 * unattended envelope) rows that arrive in pushes of any length, predicted with the weights handed to each push.
 * `num_sessions` independent sessions, one state block each on the device, ONE launch per push (one workgroup of 256
 * threads per session), nothing stored per row.  However a recording is cut into pushes, the state is that of one
 * push of the whole recording, bit for bit.
 *
 * Frames are emitted `post` rows late with td_online_plan's arithmetic: after `pushed` rows emitted =
 * max(0, pushed - post); a push that carries flush emits the rest with `post` zero rows behind the end.  The
 * prediction p of an emitted frame is the float32 value td_online_push returns in `pred` (the same operation order).
 * env[..., 0] is the attended envelope a, env[..., 1] the unattended one u.  Windows are average_data's: consecutive,
 * hop = width, the tail dropped; width 1 is train's frame-level case.
 *
 * State (td_calib_online_state_bytes; all zeros = a fresh session; the HOST counts the frames): TD_CALIB_ONLINE_SUMS
 * float64 sums, every one advanced in frame order by acc += (double)x * (double)y (the product is exact),
 *   [0, 6)    over every emitted frame: sum p, sum p^2, sum a, sum a^2, sum u, sum u^2
 *   [6, 15)   class 0 (truth x = u) over the completed windows: sum_w z [3], then the upper triangle of sum_w z z^T
 *             in the order (0,0) (0,1) (0,2) (1,1) (1,2) (2,2), z = (sum x p, sum x, sum p) of a window; the Gram
 *             takes G + z_i z_j unfused (the product rounds, then the add)
 *   [15, 24)  class 1 (truth x = a), the same
 *   [24, 29)  the open window: sum p, sum a, sum a p, sum u, sum u p (zero again when a frame completes a window)
 * then the EEG tail [pre + post][c] and the envelope tail [post][2] float32 (td_online_push's), rounded up to 8 bytes.
 *
 * td_calib_online_push: the sessions' next n rows.
 *   eeg_dev [S][n][c] float32, row stride eeg_ld, session stride eeg_session_stride (elements)
 *   env_dev [S][n][2] float32, row stride env_ld, session stride env_session_stride (elements)
 *   w_dev [S or 1][(pre + 1 + post) c], b_dev [S or 1] float32: session strides in elements, 0 = one model for all
 *   n >= 0 (n == 0 without flush: nothing is queued); a push that emits nothing still rolls the tails
 *   frames_before: rows pushed so far;  flush != 0: the recording ends behind this push
 *   state_dev, state_session_stride (BYTES, a multiple of 8, >= td_calib_online_state_bytes)
 * With td_profile_enable the launch is bracketed as td_online_push's is.
 *
 * td_calib_online_sums: out_dev [S][TD_CALIB_ONLINE_SUMS] float64, the sums in the order above.
 *
 * td_calib_online_finish: ONE launch evaluates, per session and in float64, with N = frames_emitted (the host's
 * count), n_win = N / width and the correlator as train feeds it (class 0 first):
 *   count = 2 N, sum_x = sum u + sum a, sum_x2 = sum u^2 + sum a^2, sum_y = sum p + sum p, sum_y2 = sum p^2 + sum p^2
 *   mean_x = sum_x / count, mean_y = sum_y / count,
 *   power = sqrt((sum_x2 - sum_x^2 / count) (sum_y2 - sum_y^2 / count)) / count
 *   c = (1, -mean_y, -mean_x) / (width power), c0 = mean_x mean_y / power, and per class
 *   sum_w m = c . sum z + n_win c0,  sum_w m^2 = c^T (sum z z^T) c + 2 c0 (c . sum z) + n_win c0^2
 *   mbar = sum_w m / n_win, v = sum_w m^2 / n_win - mbar^2
 *   slope = 1 / (mbar_1 - mbar_0), intercept = -slope mbar_0, d' = |mbar_1 - mbar_0| / sqrt((v_0 + v_1) / 2)
 * and writes corr_dev [S][2][3] (both speaker rows {mean_x, mean_y, power}: the layout td_online_push reads),
 * lda_dev [S][3] {1, slope, intercept}, dprime_dev [S] and status_dev [S] int32: TD_CALIB_OK; TD_CALIB_NO_WINDOW (no
 * completed window: train's "No data for class"); TD_CALIB_NO_POWER (power not finite or <= 0); TD_CALIB_SAME_MEANS
 * (equal class means: scaled LDA's "X0 and X1 ... identical").  What a session cannot give is NaN.  The state is not
 * modified: calibration can go on after a look.  Bracketed by td_profile_enable as a push is.
 *
 * TD_ERR_INVALID, before anything is queued and with the state untouched: a NULL required pointer, num_sessions
 * outside 1..65535, c outside 1..TD_CALIB_ONLINE_MAX_CHANNELS, pre or post < 0, more than TD_CALIB_ONLINE_MAX_LAGS
 * lags, width outside 1..TD_ONLINE_MAX_WIDTH, n outside 0..TD_ONLINE_MAX_PUSH, frames_before or frames_emitted < 0, a
 * row or session stride below a row, a weight stride below a model, a state stride below the state block (for
 * _sums and _finish: below the sums) or not a multiple of 8. */
#define TD_CALIB_ONLINE_MAX_CHANNELS 128
#define TD_CALIB_ONLINE_MAX_LAGS 64
#define TD_CALIB_ONLINE_SUMS 29
#define TD_CALIB_OK 0
#define TD_CALIB_NO_WINDOW 1
#define TD_CALIB_NO_POWER 2
#define TD_CALIB_SAME_MEANS 3
int td_calib_online_state_bytes(int c, int pre, int post, int64_t* bytes);
int td_calib_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t eeg_ld,
                         int64_t eeg_session_stride, const float* env_dev, int64_t env_ld,
                         int64_t env_session_stride, const float* w_dev, int64_t w_session_stride,
                         const float* b_dev, int64_t b_session_stride, int64_t n, int64_t frames_before, int c,
                         int pre, int post, int width, int flush, void* state_dev, int64_t state_session_stride);
int td_calib_online_sums(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride,
                         double* out_dev);
int td_calib_online_finish(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride,
                           int64_t frames_emitted, int width, double* corr_dev, double* lda_dev, double* dprime_dev,
                           int32_t* status_dev);

/* ------------------------------------------------------------------ online calibration of a CCA model
 * The stage behind the online CCA fit: what infer_decoder.Decoder.train(data0, data1, window_size = W) takes from a
 * labelled stretch with a CCADecoder -- per dim the correlation statistics {mean_a, mean_b, power} of ONE correlator
 * fed both classes, the scaled LDA over the `dims` columns between the window means of the unattended (class 0) and
 * the attended (class 1) correlations, d' -- for (eeg, attended features, unattended features) rows that arrive in
 * pushes of any length, projected with the model handed to each push.  `num_sessions` independent sessions, one
 * state block each on the device, ONE launch per push (one workgroup of 1024 threads per session), nothing stored
 * per row.  However a recording is cut into pushes, the state is that of one push of the whole recording, bit for bit.
 *
 * Frames are emitted post = max(post1, post2) rows late with td_online_plan's arithmetic, as td_cca_online_push
 * emits them.  Per emitted frame and with D = dims: a [D] is the EEG view's projection, b1 [D] the attended feature
 * block's, b0 [D] the unattended one's -- the float32 values td_cca_online_push returns in `proj` (the same
 * function).  Windows are average_data's: consecutive, hop = width, the tail dropped; width 1 is train's frame-level
 * case.
 *
 * State (td_ccacalib_online_state_bytes; all zeros = a fresh session; the HOST counts the frames): a head of
 * T(D) = 9 D^2 + 20 D float64 sums (29 at D = 1, td_calib_online's count; 2624 at D = 16), every per-frame sum
 * advanced in frame order by acc += (double)x * (double)y (the product is exact),
 *   [0, 6 D)    over every emitted frame: sum a, sum a^2, sum b1, sum b1^2, sum b0, sum b0^2, [D] each
 *   then class 0 (b = b0) over the completed windows: sum_w z [3 D], then the upper triangle of sum_w z z^T row-major
 *               (3 D (3 D + 1) / 2 entries), z = (sum a b [D] | sum a [D] | sum b [D]) of a window; the sum takes plain
 *               adds, the Gram G + z_i z_j unfused (the product rounds, then the add)
 *   then class 1 (b = b1), the same
 *   then the open window: sum a, sum b1, sum a b1, sum b0, sum a b0, [D] each (zero again when a frame completes a
 *               window)
 * then the EEG tail [pre1 + post][c1] and the feature tails [2][pre2 + post][c2] float32 (attended, unattended), as
 * td_cca_online_push carries them, rounded up to 8 bytes.
 *
 * td_ccacalib_online_lds_bytes: (*pass, *bytes) of a launch that emits `emitted` frames: the frames a workgroup
 * stages at once -- 64, fewer for a short push, halved until the LDS fits TD_CCA_ONLINE_LDS_BYTES -- and the
 * dynamic LDS: 8 (5 D pass) for the windows a pass completes, then float32: both means, both rotations transposed,
 * the staged rows and the pass's projections (td_cca_online_lds_bytes' terms).  A shape that does not fit at a pass
 * of one frame is refused by every entry point that takes the shape.
 *
 * td_ccacalib_online_push: the sessions' next n rows.
 *   eeg_dev [S][n][c1] float32, row stride eeg_ld, session stride eeg_session_stride (elements)
 *   att_dev, unatt_dev [S][n][c2] float32, row stride feat_ld, session stride feat_session_stride (elements)
 *   mean_x_dev [k1], rot_x_dev [k1][dims], mean_y_dev [k2], rot_y_dev [k2][dims] float32, k = c (pre + 1 + post);
 *   model_session_stride 0 (one model for all) or 1 (session s reads model s) -- read where they lie at every push
 *   n >= 0 (n == 0 without flush: nothing is queued); a push that emits nothing still rolls the tails
 *   frames_before: rows pushed so far;  flush != 0: the recording ends behind this push
 *   state_dev, state_session_stride (BYTES, a multiple of 8, >= td_ccacalib_online_state_bytes)
 * With td_profile_enable the launch is bracketed as td_online_push's is.
 *
 * td_ccacalib_online_sums: out_dev [S][T(dims)] float64, the head in the order above.
 *
 * td_ccacalib_online_finish: ONE launch (a workgroup of 256 threads per session) evaluates in float64, with
 * N = frames_emitted (the host's count), n_win = N / width and the correlator as train feeds it (class 0 first):
 *   per dim d: count = 2 N, sum_x = 2 sum a, sum_x2 = 2 sum a^2, sum_y = sum b0 + sum b1, sum_y2 = sum b0^2 + sum b1^2,
 *   mean_a = sum_x / count, mean_b = sum_y / count,
 *   power = sqrt((sum_x2 - sum_x^2 / count) (sum_y2 - sum_y^2 / count)) / count, c0_d = mean_a mean_b / power
 *   C [D][3 D]: row d holds (1, -mean_b_d, -mean_a_d) / (width power_d) at the columns (d, D + d, 2 D + d); per class
 *   sum_w m = C sum z + n_win c0,  sum_w m m^T = C (sum z z^T) C^T + (C sum z) c0^T + c0 (C sum z)^T + n_win c0 c0^T,
 *   mu = sum_w m / n_win,  S = sum_w m m^T - n_win mu mu^T
 *   Sw = S_0 + S_1,  v = Sw^-1 (mu_1 - mu_0) by Cholesky,  w = v / |v|_2 ([1] at D = 1),
 *   slope = 1 / ((mu_1 - mu_0) . w),  intercept = -slope (mu_0 . w),
 *   d' = |(mu_1 - mu_0) . w| / sqrt((w^T S_0 w + w^T S_1 w) / (2 n_win))
 * and writes corr_dev [S][2][3][D] (both speaker rows {mean_a, mean_b, power}: the layout td_cca_online_push reads),
 * lda_dev [S][D + 2] {w, slope, intercept}, dprime_dev [S] and status_dev [S] int32: TD_CALIB_OK; TD_CALIB_NO_WINDOW;
 * TD_CALIB_NO_POWER (a dim's power not finite or <= 0); TD_CALIB_NOT_POSITIVE (the pooled scatter Sw is not positive
 * definite: a Cholesky pivot <= 0 or not finite, or fewer than dims + 2 windows in all); TD_CALIB_SAME_MEANS
 * (the class means are equal along w: scaled LDA's "X0 and X1 ... identical").  What a session cannot give is NaN.
 * The state is not modified.  Bracketed by td_profile_enable as a push is.
 *
 * TD_ERR_INVALID, before anything is queued and with the state untouched: a NULL required pointer, num_sessions
 * outside 1..65535, td_cca_online_push's shape limits (128 channels, 32 features, 64 lags per view, 16 dims), a shape
 * over the LDS budget, width outside 1..TD_ONLINE_MAX_WIDTH, n outside 0..TD_ONLINE_MAX_PUSH, frames_before or
 * frames_emitted < 0, a row or session stride below a row, a model stride other than 0 or 1, a state stride below the
 * state block (for _sums and _finish: below the head) or not a multiple of 8. */
#define TD_CALIB_NOT_POSITIVE 4
int td_ccacalib_online_state_bytes(int c1, int pre1, int post1, int c2, int pre2, int post2, int dims,
                                   int64_t* bytes);
int td_ccacalib_online_lds_bytes(int c1, int pre1, int post1, int c2, int pre2, int post2, int dims,
                                 int64_t emitted, int* pass, int64_t* bytes);
int td_ccacalib_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t eeg_ld,
                            int64_t eeg_session_stride, const float* att_dev, const float* unatt_dev,
                            int64_t feat_ld, int64_t feat_session_stride, int64_t n, int c1, int pre1, int post1,
                            int c2, int pre2, int post2, int dims, const float* mean_x_dev, const float* rot_x_dev,
                            const float* mean_y_dev, const float* rot_y_dev, int64_t model_session_stride, int width,
                            int64_t frames_before, int flush, void* state_dev, int64_t state_session_stride);
int td_ccacalib_online_sums(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride,
                            int dims, double* out_dev);
int td_ccacalib_online_finish(td_handle* h, int num_sessions, const void* state_dev, int64_t state_session_stride,
                              int dims, int64_t frames_emitted, int width, double* corr_dev, double* lda_dev,
                              double* dprime_dev, int32_t* status_dev);

/* ------------------------------------------------------------------ online calibration of a DNN decoder
 * td_calib_online_push with the fully connected regressor of td_fc_online_push in front of the sums: what
 * infer_decoder.Decoder.train(data0, data1, window_size = W) takes from a labelled stretch of (eeg, attended
 * envelope, unattended envelope) rows that arrive in pushes of any length, predicted with the packed parameters
 * handed to each push.  `num_sessions` independent sessions, one state block each on the device, ONE launch per push
 * (one workgroup of 256 threads per session), nothing stored per row; however a recording is cut into pushes, the
 * state is that of one push of the whole recording, bit for bit.  (td_fccalib_: the td_fc_online_* and
 * td_calib_online_* families are each checked as a closed set against their bindings, so this one has its own.)
 *
 * The prediction p of an emitted frame is the float32 value td_fc_online_push returns in `pred` -- td_mlp_forward's
 * bits, in the operation order stated there.  Frames are emitted `post` rows late with td_online_plan's arithmetic;
 * env[..., 0] is the attended envelope a, env[..., 1] the unattended one u; windows are average_data's: consecutive,
 * hop = width, the tail dropped.
 *
 * State (td_fccalib_online_state_bytes = td_calib_online_state_bytes; all zeros = a fresh session; the HOST counts
 * the frames): td_calib_online_push's block byte for byte -- the TD_CALIB_ONLINE_SUMS float64 sums in its order,
 * advanced in frame order by the same operations (acc += (double)x * (double)y, the Grams G + z_i z_j unfused), then
 * the EEG tail [pre + post][c] and the envelope tail [post][2] float32, rounded up to 8 bytes.  td_calib_online_sums
 * and td_calib_online_finish read the head alone and serve this state as they are.
 *
 * td_fccalib_online_lds_bytes: (*pass, *bytes) of a launch that emits `emitted` frames: td_fc_online_lds_bytes'
 * formula and rule -- the 8 (4 pass) bytes that hold a pass's scores and window means there hold its frames'
 * {1, p, a, u} in float64 here -- against the same budget, TD_FC_ONLINE_LDS_BYTES.
 *
 * td_fccalib_online_push: the sessions' next n rows.
 *   eeg_dev, env_dev and their strides, n, frames_before, c, pre, post, width, flush, state_dev,
 *   state_session_stride: as td_calib_online_push (n == 0 without flush: nothing is queued; a push that emits
 *   nothing still rolls the tails)
 *   hidden_host [num_hidden], params_dev, params_session_stride (elements; 0 = one model for all): as
 *   td_fc_online_push
 * No atomics: two runs give the same bits.  With td_profile_enable the launch is bracketed as td_online_push's is.
 *
 * TD_ERR_INVALID, before anything is queued and with the state untouched -- the intersection of the two families'
 * limits: a NULL required pointer, num_sessions outside 1..65535, c outside 1..128, pre or post < 0, more than 64
 * lags, K = c (pre + 1 + post) > 8192, num_hidden outside 0..4, NULL hidden_host with num_hidden > 0, a hidden layer
 * outside 1..64 units, a shape whose pass of one frame exceeds the LDS budget, width outside 1..TD_ONLINE_MAX_WIDTH,
 * n outside 0..TD_ONLINE_MAX_PUSH, frames_before < 0, a row or session stride below a row, a parameter stride that is
 * neither 0 nor a whole model, a state stride below the state block or not a multiple of 8. */
int td_fccalib_online_state_bytes(int c, int pre, int post, int64_t* bytes);
int td_fccalib_online_lds_bytes(int c, int pre, int post, int num_hidden, const int* hidden_host, int64_t emitted,
                                int* pass, int64_t* bytes);
int td_fccalib_online_push(td_handle* h, int num_sessions, const float* eeg_dev, int64_t eeg_ld,
                           int64_t eeg_session_stride, const float* env_dev, int64_t env_ld,
                           int64_t env_session_stride, int64_t n, int64_t frames_before, int c, int pre, int post,
                           const int* hidden_host, int num_hidden, const float* params_dev,
                           int64_t params_session_stride, int width, int flush, void* state_dev,
                           int64_t state_session_stride);

/* ------------------------------------------------------------------ ingestion
 * ingest.find_mean_std, ingest.normalize_data and ingest.convert_data_to_tfrecords (ingest.py:1061-1172).
 *
 * td_ingest_moments: the joint moments of num arrays of `width` columns: data_dev[t] is [rows_host[t], width]
 * float32 (float64 when is_f64_host[t]), row stride ld_host[t].  Two passes in float64: the column sums give the
 * means, then the sums of centred squares against those means (never sum x^2).  out_dev [2 + 2 width] float64:
 * the mean and the standard deviation of everything, the column means, the column standard deviations (all
 * population moments, divided by the count).  A fixed number of launches whatever num. */
int td_ingest_moments(td_handle* h, const void* const* data_dev, const int64_t* rows_host, const int64_t* ld_host,
                      const int* is_f64_host, int num, int width, double* out_dev);
/* (a - mean) / std_dev: a_dev [rows, width] float32 (float64 when a_is_f64), row stride lda; mean_host / std_host
 * one value, or `width` values when per_column.  sub_f64: the subtraction in float64 (float32 otherwise, the mean
 * rounded to float32 first); out_f64: the division and out_dev in float64 (float32 otherwise).  A float64 input
 * needs both, and sub_f64 needs out_f64.  divide == 0: only centred.  Both operations are the correctly rounded
 * IEEE ones, so the result is numpy's bit for bit. */
int td_ingest_normalize(td_handle* h, const void* a_dev, int a_is_f64, int64_t lda, int64_t rows, int width,
                        const double* mean_host, const double* std_host, int per_column, int sub_f64, int out_f64,
                        int divide, void* out_dev, int64_t ldout);
/* The TFRecord file image of one trial, one tf.train.Example per frame: out_dev [frames * stride] bytes (16-byte
 * aligned).  template_host [stride]: one whole record with zero payloads -- the 8 length bytes (= stride - 16),
 * the masked CRC of those, the serialized Example; the last 4 bytes (the data CRC) are ignored.  Feature f is
 * feature_dev[f] [frames, width_host[f]] float32 (float64 when is_f64_host[f]: rounded to nearest even, overflow
 * to +-Inf, NaN stays NaN; float32 is copied bit for bit), row stride ld_host[f] elements; its row lands as
 * little-endian float32 at byte offset_host[f] of the record (any alignment; >= 12, inside the data).
 * reversed_host[f]: record r takes row frames - 1 - r.  Every record's data CRC (masked CRC-32C) is computed on
 * the device.  1 <= num_features <= 16. */
int td_tfrecord_encode(td_handle* h, const uint8_t* template_host, int stride, int num_features,
                       const void* const* feature_dev, const int64_t* ld_host, const int* width_host,
                       const int* offset_host, const int* is_f64_host, const int* reversed_host, int64_t frames,
                       uint8_t* out_dev);
/* The route td_tfrecord_encode takes for records of `stride` bytes.  staged 1: workgroups build `group` records
 * at a time in LDS (group * stride is a multiple of 16 and at most 48 KB) and store them with 16-byte stores;
 * staged 0 (group 0): the smallest such group does not fit, one workgroup per record writes it directly.  lanes:
 * the lanes that share one record's CRC.  Read-only; no handle. */
int td_tfrecord_route(int stride, int* staged, int* group, int* lanes);
/* The way back: checks and unpacks a TFRecord file image on the device, image_dev [frames * stride] bytes (16-byte
 * aligned), every record `stride` bytes with the same bytes outside its float payloads and its data CRC.  One pass:
 * (1) skeleton: every record against template_host [stride] (the first record with payloads and data CRC zeroed)
 * wherever mask_host [stride] is non-zero (length, length CRC, protobuf tags, names and lengths; zero on every float
 * payload and on the last 4 bytes); (2) the masked CRC-32C of bytes [12, stride - 4) of every record against the
 * stored one; (3) output o: the count_host[o] little-endian float32 at byte offset_host[o] of record r go, bit for
 * bit, to dst_dev[o][r * ld_host[o] + col_host[o] + e] (the caller folds the file's first row into dst_dev[o]; a
 * payload may serve several outputs).  0 <= num_outputs <= 16.  status_dev (one int64, 8-byte aligned): -1 when
 * every record passed, else (r << 2 | kind) of the lowest failing record r, kind 1 skeleton, 2 data CRC, skeleton
 * first when both fail there; the same value on every call.  The outputs of a file that failed are unspecified.
 * The routes are td_tfrecord_route's.  frames == 0: TD_OK, nothing is launched and status_dev is not written. */
int td_tfrecord_decode(td_handle* h, const uint8_t* image_dev, int stride, int64_t frames,
                       const uint8_t* template_host, const uint8_t* mask_host, int num_outputs,
                       const int* offset_host, const int* count_host, void* const* dst_dev, const int64_t* ld_host,
                       const int* col_host, int64_t* status_dev);

/* ------------------------------------------------------------------ raw recordings
 * ingest_brainvision.BvBrainDataFile and ingest_edf.parse_edf_file: one uploaded file image becomes a channel-major
 * matrix in one launch, and the chosen channels become the feature 'eeg' in one more.
 *
 * td_raw_decode: out_dev[s * ld_out + r * n + i] = f(sample i of signal s in data record r), n = samples_per_record.
 * Record r is the record_bytes bytes at data_offset + r * record_bytes of image_dev [image_bytes] (16-byte aligned);
 * signal s holds its n consecutive samples from byte signal_offset_host[s] of the record (signals of the file that
 * are not wanted are simply not listed).  BrainVision MULTIPLEXED: a record is a frame, n = 1, offset c * w;
 * VECTORIZED: one record, n = frames, offset c * frames * w; EDF: the header's records, offset = the sizes of the
 * signals before.  Samples are little-endian TD_RAW_INT16 or TD_RAW_FLOAT32 (w = 2 or 4 bytes); data_offset,
 * record_bytes and every signal offset are multiples of w.
 *   arith 0: out_dev float32, float(x) * float(scale_host[s]) -- one float32 multiply; offset_host[s] must be 0.
 *   arith 1: out_dev float64, scale_host[s] * (offset_host[s] + double(x)) -- a float64 add, then a multiply.
 * Each operation is rounded once and subnormal results are kept, so both are numpy's bits.
 * TD_ERR_INVALID before anything is queued: a NULL pointer, an image that is not 16-byte aligned, records that do not
 * fit the image, a signal outside its record or not aligned to w, ld_out < records * n, arith 0 with an offset, more
 * than 1024 signals.  records == 0: TD_OK, nothing is launched.  Waits for nothing. */
#define TD_RAW_INT16 0
#define TD_RAW_FLOAT32 1
int td_raw_decode(td_handle* h, const uint8_t* image_dev, int64_t image_bytes, int64_t data_offset, int64_t records,
                  int64_t record_bytes, int samples_per_record, int sample_kind, int num_signals,
                  const int64_t* signal_offset_host, const double* scale_host, const double* offset_host, int arith,
                  void* out_dev, int64_t ld_out);
/* The route td_raw_decode takes.  transposed 0 (tile_records 0): consecutive lanes take consecutive output samples of
 * one signal, loads come in runs of n samples; correct for every n.  transposed 1: runs shorter than 64 bytes
 * (n * sample_bytes < 64) of records of which at least 16 fit the 48 KB staging area -- workgroups copy tile_records
 * consecutive records into LDS with 16-byte loads and turn them there.  The number of signals does not matter; the
 * record size does.  Read-only; no handle.  TD_ERR_INVALID: n < 1, a sample size other than 2 or 4, a record
 * smaller than n samples. */
int td_raw_route(int samples_per_record, int sample_bytes, int64_t record_bytes, int* transposed, int* tile_records);
/* BrainTrial.assemble_brain_data: out_dev [frames, sum of width_host] float32 (row stride ld_out) = the sources side
 * by side in their order.  Source k is src_dev[k] [frames, width_host[k]] float32 (float64 when is_f64_host[k]:
 * rounded to nearest even, overflow to +-Inf, as astype), row stride ld_host[k] elements.  One launch.
 * 1 <= num_sources <= 1024, at most 65536 columns.  frames == 0: TD_OK, nothing is launched. */
int td_columns_assemble(td_handle* h, int num_sources, const void* const* src_dev, const int64_t* ld_host,
                        const int* width_host, const int* is_f64_host, int64_t frames, float* out_dev, int64_t ld_out);
/* The route td_columns_assemble takes.  transposed 1: every source is one column (max_width 1) and there are at
 * least 16 -- a 64 x 64 tiled transpose through LDS, loads along the frames of each source, stores along the
 * columns.  transposed 0: one lane per output element.  Read-only; no handle. */
int td_columns_route(int num_sources, int max_width, int* transposed);

/* ------------------------------------------------------------------ BioSemi BDF
 * ingest_bdf.parse_bdf_file and BrainTrial.find_status_trigger_times.
 *
 * td_raw24_decode: out_dev[s * ld_out + r * n + i] = scale_host[s] * (offset_host[s] + double(x)), n =
 * samples_per_record, x the sign-extended 24-bit little-endian sample b0 | b1 << 8 | b2 << 16 at byte
 * data_offset + r * record_bytes + signal_offset_host[s] + 3 * i of image_dev [image_bytes].  A float64 add, then a
 * multiply, each rounded once: numpy's bits.  The description of the file is td_raw_decode's (signals that are not
 * wanted are not listed, their bytes still count in record_bytes) but nothing in it needs an alignment: data_offset,
 * record_bytes and every signal offset may be any byte value.  The image must be 16-byte aligned, out_dev 8-byte
 * aligned.  No byte at or past image_bytes is read.  One route for every n >= 1, shaped for runs of 3 n >= 768 bytes
 * (BioSemi's records of one second).
 * TD_ERR_INVALID before anything is queued: a NULL pointer, an image that is not 16-byte aligned, a misaligned
 * output, records that do not fit the image, a signal outside its record, ld_out < records * n, fewer than 1 or more
 * than 1024 signals.  records == 0: TD_OK, nothing is launched.  Waits for nothing. */
int td_raw24_decode(td_handle* h, const uint8_t* image_dev, int64_t image_bytes, int64_t data_offset, int64_t records,
                    int64_t record_bytes, int samples_per_record, int num_signals, const int64_t* signal_offset_host,
                    const double* scale_host, const double* offset_host, double* out_dev, int64_t ld_out);
/* The code changes of a trigger channel, compacted in order.  signal_dev: n float64 values `stride` elements apart
 * (8-byte aligned; finite, |v| < 2^31).  code[i] = (int64)v[i] & mask (truncation toward zero), 0 < mask <= 0xffffff;
 * sample i is an event when code[i] != code[i - 1] and code[i] != 0, a code of 0 assumed before the first sample.
 *   td_code_onsets_plan   chunk = the samples a workgroup takes, groups = ceil(n / chunk).  Read-only; no handle.
 *                         TD_ERR_INVALID: n < 0.
 *   td_code_onsets_count  offsets_dev [groups + 1] int64: [g] = the events before chunk g, [groups] = the number of
 *                         events -- the 8 bytes the host reads to allocate exactly.  Two launches (n == 0: one).
 *   td_code_onsets_fill   with offsets_dev as td_code_onsets_count left it for the same signal and mask: at_dev[k] =
 *                         the sample index of event k, code_dev[k] = its code, in increasing order of the index, for
 *                         k < capacity (events from `capacity` on are not written).  One launch; capacity == 0 or
 *                         n == 0: TD_OK, nothing is launched.
 * Deterministic: per-workgroup counts, an exclusive scan by one workgroup, ranks from ballots; no workgroup waits
 * for another and no atomic is used.  Both wait for nothing. */
int td_code_onsets_plan(int64_t n, int* chunk, int64_t* groups);
int td_code_onsets_count(td_handle* h, const double* signal_dev, int64_t n, int64_t stride, int mask,
                         int64_t* offsets_dev);
int td_code_onsets_fill(td_handle* h, const double* signal_dev, int64_t n, int64_t stride, int mask,
                        const int64_t* offsets_dev, int64_t capacity, int64_t* at_dev, int32_t* code_dev);

/* ------------------------------------------------------------------ fully connected regressor
 * brain_model.BrainModelDNN (reference brain_model.py:486-549): Dense layers z = a.W + b in float32, ReLU on
 * the num_hidden hidden layers (hidden_host[i] units each), a linear output layer of d units.  The input is
 * the lagged view of x exactly as td_predict_fir reads it (column l*C + c = x~[t + l - pre, c], zero outside
 * the file, input_offset, file_offsets_host) -- never materialised.
 * Parameters: ONE packed float32 buffer in Keras order [W1 (K x h1, row-major, rows in the lag layout), b1,
 * W2, b2, ..., WL, bL], K = c (pre + 1 + post).
 * Limits (TD_ERR_INVALID before anything is queued): c <= 128 (context-free input, pre = post = 0: any c with
 * K <= 8192), pre + 1 + post <= 64, K <= 8192, num_hidden <= 4, 1 <= hidden units <= 64, 1 <= d <= 8,
 * 1 <= batch_rows <= 2048.
 *
 * td_mlp_train: `epochs` epochs of minibatch RMSprop (Keras, momentum 0: v = rho v + (1 - rho) g^2,
 * w -= lr g / (sqrt(v) + eps)) on the loss mean((p - y)^2) over rows x outputs, every layer updated after the
 * full backward pass.  The stream is the files' zipped rows, rows_used_host[f] of file f (NULL = all; the
 * caller's drop_remainder), cut into minibatches of batch_rows (a shorter last one allowed).  shuffle_seed < 0:
 * minibatch s of every epoch is stream rows [s B, (s + 1) B); >= 0: slot i of epoch e is stream row
 * perm(i), a bijection of [0, n): 4 Feistel rounds on 2 x half bits (the smallest even bit count with
 * 2^bits >= n), round key r = mix(lo ^ mix(hi ^ mix(4 e + r))) of the seed's 32-bit halves, round
 * (L, R) -> (R, L ^ (mix(R ^ key) & mask)), mix = the 32-bit finaliser x ^= x >> 16, x *= 0x7feb352d,
 * x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16, re-applied while the value is >= n (cycle walking).
 * params_dev / state_dev (the RMSprop accumulators, same layout; zeros for a fresh optimizer) are read and,
 * once every launch has been queued, overwritten; a failure leaves them unchanged.  stats_dev
 * [epochs x steps][6] float64 receives per step, from the forward pass before that step's update: sum p,
 * sum y, sum p^2, sum y^2, sum p y of output column 0 and sum (p - y)^2 over every output.
 * Three launches per step and one per epoch, queued from the host without waiting (no persistent grid).
 * Deterministic: fixed reduction orders, no atomics. */
int td_mlp_train(td_handle* h, const float* x_dev, int64_t ldx, const int64_t* file_offsets_host, int num_files,
                 int c, int pre, int post, int input_offset, const int64_t* rows_used_host, const float* y_dev,
                 int64_t ldy, int d, const int* hidden_host, int num_hidden, int batch_rows, int epochs,
                 float* params_dev, float* state_dev, float lr, float rho, float eps, int64_t shuffle_seed,
                 double* stats_dev);
/* The loss sums (stats_dev [6], as above) and the gradient of every parameter (grad_dev, the packed layout) of
 * minibatch batch_index of the unshuffled stream at params_dev, without an update: the training step's own
 * launches, the update launch writing the gradient instead of applying it. */
int td_mlp_grad(td_handle* h, const float* x_dev, int64_t ldx, const int64_t* file_offsets_host, int num_files,
                int c, int pre, int post, int input_offset, const int64_t* rows_used_host, const float* y_dev,
                int64_t ldy, int d, const int* hidden_host, int num_hidden, int batch_rows, int batch_index,
                const float* params_dev, float* grad_dev, double* stats_dev);
/* td_mlp_train / td_mlp_grad with the loss as an argument: loss 0 = mse (the same launches and bits as the
 * entry points above), loss 1 = the Pearson correlation loss (reference brain_model.py:94-126 under Keras'
 * mean over frames); any other value is TD_ERR_INVALID.  Loss 1, for a step of B rows, per output column o:
 * pm = p - mean p, ym = y - mean y over the step's rows, Spp = sum pm^2, Syy = sum ym^2, Spy = sum pm ym,
 * r_o = Spy / sqrt(Spp Syy),
 *   L = -(1 / B) sum_o r_o,   dL/dp[i, o] = -(1 / B) (ym[i, o] / sqrt(Spp Syy) - r_o pm[i, o] / Spp).
 * The five raw sums per column (sum p, y, p^2, y^2, p y of the float32 p and y) are float64, rows in order
 * within a workgroup's 64 rows, the workgroups' partials in workgroup order; r_o and the coefficients are
 * float64; each dL/dp entry is formed in float64 and rounded once to float32.  The backward pass and RMSprop
 * are those of loss 0, except that the output layer's bias gradient -- identically zero, the loss does not
 * change with a shift of p -- is written as exact 0.  Zero rule: a column with
 * sum p^2 - (sum p)^2 / B <= 32 eps64 sum p^2 (or the same in y), that is, constant within the step, has
 * r_o = 0 and a zero dL/dp column for that step (the reference divides by zero there).
 * stats_dev holds SEVEN float64 per step with loss 1 ([epochs x steps][7]; td_mlp_grad_loss: [7]): the six
 * sums above, then the step's L.  With loss 0 the stride stays six.  Loss 1 is four launches a step (the
 * head runs twice: moments, then the backward pass); no launch waits on another workgroup. */
int td_mlp_train_loss(td_handle* h, const float* x_dev, int64_t ldx, const int64_t* file_offsets_host,
                      int num_files, int c, int pre, int post, int input_offset, const int64_t* rows_used_host,
                      const float* y_dev, int64_t ldy, int d, const int* hidden_host, int num_hidden,
                      int batch_rows, int epochs, float* params_dev, float* state_dev, float lr, float rho,
                      float eps, int64_t shuffle_seed, double* stats_dev, int loss);
int td_mlp_grad_loss(td_handle* h, const float* x_dev, int64_t ldx, const int64_t* file_offsets_host,
                     int num_files, int c, int pre, int post, int input_offset, const int64_t* rows_used_host,
                     const float* y_dev, int64_t ldy, int d, const int* hidden_host, int num_hidden, int batch_rows,
                     int batch_index, const float* params_dev, float* grad_dev, double* stats_dev, int loss);
/* Inference over whole recordings: out_dev [rows, d] (row stride ldout), output row file_offsets[f] + t =
 * frame t of file f (as td_predict_fir); three launches per 4096 rows. */
int td_mlp_forward(td_handle* h, const float* x_dev, int64_t ldx, const int64_t* file_offsets_host, int num_files,
                   int c, int pre, int post, int input_offset, int d, const int* hidden_host, int num_hidden,
                   const float* params_dev, float* out_dev, int64_t ldout);

/* ------------------------------------------------------------------ match-mismatch classifier
 * brain_model.BrainModelClassifier (reference brain_model.py:554-620): the td_mlp_* network and kernels with
 *  - a second lagged view behind the first: input = [input_1 | input_2], input_2 column l*c2 + ch =
 *    x2~[t + l - pre2, ch] of x2_dev (the files of file_offsets_host, row stride ldx2), zero outside the file;
 *    a negative input_offset drops the leading rows of x2 as it does the target's.  W1 has K1 + K2 rows,
 *    K1 = c (pre + 1 + post) first, then K2 = c2 (pre2 + 1 + post2);
 *  - a sigmoid on the d output units and the binary cross-entropy, evaluated on the output logit z:
 *    entry loss = max(z, 0) - z y + log1p(exp(-|z|)) (expf / log1pf), the loss its mean over rows x outputs,
 *    dL/dz = (sigma(z) - y) / (rows d);
 *  - Adam (Keras, no amsgrad): m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, w -= lr_t m / (sqrt(v) + eps),
 *    lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) computed per update in double on the host and rounded to float32
 *    (as are 1 - b1 and 1 - b2); update i of the call has t = step0 + i + 1, step0 = the updates already
 *    applied.  state_dev holds 2 P floats: m [P], then v [P] (zeros for a fresh optimizer).
 * The six float64 sums per step are, for this family: slot 0 = the number of entries with
 * (z > 0) == (y > 0.5) (binary accuracy at threshold 0.5 times rows x d), slot 5 = the sum of the entry
 * losses, slots 1 - 4 = 0.
 * Everything else -- the stream, rows_used_host, shuffle_seed, the packed parameter layout, working on copies
 * and committing them once every launch is queued, determinism -- is as td_mlp_train.
 * Limits: those of td_mlp_*, plus K1 + K2 <= 8192, c2 <= 128 (context-free second input: any c2 within K),
 * pre2 + 1 + post2 <= 64.
 *
 * td_mlpc_train: update != 0 trains; update == 0 runs the forward passes only (params_dev is not written,
 * state_dev may be NULL) and fills stats_dev -- what evaluate uses. */
int td_mlpc_train(td_handle* h, const float* x_dev, int64_t ldx, const float* x2_dev, int64_t ldx2,
                  const int64_t* file_offsets_host, int num_files, int c, int pre, int post, int c2, int pre2,
                  int post2, int input_offset, const int64_t* rows_used_host, const float* y_dev, int64_t ldy, int d,
                  const int* hidden_host, int num_hidden, int batch_rows, int epochs, float* params_dev,
                  float* state_dev, double lr, double beta1, double beta2, double eps, int64_t step0, int update,
                  int64_t shuffle_seed, double* stats_dev);
/* The sums (stats_dev [6], as above) and the gradient of the mean binary cross-entropy in every parameter of
 * minibatch batch_index of the unshuffled stream, without an update (as td_mlp_grad). */
int td_mlpc_grad(td_handle* h, const float* x_dev, int64_t ldx, const float* x2_dev, int64_t ldx2,
                 const int64_t* file_offsets_host, int num_files, int c, int pre, int post, int c2, int pre2,
                 int post2, int input_offset, const int64_t* rows_used_host, const float* y_dev, int64_t ldy, int d,
                 const int* hidden_host, int num_hidden, int batch_rows, int batch_index, const float* params_dev,
                 float* grad_dev, double* stats_dev);
/* Inference over whole recordings: out_dev [rows, d] receives the probabilities sigma(z) of every frame of
 * every file (rows as td_mlp_forward). */
int td_mlpc_forward(td_handle* h, const float* x_dev, int64_t ldx, const float* x2_dev, int64_t ldx2,
                    const int64_t* file_offsets_host, int num_files, int c, int pre, int post, int c2, int pre2,
                    int post2, int input_offset, int d, const int* hidden_host, int num_hidden,
                    const float* params_dev, float* out_dev, int64_t ldout);

/* ------------------------------------------------------------------ many regressors in one fit
 * td_mlp_train_loss for num_models regressors of ONE architecture on the same recordings, in one chain of
 * launches: the folds of a jackknife (brain_model.fit_many, regression.jackknife_dnn), the learning rates of
 * a sweep.  Shared: x, y, the files, c / pre / post / input_offset, d, the hidden widths, batch_rows, epochs
 * and the loss (0 = mse, 1 = Pearson).  Per model m, as host arrays of num_models entries:
 * rows_used_host[m][num_files] (its stream; a file the model does not train on has 0 rows, at any position),
 * params_dev_host[m] / state_dev_host[m] (DEVICE pointers to its packed parameters and RMSprop accumulators,
 * as td_mlp_train), lr_host[m], rho_host[m], eps_host[m], shuffle_seed_host[m] (< 0: in order).
 * Model m has steps_m = ceil(its rows / batch_rows) steps an epoch.  Round t of the call carries launch t of
 * every model's own fit -- the update of its step t - 1 and the forward of its step t, epoch t / steps_m --
 * with the models in the grid's second dimension; a model whose epochs x steps_m launches are done idles.  The
 * call queues max_m(epochs steps_m) + 1 rounds.  No atomics, no wait between workgroups, the reduction orders
 * of td_mlp_train: model m's parameters, state and sums are bit for bit those of its own td_mlp_train_loss.
 * stats_dev: [num_models][epochs][max_steps][6 (loss 0) or 7 (loss 1)] float64, max_steps = max_m steps_m;
 * model m fills its first steps_m entries of every epoch, the others are not written.
 * Every argument of every model is checked before anything is queued (TD_ERR_INVALID: nothing has changed);
 * the call works on copies and overwrites params / state of every model once the last launch is queued.  Two
 * models may not share a buffer.  At most TD_DNN_MANY_MAX_MODELS models a call: a model's scratch is its row
 * tables (16 B per stream row; two of them when shuffled), the first layer's partial sums
 * (4 B x ceil(K / 64 .. ) slices x h1 x batch_rows) and the copies -- 11 MB at 240 000 rows, K = 2368,
 * [20, 20], batch 512, so 0.7 GB at the cap.  Limits otherwise as td_mlp_train. */
#define TD_DNN_MANY_MAX_MODELS 64
int td_dnn_train_many(td_handle* h, const float* x_dev, int64_t ldx, const int64_t* file_offsets_host, int num_files,
                      int c, int pre, int post, int input_offset, const float* y_dev, int64_t ldy, int d,
                      const int* hidden_host, int num_hidden, int batch_rows, int epochs, int loss, int num_models,
                      const int64_t* rows_used_host, float* const* params_dev_host, float* const* state_dev_host,
                      const float* lr_host, const float* rho_host, const float* eps_host,
                      const int64_t* shuffle_seed_host, double* stats_dev);

/* ------------------------------------------------------------------ many classifiers in one fit, or one scoring
 * td_mlpc_train for num_models classifiers of ONE architecture on the same recordings, with the structure of
 * td_dnn_train_many: round t carries launch t of every model's own td_mlpc_train, models in the grid's second
 * dimension, a model whose launches are done idles; no atomics, no wait between workgroups.  Shared: x, x2, y,
 * the files, both views' c / pre / post, input_offset, d, the hidden widths, batch_rows, epochs and update.
 * Per model m, as host arrays of num_models entries: rows_used_host[m][num_files], params_dev_host[m],
 * state_dev_host[m] (DEVICE pointers; the state is 2 P floats, Adam's m then v), lr_host[m], beta1_host[m],
 * beta2_host[m], eps_host[m] (doubles, each rounded once as td_mlpc_train rounds them), step0_host[m] (the
 * updates the model has already had) and shuffle_seed_host[m] (< 0: in order).
 * update != 0 trains: model m's parameters, m, v and six sums per step are bit for bit those of its own
 * td_mlpc_train with its rows_used, settings and step0.  lr_t of update k of model m (t = step0 + k + 1) is
 * computed on the host in double and rounded once, exactly as td_mlpc_train computes it per launch, for every
 * update of the call; the table travels in the call's scratch and the update of step k reads entry k.
 * update == 0 scores: epochs must be 1, rows are visited in order (the seeds are not read), no parameter is
 * written, the optimizer's arrays and state_dev_host (or its entries) may be NULL, and two entries may name the
 * same parameters.  Model m's six sums per step are those of td_mlpc_train(..., update = 0) on its rows_used:
 * what brain_model.evaluate_many uses, rows_used zero everywhere but on the files scored.
 * stats_dev: [num_models][epochs][max_steps][6] float64, as td_dnn_train_many.
 * Checks, copies and the commit as td_dnn_train_many; at most TD_DNN_MANY_MAX_MODELS models a call.  A model's
 * scratch is that of td_dnn_train_many with the doubled state (8 B a parameter) and its lr_t table (4 B per
 * update of the call). */
int td_clf_train_many(td_handle* h, const float* x_dev, int64_t ldx, const float* x2_dev, int64_t ldx2,
                      const int64_t* file_offsets_host, int num_files, int c, int pre, int post, int c2, int pre2,
                      int post2, int input_offset, const float* y_dev, int64_t ldy, int d, const int* hidden_host,
                      int num_hidden, int batch_rows, int epochs, int update, int num_models,
                      const int64_t* rows_used_host, float* const* params_dev_host, float* const* state_dev_host,
                      const double* lr_host, const double* beta1_host, const double* beta2_host,
                      const double* eps_host, const int64_t* step0_host, const int64_t* shuffle_seed_host,
                      double* stats_dev);

#ifdef __cplusplus
}
#endif
#endif /* TD_HOTPATH_H_ */
