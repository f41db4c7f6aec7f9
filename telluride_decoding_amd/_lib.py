"""ctypes binding of libtd_hotpath.so (the C-ABI in include/td_hotpath.h).

The product path has no CPU fallback: if the HIP library is missing or no
MI355X is visible, every entry point raises `HotPathUnavailable`.
"""
import ctypes
import os
import re

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
# (TD_HOTPATH_LIB: development -- A/B runs of two builds of the library in one GPU session)
LIB_PATH = os.environ.get('TD_HOTPATH_LIB') or os.path.join(PKG, 'libtd_hotpath.so')
HEADER = os.path.join(os.path.dirname(PKG), 'include', 'td_hotpath.h')

TD_OK = 0
TD_ERR_INVALID = -1
TD_ERR_HIP = -2
TD_ERR_SINGULAR = -3
TD_ERR_NOMEM = -4
TD_ERR_STATE = -5
TD_SOLVER_AUTO, TD_SOLVER_CHOLESKY, TD_SOLVER_CG = 0, 1, 2


class HotPathUnavailable(RuntimeError):
  """The HIP extension (or a GPU) is missing; there is no CPU fallback."""


class HotPathError(RuntimeError):
  pass


_c = ctypes
_vp, _i, _i64, _f, _d, _sz = (_c.c_void_p, _c.c_int, _c.c_int64, _c.c_float,
                              _c.c_double, _c.c_size_t)
_pi64 = _c.POINTER(_c.c_int64)
_pd = _c.POINTER(_c.c_double)

# The td_mlp_* / td_mlpc_* prototypes are built from the groups their parameter lists share, so each entry below
# reads as its prototype in include/td_hotpath.h does (tests/test_cpu_dnn.py checks them against the header).
_X = [_vp, _i64]                        # x_dev, ldx (x2_dev, ldx2)
_FILES = [_pi64, _i]                    # file_offsets_host, num_files
_VIEW = [_i, _i, _i]                    # c, pre, post (c2, pre2, post2)
_TARGETS = [_vp, _i64, _i]              # y_dev, ldy, d
_NETWORK = [_c.POINTER(_i), _i]         # hidden_host, num_hidden
_MLP = [_vp] + _X + _FILES + _VIEW                      # the handle, then one view of the files
_MLPC = [_vp] + _X + _X + _FILES + _VIEW + _VIEW        # ... two views
_FIT = [_i, _pi64] + _TARGETS + _NETWORK + [_i]         # input_offset, rows_used_host, ..., batch_rows
_EPOCHS = [_i, _vp, _vp]                # epochs, params_dev, state_dev (the optimizer's settings follow)
_SEED_STATS = [_i64, _vp]               # shuffle_seed, stats_dev
_GRAD = [_i, _vp, _vp, _vp]             # batch_index, params_dev, grad_dev, stats_dev
_FORWARD = [_i, _i] + _NETWORK + [_vp, _vp, _i64]       # input_offset, d, ..., params_dev, out_dev, ldout
_pf = _c.POINTER(_f)
# per model, host arrays: rows_used, params_dev / state_dev pointers, lr, rho, eps, shuffle_seed
_MANY = [_pi64, _c.POINTER(_vp), _c.POINTER(_vp), _pf, _pf, _pf, _pi64]
# ... the classifier's: rows_used, params_dev / state_dev pointers, lr, beta1, beta2, eps, step0, shuffle_seed
_MANY_ADAM = [_pi64, _c.POINTER(_vp), _c.POINTER(_vp), _pd, _pd, _pd, _pd, _pi64, _pi64]

# name -> argtypes (restype is int unless listed in _RESTYPE)
SIGNATURES = {
    'td_version': [],
    'td_device_count': [_c.POINTER(_i)],
    'td_create': [_i, _c.POINTER(_vp)],
    'td_destroy': [_vp],
    'td_last_error': [_vp],
    'td_set_stream': [_vp, _vp],
    'td_use_own_stream': [_vp],
    'td_stream_create_masked': [_i, _i, _i, _c.POINTER(_vp)],
    'td_stream_destroy': [_vp],
    'td_set_accumulate_mode': [_vp, _i],
    'td_synchronize': [_vp],
    'td_malloc': [_vp, _sz, _c.POINTER(_vp)],
    'td_free': [_vp, _vp],
    'td_memcpy_h2d': [_vp, _vp, _vp, _sz],
    'td_memcpy_d2h': [_vp, _vp, _vp, _sz],
    'td_memset': [_vp, _vp, _i, _sz],
    'td_timer_start': [_vp],
    'td_timer_stop': [_vp, _c.POINTER(_f)],
    'td_profile_enable': [_vp, _i],
    'td_set_cu_count': [_vp, _i],
    'td_probe_bf16_mfma': [_vp, _i, _pd],
    'td_profile_read': [_vp, _pi64, _pd, _pd],
    'td_stats_create': [_vp, _i, _i, _i, _i, _i, _i, _i, _c.POINTER(_vp)],
    'td_stats_destroy': [_vp, _vp],
    'td_stats_reset': [_vp, _vp],
    'td_stats_complete': [_vp, _vp],
    'td_stats_accumulate': [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _pi64, _i, _i,
                            _pi64],
    'td_stats_accumulate_parts': [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _pi64, _i, _i,
                            _pi64, _i],
    'td_stats_accumulate_ranges': [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _pi64, _i, _i,
                                   _pi64, _pi64, _pi64, _c.POINTER(_i), _i],
    'td_stats_counts': [_vp, _vp, _pi64, _pi64],
    'td_stats_combine': [_vp, _vp, _c.POINTER(_vp), _i],
    'td_stats_packed_len': [_vp, _vp, _i64, _pi64],
    'td_stats_pack': [_vp, _vp, _vp, _i64, _i64],
    'td_stats_unpack': [_vp, _vp, _vp, _i64],
    'td_stats_unpack_known': [_vp, _vp, _vp, _i64, _i64],
    'td_stats_accumulate_each': [_vp, _c.POINTER(_vp), _vp, _i64, _vp, _i64, _pi64, _i, _i, _pi64, _c.POINTER(_i)],
    'td_stats_allreduce': [_vp, _vp, _vp, _i64, _i64, _i64],
    'td_allreduce_f64': [_vp, _vp, _i64, _vp],
    'td_rccl_available': [_vp],
    'td_rccl_unique_id': [_vp, _vp],
    'td_rccl_comm_create': [_vp, _i, _i, _vp, _c.POINTER(_vp)],
    'td_rccl_comm_count': [_vp, _vp, _c.POINTER(_i)],
    'td_rccl_comm_destroy': [_vp, _vp],
    'td_stats_moments': [_vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'td_ridge_solve': [_vp, _vp, _pd, _i, _vp, _vp],
    'td_set_solver': [_vp, _i],
    'td_set_option': [_vp, _c.c_char_p, _i64],
    'td_scratch_bytes': [_vp, _pi64],
    'td_last_solve_info': [_vp, _c.POINTER(_i), _c.POINTER(_i), _c.POINTER(_i)],
    'td_last_cg_plan': [_vp, _c.POINTER(_i), _c.POINTER(_i), _c.POINTER(_i)],
    'td_ridge_solve_async': [_vp, _vp, _pd, _i, _vp, _vp, _vp],
    'td_ridge_solve_multi': [_vp, _c.POINTER(_vp), _i, _pd, _i, _vp, _vp, _vp],
    'td_ridge_solve_loso': [_vp, _vp, _c.POINTER(_vp), _i, _pd, _i, _i, _d, _vp, _vp, _c.POINTER(_i),
                            _c.POINTER(_i)],
    'td_ridge_solve_loso_terms': [_vp, _vp, _c.POINTER(_vp), _c.POINTER(_i), _pd, _i, _pd, _i, _i, _d, _i, _vp, _vp,
                                  _c.POINTER(_i), _c.POINTER(_i)],
    'td_cca_solve_loso_terms': [_vp, _vp, _c.POINTER(_vp), _c.POINTER(_i), _pd, _i, _pi64, _i, _pd, _i, _i, _d, _vp,
                                _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'td_spd_solve': [_vp, _vp, _vp, _i, _i, _i],
    'td_general_solve': [_vp, _vp, _vp, _i, _i],
    'td_shrinkage_moment': [_vp, _vp, _i64, _i, _i, _i, _pi64, _i, _i, _pi64, _i64, _vp],
    'td_shrinkage_terms': [_vp, _vp, _i64, _i, _vp, _c.c_double, _pd],
    'td_shrunk_covariance': [_vp, _vp, _i64, _i, _c.c_double, _c.c_double, _vp, _vp],
    'td_predict_fir': [_vp, _vp, _i64, _pi64, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i64],
    'td_predict_fir_per_file': [_vp, _vp, _i64, _pi64, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i64],
    'td_cca_transform': [_vp, _vp, _i64, _i, _i, _i, _vp, _i64, _i, _i, _i, _pi64, _i, _i,
                         _vp, _vp, _vp, _vp, _i, _vp, _i64],
    'td_cca_solve': [_vp, _vp, _d, _d, _d, _i, _vp, _vp, _vp, _vp, _vp, _c.POINTER(_i)],
    'td_sym_eigh': [_vp, _vp, _i, _vp, _vp, _c.POINTER(_i)],
    'td_jacobi_svd': [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _c.POINTER(_i)],
    'td_window_count': [_pi64, _i, _i, _i, _pi64, _pi64],
    'td_window_sums': [_vp, _vp, _i64, _vp, _i64, _i, _pi64, _i, _i, _i, _vp],
    'td_window_sums_cycled': [_vp, _vp, _i64, _vp, _i64, _i, _i, _pi64, _i, _i, _i, _vp],
    'td_window_scores': [_vp, _vp, _i64, _i, _i, _i, _i, _pd, _pd, _pd, _vp],
    'td_window_pearson': [_vp, _vp, _i64, _i, _i, _i, _vp],
    'td_frame_scores': [_vp, _vp, _i64, _vp, _i64, _i, _i64, _i, _pd, _pd, _pd, _pd, _d,
                        _d, _vp],
    'td_window_means': [_vp, _vp, _pi64, _i, _i, _i, _vp],
    'td_window_class_moments': [_vp, _vp, _i64, _vp, _i64, _i, _i64, _i, _pd, _pd, _pd, _vp, _vp],
    'td_decide_wta': [_vp, _vp, _vp, _i64, _vp],
    'td_decide_step': [_vp, _vp, _vp, _pi64, _i, _vp, _pd],
    'td_decode_ssd': [_vp, _vp, _vp, _pi64, _i, _pd, _pd, _vp],
    'td_decode_ssd_stream': [_vp, _vp, _vp, _pi64, _i, _pd, _pd, _vp, _vp],
    'td_ssd_state_doubles': [],
    'td_attention_sweep': [_vp, _vp, _i64, _vp, _i64, _i, _vp, _i64, _c.POINTER(_i), _i, _i, _vp, _vp, _vp],
    'td_decode_fused': [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _i64, _pi64, _i, _i,
                        _i, _pd, _vp, _vp],
    'td_online_state_bytes': [_i, _i, _i, _i, _pi64],
    'td_online_plan': [_i64, _i64, _i, _i, _i, _i, _pi64, _pi64, _pi64, _pi64],
    # h, sessions | eeg, ld, stride | env, ld, stride | n, c, pre, post | w, stride, b, stride | corr, reduction,
    # lda | width, hop, decoder, frames_before, flush | state, stride | scores, decisions, pred, frame
    'td_online_push': [_vp, _i] + [_vp, _i64, _i64] * 2 + [_i64, _i, _i, _i] + [_vp, _i64] * 2 +
                      [_vp, _i, _vp] + [_i, _i, _i, _i64, _i] + [_vp, _i64] + [_vp, _vp, _vp, _vp],
    'td_cca_online_state_bytes': _VIEW + _VIEW + [_i, _pi64],
    'td_cca_online_lds_bytes': _VIEW + _VIEW + [_i, _i64, _c.POINTER(_i), _pi64],
    # h, sessions | eeg, ld, stride | feat1, feat2, ld, stride | n | c1, pre1, post1 | c2, pre2, post2 | dims |
    # mean_x, rot_x, mean_y, rot_y, model stride | corr, reduction, lda | width, hop, decoder, frames_before,
    # flush | state, stride | scores, decisions, proj, frame
    'td_cca_online_push': [_vp, _i] + [_vp, _i64, _i64] + [_vp, _vp, _i64, _i64] + [_i64] + _VIEW + _VIEW + [_i] +
                          [_vp, _vp, _vp, _vp, _i64] + [_vp, _i, _vp] + [_i, _i, _i, _i64, _i] + [_vp, _i64] +
                          [_vp, _vp, _vp, _vp],
    'td_fc_online_lds_bytes': [_i, _i, _i, _i, _c.POINTER(_i), _i64, _c.POINTER(_i), _pi64],
    # h, sessions | eeg, ld, stride | env, ld, stride | n, c, pre, post | hidden, num_hidden | params, stride | corr,
    # reduction, lda | width, hop, decoder, frames_before, flush | state, stride | scores, decisions, pred, frame
    'td_fc_online_push': [_vp, _i] + [_vp, _i64, _i64] * 2 + [_i64, _i, _i, _i] + [_c.POINTER(_i), _i] +
                          [_vp, _i64] + [_vp, _i, _vp] + [_i, _i, _i, _i64, _i] + [_vp, _i64] + [_vp, _vp, _vp, _vp],
    'td_sos_filter': [_vp, _vp, _i, _i64, _i, _pi64, _i, _pd, _i, _i, _pd, _i, _vp, _vp, _pi64, _vp, _i64],
    'td_sos_filter_plan': [_i64, _i64, _i, _c.POINTER(_i), _c.POINTER(_i)],
    'td_reref_select': [_vp, _vp, _i, _i64, _i, _vp, _i64, _i, _c.POINTER(_i), _c.POINTER(_i),
                        _c.POINTER(_i), _c.POINTER(_i), _c.POINTER(_i), _i, _vp, _i64],
    'td_mean_f64': [_vp, _vp, _i64, _i, _i64, _vp],
    'td_context_out': [_vp, _vp, _i64, _i, _i64, _vp, _i64, _i, _i, _d, _d, _vp, _vp, _i64, _vp],
    'td_frontend_state_bytes': [_i, _i, _pi64],
    'td_frontend_plan': [_i64, _i64, _d, _d, _i, _pi64, _pi64, _pi64],
    'td_frontend_lds_bytes': [_i, _i, _i64, _c.POINTER(_i), _pi64],
    # h, sessions | x, is_f64, ld, stride | n, c | sos, sections, split, zi | fs_in, fs_out | groups, ref_ptr, ref_idx,
    # chan_ptr, chan_idx | sel, cs | mean, std, stride | rows_before, flush | state, stride | out32, out64, ld, stride
    'td_frontend_push': [_vp, _i] + [_vp, _i, _i64, _i64] + [_i64, _i] + [_pd, _i, _i, _pd] + [_d, _d] +
                        [_i] + [_c.POINTER(_i)] * 4 + [_c.POINTER(_i), _i] + [_vp, _vp, _i64] + [_i64, _i] +
                        [_vp, _i64] + [_vp, _vp, _i64, _i64],
    'td_audio_intensity': [_vp, _vp, _i64, _vp, _i, _i64, _i64, _i, _i, _i64, _d, _d, _d, _i, _d, _vp, _vp],
    'td_audio_passthrough': [_vp, _vp, _i64, _vp, _i, _i64, _i64, _i, _i, _i64, _i64, _i, _d, _vp, _vp],
    'td_audio_spectrogram': [_vp, _vp, _i64, _i, _i, _i, _pd, _i, _i64, _vp],
    'td_audio_online_plan': [_i64, _i64, _d, _d, _d, _i, _pi64, _pi64, _pi64, _pi64],
    'td_audio_online_state_bytes': [_i, _i64, _pi64],
    # h, sessions | x, type, ld, stride | n, c | rows_before, flush | fs_in, fs_out, window, exponent |
    # state, stride, live | out32, out64, ld, stride | windows
    'td_audio_online_push': [_vp, _i] + [_vp, _i, _i64, _i64] + [_i64, _i] + [_i64, _i] + [_d, _d, _d, _d] +
                            [_vp, _i64, _i] + [_vp, _vp, _i64, _i64] + [_vp],
    'td_fit_online_state_bytes': [_i, _i, _i, _i, _pi64],
    # h, sessions | eeg, ld, stride | target, ld, stride | n, c, pre, post, d | frames_before, pushes_before, flush |
    # forget | state, stride
    'td_fit_online_push': [_vp, _i] + [_vp, _i64, _i64] * 2 + [_i64, _i, _i, _i, _i] + [_i64, _i64, _i] + [_d] +
                          [_vp, _i64],
    'td_fit_online_moments': [_vp, _i, _vp, _i64, _i, _i, _i, _i, _vp, _vp],
    # h, sessions | state, stride | c, pre, post, d | frames_emitted | lambdas, n_lambda | w, b
    'td_fit_online_solve': [_vp, _i, _vp, _i64, _i, _i, _i, _i, _i64, _pd, _i, _vp, _vp],
    'td_ccafit_online_state_bytes': _VIEW + _VIEW + [_pi64],
    # h, sessions | eeg, ld, stride | feat, ld, stride | n | c1, pre1, post1 | c2, pre2, post2 | frames_before,
    # pushes_before, flush | forget | state, stride
    'td_ccafit_online_push': [_vp, _i] + [_vp, _i64, _i64] * 2 + [_i64] + _VIEW + _VIEW + [_i64, _i64, _i] + [_d] +
                             [_vp, _i64],
    'td_ccafit_online_moments': [_vp, _i, _vp, _i64] + _VIEW + _VIEW + [_vp, _vp, _vp, _vp],
    # h, sessions | state, stride | the two views | frames_emitted | lambdas, n_lambda | dim, eps_eig | rot_x, rot_y,
    # mean_x, mean_y, e, corr | info
    'td_ccafit_online_solve': [_vp, _i, _vp, _i64] + _VIEW + _VIEW + [_i64, _pd, _i] + [_i, _d] + [_vp] * 6 +
                              [_c.POINTER(_i)],
    'td_calib_online_state_bytes': [_i, _i, _i, _pi64],
    # h, sessions | eeg, ld, stride | env, ld, stride | w, stride | b, stride | n, frames_before | c, pre, post, width,
    # flush | state, stride
    'td_calib_online_push': [_vp, _i] + [_vp, _i64, _i64] * 2 + [_vp, _i64] * 2 + [_i64, _i64] + [_i] * 5 +
                            [_vp, _i64],
    'td_calib_online_sums': [_vp, _i, _vp, _i64, _vp],
    # h, sessions | state, stride | frames_emitted, width | corr, lda, dprime, status
    'td_calib_online_finish': [_vp, _i, _vp, _i64, _i64, _i, _vp, _vp, _vp, _vp],
    'td_ccacalib_online_state_bytes': _VIEW + _VIEW + [_i, _pi64],
    'td_ccacalib_online_lds_bytes': _VIEW + _VIEW + [_i, _i64, _c.POINTER(_i), _pi64],
    # h, sessions | eeg, ld, stride | attended, unattended, ld, stride | n | c1, pre1, post1 | c2, pre2, post2 | dims |
    # mean_x, rot_x, mean_y, rot_y, model stride | width, frames_before, flush | state, stride
    'td_ccacalib_online_push': [_vp, _i] + [_vp, _i64, _i64] + [_vp, _vp, _i64, _i64] + [_i64] + _VIEW + _VIEW + [_i] +
                               [_vp, _vp, _vp, _vp, _i64] + [_i, _i64, _i] + [_vp, _i64],
    'td_ccacalib_online_sums': [_vp, _i, _vp, _i64, _i, _vp],
    # h, sessions | state, stride | dims | frames_emitted, width | corr, lda, dprime, status
    'td_ccacalib_online_finish': [_vp, _i, _vp, _i64, _i, _i64, _i, _vp, _vp, _vp, _vp],
    'td_fccalib_online_state_bytes': [_i, _i, _i, _pi64],
    'td_fccalib_online_lds_bytes': [_i, _i, _i, _i, _c.POINTER(_i), _i64, _c.POINTER(_i), _pi64],
    # h, sessions | eeg, ld, stride | env, ld, stride | n, frames_before | c, pre, post | hidden, num_hidden | params,
    # stride | width, flush | state, stride
    'td_fccalib_online_push': [_vp, _i] + [_vp, _i64, _i64] * 2 + [_i64, _i64] + [_i, _i, _i] +
                              [_c.POINTER(_i), _i] + [_vp, _i64] + [_i, _i] + [_vp, _i64],
    'td_ingest_moments': [_vp, _c.POINTER(_vp), _pi64, _pi64, _c.POINTER(_i), _i, _i, _vp],
    'td_ingest_normalize': [_vp, _vp, _i, _i64, _i64, _i, _pd, _pd, _i, _i, _i, _i, _vp, _i64],
    'td_tfrecord_encode': [_vp, _c.c_char_p, _i, _i, _c.POINTER(_vp), _pi64, _c.POINTER(_i), _c.POINTER(_i),
                           _c.POINTER(_i), _c.POINTER(_i), _i64, _vp],
    'td_tfrecord_route': [_i, _c.POINTER(_i), _c.POINTER(_i), _c.POINTER(_i)],
    'td_tfrecord_decode': [_vp, _vp, _i, _i64, _c.c_char_p, _c.c_char_p, _i, _c.POINTER(_i), _c.POINTER(_i),
                           _c.POINTER(_vp), _pi64, _c.POINTER(_i), _vp],
    'td_raw_decode': [_vp, _vp, _i64, _i64, _i64, _i64, _i, _i, _i, _pi64, _pd, _pd, _i, _vp, _i64],
    'td_raw_route': [_i, _i, _i64, _c.POINTER(_i), _c.POINTER(_i)],
    'td_columns_assemble': [_vp, _i, _c.POINTER(_vp), _pi64, _c.POINTER(_i), _c.POINTER(_i), _i64, _vp, _i64],
    'td_columns_route': [_i, _i, _c.POINTER(_i)],
    'td_raw24_decode': [_vp, _vp, _i64, _i64, _i64, _i64, _i, _i, _pi64, _pd, _pd, _vp, _i64],
    'td_code_onsets_plan': [_i64, _c.POINTER(_i), _pi64],
    'td_code_onsets_count': [_vp, _vp, _i64, _i64, _i, _vp],
    'td_code_onsets_fill': [_vp, _vp, _i64, _i64, _i, _vp, _i64, _vp, _vp],
    'td_mlp_train': _MLP + _FIT + _EPOCHS + [_f, _f, _f] + _SEED_STATS,
    'td_mlp_grad': _MLP + _FIT + _GRAD,
    'td_mlp_train_loss': _MLP + _FIT + _EPOCHS + [_f, _f, _f] + _SEED_STATS + [_i],
    'td_mlp_grad_loss': _MLP + _FIT + _GRAD + [_i],
    'td_mlp_forward': _MLP + _FORWARD,
    'td_mlpc_train': _MLPC + _FIT + _EPOCHS + [_d, _d, _d, _d, _i64, _i] + _SEED_STATS,
    'td_mlpc_grad': _MLPC + _FIT + _GRAD,
    'td_mlpc_forward': _MLPC + _FORWARD,
    # (the shared arguments of td_mlp_train_loss, then epochs, loss, num_models, the per-model arrays, stats_dev)
    'td_dnn_train_many': _MLP + [_i] + _TARGETS + _NETWORK + [_i, _i, _i, _i] + _MANY + [_vp],
    # (the shared arguments of td_mlpc_train, then epochs, update, num_models, the per-model arrays, stats_dev)
    'td_clf_train_many': _MLPC + [_i] + _TARGETS + _NETWORK + [_i, _i, _i, _i] + _MANY_ADAM + [_vp],
}
_RESTYPE = {'td_last_error': _c.c_char_p}

_lib = None


def header_symbols():
  """Every function name the C header declares."""
  with open(HEADER) as f:
    text = f.read()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  return sorted(set(re.findall(r'\b(td_[a-z0-9_]+)\s*\(', text)))


def load():
  """Loads the shared library (no GPU needed) and sets the prototypes."""
  global _lib
  if _lib is not None:
    return _lib
  try:
    # PyTorch-ROCm ships its own libamdhip64; it must be the one HIP runtime of the
    # process.  Loading ours first (it resolves libamdhip64 from /opt/rocm) and torch
    # afterwards leaves torch without devices ("No HIP GPUs are available").
    import torch  # noqa: F401
  except ImportError:
    pass
  if not os.path.exists(LIB_PATH):
    raise HotPathUnavailable(
        'HIP extension %s is missing: build it with '
        '`python -m telluride_decoding_amd.build` (hipcc, gfx950). '
        'There is no CPU fallback for the hot path.' % LIB_PATH)
  lib = ctypes.CDLL(LIB_PATH)
  for name, args in SIGNATURES.items():
    fn = getattr(lib, name)   # AttributeError if the .so lacks a declared symbol
    fn.argtypes = args
    fn.restype = _RESTYPE.get(name, _i)
  _lib = lib
  return lib


def check(handle_ptr, status):
  if status == TD_OK:
    return
  lib = load()
  msg = lib.td_last_error(handle_ptr)
  msg = msg.decode() if msg else 'status %d' % status
  if status == TD_ERR_INVALID:
    raise ValueError(msg)
  if status == TD_ERR_SINGULAR:
    raise np.linalg.LinAlgError(msg)
  if status == TD_ERR_NOMEM:
    raise MemoryError(msg)
  if status == TD_ERR_HIP and handle_ptr is None:
    raise HotPathUnavailable(msg)
  raise HotPathError(msg)


def i64_array(values):
  arr = np.ascontiguousarray(values, dtype=np.int64)
  return arr, arr.ctypes.data_as(_pi64)


def f64_array(values):
  arr = np.ascontiguousarray(values, dtype=np.float64)
  return arr, arr.ctypes.data_as(_pd)
