"""The seven online push wrappers of device.py against the parent commit's own words and bytes.

The wrappers -- online_push, cca_online_push, dnn_online_push, frontend_push, audio_online_push, online_fit_push,
online_calib_push -- state their shared pieces once (the row block of a push, the state stride, the dtype-and-device
loop, the spare-element outputs, the body of online_push / dnn_online_push).  Two things pin that nothing a caller
sees moved:

REFUSALS: every argument a wrapper refuses in Python, before any launch -- the exception's type and its whole message,
compared with ==.  Two rows give two bad arguments at once: which one is reported first is part of the contract.

DIGESTS: tests/test_gpu_online_pinned.py pins every output byte of four of the wrappers; frontend_push,
audio_online_push and online_fit_push get the same here: a fixed-seed recording (np.random.RandomState) through
pushes of 1 row (the row-stride fallback), 7 rows and a flush (without rows; for the fit also one that carries rows),
the rows a slice whose row and session strides are wider than a row and a block, 1 and 3 sessions, 1 and 3 channels;
the SHA-256 of every output and of the state bytes.

PARENT_REFUSALS and PARENT_SHA256 were produced once by this file's own refusal_of and run_case with the package of
the parent commit 28f8590 ("Share the online push kernels' common blocks in online_common.h") on the path, on the
MI355X.  They are never to be produced from the code under test."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, N = 2, 4                                  # the sessions and rows of a refused call
SOS = np.array([[0.2, 0.4, 0.2, 1.0, -0.3, 0.1], [0.5, -1.0, 0.5, 1.0, -0.5, 0.25]], np.float64)
ZI = np.array([[0.3, -0.1], [-0.5, 0.2]], np.float64)


def _f32(*shape):
  import torch
  return torch.zeros(shape, dtype=torch.float32, device='cuda')


def _f64(*shape):
  import torch
  return torch.zeros(shape, dtype=torch.float64, device='cuda')


def _u8(*shape):
  import torch
  return torch.zeros(shape, dtype=torch.uint8, device='cuda')


def _good(dev, wrapper):
  """The arguments of a call of `wrapper` that it accepts: S sessions, N rows, 3 channels."""
  from telluride_decoding_amd import online
  if wrapper == 'online_push':        # k = 3 lags x 3 channels
    return dict(eeg=_f32(S, N, 3), env=_f32(S, N, 2), w=_f32(1, 9), b=_f32(1), corr=_f64(S, 2, 3),
                state=_u8(S, dev.online_state_bytes(3, 1, 1, 5)), frames_before=0, pre=1, post=1, width=5, hop=2)
  if wrapper == 'dnn_online_push':    # hidden [4] on 9 inputs: 9 * 4 + 4 + 4 + 1 = 45 parameters
    return dict(eeg=_f32(S, N, 3), env=_f32(S, N, 2), params=_f32(1, 45), hidden=[4], corr=_f64(S, 2, 3),
                state=_u8(S, dev.online_state_bytes(3, 1, 1, 5)), frames_before=0, pre=1, post=1, width=5, hop=2)
  if wrapper == 'cca_online_push':    # k1 = 3 x 3, k2 = 2 lags x 2 features, 2 dims
    return dict(eeg=_f32(S, N, 3), feat1=_f32(S, N, 2), feat2=_f32(S, N, 2), mean_x=_f32(1, 9), rot_x=_f32(1, 9, 2),
                mean_y=_f32(1, 4), rot_y=_f32(1, 4, 2), corr=_f64(S, 2, 3, 2),
                state=_u8(S, dev.cca_online_state_bytes(3, 1, 1, 2, 0, 1, 5)), frames_before=0, pre1=1, post1=1,
                pre2=0, post2=1, width=5, hop=2)
  if wrapper == 'frontend_push':
    return dict(x=_f32(S, N, 3), sos=None, stage_split=0, zi=None, fs_in=100.0, fs_out=100.0, groups=(), select=None,
                mean=_f64(1), std=_f64(1) + 1.0, state=_u8(S, dev.frontend_state_bytes(3, 0)), rows_before=0)
  if wrapper == 'audio_online_push':
    tail = online.audio_tail_rows(8.0, 4.0, 2.0)
    return dict(x=_f32(S, N, 3), fs_in=8.0, fs_out=4.0, window=2.0, exponent=1.0,
                state=_u8(S, dev.audio_online_state_bytes(3, tail)), live=0, rows_before=0)
  if wrapper == 'online_fit_push':
    return dict(eeg=_f32(S, N, 3), target=_f32(S, N, 2), state=_u8(S, dev.online_fit_state_bytes(3, 1, 1, 2)),
                frames_before=0, pushes_before=0, pre=1, post=1)
  assert wrapper == 'online_calib_push'
  return dict(eeg=_f32(S, N, 3), env=_f32(S, N, 2), w=_f32(1, 9), b=_f32(1),
              state=_u8(S, dev.online_calib_state_bytes(3, 1, 1)), frames_before=0, pre=1, post=1, width=5)


def _wide(t):
  """t's values as every second column of a tensor twice as wide: a column stride of 2."""
  import torch
  return torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)[..., ::2]


# (wrapper, what is wrong, {argument: a function of the good call's arguments that gives the bad value})
REFUSALS = [
    ('online_push', 'reduction', dict(reduction=lambda a: 'second')),
    ('online_push', 'decoder', dict(decoder=lambda a: 'ssd')),
    ('online_push', 'weights-not-lags', dict(w=lambda a: _f32(1, 10))),
    ('online_push', 'eeg-shape', dict(eeg=lambda a: _f32(S, N, 4))),
    ('online_push', 'env-missing', dict(env=lambda a: None)),
    ('online_push', 'eeg-float64', dict(eeg=lambda a: a['eeg'].double())),
    ('online_push', 'env-cpu', dict(env=lambda a: a['env'].cpu())),
    ('online_push', 'state-float32', dict(state=lambda a: a['state'].float())),
    ('online_push', 'columns', dict(eeg=lambda a: _wide(a['eeg']))),
    ('online_push', 'model-rows', dict(w=lambda a: _f32(3, 9), b=lambda a: _f32(3))),
    ('online_push', 'corr-shape', dict(corr=lambda a: _f64(S, 3))),
    ('online_push', 'lda-shape', dict(reduction=lambda a: 'lda', lda=lambda a: _f64(S, 2))),
    ('online_push', 'two-reduction-then-decoder', dict(reduction=lambda a: 'all', decoder=lambda a: 'ssd')),
    ('online_push', 'two-dtype-then-corr', dict(env=lambda a: a['env'].double(), corr=lambda a: _f64(S, 3))),
    ('dnn_online_push', 'reduction', dict(reduction=lambda a: 'second')),
    ('dnn_online_push', 'decoder', dict(decoder=lambda a: 'ssd')),
    ('dnn_online_push', 'parameter-count', dict(params=lambda a: _f32(1, 44))),
    ('dnn_online_push', 'model-rows', dict(params=lambda a: _f32(3, 45))),
    ('dnn_online_push', 'eeg-shape', dict(eeg=lambda a: _f32(S, N, 4))),
    ('dnn_online_push', 'eeg-float64', dict(eeg=lambda a: a['eeg'].double())),
    ('dnn_online_push', 'params-cpu', dict(params=lambda a: a['params'].cpu())),
    ('dnn_online_push', 'columns', dict(env=lambda a: _wide(a['env']))),
    ('dnn_online_push', 'corr-shape', dict(corr=lambda a: _f64(S, 2, 4))),
    ('dnn_online_push', 'lda-shape', dict(reduction=lambda a: 'lda', lda=lambda a: _f64(1, 3))),
    ('cca_online_push', 'reduction', dict(reduction=lambda a: 'all')),
    ('cca_online_push', 'decoder', dict(decoder=lambda a: 'ssd')),
    ('cca_online_push', 'model-dims', dict(mean_x=lambda a: _f32(9))),
    ('cca_online_push', 'rotation-not-lags', dict(rot_x=lambda a: _f32(1, 10, 2), mean_x=lambda a: _f32(1, 10))),
    ('cca_online_push', 'model-rows', dict(mean_x=lambda a: _f32(3, 9), rot_x=lambda a: _f32(3, 9, 2),
                                           mean_y=lambda a: _f32(3, 4), rot_y=lambda a: _f32(3, 4, 2))),
    ('cca_online_push', 'feature-shape', dict(feat2=lambda a: _f32(S, N, 3))),
    ('cca_online_push', 'feat1-float64', dict(feat1=lambda a: a['feat1'].double())),
    ('cca_online_push', 'rot_y-cpu', dict(rot_y=lambda a: a['rot_y'].cpu())),
    ('cca_online_push', 'columns', dict(feat1=lambda a: _wide(a['feat1']))),
    ('cca_online_push', 'corr-shape', dict(corr=lambda a: _f64(S, 2, 3))),
    ('cca_online_push', 'lda-shape', dict(reduction=lambda a: 'lda', lda=lambda a: _f64(S, 3))),
    ('frontend_push', 'x-sessions', dict(x=lambda a: _f32(3, N, 3))),
    ('frontend_push', 'x-int32', dict(x=lambda a: a['x'].int())),
    ('frontend_push', 'x-cpu', dict(x=lambda a: a['x'].cpu())),
    ('frontend_push', 'columns', dict(x=lambda a: _wide(a['x']))),
    ('frontend_push', 'flush-without-c', dict(x=lambda a: None, flush=lambda a: True)),
    ('frontend_push', 'mean-float32', dict(mean=lambda a: a['mean'].float())),
    ('frontend_push', 'state-cpu', dict(state=lambda a: a['state'].cpu())),
    ('frontend_push', 'mean-count', dict(mean=lambda a: _f64(3), std=lambda a: _f64(3))),
    ('frontend_push', 'nothing-wanted', dict(want32=lambda a: False)),
    ('audio_online_push', 'x-sessions', dict(x=lambda a: _f32(3, N, 3))),
    ('audio_online_push', 'x-int32', dict(x=lambda a: a['x'].int())),
    ('audio_online_push', 'x-cpu', dict(x=lambda a: a['x'].cpu())),
    ('audio_online_push', 'columns', dict(x=lambda a: _wide(a['x']))),
    ('audio_online_push', 'flush-without-c', dict(x=lambda a: None, flush=lambda a: True)),
    ('audio_online_push', 'state-float32', dict(state=lambda a: a['state'].float())),
    ('audio_online_push', 'nothing-wanted', dict(want32=lambda a: False)),
    ('online_fit_push', 'state-1d', dict(state=lambda a: a['state'].reshape(-1))),
    ('online_fit_push', 'state-float32', dict(state=lambda a: a['state'].float())),
    ('online_fit_push', 'target-rows', dict(target=lambda a: _f32(S, N + 1, 2))),
    ('online_fit_push', 'target-missing', dict(target=lambda a: None)),
    ('online_fit_push', 'eeg-float64', dict(eeg=lambda a: a['eeg'].double())),
    ('online_fit_push', 'target-cpu', dict(target=lambda a: a['target'].cpu())),
    ('online_fit_push', 'columns', dict(target=lambda a: _wide(a['target']))),
    ('online_fit_push', 'flush-without-c-d', dict(eeg=lambda a: None, target=lambda a: None, flush=lambda a: True,
                                                  c=lambda a: 3)),
    ('online_calib_push', 'state-1d', dict(state=lambda a: a['state'].reshape(-1))),
    ('online_calib_push', 'state-float32', dict(state=lambda a: a['state'].float())),
    ('online_calib_push', 'env-shape', dict(env=lambda a: _f32(S, N, 3))),
    ('online_calib_push', 'eeg-float64', dict(eeg=lambda a: a['eeg'].double())),
    ('online_calib_push', 'w-cpu', dict(w=lambda a: a['w'].cpu())),
    ('online_calib_push', 'columns', dict(eeg=lambda a: _wide(a['eeg']))),
    ('online_calib_push', 'model-rows', dict(w=lambda a: _f32(3, 9), b=lambda a: _f32(3))),
    ('online_calib_push', 'weights-not-lags', dict(w=lambda a: _f32(1, 10))),
    ('online_calib_push', 'flush-without-c', dict(eeg=lambda a: None, env=lambda a: None, flush=lambda a: True)),
]
REFUSAL_IDS = ['%s-%s' % (r[0], r[1]) for r in REFUSALS]

# what the parent commit raised; its messages name the device as
PARENT_DEVICE = 'cuda:0'
# {wrapper-what: (exception type, message)}
PARENT_REFUSALS = {
 'online_push-reduction': ('ValueError', "online_push: reduction 'second' (one of first, mean, mean-squared, lda)"),
 'online_push-decoder': ('ValueError', "online_push: unknown decoder 'ssd'"),
 'online_push-weights-not-lags': ('ValueError', 'online_push: 10 weights for 3 lags'),
 'online_push-eeg-shape': ('ValueError',
                           'online_push: eeg of (2, 4, 4) and env of (2, 4, 2) for 2 sessions of 3 channels'),
 'online_push-env-missing': ('ValueError',
                             'online_push: eeg of (2, 4, 3) and env of None for 2 sessions of 3 channels'),
 'online_push-eeg-float64': ('TypeError',
                             'online_push: eeg must be a torch.float32 tensor on cuda:0, not torch.float64 on '
                             'cuda:0'),
 'online_push-env-cpu': ('TypeError',
                         'online_push: env must be a torch.float32 tensor on cuda:0, not torch.float32 on cpu'),
 'online_push-state-float32': ('TypeError',
                               'online_push: state must be a torch.uint8 tensor on cuda:0, not torch.float32 on '
                               'cuda:0'),
 'online_push-columns': ('ValueError', 'online_push: the columns of eeg and env must be contiguous'),
 'online_push-model-rows': ('ValueError', 'online_push: 3 models and 3 biases for 2 sessions'),
 'online_push-corr-shape': ('ValueError', 'online_push: corr must be [2, 2, 3] and lda [2, 3]'),
 'online_push-lda-shape': ('ValueError', 'online_push: corr must be [2, 2, 3] and lda [2, 3]'),
 'online_push-two-reduction-then-decoder': ('ValueError',
                                            "online_push: reduction 'all' (one of first, mean, mean-squared, lda)"),
 'online_push-two-dtype-then-corr': ('TypeError',
                                     'online_push: env must be a torch.float32 tensor on cuda:0, not torch.float64 '
                                     'on cuda:0'),
 'dnn_online_push-reduction': ('ValueError',
                               "dnn_online_push: reduction 'second' (one of first, mean, mean-squared, lda)"),
 'dnn_online_push-decoder': ('ValueError', "dnn_online_push: unknown decoder 'ssd'"),
 'dnn_online_push-parameter-count': ('ValueError', 'dnn_online_push: 44 parameters for hidden layers [4] on 3 lags'),
 'dnn_online_push-model-rows': ('ValueError', 'dnn_online_push: params of (3, 45) for 2 sessions ([S or 1, P])'),
 'dnn_online_push-eeg-shape': ('ValueError',
                               'dnn_online_push: eeg of (2, 4, 4) and env of (2, 4, 2) for 2 sessions of 3 channels'),
 'dnn_online_push-eeg-float64': ('TypeError',
                                 'dnn_online_push: eeg must be a torch.float32 tensor on cuda:0, not torch.float64 '
                                 'on cuda:0'),
 'dnn_online_push-params-cpu': ('TypeError',
                                'dnn_online_push: params must be a torch.float32 tensor on cuda:0, not torch.float32 '
                                'on cpu'),
 'dnn_online_push-columns': ('ValueError', 'dnn_online_push: the columns of eeg and env must be contiguous'),
 'dnn_online_push-corr-shape': ('ValueError', 'dnn_online_push: corr must be [2, 2, 3] and lda [2, 3]'),
 'dnn_online_push-lda-shape': ('ValueError', 'dnn_online_push: corr must be [2, 2, 3] and lda [2, 3]'),
 'cca_online_push-reduction': ('ValueError',
                               "cca_online_push: reduction 'all' (one of first, second, mean, mean-squared, lda)"),
 'cca_online_push-decoder': ('ValueError', "cca_online_push: unknown decoder 'ssd'"),
 'cca_online_push-model-dims': ('ValueError', 'cca_online_push: the means are [M, k] and the rotations [M, k, dims]'),
 'cca_online_push-rotation-not-lags': ('ValueError',
                                       'cca_online_push: rotations of (1, 10, 2) and (1, 4, 2) with means of (1, 10) '
                                       'and (1, 4) for 3 + 2 lags and 2 sessions'),
 'cca_online_push-model-rows': ('ValueError',
                                'cca_online_push: rotations of (3, 9, 2) and (3, 4, 2) with means of (3, 9) and (3, '
                                '4) for 3 + 2 lags and 2 sessions'),
 'cca_online_push-feature-shape': ('ValueError',
                                   'cca_online_push: eeg of (2, 4, 3) and features of (2, 4, 2) and (2, 4, 3) for 2 '
                                   'sessions of 3 channels and 2 features'),
 'cca_online_push-feat1-float64': ('TypeError',
                                   'cca_online_push: feat1 must be a torch.float32 tensor on cuda:0, not '
                                   'torch.float64 on cuda:0'),
 'cca_online_push-rot_y-cpu': ('TypeError',
                               'cca_online_push: rot_y must be a torch.float32 tensor on cuda:0, not torch.float32 '
                               'on cpu'),
 'cca_online_push-columns': ('ValueError', 'cca_online_push: the columns of eeg and the features must be contiguous'),
 'cca_online_push-corr-shape': ('ValueError', 'cca_online_push: corr must be [2, 2, 3, 2] and lda [2, 4]'),
 'cca_online_push-lda-shape': ('ValueError', 'cca_online_push: corr must be [2, 2, 3, 2] and lda [2, 4]'),
 'frontend_push-x-sessions': ('ValueError', 'frontend_push: x of (3, 4, 3) for 2 sessions'),
 'frontend_push-x-int32': ('TypeError',
                           'frontend_push: x must be a float32 or float64 tensor on cuda:0, not torch.int32 on '
                           'cuda:0'),
 'frontend_push-x-cpu': ('TypeError',
                         'frontend_push: x must be a float32 or float64 tensor on cuda:0, not torch.float32 on cpu'),
 'frontend_push-columns': ('ValueError', 'frontend_push: the columns of x must be contiguous'),
 'frontend_push-flush-without-c': ('ValueError', 'frontend_push: a flush without rows needs the channel count c'),
 'frontend_push-mean-float32': ('TypeError',
                                'frontend_push: mean must be a torch.float64 tensor on cuda:0, not torch.float32 on '
                                'cuda:0'),
 'frontend_push-state-cpu': ('TypeError',
                             'frontend_push: state must be a torch.uint8 tensor on cuda:0, not torch.uint8 on cpu'),
 'frontend_push-mean-count': ('ValueError', 'frontend_push: 3 means and 3 stds for 2 sessions'),
 'frontend_push-nothing-wanted': ('ValueError',
                                  'frontend_push: neither the float32 nor the float64 output is wanted'),
 'audio_online_push-x-sessions': ('ValueError', 'audio_online_push: x of (3, 4, 3) for 2 sessions'),
 'audio_online_push-x-int32': ('TypeError',
                               'audio_online_push: x must be an int16, float32 or float64 tensor on cuda:0, not '
                               'torch.int32 on cuda:0'),
 'audio_online_push-x-cpu': ('TypeError',
                             'audio_online_push: x must be an int16, float32 or float64 tensor on cuda:0, not '
                             'torch.float32 on cpu'),
 'audio_online_push-columns': ('ValueError', 'audio_online_push: the columns of x must be contiguous'),
 'audio_online_push-flush-without-c': ('ValueError',
                                       'audio_online_push: a flush without rows needs the channel count c'),
 'audio_online_push-state-float32': ('TypeError',
                                     'audio_online_push: state must be a uint8 tensor on cuda:0, not torch.float32 '
                                     'on cuda:0'),
 'audio_online_push-nothing-wanted': ('ValueError',
                                      'audio_online_push: neither the float32 nor the float64 output is wanted'),
 'online_fit_push-state-1d': ('TypeError',
                              'online_fit_push: state must be a [S, bytes] uint8 tensor on cuda:0, not (2048,) '
                              'torch.uint8 on cuda:0'),
 'online_fit_push-state-float32': ('TypeError',
                                   'online_fit_push: state must be a [S, bytes] uint8 tensor on cuda:0, not (2, '
                                   '1024) torch.float32 on cuda:0'),
 'online_fit_push-target-rows': ('ValueError',
                                 'online_fit_push: eeg of (2, 4, 3) and target of (2, 5, 2) for 2 sessions'),
 'online_fit_push-target-missing': ('ValueError',
                                    'online_fit_push: eeg of (2, 4, 3) and target of None for 2 sessions'),
 'online_fit_push-eeg-float64': ('TypeError',
                                 'online_fit_push: eeg must be a float32 tensor on cuda:0, not torch.float64 on '
                                 'cuda:0'),
 'online_fit_push-target-cpu': ('TypeError',
                                'online_fit_push: target must be a float32 tensor on cuda:0, not torch.float32 on '
                                'cpu'),
 'online_fit_push-columns': ('ValueError', 'online_fit_push: the columns of eeg and target must be contiguous'),
 'online_fit_push-flush-without-c-d': ('ValueError',
                                       'online_fit_push: a flush without rows needs the channel count c and the '
                                       'output count d'),
 'online_calib_push-state-1d': ('TypeError',
                                'online_calib_push: state must be a [S, bytes] uint8 tensor on cuda:0, not (528,) '
                                'torch.uint8 on cuda:0'),
 'online_calib_push-state-float32': ('TypeError',
                                     'online_calib_push: state must be a [S, bytes] uint8 tensor on cuda:0, not (2, '
                                     '264) torch.float32 on cuda:0'),
 'online_calib_push-env-shape': ('ValueError',
                                 'online_calib_push: eeg of (2, 4, 3) and env of (2, 4, 3) for 2 sessions'),
 'online_calib_push-eeg-float64': ('TypeError',
                                   'online_calib_push: eeg must be a float32 tensor on cuda:0, not torch.float64 on '
                                   'cuda:0'),
 'online_calib_push-w-cpu': ('TypeError',
                             'online_calib_push: w must be a float32 tensor on cuda:0, not torch.float32 on cpu'),
 'online_calib_push-columns': ('ValueError', 'online_calib_push: the columns of eeg and env must be contiguous'),
 'online_calib_push-model-rows': ('ValueError', 'online_calib_push: (3, 9) weights and 3 biases for 2 sessions'),
 'online_calib_push-weights-not-lags': ('ValueError', 'online_calib_push: 10 weights for 3 lags of 3 channels'),
 'online_calib_push-flush-without-c': ('ValueError',
                                       'online_calib_push: a flush without rows needs the channel count c'),
}


def refusal_of(dev, wrapper, changes):
  """(exception type's name, message) of the call of `wrapper` with `changes` made to a good call's arguments."""
  args = _good(dev, wrapper)
  bad = dict((name, make(args)) for name, make in changes.items())
  args.update(bad)
  try:
    getattr(dev, wrapper)(**args)
  except Exception as e:          # (whatever it is: the table says what it has to be)
    return type(e).__name__, str(e)
  return None, None


# -- the bytes of the three wrappers tests/test_gpu_online_pinned.py does not cover
# pushes of a recording, then the rows its flush carries (0: a flush without rows)
PUSHES = (1, 7)

# (sessions, channels, dtype, sections, re-reference and select, per-session mean / std, fs_out of fs_in = 100)
FRONTEND = [
    (1, 1, 'float32', 0, False, False, 100.0),
    (3, 3, 'float64', 2, True, True, 64.0),
    (3, 3, 'float32', 1, False, False, 64.0),
    (1, 3, 'float64', 0, True, False, 100.0),
    (3, 1, 'float32', 2, False, True, 100.0),
]
# (sessions, channels, dtype, want64)
AUDIO = [
    (1, 1, 'int16', False),
    (3, 3, 'float32', True),
    (3, 1, 'int16', True),
    (1, 3, 'float32', False),
]
# (sessions, channels, outputs, pre, post, rows the flush carries, forgetting)
FIT = [
    (1, 1, 1, 1, 2, 3, 1.0),
    (3, 3, 2, 1, 2, 3, 0.9),
    (3, 1, 2, 0, 0, 0, 1.0),
    (1, 3, 1, 2, 1, 0, 0.9),
]


def _name(case):
  return '-'.join(str(v) for v in case)


CASES = ([('frontend-' + _name(c), 'frontend', c) for c in FRONTEND] +
         [('audio-' + _name(c), 'audio', c) for c in AUDIO] + [('fit-' + _name(c), 'fit', c) for c in FIT])

# the parent commit's outputs: {case: {output: SHA-256}}
PARENT_SHA256 = {
    'frontend-1-1-float32-0-False-False-100.0': {
        'out32': 'b7e5e9103f11dc1122171cee0f6ec7a5e13eb60b15d29d46e23f47f4255209b0',
        'out64': '62b4f1f76c7300f61126f79c8b421bdf51f1765684a887ed2cea24f904695d5d',
        'state': '8ae2010fbf0a1148c7a045f64143d9bf5d445a8038f33345bbf6f9218bf0e77a',
    },
    'frontend-3-3-float64-2-True-True-64.0': {
        'out32': '429cd4a0432bcfb288133f08757368f07f6de2ed4694e104268eebf407160b4f',
        'out64': '4fbdd7df535d2920bb4c268f17d88326248a7a02d955616bc6984b1695613bca',
        'state': '15a377ad912bc9b9425c44379e9cb8019e33848a6bb9b2375accbab3e06e6e93',
    },
    'frontend-3-3-float32-1-False-False-64.0': {
        'out32': '381baa64bcfc483da1b0b45ef65abc933a96eaeea7f8092d8af15b445e3583de',
        'out64': '9fbbda2adb9f7e3cfdb24e434af56e2cd956f1f006fdf0d85a6ca1aaa2033d99',
        'state': '6d195538112adb21d00a4ed31d2cb88f866746c568a4d08150f8da41682725d2',
    },
    'frontend-1-3-float64-0-True-False-100.0': {
        'out32': '5a8768933d4bb85182714e811c2d7df72a7537a51efb81729b9746cd0cea8682',
        'out64': '6d01eeecb84ff649120624cdad00fb20cde0fc33716548b05affb65afce1ce82',
        'state': 'd46d05a6119ed91a2fc720384648dd311cf25753ab1388918475f4d6777155a9',
    },
    'frontend-3-1-float32-2-False-True-100.0': {
        'out32': '27e6970cbfdbe8f37e39f36d31aa90f945e3eb89ed9909b1c97621233353fbb6',
        'out64': '814bd24b27bbdae94e30f92d918daede8a3b21ab6d99ce5a4fa2cf26598ec319',
        'state': 'f89ec4ffd8a53ce3c5ae5cb7ef8bb65a4df589554418de86fe7160d68dd524cd',
    },
    'audio-1-1-int16-False': {
        'out32': 'abd52491099b52a365efd39486e60c9ba2c47535b55496c38b675539f3ecac7f',
        'out64': 'e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855',
        'windows': '4a3d49ca53e31c070a8690732185b539e1e9cd893714acc5380595943255044f',
        'state': '4513c93833db1a38e7ddf65af83a6222755195b284ba8cd53350c1c364ebf913',
    },
    'audio-3-3-float32-True': {
        'out32': '9d276f5fafecf78ba297510664399791b47e01efe4cb813ffba2f8da4fc4e214',
        'out64': 'fc2abf6321af0bc47642cfb3caccb9116b842883ab52aea3657f89a5b140fd50',
        'windows': '4a3d49ca53e31c070a8690732185b539e1e9cd893714acc5380595943255044f',
        'state': 'c2b3a77f1bdcf48b084b5fe5231a60903d87b3cb70844faf888ae811fafb2e96',
    },
    'audio-3-1-int16-True': {
        'out32': 'c22f896f498590cb138358371014fef8c1bbad8d424cace3a7e57c1667c1ab7d',
        'out64': '2b57248ae3d7124b23f220f20ad3300df67f91ac0744692c58438dcc372ce411',
        'windows': '4a3d49ca53e31c070a8690732185b539e1e9cd893714acc5380595943255044f',
        'state': '61bf816d36812b453aa08244c412995d9ddd87c6d9911d957cdfd375237d5891',
    },
    'audio-1-3-float32-False': {
        'out32': 'cff430af8454589323ed23e516b81d0abf06687dc6e5822e105ed7e9ceef8e97',
        'out64': 'e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855',
        'windows': '4a3d49ca53e31c070a8690732185b539e1e9cd893714acc5380595943255044f',
        'state': 'a801e8f0cc5bb0bdd559e9181b0f53fdaa355118a67f09c3f55e6460338c40b5',
    },
    'fit-1-1-1-1-2-3-1.0': {'state': '657ccb88d51f57a3769cefccaeb8ca886161824d489950efceb6df29ecec9315'},
    'fit-3-3-2-1-2-3-0.9': {'state': '188c047e40f71fd282dccca21aa3cddbb8507ffe1d5d6920c43d4b0f29deb61a'},
    'fit-3-1-2-0-0-0-1.0': {'state': '1a7db2ca394582a23bee52ef0fae2a6d0b66eeb0c93b83cfb0e3ad13ebd3bc79'},
    'fit-1-3-1-2-1-0-0.9': {'state': '3e8f3353f137ab9f3f3d8f00c7882465627e700b6ba0f4b49aa775551bada9ca'},
}


class _Recording(object):
  """Seeded rows on the device, handed out push by push as slices with a row stride of columns + 3 and a session
  stride of two rows more than the recording."""

  def __init__(self, rs, sessions, frames, columns, dtype='float32'):
    import torch
    values = rs.standard_normal((sessions, frames + 2, columns + 3))
    values = np.rint(2000.0 * values).astype(np.int16) if dtype == 'int16' else values.astype(dtype)
    self.at, self.columns = 0, columns
    self.full = torch.from_numpy(values).to('cuda')

  def take(self, n):
    out = self.full[:, self.at:self.at + n, :self.columns]
    self.at += n
    return out


class _Hashes(object):
  def __init__(self, names):
    self.h = dict((n, hashlib.sha256()) for n in names)

  def add(self, name, tensor):
    self.h[name].update(tensor.cpu().numpy().tobytes())

  def digests(self):
    return dict((n, h.hexdigest()) for n, h in self.h.items())


def _steps(last):
  return [(n, False) for n in PUSHES] + [(last, True)]


def _run_frontend(dev, case, rs):
  import torch
  sessions, c, dtype, sections, reref, own_stats, fs_out = case
  rec = _Recording(rs, sessions, sum(PUSHES), c, dtype)
  groups = [([0], list(range(1, c)) or [0])] if reref else []
  select = ([c - 1, 0] if c > 1 else [0]) if reref else None
  stats = rs.standard_normal((sessions if own_stats else 1, 2))
  mean = torch.from_numpy(stats[:, 0].copy()).to('cuda')
  std = torch.from_numpy(1.0 + np.abs(stats[:, 1])).to('cuda')
  state = _u8(sessions, dev.frontend_state_bytes(c, sections))
  out = _Hashes(('out32', 'out64', 'state'))
  pushed = 0
  for n, flush in _steps(0):
    r = dev.frontend_push(rec.take(n) if n else None, SOS[:sections] if sections else None, min(1, sections),
                          ZI[:sections] if sections else None, 100.0, fs_out, groups, select, mean, std, state,
                          pushed, c=c, flush=flush, want64=True)
    pushed += n
    out.add('out32', r.out32)
    out.add('out64', r.out64)
  assert r.plan.frames_after == int(np.round(pushed / 100.0 * fs_out))      # (flushed: every frame is out)
  out.add('state', state)
  return out.digests()


def _run_audio(dev, case, rs):
  from telluride_decoding_amd import online
  sessions, c, dtype, want64 = case
  fs_in, fs_out, window = 8.0, 4.0, 2.0
  rec = _Recording(rs, sessions, sum(PUSHES), c, dtype)
  state = _u8(sessions, dev.audio_online_state_bytes(c, online.audio_tail_rows(fs_in, fs_out, window)))
  out = _Hashes(('out32', 'out64', 'windows', 'state'))
  pushed = live = 0
  for n, flush in _steps(0):
    r = dev.audio_online_push(rec.take(n) if n else None, fs_in, fs_out, window, 0.6, state, live, pushed, c=c,
                              flush=flush, want64=want64, windows=True)
    pushed, live = pushed + n, r.live
    out.add('out32', r.out32)
    if want64:
      out.add('out64', r.out64)
    out.add('windows', r.windows)
  assert r.plan.frames_after == 4 and live == 0                     # (8 rows at 8 -> 4 Hz; two pushes with rows)
  out.add('state', state)
  return out.digests()


def _run_fit(dev, case, rs):
  sessions, c, d, pre, post, last, forget = case
  eeg = _Recording(rs, sessions, sum(PUSHES) + last, c)
  target = _Recording(rs, sessions, sum(PUSHES) + last, d)
  state = _u8(sessions, dev.online_fit_state_bytes(c, pre, post, d))
  out = _Hashes(('state',))
  pushed = pushes = 0
  for n, flush in _steps(last):
    pushed = dev.online_fit_push(eeg.take(n) if n else None, target.take(n) if n else None, state, pushed, pushes,
                                 pre, post, c=c, d=d, flush=flush, forget=forget)
    pushes += 1 if n else 0
    out.add('state', state)                                                 # (after every push)
  assert pushed == sum(PUSHES) + last
  return out.digests()


def run_case(dev, name, kind, case):
  """{output: SHA-256} of one case; the seed is the case's place in CASES."""
  rs = np.random.RandomState(20271 + [c[0] for c in CASES].index(name))
  return {'frontend': _run_frontend, 'audio': _run_audio, 'fit': _run_fit}[kind](dev, case, rs)


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def test_the_device_is_named_as_the_parent_named_it(dev):
  assert str(dev.default_handle().device) == PARENT_DEVICE


@pytest.mark.parametrize('wrapper,what,changes', REFUSALS, ids=REFUSAL_IDS)
def test_every_refusal_is_the_parents_word_for_word(dev, wrapper, what, changes):
  got = refusal_of(dev, wrapper, changes)
  print('%s-%s: %r' % (wrapper, what, got))
  assert got == PARENT_REFUSALS['%s-%s' % (wrapper, what)]


@pytest.mark.parametrize('name,kind,case', CASES, ids=[c[0] for c in CASES])
def test_every_output_has_the_parents_bytes(dev, name, kind, case):
  got = run_case(dev, name, kind, case)
  for output in sorted(got):
    print('%s %s %s' % (name, output, got[output]))
  assert got == PARENT_SHA256[name]
