"""The two online front ends before any row: OnlinePreprocessor and OnlineAudioFeatures share their push path
(online._FrontEnd), so a flush that no push came before -- the row width still unknown -- answers alike: flush() an
empty float32 [S, 0, 0], flush(want64=True) the pair want64 promises everywhere else, and the bank is flushed
afterwards.  (OnlinePreprocessor used to return the bare float32 array for want64=True, which a caller's
`out32, out64 = ...` unpacked into the two sessions of a bank of two.)"""
import numpy as np
import pytest

from tests import host_online_audio as ha
from tests import host_online_pre as hp

FRONTS = {
    'pre': (lambda online, s: online.OnlinePreprocessor(hp.make(hp.config(2, 1000, 100, 5)), num_sessions=s),
            'The front end was flushed: reset() starts the next recording.', np.zeros((4, 5), np.float32)),
    'audio': (lambda online, s: online.OnlineAudioFeatures(ha.features(16000, 64, 1), num_sessions=s),
              'The audio front end was flushed: reset() starts the next recording.', np.zeros((4, 2), np.int16)),
}


@pytest.fixture
def host_only(monkeypatch):
  """The NumPy sessions, whatever the machine has."""
  from telluride_decoding_amd import device
  monkeypatch.setattr(device, 'gpu_available', lambda: False)


@pytest.mark.parametrize('sessions', [1, 2])
@pytest.mark.parametrize('front', sorted(FRONTS))
@pytest.mark.parametrize('want64', [False, True])
def test_a_flush_before_any_row(host_only, front, sessions, want64):
  from telluride_decoding_amd import online
  make, sentence, rows = FRONTS[front]
  bank = make(online, sessions)
  out = bank.flush(want64=True) if want64 else bank.flush()
  if want64:
    assert isinstance(out, tuple) and len(out) == 2
    out, out64 = out
    assert isinstance(out64, np.ndarray) and out64.shape == (sessions, 0, 0) and out64.dtype == np.float64
  assert isinstance(out, np.ndarray) and out.shape == (sessions, 0, 0) and out.dtype == np.float32
  assert bank.flushed and bank.channels is None and (bank.rows_pushed, bank.frames_emitted) == (0, 0)
  with pytest.raises(ValueError) as refusal:
    bank.push(np.stack([rows] * sessions))
  assert str(refusal.value) == sentence
