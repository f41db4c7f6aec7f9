"""The life cycle the four training banks of the online chain share (online._TrainingBank), through every one of them
on the NumPy sessions: a flush with only some of the last rows and a push after the flush are refused in the class's
own sentence, and reset() returns the counters to fresh and the next identical run to the same bits."""
import numpy as np
import pytest

from tests import host_online_training as hot


@pytest.fixture
def host_only(monkeypatch):
  from telluride_decoding_amd import device
  monkeypatch.setattr(device, 'gpu_available', lambda: False)


def _fresh(bank, spec):
  return (bank.rows_pushed, getattr(bank, spec.counter), bank.flushed, bank._pushes) == (0, 0, False, 0)


@pytest.mark.parametrize('name', sorted(hot.BANKS))
def test_flush_takes_all_of_the_last_rows_or_none(host_only, name):
  spec = hot.BANKS[name]
  bank, rows = spec.make(), spec.rows()
  last = [r[:, 8:] for r in rows]
  for given in range(1, 2 ** len(rows) - 1):                             # some of them: neither none nor all
    some = [r if given >> i & 1 else None for i, r in enumerate(last)]
    with pytest.raises(ValueError) as refusal:
      bank.flush(*some)
    assert str(refusal.value) == spec.last_rows
  assert _fresh(bank, spec)                                              # (a refused flush leaves the bank alone)
  assert bank.flush() == 0 and bank.flushed


@pytest.mark.parametrize('name', sorted(hot.BANKS))
def test_a_flushed_bank_refuses_rows_until_reset(host_only, name):
  spec = hot.BANKS[name]
  bank, rows = spec.make(), spec.rows()
  assert hot.run(bank, rows)[-1] == hot.FRAMES
  for call in (lambda: bank.push(*[r[:, :1] for r in rows]), lambda: bank.flush(*[r[:, :1] for r in rows]),
               bank.flush):
    with pytest.raises(ValueError) as refusal:
      call()
    assert str(refusal.value) == spec.flushed
  assert (bank.rows_pushed, getattr(bank, spec.counter)) == (hot.FRAMES, hot.FRAMES)


@pytest.mark.parametrize('name', sorted(hot.BANKS))
def test_reset_starts_over_and_the_next_run_gives_the_same_bits(host_only, name):
  spec = hot.BANKS[name]
  bank, rows = spec.make(), spec.rows()
  assert _fresh(bank, spec)
  counted = hot.run(bank, rows)
  assert counted == [0, 8 - bank.delay, hot.FRAMES] and bank.delay == 1
  assert (bank.rows_pushed, bank.flushed, bank._pushes) == (hot.FRAMES, True, 3)
  first = [np.array(r) for r in spec.results(bank)]
  assert all(r.dtype == np.float64 and r.any() for r in first)
  bank.reset()
  assert _fresh(bank, spec)
  assert not any(np.asarray(r).any() for r in spec.results(bank))
  assert hot.run(bank, rows) == counted
  for got, want in zip(spec.results(bank), first):
    np.testing.assert_array_equal(got, want)
