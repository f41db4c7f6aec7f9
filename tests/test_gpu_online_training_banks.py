"""Host arrays into a device bank, through every training bank of the online chain (online._TrainingBank's conversion):
the same fixed-seed recording of two sessions goes through pushes of 1 and 7 rows and a flush that carries 4, once as
NumPy arrays and once as device tensors; the state bytes and moments() / sums() must be equal."""
import pytest

from tests import host_online_training as hot

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(hot.BANKS))
def test_arrays_and_tensors_give_the_same_state_bytes(name):
  import torch
  from telluride_decoding_amd import device
  assert device.gpu_available()
  spec = hot.BANKS[name]
  rows = spec.rows()
  from_arrays, from_tensors = spec.make(), spec.make()
  assert from_arrays._dev is not None and from_arrays._host is None
  counted = hot.run(from_arrays, rows)
  assert hot.run(from_tensors, rows, convert=lambda a: torch.from_numpy(a).to('cuda')) == counted
  assert counted[-1] == hot.FRAMES == getattr(from_arrays, spec.counter)
  assert from_arrays._pushes == from_tensors._pushes == 3
  assert from_arrays._dev['state'].any()
  assert torch.equal(from_arrays._dev['state'], from_tensors._dev['state'])
  for got, want in zip(spec.results(from_arrays), spec.results(from_tensors)):
    assert got.is_cuda and got.dtype == torch.float64 and torch.equal(got, want)
