"""Host side of the device TFRecord reader: tfrecord.decode_plan (the record template, the byte mask and the payload
layout the kernel works from) on the reference's own file and on files it must turn down, and the C entry's
declaration and export."""
import os

import numpy as np

from telluride_decoding_amd import _lib
from telluride_decoding_amd import tfrecord

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, 'golden', 'meg_subj01_400.tfrecords')


def read_bytes(path):
  with open(path, 'rb') as f:
    return f.read()


def test_plan_of_the_reference_file():
  plan = tfrecord.decode_plan(GOLDEN_FILE)
  assert plan['stride'] == 650 and plan['frames'] == 400
  assert sorted(offset for _, offset, _ in plan['layout']) == [33, 54]
  assert {name for name, _, _ in plan['layout']} == set(tfrecord.read_file(GOLDEN_FILE))
  mask = np.frombuffer(plan['mask'], np.uint8)
  template = np.frombuffer(plan['template'], np.uint8)
  assert mask.shape == template.shape == (650,) and set(mask.tolist()) == {0, 1}
  free = np.zeros(650, bool)
  free[-4:] = True
  for _, offset, count in plan['layout']:
    assert not free[offset:offset + 4 * count].any()          # (the payloads do not overlap)
    free[offset:offset + 4 * count] = True
  assert np.array_equal(mask == 0, free)
  first = np.frombuffer(read_bytes(GOLDEN_FILE)[:650], np.uint8)
  assert not (template ^ first)[mask == 1].any()
  assert not template[mask == 0].any()
  # every record of the file keeps to the skeleton, and the layout is the one the encoder's template has
  records = np.frombuffer(read_bytes(GOLDEN_FILE), np.uint8).reshape(400, 650)
  assert np.array_equal(records[:, mask == 1], np.broadcast_to(template[mask == 1], (400, int(mask.sum()))))
  want_template, want_layout = tfrecord.record_template({name: count for name, _, count in plan['layout']})
  assert plan['template'] == want_template and plan['layout'] == want_layout


def test_plan_payload_matches_read_file():
  plan = tfrecord.decode_plan(GOLDEN_FILE)
  records = np.frombuffer(read_bytes(GOLDEN_FILE), np.uint8).reshape(400, 650)
  want = tfrecord.read_file(GOLDEN_FILE, verify=True)
  for name, offset, count in plan['layout']:
    got = np.ascontiguousarray(records[:, offset:offset + 4 * count]).view('<u4')
    assert np.array_equal(got, want[name].view(np.uint32))


def test_no_plan_for_files_that_are_not_regular(tmp_path):
  rng = np.random.default_rng(0)
  eeg = rng.standard_normal((6, 3)).astype(np.float32)
  typed = str(tmp_path / 'typed.tfrecords')
  tfrecord.write_file_typed(typed, {'eeg': eeg, 'label': np.arange(6, dtype=np.int64).reshape(6, 1)})
  assert tfrecord.decode_plan(typed) is None
  good = str(tmp_path / 'good.tfrecords')
  tfrecord.write_file(good, {'eeg': eeg})
  assert tfrecord.decode_plan(good)['frames'] == 6
  cut = str(tmp_path / 'cut.tfrecords')
  with open(cut, 'wb') as f:
    f.write(read_bytes(good)[:-1])
  assert tfrecord.decode_plan(cut) is None
  # records of two widths
  wide = str(tmp_path / 'wide.tfrecords')
  tfrecord.write_file(wide, {'eeg': rng.standard_normal((1, 4)).astype(np.float32)})
  mixed = str(tmp_path / 'mixed.tfrecords')
  with open(mixed, 'wb') as f:
    f.write(read_bytes(good) + read_bytes(wide))
  assert os.path.getsize(mixed) % tfrecord.decode_plan(good)['stride']
  assert tfrecord.decode_plan(mixed) is None
  # nothing to go by, and a first record whose length CRC is wrong
  empty = str(tmp_path / 'empty.tfrecords')
  open(empty, 'wb').close()
  assert tfrecord.decode_plan(empty) is None
  image = bytearray(read_bytes(good))
  image[9] ^= 0x10
  bad = str(tmp_path / 'lengthcrc.tfrecords')
  with open(bad, 'wb') as f:
    f.write(bytes(image))
  assert tfrecord.decode_plan(bad) is None


def test_the_entry_is_declared_bound_and_exported():
  assert 'td_tfrecord_decode' in _lib.header_symbols()
  assert 'td_tfrecord_decode' in _lib.SIGNATURES
  lib = _lib.load()
  assert lib.td_tfrecord_decode.argtypes == _lib.SIGNATURES['td_tfrecord_decode']
  with open(_lib.HEADER) as f:
    text = f.read()
  declaration = text[text.index('int td_tfrecord_decode('):]
  declaration = declaration[:declaration.index(';')]
  assert declaration.count(',') + 1 == len(_lib.SIGNATURES['td_tfrecord_decode'])


def test_data_options_keep_their_fields():
  from telluride_decoding_amd import decoding
  assert len(decoding.DecodingOptions._DEFAULTS) == 37
