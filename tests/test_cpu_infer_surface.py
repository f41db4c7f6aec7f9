"""The file-driven half of the reference's infer / infer_decoder surface against fixture G14 (the
reference's own signatures): what tests/test_cpu_surface.py lists as out of scope or as deviations and
DESIGN section 24 builds -- create_brain_data, get_data_for_model, load_model, main, create_dataset,
Decoder.load_decoding_model, the leading parameters of run_reduction_test / run_comparison_test, and the
flags of make_parser."""
import inspect
import json
import os

import pytest

from telluride_decoding_amd import infer
from telluride_decoding_amd import infer_decoder
from tests.surface import member_rows, module_surface

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden():
  with open(os.path.join(HERE, 'golden', 'g14_surface.json')) as fp:
    return json.load(fp)['surface']


@pytest.mark.parametrize('module, name', [
    (infer, 'create_brain_data'), (infer, 'get_data_for_model'), (infer, 'load_model'),
    (infer_decoder, 'create_dataset')])
def test_function_has_the_references_parameters(module, name):
  """Name, kind, order and default of every parameter; nothing added."""
  want = _golden()[module.__name__.rsplit('.', 1)[1]][name]
  assert module_surface(module)[name] == want


def test_main_takes_argv():
  """The reference's main(argv) is called by absl with the program's arguments; here argv defaults to None
  (sys.argv[1:]), as decoding.main's does."""
  want = _golden()['infer']['main']
  got = module_surface(infer)['main']
  assert [row[:2] for row in got] == [row[:2] for row in want] == [['argv', 'POSITIONAL_OR_KEYWORD']]
  assert inspect.signature(infer.main).parameters['argv'].default is None


def test_load_decoding_model_has_the_references_parameters():
  want = _golden()['infer_decoder']['Decoder']['members']['load_decoding_model']
  assert member_rows(infer_decoder.Decoder, 'load_decoding_model') == want
  # and save_parameters leads with the reference's, what it adds is optional
  want = _golden()['infer_decoder']['Decoder']['members']['save_parameters']
  got = member_rows(infer_decoder.Decoder, 'save_parameters')
  assert got[:len(want)] == want and all(row[2] is not None for row in got[len(want):])


@pytest.mark.parametrize('name', ['run_reduction_test', 'run_comparison_test'])
def test_sweeps_lead_with_the_references_parameters(name):
  want = _golden()['infer'][name]
  got = module_surface(infer)[name]
  assert [row[0] for row in got[:len(want)]] == [row[0] for row in want]
  assert all(row[1] == 'POSITIONAL_OR_KEYWORD' for row in got[:len(want)])
  # what follows is keyword-only
  extra = {row[0]: row for row in got[len(want):]}
  assert all(row[1] in ('KEYWORD_ONLY', 'VAR_KEYWORD') for row in extra.values())
  if name == 'run_reduction_test':
    assert set(extra) == {'bd1_train', 'bd2_train', 'frame_rate', 'window_list', 'ssd_offset', 'details',
                          'save_results_csv'}
  else:
    assert {'bd1_train', 'bd2_train'} <= set(extra)


def test_parser_flags_and_defaults():
  parser = infer.make_parser()
  flags = vars(parser.parse_args([]))
  assert flags == {
      'tf_dir': None, 'model_dir': None, 'plot_dir': None, 'save_results_csv': None, 'train_files': [],
      'test_files': [], 'window_width': 1000, 'window_step': 500, 'window_overlap': 0.5, 'frame_rate': 100,
      'reduction': 'lda', 'decoder': 'wta', 'window_test': False, 'comparison_test': False,
      'audio_label': 'loudness'}
  flags = parser.parse_args(['--train_files', 'a', '--train_files=b', '--test_files', 'c', '--reduction', 'all',
                             '--decoder=ssd', '--comparison_test', '--nowindow_test', '--frame_rate', '64'])
  assert flags.train_files == ['a', 'b'] and flags.test_files == ['c']
  assert (flags.reduction, flags.decoder, flags.comparison_test, flags.window_test) == ('all', 'ssd', True, False)
  assert flags.frame_rate == 64.0
  for bad in (['--reduction', 'median'], ['--decoder', 'best']):
    with pytest.raises(SystemExit):
      parser.parse_args(bad)


def test_main_needs_its_directories(tmp_path, capsys):
  for argv in ([], ['--tf_dir', str(tmp_path)], ['--model_dir', str(tmp_path)],
               ['--tf_dir', str(tmp_path / 'missing'), '--model_dir', str(tmp_path)]):
    with pytest.raises(SystemExit) as info:
      infer.main(argv)
    assert info.value.code == 2
    assert 'Can not find' in capsys.readouterr().err
