"""bench.py's N > 1 logic on the real device layer of a one-GPU box."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_ranks_share_the_gpu():
  """`bench.py --gpus 2 --share-gpu --full`: the launcher starts two ranks, both on GPU 0 over gloo (RCCL
  needs a GPU per rank), and the whole N > 1 path of the file runs on the device: recordings dealt
  to ranks, FitPipeline with the statistics all-reduce on its solve streams, one solver rank per
  fit, the barrier / max-over-ranks timing, the strong-scaling leg by time ranges + halo, and the
  C5 (LOSO x lambda sweep, subjects sharded) and C4 (decode replicas) legs of an N > 1 run.  Only
  the plumbing and the results are judged here (the timings of two ranks on one GPU through gloo mean nothing)."""
  env = {k: v for k, v in os.environ.items()
         if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
  res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--share-gpu',
                        '--steps', '3', '--warmup', '1', '--full', '--no-cpu', '--watchdog-seconds', '150'],
                       env=env, capture_output=True, text=True, timeout=900)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
  line = json.loads([l for l in res.stdout.splitlines() if l.startswith('{')][-1])
  assert line['n_gpus'] == 2 and line['ranks_seen'] == 2 and line['launcher'] == 'self'
  assert line['full'] is True
  assert line['steps'] == 3 and line['value'] > 0 and line['scaling'] == 'weak'
  assert line['strong']['fit_ms_per_step'] > 0
  assert line['strong_8e6']['fit_ms_per_step'] > 0 and line['strong_8e6']['samples_per_s'] > 0
  assert line['collective']['ranks'] == 2
  assert line['roofline']['launches'] == 3
  # BASELINE configs C5 and C4 over the two ranks: subjects / trials dealt to the ranks, the C5 table
  # equal to rank 0's one-GPU sweep to 2e-6, the 10 200 gathered decisions identical to its one-GPU decode
  assert line['loso']['ranks'] == 2 and line['loso']['fits'] == 640 and line['loso']['seconds'] > 0
  assert line['loso']['matches_one_gpu_to_2e-6'] is True, line['loso']['max_abs_diff_vs_one_gpu']
  assert line['loso']['collective']['ranks'] == 2
  assert line['decode']['ranks'] == 2 and line['decode']['windows'] == 10200
  assert line['decode']['decisions_identical_to_one_gpu'] is True
  assert line['decode']['windows_per_s'] > 0


# what only a --full run measures; a plain run's line carries none of it
FULL_ONLY = ('cpu_baseline', 'decode', 'cca', 'loso', 'loso_first_sweep_s', 'decoder_train', 'ledoit_wolf',
             'shapes', 'f32_mode', 'bf16x3_mode', 'serial_ms_per_step', 'serial_solver', 'roofline_whole_chip',
             'single_fit', 'single_fit_latency_ms', 'accumulate_only_ms_per_step', 'strong_share_bound_one_gpu',
             'strong', 'strong_8e6')


def test_bench_plain_run_is_the_headline_alone(tmp_path):
  """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` without --full: the timed steps, the
  dumped W and b of the last one, and the headline line with the roofline of those steps' own launches --
  none of the legs that run after the timed region."""
  env = {k: v for k, v in os.environ.items()
         if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
  out = tmp_path / 'out'
  res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3',
                        '--warmup', '1', '--dump-outputs', str(out), '--watchdog-seconds', '150'],
                       env=env, capture_output=True, text=True, timeout=300)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
  line = json.loads([l for l in res.stdout.splitlines() if l.startswith('{')][-1])
  assert line['metric'] == 'TRF-fit samples/sec' and line['unit'] == 'samples/s'
  assert line['higher_is_better'] is True and line['dtype'].startswith('f32')
  assert line['value'] > 0 and line['ms_per_step'] > 0
  assert abs(line['value'] * line['ms_per_step'] * 1e-3 - 1e6) < 1.0
  assert line['steps'] == 3 and line['warmup'] == 1 and line['full'] is False
  assert line['roofline']['launches'] == 3 and line['roofline']['achieved'] > 0
  assert line['collective']['ranks'] == 1
  assert [k for k in FULL_ONLY if k in line] == []
  w, b = np.load(str(out / 'w.npy')), np.load(str(out / 'b.npy'))
  assert w.shape == (1, 64 * 32, 1) and b.shape == (1, 1)
  assert np.isfinite(w).all() and np.isfinite(b).all() and np.abs(w).max() > 0
