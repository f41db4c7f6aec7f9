"""The many-output FIR and CCA projection kernels of csrc/decode.hip at their edges: what tests/test_cpu_fir_edges.py
(no GPU) and tests/test_gpu_fir_edges.py share.  Test infrastructure.

  * the launch ladder of td_launch_fir / td_cca_transform restated (fir_route, cca_route, strip_rows), with its constants
    parsed out of the source (source_constants);
  * the case tables: every case names the route it is there for;
  * three fillings -- exact (integers whose every product and partial sum is a float32), real (the recipe of
    test_predict_fir_streamed_kernel_edges) and non-finite -- with their float64 references
    (oracle.lag.lag_matrix @ w + b, oracle.cca.cca_transform);
  * reference-side models: a pessimistic float32 chain (the bound of the real tier) and six wrong kernels (what the
    tiers must be able to see).
"""
import collections
import functools
import os
import re
import zlib

import numpy as np

from oracle import cca as o_cca
from oracle import lag as o_lag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- constants of decode.hip / decode_common.h, restated (test_cpu_fir_edges compares them with the source) ----------
THREADS = 256                # kThreads: four waves per workgroup
FIR_MAX_D = 16               # kFirMaxD: the most dims of td_cca_transform
FIR_TILE_DW = 4 * 3 * 64 * 4   # kFirTileDw: dwords of one 32-lag weight tile of predict_fir_mfma_kernel
FIR_LDS_MAX = 80 * 1024      # kFirLdsMax: LDS a workgroup of predict_fir_mfma_kernel may ask for
RING_START, RING_MARGIN = 64, 32   # ring = 64; while (ring < 32 + nl) ring *= 2
PROJ_WAVES = 4               # kProjWaves: cca_project_kernel walks 32 * kProjWaves rows per workgroup at least
FIR_WAVES_PER_CU = 8         # kFirWavesPerCu
PROJ_WAVES_PER_CU = 12       # kProjWavesPerCu
STRIP_MIN = 128              # project_mfma_kernel, predict_fir_mfma_kernel, predict_fir_wave_kernel
MFMA_STRIP_CAP = 4096
WAVE_STRIP_CAP = 8192
WAVE_STRIP_PER_TAP = 8       # predict_fir_wave_kernel: a strip is at least 8 * NL rows
VALU_TILE = THREADS          # predict_fir_kernel: one workgroup = 256 frames
CUS = 256

CONSTANT_NAMES = {'kThreads': THREADS, 'kFirMaxD': FIR_MAX_D, 'kFirTileDw': FIR_TILE_DW, 'kFirLdsMax': FIR_LDS_MAX,
                  'kProjWaves': PROJ_WAVES, 'kFirWavesPerCu': FIR_WAVES_PER_CU, 'kProjWavesPerCu': PROJ_WAVES_PER_CU}


def _product(text):
  value = 1
  for part in text.split('*'):
    value *= int(part)
  return value


def source_constants():
  """{name: value} of what is restated above, read from the text of csrc/decode.hip and csrc/decode_common.h: the
  constexpr constants by name, the ring rule, and the strip minima and caps of td_launch_fir in source order."""
  text = ''
  for name in ('decode_common.h', 'decode.hip'):
    with open(os.path.join(ROOT, 'telluride_decoding_amd', 'csrc', name)) as f:
      text += f.read()
  found = {}
  for m in re.finditer(r'constexpr\s+(?:int|size_t)\s+(\w+)\s*=\s*([\d\s*]+);', text):
    if m.group(1) in CONSTANT_NAMES:
      assert m.group(1) not in found, m.group(1)
      found[m.group(1)] = _product(m.group(2))
  m = re.search(r'int ring = (\d+);\s*while \(ring < (\d+) \+ nl\) ring \*= 2;', text)
  found['ring'] = (int(m.group(1)), int(m.group(2)))
  launch = text[text.index('int td_launch_fir(td_handle* h, const float* x, int64_t ldx, const int64_t* offs, int num_files,\n'
                           '                  int c, int pre, int post, const float* w, const float* bias, int d, float* out,\n'
                           '                  int64_t ldout, int64_t shift, int64_t w_file_stride'):]
  launch = launch[:launch.index('extern "C"')]
  found['strip_min'] = [int(v) for v in re.findall(r'if \(strip < (\d+)\) strip = \1;', launch)]
  found['strip_cap'] = [int(v) for v in re.findall(r'if \(strip > (\d+)\) strip = \1;', launch)]
  found['strip_per_tap'] = [int(v) for v in re.findall(r'if \(strip < (\d+) \* nlv\) strip = \1 \* nlv;', launch)]
  found['valu_tile'] = re.findall(r't0 < n; t0 \+= (\w+)\)', launch)
  m = re.search(r'if \(strip < 32 \* kProjWaves\) strip = 32 \* kProjWaves;', text)
  found['cca_strip_min'] = 32 * found['kProjWaves'] if m else None
  return found


def restated_constants():
  """The same dictionary from the constants of this module."""
  out = dict(CONSTANT_NAMES)
  out.update(ring=(RING_START, RING_MARGIN), strip_min=[STRIP_MIN] * 3, strip_cap=[MFMA_STRIP_CAP, WAVE_STRIP_CAP],
             strip_per_tap=[WAVE_STRIP_PER_TAP], valu_tile=['kThreads'], cca_strip_min=32 * PROJ_WAVES)
  return out


# ---- the ladder of td_launch_fir, restated --------------------------------------------------------------------------
Route = collections.namedtuple('Route', 'name detail')


def _ceil_div(a, b):
  return -(-a // b)


def _round_up(a, b):
  return _ceil_div(a, b) * b


def mfma_plan(c, nl, d):
  """(dq_max, groups, tpq, ring, lds bytes) of predict_fir_mfma_kernel for d outputs of nl lags over c channels."""
  nch, tpq = _ceil_div(c, 64), _ceil_div(nl, 32)
  ring = RING_START
  while ring < RING_MARGIN + nl:
    ring *= 2
  waves = THREADS // 64

  def lds_for(dq):
    return 4 * (dq * tpq * nch * FIR_TILE_DW + waves * (nch * 2048 + ring * dq))
  dq_max = min(d, 16)
  while dq_max > 1 and lds_for(dq_max) > FIR_LDS_MAX:
    dq_max -= 1
  return dq_max, _ceil_div(d, dq_max), tpq, ring, lds_for(dq_max)


def valu_passes(d):
  out, q0 = [], 0
  while q0 < d:
    db = 4 if d - q0 >= 4 else 2 if d - q0 >= 2 else 1
    out.append(db)
    q0 += db
  return out


def fir_route(c, pre, post, d, ldx, base_aligned=True, per_file=False, mode='f16x2'):
  """The kernel td_launch_fir picks.  Route names: project4|8|16|32, stream, mfma (detail: dq_max, groups, tpq, ring),
  wave32x2 / wave32x1 / wave4x8 (detail: channel passes, output passes), valu (detail: the DB of every pass),
  per_file_each (detail: the route of each per-recording recursion).  (Recordings are far below the 2 GB at which the
  streamed kernel steps aside; `mode` only chooses among the streamed kernel's instances.)"""
  nl = pre + 1 + post
  dq_max, groups, tpq, ring, lds = mfma_plan(c, nl, d)
  vec4 = ldx % 4 == 0 and c % 4 == 0 and base_aligned
  mfma_ok = c <= 64 and vec4 and lds <= FIR_LDS_MAX
  if per_file and not mfma_ok:
    return Route('per_file_each', fir_route(c, pre, post, d, ldx, base_aligned, False, mode))
  if not per_file and nl == 1 and 4 <= c <= 64 and vec4 and d <= 32:
    return Route('project%d' % (4 if c <= 8 else 8 if c <= 16 else 16 if c <= 32 else 32), None)
  if not per_file and d == 1 and nl <= 64 and 1 <= c <= 128 and ldx <= 8192:
    return Route('stream', None)
  if mfma_ok:
    return Route('mfma', (dq_max, groups, tpq, ring))
  if nl <= 32:
    nlv = 4 if nl <= 4 else 32
    dqv = 8 if nl <= 4 else 2 if d > 1 else 1
    return Route('wave%dx%d' % (nlv, dqv), (_ceil_div(c, 64), _ceil_div(d, dqv)))
  return Route('valu', tuple(valu_passes(d)))


def leaf(route):
  return route.detail if route.name == 'per_file_each' else route


def strip_rows(route, total=0):
  """Rows of a strip (a wave's share; a workgroup's for valu and the fused CCA kernels) at `total` rows in the call."""
  name = leaf(route).name if isinstance(route, Route) else route
  if name.startswith('project'):
    return max(STRIP_MIN, _round_up(_ceil_div(total, 256 * PROJ_WAVES_PER_CU), 64))
  if name == 'mfma':
    return min(MFMA_STRIP_CAP, max(STRIP_MIN, _round_up(_ceil_div(total, 256 * FIR_WAVES_PER_CU), 32)))
  if name.startswith('wave'):
    nlv = 4 if name.startswith('wave4') else 32
    return min(WAVE_STRIP_CAP, max(STRIP_MIN, WAVE_STRIP_PER_TAP * nlv, _round_up(_ceil_div(total, 256 * 16), 32)))
  if name == 'valu':
    return VALU_TILE
  if name.startswith('cca_project'):
    return max(32 * PROJ_WAVES, _round_up(_ceil_div(total, 3 * CUS), 32 * PROJ_WAVES))
  raise ValueError(name)


def cca_route(c1, pre1, post1, c2, pre2, post2, dims, ldx, ldx2, base_aligned=True, base2_aligned=True, mode='f16x2'):
  """td_cca_transform: cca_stream, cca_project108, cca_project76, or fallback with the FIR routes of the two views."""
  assert 1 <= dims <= FIR_MAX_D
  aligned = (ldx % 4 == 0 and c1 % 4 == 0 and base_aligned and ldx2 % 4 == 0 and c2 % 4 == 0 and base2_aligned)
  if pre1 + post1 == 0 and pre2 + post2 == 0 and c1 <= 64 and c2 <= 32 and 2 * dims <= 16 and aligned and mode != 'f32':
    if c2 <= 8 and ldx < (1 << 20) and ldx2 < (1 << 20):
      return Route('cca_stream', None)
    return Route('cca_project76' if c2 <= 8 else 'cca_project108', None)
  return Route('fallback', (fir_route(c1, pre1, post1, dims, ldx, base_aligned, False, mode),
                            fir_route(c2, pre2, post2, dims, ldx2, base2_aligned, False, mode)))


# ---- the case tables ------------------------------------------------------------------------------------------------
R128 = (1, 31, 32, 33, 127, 128, 129, 0, 300)     # 128-row strips; an empty recording in the middle
R256 = (1, 33, 255, 256, 257, 0, 600)             # predict_fir_wave_kernel at NL = 32 (256-row strips), the VALU tiles
RSHORT = (5, 3, 2)                                # shorter than a context of pre = post = 6
RCCA = (1, 31, 33, 97, 128, 129, 0, 300)
RPF = (300, 0, 1, 129, 33)                        # per-file weights: padding strips make whole workgroups
MAX_ROWS = 700

FirCase = collections.namedtuple('FirCase', 'route c pre post d lens off pad per_file detail')
CcaCase = collections.namedtuple('CcaCase', 'route c1 c2 dims lens off pre1 pad mode detail')


def _fir(route, c, pre, post, d, lens, off=0, pad=0, per_file=False, detail=None):
  return FirCase(route, c, pre, post, d, tuple(lens), off, pad, per_file, detail)


FIR_CASES = [
    # ---- project_mfma_kernel<4|8|16|32>: every instance at both ends of its channel range; halves that stick out of
    # a narrow row (c = 4, 12, 20, 36, 60); d = 33 leaves for the matrix-core kernel in groups of three
    _fir('project4', 4, 0, 0, 1, R128),
    _fir('project4', 8, 0, 0, 2, R128, off=2),
    _fir('project8', 12, 0, 0, 16, R128),
    _fir('project8', 16, 0, 0, 31, R128),
    _fir('project16', 20, 0, 0, 32, R128),
    _fir('project16', 32, 0, 0, 1, R128, off=2),
    _fir('project32', 36, 0, 0, 2, R128),
    _fir('project32', 60, 0, 0, 16, R128),
    _fir('project32', 64, 0, 0, 31, R128),
    _fir('project32', 64, 0, 0, 32, R128, off=2),
    _fir('project8', 16, 0, 0, 2, R128, pad=4),
    _fir('project32', 60, 0, 0, 31, R128, pad=4),
    _fir('wave4x8', 16, 0, 0, 2, R128, pad=1, detail=(1, 1)),            # unaligned rows leave the route
    _fir('wave4x8', 64, 0, 0, 9, R128, pad=3, detail=(1, 2)),
    _fir('mfma', 8, 0, 0, 33, R128, detail=(3, 11, 1, 64)),              # d = 33 leaves the route
    _fir('project4', 4, 0, 0, 2, RSHORT),
    # ---- predict_fir_mfma_kernel: detail = (dq_max, groups, tpq, ring)
    _fir('mfma', 64, 0, 31, 3, R128, detail=(3, 1, 1, 64)),              # the production lags, unmasked interior load
    _fir('mfma', 64, 31, 0, 7, R128, detail=(3, 3, 1, 64)),              # all the context before; last group of one
    _fir('mfma', 64, 15, 16, 17, R128, off=2, detail=(3, 6, 1, 64)),     # split; last group of two
    _fir('mfma', 36, 0, 1, 2, R128, detail=(2, 1, 1, 64)),
    _fir('mfma', 4, 1, 0, 4, R128, detail=(3, 2, 1, 64)),
    _fir('mfma', 60, 0, 30, 7, R128, detail=(3, 3, 1, 64)),              # 31 lags: one padded column
    _fir('mfma', 36, 30, 0, 3, R128, off=2, detail=(3, 1, 1, 64)),
    _fir('mfma', 4, 15, 15, 17, R128, detail=(3, 6, 1, 64)),
    _fir('mfma', 4, 16, 16, 2, R128, detail=(1, 2, 2, 128)),             # 33 lags: tpq 2, the 128-slot ring
    _fir('mfma', 64, 0, 32, 3, R128, detail=(1, 3, 2, 128)),
    _fir('mfma', 60, 32, 0, 4, R128, off=2, detail=(1, 4, 2, 128)),
    _fir('mfma', 64, 0, 63, 2, R128, detail=(1, 2, 2, 128)),             # 64 lags: two whole tiles
    _fir('mfma', 36, 63, 0, 3, R128, detail=(1, 3, 2, 128)),
    _fir('mfma', 4, 32, 32, 2, R128, detail=(1, 2, 3, 128)),             # 65 lags: tpq 3
    _fir('mfma', 64, 0, 64, 1, R128, detail=(1, 1, 3, 128)),             # one output, past the streamed kernel's 64 lags
    _fir('mfma', 36, 40, 40, 1, R128, off=2, detail=(1, 1, 3, 128)),
    _fir('mfma', 64, 0, 95, 2, R128, detail=(1, 2, 3, 128)),             # 96 lags: the last shape inside 80 KB
    _fir('mfma', 60, 95, 0, 1, R128, detail=(1, 1, 3, 128)),
    _fir('mfma', 36, 47, 48, 3, R128, detail=(1, 3, 3, 128)),
    _fir('mfma', 64, 0, 31, 3, R128, pad=4, detail=(3, 1, 1, 64)),       # rows wider than the channels used
    _fir('mfma', 36, 2, 2, 4, R128, pad=4, off=2, detail=(3, 2, 1, 64)),
    _fir('wave32x2', 64, 0, 31, 3, R256, pad=1, detail=(1, 2)),          # unaligned rows leave the route
    _fir('valu', 64, 0, 32, 3, R256, pad=3, detail=(2, 1)),
    _fir('mfma', 4, 6, 6, 2, RSHORT, detail=(2, 1, 1, 64)),              # recordings shorter than the context
    _fir('mfma', 64, 6, 6, 7, RSHORT, detail=(3, 3, 1, 64)),
    # ---- td_predict_fir_per_file
    _fir('mfma', 64, 0, 31, 3, RPF, per_file=True, detail=(3, 1, 1, 64)),
    _fir('per_file_each', 70, 0, 3, 2, RPF, per_file=True, detail=Route('wave4x8', (2, 1))),
    _fir('per_file_each', 63, 2, 5, 2, RPF, off=2, per_file=True, detail=Route('wave32x2', (1, 1))),
    # ---- predict_fir_wave_kernel<32, 2>: detail = (channel passes, output passes)
    _fir('wave32x2', 1, 0, 4, 2, R256, detail=(1, 1)),
    _fir('wave32x2', 5, 12, 0, 3, R256, detail=(1, 2)),
    _fir('wave32x2', 63, 0, 31, 5, R256, detail=(1, 3)),
    _fir('wave32x2', 65, 15, 15, 2, R256, off=2, detail=(2, 1)),
    _fir('wave32x2', 69, 0, 31, 3, R256, detail=(2, 2)),
    _fir('wave32x2', 128, 2, 2, 5, R256, detail=(2, 3)),
    _fir('wave32x2', 129, 6, 6, 2, R256, detail=(3, 1)),
    _fir('wave32x2', 130, 31, 0, 3, R256, off=2, detail=(3, 2)),
    _fir('wave32x2', 5, 6, 6, 2, RSHORT, detail=(1, 1)),
    _fir('wave32x2', 63, 30, 0, 2, R256, detail=(1, 1)),
    # ---- predict_fir_wave_kernel<32, 1>: one output outside the streamed kernel's shapes
    _fir('wave32x1', 129, 0, 31, 1, R256, detail=(3, 1)),
    _fir('wave32x1', 130, 4, 0, 1, R256, off=2, detail=(3, 1)),
    _fir('wave32x1', 193, 6, 6, 1, R256, detail=(4, 1)),
    _fir('wave32x1', 63, 0, 31, 1, (300,), pad=8193 - 63, detail=(1, 1)),   # rows 8193 floats apart
    _fir('wave32x1', 129, 6, 6, 1, RSHORT, detail=(3, 1)),
    # ---- predict_fir_wave_kernel<4, 8>
    _fir('wave4x8', 1, 0, 0, 2, R128, detail=(1, 1)),
    _fir('wave4x8', 3, 0, 1, 8, R128, detail=(1, 1)),
    _fir('wave4x8', 7, 1, 2, 9, R128, off=2, detail=(1, 2)),
    _fir('wave4x8', 63, 0, 0, 17, R128, detail=(1, 3)),
    _fir('wave4x8', 65, 1, 0, 2, R128, detail=(2, 1)),
    _fir('wave4x8', 130, 0, 3, 8, R128, detail=(3, 1)),
    _fir('wave4x8', 130, 0, 0, 1, R128, off=2, detail=(3, 1)),
    _fir('wave4x8', 65, 1, 2, 17, R128, detail=(2, 3)),
    _fir('wave4x8', 3, 1, 1, 9, RSHORT, detail=(1, 2)),
    # ---- predict_fir_kernel<4|2|1>: detail = the DB of every pass
    _fir('valu', 5, 0, 32, 2, R256, detail=(2,)),
    _fir('valu', 63, 32, 31, 3, R256, detail=(2, 1)),
    _fir('valu', 65, 0, 64, 1, R256, detail=(1,)),
    _fir('valu', 130, 16, 16, 4, R256, off=2, detail=(4,)),
    _fir('valu', 5, 64, 0, 7, R256, detail=(4, 2, 1)),
    _fir('valu', 130, 0, 32, 1, R256, detail=(1,)),
    _fir('valu', 64, 0, 96, 2, R256, detail=(2,)),                       # 97 lags: past the 80 KB of the matrix-core kernel
    _fir('valu', 63, 40, 24, 7, RSHORT, detail=(4, 2, 1)),
]


def _cca(route, c1, c2, dims, lens, off=0, pre1=0, pad=0, mode='f16x2', detail=None):
  return CcaCase(route, c1, c2, dims, tuple(lens), off, pre1, pad, mode, detail)


_P = lambda name: Route(name, None)      # noqa: E731
CCA_CASES = [
    # ---- cca_project_kernel<108>: second view of 12 .. 32 columns
    _cca('cca_project108', 4, 12, 1, RCCA),
    _cca('cca_project108', 32, 16, 3, RCCA, off=2),
    _cca('cca_project108', 36, 28, 8, RCCA, off=-3),
    _cca('cca_project108', 64, 32, 8, RCCA),
    _cca('cca_project108', 64, 12, 3, RCCA, off=-3),
    _cca('cca_project108', 36, 32, 1, RCCA, off=2),
    _cca('cca_project108', 32, 16, 8, RCCA, off=2, pad=4),
    _cca('cca_project108', 64, 28, 3, RSHORT, off=-3),
    # ---- the fallback: two bias kernels and two td_launch_fir calls
    _cca('fallback', 32, 16, 3, RCCA, off=2, pad=1, detail=(Route('wave4x8', (1, 1)), Route('wave4x8', (1, 1)))),
    _cca('fallback', 64, 8, 9, RCCA, off=-3, detail=(_P('project32'), _P('project4'))),
    _cca('fallback', 64, 32, 16, RCCA, off=2, detail=(_P('project32'), _P('project16'))),
    _cca('fallback', 63, 8, 3, RCCA, off=2, detail=(Route('wave4x8', (1, 1)), _P('project4'))),
    _cca('fallback', 65, 12, 8, RCCA, off=-3, detail=(Route('wave4x8', (2, 1)), _P('project8'))),
    _cca('fallback', 64, 8, 2, RCCA, pre1=2, off=2, detail=(Route('mfma', (2, 1, 1, 64)), _P('project4'))),
    _cca('fallback', 64, 8, 4, RCCA, mode='f32', off=-3, detail=(_P('project32'), _P('project4'))),
    _cca('fallback', 36, 28, 8, RCCA, mode='f32', detail=(_P('project32'), _P('project16'))),
]


def fir_id(case):
  return '%s-c%d-pre%d-post%d-d%d-n%d-off%d-pad%d%s' % (case.route, case.c, case.pre, case.post, case.d, len(case.lens),
                                                        case.off, case.pad, '-perfile' if case.per_file else '')


def cca_id(case):
  return '%s-c%d+%d-dims%d-n%d-off%d-pre%d-pad%d-%s' % (case.route, case.c1, case.c2, case.dims, len(case.lens), case.off,
                                                       case.pre1, case.pad, case.mode)


def fir_case_route(case):
  return fir_route(case.c, case.pre, case.post, case.d, case.c + case.pad, True, case.per_file)


def cca_case_route(case):
  return cca_route(case.c1, case.pre1, 0, case.c2, 0, 0, case.dims, case.c1 + case.pad, case.c2 + case.pad, True, True,
                   case.mode)


def fir_edges(case):
  """The edges a FIR case reaches, as tags."""
  route = fir_case_route(case)
  lf, nl = leaf(route), case.pre + 1 + case.post
  tags = {lf.name, 'lens%d' % len(case.lens), 'off%d' % case.off}
  if route.name == 'per_file_each':
    tags.add('per_file_each')
  if case.per_file and route.name == 'mfma':
    tags.add('per_file_mfma')
  tags.add('pad0' if case.pad == 0 else 'pad4' if case.pad % 4 == 0 else 'pad_odd')
  if 0 in case.lens:
    tags.add('empty_recording')
  if max(case.lens) <= case.pre:
    tags.add('shorter_than_context')
  tags.add('context_%s' % ('none' if nl == 1 else 'after' if case.pre == 0 else 'before' if case.post == 0 else 'split'))
  if lf.name.startswith('project'):
    kh = int(lf.name[7:])
    tags.add('%s_%s' % (lf.name, 'widest' if case.c == 2 * kh else 'narrowest' if case.c == (4 if kh == 4 else kh + 4) else 'mid'))
    if case.c < 2 * kh:
      tags.add('project_half_sticks_out')
    tags.add('project_d%d' % case.d)
  if lf.name == 'mfma':
    dq_max, groups, tpq, ring = lf.detail
    tags.update({'mfma_tpq%d' % tpq, 'mfma_ring%d' % ring, 'mfma_dq%d' % dq_max, 'mfma_nl%d' % nl, 'mfma_c%d' % case.c})
    if case.d % dq_max:
      tags.add('mfma_partial_group_dq%d' % dq_max)
    if groups > 1:
      tags.add('mfma_groups_tpq%d' % min(tpq, 2))
    if case.d == 1:
      tags.add('mfma_one_output')
  if lf.name.startswith('wave'):
    tags.update({'%s_c%d' % (lf.name, case.c), '%s_nl%d' % (lf.name, nl), '%s_d%d' % (lf.name, case.d),
                 '%s_channel_passes%d' % (lf.name, min(lf.detail[0], 3))})
    if case.c + case.pad > 8192:
      tags.add('wave32x1_wide_rows')
  if lf.name == 'valu':
    tags.update({'valu_c%d' % case.c, 'valu_nl%d' % nl, 'valu_db%s' % ''.join(str(v) for v in lf.detail)})
  return tags


REQUIRED_FIR_EDGES = (
    {'project4', 'project8', 'project16', 'project32', 'mfma', 'wave32x2', 'wave32x1', 'wave4x8', 'valu',
     'per_file_each', 'per_file_mfma', 'empty_recording', 'shorter_than_context', 'off0', 'off2', 'pad0', 'pad4',
     'pad_odd', 'context_none', 'context_after', 'context_before', 'context_split', 'project_half_sticks_out',
     'mfma_ring64', 'mfma_ring128', 'mfma_tpq1', 'mfma_tpq2', 'mfma_tpq3', 'mfma_dq3', 'mfma_dq1',
     'mfma_partial_group_dq3', 'mfma_groups_tpq1', 'mfma_groups_tpq2', 'mfma_one_output', 'wave32x1_wide_rows',
     'valu_db1', 'valu_db2', 'valu_db21', 'valu_db4', 'valu_db421'}
    | {'project%d_%s' % (k, e) for k in (4, 8, 16, 32) for e in ('widest', 'narrowest')}
    | {'project_d%d' % d for d in (1, 2, 16, 31, 32)}
    | {'mfma_c%d' % c for c in (4, 36, 60, 64)} | {'mfma_nl%d' % n for n in (2, 31, 32, 33, 64, 65, 96)}
    | {'wave32x2_c%d' % c for c in (1, 5, 63, 65, 69, 128, 129, 130)} | {'wave32x2_nl%d' % n for n in (5, 13, 31, 32)}
    | {'wave32x2_d%d' % d for d in (2, 3, 5)} | {'wave32x1_c%d' % c for c in (129, 130, 193, 63)}
    | {'wave4x8_c%d' % c for c in (1, 3, 7, 63, 65, 130)} | {'wave4x8_nl%d' % n for n in (1, 2, 4)}
    | {'wave4x8_d%d' % d for d in (1, 2, 8, 9, 17)} | {'wave%s_channel_passes%d' % (k, p) for k in ('32x2', '4x8') for p in (1, 2, 3)}
    | {'valu_c%d' % c for c in (5, 63, 65, 130, 64)} | {'valu_nl%d' % n for n in (33, 64, 65, 97)})


def cca_edges(case):
  route = cca_case_route(case)
  tags = {route.name, 'cca_off%d' % case.off, 'cca_dims%d' % case.dims}
  if route.name == 'cca_project108':
    tags.update({'cca108_c1_%d' % case.c1, 'cca108_c2_%d' % case.c2, 'cca108_dims%d' % case.dims})
  else:
    tags.update({'fallback_' + r.name for r in route.detail})
    if case.mode == 'f32':
      tags.add('fallback_f32')
    if case.pre1:
      tags.add('fallback_context')
    if case.pad % 4:
      tags.add('fallback_unaligned')
    tags.add('fallback_c1_%d' % case.c1)
  if 0 in case.lens:
    tags.add('empty_recording')
  if case.pad and case.pad % 4 == 0:
    tags.add('cca_pad4')
  return tags


REQUIRED_CCA_EDGES = (
    {'cca_project108', 'fallback', 'cca_off0', 'cca_off2', 'cca_off-3', 'cca_dims9', 'cca_dims16', 'fallback_f32',
     'fallback_context', 'fallback_unaligned', 'fallback_c1_63', 'fallback_c1_65', 'empty_recording', 'cca_pad4',
     'fallback_mfma', 'fallback_wave4x8', 'fallback_project32', 'fallback_project4'}
    | {'cca108_c1_%d' % c for c in (4, 32, 36, 64)} | {'cca108_c2_%d' % c for c in (12, 16, 28, 32)}
    | {'cca108_dims%d' % d for d in (1, 3, 8)})


# ---- data -----------------------------------------------------------------------------------------------------------
SENTINEL = np.float32(-12345.0)
EXACT_LIMIT = 2.0 ** 23
FirData = collections.namedtuple('FirData', 'x w b')            # x [rows, c], w [K, d] or [files, K, d], b [d] or [files, d]
CcaData = collections.namedtuple('CcaData', 'x x2 mean1 rot1 mean2 rot2')


def _seed(*parts):
  return zlib.crc32(repr(parts).encode())


def _signed(rng, top, shape):
  """Integers in [-top, top], none of them zero where top >= 1."""
  v = rng.integers(1, max(int(top), 1) + 1, size=shape)
  return (v * rng.choice((-1, 1), size=shape)).astype(np.float64)


def _three_piece(rng):
  """+-(2^18 .. 2^19), bit 10 clear, bits 9 and 0 set: the high bf16 piece rounds down, the middle one holds bits 9 .. 2
  and the low one is not zero."""
  v = (int(rng.integers(2 ** 7, 2 ** 8)) << 11) + (1 << 9) + (int(rng.integers(0, 2 ** 8)) << 1) + 1
  return float(rng.choice((-1, 1)) * v)


def _wide_rows(rng, lens, c, nl, k):
  """The wide operand as x: integers up to 2^19 / K everywhere, and in rows more than nl apart one sample of
  2^18 .. 2^19 with all three bf16 pieces live (_three_piece), so that a window holds at most one of them."""
  x = _signed(rng, 2 ** 19 // k, (int(np.sum(lens)), c))
  row0 = 0
  for n in lens:
    for r in range(int(rng.integers(0, nl + 1)), n, nl + 1 + int(rng.integers(0, 8))):
      x[row0 + r, rng.integers(0, c)] = _three_piece(rng)
    row0 += n
  return x


def _wide_cols(rng, k, d):
  """The wide operand as w: the same, one large odd weight per output column."""
  w = _signed(rng, 2 ** 19 // k, (k, d))
  for q in range(d):
    w[rng.integers(0, k), q] = _three_piece(rng)
  return w


EXACT_KINDS = ('wide_x', 'wide_w', 'mid_mid')


def exact_kinds(k):
  """mid_mid (x, w = +-(2^9 + j): the m . m product of the six-product scheme is live) needs K (2^9 + 3)^2 <= 2^22."""
  return EXACT_KINDS if k <= 16 else EXACT_KINDS[:2]


def _weights_shape(case, k):
  return (len(case.lens), k, case.d) if case.per_file else (k, case.d)


@functools.lru_cache(maxsize=None)
def fir_exact(case, kind):
  """Integer data with sum |x| |w| + |b| <= 2^23 per output: one operand wide (see _wide_rows), the other at most 7 in
  magnitude -- one bf16 piece, so the products the six-product scheme drops (m.l, l.m, l.l) are zero -- or both
  +-(2^9 + j).  Every kernel of the ladder then multiplies exactly and sums integers below 2^24 in whatever order."""
  rng = np.random.default_rng(_seed('exact', case, kind))
  nl = case.pre + 1 + case.post
  k, rows = case.c * nl, int(np.sum(case.lens))
  shape = _weights_shape(case, k)
  if kind == 'wide_x':
    x = _wide_rows(rng, case.lens, case.c, nl, k)
    w = _signed(rng, 7, shape)
  elif kind == 'wide_w':
    x = _signed(rng, 7, (rows, case.c))
    w = np.stack([_wide_cols(rng, k, case.d) for _ in case.lens]) if case.per_file else _wide_cols(rng, k, case.d)
  else:
    x = (2 ** 9 + rng.integers(0, 4, size=(rows, case.c))) * rng.choice((-1.0, 1.0), size=(rows, case.c))
    w = (2 ** 9 + rng.integers(0, 4, size=shape)) * rng.choice((-1.0, 1.0), size=shape)
  b = _signed(rng, 2 ** 20, shape[:-2] + (case.d,))
  return FirData(x.astype(np.float32), w.astype(np.float32), b.astype(np.float32))


def _real_rows(rng, lens, c):
  """Rows 2^-20 .. 2^20 apart in scale, an all-zero row and one sample of 3e30 in every recording of more than 40."""
  x = rng.standard_normal((int(np.sum(lens)), c)).astype(np.float32)
  x *= np.exp2(rng.integers(-20, 21, size=(x.shape[0], 1))).astype(np.float32)
  row0 = 0
  for n in lens:
    if n > 40:
      x[row0 + 7] = 0.0
      x[row0 + 20, min(3, c - 1)] = 3.0e30
    row0 += n
  return x


REDRAWS = 8


def _fir_real_draw(case, draw):
  rng = np.random.default_rng(_seed('real', case, draw))
  k = case.c * (case.pre + 1 + case.post)
  shape = _weights_shape(case, k)
  w = (rng.standard_normal(shape) / np.sqrt(k)).astype(np.float32)
  b = rng.standard_normal(shape[:-2] + (case.d,)).astype(np.float32)
  return FirData(_real_rows(rng, case.lens, case.c), w, b)


REAL_FLOOR = 4e-7          # the project's bound for this product (test_predict_fir_streamed_kernel_edges)
REAL_CAP = 2e-6


@functools.lru_cache(maxsize=None)
def fir_real(case):
  """(data, bound): the real filling and max(4e-7, 2 x the distance of the pessimistic float32 model on it).  A draw
  whose bound passes the cap is redrawn, at most REDRAWS times, from the next seed."""
  for draw in range(REDRAWS):
    data = _fir_real_draw(case, draw)
    bound = max(REAL_FLOOR, 2.0 * fir_distance(case, data, fir_chain_model(case, data)))
    if bound <= REAL_CAP:
      break
  return data, bound


def strip_edge_rows(case_lens, strip, turn=0):
  """Where the non-finite samples go: {recording: [(row, value)]}.  By length: the longest recording gets an Inf and a
  NaN on the two sides of its first strip edge (its middle where it has one strip), the next one a NaN in its last row,
  then one in the first row, an Inf a row away from the previous recording, a NaN a row away from the next (`turn`
  rotates that list).  The NaN sits in the last channel, the Inf four channels before the end (or in channel 0)."""
  order = sorted(range(len(case_lens)), key=lambda f: -case_lens[f])
  places = {}
  for rank, f in enumerate(order[:5]):
    n = case_lens[f]
    if n < 2:
      continue
    edge = strip if n > strip + 1 else n // 2
    spots = ([(edge - 1, np.inf), (edge, np.nan)], [(n - 1, np.nan)], [(0, np.nan)], [(1, np.inf)], [(n - 2, np.nan)])
    places[f] = spots[(rank + turn) % len(spots)]
  return places


def _put_nonfinite(x, lens, strip, off=0, turn=0):
  """In place.  Rows counted from a recording's start move with the `off` leading rows the call drops."""
  c = x.shape[1]
  row0 = np.concatenate(([0], np.cumsum(lens)))
  for f, spots in strip_edge_rows(lens, strip, turn).items():
    for row, value in spots:
      r = row if row >= lens[f] - 2 else min(row + off, lens[f] - 1)
      x[row0[f] + r, c - 1 if np.isnan(value) else max(c - 4, 0)] = value
  return x


@functools.lru_cache(maxsize=None)
def fir_nonfinite(case):
  rng = np.random.default_rng(_seed('nonfinite', case))
  k = case.c * (case.pre + 1 + case.post)
  shape = _weights_shape(case, k)
  x = rng.standard_normal((int(np.sum(case.lens)), case.c)).astype(np.float32)
  w = (rng.standard_normal(shape) / np.sqrt(k)).astype(np.float32)
  w[w == 0] = 1.0
  b = rng.standard_normal(shape[:-2] + (case.d,)).astype(np.float32)
  return FirData(_put_nonfinite(x, case.lens, strip_rows(fir_case_route(case)), case.off), w, b)


# ---- references -----------------------------------------------------------------------------------------------------
def recordings(lens, off=0):
  """(first row, rows that exist after the offset, first output row) of every recording that has any."""
  row0 = np.concatenate(([0], np.cumsum(lens)))
  return [(int(row0[f]) + off, lens[f] - off, int(row0[f])) for f in range(len(lens)) if lens[f] - off > 0]


def _file_index(lens, off):
  return [f for f in range(len(lens)) if lens[f] - off > 0]


def fir_lagged(case, data):
  """[(output row 0, lag matrix in float64, w, b in float64)] of every recording with rows."""
  out = []
  for f, (r0, n, o0) in zip(_file_index(case.lens, case.off), recordings(case.lens, case.off)):
    w, b = (data.w[f], data.b[f]) if case.per_file else (data.w, data.b)
    out.append((o0, o_lag.lag_matrix(data.x[r0:r0 + n].astype(np.float64), case.pre, case.post),
                w.astype(np.float64), b.astype(np.float64)))
  return out


def fir_reference(case, data):
  """(want [rows, d] float64, size [rows, d] = |xl| @ |w| + |b|, defined [rows] bool)."""
  rows = int(np.sum(case.lens))
  want, size, defined = np.zeros((rows, case.d)), np.zeros((rows, case.d)), np.zeros(rows, bool)
  with np.errstate(invalid='ignore', over='ignore'):
    for o0, xl, w, b in fir_lagged(case, data):
      want[o0:o0 + len(xl)] = xl @ w + b
      size[o0:o0 + len(xl)] = np.abs(xl) @ np.abs(w) + np.abs(b)
      defined[o0:o0 + len(xl)] = True
  return want, size, defined


def fir_distance(case, data, got):
  """max |got - want| / (|xl| @ |w| + |b|) over the defined outputs."""
  want, size, defined = fir_reference(case, data)
  return float(np.max(np.abs(np.asarray(got, np.float64)[defined] - want[defined]) / size[defined]))


def fir_chain_model(case, data):
  """The pessimistic float32 model: every product rounded to float32, one sequential chain of float32 additions in
  (lag, channel) order, the bias last.  No kernel of the ladder orders its sum worse: they fuse the multiply-add or
  multiply exactly, and all of them split the chain over lanes, tiles or passes."""
  out = np.full((int(np.sum(case.lens)), case.d), SENTINEL, np.float32)
  parts = fir_lagged(case, data)
  if not case.per_file:            # one chain for all recordings: they share the weights
    parts = [(None, np.concatenate([p[1] for p in parts]), parts[0][2], parts[0][3])]
  got = []
  for _, xl, w, b in parts:
    xl32, w32 = xl.astype(np.float32), w.astype(np.float32)
    acc = np.zeros((len(xl), case.d), np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
      for k in range(xl.shape[1]):
        acc += xl32[:, k:k + 1] * w32[k:k + 1]
    got.append(acc + b.astype(np.float32))
  got, at = np.concatenate(got), 0
  for o0, xl, _, _ in fir_lagged(case, data):
    out[o0:o0 + len(xl)] = got[at:at + len(xl)]
    at += len(xl)
  return out


def fir_exact_sizes(case, kind):
  """The largest sum |x| |w| + |b| of any output of the exact filling."""
  _, size, defined = fir_reference(case, fir_exact(case, kind))
  return float(size[defined].max())


def bf16_pieces(v):
  """The three round-to-nearest-even bf16 pieces of float32 values (td_split3), as float32 arrays."""
  def rne(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)
  v = np.asarray(v, np.float32)
  h = rne(v)
  m = rne(v - h)
  return h, m, rne(v - h - m)


# ---- wrong kernels ----------------------------------------------------------------------------------------------------
WRONG_MODELS = ('strip_last_row_dropped', 'lags_shifted', 'last_group_skipped', 'low_piece_dropped',
                'second_pass_overwrites', 'file0_weights')


def _last_group_columns(case):
  """The output columns of a partly filled last group / pass of the case's kernel; () where it has none."""
  lf = leaf(fir_case_route(case))
  per = {'mfma': lambda: lf.detail[0], 'wave32x2': lambda: 2, 'wave4x8': lambda: 8}.get(lf.name)
  if per is None or case.d % per() == 0 or case.d < per():
    return ()
  return tuple(range(case.d - case.d % per(), case.d))


def wrong_applies(case, model):
  if model == 'last_group_skipped':
    return bool(_last_group_columns(case))
  if model == 'second_pass_overwrites':
    return case.c > 64
  if model == 'file0_weights':
    return case.per_file
  if model == 'strip_last_row_dropped':
    return max(case.lens) - case.off > 1
  if model == 'lags_shifted':
    return max(case.lens) - case.off > 1
  return True


def fir_wrong(case, data, model):
  """What a kernel with the named defect returns on `data` (float64 arithmetic otherwise, as float32)."""
  strip = strip_rows(fir_case_route(case))
  out = np.full((int(np.sum(case.lens)), case.d), SENTINEL, np.float32)
  x = data.x
  if model == 'low_piece_dropped':        # of the rows: x as h + m only
    h, m, _ = bf16_pieces(x)
    x = h + m
  files = _file_index(case.lens, case.off)
  for f, (r0, n, o0) in zip(files, recordings(case.lens, case.off)):
    fw = 0 if model == 'file0_weights' else f
    w, b = (data.w[fw], data.b[fw]) if case.per_file else (data.w, data.b)
    w, b = w.astype(np.float64), b.astype(np.float64)
    xf = x[r0:r0 + n].astype(np.float64)
    if model == 'strip_last_row_dropped':     # the row is not loaded: it counts as zero
      xf = xf.copy()
      xf[strip - 1::strip] = 0.0
      xf[-1] = 0.0
    if model == 'lags_shifted':
      xf = np.concatenate((xf[1:], np.zeros((1, case.c))))
    xl = o_lag.lag_matrix(xf, case.pre, case.post)
    if model == 'second_pass_overwrites':
      nl = case.pre + 1 + case.post
      keep = np.tile(np.arange(case.c) >= 64 * ((case.c - 1) // 64), nl)
      xl = xl * keep
    with np.errstate(over='ignore', invalid='ignore'):
      got = (xl @ w + b).astype(np.float32)
    if model == 'last_group_skipped':
      got[:, list(_last_group_columns(case))] = SENTINEL
    out[o0:o0 + n] = got
  return out


def fir_exact_want(case, data):
  """The float32 image of the exact filling's float64 reference, SENTINEL where nothing is defined."""
  want, _, defined = fir_reference(case, data)
  out = np.full(want.shape, SENTINEL, np.float32)
  out[defined] = want[defined].astype(np.float32)
  return out


def fir_nonfinite_want(case, data):
  """numpy's set of non-finite outputs [rows, d]; undefined rows are False (the sentinel is finite)."""
  want, _, defined = fir_reference(case, data)
  return ~np.isfinite(want) & defined[:, None]


# ---- CCA ------------------------------------------------------------------------------------------------------------
def cca_rows(case):
  """[(x row 0, x rows, x2 row 0, x2 rows, output row 0)] of every recording."""
  dx, dy = max(case.off, 0), max(-case.off, 0)
  row0 = np.concatenate(([0], np.cumsum(case.lens)))
  return [(int(row0[f]) + dx, max(case.lens[f] - dx, 0), int(row0[f]) + dy, max(case.lens[f] - dy, 0), int(row0[f]))
          for f in range(len(case.lens))]


def cca_reference(case, data):
  """(want [rows, 2 dims] float64, size, defined [rows, 2 dims] bool): each view's rows are defined separately."""
  rows, dims = int(np.sum(case.lens)), case.dims
  want, size, defined = np.zeros((rows, 2 * dims)), np.zeros((rows, 2 * dims)), np.zeros((rows, 2 * dims), bool)
  m1, r1, m2, r2 = (v.astype(np.float64) for v in (data.mean1, data.rot1, data.mean2, data.rot2))
  with np.errstate(invalid='ignore', over='ignore'):
    for x0, nx, y0, ny, o0 in cca_rows(case):
      xl = o_lag.lag_matrix(data.x[x0:x0 + nx].astype(np.float64), case.pre1, 0)
      yl = data.x2[y0:y0 + ny].astype(np.float64)
      n = max(nx, ny)
      # (the two views of a recording end together; the one an offset shortens has fewer rows: pad it for the oracle)
      xp = np.concatenate((xl, np.zeros((n - nx, xl.shape[1]))))
      yp = np.concatenate((yl, np.zeros((n - ny, yl.shape[1]))))
      both = o_cca.cca_transform(xp, yp, m1, m2, r1, r2)
      want[o0:o0 + nx, :dims] = both[:nx, :dims]
      want[o0:o0 + ny, dims:] = both[:ny, dims:]
      size[o0:o0 + nx, :dims] = (np.abs(xl) + np.abs(m1)) @ np.abs(r1)
      size[o0:o0 + ny, dims:] = (np.abs(yl) + np.abs(m2)) @ np.abs(r2)
      defined[o0:o0 + nx, :dims] = True
      defined[o0:o0 + ny, dims:] = True
  return want, size, defined


@functools.lru_cache(maxsize=None)
def cca_exact(case, kind):
  """The exact filling of both views: out = x R - m R with sum |x| |R| + |m| . |R| <= 2^23 (means of at most 1)."""
  rng = np.random.default_rng(_seed('cca exact', case, kind))
  rows, k1 = int(np.sum(case.lens)), case.c1 * (case.pre1 + 1)
  if kind == 'wide_x':
    x = _wide_rows(rng, case.lens, case.c1, case.pre1 + 1, k1)
    x2 = _wide_rows(rng, case.lens, case.c2, 1, case.c2)
    r1, r2 = _signed(rng, 7, (k1, case.dims)), _signed(rng, 7, (case.c2, case.dims))
  elif kind == 'wide_w':
    x, x2 = _signed(rng, 7, (rows, case.c1)), _signed(rng, 7, (rows, case.c2))
    r1, r2 = _wide_cols(rng, k1, case.dims), _wide_cols(rng, case.c2, case.dims)
  else:
    x, x2, r1, r2 = ((2 ** 9 + rng.integers(0, 4, size=s)) * rng.choice((-1.0, 1.0), size=s)
                     for s in ((rows, case.c1), (rows, case.c2), (k1, case.dims), (case.c2, case.dims)))
  m1, m2 = (rng.integers(-1, 2, size=n).astype(np.float32) for n in (k1, case.c2))
  return CcaData(x.astype(np.float32), x2.astype(np.float32), m1, r1.astype(np.float32), m2, r2.astype(np.float32))


def cca_exact_kinds(case):
  return exact_kinds(max(case.c1 * (case.pre1 + 1), case.c2))


CCA_BOUND = 6e-7           # of test_cca_transform_streamed_kernel_edges


@functools.lru_cache(maxsize=None)
def cca_real(case):
  """The view scales of test_cca_transform_streamed_kernel_edges: EEG in volts with rows 2^30 apart, envelopes in
  thousands, rotations that bring both to O(1)."""
  rng = np.random.default_rng(_seed('cca real', case))
  rows, k1 = int(np.sum(case.lens)), case.c1 * (case.pre1 + 1)
  x = (rng.standard_normal((rows, case.c1)) * 2e-5).astype(np.float32)
  x2 = (rng.standard_normal((rows, case.c2)) * 3e3 + 1e3).astype(np.float32)
  x *= np.exp2(rng.integers(-15, 16, size=(rows, 1))).astype(np.float32)
  mean1 = np.tile(x.mean(0), case.pre1 + 1).astype(np.float32)
  mean2 = x2.mean(0).astype(np.float32)
  rot1 = (rng.standard_normal((k1, case.dims)) * 1e4).astype(np.float32)
  rot2 = (rng.standard_normal((case.c2, case.dims)) * 1e-3).astype(np.float32)
  return CcaData(x, x2, mean1, rot1, mean2, rot2)


@functools.lru_cache(maxsize=None)
def cca_nonfinite(case):
  """O(1) views with the non-finite samples of strip_edge_rows in the first view and, one recording on, in the
  second: a row's outputs of the other view, and the rows only the other view has, must stay finite."""
  rng = np.random.default_rng(_seed('cca nonfinite', case))
  rows, k1 = int(np.sum(case.lens)), case.c1 * (case.pre1 + 1)
  x = rng.standard_normal((rows, case.c1)).astype(np.float32)
  x2 = rng.standard_normal((rows, case.c2)).astype(np.float32)
  _put_nonfinite(x, case.lens, 128, max(case.off, 0))
  _put_nonfinite(x2, case.lens, 128, max(-case.off, 0), turn=2)
  mean1, mean2 = rng.standard_normal(k1).astype(np.float32), rng.standard_normal(case.c2).astype(np.float32)
  rot1 = (rng.standard_normal((k1, case.dims)) / np.sqrt(k1)).astype(np.float32)
  rot2 = (rng.standard_normal((case.c2, case.dims)) / np.sqrt(case.c2)).astype(np.float32)
  return CcaData(x, x2, mean1, rot1, mean2, rot2)


def cca_distance(case, data, got):
  want, size, defined = cca_reference(case, data)
  return float(np.max(np.abs(np.asarray(got, np.float64)[defined] - want[defined]) / size[defined]))


def cca_exact_want(case, data):
  want, _, defined = cca_reference(case, data)
  out = np.full(want.shape, SENTINEL, np.float32)
  out[defined] = want[defined].astype(np.float32)
  return out


def cca_nonfinite_want(case, data):
  want, _, defined = cca_reference(case, data)
  return ~np.isfinite(want) & defined
