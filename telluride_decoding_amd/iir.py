"""Butterworth second-order-section design in NumPy: what the reference gets from
`scipy.signal.butter(order, cutoff, 'hp' | 'lp', output='sos', fs=fs)` and `scipy.signal.sosfilt_zi`
(preprocess.py:118-146, 293-300), restated so that the package needs no scipy at run time.

The steps are scipy's (its documented algorithm, BSD-licensed): the analog Butterworth prototype, the
low-pass -> low-/high-pass transform at the pre-warped cutoff, the bilinear transform at fs = 2, and
`zpk2sos` with 'nearest' pairing (the "worst" poles -- closest to the unit circle -- in the last
sections).  tests/test_cpu_preprocess.py pins the result against scipy to 1e-12.
"""
import numpy as np


def _cplxreal(z):
  """(complex halves with positive imaginary part, reals), conjugate pairs averaged (scipy _cplxreal)."""
  z = np.atleast_1d(z)
  if z.size == 0:
    return z, z
  tol = 100 * np.finfo((1.0 * z).dtype).eps
  z = z[np.lexsort((abs(z.imag), z.real))]
  real_indices = abs(z.imag) <= tol * abs(z)
  zr = z[real_indices].real
  if len(zr) == len(z):
    return np.array([]), zr
  z = z[~real_indices]
  zp = z[z.imag > 0]
  zn = z[z.imag < 0]
  if len(zp) != len(zn):
    raise ValueError('Array contains complex value with no matching conjugate.')
  same_real = np.diff(zp.real) <= tol * abs(zp[:-1])
  diffs = np.diff(np.concatenate(([0], same_real, [0])))
  run_starts = np.nonzero(diffs > 0)[0]
  run_stops = np.nonzero(diffs < 0)[0]
  for start, stop in zip(run_starts, run_stops + 1):
    for chunk in (zp[start:stop], zn[start:stop]):
      chunk[...] = chunk[np.lexsort([abs(chunk.imag)])]
  if any(abs(zp - zn.conj()) > tol * abs(zn)):
    raise ValueError('Array contains complex value with no matching conjugate.')
  return (zp + zn.conj()) / 2, zr


def _poly_real(roots):
  c = np.atleast_1d(np.poly(roots)) if len(roots) else np.array([1.0])
  return c.real.copy() if np.iscomplexobj(c) else c


def _single_section(z, p):
  sos = np.zeros(6)
  b, a = _poly_real(z), _poly_real(p)
  sos[3 - len(b):3] = b
  sos[6 - len(a):6] = a
  return sos


def _nearest_idx(fro, to, which):
  order = np.argsort(np.abs(fro - to))
  if which == 'any':
    return order[0]
  mask = np.isreal(fro[order])
  if which == 'complex':
    mask = ~mask
  return order[np.nonzero(mask)[0][0]]


def zpk2sos(z, p, k):
  """Digital zeros / poles / gain -> second-order sections, 'nearest' pairing (scipy.signal.zpk2sos)."""
  if len(z) == len(p) == 0:
    return np.array([[k, 0., 0., 1., 0., 0.]])
  p = np.concatenate((p, np.zeros(max(len(z) - len(p), 0))))
  z = np.concatenate((z, np.zeros(max(len(p) - len(z), 0))))
  n_sections = (max(len(p), len(z)) + 1) // 2
  if len(p) % 2 == 1:
    p = np.concatenate((p, [0.]))
    z = np.concatenate((z, [0.]))
  z = np.concatenate(_cplxreal(z))
  p = np.concatenate(_cplxreal(p))
  k = np.real(k)

  def idx_worst(v):
    return np.argmin(np.abs(1 - np.abs(v)))

  sos = np.zeros((n_sections, 6))
  for si in range(n_sections - 1, -1, -1):
    p1_idx = idx_worst(p)
    p1 = p[p1_idx]
    p = np.delete(p, p1_idx)
    if np.isreal(p1) and np.isreal(p).sum() == 0:
      z1_idx = _nearest_idx(z, p1, 'real')
      z1 = z[z1_idx]
      z = np.delete(z, z1_idx)
      sos[si] = _single_section([z1, 0], [p1, 0])
    elif (len(p) + 1 == len(z) and not np.isreal(p1) and np.isreal(p).sum() == 1
          and np.isreal(z).sum() == 1):
      z1_idx = _nearest_idx(z, p1, 'complex')
      z1 = z[z1_idx]
      z = np.delete(z, z1_idx)
      sos[si] = _single_section([z1, z1.conj()], [p1, p1.conj()])
    else:
      if np.isreal(p1):
        prealidx = np.flatnonzero(np.isreal(p))
        p2_idx = prealidx[idx_worst(p[prealidx])]
        p2 = p[p2_idx]
        p = np.delete(p, p2_idx)
      else:
        p2 = p1.conj()
      if len(z) > 0:
        z1_idx = _nearest_idx(z, p1, 'any')
        z1 = z[z1_idx]
        z = np.delete(z, z1_idx)
        if not np.isreal(z1):
          sos[si] = _single_section([z1, z1.conj()], [p1, p2])
        elif len(z) > 0:
          z2_idx = _nearest_idx(z, p1, 'real')
          z2 = z[z2_idx]
          z = np.delete(z, z2_idx)
          sos[si] = _single_section([z1, z2], [p1, p2])
        else:
          sos[si] = _single_section([z1], [p1, p2])
      else:
        sos[si] = _single_section([], [p1, p2])
  sos[0][:3] *= k
  return sos


def butter_sos(order, cutoff, btype, fs):
  """scipy.signal.butter(order, cutoff, btype, output='sos', fs=fs); btype 'lp' / 'lowpass' or 'hp' /
  'highpass'.  The cutoff must lie strictly between 0 and fs / 2 (ValueError, as scipy)."""
  order = int(order)
  if order < 1:
    raise ValueError('Filter order must be a positive integer, not %r' % (order,))
  btype = {'lp': 'lowpass', 'low': 'lowpass', 'lowpass': 'lowpass',
           'hp': 'highpass', 'high': 'highpass', 'highpass': 'highpass'}[btype]
  wn = 2 * float(cutoff) / fs
  if wn <= 0 or wn >= 1:
    raise ValueError('Digital filter critical frequencies must be 0 < Wn < fs/2 (fs=%s -> fs/2=%s)'
                     % (fs, fs / 2))
  # analog prototype (scipy buttap): N poles on the left unit half-circle, no zeros, gain 1
  m = np.arange(-order + 1, order, 2)
  p = -np.exp(1j * np.pi * m / (2 * order))
  z = np.array([])
  k = 1
  warped = 2 * 2.0 * np.tan(np.pi * wn / 2.0)          # pre-warp at fs = 2
  degree = len(p) - len(z)
  if btype == 'lowpass':
    z, p, k = warped * z, warped * p, k * warped ** degree
  else:
    z_hp, p_hp = warped / z, warped / p
    k = k * np.real(np.prod(-z) / np.prod(-p))
    z, p = np.append(z_hp, np.zeros(degree)), p_hp
  fs2 = 4.0                                            # bilinear transform at fs = 2
  degree = len(p) - len(z)
  z_z = (fs2 + z) / (fs2 - z)
  p_z = (fs2 + p) / (fs2 - p)
  z_z = np.append(z_z, -np.ones(degree))
  k = k * np.real(np.prod(fs2 - z) / np.prod(fs2 - p))
  return zpk2sos(z_z, p_z, k)


def _lfilter_zi(b, a):
  b = np.atleast_1d(b).astype(np.float64)
  a = np.atleast_1d(a).astype(np.float64)
  while len(a) > 1 and a[0] == 0.0:
    a = a[1:]
  if a[0] != 1.0:
    b = b / a[0]
    a = a / a[0]
  n = max(len(a), len(b))
  a = np.r_[a, np.zeros(n - len(a))]
  b = np.r_[b, np.zeros(n - len(b))]
  companion = np.zeros((n - 1, n - 1))
  companion[0, :] = -a[1:] / a[0]
  companion[np.arange(1, n - 1), np.arange(0, n - 2)] = 1
  i_minus_a = np.eye(n - 1) - companion.T
  rhs = b[1:] - a[1:] * b[0]
  return np.linalg.solve(i_minus_a, rhs)


def sosfilt_zi(sos):
  """Step-response steady state of every section, [S, 2] (scipy.signal.sosfilt_zi)."""
  sos = np.asarray(sos, dtype=np.float64)
  zi = np.empty((sos.shape[0], 2))
  scale = 1.0
  for s in range(sos.shape[0]):
    b, a = sos[s, :3], sos[s, 3:]
    zi[s] = scale * _lfilter_zi(b, a)
    scale *= b.sum() / a.sum()
  return zi
