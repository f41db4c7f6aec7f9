"""Per-kernel comparison of the gfx950 code of two source trees:
python tools/isa_diff.py <parent-csrc-dir> <new-csrc-dir> --out <dir outside the repository>.

Every *.hip of both directories is compiled with build.py's flags plus --cuda-device-only -S (the .s files
go to --out), cut into kernels by symbol and compared as text: comments and blank lines dropped, whitespace
collapsed, .LBB<n>_ / .Lfunc_end<n> renumbered.  One line per kernel symbol: same / changed (opcode counts and
.amdhsa_* lines that differ) / missing / new, and the file that holds it on each side (`a + b`: a kernel
defined in a header, the same code in both files; copies that differ end the run).  Exit status 0 only
when both sides hold the same symbols and every one is `same`."""
import collections, glob, os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from telluride_decoding_amd import build

def compile_dir(csrc, out):
  """{kernel symbol: (file, [normalised body lines], [.amdhsa_* lines])} of every *.hip in csrc."""
  os.makedirs(out, exist_ok=True)
  srcs = sorted(glob.glob(os.path.join(csrc, '*.hip')))
  def cc(src):
    asm = os.path.join(out, os.path.basename(src) + '.s')
    r = subprocess.run([build._hipcc()] + build.compile_flags(csrc) + ['--cuda-device-only', '-S', src, '-o', asm],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode: sys.exit('hipcc failed on %s:\n%s' % (src, r.stdout))
    return asm
  with ThreadPoolExecutor(16) as pool: asms = list(pool.map(cc, srcs))
  kernels = {}
  for asm in asms:
    name = os.path.basename(asm)[:-2]
    lines = [re.sub(r'\s+', ' ', l.split(';')[0]).strip() for l in open(asm)]
    lines = [l for l in lines if l]
    desc = {}                                   # symbol -> its .amdhsa_* lines
    for i, l in enumerate(lines):
      if l.startswith('.amdhsa_kernel '):
        desc[l.split()[1]] = lines[i + 1:lines.index('.end_amdhsa_kernel', i)]
    for sym, d in desc.items():
      i = lines.index(sym + ':')
      j = next(k for k in range(i, len(lines)) if lines[k].startswith('.Lfunc_end'))
      n = re.match(r'\.Lfunc_end(\d+)', lines[j]).group(1)
      body = [re.sub(r'\.LBB%s_' % n, '.LBB_', l) for l in lines[i + 1:j]]
      if sym in kernels:                        # a header's kernel: one line, if every file holds the same code
        if kernels[sym][1:] != (body, d): sys.exit('%s: in %s and in %s, not the same' % (sym, kernels[sym][0], name))
        name = kernels[sym][0] + ' + ' + name
      kernels[sym] = (name, body, d)
  return kernels

def main():
  if len(sys.argv) != 5 or sys.argv[3] != '--out': sys.exit(__doc__)
  out = os.path.abspath(sys.argv[4])
  if os.path.commonpath([out, ROOT]) == ROOT: sys.exit('--out must lie outside the repository')
  old = compile_dir(os.path.abspath(sys.argv[1]), os.path.join(out, 'parent'))
  new = compile_dir(os.path.abspath(sys.argv[2]), os.path.join(out, 'new'))
  bad = 0
  for sym in sorted(set(old) | set(new)):
    where = '%s -> %s' % (old[sym][0] if sym in old else '-', new[sym][0] if sym in new else '-')
    if sym not in new or sym not in old: state = 'missing' if sym in old else 'new'
    elif old[sym][1:] == new[sym][1:]: state = 'same'
    else:
      a, b = (collections.Counter(l.split()[0] for l in k[1]) for k in (old[sym], new[sym]))
      ops = ['%s %d->%d' % (op, a[op], b[op]) for op in sorted(set(a) | set(b)) if a[op] != b[op]]
      hsa = ['%s -> %s' % (x, y) for x, y in zip(old[sym][2], new[sym][2]) if x != y]
      state = 'changed [%s]' % '; '.join(ops + hsa or ['the same opcodes, other operands or order'])
    bad += state != 'same'
    print('%-8s %s  (%s)' % (state.split()[0], sym, where) + (state[7:] if state.startswith('changed') else ''))
  print('%d kernels on the parent side, %d on the new side, %d not the same' % (len(old), len(new), bad))
  return 1 if bad else 0

if __name__ == '__main__':
  sys.exit(main())
