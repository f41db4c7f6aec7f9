"""Cuts the first 400 records of the reference's MEG test recording
(/root/reference/test_data/meg/subj01_1ksamples.tfrecords, a data file of the reference's
own tests: BUILD.bazel:40-47) into tests/golden/meg_subj01_400.tfrecords, keeping only the
'meg' and 'envelope' features, and stores the whole recording, byte for byte, as
tests/golden/meg_subj01_1ksamples.tfrecords.gz (the reference's subj02 / subj03 files are
identical copies of it).  Run in the build container (the reference is not on the GPU
box)."""
import gzip
import os
import shutil
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from telluride_decoding_amd import tfrecord

src = '/root/reference/test_data/meg/subj01_1ksamples.tfrecords'
here = os.path.dirname(os.path.abspath(__file__))
dst = os.path.join(here, 'meg_subj01_400.tfrecords')
feats = tfrecord.read_file(src, fields=['meg', 'envelope'], verify=True)
tfrecord.write_file(dst, {k: v[:400] for k, v in feats.items()})
print(dst, os.path.getsize(dst))
whole = os.path.join(here, 'meg_subj01_1ksamples.tfrecords.gz')
with open(src, 'rb') as fin, open(whole, 'wb') as raw:
  with gzip.GzipFile(filename='', mode='wb', compresslevel=9, fileobj=raw, mtime=0) as fout:
    shutil.copyfileobj(fin, fout)
print(whole, os.path.getsize(whole))
