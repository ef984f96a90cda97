"""csrc/kb_layout.h on the host (no GPU needed): the header compiles with a plain host compiler, and tests/kb_layout_walk.cpp --
a stand-alone program built here with the address and undefined-behaviour sanitizers and run as a child process -- walks the
work line of every agent transfer (kb_fork, kb_fork_rebuild, kb_unshare, kb_share) over dictionaries of 0 .. 320 landmarks in
all three storages, under each of the four cuts: every double of [64, top) lies in exactly one run, no run is empty, ragged or
across its cut, every run is where the scan and kb_shells_before say it is, and kb_shells_before is the sum of the shells'
sizes in every storage."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'network-slicing_amd', 'csrc')


def test_walker_under_sanitizers(tmp_path):
    cxx = shutil.which('g++')
    assert cxx, 'no g++ to build the host program with'
    exe = str(tmp_path / 'kb_layout_walk')
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                            '-static-libasan', '-static-libubsan', '-fno-sanitize-recover=all', '-I', CSRC, '-o', exe,
                            os.path.join(ROOT, 'tests', 'kb_layout_walk.cpp')],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)   # (the runtimes are linked in: nothing to preload)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stderr and 'AddressSanitizer' not in run.stderr, run.stderr
    lines = run.stdout.strip().splitlines()
    # three storages x (whole shell, page / rest) + the two that store tiles x (common / partial sums, common / tile by tile)
    assert len(lines) == 11 and lines[-1].endswith(' runs') and int(lines[-1].split()[0]) > 1000


def test_header_includes_nothing_from_hip():
    text = open(os.path.join(CSRC, 'kb_layout.h')).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith('#include')]
    assert includes == ['<stdint.h>']
    kbrl = open(os.path.join(CSRC, 'kb_kbrl.hip')).read()
    assert '#include "kb_layout.h"' in kbrl
    for name in ('KB_CH', 'KB_TILE', 'KB_VEC_ROWS', 'KB_VEC', 'KB_TRI_NONE'):   # moved, not copied
        assert '#define %s ' % name in text and '#define %s ' % name not in kbrl, name
