"""The single list pass's counters, doubled by call parity (csrc/vt_plan.h: ParityCounters,
parity_begin, parity_last_offset), on the host: tests/parity_counters_main.cpp
simulates pruned calls of varying template-block counts and list lengths on a buffer that is
zeroed only when it is allocated.  Every call must find its own parity's counters at zero
(the call before zeroed them), and the previous call's counts must stay readable, any number
of times, until the next call begins; every offset stays inside the exact allocation.  Built
with the host compiler and -fsanitize=address,undefined and run as a child process; the
sanitizer is linked into the program, nothing is preloaded.  CPU only; skipped where the host
compiler is absent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')


@pytest.mark.skipif(not CXX, reason='host C++ compiler absent')
def test_every_call_starts_from_zero_and_the_last_counts_stay_readable(tmp_path):
    exe = str(tmp_path / 'parity_counters')
    # the sanitizer runtimes linked into the program (clang's default; gcc's is shared)
    gcc = 'clang' not in subprocess.run([CXX, '--version'], stdout=subprocess.PIPE, text=True).stdout
    static = ['-static-libasan', '-static-libubsan'] if gcc else []
    subprocess.check_call([CXX, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', *static,
                           '-I' + os.path.join(ROOT, 'pyratslam_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'parity_counters_main.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
