"""The plane scan's batch assignment (csrc/vt_plan.h: list_use, take_plan, take_batch), the
arithmetic vt_scan_plane_kernel runs, on the host: tests/list_take_main.cpp simulates launches
for every list length 0..200, per 1..4 and nqc in {1, 2, 7, 8, 16, 32, 128} with the blocks'
takes interleaved in order, reversed, round robin and in a few hundred seeded shuffles, and
checks that every batch of every group is computed exactly once, that blocks without a static
batch never touch a counter, that exactly one block per used counter sees the last-user
value, that every counter is zero afterwards, and that the next launch (another length, the
same counters) is correct again.  Built with the host compiler and
-fsanitize=address,undefined and run as a child process; the sanitizer is linked into the
program, nothing is preloaded.  CPU only; skipped where the host compiler is absent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')


@pytest.mark.skipif(not CXX, reason='host C++ compiler absent')
def test_static_first_batch_and_counter_rewind_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'list_take')
    # the sanitizer runtimes linked into the program (clang's default; gcc's is shared)
    gcc = 'clang' not in subprocess.run([CXX, '--version'], stdout=subprocess.PIPE, text=True).stdout
    static = ['-static-libasan', '-static-libubsan'] if gcc else []
    subprocess.check_call([CXX, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', *static,
                           '-I' + os.path.join(ROOT, 'pyratslam_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'list_take_main.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
