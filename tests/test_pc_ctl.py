"""The pose-cell control records formed on the host and the halo form's record rule
(csrc/pc_ctl.h: make_ctl_halo, make_ctl_inline, halo_key_from_records), on the host:
tests/pc_ctl_main.cpp checks them against a brute-force restatement of what the step
kernels rely on, over seeded shift sets on six grids.  It is built with the host compiler
and -fsanitize=address,undefined and run as a child process.  The sanitizer is linked into
the program; nothing is preloaded.  CPU only; skipped where the host compiler is absent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')


@pytest.mark.skipif(not CXX, reason='host C++ compiler absent')
def test_halo_control_and_record_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'pc_ctl')
    # the sanitizer runtimes linked into the program (clang's default; gcc's is shared)
    gcc = 'clang' not in subprocess.run([CXX, '--version'], stdout=subprocess.PIPE, text=True).stdout
    static = ['-static-libasan', '-static-libubsan'] if gcc else []
    subprocess.check_call([CXX, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', *static,
                           '-I' + os.path.join(ROOT, 'include'),
                           '-I' + os.path.join(ROOT, 'pyratslam_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'pc_ctl_main.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
