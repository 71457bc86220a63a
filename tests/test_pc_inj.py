"""The rule of a run's injections (csrc/pc_ctl.h: pc_inj_first_bad, what rs_pc_run_odom_inject
refuses before any device work), on the host: tests/pc_inj_main.cpp checks it against a
restatement that judges every injection on its own, on exact-size heap arrays.  It is built
with the host compiler and -fsanitize=address,undefined and run as a child process.  The
sanitizer is linked into the program; nothing is preloaded.  CPU only; skipped where the
host compiler is absent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')


@pytest.mark.skipif(not CXX, reason='host C++ compiler absent')
def test_injection_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'pc_inj')
    # the sanitizer runtimes linked into the program (clang's default; gcc's is shared)
    gcc = 'clang' not in subprocess.run([CXX, '--version'], stdout=subprocess.PIPE, text=True).stdout
    static = ['-static-libasan', '-static-libubsan'] if gcc else []
    subprocess.check_call([CXX, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', *static,
                           '-I' + os.path.join(ROOT, 'include'),
                           '-I' + os.path.join(ROOT, 'pyratslam_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'pc_inj_main.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
