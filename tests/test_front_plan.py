"""The fused front's launch rule (csrc/vt_plan.h: front_fused, front_grid) on the host:
tests/front_plan_main.cpp checks, for 1..2,000 template blocks, that the rule fuses exactly the
libraries one thread block covers (the wider rule, "or the query groups fill the resident
thread blocks", measured slower where it applied and was taken out), and, for 1..20,000
queries, that the grid, walked as vt_front_kernel walks it, serves every query group exactly
once within the cap.  Built with the host compiler and
-fsanitize=address,undefined and run as a child process; the sanitizer is linked into the
program, nothing is preloaded.  CPU only; skipped where the host compiler is absent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')


@pytest.mark.skipif(not CXX, reason='host C++ compiler absent')
def test_front_rule_and_grid_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'front_plan')
    # the sanitizer runtimes linked into the program (clang's default; gcc's is shared)
    gcc = 'clang' not in subprocess.run([CXX, '--version'], stdout=subprocess.PIPE, text=True).stdout
    static = ['-static-libasan', '-static-libubsan'] if gcc else []
    subprocess.check_call([CXX, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', *static,
                           '-I' + os.path.join(ROOT, 'pyratslam_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'front_plan_main.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
