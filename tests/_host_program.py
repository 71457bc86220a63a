"""The one recipe of the stand-alone host programs (tests/*_main.cpp), shared by their tests.

A program includes headers of csrc/ that need no device, is built with the host compiler and
-fsanitize=address,undefined, and run as a child process: the sanitizer is linked into the
program, nothing is preloaded.  Each test keeps its own assertions on what run() returns."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')
CXX = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')


def run(tmp_path, source, include=(), defines=(), flags=(), hip=False, timeout=60):
    """Build tests/``source`` into ``tmp_path`` and run it; returns the finished process with
    stdout and stderr in ``stdout`` (printed, for the check counts).

    include: directories under the repository root searched besides pyratslam_amd/csrc;
    defines, flags: further -D names and compiler flags; hip: the program includes the HIP
    headers (not the runtime).  Skips where the host compiler or those headers are absent."""
    if not CXX:
        pytest.skip('host C++ compiler absent')
    if hip and not os.path.exists(os.path.join(ROCM, 'include', 'hip', 'hip_runtime.h')):
        pytest.skip('HIP headers absent')
    exe = str(tmp_path / source.rsplit('_main.cpp', 1)[0])
    # the sanitizer runtimes linked into the program (clang's default; gcc's is shared)
    gcc = 'clang' not in subprocess.run([CXX, '--version'], stdout=subprocess.PIPE, text=True).stdout
    static = ['-static-libasan', '-static-libubsan'] if gcc else []
    dirs = ([os.path.join(ROCM, 'include')] if hip else []) + [os.path.join(ROOT, d) for d in include]
    subprocess.check_call([CXX, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', *flags, *static, *('-D' + d for d in defines),
                           *('-I' + d for d in dirs), '-I' + os.path.join(ROOT, 'pyratslam_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', source), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    print(r.stdout)
    return r
