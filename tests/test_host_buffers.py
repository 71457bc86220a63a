"""rs::DevBuf / rs::PinnedBuf, rs::grown (csrc/rs_common.h) and the handles' growth idiom, on the host:
tests/host_buffers_main.cpp defines the four allocation functions itself (malloc-backed,
counting live blocks, refusing the k-th call) in place of rs_common.cpp, is built with the
host compiler and -fsanitize=address,undefined, and run as a child process.  The sanitizer
is linked into the program; nothing is preloaded.  CPU only; skipped where the host
compiler or the HIP headers are absent.  (The handles themselves need HIP: their growth
sites are covered on the GPU by test_handle_buffers_gpu.py.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')
CXX = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')


@pytest.mark.skipif(not CXX, reason='host C++ compiler absent')
@pytest.mark.skipif(not os.path.exists(os.path.join(ROCM, 'include', 'hip', 'hip_runtime.h')),
                    reason='HIP headers absent')
def test_buffer_types_and_growth_idiom_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'host_buffers')
    # the sanitizer runtimes linked into the program (clang's default; gcc's is shared)
    gcc = 'clang' not in subprocess.run([CXX, '--version'], stdout=subprocess.PIPE, text=True).stdout
    static = ['-static-libasan', '-static-libubsan'] if gcc else []
    subprocess.check_call([CXX, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', *static, '-D__HIP_PLATFORM_AMD__',
                           '-I' + os.path.join(ROCM, 'include'), '-I' + os.path.join(ROOT, 'include'),
                           '-I' + os.path.join(ROOT, 'pyratslam_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'host_buffers_main.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed, 0 live' in r.stdout
