"""rs::DevBuf / rs::PinnedBuf, rs::Stream / rs::Event, rs::grown (csrc/rs_common.h) and the handles'
idioms (group growth, the lazily created stream groups, the event pool, a create's failure
exit), on the host: tests/host_buffers_main.cpp defines the four allocation functions and the
four stream and event functions itself (malloc-backed, counting what is live, refusing the
k-th call) in place of rs_common.cpp, is built with the host compiler and
-fsanitize=address,undefined, and run as a child process.  The sanitizer
is linked into the program; nothing is preloaded.  CPU only; skipped where the host
compiler or the HIP headers are absent.  (The handles themselves need HIP: their growth
sites are covered on the GPU by test_handle_buffers_gpu.py.)"""
import _host_program


def test_buffer_types_and_growth_idiom_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'host_buffers_main.cpp', include=('include',), defines=('__HIP_PLATFORM_AMD__',),
                          hip=True, timeout=60)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed, 0 live' in r.stdout
