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
import _host_program


def test_static_first_batch_and_counter_rewind_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'list_take_main.cpp', timeout=120)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
