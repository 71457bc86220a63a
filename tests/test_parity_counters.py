"""The single list pass's counters, doubled by call parity (csrc/vt_plan.h: ParityCounters,
parity_begin, parity_last_offset), on the host: tests/parity_counters_main.cpp
simulates pruned calls of varying template-block counts and list lengths on a buffer that is
zeroed only when it is allocated.  Every call must find its own parity's counters at zero
(the call before zeroed them), and the previous call's counts must stay readable, any number
of times, until the next call begins; every offset stays inside the exact allocation.  Built
with the host compiler and -fsanitize=address,undefined and run as a child process; the
sanitizer is linked into the program, nothing is preloaded.  CPU only; skipped where the host
compiler is absent."""
import _host_program


def test_every_call_starts_from_zero_and_the_last_counts_stay_readable(tmp_path):
    r = _host_program.run(tmp_path, 'parity_counters_main.cpp', timeout=120)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
