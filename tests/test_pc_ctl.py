"""The pose-cell control records formed on the host and the halo form's record rule
(csrc/pc_ctl.h: make_ctl_halo, make_ctl_inline, halo_key_from_records), on the host:
tests/pc_ctl_main.cpp checks them against a brute-force restatement of what the step
kernels rely on, over seeded shift sets on six grids.  It is built with the host compiler
and -fsanitize=address,undefined and run as a child process.  The sanitizer is linked into
the program; nothing is preloaded.  CPU only; skipped where the host compiler is absent."""
import _host_program


def test_halo_control_and_record_rule_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'pc_ctl_main.cpp', include=('include',), timeout=60)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
