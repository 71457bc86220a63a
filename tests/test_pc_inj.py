"""The rule of a run's injections (csrc/pc_ctl.h: pc_inj_first_bad, what rs_pc_run_odom_inject
refuses before any device work), on the host: tests/pc_inj_main.cpp checks it against a
restatement that judges every injection on its own, on exact-size heap arrays.  It is built
with the host compiler and -fsanitize=address,undefined and run as a child process.  The
sanitizer is linked into the program; nothing is preloaded.  CPU only; skipped where the
host compiler is absent."""
import _host_program


def test_injection_rule_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'pc_inj_main.cpp', include=('include',), timeout=60)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
