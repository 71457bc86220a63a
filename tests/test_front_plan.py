"""The fused front's launch rule (csrc/vt_plan.h: front_fused, front_grid) on the host:
tests/front_plan_main.cpp checks, for 1..2,000 template blocks, that the rule fuses exactly the
libraries one thread block covers (the wider rule, "or the query groups fill the resident
thread blocks", measured slower where it applied and was taken out), and, for 1..20,000
queries, that the grid, walked as vt_front_kernel walks it, serves every query group exactly
once within the cap.  Built with the host compiler and
-fsanitize=address,undefined and run as a child process; the sanitizer is linked into the
program, nothing is preloaded.  CPU only; skipped where the host compiler is absent."""
import _host_program


def test_front_rule_and_grid_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'front_plan_main.cpp', timeout=120)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
