"""The view-template matcher's host decisions (csrc/vt_plan.h: local_count_of, plane_split,
prunes, the prefilter and export grids, the folded-keys decision, stream_path, host_groups),
on the host: tests/vt_plan_main.cpp checks them against an independent restatement of each
rule, by brute force where there is one.  It is built with the host compiler and
-fsanitize=address,undefined and run as a child process.  The sanitizer is linked into the
program; nothing is preloaded.  CPU only; skipped where the host compiler is absent."""
import _host_program


def test_scan_and_stream_plans_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'vt_plan_main.cpp', include=('include',), timeout=60)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
