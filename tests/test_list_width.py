"""The list passes' entries per batch (csrc/vt_plan.h), on the host: tests/list_width_main.cpp

  * checks list_width(entries, per, fill, nqc) for every entries 0..2,000, per 1..4, fill
    1..512 and nqc in {1, 2, 7, 8, 16, 32, 128}: it returns 4, 2 or 1, never a narrower width
    than needed (the next wider one misses fill), and 4 whenever fill <= 1;
  * simulates the kernel's walk at 1, 2 and 4 entries per batch, the width changing from
    launch to launch on counters that are never reset: every entry of every list of length
    0..200 is computed exactly once, no block without a static batch takes, every touched
    counter has one last user and every counter is zero afterwards -- in order, reversed and
    in 300 seeded shuffles;
  * checks the lanes that read the static batch's ids before the length is known: for every
    width they hold exactly the static batch's entries, and no index leaves the slab;
  * checks that the rule's cap of one resident round of blocks (list_round) keeps whole groups
    of eight and that the walk above holds under it, and that both numberings of the grid's
    blocks (block_id) name every (template block, block) once.

Built with the host compiler and -fsanitize=address,undefined and run as a child process; the
sanitizer is linked into the program, nothing is preloaded.  CPU only; skipped where the host
compiler is absent."""
import _host_program


def test_width_rule_walk_and_speculative_lanes_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'list_width_main.cpp', timeout=120)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
