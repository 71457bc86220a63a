#!/bin/bash
# GPU-box run of the test suite and the full bench (run from the repo root):
#   tools/gpu_check.sh <tag> [pytest selection...]
# Logs go to $OUT_DIR (default: check_out/ under the repo root).
# Steps run under their own time limits; a step that times out, aborts or
# faults (124/134/137/139) ends the script, a step that merely fails does not.
tag=${1:?tag}
shift
cd "${GRAFT_REPO_ROOT:-.}" || exit 1
out=${OUT_DIR:-check_out}
mkdir -p "$out"
fatal() { case $1 in 124|134|137|139) return 0;; *) return 1;; esac; }
sel=("$@")
[ ${#sel[@]} -eq 0 ] && sel=(tests)
timeout -k 10 900 python -u -m pytest "${sel[@]}" -m gpu -v --timeout 300 --timeout-method thread \
    > "$out/gputest_$tag.log" 2>&1
rc=$?
tail -5 "$out/gputest_$tag.log"
if fatal $rc; then echo "tests ended with $rc: stopping"; exit $rc; fi
timeout -k 10 600 python -u bench.py --full > "$out/bench_$tag.json" 2> "$out/bench_$tag.err"
brc=$?
tail -c 600 "$out/bench_$tag.json"
echo "pytest rc=$rc bench rc=$brc"
exit $(( rc != 0 ? rc : brc ))
