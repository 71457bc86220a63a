#!/bin/bash
# tools/pc_probe.hip built against an edited copy of the pose-cell sources (the product
# sources stay untouched): abtmp/<name>_probe, each "old=>new" argument a literal
# substitution in a copy of csrc/ (must match in exactly one file; tools/build_variant.py).
# usage: tools/build_probe_edit.sh <name> ['old=>new' ...]
set -euo pipefail
name=$1; shift
exec python3 "$(dirname "$0")/build_variant.py" "$name" --source posecell.hip --probe "${@/#/--edit=}"
