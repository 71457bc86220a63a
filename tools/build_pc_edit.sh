#!/bin/bash
# A/B variant of the library from an edited copy of the pose-cell sources (the product
# sources stay untouched): abtmp/<name>.so, with each "old=>new" argument applied as a
# literal substitution to a copy of csrc/ in abtmp/<name>/ (posecell.hip, its pc_*.h parts,
# pc_ctl.h: it must match in exactly one file; tools/build_variant.py).
# usage: tools/build_pc_edit.sh <name> 'old=>new' ['old=>new' ...]
set -euo pipefail
name=$1; shift
exec python3 "$(dirname "$0")/build_variant.py" "$name" --source posecell.hip "${@/#/--edit=}"
