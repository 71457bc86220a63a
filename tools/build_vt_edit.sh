#!/bin/bash
# A/B variant of the library from an edited copy of view_templates.hip (the product
# source stays untouched): abtmp/<name>.so, each "old=>new" argument a literal
# substitution in a copy of csrc/ (must match in exactly one file; tools/build_variant.py).
# usage: tools/build_vt_edit.sh <name> ['old=>new' ...]
set -euo pipefail
name=$1; shift
exec python3 "$(dirname "$0")/build_variant.py" "$name" --source view_templates.hip "${@/#/--edit=}"
