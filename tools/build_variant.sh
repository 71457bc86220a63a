#!/bin/bash
# A/B variant of the library: tools/ab/<name>.so from view_templates.hip (or a given
# source file in its place) with extra hipcc flags on top of the product's
# (tools/build_variant.py).
# usage: tools/build_variant.sh <name> [vt_source.hip] [extra hipcc flags...]
set -euo pipefail
name=$1; src=${2:-}; shift; shift || true
exec python3 "$(dirname "$0")/build_variant.py" "$name" --source view_templates.hip --out "tools/ab/$name.so" \
    ${src:+--file "$src"} -- "$@"
