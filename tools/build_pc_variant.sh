#!/bin/bash
# A/B variant of the library: abtmp/<name>.so from posecell.hip compiled with extra hipcc
# flags (e.g. -DPC_CO_YREG=1) on top of the product's (tools/build_variant.py).
# usage: tools/build_pc_variant.sh <name> [extra hipcc flags...]
set -euo pipefail
name=$1; shift
exec python3 "$(dirname "$0")/build_variant.py" "$name" --source posecell.hip -- "$@"
