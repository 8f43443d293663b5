#!/bin/bash
# Generates the golden reference outputs of the Cylinder2DDustGrid models under tests/golden/ref_cyl/: one lean
# make_fixtures.sh run (reference SKIRT v7.3, `skirt -t 1`, seed 4357) per model. They live beside
# tests/golden/ref/ because that folder's file list is pinned to make_fixtures.sh's own fixture list.
#   usage: make_cyl_fixtures.sh [model]      (no argument: every model)
#   LIST=1 make_cyl_fixtures.sh prints the fixture list ("ski seed tag lean" per line) and runs nothing
#   DEST=<dir> writes elsewhere than tests/golden/ref_cyl (the regeneration test compares the two)
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
export DEST=${DEST:-$HERE/ref_cyl}
MODELS="pan_cyl pan_cyl_sa pan_cyl_cs disk_cyl disk_cyl_log oligo_cyl"
for m in ${1:-$MODELS}; do
  bash "$HERE/make_fixtures.sh" "$m" 4357 "${m}_s4357" 1
done
