#!/bin/bash
# Generates the golden reference outputs of the Sphere1DDustGrid and Sphere2DDustGrid models under
# tests/golden/ref_sph/: one lean make_fixtures.sh run (reference SKIRT v7.3, `skirt -t 1`, seed 4357) per model.
# They live beside tests/golden/ref/ because that folder's file list is pinned to make_fixtures.sh's own fixture
# list.
#   usage: make_sph_fixtures.sh [model]      (no argument: every model)
#   LIST=1 make_sph_fixtures.sh prints the fixture list ("ski seed tag lean" per line) and runs nothing
#   DEST=<dir> writes elsewhere than tests/golden/ref_sph (the regeneration test compares the two)
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
export DEST=${DEST:-$HERE/ref_sph}
MODELS="pan_sph1 pan_sph1_sa pan_sph1_log pan_sph2 disk_sph2 pan_sph2_sa pan_sph2_cs oligo_sph2"
for m in ${1:-$MODELS}; do
  bash "$HERE/make_fixtures.sh" "$m" 4357 "${m}_s4357" 1
done
