#!/bin/bash
# Generates the golden reference outputs of the polarised models (ElectronDustMix: Stokes Q, U, V frames and SED
# columns of the FullInstruments) under tests/golden/ref_pol/: one make_fixtures.sh run (reference SKIRT v7.3,
# `skirt -t 1`, seed 4357) per model, not lean: every FITS frame (16 x 16 pixels, 5,760 bytes each), the SEDs,
# ds_convergence and the log excerpt. pol_torus_cart's ds_cellprops is kept as a digest
# (bench_digest.cellprops_digest), as make_geom_fixtures.sh keeps them.
#   usage: make_pol_fixtures.sh [model]      (no argument: every model)
#   LIST=1 make_pol_fixtures.sh prints the fixture list ("ski seed tag lean" per line) and runs nothing
#   DEST=<dir> writes elsewhere than tests/golden/ref_pol (the regeneration test compares the two)
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
export DEST=${DEST:-$HERE/ref_pol}
MODELS="pol_torus_cart pol_2comp_sph2"
for m in ${1:-$MODELS}; do
  bash "$HERE/make_fixtures.sh" "$m" 4357 "${m}_s4357" 0
  [ -z "${LIST:-}" ] || continue
  f="$DEST/${m}_s4357_ds_cellprops.dat"
  [ -f "$f" ] || continue
  (cd "$HERE" && python3 -c "import json, sys, bench_digest as B; print(json.dumps(B.cellprops_digest(sys.argv[1]), indent=1, sort_keys=True))" "$f") > "$DEST/${m}_s4357_ds_cellprops_digest.json"
  rm "$f"
done
