#!/bin/bash
# Generates the golden reference outputs of the models with the closed-form geometries (ShellGeometry, GammaGeometry,
# GaussianGeometry, TTauriDiskGeometry, TorusGeometry, ConicalShellGeometry) under tests/golden/ref_geom/: one lean
# make_fixtures.sh run (reference SKIRT v7.3, `skirt -t 1`, seed 4357) per model. They live beside
# tests/golden/ref/ because that folder's file list is pinned to make_fixtures.sh's own fixture list.
# The large per-cell tables are kept small, as tests/golden/ref/bench does: the ds_cellprops of the octree, the
# Cartesian and the Voronoi model as a digest (bench_digest.cellprops_digest: rows, SHA-256 of the rows and of each
# column, column sums), the 4096-cell ds_isrf of gauss_gamma_cart gzipped (gzip -n: no name, no time stamp).
#   usage: make_geom_fixtures.sh [model]      (no argument: every model)
#   LIST=1 make_geom_fixtures.sh prints the fixture list ("ski seed tag lean" per line) and runs nothing
#   DEST=<dir> writes elsewhere than tests/golden/ref_geom (the regeneration test compares the two)
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
export DEST=${DEST:-$HERE/ref_geom}
MODELS="shell_sph1 torus_sph2 torus_oct cone_cyl ttauri_cyl gauss_gamma_cart vor_geoms free_shell free_gamma free_gauss free_ttauri free_torus free_cone"
for m in ${1:-$MODELS}; do
  bash "$HERE/make_fixtures.sh" "$m" 4357 "${m}_s4357" 1
  [ -z "${LIST:-}" ] || continue
  case "$m" in torus_oct|gauss_gamma_cart|vor_geoms)
    f="$DEST/${m}_s4357_ds_cellprops.dat"
    (cd "$HERE" && python3 -c "import json, sys, bench_digest as B; print(json.dumps(B.cellprops_digest(sys.argv[1]), indent=1, sort_keys=True))" "$f") > "$DEST/${m}_s4357_ds_cellprops_digest.json"
    rm "$f" ;;
  esac
  [ "$m" != gauss_gamma_cart ] || gzip -n -9 -f "$DEST/${m}_s4357_ds_isrf.dat"
done
