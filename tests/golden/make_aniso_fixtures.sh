#!/bin/bash
# Generates the golden reference outputs of the models with anisotropic sources (NetzerAccretionDiskGeometry,
# StellarSurfaceGeometry, SpheBackgroundGeometry, CubBackgroundGeometry, SolarPatchGeometry, LaserGeometry) under
# tests/golden/ref_aniso/: one lean make_fixtures.sh run (reference SKIRT v7.3, `skirt -t 1`, seed 4357) per model.
# They live beside tests/golden/ref/ because that folder's file list is pinned to make_fixtures.sh's own fixture list.
# The large per-cell tables are kept small: the ds_isrf of the 4096-cell Cartesian model and of the octree model
# gzipped (gzip -n: no name, no time stamp).
#   usage: make_aniso_fixtures.sh [model]      (no argument: every model)
#   LIST=1 make_aniso_fixtures.sh prints the fixture list ("ski seed tag lean" per line) and runs nothing
#   DEST=<dir> writes elsewhere than tests/golden/ref_aniso (the regeneration test compares the two)
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
export DEST=${DEST:-$HERE/ref_aniso}
MODELS="free_netzer free_surface free_sphebg free_cubbg free_patch free_laser netzer_torus_sph2 netzer_cone_cyl surface_shell_sph1 sphebg_plummer_cart cubbg_oct"
for m in ${1:-$MODELS}; do
  bash "$HERE/make_fixtures.sh" "$m" 4357 "${m}_s4357" 1
  [ -z "${LIST:-}" ] || continue
  case "$m" in sphebg_plummer_cart|cubbg_oct) gzip -n -9 -f "$DEST/${m}_s4357_ds_isrf.dat" ;; esac
done
