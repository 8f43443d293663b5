#!/bin/bash
# Generates the golden reference outputs of the particle-dust models (SPHDustDistribution; the particle files are
# tests/golden/particles/*.dat, written by make_particles.py there) under tests/golden/ref_particles/: the reference
# SKIRT v7.3 built by oracle/ref.mk, `skirt -t 1 -b -i tests/golden/particles`, seed 4357. A script of its own beside
# make_fixtures.sh, which knows no input folder. Lean outputs: the SEDs, ds_convergence, ds_cellprops, ds_isrf and a
# log excerpt (particle, node and leaf counts). The per-cell tables (ds_cellprops, ds_isrf) are gzipped (gzip -n: no
# name, no time stamp), so every file stays under 256 KiB.
#   usage: make_particle_fixtures.sh [model]      (no argument: every model)
#   LIST=1 make_particle_fixtures.sh prints the fixture list ("ski seed tag lean" per line) and runs nothing
#   DEST=<dir> writes elsewhere than tests/golden/ref_particles (the regeneration test compares the two)
#   SKIRT_REF_BIN=<path> uses that binary and builds nothing
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
REPO=$(cd "$HERE/../.." && pwd)
BIN=${SKIRT_REF_BIN:-$REPO/oracle/_ref/skirt}
MODELS="part_oct part_oct_neg part_oct_bary part_cart part_vor part_vor_dd part_few"
if [ -n "${LIST:-}" ]; then
  for m in ${1:-$MODELS}; do echo "$m 4357 ${m}_s4357 1"; done
  exit 0
fi
[ -n "${SKIRT_REF_BIN:-}" ] || make -s -C "$REPO" -f oracle/ref.mk -j"${JOBS:-8}" >&2
DEST=${DEST:-$HERE/ref_particles}
WORK=$(mktemp -d)
mkdir -p "$DEST"
for m in ${1:-$MODELS}; do
  tag=${m}_s4357
  sed 's/seed="[0-9]*"/seed="4357"/' "$HERE/ski/$m.ski" > "$WORK/$tag.ski"
  (cd "$WORK" && "$BIN" -t 1 -b -i "$HERE/particles" -o "$WORK" "$WORK/$tag.ski" > "$WORK/$tag.console" 2>&1)
  for f in "$WORK/$tag"_*_sed.dat "$WORK/$tag"_ds_convergence.dat "$WORK/$tag"_ds_cellprops.dat "$WORK/$tag"_ds_isrf.dat; do
    [ -f "$f" ] || continue  # (a Pan model without dust emission writes no ds_isrf)
    cp "$f" "$DEST/"
    g="$DEST/$(basename "$f")"
    case "$g" in *_ds_cellprops.dat|*_ds_isrf.dat) gzip -n -9 -f "$g" ;; esac
  done
  grep -h "Number of high-temperature\|Number of SPH gas\|number of particles per cell\|Total number of\|Computed Voronoi\|neighbors per cell" \
    "$WORK/$tag"_log.txt | sed 's/^[^ ]* [^ ]* *//' > "$DEST/${tag}_log_excerpt.txt" || true
done
rm -rf "$WORK"
