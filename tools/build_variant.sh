#!/bin/bash
# build a tuning variant of the engine: tools/build_variant.sh TAG [extra hipcc flags...]
# -> skirt_amd/libskirt_amd_TAG.so (select with SKIRT_AMD_LIB=libskirt_amd_TAG.so)
# The -D flags among the extra ones go to the engine's host sources too: they size LDS and pack the Voronoi
# slots with the same constants (SKIRT_LABS_BUF, SKIRT_VOR_GROUPS in device/engine_args.hpp).
set -e
tag=$1; shift
cd "$(dirname "$0")/../skirt_amd/csrc"
HOST="build/xml.o build/units.o build/build.o build/outputs.o build/dustemission.o build/voronoi.o build/sim.o build/rccl_reducer.o build/describe.o build/voronoi_cells.o"
make -s $HOST
defs=()
for f in "$@"; do case "$f" in -D*) defs+=("$f") ;; esac; done
ENGINE_HOST=""
for s in engine_layout engine_setup engine_phase; do
    ${CXX:-g++} -O2 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
        "${defs[@]}" -c -o build/${s}_$tag.o host/$s.cpp
    ENGINE_HOST="$ENGINE_HOST build/${s}_$tag.o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -ffp-contract=off -mllvm -disable-machine-licm "$@" \
    -c -o build/engine_$tag.o ${SRC:-device/engine.hip}
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libskirt_amd_$tag.so build/engine_$tag.o \
    $ENGINE_HOST $HOST -L/opt/rocm/lib -lrccl -ldl -lpthread
