#!/bin/bash
# Build a variant of the engine library with extra compiler flags (timing-only experiments, A/B candidates):
#   tools/build_variant.sh NAME [-DFLAG ...]   ->  chimeralm_amd/csrc/libclm_NAME.so   (run with CLM_LIB=<that path>, tools/ab.sh)
set -e
R=$(cd "$(dirname "$0")/.." && pwd); C=$R/chimeralm_amd/csrc; name=$1; shift
T=$(mktemp -d)
# (the product's own source list: chimeralm_amd/build.py SOURCES)
srcs=$(cd $R && python3 -c "from chimeralm_amd.build import SOURCES; print(' '.join(SOURCES))")
for s in $srcs; do
  arch="--offload-arch=gfx950 -Wno-pass-failed"; [ "${s##*.}" = cpp ] && arch=""
  hipcc $arch -O3 -std=c++17 -fPIC -ffp-contract=fast -Wno-unused-function "$@" -I$R/include -I$C -c $C/$s -o $T/${s%.*}.o &
done
wait
hipcc --offload-arch=gfx950 -shared -fPIC -o $C/libclm_$name.so $T/*.o -lz -lpthread
rm -rf $T
echo $C/libclm_$name.so
