#!/bin/bash
# Build a variant of libmadipm_hip.so with extra compile definitions for the ldl*.hip units (A/B
# measurements; MADIPM_FOLD_GP, PUSH_NC2, PUSH_NC3 and SYRK_WAVES are read by ldl.hip):
#   bash tools/build_variant.sh TAG -DMADIPM_FOLD_GP=32 ...
# -> madipm.jl_amd/madipm_amd/lib/variants/libmadipm_hip_TAG.so (select with MADIPM_LIB=<path>)
set -e
TAG=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CS=$ROOT/madipm.jl_amd/csrc
OBJ=$ROOT/build/obj
OUT=$ROOT/madipm.jl_amd/madipm_amd/lib/variants
mkdir -p $OUT $OBJ/variants
make -s -C $CS >/dev/null
OBJS=$(ls $OBJ/*.o)
for SRC in $CS/ldl*.hip; do  # every LDL^T unit: the variant's object in place of the default one
  U=$(basename $SRC .hip)
  /opt/rocm/bin/hipcc -O3 -fPIC -std=c++17 -Wall -Wno-unused-function -I$ROOT/include --offload-arch=gfx950 \
    -munsafe-fp-atomics "$@" -c $SRC -o $OBJ/variants/${U}_$TAG.o
  OBJS=$(echo "$OBJS" | grep -v "/$U.hip.o$"; echo $OBJ/variants/${U}_$TAG.o)
done
/opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o $OUT/libmadipm_hip_$TAG.so $OBJS \
  -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
echo $OUT/libmadipm_hip_$TAG.so
