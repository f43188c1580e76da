#!/bin/bash
# Build an alternate libtapeec (varlib/lib_<name>.so) whose decode class kernels are generated with
# build-time options (dec_class.hpp DecClassGenOpt), for A/B timing through TAPE_EC_LIB.
#   bash scripts/build_class_var.sh late "TEC_GEN_LATE=1"     (needs tape_amd/build/*.o)
set -e
cd "$(dirname "$0")/.."
name=$1; envs=$2
d=/tmp/varlib_gen_$name
mkdir -p $d
env $envs tape_amd/build/gen_dec_class $d
# as tape_amd/Makefile: the node-recover classes (8..23) are built without the ranged-read window
for f in $d/dec_class_[0-9]*.hip; do
  id=${f##*dec_class_}; id=${id%.hip}
  [ "$id" -ge 8 ] && echo "$f -DTEC_DCLS_WINDOW=0" || echo "$f -DTEC_DCLS_WINDOW=1"
done | xargs -P 8 -L 1 sh -c '/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++20 -fPIC -Wno-unused-variable -Itape_amd/csrc $1 -c -o $0.o $0'
objs=$(ls tape_amd/build/*.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o varlib/lib_$name.so $objs $d/*.hip.o -L/opt/rocm/lib -lhiprtc
echo built varlib/lib_$name.so
