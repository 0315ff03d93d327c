#!/bin/bash
# build a variant of liblde.so that differs in lde_pendulum.o only:  abl/variant_lib.sh <tag> "<extra hipcc flags>"  →  abl/liblde_<tag>.so
# (run the bench against it with LDE_LIB_PATH=abl/liblde_<tag>.so; abl/*.so are git-ignored). Every other object comes from the product
# build's _obj/ (run build_lib() first). LDE_VARIANT_CSRC=<dir> compiles lde_pendulum.hip from another source tree (an older commit's
# csrc/, with that commit's include/ two levels above it).
set -e
cd "$(dirname "$0")/../latentdiffeq.jl_amd"
tag=$1; shift
csrc=${LDE_VARIANT_CSRC:-csrc}
mkdir -p /tmp/lde_var_$tag
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $@ -c $csrc/lde_pendulum.hip -o /tmp/lde_var_$tag/lde_pendulum.o
others=$(ls _obj/*.o | grep -v '/lde_pendulum\.o$')
hipcc --offload-arch=gfx950 -shared -fPIC -o ../abl/liblde_$tag.so /tmp/lde_var_$tag/lde_pendulum.o $others -ldl
echo built abl/liblde_$tag.so
