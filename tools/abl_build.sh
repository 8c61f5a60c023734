#!/bin/bash
# Builds experiment variants of libsapca.so that differ only in compile-time switches of the quad format's builders
# (tiled_build.hip: -DSAPCA_QF_WGS=n) or of the format both they and the staged-entry sweep read through quad_format.h
# (spmm_tiled.hip too: -DSAPCA_QWAVES=8, -DSAPCA_EVEN_STEPS).  Both files are compiled with the switches given:
#   tools/abl_build.sh NAME "-DSAPCA_QF_WGS=2048 ..."   ->  single-algebra_amd/lib/exp/libsapca_NAME.so
# Run one with SAPCA_LIB_PATH=single-algebra_amd/lib/exp/libsapca_NAME.so python bench.py ...
set -e
cd "$(dirname "$0")/../single-algebra_amd"
name=$1; shift
mkdir -p build/exp lib/exp
for f in spmm_tiled tiled_build; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $@ -c csrc/$f.hip -o build/exp/${f}_$name.o
done
objs=$(ls build/*.o | grep -v -E "build/(spmm_tiled|tiled_build)\\.o")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o lib/exp/libsapca_$name.so $objs build/exp/spmm_tiled_$name.o build/exp/tiled_build_$name.o -ldl -Wl,-rpath,/opt/rocm/lib
echo built lib/exp/libsapca_$name.so
