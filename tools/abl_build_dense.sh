#!/bin/bash
# like abl_build.sh, for one of the dense panel units (gram, chol, panel_gemm, sym_eig, panel_ops):
#   tools/abl_build_dense.sh UNIT NAME "-DFLAG=1"
set -e
cd "$(dirname "$0")/../single-algebra_amd"
unit=$1; name=$2; shift 2
mkdir -p build/exp lib/exp
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $@ -c csrc/$unit.hip -o build/exp/${unit}_$name.o
objs=$(ls build/*.o | grep -v "build/$unit.o")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o lib/exp/libsapca_$name.so $objs build/exp/${unit}_$name.o -ldl -Wl,-rpath,/opt/rocm/lib
echo built lib/exp/libsapca_$name.so
