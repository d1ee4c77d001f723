#!/bin/bash
# A/B build of ONE csrc file with extra -D flags, linked against the main build's other
# objects:  scripts/ab_build_one.sh <name> <file.hip> -DFOO=1 ...  -> _lib_ab/<name>/libgpk.so
# Only for a switch that ONE unit reads (e.g. GPK_ADJR_* in gpk_var_reg.hip, GPK_VAR_SKIP in
# gpk_var_tiled.hip). The variational path is several units: a switch from gpk_var_common.h
# (GPK_VAR_LREG, GPK_VAR_REG, GPK_KGRAM_SPL, GPK_FWD_OCC, GPK_ADJ_LDS_WAIT) needs
# python build_native.py -DFOO=1 --out-dir <dir>.
set -e
R=$(cd "$(dirname "$0")/.." && pwd); P=$R/fine_grained_gaussian_process_forcasting_amd
name=$1; src=$2; shift 2
out=$P/_lib_ab/$name; mkdir -p $out
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -munsafe-fp-atomics "$@" -I $R/include -c $P/csrc/$src -o $out/$src.o
objs=$(ls $P/_lib/*.o | grep -v "/$src.o")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs $out/$src.o -o $out/libgpk.so
echo $out/libgpk.so
