#!/bin/bash
# A/B build of ONE OR MORE csrc units with extra -D flags, linked against the main build's other
# objects:  scripts/ab_build_one.sh <name> <unit.hip | 'glob'>... -DFOO=1 ...  -> _lib_ab/<name>/libgpk.so
# For a switch that only those units read, e.g. GPK_ADJR_* (gpk_var_reg.hip), GPK_VAR_SKIP
# (gpk_var_tiled.hip), or a gpk_exact_dev.h switch of the exact forward, whose units are
# 'gpk_exact_nb*.hip' (quote the glob; with -DGPK_EXACT_DEV=1 only N = 128 / 256 are compiled).
# A switch from gpk_var_common.h (GPK_VAR_LREG, GPK_VAR_REG, GPK_KGRAM_SPL, GPK_FWD_OCC,
# GPK_ADJ_LDS_WAIT) is read by every variational unit: python build_native.py -DFOO=1 --out-dir <dir>.
set -e
R=$(cd "$(dirname "$0")/.." && pwd); P=$R/fine_grained_gaussian_process_forcasting_amd
name=$1; shift
out=$P/_lib_ab/$name; mkdir -p $out
srcs=; defs=
for a in "$@"; do case $a in -*) defs="$defs $a";; *) srcs="$srcs $(cd $P/csrc && ls $a)";; esac; done
own=; skip=; pids=
for src in $srcs; do
  rm -f $out/$src.o
  /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -munsafe-fp-atomics $defs -I $R/include -c $P/csrc/$src -o $out/$src.o &
  pids="$pids $!"; own="$own $out/$src.o"; skip="$skip -e /$src.o"
done
for p in $pids; do wait $p; done   # (set -e: a failed compile ends the script here)
objs=$(ls $P/_lib/*.o | grep -v $skip)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs $own -o $out/libgpk.so
echo $out/libgpk.so
