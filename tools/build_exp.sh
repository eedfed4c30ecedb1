#!/bin/bash
# Build a library with extra compiler flags ($2...) from the working copy into
# depth-map-fusion-utils_amd/build_exp/<name>/libdmf.so: the Makefile's own rules, flags and
# object list, every object rebuilt with the extra flags.  Run with DMF_LIB=<that path>.
#   tools/build_exp.sh stats -DDMF_EXP_STATS
set -e
NAME=$1; shift
OUT=build_exp/$NAME
make -s -j"${JOBS:-8}" -C "$(dirname "$0")/../depth-map-fusion-utils_amd" OUT="$OUT" EXTRA="$*" "$OUT/libdmf.so"
echo "$OUT/libdmf.so"
