#!/bin/bash
# Build a variant of the library with extra compile flags into abv/lib<name>.so
# (timing experiments, A/B runs through LATTICEUM_AMD_LIB): tools/build_variant.sh name -DFLAG ...
# The sources and the per-file flags are the Makefile's.
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$ROOT/abv"
make -s -j16 -C "$ROOT/latticeum_amd/csrc" BUILD="/tmp/lf_variant_$NAME" OUT="$ROOT/abv/lib$NAME.so" EXTRA_FLAGS="$*"
echo "abv/lib$NAME.so"
