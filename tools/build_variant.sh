#!/bin/bash
# Build a variant of libsacx for A/B runs (SACX_LIBPATH=<out>), from the Makefile's own object list and flags:
#   tools/build_variant.sh <name> ["<-DSACX_...=... flags>"] [<source tree>]  -> tools/libvar/libsacx_<name>.so
# <source tree>: another checkout's root (the parent commit's, `git worktree add`), default this one.
set -eu
cd "$(dirname "$0")/.."
name=$1; flags=${2:-}; src=${3:-.}
out=$PWD/tools/libvar
csrc=$src/sac-expert_amd/csrc
mkdir -p "$out"
# the Makefile's FLAGS, so a command-line FLAGS (which replaces the Makefile's) only adds to them
base=$(make -s -C "$csrc" --eval 'print-flags: ; @echo $(FLAGS)' print-flags)
make -s -C "$csrc" -j"${MAX_JOBS:-4}" OUT="$out/libsacx_$name.so" OBJ="$out/obj_$name" FLAGS="$base $flags"
rm -rf "$out/obj_$name"
echo "tools/libvar/libsacx_$name.so"
