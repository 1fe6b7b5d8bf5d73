#!/bin/bash
# build_variant.sh NAME [extra hipcc flags...]: an experiment build of libpsk into tools/bin/ab_NAME/
# (objects in /tmp, the in-tree build untouched); CPU side only. Sources and flags are the Makefile's.
set -e
name=$1; shift
root="$(cd "$(dirname "$0")/.." && pwd)"
out="$root/tools/bin/ab_$name/libpsk.so"
make -C "$root/pysolvers_amd/csrc" BUILD="/tmp/bv_$name" OUT="$out" EXTRA="$*" -j16 "$out"
