#!/bin/bash
# build_worktree.sh WORKTREE OUTDIR: libpsk from another checkout, by that checkout's own Makefile (its
# sources, its flags); objects in /tmp where its Makefile has BUILD, else in its csrc/build
set -e
out="$(realpath -m "$2")/libpsk.so"
make -C "$1/pysolvers_amd/csrc" BUILD="/tmp/bwt_$(basename "$2")" OUT="$out" -j16 "$out"
