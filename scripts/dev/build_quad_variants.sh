#!/bin/bash
# Builds libwdg_hip_<variant>.so under when-do-gnns-help_amd/lib/variants/ for the quad-row kernel's (threads, depth) variants:
# the shipped objects of every other file + spmm_quad.hip compiled with -DWDG_Q_FAST_THREADS / -DWDG_Q_DEPTH (+ $QUAD_EXTRA) on top
# of the Makefile's own flags for it (`make variant`).
# usage: scripts/dev/build_quad_variants.sh "1024 1" "768 2" ...   A/B: scripts/dev/ab_quad_variants.py
set -e
cd "$(dirname "$0")/../.."
make -s all
for v in "$@"; do
  set -- $v
  make -s variant UNIT=spmm_quad NAME=t$1d$2 VFLAGS="-DWDG_Q_FAST_THREADS=$1 -DWDG_Q_DEPTH=$2 $QUAD_EXTRA" &
done
wait
