#!/bin/bash
# Builds when-do-gnns-help_amd/lib/variants/libwdg_hip_kr_<name>.so: the shipped objects of every other file + kernel_reg.hip (the
# solver) compiled with extra flags on top of the Makefile's own for it (e.g. -DK2_PROFILE: one workgroup prints its shader clocks
# per phase).  usage: build_kr_variant.sh <name> "<flags>"
set -e
cd "$(dirname "$0")/../.."
make -s variant UNIT=kernel_reg NAME=kr_$1 VFLAGS="$2"
