#!/bin/bash
# build an experimental variant of the library: tools/variant.sh NAME -DFLAG...   -> slow5tools_amd/_variants/libs5_NAME.so
# (git-ignored; use with S5GPU_LIB=... python tools/stage_time.py).  Never part of the product build.
cd "$(dirname "$0")/.." || exit 1
name=$1; shift
V=slow5tools_amd/_variants
mkdir -p $V
C=slow5tools_amd/csrc
objs=
for u in encode_kernels decode_kernels batch_kernels order_launch; do   # the -D flags reach all four units of the press path
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-sched-strategy=max-memory-clause "$@" -c $C/$u.hip -o $V/${u}_$name.o || exit 1
    objs="$objs $V/${u}_$name.o"
done
hipcc --offload-arch=gfx950 -shared -fPIC -o $V/libs5_$name.so $objs $C/host_api.o $C/ascii_kernels.o $C/ascii_api.o $C/slow5_compat.o $C/blow5_file.o && ls -la $V/libs5_$name.so
