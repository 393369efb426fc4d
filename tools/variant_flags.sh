#!/bin/bash
# like variant.sh, but the caller names ALL code-generation flags behind -O3 (variant.sh always adds the product's scheduler flag):
#   tools/variant_flags.sh NAME [flags...]  -> slow5tools_amd/_variants/libs5_NAME.so
cd "$(dirname "$0")/.." || exit 1
name=$1; shift
V=slow5tools_amd/_variants
mkdir -p $V
C=slow5tools_amd/csrc
objs=
for u in encode_kernels decode_kernels batch_kernels order_launch; do   # the flags reach all four units of the press path
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC "$@" -c $C/$u.hip -o $V/${u}_$name.o || exit 1
    objs="$objs $V/${u}_$name.o"
done
hipcc --offload-arch=gfx950 -shared -fPIC -o $V/libs5_$name.so $objs $C/host_api.o $C/ascii_kernels.o $C/ascii_api.o $C/slow5_compat.o $C/blow5_file.o && ls -la $V/libs5_$name.so
rm -f $objs
