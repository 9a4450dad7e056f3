#!/bin/bash
# Build an A/B variant of libhdpgpc_hip.so:  tools/build_variant.sh NAME -DFLAG...  ->  hdpgpc_amd/lib/ab/libhgp_NAME.so
# (hdpgpc_amd/lib/ab/ travels to the GPU box, build/ does not; both are git-ignored)
set -e
name=$1; shift
od=build/probe/obj_$name
mkdir -p $od hdpgpc_amd/lib/ab
FLAGS="-O3 --offload-arch=gfx950 -mllvm -pragma-unroll-threshold=1048576 -fPIC -Wno-unused-result"
for src in hdpgpc_amd/csrc/*.hip; do   # the Makefile's SRCS
  /opt/rocm/bin/hipcc $FLAGS "$@" -c -o $od/$(basename $src .hip).o $src &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o hdpgpc_amd/lib/ab/libhgp_$name.so $od/*.o
echo built hdpgpc_amd/lib/ab/libhgp_$name.so
