#!/usr/bin/env bash
# Build libake_hip.so for gfx950 in-tree (the .so travels to the GPU box with the snapshot).
set -euo pipefail
cd "$(dirname "$0")"
OUT=../libake_hip.so
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result"
BUILD=build
mkdir -p $BUILD
HEADERS="common.h bf16_split.h philox.h keys.h cqt_stream.h profile.h changes.h pcnet_kernels.h pcnet_bwd_kernels.h pcnet_net.h pcnet_plan.h pcnet_forward.h pcnet_backward.h ../../include/ake_hip.h"
pids=()
for f in common.cpp cqt.hip pcnet.hip pipeline.hip optim.hip audio.hip loss.hip track.hip smooth.hip synth.hip tuning.hip profile.hip profile_tuned.hip stream.hip stream_profile.hip changes.hip stream_changes.hip; do
  obj=$BUILD/${f%.*}.o
  stale=0
  [ -f "$obj" ] || stale=1
  for d in "$f" $HEADERS; do [ "$d" -nt "$obj" ] && stale=1; done
  if [ $stale = 1 ]; then
    extra=""
    # cqt.hip: the SLP vectoriser turns the FIR taps into v_pk_* math fed by ds_read2_b32 gathers (4-way LDS bank
    # conflicts, measured: half of all LDS cycles); plain ds_read_b128 + scalar FMAs are faster
    [ "$f" = cqt.hip ] && extra="-fno-slp-vectorize"
    ( $HIPCC $FLAGS $extra -x hip -c "$f" -o "$obj" ) &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC $BUILD/common.o $BUILD/cqt.o $BUILD/pcnet.o $BUILD/pipeline.o $BUILD/optim.o $BUILD/audio.o $BUILD/loss.o $BUILD/track.o $BUILD/smooth.o $BUILD/synth.o $BUILD/tuning.o $BUILD/profile.o $BUILD/profile_tuned.o $BUILD/stream.o $BUILD/stream_profile.o $BUILD/changes.o $BUILD/stream_changes.o -o $OUT
echo "built $(realpath $OUT)"
