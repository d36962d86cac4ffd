#!/bin/bash
# Diagnostic tracker build: the tracker units that hold the RANSAC stamps (TRK_STAMPS) or the GFTT selection
# breakdown (GFTT_DEBUG) recompiled with those defines, linked with the other objects of the in-tree build into
# tools/probe/libvio360_dbg.so
# (use: VIO360_LIB=tools/probe/libvio360_dbg.so python3 tools/trk_time.py 5).  Built here, on the CPU.
set -e
root=$(cd "$(dirname "$0")/../.." && pwd)
cd "$root/360_visual_inertial_odometry_amd/csrc"
make -s
mkdir -p /tmp/trkdbg
objs=$(ls build/*.o)
for src in $(grep -lE 'TRK_STAMPS|GFTT_DEBUG' trk_*.hip); do
  unit=${src%.hip}
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I../../include -I. -ffp-contract=off \
    -DTRK_STAMPS -DGFTT_DEBUG -w -c "$src" -o "/tmp/trkdbg/$unit.o"
  objs=$(echo "$objs" | sed "s|^build/$unit\.o\$|/tmp/trkdbg/$unit.o|")
  echo "recompiled $src"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o "$root/tools/probe/libvio360_dbg.so" $objs
echo "built $root/tools/probe/libvio360_dbg.so"
