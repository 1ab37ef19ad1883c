# The instrumented library of tools/ws_phases.py (-DVQVS_TIMING) WITHOUT the no-scratch gate of csrc/Makefile: since round 6 the phase
# counters push one bf16 instantiation (<256, 128, resident>) over its register budget -- a spill there is harmless for this TOOL, which
# profiles the fp16 instantiations (none of which spills: the gate's report is printed).  The product build keeps the gate.
#   bash tools/build_timing_nogate.sh        -> vq_voice_swap_amd/libvqvs_timing.so
set -e
cd "$(dirname "$0")/../vq_voice_swap_amd/csrc"
B=build_timing; mkdir -p $B
FLAGS="-DVQVS_TIMING -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-unused-result"
SRCS=$(sed -n 's/^SRCS = //p' Makefile)  # the product's source list, so this one cannot fall behind it
[ -n "$SRCS" ] || { echo "no SRCS line in csrc/Makefile"; exit 1; }
for f in $SRCS; do
  [ $f = conv_ws.hip ] && continue  # (below, with its own flags)
  /opt/rocm/bin/hipcc $FLAGS -DVQVS_BUILD_ID=\"timing\" -x hip -c $f -o $B/$f.o &
done
/opt/rocm/bin/hipcc $FLAGS -fno-slp-vectorize -Rpass-analysis=kernel-resource-usage -x hip -c conv_ws.hip -o $B/conv_ws.hip.o 2> $B/conv_ws.resource.txt
wait
python3 ../../tools/check_no_scratch.py $B/conv_ws.resource.txt conv_ws_kernel || echo "(tool build: continuing)"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libvqvs_timing.so $B/*.o
ls -la ../libvqvs_timing.so
