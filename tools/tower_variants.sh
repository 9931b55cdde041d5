# Profiling builds of the persistent tower kernel -> tools/_var/libsde_t<name>.so, each built with
# the compiler options given as NAME=OPTS arguments (e.g. split="-DSDE_SPLIT_ACT=1", or a generated probe header:
# phase="-DSDE_H16_HEADER='\"$PWD/tools/_var/tower_h16_phase.h\"'", tools/variants/make_phase_header.py).
# Run here (CPU), then time on the GPU with tools/tower_variants.py.
set -e
cd "$(dirname "$0")/.."
rm -rf tools/_var; mkdir -p tools/_var
O=scenedepthestimation_amd/_obj
for a in "$@"; do
  n=${a%%=*}; d=${a#*=}
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden \
    -Iinclude -Iscenedepthestimation_amd/csrc $d -c scenedepthestimation_amd/csrc/tower.hip \
    -o tools/_var/tower_$n.o &
done
wait
for a in "$@"; do
  n=${a%%=*}
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/_var/libsde_$n.so tools/_var/tower_$n.o \
    $O/cbca.o $O/cv_row.o $O/sgm.o $O/cost_volume.o
  rm tools/_var/tower_$n.o
done
ls tools/_var/*.so
