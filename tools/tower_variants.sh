# Profiling builds of the tower -> tools/_var/libsde_<name>.so, each with every csrc/tower*.hip rebuilt with
# the compiler options given as NAME=OPTS arguments (e.g. split="-DSDE_SPLIT_ACT=1", read by tower.hip, or a
# generated probe header, read by tower_h16.hip:
# phase="-DSDE_H16_HEADER='\"$PWD/tools/_var/tower_h16_phase.h\"'", tools/variants/make_phase_header.py) and
# linked against the product build's other objects.  OPTS pass through the shell once more (eval), so that quotes
# inside them, as in the header path above, reach the compiler.  Earlier libraries and objects in tools/_var are
# removed, generated headers there are kept.  Every tower source of every variant compiles at once: give as many
# variants as the machine has cores / 7.
# Run here (CPU), then time on the GPU with tools/tower_variants.py.
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/_var; rm -f tools/_var/*.so tools/_var/*.o
C=scenedepthestimation_amd/csrc
O=scenedepthestimation_amd/_obj
for a in "$@"; do
  n=${a%%=*}; d=${a#*=}
  for s in $C/tower*.hip; do
    b=$(basename $s .hip)
    eval /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden \
      -Iinclude -I$C $d -c $s -o tools/_var/${b}__$n.o &
  done
done
wait
REST=""
for o in $O/*.o; do
  case "$(basename $o)" in tower*.o) ;; *) REST="$REST $o" ;; esac
done
for a in "$@"; do
  n=${a%%=*}
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/_var/libsde_$n.so tools/_var/tower*__$n.o $REST
  rm tools/_var/tower*__$n.o
done
ls tools/_var/*.so
