# tools/_var/libsde_NAME.so: the library with one source file rebuilt with extra flags (A/B timing).
# usage: bash tools/build_file_variant.sh FILE.hip NAME [hipcc flags...]
#        SRC=path/to/other.hip bash tools/build_file_variant.sh FILE.hip NAME ...  (FILE.hip replaced by SRC)
# The tower is one file per kernel family: tower_h16.hip takes -DSDE_H16_HEADER=... (a probe copy of tower_h16.h),
# tower_h16s.hip -DSDE_H16S_HEADER=... (tower_h16.h + tower_h16s.h, tools/variants/make_phase_header.py),
# tower.hip -DSDE_SPLIT_ACT=1; tower_x6p.hip, tower_wino.hip and tower_fp32.hip hold the other families.
# An SGM variant rebuilds sgm.hip (it includes sgm_scan.h, sgm_faithful.h and sgm_wave.h): ... sgm.hip sgm_NAME;
# the post-processing kernels are postprocess.hip.
# The cost volume is one file per concern: a cvlr3_kernel variant (cv_lr.h) rebuilds cv_volume.hip; a fix-up, tile-path
# (cv_tile.h) or chunk-merge variant rebuilds cv_wta.hip; the exact kernels (cv_exact.h) are in both objects: rebuild
# the one whose entry point is timed; the row sweep is cv_row.hip (its two extra flags are added below); sde_wta's
# kernels are wta.hip.
set -e
cd "$(dirname "$0")/.."
F=$1; NAME=$2; shift 2
C=scenedepthestimation_amd/csrc
O=scenedepthestimation_amd/_obj
mkdir -p tools/_var
EXTRA=""
[ "$F" = "cv_row.hip" ] && EXTRA="-fno-honor-nans -mno-amdgpu-ieee"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden \
  -Wno-unused-function -Iinclude -I$C $EXTRA "$@" -c ${SRC:-$C/$F} -o tools/_var/v_$NAME.o
OBJS=""
for o in $O/*.o; do
  [ "$(basename $o)" = "${F%.hip}.o" ] || OBJS="$OBJS $o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/_var/libsde_$NAME.so tools/_var/v_$NAME.o $OBJS
rm tools/_var/v_$NAME.o
