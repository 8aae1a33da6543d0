# usage: scripts/build_variant.sh NAME "-DFLAGS" [SOURCE.hip ...]  -> radfoam_amd/libradfoam_hip_NAME.so
# Compiles the named sources of radfoam_amd/csrc (default: rf_kernels.hip) with build.py's flags plus FLAGS and links
# them with the objects build.py made of every other source (radfoam_amd/csrc/_obj: run radfoam_amd/build.py first),
# so that a variant carries the whole C-ABI and _lib.load() binds it.
set -e
cd "$(dirname "$0")/.."
NAME=$1
FLAGS=$2
shift 2 || true
VARIED="${*:-rf_kernels.hip}"
OUT=radfoam_amd/libradfoam_hip_$NAME.so
OBJ=radfoam_amd/csrc/_obj
VDIR=$OBJ/variant_$NAME
mkdir -p $VDIR
OBJS=""
for o in $OBJ/*.o; do
  b=$(basename $o .o)
  case " $VARIED " in *" $b.hip "*) ;; *) OBJS="$OBJS $o";; esac
done
for s in $VARIED; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-result $FLAGS \
    -c radfoam_amd/csrc/$s -o $VDIR/$(basename $s .hip).o
  OBJS="$OBJS $VDIR/$(basename $s .hip).o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT $OBJS
echo built $OUT
