# Build a variant of the library for same-box A/B measurements: tools/build_variant.sh <name> <extra hipcc flags...>
# -> gpurun_variants/libkzg_<name>.so (travels with the gpurun snapshot; select it with KZG_LIB_PATH)
# The units are the Makefile's SRCS.  CSRC=<dir> builds another tree's sources (a worktree of the parent commit: the other side of an A/B
# of a source change).
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=${CSRC:-$ROOT/rust-kzg-bn254_amd/csrc}
NAME=$1; shift
B=/tmp/kzg_variant_$NAME; mkdir -p $B $ROOT/gpurun_variants
for f in $(sed -n 's/^SRCS *= *//p' $CSRC/Makefile); do
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function "$@" -c $CSRC/$f -o $B/${f%.hip}.o &
done
wait
hipcc --offload-arch=gfx950 -shared -fPIC -o $ROOT/gpurun_variants/libkzg_$NAME.so $B/*.o
ls -la $ROOT/gpurun_variants/libkzg_$NAME.so
